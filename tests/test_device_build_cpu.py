"""The device-cloud upload without a GPU: the header declares and the library exports the two new entries, and the tensor checks of
Engine.set_frame_device reject what the C entry cannot take before any library call."""
import os
import re

import pytest

from mvicp import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mvicp_set_frame_device", "mvicp_get_structure")


def test_header_declares_and_library_exports_the_device_build(engine_lib):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mvicp.h")).read(), flags=re.S)
    assert re.search(r"int\s+mvicp_set_frame_device\s*\(\s*mvicp_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)", txt)
    assert re.search(r"long\s+long\s+mvicp_get_structure\s*\(\s*mvicp_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*,\s*const\s+char\s*\*\s*\w+\s*,\s*void\s*\*\s*\w+\s*,\s*long\s+long\s+\w+\s*\)", txt)
    for s in NEW:
        assert hasattr(engine_lib, s), s
        assert s in L.SYMBOLS
    assert "scalars" in L.STRUCTURE_NAMES and len(L.STRUCTURE_NAMES) == 16


def test_tensor_checks_without_a_gpu():
    torch = pytest.importorskip("torch")
    good = torch.zeros((10, 3), dtype=torch.float64)
    with pytest.raises(TypeError):
        L.check_device_cloud(good, 0)                                   # a CPU tensor
    with pytest.raises(TypeError):
        L.check_device_cloud(good.float(), 0)                           # float32
    with pytest.raises(TypeError):
        L.check_device_cloud(good.numpy(), 0)                           # not a tensor
    with pytest.raises(ValueError):
        L.check_device_cloud(torch.zeros((3, 10), dtype=torch.float64).t(), 0)   # non-contiguous (10, 3)
    for shape in ((10,), (10, 4), (2, 5, 3)):
        with pytest.raises(ValueError):
            L.check_device_cloud(torch.zeros(shape, dtype=torch.float64), 0)
    with pytest.raises(ValueError):
        L.check_device_cloud(good, 0, n=11, name="nor")                 # normals of another length
