// The last step of the stages that select rows of a stored cloud (outlier.hip, iss.hip, cluster.hip, plane.hip, boundary.hip): 0 / 1 flags over
// the original index -> the flagged rows as xyz / nrm / idx (and their labels) in ascending original index, in the stage's RowSelection
// (common.h).  row_select.hip holds the kernels and the host half; the stages keep only what writes their flags.
#pragma once
#include <functional>

#include "common.h"

namespace mvicp {

// Selects rows of f (valid, uploaded; sel reserved for f.n rows by the stage call, so nothing is allocated here) into sel:
//   flags     sel.flag[i] = (flags[i] == want), or, flags == null, what the stage has already written into sel.flag on the context's stream --
//             or writes now through write_flags (launches on the stream given, inside the profile scope)
//   select    exclusive scan of sel.flag (rocprim) -> one lane per point stores its row at its rank (compact_rows_kernel) -> the number
//             kept through the pinned word -> ONE wait -> 0 <= kept <= n, else MVICP_ERR_INTERNAL naming `stage`
// label (n ints or null) travels with the row into sel.klabel.  The selection carries normals iff f has stored normals now.  The launches
// run under the profile scope `scope` with the byte model bytes_per_row x n.  Returns the rows kept or a negative status (no selection then).
long long select_rows(mvicp_ctx* c, RowSelection& sel, const FrameDev& f, const char* stage, const char* scope, double bytes_per_row, const unsigned char* flags,
                      int want, const int* label = nullptr, const std::function<void(hipStream_t, int*)>& write_flags = nullptr);

}  // namespace mvicp
