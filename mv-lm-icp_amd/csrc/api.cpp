// C-ABI of libmvicp_hip.so (include/mvicp.h): context, uploads, the correspondence pipeline
// (S1: NN -> cutoff/compaction -> median), per-edge normal equations, profiling.
// The LM solve (S2) lives in host/lm.cpp; the RCCL glue in comm.cpp.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <limits>
#include <mutex>
#include <new>
#include <thread>

#include "common.h"
#include "comm.h"
#include "nn_tie.h"
#include "lin_table.h"
#include "../host/se3.h"

namespace mvicp {

static thread_local char g_err[1024] = "";

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int abi_exception() noexcept {
  try { throw; }
  catch (const std::bad_alloc&) { set_error("out of host memory"); }
  catch (const std::exception& e) { set_error("internal error: %s", e.what()); }
  catch (...) { set_error("internal error (unknown exception)"); }
  return MVICP_ERR_INTERNAL;
}

// squared search radius of the NN kernels for a cutoff whose squared bound is d2_bound (ctx::nn_search_factor)
double search_bound(const mvicp_ctx* c, double d2_bound) {
  if (!(c->nn_search_factor > 0.0)) return 1.7976931348623157e308;
  const double f = std::max(1.0, c->nn_search_factor);
  const double b = d2_bound * f * f * (1.0 + 1e-9);
  return std::isfinite(b) ? b : 1.7976931348623157e308;
}

int cached_upload(mvicp_ctx* c, const char* key, const void* src, size_t bytes, void** dptr) {
  mvicp_ctx::CachedTable& t = c->tables[key];
  if (t.d && t.bytes.size() == bytes && std::memcmp(t.bytes.data(), src, bytes) == 0) { *dptr = t.d; return MVICP_OK; }
  MV_HIP(hipStreamSynchronize(c->stream));  // earlier kernels may still read the old copy
  if (bytes > t.cap) {
    if (t.d) MV_HIP(hipFree(t.d));
    t.d = nullptr;
    MV_HIP(hipMalloc(&t.d, std::max<size_t>(bytes, 256)));
    t.cap = std::max<size_t>(bytes, 256);
  }
  MV_HIP(hipMemcpy(t.d, src, bytes, hipMemcpyHostToDevice));
  t.bytes.assign((const char*)src, (const char*)src + bytes);
  *dptr = t.d;
  return MVICP_OK;
}

void scratch_reset(mvicp_ctx* c) { c->scratch_used = 0; }

int scratch_upload(mvicp_ctx* c, const void* src, size_t bytes, void** dptr) {
  const size_t aligned = (bytes + 255) & ~(size_t)255;
  if (c->scratch_used + aligned > c->scratch_bytes) {
    // grow: wait for in-flight users, then reallocate (callers re-upload everything after a reset)
    if (c->scratch_used != 0) { set_error("scratch overflow (%zu + %zu > %zu)", c->scratch_used, aligned, c->scratch_bytes); return MVICP_ERR_STATE; }
    MV_HIP(hipStreamSynchronize(c->stream));
    if (c->d_scratch) MV_HIP(hipFree(c->d_scratch));
    c->scratch_bytes = std::max<size_t>(aligned * 4, 1 << 20);
    MV_HIP(hipMalloc((void**)&c->d_scratch, c->scratch_bytes));
  }
  void* d = c->d_scratch + c->scratch_used;
  // stream-ordered w.r.t. earlier kernels that may still read the scratch, then synchronous for the host source
  MV_HIP(hipMemcpyAsync(d, src, bytes, hipMemcpyHostToDevice, c->stream));
  MV_HIP(hipStreamSynchronize(c->stream));
  c->scratch_used += aligned;
  *dptr = d;
  return MVICP_OK;
}

ProfScope::ProfScope(mvicp_ctx* ctx, const char* nm, double bytes) : c(ctx), name(nm), on(ctx->profile) {
  // level 2: only the two roofline scopes (every event pair is two extra queue packets between kernels)
  if (on && ctx->profile_level >= 2 && ((std::strncmp(nm, "nn_", 3) != 0 && std::strncmp(nm, "linearize", 9) != 0 && std::strcmp(nm, "comm") != 0) ||
                                        std::strcmp(nm, "nn_tie") == 0)) on = false;   // (the tie fix-up is a few microseconds per moving round: not worth two packets)
  if (!on) return;
  ProfEntry& pe = c->prof[name];
  auto get = [&]() {
    hipEvent_t ev = nullptr;
    if (!pe.pool.empty()) { ev = pe.pool.back(); pe.pool.pop_back(); }
    else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr;
    return ev;
  };
  a = get(); b = get();
  pe.bytes += bytes;
  if (std::strncmp(nm, "nn_", 3) == 0) { pe.survey_bytes += bytes; pe.queries += bytes / 36.0; }   // NN scopes open with 36 B per query (24 B read + 12 B result)
  pe.launches += 1;
  if (a) (void)hipEventRecord(a, c->stream);
}
ProfScope::~ProfScope() {
  if (!on) return;
  if (b) (void)hipEventRecord(b, c->stream);
  if (a && b) c->prof[name].pending.push_back(std::make_pair(a, b));
}
static double now_ms() {
  timespec ts;
  clock_gettime(CLOCK_MONOTONIC, &ts);
  return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
HostScope::HostScope(mvicp_ctx* ctx, const char* nm) : c(ctx), name(nm), t0(0.0), on(ctx->profile) { if (on) t0 = now_ms(); }
HostScope::~HostScope() {
  if (!on) return;
  ProfEntry& pe = c->prof[name];
  pe.ms += now_ms() - t0;
  pe.launches += 1;
}
// The hot calls (mvicp_correspond / mvicp_optimize / mvicp_linearize) only collect once a scope holds more than 256 unresolved event pairs: resolving
// them costs a hipEventSynchronize + hipEventElapsedTime per pair — 10-30 us of host time per ICP round with four scopes live, INSIDE the timed
// region of a bench run that needs the scopes for its roofline (5 % of a cfg4 fixed-point round, 15 % of a shard8 one).  The readers
// (mvicp_profile_get / _reset) always collect everything.
void prof_collect_lazy(mvicp_ctx* c) {
  for (auto& kv : c->prof) if (kv.second.pending.size() > 256) { prof_collect(c); return; }
}
void prof_collect(mvicp_ctx* c) {
  for (auto& kv : c->prof) {
    ProfEntry& pe = kv.second;
    for (auto& pr : pe.pending) {
      float ms = 0.f;
      if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) pe.ms += ms;
      pe.pool.push_back(pr.first);
      pe.pool.push_back(pr.second);
    }
    pe.pending.clear();
  }
}

namespace {

template <typename T> int dev_alloc(T** p, size_t n) {
  *p = nullptr;
  if (n == 0) n = 1;
  MV_HIP(hipMalloc((void**)p, sizeof(T) * n));
  return MVICP_OK;
}
template <typename T> void dev_free(T*& p) {
  if (p) (void)hipFree(p);
  p = nullptr;
}

void free_graph(mvicp_ctx* c) {
  dev_free(c->d_esrc); dev_free(c->d_edst); dev_free(c->d_cap_off); dev_free(c->d_count);
  dev_free(c->d_ctl); c->d_nsrc = nullptr; c->d_a = nullptr; c->d_xf = nullptr; c->d_rel = nullptr; c->d_rel2 = nullptr; c->d_dirty = nullptr;
  dev_free(c->d_nn_idx); dev_free(c->d_nn_d2); dev_free(c->d_nn_lb); dev_free(c->d_first); dev_free(c->d_second);
  dev_free(c->d_sblock_off); dev_free(c->d_sel_keys1); c->n_sblocks = 0;
  dev_free(c->d_cd2); dev_free(c->d_qpos); dev_free(c->d_dirty_slots); dev_free(c->d_dslot_off); dev_free(c->d_stream); dev_free(c->d_cblock_off); dev_free(c->d_cblock_cnt);
  dev_free(c->d_sel_hist); dev_free(c->d_median); dev_free(c->d_chunk_edge); dev_free(c->d_chunk_start);
  dev_free(c->d_chunk_first); dev_free(c->d_partials); dev_free(c->d_out);
  c->sym_lo_pin.release(); c->sym_lo_dev.release();
  if (c->h_pin) (void)hipHostFree(c->h_pin);
  c->h_pin = nullptr; c->h_pin_doubles = 0; c->d_res_host = nullptr; c->d_blocks_host = nullptr; c->lin_out = nullptr;
  c->census_pending = false; c->spec_ready = false; c->spec2_ready = false; c->spec_arm = false; c->d_spec_host = nullptr; c->d_adev_host = nullptr; c->d_res_target = nullptr; c->d_a_check = nullptr;
  dev_free(c->d_xblock_cnt); c->export_valid = false; c->export_in_flight = false; c->export_chunks = 0;
  for (hipEvent_t ev : c->export_events) (void)hipEventDestroy(ev);
  c->export_events.clear();
  if (c->d_export) (void)hipFree(c->d_export);
  if (c->h_export) (void)hipHostFree(c->h_export);
  c->d_export = nullptr; c->h_export = nullptr; c->export_cap = 0;
  c->E = 0; c->total_cap = 0; c->n_cblocks = 0; c->n_chunks = 0; c->n_lin_wg = 0; c->hist.have_corr = false;
}

int bind(mvicp_ctx* c) {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  MV_HIP(hipSetDevice(c->device));
  return MVICP_OK;
}

int ensure_pin(mvicp_ctx* c, size_t doubles) {
  if (doubles <= c->h_pin_doubles) return MVICP_OK;
  if (c->h_pin) MV_HIP(hipHostFree(c->h_pin));
  c->h_pin = nullptr;
  MV_HIP(hipHostMalloc((void**)&c->h_pin, sizeof(double) * doubles, hipHostMallocMapped));
  std::memset(c->h_pin, 0, sizeof(double) * doubles);
  c->h_pin_doubles = doubles;
  return MVICP_OK;
}

}  // namespace

// Per-edge relative transform for the LM kernels: A = R_d^T R_s, t = R_d^T (t_s - t_d).
static void fill_rel_into(mvicp_ctx* c, const double* poses, double* h);
void fill_rel(mvicp_ctx* c, const double* poses) {
  fill_rel_into(c, poses, c->h_pin + c->ctl_r2_off);  // region 2 of the control block: rel | a (a = SoftLOne scales, set by correspond)
}
static void fill_rel_into(mvicp_ctx* c, const double* poses, double* h) {
  for (int e = 0; e < c->E; ++e) {
    const double* Ps = poses + 16 * (size_t)c->esrc[e];
    const double* Pd = poses + 16 * (size_t)c->edst[e];
    double* r = h + (size_t)e * kEdgeRel;
    for (int j = 0; j < 3; ++j)
      for (int i = 0; i < 3; ++i) r[i + 3 * j] = Pd[0 + 4 * i] * Ps[0 + 4 * j] + Pd[1 + 4 * i] * Ps[1 + 4 * j] + Pd[2 + 4 * i] * Ps[2 + 4 * j];
    const double dt[3] = {Ps[12] - Pd[12], Ps[13] - Pd[13], Ps[14] - Pd[14]};
    for (int i = 0; i < 3; ++i) r[9 + i] = Pd[0 + 4 * i] * dt[0] + Pd[1 + 4 * i] * dt[1] + Pd[2 + 4 * i] * dt[2];
  }
}
int upload_rel(mvicp_ctx* c, const double* poses) {
  fill_rel(c, poses);
  MV_HIP(hipMemcpyAsync(c->d_rel, c->h_pin + c->ctl_r2_off, sizeof(double) * c->ctl_r2, hipMemcpyHostToDevice, c->stream));
  return MVICP_OK;
}

// The symmetric objective's relative transforms.  Its residual m . (A p + t - q) is a small difference of large terms in which an error of the
// relative transform is COMMON to all correspondences of the edge, so it adds up over N terms where the residuals themselves add up like sqrt(N):
// the fp64 rounding of (A, t), and the defect of R_d^T against R_d^-1 for a pose that is orthonormal to a few eps only, would cost g a factor
// sqrt(N) (|t| + |p|) / |r| (measured: 80 - 600 x the error of a plain fp64 evaluation in the world frame, tests/test_gpu_sym_accuracy.py).  So
// A = R_d^-1 R_s and t = R_d^-1 (t_s - t_d) are formed with the TRUE inverse in extended precision (for a rotation R_d^-1 = R_d^T) and split into
// hi + lo: hi goes where fill_rel puts the relative transform (the kernel's moments and reduce_expand_kernel read it), lo to a small buffer of
// its own (sym_lo_pin -> sym_lo_dev, copied in stream order right behind the control block), which the kernel adds to the residual only.
// A destination matrix whose determinant is not within (0.5, 2) is no rotation: for it the transpose is used, as fill_rel does.
static void fill_rel_sym(mvicp_ctx* c, const double* poses, double* h, double* lo) {
  typedef long double ld;
  for (int e = 0; e < c->E; ++e) {
    const double* Ps = poses + 16 * (size_t)c->esrc[e];
    const double* Pd = poses + 16 * (size_t)c->edst[e];
    ld M[3][3];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) M[i][j] = Pd[i + 4 * j];
    ld C[3][3];   // cofactors
    C[0][0] = M[1][1] * M[2][2] - M[1][2] * M[2][1]; C[0][1] = M[1][2] * M[2][0] - M[1][0] * M[2][2]; C[0][2] = M[1][0] * M[2][1] - M[1][1] * M[2][0];
    C[1][0] = M[0][2] * M[2][1] - M[0][1] * M[2][2]; C[1][1] = M[0][0] * M[2][2] - M[0][2] * M[2][0]; C[1][2] = M[0][1] * M[2][0] - M[0][0] * M[2][1];
    C[2][0] = M[0][1] * M[1][2] - M[0][2] * M[1][1]; C[2][1] = M[0][2] * M[1][0] - M[0][0] * M[1][2]; C[2][2] = M[0][0] * M[1][1] - M[0][1] * M[1][0];
    ld det = M[0][0] * C[0][0] + M[0][1] * C[0][1] + M[0][2] * C[0][2];
    if (!(det > 0.5L && det < 2.0L)) {
      // not a rotation (a degenerate or reflected matrix): no inverse worth forming.  Use the transpose, as fill_rel does, so that the values stay finite
      for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) C[i][j] = M[i][j];
      det = 1.0L;
    }
    ld v[kEdgeRel];
    const ld dt[3] = {(ld)Ps[12] - (ld)Pd[12], (ld)Ps[13] - (ld)Pd[13], (ld)Ps[14] - (ld)Pd[14]};
    for (int i = 0; i < 3; ++i) {
      const ld inv_i[3] = {C[0][i] / det, C[1][i] / det, C[2][i] / det};   // row i of R_d^-1
      for (int j = 0; j < 3; ++j) v[i + 3 * j] = inv_i[0] * (ld)Ps[0 + 4 * j] + inv_i[1] * (ld)Ps[1 + 4 * j] + inv_i[2] * (ld)Ps[2 + 4 * j];
      v[9 + i] = inv_i[0] * dt[0] + inv_i[1] * dt[1] + inv_i[2] * dt[2];
    }
    for (int k = 0; k < kEdgeRel; ++k) {
      const double hi = (double)v[k];
      h[(size_t)e * kEdgeRel + k] = hi;
      lo[(size_t)e * kEdgeRel + k] = (double)(v[k] - (ld)hi);
    }
  }
}
int upload_rel_sym(mvicp_ctx* c, const double* poses) {
  const size_t bytes = sizeof(double) * (size_t)c->E * kEdgeRel;
  MV_CHECK(c->sym_lo_pin.reserve(bytes));   // (every evaluation ends with a wait for the stream, so the previous copy out of this buffer is done)
  MV_CHECK(c->sym_lo_dev.reserve(bytes));
  fill_rel_sym(c, poses, c->h_pin + c->ctl_r2_off, (double*)c->sym_lo_pin.p);
  MV_HIP(hipMemcpyAsync(c->d_rel, c->h_pin + c->ctl_r2_off, sizeof(double) * c->ctl_r2, hipMemcpyHostToDevice, c->stream));
  MV_HIP(hipMemcpyAsync(c->sym_lo_dev.p, c->sym_lo_pin.p, bytes, hipMemcpyHostToDevice, c->stream));
  return MVICP_OK;
}

// Wait for the stream.  The hot loop waits ~5 times per ICP round for a few hundred microseconds of GPU work; a blocking
// wait adds a scheduler wake-up to each, so poll first and only block when the work is long.
int stream_wait(mvicp_ctx* c) {
  if (c->spin_wait) {
    const double t0 = now_ms();
    for (;;) {
      const hipError_t q = hipStreamQuery(c->stream);
      if (q == hipSuccess) return MVICP_OK;
      if (q != hipErrorNotReady) { set_error("hipStreamQuery -> %s", hipGetErrorString(q)); return MVICP_ERR_HIP; }
      if (now_ms() - t0 > 2.0) break;
    }
  }
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
}

// NN census (profiling only): the counters of the last NN launch were copied to pinned memory asynchronously; fold them
// into the "nn" profile entry once the stream has been waited for anyway.
void census_resolve(mvicp_ctx* c) {
  if (!c->census_pending) return;
  c->census_pending = false;
  const unsigned long long* st = c->h_census;
  const double nq = c->census_nq;
  ProfEntry& pe = c->prof[c->census_scope];
  // SURVEY.md §8(d) algorithmic bytes of an NN launch = 36 B per query (already in the scope) + 24 B per candidate point FETCHED FROM
  // MEMORY + 8 B per cell / box looked up; the library's own finer model (record widths, cache state) goes to pe.bytes as before
  if (c->census_kind == 3) {
    // cell-staging kernel: st[4] points staged into LDS (24 B each, once per wave), st[5] distinct cells looked up per wave (16-B brick
    // entry + 8-B cell-table entry), st[0] candidates scanned from LDS (no memory traffic), far part (st[1] boxes) from nn_far_kernel
    const double hits = (double)st[3];
    pe.bytes += 36.0 * hits + 24.0 * (double)st[4] + 24.0 * (double)st[5] + 32.0 * (double)st[1];
    c->nn_candidates += (double)st[0]; c->nn_nodes += (double)st[1] + (double)st[5]; c->nn_far += (double)st[2]; c->nn_queries += nq; c->nn_hits += hits;
    c->nn_fetched += (double)st[4];
    pe.survey_bytes += 24.0 * (double)st[4] + 8.0 * ((double)st[1] + (double)st[5]);
  } else if (c->census_kind == 2) {
    c->nn_fetched += (double)st[0];
    pe.survey_bytes += 24.0 * (double)st[0] + 8.0 * (double)st[1];
    // tile kernel, memory side: every opened tile is loaded ONCE per wave (24 B xyz + 4 B index per point) and every tested
    // box once per wave (24 B); the per-lane distance evaluations (st[2]) are served from LDS.
    pe.bytes += 28.0 * (double)st[0] + 24.0 * (double)st[1];
    c->nn_candidates += (double)st[2]; c->nn_nodes += (double)st[1]; c->nn_queries += nq;
    for (int k = 0; k < 4; ++k) c->nn_dbg[k] += (double)st[4 + k];
    c->nn_hits += (double)st[3]; pe.bytes += 36.0 * (double)st[3];   // cache-aware rounds: lanes answered by the temporal cache (index, bound, neighbour point, bound write)
  } else {
    // cache hit: previous index 4 B + fp32 bound 4 B + one 24-B point + bound write 4 B; searched query: 8 hash slots x 16 B + bound
    // write 4 B; every candidate point examined: one 32-B record; every tree box tested: 32 B
    const double hits = (double)st[3], searched = nq - hits;
    pe.bytes += 36.0 * hits + (c->census_kind == 1 ? 4.0 : 132.0) * searched + 32.0 * (double)st[0] + 32.0 * (double)st[1];
    c->nn_candidates += (double)st[0]; c->nn_nodes += (double)st[1]; c->nn_far += (double)st[2]; c->nn_queries += nq; c->nn_hits += hits;
    c->nn_fetched += (double)st[0];   // per-lane kernel: every candidate examined is a record fetched
    pe.survey_bytes += 24.0 * (double)st[0] + 8.0 * (double)st[1];
  }
}

// ---- background structure builds (mvicp_set_frame) ---------------------------------------------------------------------------------------
namespace {
// at most one build per hardware thread at a time (each build forks a few threads of its own for the k-d order)
struct BuildSlots {
  std::mutex m; std::condition_variable cv; int free_slots;
  BuildSlots() : free_slots((int)std::max(2u, std::min(32u, std::thread::hardware_concurrency()))) {}
  void acquire() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [this]() { return free_slots > 0; }); --free_slots; }
  void release() { { std::lock_guard<std::mutex> lk(m); ++free_slots; } cv.notify_one(); }
};
BuildSlots& build_slots() { static BuildSlots s; return s; }
}  // namespace

// upload of the normals in the cloud's sorted order (needs the order the build produced)
static int upload_sorted_normals(FrameDev& f, const double* nrm) {
  const int n = f.n;
  std::vector<double> sn(3 * (size_t)n);
  for (int i = 0; i < n; ++i) std::memcpy(&sn[3 * (size_t)i], nrm + 3 * (size_t)f.grid.h_order[i], 24);
  MV_HIP(hipMalloc((void**)&f.grid.snor, sizeof(double) * 3 * (size_t)std::max(n, 1)));
  MV_HIP(hipMemcpy(f.grid.snor, sn.data(), sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
  return MVICP_OK;
}

static bool injected_build_failure(mvicp_ctx* c) {
  if (c->fault_inject_build.load() > 0 && c->fault_inject_build.fetch_sub(1) == 1) { set_error("injected structure-build failure (option fault_inject_build)"); return true; }
  return false;
}

static int build_frame_structures(mvicp_ctx* c, FrameDev& f, const double* xyz, const double* nrm) {
  if (injected_build_failure(c)) return MVICP_ERR_INTERNAL;
  const auto t0 = std::chrono::steady_clock::now();
  MV_CHECK(build_grid(c, f, xyz));
  if (nrm) MV_CHECK(upload_sorted_normals(f, nrm));
  f.build_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  f.build_ms[1] = -1.0;
  return MVICP_OK;
}

// the device build of a cloud that mvicp_set_frame_device has copied to f.pts / f.nor (build.hip); the sorted normals are gathered there
static int build_frame_structures_device(mvicp_ctx* c, FrameDev& f, const DevBounds& b, int grid_curve, double grid_target) {
  if (injected_build_failure(c)) return MVICP_ERR_INTERNAL;
  return build_grid_device(c, f, b, grid_curve, grid_target);
}

int finish_builds(mvicp_ctx* c) {
  for (FrameDev& f : c->frames) {
    if (!f.job) continue;
    int s1 = MVICP_ERR_INTERNAL;
    try { s1 = f.job->fut.get(); } catch (...) { f.job->err = "structure build threw"; }
    if (s1 != MVICP_OK) {
      // sticky: the frame stays unusable (and says why) until it is uploaded again; its half-built structures are released now
      f.build_error = f.job->err.empty() ? std::string("structure build failed") : f.job->err;
      (void)hipSetDevice(c->device);
      free_grid(f.grid); f.has_grid = false;
    }
    f.job.reset();
  }
  for (size_t i = 0; i < c->frames.size(); ++i)
    if (!c->frames[i].build_error.empty()) {
      set_error("frame %d: %s (upload the cloud again with mvicp_set_frame)", (int)i, c->frames[i].build_error.c_str());
      return MVICP_ERR_STATE;
    }
  return MVICP_OK;
}

// Back-pressure of the background builds: each pending build holds a private copy of its cloud (48 B per point) and a parked thread; only the
// builds themselves are throttled by the slots.  An upload loop over many large clouds (64 x 1 M points = 3 GB of copies) therefore waits here
// for its oldest pending build once as many are pending as there are slots.  (The job's status is kept for finish_builds.)
static void throttle_builds(mvicp_ctx* c) {
  const int limit = std::max(2, (int)std::min(32u, std::thread::hardware_concurrency()));
  for (;;) {
    int pending = 0;
    BuildJob* oldest = nullptr;
    for (FrameDev& f : c->frames)
      if (f.job && f.job->fut.valid() && f.job->fut.wait_for(std::chrono::seconds(0)) != std::future_status::ready) { if (!oldest) oldest = f.job.get(); ++pending; }
    if (pending < limit || !oldest) return;
    oldest->fut.wait();
  }
}

// One device evaluation of all per-edge blocks at `poses` -> host `out` (E x 91), all-reduced over ranks.
// (`metric` is an mvicp_metric: 0 point, 1 plane, 2 symmetric — the older entry points hand in their point_to_plane flag as 0 / 1)
static int check_evaluable(mvicp_ctx* c, int metric) {
  if (!c->hist.have_corr) { set_error("no correspondences: call mvicp_correspond or mvicp_set_correspondences first"); return MVICP_ERR_STATE; }
  if (metric == MVICP_METRIC_SYMMETRIC || metric == kMetricGicp) {
    // the mean normal, and the sum of the two covariances, need both normals: the destination's (baked into the operand stream) and the source's (read from its sorted normals)
    for (int e = 0; e < c->E; ++e)
      if (c->owned[e] && c->hist.h_count[e] > 0) {
        const int missing = c->frames[c->edst[e]].grid.snor == nullptr ? c->edst[e] : c->frames[c->esrc[e]].grid.snor == nullptr ? c->esrc[e] : -1;
        if (missing >= 0) { set_error("%s needs normals on frame %d", metric == kMetricGicp ? "gicp" : "symmetric", missing); return MVICP_ERR_STATE; }
      }
  } else if (metric) {
    for (int e = 0; e < c->E; ++e)
      if (c->owned[e] && c->hist.h_count[e] > 0 && c->frames[c->edst[e]].grid.snor == nullptr) {
        set_error("point-to-plane needs normals on frame %d", c->edst[e]);
        return MVICP_ERR_STATE;
      }
  }
  return MVICP_OK;
}

// Single rank: the blocks at poses_a and at poses_b from ONE paired launch (linearize.hip), each what evaluate_blocks gives for its poses bit for bit.  The
// queued evaluations of the last search, their buffers and the candidate-pose prediction are left alone.
int evaluate_pair(mvicp_ctx* c, const double* poses_a, const double* poses_b, int plane, int robust, double* out_a, double* out_b) {
  MV_CHECK(check_evaluable(c, plane));
  HostScope hs(c, "host.evaluate");
  const size_t n = (size_t)c->E * MVICP_EDGE_BLOCK;
  fill_rel_into(c, poses_b, c->h_pin + c->ctl_rel2_off);
  fill_rel(c, poses_a);
  // rel2 | rel | a are adjacent in the control block: one upload
  MV_HIP(hipMemcpyAsync(c->d_rel2, c->h_pin + c->ctl_rel2_off, sizeof(double) * ((size_t)c->E * kEdgeRel + c->ctl_r2), hipMemcpyHostToDevice, c->stream));
  MV_CHECK(launch_linearize_pair(c, plane, robust, c->d_blocks_host, c->d_blocks2_host));
  MV_CHECK(stream_wait(c));
  std::memcpy(out_a, c->h_pin + c->pin_blocks_off, sizeof(double) * n);
  std::memcpy(out_b, c->h_pin + c->pin_blocks2_off, sizeof(double) * n);
  return MVICP_OK;
}

// One launch of the metric's accumulation kernel + the per-edge expansion on the uploaded relative transforms
static int launch_metric(mvicp_ctx* c, int metric, int robust) {
  if (metric == kMetricGicp) return launch_linearize_gicp(c, c->gicp_eps, robust);
  return metric == MVICP_METRIC_SYMMETRIC ? launch_linearize_sym(c, robust) : launch_linearize(c, metric, robust);
}

// `plane` is the metric (0 point, 1 plane, 2 symmetric, kMetricGicp plane-to-plane at c->gicp_eps).  Only point and plane evaluations are ever queued ahead, so a symmetric
// or plane-to-plane one matches no
// queued result (spec_q_plane / spec2_plane are 0 or 1), drops them like any evaluation they were not made for, and takes the ordinary route below.
// With an exchange configured a refusal of check_evaluable is a LOCAL verdict (it looks at the edges this rank owns: only the owner knows the count of
// an explicit list), so it is treated like a failed local launch: the rank enters the evaluation's collective with the slot poisoned, and every
// rank returns non-OK from the same call (the refusing rank its own MVICP_ERR_STATE, the peers MVICP_ERR_COMM) instead of the peers waiting in it.
// No rank serves such an evaluation from the queue: a searched non-empty list whose target has no normals disarms the queued evaluation on
// every rank (mvicp_correspond decides that from the frames, which every rank holds).
int evaluate_blocks(mvicp_ctx* c, const double* poses, int plane, int robust, double* out) {
  const bool exchange = c->comm || c->ar_fn;
  const int st_chk = check_evaluable(c, plane);
  if (st_chk != MVICP_OK && !exchange) return st_chk;
  HostScope hs(c, "host.evaluate");
  const size_t n = (size_t)c->E * MVICP_EDGE_BLOCK;
  if (st_chk != MVICP_OK) { c->spec_ready = false; c->spec2_ready = false; }
  if (c->spec_ready) {
    // the evaluation mvicp_correspond queued ahead: valid only for exactly these poses and flags
    c->spec_ready = false;
    if (plane == c->spec_q_plane && robust == c->spec_q_robust && c->spec_poses.size() == 16 * (size_t)c->n_frames &&
        std::memcmp(poses, c->spec_poses.data(), sizeof(double) * c->spec_poses.size()) == 0) {
      std::memcpy(out, c->h_pin + c->pin_spec_off, sizeof(double) * n);
      if (c->profile) c->prof["spec.hit"].launches += 1;   // (observable for tests / bench: evaluations served by the queued launch)
      return MVICP_OK;
    }
    c->spec2_ready = false;   // the solve did not start where the queued evaluations assumed: the second one is void as well
  }
  if (c->spec2_ready) {
    // the second queued evaluation (see common.h): valid only for exactly these poses and flags
    c->spec2_ready = false;
    if (plane == c->spec2_plane && robust == c->spec2_robust && c->spec2_poses.size() == 16 * (size_t)c->n_frames &&
        std::memcmp(poses, c->spec2_poses.data(), sizeof(double) * c->spec2_poses.size()) == 0) {
      std::memcpy(out, c->h_pin + c->pin_spec2_off, sizeof(double) * n);
      if (c->profile) c->prof["spec2.hit"].launches += 1;
      c->hist.last_cand_poses.assign(poses, poses + 16 * (size_t)c->n_frames); c->hist.last_cand_plane = plane; c->hist.last_cand_robust = robust;
      return MVICP_OK;
    }
  }
  // (an evaluation beyond the solve's first: what the next solve's candidate evaluation will most likely be asked at, if the poses do not move)
  c->hist.last_cand_poses.assign(poses, poses + 16 * (size_t)c->n_frames); c->hist.last_cand_plane = plane; c->hist.last_cand_robust = robust;
  double* h = c->h_pin + c->pin_blocks_off;
  if (exchange) {
    // One collective per evaluation: [E x 91 blocks | poison slot].  The slot right behind the blocks (the buffer's tail region, rewritten
    // by every search) is zeroed, or — if this rank refused the evaluation, or its upload / launch failed — poisoned with a NaN, so that a local
    // failure reaches every rank through the collective instead of leaving the peers blocked in it (see mvicp_correspond).
    c->lin_out = c->d_out;
    int st_l = st_chk;
    if (st_l == MVICP_OK) st_l = (plane == MVICP_METRIC_SYMMETRIC || plane == kMetricGicp) ? upload_rel_sym(c, poses) : upload_rel(c, poses);
    if (st_l == MVICP_OK && c->fault_inject_eval > 0 && --c->fault_inject_eval == 0) { set_error("injected launch failure (option fault_inject_eval)"); st_l = MVICP_ERR_HIP; }
    if (st_l == MVICP_OK) st_l = launch_metric(c, plane, robust);
    char local_msg[sizeof(g_err)] = "";
    if (st_l != MVICP_OK) std::memcpy(local_msg, g_err, sizeof(local_msg));
    if (hipMemsetAsync(c->d_out + n, st_l == MVICP_OK ? 0 : 0xFF, sizeof(double), c->stream) != hipSuccess) {
      if (st_l != MVICP_OK) return st_l;
      set_error("hipMemsetAsync of the poison slot failed"); return MVICP_ERR_HIP;
    }
    { ProfScope pc(c, "comm", 8.0 * (double)(n + 1)); MV_CHECK(comm_allreduce_sum(c, c->d_out, n + 1)); }
    double* hx = c->h_pin + c->pin_spec_off;   // (the spec region holds E x 94 + 2 doubles: room for the slot; the queued blocks in it were consumed or dropped above)
    MV_HIP(hipMemcpyAsync(hx, c->d_out, sizeof(double) * (n + 1), hipMemcpyDeviceToHost, c->stream));
    MV_CHECK(stream_wait(c));
    if (std::isnan(hx[n])) {
      if (st_l != MVICP_OK) { set_error("%s", local_msg); return st_l; }
      set_error("a peer rank failed before the exchange of this evaluation (poisoned exchange buffer)");
      return MVICP_ERR_COMM;
    }
    std::memcpy(out, hx, sizeof(double) * n);
    return MVICP_OK;
  } else {
    MV_CHECK((plane == MVICP_METRIC_SYMMETRIC || plane == kMetricGicp) ? upload_rel_sym(c, poses) : upload_rel(c, poses));
    c->lin_out = c->d_blocks_host;   // 8 * 91 * E bytes: the reduce kernel stores them straight into mapped host memory
    MV_CHECK(launch_metric(c, plane, robust));
  }
  MV_CHECK(stream_wait(c));
  std::memcpy(out, h, sizeof(double) * n);
  return MVICP_OK;
}

}  // namespace mvicp

using namespace mvicp;

extern "C" {

const char* mvicp_last_error(void) { return g_err; }
const char* mvicp_version(void) { return "mvicp_hip 0.5 (gfx950)"; }

int mvicp_create(int device, mvicp_ctx** out) try {
  if (!out) { set_error("out is null"); return MVICP_ERR_ARG; }
  *out = nullptr;
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev <= 0) {
    set_error("no HIP device available (%s): libmvicp_hip has no CPU fallback", e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    return MVICP_ERR_HIP;
  }
  if (device < 0 || device >= ndev) { set_error("device %d out of range [0,%d)", device, ndev); return MVICP_ERR_ARG; }
  mvicp_ctx* c = new mvicp_ctx();
  c->device = device;
  MV_HIP(hipSetDevice(device));
  MV_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  *out = c;
  return MVICP_OK;
} MVICP_GUARD_ABI

// the results and the buffers of every stage that keeps its last result on the context (common.h)
static void release_stages(mvicp_ctx* c) {
  c->vox.release(); c->out.release(); c->knn.release(); c->fpfh.release();
  c->match.release(); c->cons.release(); c->coarse.release(); c->iss.release(); c->nrm.release();
  c->ori.release(); c->agree.release(); c->clu.release(); c->plane.release(); c->bnd.release();
}

int mvicp_destroy(mvicp_ctx* c) try {
  if (!c) return MVICP_OK;
  (void)hipSetDevice(c->device);
  (void)finish_builds(c);
  (void)hipStreamSynchronize(c->stream);
  comm_destroy(c);
  free_graph(c);
  for (FrameDev& f : c->frames) { dev_free(f.pts); dev_free(f.nor); free_grid(f.grid); free_tie(f); }
  dev_free(c->d_split_idx); dev_free(c->d_split_d2); dev_free(c->d_scratch);
  free_overlap(c);
  release_stages(c);
  for (auto& kv : c->tables) if (kv.second.d) (void)hipFree(kv.second.d);
  if (c->d_census) (void)hipFree(c->d_census);
  if (c->h_census) (void)hipHostFree(c->h_census);
  if (c->d_tie_list) (void)hipFree(c->d_tie_list);
  if (c->d_tie_count) (void)hipFree(c->d_tie_count);
  if (c->d_tie_deep) (void)hipFree(c->d_tie_deep);
  if (c->h_tie_seen) (void)hipHostFree(c->h_tie_seen);
  if (c->h_far_seen) (void)hipHostFree(c->h_far_seen);
  if (c->d_far_list) (void)hipFree(c->d_far_list);
  if (c->d_far_count) (void)hipFree(c->d_far_count);
  for (auto& kv : c->prof) {
    for (auto& pr : kv.second.pending) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t ev : kv.second.pool) (void)hipEventDestroy(ev);
  }
  (void)hipStreamDestroy(c->stream);
  delete c;
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_set_num_frames(mvicp_ctx* c, int n_frames) try {
  MV_CHECK(bind(c));
  if (n_frames < 0) { set_error("n_frames < 0"); return MVICP_ERR_ARG; }
  (void)finish_builds(c);   // (builds of clouds that are dropped right here: their outcome no longer matters)
  if (c->E) free_graph(c);
  release_stages(c);   // (the last result of every stage ends here; every stage's call waits for its own work)
  for (FrameDev& f : c->frames) { dev_free(f.pts); dev_free(f.nor); free_grid(f.grid); free_tie(f); }
  c->frames.assign(n_frames, FrameDev());
  c->n_frames = n_frames;
  return MVICP_OK;
} MVICP_GUARD_ABI

// the results that an upload to `frame` ends: every stage that remembers the frame it was computed for
static void drop_results_of(mvicp_ctx* c, int frame) {
  if (c->nrm.frame == frame) c->nrm.drop_result();   // (estimated normals of the cloud the upload replaces: nothing to adopt them into)
  if (c->ori.frame == frame) c->ori.drop_result();   // (and its oriented normals)
  if (c->clu.frame == frame) c->clu.drop_result();   // (and its clusters: a selection would read the new rows)
  if (c->plane.frame == frame) c->plane.drop_result();   // (and its plane, for the same reason)
  if (c->bnd.frame == frame) c->bnd.drop_result();   // (and its boundary points, for the same reason)
}

int mvicp_set_frame(mvicp_ctx* c, int frame, const double* xyz, const double* nrm, int n) try {
  MV_CHECK(bind(c));
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (n < 0 || (n > 0 && !xyz)) { set_error("bad cloud (n=%d)", n); return MVICP_ERR_ARG; }
  if (c->E) { set_error("set frames before mvicp_set_graph"); return MVICP_ERR_STATE; }
  // every check comes before the frame is touched: a refused upload leaves the frame's cloud, structures and pending build as they were
  double max_norm = 0.0;
  for (int i = 0; i < n; ++i) {
    const double* p = xyz + 3 * (size_t)i;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) { set_error("non-finite coordinate in cloud"); return MVICP_ERR_ARG; }   // (reported by this call, not by a later one)
    max_norm = std::max(max_norm, std::sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]));
  }
  FrameDev& f = c->frames[frame];
  drop_results_of(c, frame);
  if (f.job) { try { (void)f.job->fut.get(); } catch (...) {} f.job.reset(); }   // a build of the cloud this call replaces
  dev_free(f.pts); dev_free(f.nor); free_grid(f.grid); free_tie(f);
  f.has_grid = false; f.build_error.clear();
  f.n = 0; f.max_norm = 0.0;   // (a failed allocation or copy below leaves an empty frame, not a cloud of undefined bytes)
  MV_CHECK(dev_alloc(&f.pts, 3 * (size_t)n));
  if (n) MV_HIP(hipMemcpy(f.pts, xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
  if (nrm) {
    MV_CHECK(dev_alloc(&f.nor, 3 * (size_t)n));
    if (n) MV_HIP(hipMemcpy(f.nor, nrm, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
  }
  f.n = n;
  f.max_norm = max_norm;
  if (n == 0) return MVICP_OK;
  if (!c->async_build) {
    const int st = build_frame_structures(c, f, xyz, nrm);
    if (st != MVICP_OK) { f.build_error = g_err; free_grid(f.grid); f.has_grid = false; }
    return st;
  }
  // The per-cloud structures (k-d order, box hierarchy, matrix-pipe operands, hash: ~0.1 s of host work per 200 k points) are built on a
  // thread of their own from a private copy of the cloud, so that a driver's upload loop builds its clouds side by side (cfg4: 32 clouds,
  // 2.9 s one after the other); whoever needs a structure first waits for the pending builds (finish_builds).
  throttle_builds(c);
  std::shared_ptr<BuildJob> job = std::make_shared<BuildJob>();
  job->xyz.assign(xyz, xyz + 3 * (size_t)n);
  if (nrm) job->nrm.assign(nrm, nrm + 3 * (size_t)n);
  FrameDev* fp = &f;   // (stable: mvicp_set_num_frames, the only call that moves the frames, waits for the builds first)
  BuildJob* jp = job.get();
  job->fut = std::async(std::launch::async, [c, fp, jp]() -> int {
    build_slots().acquire();
    int st = MVICP_ERR_INTERNAL;
    try {
      st = hipSetDevice(c->device) == hipSuccess ? build_frame_structures(c, *fp, jp->xyz.data(), jp->nrm.empty() ? nullptr : jp->nrm.data()) : MVICP_ERR_HIP;
      if (st != MVICP_OK) jp->err = g_err;   // (this worker's thread-local message)
    } catch (const std::exception& e) { jp->err = std::string("structure build: ") + e.what(); }
    catch (...) { jp->err = "structure build threw"; }
    std::vector<double>().swap(jp->xyz); std::vector<double>().swap(jp->nrm);
    build_slots().release();
    return st;
  });
  f.job = job;
  return MVICP_OK;
} MVICP_GUARD_ABI

// a device pointer of this context's device (hipPointerGetAttributes), else MVICP_ERR_ARG
static int check_device_pointer(mvicp_ctx* c, const void* p, const char* what) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) {
    (void)hipGetLastError();   // (the failed query leaves its error behind; the next launch check must not report it)
    set_error("%s is not a device pointer (%s)", what, hipGetErrorString(e));
    return MVICP_ERR_ARG;
  }
  if (at.type != hipMemoryTypeDevice) { set_error("%s is not device memory (memory type %d)", what, (int)at.type); return MVICP_ERR_ARG; }
  if (at.device != c->device) { set_error("%s lives on device %d, the context on device %d", what, at.device, c->device); return MVICP_ERR_ARG; }
  return MVICP_OK;
}

int mvicp_set_frame_device(mvicp_ctx* c, int frame, const double* d_xyz, const double* d_nrm, int n) try {
  MV_CHECK(bind(c));
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (n < 0 || (n > 0 && !d_xyz)) { set_error("bad cloud (n=%d)", n); return MVICP_ERR_ARG; }
  if (c->E) { set_error("set frames before mvicp_set_graph"); return MVICP_ERR_STATE; }
  if (n > 0) {
    MV_CHECK(check_device_pointer(c, d_xyz, "xyz"));
    if (d_nrm) MV_CHECK(check_device_pointer(c, d_nrm, "nrm"));
  }
  // The one reduction the call itself needs -- finiteness (reported by this call), max_norm, the bounding box and max |coordinate| of the
  // build -- runs over the CALLER's array before the frame is touched: a refused upload leaves the frame's cloud, structures and pending
  // build as they were.  (The library's copy below holds the same bytes, so the build sees the same bounds.)
  const auto t0 = std::chrono::steady_clock::now();
  DevBounds b;
  std::memset(&b, 0, sizeof(b));
  if (n > 0) {
    MV_CHECK(device_bounds(c->stream, d_xyz, n, &b));
    if (b.nonfinite) { set_error("non-finite coordinate in cloud"); return MVICP_ERR_ARG; }
  }
  FrameDev& f = c->frames[frame];
  drop_results_of(c, frame);
  if (f.job) { try { (void)f.job->fut.get(); } catch (...) {} f.job.reset(); }   // a build of the cloud this call replaces
  dev_free(f.pts); dev_free(f.nor); free_grid(f.grid); free_tie(f);
  f.has_grid = false; f.build_error.clear();
  f.n = 0; f.max_norm = 0.0;   // (a failed allocation or copy below leaves an empty frame, not a cloud of undefined bytes)
  // library-owned copies, complete when the call returns: the caller may reuse its buffers, and the build reads them on a stream of its own
  MV_CHECK(dev_alloc(&f.pts, 3 * (size_t)n));
  if (n) MV_HIP(hipMemcpyAsync(f.pts, d_xyz, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
  if (d_nrm) {
    MV_CHECK(dev_alloc(&f.nor, 3 * (size_t)n));
    if (n) MV_HIP(hipMemcpyAsync(f.nor, d_nrm, sizeof(double) * 3 * (size_t)n, hipMemcpyDeviceToDevice, c->stream));
  }
  MV_HIP(hipStreamSynchronize(c->stream));
  f.n = n;
  if (n == 0) return MVICP_OK;
  b.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  f.max_norm = b.max_norm;
  const int curve = c->grid_curve;
  const double target = c->grid_target;
  if (!c->async_build) {
    const int st = build_frame_structures_device(c, f, b, curve, target);
    if (st != MVICP_OK) { f.build_error = g_err; free_grid(f.grid); f.has_grid = false; }
    return st;
  }
  // the rest of the build runs behind the call, as mvicp_set_frame's does, on a stream of its own; no host copy of the cloud is held
  throttle_builds(c);
  std::shared_ptr<BuildJob> job = std::make_shared<BuildJob>();
  FrameDev* fp = &f;
  BuildJob* jp = job.get();
  job->fut = std::async(std::launch::async, [c, fp, jp, b, curve, target]() -> int {
    build_slots().acquire();
    int st = MVICP_ERR_INTERNAL;
    try {
      st = hipSetDevice(c->device) == hipSuccess ? build_frame_structures_device(c, *fp, b, curve, target) : MVICP_ERR_HIP;
      if (st != MVICP_OK) jp->err = g_err;
    } catch (const std::exception& e) { jp->err = std::string("structure build: ") + e.what(); }
    catch (...) { jp->err = "structure build threw"; }
    build_slots().release();
    return st;
  });
  f.job = job;
  return MVICP_OK;
} MVICP_GUARD_ABI

long long mvicp_get_structure(mvicp_ctx* c, int frame, const char* name, void* out, long long cap_bytes) try {
  MV_CHECK(bind(c));
  if (frame < 0 || frame >= c->n_frames || !name) { set_error("frame %d out of range [0,%d) or no name", frame, c->n_frames); return MVICP_ERR_ARG; }
  MV_CHECK(finish_builds(c));
  const FrameDev& f = c->frames[frame];
  if (!f.has_grid) { set_error("frame %d has no structures (n = %d)", frame, f.n); return MVICP_ERR_STATE; }
  const GridDev& G = f.grid;
  const size_t n = (size_t)f.n;
  const void* dsrc = nullptr; const void* hsrc = nullptr; size_t bytes = 0;
  std::vector<double> sc;
  const int tiles = (f.n + 31) / 32, blocks = (tiles + 63) / 64;
  if (!std::strcmp(name, "spts")) { dsrc = G.spts; bytes = 24 * n; }
  else if (!std::strcmp(name, "sidx")) { dsrc = G.sidx; bytes = 4 * n; }
  else if (!std::strcmp(name, "srec")) { dsrc = G.srec; bytes = sizeof(PointRec) * n; }
  else if (!std::strcmp(name, "crec")) { dsrc = G.crec; bytes = sizeof(PointRec) * n; }
  else if (!std::strcmp(name, "inv")) { dsrc = G.inv; bytes = 4 * n; }
  else if (!std::strcmp(name, "snor")) { dsrc = G.snor; bytes = G.snor ? 24 * n : 0; }
  else if (!std::strcmp(name, "table")) { dsrc = G.table; bytes = 16 * ((size_t)G.table_mask + 1); }
  else if (!std::strcmp(name, "oct")) { dsrc = G.oct; bytes = 32 * (size_t)(8 * G.oct_first_leaf + 1); }
  else if (!std::strcmp(name, "wide")) { dsrc = G.wide; bytes = 4 * (size_t)(G.wide_off[G.wide_levels - 1] + 6ll * G.wide_cnt[G.wide_levels - 1]); }
  else if (!std::strcmp(name, "mf_ops")) { dsrc = G.mf_ops; bytes = (size_t)std::max(tiles, 1) * 64 * 16; }
  else if (!std::strcmp(name, "mf_blk")) { dsrc = G.mf_blk; bytes = (size_t)std::max(blocks, 1) * 48; }
  else if (!std::strcmp(name, "bricks")) { dsrc = G.bricks; bytes = G.bricks ? 16 * (size_t)G.bdims[0] * G.bdims[1] * G.bdims[2] : 0; }
  else if (!std::strcmp(name, "celltab")) { dsrc = G.celltab; bytes = G.celltab ? G.celltab_bytes : 0; }
  else if (!std::strcmp(name, "h_order")) { hsrc = G.h_order.data(); bytes = 4 * G.h_order.size(); }
  else if (!std::strcmp(name, "h_inv")) { hsrc = G.h_inv.data(); bytes = 4 * G.h_inv.size(); }
  else if (!std::strcmp(name, "scalars") || !std::strcmp(name, "build_ms")) {
    if (name[0] == 's') {
      for (int a = 0; a < 3; ++a) sc.push_back(G.dims[a]);
      for (int a = 0; a < 3; ++a) sc.push_back(G.origin[a]);
      sc.push_back(G.cell); sc.push_back(G.inv_cell); sc.push_back(G.n_cells); sc.push_back(G.table_mask); sc.push_back(G.table_shift);
      sc.push_back(G.oct_leaf); sc.push_back((double)G.oct_first_leaf); sc.push_back(G.wide_levels);
      for (int l = 0; l < 6; ++l) sc.push_back(G.wide_cnt[l]);
      for (int l = 0; l < 6; ++l) sc.push_back((double)G.wide_off[l]);
      sc.push_back(G.maxabs); sc.push_back(G.struct_bytes); sc.push_back(f.max_norm);
      for (int a = 0; a < 3; ++a) sc.push_back(G.bdims[a]);
    } else {
      sc.push_back(f.build_ms[0]); sc.push_back(f.build_ms[1]);
    }
    hsrc = sc.data(); bytes = sizeof(double) * sc.size();
  } else { set_error("unknown structure name \"%s\"", name); return MVICP_ERR_ARG; }
  if (!out) return (long long)bytes;
  if (cap_bytes < (long long)bytes) { set_error("%s: %zu bytes do not fit in %lld", name, bytes, cap_bytes); return MVICP_ERR_ARG; }
  if (bytes == 0) return 0;
  if (hsrc) std::memcpy(out, hsrc, bytes);
  else {
    MV_HIP(hipStreamSynchronize(c->stream));   // (mvicp_recompute_normals rewrites snor on the context's stream)
    MV_HIP(hipMemcpy(out, dsrc, bytes, hipMemcpyDeviceToHost));
  }
  return (long long)bytes;
} MVICP_GUARD_ABI

// What follows new normals of `frame` (mvicp_recompute_normals, mvicp_normals_adopt), `st` being the status of the call so far: queued
// evaluations are void, and after a success every owned list that points into the frame is re-gathered.
static int normals_changed(mvicp_ctx* c, int frame, int st) {
  c->spec_ready = false; c->spec2_ready = false;
  if (st == MVICP_OK && c->E > 0) {
    // The packed operand stream bakes the dst normals in (n and c = n . q, gathered at correspond time) while the reference
    // reads dstCloud.nor when it builds the problem (icp-ceres.cpp:270-292): every list that points INTO this frame is stale.
    // Re-gather those edges now and never reuse their lists unchecked.
    bool any = false;
    std::vector<int> dirty(c->E, 0);
    for (int e = 0; e < c->E; ++e)
      if (c->owned[e] && c->edst[e] == frame) { c->hist.list_valid[e] = 0; if (c->hist.have_corr && c->hist.h_count[e] > 0) { dirty[e] = 1; any = true; } }
    if (any) {
      MV_HIP(hipMemcpy(c->d_dirty, dirty.data(), sizeof(int) * c->E, hipMemcpyHostToDevice));
      MV_CHECK(launch_gather_stream(c));
      MV_HIP(hipStreamSynchronize(c->stream));
    }
  }
  if (c->profile) prof_collect_lazy(c);
  return st;
}

int mvicp_recompute_normals(mvicp_ctx* c, int frame, int k, double* nrm_out, int* knn_out) try {
  MV_CHECK(bind(c));
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range", frame); return MVICP_ERR_ARG; }
  MV_CHECK(finish_builds(c));
  FrameDev& f = c->frames[frame];
  if (f.n < k) { set_error("frame %d has %d points < k = %d (common.h:333 asserts >= 3)", frame, f.n, k); return MVICP_ERR_STATE; }
  // launch_normals' own conditions, decided before anything is allocated: a refused call must not leave a frame without normals holding
  // normal buffers nobody has written (check_evaluable and the gather take a non-null snor for "this frame has normals")
  if (k < 3 || k > 16) { set_error("k = %d outside [3, 16]", k); return MVICP_ERR_ARG; }
  if (!f.has_grid) { set_error("frame %d: normals need the per-cloud hash structure", frame); return MVICP_ERR_STATE; }
  const bool fresh_nor = !f.nor, fresh_snor = !f.grid.snor;
  int* d_knn = nullptr;
  int st = MVICP_OK;
  if (fresh_nor) st = dev_alloc(&f.nor, 3 * (size_t)f.n);
  if (st == MVICP_OK && fresh_snor) st = dev_alloc(&f.grid.snor, 3 * (size_t)f.n);
  if (st == MVICP_OK && knn_out) st = dev_alloc(&d_knn, (size_t)f.n * k);
  if (st == MVICP_OK) st = launch_normals(c, f, k, d_knn);
  if (st == MVICP_OK) {
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess && nrm_out) e = hipMemcpy(nrm_out, f.nor, sizeof(double) * 3 * (size_t)f.n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && knn_out) e = hipMemcpy(knn_out, d_knn, sizeof(int) * (size_t)f.n * k, hipMemcpyDeviceToHost);
    if (e != hipSuccess) { set_error("recompute_normals: %s", hipGetErrorString(e)); st = MVICP_ERR_HIP; }
  }
  dev_free(d_knn);
  if (st != MVICP_OK) {   // what this call allocated goes with it: the frame has normals only if a call computed them
    (void)hipStreamSynchronize(c->stream);
    if (fresh_nor) dev_free(f.nor);
    if (fresh_snor) dev_free(f.grid.snor);
  }
  return normals_changed(c, frame, st);
} MVICP_GUARD_ABI

int mvicp_set_shard(mvicp_ctx* c, int rank, int world) try {
  MV_CHECK(bind(c));
  if (world < 1 || rank < 0 || rank >= world) { set_error("bad shard %d/%d", rank, world); return MVICP_ERR_ARG; }
  if (c->E) { set_error("call mvicp_set_shard before mvicp_set_graph"); return MVICP_ERR_STATE; }
  c->rank = rank; c->world = world;
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_edge_owner(int n_edges, const int* n_src, int world, int* owner) try {
  if (n_edges < 0 || world < 1 || (n_edges > 0 && (!n_src || !owner))) { set_error("bad arguments"); return MVICP_ERR_ARG; }
  double total = 0, cum = 0;
  for (int e = 0; e < n_edges; ++e) total += n_src[e];
  for (int e = 0; e < n_edges; ++e) {
    const double n = n_src[e];
    int o = total > 0 ? (int)std::floor((cum + 0.5 * n) * world / total) : 0;
    owner[e] = std::min(std::max(o, 0), world - 1);
    cum += n;
  }
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_overlap(mvicp_ctx* c, const double* poses, float thresh, int max_samples, int* samples, int* hits, long long* sumq, int* q_exp) try {
  MV_CHECK(bind(c));
  if (!poses || !samples || !hits) { set_error("poses / samples / hits is null"); return MVICP_ERR_ARG; }
  if (!std::isfinite(thresh) || !(thresh > 0.f)) { set_error("thresh must be finite and > 0"); return MVICP_ERR_ARG; }
  const int K = c->n_frames;
  if (K <= 0) { set_error("no frames: call mvicp_set_num_frames first"); return MVICP_ERR_STATE; }
  for (size_t k = 0; k < 16 * (size_t)K; ++k)
    if (!std::isfinite(poses[k])) { set_error("non-finite pose entry (frame %d)", (int)(k / 16)); return MVICP_ERR_ARG; }
  for (int i = 0; i < K; ++i)
    if (!c->frames[i].pts) { set_error("frame %d was never uploaded", i); return MVICP_ERR_STATE; }
  MV_CHECK(finish_builds(c));
  // sqrt(d2) < thresh <=> d2 < B2; every term floor(d2 * 2^q) of sumq is then below B2 * 2^q < 2^31
  const double B2 = sqrt_bound((double)thresh);
  int ex = 0;
  (void)std::frexp(B2, &ex);   // B2 = m 2^ex, m in [0.5, 1)
  const int q = 31 - ex;
  if (q_exp) *q_exp = q;
  std::vector<double> xf(kXfRigid * (size_t)K * K, 0.0);
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j)
      if (i != j) fill_query_xf(poses + 16 * (size_t)i, poses + 16 * (size_t)j, &xf[kXfRigid * ((size_t)i * K + j)]);
  return overlap_census(c, xf.data(), B2, std::ldexp(1.0, q), max_samples, samples, hits, sumq);
} MVICP_GUARD_ABI

long long mvicp_voxel_grid(mvicp_ctx* c, int n_sel, const int* frames, const double* poses, double voxel, int* has_normals) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (!std::isfinite(voxel) || !(voxel > 0.0)) { set_error("voxel must be finite and > 0"); return MVICP_ERR_ARG; }
  if (n_sel < 0) { set_error("n_sel < 0"); return MVICP_ERR_ARG; }
  const int K = c->n_frames;
  if (K <= 0) { set_error("no frames: call mvicp_set_num_frames first"); return MVICP_ERR_STATE; }
  std::vector<int> sel;
  if (!frames) { sel.resize((size_t)K); for (int i = 0; i < K; ++i) sel[i] = i; }
  else {
    std::vector<char> seen((size_t)K, 0);
    for (int k = 0; k < n_sel; ++k) {
      const int i = frames[k];
      if (i < 0 || i >= K) { set_error("frames[%d] = %d out of range [0,%d)", k, i, K); return MVICP_ERR_ARG; }
      if (seen[i]) { set_error("frame %d is listed twice", i); return MVICP_ERR_ARG; }
      seen[i] = 1;
      sel.push_back(i);
    }
  }
  if (poses)
    for (size_t k = 0; k < 16 * (size_t)K; ++k)
      if (!std::isfinite(poses[k])) { set_error("non-finite pose entry (frame %d)", (int)(k / 16)); return MVICP_ERR_ARG; }
  long long total = 0;
  for (int i : sel) {
    if (!c->frames[i].pts) { set_error("frame %d was never uploaded", i); return MVICP_ERR_STATE; }
    total += c->frames[i].n;
  }
  if (total >= (1ll << 31)) { set_error("%lld input points: the voxel grid takes fewer than 2^31", total); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  return voxel_reduce(c, (int)sel.size(), sel.data(), poses, voxel, has_normals);
} MVICP_GUARD_ABI

// where a destination of mvicp_voxel_fetch lives: 1 = device memory of the context's device, 0 = host memory; another device's memory is MVICP_ERR_ARG
static int destination_kind(mvicp_ctx* c, const void* p, const char* what) {
  hipPointerAttribute_t at;
  std::memset(&at, 0, sizeof(at));
  const hipError_t e = hipPointerGetAttributes(&at, p);
  if (e != hipSuccess) { (void)hipGetLastError(); return 0; }   // (a pointer the runtime does not know: plain host memory)
  if (at.type != hipMemoryTypeDevice) return 0;
  if (at.device != c->device) { set_error("%s lives on device %d, the context on device %d", what, at.device, c->device); return MVICP_ERR_ARG; }
  return 1;
}

// The tail of every fetch: each part with a destination and bytes to copy goes from the library's device memory to where its destination
// lives.  Every destination is classified before the first copy is queued, so a refused one leaves nothing copied; one wait at the end.
struct FetchPart { void* dst; const void* src; size_t bytes; const char* name; };
extern "C++" {
template <int N>
static int fetch_parts(mvicp_ctx* c, const FetchPart (&parts)[N]) {
  MV_CHECK(bind(c));
  int kind[N];
  for (int t = 0; t < N; ++t) {
    kind[t] = 0;
    if (parts[t].dst && parts[t].bytes) { kind[t] = destination_kind(c, parts[t].dst, parts[t].name); if (kind[t] < 0) return kind[t]; }
  }
  for (int t = 0; t < N; ++t)
    if (parts[t].dst && parts[t].bytes)
      MV_HIP(hipMemcpyAsync(parts[t].dst, parts[t].src, parts[t].bytes, kind[t] ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
}
}  // extern "C++"

// The kept rows of a stage's selection (the stage's own "no result" check comes first, in the caller), and in the same fetch the stage's
// per-point arrays of n rows each (`more`; at most three).  The texts that differ between the entry points: cap_name / what ("cap_kept", "kept
// rows"), select_call (what makes a selection), no_normals (the whole message).
static int fetch_kept(mvicp_ctx* c, const RowSelection& sel, long long cap, double* xyz, double* nrm, int* idx, int* label, const char* cap_name, const char* what,
                      const char* select_call, const char* no_normals, long long cap_n = 0, long long n = 0, std::initializer_list<FetchPart> more = {}) {
  if (sel.kept < 0) { set_error("no selection: call %s first", select_call); return MVICP_ERR_STATE; }
  if (cap < sel.kept) { set_error("%s %lld < %lld %s", cap_name, cap, sel.kept, what); return MVICP_ERR_ARG; }
  const size_t m = (size_t)sel.kept;
  FetchPart parts[7] = {{xyz, sel.xyz, 24 * m, "xyz"}, {nrm, sel.nrm, 24 * m, "nrm"}, {idx, sel.idx, 4 * m, "idx"}, {label, sel.klabel, 4 * m, "label"}};
  bool per_point = false;
  int t = 4;
  for (const FetchPart& p : more) { parts[t++] = p; per_point = per_point || p.dst; }
  if (per_point && cap_n < n) { set_error("cap_n %lld < %lld points", cap_n, n); return MVICP_ERR_ARG; }
  if (nrm && !sel.has_normals) { set_error("%s", no_normals); return MVICP_ERR_STATE; }
  if (m == 0 && n == 0) return MVICP_OK;
  return fetch_parts(c, parts);
}

// the frame a result of n rows was computed for is still the cloud it was computed for (an upload to it drops the result; mvicp_set_num_frames
// can take the slot away)
static bool frame_unchanged(const mvicp_ctx* c, int frame, long long n) {
  return frame >= 0 && frame < c->n_frames && c->frames[frame].n == n && (n == 0 || c->frames[frame].pts);
}

// the normals a stage reads for frame f: source 0 the frame's stored ones (`missing`: what to say when it has none), 1 the last estimate of this frame
static int normals_source(mvicp_ctx* c, int frame, const FrameDev& f, int source, const char* missing, const double** N) {
  if (source == 0) {
    if (f.n > 0 && !f.nor) { set_error("frame %d has no normals%s", frame, missing); return MVICP_ERR_STATE; }
    *N = f.nor;
  } else {
    if (c->nrm.rows < 0 || c->nrm.frame != frame || c->nrm.rows != f.n) {
      set_error("no estimated normals of frame %d: call mvicp_estimate_normals on it first (an upload to the frame drops the result)", frame);
      return MVICP_ERR_STATE;
    }
    *N = c->nrm.nrm;
  }
  return MVICP_OK;
}

int mvicp_voxel_fetch(mvicp_ctx* c, long long cap, double* xyz, double* nrm, int* cnt) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->vox.m < 0) { set_error("no voxel grid: call mvicp_voxel_grid first"); return MVICP_ERR_STATE; }
  if (cap < c->vox.m) { set_error("cap %lld < %lld voxels", cap, c->vox.m); return MVICP_ERR_ARG; }
  if (nrm && !c->vox.has_normals) { set_error("the voxel grid has no normals"); return MVICP_ERR_STATE; }
  const size_t m = (size_t)c->vox.m;
  if (m == 0) return MVICP_OK;
  const FetchPart parts[] = {{xyz, c->vox.xyz, 24 * m, "xyz"}, {nrm, c->vox.nrm, 24 * m, "nrm"}, {cnt, c->vox.cnt, 4 * m, "cnt"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_outlier_filter(mvicp_ctx* c, int frame, int k, double std_ratio, double radius, mvicp_outlier_stats* stats) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (k < 1 || k > 32) { set_error("k = %d outside [1, 32]", k); return MVICP_ERR_ARG; }
  if (!std::isfinite(std_ratio)) { set_error("std_ratio must be finite (negative: statistical rule off)"); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: radius rule off)"); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (!c->frames[frame].pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  const int n = c->frames[frame].n;
  if (n > 0 && n <= k) { set_error("frame %d has %d points: k = %d needs more than k", frame, n, k); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long kept = outlier_filter(c, c->frames[frame], k, std_ratio, radius, stats);
  if (c->profile) prof_collect_lazy(c);
  return kept;
} MVICP_GUARD_ABI

int mvicp_outlier_fetch(mvicp_ctx* c, long long cap_kept, double* xyz, double* nrm, int* idx, long long cap_n, double* mdist, double* kd2) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->out.n < 0) { set_error("no outlier result: call mvicp_outlier_filter first"); return MVICP_ERR_STATE; }
  const size_t n = (size_t)c->out.n;
  return fetch_kept(c, c->out.sel, cap_kept, xyz, nrm, idx, nullptr, "cap_kept", "kept rows", "mvicp_outlier_filter", "the filtered frame has no normals", cap_n, c->out.n,
                    {{mdist, c->out.mdist, 8 * n, "mdist"}, {kd2, c->out.kd2, 8 * n, "kd2"}});
} MVICP_GUARD_ABI

long long mvicp_cluster(mvicp_ctx* c, int frame, double radius, int min_pts, mvicp_cluster_stats* stats) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (min_pts < 1 || min_pts > (1 << 30)) { set_error("min_pts = %d outside [1, 2^30]", min_pts); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius) || !(radius > 0.0)) { set_error("radius must be finite and > 0"); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (!c->frames[frame].pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long clusters = cluster_points(c, c->frames[frame], frame, sqrt_bound(radius), min_pts, stats);
  if (c->profile) prof_collect_lazy(c);
  return clusters;
} MVICP_GUARD_ABI

int mvicp_cluster_fetch(mvicp_ctx* c, long long cap_n, int* label, unsigned char* core, long long cap_clusters, int* size) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->clu.n < 0) { set_error("no cluster result: call mvicp_cluster first"); return MVICP_ERR_STATE; }
  if ((label || core) && cap_n < c->clu.n) { set_error("cap_n %lld < %lld points", cap_n, c->clu.n); return MVICP_ERR_ARG; }
  if (size && cap_clusters < c->clu.clusters) { set_error("cap_clusters %lld < %lld clusters", cap_clusters, c->clu.clusters); return MVICP_ERR_ARG; }
  if (c->clu.n == 0) return MVICP_OK;
  const size_t n = (size_t)c->clu.n, k = (size_t)c->clu.clusters;
  const FetchPart parts[] = {{label, c->clu.label, 4 * n, "label"}, {core, c->clu.core, n, "core"}, {size, c->clu.size, 4 * k, "size"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_cluster_select(mvicp_ctx* c, long long min_size, long long max_clusters) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (min_size < 0 || max_clusters < 0) { set_error("min_size and max_clusters must be >= 0"); return MVICP_ERR_ARG; }
  if (c->clu.n < 0) { set_error("no cluster result: call mvicp_cluster first"); return MVICP_ERR_STATE; }
  const int frame = c->clu.frame;
  if (!frame_unchanged(c, frame, c->clu.n)) {
    set_error("the clustered frame is gone: call mvicp_cluster again");
    return MVICP_ERR_STATE;
  }
  MV_CHECK(bind(c));
  const long long kept = cluster_select(c, c->frames[frame], min_size, max_clusters);
  if (c->profile) prof_collect_lazy(c);
  return kept;
} MVICP_GUARD_ABI

int mvicp_cluster_fetch_kept(mvicp_ctx* c, long long cap, double* xyz, double* nrm, int* idx, int* label) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->clu.n < 0) { set_error("no cluster result: call mvicp_cluster first"); return MVICP_ERR_STATE; }
  return fetch_kept(c, c->clu.sel, cap, xyz, nrm, idx, label, "cap", "kept rows", "mvicp_cluster_select", "the clustered frame has no normals");
} MVICP_GUARD_ABI

int mvicp_segment_plane(mvicp_ctx* c, int frame, long long hypotheses, unsigned long long seed, double tau, const double* axis, double cos_min, int refine,
                        mvicp_plane_result* result) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (!result) { set_error("null result"); return MVICP_ERR_ARG; }
  if (hypotheses < 1 || hypotheses > (1ll << 24)) { set_error("hypotheses = %lld outside [1, 2^24]", hypotheses); return MVICP_ERR_ARG; }
  if (!std::isfinite(tau) || !(tau > 0.0)) { set_error("tau must be finite and > 0"); return MVICP_ERR_ARG; }
  if (axis) {
    if (!std::isfinite(axis[0]) || !std::isfinite(axis[1]) || !std::isfinite(axis[2]) || (axis[0] == 0.0 && axis[1] == 0.0 && axis[2] == 0.0)) {
      set_error("axis must be finite and not all zero");
      return MVICP_ERR_ARG;
    }
    if (!(cos_min >= 0.0 && cos_min <= 1.0)) { set_error("cos_min must lie in [0, 1]"); return MVICP_ERR_ARG; }
  }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (!c->frames[frame].pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  const int st = plane_segment(c, c->frames[frame], frame, hypotheses, seed, tau, axis, cos_min, refine, result);
  if (c->profile) prof_collect_lazy(c);
  return st;
} MVICP_GUARD_ABI

int mvicp_plane_fetch(mvicp_ctx* c, long long cap_h, int* count, long long cap_n, unsigned char* flags) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->plane.n < 0) { set_error("no plane result: call mvicp_segment_plane first"); return MVICP_ERR_STATE; }
  if (count && cap_h < c->plane.H) { set_error("cap_h %lld < %lld hypotheses", cap_h, c->plane.H); return MVICP_ERR_ARG; }
  if (flags && cap_n < c->plane.n) { set_error("cap_n %lld < %lld points", cap_n, c->plane.n); return MVICP_ERR_ARG; }
  const FetchPart parts[] = {{count, c->plane.count, 4 * (size_t)c->plane.H, "count"}, {flags, c->plane.n ? c->plane.flags : nullptr, (size_t)c->plane.n, "flags"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_plane_select(mvicp_ctx* c, int inliers) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->plane.n < 0) { set_error("no plane result: call mvicp_segment_plane first"); return MVICP_ERR_STATE; }
  const int frame = c->plane.frame;
  if (!frame_unchanged(c, frame, c->plane.n)) {
    set_error("the segmented frame is gone: call mvicp_segment_plane again");
    return MVICP_ERR_STATE;
  }
  MV_CHECK(bind(c));
  const long long kept = plane_select(c, c->frames[frame], inliers);
  if (c->profile) prof_collect_lazy(c);
  return kept;
} MVICP_GUARD_ABI

int mvicp_plane_fetch_kept(mvicp_ctx* c, long long cap, double* xyz, double* nrm, int* idx) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->plane.n < 0) { set_error("no plane result: call mvicp_segment_plane first"); return MVICP_ERR_STATE; }
  return fetch_kept(c, c->plane.sel, cap, xyz, nrm, idx, nullptr, "cap", "kept rows", "mvicp_plane_select", "the segmented frame has no normals");
} MVICP_GUARD_ABI

long long mvicp_boundary(mvicp_ctx* c, int frame, int source, int max_nn, double radius, double cos_gap) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (source != 0 && source != 1) { set_error("source = %d: 0 (the frame's stored normals) or 1 (the last mvicp_estimate_normals / mvicp_fit_normals)", source); return MVICP_ERR_ARG; }
  if (max_nn < 3 || max_nn > 64) { set_error("max_nn = %d outside [3, 64]", max_nn); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: no radius)"); return MVICP_ERR_ARG; }
  if (!(cos_gap > -1.0 && cos_gap < 1.0)) { set_error("cos_gap must lie in (-1, 1)"); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  const double* N = nullptr;
  MV_CHECK(normals_source(c, frame, f, source, "", &N));
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long flagged = boundary_points(c, f, frame, N, max_nn, radius, radius > 0.0 ? sqrt_bound(radius) : 0.0, cos_gap);
  if (c->profile) prof_collect_lazy(c);
  return flagged;
} MVICP_GUARD_ABI

int mvicp_boundary_fetch(mvicp_ctx* c, long long cap_rows, unsigned char* flag, int* open, int* valid, int* used) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->bnd.n < 0) { set_error("no boundary result: call mvicp_boundary first"); return MVICP_ERR_STATE; }
  if (cap_rows < c->bnd.n) { set_error("cap_rows %lld < %lld rows", cap_rows, c->bnd.n); return MVICP_ERR_ARG; }
  if (c->bnd.n == 0) return MVICP_OK;
  const size_t n = (size_t)c->bnd.n;
  const FetchPart parts[] = {{flag, c->bnd.flag, n, "flag"}, {open, c->bnd.open, 4 * n, "open"}, {valid, c->bnd.valid, 4 * n, "valid"}, {used, c->bnd.used, 4 * n, "used"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_boundary_select(mvicp_ctx* c, int boundary) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->bnd.n < 0) { set_error("no boundary result: call mvicp_boundary first"); return MVICP_ERR_STATE; }
  const int frame = c->bnd.frame;
  if (!frame_unchanged(c, frame, c->bnd.n)) {
    set_error("the frame of the boundary result is gone: call mvicp_boundary again");
    return MVICP_ERR_STATE;
  }
  MV_CHECK(bind(c));
  const long long kept = boundary_select(c, c->frames[frame], boundary);
  if (c->profile) prof_collect_lazy(c);
  return kept;
} MVICP_GUARD_ABI

int mvicp_boundary_fetch_kept(mvicp_ctx* c, long long cap, double* xyz, double* nrm, int* idx) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->bnd.n < 0) { set_error("no boundary result: call mvicp_boundary first"); return MVICP_ERR_STATE; }
  return fetch_kept(c, c->bnd.sel, cap, xyz, nrm, idx, nullptr, "cap", "kept rows", "mvicp_boundary_select", "the frame of the boundary result has no normals");
} MVICP_GUARD_ABI

// What follows a new, changed or cleared reject mask of `frame`; roles = the old and the new roles together.  Modelled on normals_changed:
// queued evaluations are void, and every owned edge the mask bears on loses its list (list_valid: the next search re-compacts and re-gathers
// it, so nothing_can_change / sel_skip cannot hold) and its "this is last search's result" mark (qpos_valid: the edge gets a new epoch
// then).  The temporal NN cache -- seeds, bounds, nn_cache_valid, nn_cache_edge -- is a fact about nearest neighbours and stays.
static void reject_mask_changed(mvicp_ctx* c, int frame, int roles) {
  c->spec_ready = false; c->spec2_ready = false;
  for (int e = 0; e < c->E; ++e) {
    if (!c->owned[e]) continue;
    if (((roles & MVICP_REJECT_AS_TARGET) && c->edst[e] == frame) || ((roles & MVICP_REJECT_AS_SOURCE) && c->esrc[e] == frame)) {
      c->hist.list_valid[e] = 0; c->hist.qpos_valid[e] = 0;
    }
  }
}

// `src` (f.n bytes in device memory of this context, or host memory when !on_device) becomes the mask of `frame` in `roles` (1..3).  The
// checks are the callers'; a failure after the first write leaves the frame without a mask.
static int install_reject_mask(mvicp_ctx* c, int frame, const unsigned char* src, bool on_device, int roles) {
  FrameDev& f = c->frames[frame];
  const int old_roles = f.grid.mask_roles;
  MV_HIP(hipStreamSynchronize(c->stream));   // (a search in flight may still read the old bytes)
  int st = MVICP_OK;
  if (!f.grid.omask) st = dev_alloc(&f.grid.omask, (size_t)f.n);
  if (st == MVICP_OK && !f.grid.smask) st = dev_alloc(&f.grid.smask, (size_t)f.n);
  if (st == MVICP_OK && f.n > 0) {
    f.grid.mask_roles = 0;
    hipError_t e = hipMemcpyAsync(f.grid.omask, src, (size_t)f.n, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) { st = launch_mask_permute(c, f); if (st == MVICP_OK) e = hipStreamSynchronize(c->stream); }
    if (e != hipSuccess) { set_error("reject mask of frame %d: %s", frame, hipGetErrorString(e)); st = MVICP_ERR_HIP; }
  }
  if (st == MVICP_OK) f.grid.mask_roles = roles;
  reject_mask_changed(c, frame, old_roles | f.grid.mask_roles);
  if (c->profile) prof_collect_lazy(c);
  return st;
}

static int clear_reject_mask(mvicp_ctx* c, int frame) {
  FrameDev& f = c->frames[frame];
  const int old_roles = f.grid.mask_roles;
  if (old_roles == 0) return MVICP_OK;   // (nothing set: nothing changes)
  MV_CHECK(bind(c));
  MV_HIP(hipStreamSynchronize(c->stream));
  f.grid.mask_roles = 0;   // (the buffers stay for the next mask of this cloud)
  reject_mask_changed(c, frame, old_roles);
  return MVICP_OK;
}

int mvicp_set_reject_mask(mvicp_ctx* c, int frame, const unsigned char* mask, int roles) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (roles < 0 || roles > 3) { set_error("roles = %d outside [0, 3] (MVICP_REJECT_AS_TARGET | MVICP_REJECT_AS_SOURCE)", roles); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (!mask || roles == 0) return clear_reject_mask(c, frame);
  FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  if (f.n > 0 && !f.has_grid) { set_error("frame %d: a reject mask needs the per-cloud structure", frame); return MVICP_ERR_STATE; }
  const int kind = f.n > 0 ? destination_kind(c, mask, "mask") : 0;
  if (kind < 0) return kind;
  return install_reject_mask(c, frame, mask, kind == 1, roles);
} MVICP_GUARD_ABI

int mvicp_boundary_adopt(mvicp_ctx* c, int roles) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (roles < 0 || roles > 3) { set_error("roles = %d outside [0, 3] (MVICP_REJECT_AS_TARGET | MVICP_REJECT_AS_SOURCE)", roles); return MVICP_ERR_ARG; }
  const int frame = c->bnd.frame;
  if (c->bnd.n < 0 || !frame_unchanged(c, frame, c->bnd.n)) {
    set_error("no boundary result to adopt: call mvicp_boundary first (an upload to its frame drops the result)");
    return MVICP_ERR_STATE;
  }
  if (roles == 0) return clear_reject_mask(c, frame);
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  if (c->bnd.n > 0 && !c->frames[frame].has_grid) { set_error("frame %d: a reject mask needs the per-cloud structure", frame); return MVICP_ERR_STATE; }
  return install_reject_mask(c, frame, c->bnd.flag, true, roles);
} MVICP_GUARD_ABI

long long mvicp_get_reject_mask(mvicp_ctx* c, int frame, unsigned char* out, long long cap, int* roles) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (f.grid.mask_roles == 0) { if (roles) *roles = 0; return 0; }
  if (out && cap < f.n) { set_error("cap %lld < %d bytes", cap, f.n); return MVICP_ERR_ARG; }
  if (out && f.n > 0) {
    const FetchPart parts[] = {{out, f.grid.omask, (size_t)f.n, "mask"}};
    MV_CHECK(fetch_parts(c, parts));
  }
  if (roles) *roles = f.grid.mask_roles;
  return f.n;
} MVICP_GUARD_ABI

long long mvicp_knn_search(mvicp_ctx* c, int frame, const double* queries, long long m, int k, double radius) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (k < 0 || k > 64) { set_error("k = %d outside [0, 64]", k); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: no radius)"); return MVICP_ERR_ARG; }
  if (k == 0 && !(radius > 0.0)) { set_error("k = 0 (every neighbour within the radius) needs radius > 0"); return MVICP_ERR_ARG; }
  if (queries && (m < 0 || m >= (1ll << 31))) { set_error("m = %lld outside [0, 2^31)", m); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  if (!c->frames[frame].pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  int on_device = 0;
  if (queries && m > 0) { on_device = destination_kind(c, queries, "queries"); if (on_device < 0) return on_device; }
  MV_CHECK(finish_builds(c));
  const long long total = knn_search(c, c->frames[frame], queries, on_device, m, k, radius, radius > 0.0 ? sqrt_bound(radius) : 0.0);
  if (c->profile) prof_collect_lazy(c);
  return total;
} MVICP_GUARD_ABI

int mvicp_knn_fetch(mvicp_ctx* c, long long cap_rows, long long cap_entries, int* cnt, long long* off, int* idx, double* d2) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->knn.m < 0) { set_error("no neighbour search result: call mvicp_knn_search first"); return MVICP_ERR_STATE; }
  const long long entries = c->knn.k ? c->knn.m * c->knn.k : c->knn.total;
  if ((cnt || off) && cap_rows < c->knn.m) { set_error("cap_rows %lld < %lld rows", cap_rows, c->knn.m); return MVICP_ERR_ARG; }
  if ((idx || d2) && cap_entries < entries) { set_error("cap_entries %lld < %lld entries", cap_entries, entries); return MVICP_ERR_ARG; }
  const size_t m = (size_t)c->knn.m, e = (size_t)entries;
  const FetchPart parts[] = {{cnt, c->knn.cnt, 4 * m, "cnt"}, {off, c->knn.off, 8 * (m + 1), "off"}, {idx, c->knn.idx, 4 * e, "idx"}, {d2, c->knn.d2, 8 * e, "d2"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_fpfh(mvicp_ctx* c, int frame, double radius, int max_nn) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (max_nn < 2 || max_nn > 64) { set_error("max_nn = %d outside [2, 64]", max_nn); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius) || !(radius > 0.0)) { set_error("radius must be finite and > 0"); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  if (f.n > 0 && !f.nor) { set_error("frame %d has no normals: the descriptors need them", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long rows = fpfh_compute(c, f, max_nn, radius, sqrt_bound(radius));
  if (c->profile) prof_collect_lazy(c);
  return rows;
} MVICP_GUARD_ABI

int mvicp_fpfh_fetch(mvicp_ctx* c, long long cap_rows, double* desc, int* used) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->fpfh.rows < 0) { set_error("no descriptors: call mvicp_fpfh first"); return MVICP_ERR_STATE; }
  if (cap_rows < c->fpfh.rows) { set_error("cap_rows %lld < %lld rows", cap_rows, c->fpfh.rows); return MVICP_ERR_ARG; }
  if (c->fpfh.rows == 0) return MVICP_OK;
  const size_t n = (size_t)c->fpfh.rows;
  const FetchPart parts[] = {{desc, c->fpfh.desc, 33 * 8 * n, "desc"}, {used, c->fpfh.used, 4 * n, "used"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_estimate_normals(mvicp_ctx* c, int frame, int max_nn, double radius, const double* viewpoint) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (max_nn < 3 || max_nn > 64) { set_error("max_nn = %d outside [3, 64]", max_nn); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: no radius)"); return MVICP_ERR_ARG; }
  double vp[3] = {0.0, 0.0, 0.0};
  for (int a = 0; viewpoint && a < 3; ++a) {
    if (!std::isfinite(viewpoint[a])) { set_error("viewpoint[%d] is not finite", a); return MVICP_ERR_ARG; }
    vp[a] = viewpoint[a];
  }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long rows = normals_estimate(c, f, max_nn, radius, radius > 0.0 ? sqrt_bound(radius) : 0.0, vp);
  if (rows >= 0) c->nrm.frame = frame;
  if (c->profile) prof_collect_lazy(c);
  return rows;
} MVICP_GUARD_ABI

long long mvicp_fit_normals(mvicp_ctx* c, int frame, int max_nn, double radius, const double* viewpoint, int degree) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (max_nn < 3 || max_nn > 64) { set_error("max_nn = %d outside [3, 64]", max_nn); return MVICP_ERR_ARG; }
  if (degree != 2 && degree != 3) { set_error("degree = %d: 2 or 3", degree); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: no radius)"); return MVICP_ERR_ARG; }
  double vp[3] = {0.0, 0.0, 0.0};
  for (int a = 0; viewpoint && a < 3; ++a) {
    if (!std::isfinite(viewpoint[a])) { set_error("viewpoint[%d] is not finite", a); return MVICP_ERR_ARG; }
    vp[a] = viewpoint[a];
  }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long rows = normals_fit(c, f, max_nn, radius, radius > 0.0 ? sqrt_bound(radius) : 0.0, vp, degree);
  if (rows >= 0) c->nrm.frame = frame;
  if (c->profile) prof_collect_lazy(c);
  return rows;
} MVICP_GUARD_ABI

int mvicp_normals_fit_fetch(mvicp_ctx* c, long long cap_rows, unsigned char* fitted) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->nrm.rows < 0 || !c->nrm.has_fit) { set_error("no fitted normals: the last estimate was not mvicp_fit_normals"); return MVICP_ERR_STATE; }
  if (cap_rows < c->nrm.rows) { set_error("cap_rows %lld < %lld rows", cap_rows, c->nrm.rows); return MVICP_ERR_ARG; }
  if (c->nrm.rows == 0) return MVICP_OK;
  const FetchPart parts[] = {{fitted, c->nrm.fitted, (size_t)c->nrm.rows, "fitted"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_smooth_points(mvicp_ctx* c, int frame, int max_nn, double radius, const double* viewpoint, int degree, double max_shift) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (max_nn < 3 || max_nn > 64) { set_error("max_nn = %d outside [3, 64]", max_nn); return MVICP_ERR_ARG; }
  if (degree != 2 && degree != 3) { set_error("degree = %d: 2 or 3", degree); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: no radius)"); return MVICP_ERR_ARG; }
  if (std::isnan(max_shift)) { set_error("max_shift is a NaN (<= 0: no limit)"); return MVICP_ERR_ARG; }
  double vp[3] = {0.0, 0.0, 0.0};
  for (int a = 0; viewpoint && a < 3; ++a) {
    if (!std::isfinite(viewpoint[a])) { set_error("viewpoint[%d] is not finite", a); return MVICP_ERR_ARG; }
    vp[a] = viewpoint[a];
  }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long rows = smooth_points(c, f, max_nn, radius, radius > 0.0 ? sqrt_bound(radius) : 0.0, vp, degree, max_shift);
  if (rows >= 0) c->nrm.frame = frame;
  if (c->profile) prof_collect_lazy(c);
  return rows;
} MVICP_GUARD_ABI

int mvicp_smooth_fetch(mvicp_ctx* c, long long cap_rows, double* xyz, double* shift, unsigned char* moved, double* H, double* K) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->nrm.rows < 0 || !c->nrm.has_smooth) { set_error("no smoothed points: the last estimate was not mvicp_smooth_points"); return MVICP_ERR_STATE; }
  if (cap_rows < c->nrm.rows) { set_error("cap_rows %lld < %lld rows", cap_rows, c->nrm.rows); return MVICP_ERR_ARG; }
  if (c->nrm.rows == 0) return MVICP_OK;
  const size_t n = (size_t)c->nrm.rows;
  const FetchPart parts[] = {{xyz, c->nrm.xyz, 24 * n, "xyz"}, {shift, c->nrm.shift, 8 * n, "shift"}, {moved, c->nrm.moved, n, "moved"},
                             {H, c->nrm.H, 8 * n, "H"}, {K, c->nrm.K, 8 * n, "K"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

int mvicp_normals_fetch(mvicp_ctx* c, long long cap_rows, double* nrm, double* curvature, int* used) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->nrm.rows < 0) { set_error("no estimated normals: call mvicp_estimate_normals first"); return MVICP_ERR_STATE; }
  if (cap_rows < c->nrm.rows) { set_error("cap_rows %lld < %lld rows", cap_rows, c->nrm.rows); return MVICP_ERR_ARG; }
  if (c->nrm.rows == 0) return MVICP_OK;
  const size_t n = (size_t)c->nrm.rows;
  const FetchPart parts[] = {{nrm, c->nrm.nrm, 24 * n, "nrm"}, {curvature, c->nrm.curv, 8 * n, "curvature"}, {used, c->nrm.used, 4 * n, "used"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

// The shared part of mvicp_normals_adopt and mvicp_orient_adopt: `nrm` (rows x 3 doubles in library-owned device memory, computed for
// `frame`) becomes the frame's normals, as a successful mvicp_recompute_normals would leave them.
static int adopt_normals_into(mvicp_ctx* c, int frame, long long rows, const double* nrm, const char* what) {
  FrameDev& f = c->frames[frame];
  if (rows != f.n) { set_error("the %s normals have %lld rows, frame %d has %d points", what, rows, frame, f.n); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  if (f.n == 0) return MVICP_OK;   // (nothing to write)
  if (!f.has_grid) { set_error("frame %d: adopting normals needs the per-cloud hash structure", frame); return MVICP_ERR_STATE; }
  const bool fresh_nor = !f.nor, fresh_snor = !f.grid.snor;
  int st = MVICP_OK;
  if (fresh_nor) st = dev_alloc(&f.nor, 3 * (size_t)f.n);
  if (st == MVICP_OK && fresh_snor) st = dev_alloc(&f.grid.snor, 3 * (size_t)f.n);
  if (st == MVICP_OK) st = normals_adopt(c, f, nrm);
  if (st != MVICP_OK) {   // what this call allocated goes with it: the frame has normals only if a call wrote them
    (void)hipStreamSynchronize(c->stream);
    if (fresh_nor) dev_free(f.nor);
    if (fresh_snor) dev_free(f.grid.snor);
  }
  return normals_changed(c, frame, st);
}

int mvicp_normals_adopt(mvicp_ctx* c) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->nrm.rows < 0 || c->nrm.frame < 0 || c->nrm.frame >= c->n_frames) {
    set_error("no estimated normals to adopt: call mvicp_estimate_normals first (an upload to its frame drops the result)");
    return MVICP_ERR_STATE;
  }
  return adopt_normals_into(c, c->nrm.frame, c->nrm.rows, c->nrm.nrm, "estimated");
} MVICP_GUARD_ABI

long long mvicp_orient_normals(mvicp_ctx* c, int frame, int source, int k, double radius, int mode, const double* ref3) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (source != 0 && source != 1) { set_error("source = %d: 0 (the frame's stored normals) or 1 (the last mvicp_estimate_normals)", source); return MVICP_ERR_ARG; }
  if (k < 2 || k > 64) { set_error("k = %d outside [2, 64]", k); return MVICP_ERR_ARG; }
  if (mode < MVICP_ORIENT_ANCHOR || mode > MVICP_ORIENT_DIRECTION) { set_error("mode = %d outside mvicp_orient_mode", mode); return MVICP_ERR_ARG; }
  if (!std::isfinite(radius)) { set_error("radius must be finite (<= 0: no radius)"); return MVICP_ERR_ARG; }
  if (!ref3 && mode == MVICP_ORIENT_DIRECTION) { set_error("MVICP_ORIENT_DIRECTION needs a direction"); return MVICP_ERR_ARG; }
  double ref[3] = {0.0, 0.0, 0.0};
  for (int a = 0; ref3 && a < 3; ++a) {
    if (!std::isfinite(ref3[a])) { set_error("ref[%d] is not finite", a); return MVICP_ERR_ARG; }
    ref[a] = ref3[a];
  }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  const double* N = nullptr;
  MV_CHECK(normals_source(c, frame, f, source, " to orient", &N));
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  const long long comps = orient_normals(c, f, N, k, radius, radius > 0.0 ? sqrt_bound(radius) : 0.0, mode, ref);
  if (comps >= 0) c->ori.frame = frame;
  if (c->profile) prof_collect_lazy(c);
  return comps;
} MVICP_GUARD_ABI

int mvicp_orient_fetch(mvicp_ctx* c, long long cap_rows, double* nrm, unsigned char* flip, int* comp) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->ori.rows < 0) { set_error("no oriented normals: call mvicp_orient_normals first"); return MVICP_ERR_STATE; }
  if (cap_rows < c->ori.rows) { set_error("cap_rows %lld < %lld rows", cap_rows, c->ori.rows); return MVICP_ERR_ARG; }
  if (c->ori.rows == 0) return MVICP_OK;
  const size_t n = (size_t)c->ori.rows;
  const FetchPart parts[] = {{nrm, c->ori.nrm, 24 * n, "nrm"}, {flip, c->ori.flip, n, "flip"}, {comp, c->ori.comp, 4 * n, "comp"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

int mvicp_orient_adopt(mvicp_ctx* c) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->ori.rows < 0 || c->ori.frame < 0 || c->ori.frame >= c->n_frames) {
    set_error("no oriented normals to adopt: call mvicp_orient_normals first (an upload to its frame drops the result)");
    return MVICP_ERR_STATE;
  }
  return adopt_normals_into(c, c->ori.frame, c->ori.rows, c->ori.nrm, "oriented");
} MVICP_GUARD_ABI

int mvicp_negate_normals(mvicp_ctx* c, int frame) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  if (f.n > 0 && !f.nor) { set_error("frame %d has no normals to negate", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  if (f.n == 0) return MVICP_OK;   // (nothing to write)
  if (!f.grid.snor) { set_error("frame %d: negating normals needs the per-cloud hash structure", frame); return MVICP_ERR_STATE; }
  return normals_changed(c, frame, negate_normals(c, f));
} MVICP_GUARD_ABI

int mvicp_normal_agreement(mvicp_ctx* c, const double* poses, int* pos, int* neg) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (!poses) { set_error("poses is null"); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  MV_CHECK(check_evaluable(c, MVICP_METRIC_SYMMETRIC));
  std::vector<char> use((size_t)c->E, 0);
  for (int e = 0; e < c->E; ++e) use[e] = c->owned[e] && c->hist.h_count[e] > 0 && !((int)c->src_fixed.size() == c->E && c->src_fixed[e]);
  const int st = normal_agreement(c, poses, use.data(), pos, neg);
  if (c->profile) prof_collect_lazy(c);
  return st;
} MVICP_GUARD_ABI

int mvicp_signs_from_agreement(int n_frames, int n_edges, const int* src, const int* dst, const int* pos, const int* neg, int min_count,
                               unsigned char* flip, int* component) try {
  if (!flip || n_frames < 1 || n_edges < 0 || min_count < 0 || (n_edges > 0 && (!src || !dst || !pos || !neg))) { set_error("bad arguments"); return MVICP_ERR_ARG; }
  for (int e = 0; e < n_edges; ++e) {
    if (src[e] < 0 || src[e] >= n_frames || dst[e] < 0 || dst[e] >= n_frames || src[e] == dst[e]) { set_error("edge %d: bad frame indices", e); return MVICP_ERR_ARG; }
    if (pos[e] < 0 || neg[e] < 0) { set_error("edge %d: a negative count", e); return MVICP_ERR_ARG; }
  }
  std::vector<int> order;
  for (int e = 0; e < n_edges; ++e)
    if ((long long)pos[e] + neg[e] >= min_count && pos[e] != neg[e]) order.push_back(e);
  auto margin = [&](int e) { return std::llabs((long long)pos[e] - neg[e]); };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return margin(a) > margin(b); });   // (stable: e ascending among equals)
  // Kruskal with a weighted union-find: par[f] = (parent, parity to it); the lower index is always the root, so a root is its tree's anchor
  std::vector<int> par((size_t)n_frames), px((size_t)n_frames, 0);
  for (int i = 0; i < n_frames; ++i) par[i] = i;
  auto find = [&](int i, int* parity) { int x = 0; while (par[i] != i) { x ^= px[i]; i = par[i]; } *parity = x; return i; };
  for (int e : order) {
    int xa = 0, xb = 0;
    const int ra = find(src[e], &xa), rb = find(dst[e], &xb);
    if (ra == rb) continue;
    const int f = pos[e] < neg[e] ? 1 : 0;
    const int lo = std::min(ra, rb), hi = std::max(ra, rb);
    par[hi] = lo; px[hi] = xa ^ xb ^ f;
  }
  int comps = 0;
  for (int i = 0; i < n_frames; ++i) {
    int x = 0;
    const int r = find(i, &x);
    flip[i] = (unsigned char)x;
    if (component) component[i] = r;
    if (r == i) ++comps;
  }
  return comps;
} MVICP_GUARD_ABI

long long mvicp_iss_keypoints(mvicp_ctx* c, int frame, double salient_radius, double non_max_radius, double gamma21, double gamma32, int min_neighbors) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  const double r_lo = std::ldexp(1.0, -300), r_hi = std::ldexp(1.0, 300);
  if (!std::isfinite(salient_radius) || !(salient_radius >= r_lo && salient_radius <= r_hi)) { set_error("salient_radius must be finite and lie in [2^-300, 2^300]"); return MVICP_ERR_ARG; }
  if (!std::isfinite(non_max_radius) || !(non_max_radius >= r_lo && non_max_radius <= r_hi)) { set_error("non_max_radius must be finite and lie in [2^-300, 2^300]"); return MVICP_ERR_ARG; }
  if (!std::isfinite(gamma21) || !(gamma21 > 0.0)) { set_error("gamma21 must be finite and > 0"); return MVICP_ERR_ARG; }
  if (!std::isfinite(gamma32) || !(gamma32 > 0.0)) { set_error("gamma32 must be finite and > 0"); return MVICP_ERR_ARG; }
  if (min_neighbors < 1 || min_neighbors > 1024) { set_error("min_neighbors = %d outside [1, 1024]", min_neighbors); return MVICP_ERR_ARG; }
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range [0,%d)", frame, c->n_frames); return MVICP_ERR_ARG; }
  const FrameDev& f = c->frames[frame];
  if (!f.pts) { set_error("frame %d was never uploaded", frame); return MVICP_ERR_STATE; }
  MV_CHECK(bind(c));
  MV_CHECK(finish_builds(c));
  int e = 0;
  (void)std::frexp(salient_radius, &e);   // salient_radius = f 2^e, f in [0.5, 1)
  const long long k = iss_keypoints(c, f, sqrt_bound(salient_radius), sqrt_bound(non_max_radius), 20 - e, gamma21, gamma32, min_neighbors);
  if (c->profile) prof_collect_lazy(c);
  return k;
} MVICP_GUARD_ABI

int mvicp_iss_fetch(mvicp_ctx* c, long long cap_keys, int* idx, double* xyz, double* nrm, long long cap_n, double* saliency, int* cnt_salient, int* cnt_nms) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->iss.n < 0) { set_error("no keypoints: call mvicp_iss_keypoints first"); return MVICP_ERR_STATE; }
  const size_t n = (size_t)c->iss.n;
  // (cap_keys counts only when a keypoint array is asked for)
  return fetch_kept(c, c->iss.sel, (idx || xyz || nrm) ? cap_keys : c->iss.sel.kept, xyz, nrm, idx, nullptr, "cap_keys", "keypoints", "mvicp_iss_keypoints",
                    "the frame of the keypoints has no normals", cap_n, c->iss.n,
                    {{saliency, c->iss.sal, 8 * n, "saliency"}, {cnt_salient, c->iss.cnt_s, 4 * n, "cnt_salient"}, {cnt_nms, c->iss.cnt_n, 4 * n, "cnt_nms"}});
} MVICP_GUARD_ABI

long long mvicp_feature_match(mvicp_ctx* c, const double* a, long long m, const double* b, long long n, int dim) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (dim < 1 || dim > 64) { set_error("dim = %d outside [1, 64]", dim); return MVICP_ERR_ARG; }
  if (m < 0 || m >= (1ll << 31) || n < 0 || n >= (1ll << 31)) { set_error("m = %lld, n = %lld outside [0, 2^31)", m, n); return MVICP_ERR_ARG; }
  if ((m > 0 && !a) || (n > 0 && !b)) { set_error("null descriptors"); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  int a_dev = 0, b_dev = 0;
  if (m > 0) { a_dev = destination_kind(c, a, "a"); if (a_dev < 0) return a_dev; }
  if (n > 0) { b_dev = destination_kind(c, b, "b"); if (b_dev < 0) return b_dev; }
  const long long rows = feature_match(c, a, a_dev, m, b, b_dev, n, dim);
  if (c->profile) prof_collect_lazy(c);
  return rows;
} MVICP_GUARD_ABI

int mvicp_feature_match_fetch(mvicp_ctx* c, long long cap_m, long long cap_n, int* fwd_idx, double* fwd_d2, int* bwd_idx, double* bwd_d2) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->match.m < 0) { set_error("no matches: call mvicp_feature_match first"); return MVICP_ERR_STATE; }
  if ((fwd_idx || fwd_d2) && cap_m < c->match.m) { set_error("cap_m %lld < %lld rows", cap_m, c->match.m); return MVICP_ERR_ARG; }
  if ((bwd_idx || bwd_d2) && cap_n < c->match.n) { set_error("cap_n %lld < %lld rows", cap_n, c->match.n); return MVICP_ERR_ARG; }
  const size_t m = (size_t)c->match.m, n = (size_t)c->match.n;
  const FetchPart parts[] = {{fwd_idx, c->match.fwd_idx, 8 * m, "fwd_idx"}, {fwd_d2, c->match.fwd_d2, 16 * m, "fwd_d2"},
                             {bwd_idx, c->match.bwd_idx, 8 * n, "bwd_idx"}, {bwd_d2, c->match.bwd_d2, 16 * n, "bwd_d2"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_match_pairs(long long m, long long n, const int* fwd_idx, const double* fwd_d2, const int* bwd_idx, int mutual, double ratio,
                            int* pairs) try {
  if (m < 0 || n < 0 || !fwd_idx || !fwd_d2 || !bwd_idx || !pairs) { set_error("match pairs: needs m, n >= 0 and four arrays"); return MVICP_ERR_ARG; }
  if (!(ratio > 0.0)) { set_error("match pairs: ratio must be > 0"); return MVICP_ERR_ARG; }
  // (this TU is built without fma contraction: the product of the ratio test is rounded on its own)
  const double r2 = ratio * ratio;
  long long k = 0;
  for (long long i = 0; i < m; ++i) {
    const long long j = fwd_idx[2 * i];
    if (j < 0) continue;
    if (j >= n) { set_error("match pairs: fwd_idx[%lld][0] = %lld with n = %lld", i, j, n); return MVICP_ERR_ARG; }
    if (mutual && (long long)bwd_idx[2 * j] != i) continue;
    if (!(ratio >= 1.0) && !(fwd_d2[2 * i] <= r2 * fwd_d2[2 * i + 1])) continue;
    pairs[2 * k] = (int)i; pairs[2 * k + 1] = (int)j;
    ++k;
  }
  return k;
} MVICP_GUARD_ABI

int mvicp_consensus(mvicp_ctx* c, const double* p, const double* q, long long n_pairs, long long hypotheses, unsigned long long seed, double tau,
                    double edge_sim, mvicp_consensus_result* result) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (n_pairs < 3 || n_pairs >= (1ll << 31)) { set_error("%lld pairs outside [3, 2^31)", n_pairs); return MVICP_ERR_ARG; }
  if (hypotheses < 1 || hypotheses > (1ll << 24)) { set_error("%lld hypotheses outside [1, 2^24]", hypotheses); return MVICP_ERR_ARG; }
  if (!std::isfinite(tau) || !(tau > 0.0)) { set_error("tau must be finite and > 0"); return MVICP_ERR_ARG; }
  if (!(edge_sim >= 0.0 && edge_sim < 1.0)) { set_error("edge_sim must be in [0, 1)"); return MVICP_ERR_ARG; }
  if (!p || !q) { set_error("null pairs"); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  const int p_dev = destination_kind(c, p, "p"); if (p_dev < 0) return p_dev;
  const int q_dev = destination_kind(c, q, "q"); if (q_dev < 0) return q_dev;
  const int st = consensus(c, p, p_dev, q, q_dev, n_pairs, hypotheses, seed, tau, edge_sim, result);
  if (c->profile) prof_collect_lazy(c);
  return st;
} MVICP_GUARD_ABI

int mvicp_consensus_fetch(mvicp_ctx* c, long long cap_h, int* count, long long cap_c, unsigned char* flags) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->cons.H < 0) { set_error("no consensus: call mvicp_consensus first"); return MVICP_ERR_STATE; }
  if (count && cap_h < c->cons.H) { set_error("cap_h %lld < %lld hypotheses", cap_h, c->cons.H); return MVICP_ERR_ARG; }
  if (flags && cap_c < c->cons.c) { set_error("cap_c %lld < %lld pairs", cap_c, c->cons.c); return MVICP_ERR_ARG; }
  const FetchPart parts[] = {{count, c->cons.count, 4 * (size_t)c->cons.H, "count"}, {flags, c->cons.flags, (size_t)c->cons.c, "flags"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

long long mvicp_coarse_pairs(mvicp_ctx* c, const double* desc, const double* xyz, const long long* offsets, int n_sets, int dim, int n_edges,
                             const int* src, const int* dst, const unsigned long long* seeds, int mutual, double ratio, long long hypotheses,
                             double tau, double edge_sim, mvicp_coarse_edge* results) try {
  // every argument error that needs no GPU first: nothing of the context has been touched when one of them is reported
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (dim < 1 || dim > 64) { set_error("dim = %d outside [1, 64]", dim); return MVICP_ERR_ARG; }
  if (n_sets < 1) { set_error("n_sets = %d < 1", n_sets); return MVICP_ERR_ARG; }
  if (n_edges < 0 || n_edges > 65535) { set_error("n_edges = %d outside [0, 65535]", n_edges); return MVICP_ERR_ARG; }
  if (!offsets) { set_error("null offsets"); return MVICP_ERR_ARG; }
  if (offsets[0] != 0) { set_error("offsets[0] = %lld, not 0", offsets[0]); return MVICP_ERR_ARG; }
  for (int s = 0; s < n_sets; ++s)
    if (offsets[s + 1] < offsets[s]) { set_error("offsets decrease at set %d", s); return MVICP_ERR_ARG; }
  const long long total = offsets[n_sets];
  if (total >= (1ll << 31)) { set_error("%lld rows in all, not below 2^31", total); return MVICP_ERR_ARG; }
  if (total > 0 && (!desc || !xyz)) { set_error("null descriptors or points"); return MVICP_ERR_ARG; }
  if (n_edges > 0 && (!src || !dst || !seeds || !results)) { set_error("null edge arrays"); return MVICP_ERR_ARG; }
  for (int e = 0; e < n_edges; ++e)
    if (src[e] < 0 || src[e] >= n_sets || dst[e] < 0 || dst[e] >= n_sets || src[e] == dst[e]) {
      set_error("edge %d = (%d, %d) with %d sets", e, src[e], dst[e], n_sets); return MVICP_ERR_ARG;
    }
  if (hypotheses < 1 || hypotheses > (1ll << 24)) { set_error("%lld hypotheses outside [1, 2^24]", hypotheses); return MVICP_ERR_ARG; }
  if ((long long)n_edges * hypotheses > (1ll << 28)) { set_error("n_edges x hypotheses = %lld above 2^28", (long long)n_edges * hypotheses); return MVICP_ERR_ARG; }
  if (!(ratio > 0.0)) { set_error("ratio must be > 0"); return MVICP_ERR_ARG; }
  if (!std::isfinite(tau) || !(tau > 0.0)) { set_error("tau must be finite and > 0"); return MVICP_ERR_ARG; }
  if (!(edge_sim >= 0.0 && edge_sim < 1.0)) { set_error("edge_sim must be in [0, 1)"); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  int desc_dev = 0, xyz_dev = 0;
  if (total > 0) {
    desc_dev = destination_kind(c, desc, "desc"); if (desc_dev < 0) return desc_dev;
    xyz_dev = destination_kind(c, xyz, "xyz"); if (xyz_dev < 0) return xyz_dev;
  }
  const long long got = coarse_pairs(c, desc, desc_dev, xyz, xyz_dev, offsets, n_sets, dim, n_edges, src, dst, seeds, mutual, ratio, hypotheses, tau, edge_sim, results);
  if (c->profile) prof_collect_lazy(c);
  return got;
} MVICP_GUARD_ABI

int mvicp_coarse_pairs_fetch(mvicp_ctx* c, int edge, long long cap_pairs, int* pairs, unsigned char* flags) try {
  if (!c) { set_error("null context"); return MVICP_ERR_ARG; }
  if (c->coarse.edges < 0) { set_error("no coarse pairs: call mvicp_coarse_pairs first"); return MVICP_ERR_STATE; }
  if (edge < 0 || edge >= c->coarse.edges) { set_error("edge %d out of range [0,%d)", edge, c->coarse.edges); return MVICP_ERR_ARG; }
  const long long n = c->coarse.cnt[edge];
  if ((pairs || flags) && cap_pairs < n) { set_error("cap_pairs %lld < %lld pairs", cap_pairs, n); return MVICP_ERR_ARG; }
  if (n == 0) return MVICP_OK;
  const size_t seg = (size_t)c->coarse.seg[edge];
  const FetchPart parts[] = {{pairs, c->coarse.pairs + 2 * seg, 8 * (size_t)n, "pairs"}, {flags, c->coarse.flags + seg, (size_t)n, "flags"}};
  return fetch_parts(c, parts);
} MVICP_GUARD_ABI

// a (R, t) product of two column-major poses, each operation rounded on its own (this TU is built without fma contraction)
static void compose_pose(const double* A, const double* B, double* out) {
  double r[16];
  for (int row = 0; row < 3; ++row) {
    const double a0 = A[row], a1 = A[4 + row], a2 = A[8 + row];
    for (int col = 0; col < 3; ++col) r[4 * col + row] = (a0 * B[4 * col] + a1 * B[4 * col + 1]) + a2 * B[4 * col + 2];
    r[12 + row] = ((a0 * B[12] + a1 * B[13]) + a2 * B[14]) + A[12 + row];
  }
  r[3] = 0.0; r[7] = 0.0; r[11] = 0.0; r[15] = 1.0;
  std::memcpy(out, r, sizeof(r));
}

// [R^T | -(R^T t)] of a column-major pose
static void invert_pose(const double* T, double* out) {
  for (int row = 0; row < 3; ++row) {   // row `row` of R^T is column `row` of R
    const double r0 = T[4 * row], r1 = T[4 * row + 1], r2 = T[4 * row + 2];
    out[row] = r0; out[4 + row] = r1; out[8 + row] = r2;
    out[12 + row] = -((r0 * T[12] + r1 * T[13]) + r2 * T[14]);
  }
  out[3] = 0.0; out[7] = 0.0; out[11] = 0.0; out[15] = 1.0;
}

int mvicp_poses_from_pairs(int n_frames, int n_edges, const int* src, const int* dst, const int* count, const double* pose, int min_count,
                           int root, const double* root_pose, double* poses_out, int* parent, int* parent_edge, int* component) try {
  if (n_frames < 1 || n_edges < 0 || !poses_out) { set_error("poses from pairs: needs n_frames >= 1, n_edges >= 0 and poses_out"); return MVICP_ERR_ARG; }
  if (n_edges > 0 && (!src || !dst || !count || !pose)) { set_error("poses from pairs: null edge arrays"); return MVICP_ERR_ARG; }
  if (root < 0 || root >= n_frames) { set_error("poses from pairs: root %d out of range [0,%d)", root, n_frames); return MVICP_ERR_ARG; }
  if (min_count < 0) { set_error("poses from pairs: min_count < 0"); return MVICP_ERR_ARG; }
  for (int e = 0; e < n_edges; ++e)
    if (src[e] < 0 || src[e] >= n_frames || dst[e] < 0 || dst[e] >= n_frames || src[e] == dst[e]) {
      set_error("poses from pairs: edge %d = (%d, %d) with %d frames", e, src[e], dst[e], n_frames); return MVICP_ERR_ARG;
    }
  const double identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<char> reached((size_t)n_frames, 0);
  std::vector<int> par((size_t)n_frames, -1), pedge((size_t)n_frames, -1), comp((size_t)n_frames, -1);
  int components = 0, start = root, left = n_frames;
  while (left > 0) {
    reached[start] = 1; comp[start] = components; --left;
    std::memcpy(poses_out + 16 * (size_t)start, components == 0 && root_pose ? root_pose : identity, sizeof(identity));
    for (;;) {
      int pick = -1;
      for (int e = 0; e < n_edges; ++e)
        if (count[e] >= min_count && reached[src[e]] != reached[dst[e]] && (pick < 0 || count[e] > count[pick])) pick = e;
      if (pick < 0) break;
      const bool child_is_dst = reached[src[pick]] != 0;
      const int child = child_is_dst ? dst[pick] : src[pick], from = child_is_dst ? src[pick] : dst[pick];
      const double* T = pose + 16 * (size_t)pick;
      double inv[16];
      if (child_is_dst) invert_pose(T, inv);
      compose_pose(poses_out + 16 * (size_t)from, child_is_dst ? inv : T, poses_out + 16 * (size_t)child);
      reached[child] = 1; par[child] = from; pedge[child] = pick; comp[child] = components; --left;
    }
    ++components;
    for (start = 0; start < n_frames && reached[start]; ++start) {}
  }
  for (int i = 0; i < n_frames; ++i) {
    if (parent) parent[i] = par[i];
    if (parent_edge) parent_edge[i] = pedge[i];
    if (component) component[i] = comp[i];
  }
  return components;
} MVICP_GUARD_ABI

int mvicp_cluster_keep_rule(long long n_clusters, const int* size, long long min_size, long long max_clusters, unsigned char* keep) try {
  if (n_clusters < 0 || min_size < 0 || max_clusters < 0) { set_error("cluster keep rule: negative argument"); return MVICP_ERR_ARG; }
  if (!size || !keep) { set_error("cluster keep rule: needs size and keep"); return MVICP_ERR_ARG; }
  std::vector<long long> order((size_t)n_clusters);
  for (long long k = 0; k < n_clusters; ++k) order[(size_t)k] = k;
  // rank by (size descending, label ascending): a stable sort of the labels by size
  std::stable_sort(order.begin(), order.end(), [&](long long a, long long b) { return size[a] > size[b]; });
  for (long long r = 0; r < n_clusters; ++r) {
    const long long k = order[(size_t)r];
    keep[k] = (size[k] >= min_size && (max_clusters == 0 || r < max_clusters)) ? 1 : 0;
  }
  return MVICP_OK;
} MVICP_GUARD_ABI

// one Jacobi rotation on the pair (p, q), p < q, of the symmetric 3 x 3 A with the vectors V: the rotation of csrc/jacobi3.h (whose __d*_rn
// intrinsics exist on the device only) in plain operators -- this TU is built without fma contraction, so every one is rounded on its own
static void plane_jacobi_rotate(double (&A)[3][3], double (&V)[3][3], int p, int q) {
  const double apq = A[p][q];
  if (apq == 0.0) return;
  const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
  const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
  const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
  for (int r = 0; r < 3; ++r) { const double xp = A[r][p], xq = A[r][q]; A[r][p] = cs * xp - sn * xq; A[r][q] = sn * xp + cs * xq; }   // A <- A J
  for (int r = 0; r < 3; ++r) { const double xp = A[p][r], xq = A[q][r]; A[p][r] = cs * xp - sn * xq; A[q][r] = sn * xp + cs * xq; }   // A <- J^T A
  for (int r = 0; r < 3; ++r) { const double xp = V[r][p], xq = V[r][q]; V[r][p] = cs * xp - sn * xq; V[r][q] = sn * xp + cs * xq; }   // V <- V J
}

int mvicp_plane_from_moments(long long c, const long long* s, const long long* S, int q, const double* a, const double* m, double* normal, double* point) try {
  if (c < 1 || c >= (1ll << 31)) { set_error("plane from moments: needs 1 <= c < 2^31"); return MVICP_ERR_ARG; }
  if (!s || !S || !a || !m || !normal || !point) { set_error("plane from moments: needs s, S, a, m, normal and point"); return MVICP_ERR_ARG; }
  if (q < -1100 || q > 1100) { set_error("plane from moments: q = %d outside [-1100, 1100]", q); return MVICP_ERR_ARG; }
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(a[k]) || !std::isfinite(m[k])) { set_error("plane from moments: a and m must be finite"); return MVICP_ERR_ARG; }
  // the 128-bit integers c S_kl - s_k s_l (|c S| < 2^94, |s s| <= 2^126: no overflow), each converted with round-to-nearest-even
  static const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
  double A[3][3], V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
  for (int k = 0; k < 3; ++k)
    for (int l = 0; l < 3; ++l) {
      const __int128 v = (__int128)c * S[at[k][l]] - (__int128)s[k] * s[l];
      if (k == l && (S[at[k][k]] < 0 || v < 0)) { set_error("plane from moments: S_%d%d or c S - s s is negative (not the sums of one set)", k, k); return MVICP_ERR_ARG; }
      A[k][l] = (double)v;
    }
  for (int sweep = 0; sweep < 6; ++sweep) { plane_jacobi_rotate(A, V, 0, 1); plane_jacobi_rotate(A, V, 0, 2); plane_jacobi_rotate(A, V, 1, 2); }
  int j = 0;
  if (A[1][1] < A[j][j]) j = 1;
  if (A[2][2] < A[j][j]) j = 2;
  const double v0 = V[0][j], v1 = V[1][j], v2 = V[2][j];
  const double ln = std::sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  double nv[3] = {v0 / ln, v1 / ln, v2 / ln};
  if ((nv[0] * m[0] + nv[1] * m[1]) + nv[2] * m[2] < 0) { nv[0] = -nv[0]; nv[1] = -nv[1]; nv[2] = -nv[2]; }
  const double dc = (double)c;
  for (int k = 0; k < 3; ++k) {
    normal[k] = nv[k];
    point[k] = a[k] + std::ldexp((double)s[k] / dc + 0.5, -q);
  }
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_outlier_threshold(long long n, unsigned long long s1, unsigned long long s2_hi, unsigned long long s2_lo, double std_ratio, double* T) try {
  if (n < 2 || !T || !std::isfinite(std_ratio)) { set_error("outlier threshold: needs n >= 2, a finite std_ratio and T"); return MVICP_ERR_ARG; }
  typedef unsigned __int128 u128;
  const u128 s2 = ((u128)s2_hi << 64) | s2_lo, nn = (u128)(unsigned long long)n;
  if (s2 > ~(u128)0 / nn) { set_error("outlier threshold: n S2 does not fit 128 bits"); return MVICP_ERR_ARG; }
  const u128 a = nn * s2, b = (u128)s1 * s1;
  if (b > a) { set_error("outlier threshold: S1^2 > n S2 (not the sums of one set)"); return MVICP_ERR_ARG; }
  // every operation rounded on its own (this TU is built without fma contraction); the 128-bit integer converts with round-to-nearest-even
  const double dn = (double)n;
  const double mean = (double)s1 / dn;
  const double var = ((double)(a - b) / dn) / (dn - 1.0);
  const double spread = std_ratio * std::sqrt(var);
  *T = mean + spread;
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_cache_allowance(const double* pose_src_old, const double* pose_dst_old, const double* pose_src, const double* pose_dst, double max_norm, double* out) try {
  if (!pose_src_old || !pose_dst_old || !pose_src || !pose_dst || !out || !(max_norm >= 0.0)) { set_error("cache allowance: needs four poses, max_norm >= 0 and out"); return MVICP_ERR_ARG; }
  double xo[kXfRigid], xn[kXfRigid];
  fill_query_xf(pose_src_old, pose_dst_old, xo);
  fill_query_xf(pose_src, pose_dst, xn);
  *out = cache_allowance_xf(xo, xn, max_norm);
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_graph_from_overlap(int n_frames, const int* samples, const int* hits, const long long* sumq, int knn, double min_fraction,
                             int skip_frame0, int cap, int* src, int* dst, int* n_components) try {
  const int K = n_frames;
  if (K < 0 || knn < 0 || cap < 0 || (K > 0 && (!samples || !hits)) || !(min_fraction == min_fraction)) { set_error("bad arguments"); return MVICP_ERR_ARG; }
  std::vector<int> parent((size_t)K);
  for (int i = 0; i < K; ++i) parent[i] = i;
  auto root = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
  int n_edges = 0;
  std::vector<int> cand;
  for (int i = 0; i < K; ++i) {
    cand.clear();
    const int* h = hits + (size_t)i * K;
    const long long* sq = sumq ? sumq + (size_t)i * K : nullptr;
    for (int j = 0; j < K; ++j)
      if (j != i && h[j] > 0 && (double)h[j] >= min_fraction * (double)samples[i]) cand.push_back(j);
    // most hits first; equal hits: the smaller sumq (the smaller mean: an exact integer comparison), then the lower j
    std::sort(cand.begin(), cand.end(), [&](int a, int b) {
      if (h[a] != h[b]) return h[a] > h[b];
      if (sq && sq[a] != sq[b]) return sq[a] < sq[b];
      return a < b;
    });
    const int take = std::min<int>(knn, (int)cand.size());
    for (int k = 0; k < take; ++k) {
      parent[root(i)] = root(cand[k]);
      if (i == 0 && skip_frame0) continue;
      if (n_edges >= cap) { set_error("more than cap = %d edges (frame %d of %d, knn = %d)", cap, i, K, knn); return MVICP_ERR_ARG; }
      if (!src || !dst) { set_error("src / dst is null"); return MVICP_ERR_ARG; }
      src[n_edges] = i; dst[n_edges] = cand[k]; ++n_edges;
    }
  }
  if (n_components) {
    int comps = 0;
    for (int i = 0; i < K; ++i) comps += root(i) == i ? 1 : 0;
    *n_components = comps;
  }
  return n_edges;
} MVICP_GUARD_ABI

int mvicp_set_graph(mvicp_ctx* c, int n_edges, const int* src, const int* dst) try {
  MV_CHECK(bind(c));
  if (n_edges < 0 || (n_edges > 0 && (!src || !dst))) { set_error("bad edge list"); return MVICP_ERR_ARG; }
  for (int e = 0; e < n_edges; ++e)
    if (src[e] < 0 || src[e] >= c->n_frames || dst[e] < 0 || dst[e] >= c->n_frames || src[e] == dst[e]) {
      set_error("edge %d (%d->%d) invalid", e, src[e], dst[e]);
      return MVICP_ERR_ARG;
    }
  MV_CHECK(finish_builds(c));   // every cloud's structures are needed from here on
  free_graph(c);
  const int E = n_edges;
  c->E = E;
  c->esrc.assign(src, src + E);
  c->edst.assign(dst, dst + E);
  c->owned.assign(E, 0);
  c->active.assign(E, 0);
  c->src_fixed.assign(E, 0);
  c->hist.new_graph(E);   // every per-edge row of the search history: the new graph's size, describing no search
  // contiguous edge chunks balanced by N_src
  {
    std::vector<int> ns(E), owner(E);
    for (int e = 0; e < E; ++e) ns[e] = c->frames[src[e]].n;
    MV_CHECK(mvicp_edge_owner(E, ns.data(), c->world, owner.data()));
    for (int e = 0; e < E; ++e) c->owned[e] = owner[e] == c->rank;
  }
  // linearize workgroup chunk: from the GLOBAL source-point total (identical on every rank, so per-edge sums
  // have the same association order for any GPU count); small problems get small chunks to fill 256 CUs.
  {
    double total = 0;
    for (int e = 0; e < E; ++e) total += c->frames[src[e]].n;
    c->lin_chunk = total >= 6e6 ? 8192 : total >= 2e6 ? 4096 : total >= 5e5 ? 1024 : 512;
    if (c->lin_chunk_override > 0) c->lin_chunk = c->lin_chunk_override;
  }
  const int kLinChunk = c->lin_chunk;
  c->cap_off.assign(E + 1, 0);
  c->cblock_off.assign(E + 1, 0);
  c->chunk_first.assign(E + 1, 0);
  std::vector<int> chunk_edge, chunk_start;
  for (int e = 0; e < E; ++e) {
    const long long n = c->owned[e] ? c->frames[src[e]].n : 0;
    c->cap_off[e + 1] = c->cap_off[e] + ((n + 63) / 64) * 64;
    c->cblock_off[e + 1] = c->cblock_off[e] + (int)((n + kCompactBlock - 1) / kCompactBlock);
    const int nch = (int)((n + kLinChunk - 1) / kLinChunk);
    c->chunk_first[e + 1] = c->chunk_first[e] + nch;
  }
  c->total_cap = c->cap_off[E];
  c->n_cblocks = c->cblock_off[E];
  c->n_chunks = c->chunk_first[E];
  {
    // the launch order of the linearize workgroups (lin_table.h: options "lin_interleave", "lin_tail_last"); slots of the partials are per edge (linearize.hip)
    std::vector<long long> ns(E);
    for (int e = 0; e < E; ++e) ns[e] = c->owned[e] ? c->frames[src[e]].n : 0;
    lin_launch_table(E, src, ns.data(), kLinChunk, c->lin_interleave, c->lin_tail_last, chunk_edge, chunk_start);
  }
  c->n_lin_wg = (int)chunk_edge.size();   // workgroups of a launch: the n_chunks chunks + the table's pads
  const size_t cap = (size_t)c->total_cap;
  MV_CHECK(dev_alloc(&c->d_esrc, E)); MV_CHECK(dev_alloc(&c->d_edst, E)); MV_CHECK(dev_alloc(&c->d_cap_off, E + 1));
  MV_CHECK(dev_alloc(&c->d_count, E));
  // control block (see common.h): region 1 = xf | nsrc | dirty, rel2 (second pose set of a paired evaluation), region 2 = rel | a
  c->ctl_r1 = (size_t)E * kEdgeXf + (size_t)E + 2 * (size_t)E;  // xf | 2E ints = E doubles | select brackets (lo, hi) per edge
  c->ctl_rel2_off = (c->ctl_r1 + 1) & ~(size_t)1;              // 16-B aligned
  c->ctl_r2_off = c->ctl_rel2_off + (size_t)E * kEdgeRel;      // (E x 12 doubles: still 16-B aligned)
  c->ctl_r2 = (size_t)E * (kEdgeRel + 1);
  MV_CHECK(dev_alloc(&c->d_ctl, c->ctl_r2_off + c->ctl_r2));
  MV_HIP(hipMemset(c->d_ctl, 0, sizeof(double) * std::max<size_t>(c->ctl_r2_off + c->ctl_r2, 1)));
  c->d_xf = c->d_ctl; c->d_nsrc = reinterpret_cast<int*>(c->d_ctl + (size_t)E * kEdgeXf); c->d_dirty = c->d_nsrc + E;
  c->d_sel_lohi = c->d_ctl + (size_t)E * (kEdgeXf + 1);
  c->d_rel = c->d_ctl + c->ctl_r2_off; c->d_a = c->d_rel + (size_t)E * kEdgeRel; c->d_rel2 = c->d_ctl + c->ctl_rel2_off;
  MV_CHECK(dev_alloc(&c->d_nn_idx, cap)); MV_CHECK(dev_alloc(&c->d_nn_d2, cap)); MV_CHECK(dev_alloc(&c->d_nn_lb, cap));
  MV_CHECK(dev_alloc(&c->d_first, cap)); MV_CHECK(dev_alloc(&c->d_second, cap)); MV_CHECK(dev_alloc(&c->d_cd2, cap));
  MV_CHECK(dev_alloc(&c->d_stream, 10 * cap));
  MV_CHECK(dev_alloc(&c->d_qpos, cap));
  MV_HIP(hipMemset(c->d_qpos, 0xff, sizeof(int) * std::max<size_t>(cap, 1)));
  c->export_valid = false; c->export_off.assign((size_t)E + 1, 0);
  c->corr_epoch.assign(E, 0);
  for (int e = 0; e < E; ++e) c->corr_epoch[e] = ++c->epoch_counter;
  c->dslot_off.assign(E + 1, 0);
  for (int e = 0; e < E; ++e) c->dslot_off[e + 1] = c->dslot_off[e] + (int)(((c->owned[e] ? c->frames[src[e]].n : 0) + 255) / 256);
  c->n_dslots = c->dslot_off[E];
  MV_CHECK(dev_alloc(&c->d_dirty_slots, (size_t)c->n_dslots)); MV_CHECK(dev_alloc(&c->d_dslot_off, (size_t)E + 1));
  MV_HIP(hipMemset(c->d_dirty_slots, 0, sizeof(int) * std::max<size_t>((size_t)c->n_dslots, 1)));   // dirty_reduce_kernel re-zeroes what it reads
  MV_HIP(hipMemcpy(c->d_dslot_off, c->dslot_off.data(), sizeof(int) * (E + 1), hipMemcpyHostToDevice));
  MV_CHECK(dev_alloc(&c->d_cblock_off, E + 1)); MV_CHECK(dev_alloc(&c->d_cblock_cnt, (size_t)c->n_cblocks));
  MV_CHECK(dev_alloc(&c->d_sel_hist, (size_t)E * (2048 + 2)));   // cnt_lt [E] | cnt_mid [E] | hist [E][2048] (corr.hip); zeroed here, kept zero by the select kernels
  MV_HIP(hipMemset(c->d_sel_hist, 0, sizeof(unsigned int) * std::max<size_t>((size_t)E * (2048 + 2), 1)));
  c->sel_scratch_clean = true;
  c->sblock_off.assign(E + 1, 0);
  for (int e = 0; e < E; ++e) c->sblock_off[e + 1] = c->sblock_off[e] + (int)(((c->owned[e] ? c->frames[src[e]].n : 0) + kSelBlock - 1) / kSelBlock);
  c->n_sblocks = c->sblock_off[E];
  MV_CHECK(dev_alloc(&c->d_sblock_off, (size_t)E + 1));
  MV_HIP(hipMemcpy(c->d_sblock_off, c->sblock_off.data(), sizeof(int) * (E + 1), hipMemcpyHostToDevice));
  MV_CHECK(dev_alloc(&c->d_sel_keys1, cap));
  // the grid kernel's far-query list (worst case every query): allocated here, not lazily inside the first grid launch — a
  // 100 MB hipMalloc in the middle of an ICP loop costs milliseconds
  if (cap > c->far_cap) {
    if (c->d_far_list) MV_HIP(hipFree(c->d_far_list));
    c->d_far_list = nullptr; c->far_cap = 0;
    MV_HIP(hipMalloc(&c->d_far_list, sizeof(int) * 2 * cap));
    c->far_cap = cap;
  }
  MV_CHECK(warm_nn_grid(c)); MV_CHECK(warm_nn_tile(c)); MV_CHECK(warm_nn_mfma(c));
  if (c->opt.tie_rule && !(c->opt.tie_lazy && c->world == 1)) {   // the reference's own trees over the targets of the edges THIS RANK owns: they decide exact distance ties (the others are never searched here)
    std::vector<int> need;
    for (int e = 0; e < E; ++e) if (c->owned[e]) need.push_back(dst[e]);
    MV_CHECK(ensure_tie_trees(c, need));
  }
  MV_CHECK(dev_alloc(&c->d_median, E));
  MV_CHECK(dev_alloc(&c->d_chunk_edge, (size_t)c->n_lin_wg)); MV_CHECK(dev_alloc(&c->d_chunk_start, (size_t)c->n_lin_wg));
  MV_CHECK(dev_alloc(&c->d_chunk_first, E + 1));
  MV_CHECK(dev_alloc(&c->d_partials, 2 * (size_t)c->n_chunks * kLinPartial));   // (second half: the second pose set of a paired launch)
  MV_CHECK(dev_alloc(&c->d_out, (size_t)E * (MVICP_EDGE_BLOCK + 3) + 2));   // blocks | (count, median d2) x E | armed | a x E  (see common.h)
  MV_HIP(hipMemset(c->d_out, 0, sizeof(double) * ((size_t)E * (MVICP_EDGE_BLOCK + 3) + 2)));
  if (E) {
    MV_HIP(hipMemcpy(c->d_esrc, src, sizeof(int) * E, hipMemcpyHostToDevice));
    MV_HIP(hipMemcpy(c->d_edst, dst, sizeof(int) * E, hipMemcpyHostToDevice));
    MV_HIP(hipMemset(c->d_count, 0, sizeof(int) * E));
  }
  MV_HIP(hipMemcpy(c->d_cap_off, c->cap_off.data(), sizeof(long long) * (E + 1), hipMemcpyHostToDevice));
  MV_HIP(hipMemcpy(c->d_cblock_off, c->cblock_off.data(), sizeof(int) * (E + 1), hipMemcpyHostToDevice));
  MV_HIP(hipMemcpy(c->d_chunk_first, c->chunk_first.data(), sizeof(int) * (E + 1), hipMemcpyHostToDevice));
  if (c->n_lin_wg) {
    MV_HIP(hipMemcpy(c->d_chunk_edge, chunk_edge.data(), sizeof(int) * c->n_lin_wg, hipMemcpyHostToDevice));
    MV_HIP(hipMemcpy(c->d_chunk_start, chunk_start.data(), sizeof(int) * c->n_lin_wg, hipMemcpyHostToDevice));
  }
  // pinned, device-mapped staging: control-block mirror | blocks | results | misc
  c->pin_blocks_off = c->ctl_r2_off + c->ctl_r2;
  c->pin_res_off = c->pin_blocks_off + (size_t)E * MVICP_EDGE_BLOCK;
  c->pin_misc_off = c->pin_res_off + 2 * (size_t)E + 2;           // (+ the "armed" slot the select kernels write behind the E pairs)
  c->pin_spec_off = c->pin_misc_off + 4 * (size_t)E + 64;          // blocks of the speculative first evaluation (+ the exchanged tail with N > 1 ranks)
  c->pin_adev_off = c->pin_spec_off + (size_t)E * (MVICP_EDGE_BLOCK + 3) + 2; // SoftLOne scales as the device computed them (single rank)
  if (c->h_pin) { MV_HIP(hipHostFree(c->h_pin)); c->h_pin = nullptr; c->h_pin_doubles = 0; }
  c->pin_spec2_off = (c->pin_adev_off + (size_t)E + 8 + 1) & ~(size_t)1;                 // blocks of the second queued evaluation (16-B aligned)
  c->pin_rel2_off = c->pin_spec2_off + (size_t)E * MVICP_EDGE_BLOCK + ((size_t)E * MVICP_EDGE_BLOCK & 1);   // its relative transforms (E x 12), copied into d_rel in stream order
  c->pin_blocks2_off = (c->pin_rel2_off + (size_t)E * kEdgeRel + 1) & ~(size_t)1;         // second block set of mvicp_linearize_pair (16-B aligned)
  MV_CHECK(ensure_pin(c, c->pin_blocks2_off + (size_t)E * MVICP_EDGE_BLOCK + 8));
  {
    void* dp = nullptr;
    MV_HIP(hipHostGetDevicePointer(&dp, c->h_pin, 0));
    c->d_blocks_host = (double*)dp + c->pin_blocks_off;
    c->d_res_host = (double*)dp + c->pin_res_off;
    c->d_spec_host = (double*)dp + c->pin_spec_off;
    c->d_adev_host = (double*)dp + c->pin_adev_off;
    c->d_spec2_host = (double*)dp + c->pin_spec2_off;
    c->d_blocks2_host = (double*)dp + c->pin_blocks2_off;
  }
  c->spec_ready = false; c->spec_arm = false;
  c->spec2_ready = false; c->spec2_armed = false;
  if (!c->h_census) MV_HIP(hipHostMalloc((void**)&c->h_census, 8 * sizeof(unsigned long long), hipHostMallocDefault));
  return MVICP_OK;
} MVICP_GUARD_ABI

// everything earlier searches left behind (host-side bookkeeping only): the history, and what of it the context mirrors
static void forget_history(mvicp_ctx* c) {
  c->hist.forget(c->E);
  c->export_valid = false;
  for (int e = 0; e < c->E; ++e) c->corr_epoch[e] = ++c->epoch_counter;
  c->spec_ready = false; c->spec_arm = false;
  c->spec2_ready = false; c->spec2_armed = false;
}

int mvicp_reset_history(mvicp_ctx* c) try {
  MV_CHECK(bind(c));
  MV_HIP(hipStreamSynchronize(c->stream));
  forget_history(c);
  return MVICP_OK;
} MVICP_GUARD_ABI

// mvicp_correspond: the policy, its options and the table of the cross-round state are csrc/search_plan.h; what follows executes a plan.
static int correspond_once(mvicp_ctx* c, const double* poses, const unsigned char* fixed, float thresh, int nn_method, int* counts, float* weights, bool* tie_unresolved);

int mvicp_correspond(mvicp_ctx* c, const double* poses, const unsigned char* fixed, float thresh, int nn_method, int* counts, float* weights) try {
  MV_CHECK(bind(c));
  // A search that does not return OK — an argument error, a failed launch, an exception — may have got as far as overwriting prev_xf / prev_q with
  // transforms that were never searched, while seeds, bounds, lists and the cache flags still describe the last search that succeeded.  Nothing of that
  // mixture may meet the next search: whatever way this call ends other than OK, the cross-round state is dropped (host bookkeeping, after the stream
  // has drained) and every edge gets a new epoch — the next search is a first search.
  struct Forget { mvicp_ctx* c; bool ok = false; ~Forget() { if (!ok) { (void)hipStreamSynchronize(c->stream); forget_history(c); } } } forget{c};
  bool unresolved = false;
  MV_CHECK(correspond_once(c, poses, fixed, thresh, nn_method, counts, weights, &unresolved));
  if (!unresolved) { forget.ok = true; return MVICP_OK; }
  // Lazy tie trees (single rank): the search reported an exact distance tie on a target whose reference-equivalent tree does not exist yet, so that
  // query still carries the kernels' own rule (lowest index).  Build the trees of every searched target now — once per cloud, like the reference's
  // lazily built index — forget what this search left behind and search again: this time the fix-up decides the ties the way nanoflann does.
  std::vector<int> need;
  for (int e = 0; e < c->E; ++e) if (c->active[e] && !c->frames[c->edst[e]].has_tie) need.push_back(c->edst[e]);
  MV_HIP(hipStreamSynchronize(c->stream));
  MV_CHECK(ensure_tie_trees(c, need));
  forget_history(c);
  unresolved = false;
  MV_CHECK(correspond_once(c, poses, fixed, thresh, nn_method, counts, weights, &unresolved));
  if (unresolved) { set_error("tie fix-up still without a tree after building them"); return MVICP_ERR_INTERNAL; }
  forget.ok = true;
  return MVICP_OK;
} MVICP_GUARD_ABI

// ---- the executor: builds the inputs, asks search_plan.h for the plan, then uploads, launches, exchanges and waits as the plan says ----

namespace {
struct CorrMarks {   // the host.corr.* profile scopes: each mark closes the interval since the one before
  mvicp_ctx* c; double t;
  void operator()(const char* nm) { if (c->profile) { const double now = now_ms(); ProfEntry& pe = c->prof[nm]; pe.ms += now - t; pe.launches += 1; t = now; } }
};
// the exchanged / pinned result buffer: E x 91 blocks | (count, median d2) x E | armed | a x E
size_t out_blocks(const mvicp_ctx* c) { return (size_t)c->E * MVICP_EDGE_BLOCK; }
size_t out_tail(const mvicp_ctx* c) { return 3 * (size_t)c->E + 1; }
size_t out_armed(const mvicp_ctx* c) { return out_blocks(c) + 2 * (size_t)c->E; }
void spec_failed(mvicp_ctx* c) { c->hist.spec_flags_valid = false; c->spec_arm = false; }
}  // namespace

// what a search is a function of (search_plan.h), read off the context
static SearchInputs search_inputs(mvicp_ctx* c, const double* poses, const unsigned char* fixed, float thresh, int nn_method) {
  c->plan_frames.resize(c->frames.size());
  for (size_t k = 0; k < c->frames.size(); ++k) {
    const FrameDev& f = c->frames[k];
    PlanFrame& pf = c->plan_frames[k];
    pf.n = f.n; pf.max_norm = f.max_norm; pf.cell = f.grid.cell; pf.has_grid = f.has_grid; pf.has_tie = f.has_tie; pf.has_snor = f.grid.snor != nullptr;
  }
  SearchInputs in;
  in.E = c->E; in.n_frames = c->n_frames;
  in.esrc = c->esrc.data(); in.edst = c->edst.data(); in.owned = c->owned.data(); in.frames = c->plan_frames.data();
  in.poses = poses; in.fixed = fixed; in.thresh = thresh; in.nn_method = nn_method;
  in.exchange = c->comm != nullptr || c->ar_fn != nullptr; in.world = c->world;
  return in;
}

// The poses of the queued evaluations, staged behind region 1 of the control-block mirror.  -> how many doubles of it go up with the search
static size_t stage_queued_evaluations(mvicp_ctx* c, const SearchPlan& plan, const double* poses) {
  if (!plan.spec_arm) return c->ctl_r1;
  // the solve evaluates at x_to_pose(pose_to_x(P)) (host/lm.cpp): the same round trip here, so the poses match bit for bit.  The
  // relative transforms of that evaluation ride on the control-block upload (region 2 follows region 1; the SoftLOne scales
  // behind them are written on the device by the select kernels later in the stream)
  c->spec_poses.resize(16 * (size_t)c->n_frames);
  double xp[7];
  for (int k = 0; k < c->n_frames; ++k) { se3::pose_to_x(c->hist.spec_param, poses + 16 * (size_t)k, xp); se3::x_to_pose(c->hist.spec_param, xp, &c->spec_poses[16 * (size_t)k]); }
  fill_rel(c, c->spec_poses.data());
  c->spec_q_plane = c->hist.spec_plane; c->spec_q_robust = c->hist.spec_robust;
  // paired launch (option lin_pair): its relative transforms lie between region 1 and rel, so they ride on the same upload
  if (plan.spec2_plan && c->opt.lin_pair) fill_rel_into(c, c->hist.last_cand_poses.data(), c->h_pin + c->ctl_rel2_off);
  return c->ctl_r2_off + (size_t)c->E * kEdgeRel;
}

// The local launches of a search: control-block upload, the NN kernel of the plan, list maintenance, the select
static int launch_local_search(mvicp_ctx* c, const SearchInputs& in, const SearchPlan& plan, double bound, size_t upload_doubles, CorrMarks& mark) {
  MV_HIP(hipMemcpyAsync(c->d_ctl, c->h_pin, sizeof(double) * upload_doubles, hipMemcpyHostToDevice, c->stream));
  if (c->fault_inject > 0 && --c->fault_inject == 0) { set_error("injected launch failure (option fault_inject)"); return MVICP_ERR_HIP; }   // tests: a local failure before the exchange
  if (plan.method == MVICP_NN_BRUTE) MV_CHECK(launch_nn_brute_edges(c));
  else if (plan.method == MVICP_NN_GRID) MV_CHECK(launch_nn_grid_edges(c, bound, plan));
  else {
    if (c->profile && plan.eps_over_mu >= 0.0) { ProfEntry& pe = c->prof["auto.eps_over_mu"]; pe.ms = plan.eps_over_mu; pe.launches += 1; }   // (observable: the last cache-aware round's ratio)
    MV_CHECK(launch_nn_tile_edges(c, bound, plan));
  }
  record_queued(in, c->opt, plan, c->hist);
  if (!plan.all_unchanged) c->export_valid = false;   // (a search that reproduces every list leaves the exported copy what it is)
  mark("host.corr.nn_launch");
  if (!plan.nothing_can_change) {
    MV_CHECK(launch_compact(c, bound));
    MV_CHECK(launch_gather_stream(c));
  }
  if (plan.sel_skip) { c->h_pin[c->pin_res_off + 2 * (size_t)c->E] = plan.spec_arm ? 1.0 : 0.0; return MVICP_OK; }   // (nothing on the device writes the mapped results in this search)
  return plan.use_bracket ? launch_select_bracket(c) : launch_select_median(c, bound);
}

// This rank's share of the exchanged buffer (N > 1 ranks): the queued first evaluation, or zeros
static int queue_exchanged_evaluation(mvicp_ctx* c, const SearchPlan& plan) {
  c->lin_out = c->d_out;
  if (plan.spec_arm) return launch_linearize(c, c->spec_q_plane, c->spec_q_robust);
  // this rank queued no evaluation: its share of the block region and of the scale slots is ZERO, not whatever the last exchange left
  // there (already-summed values would be summed again round after round).  Every rank sends the same buffer size whatever it decided.
  if (hipMemsetAsync(c->d_out, 0, sizeof(double) * out_blocks(c), c->stream) != hipSuccess ||
      hipMemsetAsync(c->d_out + out_armed(c) + 1, 0, sizeof(double) * (size_t)c->E, c->stream) != hipSuccess) { set_error("hipMemsetAsync of the exchange buffer failed"); return MVICP_ERR_HIP; }
  return MVICP_OK;
}

// The queued evaluations of a single rank (the plan armed): one, or at a fixed point two — paired in one launch or as two launches
static int queue_evaluations(mvicp_ctx* c, const SearchPlan& plan) {
  auto second_armed = [c]() { c->spec2_armed = true; c->spec2_poses = c->hist.last_cand_poses; c->spec2_plane = c->spec_q_plane; c->spec2_robust = c->spec_q_robust; };
  c->spec2_armed = false;
  if (plan.spec2_plan && c->opt.lin_pair) {
    // both queued evaluations in one pass over the operand stream: first blocks -> d_spec_host, second -> d_spec2_host
    const int st = launch_linearize_pair(c, c->spec_q_plane, c->spec_q_robust, c->d_spec_host, c->d_spec2_host);
    if (st == MVICP_OK) second_armed();
    return st;
  }
  c->lin_out = c->d_spec_host;
  int st = launch_linearize(c, c->spec_q_plane, c->spec_q_robust);
  if (st == MVICP_OK && plan.spec2_plan) {
    fill_rel_into(c, c->hist.last_cand_poses.data(), c->h_pin + c->pin_rel2_off);
    if (hipMemcpyAsync(c->d_rel, c->h_pin + c->pin_rel2_off, sizeof(double) * (size_t)c->E * kEdgeRel, hipMemcpyHostToDevice, c->stream) == hipSuccess) {
      c->lin_out = c->d_spec2_host;
      st = launch_linearize(c, c->spec_q_plane, c->spec_q_robust);
      if (st == MVICP_OK) second_armed();
    }
  }
  return st;
}

// One collective of a search: d_out[off, off + len) summed over the ranks, then copied to its pinned mirror (`what` names it in the error).
// Failure semantics with N > 1 ranks.  A rank that failed locally before the collective (an allocation, an upload, a
// launch) used to return at once — and its peers blocked in the collective forever.  Now every local step up to the exchange only records
// its status (st_local); a rank whose share cannot be delivered still ENTERS the collective, with the "armed" slot of the exchanged buffer
// poisoned (eight 0xFF bytes = a NaN): the sum is NaN on every rank, every rank sees it after its own wait, drops its cross-round state and
// returns an error from this same call — the failing rank its own status (its message kept in local_msg), the others MVICP_ERR_COMM.  (A
// device that no longer executes anything cannot poison or exchange: that stays fatal for the job, as any collective library has it; then
// *entered is false and the caller returns st_local.)
static int exchange_out(mvicp_ctx* c, size_t off, size_t len, const char* what, int st_local, char* local_msg, bool* entered) {
  *entered = true;
  if (st_local != MVICP_OK) {
    std::memcpy(local_msg, g_err, sizeof(g_err));
    if (hipMemsetAsync(c->d_out + out_armed(c), 0xFF, sizeof(double), c->stream) != hipSuccess) {
      if (off == 0) set_error("%s — and the exchange buffer could not be poisoned: the peers of this rank will block in the collective", local_msg);
      *entered = false;
      return st_local;
    }
  }
  int st;
  { ProfScope pc(c, "comm", 8.0 * (double)len); st = comm_allreduce_sum(c, c->d_out + off, len); }
  if (st == MVICP_OK && hipMemcpyAsync(c->h_pin + c->pin_spec_off + off, c->d_out + off, sizeof(double) * len, hipMemcpyDeviceToHost, c->stream) != hipSuccess) {
    set_error("hipMemcpyAsync of the exchanged %s failed", what); st = MVICP_ERR_HIP;
  }
  return st;
}

// A median left its bracket (flagged -1 in its slot): with N > 1 ranks every rank sees the summed slots, so every rank takes the same
// decision: full select for everything (rare once the registration has settled) and a second, tail-only exchange
static int redo_select(mvicp_ctx* c, double bound, bool exchange, char* local_msg) {
  int st = launch_select_median(c, bound);
  if (exchange) {
    const int st_r = st;
    bool entered;
    st = exchange_out(c, out_blocks(c), out_tail(c), "tail", st_r, local_msg, &entered);
    if (!entered) { spec_failed(c); return st_r; }
    if (st == MVICP_OK) st = stream_wait(c);
    if (st != MVICP_OK) { spec_failed(c); return st; }
    if (std::isnan(c->h_pin[c->pin_spec_off + out_armed(c)])) {
      forget_history(c);
      if (st_r != MVICP_OK) { set_error("%s", local_msg); return st_r; }
      set_error("a peer rank failed before the second exchange of this search (poisoned exchange buffer); cross-round state dropped on every rank");
      return MVICP_ERR_COMM;
    }
    return MVICP_OK;
  }
  if (st == MVICP_OK) st = stream_wait(c);
  if (st != MVICP_OK) spec_failed(c);
  return st;
}

static int correspond_once(mvicp_ctx* c, const double* poses, const unsigned char* fixed, float thresh, int nn_method, int* counts, float* weights, bool* tie_unresolved) {
  // whatever way a search ends other than OK (an error status, an exception): the next one neither reuses its select result nor trusts the
  // self-cleaning select scratch (a kernel that never ran has not re-zeroed what its predecessor filled)
  struct Guard { mvicp_ctx* c; bool ok = false; ~Guard() { if (!ok) { c->hist.sel_result_valid = false; c->sel_scratch_clean = false; } } } guard{c};
  if (!poses) { set_error("poses is null"); return MVICP_ERR_ARG; }
  if (c->E == 0) { set_error("no graph: call mvicp_set_graph first"); return MVICP_ERR_STATE; }
  const int E = c->E;
  HostScope hs_all(c, "host.correspond");
  CorrMarks mark{c, now_ms()};
  // the plan.  Region 1 of the control block (xf | nsrc | dirty | select brackets) is planned straight into its pinned mirror and goes up in ONE copy
  const SearchInputs in = search_inputs(c, poses, fixed, thresh, nn_method);
  SearchPlan& plan = c->plan;
  plan.active = c->active.data(); plan.src_fixed = c->src_fixed.data();
  plan.xf = c->h_pin; plan.nsrc = reinterpret_cast<int*>(c->h_pin + (size_t)E * kEdgeXf); plan.dirty = plan.nsrc + E; plan.lohi = c->h_pin + (size_t)E * (kEdgeXf + 1);
  plan_search(in, c->opt, c->hist, plan);
  // every local step up to the exchange only records its status: see exchange_out
  int st_local = MVICP_OK;
  if (!plan.tie_need.empty()) st_local = ensure_tie_trees(c, plan.tie_need);
  const double bound = sqrt_bound((double)thresh);
  mark("host.corr.setup");
  if (plan.status != MVICP_OK) { set_error("unknown nn_method %d", nn_method); return plan.status; }
  c->spec_ready = false; c->spec2_ready = false;
  c->spec_arm = plan.spec_arm;
  const size_t nb = out_blocks(c), armed = out_armed(c);
  c->d_res_target = in.exchange ? c->d_out + nb : nullptr;
  c->d_a_check = in.exchange ? c->d_out + armed + 1 : c->d_adev_host;   // where the select kernels copy the scales they derive
  const size_t upload_doubles = stage_queued_evaluations(c, plan, poses);
  if (st_local == MVICP_OK) st_local = launch_local_search(c, in, plan, bound, upload_doubles, mark);
  if (st_local != MVICP_OK && !in.exchange) { c->hist.spec_flags_valid = false; return st_local; }
  // the queued first evaluation (its relative transforms went up with the control block).  With N > 1 ranks: ONE collective per
  // search — [E x 91 blocks | (count, median d2) x E | armed | a x E], always the full buffer — and ONE wait.
  int st_q = MVICP_OK;
  char local_msg[sizeof(g_err)] = "";
  if (in.exchange) {
    if (st_local == MVICP_OK) st_local = queue_exchanged_evaluation(c, plan);
    bool entered;
    st_q = exchange_out(c, 0, nb + out_tail(c), "buffer", st_local, local_msg, &entered);
    if (!entered) { spec_failed(c); return st_local; }
  } else if (plan.spec_arm) st_q = queue_evaluations(c, plan);
  mark("host.corr.post_launch");
  // (count, median d2) per edge arrive in mapped host memory, written by bracket_final_kernel (single rank), or summed over ranks
  // behind the blocks
  if (st_q == MVICP_OK) st_q = stream_wait(c);
  if (st_q != MVICP_OK) { spec_failed(c); return st_q; }
  if (in.exchange && std::isnan(c->h_pin[c->pin_spec_off + armed])) {
    // some rank (this one if st_local says so) entered the collective without its share: nothing of this search is usable anywhere.  Every
    // rank forgets what earlier searches left behind — the next search is a first search on all of them, so their states agree again.
    forget_history(c);
    c->census_pending = false;
    if (st_local != MVICP_OK) { set_error("%s", local_msg); return st_local; }
    set_error("a peer rank failed before the exchange of this search (poisoned exchange buffer); nothing was updated, cross-round state dropped on every rank");
    return MVICP_ERR_COMM;
  }
  census_resolve(c);
  if (plan.tie_launched && c->h_tie_seen && c->h_tie_seen[1] != 0u) *tie_unresolved = true;
  if (plan.tie_launched && c->h_tie_seen && c->h_tie_seen[2] != 0u) { set_error("tie fix-up: a walk ran out of stack (a tree deeper than its recorded levels)"); return MVICP_ERR_INTERNAL; }
  mark("host.corr.wait");
  const double* hr = in.exchange ? c->h_pin + c->pin_spec_off + nb : c->h_pin + c->pin_res_off;
  bool redone = false;
  for (int e = 0; e < E; ++e) if (hr[2 * e + 1] < 0.0) redone = true;
  if (redone) MV_CHECK(redo_select(c, bound, in.exchange, local_msg));
  c->spec_ready = record_arrived(in, plan, c->hist, c->h_tie_seen ? *c->h_tie_seen : 1u, c->h_far_seen ? *c->h_far_seen : 1u, hr,
                                 in.exchange ? hr + 2 * (size_t)E + 1 : c->h_pin + c->pin_adev_off, redone);
  c->spec2_ready = c->spec_ready && c->spec2_armed;   // (same scales, same lists: valid whenever the first one is)
  c->spec2_armed = false;
  c->spec_arm = false;
  double* ha = c->h_pin + c->ctl_r2_off + (size_t)E * kEdgeRel;   // `a` slice of region 2: uploaded with rel by the next evaluation
  for (int e = 0; e < E; ++e) {
    ha[e] = (double)c->hist.h_weight[e];
    if (counts) counts[e] = c->hist.h_count[e];
    if (weights) weights[e] = c->hist.h_weight[e];
    if (!plan.unchanged[e]) c->corr_epoch[e] = ++c->epoch_counter;
  }
  mark("host.corr.finish");
  if (c->profile) prof_collect_lazy(c);
  guard.ok = true;
  return MVICP_OK;
}

// every exportable edge's list of the last search, un-sorted on the device into the reference's layout and copied once (export.hip)
static int ensure_export(mvicp_ctx* c, bool wait = true) {
  if (!c->export_valid) {
    HostScope hs(c, "host.export");
    MV_CHECK(launch_export(c));
    c->export_valid = true;
  }
  if (wait && c->export_in_flight) {
    MV_CHECK(stream_wait(c));
    c->export_in_flight = false;
    if (c->profile) prof_collect_lazy(c);
  }
  return MVICP_OK;
}

int mvicp_map_correspondences(mvicp_ctx* c, const mvicp_corr** triples, const long long** offsets) try {
  MV_CHECK(bind(c));
  if (!triples || !offsets) { set_error("null output"); return MVICP_ERR_ARG; }
  if (!c->hist.have_corr) { set_error("no correspondences yet"); return MVICP_ERR_STATE; }
  MV_CHECK(ensure_export(c));
  *triples = (const mvicp_corr*)c->h_export;
  *offsets = c->export_off.data();
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_map_correspondences_async(mvicp_ctx* c, const mvicp_corr** triples, const long long** offsets) try {
  MV_CHECK(bind(c));
  if (!triples || !offsets) { set_error("null output"); return MVICP_ERR_ARG; }
  if (!c->hist.have_corr) { set_error("no correspondences yet"); return MVICP_ERR_STATE; }
  MV_CHECK(ensure_export(c, false));
  *triples = (const mvicp_corr*)c->h_export;
  *offsets = c->export_off.data();
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_wait_correspondences(mvicp_ctx* c, int edge) try {
  MV_CHECK(bind(c));
  if (edge < 0 || edge >= c->E) { set_error("edge %d out of range", edge); return MVICP_ERR_ARG; }
  if (!c->export_valid) { set_error("no export in flight: call mvicp_map_correspondences_async after the search"); return MVICP_ERR_STATE; }
  if (!c->export_in_flight || c->export_chunks == 0) return MVICP_OK;
  const int k = c->export_edge_chunk[edge];
  MV_HIP(hipEventSynchronize(c->export_events[k]));
  if (k == c->export_chunks - 1) c->export_in_flight = false;   // (the last chunk's event is behind every other one on the stream)
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_correspondence_epochs(mvicp_ctx* c, const unsigned long long** epochs) try {
  MV_CHECK(bind(c));
  if (!epochs) { set_error("null output"); return MVICP_ERR_ARG; }
  if (c->E == 0) { set_error("no graph"); return MVICP_ERR_STATE; }
  *epochs = c->corr_epoch.data();
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_get_correspondences(mvicp_ctx* c, int edge, int cap, int* first, int* second, double* dist) try {
  MV_CHECK(bind(c));
  if (edge < 0 || edge >= c->E) { set_error("edge %d out of range", edge); return MVICP_ERR_ARG; }
  if (!c->hist.have_corr) { set_error("no correspondences yet"); return MVICP_ERR_STATE; }
  if (!c->owned[edge]) { set_error("edge %d is owned by another rank", edge); return MVICP_ERR_STATE; }
  const int n = c->hist.h_count[edge];
  if (cap < n) { set_error("capacity %d < count %d", cap, n); return MVICP_ERR_ARG; }
  if (!c->hist.explicit_list[edge]) {
    // a list built by mvicp_correspond: slice of the one export of this search (first call after a search runs it for ALL edges)
    if (n == 0) return 0;
    MV_CHECK(ensure_export(c));
    const mvicp_corr* t = (const mvicp_corr*)c->h_export + c->export_off[edge];
    if (c->export_off[edge + 1] - c->export_off[edge] != n) { set_error("export of edge %d holds %lld triples, expected %d", edge, c->export_off[edge + 1] - c->export_off[edge], n); return MVICP_ERR_STATE; }
    for (int i = 0; i < n; ++i) {
      if (first) first[i] = t[i].first;
      if (second) second[i] = t[i].second;
      if (dist) dist[i] = t[i].dist;
    }
    return n;
  }
  // an explicit list (mvicp_set_correspondences: any order, repeats allowed) has no per-query positions: host-side un-sort
  const size_t off = (size_t)c->cap_off[edge];
  MV_HIP(hipStreamSynchronize(c->stream));
  std::vector<int> a(n), b(n);
  std::vector<double> d(n);
  if (n) {
    MV_HIP(hipMemcpy(a.data(), c->d_first + off, sizeof(int) * n, hipMemcpyDeviceToHost));
    MV_HIP(hipMemcpy(b.data(), c->d_second + off, sizeof(int) * n, hipMemcpyDeviceToHost));
    MV_HIP(hipMemcpy(d.data(), c->d_cd2 + off, sizeof(double) * n, hipMemcpyDeviceToHost));
  }
  const std::vector<int>& so = c->frames[c->esrc[edge]].grid.h_order;
  const std::vector<int>& dorder = c->frames[c->edst[edge]].grid.h_order;
  std::vector<int> perm(n);
  for (int i = 0; i < n; ++i) { a[i] = so[a[i]]; b[i] = dorder[b[i]]; perm[i] = i; }
  std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return a[x] < a[y]; });
  for (int i = 0; i < n; ++i) {
    const int k = perm[i];
    if (first) first[i] = a[k];
    if (second) second[i] = b[k];
    if (dist) dist[i] = std::sqrt(d[k]);  // frame.cpp:139 pointDist = sqrt(pointDistSquared), IEEE on the host
  }
  return n;
} MVICP_GUARD_ABI

int mvicp_set_correspondences(mvicp_ctx* c, int edge, int n, const int* first, const int* second, float weight) try {
  MV_CHECK(bind(c));
  if (edge < 0 || edge >= c->E) { set_error("edge %d out of range", edge); return MVICP_ERR_ARG; }
  if (!c->owned[edge]) { set_error("edge %d is owned by another rank", edge); return MVICP_ERR_STATE; }
  const int ns = c->frames[c->esrc[edge]].n, nd = c->frames[c->edst[edge]].n;
  if (n < 0 || n > ns) { set_error("n=%d exceeds the edge capacity N_src=%d", n, ns); return MVICP_ERR_ARG; }
  if (n > 0 && (!first || !second)) { set_error("null correspondence list (n=%d)", n); return MVICP_ERR_ARG; }
  for (int i = 0; i < n; ++i)
    if (first[i] < 0 || first[i] >= ns || second[i] < 0 || second[i] >= nd) { set_error("correspondence %d out of range", i); return MVICP_ERR_ARG; }
  const size_t off = (size_t)c->cap_off[edge];
  MV_HIP(hipStreamSynchronize(c->stream));
  if (n) {
    // device lists are kept in sorted positions
    const std::vector<int>& si = c->frames[c->esrc[edge]].grid.h_inv;
    const std::vector<int>& di = c->frames[c->edst[edge]].grid.h_inv;
    std::vector<int> a(n), b(n);
    for (int i = 0; i < n; ++i) { a[i] = si[first[i]]; b[i] = di[second[i]]; }
    MV_HIP(hipMemcpy(c->d_first + off, a.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    MV_HIP(hipMemcpy(c->d_second + off, b.data(), sizeof(int) * n, hipMemcpyHostToDevice));
    MV_HIP(hipMemset(c->d_cd2 + off, 0, sizeof(double) * n));
  }
  c->hist.explicit_edge(edge, n, weight);
  c->spec_ready = false; c->spec2_ready = false;
  c->export_valid = false;
  c->corr_epoch[edge] = ++c->epoch_counter;
  const double a = (double)weight;
  MV_HIP(hipMemcpy(c->d_count + edge, &n, sizeof(int), hipMemcpyHostToDevice));
  {   // an explicit list is arbitrary (repeats, any order): never the identity list the linearize kernel may shortcut
    const int not_identity = -1;
    MV_HIP(hipMemcpy(c->d_nsrc + edge, &not_identity, sizeof(int), hipMemcpyHostToDevice));
  }
  MV_HIP(hipMemcpy(c->d_a + edge, &a, sizeof(double), hipMemcpyHostToDevice));
  c->h_pin[c->ctl_r2_off + (size_t)c->E * kEdgeRel + edge] = a;   // host mirror: region 2 is re-uploaded by every evaluation
  const int one = 1;
  MV_HIP(hipMemcpy(c->d_dirty + edge, &one, sizeof(int), hipMemcpyHostToDevice));  // this edge's operands must be (re)gathered
  MV_CHECK(launch_gather_stream(c));
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_nn_query(mvicp_ctx* c, int frame, const double* queries, int n, int nn_method, int* idx, double* d2) try {
  MV_CHECK(bind(c));
  if (frame < 0 || frame >= c->n_frames) { set_error("frame %d out of range", frame); return MVICP_ERR_ARG; }
  if (n < 0 || (n && (!queries || !idx || !d2))) { set_error("bad query buffers"); return MVICP_ERR_ARG; }
  if (nn_method < MVICP_NN_AUTO || nn_method > MVICP_NN_TILE) { set_error("unknown nn_method %d", nn_method); return MVICP_ERR_ARG; }   // (before anything is allocated or built)
  MV_CHECK(finish_builds(c));
  const FrameDev& f = c->frames[frame];
  if (f.n == 0) { set_error("frame %d is empty (nanoflann throws here: nanoflann.hpp:904)", frame); return MVICP_ERR_STATE; }
  if (n == 0) return MVICP_OK;
  double* dq = nullptr; int* di = nullptr; double* dd = nullptr;
  MV_CHECK(dev_alloc(&dq, 3 * (size_t)n)); MV_CHECK(dev_alloc(&di, (size_t)n)); MV_CHECK(dev_alloc(&dd, (size_t)n));
  MV_HIP(hipMemcpy(dq, queries, sizeof(double) * 3 * (size_t)n, hipMemcpyHostToDevice));
  int method = (nn_method == MVICP_NN_AUTO || nn_method == MVICP_NN_TILE) ? MVICP_NN_GRID : nn_method;  // raw queries are not patch-ordered
  if (c->opt.tie_rule) MV_CHECK(ensure_tie_trees(c, std::vector<int>(1, frame)));
  if (method == MVICP_NN_GRID && !f.has_grid) method = MVICP_NN_BRUTE;
  int st;
  if (method == MVICP_NN_BRUTE) st = launch_nn_brute_queries(c, f, dq, n, di, dd);
  else if (method == MVICP_NN_GRID) st = launch_nn_grid_queries(c, f, dq, n, di, dd);
  else { set_error("unknown nn_method %d", nn_method); st = MVICP_ERR_ARG; }
  if (st == MVICP_OK) {
    hipError_t e1 = hipStreamSynchronize(c->stream);
    if (e1 == hipSuccess) census_resolve(c);
    if (e1 == hipSuccess && c->opt.tie_rule && c->h_tie_seen && c->h_tie_seen[2] != 0u) { set_error("tie fix-up: a walk ran out of stack (a tree deeper than its recorded levels)"); st = MVICP_ERR_INTERNAL; }
    hipError_t e2 = hipMemcpy(idx, di, sizeof(int) * n, hipMemcpyDeviceToHost);
    hipError_t e3 = hipMemcpy(d2, dd, sizeof(double) * n, hipMemcpyDeviceToHost);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { set_error("nn_query copy-back failed"); st = MVICP_ERR_HIP; }
  }
  dev_free(dq); dev_free(di); dev_free(dd);
  if (c->profile) prof_collect_lazy(c);
  return st;
} MVICP_GUARD_ABI

int mvicp_linearize(mvicp_ctx* c, const double* poses, int point_to_plane, int robust, double* out) try {
  MV_CHECK(bind(c));
  if (!poses || !out) { set_error("null argument"); return MVICP_ERR_ARG; }
  if (c->E == 0) { set_error("no graph"); return MVICP_ERR_STATE; }
  MV_CHECK(evaluate_blocks(c, poses, point_to_plane ? MVICP_METRIC_PLANE : MVICP_METRIC_POINT, robust, out));   // (any non-zero flag is plane)
  if (c->profile) prof_collect_lazy(c);
  return MVICP_OK;
} MVICP_GUARD_ABI

// mvicp_linearize with the objective named: metric 0 / 1 ARE mvicp_linearize(point_to_plane = 0 / 1)
int mvicp_linearize_metric(mvicp_ctx* c, const double* poses, int metric, int robust, double* out) try {
  if (metric != MVICP_METRIC_POINT && metric != MVICP_METRIC_PLANE && metric != MVICP_METRIC_SYMMETRIC) { set_error("metric %d is not an mvicp_metric", metric); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  if (!poses || !out) { set_error("null argument"); return MVICP_ERR_ARG; }
  if (c->E == 0) { set_error("no graph"); return MVICP_ERR_STATE; }
  MV_CHECK(evaluate_blocks(c, poses, metric, robust, out));
  if (c->profile) prof_collect_lazy(c);
  return MVICP_OK;
} MVICP_GUARD_ABI

// The plane-to-plane objective: an entry point of its own because epsilon does not fit mvicp_linearize_metric (mvicp_metric stays as it is)
int mvicp_linearize_gicp(mvicp_ctx* c, const double* poses, double epsilon, int robust, double* out) try {
  if (!gicp_epsilon_ok(epsilon)) { set_error("gicp epsilon %g is not within [1e-6, 1]", epsilon); return MVICP_ERR_ARG; }
  MV_CHECK(bind(c));
  if (!poses || !out) { set_error("null argument"); return MVICP_ERR_ARG; }
  if (c->E == 0) { set_error("no graph"); return MVICP_ERR_STATE; }
  c->gicp_eps = epsilon;
  MV_CHECK(evaluate_blocks(c, poses, kMetricGicp, robust, out));
  if (c->profile) prof_collect_lazy(c);
  return MVICP_OK;
} MVICP_GUARD_ABI

// Two evaluations on the current correspondences in one pass over the operand stream (single rank); see include/mvicp.h
int mvicp_linearize_pair(mvicp_ctx* c, const double* poses_a, const double* poses_b, int point_to_plane, int robust, double* out_a, double* out_b) try {
  MV_CHECK(bind(c));
  if (!poses_a || !poses_b || !out_a || !out_b) { set_error("null argument"); return MVICP_ERR_ARG; }
  if (c->E == 0) { set_error("no graph"); return MVICP_ERR_STATE; }
  if (c->comm || c->ar_fn) {   // an exchange is configured: two ordinary evaluations (one collective each)
    MV_CHECK(evaluate_blocks(c, poses_a, point_to_plane ? MVICP_METRIC_PLANE : MVICP_METRIC_POINT, robust, out_a));
    MV_CHECK(evaluate_blocks(c, poses_b, point_to_plane ? MVICP_METRIC_PLANE : MVICP_METRIC_POINT, robust, out_b));
  } else {
    MV_CHECK(evaluate_pair(c, poses_a, poses_b, point_to_plane ? MVICP_METRIC_PLANE : MVICP_METRIC_POINT, robust, out_a, out_b));
  }
  if (c->profile) prof_collect_lazy(c);
  return MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_set_option(mvicp_ctx* c, const char* name, double value) try {
  MV_CHECK(bind(c));
  if (!name) { set_error("null option name"); return MVICP_ERR_ARG; }
  if (std::strcmp(name, "async_build") == 0) { c->async_build = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "grid_target") == 0 || std::strcmp(name, "grid_curve") == 0) MV_CHECK(finish_builds(c));   // (pending builds read them)
  if (std::strcmp(name, "nn_tree_only") == 0) { c->opt.nn_tree_only = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "nn_cache") == 0) { c->opt.nn_cache_enable = value != 0.0; c->hist.nn_cache_valid = false; return MVICP_OK; }
  if (std::strcmp(name, "lin_chunk") == 0) { c->lin_chunk_override = (int)value; return MVICP_OK; }  // takes effect at the next mvicp_set_graph
  if (std::strcmp(name, "list_reuse") == 0) { c->opt.list_reuse = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "lin_tail_last") == 0) { c->lin_tail_last = value != 0.0; return MVICP_OK; }   // takes effect at the next mvicp_set_graph
  if (std::strcmp(name, "lin_interleave") == 0) { c->lin_interleave = value != 0.0; return MVICP_OK; }   // takes effect at the next mvicp_set_graph
  if (std::strcmp(name, "lin_share_p") == 0) { c->lin_share_p = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "lin_pair") == 0) { c->opt.lin_pair = value != 0.0; return MVICP_OK; }   // 0: the two queued evaluations of a fixed-point round as two launches
  if (std::strcmp(name, "nn_census") == 0) { c->nn_census = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "nn_skip_far") == 0) { c->opt.nn_skip_far = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "sel_bracket") == 0) { c->opt.sel_bracket = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "sel_reuse") == 0) { c->opt.sel_reuse = value != 0.0; return MVICP_OK; }   // 0: launch the median select in every search
  if (std::strcmp(name, "prune_rho") == 0) { c->prune_rho = value; return MVICP_OK; }
  if (std::strcmp(name, "grid_curve") == 0) { c->grid_curve = (int)value; return MVICP_OK; }   // takes effect at the next mvicp_set_frame
  if (std::strcmp(name, "auto_settle") == 0) { c->opt.auto_settle = value; return MVICP_OK; }
  if (std::strcmp(name, "auto_switch") == 0) { c->opt.auto_switch = value; return MVICP_OK; }
  if (std::strcmp(name, "nn_cell") == 0) { c->opt.nn_cell = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "nn_search_factor") == 0) { if (!(value >= 0.0)) { set_error("nn_search_factor < 0"); return MVICP_ERR_ARG; } c->nn_search_factor = value; c->hist.nn_cache_valid = false; return MVICP_OK; }
  if (std::strcmp(name, "tie_rule") == 0) {
    // the rule is an INPUT of every search (which target a tied query gets), not a tuning knob: a change drops what earlier searches left behind —
    // lists, seeds, the "no tie was reported" memory, the exported copy — and gives every edge a new epoch, like mvicp_reset_history
    const bool on = value != 0.0;
    if (on != c->opt.tie_rule) { MV_HIP(hipStreamSynchronize(c->stream)); c->opt.tie_rule = on; forget_history(c); }
    return MVICP_OK;
  }
  if (std::strcmp(name, "tie_lazy") == 0) { c->opt.tie_lazy = value != 0.0; return MVICP_OK; }   // takes effect at the next mvicp_set_graph
  if (std::strcmp(name, "tile_seed") == 0) { c->tile_seed = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "tile_bounds") == 0) { c->opt.tile_bounds = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "tile_mu") == 0) { if (!(value > 0.0 && value <= 1.0)) { set_error("tile_mu outside (0, 1]"); return MVICP_ERR_ARG; } c->opt.tile_mu = value; return MVICP_OK; }
  if (std::strcmp(name, "mfma_kacc") == 0) { if (!(value >= 1.0 && value <= 1024.0)) { set_error("mfma_kacc outside [1, 1024]"); return MVICP_ERR_ARG; } c->mfma_kacc = value; return MVICP_OK; }
  if (std::strcmp(name, "mfma_lbt") == 0) { c->mfma_lbt = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "mfma_entry") == 0) { c->mfma_entry = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "mfma_trig") == 0) { c->mfma_trig = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "tile_mfma") == 0) { c->opt.tile_mfma = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "tile_waves") == 0) { c->tile_waves = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "cache_mfma_ratio") == 0) { c->opt.cache_mfma_ratio = value; return MVICP_OK; }
  if (std::strcmp(name, "reject_cache") == 0) { c->reject_cache = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "tile_miss") == 0) { if (!(value >= 0.0 && value <= 64.0)) { set_error("tile_miss outside [0, 64]"); return MVICP_ERR_ARG; } c->tile_miss = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "tile_cache") == 0) { c->opt.tile_cache = (int)value; return MVICP_OK; }
  if (std::strcmp(name, "voxel_permute") == 0) { c->voxel_permute = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "knn_order") == 0) { c->knn_order = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "match_chunk") == 0) {
    if (!(value >= 1.0 && value < 2147483648.0)) { set_error("match_chunk must be in [1, 2^31)"); return MVICP_ERR_ARG; }
    c->match_chunk = (int)value; return MVICP_OK;
  }
  if (std::strcmp(name, "spin_wait") == 0) { c->spin_wait = value != 0.0; return MVICP_OK; }
  if (std::strcmp(name, "fault_inject") == 0) { c->fault_inject = (int)value; return MVICP_OK; }            // tests: the value-th mvicp_correspond from now fails locally before its exchange
  if (std::strcmp(name, "fault_inject_build") == 0) { c->fault_inject_build.store((int)value); return MVICP_OK; }      // tests: the value-th structure build from now fails
  if (std::strcmp(name, "fault_inject_eval") == 0) { c->fault_inject_eval = (int)value; return MVICP_OK; }  // tests: the value-th exchanged LM evaluation from now fails locally
  if (std::strcmp(name, "spec_eval") == 0) { c->opt.spec_enable = value != 0.0; c->spec_ready = false; c->spec2_ready = false; return MVICP_OK; }
  if (std::strcmp(name, "spec2_eval") == 0) { c->opt.spec2_enable = value != 0.0; c->spec2_ready = false; return MVICP_OK; }
  if (std::strcmp(name, "grid_target") == 0) {
    if (!(value >= 0.5 && value <= 64.0)) { set_error("grid_target out of range"); return MVICP_ERR_ARG; }
    c->grid_target = value;
    return MVICP_OK;
  }
  set_error("unknown option '%s'", name);
  return MVICP_ERR_ARG;
} MVICP_GUARD_ABI
int mvicp_nn_census_ex(mvicp_ctx* c, double* out, int cap) try {
  MV_CHECK(bind(c));
  if (!out || cap < 0) { set_error("bad output buffer"); return MVICP_ERR_ARG; }
  const double v[10] = {c->nn_queries, c->nn_candidates, c->nn_nodes, c->nn_far, c->nn_hits, c->nn_fetched, c->nn_dbg[0], c->nn_dbg[1], c->nn_dbg[2], c->nn_dbg[3]};
  const int n = std::min(cap, 10);
  for (int i = 0; i < n; ++i) out[i] = v[i];
  return n;
} MVICP_GUARD_ABI
const char* mvicp_last_nn_launch(mvicp_ctx* c) { return c ? c->last_nn_launch : ""; }   // (host state only: binds no device, cannot throw)
int mvicp_nn_census(mvicp_ctx* c, double* out5) try {   // the original 5-counter contract (a caller's 5-element buffer is never overrun)
  const int n = mvicp_nn_census_ex(c, out5, 5);
  return n < 0 ? n : MVICP_OK;
} MVICP_GUARD_ABI

int mvicp_profile_enable(mvicp_ctx* c, int on) try {
  MV_CHECK(bind(c));
  c->profile = on != 0;
  c->profile_level = on;
  return MVICP_OK;
} MVICP_GUARD_ABI
int mvicp_profile_reset(mvicp_ctx* c) try {
  MV_CHECK(bind(c));
  MV_HIP(hipStreamSynchronize(c->stream));
  prof_collect(c);
  for (auto& kv : c->prof) { kv.second.ms = 0; kv.second.launches = 0; kv.second.bytes = 0; kv.second.survey_bytes = 0; kv.second.queries = 0; }
  c->nn_candidates = c->nn_nodes = c->nn_far = c->nn_queries = c->nn_hits = c->nn_fetched = 0;
  for (int k = 0; k < 4; ++k) c->nn_dbg[k] = 0;
  return MVICP_OK;
} MVICP_GUARD_ABI
// "nn" = every NN kernel scope together (nn_brute, nn_grid, nn_tile, nn_mfma)
static void prof_sum(mvicp_ctx* c, const char* kernel, double out[5]) {
  for (int k = 0; k < 5; ++k) out[k] = 0.0;
  const std::string key = kernel ? kernel : "";
  for (const auto& kv : c->prof) {
    if (!(kv.first == key || (key == "nn" && kv.first.compare(0, 3, "nn_") == 0))) continue;
    out[0] += kv.second.ms;
    // "nn": the auxiliary scopes (nn_far: phase 2 + list flags, nn_tie: the tie fix-up) add their time, but a search is ONE launch of a primary kernel
    if (key == "nn" && (kv.first == "nn_far" || kv.first == "nn_tie")) continue;
    out[1] += (double)kv.second.launches; out[2] += kv.second.bytes; out[3] += kv.second.survey_bytes; out[4] += kv.second.queries;
  }
}
int mvicp_profile_get(mvicp_ctx* c, const char* kernel, double* total_ms, long long* launches, double* alg_bytes) try {
  MV_CHECK(bind(c));
  MV_HIP(hipStreamSynchronize(c->stream));
  prof_collect(c);
  double v[5];
  prof_sum(c, kernel, v);
  if (total_ms) *total_ms = v[0];
  if (launches) *launches = (long long)v[1];
  if (alg_bytes) *alg_bytes = v[2];
  return MVICP_OK;
} MVICP_GUARD_ABI
int mvicp_profile_get_ex(mvicp_ctx* c, const char* kernel, double* out, int cap) try {
  MV_CHECK(bind(c));
  if (!out || cap < 0) { set_error("bad output buffer"); return MVICP_ERR_ARG; }
  MV_HIP(hipStreamSynchronize(c->stream));
  prof_collect(c);
  double v[5];
  prof_sum(c, kernel, v);
  const int n = std::min(cap, 5);
  for (int k = 0; k < n; ++k) out[k] = v[k];
  return n;
} MVICP_GUARD_ABI
void* mvicp_stream(mvicp_ctx* c) { return c ? (void*)c->stream : nullptr; }
int mvicp_sync(mvicp_ctx* c) try {
  MV_CHECK(bind(c));
  MV_HIP(hipStreamSynchronize(c->stream));
  return MVICP_OK;
} MVICP_GUARD_ABI

}  // extern "C"
