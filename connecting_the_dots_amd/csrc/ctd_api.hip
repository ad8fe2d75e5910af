// ctd_api.hip -- the extern "C" surface declared in include/ctd_hip.h.
// Argument validation lives here; kernels assume validated shapes.
#include "ctd_internal.h"
#include "ctd_prepass.h"
#include "../../include/ctd_hip_bench.h"

#include <deque>
#include <utility>
#include <vector>

using namespace ctd;

namespace ctd {
// Bench instrumentation (include/ctd_hip_bench.h, ctd_kernel_timing_*): NOT part of the drop-in ABI of
// include/ctd_hip.h.  The state is per calling thread (thread_local): the thread that enables it sees its own launches
// only, other threads of the process launch un-instrumented and race with nothing.
// The events come from a pool created when timing is switched on (no hipEventCreate between launches) and carry
// hipEventDisableSystemFence: a default event makes the queue release to system scope at every record (an L2
// write-back of whatever the previous kernel left dirty), which the un-instrumented path never pays.
static thread_local bool g_timing = false;
static thread_local int g_timing_columns = 0;
static thread_local std::deque<hipEvent_t> g_pool;                                    // free events, reused first-in first-out
static thread_local std::vector<std::pair<hipEvent_t, hipEvent_t>> g_events;          // recorded (start, stop) pairs
static thread_local hipEvent_t g_pending = nullptr;
static hipEvent_t pool_get() {
  if (!g_pool.empty()) {
    hipEvent_t e = g_pool.front();
    g_pool.pop_front();
    return e;
  }
  hipEvent_t e = nullptr;
  if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return nullptr;
  return e;
}
bool timing_enabled() { return g_timing; }
void timing_begin(hipStream_t stream) {
  if (!g_timing) return;
  if (!g_pending) g_pending = pool_get();            // (a launch that failed between begin and end left its event here)
  if (g_pending) (void)hipEventRecord(g_pending, stream);
}
void timing_end(hipStream_t stream, int columns) {
  if (!g_timing || !g_pending) return;
  hipEvent_t stop = pool_get();
  if (!stop) return;
  (void)hipEventRecord(stop, stream);
  g_events.emplace_back(g_pending, stop);
  g_pending = nullptr;
  g_timing_columns = columns;
}
}  // namespace ctd

extern "C" {

int ctd_version(void) { return 5; }

void ctd_kernel_timing_enable(int enable) {
  g_timing = enable != 0;
  if (g_timing) {
    // fill the pool up front (enough for a default bench region) and record every new event once: the runtime
    // allocates an event's signal at its first record, and that must not happen between the start event and the
    // kernel it brackets
    bool fresh = false;
    const size_t want = enable > 128 ? (size_t)enable : 128;          // `enable` doubles as the number of events to hold ready
    while (g_pool.size() < want) {
      hipEvent_t e = nullptr;
      if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) break;
      (void)hipEventRecord(e, nullptr);
      g_pool.push_back(e);
      fresh = true;
    }
    if (fresh) (void)hipStreamSynchronize(nullptr);
  } else if (g_pending) {
    g_pool.push_back(g_pending);
    g_pending = nullptr;
  }
}

int ctd_kernel_timing_collect(double* avg_ms, int* columns) {
  double total = 0;
  int n = 0;
  for (auto& ev : g_events) {
    float ms = 0.f;
    if (hipEventSynchronize(ev.second) == hipSuccess && hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
      total += ms;
      ++n;
    }
    g_pool.push_back(ev.first);
    g_pool.push_back(ev.second);
  }
  g_events.clear();
  if (avg_ms) *avg_ms = n ? total / n : 0.0;
  if (columns) *columns = g_timing_columns;
  return n;
}

const char* ctd_status_string(int status) {
  switch (status) {
    case CTD_OK: return "ok";
    case CTD_ERR_INVALID_ARG: return "invalid argument";
    case CTD_ERR_WORKSPACE: return "workspace missing or too small";
    case CTD_ERR_UNSUPPORTED: return "unsupported parameter combination";
    default: break;
  }
  if (status >= CTD_ERR_HIP) return hipGetErrorString((hipError_t)(status - CTD_ERR_HIP));
  return "unknown status";
}

static bool vol_shape_ok(int frames, int C, int H, int W, int D, int bs) {
  if (frames < 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0 || bs <= 0) return false;
  // the reference indexes outputs with int (common_cuda.h:65-66, ext_cpu.cpp:8-9)
  if ((double)D * H * W >= 2147483648.0) return false;
  return true;
}

size_t ctd_xcorrvol_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size)) return 0;
  // worst case over "pattern shared" / "pattern per frame"
  size_t exact = ncc_exact_workspace_bytes(frames, C, H, W, D, block_size, true);
  if (algo == CTD_NCC_EXACT) return exact;
  size_t fast = ncc_fast_workspace_bytes(frames, C, H, W, D, block_size, true);
  return fast > exact ? fast : exact;
}

int ctd_xcorrvol_pattern_prepare_f32(const float* in1, long in1_frame_stride, int frames, int C, int H, int W, int D,
                                     int block_size, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || in1_frame_stride < 0 || frames == 0 || !in1) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return ncc_fast_prepare_pattern_f32(in1, in1_frame_stride, frames, C, H, W, D, block_size, workspace, workspace_bytes,
                                      (hipStream_t)stream);
}

int ctd_xcorrvol_f32(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames, int C, int H,
                     int W, int D, int block_size, int algo, void* workspace, size_t workspace_bytes, int device,
                     void* stream) {
  const bool prepared = (algo & CTD_PATTERN_PREPARED) != 0;
  algo &= ~CTD_PATTERN_PREPARED;
  if (prepared && algo != CTD_NCC_FAST) return CTD_ERR_INVALID_ARG;
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || in1_frame_stride < 0) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !out) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  if (algo == CTD_NCC_EXACT)
    return ncc_exact_f32(in0, in1, in1_frame_stride, out, frames, C, H, W, D, block_size, workspace, workspace_bytes,
                         (hipStream_t)stream);
  if (algo == CTD_NCC_FAST)
    return ncc_fast_f32(in0, in1, in1_frame_stride, out, frames, C, H, W, D, block_size, workspace, workspace_bytes,
                        nullptr, prepared, (hipStream_t)stream);
  return CTD_ERR_INVALID_ARG;
}

int ctd_xcorrvol_f64(const double* in0, const double* in1, long in1_frame_stride, double* out, int frames, int C,
                     int H, int W, int D, int block_size, void* workspace, size_t workspace_bytes, int device,
                     void* stream) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || in1_frame_stride < 0) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !out) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return ncc_exact_f64(in0, in1, in1_frame_stride, out, frames, C, H, W, D, block_size, workspace, workspace_bytes,
                       (hipStream_t)stream);
}

int ctd_argmax_disp_f32(const float* vol, int64_t* idx, float* best, int frames, int D, int H, int W, int device,
                        void* stream) {
  if (frames < 0 || D <= 0 || H <= 0 || W <= 0) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!vol || !idx) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return argmax_disp_f32(vol, idx, best, frames, D, H, W, (hipStream_t)stream);
}

int ctd_xcorrvol_rank_supported(int C, int H, int W, int D, int block_size) {
  return vol_shape_ok(1, C, H, W, D, block_size) && ncc_fast_rank_supported(C, H, W, D, block_size) ? 1 : 0;
}

int ctd_xcorrvol_rank_layout(int frames, int H, int W, int D, int per_frame_pattern, size_t* offsets) {
  if (!offsets || frames <= 0 || !vol_shape_ok(frames, 1, H, W, D, 9)) return CTD_ERR_INVALID_ARG;
  ncc_fast_rank_offsets(frames, H, W, D, per_frame_pattern != 0, offsets);
  return CTD_OK;
}

size_t ctd_xcorrvol_argmax_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo) {
  size_t base = ctd_xcorrvol_workspace_bytes(frames, C, H, W, D, block_size, algo);
  if (base == 0 || algo != CTD_NCC_FAST) return base;
  // old path: work list behind a 16-byte counter at the start of the workspace
  size_t need = 16 + sizeof(int64_t) * (size_t)frames * H * W;
  if (ncc_fast_rank_supported(C, H, W, D, block_size)) need = ncc_fast_rank_workspace_bytes(frames, H, W, D, true);
  return need > base ? need : base;
}

int ctd_xcorrvol_argmax_f32(const float* in0, const float* in1, long in1_frame_stride, float* vol_out, int64_t* idx,
                            float* best, int frames, int C, int H, int W, int D, int block_size, int algo,
                            float rerank_eps, void* workspace, size_t workspace_bytes, int device, void* stream) {
  const bool prepared = (algo & CTD_PATTERN_PREPARED) != 0;
  algo &= ~CTD_PATTERN_PREPARED;
  if (prepared && algo != CTD_NCC_FAST) return CTD_ERR_INVALID_ARG;
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || in1_frame_stride < 0) return CTD_ERR_INVALID_ARG;
  if (C != 1) return CTD_ERR_UNSUPPORTED;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !idx) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  if (algo == CTD_NCC_EXACT)
    return ncc_exact_argmax_f32(in0, in1, in1_frame_stride, vol_out, idx, best, frames, H, W, D, block_size, workspace,
                                workspace_bytes, (hipStream_t)stream);
  if (algo == CTD_NCC_FAST) {
    if (rerank_eps != rerank_eps) return CTD_ERR_INVALID_ARG;
    // rerank_eps < 0 (plain argmax of the fast scores, no exact re-scoring) is defined on a materialised volume: the
    // scores of listed windows exist only there (fix-up pass), so such a call ranks the patched volume in one more pass
    const bool plain = rerank_eps < 0.f && vol_out;
    if (!plain && ncc_fast_rank_supported(1, H, W, D, block_size) && ((uintptr_t)vol_out) % 16 == 0) {
      // ranked inside the all-D volume kernel: {top, runner-up} per pixel in LDS across every disparity; the kernel
      // writes idx / best / work list itself -- no partial planes, no merge, no pass over the volume
      RankPlan rp;
      rp.eps = rerank_eps < 0.f ? 0.f : rerank_eps;                        // (no volume: negative eps means 0)
      rp.idx = idx;
      rp.best = best;
      const hipStream_t hs = (hipStream_t)stream;
      int st = ncc_fast_f32(in0, in1, in1_frame_stride, vol_out, frames, 1, H, W, D, block_size, workspace,
                            workspace_bytes, &rp, prepared, hs);       // pre-pass + all-D kernel
      if (st) return st;
      st = ncc_fast_fixup_ranked(in0, in1, in1_frame_stride, vol_out, frames, H, W, D, block_size, workspace, rp, rp.best, hs);
      if (st) return st;
      return rank_tail_f32(rp, vol_out, in0, in1, in1_frame_stride, idx, rp.best, frames, D, H, W, block_size, hs);
    }
    if (!vol_out) return CTD_ERR_INVALID_ARG;                              // this shape ranks a materialised volume
    int st = ncc_fast_f32(in0, in1, in1_frame_stride, vol_out, frames, 1, H, W, D, block_size, workspace,
                          workspace_bytes, nullptr, prepared, (hipStream_t)stream);
    if (st) return st;
    return argmax_rerank_f32(vol_out, in0, in1, in1_frame_stride, idx, best, frames, D, H, W, block_size, rerank_eps,
                             workspace, workspace_bytes, /*counter_cleared=*/true, (hipStream_t)stream);
  }
  return CTD_ERR_INVALID_ARG;
}

int ctd_lcn_xcorrvol_supported(int H, int W, int D, int radius, int block_size) {
  return vol_shape_ok(1, 1, H, W, D, block_size) && ncc_fast_rank_supported(1, H, W, D, block_size) &&
                 lcn_stream_supported(H, W, radius, block_size) ? 1 : 0;
}

int ctd_lcn_xcorrvol_argmax_f32(const float* raw, float* lcn_out, float* std_out, int radius, float lcn_eps, int lcn_algo,
                                const float* in1, long in1_frame_stride, float* vol_out, int64_t* idx, float* best,
                                int frames, int H, int W, int D, int block_size, int algo, float rerank_eps,
                                void* workspace, size_t workspace_bytes, int device, void* stream) {
  const bool prepared = (algo & CTD_PATTERN_PREPARED) != 0;
  algo &= ~CTD_PATTERN_PREPARED;
  if (algo != CTD_NCC_FAST || (lcn_algo != CTD_LCN_EXACT && lcn_algo != CTD_LCN_FAST)) return CTD_ERR_INVALID_ARG;
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || in1_frame_stride < 0 || radius < 0 || rerank_eps != rerank_eps)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!raw || !lcn_out || !std_out || !in1 || !idx) return CTD_ERR_INVALID_ARG;
  if (!ctd_lcn_xcorrvol_supported(H, W, D, radius, block_size) || ((uintptr_t)vol_out) % 16 != 0) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  const FusedLcn fused = {raw, std_out, radius, lcn_eps, lcn_algo == CTD_LCN_EXACT};
  RankPlan rp;
  rp.eps = rerank_eps < 0.f ? 0.f : rerank_eps;             // (as ctd_xcorrvol_argmax_f32 without a plain-argmax pass)
  rp.idx = idx;
  rp.best = best;
  int st = ncc_fast_f32(lcn_out, in1, in1_frame_stride, vol_out, frames, 1, H, W, D, block_size, workspace, workspace_bytes,
                        &rp, prepared, hs, &fused);           // streaming LCN + statistics, then the all-D kernel
  if (st) return st;
  st = ncc_fast_fixup_ranked(lcn_out, in1, in1_frame_stride, vol_out, frames, H, W, D, block_size, workspace, rp, rp.best, hs);
  if (st) return st;
  return rank_tail_f32(rp, vol_out, lcn_out, in1, in1_frame_stride, idx, rp.best, frames, D, H, W, block_size, hs);
}

int ctd_lcn_f32(const float* x, float* y, float* std_out, int N, int H, int W, int radius, float eps, int device,
                void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || radius < 0 || radius >= H || radius >= W || (double)H * W >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!x || !y || !std_out) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return lcn_f32(x, y, std_out, N, H, W, radius, eps, (hipStream_t)stream);
}

int ctd_lcn_fast_f32(const float* x, float* y, float* std_out, int N, int H, int W, int radius, float eps, int device,
                     void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || radius < 0 || radius >= H || radius >= W || (double)H * W >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!x || !y || !std_out) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return lcn_fast_f32(x, y, std_out, N, H, W, radius, eps, (hipStream_t)stream);
}

int ctd_lcn_datagen_f32(const float* img, float* out, float* out_std, int N, int H, int W, int kernel_size, float eps,
                        int device, void* stream) {
  if (N < 0 || H <= 0 || W <= 0 || kernel_size < 0 || N > 65535) return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!img || !out || !out_std) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return lcn_datagen_f32(img, out, out_std, N, H, W, kernel_size, eps, (hipStream_t)stream);
}

static bool photo_shape_ok(int B, int C, int H, int W, int bs, int type) {
  return B >= 0 && C > 0 && H > 0 && W > 0 && bs > 0 && type >= 0 && type <= 3 &&
         (double)B * C * H * W < 2147483648.0;                 // int indices in the reference (ext.h:220-235)
}

#define CTD_PHOTO_ENTRY(SFX, T)                                                                                   \
  int ctd_photometric_fwd_##SFX(const T* es, const T* ta, T* out, int B, int C, int H, int W, int block_size,      \
                                int type, float eps, int device, void* stream) {                                   \
    if (!photo_shape_ok(B, C, H, W, block_size, type)) return CTD_ERR_INVALID_ARG;                                 \
    if (B == 0) return CTD_OK;                                                                                     \
    if (!es || !ta || !out) return CTD_ERR_INVALID_ARG;                                                            \
    DeviceGuard g(device);                                                                                         \
    if (g.status) return g.status;                                                                                 \
    return photometric_fwd_##SFX(es, ta, out, B, C, H, W, block_size, type, eps, (hipStream_t)stream);             \
  }                                                                                                                \
  int ctd_photometric_bwd_##SFX(const T* es, const T* ta, const T* grad_out, T* grad_es, int B, int C, int H,      \
                                int W, int block_size, int type, float eps, int device, void* stream) {            \
    if (!photo_shape_ok(B, C, H, W, block_size, type)) return CTD_ERR_INVALID_ARG;                                 \
    if (B == 0) return CTD_OK;                                                                                     \
    if (!es || !ta || !grad_out || !grad_es) return CTD_ERR_INVALID_ARG;                                           \
    DeviceGuard g(device);                                                                                         \
    if (g.status) return g.status;                                                                                 \
    return photometric_bwd_##SFX(es, ta, grad_out, grad_es, B, C, H, W, block_size, type, eps, (hipStream_t)stream); \
  }
CTD_PHOTO_ENTRY(f32, float)
CTD_PHOTO_ENTRY(f64, double)
CTD_PHOTO_ENTRY(fast_f32, float)
#undef CTD_PHOTO_ENTRY

static bool img_shape_ok(int B, int H, int W);

size_t ctd_pattern_loss_workspace_bytes(int B, int H, int W) {
  return img_shape_ok(B, H, W) ? pattern_loss_workspace_bytes(B, H, W) : 0;
}

int ctd_pattern_loss_fwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                             float* pattern_proj, float* terms, int B, int H, int W, int type, float eps,
                             void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  if (!disp || !im || !pattern || !pattern_proj || !terms) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_fwd_f32(disp, im, mask, pattern, pattern_proj, terms, B, H, W, type, eps, workspace, workspace_bytes,
                              (hipStream_t)stream);
}

int ctd_pattern_loss_bwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                             const float* terms, const float* grad_val, const float* grad_proj, float* grad_disp,
                             int B, int H, int W, int type, float eps, int device, void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  if (!disp || !im || !pattern || !terms || !grad_val || !grad_disp) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_bwd_f32(disp, im, mask, pattern, terms, grad_val, grad_proj, grad_disp, B, H, W, type, eps,
                              (hipStream_t)stream);
}

size_t ctd_pattern_loss_multi_workspace_bytes(int n_levels, const ctd_pattern_level* levels) {
  return pattern_loss_multi_workspace_bytes(n_levels, levels);
}

int ctd_pattern_loss_multi_fwd_f32(int n_levels, const ctd_pattern_level* levels, float* terms, int type, float eps,
                                   void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!terms || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_multi_fwd_f32(n_levels, levels, terms, type, eps, workspace, workspace_bytes, (hipStream_t)stream);
}

int ctd_pattern_loss_multi_bwd_f32(int n_levels, const ctd_pattern_level* levels, const float* terms,
                                   const float* grad_vals, int type, float eps, int device, void* stream) {
  if (!terms || !grad_vals || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_multi_bwd_f32(n_levels, levels, terms, grad_vals, type, eps, (hipStream_t)stream);
}

int ctd_costvol_f32(const float* im, const float* pattern, long pattern_frame_stride, float* cost, int frames, int H,
                    int W, int D, int block_size, int type, float eps, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || pattern_frame_stride < 0 ||
      (long)frames * D > 65535)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !cost) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_f32(im, pattern, pattern_frame_stride, cost, frames, H, W, D, block_size, type, eps,
                     (hipStream_t)stream);
}

size_t ctd_costvol_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3) return 0;
  if (!costvol_sep_supported(H, W, D, block_size, type)) return 0;          // the other kernels need none
  return costvol_sep_workspace_bytes(frames, H, W, D, per_frame_pattern != 0);
}

int ctd_costvol_fast_f32(const float* im, const float* pattern, long pattern_frame_stride, float* cost, int frames, int H,
                         int W, int D, int block_size, int type, float eps, void* workspace, size_t workspace_bytes,
                         int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || pattern_frame_stride < 0)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !cost) return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_fast_f32(im, pattern, pattern_frame_stride, cost, frames, H, W, D, block_size, type, eps, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

size_t ctd_costvol_argmin_workspace_bytes(int frames, int H, int W, int D, int block_size, int type,
                                          int per_frame_pattern) {
  (void)per_frame_pattern;                                                  // (the layout does not depend on it)
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || (block_size & 1) == 0) return 0;
  if (!costvol_rank_supported(frames, H, W, D, block_size)) return 0;
  return costvol_argmin_workspace_bytes(frames, H, W, D);
}

int ctd_costvol_argmin_f32(const float* im, const float* pattern, long pattern_frame_stride, int64_t* idx, float* best,
                           int frames, int H, int W, int D, int block_size, int type, float eps, float rerank_rel,
                           void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || (block_size & 1) == 0 ||
      pattern_frame_stride < 0 || rerank_rel != rerank_rel)
    return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !idx) return CTD_ERR_INVALID_ARG;
  if (!costvol_rank_supported(frames, H, W, D, block_size)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_argmin_f32(im, pattern, pattern_frame_stride, idx, best, frames, H, W, D, block_size, type, eps,
                            rerank_rel, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t ctd_xcorrvol_subpixel_workspace_bytes(int frames, int H, int W, int D, int block_size, int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0) return 0;
  return xcorrvol_subpixel_workspace_bytes(frames, H, W, D, per_frame_pattern != 0);
}

int ctd_xcorrvol_subpixel_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                              float* disp, uint8_t* refined, int frames, int H, int W, int D, int block_size, int mode,
                              void* workspace, size_t workspace_bytes, int device, void* stream) {
  const bool prepared = (mode & CTD_PATTERN_PREPARED) != 0;
  mode &= ~CTD_PATTERN_PREPARED;
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0 ||
      (mode != CTD_SUBPIXEL_PARABOLA && mode != CTD_SUBPIXEL_EQUIANGULAR))
    return CTD_ERR_INVALID_ARG;
  if (in1_frame_stride != 0 && in1_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !idx || !disp) return CTD_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < xcorrvol_subpixel_workspace_bytes(frames, H, W, D, in1_frame_stride != 0))
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return xcorrvol_subpixel_f32(in0, in1, in1_frame_stride, idx, disp, refined, frames, H, W, D, block_size, mode,
                               prepared, workspace, (hipStream_t)stream);
}

int ctd_costvol_subpixel_f32(const float* im, const float* pattern, long pattern_frame_stride, const int64_t* idx,
                             float* disp, uint8_t* refined, int frames, int H, int W, int D, int block_size, int type,
                             float eps, int mode, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0 || type < 0 || type > 3 ||
      (mode != CTD_SUBPIXEL_PARABOLA && mode != CTD_SUBPIXEL_EQUIANGULAR))
    return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !idx || !disp) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_subpixel_f32(im, pattern, pattern_frame_stride, idx, disp, refined, frames, H, W, D, block_size, type,
                              eps, mode, (hipStream_t)stream);
}

// ---- match validity (match_validity.hip) ----
static bool validity_args_ok(int lr_tol, float min_gap) { return lr_tol >= 0 && min_gap >= 0.f; }   // (a NaN fails >=)
static bool validity_block_fast(int bs) { return bs == 3 || bs == 5 || bs == 7 || bs == 9; }

int ctd_match_validity_f32(const float* vol, int maximise, const int64_t* idx, uint8_t* flags, int64_t* idx_r, float* gap,
                           int frames, int D, int H, int W, int lr_tol, float min_gap, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, 1) || !validity_args_ok(lr_tol, min_gap)) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!vol || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!match_validity_supported(frames, H, W)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  int st = match_validity_scan_f32(vol, maximise != 0, false, idx, flags, idx_r, gap, frames, D, H, W, min_gap, nullptr,
                                   nullptr, nullptr, hs);
  if (st) return st;
  return match_validity_flags(idx, idx_r, flags, frames, H, W, lr_tol, hs);
}

// scan of the volume in the workspace, exact re-scoring of the listed items (fast volumes), flag pass
static int validity_finish(const ValidityLayout& l, void* workspace, bool fast, int family, const float* in0,
                           const float* in1, long in1_frame_stride, const int64_t* idx, uint8_t* flags, int64_t* idx_r,
                           float* gap, int frames, int H, int W, int D, int bs, float eps, int lr_tol, float min_gap,
                           hipStream_t hs) {
  char* ws = (char*)workspace;
  unsigned* counters = (unsigned*)(ws + l.counters);
  unsigned* pix_list = (unsigned*)(ws + l.pix_list);
  unsigned* col_list = (unsigned*)(ws + l.col_list);
  int st = match_validity_scan_f32((const float*)(ws + l.vol), family == 4, fast, idx, flags, idx_r, gap, frames, D, H, W,
                                   min_gap, counters, pix_list, col_list, hs);
  if (st) return st;
  if (fast) {
    st = match_validity_rescore_f32(family, in0, in1, in1_frame_stride, idx, flags, idx_r, gap, frames, H, W, D, bs, eps,
                                    min_gap, counters, pix_list, col_list, hs);
    if (st) return st;
  }
  return match_validity_flags(idx, idx_r, flags, frames, H, W, lr_tol, hs);
}

static bool xcorrvol_validity_algo_ok(int C, int D, int bs, int algo) {
  return algo == CTD_NCC_EXACT || (C == 1 && validity_block_fast(bs) && D <= 512);
}

size_t ctd_xcorrvol_validity_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || frames == 0 || (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST)) return 0;
  if (!match_validity_supported(frames, H, W) || !xcorrvol_validity_algo_ok(C, D, block_size, algo)) return 0;
  return validity_layout(frames, H, W, D, ctd_xcorrvol_workspace_bytes(frames, C, H, W, D, block_size, algo)).bytes;
}

int ctd_xcorrvol_validity_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                              uint8_t* flags, int64_t* idx_r, float* gap, int frames, int C, int H, int W, int D,
                              int block_size, int algo, int lr_tol, float min_gap, void* workspace,
                              size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || !validity_args_ok(lr_tol, min_gap) ||
      (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST))
    return CTD_ERR_INVALID_ARG;
  if (in1_frame_stride != 0 && in1_frame_stride != (long)C * H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!match_validity_supported(frames, H, W) || !xcorrvol_validity_algo_ok(C, D, block_size, algo)) return CTD_ERR_UNSUPPORTED;
  const ValidityLayout l = validity_layout(frames, H, W, D, ctd_xcorrvol_workspace_bytes(frames, C, H, W, D, block_size, algo));
  if (!workspace || workspace_bytes < l.bytes || ((uintptr_t)workspace & 255)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  char* ws = (char*)workspace;
  CTD_HIP_TRY(hipMemsetAsync(ws + l.counters, 0, 2 * sizeof(unsigned), hs));
  int st = ctd_xcorrvol_f32(in0, in1, in1_frame_stride, (float*)(ws + l.vol), frames, C, H, W, D, block_size, algo,
                            ws + l.inner, l.bytes - l.inner, -1, stream);
  if (st) return st;
  return validity_finish(l, workspace, algo == CTD_NCC_FAST, 4, in0, in1, in1_frame_stride, idx, flags, idx_r, gap, frames,
                         H, W, D, block_size, 0.f, lr_tol, min_gap, hs);
}

static bool costvol_validity_algo_ok(int frames, int D, int bs, int algo) {
  return algo == CTD_NCC_FAST ? validity_block_fast(bs) : (long)frames * D <= 65535;   // (the grid of ctd_costvol_f32)
}

size_t ctd_costvol_validity_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int algo,
                                            int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || frames == 0 || type < 0 || type > 3 ||
      (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST))
    return 0;
  if (!match_validity_supported(frames, H, W) || !costvol_validity_algo_ok(frames, D, block_size, algo)) return 0;
  const size_t inner = algo == CTD_NCC_FAST ? ctd_costvol_workspace_bytes(frames, H, W, D, block_size, type, per_frame_pattern) : 0;
  return validity_layout(frames, H, W, D, inner).bytes;
}

int ctd_costvol_validity_f32(const float* im, const float* pattern, long pattern_frame_stride, const int64_t* idx,
                             uint8_t* flags, int64_t* idx_r, float* gap, int frames, int H, int W, int D, int block_size,
                             int type, float eps, int algo, int lr_tol, float min_gap, void* workspace,
                             size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || !validity_args_ok(lr_tol, min_gap) ||
      (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST))
    return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!match_validity_supported(frames, H, W) || !costvol_validity_algo_ok(frames, D, block_size, algo)) return CTD_ERR_UNSUPPORTED;
  const bool fast = algo == CTD_NCC_FAST;
  const size_t inner = fast ? ctd_costvol_workspace_bytes(frames, H, W, D, block_size, type, pattern_frame_stride != 0) : 0;
  const ValidityLayout l = validity_layout(frames, H, W, D, inner);
  if (!workspace || workspace_bytes < l.bytes || ((uintptr_t)workspace & 255)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  char* ws = (char*)workspace;
  CTD_HIP_TRY(hipMemsetAsync(ws + l.counters, 0, 2 * sizeof(unsigned), hs));
  float* vol = (float*)(ws + l.vol);
  int st = fast ? ctd_costvol_fast_f32(im, pattern, pattern_frame_stride, vol, frames, H, W, D, block_size, type, eps,
                                       inner ? ws + l.inner : nullptr, inner, -1, stream)
                : ctd_costvol_f32(im, pattern, pattern_frame_stride, vol, frames, H, W, D, block_size, type, eps, -1, stream);
  if (st) return st;
  return validity_finish(l, workspace, fast, type, im, pattern, pattern_frame_stride, idx, flags, idx_r, gap, frames, H, W, D,
                         block_size, eps, lr_tol, min_gap, hs);
}

// ---- semi-global aggregation (sgm.hip) ----
static bool sgm_args_ok(int frames, int D, int H, int W, int paths, float p1, float p2) {
  if (frames <= 0 || D <= 0 || H <= 0 || W <= 0 || (paths != 4 && paths != 8)) return false;
  if ((double)frames * D * H * W >= 2147483648.0) return false;
  return p1 >= 0.f && p2 >= p1 && p2 <= 3.402823466e38f;                                       // (a NaN fails >=)
}

size_t ctd_sgm_workspace_bytes(int frames, int D, int H, int W, int paths, int want_volume) {
  if (!sgm_args_ok(frames, D, H, W, paths, 0.f, 0.f) || !sgm_supported(frames, D, H, W) || want_volume) return 0;
  return sizeof(float) * (size_t)frames * D * H * W;
}

int ctd_sgm_aggregate_f32(const float* vol, int maximise, float p1, float p2, int paths, float* S_out, int64_t* idx,
                          float* best, int frames, int D, int H, int W, void* workspace, size_t workspace_bytes,
                          int device, void* stream) {
  if (!sgm_args_ok(frames, D, H, W, paths, p1, p2)) return CTD_ERR_INVALID_ARG;
  if (!vol || !idx || !best) return CTD_ERR_INVALID_ARG;
  if (!sgm_supported(frames, D, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!S_out && (!workspace || workspace_bytes < ctd_sgm_workspace_bytes(frames, D, H, W, paths, 0) ||
                 ((uintptr_t)workspace & 15)))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return sgm_aggregate_f32(vol, maximise != 0, p1, p2, paths, S_out ? S_out : (float*)workspace, idx, best, frames, D, H, W,
                           (hipStream_t)stream);
}

// ---- disparity post-filters (disp_filter.hip) ----
static bool disp_filter_args_ok(int frames, int H, int W) {
  return frames >= 0 && H > 0 && W > 0 && (double)H * W < 2147483648.0 && (double)frames * H * W < 2147483648.0;
}

static bool disp_link_args_ok(float max_diff, int connectivity) {
  return max_diff >= 0.f && (connectivity == 4 || connectivity == 8);                           // (a NaN fails >=)
}

size_t ctd_disp_components_workspace_bytes(int frames, int H, int W) {
  if (frames <= 0 || !disp_filter_args_ok(frames, H, W)) return 0;
  return sizeof(int) * disp_components_workspace_ints(frames, H, W);
}

static int disp_components_call(const float* disp, const uint8_t* valid, float max_diff, int connectivity, int max_size,
                                int32_t* label, int32_t* size, uint8_t* keep, int frames, int H, int W, void* workspace,
                                size_t workspace_bytes, int device, void* stream) {
  if (frames == 0) return CTD_OK;
  if (!disp_filter_supported(frames, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < ctd_disp_components_workspace_bytes(frames, H, W) || ((uintptr_t)workspace & 15))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disp_components_f32(disp, valid, max_diff, connectivity, max_size, label, size, keep, frames, H, W,
                             (int*)workspace, (hipStream_t)stream);
}

int ctd_disp_components_f32(const float* disp, const uint8_t* valid, float max_diff, int connectivity, int32_t* label,
                            int32_t* size, int frames, int H, int W, void* workspace, size_t workspace_bytes, int device,
                            void* stream) {
  if (!disp_filter_args_ok(frames, H, W) || !disp_link_args_ok(max_diff, connectivity)) return CTD_ERR_INVALID_ARG;
  if (!disp || !label || !size) return CTD_ERR_INVALID_ARG;
  return disp_components_call(disp, valid, max_diff, connectivity, 0, label, size, nullptr, frames, H, W, workspace,
                              workspace_bytes, device, stream);
}

int ctd_disp_speckle_f32(const float* disp, const uint8_t* valid, float max_diff, int max_size, int connectivity,
                         uint8_t* keep, int32_t* size, int frames, int H, int W, void* workspace, size_t workspace_bytes,
                         int device, void* stream) {
  if (!disp_filter_args_ok(frames, H, W) || !disp_link_args_ok(max_diff, connectivity) || max_size < 0)
    return CTD_ERR_INVALID_ARG;
  if (!disp || !keep) return CTD_ERR_INVALID_ARG;
  return disp_components_call(disp, valid, max_diff, connectivity, max_size, nullptr, size, keep, frames, H, W, workspace,
                              workspace_bytes, device, stream);
}

int ctd_disp_median_f32(const float* disp, const uint8_t* valid, int window, int fill_min, float* out, uint8_t* valid_out,
                        int frames, int H, int W, int device, void* stream) {
  if (!disp_filter_args_ok(frames, H, W) || (window != 3 && window != 5 && window != 7) || fill_min < 0)
    return CTD_ERR_INVALID_ARG;
  if (!disp || !out || !valid_out || out == disp || (const uint8_t*)valid_out == valid) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!disp_filter_supported(frames, H, W)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disp_median_f32(disp, valid, window, fill_min, out, valid_out, frames, H, W, (hipStream_t)stream);
}

// ---- multi-view depth consistency and point fusion (depth_fusion.hip) ----
static bool depth_fusion_sizes_ok(int B, int V, int H, int W) {
  // H, W <= 2^24: the bounds of the projected pixel are compared in f32, where W - 1 and H - 1 must be exact
  return B >= 0 && V >= 1 && H >= 1 && W >= 1 && H <= (1 << 24) && W <= (1 << 24) &&
         (double)B * V * H * W < 2147483648.0;
}

static bool depth_fusion_params_ok(float max_px, float max_rel, int min_views) {
  const float big = 3.402823466e38f;                                                          // (a NaN fails >=)
  return max_px >= 0.f && max_px <= big && max_rel >= 0.f && max_rel <= big && min_views >= 0 && min_views <= 255;
}

struct Span {
  const void* p;
  size_t bytes;
};
// true when one of the first n_out spans (the buffers a call writes) shares a byte with any other span; NULL spans are absent
static bool spans_overlap(const Span* s, int n_out, int n) {
  for (int i = 0; i < n_out; ++i)
    for (int j = 0; j < n; ++j) {
      if (j == i || (j < n_out && j < i) || !s[i].p || !s[j].p || !s[i].bytes || !s[j].bytes) continue;
      const uintptr_t a = (uintptr_t)s[i].p, b = (uintptr_t)s[j].p;
      if (a < b + s[j].bytes && b < a + s[i].bytes) return true;
    }
  return false;
}

int ctd_depth_consistency_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                              const float* t, float max_px, float max_rel, int min_views, uint8_t* count, uint8_t* keep,
                              float* fused, int B, int V, int H, int W, int device, void* stream) {
  if (!depth_fusion_sizes_ok(B, V, H, W) || !depth_fusion_params_ok(max_px, max_rel, min_views)) return CTD_ERR_INVALID_ARG;
  if (!depth || !ray || !K || !R || !t || !count || !keep || !fused) return CTD_ERR_INVALID_ARG;
  if (V > 64 || !depth_fusion_supported(B, V, H, W)) return CTD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * V * H * W, views = (size_t)B * V;
  const Span s[] = {{count, n}, {keep, n}, {fused, 4 * n}, {depth, 4 * n}, {valid, n}, {ray, 12 * (size_t)H * W},
                    {K, 36}, {R, 36 * views}, {t, 12 * views}};
  if (spans_overlap(s, 3, 9)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_consistency_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, count, keep, fused, B, V, H, W,
                               (hipStream_t)stream);
}

size_t ctd_depth_fuse_workspace_bytes(int B, int V, int H, int W) {
  if (B <= 0 || V > 64 || !depth_fusion_sizes_ok(B, V, H, W) || !depth_fusion_supported(B, V, H, W)) return 0;
  return depth_fuse_workspace_bytes(B, V, H, W);
}

int ctd_depth_fuse_points_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                              const float* t, float max_px, float max_rel, int min_views, int dedupe, float* points,
                              int64_t* src, int64_t* n_per_track, uint8_t* count, uint8_t* keep, float* fused, int B,
                              int V, int H, int W, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!depth_fusion_sizes_ok(B, V, H, W) || !depth_fusion_params_ok(max_px, max_rel, min_views)) return CTD_ERR_INVALID_ARG;
  if (!depth || !ray || !K || !R || !t || !points || !src || !n_per_track) return CTD_ERR_INVALID_ARG;
  if (V > 64 || !depth_fusion_supported(B, V, H, W)) return CTD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * V * H * W, views = (size_t)B * V;
  const size_t need = ctd_depth_fuse_workspace_bytes(B, V, H, W);
  const Span s[] = {{points, 12 * n}, {src, 8 * n}, {n_per_track, 8 * (size_t)B}, {count, n}, {keep, n}, {fused, 4 * n},
                    {workspace, need}, {depth, 4 * n}, {valid, n}, {ray, 12 * (size_t)H * W}, {K, 36}, {R, 36 * views},
                    {t, 12 * views}};
  if (spans_overlap(s, 7, 13)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!workspace || workspace_bytes < need || ((uintptr_t)workspace & 255)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_fuse_points_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, dedupe, points, src, n_per_track,
                               count, keep, fused, B, V, H, W, workspace, (hipStream_t)stream);
}

int ctd_disp_to_depth_fwd_f32(const float* disp, float* depth, long n, float baseline_focal, int device, void* stream) {
  if (n < 0) return CTD_ERR_INVALID_ARG;
  if (n == 0) return CTD_OK;
  if (!disp || !depth) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disp_to_depth_fwd_f32(disp, depth, n, baseline_focal, (hipStream_t)stream);
}

int ctd_idx_to_depth_f32(const int64_t* idx, float* depth, long n, float baseline_focal, float disp_offset, int device,
                         void* stream) {
  if (n < 0) return CTD_ERR_INVALID_ARG;
  if (n == 0) return CTD_OK;
  if (!idx || !depth) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return idx_to_depth_f32(idx, depth, n, baseline_focal, disp_offset, (hipStream_t)stream);
}

int ctd_disp_to_depth_bwd_f32(const float* disp, const float* grad_depth, float* grad_disp, long n,
                              float baseline_focal, int device, void* stream) {
  if (n < 0) return CTD_ERR_INVALID_ARG;
  if (n == 0) return CTD_OK;
  if (!disp || !grad_depth || !grad_disp) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disp_to_depth_bwd_f32(disp, grad_depth, grad_disp, n, baseline_focal, (hipStream_t)stream);
}

static bool img_shape_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && B <= 65535 && (double)B * H * W < 2147483648.0;
}

size_t ctd_disparity_loss_workspace_bytes(int B, int H, int W) {
  return img_shape_ok(B, H, W) ? disparity_loss_workspace_bytes(B, H, W) : 0;
}

int ctd_disparity_loss_fwd_f32(const float* disp, const float* edge, float* loss, int B, int H, int W, void* workspace,
                               size_t workspace_bytes, int device, void* stream) {
  if (!img_shape_ok(B, H, W) || !disp || !loss) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disparity_loss_fwd_f32(disp, edge, loss, B, H, W, workspace, workspace_bytes, (hipStream_t)stream);
}

int ctd_disparity_loss_bwd_f32(const float* disp, const float* edge, const float* grad_loss, float* grad_disp,
                               float* grad_edge, int B, int H, int W, void* workspace, size_t workspace_bytes,
                               int device, void* stream) {
  if (!img_shape_ok(B, H, W) || !disp || !grad_loss || !grad_disp) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disparity_loss_bwd_f32(disp, edge, grad_loss, grad_disp, grad_edge, B, H, W, workspace, workspace_bytes,
                                (hipStream_t)stream);
}

size_t ctd_geometric_workspace_bytes(int B, int H, int W) {
  return img_shape_ok(B, H, W) ? geometric_workspace_bytes(B, H, W) : 0;
}

int ctd_geometric_fwd_f32(const float* depth0, const float* depth1, const float* ray, const float* K, const float* R0,
                          const float* t0, const float* R1, const float* t1, float* loss, int accumulate, int B, int H,
                          int W, float clamp, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || !depth0 || !depth1 || !ray || !K || !R0 || !t0 || !R1 || !t1 || !loss)
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return geometric_fwd_f32(depth0, depth1, ray, K, R0, t0, R1, t1, loss, accumulate, B, H, W, clamp, workspace,
                           workspace_bytes, (hipStream_t)stream);
}

int ctd_geometric_sym_fwd_f32(const float* depth0, const float* depth1, const float* ray, const float* K, const float* R0,
                              const float* t0, const float* R1, const float* t1, float* loss, int B, int H, int W,
                              float clamp, void* workspace, size_t workspace_bytes, unsigned* ticket, int device,
                              void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || !depth0 || !depth1 || !ray || !K || !R0 || !t0 || !R1 || !t1 || !loss ||
      !ticket)
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return geometric_sym_fwd_f32(depth0, depth1, ray, K, R0, t0, R1, t1, loss, B, H, W, clamp, workspace, workspace_bytes,
                               ticket, (hipStream_t)stream);
}

int ctd_geometric_bwd_f32(const float* depth0, const float* depth1, const float* ray, const float* K, const float* R0,
                          const float* t0, const float* R1, const float* t1, const float* grad_loss,
                          float* grad_depth0, int accumulate0, float* grad_depth1, int B, int H, int W, float clamp,
                          int device, void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || !depth0 || !depth1 || !ray || !K || !R0 || !t0 || !R1 || !t1 ||
      !grad_loss || !grad_depth0 || !grad_depth1)
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return geometric_bwd_f32(depth0, depth1, ray, K, R0, t0, R1, t1, grad_loss, grad_depth0, accumulate0, grad_depth1, B,
                           H, W, clamp, (hipStream_t)stream);
}

int ctd_nn_f32(const float* in0, const float* in1, long n0, long n1, int64_t* out, int device, void* stream) {
  if (n0 < 0 || n1 < 0) return CTD_ERR_INVALID_ARG;
  if (n0 == 0) return CTD_OK;
  if (!in0 || !out || (n1 > 0 && !in1)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return nn_f32(in0, in1, n0, n1, out, (hipStream_t)stream);
}

int ctd_nn_f64(const double* in0, const double* in1, long n0, long n1, int64_t* out, int device, void* stream) {
  if (n0 < 0 || n1 < 0) return CTD_ERR_INVALID_ARG;
  if (n0 == 0) return CTD_OK;
  if (!in0 || !out || (n1 > 0 && !in1)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return nn_f64(in0, in1, n0, n1, out, (hipStream_t)stream);
}

int ctd_crosscheck(const int64_t* in0, const int64_t* in1, long n0, long n1, uint8_t* out, int device, void* stream) {
  if (n0 < 0 || n1 < 0) return CTD_ERR_INVALID_ARG;
  if (n0 == 0) return CTD_OK;
  if (!in0 || !out || (n1 > 0 && !in1)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return crosscheck_i64(in0, in1, n0, n1, out, (hipStream_t)stream);
}

int ctd_proj_nn_f32(const float* xyz0, const float* xyz1, const float* K, int B, int H, int W, int patch_size,
                    int64_t* out, int device, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || patch_size < 0) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!xyz0 || !xyz1 || !K || !out) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return proj_nn_f32(xyz0, xyz1, K, B, H, W, patch_size, out, (hipStream_t)stream);
}

int ctd_proj_nn_f64(const double* xyz0, const double* xyz1, const double* K, int B, int H, int W, int patch_size,
                    int64_t* out, int device, void* stream) {
  if (B < 0 || H <= 0 || W <= 0 || patch_size < 0) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!xyz0 || !xyz1 || !K || !out) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return proj_nn_f64(xyz0, xyz1, K, B, H, W, patch_size, out, (hipStream_t)stream);
}

int ctd_render_mesh_proj_f32(const float* verts, const float* colors, int n_verts, const int* faces, int n_faces,
                             const float* cam, int cam_width, int cam_height, const float* proj, int proj_width,
                             int proj_height, const float* shader, const float* pattern, float d_alpha, float d_beta,
                             float* depth, float* color, float* normal, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || cam_width <= 0 || cam_height <= 0 || proj_width <= 0 || proj_height <= 0 ||
      (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!cam || !proj || !shader || !pattern || !color || (n_faces > 0 && (!verts || !colors || !faces)))
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_proj_f32(verts, colors, faces, n_faces, cam, cam_width, cam_height, proj, proj_width, proj_height,
                              shader, pattern, d_alpha, d_beta, depth, color, normal, (hipStream_t)stream);
}

int ctd_render_mesh_f32(const float* verts, const float* colors, const float* normals, int n_verts, const int* faces,
                        int n_faces, const float* cam, int cam_width, int cam_height, const float* shader, float* depth,
                        float* color, float* normal, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || cam_width <= 0 || cam_height <= 0 || (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!cam || !shader || (n_faces > 0 && (!verts || !faces))) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && ((color && !colors) || ((color || normal) && !normals))) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_f32(verts, colors, normals, faces, n_faces, cam, cam_width, cam_height, shader, depth, color, normal,
                         (hipStream_t)stream);
}

size_t ctd_mesh_bvh_bytes(int n_faces) {
  return n_faces < 0 || n_faces > kBvhMaxFaces ? 0 : mesh_bvh_bytes(n_faces);
}

size_t ctd_mesh_bvh_workspace_bytes(int n_faces) {
  return n_faces < 0 || n_faces > kBvhMaxFaces ? 0 : mesh_bvh_workspace_bytes(n_faces);
}

int ctd_mesh_bvh_build_f32(const float* verts, int n_verts, const int* faces, int n_faces, void* bvh, size_t bvh_bytes,
                           void* workspace, size_t workspace_bytes, int* depth, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > kBvhMaxFaces || !bvh) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && (!verts || !faces || !workspace || n_verts == 0)) return CTD_ERR_INVALID_ARG;
  if ((uintptr_t)bvh % 16 || (uintptr_t)workspace % 16) return CTD_ERR_INVALID_ARG;
  if (bvh_bytes < mesh_bvh_bytes(n_faces)) return CTD_ERR_INVALID_ARG;
  if (workspace_bytes < mesh_bvh_workspace_bytes(n_faces)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_bvh_build_f32(verts, faces, n_faces, bvh, workspace, depth, (hipStream_t)stream);
}

int ctd_render_mesh_proj_bvh_f32(const void* bvh, const float* verts, const float* colors, int n_verts, const int* faces,
                                 int n_faces, const float* cam, int cam_width, int cam_height, const float* proj,
                                 int proj_width, int proj_height, const float* shader, const float* pattern,
                                 float d_alpha, float d_beta, float* depth, float* color, float* normal, int device,
                                 void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > kBvhMaxFaces || cam_width <= 0 || cam_height <= 0 || proj_width <= 0 ||
      proj_height <= 0 || (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!bvh || (uintptr_t)bvh % 16 || !cam || !proj || !shader || !pattern || !color ||
      (n_faces > 0 && (!verts || !colors || !faces)))
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_proj_bvh_f32(bvh, verts, colors, faces, n_faces, cam, cam_width, cam_height, proj, proj_width,
                                  proj_height, shader, pattern, d_alpha, d_beta, depth, color, normal, (hipStream_t)stream);
}

int ctd_render_mesh_bvh_f32(const void* bvh, const float* verts, const float* colors, const float* normals, int n_verts,
                            const int* faces, int n_faces, const float* cam, int cam_width, int cam_height,
                            const float* shader, float* depth, float* color, float* normal, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > kBvhMaxFaces || cam_width <= 0 || cam_height <= 0 ||
      (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!bvh || (uintptr_t)bvh % 16 || !cam || !shader || (n_faces > 0 && (!verts || !faces))) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && ((color && !colors) || ((color || normal) && !normals))) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_bvh_f32(bvh, verts, colors, normals, faces, n_faces, cam, cam_width, cam_height, shader, depth,
                             color, normal, (hipStream_t)stream);
}

static bool syn_shape_ok(int N, int H, int W) {
  return N >= 0 && N <= 65535 && H > 0 && W > 0 && (double)H * W * 3 < 2147483648.0;
}

int ctd_syn_finish_f32(const float* depth, const float* color, const float* normal, const double* blend,
                       double baseline_focal, float grad_threshold, int lcn_radius, float lcn_eps, int lcn_clip,
                       float* im, float* ambient, float* grad, float* disp, float* mask, int N, int H, int W, int device,
                       void* stream) {
  if (!syn_shape_ok(N, H, W) || lcn_radius < 0) return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!depth || !color || !normal || !blend || !im || !ambient || !grad) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return syn_finish_f32(depth, color, normal, blend, baseline_focal, grad_threshold, lcn_radius, lcn_eps, lcn_clip, im,
                        ambient, grad, disp, mask, N, H, W, (hipStream_t)stream);
}

int ctd_augment_f32(const float* img, const void* noise, int noise_f64, const ctd_augment_params* params, float* out,
                    uint32_t* minmax, int N, int H, int W, int device, void* stream) {
  if (!syn_shape_ok(N, H, W) || (noise_f64 != 0 && noise_f64 != 1)) return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!img || !params || !out || !minmax) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return augment_f32(img, noise, noise_f64, params, out, minmax, N, H, W, (hipStream_t)stream);
}

int ctd_salt_pepper_f32(float* img, const uint32_t* minmax, const int32_t* counts, const int64_t* salt,
                        const int64_t* pepper, int kmax, int N, int H, int W, int device, void* stream) {
  if (!syn_shape_ok(N, H, W) || kmax < 0) return CTD_ERR_INVALID_ARG;
  if (N == 0 || kmax == 0) return CTD_OK;
  if (!img || !minmax || !counts || !salt || !pepper) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return salt_pepper_f32(img, minmax, counts, salt, pepper, kmax, N, H, W, (hipStream_t)stream);
}

int ctd_hyperdepth_eval_f32(const ctd_hd_tables* tables, const uint8_t* ims, int N, int H, int W, int row_from,
                            int row_to, int n_disp_bins, float* out, int device, void* stream) {
  if (!tables) return CTD_ERR_INVALID_ARG;
  const ctd_hd_tables t = *tables;
  if (N < 0 || H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24)) return CTD_ERR_INVALID_ARG;
  if (row_from < 0 || row_from > row_to || row_to > H) return CTD_ERR_INVALID_ARG;
  if (t.n_trees < 1 || t.n_trees > 16 || t.n_classes < 2 || n_disp_bins < 1 || t.n_nodes < 0 || t.n_leaves < 0 ||
      t.n_entries < 0 || t.max_depth < 0 || t.n_rows < 0)
    return CTD_ERR_INVALID_ARG;
  if (row_from < row_to && (row_from < t.row0 || (long)row_to > (long)t.row0 + t.n_rows)) return CTD_ERR_INVALID_ARG;
  if (!ims || !out || !t.roots || !t.leaf_off || !t.leaf_sum || (t.n_nodes > 0 && !t.nodes) ||
      (t.n_entries > 0 && !t.entries))
    return CTD_ERR_INVALID_ARG;
  // the kernel reads nodes as int4 pairs, entries as int2, offsets as int64
  if ((uintptr_t)t.nodes % 16 || (uintptr_t)t.entries % 8 || (uintptr_t)t.leaf_off % 8 || (uintptr_t)t.roots % 4 ||
      (uintptr_t)t.leaf_sum % 4 || (uintptr_t)out % 4)
    return CTD_ERR_INVALID_ARG;
  if (hyperdepth_lds_bytes(t.n_trees, t.n_classes) > 65536) return CTD_ERR_UNSUPPORTED;
  if (hyperdepth_grid(N, H, W) > 2147483647L) return CTD_ERR_UNSUPPORTED;
  if (N == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return hyperdepth_eval_f32(t, ims, N, H, W, row_from, row_to, n_disp_bins, out, (hipStream_t)stream);
}

static bool hd_train_shape_ok(int N, int H, int W, int row_from, int row_to, int nb) {
  if (N < 1 || H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24)) return false;
  if ((long long)N * H * W >= (1ll << 31)) return false;
  if (row_from < 0 || row_from >= row_to || row_to > H) return false;
  return nb >= 1 && (long long)W * nb < (1ll << 31);
}

static bool hd_train_params_ok(const ctd_hd_train_params* p) {
  return p && p->n_trees >= 1 && p->n_trees <= 16 && p->max_tree_depth >= 0 && p->max_tree_depth <= 24 &&
         p->n_test_split_functions >= 0 && p->n_test_split_functions < (1 << 20) && p->n_test_thresholds >= 0 &&
         p->n_test_thresholds < (1 << 16) && p->n_test_samples >= 1 && p->n_test_samples <= 8192 &&
         p->min_samples_to_split >= 0 && p->min_samples_for_leaf >= 1 && p->n_disp_bins >= 1;
}

int ctd_hyperdepth_train_count_f32(const float* disps, int N, int H, int W, int row_from, int row_to,
                                   int n_disp_bins, int64_t* counts, int device, void* stream) {
  if (!disps || !counts || !hd_train_shape_ok(N, H, W, row_from, row_to, n_disp_bins)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return hyperdepth_train_count_f32(disps, N, H, W, row_from, row_to, n_disp_bins, counts, (hipStream_t)stream);
}

size_t ctd_hyperdepth_train_workspace_bytes(const ctd_hd_train_params* params, int n_rows, const int64_t* row_counts,
                                            int64_t cap_leaves) {
  if (!hd_train_params_ok(params) || n_rows < 1 || !row_counts || cap_leaves < 0) return 0;
  for (int r = 0; r < n_rows; ++r)
    if (row_counts[r] < 0) return 0;
  return hyperdepth_train_workspace_bytes(*params, n_rows, row_counts, cap_leaves);
}

int ctd_hyperdepth_train_f32(const ctd_hd_train_params* params, const int64_t* X, int n_x, const uint8_t* ims,
                             const float* disps, int N, int H, int W, int row_from, int row_to,
                             const int64_t* row_counts, void* workspace, size_t workspace_bytes,
                             const ctd_hd_train_out* out, int device, void* stream) {
  if (!hd_train_params_ok(params) || !X || !ims || !disps || !row_counts || !workspace || !out) return CTD_ERR_INVALID_ARG;
  if (!hd_train_shape_ok(N, H, W, row_from, row_to, params->n_disp_bins)) return CTD_ERR_INVALID_ARG;
  if (n_x < params->n_test_samples + 1) return CTD_ERR_INVALID_ARG;
  const ctd_hd_train_out o = *out;
  if (!o.roots || !o.leaf_off || !o.leaf_sum || !o.used || o.cap_nodes < 0 || o.cap_leaves < 0 || o.cap_entries < 0 ||
      (o.cap_nodes > 0 && !o.nodes) || (o.cap_entries > 0 && !o.entries))
    return CTD_ERR_INVALID_ARG;
  if ((uintptr_t)o.entries % 8 || (uintptr_t)o.leaf_off % 8 || (uintptr_t)o.used % 8 || (uintptr_t)X % 8 ||
      (uintptr_t)workspace % 256)
    return CTD_ERR_INVALID_ARG;
  for (int r = 0; r < row_to - row_from; ++r)
    if (row_counts[r] < 0) return CTD_ERR_INVALID_ARG;
  if (workspace_bytes < hyperdepth_train_workspace_bytes(*params, row_to - row_from, row_counts, o.cap_leaves))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return hyperdepth_train_f32(*params, X, ims, disps, N, H, W, row_from, row_to, row_counts, workspace,
                              workspace_bytes, o, (hipStream_t)stream);
}

}  // extern "C"
