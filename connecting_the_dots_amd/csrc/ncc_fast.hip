// ncc_fast.hip -- host side of the NCC family: workspace layout, ranking buffers and launch sequences of the fast path
// (CTD_NCC_FAST), and, at the end, the family's C entry points (ctd_xcorrvol_*, ctd_lcn_xcorrvol_*; those of the exact
// kernels alone -- ctd_xcorrvol_f64, ctd_argmax_disp_f32 -- are in ncc_exact.hip).  The kernels live one family per
// file; a fast call runs them in this order:
//   plain call (ncc_fast_f32, no ranking)
//     1. ncc_prepass.hip   centred planes + window statistics of frames and pattern, lists of ill-conditioned windows
//     2. ncc_alld.hip      the volume (block 9, W % 4 == 0, one channel), else ncc_tiles.hip / ncc_t256.hip per channel
//     3. ncc_fixup.hip     listed windows recomputed in the reference's order, fully clamped runs spread
//   ranked call (ctd_xcorrvol_argmax_f32: ncc_fast_f32 with a RankPlan, then ncc_fast_fixup_ranked)
//     1. ncc_prepass.hip   as above (also clears the work-list counters)
//     2. ncc_alld.hip      volume (optional) + in-kernel ranking: index, best score, work-list flags -- ncc_fast_f32 ends here
//     3. ncc_fixup.hip     listed windows against each pixel's best (ncc_fast_fixup_ranked)
//     4. argmax_rerank.hip tail kernel: runs, decode, exact re-scoring of the work list (rank_tail_f32, the caller's)
//   fused call (ctd_lcn_xcorrvol_argmax_f32): a ranked call whose stage 1 is lcn_stream.hip for the frames (LCN and
//     their planes in one launch) and ncc_prepass.hip for the pattern alone, unless the pattern was prepared
//   prepared pattern (ncc_fast_prepare_pattern_f32): the pattern half of stage 1, once; later calls skip it.  Block 9,
//     single channel: a small launch behind it (ncc_fixup_table_kernel) fills the table at FastWorkspace::fix_tab_end (the unused end of flag_b), the pattern side of
//     the fix-up items (centred taps and their sum of squares per listed pattern window, in flag_b order, the first
//     kFixTabCap of them or as many as fit there).  The table is the pattern's, like counters[1..2], flag_b and run_rows: no per-call kernel
//     writes it.  Calls on the prepared pattern hand it to the fix-up, which then runs one item per (listed pattern
//     window, frame, block of 64 disparities) -- ncc_fixup_items_kernel; unprepared calls pass null and launch the
//     table-less kernel.
// Shared declarations: ctd_ncc_fast.h.  Same op as ncc_exact.hip, to |a-b| <= 1e-5*|b| + 1e-6 (ncc_tiles.hip, ncc_fixup.hip).
#include "ctd_ncc_fast.h"
#include "ctd_prepass.h"
#include "ctd_validate.h"

namespace ctd {

// A fused call: the frames arrive raw and `in0` of ncc_fast_f32 is the buffer their LCN goes to (lcn_stream.hip).
struct FusedLcn {
  const float* raw;           // [frames][H][W] raw frames
  float* stds;                // [frames][H][W] LCN deviation output (the LCN output itself is `in0`)
  int radius;
  float eps;
  bool exact;                 // f64 box sums + the reference's f32 tail (the oracle's bits) | f32 sums, v_rcp / v_sqrt tail
};

static FastWorkspace fast_workspace(void* base, int frames, int C, int H, int W, int D, bool per_frame_pattern) {
  FastWorkspace ws;
  const PlaneGeometry g = plane_geometry(W, D);
  ws.Wp = g.Wp;
  ws.W1 = g.W1;
  ws.xoff = g.xoff;
  size_t off = 0;                                                  // every buffer starts 256-byte aligned
  auto take = [&](size_t bytes) {
    char* p = (char*)base + off;
    off += align_up(bytes, 256);
    return p;
  };
  const size_t img0 = (size_t)frames * C * H, img1 = (size_t)(per_frame_pattern ? frames : 1) * C * H;   // image rows
  const size_t n0 = img0 * ws.Wp * sizeof(float), n1 = img1 * ws.W1 * sizeof(float);
  ws.ac = (float*)take(n0);
  ws.m0 = (float*)take(n0);
  ws.v0 = (float*)take(n0);
  ws.bc = (float*)take(n1);
  ws.m1 = (float*)take(n1);
  ws.v1 = (float*)take(n1);
  ws.counters = (unsigned*)take(256);
  // flag lists: room for every frame window and every pattern window the outputs can touch
  ws.flag_a = (unsigned long long*)take(img0 * W * sizeof(unsigned long long));
  ws.flag_b = (unsigned long long*)take(img1 * ws.W1 * sizeof(unsigned long long));
  ws.flag_b_cap = (unsigned)(img1 * ws.W1);
  ws.fix_tab_end = (float*)(ws.flag_b + ws.flag_b_cap);        // the fix-up's table grows down from the list's end (ctd_ncc_fast.h)
  ws.run_rows = (unsigned long long*)take(img1 * sizeof(unsigned long long));
  ws.run_vals = (float*)take((size_t)frames * H * D * sizeof(float));
  ws.bytes = off;
  return ws;
}

static size_t ncc_fast_workspace_bytes(int frames, int C, int H, int W, int D, int bs, bool per_frame_pattern) {
  (void)bs;
  return fast_workspace(nullptr, frames, C, H, W, D, per_frame_pattern).bytes;
}

static bool ncc_fast_rank_supported(int C, int H, int W, int D, int bs) {
  (void)H;
  return C == 1 && bs == 9 && W % 4 == 0 && D <= 512;      // the all-D kernel, single channel
}

// ranking buffers behind the volume pass's workspace
static RankPlan rank_plan(void* base, size_t offset, int frames, int H, int W, int D) {
  RankPlan rp;
  rp.eps = 0.f;
  rp.idx = nullptr;
  rp.best = nullptr;
  (void)D;
  const size_t nflag = align_up((size_t)frames * H * W, 256);
  // work list: kWorkListParts segments keyed by image row, behind their counters (one cache line each)
  const long seg_cap = (long)ceil_div(frames * H, kWorkListParts) * W;
  const size_t ncnt = align_up(sizeof(unsigned) * kWorkListStride * kWorkListParts, 256);
  const size_t nlist = ncnt + align_up((size_t)kWorkListParts * seg_cap * sizeof(int64_t), 256);
  char* p = (char*)base + offset;
  rp.flags = (unsigned char*)p;
  rp.work.counters = (unsigned*)(p + nflag);
  rp.work.list = (int64_t*)(p + nflag + ncnt);
  rp.work.parts = kWorkListParts;
  rp.work.row_width = W;
  rp.work.seg_cap = seg_cap;
  rp.best_scratch = (float*)(p + nflag + nlist);
  rp.bytes = offset + nflag + nlist + align_up((size_t)frames * H * W * sizeof(float), 256);
  return rp;
}

static void ncc_fast_rank_offsets(int frames, int H, int W, int D, bool per_frame_pattern, size_t* off) {
  const FastWorkspace ws = fast_workspace(nullptr, frames, 1, H, W, D, per_frame_pattern);
  const RankPlan rp = rank_plan(nullptr, ws.bytes, frames, H, W, D);
  const AlldPlan ap = alld_plan(frames, H, W, D);
  off[0] = (size_t)ap.band_rows; off[1] = (size_t)rp.flags; off[2] = (size_t)rp.work.counters; off[3] = (size_t)rp.work.list;
  off[4] = (size_t)ap.n_pass;
}

static size_t ncc_fast_rank_workspace_bytes(int frames, int H, int W, int D, bool per_frame_pattern) {
  const size_t off = fast_workspace(nullptr, frames, 1, H, W, D, per_frame_pattern).bytes;
  return rank_plan(nullptr, off, frames, H, W, D).bytes;
}

// what the packed list entries (20-bit row, 19-bit column, 24-bit image) and the kernels' key tags (D <= 512) can hold
static bool fast_shape_supported(int frames, int C, int H, int W, int D, int bs) {
  if (bs < 2 || bs > 33) return false;
  return !(H >= (1 << 20) || W + D >= (1 << 19) || D > 512 || (long)frames * C >= (1 << 24));
}

// The two halves of a pre-pass launch: window statistics of the frames (per pixel; `in0`, n_frame_img images) and of the
// pattern (per unclamped window-centre column x = w - d; windows x <= -(bs-1-bs/2) are all the same fully clamped window
// and are listed once; `in1`, n_pat_img images).  A half with 0 images is skipped by the kernel.
struct PrepassJobs {
  PrepassJob frames, pattern;
};
static PrepassJobs prepass_jobs(const FastWorkspace& ws, const float* in0, const float* in1, int C, int H, int W, int bs,
                                int n_frame_img, int n_pat_img) {
  PrepassJobs j;
  j.frames = {in0, (long)H * W, ws.ac, ws.m0, ws.v0, 0, W, n_frame_img, ws.counters, ws.flag_a, 0, W,
              nullptr, nullptr, -(double)(bs * bs), kFlagRatio / C, ws.Wp, 4, 4};
  j.pattern = {in1, (long)H * W, ws.bc, ws.m1, ws.v1, -ws.xoff, ws.W1, n_pat_img, ws.counters + 1, ws.flag_b,
               -(bs - 1 - bs / 2), W, ws.counters + 2, ws.run_rows, 1.0, kFlagRatio / C, ws.W1, 0, 0};
  return j;
}

// Pattern half of the pre-pass alone (ctd_xcorrvol_pattern_prepare_f32): the pattern's planes, its list of listed windows
// and run rows stay in `workspace`; calls with `pattern_prepared` on the SAME workspace and shape then skip that half (the
// reference prepares the pattern once per run, model/exp_synph.py:64-71).  The layout depends on `frames`.
static int ncc_fast_prepare_pattern_f32(const float* in1, long in1_frame_stride, int frames, int C, int H, int W, int D,
                                        int bs, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  if (!fast_shape_supported(frames, C, H, W, D, bs)) return CTD_ERR_UNSUPPORTED;
  const bool per_frame = in1_frame_stride != 0;
  if (per_frame && in1_frame_stride != (long)C * H * W) return CTD_ERR_INVALID_ARG;
  FastWorkspace ws = fast_workspace(workspace, frames, C, H, W, D, per_frame);
  if (workspace == nullptr || workspace_bytes < ws.bytes) return CTD_ERR_WORKSPACE;
  CTD_HIP_TRY(hipMemsetAsync(ws.counters, 0, 16, stream));
  const PrepassJobs j = prepass_jobs(ws, in1, in1, C, H, W, bs, 0, (per_frame ? frames : 1) * C);   // (no frame images in this launch)
  const int st = launch_prepass(j.frames, j.pattern, H, W, bs, nullptr, stream);
  if (st) return st;
  return launch_fixup_table(in1, in1_frame_stride, C, H, W, bs, ws, stream);   // the fix-up's pattern side, once (ncc_fixup.hip)
}

// The volume stage.  Block 9, W % 4 == 0, one channel, aligned volume: the all-D kernel, with the ranking (`rank`) or
// without it (the same bits); every other shape: by disparity groups, unranked only.
static int launch_volume(float* out, int frames, int C, int H, int W, int D, int bs, const FastWorkspace& ws, bool per_frame,
                         const RankPlan* rank, hipStream_t stream) {
  const long st1_stride = per_frame ? (long)C * H * ws.W1 : 0;
  const bool alld = bs == 9 && W % 4 == 0 && C == 1 && ((uintptr_t)out) % 16 == 0;
  if (rank && !alld) return CTD_ERR_UNSUPPORTED;
  if (!alld) return launch_tiles(out, frames, C, H, W, D, bs, ws, st1_stride, stream);
  const AlldOperands op = {ws.ac, ws.m0, ws.v0, ws.bc, ws.m1, ws.v1, st1_stride, ws.Wp, ws.W1, ws.xoff};
  const int mode = rank ? (out ? kAStore | kARank : kARank) : kAStore;
  return launch_alld(mode, op, out, rank, frames, H, W, D, true, stream);
}

// `rank` non-null (in: eps, idx, best -- best may be null): the all-D kernel computes the volume (`out` may be null:
// nothing is materialised then), ranks every pixel's scores in LDS and writes idx / best / work-list flags itself;
// *rank comes back filled with the buffers the later passes need and the call STOPS after that kernel -- the caller
// runs ncc_fast_fixup_ranked (which needs the best scores and indices), then rank_tail_f32.
static int ncc_fast_f32(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames, int C, int H,
                        int W, int D, int bs, void* workspace, size_t workspace_bytes, RankPlan* rank,
                        bool pattern_prepared, hipStream_t stream, const FusedLcn* fused = nullptr) {
  if (!fast_shape_supported(frames, C, H, W, D, bs)) return CTD_ERR_UNSUPPORTED;
  if (fused && (C != 1 || !lcn_stream_supported(H, W, fused->radius, bs))) return CTD_ERR_UNSUPPORTED;
  if (!out && !rank) return CTD_ERR_INVALID_ARG;
  if (rank && !ncc_fast_rank_supported(C, H, W, D, bs)) return CTD_ERR_UNSUPPORTED;
  const bool per_frame = in1_frame_stride != 0;
  FastWorkspace ws = fast_workspace(workspace, frames, C, H, W, D, per_frame);
  size_t need = ws.bytes;
  if (rank) {
    const RankPlan in = *rank;
    *rank = rank_plan(workspace, ws.bytes, frames, H, W, D);
    rank->eps = in.eps;
    rank->idx = in.idx;
    rank->best = in.best ? in.best : rank->best_scratch;
    rank->run_vals = ws.run_vals;
    rank->run_rows = ws.run_rows;
    rank->counters = ws.counters;
    rank->flag_a = ws.flag_a;
    rank->flag_b = ws.flag_b;
    rank->v1 = ws.v1;
    rank->W1 = ws.W1;
    rank->xoff = ws.xoff;
    need = rank->bytes;
  }
  if (workspace == nullptr || workspace_bytes < need) return CTD_ERR_WORKSPACE;
  if (rank && !rank->idx) return CTD_ERR_INVALID_ARG;
  // counters: [0] listed frame windows, [1] listed pattern windows, [2] listed run rows -- the last two belong to the
  // pattern and survive when it was prepared
  // (a ranked call on a prepared pattern finds [0] at zero: the prepare call and every ranked call's tail kernel leave it so)
  if (!(rank && pattern_prepared)) CTD_HIP_TRY(hipMemsetAsync(ws.counters, 0, pattern_prepared ? 4 : 16, stream));
  if (per_frame && in1_frame_stride != (long)C * H * W) return CTD_ERR_INVALID_ARG;
  const PrepassJobs j = prepass_jobs(ws, in0, in1, C, H, W, bs, frames * C, pattern_prepared ? 0 : (per_frame ? frames : 1) * C);
  int st;
  if (fused) {
    // fused call: `in0` is the LCN OUTPUT buffer -- the streaming kernel (lcn_stream.hip) writes it and the frames'
    // planes from the raw frames in one launch; the pattern's half (if not prepared) keeps the tiled kernel
    const StatPlanes sp = {ws.ac, ws.m0, ws.v0, ws.Wp, 4, ws.counters, ws.flag_a, -(float)(bs * bs), (float)kFlagRatio};
    st = lcn_stream_f32(fused->raw, const_cast<float*>(in0), fused->stds, frames, H, W, fused->eps, sp,
                        rank ? rank->work.counters : nullptr, rank ? rank->work.parts : 0, fused->exact, stream);
    if (st) return st;
    if (!pattern_prepared) {
      PrepassJob none = j.frames;
      none.nimg = 0;
      st = launch_prepass(none, j.pattern, H, W, bs, nullptr, stream);
    }
  } else {
    st = launch_prepass(j.frames, j.pattern, H, W, bs, rank ? &rank->work : nullptr, stream);
  }
  if (st) return st;
  st = launch_volume(out, frames, C, H, W, D, bs, ws, per_frame, rank, stream);
  if (st || rank) return st;
  st = launch_fixup(in0, in1, in1_frame_stride, out, frames, C, H, W, D, bs, ws, per_frame,
                    pattern_prepared ? ws.fix_tab_end : nullptr, nullptr, nullptr, (unsigned*)workspace, stream);
  if (st == CTD_OK && pattern_prepared) CTD_HIP_TRY(hipMemsetAsync(ws.counters, 0, 4, stream));   // (see above: [0] stays zero between calls)
  return st;
}

// Second half of a ranked call, after the all-D kernel: fix-up of the listed windows (volume patch when there is one,
// run values) with every recomputed score held against the `best` / `idx` of its pixel.
static int ncc_fast_fixup_ranked(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames,
                                 int H, int W, int D, int bs, void* workspace, const RankPlan& rank, const float* best,
                                 bool pattern_prepared, hipStream_t stream) {
  const bool per_frame = in1_frame_stride != 0;
  FastWorkspace ws = fast_workspace(workspace, frames, 1, H, W, D, per_frame);
  return launch_fixup(in0, in1, in1_frame_stride, out, frames, 1, H, W, D, bs, ws, per_frame,
                      pattern_prepared ? ws.fix_tab_end : nullptr, &rank, best, nullptr, stream);
}

}  // namespace ctd

using namespace ctd;

extern "C" {

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
      st = ncc_fast_fixup_ranked(in0, in1, in1_frame_stride, vol_out, frames, H, W, D, block_size, workspace, rp, rp.best, prepared, hs);
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
  st = ncc_fast_fixup_ranked(lcn_out, in1, in1_frame_stride, vol_out, frames, H, W, D, block_size, workspace, rp, rp.best, prepared, hs);
  if (st) return st;
  return rank_tail_f32(rp, vol_out, lcn_out, in1, in1_frame_stride, idx, rp.best, frames, D, H, W, block_size, hs);
}

}  // extern "C"
