// ctd_ncc_fast.h -- what the translation units of the fast NCC family share (ncc_fast.hip: the map of the family):
// the padded-plane geometry and workspace, the pre-pass job, the all-D plan and the stage launchers.
#pragma once
#include "ctd_internal.h"

namespace ctd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kFND = 4;        // disparities per lane (narrow kernel, ncc_tiles.hip)
constexpr int kFWaves = 4;     // consumer wavefronts per workgroup (adjacent disparity groups)
constexpr int kFDG = kFND * kFWaves;   // disparities per workgroup; the pattern planes are padded to a multiple of it

constexpr int gcd_ce(int a, int b) { return b == 0 ? a : gcd_ce(b, a % b); }
constexpr int lcm_ce(int a, int b) { return a / gcd_ce(a, b) * b; }

// Padded operand planes of the volume kernels.  Frames: row pitch Wp, column c at c + 4 (replicate border baked in).
// Pattern: one column per UNCLAMPED window centre x = w - d, row pitch W1, column x at x + xoff.
struct PlaneGeometry {
  int Wp, W1, xoff;
};
inline PlaneGeometry plane_geometry(int W, int D) {
  PlaneGeometry g;
  // + 32: the last disparity group (tile-256 kernel) / pass (all-D kernel) stages pattern columns for up to 29
  // disparities past D; their outputs are never stored, their operands still come from inside the plane
  const int Dpad = (D + kFDG - 1) / kFDG * kFDG + 32;
  // x = w - d ranges over [-(Dpad-1) - 4, W + 3] (4 halo columns either side).  xoff = 3 (mod 4) makes
  // the first span slot of every workgroup 16-byte aligned (w_lo and the disparity-group base are
  // multiples of 4), which the dwordx4 LDS-DMA of the wide kernel relies on.
  g.xoff = Dpad + 3;
  g.W1 = (int)align_up((size_t)(W + 4 + g.xoff), 4);
  g.Wp = (int)align_up((size_t)(W + 8), 4);
  return g;
}

// Pattern-side table of the fix-up pass (ncc_fixup.hip): per listed pattern window the 81 centred taps and the sum of
// their squares, padded to a multiple of 4 floats; block 9, single channel, the first kFixTabCap listed windows (1.3 MB).
// The table takes no workspace of its own (the sizes the workspace queries answer are part of the ABI): it lives in the
// unused END of the pattern's window list.  That list has room for every window of the pattern planes (H x W1 per image)
// and even an all-constant pattern lists H x (W + 4) of them, so row j sits at the buffer's end minus (j + 1) rows, and
// the rows that fit behind the n_b entries actually listed -- fixup_table_rows, evaluated on the device by the kernel
// that fills the table and by the one that reads it -- are the table; windows past them are staged in the kernel.
constexpr int kFixTabCap = 4096, kFixTabRow = 84;
inline bool fixup_table_covers(int C, int bs) { return C == 1 && bs == 9; }
__host__ __device__ inline unsigned fixup_table_rows(unsigned n_b, unsigned list_cap) {
  const unsigned used = n_b < list_cap ? n_b : list_cap;
  const unsigned long long room = (unsigned long long)(list_cap - used) * sizeof(unsigned long long) / (kFixTabRow * sizeof(float));
  const unsigned want = used < (unsigned)kFixTabCap ? used : (unsigned)kFixTabCap;
  return room < want ? (unsigned)room : want;
}

struct FastWorkspace {
  float *ac, *m0, *v0;        // centred frames, their window mean (centred) / deviation planes   [N*C][H][W]
  float *bc, *m1, *v1;        // same for the pattern, per UNCLAMPED window-centre column          [..][H][W1]
  int Wp;                     // frame plane row pitch: W + 8, column c lives at c + 4 (replicate border baked in)
  int W1, xoff;               // pattern plane row pitch and origin: column x lives at x + xoff
  unsigned* counters;         // [0] flagged frame windows, [1] flagged pattern windows (see ncc_fixup_kernel)
  unsigned long long *flag_a, *flag_b;
  unsigned long long* run_rows;   // (pattern image << 20 | h) of the listed fully clamped pattern windows
  float* run_vals;            // [frames][H][D] exact values of the fully clamped runs (ncc_fixup_runs_kernel)
  unsigned flag_b_cap;        // entries flag_b has room for
  float* fix_tab_end;         // end of flag_b's buffer: row j of the fix-up's pattern-side table (ncc_fixup.hip) is the
                              // kFixTabRow floats at fix_tab_end - (j + 1) * kFixTabRow, in flag_b order; filled when the
                              // pattern is prepared and, like counters[1..2], flag_b and run_rows, the pattern's: no
                              // per-call kernel writes it
  size_t bytes;               // end of the volume pass's own workspace; the ranking buffers (RankPlan) follow
};

// 1 / (sa * sb + 1e-8) from the RECIPROCAL deviations the pre-pass stores: t = ra * rb, ONE multiply.  The reference's
// 1e-8 changes the quotient by the relative amount 1e-8 * t: below 2.1e-6 because the pre-pass lists every window whose
// deviation is under kDevFloor = 7e-2 (t <= 1 / kDevFloor^2 = 204), and listed windows go through the fix-up pass in the
// reference's own arithmetic.  (Until round 3 the first-order term t * (1 - 1e-8 t) was kept and the floor was 6e-3:
// two more instructions on each of the eight scores of a lane and row -- 10 % of the volume kernels' vector work, which
// is what bounds the all-D kernel; LCN'd images have t ~ 0.01, where the term is 1e-10.)
__device__ inline float ncc_inv_norm(float ra, float rb) { return ra * rb; }

// ncc_prepass.hip ------------------------------------------------------------------------
// out_mean = mean_scale * (window mean - cval), out_dev = 1 / sqrt(sum of squared deviations) (0: listed window), out_img = img - cval
// (replicate border baked in), all laid out [image][H][W_out] with column x = xi + x_start;
// cval = f64 window mean at the image centre, recomputed identically by every workgroup.
// One launch serves the frames (job a) and the pattern (job b): blockIdx.z < a.nimg -> image blockIdx.z of job a,
// else image blockIdx.z - a.nimg of job b; workgroups past a job's plane width exit at once.
struct PrepassJob {
  const float* in;
  long frame_stride;
  float *out_img, *out_mean, *out_dev;
  int x_start, W_out, nimg;
  unsigned* n_flag;
  unsigned long long* flag_list;
  int col_lo, col_hi;
  unsigned* n_runs;
  unsigned long long* run_rows;
  double mean_scale;          // out_mean = mean_scale * (window mean - cval): -bs^2 for the frames (the kernels' n*ma*mb
                              // term then needs no multiply of its own), 1 for the pattern
  double flag_ratio;          // list a window when F - 1 > flag_ratio: kFlagRatio / C (the channels' errors add up in the sum)
  int pitch, o_off, halo;     // output row pitch and column offset of xi = 0; halo > 0: the planes carry `halo` replicate
                              // columns either side of the W_out computed ones, and out_img's are filled here (copies of
                              // columns 0 and W_out - 1; the statistics planes' halo columns are never read).  The frames'
                              // planes: computing the halo columns as windows of their own made a ninth column of
                              // workgroups for 8 of 520 columns.
};
// `work` non-null: the launch also clears that work list's counters (ranked calls)
int launch_prepass(const PrepassJob& ja, const PrepassJob& jb, int H, int W, int bs, const WorkList* work,
                   hipStream_t stream);

// ncc_fixup.hip: fix-up of the listed windows (+ the run spreading of an unranked call).  `tab`: the pattern-side table
// of a prepared pattern (ws.fix_tab_end), or null: the pattern side is staged in the kernel.
int launch_fixup(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames, int C, int H, int W,
                 int D, int bs, const FastWorkspace& ws, bool per_frame, const float* tab, const RankPlan* rank,
                 const float* best, unsigned* scan_counter, hipStream_t stream);
// the table itself, behind the pattern's pre-pass (ncc_fast_prepare_pattern_f32)
int launch_fixup_table(const float* in1, long in1_frame_stride, int C, int H, int W, int bs, const FastWorkspace& ws,
                       hipStream_t stream);

// ncc_tiles.hip: the volume by disparity groups, one accumulating launch per channel; bs in {3, 5, 7, 9}.  Block 9 with
// W % 4 == 0 and an aligned volume goes to the tile-256 kernel (ncc_t256.hip), every other shape to the wide + narrow pair.
int launch_tiles(float* out, int frames, int C, int H, int W, int D, int bs, const FastWorkspace& ws, long st1_stride,
                 hipStream_t stream);
int launch_t256(float* out, int frames, int C, int H, int W, int D, const FastWorkspace& ws, long st1_stride,
                hipStream_t stream);

// ncc_alld.hip ---------------------------------------------------------------------------
// How the all-D kernel cuts a call into workgroups: disparities per pass (dealt evenly over ceil(D / 30) passes), and
// the band height.  One workgroup per CU is resident (LDS), every workgroup costs about (rows + 8 warm-up rows) x passes,
// so the bands are chosen to minimise ceil(workgroups / 256) x (band rows rounded up to the 6-row unroll + 8).
struct AlldPlan {
  int n_pass, dgs, band_rows, bands, chunk_rows, n_psplit;
  size_t lds;                 // dynamic LDS of the launch: the staging ring, and the rank slots of a ranked plan
};
// `ranked`: the workgroup keeps the ranking of its pixels in LDS (band height limited by the slots, every disparity in one
// workgroup, n_psplit = 1).  Otherwise the band may be as tall as the image and the passes may be split over workgroups.
AlldPlan alld_plan(int frames, int H, int W, int D, bool ranked = true);

constexpr int kAStore = 1, kARank = 2;          // MODE bits of the all-D kernel: materialise the volume / rank the scores
// Block SAD / MSE cost volume through the same pipeline (with kAStore, never with kARank): the per-pixel
// plane |P[r][c - d] - I[r][c]| (squared for MSE) takes the place of the product a * b, and its 9 x 9 window sum / 81 is the
// output -- no statistics rows, no normalisation.  See costvol_sep_f32.
constexpr int kASad = 4, kAMse = 8;

// operand planes of an all-D launch (cost modes: value planes only, the statistics planes are null)
struct AlldOperands {
  const float *ac, *m0, *v0, *bc, *m1, *v1;
  long st1_stride;            // pattern planes: elements between two frames' planes (0: one pattern for all frames)
  int Wp, W1, xoff;
};
// The one launch of ncc_fast_alld_kernel<mode, plan's chunk rows>: block 9, W % 4 == 0, single channel, `out` 16-byte
// aligned.  kARank in `mode` <=> `rank` non-null (idx / best / flags / work list / eps come from it, the ranked plan
// applies); `out` may be null without kAStore.  `timed`: the launch is bracketed by the timing hooks.
int launch_alld(int mode, const AlldOperands& op, float* out, const RankPlan* rank, int frames, int H, int W, int D,
                bool timed, hipStream_t stream);

}  // namespace ctd
