/*
 * ctd_hip.h -- C ABI of libctd_hip.so, the MI355X (gfx950) implementation of the
 * disparity hot path of autonomousvision/connecting_the_dots.
 *
 * This is the drop-in boundary: each entry point replaces one pybind11 function of
 * the reference's CUDA extension (torchext/ext/ext_cuda.cpp:126-135) or fuses a chain
 * of stock PyTorch ops of model/networks.py.  Signatures carry plain device pointers,
 * sizes, a device ordinal and a hipStream_t (as void*); no torch / pybind types.
 *
 * Conventions
 *   - all tensors are dense, row-major, already resident in device memory;
 *   - the callee never allocates, frees or synchronises: outputs and workspaces are
 *     provided by the caller (the reference allocated outputs with ATen inside the
 *     call, ext_cuda.cpp:81,100,119; here the Python wrapper does it with torch.empty);
 *   - `device` is the HIP device ordinal the pointers live on (-1 = current device);
 *     `stream` is the hipStream_t to launch on (NULL = default stream).  The reference
 *     launched on the legacy default stream with no device guard (common_cuda.h:168);
 *   - return value: 0 on success, otherwise a ctd_status code (never exit(), unlike
 *     common_cuda.h:11-20); ctd_status_string() names it;
 *   - kernels are deterministic (no floating-point atomics) except ctd_geometric_bwd_f32, whose
 *     bilinear scatter into grad_depth1 uses float atomics like ATen's grid_sample backward.
 */
#ifndef CTD_HIP_H
#define CTD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum ctd_status {
  CTD_OK = 0,
  CTD_ERR_INVALID_ARG = 1,     /* bad size / null pointer / unsupported parameter        */
  CTD_ERR_WORKSPACE = 2,       /* workspace too small                                     */
  CTD_ERR_UNSUPPORTED = 3,     /* valid request this build has no kernel for              */
  CTD_ERR_HIP = 1000           /* 1000 + hipError_t of the failing runtime call           */
};

int ctd_version(void);                       /* ABI version, currently 5 (5, additive since: ctd_syn_finish_f32 / ctd_augment_f32 / ctd_salt_pepper_f32, ctd_costvol_argmin_f32 / ctd_costvol_argmin_workspace_bytes, ctd_xcorrvol_subpixel_f32 / ctd_xcorrvol_subpixel_workspace_bytes / ctd_costvol_subpixel_f32, ctd_hyperdepth_eval_f32 / ctd_hd_tables, ctd_hyperdepth_train_count_f32 / ctd_hyperdepth_train_workspace_bytes / ctd_hyperdepth_train_f32 / ctd_hd_train_params / ctd_hd_train_out, ctd_mesh_bvh_bytes / ctd_mesh_bvh_workspace_bytes / ctd_mesh_bvh_build_f32 / ctd_render_mesh_proj_bvh_f32 / ctd_render_mesh_bvh_f32, ctd_match_validity_f32 / ctd_xcorrvol_validity_f32 / ctd_xcorrvol_validity_workspace_bytes / ctd_costvol_validity_f32 / ctd_costvol_validity_workspace_bytes -- no existing signature changed; 5: + ctd_lcn_xcorrvol_argmax_f32 / ctd_lcn_xcorrvol_supported; 4: ctd_costvol_fast_f32 takes a workspace, ctd_costvol_workspace_bytes; 2: ranked argmax inside the all-D volume kernel, its workspace is ctd_xcorrvol_argmax_workspace_bytes(); 3: + ctd_xcorrvol_pattern_prepare_f32 / CTD_PATTERN_PREPARED, ctd_geometric_sym_fwd_f32) */
const char* ctd_status_string(int status);

/* (Bench instrumentation -- per-kernel device timing of the volume kernel -- is declared in ctd_hip_bench.h: it is not
 * part of the drop-in interface.) */

/* photometric loss types -- torchext/ext/ext.h:196-199, torchext/functions.py:106-118 */
#define CTD_PHOTOMETRIC_MSE 0
#define CTD_PHOTOMETRIC_SAD 1
#define CTD_PHOTOMETRIC_CENSUS_MSE 2
#define CTD_PHOTOMETRIC_CENSUS_SAD 3

/* algorithm selector of the NCC volume */
#define CTD_NCC_EXACT 0   /* reference operation order, bit-identical to ext_cpu.cpp        */
#define CTD_NCC_FAST 1    /* separable window sums; |a-b| <= 1e-5|b| + 1e-6 of the exact (C > 1: the sum of the
                             channels' bounds -- the volume is the sum of per-channel NCCs, and where two channels
                             cancel no f32 order keeps 1e-5 of the sum)                                     */

/* --------------------------------------------------------------------------------------
 * Zero-mean NCC block-matching volume.
 * Replaces  xcorrvol_cuda(in0, in1, n_disps, block_size)  -- ext_cuda.cpp:73-86,
 * kernel ext_kernel.cu:40-50, functor ext.h:120-191.
 *
 *   in0  [frames][C][H][W]   IR frames
 *   in1  [C][H][W]           pattern, shared by all frames when in1_frame_stride == 0,
 *                            else in1 + f*in1_frame_stride (elements) is frame f's pattern
 *   out  [frames][D][H][W]
 * The reference op has no batch axis (functions.py:73-74 is called per frame);
 * frames == 1 reproduces it exactly, frames > 1 is the same op applied per frame in
 * one launch.  `algo` = CTD_NCC_EXACT | CTD_NCC_FAST.
 * Workspace: ctd_xcorrvol_workspace_bytes() bytes, 256-byte aligned, contents scratch.
 * -------------------------------------------------------------------------------------- */
size_t ctd_xcorrvol_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo);

int ctd_xcorrvol_f32(const float* in0, const float* in1, long in1_frame_stride, float* out,
                     int frames, int C, int H, int W, int D, int block_size, int algo,
                     void* workspace, size_t workspace_bytes, int device, void* stream);

/* Pattern half of the fast path's pre-pass, ONCE per pattern: the reference prepares the pattern once per run
 * (model/exp_synph.py:64-71: LCN of the pattern in the Worker's constructor), its xcorrvol op re-reads it on every call.
 * Writes the pattern's window statistics, its list of windows for the fix-up pass, its run rows and (block 9, C = 1) the
 * pattern-side tables of the fix-up pass -- per listed pattern window the centred taps and the sum of their squares, up
 * to 4096 windows, in the unused end of that list's buffer (the workspace sizes are unchanged) -- into `workspace`
 * (ctd_xcorrvol_argmax_workspace_bytes() for the same frames / shape: the layout depends on all of them).  Afterwards
 * ctd_xcorrvol_f32 / ctd_xcorrvol_argmax_f32 calls with algo = CTD_NCC_FAST | CTD_PATTERN_PREPARED, the SAME workspace,
 * in1, in1_frame_stride, frames and shape skip that half.  The caller keeps the workspace to these calls in between. */
#define CTD_PATTERN_PREPARED 0x100
int ctd_xcorrvol_pattern_prepare_f32(const float* in1, long in1_frame_stride, int frames, int C, int H,
                                     int W, int D, int block_size, void* workspace,
                                     size_t workspace_bytes, int device, void* stream);

int ctd_xcorrvol_f64(const double* in0, const double* in1, long in1_frame_stride, double* out,
                     int frames, int C, int H, int W, int D, int block_size,
                     void* workspace, size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * argmax over the disparity axis:  idx = torch.argmax(vol, dim=0)  (first index wins
 * ties), best = vol.max(0).  No reference code.
 *   vol [frames][D][H][W] -> idx int64 [frames][H][W], best f32 [frames][H][W] (may be NULL)
 * -------------------------------------------------------------------------------------- */
int ctd_argmax_disp_f32(const float* vol, int64_t* idx, float* best, int frames, int D, int H,
                        int W, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * NCC volume + argmax over disparity (C == 1 only).
 * CTD_NCC_EXACT: fused, vol_out may be NULL (no volume written) or [frames][D][H][W]
 *   (written as well); indices equal torch.argmax(xcorrvol_cpu(...), 0) bit for bit and
 *   best is the reference-order score.
 * CTD_NCC_FAST: every disparity whose fast score lies within `rerank_eps` of the pixel's
 *   best is re-scored in reference order, so the indices are those of the reference-order
 *   volume whenever |fast - exact| <= rerank_eps / 2.  Where ctd_xcorrvol_rank_supported()
 *   holds (block 9, W % 4 == 0, D <= 512) the all-D volume kernel ranks the scores itself:
 *   one workgroup walks every disparity of its (column tile, band, frame) and keeps the best
 *   and the runner-up of every pixel in LDS, so idx / best leave that kernel directly (no
 *   partial planes, no second pass over the volume) and vol_out may be NULL: nothing is
 *   materialised then.  Otherwise vol_out is required (CTD_ERR_INVALID_ARG if NULL) and
 *   ranked in one more pass.  best = the fast score of idx to within 2.4e-7 absolute (the
 *   ranking keys are fixed point, 2^-21 apart; it is the reference-order score for re-scored
 *   pixels when no volume is written).
 *   rerank_eps < 0 = plain argmax of the fast scores, no exact re-scoring: defined on a
 *   materialised volume (vol_out != NULL: the patched volume is ranked in one more pass);
 *   without a volume a negative value is taken as 0.
 * Workspace: ctd_xcorrvol_argmax_workspace_bytes().
 * -------------------------------------------------------------------------------------- */
int ctd_xcorrvol_rank_supported(int C, int H, int W, int D, int block_size);
/* Inspection aid for tests / tools: how a ranked ctd_xcorrvol_argmax_f32 call is laid out.  offsets[0] = rows per band
 * of the all-D kernel, offsets[4] = its passes over the disparities; byte offsets inside the workspace of
 * offsets[1] = flag bytes [frames][H][W], offsets[2] = the work-list counters (16 x u32, 256 bytes apart, one per key =
 * image row & 15), offsets[3] = the work list (i64 flat pixel indices, 16 segments of ceil(frames * H / 16) * W entries,
 * one per key).  `offsets` has 5 entries. */
int ctd_xcorrvol_rank_layout(int frames, int H, int W, int D, int per_frame_pattern, size_t* offsets);
size_t ctd_xcorrvol_argmax_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo);
int ctd_xcorrvol_argmax_f32(const float* in0, const float* in1, long in1_frame_stride,
                            float* vol_out, int64_t* idx, float* best, int frames, int C, int H,
                            int W, int D, int block_size, int algo, float rerank_eps,
                            void* workspace, size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Photometric block loss, forward and backward.
 * Replaces photometric_loss_forward / photometric_loss_backward -- ext_cuda.cpp:92-123,
 * kernels ext_kernel.cu:54-112, functors ext.h:201-344.
 *   es, ta [B][C][H][W] -> out [B][1][H][W];  grad_out [B][1][H][W] -> grad_es [B][C][H][W]
 * `eps` is a C float for both dtypes, as in the reference binding (ext_cuda.cpp:92).
 * The backward is a deterministic gather (no atomics, no pre-zeroed buffer needed); the
 * reference scatter-adds with atomicAdd into at::zeros (ext.h:315,338-339).
 * -------------------------------------------------------------------------------------- */
int ctd_photometric_fwd_f32(const float* es, const float* ta, float* out, int B, int C, int H,
                            int W, int block_size, int type, float eps, int device, void* stream);
int ctd_photometric_bwd_f32(const float* es, const float* ta, const float* grad_out,
                            float* grad_es, int B, int C, int H, int W, int block_size, int type,
                            float eps, int device, void* stream);
/* Tolerance-level variants (f32, odd block sizes 3/5/7/9; CTD_ERR_UNSUPPORTED otherwise): same functions with
 * the summation order left free and v_rsq_f32 in place of the correctly rounded sqrt/divide chains;
 * |fast - reference| <= 1e-5 |reference| + 1e-6 (for the gradient: of the gradient's scale).  The backward
 * evaluates one term per pixel pair using K(q,p) = -K(p,q) (see ctd_photo_tile.h), no atomics. */
int ctd_photometric_fwd_fast_f32(const float* es, const float* ta, float* out, int B, int C, int H,
                                 int W, int block_size, int type, float eps, int device,
                                 void* stream);
int ctd_photometric_bwd_fast_f32(const float* es, const float* ta, const float* grad_out,
                                 float* grad_es, int B, int C, int H, int W, int block_size,
                                 int type, float eps, int device, void* stream);
int ctd_photometric_fwd_f64(const double* es, const double* ta, double* out, int B, int C, int H,
                            int W, int block_size, int type, float eps, int device, void* stream);
int ctd_photometric_bwd_f64(const double* es, const double* ta, const double* grad_out,
                            double* grad_es, int B, int C, int H, int W, int block_size, int type,
                            float eps, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * SAD / soft-census cost volume, defined by composition of reference ops:
 *   cost[d] = photometric_loss_forward(es = P_d, ta = I)[0,0],  P_d[h,x] = P[h, clamp(x-d)]
 *   im [frames][H][W], pattern [H][W] (stride as above) -> cost [frames][D][H][W]
 * -------------------------------------------------------------------------------------- */
int ctd_costvol_f32(const float* im, const float* pattern, long pattern_frame_stride, float* cost,
                    int frames, int H, int W, int D, int block_size, int type, float eps,
                    int device, void* stream);
/* tolerance-level variant (odd block sizes 3/5/7/9): |fast - exact| <= 1e-5 |exact| + 1e-6.
 * SAD / MSE with block 9 and W % 4 == 0 are evaluated as a replicate-border 9 x 9 box filter of the per-pixel plane
 * |P[r][clamp(c - d)] - I[r][c]| (one subtract per output instead of 81) by the NCC volume kernel's pipeline; that path
 * needs `workspace` (ctd_costvol_workspace_bytes(), 16-byte aligned; 0 bytes / NULL: the LDS-tiled 81-tap kernel runs
 * instead).  The census types use the census-transform kernel and no workspace.  (Signature since ABI version 4.)
 * pattern_frame_stride: 0 (one pattern for all frames) or H * W (dense per-frame patterns); anything else is
 * CTD_ERR_INVALID_ARG here -- ctd_costvol_f32 takes arbitrary strides. */
size_t ctd_costvol_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int per_frame_pattern);
int ctd_costvol_fast_f32(const float* im, const float* pattern, long pattern_frame_stride, float* cost,
                    int frames, int H, int W, int D, int block_size, int type, float eps,
                    void* workspace, size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * argmin over the disparities of the SAD / soft-census cost volume, without the volume (additive in ABI version 5).
 *   Arguments as ctd_costvol_fast_f32 (pattern_frame_stride 0 or H * W), outputs idx int64 [frames][H][W] and best f32
 *   [frames][H][W] (may be NULL).  Nothing of size frames * D * H * W is written.
 *   idx == torch.argmin(V, 1) bit for bit, first index on ties, V = the ctd_costvol_f32 volume of the same arguments.
 * How: the tolerance-level volume kernel (census transform for the census types, the LDS-tiled kernel for SAD / MSE, all
 * block sizes) ranks its costs instead of storing them: per pixel and 128 disparities the best fast cost b1, its first
 * index i1 and the runner-up b2.  A pixel's fast winner is accepted when
 *     b2 - b1 > rerank_rel * (b1 + b2) + 2e-6
 * which, under the fast bound |fast - exact| <= rerank_rel |exact| + 1e-6, implies exact(i1) < exact(d) for every other d
 * (costvol_argmin.hip has the derivation); every other pixel (exact ties included) is re-scored: all D costs in the
 * reference order, first-index argmin.
 *   rerank_rel: 1e-5 (the default of the Python wrapper) = the bound ctd_costvol_fast_f32 documents; larger values
 *     re-score more pixels; < 0 = plain argmin of the fast costs, nothing re-scored (indices may then differ from V's
 *     where two costs lie within the bound); NaN = CTD_ERR_INVALID_ARG.
 *   best: for a re-scored pixel the reference-order cost V[f][idx][h][w], bit for bit; for every other pixel the fast
 *     cost of idx, within 1e-5 |V| + 1e-6.
 * Workspace: ctd_costvol_argmin_workspace_bytes() bytes, 256-byte aligned, O(frames * H * W * ceil(D / 128)):
 *   bytes [0, 4): u32 number n of re-scored pixels (0 when rerank_rel < 0),
 *   bytes [256, 256 + 4 n): their flat indices f * H * W + h * W + w (u32, order unspecified), then the rank triples.
 * Errors, before any HIP call: an even block size, a type outside 0..3 or a stride other than 0 / H * W is
 * CTD_ERR_INVALID_ARG; block sizes other than 3/5/7/9, frames * H * W >= 2^32 or grids beyond the launch limits are
 * CTD_ERR_UNSUPPORTED (compose ctd_costvol_f32 and an argmin then).  The workspace query returns 0 for both and for
 * frames == 0.
 * -------------------------------------------------------------------------------------- */
size_t ctd_costvol_argmin_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int per_frame_pattern);
int ctd_costvol_argmin_f32(const float* im, const float* pattern, long pattern_frame_stride,
                           int64_t* idx, float* best, int frames, int H, int W, int D, int block_size, int type,
                           float eps, float rerank_rel, void* workspace, size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Sub-pixel refinement of a matcher index (additive in ABI version 5): a parabola or equiangular fit through the
 * reference-order scores at d-1, d, d+1 around d = idx[f][h][w].
 *   NCC:   the scores of ctd_xcorrvol_f32(CTD_NCC_EXACT) (bit-identical to the reference), a maximum; C == 1.
 *   Costs: the costs of ctd_costvol_f32 of the same arguments, a minimum.
 * The refined disparity is a function of these three volume entries alone, evaluated in float32 in this order (no FMA,
 * IEEE divide):
 *   NCC (maximum; sm, s0, sp = exact scores at d-1, d, d+1):
 *     parabola:    den = (sm - s0) + (sp - s0); refined iff den < 0, then delta = 0.5f * ((sm - sp) / den)
 *     equiangular: if sp > sm: delta = 0.5f * ((sp - sm) / (s0 - sm)), refined iff s0 - sm > 0
 *                  else:       delta = 0.5f * ((sp - sm) / (s0 - sp)), refined iff s0 - sp > 0
 *   Costs (minimum; cm, c0, cp = exact costs at d-1, d, d+1):
 *     parabola:    den = (cm - c0) + (cp - c0); refined iff den > 0, then delta = 0.5f * ((cm - cp) / den)
 *     equiangular: if cp < cm: delta = 0.5f * ((cm - cp) / (cm - c0)), refined iff cm - c0 > 0
 *                  else:       delta = 0.5f * ((cm - cp) / (cp - c0)), refined iff cp - c0 > 0
 *   For both families: delta is clamped to [-0.5f, 0.5f] (this only matters when idx is not the exact argmax / argmin,
 *   e.g. with rerank_eps < 0); disp = (float)d + delta where refined, (float)d where not (the not-refined cases include
 *   d == 0, d == D-1 and 0/0 on flat windows); an idx outside [0, D) gives disp = NaN and refined = 0 and is never
 *   used to read.
 * Outputs disp f32 [frames][H][W] and refined u8 [frames][H][W] (may be NULL).  idx int64 [frames][H][W].
 * The soft-census costs are too non-linear in d for either fit to improve accuracy; their refinement is defined (and
 * tested bit for bit) but not recommended.
 * mode: CTD_SUBPIXEL_PARABOLA or CTD_SUBPIXEL_EQUIANGULAR.  For the NCC call mode may carry CTD_PATTERN_PREPARED: the
 *   workspace then already holds the pattern planes of an earlier call with the same in1, frames, H, W, D, block_size
 *   and stride, and only the frame half is recomputed.
 * Workspace (NCC only): ctd_xcorrvol_subpixel_workspace_bytes() bytes, 256-byte aligned: the quotients x / bs^2 of the
 *   frames and the pattern(s), and (mean, sum of squared deviations) of every pattern window centre x in [-(D-1), W-1].
 * Errors, before any HIP call (CTD_ERR_INVALID_ARG): an even or < 1 block size, a mode outside {0, 1}, a type outside
 * 0..3, a stride other than 0 / H * W, D < 1, H or W < 1, frames < 0, D * H * W >= 2^31, a NULL in0 / in1 / im /
 * pattern / idx / disp, or a workspace that is NULL, too small or not 256-byte aligned.  frames == 0 is CTD_OK.  The
 * workspace query returns 0 for invalid shapes and for frames == 0.
 * -------------------------------------------------------------------------------------- */
#define CTD_SUBPIXEL_PARABOLA 0
#define CTD_SUBPIXEL_EQUIANGULAR 1
size_t ctd_xcorrvol_subpixel_workspace_bytes(int frames, int H, int W, int D, int block_size, int per_frame_pattern);
int ctd_xcorrvol_subpixel_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                              float* disp, uint8_t* refined, int frames, int H, int W, int D, int block_size, int mode,
                              void* workspace, size_t workspace_bytes, int device, void* stream);
int ctd_costvol_subpixel_f32(const float* im, const float* pattern, long pattern_frame_stride, const int64_t* idx,
                             float* disp, uint8_t* refined, int frames, int H, int W, int D, int block_size, int type,
                             float eps, int mode, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Match validity (additive in ABI version 5): which disparities of a winner-takes-all matcher can be trusted -- the
 * left-right consistency check and the uniqueness check of classical stereo / structured-light matchers.
 *
 * Definitions.  Let V[f][d][h][w] be the reference-order volume: for NCC the volume of ctd_xcorrvol_f32(CTD_NCC_EXACT),
 * higher is better; for the costs the volume of ctd_costvol_f32, lower is better.  Below, "better" and "best" follow
 * the family.  Inputs are assumed finite.  idx is the int64 [frames][H][W] index tensor the caller passes, normally the
 * matcher's output; any index is accepted, as in the sub-pixel ops.
 *   1. Pattern-side match idx_r[f][h][x] (int64 [frames][H][W], x = pattern column): the first index of the best
 *      V[f][d][h][x + d] over d in [0, min(D, W - x)) -- the disparity at which pattern column x is best explained by
 *      the frame, by the same scores and the same tie rule as the frame-side argmax.  The range is never empty
 *      (d = 0 is always in it).
 *   2. gap[f][h][w] (f32).  With d0 = idx, s1 = V[d0] and s2 = the best V[d] over |d - d0| >= 2:
 *      NCC: gap = s1 - s2;  costs: gap = s2 - s1;  both one f32 subtraction.  gap = +inf when no such d exists,
 *      gap = NaN when idx is outside [0, D).
 *   3. flags[f][h][w] (uint8 bit field):
 *      bit 0 IN_PATTERN: 0 <= idx < D and x = w - idx >= 0 (such a match does not rest on the replicated left border,
 *            ext.h:152-154);
 *      bit 1 LR_OK: bit 0 holds and |idx_r[f][h][x] - idx| <= lr_tol (lr_tol an int >= 0);
 *      bit 2 UNIQUE: 0 <= idx < D and gap > min_gap (an f32 compare; +inf passes; min_gap an f32 >= 0).
 *      valid = (flags == 7).
 *
 * ctd_match_validity_f32: the three outputs of a caller-supplied volume vol [frames][D][H][W], taken as exact (it IS V).
 *   maximise != 0: higher is better (NCC), 0: lower is better (costs).  No workspace.  idx, flags, idx_r and gap must
 *   not overlap.
 * ctd_xcorrvol_validity_f32 / ctd_costvol_validity_f32: compute the volume into the workspace (ctd_xcorrvol_f32 with
 *   `algo`; ctd_costvol_f32 for algo = CTD_NCC_EXACT, ctd_costvol_fast_f32 for CTD_NCC_FAST -- the same 0 / 1), then
 *   the three outputs.  What is exact: idx_r and flags are those of V bit for bit with either algo.  gap equals V's gap
 *   bit for bit with CTD_NCC_EXACT; with CTD_NCC_FAST it is within 1e-5 (|s1| + |s2|) + 2e-6 of it (the sum of the fast
 *   bounds of its operands) and bit-exact on the re-scored pixels.
 *   How CTD_NCC_FAST keeps decisions exact: a decision taken on fast scores is accepted only where the fast bound
 *   |fast - exact| <= 1e-5 |exact| + 1e-6 proves it -- pattern side: best and runner-up of the diagonal (the runner-up
 *   anywhere) farther apart than both bounds; uniqueness: |gap_fast - min_gap| larger than both bounds plus the
 *   rounding of the subtraction (csrc/match_validity.hip has the derivation).  Every other pixel / pattern column,
 *   exact ties included, goes on a list; all its D scores are evaluated again in the reference order and the decision
 *   is taken on them.  LR_OK is taken after the pattern-side list is resolved.  Each list has room for every pixel /
 *   column.
 *   Arguments as ctd_xcorrvol_f32 (in1_frame_stride 0 or C * H * W) / ctd_costvol_fast_f32 (pattern_frame_stride 0 or
 *   H * W).
 * Workspace: *_validity_workspace_bytes() bytes, 256-byte aligned.  With P = frames * H * W:
 *   bytes [0, 4): u32 number of re-scored pixels, bytes [4, 8): u32 number of re-scored pattern columns (both 0 with
 *   CTD_NCC_EXACT); from byte 256: the re-scored pixels' flat indices f * H * W + h * W + w (u32, order unspecified);
 *   from byte 256 + 4 P rounded up to a multiple of 256: the re-scored columns' flat indices f * H * W + h * W + x;
 *   then the volume and the volume kernels' scratch.
 * Errors, before any HIP call: CTD_ERR_INVALID_ARG for lr_tol < 0, a negative or NaN min_gap, an algo / type outside its
 *   values, a pattern stride other than the two above, bad sizes (D * H * W >= 2^31 included) or a NULL pointer;
 *   CTD_ERR_UNSUPPORTED for H or frames > 65535, frames * H * W >= 2^32, CTD_NCC_FAST with C > 1, D > 512 or a block
 *   size outside 3/5/7/9 (use CTD_NCC_EXACT), and the exact cost volume with frames * D > 65535; CTD_ERR_WORKSPACE for a
 *   NULL, short or misaligned workspace.  frames == 0 is CTD_OK.  The workspace queries return 0 for all of these.
 * -------------------------------------------------------------------------------------- */
#define CTD_VALID_IN_PATTERN 1
#define CTD_VALID_LR_OK 2
#define CTD_VALID_UNIQUE 4
int ctd_match_validity_f32(const float* vol, int maximise, const int64_t* idx, uint8_t* flags, int64_t* idx_r, float* gap,
                           int frames, int D, int H, int W, int lr_tol, float min_gap, int device, void* stream);
size_t ctd_xcorrvol_validity_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo);
int ctd_xcorrvol_validity_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                              uint8_t* flags, int64_t* idx_r, float* gap, int frames, int C, int H, int W, int D,
                              int block_size, int algo, int lr_tol, float min_gap, void* workspace,
                              size_t workspace_bytes, int device, void* stream);
size_t ctd_costvol_validity_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int algo,
                                            int per_frame_pattern);
int ctd_costvol_validity_f32(const float* im, const float* pattern, long pattern_frame_stride, const int64_t* idx,
                             uint8_t* flags, int64_t* idx_r, float* gap, int frames, int H, int W, int D, int block_size,
                             int type, float eps, int algo, int lr_tol, float min_gap, void* workspace,
                             size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Semi-global cost aggregation (additive in ABI version 5): Hirschmueller's SGM path aggregation over a materialised
 * volume, the step between "cost volume" and "argmin" that lets a pixel's choice be informed by its neighbours.
 *
 * Definition (f32 throughout; only add, sub and min, so the result is defined bit for bit).  The input is
 * vol [frames][D][H][W].  C = vol when maximise == 0 (costs, lower is better), C = -vol otherwise (scores; the negation is
 * exact).  A path direction is a step (dy, dx); the predecessor of pixel p = (y, x) is q = (y - dy, x - dx).
 *   q outside the image:  L(p,d) = C(p,d)
 *   otherwise:            m = min_k L(q,k)
 *                         t = min(L(q,d), m + P2, L(q,d-1) + P1 [if d >= 1], L(q,d+1) + P1 [if d + 1 < D])
 *                         L(p,d) = C(p,d) + (t - m)                                   in exactly that association
 * Directions, as (dy, dx): right (0,+1), left (0,-1), down (+1,0), down-right (+1,+1), down-left (+1,-1), up (-1,0),
 * up-right (-1,+1), up-left (-1,-1).  The sum is taken in a fixed order:
 *   paths = 4:  S = ((L_right + L_left) + L_down) + L_up
 *   paths = 8:  S = ((((((L_right + L_left) + L_down) + L_down_right) + L_down_left) + L_up) + L_up_right) + L_up_left
 * Outputs: S (optional), idx [frames][H][W] = argmin_d S (int64, the first index wins), best = S[idx] (f32).  S and best
 * are in COST sign also when maximise != 0 (lower is better; they are sums of -vol plus penalties).
 * Arguments: 0 <= P1 <= P2, both finite.  Inputs must be finite; non-finite inputs give unspecified values.
 *
 * ctd_sgm_aggregate_f32: S_out [frames][D][H][W] or NULL; when NULL, S lives in the workspace
 *   (ctd_sgm_workspace_bytes(..., want_volume = 0) = frames * D * H * W floats, 16-byte aligned; 0 bytes and no workspace
 *   with want_volume != 0).  vol is never written and must not overlap S_out or the workspace; the contents of S_out and
 *   of the workspace on entry do not matter.  Every D in [1, 256] and every H, W >= 1 is supported.
 * Errors, before any HIP call: CTD_ERR_INVALID_ARG for paths outside {4, 8}, p1 < 0, p2 < p1, a non-finite penalty, a
 *   size <= 0, frames * D * H * W >= 2^31 or a NULL vol / idx / best; CTD_ERR_UNSUPPORTED for D > 256;
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace when S_out is NULL.  The workspace query returns 0 for
 *   the first two.
 * -------------------------------------------------------------------------------------- */
size_t ctd_sgm_workspace_bytes(int frames, int D, int H, int W, int paths, int want_volume);
int ctd_sgm_aggregate_f32(const float* vol, int maximise, float p1, float p2, int paths, float* S_out, int64_t* idx,
                          float* best, int frames, int D, int H, int W, void* workspace, size_t workspace_bytes,
                          int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Disparity post-filters (additive in ABI version 5): the step after the validity flags, on the disparity map itself --
 * speckle removal (connected components) and a validity-aware median.  Both look at a pixel's neighbours.
 *
 * Common terms.  All maps are [frames][H][W]; disparities are f32.  A pixel is LIVE when its `valid` byte is nonzero and
 * its disparity is finite; a NULL `valid` counts as nonzero everywhere.  The inputs are never written and the outputs
 * must not overlap them or the workspace.
 *
 * 1. Components, ctd_disp_components_f32.  Two neighbouring pixels p, q are LINKED when both are live and
 *      fabsf(disp[p] - disp[q]) <= max_diff                                              (one f32 subtraction).
 *    Neighbours are the 4 edge neighbours (connectivity = 4) plus the 4 diagonal ones (connectivity = 8), inside the
 *    frame; nothing crosses frames.  Components are the transitive closure of the links (a chain 0, 1, 2, 3 with
 *    max_diff = 1 is one component although its ends differ by 3).  Outputs:
 *      label (int32) = the smallest in-frame linear index h * W + w among the pixels of p's component; -1 if p is not live
 *      size  (int32) = the number of pixels of p's component; 0 if p is not live
 *    Both are fully determined: the kernels use integer atomics only (a minimum for the unions, an add for the counts),
 *    and the root of a set is its smallest index whatever order they land in.  max_diff = +inf is allowed and gives the
 *    components of the live mask.  Every H, W >= 1 is supported.
 *    Workspace: ctd_disp_components_workspace_bytes(frames, H, W) bytes, 16-byte aligned (three int32 per pixel); its
 *    contents on entry, and those of the outputs, do not matter.
 * 2. Speckle filter, ctd_disp_speckle_f32.  With the components of 1:
 *      keep (uint8) = 1 where p is live and size > max_size, 0 elsewhere
 *    i.e. components of at most max_size pixels are removed (the rule of OpenCV's filterSpeckles); max_size = 0 keeps
 *    every live pixel.  `size` is optional (NULL: not written).  Same workspace as 1.
 * 3. Masked median, ctd_disp_median_f32, window = 3, 5 or 7.  For pixel p collect the disparities of the live pixels
 *    inside the window x window square centred on p -- in-image pixels only, no border replication -- and let m be their
 *    number.  Put them in ascending order; equal values (the two signed zeros compare equal) keep the raster order of
 *    the window, rows first.
 *      p live:                                   out = the element of rank (m - 1) / 2 (integer division: the lower
 *                                                median; p itself is in the window, so m >= 1), valid_out = 1
 *      p not live, fill_min > 0, m >= fill_min:  the same (hole filling)
 *      otherwise:                                out = NaN, valid_out = 0
 *    The result is a selection, so it is defined bit for bit.  No workspace.
 * Errors, before any HIP call: CTD_ERR_INVALID_ARG for a negative or NaN max_diff, a connectivity outside {4, 8}, a
 *   negative max_size or fill_min, a window outside {3, 5, 7}, H <= 0, W <= 0, frames < 0, H * W >= 2^31,
 *   frames * H * W >= 2^31, a NULL disp or output other than the speckle filter's `size`, or a median output that is
 *   one of its inputs; CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.  frames == 0 is CTD_OK and touches
 *   nothing.  The workspace query returns 0 for sizes the calls reject.
 * -------------------------------------------------------------------------------------- */
size_t ctd_disp_components_workspace_bytes(int frames, int H, int W);
int ctd_disp_components_f32(const float* disp, const uint8_t* valid, float max_diff, int connectivity, int32_t* label,
                            int32_t* size, int frames, int H, int W, void* workspace, size_t workspace_bytes, int device,
                            void* stream);
int ctd_disp_speckle_f32(const float* disp, const uint8_t* valid, float max_diff, int max_size, int connectivity,
                         uint8_t* keep, int32_t* size, int frames, int H, int W, void* workspace, size_t workspace_bytes,
                         int device, void* stream);
int ctd_disp_median_f32(const float* disp, const uint8_t* valid, int window, int fill_min, float* out, uint8_t* valid_out,
                        int frames, int H, int W, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Multi-view depth consistency and point-cloud fusion (additive in ABI version 5): the multi-view counterpart of the
 * validity flags, and the step from the depth maps of a track -- several views of one scene with known poses -- to a
 * point cloud.  The reference has no counterpart (its co/geometry.py projects single depth maps on the CPU), so the
 * rules are defined here, bit for bit: they use IEEE f32 add, sub, mul, div, floor and compares only, in the written
 * association, never contracted to fused multiply-adds.
 *
 * Common terms.  depth [B][V][H][W] f32: V views of one track, B tracks.  valid [B][V][H][W] uint8 or NULL (NULL counts
 * as nonzero everywhere).  ray [H*W][3] and K [3][3] are shared by the call, exactly as ctd_geometric_fwd_f32 takes
 * them.  Poses R [B][V][3][3], t [B][V][3] in the convention of the geometric loss: X_cam = R X_world + t.  A pixel is
 * LIVE when its valid byte is nonzero and its depth is finite and greater than 0.
 * The transform from view a to view b of depth d at pixel q (in-view linear index), in the association of the geometric
 * loss's forward:
 *      P_i   = d*ray[q][i] - t_a[i]
 *      Q_j   = P0*Ra[0][j] + P1*Ra[1][j] + P2*Ra[2][j]
 *      S_j   = Q0*Rb[j][0] + Q1*Rb[j][1] + Q2*Rb[j][2] + t_b[j]
 *      uvd_j = S0*K[j][0] + S1*K[j][1] + S2*K[j][2]
 * and the pixel coordinates are u = uvd0/uvd2, v = uvd1/uvd2 (IEEE division).  This is the geometric projection itself,
 * NOT the coordinate ctd_geometric_fwd_f32 samples at: that one is normalised with (W-1), (H-1) and un-normalised by
 * grid_sample with align_corners = False, a quirk of the reference's training loss that has to be kept there for parity
 * and that a consistency check must not inherit.
 *
 * 1. ctd_depth_consistency_f32.  For each reference view r, each live pixel p = (y, x) of it with depth d_r, and each
 *    source view s != r of the same track:
 *    a. uvd = transform r -> s of d_r at p; fail unless uvd2 > 0; u1 = uvd0/uvd2, v1 = uvd1/uvd2;
 *       xs = floorf(u1 + 0.5f), ys = floorf(v1 + 0.5f); fail unless 0 <= xs <= W-1 and 0 <= ys <= H-1 (float compares,
 *       before any conversion: a NaN fails); fail unless the source pixel q = (ys, xs) of view s is live.  The sampling
 *       is nearest neighbour on purpose: a bilinear one would mix depths across occlusion edges and holes.
 *    b. uvd' = transform s -> r of d_s at q; fail unless uvd'2 > 0; u' = uvd'0/uvd'2, v' = uvd'1/uvd'2, z' = uvd'2.
 *    c. with du = u' - (float)x, dv = v' - (float)y, view s is CONSISTENT with (r, p) iff
 *         du*du + dv*dv <= max_px*max_px   and   fabsf(z' - d_r) <= max_rel*d_r.
 *    Outputs, all [B][V][H][W]:
 *      count (uint8) = the number of consistent source views; 0 for a pixel that is not live
 *      keep  (uint8) = 1 where the pixel is live and count >= min_views, else 0
 *      fused (f32)   = acc / (float)(1 + count), where acc starts as d_r and takes acc = acc + z'_s for each consistent
 *                      view in ascending s; NaN where keep == 0
 *    V = 1 gives count = 0 everywhere; min_views = 0 keeps exactly the live pixels with fused = depth.
 * 2. ctd_depth_fuse_points_f32 runs 1 and then decides per pixel whether to emit it:
 *      dedupe == 0: emit(r, p) = keep(r, p)
 *      dedupe != 0: keep(r, p), and there is no s < r such that s is consistent with (r, p) and keep(s, q_s(r, p)) holds,
 *                   q_s(r, p) being the source pixel of step a
 *    ("first view wins": it removes most duplicates of a surface that several views see; it is a definition, not a
 *    symmetry claim).  For every emitted pixel, with fused of 1:
 *      P_i = fused*ray[p][i] - t_r[i];   point_j = P0*R_r[0][j] + P1*R_r[1][j] + P2*R_r[2][j]       (a world point)
 *      src = ((b*V + r)*H + y)*W + x                                                   (the flat index of the pixel)
 *    points [M][3] f32 and src [M] int64 are written densely in ascending src order -- tracks one after the other --
 *    and n_per_track [B] int64 gets the number of points of each track (M = their sum).  The caller provides points and
 *    src with the capacity B*V*H*W; entries from M on are left as they were.  count, keep and fused of 1 are written
 *    as well where their pointers are given; each of the three may be NULL.
 *    Workspace: ctd_depth_fuse_workspace_bytes(B, V, H, W) bytes, 256-byte aligned; its contents on entry, and those of
 *    the outputs, do not matter.  The compaction is three launches (counts per workgroup, their exclusive scan in one
 *    workgroup, the scatter); no workgroup waits for another and there are no atomics, so every run gives the same bits.
 * The inputs are never written; the outputs must not overlap the inputs, each other or the workspace.
 * Limits: V in [1, 64]; B*V*H*W < 2^31; every H, W >= 1 up to 2^24 (W - 1 and H - 1 are compared in f32); fewer than
 *   2^24 workgroups per launch, B*V*ceil(W/64)*ceil(H/4) < 2^24 and B*V*ceil(H*W/256) < 2^24, which only a batch of more
 *   than four million views of under 1024 pixels each can reach (a launch stays below 2^32 threads).
 * Errors, before any HIP call: CTD_ERR_INVALID_ARG for a negative or non-finite max_px or max_rel, min_views outside
 *   [0, 255], B < 0, V < 1, H < 1, W < 1, H or W > 2^24, B*V*H*W >= 2^31, a NULL pointer other than valid (and, for the
 *   fusion, count / keep / fused) or overlapping buffers; CTD_ERR_UNSUPPORTED for V > 64 or 2^24 workgroups and more; CTD_ERR_WORKSPACE for a NULL,
 *   short or misaligned workspace.  B == 0 is CTD_OK and touches nothing.  The workspace query returns 0 for sizes the
 *   calls reject (and for B == 0).
 * -------------------------------------------------------------------------------------- */
int ctd_depth_consistency_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                              const float* t, float max_px, float max_rel, int min_views, uint8_t* count, uint8_t* keep,
                              float* fused, int B, int V, int H, int W, int device, void* stream);
size_t ctd_depth_fuse_workspace_bytes(int B, int V, int H, int W);
int ctd_depth_fuse_points_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                              const float* t, float max_px, float max_rel, int min_views, int dedupe, float* points,
                              int64_t* src, int64_t* n_per_track, uint8_t* count, uint8_t* keep, float* fused, int B,
                              int V, int H, int W, void* workspace, size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Local contrast normalisation, fused.  Replaces the op chain of LCN.tforward,
 * model/networks.py:507-533 (ReflectionPad2d + two all-ones Conv2d + 6 elementwise ops).
 *   x [N][1][H][W] -> y = (x-avg)/std, std  (both [N][1][H][W]);  radius < min(H, W)
 * Box sums in f64 in the order of the CPU oracle (rows, then columns, ascending), rounded once, and the reference's f32
 * tail: the oracle's bits at every pixel (tests/test_lcn_f64_gpu.py, trap and high-dynamic-range frames included).
 * -------------------------------------------------------------------------------------- */
int ctd_lcn_f32(const float* x, float* y, float* std_out, int N, int H, int W, int radius,
                float eps, int device, void* stream);
/* tolerance-level variant, radius 7 only (CTD_ERR_UNSUPPORTED otherwise: at radii 1 .. 6 it failed the float64 rule
 * below, on frames with dark and bright rows and on flat quantised levels; call ctd_lcn_f32): f32 sliding-window box
 * sums of samples centred per 64 x 16 tile by a constant between 0 and every sample of the tile (0 where the tile
 * reaches zero, its mean where every sample is within a factor 2 of it, else the sample closest to zero).  Every output within
 * 1e-6 |b| + 1e-6 + 64 u kappa of the float64 LCN (u = 2^-24, kappa from the window's f64 E[x^2], var and std: the rule
 * of tests/test_lcn_f64_gpu.py), with its largest error at most 1.25 x the stock-torch f32 error plus that floor. */
int ctd_lcn_fast_f32(const float* x, float* y, float* std_out, int N, int H, int W, int radius,
                     float eps, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * LCN of the frames + NCC volume + argmax over disparity in one call (C == 1): the step
 *   ir = LCN(raw)  (model/networks.py:507-533, applied to the input images at model/exp_synph.py:84-91)
 *   vol = xcorrvol(ir, pattern)  (ext_cuda.cpp:73-86);  idx = argmax_d vol
 * of a matcher built on the reference's ops, without the round trip of the LCN output through memory before the
 * matcher's window statistics: one streaming kernel (a wavefront per 232-column strip and band of rows) reads the raw
 * frames once and writes lcn_out, std_out and the frame-side planes of the fast NCC path.
 *   raw [frames][1][H][W] -> lcn_out, std_out [frames][1][H][W] (both required);  in1 = the LCN'd pattern, as for
 *   ctd_xcorrvol_argmax_f32, whose remaining arguments, outputs, workspace and CTD_PATTERN_PREPARED rule apply unchanged
 *   (algo = CTD_NCC_FAST [| CTD_PATTERN_PREPARED]).
 * lcn_algo: CTD_LCN_EXACT -- f64 box sums (a fresh 11-row sum per row) and the reference's f32 elementwise tail:
 *   lcn_out / std_out carry the bits of ctd_lcn_f32 wherever a window's f64 sums are exact in any order, that is where
 *   hi - lo <= 53 with hi = ceil(log2 sum |v|) over the window and lo the lowest set bit of its nonzero samples, for the
 *   samples and for their f32 squares alike; no rounding outlives the window it was made in;
 *   CTD_LCN_FAST -- f32 sums of samples centred by one constant per wavefront (the in-image sample nearest zero of the
 *   first row a band reads), sliding over the band's rows, v_rcp / v_sqrt tail: within 1e-6 |b| + 4e-6 + 64 u kappa of
 *   the float64 LCN (the rule of tests/test_lcn_f64_gpu.py; the 4e-6 is an estimate of the rounding a bright sample of
 *   magnitude up to 1 leaves in a band's sliding sums, tested at bands of up to 64 rows), and at most 1.25 x the
 *   stock-torch f32 error plus that floor -- on frames without long runs of a dark level next to a bright one: a dark
 *   window below a bright first row cancels against that centre, and one after a bright level has slid out of the sums
 *   keeps its roundings (std 7.6 x that bound, 3.3 x the stock-f32 error, on rows of 0.02 under rows of 0.7 .. 1).  Use CTD_LCN_EXACT there.
 * rerank_eps < 0 ranks with eps = 0 here: there is no plain argmax of the fast scores (a caller that wants one with a
 *   volume calls ctd_lcn_f32 + ctd_xcorrvol_argmax_f32, as the Python wrapper does).
 * Supported where ctd_lcn_xcorrvol_supported() says so (radius 5, block 9, W % 4 == 0, W >= 16, H >= 11 and the ranked
 * fast path of ctd_xcorrvol_rank_supported()); CTD_ERR_UNSUPPORTED otherwise (call ctd_lcn_f32 + ctd_xcorrvol_argmax_f32).
 * -------------------------------------------------------------------------------------- */
#define CTD_LCN_EXACT 0
#define CTD_LCN_FAST 1
int ctd_lcn_xcorrvol_supported(int H, int W, int D, int radius, int block_size);
int ctd_lcn_xcorrvol_argmax_f32(const float* raw, float* lcn_out, float* std_out, int radius, float lcn_eps, int lcn_algo,
                                const float* in1, long in1_frame_stride, float* vol_out, int64_t* idx, float* best,
                                int frames, int H, int W, int D, int block_size, int algo, float rerank_eps,
                                void* workspace, size_t workspace_bytes, int device, void* stream);

/* Data-generation variant, data/lcn/lcn.pyx:16-58 (`lcn.normalize(img, kernel_size, epsilon)`): two-pass window mean
 * / std in f32 in the Cython loop's tap order (bit-identical), out = (x - mean) / (std + eps), out_std = raw std, a
 * border of width kernel_size stays zero.  img, out, out_std [N][H][W]. */
int ctd_lcn_datagen_f32(const float* img, float* out, float* out_std, int N, int H, int W,
                        int kernel_size, float eps, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * DispToDepth.tforward, model/networks.py:313-321, and its backward.
 *   depth = (baseline*focal) / (relu(disp) + 1e-12)
 * -------------------------------------------------------------------------------------- */
int ctd_disp_to_depth_fwd_f32(const float* disp, float* depth, long n, float baseline_focal,
                              int device, void* stream);
int ctd_disp_to_depth_bwd_f32(const float* disp, const float* grad_depth, float* grad_disp, long n,
                              float baseline_focal, int device, void* stream);
/* Same forward for a disparity given as the argmax index of ctd_xcorrvol_argmax_f32 (int64) plus a constant offset:
 * depth = (baseline*focal) / (relu(float(idx) + disp_offset) + 1e-12).  Not differentiable (additive, no reference
 * counterpart: saves the int64 -> float and offset passes between the matcher and the geometric loss). */
int ctd_idx_to_depth_f32(const int64_t* idx, float* depth, long n, float baseline_focal, float disp_offset,
                         int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Edge-aware disparity loss: SobelFilter (5x5, replicate pad) + DisparityLoss.tforward,
 * model/networks.py:380-412, 537-565, fused.
 *   disp [B][1][H][W], edge [B][1][H][W] or NULL  ->  loss[0] (device scalar, mean over B*H*W)
 *   with edge   : mean(-log(clamp((1-e)/b0*exp(-g/b0) + e/b1*exp(-g/b1), 1e-4)))
 *   without edge: mean(clamp(g, 0, 1)),   g = sqrt(gx^2 + gy^2 + 1e-8)
 * Backward: grad_loss is a device scalar; grad_disp always written, grad_edge optional (NULL).
 * Workspace: ctd_disparity_loss_workspace_bytes() bytes, shared layout for both directions.
 * -------------------------------------------------------------------------------------- */
size_t ctd_disparity_loss_workspace_bytes(int B, int H, int W);
int ctd_disparity_loss_fwd_f32(const float* disp, const float* edge, float* loss, int B, int H, int W,
                               void* workspace, size_t workspace_bytes, int device, void* stream);
int ctd_disparity_loss_bwd_f32(const float* disp, const float* edge, const float* grad_loss,
                               float* grad_disp, float* grad_edge, int B, int H, int W,
                               void* workspace, size_t workspace_bytes, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Two-view geometric loss, ONE direction: ProjectionDepthSimilarityLoss.fwd,
 * model/networks.py:483-498 (unproject depth0 along `ray`, rigid transform by (R0,t0) then
 * (R1,t1), project with K, bilinear border-mode sample of depth1, mean clamped |d - sample|).
 *   depth0, depth1 [B][1][H][W]; ray [H*W][3] = [u v 1] @ Ki^T (networks.py:428-434);
 *   K [3][3]; R0, R1 [B][3][3]; t0, t1 [B][3]  (all device, f32);  clamp <= 0 disables clamping
 *   loss[0] = (accumulate ? loss[0] : 0) + mean            (the module sums both directions)
 * Backward: grad_depth0 = (accumulate0 ? grad_depth0 : 0) + d/d depth0; grad_depth1 is
 * ACCUMULATED with float atomics (caller zero-fills once per backward).
 * -------------------------------------------------------------------------------------- */
size_t ctd_geometric_workspace_bytes(int B, int H, int W);
int ctd_geometric_fwd_f32(const float* depth0, const float* depth1, const float* ray, const float* K,
                          const float* R0, const float* t0, const float* R1, const float* t1,
                          float* loss, int accumulate, int B, int H, int W, float clamp,
                          void* workspace, size_t workspace_bytes, int device, void* stream);
/* Additive: BOTH directions (the module's tforward, model/networks.py:500-503) in one launch, the two means formed by the
 * last workgroup to finish: loss[0] = mean(depth0 -> view 1) + mean(depth1 -> view 0), the same bits as the two
 * ctd_geometric_fwd_f32 calls (accumulate 0, then 1 with the views swapped).
 *   workspace: ctd_geometric_workspace_bytes(2 * B, H, W) bytes (contents irrelevant);
 *   ticket: 65 4-byte device words (260 bytes) owned by the caller, ZERO before the first call on them; every call
 *           leaves them zero.  Calls that may run concurrently (different streams) need tickets (and a workspace) each. */
int ctd_geometric_sym_fwd_f32(const float* depth0, const float* depth1, const float* ray, const float* K,
                              const float* R0, const float* t0, const float* R1, const float* t1,
                              float* loss, int B, int H, int W, float clamp, void* workspace,
                              size_t workspace_bytes, unsigned* ticket, int device, void* stream);
int ctd_geometric_bwd_f32(const float* depth0, const float* depth1, const float* ray, const float* K,
                          const float* R0, const float* t0, const float* R1, const float* t1,
                          const float* grad_loss, float* grad_depth0, int accumulate0,
                          float* grad_depth1, int B, int H, int W, float clamp, int device,
                          void* stream);

/* --------------------------------------------------------------------------------------
 * Fused pattern similarity loss (tolerance level, f32, block 9): RectifiedPatternSimilarityLoss.tforward,
 * model/networks.py:358-378 -- warp of the reference pattern by the predicted disparity
 * (grid_sample bilinear / border / align_corners=False on the grid of :362-369), block photometric
 * loss against the image (:376) and masked mean (:377) in one forward and one backward kernel.
 *   disp, im [B][1][H][W]; mask [B][1][H][W] or NULL (= ones); pattern [H][W] shared by the batch
 *   pattern_proj [B][1][H][W] (written); terms[3] (device) = { sum(mask*diff), sum(mask), their ratio }
 *   backward: grad_val (device scalar, d/d terms[2]), grad_proj [B][1][H][W] or NULL -> grad_disp
 * Workspace (forward only): ctd_pattern_loss_workspace_bytes().  The reduction is a fixed-order
 * tree: bitwise reproducible run to run.
 * -------------------------------------------------------------------------------------- */
size_t ctd_pattern_loss_workspace_bytes(int B, int H, int W);
int ctd_pattern_loss_fwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                             float* pattern_proj, float* terms, int B, int H, int W, int type,
                             float eps, void* workspace, size_t workspace_bytes, int device,
                             void* stream);
int ctd_pattern_loss_bwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                             const float* terms, const float* grad_val, const float* grad_proj,
                             float* grad_disp, int B, int H, int W, int type, float eps, int device,
                             void* stream);

/* Several pyramid levels (and any number of track frames stacked in B) in ONE forward and ONE backward launch
 * (the reference loops over the scales in Python, model/exp_synph.py:107-111,
 * model/exp_synphge.py:141-150).  Results per level are identical to the single-level calls.
 *   levels[l]: tensors of level l as in ctd_pattern_loss_fwd/bwd_f32 (mask, grad_proj may be NULL;
 *   pattern_proj is written by the forward, grad_disp by the backward); at most 8 levels.
 *   terms [n_levels][3], grad_vals [n_levels] (device). */
typedef struct ctd_pattern_level {
  const float *disp, *im, *mask, *pattern;
  float* pattern_proj;
  const float* grad_proj;
  float* grad_disp;
  int B, H, W;
} ctd_pattern_level;
size_t ctd_pattern_loss_multi_workspace_bytes(int n_levels, const ctd_pattern_level* levels);
int ctd_pattern_loss_multi_fwd_f32(int n_levels, const ctd_pattern_level* levels, float* terms, int type,
                                   float eps, void* workspace, size_t workspace_bytes, int device,
                                   void* stream);
int ctd_pattern_loss_multi_bwd_f32(int n_levels, const ctd_pattern_level* levels, const float* terms,
                                   const float* grad_vals, int type, float eps, int device,
                                   void* stream);

/* --------------------------------------------------------------------------------------
 * Nearest-neighbour consistency ops (integer results, bit-exact).
 * Replace nn_cuda / crosscheck_cuda / proj_nn_cuda -- torchext/ext/ext_cuda.cpp:17-68,
 * functors torchext/ext/ext.h:13-117, Python torchext/functions.py:5-56.
 *   ctd_nn:         in0 [n0][3], in1 [n1][3] -> out int64 [n0] = argmin_j |in0[i] - in1[j]|^2
 *                   (first index wins ties; -1 if no squared distance is below 1e9)
 *   ctd_crosscheck: in0 int64 [n0], in1 int64 [n1] -> out uint8 [n0] = 1 where
 *                   in1[in0[i]] == i (in0[i] truncated to int as in ext.h:61; an index
 *                   >= n1, which the reference reads out of bounds, gives 0)
 *   ctd_proj_nn:    xyz0, xyz1 [B][H][W][3], K [3][3] (device) -> out int64 [B][H][W] =
 *                   flat index of the closest xyz1 point in the patch_size^2 patch around
 *                   the projection of xyz0 (ext.h:86-114), -1 if the patch is empty
 * -------------------------------------------------------------------------------------- */
int ctd_nn_f32(const float* in0, const float* in1, long n0, long n1, int64_t* out, int device,
               void* stream);
int ctd_nn_f64(const double* in0, const double* in1, long n0, long n1, int64_t* out, int device,
               void* stream);
int ctd_crosscheck(const int64_t* in0, const int64_t* in1, long n0, long n1, uint8_t* out,
                   int device, void* stream);
int ctd_proj_nn_f32(const float* xyz0, const float* xyz1, const float* K, int B, int H, int W,
                    int patch_size, int64_t* out, int device, void* stream);
int ctd_proj_nn_f64(const double* xyz0, const double* xyz1, const double* K, int B, int H, int W,
                    int patch_size, int64_t* out, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Synthetic structured-light rendering (data side of the path).
 * Replaces RendererGpu<float>::render_mesh_proj -- renderer/render/render_gpu.h,
 * functor RenderProjectorFunctor renderer/render/render.h:251-364 (Python: PyRenderer.mesh_proj,
 * renderer/cyrender.pyx:196-199): brute-force ray casting of a triangle mesh from the camera,
 * shadow ray from the projector, bilinear fetch of the projected pattern with distance decay
 * max(1, (d_alpha + d_beta * d)^2), Phong-shaded vertex colours as the ambient image.
 *   verts, colors [n_verts][3] f32, faces [n_faces][3] int32, pattern [proj_height][proj_width][3]: device
 *   cam, proj = { fx, fy, px, py, R[9] row-major, t[3] } (16 floats), shader = { ka, kd, ks, alpha }: HOST
 *   depth [H][W] (-1 where nothing is hit; may be NULL), color [H][W][3], normal [H][W][3] (may be NULL;
 *   left untouched where nothing is hit, as in the reference): device
 * depth / color are bit-identical to the reference CPU build; normal too when ks == 0.
 * -------------------------------------------------------------------------------------- */
int ctd_render_mesh_proj_f32(const float* verts, const float* colors, int n_verts, const int* faces,
                             int n_faces, const float* cam, int cam_width, int cam_height,
                             const float* proj, int proj_width, int proj_height, const float* shader,
                             const float* pattern, float d_alpha, float d_beta, float* depth,
                             float* color, float* normal, int device, void* stream);

/* Replaces RendererGpu<float>::render_mesh -- functor RenderMeshFunctor renderer/render/render.h:150-223
 * (Python: PyRenderer.mesh, renderer/cyrender.pyx:193-194): camera rays only.
 *   normals [n_verts][3] f32: device (the reference interpolates the given vertex normals, unnormalised)
 *   depth [H][W] (-1 where nothing is hit), color [H][W][3] = clamp(phong * interpolated vertex colour, 0, 1),
 *   normal [H][W][3] = interpolated vertex normal flipped towards the camera; colour and normal are 0 where
 *   nothing is hit.  Each of the three outputs may be NULL (skipped), as the reference's Buffer allows.
 * Bit-identical to the reference CPU build (colour: when ks == 0, else up to powf's last bits). */
int ctd_render_mesh_f32(const float* verts, const float* colors, const float* normals, int n_verts,
                        const int* faces, int n_faces, const float* cam, int cam_width, int cam_height,
                        const float* shader, float* depth, float* color, float* normal, int device,
                        void* stream);

/* --------------------------------------------------------------------------------------
 * BVH ray casting (additive in ABI version 5): the same two renderers over a bounding volume hierarchy built
 * on the device once per mesh.  Outputs are bit-identical to ctd_render_mesh_proj_f32 / ctd_render_mesh_f32
 * (same hit face, t, u, v for every ray; the pruning bound is derived in csrc/render_bvh.hip).
 *   ctd_mesh_bvh_bytes(n) / ctd_mesh_bvh_workspace_bytes(n): sizes of the tree buffer and of the build's
 *   scratch (0 for n < 0 or n > 2^28).  Both device buffers must be 16-byte aligned.
 *   ctd_mesh_bvh_build_f32: verts [n_verts][3] f32, faces [n_faces][3] int32 (device; indices are NOT checked,
 *   they must lie in [0, n_verts)) -> bvh.  Deterministic: the buffer is a pure function of verts/faces, byte for
 *   byte.  Synchronises `stream` once to read the tree depth into *depth (may be NULL).  Returns
 *   CTD_ERR_UNSUPPORTED for a tree deeper than the traversal stack (62 levels; the buffer is then complete but
 *   refused by the renderers -- use the brute-force entries), CTD_ERR_WORKSPACE for a short workspace.
 *   n_faces == 0 is valid (an empty tree: every pixel is "nothing hit").
 *   ctd_render_mesh_proj_bvh_f32 / ctd_render_mesh_bvh_f32: the arguments of the brute-force entries plus the
 *   tree.  The tree must have been built from the same verts / faces pointers with the same contents; a stale
 *   tree gives undefined results.  Each call reads the tree's 64-byte header (a synchronous copy on `stream`)
 *   and returns CTD_ERR_INVALID_ARG if it is not a tree of n_faces faces, CTD_ERR_UNSUPPORTED if too deep.
 * -------------------------------------------------------------------------------------- */
size_t ctd_mesh_bvh_bytes(int n_faces);
size_t ctd_mesh_bvh_workspace_bytes(int n_faces);
int ctd_mesh_bvh_build_f32(const float* verts, int n_verts, const int* faces, int n_faces, void* bvh,
                           size_t bvh_bytes, void* workspace, size_t workspace_bytes, int* depth, int device,
                           void* stream);
int ctd_render_mesh_proj_bvh_f32(const void* bvh, const float* verts, const float* colors, int n_verts,
                                 const int* faces, int n_faces, const float* cam, int cam_width,
                                 int cam_height, const float* proj, int proj_width, int proj_height,
                                 const float* shader, const float* pattern, float d_alpha, float d_beta,
                                 float* depth, float* color, float* normal, int device, void* stream);
int ctd_render_mesh_bvh_f32(const void* bvh, const float* verts, const float* colors, const float* normals,
                            int n_verts, const int* faces, int n_faces, const float* cam, int cam_width,
                            int cam_height, const float* shader, float* depth, float* color, float* normal,
                            int device, void* stream);

/* --------------------------------------------------------------------------------------
 * Training-sample finishing of the synthetic data path (additive in ABI version 5).
 *
 * ctd_syn_finish_f32: data/create_syn_data.py:163-188 for N rendered frames of one size (the outputs of
 * ctd_render_mesh_proj_f32; `normal` holds the shaded ambient image and must be zero where nothing was hit).
 *   depth [N][H][W], color [N][H][W][3], normal [N][H][W][3], blend [N] (f64): device
 *   im, ambient, grad [N][H][W] written; disp, mask [N][H][W] written unless NULL
 * Operation order, all f32 without FMA (numpy 1.x value-based casting of the reference's f64 scalars):
 *   im_c = ((c0 + c1) + c2) / 3.0f;  ambient = ((n0 + n1) + n2) / 3.0f             (np.mean(axis=2))
 *   im   = (float)b * im_c + (float)(1.0 - b) * ambient                           (1 - b formed in double)
 *   disp = (float)baseline_focal / depth  (inf where depth == 0, negative where the renderer left -1);
 *   mask = depth > 0 ? 1 : 0
 *   gx, gy = cv2.Sobel(ambient, CV_32F, 1,0 | 0,1, ksize=5), unnormalised: gx = derivative taps [-1,-2,0,2,1] along x,
 *     smoothing taps [1,4,6,4,1] along y, gy the transpose; BORDER_REFLECT_101; separable, the row pass first, then
 *     the column pass, each output of a pass s = 0, s += k[j] * v[j] for j = 0..4 in f32
 *   pre  = fmaxf(sqrtf(gx*gx + gy*gy) - grad_threshold, 0)
 *   grad = lcn_datagen(pre, lcn_radius, lcn_eps), clipped to [0, 1] when lcn_clip != 0: BIT-IDENTICAL to
 *     ctd_lcn_datagen_f32 applied to `pre` (the same window code; the border of width lcn_radius is zero, all of the
 *     output when H or W <= 2 * lcn_radius)
 * Exact: every output is bit-identical to a numpy f32 evaluation in this order.  Assumed, not verified (cv2 is not
 * part of the test environment): that OpenCV's float Sobel equals this order -- its SIMD row / column filters may
 * group the symmetric taps differently, which moves |Sobel| by a few ulp; the bound against a float64 evaluation is
 * what tests/test_synth_gpu.py checks.  CTD_ERR_UNSUPPORTED when the LDS tile of lcn_radius exceeds 64 KiB.
 *
 * ctd_augment_f32: data/commons.py:46-107 `augment_image` with max_shift = 0, blur + noise + clip; salt and pepper is
 * the separate ctd_salt_pepper_f32 after it.  One parameter row per image, on the device:
 *   blur != 0: 5x5 Gaussian blur, cv2.GaussianBlur(img, (5,5), sigma) on f32 with taps k[j] = (float)(e_j / sum(e)),
 *     e_j = exp(-(j-2)^2 / (2 sigma^2)) (formed in double by the caller); BORDER_REFLECT_101; row pass then column
 *     pass, s = 0, s += k[j] * v[j] in f32.  blur == 0: the image passes through untouched.
 *   v = (double)blurred + (double)noise * noise_scale, clipped to [0, 1] in double, rounded to f32 once.  noise is
 *     [N][H][W] f32 (noise_f64 = 0) or f64 (noise_f64 = 1: the reference's f64 noise term itself, bit for bit), or
 *     NULL (no noise).
 *   minmax [N][2] (u32, device): the min and max of the INPUT image as ordered keys, key(x) = bits(x) ^ (x < 0 ?
 *     0xffffffff : 0x80000000); word 0 holds ~key(min), word 1 key(max).  The call zeroes them on `stream` first.
 * Exact: bit-identical to a numpy evaluation in this order; with blur == 0 bit-identical to augment_image itself.
 * Assumed, not verified: OpenCV builds the f32 Gaussian taps as e_j * (1 / sum(e)) in double (not e_j / sum(e)),
 * which can differ in the last bit of the double and, rarely, of the f32 tap; and it may group the symmetric taps
 * of its SIMD filters differently (a few ulp).  Against a float64 blur with exact taps the stated order is within its
 * forward-error bound 14 * 2^-24 * blur(|x|) (tests/test_synth_gpu.py); 2 ulp of the result is NOT a bound of it.
 *
 * ctd_salt_pepper_f32: commons.py:96-101 on the output of ctd_augment_f32.  Per image n, counts[n] (clamped to
 * [0, kmax]) indices into the flattened image from salt[n][0..] and pepper[n][0..] (int64 [N][kmax], drawn with
 * replacement): writes clip(max) at the salt indices, then clip(min) at the pepper indices (pepper wins a shared
 * index), min / max decoded from `minmax`.  Indices outside [0, H*W) are skipped.  No workspace.
 * -------------------------------------------------------------------------------------- */
typedef struct ctd_augment_params {
  int32_t blur;                  /* 1: blur with taps[], 0: no blur                     */
  float taps[5];                 /* Gaussian taps, f32                                   */
  double noise_scale;            /* multiplies the noise plane, in double               */
} ctd_augment_params;            /* 32 bytes, one per image                              */
int ctd_syn_finish_f32(const float* depth, const float* color, const float* normal, const double* blend,
                       double baseline_focal, float grad_threshold, int lcn_radius, float lcn_eps, int lcn_clip,
                       float* im, float* ambient, float* grad, float* disp, float* mask, int N, int H, int W,
                       int device, void* stream);
int ctd_augment_f32(const float* img, const void* noise, int noise_f64, const ctd_augment_params* params, float* out,
                    uint32_t* minmax, int N, int H, int W, int device, void* stream);
int ctd_salt_pepper_f32(float* img, const uint32_t* minmax, const int32_t* counts, const int64_t* salt,
                        const int64_t* pepper, int kmax, int N, int H, int W, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * HyperDepth random-forest disparity evaluation (additive in ABI version 5).
 * Replaces hyperdepth.pyx `eval_forest` -> hyperdepth.h:253-287 `eval` (rf/forest.h inferencemt + the leaf
 * reduction HyperdepthLeafFunction::Reduce / argmax / prob_vec, hyperdepth.h:82-131), bit for bit.
 *
 * Per pixel (n, row, col) of ims [N][H][W] (u8), row in [row_from, row_to), with the forest of `row`:
 *   split test: v(h, w) = (float)ims[n][clamp(row + h - 16, 0, H-1)][clamp(col + w - 16, 0, W-1)]; the walk goes to
 *     `left` iff v(h0, w0) - v(h1, w1) < threshold (f32; a NaN threshold always goes right);
 *   S[c] = sum over the trees of the reached leaves' counts[c], c < C = n_classes;
 *   pos  = first index of the maximum of S;  pos2 = first index of the maximum of S without pos
 *     (with < 2 non-zero classes: none -> pos = 0, pos2 = 1; one -> pos2 = pos == 0 ? 1 : 0);
 *   out[n][row][col][0] = (float)col - (float)pos / (float)n_disp_bins
 *   out[n][row][col][1] = (float)S[pos] / (float)sum(S)          (NaN when every count is 0)
 *   out[n][row][col][2] = |out[..][0] - ((float)col - (float)pos2 / (float)n_disp_bins)|
 * IEEE f32 division, no contraction.  Rows outside [row_from, row_to) are written NaN.
 *
 * Device tables (every pointer in device memory; the struct itself is host memory, read during the call only):
 *   nodes    [n_nodes][8] int32   split nodes: { threshold (f32 bits), h0, w0, h1, w1, left, right, 0 }
 *                                 (the file's c0 / c1 are not stored: the reference's samples have one channel)
 *   roots    [n_rows][n_trees]    root of tree t of image row row0 + r
 *            a child / root value v >= 0 is node v, v < 0 is leaf ~v (= -v - 1)
 *   leaf_off [n_leaves + 1] int64 CSR offsets of the leaves' lists into entries (non-decreasing, leaf_off[0] = 0)
 *   leaf_sum [n_leaves] int32     sum of the leaf's counts
 *   entries  [n_entries][2] int32 (class, count), classes strictly increasing within a leaf, 0 <= class < n_classes,
 *                                 count >= 0; zero counts may be left out (the loader stores non-zero ones only)
 *   max_depth                     the longest root-to-leaf path, in split nodes
 * The caller guarantees counts >= 0 and that the per-pixel sum of leaf_sum over the trees fits an int32
 * (connecting_the_dots_amd/hyperdepth.py checks both at load).  Table contents are not validated here, but
 * malformed tables cannot make the kernel access memory out of bounds or loop forever: a walk longer than max_depth,
 * a node / leaf index out of range or a leaf list outside entries makes that pixel NaN, and classes outside
 * [0, n_classes) are skipped.
 *
 * Errors, before any HIP call: CTD_ERR_INVALID_ARG for a NULL pointer (nodes / entries may be NULL when their counts
 * are 0), N < 0, H or W < 1 or >= 2^24, rows outside 0 <= row_from <= row_to <= H, a non-empty row range outside
 * [row0, row0 + n_rows), n_trees outside [1, 16], n_classes < 2, n_disp_bins < 1, negative table sizes or max_depth;
 * CTD_ERR_UNSUPPORTED when 4 * n_classes + 1024 * n_trees > 65536 (the per-workgroup LDS histogram) or the grid
 * exceeds the launch limits.  No workspace.
 * -------------------------------------------------------------------------------------- */
typedef struct ctd_hd_tables {
  const int32_t* nodes;
  const int32_t* roots;
  const int64_t* leaf_off;
  const int32_t* leaf_sum;
  const int32_t* entries;
  int64_t n_nodes, n_leaves, n_entries;
  int32_t row0, n_rows, n_trees, n_classes, max_depth, reserved;
} ctd_hd_tables;                 /* 88 bytes */
int ctd_hyperdepth_eval_f32(const ctd_hd_tables* tables, const uint8_t* ims, int N, int H, int W, int row_from,
                            int row_to, int n_disp_bins, float* out, int device, void* stream);

/* --------------------------------------------------------------------------------------
 * HyperDepth random-forest training (additive in ABI version 5).
 * The reference's trainer (hyperdepth.pyx `train_forest` -> hyperdepth.h `train`: extract_row_samples,
 * rf/train.h TrainForestQueued / OptimizeSplitFunction / SampleData / Split, HyperdepthSplitEvaluator,
 * HyperdepthLeafFunction::Create) with its std::random_device / std::mt19937 draws replaced by the counter-based
 * generator below: the output is an exact function of the inputs and the seed.  It departs from the reference only
 * where the reference is non-deterministic or would round differently on another machine (the cost, see below).
 *
 * Samples of row r: the pairs (n, col), n-major then col, for which d = disps[n][r][col] gives
 *   cl = (int)trunc((float)((float)col - d) * (float)n_disp_bins)      (f32, no contraction)
 * with d >= 0 and 0 <= cl < W * n_disp_bins (a NaN d is excluded, as the reference's cvttss2si does on x86; a product
 * in (-1, 0) gives cl = 0; the upper bound cannot fail for W * n_disp_bins < 2^24 -- the reference would index past
 * its counts otherwise).
 * Trees: n_trees per row, each starts from all of the row's samples.  Nodes: heap ids (root 1, children 2i, 2i + 1),
 * the root at depth 0.  A node of n samples tries to split iff depth < max_tree_depth and n > min_samples_to_split,
 * otherwise it is a leaf.
 * Randomness, uint64 wrapping arithmetic:
 *   mix64(x): x ^= x >> 30; x *= 0xbf58476d1ce4e5b9; x ^= x >> 27; x *= 0x94d049bb133111eb; x ^= x >> 31
 *   base = mix64(mix64(mix64(mix64(seed) ^ row) ^ tree) ^ node)     (row = absolute image row, node = heap id)
 *   draw(slot, m) = ((mix64(base ^ slot) >> 32) * m) >> 32           in [0, m)
 * Split subset, k' = min(n_test_samples, n): all n samples if n <= n_test_samples, else Floyd: for i in [0, k'):
 *   j = n - k' + i, t = draw(i, j + 1); choose j if t is chosen already, else t.  Chosen positions in increasing
 *   order (the reference's std::set).
 * Candidates: for f in [0, F): h0, w0, h1, w1 = draw(2^40 + 8f + e, 32), e = 0..3 (c0 = c1 = 0: one channel); for j
 *   in [0, J): threshold = feature of subset element draw(2^41 + f * 2^16 + j, k'); feature = v(h0, w0) - v(h1, w1)
 *   in f32 with v as in the eval block below (clamped 32 x 32 patch, centre at +16).  Left iff feature < threshold.
 * Cost on the subset: valid iff both sides hold >= min_samples_for_leaf samples; class = cl / n_disp_bins at
 *   depth < depth_switch, cl otherwise; with the caller's table X[x] = int64(rint(x * log(x) * 2^32)), X[0] = X[1] = 0,
 *   cost = X[nL] + X[nR] - sum_c X[cL(c)] - sum_c X[cR(c)]  (int64: n * 2^32 * the reference's normalised weighted
 *   entropy, exact and independent of summation order).  The best is the valid candidate with the smallest
 *   (cost, f, j) (the reference's strict <: the first wins ties); none valid -> leaf.  Otherwise all n samples are
 *   partitioned, order preserved, into left (feature < threshold) and right.
 * Leaf: dense counts of the fine cl over its samples, n_counts = W * n_disp_bins, sum_counts = n, header n_classes_
 *   = -1 (Create builds it with the default constructor).  A row without samples gives n_trees single-leaf trees
 *   with all-zero counts.
 *
 * Output: the ctd_hd_tables layout of the eval block (nodes, roots [n_rows][n_trees], leaf_off, leaf_sum, entries with
 * the non-zero counts only, class-sorted), indices assigned level by level in a deterministic order, so that the
 * tables can be evaluated without leaving the device.  used[5] (device int64) receives n_nodes, n_leaves, n_entries,
 * max_depth and an error flag (non-zero: a capacity below the bounds below was passed, or the counts the workspace
 * was sized for are smaller than the device's own; the tables are then incomplete).  Bounds per tree of a row with
 * n_r samples (D = max_tree_depth): split nodes <= min(2^D - 1, max(n_r - 1, 0)), leaves <= splits + 1, entries
 * <= n_r; leaf_off needs cap_leaves + 1 entries.
 * ctd_hyperdepth_train_count_f32 writes the per-row sample counts (device int64 [row_to - row_from]); the workspace
 * query and the training call take the same counts in HOST memory (row_counts), copied by the caller.
 * X is a device int64 table of n_x >= n_test_samples + 1 entries.  The callee never allocates.
 *
 * Errors, before any HIP call: CTD_ERR_INVALID_ARG for NULL pointers, N < 1, H or W < 1 or >= 2^24,
 * N * H * W >= 2^31, rows outside 0 <= row_from < row_to <= H, n_disp_bins < 1, W * n_disp_bins >= 2^31,
 * n_trees outside [1, 16], max_tree_depth outside [0, 24], n_test_split_functions outside [0, 2^20),
 * n_test_thresholds outside [0, 2^16), n_test_samples outside [1, 8192], min_samples_to_split < 0,
 * min_samples_for_leaf < 1, negative row counts, n_x < n_test_samples + 1, negative capacities;
 * CTD_ERR_WORKSPACE for a short workspace.
 * -------------------------------------------------------------------------------------- */
typedef struct ctd_hd_train_params {
  int32_t n_trees, max_tree_depth, n_test_split_functions, n_test_thresholds, n_test_samples;
  int32_t min_samples_to_split, min_samples_for_leaf, depth_switch, n_disp_bins, reserved;
  uint64_t seed;
} ctd_hd_train_params;           /* 48 bytes */
typedef struct ctd_hd_train_out {
  int32_t* nodes;                /* [cap_nodes][8]     */
  int32_t* roots;                /* [n_rows][n_trees]  */
  int64_t* leaf_off;             /* [cap_leaves + 1]   */
  int32_t* leaf_sum;             /* [cap_leaves]       */
  int32_t* entries;              /* [cap_entries][2]   */
  int64_t* used;                 /* [5]                */
  int64_t cap_nodes, cap_leaves, cap_entries;
} ctd_hd_train_out;              /* 72 bytes */
int ctd_hyperdepth_train_count_f32(const float* disps, int N, int H, int W, int row_from, int row_to,
                                   int n_disp_bins, int64_t* counts, int device, void* stream);
size_t ctd_hyperdepth_train_workspace_bytes(const ctd_hd_train_params* params, int n_rows, const int64_t* row_counts,
                                            int64_t cap_leaves);
int ctd_hyperdepth_train_f32(const ctd_hd_train_params* params, const int64_t* X, int n_x, const uint8_t* ims,
                             const float* disps, int N, int H, int W, int row_from, int row_to,
                             const int64_t* row_counts, void* workspace, size_t workspace_bytes,
                             const ctd_hd_train_out* out, int device, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CTD_HIP_H */
