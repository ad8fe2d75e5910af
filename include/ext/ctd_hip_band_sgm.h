/* ctd_hip_band_sgm.h -- band-limited semi-global matching of libctd_hip.so: the band matchers' scores written as a
 * band volume of `slots` planes, and semi-global aggregation within every pixel's own disparity range [lo, hi].
 *
 * An addition beside include/ctd_hip.h and include/ctd_hip_band.h (neither includes it; ctd_version() is unchanged).
 * The status codes and CTD_PATTERN_PREPARED are those of ctd_hip.h; pointers are device pointers, `device` and
 * `stream` mean what they mean there.
 *
 * The band.  lo and hi are int32 [frames][H][W], inclusive; every op takes a slot count `slots`, 1 <= slots <= 64.
 *
 * - lo' = max(lo, 0).
 * - hi'' = min(hi, D - 1, lo' + slots - 1).
 * - Pixel p *holds* d when lo' <= d <= hi''.  Its slot is k = d - lo'.  n(p) is the number it holds (0: empty band).
 * - A band wider than `slots` is truncated to its first `slots` disparities: the library cannot look at device data
 *   before it launches, so truncation is the rule and not an error.
 *
 * The band volume.  Let V[f][d][h][w] be the reference-order volume of include/ctd_hip_band.h (NCC:
 * ctd_xcorrvol_f32(CTD_NCC_EXACT), C == 1, higher is better; costs: ctd_costvol_f32, lower is better).  Inputs are
 * assumed finite.  ctd_xcorrvol_band_volume_f32 and ctd_costvol_band_volume_f32 write Vb [frames][slots][H][W] (f32):
 *
 * - Vb[f][k][h][w] is V[f][lo'+k][h][w] bit for bit for k < n(p).
 * - It is NaN in every other slot.
 * - Nothing of size frames * D * H * W is read or written.
 *
 * The NCC call takes the arguments and the workspace of ctd_xcorrvol_argmax_band_f32 (the query
 * ctd_xcorrvol_argmax_band_workspace_bytes, 256-byte aligned, CTD_PATTERN_PREPARED included), the cost call those of
 * ctd_costvol_argmin_band_f32; `vol_b` stands where idx and best stand there.
 *
 * Aggregation.  ctd_band_sgm_aggregate_f32 runs the rule of ctd_sgm_aggregate_f32 over a band volume.  C = Vb when
 * `maximise` is 0 (costs), or -Vb when it is 1 (scores).  Along a direction (dy, dx), with q = (y - dy, x - dx):
 *
 * - q outside the image, or n(q) = 0: L(p, d) = C(p, d) for every d that p holds.
 * - Otherwise:
 *   - m = min L(q, k) over the k that q holds.
 *   - t = min(L(q, d) [q holds d], m + p2, L(q, d-1) + p1 [q holds d-1], L(q, d+1) + p1 [q holds d+1]).
 *   - L(p, d) = C(p, d) + (t - m).
 * - The association order, the directions (right, left, down, up for paths == 4; right, left, down, down-right,
 *   down-left, up, up-right, up-left for paths == 8) and the summation order S = ((L0 + L1) + L2) ... are those of
 *   ctd_sgm_aggregate_f32.
 * - idx[f][h][w] (int64) = lo' + the first argmin slot of S.  best (f32) = S at it.  An empty band gives idx = -1 and
 *   best = NaN.
 * - S_b [frames][slots][H][W] (f32, may be NULL) is S by slot.  Its unheld slots are NaN.
 * - S and best are in cost sign (lower is better), also with maximise == 1.
 * - Only f32 add, sub and min occur, and there are no atomics.  Every run returns the same bits.
 *
 * Why this rule.  Where every pixel holds at least one disparity, it is exactly ctd_sgm_aggregate_f32 on the full
 * [frames][D][H][W] volume with +inf outside each pixel's band: an unheld neighbour term is +inf there and drops out
 * of every min, and m, the minimum over all D, is the minimum over what q holds.  tests/test_band_sgm_host.py holds
 * the two against each other bit for bit.  The restart at an empty predecessor is the one place where the masked full
 * volume would produce inf - inf (every L(q, .) is +inf, so m is); the band rule starts the path again there, as it
 * does at the image border.
 *
 * Workspace of the aggregation: ctd_band_sgm_workspace_bytes() bytes, 16-byte aligned; it holds S when S_b is NULL and
 * is not needed (may be NULL) when S_b is given.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for slots < 1, paths not 4 or 8, p1 < 0, p1 > p2, a non-finite penalty, and for what
 *     ctd_hip_band.h rejects with this code (an even or < 1 block size, a type outside 0..3, flags other than 0 /
 *     CTD_PATTERN_PREPARED, a stride other than 0 / H * W, D, H or W < 1, frames < 0, D * H * W >= 2^31); then,
 *     unless frames == 0, for a NULL in0 / in1 / im / pattern / lo / hi / vol_b / idx / best;
 *   CTD_ERR_UNSUPPORTED for slots > 64, frames * H * W >= 2^31 or frames * slots * H * W >= 2^31;
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * frames == 0 is CTD_OK and touches nothing.  ctd_band_sgm_workspace_bytes returns 0 for invalid or unsupported
 * arguments, for frames == 0 and when want_volume != 0.
 */
#ifndef CTD_HIP_BAND_SGM_H
#define CTD_HIP_BAND_SGM_H

#include "../ctd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* in0 [frames][H][W], in1 [H][W] (in1_frame_stride 0) or [frames][H][W] (in1_frame_stride H * W);
 * vol_b [frames][slots][H][W] */
int ctd_xcorrvol_band_volume_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                 const int32_t* hi, float* vol_b, int frames, int slots, int H, int W, int D,
                                 int block_size, int flags, void* workspace, size_t workspace_bytes, int device,
                                 void* stream);

/* im [frames][H][W], pattern [H][W] (pattern_frame_stride 0) or [frames][H][W] (pattern_frame_stride H * W);
 * type 0 mse, 1 sad, 2 census_mse, 3 census_sad (eps: the soft step of the census types), as ctd_costvol_f32 */
int ctd_costvol_band_volume_f32(const float* im, const float* pattern, long pattern_frame_stride, const int32_t* lo,
                                const int32_t* hi, float* vol_b, int frames, int slots, int H, int W, int D,
                                int block_size, int type, float eps, int device, void* stream);

size_t ctd_band_sgm_workspace_bytes(int frames, int slots, int H, int W, int D, int paths, int want_volume);

/* vol_b [frames][slots][H][W] (never written); S_b as vol_b or NULL; idx, best [frames][H][W] */
int ctd_band_sgm_aggregate_f32(const float* vol_b, const int32_t* lo, const int32_t* hi, int maximise, float p1,
                               float p2, int paths, float* S_b, int64_t* idx, float* best, int frames, int slots,
                               int H, int W, int D, void* workspace, size_t workspace_bytes, int device,
                               void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_BAND_SGM_H */
