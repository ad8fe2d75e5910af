/* ctd_hip_band_validity.h -- match validity of the band matchers of libctd_hip.so: the band match of every pixel
 * together with its left-right check and its uniqueness gap *within the band*, without a volume.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h and ctd_hip_warp.h (none of which includes it; ctd_version() is
 * unchanged): include ctd_hip.h and ctd_hip_band.h with it.  The status codes, CTD_NCC_EXACT, CTD_PATTERN_PREPARED and
 * the CTD_VALID_* bits are those of ctd_hip.h; pointers are device pointers, `device` and `stream` mean what they mean
 * there.
 *
 * Definition.  V[f][d][h][w] is the reference-order volume, as in include/ctd_hip_band.h:
 *
 * - NCC: ctd_xcorrvol_f32(CTD_NCC_EXACT), C == 1, higher is better.
 * - Costs: ctd_costvol_f32, lower is better.
 *
 * Inputs are finite.  lo' and hi' are the clipped band of ctd_hip_band.h.  Pixel (f,h,w) *holds* disparity d when
 * lo' <= d <= hi'.  "Best" and "better" follow the family.
 *
 * - idx, best: exactly those of ctd_xcorrvol_argmax_band_f32 / ctd_costvol_argmin_band_f32 (-1 / NaN on an empty
 *   band).
 * - idx_r[f][h][x] (int64): the first index of the best V[f][d][h][x+d] over those d in [0, min(D, W-x)) that pixel x+d
 *   holds.  It is -1 when no pixel holds a disparity that lands on column x.  Ties go to the smaller d, by a
 *   floating-point compare, so -0.0 and +0.0 tie.
 * - gap[f][h][w] (f32): with d0 = idx and s1 = V[d0], s2 is the best V[d] over held d with |d - d0| >= 2.
 *   - NCC: s1 - s2.  Costs: s2 - s1.  One f32 subtraction.
 *   - +inf when no such d is held.  NaN when idx == -1.
 *   - A band of width <= 3 around idx always passes UNIQUE.
 * - flags (uint8), bits as CTD_VALID_* of ctd_hip.h:
 *   - IN_PATTERN: idx >= 0 and w - idx >= 0.
 *   - LR_OK: IN_PATTERN and |idx_r[f][h][w-idx] - idx| <= lr_tol.  That idx_r is never -1, because the pixel's own
 *     candidate landed there.
 *   - UNIQUE: idx >= 0 and gap > min_gap.
 * - With lo = 0, hi = D-1 everywhere, flags, idx_r and gap equal those of ctd_match_validity_f32 on V with the band
 *   matcher's idx.
 * - The same bits come out on every run.
 *
 * Unlike ctd_xcorrvol_validity_f32 / ctd_costvol_validity_f32 on a band matcher's idx, the pattern side sees only what
 * the bands hold: a periodic wrong match that no pixel's band admits cannot win a column.  Nothing of size
 * frames * D * H * W is read or written.
 *
 * How.  Every candidate (w, d) of a band is scored once, by one thread, in the reference's tap order.  The pixel side
 * (idx, best, gap) is a running state of that thread's ascending sweep.  The pattern side is a 64-bit atomic maximum on
 * column x = w - d of a key whose high word is the score mapped order-preservingly to an unsigned integer (costs
 * negated; -0.0 folded to +0.0) and whose low word is 0xFFFFFFFF - d: a maximum does not depend on the order of its
 * operands, so the bits do not depend on the order in which workgroups arrive.
 *
 * Workspace.  The NCC call takes the workspace of ctd_xcorrvol_argmax_band_f32 / ctd_xcorrvol_subpixel_f32 unchanged:
 * ctd_xcorrvol_argmax_band_workspace_bytes() bytes, 256-byte aligned; `flags_prepared` is 0 or CTD_PATTERN_PREPARED
 * with the meaning it has there (the pattern planes were filled by an earlier call of any of the three ops with the
 * same in1, H, W, D, block_size and pattern stride).  The cost call needs none.  There is no other workspace: idx_r
 * (8 bytes per column) holds the keys during the call and is decoded in place by the call's last kernel.  If a call
 * fails, the contents of idx_r (and of the other outputs) are unspecified.
 *
 * `best` may be NULL.  Every other pointer is required.
 *
 * Errors, before any HIP call, in this order:
 *   those of the band calls, in their order: CTD_ERR_INVALID_ARG for an even or < 1 block size, a type outside 0..3,
 *     flags_prepared other than 0 / CTD_PATTERN_PREPARED, a stride other than 0 / H * W, D, H or W < 1, frames < 0 or
 *     D * H * W >= 2^31; then frames == 0 is CTD_OK and touches nothing (lr_tol and min_gap are not looked at); then
 *     CTD_ERR_INVALID_ARG for a NULL in0 / in1 / im / pattern / lo / hi / idx / flags / idx_r / gap;
 *   CTD_ERR_INVALID_ARG for lr_tol < 0 or a negative or NaN min_gap;
 *   CTD_ERR_UNSUPPORTED for frames * H * W >= 2^31;
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace (NCC).
 */
#ifndef CTD_HIP_BAND_VALIDITY_H
#define CTD_HIP_BAND_VALIDITY_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* in0 [frames][H][W], in1 [H][W] (in1_frame_stride 0) or [frames][H][W] (in1_frame_stride H * W); lo, hi int32, idx and
 * idx_r int64, best and gap f32, flags uint8, each [frames][H][W] */
int ctd_xcorrvol_band_validity_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                   const int32_t* hi, int64_t* idx, float* best, uint8_t* flags, int64_t* idx_r,
                                   float* gap, int frames, int H, int W, int D, int block_size, int lr_tol, float min_gap,
                                   int flags_prepared, void* workspace, size_t workspace_bytes, int device, void* stream);

/* im [frames][H][W], pattern [H][W] (pattern_frame_stride 0) or [frames][H][W] (pattern_frame_stride H * W);
 * type 0 mse, 1 sad, 2 census_mse, 3 census_sad (eps: the soft step of the census types), as ctd_costvol_f32 */
int ctd_costvol_band_validity_f32(const float* im, const float* pattern, long pattern_frame_stride, const int32_t* lo,
                                  const int32_t* hi, int64_t* idx, float* best, uint8_t* flags, int64_t* idx_r,
                                  float* gap, int frames, int H, int W, int D, int block_size, int type, float eps,
                                  int lr_tol, float min_gap, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_BAND_VALIDITY_H */
