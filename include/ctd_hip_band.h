/* ctd_hip_band.h -- band-limited matching of libctd_hip.so: the best NCC score / block cost of every pixel within a
 * per-pixel disparity range [lo, hi], without a volume.
 *
 * An addition beside include/ctd_hip.h (which does not include it; ctd_version() is unchanged): include both.  The
 * status codes, CTD_NCC_EXACT and CTD_PATTERN_PREPARED are those of ctd_hip.h; pointers are device pointers, `device`
 * and `stream` mean what they mean there.
 *
 * Definition.  Let V[f][d][h][w] be the reference-order volume:
 *
 * - NCC: the volume of ctd_xcorrvol_f32(CTD_NCC_EXACT); C == 1; higher is better.
 * - Costs: the volume of ctd_costvol_f32 with the same arguments; lower is better.
 *
 * Inputs are assumed finite.
 *
 * lo and hi are int32 [frames][H][W], inclusive.  The kernel clips them to [0, D-1]: lo' = max(lo, 0),
 * hi' = min(hi, D-1).
 *
 * - idx[f][h][w] (int64) is the first index of the best V[f][d][h][w] over d in [lo', hi'].  It is -1 when lo' > hi'.
 * - best[f][h][w] (f32, may be NULL) is V[f][idx][h][w] bit for bit.  It is NaN where idx == -1.
 * - Nothing of size frames * D * H * W is read or written.
 * - Any band width up to D is legal.  A band of [0, D-1] everywhere returns the indices of torch.argmax / argmin of V.
 *
 * The same bits come out on every run: each score is computed by one thread in the reference's tap order and ranked in
 * ascending d with a strict compare; there are no atomics.
 *
 * NCC workspace: ctd_xcorrvol_argmax_band_workspace_bytes() bytes, 256-byte aligned, laid out exactly as the workspace
 * of ctd_xcorrvol_subpixel_f32 (the query returns the same number), so one workspace serves both calls.  `flags` may
 * carry CTD_PATTERN_PREPARED with the meaning it has there: the pattern planes of the workspace were filled by an
 * earlier call of either op with the same in1, H, W, D, block_size and pattern stride, and are not recomputed.  A call
 * without the flag fills them.  The cost call needs no workspace.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for an even or < 1 block size, a type outside 0..3, flags other than 0 / CTD_PATTERN_PREPARED,
 *     a stride other than 0 / H * W, D, H or W < 1, frames < 0, D * H * W >= 2^31, or a NULL in0 / in1 / im / pattern /
 *     lo / hi / idx;
 *   CTD_ERR_UNSUPPORTED for frames * H * W >= 2^31 (the grid is one-dimensional in tiles of pixels, so no smaller
 *     shape passes a launch limit);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * frames == 0 is CTD_OK and touches nothing.  The workspace query returns 0 for invalid shapes and for frames == 0.
 */
#ifndef CTD_HIP_BAND_H
#define CTD_HIP_BAND_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_xcorrvol_argmax_band_workspace_bytes(int frames, int H, int W, int D, int block_size,
                                                int per_frame_pattern);

/* in0 [frames][H][W], in1 [H][W] (in1_frame_stride 0) or [frames][H][W] (in1_frame_stride H * W) */
int ctd_xcorrvol_argmax_band_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                 const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D,
                                 int block_size, int flags, void* workspace, size_t workspace_bytes, int device,
                                 void* stream);

/* im [frames][H][W], pattern [H][W] (pattern_frame_stride 0) or [frames][H][W] (pattern_frame_stride H * W);
 * type 0 mse, 1 sad, 2 census_mse, 3 census_sad (eps: the soft step of the census types), as ctd_costvol_f32 */
int ctd_costvol_argmin_band_f32(const float* im, const float* pattern, long pattern_frame_stride, const int32_t* lo,
                                const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D,
                                int block_size, int type, float eps, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_BAND_H */
