/* ctd_hip_warp.h -- forward depth warping of libctd_hip.so: what every view of a track should look like given the
 * track's other views (a z-buffered forward warp), and the disparity search range of the band matchers
 * (ctd_hip_band.h) around a prior that has holes and occlusion edges.
 *
 * An addition beside include/ctd_hip.h and include/ctd_hip_band.h (neither includes it; ctd_version() is unchanged):
 * include what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device` and `stream`
 * mean what they mean there.  No buffer a call writes may overlap another buffer of the call.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_depth_warp_f32
 *
 * depth f32 [B][V][H][W], valid u8 [B][V][H][W] or NULL, ray [H*W][3], K [3][3], R [B][V][3][3], t [B][V][3] are the
 * inputs of ctd_depth_consistency_f32 (X_cam = R X_world + t).  sources and targets are u8 [B][V] or NULL (NULL: all
 * ones).  splat is 0, 1 or 2.  Outputs, each [B][V][H][W]: z f32 and src int64 (src may be NULL).
 *
 * Definition.  A source pixel q of view s is live under the rule of ctd_hip.h: valid is nonzero, and depth is finite
 * and > 0.
 *
 * For a target view r with targets[b][r] != 0, take every view s != r with sources[b][s] != 0 and every live pixel
 * q = (yq, xq) of it.  Each such pixel is treated as follows.
 *
 * - uvd = transform(depth, ray[q], R_s, t_s, R_r, t_r, K).  These are the products and sums of "the transform from
 *   view a to view b" of ctd_hip.h (P, Q, S, uvd, with a = s and b = r), in that association and uncontracted.
 * - The pixel is dropped unless uvd[2] > 0 and uvd[2] < inf.
 * - xs = floor(uvd[0] / uvd[2] + 0.5f) and ys = floor(uvd[1] / uvd[2] + 0.5f).  These are f32 operations.
 * - The pixel is dropped unless -splat <= xs <= W-1+splat and -splat <= ys <= H-1+splat.  The compares are in f32
 *   before any conversion, so a NaN fails them.
 * - The pixel is a candidate for every (y, x) = (ys+dy, xs+dx) with |dy|, |dx| <= splat that lies inside the image.
 *
 * At a target pixel the winner is the candidate with the smallest (z, s*H*W + q), q = yq*W + xq.  Order is first by
 * z = uvd[2], and a tie goes to the smaller in-track source index.  The outputs at a target pixel:
 *
 * - z is the winner's uvd[2] bit for bit.
 * - src = ((b*V + s)*H + yq)*W + xq, which is the flat-index convention of ctd_depth_fuse_points_f32.
 * - A pixel with no candidate gets z = NaN and src = -1.
 * - Every pixel of a view with targets == 0 gets z = NaN and src = -1.
 * - V == 1 gives all holes.
 *
 * The nearest surface wins: a gross foreground outlier in a source view wins too, so warp from depths that the other
 * views confirm (valid = keep of ctd_depth_consistency_f32).
 *
 * The same bits come out on every run.  Each candidate is one 64-bit unsigned atomic minimum on the key
 * (bits(z) << 32) | (s*H*W + q) of its target pixel.  Positive finite f32 bit patterns order as unsigned integers, so
 * the smallest key is the winner of the definition, and a minimum does not depend on the order of its operands.
 *
 * Workspace: ctd_depth_warp_workspace_bytes(B, V, H, W) bytes, 256-byte aligned: one 8-byte key per output pixel.  The
 * call never allocates; it sets every key itself, so the workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for a splat outside 0..2, V, H or W < 1, B < 0, V > 64, or a NULL depth / ray / K / R / t / z;
 *   CTD_ERR_UNSUPPORTED for V * H * W >= 2^32 (the key holds the index in 32 bits), B * V * H * W >= 2^31, or
 *     B * V * ceil(H * W / 256) >= 2^24 (one workgroup per 256 pixels of a view; a launch stays below 2^32 threads);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing, the workspace included.  The workspace query
 * returns 0 for shapes that one of the first two errors rejects and for B == 0.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_disparity_band_window_f32
 *
 * prior f32 [N][H][W], radius a float, D the number of disparities, window odd in 1..15 with k = window / 2, holes 0
 * (empty) or 1 (full).  Outputs lo and hi, int32 [N][H][W]: the inclusive range the band matchers take.
 *
 * Definition.  Over the (2k+1)^2 window around a pixel, clipped to the image:
 *
 * - m is the minimum of the finite priors.
 * - M is the maximum of the finite priors.
 *
 * If there is at least one finite prior:
 *
 * - lo = clamp(ceil(m - radius), 0, D).
 * - hi = clamp(floor(M + radius), -1, D-1).
 * - Each uses one f32 subtraction or addition before the rounding.
 *
 * If there is none:
 *
 * - holes == 0 gives lo = D, hi = -1.
 * - holes == 1 gives lo = 0, hi = D-1.
 *
 * A radius that is negative or NaN gives the empty band lo = D, hi = -1 everywhere, whatever `holes` is.  With
 * window == 1 and holes == 0 the result is the per-pixel band of torchext.disparity_band bit for bit.
 *
 * The same bits come out on every run: minimum and maximum are exact, and there are no atomics.  No workspace.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for an even window, a window outside 1..15, holes outside {0, 1}, D, H or W < 1, N < 0, or a
 *     NULL prior / lo / hi;
 *   CTD_ERR_UNSUPPORTED for N * H * W >= 2^31, or N * ceil(H / 4) * ceil(W / 64) >= 2^24 (one workgroup per 64 x 4
 *     tile; a launch stays below 2^32 threads).
 * N == 0 (with valid arguments otherwise) is CTD_OK and touches nothing.
 */
#ifndef CTD_HIP_WARP_H
#define CTD_HIP_WARP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_depth_warp_workspace_bytes(int B, int V, int H, int W);

int ctd_depth_warp_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                       const float* t, const uint8_t* sources, const uint8_t* targets, int splat, float* z,
                       int64_t* src, int B, int V, int H, int W, void* workspace, size_t workspace_bytes, int device,
                       void* stream);

int ctd_disparity_band_window_f32(const float* prior, float radius, int D, int window, int holes, int32_t* lo,
                                  int32_t* hi, int N, int H, int W, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_WARP_H */
