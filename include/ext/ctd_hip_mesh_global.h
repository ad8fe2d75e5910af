/* ctd_hip_mesh_global.h -- the scoring kernel of the global point-to-mesh registration of libctd_hip.so: a point set under
 * many thousands of candidate poses against a volume of quantised unsigned distances to a mesh, one exact integer score
 * per pose.  The hot middle of meshglobal.global_mesh_icp: a rotation grid times a few offsets is scored here, the best
 * few poses become the starts of ctd_mesh_register_system_f32 / ctd_mesh_robust_system_f32, which refine up to 64 of them
 * in one launch.  ctd_hip_mesh_register.h and ctd_hip_mesh_robust.h are local methods; this is what produces their starts.
 *
 * An addition beside include/ctd_hip.h and the headers next to it (none of which includes it; ctd_version() is
 * unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device`
 * and `stream` mean what they mean there.
 *
 * What it does not do.  It builds no distance volume (meshglobal.distance_levels does, in torch ops around the point
 * query of ctd_hip_mesh_sdf.h), it picks no starts and refines nothing.  No scale, no reflection.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_pose_score_u8
 *
 * Inputs: points f32 [n_points][3]; R f32 [n_rot][3][3] and base f32 [n_rot][3], a rotation and the translation that goes
 * with it; offsets f32 [n_off][3], added to every base; levels u8 [nz][ny][nx], x fastest, a distance in units of
 * trunc / 255 with 255 for "trunc or farther"; origin f32 [3], ON THE DEVICE, the centre of voxel (0,0,0); voxel, the
 * edge of a voxel.  Output: score int64 [n_rot][n_off].
 *
 * All f32 arithmetic is in the written association and uncontracted, and the division is IEEE's.  For point i with the
 * coordinates (p0, p1, p2), rotation m, offset j and c = 0, 1, 2 (x, y, z):
 *
 *   Q_c = ((R_m[c][0] * p0 + R_m[c][1] * p1) + R_m[c][2] * p2) + base_m[c]     (the association of transform_points)
 *   S_c = Q_c + offsets[j][c]
 *   u_c = (S_c - origin[c]) / voxel
 *   g_c = floorf(u_c + 0.5f)
 *
 * The point is inside when 0 <= g_c < dim_c for all three c, with (dim_0, dim_1, dim_2) = (nx, ny, nz).  The comparisons
 * are made on the floats, before any conversion to an integer: a NaN or an infinity fails them, and so does a value
 * that no int holds.  Then
 *
 *   q = levels[(g_2 * ny + g_1) * nx + g_0] when the point is inside, 255 otherwise
 *   score[m][j] = the sum over i of q * q
 *
 * The score is an exact integer: every summation order, every tiling and every order of the points gives the same bits.
 * With n_points <= 65536 a score is at most 65536 * 65025 = 4 261 478 400 < 2^32, so the kernel sums in 32-bit unsigned
 * words and widens once at the store.  A lower score is a better pose; 65025 * n_points is "no point near the surface".
 *
 * One launch (more only beyond 2^24 - 1 workgroups): one 256-thread workgroup per rotation and tile of 8 offsets.  R_m,
 * base_m, the tile's offsets, origin and voxel are uniform over the workgroup.  A thread strides over the points, computes
 * Q once per point, and per offset of the tile does three adds, the index arithmetic and one byte load.  A butterfly
 * over the wavefront, the four wavefronts' sums through LDS, one int64 store per offset.  No atomics, no workspace; the
 * volume is read with plain loads (gathers: which cache lines 64 lanes touch depends on how near their points are in
 * space, so callers sort the points along a space-filling curve once; the sort changes no bit).  Nothing outside the
 * volume is ever read.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_points < 0 or n_points > 65536; for n_rot < 1, n_off < 1, n_off > 4096 or
 *     n_rot * n_off >= 2^31; for nx, ny or nz outside [1, 1024]; for a voxel that is not finite and > 0 (a NaN fails); for
 *     a NULL R, base, offsets, levels, origin or score, or a NULL points when n_points > 0; for score overlapping points,
 *     R, base, offsets, levels or origin.
 * n_points == 0 is CTD_OK: every score is 0 (one launch, which reads no point).
 */
#ifndef CTD_HIP_MESH_GLOBAL_H
#define CTD_HIP_MESH_GLOBAL_H

#include "../ctd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ctd_pose_score_u8(const float* points, int n_points, const float* R, const float* base, int n_rot,
                      const float* offsets, int n_off, const uint8_t* levels, int nx, int ny, int nz, const float* origin,
                      float voxel, int64_t* score, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_GLOBAL_H */
