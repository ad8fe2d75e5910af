/* ctd_hip_tsdf.h -- truncated signed distance volumes of libctd_hip.so: the views of a track integrated into one voxel
 * grid per track, the surface points of the grid, and a ray cast of it into a depth map at any pose.  The model that the
 * per-view calls lack: it averages the views where they agree and yields one surface, and a ray cast of it is a depth
 * map without holes that ctd_depth_icp_system_f32 takes as a target view (frame-to-model alignment) and that
 * ctd_disparity_band_window_f32 takes as a band prior.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h and ctd_hip_icp.h (none
 * of which includes it; ctd_version() is unchanged): include what you call.  The status codes are those of ctd_hip.h;
 * pointers are device pointers, `device` and `stream` mean what they mean there.  No buffer a call writes may overlap
 * another buffer of the call.
 *
 * Common to the calls.  Per track b there is one grid of nx x ny x nz voxels.  tsdf and weight are f32 [B][nz][ny][nx],
 * x fastest.  origin f32 [B][3] is the world position of the centre of voxel (0,0,0) and voxel is a scalar f32: the
 * centre of voxel (i,j,k) is X_c = origin[b][c] + voxel * (float)index_c, with (index_0, index_1, index_2) = (i, j, k).
 * A fresh volume has weight == 0 everywhere.  tsdf is never read where weight == 0.  depth f32 [B][V][H][W], valid u8
 * [B][V][H][W] or NULL, ray [H*W][3], K [3][3], R [B][V][3][3], t [B][V][3] are the inputs of ctd_depth_consistency_f32
 * (X_cam = R X_world + t).  A pixel is live under the rule of ctd_hip.h: valid is nonzero (NULL: everywhere), and depth
 * is finite and > 0.  All arithmetic is f32 in the written association and uncontracted, with IEEE division and sqrtf.
 * "finite" means neither NaN nor +-inf.  No call uses atomics; the same bits come out on every run.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_tsdf_integrate_f32
 *
 * Updates tsdf and weight in place.  trunc is a finite float > 0, max_weight a finite float >= 1.  The documented use
 * passes the keep of ctd_depth_consistency_f32 as valid: gross outliers that reach the volume bias it.
 *
 * For each voxel, with X its centre, visit the views v = 0 .. V-1 in ascending order and apply these steps.
 *
 * 1. Compute the point in camera v: S_c = X0*R[c][0] + X1*R[c][1] + X2*R[c][2] + t[c], summed from the left.  Then
 *    uvd_j = S0*K[j][0] + S1*K[j][1] + S2*K[j][2], the last line of "the transform from view a to view b" of ctd_hip.h.
 *    Skip the view unless uvd2 > 0.
 * 2. Round to a pixel: xs = floorf(uvd0/uvd2 + 0.5f) and ys = floorf(uvd1/uvd2 + 0.5f).  Skip the view unless
 *    0 <= xs <= W-1 and 0 <= ys <= H-1, compared in f32 before any conversion, so a NaN fails them.  q = ys*W + xs.
 *    Skip the view unless q is live in view v.
 * 3. sdf = depth[q]*ray[q][2] - S2.  Skip the view if sdf < -trunc.
 * 4. obs = fminf(1, sdf/trunc).
 * 5. If weight == 0 then tsdf = obs, else tsdf = (tsdf*weight + obs)/(weight + 1).
 * 6. weight = fminf(weight + 1, max_weight).
 *
 * One launch integrates all V views.  A voxel's tsdf and weight live in registers across the view loop: every voxel is
 * read at most once and written at most once per call, and a voxel that no view touched is not stored.  A workgroup
 * takes a tile of 64 voxels along x and 4 along y of one z slice of one track; a thread takes one voxel.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for nx, ny, nz, V, H or W < 1, B < 0, V > 64, a voxel or trunc that is not finite and > 0, a
 *     max_weight that is not finite and >= 1, or a NULL tsdf / weight / origin / depth / ray / K / R / t;
 *   CTD_ERR_UNSUPPORTED for nx, ny or nz > 2048, B * nx * ny * nz >= 2^31, H or W > 2^24, B * V * H * W >= 2^31, or
 *     B * nz * ceil(ny / 4) * ceil(nx / 64) >= 2^24 (one workgroup per tile; a launch stays below 2^32 threads);
 *   CTD_ERR_INVALID_ARG for tsdf or weight overlapping any other buffer of the call.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_tsdf_surface_points_f32
 *
 * The zero crossings of tsdf between neighbouring voxels.  min_weight is a finite float > 0.
 *
 * A voxel is usable when weight >= min_weight and |tsdf| < 1.  The |tsdf| < 1 clause rejects crossings against truncated
 * free space, which is where false back faces at occlusion edges come from.
 *
 * Take each voxel a and each axis c in {x, y, z}.  Let n be its +c neighbour inside the grid.  Emit a point when both are
 * usable and (T_a < 0) != (T_n < 0), with T the tsdf.
 *
 * - The point's coordinates are those of the centre of a, with component c increased by voxel * (T_a / (T_a - T_n)).
 * - src = (((b*nz + k)*ny + j)*nx + i)*3 + c.
 * - Points come out in ascending src.  n_per_track int64 [B] holds the true counts.
 *
 * The normal is the gradient of tsdf by central differences, g_c = T(+c) - T(-c), taken at whichever of a and n has
 * the smaller |T| (a on a tie).  It is normalised as g / sqrtf(g0*g0 + g1*g1 + g2*g2), summed from the left, three f32
 * divisions.  It points towards free space.  It is three NaNs when any of the six neighbours is outside the grid or has
 * weight < min_weight, or when the squared length is 0.
 *
 * Outputs: points f32 [capacity][3], normals f32 [capacity][3] or NULL, src int64 [capacity], n_per_track int64 [B].
 * The call writes the first `capacity` points (in ascending src) and always writes the true n_per_track; entries of
 * points, normals and src past the true count are not written.  With points == NULL it only counts: normals, src and
 * capacity are ignored.
 *
 * Three passes, the scheme of ctd_depth_fuse_points_f32: a workgroup takes 256 consecutive voxels of ONE track and counts
 * their crossings; one workgroup scans the counts; the workgroups write their points at the scanned offsets.
 *
 * Workspace: ctd_tsdf_surface_workspace_bytes(B, nx, ny, nz) bytes, 256-byte aligned.  The call never allocates, and
 * it writes every word of the workspace that it reads, so the workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for nx, ny or nz < 1, B < 0, a voxel or min_weight that is not finite and > 0, a NULL tsdf /
 *     weight / origin / n_per_track, or, with points != NULL, capacity < 0 or a NULL src;
 *   CTD_ERR_UNSUPPORTED for nx, ny or nz > 2048, B * nx * ny * nz >= 2^31, 3 * B * nx * ny * nz >= 2^31 (the scanned
 *     offsets are int32), or B * ceil(nx * ny * nz / 256) >= 2^24;
 *   CTD_ERR_INVALID_ARG for points, normals, src, n_per_track or the workspace overlapping any other buffer of the call
 *     (points, normals and src count with min(capacity, 3 * B * nx * ny * nz) entries: there are no more crossings);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing, the workspace included.  The workspace query
 * returns 0 for shapes that one of the first two errors rejects and for B == 0.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_tsdf_raycast_f32
 *
 * Output depth f32 [B][V][H][W]: the depth along ray[p] at which the ray of pixel p of a camera at pose R[b][v], t[b][v]
 * (any poses, not only those integrated) first crosses the surface of track b's volume from outside, NaN where it finds
 * none.  d_min is a finite float >= 0, step and min_weight finite floats > 0, n_steps an int >= 1.
 *
 * For pixel p, sample the depths d_n = d_min + step*(float)n for n = 0 .. n_steps-1.
 *
 * - World point.  P_i = d_n*ray[p][i] - t[i], then X_j = P0*R[0][j] + P1*R[1][j] + P2*R[2][j], summed from the left.
 *   This is the association of ctd_depth_fuse_points_f32.
 * - Grid coordinates.  g_c = (X_c - origin_c)/voxel, i0_c = floorf(g_c), f_c = g_c - i0_c.
 * - Defined samples.  The sample is defined when 0 <= i0_c <= n_c - 2 for every c (compared in f32, so a NaN fails) and
 *   all eight corners (i0_0 + 0|1, i0_1 + 0|1, i0_2 + 0|1) have weight >= min_weight.
 * - Value.  The value is trilinear: along x first (a = T0 + fx*(T1 - T0) for the four x edges), then y, then z, each in
 *   that same form, with T0 the corner at the lower index.
 *
 * March the samples in order.
 *
 * - At the first n where the sample is defined with value T_n <= 0: if sample n-1 was defined with T_{n-1} > 0, the
 *   depth is d_{n-1} + step*(T_{n-1}/(T_{n-1} - T_n)).  Otherwise the ray met the inside of a surface first, and the depth
 *   is NaN.  Either way the ray stops.
 * - If no such n exists, the depth is NaN.
 *
 * No normals are produced here: ctd_depth_normals_f32 of the output gives them.  A workgroup takes a 64 x 4 tile of one
 * view; a thread takes one pixel and leaves its loop at the first crossing.  Nothing is written but depth.  No workspace.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for nx, ny, nz, V, H, W or n_steps < 1, B < 0, V > 64, a voxel, step or min_weight that is not
 *     finite and > 0, a d_min that is not finite and >= 0, or a NULL tsdf / weight / origin / ray / R / t / depth;
 *   CTD_ERR_UNSUPPORTED for nx, ny or nz > 2048, B * nx * ny * nz >= 2^31, H or W > 2^24, B * V * H * W >= 2^31, or
 *     B * V * ceil(H / 4) * ceil(W / 64) >= 2^24;
 *   CTD_ERR_INVALID_ARG for depth overlapping any other buffer of the call.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing.
 */
#ifndef CTD_HIP_TSDF_H
#define CTD_HIP_TSDF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int ctd_tsdf_integrate_f32(float* tsdf, float* weight, const float* origin, float voxel, const float* depth,
                           const uint8_t* valid, const float* ray, const float* K, const float* R, const float* t,
                           float trunc, float max_weight, int B, int nx, int ny, int nz, int V, int H, int W, int device,
                           void* stream);

size_t ctd_tsdf_surface_workspace_bytes(int B, int nx, int ny, int nz);

int ctd_tsdf_surface_points_f32(const float* tsdf, const float* weight, const float* origin, float voxel, float min_weight,
                                float* points, float* normals, int64_t* src, int64_t* n_per_track, int64_t capacity, int B,
                                int nx, int ny, int nz, void* workspace, size_t workspace_bytes, int device, void* stream);

int ctd_tsdf_raycast_f32(const float* tsdf, const float* weight, const float* origin, float voxel, const float* ray,
                         const float* R, const float* t, float d_min, float step, int n_steps, float min_weight,
                         float* depth, int B, int nx, int ny, int nz, int V, int H, int W, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_TSDF_H */
