/* ctd_hip_mesh_color.h -- colours for mesh points from the views of a track, of libctd_hip.so: every point (a mesh vertex,
 * a TSDF surface point, a surface sample) is projected into each posed view, a view that sees it -- decided by casting
 * the segment from the camera centre to the point against an occluding mesh -- is sampled bilinearly, and the views
 * that see the point are blended.  verts f32 [n][3] and faces int32 [m][3] are what ctd_mesh_bvh_build_f32 of
 * include/ctd_hip.h takes, and `bvh` is the buffer that call wrote for exactly these verts and faces, or NULL.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h, ctd_hip_icp.h,
 * ctd_hip_tsdf.h, ctd_hip_mesh.h, ctd_hip_mesh_clean.h and ctd_hip_mesh_dist.h (none of which includes it; ctd_version()
 * is unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device`
 * and `stream` (a hipStream_t, passed as void* like everywhere in ctd_hip.h) mean what they mean there.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * Everything is f32 and uncontracted, in the written association, with IEEE division and sqrtf.  dot(a, b) =
 * (a0 b0 + a1 b1) + a2 b2, summed from the left.  All arguments describe one track: X_cam = R X_world + t.
 *
 * For a point X the views v = 0 .. V-1 are visited in ascending order.  flags[i][v] starts at 0; each step that passes
 * sets its bit, and a step that fails ends the view.
 *
 * 1. IN_IMAGE (1).
 * - S_j = ((X0 R[j][0] + X1 R[j][1]) + X2 R[j][2]) + t_j, the world_to_camera of csrc/ctd_view.h.
 * - uvd_j = (S0 K[j][0] + S1 K[j][1]) + S2 K[j][2], its project.  uvd2 > 0 is required.
 * - x = uvd0 / uvd2 and y = uvd1 / uvd2.  0 <= x <= W-1 and 0 <= y <= H-1 are required, compared in f32, so a NaN fails.
 * - x0 = fminf(floorf(x), W-2) and fx = x - x0; y0 and fy likewise with H.  A point on the last column or row thus
 *   samples the last pixel pair with fx = 1.
 * - With `valid`, all four pixels (y0 | y0+1, x0 | x0+1) of view v must be nonzero.
 * 2. FACING (2).
 * - Cv_c = -((R[0][c] t0 + R[1][c] t1) + R[2][c] t2), the camera centre in the association of the ray casters.
 * - d = Cv - X and cosv = dot(n, d) / sqrtf(dot(d, d)) with n the point's normal.
 * - cosv > 0 and cosv >= min_cos are required, so a NaN normal fails every view.  Then w = cosv.
 * - With normals == NULL the step always passes and w = 1.
 * 3. UNOCCLUDED (4).
 * - e = X - Cv, len = sqrtf(dot(e, e)), dir = e / len (three divisions), t_max = len - margin.
 * - The view is occluded when some face is accepted by ray_tri(Cv, dir, v0, v1, v2) of csrc/ctd_render.h (the ray
 *   casters' ray/triangle test) with ft > 0 and ft < t_max.
 * - Faces with an index outside [0, n_verts) are skipped and never dereferenced on the brute-force path.  A tree can only
 *   have been built over faces whose indices are all valid, so with a tree there are none.
 * - With n_faces == 0 nothing occludes.
 * - The answer is a boolean, so it is independent of the order in which the faces are visited.
 * 4. The sample, per channel c, of the view's image I = images[v][c]:
 *   top = I[y0][x0] + fx (I[y0][x0+1] - I[y0][x0]), bot = I[y0+1][x0] + fx (I[y0+1][x0+1] - I[y0+1][x0]),
 *   s_c = top + fy (bot - top).
 *
 * A view with flags == 7 is used.
 * - mode 0 (weighted mean): acc_c = acc_c + w s_c and wsum = wsum + w over the used views in ascending v, from 0.  Then
 *   color_c = acc_c / wsum and weight = wsum.
 * - mode 1 (best view): the used view of largest w, the lowest v on a tie.  color = its sample and weight = its w.
 * - n_views is the number of used views.  With no used view color is NaN and weight is 0.
 *
 * What is returned.
 * - The same bits on every run and on both paths, with a tree or without.  One lane owns one point: no atomics and no
 *   flag that another workgroup waits on.
 * - flags[i][v] says, on its own, which views see a point: bit 4 is the occlusion query per (point, view).
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_view_colors_f32
 *
 * points f32 [n_points][3], normals f32 [n_points][3] or NULL, images f32 [V][C][H][W], valid u8 [V][H][W] or NULL,
 * K f32 [3][3], R f32 [V][3][3], t f32 [V][3]; the occluding mesh verts, faces and, optionally, its tree
 * -> color f32 [n_points][C], weight f32 [n_points], n_views int32 [n_points] and, when flags is not NULL, flags u8
 * [n_points][V].  margin is a length in world units: a face closer than margin to the point along the segment does not
 * occlude it (the point's own surface).
 *
 * bvh == NULL: brute force over all faces, streamed in index order; this kernel is the definition.  Otherwise the tree is
 * traversed and left at the first accepted hit; a node is skipped only when no face under it can be accepted with
 * ft <= t_max (the pruning test of the ray casters, derived in csrc/ctd_bvh_ray.h), which contains the hit condition, so
 * the boolean is the brute-force path's.  A non-finite origin, direction or t_max prunes nothing, and nodes with infinite
 * boxes (faces with non-finite vertices) are never pruned.  The call reads the tree's header with one small synchronous
 * copy.  There is no workspace.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_points, n_verts or n_faces < 0; for V < 1 or V > 64; for C < 1 or C > 4; for H or W < 2; for
 *     a mode that is not 0 or 1; for a margin that is not finite and >= 0; for a min_cos that is not finite or lies
 *     outside [0, 1); with n_points > 0 for a NULL points, images, K, R, t, color, weight or n_views; for a NULL faces
 *     when n_faces > 0, or a NULL verts when n_faces > 0 and n_verts > 0; for a bvh that is not 16-byte aligned.
 *   CTD_ERR_UNSUPPORTED for H or W > 2^24 (the bounds of a projected pixel are compared in f32); for V*C*H*W >= 2^31,
 *     3*n_points >= 2^31 or n_points*V >= 2^31; for n_faces > 2^28 (the limit of ctd_mesh_bvh_bytes).
 *   CTD_ERR_INVALID_ARG for an output (color, weight, n_views, flags) overlapping any other buffer of the call.
 * Then: CTD_ERR_INVALID_ARG for a bvh that is not a tree of n_faces faces; CTD_ERR_UNSUPPORTED for a tree deeper than
 * the traversal stack (the depth ctd_mesh_bvh_build_f32 reports and refuses likewise) -- call again with bvh == NULL.
 * n_points == 0 is CTD_OK and touches nothing.
 */
#ifndef CTD_HIP_MESH_COLOR_H
#define CTD_HIP_MESH_COLOR_H

#include <stddef.h>
#include <stdint.h>

#include "ctd_hip.h" /* the status codes */

#ifdef __cplusplus
extern "C" {
#endif

int ctd_mesh_view_colors_f32(const float* points, const float* normals /* may be NULL */, int n_points,
                             const float* images, const uint8_t* valid /* may be NULL */, const float* K, const float* R,
                             const float* t, int V, int C, int H, int W, const float* verts, int n_verts, const int* faces,
                             int n_faces, const void* bvh /* NULL: brute force over all faces */, float margin,
                             float min_cos, int mode, float* color, float* weight, int32_t* n_views,
                             uint8_t* flags /* [n][V], may be NULL */, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_COLOR_H */
