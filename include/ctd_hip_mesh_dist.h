/* ctd_hip_mesh_dist.h -- nearest-face queries of libctd_hip.so: for every query point the squared distance to the nearest
 * face of an indexed triangle mesh, that face's index and, optionally, the closest point on it.  verts f32 [n][3] and
 * faces int32 [m][3] are what ctd_mesh_bvh_build_f32 of include/ctd_hip.h takes, and `bvh` is the buffer that call wrote
 * for exactly these verts and faces (format and size unchanged), or NULL.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h, ctd_hip_icp.h,
 * ctd_hip_tsdf.h, ctd_hip_mesh.h and ctd_hip_mesh_clean.h (none of which includes it; ctd_version() is unchanged): include
 * what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device` and `stream` (a
 * hipStream_t, passed as void* like everywhere in ctd_hip.h) mean what they mean there.  No buffer the call writes may
 * overlap another buffer of the call.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * One function computes the distance.  point_tri (csrc/ctd_point_tri.h) takes a point p and a face a, b, c and returns
 * the squared distance d2 and the closest point q.
 * - It works in f32, in one fixed operation order, with no contracted multiply-adds.
 * - With ab = b - a, ac = c - a, ap = p - a, bp = p - b, cp = p - c and dot(u, v) = (u0 v0 + u1 v1) + u2 v2 it forms
 *   d1 = dot(ab, ap), d2 = dot(ac, ap), d3 = dot(ab, bp), d4 = dot(ac, bp), d5 = dot(ab, cp), d6 = dot(ac, cp),
 *   vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6, va = d3 d6 - d5 d4.
 * - It classifies by region, as Ericson's closest point on a triangle does, in this order: vertex a (d1 <= 0 and
 *   d2 <= 0), vertex b (d3 >= 0 and d4 <= d3), edge ab (vc <= 0, d1 >= 0, d3 <= 0: s = d1 / (d1 - d3), t = 0),
 *   vertex c (d6 >= 0 and d5 <= d6), edge ac (vb <= 0, d2 >= 0, d6 <= 0: s = 0, t = d2 / (d2 - d6)), edge bc (va <= 0,
 *   d4 - d3 >= 0, d5 - d6 >= 0: t = (d4 - d3) / ((d4 - d3) + (d5 - d6)), s = 1 - t), and otherwise the interior
 *   (inv = 1 / ((va + vb) + vc), s = vb inv, t = vc inv).
 * - A vertex region returns that vertex itself, so a point that is a vertex of the face has d2 == 0 exactly.
 * - Every other region clamps the two parameters after classification: s to [0, 1], then t to [0, 1 - s].  Each clamp is
 *   a comparison that a NaN fails, so a NaN parameter becomes 0.
 * - The closest point is then q = (a + s ab) + t ac, a convex combination of a, a + ab and a + ac whatever rounding did
 *   to the region tests.
 * - d2 = dx dx + dy dy + dz dz with d = p - q, summed in that order.
 *
 * The answer for a point.
 * - It is the face of smallest d2 among the faces whose d2 compares < +inf, so a NaN or overflowed d2 never wins.
 * - On equal d2 the lowest face index wins.
 * - If no face qualifies: face = -1, d2 = +inf, closest = NaN.
 *
 * Which faces take part.
 * - Faces with an index outside [0, n_verts) are skipped and never dereferenced on the brute-force path.  A tree can only
 *   have been built over faces whose indices are all valid (the build reads every vertex), so with a tree there are none.
 * - Degenerate faces are ordinary faces: collinear or coincident vertices get whatever point_tri computes for them.
 *
 * What is returned.
 * - The kernel outputs d2, not the distance.  The square root is the caller's, so no bit depends on a device sqrtf.
 * - The same bits on every run and on both paths, with a tree or without.  One lane owns one point: no atomics and no
 *   flag that another workgroup waits on.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_point_mesh_distance_f32
 *
 * points f32 [n_points][3] -> d2 f32 [n_points], face int32 [n_points] and, when closest is not NULL, closest f32
 * [n_points][3].
 *
 * bvh == NULL: brute force over all faces, streamed in index order; this kernel is the definition.  Otherwise the tree is
 * traversed, the nearer child first, and a node is skipped only when a lower bound on the distance from the point to the
 * node's box, lowered by a slack that covers the rounding of point_tri (derived in csrc/point_mesh.hip), exceeds the best
 * d2 so far.  A point with a non-finite coordinate prunes nothing, and nodes with infinite boxes (faces with non-finite
 * vertices) are never pruned.  The call reads the tree's header with one small synchronous copy.
 *
 * Errors, before any HIP call:
 *   CTD_ERR_INVALID_ARG for n_points < 0, n_verts < 0 or n_faces < 0; for 3 * n_points >= 2^31 or n_faces > 2^28 (the limit
 *     of ctd_mesh_bvh_bytes); for a NULL points, d2 or face when n_points > 0; for a NULL faces when n_faces > 0, or a
 *     NULL verts when n_faces > 0 and n_verts > 0; for a bvh that is not 16-byte aligned.
 * Then: CTD_ERR_INVALID_ARG for a bvh that is not a tree of n_faces faces; CTD_ERR_UNSUPPORTED for a tree deeper than
 * the traversal stack (the depth ctd_mesh_bvh_build_f32 reports and refuses likewise) -- call again with bvh == NULL.
 * n_points == 0 is CTD_OK and does nothing.  n_faces == 0 is CTD_OK and fills the answer of "no face qualifies".
 */
#ifndef CTD_HIP_MESH_DIST_H
#define CTD_HIP_MESH_DIST_H

#include <stddef.h>
#include <stdint.h>

#include "ctd_hip.h" /* the status codes */

#ifdef __cplusplus
extern "C" {
#endif

int ctd_point_mesh_distance_f32(const float* points, int n_points, const float* verts, int n_verts, const int* faces,
                                int n_faces, const void* bvh /* NULL: brute force over all faces */, float* d2, int* face,
                                float* closest /* [n][3], may be NULL */, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_DIST_H */
