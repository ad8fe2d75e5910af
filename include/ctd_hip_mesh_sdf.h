/* ctd_hip_mesh_sdf.h -- signed nearest-face queries of libctd_hip.so: for every query point the squared distance to the
 * nearest face of an indexed triangle mesh within a cutoff, that face, the closest point on it, the feature of the face
 * the closest point lies on (a vertex, an edge, the interior) and the side of the oriented surface the point is on.
 * verts f32 [n][3], faces int32 [m][3] and `bvh` are what ctd_point_mesh_distance_f32 of include/ctd_hip_mesh_dist.h takes;
 * face_offsets int32 [n_verts+1] and face_ids int32 [n_incident] are the incident-face rows of a meshsmooth.MeshAdjacency of
 * these faces (the adjacency call of the smoothing header writes them).
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h, ctd_hip_icp.h,
 * ctd_hip_tsdf.h, ctd_hip_mesh.h, ctd_hip_mesh_clean.h, ctd_hip_mesh_dist.h and the colour, smoothing and simplification
 * headers (none of which includes it; ctd_version() is unchanged): include what you call.  The status
 * codes are those of ctd_hip.h; pointers are device pointers, `device` and `stream` (a hipStream_t, passed as void* like
 * everywhere in ctd_hip.h) mean what they mean there.  No buffer the call writes may overlap another buffer of the call.
 *
 * The sign convention is that of ctd_hip_mesh.h, which orients every triangle so that (v1 - v0) x (v2 - v0) points from
 * inside (T < 0) towards free space: sign +1 is the side the normals point to, the side on which a TSDF is positive.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * Nearest face.  Exactly the rule of ctd_hip_mesh_dist.h: the same point_tri, the same selection, the same skipped faces.
 * - One addition, the cutoff max_d2: +inf or a finite float >= 0.
 * - A face qualifies when its d2 compares <= max_d2 and < +inf.
 * - With max_d2 = +inf the outputs d2, face and closest are those of ctd_point_mesh_distance_f32, bit for bit.
 * - If no face qualifies: face = -1, d2 = +inf, closest = NaN, feature = -1, sign = 0.
 * - In the tree a node is pruned when its bound exceeds min(best d2, max_d2).  The forward-error argument of
 *   csrc/point_mesh.hip covers this without change: no face under such a node can qualify.
 * - Brute force stays the definition, and the tree gives its bits.
 *
 * Feature (int8).  The branch that point_tri took for the winning face, not a reclassification of the clamped parameters:
 * 0, 1, 2 for vertex a, b, c; 3, 4, 5 for edge ab, ac, bc; 6 for the interior.  (On edge bc point_tri sets s = 1 - t and
 * then m = 1 - s, and rounding can make t != m: the parameters do not say which branch produced them.)
 *
 * Pseudonormal N (Baerentzen and Aanaes, angle weighted).  All of it in f64, computed from the f32 vertices, with no
 * contracted multiply-adds, in the association written here.
 * - A face is valid as in the smoothing header: its indices lie in [0, n_verts) and are pairwise different.
 * - unit(g), with the stored corners (v0,v1,v2): e1 = v1 - v0, e2 = v2 - v0,
 *   c = (e1y e2z - e1z e2y, e1z e2x - e1x e2z, e1x e2y - e1y e2x), l = sqrt((cx cx + cy cy) + cz cz),
 *   unit = c / l (three divisions) when l > 0 and l is finite.  Otherwise the face contributes nothing.
 * - Interior of face f: N = c of f, not normalised.
 * - Edge {i,j} of face f: walk the row of incident faces of vertex min(i,j) in ascending order (the order of the row).
 *   Every valid face with min(i,j) at one corner and max(i,j) at another adds its unit(g).  That includes f itself; a
 *   boundary edge gets one term, a non-manifold edge all of its terms, i == j none.
 * - Vertex i: walk the row of i in ascending order.  Every valid face g with i at a corner adds alpha_g * unit(g) (three
 *   multiplications), where u and w run from i to g's next and next-but-one corner in stored cyclic order, x = u x w
 *   computed as c above, and alpha_g = atan2(sqrt((xx xx + xy xy) + xz xz), (u0 w0 + u1 w1) + u2 w2).  A term with a
 *   component that is not finite adds nothing.
 * - N starts at 0 and every term is added per component, N = N + term, in row order.
 * - Sign: r = (double)p - (double)q and dot = (r0 N0 + r1 N1) + r2 N2.  sign = +1 when dot > 0, -1 when dot < 0 and 0
 *   otherwise: dot == 0, a NaN, p on the mesh, no contributing face.
 * - This is exact for closed, consistently oriented manifold meshes.  On open meshes it says which side of the nearest piece
 *   of surface the point is on.  The sign follows the stored winding; nothing repairs an inconsistently oriented mesh.
 *
 * Bounds.  The rows are any values, as in the smoothing and normals calls of the smoothing header.
 * - A row is empty unless 0 <= face_offsets[i] <= face_offsets[i+1] <= n_incident.
 * - A face id outside [0, n_faces) is never dereferenced.
 * - A vertex index outside [0, n_verts) is never dereferenced.
 *
 * What is returned.
 * - d2, not the distance, and a sign beside it: the square root and the product are the caller's.
 * - d2, face, closest and feature are the same bits on every run and on both paths, with a tree or without.  So is sign on
 *   one device: its only operation that is not correctly rounded is the atan2 of the vertex weights.
 * - One lane owns one point: no atomics and no flag that another workgroup waits on.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_point_mesh_signed_f32
 *
 * points f32 [n_points][3] -> d2 f32 [n_points], face int32 [n_points], feature int8 [n_points], sign int8 [n_points] and,
 * when closest is not NULL, closest f32 [n_points][3].
 *
 * Two launches: the nearest-face kernel of ctd_point_mesh_distance_f32 (bvh == NULL: brute force, the definition;
 * otherwise the traversal) with the cutoff and the recorded branch, then one lane per point for the sign, which reads at
 * most one row of incident faces.  A row is as long as it says; the rows of an adjacency that is fit for use hold at most the
 * smoothing header's cap of 1024 incident faces, so a lane's loop is bounded.  The call reads the tree's header with one small synchronous copy.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_points < 0, n_verts < 0, n_faces < 0 or n_incident < 0; for 3 * n_points >= 2^31 or
 *     n_faces > 2^28 (the limit of ctd_mesh_bvh_bytes); for a max_d2 that is NaN or negative; for a NULL points, d2, face,
 *     feature, sign, face_offsets or face_ids when n_points > 0; for a NULL faces when n_faces > 0, or a NULL verts when
 *     n_faces > 0 and n_verts > 0; for a bvh that is not 16-byte aligned.
 * Then: CTD_ERR_INVALID_ARG for a bvh that is not a tree of n_faces faces; CTD_ERR_UNSUPPORTED for a tree deeper than
 * the traversal stack -- call again with bvh == NULL.
 * n_points == 0 is CTD_OK and does nothing.  n_faces == 0 is CTD_OK and fills the answer of "no face qualifies".
 */
#ifndef CTD_HIP_MESH_SDF_H
#define CTD_HIP_MESH_SDF_H

#include <stddef.h>
#include <stdint.h>

#include "ctd_hip.h" /* the status codes */

#ifdef __cplusplus
extern "C" {
#endif

int ctd_point_mesh_signed_f32(const float* points, int n_points, const float* verts, int n_verts, const int* faces,
                              int n_faces, const int32_t* face_offsets, const int32_t* face_ids, int64_t n_incident,
                              const void* bvh /* NULL: brute force over all faces */, float max_d2, float* d2, int* face,
                              float* closest /* [n][3], may be NULL */, int8_t* feature, int8_t* sign, int device,
                              void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_SDF_H */
