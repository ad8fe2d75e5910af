/* ctd_hip_mesh_register.h -- point-to-mesh ICP of libctd_hip.so: the 6 x 6 normal equations that align a point set, under
 * each of K candidate poses, to an indexed triangle mesh, and the pose update that solves them.  The remedy for a model
 * that sits a small rigid motion away from the mesh it is to be compared with: a few rounds of system + update bring it
 * into the mesh's frame.  It joins two halves the library already has, the nearest-face query of
 * include/ctd_hip_mesh_dist.h / ctd_hip_mesh_sdf.h and the system and solve of include/ctd_hip_icp.h.
 *
 * An addition beside include/ctd_hip.h and the headers next to it (none of which includes it; ctd_version() is
 * unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device`
 * and `stream` mean what they mean there.  No buffer a call writes may overlap another buffer of the call.
 *
 * What it does not do.  No global registration: it converges from the errors a local method converges from (degrees
 * and a fraction of the object's size), and K starts cost one launch so that a caller can try several;
 * ctd_hip_mesh_global.h, next to this header, scores a grid of poses and so finds the starts to try.  No scale.  No
 * robust weights and no rejection of matches on boundary edges in these calls: a point set that overhangs an open mesh
 * pulls towards its rim, and max_d2 is the blunt remedy.  ctd_hip_mesh_robust.h, next to this header, has the weighted
 * and gated system (Huber and Tukey weights, rim rejection, a normal gate); its update is the one below.
 *
 * Common to the calls.  All f32 arithmetic is in the written association and uncontracted.  The cross product u x w is
 * (u1*w2 - u2*w1, u2*w0 - u0*w2, u0*w1 - u1*w0), each component two f32 products and one f32 subtraction, as in
 * ctd_hip_icp.h.  "finite" means neither NaN nor +-inf.  Each product that enters a sum of the system is formed in f64
 * from its two f32 factors and is therefore exact; only the sums round.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_register_system_f32
 *
 * Inputs: points f32 [n_points][3]; K candidate poses R f32 [K][3][3], t f32 [K][3] (multi-start costs one launch);
 * verts f32 [n_verts][3], faces int32 [n_faces][3] and `bvh` (NULL: brute force, the definition) as
 * ctd_point_mesh_distance_f32 takes them; metric 0 (point to plane) or 1 (point to point); max_d2, +inf or a finite float
 * >= 0; hint int32 [K][n_points] or NULL.
 *
 * For every point p = points[i] and pose k:
 *
 * - S_j = ((R_k[j][0] * p0 + R_k[j][1] * p1) + R_k[j][2] * p2) + t_k[j] for j = 0, 1, 2.
 * - (d2, f, q) is exactly what the cutoff query of ctd_hip_mesh_sdf.h gives for the point S with this max_d2: the same
 *   point_tri, the same selection, the same skipped faces; brute force is the definition and the tree gives its bits.
 * - The point is dropped when f == -1 (no face qualifies).  That covers a non-finite S too: every d2 of such a point
 *   is NaN or +inf.
 * - D = S - q, three f32 subtractions.
 *
 * metric 0, one row per point:
 *
 * - (v0, v1, v2) are the stored corners of face f.  e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2,
 *   l = sqrtf(c0*c0 + c1*c1 + c2*c2), summed from the left, n = c / l, three f32 divisions.
 * - The point is dropped unless l > 0 and l is finite.
 * - e = n0*D0 + n1*D1 + n2*D2, summed from the left.  J = (S x n, n), six f32 values.
 * - residual = e.
 *
 * metric 1, three rows per point, r = 0, 1, 2 in this order:
 *
 * - u_r is the unit axis r.  e_r = D_r and J_r = (S x u_r, u_r), the cross product computed as written above.
 * - The three rows are added to every sum one after the other, so sum e*e grows by D0*D0, D1*D1, D2*D2 in turn.
 * - The count is incremented once per point.
 * - residual = sqrtf(d2), with d2 the query's.
 *
 * e is the distance the update drives to zero.  For a small motion (omega, v) of the point, S -> S + omega x S + v, it
 * changes by J . (omega, v).
 *
 * Outputs:
 *
 * - system f64 [K][29] over the points of the pose that were not dropped, in the layout of ctd_depth_icp_system_f32:
 *     [0..20]  the 21 upper-triangle entries of sum J J^T, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5);
 *     [21..26] the 6 entries of sum J e;
 *     [27]     sum e*e;
 *     [28]     the number of points.
 * - face int32 [K][n_points], which may be NULL: f, or -1 where the point was dropped.  It is the next round's hint, and
 *   must not overlap this round's.
 * - residual f32 [K][n_points], which may be NULL: as above, or NaN where the point was dropped.
 * - closest f32 [K][n_points][3], which may be NULL: q as the query gives it (three NaNs where no face qualified).
 *
 * The hint.  hint[k][i] names the face that point i had under pose k last time.  It is used when it lies in
 * [0, n_faces) and that face's three vertex indices lie in [0, n_verts), and ignored otherwise; the traversal of the tree
 * then starts with that face as its best instead of with nothing.  It changes no bit of any output, whatever it holds
 * (csrc/ctd_point_mesh_nearest.h argues why); brute force ignores it.
 *
 * The order of every sum is fixed, so the same bits come out on every run; it is that of ctd_depth_icp_system_f32 with
 * the point index in place of the pixel index and a pose in place of a view.  A workgroup of 256 threads takes 1024
 * consecutive points of ONE pose: thread i sums the points i, i + 256, i + 512, i + 768 of the chunk, ascending, into 29
 * f64 registers; a butterfly over the lane distances 32, 16, 8, 4, 2, 1 sums the 64 lanes of a wavefront; the four
 * wavefronts are summed ascending; the workgroup's 29 sums go to the workspace.  A second pass sums a pose's workgroups
 * ascending.  No atomics.  A term that overflows f32 in J or e (inf or NaN) poisons its sums, as it would any sum.
 *
 * Four launches: the posed points S go to the workspace, the nearest-face kernel of ctd_point_mesh_distance_f32 (with
 * the cutoff and the hint) answers for all K * n_points of them at once, the system kernel reads S, d2, f and q back and
 * reduces, and the finish kernel sums the workgroups.  With a tree the call reads its header with one small synchronous
 * copy, like the queries.
 *
 * Workspace: ctd_mesh_register_workspace_bytes(K, n_points) bytes, 256-byte aligned: S, d2, f, q of every posed point
 * and 29 f64 per workgroup.  The call never allocates, and it writes every word of the workspace that it reads, so the
 * workspace may hold anything.  The query returns 0 for arguments that the first three errors reject and for
 * n_points == 0.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_points < 0, n_verts < 0 or n_faces < 0; for K < 1 or K > 64; for 3 * K * n_points >= 2^31 or
 *     n_faces > 2^28; for a metric other than 0 and 1; for a max_d2 that is NaN or negative; for a NULL R, t or system, a
 *     NULL points when n_points > 0, a NULL faces when n_faces > 0, or a NULL verts when n_faces > 0 and n_verts > 0; for a
 *     bvh that is not 16-byte aligned; for system, face, residual, closest or the workspace overlapping any other buffer
 *     of the call, hint included;
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace (unless n_points == 0, which needs none).
 * Then: CTD_ERR_INVALID_ARG for a bvh that is not a tree of n_faces faces; CTD_ERR_UNSUPPORTED for a tree deeper than
 * the traversal stack -- call again with bvh == NULL.
 * n_points == 0 or n_faces == 0 is CTD_OK: systems of zeros, and for n_faces == 0 face -1, residual NaN and closest NaN.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_register_update_f32
 *
 * Inputs: system f64 [K][29] as above, R, t, min_count an int >= 0, min_pivot and damping doubles >= 0.  Outputs:
 * R_out f32 [K][3][3], t_out f32 [K][3], ok u8 [K].  One thread per pose; everything below is f64, in the written
 * association and uncontracted, on the f32 inputs converted exactly.
 *
 * - The damped LDL^T of the system, the refusal conditions (system[28] < min_count, a pivot that is not finite, a pivot
 *   D_j <= min_pivot * A_jj), the three solves for xi = (omega, v) and the Rodrigues step (Rr, tr = v) are those of
 *   ctd_depth_icp_update_f32 in include/ctd_hip_icp.h, word for word; the two calls run the same code.
 * - Every S above becomes Rr S + tr: R'_ij = Rr_i0 * R_0j + Rr_i1 * R_1j + Rr_i2 * R_2j and
 *   t'_i = Rr_i0 * t_0 + Rr_i1 * t_1 + Rr_i2 * t_2 + tr_i, each summed from the left.
 * - R' and t' are rounded to f32 once, at the end, and ok = 1.
 * - A refused pose is copied through, R_out = R and t_out = t bit for bit, with ok = 0.
 *
 * R is not re-orthonormalised.  No workspace.  ok speaks of this call alone: when system and update are iterated, a
 * pose whose last round ends with ok = 0 keeps whatever the earlier rounds left it with, and is not to be used.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for K < 1 or K > 64, min_count < 0, a negative or NaN min_pivot or damping, a NULL system / R /
 *     t / R_out / t_out / ok, or R_out, t_out or ok overlapping any other buffer of the call.
 */
#ifndef CTD_HIP_MESH_REGISTER_H
#define CTD_HIP_MESH_REGISTER_H

#include "../ctd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_mesh_register_workspace_bytes(int K, int n_points);

int ctd_mesh_register_system_f32(const float* points, int n_points, const float* R, const float* t, int K,
                                 const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh,
                                 int metric, float max_d2, const int32_t* hint, double* system, int32_t* face,
                                 float* residual, float* closest, void* workspace, size_t workspace_bytes, int device,
                                 void* stream);

int ctd_mesh_register_update_f32(const double* system, const float* R, const float* t, int min_count, double min_pivot,
                                 double damping, float* R_out, float* t_out, uint8_t* ok, int K, int device,
                                 void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_REGISTER_H */
