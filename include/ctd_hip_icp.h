/* ctd_hip_icp.h -- depth-map normals and projective point-to-plane ICP of libctd_hip.so: per-pixel surface normals of
 * a track's depth maps, the 6 x 6 normal equations that align one view of a track to another, and the pose update that
 * solves them.  The remedy for poses that are slightly wrong (odometry, a real sensor): a few rounds of system + update
 * bring a view back to where ctd_depth_consistency_f32 and ctd_depth_warp_f32 confirm it again.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h and ctd_hip_band_validity.h (none of which
 * includes it; ctd_version() is unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are
 * device pointers, `device` and `stream` mean what they mean there.  No buffer a call writes may overlap another buffer
 * of the call.
 *
 * Common to the calls.  depth f32 [B][V][H][W], valid u8 [B][V][H][W] or NULL, ray [H*W][3], K [3][3], R [B][V][3][3],
 * t [B][V][3] are the inputs of ctd_depth_consistency_f32 (X_cam = R X_world + t).  A pixel is live under the rule of
 * ctd_hip.h: valid is nonzero (NULL: everywhere), and depth is finite and > 0.  All f32 arithmetic is in the written
 * association and uncontracted.  The cross product u x w is (u1*w2 - u2*w1, u2*w0 - u0*w2, u0*w1 - u1*w0), each
 * component two f32 products and one f32 subtraction.  "finite" means neither NaN nor +-inf.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_depth_normals_f32
 *
 * Output normal f32 [B][V][H][W][3]: the unit normal of the surface at each pixel, in the frame of the pixel's own
 * camera, facing the camera.  No pose is needed.  max_rel is a float >= 0.
 *
 * A pixel (y, x) of a view gets a normal when all of the following hold:
 *
 * - 1 <= x <= W-2 and 1 <= y <= H-2.
 * - The pixel and its four axis neighbours (y, x-1), (y, x+1), (y-1, x), (y+1, x) are live.
 * - Every neighbour satisfies |d_nb - d| <= max_rel * d, with d the pixel's depth (one f32 subtraction, one f32
 *   product).
 *
 * The normal is computed as follows:
 *
 * - P(q) = d(q) * ray[q], three f32 products.
 * - a = P(y,x+1) - P(y,x-1) and b = P(y+1,x) - P(y-1,x).
 * - c = a x b.
 * - l = sqrtf(c0*c0 + c1*c1 + c2*c2), summed from the left.
 * - The pixel gets no normal unless l > 0 and l < inf.
 * - n = c / l, three f32 divisions.
 * - n is negated when n0*P0 + n1*P1 + n2*P2 > 0, with P = P(y,x), summed from the left.
 *
 * Every other pixel gets three NaNs.  No atomics; the same bits come out on every run.  No workspace.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for V, H or W < 1, B < 0, V > 64, a negative or NaN max_rel, or a NULL depth / ray / normal;
 *   CTD_ERR_UNSUPPORTED for H or W > 2^24, B * V * H * W >= 2^31, or B * V * ceil(H / 4) * ceil(W / 64) >= 2^24 (one
 *     workgroup per 64 x 4 tile; a launch stays below 2^32 threads);
 *   CTD_ERR_INVALID_ARG for normal overlapping depth, valid or ray.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_depth_icp_system_f32
 *
 * Inputs: the track, normal f32 [B][V][H][W][3] as above (NaN where a pixel has none), target int32 [B][V] or NULL,
 * max_dist a float >= 0.
 *
 * View s of track b is aligned to view a = target[b][s].  A value outside 0..V-1, or equal to s, skips the view.  A NULL
 * target stands for zeros: every view s >= 1 is aligned to view 0, and view 0 is skipped.  A skipped view gets a system
 * of zeros, a residual of NaN and an assoc of -1 at every pixel.
 *
 * For every live pixel q of view s, with d its depth:
 *
 * - S and uvd are those of "the transform from view a to view b" of ctd_hip.h with the source view s in the role of its
 *   a and the target view a in the role of its b: P = d * ray[q] - t_s, Q = P R_s (row vector times matrix),
 *   S = R_a Q + t_a, uvd = K S, in that association.  S is the point in the frame of camera a.
 * - The pixel is dropped unless uvd2 > 0.
 * - xs = floor(uvd0 / uvd2 + 0.5f) and ys = floor(uvd1 / uvd2 + 0.5f).  These are f32 operations.
 * - The pixel is dropped unless 0 <= xs <= W-1 and 0 <= ys <= H-1.  The compares are in f32 before any conversion, so a
 *   NaN fails them.
 * - p = ys*W + xs.  The pixel is dropped unless p is live in view a and the three components of normal[b][a][p] are
 *   finite.
 * - Y = d_a(p) * ray[p] and D = S - Y.
 * - The pixel is dropped unless D0*D0 + D1*D1 + D2*D2 <= max_dist*max_dist (summed from the left; the right side is
 *   one f32 product; a NaN fails the compare).
 * - n = normal[b][a][p] and e = n0*D0 + n1*D1 + n2*D2, summed from the left.
 * - J = (S x n, n), six f32 values.
 *
 * e is the signed distance of the point from the tangent plane of the surface that view a sees at p.  For a small
 * motion (omega, v) of the point, S -> S + omega x S + v, it changes by J . (omega, v).
 *
 * Outputs:
 *
 * - residual f32 [B][V][H][W], which may be NULL: e, or NaN where the pixel was dropped or is not live.
 * - assoc int64 [B][V][H][W], which may be NULL: the flat index ((b*V + a)*H + ys)*W + xs of the pixel hit (the
 *   convention of ctd_depth_fuse_points_f32), or -1 where the pixel was dropped or is not live.
 * - system f64 [B][V][29] over the pixels of the view that were not dropped:
 *     [0..20]  the 21 upper-triangle entries of sum J J^T, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5);
 *     [21..26] the 6 entries of sum J e;
 *     [27]     sum e*e;
 *     [28]     the number of pixels.
 *
 * Each product is formed in f64 from its two f32 factors and is therefore exact; only the sums round.  A term that
 * overflows f32 in J or e (inf or NaN) poisons its sums, as it would any sum.
 *
 * The order of every sum is fixed, so the same bits come out on every run.  A workgroup of 256 threads takes 1024
 * consecutive pixels of ONE view: thread i sums the pixels i, i + 256, i + 512, i + 768 of the chunk, ascending, into
 * 29 f64 registers; a butterfly over the lane distances 32, 16, 8, 4, 2, 1 sums the 64 lanes of a wavefront; the four
 * wavefronts are summed ascending; the workgroup's 29 sums go to the workspace.  A second pass sums a view's workgroups
 * ascending.  No atomics.
 *
 * Workspace: ctd_depth_icp_workspace_bytes(B, V, H, W) bytes, 256-byte aligned: 29 f64 per workgroup.  The call never
 * allocates, and it writes every word of the workspace that it reads, so the workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for V, H or W < 1, B < 0, V > 64, a negative or NaN max_dist, or a NULL depth / normal / ray /
 *     K / R / t / system;
 *   CTD_ERR_UNSUPPORTED for H or W > 2^24, B * V * H * W >= 2^31, or B * V * ceil(H * W / 1024) >= 2^24;
 *   CTD_ERR_INVALID_ARG for system, residual, assoc or the workspace overlapping any other buffer of the call;
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing, the workspace included.  The workspace query
 * returns 0 for shapes that one of the first two errors rejects and for B == 0.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_depth_icp_update_f32
 *
 * Inputs: system f64 [B][V][29] as above, R, t, target (or NULL) as above, min_count an int >= 0, min_pivot and damping
 * doubles >= 0.  Outputs: R_out f32 [B][V][3][3], t_out f32 [B][V][3], ok u8 [B][V].  One thread per view; everything
 * below is f64, in the written association and uncontracted, on the f32 inputs converted exactly.
 *
 * - A is the symmetric 6 x 6 matrix of the triangle and g = system[21..26].  Ad is A with each diagonal entry replaced
 *   by A_ii + damping * A_ii.
 * - Ad = L D L^T with L unit lower triangular, column by column, j = 0..5:
 *     D_j = Ad_jj - sum_{k<j} (L_jk * L_jk) * D_k, the terms subtracted one after the other, k ascending;
 *     L_ij = (Ad_ij - sum_{k<j} (L_ik * L_jk) * D_k) / D_j for i > j, likewise.
 * - The view is left unchanged when any of these holds:
 *     the view is skipped (its target is outside 0..V-1 or equal to s);
 *     system[28] < min_count (a NaN count fails too);
 *     any pivot D_j is not finite;
 *     any pivot D_j <= min_pivot * A_jj, with A_jj the undamped diagonal entry (a NaN product fails too).
 * - Unchanged means R_out = R and t_out = t bit for bit, with ok = 0.
 * - Otherwise xi = -Ad^-1 g by the three solves: y_i = -g_i - sum_{k<i} L_ik * y_k (k ascending), z_i = y_i / D_i,
 *   x_i = z_i - sum_{k>i} L_ki * x_k (i descending, k ascending).  omega = x[0..2], v = x[3..5].
 * - th2 = omega0*omega0 + omega1*omega1 + omega2*omega2 and th = sqrt(th2).
 *     th < 1e-4:  ca = 1 - th2 / 6 and cb = 0.5 - th2 / 24 (the series);
 *     otherwise:  ca = sin(th) / th and cb = (1 - cos(th)) / th2.
 * - Rr_ij = delta_ij + ca * Wx_ij + cb * (omega_i * omega_j - th2 * delta_ij), with Wx = [omega]x, i.e.
 *   Wx_01 = -omega2, Wx_02 = omega1, Wx_10 = omega2, Wx_12 = -omega0, Wx_20 = -omega1, Wx_21 = omega0.  tr = v.
 * - The new pose of s is the one for which every S above becomes Rr S + tr while view a stays where it is:
 *   [R_a|t_a] [R_s'|t_s']^-1 = [Rr|tr] [R_a|t_a] [R_s|t_s]^-1, that is
 *     M = Rr^T R_a, N = R_a^T M, R_s' = R_s N;
 *     u = t_a - tr, w = Rr^T u - t_a, tn = R_a^T w, t_s' = R_s tn + t_s.
 *   Every matrix product sums its three terms from the left.  R_a and t_a are the INPUT pose of view a, also when view
 *   a is itself updated by the same call.
 * - R_s' and t_s' are rounded to f32 once, at the end, and ok = 1.
 *
 * R is not re-orthonormalised.  No workspace.
 *
 * ok speaks of this call alone.  When system and update are iterated, a view whose last round ends with ok = 0 keeps
 * whatever pose the earlier rounds (each of which may have had ok = 1) left it with, which can be far from any surface:
 * such a pose is not to be used.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for V < 1, B < 0, V > 64, min_count < 0, a negative or NaN min_pivot or damping, or a NULL
 *     system / R / t / R_out / t_out / ok;
 *   CTD_ERR_UNSUPPORTED for B * V >= 2^24;
 *   CTD_ERR_INVALID_ARG for R_out, t_out or ok overlapping any other buffer of the call.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing.
 */
#ifndef CTD_HIP_ICP_H
#define CTD_HIP_ICP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int ctd_depth_normals_f32(const float* depth, const uint8_t* valid, const float* ray, float max_rel, float* normal, int B,
                          int V, int H, int W, int device, void* stream);

size_t ctd_depth_icp_workspace_bytes(int B, int V, int H, int W);

int ctd_depth_icp_system_f32(const float* depth, const uint8_t* valid, const float* normal, const float* ray,
                             const float* K, const float* R, const float* t, const int32_t* target, float max_dist,
                             double* system, float* residual, int64_t* assoc, int B, int V, int H, int W, void* workspace,
                             size_t workspace_bytes, int device, void* stream);

int ctd_depth_icp_update_f32(const double* system, const float* R, const float* t, const int32_t* target, int min_count,
                             double min_pivot, double damping, float* R_out, float* t_out, uint8_t* ok, int B, int V,
                             int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_ICP_H */
