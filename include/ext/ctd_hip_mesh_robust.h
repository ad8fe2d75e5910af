/* ctd_hip_mesh_robust.h -- robust point-to-mesh ICP of libctd_hip.so: the system of ctd_hip_mesh_register.h with an
 * M-estimator weight per point (Huber or Tukey), with matches on the rim of an open mesh rejected, and with matches
 * whose normals disagree rejected; and the per-face table that says which features of a face lie on the rim.  The remedy
 * for what the plain system cannot cope with on the meshes a reconstruction really produces: outliers, and a point set
 * that overhangs an open surface and is pulled towards its boundary.  The update stays ctd_mesh_register_update_f32.
 *
 * An addition beside include/ctd_hip.h and the headers next to it (none of which includes it; ctd_version() is
 * unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device`
 * and `stream` mean what they mean there.  No buffer a call writes may overlap another buffer of the call.
 *
 * What it does not do.  No global registration (ctd_hip_mesh_global.h finds the starts) and no scale, as
 * ctd_hip_mesh_register.h.  It does not estimate the
 * robust scale: that is a median, which the caller computes between rounds (meshrobust.robust_scale) and hands over
 * on the device.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_face_rim_u8
 *
 * Inputs: faces int32 [n_faces][3] over n_verts vertices; face_offsets int32 [n_verts+1] and face_ids int32 [n_incident],
 * the incident-face rows, and vflags u8 [n_verts], all three of a meshsmooth.MeshAdjacency of these faces (the adjacency
 * call of include/ctd_hip_mesh_smooth.h writes them).  Output: rim u8 [n_faces].
 *
 * A face is valid as in ctd_hip_mesh_smooth.h: its indices lie in [0, n_verts) and are pairwise different.  For a valid
 * face with the stored corners (a, b, c):
 *
 * - bits 0, 1, 2 are set when vflags[a], vflags[b], vflags[c] have CTD_MESH_VERT_BOUNDARY (2) set;
 * - bits 3, 4, 5 are set when the edges ab, ac, bc have multiplicity 1.  The multiplicity of the edge {i, j} is found by
 *   the walk that the pseudonormal of ctd_hip_mesh_sdf.h makes: over the row of min(i, j), the number of valid faces
 *   with min(i, j) at one corner and max(i, j) at another.  A non-manifold edge (more than 2) is not rim, and neither
 *   is an edge that its row does not hold;
 * - bits 6 and 7 are 0.
 *
 * The bit numbers are the feature codes 0 .. 5 of ctd_hip_mesh_sdf.h, so that `rim[f] >> feature & 1` says whether the
 * closest point of a query lies on the boundary of the surface.  An invalid face gets 0.
 *
 * Bounds, as in ctd_hip_mesh_sdf.h: the rows are any values.  A row is empty unless
 * 0 <= face_offsets[i] <= face_offsets[i+1] <= n_incident; a face id outside [0, n_faces) and a vertex index outside
 * [0, n_verts) are never dereferenced.
 *
 * One launch, one thread per face, at most three rows walked; integer work, no atomics, the same bits on every run.
 * It is called once per mesh.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_faces < 0, n_verts < 0 or n_incident < 0; for n_faces > 2^28; for a NULL faces, face_offsets,
 *     face_ids, vflags or rim when n_faces > 0; for rim overlapping any other buffer of the call.
 * n_faces == 0 is CTD_OK and does nothing.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_robust_system_f32
 *
 * The arguments of ctd_mesh_register_system_f32, with the same limits, the same hint, the same 29-entry layout and
 * K <= 64 poses per launch, and:
 *
 * - kernel: 0 (none), 1 (Huber) or 2 (Tukey's biweight);
 * - scale f32 [K], ON THE DEVICE: the kernel's c for each pose.  NULL only with kernel 0, which does not read it.  A
 *   device pointer lets a loop estimate the scale from one round's residuals and use it in the next without a host
 *   synchronisation;
 * - rim u8 [n_faces] as ctd_mesh_face_rim_u8 writes it, or NULL: no rim rejection;
 * - normals f32 [n_points][3], one per point in the points' frame, or NULL: no normal gate; min_cos, a float in [-1, 1].
 *
 * All f32 arithmetic is in the written association and uncontracted.  S, the query (d2, f, q) with its feature, D, the
 * face normal n with its length l, e and J are those of ctd_hip_mesh_register.h, word for word.  Per point and pose, the
 * first of these that applies gives the point's status, and a status other than 0 gates the point away:
 *
 * 1. No face qualifies (f == -1): status 1.
 * 2. The face normal n is computed for metric 0, and for metric 1 when `normals` is given.  Unless l > 0 and l is
 *    finite: status 2.
 * 3. `rim` is given, the query's feature lies in 0 .. 5 and bit `feature` of rim[f] is set: status 3.
 * 4. `normals` is given: with (a0, a1, a2) = normals[i], m_j = (R_k[j][0] * a0 + R_k[j][1] * a1) + R_k[j][2] * a2 for
 *    j = 0, 1, 2 (the point's normal under the pose) and cosang = (m0 * n0 + m1 * n1) + m2 * n2.  Unless
 *    cosang >= min_cos (a NaN fails): status 4.
 * 5. r = fabsf(e) for metric 0 and sqrtf(d2) for metric 1; c = scale[k].
 *    - kernel 0: w = 1, and c is not read.
 *    - Otherwise, unless c > 0 (a NaN fails; +inf is allowed): status 5, for every point of the pose that came this far.
 *    - Huber: w = 1 when r <= c, else w = c / r.
 *    - Tukey: when r < c, u = r / c, v = 1 - u * u, w = v * v; otherwise status 5.
 *    - w == 0: status 5.
 * 6. Otherwise status 0, and every term that the plain system adds is added as (double)w * ((double)x * (double)y): the
 *    inner product of two f32 factors is exact, the one multiplication by w rounds once in f64, and the sums run in the
 *    fixed order of ctd_hip_mesh_register.h.  [27] is sum w e e, [28] the number of points with status 0 (not the sum
 *    of the weights).  For metric 1 the point's one weight multiplies all three rows.
 * 7. A point with a status other than 0 adds +0.0 to every sum, which changes none.
 *
 * With kernel 0, rim == NULL and normals == NULL the 29 entries are those of ctd_mesh_register_system_f32 bit for bit:
 * the same points take part, and 1.0 * x is exact.
 *
 * Outputs, each of the maps may be NULL:
 *
 * - system f64 [K][29], the layout of ctd_mesh_register_system_f32.
 * - face int32 [K][n_points]: the query's f, -1 only where no face qualified.  It is NOT reset for a point that a later
 *   step gated away: it stays the next round's hint.  It must not overlap this round's hint.
 * - residual f32 [K][n_points]: e (metric 0) or sqrtf(d2) (metric 1) for status 0, NaN otherwise.
 * - weight f32 [K][n_points]: w for status 0, 0 otherwise.
 * - status int8 [K][n_points]: 0 .. 5 as above.
 * - closest f32 [K][n_points][3]: q as the query gives it (three NaNs where no face qualified), whatever the status.
 *
 * Launches: those of ctd_mesh_register_system_f32 -- pose, query (here with the recorded branch switched on, which
 * changes no bit of d2, f and q), system, finish -- and in the system kernel one byte gathered per point from rim.
 * Workspace: ctd_mesh_robust_workspace_bytes(K, n_points) bytes, 256-byte aligned: that of the plain call and the
 * feature byte of every posed point.  The call never allocates, and it writes every word of the workspace that it
 * reads.  The query returns 0 for arguments that the first three errors reject and for n_points == 0.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_points < 0, n_verts < 0 or n_faces < 0; for K < 1 or K > 64; for 3 * K * n_points >= 2^31 or
 *     n_faces > 2^28; for a metric other than 0 and 1; for a kernel other than 0, 1 and 2; for a max_d2 that is NaN or
 *     negative; for a min_cos that is NaN or outside [-1, 1]; for a NULL R, t or system, a NULL scale when kernel != 0, a
 *     NULL points when n_points > 0, a NULL faces when n_faces > 0, or a NULL verts when n_faces > 0 and n_verts > 0; for a
 *     bvh that is not 16-byte aligned; for system, face, residual, weight, status, closest or the workspace overlapping
 *     any other buffer of the call, hint, scale, rim and normals included;
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace (unless n_points == 0, which needs none).
 * Then: CTD_ERR_INVALID_ARG for a bvh that is not a tree of n_faces faces; CTD_ERR_UNSUPPORTED for a tree deeper than
 * the traversal stack -- call again with bvh == NULL.
 * n_points == 0 or n_faces == 0 is CTD_OK: systems of zeros, and for n_faces == 0 face -1, residual NaN, weight 0,
 * status 1 and closest NaN.
 */
#ifndef CTD_HIP_MESH_ROBUST_H
#define CTD_HIP_MESH_ROBUST_H

#include "../ctd_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int ctd_mesh_face_rim_u8(const int* faces, int n_faces, int n_verts, const int32_t* face_offsets, const int32_t* face_ids,
                         int64_t n_incident, const uint8_t* vflags, uint8_t* rim, int device, void* stream);

size_t ctd_mesh_robust_workspace_bytes(int K, int n_points);

int ctd_mesh_robust_system_f32(const float* points, int n_points, const float* R, const float* t, int K,
                               const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh, int metric,
                               float max_d2, const int32_t* hint, int kernel, const float* scale, const uint8_t* rim,
                               const float* normals, float min_cos, double* system, int32_t* face, float* residual,
                               float* weight, int8_t* status, float* closest, void* workspace, size_t workspace_bytes,
                               int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_ROBUST_H */
