/* ctd_hip_mesh_smooth.h -- the connectivity by vertex of an indexed triangle mesh (incident faces, one-rings, boundary and
 * non-manifold edges), Taubin lambda|mu smoothing over the one-rings, and area-weighted vertex normals, of
 * libctd_hip.so.  faces int32 [m][3] over n_verts vertices is what ctd_tsdf_mesh_faces_i32 of include/ctd_hip_mesh.h
 * writes for one track and what ctd_mesh_clean_i32 of include/ctd_hip_mesh_clean.h compacts.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h, ctd_hip_icp.h,
 * ctd_hip_tsdf.h, ctd_hip_mesh.h, ctd_hip_mesh_clean.h, ctd_hip_mesh_dist.h and ctd_hip_mesh_color.h (none of which
 * includes it; ctd_version() is unchanged): include what you call.  The status codes are those of ctd_hip.h; pointers are
 * device pointers, `device` and `stream` mean what they mean there.  No buffer a call writes may overlap another buffer
 * of the call.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * Valid faces.  As in ctd_hip_mesh_clean.h without drop_degenerate.  A face is valid when both of these hold:
 * - Its three indices lie in [0, n_verts).
 * - Its three indices are pairwise different.
 * Out-of-range indices are never dereferenced.
 *
 * Incidence.  The incident faces of vertex i are the valid faces that use i, in ascending face index.
 *
 * One-ring.
 * - For every valid face (a,b,c), the row of a receives b and c, the row of b receives a and c, and the row of c receives
 *   a and b.
 * - The one-ring of i is the set of values in its row, ascending, each once.
 * - The multiplicity of j in row i is the number of valid faces that use the edge {i,j}.
 *
 * Edges.
 * - An edge is a pair i < j with j in the ring of i.
 * - A boundary edge has multiplicity 1.
 * - A non-manifold edge has multiplicity > 2.
 *
 * Vertex flags (uint8), one bit each:
 * - CTD_MESH_VERT_REFERENCED (1): the ring is not empty.
 * - CTD_MESH_VERT_BOUNDARY (2): the vertex is an end of a boundary edge.
 * - CTD_MESH_VERT_NONMANIFOLD (4): the vertex is an end of a non-manifold edge.
 *
 * Counts (int64 [6]): nnz, which is 2 x the number of edges; the number of edges; the number of boundary edges; the
 * number of non-manifold edges; max_incident, the largest number of valid faces at one vertex; the number of valid faces.
 *
 * Bounded work.  CTD_MESH_ADJ_MAX_INCIDENT = 1024.  No lane, wavefront or workgroup does work that grows quadratically
 * in a row longer than that.  If max_incident exceeds the cap, the call still returns CTD_OK and always writes the true
 * counts; all other outputs are then unspecified and must not be used.
 *
 * All of this is integer work, so every output is exact and the same on every run.
 *
 * Smoothing pass with factor f.  Everything is f32, uncontracted, in the written association.
 * - For vertex i, a row is empty unless 0 <= offsets[i] <= offsets[i+1] <= nnz.
 * - A row entry outside [0, n_verts) is never dereferenced, adds nothing, and does not count.
 * - Let d be the number of counted entries.
 * - If d == 0, or fix_boundary is set and the vertex has BOUNDARY set, then out = in, bit for bit.
 * - Otherwise, per component c: s_c = 0; then s_c = s_c + x[j]_c over the ring in ascending order (the order of the row);
 *   m_c = s_c / (float)d (IEEE division); out_c = x_c + f * (m_c - x_c).
 * - One iteration is a pass with lambda over all vertices, then a pass with mu over the result.
 * - With mu == 0 the second pass is not run.
 * - With iters == 0 the output is a copy.
 * - Passes ping-pong between the output and the workspace.  No pass reads what it writes.
 * - A NaN or infinite coordinate spreads to its ring and nowhere else per pass.
 *
 * Vertex normals.
 * - For vertex i, a row of face_ids is empty unless 0 <= face_offsets[i] <= face_offsets[i+1] <= n_incident.
 * - A face id outside [0, n_faces), and a face with an index outside [0, n_verts), is never dereferenced and adds nothing.
 * - acc = 0.  Then over the incident faces in ascending order (the order of the row), with the face's stored corner order
 *   (v0,v1,v2): e1 = v1 - v0; e2 = v2 - v0; cx = e1y*e2z - e1z*e2y; cy = e1z*e2x - e1x*e2z; cz = e1x*e2y - e1y*e2x;
 *   acc = acc + c.  This is area weighting: |c| is twice the face's area.
 * - len = sqrtf((ax*ax + ay*ay) + az*az).
 * - normal = acc / len (three divisions) when len > 0 and len is finite.  Otherwise the normal is three NaNs.
 * - So an unreferenced vertex has a NaN normal, as the view-colour kernel of ctd_hip_mesh_color.h expects.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_adjacency_i32
 *
 * Outputs offsets int32 [n_verts+1] and neighbors int32 [cap_neighbors] (the one-rings in compressed rows: the ring of i
 * is neighbors[offsets[i] .. offsets[i+1]); at most 6 * n_faces entries), face_offsets int32 [n_verts+1] and face_ids
 * int32 [cap_face_ids] (the incident faces, likewise; at most 3 * n_faces entries), vflags uint8 [n_verts] and counts
 * int64 [6].  The call writes the first cap_neighbors entries of neighbors and the first cap_face_ids entries of face_ids,
 * and always writes offsets, vflags and the true counts; entries past the true counts are not written.  Each of
 * neighbors, face_offsets and face_ids may be NULL and is then not written (its capacity is ignored).
 *
 * Passes (a workgroup takes 256 consecutive faces or vertices): per valid face one integer atomic add at each of its
 * vertices' counters; per 256 vertices the sum and the maximum of their counters; one workgroup takes the largest of the
 * maxima, max_incident, and one workgroup scans the sums; every vertex its face_offsets, and the number of valid faces
 * is a third of their total; per valid face and corner a slot of the vertex's row drawn from its counter by an integer
 * atomic, where the face id and the two other corners go (in an order that depends on the atomics); then every row is
 * sorted, which removes that order: a vertex with at most 16 incident faces by ONE LANE, an insertion sort over a
 * copy of the row in LDS; every longer row by THE WORKGROUP of its 256 vertices, one row after the other, a bitonic
 * network over the row in global memory (n log^2 n compare-exchanges for a row of n, whatever its length, so rows past
 * the cap cost no quadratic work either).  In a sorted row, an entry that differs from the one before starts a run, and
 * the run's length capped at 3 is read from the two entries after it: the ring's size, the flags and the boundary and
 * non-manifold edges (counted at the smaller end; one 64-bit integer add per workgroup each) need nothing else.  One
 * workgroup scans the ring sizes of the 256-vertex chunks; every vertex its offsets; the run starts of every row go to
 * neighbors below the capacity (one lane, or the workgroup with a prefix sum for the longer rows), and the sorted face
 * ids are copied to face_ids.  Atomics are integer add, subtract and or only, whose final results do not depend on their
 * order.  No flag that another workgroup waits on: the same bits on every run.
 *
 * ctd_mesh_smooth_f32
 *
 * Output verts_out f32 [n_verts][3]: verts f32 [n_verts][3] after iters iterations by the rule, over offsets int32
 * [n_verts+1], neighbors int32 [nnz] and vflags uint8 [n_verts] of ctd_mesh_adjacency_i32 (any values: what the rule
 * does not accept is skipped).  vflags may be NULL when fix_boundary == 0 and is not read then.  One launch per pass,
 * thread = vertex.
 *
 * ctd_mesh_vertex_normals_f32
 *
 * Output normals f32 [n_verts][3] by the rule, over face_offsets int32 [n_verts+1] and face_ids int32 [n_incident] of
 * ctd_mesh_adjacency_i32 (any values, as above).  One launch, thread = vertex.  No workspace.
 *
 * Workspace: ctd_mesh_adjacency_workspace_bytes(n_verts, n_faces) and ctd_mesh_smooth_workspace_bytes(n_verts) bytes,
 * 256-byte aligned.  The calls never allocate, and they write every word of the workspace that they read, so the
 * workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for a negative n_verts, n_faces, nnz or n_incident, a NULL faces, offsets, vflags (adjacency),
 *     counts, verts, verts_out, neighbors (smoothing), normals, face_offsets or face_ids (normals) (also at size 0), a
 *     NULL vflags with fix_boundary != 0, a negative capacity of an output that is not NULL, iters outside [0, 1024],
 *     lambda not finite or outside (0, 1], mu not finite or outside [-2, 0];
 *   CTD_ERR_UNSUPPORTED for 6 * n_faces >= 2^31, n_verts >= 2^31, nnz >= 2^31, n_incident >= 2^31, or ceil(n_faces / 256)
 *     or ceil(n_verts / 256) >= 2^24;
 *   CTD_ERR_INVALID_ARG for an output or the workspace overlapping any other buffer of the call (neighbors counts with
 *     min(cap_neighbors, 6 * n_faces) entries, face_ids with min(cap_face_ids, 3 * n_faces): there are no more);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * Empty inputs (with valid arguments otherwise) are CTD_OK; the adjacency of no face has zero counts, zero offsets and
 * zero flags.  The workspace queries return 0 for sizes that one of the first two errors rejects.
 */
#ifndef CTD_HIP_MESH_SMOOTH_H
#define CTD_HIP_MESH_SMOOTH_H

#include <stddef.h>
#include <stdint.h>

#include "ctd_hip.h" /* the status codes */

#define CTD_MESH_ADJ_MAX_INCIDENT 1024
#define CTD_MESH_VERT_REFERENCED 1
#define CTD_MESH_VERT_BOUNDARY 2
#define CTD_MESH_VERT_NONMANIFOLD 4

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_mesh_adjacency_workspace_bytes(int64_t n_verts, int64_t n_faces);

int ctd_mesh_adjacency_i32(const int32_t* faces, int64_t n_verts, int64_t n_faces, int32_t* offsets, int32_t* neighbors,
                           int64_t cap_neighbors, int32_t* face_offsets, int32_t* face_ids, int64_t cap_face_ids,
                           uint8_t* vflags, int64_t* counts /* [6] */, void* workspace, size_t workspace_bytes, int device,
                           void* stream);

size_t ctd_mesh_smooth_workspace_bytes(int64_t n_verts);

int ctd_mesh_smooth_f32(const float* verts, int64_t n_verts, const int32_t* offsets, const int32_t* neighbors, int64_t nnz,
                        const uint8_t* vflags, int iters, float lambda, float mu, int fix_boundary, float* verts_out,
                        void* workspace, size_t workspace_bytes, int device, void* stream);

int ctd_mesh_vertex_normals_f32(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                const int32_t* face_offsets, const int32_t* face_ids, int64_t n_incident, float* normals,
                                int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_SMOOTH_H */
