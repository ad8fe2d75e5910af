/* ctd_hip_mesh_simplify.h -- mesh simplification of libctd_hip.so: uniform-grid vertex clustering (Rossignac-Borrel; the
 * out-of-core scheme of Lindstrom 2000) with every cluster's vertex placed at the minimum of its summed plane quadrics
 * (Garland-Heckbert), the quadrics weighted by area squared as Lindstrom does, so no square root is taken.  A regulariser
 * pulls the solve toward the cluster's mean, so the usual cluster, a flat one with a rank-1 quadric, is well posed
 * without an eigen-decomposition.  verts f32 [n_verts][3] and faces int32 [n_faces][3] are one track of a mesh.TsdfMesh;
 * face_offsets and face_ids are the incident-face rows of a meshsmooth.MeshAdjacency of these faces.
 *
 * An addition beside the other headers of include/ (none of which includes it; ctd_version() is unchanged): include
 * what you call.  The status codes are those of ctd_hip.h; pointers are device pointers, `device` and `stream` mean what
 * they mean there.  No buffer a call writes may overlap another buffer of the call.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * 1. Validity.  As in the smoothing header.  A face is valid when both of these hold:
 * - Its three indices lie in [0, n_verts).
 * - Its three indices are pairwise different.
 * Out-of-range indices are never dereferenced.
 *
 * 2. Cell.  The cell of vertex v is i_k = floorf((x_k - origin_k) / cell) for k = 0, 1, 2, computed in f32 with IEEE
 * sub, div and floor.
 * - v is clusterable when it is used by a valid face and all three i_k are finite and in [0, 2^20).
 *   CTD_MESH_SIMPLIFY_MAX_CELLS_PER_AXIS = 1048576.
 * - A NaN or infinite coordinate, or a cell out of range, makes the vertex unclusterable.
 * - Every face that uses an unclusterable vertex is dropped and counted.  It is never an error.
 *
 * 3. Cluster.  A cluster is the set of clusterable vertices of one cell.  Its leader is its smallest vertex index.
 *
 * 4. Vertex quadric.  The quadric of a clusterable vertex v is Q_v = (A_v [6], b_v [3]), all in f64, from 0.
 * - The row of v is empty unless 0 <= face_offsets[v] <= face_offsets[v+1] <= n_incident.
 * - The sum runs over the entries of the row in the row's order, which is ascending face index in an undamaged
 *   adjacency.
 * - An entry outside [0, n_faces), a face that is not valid, and a face whose corners are not all clusterable is never
 *   dereferenced further and adds nothing.
 * - Per corner of the face, in its stored order (p0,p1,p2): q = (double)p - (double)origin.
 * - e1 = q1 - q0; e2 = q2 - q0.
 * - cx = e1y*e2z - e1z*e2y; cy = e1z*e2x - e1x*e2z; cz = e1x*e2y - e1y*e2x.  |c| is twice the face's area.
 * - d = -((cx*q0x + cy*q0y) + cz*q0z).
 * - A00 += cx*cx; A01 += cx*cy; A02 += cx*cz; A11 += cy*cy; A12 += cy*cz; A22 += cz*cz.
 * - b0 += d*cx; b1 += d*cy; b2 += d*cz.
 *
 * 5. Cluster quadric and mean.
 * - The cluster's quadric (A, b) is the sum of Q_v over its members in ascending vertex index, from 0.
 * - s is the sum of the members' q = (double)p - (double)origin, in the same order, from 0.
 * - mean = s / (double)count (three IEEE divisions).
 *
 * 6. Placement.  All in f64.
 * - lambda = reg * ((A00 + A11) + A22).
 * - r0 = -(((A00*mean0 + A01*mean1) + A02*mean2) + b0); r1 = -(((A01*mean0 + A11*mean1) + A12*mean2) + b1);
 *   r2 = -(((A02*mean0 + A12*mean1) + A22*mean2) + b2).
 * - m00 = A00 + lambda; m11 = A11 + lambda; m22 = A22 + lambda; m01 = A01; m02 = A02; m12 = A12.
 * - c00 = m11*m22 - m12*m12; c01 = m02*m12 - m01*m22; c02 = m01*m12 - m02*m11; c11 = m00*m22 - m02*m02;
 *   c12 = m01*m02 - m00*m12; c22 = m00*m11 - m01*m01.
 * - det = (m00*c00 + m01*c01) + m02*c02.
 * - delta0 = ((c00*r0 + c01*r1) + c02*r2) / det; delta1 = ((c01*r0 + c11*r1) + c12*r2) / det;
 *   delta2 = ((c02*r0 + c12*r1) + c22*r2) / det.
 * - x = mean + delta.
 * - lo_k = (double)i_k * (double)cell, with i_k the cell of the cluster.
 * - The cluster falls back to x = mean, and is counted, when lambda is not finite or not > 0, when det is not finite or
 *   not > 0, when any x_k is not finite, or when any x_k lies outside
 *   [lo_k - (double)cell * 0.5, lo_k + (double)cell * 1.5].
 * - The output vertex is (float)(x + (double)origin).
 * - Only IEEE + - * /, compares and conversions are used.  There is no FMA.
 *
 * 7. Kept faces.
 * - A valid face with all corners clusterable maps to its three clusters.
 * - It is collapsed (dropped and counted) when two of them are equal.
 * - With drop_duplicates, of all non-collapsed faces with the same set of three clusters, the one with the smallest
 *   face index is kept.  Order and winding do not matter in the comparison.  The others are counted as duplicates.
 *
 * 8. Output order.
 * - Kept faces keep their order and their winding.
 * - A cluster is emitted when a kept face uses it.
 * - Emitted clusters are numbered in ascending order of their leaders.
 *
 * 9. Outputs.  verts_out f32 [n'][3], the placed vertices; leader int32 [n'], the leader of each emitted cluster;
 * vert_cluster int32 [n_verts], the output index of the vertex's cluster, or -1; faces_out int32 [k][3], the kept faces
 * over the output indices; face_index int32 [k], the old face index of each kept face; counts int64 [8]: n'; k; the
 * clusters before the drop; the faces dropped as invalid or unclusterable; the collapsed faces; the duplicate faces; the
 * mean fallbacks among the emitted clusters; the largest cluster.
 *
 * Capacities.  The call writes the first min(n', cap_verts) rows of verts_out and leader and the first min(k, cap_faces)
 * rows of faces_out and face_index; it always writes vert_cluster and the true counts; nothing is written past a
 * capacity or past a true count.  n' <= n_verts and k <= n_faces.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_simplify_f32
 *
 * Passes (a workgroup takes 256 consecutive faces or vertices; scans and prefixes are those of the other mesh calls).
 * Cells to clusters: an open-addressing table of 64-bit cell keys, (i_0 << 40) | (i_1 << 20) | i_2, with linear probing;
 * a key is inserted by a 64-bit integer compare-and-swap and the slot's leader is an integer min over the vertices that
 * found the key.  No output depends on where a key landed: a cluster is known by its leader, and the output numbers come
 * from a scan over the flags of the emitted leaders.  The table has table(n_verts) slots, the smallest power of two
 * >= max(2 * n_verts, 256), so a probe always ends.  Members by cluster: count (one integer atomic add at the leader),
 * scan, fill (a slot drawn from the leader's counter by an integer atomic), then every row sorted ascending: at most 16
 * members by ONE LANE, longer rows by THE WORKGROUP, whatever their length (over a copy in LDS where the row fits).  The
 * leaders of the longer rows are first put on a list, a range of it per workgroup drawn by one integer atomic add, and
 * workgroups stride over that list, since long rows come in runs of neighbouring leaders; the order of the list reaches
 * no output.  Quadrics: one thread per vertex; then one thread per cluster of at most 16 members, and a workgroup for a
 * longer one, which stages 256 members' summands in LDS at a time and lets 12 threads add them in the row's order, one
 * component each, so the association is that of the rule.  Duplicate faces: a second table of table(n_faces) 32-bit slots
 * that hold a face index; two faces are equal when their sorted cluster triples are equal; an empty slot is taken by a
 * compare-and-swap and an equal face joins by an integer min, so a slot's triple never changes and the smallest index
 * wins.  Kept faces and emitted clusters are counted per workgroup, scanned by one workgroup and scattered.
 * Atomics are integer compare-and-swap, min, max, add and subtract only, whose final results do not depend on their
 * order.  No floating-point atomic.  No flag that another workgroup waits on: the same bits on every run.
 *
 * Workspace: ctd_mesh_simplify_workspace_bytes(n_verts, n_faces) bytes, 256-byte aligned.  The call never allocates, and
 * it writes every word of the workspace that it reads, so the workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for a negative n_verts, n_faces, n_incident, cap_verts or cap_faces, a NULL verts, faces,
 *     face_offsets, face_ids, verts_out, leader, vert_cluster, faces_out, face_index or counts (also at size 0), an origin
 *     that is not finite, a cell that is not finite or not > 0, a reg that is not finite or < 0;
 *   CTD_ERR_UNSUPPORTED for 6 * n_faces >= 2^31, n_verts >= 2^31, n_incident >= 2^31, or ceil(n_faces / 256) or
 *     ceil(n_verts / 256) >= 2^24;
 *   CTD_ERR_INVALID_ARG for an output or the workspace overlapping any other buffer of the call (verts_out and leader
 *     count with min(cap_verts, n_verts) rows, faces_out and face_index with min(cap_faces, n_faces): there are no more);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * Empty inputs (with valid arguments otherwise) are CTD_OK with zero counts.  The workspace query returns 0 for sizes
 * that one of the first two errors rejects.
 */
#ifndef CTD_HIP_MESH_SIMPLIFY_H
#define CTD_HIP_MESH_SIMPLIFY_H

#include <stddef.h>
#include <stdint.h>

#include "ctd_hip.h" /* the status codes */

#define CTD_MESH_SIMPLIFY_MAX_CELLS_PER_AXIS 1048576

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces);

int ctd_mesh_simplify_f32(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                          const int32_t* face_offsets, const int32_t* face_ids, int64_t n_incident, float origin_x,
                          float origin_y, float origin_z, float cell, double reg, int drop_duplicates, float* verts_out,
                          int32_t* leader, int64_t cap_verts, int32_t* vert_cluster, int32_t* faces_out, int32_t* face_index,
                          int64_t cap_faces, int64_t* counts /* [8] */, void* workspace, size_t workspace_bytes, int device,
                          void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_SIMPLIFY_H */
