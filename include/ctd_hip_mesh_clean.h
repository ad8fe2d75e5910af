/* ctd_hip_mesh_clean.h -- mesh clean-up of libctd_hip.so: the connected components of an indexed triangle mesh, the
 * removal of small components, of faces with coincident vertices and of unreferenced vertices, and the compaction of
 * what is left.  faces int32 [m][3] over n_verts vertices is what ctd_tsdf_mesh_faces_i32 of include/ctd_hip_mesh.h
 * writes for one track and what ctd_mesh_bvh_build_f32 of include/ctd_hip.h takes.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h, ctd_hip_icp.h,
 * ctd_hip_tsdf.h and ctd_hip_mesh.h (none of which includes it; ctd_version() is unchanged): include what you call.
 * The status codes are those of ctd_hip.h; pointers are device pointers, `device` and `stream` mean what they mean
 * there.  No buffer a call writes may overlap another buffer of the call.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * Inputs: faces int32 [m][3], n_verts, and optionally verts f32 [n][3].
 *
 * Valid faces.  A face is valid when all of these hold:
 * - Its three indices lie in [0, n_verts).
 * - Its three indices are pairwise different.
 * - With drop_degenerate, no two of its vertices have equal positions.  Positions are equal when x, y and z each
 *   compare == as f32.  So -0.0 equals 0, and a NaN coordinate equals nothing.
 * Out-of-range indices are never dereferenced.
 *
 * Components.
 * - Two valid faces belong to one component when a chain of valid faces links them, each sharing a vertex index with
 *   the next.  Vertex connectivity is by index, not by position.
 * - A component's label is the smallest vertex index any of its faces uses.
 * - A component's size is the number of its valid faces.
 * - An invalid face has label -1 and size 0.
 *
 * Kept faces.  A face is kept when all of these hold:
 * - It is valid.
 * - Its size is at least min_faces.
 * - With keep_largest, its component is the one of largest size.  On a tie that is the one with the smallest label.
 *   min_faces still applies to it.
 *
 * Kept vertices.  A vertex is kept when a kept face uses it.
 * - Kept vertices keep their order.  A vertex's new index is the number of kept vertices with a smaller old index.
 * - Kept faces keep their order and their winding, with the indices remapped.
 * - Nothing else changes.  Coincident vertices are not welded.  Dropping zero-area faces can therefore open a
 *   combinatorial hole of zero size in an otherwise closed mesh.
 *
 * All of this is integer work (the position test is an exact comparison), so every output is exact and the same on
 * every run.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_mesh_components_i32
 *
 * Outputs label int32 [m], size int32 [m] (per face, by the rule) and n_components int64 [1], the number of components.
 * verts may be NULL when drop_degenerate == 0 and is not read then.
 *
 * ctd_mesh_clean_i32
 *
 * Outputs faces_out int32 [cap_faces][3] (the kept faces, remapped), face_index int32 [cap_faces] (the old index of each
 * kept face), vert_index int32 [cap_verts] (the old index of each kept vertex) and counts int64 [4]: kept vertices, kept
 * faces, components, components kept.  The call writes the first cap_faces kept faces and their face_index, the first
 * cap_verts entries of vert_index, and always writes the true counts; entries past the true counts are not written.
 * Each of faces_out, face_index and vert_index may be NULL and is then not written (its capacity is ignored); with all
 * three NULL the call only counts.  The gather of positions, normals or colours of the kept vertices is an index select
 * by vert_index on the caller's side: bit-exact, no kernel.
 *
 * Passes (a workgroup takes 256 consecutive faces or vertices): every vertex its own parent; per valid face the unions
 * (v0,v1) and (v0,v2), by integer atomic min, so that the root of a set is its smallest index whatever order the atomics
 * land in; per face the root, and the size at the root by one integer atomic add per run of equal roots inside a
 * wavefront; per vertex that is a root of a counted set the number of components and, with keep_largest, one 64-bit
 * integer atomic max over the key (size, inverted label); per face the kept flag, a byte store of 1 at its vertices and
 * the workgroup's count; per 256 vertices their count; one workgroup scans each list of counts; the kept vertices and
 * faces go to the scanned offsets, the faces remapped through the vertices' new indices.  Atomics are integer min, add
 * and max only, whose results do not depend on their order.  No flag that another workgroup waits on: the same bits on
 * every run.
 *
 * Workspace: ctd_mesh_clean_workspace_bytes(n_verts, n_faces) bytes, 256-byte aligned, for either call.  The calls never
 * allocate, and they write every word of the workspace that they read, so the workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for n_verts < 0, n_faces < 0, min_faces < 1, a NULL faces (also at n_faces == 0), a NULL label /
 *     size / n_components or counts, a NULL verts with drop_degenerate != 0, or a negative capacity of an output that is
 *     not NULL;
 *   CTD_ERR_UNSUPPORTED for 3 * n_faces >= 2^31, n_verts >= 2^31, or ceil(n_faces / 256) or ceil(n_verts / 256) >= 2^24;
 *   CTD_ERR_INVALID_ARG for an output or the workspace overlapping any other buffer of the call (faces_out and face_index
 *     count with min(cap_faces, n_faces) entries, vert_index with min(cap_verts, n_verts): there are no more);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * n_faces == 0 and n_verts == 0 (with valid arguments otherwise) are CTD_OK and write zero counts.  The workspace query
 * returns 0 for sizes that one of the first two errors rejects.
 */
#ifndef CTD_HIP_MESH_CLEAN_H
#define CTD_HIP_MESH_CLEAN_H

#include <stddef.h>
#include <stdint.h>

#include "ctd_hip.h" /* the status codes */

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_mesh_clean_workspace_bytes(int64_t n_verts, int64_t n_faces);

int ctd_mesh_components_i32(const int32_t* faces, const float* verts, int64_t n_verts, int64_t n_faces, int drop_degenerate,
                            int32_t* label, int32_t* size, int64_t* n_components, void* workspace, size_t workspace_bytes,
                            int device, void* stream);

int ctd_mesh_clean_i32(const int32_t* faces, const float* verts, int64_t n_verts, int64_t n_faces, int drop_degenerate,
                       int min_faces, int keep_largest, int32_t* faces_out, int32_t* face_index, int64_t cap_faces,
                       int32_t* vert_index, int64_t cap_verts, int64_t* counts /* [4] */, void* workspace,
                       size_t workspace_bytes, int device, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_CLEAN_H */
