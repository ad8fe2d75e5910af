/* ctd_hip_mesh.h -- the triangle mesh of a truncated signed distance volume of libctd_hip.so: marching cubes over the
 * grid of include/ctd_hip_tsdf.h, as faces that index the surface points of ctd_tsdf_surface_points_f32.  Those points
 * are exactly the vertices of marching cubes (one per zero-crossing grid edge, in ascending src), so the result is a
 * welded, indexed mesh without hashing or vertex merging, and its vertices are bit for bit the points a caller already
 * gets.  verts f32 [n][3] and faces int32 [m][3] of one track are what ctd_mesh_bvh_build_f32 and the render calls of
 * ctd_hip.h take.
 *
 * An addition beside include/ctd_hip.h, ctd_hip_band.h, ctd_hip_warp.h, ctd_hip_band_validity.h, ctd_hip_icp.h and
 * ctd_hip_tsdf.h (none of which includes it; ctd_version() is unchanged): include what you call.  The status codes are
 * those of ctd_hip.h; pointers are device pointers, `device` and `stream` mean what they mean there.  No buffer a call
 * writes may overlap another buffer of the call.  tsdf and weight are f32 [B][nz][ny][nx], x fastest, as in
 * ctd_hip_tsdf.h; min_weight is a finite float > 0.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * The rule
 *
 * Cells, corners and cases.
 * - Cell (i,j,k) of track b exists for i < nx-1, j < ny-1, k < nz-1.
 * - Corner n = dx + 2*dy + 4*dz is voxel (i+dx, j+dy, k+dz).
 * - A cell is meshed when all eight corners are usable under the rule of ctd_hip_tsdf.h: weight >= min_weight and
 *   |tsdf| < 1.
 * - Bit n of the cell's case is set when T_n < 0.  This is the same comparison as the crossing test of the surface
 *   points, so -0.0 and 0 are outside.
 *
 * Edges and vertices.
 * - Edge e = 4*c + r runs along axis c from the r-th corner (ascending n) that has coordinate c equal to 0.
 * - The vertex on a crossing edge is the surface point with src = 3*g(lower corner) + c, g the voxel's index
 *   ((b*nz + k)*ny + j)*nx + i.
 * - In a meshed cell every crossing edge has both ends usable, so that point exists.
 *
 * Segments on the six cell faces.
 * - Take the four corners of a face in cyclic order.  Zero, two or four of the face's edges cross.
 * - Two crossing edges: one segment joins them.
 * - Four crossing edges: at each inside corner, the two face edges that meet there are joined, so the inside corners
 *   are separated.
 * - This depends only on the face's four signs.  Both cells that share a face therefore draw the same segments on it.
 *
 * Loops.
 * - Every crossing edge lies on two faces, so the segments close into loops.
 * - A loop starts at its lowest e.  Its direction is the one for which (v1-v0) x (v2-v0) of its triangles points from
 *   inside (T < 0) towards free space.  That is the side the normals of ctd_tsdf_surface_points_f32 point to.
 * - The loops of a case come in ascending order of their lowest e.
 *
 * Triangles.
 * - A loop q of length m is a fan (q0, q_i, q_{i+1}) for i = 1 .. m-2.
 * - Rotate the loop to the first apex, in loop order from the start, for which no fan diagonal joins two edges of one
 *   cell face.  A diagonal lying in a face can coincide with the neighbour cell's diagonal on an ambiguous face and
 *   break manifoldness.
 *
 * Faces.
 * - Faces are int32, track-local: index 0 is the track's first surface point.
 * - They come in ascending cell order ((b*nz + k)*ny + j)*nx + i, and within a cell in table order.
 * - n_faces_per_track is int64 [B].
 * - Nothing is removed.  Surface points on edges of no meshed cell stay as unreferenced vertices.  A crossing at a
 *   voxel whose tsdf is exactly 0 can yield zero-area triangles.
 *
 * What the rule gives (tools/make_mc_table.py generates the table from it, tests/mesh_ref.py restates it): every one of
 * the 256 cases closes into loops; the longest loop has 7 edges; no case has more than 5 triangles; the table holds 820
 * triangles, and the cases with 0, 1, 2, 3, 4, 5 triangles number 2, 16, 50, 80, 76, 32; an apex other than the loop's
 * start is needed in 18 cases and an admissible apex always exists.  Where every cell around the surface is meshed the
 * faces form a closed, consistently oriented edge-manifold: every directed edge occurs once and its reverse once.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_tsdf_mesh_faces_i32
 *
 * Output faces int32 [capacity][3] and n_faces_per_track int64 [B].  The indices refer to the points that
 * ctd_tsdf_surface_points_f32 returns for the same tsdf, weight and min_weight.  The call writes the first `capacity`
 * faces (the tracks one after the other) and always writes the true n_faces_per_track; entries of faces past the true
 * count are not written.  With faces == NULL it only counts: capacity is ignored.
 *
 * Passes, in the chunking of the surface points (a workgroup takes 256 consecutive voxels of ONE track): the crossing
 * flags and their count per workgroup; one workgroup scans the counts; per voxel with a flag the track-local index of
 * its first point, per cell (a thread takes the cell whose corner 0 is its voxel) the case byte, 0 when not meshed, and
 * the workgroup's number of triangles; one workgroup scans those; the workgroups that have triangles write them at the
 * scanned offsets, a corner's vertex being its voxel's first index plus the number of its lower flags.  No atomics, no
 * flag that another workgroup waits on: the same bits on every run.
 *
 * Workspace: ctd_tsdf_mesh_workspace_bytes(B, nx, ny, nz) bytes, 256-byte aligned.  The call never allocates, and it
 * writes every word of the workspace that it reads, so the workspace may hold anything.
 *
 * Errors, before any HIP call, in this order:
 *   CTD_ERR_INVALID_ARG for nx, ny or nz < 1, B < 0, a min_weight that is not finite and > 0, a NULL tsdf / weight /
 *     n_faces_per_track, or, with faces != NULL, capacity < 0;
 *   CTD_ERR_UNSUPPORTED for nx, ny or nz > 2048, B * nx * ny * nz >= 2^31, 5 * B * nx * ny * nz >= 2^31 (the scanned
 *     face offsets are int32), or B * ceil(nx * ny * nz / 256) >= 2^24;
 *   CTD_ERR_INVALID_ARG for faces, n_faces_per_track or the workspace overlapping any other buffer of the call (faces
 *     counts with min(capacity, 5 * B * nx * ny * nz) entries: there are no more triangles);
 *   CTD_ERR_WORKSPACE for a NULL, short or misaligned workspace.
 * B == 0 (with valid arguments otherwise) is CTD_OK and touches nothing, the workspace included.  The workspace query
 * returns 0 for shapes that one of the first two errors rejects and for B == 0.
 *
 * ---------------------------------------------------------------------------------------------------------------------
 * ctd_tsdf_mesh_case
 *
 * Host only; makes no HIP call.  Writes the triangles of case mc_case as edge ids, three per triangle in table order,
 * into edges[0 .. 3*count-1], and -1 into the rest of edges[15]; returns the number of triangles.  Outside 0 .. 255, or
 * with edges == NULL, it returns -1 and writes nothing.
 */
#ifndef CTD_HIP_MESH_H
#define CTD_HIP_MESH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t ctd_tsdf_mesh_workspace_bytes(int B, int nx, int ny, int nz);

int ctd_tsdf_mesh_faces_i32(const float* tsdf, const float* weight, float min_weight, int32_t* faces,
                            int64_t* n_faces_per_track, int64_t capacity, int B, int nx, int ny, int nz, void* workspace,
                            size_t workspace_bytes, int device, void* stream);

int ctd_tsdf_mesh_case(int mc_case, int32_t* edges /* [15] */);

#ifdef __cplusplus
}
#endif

#endif /* CTD_HIP_MESH_H */
