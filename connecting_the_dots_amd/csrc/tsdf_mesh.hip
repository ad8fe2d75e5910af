// tsdf_mesh.hip -- marching cubes over a truncated signed distance volume, as faces that index the points of
// ctd_tsdf_surface_points_f32 (ctd_tsdf_mesh_faces_i32, ctd_tsdf_mesh_case; the rule is stated word for word in
// include/ctd_hip_mesh.h, the table csrc/ctd_mc_table.h is generated from it by tools/make_mc_table.py).
//
// The voxel of a thread, the usability rule and surf_count_kernel are those of ctd_tsdf_surf.h (shared with tsdf.hip:
// the faces index what that file emits, so the flags, their counts and their order come from the same code), the
// workgroup prefixes and fuse_scan_kernel those of ctd_compact.h.  A workgroup takes 256 consecutive voxels of ONE
// track; a thread takes a voxel and the cell whose corner 0 that voxel is.
//   surf_count_kernel  -- the three crossing flags of a voxel as one byte, the workgroup's number of points.  Per voxel
//     8 B read + the +x, +y, +z neighbours (cached rows), 1 B written.
//   fuse_scan_kernel   -- ONE workgroup: exclusive scan of the point counts (the per-track totals go to the workspace).
//   mesh_case_kernel   -- per voxel the track-local index of its first point (workgroup offset + flags before the
//     thread), stored where the voxel has a flag: nothing else reads it; per cell the case byte from the eight
//     corners' usability and signs (0 when not meshed; the corners are read up to the first unusable one) and, from the
//     table's count column, the workgroup's number of triangles.  Per voxel 1 B flags read, 1 B case written, the eight
//     corners' weight and tsdf (8 B compulsory, the rest cached rows and slices), and 4 B index written per flagged voxel.
//   fuse_scan_kernel   -- ONE workgroup: exclusive scan of the triangle counts, n_faces_per_track.
//   mesh_scatter_kernel -- a workgroup whose scanned offsets show no face, or none below the capacity, leaves at once;
//     the others: the table in LDS (256 x 16 B, one row per thread); offset of the workgroup + an in-workgroup
//     prefix of the cells' counts 0 .. 5; per triangle three vertices, each the first index of the edge's lower corner +
//     the popcount of its lower flags: per voxel 1 B case read, per triangle 3 x (4 B + 1 B) gathered and 12 B written.
// No atomics, no flag that another workgroup waits on: the same bits on every run.
#include "../../include/ctd_hip_mesh.h"
#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_mc_table.h"
#include "ctd_tsdf_surf.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

// one row per case: the edge ids of up to 5 triangles, then the number of triangles
alignas(16) __device__ const uint8_t kMcTableDevice[256][16] = {CTD_MC_TABLE_ROWS};
const uint8_t kMcTableHost[256][16] = {CTD_MC_TABLE_ROWS};

__global__ __launch_bounds__(kChunk) void mesh_case_kernel(const float* __restrict__ tsdf,
                                                           const float* __restrict__ weight, float min_weight,
                                                           const uint8_t* __restrict__ emit,
                                                           const int* __restrict__ point_offsets,
                                                           int* __restrict__ first_point, uint8_t* __restrict__ cases,
                                                           int* __restrict__ wg_faces, Grid gr, long nvox, int chunks) {
  __shared__ int wave_points[kChunk / 64];
  __shared__ int wave_faces[kChunk / 64];
  const SurfVoxel s = surf_voxel_of_block(gr, nvox, chunks);
  const bool live = s.p < nvox;
  const int f = live ? emit[s.g] : 0;
  int cs = 0;                                                   // the cell's case
  // the cell's position in 32-bit arithmetic (p < nx * ny * nz < 2^31); s.i, s.j, s.k, from 64-bit divisions, stay unused
  const unsigned p32 = (unsigned)s.p, row = p32 / (unsigned)gr.nx;
  const int ci = (int)(p32 - row * (unsigned)gr.nx), ck = (int)(row / (unsigned)gr.ny), cj = (int)(row - (unsigned)ck * (unsigned)gr.ny);
  if (live && ci + 1 < gr.nx && cj + 1 < gr.ny && ck + 1 < gr.nz) {
    const long sy = gr.nx, sz = (long)gr.nx * gr.ny;
    bool meshed = true;
#pragma unroll
    for (int n = 0; n < 8; ++n) {
      float T = 0.f;
      const long g = s.g + (n & 1) + ((n >> 1) & 1) * sy + ((n >> 2) & 1) * sz;
      if (meshed && surf_usable(tsdf, weight, g, min_weight, T))
        cs |= (T < 0.f ? 1 : 0) << n;
      else
        meshed = false;
    }
    if (!meshed) cs = 0;
  }
  // the voxel's first point, in the order of surf_scatter_kernel (ascending voxel, then axis), and the workgroup's faces
  int n_points, n_faces;
  const int before = wg_flags3_before<kChunk>(f, wave_points, n_points);
  (void)wg_exclusive_sum<kChunk>(kMcTableDevice[cs][15], wave_faces, n_faces);
  if (live) {
    const int o = point_offsets[blockIdx.x] - point_offsets[(long)s.b * chunks] + before;
    if (f) first_point[s.g] = o;                                // read only through a set flag of the voxel
    cases[s.g] = (uint8_t)cs;
  }
  if (threadIdx.x == 0) wg_faces[blockIdx.x] = n_faces;
}

__global__ __launch_bounds__(kChunk) void mesh_scatter_kernel(const uint8_t* __restrict__ emit,
                                                              const int* __restrict__ first_point,
                                                              const uint8_t* __restrict__ cases,
                                                              const int* __restrict__ face_offsets,
                                                              int32_t* __restrict__ faces, long capacity, Grid gr,
                                                              long nvox, int chunks) {
  __shared__ uint4 table[256];                                // kMcTableDevice, a row per thread
  __shared__ int wave_sum[kChunk / 64];
  // a workgroup without faces, or with all of them past the capacity, has nothing to write (uniform: before any barrier)
  const int first = face_offsets[blockIdx.x];
  if (face_offsets[blockIdx.x + 1] == first || first >= capacity) return;
  table[threadIdx.x] = reinterpret_cast<const uint4*>(&kMcTableDevice[0][0])[threadIdx.x];
  const SurfVoxel s = surf_voxel_of_block(gr, nvox, chunks);
  const int cs = s.p < nvox ? cases[s.g] : 0;
  __syncthreads();
  const uint8_t* row = reinterpret_cast<const uint8_t*>(&table[cs]);
  const int n = row[15];
  int total;
  long o = (long)first + wg_exclusive_sum<kChunk>(n, wave_sum, total);
  if (n == 0) return;                                         // (cs != 0 only at a cell inside the grid)
  const long stride[3] = {1, gr.nx, (long)gr.nx * gr.ny};
  for (int t = 0; t < n; ++t, ++o) {
    if (o >= capacity) return;                                // ascending: every later face of the thread is past it too
#pragma unroll
    for (int m = 0; m < 3; ++m) {
      const int e = row[t * 3 + m], c = e >> 2, r = e & 3;
      // the edge's lower corner: r counts the corners with coordinate c == 0 upwards, over the two other axes
      const int a0 = c == 0 ? 1 : 0, a1 = c == 2 ? 1 : 2;
      const long g = s.g + (r & 1) * stride[a0] + (r >> 1) * stride[a1];
      faces[o * 3 + m] = first_point[g] + __popc((unsigned)emit[g] & ((1u << c) - 1u));
    }
  }
}

struct MeshLayout {                                           // byte offsets into the workspace
  size_t emit, point_offsets, first_point, cases, face_offsets, n_points, bytes;
};
MeshLayout mesh_layout(int B, int nx, int ny, int nz) {
  const size_t nv = (size_t)B * nx * ny * nz, wgs = (size_t)B * surf_chunks(nx, ny, nz);
  WorkspaceCursor c;
  MeshLayout l;
  l.emit = c.take(nv);
  l.point_offsets = c.take_counts(wgs);
  l.first_point = c.take(sizeof(int) * nv);
  l.cases = c.take(nv);
  l.face_offsets = c.take_counts(wgs);
  l.n_points = c.take(sizeof(int64_t) * (size_t)B);
  l.bytes = c.bytes;
  return l;
}

int mesh_shape_status(int B, int nx, int ny, int nz) {
  const int st = surf_shape_status(B, nx, ny, nz);
  if (st != CTD_OK) return st;
  if (5.0 * B * nx * ny * nz >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

}  // namespace

static int tsdf_mesh_faces_i32(const float* tsdf, const float* weight, float min_weight, int32_t* faces,
                               int64_t* n_faces_per_track, int64_t capacity, int B, int nx, int ny, int nz, void* workspace,
                               hipStream_t stream) {
  const MeshLayout l = mesh_layout(B, nx, ny, nz);
  char* ws = (char*)workspace;
  uint8_t* emit = (uint8_t*)(ws + l.emit);
  int* point_offsets = (int*)(ws + l.point_offsets);
  int* first_point = (int*)(ws + l.first_point);
  uint8_t* cases = (uint8_t*)(ws + l.cases);
  int* face_offsets = (int*)(ws + l.face_offsets);
  int64_t* n_points = (int64_t*)(ws + l.n_points);
  const Grid gr = {nx, ny, nz};
  const long nvox = (long)nx * ny * nz;
  const int chunks = (int)surf_chunks(nx, ny, nz), blocks = B * chunks;
  surf_count_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(tsdf, weight, min_weight, emit, point_offsets,
                                                                            gr, nvox, chunks);
  CTD_LAUNCH_CHECK();
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(point_offsets, blocks, chunks, n_points, B);
  CTD_LAUNCH_CHECK();
  mesh_case_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(tsdf, weight, min_weight, emit, point_offsets,
                                                                           first_point, cases, face_offsets, gr, nvox, chunks);
  CTD_LAUNCH_CHECK();
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(face_offsets, blocks, chunks, n_faces_per_track, B);
  CTD_LAUNCH_CHECK();
  if (!faces || capacity == 0) return CTD_OK;
  mesh_scatter_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(emit, first_point, cases, face_offsets, faces,
                                                                              (long)capacity, gr, nvox, chunks);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_tsdf_mesh_workspace_bytes(int B, int nx, int ny, int nz) {
  if (B <= 0 || mesh_shape_status(B, nx, ny, nz) != CTD_OK) return 0;
  return mesh_layout(B, nx, ny, nz).bytes;
}

int ctd_tsdf_mesh_faces_i32(const float* tsdf, const float* weight, float min_weight, int32_t* faces,
                            int64_t* n_faces_per_track, int64_t capacity, int B, int nx, int ny, int nz, void* workspace,
                            size_t workspace_bytes, int device, void* stream) {
  if (grid_status(B, nx, ny, nz, true) != CTD_OK || !positive_finite(min_weight)) return CTD_ERR_INVALID_ARG;
  if (!tsdf || !weight || !n_faces_per_track || (faces && capacity < 0)) return CTD_ERR_INVALID_ARG;
  const int st = mesh_shape_status(B, nx, ny, nz);
  if (st != CTD_OK) return st;
  const size_t nv = (size_t)B * nx * ny * nz;
  const size_t cap = !faces ? 0 : (size_t)capacity < 5 * nv ? (size_t)capacity : 5 * nv;   // no more faces than 5 a cell
  const size_t need = ctd_tsdf_mesh_workspace_bytes(B, nx, ny, nz);
  const Span s[] = {{faces, 12 * cap}, {n_faces_per_track, 8 * (size_t)B}, {workspace, need}, {tsdf, 4 * nv}, {weight, 4 * nv}};
  if (spans_overlap(s, 3, 5)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return tsdf_mesh_faces_i32(tsdf, weight, min_weight, faces, n_faces_per_track, capacity, B, nx, ny, nz, workspace,
                             (hipStream_t)stream);
}

int ctd_tsdf_mesh_case(int mc_case, int32_t* edges) {
  if (mc_case < 0 || mc_case > 255 || !edges) return -1;
  const uint8_t* row = kMcTableHost[mc_case];
  for (int i = 0; i < 15; ++i) edges[i] = i < 3 * row[15] ? (int32_t)row[i] : -1;
  return row[15];
}

}  // extern "C"
