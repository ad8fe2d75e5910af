// mesh_smooth_args_check.cpp -- the argument validation of csrc/mesh_smooth.hip (include/ctd_hip_mesh_smooth.h) under host
// sanitizers: a stand-alone program with its own main that walks the rejections of the three entry points and the two
// workspace queries with host buffers standing in for device pointers.  Every call returns before any HIP call, so it
// needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_smooth.hip \
//         tools/mesh_smooth_args_check.cpp -o tools/bin/mesh_smooth_args_check && tools/bin/mesh_smooth_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ctd_hip_mesh_smooth.h"
#include "args_check.h"
int main() {
  const Arena P(16384, 9);
  int32_t *faces = (int32_t*)P(0), *off = (int32_t*)P(1), *nb = (int32_t*)P(2), *fo = (int32_t*)P(3), *fi = (int32_t*)P(4);
  uint8_t* fl = (uint8_t*)P(5);
  int64_t* counts = (int64_t*)P(6);
  void* ws = P(7);
  float *verts = (float*)P(0), *out = (float*)P(8);
  const int64_t n = 100, m = 200, big_m = (int64_t(1) << 31) / 6 + 1, big_n = int64_t(1) << 31;
  const float nan = std::nanf(""), inf = INFINITY;
  // the workspace queries
  const size_t nws = ctd_mesh_adjacency_workspace_bytes(n, m), sws = ctd_mesh_smooth_workspace_bytes(n);
  if (nws != 512 + 512 + 512 + 2560 + 4864 + 3 * 256 || sws != 1280) { ++fails; std::printf("workspace %zu %zu\n", nws, sws); }
  if (ctd_mesh_adjacency_workspace_bytes(-1, m) != 0 || ctd_mesh_adjacency_workspace_bytes(n, -1) != 0 ||
      ctd_mesh_adjacency_workspace_bytes(big_n, m) != 0 || ctd_mesh_adjacency_workspace_bytes(n, big_m) != 0 ||
      ctd_mesh_adjacency_workspace_bytes(INT64_MIN, INT64_MAX) != 0 || ctd_mesh_adjacency_workspace_bytes(INT64_MAX, INT64_MIN) != 0 ||
      ctd_mesh_adjacency_workspace_bytes(0, 0) == 0 || ctd_mesh_adjacency_workspace_bytes(big_n - 1, big_m - 1) == 0 ||
      ctd_mesh_smooth_workspace_bytes(-1) != 0 || ctd_mesh_smooth_workspace_bytes(big_n) != 0 ||
      ctd_mesh_smooth_workspace_bytes(INT64_MAX) != 0 || ctd_mesh_smooth_workspace_bytes(INT64_MIN) != 0 ||
      ctd_mesh_smooth_workspace_bytes(0) != 0 || ctd_mesh_smooth_workspace_bytes(big_n - 1) == 0) { ++fails; std::printf("workspace query\n"); }
  // adjacency
  EXPECT(ctd_mesh_adjacency_i32(faces, -1, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, INT64_MIN, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(nullptr, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(nullptr, n, 0, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, nullptr, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, nullptr, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, nullptr, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, -1, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, INT64_MIN, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, big_m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_mesh_adjacency_i32(faces, big_n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_mesh_adjacency_i32(faces, INT64_MAX, INT64_MAX, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, big_m, off, nb, -1, fo, fi, 3 * m, fl, counts, nullptr, 0, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, big_m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, faces, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, off, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, off + 100, fi, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, nb + 6 * m - 1, 3 * m, fl, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, (uint8_t*)counts + 47, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, (int64_t*)ws, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, faces, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, INT64_MAX, fo, fi, INT64_MAX, fl, counts, nullptr, nws, -1, nullptr), 2);   // the capacities count up to 6 and 3 * n_faces
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, nullptr, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, ws, nws - 1, -1, nullptr), 2);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nb, 6 * m, fo, fi, 3 * m, fl, counts, (char*)ws + 8, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_adjacency_i32(faces, n, m, off, nullptr, -9, nullptr, nullptr, -9, fl, counts, ws, 0, -1, nullptr), 2);
  EXPECT(ctd_mesh_adjacency_i32(faces, 0, 0, off, nb, 0, fo, fi, 0, fl, counts, nullptr, 0, -1, nullptr), 2);
  // smoothing
  const int64_t nnz = 600;
  EXPECT(ctd_mesh_smooth_f32(verts, -1, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, INT64_MIN, fl, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(nullptr, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(nullptr, 0, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, nullptr, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nullptr, nnz, fl, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, nullptr, 10, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, nullptr, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, -1, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 1025, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, INT32_MIN, 0.5f, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  const float bad_lambda[] = {0.f, -0.f, -0.5f, 1.0001f, nan, inf, -inf}, bad_mu[] = {0.001f, -2.001f, nan, inf, -inf};
  for (float v : bad_lambda) EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, v, -0.53f, 1, out, ws, sws, -1, nullptr), 1);
  for (float v : bad_mu) EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, v, 1, out, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, big_n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, big_n, fl, 10, 0.5f, -0.53f, 1, out, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_smooth_f32(verts, INT64_MAX, off, nb, INT64_MAX, fl, 10, 0.5f, -0.53f, 1, out, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_smooth_f32(verts, big_n, off, nb, nnz, fl, 10, 2.f, -0.53f, 1, out, nullptr, 0, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, verts, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, (float*)nb + nnz - 1, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, (float*)fl, ws, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, out, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, off, sws, -1, nullptr), 1);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 0, (float*)fl, nullptr, sws, -1, nullptr), 2);   // vflags is not read
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, nullptr, 10, 0.5f, -0.53f, 0, out, nullptr, sws, -1, nullptr), 2);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 0, 1.f, 0.f, 1, out, nullptr, sws, -1, nullptr), 2);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 1024, 1.f, -2.f, 1, out, ws, sws - 1, -1, nullptr), 2);
  EXPECT(ctd_mesh_smooth_f32(verts, n, off, nb, nnz, fl, 10, 0.5f, -0.53f, 1, out, (char*)ws + 128, sws, -1, nullptr), 2);
  EXPECT(ctd_mesh_smooth_f32(verts, 0, off, nb, 0, fl, 10, 0.5f, -0.53f, 1, out, nullptr, 0, -1, nullptr), 2);
  // normals
  const int64_t ninc = 3 * m;
  float* normals = out;
  EXPECT(ctd_mesh_vertex_normals_f32(verts, -1, (int32_t*)P(1), m, fo, fi, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), -1, fo, fi, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, INT64_MIN, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(nullptr, n, (int32_t*)P(1), m, fo, fi, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, nullptr, m, fo, fi, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, nullptr, 0, fo, fi, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, nullptr, fi, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, nullptr, ninc, normals, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, ninc, nullptr, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, 0, (int32_t*)P(1), m, fo, fi, ninc, nullptr, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), big_m, fo, fi, ninc, normals, -1, nullptr), 3);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, big_n, (int32_t*)P(1), m, fo, fi, ninc, normals, -1, nullptr), 3);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, big_n, normals, -1, nullptr), 3);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, INT64_MAX, (int32_t*)P(1), INT64_MAX, fo, fi, INT64_MAX, normals, -1, nullptr), 3);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), big_m, fo, fi, ninc, nullptr, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), big_m, fo, fi, ninc, verts, -1, nullptr), 3);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, ninc, verts, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, ninc, (float*)P(1) + 3 * m - 1, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, ninc, (float*)fo + n, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, ninc, (float*)fi + ninc - 1, -1, nullptr), 1);
  EXPECT(ctd_mesh_vertex_normals_f32(verts, n, (int32_t*)P(1), m, fo, fi, ninc, (float*)P(1) - 3 * n + 1, -1, nullptr), 1);   // ends 4 bytes into faces
  return report();
}
