// mesh_clean_args_check.cpp -- the argument validation of csrc/mesh_clean.hip (include/ctd_hip_mesh_clean.h) under host
// sanitizers: a stand-alone program with its own main that walks the rejections of the two entry points and the workspace
// query with host buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_clean.hip \
//         tools/mesh_clean_args_check.cpp -o tools/bin/mesh_clean_args_check && tools/bin/mesh_clean_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ctd_hip_mesh_clean.h"
#include "args_check.h"
int main() {
  const Arena P(8192, 8);
  int32_t *faces = (int32_t*)P(0), *fo = (int32_t*)P(2), *fi = (int32_t*)P(3), *vi = (int32_t*)P(4), *label = (int32_t*)P(2), *size = (int32_t*)P(3);
  float* verts = (float*)P(1);
  int64_t* counts = (int64_t*)P(5);
  void* ws = P(6);
  const int64_t n = 100, m = 200, big_m = (int64_t(1) << 31) / 3 + 1, big_n = int64_t(1) << 31;
  // the workspace query
  const size_t nws = ctd_mesh_clean_workspace_bytes(n, m);
  if (nws != 3 * 512 + 1024 + 256 + 256 + 256 + 256 + 256) { ++fails; std::printf("workspace %zu\n", nws); }
  if (ctd_mesh_clean_workspace_bytes(-1, m) != 0 || ctd_mesh_clean_workspace_bytes(n, -1) != 0 ||
      ctd_mesh_clean_workspace_bytes(big_n, m) != 0 || ctd_mesh_clean_workspace_bytes(n, big_m) != 0 ||
      ctd_mesh_clean_workspace_bytes(INT64_MIN, INT64_MAX) != 0 || ctd_mesh_clean_workspace_bytes(INT64_MAX, INT64_MIN) != 0 ||
      ctd_mesh_clean_workspace_bytes(0, 0) == 0 || ctd_mesh_clean_workspace_bytes(big_n - 1, big_m - 1) == 0) { ++fails; std::printf("workspace query\n"); }
  // clean
  EXPECT(ctd_mesh_clean_i32(faces, verts, -1, m, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, -1, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 0, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, INT32_MIN, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(nullptr, verts, n, m, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(nullptr, verts, n, 0, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, nullptr, n, m, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, m, vi, n, nullptr, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, -1, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, nullptr, fi, INT64_MIN, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, m, vi, -1, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, big_m, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_mesh_clean_i32(faces, verts, big_n, m, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_mesh_clean_i32(faces, verts, INT64_MAX, INT64_MAX, 1, 1, 0, fo, fi, m, vi, n, counts, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, big_m, 1, 0, 0, fo, fi, m, vi, n, counts, nullptr, 0, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, big_m, 1, 1, 0, fo, fi, m, vi, n, counts, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, faces, fi, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fo, m, vi, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, m, (int32_t*)verts + 299, n, counts, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, m, vi, n, (int64_t*)ws, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, m, vi, n, counts, faces, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, INT64_MAX, vi, INT64_MAX, counts, nullptr, nws, -1, nullptr), 2);   // the capacities count up to n_faces, n_verts
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 0, fo, fi, m, (int32_t*)verts, n, counts, nullptr, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_clean_i32(faces, nullptr, n, m, 0, 1, 0, fo, fi, m, (int32_t*)verts, n, counts, nullptr, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 1, fo, fi, m, vi, n, counts, nullptr, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 1, fo, fi, m, vi, n, counts, ws, nws - 1, -1, nullptr), 2);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 1, fo, fi, m, vi, n, counts, (char*)ws + 8, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_clean_i32(faces, verts, n, m, 1, 1, 1, nullptr, nullptr, -9, nullptr, -9, counts, ws, 0, -1, nullptr), 2);
  EXPECT(ctd_mesh_clean_i32(faces, verts, 0, 0, 1, 1, 1, fo, fi, 0, vi, 0, counts, nullptr, 0, -1, nullptr), 2);
  // components
  int64_t* ncomp = counts;
  EXPECT(ctd_mesh_components_i32(faces, verts, -1, m, 1, label, size, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, INT64_MIN, 1, label, size, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(nullptr, verts, n, 0, 1, label, size, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, nullptr, n, m, 1, label, size, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, nullptr, size, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, nullptr, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, size, nullptr, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, big_m, 1, label, size, ncomp, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_components_i32(faces, verts, big_n, m, 1, label, size, ncomp, nullptr, 0, -1, nullptr), 3);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, big_m, 1, label, size, nullptr, nullptr, 0, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, label, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, (int32_t*)verts + 299, ncomp, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, size, (int64_t*)faces, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, size, ncomp, label, nws, -1, nullptr), 1);
  EXPECT(ctd_mesh_components_i32(faces, nullptr, n, m, 0, label, size, ncomp, nullptr, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, size, ncomp, ws, nws - 1, -1, nullptr), 2);
  EXPECT(ctd_mesh_components_i32(faces, verts, n, m, 1, label, size, ncomp, (char*)ws + 128, nws, -1, nullptr), 2);
  EXPECT(ctd_mesh_components_i32(faces, verts, 0, 0, 0, label, size, ncomp, nullptr, 0, -1, nullptr), 2);
  return report();
}
