// mesh_simplify_args_check.cpp -- the argument validation of csrc/mesh_simplify.hip (include/ctd_hip_mesh_simplify.h) under
// host sanitizers: a stand-alone program with its own main that walks the rejections of the entry point and the workspace
// query with host buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_simplify.hip \
//         tools/mesh_simplify_args_check.cpp -o tools/bin/mesh_simplify_args_check && tools/bin/mesh_simplify_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ctd_hip_mesh_simplify.h"
#include "args_check.h"
int main() {
  const Arena P(16384, 13);                                   // (the workspace, the last, is longer than a slot)
  float *verts = (float*)P(0), *out = (float*)P(4);
  int32_t *faces = (int32_t*)P(1), *fo = (int32_t*)P(2), *fi = (int32_t*)P(3), *leader = (int32_t*)P(5), *vc = (int32_t*)P(6);
  int32_t *fout = (int32_t*)P(7), *fidx = (int32_t*)P(8);
  int64_t* counts = (int64_t*)P(9);
  void* ws = P(10);
  const int64_t n = 100, m = 200, ni = 600, big_m = (int64_t(1) << 31) / 6 + 1, big_n = int64_t(1) << 31;
  const float nan = std::nanf(""), inf = INFINITY;
  const double dnan = std::nan(""), dinf = INFINITY;
  const size_t nws = ctd_mesh_simplify_workspace_bytes(n, m);
  if (nws != 9 * 512 + 512 + 1280 + 7424 + 12 * 256 + 2560 + 256 + 1024 + 4 * 512 + 3 * 256 + 256) { ++fails; std::printf("workspace %zu\n", nws); }
  if (ctd_mesh_simplify_workspace_bytes(-1, m) != 0 || ctd_mesh_simplify_workspace_bytes(n, -1) != 0 ||
      ctd_mesh_simplify_workspace_bytes(big_n, m) != 0 || ctd_mesh_simplify_workspace_bytes(n, big_m) != 0 ||
      ctd_mesh_simplify_workspace_bytes(INT64_MIN, INT64_MAX) != 0 || ctd_mesh_simplify_workspace_bytes(INT64_MAX, INT64_MIN) != 0 ||
      ctd_mesh_simplify_workspace_bytes(0, 0) == 0 || ctd_mesh_simplify_workspace_bytes(big_n - 1, big_m - 1) == 0) {
    ++fails;
    std::printf("workspace query\n");
  }
#define CALL(verts_, n_, faces_, m_, fo_, fi_, ni_, ox_, cell_, reg_, out_, leader_, cv_, vc_, fout_, fidx_, cf_, counts_, ws_, nws_) \
  ctd_mesh_simplify_f32(verts_, n_, faces_, m_, fo_, fi_, ni_, ox_, 0.f, 0.f, cell_, reg_, 1, out_, leader_, cv_, vc_, fout_, fidx_, cf_, \
                        counts_, ws_, nws_, -1, nullptr)
  EXPECT(CALL(verts, -1, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, INT64_MIN, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, -1, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, -1, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, INT64_MIN, counts, ws, nws), 1);
  EXPECT(CALL(nullptr, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(nullptr, 0, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, nullptr, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, nullptr, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, nullptr, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, nullptr, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, nullptr, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, nullptr, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, nullptr, fidx, 0, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, nullptr, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, nullptr, ws, nws), 1);
  const float bad_cell[] = {0.f, -1.f, nan, inf, -inf};
  for (float v : bad_cell) EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, v, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  const float bad_origin[] = {nan, inf, -inf};
  for (float v : bad_origin) EXPECT(CALL(verts, n, faces, m, fo, fi, ni, v, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  const double bad_reg[] = {-1e-300, dnan, dinf, -dinf};
  for (double v : bad_reg) EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, v, out, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, big_m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, nullptr, 0), 3);
  EXPECT(CALL(verts, big_n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, nullptr, 0), 3);
  EXPECT(CALL(verts, n, faces, m, fo, fi, big_n, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, nullptr, 0), 3);
  EXPECT(CALL(verts, INT64_MAX, faces, INT64_MAX, fo, fi, INT64_MAX, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, nullptr, 0), 3);
  EXPECT(CALL(verts, n, faces, big_m, fo, fi, ni, 0.f, 0.f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, nullptr, 0), 1);
  EXPECT(CALL(verts, big_n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, verts, leader, n, vc, fout, fidx, m, counts, nullptr, 0), 3);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, verts, leader, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, (int32_t*)out + 3 * n - 1, n, vc, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, fi + ni - 1, fout, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, faces + 3 * m - 1, fidx, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fo + n, m, counts, ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, (int64_t*)((char*)ws - 63), ws, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, verts, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, INT64_MAX, vc, fout, fidx, INT64_MAX, counts, nullptr, nws), 2);   // the capacities count up to n_verts and n_faces
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, (float*)faces - 6, leader, 2, vc, fout, fidx, m, counts, nullptr, nws), 2);   // two rows end where faces starts
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, (float*)faces - 6, leader, 3, vc, fout, fidx, m, counts, nullptr, nws), 1);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, nullptr, nws), 2);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, ws, nws - 1), 2);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 1e-3, out, leader, n, vc, fout, fidx, m, counts, (char*)ws + 8, nws), 2);
  EXPECT(CALL(verts, n, faces, m, fo, fi, ni, 0.f, 0.1f, 0.0, out, leader, 0, vc, fout, fidx, 0, counts, nullptr, 0), 2);
  EXPECT(CALL(verts, 0, faces, 0, fo, fi, 0, 0.f, 0.1f, 1e-3, out, leader, 0, vc, fout, fidx, 0, counts, nullptr, 0), 2);
  return report();
}
