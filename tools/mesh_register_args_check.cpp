// mesh_register_args_check.cpp -- the argument validation of csrc/mesh_register.hip (include/ext/ctd_hip_mesh_register.h)
// under host sanitizers: a stand-alone program with its own main that walks the rejections of the three entry points with
// host buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_register.hip \
//         tools/mesh_register_args_check.cpp -o tools/bin/mesh_register_args_check && tools/bin/mesh_register_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ext/ctd_hip_mesh_register.h"
#include "args_check.h"
int main() {
  const Arena P(4096, 14);
  float *points = (float*)P(0), *R = (float*)P(1), *t = (float*)P(2), *verts = (float*)P(3);
  int* faces = (int*)P(4);
  double* sys = (double*)P(5);
  void *ws = P(6), *bvh = P(7);
  int32_t *face = (int32_t*)P(8), *hint = (int32_t*)P(9);
  float *residual = (float*)P(10), *closest = (float*)P(11), *R_out = (float*)P(12), *t_out = (float*)P(13);
  uint8_t* ok = (uint8_t*)P(9);
  const int n = 10, K = 2, nv = 8, nf = 4;
  const float nan = std::nanf(""), inf = INFINITY;
  const size_t need = ctd_mesh_register_workspace_bytes(K, n);
  EXPECT((int)(need > 0 && need % 256 == 0 && need <= 4096), 1);
  EXPECT((int)ctd_mesh_register_workspace_bytes(0, n), 0);
  EXPECT((int)ctd_mesh_register_workspace_bytes(65, n), 0);
  EXPECT((int)ctd_mesh_register_workspace_bytes(K, -1), 0);
  EXPECT((int)ctd_mesh_register_workspace_bytes(K, 0), 0);
  EXPECT((int)ctd_mesh_register_workspace_bytes(64, 1 << 24), 0);
  EXPECT((int)ctd_mesh_register_workspace_bytes(INT32_MIN, INT32_MAX), 0);
#define SYS(points_, n_, R_, t_, K_, verts_, nv_, faces_, nf_, bvh_, metric_, max_, hint_, sys_, face_, res_, clo_, ws_, nws_) \
  ctd_mesh_register_system_f32(points_, n_, R_, t_, K_, verts_, nv_, faces_, nf_, bvh_, metric_, max_, hint_, sys_, face_, res_, clo_, ws_, nws_, -1, nullptr)
  // sizes, in their order
  EXPECT(SYS(points, -1, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, -1, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, -1, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, INT32_MIN, R, t, INT32_MIN, verts, INT32_MIN, faces, INT32_MIN, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  const int bad_K[] = {0, -1, 65, INT32_MAX, INT32_MIN};
  for (int k : bad_K) EXPECT(SYS(points, n, R, t, k, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, 1 << 30, R, t, 1, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, INT32_MAX, R, t, 64, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, (1 << 28) + 1, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  // the metric and the cutoff
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 2, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, -1, inf, hint, sys, face, residual, closest, ws, need), 1);
  const float bad_max[] = {nan, -nan, -inf, -1.f, -1e-45f};
  for (float v : bad_max) {
    EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, v, hint, sys, face, residual, closest, ws, need), 1);
    EXPECT(SYS(points, 0, R, t, K, verts, nv, faces, nf, bvh, 1, v, hint, sys, face, residual, closest, ws, need), 1);
  }
  // pointers
  EXPECT(SYS(nullptr, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, nullptr, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, nullptr, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, nullptr, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, 0, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, nullptr, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, nullptr, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, nullptr, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, (char*)bvh + 4, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, (char*)bvh + 8, 0, inf, hint, sys, face, residual, closest, ws, need), 1);
  // overlap: an output on an input, on another output, on the workspace, this round's faces on its hint
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, (double*)R, face, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, (int32_t*)points, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, (float*)face + 19, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, (float*)ws, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, hint, residual, closest, ws, need), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, faces, need), 1);
  // the workspace, last
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, nullptr, need), 2);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, ws, need - 1), 2);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, face, residual, closest, (char*)ws + 16, need), 2);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, nullptr, sys, nullptr, nullptr, nullptr, ws, 0), 2);
  // precedence: sizes before the metric, the metric before the cutoff, the cutoff before pointers, overlap before the workspace
  EXPECT(SYS(nullptr, -1, R, t, K, verts, nv, faces, nf, bvh, 7, nan, hint, sys, face, residual, closest, nullptr, 0), 1);
  EXPECT(SYS(nullptr, n, nullptr, nullptr, K, verts, nv, faces, nf, bvh, 0, -1.f, hint, nullptr, face, residual, closest, nullptr, 0), 1);
  EXPECT(SYS(points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, sys, hint, residual, closest, nullptr, 0), 1);

#define UPD(sys_, R_, t_, mc_, mp_, da_, Ro_, to_, ok_, K_) ctd_mesh_register_update_f32(sys_, R_, t_, mc_, mp_, da_, Ro_, to_, ok_, K_, -1, nullptr)
  for (int k : bad_K) EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R_out, t_out, ok, k), 1);
  EXPECT(UPD(sys, R, t, -1, 1e-4, 0.0, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, -1e-4, 0.0, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, (double)nan, 0.0, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, -0.5, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, (double)nan, R_out, t_out, ok, K), 1);
  EXPECT(UPD(nullptr, R, t, 64, 1e-4, 0.0, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, nullptr, t, 64, 1e-4, 0.0, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, nullptr, 64, 1e-4, 0.0, R_out, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, nullptr, t_out, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R_out, nullptr, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R_out, t_out, nullptr, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R, t_out, ok, K), 1);                       // in place is refused
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R_out, t, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R_out, R_out + 17, ok, K), 1);
  EXPECT(UPD(sys, R, t, 64, 1e-4, 0.0, R_out, t_out, (uint8_t*)sys + 463, K), 1);
  return report();
}
