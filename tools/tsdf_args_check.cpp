// tsdf_args_check.cpp -- the argument validation of csrc/tsdf.hip (include/ctd_hip_tsdf.h) under host sanitizers: a
// stand-alone program with its own main that walks the rejections of the three entry points and the workspace query with
// host buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/tsdf.hip tools/tsdf_args_check.cpp \
//         -o tools/bin/tsdf_args_check && tools/bin/tsdf_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ctd_hip_tsdf.h"
#include "args_check.h"
int main() {
  const Arena arena(4096, 12);
  auto P = [&](int i) { return (float*)arena(i); };
  float *tsdf = P(0), *weight = P(1), *origin = P(2), *depth = P(3), *ray = P(5), *K = P(6), *R = P(7), *t = P(8), *pts = P(9), *nrm = P(10);
  uint8_t* valid = (uint8_t*)P(4);
  int64_t* src = (int64_t*)P(11);
  int64_t npt[4];
  const float nan = std::nanf(""), inf = INFINITY;
  // integrate
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 2, 0, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, nan, depth, valid, ray, K, R, t, 0.4f, 64.f, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, inf, 64.f, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 0.5f, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(nullptr, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 0, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 1 << 20, 2048, 1, 1, 3, 4, 5, -1, nullptr), 3);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 2, 2049, 4, 5, 3, 4, 5, -1, nullptr), 3);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 2147483647, 2048, 2048, 2048, 64, 1 << 24, 1 << 24, -1, nullptr), 3);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 8192, 1, 1, 2048, 1, 1, 1, -1, nullptr), 3);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, tsdf, origin, 0.1f, depth, valid, ray, K, R, t, 0.4f, 64.f, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, valid, (float*)((char*)weight + 476), K, R, t, 0.4f, 64.f, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_integrate_f32(tsdf, weight, origin, 0.1f, depth, nullptr, ray, K, R, t, 0.4f, 64.f, 0, 3, 4, 5, 3, 4, 5, -1, nullptr), 0);
  // surface points and its workspace query
  const size_t nws = ctd_tsdf_surface_workspace_bytes(2, 3, 4, 5);
  if (nws != 512) { ++fails; std::printf("workspace %zu\n", nws); }
  if (ctd_tsdf_surface_workspace_bytes(2147483647, 2048, 2048, 2048) != 0 || ctd_tsdf_surface_workspace_bytes(0, 3, 4, 5) != 0 ||
      ctd_tsdf_surface_workspace_bytes(1, 1024, 1024, 1024) != 0 || ctd_tsdf_surface_workspace_bytes(1 << 24, 1, 1, 1) != 0 ||
      ctd_tsdf_surface_workspace_bytes(-2147483647 - 1, -5, 0, 3) != 0) { ++fails; std::printf("workspace query\n"); }
  void* ws = P(8);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, src, npt, 100, 2, 3, 4, -1, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, -inf, pts, nrm, src, npt, 100, 2, 3, 4, 5, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, src, npt, -1, 2, 3, 4, 5, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, nullptr, npt, 100, 2, 3, 4, 5, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, src, npt, 100, 1, 1024, 1024, 1024, ws, nws, -1, nullptr), 3);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, src, npt, INT64_MAX, 2, 3, 4, 5, ws, nws, -1, nullptr), 1);   // spans of 2^63 * 12 wrap: still an overlap or not, never a crash
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, pts, src, npt, 100, 2, 3, 4, 5, ws, nws, -1, nullptr), 1);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, src, npt, 100, 2, 3, 4, 5, nullptr, nws, -1, nullptr), 2);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, pts, nrm, src, npt, 100, 2, 3, 4, 5, (char*)ws + 8, nws, -1, nullptr), 2);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, nullptr, nullptr, nullptr, npt, -9, 2, 3, 4, 5, ws, nws - 1, -1, nullptr), 2);
  EXPECT(ctd_tsdf_surface_points_f32(tsdf, weight, origin, 0.1f, 1.f, nullptr, nullptr, nullptr, npt, 0, 0, 3, 4, 5, nullptr, 0, -1, nullptr), 0);
  // ray cast
  float* out = P(9);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 0, 1.f, out, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, -0.5f, 0.05f, 8, 1.f, out, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, nan, 8, 1.f, out, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 8, 1.f, out, 2, 3, 4, 5, 65, 1, 1, -1, nullptr), 1);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 8, 1.f, nullptr, 0, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 8, 1.f, out, 2, 3, 4, 5, 3, (1 << 24) + 1, 1, -1, nullptr), 3);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 8, 1.f, out, 1 << 18, 1, 1, 1, 64, 1, 1, -1, nullptr), 3);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 2147483647, 1.f, out, 2147483647, 2048, 2048, 2048, 64, 1 << 24, 1 << 24, -1, nullptr), 3);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.5f, 0.05f, 8, 1.f, ray + 2, 2, 3, 4, 5, 3, 4, 5, -1, nullptr), 1);
  EXPECT(ctd_tsdf_raycast_f32(tsdf, weight, origin, 0.1f, ray, R, t, 0.f, 0.05f, 1, 1.f, out, 0, 3, 4, 5, 3, 4, 5, -1, nullptr), 0);
  return report();
}
