// mesh_sdf_args_check.cpp -- the argument validation of csrc/mesh_sdf.hip (include/ctd_hip_mesh_sdf.h) under host
// sanitizers: a stand-alone program with its own main that walks the rejections of the entry point with host buffers
// standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_sdf.hip \
//         tools/mesh_sdf_args_check.cpp -o tools/bin/mesh_sdf_args_check && tools/bin/mesh_sdf_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ctd_hip_mesh_sdf.h"
#include "args_check.h"
int main() {
  const Arena P(4096, 12);
  float *points = (float*)P(0), *verts = (float*)P(1), *d2 = (float*)P(6), *closest = (float*)P(8);
  int *faces = (int*)P(2), *face = (int*)P(7);
  int32_t *fo = (int32_t*)P(3), *fi = (int32_t*)P(4);
  void* bvh = P(5);
  int8_t *feature = (int8_t*)P(9), *sign = (int8_t*)P(10);
  const int n = 10, nv = 10, nf = 10, big_n = (1 << 30) / 3 * 2 + 1 /* 3 n >= 2^31 */, big_f = (1 << 28) + 1;
  const int64_t ni = 30;
  const float nan = std::nanf(""), inf = INFINITY;
#define CALL(points_, n_, verts_, nv_, faces_, nf_, fo_, fi_, ni_, bvh_, max_, d2_, face_, closest_, feature_, sign_) \
  ctd_point_mesh_signed_f32(points_, n_, verts_, nv_, faces_, nf_, fo_, fi_, ni_, bvh_, max_, d2_, face_, closest_, feature_, sign_, -1, nullptr)
  // sizes
  EXPECT(CALL(points, -1, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, -1, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, -1, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, -1, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, INT64_MIN, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, INT32_MIN, verts, INT32_MIN, faces, INT32_MIN, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, big_n, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, INT32_MAX, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, big_f, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  // the cutoff
  const float bad_max[] = {nan, -nan, -inf, -1.f, -1e-45f};
  for (float v : bad_max) {
    EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, bvh, v, d2, face, closest, feature, sign), 1);
    EXPECT(CALL(points, 0, verts, nv, faces, nf, fo, fi, ni, bvh, v, d2, face, closest, feature, sign), 1);
  }
  // pointers
  EXPECT(CALL(nullptr, n, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, bvh, inf, nullptr, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, nullptr, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, nullptr, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, nullptr), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, nullptr, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, nullptr, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, nullptr, 0, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, nullptr, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, nullptr, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, nullptr, nf, fo, fi, ni, nullptr, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, (char*)bvh + 4, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, n, verts, nv, faces, nf, fo, fi, ni, (char*)bvh + 8, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, 0, verts, nv, faces, nf, fo, fi, ni, (char*)bvh + 4, inf, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(points, 0, verts, nv, nullptr, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 1);
  // precedence: a size error before the cutoff, the cutoff before the pointers
  EXPECT(CALL(nullptr, -1, verts, nv, faces, nf, fo, fi, ni, bvh, nan, d2, face, closest, feature, sign), 1);
  EXPECT(CALL(nullptr, n, verts, nv, faces, nf, fo, fi, ni, bvh, -1.f, nullptr, nullptr, nullptr, nullptr, nullptr), 1);
  // nothing to do: CTD_OK before any HIP call
  EXPECT(CALL(points, 0, verts, nv, faces, nf, fo, fi, ni, bvh, inf, d2, face, closest, feature, sign), 0);
  EXPECT(CALL(points, 0, verts, nv, faces, nf, fo, fi, ni, nullptr, 0.f, d2, face, nullptr, feature, sign), 0);
  EXPECT(CALL(nullptr, 0, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, inf, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
  EXPECT(CALL(nullptr, 0, nullptr, nv, nullptr, 0, nullptr, nullptr, 0, nullptr, 3.4e38f, nullptr, nullptr, nullptr, nullptr, nullptr), 0);
  return report();
}
