// mesh_global_args_check.cpp -- the argument validation of csrc/mesh_global.hip (include/ext/ctd_hip_mesh_global.h) under
// host sanitizers: a stand-alone program with its own main that walks the rejections of the entry point with host
// buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_global.hip \
//         tools/mesh_global_args_check.cpp -o tools/bin/mesh_global_args_check && tools/bin/mesh_global_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ext/ctd_hip_mesh_global.h"
#include "args_check.h"
int main() {
  const Arena P(4096, 8);
  float *points = (float*)P(0), *R = (float*)P(1), *base = (float*)P(2), *offsets = (float*)P(3), *origin = (float*)P(5);
  uint8_t* levels = (uint8_t*)P(4);
  int64_t* score = (int64_t*)P(6);
  const float nan = std::nanf(""), inf = INFINITY;
  // the arguments of a good call, one of them replaced at a time
  struct A {
    const float* points; int n; const float* R; const float* base; int M; const float* offsets; int T; const uint8_t* levels;
    int nx, ny, nz; const float* origin; float voxel; int64_t* score;
  };
  const A good = {points, 10, R, base, 4, offsets, 5, levels, 3, 4, 5, origin, 0.5f, score};
  auto call = [](const A& a) {
    return ctd_pose_score_u8(a.points, a.n, a.R, a.base, a.M, a.offsets, a.T, a.levels, a.nx, a.ny, a.nz, a.origin, a.voxel,
                             a.score, -1, nullptr);
  };
#define WITH(change) [&] { A a = good; change; return call(a); }()
  // the number of points
  const int bad_n[] = {-1, 65537, 1 << 30, INT32_MAX, INT32_MIN};
  for (int v : bad_n) EXPECT(WITH(a.n = v), 1);
  // the numbers of rotations and offsets, and their product
  const int bad_M[] = {0, -1, INT32_MIN};
  for (int v : bad_M) EXPECT(WITH(a.M = v), 1);
  const int bad_T[] = {0, -1, 4097, INT32_MAX, INT32_MIN};
  for (int v : bad_T) EXPECT(WITH(a.T = v), 1);
  EXPECT(WITH(a.M = 1 << 19; a.T = 4096), 1);                  // 2^31
  EXPECT(WITH(a.M = INT32_MAX; a.T = 2), 1);
  EXPECT(WITH(a.M = INT32_MAX; a.T = 4096), 1);
  // the volume
  const int bad_dim[] = {0, -1, 1025, INT32_MAX, INT32_MIN};
  for (int v : bad_dim) {
    EXPECT(WITH(a.nx = v), 1);
    EXPECT(WITH(a.ny = v), 1);
    EXPECT(WITH(a.nz = v), 1);
  }
  const float bad_voxel[] = {0.f, -0.f, -1.f, nan, -nan, inf, -inf, -1e-45f};
  for (float v : bad_voxel) {
    EXPECT(WITH(a.voxel = v), 1);
    EXPECT(WITH(a.voxel = v; a.n = 0; a.points = nullptr), 1);
  }
  // pointers
  EXPECT(WITH(a.points = nullptr), 1);
  EXPECT(WITH(a.R = nullptr), 1);
  EXPECT(WITH(a.base = nullptr), 1);
  EXPECT(WITH(a.offsets = nullptr), 1);
  EXPECT(WITH(a.levels = nullptr), 1);
  EXPECT(WITH(a.origin = nullptr), 1);
  EXPECT(WITH(a.score = nullptr), 1);
  EXPECT(WITH(a.score = nullptr; a.n = 0; a.points = nullptr), 1);
  // overlap: the scores (8 * 4 * 5 = 160 bytes) on any input
  EXPECT(WITH(a.score = (int64_t*)points), 1);
  EXPECT(WITH(a.score = (int64_t*)((char*)points + 112)), 1);  // the last 8 of the points' 120 bytes
  EXPECT(WITH(a.score = (int64_t*)R), 1);
  EXPECT(WITH(a.score = (int64_t*)((char*)base + 40)), 1);
  EXPECT(WITH(a.score = (int64_t*)((char*)offsets - 152)), 1); // its last 8 bytes on the first offset
  EXPECT(WITH(a.score = (int64_t*)((char*)levels + 56)), 1);   // 3 * 4 * 5 = 60 bytes of levels
  EXPECT(WITH(a.score = (int64_t*)((char*)origin + 8)), 1);
  EXPECT(WITH(a.score = (int64_t*)((char*)origin - 152)), 1);
  // precedence: the points before the poses, the poses before the volume, the volume before the voxel, the voxel before
  // the pointers, the pointers before the overlap -- every one is CTD_ERR_INVALID_ARG, and none reaches a HIP call
  EXPECT(WITH(a.n = -1; a.M = 0; a.nx = 0; a.voxel = nan; a.R = nullptr; a.score = (int64_t*)points), 1);
  EXPECT(WITH(a.T = 4097; a.nz = 1025; a.voxel = 0.f; a.levels = nullptr), 1);
  EXPECT(WITH(a.ny = 0; a.voxel = inf; a.origin = nullptr), 1);
  EXPECT(WITH(a.voxel = -1.f; a.score = nullptr), 1);
  EXPECT(WITH(a.points = nullptr; a.score = (int64_t*)R), 1);
  // the limits themselves pass the size checks: the NULL score answers
  EXPECT(WITH(a.n = 65536; a.score = nullptr), 1);
  EXPECT(WITH(a.M = (1 << 19) - 1; a.T = 4096; a.score = nullptr), 1);
  EXPECT(WITH(a.nx = 1024; a.ny = 1024; a.nz = 1024; a.score = nullptr), 1);
  EXPECT(WITH(a.voxel = 1e-45f; a.score = nullptr), 1);
  return report();
}
