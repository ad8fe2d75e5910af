// mesh_robust_args_check.cpp -- the argument validation of csrc/mesh_robust.hip (include/ext/ctd_hip_mesh_robust.h) under
// host sanitizers: a stand-alone program with its own main that walks the rejections of the three entry points with host
// buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_robust.hip \
//         tools/mesh_robust_args_check.cpp -o tools/bin/mesh_robust_args_check && tools/bin/mesh_robust_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ext/ctd_hip_mesh_robust.h"
#include "args_check.h"
int main() {
  const Arena P(4096, 20);
  float *points = (float*)P(0), *R = (float*)P(1), *t = (float*)P(2), *verts = (float*)P(3);
  int* faces = (int*)P(4);
  double* sys = (double*)P(5);
  void *ws = P(6), *bvh = P(7);
  int32_t *face = (int32_t*)P(8), *hint = (int32_t*)P(9);
  float *residual = (float*)P(10), *closest = (float*)P(11), *weight = (float*)P(12), *scale = (float*)P(13);
  float* normals = (float*)P(14);
  int8_t* status = (int8_t*)P(15);
  uint8_t *rim = (uint8_t*)P(16), *vflags = (uint8_t*)P(17);
  int32_t *offsets = (int32_t*)P(18), *ids = (int32_t*)P(19);
  const int n = 10, K = 2, nv = 8, nf = 4;
  const float nan = std::nanf(""), inf = INFINITY;
  const size_t need = ctd_mesh_robust_workspace_bytes(K, n);
  EXPECT((int)(need > 0 && need % 256 == 0 && need <= 4096), 1);
  EXPECT((int)ctd_mesh_robust_workspace_bytes(0, n), 0);
  EXPECT((int)ctd_mesh_robust_workspace_bytes(65, n), 0);
  EXPECT((int)ctd_mesh_robust_workspace_bytes(K, -1), 0);
  EXPECT((int)ctd_mesh_robust_workspace_bytes(K, 0), 0);
  EXPECT((int)ctd_mesh_robust_workspace_bytes(64, 1 << 24), 0);
  EXPECT((int)ctd_mesh_robust_workspace_bytes(INT32_MIN, INT32_MAX), 0);
  // the arguments of a good call, one of them replaced at a time
  struct A {
    const float* points; int n; const float* R; const float* t; int K; const float* verts; int nv; const int* faces; int nf;
    const void* bvh; int metric; float max_d2; const int32_t* hint; int kernel; const float* scale; const uint8_t* rim;
    const float* normals; float min_cos; double* sys; int32_t* face; float* residual; float* weight; int8_t* status;
    float* closest; void* ws; size_t nws;
  };
  const A good = {points, n, R, t, K, verts, nv, faces, nf, bvh, 0, inf, hint, 2, scale, rim, normals, 0.f, sys, face,
                  residual, weight, status, closest, ws, need};
  auto call = [](const A& a) {
    return ctd_mesh_robust_system_f32(a.points, a.n, a.R, a.t, a.K, a.verts, a.nv, a.faces, a.nf, a.bvh, a.metric, a.max_d2,
                                      a.hint, a.kernel, a.scale, a.rim, a.normals, a.min_cos, a.sys, a.face, a.residual,
                                      a.weight, a.status, a.closest, a.ws, a.nws, -1, nullptr);
  };
#define WITH(change) [&] { A a = good; change; return call(a); }()
  // sizes, in their order
  EXPECT(WITH(a.n = -1), 1);
  EXPECT(WITH(a.nv = -1), 1);
  EXPECT(WITH(a.nf = -1), 1);
  EXPECT(WITH(a.n = a.K = a.nv = a.nf = INT32_MIN), 1);
  const int bad_K[] = {0, -1, 65, INT32_MAX, INT32_MIN};
  for (int k : bad_K) EXPECT(WITH(a.K = k), 1);
  EXPECT(WITH(a.n = 1 << 30; a.K = 1), 1);
  EXPECT(WITH(a.n = INT32_MAX; a.K = 64), 1);
  EXPECT(WITH(a.nf = (1 << 28) + 1), 1);
  // the metric, the kernel, the cutoff and the cosine
  const int bad_code[] = {-1, 3, INT32_MAX, INT32_MIN};
  for (int v : bad_code) {
    EXPECT(WITH(a.metric = v), 1);
    EXPECT(WITH(a.kernel = v), 1);
  }
  EXPECT(WITH(a.metric = 2), 1);
  const float bad_max[] = {nan, -nan, -inf, -1.f, -1e-45f};
  for (float v : bad_max) {
    EXPECT(WITH(a.max_d2 = v), 1);
    EXPECT(WITH(a.max_d2 = v; a.n = 0; a.metric = 1), 1);
  }
  const float bad_cos[] = {nan, -nan, inf, -inf, 1.0000001f, -1.0000001f, 2.f};
  for (float v : bad_cos) {
    EXPECT(WITH(a.min_cos = v), 1);
    EXPECT(WITH(a.min_cos = v; a.normals = nullptr), 1);
  }
  // pointers
  EXPECT(WITH(a.points = nullptr), 1);
  EXPECT(WITH(a.R = nullptr), 1);
  EXPECT(WITH(a.t = nullptr), 1);
  EXPECT(WITH(a.sys = nullptr), 1);
  EXPECT(WITH(a.sys = nullptr; a.n = 0), 1);
  EXPECT(WITH(a.scale = nullptr), 1);
  EXPECT(WITH(a.scale = nullptr; a.kernel = 1), 1);
  EXPECT(WITH(a.verts = nullptr), 1);
  EXPECT(WITH(a.faces = nullptr), 1);
  EXPECT(WITH(a.bvh = (char*)bvh + 4), 1);
  EXPECT(WITH(a.bvh = (char*)bvh + 8), 1);
  // overlap: an output on an input, on another output, on the workspace, this round's faces on its hint
  EXPECT(WITH(a.sys = (double*)R), 1);
  EXPECT(WITH(a.face = (int32_t*)points), 1);
  EXPECT(WITH(a.residual = (float*)face + 19), 1);
  EXPECT(WITH(a.closest = (float*)ws), 1);
  EXPECT(WITH(a.face = (int32_t*)hint), 1);
  EXPECT(WITH(a.ws = faces), 1);
  EXPECT(WITH(a.weight = (float*)scale + 1), 1);
  EXPECT(WITH(a.status = (int8_t*)rim + 3), 1);
  EXPECT(WITH(a.status = (int8_t*)normals + 119), 1);
  EXPECT(WITH(a.weight = (float*)status + 4), 1);
  EXPECT(WITH(a.scale = (float*)sys + 115), 1);
  EXPECT(WITH(a.rim = (uint8_t*)closest + 239), 1);
  EXPECT(WITH(a.normals = residual), 1);
  // the workspace, last
  EXPECT(WITH(a.ws = nullptr), 2);
  EXPECT(WITH(a.nws = need - 1), 2);
  EXPECT(WITH(a.ws = (char*)ws + 16), 2);
  EXPECT(WITH(a.nws = 0; a.hint = nullptr; a.face = nullptr; a.residual = nullptr; a.weight = nullptr; a.status = nullptr;
              a.closest = nullptr; a.kernel = 0; a.scale = nullptr; a.rim = nullptr; a.normals = nullptr), 2);
  // precedence: sizes before the codes, the codes before the cutoff, the cutoff before pointers, overlap before the workspace
  EXPECT(WITH(a.points = nullptr; a.n = -1; a.metric = 7; a.kernel = 9; a.max_d2 = nan; a.ws = nullptr; a.nws = 0), 1);
  EXPECT(WITH(a.R = nullptr; a.t = nullptr; a.sys = nullptr; a.max_d2 = -1.f; a.ws = nullptr; a.nws = 0), 1);
  EXPECT(WITH(a.face = (int32_t*)hint; a.ws = nullptr; a.nws = 0), 1);

#define RIM(faces_, nf_, nv_, off_, ids_, ninc_, vf_, rim_) ctd_mesh_face_rim_u8(faces_, nf_, nv_, off_, ids_, ninc_, vf_, rim_, -1, nullptr)
  EXPECT(RIM(faces, -1, nv, offsets, ids, 12, vflags, rim), 1);
  EXPECT(RIM(faces, nf, -1, offsets, ids, 12, vflags, rim), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, -1, vflags, rim), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, INT64_MIN, vflags, rim), 1);
  EXPECT(RIM(faces, INT32_MIN, INT32_MIN, offsets, ids, 12, vflags, rim), 1);
  EXPECT(RIM(faces, (1 << 28) + 1, nv, offsets, ids, 12, vflags, rim), 1);
  EXPECT(RIM(nullptr, nf, nv, offsets, ids, 12, vflags, rim), 1);
  EXPECT(RIM(faces, nf, nv, nullptr, ids, 12, vflags, rim), 1);
  EXPECT(RIM(faces, nf, nv, offsets, nullptr, 12, vflags, rim), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, 12, nullptr, rim), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, 12, vflags, nullptr), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, 12, vflags, (uint8_t*)faces + 47), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, 12, vflags, (uint8_t*)offsets + 35), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, 12, vflags, (uint8_t*)ids + 47), 1);
  EXPECT(RIM(faces, nf, nv, offsets, ids, 12, vflags, vflags + 7), 1);
  EXPECT(RIM(nullptr, 0, nv, nullptr, nullptr, 0, nullptr, nullptr), 0);         // nothing to do: CTD_OK before any HIP call
  return report();
}
