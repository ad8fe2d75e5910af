// mesh_color_args_check.cpp -- the argument validation of csrc/mesh_color.hip (include/ctd_hip_mesh_color.h) under host
// sanitizers: a stand-alone program with its own main that walks the rejections of the entry point with host buffers
// standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/mesh_color.hip \
//         tools/mesh_color_args_check.cpp -o tools/bin/mesh_color_args_check && tools/bin/mesh_color_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ctd_hip_mesh_color.h"
#include "args_check.h"

struct Args {
  float *points, *normals, *images, *K, *R, *t, *verts, *color, *weight;
  uint8_t *valid, *flags;
  int32_t *faces, *n_views;
  void* bvh;
  int n = 10, V = 3, C = 1, H = 4, W = 5, nv = 10, nf = 10, mode = 0;
  float margin = 0.01f, min_cos = 0.f;
  int call() const {
    return ctd_mesh_view_colors_f32(points, normals, n, images, valid, K, R, t, V, C, H, W, verts, nv, faces, nf, bvh, margin,
                                    min_cos, mode, color, weight, n_views, flags, -1, nullptr);
  }
};

int main() {
  const Arena P(4096, 15);
  Args a;
  a.points = (float*)P(0); a.normals = (float*)P(1); a.images = (float*)P(2); a.valid = (uint8_t*)P(3); a.K = (float*)P(4);
  a.R = (float*)P(5); a.t = (float*)P(6); a.verts = (float*)P(7); a.faces = (int32_t*)P(8); a.bvh = P(9);
  a.color = (float*)P(10); a.weight = (float*)P(11); a.n_views = (int32_t*)P(12); a.flags = (uint8_t*)P(13);
  const float nan = std::nanf(""), inf = INFINITY;
  Args b;
  // CTD_ERR_INVALID_ARG
  b = a; b.n = -1; EXPECT(b.call(), 1);
  b = a; b.n = INT32_MIN; EXPECT(b.call(), 1);
  b = a; b.nv = -1; EXPECT(b.call(), 1);
  b = a; b.nf = -1; EXPECT(b.call(), 1);
  b = a; b.V = 0; EXPECT(b.call(), 1);
  b = a; b.V = 65; EXPECT(b.call(), 1);
  b = a; b.V = INT32_MAX; EXPECT(b.call(), 1);
  b = a; b.C = 0; EXPECT(b.call(), 1);
  b = a; b.C = 5; EXPECT(b.call(), 1);
  b = a; b.H = 1; EXPECT(b.call(), 1);
  b = a; b.W = 1; EXPECT(b.call(), 1);
  b = a; b.W = INT32_MIN; EXPECT(b.call(), 1);
  b = a; b.mode = 2; EXPECT(b.call(), 1);
  b = a; b.mode = -1; EXPECT(b.call(), 1);
  for (float m : {-1e-3f, nan, inf, -inf}) { b = a; b.margin = m; EXPECT(b.call(), 1); }
  for (float c : {-0.1f, 1.f, 2.f, nan, inf, -inf}) { b = a; b.min_cos = c; EXPECT(b.call(), 1); }
  b = a; b.points = nullptr; EXPECT(b.call(), 1);
  b = a; b.images = nullptr; EXPECT(b.call(), 1);
  b = a; b.K = nullptr; EXPECT(b.call(), 1);
  b = a; b.R = nullptr; EXPECT(b.call(), 1);
  b = a; b.t = nullptr; EXPECT(b.call(), 1);
  b = a; b.color = nullptr; EXPECT(b.call(), 1);
  b = a; b.weight = nullptr; EXPECT(b.call(), 1);
  b = a; b.n_views = nullptr; EXPECT(b.call(), 1);
  b = a; b.faces = nullptr; EXPECT(b.call(), 1);
  b = a; b.verts = nullptr; EXPECT(b.call(), 1);
  b = a; b.bvh = (char*)a.bvh + 4; EXPECT(b.call(), 1);
  b = a; b.bvh = (char*)a.bvh + 8; EXPECT(b.call(), 1);
  b = a; b.n = 0; b.nf = -1; EXPECT(b.call(), 1);
  b = a; b.n = 0; b.margin = nan; EXPECT(b.call(), 1);
  // CTD_ERR_UNSUPPORTED, after the class above
  b = a; b.H = (1 << 24) + 1; b.W = 2; EXPECT(b.call(), 3);
  b = a; b.W = (1 << 24) + 1; b.H = 2; EXPECT(b.call(), 3);
  b = a; b.H = INT32_MAX; b.W = INT32_MAX; EXPECT(b.call(), 3);
  b = a; b.V = 64; b.C = 4; b.H = 1 << 12; b.W = 1 << 11; EXPECT(b.call(), 3);
  b = a; b.n = (int)((1ll << 31) / 3 + 1); b.V = 1; EXPECT(b.call(), 3);
  b = a; b.n = 1 << 25; b.V = 64; EXPECT(b.call(), 3);
  b = a; b.n = INT32_MAX; EXPECT(b.call(), 3);
  b = a; b.nf = (1 << 28) + 1; EXPECT(b.call(), 3);
  b = a; b.nf = INT32_MAX; b.nv = INT32_MAX; EXPECT(b.call(), 3);
  b = a; b.V = 65; b.H = (1 << 24) + 1; EXPECT(b.call(), 1);
  // an output overlapping any other buffer of the call: last
  b = a; b.color = a.points; EXPECT(b.call(), 1);
  b = a; b.weight = a.images + 4; EXPECT(b.call(), 1);
  b = a; b.n_views = (int32_t*)a.R; EXPECT(b.call(), 1);
  b = a; b.flags = (uint8_t*)a.t; EXPECT(b.call(), 1);
  b = a; b.color = a.weight; EXPECT(b.call(), 1);
  b = a; b.flags = (uint8_t*)a.color + 36; EXPECT(b.call(), 1);
  b = a; b.weight = a.K + 8; EXPECT(b.call(), 1);
  b = a; b.color = a.verts + 25; EXPECT(b.call(), 1);
  b = a; b.weight = (float*)a.faces; EXPECT(b.call(), 1);
  b = a; b.flags = a.valid + 59; EXPECT(b.call(), 1);
  b = a; b.color = a.normals; EXPECT(b.call(), 1);
  b = a; b.n_views = (int32_t*)((char*)a.bvh + 64); EXPECT(b.call(), 1);
  b = a; b.H = (1 << 24) + 1; b.color = a.points; EXPECT(b.call(), 3);
  // nothing to do: CTD_OK before any HIP call
  b = a; b.n = 0; EXPECT(b.call(), 0);
  b = a; b.n = 0; b.bvh = nullptr; b.flags = nullptr; b.normals = nullptr; b.valid = nullptr; EXPECT(b.call(), 0);
  b = a; b.n = 0; b.nf = 0; b.points = b.images = b.K = b.R = b.t = b.color = b.weight = b.verts = nullptr; b.n_views = nullptr;
  b.faces = nullptr; EXPECT(b.call(), 0);
  return report();
}
