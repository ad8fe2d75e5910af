// point_cloud_args_check.cpp -- the argument validation of csrc/point_cloud.hip (include/ext/ctd_hip_point_cloud.h) under
// host sanitizers: a stand-alone program with its own main that walks the rejections of the five entry points with host
// buffers standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/point_cloud.hip \
//         tools/point_cloud_args_check.cpp -o tools/bin/point_cloud_args_check && tools/bin/point_cloud_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ext/ctd_hip_point_cloud.h"
#include "args_check.h"
int main() {
  const Arena P(4096, 10);
  float *f0 = (float*)P(0), *f4 = (float*)P(4), *f6 = (float*)P(6);
  int32_t *i1 = (int32_t*)P(1), *i3 = (int32_t*)P(3), *i5 = (int32_t*)P(5);
  int64_t* k2 = (int64_t*)P(2);
  const float nan = std::nanf(""), inf = INFINITY;
  const int big = 1 << 21;

  // ---- ctd_point_cell_keys_f32: points P0 (10 x 12 bytes) -> keys P2 (10 x 8 bytes)
  auto keys = [&](const float* pts, int n, float ox, float cell, int64_t* out) {
    return ctd_point_cell_keys_f32(pts, n, ox, 0.f, 0.f, cell, out, -1, nullptr);
  };
  EXPECT(keys(f0, -1, 0.f, 0.5f, k2), 1);
  EXPECT(keys(f0, INT32_MIN, 0.f, 0.5f, k2), 1);
  const float bad_cell[] = {0.f, -0.f, -1.f, nan, -nan, inf, -inf, -1e-45f};
  for (float v : bad_cell) {
    EXPECT(keys(f0, 10, 0.f, v, k2), 1);
    EXPECT(keys(nullptr, 0, 0.f, v, nullptr), 1);              // before the n == 0 exit
  }
  const float bad_origin[] = {nan, inf, -inf};
  for (float v : bad_origin) EXPECT(keys(f0, 10, v, 0.5f, k2), 1);
  EXPECT(keys(nullptr, 10, 0.f, 0.5f, k2), 1);
  EXPECT(keys(f0, 10, 0.f, 0.5f, nullptr), 1);
  EXPECT(keys(f0, 10, 0.f, 0.5f, (int64_t*)f0), 1);
  EXPECT(keys(f0, 10, 0.f, 0.5f, (int64_t*)((char*)f0 + 112)), 1);
  EXPECT(keys(f0, 10, 0.f, 0.5f, (int64_t*)((char*)f0 - 72)), 1);
  EXPECT(keys(nullptr, 0, 0.f, 0.5f, nullptr), 0);            // nothing to do
  EXPECT(keys(f0, 10, 0.f, 1e-45f, nullptr), 1);              // the smallest cell passes: the NULL answers

  // ---- ctd_point_knn_f32
  struct A {
    const float* pts; const int32_t* order; int ns; const int64_t* keys; const int32_t* start; int nc, dx, dy, dz;
    float ox, oy, oz, cell; const float* queries; int nq, k; float md2; int32_t* idx; float* d2;
  };
  const A good = {f0, i1, 10, k2, i3, 4, 3, 4, 5, 0.f, 0.f, 0.f, 0.5f, f4, 7, 16, inf, i5, f6};
  auto knn = [](const A& a) {
    return ctd_point_knn_f32(a.pts, a.order, a.ns, a.keys, a.start, a.nc, a.dx, a.dy, a.dz, a.ox, a.oy, a.oz, a.cell, a.queries,
                             a.nq, a.k, a.md2, a.idx, a.d2, -1, nullptr);
  };
#define WITH(change) [&] { A a = good; change; return knn(a); }()
  const int bad_count[] = {-1, INT32_MIN};
  for (int v : bad_count) {
    EXPECT(WITH(a.ns = v), 1);
    EXPECT(WITH(a.nc = v), 1);
    EXPECT(WITH(a.nq = v), 1);
  }
  EXPECT(WITH(a.nc = 11), 1);                                  // more cells than points
  EXPECT(WITH(a.nc = 0), 1);                                   // points without a cell
  EXPECT(WITH(a.ns = 0), 1);
  const int bad_k[] = {0, -1, 65, INT32_MAX, INT32_MIN};
  for (int v : bad_k) EXPECT(WITH(a.k = v), 1);
  const int bad_dim[] = {0, -1, big + 1, INT32_MAX, INT32_MIN};
  for (int v : bad_dim) {
    EXPECT(WITH(a.dx = v), 1);
    EXPECT(WITH(a.dy = v), 1);
    EXPECT(WITH(a.dz = v), 1);
  }
  for (float v : bad_cell) EXPECT(WITH(a.cell = v), 1);
  for (float v : bad_origin) {
    EXPECT(WITH(a.ox = v), 1);
    EXPECT(WITH(a.oy = v), 1);
    EXPECT(WITH(a.oz = v), 1);
  }
  const float bad_md2[] = {nan, -nan, -1.f, -inf, -1e-45f};
  for (float v : bad_md2) EXPECT(WITH(a.md2 = v), 1);
  EXPECT(WITH(a.nq = 1 << 27), 3);                             // 2^27 * 16 = 2^31
  EXPECT(WITH(a.nq = INT32_MAX; a.k = 64), 3);
  EXPECT(WITH(a.nq = INT32_MAX; a.k = 1; a.idx = nullptr), 1); // below 2^31: the NULL answers
  EXPECT(WITH(a.queries = nullptr; a.nq = 9), 1);              // the points query themselves: all of them
  EXPECT(WITH(a.idx = nullptr), 1);
  EXPECT(WITH(a.d2 = nullptr), 1);
  EXPECT(WITH(a.pts = nullptr), 1);
  EXPECT(WITH(a.order = nullptr), 1);
  EXPECT(WITH(a.keys = nullptr), 1);
  EXPECT(WITH(a.start = nullptr), 1);
  EXPECT(WITH(a.ns = 0; a.nc = 0; a.queries = nullptr; a.nq = 5; a.order = nullptr), 1);   // no cell, but order names the rows
  // overlap: idx and d2 (7 x 16 x 4 = 448 bytes each) on each other and on every input
  EXPECT(WITH(a.idx = (int32_t*)f6), 1);
  EXPECT(WITH(a.d2 = (float*)((char*)i5 + 444)), 1);
  EXPECT(WITH(a.d2 = f0), 1);
  EXPECT(WITH(a.idx = (int32_t*)((char*)i1 + 36)), 1);         // the last of the 10 order entries
  EXPECT(WITH(a.d2 = (float*)((char*)k2 + 24)), 1);
  EXPECT(WITH(a.idx = (int32_t*)((char*)i3 + 16)), 1);         // start has n_cells + 1 entries
  EXPECT(WITH(a.d2 = (float*)((char*)f4 + 80)), 1);
  EXPECT(WITH(a.idx = (int32_t*)((char*)f4 - 444)), 1);
  // precedence: counts, k, dims, grid scalars, max_d2, the size limit, the self-query count, pointers, overlap
  EXPECT(WITH(a.ns = -1; a.k = 0; a.dx = 0; a.cell = nan; a.md2 = nan; a.nq = 1 << 27; a.idx = nullptr), 1);
  EXPECT(WITH(a.k = 65; a.nq = 1 << 27), 1);
  EXPECT(WITH(a.md2 = -1.f; a.nq = 1 << 27), 1);
  EXPECT(WITH(a.nq = 1 << 27; a.idx = nullptr; a.d2 = f0), 3);
  // the limits themselves pass: the NULL idx answers; and nothing to do is CTD_OK
  EXPECT(WITH(a.dx = big; a.dy = big; a.dz = big; a.k = 64; a.md2 = 0.f; a.idx = nullptr), 1);
  EXPECT(WITH(a.k = 1; a.cell = 1e-45f; a.idx = nullptr), 1);
  EXPECT(WITH(a.nq = 0; a.idx = nullptr; a.d2 = nullptr; a.queries = nullptr; a.ns = 0; a.nc = 0), 0);
  EXPECT(WITH(a.nq = 0; a.k = 0), 1);
#undef WITH

  // ---- ctd_point_mean_dist_f32: d2 P0 (10 x 16 x 4 = 640 bytes) -> mean P4 (40 bytes)
  auto mean = [&](const float* d2, int n, int k, float* out) { return ctd_point_mean_dist_f32(d2, n, k, out, -1, nullptr); };
  EXPECT(mean(f0, -1, 16, f4), 1);
  for (int v : bad_k) EXPECT(mean(f0, 10, v, f4), 1);
  EXPECT(mean(f0, 1 << 27, 16, f4), 3);
  EXPECT(mean(f0, INT32_MAX, 64, f4), 3);
  EXPECT(mean(nullptr, 10, 16, f4), 1);
  EXPECT(mean(f0, 10, 16, nullptr), 1);
  EXPECT(mean(f0, 10, 16, f0), 1);
  EXPECT(mean(f0, 10, 16, (float*)((char*)f0 + 636)), 1);
  EXPECT(mean(f0, 10, 16, (float*)((char*)f0 - 36)), 1);
  EXPECT(mean(nullptr, 0, 16, nullptr), 0);
  EXPECT(mean(nullptr, 0, 0, nullptr), 1);

  // ---- ctd_point_normals_f32
  struct N {
    const float* pts; int n; const int32_t* idx; int k; const float* toward; int stride; float* nrm; float* var; uint8_t* ok;
    double* cov;
  };
  const N fine = {f0, 10, i1, 16, f4, 3, (float*)P(5), f6, (uint8_t*)P(7), (double*)P(8)};
  auto normals = [](const N& a) {
    return ctd_point_normals_f32(a.pts, a.n, a.idx, a.k, a.toward, a.stride, a.nrm, a.var, a.ok, a.cov, -1, nullptr);
  };
#define WITH(change) [&] { N a = fine; change; return normals(a); }()
  EXPECT(WITH(a.n = -1), 1);
  for (int v : bad_k) EXPECT(WITH(a.k = v), 1);
  const int bad_stride[] = {1, 2, -3, 6, INT32_MIN};
  for (int v : bad_stride) EXPECT(WITH(a.stride = v), 1);
  EXPECT(WITH(a.n = 1 << 27), 3);
  EXPECT(WITH(a.pts = nullptr), 1);
  EXPECT(WITH(a.idx = nullptr), 1);
  EXPECT(WITH(a.nrm = nullptr), 1);
  EXPECT(WITH(a.var = nullptr), 1);
  EXPECT(WITH(a.ok = nullptr), 1);
  EXPECT(WITH(a.nrm = f0), 1);
  EXPECT(WITH(a.var = (float*)((char*)i1 + 636)), 1);
  EXPECT(WITH(a.ok = (uint8_t*)f4 + 119), 1);
  EXPECT(WITH(a.stride = 0; a.ok = (uint8_t*)f4 + 11), 1);     // one viewpoint is 12 bytes ...
  EXPECT(WITH(a.stride = 0; a.ok = (uint8_t*)f4 + 12; a.nrm = nullptr), 1);   // ... and no more: the NULL answers
  EXPECT(WITH(a.cov = (double*)((char*)P(5) + 112)), 1);       // two outputs on each other
  EXPECT(WITH(a.var = (float*)P(5)), 1);
  EXPECT(WITH(a.cov = (double*)((char*)P(7) - 712)), 1);
  EXPECT(WITH(a.toward = nullptr; a.stride = 0; a.cov = nullptr; a.nrm = nullptr), 1);   // both optional: the NULL answers
  EXPECT(WITH(a.n = 0; a.pts = nullptr; a.idx = nullptr; a.nrm = nullptr; a.var = nullptr; a.ok = nullptr; a.cov = nullptr), 0);
  EXPECT(WITH(a.stride = 1; a.n = 1 << 27; a.pts = nullptr), 1);
#undef WITH

  // ---- ctd_point_voxel_mean_f32: values P0 (10 x 3), order P1, start P3 (4 + 1 entries) -> out P4 (4 x 3 x 4 = 48 bytes)
  auto voxel = [&](const float* v, int n, int C, const int32_t* order, const int32_t* start, int m, float* out) {
    return ctd_point_voxel_mean_f32(v, n, C, order, start, m, out, -1, nullptr);
  };
  EXPECT(voxel(f0, -1, 3, i1, i3, 4, f4), 1);
  EXPECT(voxel(f0, 10, 3, i1, i3, -1, f4), 1);
  const int bad_C[] = {0, -1, 65, INT32_MAX, INT32_MIN};
  for (int v : bad_C) EXPECT(voxel(f0, 10, v, i1, i3, 4, f4), 1);
  EXPECT(voxel(f0, 1 << 30, 3, i1, i3, 4, f4), 3);
  EXPECT(voxel(f0, 10, 3, i1, i3, 1 << 30, f4), 3);
  EXPECT(voxel(nullptr, 10, 3, i1, i3, 4, f4), 1);
  EXPECT(voxel(f0, 10, 3, nullptr, i3, 4, f4), 1);
  EXPECT(voxel(f0, 10, 3, i1, nullptr, 4, f4), 1);
  EXPECT(voxel(f0, 10, 3, i1, i3, 4, nullptr), 1);
  EXPECT(voxel(f0, 10, 3, i1, i3, 4, f0), 1);
  EXPECT(voxel(f0, 10, 3, i1, i3, 4, (float*)((char*)f0 + 116)), 1);
  EXPECT(voxel(f0, 10, 3, i1, i3, 4, (float*)((char*)i3 + 16)), 1);
  EXPECT(voxel(f0, 10, 3, i1, i3, 4, (float*)((char*)i3 - 44)), 1);
  EXPECT(voxel(nullptr, 10, 3, nullptr, nullptr, 0, nullptr), 0);
  EXPECT(voxel(f0, 10, 64, i1, i3, 4, nullptr), 1);            // the largest C passes: the NULL answers
  return report();
}
