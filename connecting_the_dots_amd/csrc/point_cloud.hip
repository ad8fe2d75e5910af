// point_cloud.hip -- the point-cloud family (include/ext/ctd_hip_point_cloud.h states every rule word for word): cell keys,
// exact k-nearest-neighbours over the sorted grid, and the consumers of its lists.
//
// Every f32 and f64 product, sum and quotient is in the association of the header and the build never contracts them.
//   cell_keys_kernel   -- a thread per point: three IEEE divisions, three floors, one int64 store.
//   knn_kernel<K>      -- a thread per query.  The K best (d2, index) pairs live in 2 K registers, sorted; a candidate
//     that beats the last one is carried through a fully unrolled chain of K compare-exchanges.  Every index into the two
//     arrays is a compile-time constant after unrolling, so they stay in VGPRs (private_segment_fixed_size = 0 for all
//     four K; the counts are in DESIGN.md).  Queries of one wavefront are neighbours in the sorted order when the points
//     query themselves, so their candidate loads hit the same lines.
//   mean_dist_kernel, normals_kernel, voxel_mean_kernel -- a thread per row (per row and column for the means), f64 sums in
//     list order.  The Jacobi rotations are written on named scalars: nothing is indexed at run time.
// No atomics, no LDS, no workspace; every store is a plain one.
#include <cstdint>

#include "../../include/ext/ctd_hip_point_cloud.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

constexpr int kThreads = 256;
constexpr int kKnnThreads = 64;                                // uneven work per query: a workgroup is one wavefront
constexpr int kMaxK = 64;
constexpr int kCellBits = 21;
constexpr int kMaxDim = 1 << kCellBits;
constexpr int64_t kNoCell = INT64_MAX;
constexpr long kMaxGroups = (1L << 24) - 1;                    // a launch stays below 2^32 threads

__host__ __device__ inline bool finitef(float v) { return v - v == 0.f; }                   // (false for NaN and +-inf)
__device__ inline int64_t cell_key(int x, int y, int z) {
  return (int64_t)x + ((int64_t)y << kCellBits) + ((int64_t)z << (2 * kCellBits));
}

__global__ __launch_bounds__(kThreads) void cell_keys_kernel(const float* __restrict__ points, int n, float ox, float oy,
                                                             float oz, float cell, int64_t* __restrict__ keys) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const float px = points[(long)i * 3], py = points[(long)i * 3 + 1], pz = points[(long)i * 3 + 2];
  const float gx = floorf((px - ox) / cell), gy = floorf((py - oy) / cell), gz = floorf((pz - oz) / cell);
  const float lim = (float)kMaxDim;
  const bool finite = finitef(px) && finitef(py) && finitef(pz);
  const bool in = finite & (gx >= 0.f) & (gx < lim) & (gy >= 0.f) & (gy < lim) & (gz >= 0.f) & (gz < lim);
  // (compared on the floats; converted only in range)
  keys[i] = in ? cell_key((int)gx, (int)gy, (int)gz) : kNoCell;
}

// the first position in keys[lo, hi) whose key is not below v
__device__ inline int lower_bound(const int64_t* __restrict__ keys, int lo, int hi, int64_t v) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (keys[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

struct KnnArgs {
  const float* pts;                                            // sorted points [n_sorted][3]
  const int32_t* order;
  int n_sorted;
  const int64_t* keys;
  const int32_t* start;
  int n_cells, dx, dy, dz;
  float ox, oy, oz, cell;
  const float* queries;
  int n_queries, k;
  float max_d2;
  int32_t* idx;
  float* d2;
  long first;                                                  // the first query of this launch
};

// the query's g on one axis, clamped into [0, dim): the cell of the box nearest to it (q is finite; a NaN quotient of
// an overflowed difference goes to 0, any cell serves: the bound below is computed from q itself)
__device__ inline int clamped_cell(float q, float o, float cell, int dim) {
  const float g = floorf((q - o) / cell);
  return g >= (float)(dim - 1) ? dim - 1 : (g > 0.f ? (int)g : 0);
}

// The gap on one axis between the query coordinate q and every point outside the searched cells [c - r, c + r] of that
// axis, never above the true one.  A point with g >= G = c + r + 1 has fl(fl(p - o) / cell) >= G; G is an integer below
// 2^22, so the quotient before rounding is >= G (1 - 2^-24), and the difference p - o before rounding >= G cell
// (1 - 2^-24)^2: p >= o + G cell (1 - 2^-23).  A point with g <= c - r - 1 has the rounded quotient < H = c - r, so
// p < o + H cell (1 + 2^-23) in the same way.  The margin is twice that, 2^-22, plus 2^-50 of |o| + |q| for the f64
// rounding of this very expression.  No face on a side (the block reaches the end of dims there): +inf.
__device__ inline double axis_gap(float q, float o, float cell, int c, int r, int dim) {
  const double inf = __builtin_inf(), slack = (fabs((double)o) + fabs((double)q)) * 0x1p-50;
  double gap = inf;
  if (c + r + 1 <= dim - 1) {
    const double w = (double)(c + r + 1) * (double)cell;
    gap = (((double)o + w) - (double)q) - (w * 0x1p-22 + slack);
  }
  if (c - r - 1 >= 0) {
    const double w = (double)(c - r) * (double)cell;
    const double g = ((double)q - ((double)o + w)) - (w * 0x1p-22 + slack);
    gap = g < gap ? g : gap;
  }
  return gap;
}

template <int K>
__global__ __launch_bounds__(kKnnThreads) void knn_kernel(const KnnArgs a) {
  const long t = a.first + (long)blockIdx.x * kKnnThreads + threadIdx.x;
  if (t >= a.n_queries) return;
  const float inf = __builtin_inff();
  float bd[K];
  int bi[K];
#pragma unroll
  for (int j = 0; j < K; ++j) { bd[j] = inf; bi[j] = -1; }
  long row = t;
  int self = -1;
  bool live = a.n_cells > 0;
  float qx = 0.f, qy = 0.f, qz = 0.f;
  if (a.queries) {
    qx = a.queries[t * 3]; qy = a.queries[t * 3 + 1]; qz = a.queries[t * 3 + 2];
  } else {
    row = self = a.order[t];
    live = t < a.n_sorted;                                     // (the points of no cell come after the sorted ones)
    if (live) { qx = a.pts[t * 3]; qy = a.pts[t * 3 + 1]; qz = a.pts[t * 3 + 2]; }
  }
  live = live && finitef(qx) && finitef(qy) && finitef(qz);
  if (live) {
    const int cx = clamped_cell(qx, a.ox, a.cell, a.dx), cy = clamped_cell(qy, a.oy, a.cell, a.dy),
              cz = clamped_cell(qz, a.oz, a.cell, a.dz);
    const float max_d2 = a.max_d2;
    // the candidates of the cells xlo .. xhi of row (y, z), which lie in keys[from, to): from moves past them
    auto scan = [&](int xlo, int xhi, int y, int z, int& from, int to) {
      const int64_t klo = cell_key(xlo, y, z), khi = cell_key(xhi, y, z);
      const int pos = lower_bound(a.keys, from, to, klo);
      int end = pos;
      while (end < to && a.keys[end] <= khi) ++end;            // (at most xhi - xlo + 1 steps)
      from = end;
      if (end == pos) return;
      const int s1 = a.start[end];
      for (int s = a.start[pos]; s < s1; ++s) {                // a row's points are contiguous in the sorted order
        const int oi = a.order[s];
        const float dx = a.pts[(long)s * 3] - qx, dy = a.pts[(long)s * 3 + 1] - qy, dz = a.pts[(long)s * 3 + 2] - qz;
        const float d2 = ((dx * dx) + (dy * dy)) + (dz * dz);
        if (oi == self || !(d2 <= max_d2)) continue;
        if (!((d2 < bd[K - 1]) | ((d2 == bd[K - 1]) & (oi < bi[K - 1])))) continue;   // (+inf never enters)
        float cd = d2;
        int ci = oi;
#pragma unroll
        for (int j = 0; j < K; ++j) {                          // carry (cd, ci) down the sorted list
          const bool lt = (cd < bd[j]) | ((cd == bd[j]) & (ci < bi[j]));
          const float nd = lt ? cd : bd[j];
          const int ni = lt ? ci : bi[j];
          cd = lt ? bd[j] : cd;
          ci = lt ? bi[j] : ci;
          bd[j] = nd;
          bi[j] = ni;
        }
      }
    };
    for (int r = 1;; ++r) {
      // pass r: the whole block of radius 1 first, then the ring of Chebyshev radius r alone
      const int z0 = cz - r > 0 ? cz - r : 0, z1 = cz + r < a.dz - 1 ? cz + r : a.dz - 1;
      const int y0 = cy - r > 0 ? cy - r : 0, y1 = cy + r < a.dy - 1 ? cy + r : a.dy - 1;
      const int x0 = cx - r > 0 ? cx - r : 0, x1 = cx + r < a.dx - 1 ? cx + r : a.dx - 1;
      int next = 0;
      for (int z = z0; z <= z1; ++z) {
        // the cells of rows y0 .. y1 of this plane are keys[from, to): an empty plane costs these two searches
        int from = lower_bound(a.keys, next, a.n_cells, cell_key(0, y0, z));
        const int to = lower_bound(a.keys, from, a.n_cells, cell_key(0, y1 + 1, z));
        next = to;
        const bool zface = (r == 1) | (z == cz - r) | (z == cz + r);
        for (int y = y0; y <= y1 && from < to; ++y) {
          if (zface | (y == cy - r) | (y == cy + r)) {
            scan(x0, x1, y, z, from, to);
          } else {                                             // a row through the inside of the ring: its two ends
            if (cx - r >= 0) scan(cx - r, cx - r, y, z, from, to);
            if (cx + r <= a.dx - 1) scan(cx + r, cx + r, y, z, from, to);
          }
        }
      }
      // Stop?  Every unsearched point lies beyond the block on some axis, so its true distance to q is at least the
      // least of the six gaps; the f32 d2 of the rule is at least gap^2 (1 - 2^-24)^5 (two roundings of a difference
      // and its square, two sums of non-negative terms; below 1e-30 the squares may underflow: the bound is then 0).
      // A candidate enters the list only with d2 <= max_d2 and (d2, index) below the k-th: when min(k-th d2, max_d2)
      // is STRICTLY below the bound, none can, ties included.
      const double gx = axis_gap(qx, a.ox, a.cell, cx, r, a.dx), gy = axis_gap(qy, a.oy, a.cell, cy, r, a.dy),
                   gz = axis_gap(qz, a.oz, a.cell, cz, r, a.dz);
      double gap = gx < gy ? gx : gy;
      gap = gz < gap ? gz : gap;
      if (gap == __builtin_inf()) break;                       // the block covers dims
      gap = gap > 0.0 ? gap : 0.0;
      double bound = gap * gap * (1.0 - 0x1p-20);
      bound = bound < 1e-30 ? 0.0 : bound;
      float kth = bd[K - 1];
#pragma unroll
      for (int j = 0; j < K; ++j) kth = j == a.k - 1 ? bd[j] : kth;        // (uniform selects, no run-time index)
      if ((double)(kth < max_d2 ? kth : max_d2) < bound) break;
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j)
    if (j < a.k) {
      a.idx[row * a.k + j] = bi[j];
      a.d2[row * a.k + j] = bd[j];
    }
}

__global__ __launch_bounds__(kThreads) void mean_dist_kernel(const float* __restrict__ d2, int n, int k,
                                                             float* __restrict__ mean) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  int count = 0;
  for (int j = 0; j < k; ++j) {
    const float d = d2[(long)i * k + j];
    if (d < __builtin_inff()) { s += sqrt((double)d); ++count; }
  }
  mean[i] = count ? (float)(s / (double)count) : __builtin_nanf("");
}

// one Jacobi rotation that zeroes a_pq of a symmetric 3 x 3 matrix; r is the third index, (vkp, vkq) the two columns
// of the eigenvector matrix (Rutishauser's formulas)
#define CTD_JACOBI(app, aqq, apq, arp, arq, v0p, v0q, v1p, v1q, v2p, v2q)               \
  if (apq != 0.0) {                                                                     \
    const double theta = (aqq - app) / (2.0 * apq);                                     \
    const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0)); \
    const double cc = 1.0 / sqrt(tt * tt + 1.0), ss = tt * cc;                          \
    app = app - tt * apq;                                                               \
    aqq = aqq + tt * apq;                                                               \
    apq = 0.0;                                                                          \
    const double rp = cc * arp - ss * arq, rq = ss * arp + cc * arq;                    \
    arp = rp; arq = rq;                                                                 \
    const double u0 = cc * v0p - ss * v0q, w0 = ss * v0p + cc * v0q;                    \
    v0p = u0; v0q = w0;                                                                 \
    const double u1 = cc * v1p - ss * v1q, w1 = ss * v1p + cc * v1q;                    \
    v1p = u1; v1q = w1;                                                                 \
    const double u2 = cc * v2p - ss * v2q, w2 = ss * v2p + cc * v2q;                    \
    v2p = u2; v2q = w2;                                                                 \
  }

// (la, column a) and (lb, column b) change places when la > lb
#define CTD_CSWAP(la, ax, ay, az, lb, bx, by, bz)                                       \
  if (la > lb) {                                                                        \
    double t_;                                                                          \
    t_ = la; la = lb; lb = t_;                                                          \
    t_ = ax; ax = bx; bx = t_;                                                          \
    t_ = ay; ay = by; by = t_;                                                          \
    t_ = az; az = bz; bz = t_;                                                          \
  }

__global__ __launch_bounds__(kThreads) void normals_kernel(const float* __restrict__ points, int n,
                                                           const int32_t* __restrict__ idx, int k,
                                                           const float* __restrict__ toward, int toward_stride,
                                                           float* __restrict__ normals, float* __restrict__ variation,
                                                           uint8_t* __restrict__ ok, double* __restrict__ cov) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const double px = points[(long)i * 3], py = points[(long)i * 3 + 1], pz = points[(long)i * 3 + 2];
  double sx = px, sy = py, sz = pz;
  int count = 1;
  for (int j = 0; j < k; ++j) {
    const int m = idx[(long)i * k + j];
    if ((unsigned)m >= (unsigned)n) continue;
    sx += (double)points[(long)m * 3]; sy += (double)points[(long)m * 3 + 1]; sz += (double)points[(long)m * 3 + 2];
    ++count;
  }
  const double cx = sx / (double)count, cy = sy / (double)count, cz = sz / (double)count;
  double dx = px - cx, dy = py - cy, dz = pz - cz;
  double xx = dx * dx, xy = dx * dy, xz = dx * dz, yy = dy * dy, yz = dy * dz, zz = dz * dz;
  for (int j = 0; j < k; ++j) {
    const int m = idx[(long)i * k + j];
    if ((unsigned)m >= (unsigned)n) continue;
    dx = (double)points[(long)m * 3] - cx; dy = (double)points[(long)m * 3 + 1] - cy; dz = (double)points[(long)m * 3 + 2] - cz;
    xx += dx * dx; xy += dx * dy; xz += dx * dz; yy += dy * dy; yz += dy * dz; zz += dz * dz;
  }
  if (cov) {
    double* c = cov + (long)i * 9;
    c[0] = cx; c[1] = cy; c[2] = cz; c[3] = xx; c[4] = xy; c[5] = xz; c[6] = yy; c[7] = yz; c[8] = zz;
  }
  double a00 = xx, a01 = xy, a02 = xz, a11 = yy, a12 = yz, a22 = zz;
  double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
  for (int sweep = 0; sweep < 10; ++sweep) {
    CTD_JACOBI(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21)
    CTD_JACOBI(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22)
    CTD_JACOBI(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22)
  }
  double l0 = a00, l1 = a11, l2 = a22;                         // column c of v goes with l_c
  CTD_CSWAP(l0, v00, v10, v20, l1, v01, v11, v21)
  CTD_CSWAP(l1, v01, v11, v21, l2, v02, v12, v22)
  CTD_CSWAP(l0, v00, v10, v20, l1, v01, v11, v21)
  const bool good = (count >= 3) & (l1 - l0 > 1e-9 * l2);      // (a NaN fails)
  const double len = sqrt((v00 * v00 + v10 * v10) + v20 * v20);
  double nx = v00 / len, ny = v10 / len, nz = v20 / len;
  if (toward) {
    const float* tw = toward + (long)i * toward_stride;
    const double tx = (double)tw[0] - px, ty = (double)tw[1] - py, tz = (double)tw[2] - pz;
    if (((nx * tx) + (ny * ty)) + (nz * tz) < 0.0) { nx = -nx; ny = -ny; nz = -nz; }
  }
  const float nan = __builtin_nanf("");
  normals[(long)i * 3] = good ? (float)nx : nan;
  normals[(long)i * 3 + 1] = good ? (float)ny : nan;
  normals[(long)i * 3 + 2] = good ? (float)nz : nan;
  variation[i] = good ? (float)(l0 / ((l0 + l1) + l2)) : nan;
  ok[i] = good ? 1 : 0;
}

__global__ __launch_bounds__(kThreads) void voxel_mean_kernel(const float* __restrict__ values, int n, int C,
                                                              const int32_t* __restrict__ order,
                                                              const int32_t* __restrict__ start, int n_cells,
                                                              float* __restrict__ out) {
  const long t = (long)blockIdx.x * kThreads + threadIdx.x;
  if (t >= (long)n_cells * C) return;
  const int c = (int)(t / C), j = (int)(t % C);
  double s = 0.0;
  int count = 0;
  const int s1 = start[c + 1];
  for (int p = start[c]; p < s1; ++p) {
    const int m = order[p];
    if ((unsigned)m >= (unsigned)n) continue;
    s += (double)values[(long)m * C + j];
    ++count;
  }
  out[t] = (float)(s / (double)count);
}

template <int K>
int launch_knn(KnnArgs a, hipStream_t stream) {
  const long groups = ((long)a.n_queries + kKnnThreads - 1) / kKnnThreads;
  for (long first = 0; first < groups; first += kMaxGroups) {
    const long count = groups - first < kMaxGroups ? groups - first : kMaxGroups;
    a.first = first * kKnnThreads;
    knn_kernel<K><<<dim3((unsigned)count), dim3(kKnnThreads), 0, stream>>>(a);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

inline bool grid_scalars_ok(float ox, float oy, float oz, float cell) {
  return positive_finite(cell) && finitef(ox) && finitef(oy) && finitef(oz);
}
inline bool too_many(double elements) { return elements >= 2147483648.0; }

}  // namespace
}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_point_cell_keys_f32(const float* points, int n, float origin_x, float origin_y, float origin_z, float cell,
                            int64_t* keys, int device, void* stream) {
  if (n < 0) return CTD_ERR_INVALID_ARG;
  if (!grid_scalars_ok(origin_x, origin_y, origin_z, cell)) return CTD_ERR_INVALID_ARG;
  if (n == 0) return CTD_OK;
  if (!points || !keys) return CTD_ERR_INVALID_ARG;
  const Span sp[] = {{keys, 8 * (size_t)n}, {points, 12 * (size_t)n}};
  if (spans_overlap(sp, 1, 2)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  cell_keys_kernel<<<dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream>>>(points, n, origin_x, origin_y,
                                                                                           origin_z, cell, keys);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

int ctd_point_knn_f32(const float* sorted_points, const int32_t* order, int n_sorted, const int64_t* keys,
                      const int32_t* start, int n_cells, int dim_x, int dim_y, int dim_z, float origin_x, float origin_y,
                      float origin_z, float cell, const float* queries, int n_queries, int k, float max_d2, int32_t* idx,
                      float* d2, int device, void* stream) {
  if (n_sorted < 0 || n_cells < 0 || n_queries < 0 || n_cells > n_sorted || (n_cells == 0) != (n_sorted == 0))
    return CTD_ERR_INVALID_ARG;
  if (k < 1 || k > kMaxK) return CTD_ERR_INVALID_ARG;
  if (dim_x < 1 || dim_y < 1 || dim_z < 1 || dim_x > kMaxDim || dim_y > kMaxDim || dim_z > kMaxDim) return CTD_ERR_INVALID_ARG;
  if (!grid_scalars_ok(origin_x, origin_y, origin_z, cell)) return CTD_ERR_INVALID_ARG;
  if (!(max_d2 >= 0.f)) return CTD_ERR_INVALID_ARG;                                     // (a NaN fails)
  if (too_many((double)n_queries * k)) return CTD_ERR_UNSUPPORTED;
  if (!queries && n_queries < n_sorted) return CTD_ERR_INVALID_ARG;
  if (n_queries == 0) return CTD_OK;
  if (!idx || !d2) return CTD_ERR_INVALID_ARG;
  if (n_sorted > 0 && (!sorted_points || !order || !keys || !start)) return CTD_ERR_INVALID_ARG;
  if (!queries && !order) return CTD_ERR_INVALID_ARG;
  const size_t n_order = queries ? (size_t)n_sorted : (size_t)n_queries;
  const Span sp[] = {{idx, 4 * (size_t)n_queries * k}, {d2, 4 * (size_t)n_queries * k}, {sorted_points, 12 * (size_t)n_sorted},
                     {order, 4 * n_order}, {keys, 8 * (size_t)n_cells}, {start, 4 * ((size_t)n_cells + 1)},
                     {queries, 12 * (size_t)n_queries}};
  if (spans_overlap(sp, 2, 7)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  KnnArgs a = {sorted_points, order, n_sorted, keys, start, n_cells, dim_x, dim_y, dim_z, origin_x, origin_y, origin_z, cell,
               queries, n_queries, k, max_d2, idx, d2, 0};
  if (k <= 8) return launch_knn<8>(a, (hipStream_t)stream);
  if (k <= 16) return launch_knn<16>(a, (hipStream_t)stream);
  if (k <= 32) return launch_knn<32>(a, (hipStream_t)stream);
  return launch_knn<64>(a, (hipStream_t)stream);
}

int ctd_point_mean_dist_f32(const float* d2, int n, int k, float* mean, int device, void* stream) {
  if (n < 0 || k < 1 || k > kMaxK) return CTD_ERR_INVALID_ARG;
  if (too_many((double)n * k)) return CTD_ERR_UNSUPPORTED;
  if (n == 0) return CTD_OK;
  if (!d2 || !mean) return CTD_ERR_INVALID_ARG;
  const Span sp[] = {{mean, 4 * (size_t)n}, {d2, 4 * (size_t)n * k}};
  if (spans_overlap(sp, 1, 2)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  mean_dist_kernel<<<dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream>>>(d2, n, k, mean);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

int ctd_point_normals_f32(const float* points, int n, const int32_t* idx, int k, const float* toward, int toward_stride,
                          float* normals, float* variation, uint8_t* ok, double* cov, int device, void* stream) {
  if (n < 0 || k < 1 || k > kMaxK || (toward_stride != 0 && toward_stride != 3)) return CTD_ERR_INVALID_ARG;
  if (too_many((double)n * k)) return CTD_ERR_UNSUPPORTED;
  if (n == 0) return CTD_OK;
  if (!points || !idx || !normals || !variation || !ok) return CTD_ERR_INVALID_ARG;
  const Span sp[] = {{normals, 12 * (size_t)n}, {variation, 4 * (size_t)n}, {ok, (size_t)n}, {cov, 72 * (size_t)n},
                     {points, 12 * (size_t)n}, {idx, 4 * (size_t)n * k}, {toward, toward_stride ? 12 * (size_t)n : 12}};
  if (spans_overlap(sp, 4, 7)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  normals_kernel<<<dim3(ceil_div(n, kThreads)), dim3(kThreads), 0, (hipStream_t)stream>>>(points, n, idx, k, toward,
                                                                                         toward_stride, normals, variation, ok, cov);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

int ctd_point_voxel_mean_f32(const float* values, int n, int C, const int32_t* order, const int32_t* start, int n_cells,
                             float* out, int device, void* stream) {
  if (n < 0 || n_cells < 0 || C < 1 || C > 64) return CTD_ERR_INVALID_ARG;
  if (too_many((double)n * C) || too_many((double)n_cells * C)) return CTD_ERR_UNSUPPORTED;
  if (n_cells == 0) return CTD_OK;
  if (!values || !order || !start || !out) return CTD_ERR_INVALID_ARG;
  const Span sp[] = {{out, 4 * (size_t)n_cells * C}, {values, 4 * (size_t)n * C}, {start, 4 * ((size_t)n_cells + 1)}};
  if (spans_overlap(sp, 1, 3)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const long threads = (long)n_cells * C;
  voxel_mean_kernel<<<dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream>>>(
      values, n, C, order, start, n_cells, out);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // extern "C"
