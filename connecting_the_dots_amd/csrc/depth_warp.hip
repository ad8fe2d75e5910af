// depth_warp.hip -- forward depth warping of a track's views into each other (ctd_depth_warp_f32) and the windowed
// disparity band around a prior with holes and edges (ctd_disparity_band_window_f32); both definitions, word for word:
// include/ctd_hip_warp.h.
//
// The warp is a scatter, the mirror of depth_fusion.hip's gathers: a source pixel knows where it lands, a target pixel
// does not know who lands on it.  The z-buffer is one 64-bit key per target pixel, (bits(z) << 32) | (s*H*W + q):
// positive finite f32 bit patterns order as unsigned integers, so an unsigned minimum picks the nearest surface and, among
// equal depths, the smaller in-track source index.  A minimum does not depend on the order of its operands: the same
// bits on every run, whatever order the workgroups arrive in.
//   the keys are set to all-ones (no finite z has the bits 0xffffffff) by hipMemsetAsync on the caller's stream: 8 B / pixel;
//   warp_scatter_kernel -- 256 consecutive pixels of ONE (b, s) plane (a chunk never crosses a view, so the poses stay
//     block-uniform scalar loads, as in fuse_count_kernel), thread = source pixel, loop over the target views; per
//     candidate one plain 8-B load of the key and, unless the key already there is smaller (keys only ever decrease, so
//     a stale load can only cost an atomic, never lose one), one atomicMin.  Per source pixel 5 B + 12 B ray read; per
//     target view and splat position 8 B read and at most 8 B of atomic.
//   warp_resolve_kernel -- thread = target pixel: 8 B read, 4 B (z) + 8 B (src) written.
//
// band_window_kernel -- a 64 x 4 pixel tile plus a halo of k = window / 2 in LDS as two planes, a hole (a non-finite
// prior, a pixel outside the image) as +inf in the plane of the minimum and -inf in the plane of the maximum; minimum
// and maximum are separable: rows first (into two more planes of 64 columns), then columns.  Per pixel 4 B read (plus
// the halo's share), 8 B written.  No atomics.
#include "../../include/ctd_hip_warp.h"
#include "ctd_common.h"
#include "ctd_validate.h"
#include "ctd_view.h"

namespace ctd {
namespace {

constexpr int kWarpChunk = 256;                               // source pixels per workgroup of the scatter kernel
constexpr unsigned long long kNoKey = ~0ull;

template <int SPLAT>
__global__ __launch_bounds__(kWarpChunk) void warp_scatter_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ valid, const float* __restrict__ ray,
    const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ t,
    const uint8_t* __restrict__ sources, const uint8_t* __restrict__ targets, unsigned long long* keys, int V, int H,
    int W, int chunks) {
  const long plane = (long)H * W;
  const int bv = blockIdx.x / chunks, b = bv / V, s = bv % V;
  if (sources && !sources[bv]) return;
  const long p = (long)(blockIdx.x % chunks) * kWarpChunk + threadIdx.x;
  if (p >= plane) return;
  const long g = (long)bv * plane + p;
  if (!live_at(depth, valid, g)) return;
  const float d = depth[g];
  R += (long)b * V * 9;
  t += (long)b * V * 3;
  if (targets) targets += (long)b * V;
  keys += (long)b * V * plane;
  const unsigned long long low = (unsigned long long)((long)s * plane + p);       // < 2^32
  const float fs = (float)SPLAT, x_max = (float)((long)W - 1 + SPLAT), y_max = (float)((long)H - 1 + SPLAT);
  for (int r = 0; r < V; ++r) {
    if (r == s || (targets && !targets[r])) continue;
    float uvd[3];
    view_transform(ray + p * 3, d, R + s * 9, t + s * 3, R + r * 9, t + r * 3, K, uvd);
    if (!(uvd[2] > 0.f && uvd[2] < __builtin_inff())) continue;
    const float xs = floorf(uvd[0] / uvd[2] + 0.5f), ys = floorf(uvd[1] / uvd[2] + 0.5f);
    if (!(xs >= -fs && xs <= x_max && ys >= -fs && ys <= y_max)) continue;        // (a NaN fails the compares)
    const long xi = (long)xs, yi = (long)ys;                                      // |.| <= 2^31 + 2: no overflow
    const unsigned long long key = ((unsigned long long)__float_as_uint(uvd[2]) << 32) | low;
    unsigned long long* kr = keys + r * plane;
#pragma unroll
    for (int dy = -SPLAT; dy <= SPLAT; ++dy) {
      const long y = yi + dy;
      if (y < 0 || y >= H) continue;
#pragma unroll
      for (int dx = -SPLAT; dx <= SPLAT; ++dx) {
        const long x = xi + dx;
        if (x < 0 || x >= W) continue;
        unsigned long long* a = kr + y * W + x;
        if (key < __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(a, key);
      }
    }
  }
}

// track = V * H * W: the low word of a key is the winner's index within its track
__global__ __launch_bounds__(256) void warp_resolve_kernel(const unsigned long long* __restrict__ keys,
                                                           float* __restrict__ z, int64_t* __restrict__ src, long n,
                                                           long track) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long key = keys[i];
  const bool hole = key == kNoKey;
  z[i] = hole ? __builtin_nanf("") : __uint_as_float((unsigned)(key >> 32));
  if (src) src[i] = hole ? (int64_t)-1 : (int64_t)(i / track * track + (long)(key & 0xffffffffull));
}

inline int warp_chunks(int H, int W) { return (int)(((long)H * W + kWarpChunk - 1) / kWarpChunk); }

// ---------------------------------------------------------------------------------------------------------------------
constexpr int kBwTW = 64, kBwTH = 4, kBwMaxK = 7;             // pixel tile of a workgroup (256 threads); window <= 15

__global__ __launch_bounds__(256) void band_window_kernel(const float* __restrict__ prior, float radius, int D, int k,
                                                          int holes, int32_t* __restrict__ lo, int32_t* __restrict__ hi,
                                                          int H, int W, int tiles_x, int tiles_y) {
  constexpr int SW_MAX = kBwTW + 2 * kBwMaxK, SH_MAX = kBwTH + 2 * kBwMaxK;
  __shared__ float sMin[SH_MAX * SW_MAX], sMax[SH_MAX * SW_MAX];  // the tile + halo: holes as +inf / -inf
  __shared__ float rMin[SH_MAX * kBwTW], rMax[SH_MAX * kBwTW];    // after the row pass
  const float inf = __builtin_inff();
  const int SW = kBwTW + 2 * k, SH = kBwTH + 2 * k, win = 2 * k + 1;
  const long HW = (long)H * W;
  const int tx = blockIdx.x % tiles_x;
  const int ty = (blockIdx.x / tiles_x) % tiles_y;
  const long f = blockIdx.x / tiles_x / tiles_y;
  const int h0 = ty * kBwTH, w0 = tx * kBwTW;
  const float* a = prior + f * HW;
  for (int i = threadIdx.x; i < SH * SW; i += 256) {
    const int y = i / SW, x = i - y * SW;
    const int gy = h0 + y - k, gx = w0 + x - k;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const float v = in ? a[(long)gy * W + gx] : inf;
    const bool finite = fabsf(v) < inf;                       // (a NaN fails the compare)
    sMin[i] = finite ? v : inf;
    sMax[i] = finite ? v : -inf;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < SH * kBwTW; i += 256) {
    const int y = i / kBwTW, x = i - y * kBwTW;
    float m = inf, M = -inf;
    for (int j = 0; j < win; ++j) {
      m = fminf(m, sMin[y * SW + x + j]);
      M = fmaxf(M, sMax[y * SW + x + j]);
    }
    rMin[i] = m;
    rMax[i] = M;
  }
  __syncthreads();
  const int lx = threadIdx.x & (kBwTW - 1), ly = threadIdx.x / kBwTW;
  if (h0 + ly >= H || w0 + lx >= W) return;
  float m = inf, M = -inf;
  for (int j = 0; j < win; ++j) {
    m = fminf(m, rMin[(ly + j) * kBwTW + lx]);
    M = fmaxf(M, rMax[(ly + j) * kBwTW + lx]);
  }
  int l = D, u = -1;                                            // the empty band
  if (radius >= 0.f) {                                          // (a NaN radius fails the compare)
    if (m < inf) {
      const float cl = ceilf(m - radius), fl = floorf(M + radius);
      l = cl <= 0.f ? 0 : (cl >= (float)D ? D : (int)cl);
      u = fl <= -1.f ? -1 : (fl >= (float)(D - 1) ? D - 1 : (int)fl);
    } else if (holes) {
      l = 0;
      u = D - 1;
    }
  }
  const long p = f * HW + (long)(h0 + ly) * W + (w0 + lx);
  lo[p] = l;
  hi[p] = u;
}

}  // namespace

static int depth_warp_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                          const float* t, const uint8_t* sources, const uint8_t* targets, int splat, float* z,
                          int64_t* src, int B, int V, int H, int W, void* workspace, hipStream_t stream) {
  const long n = (long)B * V * H * W;
  unsigned long long* keys = (unsigned long long*)workspace;
  CTD_HIP_TRY(hipMemsetAsync(keys, 0xff, 8 * (size_t)n, stream));
  const int chunks = warp_chunks(H, W);
  const dim3 grid((unsigned)((long)B * V * chunks));
  if (V > 1) {                                                  // a single view has no source: all holes
    switch (splat) {
      case 0: hipLaunchKernelGGL(warp_scatter_kernel<0>, grid, dim3(kWarpChunk), 0, stream, depth, valid, ray, K, R, t, sources, targets, keys, V, H, W, chunks); break;
      case 1: hipLaunchKernelGGL(warp_scatter_kernel<1>, grid, dim3(kWarpChunk), 0, stream, depth, valid, ray, K, R, t, sources, targets, keys, V, H, W, chunks); break;
      default: hipLaunchKernelGGL(warp_scatter_kernel<2>, grid, dim3(kWarpChunk), 0, stream, depth, valid, ray, K, R, t, sources, targets, keys, V, H, W, chunks); break;
    }
    CTD_LAUNCH_CHECK();
  }
  warp_resolve_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(keys, z, src, n, (long)V * H * W);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int disparity_band_window_f32(const float* prior, float radius, int D, int window, int holes, int32_t* lo,
                                     int32_t* hi, int N, int H, int W, hipStream_t stream) {
  const int tiles_x = ceil_div(W, kBwTW), tiles_y = ceil_div(H, kBwTH);
  band_window_kernel<<<dim3((unsigned)((long)N * tiles_y * tiles_x)), dim3(256), 0, stream>>>(
      prior, radius, D, window / 2, holes, lo, hi, H, W, tiles_x, tiles_y);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// 0 ok, else the status of the first failing check of the header's list (the pointers excepted)
static int depth_warp_shape_status(int B, int V, int H, int W) {
  if (track_shape_invalid(B, V, H, W)) return CTD_ERR_INVALID_ARG;
  const double plane = (double)H * W;
  if (V * plane >= 4294967296.0 || B * (V * plane) >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  if (!launch_ok((double)B * V * (double)warp_chunks(H, W))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_depth_warp_workspace_bytes(int B, int V, int H, int W) {
  if (B <= 0 || depth_warp_shape_status(B, V, H, W) != CTD_OK) return 0;
  return align_up(8 * (size_t)B * V * H * W, 256);
}

int ctd_depth_warp_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                       const float* t, const uint8_t* sources, const uint8_t* targets, int splat, float* z,
                       int64_t* src, int B, int V, int H, int W, void* workspace, size_t workspace_bytes, int device,
                       void* stream) {
  if (splat < 0 || splat > 2 || track_shape_invalid(B, V, H, W)) return CTD_ERR_INVALID_ARG;
  if (!depth || !ray || !K || !R || !t || !z) return CTD_ERR_INVALID_ARG;
  const int st = depth_warp_shape_status(B, V, H, W);
  if (st != CTD_OK) return st;
  if (B == 0) return CTD_OK;
  if (!workspace_ok(workspace, workspace_bytes, ctd_depth_warp_workspace_bytes(B, V, H, W))) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_warp_f32(depth, valid, ray, K, R, t, sources, targets, splat, z, src, B, V, H, W, workspace,
                        (hipStream_t)stream);
}

int ctd_disparity_band_window_f32(const float* prior, float radius, int D, int window, int holes, int32_t* lo,
                                  int32_t* hi, int N, int H, int W, int device, void* stream) {
  if ((window & 1) == 0 || window < 1 || window > 2 * kBwMaxK + 1 || holes < 0 || holes > 1 || D < 1 || H < 1 || W < 1 ||
      N < 0)
    return CTD_ERR_INVALID_ARG;
  if (!prior || !lo || !hi) return CTD_ERR_INVALID_ARG;
  static_assert(kBwTW == 64 && kBwTH == 4, "the tile of band_window_kernel is the one tiles_64x4() counts");
  if ((double)N * H * W >= 2147483648.0 || !launch_ok((double)N * tiles_64x4(H, W))) return CTD_ERR_UNSUPPORTED;
  if (N == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disparity_band_window_f32(prior, radius, D, window, holes, lo, hi, N, H, W, (hipStream_t)stream);
}

}  // extern "C"
