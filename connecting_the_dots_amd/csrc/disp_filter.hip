// disp_filter.hip -- post-filters of a disparity map [frames][H][W] (ctd_disp_components_f32, ctd_disp_speckle_f32,
// ctd_disp_median_f32; the rules are stated word for word in include/ctd_hip.h).
//
// Connected components by union-find with integer atomics.  parent[] holds in-frame linear indices; a parent is never
// larger than its child and a larger root is always hung under a smaller one (atomic min), so when all unions are done
// the root of a set is its smallest index, whatever order the atomics landed in.  Every traversal may read a stale
// parent: an older parent is still an ancestor in the same set, and the returning atomic min decides, so staleness costs
// iterations, never the result.
//   cc_tile_kernel    -- a 64 x 16 tile, thread = pixel, wavefront = tile row.  Row runs by one ballot of the "linked to
//     my left neighbour" bits (label = the first lane of the maximal chain of set bits); runs are joined upwards (and
//     diagonally for connectivity 8) by union-find in LDS, skipping a link that two neighbours' links already imply;
//     flattened, the labels go out as in-frame indices, the dead pixels as -1, and the counters are zeroed.
//   cc_seam_kernel    -- thread = pixel next to a tile border: the links that cross the border, in global memory.
//   cc_flatten_kernel -- thread = pixel: the root (path halving on the way), and one integer atomic add on the root's
//     counter per run of equal roots inside the wavefront.
//   cc_finish_kernel  -- thread = pixel: size = the root's counter, keep = size > max_size.
// Traffic per pixel: 5 B read + 8 B written (tile), 4 + 4 (flatten, plus the chain), 8 read + 4 or 1 written (finish).
//
// disp_median_kernel<WIN> -- a 32 x 8 tile with its halo in LDS, dead pixels as NaN; a thread holds its WIN x WIN taps
//   in registers and selects by counting ranks (ties in window raster order; a NaN tap compares false, so dead taps
//   never take part).
#include "ctd_common.h"
#include "ctd_union_find.h"

namespace ctd {
namespace {

constexpr int kTW = 64, kTH = 16, kTile = kTW * kTH;          // labelling tile
constexpr int kMW = 32, kMH = 8;                              // median tile

__device__ inline float dead_value() { return __builtin_nanf(""); }

// the disparity of a live pixel, NaN for every other one
__device__ inline float load_live(const float* __restrict__ disp, const uint8_t* __restrict__ valid, size_t g) {
  const float v = disp[g];
  return ((!valid || valid[g]) && fabsf(v) < __builtin_inff()) ? v : dead_value();
}

// both live (a dead pixel is NaN and fails the compare) and within max_diff: one f32 subtraction
__device__ inline bool linked(float a, float b, float max_diff) { return fabsf(a - b) <= max_diff; }

// uf_find, uf_union, uf_count_runs and the scopes kWg, kAgent: ctd_union_find.h (shared with mesh_clean.hip)

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTile) void cc_tile_kernel(const float* __restrict__ disp, const uint8_t* __restrict__ valid,
                                                        int* __restrict__ parent, int* __restrict__ count, int H, int W,
                                                        int tiles_x, int tiles, float max_diff, int conn8) {
  __shared__ float sd[kTile];
  __shared__ int sl[kTile];
  __shared__ unsigned long long sbits[kTH];                   // per tile row: the "linked left" bits
  const int t = threadIdx.x, c = t & (kTW - 1), r = t / kTW;
  const int tile = blockIdx.x % tiles;
  const size_t fo = (size_t)(blockIdx.x / tiles) * H * W;
  const int x0 = (tile % tiles_x) * kTW, y0 = (tile / tiles_x) * kTH;
  const int x = x0 + c, y = y0 + r;
  const bool in = x < W && y < H;
  const size_t g = fo + (size_t)y * W + x;
  const float d = in ? load_live(disp, valid, g) : dead_value();
  sd[t] = d;

  const float dl = __shfl_up(d, 1);
  const bool ll = c > 0 && linked(d, dl, max_diff);
  const unsigned long long lb = __ballot(ll);
  if (c == 0) sbits[r] = lb;
  const unsigned long long stops = ~lb & ((2ull << c) - 1ull);   // lanes <= c that start a run (bit 0 is always set)
  sl[t] = r * kTW + (63 - __clzll(stops));
  __syncthreads();

  // links to the row above.  A link is skipped when two links that are made anyway imply it.
  const bool up = r > 0;
  const bool lu = up && linked(d, sd[up ? t - kTW : t], max_diff);
  const unsigned long long ub = __ballot(lu);
  const unsigned long long pb = up ? sbits[r - 1] : 0ull;      // "linked left" of the row above
  const bool left_up = ll && ((ub >> (c - 1)) & 1);            // (r, c) ~ (r, c-1) ~ (r-1, c-1)
  if (lu && !(left_up && ((pb >> c) & 1))) uf_union<kWg>(sl, t, t - kTW);
  if (conn8 && up) {
    const bool lul = c > 0 && linked(d, sd[c > 0 ? t - kTW - 1 : t], max_diff);
    const bool lur = c < kTW - 1 && linked(d, sd[c < kTW - 1 ? t - kTW + 1 : t], max_diff);
    if (lul && !((lu && ((pb >> c) & 1)) || left_up)) uf_union<kWg>(sl, t, t - kTW - 1);
    if (lur) {
      const int c1 = c + 1;                                    // (r-1, c+1) ~ (r-1, c) ~ (r, c), or through (r, c+1)
      const bool implied = (lu && ((pb >> c1) & 1)) || (((lb >> c1) & 1) && ((ub >> c1) & 1));
      if (!implied) uf_union<kWg>(sl, t, t - kTW + 1);
    }
  }
  __syncthreads();

  if (in) {
    const int rt = uf_find<kWg>(sl, t);
    parent[g] = d == d ? (y0 + rt / kTW) * W + x0 + (rt & (kTW - 1)) : -1;
    count[g] = 0;
  }
}

// the links of pixel p = (x, y) to q = (xq, yq) across a tile border; parent and disp point at the frame
__device__ inline void seam_link(const float* __restrict__ disp, const uint8_t* __restrict__ valid, int* parent, int W,
                                 int x, int y, int xq, int yq, float max_diff) {
  const size_t p = (size_t)y * W + x, q = (size_t)yq * W + xq;
  if (linked(load_live(disp, valid, p), load_live(disp, valid, q), max_diff)) uf_union<kAgent>(parent, (int)p, (int)q);
}

__global__ __launch_bounds__(256) void cc_seam_kernel(const float* __restrict__ disp, const uint8_t* __restrict__ valid,
                                                      int* parent, int H, int W, long per_frame, long total,
                                                      float max_diff, int conn8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const size_t fo = (size_t)(i / per_frame) * H * W;
  long s = i % per_frame;
  disp += fo;
  if (valid) valid += fo;
  parent += fo;
  const long across = (long)((H - 1) / kTH) * W;               // pixels below a horizontal border
  if (s < across) {
    const int x = (int)(s % W), y = (int)(s / W + 1) * kTH;
    seam_link(disp, valid, parent, W, x, y, x, y - 1, max_diff);
    if (conn8) {
      if (x > 0) seam_link(disp, valid, parent, W, x, y, x - 1, y - 1, max_diff);
      if (x + 1 < W) seam_link(disp, valid, parent, W, x, y, x + 1, y - 1, max_diff);
    }
  } else {                                                     // pixels right of a vertical border
    s -= across;
    const int y = (int)(s % H), x = (int)(s / H + 1) * kTW;
    seam_link(disp, valid, parent, W, x, y, x - 1, y, max_diff);
    if (conn8 && y > 0) {
      seam_link(disp, valid, parent, W, x, y, x - 1, y - 1, max_diff);
      seam_link(disp, valid, parent, W, x - 1, y, x, y - 1, max_diff);
    }
  }
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(int* parent, int* __restrict__ root, int* count, long plane,
                                                         long pixels) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  long key = -1;                                               // the root as an index into the whole batch
  if (g < pixels) {
    const long fo = g / plane * plane;
    int rt = -1;
    if (parent[g] >= 0) {
      rt = uf_find<kAgent>(parent + fo, (int)(g - fo));
      key = fo + rt;
    }
    root[g] = rt;
  }
  uf_count_runs(count, key);                                   // one add per run of equal roots inside the wavefront
}

__global__ __launch_bounds__(256) void cc_finish_kernel(const int* __restrict__ root, const int* __restrict__ count,
                                                        int* __restrict__ size, uint8_t* __restrict__ keep, long plane,
                                                        long pixels, int max_size) {
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= pixels) return;
  const int rt = root[g];
  const int n = rt >= 0 ? count[g / plane * plane + rt] : 0;
  if (size) size[g] = n;
  if (keep) keep[g] = rt >= 0 && n > max_size ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------
template <int WIN>
__global__ __launch_bounds__(kMW* kMH) void disp_median_kernel(const float* __restrict__ disp,
                                                               const uint8_t* __restrict__ valid, float* __restrict__ out,
                                                               uint8_t* __restrict__ valid_out, int H, int W, int tiles_x,
                                                               int tiles, int fill_min) {
  constexpr int R = WIN / 2, LW = kMW + 2 * R, LH = kMH + 2 * R, K = WIN * WIN;
  __shared__ float s[LH * LW];
  const int t = threadIdx.x;
  const int tile = blockIdx.x % tiles;
  const size_t fo = (size_t)(blockIdx.x / tiles) * H * W;
  const int x0 = (tile % tiles_x) * kMW, y0 = (tile / tiles_x) * kMH;
  for (int i = t; i < LH * LW; i += kMW * kMH) {
    const int gx = x0 - R + i % LW, gy = y0 - R + i / LW;
    s[i] = gx >= 0 && gx < W && gy >= 0 && gy < H ? load_live(disp, valid, fo + (size_t)gy * W + gx) : dead_value();
  }
  __syncthreads();
  const int c = t % kMW, r = t / kMW, x = x0 + c, y = y0 + r;
  if (x >= W || y >= H) return;

  float v[K];
  int m = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = s[(r + k / WIN) * LW + c + k % WIN];
    m += v[k] == v[k] ? 1 : 0;
  }
  float o = dead_value();
  const bool centre_live = v[K / 2] == v[K / 2];
  const bool ok = centre_live || (fill_min > 0 && m >= fill_min);
  if (ok) {
    const int want = (m - 1) / 2;                              // the lower median
#pragma unroll
    for (int i = 0; i < K; ++i) {
      int rank = 0;                                            // position of tap i in the stable ascending order
#pragma unroll
      for (int j = 0; j < K; ++j)
        if (j != i) rank += (j < i ? v[j] <= v[i] : v[j] < v[i]) ? 1 : 0;
      if (v[i] == v[i] && rank == want) o = v[i];
    }
  }
  const size_t g = fo + (size_t)y * W + x;
  out[g] = o;
  valid_out[g] = ok ? 1 : 0;
}

template <int WIN>
int launch_median(const float* disp, const uint8_t* valid, float* out, uint8_t* valid_out, int frames, int H, int W,
                  int fill_min, hipStream_t stream) {
  const int tiles_x = ceil_div(W, kMW), tiles = tiles_x * ceil_div(H, kMH);
  disp_median_kernel<WIN><<<dim3((unsigned)((long)tiles * frames)), dim3(kMW * kMH), 0, stream>>>(
      disp, valid, out, valid_out, H, W, tiles_x, tiles, fill_min);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace

static bool disp_filter_supported(int frames, int H, int W) {
  // one workgroup per (frame, tile) on grid.x; the median's tiles are the smaller ones
  return (double)frames * ceil_div(W, kMW) * ceil_div(H, kMH) < 2147483648.0;
}

static size_t disp_components_workspace_ints(int frames, int H, int W) {   // parent, count, root
  return 3 * (((size_t)frames * H * W + 3) & ~(size_t)3);
}

static int disp_components_f32(const float* disp, const uint8_t* valid, float max_diff, int connectivity, int max_size,
                               int32_t* label, int32_t* size, uint8_t* keep, int frames, int H, int W, int* workspace,
                               hipStream_t stream) {
  const long plane = (long)H * W, pixels = plane * frames;
  const size_t seg = ((size_t)pixels + 3) & ~(size_t)3;
  int* parent = workspace;
  int* count = workspace + seg;
  int* root = label ? label : workspace + 2 * seg;
  const int conn8 = connectivity == 8 ? 1 : 0;
  const int tiles_x = ceil_div(W, kTW), tiles = tiles_x * ceil_div(H, kTH);
  cc_tile_kernel<<<dim3((unsigned)((long)tiles * frames)), dim3(kTile), 0, stream>>>(disp, valid, parent, count, H, W,
                                                                                     tiles_x, tiles, max_diff, conn8);
  CTD_LAUNCH_CHECK();
  const long per_frame = (long)((H - 1) / kTH) * W + (long)((W - 1) / kTW) * H, total = per_frame * frames;
  if (total > 0) {
    cc_seam_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream>>>(disp, valid, parent, H, W, per_frame,
                                                                                    total, max_diff, conn8);
    CTD_LAUNCH_CHECK();
  }
  const unsigned blocks = (unsigned)((pixels + 255) / 256);
  cc_flatten_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(parent, root, count, plane, pixels);
  CTD_LAUNCH_CHECK();
  if (size || keep) {
    cc_finish_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(root, count, size, keep, plane, pixels, max_size);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

static int disp_median_f32(const float* disp, const uint8_t* valid, int window, int fill_min, float* out,
                           uint8_t* valid_out, int frames, int H, int W, hipStream_t stream) {
  switch (window) {
    case 3: return launch_median<3>(disp, valid, out, valid_out, frames, H, W, fill_min, stream);
    case 5: return launch_median<5>(disp, valid, out, valid_out, frames, H, W, fill_min, stream);
    case 7: return launch_median<7>(disp, valid, out, valid_out, frames, H, W, fill_min, stream);
  }
  return CTD_ERR_INVALID_ARG;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

static bool disp_filter_args_ok(int frames, int H, int W) {
  return frames >= 0 && H > 0 && W > 0 && (double)H * W < 2147483648.0 && (double)frames * H * W < 2147483648.0;
}

static bool disp_link_args_ok(float max_diff, int connectivity) {
  return max_diff >= 0.f && (connectivity == 4 || connectivity == 8);                           // (a NaN fails >=)
}

size_t ctd_disp_components_workspace_bytes(int frames, int H, int W) {
  if (frames <= 0 || !disp_filter_args_ok(frames, H, W)) return 0;
  return sizeof(int) * disp_components_workspace_ints(frames, H, W);
}

static int disp_components_call(const float* disp, const uint8_t* valid, float max_diff, int connectivity, int max_size,
                                int32_t* label, int32_t* size, uint8_t* keep, int frames, int H, int W, void* workspace,
                                size_t workspace_bytes, int device, void* stream) {
  if (frames == 0) return CTD_OK;
  if (!disp_filter_supported(frames, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < ctd_disp_components_workspace_bytes(frames, H, W) || ((uintptr_t)workspace & 15))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disp_components_f32(disp, valid, max_diff, connectivity, max_size, label, size, keep, frames, H, W,
                             (int*)workspace, (hipStream_t)stream);
}

int ctd_disp_components_f32(const float* disp, const uint8_t* valid, float max_diff, int connectivity, int32_t* label,
                            int32_t* size, int frames, int H, int W, void* workspace, size_t workspace_bytes, int device,
                            void* stream) {
  if (!disp_filter_args_ok(frames, H, W) || !disp_link_args_ok(max_diff, connectivity)) return CTD_ERR_INVALID_ARG;
  if (!disp || !label || !size) return CTD_ERR_INVALID_ARG;
  return disp_components_call(disp, valid, max_diff, connectivity, 0, label, size, nullptr, frames, H, W, workspace,
                              workspace_bytes, device, stream);
}

int ctd_disp_speckle_f32(const float* disp, const uint8_t* valid, float max_diff, int max_size, int connectivity,
                         uint8_t* keep, int32_t* size, int frames, int H, int W, void* workspace, size_t workspace_bytes,
                         int device, void* stream) {
  if (!disp_filter_args_ok(frames, H, W) || !disp_link_args_ok(max_diff, connectivity) || max_size < 0)
    return CTD_ERR_INVALID_ARG;
  if (!disp || !keep) return CTD_ERR_INVALID_ARG;
  return disp_components_call(disp, valid, max_diff, connectivity, max_size, nullptr, size, keep, frames, H, W, workspace,
                              workspace_bytes, device, stream);
}

int ctd_disp_median_f32(const float* disp, const uint8_t* valid, int window, int fill_min, float* out, uint8_t* valid_out,
                        int frames, int H, int W, int device, void* stream) {
  if (!disp_filter_args_ok(frames, H, W) || (window != 3 && window != 5 && window != 7) || fill_min < 0)
    return CTD_ERR_INVALID_ARG;
  if (!disp || !out || !valid_out || out == disp || (const uint8_t*)valid_out == valid) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!disp_filter_supported(frames, H, W)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return disp_median_f32(disp, valid, window, fill_min, out, valid_out, frames, H, W, (hipStream_t)stream);
}

}  // extern "C"
