// pattern_loss.hip -- fused pattern similarity loss: RectifiedPatternSimilarityLoss.tforward,
// model/networks.py:358-378, as one forward and one backward kernel, for one image size or for every level of the
// training pyramid in one launch.  Tile, block loss and its backward: ctd_photo_tile.h.
//   u1 = u - disp; gx = 2*(u1/(W-1) - 0.5); gy = 2*(v/(H-1) - 0.5)                       (:362-369)
//   pattern_proj = grid_sample(pattern, (gx, gy), bilinear, border, align_corners=False)   (:371)
//   diff = photometric_loss(pattern_proj, im, 9, type, eps); val = sum(mask*diff)/sum(mask) (:376-377)
// The warped pattern is sampled straight into the LDS tile (halo included: the block loss reads
// replicate-clamped taps of pattern_proj, i.e. the sample at the clamped pixel); it is written once because
// the module returns it.  Backward recomputes the tile, runs the pair-symmetric block-loss backward and
// applies d pattern_proj / d disp = -(W/(W-1)) * d/dix of the bilinear interpolant (0 where ATen clips).
#include "ctd_common.h"
#include "ctd_dispatch.h"
#include "ctd_photo_tile.h"
#include "ctd_validate.h"

namespace ctd {

struct WarpSample {
  float value, d_ddisp;
};

// ATen grid_sampler_2d, bilinear / border / align_corners=false, for the grid networks.py builds
__device__ inline WarpSample warp_pattern(const float* __restrict__ pat, int H, int W, int x, int y, float disp) {
  const float u1 = (float)x - disp;
  const float gx = 2.f * (u1 / (float)(W - 1) - 0.5f), gy = 2.f * ((float)y / (float)(H - 1) - 0.5f);
  float ix = ((gx + 1.f) * (float)W - 1.f) / 2.f, iy = ((gy + 1.f) * (float)H - 1.f) / 2.f;   // unnormalize
  // clip_coordinates_set_grad: gradient 0 at and beyond the borders
  float gmul = 1.f;
  if (ix <= 0.f) { ix = 0.f; gmul = 0.f; }
  else if (ix >= (float)(W - 1)) { ix = (float)(W - 1); gmul = 0.f; }
  iy = fminf(fmaxf(iy, 0.f), (float)(H - 1));
  const float fx = floorf(ix), fy = floorf(iy);
  const int x0 = (int)fx, y0 = (int)fy, x1 = x0 + 1, y1 = y0 + 1;
  const float wx1 = ix - fx, wx0 = 1.f - wx1, wy1 = iy - fy, wy0 = 1.f - wy1;
  const bool xin = x1 <= W - 1, yin = y1 <= H - 1;      // x0, y0 are inside after clipping
  const float p00 = pat[(long)y0 * W + x0];
  const float p01 = xin ? pat[(long)y0 * W + x1] : 0.f;
  const float p10 = yin ? pat[(long)y1 * W + x0] : 0.f;
  const float p11 = (xin && yin) ? pat[(long)y1 * W + x1] : 0.f;
  WarpSample r;
  r.value = p00 * (wx0 * wy0) + p01 * (wx1 * wy0) + p10 * (wx0 * wy1) + p11 * (wx1 * wy1);
  const float dv_dix = (p01 - p00) * wy0 + (p11 - p10) * wy1;
  // d ix / d gx = W/2, d gx / d u1 = 2/(W-1), d u1 / d disp = -1
  r.d_ddisp = -gmul * dv_dix * ((float)W / (float)(W - 1));
  return r;
}

template <int BS>
__device__ inline void stage_warped(float (*dst)[kPTW + BS - 1], const float* __restrict__ pat,
                                    const float* __restrict__ disp, int H, int W, int x0, int y0) {
  constexpr int HALF = BS / 2, TW = kPTW + BS - 1, TH = kPTH + BS - 1;
  for (int i = threadIdx.x; i < TW * TH; i += 256) {
    const int r = i / TW, c = i - r * TW;
    const int y = clampi(y0 + r - HALF, 0, H - 1), x = clampi(x0 + c - HALF, 0, W - 1);
    dst[r][c] = warp_pattern(pat, H, W, x, y, disp[(long)y * W + x]).value;
  }
}

// (sum mask*diff, sum mask) over the tile's pixels, fixed-order tree; the result is valid in thread 0
template <int TYPE, int BS>
__device__ inline float2 pattern_fwd_tile(const float* __restrict__ disp, const float* __restrict__ im,
                                          const float* __restrict__ mask, const float* __restrict__ pattern,
                                          float* __restrict__ proj_out, int H, int W, int x0, int y0, int n,
                                          float eps) {
  constexpr int TW = kPTW + BS - 1, TH = kPTH + BS - 1, HALF = BS / 2;
  __shared__ float sE[TH][TW], sT[TH][TW];
  __shared__ float2 red[256];
  const int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
  const long HW = (long)H * W;
  stage_warped<BS>(sE, pattern, disp + (long)n * HW, H, W, x0, y0);
  stage_tile<BS>(sT, im + (long)n * HW, H, W, x0, y0);
  __syncthreads();
  float2 acc = make_float2(0.f, 0.f);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int ty = ty0 + 4 * k, x = x0 + tx, y = y0 + ty;
    if (x < W && y < H) {
      const float diff = fwd_pixel<TYPE, BS>(sE, sT, tx, ty, eps);
      const long o = (long)n * HW + (long)y * W + x;
      const float m = mask ? mask[o] : 1.f;
      acc.x = fmaf(m, diff, acc.x);
      acc.y += m;
      proj_out[o] = sE[ty + HALF][tx + HALF];
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) {
      red[threadIdx.x].x += red[threadIdx.x + stride].x;
      red[threadIdx.x].y += red[threadIdx.x + stride].y;
    }
    __syncthreads();
  }
  return red[0];
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void pattern_loss_fwd_kernel(const float* __restrict__ disp,
                                                               const float* __restrict__ im,
                                                               const float* __restrict__ mask,
                                                               const float* __restrict__ pattern,
                                                               float* __restrict__ proj_out,
                                                               float2* __restrict__ partials, int H, int W,
                                                               float eps) {
  const float2 r = pattern_fwd_tile<TYPE, BS>(disp, im, mask, pattern, proj_out, H, W, blockIdx.x * kPTW,
                                              blockIdx.y * kPTH, blockIdx.z, eps);
  if (threadIdx.x == 0) partials[((long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
}

// ---- several pyramid levels in one launch (the training loop calls the loss once per scale on
// shrinking images, exp_synph.py:107-111; the 60x80 levels are launch-bound).  The level table travels in the
// kernel arguments; a workgroup finds its level from its linear index.
constexpr int kMaxLevels = 8;
struct PatternLevelDev {
  const float *disp, *im, *mask, *pattern, *grad_proj;
  float *proj, *grad_disp;
  int B, H, W, tiles_x, tiles_y;
  unsigned block_begin;                      // first workgroup (== first partial) of this level
};
struct PatternLevelsDev {
  PatternLevelDev lv[kMaxLevels];
  int n;
};

__device__ inline int find_level(const PatternLevelsDev& t, unsigned block, int& bx, int& by, int& n) {
  int l = 0;
#pragma unroll
  for (int k = 1; k < kMaxLevels; ++k)
    if (k < t.n && block >= t.lv[k].block_begin) l = k;
  const unsigned local = block - t.lv[l].block_begin;
  bx = (int)(local % t.lv[l].tiles_x);
  by = (int)((local / t.lv[l].tiles_x) % t.lv[l].tiles_y);
  n = (int)(local / ((unsigned)t.lv[l].tiles_x * t.lv[l].tiles_y));
  return l;
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void pattern_loss_multi_fwd_kernel(PatternLevelsDev t, float2* __restrict__ partials,
                                                                     float eps) {
  int bx, by, n;
  const int l = find_level(t, blockIdx.x, bx, by, n);
  const PatternLevelDev& L = t.lv[l];
  const float2 r = pattern_fwd_tile<TYPE, BS>(L.disp, L.im, L.mask, L.pattern, L.proj, L.H, L.W, bx * kPTW, by * kPTH, n, eps);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// one workgroup per level: terms[level][3]
__global__ __launch_bounds__(256) void pattern_loss_multi_finish_kernel(PatternLevelsDev t, unsigned total_blocks,
                                                                        const float2* __restrict__ partials,
                                                                        float* __restrict__ terms) {
  __shared__ double rx[256], ry[256];
  const int l = blockIdx.x;
  const unsigned lo = t.lv[l].block_begin, hi = l + 1 < t.n ? t.lv[l + 1].block_begin : total_blocks;
  double ax = 0, ay = 0;
  for (unsigned i = lo + threadIdx.x; i < hi; i += 256) { ax += (double)partials[i].x; ay += (double)partials[i].y; }
  rx[threadIdx.x] = ax;
  ry[threadIdx.x] = ay;
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) { rx[threadIdx.x] += rx[threadIdx.x + stride]; ry[threadIdx.x] += ry[threadIdx.x + stride]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    terms[3 * l + 0] = (float)rx[0];
    terms[3 * l + 1] = (float)ry[0];
    terms[3 * l + 2] = (float)rx[0] / (float)ry[0];
  }
}

// terms[0] = numerator, terms[1] = denominator, terms[2] = numerator / denominator; one workgroup, fixed order
__global__ __launch_bounds__(256) void pattern_loss_finish_kernel(const float2* __restrict__ partials, long n,
                                                                  float* __restrict__ terms) {
  __shared__ double rx[256], ry[256];
  double ax = 0, ay = 0;
  for (long i = threadIdx.x; i < n; i += 256) { ax += (double)partials[i].x; ay += (double)partials[i].y; }
  rx[threadIdx.x] = ax;
  ry[threadIdx.x] = ay;
  __syncthreads();
  for (int stride = 128; stride > 0; stride >>= 1) {
    if (threadIdx.x < stride) { rx[threadIdx.x] += rx[threadIdx.x + stride]; ry[threadIdx.x] += ry[threadIdx.x + stride]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    terms[0] = (float)rx[0];
    terms[1] = (float)ry[0];
    terms[2] = (float)rx[0] / (float)ry[0];
  }
}

// grad_disp = d val / d disp for val = terms[0] / terms[1]:  go[p] = grad_val * mask[p] / terms[1]
// (+ optionally grad_proj, the gradient arriving at the returned pattern_proj)
template <int TYPE, int BS>
__device__ inline void pattern_bwd_tile(const float* __restrict__ disp, const float* __restrict__ im,
                                        const float* __restrict__ mask, const float* __restrict__ pattern,
                                        float scale, const float* __restrict__ grad_proj,
                                        float* __restrict__ grad_disp, int H, int W, int x0, int y0, int n, float eps) {
  constexpr int HALF = BS / 2, TW = kPTW + BS - 1, TH = kPTH + BS - 1;
  __shared__ float sE[TH][TW], sT[TH][TW], sG[TH][TW];
  const long HW = (long)H * W;
  const float* dsp = disp + (long)n * HW;
  stage_warped<BS>(sE, pattern, dsp, H, W, x0, y0);
  stage_tile<BS>(sT, im + (long)n * HW, H, W, x0, y0);
  if (mask) {
    stage_tile<BS>(sG, mask + (long)n * HW, H, W, x0, y0);
    __syncthreads();
    for (int i = threadIdx.x; i < TW * TH; i += 256) (&sG[0][0])[i] *= scale;
  } else {
    for (int i = threadIdx.x; i < TW * TH; i += 256) (&sG[0][0])[i] = scale;
  }
  __syncthreads();
  const bool interior = x0 >= 2 * HALF && y0 >= 2 * HALF && x0 + kPTW - 1 <= W - 1 - 2 * HALF &&
                        y0 + kPTH - 1 <= H - 1 - 2 * HALF;
  auto sink = [&](int qx, int qy, float g) {
    const long o = (long)qy * W + qx;
    if (grad_proj) g += grad_proj[(long)n * HW + o];
    grad_disp[(long)n * HW + o] = g * warp_pattern(pattern, H, W, qx, qy, dsp[o]).d_ddisp;
  };
  if (interior) bwd_tile<TYPE, BS, false>(sE, sT, sG, sink, H, W, x0, y0, eps);
  else bwd_tile<TYPE, BS, true>(sE, sT, sG, sink, H, W, x0, y0, eps);
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void pattern_loss_bwd_kernel(const float* __restrict__ disp,
                                                               const float* __restrict__ im,
                                                               const float* __restrict__ mask,
                                                               const float* __restrict__ pattern,
                                                               const float* __restrict__ terms,
                                                               const float* __restrict__ grad_val,
                                                               const float* __restrict__ grad_proj,
                                                               float* __restrict__ grad_disp, int H, int W,
                                                               float eps) {
  pattern_bwd_tile<TYPE, BS>(disp, im, mask, pattern, grad_val[0] / terms[1], grad_proj, grad_disp, H, W,
                             blockIdx.x * kPTW, blockIdx.y * kPTH, blockIdx.z, eps);
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void pattern_loss_multi_bwd_kernel(PatternLevelsDev t, const float* __restrict__ terms,
                                                                     const float* __restrict__ grad_vals, float eps) {
  int bx, by, n;
  const int l = find_level(t, blockIdx.x, bx, by, n);
  const PatternLevelDev& L = t.lv[l];
  pattern_bwd_tile<TYPE, BS>(L.disp, L.im, L.mask, L.pattern, grad_vals[l] / terms[3 * l + 1], L.grad_proj, L.grad_disp,
                             L.H, L.W, bx * kPTW, by * kPTH, n, eps);
}

static size_t pattern_loss_workspace_bytes(int B, int H, int W) {
  return sizeof(float2) * (size_t)B * ceil_div(H, kPTH) * ceil_div(W, kPTW);
}

static int pattern_loss_fwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                                float* proj, float* terms, int B, int H, int W, int type, float eps, void* ws,
                                size_t ws_bytes, hipStream_t stream) {
  if (!ws || ws_bytes < pattern_loss_workspace_bytes(B, H, W)) return CTD_ERR_WORKSPACE;
  const dim3 grid(ceil_div(W, kPTW), ceil_div(H, kPTH), B);
  float2* partials = (float2*)ws;
  return dispatch_type(type, [&](auto type_c) -> int {
    hipLaunchKernelGGL((pattern_loss_fwd_kernel<decltype(type_c)::value, 9>), grid, dim3(256), 0, stream, disp, im, mask,
                       pattern, proj, partials, H, W, eps);
    CTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(pattern_loss_finish_kernel, dim3(1), dim3(256), 0, stream, partials,
                       (long)grid.x * grid.y * grid.z, terms);
    CTD_LAUNCH_CHECK();
    return CTD_OK;
  });
}

static int pattern_loss_bwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                                const float* terms, const float* grad_val, const float* grad_proj, float* grad_disp,
                                int B, int H, int W, int type, float eps, hipStream_t stream) {
  const dim3 grid(ceil_div(W, kPTW), ceil_div(H, kPTH), B);
  return dispatch_type(type, [&](auto type_c) -> int {
    hipLaunchKernelGGL((pattern_loss_bwd_kernel<decltype(type_c)::value, 9>), grid, dim3(256), 0, stream, disp, im, mask,
                       pattern, terms, grad_val, grad_proj, grad_disp, H, W, eps);
    CTD_LAUNCH_CHECK();
    return CTD_OK;
  });
}

static int build_levels(int n_levels, const ctd_pattern_level* levels, PatternLevelsDev& t, unsigned& total) {
  if (n_levels < 1 || n_levels > kMaxLevels || !levels) return CTD_ERR_INVALID_ARG;
  total = 0;
  t.n = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    const ctd_pattern_level& s = levels[l];
    if (s.B <= 0 || s.H < 2 || s.W < 2 || !s.disp || !s.im || !s.pattern) return CTD_ERR_INVALID_ARG;
    PatternLevelDev& d = t.lv[l];
    d.disp = s.disp; d.im = s.im; d.mask = s.mask; d.pattern = s.pattern; d.grad_proj = s.grad_proj;
    d.proj = s.pattern_proj; d.grad_disp = s.grad_disp;
    d.B = s.B; d.H = s.H; d.W = s.W;
    d.tiles_x = ceil_div(s.W, kPTW);
    d.tiles_y = ceil_div(s.H, kPTH);
    d.block_begin = total;
    const double blocks = (double)d.tiles_x * d.tiles_y * s.B;
    if (total + blocks >= 2147483648.0) return CTD_ERR_INVALID_ARG;
    total += (unsigned)blocks;
  }
  return CTD_OK;
}

static size_t pattern_loss_multi_workspace_bytes(int n_levels, const ctd_pattern_level* levels) {
  PatternLevelsDev t;
  unsigned total = 0;
  if (build_levels(n_levels, levels, t, total)) return 0;
  return sizeof(float2) * (size_t)total;
}

static int pattern_loss_multi_fwd_f32(int n_levels, const ctd_pattern_level* levels, float* terms, int type, float eps,
                                      void* ws, size_t ws_bytes, hipStream_t stream) {
  PatternLevelsDev t;
  unsigned total = 0;
  int st = build_levels(n_levels, levels, t, total);
  if (st) return st;
  for (int l = 0; l < n_levels; ++l)
    if (!levels[l].pattern_proj) return CTD_ERR_INVALID_ARG;
  if (!ws || ws_bytes < sizeof(float2) * (size_t)total) return CTD_ERR_WORKSPACE;
  float2* partials = (float2*)ws;
  int st_fwd = dispatch_type(type, [&](auto type_c) -> int {
    hipLaunchKernelGGL((pattern_loss_multi_fwd_kernel<decltype(type_c)::value, 9>), dim3(total), dim3(256), 0, stream, t,
                       partials, eps);
    CTD_LAUNCH_CHECK();
    return CTD_OK;
  });
  if (st_fwd) return st_fwd;
  hipLaunchKernelGGL(pattern_loss_multi_finish_kernel, dim3(n_levels), dim3(256), 0, stream, t, total, partials, terms);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int pattern_loss_multi_bwd_f32(int n_levels, const ctd_pattern_level* levels, const float* terms,
                                      const float* grad_vals, int type, float eps, hipStream_t stream) {
  PatternLevelsDev t;
  unsigned total = 0;
  int st = build_levels(n_levels, levels, t, total);
  if (st) return st;
  for (int l = 0; l < n_levels; ++l)
    if (!levels[l].grad_disp) return CTD_ERR_INVALID_ARG;
  return dispatch_type(type, [&](auto type_c) -> int {
    hipLaunchKernelGGL((pattern_loss_multi_bwd_kernel<decltype(type_c)::value, 9>), dim3(total), dim3(256), 0, stream, t,
                       terms, grad_vals, eps);
    CTD_LAUNCH_CHECK();
    return CTD_OK;
  });
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_pattern_loss_workspace_bytes(int B, int H, int W) {
  return img_shape_ok(B, H, W) ? pattern_loss_workspace_bytes(B, H, W) : 0;
}

int ctd_pattern_loss_fwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                             float* pattern_proj, float* terms, int B, int H, int W, int type, float eps,
                             void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  if (!disp || !im || !pattern || !pattern_proj || !terms) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_fwd_f32(disp, im, mask, pattern, pattern_proj, terms, B, H, W, type, eps, workspace, workspace_bytes,
                              (hipStream_t)stream);
}

int ctd_pattern_loss_bwd_f32(const float* disp, const float* im, const float* mask, const float* pattern,
                             const float* terms, const float* grad_val, const float* grad_proj, float* grad_disp,
                             int B, int H, int W, int type, float eps, int device, void* stream) {
  if (!img_shape_ok(B, H, W) || H < 2 || W < 2 || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  if (!disp || !im || !pattern || !terms || !grad_val || !grad_disp) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_bwd_f32(disp, im, mask, pattern, terms, grad_val, grad_proj, grad_disp, B, H, W, type, eps,
                              (hipStream_t)stream);
}

size_t ctd_pattern_loss_multi_workspace_bytes(int n_levels, const ctd_pattern_level* levels) {
  return pattern_loss_multi_workspace_bytes(n_levels, levels);
}

int ctd_pattern_loss_multi_fwd_f32(int n_levels, const ctd_pattern_level* levels, float* terms, int type, float eps,
                                   void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!terms || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_multi_fwd_f32(n_levels, levels, terms, type, eps, workspace, workspace_bytes, (hipStream_t)stream);
}

int ctd_pattern_loss_multi_bwd_f32(int n_levels, const ctd_pattern_level* levels, const float* terms,
                                   const float* grad_vals, int type, float eps, int device, void* stream) {
  if (!terms || !grad_vals || type < 0 || type > 3) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return pattern_loss_multi_bwd_f32(n_levels, levels, terms, grad_vals, type, eps, (hipStream_t)stream);
}

}  // extern "C"
