// synth.hip -- training-sample finishing of the synthetic data path: the per-pixel half of
// data/create_syn_data.py:163-188 (blend of the rendered pattern with the ambient image, disparity and mask, the
// ambient image's Sobel magnitude and its data-generation LCN as the edge target) and data/commons.py:46-107
// `augment_image` with max_shift = 0 (5x5 Gaussian blur, per-pixel noise, salt and pepper, clip to [0, 1]).
//
// The operation orders these kernels keep, and what they assume of OpenCV, are stated with the entry points in
// include/ctd_hip.h (ctd_syn_finish_f32, ctd_augment_f32, ctd_salt_pepper_f32).  Nothing here uses an FMA: the
// library builds with -ffp-contract=off.
#include "ctd_common.h"
#include "ctd_lcn_window.h"

namespace ctd {

// cv::borderInterpolate(i, n, BORDER_REFLECT_101) for any i (a 1-pixel axis maps everything to 0)
__device__ inline int reflect101(int i, int n) {
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  i %= p;
  if (i < 0) i += p;
  return i < n ? i : p - i;
}

// ---------------------------------------------------------------------------------------------------------
// Render finishing + edge target, one fused kernel.  A workgroup owns a 64 x 8 output tile.  It stages the ambient
// image (channel mean of `normal`) with a halo of ks + 2 in LDS, runs the Sobel row pass and column pass from there
// into a second tile of `pre = max(|Sobel| - thr, 0)` with a halo of ks, then the datagen LCN windows
// (ctd_lcn_window.h, the bits of lcn_datagen_kernel) read `pre` from LDS.  Halo positions outside the image hold
// reflected values that only border pixels (whose LCN output is zero) could reach.
// ---------------------------------------------------------------------------------------------------------
constexpr int kFinTW = 64, kFinTH = 8;

__global__ __launch_bounds__(256) void syn_finish_kernel(const float* __restrict__ depth, const float* __restrict__ color,
                                                         const float* __restrict__ normal, const double* __restrict__ blend,
                                                         float bf, float thr, int ks, float eps, int clip,
                                                         float* __restrict__ im, float* __restrict__ amb_out,
                                                         float* __restrict__ grad, float* __restrict__ disp,
                                                         float* __restrict__ mask, int H, int W) {
  extern __shared__ float lds_f[];
  const int R = ks + 2;
  const int TCa = kFinTW + 2 * R, TRa = kFinTH + 2 * R;     // ambient tile
  const int TCp = kFinTW + 2 * ks, TRp = kFinTH + 2 * ks;   // pre tile
  float* amb = lds_f;                                       // [TRa][TCa]
  float* hd = amb + TRa * TCa;                              // [TRa][TCp] row pass, derivative taps
  float* hs = hd + TRa * TCp;                               // [TRa][TCp] row pass, smoothing taps
  float* pre = hs + TRa * TCp;                              // [TRp][TCp]
  const float kD[5] = {-1.f, -2.f, 0.f, 2.f, 1.f};          // cv::getDerivKernels(dx = 1, ksize = 5)
  const float kS[5] = {1.f, 4.f, 6.f, 4.f, 1.f};            // cv::getDerivKernels(dx = 0, ksize = 5)
  const int x0 = blockIdx.x * kFinTW, y0 = blockIdx.y * kFinTH;
  const long base = (long)blockIdx.z * H * W;

  for (int i = threadIdx.x; i < TRa * TCa; i += 256) {
    const int r = i / TCa, c = i - r * TCa;
    const float* nv = normal + 3 * (base + (long)reflect101(y0 - R + r, H) * W + reflect101(x0 - R + c, W));
    amb[i] = ((nv[0] + nv[1]) + nv[2]) / 3.0f;              // np.mean(axis=2) on f32
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TRa * TCp; i += 256) {
    const int r = i / TCp, c = i - r * TCp;
    const float* a = amb + r * TCa + c;
    float sd = 0.f, ss = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      sd += kD[j] * a[j];
      ss += kS[j] * a[j];
    }
    hd[i] = sd;
    hs[i] = ss;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TRp * TCp; i += 256) {
    const int r = i / TCp, c = i - r * TCp;
    float gx = 0.f, gy = 0.f;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      gx += kS[j] * hd[(r + j) * TCp + c];
      gy += kD[j] * hs[(r + j) * TCp + c];
    }
    const float g = sqrtf(gx * gx + gy * gy);
    pre[i] = fmaxf(g - thr, 0.f);
  }
  __syncthreads();

  const float num = (float)((2 * ks + 1) * (2 * ks + 1));
  const double b = blend[blockIdx.z];
  const float wb = (float)b, wa = (float)(1.0 - b);        // f64 scalar * f32 array -> f32 (numpy 1.x)
  const int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kFinTH / 4; ++k) {
    const int ty = ty0 + 4 * k, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) continue;
    const long o = base + (long)y * W + x;
    float gv = 0.f;
    if (y >= ks && y < H - ks && x >= ks && x < W - ks) {
      float sd;
      gv = lcn_datagen_window(pre + ty * TCp + tx, TCp, ks, num, eps, &sd);
      if (clip) gv = fminf(fmaxf(gv, 0.f), 1.f);
    }
    grad[o] = gv;
    const float a = amb[(ty + R) * TCa + tx + R];
    const float* cv = color + 3 * o;
    const float imc = ((cv[0] + cv[1]) + cv[2]) / 3.0f;
    im[o] = wb * imc + wa * a;
    amb_out[o] = a;
    const float d = depth[o];
    if (disp) disp[o] = bf / d;
    if (mask) mask[o] = d > 0.f ? 1.f : 0.f;
  }
}

static int syn_finish_f32(const float* depth, const float* color, const float* normal, const double* blend, double bf,
                          float thr, int ks, float eps, int clip, float* im, float* amb, float* grad, float* disp,
                          float* mask, int N, int H, int W, hipStream_t stream) {
  const int R = ks + 2;
  const size_t lds = sizeof(float) * ((size_t)(kFinTW + 2 * R) * (kFinTH + 2 * R) +
                                      2 * (size_t)(kFinTH + 2 * R) * (kFinTW + 2 * ks) +
                                      (size_t)(kFinTH + 2 * ks) * (kFinTW + 2 * ks));
  if (lds > 64 * 1024) return CTD_ERR_UNSUPPORTED;
  dim3 grid(ceil_div(W, kFinTW), ceil_div(H, kFinTH), N);
  hipLaunchKernelGGL(syn_finish_kernel, grid, dim3(256), lds, stream, depth, color, normal, blend, (float)bf, thr, ks, eps,
                     clip, im, amb, grad, disp, mask, H, W);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Augmentation: blur (per-image flag), noise, clip; min / max of the input image as ordered-int keys, one pair of
// atomics per workgroup.  A workgroup owns a 64 x 16 tile (a thread: 4 rows of one column).
// ---------------------------------------------------------------------------------------------------------
constexpr int kAugTW = 64, kAugTH = 16;

// monotone map f32 -> u32 (total order of the non-NaN floats; 0 is below every key of a number)
__device__ inline unsigned ord_key(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float ord_val(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void augment_kernel(const float* __restrict__ img, const void* __restrict__ noise,
                                                      int noise_f64, const ctd_augment_params* __restrict__ params,
                                                      float* __restrict__ out, unsigned* __restrict__ minmax, int H,
                                                      int W) {
  __shared__ float tile[kAugTH + 4][kAugTW + 4];
  __shared__ float hb[kAugTH + 4][kAugTW];
  __shared__ float red[2][4];
  const ctd_augment_params p = params[blockIdx.z];
  const int x0 = blockIdx.x * kAugTW, y0 = blockIdx.y * kAugTH;
  const long base = (long)blockIdx.z * H * W;
  const int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
  if (p.blur) {                                             // uniform across the workgroup
    for (int i = threadIdx.x; i < (kAugTH + 4) * (kAugTW + 4); i += 256) {
      const int r = i / (kAugTW + 4), c = i - r * (kAugTW + 4);
      (&tile[0][0])[i] = img[base + (long)reflect101(y0 - 2 + r, H) * W + reflect101(x0 - 2 + c, W)];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < (kAugTH + 4) * kAugTW; i += 256) {
      const int r = i / kAugTW, c = i - r * kAugTW;
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) s += p.taps[j] * tile[r][c + j];
      hb[r][c] = s;
    }
    __syncthreads();
  }
  float mn = INFINITY, mx = -INFINITY;
#pragma unroll
  for (int k = 0; k < kAugTH / 4; ++k) {
    const int ty = ty0 + 4 * k, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) continue;
    const long o = base + (long)y * W + x;
    float v;
    if (p.blur) {
      const float xin = tile[ty + 2][tx + 2];
      mn = fminf(mn, xin);
      mx = fmaxf(mx, xin);
      float s = 0.f;
#pragma unroll
      for (int j = 0; j < 5; ++j) s += p.taps[j] * hb[ty + j][tx];
      v = s;
    } else {
      v = img[o];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
    double d = (double)v;
    if (noise) d = d + (noise_f64 ? ((const double*)noise)[o] : (double)((const float*)noise)[o]) * p.noise_scale;
    d = d < 0.0 ? 0.0 : d;                                  // np.maximum / np.minimum in f64, then one rounding
    d = d > 1.0 ? 1.0 : d;
    out[o] = (float)d;
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, s));
    mx = fmaxf(mx, __shfl_xor(mx, s));
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = mn;
    red[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    mn = fminf(fminf(red[0][0], red[0][1]), fminf(red[0][2], red[0][3]));
    mx = fmaxf(fmaxf(red[1][0], red[1][1]), fmaxf(red[1][2], red[1][3]));
    atomicMax(minmax + 2 * blockIdx.z, ~ord_key(mn));     // word 0: complemented key of the minimum
    atomicMax(minmax + 2 * blockIdx.z + 1, ord_key(mx));  // word 1: key of the maximum
  }
}

static int augment_f32(const float* img, const void* noise, int noise_f64, const ctd_augment_params* params, float* out,
                       uint32_t* minmax, int N, int H, int W, hipStream_t stream) {
  CTD_HIP_TRY(hipMemsetAsync(minmax, 0, sizeof(uint32_t) * 2 * (size_t)N, stream));
  dim3 grid(ceil_div(W, kAugTW), ceil_div(H, kAugTH), N);
  hipLaunchKernelGGL(augment_kernel, grid, dim3(256), 0, stream, img, noise, noise_f64, params, out, minmax, H, W);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// ---------------------------------------------------------------------------------------------------------
// Salt and pepper (commons.py:96-101): one workgroup per image; salt, barrier, pepper (pepper wins a shared index).
// Indices outside [0, H*W) are skipped; counts are clamped to [0, kmax].
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void salt_pepper_kernel(float* __restrict__ img, const unsigned* __restrict__ minmax,
                                                          const int32_t* __restrict__ counts,
                                                          const int64_t* __restrict__ salt,
                                                          const int64_t* __restrict__ pepper, int kmax, long HW) {
  const int n = blockIdx.x;
  const int k = min(max(counts[n], 0), kmax);
  float* im = img + (long)n * HW;
  const float vmin = fminf(fmaxf(ord_val(~minmax[2 * n]), 0.f), 1.f);
  const float vmax = fminf(fmaxf(ord_val(minmax[2 * n + 1]), 0.f), 1.f);
  const int64_t* s = salt + (long)n * kmax;
  const int64_t* q = pepper + (long)n * kmax;
  for (int i = threadIdx.x; i < k; i += 256) {
    const int64_t j = s[i];
    if (j >= 0 && j < HW) im[j] = vmax;
  }
  __syncthreads();                                          // waits for the salt stores: pepper lands after them
  for (int i = threadIdx.x; i < k; i += 256) {
    const int64_t j = q[i];
    if (j >= 0 && j < HW) im[j] = vmin;
  }
}

static int salt_pepper_f32(float* img, const uint32_t* minmax, const int32_t* counts, const int64_t* salt,
                           const int64_t* pepper, int kmax, int N, int H, int W, hipStream_t stream) {
  if (kmax == 0) return CTD_OK;
  hipLaunchKernelGGL(salt_pepper_kernel, dim3(N), dim3(256), 0, stream, img, minmax, counts, salt, pepper, kmax,
                     (long)H * W);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

static bool syn_shape_ok(int N, int H, int W) {
  return N >= 0 && N <= 65535 && H > 0 && W > 0 && (double)H * W * 3 < 2147483648.0;
}

int ctd_syn_finish_f32(const float* depth, const float* color, const float* normal, const double* blend,
                       double baseline_focal, float grad_threshold, int lcn_radius, float lcn_eps, int lcn_clip,
                       float* im, float* ambient, float* grad, float* disp, float* mask, int N, int H, int W, int device,
                       void* stream) {
  if (!syn_shape_ok(N, H, W) || lcn_radius < 0) return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!depth || !color || !normal || !blend || !im || !ambient || !grad) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return syn_finish_f32(depth, color, normal, blend, baseline_focal, grad_threshold, lcn_radius, lcn_eps, lcn_clip, im,
                        ambient, grad, disp, mask, N, H, W, (hipStream_t)stream);
}

int ctd_augment_f32(const float* img, const void* noise, int noise_f64, const ctd_augment_params* params, float* out,
                    uint32_t* minmax, int N, int H, int W, int device, void* stream) {
  if (!syn_shape_ok(N, H, W) || (noise_f64 != 0 && noise_f64 != 1)) return CTD_ERR_INVALID_ARG;
  if (N == 0) return CTD_OK;
  if (!img || !params || !out || !minmax) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return augment_f32(img, noise, noise_f64, params, out, minmax, N, H, W, (hipStream_t)stream);
}

int ctd_salt_pepper_f32(float* img, const uint32_t* minmax, const int32_t* counts, const int64_t* salt,
                        const int64_t* pepper, int kmax, int N, int H, int W, int device, void* stream) {
  if (!syn_shape_ok(N, H, W) || kmax < 0) return CTD_ERR_INVALID_ARG;
  if (N == 0 || kmax == 0) return CTD_OK;
  if (!img || !minmax || !counts || !salt || !pepper) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return salt_pepper_f32(img, minmax, counts, salt, pepper, kmax, N, H, W, (hipStream_t)stream);
}

}  // extern "C"
