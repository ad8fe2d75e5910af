// photometric_fast.hip -- tolerance-level (|a-b| <= 1e-5|b| + 1e-6) block photometric loss, f32: the functions of
// photometric.hip (PhotometricLossForward / PhotometricLossBackward, torchext/ext/ext.h:201-344) on the LDS tile of
// ctd_photo_tile.h, which also holds the per-pixel arithmetic and the derivation of the atomic-free backward.
#include "ctd_common.h"
#include "ctd_dispatch.h"
#include "ctd_photo_tile.h"
#include "ctd_validate.h"

namespace ctd {

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void photometric_fast_fwd_kernel(const float* __restrict__ es,
                                                                   const float* __restrict__ ta,
                                                                   float* __restrict__ out, int C, int H, int W,
                                                                   float eps) {
  constexpr int TW = kPTW + BS - 1, TH = kPTH + BS - 1;
  __shared__ float sE[TH][TW], sT[TH][TW];
  const int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
  const int x0 = blockIdx.x * kPTW, y0 = blockIdx.y * kPTH, n = blockIdx.z;
  const long HW = (long)H * W;
  float loss[2] = {0.f, 0.f};
  for (int c = 0; c < C; ++c) {
    __syncthreads();
    stage_tile<BS>(sE, es + ((long)n * C + c) * HW, H, W, x0, y0);
    stage_tile<BS>(sT, ta + ((long)n * C + c) * HW, H, W, x0, y0);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 2; ++k) loss[k] += fwd_pixel<TYPE, BS>(sE, sT, tx, ty0 + 4 * k, eps);
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const int x = x0 + tx, y = y0 + ty0 + 4 * k;
    if (x < W && y < H) out[(long)n * HW + (long)y * W + x] = loss[k];
  }
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void photometric_fast_bwd_kernel(const float* __restrict__ es,
                                                                   const float* __restrict__ ta,
                                                                   const float* __restrict__ grad_out,
                                                                   float* __restrict__ grad_in, int C, int H, int W,
                                                                   float eps) {
  constexpr int HALF = BS / 2, TW = kPTW + BS - 1, TH = kPTH + BS - 1;
  __shared__ float sE[TH][TW], sT[TH][TW], sG[TH][TW];
  const int x0 = blockIdx.x * kPTW, y0 = blockIdx.y * kPTH, n = blockIdx.z;
  const long HW = (long)H * W;
  // a tile whose pixels all lie at least 2*HALF from the image border only meets multiplicities of 1
  const bool interior = x0 >= 2 * HALF && y0 >= 2 * HALF && x0 + kPTW - 1 <= W - 1 - 2 * HALF &&
                        y0 + kPTH - 1 <= H - 1 - 2 * HALF;
  stage_tile<BS>(sG, grad_out + (long)n * HW, H, W, x0, y0);
  for (int c = 0; c < C; ++c) {
    __syncthreads();
    stage_tile<BS>(sE, es + ((long)n * C + c) * HW, H, W, x0, y0);
    stage_tile<BS>(sT, ta + ((long)n * C + c) * HW, H, W, x0, y0);
    __syncthreads();
    float* plane = grad_in + ((long)n * C + c) * HW;
    auto sink = [&](int qx, int qy, float g) { plane[(long)qy * W + qx] = g; };
    if (interior) bwd_tile<TYPE, BS, false>(sE, sT, sG, sink, H, W, x0, y0, eps);
    else bwd_tile<TYPE, BS, true>(sE, sT, sG, sink, H, W, x0, y0, eps);
  }
}

// forward (go == nullptr, dst = loss) or backward (dst = grad_es)
static int launch_fast(const float* es, const float* ta, const float* go, float* dst, int B, int C, int H, int W, int bs,
                       int type, float eps, hipStream_t stream) {
  const dim3 grid(ceil_div(W, kPTW), ceil_div(H, kPTH), B);
  return dispatch_block(bs, [&](auto bs_c) {
    return dispatch_type(type, [&](auto type_c) -> int {
      constexpr int BS = decltype(bs_c)::value, TYPE = decltype(type_c)::value;
      if (go)
        hipLaunchKernelGGL((photometric_fast_bwd_kernel<TYPE, BS>), grid, dim3(256), 0, stream, es, ta, go, dst, C, H, W, eps);
      else
        hipLaunchKernelGGL((photometric_fast_fwd_kernel<TYPE, BS>), grid, dim3(256), 0, stream, es, ta, dst, C, H, W, eps);
      CTD_LAUNCH_CHECK();
      return CTD_OK;
    });
  });
}

static int photometric_fwd_fast_f32(const float* es, const float* ta, float* out, int B, int C, int H, int W, int bs,
                                    int type, float eps, hipStream_t s) {
  return launch_fast(es, ta, nullptr, out, B, C, H, W, bs, type, eps, s);
}
static int photometric_bwd_fast_f32(const float* es, const float* ta, const float* go, float* gi, int B, int C, int H,
                                    int W, int bs, int type, float eps, hipStream_t s) {
  return launch_fast(es, ta, go, gi, B, C, H, W, bs, type, eps, s);
}

}  // namespace ctd

using namespace ctd;

extern "C" {

CTD_PHOTO_ENTRY(fast_f32, float)

}  // extern "C"
