// ctd_subpixel_ws.h -- the workspace of the reference-order NCC point scorers (subpixel.hip: three scores around an
// index; band_match.hip: every score of a per-pixel range): its layout and the two kernels that fill its pattern planes.
// One workspace serves both ops, so a workspace whose pattern planes one of them has filled (CTD_PATTERN_PREPARED) is
// prepared for the other too.
//
// The planes hold parts of the accumulator chains of XCorrVolFunctor (ext.h:120-191) that do not depend on the frame:
//   - the quotients x / bs^2 of every pattern sample (and, for the sub-pixel op, of every frame sample);
//   - the pattern half (mu1, then s1) per pattern row and UNCLAMPED window centre x = w - d (ext.h:152 shifts before it
//     clamps), x in [-(D-1), W-1].
#pragma once
#include "ctd_common.h"

namespace ctd {

struct SubpixelLayout {
  size_t q0, q1, pstat, bytes;
};

static SubpixelLayout subpixel_layout(int frames, int H, int W, int D, bool per_frame_pattern) {
  const size_t HW = (size_t)H * W;
  const size_t P = per_frame_pattern ? (size_t)frames : 1;
  SubpixelLayout l;
  l.q0 = 0;                                                     // f32 [frames][H][W]: in0 / bs^2
  l.q1 = align_up(l.q0 + 4 * (size_t)frames * HW, 256);         // f32 [P][H][W]: in1 / bs^2
  l.pstat = align_up(l.q1 + 4 * P * HW, 256);                   // float2 [P][H][W + D - 1]: (mu1, s1) at x = col - (D-1)
  l.bytes = align_up(l.pstat + 8 * P * (size_t)H * (W + D - 1), 256);
  return l;
}

static size_t xcorrvol_subpixel_workspace_bytes(int frames, int H, int W, int D, bool per_frame_pattern) {
  if (frames <= 0) return 0;
  return subpixel_layout(frames, H, W, D, per_frame_pattern).bytes;
}

static __global__ __launch_bounds__(256) void subpixel_quotient_kernel(const float* __restrict__ x,
                                                                       float* __restrict__ q, long n, float bs2) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) q[i] = x[i] / bs2;
}

// (mu1, s1) of the pattern window centred at (h, x), x = xo - (D-1), unclamped; the columns clamp tap by tap
template <int BS>
__global__ __launch_bounds__(256) void subpixel_pattern_stats_kernel(const float* __restrict__ in1,
                                                                     const float* __restrict__ q1,
                                                                     float2* __restrict__ pstat, int P, int H, int W,
                                                                     int D, int bs_rt) {
  const int bs = BS ? BS : bs_rt;
  const int half = bs / 2;
  const long Wo = (long)W + D - 1;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)P * H * Wo) return;
  const long ph = i / Wo;
  const int x = (int)(i - ph * Wo) - (D - 1);
  const int p = (int)(ph / H), h = (int)(ph - (long)p * H);
  const float* e = in1 + (long)p * H * W;
  const float* eq = q1 + (long)p * H * W;
  float mu = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
#pragma unroll
    for (int bw = 0; bw < bs; ++bw) mu += eq[r + clampi(x + bw - half, 0, W - 1)];
  }
  float s = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
#pragma unroll
    for (int bw = 0; bw < bs; ++bw) {
      const float v = e[r + clampi(x + bw - half, 0, W - 1)] - mu;
      s += v * v;
    }
  }
  pstat[i] = make_float2(mu, s);
}

// fills the pattern planes (q1, pstat) of a workspace laid out by subpixel_layout
static int subpixel_fill_pattern_planes(const float* in1, float* q1, float2* pstat, int P, int H, int W, int D, int bs,
                                        hipStream_t stream) {
  const float bs2 = (float)(bs * bs);
  const long n1 = (long)P * H * W;
  hipLaunchKernelGGL(subpixel_quotient_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, stream, in1, q1, n1,
                     bs2);
  CTD_LAUNCH_CHECK();
  const long ns = (long)P * H * ((long)W + D - 1);
  const dim3 g((unsigned)((ns + 255) / 256));
  switch (bs) {
    case 3: hipLaunchKernelGGL(subpixel_pattern_stats_kernel<3>, g, dim3(256), 0, stream, in1, q1, pstat, P, H, W, D, bs); break;
    case 5: hipLaunchKernelGGL(subpixel_pattern_stats_kernel<5>, g, dim3(256), 0, stream, in1, q1, pstat, P, H, W, D, bs); break;
    case 7: hipLaunchKernelGGL(subpixel_pattern_stats_kernel<7>, g, dim3(256), 0, stream, in1, q1, pstat, P, H, W, D, bs); break;
    case 9: hipLaunchKernelGGL(subpixel_pattern_stats_kernel<9>, g, dim3(256), 0, stream, in1, q1, pstat, P, H, W, D, bs); break;
    default: hipLaunchKernelGGL(subpixel_pattern_stats_kernel<0>, g, dim3(256), 0, stream, in1, q1, pstat, P, H, W, D, bs); break;
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd
