// ctd_costvol_ref.h -- reference-order block cost of one (pixel, disparity) of the SAD / census cost volume, shared by
// costvol_kernel (photometric.hip, the whole volume) and the exact re-scoring pass of the argmin (costvol_argmin.hip),
// so that both produce the same bits.
#pragma once
#include "ctd_common.h"

namespace ctd {

__device__ inline float t_sqrt(float x) { return sqrtf(x); }
__device__ inline double t_sqrt(double x) { return sqrt(x); }

// h(x) = 0.5 * (1 + x / sqrt(x^2 + eps)); inner part in T, the 0.5 multiply in double (ext.h:249)
template <typename T>
__device__ inline T soft_step(T x, T eps) {
  return (T)(0.5 * (double)((T)1 + x / t_sqrt(x * x + eps)));
}

// cost[d] of output (h, w) = photometric_loss_forward(es = P_d, ta = I) at (h, w), P_d[h][x] = P[h][clamp(x - d)]:
// taps in the reference order (row outer, column inner; clamp of the tap column first, shift second; each term divided
// by bs^2 before it is accumulated).  t = image plane, e = pattern plane, both [H][W].
template <int TYPE>
__device__ inline float costvol_ref_cost(const float* __restrict__ t, const float* __restrict__ e, int h, int w, int d,
                                         int H, int W, int bs, float eps) {
  const int half = bs / 2;
  const float bs2 = (float)(bs * bs);
  const float ec = e[(long)h * W + clampi(w - d, 0, W - 1)];
  const float tc = t[(long)h * W + w];
  float loss = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const int h0 = clampi(h + bh - half, 0, H - 1);
    for (int bw = 0; bw < bs; ++bw) {
      const int w0 = clampi(w + bw - half, 0, W - 1);
      const float ev = e[(long)h0 * W + clampi(w0 - d, 0, W - 1)];
      const float tv = t[(long)h0 * W + w0];
      if (TYPE == 0 || TYPE == 1) {
        const float diff = ev - tv;
        if (TYPE == 0) loss += diff * diff / bs2;
        else loss += fabsf(diff) / bs2;
      } else {
        const float diff = soft_step(ev - ec, eps) - soft_step(tv - tc, eps);
        if (TYPE == 2) loss += diff * diff / bs2;
        else loss += fabsf(diff) / bs2;
      }
    }
  }
  return loss;
}

}  // namespace ctd
