// ctd_lcn_window.h -- one output of data/lcn/lcn.pyx:36-53 (`lcn.normalize`) read from a tile in LDS.  Shared by
// lcn_datagen_kernel (lcn.hip) and the fused render-finishing kernel (synth.hip), so that both give the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace ctd {

// win: top-left tap of the (2ks+1)^2 window, rows `pitch` floats apart; num = (2ks+1)^2 as f32 (lcn.pyx:33).
// Two passes in f32 in the Cython loop's row-major tap order: the mean, then the sum of squared deviations (no FMA: the
// library builds with -ffp-contract=off).  Returns (x - mean) / (std + eps) and stores the raw std in *sd.
__device__ inline float lcn_datagen_window(const float* win, int pitch, int ks, float num, float eps, float* sd) {
  float mean = 0.f;
  for (int i = 0; i <= 2 * ks; ++i)
    for (int j = 0; j <= 2 * ks; ++j) mean += win[i * pitch + j];
  mean = mean / num;
  float acc = 0.f;
  for (int i = 0; i <= 2 * ks; ++i)
    for (int j = 0; j <= 2 * ks; ++j) {
      const float d = win[i * pitch + j] - mean;
      acc = acc + d * d;
    }
  const float s = sqrtf(acc / num);
  *sd = s;
  return (win[ks * pitch + ks] - mean) / (s + eps);
}

}  // namespace ctd
