// ctd_view.h -- the device helpers every multi-view kernel shares (depth_fusion.hip, depth_warp.hip, depth_icp.hip, tsdf.hip): which pixels
// of a depth map are live, and the projection of a pixel of one posed view into another.  Every product and sum of
// view_transform is in the association of include/ctd_hip.h (that of geo_forward in losses.hip); the build never
// contracts them, so every kernel that includes this header computes the same bits.
#pragma once

#include "ctd_common.h"

namespace ctd {

// live: valid nonzero (NULL: everywhere) and depth finite and > 0
__device__ inline bool live_at(const float* __restrict__ depth, const uint8_t* __restrict__ valid, long g) {
  const float d = depth[g];
  return (!valid || valid[g]) && d > 0.f && d < __builtin_inff();
}

// depth d along ray3 in view a -> uvd in view b (X_cam = R X_world + t)
__device__ inline void view_transform(const float* __restrict__ ray3, float d, const float* __restrict__ Ra,
                                      const float* __restrict__ ta, const float* __restrict__ Rb,
                                      const float* __restrict__ tb, const float* __restrict__ K, float* uvd) {
  float p[3], q[3], s[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = d * ray3[i] - ta[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) q[j] = p[0] * Ra[0 * 3 + j] + p[1] * Ra[1 * 3 + j] + p[2] * Ra[2 * 3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) s[j] = q[0] * Rb[j * 3 + 0] + q[1] * Rb[j * 3 + 1] + q[2] * Rb[j * 3 + 2] + tb[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) uvd[j] = s[0] * K[j * 3 + 0] + s[1] * K[j * 3 + 1] + s[2] * K[j * 3 + 2];
}

// view_transform that also hands out s, the point in the frame of camera b (depth_icp.hip): the same products and sums
// in the same association, so uvd has the bits view_transform gives
__device__ inline void view_transform_point(const float* __restrict__ ray3, float d, const float* __restrict__ Ra,
                                            const float* __restrict__ ta, const float* __restrict__ Rb,
                                            const float* __restrict__ tb, const float* __restrict__ K, float* s,
                                            float* uvd) {
  float p[3], q[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = d * ray3[i] - ta[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) q[j] = p[0] * Ra[0 * 3 + j] + p[1] * Ra[1 * 3 + j] + p[2] * Ra[2 * 3 + j];
#pragma unroll
  for (int j = 0; j < 3; ++j) s[j] = q[0] * Rb[j * 3 + 0] + q[1] * Rb[j * 3 + 1] + q[2] * Rb[j * 3 + 2] + tb[j];
#pragma unroll
  for (int j = 0; j < 3; ++j) uvd[j] = s[0] * K[j * 3 + 0] + s[1] * K[j * 3 + 1] + s[2] * K[j * 3 + 2];
}

}  // namespace ctd
