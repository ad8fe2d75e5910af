// ctd_view.h -- the device helpers the kernels over posed views share (depth_fusion.hip, depth_warp.hip, depth_icp.hip,
// tsdf.hip): which pixels of a depth map are live, and the three steps between a pixel of one view, the world and a
// pixel of another view (X_cam = R X_world + t).  Every product and sum is in the association of include/ctd_hip.h
// (that of geo_forward in losses.hip), stated here and nowhere else; the build never contracts them, so every kernel
// that includes this header computes the same bits.
#pragma once

#include "ctd_common.h"

namespace ctd {

// live: valid nonzero (NULL: everywhere) and depth finite and > 0
__device__ inline bool live_at(const float* __restrict__ depth, const uint8_t* __restrict__ valid, long g) {
  const float d = depth[g];
  return (!valid || valid[g]) && d > 0.f && d < __builtin_inff();
}

// depth d along ray3 in the view (R, t) -> the world point X = (d ray3 - t) @ R
__device__ inline void camera_to_world(const float* ray3, float d, const float* R, const float* t, float* X) {
  float p[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) p[i] = d * ray3[i] - t[i];
#pragma unroll
  for (int j = 0; j < 3; ++j) X[j] = p[0] * R[0 * 3 + j] + p[1] * R[1 * 3 + j] + p[2] * R[2 * 3 + j];
}

// the world point X -> s = R X + t in the frame of the camera (R, t)
__device__ inline void world_to_camera(const float* X, const float* R, const float* t, float* s) {
#pragma unroll
  for (int j = 0; j < 3; ++j) s[j] = X[0] * R[j * 3 + 0] + X[1] * R[j * 3 + 1] + X[2] * R[j * 3 + 2] + t[j];
}

// the camera point s -> uvd = K s (the pixel is uvd[0] / uvd[2], uvd[1] / uvd[2])
__device__ inline void project(const float* s, const float* K, float* uvd) {
#pragma unroll
  for (int j = 0; j < 3; ++j) uvd[j] = s[0] * K[j * 3 + 0] + s[1] * K[j * 3 + 1] + s[2] * K[j * 3 + 2];
}

// depth d along ray3 in view a -> s, the point in the frame of camera b, and its uvd in view b
__device__ inline void view_transform_point(const float* __restrict__ ray3, float d, const float* __restrict__ Ra,
                                            const float* __restrict__ ta, const float* __restrict__ Rb,
                                            const float* __restrict__ tb, const float* __restrict__ K, float* s,
                                            float* uvd) {
  float X[3];
  camera_to_world(ray3, d, Ra, ta, X);
  world_to_camera(X, Rb, tb, s);
  project(s, K, uvd);
}

__device__ inline void view_transform(const float* __restrict__ ray3, float d, const float* __restrict__ Ra,
                                      const float* __restrict__ ta, const float* __restrict__ Rb,
                                      const float* __restrict__ tb, const float* __restrict__ K, float* uvd) {
  float s[3];
  view_transform_point(ray3, d, Ra, ta, Rb, tb, K, s, uvd);
}

}  // namespace ctd
