// ctd_scan.h -- the one-workgroup scan of the count / scan / scatter scheme that depth_fusion.hip and tsdf.hip share:
// workgroups that each own a run of consecutive items count what they emit, this kernel turns the counts into offsets
// and per-track totals, and the workgroups write their items at the offsets.  No atomics, no flag that another workgroup
// waits on: the same bits on every run.
#pragma once

#include "ctd_common.h"

namespace ctd {
namespace {

constexpr int kScan = 1024;                                   // threads of the scan workgroup

// offsets[i] = counts[0] + ... + counts[i-1] for i = 0 .. n (the scan may run in place); n_per_track from the offsets
__global__ __launch_bounds__(kScan) void fuse_scan_kernel(int* offsets, int n, int per_track, int64_t* __restrict__ n_per_track,
                                                          int B) {
  __shared__ int wave_sum[kScan / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;
  for (int base = 0; base < n; base += kScan) {
    const int i = base + tid;
    const int v = i < n ? offsets[i] : 0;
    int incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d);
      if (lane >= d) incl += up;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kScan / 64; ++w) {
      before += w < wave ? wave_sum[w] : 0;
      total += wave_sum[w];
    }
    if (i < n) offsets[i] = carry + before + incl - v;
    carry += total;
    __syncthreads();
  }
  if (tid == 0) offsets[n] = carry;
  __syncthreads();                                            // the offsets this workgroup wrote are read back below
  for (int b = tid; b < B; b += kScan)
    n_per_track[b] = (int64_t)(offsets[(long)(b + 1) * per_track] - offsets[(long)b * per_track]);
}

}  // namespace
}  // namespace ctd
