// ctd_compact.h -- the count / scan / scatter scheme of depth_fusion.hip, tsdf.hip, tsdf_mesh.hip and mesh_clean.hip,
// stated once: workgroups that each own a chunk of 256 consecutive items count what they emit, ONE workgroup turns the
// counts into offsets and per-track totals, and the workgroups write their items at the offsets.  No atomics, no flag
// that another workgroup waits on: the same bits on every run.
#pragma once

#include "ctd_common.h"

namespace ctd {
namespace {

constexpr int kChunk = 256;                                   // items, and threads, per workgroup of a count or scatter kernel
constexpr int kScan = 1024;                                   // threads of the scan workgroup

inline long chunks_of(long n) { return (n + kChunk - 1) / kChunk; }

// the item of a thread where every group (a view, a track) is cut into `chunks` chunks: item p of its group
// (p >= the group's size: past its end).  A chunk never crosses a group, so what is indexed by the group stays uniform.
struct ChunkItem {
  int group;
  long p;
};
__device__ inline ChunkItem chunk_item(int chunks) {
  return {(int)(blockIdx.x / chunks), (long)(blockIdx.x % chunks) * kChunk + threadIdx.x};
}

// The workgroup prefixes.  Every thread of the workgroup calls (there is a barrier inside); wave_n is one int per
// wavefront in LDS, free for reuse after the next barrier; total = the sum over the whole workgroup.

// the three crossing flags of a voxel (bits 0 .. 2 of f), in the order thread, then bit: the number of set bits of the
// threads before this one
template <int THREADS>
__device__ inline int wg_flags3_before(int f, int* wave_n, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long b0 = __ballot(f & 1), b1 = __ballot(f & 2), b2 = __ballot(f & 4);
  if (lane == 0) wave_n[wave] = __popcll(b0) + __popcll(b1) + __popcll(b2);
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  int before = __popcll(b0 & below) + __popcll(b1 & below) + __popcll(b2 & below);
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    before += w < wave ? wave_n[w] : 0;
    total += wave_n[w];
  }
  return before;
}

// one flag: the number of set flags of the threads before this one (the ballots of the two absent bits fold away)
template <int THREADS>
__device__ inline int wg_flags_before(bool flag, int* wave_n, int& total) {
  return wg_flags3_before<THREADS>(flag ? 1 : 0, wave_n, total);
}

// sum of v over the lanes of the wavefront up to and including this one
__device__ inline int wave_inclusive_sum(int v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(v, d);
    if (lane >= d) v += up;
  }
  return v;
}

// sum of v over the threads before this one (the loop over wave_n stands here a second time: as a helper of its own
// it cost mc_vert_scatter_kernel two VGPRs)
template <int THREADS>
__device__ inline int wg_exclusive_sum(int v, int* wave_n, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, incl = wave_inclusive_sum(v);
  if (lane == 63) wave_n[wave] = incl;
  __syncthreads();
  int before = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < THREADS / 64; ++w) {
    before += w < wave ? wave_n[w] : 0;
    total += wave_n[w];
  }
  return before + incl - v;
}

// ONE workgroup: offsets[i] = counts[0] + ... + counts[i-1] for i = 0 .. n, kScan at a time with a carry (the scan may
// run in place); then n_per_track, the B differences of the offsets `per_track` counts apart
__global__ __launch_bounds__(kScan) void fuse_scan_kernel(int* offsets, int n, int per_track, int64_t* __restrict__ n_per_track,
                                                          int B) {
  __shared__ int wave_n[kScan / 64];
  const int tid = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < n; base += kScan) {
    const int i = base + tid;
    int total;
    const int before = wg_exclusive_sum<kScan>(i < n ? offsets[i] : 0, wave_n, total);
    if (i < n) offsets[i] = carry + before;
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
