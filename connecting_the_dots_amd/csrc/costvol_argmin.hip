// costvol_argmin.hip -- argmin over the disparities of the SAD / soft-census cost volume without the volume
// (ctd_costvol_argmin_f32), with the indices of the reference-order volume (ctd_costvol_f32) bit for bit.
//
//   1. ranking pass: the tolerance-level volume kernel in its ranking instantiation (costvol_fast.hip) writes one
//      Top2 triple (b1, i1, b2) per (pixel, 128 disparities) into the workspace instead of the costs;
//   2. combine pass: one thread per pixel merges its chunk triples into idx / best and puts the pixel on the work list
//      unless the fast bound proves the fast winner is the exact one (margin below);
//   3. re-scoring pass: one wavefront per listed pixel evaluates all D costs in the reference order
//      (costvol_ref_cost, the tap loop of costvol_kernel) and takes the first-index argmin.
//
// Why the margin is enough.  The fast costs f(d) and the reference-order costs x(d) >= 0 obey
//     |f(d) - x(d)| <= r x(d) + a,      r = 1e-5, a = 1e-6   (ctd_costvol_fast_f32's stated bound)
// so  x(i1) <= (b1 + a) / (1 - r)  and, for every d != i1,  x(d) >= (f(d) - a) / (1 + r) >= (b2 - a) / (1 + r)  (b2 is
// the least fast cost over d != i1).  Hence
//     (b1 + a)(1 + r) < (b2 - a)(1 - r)   <=>   b2 - b1 > r (b1 + b2) + 2 a
// implies x(i1) < x(d) for every d != i1: i1 is the reference volume's unique minimum, its first-index argmin.  The
// test runs in f64 (b1, b2 and b2 - b1 exact there) with the right side raised by 2^-40 of itself for the rounding of
// the products.  Exact ties (b2 == b1) always fail it, so they are settled in the reference order, first index first.
#include "ctd_costvol_ref.h"
#include "ctd_internal.h"
#include "ctd_top2.h"
#include "ctd_validate.h"

namespace ctd {

constexpr double kArgminAbs = 1e-6;          // the bound's absolute term (fixed; the relative one is rerank_rel)

struct ArgminLayout {
  size_t counter, list, b1, i1, b2, bytes;
};

static ArgminLayout argmin_layout(int frames, int H, int W, int D) {
  const size_t P = (size_t)frames * H * W;
  const size_t T = P * (size_t)ceil_div(D, kRankChunk);
  ArgminLayout l;
  l.counter = 0;
  l.list = 256;
  l.b1 = align_up(l.list + 4 * P, 256);
  l.i1 = align_up(l.b1 + 4 * T, 256);
  l.b2 = align_up(l.i1 + 4 * T, 256);
  l.bytes = align_up(l.b2 + 4 * T, 256);
  return l;
}

static size_t costvol_argmin_workspace_bytes(int frames, int H, int W, int D) {
  if (frames <= 0) return 0;
  return argmin_layout(frames, H, W, D).bytes;
}

__global__ __launch_bounds__(256) void costvol_argmin_combine_kernel(Top2Planes top, int64_t* __restrict__ idx,
                                                                     float* __restrict__ best, long P, long HW,
                                                                     int n_chunks, float rerank_rel,
                                                                     unsigned* __restrict__ counter,
                                                                     unsigned* __restrict__ list) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const long f = p / HW, px = p - f * HW;
  const long base = f * n_chunks * HW + px;
  Top2 m{top.b1[base], top.i1[base], top.b2[base]};
  for (int c = 1; c < n_chunks; ++c) {               // chunk c holds greater indices than every earlier one
    const long i = base + (long)c * HW;
    m = top2_merge(m, Top2{top.b1[i], top.i1[i], top.b2[i]});
  }
  idx[p] = m.i1;
  if (best) best[p] = m.b1;
  if (rerank_rel < 0.f) return;                      // plain argmin of the fast costs
  bool sure = m.b2 == __builtin_inff();              // a single disparity: nothing to compare with
  if (!sure) {
    const double b1 = m.b1, b2 = m.b2, r = rerank_rel;
    const double margin = r * (b1 + b2) + 2.0 * kArgminAbs;
    sure = b2 - b1 > margin * (1.0 + 0x1p-40);
  }
  if (!sure) list[atomicAdd(counter, 1u)] = (unsigned)p;
}

// one wavefront per listed pixel: lane l evaluates d = l, l + 64, ... in the reference order, then a (cost, d)
// lexicographic minimum across the lanes -- the first-index argmin of the reference-order costs
template <int TYPE>
__global__ __launch_bounds__(256) void costvol_argmin_rescore_kernel(const float* __restrict__ im,
                                                                     const float* __restrict__ pat,
                                                                     long pat_frame_stride, int64_t* __restrict__ idx,
                                                                     float* __restrict__ best, int H, int W, int D,
                                                                     int bs, float eps,
                                                                     const unsigned* __restrict__ counter,
                                                                     const unsigned* __restrict__ list) {
  const unsigned n = *counter;                       // read on the device: the grid is sized without a host sync
  const int lane = threadIdx.x & 63;
  const long HW = (long)H * W;
  for (unsigned k = blockIdx.x * 4 + (threadIdx.x >> 6); k < n; k += gridDim.x * 4) {
    const unsigned p = list[k];
    const long f = p / HW, px = p - f * HW;
    const int h = (int)(px / W), w = (int)(px - (long)h * W);
    const float* t = im + f * HW;
    const float* e = pat + f * pat_frame_stride;
    float v = __builtin_inff();
    int di = INT_MAX;
    for (int d = lane; d < D; d += 64) {             // ascending d per lane: strict < keeps the first
      const float c = costvol_ref_cost<TYPE>(t, e, h, w, d, H, W, bs, eps);
      if (c < v) {
        v = c;
        di = d;
      }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const float ov = __shfl_xor(v, s);
      const int od = __shfl_xor(di, s);
      if (ov < v || (ov == v && od < di)) {
        v = ov;
        di = od;
      }
    }
    if (lane == 0) {
      idx[p] = di;
      if (best) best[p] = v;
    }
  }
}

static int costvol_argmin_f32(const float* im, const float* pat, long pat_frame_stride, int64_t* idx, float* best,
                              int frames, int H, int W, int D, int bs, int type, float eps, float rerank_rel,
                              void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const ArgminLayout l = argmin_layout(frames, H, W, D);
  if (!workspace || workspace_bytes < l.bytes || ((uintptr_t)workspace & 255)) return CTD_ERR_WORKSPACE;
  char* ws = (char*)workspace;
  unsigned* counter = (unsigned*)(ws + l.counter);
  unsigned* list = (unsigned*)(ws + l.list);
  const Top2Planes top{(float*)(ws + l.b1), (int*)(ws + l.i1), (float*)(ws + l.b2)};
  const bool rescore = rerank_rel >= 0.f;
  CTD_HIP_TRY(hipMemsetAsync(counter, 0, sizeof(unsigned), stream));
  int st = costvol_rank_f32(im, pat, pat_frame_stride, top, frames, H, W, D, bs, type, eps, stream);
  if (st) return st;
  const long P = (long)frames * H * W;
  hipLaunchKernelGGL(costvol_argmin_combine_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, top, idx,
                     best, P, (long)H * W, ceil_div(D, kRankChunk), rerank_rel, counter, list);
  CTD_LAUNCH_CHECK();
  if (!rescore) return CTD_OK;
  const long wgs_needed = (P + 3) / 4;                 // four wavefronts per workgroup, a pixel each
  const unsigned grid = (unsigned)(wgs_needed < 4L * device_cu_count() ? wgs_needed : 4L * device_cu_count());
  switch (type) {
    case 0: hipLaunchKernelGGL(costvol_argmin_rescore_kernel<0>, dim3(grid), dim3(256), 0, stream, im, pat, pat_frame_stride, idx, best, H, W, D, bs, eps, counter, list); break;
    case 1: hipLaunchKernelGGL(costvol_argmin_rescore_kernel<1>, dim3(grid), dim3(256), 0, stream, im, pat, pat_frame_stride, idx, best, H, W, D, bs, eps, counter, list); break;
    case 2: hipLaunchKernelGGL(costvol_argmin_rescore_kernel<2>, dim3(grid), dim3(256), 0, stream, im, pat, pat_frame_stride, idx, best, H, W, D, bs, eps, counter, list); break;
    default: hipLaunchKernelGGL(costvol_argmin_rescore_kernel<3>, dim3(grid), dim3(256), 0, stream, im, pat, pat_frame_stride, idx, best, H, W, D, bs, eps, counter, list); break;
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_costvol_argmin_workspace_bytes(int frames, int H, int W, int D, int block_size, int type,
                                          int per_frame_pattern) {
  (void)per_frame_pattern;                                                  // (the layout does not depend on it)
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || (block_size & 1) == 0) return 0;
  if (!costvol_rank_supported(frames, H, W, D, block_size)) return 0;
  return costvol_argmin_workspace_bytes(frames, H, W, D);
}

int ctd_costvol_argmin_f32(const float* im, const float* pattern, long pattern_frame_stride, int64_t* idx, float* best,
                           int frames, int H, int W, int D, int block_size, int type, float eps, float rerank_rel,
                           void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || (block_size & 1) == 0 ||
      pattern_frame_stride < 0 || rerank_rel != rerank_rel)
    return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !idx) return CTD_ERR_INVALID_ARG;
  if (!costvol_rank_supported(frames, H, W, D, block_size)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_argmin_f32(im, pattern, pattern_frame_stride, idx, best, frames, H, W, D, block_size, type, eps,
                            rerank_rel, workspace, workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
