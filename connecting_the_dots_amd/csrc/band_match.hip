// band_match.hip -- band-limited matching (ctd_xcorrvol_argmax_band_f32, ctd_costvol_argmin_band_f32): the first index
// of the best reference-order score of every pixel over its own disparity range [lo, hi], without a volume (the
// definition, word for word: include/ctd_hip_band.h).
//
// It generalises subpixel.hip's "three scores around idx" to "every score of [lo, hi], ranked".  The scorers -- 64 x 4
// pixel tiles staged in LDS, register groups of 8 / 4 candidates, every score in the reference's tap order -- live in
// ctd_band_score.h, which band_validity.hip shares; the kernels here hand them the sink BandBest: a running (best, first
// index) in ascending d with a strict compare.  No atomics, nothing shared between workgroups: the same bits on every
// run.
#include "../../include/ctd_hip_band.h"
#include "ctd_band_score.h"

namespace ctd {

// block sizes 3/5/7/9: the 64 x 4 tile of workgroup blockIdx.x = (f * tiles_y + ty) * tiles_x + tx
template <int BS>
__global__ __launch_bounds__(256) void xcorrvol_band_kernel(const float* __restrict__ in0,
                                                            const float* __restrict__ in1,
                                                            const float2* __restrict__ pstat, long in1_frame_stride,
                                                            const int32_t* __restrict__ lo,
                                                            const int32_t* __restrict__ hi, int64_t* __restrict__ idx,
                                                            float* __restrict__ best, int H, int W, int D, int tiles_x,
                                                            int tiles_y) {
  BandBest<true> sk;
  long p;
  const bool inside = xcorrvol_band_tile<BS>(in0, in1, pstat, in1_frame_stride, lo, hi, H, W, D, tiles_x, tiles_y, sk, p);
  if (inside) band_store(idx, best, p, sk.bi, sk.best);
}

// any other odd block size: thread per pixel, every tap from global memory
__global__ __launch_bounds__(256) void xcorrvol_band_rt_kernel(const float* __restrict__ in0,
                                                               const float* __restrict__ in1,
                                                               const float2* __restrict__ pstat, long in1_frame_stride,
                                                               const int32_t* __restrict__ lo,
                                                               const int32_t* __restrict__ hi,
                                                               int64_t* __restrict__ idx, float* __restrict__ best,
                                                               int frames, int H, int W, int D, int bs) {
  BandBest<true> sk;
  long p;
  const bool inside = xcorrvol_band_rt_pixel(in0, in1, pstat, in1_frame_stride, lo, hi, frames, H, W, D, bs, sk, p);
  if (inside) band_store(idx, best, p, sk.bi, sk.best);
}

static int xcorrvol_argmax_band_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                    const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D,
                                    int bs, bool prepared, void* workspace, hipStream_t stream) {
  const bool per_frame = in1_frame_stride != 0;
  const SubpixelLayout l = subpixel_layout(frames, H, W, D, per_frame);
  char* ws = (char*)workspace;
  float2* pstat = (float2*)(ws + l.pstat);
  if (!prepared) {
    const int st = subpixel_fill_pattern_planes(in1, (float*)(ws + l.q1), pstat, per_frame ? frames : 1, H, W, D, bs,
                                                stream);
    if (st != CTD_OK) return st;
  }
  const int tiles_x = ceil_div(W, kBandTW), tiles_y = ceil_div(H, kBandTH);
  const dim3 g((unsigned)((long)frames * tiles_y * tiles_x));   // <= frames * H * W < 2^31
  switch (bs) {
    case 3: hipLaunchKernelGGL(xcorrvol_band_kernel<3>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, idx, best, H, W, D, tiles_x, tiles_y); break;
    case 5: hipLaunchKernelGGL(xcorrvol_band_kernel<5>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, idx, best, H, W, D, tiles_x, tiles_y); break;
    case 7: hipLaunchKernelGGL(xcorrvol_band_kernel<7>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, idx, best, H, W, D, tiles_x, tiles_y); break;
    case 9: hipLaunchKernelGGL(xcorrvol_band_kernel<9>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, idx, best, H, W, D, tiles_x, tiles_y); break;
    default: {
      const long n = (long)frames * H * W;
      hipLaunchKernelGGL(xcorrvol_band_rt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in0, in1,
                         pstat, in1_frame_stride, lo, hi, idx, best, frames, H, W, D, bs);
    }
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// BS 3/5/7/9: 64 x 4 tiles as xcorrvol_band_kernel; BS 0: thread per pixel, block size bs_rt
template <int TYPE, int BS>
__global__ __launch_bounds__(256) void costvol_band_kernel(const float* __restrict__ im, const float* __restrict__ pat,
                                                           long pat_frame_stride, const int32_t* __restrict__ lo,
                                                           const int32_t* __restrict__ hi, int64_t* __restrict__ idx,
                                                           float* __restrict__ best, int frames, int H, int W, int D,
                                                           int bs_rt, float eps, int tiles_x, int tiles_y) {
  BandBest<false> sk;
  long p;
  const bool inside = costvol_band_pixel<TYPE, BS>(im, pat, pat_frame_stride, lo, hi, frames, H, W, D, bs_rt, eps, tiles_x,
                                              tiles_y, sk, p);
  if (inside) band_store(idx, best, p, sk.bi, sk.best);
}

template <int TYPE>
static void costvol_band_launch(const float* im, const float* pat, long pat_frame_stride, const int32_t* lo,
                                const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D, int bs,
                                float eps, hipStream_t stream) {
  const int tiles_x = ceil_div(W, kBandTW), tiles_y = ceil_div(H, kBandTH);
  const dim3 g((unsigned)((long)frames * tiles_y * tiles_x));   // <= frames * H * W < 2^31
  switch (bs) {
    case 3: hipLaunchKernelGGL((costvol_band_kernel<TYPE, 3>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    case 5: hipLaunchKernelGGL((costvol_band_kernel<TYPE, 5>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    case 7: hipLaunchKernelGGL((costvol_band_kernel<TYPE, 7>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    case 9: hipLaunchKernelGGL((costvol_band_kernel<TYPE, 9>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    default: {
      const long n = (long)frames * H * W;
      hipLaunchKernelGGL((costvol_band_kernel<TYPE, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, im,
                         pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, tiles_x, tiles_y);
    }
  }
}

static int costvol_argmin_band_f32(const float* im, const float* pat, long pat_frame_stride, const int32_t* lo,
                                   const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D,
                                   int bs, int type, float eps, hipStream_t stream) {
  switch (type) {
    case 0: costvol_band_launch<0>(im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, stream); break;
    case 1: costvol_band_launch<1>(im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, stream); break;
    case 2: costvol_band_launch<2>(im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, stream); break;
    default: costvol_band_launch<3>(im, pat, pat_frame_stride, lo, hi, idx, best, frames, H, W, D, bs, eps, stream); break;
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_xcorrvol_argmax_band_workspace_bytes(int frames, int H, int W, int D, int block_size,
                                                int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0) return 0;
  return xcorrvol_subpixel_workspace_bytes(frames, H, W, D, per_frame_pattern != 0);
}

int ctd_xcorrvol_argmax_band_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                 const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D,
                                 int block_size, int flags, void* workspace, size_t workspace_bytes, int device,
                                 void* stream) {
  if (!band_shape_ok(frames, H, W, D, block_size, in1_frame_stride) || (flags & ~CTD_PATTERN_PREPARED) != 0)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !lo || !hi || !idx) return CTD_ERR_INVALID_ARG;
  if ((double)frames * H * W >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < xcorrvol_subpixel_workspace_bytes(frames, H, W, D, in1_frame_stride != 0))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return xcorrvol_argmax_band_f32(in0, in1, in1_frame_stride, lo, hi, idx, best, frames, H, W, D, block_size,
                                  (flags & CTD_PATTERN_PREPARED) != 0, workspace, (hipStream_t)stream);
}

int ctd_costvol_argmin_band_f32(const float* im, const float* pattern, long pattern_frame_stride, const int32_t* lo,
                                const int32_t* hi, int64_t* idx, float* best, int frames, int H, int W, int D,
                                int block_size, int type, float eps, int device, void* stream) {
  if (!band_shape_ok(frames, H, W, D, block_size, pattern_frame_stride) || type < 0 || type > 3)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !lo || !hi || !idx) return CTD_ERR_INVALID_ARG;
  if ((double)frames * H * W >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_argmin_band_f32(im, pattern, pattern_frame_stride, lo, hi, idx, best, frames, H, W, D, block_size, type,
                                 eps, (hipStream_t)stream);
}

}  // extern "C"
