// band_match.hip -- band-limited matching (ctd_xcorrvol_argmax_band_f32, ctd_costvol_argmin_band_f32): the first index
// of the best reference-order score of every pixel over its own disparity range [lo, hi], without a volume (the
// definition, word for word: include/ctd_hip_band.h).
//
// It generalises subpixel.hip's "three scores around idx" to "every score of [lo, hi], ranked".  As there, every score
// keeps its own accumulator chains in the reference's tap order (-ffp-contract=off), so its bits are the volume's:
//   NCC    the frame half (mu0, then s0) once per pixel; the pattern half (mu1, s1) of a candidate from the table of
//          ctd_subpixel_ws.h; one `dot` chain per candidate;
//   costs  the tap loop of costvol_ref_cost (ctd_costvol_ref.h), the image-side soft step of the census types once per
//          tap and group.
//
// Shape.  A workgroup owns a 64 x 4 pixel tile (a wavefront: 64 pixels of one row) and stages the frame tile plus halo
// in LDS with the replicate border baked in -- neighbouring pixels share all but one column of their taps.  Candidates
// are taken in register groups of K = 8 (K = 4 once no lane of the wavefront has more than 4 left): one pass over the
// taps reads each frame tap once and bs + K - 1 pattern samples per row (clamped addresses, served by L1 / L2: the
// lanes of a row read overlapping spans) for K chains, because the taps of d, d+1, ... in a row are one span shifted
// by one.  Each lane starts at its own lo', the groups loop up to the wavefront's widest band, and lanes beyond their
// hi' keep computing on clamped addresses but are not ranked.  Ranking is a running (best, first index) in ascending d
// with a strict compare.  No atomics, nothing shared between workgroups: the same bits on every run.
//
// The cost volume clamps the tap column before it shifts (ctd_costvol_ref.h), so within `half` columns of the right
// border the taps of a row are no longer one shifted span; those lanes, and every block size without a template
// (3/5/7/9 have one), take the run-time group scorers, which address every tap on its own.
#include "../../include/ctd_hip_band.h"
#include "ctd_common.h"
#include "ctd_costvol_ref.h"
#include "ctd_ncc_point.h"
#include "ctd_subpixel_ws.h"
#include "ctd_validate.h"

namespace ctd {

constexpr int kBandTW = 64, kBandTH = 4;         // pixel tile of a workgroup (256 threads)

__device__ inline void band_take(float s, int d, int hi, bool maximum, float& best, int& bi) {
  if (d <= hi && (bi < 0 || (maximum ? s > best : s < best))) {
    best = s;
    bi = d;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// NCC
// ---------------------------------------------------------------------------------------------------------------------

// candidates d0 .. d0 + K - 1 of pixel (h, w); ps = the (mu1, s1) row of h at x = w (ps[-d]: the window centred w - d);
// tap(bh, bw) = the frame tap.  Pattern tap (bh, bw) of d0 + k is column clamp(w - half + bw - d0 - k): sample
// bw + K - 1 - k of the row span that starts at w - half - d0 - (K - 1).
template <int BS, int K, typename Tap>
__device__ inline void ncc_band_group(Tap tap, const float* __restrict__ e, const float2* __restrict__ ps, int h, int w,
                                      int H, int W, int D, int bs_rt, int d0, int hi, float mu0, float s0, float& best,
                                      int& bi) {
  const int bs = BS ? BS : bs_rt;
  const int half = bs / 2;
  float mu1[K], s1[K], dot[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float2 st = ps[-min(d0 + k, D - 1)];                  // (lanes past their band stay inside the table)
    mu1[k] = st.x;
    s1[k] = st.y;
    dot[k] = 0.f;
  }
  const int base = w - half - d0 - (K - 1);
  for (int bh = 0; bh < bs; ++bh) {
    const float* er = e + (long)clampi(h + bh - half, 0, H - 1) * W;
    if constexpr (BS > 0) {
      float pr[BS + K - 1];
#pragma unroll
      for (int j = 0; j < BS + K - 1; ++j) pr[j] = er[clampi(base + j, 0, W - 1)];
#pragma unroll
      for (int bw = 0; bw < BS; ++bw) {
        const float v0 = tap(bh, bw) - mu0;
#pragma unroll
        for (int k = 0; k < K; ++k) dot[k] += v0 * (pr[bw + K - 1 - k] - mu1[k]);
      }
    } else {
      for (int bw = 0; bw < bs; ++bw) {
        const float v0 = tap(bh, bw) - mu0;
#pragma unroll
        for (int k = 0; k < K; ++k) dot[k] += v0 * (er[clampi(base + bw + K - 1 - k, 0, W - 1)] - mu1[k]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float s = 0.f;                                              // val = 0; val += dot / norm  (ext.h:142, 186)
    s += dot[k] / ncc_norm(s0, s1[k]);
    band_take(s, d0 + k, hi, true, best, bi);
  }
}

// the frame half, then the groups; every lane of the wavefront must call this (the group width is wave-uniform)
template <int BS, typename Tap, typename TapQ>
__device__ inline void ncc_band_pixel(Tap tap, TapQ tapq, const float* __restrict__ e, const float2* __restrict__ ps,
                                      int h, int w, int H, int W, int D, int bs_rt, int lo, int hi, float& best,
                                      int& bi) {
  const int bs = BS ? BS : bs_rt;
  float mu0 = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
#pragma unroll
    for (int bw = 0; bw < bs; ++bw) mu0 += tapq(bh, bw);
  }
  float s0 = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
#pragma unroll
    for (int bw = 0; bw < bs; ++bw) {
      const float v0 = tap(bh, bw) - mu0;
      s0 += v0 * v0;
    }
  }
  int d0 = lo;
  while (true) {
    const int left = hi - d0 + 1;
    if (!__any(left > 0)) break;
    if (__any(left > 4)) {
      ncc_band_group<BS, 8>(tap, e, ps, h, w, H, W, D, bs_rt, d0, hi, mu0, s0, best, bi);
      d0 = min(d0 + 8, D);
    } else {
      ncc_band_group<BS, 4>(tap, e, ps, h, w, H, W, D, bs_rt, d0, hi, mu0, s0, best, bi);
      d0 = min(d0 + 4, D);
    }
  }
}

__device__ inline void band_store(int64_t* __restrict__ idx, float* __restrict__ best, long p, int bi, float bv) {
  idx[p] = bi;
  if (best) best[p] = bi < 0 ? __builtin_nanf("") : bv;
}

// block sizes 3/5/7/9: the 64 x 4 tile of workgroup blockIdx.x = (f * tiles_y + ty) * tiles_x + tx
template <int BS>
__global__ __launch_bounds__(256) void xcorrvol_band_kernel(const float* __restrict__ in0,
                                                            const float* __restrict__ in1,
                                                            const float2* __restrict__ pstat, long in1_frame_stride,
                                                            const int32_t* __restrict__ lo,
                                                            const int32_t* __restrict__ hi, int64_t* __restrict__ idx,
                                                            float* __restrict__ best, int H, int W, int D, int tiles_x,
                                                            int tiles_y) {
  constexpr int SW = kBandTW + BS - 1, SH = kBandTH + BS - 1, half = BS / 2;
  __shared__ float sA[SH * SW], sAq[SH * SW];                   // the frame tile + halo and its quotients x / bs^2
  const long HW = (long)H * W;
  const int tx = blockIdx.x % tiles_x;
  const int ty = (blockIdx.x / tiles_x) % tiles_y;
  const long f = blockIdx.x / tiles_x / tiles_y;
  const int h0 = ty * kBandTH, w0 = tx * kBandTW;
  const float* a = in0 + f * HW;
  const float bs2 = (float)(BS * BS);
  for (int i = threadIdx.x; i < SH * SW; i += 256) {
    const int y = i / SW, x = i - y * SW;
    const float v = a[(long)clampi(h0 + y - half, 0, H - 1) * W + clampi(w0 + x - half, 0, W - 1)];
    sA[i] = v;
    sAq[i] = v / bs2;
  }
  __syncthreads();
  const int lx = threadIdx.x & (kBandTW - 1), ly = threadIdx.x / kBandTW;
  const bool inside = h0 + ly < H && w0 + lx < W;
  const int h = min(h0 + ly, H - 1), w = min(w0 + lx, W - 1);   // (lanes outside the image: an empty band, valid reads)
  const long p = f * HW + (long)h * W + w;
  const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
  const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
  const float* e = in1 + (in1_frame_stride ? f * HW : 0);
  const long Wo = (long)W + D - 1;
  const float2* ps = pstat + (in1_frame_stride ? f * (long)H * Wo : 0) + (long)h * Wo + (w + D - 1);
  const float* tA = sA + ly * SW + lx;
  const float* tQ = sAq + ly * SW + lx;
  float bv = 0.f;
  int bi = -1;
  ncc_band_pixel<BS>([=](int bh, int bw) { return tA[bh * SW + bw]; }, [=](int bh, int bw) { return tQ[bh * SW + bw]; },
                     e, ps, h, w, H, W, D, BS, l, u, bv, bi);
  if (inside) band_store(idx, best, p, bi, bv);
}

// any other odd block size: thread per pixel, every tap from global memory
__global__ __launch_bounds__(256) void xcorrvol_band_rt_kernel(const float* __restrict__ in0,
                                                               const float* __restrict__ in1,
                                                               const float2* __restrict__ pstat, long in1_frame_stride,
                                                               const int32_t* __restrict__ lo,
                                                               const int32_t* __restrict__ hi,
                                                               int64_t* __restrict__ idx, float* __restrict__ best,
                                                               int frames, int H, int W, int D, int bs) {
  const long HW = (long)H * W, n = (long)frames * HW;
  const long pt = (long)blockIdx.x * 256 + threadIdx.x;
  const bool inside = pt < n;
  const long p = inside ? pt : n - 1;
  const long f = p / HW, px = p - f * HW;
  const int h = (int)(px / W), w = (int)(px - (long)h * W);
  const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
  const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
  const float* a = in0 + f * HW;
  const float* e = in1 + (in1_frame_stride ? f * HW : 0);
  const long Wo = (long)W + D - 1;
  const float2* ps = pstat + (in1_frame_stride ? f * (long)H * Wo : 0) + (long)h * Wo + (w + D - 1);
  const int half = bs / 2;
  const float bs2 = (float)(bs * bs);
  auto tap = [=](int bh, int bw) {
    return a[(long)clampi(h + bh - half, 0, H - 1) * W + clampi(w + bw - half, 0, W - 1)];
  };
  float bv = 0.f;
  int bi = -1;
  ncc_band_pixel<0>(tap, [=](int bh, int bw) { return tap(bh, bw) / bs2; }, e, ps, h, w, H, W, D, bs, l, u, bv, bi);
  if (inside) band_store(idx, best, p, bi, bv);
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

// ---------------------------------------------------------------------------------------------------------------------
// costs
// ---------------------------------------------------------------------------------------------------------------------

template <int TYPE>
__device__ inline float band_cost_term(float ev, float tv, float ec, float st, float eps, float bs2) {
  if (TYPE == 0 || TYPE == 1) {
    const float diff = ev - tv;
    return TYPE == 0 ? diff * diff / bs2 : fabsf(diff) / bs2;
  } else {
    const float diff = soft_step(ev - ec, eps) - st;            // st: the image side, independent of d
    return TYPE == 2 ? diff * diff / bs2 : fabsf(diff) / bs2;
  }
}

// candidates d0 .. d0 + K - 1 of pixel (h, w), w + half <= W - 1: no tap column is clamped at the right border, so
// pattern tap (bh, bw) of d0 + k is column clamp(w - half + bw - d0 - k) (a tap column clamped at the left border
// gives column 0 either way) -- the row span of ncc_band_group.  tap(bh, bw) = the image tap (replicate border).
template <int TYPE, int BS, int K, typename Tap>
__device__ inline void cost_band_group_span(Tap tap, const float* __restrict__ e, int h, int w, int H, int W, int d0,
                                            int hi, float tc, float eps, float& best, int& bi) {
  constexpr int half = BS / 2;
  const float bs2 = (float)(BS * BS);
  float ec[K], loss[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    ec[k] = TYPE >= 2 ? e[(long)h * W + clampi(w - d0 - k, 0, W - 1)] : 0.f;
    loss[k] = 0.f;
  }
  const int base = w - half - d0 - (K - 1);
  for (int bh = 0; bh < BS; ++bh) {
    const float* er = e + (long)clampi(h + bh - half, 0, H - 1) * W;
    float pr[BS + K - 1];
#pragma unroll
    for (int j = 0; j < BS + K - 1; ++j) pr[j] = er[clampi(base + j, 0, W - 1)];
#pragma unroll
    for (int bw = 0; bw < BS; ++bw) {
      const float tv = tap(bh, bw);
      const float st = TYPE >= 2 ? soft_step(tv - tc, eps) : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) loss[k] += band_cost_term<TYPE>(pr[bw + K - 1 - k], tv, ec[k], st, eps, bs2);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) band_take(loss[k], d0 + k, hi, false, best, bi);
}

// the same for any pixel and block size: every tap addressed as costvol_ref_cost addresses it
template <int TYPE, int K>
__device__ inline void cost_band_group_rt(const float* __restrict__ t, const float* __restrict__ e, int h, int w, int H,
                                          int W, int bs, int d0, int hi, float tc, float eps, float& best, int& bi) {
  const int half = bs / 2;
  const float bs2 = (float)(bs * bs);
  float ec[K], loss[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    ec[k] = TYPE >= 2 ? e[(long)h * W + clampi(w - d0 - k, 0, W - 1)] : 0.f;
    loss[k] = 0.f;
  }
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
    for (int bw = 0; bw < bs; ++bw) {
      const int wt = clampi(w + bw - half, 0, W - 1);
      const float tv = t[r + wt];
      const float st = TYPE >= 2 ? soft_step(tv - tc, eps) : 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k)
        loss[k] += band_cost_term<TYPE>(e[r + clampi(wt - d0 - k, 0, W - 1)], tv, ec[k], st, eps, bs2);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) band_take(loss[k], d0 + k, hi, false, best, bi);
}

// BS 3/5/7/9: 64 x 4 tiles as xcorrvol_band_kernel; BS 0: thread per pixel, block size bs_rt
template <int TYPE, int BS>
__global__ __launch_bounds__(256) void costvol_band_kernel(const float* __restrict__ im, const float* __restrict__ pat,
                                                           long pat_frame_stride, const int32_t* __restrict__ lo,
                                                           const int32_t* __restrict__ hi, int64_t* __restrict__ idx,
                                                           float* __restrict__ best, int frames, int H, int W, int D,
                                                           int bs_rt, float eps, int tiles_x, int tiles_y) {
  const long HW = (long)H * W;
  long f, p;
  int h, w;
  bool inside;
  if constexpr (BS > 0) {
    constexpr int SW = kBandTW + BS - 1, SH = kBandTH + BS - 1, half = BS / 2;
    __shared__ float sT[SH * SW];                               // the image tile + halo, replicate border baked in
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    f = blockIdx.x / tiles_x / tiles_y;
    const int h0 = ty * kBandTH, w0 = tx * kBandTW;
    const float* t = im + f * HW;
    for (int i = threadIdx.x; i < SH * SW; i += 256) {
      const int y = i / SW, x = i - y * SW;
      sT[i] = t[(long)clampi(h0 + y - half, 0, H - 1) * W + clampi(w0 + x - half, 0, W - 1)];
    }
    __syncthreads();
    const int lx = threadIdx.x & (kBandTW - 1), ly = threadIdx.x / kBandTW;
    inside = h0 + ly < H && w0 + lx < W;
    h = min(h0 + ly, H - 1);
    w = min(w0 + lx, W - 1);
    p = f * HW + (long)h * W + w;
    const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
    const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
    const float* e = pat + f * pat_frame_stride;
    const float* tT = sT + ly * SW + lx;
    auto tap = [=](int bh, int bw) { return tT[bh * SW + bw]; };
    const float tc = tT[half * SW + half];
    const bool span = w + half <= W - 1;
    float bv = 0.f;
    int bi = -1, d0 = l;
    while (true) {
      const int left = u - d0 + 1;
      if (!__any(left > 0)) break;
      if (__any(left > 4)) {
        if (span) cost_band_group_span<TYPE, BS, 8>(tap, e, h, w, H, W, d0, u, tc, eps, bv, bi);
        else cost_band_group_rt<TYPE, 8>(t, e, h, w, H, W, BS, d0, u, tc, eps, bv, bi);
        d0 = min(d0 + 8, D);
      } else {
        if (span) cost_band_group_span<TYPE, BS, 4>(tap, e, h, w, H, W, d0, u, tc, eps, bv, bi);
        else cost_band_group_rt<TYPE, 4>(t, e, h, w, H, W, BS, d0, u, tc, eps, bv, bi);
        d0 = min(d0 + 4, D);
      }
    }
    if (inside) band_store(idx, best, p, bi, bv);
  } else {
    const long n = (long)frames * HW;
    const long pt = (long)blockIdx.x * 256 + threadIdx.x;
    inside = pt < n;
    p = inside ? pt : n - 1;
    f = p / HW;
    const long px = p - f * HW;
    h = (int)(px / W);
    w = (int)(px - (long)h * W);
    const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
    const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
    const float* t = im + f * HW;
    const float* e = pat + f * pat_frame_stride;
    const float tc = t[(long)h * W + w];
    float bv = 0.f;
    int bi = -1, d0 = l;
    while (true) {
      const int left = u - d0 + 1;
      if (!__any(left > 0)) break;
      if (__any(left > 4)) {
        cost_band_group_rt<TYPE, 8>(t, e, h, w, H, W, bs_rt, d0, u, tc, eps, bv, bi);
        d0 = min(d0 + 8, D);
      } else {
        cost_band_group_rt<TYPE, 4>(t, e, h, w, H, W, bs_rt, d0, u, tc, eps, bv, bi);
        d0 = min(d0 + 4, D);
      }
    }
    if (inside) band_store(idx, best, p, bi, bv);
  }
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

static bool band_shape_ok(int frames, int H, int W, int D, int bs, long stride) {
  return vol_shape_ok(frames, 1, H, W, D, bs) && (bs & 1) != 0 && (stride == 0 || stride == (long)H * W);
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
