// ctd_band_score.h -- the scorers of band-limited matching, shared by band_match.hip (idx, best) and band_validity.hip
// (idx, best and the validity of the match): every reference-order score of a pixel's band [lo', hi'], once, in
// ascending d, handed to a sink.
//
// As in subpixel.hip, every score keeps its own accumulator chains in the reference's tap order (-ffp-contract=off), so
// its bits are the volume's:
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
// hi' keep computing on clamped addresses but their scores are not ranked.
//
// The cost volume clamps the tap column before it shifts (ctd_costvol_ref.h), so within `half` columns of the right
// border the taps of a row are no longer one shifted span; those lanes, and every block size without a template
// (3/5/7/9 have one), take the run-time group scorers, which address every tap on its own.
//
// A sink is what a pixel does with its scores:
//   void open(long row, int w)    once, before the first score: row = (f * H + h) * W, the flat index of the pixel's
//                                 row (a lane outside the image has an empty band and is never given a score);
//   void take(float s, int d)     the score of candidate d, lo' <= d <= hi', in ascending d.
// BandBest is the sink of the band matchers: a running (best, first index) with a strict compare.
#pragma once
#include "ctd_common.h"
#include "ctd_costvol_ref.h"
#include "ctd_ncc_point.h"
#include "ctd_subpixel_ws.h"
#include "ctd_validate.h"

namespace ctd {

constexpr int kBandTW = 64, kBandTH = 4;         // pixel tile of a workgroup (256 threads)

template <bool MAXI>
struct BandBest {
  float best;
  int bi;
  __device__ inline void open(long, int) {
    best = 0.f;
    bi = -1;
  }
  __device__ inline void take(float s, int d) {
    if (bi < 0 || (MAXI ? s > best : s < best)) {
      best = s;
      bi = d;
    }
  }
};

// ---------------------------------------------------------------------------------------------------------------------
// NCC
// ---------------------------------------------------------------------------------------------------------------------

// candidates d0 .. d0 + K - 1 of pixel (h, w); ps = the (mu1, s1) row of h at x = w (ps[-d]: the window centred w - d);
// tap(bh, bw) = the frame tap.  Pattern tap (bh, bw) of d0 + k is column clamp(w - half + bw - d0 - k): sample
// bw + K - 1 - k of the row span that starts at w - half - d0 - (K - 1).
template <int BS, int K, typename Tap, typename Sink>
__device__ inline void ncc_band_group(Tap tap, const float* __restrict__ e, const float2* __restrict__ ps, int h, int w,
                                      int H, int W, int D, int bs_rt, int d0, int hi, float mu0, float s0, Sink& sk) {
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
    if (d0 + k <= hi) sk.take(s, d0 + k);
  }
}

// the frame half, then the groups; every lane of the wavefront must call this (the group width is wave-uniform)
template <int BS, typename Tap, typename TapQ, typename Sink>
__device__ inline void ncc_band_pixel(Tap tap, TapQ tapq, const float* __restrict__ e, const float2* __restrict__ ps,
                                      int h, int w, int H, int W, int D, int bs_rt, int lo, int hi, Sink& sk) {
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
      ncc_band_group<BS, 8>(tap, e, ps, h, w, H, W, D, bs_rt, d0, hi, mu0, s0, sk);
      d0 = min(d0 + 8, D);
    } else {
      ncc_band_group<BS, 4>(tap, e, ps, h, w, H, W, D, bs_rt, d0, hi, mu0, s0, sk);
      d0 = min(d0 + 4, D);
    }
  }
}

// block sizes 3/5/7/9: the pixel of this thread in the 64 x 4 tile of workgroup blockIdx.x =
// (f * tiles_y + ty) * tiles_x + tx, scored into sk.  p = the pixel's flat index; returns false for a thread outside the
// image (which must not store).
template <int BS, typename Sink>
__device__ inline bool xcorrvol_band_tile(const float* __restrict__ in0, const float* __restrict__ in1,
                                          const float2* __restrict__ pstat, long in1_frame_stride,
                                          const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int H, int W,
                                          int D, int tiles_x, int tiles_y, Sink& sk, long& p) {
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
  p = f * HW + (long)h * W + w;
  const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
  const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
  const float* e = in1 + (in1_frame_stride ? f * HW : 0);
  const long Wo = (long)W + D - 1;
  const float2* ps = pstat + (in1_frame_stride ? f * (long)H * Wo : 0) + (long)h * Wo + (w + D - 1);
  const float* tA = sA + ly * SW + lx;
  const float* tQ = sAq + ly * SW + lx;
  sk.open(p - w, w);
  ncc_band_pixel<BS>([=](int bh, int bw) { return tA[bh * SW + bw]; }, [=](int bh, int bw) { return tQ[bh * SW + bw]; },
                     e, ps, h, w, H, W, D, BS, l, u, sk);
  return inside;
}

// any other odd block size: thread per pixel, every tap from global memory
template <typename Sink>
__device__ inline bool xcorrvol_band_rt_pixel(const float* __restrict__ in0, const float* __restrict__ in1,
                                              const float2* __restrict__ pstat, long in1_frame_stride,
                                              const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int frames,
                                              int H, int W, int D, int bs, Sink& sk, long& p) {
  const long HW = (long)H * W, n = (long)frames * HW;
  const long pt = (long)blockIdx.x * 256 + threadIdx.x;
  const bool inside = pt < n;
  p = inside ? pt : n - 1;
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
  sk.open(p - w, w);
  ncc_band_pixel<0>(tap, [=](int bh, int bw) { return tap(bh, bw) / bs2; }, e, ps, h, w, H, W, D, bs, l, u, sk);
  return inside;
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
template <int TYPE, int BS, int K, typename Tap, typename Sink>
__device__ inline void cost_band_group_span(Tap tap, const float* __restrict__ e, int h, int w, int H, int W, int d0,
                                            int hi, float tc, float eps, Sink& sk) {
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
  for (int k = 0; k < K; ++k) {
    if (d0 + k <= hi) sk.take(loss[k], d0 + k);
  }
}

// the same for any pixel and block size: every tap addressed as costvol_ref_cost addresses it
template <int TYPE, int K, typename Sink>
__device__ inline void cost_band_group_rt(const float* __restrict__ t, const float* __restrict__ e, int h, int w, int H,
                                          int W, int bs, int d0, int hi, float tc, float eps, Sink& sk) {
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
  for (int k = 0; k < K; ++k) {
    if (d0 + k <= hi) sk.take(loss[k], d0 + k);
  }
}

// BS 3/5/7/9: the pixel of this thread in a 64 x 4 tile, as xcorrvol_band_tile; BS 0: thread per pixel, block size
// bs_rt.  p and the return value as there.
template <int TYPE, int BS, typename Sink>
__device__ inline bool costvol_band_pixel(const float* __restrict__ im, const float* __restrict__ pat,
                                          long pat_frame_stride, const int32_t* __restrict__ lo,
                                          const int32_t* __restrict__ hi, int frames, int H, int W, int D, int bs_rt,
                                          float eps, int tiles_x, int tiles_y, Sink& sk, long& p) {
  const long HW = (long)H * W;
  if constexpr (BS > 0) {
    constexpr int SW = kBandTW + BS - 1, SH = kBandTH + BS - 1, half = BS / 2;
    __shared__ float sT[SH * SW];                               // the image tile + halo, replicate border baked in
    const int tx = blockIdx.x % tiles_x;
    const int ty = (blockIdx.x / tiles_x) % tiles_y;
    const long f = blockIdx.x / tiles_x / tiles_y;
    const int h0 = ty * kBandTH, w0 = tx * kBandTW;
    const float* t = im + f * HW;
    for (int i = threadIdx.x; i < SH * SW; i += 256) {
      const int y = i / SW, x = i - y * SW;
      sT[i] = t[(long)clampi(h0 + y - half, 0, H - 1) * W + clampi(w0 + x - half, 0, W - 1)];
    }
    __syncthreads();
    const int lx = threadIdx.x & (kBandTW - 1), ly = threadIdx.x / kBandTW;
    const bool inside = h0 + ly < H && w0 + lx < W;
    const int h = min(h0 + ly, H - 1), w = min(w0 + lx, W - 1);
    p = f * HW + (long)h * W + w;
    const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
    const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
    const float* e = pat + f * pat_frame_stride;
    const float* tT = sT + ly * SW + lx;
    auto tap = [=](int bh, int bw) { return tT[bh * SW + bw]; };
    const float tc = tT[half * SW + half];
    const bool span = w + half <= W - 1;
    sk.open(p - w, w);
    int d0 = l;
    while (true) {
      const int left = u - d0 + 1;
      if (!__any(left > 0)) break;
      if (__any(left > 4)) {
        if (span) cost_band_group_span<TYPE, BS, 8>(tap, e, h, w, H, W, d0, u, tc, eps, sk);
        else cost_band_group_rt<TYPE, 8>(t, e, h, w, H, W, BS, d0, u, tc, eps, sk);
        d0 = min(d0 + 8, D);
      } else {
        if (span) cost_band_group_span<TYPE, BS, 4>(tap, e, h, w, H, W, d0, u, tc, eps, sk);
        else cost_band_group_rt<TYPE, 4>(t, e, h, w, H, W, BS, d0, u, tc, eps, sk);
        d0 = min(d0 + 4, D);
      }
    }
    return inside;
  } else {
    const long n = (long)frames * HW;
    const long pt = (long)blockIdx.x * 256 + threadIdx.x;
    const bool inside = pt < n;
    p = inside ? pt : n - 1;
    const long f = p / HW;
    const long px = p - f * HW;
    const int h = (int)(px / W), w = (int)(px - (long)h * W);
    const int l = inside ? clampi(lo[p], 0, D) : 0;          // (any int32 is legal: no overflow below)
    const int u = inside ? clampi(hi[p], -1, D - 1) : -1;
    const float* t = im + f * HW;
    const float* e = pat + f * pat_frame_stride;
    const float tc = t[(long)h * W + w];
    sk.open(p - w, w);
    int d0 = l;
    while (true) {
      const int left = u - d0 + 1;
      if (!__any(left > 0)) break;
      if (__any(left > 4)) {
        cost_band_group_rt<TYPE, 8>(t, e, h, w, H, W, bs_rt, d0, u, tc, eps, sk);
        d0 = min(d0 + 8, D);
      } else {
        cost_band_group_rt<TYPE, 4>(t, e, h, w, H, W, bs_rt, d0, u, tc, eps, sk);
        d0 = min(d0 + 4, D);
      }
    }
    return inside;
  }
}

__device__ inline void band_store(int64_t* __restrict__ idx, float* __restrict__ best, long p, int bi, float bv) {
  idx[p] = bi;
  if (best) best[p] = bi < 0 ? __builtin_nanf("") : bv;
}

inline bool band_shape_ok(int frames, int H, int W, int D, int bs, long stride) {
  return vol_shape_ok(frames, 1, H, W, D, bs) && (bs & 1) != 0 && (stride == 0 || stride == (long)H * W);
}

}  // namespace ctd
