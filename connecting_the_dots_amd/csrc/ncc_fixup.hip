// ncc_fixup.hip -- fix-up pass of the fast NCC path: the outputs of the windows the pre-pass listed, recomputed in the
// reference's operation order (the stages of a call: ncc_fast.hip).  Two kernels, one per call kind:
//   ncc_fixup_kernel        table-less calls: one wavefront per listed window (a shared single-channel pattern window: per
//                           group of kFixFrames frames), which stages and reduces the window's own side itself;
//   ncc_fixup_items_kernel  calls on a prepared pattern (block 9, single channel): the pattern side of every listed
//                           pattern window comes from a table that ncc_fixup_table_kernel filled when the pattern was
//                           prepared (81 centred taps + their sum of squares per window), and an item is (listed pattern
//                           window, ONE frame, ONE block of 64 disparities) -- a quarter of the dependent work per
//                           wavefront, four times the wavefronts.  Listed frame windows and pattern windows past the
//                           table's cap keep the in-kernel staging, in the same launch.
// Both give the same bits: the table rows are computed by the device function the table-less kernel runs per item.
#include "ctd_ncc_fast.h"
#include "ctd_ncc_point.h"
#include "ctd_rank.h"
#include "ctd_tail.h"
#include "ctd_post_stamps.h"

namespace ctd {

// Fix-up pass of the fast path.
//
// Error model of the fast kernel (tools/err_vs_factor.py): cov = S_ab - n*ma*mb is formed from values
// centred by one constant per image, so |fast - exact| <~ c * 2^-24 * sqrt(Fa * Fb) per channel with
// F = 1 + n*(window mean - centring)^2 / (sum of squared deviations) per window and c <= ~7 (ten f32
// roundings along the longest summation path; 6.3 measured on clipped plateaus, tests/test_matcher_bounds_gpu.py),
// plus |NCC| * 1e-8 / (sa * sb) for the reference denominator's 1e-8, which kDevFloor keeps <= 2.1e-6 relative.
// The pre-pass lists every window with F - 1 > kFlagRatio / C (and marks it with a zero reciprocal deviation), so an
// unlisted output has sum_c sqrt(Fa * Fb) <= C + kFlagRatio, and kFlagRatio = 1.39 makes 7 * 2^-24 * (C + 1.39)
// <= C * 1e-6: the contract |a-b| <= 1e-5|b| + 1e-6 holds for C = 1, and for C > 1 the sum of the per-channel bounds,
// 1e-5 * sum_c |b_c| + C * 1e-6 (include/ctd_hip.h) -- where channels cancel, the reference order's own rounding of
// its C channels (1.6e-6 from float64 at C = 2) already exceeds a single 1e-6.  LCN'd input has F ~ 1 except in flat
// regions and in the low-variance windows clamped to column 0.  This kernel visits the listed windows and recomputes
// every output they take part in in the reference's operation order
// (bit-identical to CTD_NCC_EXACT).
// One wavefront per listed window, lane <-> disparity; the window itself (FIX, bs x bs) and the rows of
// the other image it meets over all disparities (SPAN, bs x (bs + D - 1)) are staged in LDS per channel.
//   frame window  (f, h, w): outputs (f, d, h, w);        SPAN = pattern columns w-half-(D-1) .. w+half
//   pattern window (p, h, x): outputs (f, d, h, x + d), 0 <= x + d < W, every frame f that uses p;
//                             SPAN = frame columns x-half .. x+(D-1)+half.  x = -(bs-1-half) stands for all
//                             fully clamped windows x <= -(bs-1-half): lane d's value is written to the
//                             whole run d' >= d of pixel w = x + d (ext.h:152-154 makes the run constant).
// The NCC is symmetric in the two windows (dot and sigma0*sigma1 commute exactly), so one staging layout
// serves both cases.
// Ranked calls (ncc_fast_fixup_ranked, after the all-D kernel): the in-kernel ranking saw the placeholder score 0
// instead of these, so every recomputed one is held against the pixel's best; a pixel whose best is not clear of it by
// the re-ranking margin, or whose index IS the placeholder's disparity, joins the work list of the exact re-scoring
// (once: its flag byte is claimed atomically).  `out` may be null then (nothing was materialised).
constexpr int kFixupBlocks = 2048;

// Loops over the window rows stay rolled (a fully unrolled body is ~40 KB of straight-line code that every
// wavefront executes once -- instruction-fetch bound); BS > 0 unrolls the inner tap loop only.
// Outputs of the fully clamped run are not written here (one store per disparity plane and lane thrashes
// the TLB): the run's value goes to `run_vals[f][h][d_first]` (NaN = keep the fast value) and
// ncc_fixup_runs_kernel spreads it plane by plane.
// A pattern window shared by all frames (single channel) is one item per group of kFixFrames frames: its own side
// (window, mean, deviations) is staged once, the frames' rows follow one another with the next frame's rows already
// on their way (register prefetch) -- the pass is latency-bound, a lone wavefront per item, and this takes the global
// round trips of all but the first frame off its critical path.  Same arithmetic, same order as the generic path.
constexpr int kFixFrames = 2;
constexpr int kFixSpanRegs = 20;       // prefetched SPAN elements per lane (bs * (bs + D - 1) <= 64 * 20)

// Pattern side of an item whose FIX window is a pattern window: the window raw (sF), every tap divided by n (sFq: the
// reference divides before it sums), the row-major sum of the quotients as the mean, the centred taps (sFv) and the
// row-major sum of their squares, which is returned.  One wavefront, wave-private LDS.  The fix-up kernel (table-less
// calls) and ncc_fixup_table_kernel (prepared patterns) both run THIS code, so a table row carries the bits the kernel
// would have staged itself.
template <int BS>
__device__ __forceinline__ float fixup_pattern_side(const float* __restrict__ img, int h, int col, int H, int W, int bs_rt,
                                                    float* sF, float* sFq, float* sFv, int lane) {
  const int bs = BS > 0 ? BS : bs_rt;
  const int half = bs / 2, taps = bs * bs;
  const float n = (float)taps;
  for (int i0 = lane; i0 < taps; i0 += 64 * 2) {
    float t[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = min(i0 + 64 * u, taps - 1);
      const int bh = i / bs, bw = i - bh * bs;
      t[u] = img[(long)clampi(h + bh - half, 0, H - 1) * W + clampi(col + bw - half, 0, W - 1)];
    }
#pragma unroll
    for (int u = 0; u < 2; ++u)
      if (i0 + 64 * u < taps) {
        sF[i0 + 64 * u] = t[u];
        sFq[i0 + 64 * u] = t[u] / n;
      }
  }
  float mu_f = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
#pragma unroll
    for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) mu_f += sFq[bh * BS + bw];
    if (BS == 0)
      for (int bw = 0; bw < bs; ++bw) mu_f += sFq[bh * bs + bw];
  }
  for (int i = lane; i < taps; i += 64) sFv[i] = sF[i] - mu_f;
  float s_f = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
#pragma unroll
    for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) s_f += sFv[bh * BS + bw] * sFv[bh * BS + bw];
    if (BS == 0)
      for (int bw = 0; bw < bs; ++bw) s_f += sFv[bh * bs + bw] * sFv[bh * bs + bw];
  }
  return s_f;
}

template <int BS>
__device__ __forceinline__ void fixup_grouped_item(const float* __restrict__ in0, const float* __restrict__ in1,
                                                float* __restrict__ out, float* __restrict__ run_vals,
                                                const float* __restrict__ best, unsigned long long* __restrict__ idx,
                                                float rank_eps,
                                                unsigned* __restrict__ flags, WorkList work, float* sF, float* sFq,
                                                float* sFv,
                                                float* sS, float* sSq, int f_lo, int f_hi, int h, int col, bool run_item,
                                                int H, int W, int D, int bs_rt, int lane, unsigned* stamp) {
  const int bs = BS > 0 ? BS : bs_rt;
  const int half = bs / 2, span = bs + D - 1, taps = bs * bs;
  const float n = (float)taps;
  const long HW = (long)H * W;
  const int span_col0 = col - half;
  // the lane's SPAN element offsets inside a frame (the same for every frame) and the first frame's elements
  float pre[kFixSpanRegs];
  int soff[kFixSpanRegs];
#pragma unroll
  for (int k = 0; k < kFixSpanRegs; ++k) {
    const int i = min(lane + 64 * k, bs * span - 1);
    const int bh = i / span, cc = i - bh * span;
    soff[k] = clampi(h + bh - half, 0, H - 1) * W + clampi(span_col0 + cc, 0, W - 1);
    pre[k] = in0[(long)f_lo * HW + soff[k]];
  }
  const float s_f = fixup_pattern_side<BS>(in1, h, col, H, W, bs, sF, sFq, sFv, lane);
  CTD_POST_STAMP_V(stamp, 3, s_f);                             // pattern side ready
  const int rounds = (D + 127) / 128;
  // ranked calls: contenders of the whole item are claimed and pushed at its end, all atomics in flight together
  constexpr int kCand = kFixFrames * 2;
  bool cand[kCand];
  long cpix[kCand];
#pragma unroll
  for (int i = 0; i < kCand; ++i) { cand[i] = false; cpix[i] = 0; }
  auto flush_candidates = [&]() {
    if (!best) return;
    bool tk[kCand];
#pragma unroll
    for (int i = 0; i < kCand; ++i) tk[i] = cand[i] && worklist_claim(flags, cpix[i]);
#pragma unroll
    for (int g = 0; g < kFixFrames; ++g)                       // the two candidates of a frame lie in one image row
      worklist_push2_same_row(tk[2 * g], cpix[2 * g], tk[2 * g + 1], cpix[2 * g + 1], work);
#pragma unroll
    for (int i = 0; i < kCand; ++i) cand[i] = false;
  };
  for (int f = f_lo; f < f_hi; ++f) {
    // this frame's rows come out of the prefetch registers; the next frame's are requested right away
#pragma unroll
    for (int k = 0; k < kFixSpanRegs; ++k)
      if (lane + 64 * k < bs * span) {
        sS[lane + 64 * k] = pre[k];
        sSq[lane + 64 * k] = pre[k] / n;
      }
    if (f + 1 < f_hi) {
#pragma unroll
      for (int k = 0; k < kFixSpanRegs; ++k) pre[k] = in0[(long)(f + 1) * HW + soff[k]];
    }
    if (f == f_lo) CTD_POST_STAMP(stamp, 4);                   // span staged (the stamps 4..8: first frame, first round)
    // two disparities per lane and pass (d, d + 64): two independent serial chains in flight -- a lone wavefront
    // spends this loop waiting for its own LDS reads and dependent adds
    for (int r = 0; r < rounds; ++r) {
      int dd[2];
      bool bad[2];
      float val[2], mb[2];
      bool won[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        dd[t] = r * 128 + 64 * t + lane;
        const int w = col + dd[t];
        bad[t] = dd[t] < D && w >= 0 && w < W;
        val[t] = 0.f;
        // the pixel's best score and index (ranked calls): requested now, needed after the exact evaluation
        mb[t] = (best && bad[t]) ? best[((long)f * H + h) * W + w] : 0.f;
        won[t] = best && bad[t] && idx[((long)f * H + h) * W + w] == (unsigned long long)dd[t];   // the placeholder came out on top
      }
      const int o0 = min(dd[0], D - 1), o1 = min(dd[1], D - 1);    // clamped: lanes past D read valid LDS, results unused
      if (__any(bad[0] || bad[1])) {
        float mu0 = 0.f, mu1 = 0.f;
        for (int bh = 0; bh < bs; ++bh) {
          const float* q0 = sSq + bh * span + o0;
          const float* q1 = sSq + bh * span + o1;
#pragma unroll
          for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) { mu0 += q0[bw]; mu1 += q1[bw]; }
          if (BS == 0)
            for (int bw = 0; bw < bs; ++bw) { mu0 += q0[bw]; mu1 += q1[bw]; }
        }
        if (f == f_lo && r == 0) CTD_POST_STAMP_V(stamp, 5, mu0 + mu1);   // means done
        float ss0 = 0.f, ss1 = 0.f, dot0 = 0.f, dot1 = 0.f;
        for (int bh = 0; bh < bs; ++bh) {
          const float* x0 = sS + bh * span + o0;
          const float* x1 = sS + bh * span + o1;
          const float* vf = sFv + bh * bs;
#pragma unroll
          for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) {
            const float v0 = x0[bw] - mu0, v1 = x1[bw] - mu1;
            dot0 += vf[bw] * v0;
            ss0 += v0 * v0;
            dot1 += vf[bw] * v1;
            ss1 += v1 * v1;
          }
          if (BS == 0)
            for (int bw = 0; bw < bs; ++bw) {
              const float v0 = x0[bw] - mu0, v1 = x1[bw] - mu1;
              dot0 += vf[bw] * v0;
              ss0 += v0 * v0;
              dot1 += vf[bw] * v1;
              ss1 += v1 * v1;
            }
        }
        val[0] = 0.f + dot0 / ncc_norm(s_f, ss0);            // "T val = 0; val += dot / norm" (ext.h:142,186)
        val[1] = 0.f + dot1 / ncc_norm(s_f, ss1);
      }
      if (f == f_lo && r == 0) CTD_POST_STAMP_V(stamp, 6, val[0] + val[1]);   // chains done
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int d = dd[t], w = col + d;
        if (run_item) {
          if (d < D) run_vals[((long)f * H + h) * D + d] = bad[t] ? val[t] : __int_as_float(0x7fc00000);
        } else if (bad[t]) {
          if (out) out[((long)f * D + d) * HW + (long)h * W + w] = val[t];
        }
        if (best) {                                            // wave-uniform: ranked call
          const long pixc = ((long)f * H + h) * W + w;
          // clearly above everything the ranking saw: straight into the pixel's index word (ctd_tail.h); inside the
          // margin of the best, or the placeholder itself came out on top with no such lead: exact re-scoring
          const bool clear = bad[t] && val[t] > mb[t] + rank_margin(rank_eps, mb[t]);
          if (clear) atomicMax(idx + pixc, patch_key(val[t], d));
          const bool contender = bad[t] && !clear && (won[t] || !(val[t] < mb[t] - rank_margin(rank_eps, mb[t])));
          if (rounds == 1) {                                   // one slot per (frame of the item, t): flushed at the end
#pragma unroll
            for (int i = 0; i < kCand; ++i)
              if (i == (f - f_lo) * 2 + t) { cand[i] = contender; cpix[i] = ((long)f * H + h) * W + w; }
          } else {
            const long pix = ((long)f * H + h) * W + w;
            worklist_push(contender && worklist_claim(flags, pix), pix, work);
          }
        }
      }
      if (f == f_lo && r == 0) CTD_POST_STAMP(stamp, 7);       // best / idx compared, volume and patch stores issued
    }
  }
  flush_candidates();
  CTD_POST_STAMP(stamp, 8);                                    // stores issued (work-list appends of the whole item)
}

// One item of the generic path: every output of the listed window (is_a: frame window of frame f | pattern window met by
// frame f), all channels, 64 disparities per round.  `lds`: this wavefront's 3 * taps + 2 * bs * span floats.
template <int BS>
__device__ __forceinline__ void fixup_generic_item(const float* __restrict__ in0, const float* __restrict__ in1,
                                                   long in1_frame_stride, float* __restrict__ out,
                                                   float* __restrict__ run_vals, const float* __restrict__ best,
                                                   unsigned long long* __restrict__ idx, float rank_eps,
                                                   unsigned* __restrict__ flags, WorkList work, float* lds, bool is_a, int f,
                                                   int h, int col, bool run_item, int C, int H, int W, int D, int bs_rt,
                                                   int lane) {
  const int bs = BS > 0 ? BS : bs_rt;
  const int half = bs / 2, span = bs + D - 1, taps = bs * bs;
  const float n = (float)taps;
  float* sF = lds;
  float* sFq = sF + taps;
  float* sFv = sFq + taps;
  float* sS = sFv + taps;
  float* sSq = sS + bs * span;
  const long HW = (long)H * W;
  const int rounds = (D + 63) / 64;
  const float* fix_img = is_a ? in0 + (long)f * C * HW : in1 + (long)f * in1_frame_stride;
  const float* span_img = is_a ? in1 + (long)f * in1_frame_stride : in0 + (long)f * C * HW;
  const int span_col0 = is_a ? col - half - (D - 1) : col - half;
  int staged_c = -1;
  float mu_f = 0.f, s_f = 0.f;
  for (int r = 0; r < rounds; ++r) {
    const int d = r * 64 + lane;
    const int w = is_a ? col : col + d;
    // every output of a listed window is recomputed (the fast kernels wrote NaN there)
    const bool bad = d < D && w >= 0 && w < W;
    float val = 0.f;
    const float mbest = (best && bad) ? best[((long)f * H + h) * W + w] : 0.f;   // ranked calls: needed at the end
    const bool won = best && bad && idx[((long)f * H + h) * W + w] == (unsigned long long)d;   // the placeholder came out on top
    if (__any(bad)) {
      for (int c = 0; c < C; ++c) {
        if (staged_c != c) {
          staged_c = c;
          // batches of independent loads: a lone wavefront must not pay one memory round trip per element
          for (int i0 = lane; i0 < taps; i0 += 64 * 2) {
            float t[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
              const int i = min(i0 + 64 * u, taps - 1);
              const int bh = i / bs, bw = i - bh * bs;
              t[u] = fix_img[(long)c * HW + (long)clampi(h + bh - half, 0, H - 1) * W + clampi(col + bw - half, 0, W - 1)];
            }
#pragma unroll
            for (int u = 0; u < 2; ++u)
              if (i0 + 64 * u < taps) {
                sF[i0 + 64 * u] = t[u];
                sFq[i0 + 64 * u] = t[u] / n;            // the reference divides every tap before summing
              }
          }
          for (int i0 = lane; i0 < bs * span; i0 += 64 * 8) {
            float t[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
              const int i = min(i0 + 64 * u, bs * span - 1);
              const int bh = i / span, cc = i - bh * span;
              t[u] = span_img[(long)c * HW + (long)clampi(h + bh - half, 0, H - 1) * W + clampi(span_col0 + cc, 0, W - 1)];
            }
#pragma unroll
            for (int u = 0; u < 8; ++u)
              if (i0 + 64 * u < bs * span) {
                sS[i0 + 64 * u] = t[u];
                sSq[i0 + 64 * u] = t[u] / n;
              }
          }
          // the FIX side (mean, deviations, sigma) is the same for every disparity: once per staging
          mu_f = 0.f;
          for (int bh = 0; bh < bs; ++bh) {
#pragma unroll
            for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) mu_f += sFq[bh * BS + bw];
            if (BS == 0)
              for (int bw = 0; bw < bs; ++bw) mu_f += sFq[bh * bs + bw];
          }
          for (int i = lane; i < taps; i += 64) sFv[i] = sF[i] - mu_f;
          s_f = 0.f;
          for (int bh = 0; bh < bs; ++bh) {
#pragma unroll
            for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) s_f += sFv[bh * BS + bw] * sFv[bh * BS + bw];
            if (BS == 0)
              for (int bw = 0; bw < bs; ++bw) s_f += sFv[bh * bs + bw] * sFv[bh * bs + bw];
          }
        }
        if (bad) {
          const int off = is_a ? (D - 1) - d : d;
          float mu_s = 0.f, s_s = 0.f, dot = 0.f;
          for (int bh = 0; bh < bs; ++bh) {
            const float* q = sSq + bh * span + off;
#pragma unroll
            for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) mu_s += q[bw];
            if (BS == 0)
              for (int bw = 0; bw < bs; ++bw) mu_s += q[bw];
          }
          for (int bh = 0; bh < bs; ++bh) {
            const float* x = sS + bh * span + off;
            const float* vf = sFv + bh * bs;
#pragma unroll
            for (int bw = 0; bw < (BS > 0 ? BS : 0); ++bw) {
              const float vs = x[bw] - mu_s;
              dot += vf[bw] * vs;
              s_s += vs * vs;
            }
            if (BS == 0)
              for (int bw = 0; bw < bs; ++bw) {
                const float vs = x[bw] - mu_s;
                dot += vf[bw] * vs;
                s_s += vs * vs;
              }
          }
          val += dot / ncc_norm(s_f, s_s);              // ext.h:185-186 (sigma0 * sigma1 commutes)
        }
      }
    }
    if (run_item) {
      if (d < D) run_vals[((long)f * H + h) * D + d] = bad ? val : __int_as_float(0x7fc00000);
    } else if (bad) {
      if (out) out[((long)f * D + d) * HW + (long)h * W + w] = val;
    }
    if (best) {                                            // wave-uniform: ranked call
      bool take = false;
      const long pix = ((long)f * H + h) * W + w;
      const bool clear = bad && val > mbest + rank_margin(rank_eps, mbest);      // (see the grouped path)
      if (clear) atomicMax(idx + pix, patch_key(val, d));
      if (bad && !clear && (won || !(val < mbest - rank_margin(rank_eps, mbest)))) take = worklist_claim(flags, pix);
      worklist_push(take, pix, work);
    }
  }
}

template <int BS>
__global__ __launch_bounds__(256, 2) void ncc_fixup_kernel(const float* __restrict__ in0, const float* __restrict__ in1,
                                                        long in1_frame_stride, float* __restrict__ out,
                                                        unsigned* __restrict__ counters,
                                                        const unsigned long long* __restrict__ list_a,
                                                        const unsigned long long* __restrict__ list_b,
                                                        float* __restrict__ run_vals,
                                                        const float* __restrict__ best,
                                                        unsigned long long* __restrict__ idx, float rank_eps,
                                                        unsigned* __restrict__ flags, WorkList work, int frames, int C, int H,
                                                        int W, int D, int bs_rt) {
  extern __shared__ float lds_fix[];
  const int bs = BS > 0 ? BS : bs_rt;
  const int lane = threadIdx.x & 63;
  const int half = bs / 2, span = bs + D - 1, taps = bs * bs;
  // per-wave staging: FIX window raw / divided by n / minus its mean, SPAN rows raw / divided by n
  float* sF = lds_fix + (threadIdx.x >> 6) * (3 * taps + 2 * bs * span);
  float* sFq = sF + taps;
  float* sFv = sFq + taps;
  float* sS = sFv + taps;
  float* sSq = sS + bs * span;
  unsigned* stamp = CTD_POST_STAMP_SLOT(0u);                    // entry
  const unsigned n_a = counters[0], n_b = counters[1];
  CTD_POST_STAMP_S(stamp, 1, n_b);                             // counters read
  // ranked calls: the tail kernel reads the number of listed frame windows from slot 3 and clears slot 0 for the next
  // call's pre-pass (which counts in it) -- no memset launch in front of a call on a prepared pattern
  if (best && blockIdx.x == 0 && threadIdx.x == 0) counters[3] = n_a;
  const unsigned per_b = in1_frame_stride == 0 ? (unsigned)frames : 1u;   // a shared pattern window meets every frame
  // single channel, shared pattern, SPAN small enough for the prefetch registers: kFixFrames frames per item
  const bool grouped = per_b > 1u && C == 1 && bs * span <= 64 * kFixSpanRegs;
  const unsigned groups = grouped ? (per_b + kFixFrames - 1) / kFixFrames : per_b;
  const unsigned n_items = n_a + n_b * groups;
  const unsigned n_waves = gridDim.x * (blockDim.x >> 6);
  for (unsigned item = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); item < n_items; item += n_waves) {
    const bool is_a = item < n_a;
    const unsigned jb = is_a ? 0u : (item - n_a) / groups;
    const unsigned long long e = is_a ? list_a[item] : list_b[jb];
    const int z = (int)(e >> 40), h = (int)((e >> 20) & 0xFFFFF), col = (int)(e & 0xFFFFF) - 0x80000;
    const bool run_item = !is_a && col == -(bs - 1 - half);
    CTD_POST_STAMP_S(stamp, 2, col);                           // list entry read
    CTD_POST_STAMP_ITEM(stamp);
    if (grouped && !is_a) {
      const int f_lo = (int)((item - n_a) - jb * groups) * kFixFrames;
      fixup_grouped_item<BS>(in0, in1, out, run_vals, best, idx, rank_eps, flags, work, sF, sFq, sFv, sS, sSq,
                             f_lo, min(frames, f_lo + kFixFrames), h, col, run_item, H, W, D, bs, lane, stamp);
      CTD_POST_STAMP(stamp, 9);                                // exit of the wavefront's first item
      stamp = nullptr;
      continue;
    }
    const int f = (is_a || per_b == 1u) ? z / C : (int)((item - n_a) - jb * groups);
    fixup_generic_item<BS>(in0, in1, in1_frame_stride, out, run_vals, best, idx, rank_eps, flags, work, sF, is_a, f, h, col,
                           run_item, C, H, W, D, bs, lane);
  }
}

// ---- Prepared patterns (block 9, single channel): pattern-side tables and one-frame items --------------------------
//
// The pattern side of a pattern-window item (centred taps, sum of their squares) does not depend on the frames.
// ncc_fixup_table_kernel computes it ONCE, when the pattern is prepared, for the first fixup_table_rows() entries of
// `list_b` (ctd_ncc_fast.h: at most kFixTabCap, and what fits in the unused end of the list's buffer, where the table
// lives; row j of the table <-> list_b[j], at tab_end - (j + 1) rows; kFixTabRow floats: 81 centred taps, their sum of squares, 2 of padding), with
// fixup_pattern_side, the code the table-less kernel runs per item -- the bits are the same by construction.
__global__ __launch_bounds__(256) void ncc_fixup_table_kernel(const float* __restrict__ in1, long in1_frame_stride,
                                                              const unsigned* __restrict__ counters,
                                                              const unsigned long long* __restrict__ list_b,
                                                              unsigned list_b_cap, float* __restrict__ tab_end, int H,
                                                              int W) {
  __shared__ float s_side[4 * 3 * 81];
  const int lane = threadIdx.x & 63;
  float* sF = s_side + (threadIdx.x >> 6) * (3 * 81);
  float* sFq = sF + 81;
  float* sFv = sFq + 81;
  const unsigned n_t = fixup_table_rows(counters[1], list_b_cap);
  for (unsigned j = blockIdx.x * 4 + (threadIdx.x >> 6); j < n_t; j += gridDim.x * 4) {
    const unsigned long long e = list_b[j];
    const int z = (int)(e >> 40), h = (int)((e >> 20) & 0xFFFFF), col = (int)(e & 0xFFFFF) - 0x80000;
    const float s_f = fixup_pattern_side<9>(in1 + (long)z * in1_frame_stride, h, col, H, W, 9, sF, sFq, sFv, lane);
    float* row = tab_end - (size_t)(j + 1) * kFixTabRow;
    for (int i = lane; i < 81; i += 64) row[i] = sFv[i];
    if (lane < kFixTabRow - 81) row[81 + lane] = lane == 0 ? s_f : 0.f;
  }
}

// One item of the table path: (listed pattern window, frame f, the 64 disparities d0 .. d0 + 63), lane <-> disparity.
// Everything the item reads from global memory -- the 9 x (9 + 63) frame elements the block meets, the table row, the
// lane's best score and index word -- is requested in one batch; one chain per lane follows.  Per output the
// operations and their order are those of the generic path: mean over the 81 quotients row-major, centred products
// row-major, ncc_norm, 0.f + dot / norm.  The span lives in LDS ONCE: first divided by n, for the means; then the raw
// elements, still in the registers they were loaded into, are written over the quotients for the products (one
// wavefront, LDS operations in order: every lane's reads of the quotients are behind it) -- half the LDS, which is what
// lets every item-carrying workgroup of config 2 be resident at once (see the kernel).
constexpr int kFixItemSpan = 9 + 63, kFixItemElems = 9 * kFixItemSpan;            // 72 columns, 648 elements
constexpr int kFixItemRegs = (kFixItemElems + 63) / 64;                           // 11 per lane
constexpr int kFixItemLds = kFixTabRow + kFixItemElems;                           // floats per wavefront (2 928 bytes)

__device__ __forceinline__ void fixup_table_item(const float* __restrict__ in0, const float* __restrict__ row,
                                                 float* __restrict__ out, float* __restrict__ run_vals,
                                                 const float* __restrict__ best, unsigned long long* __restrict__ idx,
                                                 float rank_eps, unsigned* __restrict__ flags, WorkList work, float* sFv,
                                                 float* sS, int f, int h, int col, int d0, bool run_item, int H,
                                                 int W, int D, int lane, unsigned* stamp) {
  constexpr int bs = 9, half = 4, span = kFixItemSpan;
  const float n = 81.f;
  const long HW = (long)H * W;
  const int d = d0 + lane, w = col + d;
  const bool bad = d < D && w >= 0 && w < W;
  const long pix = ((long)f * H + h) * W + w;
  const float mb = (best && bad) ? best[pix] : 0.f;
  const bool won = best && bad && idx[pix] == (unsigned long long)d;             // the placeholder came out on top
  const float r0 = row[lane], r1 = row[64 + min(lane, kFixTabRow - 65)];
  const float* img = in0 + (long)f * HW;
  float t[kFixItemRegs];
#pragma unroll
  for (int k = 0; k < kFixItemRegs; ++k) {
    const int i = min(lane + 64 * k, kFixItemElems - 1);
    const int bh = i / span, cc = i - bh * span;
    t[k] = img[clampi(h + bh - half, 0, H - 1) * W + clampi(col - half + d0 + cc, 0, W - 1)];   // (int: as the grouped path's soff)
  }
  sFv[lane] = r0;
  if (lane < kFixTabRow - 64) sFv[64 + lane] = r1;
#pragma unroll
  for (int k = 0; k < kFixItemRegs; ++k)
    if (lane + 64 * k < kFixItemElems) sS[lane + 64 * k] = t[k] / n;
  CTD_POST_STAMP(stamp, 4);                                    // span staged
  float val = 0.f;
  if (__any(bad)) {
    const float s_f = sFv[81];
    const int o = min(lane, D - 1 - d0);                       // clamped: lanes past D read valid LDS, results unused
    // (three rows per trip: fully unrolled, the 81-tap loops need more than the kernel's 64 vector registers)
    float mu = 0.f;
#pragma unroll 3
    for (int bh = 0; bh < bs; ++bh) {
      const float* q = sS + bh * span + o;
#pragma unroll
      for (int bw = 0; bw < bs; ++bw) mu += q[bw];
    }
    CTD_POST_STAMP_V(stamp, 5, mu);                           // means done
#pragma unroll
    for (int k = 0; k < kFixItemRegs; ++k)
      if (lane + 64 * k < kFixItemElems) sS[lane + 64 * k] = t[k];
    float ss = 0.f, dot = 0.f;
#pragma unroll 3
    for (int bh = 0; bh < bs; ++bh) {
      const float* x = sS + bh * span + o;
      const float* vf = sFv + bh * bs;
#pragma unroll
      for (int bw = 0; bw < bs; ++bw) {
        const float v = x[bw] - mu;
        dot += vf[bw] * v;
        ss += v * v;
      }
    }
    val = 0.f + dot / ncc_norm(s_f, ss);                      // "T val = 0; val += dot / norm" (ext.h:142,186)
  }
  CTD_POST_STAMP_V(stamp, 6, val);                             // chains done
  if (run_item) {
    if (d < D) run_vals[((long)f * H + h) * D + d] = bad ? val : __int_as_float(0x7fc00000);
  } else if (bad) {
    if (out) out[((long)f * D + d) * HW + (long)h * W + w] = val;
  }
  if (best) {                                                  // wave-uniform: ranked call (see the grouped path)
    const bool clear = bad && val > mb + rank_margin(rank_eps, mb);
    if (clear) atomicMax(idx + pix, patch_key(val, d));
    const bool contender = bad && !clear && (won || !(val < mb - rank_margin(rank_eps, mb)));
    CTD_POST_STAMP(stamp, 7);                                  // best / idx compared
    worklist_push(contender && worklist_claim(flags, pix), pix, work);
  }
  CTD_POST_STAMP(stamp, 8);                                    // stores issued
}

// The fix-up kernel of a call on a prepared pattern (`tab`: the pattern's table).  Items come in two phases:
//   1. table items: item -> (jb = item / (frames x blocks), frame, block of 64 disparities), jb < fixup_table_rows(),
//      one wavefront each.  The list entry is indexed from the item number alone, so its load leaves together with the
//      counters' (reads past n_b stay inside the list's allocation, `list_b_cap` entries, and are discarded).
//   2. what has no table row -- listed frame windows and pattern windows past the cap -- through the generic path, by
//      the first wavefront of every workgroup on the whole workgroup's LDS, behind a workgroup barrier.
// Workgroup shape: 4 independent wavefronts with kFixItemLds floats each, 11 712 bytes a workgroup, at most 64 vector
// registers: 8 workgroups fit a CU (8 wavefronts per SIMD, the hardware's limit; LDS would hold 12), 2 048 on 256 CUs --
// the whole grid.  Config 2 lists 256 pattern windows: 256 x 16 x 2 = 8 192 items, one per wavefront of the grid, all
// resident in the first round.
__global__ __launch_bounds__(256, 8) void ncc_fixup_items_kernel(
    const float* __restrict__ in0, const float* __restrict__ in1, long in1_frame_stride, float* __restrict__ out,
    unsigned* __restrict__ counters, const unsigned long long* __restrict__ list_a,
    const unsigned long long* __restrict__ list_b, unsigned list_b_cap, const float* __restrict__ tab_end,
    float* __restrict__ run_vals, const float* __restrict__ best, unsigned long long* __restrict__ idx, float rank_eps,
    unsigned* __restrict__ flags, WorkList work, int frames, int H, int W, int D) {
  extern __shared__ float lds_fix[];
  // (the wavefront number as a scalar: item, list entry, frame and block are then scalars too, and the item's loads take
  // a scalar base and one 32-bit offset register each -- the kernel has 64 vector registers)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  unsigned* stamp = CTD_POST_STAMP_SLOT(0u);                    // entry
  float* sFv = lds_fix + wave * kFixItemLds;
  float* sS = sFv + kFixTabRow;
  const unsigned per_b = in1_frame_stride == 0 ? (unsigned)frames : 1u;   // a shared pattern window meets every frame
  const unsigned blocks = (unsigned)(D + 63) / 64u, per_win = per_b * blocks;
  const unsigned n_waves = gridDim.x * 4u;
  unsigned item = blockIdx.x * 4u + wave;
  unsigned jb = item / per_win;
  unsigned long long e = list_b[min(jb, list_b_cap - 1u)];
  const unsigned n_a = counters[0], n_b = counters[1];
  CTD_POST_STAMP_S(stamp, 1, n_b);                             // counters read
  // ranked calls: slot 3 for the tail kernel (see ncc_fixup_kernel)
  if (best && blockIdx.x == 0 && threadIdx.x == 0) counters[3] = n_a;
  const unsigned n_t = fixup_table_rows(n_b, list_b_cap);
  const unsigned n_items = n_t * per_win;                      // (the host passes a table only when this cannot overflow)
  while (item < n_items) {
    const int z = (int)(e >> 40), h = (int)((e >> 20) & 0xFFFFF), col = (int)(e & 0xFFFFF) - 0x80000;
    CTD_POST_STAMP_S(stamp, 2, col);                           // list entry read
    CTD_POST_STAMP_ITEM(stamp);
    const unsigned r = item - jb * per_win, fi = r / blocks, blk = r - fi * blocks;
    const int f = per_b == 1u ? z : (int)fi;                   // (single channel: z of a per-frame pattern is its frame)
    CTD_POST_STAMP(stamp, 3);                                  // pattern side ready (a table row: nothing to do)
    fixup_table_item(in0, tab_end - (size_t)(jb + 1) * kFixTabRow, out, run_vals, best, idx, rank_eps, flags, work, sFv, sS, f,
                     h, col, (int)blk * 64, col == -(9 - 1 - 4), H, W, D, lane, stamp);
    CTD_POST_STAMP(stamp, 9);                                  // exit of the wavefront's first item
    stamp = nullptr;
    item += n_waves;
    if (item >= n_items) break;
    jb = item / per_win;
    e = list_b[jb];
  }
  const unsigned n_rest = n_a + (n_b - n_t) * per_b;
  if (n_rest == 0) return;                                     // (uniform over the grid)
  __syncthreads();                                             // the workgroup's LDS now serves its first wavefront alone
  if (wave != 0) return;
  for (unsigned it = blockIdx.x; it < n_rest; it += gridDim.x) {
    const bool is_a = it < n_a;
    const unsigned k = is_a ? 0u : (it - n_a) / per_b;
    const unsigned long long e2 = is_a ? list_a[it] : list_b[n_t + k];
    const int z = (int)(e2 >> 40), h = (int)((e2 >> 20) & 0xFFFFF), col = (int)(e2 & 0xFFFFF) - 0x80000;
    const int f = (is_a || per_b == 1u) ? z : (int)((it - n_a) - k * per_b);
    fixup_generic_item<9>(in0, in1, in1_frame_stride, out, run_vals, best, idx, rank_eps, flags, work, lds_fix, is_a, f, h,
                          col, !is_a && col == -(9 - 1 - 4), 1, H, W, D, 9, lane);
  }
}

// Second half of the run items (ctd_tail.h: runs_role), as a kernel of its own for the unranked call; a ranked call runs
// the same role inside its tail kernel (argmax_rerank.hip).
__global__ __launch_bounds__(256) void ncc_fixup_runs_kernel(float* __restrict__ out, const float* __restrict__ run_vals,
                                                             const unsigned* __restrict__ counters,
                                                             const unsigned long long* __restrict__ run_rows, int per_frame,
                                                             int frames, int C, int H, int W, int D, int bs,
                                                             unsigned* __restrict__ rank_counter) {
  extern __shared__ int s_rows[];                          // up to C * H rows of this frame's pattern
  // the work-list counter of the ranking pass that may follow (argmax_rerank.hip) lives at the start of the
  // workspace, which the volume kernel is done with by now: cleared here instead of by a memset of its own
  if (rank_counter && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *rank_counter = 0u;
  runs_role(out, run_vals, counters, run_rows, per_frame, C, H, W, D, bs, (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y, s_rows);
}

// Fills the pattern-side table of a prepared pattern from its list of listed windows (after the pattern's pre-pass, same
// stream): one wavefront per listed window, grid-stride over the count the pre-pass left on the device.  Block 9, single
// channel; other calls have no table and nothing is launched.
CTD_POST_STAMP_EXPORT(ctd_debug_read_fixup_stamps)

int launch_fixup_table(const float* in1, long in1_frame_stride, int C, int H, int W, int bs, const FastWorkspace& ws,
                       hipStream_t stream) {
  if (!fixup_table_covers(C, bs)) return CTD_OK;
  hipLaunchKernelGGL(ncc_fixup_table_kernel, dim3(256), dim3(256), 0, stream, in1, in1_frame_stride, ws.counters, ws.flag_b,
                     ws.flag_b_cap, ws.fix_tab_end, H, W);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

int launch_fixup(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames, int C, int H,
                        int W, int D, int bs, const FastWorkspace& ws, bool per_frame, const float* tab, const RankPlan* rank,
                        const float* best, unsigned* scan_counter, hipStream_t stream) {
  // reference-order recomputation of the outputs of listed (ill-conditioned) windows; the grid drains
  // immediately when nothing was listed
  const size_t lds_wave = sizeof(float) * (3 * (size_t)bs * bs + 2 * (size_t)bs * (bs + D - 1));
  const float* rbest = rank ? best : nullptr;
  unsigned long long* ridx = rank ? (unsigned long long*)rank->idx : nullptr;
  const float reps = rank ? rank->eps : -1.f;
  unsigned* rflags = rank ? (unsigned*)rank->flags : nullptr;
  const WorkList rwork = rank ? rank->work : WorkList{};
  // prepared pattern: one-frame items on the table, as long as 32-bit item numbers hold every (window, frame, block)
  const long per_win = (long)(per_frame ? 1 : frames) * ceil_div(D, 64);
#ifdef CTD_FIXUP_NO_TABLE   // (diagnostic builds: the table-less kernel on a prepared pattern, for before / after timelines)
  tab = nullptr;
#endif
  if (tab && fixup_table_covers(C, bs) && (long)kFixTabCap * per_win < (1L << 31)) {
    size_t lds = sizeof(float) * 4 * (size_t)kFixItemLds;
    if (lds < lds_wave) lds = lds_wave;                        // (the generic items of a workgroup run on all of its LDS)
    if (lds > 160 * 1024) return CTD_ERR_UNSUPPORTED;
    if (lds > 64 * 1024)
      CTD_HIP_TRY(hipFuncSetAttribute((const void*)ncc_fixup_items_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(ncc_fixup_items_kernel, dim3(kFixupBlocks), dim3(256), lds, stream, in0, in1, in1_frame_stride, out,
                       ws.counters, ws.flag_a, ws.flag_b, ws.flag_b_cap, tab, ws.run_vals, rbest, ridx, reps, rflags, rwork,
                       frames, H, W, D);
  } else {
    const size_t lds = 4 * lds_wave;
    if (lds > 160 * 1024) return CTD_ERR_UNSUPPORTED;
    auto fix = bs == 9 ? ncc_fixup_kernel<9> : ncc_fixup_kernel<0>;
    if (lds > 64 * 1024)
      CTD_HIP_TRY(hipFuncSetAttribute((const void*)fix, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(fix, dim3(kFixupBlocks), dim3(256), lds, stream, in0, in1, in1_frame_stride, out, ws.counters,
                       ws.flag_a, ws.flag_b, ws.run_vals, rbest, ridx, reps, rflags, rwork, frames, C, H, W, D, bs);
  }
  CTD_LAUNCH_CHECK();
  if (!out || rank) return CTD_OK;                           // nothing to spread without a volume; ranked calls spread in their tail kernel
  const size_t lds_rows = sizeof(int) * (size_t)C * H;
  if (lds_rows > 64 * 1024) return CTD_ERR_UNSUPPORTED;
  // (the old scan's work-list counter sits at the start of the workspace, which the volume kernel is done with by
  // now: cleared by the runs kernel instead of by a memset of its own)
  hipLaunchKernelGGL(ncc_fixup_runs_kernel, dim3((unsigned)(frames * ceil_div(D, kRunPlanes)), 4), dim3(256), lds_rows, stream, out, ws.run_vals,
                     ws.counters, ws.run_rows, per_frame ? 1 : 0, frames, C, H, W, D, bs, scan_counter);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd
