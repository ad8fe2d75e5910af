// ncc_fixup.hip -- fix-up pass of the fast NCC path: the outputs of the windows the pre-pass listed, recomputed in the
// reference's operation order (the stages of a call: ncc_fast.hip).
#include "ctd_ncc_fast.h"
#include "ctd_ncc_point.h"
#include "ctd_rank.h"
#include "ctd_tail.h"

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

template <int BS>
__device__ __forceinline__ void fixup_grouped_item(const float* __restrict__ in0, const float* __restrict__ in1,
                                                float* __restrict__ out, float* __restrict__ run_vals,
                                                const float* __restrict__ best, unsigned long long* __restrict__ idx,
                                                float rank_eps,
                                                unsigned* __restrict__ flags, WorkList work, float* sF, float* sFq,
                                                float* sFv,
                                                float* sS, float* sSq, int f_lo, int f_hi, int h, int col, bool run_item,
                                                int H, int W, int D, int bs_rt, int lane) {
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
  // FIX side: the pattern window, its mean (every tap divided before the sum, as the reference does) and deviations
  for (int i0 = lane; i0 < taps; i0 += 64 * 2) {
    float t[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = min(i0 + 64 * u, taps - 1);
      const int bh = i / bs, bw = i - bh * bs;
      t[u] = in1[(long)clampi(h + bh - half, 0, H - 1) * W + clampi(col + bw - half, 0, W - 1)];
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
    }
  }
  flush_candidates();
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
  const float n = (float)taps;
  // per-wave staging: FIX window raw / divided by n / minus its mean, SPAN rows raw / divided by n
  float* sF = lds_fix + (threadIdx.x >> 6) * (3 * taps + 2 * bs * span);
  float* sFq = sF + taps;
  float* sFv = sFq + taps;
  float* sS = sFv + taps;
  float* sSq = sS + bs * span;
  const long HW = (long)H * W;
  const unsigned n_a = counters[0], n_b = counters[1];
  // ranked calls: the tail kernel reads the number of listed frame windows from slot 3 and clears slot 0 for the next
  // call's pre-pass (which counts in it) -- no memset launch in front of a call on a prepared pattern
  if (best && blockIdx.x == 0 && threadIdx.x == 0) counters[3] = n_a;
  const unsigned per_b = in1_frame_stride == 0 ? (unsigned)frames : 1u;   // a shared pattern window meets every frame
  // single channel, shared pattern, SPAN small enough for the prefetch registers: kFixFrames frames per item
  const bool grouped = per_b > 1u && C == 1 && bs * span <= 64 * kFixSpanRegs;
  const unsigned groups = grouped ? (per_b + kFixFrames - 1) / kFixFrames : per_b;
  const unsigned n_items = n_a + n_b * groups;
  const unsigned n_waves = gridDim.x * (blockDim.x >> 6);
  const int rounds = (D + 63) / 64;
  for (unsigned item = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); item < n_items; item += n_waves) {
    const bool is_a = item < n_a;
    const unsigned jb = is_a ? 0u : (item - n_a) / groups;
    const unsigned long long e = is_a ? list_a[item] : list_b[jb];
    const int z = (int)(e >> 40), h = (int)((e >> 20) & 0xFFFFF), col = (int)(e & 0xFFFFF) - 0x80000;
    const bool run_item = !is_a && col == -(bs - 1 - half);
    if (grouped && !is_a) {
      const int f_lo = (int)((item - n_a) - jb * groups) * kFixFrames;
      fixup_grouped_item<BS>(in0, in1, out, run_vals, best, idx, rank_eps, flags, work, sF, sFq, sFv, sS, sSq,
                             f_lo, min(frames, f_lo + kFixFrames), h, col, run_item, H, W, D, bs, lane);
      continue;
    }
    const int f = (is_a || per_b == 1u) ? z / C : (int)((item - n_a) - jb * groups);
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

int launch_fixup(const float* in0, const float* in1, long in1_frame_stride, float* out, int frames, int C, int H,
                        int W, int D, int bs, const FastWorkspace& ws, bool per_frame, const RankPlan* rank, const float* best,
                        unsigned* scan_counter, hipStream_t stream) {
  // reference-order recomputation of the outputs of listed (ill-conditioned) windows; the grid drains
  // immediately when nothing was listed
  const size_t lds = sizeof(float) * 4 * (3 * (size_t)bs * bs + 2 * (size_t)bs * (bs + D - 1));
  if (lds > 160 * 1024) return CTD_ERR_UNSUPPORTED;
  auto fix = bs == 9 ? ncc_fixup_kernel<9> : ncc_fixup_kernel<0>;
  if (lds > 64 * 1024)
    CTD_HIP_TRY(hipFuncSetAttribute((const void*)fix, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fix, dim3(kFixupBlocks), dim3(256), lds, stream, in0, in1, in1_frame_stride, out, ws.counters,
                     ws.flag_a, ws.flag_b, ws.run_vals, rank ? best : nullptr, rank ? (unsigned long long*)rank->idx : nullptr,
                     rank ? rank->eps : -1.f,
                     rank ? (unsigned*)rank->flags : nullptr, rank ? rank->work : WorkList{}, frames, C, H, W, D, bs);
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
