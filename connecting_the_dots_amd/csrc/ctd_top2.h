// ctd_top2.h -- best / runner-up of a set of block costs, the reduction of the volume-free cost argmin
// (ctd_costvol_argmin_f32): the ranking instantiations of the cost-volume kernels (costvol_fast.hip) and the
// combine pass (costvol_argmin.hip).
//
// Top2 {b1, i1, b2} of a set S of (cost, d): b1 = min cost, i1 = the LOWEST d with that cost, b2 = min cost over S
// without the element (b1, i1) (so b2 == b1 when the minimum is tied).  The merge below is associative and
// commutative, and "lower d wins" at every step, so any merge tree gives the first-index argmin of the union.
// Costs are non-negative: f32 compares are value compares; the empty set is {+inf, INT_MAX, +inf}.
#pragma once
#include <climits>

#include "ctd_common.h"

namespace ctd {

struct Top2 {
  float b1;
  int i1;
  float b2;
};

constexpr int kRankChunk = 128;       // disparities per workspace triple

__device__ inline Top2 top2_empty() { return Top2{__builtin_inff(), INT_MAX, __builtin_inff()}; }

// add (v, d) with d greater than every index already in `a` (an ascending scan): strict <, so ties keep the first
__device__ inline void top2_push(Top2& a, float v, int d) {
  if (v < a.b1) {
    a.b2 = a.b1;
    a.b1 = v;
    a.i1 = d;
  } else {
    a.b2 = fminf(a.b2, v);
  }
}

__device__ inline Top2 top2_merge(const Top2& a, const Top2& b) {
  const bool bw = b.b1 < a.b1 || (b.b1 == a.b1 && b.i1 < a.i1);
  const Top2& w = bw ? b : a;
  const Top2& l = bw ? a : b;
  return Top2{w.b1, w.i1, fminf(w.b2, l.b1)};
}

// planar workspace triples [frames][n_chunks][H][W], chunk c = disparities [c * kRankChunk, (c + 1) * kRankChunk)
struct Top2Planes {
  float* b1;
  int* i1;
  float* b2;
};

__device__ inline void top2_store(const Top2Planes& p, long i, const Top2& t) {
  p.b1[i] = t.b1;
  p.i1[i] = t.i1;
  p.b2[i] = t.b2;
}

}  // namespace ctd
