// ctd_union_find.h -- the union-find with integer atomics that disp_filter.hip and mesh_clean.hip share.
//
// L[] holds indices; a parent is never larger than its child and a larger root is always hung under a smaller one (atomic
// min), so when all unions are done the root of a set is its smallest index, whatever order the atomics landed in.  Every
// traversal may read a stale parent: an older parent is still an ancestor in the same set, and the returning atomic min
// decides, so staleness costs iterations, never the result.
#pragma once

#include "ctd_common.h"

namespace ctd {
namespace {

template <int SCOPE>
__device__ inline int uf_find(int* L, int x) {                // path halving; every write is an atomic min
  for (;;) {
    const int p1 = __hip_atomic_load(L + x, __ATOMIC_RELAXED, SCOPE);
    if (p1 == x) return x;
    const int p2 = __hip_atomic_load(L + p1, __ATOMIC_RELAXED, SCOPE);
    if (p2 == p1) return p1;
    __hip_atomic_fetch_min(L + x, p2, __ATOMIC_RELAXED, SCOPE);
    x = p2;
  }
}

template <int SCOPE>
__device__ inline void uf_union(int* L, int a, int b) {
  for (;;) {
    a = uf_find<SCOPE>(L, a);
    b = uf_find<SCOPE>(L, b);
    if (a == b) return;
    if (a > b) { const int t = a; a = b; b = t; }
    const int old = __hip_atomic_fetch_min(L + b, a, __ATOMIC_RELAXED, SCOPE);
    if (old == b) return;                                     // b was a root: hung under a
    b = old;                                                  // b had a parent already: join a with that one
  }
}

constexpr int kWg = __HIP_MEMORY_SCOPE_WORKGROUP, kAgent = __HIP_MEMORY_SCOPE_AGENT;

// one integer atomic add of the run length on count[key] per run of equal keys inside the wavefront (key < 0: no add).
// Every lane of the wavefront must call it.
__device__ inline void uf_count_runs(int* count, long key) {
  const int lane = threadIdx.x & 63;
  const long prev = __shfl_up(key, 1);
  const bool head = lane == 0 || key != prev;
  const unsigned long long rest = (__ballot(head) >> lane) >> 1;
  if (head && key >= 0) atomicAdd(count + key, rest ? __ffsll(rest) : 64 - lane);
}

}  // namespace
}  // namespace ctd
