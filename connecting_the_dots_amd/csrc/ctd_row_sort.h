// ctd_row_sort.h -- the two row sorts of mesh_smooth.hip and mesh_simplify.hip, stated once: rows whose entries were
// placed by integer atomics are sorted ascending, which removes the order the atomics left.  A short row by one lane
// over a copy in LDS, a long row by the workgroup over the row in global memory, whatever its length.
#pragma once

#include "ctd_compact.h"

namespace ctd {
namespace {

// one lane: r entries `kChunk` apart in LDS, ascending
__device__ inline void lane_sort(int* col, int r) {
  for (int k = 1; k < r; ++k) {
    const int v = col[k * kChunk];
    int j = k;
    for (; j > 0 && col[(j - 1) * kChunk] > v; --j) col[j * kChunk] = col[(j - 1) * kChunk];
    col[j * kChunk] = v;
  }
}

// the workgroup: a[0 .. n) in global memory, ascending.  Merges of size k = 2, 4, ...: first the comparators (i, its mirror
// in the block of k), then distances k/4 .. 1; the smaller value always goes to the smaller index, so values past the end
// (+infinity in thought) never move and comparators that reach them are skipped.  Ends with a barrier.
__device__ inline void wg_sort(int* a, int n) {
  for (long k = 2; (k >> 1) < n; k <<= 1) {
    const long h = k >> 1, pairs = (n + k - 1) / k * h;        // h comparators in every block of k that starts inside the row
    for (long t = threadIdx.x; t < pairs; t += kChunk) {
      const long base = (t / h) * k, off = t % h, i = base + off, p = base + k - 1 - off;
      if (p < n) {
        const int x = a[i], y = a[p];
        if (x > y) { a[i] = y; a[p] = x; }
      }
    }
    __syncthreads();
    for (long j = h >> 1; j >= 1; j >>= 1) {
      const long pairs_j = (n + 2 * j - 1) / (2 * j) * j;
      for (long t = threadIdx.x; t < pairs_j; t += kChunk) {
        const long i = (t / j) * 2 * j + t % j, p = i + j;
        if (p < n) {
          const int x = a[i], y = a[p];
          if (x > y) { a[i] = y; a[p] = x; }
        }
      }
      __syncthreads();
    }
  }
}

}  // namespace
}  // namespace ctd
