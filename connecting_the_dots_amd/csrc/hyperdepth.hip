// hyperdepth.hip -- HyperDepth random-forest disparity evaluation: hyperdepth.h:253-287 `eval` of the reference
// (per row, per pixel: walk every tree of the row's forest over the 32 x 32 patch, sum the reached leaves' class
// histograms, take the two best classes).  The semantics and the device table layout are stated with the entry point
// in include/ctd_hip.h (ctd_hyperdepth_eval_f32); everything here is integer work except the three f32 outputs, which
// use the reference's operations in its order (the library builds with -ffp-contract=off).
//
// The reference builds a dense W * n_disp_bins histogram per tree and pixel (hyperdepth.h:82-96) and scans the sum
// twice.  Here the leaves are class-sorted sparse lists (class, count) and the histogram is one dense int array in LDS
// per workgroup that is touched only where the lists land:
//   - a workgroup is one wave and owns 64 consecutive pixels of one (image, row); lane = pixel for the walk;
//   - walk: each lane walks the T trees for its pixel (nodes from global memory, the patch gathers from the image
//     through L1 / L2) and stores the reached leaves' list offsets, lengths and sums in LDS;
//   - then per pixel p, all 64 lanes: pass 1 scatters the concatenated T lists into the histogram with integer LDS
//     atomics (exact, order-free); pass 2 reads each touched class back with atomicExch(.., 0), which also restores
//     the all-zero histogram for the next pixel.  Each touched class is read non-zero by exactly one lane;
//   - top-2 by the key (S << 32) | ~class: larger S first, then the smaller class.  A wave butterfly merges the lanes'
//     (best, second) pairs.  Cost per pixel O(sum of the T list lengths), never O(C).
//
// Why the key order is the reference's (argmax(), hyperdepth.h:99-117).  Its loop keeps (max_idx, max2_idx) and
// preserves the invariant: after index i, max_idx is the first index of the maximum of counts[0..i] and max2_idx the
// first index of the maximum of counts[0..i] without max_idx.  Initially (i = 0, max2 = -1 / count -1) it holds.
// Step i + 1 with value c: if c > max, i + 1 is the new first maximum, and the old max_idx -- the first index holding
// the old maximum, which bounds every other value -- is the first maximum of the rest; else max_idx stays, and
// max2_idx moves to i + 1 only if c > max2 strictly (c == max, c > max2 included: then c is the maximum of the rest),
// so max2_idx stays the FIRST index of the rest's maximum.  So pos / pos2 are the first indices of the maximum of S
// over [0, C) and over [0, C) without pos: exactly the first two keys above when at least two classes are non-zero.
// With counts >= 0 a zero class never beats a non-zero one, so with one non-zero class pos2 is the first zero class
// (0, or 1 when pos == 0), and with none pos = 0, pos2 = 1 (C >= 2, checked at the boundary).
#include "ctd_common.h"

namespace ctd {

constexpr int kHdPix = 64;          // pixels per workgroup = its one wave's lanes
constexpr int kHdCache = 8;         // list entries per lane kept in registers from pass 1 to pass 2
constexpr int kHdOffClamp = 1 << 28;  // split offsets are clamped to this first (no int overflow; H, W < 2^24)

__device__ inline int hd_clamp_off(int v) { return min(max(v, -kHdOffClamp), kHdOffClamp); }

// entry j of pixel p's concatenated lists: tree t, list offset s_beg + (j - base); (t, base, end) only move forward
__device__ __forceinline__ long long hd_locate(int j, int& t, int& base, int& end, const int* s_len,
                                               const long long* s_beg, int p) {
  while (j >= end) {
    base = end;
    ++t;
    end += s_len[t * kHdPix + p];
  }
  return s_beg[t * kHdPix + p] + (j - base);
}

// pass 2: the class's total, read and cleared at once; keeps this lane's best and second key
__device__ __forceinline__ void hd_take(int2 e, int C, int* hist, unsigned long long& k1, unsigned long long& k2) {
  if ((unsigned)e.x < (unsigned)C) {
    const int s = atomicExch(&hist[e.x], 0);
    if (s > 0) {                                  // a zero class is settled by the zero rules
      const unsigned long long key = ((unsigned long long)(unsigned)s << 32) | (unsigned)~e.x;
      const unsigned long long lo = key > k1 ? k1 : key;   // selects, not branches: no pair in scratch
      k1 = key > k1 ? key : k1;
      k2 = lo > k2 ? lo : k2;
    }
  }
}

__global__ __launch_bounds__(kHdPix) void hd_eval_kernel(const ctd_hd_tables tab, const uint8_t* __restrict__ ims,
                                                         int N, int H, int W, int row_from, int row_to, int nb,
                                                         float* __restrict__ out, int chunks, long total, long per_xcd) {
  // Blocks b and b + 8 share an XCD: each XCD gets a contiguous run of the (row, image, chunk) work items, so one
  // row's tables are read through one L2.  A speed matter only.
  const long b = blockIdx.x;
  const long work = (b & 7) * per_xcd + (b >> 3);
  if (work >= total) return;
  const int lane = threadIdx.x;
  const int chunk = (int)(work % chunks);
  const long rest = work / chunks;
  const int n = (int)(rest % N);
  const int row = (int)(rest / N);
  const int col = chunk * kHdPix + lane;
  const bool valid = col < W;
  float* o = out + (((long)n * H + row) * W + col) * 3;
  if (row < row_from || row >= row_to) {
    if (valid) o[0] = o[1] = o[2] = __builtin_nanf("");
    return;
  }

  const int T = tab.n_trees, C = tab.n_classes;
  extern __shared__ long long hd_lds[];
  long long* s_beg = hd_lds;                    // [T][64] list offset of the leaf tree t reached for pixel p
  int* s_len = (int*)(s_beg + T * kHdPix);      // [T][64] its length, -1 = malformed tables (pixel -> NaN)
  int* s_sum = s_len + T * kHdPix;              // [T][64] its count sum
  int* hist = s_sum + T * kHdPix;               // [C]
  for (int c = lane; c < C; c += kHdPix) hist[c] = 0;

  // ---- walk: lane = pixel ----
  const uint8_t* im = ims + (long)n * H * W;
  const int* roots = tab.roots + (long)(row - tab.row0) * T;
  const int4* nodes = (const int4*)tab.nodes;
  for (int t = 0; t < T; ++t) {
    long long beg = 0;
    int len = 0, sum = 0;
    if (valid) {
      int v = roots[t];
      int steps = 0;
      while (v >= 0 && v < tab.n_nodes && steps < tab.max_depth) {
        const int4 a = nodes[2 * (long)v];        // threshold bits, h0, w0, h1
        const int4 c = nodes[2 * (long)v + 1];    // w1, left, right, 0
        const int r0 = clampi(row + hd_clamp_off(a.y) - 16, 0, H - 1);
        const int c0 = clampi(col + hd_clamp_off(a.z) - 16, 0, W - 1);
        const int r1 = clampi(row + hd_clamp_off(a.w) - 16, 0, H - 1);
        const int c1 = clampi(col + hd_clamp_off(c.x) - 16, 0, W - 1);
        const float d = (float)im[(long)r0 * W + c0] - (float)im[(long)r1 * W + c1];
        v = d < __int_as_float(a.x) ? c.y : c.z;  // RawSample::at / Split: left iff d < threshold (NaN: right)
        ++steps;
      }
      len = -1;
      if (v < 0 && (long long)~v < tab.n_leaves) {
        const long long leaf = ~v;
        const long long e0 = tab.leaf_off[leaf], e1 = tab.leaf_off[leaf + 1];
        if (e0 >= 0 && e0 <= e1 && e1 <= tab.n_entries && e1 - e0 <= C) {
          beg = e0;
          len = (int)(e1 - e0);
          sum = tab.leaf_sum[leaf];
        }
      }
    }
    s_beg[t * kHdPix + lane] = beg;
    s_len[t * kHdPix + lane] = len;
    s_sum[t * kHdPix + lane] = sum;
  }
  __syncthreads();

  // ---- per pixel: all lanes merge its T lists ----
  const int2* ent = (const int2*)tab.entries;
  const int npix = min(kHdPix, W - chunk * kHdPix);
  float res0 = __builtin_nanf(""), res1 = res0, res2 = res0;
  for (int p = 0; p < npix; ++p) {
    int total = 0, sum = 0;
    bool bad = false;
    for (int t = 0; t < T; ++t) {                 // wave-uniform (LDS broadcast)
      const int l = s_len[t * kHdPix + p];
      bad |= l < 0;
      total += l;
      sum += s_sum[t * kHdPix + p];
    }
    if (bad) continue;                            // malformed tables: this pixel stays NaN

    int t = 0, base = 0, end = s_len[p];
    int2 cache[kHdCache];
#pragma unroll
    for (int k = 0; k < kHdCache; ++k) {
      const int j = k * kHdPix + lane;
      if (j < total) cache[k] = ent[hd_locate(j, t, base, end, s_len, s_beg, p)];
    }
    const int t_tail = t, base_tail = base, end_tail = end;
#pragma unroll
    for (int k = 0; k < kHdCache; ++k) {
      const int j = k * kHdPix + lane;
      if (j < total && (unsigned)cache[k].x < (unsigned)C) atomicAdd(&hist[cache[k].x], cache[k].y);
    }
    for (int j = kHdCache * kHdPix + lane; j < total; j += kHdPix) {
      const int2 e = ent[hd_locate(j, t, base, end, s_len, s_beg, p)];
      if ((unsigned)e.x < (unsigned)C) atomicAdd(&hist[e.x], e.y);
    }
    __syncthreads();

    unsigned long long k1 = 0, k2 = 0;            // best and second key of this lane, 0 = none
#pragma unroll
    for (int k = 0; k < kHdCache; ++k)
      if (k * kHdPix + lane < total) hd_take(cache[k], C, hist, k1, k2);
    t = t_tail;
    base = base_tail;
    end = end_tail;
    for (int j = kHdCache * kHdPix + lane; j < total; j += kHdPix)
      hd_take(ent[hd_locate(j, t, base, end, s_len, s_beg, p)], C, hist, k1, k2);

    // keys are distinct across lanes (one lane per class reads it non-zero): merge (best, second) pairs
#pragma unroll
    for (int m = kHdPix / 2; m >= 1; m >>= 1) {
      const unsigned long long o1 = __shfl_xor(k1, m), o2 = __shfl_xor(k2, m);
      const unsigned long long lo = k1 > o1 ? o1 : k1, sec = k1 > o1 ? k2 : o2;
      k1 = k1 > o1 ? k1 : o1;
      k2 = lo > sec ? lo : sec;
    }
    int pos = 0, pos2 = 1;
    if (k1) {
      pos = (int)~(unsigned)k1;
      pos2 = k2 ? (int)~(unsigned)k2 : (pos == 0 ? 1 : 0);
    }
    if (lane == p) {
      const float fc = (float)col;
      const float d = fc - (float)pos / (float)nb;
      const float d2 = fc - (float)pos2 / (float)nb;
      res0 = d;
      res1 = (float)(int)(k1 >> 32) / (float)sum;
      res2 = fabsf(d - d2);
    }
    __syncthreads();                              // pass 2's clears land before the next pixel's adds
  }
  if (valid) {
    o[0] = res0;
    o[1] = res1;
    o[2] = res2;
  }
}

static size_t hyperdepth_lds_bytes(int n_trees, int n_classes) {
  return (size_t)n_trees * kHdPix * 16 + (size_t)n_classes * 4;
}

static long hyperdepth_grid(int N, int H, int W) {
  const long total = (long)H * N * ceil_div(W, kHdPix);
  return (total + 7) / 8 * 8;
}

static int hyperdepth_eval_f32(const ctd_hd_tables& tab, const uint8_t* ims, int N, int H, int W, int row_from,
                               int row_to, int n_disp_bins, float* out, hipStream_t stream) {
  const int chunks = ceil_div(W, kHdPix);
  const long total = (long)H * N * chunks;
  const long per_xcd = (total + 7) / 8;
  hipLaunchKernelGGL(hd_eval_kernel, dim3((unsigned)(per_xcd * 8)), dim3(kHdPix),
                     hyperdepth_lds_bytes(tab.n_trees, tab.n_classes), stream, tab, ims, N, H, W, row_from, row_to,
                     n_disp_bins, out, chunks, total, per_xcd);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_hyperdepth_eval_f32(const ctd_hd_tables* tables, const uint8_t* ims, int N, int H, int W, int row_from,
                            int row_to, int n_disp_bins, float* out, int device, void* stream) {
  if (!tables) return CTD_ERR_INVALID_ARG;
  const ctd_hd_tables t = *tables;
  if (N < 0 || H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24)) return CTD_ERR_INVALID_ARG;
  if (row_from < 0 || row_from > row_to || row_to > H) return CTD_ERR_INVALID_ARG;
  if (t.n_trees < 1 || t.n_trees > 16 || t.n_classes < 2 || n_disp_bins < 1 || t.n_nodes < 0 || t.n_leaves < 0 ||
      t.n_entries < 0 || t.max_depth < 0 || t.n_rows < 0)
    return CTD_ERR_INVALID_ARG;
  if (row_from < row_to && (row_from < t.row0 || (long)row_to > (long)t.row0 + t.n_rows)) return CTD_ERR_INVALID_ARG;
  if (!ims || !out || !t.roots || !t.leaf_off || !t.leaf_sum || (t.n_nodes > 0 && !t.nodes) ||
      (t.n_entries > 0 && !t.entries))
    return CTD_ERR_INVALID_ARG;
  // the kernel reads nodes as int4 pairs, entries as int2, offsets as int64
  if ((uintptr_t)t.nodes % 16 || (uintptr_t)t.entries % 8 || (uintptr_t)t.leaf_off % 8 || (uintptr_t)t.roots % 4 ||
      (uintptr_t)t.leaf_sum % 4 || (uintptr_t)out % 4)
    return CTD_ERR_INVALID_ARG;
  if (hyperdepth_lds_bytes(t.n_trees, t.n_classes) > 65536) return CTD_ERR_UNSUPPORTED;
  if (hyperdepth_grid(N, H, W) > 2147483647L) return CTD_ERR_UNSUPPORTED;
  if (N == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return hyperdepth_eval_f32(t, ims, N, H, W, row_from, row_to, n_disp_bins, out, (hipStream_t)stream);
}

}  // extern "C"
