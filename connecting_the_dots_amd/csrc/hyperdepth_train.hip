// hyperdepth_train.hip -- HyperDepth random-forest training: the reference's per-row forest trainer
// (hyperdepth.h `train`, rf/train.h TrainForestQueued) with its randomness defined by a counter-based generator, so
// that the result is an exact function of (ims, disps, params, seed).  The contract is stated with the entry point in
// include/ctd_hip.h (ctd_hyperdepth_train_f32); tests/hyperdepth_train_ref.py restates it in numpy.
//
// Training goes level by level over every (row, tree) of the call at once.  Each tree owns a region of T * S sample
// slots (S = valid samples of all rows); a node is a segment [seg, seg + n) of its tree's region, and a split
// partitions its segment in place (stably, into the other of two ping-pong buffers), so that the segments of a tree's
// leaves are disjoint.  Per level, over the frontier (device-resident list, count in device memory, grid-stride):
//   1. subset:   nodes that try to split draw their subset (Floyd, one lane, bitmap in LDS or, for nodes beyond
//                2^19 samples, in the workspace), compact it in position order, sort it by cost class (bitonic, LDS)
//                and store the sorted gather coordinates and the class run ends;
//   2. cand:     per node, for every split function: its k' features once into LDS, then the thresholds kTJ at a
//                time, each lane counting the left samples of its class runs; nodes with k' <= 64 take one wave
//                each instead (hdt_cand_small_kernel: a ballot per threshold).  The int64 table-X cost is exact, so
//                the lexicographic (cost, f, j) minimum does not depend on the summation order;
//   3. part_leaf: split nodes partition their full segment (count, then a stable ballot scan); leaf nodes build
//                their sparse class-sorted (class, count) list into a scratch slot at their own segment offset;
//   4. plan:     one workgroup assigns split / leaf / entry indices in frontier order (deterministic), writes the
//                ctd_hd_tables records, links every node into its parent and emits the next frontier.
// A final pass moves the leaf lists from their scratch slots to the packed entries.  Nothing returns to the host.
#include "ctd_common.h"

namespace ctd {

constexpr int kTB = 256;                     // threads of every training workgroup
constexpr int kTWv = kTB / 64;               // its waves
constexpr int kTJ = 8;                       // thresholds counted per pass over the runs
constexpr int kTBitmapLds = 1 << 19;         // Floyd bitmap in LDS up to this many node samples (64 KiB)
constexpr int kTHistChunk = 8192;            // leaf histogram classes per pass (32 KiB)
constexpr int kTGrid = 4096;                 // grid-stride workgroups per level kernel, at most
constexpr size_t kTSubsetLds = 65536;

struct HdtFront {                            // one frontier node
  long long seg;                             // first slot of its segment (tree region included)
  long long link;                            // >= 0: nodes[] slot (parent split's left / right); < 0: roots[~link]
  int rt, heap, n, pad;                      // (row - row_from) * T + tree, heap id, samples
};

struct HdtRes {                              // per frontier node, written by the level's kernels
  int split;                                 // 1 = split (cand), 0 = leaf
  int nL;                                    // left samples of the full segment (part_leaf)
  int nruns;                                 // class runs of the sorted subset (subset)
  int elen;                                  // leaf list length (part_leaf)
  float thr;
  int h0, w0, h1, w1, pad;
};

struct HdtCtx {
  const uint8_t* ims;
  const float* disps;
  const long long* X;
  int N, H, W, row_from, R, T, nb, dsw, C, F, J, nts, msplit, mleaf, D, kmax;
  unsigned long long seed;
  long long S, TS, Fcap;
  long long* counts;                         // [R]
  long long* row_off;                        // [R + 1]
  int2* spx;                                 // [S] {n * H * W, col}
  int* scl;                                  // [S] fine class
  int* buf[2];                               // [TS] sample ids (row-local), ping-pong
  int* sub;                                  // [TS] subset, position order
  int2* sg;                                  // [TS] subset gather coordinates, class order
  int* runs;                                 // [TS] run ends of the sorted subset
  int2* etmp;                                // [TS] leaf lists at their segment offsets
  unsigned* bm;                              // [TS / 32 + Fcap + 1] Floyd bitmaps of large nodes
  HdtFront* fr[2];                           // [Fcap]
  HdtRes* res;                               // [Fcap]
  long long* ltmp;                           // [cap_leaves] scratch offset of each leaf's list
  int* llen;                                 // [cap_leaves]
  long long* ctr;                            // [8] splits, leaves, entries, max depth, frontier counts [4], [5], error
  ctd_hd_train_out out;
};

// ---- randomness (the contract's mix64 / draw) ----
__host__ __device__ inline unsigned long long hdt_mix64(unsigned long long x) {
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}
__device__ inline unsigned long long hdt_base(unsigned long long seed, int row, int tree, int node) {
  return hdt_mix64(hdt_mix64(hdt_mix64(hdt_mix64(seed) ^ (unsigned long long)(long long)row) ^
                             (unsigned long long)(long long)tree) ^ (unsigned long long)(long long)node);
}
__device__ inline unsigned hdt_draw(unsigned long long base, unsigned long long slot, unsigned long long m) {
  return (unsigned)(((hdt_mix64(base ^ slot) >> 32) * m) >> 32);
}

// the sample rule: valid iff d >= 0 and 0 <= trunc(((float)col - d) * nb) < C (f32, no contraction)
__device__ inline bool hdt_sample(float d, int col, int nb, int C, int& cl) {
  const float p = ((float)col - d) * (float)nb;
  if (!(d >= 0.f) || !(p > -1.f) || !(p < 2147483648.f)) return false;
  cl = (int)p;
  return cl < C;
}

// v(h0, w0) - v(h1, w1) of the sample at {n * H * W, col} in image row `row`
__device__ inline float hdt_feat(const uint8_t* ims, int2 s, int row, int H, int W, int h0, int w0, int h1, int w1) {
  const uint8_t* im = ims + s.x;
  const int r0 = clampi(row + h0 - 16, 0, H - 1), c0 = clampi(s.y + w0 - 16, 0, W - 1);
  const int r1 = clampi(row + h1 - 16, 0, H - 1), c1 = clampi(s.y + w1 - 16, 0, W - 1);
  return (float)im[r0 * W + c0] - (float)im[r1 * W + c1];
}

// exclusive prefix of a flag over the workgroup; `total` = number of set flags
__device__ inline int hdt_flag_scan(bool f, int& total, int* s_w) {
  const unsigned long long m = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) s_w[w] = __popcll(m);
  __syncthreads();
  int base = 0;
  total = 0;
  for (int i = 0; i < kTWv; ++i) {
    const int v = s_w[i];
    base += i < w ? v : 0;
    total += v;
  }
  __syncthreads();
  return base + pre;
}

// exclusive prefix of an int64 over the workgroup
__device__ inline long long hdt_scan(long long v, long long& total, long long* s_w) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  long long x = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const long long y = __shfl_up(x, o);
    if (lane >= o) x += y;
  }
  if (lane == 63) s_w[w] = x;
  __syncthreads();
  long long base = 0;
  total = 0;
  for (int i = 0; i < kTWv; ++i) {
    const long long t = s_w[i];
    base += i < w ? t : 0;
    total += t;
  }
  __syncthreads();
  return base + x - v;
}

__device__ inline long long hdt_sum(long long v, long long* s_w) {
  long long t;
  (void)hdt_scan(v, t, s_w);
  return t;
}

__device__ inline bool hdt_tries(const HdtCtx& c, const HdtFront& f, int depth) {
  return depth < c.D && f.n > c.msplit;
}

// ---- setup ----
__global__ __launch_bounds__(kTB) void hdt_count_kernel(const float* __restrict__ disps, int N, int H, int W,
                                                        int row_from, int nb, int C, long long* counts) {
  __shared__ long long s_w[kTWv];
  const int row = row_from + blockIdx.x;
  long long cnt = 0;
  for (long long i = threadIdx.x; i < (long long)N * W; i += kTB) {
    const int n = (int)(i / W), col = (int)(i % W);
    int cl;
    cnt += hdt_sample(disps[((long long)n * H + row) * W + col], col, nb, C, cl);
  }
  const long long t = hdt_sum(cnt, s_w);
  if (threadIdx.x == 0) counts[blockIdx.x] = t;
}

// row offsets, the first frontier (every tree's root) and the counters; refuses (error flag, empty frontier) when the
// device counts exceed the sample total the workspace was sized for
__global__ __launch_bounds__(kTB) void hdt_setup_kernel(HdtCtx c) {
  __shared__ int s_ok;
  if (threadIdx.x == 0) {
    long long s = 0;
    for (int r = 0; r < c.R; ++r) {
      c.row_off[r] = s;
      s += c.counts[r];
    }
    c.row_off[c.R] = s;
    s_ok = s <= c.S;
    for (int i = 0; i < 8; ++i) c.ctr[i] = 0;
    c.ctr[4] = s_ok ? (long long)c.R * c.T : 0;
    c.ctr[6] = !s_ok;
  }
  __syncthreads();
  if (!s_ok) return;
  for (int rt = threadIdx.x; rt < c.R * c.T; rt += kTB) {
    const int r = rt / c.T, t = rt % c.T;
    HdtFront f;
    f.seg = c.T * c.row_off[r] + t * c.counts[r];
    f.link = ~(long long)rt;
    f.rt = rt;
    f.heap = 1;
    f.n = (int)c.counts[r];
    f.pad = 0;
    c.fr[0][rt] = f;
  }
}

// per row: the valid samples in (n, col) order, and every tree's identity permutation
__global__ __launch_bounds__(kTB) void hdt_extract_kernel(HdtCtx c) {
  __shared__ int s_w[kTWv];
  if (c.ctr[6]) return;
  const int r = blockIdx.x, row = c.row_from + r;
  const long long o = c.row_off[r], n_r = c.counts[r];
  long long base = 0;
  for (long long i0 = 0; i0 < (long long)c.N * c.W; i0 += kTB) {
    const long long i = i0 + threadIdx.x;
    int cl = 0, n = 0, col = 0;
    bool v = false;
    if (i < (long long)c.N * c.W) {
      n = (int)(i / c.W);
      col = (int)(i % c.W);
      v = hdt_sample(c.disps[((long long)n * c.H + row) * c.W + col], col, c.nb, c.C, cl);
    }
    int tot;
    const int pre = hdt_flag_scan(v, tot, s_w);
    if (v && base + pre < n_r) {
      c.spx[o + base + pre] = make_int2(n * c.H * c.W, col);
      c.scl[o + base + pre] = cl;
    }
    base += tot;
  }
  for (int t = 0; t < c.T; ++t) {
    int* b = c.buf[0] + c.T * o + t * n_r;
    for (long long i = threadIdx.x; i < n_r; i += kTB) b[i] = (int)i;
  }
}

// ---- 1. subset: Floyd, compaction, class sort ----
__global__ __launch_bounds__(kTB) void hdt_subset_kernel(HdtCtx c, int cur, int depth) {
  extern __shared__ unsigned long long hdt_lds64[];      // 64 KiB: the bitmap, then the sort keys
  __shared__ long long s_wl[kTWv];
  __shared__ int s_wi[kTWv];
  const long long nf = c.ctr[4 + cur];
  const HdtFront* fr = c.fr[cur];
  const int* src = c.buf[depth & 1];
  const int tid = threadIdx.x;
  for (long long i = blockIdx.x; i < nf; i += gridDim.x) {
    const HdtFront f = fr[i];
    if (!hdt_tries(c, f, depth)) continue;                // uniform over the workgroup
    const int n = f.n, kp = min(c.nts, n);
    const int r = f.rt / c.T, t = f.rt % c.T;
    const unsigned long long base = hdt_base(c.seed, c.row_from + r, t, f.heap);
    const int* s = src + f.seg;
    int* sub = c.sub + f.seg;
    if (n <= c.nts) {
      for (int j = tid; j < n; j += kTB) sub[j] = s[j];
    } else {
      const int words = (n + 31) >> 5;
      unsigned* bm = n <= kTBitmapLds ? (unsigned*)hdt_lds64 : c.bm + (f.seg >> 5) + i;
      for (int w = tid; w < words; w += kTB) bm[w] = 0u;
      __syncthreads();
      if (tid == 0) {                                     // Floyd: the draws are one serial sequence
        for (int q = 0; q < kp; ++q) {
          const unsigned jj = (unsigned)(n - kp + q);
          unsigned tt = hdt_draw(base, (unsigned long long)q, (unsigned long long)jj + 1ull);
          if (bm[tt >> 5] & (1u << (tt & 31))) tt = jj;
          bm[tt >> 5] |= 1u << (tt & 31);
        }
      }
      __syncthreads();
      long long ob = 0;
      for (int w0 = 0; w0 < words; w0 += kTB) {           // chosen positions in increasing order
        const int w = w0 + tid;
        unsigned m = w < words ? bm[w] : 0u;
        long long tot;
        long long o = ob + hdt_scan(__popc(m), tot, s_wl);
        while (m) {
          const int b = __ffs(m) - 1;
          m &= m - 1u;
          sub[o++] = s[(long long)w * 32 + b];
        }
        ob += tot;
      }
    }
    __syncthreads();
    int P = 1;
    while (P < kp) P <<= 1;
    const long long rb = c.row_off[r];
    for (int j = tid; j < P; j += kTB) {
      unsigned long long key = ~0ull;
      if (j < kp) {
        int cl = c.scl[rb + sub[j]];
        if (depth < c.dsw) cl /= c.nb;
        key = ((unsigned long long)(unsigned)cl << 32) | (unsigned)j;
      }
      hdt_lds64[j] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1) {
      for (int jm = k >> 1; jm > 0; jm >>= 1) {
        for (int x = tid; x < P; x += kTB) {
          const int y = x ^ jm;
          if (y > x) {
            const unsigned long long a = hdt_lds64[x], b = hdt_lds64[y];
            if ((a > b) == ((x & k) == 0)) {
              hdt_lds64[x] = b;
              hdt_lds64[y] = a;
            }
          }
        }
        __syncthreads();
      }
    }
    int runbase = 0;
    for (int j0 = 0; j0 < kp; j0 += kTB) {
      const int j = j0 + tid;
      bool end = false;
      if (j < kp) {
        const unsigned long long key = hdt_lds64[j];
        c.sg[f.seg + j] = c.spx[rb + sub[(unsigned)key]];
        end = j == kp - 1 || (hdt_lds64[j + 1] >> 32) != (key >> 32);
      }
      int tot;
      const int pre = hdt_flag_scan(end, tot, s_wi);
      if (end) c.runs[f.seg + runbase + pre] = j + 1;
      runbase += tot;
    }
    if (tid == 0) c.res[i].nruns = runbase;
    __syncthreads();                                      // the keys are rewritten by the next node
  }
}

// ---- 2. candidates ----
// subsets of at most one wave's lanes go to hdt_cand_small_kernel, the rest to hdt_cand_kernel
__device__ inline bool hdt_small(const HdtCtx& c, const HdtFront& f, int depth) {
  return hdt_tries(c, f, depth) && min(c.nts, f.n) <= 64;
}

// one wave per node, lane = subset element in class order: a threshold's left set is one ballot, and the left count
// of the class run a lane owns is the popcount of that ballot under the run's bit mask
__global__ __launch_bounds__(kTB) void hdt_cand_small_kernel(HdtCtx c, int cur, int depth) {
  const long long nf = c.ctr[4 + cur];
  const HdtFront* fr = c.fr[cur];
  const int lane = threadIdx.x & 63;
  for (long long i = (long long)blockIdx.x * kTWv + (threadIdx.x >> 6); i < nf; i += (long long)gridDim.x * kTWv) {
    const HdtFront f = fr[i];
    if (!hdt_small(c, f, depth)) continue;                // wave-uniform
    const int kp = min(c.nts, f.n);
    const int r = f.rt / c.T, t = f.rt % c.T, row = c.row_from + r;
    const unsigned long long base = hdt_base(c.seed, row, t, f.heap);
    const int nruns = c.res[i].nruns;
    const long long rb = c.row_off[r];
    int b = 0, e = 0;
    if (lane < nruns) {
      e = c.runs[f.seg + lane];
      b = lane ? c.runs[f.seg + lane - 1] : 0;
    }
    const int len = e - b;
    const unsigned long long rmask = lane < nruns ? (len == 64 ? ~0ull : ((1ull << len) - 1ull)) << b : 0ull;
    const int2 me = lane < kp ? c.sg[f.seg + lane] : make_int2(0, 0);
    long long best = 0x7fffffffffffffffll;
    int bf = -1, bj = -1;
    for (int fi = 0; fi < c.F; ++fi) {
      const unsigned long long fs = (1ull << 40) + 8ull * (unsigned long long)fi;
      const int h0 = hdt_draw(base, fs, 32), w0 = hdt_draw(base, fs + 1, 32);
      const int h1 = hdt_draw(base, fs + 2, 32), w1 = hdt_draw(base, fs + 3, 32);
      const float v = lane < kp ? hdt_feat(c.ims, me, row, c.H, c.W, h0, w0, h1, w1) : 0.f;
      for (int j0 = 0; j0 < c.J; j0 += 64) {
        float thr_l = 0.f;
        if (j0 + lane < c.J) {
          const unsigned long long js = (1ull << 41) + ((unsigned long long)fi << 16) + (unsigned long long)(j0 + lane);
          const int s = c.sub[f.seg + hdt_draw(base, js, (unsigned long long)kp)];
          thr_l = hdt_feat(c.ims, c.spx[rb + s], row, c.H, c.W, h0, w0, h1, w1);
        }
        const int ju = min(64, c.J - j0);
        for (int u = 0; u < ju; ++u) {
          const float thr = __shfl(thr_l, u);
          const unsigned long long L = __ballot(lane < kp && v < thr);
          const int cnt = __popcll(L & rmask);
          long long acc = lane < nruns ? c.X[cnt] + c.X[len - cnt] : 0;
#pragma unroll
          for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
          const int nL = __popcll(L), nR = kp - nL;
          if (nL < c.mleaf || nR < c.mleaf) continue;     // wave-uniform
          const long long cost = c.X[nL] + c.X[nR] - acc;
          if (cost < best) {                              // (f, j) ascending, strict <: the first minimum wins
            best = cost;
            bf = fi;
            bj = j0 + u;
          }
        }
      }
    }
    if (lane == 0) {
      HdtRes out = {};
      if (bf >= 0) {
        const unsigned long long fs = (1ull << 40) + 8ull * (unsigned long long)bf;
        out.split = 1;
        out.h0 = hdt_draw(base, fs, 32);
        out.w0 = hdt_draw(base, fs + 1, 32);
        out.h1 = hdt_draw(base, fs + 2, 32);
        out.w1 = hdt_draw(base, fs + 3, 32);
        const unsigned long long js = (1ull << 41) + ((unsigned long long)bf << 16) + (unsigned long long)bj;
        const int s = c.sub[f.seg + hdt_draw(base, js, (unsigned long long)kp)];
        out.thr = hdt_feat(c.ims, c.spx[rb + s], row, c.H, c.W, out.h0, out.w0, out.h1, out.w1);
      }
      c.res[i] = out;
    }
  }
}

__global__ __launch_bounds__(kTB) void hdt_cand_kernel(HdtCtx c, int cur, int depth) {
  extern __shared__ float hdt_ldsf[];                   // feat[kmax], runs[kmax]
  float* feat = hdt_ldsf;
  int* runs = (int*)(hdt_ldsf + c.kmax);
  __shared__ float s_thr[kTJ];
  __shared__ long long s_acc[kTWv][kTJ];
  __shared__ int s_nl[kTWv][kTJ];
  const long long nf = c.ctr[4 + cur];
  const HdtFront* fr = c.fr[cur];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (long long i = blockIdx.x; i < nf; i += gridDim.x) {
    const HdtFront f = fr[i];
    if (hdt_small(c, f, depth)) continue;                 // hdt_cand_small_kernel's
    HdtRes out = {};
    if (hdt_tries(c, f, depth) && min(c.nts, f.n) > c.kmax) {
      if (tid == 0) c.ctr[6] = 1;                       // the LDS was sized from the caller's counts: refuse
    } else if (hdt_tries(c, f, depth)) {
      const int n = f.n, kp = min(c.nts, n);
      const int r = f.rt / c.T, t = f.rt % c.T, row = c.row_from + r;
      const unsigned long long base = hdt_base(c.seed, row, t, f.heap);
      const int nruns = c.res[i].nruns;
      const long long rb = c.row_off[r];
      for (int q = tid; q < nruns; q += kTB) runs[q] = c.runs[f.seg + q];
      long long best = 0x7fffffffffffffffll;
      int bf = -1, bj = -1;
      for (int fi = 0; fi < c.F; ++fi) {
        const unsigned long long fs = (1ull << 40) + 8ull * (unsigned long long)fi;
        const int h0 = hdt_draw(base, fs, 32), w0 = hdt_draw(base, fs + 1, 32);
        const int h1 = hdt_draw(base, fs + 2, 32), w1 = hdt_draw(base, fs + 3, 32);
        __syncthreads();                                  // the previous function's features are consumed
        for (int j = tid; j < kp; j += kTB) feat[j] = hdt_feat(c.ims, c.sg[f.seg + j], row, c.H, c.W, h0, w0, h1, w1);
        for (int j0 = 0; j0 < c.J; j0 += kTJ) {
          if (tid < kTJ && j0 + tid < c.J) {
            const unsigned long long js = (1ull << 41) + ((unsigned long long)fi << 16) + (unsigned long long)(j0 + tid);
            const int e = c.sub[f.seg + hdt_draw(base, js, (unsigned long long)kp)];
            s_thr[tid] = hdt_feat(c.ims, c.spx[rb + e], row, c.H, c.W, h0, w0, h1, w1);
          }
          __syncthreads();
          float thr[kTJ];
#pragma unroll
          for (int u = 0; u < kTJ; ++u) thr[u] = s_thr[u];
          long long acc[kTJ];
          int nl[kTJ];
#pragma unroll
          for (int u = 0; u < kTJ; ++u) acc[u] = 0, nl[u] = 0;
          for (int q = tid; q < nruns; q += kTB) {
            const int b = q ? runs[q - 1] : 0, e = runs[q];
            int cnt[kTJ];
#pragma unroll
            for (int u = 0; u < kTJ; ++u) cnt[u] = 0;
            for (int x = b; x < e; ++x) {
              const float v = feat[x];
#pragma unroll
              for (int u = 0; u < kTJ; ++u) cnt[u] += v < thr[u];
            }
#pragma unroll
            for (int u = 0; u < kTJ; ++u) {
              acc[u] += c.X[cnt[u]] + c.X[e - b - cnt[u]];
              nl[u] += cnt[u];
            }
          }
#pragma unroll
          for (int u = 0; u < kTJ; ++u) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
              acc[u] += __shfl_xor(acc[u], m);
              nl[u] += __shfl_xor(nl[u], m);
            }
          }
          if (lane == 0) {
#pragma unroll
            for (int u = 0; u < kTJ; ++u) s_acc[wv][u] = acc[u], s_nl[wv][u] = nl[u];
          }
          __syncthreads();
          if (tid == 0) {
            for (int u = 0; u < kTJ && j0 + u < c.J; ++u) {  // (f, j) ascending, strict <: the first minimum wins
              long long a = 0;
              int nL = 0;
              for (int w = 0; w < kTWv; ++w) a += s_acc[w][u], nL += s_nl[w][u];
              const int nR = kp - nL;
              if (nL < c.mleaf || nR < c.mleaf) continue;
              const long long cost = c.X[nL] + c.X[nR] - a;
              if (cost < best) {
                best = cost;
                bf = fi;
                bj = j0 + u;
              }
            }
          }
          __syncthreads();                                // s_thr / s_acc are rewritten next pass
        }
      }
      if (tid == 0 && bf >= 0) {
        const unsigned long long fs = (1ull << 40) + 8ull * (unsigned long long)bf;
        out.split = 1;
        out.h0 = hdt_draw(base, fs, 32);
        out.w0 = hdt_draw(base, fs + 1, 32);
        out.h1 = hdt_draw(base, fs + 2, 32);
        out.w1 = hdt_draw(base, fs + 3, 32);
        const unsigned long long js = (1ull << 41) + ((unsigned long long)bf << 16) + (unsigned long long)bj;
        const int e = c.sub[f.seg + hdt_draw(base, js, (unsigned long long)kp)];
        out.thr = hdt_feat(c.ims, c.spx[rb + e], row, c.H, c.W, out.h0, out.w0, out.h1, out.w1);
      }
    }
    if (tid == 0) c.res[i] = out;
    __syncthreads();
  }
}

// ---- 3. partition the split nodes, build the leaves' lists ----
__global__ __launch_bounds__(kTB) void hdt_part_leaf_kernel(HdtCtx c, int cur, int depth) {
  extern __shared__ int hdt_hist[];                     // kTHistChunk
  __shared__ long long s_wl[kTWv];
  __shared__ int s_wi[kTWv];
  __shared__ int s_cl[kTB];
  __shared__ int s_first[kTB];
  const long long nf = c.ctr[4 + cur];
  const HdtFront* fr = c.fr[cur];
  const int* src = c.buf[depth & 1];
  int* dst = c.buf[(depth & 1) ^ 1];
  const int tid = threadIdx.x;
  for (long long i = blockIdx.x; i < nf; i += gridDim.x) {
    const HdtFront f = fr[i];
    const HdtRes rs = c.res[i];
    const int n = f.n;
    const int r = f.rt / c.T, row = c.row_from + r;
    const long long rb = c.row_off[r];
    const int* s = src + f.seg;
    if (rs.split) {
      long long nl = 0;
      for (int j = tid; j < n; j += kTB)
        nl += hdt_feat(c.ims, c.spx[rb + s[j]], row, c.H, c.W, rs.h0, rs.w0, rs.h1, rs.w1) < rs.thr;
      const int nL = (int)hdt_sum(nl, s_wl);
      int lb = 0, rbase = nL;
      for (int j0 = 0; j0 < n; j0 += kTB) {
        const int j = j0 + tid;
        bool left = false;
        int e = 0;
        if (j < n) {
          e = s[j];
          left = hdt_feat(c.ims, c.spx[rb + e], row, c.H, c.W, rs.h0, rs.w0, rs.h1, rs.w1) < rs.thr;
        }
        int tot;
        const int pre = hdt_flag_scan(left, tot, s_wi);
        if (j < n) dst[f.seg + (left ? lb + pre : rbase + (j - j0) - pre)] = e;
        lb += tot;
        rbase += min(kTB, n - j0) - tot;
      }
      if (tid == 0) c.res[i].nL = nL;
    } else {
      int len = 0;
      int2* ent = c.etmp + f.seg;
      if (n <= kTB) {                                     // rank of each first-of-its-class sample
        int cl = 0;
        if (tid < n) s_cl[tid] = cl = c.scl[rb + s[tid]];
        __syncthreads();
        int cnt = 0, first = 1;
        if (tid < n) {
          for (int k = 0; k < n; ++k) {
            const int o = s_cl[k];
            cnt += o == cl;
            first &= !(o == cl && k < tid);
          }
        }
        first &= tid < n;
        s_first[tid] = first;
        __syncthreads();
        if (first) {
          int rank = 0;
          for (int k = 0; k < n; ++k) rank += s_first[k] && s_cl[k] < cl;
          ent[rank] = make_int2(cl, cnt);
        }
        len = (int)hdt_sum(first, s_wl);
      } else {                                            // class histogram, kTHistChunk classes per pass
        long long lo = 0x7fffffff, hi = 0;
        for (int j = tid; j < n; j += kTB) {
          const int cl = c.scl[rb + s[j]];
          lo = min(lo, (long long)cl);
          hi = max(hi, (long long)cl);
        }
        for (int m = 32; m >= 1; m >>= 1) {
          lo = min(lo, (long long)__shfl_xor(lo, m));
          hi = max(hi, (long long)__shfl_xor(hi, m));
        }
        __syncthreads();
        if ((tid & 63) == 0) s_wl[tid >> 6] = lo;
        __syncthreads();
        for (int w = 0; w < kTWv; ++w) lo = min(lo, s_wl[w]);
        __syncthreads();
        if ((tid & 63) == 0) s_wl[tid >> 6] = hi;
        __syncthreads();
        for (int w = 0; w < kTWv; ++w) hi = max(hi, s_wl[w]);
        __syncthreads();
        for (long long c0 = lo; c0 <= hi; c0 += kTHistChunk) {
          for (int k = tid; k < kTHistChunk; k += kTB) hdt_hist[k] = 0;
          __syncthreads();
          for (int j = tid; j < n; j += kTB) {
            const long long cl = c.scl[rb + s[j]];
            if (cl >= c0 && cl < c0 + kTHistChunk) atomicAdd(&hdt_hist[cl - c0], 1);
          }
          __syncthreads();
          for (int k0 = 0; k0 < kTHistChunk; k0 += kTB) {
            const int h = hdt_hist[k0 + tid];
            int tot;
            const int pre = hdt_flag_scan(h != 0, tot, s_wi);
            if (h) ent[len + pre] = make_int2((int)(c0 + k0 + tid), h);
            len += tot;
          }
        }
      }
      if (tid == 0) c.res[i].elen = len;
    }
    __syncthreads();
  }
}

// ---- 4. plan: indices in frontier order, table records, links, next frontier ----
__global__ __launch_bounds__(kTB) void hdt_plan_kernel(HdtCtx c, int cur, int depth) {
  __shared__ int s_wi[kTWv];
  __shared__ long long s_wl[kTWv];
  __shared__ int s_leaf, s_err;
  const long long nf = c.ctr[4 + cur];
  const HdtFront* fr = c.fr[cur];
  HdtFront* nx = c.fr[cur ^ 1];
  const int tid = threadIdx.x;
  if (tid == 0) s_leaf = 0, s_err = 0;
  __syncthreads();
  long long S0 = c.ctr[0], L0 = c.ctr[1], E0 = c.ctr[2], ns = 0;
  for (long long i0 = 0; i0 < nf; i0 += kTB) {
    const long long i = i0 + tid;
    const bool on = i < nf;
    HdtFront f = {};
    HdtRes rs = {};
    if (on) f = fr[i], rs = c.res[i];
    const bool sp = on && rs.split, lf = on && !rs.split;
    int ts, tl;
    const int ps = hdt_flag_scan(sp, ts, s_wi);
    const int pl = hdt_flag_scan(lf, tl, s_wi);
    long long te;
    const long long pe = hdt_scan(lf ? rs.elen : 0, te, s_wl);
    int v = 0;
    bool ok = true;
    if (sp) {
      const long long s = S0 + ps, k = 2 * (ns + ps);
      if (s >= c.out.cap_nodes || s > 0x7fffffffll || k + 1 >= c.Fcap) {
        ok = false;
      } else {
        int* nd = c.out.nodes + 8 * s;
        nd[0] = __float_as_int(rs.thr);
        nd[1] = rs.h0;
        nd[2] = rs.w0;
        nd[3] = rs.h1;
        nd[4] = rs.w1;
        nd[5] = -1;
        nd[6] = -1;
        nd[7] = 0;
        HdtFront a = f, b = f;
        a.link = 8 * s + 5;
        a.heap = 2 * f.heap;
        a.n = rs.nL;
        b.seg = f.seg + rs.nL;
        b.link = 8 * s + 6;
        b.heap = 2 * f.heap + 1;
        b.n = f.n - rs.nL;
        nx[k] = a;
        nx[k + 1] = b;
        v = (int)s;
      }
    } else if (lf) {
      const long long l = L0 + pl, e = E0 + pe;
      if (l >= c.out.cap_leaves || l > 0x7fffffffll || e + rs.elen > c.out.cap_entries) {
        ok = false;
      } else {
        c.out.leaf_off[l] = e;
        c.out.leaf_sum[l] = f.n;
        c.ltmp[l] = f.seg;
        c.llen[l] = rs.elen;
        v = ~(int)l;
        s_leaf = 1;
      }
    }
    if (!ok) s_err = 1;
    if (on && ok) {
      if (f.link >= 0)
        c.out.nodes[f.link] = v;
      else
        c.out.roots[~f.link] = v;
    }
    S0 += ts;
    L0 += tl;
    E0 += te;
    ns += ts;
  }
  __syncthreads();
  if (tid == 0) {
    c.ctr[0] = S0;
    c.ctr[1] = L0;
    c.ctr[2] = E0;
    if (s_leaf) c.ctr[3] = depth;
    if (s_err) c.ctr[6] = 1;
    c.ctr[4 + (cur ^ 1)] = s_err ? 0 : min(2 * ns, c.Fcap);
  }
}

// ---- final: packed entries, used sizes ----
__global__ __launch_bounds__(kTB) void hdt_final_kernel(HdtCtx c) {
  const long long L = c.ctr[1];
  for (long long l = blockIdx.x; l < L; l += gridDim.x) {
    const long long o = c.out.leaf_off[l], s = c.ltmp[l];
    const int len = c.llen[l];
    for (int k = threadIdx.x; k < len; k += kTB) ((int2*)c.out.entries)[o + k] = c.etmp[s + k];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (L < c.out.cap_leaves + 1) c.out.leaf_off[L] = c.ctr[2];
    c.out.used[0] = c.ctr[0];
    c.out.used[1] = L;
    c.out.used[2] = c.ctr[2];
    c.out.used[3] = c.ctr[3];
    c.out.used[4] = c.ctr[6];
  }
}

// ---- host side ----
struct HdtLayout {
  long long S = 0, TS = 0, Fcap = 0, maxn = 0;
  size_t off[16] = {};
  size_t bytes = 0;
};

static HdtLayout hdt_layout(const ctd_hd_train_params& p, int R, const int64_t* counts) {
  HdtLayout L;
  const long long T = p.n_trees;
  const long long lim = 1ll << p.max_tree_depth;
  for (int r = 0; r < R; ++r) {
    const long long n = counts[r];
    L.S += n;
    L.maxn = n > L.maxn ? n : L.maxn;
    long long f = n / p.min_samples_for_leaf;
    f = f < lim ? f : lim;
    L.Fcap += T * (f > 1 ? f : 1);
  }
  L.TS = T * L.S;
  const size_t sz[] = {
      8 * (size_t)R,                                        // 0 counts
      8 * ((size_t)R + 1),                                  // 1 row_off
      8 * (size_t)L.S,                                      // 2 spx
      4 * (size_t)L.S,                                      // 3 scl
      4 * (size_t)L.TS,                                     // 4 buf 0
      4 * (size_t)L.TS,                                     // 5 buf 1
      4 * (size_t)L.TS,                                     // 6 sub
      8 * (size_t)L.TS,                                     // 7 sg
      4 * (size_t)L.TS,                                     // 8 runs
      8 * (size_t)L.TS,                                     // 9 etmp
      4 * ((size_t)L.TS / 32 + (size_t)L.Fcap + 1),         // 10 bm
      sizeof(HdtFront) * (size_t)L.Fcap,                    // 11 fr 0
      sizeof(HdtFront) * (size_t)L.Fcap,                    // 12 fr 1
      sizeof(HdtRes) * (size_t)L.Fcap,                      // 13 res
      8 * 8,                                                // 14 ctr
  };
  size_t o = 0;
  for (int k = 0; k < 15; ++k) {
    L.off[k] = o;
    o = align_up(o + sz[k], 256);
  }
  L.bytes = o;
  return L;
}

static size_t hyperdepth_train_workspace_bytes(const ctd_hd_train_params& p, int R, const int64_t* counts,
                                               long long cap_leaves) {
  return hdt_layout(p, R, counts).bytes + align_up(12 * (size_t)(cap_leaves > 0 ? cap_leaves : 0), 256);
}

static int hyperdepth_train_count_f32(const float* disps, int N, int H, int W, int row_from, int row_to, int nb,
                                      int64_t* counts, hipStream_t stream) {
  hipLaunchKernelGGL(hdt_count_kernel, dim3(row_to - row_from), dim3(kTB), 0, stream, disps, N, H, W, row_from, nb,
                     W * nb, (long long*)counts);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int hyperdepth_train_f32(const ctd_hd_train_params& p, const int64_t* X, const uint8_t* ims, const float* disps,
                                int N, int H, int W, int row_from, int row_to, const int64_t* counts, void* ws,
                                size_t ws_bytes, const ctd_hd_train_out& out, hipStream_t stream) {
  const int R = row_to - row_from;
  const HdtLayout L = hdt_layout(p, R, counts);
  if (ws_bytes < hyperdepth_train_workspace_bytes(p, R, counts, out.cap_leaves)) return CTD_ERR_WORKSPACE;
  char* w = (char*)ws;
  HdtCtx c;
  c.ims = ims;
  c.disps = disps;
  c.X = (const long long*)X;
  c.N = N, c.H = H, c.W = W, c.row_from = row_from, c.R = R, c.T = p.n_trees, c.nb = p.n_disp_bins;
  c.dsw = p.depth_switch, c.C = W * p.n_disp_bins, c.F = p.n_test_split_functions, c.J = p.n_test_thresholds;
  c.nts = p.n_test_samples, c.msplit = p.min_samples_to_split, c.mleaf = p.min_samples_for_leaf;
  c.D = p.max_tree_depth;
  c.kmax = (int)(L.maxn < p.n_test_samples ? L.maxn : p.n_test_samples);
  if (c.kmax < 1) c.kmax = 1;
  c.seed = p.seed;
  c.S = L.S, c.TS = L.TS, c.Fcap = L.Fcap;
  c.counts = (long long*)(w + L.off[0]);
  c.row_off = (long long*)(w + L.off[1]);
  c.spx = (int2*)(w + L.off[2]);
  c.scl = (int*)(w + L.off[3]);
  c.buf[0] = (int*)(w + L.off[4]);
  c.buf[1] = (int*)(w + L.off[5]);
  c.sub = (int*)(w + L.off[6]);
  c.sg = (int2*)(w + L.off[7]);
  c.runs = (int*)(w + L.off[8]);
  c.etmp = (int2*)(w + L.off[9]);
  c.bm = (unsigned*)(w + L.off[10]);
  c.fr[0] = (HdtFront*)(w + L.off[11]);
  c.fr[1] = (HdtFront*)(w + L.off[12]);
  c.res = (HdtRes*)(w + L.off[13]);
  c.ctr = (long long*)(w + L.off[14]);
  c.ltmp = (long long*)(w + L.bytes);
  c.llen = (int*)(w + L.bytes + 8 * (size_t)(out.cap_leaves > 0 ? out.cap_leaves : 0));
  c.out = out;

  // the device recounts (the same rule as ctd_hyperdepth_train_count_f32) and refuses, through the error flag, a
  // total above the one the workspace was sized for
  hipLaunchKernelGGL(hdt_count_kernel, dim3(R), dim3(kTB), 0, stream, disps, N, H, W, row_from, c.nb, c.C, c.counts);
  CTD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hdt_setup_kernel, dim3(1), dim3(kTB), 0, stream, c);
  CTD_LAUNCH_CHECK();
  hipLaunchKernelGGL(hdt_extract_kernel, dim3(R), dim3(kTB), 0, stream, c);
  CTD_LAUNCH_CHECK();
  const size_t cand_lds = 8 * (size_t)c.kmax;
  for (int d = 0; d <= c.D; ++d) {
    // frontier bound of level d (grid size only; the kernels read the true count from the device)
    long long fb = 0;
    for (int r = 0; r < R; ++r) {
      long long f = d == 0 ? 1 : counts[r] / c.mleaf;
      const long long lim = 1ll << d;
      f = f < lim ? f : lim;
      fb += (long long)c.T * (f > 1 ? f : 1);
    }
    const unsigned grid = (unsigned)(fb < kTGrid ? (fb > 0 ? fb : 1) : kTGrid);
    const int cur = d & 1;
    if (d < c.D) {
      hipLaunchKernelGGL(hdt_subset_kernel, dim3(grid), dim3(kTB), kTSubsetLds, stream, c, cur, d);
      CTD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(hdt_cand_kernel, dim3(grid), dim3(kTB), cand_lds, stream, c, cur, d);
    CTD_LAUNCH_CHECK();
    if (d < c.D) {
      hipLaunchKernelGGL(hdt_cand_small_kernel, dim3((grid + kTWv - 1) / kTWv), dim3(kTB), 0, stream, c, cur, d);
      CTD_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(hdt_part_leaf_kernel, dim3(grid), dim3(kTB), 4 * kTHistChunk, stream, c, cur, d);
    CTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(hdt_plan_kernel, dim3(1), dim3(kTB), 0, stream, c, cur, d);
    CTD_LAUNCH_CHECK();
  }
  long long lb = out.cap_leaves < kTGrid ? out.cap_leaves : kTGrid;
  hipLaunchKernelGGL(hdt_final_kernel, dim3((unsigned)(lb > 0 ? lb : 1)), dim3(kTB), 0, stream, c);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

static bool hd_train_shape_ok(int N, int H, int W, int row_from, int row_to, int nb) {
  if (N < 1 || H < 1 || W < 1 || H >= (1 << 24) || W >= (1 << 24)) return false;
  if ((long long)N * H * W >= (1ll << 31)) return false;
  if (row_from < 0 || row_from >= row_to || row_to > H) return false;
  return nb >= 1 && (long long)W * nb < (1ll << 31);
}

static bool hd_train_params_ok(const ctd_hd_train_params* p) {
  return p && p->n_trees >= 1 && p->n_trees <= 16 && p->max_tree_depth >= 0 && p->max_tree_depth <= 24 &&
         p->n_test_split_functions >= 0 && p->n_test_split_functions < (1 << 20) && p->n_test_thresholds >= 0 &&
         p->n_test_thresholds < (1 << 16) && p->n_test_samples >= 1 && p->n_test_samples <= 8192 &&
         p->min_samples_to_split >= 0 && p->min_samples_for_leaf >= 1 && p->n_disp_bins >= 1;
}

int ctd_hyperdepth_train_count_f32(const float* disps, int N, int H, int W, int row_from, int row_to,
                                   int n_disp_bins, int64_t* counts, int device, void* stream) {
  if (!disps || !counts || !hd_train_shape_ok(N, H, W, row_from, row_to, n_disp_bins)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return hyperdepth_train_count_f32(disps, N, H, W, row_from, row_to, n_disp_bins, counts, (hipStream_t)stream);
}

size_t ctd_hyperdepth_train_workspace_bytes(const ctd_hd_train_params* params, int n_rows, const int64_t* row_counts,
                                            int64_t cap_leaves) {
  if (!hd_train_params_ok(params) || n_rows < 1 || !row_counts || cap_leaves < 0) return 0;
  for (int r = 0; r < n_rows; ++r)
    if (row_counts[r] < 0) return 0;
  return hyperdepth_train_workspace_bytes(*params, n_rows, row_counts, cap_leaves);
}

int ctd_hyperdepth_train_f32(const ctd_hd_train_params* params, const int64_t* X, int n_x, const uint8_t* ims,
                             const float* disps, int N, int H, int W, int row_from, int row_to,
                             const int64_t* row_counts, void* workspace, size_t workspace_bytes,
                             const ctd_hd_train_out* out, int device, void* stream) {
  if (!hd_train_params_ok(params) || !X || !ims || !disps || !row_counts || !workspace || !out) return CTD_ERR_INVALID_ARG;
  if (!hd_train_shape_ok(N, H, W, row_from, row_to, params->n_disp_bins)) return CTD_ERR_INVALID_ARG;
  if (n_x < params->n_test_samples + 1) return CTD_ERR_INVALID_ARG;
  const ctd_hd_train_out o = *out;
  if (!o.roots || !o.leaf_off || !o.leaf_sum || !o.used || o.cap_nodes < 0 || o.cap_leaves < 0 || o.cap_entries < 0 ||
      (o.cap_nodes > 0 && !o.nodes) || (o.cap_entries > 0 && !o.entries))
    return CTD_ERR_INVALID_ARG;
  if ((uintptr_t)o.entries % 8 || (uintptr_t)o.leaf_off % 8 || (uintptr_t)o.used % 8 || (uintptr_t)X % 8 ||
      (uintptr_t)workspace % 256)
    return CTD_ERR_INVALID_ARG;
  for (int r = 0; r < row_to - row_from; ++r)
    if (row_counts[r] < 0) return CTD_ERR_INVALID_ARG;
  if (workspace_bytes < hyperdepth_train_workspace_bytes(*params, row_to - row_from, row_counts, o.cap_leaves))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return hyperdepth_train_f32(*params, X, ims, disps, N, H, W, row_from, row_to, row_counts, workspace,
                              workspace_bytes, o, (hipStream_t)stream);
}

}  // extern "C"
