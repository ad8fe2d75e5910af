// match_validity.hip -- which disparities of a winner-takes-all matcher can be trusted: the pattern-side match idx_r,
// the uniqueness gap and the flag byte of include/ctd_hip.h (ctd_match_validity_f32, ctd_xcorrvol_validity_f32,
// ctd_costvol_validity_f32; the three definitions are stated there word for word).
//
//   1. scan pass: one thread per (frame, row, column) walks the disparities of a materialised volume once.  As pixel w
//      it keeps s1 = V[idx] and the best score s2 over |d - idx| >= 2; as pattern column x = w it keeps the best score
//      b1, its first index i1 and the runner-up b2 along the diagonal V[d][x + d].  Row d is read at w and at w + d:
//      both loads are coalesced and the second one finds the row in cache, so the volume leaves memory once.  Costs
//      are negated as they are loaded (exact), so that one set of comparisons serves both families.
//      On an exact volume the pass is final.  On a fast (tolerance-level) volume it takes the decisions the bound
//      proves and lists the others (below); the decision is taken where the scores sit in registers, not in a pass of
//      its own.
//   2. re-scoring pass (fast volumes only): one wavefront per listed pixel / pattern column evaluates all its D scores
//      in the reference order (ncc_ref_point below = XCorrVolFunctor; costvol_ref_cost = the tap loop of
//      ctd_costvol_f32) and takes the decision again.
//   3. flag pass: LR_OK is the gather idx_r[w - idx], after every idx_r is final.
//
// Why a decision on fast scores stands.  Fast scores f and reference-order scores x obey |f - x| <= r |x| + a
// (r = 1e-5, a = 1e-6: the bounds ctd_hip.h states for CTD_NCC_FAST with one channel and for ctd_costvol_fast_f32), so
// |x| <= (|f| + a) / (1 - r) and
//     |f - x| <= e(f) := r (|f| + a) / (1 - r) + a.
// f + e(f) and f - e(f) both grow with f (slope 1 -+ r / (1 - r) > 0).  In the maximising domain (costs negated):
//   pattern side: every d != i1 has f(d) <= b2, so x(d) <= b2 + e(b2), and x(i1) >= b1 - e(b1).  If
//       b1 - b2 > e(b1) + e(b2)
//     then x(i1) > x(d) for every other d: i1 is the unique best of the reference-order diagonal, its first index.
//     Exact ties (b2 == b1) always fail the test.
//   uniqueness: s1 = x(idx) lies within e(f(idx)) of the fast score, and s2 = max x over the non-adjacent d lies within
//     e(s2_fast) of the fast maximum (the maximum of x is at most max (f + e(f)) = s2_fast + e(s2_fast) and at least
//     x at the fast maximum's index).  With E = e(s1_fast) + e(s2_fast) the real difference s1 - s2 lies within E of
//     the fast one; gap is that difference rounded to f32 once, which moves it by at most 2^-24 of itself and never
//     across a float it does not reach.  So `gap > min_gap` is decided when
//       |gap_fast - min_gap| > E + rho,   rho = 2^-22 (|gap_fast| + E + min_gap)
//     (evaluated in f64; every right side is raised by 2^-40 of itself for the rounding of the products).
// Comparisons are written so that a NaN lists the pixel / column.
#include <limits.h>

#include "ctd_costvol_ref.h"
#include "ctd_internal.h"
#include "ctd_ncc_point.h"
#include "ctd_validate.h"

namespace ctd {

constexpr double kValRel = 1e-5, kValAbs = 1e-6;
constexpr int kValBatch = 8;                   // independent row loads in flight per thread and side
constexpr int kFamNcc = 4;                     // score family of the re-scoring pass: 0..3 cost types, 4 NCC

__device__ inline double val_err(double f) {
  return (kValRel * (fabs(f) + kValAbs) / (1.0 - kValRel) + kValAbs) * (1.0 + 0x1p-40);
}

// appends `item` to list for every lane with `take`: one atomic per wavefront
__device__ inline void val_append(bool take, unsigned item, unsigned* __restrict__ counter, unsigned* __restrict__ list) {
  const unsigned long long m = __ballot(take);
  if (!m) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((long long)m) - 1;
  unsigned base = 0;
  if (lane == leader) base = atomicAdd(counter, (unsigned)__popcll(m));
  base = __shfl(base, leader);
  if (take) list[base + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = item;
}

// grid (ceil(W / 256), H, frames).  Writes gap, idx_r and bits 0 and 2 of flags (bit 1 is the flag pass's).
template <bool MAXI, bool FAST>
__global__ __launch_bounds__(256) void validity_scan_kernel(const float* __restrict__ vol, const int64_t* __restrict__ idx,
                                                            uint8_t* __restrict__ flags, int64_t* __restrict__ idx_r,
                                                            float* __restrict__ gap, int D, int H, int W, float min_gap,
                                                            unsigned* __restrict__ counters,
                                                            unsigned* __restrict__ pix_list,
                                                            unsigned* __restrict__ col_list) {
  const int w = blockIdx.x * 256 + threadIdx.x;
  if (w >= W) return;
  const int h = blockIdx.y;
  const long f = blockIdx.z;
  const long HW = (long)H * W;
  const long p = f * HW + (long)h * W + w;
  const float* v = vol + f * D * HW + (long)h * W + w;
  const int64_t di = idx[p];
  const bool in_range = di >= 0 && di < D;
  const int d0 = in_range ? (int)di : INT_MIN / 2;       // out of range: never equal, never adjacent (unused then)
  const float ninf = -__builtin_inff();
  float s1 = ninf, s2 = ninf;                            // pixel side
  float b1 = ninf, b2 = ninf;                            // pattern side
  int i1 = 0;
  const int n_diag = min(D, W - w);                      // disparities of pattern column x = w: x + d < W
  for (int db = 0; db < D; db += kValBatch) {
    float a[kValBatch], b[kValBatch];
#pragma unroll
    for (int u = 0; u < kValBatch; ++u) {
      const int d = min(db + u, D - 1);
      a[u] = v[(long)d * HW];
      const int dx = d < n_diag ? d : 0;                 // (w + dx < W: inside the row)
      b[u] = v[(long)dx * HW + dx];
    }
#pragma unroll
    for (int u = 0; u < kValBatch; ++u) {
      const int d = db + u;
      const float ya = MAXI ? a[u] : -a[u];
      const float yb = MAXI ? b[u] : -b[u];
      if (d < D) {
        const int ad = d > d0 ? d - d0 : d0 - d;
        s1 = d == d0 ? ya : s1;
        s2 = ad >= 2 ? fmaxf(s2, ya) : s2;
      }
      if (d < n_diag) {
        b2 = __builtin_amdgcn_fmed3f(b1, b2, yb);        // runner-up = second largest of {b1 >= b2, yb}
        i1 = yb > b1 ? d : i1;                           // strict >: the first index keeps a tie
        b1 = fmaxf(b1, yb);
      }
    }
  }
  // pixel side
  float g = __builtin_nanf("");
  bool unique = false, list_pix = false;
  if (in_range) {
    g = s1 - s2;                                         // +inf when no non-adjacent disparity exists
    unique = g > min_gap;
    if (FAST && s2 != ninf) {
      const double E = val_err(s1) + val_err(s2);
      const double df = (double)s1 - (double)s2;
      const double rho = 0x1p-22 * (fabs(df) + E + (double)min_gap);
      list_pix = !(fabs(df - (double)min_gap) > (E + rho) * (1.0 + 0x1p-40));
    }
  }
  gap[p] = g;
  flags[p] = (uint8_t)((in_range && w - d0 >= 0 ? 1 : 0) | (unique ? 4 : 0));
  // pattern side
  idx_r[p] = i1;
  if (FAST) {
    const bool sure = b2 == ninf || (double)b1 - (double)b2 > val_err(b1) + val_err(b2);
    val_append(list_pix, (unsigned)p, counters, pix_list);
    val_append(!sure, (unsigned)p, counters + 1, col_list);
  }
}

// XCorrVolFunctor<float>::operator(), ext.h:133-190, one channel: means of the quotients first, then the three sums, every
// accumulator its own chain in tap order; the pattern column shifts before it clamps (ext.h:152-154)
__device__ inline float ncc_ref_point(const float* __restrict__ a, const float* __restrict__ e, int h, int w, int d, int H,
                                      int W, int bs) {
  const int half = bs / 2;
  const float bs2 = (float)(bs * bs);
  float mu0 = 0.f, mu1 = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
    for (int bw = 0; bw < bs; ++bw) {
      const int w0 = w + bw - half;
      mu0 += a[r + clampi(w0, 0, W - 1)] / bs2;
      mu1 += e[r + clampi(w0 - d, 0, W - 1)] / bs2;
    }
  }
  float s0 = 0.f, s1 = 0.f, dot = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
    for (int bw = 0; bw < bs; ++bw) {
      const int w0 = w + bw - half;
      const float v0 = a[r + clampi(w0, 0, W - 1)] - mu0;
      const float v1 = e[r + clampi(w0 - d, 0, W - 1)] - mu1;
      dot += v0 * v1;
      s0 += v0 * v0;
      s1 += v1 * v1;
    }
  }
  float val = 0.f;
  val += dot / ncc_norm(s0, s1);
  return val;
}

// reference-order score of (h, w, d) in the maximising domain
template <int FAM>
__device__ inline float val_ref_score(const float* __restrict__ t, const float* __restrict__ e, int h, int w, int d, int H,
                                      int W, int bs, float eps) {
  if constexpr (FAM == kFamNcc) return ncc_ref_point(t, e, h, w, d, H, W, bs);
  else return -costvol_ref_cost<FAM>(t, e, h, w, d, H, W, bs, eps);
}

__device__ inline float val_wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// one wavefront per listed item, lane l evaluates d = l, l + 64, ...; the counts are read on the device (the grid is
// sized without a host sync).  Items [0, n_pix) are pixels, the rest pattern columns.
template <int FAM>
__global__ __launch_bounds__(256) void validity_rescore_kernel(const float* __restrict__ in0, const float* __restrict__ in1,
                                                               long in1_frame_stride, const int64_t* __restrict__ idx,
                                                               uint8_t* __restrict__ flags, int64_t* __restrict__ idx_r,
                                                               float* __restrict__ gap, int H, int W, int D, int bs,
                                                               float eps, float min_gap,
                                                               const unsigned* __restrict__ counters,
                                                               const unsigned* __restrict__ pix_list,
                                                               const unsigned* __restrict__ col_list) {
  const unsigned long long n_pix = counters[0], n = n_pix + counters[1];
  const int lane = threadIdx.x & 63;
  const long HW = (long)H * W;
  const float ninf = -__builtin_inff();
  for (unsigned long long k = (unsigned long long)blockIdx.x * 4 + (threadIdx.x >> 6); k < n;
       k += (unsigned long long)gridDim.x * 4) {
    const bool is_pix = k < n_pix;                       // wave-uniform
    const unsigned p = is_pix ? pix_list[k] : col_list[k - n_pix];
    const long f = p / HW, px = p - f * HW;
    const int h = (int)(px / W), w = (int)(px - (long)h * W);
    const float* t = in0 + f * HW;
    const float* e = in1 + f * in1_frame_stride;
    if (is_pix) {
      const int d0 = (int)idx[p];                        // listed pixels have 0 <= idx < D
      float s1 = ninf, s2 = ninf;
      for (int d = lane; d < D; d += 64) {
        const float y = val_ref_score<FAM>(t, e, h, w, d, H, W, bs, eps);
        const int ad = d > d0 ? d - d0 : d0 - d;
        if (ad == 0) s1 = y;
        else if (ad >= 2) s2 = fmaxf(s2, y);
      }
      s1 = val_wave_max(s1);
      s2 = val_wave_max(s2);
      if (lane == 0) {
        const float g = s1 - s2;
        gap[p] = g;
        flags[p] = (uint8_t)((flags[p] & ~4) | (g > min_gap ? 4 : 0));
      }
    } else {
      const int n_diag = min(D, W - w);
      float b = ninf;
      int di = INT_MAX;
      for (int d = lane; d < n_diag; d += 64) {          // ascending d per lane: strict > keeps the first
        const float y = val_ref_score<FAM>(t, e, h, w + d, d, H, W, bs, eps);
        if (y > b) {
          b = y;
          di = d;
        }
      }
#pragma unroll
      for (int s = 32; s > 0; s >>= 1) {
        const float ob = __shfl_xor(b, s);
        const int od = __shfl_xor(di, s);
        if (ob > b || (ob == b && od < di)) {
          b = ob;
          di = od;
        }
      }
      if (lane == 0) idx_r[p] = di == INT_MAX ? 0 : di;
    }
  }
}

// LR_OK (bit 1): bit 0 holds and |idx_r[f][h][w - idx] - idx| <= lr_tol
__global__ __launch_bounds__(256) void validity_flag_kernel(const int64_t* __restrict__ idx,
                                                            const int64_t* __restrict__ idx_r,
                                                            uint8_t* __restrict__ flags, long P, int lr_tol) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const uint8_t fl = flags[p];
  if (!(fl & 1)) return;                                 // (bit 0: 0 <= idx < D and w - idx >= 0, the same row)
  const int64_t d = idx[p];
  const int64_t diff = idx_r[p - d] - d;
  if ((diff < 0 ? -diff : diff) <= (int64_t)lr_tol) flags[p] = (uint8_t)(fl | 2);
}

struct ValidityLayout {                        // workspace of the *_validity calls (byte offsets; ctd_hip.h documents it)
  size_t counters, pix_list, col_list, vol, inner, bytes;
};

static bool match_validity_supported(int frames, int H, int W) {
  return H <= 65535 && frames <= 65535 && (double)frames * H * W < 4294967296.0;
}

static ValidityLayout validity_layout(int frames, int H, int W, int D, size_t inner_bytes) {
  const size_t P = (size_t)frames * H * W;
  ValidityLayout l;
  l.counters = 0;
  l.pix_list = 256;
  l.col_list = align_up(l.pix_list + 4 * P, 256);
  l.vol = align_up(l.col_list + 4 * P, 256);
  l.inner = align_up(l.vol + 4 * P * (size_t)D, 256);
  l.bytes = align_up(l.inner + inner_bytes, 256);
  return l;
}

static int match_validity_scan_f32(const float* vol, bool maximise, bool fast, const int64_t* idx, uint8_t* flags,
                                   int64_t* idx_r, float* gap, int frames, int D, int H, int W, float min_gap,
                                   unsigned* counters, unsigned* pix_list, unsigned* col_list, hipStream_t stream) {
  const dim3 grid(ceil_div(W, 256), H, frames), block(256);
  auto kern = maximise ? (fast ? validity_scan_kernel<true, true> : validity_scan_kernel<true, false>)
                       : (fast ? validity_scan_kernel<false, true> : validity_scan_kernel<false, false>);
  hipLaunchKernelGGL(kern, grid, block, 0, stream, vol, idx, flags, idx_r, gap, D, H, W, min_gap, counters, pix_list,
                     col_list);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int match_validity_rescore_f32(int family, const float* in0, const float* in1, long in1_frame_stride,
                                      const int64_t* idx, uint8_t* flags, int64_t* idx_r, float* gap, int frames, int H,
                                      int W, int D, int bs, float eps, float min_gap, const unsigned* counters,
                                      const unsigned* pix_list, const unsigned* col_list, hipStream_t stream) {
  const long wgs_needed = ((long)frames * H * W * 2 + 3) / 4;      // four wavefronts per workgroup, an item each
  const unsigned grid = (unsigned)(wgs_needed < 4L * device_cu_count() ? wgs_needed : 4L * device_cu_count());
#define CTD_VAL_RESCORE(FAM)                                                                                         \
  hipLaunchKernelGGL(validity_rescore_kernel<FAM>, dim3(grid), dim3(256), 0, stream, in0, in1, in1_frame_stride, idx, \
                     flags, idx_r, gap, H, W, D, bs, eps, min_gap, counters, pix_list, col_list)
  switch (family) {
    case 0: CTD_VAL_RESCORE(0); break;
    case 1: CTD_VAL_RESCORE(1); break;
    case 2: CTD_VAL_RESCORE(2); break;
    case 3: CTD_VAL_RESCORE(3); break;
    default: CTD_VAL_RESCORE(kFamNcc); break;
  }
#undef CTD_VAL_RESCORE
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int match_validity_flags(const int64_t* idx, const int64_t* idx_r, uint8_t* flags, int frames, int H, int W,
                                int lr_tol, hipStream_t stream) {
  const long P = (long)frames * H * W;
  hipLaunchKernelGGL(validity_flag_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, idx, idx_r, flags, P,
                     lr_tol);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

static bool validity_args_ok(int lr_tol, float min_gap) { return lr_tol >= 0 && min_gap >= 0.f; }   // (a NaN fails >=)
static bool validity_block_fast(int bs) { return bs == 3 || bs == 5 || bs == 7 || bs == 9; }

int ctd_match_validity_f32(const float* vol, int maximise, const int64_t* idx, uint8_t* flags, int64_t* idx_r, float* gap,
                           int frames, int D, int H, int W, int lr_tol, float min_gap, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, 1) || !validity_args_ok(lr_tol, min_gap)) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!vol || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!match_validity_supported(frames, H, W)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  int st = match_validity_scan_f32(vol, maximise != 0, false, idx, flags, idx_r, gap, frames, D, H, W, min_gap, nullptr,
                                   nullptr, nullptr, hs);
  if (st) return st;
  return match_validity_flags(idx, idx_r, flags, frames, H, W, lr_tol, hs);
}

// scan of the volume in the workspace, exact re-scoring of the listed items (fast volumes), flag pass
static int validity_finish(const ValidityLayout& l, void* workspace, bool fast, int family, const float* in0,
                           const float* in1, long in1_frame_stride, const int64_t* idx, uint8_t* flags, int64_t* idx_r,
                           float* gap, int frames, int H, int W, int D, int bs, float eps, int lr_tol, float min_gap,
                           hipStream_t hs) {
  char* ws = (char*)workspace;
  unsigned* counters = (unsigned*)(ws + l.counters);
  unsigned* pix_list = (unsigned*)(ws + l.pix_list);
  unsigned* col_list = (unsigned*)(ws + l.col_list);
  int st = match_validity_scan_f32((const float*)(ws + l.vol), family == 4, fast, idx, flags, idx_r, gap, frames, D, H, W,
                                   min_gap, counters, pix_list, col_list, hs);
  if (st) return st;
  if (fast) {
    st = match_validity_rescore_f32(family, in0, in1, in1_frame_stride, idx, flags, idx_r, gap, frames, H, W, D, bs, eps,
                                    min_gap, counters, pix_list, col_list, hs);
    if (st) return st;
  }
  return match_validity_flags(idx, idx_r, flags, frames, H, W, lr_tol, hs);
}

static bool xcorrvol_validity_algo_ok(int C, int D, int bs, int algo) {
  return algo == CTD_NCC_EXACT || (C == 1 && validity_block_fast(bs) && D <= 512);
}

size_t ctd_xcorrvol_validity_workspace_bytes(int frames, int C, int H, int W, int D, int block_size, int algo) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || frames == 0 || (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST)) return 0;
  if (!match_validity_supported(frames, H, W) || !xcorrvol_validity_algo_ok(C, D, block_size, algo)) return 0;
  return validity_layout(frames, H, W, D, ctd_xcorrvol_workspace_bytes(frames, C, H, W, D, block_size, algo)).bytes;
}

int ctd_xcorrvol_validity_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                              uint8_t* flags, int64_t* idx_r, float* gap, int frames, int C, int H, int W, int D,
                              int block_size, int algo, int lr_tol, float min_gap, void* workspace,
                              size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, C, H, W, D, block_size) || !validity_args_ok(lr_tol, min_gap) ||
      (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST))
    return CTD_ERR_INVALID_ARG;
  if (in1_frame_stride != 0 && in1_frame_stride != (long)C * H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!match_validity_supported(frames, H, W) || !xcorrvol_validity_algo_ok(C, D, block_size, algo)) return CTD_ERR_UNSUPPORTED;
  const ValidityLayout l = validity_layout(frames, H, W, D, ctd_xcorrvol_workspace_bytes(frames, C, H, W, D, block_size, algo));
  if (!workspace || workspace_bytes < l.bytes || ((uintptr_t)workspace & 255)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  char* ws = (char*)workspace;
  CTD_HIP_TRY(hipMemsetAsync(ws + l.counters, 0, 2 * sizeof(unsigned), hs));
  int st = ctd_xcorrvol_f32(in0, in1, in1_frame_stride, (float*)(ws + l.vol), frames, C, H, W, D, block_size, algo,
                            ws + l.inner, l.bytes - l.inner, -1, stream);
  if (st) return st;
  return validity_finish(l, workspace, algo == CTD_NCC_FAST, 4, in0, in1, in1_frame_stride, idx, flags, idx_r, gap, frames,
                         H, W, D, block_size, 0.f, lr_tol, min_gap, hs);
}

static bool costvol_validity_algo_ok(int frames, int D, int bs, int algo) {
  return algo == CTD_NCC_FAST ? validity_block_fast(bs) : (long)frames * D <= 65535;   // (the grid of ctd_costvol_f32)
}

size_t ctd_costvol_validity_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int algo,
                                            int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || frames == 0 || type < 0 || type > 3 ||
      (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST))
    return 0;
  if (!match_validity_supported(frames, H, W) || !costvol_validity_algo_ok(frames, D, block_size, algo)) return 0;
  const size_t inner = algo == CTD_NCC_FAST ? ctd_costvol_workspace_bytes(frames, H, W, D, block_size, type, per_frame_pattern) : 0;
  return validity_layout(frames, H, W, D, inner).bytes;
}

int ctd_costvol_validity_f32(const float* im, const float* pattern, long pattern_frame_stride, const int64_t* idx,
                             uint8_t* flags, int64_t* idx_r, float* gap, int frames, int H, int W, int D, int block_size,
                             int type, float eps, int algo, int lr_tol, float min_gap, void* workspace,
                             size_t workspace_bytes, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || !validity_args_ok(lr_tol, min_gap) ||
      (algo != CTD_NCC_EXACT && algo != CTD_NCC_FAST))
    return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!match_validity_supported(frames, H, W) || !costvol_validity_algo_ok(frames, D, block_size, algo)) return CTD_ERR_UNSUPPORTED;
  const bool fast = algo == CTD_NCC_FAST;
  const size_t inner = fast ? ctd_costvol_workspace_bytes(frames, H, W, D, block_size, type, pattern_frame_stride != 0) : 0;
  const ValidityLayout l = validity_layout(frames, H, W, D, inner);
  if (!workspace || workspace_bytes < l.bytes || ((uintptr_t)workspace & 255)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t hs = (hipStream_t)stream;
  char* ws = (char*)workspace;
  CTD_HIP_TRY(hipMemsetAsync(ws + l.counters, 0, 2 * sizeof(unsigned), hs));
  float* vol = (float*)(ws + l.vol);
  int st = fast ? ctd_costvol_fast_f32(im, pattern, pattern_frame_stride, vol, frames, H, W, D, block_size, type, eps,
                                       inner ? ws + l.inner : nullptr, inner, -1, stream)
                : ctd_costvol_f32(im, pattern, pattern_frame_stride, vol, frames, H, W, D, block_size, type, eps, -1, stream);
  if (st) return st;
  return validity_finish(l, workspace, fast, type, im, pattern, pattern_frame_stride, idx, flags, idx_r, gap, frames, H, W, D,
                         block_size, eps, lr_tol, min_gap, hs);
}

}  // extern "C"
