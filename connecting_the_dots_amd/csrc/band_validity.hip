// band_validity.hip -- match validity of the band matchers (ctd_xcorrvol_band_validity_f32,
// ctd_costvol_band_validity_f32): idx and best of band_match.hip plus the pattern-side match idx_r, the uniqueness gap
// and the flag byte, all over what the bands hold, without a volume (the definition, word for word:
// include/ctd_hip_band_validity.h).
//
// The scores the rule needs already sit in the band kernels' registers: ctd_band_score.h scores every candidate (w, d)
// of a band once, in ascending d, and hands it to a sink.  The sink here, BandValid, does three things with a score
// y (costs negated, so that larger is better for both families; the negation is exact):
//   rank      the running (best, first index) of band_match.hip;
//   gap       s2 = the best score over held d with |d - idx| >= 2, from the same sweep in O(1) registers: p0 / p1 are
//             the maxima over d' <= d - 1 / d' <= d - 2 (a prefix maximum lagged by two), `left` is p1 as it stood when
//             the best last changed (everything at least two below the best), `right` the running maximum over
//             d >= best index + 2, reset when the best changes.  s2 = max(left, right); -inf gives gap = +inf;
//   scatter   the key (ord(y + 0.0f) << 32) | (0xFFFFFFFF - d) to column w - d of the row's key array, which is idx_r
//             itself.  ord maps f32 bits to u32 order-preservingly; + 0.0f folds -0.0 into +0.0, so equal scores have
//             equal high words and the low word gives the tie to the smaller d.  A plain 8-byte load first, and only
//             if the key is larger one 64-bit atomicMax (as depth_warp.hip does with atomicMin): most candidates lose
//             against what the column already holds and cost a cached load.  A maximum does not depend on the order of
//             its operands: the same bits on every run.  Key 0 = no candidate (no finite score has ord 0).
//
// Launches, on the caller's stream:
//   1. hipMemsetAsync of idx_r to 0;
//   2. the band kernel with BandValid: writes idx, best, gap and flag bits 0 and 2;
//   3. band_valid_flag_kernel: LR_OK from the raw key at column w - idx (never 0: the pixel's own candidate landed there);
//   4. band_valid_decode_kernel: key -> idx_r in place; a launch of its own, after every gather of 3 has read.
#include "../../include/ctd_hip_band.h"
#include "../../include/ctd_hip_band_validity.h"
#include "ctd_band_score.h"

namespace ctd {

__device__ inline unsigned band_valid_ord(float y) {            // u < v as unsigned  <=>  x < y as floats (no NaNs)
  const unsigned u = __float_as_uint(y);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

template <bool MAXI>
struct BandValid {
  float b, left, right, p0, p1;                  // in the maximising domain
  int bi, w;
  unsigned long long* krow;                      // the keys of this pixel's row
  unsigned long long* keys;

  __device__ inline void open(long row, int w_) {
    const float ninf = -__builtin_inff();
    b = left = right = p0 = p1 = ninf;
    bi = -1;
    w = w_;
    krow = keys + row;
  }
  __device__ inline void take(float s, int d) {
    const float y = MAXI ? s : -s;
    if (bi < 0 || y > b) {
      b = y;
      bi = d;
      left = p1;
      right = -__builtin_inff();
    } else if (d >= bi + 2) {
      right = fmaxf(right, y);
    }
    p1 = p0;
    p0 = fmaxf(p0, y);
    if (w - d >= 0) {                            // (0 <= w - d <= w < W: inside the row)
      const unsigned long long key =
          ((unsigned long long)band_valid_ord(y + 0.0f) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)d);
      unsigned long long* a = krow + (w - d);
      if (key > __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(a, key);
    }
  }
  // idx, best, gap and flag bits 0 and 2 of pixel p
  __device__ inline void store(long p, int64_t* __restrict__ idx, float* __restrict__ best, uint8_t* __restrict__ flags,
                               float* __restrict__ gap, float min_gap) const {
    band_store(idx, best, p, bi, MAXI ? b : -b);
    const float g = bi < 0 ? __builtin_nanf("") : b - fmaxf(left, right);
    gap[p] = g;
    flags[p] = (uint8_t)((bi >= 0 && w - bi >= 0 ? 1 : 0) | (bi >= 0 && g > min_gap ? 4 : 0));
  }
};

template <int BS>
__global__ __launch_bounds__(256) void xcorrvol_band_valid_kernel(
    const float* __restrict__ in0, const float* __restrict__ in1, const float2* __restrict__ pstat, long in1_frame_stride,
    const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int64_t* __restrict__ idx, float* __restrict__ best,
    uint8_t* __restrict__ flags, unsigned long long* keys, float* __restrict__ gap, float min_gap, int H, int W, int D,
    int tiles_x, int tiles_y) {
  BandValid<true> sk;
  sk.keys = keys;
  long p;
  const bool inside = xcorrvol_band_tile<BS>(in0, in1, pstat, in1_frame_stride, lo, hi, H, W, D, tiles_x, tiles_y, sk, p);
  if (inside) sk.store(p, idx, best, flags, gap, min_gap);
}

__global__ __launch_bounds__(256) void xcorrvol_band_valid_rt_kernel(
    const float* __restrict__ in0, const float* __restrict__ in1, const float2* __restrict__ pstat, long in1_frame_stride,
    const int32_t* __restrict__ lo, const int32_t* __restrict__ hi, int64_t* __restrict__ idx, float* __restrict__ best,
    uint8_t* __restrict__ flags, unsigned long long* keys, float* __restrict__ gap, float min_gap, int frames, int H,
    int W, int D, int bs) {
  BandValid<true> sk;
  sk.keys = keys;
  long p;
  const bool inside = xcorrvol_band_rt_pixel(in0, in1, pstat, in1_frame_stride, lo, hi, frames, H, W, D, bs, sk, p);
  if (inside) sk.store(p, idx, best, flags, gap, min_gap);
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void costvol_band_valid_kernel(
    const float* __restrict__ im, const float* __restrict__ pat, long pat_frame_stride, const int32_t* __restrict__ lo,
    const int32_t* __restrict__ hi, int64_t* __restrict__ idx, float* __restrict__ best, uint8_t* __restrict__ flags,
    unsigned long long* keys, float* __restrict__ gap, float min_gap, int frames, int H, int W, int D, int bs_rt,
    float eps, int tiles_x, int tiles_y) {
  BandValid<false> sk;
  sk.keys = keys;
  long p;
  const bool inside = costvol_band_pixel<TYPE, BS>(im, pat, pat_frame_stride, lo, hi, frames, H, W, D, bs_rt, eps, tiles_x,
                                              tiles_y, sk, p);
  if (inside) sk.store(p, idx, best, flags, gap, min_gap);
}

__device__ inline int64_t band_valid_key_disp(unsigned long long key) {
  return (int64_t)(0xFFFFFFFFu - (unsigned)(key & 0xffffffffull));
}

// LR_OK (bit 1): bit 0 holds and |idx_r[f][h][w - idx] - idx| <= lr_tol, on the raw keys
__global__ __launch_bounds__(256) void band_valid_flag_kernel(const int64_t* __restrict__ idx,
                                                              const unsigned long long* __restrict__ keys,
                                                              uint8_t* __restrict__ flags, long P, int lr_tol) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const uint8_t fl = flags[p];
  if (!(fl & 1)) return;                                 // (bit 0: idx >= 0 and w - idx >= 0, the same row)
  const int64_t d = idx[p];
  const int64_t diff = band_valid_key_disp(keys[p - d]) - d;
  if ((diff < 0 ? -diff : diff) <= (int64_t)lr_tol) flags[p] = (uint8_t)(fl | 2);
}

__global__ __launch_bounds__(256) void band_valid_decode_kernel(int64_t* idx_r, long P) {
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const unsigned long long key = (unsigned long long)idx_r[p];
  idx_r[p] = key ? band_valid_key_disp(key) : (int64_t)-1;
}

// launches 3 and 4
static int band_valid_finish(const int64_t* idx, uint8_t* flags, int64_t* idx_r, long P, int lr_tol,
                             hipStream_t stream) {
  const dim3 g((unsigned)((P + 255) / 256));
  hipLaunchKernelGGL(band_valid_flag_kernel, g, dim3(256), 0, stream, idx, (const unsigned long long*)idx_r, flags, P,
                     lr_tol);
  CTD_LAUNCH_CHECK();
  hipLaunchKernelGGL(band_valid_decode_kernel, g, dim3(256), 0, stream, idx_r, P);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int xcorrvol_band_validity_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                      const int32_t* hi, int64_t* idx, float* best, uint8_t* flags, int64_t* idx_r,
                                      float* gap, int frames, int H, int W, int D, int bs, int lr_tol, float min_gap,
                                      bool prepared, void* workspace, hipStream_t stream) {
  const bool per_frame = in1_frame_stride != 0;
  const SubpixelLayout l = subpixel_layout(frames, H, W, D, per_frame);
  char* ws = (char*)workspace;
  float2* pstat = (float2*)(ws + l.pstat);
  if (!prepared) {
    const int st = subpixel_fill_pattern_planes(in1, (float*)(ws + l.q1), pstat, per_frame ? frames : 1, H, W, D, bs,
                                                stream);
    if (st != CTD_OK) return st;
  }
  const long P = (long)frames * H * W;
  unsigned long long* keys = (unsigned long long*)idx_r;
  CTD_HIP_TRY(hipMemsetAsync(idx_r, 0, (size_t)P * sizeof(int64_t), stream));
  const int tiles_x = ceil_div(W, kBandTW), tiles_y = ceil_div(H, kBandTH);
  const dim3 g((unsigned)((long)frames * tiles_y * tiles_x));   // <= frames * H * W < 2^31
#define CTD_BAND_VALID_NCC(BS)                                                                                        \
  hipLaunchKernelGGL(xcorrvol_band_valid_kernel<BS>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, \
                     idx, best, flags, keys, gap, min_gap, H, W, D, tiles_x, tiles_y)
  switch (bs) {
    case 3: CTD_BAND_VALID_NCC(3); break;
    case 5: CTD_BAND_VALID_NCC(5); break;
    case 7: CTD_BAND_VALID_NCC(7); break;
    case 9: CTD_BAND_VALID_NCC(9); break;
    default:
      hipLaunchKernelGGL(xcorrvol_band_valid_rt_kernel, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, stream, in0, in1,
                         pstat, in1_frame_stride, lo, hi, idx, best, flags, keys, gap, min_gap, frames, H, W, D, bs);
  }
#undef CTD_BAND_VALID_NCC
  CTD_LAUNCH_CHECK();
  return band_valid_finish(idx, flags, idx_r, P, lr_tol, stream);
}

template <int TYPE>
static void costvol_band_valid_launch(const float* im, const float* pat, long pat_frame_stride, const int32_t* lo,
                                      const int32_t* hi, int64_t* idx, float* best, uint8_t* flags,
                                      unsigned long long* keys, float* gap, float min_gap, int frames, int H, int W, int D,
                                      int bs, float eps, hipStream_t stream) {
  const int tiles_x = ceil_div(W, kBandTW), tiles_y = ceil_div(H, kBandTH);
  const dim3 g((unsigned)((long)frames * tiles_y * tiles_x));   // <= frames * H * W < 2^31
#define CTD_BAND_VALID_COST(BS, GRID)                                                                                 \
  hipLaunchKernelGGL((costvol_band_valid_kernel<TYPE, BS>), GRID, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, \
                     hi, idx, best, flags, keys, gap, min_gap, frames, H, W, D, bs, eps, tiles_x, tiles_y)
  switch (bs) {
    case 3: CTD_BAND_VALID_COST(3, g); break;
    case 5: CTD_BAND_VALID_COST(5, g); break;
    case 7: CTD_BAND_VALID_COST(7, g); break;
    case 9: CTD_BAND_VALID_COST(9, g); break;
    default: {
      const long n = (long)frames * H * W;
      CTD_BAND_VALID_COST(0, dim3((unsigned)((n + 255) / 256)));
    }
  }
#undef CTD_BAND_VALID_COST
}

static int costvol_band_validity_f32(const float* im, const float* pat, long pat_frame_stride, const int32_t* lo,
                                     const int32_t* hi, int64_t* idx, float* best, uint8_t* flags, int64_t* idx_r,
                                     float* gap, int frames, int H, int W, int D, int bs, int type, float eps, int lr_tol,
                                     float min_gap, hipStream_t stream) {
  const long P = (long)frames * H * W;
  unsigned long long* keys = (unsigned long long*)idx_r;
  CTD_HIP_TRY(hipMemsetAsync(idx_r, 0, (size_t)P * sizeof(int64_t), stream));
  switch (type) {
    case 0: costvol_band_valid_launch<0>(im, pat, pat_frame_stride, lo, hi, idx, best, flags, keys, gap, min_gap, frames, H, W, D, bs, eps, stream); break;
    case 1: costvol_band_valid_launch<1>(im, pat, pat_frame_stride, lo, hi, idx, best, flags, keys, gap, min_gap, frames, H, W, D, bs, eps, stream); break;
    case 2: costvol_band_valid_launch<2>(im, pat, pat_frame_stride, lo, hi, idx, best, flags, keys, gap, min_gap, frames, H, W, D, bs, eps, stream); break;
    default: costvol_band_valid_launch<3>(im, pat, pat_frame_stride, lo, hi, idx, best, flags, keys, gap, min_gap, frames, H, W, D, bs, eps, stream); break;
  }
  CTD_LAUNCH_CHECK();
  return band_valid_finish(idx, flags, idx_r, P, lr_tol, stream);
}

static bool band_valid_args_ok(int lr_tol, float min_gap) { return lr_tol >= 0 && min_gap >= 0.f; }   // (a NaN fails >=)

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_xcorrvol_band_validity_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                   const int32_t* hi, int64_t* idx, float* best, uint8_t* flags, int64_t* idx_r,
                                   float* gap, int frames, int H, int W, int D, int block_size, int lr_tol, float min_gap,
                                   int flags_prepared, void* workspace, size_t workspace_bytes, int device,
                                   void* stream) {
  if (!band_shape_ok(frames, H, W, D, block_size, in1_frame_stride) || (flags_prepared & ~CTD_PATTERN_PREPARED) != 0)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !lo || !hi || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!band_valid_args_ok(lr_tol, min_gap)) return CTD_ERR_INVALID_ARG;
  if ((double)frames * H * W >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < xcorrvol_subpixel_workspace_bytes(frames, H, W, D, in1_frame_stride != 0))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return xcorrvol_band_validity_f32(in0, in1, in1_frame_stride, lo, hi, idx, best, flags, idx_r, gap, frames, H, W, D,
                                    block_size, lr_tol, min_gap, (flags_prepared & CTD_PATTERN_PREPARED) != 0, workspace,
                                    (hipStream_t)stream);
}

int ctd_costvol_band_validity_f32(const float* im, const float* pattern, long pattern_frame_stride, const int32_t* lo,
                                  const int32_t* hi, int64_t* idx, float* best, uint8_t* flags, int64_t* idx_r,
                                  float* gap, int frames, int H, int W, int D, int block_size, int type, float eps,
                                  int lr_tol, float min_gap, int device, void* stream) {
  if (!band_shape_ok(frames, H, W, D, block_size, pattern_frame_stride) || type < 0 || type > 3)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !lo || !hi || !idx || !flags || !idx_r || !gap) return CTD_ERR_INVALID_ARG;
  if (!band_valid_args_ok(lr_tol, min_gap)) return CTD_ERR_INVALID_ARG;
  if ((double)frames * H * W >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_band_validity_f32(im, pattern, pattern_frame_stride, lo, hi, idx, best, flags, idx_r, gap, frames, H, W,
                                   D, block_size, type, eps, lr_tol, min_gap, (hipStream_t)stream);
}

}  // extern "C"
