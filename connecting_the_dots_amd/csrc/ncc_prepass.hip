// ncc_prepass.hip -- window-statistics pre-pass of the fast NCC path (the stages of a call: ncc_fast.hip).
#include <type_traits>

#include "ctd_ncc_fast.h"
#include "ctd_prepass.h"

namespace ctd {

// ------------------------------------------------------------------------------------
// pre-pass: (mean, sqrt(sum of squared deviations)) of the clamped bs x bs window centred
// at the unclamped column x = xi + x_start, separable f64 sums through LDS.
// ------------------------------------------------------------------------------------
#ifndef CTD_PRE_TW
// (A/B of the f32 kernel, tools/ab_tail.sh, frames only: 64 x 16 24.6 us, 64 x 12 25.3, 64 x 24 26.1, 32 x 24 26.7, 32 x 32 27.6,
// 32 x 16 28.2, 128 x 16 28.3, 64 x 32 28.8, 128 x 8 30.0; the f64 kernel of rounds 1-3 preferred 32 x 24)
#define CTD_PRE_TW 64
#define CTD_PRE_TH 16
#endif
constexpr int kSTW = CTD_PRE_TW, kSTH = CTD_PRE_TH, kSRows = 256 / CTD_PRE_TW;   // (A/B, rocprofv3, with the pattern job: 64 x 16: 36.9 us, 32 x 32: 35.1, 32 x 24: 34.0, 32 x 16: 37.1, 32 x 48: 39.4)
// kDevFloor, kFlagRatio (the listing rule's two constants): ctd_prepass.h
#ifndef CTD_PREPASS_F32
#define CTD_PREPASS_F32 1
#endif
constexpr bool kPrepassF32 = CTD_PREPASS_F32 != 0;   // block 9: f32 window sums on centred samples (see ncc_prepass_kernel)

// (PrepassJob, and what the planes it fills hold: ctd_ncc_fast.h)

// BSC > 0: compile-time block size (tap loops unrolled); BSC == 0: run-time `bs_rt`
// F32 (round 4, block 9): the window sums in f32 on samples CENTRED by the image's constant (the planes hold centred
// values anyway): sum of squared deviations = s2' - s1' * mean', whose relative error is ~F * 2^-24 * (number of
// roundings) with F = s2' / var = 1 + n (mean - centring)^2 / var -- the very factor the listing rule bounds by 1 + kFlagRatio
// (windows above it are recomputed by the fix-up pass), so unlisted windows keep their reciprocal deviation to ~1e-6
// relative, well inside the fast path's error budget; the raw mean for the flat-window test is mean' + centring.  Half the
// LDS, no f32 -> f64 conversions, full-rate additions.
template <int BSC, bool F32 = false>
__global__ __launch_bounds__(kSTW* kSRows) void ncc_prepass_kernel(PrepassJob ja, PrepassJob jb, int H, int W, int bs_rt,
                                                                   unsigned* __restrict__ clear_counters, int n_clear) {
  // the work-list counters of a ranked call (first used two kernels later): cleared here instead of by a memset launch
  if (clear_counters && blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && (int)(threadIdx.y * kSTW + threadIdx.x) < n_clear)
    clear_counters[(threadIdx.y * kSTW + threadIdx.x) * kWorkListStride] = 0u;
  const bool is_a = (int)blockIdx.z < ja.nimg;
  const PrepassJob& jp = is_a ? ja : jb;
  const int img_idx = is_a ? (int)blockIdx.z : (int)blockIdx.z - ja.nimg;
  const float* __restrict__ in = jp.in;
  const long frame_stride = jp.frame_stride;
  float* __restrict__ out_img = jp.out_img;
  float* __restrict__ out_mean = jp.out_mean;
  float* __restrict__ out_dev = jp.out_dev;
  const int x_start = jp.x_start, W_out = jp.W_out, col_lo = jp.col_lo, col_hi = jp.col_hi;
  unsigned* __restrict__ n_flag = jp.n_flag;
  unsigned long long* __restrict__ flag_list = jp.flag_list;
  unsigned* __restrict__ n_runs = jp.n_runs;
  unsigned long long* __restrict__ run_rows = jp.run_rows;
  if ((int)blockIdx.x * kSTW >= W_out) return;
  extern __shared__ double lds_d[];
  __shared__ double cred[1];
  typedef typename std::conditional<F32, float, double>::type acc_t;
  const int bs = BSC > 0 ? BSC : bs_rt;
  const int half = bs / 2;
  const int TRr = kSTH + bs - 1, TCc = kSTW + bs - 1;
  acc_t* rs1 = (acc_t*)lds_d;
  acc_t* rs2 = rs1 + TRr * kSTW;
  float* tile = (float*)(rs2 + TRr * kSTW);
  const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kSTW + tx;
  const int xi_lo = blockIdx.x * kSTW, h_lo = blockIdx.y * kSTH;
  const float* img = in + (long)img_idx * frame_stride;          // image = frame * C + channel
  // centring constant of the image = mean of its centre window: the first wavefront sums it with a fixed shuffle
  // butterfly (the same bits in every workgroup), everyone else goes straight to the staging loads
  if (tid < 64) {
    double t = 0;
    for (int k = tid; k < bs * bs; k += 64) {
      int hh = clampi(H / 2 + k / bs - half, 0, H - 1), ww = clampi(W / 2 + k % bs - half, 0, W - 1);
      t += (double)img[(long)hh * W + ww];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
    if (tid == 0) cred[0] = t;
  }
  // batches of independent loads: one memory round trip per 8 elements of a thread instead of one each
  for (int i0 = tid; i0 < TRr * TCc; i0 += kSTW * kSRows * 8) {
    float t[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = min(i0 + kSTW * kSRows * u, TRr * TCc - 1);
      const int r = i / TCc, c = i - r * TCc;
      const int hh = clampi(h_lo + r - half, 0, H - 1);
      const int ww = clampi(xi_lo + x_start + c - half, 0, W - 1);
      t[u] = img[(long)hh * W + ww];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + kSTW * kSRows * u < TRr * TCc) tile[i0 + kSTW * kSRows * u] = t[u];
  }
  __syncthreads();
  const double n = (double)(bs * bs), inv_n = 1.0 / n;
  const float cval = (float)(cred[0] / n);
  const acc_t shift = F32 ? (acc_t)cval : (acc_t)0;                // F32: sums of the centred samples
  for (int r = ty; r < TRr; r += kSRows) {
    const float* row = tile + r * TCc + tx;
    acc_t s1 = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < BSC; ++k) {
      acc_t v = (acc_t)row[k] - shift;
      s1 += v;
      s2 += v * v;
    }
    if (BSC == 0)
      for (int k = 0; k < bs; ++k) {
        acc_t v = (acc_t)row[k] - shift;
        s1 += v;
        s2 += v * v;
      }
    rs1[r * kSTW + tx] = s1;
    rs2[r * kSTW + tx] = s2;
  }
  __syncthreads();
  const int xi = xi_lo + tx;
  for (int r = ty; r < kSTH; r += kSRows) {
    const int h = h_lo + r;
    if (xi >= W_out || h >= H) continue;
    acc_t a1 = 0, a2 = 0;
#pragma unroll
    for (int k = 0; k < BSC; ++k) {
      a1 += rs1[(r + k) * kSTW + tx];
      a2 += rs2[(r + k) * kSTW + tx];
    }
    if (BSC == 0)
      for (int k = 0; k < bs; ++k) {
        a1 += rs1[(r + k) * kSTW + tx];
        a2 += rs2[(r + k) * kSTW + tx];
      }
    // F32: a1, a2 are sums of centred samples -- mean = centred mean + centring, var is shift-invariant
    const double s1 = (double)a1, s2 = (double)a2;
    const double mean_c = F32 ? (double)(a1 * (acc_t)inv_n) : s1 * inv_n;     // mean of the summed samples
    double var = F32 ? (double)(a2 - a1 * (acc_t)mean_c) : s2 - s1 * mean_c;  // sum of squared deviations (sigma of ext.h:180-181)
    const double mean = F32 ? mean_c + (double)cval : mean_c;
    // Windows whose outputs the fast kernel cannot deliver within tolerance are listed for ncc_fixup_kernel
    // (see there), which recomputes EVERY output they take part in:
    //  * deviation small against the offset from the centring constant: cov = S_ab - n*ma*mb cancels in f32;
    //  * (nearly) flat window, rms deviation below 6.3e-4 of its mean (kFlatRatio): the reference's own value is then decided by
    //    the rounding of its mean (ext.h:157-158) and only the same operation order reproduces it; or deviation
    //    below kDevFloor, where the 1e-8 of the reference's denominator stops being a small correction.
    // A listed window's reciprocal deviation is stored as 0: the fast kernels then produce the placeholder score 0 for
    // exactly the outputs the fix-up pass overwrites (finite, so the in-kernel ranking's integer keys stay ordered;
    // what the ranking does about placeholders: see the all-D kernel).
    const double mc = F32 ? mean_c : mean - (double)cval;
    const bool flat = kFlatRatio * n * mean * mean > var || var < kDevFloor * kDevFloor;
    const bool listed = flat || n * mc * mc > jp.flag_ratio * var;
    // reciprocal deviation (see ncc_inv_norm): v_rsq_f32 and one Newton step in f32, 1e-7 relative -- the f64 square
    // root and the two f64 divisions this line and `mean` used to cost were 60 % of the kernel's instructions
    const float vf = (float)(var > 0 ? var : 1.0);
    float rdev = __builtin_amdgcn_rsqf(vf);
    rdev = fmaf(0.5f * rdev, fmaf(-vf * rdev, rdev, 1.f), rdev);
    const long o = ((long)img_idx * H + h) * jp.pitch + jp.o_off + xi;
    const int col = xi + x_start;
    out_mean[o] = (float)(jp.mean_scale * mc);
    out_dev[o] = listed ? 0.f : rdev;
    const float centred = tile[(r + half) * TCc + tx + half] - cval;
    out_img[o] = centred;
    if (jp.halo > 0) {
      if (xi == 0)
        for (int k = 1; k <= jp.halo; ++k) out_img[o - k] = centred;
      if (xi == W_out - 1)
        for (int k = 1; k <= jp.halo; ++k) out_img[o + k] = centred;
    }
    if (listed && col >= col_lo && col < col_hi) {
      flag_list[atomicAdd(n_flag, 1u)] = ((unsigned long long)img_idx << 40) | ((unsigned long long)h << 20) |
                                         (unsigned long long)(col + 0x80000);
      if (run_rows && col == col_lo) run_rows[atomicAdd(n_runs, 1u)] = ((unsigned long long)img_idx << 20) | (unsigned long long)h;
    }
  }
}

int launch_prepass(const PrepassJob& ja, const PrepassJob& jb, int H, int W, int bs, const WorkList* work,
                          hipStream_t stream) {
  const int TRr = kSTH + bs - 1, TCc = kSTW + bs - 1;
  const bool f32 = bs == 9 && kPrepassF32;
  size_t lds = (f32 ? sizeof(float) : sizeof(double)) * 2 * TRr * kSTW + sizeof(float) * (size_t)TRr * TCc;
  if (lds > 60 * 1024) return CTD_ERR_UNSUPPORTED;
  const int w_out = jb.nimg == 0 ? ja.W_out : (ja.nimg == 0 || jb.W_out > ja.W_out ? jb.W_out : ja.W_out);
  dim3 grid(ceil_div(w_out, kSTW), ceil_div(H, kSTH), ja.nimg + jb.nimg), block(kSTW, kSRows);
  auto kern = ncc_prepass_kernel<0, false>;
  if (bs == 9) kern = f32 ? ncc_prepass_kernel<9, true> : ncc_prepass_kernel<9, false>;
  hipLaunchKernelGGL(kern, grid, block, lds, stream, ja, jb, H, W, bs, work ? work->counters : nullptr, work ? work->parts : 0);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd
