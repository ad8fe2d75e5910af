// subpixel.hip -- sub-pixel disparity refinement of an integer matcher index (ctd_xcorrvol_subpixel_f32,
// ctd_costvol_subpixel_f32): a parabola or equiangular fit through the reference-order scores at d-1, d, d+1
// (the rule, word for word: include/ctd_hip.h).
//
// NCC.  The three scores are the bits of ctd_xcorrvol_f32(CTD_NCC_EXACT), i.e. of XCorrVolFunctor, ext.h:120-191.
// Each accumulator there is its own chain in tap order, so parts of it can be computed elsewhere without changing bits:
//   - the quotients x / bs^2 of every frame and pattern sample: one elementwise pass into the workspace;
//   - the pattern half (mu1, then s1), which depends only on the pattern row and the UNCLAMPED window centre
//     x = w - d (ext.h:152 shifts before it clamps), x in [-(D-1), W-1]: one plane per pattern, tabulated once per call
//     or kept from an earlier call (CTD_PATTERN_PREPARED);
//   - the frame half (mu0, then s0) is shared by the three disparities.
// What remains per pixel is three `dot` chains over the same frame taps; the pattern taps of d+1, d, d-1 are columns
// j, j+1, j+2 of one row of bs + 2 samples.
//
// The workspace layout and the kernels of the first two items: ctd_subpixel_ws.h (shared with band_match.hip).
//
// Costs.  costvol_ref_cost (ctd_costvol_ref.h) is the tap loop of ctd_costvol_f32; subpixel_cost3 below walks the taps
// once for the three disparities, with the image-side soft step of the census types (independent of d) computed once
// per tap.  Every cost keeps its own chain and its own per-term operations, so the bits are those of ctd_costvol_f32.
#include "ctd_common.h"
#include "ctd_costvol_ref.h"
#include "ctd_ncc_point.h"
#include "ctd_subpixel_ws.h"
#include "ctd_validate.h"

namespace ctd {

// the rule of include/ctd_hip.h; `maximum`: NCC scores (else costs, a minimum).  Returns the disparity, sets *ok.
__device__ inline float subpixel_fit(float sm, float s0, float sp, bool maximum, int mode, int d, bool* ok) {
  float delta = 0.f;
  bool r;
  if (maximum) {
    if (mode == CTD_SUBPIXEL_PARABOLA) {
      const float den = (sm - s0) + (sp - s0);
      r = den < 0.f;
      delta = 0.5f * ((sm - sp) / den);
    } else if (sp > sm) {
      const float q = s0 - sm;
      r = q > 0.f;
      delta = 0.5f * ((sp - sm) / q);
    } else {
      const float q = s0 - sp;
      r = q > 0.f;
      delta = 0.5f * ((sp - sm) / q);
    }
  } else {
    if (mode == CTD_SUBPIXEL_PARABOLA) {
      const float den = (sm - s0) + (sp - s0);
      r = den > 0.f;
      delta = 0.5f * ((sm - sp) / den);
    } else if (sp < sm) {
      const float q = sm - s0;
      r = q > 0.f;
      delta = 0.5f * ((sm - sp) / q);
    } else {
      const float q = sp - s0;
      r = q > 0.f;
      delta = 0.5f * ((sm - sp) / q);
    }
  }
  *ok = r;
  if (!r) return (float)d;
  delta = delta < -0.5f ? -0.5f : (delta > 0.5f ? 0.5f : delta);   // (a NaN passes, as torch.clamp lets it)
  return (float)d + delta;
}

// thread per pixel; the pattern taps of d+1, d, d-1 in row r are pr[clamp(base + j)], j = bw, bw + 1, bw + 2
template <int BS>
__global__ __launch_bounds__(256) void xcorrvol_subpixel_kernel(const float* __restrict__ in0,
                                                                const float* __restrict__ q0,
                                                                const float* __restrict__ in1,
                                                                const float2* __restrict__ pstat, long in1_frame_stride,
                                                                const int64_t* __restrict__ idx,
                                                                float* __restrict__ disp, uint8_t* __restrict__ refined,
                                                                int frames, int H, int W, int D, int bs_rt, int mode) {
  const int bs = BS ? BS : bs_rt;
  const int half = bs / 2;
  const long HW = (long)H * W;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)frames * HW) return;
  const long f = p / HW, px = p - f * HW;
  const int h = (int)(px / W), w = (int)(px - (long)h * W);
  const int64_t di = idx[p];
  if (di < 0 || di >= D) {                                      // never read with an index outside [0, D)
    disp[p] = __builtin_nanf("");
    if (refined) refined[p] = 0;
    return;
  }
  const int d = (int)di;
  if (d == 0 || d == D - 1) {                                   // a neighbour is missing: not refined
    disp[p] = (float)d;
    if (refined) refined[p] = 0;
    return;
  }
  const float* a = in0 + f * HW;
  const float* aq = q0 + f * HW;
  const float* e = in1 + (in1_frame_stride ? f * HW : 0);
  const long Wo = (long)W + D - 1;
  const float2* ps = pstat + (in1_frame_stride ? f * (long)H * Wo : 0) + (long)h * Wo + (w + D - 1);
  const float2 stp = ps[-(d + 1)], stz = ps[-d], stm = ps[-(d - 1)];

  float mu0 = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
#pragma unroll
    for (int bw = 0; bw < bs; ++bw) mu0 += aq[r + clampi(w + bw - half, 0, W - 1)];
  }
  const int base = w - (d + 1) - half;
  float s0 = 0.f, dotp = 0.f, dotz = 0.f, dotm = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
    if constexpr (BS > 0) {
      float pr[BS + 2];
#pragma unroll
      for (int j = 0; j < BS + 2; ++j) pr[j] = e[r + clampi(base + j, 0, W - 1)];
#pragma unroll
      for (int bw = 0; bw < BS; ++bw) {
        const float v0 = a[r + clampi(w + bw - half, 0, W - 1)] - mu0;
        s0 += v0 * v0;
        dotp += v0 * (pr[bw] - stp.x);
        dotz += v0 * (pr[bw + 1] - stz.x);
        dotm += v0 * (pr[bw + 2] - stm.x);
      }
    } else {
      for (int bw = 0; bw < bs; ++bw) {
        const float v0 = a[r + clampi(w + bw - half, 0, W - 1)] - mu0;
        s0 += v0 * v0;
        dotp += v0 * (e[r + clampi(base + bw, 0, W - 1)] - stp.x);
        dotz += v0 * (e[r + clampi(base + bw + 1, 0, W - 1)] - stz.x);
        dotm += v0 * (e[r + clampi(base + bw + 2, 0, W - 1)] - stm.x);
      }
    }
  }
  // val = 0; val += dot / norm  (ext.h:142, 186)
  float sp = 0.f, sz = 0.f, sm = 0.f;
  sp += dotp / ncc_norm(s0, stp.y);
  sz += dotz / ncc_norm(s0, stz.y);
  sm += dotm / ncc_norm(s0, stm.y);
  bool ok;
  disp[p] = subpixel_fit(sm, sz, sp, true, mode, d, &ok);
  if (refined) refined[p] = ok ? 1 : 0;
}

static int xcorrvol_subpixel_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                                 float* disp, uint8_t* refined, int frames, int H, int W, int D, int bs, int mode,
                                 bool prepared, void* workspace, hipStream_t stream) {
  const bool per_frame = in1_frame_stride != 0;
  const SubpixelLayout l = subpixel_layout(frames, H, W, D, per_frame);
  char* ws = (char*)workspace;
  float* q0 = (float*)(ws + l.q0);
  float* q1 = (float*)(ws + l.q1);
  float2* pstat = (float2*)(ws + l.pstat);
  const long HW = (long)H * W;
  const int P = per_frame ? frames : 1;
  const float bs2 = (float)(bs * bs);
  const long n0 = (long)frames * HW;
  hipLaunchKernelGGL(subpixel_quotient_kernel, dim3((unsigned)((n0 + 255) / 256)), dim3(256), 0, stream, in0, q0, n0,
                     bs2);
  CTD_LAUNCH_CHECK();
  if (!prepared) {
    const int st = subpixel_fill_pattern_planes(in1, q1, pstat, P, H, W, D, bs, stream);
    if (st != CTD_OK) return st;
  }
  const dim3 g((unsigned)((n0 + 255) / 256));
  switch (bs) {
    case 3: hipLaunchKernelGGL(xcorrvol_subpixel_kernel<3>, g, dim3(256), 0, stream, in0, q0, in1, pstat, in1_frame_stride, idx, disp, refined, frames, H, W, D, bs, mode); break;
    case 5: hipLaunchKernelGGL(xcorrvol_subpixel_kernel<5>, g, dim3(256), 0, stream, in0, q0, in1, pstat, in1_frame_stride, idx, disp, refined, frames, H, W, D, bs, mode); break;
    case 7: hipLaunchKernelGGL(xcorrvol_subpixel_kernel<7>, g, dim3(256), 0, stream, in0, q0, in1, pstat, in1_frame_stride, idx, disp, refined, frames, H, W, D, bs, mode); break;
    case 9: hipLaunchKernelGGL(xcorrvol_subpixel_kernel<9>, g, dim3(256), 0, stream, in0, q0, in1, pstat, in1_frame_stride, idx, disp, refined, frames, H, W, D, bs, mode); break;
    default: hipLaunchKernelGGL(xcorrvol_subpixel_kernel<0>, g, dim3(256), 0, stream, in0, q0, in1, pstat, in1_frame_stride, idx, disp, refined, frames, H, W, D, bs, mode); break;
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// costs
// ---------------------------------------------------------------------------------------------------------------------

// costvol_ref_cost<TYPE> at d+1, d, d-1 (outputs cp, c0, cm) in one walk over the taps: per cost the same chain and the
// same per-term operations, so the bits of each are those of costvol_ref_cost
template <int TYPE>
__device__ inline void subpixel_cost3(const float* __restrict__ t, const float* __restrict__ e, int h, int w, int d,
                                      int H, int W, int bs, float eps, float* cp, float* c0, float* cm) {
  const int half = bs / 2;
  const float bs2 = (float)(bs * bs);
  const long hr = (long)h * W;
  const float ecp = e[hr + clampi(w - d - 1, 0, W - 1)];
  const float ec0 = e[hr + clampi(w - d, 0, W - 1)];
  const float ecm = e[hr + clampi(w - d + 1, 0, W - 1)];
  const float tc = t[hr + w];
  float lp = 0.f, l0 = 0.f, lm = 0.f;
  for (int bh = 0; bh < bs; ++bh) {
    const long r = (long)clampi(h + bh - half, 0, H - 1) * W;
    for (int bw = 0; bw < bs; ++bw) {
      const int w0 = clampi(w + bw - half, 0, W - 1);
      const float evp = e[r + clampi(w0 - d - 1, 0, W - 1)];
      const float ev0 = e[r + clampi(w0 - d, 0, W - 1)];
      const float evm = e[r + clampi(w0 - d + 1, 0, W - 1)];
      const float tv = t[r + w0];
      if (TYPE == 0 || TYPE == 1) {
        const float fp = evp - tv, f0 = ev0 - tv, fm = evm - tv;
        if (TYPE == 0) {
          lp += fp * fp / bs2;
          l0 += f0 * f0 / bs2;
          lm += fm * fm / bs2;
        } else {
          lp += fabsf(fp) / bs2;
          l0 += fabsf(f0) / bs2;
          lm += fabsf(fm) / bs2;
        }
      } else {
        const float st = soft_step(tv - tc, eps);              // image side: independent of d
        const float fp = soft_step(evp - ecp, eps) - st;
        const float f0 = soft_step(ev0 - ec0, eps) - st;
        const float fm = soft_step(evm - ecm, eps) - st;
        if (TYPE == 2) {
          lp += fp * fp / bs2;
          l0 += f0 * f0 / bs2;
          lm += fm * fm / bs2;
        } else {
          lp += fabsf(fp) / bs2;
          l0 += fabsf(f0) / bs2;
          lm += fabsf(fm) / bs2;
        }
      }
    }
  }
  *cp = lp;
  *c0 = l0;
  *cm = lm;
}

template <int TYPE>
__global__ __launch_bounds__(256) void costvol_subpixel_kernel(const float* __restrict__ im,
                                                               const float* __restrict__ pat, long pat_frame_stride,
                                                               const int64_t* __restrict__ idx,
                                                               float* __restrict__ disp, uint8_t* __restrict__ refined,
                                                               int frames, int H, int W, int D, int bs, float eps,
                                                               int mode) {
  const long HW = (long)H * W;
  const long p = (long)blockIdx.x * 256 + threadIdx.x;
  if (p >= (long)frames * HW) return;
  const long f = p / HW, px = p - f * HW;
  const int h = (int)(px / W), w = (int)(px - (long)h * W);
  const int64_t di = idx[p];
  if (di < 0 || di >= D) {
    disp[p] = __builtin_nanf("");
    if (refined) refined[p] = 0;
    return;
  }
  const int d = (int)di;
  if (d == 0 || d == D - 1) {
    disp[p] = (float)d;
    if (refined) refined[p] = 0;
    return;
  }
  float cp, c0, cm;
  subpixel_cost3<TYPE>(im + f * HW, pat + f * pat_frame_stride, h, w, d, H, W, bs, eps, &cp, &c0, &cm);
  bool ok;
  disp[p] = subpixel_fit(cm, c0, cp, false, mode, d, &ok);
  if (refined) refined[p] = ok ? 1 : 0;
}

static int costvol_subpixel_f32(const float* im, const float* pat, long pat_frame_stride, const int64_t* idx,
                                float* disp, uint8_t* refined, int frames, int H, int W, int D, int bs, int type,
                                float eps, int mode, hipStream_t stream) {
  const long n = (long)frames * H * W;
  const dim3 g((unsigned)((n + 255) / 256));
  switch (type) {
    case 0: hipLaunchKernelGGL(costvol_subpixel_kernel<0>, g, dim3(256), 0, stream, im, pat, pat_frame_stride, idx, disp, refined, frames, H, W, D, bs, eps, mode); break;
    case 1: hipLaunchKernelGGL(costvol_subpixel_kernel<1>, g, dim3(256), 0, stream, im, pat, pat_frame_stride, idx, disp, refined, frames, H, W, D, bs, eps, mode); break;
    case 2: hipLaunchKernelGGL(costvol_subpixel_kernel<2>, g, dim3(256), 0, stream, im, pat, pat_frame_stride, idx, disp, refined, frames, H, W, D, bs, eps, mode); break;
    default: hipLaunchKernelGGL(costvol_subpixel_kernel<3>, g, dim3(256), 0, stream, im, pat, pat_frame_stride, idx, disp, refined, frames, H, W, D, bs, eps, mode); break;
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_xcorrvol_subpixel_workspace_bytes(int frames, int H, int W, int D, int block_size, int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0) return 0;
  return xcorrvol_subpixel_workspace_bytes(frames, H, W, D, per_frame_pattern != 0);
}

int ctd_xcorrvol_subpixel_f32(const float* in0, const float* in1, long in1_frame_stride, const int64_t* idx,
                              float* disp, uint8_t* refined, int frames, int H, int W, int D, int block_size, int mode,
                              void* workspace, size_t workspace_bytes, int device, void* stream) {
  const bool prepared = (mode & CTD_PATTERN_PREPARED) != 0;
  mode &= ~CTD_PATTERN_PREPARED;
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0 ||
      (mode != CTD_SUBPIXEL_PARABOLA && mode != CTD_SUBPIXEL_EQUIANGULAR))
    return CTD_ERR_INVALID_ARG;
  if (in1_frame_stride != 0 && in1_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !idx || !disp) return CTD_ERR_INVALID_ARG;
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < xcorrvol_subpixel_workspace_bytes(frames, H, W, D, in1_frame_stride != 0))
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return xcorrvol_subpixel_f32(in0, in1, in1_frame_stride, idx, disp, refined, frames, H, W, D, block_size, mode,
                               prepared, workspace, (hipStream_t)stream);
}

int ctd_costvol_subpixel_f32(const float* im, const float* pattern, long pattern_frame_stride, const int64_t* idx,
                             float* disp, uint8_t* refined, int frames, int H, int W, int D, int block_size, int type,
                             float eps, int mode, int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || (block_size & 1) == 0 || type < 0 || type > 3 ||
      (mode != CTD_SUBPIXEL_PARABOLA && mode != CTD_SUBPIXEL_EQUIANGULAR))
    return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !idx || !disp) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_subpixel_f32(im, pattern, pattern_frame_stride, idx, disp, refined, frames, H, W, D, block_size, type,
                              eps, mode, (hipStream_t)stream);
}

}  // extern "C"
