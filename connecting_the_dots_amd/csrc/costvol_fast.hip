// costvol_fast.hip -- tolerance-level (|a-b| <= 1e-5|b| + 1e-6) SAD / MSE / soft-census cost volumes, f32
// (ctd_costvol_fast_f32), and their ranking instantiations (ctd_costvol_argmin_f32).  Three paths:
//   separable path  costvol_sep.hip           SAD / MSE, block 9, W % 4 == 0, with the caller's workspace: a box filter of
//                                              |P[r][c - d] - I[r][c]| through the all-D pipeline; store only
//   census kernel   costvol_census_kernel     census_mse / census_sad, blocks 3 / 5 / 7 / 9
//   tiled kernel    costvol_fast_kernel       SAD / MSE, blocks 3 / 5 / 7 / 9: whatever the separable path does not take
// The two kernels of this file come in two instantiations each:
//   store    <TYPE, BS, false>   cost[f][d][y][x]                                                 costvol_fast_f32
//   ranking  <TYPE, BS, true>    one Top2 triple per (pixel, kRankChunk disparities), no volume   costvol_rank_f32
// costvol_fast_f32 tries the separable path, then picks the kernel by type; costvol_rank_f32 (the ranking pass of
// costvol_argmin.hip) picks the kernel by type.  Each kernel has one launcher, which owns its grid and its limits.
// The tile (kPTW x kPTH, stage_tile) is ctd_photo_tile.h's.
#include <type_traits>

#include "ctd_dispatch.h"
#include "ctd_internal.h"
#include "ctd_photo_tile.h"
#include "ctd_top2.h"
#include "ctd_validate.h"

namespace ctd {

// ------------------------------------------------------------------------------------------------------
// The tiled kernel: cost[f][d] = photometric_loss(P_d, I) with
// P_d[h][x] = P[h][clamp(x - d)] and the block loss's own replicate-clamped taps, i.e. the pattern tap of
// output (h, x), offset (dy, dx) is P[clamp(h+dy)][clamp(clamp(x+dx) - d)].  64x8 output tiles, the image tile
// and the pattern span of kCvChunk disparities in LDS; a thread keeps 8 disparities x 2 pixels of accumulators
// so that the image-side soft step of a tap is computed once for 8 disparities.
// Built for SAD / MSE only; its TYPE >= 2 arithmetic is the census cost term by term, the statement that
// costvol_census_kernel's transform reproduces.
// ------------------------------------------------------------------------------------------------------
constexpr int kCvChunk = 32, kCvD = 8;
// RANK (the ranking instantiation of ctd_costvol_argmin_f32): the workgroup walks the kRankChunk / kCvChunk chunks of
// one ranking chunk (z = frame * n_chunks + ranking chunk), restaging the pattern span per chunk, keeps a Top2 per
// pixel in registers (each thread owns every disparity of its two pixels: no cross-thread merge) and writes one triple
// per pixel into `top` instead of the costs.  The costs it ranks are the bits the store instantiation writes.
template <int TYPE, int BS, bool RANK = false>
__global__ __launch_bounds__(256) void costvol_fast_kernel(const float* __restrict__ im, const float* __restrict__ pat,
                                                           long pat_frame_stride, float* __restrict__ cost, int H, int W,
                                                           int D, int n_chunks, float eps, Top2Planes top = {}) {
  static_assert(TYPE == 0 || TYPE == 1, "SAD / MSE only: the census types run costvol_census_kernel");
  constexpr int HALF = BS / 2, TW = kPTW + BS - 1, TH = kPTH + BS - 1, SW = TW + kCvChunk - 1;
  constexpr int NSUB = RANK ? kRankChunk / kCvChunk : 1;
  __shared__ float sT[TH][TW], sP[TH][SW];
  const int tx = threadIdx.x & 63, ty0 = threadIdx.x >> 6;
  const int x0 = blockIdx.x * kPTW, y0 = blockIdx.y * kPTH;
  const int f = blockIdx.z / n_chunks, chunk = blockIdx.z - f * n_chunks;
  const long HW = (long)H * W;
  stage_tile<BS>(sT, im + (long)f * HW, H, W, x0, y0);
  Top2 best[2] = {top2_empty(), top2_empty()};
  for (int sub = 0; sub < NSUB; ++sub) {
    const int d0 = (chunk * NSUB + sub) * kCvChunk;
    if (RANK) {
      if (d0 >= D) break;                              // (uniform)
      if (sub) __syncthreads();                        // everybody is done with the previous span
    }
    // span column s of the tile holds pattern column (x0 - HALF - (kCvChunk - 1)) + s - d0, clamped (the second clamp)
    const float* p = pat + (long)f * pat_frame_stride;
    const int span_col0 = x0 - HALF - (kCvChunk - 1) - d0;
    for (int i = threadIdx.x; i < TH * SW; i += 256) {
      const int r = i / SW, c = i - r * SW;
      sP[r][c] = p[(long)clampi(y0 + r - HALF, 0, H - 1) * W + clampi(span_col0 + c, 0, W - 1)];
    }
    __syncthreads();
    const int x = x0 + tx;
    // first clamp of the tap column, tile relative: tap dx of pixel x sits at image column clamp(x + dx - HALF)
    int cx[BS];
#pragma unroll
    for (int dx = 0; dx < BS; ++dx) cx[dx] = clampi(x + dx - HALF, 0, W - 1) - x0 + HALF + (kCvChunk - 1);
    for (int db = 0; db < kCvChunk; db += kCvD) {
      if (d0 + db >= D) break;
      float acc[2][kCvD], ec[2][kCvD], tc[2];
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        tc[k] = sT[ty0 + 4 * k + HALF][tx + HALF];
#pragma unroll
        for (int q = 0; q < kCvD; ++q) {
          acc[k][q] = 0.f;
          ec[k][q] = sP[ty0 + 4 * k + HALF][cx[HALF] - (db + q)];    // centre of P_d: P[y][clamp(x - d)]
        }
      }
#pragma unroll 1
      for (int dy = 0; dy < BS; ++dy)
#pragma unroll
        for (int dx = 0; dx < BS; ++dx)
#pragma unroll
          for (int k = 0; k < 2; ++k) {
            const int ty = ty0 + 4 * k;
            const float t = sT[ty + dy][tx + dx];
            float tb = 0.f;
            if (TYPE >= 2) {
              const float dta = t - tc[k];
              tb = dta * __builtin_amdgcn_rsqf(fmaf(dta, dta, eps));
            }
            const float* row = &sP[ty + dy][cx[dx] - db];
#pragma unroll
            for (int q = 0; q < kCvD; ++q) {
              const float e = row[-q];
              if (TYPE == 0) {
                const float df = e - t;
                acc[k][q] = fmaf(df, df, acc[k][q]);
              } else if (TYPE == 1) {
                acc[k][q] += fabsf(e - t);
              } else {
                const float des = e - ec[k][q];
                const float d2 = des * __builtin_amdgcn_rsqf(fmaf(des, des, eps)) - tb;   // 2 * (h(des) - h(dta))
                if (TYPE == 2) acc[k][q] = fmaf(d2, d2, acc[k][q]);
                else acc[k][q] += fabsf(d2);
              }
            }
          }
      const float scale = (TYPE == 2 ? 0.25f : (TYPE == 3 ? 0.5f : 1.f)) / (float)(BS * BS);
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int y = y0 + ty0 + 4 * k;
        if (x < W && y < H) {
#pragma unroll
          for (int q = 0; q < kCvD; ++q) {
            const int d = d0 + db + q;
            if constexpr (RANK) {
              if (d < D) top2_push(best[k], acc[k][q] * scale, d);           // ascending d
            } else {
              if (d < D) cost[((long)f * D + d) * HW + (long)y * W + x] = acc[k][q] * scale;
            }
          }
        }
      }
    }
  }
  if constexpr (RANK) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int x = x0 + tx, y = y0 + ty0 + 4 * k;
      if (x < W && y < H) top2_store(top, ((long)f * n_chunks + chunk) * HW + (long)y * W + x, best[k]);
    }
  }
}

// ------------------------------------------------------------------------------------------------------
// Census TRANSFORM cost volume (types 2 / 3): the soft census term of a tap, h(P_d[tap] - P_d[centre]), does not
// depend on d away from the right image border -- with x' = x - d it is the pattern's own census value
//     CP(y, x'; dy, dx) = h(P[clamp(y+dy)][clamp(x'+dx)] - P[y][clamp(x')])        (x' may be negative: both clamps apply)
// so it is evaluated once per pattern column and tap, not once per output and tap (the v_rsq_f32 leaves the disparity
// loop: 81 per PATTERN PIXEL instead of 81 per output, D = 128..256 times fewer), and likewise CI(y, x; dy, dx) once
// per image pixel.  Per tap the workgroup stages CI for its 64 x 2 pixels and CP for the 64 + 127 pattern columns its
// 128 disparities reach (2 evaluations per thread and tap, three taps per barrier), then every thread accumulates its
// 4 pixels x 16 disparities:
//   census_sad: the values are staged as 24-bit FIXED POINT, u = round((t + 1) * 2^23) with t = des * rsq(des^2 + eps) in
//     (-1, 1), and one v_sad_u32 per output and tap does |u_p - u_i| + acc (exact integer sum, 81 * 2^24 < 2^32; the
//     rounding of a staged value is 2^-24, that of an f32 t 3e-8: the same accuracy);
//   census_mse: staged as floats, one subtract and one fma per output and tap.
// Only the HALF right-most image columns differ (there the tap column is clamped to W-1 BEFORE the shift by d, so the
// term does depend on d): the workgroups of the last tile column recompute those outputs term by term afterwards.
// Reference: torchext/ext/ext.h:244-259 (per-tap soft census), composition rule of SURVEY 8a/A6.
// ------------------------------------------------------------------------------------------------------
constexpr int kCcW = 64, kCcR = 2, kCcD = 128, kCcDT = 16;   // pixel tile, disparities per workgroup / per thread
constexpr int kCcTaps = 3;                                    // taps staged per barrier

__device__ inline unsigned sad_u32(unsigned a, unsigned b, unsigned acc) {   // |a - b| + acc in one VALU instruction (no builtin)
  unsigned r;
  asm("v_sad_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
  return r;
}

// RANK (the ranking instantiation of ctd_costvol_argmin_f32): the epilogue reduces instead of storing.  Each thread
// folds its 16 disparities of each of its 4 pixels into a Top2, the two half-waves that share the pixels merge through
// a lane swap (lane ^ 32: the lower disparities sit in the lower half), the four wavefronts through LDS; the right-most
// columns' recomputed costs go to LDS and are folded in last.  One triple per (pixel, 128 disparities) leaves for `top`.
template <int TYPE, int BS, bool RANK = false>
__global__ __launch_bounds__(256) void costvol_census_kernel(const float* __restrict__ im, const float* __restrict__ pat,
                                                             long pat_frame_stride, float* __restrict__ cost, int H, int W,
                                                             int D, int n_chunks, float eps, Top2Planes top = {}) {
  static_assert(kCcD == kRankChunk, "one ranking chunk per workgroup");
  static_assert(TYPE == 2 || TYPE == 3, "census types only");
  constexpr int HALF = BS / 2, TH = kCcR + BS - 1, TW = kCcW + BS - 1;
  constexpr int CPW = kCcW + kCcD;                  // staged pattern census columns j = x' - xp0, j in [0, CPW)
  constexpr int SPW = CPW + BS - 1;                 // raw pattern span: column xp0 - HALF + s
  typedef typename std::conditional<TYPE == 3, unsigned, float>::type cen_t;
  __shared__ float sI[TH][TW];
  __shared__ float sP[TH][SPW];
  constexpr int TS = kCcTaps;                       // taps staged per barrier
  __shared__ __attribute__((aligned(16))) cen_t cI[2][TS][kCcR][kCcW];
  __shared__ __attribute__((aligned(16))) cen_t cP[2][TS][kCcR][CPW];
  const int t = threadIdx.x;
  const int x0 = blockIdx.x * kCcW, y0 = blockIdx.y * kCcR;
  const int f = blockIdx.z / n_chunks, d0 = (blockIdx.z - f * n_chunks) * kCcD;
  const long HW = (long)H * W;
  const float* ip = im + (long)f * HW;
  const float* pp = pat + (long)f * pat_frame_stride;
  const int xp0 = x0 - d0 - kCcD;                   // pattern column of census slot 0 (may be negative)
  // raw tiles, both clamps baked in: image columns clamp(x0 - HALF + c), pattern columns clamp(xp0 - HALF + s)
  for (int i0 = t; i0 < TH * TW; i0 += 256 * 4) {
    float v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int i = min(i0 + 256 * u, TH * TW - 1);
      const int r = i / TW, c = i - r * TW;
      v[u] = ip[(long)clampi(y0 + r - HALF, 0, H - 1) * W + clampi(x0 + c - HALF, 0, W - 1)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i0 + 256 * u < TH * TW) (&sI[0][0])[i0 + 256 * u] = v[u];
  }
  for (int i0 = t; i0 < TH * SPW; i0 += 256 * 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = min(i0 + 256 * u, TH * SPW - 1);
      const int r = i / SPW, c = i - r * SPW;
      v[u] = pp[(long)clampi(y0 + r - HALF, 0, H - 1) * W + clampi(xp0 + c - HALF, 0, W - 1)];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u)
      if (i0 + 256 * u < TH * SPW) (&sP[0][0])[i0 + 256 * u] = v[u];
  }
  // this thread's outputs: pixel quad q of row `row`, disparities d0 + 16 g + k
  const int q = t & 15, row = (t >> 4) & 1, g = t >> 5;
  const int jb = 4 * q - kCcDT * g + kCcD - kCcDT;  // first staged pattern column of its five quads (multiple of 4)
  // its two census evaluations per tap: element e = t and t + 256 of [image 2 x 64 | pattern 2 x CPW]
  constexpr int NI = kCcR * kCcW;
  static_assert(NI + kCcR * CPW == 512, "two staged census values per thread and tap");
  typename std::conditional<TYPE == 3, unsigned, float>::type acc[4][kCcDT];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < kCcDT; ++k) acc[i][k] = 0;
  __syncthreads();
  // centre values of the two elements (tap independent) and their tile coordinates
  const bool e0_img = t < NI;                       // (NI = 128: the first two wavefronts; wave-uniform)
  const int e0r = e0_img ? t / kCcW : (t - NI) / CPW, e0c = e0_img ? t % kCcW : (t - NI) % CPW;
  const int e1 = t + 256 - NI, e1r = e1 / CPW, e1c = e1 % CPW;
  const float c0 = e0_img ? sI[e0r + HALF][e0c + HALF] : sP[e0r + HALF][e0c + HALF];
  const float c1 = sP[e1r + HALF][e1c + HALF];
  auto soft = [&](float des) -> cen_t {
    const float tt = des * __builtin_amdgcn_rsqf(fmaf(des, des, eps));      // 2 h(des) - 1, in (-1, 1)
    if constexpr (TYPE == 3) return (unsigned)fmaf(tt, 8388608.f, 8388608.5f);   // round((tt + 1) * 2^23)
    else return tt;
  };
  int buf = 0;
  // taps in groups of TS per barrier (81 = 27 x 3 for block 9; a last partial group stages and accumulates fewer):
  // one barrier per group -- a thread that writes buffer b for group n + 2 has passed the barrier of group n + 1, i.e.
  // everybody finished reading group n
#pragma unroll 1
  for (int tap0 = 0; tap0 < BS * BS; tap0 += TS) {
#pragma unroll
    for (int u = 0; u < TS; ++u) {
      const int tap = tap0 + u;
      if (tap < BS * BS) {                           // (uniform)
        const int dy = tap / BS, dx = tap - dy * BS;
        const float v0 = e0_img ? sI[e0r + dy][e0c + dx] : sP[e0r + dy][e0c + dx];
        const float v1 = sP[e1r + dy][e1c + dx];
        if (e0_img) cI[buf][u][e0r][e0c] = soft(v0 - c0);
        else cP[buf][u][e0r][e0c] = soft(v0 - c0);
        cP[buf][u][e1r][e1c] = soft(v1 - c1);
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < TS; ++u) {
      if (tap0 + u >= BS * BS) break;
      typedef cen_t c4 __attribute__((ext_vector_type(4)));
      const c4 ci = *(const c4*)&cI[buf][u][row][4 * q];
      cen_t cp[20];
#pragma unroll
      for (int m = 0; m < 5; ++m) {
        const c4 w4 = *(const c4*)&cP[buf][u][row][jb + 4 * m];
        cp[4 * m] = w4[0]; cp[4 * m + 1] = w4[1]; cp[4 * m + 2] = w4[2]; cp[4 * m + 3] = w4[3];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int k = 0; k < kCcDT; ++k) {
          if constexpr (TYPE == 3) {
            acc[i][k] = sad_u32(cp[i - k + kCcDT], ci[i], acc[i][k]);                    // |u_p - u_i| + acc
          } else {
            const float d2 = cp[i - k + kCcDT] - ci[i];
            acc[i][k] = fmaf(d2, d2, acc[i][k]);
          }
        }
    }
    buf ^= 1;
  }
  // 2 (h_p - h_i) = t_p - t_i: census_sad 0.5 / bs^2 (and 2^-23 for the fixed point), census_mse 0.25 / bs^2
  const float scale = TYPE == 3 ? 0.5f / (float)(BS * BS) / 8388608.f : 0.25f / (float)(BS * BS);
  const int y = y0 + row, xq = x0 + 4 * q;
  const int x_last_plain = W - 1 - (BS - 1 - HALF);  // right of it the first clamp makes the term depend on d
  if constexpr (!RANK) {
    if (y < H) {
#pragma unroll
      for (int k = 0; k < kCcDT; ++k) {
        const int d = d0 + kCcDT * g + k;
        if (d >= D) break;
        float* o = cost + ((long)f * D + d) * HW + (long)y * W + xq;
        if (xq + 3 <= x_last_plain && (W & 3) == 0 && ((uintptr_t)cost & 15) == 0) {
          typedef float f4 __attribute__((ext_vector_type(4)));
          *(f4*)o = f4{(float)acc[0][k] * scale, (float)acc[1][k] * scale, (float)acc[2][k] * scale, (float)acc[3][k] * scale};
        } else {
#pragma unroll
          for (int i = 0; i < 4; ++i)
            if (xq + i <= x_last_plain) o[i] = (float)acc[i][k] * scale;
        }
      }
    }
  }
  constexpr int NBMAX = HALF > 0 ? HALF : 1;          // right-most columns a tile can hold (BS - 1 - HALF = HALF)
  __shared__ Top2 red[RANK ? 4 : 1][kCcR][kCcW];
  __shared__ float bord[RANK ? kCcD : 1][kCcR][NBMAX];
  if constexpr (RANK) {
    Top2 tp[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      tp[i] = top2_empty();
      const bool plain = y < H && xq + i <= x_last_plain;
#pragma unroll
      for (int k = 0; k < kCcDT; ++k) {
        const int d = d0 + kCcDT * g + k;
        if (plain && d < D) top2_push(tp[i], (float)acc[i][k] * scale, d);   // the bits the store writes, ascending d
      }
      Top2 o;
      o.b1 = __shfl_xor(tp[i].b1, 32);
      o.i1 = __shfl_xor(tp[i].i1, 32);
      o.b2 = __shfl_xor(tp[i].b2, 32);
      tp[i] = top2_merge(tp[i], o);
    }
    if ((t & 32) == 0) {
#pragma unroll
      for (int i = 0; i < 4; ++i) red[t >> 6][row][4 * q + i] = tp[i];
    }
  }
  // the right-most columns, term by term (ext.h:244-259 order of clamps: tap column first, shift second): the
  // workgroup's threads share them, pixel fastest
  const int xb0 = max(x0, x_last_plain + 1), nb = min(x0 + kCcW, W) - xb0;
  if (nb > 0) {
    const int nd = min(kCcD, D - d0);
    for (int o = t; o < nb * kCcR * nd; o += 256) {
      const int px = o % nb, r = (o / nb) % kCcR, dd = o / (nb * kCcR);
      const int x = xb0 + px, yy = y0 + r, d = d0 + dd;
      if (yy >= H) continue;
      // (span slots are addressed by the UNCLAMPED column, x - d >= xp0 + 1: the staged values carry the clamp)
      const float ec = sP[r + HALF][x - d - xp0 + HALF];
      const float tc = sI[r + HALF][x - x0 + HALF];
      float a = 0.f;
      for (int dy = 0; dy < BS; ++dy)
#pragma unroll
        for (int dx = 0; dx < BS; ++dx) {
          const int cw = min(x + dx - HALF, W - 1);                          // first clamp (x + dx - HALF >= 0 here)
          const float e = sP[r + dy][cw - d - xp0 + HALF];
          const float des = e - ec, dta = sI[r + dy][x - x0 + dx] - tc;
          const float d2 = des * __builtin_amdgcn_rsqf(fmaf(des, des, eps)) - dta * __builtin_amdgcn_rsqf(fmaf(dta, dta, eps));
          a = TYPE == 2 ? fmaf(d2, d2, a) : a + fabsf(d2);
        }
      const float v = a * ((TYPE == 2 ? 0.25f : 0.5f) / (float)(BS * BS));
      if constexpr (RANK) bord[dd][r][px] = v;
      else cost[((long)f * D + d) * HW + (long)yy * W + x] = v;
    }
  }
  if constexpr (RANK) {
    __syncthreads();
    if (t < kCcR * kCcW) {
      const int r = t >> 6, c = t & 63, x = x0 + c, yy = y0 + r;
      if (x < W && yy < H) {
        Top2 m = red[0][r][c];
#pragma unroll
        for (int w = 1; w < 4; ++w) m = top2_merge(m, red[w][r][c]);
        if (x >= xb0) {                              // a right-most column: no plain costs were folded in above
          const int nd = min(kCcD, D - d0);
          for (int dd = 0; dd < nd; ++dd) top2_push(m, bord[dd][r][x - xb0], d0 + dd);
        }
        top2_store(top, ((long)f * n_chunks + blockIdx.z % n_chunks) * HW + (long)yy * W + x, m);
      }
    }
  }
}

// The launchers: the store instantiation into `cost`, or, given `top`, the ranking one.  A call that is wrong on two
// counts keeps the status it always had: the tiled launcher checks its grid before the block size, the census one after.
// `type` arrives validated (0..3, by the entry points below and in costvol_argmin.hip); each launcher answers
// CTD_ERR_INVALID_ARG for the other kernel's types.
static int launch_tiled(int bs, int type, const float* im, const float* pat, long pat_frame_stride, float* cost,
                        const Top2Planes* top, int frames, int H, int W, int D, float eps, hipStream_t stream) {
  const int n_chunks = ceil_div(D, top ? kRankChunk : kCvChunk);
  if ((long)frames * n_chunks > 65535) return CTD_ERR_INVALID_ARG;
  const dim3 grid(ceil_div(W, kPTW), ceil_div(H, kPTH), frames * n_chunks);
  return dispatch_block(bs, [&](auto bs_c) {
    return dispatch_type(type, [&](auto type_c) -> int {
      constexpr int BS = decltype(bs_c)::value, TYPE = decltype(type_c)::value;
      if constexpr (TYPE < 2) {
        if (top)
          hipLaunchKernelGGL((costvol_fast_kernel<TYPE, BS, true>), grid, dim3(256), 0, stream, im, pat, pat_frame_stride,
                             nullptr, H, W, D, n_chunks, eps, *top);
        else
          hipLaunchKernelGGL((costvol_fast_kernel<TYPE, BS, false>), grid, dim3(256), 0, stream, im, pat, pat_frame_stride,
                             cost, H, W, D, n_chunks, eps);
        CTD_LAUNCH_CHECK();
        return CTD_OK;
      } else {
        return CTD_ERR_INVALID_ARG;
      }
    });
  });
}

static int launch_census(int bs, int type, const float* im, const float* pat, long pat_frame_stride, float* cost,
                         const Top2Planes* top, int frames, int H, int W, int D, float eps, hipStream_t stream) {
  const int n_chunks = ceil_div(D, kCcD);
  return dispatch_block(bs, [&](auto bs_c) -> int {
    const dim3 grid(ceil_div(W, kCcW), ceil_div(H, kCcR), frames * n_chunks);
    if (grid.y > 65535 || (long)frames * n_chunks > 65535) return CTD_ERR_INVALID_ARG;
    return dispatch_type(type, [&](auto type_c) -> int {
      constexpr int BS = decltype(bs_c)::value, TYPE = decltype(type_c)::value;
      if constexpr (TYPE >= 2) {
        if (top)
          hipLaunchKernelGGL((costvol_census_kernel<TYPE, BS, true>), grid, dim3(256), 0, stream, im, pat, pat_frame_stride,
                             nullptr, H, W, D, n_chunks, eps, *top);
        else
          hipLaunchKernelGGL((costvol_census_kernel<TYPE, BS, false>), grid, dim3(256), 0, stream, im, pat,
                             pat_frame_stride, cost, H, W, D, n_chunks, eps);
        CTD_LAUNCH_CHECK();
        return CTD_OK;
      } else {
        return CTD_ERR_INVALID_ARG;
      }
    });
  });
}

static int costvol_fast_f32(const float* im, const float* pat, long pat_frame_stride, float* cost, int frames, int H,
                            int W, int D, int bs, int type, float eps, void* workspace, size_t workspace_bytes,
                            hipStream_t stream) {
  // SAD / MSE, block 9: the sum is separable (a replicate-border box filter of |P[r][c - d] - I[r][c]|) -- the all-D
  // pipeline of ncc_alld.hip (costvol_sep.hip), one subtract per output instead of 81; needs the caller's workspace for the padded planes
  if (workspace && costvol_sep_supported(H, W, D, bs, type) && ((uintptr_t)cost) % 16 == 0 &&
      workspace_bytes >= costvol_sep_workspace_bytes(frames, H, W, D, pat_frame_stride != 0))
    return costvol_sep_f32(im, pat, pat_frame_stride, cost, frames, H, W, D, type, workspace, workspace_bytes, stream);
  return (type >= 2 ? launch_census : launch_tiled)(bs, type, im, pat, pat_frame_stride, cost, nullptr, frames, H, W, D, eps,
                                                    stream);
}

// Ranking instantiations of the two volume kernels (ctd_costvol_argmin_f32): one Top2 triple per (pixel, kRankChunk
// disparities) into `top`, no volume.  SAD / MSE run on the LDS-tiled kernel for every block size (the separable
// block-9 path has no ranking mode).
bool costvol_rank_supported(int frames, int H, int W, int D, int bs) {
  if (bs != 3 && bs != 5 && bs != 7 && bs != 9) return false;
  if ((double)frames * H * W >= 4294967296.0) return false;            // u32 flat pixel indices on the work list
  return ceil_div(H, kCcR) <= 65535 && (long)frames * ceil_div(D, kRankChunk) <= 65535;
}

int costvol_rank_f32(const float* im, const float* pat, long pat_frame_stride, const Top2Planes& top, int frames, int H,
                     int W, int D, int bs, int type, float eps, hipStream_t stream) {
  return (type >= 2 ? launch_census : launch_tiled)(bs, type, im, pat, pat_frame_stride, nullptr, &top, frames, H, W, D, eps,
                                                    stream);
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_costvol_workspace_bytes(int frames, int H, int W, int D, int block_size, int type, int per_frame_pattern) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3) return 0;
  if (!costvol_sep_supported(H, W, D, block_size, type)) return 0;          // the other kernels need none
  return costvol_sep_workspace_bytes(frames, H, W, D, per_frame_pattern != 0);
}

int ctd_costvol_fast_f32(const float* im, const float* pattern, long pattern_frame_stride, float* cost, int frames, int H,
                         int W, int D, int block_size, int type, float eps, void* workspace, size_t workspace_bytes,
                         int device, void* stream) {
  if (!vol_shape_ok(frames, 1, H, W, D, block_size) || type < 0 || type > 3 || pattern_frame_stride < 0)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !cost) return CTD_ERR_INVALID_ARG;
  if (pattern_frame_stride != 0 && pattern_frame_stride != (long)H * W) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_fast_f32(im, pattern, pattern_frame_stride, cost, frames, H, W, D, block_size, type, eps, workspace,
                          workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
