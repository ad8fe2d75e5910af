// ncc_tiles.hip -- zero-mean NCC block-matching volume, separable window sums (CTD_NCC_FAST): the kernels that
// work by disparity GROUPS -- narrow, wide and tile-256 (the all-D kernel: ncc_alld.hip; the stages of a call: ncc_fast.hip).
//
// Same op as ncc_exact.hip (XCorrVolFunctor, torchext/ext/ext.h:120-191) but evaluated as
//     NCC = (S_ab - n*ma*mb) / (sa*sb + 1e-8),   S_ab = sum over the bs x bs window of a*b
// so that each output costs ~20 VALU slots instead of >= 243 and the kernel is bound by
// the 4 B/output volume store (HBM roofline).  Results agree with the reference order
// to |a-b| <= 1e-5*|b| + 1e-6 (C > 1: the sum of that bound over the channels' NCCs, see the error model above
// ncc_fixup_kernel), not bit for bit; bit-exact indices come from the re-rank in ctd_xcorrvol_argmax_f32.
//
// Work decomposition (one wavefront = 64 product columns, 4 disparities per lane):
//   * a workgroup is 4 consumer wavefronts (16 adjacent disparities of one column tile)
//     plus 1 LOADER wavefront.  The loader streams each row's operands (frame sample,
//     pattern span, window statistics) global -> LDS with LDS-DMA, a few rows ahead, and
//     is the only wave that ever waits on a load.  Consumers touch global memory only to
//     store: on gfx950 loads and stores retire in order on one counter (vmcnt), so a wave
//     that both loads and stores stalls on its own stores' HBM latency every row;
//   * consumer lane l owns the UNCLAMPED product column w0 = w_lo - HALF + l and marches
//     down the rows of a band.  Per row it forms p = a'(r,w0) * b'(r,w0-d) for its ND
//     disparities;
//   * vertical bs-sum of p: registers only, as a 3+3+3 tree over a ring of past rows
//     (no running sums, so no drift: every output is a fresh <= 4-level sum);
//   * horizontal bs-sum across lanes: +-1 with DPP wave shifts, +-3 with ds_bpermute;
//     64-(bs-1) of the 64 lanes produce outputs, stored as one contiguous row segment;
//   * a', b' are the inputs minus one constant per image (the window mean at the image
//     centre): an exact-arithmetic no-op for NCC that removes the cancellation in
//     S_ab - n*ma*mb for inputs with a DC offset.  The pre-pass writes the centred copies,
//     so the main kernels never subtract; one constant per image also keeps the
//     reference's exact ties along d at the left border exact (same operands, same order).
// Window means / deviations (ma, sa, mb, sb) come from the same separable f64 pre-pass.
#include "ctd_ncc_fast.h"
#include "ctd_wave.h"

namespace ctd {

// (kFND, kFWaves, kFDG: ctd_ncc_fast.h -- the plane geometry pads to kFDG)
constexpr int kFSpan = 64 + kFDG - 1;  // pattern columns one row of a workgroup touches (79)
constexpr int kFSpanPad = 80;
constexpr int kFPack = 3 * 64 + 3 * kFSpanPad;   // floats per staged row: A MA SA | B MB SB
constexpr int kFRows = 3;      // rows per LDS chunk (one barrier per chunk)
constexpr int kFBufs = 4;      // LDS chunks in the ring (loader runs kFBufs-1 chunks ahead)
constexpr int kFDmaPerRow = 9; // LDS-DMA instructions the loader issues per row

// (ncc_inv_norm: ctd_ncc_fast.h)

// cross-lane helpers (wave64) -----------------------------------------------------------
__device__ inline float lane_prev1(float x) {   // result[l] = x[l-1]
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ inline float lane_next1(float x) {   // result[l] = x[l+1]
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}
__device__ inline float lane_gather(float x, int byte_addr) {   // result[l] = x[byte_addr[l] / 4]
  return __int_as_float(__builtin_amdgcn_ds_bpermute(byte_addr, __float_as_int(x)));
}

// horizontal window sum: s[l] = sum_{k=0..BS-1} x[l - HALF + k]
template <int BS>
__device__ inline float lane_window_sum(float x, int lane) {
  constexpr int HALF = BS / 2;
  if constexpr (BS == 9) {
    float s3 = x + lane_prev1(x) + lane_next1(x);
    float m3 = lane_gather(s3, ((lane - 3) & 63) * 4);
    float p3 = lane_gather(s3, ((lane + 3) & 63) * 4);
    return s3 + m3 + p3;
  } else if constexpr (BS == 3) {
    return x + lane_prev1(x) + lane_next1(x);
  } else {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < BS; ++k) s += lane_gather(x, ((lane - HALF + k) & 63) * 4);
    return s;
  }
}

// ------------------------------------------------------------------------------------
// main kernel.  grid (w tiles, bands, frames * d groups), block 64 * (kFWaves + 1).
// Vertical sum of BS rows: for BS == 9 the 3+3+3 tree (ring of 2 products + 6 triple
// sums); other BS keep a ring of the last BS-1 products.
// ------------------------------------------------------------------------------------
// (dma_dword / dma_quad: ctd_wave.h)

// (lcm_ce: ctd_ncc_fast.h; wait_vmcnt / wait_lgkmcnt0 / wg_barrier: ctd_wave.h)

template <int BS, bool ACCUM>
__global__ __launch_bounds__(64 * (kFWaves + 1)) void ncc_fast_kernel(
    const float* __restrict__ ac, const float* __restrict__ m0, const float* __restrict__ v0,
    const float* __restrict__ bc, const float* __restrict__ m1, const float* __restrict__ v1, long st1_frame_stride,
    float* __restrict__ out, int C, int c, int H, int W, int D, int band_rows, int n_dgroups, int Wp, int W1,
    int xoff, int w_start) {
  constexpr int HALF = BS / 2;
  constexpr int TAIL = BS - 1 - HALF;          // window rows/cols after the centre
  constexpr int WOUT = 64 - (BS - 1);          // output columns per wavefront
  constexpr int UNROLL = (BS == 9) ? 6 : (BS - 1);
  extern __shared__ float lds[];               // [kFBufs][kFRows][kFPack]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.z / n_dgroups, dg = blockIdx.z - f * n_dgroups;
  const int w_lo = w_start + blockIdx.x * WOUT;
  const int h_lo = blockIdx.y * band_rows;
  const int h_hi = min(h_lo + band_rows, H);   // exclusive
  const long HW = (long)H * W;
  const int r_begin = h_lo - HALF, r_end = h_hi - 1 + TAIL;       // inclusive product rows
  const int n_rows = r_end - r_begin + 1;
  constexpr int STEP = lcm_ce(UNROLL, kFRows);                     // rows per outer iteration
  const int n_iters = (n_rows + STEP - 1) / STEP;
  const int n_chunks = n_iters * (STEP / kFRows);

  const float* a_img = ac + ((long)f * C + c) * H * Wp + 4;      // +4: column c lives at c + 4
  const float* b_img = bc + (long)f * st1_frame_stride + (long)c * H * W1;
  const float* m0i = m0 + ((long)f * C + c) * H * Wp + 4;
  const float* v0i = v0 + ((long)f * C + c) * H * Wp + 4;
  const float* m1i = m1 + (long)f * st1_frame_stride + (long)c * H * W1;
  const float* v1i = v1 + (long)f * st1_frame_stride + (long)c * H * W1;
  const int xb = w_lo - HALF - (dg * kFDG + kFDG - 1);      // unclamped pattern column of span slot 0

  if (wave == kFWaves) {
    // ------------------------------ loader wavefront ------------------------------
    const int wa = clampi(w_lo - HALF + lane, 0, W - 1);
    const int q1 = 64 + lane;                                 // second DMA of a span: slots 64..78
    const int sc0 = clampi(xb + lane, -xoff, W - 1) + xoff, sc1 = clampi(xb + q1, -xoff, W - 1) + xoff;
    const bool second = q1 < kFSpan;
    auto issue_chunk = [&](int chunk) {
      float* buf = lds + (chunk % kFBufs) * (kFRows * kFPack);
#pragma unroll
      for (int s = 0; s < kFRows; ++s) {
        const int r = r_begin + chunk * kFRows + s;
        const int rc = clampi(r, 0, H - 1);
        const int hs = clampi(r - TAIL, 0, H - 1);
        float* pk = buf + s * kFPack;
        dma_dword(a_img + (long)rc * Wp + wa, pk);
        dma_dword(m0i + (long)hs * Wp + wa, pk + 64);
        dma_dword(v0i + (long)hs * Wp + wa, pk + 128);
        dma_dword(b_img + (long)rc * W1 + sc0, pk + 192);
        dma_dword(m1i + (long)hs * W1 + sc0, pk + 192 + kFSpanPad);
        dma_dword(v1i + (long)hs * W1 + sc0, pk + 192 + 2 * kFSpanPad);
        // lanes >= 15 re-fetch slot 78's column into the pad slot / next array's head;
        // harmless: the pad is never read and the next array is rewritten by ITS OWN DMA
        // only if issued later -- so issue the tails BEFORE nothing depends on order:
        if (second) {
          dma_dword(b_img + (long)rc * W1 + sc1, pk + 192 + 64);
          dma_dword(m1i + (long)hs * W1 + sc1, pk + 192 + kFSpanPad + 64);
          dma_dword(v1i + (long)hs * W1 + sc1, pk + 192 + 2 * kFSpanPad + 64);
        }
      }
    };
    constexpr int L = kFRows * kFDmaPerRow;                   // DMA instructions per chunk
#pragma unroll
    for (int k = 0; k < kFBufs - 1; ++k)
      if (k < n_chunks) issue_chunk(k);
    // chunk 0 landed when at most (kFBufs-2) younger chunks are still in flight
    if (n_chunks >= kFBufs - 1) wait_vmcnt<L*(kFBufs - 2)>(); else wait_vmcnt<0>();
    wg_barrier();
    for (int ch = 0; ch < n_chunks; ++ch) {
      // buffer (ch-1) % kFBufs was released by the consumers at the previous barrier
      const int nxt = ch + kFBufs - 1;
      if (nxt < n_chunks) {
        issue_chunk(nxt);
        wait_vmcnt<L*(kFBufs - 2)>();                         // chunk ch+1 has landed
      } else {
        wait_vmcnt<0>();
      }
      wg_barrier();
    }
    return;
  }

  // -------------------------------- consumer wavefronts --------------------------------
  const int d_base = dg * kFDG + wave * kFND;
  const int w0 = w_lo - HALF + lane;           // unclamped product column == output column
  float* vol = out + (long)f * D * HW;
  const bool lane_out = (lane >= HALF) && (lane < 64 - TAIL) && (w0 < W);
  const int bq = lane + (kFDG - 1) - wave * kFND;   // span slot of (lane, j = 0); j-th disparity reads bq - j

  float P[kFND][BS == 9 ? 2 : BS - 1];
  float T[kFND][BS == 9 ? 6 : 1];
#pragma unroll
  for (int j = 0; j < kFND; ++j) {
#pragma unroll
    for (int k = 0; k < (BS == 9 ? 2 : BS - 1); ++k) P[j][k] = 0.f;
#pragma unroll
    for (int k = 0; k < (BS == 9 ? 6 : 1); ++k) T[j][k] = 0.f;
  }

  wg_barrier();                                                    // chunk 0 is in LDS
  int chunk = 0;
  for (int it = 0; it < n_iters; ++it) {
#pragma unroll
    for (int u = 0; u < STEP; ++u) {
      const int r = r_begin + it * STEP + u;
      const float* pk = lds + ((chunk % kFBufs) * kFRows + (u % kFRows)) * kFPack;
      const float a = pk[lane];
      const float mav = pk[64 + lane], sav = pk[128 + lane];
      float bv[kFND], mbv[kFND], sbv[kFND];
#pragma unroll
      for (int j = 0; j < kFND; ++j) {
        bv[j] = pk[192 + bq - j];
        mbv[j] = pk[192 + kFSpanPad + bq - j];
        sbv[j] = pk[192 + 2 * kFSpanPad + bq - j];
      }
      const int h = r - TAIL;                                     // output row completed by product row r
      const bool row_out = (h >= h_lo) && (h < h_hi);             // wave-uniform
      const float nma = mav;                                      // -bs^2 * (window mean), from the pre-pass
#pragma unroll
      for (int j = 0; j < kFND; ++j) {
        const float p = a * bv[j];
        float v;
        if constexpr (BS == 9) {
          const float t3 = p + P[j][(u + 1) % 2] + P[j][u % 2];
          P[j][u % 2] = p;
          v = t3 + T[j][(u + 3) % 6] + T[j][u % 6];
          T[j][u % 6] = t3;
        } else {
          v = p;
#pragma unroll
          for (int k = 0; k < BS - 1; ++k) v += P[j][k];
          P[j][u % (BS - 1)] = p;
        }
        const float s = lane_window_sum<BS>(v, lane);
        const float cov = fmaf(nma, mbv[j], s);
        float val = cov * ncc_inv_norm(sav, sbv[j]);
        const int d = d_base + j;
        if (lane_out && row_out && d < D) {
          const long o = (long)d * HW + (long)h * W + w0;
          if (ACCUM) val += vol[o];
          vol[o] = val;
        }
      }
      if ((u % kFRows) == kFRows - 1) {                            // chunk consumed: hand the buffer back
        wait_lgkmcnt0();
        wg_barrier();
        ++chunk;
      }
    }
  }
}

// ------------------------------------------------------------------------------------
// WIDE kernel: every lane owns 4 adjacent product columns, a wavefront 256 of them.
// A bs <= 9 window then reaches only into the two neighbouring lanes, so the horizontal
// window sum needs nothing but +-1 lane DPP shifts of per-lane prefix / suffix sums
// (no LDS crossbar traffic), 62 of 64 lanes produce outputs, frame-side LDS reads are
// one ds_read_b128 per array and each lane stores 16 contiguous bytes (1 KB per wave
// instruction).  Same loader / consumer split and LDS ring as the narrow kernel above,
// which remains in use for the columns left over when W is not a multiple of 248.
// ------------------------------------------------------------------------------------
constexpr int kWCols = 4;                     // product columns per lane
constexpr int kWND = 2;                       // disparities per lane
constexpr int kWWaves = 8;                    // consumer wavefronts per workgroup
constexpr int kWDG = kWND * kWWaves;          // disparities per workgroup (8)
constexpr int kWTile = 64 * kWCols;           // product columns per wavefront (256)
constexpr int kWOut = 62 * kWCols;            // output columns per wavefront (248)
constexpr int kWSpan = kWTile + kWDG - 1;     // 263 pattern columns per row
constexpr int kWSpanPad = (kWSpan + 1 + 3) / 4 * 4;   // multiple of 4, > kWSpan
constexpr int kWPack = 3 * kWTile + 3 * kWSpanPad;   // 1560 floats per staged row
constexpr int kWRows = 3;                     // rows per LDS chunk
constexpr int kWBufs = 3;                     // chunks in the ring
constexpr int kWDmaPerRow = 3 + 3 * 2;        // dwordx4 LDS-DMA instructions per row

// Four floats starting OFF slots after the lane's own quad of a 16-byte aligned LDS array:
// one or two conflict-free ds_read_b128 (a stride-4 ds_read_b32 pattern is a 4-way bank conflict).

template <int OFF>
__device__ inline void lds_read4(const float* arr, int lane, float (&o)[4]) {
  constexpr int Q = OFF / 4, S = OFF % 4;
  // the empty asm "uses" all four elements: it keeps the compiler from narrowing the loads to the
  // elements actually consumed (ds_read_b32 / read2 at a 16-byte lane stride, which is exactly the
  // conflicting pattern this helper avoids)
  f32x4 A = *(const f32x4*)(arr + 4 * (lane + Q));
  asm("" : "+v"(A));
  const float a[4] = {A[0], A[1], A[2], A[3]};
  if constexpr (S == 0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = a[i];
  } else {
    f32x4 B = *(const f32x4*)(arr + 4 * (lane + Q + 1));
    asm("" : "+v"(B));
    const float b[4] = {B[0], B[1], B[2], B[3]};
#pragma unroll
    for (int i = 0; i < 4; ++i) o[i] = (S + i < 4) ? a[(S + i) & 3] : b[(S + i) & 3];
  }
}

// Five floats starting OFF slots after the lane's own quad, from two aligned quads: element k of `lo5` is
// slot OFF + k.  Two adjacent disparities of a lane (span offsets OFF+1 and OFF) read the same two quads.
template <int OFF>
__device__ inline void lds_read5(const float* arr, int lane, float (&o)[5]) {
  constexpr int Q = OFF / 4, S = OFF % 4;
  f32x4 A = *(const f32x4*)(arr + 4 * (lane + Q));
  f32x4 B = *(const f32x4*)(arr + 4 * (lane + Q + 1));
  asm("" : "+v"(A));
  asm("" : "+v"(B));
  const float e[8] = {A[0], A[1], A[2], A[3], B[0], B[1], B[2], B[3]};
#pragma unroll
  for (int k = 0; k < 5; ++k) o[k] = e[S + k];
}

// (window_combine4: ctd_wave.h)

template <int BS, bool ACCUM, bool VEC4, int WAVE>
__device__ __forceinline__ void wide_consume(const float* lds, float* __restrict__ out, int f, int dg, int lane,
                                             int w_lo, int c_lo, int h_lo, int h_hi, int r_begin, int n_iters, int H,
                                             int W, int D) {
  constexpr int HALF = BS / 2;
  constexpr int TAIL = BS - 1 - HALF;
  constexpr int UNROLL = (BS == 9) ? 6 : (BS - 1);
  constexpr int STEP = lcm_ce(UNROLL, kWRows);
  const long HW = (long)H * W;
  const int d_base = dg * kWDG + WAVE * kWND;
  const int c0 = c_lo + kWCols * lane;         // unclamped first column of this lane
  float* vol = out + (long)f * D * HW;
  const bool lane_out = (lane >= 1) && (lane <= 62) && (c0 < W);

  float P[kWND][kWCols][BS == 9 ? 2 : BS - 1];
  float T[kWND][kWCols][BS == 9 ? 6 : 1];
#pragma unroll
  for (int j = 0; j < kWND; ++j)
#pragma unroll
    for (int i = 0; i < kWCols; ++i) {
#pragma unroll
      for (int k = 0; k < (BS == 9 ? 2 : BS - 1); ++k) P[j][i][k] = 0.f;
#pragma unroll
      for (int k = 0; k < (BS == 9 ? 6 : 1); ++k) T[j][i][k] = 0.f;
    }

  // All LDS operands of one product row (and of the output row it completes).
  struct RowOps {
    float a[4], ma[4], sa[4];
    float b[kWND][4], mb[kWND][4], sb[kWND][4];
  };
  constexpr int kOff0 = (kWDG - 1) - WAVE * kWND;                  // span slot offset of disparity j = 0
  auto load_row = [&](const float* pk) {
    RowOps o;
    lds_read4<0>(pk, lane, o.a);
    lds_read4<0>(pk + kWTile, lane, o.ma);
    lds_read4<0>(pk + 2 * kWTile, lane, o.sa);
    lds_read4<kOff0>(pk + 3 * kWTile, lane, o.b[0]);
    lds_read4<kOff0>(pk + 3 * kWTile + kWSpanPad, lane, o.mb[0]);
    lds_read4<kOff0>(pk + 3 * kWTile + 2 * kWSpanPad, lane, o.sb[0]);
    if constexpr (kWND == 2) {
      lds_read4<(kOff0 > 0 ? kOff0 - 1 : 0)>(pk + 3 * kWTile, lane, o.b[kWND - 1]);
      lds_read4<(kOff0 > 0 ? kOff0 - 1 : 0)>(pk + 3 * kWTile + kWSpanPad, lane, o.mb[kWND - 1]);
      lds_read4<(kOff0 > 0 ? kOff0 - 1 : 0)>(pk + 3 * kWTile + 2 * kWSpanPad, lane, o.sb[kWND - 1]);
    }
    return o;
  };
  static_assert(kWND == 1 || kWND == 2, "load_row spells out one or two disparities");

  wg_barrier();                                                    // chunk 0 is in LDS
  int chunk = 0;
  for (int it = 0; it < n_iters; ++it) {
#pragma unroll
    for (int u = 0; u < STEP; ++u) {
      const int r = r_begin + it * STEP + u;
      const bool last_of_chunk = (u % kWRows) == kWRows - 1;
      // every LDS operand of the row is requested up front (15 ds_read_b128 in flight)
      const RowOps cur = load_row(lds + ((chunk % kWBufs) * kWRows + (u % kWRows)) * kWPack);
      float nma[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) nma[i] = cur.ma[i];              // -bs^2 * (window mean), from the pre-pass
      const int h = r - TAIL;
      const bool row_out = (h >= h_lo) && (h < h_hi);             // wave-uniform
#pragma unroll
      for (int j = 0; j < kWND; ++j) {
        float x[kWCols];
#pragma unroll
        for (int i = 0; i < kWCols; ++i) {
          const float p = cur.a[i] * cur.b[j][i];
          if constexpr (BS == 9) {
            const float t3 = p + P[j][i][(u + 1) % 2] + P[j][i][u % 2];
            P[j][i][u % 2] = p;
            x[i] = t3 + T[j][i][(u + 3) % 6] + T[j][i][u % 6];
            T[j][i][u % 6] = t3;
          } else {
            float v = p;
#pragma unroll
            for (int k = 0; k < BS - 1; ++k) v += P[j][i][k];
            P[j][i][u % (BS - 1)] = p;
            x[i] = v;
          }
        }
        // horizontal window sums of the lane's 4 columns from prefix / suffix sums of the
        // neighbouring lanes: out_i = suffix_prev(i - HALF + 4) + own(i-HALF .. i+TAIL) + prefix_next(i + TAIL - 4)
        float pre[kWCols], suf[kWCols];                            // pre[k] = x0..xk, suf[k] = xk..x3
        pre[0] = x[0];
#pragma unroll
        for (int k = 1; k < kWCols; ++k) pre[k] = pre[k - 1] + x[k];
        suf[kWCols - 1] = x[kWCols - 1];
#pragma unroll
        for (int k = kWCols - 2; k >= 0; --k) suf[k] = suf[k + 1] + x[k];
        float s[kWCols];
        if constexpr (BS == 9) {
          // window = previous lane's columns i..3, all four own columns, next lane's columns 0..i
          window_combine4(suf, pre[kWCols - 1], pre, s);
        } else {
#pragma unroll
          for (int i = 0; i < kWCols; ++i) {
            const int lo = i - HALF, hi = i + TAIL;                // window in own-lane column units
            const int o_lo = lo < 0 ? 0 : lo, o_hi = hi > kWCols - 1 ? kWCols - 1 : hi;
            float own;
            if (o_lo == 0) own = pre[o_hi];
            else if (o_hi == kWCols - 1) own = suf[o_lo];
            else { own = x[o_lo]; for (int k = o_lo + 1; k <= o_hi; ++k) own += x[k]; }
            float acc = own;
            if (lo < 0) acc = lane_prev1(suf[lo + kWCols]) + acc;  // previous lane's columns lo+4 .. 3
            if (hi > kWCols - 1) acc = acc + lane_next1(pre[hi - kWCols]);   // next lane's columns 0 .. hi-4
            s[i] = acc;
          }
        }
        float val[kWCols];
#pragma unroll
        for (int i = 0; i < kWCols; ++i) {
          const float cov = fmaf(nma[i], cur.mb[j][i], s[i]);
          val[i] = cov * ncc_inv_norm(cur.sa[i], cur.sb[j][i]);
        }
        const int d = d_base + j;
        if (row_out && lane_out && d < D) {
          float* o = vol + (long)d * HW + (long)h * W + c0;
          if constexpr (VEC4) {   // W % 4 == 0 and 16-byte aligned volume: c0 < W implies c0 + 3 < W
            float4 v4 = make_float4(val[0], val[1], val[2], val[3]);
            if (ACCUM) {
              const float4 old = *(const float4*)o;
              v4.x += old.x; v4.y += old.y; v4.z += old.z; v4.w += old.w;
            }
            __builtin_nontemporal_store(f32x4{v4.x, v4.y, v4.z, v4.w}, (f32x4*)o);   // see ncc_fast_t256_kernel
          } else {
#pragma unroll
            for (int i = 0; i < kWCols; ++i)
              if (c0 + i < W) o[i] = ACCUM ? o[i] + val[i] : val[i];
          }
        }
      }
      if (last_of_chunk) {
        wait_lgkmcnt0();
        wg_barrier();
        ++chunk;
      }
    }
  }
}

template <int BS, bool ACCUM, bool VEC4>
__global__ __launch_bounds__(64 * (kWWaves + 1)) void ncc_fast_wide_kernel(
    const float* __restrict__ ac, const float* __restrict__ m0, const float* __restrict__ v0,
    const float* __restrict__ bc, const float* __restrict__ m1, const float* __restrict__ v1, long st1_frame_stride,
    float* __restrict__ out, int C, int c, int H, int W, int D, int band_rows, int n_dgroups, int Wp, int W1,
    int xoff) {
  constexpr int HALF = BS / 2;
  constexpr int TAIL = BS - 1 - HALF;
  static_assert(HALF <= kWCols && TAIL <= kWCols, "window must stay inside the neighbouring lanes");
  constexpr int UNROLL = (BS == 9) ? 6 : (BS - 1);
  constexpr int STEP = lcm_ce(UNROLL, kWRows);
  extern __shared__ float lds[];               // [kWBufs][kWRows][kWPack]

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int f = blockIdx.z / n_dgroups, dg = blockIdx.z - f * n_dgroups;
  const int w_lo = blockIdx.x * kWOut;
  const int h_lo = blockIdx.y * band_rows;
  const int h_hi = min(h_lo + band_rows, H);
  const int r_begin = h_lo - HALF, r_end = h_hi - 1 + TAIL;
  const int n_rows = r_end - r_begin + 1;
  const int n_iters = (n_rows + STEP - 1) / STEP;
  const int n_chunks = n_iters * (STEP / kWRows);

  const float* a_img = ac + ((long)f * C + c) * H * Wp + 4;      // +4: column c lives at c + 4
  const float* b_img = bc + (long)f * st1_frame_stride + (long)c * H * W1;
  const float* m0i = m0 + ((long)f * C + c) * H * Wp + 4;
  const float* v0i = v0 + ((long)f * C + c) * H * Wp + 4;
  const float* m1i = m1 + (long)f * st1_frame_stride + (long)c * H * W1;
  const float* v1i = v1 + (long)f * st1_frame_stride + (long)c * H * W1;
  const int c_lo = w_lo - kWCols;                              // unclamped product column of slot 0
  const int xb = c_lo - (dg * kWDG + kWDG - 1);                // unclamped pattern column of span slot 0

  if (wave == kWWaves) {
    // ------------------------------ loader wavefront ------------------------------
    // 16 bytes per lane and DMA: one instruction moves a whole 256-column array row.  All sources are
    // 16-byte aligned by construction (padded planes, see fast_workspace); lanes past the image are
    // clamped to the last quad, which only ever feeds columns that produce no output.
    const int aq = min(c_lo + kWCols * lane, Wp - 8);                         // frame quad of this lane (>= -4)
    const int sq0 = min(xb + xoff + kWCols * lane, W1 - kWCols);              // pattern quad, slots 0..255
    const int sq1 = min(xb + xoff + kWTile + kWCols * lane, W1 - kWCols);     // slots 256.. (first 2 lanes)
    const bool tail_lane = kWTile + kWCols * lane < kWSpan;
    auto issue_chunk = [&](int chunk) {
      float* buf = lds + (chunk % kWBufs) * (kWRows * kWPack);
#pragma unroll
      for (int s = 0; s < kWRows; ++s) {
        const int r = r_begin + chunk * kWRows + s;
        const int rc = clampi(r, 0, H - 1);
        const int hs = clampi(r - TAIL, 0, H - 1);
        float* pk = buf + s * kWPack;
        dma_quad(a_img + (long)rc * Wp + aq, pk);
        dma_quad(m0i + (long)hs * Wp + aq, pk + kWTile);
        dma_quad(v0i + (long)hs * Wp + aq, pk + 2 * kWTile);
        dma_quad(b_img + (long)rc * W1 + sq0, pk + 3 * kWTile);
        dma_quad(m1i + (long)hs * W1 + sq0, pk + 3 * kWTile + kWSpanPad);
        dma_quad(v1i + (long)hs * W1 + sq0, pk + 3 * kWTile + 2 * kWSpanPad);
        if (tail_lane) {
          dma_quad(b_img + (long)rc * W1 + sq1, pk + 3 * kWTile + kWTile);
          dma_quad(m1i + (long)hs * W1 + sq1, pk + 3 * kWTile + kWSpanPad + kWTile);
          dma_quad(v1i + (long)hs * W1 + sq1, pk + 3 * kWTile + 2 * kWSpanPad + kWTile);
        }
      }
    };
    constexpr int L = kWRows * kWDmaPerRow;                   // DMA instructions per chunk
    static_assert(L * (kWBufs - 2) < 64, "in-flight DMA count must fit vmcnt");
#pragma unroll
    for (int k = 0; k < kWBufs - 1; ++k)
      if (k < n_chunks) issue_chunk(k);
    if (n_chunks >= kWBufs - 1) wait_vmcnt<L*(kWBufs - 2)>(); else wait_vmcnt<0>();
    wg_barrier();
    for (int ch = 0; ch < n_chunks; ++ch) {
      const int nxt = ch + kWBufs - 1;
      if (nxt < n_chunks) {
        issue_chunk(nxt);
        wait_vmcnt<L*(kWBufs - 2)>();
      } else {
        wait_vmcnt<0>();
      }
      wg_barrier();
    }
    return;
  }

  // -------------------------------- consumer wavefronts --------------------------------
  // the span offset of a wave's disparities is a compile-time constant of its wave index,
  // which turns the unaligned 4-float pattern reads into aligned ds_read_b128 pairs
#define CTD_WCASE(WV) \
  case WV: wide_consume<BS, ACCUM, VEC4, (WV < kWWaves ? WV : 0)>(lds, out, f, dg, lane, w_lo, c_lo, h_lo, h_hi, r_begin, n_iters, H, W, D); break;
  switch (wave) {
    CTD_WCASE(0) CTD_WCASE(1) CTD_WCASE(2) CTD_WCASE(3) CTD_WCASE(4) CTD_WCASE(5) CTD_WCASE(6) CTD_WCASE(7)
    default: break;
  }
#undef CTD_WCASE
}

static int pick_bands(long wg_per_band, int H, int bs) {
  // enough workgroups to fill 256 CUs a few times over, few enough that the (bs-1)-row
  // warm-up of every band stays a small fraction of its rows
  int bands = 1;
  while (bands < 8 && wg_per_band * bands < 2048 && H / (bands * 2) >= 8 * (bs - 1)) bands *= 2;
  return bands;
}

template <int BS>
static int launch_tiles_bs(float* out, int frames, int C, int H, int W, int D, const FastWorkspace& ws, long st1_stride,
                           hipStream_t stream) {
  constexpr int WOUT = 64 - (BS - 1);
  // column split: full 248-column wide tiles (plus one more when the remainder is large),
  // the rest in 64-(BS-1)-column narrow tiles
  int n_wide = W / kWOut;
  if (W - n_wide * kWOut > kWOut / 2) ++n_wide;
  const int w_rem = n_wide * kWOut < W ? n_wide * kWOut : W;     // first column of the narrow part
  for (int c = 0; c < C; ++c) {
    if (n_wide > 0) {
      const int n_dg = ceil_div(D, kWDG);
      const int bands = pick_bands((long)n_wide * frames * n_dg, H, BS);
      const int band_rows = ceil_div(H, bands);
      dim3 grid(n_wide, ceil_div(H, band_rows), frames * n_dg), block(64 * (kWWaves + 1));
      const size_t lds = sizeof(float) * kWBufs * kWRows * kWPack;
      const bool vec4 = (W % 4 == 0) && (((uintptr_t)out) % 16 == 0);
      auto kern = c == 0 ? (vec4 ? ncc_fast_wide_kernel<BS, false, true> : ncc_fast_wide_kernel<BS, false, false>)
                         : (vec4 ? ncc_fast_wide_kernel<BS, true, true> : ncc_fast_wide_kernel<BS, true, false>);
      timing_begin(stream);
      hipLaunchKernelGGL(kern, grid, block, lds, stream, ws.ac, ws.m0, ws.v0, ws.bc, ws.m1, ws.v1, st1_stride, out, C,
                         c, H, W, D, band_rows, n_dg, ws.Wp, ws.W1, ws.xoff);
      timing_end(stream, w_rem);
      CTD_LAUNCH_CHECK();
    }
    if (w_rem < W) {
      const int n_dg = ceil_div(D, kFDG);
      const int n_tiles = ceil_div(W - w_rem, WOUT);
      const int bands = pick_bands((long)n_tiles * frames * n_dg, H, BS);
      const int band_rows = ceil_div(H, bands);
      dim3 grid(n_tiles, ceil_div(H, band_rows), frames * n_dg), block(64 * (kFWaves + 1));
      const size_t lds = sizeof(float) * kFBufs * kFRows * kFPack;
      auto kern = c == 0 ? ncc_fast_kernel<BS, false> : ncc_fast_kernel<BS, true>;
      hipLaunchKernelGGL(kern, grid, block, lds, stream, ws.ac, ws.m0, ws.v0, ws.bc, ws.m1, ws.v1, st1_stride, out, C,
                         c, H, W, D, band_rows, n_dg, ws.Wp, ws.W1, ws.xoff, w_rem);
      CTD_LAUNCH_CHECK();
    }
  }
  return CTD_OK;
}

int launch_tiles(float* out, int frames, int C, int H, int W, int D, int bs, const FastWorkspace& ws, long st1_stride,
                 hipStream_t stream) {
  if (bs == 9 && W % 4 == 0 && ((uintptr_t)out) % 16 == 0) return launch_t256(out, frames, C, H, W, D, ws, st1_stride, stream);
  switch (bs) {
    case 3: return launch_tiles_bs<3>(out, frames, C, H, W, D, ws, st1_stride, stream);
    case 5: return launch_tiles_bs<5>(out, frames, C, H, W, D, ws, st1_stride, stream);
    case 7: return launch_tiles_bs<7>(out, frames, C, H, W, D, ws, st1_stride, stream);
    case 9: return launch_tiles_bs<9>(out, frames, C, H, W, D, ws, st1_stride, stream);
    default: return CTD_ERR_UNSUPPORTED;
  }
}

}  // namespace ctd
