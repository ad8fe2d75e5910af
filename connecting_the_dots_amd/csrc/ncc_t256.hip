// ncc_t256.hip -- tile-256 kernel of the fast NCC path: the volume by disparity groups in 256-column tiles, what a
// call with several channels launches (the stages of a call: ncc_fast.hip; work decomposition: ncc_tiles.hip).
#include <type_traits>

#include "ctd_ncc_fast.h"
#include "ctd_wave.h"

namespace ctd {

// ------------------------------------------------------------------------------------
// TILE-256 kernel (bs == 9, W % 4 == 0): the production kernel.
// Same consumer pipeline as the wide kernel, but a wavefront's 64 lanes own exactly 256
// OUTPUT columns (1 KB-aligned 16-byte stores, every lane valid, W = 512 is two tiles with
// no leftover columns).  The two halo quads a tile needs (4 product columns left of lane 0,
// 4 right of lane 63) are computed by the LOADER wavefront: its lanes hold, per consumer
// wave and disparity, the vertical ring of the halo quad and publish its suffix / prefix
// sums into the staged row, one chunk ahead of the consumers and under the same barrier.
// Volume stores that are not 128-byte aligned cost ~25 % of HBM write bandwidth
// (tools/ubench_store.hip), and per-CU operand staging is limited to ~10 B/clk
// (tools/ubench_struct.hip), hence >= 12 disparities per workgroup (14: seven consumer wavefronts of two).
// ------------------------------------------------------------------------------------
constexpr int kTWaves = 7;                     // consumer wavefronts per workgroup.  7 (+ loader) = two 8-wave workgroups per CU at
                                               // 128 VGPRs = exactly 4 waves on every SIMD; with 6 two SIMDs carry 4 waves and two
                                               // carry 3, and the chunk barrier makes the lighter ones wait (measured: 7 is 9 % faster
                                               // although 10 groups of 14 disparities compute 140 for D = 128)
constexpr int kTND = 2;                        // disparities per lane
constexpr int kTDG = kTWaves * kTND;           // 14 disparities per workgroup
constexpr int kTTile = 256;                    // output columns per workgroup
constexpr int kTA = kTTile + 8;                // frame-side array: 4 halo columns either side
constexpr int kTSpanPad = (kTA + kTDG - 1 + 1 + 3) / 4 * 4;   // multiple of 4, > span
static_assert(kTA + kTDG - 1 < kTSpanPad, "pattern span must fit its padded array");
constexpr int kTHalo = kTWaves * kTND * 2 * 4; // [wave][j][side][4] halo sums
constexpr int kTPack = 3 * kTA + 3 * kTSpanPad + kTHalo;   // 1760 floats per staged row
constexpr int kTRows = 3;
constexpr int kTBufs = 3;
constexpr int kTDmaPerRow = 12;                // 3 x 2 frame-side + 3 x 2 pattern-side dwordx4 DMAs
constexpr int kTOffB = 3 * kTA, kTOffH = 3 * kTA + 3 * kTSpanPad;

// KS = sub-quad shift of the wavefront's pattern-side operands, (12 - 2 * wave) % 4: 0 for even consumer wavefronts, 2
// for odd ones.  Everything else that depends on the wavefront index (quad offset, halo slot) is a run-time scalar, so
// the kernel carries TWO copies of the consumer loop, not seven: with one copy per wavefront the seven hot loops of a
// workgroup (plus the loader's) are a 77 KB instruction working set against a 64 KB instruction cache shared by two CUs.
template <bool ACCUM, int KS>
__device__ __forceinline__ void t256_consume(float* lds, float* __restrict__ out, int WAVE, int f, int dg, int lane,
                                             int w_lo, int h_lo, int h_hi, int r_begin, int n_iters, int H, int W, int D) {
  constexpr int TAIL = 4, STEP = lcm_ce(6, kTRows);               // block size 9
  const long HW = (long)H * W;
  const int d_base = dg * kTDG + WAVE * kTND;
  // per-lane column arithmetic is kept to ONE register, 4 * lane: everything else about the column tile (w_lo) goes
  // into scalar bases -- the consumers run at the 128-VGPR limit of four wavefronts per SIMD
  const unsigned l4 = 4u * (unsigned)lane;                         // first column of the lane, relative to w_lo
  float* vol = out + (long)f * D * HW + w_lo;
  const bool lane_out = w_lo + (int)l4 < W;
  float P[kTND][4][2], T[kTND][4][6];
#pragma unroll
  for (int j = 0; j < kTND; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      P[j][i][0] = P[j][i][1] = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) T[j][i][k] = 0.f;
    }
  const int kOff0 = (kTDG - 1) - WAVE * kTND;                      // span slot offset of disparity j = 0
  const int kQ = (kOff0 - 1) / 4;                                  // disparity j = 1 sits one span slot below j = 0:
  constexpr int kS = KS;                                           // both come out of the same two aligned quads
  static_assert(kTND == 2 && (kTDG - 2) % 4 == 0, "two disparities per lane; (kOff0 - 1) % 4 alternates 0, 2");
  // halo sums: lane 0 takes the left quad's suffix sums, lane 63 the right quad's prefix sums, others zero
  const int halo4 = lane == 63 ? 4 : 0;
  // applied as a multiplicative mask: hipcc 7.2 miscompiles the select form `halo_lane ? hq[i] : 0.f` here
  // (it zeroes the value for every lane < 63, lane 0 included)
  const float halo_mask = (lane == 0 || lane == 63) ? 1.f : 0.f;
  auto quad = [](const float* p) { return *(const f32x4*)p; };

  wg_barrier();                                                    // chunk 0 (operands + halos) is in LDS
  if (d_base >= D) {
    // both disparities of this wavefront lie past D (last disparity group): keep the barrier protocol, skip the work
    for (int it = 0; it < n_iters * (STEP / kTRows); ++it) wg_barrier();
    return;
  }
  int chunk = 0;
  f32x4 qa, qb0, qb1;                                              // value quads of the row (frame, pattern x 2)
  for (int it = 0; it < n_iters; ++it) {
#pragma unroll
    for (int u = 0; u < STEP; ++u) {
      const int r = r_begin + it * STEP + u;
      const bool last_of_chunk = (u % kTRows) == kTRows - 1;
      // Phase A, every row: products and the vertical 3+3+3 rings of both disparities (needs only the two value
      // quads).  Phase B, output rows only (wave-uniform branch; the (bs-1) warm-up rows of a band skip it):
      // statistics quads requested first so that they arrive under the horizontal sums, then window sums,
      // normalisation and the store.
      // One per-lane base per row, made opaque: every LDS operand of the row is then base + 16-bit immediate.
      // (Likewise every address below is an opaque per-row SCALAR plus one of two loop-invariant lane registers, l4 or
      // halo4: anything the compiler can prove loop-invariant it hoists into a register of its own, and there are none
      // to spare.)
      int row_o = ((chunk % kTBufs) * kTRows + (u % kTRows)) * kTPack + 4;
      asm("" : "+s"(row_o));
      int own_o = row_o + (int)l4;
      asm("" : "+v"(own_o));
      const float* own = lds + own_o;                              // own quad after the left halo
      int pat_s = row_o + kTOffB + 4 * kQ;
      asm("" : "+s"(pat_s));
      int pat_o = pat_s + (int)l4;
      asm("" : "+v"(pat_o));
      const float* pat = lds + pat_o;                              // first of the lane's two pattern-side quads
      int hq_s = row_o - 4 + kTOffH + WAVE * (kTND * 2 * 4);
      asm("" : "+s"(hq_s));
      int hq_o = hq_s + halo4;
      asm("" : "+v"(hq_o));
      const float* hqp = lds + hq_o;                               // halo sums of (this wave, j 0) on this lane's side
      // The value quads of a chunk's first row are read here; those of its other rows were requested under phase B of
      // the previous row.
      if ((u % kTRows) == 0) {
        qa = quad(own);
        qb0 = quad(pat);
        qb1 = quad(pat + 4);
      }
      asm("" : "+v"(qa), "+v"(qb0), "+v"(qb1));
      const float av[4] = {qa[0], qa[1], qa[2], qa[3]};
      const float be[8] = {qb0[0], qb0[1], qb0[2], qb0[3], qb1[0], qb1[1], qb1[2], qb1[3]};
      const int h = r - TAIL;
      const bool row_out = (h >= h_lo) && (h < h_hi);             // wave-uniform
      float x[kTND][4];
#pragma unroll
      for (int j = 0; j < kTND; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = av[i] * be[kS + (1 - j) + i];            // b[j][i] = slot kOff0 - j + i
          const float t3 = p + P[j][i][(u + 1) % 2] + P[j][i][u % 2];
          P[j][i][u % 2] = p;
          x[j][i] = t3 + T[j][i][(u + 3) % 6] + T[j][i][u % 6];
          T[j][i][u % 6] = t3;
        }
      auto prefetch_next = [&]() {                                 // next row of the same chunk: one ring row further
        if (!last_of_chunk) {
          qa = quad(own + kTPack);
          qb0 = quad(pat + kTPack);
          qb1 = quad(pat + kTPack + 4);
        }
      };
      if (row_out) {
        f32x4 qma = quad(own + kTA), qsa = quad(own + 2 * kTA);
        f32x4 qm0 = quad(pat + kTSpanPad), qm1 = quad(pat + kTSpanPad + 4);
        f32x4 qs0 = quad(pat + 2 * kTSpanPad), qs1 = quad(pat + 2 * kTSpanPad + 4);
        prefetch_next();                                           // requested under the whole of phase B
        float me[8], se[8];
#pragma unroll
        for (int j = 0; j < kTND; ++j) {
          float pre[4], suf[4];
          pre[0] = x[j][0];
          pre[1] = pre[0] + x[j][1];
          pre[2] = pre[1] + x[j][2];
          pre[3] = pre[2] + x[j][3];
          suf[3] = x[j][3];
          suf[2] = suf[3] + x[j][2];
          suf[1] = suf[2] + x[j][1];
          suf[0] = suf[1] + x[j][0];
          float sj[4];
          window_combine4(suf, pre[3], pre, sj);                    // wave-edge lanes get 0 from the missing neighbour
          if (j == 0) {
            // statistics quads: pinned after the first window sums (data dependency keeps the wait here)
            asm("" : "+v"(qma), "+v"(qsa), "+v"(qm0), "+v"(qm1) : "v"(sj[0]), "v"(sj[3]));
            asm("" : "+v"(qs0), "+v"(qs1) : "v"(sj[0]), "v"(sj[3]));
#pragma unroll
            for (int k = 0; k < 4; ++k) { me[k] = qm0[k]; me[4 + k] = qm1[k]; se[k] = qs0[k]; se[4 + k] = qs1[k]; }
          }
          f32x4 hq = quad(hqp + j * 2 * 4);
          asm("" : "+v"(hq));
          float val[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float sh = fmaf(halo_mask, hq[i], sj[i]);
            const float cov = fmaf(qma[i], me[kS + (1 - j) + i], sh);   // qma = -bs^2 * (window mean), from the pre-pass
            val[i] = cov * ncc_inv_norm(qsa[i], se[kS + (1 - j) + i]);
          }
          const int d = d_base + j;
          if (lane_out && d < D) {
            long ooff = (long)d * HW + (long)h * W;
            asm("" : "+s"(ooff));
            float4* o = (float4*)(vol + ooff + l4);
            float4 v4 = make_float4(val[0], val[1], val[2], val[3]);
            if (ACCUM) {
              const float4 old = *o;
              v4.x += old.x; v4.y += old.y; v4.z += old.z; v4.w += old.w;
            }
            // written once, next read by another kernel after 1.8 GB more: non-temporal (-8 % on the launch)
            __builtin_nontemporal_store(f32x4{v4.x, v4.y, v4.z, v4.w}, (f32x4*)o);
          }
        }
      } else {
        prefetch_next();
      }
      if (last_of_chunk) {
        wait_lgkmcnt0();
        wg_barrier();
        ++chunk;
      }
    }
  }
}

template <bool ACCUM>
__global__ __launch_bounds__(64 * (kTWaves + 1), 4) void ncc_fast_t256_kernel(
    const float* __restrict__ ac, const float* __restrict__ m0, const float* __restrict__ v0,
    const float* __restrict__ bc, const float* __restrict__ m1, const float* __restrict__ v1, long st1_frame_stride,
    float* __restrict__ out, int C, int c, int H, int W, int D, int band_rows, int n_dgroups, int Wp, int W1, int xoff) {
  constexpr int HALF = 4, TAIL = 4, STEP = lcm_ce(6, kTRows), CPI = STEP / kTRows;   // chunks per outer iteration
  extern __shared__ float lds[];                                  // [kTBufs][kTRows][kTPack]
  // the wave index feeds scalar arithmetic (disparity base, LDS offsets): make it a scalar for the compiler
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int f = blockIdx.z / n_dgroups, dg = blockIdx.z - f * n_dgroups;
  const int w_lo = blockIdx.x * kTTile;
  const int h_lo = blockIdx.y * band_rows;
  const int h_hi = min(h_lo + band_rows, H);
  const int r_begin = h_lo - HALF, r_end = h_hi - 1 + TAIL;
  const int n_rows = r_end - r_begin + 1;
  const int n_iters = (n_rows + STEP - 1) / STEP;
  const int n_chunks = n_iters * CPI;

  if (wave == kTWaves) {
    // every chunk barrier waits for this wavefront's DMA issue and halo sums: it goes first on its SIMD (-4 %)
    __builtin_amdgcn_s_setprio(3);
    // ------------------------------ loader + halo wavefront ------------------------------
    const float* a_img = ac + ((long)f * C + c) * H * Wp + 4;      // +4: column c lives at c + 4
    const float* m0i = m0 + ((long)f * C + c) * H * Wp + 4;
    const float* v0i = v0 + ((long)f * C + c) * H * Wp + 4;
    const float* b_img = bc + (long)f * st1_frame_stride + (long)c * H * W1;
    const float* m1i = m1 + (long)f * st1_frame_stride + (long)c * H * W1;
    const float* v1i = v1 + (long)f * st1_frame_stride + (long)c * H * W1;
    const int c_lo = w_lo - 4;
    const int xb = c_lo - (dg * kTDG + kTDG - 1);                  // unclamped pattern column of span slot 0
    const int aq0 = min(c_lo + 4 * lane, Wp - 8), aq1 = min(c_lo + 256 + 4 * lane, Wp - 8);
    const int sq0 = min(xb + xoff + 4 * lane, W1 - 4), sq1 = min(xb + xoff + 256 + 4 * lane, W1 - 4);
    const bool a_tail = 256 + 4 * lane < kTA, s_tail = 256 + 4 * lane < kTSpanPad;
    auto issue_chunk = [&](int chunk) {
      float* buf = lds + (chunk % kTBufs) * (kTRows * kTPack);
#pragma unroll
      for (int s = 0; s < kTRows; ++s) {
        const int r = r_begin + chunk * kTRows + s;
        const int rc = clampi(r, 0, H - 1);
        const int hs = clampi(r - TAIL, 0, H - 1);
        float* pk = buf + s * kTPack;
        dma_quad(a_img + (long)rc * Wp + aq0, pk);
        dma_quad(m0i + (long)hs * Wp + aq0, pk + kTA);
        dma_quad(v0i + (long)hs * Wp + aq0, pk + 2 * kTA);
        dma_quad(b_img + (long)rc * W1 + sq0, pk + kTOffB);
        dma_quad(m1i + (long)hs * W1 + sq0, pk + kTOffB + kTSpanPad);
        dma_quad(v1i + (long)hs * W1 + sq0, pk + kTOffB + 2 * kTSpanPad);
        if (a_tail) {
          dma_quad(a_img + (long)rc * Wp + aq1, pk + 256);
          dma_quad(m0i + (long)hs * Wp + aq1, pk + kTA + 256);
          dma_quad(v0i + (long)hs * Wp + aq1, pk + 2 * kTA + 256);
        }
        if (s_tail) {
          dma_quad(b_img + (long)rc * W1 + sq1, pk + kTOffB + 256);
          dma_quad(m1i + (long)hs * W1 + sq1, pk + kTOffB + kTSpanPad + 256);
          dma_quad(v1i + (long)hs * W1 + sq1, pk + kTOffB + 2 * kTSpanPad + 256);
        }
      }
    };
    // halo job of this lane: consumer wave cw, disparity j, side (0 = quad left of the tile, 1 = right of it)
    const int cw = lane >> 2, hj = (lane >> 1) & 1, side = lane & 1;
    const bool has_job = lane < 4 * kTWaves;
    const int a_slot = side ? (kTA - 4) : 0;
    const int b_slot = a_slot + (kTDG - 1) - (cw * kTND + hj);
    float hP[4][2], hT[4][6];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hP[i][0] = hP[i][1] = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) hT[i][k] = 0.f;
    }
    // vertical ring update of the halo quad for the rows of one chunk; UB = ring phase of its first row
    auto halo_chunk = [&](int chunk, auto ub_tag) {
      constexpr int UB = decltype(ub_tag)::value;
      const float* buf = lds + (chunk % kTBufs) * (kTRows * kTPack);
#pragma unroll
      for (int s = 0; s < kTRows; ++s) {
        const int u = (UB + s) % 6;
        const float* pk = buf + s * kTPack;
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = has_job ? pk[a_slot + i] * pk[kTOffB + b_slot + i] : 0.f;
          const float t3 = p + hP[i][(u + 1) % 2] + hP[i][u % 2];
          hP[i][u % 2] = p;
          x[i] = t3 + hT[i][(u + 3) % 6] + hT[i][u % 6];
          hT[i][u % 6] = t3;
        }
        float o4[4];
        if (side) {                                                // prefix sums: columns 0..i of the right quad
          o4[0] = x[0]; o4[1] = o4[0] + x[1]; o4[2] = o4[1] + x[2]; o4[3] = o4[2] + x[3];
        } else {                                                   // suffix sums: columns i..3 of the left quad
          o4[3] = x[3]; o4[2] = o4[3] + x[2]; o4[1] = o4[2] + x[1]; o4[0] = o4[1] + x[0];
        }
        if (has_job) {
          float* hq = const_cast<float*>(pk) + kTOffH + lane * 4;  // lane == ((cw*kTND + hj)*2 + side)
          hq[0] = o4[0]; hq[1] = o4[1]; hq[2] = o4[2]; hq[3] = o4[3];
        }
      }
    };
    constexpr int L = kTRows * kTDmaPerRow;
    static_assert(L * (kTBufs - 2) < 64, "in-flight DMA count must fit vmcnt");
#pragma unroll
    for (int k = 0; k < kTBufs - 1; ++k)
      if (k < n_chunks) issue_chunk(k);
    if (n_chunks >= kTBufs - 1) wait_vmcnt<L*(kTBufs - 2)>(); else wait_vmcnt<0>();
    halo_chunk(0, std::integral_constant<int, 0>{});
    wait_lgkmcnt0();
    wg_barrier();
    for (int it = 0; it < n_iters; ++it) {
#pragma unroll
      for (int cc = 0; cc < CPI; ++cc) {
        const int ch = it * CPI + cc;
        const int nxt = ch + kTBufs - 1;
        if (nxt < n_chunks) {
          issue_chunk(nxt);
          wait_vmcnt<L*(kTBufs - 2)>();                       // chunk ch+1 has landed
        } else {
          wait_vmcnt<0>();
        }
        if (ch + 1 < n_chunks) {
          if (cc == 0) halo_chunk(ch + 1, std::integral_constant<int, (1 * kTRows) % 6>{});
          else if (cc == 1) halo_chunk(ch + 1, std::integral_constant<int, (2 * kTRows) % 6>{});
          else if (cc == 2) halo_chunk(ch + 1, std::integral_constant<int, (3 * kTRows) % 6>{});
          else if (cc == 3) halo_chunk(ch + 1, std::integral_constant<int, (4 * kTRows) % 6>{});
          else if (cc == 4) halo_chunk(ch + 1, std::integral_constant<int, (5 * kTRows) % 6>{});
          else halo_chunk(ch + 1, std::integral_constant<int, (6 * kTRows) % 6>{});
        }
        wait_lgkmcnt0();
        wg_barrier();
      }
    }
    return;
  }

  // two copies of the consumer loop: the sub-quad shift of the pattern-side operands alternates with the wave index
  if (wave & 1)
    t256_consume<ACCUM, (kTDG - 2 - kTND) % 4>(lds, out, wave, f, dg, lane, w_lo, h_lo, h_hi, r_begin, n_iters, H, W, D);
  else
    t256_consume<ACCUM, (kTDG - 2) % 4>(lds, out, wave, f, dg, lane, w_lo, h_lo, h_hi, r_begin, n_iters, H, W, D);
}

// block 9, W % 4 == 0, `out` 16-byte aligned; one accumulating launch per channel
int launch_t256(float* out, int frames, int C, int H, int W, int D, const FastWorkspace& ws, long st1_stride,
                hipStream_t stream) {
  // several channels (accumulating launches): 256-column tiles per disparity group, every store a full aligned KB
  const int n_dg = ceil_div(D, kTDG);
  const int n_tiles = ceil_div(W, kTTile);
  // Bands of ~44 rows (5.5x the (bs-1)-row warm-up).  Measured on config 2 (H = 432): 4 bands 0.448 ms, 8: 0.418,
  // 10: 0.394, 12: 0.398, 16: 0.439 -- short bands cost warm-up rows but interleave the store-free warm-up of
  // some workgroups with the store phase of others and even out the tail.
  const int bands = H >= 66 ? (H + 22) / 44 : 1;
  const int band_rows = ceil_div(H, bands);
  dim3 grid(n_tiles, ceil_div(H, band_rows), frames * n_dg), block(64 * (kTWaves + 1));
  const size_t lds = sizeof(float) * kTBufs * kTRows * kTPack;
  for (int c = 0; c < C; ++c) {
    auto kern = c == 0 ? ncc_fast_t256_kernel<false> : ncc_fast_t256_kernel<true>;
    if (lds > 64 * 1024)
      CTD_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    timing_begin(stream);
    hipLaunchKernelGGL(kern, grid, block, lds, stream, ws.ac, ws.m0, ws.v0, ws.bc, ws.m1, ws.v1, st1_stride, out, C, c, H,
                       W, D, band_rows, n_dg, ws.Wp, ws.W1, ws.xoff);
    timing_end(stream, W);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

}  // namespace ctd
