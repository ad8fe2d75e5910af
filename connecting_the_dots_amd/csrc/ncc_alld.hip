// ncc_alld.hip -- the all-D kernel of the fast NCC path (volume and / or in-kernel ranking, SAD / MSE cost volume), its
// plan and its one launcher (the stages of a call: ncc_fast.hip; the consumer pipeline it shares with the tile-256
// kernel is described in ncc_tiles.hip).
#include <type_traits>

#include "ctd_ncc_fast.h"
#include "ctd_rank.h"
#include "ctd_stamps.h"
#include "ctd_wave.h"

namespace ctd {

// ------------------------------------------------------------------------------------
// ALL-D kernel (bs == 9, W % 4 == 0, C == 1): volume + in-kernel ranking, what ctd_xcorrvol_argmax_f32 launches.
//
// Same consumer pipeline as the tile-256 kernel, but ONE workgroup owns a (256-column tile, band of rows, frame) for
// EVERY disparity: 15 consumer wavefronts + 1 loader (1024 threads, one workgroup per CU = four wavefronts on every
// SIMD), 2 disparities per lane, so a pass over the band covers up to 30 disparities and the workgroup makes
// ceil(D / 30) passes (dealt evenly: D = 128 -> 5 passes of 26 on 13 wavefronts, see alld_plan).  What that buys:
//   * the ranking state lives in LDS for the whole band -- two u32 slots {top, runner-up} per pixel, fed by LDS
//     atomics from all consumer wavefronts across all passes -- and what leaves the kernel is the final index (int64),
//     the best score, the work-list flag: no per-group partial planes (141 MB at config 2) and no merge kernel;
//   * the frame-side operands of the band are re-read by the SAME workgroup on every pass (the same CU, the same L2)
//     instead of by ten workgroups scattered over the eight XCDs' L2s;
//   * half the passes for the loader's DMA and halo work, 15 of 16 wavefronts computing instead of 7 of 8;
//   * at most 256 workgroups are resident: the store-only ceiling of exactly this pattern is 6.0-6.7 TB/s against
//     5.8-6.0 for the per-group grid (profiles/round3_store_ceiling.txt).
// KEY of a score: t = 6 + score lies in [4, 8) for every |score| <= 1 + 1e-5, where consecutive floats are 2^-21 apart
// and ordered like their bit patterns: key = (bits(t) << 9) | (511 - d) is an unsigned integer ordered by score first
// (absolute resolution 2^-21 = 4.8e-7, against 2^-19 RELATIVE for the mantissa-tag keys it replaces) and by LOWER
// disparity second -- so u32 maxima carry the argmax with first-index-wins ties.  Per pixel:
//     old = ds_max_rtn_u32(top, hi);  ds_max_u32(second, med3(old, hi, lo))      (hi >= lo: the lane's two keys)
// -- every key that is not the final maximum is, at some point, the loser of such an exchange, so `second` ends up as
// the runner-up; the second atomic rides on the next row (its operand is the first one's return value).
// Scores of LISTED windows: the pre-pass stores a zero reciprocal deviation for them, so the kernels produce the
// placeholder score 0 for exactly the outputs the fix-up pass recomputes.  A placeholder can only matter for the
// ranking if it comes out on top or within the margin of the top: ncc_fixup_kernel sends a pixel to the exact
// re-scoring when the exact score is a contender OR when the pixel's index is the placeholder's disparity.  Scores past
// the start of the fully clamped run (ext.h:152-154 makes them copies of its first element) get key 0.
// ------------------------------------------------------------------------------------
constexpr int kAWaves = 15;                    // consumer wavefronts per workgroup
constexpr int kADGMax = kAWaves * 2;           // disparities per pass, at most
constexpr int kAA = 256 + 8;                   // frame-side array: 4 halo columns either side
constexpr int kASpanPad = (kAA + kADGMax - 1 + 1 + 3) / 4 * 4;   // 296: multiple of 4, > span
static_assert(kAA + kADGMax - 1 < kASpanPad, "pattern span must fit its padded array");
constexpr int kAHalo = kAWaves * 2 * 2 * 4;    // [wave][j][side][4] halo sums
constexpr int kAPack = 3 * kAA + 3 * kASpanPad + kAHalo;   // 1920 floats per staged row
constexpr int kABufs = 3;                     // LDS chunks in the ring; a chunk is ROWS = 3 or 2 staged rows (template parameter)
constexpr int kAOffB = 3 * kAA, kAOffH = 3 * kAA + 3 * kASpanPad;
// band height limit: rank slots (2 KB per row) + staging ring <= 160 KB -- 44 rows with 3-row chunks, 57 with 2-row chunks
constexpr int alld_max_band_rows(int rows) { return (160 * 1024 - (int)sizeof(float) * kABufs * rows * kAPack) / 2048; }
constexpr int kAllowTwoRowChunks = 2;           // 3: never use 2-row chunks
constexpr double kTwoRowPenalty = 1.03;
constexpr int kTagBits = 9;                    // D <= 512
constexpr unsigned kTagMask = (1u << kTagBits) - 1u;
constexpr float kKeyBias = 6.f;
static_assert(alld_max_band_rows(3) == 46 && alld_max_band_rows(2) == 57, "LDS budget");

__device__ inline unsigned umed3(unsigned a, unsigned b, unsigned c) {
  unsigned r;
  asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// fixed-point units of the keys per unit of score, and the re-ranking margin in those units (ctd_rank.h: rank_margin)
__device__ inline unsigned key_margin_units(float eps) { return (unsigned)ceilf(rank_margin(eps, 1.f) * 2097152.f); }

// where the diagnostic stamps (ctd_stamps.h) of a workgroup live: behind its staging ring
#define CTD_STAMP_AREA(ring, rows) ((unsigned*)((ring) + kABufs * (rows) * kAPack))

// JM: which of the pair's two disparities this wavefront works on -- 3 = both (the regular consumer), 1 = j 0 only,
// 2 = j 1 only: the two halves of a SPLIT pair, run by two wavefronts on different SIMDs (see the kernel: with 13 pairs
// per pass the thirteenth pair would otherwise put a fourth full consumer on one SIMD and the chunk barrier makes
// everybody wait for that SIMD).  WAVE is the PAIR index (span slots, halo slots, disparity base); `wave_id` the
// wavefront's own number (diagnostic stamps only).
template <int MODE, int KS, int ROWS, int JM = 3>
__device__ __forceinline__ void alld_consume(float* lds, unsigned* rank_lds, float* __restrict__ out, int WAVE, int f,
                                             int lane, int w_lo, int h_lo, int h_hi, int r_begin, int n_iters,
                                             int n_pass, int rot, int dgs, int H, int W, int D, int wave_id) {
  constexpr int J0 = (JM & 1) ? 0 : 1;                             // first active j
  constexpr int TAIL = 4, STEP = 6, CPI = STEP / ROWS;            // block size 9
  constexpr bool STORE = (MODE & kAStore) != 0, RANK = (MODE & kARank) != 0;
  static_assert(STEP % ROWS == 0, "a chunk never straddles two outer iterations");
  const long HW = (long)H * W;
  const unsigned l4 = 4u * (unsigned)lane;                         // first column of the lane, relative to w_lo
  float* vol = out + (long)f * D * HW + w_lo;
  const bool lane_out = w_lo + (int)l4 < W;
  float P[2][4][2], T[2][4][6];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      P[j][i][0] = P[j][i][1] = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) T[j][i][k] = 0.f;
    }
  const int kOff0 = (dgs - 1) - WAVE * 2;                          // span slot offset of disparity j = 0
  const int kQ = (kOff0 - 1) / 4;                                  // disparity j = 1 sits one span slot below j = 0:
  constexpr int kS = KS;                                           // both come out of the same two aligned quads
  const int halo4 = lane == 63 ? 4 : 0;
  const float halo_mask = (lane == 0 || lane == 63) ? 1.f : 0.f;  // (multiplicative: see t256_consume)
  auto quad = [](const float* p) { return *(const f32x4*)p; };

  // The runner-up update needs the value the first atomic returns: it is issued at the start of the next row, behind
  // that row's operand reads -- LDS answers in order, so the returns are there by the time the operands are.
  // Unconditional (a row without outputs leaves key 0 here, a no-op for the maximum): a flag would keep these twelve
  // registers alive across the whole loop.
  unsigned rk_hi[4], rk_lo[4], rk_old[4];
  unsigned* rk_sl = rank_lds + lane;
#pragma unroll
  for (int i = 0; i < 4; ++i) rk_hi[i] = rk_lo[i] = rk_old[i] = 0u;
  auto rank_second = [&]() {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      (void)__hip_atomic_fetch_max(rk_sl + 256 + 64 * i, umed3(rk_old[i], rk_hi[i], rk_lo[i]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_WORKGROUP);
  };

  wg_barrier();                                                    // chunk 0 (operands + halos) and the cleared slots are in LDS
  int slot = 0;                                                    // ring slot of the current chunk
  f32x4 qa, qb0, qb1;                                              // value quads of the row (frame, pattern x 2)
  for (int pass = 0; pass < n_pass; ++pass) {
    const int grp = pass + rot;                                    // (rot: the workgroup's first disparity group)
    const int d_base = grp * dgs + WAVE * 2;
    if (WAVE * 2 >= dgs || d_base + J0 >= D) {
      // a wavefront without disparities in this pass (the pass is narrower than 15 pairs, or it is the last pass and
      // both disparities lie past D): keep the barrier protocol, skip the work
      for (int k = 0; k < n_iters * CPI; ++k) {
        CTD_STAMP_ARRIVE(CTD_STAMP_AREA(lds, ROWS), wave_id, pass, k, lane);
        wg_barrier();
        CTD_STAMP_LEAVE(CTD_STAMP_AREA(lds, ROWS), wave_id, pass, k, lane);
        slot = slot == kABufs - 1 ? 0 : slot + 1;
      }
      continue;
    }
    const unsigned tag0 = kTagMask - (unsigned)d_base;             // key tag of disparity j = 0 (j = 1: one less)
    // only the first column tile can reach the fully clamped run (d > w + TAIL needs d_base + 1 > w_lo + TAIL)
    const bool run_masks = d_base + 1 > w_lo + TAIL;
    for (int it = 0; it < n_iters; ++it) {
#pragma unroll
      for (int u = 0; u < STEP; ++u) {
        const int r = r_begin + it * STEP + u;
        const bool last_of_chunk = (u % ROWS) == ROWS - 1;
        // (addressing: one opaque per-row scalar plus one of two loop-invariant lane registers, see t256_consume)
        int row_o = (slot * ROWS + (u % ROWS)) * kAPack + 4;
        asm("" : "+s"(row_o));
        int own_o = row_o + (int)l4;
        asm("" : "+v"(own_o));
        const float* own = lds + own_o;                            // own quad after the left halo
        int pat_s = row_o + kAOffB + 4 * kQ;
        asm("" : "+s"(pat_s));
        int pat_o = pat_s + (int)l4;
        asm("" : "+v"(pat_o));
        const float* pat = lds + pat_o;                            // first of the lane's two pattern-side quads
        int hq_s = row_o - 4 + kAOffH + WAVE * (2 * 2 * 4);
        asm("" : "+s"(hq_s));
        int hq_o = hq_s + halo4;
        asm("" : "+v"(hq_o));
        const float* hqp = lds + hq_o;                             // halo sums of (this wave, j 0) on this lane's side
        // The value quads of a chunk's first row are read here; those of its other rows were requested at the end of
        // the previous row, AHEAD of that row's returning atomics: LDS answers in order, and a read queued behind the
        // atomics would make phase A wait for their round trip.
        if ((u % ROWS) == 0) {
          qa = quad(own);
          qb0 = quad(pat);
          qb1 = quad(pat + 4);
        }
        asm("" : "+v"(qa), "+v"(qb0), "+v"(qb1));
        const float av[4] = {qa[0], qa[1], qa[2], qa[3]};
        const float be[8] = {qb0[0], qb0[1], qb0[2], qb0[3], qb1[0], qb1[1], qb1[2], qb1[3]};
        const int h = r - TAIL;
        const bool row_out = (h >= h_lo) && (h < h_hi);           // wave-uniform
        // 9-row sums as 3 x 3: t3 = rows r-2 .. r of the products, x = t3 of rows r, r-3, r-6.  The two OLD ring entries
        // are added first and die there, so the new entry (p, t3) can take the register of the one it replaces: summed
        // as (p + P') + P the new and the old value were live together and every ring slot cost a v_mov at the loop's
        // back edge (48 of 979 vector instructions per 6 rows).
        float x[2][4];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (!(JM & (1 << j))) continue;
            float sP = P[j][i][(u + 1) % 2] + P[j][i][u % 2];
            float sT = T[j][i][(u + 3) % 6] + T[j][i][u % 6];
            asm("" : "+v"(sP), "+v"(sT));                          // (formed before the slots are reused)
            float p;                                               // b[j][i] = slot kOff0 - j + i
            if constexpr ((MODE & kASad) != 0) {
              p = fabsf(av[i] - be[kS + (1 - j) + i]);
            } else if constexpr ((MODE & kAMse) != 0) {
              const float df = av[i] - be[kS + (1 - j) + i];
              p = df * df;
            } else {
              p = av[i] * be[kS + (1 - j) + i];
            }
            const float t3 = p + sP;
            P[j][i][u % 2] = p;
            x[j][i] = t3 + sT;
            T[j][i][u % 6] = t3;
          }
        // previous output row's runner-up update (possibly of the previous chunk): its returns are in by now
        if constexpr (RANK) rank_second();
        auto prefetch_next = [&]() {                               // next row of the same chunk: one ring row further
          if (!last_of_chunk) {
            qa = quad(own + kAPack);
            qb0 = quad(pat + kAPack);
            qb1 = quad(pat + kAPack + 4);
          }
        };
        if (row_out) {
          constexpr bool COST = (MODE & (kASad | kAMse)) != 0;      // SAD / MSE cost volume: no statistics, no normalisation
          f32x4 qma, qsa, qm0, qm1, qs0, qs1;
          if constexpr (!COST) {
            qma = quad(own + kAA), qsa = quad(own + 2 * kAA);
            qm0 = quad(pat + kASpanPad), qm1 = quad(pat + kASpanPad + 4);
            qs0 = quad(pat + 2 * kASpanPad), qs1 = quad(pat + 2 * kASpanPad + 4);
          }
          float me[8], se[8];
          unsigned key[2][4];
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            if (!(JM & (1 << j))) continue;
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
            window_combine4(suf, pre[3], pre, sj);                  // wave-edge lanes get 0 from the missing neighbour
            if constexpr (!COST) {
              if (j == J0) {
                // statistics quads: pinned after the first window sums (data dependency keeps the wait here)
                asm("" : "+v"(qma), "+v"(qsa), "+v"(qm0), "+v"(qm1) : "v"(sj[0]), "v"(sj[3]));
                asm("" : "+v"(qs0), "+v"(qs1) : "v"(sj[0]), "v"(sj[3]));
#pragma unroll
                for (int k = 0; k < 4; ++k) { me[k] = qm0[k]; me[4 + k] = qm1[k]; se[k] = qs0[k]; se[4 + k] = qs1[k]; }
              }
            }
            f32x4 hq = quad(hqp + j * 2 * 4);
            asm("" : "+v"(hq));
            const int d = d_base + j;
            float val[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float sh = fmaf(halo_mask, hq[i], sj[i]);
              if constexpr (COST) {
                val[i] = sh * (1.f / 81.f);                         // mean over the 9 x 9 block
              } else {
                const float cov = fmaf(qma[i], me[kS + (1 - j) + i], sh);   // qma = -bs^2 * (window mean), from the pre-pass
                const float inv = ncc_inv_norm(qsa[i], se[kS + (1 - j) + i]);
                if (STORE) val[i] = cov * inv;                      // the same bits as the plain volume kernels'
                if constexpr (RANK) key[j][i] = (__float_as_uint(fmaf(cov, inv, kKeyBias)) << kTagBits) | (tag0 - (unsigned)j);
              }
            }
            if (STORE && lane_out && d < D) {
              long ooff = (long)d * HW + (long)h * W;
              asm("" : "+s"(ooff));
              // written once, next read by another kernel after 1.8 GB more: non-temporal
              __builtin_nontemporal_store(f32x4{val[0], val[1], val[2], val[3]}, (f32x4*)(vol + ooff + l4));
            }
            if constexpr (RANK) {
              if (d < D) {                                         // wave-uniform branch (a select would be 4 VALU slots)
                if (run_masks) {                                   // wave-uniform: first column tile only
                  // d > w + TAIL: copy of the run's first element.  Loop-invariant compare: hoisted into a lane mask.
#pragma unroll
                  for (int i = 0; i < 4; ++i)
                    if (d - TAIL - i - w_lo > (int)l4) key[j][i] = 0u;
                }
              } else {
                // (volatile: as plain assignments the compiler runs these four moves on EVERY row, ahead of the branch)
#pragma unroll
                for (int i = 0; i < 4; ++i) asm volatile("v_mov_b32 %0, 0" : "=v"(key[j][i]));
              }
            }
          }
          prefetch_next();
          if constexpr (RANK) {
            // slots of output row h: [row][top | second][column-in-quad][lane]
            rk_sl = rank_lds + (it * STEP + u - 2 * TAIL) * 512 + lane;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              if (JM == 3) {
                rk_hi[i] = max(key[0][i], key[1][i]);
                rk_lo[i] = min(key[0][i], key[1][i]);
              } else {
                rk_hi[i] = key[J0][i];                             // one key per pixel and row: the loser of the exchange
                rk_lo[i] = 0u;                                     // with the slot's top is min(old, key) = med3(old, key, 0)
              }
              rk_old[i] = __hip_atomic_fetch_max(rk_sl + 64 * i, rk_hi[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
          }
        } else {
          prefetch_next();
          if constexpr (RANK) {
            // only the returned old top is reset: the next rank_second() then offers min(hi, lo) of the last output row
            // once more -- a genuine non-top key of that pixel, harmless
#pragma unroll
            for (int i = 0; i < 4; ++i) rk_old[i] = 0u;
          }
        }
        if (last_of_chunk) {
          // the pass's last chunk has no next row to ride on: complete its slots before its barrier (wave-uniform)
          if constexpr (RANK) {
            if (it == n_iters - 1 && u == STEP - 1) {
              rank_second();
#pragma unroll
              for (int i = 0; i < 4; ++i) rk_hi[i] = rk_lo[i] = rk_old[i] = 0u;
            }
          }
          wait_lgkmcnt0();
          // (not in the volume + ranking instantiation: with the stamps' scalars on top hipcc 7.2 fails to spill its
          // scalar registers -- "illegal VGPR to SGPR copy"; the timeline is taken in the two other modes)
          if constexpr (MODE != (kAStore | kARank)) CTD_STAMP_ARRIVE(CTD_STAMP_AREA(lds, ROWS), wave_id, pass, it * CPI + u / ROWS, lane);
          wg_barrier();
          if constexpr (MODE != (kAStore | kARank)) CTD_STAMP_LEAVE(CTD_STAMP_AREA(lds, ROWS), wave_id, pass, it * CPI + u / ROWS, lane);
          slot = slot == kABufs - 1 ? 0 : slot + 1;
        }
      }
    }
  }
}

// What the statistics DMAs of a chunk need (either loader).
struct AlldStatsArgs {
  const float *m0i, *v0i, *m1i, *v1i;       // this frame's mean / reciprocal-deviation planes (frame side: column c at c + 4)
  float* lds;                               // staging ring
  int Wp, W1, xoff, c_lo, r_begin, h_lo, h_hi, n_pass, n_chunks, dgs, first_grp;
};
constexpr int kAStatsPerRow = 8, kAValuesPerRow = 4;   // dwordx4 LDS-DMA instructions per staged row

// statistics rows of chunk (pass ip, chunk ic) into ring slot `sl`
template <int ROWS>
__device__ __forceinline__ void alld_issue_stats(const AlldStatsArgs& a, int ip, int ic, int sl, int lane) {
  constexpr int TAIL = 4;
  const int aq0 = min(a.c_lo + 4 * lane, a.Wp - 8), aq1 = min(a.c_lo + 256 + 4 * lane, a.Wp - 8);
  const bool a_tail = 256 + 4 * lane < kAA, s_tail = 256 + 4 * lane < kASpanPad;
  float* buf = a.lds + sl * (ROWS * kAPack);
  const int xb = a.c_lo - ((ip + a.first_grp) * a.dgs + a.dgs - 1);   // unclamped pattern column of span slot 0
  const int sq0 = min(xb + a.xoff + 4 * lane, a.W1 - 4), sq1 = min(xb + a.xoff + 256 + 4 * lane, a.W1 - 4);
#pragma unroll
  for (int s2 = 0; s2 < ROWS; ++s2) {
    const int r = a.r_begin + ic * ROWS + s2;
    // statistics of output row r - TAIL (rows of a mixed chunk that complete no output re-read a row the band needs anyway)
    const int hs = clampi(r - TAIL, a.h_lo, a.h_hi - 1);
    float* pk = buf + s2 * kAPack;
    dma_quad(a.m0i + (long)hs * a.Wp + aq0, pk + kAA);
    dma_quad(a.v0i + (long)hs * a.Wp + aq0, pk + 2 * kAA);
    dma_quad(a.m1i + (long)hs * a.W1 + sq0, pk + kAOffB + kASpanPad);
    dma_quad(a.v1i + (long)hs * a.W1 + sq0, pk + kAOffB + 2 * kASpanPad);
    if (a_tail) {
      dma_quad(a.m0i + (long)hs * a.Wp + aq1, pk + kAA + 256);
      dma_quad(a.v0i + (long)hs * a.Wp + aq1, pk + 2 * kAA + 256);
    }
    if (s_tail) {
      dma_quad(a.m1i + (long)hs * a.W1 + sq1, pk + kAOffB + kASpanPad + 256);
      dma_quad(a.v1i + (long)hs * a.W1 + sq1, pk + kAOffB + 2 * kASpanPad + 256);
    }
  }
}

// a chunk is LIGHT when none of its rows completes an output row of the band (the 8 warm-up rows of a pass and the padding
// behind the last output row): nobody reads statistics there, none are staged
template <int ROWS>
__device__ __forceinline__ bool alld_chunk_is_light(int ch, int n_out_rows) {
  return ch * ROWS + ROWS - 1 < 8 || ch * ROWS >= 8 + n_out_rows;
}

// The second loader (a spare consumer wavefront, see the roles in the kernel): the statistics rows, two chunks ahead,
// in step with the chunk barriers; before each barrier everything but the newest chunk has landed.
template <int ROWS>
__device__ __forceinline__ void alld_stats_loader(const AlldStatsArgs& a, int lane) {
  constexpr int LS = ROWS * kAStatsPerRow;
  static_assert(LS < 64, "in-flight DMA count must fit vmcnt");
  __builtin_amdgcn_s_setprio(3);
  const int total = a.n_pass * a.n_chunks, n_out_rows = a.h_hi - a.h_lo;
  int i_slot = 0, i_pass = 0, i_ch = 0, i_n = 0;
  auto issue_next = [&]() {                                        // returns whether anything was issued
    const bool light = alld_chunk_is_light<ROWS>(i_ch, n_out_rows);
    if (!light) alld_issue_stats<ROWS>(a, i_pass, i_ch, i_slot, lane);
    ++i_n;
    i_slot = i_slot == kABufs - 1 ? 0 : i_slot + 1;
    if (++i_ch == a.n_chunks) { i_ch = 0; ++i_pass; }
    return !light;
  };
  issue_next();
  if (issue_next()) wait_vmcnt<LS>(); else wait_vmcnt<0>();        // chunk 0 has landed
  wg_barrier();
  int c_pass = 0, c_ch = 0;                                        // the chunk the consumers are working on (stamps)
  (void)c_pass;
  for (int g = 0; g < total; ++g) {
    if (i_n < total) {
      if (issue_next()) wait_vmcnt<LS>(); else wait_vmcnt<0>();    // chunk g + 1 has landed
    } else {
      wait_vmcnt<0>();
    }
    CTD_STAMP_ARRIVE(CTD_STAMP_AREA(a.lds, ROWS), kAWaves - 1, c_pass, c_ch, lane);
    wg_barrier();
    CTD_STAMP_LEAVE(CTD_STAMP_AREA(a.lds, ROWS), kAWaves - 1, c_pass, c_ch, lane);
    if (++c_ch == a.n_chunks) { c_ch = 0; ++c_pass; }
  }
}

// MODE_STORE: the volume is materialised as well; otherwise nothing but indices / best scores / work list leave.
template <int MODE, int ROWS>
__global__ __launch_bounds__(64 * (kAWaves + 1)) void ncc_fast_alld_kernel(
    const float* __restrict__ ac, const float* __restrict__ m0, const float* __restrict__ v0,
    const float* __restrict__ bc, const float* __restrict__ m1, const float* __restrict__ v1, long st1_frame_stride,
    float* __restrict__ out, int64_t* __restrict__ idx_out, float* __restrict__ best_out,
    unsigned char* __restrict__ flags_out, WorkList work, float rank_eps, int frames, int n_items, int H, int W, int D,
    int band_rows, int n_pass_all, int dgs, int Wp, int W1, int xoff, int n_psplit) {
  constexpr int HALF = 4, TAIL = 4, STEP = 6, CPI = STEP / ROWS;
  // [band_rows][top | second][256] rank slots first (their row base goes into one lane register), then the staging ring
  extern __shared__ float lds_all[];
  constexpr bool RANK = (MODE & kARank) != 0;
  unsigned* rank_lds = (unsigned*)lds_all;
  float* lds = lds_all + (RANK ? band_rows * 512 : 0);             // [kABufs][ROWS][kAPack]
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // Work item of this workgroup: column tile fastest, then band, then frame.  (XCD-aware orders -- every XCD a
  // contiguous range of the band-major list, so that co-resident workgroups share pattern rows in its L2 -- cut the
  // operand fetches from 2 x 99 to 2 x 59-68 MiB and were 1-2.5 % SLOWER in four A/B runs: the kernel is bound by vector
  // issue, not by its 5-10 % of operand traffic.  Pass order rotated per workgroup: slower as well.)
  // Calls with few frames (one 1024 x 1024 frame is 4 column tiles) would need short bands to fill the chip, and every
  // band pays 8 warm-up rows per pass: without a ranking the DISPARITY GROUPS of an item can go to `n_psplit` different
  // workgroups instead (pass split fastest in the item number), each walking its share of the passes over a tall band.
  int item = (int)blockIdx.x;
  if (item >= n_items) return;                                     // whole workgroup, before any barrier
  const int ps = item % n_psplit;
  item /= n_psplit;
  const int ppg = (n_pass_all + n_psplit - 1) / n_psplit;          // passes per workgroup
  const int rot = ps * ppg;                                        // first disparity group of this workgroup
  const int n_pass = min(ppg, n_pass_all - rot);
  if (n_pass <= 0) return;
  const int n_tiles = (W + 255) / 256;
  const int n_bands = n_items / (frames * n_tiles * n_psplit);
  const int w_lo = (item % n_tiles) * 256;
  const int band = (item / n_tiles) % n_bands;
  const int f = item / (n_tiles * n_bands);
  const int h_lo = band * band_rows;
  const int h_hi = min(h_lo + band_rows, H);
  const int r_begin = h_lo - HALF, r_end = h_hi - 1 + TAIL;
  const int n_rows = r_end - r_begin + 1;
  const int n_iters = (n_rows + STEP - 1) / STEP;
  const int n_chunks = n_iters * CPI;                              // per pass; a multiple of CPI
  const int n_act = dgs / 2;                                       // consumer wavefronts with work
  CTD_STAMP_BEGIN(CTD_STAMP_AREA(lds, ROWS), n_chunks);

  // every wavefront clears its share of the rank slots (key 0 = below every score)
  if constexpr (RANK)
    for (int k = threadIdx.x; k < band_rows * 128; k += 64 * (kAWaves + 1)) ((uint4*)rank_lds)[k] = make_uint4(0u, 0u, 0u, 0u);
  wait_lgkmcnt0();                                                 // (the consumers' first barrier is a raw s_barrier)

  // ---- roles.  Pairs of disparities per pass: n_act = dgs / 2 (13 for D = 128).  The chunk barrier makes every
  // wavefront wait for the slowest SIMD, and wavefront w sits on SIMD w % 4 (the timeline of the -DCTD_STAMPS build:
  // profiles/round4_alld_timeline.txt), so the roles are dealt to even out the four SIMDs:
  //   * wavefront 15: loader of the VALUE rows (frame and pattern samples) + the halo sums;
  //   * with a spare wavefront (n_act <= 14), wavefront 14 is a second loader for the STATISTICS rows (mean / reciprocal
  //     deviation planes, needed by output rows only): the halo sums need the values alone, so nobody waits for it
  //     but the barrier, and the first loader's chunk drops from 24 DMA instructions to 8;
  //   * with two spare wavefronts (n_act == 13) the last pair is SPLIT: wavefront 12 takes its first disparity,
  //     wavefront 13 the second -- SIMDs 0 and 1 then carry 3.5 pairs each, 2 and 3 carry 3 pairs and a loader,
  //     instead of 4 / 3 / 3 / 3 + loader.
  constexpr bool COST = (MODE & (kASad | kAMse)) != 0;             // SAD / MSE cost volume: value rows only, no statistics
  const bool has_helper = !COST && n_act <= kAWaves - 1;
  const bool split_last = n_act == kAWaves - 2;
  const int n_out_rows = h_hi - h_lo;
  auto chunk_is_light = [&](int ch) { return alld_chunk_is_light<ROWS>(ch, n_out_rows); };
  constexpr int LV = ROWS * kAValuesPerRow, LS = ROWS * kAStatsPerRow;   // DMA instructions per chunk: values, statistics
  static_assert(LV + LS < 64, "in-flight DMA count must fit vmcnt");
  static_assert(kABufs == 3, "the loaders run two chunks ahead of the consumers");
  const int c_lo = w_lo - 4;
  const int total = n_pass * n_chunks;                             // chunks of the whole workgroup, all passes
  const AlldStatsArgs sa = {m0 + (long)f * H * Wp + 4, v0 + (long)f * H * Wp + 4, m1 + (long)f * st1_frame_stride,
                            v1 + (long)f * st1_frame_stride, lds, Wp, W1, xoff, c_lo, r_begin, h_lo, h_hi, n_pass, n_chunks, dgs, rot};

  if (wave == kAWaves - 1 && has_helper) {
    // ------------------------------ statistics loader (spare consumer wavefront) ------------------------------
    alld_stats_loader<ROWS>(sa, lane);
    CTD_STAMP_DUMP(CTD_STAMP_AREA(lds, ROWS));
    return;                                                        // (the emit rows are dealt to the consumer wavefronts only)
  }
  if (wave == kAWaves) {
    // every chunk barrier waits for this wavefront's DMA issue and halo sums: it goes first on its SIMD
    __builtin_amdgcn_s_setprio(3);
    // ------------------------------ value loader + halo wavefront ------------------------------
    const float* a_img = ac + (long)f * H * Wp + 4;
    const float* b_img = bc + (long)f * st1_frame_stride;
    const int aq0 = min(c_lo + 4 * lane, Wp - 8), aq1 = min(c_lo + 256 + 4 * lane, Wp - 8);
    const bool a_tail = 256 + 4 * lane < kAA, s_tail = 256 + 4 * lane < kASpanPad;
    int i_slot = 0, i_pass = 0, i_ch = 0, i_n = 0;                 // the next chunk to issue: ring slot, pass, chunk in the pass
    auto issue_chunk = [&]() {                                     // returns whether the statistics went with it
      float* buf = lds + i_slot * (ROWS * kAPack);
      const int i_grp = i_pass + rot;
      const int xb = c_lo - (i_grp * dgs + dgs - 1);               // unclamped pattern column of span slot 0
      const int sq0 = min(xb + xoff + 4 * lane, W1 - 4), sq1 = min(xb + xoff + 256 + 4 * lane, W1 - 4);
#pragma unroll
      for (int s2 = 0; s2 < ROWS; ++s2) {
        const int r = r_begin + i_ch * ROWS + s2;
        const int rc = clampi(r, 0, H - 1);
        float* pk = buf + s2 * kAPack;
        dma_quad(a_img + (long)rc * Wp + aq0, pk);
        dma_quad(b_img + (long)rc * W1 + sq0, pk + kAOffB);
        if (a_tail) dma_quad(a_img + (long)rc * Wp + aq1, pk + 256);
        if (s_tail) dma_quad(b_img + (long)rc * W1 + sq1, pk + kAOffB + 256);
      }
      const bool with_stats = !COST && !has_helper && !chunk_is_light(i_ch);
      if (with_stats) alld_issue_stats<ROWS>(sa, i_pass, i_ch, i_slot, lane);
      ++i_n;
      i_slot = i_slot == kABufs - 1 ? 0 : i_slot + 1;
      if (++i_ch == n_chunks) { i_ch = 0; ++i_pass; }
      return with_stats;
    };
    // halo job of this lane: consumer pair cw, disparity j, side (0 = quad left of the tile, 1 = right of it)
    const int cw = lane >> 2, hj = (lane >> 1) & 1, side = lane & 1;
    const bool has_job = cw < n_act;
    const int a_slot = side ? (kAA - 4) : 0;
    const int b_slot = has_job ? a_slot + (dgs - 1) - (cw * 2 + hj) : 0;
    // SAD / MSE: right of the image the per-pixel plane is a COPY of its last column (the tap column is clamped before
    // the shift), not the pairing a[W-1], b[w0 - d] of the NCC border rule: the four halo columns right of the LAST tile
    // all take the pattern sample of column W - 1 (span slot b_slot - 1).  (Images that end inside a tile: see
    // cost_border_kernel.)
    const bool copy_last = COST && side == 1 && w_lo + 256 == W;
    float hP[4][2], hT[4][6];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      hP[i][0] = hP[i][1] = 0.f;
#pragma unroll
      for (int k = 0; k < 6; ++k) hT[i][k] = 0.f;
    }
    // vertical ring update of the halo quad for the rows of one chunk; UB = ring phase of its first row.  (The rings
    // run on across passes: the first 8 rows of a pass are warm-up rows, whatever the rings held before.)
    int h_slot = 0;                                                // ring slot of the next chunk to get its halo sums
    auto halo_chunk = [&](auto ub_tag) {
      constexpr int UB = decltype(ub_tag)::value;
      const float* buf = lds + h_slot * (ROWS * kAPack);
#pragma unroll
      for (int s2 = 0; s2 < ROWS; ++s2) {
        const int u = (UB + s2) % 6;
        const float* pk = buf + s2 * kAPack;
        float x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float p2 = 0.f;
          if (has_job) {
            const float av = pk[a_slot + i], bv = pk[kAOffB + (copy_last ? b_slot - 1 : b_slot + i)];
            p2 = (MODE & kASad) ? fabsf(av - bv) : ((MODE & kAMse) ? (av - bv) * (av - bv) : av * bv);
          }
          const float t3 = p2 + hP[i][(u + 1) % 2] + hP[i][u % 2];
          hP[i][u % 2] = p2;
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
          float* hq = const_cast<float*>(pk) + kAOffH + lane * 4;  // lane == ((cw*2 + hj)*2 + side)
          hq[0] = o4[0]; hq[1] = o4[1]; hq[2] = o4[2]; hq[3] = o4[3];
        }
      }
      h_slot = h_slot == kABufs - 1 ? 0 : h_slot + 1;
    };
    // after issuing chunk X (LV value DMAs, + LS statistics DMAs when it carried them) everything older has landed once
    // at most that many are outstanding
    auto wait_older = [&](bool with_stats) {
      if (with_stats) wait_vmcnt<LV + LS>(); else wait_vmcnt<LV>();
    };
    issue_chunk();                                                 // total >= 2 (a pass has CPI >= 2 chunks)
    wait_older(issue_chunk());                                     // chunk 0 has landed
    halo_chunk(std::integral_constant<int, 0>{});
    wait_lgkmcnt0();
    wg_barrier();
    // chunk g of the flat sequence is chunk g % n_chunks of pass g / n_chunks; n_chunks is a multiple of CPI, so the
    // ring phase of the first row of chunk g is (g % CPI) * ROWS, across pass boundaries too
    for (int g = 0; g < total; g += CPI) {
#pragma unroll
      for (int cc = 0; cc < CPI; ++cc) {
        if (i_n < total) {
          wait_older(issue_chunk());                               // chunk g + cc + 1 has landed
        } else {
          wait_vmcnt<0>();
        }
        if (g + cc + 1 < total) {
          if (cc == 0) halo_chunk(std::integral_constant<int, (1 % CPI) * ROWS>{});
          else if (cc == 1) halo_chunk(std::integral_constant<int, (2 % CPI) * ROWS>{});
          else halo_chunk(std::integral_constant<int, (3 % CPI) * ROWS>{});
        }
        wait_lgkmcnt0();
        CTD_STAMP_ARRIVE(CTD_STAMP_AREA(lds, ROWS), kAWaves, (g + cc) / n_chunks, (g + cc) % n_chunks, lane);
        wg_barrier();
        CTD_STAMP_LEAVE(CTD_STAMP_AREA(lds, ROWS), kAWaves, (g + cc) / n_chunks, (g + cc) % n_chunks, lane);
      }
    }
    CTD_STAMP_DUMP(CTD_STAMP_AREA(lds, ROWS));
    return;
  }

  // Consumers.  Two copies of the regular loop -- the sub-quad shift of the pattern-side operands, (dgs - 2 - 2 * pair) % 4,
  // alternates with the pair index -- and, for a split last pair, one copy per half.
  {
    const int pair = (split_last && wave == n_act) ? n_act - 1 : wave;
    const bool ks2 = ((dgs - 2 - 2 * pair) & 2) != 0;
    if (split_last && wave >= n_act - 1) {
      if (wave == n_act - 1) {
        if (ks2) alld_consume<MODE, 2, ROWS, 1>(lds, rank_lds, out, pair, f, lane, w_lo, h_lo, h_hi, r_begin, n_iters, n_pass, rot, dgs, H, W, D, wave);
        else alld_consume<MODE, 0, ROWS, 1>(lds, rank_lds, out, pair, f, lane, w_lo, h_lo, h_hi, r_begin, n_iters, n_pass, rot, dgs, H, W, D, wave);
      } else {
        if (ks2) alld_consume<MODE, 2, ROWS, 2>(lds, rank_lds, out, pair, f, lane, w_lo, h_lo, h_hi, r_begin, n_iters, n_pass, rot, dgs, H, W, D, wave);
        else alld_consume<MODE, 0, ROWS, 2>(lds, rank_lds, out, pair, f, lane, w_lo, h_lo, h_hi, r_begin, n_iters, n_pass, rot, dgs, H, W, D, wave);
      }
    } else if (ks2) {
      alld_consume<MODE, 2, ROWS>(lds, rank_lds, out, pair, f, lane, w_lo, h_lo, h_hi, r_begin, n_iters, n_pass, rot, dgs, H, W, D, wave);
    } else {
      alld_consume<MODE, 0, ROWS>(lds, rank_lds, out, pair, f, lane, w_lo, h_lo, h_hi, r_begin, n_iters, n_pass, rot, dgs, H, W, D, wave);
    }
  }

  if constexpr (!RANK) {                                         // plain volume call: nothing to emit
    CTD_STAMP_DUMP(CTD_STAMP_AREA(lds, ROWS));
    return;
  }
  // ---- emit: the band's final {top, second} -> index, best score, work-list flag.  The last chunk barrier (behind
  // every wavefront's lgkmcnt(0)) has made all slot updates visible.
  const unsigned l4 = 4u * (unsigned)lane;
  const bool lane_out = w_lo + (int)l4 < W;
  const unsigned margin = rank_eps >= 0.f ? key_margin_units(rank_eps) : 0u;
  const int n_emit = has_helper ? kAWaves - 1 : kAWaves;           // wavefronts that reach this point
  for (int row = wave; row < h_hi - h_lo; row += n_emit) {
    const unsigned* sl = rank_lds + row * 512 + lane;
    const long p0 = ((long)f * H + h_lo + row) * W + w_lo + l4;    // first of the lane's four pixels
    long d64[4];
    f32x4 b4;
    unsigned listed4 = 0, n_hard = 0;
    bool hard[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const unsigned t = sl[64 * i], q = sl[256 + 64 * i];
      d64[i] = (long)(kTagMask - (t & kTagMask));
      const unsigned ft = t >> kTagBits, fq = q >> kTagBits;       // 23-bit fixed-point scores
      b4[i] = __uint_as_float(0x40800000u | ft) - kKeyBias;
      // runner-up within the margin of the best -> exact re-scoring (q == 0: the pixel has a single score)
      hard[i] = lane_out && rank_eps >= 0.f && q != 0u && ft - fq <= margin;
      if (hard[i]) { listed4 |= 1u << (8 * i); ++n_hard; }
    }
    if (lane_out) {
      typedef long l64x2 __attribute__((ext_vector_type(2)));
      *(l64x2*)(idx_out + p0) = l64x2{d64[0], d64[1]};
      *(l64x2*)(idx_out + p0 + 2) = l64x2{d64[2], d64[3]};
      *(f32x4*)(best_out + p0) = b4;
      *(unsigned*)(flags_out + p0) = listed4;
    }
    // all pixels of the row share the work-list key: one counter update per wavefront and row that has any
    if (__any(n_hard != 0)) {
      unsigned before = n_hard;                                    // exclusive prefix over the lanes
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const unsigned v = __shfl_up(before, o);
        if (lane >= o) before += v;
      }
      const unsigned total_hard = __shfl(before, 63);
      before -= n_hard;
      const int key = worklist_key(work, p0);
      unsigned base = 0;
      if (lane == 0) base = atomicAdd(work.counters + key * kWorkListStride, total_hard);
      base = __shfl(base, 0);
      int64_t* dst = work.list + (long)key * work.seg_cap + base + before;
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (hard[i]) *dst++ = p0 + i;
    }
  }
  CTD_STAMP_DUMP(CTD_STAMP_AREA(lds, ROWS));
}

// compute units of the current device (the plan's cost model counts rounds of one workgroup per CU); asked once per device
int device_cu_count() {
  static int cus[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
  if (cus[dev] == 0) {
    int n = 0;
    cus[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  }
  return cus[dev];
}

static AlldPlan alld_plan_compute(int frames, int H, int W, int D, bool ranked, int n_cu);
// (the unranked plan tries every band height for every pass split: ~5 K candidates at 1024 x 1024 x 256, on the launch path
// of a sub-millisecond call -- the last few shapes' plans are kept; a plan is a pure function of its key)
AlldPlan alld_plan(int frames, int H, int W, int D, bool ranked) {
  struct Key { int frames, H, W, D, ranked, n_cu; AlldPlan plan; };
  static thread_local Key cache[8];
  static thread_local int next = 0;
  const int n_cu = device_cu_count();
  for (const Key& k : cache)
    if (k.frames == frames && k.H == H && k.W == W && k.D == D && k.ranked == (int)ranked && k.n_cu == n_cu && k.frames > 0) return k.plan;
  Key& k = cache[next];
  next = (next + 1) % 8;
  k = Key{frames, H, W, D, (int)ranked, n_cu, alld_plan_compute(frames, H, W, D, ranked, n_cu)};
  return k.plan;
}

static AlldPlan alld_plan_compute(int frames, int H, int W, int D, bool ranked, int n_cu) {
  AlldPlan ap;
  ap.n_psplit = 1;
  // The disparities are dealt evenly over the ceil(D / 30) passes (D = 128: 5 x 26 on 13 wavefronts).  Four full passes
  // of 30 and a last one of 8 measured 4 % SLOWER: a pass costs about the same whether 13 or 15 wavefronts work in it
  // (the row's dependent chain and the chunk barrier, not the sum of the wavefronts' instructions), so the short pass
  // is a whole pass's time for a quarter of its outputs.
  ap.n_pass = ceil_div(D, kADGMax);
  ap.dgs = 2 * ceil_div(ceil_div(D, 2), ap.n_pass);
  const long base = (long)ceil_div(W, 256) * frames;
  // Band height and chunk size: 3-row chunks allow bands of up to 46 rows, 2-row chunks (a third more chunk barriers,
  // priced at kTwoRowPenalty) up to 57 -- config 2 is then ONE round of 256 workgroups of 54 rows (62 row steps per pass,
  // 66 with the unroll) instead of two rounds of 27 (2 x 36).
  double best_cost = -1;
  ap.band_rows = H < 44 ? H : 44;
  ap.chunk_rows = 3;
  for (int cr = 3; cr >= kAllowTwoRowChunks; --cr) {
    const int max_rows = alld_max_band_rows(cr) < 44 || cr == 2 ? alld_max_band_rows(cr) : 44;
    for (int rows = max_rows; rows >= 4; --rows) {
      if (rows > H) continue;
      const long wgs = base * ceil_div(H, rows);
      const double cost = (double)((wgs + n_cu - 1) / n_cu) * (double)(ceil_div(rows + 8, 6) * 6) * (cr == 2 ? kTwoRowPenalty : 1.0);
      if (best_cost < 0 || cost < best_cost) { best_cost = cost; ap.band_rows = rows; ap.chunk_rows = cr; }
    }
  }
  if (!ranked) {
    // no rank slots: 3-row chunks, any band height; try every pass split
    ap.chunk_rows = 3;
    best_cost = -1;
    for (int sp = 1; sp <= ap.n_pass; ++sp) {
      const int ppg = ceil_div(ap.n_pass, sp);
      if (ceil_div(ap.n_pass, ppg) != sp) continue;                // (the same passes per workgroup with fewer workgroups)
      for (int rows = H; rows >= 4; --rows) {
        const long wgs = base * ceil_div(H, rows) * sp;
        const double cost = (double)((wgs + n_cu - 1) / n_cu) * ppg * (double)(ceil_div(rows + 8, 6) * 6);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; ap.band_rows = rows; ap.n_psplit = sp; }
      }
    }
  }
  ap.bands = ceil_div(H, ap.band_rows);
  ap.band_rows = ceil_div(H, ap.bands);                          // the same number of bands, evenly tall
  // rank slots (2 KB per band row) in front of the staging ring, for a ranked plan only
  ap.lds = (ranked ? (size_t)ap.band_rows * 2048 : 0) + sizeof(float) * kABufs * ap.chunk_rows * kAPack;
  return ap;
}

using AlldKernel = decltype(&ncc_fast_alld_kernel<kAStore, 3>);
template <int MODE>
static AlldKernel alld_kernel(int chunk_rows) {
  return chunk_rows == 3 ? ncc_fast_alld_kernel<MODE, 3> : ncc_fast_alld_kernel<MODE, 2>;
}

int launch_alld(int mode, const AlldOperands& op, float* out, const RankPlan* rank, int frames, int H, int W, int D,
                bool timed, hipStream_t stream) {
  if (((mode & kARank) != 0) != (rank != nullptr)) return CTD_ERR_INVALID_ARG;
  const AlldPlan ap = alld_plan(frames, H, W, D, rank != nullptr);
  AlldKernel kern;
  switch (mode) {
    case kAStore | kARank: kern = alld_kernel<kAStore | kARank>(ap.chunk_rows); break;
    case kARank: kern = alld_kernel<kARank>(ap.chunk_rows); break;
    case kAStore: kern = alld_kernel<kAStore>(ap.chunk_rows); break;
    case kAStore | kASad: kern = alld_kernel<kAStore | kASad>(ap.chunk_rows); break;
    case kAStore | kAMse: kern = alld_kernel<kAStore | kAMse>(ap.chunk_rows); break;
    default: return CTD_ERR_INVALID_ARG;
  }
  // one workgroup per (column tile, band, frame) and, unranked, per share of the passes
  const int n_items = ceil_div(W, 256) * ap.bands * frames * ap.n_psplit;
  const size_t lds = ap.lds + stamp_lds_bytes();
  CTD_HIP_TRY(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  if (timed) timing_begin(stream);
  hipLaunchKernelGGL(kern, dim3(n_items), dim3(64 * (kAWaves + 1)), lds, stream, op.ac, op.m0, op.v0, op.bc, op.m1, op.v1,
                     op.st1_stride, out, rank ? rank->idx : nullptr, rank ? rank->best : nullptr,
                     rank ? rank->flags : nullptr, rank ? rank->work : WorkList{}, rank ? rank->eps : -1.f, frames,
                     n_items, H, W, D, ap.band_rows, ap.n_pass, ap.dgs, op.Wp, op.W1, op.xoff, ap.n_psplit);
  if (timed) timing_end(stream, W);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd
