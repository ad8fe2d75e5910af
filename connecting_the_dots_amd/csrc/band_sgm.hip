// band_sgm.hip -- band-limited semi-global matching (ctd_xcorrvol_band_volume_f32, ctd_costvol_band_volume_f32,
// ctd_band_sgm_aggregate_f32; the definition, word for word: include/ext/ctd_hip_band_sgm.h).
//
// Band volumes.  The scorers of ctd_band_score.h hand every in-band score of a pixel to a sink in ascending d; the sink
// here, BandSlots, stores by slot: the first score it is given is slot 0 (d = lo'), a score of slot >= slots is dropped
// (the truncation rule), and after the last group the kernel fills the slots that were not given a score with NaN.
// The scores are the scorers', so they are the bits of band_match.hip, which this file leaves alone.
//
// Aggregation.  One launch per direction in the summation order of sgm.hip, each adding its L to S (the first one
// stores, and writes NaN into the slots a pixel does not hold), then an argmin over the slots.  A predecessor's slot
// for disparity d is d - lo'(q), an offset that differs per pixel, so L(q, .) lives in LDS and never in a register
// array that would be indexed with it.
//   band_sweep_kernel -- the six directions with dy != 0.  A thread owns one slot of one path (thread = path * SB +
//     slot, 256 / SB paths per workgroup, the SB lanes of a path inside one wavefront).  The path walks the rows with
//     its column moving by dx per row and re-enters on the other side, restarting, when it leaves the image (as
//     sgm_sweep_kernel does).  Per row a lane writes its L to LDS [2][256] (two row parities) and reads the
//     predecessor's slots k + sh - 1, k + sh, k + sh + 1 of its own path from it; the minimum over the path's lanes is
//     log2(SB) lane exchanges.  Nothing crosses a wavefront, so there is no barrier.  The C, S, lo and hi of the next
//     16 rows are loaded while the current 16 are computed.
//   band_scan_kernel -- the two horizontal directions.  A workgroup owns R image rows; [slots][R][32] slabs of them go
//     through LDS with coalesced loads and stores (four in flight per thread), and inside a slab thread r < R scans
//     row r column by column with all SB slots in registers (band_pixel), L(q, .) in LDS [2][SB][R].
//   band_argmin_kernel -- thread per pixel, first slot of the least S.
// SB is the slot bucket (4 / 8 / 16 / 32 / 64) that `slots` falls into.
//
// Traffic with Vb = the band volume's bytes and P = the bytes of lo and hi: the first direction reads C and stores S
// (2 Vb + P), every other one reads C and S and stores S (3 Vb + P), the argmin reads S and the band:
// 12 Vb + 5 P for 4 paths, 24 Vb + 9 P for 8.
#include "../../include/ext/ctd_hip_band_sgm.h"
#include "ctd_band_score.h"

namespace ctd {
namespace {

constexpr int kMaxSlots = 64;
constexpr int kScanCols = 32;                    // columns per LDS slab
constexpr int kScanPitch = kScanCols + 1;

__device__ inline float bs_inf() { return __builtin_inff(); }
__device__ inline float bs_nan() { return __builtin_nanf(""); }

// the band rule: lo' (clamped to D: no overflow below, and a pixel with lo' >= D holds nothing) and n
__device__ inline void band_of(int lo, int hi, int D, int slots, int& l, int& n) {
  l = clampi(lo, 0, D);
  const int u = min(clampi(hi, -1, D - 1), l + slots - 1);
  n = max(u - l + 1, 0);
}

// ---------------------------------------------------------------------------------------------------------------------
// band volumes
// ---------------------------------------------------------------------------------------------------------------------

struct BandSlots {
  float* vb;                                     // [frames][slots][H][W]
  long plane;
  int slots;
  float* px;                                     // slot 0 of the pixel
  int first, cnt;
  __device__ inline void open(long row, int w) {
    const long p = row + w, f = p / plane;
    px = vb + f * slots * plane + (p - f * plane);
    first = -1;
    cnt = 0;
  }
  __device__ inline void take(float s, int d) {
    if (first < 0) first = d;
    const int k = d - first;
    if (k < slots) {
      px[k * plane] = s;
      cnt = k + 1;
    }
  }
  __device__ inline void finish() {              // (the pixel's own thread, once, after its last score)
    for (int k = cnt; k < slots; ++k) px[k * plane] = bs_nan();
  }
};

template <int BS>
__global__ __launch_bounds__(256) void xcorrvol_bandvol_kernel(const float* __restrict__ in0,
                                                               const float* __restrict__ in1,
                                                               const float2* __restrict__ pstat, long in1_frame_stride,
                                                               const int32_t* __restrict__ lo,
                                                               const int32_t* __restrict__ hi, float* __restrict__ vb,
                                                               int slots, int H, int W, int D, int tiles_x,
                                                               int tiles_y) {
  BandSlots sk{vb, (long)H * W, slots};
  long p;
  const bool inside = xcorrvol_band_tile<BS>(in0, in1, pstat, in1_frame_stride, lo, hi, H, W, D, tiles_x, tiles_y, sk, p);
  if (inside) sk.finish();
}

__global__ __launch_bounds__(256) void xcorrvol_bandvol_rt_kernel(const float* __restrict__ in0,
                                                                  const float* __restrict__ in1,
                                                                  const float2* __restrict__ pstat,
                                                                  long in1_frame_stride, const int32_t* __restrict__ lo,
                                                                  const int32_t* __restrict__ hi,
                                                                  float* __restrict__ vb, int slots, int frames, int H,
                                                                  int W, int D, int bs) {
  BandSlots sk{vb, (long)H * W, slots};
  long p;
  const bool inside = xcorrvol_band_rt_pixel(in0, in1, pstat, in1_frame_stride, lo, hi, frames, H, W, D, bs, sk, p);
  if (inside) sk.finish();
}

template <int TYPE, int BS>
__global__ __launch_bounds__(256) void costvol_bandvol_kernel(const float* __restrict__ im,
                                                              const float* __restrict__ pat, long pat_frame_stride,
                                                              const int32_t* __restrict__ lo,
                                                              const int32_t* __restrict__ hi, float* __restrict__ vb,
                                                              int slots, int frames, int H, int W, int D, int bs_rt,
                                                              float eps, int tiles_x, int tiles_y) {
  BandSlots sk{vb, (long)H * W, slots};
  long p;
  const bool inside = costvol_band_pixel<TYPE, BS>(im, pat, pat_frame_stride, lo, hi, frames, H, W, D, bs_rt, eps,
                                                   tiles_x, tiles_y, sk, p);
  if (inside) sk.finish();
}

int xcorrvol_band_volume_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                             const int32_t* hi, float* vb, int frames, int slots, int H, int W, int D, int bs,
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
  const int tiles_x = ceil_div(W, kBandTW), tiles_y = ceil_div(H, kBandTH);
  const dim3 g((unsigned)((long)frames * tiles_y * tiles_x));   // <= frames * H * W < 2^31
  switch (bs) {
    case 3: hipLaunchKernelGGL(xcorrvol_bandvol_kernel<3>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, vb, slots, H, W, D, tiles_x, tiles_y); break;
    case 5: hipLaunchKernelGGL(xcorrvol_bandvol_kernel<5>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, vb, slots, H, W, D, tiles_x, tiles_y); break;
    case 7: hipLaunchKernelGGL(xcorrvol_bandvol_kernel<7>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, vb, slots, H, W, D, tiles_x, tiles_y); break;
    case 9: hipLaunchKernelGGL(xcorrvol_bandvol_kernel<9>, g, dim3(256), 0, stream, in0, in1, pstat, in1_frame_stride, lo, hi, vb, slots, H, W, D, tiles_x, tiles_y); break;
    default: {
      const long n = (long)frames * H * W;
      hipLaunchKernelGGL(xcorrvol_bandvol_rt_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, in0, in1,
                         pstat, in1_frame_stride, lo, hi, vb, slots, frames, H, W, D, bs);
    }
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

template <int TYPE>
void costvol_bandvol_launch(const float* im, const float* pat, long pat_frame_stride, const int32_t* lo,
                            const int32_t* hi, float* vb, int frames, int slots, int H, int W, int D, int bs, float eps,
                            hipStream_t stream) {
  const int tiles_x = ceil_div(W, kBandTW), tiles_y = ceil_div(H, kBandTH);
  const dim3 g((unsigned)((long)frames * tiles_y * tiles_x));   // <= frames * H * W < 2^31
  switch (bs) {
    case 3: hipLaunchKernelGGL((costvol_bandvol_kernel<TYPE, 3>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, vb, slots, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    case 5: hipLaunchKernelGGL((costvol_bandvol_kernel<TYPE, 5>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, vb, slots, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    case 7: hipLaunchKernelGGL((costvol_bandvol_kernel<TYPE, 7>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, vb, slots, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    case 9: hipLaunchKernelGGL((costvol_bandvol_kernel<TYPE, 9>), g, dim3(256), 0, stream, im, pat, pat_frame_stride, lo, hi, vb, slots, frames, H, W, D, bs, eps, tiles_x, tiles_y); break;
    default: {
      const long n = (long)frames * H * W;
      hipLaunchKernelGGL((costvol_bandvol_kernel<TYPE, 0>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, im,
                         pat, pat_frame_stride, lo, hi, vb, slots, frames, H, W, D, bs, eps, tiles_x, tiles_y);
    }
  }
}

int costvol_band_volume_f32(const float* im, const float* pat, long pat_frame_stride, const int32_t* lo,
                            const int32_t* hi, float* vb, int frames, int slots, int H, int W, int D, int bs, int type,
                            float eps, hipStream_t stream) {
  switch (type) {
    case 0: costvol_bandvol_launch<0>(im, pat, pat_frame_stride, lo, hi, vb, frames, slots, H, W, D, bs, eps, stream); break;
    case 1: costvol_bandvol_launch<1>(im, pat, pat_frame_stride, lo, hi, vb, frames, slots, H, W, D, bs, eps, stream); break;
    case 2: costvol_bandvol_launch<2>(im, pat, pat_frame_stride, lo, hi, vb, frames, slots, H, W, D, bs, eps, stream); break;
    default: costvol_bandvol_launch<3>(im, pat, pat_frame_stride, lo, hi, vb, frames, slots, H, W, D, bs, eps, stream); break;
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// aggregation
// ---------------------------------------------------------------------------------------------------------------------

// L(p, .) of one pixel for all SB slots at once.  prev = the predecessor's L by slot (stride `pitch`; its slots >= nq
// hold anything), sh = lo'(p) - lo'(q): the predecessor's slot for p's slot k is k + sh.  The shift goes into the LDS
// addresses -- SB + 2 reads, clamped to stay inside the array, masked to +inf where q holds nothing -- so every
// register array below is indexed at compile time.  Slots >= n(p) of Lv come out as anything.
template <int SB>
__device__ inline void band_pixel(const float (&C)[SB], float (&Lv)[SB], const float* prev, int pitch, int sh, int nq,
                                  float mq, float p1, float p2, bool fresh) {
  const float inf = bs_inf();
  float q[SB + 2];                               // q[i] = L(q, slot sh + i - 1)
#pragma unroll
  for (int i = 0; i < SB + 2; ++i) {
    const int kq = sh + i - 1;
    const float v = prev[clampi(kq, 0, SB - 1) * pitch];
    q[i] = (unsigned)kq < (unsigned)nq ? v : inf;
  }
  const float mp2 = mq + p2;
#pragma unroll
  for (int k = 0; k < SB; ++k) {
    const float t = fminf(fminf(q[k + 1], mp2), fminf(q[k] + p1, q[k + 2] + p1));
    Lv[k] = fresh ? C[k] : C[k] + (t - mq);
  }
}

// minimum over the SB consecutive lanes (SB a power of two <= 64) that hold one path, in every one of them
template <int SB>
__device__ inline float group_min(float v) {
#pragma unroll
  for (int mask = 1; mask < SB; mask <<= 1) v = fminf(v, __shfl_xor(v, mask, 64));
  return v;
}

constexpr int kSweepAhead = 16;                  // rows of a path whose loads are in flight together

template <int SB>
__global__ __launch_bounds__(256) void band_sweep_kernel(const float* __restrict__ vb, const int32_t* __restrict__ lo,
                                                         const int32_t* __restrict__ hi, float* __restrict__ S,
                                                         int slots, int D, int H, int W, int tiles, int dy, int dx,
                                                         float p1, float p2, int maximise, int accumulate) {
  constexpr int TP = 256 / SB;                   // paths of a workgroup; thread = path * SB + slot
  __shared__ float Lq[2][256];                   // [row parity][thread]: L(q, .), read by the lanes of the same path only
  const int t = threadIdx.x, k = t % SB, pl = t / SB;
  const int path_raw = (blockIdx.x % tiles) * TP + pl;
  const bool active = path_raw < W && k < slots; // (an idle lane computes on valid addresses and stores nothing)
  const int path = min(path_raw, W - 1), kc = min(k, slots - 1);
  const size_t plane = (size_t)H * W;
  const size_t f = blockIdx.x / tiles;
  const float* vf = vb + (f * slots + kc) * plane;
  float* sf = S + (f * slots + kc) * plane;
  const int32_t* lf = lo + f * plane;
  const int32_t* hf = hi + f * plane;
  // row r of the path (r = 0 is where it starts) is image row y(r), column (path + dx * r) mod W: when the path
  // leaves the image on one side it re-enters on the other and restarts
  auto column_of = [&](int r) {
    const int x = (path + dx * r) % W;
    return x < 0 ? x + W : x;
  };
  auto offset_of = [&](int r, int x) { return (size_t)(dy > 0 ? r : H - 1 - r) * W + x; };

  float cn[kSweepAhead], sn[kSweepAhead];
  int ln[kSweepAhead], hn[kSweepAhead];
  auto load_rows = [&](int r0) {                 // rows r0 .. r0 + kSweepAhead - 1 (clamped to the last one)
#pragma unroll
    for (int u = 0; u < kSweepAhead; ++u) {
      const int r = min(r0 + u, H - 1);
      const size_t off = offset_of(r, column_of(r));
      ln[u] = lf[off];
      hn[u] = hf[off];
      cn[u] = vf[off];
      sn[u] = accumulate ? sf[off] : 0.f;
    }
  };
  load_rows(0);

  int lq = 0, nq = 0, xq = 0;
  float mq = 0.f;
  const float inf = bs_inf();
  for (int r0 = 0; r0 < H; r0 += kSweepAhead) {
    float cv[kSweepAhead], sv[kSweepAhead];
    int lv[kSweepAhead], hv[kSweepAhead];
#pragma unroll
    for (int u = 0; u < kSweepAhead; ++u) { cv[u] = cn[u]; sv[u] = sn[u]; lv[u] = ln[u]; hv[u] = hn[u]; }
    if (r0 + kSweepAhead < H) load_rows(r0 + kSweepAhead);      // the next rows, loaded ahead (S of them is not yet
                                                                // written: this launch writes a pixel once)
#pragma unroll
    for (int u = 0; u < kSweepAhead; ++u) {
      const int r = r0 + u;
      if (r < H) {                               // (uniform)
        const int x = column_of(r);
        int l, n;
        band_of(lv[u], hv[u], D, slots, l, n);
        // the predecessor is outside the image (the path starts or re-enters here) or holds nothing
        const bool fresh = r == 0 || x != xq + dx || nq == 0;
        const float c = maximise ? -cv[u] : cv[u];
        const float* prev = &Lq[(r & 1) ^ 1][pl * SB];
        const int kq = k + (l - lq);             // the predecessor's slot for the same disparity
        const float q0 = prev[clampi(kq - 1, 0, SB - 1)], q1 = prev[clampi(kq, 0, SB - 1)];
        const float q2 = prev[clampi(kq + 1, 0, SB - 1)];
        const float below = (unsigned)(kq - 1) < (unsigned)nq ? q0 : inf;
        const float same = (unsigned)kq < (unsigned)nq ? q1 : inf;
        const float above = (unsigned)(kq + 1) < (unsigned)nq ? q2 : inf;
        const float tt = fminf(fminf(same, mq + p2), fminf(below + p1, above + p1));
        const float Lv = fresh ? c : c + (tt - mq);
        Lq[r & 1][t] = Lv;
        const float m = group_min<SB>(k < n ? Lv : inf);
        if (active) {
          const size_t off = offset_of(r, x);
          if (k < n) sf[off] = accumulate ? sv[u] + Lv : Lv;
          else if (!accumulate) sf[off] = bs_nan();
        }
        lq = l;
        nq = n;
        mq = m;
        xq = x;
      }
    }
  }
}

template <int SB, int R>
__global__ __launch_bounds__(256) void band_scan_kernel(const float* __restrict__ vb, const int32_t* __restrict__ lo,
                                                        const int32_t* __restrict__ hi, float* __restrict__ S,
                                                        int slots, int D, int H, int W, int rows, int dir, float p1,
                                                        float p2, int maximise, int accumulate) {
  __shared__ float slab[SB][R][kScanPitch];      // C on the way in, L on the way out
  __shared__ float Lst[2][SB][R];                // [step parity][slot][row]: L(q, .)
  __shared__ int slo[R][kScanPitch], sn[R][kScanPitch];
  constexpr int kBatch = 4;                      // loads in flight per thread
  const int t = threadIdx.x;
  const int row0 = blockIdx.x * R;               // rows = frames * H < 2^31
  const size_t plane = (size_t)H * W;
  const int ntiles = ceil_div(W, kScanCols);
  const bool scans = t < R && row0 + t < rows;
  const int total = slots * R * kScanCols;

  int lq = 0, nq = 0, step = 0;
  float mq = 0.f;
  for (int ti = 0; ti < ntiles; ++ti) {
    const int x0 = (dir > 0 ? ti : ntiles - 1 - ti) * kScanCols;
    const int tw = min(kScanCols, W - x0);
    // element e of the slab: slot k, row rr, column xx; its address in a [frames][slots][H][W] volume, or -1
    auto address = [&](int e, int& k, int& rr, int& xx) -> long {
      k = e / (R * kScanCols);
      const int rem = e % (R * kScanCols);
      rr = rem / kScanCols;
      xx = rem % kScanCols;
      const int row = row0 + rr;
      if (e >= total || row >= rows || xx >= tw) return -1;
      return (long)(((size_t)(row / H) * slots + k) * plane + (size_t)(row % H) * W + x0 + xx);
    };
    for (int e = t; e < R * kScanCols; e += 256) {
      const int rr = e / kScanCols, xx = e % kScanCols, row = row0 + rr;
      if (row < rows && xx < tw) {
        const size_t off = (size_t)(row / H) * plane + (size_t)(row % H) * W + x0 + xx;
        int l, n;
        band_of(lo[off], hi[off], D, slots, l, n);
        slo[rr][xx] = l;
        sn[rr][xx] = n;
      }
    }
    for (int e0 = t; e0 < total; e0 += 256 * kBatch) {
      float v[kBatch];
      int k[kBatch], rr[kBatch], xx[kBatch];
      long a[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        a[u] = address(e0 + u * 256, k[u], rr[u], xx[u]);
        v[u] = a[u] >= 0 ? vb[a[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u)
        if (a[u] >= 0) slab[k[u]][rr[u]][xx[u]] = maximise ? -v[u] : v[u];
    }
    __syncthreads();
    if (scans) {
      for (int s = 0; s < tw; ++s, ++step) {
        const int xx = dir > 0 ? s : tw - 1 - s;
        const int l = slo[t][xx], n = sn[t][xx];
        const bool fresh = step == 0 || nq == 0;
        float C[SB], Lv[SB];
#pragma unroll
        for (int k = 0; k < SB; ++k) C[k] = slab[k][t][xx];
        band_pixel<SB>(C, Lv, &Lst[(step & 1) ^ 1][0][t], R, l - lq, nq, mq, p1, p2, fresh);
        float m = bs_inf();
#pragma unroll
        for (int k = 0; k < SB; ++k) {
          Lst[step & 1][k][t] = Lv[k];
          slab[k][t][xx] = Lv[k];
          m = fminf(m, k < n ? Lv[k] : bs_inf());
        }
        lq = l;
        nq = n;
        mq = m;
      }
    }
    __syncthreads();
    for (int e0 = t; e0 < total; e0 += 256 * kBatch) {
      float v[kBatch];
      int k[kBatch], rr[kBatch], xx[kBatch];
      long a[kBatch];
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        a[u] = address(e0 + u * 256, k[u], rr[u], xx[u]);
        v[u] = (accumulate && a[u] >= 0) ? S[a[u]] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < kBatch; ++u) {
        if (a[u] >= 0) {
          if (k[u] < sn[rr[u]][xx[u]]) S[a[u]] = accumulate ? v[u] + slab[k[u]][rr[u]][xx[u]] : slab[k[u]][rr[u]][xx[u]];
          else if (!accumulate) S[a[u]] = bs_nan();
        }
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void band_argmin_kernel(const float* __restrict__ S, const int32_t* __restrict__ lo,
                                                          const int32_t* __restrict__ hi, int64_t* __restrict__ idx,
                                                          float* __restrict__ best, long pixels, int slots, int D,
                                                          long plane) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (long)gridDim.x * blockDim.x) {
    int l, n;
    band_of(lo[p], hi[p], D, slots, l, n);
    const float* s = S + (size_t)(p / plane) * slots * plane + p % plane;
    float bv = bs_nan();
    int bi = -1;
    for (int k = 0; k < n; ++k) {
      const float v = s[(size_t)k * plane];
      if (bi < 0 || v < bv) { bv = v; bi = l + k; }            // (strict: the first slot wins)
    }
    idx[p] = bi;
    best[p] = bv;
  }
}

template <int SB, int R>
int band_direction(const float* vb, const int32_t* lo, const int32_t* hi, float* S, int frames, int slots, int D,
                   int H, int W, int dy, int dx, float p1, float p2, int maximise, int acc, hipStream_t stream) {
  if (dy == 0) {
    const int rows = frames * H;
    band_scan_kernel<SB, R><<<dim3((unsigned)ceil_div(rows, R)), dim3(256), 0, stream>>>(
        vb, lo, hi, S, slots, D, H, W, rows, dx, p1, p2, maximise, acc);
  } else {
    const int tiles = ceil_div(W, 256 / SB);
    band_sweep_kernel<SB><<<dim3((unsigned)(tiles * frames)), dim3(256), 0, stream>>>(
        vb, lo, hi, S, slots, D, H, W, tiles, dy, dx, p1, p2, maximise, acc);
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

int band_sgm_aggregate_f32(const float* vb, const int32_t* lo, const int32_t* hi, bool maximise, float p1, float p2,
                           int paths, float* S, int64_t* idx, float* best, int frames, int slots, int H, int W, int D,
                           hipStream_t stream) {
  static const int kDirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {1, 1}, {1, -1}, {-1, 0}, {-1, 1}, {-1, -1}};   // (dy, dx)
  static const int kFour[4] = {0, 1, 2, 5};
  for (int i = 0; i < paths; ++i) {
    const int* dir = kDirs[paths == 4 ? kFour[i] : i];
    const int mx = maximise ? 1 : 0, acc = i > 0 ? 1 : 0;
    int st;
    // the scan's rows per workgroup keep its slab at 33 KiB of LDS
    if (slots <= 4) st = band_direction<4, 32>(vb, lo, hi, S, frames, slots, D, H, W, dir[0], dir[1], p1, p2, mx, acc, stream);
    else if (slots <= 8) st = band_direction<8, 32>(vb, lo, hi, S, frames, slots, D, H, W, dir[0], dir[1], p1, p2, mx, acc, stream);
    else if (slots <= 16) st = band_direction<16, 16>(vb, lo, hi, S, frames, slots, D, H, W, dir[0], dir[1], p1, p2, mx, acc, stream);
    else if (slots <= 32) st = band_direction<32, 8>(vb, lo, hi, S, frames, slots, D, H, W, dir[0], dir[1], p1, p2, mx, acc, stream);
    else st = band_direction<64, 4>(vb, lo, hi, S, frames, slots, D, H, W, dir[0], dir[1], p1, p2, mx, acc, stream);
    if (st) return st;
  }
  const long plane = (long)H * W, pixels = plane * frames;
  const long want = (pixels + 255) / 256;
  const unsigned blocks = (unsigned)(want < 8192 ? want : 8192);
  band_argmin_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(S, lo, hi, idx, best, pixels, slots, D, plane);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

bool band_sgm_scalars_ok(int slots, int paths, float p1, float p2) {
  if (slots < 1 || (paths != 4 && paths != 8)) return false;
  return p1 >= 0.f && p2 >= p1 && p2 <= 3.402823466e38f;                                          // (a NaN fails >=)
}

bool band_sgm_supported(int frames, int slots, int H, int W) {
  return slots <= kMaxSlots && (double)frames * H * W < 2147483648.0 && (double)frames * slots * H * W < 2147483648.0;
}

}  // namespace
}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_xcorrvol_band_volume_f32(const float* in0, const float* in1, long in1_frame_stride, const int32_t* lo,
                                 const int32_t* hi, float* vol_b, int frames, int slots, int H, int W, int D,
                                 int block_size, int flags, void* workspace, size_t workspace_bytes, int device,
                                 void* stream) {
  if (slots < 1 || !band_shape_ok(frames, H, W, D, block_size, in1_frame_stride) ||
      (flags & ~CTD_PATTERN_PREPARED) != 0)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!in0 || !in1 || !lo || !hi || !vol_b) return CTD_ERR_INVALID_ARG;
  if (!band_sgm_supported(frames, slots, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!workspace || ((uintptr_t)workspace & 255) ||
      workspace_bytes < xcorrvol_subpixel_workspace_bytes(frames, H, W, D, in1_frame_stride != 0))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return xcorrvol_band_volume_f32(in0, in1, in1_frame_stride, lo, hi, vol_b, frames, slots, H, W, D, block_size,
                                  (flags & CTD_PATTERN_PREPARED) != 0, workspace, (hipStream_t)stream);
}

int ctd_costvol_band_volume_f32(const float* im, const float* pattern, long pattern_frame_stride, const int32_t* lo,
                                const int32_t* hi, float* vol_b, int frames, int slots, int H, int W, int D,
                                int block_size, int type, float eps, int device, void* stream) {
  if (slots < 1 || !band_shape_ok(frames, H, W, D, block_size, pattern_frame_stride) || type < 0 || type > 3)
    return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!im || !pattern || !lo || !hi || !vol_b) return CTD_ERR_INVALID_ARG;
  if (!band_sgm_supported(frames, slots, H, W)) return CTD_ERR_UNSUPPORTED;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return costvol_band_volume_f32(im, pattern, pattern_frame_stride, lo, hi, vol_b, frames, slots, H, W, D, block_size,
                                 type, eps, (hipStream_t)stream);
}

size_t ctd_band_sgm_workspace_bytes(int frames, int slots, int H, int W, int D, int paths, int want_volume) {
  if (!band_sgm_scalars_ok(slots, paths, 0.f, 0.f) || !vol_shape_ok(frames, 1, H, W, D, 1) || frames == 0 ||
      !band_sgm_supported(frames, slots, H, W) || want_volume)
    return 0;
  return sizeof(float) * (size_t)frames * slots * H * W;
}

int ctd_band_sgm_aggregate_f32(const float* vol_b, const int32_t* lo, const int32_t* hi, int maximise, float p1,
                               float p2, int paths, float* S_b, int64_t* idx, float* best, int frames, int slots,
                               int H, int W, int D, void* workspace, size_t workspace_bytes, int device,
                               void* stream) {
  if (!band_sgm_scalars_ok(slots, paths, p1, p2) || !vol_shape_ok(frames, 1, H, W, D, 1)) return CTD_ERR_INVALID_ARG;
  if (frames == 0) return CTD_OK;
  if (!vol_b || !lo || !hi || !idx || !best) return CTD_ERR_INVALID_ARG;
  if (!band_sgm_supported(frames, slots, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!S_b && (!workspace || ((uintptr_t)workspace & 15) ||
               workspace_bytes < ctd_band_sgm_workspace_bytes(frames, slots, H, W, D, paths, 0)))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return band_sgm_aggregate_f32(vol_b, lo, hi, maximise != 0, p1, p2, paths, S_b ? S_b : (float*)workspace, idx, best,
                                frames, slots, H, W, D, (hipStream_t)stream);
}

}  // extern "C"
