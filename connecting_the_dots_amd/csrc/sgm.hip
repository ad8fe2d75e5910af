// sgm.hip -- semi-global cost aggregation over a materialised volume (ctd_sgm_aggregate_f32; the rule is stated word
// for word in include/ctd_hip.h).  One launch per path direction, in the fixed summation order, each adding its L to S
// (the first one stores), then an argmin over d.  Only f32 add / sub / min: with the build's -ffp-contract=off the
// results are the bits of tests/sgm_ref.py.
//
// sgm_sweep_kernel -- the six directions with dy != 0.  A thread owns one path and DC consecutive disparities of it
//   and keeps L(q, .) in registers.  The path walks the rows with its column moving by dx per row; when it leaves the
//   image on one side it re-enters on the other and restarts with L = C (the predecessor is outside the image), so the
//   W paths of a frame cover every pixel of every row once and never exchange anything.  A workgroup is TX consecutive
//   paths x nch = ceil(D / DC) disparity chunks (thread = chunk * TX + path): every load and store of a row is TX
//   consecutive floats per disparity.  Per row the chunks exchange, through LDS, their partial minimum and their two
//   edge values (the d - 1 / d + 1 neighbours across the chunk boundary); two LDS buffers, one barrier per row.  The
//   next row's C and S are loaded before the current row is computed (the barrier is a raw s_barrier that does not
//   drain the vector-memory counter).
// sgm_scan_kernel -- the two horizontal directions, where the path runs along the contiguous axis.  A workgroup owns
//   one image row, thread = disparity.  [D x 32] slabs of the row are staged through LDS with coalesced loads and
//   stores; inside a slab the scan steps column by column, L carried in a register from slab to slab, the minimum over
//   D by DPP inside the wavefront (+ LDS across the wavefronts when D > 64), the d - 1 / d + 1 neighbours by a
//   wavefront shift.
// sgm_argmin_kernel -- thread per pixel, first index of the least S.
//
// Traffic with V = the volume's bytes: the first direction reads C and stores S (2 V), every other one reads C and S
// and stores S (3 V), the argmin reads S: 12 V for 4 paths, 24 V for 8.
#include "ctd_common.h"
#include "ctd_wave.h"

namespace ctd {
namespace {

constexpr int kSweepMaxThreads = 1024;
constexpr int kScanTile = 32;                    // columns per LDS slab
constexpr int kScanPitch = kScanTile + 1;

__device__ inline float sgm_inf() { return __builtin_inff(); }

// ---------------------------------------------------------------------------------------------------------------------
template <int DC, int TX>
__global__ __launch_bounds__(kSweepMaxThreads) void sgm_sweep_kernel(const float* __restrict__ vol, float* __restrict__ S,
                                                                      int D, int H, int W, int tiles, int dy, int dx,
                                                                      float p1, float p2, int maximise, int accumulate) {
  __shared__ float sh[2][3][kSweepMaxThreads];   // [row parity][chunk minimum | first L | last L][thread]
  const int tid = threadIdx.x, j = tid % TX, c = tid / TX, nch = blockDim.x / TX;
  const int path = (blockIdx.x % tiles) * TX + j;
  const bool active = path < W;
  const int d0 = c * DC;
  const size_t plane = (size_t)H * W;
  const size_t base = ((size_t)(blockIdx.x / tiles) * D + d0) * plane;
  const float* vf = vol + base;
  float* sf = S + base;
  const float inf = sgm_inf();

  float L[DC], Cn[DC], Sn[DC];
  int xn = active ? path : 0;                    // column of the row being loaded
  bool restart_n = true;
  int yn = dy > 0 ? 0 : H - 1;

  auto load_row = [&]() {
    const size_t off = (size_t)yn * W + xn;
#pragma unroll
    for (int k = 0; k < DC; ++k) {
      Cn[k] = inf;
      Sn[k] = 0.f;
      if (active && d0 + k < D) {
        const float v = vf[k * plane + off];
        Cn[k] = maximise ? -v : v;
        if (accumulate) Sn[k] = sf[k * plane + off];
      }
    }
  };
  load_row();
#pragma unroll
  for (int k = 0; k < DC; ++k) L[k] = inf;

  for (int r = 0; r < H; ++r) {
    float Cv[DC], So[DC];
#pragma unroll
    for (int k = 0; k < DC; ++k) { Cv[k] = Cn[k]; So[k] = Sn[k]; }
    const size_t off = (size_t)yn * W + xn;
    const bool restart = restart_n;
    if (r + 1 < H) {                             // the next row of the path, loaded ahead
      yn += dy;
      const int x1 = xn + dx;
      restart_n = x1 < 0 || x1 >= W;
      xn = x1 < 0 ? x1 + W : (x1 >= W ? x1 - W : x1);
      load_row();
    }
    if (r > 0) {
      const float* b = &sh[(r - 1) & 1][0][0];
      float m = b[j];
      for (int cc = 1; cc < nch; ++cc) m = fminf(m, b[cc * TX + j]);
      const float below = c > 0 ? b[2 * kSweepMaxThreads + tid - TX] : inf;         // L(q, d0 - 1)
      const float above = c + 1 < nch ? b[kSweepMaxThreads + tid + TX] : inf;       // L(q, d0 + DC)
      const float mp2 = m + p2;
      float Ln[DC];
#pragma unroll
      for (int k = 0; k < DC; ++k) {
        const float lo = (k > 0 ? L[k - 1] : below) + p1;
        const float hi = (k + 1 < DC ? L[k + 1] : above) + p1;
        const float t = fminf(fminf(L[k], mp2), fminf(lo, hi));
        Ln[k] = Cv[k] + (t - m);
      }
#pragma unroll
      for (int k = 0; k < DC; ++k) L[k] = restart ? Cv[k] : Ln[k];
    } else {
#pragma unroll
      for (int k = 0; k < DC; ++k) L[k] = Cv[k];
    }
    float pm = L[0];
#pragma unroll
    for (int k = 1; k < DC; ++k) pm = fminf(pm, L[k]);
    float* w = &sh[r & 1][0][0];
    w[tid] = pm;
    w[kSweepMaxThreads + tid] = L[0];
    w[2 * kSweepMaxThreads + tid] = L[DC - 1];
    if (active) {
#pragma unroll
      for (int k = 0; k < DC; ++k)
        if (d0 + k < D) sf[k * plane + off] = accumulate ? So[k] + L[k] : L[k];
    }
    wait_lgkmcnt0();
    wg_barrier();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ inline float dpp_perm(float v) {      // a DPP permutation in which every lane has a source
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false));
}
// minimum over the 64 lanes, in every lane: quads, half rows and rows by DPP, the four rows through scalar registers
__device__ inline float wave_min(float v) {
  v = fminf(v, dpp_perm<0xB1>(v));               // quad_perm:[1,0,3,2]
  v = fminf(v, dpp_perm<0x4E>(v));               // quad_perm:[2,3,0,1]
  v = fminf(v, dpp_perm<0x141>(v));              // row_half_mirror
  v = fminf(v, dpp_perm<0x140>(v));              // row_mirror
  const int i = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(i, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(i, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(i, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(i, 48));
  return fminf(fminf(r0, r1), fminf(r2, r3));
}
// the value of lane - 1 / lane + 1; `edge` where the wavefront has no such lane
__device__ inline float lane_below(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}
__device__ inline float lane_above(float v, float edge) {
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v), 0x130 /* wave_shl:1 */, 0xf, 0xf, false));
}

__global__ __launch_bounds__(256) void sgm_scan_kernel(const float* __restrict__ vol, float* __restrict__ S, int D, int H,
                                                        int W, int dir, float p1, float p2, int maximise, int accumulate) {
  extern __shared__ float lds[];                 // slab [D][kScanPitch], then xch [2][3][4]
  float* tile = lds;
  float* xch = lds + (size_t)D * kScanPitch;     // [step parity][wave minimum | lane 0's L | lane 63's L][wave]
  const int t = threadIdx.x, nt = blockDim.x, nw = nt / 64, wave = t / 64, lane = t % 64;
  const size_t plane = (size_t)H * W;
  const size_t row = (size_t)(blockIdx.x / H) * D * plane + (size_t)(blockIdx.x % H) * W;
  const bool has = t < D;
  const float inf = sgm_inf();
  const int ntiles = (W + kScanTile - 1) / kScanTile;

  float L = inf, wm = inf;
  int step = 0;
  for (int ti = 0; ti < ntiles; ++ti) {
    const int x0 = (dir > 0 ? ti : ntiles - 1 - ti) * kScanTile;
    const int tw = min(kScanTile, W - x0);
    for (int e = t; e < D * kScanTile; e += nt) {
      const int d = e / kScanTile, xx = e % kScanTile;
      if (xx < tw) {
        const float v = vol[row + d * plane + x0 + xx];
        tile[d * kScanPitch + xx] = maximise ? -v : v;
      }
    }
    __syncthreads();
    for (int s = 0; s < tw; ++s, ++step) {
      const int xx = dir > 0 ? s : tw - 1 - s;
      const float cv = has ? tile[t * kScanPitch + xx] : inf;
      float Ln = cv;
      if (step > 0) {                            // (uniform)
        float m = wm, below = inf, above = inf;
        if (nw > 1) {
          const float* b = xch + ((step - 1) & 1) * 12;
          m = b[0];
          for (int w = 1; w < nw; ++w) m = fminf(m, b[w]);
          if (wave > 0) below = b[8 + wave - 1];
          if (wave + 1 < nw) above = b[4 + wave + 1];
        }
        const float lo = lane_below(L, below) + p1;
        const float hi = lane_above(L, above) + p1;
        const float tt = fminf(fminf(L, m + p2), fminf(lo, hi));
        Ln = cv + (tt - m);
      }
      L = Ln;                                    // (inf in the threads beyond D: inf + finite)
      if (has) tile[t * kScanPitch + xx] = L;
      wm = wave_min(L);
      if (nw > 1) {
        float* b = xch + (step & 1) * 12;
        if (lane == 0) { b[wave] = wm; b[4 + wave] = L; }
        if (lane == 63) b[8 + wave] = L;
        wait_lgkmcnt0();
        wg_barrier();
      }
    }
    __syncthreads();
    for (int e = t; e < D * kScanTile; e += nt) {
      const int d = e / kScanTile, xx = e % kScanTile;
      if (xx < tw) {
        const size_t a = row + d * plane + x0 + xx;
        const float l = tile[d * kScanPitch + xx];
        S[a] = accumulate ? S[a] + l : l;
      }
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sgm_argmin_kernel(const float* __restrict__ S, int64_t* __restrict__ idx,
                                                          float* __restrict__ best, long pixels, int D, long plane) {
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (long)gridDim.x * blockDim.x) {
    const float* s = S + (size_t)(p / plane) * D * plane + p % plane;
    float bv = s[0];
    int bi = 0;
    for (int d = 1; d < D; ++d) {
      const float v = s[(size_t)d * plane];
      if (v < bv) { bv = v; bi = d; }            // (strict: the first index wins)
    }
    idx[p] = bi;
    best[p] = bv;
  }
}

template <int DC, int TX>
int launch_sweep(const float* vol, float* S, int frames, int D, int H, int W, int dy, int dx, float p1, float p2,
                 bool maximise, bool accumulate, hipStream_t stream) {
  const int tiles = ceil_div(W, TX), nch = ceil_div(D, DC);
  sgm_sweep_kernel<DC, TX><<<dim3((unsigned)(tiles * frames)), dim3(TX * nch), 0, stream>>>(
      vol, S, D, H, W, tiles, dy, dx, p1, p2, maximise ? 1 : 0, accumulate ? 1 : 0);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace

static bool sgm_supported(int frames, int D, int H, int W) {
  // one workgroup per (frame, 32 paths) / (frame, row) on grid.x
  return D <= 256 && (double)frames * ceil_div(W, 32) < 2147483648.0 && (double)frames * H < 2147483648.0;
}

static int sgm_aggregate_f32(const float* vol, bool maximise, float p1, float p2, int paths, float* S, int64_t* idx,
                             float* best, int frames, int D, int H, int W, hipStream_t stream) {
  static const int kDirs[8][2] = {{0, 1}, {0, -1}, {1, 0}, {1, 1}, {1, -1}, {-1, 0}, {-1, 1}, {-1, -1}};   // (dy, dx)
  static const int kFour[4] = {0, 1, 2, 5};
  // 64 paths per workgroup where that fills the card and the D / 8 chunks fit 1024 threads, 32 otherwise
  const bool wide = (long)frames * ceil_div(W, 64) >= 256 && D <= 128;
  for (int i = 0; i < paths; ++i) {
    const int* dir = kDirs[paths == 4 ? kFour[i] : i];
    const bool acc = i > 0;
    int st;
    if (dir[0] == 0) {
      const int nt = ceil_div(D, 64) * 64;
      const size_t lds = sizeof(float) * ((size_t)D * kScanPitch + 24);
      sgm_scan_kernel<<<dim3((unsigned)(frames * H)), dim3(nt), lds, stream>>>(vol, S, D, H, W, dir[1], p1, p2,
                                                                              maximise ? 1 : 0, acc ? 1 : 0);
      CTD_LAUNCH_CHECK();
      st = CTD_OK;
    } else if (wide) {
      st = launch_sweep<8, 64>(vol, S, frames, D, H, W, dir[0], dir[1], p1, p2, maximise, acc, stream);
    } else {
      st = launch_sweep<8, 32>(vol, S, frames, D, H, W, dir[0], dir[1], p1, p2, maximise, acc, stream);
    }
    if (st) return st;
  }
  const long plane = (long)H * W, pixels = plane * frames;
  const long want = (pixels + 255) / 256;
  const unsigned blocks = (unsigned)(want < 8192 ? want : 8192);
  sgm_argmin_kernel<<<dim3(blocks), dim3(256), 0, stream>>>(S, idx, best, pixels, D, plane);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

static bool sgm_args_ok(int frames, int D, int H, int W, int paths, float p1, float p2) {
  if (frames <= 0 || D <= 0 || H <= 0 || W <= 0 || (paths != 4 && paths != 8)) return false;
  if ((double)frames * D * H * W >= 2147483648.0) return false;
  return p1 >= 0.f && p2 >= p1 && p2 <= 3.402823466e38f;                                       // (a NaN fails >=)
}

size_t ctd_sgm_workspace_bytes(int frames, int D, int H, int W, int paths, int want_volume) {
  if (!sgm_args_ok(frames, D, H, W, paths, 0.f, 0.f) || !sgm_supported(frames, D, H, W) || want_volume) return 0;
  return sizeof(float) * (size_t)frames * D * H * W;
}

int ctd_sgm_aggregate_f32(const float* vol, int maximise, float p1, float p2, int paths, float* S_out, int64_t* idx,
                          float* best, int frames, int D, int H, int W, void* workspace, size_t workspace_bytes,
                          int device, void* stream) {
  if (!sgm_args_ok(frames, D, H, W, paths, p1, p2)) return CTD_ERR_INVALID_ARG;
  if (!vol || !idx || !best) return CTD_ERR_INVALID_ARG;
  if (!sgm_supported(frames, D, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!S_out && (!workspace || workspace_bytes < ctd_sgm_workspace_bytes(frames, D, H, W, paths, 0) ||
                 ((uintptr_t)workspace & 15)))
    return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return sgm_aggregate_f32(vol, maximise != 0, p1, p2, paths, S_out ? S_out : (float*)workspace, idx, best, frames, D, H, W,
                           (hipStream_t)stream);
}

}  // extern "C"
