// depth_icp.hip -- depth-map normals and projective point-to-plane ICP of a track's views (ctd_depth_normals_f32,
// ctd_depth_icp_system_f32, ctd_depth_icp_update_f32; the rules are stated word for word in include/ctd_hip_icp.h).
//
// live_at() and view_transform_point() are those of ctd_view.h; every f32 product and sum is in the association of the
// header and the build never contracts them.  Poses and K are indexed by block-uniform values only (track, view,
// target): scalar loads.
//   depth_normals_kernel -- a 64 x 4 tile of one view, thread = pixel: the pixel and its four axis neighbours (5 B depth +
//     valid and 12 B ray each, of which the caches serve the four neighbours), 12 B written.
//   icp_system_kernel    -- 1024 consecutive pixels of ONE view (a chunk never crosses a view): thread i takes the pixels
//     i, i + 256, i + 512, i + 768 of the chunk, ascending, into 29 f64 registers (every product of two f32 factors is exact
//     in f64, so fma() rounds once, as a product and an add would); then ONE reduction per workgroup: a butterfly over
//     the lane distances 32 .. 1 (an add commutes, so every lane ends with the same bits), the four wavefronts
//     ascending through LDS, 29 f64 to the workspace.  Per pixel 5 B + 12 B ray read, per pixel that lands one gather of
//     5 B depth + valid, 12 B normal and 12 B ray; 4 B residual and 8 B assoc written when asked for.  The workgroups of
//     a skipped view (view 0 of every track under the default target) write zeros, NaN and -1 and skip the reduction.
//   icp_finish_kernel    -- one wavefront per view: lane e < 29 sums entry e of the view's workgroups, ascending.
//   icp_update_kernel    -- one thread per view, f64: LDL^T of the damped 6 x 6 system, the three solves, Rodrigues, the
//     composition with the poses, one rounding to f32.
// No atomics, no flag that another workgroup waits on: the same bits on every run.
// The accumulation of a row, the workgroup's reduction, icp_finish_kernel and the solve up to the Rodrigues step live in
// ctd_icp_solve.h, which mesh_register.hip includes too; they are the code that stood here.
#include "../../include/ctd_hip_icp.h"
#include "ctd_common.h"
#include "ctd_icp_solve.h"
#include "ctd_validate.h"
#include "ctd_view.h"

namespace ctd {
namespace {

// the view that view s is aligned to, or -1: skipped (target NULL: zeros)
__device__ inline int icp_target(const int32_t* __restrict__ target, long bv, int s, int V) {
  const int a = target ? target[bv] : 0;
  return (a < 0 || a >= V || a == s) ? -1 : a;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_normals_kernel(const float* __restrict__ depth,
                                                            const uint8_t* __restrict__ valid,
                                                            const float* __restrict__ ray, float max_rel,
                                                            float* __restrict__ normal, int H, int W, int tiles_x,
                                                            int tiles) {
  const int tile = blockIdx.x % tiles;
  const long bv = blockIdx.x / tiles;
  const int x = (tile % tiles_x) * 64 + (threadIdx.x & 63), y = (tile / tiles_x) * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long plane = (long)H * W, q = (long)y * W + x, g = bv * plane + q;
  const float nan = __builtin_nanf("");
  float n[3] = {nan, nan, nan};
  if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && live_at(depth, valid, g)) {
    const long nb[4] = {q + 1, q - 1, q + W, q - W};          // (y,x+1), (y,x-1), (y+1,x), (y-1,x)
    const float d = depth[g], tol = max_rel * d;
    bool ok = true;
    float P[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long gk = bv * plane + nb[k];
      const bool lk = live_at(depth, valid, gk);
      const float dk = depth[gk];
      ok = ok && lk && fabsf(dk - d) <= tol;
#pragma unroll
      for (int i = 0; i < 3; ++i) P[k][i] = dk * ray[nb[k] * 3 + i];
    }
    if (ok) {
      float a[3], b[3], P0[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        a[i] = P[0][i] - P[1][i];
        b[i] = P[2][i] - P[3][i];
        P0[i] = d * ray[q * 3 + i];
      }
      const float c0 = a[1] * b[2] - a[2] * b[1], c1 = a[2] * b[0] - a[0] * b[2], c2 = a[0] * b[1] - a[1] * b[0];
      const float l = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
      if (l > 0.f && l < __builtin_inff()) {
        n[0] = c0 / l;
        n[1] = c1 / l;
        n[2] = c2 / l;
        if (n[0] * P0[0] + n[1] * P0[1] + n[2] * P0[2] > 0.f) {
          n[0] = -n[0];
          n[1] = -n[1];
          n[2] = -n[2];
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) normal[g * 3 + i] = n[i];
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIcpThreads) void icp_system_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ valid, const float* __restrict__ normal,
    const float* __restrict__ ray, const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ t,
    const int32_t* __restrict__ target, float max_dist2, double* __restrict__ partial, float* __restrict__ residual,
    int64_t* __restrict__ assoc, int V, int H, int W, int chunks) {
  __shared__ double wave_sum[kIcpThreads / 64][kSys];
  const long plane = (long)H * W;
  const long bv = blockIdx.x / chunks;
  const int b = (int)(bv / V), s = (int)(bv % V);
  const int a = icp_target(target, bv, s, V);
  const long track = (long)b * V * plane, base = (long)(blockIdx.x % chunks) * kIcpChunk;
  const float nan = __builtin_nanf("");
  if (a < 0) {                                                  // a skipped view (block-uniform): zeros, NaN, -1; no reduction
#pragma unroll
    for (int k = 0; k < kIcpPix; ++k) {
      const long q = base + k * kIcpThreads + threadIdx.x;
      if (q >= plane) break;
      if (residual) residual[track + s * plane + q] = nan;
      if (assoc) assoc[track + s * plane + q] = -1;
    }
    if (threadIdx.x < kSys) partial[(long)blockIdx.x * kSys + threadIdx.x] = 0.0;
    return;
  }
  double acc[kSys];
#pragma unroll
  for (int e = 0; e < kSys; ++e) acc[e] = 0.0;
  const float* dt = depth + track;
  const uint8_t* vt = valid ? valid + track : nullptr;
  const float* nt = normal + track * 3;
  const float* Rt = R + (long)b * V * 9;
  const float* tt = t + (long)b * V * 3;
#pragma unroll
  for (int k = 0; k < kIcpPix; ++k) {
    const long q = base + k * kIcpThreads + threadIdx.x;
    if (q >= plane) break;                                    // (ascending: every later pixel of the thread is past it too)
    const long gl = s * plane + q;
    float e = nan;
    long hit = -1;
    if (live_at(dt, vt, gl)) {
      float S[3], uvd[3];
      view_transform_point(ray + q * 3, dt[gl], Rt + s * 9, tt + s * 3, Rt + a * 9, tt + a * 3, K, S, uvd);
      if (uvd[2] > 0.f) {
        const float xs = floorf(uvd[0] / uvd[2] + 0.5f), ys = floorf(uvd[1] / uvd[2] + 0.5f);
        // float compares first (a NaN fails them); W - 1 and H - 1 are exact in f32 (H, W <= 2^24)
        if (xs >= 0.f && xs <= (float)(W - 1) && ys >= 0.f && ys <= (float)(H - 1)) {
          const long p = (long)(int)ys * W + (int)xs, ga = a * plane + p;
          const float n0 = nt[ga * 3 + 0], n1 = nt[ga * 3 + 1], n2 = nt[ga * 3 + 2];
          if (live_at(dt, vt, ga) && finite_f(n0) && finite_f(n1) && finite_f(n2)) {
            const float da = dt[ga];
            const float D0 = S[0] - da * ray[p * 3 + 0], D1 = S[1] - da * ray[p * 3 + 1], D2 = S[2] - da * ray[p * 3 + 2];
            if (D0 * D0 + D1 * D1 + D2 * D2 <= max_dist2) {
              e = n0 * D0 + n1 * D1 + n2 * D2;
              hit = track + ga;
              const float Jf[6] = {S[1] * n2 - S[2] * n1, S[2] * n0 - S[0] * n2, S[0] * n1 - S[1] * n0, n0, n1, n2};
              icp_accumulate(acc, Jf, e);
              acc[28] = acc[28] + 1.0;
            }
          }
        }
      }
    }
    if (residual) residual[track + gl] = e;
    if (assoc) assoc[track + gl] = hit;
  }
  icp_block_reduce(acc, wave_sum, partial + (long)blockIdx.x * kSys);   // one reduction per workgroup
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void icp_update_kernel(const double* __restrict__ system, const float* __restrict__ R,
                                                        const float* __restrict__ t, const int32_t* __restrict__ target,
                                                        double min_count, double min_pivot, double damping,
                                                        float* __restrict__ R_out, float* __restrict__ t_out,
                                                        uint8_t* __restrict__ ok_out, int V, long views) {
  const long bv = (long)blockIdx.x * 64 + threadIdx.x;
  if (bv >= views) return;
  const int s = (int)(bv % V);
  const long b = bv / V;
  const int a = icp_target(target, bv, s, V);
  const double* sys = system + bv * kSys;
  const float* Rs = R + bv * 9;
  const float* ts = t + bv * 3;
  double x[6], Rr[3][3];
  if (!icp_solve(sys, a >= 0, min_count, min_pivot, damping, x, Rr)) {
    for (int i = 0; i < 9; ++i) R_out[bv * 9 + i] = Rs[i];
    for (int i = 0; i < 3; ++i) t_out[bv * 3 + i] = ts[i];
    ok_out[bv] = 0;
    return;
  }
  const float* Raf = R + (b * V + a) * 9;
  const float* taf = t + (b * V + a) * 3;
  double Ra[3][3], Rsd[3][3], ta[3], tsd[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    ta[i] = (double)taf[i];
    tsd[i] = (double)ts[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      Ra[i][j] = (double)Raf[i * 3 + j];
      Rsd[i][j] = (double)Rs[i * 3 + j];
    }
  }
  double M[3][3], N[3][3], u[3], ww[3], tn[3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i][j] = Rr[0][i] * Ra[0][j] + Rr[1][i] * Ra[1][j] + Rr[2][i] * Ra[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) N[i][j] = Ra[0][i] * M[0][j] + Ra[1][i] * M[1][j] + Ra[2][i] * M[2][j];
#pragma unroll
  for (int i = 0; i < 3; ++i) u[i] = ta[i] - x[3 + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) ww[i] = Rr[0][i] * u[0] + Rr[1][i] * u[1] + Rr[2][i] * u[2] - ta[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) tn[i] = Ra[0][i] * ww[0] + Ra[1][i] * ww[1] + Ra[2][i] * ww[2];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R_out[bv * 9 + i * 3 + j] = (float)(Rsd[i][0] * N[0][j] + Rsd[i][1] * N[1][j] + Rsd[i][2] * N[2][j]);
    t_out[bv * 3 + i] = (float)(Rsd[i][0] * tn[0] + Rsd[i][1] * tn[1] + Rsd[i][2] * tn[2] + tsd[i]);
  }
  ok_out[bv] = 1;
}

inline int icp_chunks(int H, int W) { return (int)(((long)H * W + kIcpChunk - 1) / kIcpChunk); }

}  // namespace

static int depth_normals_f32(const float* depth, const uint8_t* valid, const float* ray, float max_rel, float* normal,
                             int B, int V, int H, int W, hipStream_t stream) {
  const int tiles_x = ceil_div(W, 64), tiles = tiles_x * ceil_div(H, 4);
  depth_normals_kernel<<<dim3((unsigned)((long)tiles * B * V)), dim3(256), 0, stream>>>(depth, valid, ray, max_rel, normal,
                                                                                       H, W, tiles_x, tiles);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int depth_icp_system_f32(const float* depth, const uint8_t* valid, const float* normal, const float* ray,
                                const float* K, const float* R, const float* t, const int32_t* target, float max_dist,
                                double* system, float* residual, int64_t* assoc, int B, int V, int H, int W,
                                void* workspace, hipStream_t stream) {
  const int chunks = icp_chunks(H, W);
  double* partial = (double*)workspace;
  icp_system_kernel<<<dim3((unsigned)((long)B * V * chunks)), dim3(kIcpThreads), 0, stream>>>(
      depth, valid, normal, ray, K, R, t, target, max_dist * max_dist, partial, residual, assoc, V, H, W, chunks);
  CTD_LAUNCH_CHECK();
  icp_finish_kernel<<<dim3((unsigned)(B * V)), dim3(64), 0, stream>>>(partial, system, chunks);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int depth_icp_update_f32(const double* system, const float* R, const float* t, const int32_t* target,
                                int min_count, double min_pivot, double damping, float* R_out, float* t_out, uint8_t* ok,
                                int B, int V, hipStream_t stream) {
  const long views = (long)B * V;
  icp_update_kernel<<<dim3((unsigned)((views + 63) / 64)), dim3(64), 0, stream>>>(
      system, R, t, target, (double)min_count, min_pivot, damping, R_out, t_out, ok, V, views);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_depth_normals_f32(const float* depth, const uint8_t* valid, const float* ray, float max_rel, float* normal, int B,
                          int V, int H, int W, int device, void* stream) {
  if (!(max_rel >= 0.f) || !depth || !ray || !normal) return CTD_ERR_INVALID_ARG;
  const int st = track_shape_status(B, V, H, W);                 // the sizes: INVALID_ARG, then UNSUPPORTED
  if (st != CTD_OK) return st;
  if (!launch_ok((double)B * V * tiles_64x4(H, W))) return CTD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * V * H * W;
  const Span s[] = {{normal, 12 * n}, {depth, 4 * n}, {valid, n}, {ray, 12 * (size_t)H * W}};
  if (spans_overlap(s, 1, 4)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_normals_f32(depth, valid, ray, max_rel, normal, B, V, H, W, (hipStream_t)stream);
}

static int icp_system_shape_status(int B, int V, int H, int W) {
  const int st = track_shape_status(B, V, H, W);
  if (st != CTD_OK) return st;
  if (!launch_ok((double)B * V * (double)icp_chunks(H, W))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

size_t ctd_depth_icp_workspace_bytes(int B, int V, int H, int W) {
  if (B <= 0 || icp_system_shape_status(B, V, H, W) != CTD_OK) return 0;
  return align_up(sizeof(double) * kSys * (size_t)B * V * icp_chunks(H, W), 256);
}

int ctd_depth_icp_system_f32(const float* depth, const uint8_t* valid, const float* normal, const float* ray,
                             const float* K, const float* R, const float* t, const int32_t* target, float max_dist,
                             double* system, float* residual, int64_t* assoc, int B, int V, int H, int W, void* workspace,
                             size_t workspace_bytes, int device, void* stream) {
  if (!(max_dist >= 0.f) || !depth || !normal || !ray || !K || !R || !t || !system) return CTD_ERR_INVALID_ARG;
  const int st = icp_system_shape_status(B, V, H, W);          // the sizes: INVALID_ARG, then UNSUPPORTED
  if (st != CTD_OK) return st;
  const size_t n = (size_t)B * V * H * W, views = (size_t)B * V;
  const size_t need = ctd_depth_icp_workspace_bytes(B, V, H, W);
  const Span s[] = {{system, 8 * kSys * views}, {residual, 4 * n}, {assoc, 8 * n}, {workspace, need}, {depth, 4 * n},
                       {valid, n}, {normal, 12 * n}, {ray, 12 * (size_t)H * W}, {K, 36}, {R, 36 * views},
                       {t, 12 * views}, {target, 4 * views}};
  if (spans_overlap(s, 4, 12)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_icp_system_f32(depth, valid, normal, ray, K, R, t, target, max_dist, system, residual, assoc, B, V, H, W,
                              workspace, (hipStream_t)stream);
}

int ctd_depth_icp_update_f32(const double* system, const float* R, const float* t, const int32_t* target, int min_count,
                             double min_pivot, double damping, float* R_out, float* t_out, uint8_t* ok, int B, int V,
                             int device, void* stream) {
  if (V < 1 || B < 0 || V > 64 || min_count < 0 || !(min_pivot >= 0.0) || !(damping >= 0.0)) return CTD_ERR_INVALID_ARG;
  if (!system || !R || !t || !R_out || !t_out || !ok) return CTD_ERR_INVALID_ARG;
  if ((double)B * V >= 16777216.0) return CTD_ERR_UNSUPPORTED;
  const size_t views = (size_t)B * V;
  const Span s[] = {{R_out, 36 * views}, {t_out, 12 * views}, {ok, views}, {system, 8 * kSys * views}, {R, 36 * views},
                       {t, 12 * views}, {target, 4 * views}};
  if (spans_overlap(s, 3, 7)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_icp_update_f32(system, R, t, target, min_count, min_pivot, damping, R_out, t_out, ok, B, V,
                              (hipStream_t)stream);
}

}  // extern "C"
