// tsdf.hip -- truncated signed distance volumes: integration of a track's views, surface points and the model ray cast
// (ctd_tsdf_integrate_f32, ctd_tsdf_surface_points_f32, ctd_tsdf_raycast_f32; the rules are stated word for word in
// include/ctd_hip_tsdf.h).
//
// live_at() and camera_to_world() are those of ctd_view.h, the workgroup prefix and fuse_scan_kernel those of
// ctd_compact.h, the voxel of a thread, the usability rule and surf_count_kernel those of ctd_tsdf_surf.h (shared with
// tsdf_mesh.hip); every f32 product and sum is in the association of the header and the build never contracts them.
// Poses, K and origin are indexed by block-uniform values only (track, view, loop counter): scalar loads.
//   tsdf_integrate_kernel -- a tile of 64 (x) x 4 (y) voxels of one z slice of one track, thread = voxel, loop over the
//     views with tsdf and weight in registers.  A row of the tile is 256 contiguous bytes of the volume, and its 64
//     voxels project onto a short line of neighbouring pixels, four rows onto four such lines: the gather of depth,
//     valid and ray z of a view stays within a few cache lines per wavefront.  Per voxel 4 B weight read, 4 B tsdf where
//     the weight is not 0, per view that lands 5 B + 4 B gathered, 8 B written where a view touched the voxel.
//   surf_count_kernel     -- 256 consecutive voxels of ONE track (a chunk never crosses a track, so the workgroups are
//     in ascending `src` order): the three crossing flags of a voxel as one byte and the workgroup's number of points
//     (wg_flags3_before).  Per voxel 8 B read + the +x, +y, +z neighbours (cached rows), 1 B written.
//   fuse_scan_kernel      -- ONE workgroup: exclusive scan of the workgroup counts, then the per-track totals.
//   surf_scatter_kernel   -- the chunks again: offset of the workgroup + flags before the thread, and for each
//     flag the point, its src and, when asked for, the central-difference normal.  Per voxel 1 B read; per point 16 B read
//     (+ 48 B for a normal), 12 + 8 (+ 12) B written.
//   tsdf_raycast_kernel   -- a 64 x 4 tile of one view, thread = pixel: the march along the ray, eight weights and, where
//     the sample is defined, eight tsdf values per step; the ray leaves at its first crossing.  4 B written per pixel.
// No atomics, no flag that another workgroup waits on: the same bits on every run.
#include "../../include/ctd_hip_tsdf.h"
#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_tsdf_surf.h"
#include "ctd_validate.h"
#include "ctd_view.h"

namespace ctd {
namespace {

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(
    float* __restrict__ tsdf, float* __restrict__ weight, const float* __restrict__ origin, float voxel,
    const float* __restrict__ depth, const uint8_t* __restrict__ valid, const float* __restrict__ ray,
    const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ t, float trunc, float max_weight,
    Grid gr, int V, int H, int W, int tiles_x, int tiles) {
  const int tile = blockIdx.x % tiles, bk = blockIdx.x / tiles, b = bk / gr.nz, k = bk % gr.nz;
  const int i = (tile % tiles_x) * 64 + (threadIdx.x & 63), j = (tile / tiles_x) * 4 + (threadIdx.x >> 6);
  if (i >= gr.nx || j >= gr.ny) return;
  const long g = ((long)bk * gr.ny + j) * gr.nx + i, plane = (long)H * W;
  const float* ob = origin + (long)b * 3;
  const float X0 = ob[0] + voxel * (float)i, X1 = ob[1] + voxel * (float)j, X2 = ob[2] + voxel * (float)k;
  // world_to_camera() and project() of ctd_view.h, written out: through the calls the compiler schedules this loop otherwise
  float w = weight[g];
  float T = w == 0.f ? 0.f : tsdf[g];                          // tsdf is never read where weight == 0
  bool touched = false;
  for (int v = 0; v < V; ++v) {
    const long bv = (long)b * V + v;
    const float* Rv = R + bv * 9;
    const float* tv = t + bv * 3;
    float S[3], uvd[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) S[c] = X0 * Rv[c * 3 + 0] + X1 * Rv[c * 3 + 1] + X2 * Rv[c * 3 + 2] + tv[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) uvd[c] = S[0] * K[c * 3 + 0] + S[1] * K[c * 3 + 1] + S[2] * K[c * 3 + 2];
    if (!(uvd[2] > 0.f)) continue;
    const float xs = floorf(uvd[0] / uvd[2] + 0.5f), ys = floorf(uvd[1] / uvd[2] + 0.5f);
    // float compares first (a NaN fails them); W - 1 and H - 1 are exact in f32 (H, W <= 2^24)
    if (!(xs >= 0.f && xs <= (float)(W - 1) && ys >= 0.f && ys <= (float)(H - 1))) continue;
    const long q = (long)(int)ys * W + (int)xs, gq = bv * plane + q;
    if (!live_at(depth, valid, gq)) continue;
    const float sdf = depth[gq] * ray[q * 3 + 2] - S[2];
    if (sdf < -trunc) continue;
    const float obs = fminf(1.f, sdf / trunc);
    T = w == 0.f ? obs : (T * w + obs) / (w + 1.f);
    w = fminf(w + 1.f, max_weight);
    touched = true;
  }
  if (touched) {
    tsdf[g] = T;
    weight[g] = w;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kChunk) void surf_scatter_kernel(
    const float* __restrict__ tsdf, const float* __restrict__ weight, const float* __restrict__ origin, float voxel,
    float min_weight, const uint8_t* __restrict__ emit, const int* __restrict__ offsets, float* __restrict__ points,
    float* __restrict__ normals, int64_t* __restrict__ src, long capacity, Grid gr, long nvox, int chunks) {
  __shared__ int wave_n[kChunk / 64];
  const SurfVoxel s = surf_voxel_of_block(gr, nvox, chunks);
  const int f = s.p < nvox ? emit[s.g] : 0;
  int total;
  long o = (long)offsets[blockIdx.x] + wg_flags3_before<kChunk>(f, wave_n, total);
  if (!f) return;
  const float* ob = origin + (long)s.b * 3;
  const int idx[3] = {s.i, s.j, s.k}, dim[3] = {gr.nx, gr.ny, gr.nz};
  const long stride[3] = {1, gr.nx, (long)gr.nx * gr.ny};
  const float Ta = tsdf[s.g], nan = __builtin_nanf("");
  float X[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) X[c] = ob[c] + voxel * (float)idx[c];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!(f & (1 << c))) continue;
    if (o >= capacity) return;                                // ascending: every later point of the thread is past it too
    const float Tn = tsdf[s.g + stride[c]];
#pragma unroll
    for (int e = 0; e < 3; ++e) points[o * 3 + e] = e == c ? X[e] + voxel * (Ta / (Ta - Tn)) : X[e];
    src[o] = s.g * 3 + c;
    if (normals) {
      const bool at_n = fabsf(Tn) < fabsf(Ta);                // the voxel with the smaller |T|, a on a tie
      const long m = at_n ? s.g + stride[c] : s.g;
      float gd[3] = {nan, nan, nan};
      bool ok = true;
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const int ie = idx[e] + (at_n && e == c ? 1 : 0);
        if (ok && ie >= 1 && ie + 1 < dim[e] && weight[m + stride[e]] >= min_weight && weight[m - stride[e]] >= min_weight)
          gd[e] = tsdf[m + stride[e]] - tsdf[m - stride[e]];
        else
          ok = false;
      }
      float nv[3] = {nan, nan, nan};
      if (ok) {
        const float l2 = gd[0] * gd[0] + gd[1] * gd[1] + gd[2] * gd[2];
        if (l2 != 0.f) {
          const float l = sqrtf(l2);
#pragma unroll
          for (int e = 0; e < 3; ++e) nv[e] = gd[e] / l;
        }
      }
#pragma unroll
      for (int e = 0; e < 3; ++e) normals[o * 3 + e] = nv[e];
    }
    ++o;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                           const float* __restrict__ origin, float voxel,
                                                           const float* __restrict__ ray, const float* __restrict__ R,
                                                           const float* __restrict__ t, float d_min, float step,
                                                           int n_steps, float min_weight, float* __restrict__ depth,
                                                           Grid gr, int V, int H, int W, int tiles_x, int tiles) {
  const int tile = blockIdx.x % tiles;
  const long bv = blockIdx.x / tiles;
  const int b = (int)(bv / V);
  const int x = (tile % tiles_x) * 64 + (threadIdx.x & 63), y = (tile / tiles_x) * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long p = (long)y * W + x;
  const float* Rv = R + bv * 9;
  const float* tv = t + bv * 3;
  const float* ob = origin + (long)b * 3;
  const long sy = gr.nx, sz = (long)gr.nx * gr.ny, vol = (long)b * gr.nz * sz;
  const float r[3] = {ray[p * 3 + 0], ray[p * 3 + 1], ray[p * 3 + 2]};
  const float hx = (float)(gr.nx - 2), hy = (float)(gr.ny - 2), hz = (float)(gr.nz - 2);
  float out = __builtin_nanf("");
  bool prev_def = false;
  float prev_T = 0.f;
  for (int n = 0; n < n_steps; ++n) {
    const float d = d_min + step * (float)n;
    float X[3];
    camera_to_world(r, d, Rv, tv, X);
    const float g0 = (X[0] - ob[0]) / voxel, g1 = (X[1] - ob[1]) / voxel, g2 = (X[2] - ob[2]) / voxel;
    const float i0 = floorf(g0), i1 = floorf(g1), i2 = floorf(g2);
    bool def = i0 >= 0.f && i0 <= hx && i1 >= 0.f && i1 <= hy && i2 >= 0.f && i2 <= hz;   // (a NaN fails the compares)
    float T = 0.f;
    if (def) {
      const long base = vol + (long)(int)i2 * sz + (long)(int)i1 * sy + (int)i0;
      const long c[8] = {base, base + 1, base + sy, base + sy + 1, base + sz, base + sz + 1, base + sz + sy, base + sz + sy + 1};
#pragma unroll
      for (int e = 0; e < 8; ++e) def = def && weight[c[e]] >= min_weight;
      if (def) {
        const float fx = g0 - i0, fy = g1 - i1, fz = g2 - i2;
        float a[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float T0 = tsdf[c[2 * e]], T1 = tsdf[c[2 * e + 1]];
          a[e] = T0 + fx * (T1 - T0);
        }
        const float lo = a[0] + fy * (a[1] - a[0]), hi = a[2] + fy * (a[3] - a[2]);
        T = lo + fz * (hi - lo);
      }
    }
    if (def && T <= 0.f) {
      if (prev_def && prev_T > 0.f) out = (d_min + step * (float)(n - 1)) + step * (prev_T / (prev_T - T));
      break;
    }
    prev_def = def;
    prev_T = T;
  }
  depth[bv * (long)H * W + p] = out;
}

struct SurfLayout {                                           // byte offsets into the workspace
  size_t emit, offsets, bytes;
};
SurfLayout surf_layout(int B, int nx, int ny, int nz) {
  WorkspaceCursor c;
  SurfLayout l;
  l.emit = c.take((size_t)B * nx * ny * nz);
  l.offsets = c.take_counts((size_t)B * surf_chunks(nx, ny, nz));
  l.bytes = c.bytes;
  return l;
}

}  // namespace

static int tsdf_integrate_f32(float* tsdf, float* weight, const float* origin, float voxel, const float* depth,
                              const uint8_t* valid, const float* ray, const float* K, const float* R, const float* t,
                              float trunc, float max_weight, int B, int nx, int ny, int nz, int V, int H, int W,
                              hipStream_t stream) {
  const int tiles_x = ceil_div(nx, 64), tiles = tiles_x * ceil_div(ny, 4);
  const Grid gr = {nx, ny, nz};
  tsdf_integrate_kernel<<<dim3((unsigned)((long)tiles * B * nz)), dim3(256), 0, stream>>>(
      tsdf, weight, origin, voxel, depth, valid, ray, K, R, t, trunc, max_weight, gr, V, H, W, tiles_x, tiles);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int tsdf_surface_points_f32(const float* tsdf, const float* weight, const float* origin, float voxel,
                                   float min_weight, float* points, float* normals, int64_t* src, int64_t* n_per_track,
                                   int64_t capacity, int B, int nx, int ny, int nz, void* workspace, hipStream_t stream) {
  const SurfLayout l = surf_layout(B, nx, ny, nz);
  uint8_t* emit = (uint8_t*)workspace + l.emit;
  int* offsets = (int*)((char*)workspace + l.offsets);
  const Grid gr = {nx, ny, nz};
  const long nvox = (long)nx * ny * nz;
  const int chunks = (int)surf_chunks(nx, ny, nz), blocks = B * chunks;
  surf_count_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(tsdf, weight, min_weight, emit, offsets, gr,
                                                                            nvox, chunks);
  CTD_LAUNCH_CHECK();
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(offsets, blocks, chunks, n_per_track, B);
  CTD_LAUNCH_CHECK();
  if (!points || capacity == 0) return CTD_OK;
  surf_scatter_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(
      tsdf, weight, origin, voxel, min_weight, emit, offsets, points, normals, src, (long)capacity, gr, nvox, chunks);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int tsdf_raycast_f32(const float* tsdf, const float* weight, const float* origin, float voxel, const float* ray,
                            const float* R, const float* t, float d_min, float step, int n_steps, float min_weight,
                            float* depth, int B, int nx, int ny, int nz, int V, int H, int W, hipStream_t stream) {
  const int tiles_x = ceil_div(W, 64), tiles = tiles_x * ceil_div(H, 4);
  const Grid gr = {nx, ny, nz};
  tsdf_raycast_kernel<<<dim3((unsigned)((long)tiles * B * V)), dim3(256), 0, stream>>>(
      tsdf, weight, origin, voxel, ray, R, t, d_min, step, n_steps, min_weight, depth, gr, V, H, W, tiles_x, tiles);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_tsdf_integrate_f32(float* tsdf, float* weight, const float* origin, float voxel, const float* depth,
                           const uint8_t* valid, const float* ray, const float* K, const float* R, const float* t,
                           float trunc, float max_weight, int B, int nx, int ny, int nz, int V, int H, int W, int device,
                           void* stream) {
  if (grid_status(B, nx, ny, nz, true) != CTD_OK || track_shape_invalid(B, V, H, W)) return CTD_ERR_INVALID_ARG;
  if (!positive_finite(voxel) || !positive_finite(trunc) || !(max_weight >= 1.f && max_weight < __builtin_inff()))
    return CTD_ERR_INVALID_ARG;
  if (!tsdf || !weight || !origin || !depth || !ray || !K || !R || !t) return CTD_ERR_INVALID_ARG;
  if (grid_status(B, nx, ny, nz, false) != CTD_OK || track_shape_unsupported(B, V, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!launch_ok((double)B * nz * tiles_64x4(ny, nx))) return CTD_ERR_UNSUPPORTED;
  const size_t nv = (size_t)B * nx * ny * nz, n = (size_t)B * V * H * W, views = (size_t)B * V;
  const Span s[] = {{tsdf, 4 * nv}, {weight, 4 * nv}, {origin, 12 * (size_t)B}, {depth, 4 * n}, {valid, n},
                    {ray, 12 * (size_t)H * W}, {K, 36}, {R, 36 * views}, {t, 12 * views}};
  if (spans_overlap(s, 2, 9)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return tsdf_integrate_f32(tsdf, weight, origin, voxel, depth, valid, ray, K, R, t, trunc, max_weight, B, nx, ny, nz, V, H,
                            W, (hipStream_t)stream);
}

size_t ctd_tsdf_surface_workspace_bytes(int B, int nx, int ny, int nz) {
  if (B <= 0 || surf_shape_status(B, nx, ny, nz) != CTD_OK) return 0;
  return surf_layout(B, nx, ny, nz).bytes;
}

int ctd_tsdf_surface_points_f32(const float* tsdf, const float* weight, const float* origin, float voxel, float min_weight,
                                float* points, float* normals, int64_t* src, int64_t* n_per_track, int64_t capacity, int B,
                                int nx, int ny, int nz, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (grid_status(B, nx, ny, nz, true) != CTD_OK || !positive_finite(voxel) || !positive_finite(min_weight))
    return CTD_ERR_INVALID_ARG;
  if (!tsdf || !weight || !origin || !n_per_track || (points && (capacity < 0 || !src))) return CTD_ERR_INVALID_ARG;
  const int st = surf_shape_status(B, nx, ny, nz);
  if (st != CTD_OK) return st;
  const size_t nv = (size_t)B * nx * ny * nz;
  const size_t cap = !points ? 0 : (size_t)capacity < 3 * nv ? (size_t)capacity : 3 * nv;   // no more points than 3 a voxel
  const size_t need = ctd_tsdf_surface_workspace_bytes(B, nx, ny, nz);
  const Span s[] = {{points, 12 * cap}, {points ? normals : nullptr, 12 * cap}, {points ? src : nullptr, 8 * cap},
                    {n_per_track, 8 * (size_t)B}, {workspace, need}, {tsdf, 4 * nv}, {weight, 4 * nv},
                    {origin, 12 * (size_t)B}};
  if (spans_overlap(s, 5, 8)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return tsdf_surface_points_f32(tsdf, weight, origin, voxel, min_weight, points, normals, src, n_per_track, capacity, B,
                                 nx, ny, nz, workspace, (hipStream_t)stream);
}

int ctd_tsdf_raycast_f32(const float* tsdf, const float* weight, const float* origin, float voxel, const float* ray,
                         const float* R, const float* t, float d_min, float step, int n_steps, float min_weight,
                         float* depth, int B, int nx, int ny, int nz, int V, int H, int W, int device, void* stream) {
  if (grid_status(B, nx, ny, nz, true) != CTD_OK || track_shape_invalid(B, V, H, W) || n_steps < 1)
    return CTD_ERR_INVALID_ARG;
  if (!positive_finite(voxel) || !positive_finite(step) || !positive_finite(min_weight) || !nonneg_finite(d_min))
    return CTD_ERR_INVALID_ARG;
  if (!tsdf || !weight || !origin || !ray || !R || !t || !depth) return CTD_ERR_INVALID_ARG;
  if (grid_status(B, nx, ny, nz, false) != CTD_OK || track_shape_unsupported(B, V, H, W)) return CTD_ERR_UNSUPPORTED;
  if (!launch_ok((double)B * V * tiles_64x4(H, W))) return CTD_ERR_UNSUPPORTED;
  const size_t nv = (size_t)B * nx * ny * nz, n = (size_t)B * V * H * W, views = (size_t)B * V;
  const Span s[] = {{depth, 4 * n}, {tsdf, 4 * nv}, {weight, 4 * nv}, {origin, 12 * (size_t)B}, {ray, 12 * (size_t)H * W},
                    {R, 36 * views}, {t, 12 * views}};
  if (spans_overlap(s, 1, 7)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return tsdf_raycast_f32(tsdf, weight, origin, voxel, ray, R, t, d_min, step, n_steps, min_weight, depth, B, nx, ny, nz, V,
                          H, W, (hipStream_t)stream);
}

}  // extern "C"
