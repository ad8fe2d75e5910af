// depth_fusion.hip -- multi-view depth consistency and point-cloud fusion of a track's depth maps [B][V][H][W]
// (ctd_depth_consistency_f32, ctd_depth_fuse_points_f32; the rules are stated word for word in include/ctd_hip.h).
//
// view_match() is the one place that projects a pixel of view r into view s, samples the nearest source pixel, projects
// it back and decides consistency; the consistency pass and the emit pass of the fusion both call it, so the two cannot
// drift apart.  live_at(), view_transform() and camera_to_world() are those of ctd_view.h, where every product and sum
// is in the association of the header; the chunks, the workgroup prefix and the scan are those of ctd_compact.h.  Poses
// and K are indexed by block-uniform values only (track, view, loop counter): scalar loads.
//   depth_consistency_kernel -- a 64 x 4 tile of one view, thread = reference pixel, loop over the source views.
//     Per pixel: 5 B read + 12 B ray, per source view one 5 B gather + 12 B ray of the pixel hit; 6 B written.
//   fuse_count_kernel   -- 256 consecutive pixels of ONE view (a chunk never crosses a view, so the pose stays uniform
//     and the workgroups are in ascending `src` order): the emit flag (with dedupe: the projections into the views
//     s < r again, and keep of the pixel hit) and the workgroup's number of flags (wg_flags_before).
//     Per pixel: 1 B read + 1 B written; with dedupe, for a kept pixel, 4 + 12 B and per earlier view 5 + 12 + 1 B.
//   fuse_scan_kernel    -- (ctd_compact.h) ONE workgroup: exclusive scan of the workgroup counts, 1024 at a time with
//     a carry, then the per-track totals as differences of the scanned offsets.
//   fuse_scatter_kernel -- the chunks again: offset of the workgroup + flags before the thread, and for a flagged
//     pixel the world point and its flat index.  Per pixel 1 B read; per point 4 + 12 B read, 12 + 8 B written.
// Three launches behind the consistency pass, no flag that another workgroup waits on, no atomics: the same bits on every run.
#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_validate.h"
#include "ctd_view.h"

namespace ctd {
namespace {

struct FuseTol {
  float max_px2, max_rel;                                     // max_px * max_px (one f32 product), max_rel
};

// Steps a, b, c of the header for the live pixel (x, y) of view r, depth d_r, against view s of the same track
// (depth, valid, R, t point at the track).  true = consistent; q = the source pixel of step a, z = z' of step b.
__device__ inline bool view_match(const float* __restrict__ depth, const uint8_t* __restrict__ valid,
                                  const float* __restrict__ ray, const float* __restrict__ K,
                                  const float* __restrict__ R, const float* __restrict__ t, int r, int s, int H, int W,
                                  int x, int y, float d_r, FuseTol tol, long& q, float& z) {
  const long plane = (long)H * W;
  float uvd[3];
  view_transform(ray + ((long)y * W + x) * 3, d_r, R + r * 9, t + r * 3, R + s * 9, t + s * 3, K, uvd);
  if (!(uvd[2] > 0.f)) return false;
  const float xs = floorf(uvd[0] / uvd[2] + 0.5f), ys = floorf(uvd[1] / uvd[2] + 0.5f);
  // float compares first (a NaN fails them); W - 1 and H - 1 are exact in f32 (H, W <= 2^24)
  if (!(xs >= 0.f && xs <= (float)(W - 1) && ys >= 0.f && ys <= (float)(H - 1))) return false;
  q = (long)(int)ys * W + (int)xs;
  const long gs = s * plane + q;
  if (!live_at(depth, valid, gs)) return false;
  view_transform(ray + q * 3, depth[gs], R + s * 9, t + s * 3, R + r * 9, t + r * 3, K, uvd);
  if (!(uvd[2] > 0.f)) return false;
  z = uvd[2];
  const float du = uvd[0] / uvd[2] - (float)x, dv = uvd[1] / uvd[2] - (float)y;
  return du * du + dv * dv <= tol.max_px2 && fabsf(z - d_r) <= tol.max_rel * d_r;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void depth_consistency_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ valid, const float* __restrict__ ray,
    const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ t, uint8_t* __restrict__ count,
    uint8_t* __restrict__ keep, float* __restrict__ fused, int V, int H, int W, int tiles_x, int tiles, FuseTol tol,
    int min_views) {
  const int tile = blockIdx.x % tiles, bv = blockIdx.x / tiles, b = bv / V, r = bv % V;
  const int x = (tile % tiles_x) * 64 + (threadIdx.x & 63), y = (tile / tiles_x) * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const long plane = (long)H * W, track = (long)b * V * plane, g = (long)bv * plane + (long)y * W + x;
  depth += track;
  if (valid) valid += track;
  R += (long)b * V * 9;
  t += (long)b * V * 3;
  const long gl = g - track;
  const bool live = live_at(depth, valid, gl);
  const float d_r = depth[gl];
  int n = 0;
  float acc = d_r;
  for (int s = 0; s < V; ++s) {
    long q;
    float z;
    if (live && s != r && view_match(depth, valid, ray, K, R, t, r, s, H, W, x, y, d_r, tol, q, z)) {
      ++n;
      acc = acc + z;
    }
  }
  const bool k = live && n >= min_views;
  if (count) count[g] = (uint8_t)n;
  keep[g] = k ? 1 : 0;
  fused[g] = k ? acc / (float)(1 + n) : __builtin_nanf("");
}

__global__ __launch_bounds__(kChunk) void fuse_count_kernel(
    const float* __restrict__ depth, const uint8_t* __restrict__ valid, const float* __restrict__ ray,
    const float* __restrict__ K, const float* __restrict__ R, const float* __restrict__ t,
    const uint8_t* __restrict__ keep, uint8_t* __restrict__ emit, int* __restrict__ wg_count, int V, int H, int W,
    int chunks, FuseTol tol, int dedupe) {
  __shared__ int wave_n[kChunk / 64];
  const ChunkItem c = chunk_item(chunks);                     // pixel c.p of the view c.group = view r of track b
  const int b = c.group / V, r = c.group % V;
  const long plane = (long)H * W, g = (long)c.group * plane + c.p;
  bool e = false;
  if (c.p < plane) {
    e = keep[g] != 0;
    if (e && dedupe && r > 0) {                               // first view wins: an earlier view that confirms and keeps it
      const long track = (long)b * V * plane;
      const float* dt = depth + track;
      const uint8_t* vt = valid ? valid + track : nullptr;
      const float d_r = dt[g - track];
      const int x = (int)(c.p % W), y = (int)(c.p / W);
      for (int s = 0; s < r; ++s) {
        long q;
        float z;
        if (e && view_match(dt, vt, ray, K, R + (long)b * V * 9, t + (long)b * V * 3, r, s, H, W, x, y, d_r, tol, q, z) &&
            keep[track + s * plane + q])
          e = false;
      }
    }
    emit[g] = e ? 1 : 0;
  }
  int total;
  (void)wg_flags_before<kChunk>(e, wave_n, total);
  if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
}

__global__ __launch_bounds__(kChunk) void fuse_scatter_kernel(
    const uint8_t* __restrict__ emit, const float* __restrict__ fused, const float* __restrict__ ray,
    const float* __restrict__ R, const float* __restrict__ t, const int* __restrict__ offsets, float* __restrict__ points,
    int64_t* __restrict__ src, int V, int H, int W, int chunks) {
  __shared__ int wave_n[kChunk / 64];
  const ChunkItem c = chunk_item(chunks);                     // pixel c.p of the view c.group
  const long plane = (long)H * W, g = (long)c.group * plane + c.p;
  const bool e = c.p < plane && emit[g] != 0;
  int total;
  const long o = (long)offsets[blockIdx.x] + wg_flags_before<kChunk>(e, wave_n, total);
  if (!e) return;
  camera_to_world(ray + c.p * 3, fused[g], R + (long)c.group * 9, t + (long)c.group * 3, points + o * 3);
  src[o] = g;
}

inline int plane_chunks(int H, int W) { return (int)chunks_of((long)H * W); }

struct FuseLayout {                                           // byte offsets into the workspace
  size_t keep, fused, emit, offsets, bytes;
};
FuseLayout fuse_layout(int B, int V, int H, int W) {
  const size_t n = (size_t)B * V * H * W;
  WorkspaceCursor c;
  FuseLayout l;
  l.keep = c.take(n);
  l.fused = c.take(4 * n);
  l.emit = c.take(n);
  l.offsets = c.take_counts((size_t)B * V * plane_chunks(H, W));
  l.bytes = c.bytes;
  return l;
}

}  // namespace

static bool depth_fusion_supported(int B, int V, int H, int W) {
  const double views = (double)B * V;                         // the tiles of the consistency pass, the chunks of the fusion
  return launch_ok(views * tiles_64x4(H, W)) && launch_ok(views * plane_chunks(H, W));
}

static int depth_consistency_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K,
                                 const float* R, const float* t, float max_px, float max_rel, int min_views,
                                 uint8_t* count, uint8_t* keep, float* fused, int B, int V, int H, int W,
                                 hipStream_t stream) {
  const FuseTol tol = {max_px * max_px, max_rel};
  const int tiles_x = ceil_div(W, 64), tiles = tiles_x * ceil_div(H, 4);          // <= H * W, so the grid is < 2^31
  depth_consistency_kernel<<<dim3((unsigned)((long)tiles * B * V)), dim3(256), 0, stream>>>(
      depth, valid, ray, K, R, t, count, keep, fused, V, H, W, tiles_x, tiles, tol, min_views);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int depth_fuse_points_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K,
                                 const float* R, const float* t, float max_px, float max_rel, int min_views, int dedupe,
                                 float* points, int64_t* src, int64_t* n_per_track, uint8_t* count, uint8_t* keep,
                                 float* fused, int B, int V, int H, int W, void* workspace, hipStream_t stream) {
  const FuseLayout l = fuse_layout(B, V, H, W);
  char* ws = (char*)workspace;
  if (!keep) keep = (uint8_t*)(ws + l.keep);
  if (!fused) fused = (float*)(ws + l.fused);
  uint8_t* emit = (uint8_t*)(ws + l.emit);
  int* offsets = (int*)(ws + l.offsets);
  const int st = depth_consistency_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, count, keep, fused, B, V, H,
                                       W, stream);
  if (st != CTD_OK) return st;
  const FuseTol tol = {max_px * max_px, max_rel};
  const int chunks = plane_chunks(H, W), blocks = B * V * chunks;
  fuse_count_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(depth, valid, ray, K, R, t, keep, emit, offsets,
                                                                         V, H, W, chunks, tol, dedupe);
  CTD_LAUNCH_CHECK();
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(offsets, blocks, V * chunks, n_per_track, B);
  CTD_LAUNCH_CHECK();
  fuse_scatter_kernel<<<dim3((unsigned)blocks), dim3(kChunk), 0, stream>>>(emit, fused, ray, R, t, offsets, points, src,
                                                                           V, H, W, chunks);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

static bool depth_fusion_sizes_ok(int B, int V, int H, int W) {
  // this family answers INVALID_ARG to the sizes track_shape_status() calls UNSUPPORTED, and UNSUPPORTED to V > 64
  return B >= 0 && V >= 1 && H >= 1 && W >= 1 && !track_shape_unsupported(B, V, H, W);
}

static bool depth_fusion_params_ok(float max_px, float max_rel, int min_views) {
  return nonneg_finite(max_px) && nonneg_finite(max_rel) && min_views >= 0 && min_views <= 255;
}

int ctd_depth_consistency_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                              const float* t, float max_px, float max_rel, int min_views, uint8_t* count, uint8_t* keep,
                              float* fused, int B, int V, int H, int W, int device, void* stream) {
  if (!depth_fusion_sizes_ok(B, V, H, W) || !depth_fusion_params_ok(max_px, max_rel, min_views)) return CTD_ERR_INVALID_ARG;
  if (!depth || !ray || !K || !R || !t || !count || !keep || !fused) return CTD_ERR_INVALID_ARG;
  if (V > 64 || !depth_fusion_supported(B, V, H, W)) return CTD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * V * H * W, views = (size_t)B * V;
  const Span s[] = {{count, n}, {keep, n}, {fused, 4 * n}, {depth, 4 * n}, {valid, n}, {ray, 12 * (size_t)H * W},
                    {K, 36}, {R, 36 * views}, {t, 12 * views}};
  if (spans_overlap(s, 3, 9)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_consistency_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, count, keep, fused, B, V, H, W,
                               (hipStream_t)stream);
}

size_t ctd_depth_fuse_workspace_bytes(int B, int V, int H, int W) {
  if (B <= 0 || V > 64 || !depth_fusion_sizes_ok(B, V, H, W) || !depth_fusion_supported(B, V, H, W)) return 0;
  return fuse_layout(B, V, H, W).bytes;
}

int ctd_depth_fuse_points_f32(const float* depth, const uint8_t* valid, const float* ray, const float* K, const float* R,
                              const float* t, float max_px, float max_rel, int min_views, int dedupe, float* points,
                              int64_t* src, int64_t* n_per_track, uint8_t* count, uint8_t* keep, float* fused, int B,
                              int V, int H, int W, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (!depth_fusion_sizes_ok(B, V, H, W) || !depth_fusion_params_ok(max_px, max_rel, min_views)) return CTD_ERR_INVALID_ARG;
  if (!depth || !ray || !K || !R || !t || !points || !src || !n_per_track) return CTD_ERR_INVALID_ARG;
  if (V > 64 || !depth_fusion_supported(B, V, H, W)) return CTD_ERR_UNSUPPORTED;
  const size_t n = (size_t)B * V * H * W, views = (size_t)B * V;
  const size_t need = ctd_depth_fuse_workspace_bytes(B, V, H, W);
  const Span s[] = {{points, 12 * n}, {src, 8 * n}, {n_per_track, 8 * (size_t)B}, {count, n}, {keep, n}, {fused, 4 * n},
                    {workspace, need}, {depth, 4 * n}, {valid, n}, {ray, 12 * (size_t)H * W}, {K, 36}, {R, 36 * views},
                    {t, 12 * views}};
  if (spans_overlap(s, 7, 13)) return CTD_ERR_INVALID_ARG;
  if (B == 0) return CTD_OK;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return depth_fuse_points_f32(depth, valid, ray, K, R, t, max_px, max_rel, min_views, dedupe, points, src, n_per_track,
                               count, keep, fused, B, V, H, W, workspace, (hipStream_t)stream);
}

}  // extern "C"
