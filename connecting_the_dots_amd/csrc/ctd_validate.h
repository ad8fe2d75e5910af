// ctd_validate.h -- argument predicates that the C entry points of more than one kernel family share.
#pragma once
#include "ctd_common.h"

namespace ctd {

inline bool vol_shape_ok(int frames, int C, int H, int W, int D, int bs) {
  if (frames < 0 || C <= 0 || H <= 0 || W <= 0 || D <= 0 || bs <= 0) return false;
  // the reference indexes outputs with int (common_cuda.h:65-66, ext_cpu.cpp:8-9)
  if ((double)D * H * W >= 2147483648.0) return false;
  return true;
}

inline bool photo_shape_ok(int B, int C, int H, int W, int bs, int type) {
  return B >= 0 && C > 0 && H > 0 && W > 0 && bs > 0 && type >= 0 && type <= 3 &&
         (double)B * C * H * W < 2147483648.0;                 // int indices in the reference (ext.h:220-235)
}

inline bool img_shape_ok(int B, int H, int W) {
  return B > 0 && H > 0 && W > 0 && B <= 65535 && (double)B * H * W < 2147483648.0;
}

inline bool positive_finite(float v) { return v > 0.f && v < __builtin_inff(); }   // (a NaN fails the compares)
inline bool nonneg_finite(float v) { return v >= 0.f && v < __builtin_inff(); }

// The sizes of a track's images [B][V][H][W] (depth_fusion.hip, depth_warp.hip, depth_icp.hip, tsdf.hip), the two
// classes apart for the entry points that test something else in between.  H, W <= 2^24: the bounds of a projected
// pixel are compared in f32, where W - 1 and H - 1 must be exact.
inline bool track_shape_invalid(int B, int V, int H, int W) { return V < 1 || H < 1 || W < 1 || B < 0 || V > 64; }
inline bool track_shape_unsupported(int B, int V, int H, int W) {
  return H > (1 << 24) || W > (1 << 24) || (double)B * V * H * W >= 2147483648.0;
}
inline int track_shape_status(int B, int V, int H, int W) {
  if (track_shape_invalid(B, V, H, W)) return CTD_ERR_INVALID_ARG;
  return track_shape_unsupported(B, V, H, W) ? CTD_ERR_UNSUPPORTED : CTD_OK;
}

// a launch stays below 2^32 threads: fewer than 2^24 workgroups of 256
inline bool launch_ok(double workgroups) { return workgroups < 16777216.0; }
// the number of 64 x 4 tiles (256 threads) of an H x W plane
inline double tiles_64x4(int H, int W) { return (double)(((long)H + 3) / 4) * (double)(((long)W + 63) / 64); }

inline bool workspace_ok(const void* workspace, size_t bytes, size_t need) {
  return workspace && bytes >= need && !((uintptr_t)workspace & 255);
}

// hands out the byte offsets of a workspace's parts, each 256-aligned, in the order taken; bytes = the size so far
struct WorkspaceCursor {
  size_t bytes = 0;
  size_t take(size_t n) {
    const size_t at = bytes;
    bytes += align_up(n, 256);
    return at;
  }
  size_t take_counts(size_t n) { return take(sizeof(int) * (n + 1)); }   // n workgroup counts and the scan's total
};

// a buffer of a call, for the overlap check of the entry points that state one (depth_fusion.hip, depth_icp.hip,
// tsdf.hip, tsdf_mesh.hip, mesh_clean.hip)
struct Span {
  const void* p;
  size_t bytes;
};
// true when one of the first n_out spans (the buffers a call writes) shares a byte with any other span; NULL spans are absent
inline bool spans_overlap(const Span* s, int n_out, int n) {
  for (int i = 0; i < n_out; ++i)
    for (int j = 0; j < n; ++j) {
      if (j == i || (j < n_out && j < i) || !s[i].p || !s[j].p || !s[i].bytes || !s[j].bytes) continue;
      const uintptr_t a = (uintptr_t)s[i].p, b = (uintptr_t)s[j].p;
      if (a < b + s[j].bytes && b < a + s[i].bytes) return true;
    }
  return false;
}

}  // namespace ctd

// ctd_photometric_{fwd,bwd}_<SFX> over the launchers photometric_{fwd,bwd}_<SFX> of the including file
// (photometric.hip: f32, f64; photometric_fast.hip: fast_f32)
#define CTD_PHOTO_ENTRY(SFX, T)                                                                                   \
  int ctd_photometric_fwd_##SFX(const T* es, const T* ta, T* out, int B, int C, int H, int W, int block_size,      \
                                int type, float eps, int device, void* stream) {                                   \
    if (!photo_shape_ok(B, C, H, W, block_size, type)) return CTD_ERR_INVALID_ARG;                                 \
    if (B == 0) return CTD_OK;                                                                                     \
    if (!es || !ta || !out) return CTD_ERR_INVALID_ARG;                                                            \
    DeviceGuard g(device);                                                                                         \
    if (g.status) return g.status;                                                                                 \
    return photometric_fwd_##SFX(es, ta, out, B, C, H, W, block_size, type, eps, (hipStream_t)stream);             \
  }                                                                                                                \
  int ctd_photometric_bwd_##SFX(const T* es, const T* ta, const T* grad_out, T* grad_es, int B, int C, int H,      \
                                int W, int block_size, int type, float eps, int device, void* stream) {            \
    if (!photo_shape_ok(B, C, H, W, block_size, type)) return CTD_ERR_INVALID_ARG;                                 \
    if (B == 0) return CTD_OK;                                                                                     \
    if (!es || !ta || !grad_out || !grad_es) return CTD_ERR_INVALID_ARG;                                           \
    DeviceGuard g(device);                                                                                         \
    if (g.status) return g.status;                                                                                 \
    return photometric_bwd_##SFX(es, ta, grad_out, grad_es, B, C, H, W, block_size, type, eps, (hipStream_t)stream); \
  }
