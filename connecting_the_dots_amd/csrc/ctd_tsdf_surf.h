// ctd_tsdf_surf.h -- what tsdf.hip (the surface points) and tsdf_mesh.hip (the faces over those points) share: the
// voxel of a thread, the usability rule of include/ctd_hip_tsdf.h, the crossing-flag count kernel and the checks of a
// grid's sizes.  The faces index the points, so both files must flag, count and order the crossings with the same
// code: it lives here once, over the chunks and the prefixes of ctd_compact.h.
#pragma once

#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

struct Grid {
  int nx, ny, nz;
};

// the voxel of a thread of the count and scatter kernels: voxel p = (i, j, k) of track b (p >= nvox: past the track's end)
struct SurfVoxel {
  int b, i, j, k;
  long p, g;
};
__device__ inline SurfVoxel surf_voxel_of_block(Grid gr, long nvox, int chunks) {
  const ChunkItem c = chunk_item(chunks);
  SurfVoxel s;
  s.b = c.group;
  s.p = c.p;
  s.g = (long)s.b * nvox + s.p;
  s.i = (int)(s.p % gr.nx);
  s.j = (int)((s.p / gr.nx) % gr.ny);
  s.k = (int)(s.p / ((long)gr.nx * gr.ny));
  return s;
}

// usable: weight >= min_weight and |tsdf| < 1 (the tsdf is read only behind the weight); T = the tsdf, else unset
__device__ inline bool surf_usable(const float* __restrict__ tsdf, const float* __restrict__ weight, long g,
                                   float min_weight, float& T) {
  if (!(weight[g] >= min_weight)) return false;
  T = tsdf[g];
  return fabsf(T) < 1.f;
}

__global__ __launch_bounds__(kChunk) void surf_count_kernel(const float* __restrict__ tsdf,
                                                            const float* __restrict__ weight, float min_weight,
                                                            uint8_t* __restrict__ emit, int* __restrict__ wg_count, Grid gr,
                                                            long nvox, int chunks) {
  __shared__ int wave_n[kChunk / 64];
  const SurfVoxel s = surf_voxel_of_block(gr, nvox, chunks);
  int f = 0;
  if (s.p < nvox) {
    float Ta;
    if (surf_usable(tsdf, weight, s.g, min_weight, Ta)) {
      const bool inside[3] = {s.i + 1 < gr.nx, s.j + 1 < gr.ny, s.k + 1 < gr.nz};
      const long stride[3] = {1, gr.nx, (long)gr.nx * gr.ny};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        float Tn;
        if (inside[c] && surf_usable(tsdf, weight, s.g + stride[c], min_weight, Tn) && (Ta < 0.f) != (Tn < 0.f))
          f |= 1 << c;
      }
    }
    emit[s.g] = (uint8_t)f;
  }
  int total;
  (void)wg_flags3_before<kChunk>(f, wave_n, total);
  if (threadIdx.x == 0) wg_count[blockIdx.x] = total;
}

inline long surf_chunks(int nx, int ny, int nz) { return chunks_of((long)nx * ny * nz); }

// 0 ok, else the status of the first failing check of the grid's sizes
inline int grid_status(int B, int nx, int ny, int nz, bool invalid_only) {
  if (nx < 1 || ny < 1 || nz < 1 || B < 0) return CTD_ERR_INVALID_ARG;
  if (invalid_only) return CTD_OK;
  if (nx > 2048 || ny > 2048 || nz > 2048 || (double)B * nx * ny * nz >= 2147483648.0) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

inline int surf_shape_status(int B, int nx, int ny, int nz) {
  const int st = grid_status(B, nx, ny, nz, false);
  if (st != CTD_OK) return st;
  if (3.0 * B * nx * ny * nz >= 2147483648.0 || !launch_ok((double)B * surf_chunks(nx, ny, nz))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

}  // namespace
}  // namespace ctd
