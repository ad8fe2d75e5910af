// mesh_global.hip -- the pose scoring of the global point-to-mesh registration (ctd_pose_score_u8; the rule is stated word
// for word in include/ext/ctd_hip_mesh_global.h): a point set under n_rot x n_off candidate poses against a volume of
// quantised unsigned distances, one exact integer per pose.
//
// Every f32 product, sum and quotient is in the association of the header and the build never contracts them.
//   pose_score_kernel -- workgroup = one rotation and a tile of kTile = 8 offsets, 256 threads.  R_m, base_m, the tile's
//     offsets, origin and voxel are the same for every lane: scalar loads, SGPRs.  Thread i takes the points i, i + 256,
//     ...: 12 B of the point, Q once, then per offset three adds, three (S - origin) / voxel, the three floor and bounds
//     tests on the floats, and ONE byte gathered from the volume, squared into the offset's own uint32 accumulator (a
//     whole score fits 32 bits: n_points <= 65536).  A point outside the volume loads voxel (0,0,0) and adds 255^2.  A
//     butterfly over the wavefront, the four wavefronts' sums through 128 B of LDS, one int64 store per offset by the
//     first kTile threads.  The tile's offsets past n_off are computed on the last real offset and not stored.
// Integer sums: no atomics, and the same bits whatever the order.
#include <cstdint>

#include "../../include/ext/ctd_hip_mesh_global.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

constexpr int kScoreThreads = 256;
constexpr int kTile = 8;                                       // offsets per workgroup
constexpr int kMaxScorePoints = 65536;                         // 65536 * 255^2 < 2^32
constexpr int kMaxOffsets = 4096;
constexpr int kMaxDim = 1024;
constexpr long kMaxGroups = (1L << 24) - 1;                    // a launch stays below 2^32 threads

__global__ __launch_bounds__(kScoreThreads) void pose_score_kernel(
    const float* __restrict__ points, int n_points, const float* __restrict__ R, const float* __restrict__ base,
    const float* __restrict__ offsets, int n_off, const uint8_t* __restrict__ levels, int nx, int ny, int nz,
    const float* __restrict__ origin, float voxel, int64_t* __restrict__ score, int tiles, long first_group) {
  __shared__ uint32_t wave_sum[kScoreThreads / 64][kTile];
  const long group = first_group + blockIdx.x;
  const long m = group / tiles;
  const int j0 = (int)(group % tiles) * kTile;
  const float* Rm = R + m * 9;
  const float* bm = base + m * 3;
  const float r00 = Rm[0], r01 = Rm[1], r02 = Rm[2], r10 = Rm[3], r11 = Rm[4], r12 = Rm[5], r20 = Rm[6], r21 = Rm[7],
              r22 = Rm[8];
  const float b0 = bm[0], b1 = bm[1], b2 = bm[2];
  const float o0 = origin[0], o1 = origin[1], o2 = origin[2];
  const float fx = (float)nx, fy = (float)ny, fz = (float)nz;   // (exact: at most 1024)
  float off[kTile][3];
#pragma unroll
  for (int k = 0; k < kTile; ++k) {
    const int j = j0 + k < n_off ? j0 + k : n_off - 1;
    off[k][0] = offsets[(long)j * 3];
    off[k][1] = offsets[(long)j * 3 + 1];
    off[k][2] = offsets[(long)j * 3 + 2];
  }
  uint32_t acc[kTile];
#pragma unroll
  for (int k = 0; k < kTile; ++k) acc[k] = 0u;
  for (int i = threadIdx.x; i < n_points; i += kScoreThreads) {
    const float p0 = points[(long)i * 3], p1 = points[(long)i * 3 + 1], p2 = points[(long)i * 3 + 2];
    const float q0 = ((r00 * p0 + r01 * p1) + r02 * p2) + b0;
    const float q1 = ((r10 * p0 + r11 * p1) + r12 * p2) + b1;
    const float q2 = ((r20 * p0 + r21 * p1) + r22 * p2) + b2;
    uint32_t v[kTile];
    bool in[kTile];
#pragma unroll
    for (int k = 0; k < kTile; ++k) {
      const float g0 = floorf(((q0 + off[k][0]) - o0) / voxel + 0.5f);
      const float g1 = floorf(((q1 + off[k][1]) - o1) / voxel + 0.5f);
      const float g2 = floorf(((q2 + off[k][2]) - o2) / voxel + 0.5f);
      const bool inside = (g0 >= 0.f) & (g0 < fx) & (g1 >= 0.f) & (g1 < fy) & (g2 >= 0.f) & (g2 < fz);   // (a NaN fails)
      // no branch: a point outside reads voxel (0,0,0), which exists, and drops the byte; the tile's loads go out together
      const int x = inside ? (int)g0 : 0, y = inside ? (int)g1 : 0, z = inside ? (int)g2 : 0;   // (converted only in range)
      v[k] = levels[((long)z * ny + y) * nx + x];
      in[k] = inside;
    }
#pragma unroll
    for (int k = 0; k < kTile; ++k) {
      const uint32_t q = in[k] ? v[k] : 255u;
      acc[k] += q * q;
    }
  }
#pragma unroll
  for (int k = 0; k < kTile; ++k) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc[k] += (uint32_t)__shfl_xor((int)acc[k], d, 64);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kTile; ++k) wave_sum[wave][k] = acc[k];
  }
  __syncthreads();
  if (threadIdx.x < kTile && j0 + (int)threadIdx.x < n_off) {
    uint32_t s = 0u;                                          // (the whole score fits: see kMaxScorePoints)
#pragma unroll
    for (int w = 0; w < kScoreThreads / 64; ++w) s += wave_sum[w][threadIdx.x];
    score[m * n_off + j0 + threadIdx.x] = (int64_t)s;
  }
}

}  // namespace
}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_pose_score_u8(const float* points, int n_points, const float* R, const float* base, int n_rot,
                      const float* offsets, int n_off, const uint8_t* levels, int nx, int ny, int nz, const float* origin,
                      float voxel, int64_t* score, int device, void* stream) {
  if (n_points < 0 || n_points > kMaxScorePoints) return CTD_ERR_INVALID_ARG;
  if (n_rot < 1 || n_off < 1 || n_off > kMaxOffsets || (double)n_rot * n_off >= 2147483648.0) return CTD_ERR_INVALID_ARG;
  if (nx < 1 || ny < 1 || nz < 1 || nx > kMaxDim || ny > kMaxDim || nz > kMaxDim) return CTD_ERR_INVALID_ARG;
  if (!positive_finite(voxel)) return CTD_ERR_INVALID_ARG;                               // a NaN fails the comparison
  if (!R || !base || !offsets || !levels || !origin || !score || (n_points > 0 && !points)) return CTD_ERR_INVALID_ARG;
  const Span sp[] = {{score, 8 * (size_t)n_rot * n_off}, {points, 12 * (size_t)n_points}, {R, 36 * (size_t)n_rot},
                     {base, 12 * (size_t)n_rot}, {offsets, 12 * (size_t)n_off}, {levels, (size_t)nx * ny * nz}, {origin, 12}};
  if (spans_overlap(sp, 1, 7)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const int tiles = ceil_div(n_off, kTile);
  const long groups = (long)n_rot * tiles;
  for (long first = 0; first < groups; first += kMaxGroups) {
    const long count = groups - first < kMaxGroups ? groups - first : kMaxGroups;
    pose_score_kernel<<<dim3((unsigned)count), dim3(kScoreThreads), 0, (hipStream_t)stream>>>(
        points, n_points, R, base, offsets, n_off, levels, nx, ny, nz, origin, voxel, score, tiles, first);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

}  // extern "C"
