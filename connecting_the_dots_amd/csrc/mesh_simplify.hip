// mesh_simplify.hip -- uniform-grid vertex clustering with quadric placement (ctd_mesh_simplify_f32; the rule is stated
// word for word in include/ctd_hip_mesh_simplify.h).
//
// The workgroup prefixes and fuse_scan_kernel are those of ctd_compact.h, the row sorts those of ctd_row_sort.h.  A
// workgroup takes 256 consecutive faces or vertices.  A cluster is known by its leader L, its smallest vertex: what
// belongs to a cluster (its counter, its row of members, its position, its output number) lies at index L of an array
// over the vertices, so nothing depends on where the cluster's key landed in the table.
//   sp_init_kernel     -- grid stride: both tables empty, the per-vertex flags and counters 0, the call's counts 0.
//   sp_used_kernel     -- thread = face (12 B read): used[v] = 1 at the corners of a valid face (plain stores of one value).
//   sp_insert_kernel   -- thread = vertex (12 B read): the cell; a clusterable vertex finds or takes the slot of its key
//     (a relaxed load first, a 64-bit compare-and-swap where the slot looked empty), then an integer min on the slot's
//     leader.  used[v] becomes `clusterable`.
//   sp_leader_kernel   -- thread = vertex: its leader (-1: unclusterable), one integer atomic add at the leader's counter;
//     the workgroup's number of leaders, one 64-bit add.
//   sp_sums_kernel     -- thread = vertex: the workgroup's sum of the counters and their maximum (one 64-bit max).
//   fuse_scan_kernel   -- ONE workgroup: the offsets of the workgroups' rows.
//   sp_offsets_kernel  -- thread = vertex: row starts (the row of a vertex that leads nothing is empty).
//   sp_fill_kernel     -- thread = vertex: a slot of the leader's row drawn from its counter (counting down to 0).
//   sp_rows_kernel     -- thread = vertex: a row of <= 16 members ascending (one lane, in LDS); the leaders of the longer
//     rows to a list (a range per workgroup by one integer atomic; the list's order reaches no output).
//   sp_long_rows_kernel -- workgroups stride over the list: a row ascending (up to 4096 members over a copy in LDS, more in
//     global memory).  A kernel of its own: long rows come in runs of neighbouring leaders, which their own workgroups
//     took one after the other while the rest idled (measured: 6.3 ms of a 12 ms call at 987 K faces).
//   sp_quadric_kernel  -- thread = vertex: Q_v, 9 f64, component k of vertex v at k * n_verts + v.
//   sp_place_kernel    -- thread = vertex (the leaders of <= 16 members work): the cluster's quadric and mean over its
//     sorted row, the solve, the fall-back; 12 B and a flag at the leader.
//   sp_long_place_kernel -- workgroups stride over the list: 256 members staged in LDS at a time, 12 threads add them in
//     the row's order; then the same solve.
//   sp_faces_kernel    -- thread = face: dropped, collapsed or candidate; the three leaders of a candidate.
//   sp_dedupe_kernel   -- thread = candidate face: finds or takes the slot of its sorted triple (compare-and-swap on an
//     empty slot, integer min on an equal one; the triples are those sp_faces_kernel wrote, a launch earlier).
//   sp_keep_kernel     -- thread = face: kept when its slot holds its own index; emit[L] = 1 at its leaders; the
//     workgroup's number of kept faces.
//   sp_emit_count_kernel -- thread = vertex: the workgroup's number of emitted clusters; the fall-backs among them.
//   sp_emit_verts_kernel -- thread = vertex: the output number of an emitted leader; verts_out and leader below the capacity.
//   sp_vert_cluster_kernel -- thread = vertex: vert_cluster.
//   sp_emit_faces_kernel -- thread = face: faces_out and face_index below the capacity.
// Atomics are integer compare-and-swap, min, max, add and subtract; no flag that another workgroup waits on: the same
// bits on every run.
#include "../../include/ctd_hip_mesh_simplify.h"
#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_row_sort.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kLaneRow = 16;                                  // members of a row that one lane sorts
constexpr u64 kNoKey = ~0ull;
constexpr u32 kNoFace = 0xffffffffu;
constexpr int kNoLeader = 2147483647;
constexpr unsigned kInitBlocks = 4096;                        // of the grid-stride sp_init_kernel, at most
constexpr unsigned kLongBlocks = 2048;                        // of the two kernels that stride over the long rows, at most

enum { kDropped = 0, kCollapsed = 1, kCandidate = 2, kKept = 3 };

__device__ inline bool face_valid(int a, int b, int c, long n_verts) {
  return (unsigned long)a < (unsigned long)n_verts && (unsigned long)b < (unsigned long)n_verts &&
         (unsigned long)c < (unsigned long)n_verts && a != b && a != c && b != c;
}

__device__ inline u64 mix64(u64 x) {                          // (any mixing does: no output depends on it)
  x ^= x >> 33;
  x *= 0xff51afd7ed558ccdull;
  x ^= x >> 33;
  x *= 0xc4ceb9fe1a85ec53ull;
  x ^= x >> 33;
  return x;
}

// the cell of a position: false when a coordinate's cell is not finite or outside [0, 2^20)
__device__ inline bool cell_of(const float* p, float ox, float oy, float oz, float cell, int* i) {
  const float t0 = floorf((p[0] - ox) / cell), t1 = floorf((p[1] - oy) / cell), t2 = floorf((p[2] - oz) / cell);
  const float top = (float)CTD_MESH_SIMPLIFY_MAX_CELLS_PER_AXIS;
  if (!(t0 >= 0.f && t0 < top && t1 >= 0.f && t1 < top && t2 >= 0.f && t2 < top)) return false;   // (a NaN fails)
  i[0] = (int)t0;
  i[1] = (int)t1;
  i[2] = (int)t2;
  return true;
}

struct Arrays {                                               // the workspace, as pointers
  int *used, *vleader, *ccount, *coff, *members, *emit, *cout, *cfall, *tleader, *ftri, *wg_cnt, *wg_emit, *wg_faces;
  int *long_list, *n_long_rows;
  u32 *vslot, *fslot, *dslots;
  float* cpos;
  double* quad;
  u64* tkeys;
  uint8_t* fstate;
};

__global__ __launch_bounds__(kChunk) void sp_init_kernel(Arrays a, int64_t* __restrict__ counts, long n_verts, u64 table,
                                                         u64 table_faces) {
  const u64 first = (u64)blockIdx.x * kChunk + threadIdx.x, step = (u64)gridDim.x * kChunk;
  for (u64 i = first; i < table; i += step) {
    a.tkeys[i] = kNoKey;
    a.tleader[i] = kNoLeader;
  }
  for (u64 i = first; i < table_faces; i += step) a.dslots[i] = kNoFace;
  for (u64 i = first; i < (u64)n_verts; i += step) {
    a.used[i] = 0;
    a.ccount[i] = 0;
    a.emit[i] = 0;
  }
  if (first < 8) counts[first] = 0;
  if (first == 0) *a.n_long_rows = 0;
}

__global__ __launch_bounds__(kChunk) void sp_used_kernel(const int32_t* __restrict__ faces, int* used, long n_verts, long n_faces) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!face_valid(a, b, c, n_verts)) return;
  used[a] = 1;
  used[b] = 1;
  used[c] = 1;
}

__global__ __launch_bounds__(kChunk) void sp_insert_kernel(const float* __restrict__ verts, int* __restrict__ used, u64* tkeys,
                                                           int* tleader, u32* __restrict__ vslot, long n_verts, u64 mask,
                                                           float ox, float oy, float oz, float cell) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v >= n_verts) return;
  int i[3];
  const bool ok = used[v] != 0 && cell_of(verts + 3 * v, ox, oy, oz, cell, i);
  used[v] = ok ? 1 : 0;                                       // from here on: clusterable
  if (!ok) return;
  const u64 key = ((u64)i[0] << 40) | ((u64)i[1] << 20) | (u64)i[2];
  u64 h = mix64(key) & mask;
  for (;;) {                                                  // the table has twice as many slots as there are vertices
    u64 cur = __hip_atomic_load(tkeys + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kNoKey) cur = atomicCAS(tkeys + h, kNoKey, key);   // (a stale load can only cost an atomic)
    if (cur == kNoKey || cur == key) break;
    h = (h + 1) & mask;
  }
  if ((int)v < __hip_atomic_load(tleader + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(tleader + h, (int)v);
  vslot[v] = (u32)h;                                          // (a stale load can only cost an atomic, as above)
}

__global__ __launch_bounds__(kChunk) void sp_leader_kernel(const int* __restrict__ used, const u32* __restrict__ vslot,
                                                           const int* __restrict__ tleader, int* __restrict__ vleader,
                                                           int* ccount, int64_t* counts, long n_verts) {
  __shared__ int wave_n[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  int L = -1;
  if (v < n_verts) {
    if (used[v]) {
      L = tleader[vslot[v]];
      atomicAdd(ccount + L, 1);
    }
    vleader[v] = L;
  }
  int total;
  (void)wg_flags_before<kChunk>(v < n_verts && L == (int)v, wave_n, total);
  if (threadIdx.x == 0 && total) atomicAdd((u64*)(counts + 2), (u64)total);
}

__device__ inline int wave_max(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int other = __shfl_xor(v, d);
    v = other > v ? other : v;
  }
  return v;
}

__global__ __launch_bounds__(kChunk) void sp_sums_kernel(const int* __restrict__ ccount, int* __restrict__ wg_cnt, int64_t* counts,
                                                         long n_verts) {
  __shared__ int wave_n[kChunk / 64], wave_m[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  const int n = v < n_verts ? ccount[v] : 0;
  const int top = wave_max(n);
  if ((threadIdx.x & 63) == 0) wave_m[threadIdx.x >> 6] = top;
  int total;
  (void)wg_exclusive_sum<kChunk>(n, wave_n, total);          // (its barrier covers wave_m)
  if (threadIdx.x == 0) {
    wg_cnt[blockIdx.x] = total;
    int most = wave_m[0];
#pragma unroll
    for (int w = 1; w < kChunk / 64; ++w) most = wave_m[w] > most ? wave_m[w] : most;
    if (most) atomicMax((u64*)(counts + 7), (u64)most);
  }
}

// (launched with one workgroup at least: coff[n_verts] is written at n_verts == 0 too)
__global__ __launch_bounds__(kChunk) void sp_offsets_kernel(const int* __restrict__ ccount, const int* __restrict__ wg_off,
                                                            int* __restrict__ coff, long n_verts) {
  __shared__ int wave_n[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  int total;
  const int o = wg_off[blockIdx.x] + wg_exclusive_sum<kChunk>(v < n_verts ? ccount[v] : 0, wave_n, total);
  if (v <= n_verts) coff[v] = o;
}

__global__ __launch_bounds__(kChunk) void sp_fill_kernel(const int* __restrict__ vleader, int* ccount, const int* __restrict__ coff,
                                                         int* __restrict__ members, long n_verts) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v >= n_verts) return;
  const int L = vleader[v];
  if (L < 0) return;
  members[(long)coff[L] + (atomicSub(ccount + L, 1) - 1)] = (int)v;
}

// Short rows by their lanes; the leaders of the longer rows go to long_list, a range of it per workgroup drawn from
// n_long_rows by one integer atomic (the order of the list does not reach any output): long rows come in runs of
// neighbouring leaders, which their own workgroups would take one after the other while the others idle.
__global__ __launch_bounds__(kChunk) void sp_rows_kernel(const int* __restrict__ coff, int* members, int* __restrict__ long_list,
                                                         int* n_long_rows, long n_verts) {
  __shared__ int col[kLaneRow * kChunk];
  __shared__ int wave_n[kChunk / 64];
  __shared__ int first;
  const int tid = threadIdx.x;
  const long v = (long)blockIdx.x * kChunk + tid;
  bool is_long = false;
  if (v < n_verts) {
    const long r0 = coff[v];
    const int n = coff[v + 1] - (int)r0;
    is_long = n > kLaneRow;
    if (!is_long && n > 1) {
      int* mine = col + tid;
      for (int k = 0; k < n; ++k) mine[k * kChunk] = members[r0 + k];
      lane_sort(mine, n);
      for (int k = 0; k < n; ++k) members[r0 + k] = mine[k * kChunk];
    }
  }
  int total;
  const int before = wg_flags_before<kChunk>(is_long, wave_n, total);
  if (tid == 0 && total) first = atomicAdd(n_long_rows, total);
  __syncthreads();
  if (is_long) long_list[first + before] = (int)v;
}

// the workgroup: the long rows of the list, kLongBlocks workgroups striding over it; a row of up to 4096 members over a
// copy in LDS, a longer one in global memory
__global__ __launch_bounds__(kChunk) void sp_long_rows_kernel(const int* __restrict__ coff, int* members,
                                                              const int* __restrict__ long_list,
                                                              const int* __restrict__ n_long_rows) {
  __shared__ int col[kLaneRow * kChunk];
  const int tid = threadIdx.x, todo = *n_long_rows;           // uniform
  for (int q = blockIdx.x; q < todo; q += gridDim.x) {
    const long i = long_list[q];
    const long r0 = coff[i];
    const int n = coff[i + 1] - (int)r0;
    int* row = members + r0;
    if (n <= kLaneRow * kChunk) {                             // uniform
      for (int k = tid; k < n; k += kChunk) col[k] = row[k];
      __syncthreads();
      wg_sort(col, n);                                        // (ends with a barrier)
      for (int k = tid; k < n; k += kChunk) row[k] = col[k];
      __syncthreads();
    } else {
      wg_sort(row, n);
    }
  }
}

__global__ __launch_bounds__(kChunk) void sp_quadric_kernel(const float* __restrict__ verts, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ face_offsets,
                                                            const int32_t* __restrict__ face_ids, const int* __restrict__ used,
                                                            double* __restrict__ quad, long n_verts, long n_faces,
                                                            long n_incident, float ox, float oy, float oz) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v >= n_verts || !used[v]) return;
  const double dox = (double)ox, doy = (double)oy, doz = (double)oz;
  double a00 = 0., a01 = 0., a02 = 0., a11 = 0., a12 = 0., a22 = 0., b0 = 0., b1 = 0., b2 = 0.;
  const long k0 = face_offsets[v], k1 = face_offsets[v + 1];
  if (k0 >= 0 && k0 <= k1 && k1 <= n_incident) {
    for (long k = k0; k < k1; ++k) {
      const int f = face_ids[k];
      if ((unsigned long)f >= (unsigned long)n_faces) continue;
      const int a = faces[3l * f], b = faces[3l * f + 1], c = faces[3l * f + 2];
      if (!face_valid(a, b, c, n_verts)) continue;            // nothing is dereferenced before this holds
      if (!used[a] || !used[b] || !used[c]) continue;
      const float* p0 = verts + 3l * a;
      const float* p1 = verts + 3l * b;
      const float* p2 = verts + 3l * c;
      const double q0x = (double)p0[0] - dox, q0y = (double)p0[1] - doy, q0z = (double)p0[2] - doz;
      const double q1x = (double)p1[0] - dox, q1y = (double)p1[1] - doy, q1z = (double)p1[2] - doz;
      const double q2x = (double)p2[0] - dox, q2y = (double)p2[1] - doy, q2z = (double)p2[2] - doz;
      const double e1x = q1x - q0x, e1y = q1y - q0y, e1z = q1z - q0z;
      const double e2x = q2x - q0x, e2y = q2y - q0y, e2z = q2z - q0z;
      const double cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
      const double d = -((cx * q0x + cy * q0y) + cz * q0z);
      a00 += cx * cx;
      a01 += cx * cy;
      a02 += cx * cz;
      a11 += cy * cy;
      a12 += cy * cz;
      a22 += cz * cz;
      b0 += d * cx;
      b1 += d * cy;
      b2 += d * cz;
    }
  }
  const double q[9] = {a00, a01, a02, a11, a12, a22, b0, b1, b2};
#pragma unroll
  for (int k = 0; k < 9; ++k) quad[k * n_verts + v] = q[k];
}

__device__ inline bool finite64(double x) { return x - x == 0.; }   // (false for a NaN and for an infinity)

// the placement of the cluster led by v from its summed quadric A (A00 A01 A02 A11 A12 A22 b0 b1 b2), the sum s of its
// members' q and their number: 12 B to cpos and the fall-back flag, at v
__device__ inline void place_cluster(const double* A, const double* s, long members, long v, const float* __restrict__ verts,
                                     float* __restrict__ cpos, int* __restrict__ cfall, float ox, float oy, float oz, float cell,
                                     double reg) {
  const double org[3] = {(double)ox, (double)oy, (double)oz};
  const double count = (double)members;
  const double mean[3] = {s[0] / count, s[1] / count, s[2] / count};
  const double a00 = A[0], a01 = A[1], a02 = A[2], a11 = A[3], a12 = A[4], a22 = A[5];
  const double lambda = reg * ((a00 + a11) + a22);
  const double t0 = -(((a00 * mean[0] + a01 * mean[1]) + a02 * mean[2]) + A[6]);
  const double t1 = -(((a01 * mean[0] + a11 * mean[1]) + a12 * mean[2]) + A[7]);
  const double t2 = -(((a02 * mean[0] + a12 * mean[1]) + a22 * mean[2]) + A[8]);
  const double m00 = a00 + lambda, m11 = a11 + lambda, m22 = a22 + lambda, m01 = a01, m02 = a02, m12 = a12;
  const double c00 = m11 * m22 - m12 * m12, c01 = m02 * m12 - m01 * m22, c02 = m01 * m12 - m02 * m11;
  const double c11 = m00 * m22 - m02 * m02, c12 = m01 * m02 - m00 * m12, c22 = m00 * m11 - m01 * m01;
  const double det = (m00 * c00 + m01 * c01) + m02 * c02;
  double x[3] = {mean[0] + ((c00 * t0 + c01 * t1) + c02 * t2) / det, mean[1] + ((c01 * t0 + c11 * t1) + c12 * t2) / det,
                 mean[2] + ((c02 * t0 + c12 * t1) + c22 * t2) / det};
  int idx[3] = {0, 0, 0};
  (void)cell_of(verts + 3 * v, ox, oy, oz, cell, idx);        // (the leader is clusterable: this is the cluster's cell)
  const double dc = (double)cell;
  bool fall = !(finite64(lambda) && lambda > 0.) || !(finite64(det) && det > 0.);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double lo = (double)idx[k] * dc;
    fall = fall || !finite64(x[k]) || !(x[k] >= lo - dc * 0.5 && x[k] <= lo + dc * 1.5);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) cpos[3 * v + k] = (float)((fall ? mean[k] : x[k]) + org[k]);
  cfall[v] = fall ? 1 : 0;
}

constexpr int kStageRow = kChunk + 1;                         // f64 entries between two components in LDS: no bank is shared

// the clusters of at most kLaneRow members: the leader's lane sums the row and solves
__global__ __launch_bounds__(kChunk) void sp_place_kernel(const float* __restrict__ verts, const int* __restrict__ vleader,
                                                          const int* __restrict__ coff, const int* __restrict__ members,
                                                          const double* __restrict__ quad, float* __restrict__ cpos,
                                                          int* __restrict__ cfall, long n_verts, float ox, float oy, float oz,
                                                          float cell, double reg) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v >= n_verts || vleader[v] != (int)v) return;
  const long r0 = coff[v], r1 = coff[v + 1];
  if (r1 - r0 > kLaneRow) return;
  const double org[3] = {(double)ox, (double)oy, (double)oz};
  double A[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.}, s[3] = {0., 0., 0.};
  for (long r = r0; r < r1; ++r) {
    const long j = members[r];
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] += quad[k * n_verts + j];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] += (double)verts[3 * j + k] - org[k];
  }
  place_cluster(A, s, r1 - r0, v, verts, cpos, cfall, ox, oy, oz, cell, reg);
}

// The longer clusters, kLongBlocks workgroups striding over long_list, 256 members at a time: every thread stages the 12
// summands of one member in LDS (the loads of a chunk are in flight together), then 12 threads add them in the row's
// order, one component each, so the association is the rule's; thread 0 solves.
__global__ __launch_bounds__(kChunk) void sp_long_place_kernel(const float* __restrict__ verts, const int* __restrict__ coff,
                                                               const int* __restrict__ members, const double* __restrict__ quad,
                                                               const int* __restrict__ long_list,
                                                               const int* __restrict__ n_long_rows, float* __restrict__ cpos,
                                                               int* __restrict__ cfall, long n_verts, float ox, float oy,
                                                               float oz, float cell, double reg) {
  __shared__ double stage[12 * kStageRow];
  __shared__ double sums[12];
  const int tid = threadIdx.x, todo = *n_long_rows;           // uniform
  const double org[3] = {(double)ox, (double)oy, (double)oz};
  for (int q = blockIdx.x; q < todo; q += gridDim.x) {
    const long i = long_list[q];
    const long r0 = coff[i], r1 = coff[i + 1];
    if (tid < 12) sums[tid] = 0.;
    for (long base = r0; base < r1; base += kChunk) {         // uniform
      const long r = base + tid;
      if (r < r1) {
        const long j = members[r];
#pragma unroll
        for (int k = 0; k < 9; ++k) stage[k * kStageRow + tid] = quad[k * n_verts + j];
#pragma unroll
        for (int k = 0; k < 3; ++k) stage[(9 + k) * kStageRow + tid] = (double)verts[3 * j + k] - org[k];
      }
      __syncthreads();
      if (tid < 12) {
        const int staged = r1 - base < kChunk ? (int)(r1 - base) : kChunk;
        double acc = sums[tid];
        for (int t = 0; t < staged; ++t) acc += stage[tid * kStageRow + t];
        sums[tid] = acc;
      }
      __syncthreads();
    }
    if (tid == 0) place_cluster(sums, sums + 9, r1 - r0, i, verts, cpos, cfall, ox, oy, oz, cell, reg);
    __syncthreads();                                          // sums is free again
  }
}

__device__ inline void sort3(int& a, int& b, int& c) {
  int t;
  if (a > b) { t = a; a = b; b = t; }
  if (b > c) { t = b; b = c; c = t; }
  if (a > b) { t = a; a = b; b = t; }
}

__global__ __launch_bounds__(kChunk) void sp_faces_kernel(const int32_t* __restrict__ faces, const int* __restrict__ vleader,
                                                          int* __restrict__ ftri, uint8_t* __restrict__ fstate, int64_t* counts,
                                                          long n_verts, long n_faces) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  int state = -1;                                             // past the end
  if (f < n_faces) {
    const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    state = kDropped;
    if (face_valid(a, b, c, n_verts)) {
      const int la = vleader[a], lb = vleader[b], lc = vleader[c];
      if (la >= 0 && lb >= 0 && lc >= 0) {
        state = (la == lb || la == lc || lb == lc) ? kCollapsed : kCandidate;
        ftri[3 * f] = la;
        ftri[3 * f + 1] = lb;
        ftri[3 * f + 2] = lc;
      }
    }
    fstate[f] = (uint8_t)state;
  }
  __shared__ int wave_n[kChunk / 64];
  int dropped, collapsed;
  (void)wg_flags_before<kChunk>(state == kDropped, wave_n, dropped);
  __syncthreads();
  (void)wg_flags_before<kChunk>(state == kCollapsed, wave_n, collapsed);
  if (threadIdx.x == 0) {
    if (dropped) atomicAdd((u64*)(counts + 3), (u64)dropped);
    if (collapsed) atomicAdd((u64*)(counts + 4), (u64)collapsed);
  }
}

__global__ __launch_bounds__(kChunk) void sp_dedupe_kernel(const int* __restrict__ ftri, const uint8_t* __restrict__ fstate,
                                                           u32* dslots, u32* __restrict__ fslot, long n_faces, u64 mask) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  if (f >= n_faces || fstate[f] != kCandidate) return;
  int a = ftri[3 * f], b = ftri[3 * f + 1], c = ftri[3 * f + 2];
  sort3(a, b, c);
  u64 h = mix64(mix64(((u64)(u32)a << 32) | (u32)b) ^ (u64)(u32)c) & mask;
  for (;;) {                                                  // the table has twice as many slots as there are faces
    u32 cur = __hip_atomic_load(dslots + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (cur == kNoFace) {
      cur = atomicCAS(dslots + h, kNoFace, (u32)f);
      if (cur == kNoFace) break;                              // the slot is this triple's from now on
    }
    int x = ftri[3l * cur], y = ftri[3l * cur + 1], z = ftri[3l * cur + 2];   // (cur is a candidate: written a launch earlier)
    sort3(x, y, z);
    if (x == a && y == b && z == c) {
      atomicMin(dslots + h, (u32)f);
      break;
    }
    h = (h + 1) & mask;
  }
  fslot[f] = (u32)h;
}

__global__ __launch_bounds__(kChunk) void sp_keep_kernel(const int* __restrict__ ftri, uint8_t* __restrict__ fstate,
                                                         const u32* __restrict__ dslots, const u32* __restrict__ fslot,
                                                         int* emit, int* __restrict__ wg_faces, int64_t* counts, long n_faces,
                                                         int drop_duplicates) {
  __shared__ int wave_n[kChunk / 64];
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  bool kept = false, duplicate = false;
  if (f < n_faces && fstate[f] == kCandidate) {
    kept = !drop_duplicates || dslots[fslot[f]] == (u32)f;
    duplicate = !kept;
    if (kept) {
      fstate[f] = kKept;
      emit[ftri[3 * f]] = 1;
      emit[ftri[3 * f + 1]] = 1;
      emit[ftri[3 * f + 2]] = 1;
    }
  }
  int total, dups;
  (void)wg_flags_before<kChunk>(kept, wave_n, total);
  __syncthreads();
  (void)wg_flags_before<kChunk>(duplicate, wave_n, dups);
  if (threadIdx.x == 0) {
    wg_faces[blockIdx.x] = total;
    if (dups) atomicAdd((u64*)(counts + 5), (u64)dups);
  }
}

__global__ __launch_bounds__(kChunk) void sp_emit_count_kernel(const int* __restrict__ emit, const int* __restrict__ cfall,
                                                               int* __restrict__ wg_emit, int64_t* counts, long n_verts) {
  __shared__ int wave_n[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  const bool out = v < n_verts && emit[v] != 0;
  int total, falls;
  (void)wg_flags_before<kChunk>(out, wave_n, total);
  __syncthreads();
  (void)wg_flags_before<kChunk>(out && cfall[v] != 0, wave_n, falls);
  if (threadIdx.x == 0) {
    wg_emit[blockIdx.x] = total;
    if (falls) atomicAdd((u64*)(counts + 6), (u64)falls);
  }
}

__global__ __launch_bounds__(kChunk) void sp_emit_verts_kernel(const int* __restrict__ emit, const int* __restrict__ wg_off,
                                                               const float* __restrict__ cpos, int* __restrict__ cout,
                                                               float* __restrict__ verts_out, int32_t* __restrict__ leader,
                                                               long cap, long n_verts) {
  __shared__ int wave_n[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  const bool out = v < n_verts && emit[v] != 0;
  int total;
  const long at = (long)wg_off[blockIdx.x] + wg_flags_before<kChunk>(out, wave_n, total);
  if (!out) return;
  cout[v] = (int)at;
  if (at < cap) {
    verts_out[3 * at] = cpos[3 * v];
    verts_out[3 * at + 1] = cpos[3 * v + 1];
    verts_out[3 * at + 2] = cpos[3 * v + 2];
    leader[at] = (int32_t)v;
  }
}

__global__ __launch_bounds__(kChunk) void sp_vert_cluster_kernel(const int* __restrict__ vleader, const int* __restrict__ emit,
                                                                 const int* __restrict__ cout, int32_t* __restrict__ vert_cluster,
                                                                 long n_verts) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v >= n_verts) return;
  const int L = vleader[v];
  vert_cluster[v] = (L >= 0 && emit[L]) ? cout[L] : -1;
}

__global__ __launch_bounds__(kChunk) void sp_emit_faces_kernel(const int* __restrict__ ftri, const uint8_t* __restrict__ fstate,
                                                               const int* __restrict__ wg_off, const int* __restrict__ cout,
                                                               int32_t* __restrict__ faces_out, int32_t* __restrict__ face_index,
                                                               long cap, long n_faces) {
  __shared__ int wave_n[kChunk / 64];
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  const bool kept = f < n_faces && fstate[f] == kKept;
  int total;
  const long at = (long)wg_off[blockIdx.x] + wg_flags_before<kChunk>(kept, wave_n, total);
  if (!kept || at >= cap) return;
  faces_out[3 * at] = cout[ftri[3 * f]];
  faces_out[3 * at + 1] = cout[ftri[3 * f + 1]];
  faces_out[3 * at + 2] = cout[ftri[3 * f + 2]];
  face_index[at] = (int32_t)f;
}

// the smallest power of two >= max(2 * n, 256)
inline u64 table_slots(int64_t n) {
  u64 t = 256;
  while (t < 2 * (u64)n) t <<= 1;
  return t;
}

struct Layout {                                               // byte offsets into the workspace
  size_t used, vslot, vleader, ccount, coff, members, emit, cout, cfall, cpos, quad, tkeys, tleader, ftri, fstate, fslot, dslots,
      wg_cnt, wg_emit, wg_faces, long_list, n_long_rows, bytes;
};
Layout layout(int64_t n_verts, int64_t n_faces) {
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  const size_t t = (size_t)table_slots(n_verts), tf = (size_t)table_slots(n_faces);
  WorkspaceCursor c;
  Layout l;
  l.used = c.take(4 * n);
  l.vslot = c.take(4 * n);
  l.vleader = c.take(4 * n);
  l.ccount = c.take(4 * n);
  l.coff = c.take(4 * (n + 1));
  l.members = c.take(4 * n);
  l.emit = c.take(4 * n);
  l.cout = c.take(4 * n);
  l.cfall = c.take(4 * n);
  l.cpos = c.take(12 * n);
  l.quad = c.take(72 * n);
  l.tkeys = c.take(8 * t);
  l.tleader = c.take(4 * t);
  l.ftri = c.take(12 * m);
  l.fstate = c.take(m);
  l.fslot = c.take(4 * m);
  l.dslots = c.take(4 * tf);
  l.wg_cnt = c.take_counts((size_t)chunks_of(n_verts));
  l.wg_emit = c.take_counts((size_t)chunks_of(n_verts));
  l.wg_faces = c.take_counts((size_t)chunks_of(n_faces));
  l.long_list = c.take(4 * n);
  l.n_long_rows = c.take(4);
  l.bytes = c.bytes;
  return l;
}

constexpr int64_t kInt32End = 2147483648l;                    // 2^31

// INVALID_ARG, UNSUPPORTED or OK for the sizes alone
int size_status(int64_t n_verts, int64_t n_faces, int64_t n_incident) {
  if (n_verts < 0 || n_faces < 0 || n_incident < 0) return CTD_ERR_INVALID_ARG;
  if (n_faces > (kInt32End - 1) / 6 || n_verts >= kInt32End || n_incident >= kInt32End) return CTD_ERR_UNSUPPORTED;
  if (!launch_ok((double)chunks_of(n_faces)) || !launch_ok((double)chunks_of(n_verts))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)chunks_of(n); }

inline bool finite32(float v) { return v - v == 0.f; }

}  // namespace

static int mesh_simplify_f32(const float* verts, long n, const int32_t* faces, long m, const int32_t* face_offsets,
                             const int32_t* face_ids, long n_incident, float ox, float oy, float oz, float cell, double reg,
                             int drop_duplicates, float* verts_out, int32_t* leader, long cap_verts, int32_t* vert_cluster,
                             int32_t* faces_out, int32_t* face_index, long cap_faces, int64_t* counts, void* workspace,
                             hipStream_t stream) {
  const Layout l = layout(n, m);
  char* ws = (char*)workspace;
  Arrays a;
  a.used = (int*)(ws + l.used);
  a.vslot = (u32*)(ws + l.vslot);
  a.vleader = (int*)(ws + l.vleader);
  a.ccount = (int*)(ws + l.ccount);
  a.coff = (int*)(ws + l.coff);
  a.members = (int*)(ws + l.members);
  a.emit = (int*)(ws + l.emit);
  a.cout = (int*)(ws + l.cout);
  a.cfall = (int*)(ws + l.cfall);
  a.cpos = (float*)(ws + l.cpos);
  a.quad = (double*)(ws + l.quad);
  a.tkeys = (u64*)(ws + l.tkeys);
  a.tleader = (int*)(ws + l.tleader);
  a.ftri = (int*)(ws + l.ftri);
  a.fstate = (uint8_t*)(ws + l.fstate);
  a.fslot = (u32*)(ws + l.fslot);
  a.dslots = (u32*)(ws + l.dslots);
  a.wg_cnt = (int*)(ws + l.wg_cnt);
  a.wg_emit = (int*)(ws + l.wg_emit);
  a.wg_faces = (int*)(ws + l.wg_faces);
  a.long_list = (int*)(ws + l.long_list);
  a.n_long_rows = (int*)(ws + l.n_long_rows);
  const u64 table = table_slots(n), table_faces = table_slots(m);
  const unsigned vb = blocks_of(n), fb = blocks_of(m), vb1 = blocks_of(n + 1);
  const dim3 wg(kChunk);
  const u64 most = table > table_faces ? table : table_faces;   // (both exceed n and m)
  const u64 init_blocks = (most + kChunk - 1) / kChunk;
  sp_init_kernel<<<dim3(init_blocks < kInitBlocks ? (unsigned)init_blocks : kInitBlocks), wg, 0, stream>>>(a, counts, n, table,
                                                                                                            table_faces);
  CTD_LAUNCH_CHECK();
  if (vb && fb) {
    sp_used_kernel<<<dim3(fb), wg, 0, stream>>>(faces, a.used, n, m);
    CTD_LAUNCH_CHECK();
  }
  if (vb) {
    sp_insert_kernel<<<dim3(vb), wg, 0, stream>>>(verts, a.used, a.tkeys, a.tleader, a.vslot, n, table - 1, ox, oy, oz, cell);
    CTD_LAUNCH_CHECK();
    sp_leader_kernel<<<dim3(vb), wg, 0, stream>>>(a.used, a.vslot, a.tleader, a.vleader, a.ccount, counts, n);
    CTD_LAUNCH_CHECK();
    sp_sums_kernel<<<dim3(vb), wg, 0, stream>>>(a.ccount, a.wg_cnt, counts, n);
    CTD_LAUNCH_CHECK();
  }
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(a.wg_cnt, (int)vb, (int)vb, nullptr, 0);
  CTD_LAUNCH_CHECK();
  sp_offsets_kernel<<<dim3(vb1), wg, 0, stream>>>(a.ccount, a.wg_cnt, a.coff, n);
  CTD_LAUNCH_CHECK();
  if (vb) {
    sp_fill_kernel<<<dim3(vb), wg, 0, stream>>>(a.vleader, a.ccount, a.coff, a.members, n);
    CTD_LAUNCH_CHECK();
    const unsigned lb = vb < kLongBlocks ? vb : kLongBlocks;
    sp_rows_kernel<<<dim3(vb), wg, 0, stream>>>(a.coff, a.members, a.long_list, a.n_long_rows, n);
    CTD_LAUNCH_CHECK();
    sp_long_rows_kernel<<<dim3(lb), wg, 0, stream>>>(a.coff, a.members, a.long_list, a.n_long_rows);
    CTD_LAUNCH_CHECK();
    sp_quadric_kernel<<<dim3(vb), wg, 0, stream>>>(verts, faces, face_offsets, face_ids, a.used, a.quad, n, m, n_incident, ox, oy,
                                                  oz);
    CTD_LAUNCH_CHECK();
    sp_place_kernel<<<dim3(vb), wg, 0, stream>>>(verts, a.vleader, a.coff, a.members, a.quad, a.cpos, a.cfall, n, ox, oy, oz, cell,
                                                reg);
    CTD_LAUNCH_CHECK();
    sp_long_place_kernel<<<dim3(lb), wg, 0, stream>>>(verts, a.coff, a.members, a.quad, a.long_list, a.n_long_rows, a.cpos,
                                                     a.cfall, n, ox, oy, oz, cell, reg);
    CTD_LAUNCH_CHECK();
  }
  if (fb) {
    sp_faces_kernel<<<dim3(fb), wg, 0, stream>>>(faces, a.vleader, a.ftri, a.fstate, counts, n, m);
    CTD_LAUNCH_CHECK();
    if (drop_duplicates) {
      sp_dedupe_kernel<<<dim3(fb), wg, 0, stream>>>(a.ftri, a.fstate, a.dslots, a.fslot, m, table_faces - 1);
      CTD_LAUNCH_CHECK();
    }
    sp_keep_kernel<<<dim3(fb), wg, 0, stream>>>(a.ftri, a.fstate, a.dslots, a.fslot, a.emit, a.wg_faces, counts, m, drop_duplicates);
    CTD_LAUNCH_CHECK();
  }
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(a.wg_faces, (int)fb, (int)fb, counts + 1, 1);
  CTD_LAUNCH_CHECK();
  if (vb) {
    sp_emit_count_kernel<<<dim3(vb), wg, 0, stream>>>(a.emit, a.cfall, a.wg_emit, counts, n);
    CTD_LAUNCH_CHECK();
  }
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(a.wg_emit, (int)vb, (int)vb, counts, 1);
  CTD_LAUNCH_CHECK();
  if (vb) {
    sp_emit_verts_kernel<<<dim3(vb), wg, 0, stream>>>(a.emit, a.wg_emit, a.cpos, a.cout, verts_out, leader, cap_verts, n);
    CTD_LAUNCH_CHECK();
    sp_vert_cluster_kernel<<<dim3(vb), wg, 0, stream>>>(a.vleader, a.emit, a.cout, vert_cluster, n);
    CTD_LAUNCH_CHECK();
  }
  if (fb && cap_faces > 0) {
    sp_emit_faces_kernel<<<dim3(fb), wg, 0, stream>>>(a.ftri, a.fstate, a.wg_faces, a.cout, faces_out, face_index, cap_faces, m);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces) {
  if (size_status(n_verts, n_faces, 0) != CTD_OK) return 0;
  return layout(n_verts, n_faces).bytes;
}

int ctd_mesh_simplify_f32(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                          const int32_t* face_offsets, const int32_t* face_ids, int64_t n_incident, float origin_x,
                          float origin_y, float origin_z, float cell, double reg, int drop_duplicates, float* verts_out,
                          int32_t* leader, int64_t cap_verts, int32_t* vert_cluster, int32_t* faces_out, int32_t* face_index,
                          int64_t cap_faces, int64_t* counts, void* workspace, size_t workspace_bytes, int device,
                          void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_incident < 0 || cap_verts < 0 || cap_faces < 0) return CTD_ERR_INVALID_ARG;
  if (!verts || !faces || !face_offsets || !face_ids || !verts_out || !leader || !vert_cluster || !faces_out || !face_index ||
      !counts)
    return CTD_ERR_INVALID_ARG;
  if (!finite32(origin_x) || !finite32(origin_y) || !finite32(origin_z) || !positive_finite(cell) ||
      !(reg >= 0. && reg < __builtin_inf()))
    return CTD_ERR_INVALID_ARG;
  const int st = size_status(n_verts, n_faces, n_incident);
  if (st != CTD_OK) return st;
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  const size_t cv = (size_t)cap_verts < n ? (size_t)cap_verts : n, cf = (size_t)cap_faces < m ? (size_t)cap_faces : m;
  const size_t need = ctd_mesh_simplify_workspace_bytes(n_verts, n_faces);
  const Span s[] = {{verts_out, 12 * cv},  {leader, 4 * cv},  {vert_cluster, 4 * n},        {faces_out, 12 * cf},
                    {face_index, 4 * cf},  {counts, 64},      {workspace, need},            {verts, 12 * n},
                    {faces, 12 * m},       {face_offsets, 4 * (n + 1)}, {face_ids, 4 * (size_t)n_incident}};
  if (spans_overlap(s, 7, 11)) return CTD_ERR_INVALID_ARG;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_simplify_f32(verts, (long)n_verts, faces, (long)n_faces, face_offsets, face_ids, (long)n_incident, origin_x,
                           origin_y, origin_z, cell, reg, drop_duplicates, verts_out, leader, (long)cap_verts, vert_cluster,
                           faces_out, face_index, (long)cap_faces, counts, workspace, (hipStream_t)stream);
}

}  // extern "C"
