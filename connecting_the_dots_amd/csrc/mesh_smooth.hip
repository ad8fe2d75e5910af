// mesh_smooth.hip -- the connectivity by vertex of an indexed triangle mesh, Taubin smoothing over the one-rings and
// area-weighted vertex normals (ctd_mesh_adjacency_i32, ctd_mesh_smooth_f32, ctd_mesh_vertex_normals_f32; the rule is
// stated word for word in include/ctd_hip_mesh_smooth.h).
//
// The workgroup prefix and fuse_scan_kernel are those of ctd_compact.h.  A workgroup takes 256 consecutive faces or
// vertices.  The rows of consecutive vertices lie one after the other: vertex v owns fid[foff[v] .. foff[v+1]) (its
// incident faces) and raw[2 * foff[v] .. 2 * foff[v+1]) (the two other corners of each of them).
//   ma_init_kernel    -- thread = vertex: its counter 0; the call's counts 0.  4 B written.
//   ma_count_kernel   -- thread = face (12 B read): the validity test, one integer atomic add at each vertex of a valid face.
//   ma_sums_kernel    -- thread = vertex (4 B read): the workgroup's sum and maximum of the counters.
//   ma_max_kernel     -- ONE workgroup: max_incident, the largest of the workgroups' maxima.
//   fuse_scan_kernel  -- ONE workgroup: the offsets of the workgroups' rows.
//   ma_face_offsets_kernel -- thread = vertex: foff (and face_offsets), 4 B read, 4 or 8 B written; the number of valid faces
//     is a third of the total.
//   ma_fill_kernel    -- thread = face (12 B read): per corner of a valid face a slot drawn from the vertex's counter
//     (integer atomic, counting down to 0), 4 B to fid and 8 B to raw there.  The order inside a row depends on the atomics.
//   ma_rows_kernel    -- thread = vertex, then the workgroup: sorts fid and raw of every row, which removes that order.  At
//     most kLaneRow incident faces: one lane, insertion sort in LDS (entry k of thread t at k * 256 + t: no bank is shared).
//     More: the 256 threads together, one such row after the other, a bitonic network of ascending comparators over the
//     row in global memory (any length; a comparator whose upper end lies past the row is skipped, which is what padding
//     with +infinity would do).  Then the runs of the sorted row: ring size, flags, boundary and non-manifold edges at the
//     smaller end; the workgroup's sum of ring sizes.
//   fuse_scan_kernel  -- ONE workgroup: the offsets of the workgroups' rings, nnz.
//   ma_emit_kernel    -- thread = vertex, then the workgroup: offsets; the run starts of every row to neighbors below the
//     capacity (the longer rows 256 entries at a time with the workgroup prefix).
//   ma_face_ids_kernel -- thread = entry: fid to face_ids below the capacity.
//   ms_pass_kernel    -- thread = vertex: one smoothing pass (8 B of offsets, the ring's 4 B indices, 12 B gathered per
//     neighbour, 12 B read and written).
//   ms_normals_kernel -- thread = vertex: the incident faces' 4 B ids, 12 B indices and 3 x 12 B positions gathered.
// Atomics are integer add, subtract and or; no flag that another workgroup waits on: the same bits on every run.
#include "../../include/ctd_hip_mesh_smooth.h"
#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_row_sort.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

typedef unsigned long long u64;

constexpr int kLaneRow = 16;                                  // incident faces of a row that one lane sorts
constexpr int kLaneRaw = 2 * kLaneRow;

__device__ inline bool face_valid(int a, int b, int c, long n_verts) {
  // unsigned compare: negative indices are out of range too
  return (unsigned long)a < (unsigned long)n_verts && (unsigned long)b < (unsigned long)n_verts &&
         (unsigned long)c < (unsigned long)n_verts && a != b && a != c && b != c;
}

__global__ __launch_bounds__(kChunk) void ma_init_kernel(int* __restrict__ inc, int64_t* __restrict__ counts, long n_verts) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v < n_verts) inc[v] = 0;
  if (v < 6) counts[v] = 0;
}

__global__ __launch_bounds__(kChunk) void ma_count_kernel(const int32_t* __restrict__ faces, int* inc, long n_verts,
                                                          long n_faces) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!face_valid(a, b, c, n_verts)) return;
  atomicAdd(inc + a, 1);
  atomicAdd(inc + b, 1);
  atomicAdd(inc + c, 1);
}

__device__ inline int wave_max(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int other = __shfl_xor(v, d);
    v = other > v ? other : v;
  }
  return v;
}

__global__ __launch_bounds__(kChunk) void ma_sums_kernel(const int* __restrict__ inc, int* __restrict__ wg_sum,
                                                         int* __restrict__ wg_max, long n_verts) {
  __shared__ int wave_n[kChunk / 64], wave_m[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  const int n = v < n_verts ? inc[v] : 0;
  const int top = wave_max(n);
  if ((threadIdx.x & 63) == 0) wave_m[threadIdx.x >> 6] = top;
  int total;
  (void)wg_exclusive_sum<kChunk>(n, wave_n, total);          // (its barrier covers wave_m)
  if (threadIdx.x == 0) {
    wg_sum[blockIdx.x] = total;
    int most = wave_m[0];
#pragma unroll
    for (int w = 1; w < kChunk / 64; ++w) most = wave_m[w] > most ? wave_m[w] : most;
    wg_max[blockIdx.x] = most;
  }
}

// ONE workgroup: max_incident = the largest of the n workgroup maxima (0 for none).  Not an atomic max per wavefront of
// ma_sums_kernel: thousands of them queue at one address (measured: 90 us of the build at 987 K faces).
__global__ __launch_bounds__(kScan) void ma_max_kernel(const int* __restrict__ wg_max, int n, int64_t* __restrict__ counts) {
  __shared__ int wave_m[kScan / 64];
  int top = 0;
  for (int i = threadIdx.x; i < n; i += kScan) top = wg_max[i] > top ? wg_max[i] : top;
  top = wave_max(top);
  if ((threadIdx.x & 63) == 0) wave_m[threadIdx.x >> 6] = top;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kScan / 64; ++w) top = wave_m[w] > top ? wave_m[w] : top;
    counts[4] = (int64_t)top;
  }
}

// (launched with one workgroup at least: foff[n_verts] is written at n_verts == 0 too)
__global__ __launch_bounds__(kChunk) void ma_face_offsets_kernel(const int* __restrict__ inc, const int* __restrict__ wg_off,
                                                                 int* __restrict__ foff, int32_t* __restrict__ face_offsets,
                                                                 int64_t* __restrict__ counts, long n_verts) {
  __shared__ int wave_n[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  int total;
  const int o = wg_off[blockIdx.x] + wg_exclusive_sum<kChunk>(v < n_verts ? inc[v] : 0, wave_n, total);
  if (v <= n_verts) {                                         // (v == n_verts: nothing before it is missing, o is the total)
    foff[v] = o;
    if (face_offsets) face_offsets[v] = o;
  }
  if (v == n_verts) counts[5] = (int64_t)(o / 3);             // every valid face lies in three rows
}

__global__ __launch_bounds__(kChunk) void ma_fill_kernel(const int32_t* __restrict__ faces, int* inc, const int* __restrict__ foff,
                                                         int* __restrict__ fid, int* __restrict__ raw, long n_verts, long n_faces) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  if (!face_valid(a, b, c, n_verts)) return;
  const int v[3] = {a, b, c};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const long p = (long)foff[v[k]] + (atomicSub(inc + v[k], 1) - 1);   // the counter of a vertex holds its row's length
    fid[p] = (int)f;
    raw[2 * p] = v[(k + 1) % 3];
    raw[2 * p + 1] = v[(k + 2) % 3];
  }
}

// entry k of a sorted row of r entries, `stride` apart: 0 when it continues a run, else the run's length capped at 3
__device__ inline int run_start(const int* row, int stride, int k, int r) {
  const int v = row[(long)k * stride];
  if (k > 0 && row[(long)(k - 1) * stride] == v) return 0;
  if (k + 1 >= r || row[(long)(k + 1) * stride] != v) return 1;
  return (k + 2 < r && row[(long)(k + 2) * stride] == v) ? 3 : 2;
}

// what the run that starts at an entry of value j in the row of vertex i adds (mult = run_start > 0)
__device__ inline void run_tally(int mult, int j, long i, int& deg, int& flags, int& n_boundary, int& n_nonmanifold) {
  ++deg;
  if (mult == 1) flags |= CTD_MESH_VERT_BOUNDARY;
  if (mult == 3) flags |= CTD_MESH_VERT_NONMANIFOLD;
  if (j > i) {
    n_boundary += mult == 1;
    n_nonmanifold += mult == 3;
  }
}

// (lane_sort and wg_sort: ctd_row_sort.h)

__global__ __launch_bounds__(kChunk) void ma_rows_kernel(const int* __restrict__ foff, int* fid, int* raw, int* __restrict__ deg,
                                                         uint8_t* __restrict__ vflags, int* __restrict__ wg_deg, int64_t* counts,
                                                         long n_verts) {
  __shared__ int col[kLaneRaw * kChunk];
  __shared__ int wave_n[kChunk / 64];
  __shared__ int long_rows[kChunk];
  __shared__ int n_long, acc[4];
  const int tid = threadIdx.x;
  const long v = (long)blockIdx.x * kChunk + tid;
  if (tid == 0) n_long = 0;
  __syncthreads();
  int my_deg = 0, my_flags = 0, n_boundary = 0, n_nonmanifold = 0;
  if (v < n_verts) {
    const long r0 = foff[v];
    const int n = foff[v + 1] - (int)r0;
    if (n > kLaneRow) {
      long_rows[atomicAdd(&n_long, 1)] = tid;                  // (the order of the list does not reach any output)
    } else if (n > 0) {
      int* mine = col + tid;
      for (int k = 0; k < n; ++k) mine[k * kChunk] = fid[r0 + k];
      lane_sort(mine, n);
      for (int k = 0; k < n; ++k) fid[r0 + k] = mine[k * kChunk];
      const int r = 2 * n;
      for (int k = 0; k < r; ++k) mine[k * kChunk] = raw[2 * r0 + k];
      lane_sort(mine, r);
      for (int k = 0; k < r; ++k) {
        const int j = mine[k * kChunk];
        raw[2 * r0 + k] = j;
        const int mult = run_start(mine, kChunk, k, r);
        if (mult) run_tally(mult, j, v, my_deg, my_flags, n_boundary, n_nonmanifold);
      }
      my_flags |= CTD_MESH_VERT_REFERENCED;
    }
  }
  __syncthreads();
  const int todo = n_long;                                    // uniform
  for (int q = 0; q < todo; ++q) {
    const int owner = long_rows[q];
    const long i = (long)blockIdx.x * kChunk + owner;
    const long r0 = foff[i];
    const int n = foff[i + 1] - (int)r0, r = 2 * n;
    if (tid < 4) acc[tid] = 0;
    wg_sort(fid + r0, n);
    int* row = raw + 2 * r0;
    wg_sort(row, r);                                          // (its last barrier also covers acc)
    int d = 0, fl = 0, nb = 0, nm = 0;
    for (int k = tid; k < r; k += kChunk) {
      const int mult = run_start(row, 1, k, r);
      if (mult) run_tally(mult, row[k], i, d, fl, nb, nm);
    }
    if (d) atomicAdd(&acc[0], d);
    if (fl) atomicOr(&acc[1], fl);
    if (nb) atomicAdd(&acc[2], nb);
    if (nm) atomicAdd(&acc[3], nm);
    __syncthreads();
    if (tid == owner) {
      my_deg = acc[0];
      my_flags = acc[1] | CTD_MESH_VERT_REFERENCED;
      n_boundary += acc[2];
      n_nonmanifold += acc[3];
    }
    __syncthreads();
  }
  if (v < n_verts) {
    deg[v] = my_deg;
    vflags[v] = (uint8_t)my_flags;
  }
  int total, total_b, total_nm;
  (void)wg_exclusive_sum<kChunk>(my_deg, wave_n, total);
  __syncthreads();
  (void)wg_exclusive_sum<kChunk>(n_boundary, wave_n, total_b);
  __syncthreads();
  (void)wg_exclusive_sum<kChunk>(n_nonmanifold, wave_n, total_nm);
  if (tid == 0) {
    wg_deg[blockIdx.x] = total;
    if (total_b) atomicAdd((u64*)(counts + 2), (u64)total_b);
    if (total_nm) atomicAdd((u64*)(counts + 3), (u64)total_nm);
  }
}

// (launched with one workgroup at least: offsets[n_verts] and the number of edges are written at n_verts == 0 too)
__global__ __launch_bounds__(kChunk) void ma_emit_kernel(const int* __restrict__ foff, const int* __restrict__ raw,
                                                         const int* __restrict__ deg, const int* __restrict__ wg_off,
                                                         int32_t* __restrict__ offsets, int32_t* __restrict__ neighbors,
                                                         long cap, int64_t* __restrict__ counts, long n_verts) {
  __shared__ int wave_n[kChunk / 64];
  __shared__ int long_rows[kChunk], long_at[kChunk];
  __shared__ int n_long;
  const int tid = threadIdx.x;
  const long v = (long)blockIdx.x * kChunk + tid;
  if (tid == 0) n_long = 0;
  int total;
  const int o = wg_off[blockIdx.x] + wg_exclusive_sum<kChunk>(v < n_verts ? deg[v] : 0, wave_n, total);   // (a barrier inside)
  if (v <= n_verts) offsets[v] = o;
  if (v == n_verts) counts[1] = (int64_t)(o >> 1);
  if (!neighbors || cap <= 0) return;                         // uniform
  if (v < n_verts) {
    const long r0 = foff[v];
    const int n = foff[v + 1] - (int)r0, r = 2 * n;
    if (n > kLaneRow) {
      const int q = atomicAdd(&n_long, 1);
      long_rows[q] = tid;
      long_at[q] = o;
    } else {
      const int* row = raw + 2 * r0;
      long at = o;
      int prev = -1;                                          // (no entry of a row is negative)
      for (int k = 0; k < r; ++k) {
        const int j = row[k];
        if (j != prev) {
          if (at < cap) neighbors[at] = j;
          ++at;
        }
        prev = j;
      }
    }
  }
  __syncthreads();
  const int todo = n_long;                                    // uniform
  for (int q = 0; q < todo; ++q) {
    const long i = (long)blockIdx.x * kChunk + long_rows[q];
    const long r0 = foff[i];
    const int r = 2 * (foff[i + 1] - (int)r0);
    const int* row = raw + 2 * r0;
    long at = long_at[q];
    for (int base = 0; base < r && at < cap; base += kChunk) { // uniform
      const int k = base + tid;
      const bool first = k < r && (k == 0 || row[k - 1] != row[k]);
      int n_first;
      const long mine = at + wg_flags_before<kChunk>(first, wave_n, n_first);
      if (first && mine < cap) neighbors[mine] = row[k];
      at += n_first;
      __syncthreads();                                        // wave_n is free again
    }
  }
}

__global__ __launch_bounds__(kChunk) void ma_face_ids_kernel(const int* __restrict__ fid, const int* __restrict__ foff,
                                                             int32_t* __restrict__ face_ids, long cap, long n_verts) {
  const long p = (long)blockIdx.x * kChunk + threadIdx.x;
  if (p < cap && p < foff[n_verts]) face_ids[p] = fid[p];
}

__global__ __launch_bounds__(kChunk) void ms_copy_kernel(const float* __restrict__ in, float* __restrict__ out, long n) {
  const long k = (long)blockIdx.x * kChunk + threadIdx.x;
  if (k < n) out[k] = in[k];
}

__global__ __launch_bounds__(kChunk) void ms_pass_kernel(const float* __restrict__ x, const int32_t* __restrict__ offsets,
                                                         const int32_t* __restrict__ neighbors, const uint8_t* __restrict__ vflags,
                                                         float* __restrict__ out, long n_verts, long nnz, float f) {
  const long i = (long)blockIdx.x * kChunk + threadIdx.x;
  if (i >= n_verts) return;
  const float px = x[3 * i], py = x[3 * i + 1], pz = x[3 * i + 2];
  float ox = px, oy = py, oz = pz;
  const long k0 = offsets[i], k1 = offsets[i + 1];
  if (k0 >= 0 && k0 <= k1 && k1 <= nnz && !(vflags && (vflags[i] & CTD_MESH_VERT_BOUNDARY))) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    int d = 0;
    for (long k = k0; k < k1; ++k) {
      const int j = neighbors[k];
      if ((unsigned long)j < (unsigned long)n_verts) {        // nothing is dereferenced before this holds
        sx = sx + x[3l * j];
        sy = sy + x[3l * j + 1];
        sz = sz + x[3l * j + 2];
        ++d;
      }
    }
    if (d > 0) {
      const float fd = (float)d;
      ox = px + f * (sx / fd - px);
      oy = py + f * (sy / fd - py);
      oz = pz + f * (sz / fd - pz);
    }
  }
  out[3 * i] = ox;
  out[3 * i + 1] = oy;
  out[3 * i + 2] = oz;
}

__global__ __launch_bounds__(kChunk) void ms_normals_kernel(const float* __restrict__ x, const int32_t* __restrict__ faces,
                                                            const int32_t* __restrict__ face_offsets,
                                                            const int32_t* __restrict__ face_ids, float* __restrict__ normals,
                                                            long n_verts, long n_faces, long n_incident) {
  const long i = (long)blockIdx.x * kChunk + threadIdx.x;
  if (i >= n_verts) return;
  float ax = 0.f, ay = 0.f, az = 0.f;
  const long k0 = face_offsets[i], k1 = face_offsets[i + 1];
  if (k0 >= 0 && k0 <= k1 && k1 <= n_incident) {
    for (long k = k0; k < k1; ++k) {
      const int f = face_ids[k];
      if ((unsigned long)f >= (unsigned long)n_faces) continue;
      const int a = faces[3l * f], b = faces[3l * f + 1], c = faces[3l * f + 2];
      if ((unsigned long)a >= (unsigned long)n_verts || (unsigned long)b >= (unsigned long)n_verts ||
          (unsigned long)c >= (unsigned long)n_verts)
        continue;
      const float* v0 = x + 3l * a;
      const float* v1 = x + 3l * b;
      const float* v2 = x + 3l * c;
      const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
      const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
      const float cx = e1y * e2z - e1z * e2y, cy = e1z * e2x - e1x * e2z, cz = e1x * e2y - e1y * e2x;
      ax = ax + cx;
      ay = ay + cy;
      az = az + cz;
    }
  }
  const float len = sqrtf((ax * ax + ay * ay) + az * az);
  const float nan = __builtin_nanf("");
  const bool ok = len > 0.f && len < __builtin_inff();
  normals[3 * i] = ok ? ax / len : nan;
  normals[3 * i + 1] = ok ? ay / len : nan;
  normals[3 * i + 2] = ok ? az / len : nan;
}

struct AdjLayout {                                            // byte offsets into the workspace
  size_t inc, foff, deg, fid, raw, wg_inc, wg_deg, wg_max, bytes;
};
AdjLayout adj_layout(int64_t n_verts, int64_t n_faces) {
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  WorkspaceCursor c;
  AdjLayout l;
  l.inc = c.take(sizeof(int) * n);
  l.foff = c.take(sizeof(int) * (n + 1));
  l.deg = c.take(sizeof(int) * n);
  l.fid = c.take(sizeof(int) * 3 * m);
  l.raw = c.take(sizeof(int) * 6 * m);
  l.wg_inc = c.take_counts((size_t)chunks_of(n_verts));
  l.wg_deg = c.take_counts((size_t)chunks_of(n_verts));
  l.wg_max = c.take_counts((size_t)chunks_of(n_verts));
  l.bytes = c.bytes;
  return l;
}

constexpr int64_t kInt32End = 2147483648l;                    // 2^31

// INVALID_ARG, UNSUPPORTED or OK for the sizes alone
int adj_size_status(int64_t n_verts, int64_t n_faces) {
  if (n_verts < 0 || n_faces < 0) return CTD_ERR_INVALID_ARG;
  if (n_faces > (kInt32End - 1) / 6 || n_verts >= kInt32End) return CTD_ERR_UNSUPPORTED;   // 6 * n_faces, n_verts < 2^31
  if (!launch_ok((double)chunks_of(n_faces)) || !launch_ok((double)chunks_of(n_verts))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}
int verts_size_status(int64_t n_verts, int64_t n_entries) {
  if (n_verts < 0 || n_entries < 0) return CTD_ERR_INVALID_ARG;
  if (n_verts >= kInt32End || n_entries >= kInt32End || !launch_ok((double)chunks_of(n_verts))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)chunks_of(n); }
inline unsigned blocks_past(int64_t n) { return (unsigned)chunks_of(n + 1); }   // a thread for item n too

}  // namespace

static int mesh_adjacency_i32(const int32_t* faces, long n_verts, long n_faces, int32_t* offsets, int32_t* neighbors,
                              long cap_neighbors, int32_t* face_offsets, int32_t* face_ids, long cap_face_ids, uint8_t* vflags,
                              int64_t* counts, void* workspace, hipStream_t stream) {
  const AdjLayout l = adj_layout(n_verts, n_faces);
  char* ws = (char*)workspace;
  int* inc = (int*)(ws + l.inc);
  int* foff = (int*)(ws + l.foff);
  int* deg = (int*)(ws + l.deg);
  int* fid = (int*)(ws + l.fid);
  int* raw = (int*)(ws + l.raw);
  int* wg_inc = (int*)(ws + l.wg_inc);
  int* wg_deg = (int*)(ws + l.wg_deg);
  int* wg_max = (int*)(ws + l.wg_max);
  const unsigned vb = blocks_of(n_verts), fb = blocks_of(n_faces), vb1 = blocks_past(n_verts);
  const dim3 wg(kChunk);
  ma_init_kernel<<<dim3(vb ? vb : 1u), wg, 0, stream>>>(inc, counts, n_verts);
  CTD_LAUNCH_CHECK();
  if (fb && vb) {
    ma_count_kernel<<<dim3(fb), wg, 0, stream>>>(faces, inc, n_verts, n_faces);
    CTD_LAUNCH_CHECK();
  }
  if (vb) {
    ma_sums_kernel<<<dim3(vb), wg, 0, stream>>>(inc, wg_inc, wg_max, n_verts);
    CTD_LAUNCH_CHECK();
    ma_max_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(wg_max, (int)vb, counts);
    CTD_LAUNCH_CHECK();
  }
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(wg_inc, (int)vb, (int)vb, nullptr, 0);
  CTD_LAUNCH_CHECK();
  ma_face_offsets_kernel<<<dim3(vb1), wg, 0, stream>>>(inc, wg_inc, foff, face_offsets, counts, n_verts);
  CTD_LAUNCH_CHECK();
  if (fb && vb) {
    ma_fill_kernel<<<dim3(fb), wg, 0, stream>>>(faces, inc, foff, fid, raw, n_verts, n_faces);
    CTD_LAUNCH_CHECK();
  }
  if (vb) {
    ma_rows_kernel<<<dim3(vb), wg, 0, stream>>>(foff, fid, raw, deg, vflags, wg_deg, counts, n_verts);
    CTD_LAUNCH_CHECK();
  }
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(wg_deg, (int)vb, (int)vb, counts, 1);
  CTD_LAUNCH_CHECK();
  ma_emit_kernel<<<dim3(vb1), wg, 0, stream>>>(foff, raw, deg, wg_deg, offsets, neighbors, neighbors ? cap_neighbors : 0, counts,
                                              n_verts);
  CTD_LAUNCH_CHECK();
  if (face_ids && cap_face_ids > 0 && fb && vb) {
    const long most = cap_face_ids < 3 * n_faces ? cap_face_ids : 3 * n_faces;
    ma_face_ids_kernel<<<dim3(blocks_of(most)), wg, 0, stream>>>(fid, foff, face_ids, cap_face_ids, n_verts);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

static int mesh_smooth_f32(const float* verts, long n_verts, const int32_t* offsets, const int32_t* neighbors, long nnz,
                           const uint8_t* vflags, int iters, float lambda, float mu, float* verts_out, void* workspace,
                           hipStream_t stream) {
  const unsigned vb = blocks_of(n_verts);
  if (!vb) return CTD_OK;
  const dim3 wg(kChunk);
  const int per_iter = mu == 0.f ? 1 : 2, passes = iters * per_iter;
  if (passes == 0) {
    ms_copy_kernel<<<dim3(blocks_of(3 * n_verts)), wg, 0, stream>>>(verts, verts_out, 3 * n_verts);
    CTD_LAUNCH_CHECK();
    return CTD_OK;
  }
  // the last pass writes the output, the one before it the workspace, and so back to the first, which reads verts
  const float* src = verts;
  for (int p = 0; p < passes; ++p) {
    float* dst = ((passes - 1 - p) & 1) ? (float*)workspace : verts_out;
    ms_pass_kernel<<<dim3(vb), wg, 0, stream>>>(src, offsets, neighbors, vflags, dst, n_verts, nnz,
                                               (per_iter == 2 && (p & 1)) ? mu : lambda);
    CTD_LAUNCH_CHECK();
    src = dst;
  }
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_mesh_adjacency_workspace_bytes(int64_t n_verts, int64_t n_faces) {
  if (adj_size_status(n_verts, n_faces) != CTD_OK) return 0;
  return adj_layout(n_verts, n_faces).bytes;
}

size_t ctd_mesh_smooth_workspace_bytes(int64_t n_verts) {
  if (verts_size_status(n_verts, 0) != CTD_OK) return 0;
  return align_up(12 * (size_t)n_verts, 256);
}

int ctd_mesh_adjacency_i32(const int32_t* faces, int64_t n_verts, int64_t n_faces, int32_t* offsets, int32_t* neighbors,
                           int64_t cap_neighbors, int32_t* face_offsets, int32_t* face_ids, int64_t cap_face_ids,
                           uint8_t* vflags, int64_t* counts, void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || !faces || !offsets || !vflags || !counts) return CTD_ERR_INVALID_ARG;
  if ((neighbors && cap_neighbors < 0) || (face_ids && cap_face_ids < 0)) return CTD_ERR_INVALID_ARG;
  const int st = adj_size_status(n_verts, n_faces);
  if (st != CTD_OK) return st;
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  const size_t cn = neighbors ? ((size_t)cap_neighbors < 6 * m ? (size_t)cap_neighbors : 6 * m) : 0;
  const size_t cf = face_ids ? ((size_t)cap_face_ids < 3 * m ? (size_t)cap_face_ids : 3 * m) : 0;
  const size_t need = ctd_mesh_adjacency_workspace_bytes(n_verts, n_faces);
  const Span s[] = {{offsets, 4 * (n + 1)}, {neighbors, 4 * cn}, {face_offsets, 4 * (n + 1)}, {face_ids, 4 * cf}, {vflags, n},
                    {counts, 48},           {workspace, need},   {faces, 12 * m}};
  if (spans_overlap(s, 7, 8)) return CTD_ERR_INVALID_ARG;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_adjacency_i32(faces, (long)n_verts, (long)n_faces, offsets, neighbors, (long)cap_neighbors, face_offsets, face_ids,
                            (long)cap_face_ids, vflags, counts, workspace, (hipStream_t)stream);
}

int ctd_mesh_smooth_f32(const float* verts, int64_t n_verts, const int32_t* offsets, const int32_t* neighbors, int64_t nnz,
                        const uint8_t* vflags, int iters, float lambda, float mu, int fix_boundary, float* verts_out,
                        void* workspace, size_t workspace_bytes, int device, void* stream) {
  if (n_verts < 0 || nnz < 0 || !verts || !offsets || !neighbors || !verts_out || (fix_boundary && !vflags))
    return CTD_ERR_INVALID_ARG;
  if (iters < 0 || iters > 1024 || !(lambda > 0.f && lambda <= 1.f) || !(mu >= -2.f && mu <= 0.f)) return CTD_ERR_INVALID_ARG;
  const int st = verts_size_status(n_verts, nnz);
  if (st != CTD_OK) return st;
  const size_t n = (size_t)n_verts;
  const size_t need = ctd_mesh_smooth_workspace_bytes(n_verts);
  const Span s[] = {{verts_out, 12 * n},        {workspace, need},           {verts, 12 * n},
                    {offsets, 4 * (n + 1)},     {neighbors, 4 * (size_t)nnz}, {fix_boundary ? vflags : nullptr, n}};
  if (spans_overlap(s, 2, 6)) return CTD_ERR_INVALID_ARG;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_smooth_f32(verts, (long)n_verts, offsets, neighbors, (long)nnz, fix_boundary ? vflags : nullptr, iters, lambda, mu,
                         verts_out, workspace, (hipStream_t)stream);
}

int ctd_mesh_vertex_normals_f32(const float* verts, int64_t n_verts, const int32_t* faces, int64_t n_faces,
                                const int32_t* face_offsets, const int32_t* face_ids, int64_t n_incident, float* normals,
                                int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_incident < 0 || !verts || !faces || !face_offsets || !face_ids || !normals)
    return CTD_ERR_INVALID_ARG;
  int st = adj_size_status(n_verts, n_faces);
  if (st == CTD_OK) st = verts_size_status(n_verts, n_incident);
  if (st != CTD_OK) return st;
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  const Span s[] = {{normals, 12 * n}, {verts, 12 * n}, {faces, 12 * m}, {face_offsets, 4 * (n + 1)},
                    {face_ids, 4 * (size_t)n_incident}};
  if (spans_overlap(s, 1, 5)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  if (n_verts > 0) {
    ms_normals_kernel<<<dim3(blocks_of(n_verts)), dim3(kChunk), 0, (hipStream_t)stream>>>(
        verts, faces, face_offsets, face_ids, normals, (long)n_verts, (long)n_faces, (long)n_incident);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

}  // extern "C"
