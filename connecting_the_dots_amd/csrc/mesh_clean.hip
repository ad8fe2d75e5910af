// mesh_clean.hip -- connected components, small-fragment removal and compaction of an indexed triangle mesh
// (ctd_mesh_components_i32, ctd_mesh_clean_i32; the rule is stated word for word in include/ctd_hip_mesh_clean.h).
//
// The union-find is that of ctd_union_find.h (shared with disp_filter.hip): parent[] over the vertices, every write an
// integer atomic min, so the root of a set is its smallest vertex -- the component's label -- whatever order the atomics
// landed in.  The workgroup prefix and fuse_scan_kernel (with B = 1) are those of ctd_compact.h.  A workgroup takes 256
// consecutive faces or vertices.
//   mc_init_kernel    -- thread = vertex: parent = itself, size counter and kept flag 0; the call's counters 0.  9 B written.
//   mc_union_kernel   -- thread = face: the validity test (indices, then positions where asked: 12 B + 3 x 12 B gathered),
//     v0 or -1 to root[] (4 B), and for a valid face the unions (v0,v1), (v0,v2).
//   mc_flatten_kernel -- thread = face: the root of root[] (4 B read, the chain, 4 B written) and one integer atomic add
//     at the root's counter per run of equal roots inside the wavefront.  tsdf_mesh emits faces in cell order, so with one
//     giant component the runs are whole wavefronts.
//   mc_roots_kernel   -- thread = vertex (8 B read): the roots of counted sets: their number, the number with
//     size >= min_faces (one 64-bit integer add per wavefront each), and with keep_largest the largest key
//     (size << 32 | 0x7fffffff - label): a wavefront maximum, one 64-bit integer atomic max.
//   mc_sizes_kernel   -- (components call) thread = face: size = the counter at the root.  4 B read + 4 gathered, 4 written.
//   mc_flag_kernel    -- thread = face: kept flag (4 B read, 4 gathered, 1 B written), for a kept face a byte 1 at its three
//     vertices (12 B read; racing equal stores), the workgroup's number of kept faces.
//   mc_vert_count_kernel -- thread = vertex: the workgroup's number of kept vertices (1 B read).
//   fuse_scan_kernel  -- ONE workgroup, twice: the offsets of the face and of the vertex workgroups, the two totals.
//   mc_vert_scatter_kernel -- thread = vertex: the new index (offset + flags before it), 4 B written per vertex (-1 where
//     not kept), vert_index below the capacity.
//   mc_face_scatter_kernel -- thread = face: a kept face below the capacity: 12 B read, 3 x 4 B gathered, 12 + 4 B written.
// Atomics are integer min / add / max; no flag that another workgroup waits on: the same bits on every run.
#include "../../include/ctd_hip_mesh_clean.h"
#include "ctd_common.h"
#include "ctd_compact.h"
#include "ctd_union_find.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(kChunk) void mc_init_kernel(int* __restrict__ parent, int* __restrict__ count,
                                                         uint8_t* __restrict__ vkeep, u64* __restrict__ best,
                                                         int64_t* __restrict__ n_comp, int64_t* __restrict__ n_comp_kept,
                                                         long n_verts) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  if (v < n_verts) {
    parent[v] = (int)v;
    count[v] = 0;
    vkeep[v] = 0;
  }
  if (v == 0) {
    *best = 0ull;
    *n_comp = 0;
    if (n_comp_kept) *n_comp_kept = 0;
  }
}

__device__ inline bool same_position(const float* __restrict__ verts, int a, int b) {
  const float* p = verts + 3l * a;
  const float* q = verts + 3l * b;
  return p[0] == q[0] && p[1] == q[1] && p[2] == q[2];
}

__global__ __launch_bounds__(kChunk) void mc_union_kernel(const int32_t* __restrict__ faces, const float* __restrict__ verts,
                                                          int* parent, int* __restrict__ root, long n_verts, long n_faces,
                                                          int drop_degenerate) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
  // unsigned compare: negative indices are out of range too; nothing is dereferenced before this holds
  bool valid = (unsigned long)a < (unsigned long)n_verts && (unsigned long)b < (unsigned long)n_verts &&
               (unsigned long)c < (unsigned long)n_verts && a != b && a != c && b != c;
  if (valid && drop_degenerate)
    valid = !same_position(verts, a, b) && !same_position(verts, a, c) && !same_position(verts, b, c);
  root[f] = valid ? a : -1;
  if (valid) {
    uf_union<kAgent>(parent, a, b);
    uf_union<kAgent>(parent, a, c);
  }
}

__global__ __launch_bounds__(kChunk) void mc_flatten_kernel(int* parent, int* __restrict__ root, int* count, long n_faces) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  long key = -1;
  if (f < n_faces) {
    const int v = root[f];
    if (v >= 0) {
      const int rt = uf_find<kAgent>(parent, v);
      root[f] = rt;
      key = rt;
    }
  }
  uf_count_runs(count, key);
}

__global__ __launch_bounds__(kChunk) void mc_roots_kernel(const int* __restrict__ parent, const int* __restrict__ count,
                                                          u64* best, int64_t* n_comp, int64_t* n_comp_kept, long n_verts,
                                                          int min_faces, int keep_largest) {
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int n = 0;
  if (v < n_verts && parent[v] == (int)v) n = count[v];          // > 0: the root of a component
  const u64 roots = __ballot(n > 0), big = __ballot(n >= min_faces && n > 0);
  if (lane == 0 && roots) atomicAdd((u64*)n_comp, (u64)__popcll(roots));
  if (!keep_largest) {
    if (lane == 0 && big && n_comp_kept) atomicAdd((u64*)n_comp_kept, (u64)__popcll(big));
    return;
  }
  u64 key = n > 0 ? ((u64)(unsigned)n << 32) | (u64)(0x7fffffffu - (unsigned)v) : 0ull;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const u64 other = __shfl_xor(key, d);
    key = other > key ? other : key;
  }
  if (lane == 0 && key) atomicMax(best, key);
}

__global__ __launch_bounds__(kChunk) void mc_sizes_kernel(const int* __restrict__ root, const int* __restrict__ count,
                                                          int32_t* __restrict__ size, long n_faces) {
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  if (f >= n_faces) return;
  const int rt = root[f];
  size[f] = rt >= 0 ? count[rt] : 0;
}

__global__ __launch_bounds__(kChunk) void mc_flag_kernel(const int32_t* __restrict__ faces, const int* __restrict__ root,
                                                         const int* __restrict__ count, const u64* __restrict__ best,
                                                         uint8_t* __restrict__ fkeep, uint8_t* vkeep,
                                                         int* __restrict__ wg_faces, int64_t* __restrict__ n_comp_kept,
                                                         long n_faces, int min_faces, int keep_largest) {
  __shared__ int wave_cnt[kChunk / 64];
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  const u64 top = keep_largest ? *best : 0ull;
  const int top_size = (int)(top >> 32), top_label = top ? (int)(0x7fffffffu - (unsigned)(top & 0xffffffffull)) : -1;
  bool keep = false;
  if (f < n_faces) {
    const int rt = root[f];
    keep = rt >= 0 && count[rt] >= min_faces && (!keep_largest || rt == top_label);
    fkeep[f] = keep ? 1 : 0;
    if (keep) {                                                  // a valid face: its indices are in range
      vkeep[faces[3 * f]] = 1;
      vkeep[faces[3 * f + 1]] = 1;
      vkeep[faces[3 * f + 2]] = 1;
    }
  }
  int total;
  (void)wg_flags_before<kChunk>(keep, wave_cnt, total);
  if (threadIdx.x == 0) {
    wg_faces[blockIdx.x] = total;
    if (keep_largest && blockIdx.x == 0) *n_comp_kept = top_size >= min_faces && top_size > 0 ? 1 : 0;
  }
}

__global__ __launch_bounds__(kChunk) void mc_vert_count_kernel(const uint8_t* __restrict__ vkeep, int* __restrict__ wg_verts,
                                                               long n_verts) {
  __shared__ int wave_cnt[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  int total;
  (void)wg_flags_before<kChunk>(v < n_verts && vkeep[v], wave_cnt, total);
  if (threadIdx.x == 0) wg_verts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kChunk) void mc_vert_scatter_kernel(const uint8_t* __restrict__ vkeep,
                                                                 const int* __restrict__ vert_offsets, int* __restrict__ vnew,
                                                                 int32_t* __restrict__ vert_index, long cap_verts,
                                                                 long n_verts) {
  __shared__ int wave_cnt[kChunk / 64];
  const long v = (long)blockIdx.x * kChunk + threadIdx.x;
  const bool keep = v < n_verts && vkeep[v];
  int total;
  const int o = vert_offsets[blockIdx.x] + wg_flags_before<kChunk>(keep, wave_cnt, total);
  if (v < n_verts) vnew[v] = keep ? o : -1;
  if (keep && vert_index && o < cap_verts) vert_index[o] = (int32_t)v;
}

__global__ __launch_bounds__(kChunk) void mc_face_scatter_kernel(const int32_t* __restrict__ faces,
                                                                 const uint8_t* __restrict__ fkeep,
                                                                 const int* __restrict__ face_offsets,
                                                                 const int* __restrict__ vnew, int32_t* __restrict__ faces_out,
                                                                 int32_t* __restrict__ face_index, long cap_faces,
                                                                 long n_faces) {
  __shared__ int wave_cnt[kChunk / 64];
  // a workgroup without kept faces, or with all of them past the capacity, has nothing to write (uniform: before the barrier)
  const int first = face_offsets[blockIdx.x];
  if (face_offsets[blockIdx.x + 1] == first || first >= cap_faces) return;
  const long f = (long)blockIdx.x * kChunk + threadIdx.x;
  const bool keep = f < n_faces && fkeep[f];
  int total;
  const long o = (long)first + wg_flags_before<kChunk>(keep, wave_cnt, total);
  if (!keep || o >= cap_faces) return;
  if (faces_out) {
    faces_out[3 * o] = vnew[faces[3 * f]];
    faces_out[3 * o + 1] = vnew[faces[3 * f + 1]];
    faces_out[3 * o + 2] = vnew[faces[3 * f + 2]];
  }
  if (face_index) face_index[o] = (int32_t)f;
}

struct CleanLayout {                                          // byte offsets into the workspace
  size_t parent, count, vnew, root, vkeep, fkeep, face_offsets, vert_offsets, best, bytes;
};
CleanLayout clean_layout(int64_t n_verts, int64_t n_faces) {
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  WorkspaceCursor c;
  CleanLayout l;
  l.parent = c.take(sizeof(int) * n);
  l.count = c.take(sizeof(int) * n);
  l.vnew = c.take(sizeof(int) * n);
  l.root = c.take(sizeof(int) * m);
  l.vkeep = c.take(n);
  l.fkeep = c.take(m);
  l.face_offsets = c.take_counts((size_t)chunks_of(n_faces));
  l.vert_offsets = c.take_counts((size_t)chunks_of(n_verts));
  l.best = c.take(sizeof(u64));
  l.bytes = c.bytes;
  return l;
}

// INVALID_ARG, UNSUPPORTED or OK for the sizes alone
int clean_size_status(int64_t n_verts, int64_t n_faces) {
  if (n_verts < 0 || n_faces < 0) return CTD_ERR_INVALID_ARG;
  if (n_faces > (2147483647l) / 3 || n_verts > 2147483647l) return CTD_ERR_UNSUPPORTED;   // 3 * n_faces, n_verts < 2^31
  if (!launch_ok((double)chunks_of(n_faces)) || !launch_ok((double)chunks_of(n_verts))) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)chunks_of(n); }

// init, union, flatten, roots: afterwards root[f] is the label of face f, count[label] the size
int mesh_label(const int32_t* faces, const float* verts, long n_verts, long n_faces, int drop_degenerate, int min_faces,
               int keep_largest, int* root, int64_t* n_comp, int64_t* n_comp_kept, char* ws, const CleanLayout& l,
               hipStream_t stream) {
  int* parent = (int*)(ws + l.parent);
  int* count = (int*)(ws + l.count);
  uint8_t* vkeep = (uint8_t*)(ws + l.vkeep);
  u64* best = (u64*)(ws + l.best);
  const unsigned vb = blocks_of(n_verts), fb = blocks_of(n_faces);
  mc_init_kernel<<<dim3(vb ? vb : 1u), dim3(kChunk), 0, stream>>>(parent, count, vkeep, best, n_comp, n_comp_kept, n_verts);
  CTD_LAUNCH_CHECK();
  if (fb) {
    mc_union_kernel<<<dim3(fb), dim3(kChunk), 0, stream>>>(faces, verts, parent, root, n_verts, n_faces, drop_degenerate);
    CTD_LAUNCH_CHECK();
    mc_flatten_kernel<<<dim3(fb), dim3(kChunk), 0, stream>>>(parent, root, count, n_faces);
    CTD_LAUNCH_CHECK();
  }
  if (vb && fb) {
    mc_roots_kernel<<<dim3(vb), dim3(kChunk), 0, stream>>>(parent, count, best, n_comp, n_comp_kept, n_verts, min_faces,
                                                          keep_largest);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

}  // namespace

static int mesh_components_i32(const int32_t* faces, const float* verts, long n_verts, long n_faces, int drop_degenerate,
                               int32_t* label, int32_t* size, int64_t* n_components, void* workspace, hipStream_t stream) {
  const CleanLayout l = clean_layout(n_verts, n_faces);
  char* ws = (char*)workspace;
  const int st = mesh_label(faces, verts, n_verts, n_faces, drop_degenerate, 1, 0, label, n_components, nullptr, ws, l, stream);
  if (st != CTD_OK) return st;
  if (n_faces > 0) {
    mc_sizes_kernel<<<dim3(blocks_of(n_faces)), dim3(kChunk), 0, stream>>>(label, (const int*)(ws + l.count), size, n_faces);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

static int mesh_clean_i32(const int32_t* faces, const float* verts, long n_verts, long n_faces, int drop_degenerate,
                          int min_faces, int keep_largest, int32_t* faces_out, int32_t* face_index, long cap_faces,
                          int32_t* vert_index, long cap_verts, int64_t* counts, void* workspace, hipStream_t stream) {
  const CleanLayout l = clean_layout(n_verts, n_faces);
  char* ws = (char*)workspace;
  int* count = (int*)(ws + l.count);
  int* vnew = (int*)(ws + l.vnew);
  int* root = (int*)(ws + l.root);
  uint8_t* vkeep = (uint8_t*)(ws + l.vkeep);
  uint8_t* fkeep = (uint8_t*)(ws + l.fkeep);
  int* face_offsets = (int*)(ws + l.face_offsets);
  int* vert_offsets = (int*)(ws + l.vert_offsets);
  const u64* best = (const u64*)(ws + l.best);
  const int st = mesh_label(faces, verts, n_verts, n_faces, drop_degenerate, min_faces, keep_largest, root, counts + 2,
                            counts + 3, ws, l, stream);
  if (st != CTD_OK) return st;
  const unsigned vb = blocks_of(n_verts), fb = blocks_of(n_faces);
  if (fb) {
    mc_flag_kernel<<<dim3(fb), dim3(kChunk), 0, stream>>>(faces, root, count, best, fkeep, vkeep, face_offsets, counts + 3,
                                                         n_faces, min_faces, keep_largest);
    CTD_LAUNCH_CHECK();
  }
  if (vb) {
    mc_vert_count_kernel<<<dim3(vb), dim3(kChunk), 0, stream>>>(vkeep, vert_offsets, n_verts);
    CTD_LAUNCH_CHECK();
  }
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(face_offsets, (int)fb, (int)fb, counts + 1, 1);
  CTD_LAUNCH_CHECK();
  fuse_scan_kernel<<<dim3(1), dim3(kScan), 0, stream>>>(vert_offsets, (int)vb, (int)vb, counts, 1);
  CTD_LAUNCH_CHECK();
  const bool want_faces = (faces_out || face_index) && cap_faces > 0;
  const bool want_verts = vert_index && cap_verts > 0;
  if (vb && ((want_faces && faces_out) || want_verts)) {
    mc_vert_scatter_kernel<<<dim3(vb), dim3(kChunk), 0, stream>>>(vkeep, vert_offsets, vnew, vert_index, cap_verts, n_verts);
    CTD_LAUNCH_CHECK();
  }
  if (fb && want_faces) {
    mc_face_scatter_kernel<<<dim3(fb), dim3(kChunk), 0, stream>>>(faces, fkeep, face_offsets, vnew, faces_out, face_index,
                                                                 cap_faces, n_faces);
    CTD_LAUNCH_CHECK();
  }
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_mesh_clean_workspace_bytes(int64_t n_verts, int64_t n_faces) {
  if (clean_size_status(n_verts, n_faces) != CTD_OK) return 0;
  return clean_layout(n_verts, n_faces).bytes;
}

int ctd_mesh_components_i32(const int32_t* faces, const float* verts, int64_t n_verts, int64_t n_faces, int drop_degenerate,
                            int32_t* label, int32_t* size, int64_t* n_components, void* workspace, size_t workspace_bytes,
                            int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || !faces || !label || !size || !n_components || (drop_degenerate && !verts))
    return CTD_ERR_INVALID_ARG;
  const int st = clean_size_status(n_verts, n_faces);
  if (st != CTD_OK) return st;
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  const size_t need = ctd_mesh_clean_workspace_bytes(n_verts, n_faces);
  const Span s[] = {{label, 4 * m}, {size, 4 * m}, {n_components, 8}, {workspace, need}, {faces, 12 * m},
                    {drop_degenerate ? verts : nullptr, 12 * n}};
  if (spans_overlap(s, 4, 6)) return CTD_ERR_INVALID_ARG;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_components_i32(faces, verts, (long)n_verts, (long)n_faces, drop_degenerate ? 1 : 0, label, size, n_components,
                             workspace, (hipStream_t)stream);
}

int ctd_mesh_clean_i32(const int32_t* faces, const float* verts, int64_t n_verts, int64_t n_faces, int drop_degenerate,
                       int min_faces, int keep_largest, int32_t* faces_out, int32_t* face_index, int64_t cap_faces,
                       int32_t* vert_index, int64_t cap_verts, int64_t* counts, void* workspace, size_t workspace_bytes,
                       int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || min_faces < 1 || !faces || !counts || (drop_degenerate && !verts))
    return CTD_ERR_INVALID_ARG;
  if (((faces_out || face_index) && cap_faces < 0) || (vert_index && cap_verts < 0)) return CTD_ERR_INVALID_ARG;
  const int st = clean_size_status(n_verts, n_faces);
  if (st != CTD_OK) return st;
  const size_t n = (size_t)n_verts, m = (size_t)n_faces;
  const size_t cf = (faces_out || face_index) ? ((size_t)cap_faces < m ? (size_t)cap_faces : m) : 0;
  const size_t cv = vert_index ? ((size_t)cap_verts < n ? (size_t)cap_verts : n) : 0;
  const size_t need = ctd_mesh_clean_workspace_bytes(n_verts, n_faces);
  const Span s[] = {{faces_out, 12 * cf}, {face_index, 4 * cf}, {vert_index, 4 * cv}, {counts, 32}, {workspace, need},
                    {faces, 12 * m}, {drop_degenerate ? verts : nullptr, 12 * n}};
  if (spans_overlap(s, 5, 7)) return CTD_ERR_INVALID_ARG;
  if (!workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_clean_i32(faces, verts, (long)n_verts, (long)n_faces, drop_degenerate ? 1 : 0, min_faces, keep_largest ? 1 : 0,
                        faces_out, face_index, (long)cap_faces, vert_index, (long)cap_verts, counts, workspace,
                        (hipStream_t)stream);
}

}  // extern "C"
