// render_bvh.hip -- a device-built bounding volume hierarchy for the ray caster of render.hip, and the two
// renderers (mesh_proj, mesh) traversing it.  The result is the brute-force caster's, bit for bit: the same
// ray_tri (ctd_render.h) decides every hit, and the tree only skips faces that provably cannot be the answer.
//
// Build (deterministic LBVH, Karras 2012; a pure function of verts/faces, two builds give the same bytes):
//   1. per face: centroid, and the centroid bounds by atomic min/max (order-independent);
//   2. 63-bit Morton codes (21 bits per axis) of the centroids over those bounds, non-finite centroids -> code 0;
//   3. a stable LSD radix sort of (code, face) pairs, 4-bit digits, own kernels (ties stay in face order, so the
//      sort key is in effect code.face: unique);
//   4. Karras's hierarchy over the sorted keys, the face index breaking ties of equal codes (delta = 64 + clz);
//   5. bottom-up refit with arrival counters (agent-scope acq_rel): the second arrival forms the union of both
//      children.  A node covering <= kLeafFaces faces becomes a leaf over that range of sorted faces.
//   The tree depth (leaf ranges count as depth 0) is recorded; deeper than kMaxDepth = CTD_ERR_UNSUPPORTED.
//
// Buffer (ctd_mesh_bvh_bytes(n), 16-byte aligned sections):
//   header  int32[16]: magic, n_faces, n_nodes = max(2n-1, 0), depth, root, 0...
//   box     float4[n_nodes][2]: (lo.xyz, P), (hi.xyz, E) -- P, E per-node bound coefficients, see below
//   meta    int4[n_nodes]: internal (left, right, parent, height) or leaf (-(first+1), count, parent, 0)
//   tris    float4[n][3]: sorted faces' gathered vertices v0, v1, v2 (.w of the first = original face index)
//   Internal nodes are 0..n-2, single-face leaves n-1..2n-2, root 0 (n >= 2) or 0 (= the one leaf, n = 1).
//
// Traversal: one wave per 8x8 pixel tile, one ray per lane, a per-lane stack in LDS (kStack entries, the push
// bounds-checked besides the depth check at launch).  Selection is order independent: a face accepted by ray_tri
// replaces the best if ft < t_best, or ft == t_best with a lower face index.  Since brute force keeps the first
// (lowest-index) face of minimal ft, any visiting order yields its face, t, u, v -- provided no face that
// ray_tri could accept with ft <= t_best is pruned.  The pruning rule guarantees that.
//
// Why pruning is safe: the forward-error bound of ray_tri behind `prune`, and `prune` itself, are in ctd_bvh_ray.h
// (shared with the occlusion query of mesh_color.hip).  A node is pruned only if no face under it could be accepted
// with ft <= t_best; a ray with a non-finite origin or direction (the shadow ray's pdir has z = 0) prunes nothing.
#include <cstdint>

#include "ctd_bvh.h"
#include "ctd_bvh_ray.h"
#include "ctd_common.h"
#include "ctd_mesh_query.h"
#include "ctd_render.h"

namespace ctd {

// the buffer's layout, view, header check and stack depth: ctd_bvh.h; the leaf fetch and the lane stack: ctd_mesh_query.h
constexpr int kLeafFaces = 4;       // a node over <= kLeafFaces sorted faces is a leaf
constexpr int kSortThreads = 256, kSortItems = 16, kSortTile = kSortThreads * kSortItems;
constexpr int kDigitBits = 4, kDigits = 1 << kDigitBits, kKeyBits = 63;

struct WsLayout {
  size_t keys0, keys1, vals0, vals1, hist, counters, bounds, total;
};
static WsLayout ws_layout(long n) {
  const long tiles = (n + kSortTile - 1) / kSortTile;
  WsLayout W;
  W.keys0 = 0;
  W.keys1 = W.keys0 + align16((size_t)n * 8);
  W.vals0 = W.keys1 + align16((size_t)n * 8);
  W.vals1 = W.vals0 + align16((size_t)n * 4);
  W.hist = W.vals1 + align16((size_t)n * 4);
  W.counters = W.hist + align16((size_t)tiles * kDigits * 4);
  W.bounds = W.counters + align16((size_t)n * 4);
  W.total = W.bounds + 64;
  return W;
}

static size_t mesh_bvh_bytes(long n_faces) { return bvh_layout(n_faces).total; }
static size_t mesh_bvh_workspace_bytes(long n_faces) { return ws_layout(n_faces).total; }

// ---------------------------------------------------------------------------------------------------- build

// float <-> order-preserving uint (for atomic min / max of floats)
__device__ inline unsigned f2ord(float f) {
  const unsigned b = __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ inline float ord2f(unsigned o) { return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o); }

__device__ inline void centroid(const float* __restrict__ verts, const int* __restrict__ faces, long f, float* c) {
  const float *a = verts + (long)faces[f * 3] * 3, *b = verts + (long)faces[f * 3 + 1] * 3,
              *d = verts + (long)faces[f * 3 + 2] * 3;
  for (int k = 0; k < 3; ++k) c[k] = (a[k] + b[k] + d[k]) * (1.f / 3.f);
}

__global__ void bvh_bounds_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int n,
                                  unsigned* __restrict__ bounds) {
  unsigned lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
  for (long f = blockIdx.x * (long)blockDim.x + threadIdx.x; f < n; f += (long)gridDim.x * blockDim.x) {
    float c[3];
    centroid(verts, faces, f, c);
    if (!finite3(c)) continue;
    for (int k = 0; k < 3; ++k) {
      lo[k] = min(lo[k], f2ord(c[k]));
      hi[k] = max(hi[k], f2ord(c[k]));
    }
  }
  for (int k = 0; k < 3; ++k) {
    atomicMin(bounds + k, lo[k]);
    atomicMax(bounds + 3 + k, hi[k]);
  }
}

__device__ inline unsigned long long spread21(unsigned long long x) {   // 21 bits -> every third bit
  x &= 0x1fffffull;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

__global__ void bvh_morton_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int n,
                                  const unsigned* __restrict__ bounds, unsigned long long* __restrict__ keys,
                                  int* __restrict__ vals) {
  const long f = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (f >= n) return;
  float c[3];
  centroid(verts, faces, f, c);
  unsigned long long code = 0;
  if (finite3(c)) {
    unsigned long long q[3];
    for (int k = 0; k < 3; ++k) {
      const double lo = ord2f(bounds[k]), hi = ord2f(bounds[3 + k]);
      const double x = hi > lo ? ((double)c[k] - lo) / (hi - lo) * 2097151.0 : 0.0;
      q[k] = (unsigned long long)fmin(fmax(x, 0.0), 2097151.0);
    }
    code = spread21(q[0]) << 2 | spread21(q[1]) << 1 | spread21(q[2]);
  }
  keys[f] = code;
  vals[f] = (int)f;
}

// stable LSD radix sort pass: each thread owns kSortItems consecutive items of its tile
__global__ __launch_bounds__(kSortThreads) void sort_hist_kernel(const unsigned long long* __restrict__ keys, int n,
                                                                 int shift, int tiles, unsigned* __restrict__ hist) {
  __shared__ unsigned cnt[kDigits];
  if (threadIdx.x < kDigits) cnt[threadIdx.x] = 0;
  __syncthreads();
  const long base = (long)blockIdx.x * kSortTile + (long)threadIdx.x * kSortItems;
  for (int i = 0; i < kSortItems; ++i)
    if (base + i < n) atomicAdd(&cnt[(keys[base + i] >> shift) & (kDigits - 1)], 1u);
  __syncthreads();
  if (threadIdx.x < kDigits) hist[(long)threadIdx.x * tiles + blockIdx.x] = cnt[threadIdx.x];
}

// exclusive scan of hist[kDigits][tiles] in digit-major order, one workgroup
__global__ __launch_bounds__(1024) void sort_scan_kernel(unsigned* __restrict__ hist, long len) {
  __shared__ unsigned part[1024];
  const long per = (len + 1023) / 1024, b = threadIdx.x * per, e = min(len, b + per);
  unsigned s = 0;
  for (long i = b; i < e; ++i) s += hist[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned run = 0;
    for (int i = 0; i < 1024; ++i) { const unsigned x = part[i]; part[i] = run; run += x; }
  }
  __syncthreads();
  unsigned run = part[threadIdx.x];
  for (long i = b; i < e; ++i) { const unsigned x = hist[i]; hist[i] = run; run += x; }
}

__global__ __launch_bounds__(kSortThreads) void sort_scatter_kernel(const unsigned long long* __restrict__ keys_in,
                                                                    const int* __restrict__ vals_in, int n, int shift,
                                                                    int tiles, const unsigned* __restrict__ offs,
                                                                    unsigned long long* __restrict__ keys_out,
                                                                    int* __restrict__ vals_out) {
  __shared__ unsigned cnt[kDigits][kSortThreads + 1];
  for (int d = 0; d < kDigits; ++d) cnt[d][threadIdx.x] = 0;
  const long base = (long)blockIdx.x * kSortTile + (long)threadIdx.x * kSortItems;
  for (int i = 0; i < kSortItems; ++i)
    if (base + i < n) cnt[(keys_in[base + i] >> shift) & (kDigits - 1)][threadIdx.x] += 1;
  __syncthreads();
  if (threadIdx.x < kDigits) {             // exclusive scan over the threads, per digit, plus the tile's offset
    unsigned run = offs[(long)threadIdx.x * tiles + blockIdx.x];
    for (int t = 0; t < kSortThreads; ++t) { const unsigned x = cnt[threadIdx.x][t]; cnt[threadIdx.x][t] = run; run += x; }
  }
  __syncthreads();
  for (int i = 0; i < kSortItems; ++i) {
    if (base + i >= n) break;
    const unsigned long long k = keys_in[base + i];
    const int d = (int)((k >> shift) & (kDigits - 1));
    const unsigned pos = cnt[d][threadIdx.x]++;
    keys_out[pos] = k;
    vals_out[pos] = vals_in[base + i];
  }
}

// per sorted position j: the gathered triangle, the leaf node's box and bound coefficients
__global__ void bvh_leaves_kernel(const float* __restrict__ verts, const int* __restrict__ faces, int n,
                                  const int* __restrict__ order, float4* __restrict__ box, int4* __restrict__ meta,
                                  float4* __restrict__ tris) {
  const long j = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int f = order[j];
  const float *a = verts + (long)faces[(long)f * 3] * 3, *b = verts + (long)faces[(long)f * 3 + 1] * 3,
              *c = verts + (long)faces[(long)f * 3 + 2] * 3;
  tris[j * 3 + 0] = make_float4(a[0], a[1], a[2], __int_as_float(f));
  tris[j * 3 + 1] = make_float4(b[0], b[1], b[2], 0.f);
  tris[j * 3 + 2] = make_float4(c[0], c[1], c[2], 0.f);
  float lo[3], hi[3], P, E;
  if (finite3(a) && finite3(b) && finite3(c)) {
    const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};     // as ray_tri forms them
    const float e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const float n1 = norm3(e1), n2 = norm3(e2);
    P = n1 * n2 * 1.00001f;
    E = fmaxf(n1, n2) * 1.00001f;
    if (!isfinite(P) || !isfinite(E)) P = E = INFINITY;
    for (int k = 0; k < 3; ++k) {
      lo[k] = fminf(a[k], fminf(b[k], c[k]));
      hi[k] = fmaxf(a[k], fmaxf(b[k], c[k]));
    }
  } else {
    P = E = INFINITY;
    for (int k = 0; k < 3; ++k) { lo[k] = -INFINITY; hi[k] = INFINITY; }
  }
  if (!isfinite(P)) for (int k = 0; k < 3; ++k) { lo[k] = -INFINITY; hi[k] = INFINITY; }
  const long node = (long)n - 1 + j;
  box[node * 2 + 0] = make_float4(lo[0], lo[1], lo[2], P);
  box[node * 2 + 1] = make_float4(hi[0], hi[1], hi[2], E);
  meta[node].x = -(int)(j + 1);
  meta[node].y = 1;
  meta[node].w = 0;
}

__device__ inline int karras_delta(const unsigned long long* __restrict__ k, int n, long i, long j) {
  if (j < 0 || j >= n) return -1;
  const unsigned long long a = k[i], b = k[j];
  return a != b ? __clzll((long long)(a ^ b)) : 64 + __clz((int)(i ^ j));
}

// internal node i of Karras 2012 (Fig. 4): range, split, children, parent pointers, range into counters' spare
__global__ void bvh_hierarchy_kernel(const unsigned long long* __restrict__ keys, int n, int4* __restrict__ meta,
                                     int2* __restrict__ range) {
  const long i = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (i >= n - 1) return;
  const int d = karras_delta(keys, n, i, i + 1) - karras_delta(keys, n, i, i - 1) >= 0 ? 1 : -1;
  const int dmin = karras_delta(keys, n, i, i - d);
  long lmax = 2;
  while (karras_delta(keys, n, i, i + lmax * d) > dmin) lmax *= 2;
  long l = 0;
  for (long t = lmax / 2; t >= 1; t /= 2)
    if (karras_delta(keys, n, i, i + (l + t) * d) > dmin) l += t;
  const long j = i + l * d;
  const int dnode = karras_delta(keys, n, i, j);
  long s = 0, t = l;
  while (t > 1) {
    t = (t + 1) >> 1;
    if (karras_delta(keys, n, i, i + (s + t) * d) > dnode) s += t;
  }
  const long gamma = i + s * d + min(d, 0);
  const long first = min(i, j), last = max(i, j);
  const long left = first == gamma ? (long)n - 1 + gamma : gamma;
  const long right = last == gamma + 1 ? (long)n - 1 + gamma + 1 : gamma + 1;
  meta[i].x = (int)left;
  meta[i].y = (int)right;
  meta[left].z = (int)i;
  meta[right].z = (int)i;
  range[i] = make_int2((int)first, (int)(last - first + 1));
}

// bottom-up refit from every leaf; the second thread to arrive at a node forms it (so both children are final)
__global__ void bvh_refit_kernel(int n, float4* __restrict__ box, int4* __restrict__ meta,
                                 const int2* __restrict__ range, unsigned* __restrict__ arrivals) {
  const long j = blockIdx.x * (long)blockDim.x + threadIdx.x;
  if (j >= n) return;
  int node = n - 1 + (int)j;
  while (node != 0) {
    const int parent = meta[node].z;
    __threadfence();
    if (__hip_atomic_fetch_add(arrivals + parent, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
    const int4 m = meta[parent];
    const float4 a0 = box[(long)m.x * 2], a1 = box[(long)m.x * 2 + 1];
    const float4 b0 = box[(long)m.y * 2], b1 = box[(long)m.y * 2 + 1];
    box[(long)parent * 2] = make_float4(fminf(a0.x, b0.x), fminf(a0.y, b0.y), fminf(a0.z, b0.z), fmaxf(a0.w, b0.w));
    box[(long)parent * 2 + 1] = make_float4(fmaxf(a1.x, b1.x), fmaxf(a1.y, b1.y), fmaxf(a1.z, b1.z), fmaxf(a1.w, b1.w));
    const int2 r = range[parent];
    if (r.y <= kLeafFaces) {
      meta[parent] = make_int4(-(r.x + 1), r.y, m.z, 0);
    } else {
      meta[parent].w = 1 + max(meta[m.x].w, meta[m.y].w);
    }
    node = parent;
  }
}

__global__ void bvh_header_kernel(int n, int* __restrict__ header, const int4* __restrict__ meta) {
  header[0] = kBvhMagic;
  header[1] = n;
  header[2] = n > 0 ? 2 * n - 1 : 0;
  header[3] = n > 0 ? meta[0].w : 0;
  header[4] = 0;
}

static int mesh_bvh_build_f32(const float* verts, const int* faces, int n, void* bvh, void* ws, int* depth_out,
                              hipStream_t stream) {
  const BvhLayout L = bvh_layout(n);
  const WsLayout W = ws_layout(n);
  char* B = (char*)bvh;
  char* S = (char*)ws;
  CTD_HIP_TRY(hipMemsetAsync(bvh, 0, L.total, stream));
  float4* box = (float4*)(B + L.box);
  int4* meta = (int4*)(B + L.meta);
  float4* tris = (float4*)(B + L.tris);
  if (n > 0) {
    unsigned long long* k0 = (unsigned long long*)(S + W.keys0);
    unsigned long long* k1 = (unsigned long long*)(S + W.keys1);
    int* v0 = (int*)(S + W.vals0);
    int* v1 = (int*)(S + W.vals1);
    unsigned* hist = (unsigned*)(S + W.hist);
    unsigned* counters = (unsigned*)(S + W.counters);
    unsigned* bounds = (unsigned*)(S + W.bounds);
    const unsigned init[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    // the initial bounds as six 32-bit fills (no host buffer that would have to outlive the async copy)
    for (int k = 0; k < 6; ++k) CTD_HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(bounds + k), (int)init[k], 1, stream));
    CTD_HIP_TRY(hipMemsetAsync(counters, 0, (size_t)n * 4, stream));
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(bvh_bounds_kernel, dim3((unsigned)min(blocks, 1024)), dim3(256), 0, stream, verts, faces, n, bounds);
    CTD_LAUNCH_CHECK();
    hipLaunchKernelGGL(bvh_morton_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, verts, faces, n, bounds, k0, v0);
    CTD_LAUNCH_CHECK();
    const int tiles = (int)(((long)n + kSortTile - 1) / kSortTile);
    for (int shift = 0; shift < kKeyBits; shift += kDigitBits) {
      hipLaunchKernelGGL(sort_hist_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, stream, k0, n, shift, tiles, hist);
      CTD_LAUNCH_CHECK();
      hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(1024), 0, stream, hist, (long)tiles * kDigits);
      CTD_LAUNCH_CHECK();
      hipLaunchKernelGGL(sort_scatter_kernel, dim3((unsigned)tiles), dim3(kSortThreads), 0, stream, k0, v0, n, shift,
                         tiles, hist, k1, v1);
      CTD_LAUNCH_CHECK();
      std::swap(k0, k1);
      std::swap(v0, v1);
    }
    // 16 passes: the sorted pairs are back in (k0, v0)
    hipLaunchKernelGGL(bvh_leaves_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, verts, faces, n, v0, box, meta,
                       tris);
    CTD_LAUNCH_CHECK();
    if (n > 1) {
      int2* range = (int2*)(S + W.keys1);     // the other key buffer is free now (n * 8 bytes)
      hipLaunchKernelGGL(bvh_hierarchy_kernel, dim3((unsigned)((n - 1 + 255) / 256)), dim3(256), 0, stream, k0, n,
                         meta, range);
      CTD_LAUNCH_CHECK();
      hipLaunchKernelGGL(bvh_refit_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, n, box, meta, range, counters);
      CTD_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(bvh_header_kernel, dim3(1), dim3(1), 0, stream, n, (int*)B, meta);
  CTD_LAUNCH_CHECK();
  int header[16];
  CTD_HIP_TRY(hipMemcpyAsync(header, bvh, sizeof(header), hipMemcpyDeviceToHost, stream));
  CTD_HIP_TRY(hipStreamSynchronize(stream));
  if (depth_out) *depth_out = header[3];
  return header[3] > kMaxDepth ? CTD_ERR_UNSUPPORTED : CTD_OK;
}

// ---------------------------------------------------------------------------------------------------- traversal

// lower_rel, upper_rel, finite3 and prune: ctd_bvh_ray.h

struct Hit {
  float t, u, v;
  int face;
  bool valid;
};

__device__ inline Hit bvh_nearest(const BvhView& bv, int* __restrict__ stack, const float* o, const float* d) {
  Hit h{FLT_MAX, 0.f, 0.f, 0, false};
  if (bv.n == 0) return h;
  const bool exact = finite3(o) && finite3(d);       // non-finite rays visit every face (nothing prunes them)
  const float dn = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) * 1.00001f;
  int sp = 1;
  lane_at(stack, 0) = 0;
  while (sp > 0) {
    const int node = lane_at(stack, --sp);
    if (exact && prune(o, d, dn, bv.box[(long)node * 2], bv.box[(long)node * 2 + 1], h.valid ? h.t : FLT_MAX)) continue;
    const int4 m = bv.meta[node];
    if (m.x < 0) {
      const int first = -(m.x + 1);
      for (int k = 0; k < m.y; ++k) {
        float v0[3], v1[3], v2[3];
        const int f = bvh_leaf_tri(bv, first + k, v0, v1, v2);
        float ft, fu, fv;
        if (ray_tri(o, d, v0, v1, v2, ft, fu, fv) && (ft < h.t || (ft == h.t && h.valid && f < h.face))) {
          h.t = ft;
          h.u = fu;
          h.v = fv;
          h.face = f;
          h.valid = true;
        }
      }
    } else if (sp + 2 <= kStack) {                    // always true for depth <= kMaxDepth (checked at launch)
      lane_at(stack, sp++) = m.y;
      lane_at(stack, sp++) = m.x;
    }
  }
  return h;
}

__device__ inline bool tile_pixel(int width, int height, int& h, int& w) {
  const int lane = threadIdx.x;
  h = blockIdx.y * 8 + lane / 8;
  w = blockIdx.x * 8 + lane % 8;
  return h < height && w < width;
}

__global__ __launch_bounds__(64) void render_proj_bvh_kernel(BvhView bv, const float* __restrict__ verts,
                                                             const float* __restrict__ colors, const int* __restrict__ faces,
                                                             CamDev cam, CamDev proj, float ka, float kd, float ks,
                                                             float alpha, const float* __restrict__ pattern,
                                                             float d_alpha, float d_beta, float* __restrict__ depth,
                                                             float* __restrict__ color, float* __restrict__ normal) {
  int* stack = lane_stack();
  int h, w;
  if (!tile_pixel(cam.width, cam.height, h, w)) return;
  const int idx = h * cam.width + w;
  const float orig[3] = {cam.C[0], cam.C[1], cam.C[2]};
  float dir[3];
  camera_ray(cam, h, w, dir);
  const Hit hit = bvh_nearest(bv, stack, orig, dir);
  if (depth) depth[idx] = hit.valid ? hit.t : -1;
  color[idx * 3 + 0] = 0;
  color[idx * 3 + 1] = 0;
  color[idx * 3 + 2] = 0;
  if (!hit.valid) return;
  float pt[3], pdir[3];
  const float porig[3] = {proj.C[0], proj.C[1], proj.C[2]};
  proj_camera_hit(verts, colors, faces, hit.face, orig, dir, hit.t, hit.u, hit.v, ka, kd, ks, alpha, normal, idx, porig,
                  pt, pdir);
  const Hit ph = bvh_nearest(bv, stack, porig, pdir);     // shadow ray: does the projector see the same point?
  if (!ph.valid) return;
  proj_pattern_fetch(proj, pattern, d_alpha, d_beta, pt, porig, pdir, ph.t, color, idx);
}

__global__ __launch_bounds__(64) void render_mesh_bvh_kernel(BvhView bv, const float* __restrict__ verts,
                                                             const float* __restrict__ colors,
                                                             const float* __restrict__ normals,
                                                             const int* __restrict__ faces, CamDev cam, float ka,
                                                             float kd, float ks, float alpha, float* __restrict__ depth,
                                                             float* __restrict__ color, float* __restrict__ normal) {
  int* stack = lane_stack();
  int h, w;
  if (!tile_pixel(cam.width, cam.height, h, w)) return;
  const int idx = h * cam.width + w;
  const float orig[3] = {cam.C[0], cam.C[1], cam.C[2]};
  float dir[3];
  camera_ray(cam, h, w, dir);
  const Hit hit = bvh_nearest(bv, stack, orig, dir);
  mesh_shade(verts, colors, normals, faces, hit.valid, hit.face, orig, dir, hit.t, hit.u, hit.v, ka, kd, ks, alpha, depth,
             color, normal, idx);
}

static int render_mesh_proj_bvh_f32(const void* bvh, const float* verts, const float* colors, const int* faces,
                                    int n_faces, const float* cam_p, int cam_w, int cam_h, const float* proj_p,
                                    int proj_w, int proj_h, const float* shader, const float* pattern, float d_alpha,
                                    float d_beta, float* depth, float* color, float* normal, hipStream_t stream) {
  const int st = bvh_check(bvh, n_faces, stream);
  if (st != CTD_OK) return st;
  const CamDev cam = make_cam(cam_p, cam_w, cam_h), proj = make_cam(proj_p, proj_w, proj_h);
  const dim3 grid((unsigned)ceil_div(cam_w, 8), (unsigned)ceil_div(cam_h, 8));
  hipLaunchKernelGGL(render_proj_bvh_kernel, grid, dim3(64), 0, stream, bvh_view(bvh, n_faces), verts, colors, faces, cam,
                     proj, shader[0], shader[1], shader[2], shader[3], pattern, d_alpha, d_beta, depth, color, normal);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

static int render_mesh_bvh_f32(const void* bvh, const float* verts, const float* colors, const float* normals,
                               const int* faces, int n_faces, const float* cam_p, int cam_w, int cam_h,
                               const float* shader, float* depth, float* color, float* normal, hipStream_t stream) {
  const int st = bvh_check(bvh, n_faces, stream);
  if (st != CTD_OK) return st;
  const CamDev cam = make_cam(cam_p, cam_w, cam_h);
  const dim3 grid((unsigned)ceil_div(cam_w, 8), (unsigned)ceil_div(cam_h, 8));
  hipLaunchKernelGGL(render_mesh_bvh_kernel, grid, dim3(64), 0, stream, bvh_view(bvh, n_faces), verts, colors, normals,
                     faces, cam, shader[0], shader[1], shader[2], shader[3], depth, color, normal);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_mesh_bvh_bytes(int n_faces) {
  return n_faces < 0 || n_faces > kBvhMaxFaces ? 0 : mesh_bvh_bytes(n_faces);
}

size_t ctd_mesh_bvh_workspace_bytes(int n_faces) {
  return n_faces < 0 || n_faces > kBvhMaxFaces ? 0 : mesh_bvh_workspace_bytes(n_faces);
}

int ctd_mesh_bvh_build_f32(const float* verts, int n_verts, const int* faces, int n_faces, void* bvh, size_t bvh_bytes,
                           void* workspace, size_t workspace_bytes, int* depth, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > kBvhMaxFaces || !bvh) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && (!verts || !faces || !workspace || n_verts == 0)) return CTD_ERR_INVALID_ARG;
  if ((uintptr_t)bvh % 16 || (uintptr_t)workspace % 16) return CTD_ERR_INVALID_ARG;
  if (bvh_bytes < mesh_bvh_bytes(n_faces)) return CTD_ERR_INVALID_ARG;
  if (workspace_bytes < mesh_bvh_workspace_bytes(n_faces)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_bvh_build_f32(verts, faces, n_faces, bvh, workspace, depth, (hipStream_t)stream);
}

int ctd_render_mesh_proj_bvh_f32(const void* bvh, const float* verts, const float* colors, int n_verts, const int* faces,
                                 int n_faces, const float* cam, int cam_width, int cam_height, const float* proj,
                                 int proj_width, int proj_height, const float* shader, const float* pattern,
                                 float d_alpha, float d_beta, float* depth, float* color, float* normal, int device,
                                 void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > kBvhMaxFaces || cam_width <= 0 || cam_height <= 0 || proj_width <= 0 ||
      proj_height <= 0 || (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!bvh || (uintptr_t)bvh % 16 || !cam || !proj || !shader || !pattern || !color ||
      (n_faces > 0 && (!verts || !colors || !faces)))
    return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_proj_bvh_f32(bvh, verts, colors, faces, n_faces, cam, cam_width, cam_height, proj, proj_width,
                                  proj_height, shader, pattern, d_alpha, d_beta, depth, color, normal, (hipStream_t)stream);
}

int ctd_render_mesh_bvh_f32(const void* bvh, const float* verts, const float* colors, const float* normals, int n_verts,
                            const int* faces, int n_faces, const float* cam, int cam_width, int cam_height,
                            const float* shader, float* depth, float* color, float* normal, int device, void* stream) {
  if (n_verts < 0 || n_faces < 0 || n_faces > kBvhMaxFaces || cam_width <= 0 || cam_height <= 0 ||
      (double)cam_width * cam_height * 3 >= 2147483648.0)
    return CTD_ERR_INVALID_ARG;
  if (!bvh || (uintptr_t)bvh % 16 || !cam || !shader || (n_faces > 0 && (!verts || !faces))) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && ((color && !colors) || ((color || normal) && !normals))) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return render_mesh_bvh_f32(bvh, verts, colors, normals, faces, n_faces, cam, cam_width, cam_height, shader, depth,
                             color, normal, (hipStream_t)stream);
}

}  // extern "C"
