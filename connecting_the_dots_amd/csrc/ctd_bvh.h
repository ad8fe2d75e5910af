// ctd_bvh.h -- the buffer of ctd_mesh_bvh_build_f32 as its readers see it: the layout of its sections, a view of them
// for kernels, and the header check every traversal makes before it launches.  Three files read the buffer: the ray
// casters (render_bvh.hip, which also builds the tree and documents the format), the nearest-face query (point_mesh.hip)
// and the view colours' occlusion query (mesh_color.hip); what their traversals share beyond it is in ctd_mesh_query.h.
#pragma once

#include "ctd_common.h"

namespace ctd {

constexpr int kBvhMaxFaces = 1 << 28;
constexpr int kStack = 64;          // per-lane traversal stack (LDS), entries
constexpr int kMaxDepth = kStack - 2;
constexpr int kBvhMagic = 0x42445443;   // "CTDB"

static inline size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }

struct BvhLayout {
  size_t box, meta, tris, total;
};
static BvhLayout bvh_layout(long n) {
  const long nodes = n > 0 ? 2 * n - 1 : 0;
  BvhLayout L;
  L.box = 64;
  L.meta = L.box + align16((size_t)nodes * 32);
  L.tris = L.meta + align16((size_t)nodes * 16);
  L.total = L.tris + align16((size_t)n * 48);
  return L;
}

struct BvhView {
  const float4* box;
  const int4* meta;
  const float4* tris;
  int n, n_nodes;
};

static BvhView bvh_view(const void* bvh, int n) {
  const BvhLayout L = bvh_layout(n);
  const char* B = (const char*)bvh;
  return BvhView{(const float4*)(B + L.box), (const int4*)(B + L.meta), (const float4*)(B + L.tris), n,
                 n > 0 ? 2 * n - 1 : 0};
}

// reads the tree's header (one small synchronous copy) and refuses a buffer that is not a tree of n faces or is
// deeper than the traversal stack
static int bvh_check(const void* bvh, int n, hipStream_t stream) {
  int header[16];
  CTD_HIP_TRY(hipMemcpyAsync(header, bvh, sizeof(header), hipMemcpyDeviceToHost, stream));
  CTD_HIP_TRY(hipStreamSynchronize(stream));
  if (header[0] != kBvhMagic || header[1] != n) return CTD_ERR_INVALID_ARG;
  if (header[3] < 0 || header[3] > kMaxDepth) return CTD_ERR_UNSUPPORTED;
  return CTD_OK;
}

}  // namespace ctd
