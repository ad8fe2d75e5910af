// ctd_mesh_query.h -- what point_mesh.hip, mesh_color.hip and render_bvh.hip share: the face tile of the brute-force
// kernels, the leaf fetch and the per-lane stack of the tree traversals (ctd_bvh.h), the host's choice between tree and
// brute force.  Not the loops: closest hit (a tightening limit), any hit (a constant one) and nearest face (the nearer
// child first) differ for a reason.
#pragma once

#include <cstdint>

#include "ctd_bvh.h"
#include "ctd_common.h"

namespace ctd {

// One tile of a brute-force kernel, by a workgroup of kThreads: thread tid gathers the vertices of face base + tid into
// tri[tid * 9 ..] (v0, v1, v2) and sets ok[tid] when the face exists and its three indices lie in [0, n_verts); the
// vertices of any other face are never dereferenced.  The barriers around the call are the caller's.
template <int kThreads>
__device__ inline void face_tile_load(float (&tri)[kThreads * 9], int (&ok)[kThreads], int base,
                                      const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
                                      int n_faces) {
  const int tid = threadIdx.x;
  const int j = base + tid;
  int valid = 0;
  if (j < n_faces) {
    const int i0 = faces[(long)j * 3], i1 = faces[(long)j * 3 + 1], i2 = faces[(long)j * 3 + 2];
    valid = i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts;
    if (valid) {
      const float *a = verts + (long)i0 * 3, *b = verts + (long)i1 * 3, *c = verts + (long)i2 * 3;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        tri[tid * 9 + k] = a[k];
        tri[tid * 9 + 3 + k] = b[k];
        tri[tid * 9 + 6 + k] = c[k];
      }
    }
  }
  ok[tid] = valid;
}

// sorted face i of the tree -> its vertices and its index in the mesh
__device__ inline int bvh_leaf_tri(const BvhView& bv, int i, float* v0, float* v1, float* v2) {
  const float4 a = bv.tris[(long)i * 3], b = bv.tris[(long)i * 3 + 1], c = bv.tris[(long)i * 3 + 2];
  v0[0] = a.x; v0[1] = a.y; v0[2] = a.z;
  v1[0] = b.x; v1[1] = b.y; v1[2] = b.z;
  v2[0] = c.x; v2[1] = c.y; v2[2] = c.z;
  return __float_as_int(a.w);
}

// The traversal stack of one lane: kStack entries in the LDS of a workgroup of one wave, lane-interleaved (entry e of
// lane l at e * 64 + l) so that a wave's accesses fall on 64 different banks.  lane_stack() is the lane's entry 0;
// lane_at(stack, sp++) = node pushes, lane_at(stack, --sp) pops: sp and the guards against kStack stay with the caller.
__device__ __forceinline__ int* lane_stack() {
  __shared__ int lds[kStack * 64];
  return lds + threadIdx.x;
}
__device__ inline int& lane_at(int* stack, int e) { return stack[e * 64]; }

// the pointer checks every entry point makes of its (verts, n_verts, faces, n_faces, bvh) group; the face limit is the
// entry point's own, because the status it answers with differs
static inline bool mesh_group_ok(const void* verts, int n_verts, const void* faces, int n_faces, const void* bvh) {
  return !(n_faces > 0 && (!faces || (n_verts > 0 && !verts))) && !(bvh && (uintptr_t)bvh % 16);
}

// With a tree and faces for it to hold: the header check, its error, else tree(view) launches the traversal; without:
// brute() launches brute force.  Both callables only launch.
template <class Tree, class Brute>
static int tree_or_brute(const void* bvh, int n_faces, hipStream_t stream, Tree tree, Brute brute) {
  if (bvh && n_faces > 0) {
    const int st = bvh_check(bvh, n_faces, stream);
    if (st != CTD_OK) return st;
    tree(bvh_view(bvh, n_faces));
  } else {
    brute();
  }
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd
