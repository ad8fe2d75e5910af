// ctd_point_mesh_nearest.h -- the one copy of the nearest-face loops: the brute-force kernel and the traversal of the
// mesh BVH, which point_mesh.hip (include/ctd_hip_mesh_dist.h) and mesh_sdf.hip (include/ctd_hip_mesh_sdf.h) both
// instantiate.  The selection rule, the forward-error argument that makes pruning safe, and the shape of the two
// kernels are derived in point_mesh.hip's header comment; this file only holds the code.
//
// Three compile-time switches, none of which changes a bit of d2, face or closest where it is off:
//   kCutoff  a face qualifies only when its d2 compares <= max_d2 (and < +inf, as always).  The tree prunes a node when
//            its bound exceeds min(best d2, max_d2): by (2) of point_mesh.hip every face under such a node has
//            d2 >= fl(L L) > max_d2, so none of them can qualify, and the argument for the best d2 is as before.  With
//            max_d2 = +inf the comparison d2 <= max_d2 holds for every d2 that is not NaN (which d2 < best fails
//            already) and min(best, +inf) = best: the answer is the uncut one, bit for bit.
//   kBranch  the branch that point_tri took for the winning face (PointTri::region) is stored as int8 in `feature`,
//            -1 where no face qualifies.
//   kHint    `hint` int32 [n_points] (NULL: none) names the face each point had last time (mesh_register.hip feeds a
//            round's answer to the next).  A hint h is used when 0 <= h < n_faces and the three vertex indices of face h
//            lie in [0, n_verts); any other value is ignored and nothing is dereferenced through it.  Before the traversal
//            starts, point_tri is evaluated on face h, and if its d2 qualifies (< +inf, and <= max_d2 under a cutoff) the
//            traversal starts from that face as `best` instead of nearest_none().  Nothing else changes.
//            The result is the unhinted one bit for bit, for any hint whatever.  A hinted face is a real candidate: a
//            face of the mesh that brute force visits too, evaluated by the same point_tri on the same vertex bits (the
//            tree's leaves hold copies of them), and taken only if it qualifies.  The selection keeps the smallest d2 and
//            the lowest index among equals (r.d2 == best.d2 && f < best.face), which does not depend on the order in
//            which candidates arrive, so starting from one of them is one more visiting order.  And a node is pruned
//            only when its bound exceeds the limit, min(best d2, max_d2): by (2) of point_mesh.hip every face under it
//            then has d2 > best d2 strictly, so a face of equal d2 and lower index than the hinted one is never under a
//            pruned node and is still reached.  A good hint only makes the limit tight from the first node on.
//            The brute-force kernel takes the switch and ignores the hint: it visits every face anyway.
#pragma once

#include <cstdint>

#include "ctd_bvh.h"
#include "ctd_common.h"
#include "ctd_mesh_query.h"
#include "ctd_point_tri.h"

namespace ctd {

constexpr int kBruteThreads = 256;

struct Nearest {
  float d2, q[3];
  int face, region;
};

__device__ inline Nearest nearest_none() {
  const float nan = __int_as_float(0x7fc00000);
  return Nearest{INFINITY, {nan, nan, nan}, -1, -1};
}

__device__ inline void nearest_take(Nearest& best, const PointTri& r, int f) {
  best.d2 = r.d2;
  best.q[0] = r.q[0]; best.q[1] = r.q[1]; best.q[2] = r.q[2];
  best.face = f;
  best.region = r.region;
}

template <bool kBranch>
__device__ inline void nearest_store(const Nearest& b, long i, float* __restrict__ d2, int* __restrict__ face,
                                     float* __restrict__ closest, int8_t* __restrict__ feature) {
  d2[i] = b.d2;
  face[i] = b.face;
  if (closest) {
    closest[i * 3 + 0] = b.q[0];
    closest[i * 3 + 1] = b.q[1];
    closest[i * 3 + 2] = b.q[2];
  }
  if (kBranch) feature[i] = (int8_t)b.region;
}

template <bool kCutoff, bool kBranch, bool kHint>
__global__ __launch_bounds__(kBruteThreads) void point_mesh_brute_kernel(const float* __restrict__ points, int n_points,
                                                                         const float* __restrict__ verts, int n_verts,
                                                                         const int* __restrict__ faces, int n_faces,
                                                                         float max_d2, float* __restrict__ d2,
                                                                         int* __restrict__ face, float* __restrict__ closest,
                                                                         int8_t* __restrict__ feature) {
  __shared__ float tri[kBruteThreads * 9];
  __shared__ int ok[kBruteThreads];
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * kBruteThreads + tid;
  const bool live = i < n_points;
  float p[3] = {0.f, 0.f, 0.f};
  if (live) { p[0] = points[i * 3]; p[1] = points[i * 3 + 1]; p[2] = points[i * 3 + 2]; }
  Nearest best = nearest_none();
  for (int base = 0; base < n_faces; base += kBruteThreads) {
    __syncthreads();                                   // the previous tile has been read by every lane
    face_tile_load<kBruteThreads>(tri, ok, base, verts, n_verts, faces, n_faces);
    __syncthreads();
    if (!live) continue;
    const int cnt = min(kBruteThreads, n_faces - base);
    for (int k = 0; k < cnt; ++k) {
      if (!ok[k]) continue;
      const PointTri r = point_tri(p, tri + k * 9, tri + k * 9 + 3, tri + k * 9 + 6);
      if (r.d2 < best.d2 && (!kCutoff || r.d2 <= max_d2))   // faces come in index order: the first of equal d2 stays
        nearest_take(best, r, base + k);
    }
  }
  if (live) nearest_store<kBranch>(best, i, d2, face, closest, feature);
}

// the squared lower bound of point_mesh.hip's header comment for the faces under a node with this box, or -1 when the
// node must not be pruned (NaN anywhere ends there too)
__device__ inline float node_bound2(const float* p, float4 b0, float4 b1) {
  const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
  float g2 = 0.f, m1 = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    float g = lo[k] - p[k];
    const float h = p[k] - hi[k];
    g = g > h ? g : h;
    g = g > 0.f ? g : 0.f;
    g2 += g * g;
    m1 += fmaxf(fabsf(lo[k]), fabsf(hi[k]));
  }
  const float D = sqrtf(g2) * (1.f - 1e-6f);
  const float slack = 1e-6f * (m1 + 2.f * b1.w) + 1e-18f;
  const float L = (D - slack) * (1.f - 2e-6f);
  return L > 0.f ? L * L : -1.f;
}

// what a node's bound is compared with: the best d2 so far, and under a cutoff never more than max_d2 (not a NaN)
template <bool kCutoff>
__device__ __forceinline__ float prune_limit(float best_d2, float max_d2) {
  return kCutoff && max_d2 < best_d2 ? max_d2 : best_d2;
}

// verts, n_verts, faces and hint are read under kHint only
template <bool kCutoff, bool kBranch, bool kHint>
__global__ __launch_bounds__(64) void point_mesh_bvh_kernel(BvhView bv, const float* __restrict__ points, int n_points,
                                                            const float* __restrict__ verts, int n_verts,
                                                            const int* __restrict__ faces, const int* __restrict__ hint,
                                                            float max_d2, float* __restrict__ d2, int* __restrict__ face,
                                                            float* __restrict__ closest, int8_t* __restrict__ feature) {
  int* stack = lane_stack();
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_points) return;
  const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
  const bool exact = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);   // otherwise: visit every face
  Nearest best = nearest_none();
  if (kHint && hint) {
    const int h = hint[i];
    if (h >= 0 && h < bv.n) {                          // (bv.n is n_faces)
      const int i0 = faces[(long)h * 3], i1 = faces[(long)h * 3 + 1], i2 = faces[(long)h * 3 + 2];
      if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {
        const PointTri r = point_tri(p, verts + (long)i0 * 3, verts + (long)i1 * 3, verts + (long)i2 * 3);
        if (r.d2 < best.d2 && (!kCutoff || r.d2 <= max_d2)) nearest_take(best, r, h);
      }
    }
  }
  int sp = 0, cur = bv.n > 0 ? 0 : -1;
  while (true) {
    if (cur < 0) {                                     // pop until a node survives the best as it is now
      while (sp > 0) {
        const int cand = lane_at(stack, --sp);
        if (exact && node_bound2(p, bv.box[(long)cand * 2], bv.box[(long)cand * 2 + 1]) > prune_limit<kCutoff>(best.d2, max_d2))
          continue;
        cur = cand;
        break;
      }
      if (cur < 0) break;
    }
    const int4 m = bv.meta[cur];
    if (m.x < 0) {
      const int first = -(m.x + 1);
      for (int k = 0; k < m.y; ++k) {
        float v0[3], v1[3], v2[3];
        const int f = bvh_leaf_tri(bv, first + k, v0, v1, v2);
        const PointTri r = point_tri(p, v0, v1, v2);
        if ((r.d2 < best.d2 || (r.d2 == best.d2 && f < best.face)) && (!kCutoff || r.d2 <= max_d2)) nearest_take(best, r, f);
      }
      cur = -1;
      continue;
    }
    float bl = -1.f, br = -1.f;
    if (exact) {
      bl = node_bound2(p, bv.box[(long)m.x * 2], bv.box[(long)m.x * 2 + 1]);
      br = node_bound2(p, bv.box[(long)m.y * 2], bv.box[(long)m.y * 2 + 1]);
    }
    const float lim = prune_limit<kCutoff>(best.d2, max_d2);
    const bool keep_l = !(bl > lim), keep_r = !(br > lim);
    if (keep_l && keep_r) {
      const bool right_first = br < bl;
      if (sp < kStack) lane_at(stack, sp++) = right_first ? m.x : m.y;        // always true for depth <= kMaxDepth
      cur = right_first ? m.y : m.x;
    } else {
      cur = keep_l ? m.x : (keep_r ? m.y : -1);
    }
  }
  nearest_store<kBranch>(best, i, d2, face, closest, feature);
}

// the launches of the two kernels behind tree_or_brute, for both entry points
template <bool kCutoff, bool kBranch, bool kHint = false>
static int nearest_launch(const float* points, int n_points, const float* verts, int n_verts, const int* faces, int n_faces,
                          const void* bvh, float max_d2, float* d2, int* face, float* closest, int8_t* feature, hipStream_t s,
                          const int* hint = nullptr) {
  return tree_or_brute(
      bvh, n_faces, s,
      [&](const BvhView& bv) {
        hipLaunchKernelGGL((point_mesh_bvh_kernel<kCutoff, kBranch, kHint>), dim3((unsigned)ceil_div(n_points, 64)), dim3(64), 0,
                           s, bv, points, n_points, verts, n_verts, faces, hint, max_d2, d2, face, closest, feature);
      },
      [&] {
        hipLaunchKernelGGL((point_mesh_brute_kernel<kCutoff, kBranch, kHint>), dim3((unsigned)ceil_div(n_points, kBruteThreads)),
                           dim3(kBruteThreads), 0, s, points, n_points, verts, n_verts, faces, n_faces, max_d2, d2, face, closest,
                           feature);
      });
}

}  // namespace ctd
