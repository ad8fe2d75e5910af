// point_mesh.hip -- for every query point the nearest face of a triangle mesh: squared distance, face index, closest
// point (include/ctd_hip_mesh_dist.h).  Two kernels, one answer: the brute-force kernel is the definition, the
// traversal of the ray casters' BVH (render_bvh.hip, ctd_bvh.h) gives its bits.  The same point_tri (ctd_point_tri.h)
// computes every candidate; the tree only skips faces that provably cannot be the answer.
//
// Selection.  The answer is the face of smallest d2 among those whose d2 compares < +inf, the lowest index among equal
// d2.  Brute force streams the faces in index order and replaces on d2 < best; the traversal replaces on d2 < best, or
// d2 == best with a lower index.  That is order independent, so any visiting order yields brute force's face, d2 and
// closest point -- provided no face whose computed d2 is <= best is pruned.  One lane owns one point: no atomics, no
// flags, the same bits on every run.
//
// Why pruning is safe (forward-error bound of point_tri as coded; u = 2^-24, all norms Euclidean).
//   Face a, b, c (floats), ab = fl(b-a), ac = fl(c-a): |ab_k - (b-a)_k| <= u |(b-a)_k|, the same for ac.  A vertex
//   region returns the vertex: a point of the triangle T, error 0.  Otherwise q_k = fl(fl(a_k + fl(s ab_k)) +
//   fl(t ac_k)) with floats 0 <= s <= 1, 0 <= t <= m = fl(1-s) <= (1-s) + u (the clamp; a NaN parameter became 0).
//   Four roundings: |q_k - (a_k + s ab_k + t ac_k)| <= 3.01u (|a_k| + |ab_k| + |ac_k|).  With t' = min(t, 1-s),
//   |t - t'| <= u, the point x = a + s (b-a) + t' (c-a) is a convex combination of a, b, c, so x lies in T, and
//   |(a_k + s ab_k + t ac_k) - x_k| <= s u |(b-a)_k| + t u |(c-a)_k| + u |(c-a)_k| <= 1.01u (|ab_k| + 2 |ac_k|).
//   Together, componentwise and therefore in norm:
//     |q - x| <= 5.1u (|a| + |ab| + |ac|) =: eta.                                                         (1)
//   Then d_k = fl(p_k - q_k) = (p_k - q_k)(1 + e), |e| <= u, and d2 = fl(fl(dx dx + dy dy) + dz dz) is a sum of
//   non-negative terms with at most three roundings each: d2 >= |p - q|^2 (1-u)^5 unless a product underflows, so
//     sqrt(d2) >= (1 - 2.6u) |p - q| >= (1 - 2.6u) (dist(p, T) - eta)   whenever dist(p, T) - eta >= 1e-18            (2)
//   (then the largest |d_k|^2 is >= 3e-37, a normal number, and the other terms only add).  This holds whatever region
//   the rounded tests chose, for zero-area faces too: (1) uses the clamp alone, not the classification.
//   Per node: the box is the exact union of its faces' vertex boxes, so T lies inside it and dist(p, T) >= dist(p, box);
//   |a| <= M1 = sum_k max(|lo_k|, |hi_k|) (an l1 norm, >= the Euclidean one) and |ab|, |ac| <= E, the node's largest
//   edge length rounded up by 1e-5 relative (render_bvh.hip's E), so eta <= 5.1u (M1 + 2E) = 3.04e-7 (M1 + 2E).
//   The kernel takes g_k = max(lo_k - p_k, p_k - hi_k, 0) (each difference one rounding, never rounded away from a
//   non-zero value to a larger one by more than u), D = sqrtf(g.g) (1 - 1e-6) <= dist(p, box), slack = 1e-6 (M1 + 2E) +
//   1e-18 (3.3 times eta, which also pays for the roundings of the slack itself), L = (D - slack)(1 - 2e-6), and prunes
//   the node only if L > 0 and fl(L L) > best.  By (2) every face under the node then has d2 >= L^2 (1 + u) >= fl(L L)
//   > best: it can neither beat the best nor tie with it.  Being generous with the slack costs visits, not correctness.
//   Every comparison is written so that NaN means "do not prune".  A point with a non-finite coordinate prunes nothing:
//   it visits every face, like brute force.  Faces with a non-finite vertex, or whose edge product overflows, have an
//   infinite box and E = inf (the builder's rule): g = 0, slack = inf, never pruned.  While best is +inf (no face has
//   qualified yet) nothing is pruned, since nothing compares > +inf.
//
// How far sqrt(d2) is from the true distance (what tests/pointmesh_ref.forward_bound evaluates; not needed for pruning).
//   Below: min over faces of sqrt(d2) >= (1 - 2.6u) (dist(p, mesh) - max_f eta_f) by (2).  Above: for the truly nearest
//   face f*, |p - q| <= dist(p, T) + |q - x*| with x* the true closest point, and to first order the parameters carry
//   |ds|, |dt| <= 94u E^2 R^2 / (4 A^2) in the interior (the d_i are 3-term dot products of rounded differences, error
//   <= 5.1u E R each; va, vb, vc differences of two products of them, <= 23u E^2 R^2; their sum 4 A^2, <= 71u E^2 R^2)
//   and <= 16u E R / e^2 on an edge of length e, where E = max(|ab|, |ac|), R = max(|p-a|, |p-b|, |p-c|), A the area:
//     sqrt(d2) <= (1 + 2.6u) (dist(p, T) + eta + 47.5u E^3 R^2 / A^2 + 16u E R / e_min).                   (3)
//   (3) degrades with slivers and with distance; (2) does not.  Pruning rests on (2) only.
//
// Traversal: one wave of 64 points per workgroup, one point per lane, a per-lane stack in LDS (kStack entries, lane-
// interleaved so that a wave's accesses fall on 64 different banks).  At an inner node both children's bounds are
// computed; the nearer one is visited next (straight away, its bound is still current), the farther one is pushed and
// tested again when it is popped, because the best has usually tightened by then.  At most one push per level, so the
// stack never holds more than the tree's depth (checked at launch against kMaxDepth; the push is bounds-checked too).
//
// Brute force: 256 points per workgroup, one per lane; the faces stream through LDS in tiles of 256 in index order
// (each thread gathers one face's vertices, every lane then reads the same face: a broadcast).  Faces with an index
// outside [0, n_verts) are marked in the tile and skipped; their vertices are never dereferenced.
#include <cfloat>
#include <cstdint>

#include "../../include/ctd_hip_mesh_dist.h"
#include "ctd_bvh.h"
#include "ctd_common.h"
#include "ctd_mesh_query.h"
#include "ctd_point_tri.h"

namespace ctd {

constexpr int kBruteThreads = 256;

struct Nearest {
  float d2, q[3];
  int face;
};

__device__ inline Nearest nearest_none() {
  const float nan = __int_as_float(0x7fc00000);
  return Nearest{INFINITY, {nan, nan, nan}, -1};
}

__device__ inline void nearest_store(const Nearest& b, long i, float* __restrict__ d2, int* __restrict__ face,
                                     float* __restrict__ closest) {
  d2[i] = b.d2;
  face[i] = b.face;
  if (closest) {
    closest[i * 3 + 0] = b.q[0];
    closest[i * 3 + 1] = b.q[1];
    closest[i * 3 + 2] = b.q[2];
  }
}

__global__ __launch_bounds__(kBruteThreads) void point_mesh_brute_kernel(const float* __restrict__ points, int n_points,
                                                                         const float* __restrict__ verts, int n_verts,
                                                                         const int* __restrict__ faces, int n_faces,
                                                                         float* __restrict__ d2, int* __restrict__ face,
                                                                         float* __restrict__ closest) {
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
      if (r.d2 < best.d2) {                            // faces come in index order: the first of equal d2 stays
        best.d2 = r.d2;
        best.q[0] = r.q[0]; best.q[1] = r.q[1]; best.q[2] = r.q[2];
        best.face = base + k;
      }
    }
  }
  if (live) nearest_store(best, i, d2, face, closest);
}

// the squared lower bound of the header comment for the faces under a node with this box, or -1 when the node must not
// be pruned (NaN anywhere ends there too)
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

__global__ __launch_bounds__(64) void point_mesh_bvh_kernel(BvhView bv, const float* __restrict__ points, int n_points,
                                                            float* __restrict__ d2, int* __restrict__ face,
                                                            float* __restrict__ closest) {
  int* stack = lane_stack();
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= n_points) return;
  const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
  const bool exact = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);   // otherwise: visit every face
  Nearest best = nearest_none();
  int sp = 0, cur = bv.n > 0 ? 0 : -1;
  while (true) {
    if (cur < 0) {                                     // pop until a node survives the best as it is now
      while (sp > 0) {
        const int cand = lane_at(stack, --sp);
        if (exact && node_bound2(p, bv.box[(long)cand * 2], bv.box[(long)cand * 2 + 1]) > best.d2) continue;
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
        if (r.d2 < best.d2 || (r.d2 == best.d2 && f < best.face)) {
          best.d2 = r.d2;
          best.q[0] = r.q[0]; best.q[1] = r.q[1]; best.q[2] = r.q[2];
          best.face = f;
        }
      }
      cur = -1;
      continue;
    }
    float bl = -1.f, br = -1.f;
    if (exact) {
      bl = node_bound2(p, bv.box[(long)m.x * 2], bv.box[(long)m.x * 2 + 1]);
      br = node_bound2(p, bv.box[(long)m.y * 2], bv.box[(long)m.y * 2 + 1]);
    }
    const bool keep_l = !(bl > best.d2), keep_r = !(br > best.d2);
    if (keep_l && keep_r) {
      const bool right_first = br < bl;
      if (sp < kStack) lane_at(stack, sp++) = right_first ? m.x : m.y;        // always true for depth <= kMaxDepth
      cur = right_first ? m.y : m.x;
    } else {
      cur = keep_l ? m.x : (keep_r ? m.y : -1);
    }
  }
  nearest_store(best, i, d2, face, closest);
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_point_mesh_distance_f32(const float* points, int n_points, const float* verts, int n_verts, const int* faces,
                                int n_faces, const void* bvh, float* d2, int* face, float* closest, int device,
                                void* stream) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0) return CTD_ERR_INVALID_ARG;
  if ((double)n_points * 3 >= 2147483648.0 || n_faces > kBvhMaxFaces) return CTD_ERR_INVALID_ARG;
  if (n_points > 0 && (!points || !d2 || !face)) return CTD_ERR_INVALID_ARG;
  if (!mesh_group_ok(verts, n_verts, faces, n_faces, bvh)) return CTD_ERR_INVALID_ARG;
  if (n_points == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t s = (hipStream_t)stream;
  return tree_or_brute(
      bvh, n_faces, s,
      [&](const BvhView& bv) {
        hipLaunchKernelGGL(point_mesh_bvh_kernel, dim3((unsigned)ceil_div(n_points, 64)), dim3(64), 0, s, bv, points,
                           n_points, d2, face, closest);
      },
      [&] {
        hipLaunchKernelGGL(point_mesh_brute_kernel, dim3((unsigned)ceil_div(n_points, kBruteThreads)),
                           dim3(kBruteThreads), 0, s, points, n_points, verts, n_verts, faces, n_faces, d2, face, closest);
      });
}

}  // extern "C"
