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
//
// The two kernels live in ctd_point_mesh_nearest.h, templates that mesh_sdf.hip instantiates too (with a cutoff and the
// recorded branch); this file instantiates them without either, which is the code that stood here.
#include <cfloat>
#include <cstdint>

#include "../../include/ctd_hip_mesh_dist.h"
#include "ctd_point_mesh_nearest.h"

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
  return nearest_launch<false, false>(points, n_points, verts, n_verts, faces, n_faces, bvh, INFINITY, d2, face, closest,
                                      nullptr, (hipStream_t)stream);
}

}  // extern "C"
