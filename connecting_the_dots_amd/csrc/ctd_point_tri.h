// ctd_point_tri.h -- the one function that computes the distance from a point to a triangle for both kernels of
// point_mesh.hip (brute force and BVH traversal).  Keeping one copy is what makes the two paths give the same bits: the
// tree only changes which faces reach point_tri, never what it computes for them.  The rule it implements is stated in
// include/ctd_hip_mesh_dist.h and restated operation for operation in tests/pointmesh_ref.py.
//
// f32 throughout, one IEEE operation per operator in the order written (the library is built with -ffp-contract=off and
// nothing here calls fmaf), every sum associated as the parentheses say.  The classification is Ericson's
// closest-point-on-triangle (Real-Time Collision Detection, 5.1.5): the three vertex regions, the three edge regions,
// the interior, tested in the order A, B, AB, C, AC, BC.  A vertex region returns that vertex itself, so a query point
// that is a vertex of the face has d2 == 0 exactly.  Every other region returns q = (a + s * ab) + t * ac with
// ab = b - a, ac = c - a as computed, after the clamp 0 <= s <= 1, 0 <= t <= 1 - s (each clamp a comparison that a NaN
// fails, so a NaN parameter becomes 0): whatever rounding did to the region tests, q is a convex combination of a,
// a + ab and a + ac up to the rounding of that one expression.  point_mesh.hip derives its pruning bound from this.
// `region` records the branch that was taken, for the signed query (include/ctd_hip_mesh_sdf.h), which must not
// reclassify from the clamped parameters; a caller that ignores it pays nothing, and d2 and q do not depend on it.
#pragma once

#include "ctd_common.h"

namespace ctd {

struct PointTri {
  float d2;
  float q[3];
  int region;   // the branch taken: 0, 1, 2 vertex a, b, c; 3, 4, 5 edge ab, ac, bc; 6 the interior
};

__host__ __device__ inline float pt_dot(const float* u, const float* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__host__ __device__ inline PointTri point_tri(const float* p, const float* a, const float* b, const float* c) {
  const float ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]};
  const float ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float ap[3] = {p[0] - a[0], p[1] - a[1], p[2] - a[2]};
  const float bp[3] = {p[0] - b[0], p[1] - b[1], p[2] - b[2]};
  const float cp[3] = {p[0] - c[0], p[1] - c[1], p[2] - c[2]};
  const float d1 = pt_dot(ab, ap), d2 = pt_dot(ac, ap);
  const float d3 = pt_dot(ab, bp), d4 = pt_dot(ac, bp);
  const float d5 = pt_dot(ab, cp), d6 = pt_dot(ac, cp);
  const float vc = d1 * d4 - d3 * d2;
  const float vb = d5 * d2 - d1 * d6;
  const float va = d3 * d6 - d5 * d4;
  const float e43 = d4 - d3, e56 = d5 - d6;
  PointTri r;
  int vertex = -1;                 // 0, 1, 2: the closest point is a, b, c itself
  float s = 0.f, t = 0.f;
  if (d1 <= 0.f && d2 <= 0.f) {
    vertex = 0;
    r.region = 0;
  } else if (d3 >= 0.f && d4 <= d3) {
    vertex = 1;
    r.region = 1;
  } else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) {
    s = d1 / (d1 - d3);
    r.region = 3;
  } else if (d6 >= 0.f && d5 <= d6) {
    vertex = 2;
    r.region = 2;
  } else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) {
    t = d2 / (d2 - d6);
    r.region = 4;
  } else if (va <= 0.f && e43 >= 0.f && e56 >= 0.f) {
    t = e43 / (e43 + e56);
    s = 1.f - t;
    r.region = 5;
  } else {
    const float inv = 1.f / ((va + vb) + vc);
    s = vb * inv;
    t = vc * inv;
    r.region = 6;
  }
  s = s > 0.f ? s : 0.f;
  s = s < 1.f ? s : 1.f;
  t = t > 0.f ? t : 0.f;
  const float m = 1.f - s;
  t = t < m ? t : m;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float mix = (a[k] + s * ab[k]) + t * ac[k];
    r.q[k] = vertex == 0 ? a[k] : (vertex == 1 ? b[k] : (vertex == 2 ? c[k] : mix));
  }
  const float dx = p[0] - r.q[0], dy = p[1] - r.q[1], dz = p[2] - r.q[2];
  r.d2 = (dx * dx + dy * dy) + dz * dz;
  return r;
}

}  // namespace ctd
