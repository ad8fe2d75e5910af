// ctd_bvh_ray.h -- the exact pruning test of a ray against a node of the BVH of ctd_bvh.h, shared by the ray casters
// (render_bvh.hip: nearest hit) and the occlusion query of mesh_color.hip (any hit before a limit).  One copy, so that
// both give the bits of their brute-force paths for the same reason: ray_tri (ctd_render.h) decides every hit, and
// `prune` only skips nodes none of whose faces ray_tri could accept at or before the limit.
//
// Why pruning is safe (forward-error bound of ray_tri as coded; u = 2^-24, gamma_n = nu/(1-nu)).
//   Ray o, d (floats); face v0, v1, v2; e1 = fl(v1-v0), e2 = fl(v2-v0), tvec = fl(o-v0).  Treat the computed e1,
//   e2, tvec as data: the triangle T' = v0 + {a e1 + b e2} lies within u(|e1|+|e2|) of the face's box, the line
//   with origin v0 + tvec within u|o-v0| of the ray's.  With exact Moeller-Trumbore quantities det, N_u, N_v,
//   N_t and their computed values (cross product componentwise error <= gamma_2(|a_j b_k|+|a_k b_j|), so
//   |d x e2 - fl(d x e2)| <= sqrt2 gamma_2 |d||e2|; 3-term dot <= gamma_3 |a||b|):
//     |det_c - det| <= 7u |d||e1||e2|,  |N_u,c - N_u| <= 7u |tvec||d||e2|,  |N_v,c - N_v| <= 7u |tvec||d||e1|,
//     |N_t,c - N_t| <= 7u |tvec||e1||e2|.
//   An accepted face has |det_c| >= 1e-6.  Let dP = |d||e1||e2|; if dP <= 1 then rho = |det_c-det|/|det_c| <= 0.42.
//   Then for the exact barycentrics u' = N_u/det (the same for v'):  N_c/det_c - N/det = (dN + u' ddet)/det_c,
//   and |u'| <= 1 + |du| (u_c in [0,1]) give |du| <= ((|dN_u| + |ddet|)/|det_c| + 2.1u) / (1 - rho), so
//     |du||e1| + |dv||e2| <= 28e6 u dP (R + E) + 8.4u E,   R >= |o - v0|, E >= max(|e1|, |e2|).
//   The exact line thus passes through a point X within delta = 1.67 dP (R+E) + u(R + 10.4E) of the face's box
//   (the last term adds the data roundings above); the kernel uses delta = 2 dP (R+E) + 1e-6 (R+E).  X is at
//   line parameter t' with |X - o| <= R + 2 delta, and
//     |N_t,c/det_c - t'| <= (|dN_t| + |t'||ddet|)/|det_c| <= 7e6 u |e1||e2| (2R + 2 delta) =: dt,
//   the kernel using dt = |e1||e2| (R + delta) (2.4x that).  ft = N_t,c/det_c (1+th)^2, |th| <= u.
//   Per node: the box is the union of its faces' vertex boxes, P = max |e1||e2|, E = max(|e1|, |e2|) (each
//   rounded up by 1e-5 relative); per ray: |d| rounded up and R = the largest distance from o to a box corner.
//   The node is pruned only if (a) |d| P <= 1, and (b) the line misses the box widened by delta (+2e-6 |coord|
//   against the rounding of the widening), or (c) its entry parameter tn, lowered by dt, exceeds t_best.  Slab
//   parameters (lo - o) / d carry <= 2.1u relative error: entries are lowered and exits raised by a 1e-6
//   relative slack (a multiply, so infinities stay infinite).  d_i == 0 tests o_i against the slab directly (no
//   0 * inf).  Every comparison is written so that NaN means "do not prune".  A ray with a non-finite origin or
//   direction (the shadow ray's pdir has z = 0) prunes nothing (the callers do not ask `prune` then): it visits every
//   face, like brute force.  Faces with a non-finite vertex, or whose |e1||e2| overflows, get an infinite box and P = inf:
//   never pruned.  Huge faces (the data generator's 1000-unit board) have dP > 1 or a box that covers everything;
//   that only costs the visits along their path to the root.
#pragma once

#include "ctd_common.h"

namespace ctd {

__device__ inline bool finite3(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

__device__ inline float lower_rel(float x) { return x > 0 ? x * (1.f - 1e-6f) : x * (1.f + 1e-6f); }
__device__ inline float upper_rel(float x) { return x > 0 ? x * (1.f + 1e-6f) : x * (1.f - 1e-6f); }

// true only if no face under this node can be accepted by ray_tri with ft <= t_best (header comment); dn >= |d|
__device__ inline bool prune(const float* o, const float* d, float dn, float4 b0, float4 b1, float t_best) {
  const float P = b0.w, E = b1.w;
  const float dP = dn * P;
  if (!(dP <= 1.f)) return false;
  const float lo[3] = {b0.x, b0.y, b0.z}, hi[3] = {b1.x, b1.y, b1.z};
  float r2 = 0.f;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float m = fmaxf(fabsf(o[k] - lo[k]), fabsf(o[k] - hi[k]));
    r2 += m * m;
  }
  const float R = sqrtf(r2) * 1.00001f;
  const float delta = 2.f * dP * (R + E) + 1e-6f * (R + E);
  float tn = -INFINITY, tf = INFINITY;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float l = lo[k] - (delta + 2e-6f * fabsf(lo[k])), h = hi[k] + (delta + 2e-6f * fabsf(hi[k]));
    if (d[k] == 0.f) {
      if (o[k] < l || o[k] > h) return true;
      continue;
    }
    const float ta = (l - o[k]) / d[k], tb = (h - o[k]) / d[k];
    tn = fmaxf(tn, fminf(ta, tb));
    tf = fminf(tf, fmaxf(ta, tb));
  }
  const float tn_lo = lower_rel(tn);
  if (tn_lo > upper_rel(tf)) return true;
  const float dt = P * (R + delta);
  const float L = lower_rel(tn_lo - dt);
  return L > t_best;
}

}  // namespace ctd
