// mesh_color.hip -- colours for mesh points from the views of a track (include/ctd_hip_mesh_color.h): per point and
// view the projection, the facing test, the occlusion query against a mesh and the bilinear sample, then the blend of
// the views that see the point.  Two kernels, one answer: the brute-force kernel is the definition, the traversal of the
// ray casters' BVH (render_bvh.hip, ctd_bvh.h) gives its bits.  Both run the same view_front / view_sample / Blend
// below; they differ only in which faces reach ray_tri (ctd_render.h) for the occlusion query.
//
// Why the tree gives brute force's boolean.  The query for (point X, view v) is: does ray_tri(Cv, dir, face) accept
// some face with 0 < ft < t_max?  Brute force asks every face.  The traversal skips a node when
// prune(Cv, dir, dn, box, t_best = t_max) holds, and ctd_bvh_ray.h proves that then no face under the node is accepted
// by ray_tri with ft <= t_max -- a superset of the hit condition ft < t_max, so a skipped node holds no hit.  Every face
// that could be a hit is therefore still handed to the same ray_tri with the same operands, and "some face hits" is a
// boolean: the visiting order and the early exit at the first hit cannot change it.  t_best never tightens here
// (any hit ends the query), so the test is the ray casters' at a constant limit.
//
// Why dir is normalised.  prune only acts when |dir| P <= 1 (P the node's largest |e1||e2|): its error bound needs the
// relative error of det under control.  With dir = e / len, |dir| = 1 up to rounding and dn = |dir| rounded up, so the
// test acts on every node whose faces have |e1||e2| <= 1 -- all of a reconstructed mesh -- and t_max = len - margin is a
// length in world units, as margin is.  An unnormalised e (|e| of a few units, t_max near 1) would switch pruning off
// for faces larger than 1 / |e| and make margin a fraction of the distance.
//
// NaN and infinities.  A non-finite Cv or dir (a point at the camera centre: len = 0, dir = 0/0), or a non-finite t_max,
// prunes nothing: the traversal visits every face, like brute force.  The hit test ft > 0 && ft < t_max is false for a
// NaN ft or a NaN t_max ("not occluded"), and prune's comparisons are false for NaN ("do not prune").  Nodes with an
// infinite box or P = inf (faces with non-finite vertices) are never pruned.
//
// Traversal: one wave of 64 points per workgroup, one point per lane, a per-lane stack in LDS (kStack entries, lane-
// interleaved so that a wave's accesses fall on 64 different banks), as in point_mesh.hip; an inner node pushes both
// children, so the stack never holds more than the tree's depth + 1 (checked at launch against kMaxDepth; the push is
// bounds-checked too).  The views are a loop inside the lane: the sums stay in ascending view order.
//
// Brute force: 256 points per workgroup, one per lane; for each view the faces stream through LDS in tiles of 256 in
// index order (each thread gathers one face's vertices, every lane then reads the same face: a broadcast).  Faces with
// an index outside [0, n_verts) are marked in the tile and skipped; their vertices are never dereferenced.  A view that
// no lane of the workgroup still has to decide streams nothing.
#include <cfloat>
#include <cstdint>

#include "../../include/ctd_hip_mesh_color.h"
#include "ctd_bvh.h"
#include "ctd_bvh_ray.h"
#include "ctd_common.h"
#include "ctd_mesh_query.h"
#include "ctd_render.h"
#include "ctd_validate.h"
#include "ctd_view.h"

namespace ctd {

constexpr int kColorBruteThreads = 256;
constexpr int kMaxChannels = 4;
constexpr unsigned kInImage = 1, kFacing = 2, kUnoccluded = 4, kUsed = 7;

struct ColorArgs {
  const float* points;
  const float* normals;
  int n_points;
  const float* images;
  const uint8_t* valid;
  const float* K;
  const float* R;
  const float* t;
  int V, C, H, W;
  float margin, min_cos;
  int mode;
  float* color;
  float* weight;
  int32_t* n_views;
  uint8_t* flags;
};

// what steps 1 to 3 of the rule leave for the occlusion query and the sample of one (point, view)
struct ViewGeom {
  int x0, y0;
  float fx, fy, w;
  float C[3], dir[3], t_max;
};

// steps 1 and 2 of the rule, and the ray of step 3 -> the bits passed so far (0, 1 or 3); n is read with normals only
__device__ inline unsigned view_front(const ColorArgs& a, int v, const float* X, const float* n, ViewGeom& g) {
  const float* R = a.R + v * 9;
  const float* t = a.t + v * 3;
  float S[3], uvd[3];
  world_to_camera(X, R, t, S);
  project(S, a.K, uvd);
  if (!(uvd[2] > 0.f)) return 0;
  const float x = uvd[0] / uvd[2], y = uvd[1] / uvd[2];
  if (!(x >= 0.f && x <= (float)(a.W - 1) && y >= 0.f && y <= (float)(a.H - 1))) return 0;
  const float x0 = fminf(floorf(x), (float)(a.W - 2)), y0 = fminf(floorf(y), (float)(a.H - 2));
  g.fx = x - x0;
  g.fy = y - y0;
  g.x0 = (int)x0;
  g.y0 = (int)y0;
  if (a.valid) {
    const uint8_t* m = a.valid + ((long)v * a.H + g.y0) * a.W + g.x0;
    if (!(m[0] && m[1] && m[a.W] && m[a.W + 1])) return 0;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) g.C[c] = -(R[c] * t[0] + R[3 + c] * t[1] + R[6 + c] * t[2]);
  g.w = 1.f;
  if (a.normals) {
    const float d[3] = {g.C[0] - X[0], g.C[1] - X[1], g.C[2] - X[2]};
    const float cosv = dot3(n, d) / sqrtf(dot3(d, d));
    if (!(cosv > 0.f && cosv >= a.min_cos)) return kInImage;
    g.w = cosv;
  }
  const float e[3] = {X[0] - g.C[0], X[1] - g.C[1], X[2] - g.C[2]};
  const float len = sqrtf(dot3(e, e));
  g.dir[0] = e[0] / len;
  g.dir[1] = e[1] / len;
  g.dir[2] = e[2] / len;
  g.t_max = len - a.margin;
  return kInImage | kFacing;
}

// the hit condition of step 3 for one face
__device__ inline bool occludes(const ViewGeom& g, const float* v0, const float* v1, const float* v2) {
  float ft, fu, fv;
  return ray_tri(g.C, g.dir, v0, v1, v2, ft, fu, fv) && ft > 0.f && ft < g.t_max;
}

// step 4
__device__ inline void view_sample(const ColorArgs& a, int v, const ViewGeom& g, float* s) {
  const long plane = (long)a.H * a.W;
  const float* I0 = a.images + (long)v * a.C * plane + (long)g.y0 * a.W + g.x0;
#pragma unroll
  for (int c = 0; c < kMaxChannels; ++c) {             // unrolled with a guard: s stays in registers
    if (c >= a.C) break;
    const float* I = I0 + c * plane;
    const float i00 = I[0], i01 = I[1], i10 = I[a.W], i11 = I[a.W + 1];
    const float top = i00 + g.fx * (i01 - i00), bot = i10 + g.fx * (i11 - i10);
    s[c] = top + g.fy * (bot - top);
  }
}

// the blend of the used views of one point, fed in ascending view order
struct Blend {
  float acc[kMaxChannels] = {0.f, 0.f, 0.f, 0.f};
  float wsum = 0.f;
  int n = 0;

  __device__ void add(const ColorArgs& a, const float* s, float w) {
    if (a.mode == 0) {
#pragma unroll
      for (int c = 0; c < kMaxChannels; ++c) acc[c] = c < a.C ? acc[c] + w * s[c] : 0.f;
      wsum = wsum + w;
    } else if (n == 0 || w > wsum) {                   // the first of equal w stays: the lowest v on a tie
#pragma unroll
      for (int c = 0; c < kMaxChannels; ++c) acc[c] = c < a.C ? s[c] : 0.f;
      wsum = w;
    }
    ++n;
  }

  __device__ void store(const ColorArgs& a, long i) const {
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int c = 0; c < kMaxChannels; ++c)
      if (c < a.C) a.color[i * a.C + c] = n == 0 ? nan : (a.mode == 0 ? acc[c] / wsum : acc[c]);
    a.weight[i] = n == 0 ? 0.f : wsum;
    a.n_views[i] = n;
  }
};

__device__ inline void view_finish(const ColorArgs& a, long i, int v, unsigned bits, const ViewGeom& g, Blend& blend) {
  if (a.flags) a.flags[i * a.V + v] = (uint8_t)bits;
  if (bits != kUsed) return;
  float s[kMaxChannels] = {0.f, 0.f, 0.f, 0.f};
  view_sample(a, v, g, s);
  blend.add(a, s, g.w);
}

__global__ __launch_bounds__(kColorBruteThreads) void view_colors_brute_kernel(ColorArgs a,
                                                                               const float* __restrict__ verts,
                                                                               int n_verts,
                                                                               const int* __restrict__ faces,
                                                                               int n_faces) {
  __shared__ float tri[kColorBruteThreads * 9];
  __shared__ int ok[kColorBruteThreads];
  const int tid = threadIdx.x;
  const long i = (long)blockIdx.x * kColorBruteThreads + tid;
  const bool live = i < a.n_points;
  float X[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
  if (live) {
    X[0] = a.points[i * 3]; X[1] = a.points[i * 3 + 1]; X[2] = a.points[i * 3 + 2];
    if (a.normals) { n[0] = a.normals[i * 3]; n[1] = a.normals[i * 3 + 1]; n[2] = a.normals[i * 3 + 2]; }
  }
  Blend blend;
  for (int v = 0; v < a.V; ++v) {
    ViewGeom g;
    const unsigned front = live ? view_front(a, v, X, n, g) : 0u;
    bool pending = front == (kInImage | kFacing);      // still to decide: no face has occluded the view so far
    for (int base = 0; base < n_faces; base += kColorBruteThreads) {
      // the previous tile has been read by every lane; a view that no lane has left to decide streams no more
      if (!__syncthreads_or(pending)) break;
      face_tile_load<kColorBruteThreads>(tri, ok, base, verts, n_verts, faces, n_faces);
      __syncthreads();
      if (!pending) continue;
      const int cnt = min(kColorBruteThreads, n_faces - base);
      for (int k = 0; k < cnt; ++k) {
        if (ok[k] && occludes(g, tri + k * 9, tri + k * 9 + 3, tri + k * 9 + 6)) {
          pending = false;
          break;
        }
      }
    }
    if (live) view_finish(a, i, v, front | (pending ? kUnoccluded : 0u), g, blend);
  }
  if (live) blend.store(a, i);
}

// any hit: true as soon as a face under the root is accepted with 0 < ft < t_max
__device__ inline bool bvh_occluded(const BvhView& bv, int* __restrict__ stack, const ViewGeom& g) {
  if (bv.n == 0) return false;
  const bool exact = finite3(g.C) && finite3(g.dir) && isfinite(g.t_max);   // otherwise: visit every face
  const float dn = norm3(g.dir) * 1.00001f;
  int sp = 1;
  lane_at(stack, 0) = 0;
  while (sp > 0) {
    const int node = lane_at(stack, --sp);
    if (exact && prune(g.C, g.dir, dn, bv.box[(long)node * 2], bv.box[(long)node * 2 + 1], g.t_max)) continue;
    const int4 m = bv.meta[node];
    if (m.x < 0) {
      const int first = -(m.x + 1);
      for (int k = 0; k < m.y; ++k) {
        float v0[3], v1[3], v2[3];
        bvh_leaf_tri(bv, first + k, v0, v1, v2);
        if (occludes(g, v0, v1, v2)) return true;
      }
    } else if (sp + 2 <= kStack) {                     // always true for depth <= kMaxDepth (checked at launch)
      lane_at(stack, sp++) = m.y;
      lane_at(stack, sp++) = m.x;
    }
  }
  return false;
}

__global__ __launch_bounds__(64) void view_colors_bvh_kernel(ColorArgs a, BvhView bv) {
  int* stack = lane_stack();
  const long i = (long)blockIdx.x * 64 + threadIdx.x;
  if (i >= a.n_points) return;
  const float X[3] = {a.points[i * 3], a.points[i * 3 + 1], a.points[i * 3 + 2]};
  float n[3] = {0.f, 0.f, 0.f};
  if (a.normals) { n[0] = a.normals[i * 3]; n[1] = a.normals[i * 3 + 1]; n[2] = a.normals[i * 3 + 2]; }
  Blend blend;
  for (int v = 0; v < a.V; ++v) {
    ViewGeom g;
    unsigned bits = view_front(a, v, X, n, g);
    if (bits == (kInImage | kFacing) && !bvh_occluded(bv, stack, g)) bits |= kUnoccluded;
    view_finish(a, i, v, bits, g, blend);
  }
  blend.store(a, i);
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_mesh_view_colors_f32(const float* points, const float* normals, int n_points, const float* images,
                             const uint8_t* valid, const float* K, const float* R, const float* t, int V, int C, int H,
                             int W, const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh,
                             float margin, float min_cos, int mode, float* color, float* weight, int32_t* n_views,
                             uint8_t* flags, int device, void* stream) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0 || V < 1 || V > 64 || C < 1 || C > kMaxChannels || H < 2 || W < 2)
    return CTD_ERR_INVALID_ARG;
  if ((mode != 0 && mode != 1) || !nonneg_finite(margin) || !(min_cos >= 0.f && min_cos < 1.f)) return CTD_ERR_INVALID_ARG;
  if (n_points > 0 && (!points || !images || !K || !R || !t || !color || !weight || !n_views)) return CTD_ERR_INVALID_ARG;
  if (!mesh_group_ok(verts, n_verts, faces, n_faces, bvh)) return CTD_ERR_INVALID_ARG;
  if (H > (1 << 24) || W > (1 << 24) || (double)V * C * H * W >= 2147483648.0 || (double)n_points * 3 >= 2147483648.0 ||
      (double)n_points * V >= 2147483648.0 || n_faces > kBvhMaxFaces)
    return CTD_ERR_UNSUPPORTED;
  const size_t n = (size_t)n_points, px = (size_t)H * W;
  const Span spans[] = {{color, n * C * 4},
                        {weight, n * 4},
                        {n_views, n * 4},
                        {flags, n * V},
                        {points, n * 12},
                        {normals, n * 12},
                        {images, (size_t)V * C * px * 4},
                        {valid, (size_t)V * px},
                        {K, 36},
                        {R, (size_t)V * 36},
                        {t, (size_t)V * 12},
                        {verts, (size_t)n_verts * 12},
                        {faces, (size_t)n_faces * 12},
                        {bvh, n_faces > 0 ? bvh_layout(n_faces).total : 0}};
  if (spans_overlap(spans, 4, (int)(sizeof(spans) / sizeof(spans[0])))) return CTD_ERR_INVALID_ARG;
  if (n_points == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const ColorArgs a{points, normals, n_points, images, valid, K, R, t, V, C, H, W, margin, min_cos, mode,
                    color, weight, n_views, flags};
  const hipStream_t s = (hipStream_t)stream;
  return tree_or_brute(
      bvh, n_faces, s,
      [&](const BvhView& bv) {
        hipLaunchKernelGGL(view_colors_bvh_kernel, dim3((unsigned)ceil_div(n_points, 64)), dim3(64), 0, s, a, bv);
      },
      [&] {
        hipLaunchKernelGGL(view_colors_brute_kernel, dim3((unsigned)ceil_div(n_points, kColorBruteThreads)),
                           dim3(kColorBruteThreads), 0, s, a, verts, n_verts, faces, n_faces);
      });
}

}  // extern "C"
