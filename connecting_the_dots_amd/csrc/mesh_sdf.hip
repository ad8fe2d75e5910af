// mesh_sdf.hip -- the signed point-to-mesh query (include/ctd_hip_mesh_sdf.h): the nearest face within a cutoff, the
// branch point_tri took for it, and the side of the oriented surface the point lies on.
//
// Two launches.  The first is the nearest-face kernel of ctd_point_mesh_nearest.h (brute force or the tree, the one copy
// that point_mesh.hip instantiates too) with the cutoff and the recorded branch switched on; why pruning stays safe under
// the cutoff is argued there and in point_mesh.hip's header.  The second, mesh_sdf_sign_kernel, takes one point per lane:
// it reads p, the face and the feature, the closest point q (from `closest`, or, when the caller passed NULL, from the
// same point_tri on the winning face, which gives the same bits), the face's three indices, and then at most one row
// of incident faces: none for the interior, the row of the smaller end for an edge, the row of the vertex for a
// vertex.  Everything after the reads is f64, one IEEE operation per operator in the association the header writes
// (-ffp-contract=off), summed in row order: no atomics, no flag, the same bits on every run.
//
// The only operations that are not correctly rounded are atan2 and, through it, the vertex weights: the device's atan2
// is within 2 ulp, so a vertex pseudonormal differs from a correctly rounded evaluation by about 4e-16 relative, and
// a sign can differ only where |dot| is that small against |r| * sum(alpha).  sqrt and the divisions are correctly
// rounded (no fast-math).
//
// Shape.  256 lanes per workgroup, no LDS, no barrier.  A lane's loop runs over one row, at most
// CTD_MESH_ADJ_MAX_INCIDENT entries for an adjacency the Python layer accepts, and over whatever the row says
// otherwise (bounded by n_incident); lanes of a wave diverge by feature, which costs the longest row among them.  Each
// row entry is three index loads and nine coordinate loads that the caches serve (neighbouring points share faces).
// 96 VGPRs, no scratch (the f64 atan2 is inlined).  The pass takes 0.02-0.03 ms for 10^5 points beside a nearest-face
// pass of 4-62 ms (profiles/mesh_sdf.txt), so a fused epilogue in the traversal kernel was not tried.
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/ctd_hip_mesh_sdf.h"
#include "ctd_point_mesh_nearest.h"

namespace ctd {

constexpr int kSignThreads = 256;

// e1 x e2 of the stored corners, from the f32 vertices in f64
__device__ inline void face_cross(const float* __restrict__ verts, int i0, int i1, int i2, double* c) {
  const float *a = verts + (long)i0 * 3, *b = verts + (long)i1 * 3, *d = verts + (long)i2 * 3;
  const double e1[3] = {(double)b[0] - (double)a[0], (double)b[1] - (double)a[1], (double)b[2] - (double)a[2]};
  const double e2[3] = {(double)d[0] - (double)a[0], (double)d[1] - (double)a[1], (double)d[2] - (double)a[2]};
  c[0] = e1[1] * e2[2] - e1[2] * e2[1];
  c[1] = e1[2] * e2[0] - e1[0] * e2[2];
  c[2] = e1[0] * e2[1] - e1[1] * e2[0];
}

// unit(g): false when the face contributes nothing
__device__ inline bool face_unit(const float* __restrict__ verts, int i0, int i1, int i2, double* n) {
  double c[3];
  face_cross(verts, i0, i1, i2, c);
  const double l = sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]);
  if (!(l > 0.0) || !isfinite(l)) return false;
  n[0] = c[0] / l;
  n[1] = c[1] / l;
  n[2] = c[2] / l;
  return true;
}

__device__ inline bool face_valid(int i0, int i1, int i2, int n_verts) {
  return i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts && i0 != i1 && i1 != i2 && i0 != i2;
}

__global__ __launch_bounds__(kSignThreads) void mesh_sdf_sign_kernel(
    const float* __restrict__ points, int n_points, const float* __restrict__ verts, int n_verts, const int* __restrict__ faces,
    int n_faces, const int32_t* __restrict__ face_offsets, const int32_t* __restrict__ face_ids, long n_incident,
    const int* __restrict__ face, const float* __restrict__ closest, const int8_t* __restrict__ feature,
    int8_t* __restrict__ sign) {
  const long i = (long)blockIdx.x * kSignThreads + threadIdx.x;
  if (i >= n_points) return;
  const int f = face[i], feat = feature[i];
  int8_t out = 0;
  if (f >= 0 && f < n_faces && feat >= 0 && feat <= 6) {
    const int i0 = faces[(long)f * 3], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
    if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {   // a face that won is such a face
      const float p[3] = {points[i * 3], points[i * 3 + 1], points[i * 3 + 2]};
      float q[3];
      if (closest) {
        q[0] = closest[i * 3]; q[1] = closest[i * 3 + 1]; q[2] = closest[i * 3 + 2];
      } else {
        const PointTri r = point_tri(p, verts + (long)i0 * 3, verts + (long)i1 * 3, verts + (long)i2 * 3);
        q[0] = r.q[0]; q[1] = r.q[1]; q[2] = r.q[2];
      }
      double N[3] = {0.0, 0.0, 0.0};
      if (feat == 6) {
        face_cross(verts, i0, i1, i2, N);
      } else {
        // the row to walk: of the vertex, or of the smaller end of the edge {lo, hi}
        int lo, hi = -1;
        if (feat < 3) {
          lo = feat == 0 ? i0 : (feat == 1 ? i1 : i2);
        } else {
          const int ea = feat == 5 ? i1 : i0, eb = feat == 3 ? i1 : i2;
          lo = ea < eb ? ea : eb;
          hi = ea < eb ? eb : ea;
        }
        long beg = 0, end = 0;
        if (feat < 3 || lo != hi) {
          const long b = face_offsets[lo], e = face_offsets[lo + 1];
          if (0 <= b && b <= e && e <= n_incident) { beg = b; end = e; }
        }
        for (long k = beg; k < end; ++k) {
          const int g = face_ids[k];
          if (g < 0 || g >= n_faces) continue;
          const int g0 = faces[(long)g * 3], g1 = faces[(long)g * 3 + 1], g2 = faces[(long)g * 3 + 2];
          if (!face_valid(g0, g1, g2, n_verts)) continue;
          const int at = g0 == lo ? 0 : (g1 == lo ? 1 : (g2 == lo ? 2 : -1));   // the corner of g that is the row's vertex
          if (at < 0) continue;
          double n[3];
          if (feat >= 3) {
            if (g0 != hi && g1 != hi && g2 != hi) continue;
            if (!face_unit(verts, g0, g1, g2, n)) continue;
          } else {
            if (!face_unit(verts, g0, g1, g2, n)) continue;
            const int nx = at == 0 ? g1 : (at == 1 ? g2 : g0), nn = at == 0 ? g2 : (at == 1 ? g0 : g1);
            const float *o = verts + (long)lo * 3, *un = verts + (long)nx * 3, *wn = verts + (long)nn * 3;
            const double u[3] = {(double)un[0] - (double)o[0], (double)un[1] - (double)o[1], (double)un[2] - (double)o[2]};
            const double w[3] = {(double)wn[0] - (double)o[0], (double)wn[1] - (double)o[1], (double)wn[2] - (double)o[2]};
            const double x[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]};
            const double alpha = atan2(sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]);
            n[0] = alpha * n[0];
            n[1] = alpha * n[1];
            n[2] = alpha * n[2];
            if (!isfinite(n[0]) || !isfinite(n[1]) || !isfinite(n[2])) continue;
          }
          N[0] = N[0] + n[0];
          N[1] = N[1] + n[1];
          N[2] = N[2] + n[2];
        }
      }
      const double r[3] = {(double)p[0] - (double)q[0], (double)p[1] - (double)q[1], (double)p[2] - (double)q[2]};
      const double dot = (r[0] * N[0] + r[1] * N[1]) + r[2] * N[2];
      out = dot > 0.0 ? 1 : (dot < 0.0 ? -1 : 0);
    }
  }
  sign[i] = out;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_point_mesh_signed_f32(const float* points, int n_points, const float* verts, int n_verts, const int* faces,
                              int n_faces, const int32_t* face_offsets, const int32_t* face_ids, int64_t n_incident,
                              const void* bvh, float max_d2, float* d2, int* face, float* closest, int8_t* feature,
                              int8_t* sign, int device, void* stream) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0 || n_incident < 0) return CTD_ERR_INVALID_ARG;
  if ((double)n_points * 3 >= 2147483648.0 || n_faces > kBvhMaxFaces) return CTD_ERR_INVALID_ARG;
  if (!(max_d2 >= 0.f)) return CTD_ERR_INVALID_ARG;                                      // a NaN fails the comparison
  if (n_points > 0 && (!points || !d2 || !face || !feature || !sign || !face_offsets || !face_ids)) return CTD_ERR_INVALID_ARG;
  if (!mesh_group_ok(verts, n_verts, faces, n_faces, bvh)) return CTD_ERR_INVALID_ARG;
  if (n_points == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  const hipStream_t s = (hipStream_t)stream;
  const int st = nearest_launch<true, true>(points, n_points, verts, n_verts, faces, n_faces, bvh, max_d2, d2, face, closest,
                                            feature, s);
  if (st != CTD_OK) return st;
  hipLaunchKernelGGL(mesh_sdf_sign_kernel, dim3((unsigned)ceil_div(n_points, kSignThreads)), dim3(kSignThreads), 0, s, points,
                     n_points, verts, n_verts, faces, n_faces, face_offsets, face_ids, (long)n_incident, face, closest, feature,
                     sign);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // extern "C"
