// mesh_robust.hip -- robust point-to-mesh ICP (ctd_mesh_face_rim_u8, ctd_mesh_robust_system_f32; the rules are stated word
// for word in include/ext/ctd_hip_mesh_robust.h).  The system of mesh_register.hip with a gate and a weight per point: the
// same posed points, the same nearest-face query of ctd_point_mesh_nearest.h (cutoff and hint, and here the recorded
// branch too), the same fixed-order f64 reduction of ctd_icp_solve.h.  mesh_register.hip is left as it is; what the two
// files have in common beyond those headers is the 12-line pose kernel.
//
// Every f32 product and sum is in the association of the header and the build never contracts them.
//   mesh_face_rim_kernel      -- thread = one face, once per mesh: three flag bytes and at most three rows of incident
//     faces walked (the rows of an adjacency that is fit for use hold at most 1024 entries); integer work.
//   mesh_robust_pose_kernel   -- thread = one point under one pose: S (12 B) to the workspace.
//   point_mesh_bvh_kernel / point_mesh_brute_kernel<cutoff, branch, hint> -- ONE query over all K * n posed points; the
//     branch byte goes to the workspace, face and closest to the caller's maps when there are any.
//   mesh_robust_system_kernel -- 1024 consecutive points of ONE pose, thread i the points i, i + 256, i + 512, i + 768,
//     ascending, as in mesh_register.hip; per point S, d2, f, q and the branch byte read back (33 B), the winning face's
//     corners when a normal is needed, one byte of rim[f] and 12 B of the point's normal when those gates are on.  The
//     pose's scale and rotation are block-uniform: scalar loads.  4 B residual, 4 B weight and 1 B status written when
//     asked for; `face` is the query's and is not touched again.
//   icp_finish_kernel         -- one wavefront per pose sums its workgroups, ascending.
// No atomics, no flag that another workgroup waits on: the same bits on every run.
#include <cfloat>
#include <cstdint>

#include "../../include/ext/ctd_hip_mesh_robust.h"
#include "ctd_icp_solve.h"
#include "ctd_point_mesh_nearest.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

constexpr int kMaxPoses = 64;
constexpr int kRimThreads = 256;
constexpr uint8_t kVertBoundary = 2;                          // CTD_MESH_VERT_BOUNDARY of include/ctd_hip_mesh_smooth.h

__device__ inline bool rim_face_valid(int i0, int i1, int i2, int n_verts) {
  return i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts && i0 != i1 && i1 != i2 && i0 != i2;
}

// the number of valid faces in the row of min(i, j) that have min(i, j) at one corner and max(i, j) at another; i != j,
// both in [0, n_verts)
__device__ inline int edge_multiplicity(int i, int j, const int* __restrict__ faces, int n_faces, int n_verts,
                                        const int32_t* __restrict__ face_offsets, const int32_t* __restrict__ face_ids,
                                        long n_incident) {
  const int lo = i < j ? i : j, hi = i < j ? j : i;
  const long b = face_offsets[lo], e = face_offsets[lo + 1];
  if (!(0 <= b && b <= e && e <= n_incident)) return 0;
  int count = 0;
  for (long k = b; k < e; ++k) {
    const int g = face_ids[k];
    if (g < 0 || g >= n_faces) continue;
    const int g0 = faces[(long)g * 3], g1 = faces[(long)g * 3 + 1], g2 = faces[(long)g * 3 + 2];
    if (!rim_face_valid(g0, g1, g2, n_verts)) continue;
    if ((g0 == lo || g1 == lo || g2 == lo) && (g0 == hi || g1 == hi || g2 == hi)) ++count;
  }
  return count;
}

__global__ __launch_bounds__(kRimThreads) void mesh_face_rim_kernel(const int* __restrict__ faces, int n_faces, int n_verts,
                                                                    const int32_t* __restrict__ face_offsets,
                                                                    const int32_t* __restrict__ face_ids, long n_incident,
                                                                    const uint8_t* __restrict__ vflags,
                                                                    uint8_t* __restrict__ rim) {
  const long f = (long)blockIdx.x * kRimThreads + threadIdx.x;
  if (f >= n_faces) return;
  const int a = faces[f * 3], b = faces[f * 3 + 1], c = faces[f * 3 + 2];
  unsigned out = 0;
  if (rim_face_valid(a, b, c, n_verts)) {
    if (vflags[a] & kVertBoundary) out |= 1u;
    if (vflags[b] & kVertBoundary) out |= 2u;
    if (vflags[c] & kVertBoundary) out |= 4u;
    if (edge_multiplicity(a, b, faces, n_faces, n_verts, face_offsets, face_ids, n_incident) == 1) out |= 8u;
    if (edge_multiplicity(a, c, faces, n_faces, n_verts, face_offsets, face_ids, n_incident) == 1) out |= 16u;
    if (edge_multiplicity(b, c, faces, n_faces, n_verts, face_offsets, face_ids, n_incident) == 1) out |= 32u;
  }
  rim[f] = (uint8_t)out;
}

// (mesh_register.hip's pose kernel)
__global__ __launch_bounds__(256) void mesh_robust_pose_kernel(const float* __restrict__ points, int n_points,
                                                               const float* __restrict__ R, const float* __restrict__ t,
                                                               float* __restrict__ S, int blocks) {
  const int k = blockIdx.x / blocks;
  const long i = (long)(blockIdx.x % blocks) * 256 + threadIdx.x;
  if (i >= n_points) return;
  const float* Rk = R + k * 9;
  const float* tk = t + k * 3;
  const float p0 = points[i * 3], p1 = points[i * 3 + 1], p2 = points[i * 3 + 2];
  float* out = S + ((long)k * n_points + i) * 3;
#pragma unroll
  for (int j = 0; j < 3; ++j) out[j] = ((Rk[j * 3] * p0 + Rk[j * 3 + 1] * p1) + Rk[j * 3 + 2] * p2) + tk[j];
}

// kNormals: the normal gate is on (normals != NULL).  rim == NULL: no rim gate.  kernel 0: scale is not read.
template <int kMetric, bool kNormals>
__global__ __launch_bounds__(kIcpThreads) void mesh_robust_system_kernel(
    const float* __restrict__ S, const float* __restrict__ d2, const int* __restrict__ face_q, const float* __restrict__ closest,
    const int8_t* __restrict__ feature, const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, int n_faces,
    const float* __restrict__ R, const float* __restrict__ normals, float min_cos, const uint8_t* __restrict__ rim, int kernel,
    const float* __restrict__ scale, double* __restrict__ partial, float* __restrict__ residual, float* __restrict__ weight,
    int8_t* __restrict__ status, int n_points, int chunks) {
  __shared__ double wave_sum[kIcpThreads / 64][kSys];
  const int k = blockIdx.x / chunks;
  const long base = (long)(blockIdx.x % chunks) * kIcpChunk, pose = (long)k * n_points;
  const float nan = __builtin_nanf("");
  const float c = kernel != 0 ? scale[k] : 1.f;
  const bool c_ok = kernel == 0 || c > 0.f;                   // (a NaN fails the compare)
  const float* Rk = R + k * 9;
  double acc[kSys];
#pragma unroll
  for (int e = 0; e < kSys; ++e) acc[e] = 0.0;
#pragma unroll
  for (int ci = 0; ci < kIcpPix; ++ci) {
    const long i = base + ci * kIcpThreads + threadIdx.x;
    if (i >= n_points) break;                                 // (ascending: every later point of the thread is past it too)
    const long g = pose + i;
    const int f = face_q[g];
    int st = 0;
    float res = nan, w = 0.f;
    if (f >= 0 && f < n_faces) {                              // (a face that won is such a face)
      const float Sp[3] = {S[g * 3], S[g * 3 + 1], S[g * 3 + 2]};
      const float D[3] = {Sp[0] - closest[g * 3], Sp[1] - closest[g * 3 + 1], Sp[2] - closest[g * 3 + 2]};
      float n0 = 0.f, n1 = 0.f, n2 = 0.f;
      if (kMetric == 0 || kNormals) {
        const int i0 = faces[(long)f * 3], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
        st = 2;
        if (i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts) {   // (likewise)
          const float *a = verts + (long)i0 * 3, *b = verts + (long)i1 * 3, *d = verts + (long)i2 * 3;
          const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {d[0] - a[0], d[1] - a[1], d[2] - a[2]};
          const float c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
          const float l = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
          if (l > 0.f && l < __builtin_inff()) {
            n0 = c0 / l; n1 = c1 / l; n2 = c2 / l;
            st = 0;
          }
        }
      }
      if (st == 0 && rim) {
        const int feat = feature[g];
        if (feat >= 0 && feat <= 5 && ((rim[f] >> feat) & 1)) st = 3;
      }
      if (kNormals && st == 0) {
        const float a0 = normals[i * 3], a1 = normals[i * 3 + 1], a2 = normals[i * 3 + 2];
        const float m0 = (Rk[0] * a0 + Rk[1] * a1) + Rk[2] * a2, m1 = (Rk[3] * a0 + Rk[4] * a1) + Rk[5] * a2,
                    m2 = (Rk[6] * a0 + Rk[7] * a1) + Rk[8] * a2;
        const float cosang = (m0 * n0 + m1 * n1) + m2 * n2;
        if (!(cosang >= min_cos)) st = 4;
      }
      if (st == 0) {
        const float e = kMetric == 0 ? n0 * D[0] + n1 * D[1] + n2 * D[2] : sqrtf(d2[g]);   // metric 1: the residual, not a row
        const float r = kMetric == 0 ? fabsf(e) : e;
        float wt = 1.f;
        if (!c_ok) {
          st = 5;
        } else if (kernel == 1) {
          wt = r <= c ? 1.f : c / r;
        } else if (kernel == 2) {
          if (r < c) {
            const float u = r / c, v = 1.f - u * u;
            wt = v * v;
          } else {
            st = 5;
          }
        }
        if (st == 0 && wt == 0.f) st = 5;
        if (st == 0) {
          res = e;
          w = wt;
          if (kMetric == 0) {
            const float Jf[6] = {Sp[1] * n2 - Sp[2] * n1, Sp[2] * n0 - Sp[0] * n2, Sp[0] * n1 - Sp[1] * n0, n0, n1, n2};
            icp_accumulate_weighted(acc, Jf, e, w);
          } else {
#pragma unroll
            for (int r3 = 0; r3 < 3; ++r3) {
              const float u[3] = {r3 == 0 ? 1.f : 0.f, r3 == 1 ? 1.f : 0.f, r3 == 2 ? 1.f : 0.f};
              const float Jf[6] = {Sp[1] * u[2] - Sp[2] * u[1], Sp[2] * u[0] - Sp[0] * u[2], Sp[0] * u[1] - Sp[1] * u[0],
                                   u[0], u[1], u[2]};
              icp_accumulate_weighted(acc, Jf, D[r3], w);
            }
          }
          acc[28] = acc[28] + 1.0;
        }
      }
    } else {
      st = 1;
    }
    if (residual) residual[g] = res;
    if (weight) weight[g] = w;
    if (status) status[g] = (int8_t)st;
  }
  icp_block_reduce(acc, wave_sum, partial + (long)blockIdx.x * kSys);   // one reduction per workgroup
}

inline int robust_chunks(int n_points) { return (int)(((long)n_points + kIcpChunk - 1) / kIcpChunk); }

bool robust_shape_ok(int K, int n_points) {
  return n_points >= 0 && K >= 1 && K <= kMaxPoses && (double)K * n_points * 3 < 2147483648.0;
}

// the parts of the workspace, in the order taken: mesh_register.hip's, and the feature byte before the partial sums
struct RobustWorkspace {
  size_t S, d2, face, closest, feature, partial, bytes;
  RobustWorkspace(int K, int n_points) {
    const size_t N = (size_t)K * n_points;
    WorkspaceCursor c;
    S = c.take(12 * N);
    d2 = c.take(4 * N);
    face = c.take(4 * N);
    closest = c.take(12 * N);
    feature = c.take(N);
    partial = c.take(sizeof(double) * kSys * (size_t)K * robust_chunks(n_points));
    bytes = c.bytes;
  }
};

}  // namespace

static int mesh_robust_system_f32(const float* points, int n_points, const float* R, const float* t, int K,
                                  const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh, int metric,
                                  float max_d2, const int32_t* hint, int kernel, const float* scale, const uint8_t* rim,
                                  const float* normals, float min_cos, double* system, int32_t* face, float* residual,
                                  float* weight, int8_t* status, float* closest, void* workspace, hipStream_t s) {
  const int chunks = robust_chunks(n_points);
  double* partial = nullptr;                                  // (n_points == 0: no workspace, and the finish reads none)
  if (n_points > 0) {
    const RobustWorkspace w(K, n_points);
    char* base = (char*)workspace;
    float* S = (float*)(base + w.S);
    float* d2 = (float*)(base + w.d2);
    int* face_q = face ? face : (int*)(base + w.face);
    float* q = closest ? closest : (float*)(base + w.closest);
    int8_t* feature = (int8_t*)(base + w.feature);
    partial = (double*)(base + w.partial);
    const int blocks = ceil_div(n_points, 256);
    mesh_robust_pose_kernel<<<dim3((unsigned)(K * blocks)), dim3(256), 0, s>>>(points, n_points, R, t, S, blocks);
    CTD_LAUNCH_CHECK();
    const int st = nearest_launch<true, true, true>(S, K * n_points, verts, n_verts, faces, n_faces, bvh, max_d2, d2, face_q, q,
                                                    feature, s, hint);
    if (st != CTD_OK) return st;
    const dim3 grid((unsigned)(K * chunks)), block(kIcpThreads);
#define CTD_ROBUST_LAUNCH(M, N)                                                                                          \
  mesh_robust_system_kernel<M, N><<<grid, block, 0, s>>>(S, d2, face_q, q, feature, verts, n_verts, faces, n_faces, R,   \
                                                         normals, min_cos, rim, kernel, scale, partial, residual, weight, \
                                                         status, n_points, chunks)
    if (metric == 0 && normals) CTD_ROBUST_LAUNCH(0, true);
    else if (metric == 0) CTD_ROBUST_LAUNCH(0, false);
    else if (normals) CTD_ROBUST_LAUNCH(1, true);
    else CTD_ROBUST_LAUNCH(1, false);
#undef CTD_ROBUST_LAUNCH
    CTD_LAUNCH_CHECK();
  }
  icp_finish_kernel<<<dim3((unsigned)K), dim3(64), 0, s>>>(partial, system, chunks);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

int ctd_mesh_face_rim_u8(const int* faces, int n_faces, int n_verts, const int32_t* face_offsets, const int32_t* face_ids,
                         int64_t n_incident, const uint8_t* vflags, uint8_t* rim, int device, void* stream) {
  if (n_faces < 0 || n_verts < 0 || n_incident < 0) return CTD_ERR_INVALID_ARG;
  if (n_faces > kBvhMaxFaces) return CTD_ERR_INVALID_ARG;
  if (n_faces > 0 && (!faces || !face_offsets || !face_ids || !vflags || !rim)) return CTD_ERR_INVALID_ARG;
  const Span sp[] = {{rim, (size_t)n_faces}, {faces, 12 * (size_t)n_faces}, {face_offsets, 4 * ((size_t)n_verts + 1)},
                     {face_ids, 4 * (size_t)n_incident}, {vflags, (size_t)n_verts}};
  if (spans_overlap(sp, 1, 5)) return CTD_ERR_INVALID_ARG;
  if (n_faces == 0) return CTD_OK;
  DeviceGuard g(device);
  if (g.status) return g.status;
  mesh_face_rim_kernel<<<dim3((unsigned)ceil_div(n_faces, kRimThreads)), dim3(kRimThreads), 0, (hipStream_t)stream>>>(
      faces, n_faces, n_verts, face_offsets, face_ids, (long)n_incident, vflags, rim);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

size_t ctd_mesh_robust_workspace_bytes(int K, int n_points) {
  if (!robust_shape_ok(K, n_points) || n_points == 0) return 0;
  return RobustWorkspace(K, n_points).bytes;
}

int ctd_mesh_robust_system_f32(const float* points, int n_points, const float* R, const float* t, int K,
                               const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh, int metric,
                               float max_d2, const int32_t* hint, int kernel, const float* scale, const uint8_t* rim,
                               const float* normals, float min_cos, double* system, int32_t* face, float* residual,
                               float* weight, int8_t* status, float* closest, void* workspace, size_t workspace_bytes,
                               int device, void* stream) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0) return CTD_ERR_INVALID_ARG;
  if (K < 1 || K > kMaxPoses) return CTD_ERR_INVALID_ARG;
  if (!robust_shape_ok(K, n_points) || n_faces > kBvhMaxFaces) return CTD_ERR_INVALID_ARG;
  if (metric != 0 && metric != 1) return CTD_ERR_INVALID_ARG;
  if (kernel < 0 || kernel > 2) return CTD_ERR_INVALID_ARG;
  if (!(max_d2 >= 0.f)) return CTD_ERR_INVALID_ARG;                                      // a NaN fails the comparison
  if (!(min_cos >= -1.f && min_cos <= 1.f)) return CTD_ERR_INVALID_ARG;                  // likewise
  if (!R || !t || !system || (kernel != 0 && !scale) || (n_points > 0 && !points)) return CTD_ERR_INVALID_ARG;
  if (!mesh_group_ok(verts, n_verts, faces, n_faces, bvh)) return CTD_ERR_INVALID_ARG;
  const size_t N = (size_t)K * n_points, need = ctd_mesh_robust_workspace_bytes(K, n_points);
  const Span sp[] = {{system, 8 * kSys * (size_t)K}, {face, 4 * N}, {residual, 4 * N}, {weight, 4 * N}, {status, N},
                     {closest, 12 * N}, {workspace, need}, {points, 12 * (size_t)n_points}, {R, 36 * (size_t)K},
                     {t, 12 * (size_t)K}, {verts, 12 * (size_t)n_verts}, {faces, 12 * (size_t)n_faces}, {hint, 4 * N},
                     {scale, 4 * (size_t)K}, {rim, (size_t)n_faces}, {normals, 12 * (size_t)n_points}};
  if (spans_overlap(sp, 7, 16)) return CTD_ERR_INVALID_ARG;
  if (n_points > 0 && !workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_robust_system_f32(points, n_points, R, t, K, verts, n_verts, faces, n_faces, bvh, metric, max_d2, hint, kernel,
                                scale, rim, normals, min_cos, system, face, residual, weight, status, closest, workspace,
                                (hipStream_t)stream);
}

}  // extern "C"
