// mesh_register.hip -- point-to-mesh ICP (ctd_mesh_register_system_f32, ctd_mesh_register_update_f32; the rules are
// stated word for word in include/ext/ctd_hip_mesh_register.h).  It joins the nearest-face query of
// ctd_point_mesh_nearest.h (with the cutoff and the hint) to the fixed-order f64 system and the solve of ctd_icp_solve.h,
// which depth_icp.hip runs too.
//
// Every f32 product and sum is in the association of the header and the build never contracts them.  Poses are indexed
// by a block-uniform value (the pose): scalar loads.
//   mesh_register_pose_kernel   -- thread = one point under one pose: 12 B read, S (12 B) written to the workspace.
//   point_mesh_bvh_kernel / point_mesh_brute_kernel<cutoff, no branch, hint> -- ONE query over all K * n posed points;
//     d2 and, unless the caller asked for them, face and closest go to the workspace.
//   mesh_register_system_kernel -- 1024 consecutive points of ONE pose (a chunk never crosses a pose): thread i takes the
//     points i, i + 256, i + 512, i + 768 of the chunk, ascending; per point S, d2, f, q read back (32 B) and, for the plane
//     metric, one gather of the winning face's indices and corners (48 B that the caches serve: neighbouring points share
//     faces); then the workgroup's one reduction.  4 B face and 4 B residual written when asked for.
//   icp_finish_kernel           -- one wavefront per pose sums its workgroups, ascending.
//   mesh_register_update_kernel -- one thread per pose, f64: icp_solve, R' = Rr R, t' = Rr t + tr, one rounding to f32.
// No atomics, no flag that another workgroup waits on: the same bits on every run.
//
// Why three passes and not one.  The intermediates are 32 B written and read back per posed point, 6.4 MB for 10^5 points,
// beside a traversal that takes milliseconds; the traversal wants one wave per workgroup with its stacks in LDS, the
// reduction wants 1024 points per workgroup in a fixed order.  profiles/mesh_register.txt has what the passes cost.
#include <cfloat>
#include <cstdint>

#include "../../include/ext/ctd_hip_mesh_register.h"
#include "ctd_icp_solve.h"
#include "ctd_point_mesh_nearest.h"
#include "ctd_validate.h"

namespace ctd {
namespace {

constexpr int kMaxPoses = 64;

__global__ __launch_bounds__(256) void mesh_register_pose_kernel(const float* __restrict__ points, int n_points,
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

// face_q: what the query wrote (the workspace, or the caller's `face`, which this kernel then finishes in place: a lane
// reads its own word before it writes it)
template <int kMetric>
__global__ __launch_bounds__(kIcpThreads) void mesh_register_system_kernel(
    const float* __restrict__ S, const float* __restrict__ d2, const int* face_q, const float* __restrict__ closest,
    const float* __restrict__ verts, int n_verts, const int* __restrict__ faces, int n_faces, double* __restrict__ partial,
    int* face_out, float* __restrict__ residual, int n_points, int chunks) {
  __shared__ double wave_sum[kIcpThreads / 64][kSys];
  const int k = blockIdx.x / chunks;
  const long base = (long)(blockIdx.x % chunks) * kIcpChunk, pose = (long)k * n_points;
  const float nan = __builtin_nanf("");
  double acc[kSys];
#pragma unroll
  for (int e = 0; e < kSys; ++e) acc[e] = 0.0;
#pragma unroll
  for (int c = 0; c < kIcpPix; ++c) {
    const long i = base + c * kIcpThreads + threadIdx.x;
    if (i >= n_points) break;                                 // (ascending: every later point of the thread is past it too)
    const long g = pose + i;
    int f = face_q[g];
    float res = nan;
    if (f >= 0 && f < n_faces) {                              // (a face that won is such a face)
      const float Sp[3] = {S[g * 3], S[g * 3 + 1], S[g * 3 + 2]};
      const float D[3] = {Sp[0] - closest[g * 3], Sp[1] - closest[g * 3 + 1], Sp[2] - closest[g * 3 + 2]};
      if (kMetric == 0) {
        const int i0 = faces[(long)f * 3], i1 = faces[(long)f * 3 + 1], i2 = faces[(long)f * 3 + 2];
        bool keep = i0 >= 0 && i0 < n_verts && i1 >= 0 && i1 < n_verts && i2 >= 0 && i2 < n_verts;   // (likewise)
        if (keep) {
          const float *a = verts + (long)i0 * 3, *b = verts + (long)i1 * 3, *d = verts + (long)i2 * 3;
          const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {d[0] - a[0], d[1] - a[1], d[2] - a[2]};
          const float c0 = e1[1] * e2[2] - e1[2] * e2[1], c1 = e1[2] * e2[0] - e1[0] * e2[2], c2 = e1[0] * e2[1] - e1[1] * e2[0];
          const float l = sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
          keep = l > 0.f && l < __builtin_inff();
          if (keep) {
            const float n0 = c0 / l, n1 = c1 / l, n2 = c2 / l;
            res = n0 * D[0] + n1 * D[1] + n2 * D[2];
            const float Jf[6] = {Sp[1] * n2 - Sp[2] * n1, Sp[2] * n0 - Sp[0] * n2, Sp[0] * n1 - Sp[1] * n0, n0, n1, n2};
            icp_accumulate(acc, Jf, res);
            acc[28] = acc[28] + 1.0;
          }
        }
        if (!keep) f = -1;
      } else {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const float u[3] = {r == 0 ? 1.f : 0.f, r == 1 ? 1.f : 0.f, r == 2 ? 1.f : 0.f};
          const float Jf[6] = {Sp[1] * u[2] - Sp[2] * u[1], Sp[2] * u[0] - Sp[0] * u[2], Sp[0] * u[1] - Sp[1] * u[0],
                               u[0], u[1], u[2]};
          icp_accumulate(acc, Jf, D[r]);
        }
        acc[28] = acc[28] + 1.0;
        res = sqrtf(d2[g]);
      }
    } else {
      f = -1;
    }
    if (face_out) face_out[g] = f;
    if (residual) residual[g] = res;
  }
  icp_block_reduce(acc, wave_sum, partial + (long)blockIdx.x * kSys);   // one reduction per workgroup
}

__global__ __launch_bounds__(64) void mesh_register_update_kernel(const double* __restrict__ system,
                                                                  const float* __restrict__ R, const float* __restrict__ t,
                                                                  double min_count, double min_pivot, double damping,
                                                                  float* __restrict__ R_out, float* __restrict__ t_out,
                                                                  uint8_t* __restrict__ ok_out, int K) {
  const int k = threadIdx.x;
  if (k >= K) return;
  const float* Rk = R + k * 9;
  const float* tk = t + k * 3;
  double x[6], Rr[3][3];
  if (!icp_solve(system + (long)k * kSys, true, min_count, min_pivot, damping, x, Rr)) {
    for (int i = 0; i < 9; ++i) R_out[k * 9 + i] = Rk[i];
    for (int i = 0; i < 3; ++i) t_out[k * 3 + i] = tk[i];
    ok_out[k] = 0;
    return;
  }
  double Rd[3][3], td[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    td[i] = (double)tk[i];
#pragma unroll
    for (int j = 0; j < 3; ++j) Rd[i][j] = (double)Rk[i * 3 + j];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      R_out[k * 9 + i * 3 + j] = (float)(Rr[i][0] * Rd[0][j] + Rr[i][1] * Rd[1][j] + Rr[i][2] * Rd[2][j]);
    t_out[k * 3 + i] = (float)(Rr[i][0] * td[0] + Rr[i][1] * td[1] + Rr[i][2] * td[2] + x[3 + i]);
  }
  ok_out[k] = 1;
}

inline int register_chunks(int n_points) { return (int)(((long)n_points + kIcpChunk - 1) / kIcpChunk); }

bool register_shape_ok(int K, int n_points) {
  return n_points >= 0 && K >= 1 && K <= kMaxPoses && (double)K * n_points * 3 < 2147483648.0;
}

// the parts of the workspace, in the order taken
struct RegisterWorkspace {
  size_t S, d2, face, closest, partial, bytes;
  RegisterWorkspace(int K, int n_points) {
    const size_t N = (size_t)K * n_points;
    WorkspaceCursor c;
    S = c.take(12 * N);
    d2 = c.take(4 * N);
    face = c.take(4 * N);
    closest = c.take(12 * N);
    partial = c.take(sizeof(double) * kSys * (size_t)K * register_chunks(n_points));
    bytes = c.bytes;
  }
};

}  // namespace

static int mesh_register_system_f32(const float* points, int n_points, const float* R, const float* t, int K,
                                    const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh,
                                    int metric, float max_d2, const int32_t* hint, double* system, int32_t* face,
                                    float* residual, float* closest, void* workspace, hipStream_t s) {
  const int chunks = register_chunks(n_points);
  double* partial = nullptr;                                  // (n_points == 0: no workspace, and the finish reads none)
  if (n_points > 0) {
    const RegisterWorkspace w(K, n_points);
    char* base = (char*)workspace;
    float* S = (float*)(base + w.S);
    float* d2 = (float*)(base + w.d2);
    int* face_q = face ? face : (int*)(base + w.face);
    float* q = closest ? closest : (float*)(base + w.closest);
    partial = (double*)(base + w.partial);
    const int blocks = ceil_div(n_points, 256);
    mesh_register_pose_kernel<<<dim3((unsigned)(K * blocks)), dim3(256), 0, s>>>(points, n_points, R, t, S, blocks);
    CTD_LAUNCH_CHECK();
    const int st = nearest_launch<true, false, true>(S, K * n_points, verts, n_verts, faces, n_faces, bvh, max_d2, d2, face_q,
                                                     q, nullptr, s, hint);
    if (st != CTD_OK) return st;
    if (metric == 0)
      mesh_register_system_kernel<0><<<dim3((unsigned)(K * chunks)), dim3(kIcpThreads), 0, s>>>(
          S, d2, face_q, q, verts, n_verts, faces, n_faces, partial, face, residual, n_points, chunks);
    else
      mesh_register_system_kernel<1><<<dim3((unsigned)(K * chunks)), dim3(kIcpThreads), 0, s>>>(
          S, d2, face_q, q, verts, n_verts, faces, n_faces, partial, face, residual, n_points, chunks);
    CTD_LAUNCH_CHECK();
  }
  icp_finish_kernel<<<dim3((unsigned)K), dim3(64), 0, s>>>(partial, system, chunks);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd

using namespace ctd;

extern "C" {

size_t ctd_mesh_register_workspace_bytes(int K, int n_points) {
  if (!register_shape_ok(K, n_points) || n_points == 0) return 0;
  return RegisterWorkspace(K, n_points).bytes;
}

int ctd_mesh_register_system_f32(const float* points, int n_points, const float* R, const float* t, int K,
                                 const float* verts, int n_verts, const int* faces, int n_faces, const void* bvh,
                                 int metric, float max_d2, const int32_t* hint, double* system, int32_t* face,
                                 float* residual, float* closest, void* workspace, size_t workspace_bytes, int device,
                                 void* stream) {
  if (n_points < 0 || n_verts < 0 || n_faces < 0) return CTD_ERR_INVALID_ARG;
  if (K < 1 || K > kMaxPoses) return CTD_ERR_INVALID_ARG;
  if (!register_shape_ok(K, n_points) || n_faces > kBvhMaxFaces) return CTD_ERR_INVALID_ARG;
  if (metric != 0 && metric != 1) return CTD_ERR_INVALID_ARG;
  if (!(max_d2 >= 0.f)) return CTD_ERR_INVALID_ARG;                                      // a NaN fails the comparison
  if (!R || !t || !system || (n_points > 0 && !points)) return CTD_ERR_INVALID_ARG;
  if (!mesh_group_ok(verts, n_verts, faces, n_faces, bvh)) return CTD_ERR_INVALID_ARG;
  const size_t N = (size_t)K * n_points, need = ctd_mesh_register_workspace_bytes(K, n_points);
  const Span sp[] = {{system, 8 * kSys * (size_t)K}, {face, 4 * N}, {residual, 4 * N}, {closest, 12 * N}, {workspace, need},
                     {points, 12 * (size_t)n_points}, {R, 36 * (size_t)K}, {t, 12 * (size_t)K}, {verts, 12 * (size_t)n_verts},
                     {faces, 12 * (size_t)n_faces}, {hint, 4 * N}};
  if (spans_overlap(sp, 5, 11)) return CTD_ERR_INVALID_ARG;
  if (n_points > 0 && !workspace_ok(workspace, workspace_bytes, need)) return CTD_ERR_WORKSPACE;
  DeviceGuard g(device);
  if (g.status) return g.status;
  return mesh_register_system_f32(points, n_points, R, t, K, verts, n_verts, faces, n_faces, bvh, metric, max_d2, hint, system,
                                  face, residual, closest, workspace, (hipStream_t)stream);
}

int ctd_mesh_register_update_f32(const double* system, const float* R, const float* t, int min_count, double min_pivot,
                                 double damping, float* R_out, float* t_out, uint8_t* ok, int K, int device,
                                 void* stream) {
  if (K < 1 || K > kMaxPoses || min_count < 0 || !(min_pivot >= 0.0) || !(damping >= 0.0)) return CTD_ERR_INVALID_ARG;
  if (!system || !R || !t || !R_out || !t_out || !ok) return CTD_ERR_INVALID_ARG;
  const size_t k = (size_t)K;
  const Span sp[] = {{R_out, 36 * k}, {t_out, 12 * k}, {ok, k}, {system, 8 * kSys * k}, {R, 36 * k}, {t, 12 * k}};
  if (spans_overlap(sp, 3, 6)) return CTD_ERR_INVALID_ARG;
  DeviceGuard g(device);
  if (g.status) return g.status;
  mesh_register_update_kernel<<<dim3(1), dim3(64), 0, (hipStream_t)stream>>>(system, R, t, (double)min_count, min_pivot,
                                                                            damping, R_out, t_out, ok, K);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // extern "C"
