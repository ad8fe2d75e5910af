// ctd_icp_solve.h -- what the two ICPs share: depth_icp.hip (include/ctd_hip_icp.h, a view of a track against another)
// and mesh_register.hip / mesh_robust.hip (include/ext/ctd_hip_mesh_register.h, ctd_hip_mesh_robust.h, a point set against a
// mesh, plain and weighted).  All build the same 29-entry
// f64 system in the same fixed order and solve it the same way; they differ in where a residual and its Jacobian row
// come from and in how the step is composed with a pose.  The rules are stated word for word in include/ctd_hip_icp.h.
//   icp_accumulate   -- one row (J, e) into a thread's 28 sums (the count is the caller's: a point may have three rows).
//   icp_accumulate_weighted -- the same row under a weight w (mesh_robust.hip): w * (x * y), two roundings, no fma.
//   icp_block_reduce -- ONE reduction per workgroup of kIcpThreads: a butterfly over the lane distances 32 .. 1 (an add
//     commutes, so every lane ends with the same bits), the four wavefronts ascending through LDS, 29 f64 written.
//   icp_finish_kernel -- one wavefront per system: lane e < 29 sums entry e of the system's workgroups, ascending.
//   icp_solve        -- the damped LDL^T, the refusal conditions, the three solves and the Rodrigues step, in registers.
#pragma once

#include "ctd_common.h"

namespace ctd {

constexpr int kIcpThreads = 256;                              // threads of a workgroup of a system kernel
constexpr int kIcpPix = 4;                                    // pixels / points per thread before the cross-lane step
constexpr int kIcpChunk = kIcpThreads * kIcpPix;              // pixels / points per workgroup
constexpr int kSys = 29;                                      // 21 + 6 + 1 + 1 entries of a system

__device__ inline bool finite_f(float v) { return fabsf(v) < __builtin_inff(); }   // (a NaN fails the compare)

// acc[0..27] += the terms of one row; every product of two f32 factors is exact in f64, so fma() rounds once, as a
// product and an add would
__device__ __forceinline__ void icp_accumulate(double (&acc)[kSys], const float (&Jf)[6], float e) {
  double J[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) J[i] = (double)Jf[i];
  const double ed = (double)e;
  int m = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      acc[m] = fma(J[i], J[j], acc[m]);                       // the product is exact in f64: one rounding, that of the sum
      ++m;
    }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = fma(J[i], ed, acc[21 + i]);
  acc[27] = fma(ed, ed, acc[27]);
}

// the same row under a weight (mesh_robust.hip): every term is w * (x * y), the inner product exact, the multiplication
// by w the one rounding before that of the sum; deliberately no fma, which would round once.  With w == 1 the sums are
// icp_accumulate's bit for bit.
__device__ __forceinline__ void icp_accumulate_weighted(double (&acc)[kSys], const float (&Jf)[6], float e, float w) {
  double J[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) J[i] = (double)Jf[i];
  const double ed = (double)e, wd = (double)w;
  int m = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) {
      acc[m] = acc[m] + wd * (J[i] * J[j]);
      ++m;
    }
#pragma unroll
  for (int i = 0; i < 6; ++i) acc[21 + i] = acc[21 + i] + wd * (J[i] * ed);
  acc[27] = acc[27] + wd * (ed * ed);
}

// lanes, then wavefronts; out = the workgroup's 29 words.  Every thread of the workgroup calls it.
__device__ __forceinline__ void icp_block_reduce(double (&acc)[kSys], double (&wave_sum)[kIcpThreads / 64][kSys],
                                                 double* __restrict__ out) {
#pragma unroll
  for (int e = 0; e < kSys; ++e) {
    double v = acc[e];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    acc[e] = v;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int e = 0; e < kSys; ++e) wave_sum[wave][e] = acc[e];
  }
  __syncthreads();
  if (threadIdx.x < kSys) {
    double v = wave_sum[0][threadIdx.x];
#pragma unroll
    for (int w = 1; w < kIcpThreads / 64; ++w) v = v + wave_sum[w][threadIdx.x];
    out[threadIdx.x] = v;
  }
}

// (chunks == 0: a system of zeros; nothing of `partial` is read)
static __global__ __launch_bounds__(64) void icp_finish_kernel(const double* __restrict__ partial,
                                                               double* __restrict__ system, int chunks) {
  if (threadIdx.x >= kSys) return;
  if (chunks == 0) {
    system[(long)blockIdx.x * kSys + threadIdx.x] = 0.0;
    return;
  }
  const double* p = partial + (long)blockIdx.x * chunks * kSys + threadIdx.x;
  double v = p[0];
  for (int c = 1; c < chunks; ++c) v = v + p[(long)c * kSys];
  system[(long)blockIdx.x * kSys + threadIdx.x] = v;
}

// One system -> the step (Rr, x[3..5] = tr), or false: refused (`ok` as it comes in, the count, a pivot).  Every column
// is factored, also behind a pivot that fails (ok only ever falls): fully unrolled, all in registers.
__device__ __forceinline__ bool icp_solve(const double* __restrict__ sys, bool ok, double min_count, double min_pivot,
                                          double damping, double (&x)[6], double (&Rr)[3][3]) {
  double A[6][6], L[6][6], D[6], g[6];
  {
    int m = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        A[i][j] = sys[m];
        A[j][i] = sys[m];
        ++m;
      }
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) g[i] = sys[21 + i];
  ok = ok && sys[28] >= min_count;                            // (a NaN count fails the compare)
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j] + damping * A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * D[k];
    ok = ok && fabs(d) < (double)__builtin_inff() && d > min_pivot * A[j][j];      // (a NaN fails the compares)
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v = v - (L[i][k] * L[j][k]) * D[k];
      L[i][j] = v / d;
    }
  }
  if (!ok) return false;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = v - L[i][k] * x[k];
    x[i] = v;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) x[i] = x[i] / D[i];
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = x[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v = v - L[k][i] * x[k];
    x[i] = v;
  }
  const double w0 = x[0], w1 = x[1], w2 = x[2];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2, th = sqrt(th2);
  double ca, cb;
  if (th < 1e-4) {
    ca = 1.0 - th2 / 6.0;
    cb = 0.5 - th2 / 24.0;
  } else {
    ca = sin(th) / th;
    cb = (1.0 - cos(th)) / th2;
  }
  const double w[3] = {w0, w1, w2};
  const double Wx[3][3] = {{0.0, -w2, w1}, {w2, 0.0, -w0}, {-w1, w0, 0.0}};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double dij = i == j ? 1.0 : 0.0;
      Rr[i][j] = dij + ca * Wx[i][j] + cb * (w[i] * w[j] - th2 * dij);
    }
  return true;
}

}  // namespace ctd
