// costvol_sep.hip -- separable block SAD / MSE cost volume: plain padded operand planes, the all-D kernel in its cost
// mode (ncc_alld.hip), a border kernel for images that end inside a column tile.
#include "ctd_ncc_fast.h"

namespace ctd {

// ------------------------------------------------------------------------------------
// Separable block SAD / MSE cost volume (block 9):
//     cost[f][d][h][x] = 1/81 * sum over the 9 x 9 taps of g(P[r][clamp(c - d)] - I[r][c]),  r = clamp(h + dy), c = clamp(x + dx)
// (the tap column is clamped BEFORE the shift, ext.h:231-243 composed with P_d[h][x] = P[h][clamp(x - d)]), i.e. the
// replicate-border 9 x 9 box filter of the per-pixel plane q_d[r][c] = g(P[r][clamp(c - d)] - I[r][c]), g = |.| or (.)^2.
// The all-D kernel in its kASad / kAMse mode filters that plane exactly like the NCC products: 3+3+3 vertical sums in
// registers, the horizontal 9-sum by DPP, one subtract instead of 81 per output.  Its operand planes are plain padded
// copies: frames with 4 replicate columns either side, the pattern per UNCLAMPED column x = c - d with the replicate
// border baked in (cost_planes_kernel).  One difference to the NCC border rule: right of the image the NCC product
// column w0 > W-1 pairs a[W-1] with b[w0 - d], here it must be a COPY of column W-1 (clamp before the shift) -- so the
// halo right of the last column tile takes the pattern sample of column W-1 (loader), and for an image that ends INSIDE a
// tile (W % 256 != 0) the outputs of its last four columns are recomputed by cost_border_kernel (taps summed directly).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void cost_planes_kernel(const float* __restrict__ im, const float* __restrict__ pat,
                                                          long pat_frame_stride, float* __restrict__ ac,
                                                          float* __restrict__ bc, int frames, int n_pat, int H, int W, int Wp,
                                                          int W1, int xoff) {
  const long na = (long)frames * H * Wp, nb = (long)n_pat * H * W1;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += (long)gridDim.x * blockDim.x) {
    if (i < na) {
      const int c = (int)(i % Wp) - 4;
      const long fh = i / Wp;
      ac[i] = im[fh * W + clampi(c, 0, W - 1)];
    } else {
      const long k = i - na;
      const int x = (int)(k % W1) - xoff;
      const long ph = k / W1;                                      // pattern image * H + row
      const long pimg = ph / H, h = ph - pimg * H;
      bc[k] = pat[pimg * pat_frame_stride + h * W + clampi(x, 0, W - 1)];
    }
  }
}

// outputs (f, d, h, x) for the last four image columns x = W-4 .. W-1: thread per (f, d, h), the taps of its 9 x 8
// neighbourhood summed in the reference's composition (tap column clamped, then shifted and clamped again)
template <int TYPE>
__global__ __launch_bounds__(256) void cost_border_kernel(const float* __restrict__ im, const float* __restrict__ pat,
                                                          long pat_frame_stride, float* __restrict__ cost, int frames, int H,
                                                          int W, int D) {
  const long n = (long)frames * D * H;
  const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  // (d fastest: neighbouring lanes read neighbouring pattern samples and the same image sample)
  const int d = (int)(t % D), h = (int)((t / D) % H), f = (int)(t / ((long)H * D));
  const float* I = im + (long)f * H * W;
  const float* P = pat + (long)f * pat_frame_stride;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int dy = -4; dy <= 4; ++dy) {
    const int r = clampi(h + dy, 0, H - 1);
    float q[12];                                                   // q_d at columns W-8 .. W+3 (the last four: copies of W-1)
#pragma unroll
    for (int k = 0; k < 12; ++k) {
      const int c = clampi(W - 8 + k, 0, W - 1);
      const float df = P[(long)r * W + clampi(c - d, 0, W - 1)] - I[(long)r * W + c];
      q[k] = TYPE == 0 ? df * df : fabsf(df);
    }
#pragma unroll
    for (int o = 0; o < 4; ++o) {                                   // output column W-4+o: q index 4+o, window o .. o+8
      float s9 = 0.f;
#pragma unroll
      for (int k = 0; k < 9; ++k) s9 += q[o + k];
      acc[o] += s9;
    }
  }
  float* out = cost + (((long)f * D + d) * H + h) * W + (W - 4);
#pragma unroll
  for (int o = 0; o < 4; ++o)
    if (W - 4 + o >= 0) out[o] = acc[o] * (1.f / 81.f);
}

struct CostPlanes {
  PlaneGeometry g;
  size_t off_b, bytes;
};
static CostPlanes cost_planes(int frames, int H, int W, int D, bool per_frame_pattern) {
  CostPlanes cp;
  cp.g = plane_geometry(W, D);
  cp.off_b = align_up((size_t)frames * H * cp.g.Wp * sizeof(float), 256);
  cp.bytes = cp.off_b + align_up((size_t)(per_frame_pattern ? frames : 1) * H * cp.g.W1 * sizeof(float), 256);
  return cp;
}

bool costvol_sep_supported(int H, int W, int D, int bs, int type) {
  return bs == 9 && (type == 0 || type == 1) && W % 4 == 0 && W >= 8 && H >= 1 && D <= 512;
}

size_t costvol_sep_workspace_bytes(int frames, int H, int W, int D, bool per_frame_pattern) {
  return cost_planes(frames, H, W, D, per_frame_pattern).bytes;
}

int costvol_sep_f32(const float* im, const float* pat, long pat_frame_stride, float* cost, int frames, int H, int W, int D,
                    int type, void* workspace, size_t workspace_bytes, hipStream_t stream) {
  const bool per_frame = pat_frame_stride != 0;
  const CostPlanes cp = cost_planes(frames, H, W, D, per_frame);
  if (!workspace || workspace_bytes < cp.bytes || ((uintptr_t)workspace & 15)) return CTD_ERR_WORKSPACE;
  if (((uintptr_t)cost) % 16 != 0) return CTD_ERR_UNSUPPORTED;
  float* ac = (float*)workspace;
  float* bc = (float*)((char*)workspace + cp.off_b);
  const int n_pat = per_frame ? frames : 1;
  hipLaunchKernelGGL(cost_planes_kernel, dim3(1024), dim3(256), 0, stream, im, pat, pat_frame_stride, ac, bc, frames, n_pat, H, W,
                     cp.g.Wp, cp.g.W1, cp.g.xoff);
  CTD_LAUNCH_CHECK();
  const AlldOperands op = {ac, nullptr, nullptr, bc, nullptr, nullptr, per_frame ? (long)H * cp.g.W1 : 0, cp.g.Wp, cp.g.W1, cp.g.xoff};
  const int st = launch_alld(kAStore | (type == 1 ? kASad : kAMse), op, cost, nullptr, frames, H, W, D, false, stream);
  if (st) return st;
  if (W % 256 == 0) return CTD_OK;                                // (the loader's halo rule covers the right border)
  const long nb = (long)frames * D * H;
  if (type == 0)
    hipLaunchKernelGGL(cost_border_kernel<0>, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, stream, im, pat, pat_frame_stride, cost, frames, H, W, D);
  else
    hipLaunchKernelGGL(cost_border_kernel<1>, dim3((unsigned)ceil_div(nb, 256)), dim3(256), 0, stream, im, pat, pat_frame_stride, cost, frames, H, W, D);
  CTD_LAUNCH_CHECK();
  return CTD_OK;
}

}  // namespace ctd
