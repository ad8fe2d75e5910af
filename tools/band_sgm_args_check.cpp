// band_sgm_args_check.cpp -- the argument validation of csrc/band_sgm.hip (include/ext/ctd_hip_band_sgm.h) under host
// sanitizers: a stand-alone program with its own main that walks the rejections of the entry points with host buffers
// standing in for device pointers.  Every call returns before any HIP call, so it needs no GPU:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined connecting_the_dots_amd/csrc/band_sgm.hip \
//         tools/band_sgm_args_check.cpp -o tools/bin/band_sgm_args_check && tools/bin/band_sgm_args_check
// Prints "ok: 0 failures" and exits 0; a sanitizer report or a wrong status code fails it.
#include "../include/ext/ctd_hip_band_sgm.h"
#include "args_check.h"
int main() {
  const Arena P(4096, 8);
  float *a = (float*)P(0), *b = (float*)P(1), *vb = (float*)P(2), *S = (float*)P(3), *best = (float*)P(4);
  int32_t *lo = (int32_t*)P(5), *hi = (int32_t*)P(6);
  int64_t* idx = (int64_t*)P(7);
  void* ws = P(3);
  const float nan = std::nanf(""), inf = INFINITY;
  const int INV = 1, WSP = 2, UNS = 3;
#define AGG(vol_, lo_, hi_, p1_, p2_, paths_, S_, idx_, best_, frames_, slots_, H_, W_, D_, ws_, nws_) \
  ctd_band_sgm_aggregate_f32(vol_, lo_, hi_, 0, p1_, p2_, paths_, S_, idx_, best_, frames_, slots_, H_, W_, D_, ws_, nws_, -1, nullptr)
#define NCC(in0_, in1_, st_, lo_, hi_, vb_, frames_, slots_, H_, W_, D_, bs_, flags_, ws_, nws_) \
  ctd_xcorrvol_band_volume_f32(in0_, in1_, st_, lo_, hi_, vb_, frames_, slots_, H_, W_, D_, bs_, flags_, ws_, nws_, -1, nullptr)
#define COST(im_, pat_, st_, lo_, hi_, vb_, frames_, slots_, H_, W_, D_, bs_, type_) \
  ctd_costvol_band_volume_f32(im_, pat_, st_, lo_, hi_, vb_, frames_, slots_, H_, W_, D_, bs_, type_, 0.1f, -1, nullptr)
  // --- aggregation: scalars and sizes
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 0, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, INT32_MIN, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 5, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 0, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, -0.1f, 0.16f, 8, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.2f, 0.1f, 8, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  const float bad_pen[][2] = {{nan, 0.1f}, {0.1f, nan}, {0.1f, inf}, {inf, inf}, {-inf, 0.1f}, {nan, nan}};
  for (auto& p : bad_pen) {
    EXPECT(AGG(vb, lo, hi, p[0], p[1], 8, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
    EXPECT(AGG(vb, lo, hi, p[0], p[1], 8, S, idx, best, 0, 5, 8, 8, 16, nullptr, 0), INV);
  }
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, -1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 5, 0, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 5, 8, -1, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 5, 8, 8, 0, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, INT32_MIN, 5, INT32_MAX, INT32_MAX, INT32_MAX, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 5, 65536, 65536, 1, nullptr, 0), INV);
  // nothing to do
  EXPECT(AGG(nullptr, nullptr, nullptr, 0.f, 0.f, 4, nullptr, nullptr, nullptr, 0, 1, 1, 1, 1, nullptr, 0), 0);
  EXPECT(AGG(nullptr, nullptr, nullptr, 0.02f, 0.16f, 8, nullptr, nullptr, nullptr, 0, 65, 8, 8, 16, nullptr, 0), 0);
  // pointers, before support
  EXPECT(AGG(nullptr, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 65, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, nullptr, hi, 0.02f, 0.16f, 8, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, nullptr, 0.02f, 0.16f, 8, S, idx, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, nullptr, best, 1, 5, 8, 8, 16, nullptr, 0), INV);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, nullptr, 1, 5, 8, 8, 16, nullptr, 0), INV);
  // support, before the workspace
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, nullptr, idx, best, 1, 65, 8, 8, 16, nullptr, 0), UNS);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1, INT32_MAX, 8, 8, 16, nullptr, 0), UNS);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1 << 14, 1, 512, 512, 16, nullptr, 0), UNS);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, 1 << 9, 64, 512, 512, 16, nullptr, 0), UNS);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, S, idx, best, INT32_MAX, 64, 1, 1, 1, nullptr, 0), UNS);
  // the workspace (needed only without S_b)
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, nullptr, idx, best, 1, 5, 8, 8, 16, nullptr, 0), WSP);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, nullptr, idx, best, 1, 5, 8, 8, 16, ws, 4 * 5 * 64 - 1), WSP);
  EXPECT(AGG(vb, lo, hi, 0.02f, 0.16f, 8, nullptr, idx, best, 1, 5, 8, 8, 16, (char*)ws + 4, 1 << 20), WSP);
  EXPECT((int)ctd_band_sgm_workspace_bytes(1, 5, 8, 8, 16, 8, 0), 4 * 5 * 64);
  EXPECT((int)ctd_band_sgm_workspace_bytes(1, 5, 8, 8, 16, 8, 1), 0);
  EXPECT((int)ctd_band_sgm_workspace_bytes(1, 65, 8, 8, 16, 8, 0), 0);
  EXPECT((int)ctd_band_sgm_workspace_bytes(0, 5, 8, 8, 16, 8, 0), 0);
  EXPECT((int)ctd_band_sgm_workspace_bytes(1, 5, 8, 8, 16, 6, 0), 0);
  EXPECT((int)ctd_band_sgm_workspace_bytes(INT32_MIN, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, 8, 0), 0);
  // --- the band volume calls: what ctd_hip_band.h rejects, and slots
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 0, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 4, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, -1, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 7, lo, hi, vb, 1, 5, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 1, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 0, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, -1, 5, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 65536, 65536, 1, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 0, 0, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 65, 8, 8, 16, 5, 0x100, nullptr, 0), 0);
  EXPECT(NCC(nullptr, b, 0, lo, hi, vb, 1, 65, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, nullptr, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, nullptr, hi, vb, 1, 5, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, nullptr, vb, 1, 5, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, nullptr, 1, 5, 8, 8, 16, 5, 0, ws, 1 << 20), INV);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 65, 8, 8, 16, 5, 0, nullptr, 0), UNS);
  EXPECT(NCC(a, b, 512 * 512, lo, hi, vb, 1 << 14, 1, 512, 512, 16, 5, 0, nullptr, 0), UNS);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1 << 9, 64, 512, 512, 16, 5, 0, nullptr, 0), UNS);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 0, nullptr, 1 << 20), WSP);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 0, ws, 16), WSP);
  EXPECT(NCC(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 0x100, (char*)ws + 16, 1 << 20), WSP);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1, 0, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 6, 1), INV);
  EXPECT(COST(a, b, 3, lo, hi, vb, 1, 5, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, -1), INV);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 4), INV);
  EXPECT(COST(a, b, 0, lo, hi, vb, 0, 5, 8, 8, 16, 5, 4), INV);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1, 5, 0, 8, 16, 5, 1), INV);
  EXPECT(COST(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 65, 8, 8, 16, 5, 1), 0);
  EXPECT(COST(nullptr, b, 0, lo, hi, vb, 1, 65, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, nullptr, 0, lo, hi, vb, 1, 5, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, b, 0, nullptr, hi, vb, 1, 5, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, b, 0, lo, nullptr, vb, 1, 5, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, b, 0, lo, hi, nullptr, 1, 5, 8, 8, 16, 5, 1), INV);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1, 65, 8, 8, 16, 5, 1), UNS);
  EXPECT(COST(a, b, 0, lo, hi, vb, 1 << 9, 64, 512, 512, 16, 5, 1), UNS);
  return report();
}
