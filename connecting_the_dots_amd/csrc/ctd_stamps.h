// ctd_stamps.h -- barrier timeline of the all-D kernel.  Diagnostic build only (-DCTD_STAMPS, tools/build_variant.sh):
// every wavefront notes the shader clock (s_memtime) when it ARRIVES at each chunk barrier of pass CTD_STAMP_PASS and when
// it LEAVES it, into LDS behind the staging ring; the workgroup dumps them at its end ([workgroup][kStampWords]: 8 header
// words, then [wave][chunk][arrive | leave]).  tools/alld_timeline.py reads them through ctd_debug_read_stamps.  Without
// the flag everything here compiles to nothing: no stamp executes in the product build.
// Included by ncc_alld.hip alone (the header defines the device array and the two exports).
#pragma once
#include "ctd_wave.h"

#ifdef CTD_STAMPS
#ifndef CTD_STAMP_PASS
#define CTD_STAMP_PASS 2
#endif
namespace ctd {
constexpr int kStampChunks = 34, kStampWords = 8 + 16 * kStampChunks * 2, kStampWgs = 1024;
__device__ unsigned g_stamps[kStampWgs * kStampWords];
inline size_t stamp_lds_bytes() { return sizeof(unsigned) * kStampWords; }   // host: what a launch adds to its dynamic LDS
__device__ inline unsigned stamp_now() { return (unsigned)__builtin_amdgcn_s_memtime(); }
// (no scalar of its own: the consumer loops are at the limit of the scalar registers -- hipcc 7.2 dies with "illegal VGPR
// to SGPR copy" when their spilling fails -- so the wavefront number comes from threadIdx and the stamp area's address is
// an immediate offset from the ring's base)
__device__ inline void stamp_put(unsigned* st, int pass, int chunk, int which) {
  const unsigned t = stamp_now();
  const int idx = 8 + ((int)(threadIdx.x >> 6) * kStampChunks + chunk) * 2 + which;
  if ((threadIdx.x & 63) == 0 && pass == CTD_STAMP_PASS && chunk < kStampChunks) st[idx] = t;
}
// start of the workgroup: cleared area, header words 0..3
__device__ inline void stamp_begin(unsigned* st, int n_chunks) {
  for (int k = threadIdx.x; k < kStampWords; k += blockDim.x) st[k] = 0u;
  if (threadIdx.x == 0) {
    st[0] = stamp_now();
    st[1] = (unsigned)__builtin_amdgcn_s_memrealtime();
    st[2] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));   // HW_REG_XCC_ID, bits 0..3
    st[3] = (unsigned)n_chunks;
  }
}
// end of a wavefront's role (every wavefront of the workgroup calls it once): header words 4..5, LDS -> g_stamps
__device__ inline void stamp_dump(unsigned* st) {
  wait_lgkmcnt0();
  wg_barrier();
  if (threadIdx.x == 0) {
    st[4] = stamp_now();
    st[5] = (unsigned)__builtin_amdgcn_s_memrealtime();
  }
  wait_lgkmcnt0();
  wg_barrier();
  if ((int)blockIdx.x < kStampWgs)
    for (int k = threadIdx.x; k < kStampWords; k += blockDim.x) g_stamps[blockIdx.x * kStampWords + k] = st[k];
}
}  // namespace ctd
#define CTD_STAMP_BEGIN(st, n_chunks) stamp_begin(st, n_chunks)
#define CTD_STAMP_DUMP(st) stamp_dump(st)
#define CTD_STAMP_ARRIVE(st, wave, pass, chunk, lane) stamp_put(st, pass, chunk, 0)
#define CTD_STAMP_LEAVE(st, wave, pass, chunk, lane) stamp_put(st, pass, chunk, 1)

extern "C" int ctd_debug_read_stamps(void* dst, size_t bytes) {
  const size_t have = sizeof(unsigned) * ctd::kStampWgs * ctd::kStampWords;
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(ctd::g_stamps), bytes < have ? bytes : have);
}
extern "C" int ctd_debug_stamp_layout(int* words_per_wg, int* chunks, int* pass) {
  *words_per_wg = ctd::kStampWords; *chunks = ctd::kStampChunks; *pass = CTD_STAMP_PASS;
  return 0;
}
#else
namespace ctd {
inline size_t stamp_lds_bytes() { return 0; }
}  // namespace ctd
#define CTD_STAMP_BEGIN(st, n_chunks) do {} while (0)
#define CTD_STAMP_DUMP(st) do {} while (0)
#define CTD_STAMP_ARRIVE(st, wave, pass, chunk, lane) do {} while (0)
#define CTD_STAMP_LEAVE(st, wave, pass, chunk, lane) do {} while (0)
#endif
