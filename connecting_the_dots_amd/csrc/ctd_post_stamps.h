// ctd_post_stamps.h -- phase timeline of the two post kernels of a ranked call (fix-up: ncc_fixup.hip, tail:
// argmax_rerank.hip).  Diagnostic build only (-DCTD_STAMPS, tools/build_variant.sh): every wavefront notes the shader
// clock (s_memtime) at the phase boundaries of its FIRST item, straight into its row of a global array
// ([wavefront of the grid][kPostStampWords]); tools/post_timeline.py reads the rows through the export that
// CTD_POST_STAMP_EXPORT defines in each of the two files.  Row layout:
//   0..9   phase clocks (the kernels say which; 0 = entry, 9 = exit of the first item or of the wavefront)
//   10, 11 the 100 MHz counter (s_memrealtime) at entry and at the last stamp written
//   12     role of the workgroup (tail kernel), 13 XCC id, 14 = 1 when the wavefront carried an item, 15 = 1 row written
// The _V / _S forms first pin a value (vector / scalar register) in front of the clock reading, so that the stamp cannot
// be scheduled ahead of the load that produces it.  Without the flag everything here compiles to nothing: no stamp
// executes in the product build.
#pragma once

#ifdef CTD_STAMPS
namespace ctd {
constexpr int kPostStampWords = 16, kPostStampWaves = 16384;
static __device__ unsigned g_post_stamps[kPostStampWaves * kPostStampWords];
__device__ inline unsigned* post_stamp_slot(unsigned role) {
  const unsigned id = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (id >= (unsigned)kPostStampWaves) return nullptr;
  unsigned* st = g_post_stamps + id * kPostStampWords;
  if ((threadIdx.x & 63) == 0) {
    st[0] = (unsigned)__builtin_amdgcn_s_memtime();
    st[10] = (unsigned)__builtin_amdgcn_s_memrealtime();
    st[12] = role;
    st[13] = __builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11));   // HW_REG_XCC_ID, bits 0..3
    st[14] = 0u;
    st[15] = 1u;
  }
  return st;
}
__device__ inline void post_stamp_put(unsigned* st, int k) {
  const unsigned t = (unsigned)__builtin_amdgcn_s_memtime(), r = (unsigned)__builtin_amdgcn_s_memrealtime();
  if (st && (threadIdx.x & 63) == 0) {
    st[k] = t;
    st[11] = r;
  }
}
__device__ inline void post_stamp_item(unsigned* st) {
  if (st && (threadIdx.x & 63) == 0) st[14] = 1u;
}
}  // namespace ctd
#define CTD_POST_STAMP_SLOT(role) ctd::post_stamp_slot(role)
#define CTD_POST_STAMP(st, k) ctd::post_stamp_put(st, k)
#define CTD_POST_STAMP_V(st, k, v) do { asm volatile("" ::"v"(v)); ctd::post_stamp_put(st, k); } while (0)
#define CTD_POST_STAMP_S(st, k, s) do { asm volatile("" ::"s"(s)); ctd::post_stamp_put(st, k); } while (0)
#define CTD_POST_STAMP_ITEM(st) ctd::post_stamp_item(st)
#define CTD_POST_STAMP_EXPORT(name)                                                                                   \
  extern "C" int name(void* dst, size_t bytes) {                                                                      \
    const size_t have = sizeof(unsigned) * ctd::kPostStampWaves * ctd::kPostStampWords;                               \
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(ctd::g_post_stamps), bytes < have ? bytes : have);                \
  }
#else
#define CTD_POST_STAMP_SLOT(role) nullptr
#define CTD_POST_STAMP(st, k) do {} while (0)
#define CTD_POST_STAMP_V(st, k, v) do {} while (0)
#define CTD_POST_STAMP_S(st, k, s) do {} while (0)
#define CTD_POST_STAMP_ITEM(st) do {} while (0)
#define CTD_POST_STAMP_EXPORT(name)
#endif
