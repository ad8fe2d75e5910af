// ctd_dispatch.h -- run-time (block size, loss type) to template arguments, host side.
//
//   return dispatch_block(bs, [&](auto bs_c) {
//     return dispatch_type(type, [&](auto type_c) -> int {
//       constexpr int BS = decltype(bs_c)::value, TYPE = decltype(type_c)::value;
//       hipLaunchKernelGGL((some_kernel<TYPE, BS>), ...);           // the one launch statement of some_kernel
//       ...
//
// The callback is a generic lambda: it is instantiated once per value, so a kernel that exists for some of the values
// only guards its launch with `if constexpr`.
#pragma once
#include <type_traits>

#include "ctd_common.h"

namespace ctd {

// block sizes of the LDS-tiled kernels (odd: symmetric window)
template <typename F>
inline int dispatch_block(int bs, F&& f) {
  switch (bs) {
    case 3: return f(std::integral_constant<int, 3>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 7: return f(std::integral_constant<int, 7>{});
    case 9: return f(std::integral_constant<int, 9>{});
    default: return CTD_ERR_UNSUPPORTED;
  }
}

// loss types: 0 mse, 1 sad, 2 census_mse, 3 census_sad
template <typename F>
inline int dispatch_type(int type, F&& f) {
  switch (type) {
    case 0: return f(std::integral_constant<int, 0>{});
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return CTD_ERR_INVALID_ARG;
  }
}

}  // namespace ctd
