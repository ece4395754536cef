// The exceedance threshold of the integer-count kernels that compare with a strict `>` (wbx_contingency.hip, wbx_ens_prob.hip, wbx_ens_brier.hip,
// wbx_fss_thresholds.hip).
#pragma once
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"

namespace wbx {

// Threshold k as the type the compare runs in, wave-uniform (SGPRs).  Padding slots (k >= nthr) hold +inf: never exceeded.
// float: x > thr (in float64) <=> x > rd(thr) (in float32) for every float32 x, rd = rounding toward -inf; round-to-nearest
// is not equivalent (float(0.1) > 0.1).  rd of a value beyond the float32 range is FLT_MAX / -inf, which is right as well.
template <typename T>
__device__ __forceinline__ T cont_threshold(const double* thr, int k, int nthr) {
  const double v = k < nthr ? ((const_ptr<double>)thr)[k] : (double)INFINITY;
  if constexpr (std::is_same<T, double>::value) {
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
  } else {
    float f = (float)v;    // to nearest
    if ((double)f > v) {   // (false for NaN) one step down: the next float32 towards -inf
      const uint32_t b = __float_as_uint(f);
      f = __uint_as_float(f > 0.f ? b - 1u : (f < 0.f ? b + 1u : 0x80000001u));
    }
    return __uint_as_float((uint32_t)__builtin_amdgcn_readfirstlane((int)__float_as_uint(f)));
  }
}

}  // namespace wbx
