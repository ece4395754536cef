// One point per lane: a point's ensemble members loaded into registers, padded to a generated network size, sorted there and parked
// as a column in LDS, where order statistics are read at wave-uniform rows.  Shared by the kernels that need a whole sorted
// ensemble per point at run-time ranks (wbx_ens_wasserstein.hip, wbx_ens_interval.hip, wbx_ens_quantile.hip).
#pragma once
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"
#include "wbx_sortnet3_gen.hpp"

namespace wbx {

constexpr int WASS_LDS_BYTES = 32 * 1024;  // a block's column store at the largest padded size: four blocks fit a CU's 160 KiB
template <typename T>
constexpr int WASS_THREADS = WASS_LDS_BYTES / (WBX_WASS_MAX_MEMBERS * (int)sizeof(T));  // 128 for float32, 64 for float64
static_assert(WASS_THREADS<float> == 128 && WASS_THREADS<double> == 64, "whole waves, and a block size a plan may name");

template <typename T, int NS>
__device__ __forceinline__ void wass_sort(T (&x)[NS]) {
  if constexpr (std::is_same<T, float>::value) {
    // the bare instructions, as in wbx_ens_impl.hpp: fminf / fmaxf canonicalise every loaded member first
    SortNet3<NS>::sort(
        x,
        [](float u, float v) {
          float r;
          asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(u), "v"(v));
          return r;
        },
        [](float u, float v) {
          float r;
          asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(u), "v"(v));
          return r;
        },
        [](float u, float v, float w) {
          float r;
          asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(u), "v"(v), "v"(w));
          return r;
        },
        [](float u, float v, float w) {
          float r;
          asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(u), "v"(v), "v"(w));
          return r;
        },
        [](float u, float v, float w) {
          float r;
          asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(u), "v"(v), "v"(w));
          return r;
        });
  } else {  // float64 has no three-input min / med / max: compositions of the two-input ones
    SortNet3<NS>::sort(
        x, [](double u, double v) { return fmin(u, v); }, [](double u, double v) { return fmax(u, v); },
        [](double u, double v, double w) { return fmin(fmin(u, v), w); },
        [](double u, double v, double w) { return fmax(fmin(u, v), fmin(fmax(u, v), w)); },
        [](double u, double v, double w) { return fmax(fmax(u, v), w); });
  }
}

// n members at src, padded with +inf to NS, sorted.  `nan` collects the members' NaNs.  Branch-free: the slots past n re-read the
// last member (never past it) and drop the value.
template <typename T, int NS>
__device__ __forceinline__ void wass_load_sort(const T* src, int64_t stride, int n, T (&x)[NS], bool& nan) {
  const T inf = (T)__builtin_huge_val();
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    const T v = ld_stream(src + (int64_t)(k < n ? k : n - 1) * stride);
    nan |= v != v;
    x[k] = k < n ? v : inf;
  }
  wass_sort<T, NS>(x);
}

template <typename T, int NS>
__device__ __forceinline__ void wass_park(const T* pp, int64_t stride, int M, T* col, int cs, bool& nan) {
  T x[NS];
  wass_load_sort<T, NS>(pp, stride, M, x, nan);
#pragma unroll
  for (int k = 0; k < NS; ++k) col[k * cs] = x[k];
}

// The smallest generated network that holds m members (tests/interval_cases.py and tests/quantile_error_cases.py restate it).
static inline int ivl_padded(int m) {
  const int sizes[] = {4, 8, 16, 32, 50, 51, 64};
  for (int s : sizes)
    if (m <= s) return s;
  return 0;
}

}  // namespace wbx
