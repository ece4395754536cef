// What the two ranked-probability-score units share: wbx_ens_rps.hip (thresholds from a list, wave-uniform) and
// wbx_ens_rps_field.hip (thresholds read per point).  The rounding of a float64 threshold for float32 data, the compare, the point
// (the member walk that counts the members below each threshold, and the integer numerator), the write of a partial and the
// requirements both entries make of their plan.
#pragma once
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"

namespace wbx {

constexpr int ERPS_MAX_WAVES = 4;
constexpr int ERPS_FLIGHT = 8;  // member loads in flight per lane

// int32 numerator of a point: K (M - 1) M^2 < 2^31
static_assert((int64_t)WBX_ERPS_MAX_THRESHOLDS * (WBX_ERPS_MAX_MEMBERS - 1) * WBX_ERPS_MAX_MEMBERS * WBX_ERPS_MAX_MEMBERS < ((int64_t)1 << 31),
              "a point's numerator must fit an int32");

// v rounded to float32 so that a float32 compare decides like the float64 one.  For every float32 x
//   x <= v (in float64) <=> x <= rd(v) (in float32), rd = rounding toward -inf   (cont_threshold of wbx_contingency.hip)
//   x <  v (in float64) <=> x <  ru(v) (in float32), ru = rounding toward +inf
// and rounding to nearest is equivalent to neither (float(0.1) <= 0.1 is false).  Beyond the float32 range rd gives FLT_MAX /
// -inf and ru +inf / -FLT_MAX, which decide right as well.  NaN stays NaN.
template <bool RIGHT>
__device__ __forceinline__ float erps_round(double v) {
  float f = (float)v;  // to nearest
  const uint32_t b = __float_as_uint(f);
  if constexpr (RIGHT) {
    if ((double)f > v) f = __uint_as_float(f > 0.f ? b - 1u : (f < 0.f ? b + 1u : 0x80000001u));  // one step down
  } else {
    if ((double)f < v) f = __uint_as_float(f > 0.f ? b + 1u : (f < 0.f ? b - 1u : 0x00000001u));  // one step up
  }
  return f;
}

template <bool RIGHT, typename T>
__device__ __forceinline__ bool erps_below(T x, T thr) {
  if constexpr (RIGHT)
    return x <= thr;
  else
    return x < thr;
}

// The integer numerator sum_k n_k of the point whose members start at `pm` (element stride `ms`) and whose target is `y`;
// `nan` says whether a member or the target is NaN (the numerator is then meaningless).  Slots k >= nthr are skipped.
template <typename T, int NT, bool RIGHT>
__device__ __forceinline__ int32_t erps_point(const T* pm, int64_t ms, int M, T y, const T (&pa)[NT], const T (&tb)[NT], int nthr,
                                              bool fair, bool& nan) {
  int32_t c[NT];
#pragma unroll
  for (int q = 0; q < NT; ++q) c[q] = 0;
  bool bad = y != y;
  int m = 0;
  for (; m + ERPS_FLIGHT <= M; m += ERPS_FLIGHT) {
    T v[ERPS_FLIGHT];
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u) * ms);
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) {
      bad |= v[u] != v[u];
#pragma unroll
      for (int q = 0; q < NT; ++q) c[q] += erps_below<RIGHT>(v[u], pa[q]) ? 1 : 0;
    }
  }
  if (m < M) {  // the last, short group: the loads past the end re-read the last member and are not counted
    T v[ERPS_FLIGHT];
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) v[u] = ld_stream(pm + (int64_t)(m + u < M ? m + u : M - 1) * ms);
#pragma unroll
    for (int u = 0; u < ERPS_FLIGHT; ++u) {
      if (m + u < M) {
        bad |= v[u] != v[u];
#pragma unroll
        for (int q = 0; q < NT; ++q) c[q] += erps_below<RIGHT>(v[u], pa[q]) ? 1 : 0;
      }
    }
  }
  nan = bad;
  int32_t n = 0;
#pragma unroll
  for (int q = 0; q < NT; ++q) {
    if (q < nthr) {
      const int32_t e = c[q] - (erps_below<RIGHT>(y, tb[q]) ? M : 0);
      n += fair ? (M - 1) * e * e - c[q] * (M - c[q]) : e * e;
    }
  }
  return n;
}

// One partial from its integer sums: S = sum of the numerators over the good (valid, non-NaN) points.
__device__ __forceinline__ void erps_write(double* o, int64_t nj, uint32_t flags, double denom, int64_t s, int64_t ngood,
                                           int64_t nvalid) {
  const bool skipna = flags & WBX_FLAG_SKIPNA;
  const bool poisoned = !skipna && ngood != nvalid;  // a NaN under a valid point
  o[0] = poisoned ? (double)NAN : (double)s / denom;
  if (skipna)
    o[nj] = (double)ngood;
  else if (flags & WBX_FLAG_MASKED)
    o[nj] = (double)nvalid;
}

// What both entries require of nthr, M, the data dtype and the plan (`who`: "wbx_..._partial: ").
static inline int erps_requirements(const char* who, const wbx_s1_plan* plan, int dtype, int M, int nthr) {
  WBX_REQUIRE(nthr >= 1 && nthr <= WBX_ERPS_MAX_THRESHOLDS, "%s1..%d thresholds per launch (got %d)", who, WBX_ERPS_MAX_THRESHOLDS, nthr);
  WBX_REQUIRE(M >= 1 && M <= WBX_ERPS_MAX_MEMBERS, "%s1..%d members (got %d)", who, WBX_ERPS_MAX_MEMBERS, M);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "%sunknown dtype %d", who, dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA | WBX_FLAG_FAIR)), "%sflags other than MASKED | SKIPNA | FAIR (0x%x)", who,
              plan->flags);
  WBX_REQUIRE(!(plan->flags & WBX_FLAG_FAIR) || M >= 2, "%sthe fair score needs at least 2 members (got %d)", who, M);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "%sno plane mode, no folded x weights", who);
  // |S| stays exact in fp64: a partial meets at most depth_chunk * nx points of at most nthr (M - 1) M^2 each
  WBX_REQUIRE((double)plan->depth_chunk * (double)(plan->nx > 0 ? plan->nx : 1) * (double)nthr * (double)(M > 1 ? M - 1 : 1) * (double)M *
                      (double)M < 9007199254740992.0,
              "%s2^53 or more per partial (depth_chunk * nx * nthr * (M - 1) * M^2)", who);
  return 0;
}

static inline double erps_denominator(bool fair, int M) {
  return fair ? (double)M * (double)M * (double)(M - 1) : (double)M * (double)M;
}

}  // namespace wbx
