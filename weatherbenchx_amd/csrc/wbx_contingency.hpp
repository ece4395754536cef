// What the two contingency units share: wbx_contingency.hip (thresholds from a list, wave-uniform) and wbx_contingency_field.hip
// (thresholds read per point).  The load of V consecutive x, the write of a threshold's four cells from its integer counts and the
// requirements both entries make of their plan.  The block's integer reduction of the x-summed kernels is NOT here: as a shared
// function it changed the register allocation of cont_xr_kernel (one SGPR and two instructions more in the 1-slot kernels, another
// instruction order in the others), so wbx_contingency_field.hip has its own copy of those lines and wbx_contingency.hip's gfx950
// code object stays byte for byte what it was.
#pragma once
#include <cmath>
#include <type_traits>

#include "wbx_s1.hpp"

namespace wbx {

constexpr int CONT_MAX_WAVES = 4;

// V consecutive x of one row (unit x stride: one 16-byte load -- four mask bytes: one dword --, element aligned type as in
// wbx_det.hip) or V strided elements; x stride 0 broadcasts.  p / t are streamed, mask bytes stay cached.
template <typename T, int V>
__device__ __forceinline__ void cont_load(const void* base, int64_t off, int64_t x, int64_t xs, T (&v)[V]) {
  const T* p = reinterpret_cast<const T*>(base) + off;
  if constexpr (V == 4) {
    if (xs == 1) {
      if constexpr (sizeof(T) == 1) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(p + x);
        v[0] = (T)(q & 0xffu);
        v[1] = (T)((q >> 8) & 0xffu);
        v[2] = (T)((q >> 16) & 0xffu);
        v[3] = (T)(q >> 24);
      } else {
        typedef T v4_t __attribute__((ext_vector_type(4), aligned(sizeof(T))));
        const v4_t q = __builtin_nontemporal_load(reinterpret_cast<const v4_t*>(p + x));
        v[0] = q.x;
        v[1] = q.y;
        v[2] = q.z;
        v[3] = q.w;
      }
    } else {  // xs == 0 (check_plan: vec = 4 has unit / zero x strides)
      const T s = p[0];
      v[0] = v[1] = v[2] = v[3] = s;
    }
  } else {
#pragma unroll
    for (int k = 0; k < V; ++k) {
      if constexpr (sizeof(T) > 1)
        v[k] = ld_stream(p + (x + k) * xs);
      else
        v[k] = p[(x + k) * xs];
    }
  }
}

// The four cells of threshold k (and the count lanes) from the integer counts, into lanes o[lane * nj].
__device__ __forceinline__ void cont_write(double* o, int64_t nj, int nthr, int k, uint32_t flags, uint32_t tp, uint32_t np,
                                           uint32_t no, uint32_t ngood, uint32_t nvalid) {
  const bool skipna = flags & WBX_FLAG_SKIPNA;
  const bool poisoned = !skipna && ngood != nvalid;  // a NaN under a valid point
  double v[WBX_CONT_CELLS] = {(double)tp, (double)(np - tp), (double)(no - tp), (double)(ngood - np - no + tp)};
#pragma unroll
  for (int c = 0; c < WBX_CONT_CELLS; ++c) o[(int64_t)(c * nthr + k) * nj] = poisoned ? (double)NAN : v[c];
  const int nl = WBX_CONT_CELLS * nthr;
  if (skipna) {
#pragma unroll
    for (int c = 0; c < WBX_CONT_CELLS; ++c) o[(int64_t)(nl + c * nthr + k) * nj] = (double)ngood;
  } else if ((flags & WBX_FLAG_MASKED) && k == 0) {
    o[(int64_t)nl * nj] = (double)nvalid;
  }
}

// What both entries require of nthr, the data dtype and the plan (`who`: "wbx_..._partial: ").
static inline int cont_requirements(const char* who, const wbx_s1_plan* plan, int dtype, int nthr) {
  WBX_REQUIRE(nthr >= 1 && nthr <= WBX_CONT_MAX_THRESHOLDS, "%s1..%d thresholds per launch (got %d)", who, WBX_CONT_MAX_THRESHOLDS, nthr);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "%sunknown dtype %d", who, dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "%sflags other than MASKED | SKIPNA (0x%x)", who, plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "%sno plane mode, no folded x weights", who);
  // uint32 counters: a partial meets at most depth_chunk * nx points
  WBX_REQUIRE((double)plan->depth_chunk * (double)(plan->nx > 0 ? plan->nx : 1) < 4294967296.0,
              "%s2^32 or more points per partial (depth_chunk * nx)", who);
  return 0;
}

}  // namespace wbx
