// What the two FSS entries share (wbx_fss.hip: wbx_fss_partial; wbx_fss_thresholds.hip: wbx_fss_threshold_partial): the launch
// arguments, the block-wide scan step, the three lanes of a point, the band rule and the checks both entries make.
#pragma once
#include <cstring>
#include <type_traits>

#include "wbx_common.hpp"

namespace wbx {

constexpr int FSS_THREADS = 256;
constexpr int FSS_WAVES = FSS_THREADS / 64;
constexpr int FSS_BMAX = WBX_FSS_MAX_BAND_ROWS;  // rows of a band (the x-summed row accumulators in LDS)
constexpr int FSS_NACC = 2 * WBX_FSS_LANES;
static_assert(WBX_FSS_MAX_NLON == 8 * FSS_THREADS, "a thread owns at most eight columns");

struct FssArgs {
  const void* in[3];  // p, t, mask
  const int64_t* key_off[3];
  const int64_t* depth_off[3];
  int64_t lat_stride[3], lon_stride[3];
  int64_t nkey, D, dchunk;
  int32_t nlat, nlon, nchunk, nband, B, n, x_kept, wrap;
  uint32_t flags;
  double* out;
};

template <typename V>
__device__ __forceinline__ V fss_wave_scan(V v, int lane) {  // inclusive, lanes in order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const V u = __shfl_up(v, o, 64);
    v = lane >= o ? v + u : v;
  }
  return v;
}

// F: the type the fractions and their squares are formed in -- float for n > 1 (the host route's float32 arrays), the input type
// for n == 1 (the fractions ARE the inputs).
template <typename F>
__device__ __forceinline__ void fss_lanes(F pf, F tf, double (&v)[WBX_FSS_LANES]) {
  const F d = pf - tf;
  v[0] = (double)(d * d);
  v[1] = (double)(pf * pf);
  v[2] = (double)(tf * tf);
}

// Rows of a band (include/wbx.h says how): the largest band, halved while the launch has fewer than WBX_FSS_TARGET_BLOCKS blocks and
// the halo of n - 1 rows stays at most half of the band.
static int fss_band_rows(const wbx_fss_plan* plan, int n) {
  const int64_t units = plan->nkey * plan->nchunk;
  int B = FSS_BMAX;
  while (B > WBX_FSS_MIN_BAND_ROWS && units * ((plan->nlat + B - 1) / B) < WBX_FSS_TARGET_BLOCKS && B / 2 >= 2 * (n - 1)) B /= 2;
  return B;
}

static bool fss_empty(const wbx_fss_plan* plan) { return plan->nkey == 0 || plan->ndepth == 0 || plan->nlat == 0 || plan->nlon == 0; }

// What both entries refuse; `who` is the entry's name.
static int fss_check(const char* who, wbx_ctx* ctx, const wbx_fss_plan* plan, int dtype, int n, const void* p, const void* t,
                     const uint8_t* mask, double* partial_out) {
  WBX_REQUIRE(ctx != nullptr, "%s: ctx is NULL", who);
  WBX_REQUIRE(plan != nullptr, "%s: plan is NULL", who);
  WBX_REQUIRE(plan->nkey >= 0 && plan->ndepth >= 0 && plan->nlat >= 0 && plan->nlon >= 0, "%s: negative plan extent", who);
  WBX_REQUIRE(plan->nchunk >= 1 && plan->depth_chunk >= 1, "%s: nchunk/depth_chunk must be >= 1", who);
  WBX_REQUIRE((int64_t)plan->nchunk * plan->depth_chunk >= plan->ndepth, "%s: chunks do not cover depth", who);
  WBX_REQUIRE(n >= 1 && n % 2 == 1, "%s: the neighbourhood size must be odd and at least 1 (got %d)", who, n);
  WBX_REQUIRE(plan->nlat < (int64_t)1 << 30 && plan->nlon <= WBX_FSS_MAX_NLON, "%s: nlon %lld exceeds %d (or nlat 2^30)", who,
              (long long)plan->nlon, WBX_FSS_MAX_NLON);
  WBX_REQUIRE(n == 1 || plan->nlat == 0 || plan->nlon == 0 || (n <= plan->nlat && n <= plan->nlon),
              "%s: the neighbourhood (%d) is larger than the field (%lld x %lld)", who, n, (long long)plan->nlat,
              (long long)plan->nlon);
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "%s: unknown dtype %d", who, dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "%s: flags other than MASKED | SKIPNA (0x%x)", who, plan->flags);
  if (plan->flags & WBX_FLAG_MASKED) WBX_REQUIRE(mask != nullptr, "%s: WBX_FLAG_MASKED set but mask is NULL", who);
  WBX_REQUIRE(partial_out != nullptr || plan->nkey == 0, "%s: partial_out is NULL", who);
  WBX_REQUIRE(fss_empty(plan) || (p != nullptr && t != nullptr), "%s: p/t is NULL", who);
  return 0;
}

// The launch arguments of a checked plan; the band is the caller's.
static FssArgs fss_args(const wbx_fss_plan* plan, int n, const void* p, const void* t, const uint8_t* mask, double* partial_out) {
  FssArgs a;
  memset(&a, 0, sizeof(a));
  a.in[0] = p;
  a.in[1] = t;
  a.in[2] = mask;
  for (int i = 0; i < 3; ++i) {
    a.key_off[i] = plan->key_off[i];
    a.depth_off[i] = plan->depth_off[i];
    a.lat_stride[i] = plan->lat_stride[i];
    a.lon_stride[i] = plan->lon_stride[i];
  }
  a.nkey = plan->nkey;
  a.D = plan->ndepth;
  a.dchunk = plan->depth_chunk;
  a.nlat = (int32_t)plan->nlat;
  a.nlon = (int32_t)plan->nlon;
  a.nchunk = plan->nchunk;
  a.n = n;
  a.x_kept = plan->x_kept;
  a.wrap = plan->wrap_longitude != 0;
  a.flags = plan->flags;
  a.out = partial_out;
  return a;
}

}  // namespace wbx
