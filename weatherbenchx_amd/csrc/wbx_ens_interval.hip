// Interval statistics of an ensemble, summed like any other stage-1 statistic: Covered, Confident and JaccardDistant
// (weatherbenchX/metrics/categorical.py:701-863, the three factors of Opportunism) from ONE sort of a point's members instead of two
// host quantile fields per statistic, an aligned copy of the climatology and three Boolean arrays.
//
// Reference semantics restated (include/wbx.h has them in full).  Per point the members are sorted in the input type; a quantile
// bound (k, g) -- h = q (M - 1), k = floor(h), g = h - k, formed by the host in float64 -- is NumPy's `linear` method in NumPy's
// order of operations, in float64: with A = x_(k), B = x_(min(k + 1, M - 1)), d = B - A it is A + d g where g < 0.5 and
// B - d (1 - g) otherwise, every product and sum rounded on its own and no shortcut for g == 0 (inf * 0 is NaN there too).  A NaN
// member makes every ensemble quantile of the point NaN by a flag gathered while the members are loaded (v_min / v_max drop NaN).
// The indicators are comparisons of those numbers with the target and with the climatology's two quantile fields; they are 0 or 1,
// never NaN.
//
// Mapping.  One point per lane, as wbx_ens_wasserstein.hip: the M members are loaded into registers, padded with +inf to the next
// generated network size and sorted there (wbx_ens_park.hpp), the sorted column is parked in LDS member-major, and the up to
// twelve order statistics of the up to six bounds are read back at wave-uniform rows k and min(k + 1, M - 1): no register is indexed at
// run time, no lane-dependent control flow.  The requested lanes are a kernel argument (wave-uniform branches); what no requested
// lane needs is not read (t without Covered, c with Covered alone).  The padded sizes are dispatched inside the kernel: two kernels
// per dtype.  A full sort is more than a handful of order statistics need: a network pruned to the wanted ranks is the tuning left.
//
// Arithmetic after the sort is float64 with contraction switched off (the pragma in ivl_quantile and ivl_point): a fused
// multiply-add in A + d g rounds once where NumPy rounds twice, and an indicator can hang on that bit.  The sums are integers in
// float64: a lane adds its points in the order they come, lanes and waves are summed in fixed orders, no atomics.
#include "wbx_ens_park.hpp"

namespace wbx {

static_assert(WBX_IVL_MAX_MEMBERS == WBX_WASS_MAX_MEMBERS, "the column store of wbx_ens_park.hpp is sized for this many members");

struct IvlArgs {
  wbx_ivl_lane lane[3];  // Covered, Confident, JaccardDistant (host values)
  int32_t lanes;         // WBX_IVL_* bit set
  int32_t nval;          // its population count: the value lanes
  int32_t np;            // M padded to a generated network size
};

// NumPy's linear quantile of the parked sorted column at the bound b; `nan`: the point has a NaN member.
template <typename T>
__device__ __forceinline__ double ivl_quantile(const T* col, int cs, int M, const wbx_ivl_bound& b, bool nan) {
#pragma clang fp contract(off)
  const int k1 = b.k + 1 < M ? b.k + 1 : M - 1;
  const double A = (double)col[b.k * cs], B = (double)col[k1 * cs];
  const double d = B - A;
  const double up = d * b.g, down = d * (1.0 - b.g);
  const double q = b.g < 0.5 ? A + up : B - down;
  return nan ? __builtin_nan("") : q;
}

// The indicators of the point x of the row at ro[] as 0.0 / 1.0 in v[bit index of the lane]; lanes not asked for stay 0.
template <typename T>
__device__ __forceinline__ void ivl_point(const S1Args& a, const IvlArgs& e, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x, T* col, int cs,
                                          double (&v)[3]) {
#pragma clang fp contract(off)
  const T* pp = reinterpret_cast<const T*>(a.in[0]) + ro[0] + x * a.xstride[0];
  const int M = a.M;
  bool nan = false;
  switch (e.np) {
    case 4: wass_park<T, 4>(pp, a.mstride, M, col, cs, nan); break;
    case 8: wass_park<T, 8>(pp, a.mstride, M, col, cs, nan); break;
    case 16: wass_park<T, 16>(pp, a.mstride, M, col, cs, nan); break;
    case 32: wass_park<T, 32>(pp, a.mstride, M, col, cs, nan); break;
    case 50: wass_park<T, 50>(pp, a.mstride, M, col, cs, nan); break;
    case 51: wass_park<T, 51>(pp, a.mstride, M, col, cs, nan); break;
    default: wass_park<T, 64>(pp, a.mstride, M, col, cs, nan); break;
  }
  v[0] = v[1] = v[2] = 0.0;
  if (e.lanes & WBX_IVL_COVERED) {
    const wbx_ivl_lane& l = e.lane[0];
    const double lo = ivl_quantile<T>(col, cs, M, l.lo, nan), hi = ivl_quantile<T>(col, cs, M, l.hi, nan);
    const double t = (double)ld_stream(reinterpret_cast<const T*>(a.in[1]) + ro[1] + x * a.xstride[1]);
    v[0] = (lo <= t && t <= hi) ? 1.0 : 0.0;
  }
  if (e.lanes & WBX_IVL_CONFIDENT) {
    const wbx_ivl_lane& l = e.lane[1];
    const T* cp = reinterpret_cast<const T*>(a.in[2]) + ro[2] + x * a.xstride[2];
    const double lo = ivl_quantile<T>(col, cs, M, l.lo, nan), hi = ivl_quantile<T>(col, cs, M, l.hi, nan);
    const double c_lo = (double)cp[l.lo.c_off], c_hi = (double)cp[l.hi.c_off];
    const double spread = hi - lo, c_spread = c_hi - c_lo;
    const double scaled = l.threshold * c_spread;
    v[1] = spread < scaled ? 1.0 : 0.0;
  }
  if (e.lanes & WBX_IVL_JACCARD) {
    const wbx_ivl_lane& l = e.lane[2];
    const T* cp = reinterpret_cast<const T*>(a.in[2]) + ro[2] + x * a.xstride[2];
    const double a_lo = ivl_quantile<T>(col, cs, M, l.lo, nan), a_hi = ivl_quantile<T>(col, cs, M, l.hi, nan);
    const double b_lo = (double)cp[l.lo.c_off], b_hi = (double)cp[l.hi.c_off];
    // minimum / maximum hand a NaN on (fmin / fmax would drop it), clip(min=0) keeps one, union > 0 is false for one
    const bool any_nan = a_lo != a_lo || a_hi != a_hi || b_lo != b_lo || b_hi != b_hi;
    const double gap = any_nan ? __builtin_nan("") : fmin(a_hi, b_hi) - fmax(a_lo, b_lo);
    const double overlap = gap < 0.0 ? 0.0 : gap;
    const double wa = a_hi - a_lo, wb = b_hi - b_lo;
    const double both = wa + wb;
    const double uni = both - overlap;
    const double index = uni > 0.0 ? overlap / uni : 1.0;
    const double dist = 1.0 - index;
    v[2] = dist > l.threshold ? 1.0 : 0.0;
  }
}

// The sums of a lane's points: no value is ever NaN, so the count lane of a mask and the count lanes of skipna are one number.
struct IvlSums {
  double s[3] = {0.0, 0.0, 0.0}, c = 0.0;
};

__device__ __forceinline__ void ivl_account(const S1Args& a, const IvlArgs& e, const int64_t (&ro)[WBX_MAX_INPUTS], int64_t x,
                                            const double (&v)[3], IvlSums& acc) {
  const bool valid = !(a.flags & WBX_FLAG_MASKED) || reinterpret_cast<const uint8_t*>(a.in[3])[ro[3] + x * a.xstride[3]] != 0;
#pragma unroll
  for (int l = 0; l < 3; ++l) acc.s[l] += valid ? v[l] : 0.0;  // (s[l]: the lane with bit l; lanes not asked for add 0)
  acc.c += valid ? 1.0 : 0.0;
}

extern __shared__ __attribute__((aligned(16))) unsigned char ivl_lds[];  // [np][blockDim.x] elements of T

// x summed.  grid = nkey * nchunk; the waves of a block interleave over the chunk's rows, a lane sweeps a row 64 points apart.
template <typename T>
__global__ void __launch_bounds__(WASS_THREADS<T>) ivl_xr_kernel(S1Args a, IvlArgs e, int nacc) {
  T* col = reinterpret_cast<T*>(ivl_lds) + threadIdx.x;
  const int cs = blockDim.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwave = blockDim.x >> 6;
  const int64_t b = blockIdx.x;
  const int64_t key = b / a.nchunk;
  const int chunk = (int)(b - key * a.nchunk);
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<3>(a, key, kb);
  IvlSums acc;
  for (int64_t d = d0 + wave; d < d1; d += nwave) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<3>(a, kb, key, d, ro);
    for (int64_t x = lane; x < a.nx; x += 64) {
      double v[3] = {0.0, 0.0, 0.0};
      ivl_point<T>(a, e, ro, x, col, cs, v);
      ivl_account(a, e, ro, x, v, acc);
    }
  }
  __shared__ double red[2][4];
  const double w0 = wave_sum(acc.s[0]), w1 = wave_sum(acc.s[1]), w2 = wave_sum(acc.s[2]), wc = wave_sum(acc.c);
  if (lane == 0) {
    red[wave][0] = w0;
    red[wave][1] = w1;
    red[wave][2] = w2;
    red[wave][3] = wc;
  }
  __syncthreads();
  if ((int)threadIdx.x < nacc) {
    int src = 3;  // value lane j is the j-th requested bit; behind the value lanes the count lane(s)
    for (int l = 2, j = e.nval; l >= 0; --l)
      if ((e.lanes >> l) & 1) src = --j == (int)threadIdx.x ? l : src;
    double s = 0.0;
    for (int w = 0; w < nwave; ++w) s += red[w][src];
    a.out[(key * a.nchunk + chunk) * (int64_t)nacc + threadIdx.x] = s;
  }
}

// x kept.  grid = nkey * nxtile * nchunk; a lane owns one x and walks the chunk's rows.
template <typename T>
__global__ void __launch_bounds__(WASS_THREADS<T>) ivl_xk_kernel(S1Args a, IvlArgs e, int nacc) {
  T* col = reinterpret_cast<T*>(ivl_lds) + threadIdx.x;
  const int cs = blockDim.x;
  int64_t b = blockIdx.x;
  const int chunk = (int)(b % a.nchunk);
  b /= a.nchunk;
  const int xt = (int)(b % a.nxtile);
  const int64_t key = b / a.nxtile;
  const int64_t x = (int64_t)xt * blockDim.x + threadIdx.x;
  if (x >= a.nx) return;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  int64_t kb[WBX_MAX_INPUTS];
  key_bases<3>(a, key, kb);
  IvlSums acc;
  for (int64_t d = d0; d < d1; ++d) {
    int64_t ro[WBX_MAX_INPUTS];
    row_bases<3>(a, kb, key, d, ro);
    double v[3] = {0.0, 0.0, 0.0};
    ivl_point<T>(a, e, ro, x, col, cs, v);
    ivl_account(a, e, ro, x, v, acc);
  }
  double* o = a.out + ((key * a.nchunk + chunk) * (int64_t)nacc) * a.nx + x;
  int j = 0;  // value lane j is the j-th requested bit; behind the value lanes the count lane(s)
#pragma unroll
  for (int l = 0; l < 3; ++l)
    if ((e.lanes >> l) & 1) o[(int64_t)(j++) * a.nx] = acc.s[l];
  for (; j < nacc; ++j) o[(int64_t)j * a.nx] = acc.c;
}

// A block runs the plan's threads up to what the column store holds (WASS_THREADS); the partial's layout does not depend on it.
template <typename T>
static int ivl_launch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a, const IvlArgs& e, int nacc) {
  const int threads = plan->block_threads < WASS_THREADS<T> ? plan->block_threads : WASS_THREADS<T>;
  const size_t lds = (size_t)e.np * threads * sizeof(T);
  int64_t grid;
  if (int rc = s1_grid(plan, plan->x_kept ? threads : 0, a, &grid)) return rc;
  hipLaunchKernelGGL(plan->x_kept ? ivl_xk_kernel<T> : ivl_xr_kernel<T>, dim3((unsigned)grid), dim3(threads), lds, ctx->stream, a, e,
                     nacc);
  WBX_HIP(hipGetLastError());
  return 0;
}

}  // namespace wbx

extern "C" int wbx_ens_interval_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int lanes,
                                        const wbx_ivl_lane* params, const void* p, const void* t, const void* c, const uint8_t* mask,
                                        double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_ens_interval_partial: ", "partial_out", "p"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(M >= 1 && M <= WBX_IVL_MAX_MEMBERS, "wbx_ens_interval_partial: 1..%d members (got %d)", WBX_IVL_MAX_MEMBERS, M);
  const int all = WBX_IVL_COVERED | WBX_IVL_CONFIDENT | WBX_IVL_JACCARD;
  WBX_REQUIRE(lanes != 0 && !(lanes & ~all), "wbx_ens_interval_partial: lanes must be a non-empty set of WBX_IVL_* bits (got 0x%x)", lanes);
  WBX_REQUIRE(params != nullptr, "wbx_ens_interval_partial: params is NULL");
  IvlArgs e;
  memset(&e, 0, sizeof(e));
  for (int l = 0; l < 3; ++l) {
    if (!(lanes & (1 << l))) continue;
    e.lane[l] = params[l];
    for (const wbx_ivl_bound* b : {&params[l].lo, &params[l].hi}) {
      WBX_REQUIRE(b->k >= 0 && b->k < M, "wbx_ens_interval_partial: rank %d outside 0..%d", (int)b->k, M - 1);
      WBX_REQUIRE(b->g >= 0.0 && b->g < 1.0, "wbx_ens_interval_partial: weight %g outside [0, 1)", b->g);
    }
    ++e.nval;
  }
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_ens_interval_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "wbx_ens_interval_partial: flags other than MASKED | SKIPNA (0x%x)",
              plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_ens_interval_partial: no plane mode, no folded x weights");
  const bool empty = plan->nkey == 0 || plan->ndepth == 0 || plan->nx == 0;
  WBX_REQUIRE(empty || t != nullptr || !(lanes & WBX_IVL_COVERED), "wbx_ens_interval_partial: Covered asked for but t is NULL");
  WBX_REQUIRE(empty || c != nullptr || !(lanes & (WBX_IVL_CONFIDENT | WBX_IVL_JACCARD)),
              "wbx_ens_interval_partial: a lane needs the climatology but c is NULL");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 1, p, t, mask, partial_out, a)) return rc;
  a.in[2] = c;
  const int nacc = (int)partial_lanes(plan->flags, e.nval);
  bool done;
  if (int rc = s1_zero_if_empty(ctx, plan, nacc, partial_out, &done); rc || done) return rc;
  a.M = M;
  a.mstride = member_stride;
  e.lanes = lanes;
  e.np = ivl_padded(M);
  if (dtype == WBX_F32) return ivl_launch<float>(ctx, plan, a, e, nacc);
  return ivl_launch<double>(ctx, plan, a, e, nacc);
}
