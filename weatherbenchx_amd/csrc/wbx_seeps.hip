// SEEPS (stable equitable error in probability space) for the stage-1 skeleton (wbx_s1.hpp): one more Op.
//
// Reference semantics restated (weatherbenchX/metrics/categorical.py:104-304; include/wbx.h has the contract in full).  Forecast
// and observation are each dry / light / heavy against the dry threshold and the place's climatological wet threshold at the valid
// time, and the pair is charged an entry of a 3 x 3 matrix whose entries depend on the climatological dry fraction p1 of the place.
// The reference forms six float64 indicator fields, multiplies them pairwise with six broadcast coefficient fields, adds the six
// products and blanks places whose p1 is out of range.  At most one of the six products has two non-zero indicators, so the sum is a
// function of (category of p, category of t, place): the host evaluates the reference's own expression once per category pair and
// place into a table T[3][3][place] of float64 (categorical.seeps_score_table), with everything that expression does to a p1 of 0,
// 1, NaN or outside the range, and the kernel LOOKS THE SCORE UP.  It never sees p1 and does no arithmetic on the score.
//
// Per point: p, t and the gathered wet threshold are streamed (12 B for float32), the two categories are three compares each in the
// input type, and one float64 is read from the table at input 2's row address without the gather term -- the table is 9 places
// large and a place is met once per time step, so those 8 B come from cache.  The sum is the skeleton's: float64, fixed order, no
// atomics.
#include "wbx_s1.hpp"

namespace wbx {

// MM as in wbx_det.hip: 0 = no count lane, 1 = mask only, 2 = skipna, 3 = skipna under a mask (one value lane: one count lane).
template <typename T, int MM>
struct SeepsOp {
  static constexpr int NIN = 3;
  static constexpr int NLANE = WBX_SEEPS_LANES;
  static constexpr int NACC = NLANE + (MM == 0 ? 0 : 1);
  static constexpr bool HAS_MASK = MM == 1 || MM == 3;
  static constexpr bool PLAIN_ROW2 = true;  // ro[WBX_MAX_INPUTS]: the table's row
  static constexpr int XR_UNROLL = 2, XK_UNROLL = 4, MIN_WAVES = 1;

  // 0 dry, 1 light, 2 heavy; "none" (a NaN w under a value that is not dry; a NaN v) is 0 as well: with a NaN w the other value of
  // the point is dry or none too, so the point takes cell (0, 0) either way.  Dry is tested first (the header's precondition makes
  // the three conditions exclusive).
  __device__ __forceinline__ static int category(T v, T w, T dry) { return v <= dry ? 0 : (v < w ? 1 : (v >= w ? 2 : 0)); }

  template <int V, bool XK>
  __device__ __forceinline__ static void accum(const S1Args& a, const int64_t (&ro)[WBX_MAX_INPUTS + 1], int64_t x,
                                               double (&acc)[XK ? V : 1][NACC]) {
    T p[V], t[V], w[V];
    uint8_t m[V];
    load_x<T, V>(a.in[0], ro[0], x, a.xstride[0], p);
    load_x<T, V>(a.in[1], ro[1], x, a.xstride[1], t);
    load_x<T, V>(a.in[2], ro[2], x, a.xstride[2], w);
    if constexpr (HAS_MASK) load_x<uint8_t, V>(a.in[3], ro[3], x, a.xstride[3], m);
    const T dry = (T)a.dry;  // round to nearest: what NumPy and torch compare a float32 array with
    const double* row = a.table + ro[WBX_MAX_INPUTS];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int cell = 3 * category(p[k], w[k], dry) + category(t[k], w[k], dry);
      const double entry = row[(x + k) * a.xstride[2] + cell * a.cell_stride];  // (cached: the place comes back every time step)
      const bool nan_in = p[k] != p[k] || t[k] != t[k];
      double val = nan_in ? __builtin_nan("") : entry;
      bool valid = true;
      if constexpr (HAS_MASK) {
        valid = m[k] != 0;
        val = valid ? val : 0.0;  // a masked-out point contributes exactly 0 whatever its entry is
      }
      double(&A)[NACC] = acc[XK ? k : 0];
      if constexpr (MM <= 1) {
        A[0] += val;
        if constexpr (MM == 1) A[1] += valid ? 1.0 : 0.0;
      } else {
        const bool fin = !(val != val);
        A[0] += fin ? val : 0.0;
        A[1] += (fin && valid) ? 1.0 : 0.0;
      }
    }
  }
};

// x kept: one x per lane whatever plan->vec says (four x per lane are four table gathers in flight and four accumulator pairs).
template <typename T, int MM>
static int seeps_launch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a) {
  using Op = SeepsOp<T, MM>;
  if (plan->vec == 4 && !plan->x_kept) return launch_partial<Op, 4, false>(ctx, plan, a);  // (no x-kept kernel of four x per lane is built)
  return launch_partial<Op, 1>(ctx, plan, a);
}

template <typename T>
static int seeps_dispatch(wbx_ctx* ctx, const wbx_s1_plan* plan, S1Args& a) {
  const bool masked = plan->flags & WBX_FLAG_MASKED;
  if (plan->flags & WBX_FLAG_SKIPNA) return masked ? seeps_launch<T, 3>(ctx, plan, a) : seeps_launch<T, 2>(ctx, plan, a);
  return masked ? seeps_launch<T, 1>(ctx, plan, a) : seeps_launch<T, 0>(ctx, plan, a);
}

}  // namespace wbx

extern "C" int wbx_seeps_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, double dry_threshold, const void* p, const void* t,
                                 const void* wet, const double* table, int64_t cell_stride, const uint8_t* mask,
                                 double* partial_out) {
  using namespace wbx;
  const S1Names names = {"wbx_seeps_partial: ", "partial_out", "p/t"};
  if (int rc = s1_begin(names.who, ctx, plan)) return rc;
  WBX_REQUIRE(dtype == WBX_F32 || dtype == WBX_F64, "wbx_seeps_partial: unknown dtype %d", dtype);
  WBX_REQUIRE(!(plan->flags & ~(WBX_FLAG_MASKED | WBX_FLAG_SKIPNA)), "wbx_seeps_partial: flags other than MASKED | SKIPNA (0x%x)",
              plan->flags);
  WBX_REQUIRE(plan->plane_rows == 0 && plan->x_weights == nullptr, "wbx_seeps_partial: no plane mode, no folded x weights");
  WBX_REQUIRE(p != nullptr && t != nullptr, "wbx_seeps_partial: p/t is NULL");
  WBX_REQUIRE(wet != nullptr, "wbx_seeps_partial: wet is NULL");
  WBX_REQUIRE(table != nullptr, "wbx_seeps_partial: table is NULL");
  S1Args a;
  if (int rc = s1_operands(names, ctx, plan, 2, p, t, mask, partial_out, a)) return rc;
  a.in[2] = wet;
  a.table = table;
  a.cell_stride = cell_stride;
  a.dry = dry_threshold;
  // (x kept with vec = 4: check_plan has seen unit / zero x strides; the launch below reads one x per lane all the same)
  if (dtype == WBX_F32) return seeps_dispatch<float>(ctx, plan, a);
  return seeps_dispatch<double>(ctx, plan, a);
}
