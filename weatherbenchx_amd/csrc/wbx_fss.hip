// The three terms of the fractions skill score -- (Pf - Tf)^2, Pf^2, Tf^2 with Pf, Tf the n x n neighbourhood means of p and t -- as
// ONE stage-1 partial, from one sweep over p and t (include/wbx.h has the contract in full).
//
// Reference semantics restated (weatherbenchX/metrics/spatial.py:24-277): the reference convolves every (latitude, longitude) field
// with n taps along each axis, three statistics call it four times per size, and the Aggregator then reduces three float32 fields.
// Here a block of 256 threads owns one (key, depth chunk, band of B output latitudes) and whole longitude circles:
//   * thread l owns the columns l + 256 c, c < NC = ceil(nlon / 256): a wave's row loads are coalesced where lon_stride == 1;
//   * per owned column the VERTICAL window sums of p and t (double, NaN members as 0) and their NaN counts (int) live in
//     registers and slide down the band: the entering row is added, the leaving row subtracted, so a row is read twice (the second
//     time from cache) plus a halo of n - 1 rows per band;
//   * per output row the column values go through a block-wide inclusive prefix over the circle (every thread the serial prefix
//     of a run of NC adjacent columns, one wave scan of the run totals by shuffles, the four wave totals combined in order through
//     LDS), and a point's HORIZONTAL window is a difference of two prefix values, the circle's total added or subtracted where
//     the window wraps the date line.  The two NaN counts travel packed in
//     one 64-bit integer (each stays below 2^32);
//   * the three float32 squares (and the count lanes) are summed over x in a fixed order -- thread, wave shuffles, the waves' own
//     LDS slots -- and over the chunk's fields in field order; x kept: the owning thread adds field after field into its output.
// The cost per point does not depend on n.  No atomics; every sum runs in a fixed order.
#include "wbx_fss.hpp"

namespace wbx {

// grid = nkey * nchunk * nband, block = 256.  N1: n == 1 (no window, no border).
template <typename T, int NC, bool N1>
__global__ void __launch_bounds__(FSS_THREADS) fss_kernel(FssArgs a) {
  using F = std::conditional_t<N1, T, float>;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t b = blockIdx.x;
  const int band = (int)(b % a.nband);
  b /= a.nband;
  const int chunk = (int)(b % a.nchunk);
  const int64_t key = b / a.nchunk;
  const int64_t d0 = (int64_t)chunk * a.dchunk;
  const int64_t d1 = d0 + a.dchunk < a.D ? d0 + a.dchunk : a.D;
  const int nlat = a.nlat, nlon = a.nlon, n = a.n, h = (n - 1) / 2;
  const int y0 = band * a.B, y1 = y0 + a.B < nlat ? y0 + a.B : nlat;
  const int ys = y0 > h ? y0 : h, ye = y1 < nlat - h ? y1 : nlat - h;  // the band's rows that are no border rows: [ys, ye)
  const bool masked = a.flags & WBX_FLAG_MASKED, skipna = a.flags & WBX_FLAG_SKIPNA;
  const int nacc = skipna ? 2 * WBX_FSS_LANES : (masked ? WBX_FSS_LANES + 1 : WBX_FSS_LANES);
  const double area = (double)n * (double)n;

  constexpr int NS = N1 ? 1 : NC * FSS_THREADS;
  __shared__ double sP[NS], sT[NS];
  __shared__ unsigned long long sH[NS];
  __shared__ double wP[1][FSS_WAVES], wT[1][FSS_WAVES];
  __shared__ unsigned long long wH[1][FSS_WAVES];
  __shared__ double racc[FSS_BMAX][FSS_WAVES][FSS_NACC];  // x summed: slot [row][wave] belongs to lane 0 of that wave

  if (!a.x_kept) {
    for (int i = tid; i < FSS_BMAX * FSS_WAVES * FSS_NACC; i += FSS_THREADS) (&racc[0][0][0])[i] = 0.0;
    __syncthreads();
  }

  int64_t kb[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) kb[i] = a.key_off[i] ? a.key_off[i][key] : 0;
  const T* pin = reinterpret_cast<const T*>(a.in[0]);
  const T* tin = reinterpret_cast<const T*>(a.in[1]);
  const uint8_t* min_ = reinterpret_cast<const uint8_t*>(a.in[2]);

  for (int64_t d = d0; d < d1; ++d) {
    int64_t base[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) base[i] = kb[i] + (a.depth_off[i] ? a.depth_off[i][d] : 0);

    // the vertical window sums of the owned columns
    double cp[NC], ct[NC];
    int hp[NC], ht[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      cp[c] = ct[c] = 0.0;
      hp[c] = ht[c] = 0;
    }
    auto slide = [&](int r, int sign) {  // row r enters (sign = 1) or leaves (sign = -1); 0 <= r < nlat
      const int64_t rp = base[0] + (int64_t)r * a.lat_stride[0], rt = base[1] + (int64_t)r * a.lat_stride[1];
      T pv[NC], tv[NC];
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int x = tid + c * FSS_THREADS;
        const int xs = x < nlon ? x : nlon - 1;  // (columns past the circle re-read its last point and are dropped below)
        pv[c] = pin[rp + (int64_t)xs * a.lon_stride[0]];
        tv[c] = tin[rt + (int64_t)xs * a.lon_stride[1]];
      }
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const bool in = tid + c * FSS_THREADS < nlon;
        const bool pn = pv[c] != pv[c], tn = tv[c] != tv[c];
        cp[c] += (in && !pn) ? (double)pv[c] * sign : 0.0;
        ct[c] += (in && !tn) ? (double)tv[c] * sign : 0.0;
        hp[c] += (in && pn) ? sign : 0;
        ht[c] += (in && tn) ? sign : 0;
      }
    };
    if constexpr (!N1) {
      if (ys < ye)
        for (int r = ys - h; r < ys + h; ++r) slide(r, 1);
    }

    for (int y = y0; y < y1; ++y) {
      F pf[NC], tf[NC];
      const bool brow = !N1 && (y < h || y >= nlat - h);  // block-uniform
      if constexpr (N1) {
        const int64_t rp = base[0] + (int64_t)y * a.lat_stride[0], rt = base[1] + (int64_t)y * a.lat_stride[1];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int x = tid + c * FSS_THREADS;
          const int xs = x < nlon ? x : nlon - 1;
          pf[c] = pin[rp + (int64_t)xs * a.lon_stride[0]];
          tf[c] = tin[rt + (int64_t)xs * a.lon_stride[1]];
        }
      } else if (brow) {
#pragma unroll
        for (int c = 0; c < NC; ++c) pf[c] = tf[c] = 0.f;
      } else {
        slide(y + h, 1);
        // inclusive prefix over the circle.  The column sums go to LDS at their own positions; thread `tid` then takes the RUN
        // [NC tid, NC tid + NC) of the circle (padded with zeros to 256 NC columns), forms the run's prefix serially, the block
        // scans the 256 run totals (one wave scan by shuffles, the four wave totals in order through LDS), and the run goes back.
        // Four barriers per row.  This first one closes the previous row (or field): its window reads below take OTHER threads'
        // prefix values out of sP / sT / sH, and the stores that follow overwrite other threads' positions.
        __syncthreads();
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int x = tid + c * FSS_THREADS;  // < NC * 256: inside the arrays
          sP[x] = cp[c];
          sT[x] = ct[c];
          sH[x] = (unsigned long long)(uint32_t)hp[c] | ((unsigned long long)(uint32_t)ht[c] << 32);
        }
        __syncthreads();
        double lp[NC], lt[NC];
        unsigned long long lh[NC];
        {
          double rp = 0.0, rt = 0.0;
          unsigned long long rh = 0;
#pragma unroll
          for (int j = 0; j < NC; ++j) {
            rp += sP[tid * NC + j];
            rt += sT[tid * NC + j];
            rh += sH[tid * NC + j];
            lp[j] = rp;
            lt[j] = rt;
            lh[j] = rh;
          }
          // the sum of the runs in front of this one: the wave's inclusive scan shifted by a lane, then the waves in front
          const double ip = fss_wave_scan(rp, lane), it = fss_wave_scan(rt, lane);
          const unsigned long long ih = fss_wave_scan(rh, lane);
          if (lane == 63) {
            wP[0][wave] = ip;
            wT[0][wave] = it;
            wH[0][wave] = ih;
          }
          double op = __shfl_up(ip, 1, 64), ot = __shfl_up(it, 1, 64);
          unsigned long long oh = __shfl_up(ih, 1, 64);
          if (lane == 0) {
            op = ot = 0.0;
            oh = 0;
          }
          __syncthreads();
          double bp = 0.0, bt = 0.0;
          unsigned long long bh = 0;
#pragma unroll
          for (int w = 0; w < FSS_WAVES; ++w) {
            if (w < wave) {
              bp += wP[0][w];
              bt += wT[0][w];
              bh += wH[0][w];
            }
          }
          op += bp;
          ot += bt;
          oh += bh;
#pragma unroll
          for (int j = 0; j < NC; ++j) {  // (the thread's own run: nobody else reads it before the barrier below)
            sP[tid * NC + j] = op + lp[j];
            sT[tid * NC + j] = ot + lt[j];
            sH[tid * NC + j] = oh + lh[j];
          }
        }
        __syncthreads();
        const double totp = sP[nlon - 1], tott = sT[nlon - 1];
        const unsigned long long toth = sH[nlon - 1];
#pragma unroll
        for (int c = 0; c < NC; ++c) {
          const int x = tid + c * FSS_THREADS;
          pf[c] = tf[c] = 0.f;
          if (x < nlon && (a.wrap || (x >= h && x < nlon - h))) {
            int lo = x - h - 1, hi = x + h;  // the window is (lo, hi] of the extended prefix
            const bool wlo = lo < 0, whi = hi >= nlon;
            lo = wlo ? lo + nlon : lo;  // n <= nlon: back inside [0, nlon)
            hi = whi ? hi - nlon : hi;
            double s_p = sP[hi] - sP[lo], s_t = sT[hi] - sT[lo];
            unsigned long long s_h = sH[hi] - sH[lo];
            if (wlo) {
              s_p += totp;
              s_t += tott;
              s_h += toth;
            }
            if (whi) {
              s_p += totp;
              s_t += tott;
              s_h += toth;
            }
            const float nanf_ = __builtin_nanf("");
            pf[c] = (uint32_t)s_h != 0 ? nanf_ : (float)(s_p / area);
            tf[c] = (uint32_t)(s_h >> 32) != 0 ? nanf_ : (float)(s_t / area);
          }
        }
        slide(y - h, -1);
      }

      // the row's lanes
      double acc[FSS_NACC];
#pragma unroll
      for (int l = 0; l < FSS_NACC; ++l) acc[l] = 0.0;
      const int64_t rm = masked ? base[2] + (int64_t)y * a.lat_stride[2] : 0;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        const int x = tid + c * FSS_THREADS;
        const bool in = x < nlon;
        double v[WBX_FSS_LANES];
        fss_lanes<F>(pf[c], tf[c], v);
        bool valid = true;
        if (masked) valid = min_[rm + (int64_t)(in ? x : nlon - 1) * a.lon_stride[2]] != 0;
        double one[FSS_NACC];
#pragma unroll
        for (int l = 0; l < FSS_NACC; ++l) one[l] = 0.0;
#pragma unroll
        for (int l = 0; l < WBX_FSS_LANES; ++l) {
          const double val = valid ? v[l] : 0.0;  // a masked-out point contributes exactly 0 whatever it holds
          if (skipna) {
            const bool fin = !(val != val);
            one[l] = fin ? val : 0.0;
            one[WBX_FSS_LANES + l] = (fin && valid) ? 1.0 : 0.0;
          } else {
            one[l] = val;
          }
        }
        if (masked && !skipna) one[WBX_FSS_LANES] = valid ? 1.0 : 0.0;
        if (a.x_kept) {
          if (in) {
            double* o = a.out + (((key * nlat + y) * a.nchunk + chunk) * (int64_t)nacc) * nlon + x;
#pragma unroll
            for (int l = 0; l < FSS_NACC; ++l) {
              if (l < nacc) {
                double* q = o + (int64_t)l * nlon;
                *q = d == d0 ? one[l] : *q + one[l];  // the thread owns the element: field after field
              }
            }
          }
        } else {
#pragma unroll
          for (int l = 0; l < FSS_NACC; ++l) acc[l] += in ? one[l] : 0.0;
        }
      }
      if (!a.x_kept) {
#pragma unroll
        for (int l = 0; l < FSS_NACC; ++l) {
          const double s = wave_sum(acc[l]);
          if (lane == 0) racc[y - y0][wave][l] += s;
        }
      }
    }
  }

  if (a.x_kept && d0 >= d1) {  // a chunk without fields (a plan whose chunks overshoot the depth): zeros
    for (int y = y0; y < y1; ++y)
      for (int l = 0; l < nacc; ++l)
        for (int x = tid; x < nlon; x += FSS_THREADS)
          a.out[((((key * nlat + y) * a.nchunk + chunk) * (int64_t)nacc) + l) * nlon + x] = 0.0;
  }
  if (!a.x_kept) {
    __syncthreads();
    for (int i = tid; i < (y1 - y0) * nacc; i += FSS_THREADS) {
      const int j = i / nacc, l = i - j * nacc;
      double s = 0.0;
#pragma unroll
      for (int w = 0; w < FSS_WAVES; ++w) s += racc[j][w][l];
      a.out[((key * nlat + (y0 + j)) * a.nchunk + chunk) * (int64_t)nacc + l] = s;
    }
  }
}

template <typename T, bool N1>
static int fss_launch(wbx_ctx* ctx, const FssArgs& a, int64_t grid) {
  const int nc = (a.nlon + FSS_THREADS - 1) / FSS_THREADS;
  void (*k)(FssArgs) = nc <= 1   ? fss_kernel<T, 1, N1>
                       : nc <= 2 ? fss_kernel<T, 2, N1>
                       : nc <= 4 ? fss_kernel<T, 4, N1>
                       : nc <= 6 ? fss_kernel<T, 6, N1>
                                 : fss_kernel<T, 8, N1>;
  hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(FSS_THREADS), 0, ctx->stream, a);
  WBX_HIP(hipGetLastError());
  return 0;
}

}  // namespace wbx

extern "C" int wbx_fss_partial(wbx_ctx* ctx, const wbx_fss_plan* plan, int dtype, int n, const void* p, const void* t,
                               const uint8_t* mask, double* partial_out) {
  using namespace wbx;
  if (const int rc = fss_check("wbx_fss_partial", ctx, plan, dtype, n, p, t, mask, partial_out)) return rc;
  const bool empty = fss_empty(plan);
  if (plan->nkey == 0) return 0;
  WBX_HIP(hipSetDevice(ctx->device));
  const int64_t nacc = (plan->flags & WBX_FLAG_SKIPNA) ? 2 * WBX_FSS_LANES
                                                       : ((plan->flags & WBX_FLAG_MASKED) ? WBX_FSS_LANES + 1 : WBX_FSS_LANES);
  if (empty) {
    const size_t cnt = (size_t)plan->nkey * plan->nlat * plan->nchunk * nacc * (size_t)(plan->x_kept ? plan->nlon : 1);
    if (cnt) WBX_HIP(hipMemsetAsync(partial_out, 0, cnt * sizeof(double), ctx->stream));
    return 0;
  }
  FssArgs a = fss_args(plan, n, p, t, mask, partial_out);
  const int B = fss_band_rows(plan, n);
  a.B = B;
  a.nband = (a.nlat + B - 1) / B;
  const int64_t grid = plan->nkey * plan->nchunk * a.nband;
  WBX_REQUIRE(grid < (int64_t)1 << 31, "wbx_fss_partial: grid too large (%lld blocks)", (long long)grid);
  if (n == 1) return dtype == WBX_F32 ? fss_launch<float, true>(ctx, a, grid) : fss_launch<double, true>(ctx, a, grid);
  return dtype == WBX_F32 ? fss_launch<float, false>(ctx, a, grid) : fss_launch<double, false>(ctx, a, grid);
}
