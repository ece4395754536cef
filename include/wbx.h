/*
 * wbx.h -- C ABI of libwbx_hip.so, the MI355X (gfx950) engine behind the
 * WeatherBench-X scoring hot path (Statistic.compute -> Aggregator reduce).
 *
 * The reference (google-research/weatherbenchX) is pure Python: the "FFI" a
 * maintainer would bind is the set of whole-array xarray/NumPy calls inside
 * the plugin classes.  Every entry point below names the reference call
 * site(s) it replaces (paths relative to the reference checkout).
 *
 * Conventions
 *  - plain C types only; all data pointers are DEVICE pointers unless the
 *    name says host (`h_`); the caller owns every buffer.
 *  - every function returns 0 on success or a negative wbx_status; the
 *    message is retrievable with wbx_last_error() (thread local).
 *  - all work is enqueued on the context's HIP stream and is asynchronous;
 *    wbx_ctx_synchronize() (or reading through wbx_memcpy_d2h) orders it.
 *  - a context is single-threaded; distinct contexts are independent.
 *
 * Two-stage reduction:
 *   stage 1  (HBM-bound)  per-point statistics fused with an UNWEIGHTED partial
 *            sum over every reduced dimension that weights/bin masks do not
 *            depend on -> fp64 partial[key][chunk][lane][j]
 *   stage 2  (tiny)       partial (x) W, W = product of weights and bin masks,
 *            -> sum_weighted_statistics / sum_weights accumulators.
 */
#ifndef WBX_H_
#define WBX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WBX_ABI_VERSION 13

typedef enum wbx_status {
  WBX_OK = 0,
  WBX_ERR_INVALID = -1,    /* bad argument / unsupported combination */
  WBX_ERR_HIP = -2,        /* a HIP runtime call failed              */
  WBX_ERR_NO_DEVICE = -3,  /* no gfx950 device visible               */
  WBX_ERR_FFT = -4,        /* rocFFT failure                         */
  WBX_ERR_RCCL = -5        /* RCCL missing or a collective failed    */
} wbx_status;

typedef struct wbx_ctx wbx_ctx; /* opaque: device id, stream, timers, scratch */

/* element type of the statistic inputs */
typedef enum wbx_dtype { WBX_F32 = 0, WBX_F64 = 1 } wbx_dtype;

/* ---- fused per-point statistic families ---------------------------------
 * Lane order is part of the ABI.
 * WBX_DET3  inputs (p,t):    e=p-t, |e|, e^2
 *           replaces deterministic.py:91-123 (Error, AbsoluteError, SquaredError)
 * WBX_DET6  inputs (p,t,c):  e, |e|, e^2, (p-c)^2, (t-c)^2, (p-c)(t-c)
 *           + deterministic.py:222-259 (SquaredPredictionAnomaly,
 *           SquaredTargetAnomaly, AnomalyCovariance); c is gathered through
 *           the plan's gather table (metrics/base.py:382-406 `.sel(dayofyear,hour)`)
 * WBX_PASS1 input (p):       p          (any already-materialised statistic;
 *           replaces the xr.dot of aggregation.py:335 for user-defined stats)
 * Accuracy, per output of wbx_det_partial against the exact sum of the exact lane values of the widened inputs: the inputs are
 * widened to float64 exactly, a lane value carries at most 3 roundings and the N terms of a partial are summed in float64 in a fixed
 * order (fused multiply-adds where x_weights are folded in), so |error| <= (N + 3) 2^-53 sum |term|, the weights included in the
 * terms, N = the points of the partial.  Inputs whose terms and partial sums are exact in float64 (small integers, weights k / 8)
 * give the same bits on every route: s1_xr with vec 1 / vec 4 / the mask row in LDS, s1_xk, plane mode, the flat x-weighted sweep.
 * Count lanes without x_weights are exact integers.  wbx_det_map: the lane value itself, at most 3 roundings.
 * Values that are not finite follow IEEE arithmetic of the formulas: without flags a NaN input makes the value lanes that read it
 * NaN in its own partial (its key, chunk and, where x is kept, x) and in no other; an infinite input gives +-inf there, NaN where
 * opposite infinities meet.  Under WBX_FLAG_MASKED a point whose mask byte is 0 contributes exactly 0 to every lane whatever it
 * holds, NaN and infinities included, and a count lane is never NaN.  Under WBX_FLAG_SKIPNA a NaN lane value is left out of its
 * own lane's sum and count (a NaN climatology alone drops lanes 3-5 of the point and keeps 0-2; a lane without a counted point
 * has sum 0 and count 0); an infinite lane value is kept.  tests/test_gpu_det_partial.py holds every line of this paragraph
 * output by output, on every kernel the dispatch can take, against the float64 restatement of tests/det_partial_cases.py.
 */
typedef enum wbx_det_func { WBX_DET3 = 0, WBX_DET6 = 1, WBX_PASS1 = 2 } wbx_det_func;
#define WBX_DET3_LANES 3
#define WBX_DET6_LANES 6
#define WBX_PASS1_LANES 1

/* ensemble lanes (probabilistic.py:116-336, wrappers.py:116-148):
 *  0 CRPSSkill            mean_m |p_m - t|
 *  1 CRPSSpread           sum_{m,m'} |p_m - p_m'| / (M (M - fair))
 *  2 EnsembleVariance     var_m(p, ddof=1)
 *  3 UnbiasedEnsembleMeanSquaredError  (mean_m p - t)^2 - var/M
 *  4 SquaredError of the ensemble mean (mean_m p - t)^2   (EnsembleMean + SquaredError)
 * Accuracy per point against the float64 restatement of the float32 members.  tests/test_gpu_ensemble_points.py holds every
 * line below per point, on every kernel that computes the lanes (wbx_ens_map, s1_xk / s1_xr / s1_xf1_kernel, ens_pipe_kernel and
 * its FLAT flavour, the masked / skipna wrappers, ens_atoms_kernel), with the bounds computed per point from the inputs
 * (tests/ensemble_cases.py); tests/test_gpu_round4.py holds outputs of 64 points and whole fields (geopotential-like
 * 5.5e4 +- 30, spread = 0.05 x error, a target at the ensemble mean).  u = 2^-24, eps = 2^-52; e_i = x_i - s about the shift
 * s of the kernel; A = mean |e_i|, Q = sum e_i^2 / (M - 1).
 * The rank-form fp32 kernels for M = 50 / 51 (ens_pipe_kernel, ens_atoms_kernel) sum e = x - median in fp32 chains of <= 8
 * terms, every chain of non-negative terms (s = the sorted median):
 *   lanes 0, 1      relative: <= 9 u = 5.4e-7 worst case, ~1e-7 typical
 *   lane 2          absolute: |d var| <= 9 u Q, Q <= 3 var (the subtraction (sum e)^2 / M is fp64)
 *   lane 4          = (mean_m p - t)^2 is the square of a DIFFERENCE: bounded absolutely, not relatively.  The mean error
 *                   carries d <= 9 u A, so |d lane4| <= 2 sqrt(lane 4) d + d^2; where the target sits near the ensemble mean
 *                   the relative error of lane 4 is unbounded (0.2 on N(0, 1) members, 3e2 on a target within 1e-4 of the mean)
 *   lane 3          a difference of lane 4 and lane 2 / M: |d lane3| <= (lane-4 bound) + (lane-2 bound) / M;
 *                   <= 1e-6 (lane 4 + lane 2 / M) on physical fields (tests/test_gpu_round4.py)
 * A point outside the fp32 range of these sums (member range not 0 and outside [2^-50, 2^60], a member or target magnitude above
 * 2^100, an infinite target included) sends its whole 64-lane tile through the generic fp64 operator instead (wave-uniform; the
 * tighter row below).  A NaN target does not: the magnitude test drops it (fmaxf) and the chains carry the NaN into lanes 0, 3, 4.
 * Every other ensemble kernel sums in fp64 on the widened members: padded buckets, wrappers and wbx_ens_map (M = 50 / 51
 * included) with s = the target, or the smallest member when the target is NaN / infinite; the generic operator (M > 64,
 * float64) with s = the first member in memory, whatever the target is:
 *   lane 0          relative (M + 4) eps;   lane 1  absolute 2 (M + 4) eps A (generic: relative (M + 4) eps);
 *   lane 2          absolute (M + 6) eps Q; lane 4  as above with d = (M + 4) eps A (generic: (M + 4) eps A + 2 eps |s - t|);
 *   lane 3          as above;   pair form (WBX_ENS_PAIRWISE, M <= 64): lane 1 relative (M + 1) u, its |x_i - x_j| rows are fp32.
 * Members and targets that are not finite:
 *   float32 rank form, M <= 64: a NaN OR INFINITE member makes all five lanes NaN.  Pair form, M > 64 and float64: plain IEEE
 *   arithmetic of the formulas on e = x - s, the pairs summed over i > j -- one infinite member gives lanes 0, 1, 4 = +inf and
 *   lanes 2, 3 = NaN (two of the same sign: lane 1 NaN too); on the generic operator an infinite FIRST member in memory is the
 *   shift itself and turns lane 4 NaN as well.  A NaN / infinite target leaves lanes 1 and 2 finite on every route.
 *   M = 1: lanes 2 and 3 are NaN (ddof = 1), the fair spread is NaN and the unfair spread 0. */
#define WBX_ENS_LANES 5
typedef enum wbx_ens_algo {
  WBX_ENS_SORT = 0,     /* rank / sorting-network form, probabilistic.py:214-240 (use_sort=True)  */
  WBX_ENS_PAIRWISE = 1  /* O(M^2) pairwise form,        probabilistic.py:241-247 (use_sort=False) */
} wbx_ens_algo;

#define WBX_FLAG_MASKED 1u /* input 3 (uint8 mask, nonzero = valid) is present: aggregation.py:339-352 */
#define WBX_FLAG_SKIPNA 2u /* NaN statistic values are dropped and counted out: aggregation.py:353-355 */
#define WBX_FLAG_FAIR   4u /* ensemble: fair CRPS spread (divide by M(M-1)):   probabilistic.py:239,247 */
#define WBX_FLAG_SKIPNA_ENS 8u /* ensemble: NaN members are missing members (skipna_ensemble=True), per-point
                                  ensemble size = count of non-NaN members: probabilistic.py:143-145,206-216,303-336.
                                  float32, M <= 64: members in registers, NaN -> +inf, sorted, rank form over the first n
                                  (either `algo`: the same number); otherwise the pair form over members re-read from memory */

#define WBX_MAX_INPUTS 4 /* 0 = predictions, 1 = targets, 2 = climatology, 3 = mask(uint8) */

/* Stage-1 plan.  The host flattens the statistic's index space into
 *   key   : every (key) index gets its own partial sum      [nkey]
 *   depth : summed inside stage 1, split in nchunk chunks   [ndepth]
 *   x     : the innermost, thread-mapped dimension          [nx]
 * and hands the kernel per-input ELEMENT offset tables, so any dim order /
 * any stride (the loaders' layout is arbitrary, data_loaders/xarray_loaders.py:185-188)
 * is consumed in place, without a transposed copy.
 * element address of input i at (key k, depth d, x):
 *     in[i] + key_off[i][k] + depth_off[i][d] + x * xstride[i]
 *     (+ gather_tab[gather_key[k] * n_gather_depth + gather_depth[d]] for i == 2)
 * All table pointers are device pointers; a NULL table means all zeros.
 */
typedef struct wbx_s1_plan {
  int64_t nkey;
  int64_t ndepth;
  int64_t nx;
  int32_t x_kept;        /* 1: keep one partial per x (nj = nx); 0: sum x away (nj = 1) */
  int32_t nchunk;        /* depth is cut into nchunk pieces of depth_chunk rows          */
  int64_t depth_chunk;
  int64_t xstride[WBX_MAX_INPUTS];
  const int64_t* key_off[WBX_MAX_INPUTS];   /* [nkey]   */
  const int64_t* depth_off[WBX_MAX_INPUTS]; /* [ndepth] */
  const int32_t* gather_key;   /* [nkey]   or NULL */
  const int32_t* gather_depth; /* [ndepth] or NULL */
  const int64_t* gather_tab;   /* [n_gather_key * n_gather_depth] or NULL */
  int32_t n_gather_depth;
  uint32_t flags;        /* WBX_FLAG_* */
  int32_t block_threads; /* 64, 128 or 256 */
  int32_t vec;           /* 1 or 4: x elements per lane per load (4 needs 16-B alignment of every row) */
  int32_t plane_rows;    /* 0, or R > 0 ("plane mode", x kept, deterministic families, fp32): every group of R consecutive
                            depth rows starting at a multiple of R is ONE contiguous span of R*nx elements in every input
                            (latitude-fastest chunks: rows = longitudes). The span is fetched with aligned 16-B loads
                            through LDS instead of ragged per-row dword loads. depth_chunk must be a multiple of R. */
  int32_t reserved_;
  const double* x_weights; /* NULL, or DEVICE float64[nx]: every lane of the point at x is multiplied by x_weights[x] inside
                              stage 1 and x is SUMMED there (x_kept = 0) -- for weights that depend on the innermost dim
                              only and no bins (GridAreaWeighting on latitude-fastest data); count lanes (mask / skipna)
                              take the weight too.  Always with plane_rows = R > 0 (R contiguous depth rows form one span,
                              ndepth % R == 0) and fp32 inputs.  wbx_det_partial (no flag, or WBX_FLAG_MASKED with a mask
                              stored like the data): R % 4 == 0, 16-B aligned spans streamed as one flat float4 array
                              (element e takes x_weights[e mod nx]), depth_chunk % 4 == 0, 1 <= nx <= 2045 (at nx < 4 a float4
                              spans several whole rows; no lower bound).  wbx_ens_partial
                              (any of FAIR / MASKED / SKIPNA, not SKIPNA_ENS): one point per lane walks the flat index,
                              any R, nx <= 2048. */
} wbx_s1_plan;

/* number of fp64 values stage 1 writes: nkey * nchunk * nlanes_total * nj, layout partial[key][chunk][lane][j].
 * Count lanes follow the value lanes: none without flags; ONE shared count lane with MASKED alone (validity is the
 * same for every statistic: nlanes_total = lanes + 1); one per value lane with SKIPNA (nlanes_total = 2 * lanes). */
int wbx_s1_partial_len(const wbx_s1_plan* plan, int lanes, int64_t* n_out);

/* ---- context ------------------------------------------------------------- */
int wbx_abi_version(void);
const char* wbx_last_error(void);
int wbx_device_count(int* n_out);
/* `hip_stream` may be NULL (library creates its own) or an existing hipStream_t
 * (e.g. torch.cuda.current_stream().cuda_stream) so launches order with the caller's work. */
int wbx_ctx_create(int device_id, void* hip_stream, wbx_ctx** out);
int wbx_ctx_destroy(wbx_ctx* ctx);
int wbx_ctx_synchronize(wbx_ctx* ctx);
int wbx_ctx_device_name(wbx_ctx* ctx, char* buf, size_t buflen);

/* device memory helpers for hosts without their own allocator */
int wbx_malloc(wbx_ctx* ctx, size_t bytes, void** dptr_out);
int wbx_free(wbx_ctx* ctx, void* dptr);
int wbx_memcpy_h2d(wbx_ctx* ctx, void* dptr, const void* h_src, size_t bytes);
int wbx_memcpy_d2h(wbx_ctx* ctx, void* h_dst, const void* dptr, size_t bytes); /* synchronises */
int wbx_memset(wbx_ctx* ctx, void* dptr, int value, size_t bytes);

/* Deferred results.  The reference's chunk loop (beam_pipeline.py:161-250 per chunk, CombinePerKey at :509) only
 * needs a chunk's sums when it combines them; reading them back synchronously after every chunk leaves the GPU idle
 * while the host prepares the next one.  With these the host enqueues the read-back of chunk k into pinned memory,
 * records a fence, launches chunk k+1 and waits on the fence of chunk k only when it combines it.
 *   wbx_host_alloc / wbx_host_free   page-locked host memory (hipHostMalloc)
 *   wbx_memcpy_d2h_async             enqueued on the context stream; `h_pinned` must come from wbx_host_alloc
 *   wbx_fence_*                      hipEvent (no timing) recorded on the context stream; wait blocks the host only */
typedef struct wbx_fence wbx_fence;
int wbx_host_alloc(wbx_ctx* ctx, size_t bytes, void** h_out);
int wbx_host_free(wbx_ctx* ctx, void* h_ptr);
int wbx_memcpy_d2h_async(wbx_ctx* ctx, void* h_pinned, const void* dptr, size_t bytes);
int wbx_fence_create(wbx_ctx* ctx, wbx_fence** out);
int wbx_fence_record(wbx_ctx* ctx, wbx_fence* fence);
int wbx_fence_wait(wbx_fence* fence);
int wbx_fence_destroy(wbx_fence* fence);
/* Work enqueued on `ctx` after this call starts only when `fence` (recorded on ANY context of the same process) has been
 * reached: hipStreamWaitEvent.  Orders a context's kernels behind another context's copies without blocking the host
 * (the chunk feeder's upload stream in front of the launch stream, beam_pipeline.py:69-116 -> :161-250). */
int wbx_ctx_wait_fence(wbx_ctx* ctx, wbx_fence* fence);
/* Asynchronous upload from page-locked memory (wbx_host_alloc) on the context stream: the staging half of the chunk
 * feeder's double buffer.  The source must stay untouched until a fence recorded afterwards has been reached. */
int wbx_memcpy_h2d_async(wbx_ctx* ctx, void* dptr, const void* h_pinned, size_t bytes);
int wbx_memcpy_d2d(wbx_ctx* ctx, void* dst, const void* src, size_t bytes); /* enqueued on the context stream */
/* Host side of the chunk feeder (ABI 13): dst[b][c][r] = src[b][r][c] for `batch` planes of rows x cols elements of 4 or 8
 * bytes, blocked (32 x 32 tiles, AVX2 8 x 8 blocks when the CPU has them).  The loaders hand on whatever dim order the store
 * has (weatherbenchX/data_loaders/xarray_loaders.py:185-188, 236-239: real archives are [.., longitude, latitude]); a file-backed
 * loader copies every chunk into page-locked memory anyway, and with `device_layout='lon_fastest'` that copy is this
 * transposition, so the DMA and the kernels see longitude-fastest fields (zonal transforms: 0.60 of the HBM peak instead of 0.38)
 * and no transposed copy is made on the device.  No context, no stream: plain host memory on both sides, which must not
 * overlap; thread-safe (callers split a chunk's planes over threads). */
int wbx_host_transpose(void* dst, const void* src, int64_t batch, int64_t rows, int64_t cols, int32_t elem_bytes);
/* The shader clock this device sustains with `blocks` x 256 threads of dependent fp32 FMAs running (ABI 13): s_memtime ticks
 * over s_memrealtime's constant 100 MHz, in MHz.  A measurement aid (boxes of one pool differ by 4-8 % on the same kernel):
 * bench.py prints it beside its numbers.  Synchronous; a few milliseconds. */
int wbx_clock_probe(wbx_ctx* ctx, int32_t blocks, double* shader_mhz_out);

/* ---- accumulators ------------------------------------------------------------------------------------------
 * The reference combines per-chunk AggregationStates on the host (beam.CombinePerKey(CombiningSum()),
 * beam_pipeline.py:509-510, beam_utils.py:30-50; AggregationState.sum, aggregation.py:84-110).  Here the stage-2 /
 * binned / spectrum outputs of a chunk stay in HBM and are added into a persistent float64 accumulator right behind
 * the kernel that produced them:
 *     acc[i] = (overwrite ? 0 : acc[i]) + src[i],  i < n          (stream ordered, deterministic, no atomics)
 * A rank's accumulators live in ONE device buffer that is all-reduced in place over RCCL and read back once per job. */
int wbx_acc_add(wbx_ctx* ctx, double* acc, const double* src, int64_t n, int32_t overwrite);

/* ---- accumulators across ranks (one process per GPU) ----------------------------------------------------------
 * The combine stage of the reference -- beam.CombinePerKey(CombiningSum()) over every (statistic, variable, offsets)
 * key of the job, beam_pipeline.py:509-519, beam_utils.py:30-50 -- as ONE collective on device memory:
 *     wbx_acc_allreduce:  acc[i] <- sum over ranks of acc[i], i < n      (ncclAllReduce(sum, double) in place, RCCL / xGMI,
 *                         enqueued on the context's stream: ordered behind the kernels and wbx_acc_add calls before it)
 *     wbx_acc_read:       the buffer on the host (waits for the stream)
 *     wbx_acc_reset:      acc[i] <- 0 (stream ordered)
 * Every rank lays its accumulators out identically (the caller's contract: same statistics and aggregators on every rank,
 * chunks of (init_time x lead_time) dealt round-robin); a slot only one rank wrote is zero on the others, so the
 * same sum also assembles results that keep init_time / lead_time (the reference's ConcatPerStatisticPerVariable,
 * beam_pipeline.py:253-319).
 * A communicator joins `nranks` processes: rank 0 calls wbx_comm_unique_id, hands the WBX_COMM_ID_BYTES bytes to the other
 * ranks by any means (a file, MPI, a torch.distributed store ...), and every rank calls wbx_comm_create on its own context.
 * RCCL is loaded on first use (librccl.so.1; WBX_RCCL_PATH overrides); without it these calls return WBX_ERR_RCCL. */
#define WBX_COMM_ID_BYTES 128
typedef struct wbx_comm wbx_comm; /* opaque: one RCCL communicator (rank, size, device) */
int wbx_comm_unique_id(void* id_out /* WBX_COMM_ID_BYTES */);
int wbx_comm_create(wbx_ctx* ctx, const void* unique_id, int32_t nranks, int32_t rank, wbx_comm** out);
int wbx_comm_destroy(wbx_comm* comm);
int wbx_comm_info(const wbx_comm* comm, int32_t* nranks_out, int32_t* rank_out, int64_t* collectives_out);
int wbx_acc_allreduce(wbx_ctx* ctx, wbx_comm* comm, double* acc, int64_t n);
int wbx_acc_read(wbx_ctx* ctx, const double* acc, int64_t n, double* host_out);
int wbx_acc_reset(wbx_ctx* ctx, double* acc, int64_t n);

/* valid_out[i] = !isnan(data[i]) (one byte per element, 1 = valid) over n contiguous elements: the `mask` coordinate
 * of data_loaders/base.py:25-56 (add_nan_mask_to_data) for payloads that are already in HBM -- the mask is built and
 * consumed (WBX_FLAG_MASKED, input 3) without ever visiting the host.  valid_out must be 4-byte aligned. */
int wbx_notnan_mask(wbx_ctx* ctx, const void* data, int dtype, int64_t n, uint8_t* valid_out);

/* HIP-event timer on the context stream (bench.py's roofline leg). */
int wbx_timer_start(wbx_ctx* ctx);
int wbx_timer_stop(wbx_ctx* ctx, float* ms_out); /* synchronises on the stop event */
/* Timing marks that do NOT synchronise: wbx_mark records a timing event on the context stream and returns its index;
 * wbx_mark_elapsed waits for mark i1 and returns the time between two marks of this context; wbx_marks_reset recycles
 * the events.  bench.py brackets every launch of its timed region with a pair of marks and reads them after the
 * region's closing synchronisation, so the durations it reports are those of the timed launches themselves. */
int wbx_mark(wbx_ctx* ctx, int* index_out);
int wbx_mark_elapsed(wbx_ctx* ctx, int i0, int i1, float* ms_out);
int wbx_marks_reset(wbx_ctx* ctx);

/* ---- stage 1: deterministic ----------------------------------------------
 * Replaces Statistic.compute + the stat-side einsum of Aggregator.aggregate_stat_var
 * (metrics/base.py:184-197, deterministic.py:91-123,222-259, aggregation.py:337-366). */
int wbx_det_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int func /*wbx_det_func*/,
                    int dtype /*wbx_dtype*/, const void* p, const void* t, const void* c,
                    const uint8_t* mask, double* partial_out);

/* ---- stage 1: ensemble ---------------------------------------------------
 * p has an extra member axis of length M and element stride `member_stride`
 * that is NOT part of key/depth/x.  Replaces probabilistic.py:116-336. */
int wbx_ens_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M,
                    int64_t member_stride, int algo /*wbx_ens_algo*/, const void* p,
                    const void* t, const uint8_t* mask, double* partial_out);

/* Ensemble-valued predictions AND targets (CRPSEnsembleDistance-style evaluations) with per-point member counts on both sides:
 * skipna_ensemble=True of probabilistic.py:133-145 (CRPSSkill over the non-NaN (prediction member, target member) pairs) and
 * :304-336 (UnbiasedEnsembleMeanSquaredError with both ensembles' own counts).  t has a member axis of length N and element
 * stride `target_member_stride`, like p's M / `member_stride`.  Lanes (partial layout, count lanes and flags as wbx_ens_partial):
 *   0  sum over valid pairs |p_i - t_j| / (n_p n_t)                    NaN without a valid pair
 *   1  (mean p - mean t)^2 - var(p) / n_p - var(t) / n_t  (ddof = 1)   NaN with fewer than two valid members on a side
 * WBX_FLAG_SKIPNA_ENS: NaN members are missing members; without it a NaN member makes both lanes NaN.  From-memory fp64
 * arithmetic for any M, N (O(M N) per point): a correctness path for a rare configuration, no roofline claim. */
#define WBX_ENS2_LANES 2
int wbx_ens2_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int N,
                     int64_t target_member_stride, const void* p, const void* t, const uint8_t* mask, double* partial_out);

/* ---- stage 2: weighted / binned contraction --------------------------------
 * partial is viewed as [nA][nBk][nBr][nchunk][nlane][nj];  W as [nBk][nBr][nj][nbin].
 *   sum_j = 1: out[nA][nBk][nlane][nbin]      = sum_{Br,chunk,j} partial * W
 *   sum_j = 0: out[nA][nBk][nlane][nj][nbin]  = sum_{Br,chunk}   partial * W
 * Plain multiply-add with no zero skipping, so NaN * 0 = NaN poisons a bin exactly
 * as the reference's xr.dot does (aggregation.py:272-277,335). */
typedef struct wbx_s2_plan {
  int64_t nA, nBk, nBr, nchunk, nlane, nj, nbin;
  int32_t sum_j;
} wbx_s2_plan;
int wbx_contract(wbx_ctx* ctx, const wbx_s2_plan* plan, const double* partial,
                 const double* W, double* out);

/* Same contraction for W = wt[Bk][Br][j] * mask[Bk][Br][j][bin] with BOOLEAN masks and nbin <= 64 (Regions / LandSea
 * binning, binning.py:92-201, times GridAreaWeighting): `wt` is float64[nBk][nBr][nj]; bit b of bits[nBk][nBr][nj]
 * says whether the point belongs to bin b.  Result layout and NaN semantics are identical to wbx_contract, with one exception: an
 * INFINITE partial makes its lane NaN in EVERY bin of the cell -- the kernel adds (partial * w) * 0 to every bin, which is NaN
 * for +-inf as it is for NaN -- where wbx_contract (and the reference's xr.dot) keep +-inf in the bins the point belongs to and
 * give NaN only in the others. */
int wbx_contract_bits(wbx_ctx* ctx, const wbx_s2_plan* plan, const double* partial, const double* wt,
                      const uint64_t* bits, double* out);

/* ---- stage 1: indicator ("categorical") statistics --------------------------------------------------------
 * Per point a 0/1 (or member-fraction) vector along a NEW dimension of `ncat` categories:
 *   WBX_CAT_EXCEED  ErrorExceedance (deterministic.py:262-295) and, with M > 1 members at `member_stride`,
 *                   EnsembleErrorExceedance (probabilistic.py:836-861): lane k = fraction of non-NaN members with
 *                   |p_m - t| > thresholds[k]; NaN when every member's error is NaN.  `thresholds` is a DEVICE
 *                   float64[ncat]; NaN thresholds compare false (the host patches those lanes to NaN).
 *   WBX_CAT_RANK    RankHistogram (probabilistic.py:1306-1343): lane r = [#{m : p_m < t} == r], ncat = M + 1.
 * partial_out[nkey][nchunk][lanes_total][nj] exactly like wbx_det_partial, lanes_total = ncat (+1 with
 * WBX_FLAG_MASKED, x2 with WBX_FLAG_SKIPNA), so wbx_contract / wbx_contract_bits consume it unchanged.
 * Per-thread fp64 counters live in LDS columns (the category index is data dependent): lanes_total <= 128. */
typedef enum wbx_cat_func { WBX_CAT_EXCEED = 0, WBX_CAT_RANK = 1 } wbx_cat_func;
int wbx_cat_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int func, int dtype, int ncat, int M,
                    int64_t member_stride, const void* p, const void* t, const double* thresholds,
                    const uint8_t* mask, double* partial_out);
/* WBX_CAT_EXCEED against thresholds that depend on the statistic's own dims (one set per level, per latitude ...:
 * deterministic.py:262-295 compares |p - t| with any DataArray that broadcasts).  `threshold_field` is a DEVICE float64 array
 * addressed as input 2 of the plan: threshold k of the point (key, depth, x) is
 *     threshold_field[key_off[2][key] + depth_off[2][depth] + x * xstride[2] + k * category_stride]
 * (zero strides along the dims it does not depend on).  NaN thresholds give NaN indicators, exactly as above. */
int wbx_cat_exceed_field(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int ncat, int M, int64_t member_stride,
                         const void* p, const void* t, const double* threshold_field, int64_t category_stride,
                         const uint8_t* mask, double* partial_out);

/* ---- stage 1: thresholded 2x2 contingency tables (joined ABI 13) -------------------------------------------
 * The four cells of the contingency table of a forecast and an observation at `nthr` thresholds, i.e. TruePositives /
 * FalsePositives / FalseNegatives / TrueNegatives (categorical.py:25-101) of inputs binarised by ContinuousToBinary
 * (wrappers.py:50-88), in one pass over p and t.  Per point and threshold k:
 *     P_k = (double)p > thresholds[k],  O_k = (double)t > thresholds[k]      (strict, on the threshold as given)
 *     TP = P_k & O_k,  FP = P_k & !O_k,  FN = !P_k & O_k,  TN = !P_k & !O_k  -- exactly one of them is 1
 * A comparison with a NaN threshold is false (the point counts as TN -- unlike WBX_CAT_EXCEED, where it is NaN);
 * -0.0 > 0.0 is false; +inf exceeds every finite threshold.  A point whose p or t is NaN is a NaN statistic in all
 * 4 * nthr lanes: without flags it poisons every value lane of its partial; under WBX_FLAG_MASKED alone it contributes
 * exactly 0 where the mask is 0 and poisons where it is not; under WBX_FLAG_SKIPNA it is counted out.
 * Lane order is part of the ABI: value lane cell * nthr + k, cell in (TP, FP, FN, TN).  Count lanes follow the library's
 * convention (none / one shared / one per value lane); under SKIPNA all 4 * nthr of them are equal (the number of valid,
 * non-NaN points).  partial_out[nkey][nchunk][lanes_total][nj] as for wbx_det_partial: wbx_s1_partial_len with
 * lanes = 4 * nthr, wbx_contract and wbx_contract_bits serve it unchanged.  Every output is an integer count < 2^32 held
 * in fp64 (or NaN): the result is a function of the inputs and the plan only, bit for bit.
 * `thresholds` is a DEVICE float64[nthr].  float32 inputs are compared in float32 against the threshold rounded toward
 * -inf to float32, which decides exactly like the float64 comparison for every float32 value (+-inf and thresholds
 * beyond the float32 range included; rounding to nearest would not: float(0.1) > 0.1).
 * plan: flags within MASKED | SKIPNA, plane_rows = 0, no x_weights; vec = 4 is honoured where x is summed (x kept: one x
 * per lane); depth_chunk * nx < 2^32 (the counters are uint32).  nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero
 * the partial. */
#define WBX_CONT_CELLS 4           /* TP, FP, FN, TN */
#define WBX_CONT_MAX_THRESHOLDS 16 /* per launch */
int wbx_contingency_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int nthr,
                            const void* p, const void* t, const double* thresholds /* DEVICE float64[nthr] */,
                            const uint8_t* mask, double* partial_out);

/* ---- stage 1: ranked probability score of an ensemble at a list of thresholds (joined ABI 13) ----------------
 * EnsembleRankedProbabilityScore (probabilistic.py:339-477) of an ensemble of predictions against a scalar target, in one pass
 * over p and t: no [nthr][M][frame] indicator arrays of the two ContinuousToCDF transforms (wrappers.py) are formed.  p has a
 * member axis of length M and element stride `member_stride` that is not part of key / depth / x, as for wbx_ens_partial.
 * Per point, with members x_m, target y, prediction thresholds a_k = p_thresholds[k], target thresholds b_k = t_thresholds[k]:
 *     c_k = #{m : (double)x_m <= a_k},  o_k = [(double)y <= b_k]       (`<` instead of `<=` when right_inclusive == 0)
 *     WBX_FLAG_FAIR:  n_k = (M - 1) (c_k - o_k M)^2 - c_k (M - c_k),  D = M^2 (M - 1)   [(mean - o)^2 - var(ddof = 1) / M]
 *     otherwise:      n_k = (c_k - o_k M)^2,                          D = M^2           [(mean - o)^2]
 *     value = (sum_k n_k) / D
 * Everything is a function of the integers c_k: the kernel sorts nothing and adds no floating-point numbers.  A partial is the
 * signed 64-bit sum S of sum_k n_k over its points, written once as (double)S / (double)D -- the correctly rounded quotient of
 * two integers, a function of the inputs and the plan only, bit for bit, whatever the order of summation.
 * ONE value lane.  Count lanes follow the library's convention (none / one shared / one per value lane).  A point with a NaN
 * member or a NaN target is a NaN statistic (sum(bin_dim, skipna=False) of NaN terms): without flags it poisons its partial;
 * under WBX_FLAG_MASKED alone it contributes exactly 0 where the mask is 0 and poisons where it is not; under WBX_FLAG_SKIPNA it
 * is counted out.  -0.0 <= 0.0 is true; +-inf members and targets compare as IEEE says.
 * partial_out[nkey][nchunk][lanes_total][nj] as for wbx_det_partial: wbx_s1_partial_len with lanes = 1, wbx_contract and
 * wbx_contract_bits serve it unchanged.
 * `p_thresholds` / `t_thresholds` are DEVICE float64[nthr] each; they need not be sorted or distinct, +-inf is allowed.  NaN
 * thresholds are the caller's business: a comparison with one is false here, while the reference makes the point NaN.
 * float32 inputs are compared in float32 against the threshold rounded to float32 toward -inf for `<=` and toward +inf for
 * `<`, which decides exactly like the float64 comparison for every float32 value (+-inf and thresholds beyond the float32
 * range included; rounding to nearest would not: float(0.1) <= 0.1 is false).
 * Refused (WBX_ERR_INVALID, output untouched): nthr outside 1..WBX_ERPS_MAX_THRESHOLDS, M outside 1..WBX_ERPS_MAX_MEMBERS,
 * WBX_FLAG_FAIR with M < 2, an unknown dtype, flags beyond MASKED | SKIPNA | FAIR, WBX_FLAG_MASKED with a NULL mask,
 * plane_rows != 0 or x_weights, and depth_chunk * nx * nthr * (M - 1) * M^2 >= 2^53 (S must stay exact in fp64).  vec = 4 is
 * accepted and read with dword loads (a lane owns a point and walks its members: the wave's load of one member row is
 * coalesced as it is).  nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero the partial. */
#define WBX_ERPS_MAX_THRESHOLDS 16 /* per launch */
#define WBX_ERPS_MAX_MEMBERS 256   /* sum_k n_k of a point fits an int32 */
int wbx_ens_rps_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M, int64_t member_stride,
                        int nthr, const double* p_thresholds, const double* t_thresholds /* DEVICE float64[nthr] each */,
                        int right_inclusive, const void* p, const void* t, const uint8_t* mask, double* partial_out);

/* ---- stage 1: ranked probability score of an ensemble at threshold FIELDS (joined ABI 13) -----------------------
 * wbx_ens_rps_partial with the thresholds read at the point: EnsembleRankedProbabilityScore with `prediction_bin_thresholds` /
 * `target_bin_thresholds` Datasets such as climatological terciles [bin, dayofyear, latitude, longitude], without the selected copy of
 * the thresholds (select_bin_thresholds_by_time_from_chunk) and the indicator arrays.  `c` is input 2 of the plan (key_off[2],
 * depth_off[2], xstride[2], the gather tables; zero strides where it does not vary), exactly as for wbx_ens_interval_partial.  With A
 * the address of a point in c, in elements of `thr_dtype`:
 *     a_k = c[A + k * thr_stride],   b_k = c[A + k * thr_stride + t_off],   k in 0..nthr-1
 * t_off == 0: both sides read the same thresholds, which are loaded once.  c_k, o_k, n_k, D, the value, the partial (S / D of two
 * integers, no atomics), the lanes and the layout of partial_out are those of wbx_ens_rps_partial.
 * A point is a NaN point if a member, the target, or any of its nthr prediction or target thresholds is NaN
 * (cdf.where(~isnan(da)).where(~isnan(thresholds)) followed by sum(bin_dim, skipna=False)); NaN points poison, are masked out or are
 * counted out as for wbx_ens_rps_partial.  Only the nthr thresholds of a side are read.
 * Comparisons decide as NumPy's promoted comparison does: equal types compare as they are; float32 thresholds against float64 data
 * widen exactly; float64 thresholds against float32 data are rounded per point to float32 toward -inf for `<=` and toward +inf for
 * `<` (NaN stays NaN, a value beyond the float32 range decides right) and compared in float32.
 * Refused (WBX_ERR_INVALID, output untouched): everything wbx_ens_rps_partial refuses (limits WBX_ERPS_MAX_*), an unknown thr_dtype,
 * thr_stride == 0 with nthr > 1, and a NULL c unless the extent is empty (as for p and t: nothing would be read).  vec = 4 is
 * accepted and read with dword loads; no plane mode, no x weights.
 * nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero the partial, whatever c is. */
int wbx_ens_rps_field_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* p, t: WBX_F32 | WBX_F64 */,
                              int thr_dtype /* c: WBX_F32 | WBX_F64 */, int M, int64_t member_stride, int nthr, int64_t thr_stride,
                              int64_t t_off, int right_inclusive, const void* p, const void* t, const void* c, const uint8_t* mask,
                              double* partial_out);

/* ---- stage 1: thresholded 2x2 contingency tables at threshold FIELDS (joined ABI 13) ---------------------------
 * wbx_contingency_partial with the thresholds read at the point: TruePositives .. TrueNegatives behind
 * ContinuousToBinary('both', field, dim) whose thresholds are a DataArray / Dataset (wrappers.py:50-88), such as "exceeds the
 * local climatological 95th percentile", without the [nthr][frame] indicator arrays.  `c` is input 2 of the plan (key_off[2],
 * depth_off[2], xstride[2], the gather tables; zero strides where it does not vary), exactly as for wbx_ens_rps_field_partial
 * and wbx_cat_exceed_field.  With A the address of a point in c, in elements of `thr_dtype`:
 *     thr_k = c[A + (thr_first + k) * thr_stride],   k in 0..nthr-1         (thr_first: the first threshold of this launch, so
 *                                                                            that blocks of a longer threshold axis share one c)
 *     P_k = p > thr_k,  O_k = t > thr_k    (strict; both sides read the same threshold, which is loaded once)
 * The cells, the lanes (value lane cell * nthr + k), the count lanes, NaN p or t (poisons / masked out / counted out), the
 * partial (integers < 2^32 in fp64 or NaN, a function of the inputs and the plan only, no atomics) and the layout of
 * partial_out are those of wbx_contingency_partial, word for word.
 * A comparison with a NaN threshold is false: the point counts towards TN when p and t are not NaN, which is
 * (x > NaN).where(~isnan(x)).  This is UNLIKE wbx_ens_rps_field_partial, where a NaN threshold makes the point a NaN point.
 * Comparisons decide as NumPy's promoted comparison does: equal types compare as they are; float32 thresholds against float64
 * data widen exactly; float64 thresholds against float32 data are rounded per point to float32 toward -inf (x > v <=> x > rd(v)
 * for every non-NaN float32 x; NaN stays NaN, a value beyond the float32 range decides right) and compared in float32.
 * Refused (WBX_ERR_INVALID, output untouched): everything wbx_contingency_partial refuses (nthr outside
 * 1..WBX_CONT_MAX_THRESHOLDS, an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask, plane_rows != 0
 * or x_weights, depth_chunk * nx >= 2^32), an unknown thr_dtype, thr_stride == 0 with nthr > 1, thr_first < 0, and a NULL c
 * unless the extent is empty.  vec = 4 is honoured where x is summed: p, t and -- where xstride[2] == 1 -- the field's row are
 * read with 16-byte loads of element alignment, so thr_stride needs no alignment of its own.
 * nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero the partial, whatever c is.
 * The entry is not among the wbx_fn a chunk record may hold (wbx_chunk_replay): a chunk that launches it is evaluated call by call. */
int wbx_contingency_field_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* p, t: WBX_F32 | WBX_F64 */,
                                  int thr_dtype /* c: WBX_F32 | WBX_F64 */, int nthr, int64_t thr_stride, int64_t thr_first,
                                  const void* p, const void* t, const void* c, const uint8_t* mask, double* partial_out);

/* ---- stage 1: energy score of an ensemble, both terms (joined ABI 13) -------------------------------------------
 * EnergyScoreSkill and EnergyScoreSpread (probabilistic.py:480-551) of an ensemble of predictions against a target, in one pass
 * over p and t instead of one whole-array pass per cyclic member offset.  p has a member axis of length M and element stride
 * `member_stride`, and p and t have a norm run of L elements with element strides `p_norm_stride` / `t_norm_stride` (the norm dims
 * of the score, collapsed to one run); neither is part of key / depth / x.  Per point, with members x_m in R^L and target y in R^L:
 *     lane 0 (skill)  = (sum_m ||x_m - y||) / M
 *     lane 1 (spread) = (sum_{m != m'} ||x_m - x_m'||) / D,   D = M (M - 1) under WBX_FLAG_FAIR, M^2 otherwise
 * Differences, their squares and the sum of squares are formed in the input type (fma, in the order of the run), the square root
 * is correctly rounded in the input type, everything after that is float64.  The squared distance is never formed from
 * ||a||^2 + ||b||^2 - 2 a.b.  NaN and inf are what IEEE arithmetic makes of them: a NaN member makes both lanes NaN, a NaN target
 * lane 0 only; an infinite member against finite ones gives +inf; two infinite members of one sign make lane 1 NaN (inf - inf)
 * and leave lane 0 +inf; a member is never paired with itself.
 * TWO value lanes (WBX_ENRG_LANES).  Count lanes follow the library's convention (none / one shared / one per value lane), and
 * NaN-ness is per lane: without flags a NaN lane of a point poisons that lane of its partial; under WBX_FLAG_MASKED alone a point
 * contributes exactly 0 where the mask is 0 and poisons (per lane) where it is not; under WBX_FLAG_SKIPNA a NaN lane of a point is
 * counted out of that lane.  partial_out[nkey][nchunk][lanes_total][nj] as for wbx_det_partial: wbx_s1_partial_len with lanes = 2,
 * wbx_contract and wbx_contract_bits serve it unchanged.  The result is a function of the inputs and the plan only, bit for bit:
 * every sum is formed in a fixed order, nothing is added atomically.
 * Refused (WBX_ERR_INVALID, output untouched): M outside 2..WBX_ENRG_MAX_MEMBERS, L < 1, an unknown dtype, flags beyond
 * MASKED | SKIPNA | FAIR, WBX_FLAG_MASKED with a NULL mask, plane_rows != 0 or x_weights.  vec = 4 is accepted and ignored.
 * nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero the partial. */
#define WBX_ENRG_LANES 2
#define WBX_ENRG_MAX_MEMBERS 64 /* M + 1 vectors padded to 4: 17 x 17 blocks of 4 x 4 pairs, 153 of them per point */
int wbx_ens_energy_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M, int64_t member_stride,
                           int64_t L, int64_t p_norm_stride, int64_t t_norm_stride, const void* p, const void* t,
                           const uint8_t* mask, double* partial_out);

/* ---- stage 1: variogram score of an ensemble (joined ABI 13) -----------------------------------------------------
 * VariogramScore (probabilistic.py:554-600) of an ensemble of predictions against a target, in one pass over p and t instead of one
 * whole-array pass per cyclic offset along the score's dim.  p has a member axis of length M and element stride `member_stride`,
 * and p and t have a run of L elements with element strides `p_run_stride` / `t_run_stride` (the score's dim; a negative stride
 * walks down from the first element the plan's offsets name); neither is part of key / depth / x.  Per point, with members x_m in
 * R^L and target y in R^L:
 *     VS = sum_{i, j in [0, L)} ( |y_i - y_j|^p - (1 / M) sum_m |x_i^m - x_j^m|^p )^2
 * over ordered pairs, the diagonal included, which is 0 for finite values and NaN otherwise: a point with ANY NaN or infinite value
 * among its (M + 1) L inputs is NaN (the kernel decides that with a flag per point, not by propagation), every other point is
 * twice the sum over i < j.  L = 1 gives 0 (or NaN).  `power` is a code for p, there is no general pow: WBX_VGRAM_POW_HALF (0.5),
 * WBX_VGRAM_POW_ONE (1), WBX_VGRAM_POW_TWO (2).
 * Differences are formed in the input type; |d|^p in the input type: a correctly rounded square root of |d|, |d| itself, or one
 * rounded product.  Everything from the member sum onwards is float64: the M terms in member order, the division by M, the
 * difference with the target's term, the square, the pair sum in a fixed order.  No moment identity is used.
 * ONE value lane (WBX_VGRAM_LANES).  Count lanes follow the library's convention (none / one under a mask / one under skipna): without
 * flags a NaN point poisons its partial; under WBX_FLAG_MASKED alone a point contributes exactly 0 where the mask is 0 and poisons
 * where it is not; under WBX_FLAG_SKIPNA a NaN point is counted out.  partial_out[nkey][nchunk][lanes_total][nj] as for
 * wbx_det_partial: wbx_s1_partial_len with lanes = 1, wbx_contract and wbx_contract_bits serve it unchanged.  The result is a
 * function of the inputs and the plan only, bit for bit: every sum is formed in a fixed order, nothing is added atomically.
 * Refused (WBX_ERR_INVALID, output untouched): M outside 1..WBX_VGRAM_MAX_MEMBERS, L outside 1..WBX_VGRAM_MAX_RUN, an unknown power
 * code or dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask, plane_rows != 0 or x_weights.  vec = 4 is accepted
 * and ignored; block_threads sets the x a block covers when x is kept, an x-summed launch always runs 256 threads.  nkey == 0
 * touches nothing; ndepth == 0 or nx == 0 zero the partial. */
#define WBX_VGRAM_LANES 1
#define WBX_VGRAM_MAX_MEMBERS 64
#define WBX_VGRAM_MAX_RUN 64 /* the run is resident whole: 2016 pairs per point */
#define WBX_VGRAM_POW_HALF 0
#define WBX_VGRAM_POW_ONE 1
#define WBX_VGRAM_POW_TWO 2
int wbx_ens_variogram_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M, int64_t member_stride,
                              int64_t L, int64_t p_run_stride, int64_t t_run_stride, int power /* WBX_VGRAM_POW_* */, const void* p,
                              const void* t, const uint8_t* mask, double* partial_out);

/* ---- stage 1: Wasserstein-1 distance between two ensembles (joined ABI 13) ------------------------------------------
 * WassersteinDistance (probabilistic.py) of an ensemble of predictions against an ensemble of targets, in one pass over p and t
 * instead of a pooled float64 sort and two cumulative sums.  p has a member axis of length M and element stride `member_stride`, t
 * one of length N and element stride `target_member_stride`; neither is part of key / depth / x, and the two sizes are independent.
 * Per point, with the sorted members p_(0) <= ... <= p_(M-1) and t_(0) <= ... <= t_(N-1):
 *     W1 = int_0^1 |Qp(u) - Qt(u)| du = ( sum over pieces of c |p_(i) - t_(j)| ) / (M N)
 * The pieces are the M + N - gcd(M, N) intervals between consecutive breakpoints of {i / M} u {j / N}.  A piece's length is an
 * integer in units of 1 / (M N): c = min((i + 1) N, (j + 1) M) - max(i N, j M); i advances when (i + 1) N <= (j + 1) M and j
 * when (j + 1) M <= (i + 1) N, from i = j = 0.  The sequence (i, j, c) depends on (M, N) only, not on the data.
 * Members are sorted in the input type (exact).  Differences, their absolute values, the products with the integer c and the sum are
 * float64 -- the difference rounded once, the product added to the sum by one fused multiply-add --, the sum in the order of the
 * walk; one division by (double)(M N) at the end.
 * Non-finite members are what the reference's pooled form makes of them, decided by a flag per point and not by propagation: a
 * NaN member on either side makes the point NaN; two or more +inf among the pooled M + N members make the point NaN, and so do two
 * or more -inf (the pooled form has an inf - inf gap); otherwise the arithmetic decides -- a single +inf or a single -inf, or one
 * of each, gives +inf.  (The walk alone would give +inf for p = [inf, inf], t = [0].)
 * ONE value lane (WBX_WASS_LANES).  Count lanes follow the library's convention (none / one under a mask / one under skipna): without
 * flags a NaN point poisons its partial; under WBX_FLAG_MASKED alone a point contributes exactly 0 where the mask is 0 and poisons
 * where it is not; under WBX_FLAG_SKIPNA a NaN point is counted out.  partial_out[nkey][nchunk][lanes_total][nj] as for
 * wbx_det_partial: wbx_s1_partial_len with lanes = 1, wbx_contract and wbx_contract_bits serve it unchanged.  The result is a
 * function of the inputs and the plan only, bit for bit: every sum is formed in a fixed order, nothing is added atomically.
 * Refused (WBX_ERR_INVALID, output untouched): M or N outside 1..WBX_WASS_MAX_MEMBERS, an unknown dtype, flags beyond
 * MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask, plane_rows != 0 or x_weights.  vec = 4 is accepted and ignored; a block runs
 * block_threads threads up to what its LDS holds (128 for float32, 64 for float64).  nkey == 0 touches nothing; ndepth == 0 or
 * nx == 0 zero the partial. */
#define WBX_WASS_LANES 1
#define WBX_WASS_MAX_MEMBERS 64 /* a side, the largest generated sorting network */
int wbx_ens_wasserstein_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M, int64_t member_stride,
                                int N, int64_t target_member_stride, const void* p, const void* t, const uint8_t* mask,
                                double* partial_out);

/* ---- stage 1: interval statistics of an ensemble (joined ABI 13) ----------------------------------------------------
 * Covered, Confident and JaccardDistant (categorical.py:701-863, the factors of Opportunism) of an ensemble of predictions against
 * a target and a climatology of two quantile fields, in one pass that sorts a point's members once, instead of two host quantile
 * fields per statistic, an aligned copy of the climatology and one Boolean array per statistic.  p has a member axis of length M and
 * element stride `member_stride`, which is not part of key / depth / x.  `c` is input 2 of the plan (key_off[2], depth_off[2],
 * xstride[2], the gather tables; zero strides where it does not vary), and each bound's `c_off` is added to that address: the element
 * offset of the bound's quantile label along the climatology's quantile dim.
 * `lanes` is a set of WBX_IVL_* bits; the value lanes are the requested statistics in the order Covered, Confident, JaccardDistant.
 * `params` is a HOST array of three wbx_ivl_lane in that order, read during the call (entries of lanes not asked for are ignored).
 * Per point:
 *   Members are sorted in the input type (exact).  Everything after the sort is float64, every product, sum and quotient rounded on
 *   its own (no fused multiply-add).  A quantile bound (k, g) -- the host forms h = q (M - 1), k = floor(h), g = h - k in float64 --
 *   is NumPy's `linear` method in NumPy's order of operations: with A = x_(k), B = x_(min(k + 1, M - 1)), d = B - A it is
 *       A + d g         where g < 0.5,
 *       B - d (1 - g)   otherwise,
 *   with no shortcut for g == 0 (inf * 0 gives the NaN NumPy gives).  A NaN member makes every ensemble quantile of the point NaN,
 *   by a flag gathered while the members are loaded and not by propagation; from there the formulas decide:
 *     Covered        = lo <= t && t <= hi
 *     Confident      = (hi - lo) < threshold * (c_hi - c_lo)
 *     JaccardDistant = (1 - index) > threshold, with
 *         overlap = max(min(a_hi, c_hi) - max(a_lo, c_lo), 0)   (min / max hand a NaN on, and so does the clip)
 *         union   = (a_hi - a_lo) + (c_hi - c_lo) - overlap
 *         index   = union > 0 ? overlap / union : 1             (false for a NaN union)
 *   An indicator is 0 or 1, never NaN.
 * Inputs that no requested lane needs are not read: t without Covered, c with Covered alone (c may then be NULL).
 * Count lanes follow the library's convention (none / one under a mask / one per value lane under skipna); no value is NaN, so
 * under WBX_FLAG_SKIPNA every unmasked point is counted, and under WBX_FLAG_MASKED a point contributes exactly 0 where the mask is 0.
 * partial_out[nkey][nchunk][lanes_total][nj] as for wbx_det_partial: wbx_s1_partial_len with lanes = the number of bits set,
 * wbx_contract and wbx_contract_bits serve it unchanged.  Every partial is an integer in float64 and a function of the inputs and
 * the plan only: every sum is formed in a fixed order, nothing is added atomically.
 * Refused (WBX_ERR_INVALID, output untouched): M outside 1..WBX_IVL_MAX_MEMBERS, `lanes` zero or beyond the three bits, a requested
 * bound with k outside 0..M-1 or g outside [0, 1), an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask, a
 * requested lane whose input (t for Covered, c for the other two) is NULL, plane_rows != 0 or x_weights.  vec = 4 is accepted and
 * ignored; a block runs block_threads threads up to what its LDS holds (128 for float32, 64 for float64).  nkey == 0 touches
 * nothing; ndepth == 0 or nx == 0 zero the partial. */
#define WBX_IVL_COVERED 1
#define WBX_IVL_CONFIDENT 2
#define WBX_IVL_JACCARD 4
#define WBX_IVL_MAX_MEMBERS 64 /* the largest generated sorting network */
typedef struct wbx_ivl_bound {
  int32_t k;     /* rank of the lower neighbour, 0..M-1 */
  double g;      /* weight of the upper neighbour, [0, 1) */
  int64_t c_off; /* element offset of the bound's quantile label in the climatology */
} wbx_ivl_bound;
typedef struct wbx_ivl_lane {
  wbx_ivl_bound lo, hi;
  double threshold; /* Confident: confidence_threshold; JaccardDistant: threshold; Covered: unused */
} wbx_ivl_lane;
int wbx_ens_interval_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M, int64_t member_stride,
                             int lanes /* WBX_IVL_* bit set */, const wbx_ivl_lane* params /* HOST, three entries */, const void* p,
                             const void* t, const void* c, const uint8_t* mask, double* partial_out);

/* ---- stage 1: contingency tables of ensemble event probabilities (joined ABI 13) -----------------------------------
 * The four cells TruePositives / FalsePositives / FalseNegatives / TrueNegatives (categorical.py:25-101) behind the documented chain
 * ContinuousToBinary('both', event thresholds) -> EnsembleMean('predictions') -> ContinuousToBinary('predictions', probability
 * thresholds) or ContinuousToBins('predictions', probability edges) (wrappers.py; RelativeEconomicValue and Reliability end in it),
 * in one pass over p and t: no [nthr][M][frame] indicator array, no [nthr][nslot][frame] arrays are formed.  p has a member axis of
 * length M and element stride `member_stride` that is not part of key / depth / x, as for wbx_ens_partial.
 * Counts and observation.  Per point, with members x_m, target y and event thresholds a_k = thresholds[k]:
 *     c_k = #{m : (double)x_m > a_k} in 0..M,   o_k = [(double)y > a_k]        (strict, on the threshold as given)
 * A comparison with a NaN event threshold is false; -0.0 > 0.0 is false; +-inf compare as IEEE says.  float32 inputs are compared
 * in float32 against the threshold rounded toward -inf to float32, which decides exactly like the float64 comparison for every
 * float32 value (+-inf and thresholds beyond the float32 range included; rounding to nearest would not: float(0.1) > 0.1).
 * Prediction per slot.  The member mean of the 0 / 1 indicators is a function of c_k alone, and so is whether it falls into
 * probability slot j; the caller hands every slot over as a run of counts: P_kj = (lo_j <= c_k && c_k <= hi_j), `slots` a DEVICE
 * int32[2 * nslot] of (lo, hi) pairs, lo > hi an empty slot.  The kernel never sees a probability.
 *     TP = P_kj & o_k,  FP = P_kj & !o_k,  FN = !P_kj & o_k,  TN = !P_kj & !o_k  -- exactly one of them is 1
 * Lane order is part of the ABI: 4 * nthr * nslot value lanes, cell * (nthr * nslot) + k * nslot + j, cell in (TP, FP, FN, TN).
 * Count lanes follow the library's convention (none / one shared / one per value lane); under SKIPNA all of them are equal (the
 * number of valid, non-NaN points).  partial_out[nkey][nchunk][lanes_total][nj] as for wbx_det_partial: wbx_s1_partial_len with
 * lanes = 4 * nthr * nslot; wbx_contract, wbx_contract_bits, the accumulators and the chunk records take it unchanged.
 * Per partial the integer counts #(P & O) and #P per (k, j), #O per k and the numbers of good (valid, non-NaN) and of valid points
 * are held, and the cells are formed once: FP = #P - TP, FN = #O - TP, TN = N - #P - #O + TP.  No floating-point number is added and
 * nothing is added atomically: every output is an integer < 2^32 held in fp64 (or NaN), a function of the inputs and the plan only.
 * A point with a NaN member or a NaN target is a NaN statistic in all lanes: without flags it poisons every value lane of its
 * partial; under WBX_FLAG_MASKED alone it contributes exactly 0 where the mask is 0 and poisons where it is not; under
 * WBX_FLAG_SKIPNA it is counted out -- exactly as in wbx_contingency_partial.
 * Refused (WBX_ERR_INVALID, output untouched): nthr < 1, nslot < 1 or nthr * nslot > WBX_EPC_MAX_PAIRS, M outside
 * 1..WBX_EPC_MAX_MEMBERS, an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask, plane_rows != 0 or
 * x_weights, and depth_chunk * nx >= 2^32 (the counters are uint32).  vec = 4 is accepted and read with dword loads (a lane owns a
 * point and walks its members: the wave's load of one member row is coalesced as it is).  nkey == 0 touches nothing; ndepth == 0
 * or nx == 0 zero the partial. */
#define WBX_EPC_CELLS 4        /* TP, FP, FN, TN */
#define WBX_EPC_MAX_PAIRS 16   /* nthr * nslot per launch */
#define WBX_EPC_MAX_MEMBERS 256
int wbx_ens_prob_contingency_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M,
                                     int64_t member_stride, int nthr, const double* thresholds /* DEVICE float64[nthr] */, int nslot,
                                     const int32_t* slots /* DEVICE int32[2 * nslot]: lo, hi */, const void* p, const void* t,
                                     const uint8_t* mask, double* partial_out);

/* ---- stage 1: Brier-type errors of event probabilities (joined ABI 13) -----------------------------------------------
 * Error, AbsoluteError and SquaredError (deterministic.py:91-123) of an event probability against the observed event, behind
 * ContinuousToBinary('both', event thresholds) -> EnsembleMean('predictions') or WeibullEnsembleToProbabilistic('predictions')
 * (wrappers.py): Bias, MAE and MSE / RMSE -- the Brier score -- per threshold, in one pass over p and t: no [nthr][M][frame]
 * indicator array is formed.  p has a member axis of length M and element stride `member_stride` that is not part of key / depth /
 * x, as for wbx_ens_partial.  M == 1 is the deterministic pair behind the first transform alone: `member_stride` is then ignored
 * and `denom` must be 1.
 * Per point, with members x_m (m < M), target y, thresholds a_k = thresholds[k] and D = denom (M: the member mean; M + 1: Weibull's
 * plotting position):
 *     c_k = #{m : (double)x_m > a_k}     o_k = [(double)y > a_k]     e_k = c_k - o_k * D        (strict, on the threshold as given)
 *     lane ERR * nthr + k : e_k / D      lane ABS * nthr + k : |e_k| / D      lane SQ * nthr + k : e_k^2 / D^2
 * Lane order is part of the ABI: WBX_BRIER_STATS * nthr value lanes, stat * nthr + k, stat in (ERR, ABS, SQ) = (0, 1, 2).
 * A comparison with a NaN threshold is false; -0.0 > 0.0 is false; +-inf compare as IEEE says.  float32 inputs are compared in
 * float32 against the threshold rounded toward -inf to float32, exactly as in wbx_contingency_partial.
 * No floating-point number is added anywhere and nothing is added atomically.  A partial is the signed 64-bit sum S of the integer
 * numerators e_k, |e_k| or e_k^2 over its points, written once as (double)S / (double)D (ERR, ABS) or (double)S / (double)(D * D)
 * (SQ): every written value is the correctly rounded quotient of two integers, a function of the inputs and the plan only, bit for
 * bit, in any summation order.
 * A point with a NaN member or a NaN target is a NaN statistic in all 3 * nthr lanes: without flags it poisons every value lane of
 * its partial; under WBX_FLAG_MASKED alone it contributes exactly 0 where the mask is 0 and poisons where it is not; under
 * WBX_FLAG_SKIPNA it is counted out.  Count lanes follow the library's convention (none / one shared / one per value lane); under
 * SKIPNA all of them are equal (the number of valid, non-NaN points).  partial_out[nkey][nchunk][lanes_total][nj] as for
 * wbx_det_partial: wbx_s1_partial_len with lanes = 3 * nthr; wbx_contract, wbx_contract_bits, the accumulators and the chunk records
 * take it unchanged.
 * Refused (WBX_ERR_INVALID, output untouched): nthr outside 1..WBX_BRIER_MAX_THRESHOLDS, M outside 1..WBX_BRIER_MAX_MEMBERS, denom
 * not in {M, M + 1} (not 1 when M == 1), an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask,
 * plane_rows != 0 or x_weights, a NULL threshold table, and depth_chunk * nx * denom^2 >= 2^53 (S must stay exact in fp64).
 * vec = 4 is accepted and read with dword loads (a lane owns a point and walks its members).  nkey == 0 touches nothing;
 * ndepth == 0 or nx == 0 zero the partial. */
#define WBX_BRIER_STATS 3            /* ERR, ABS, SQ */
#define WBX_BRIER_MAX_THRESHOLDS 16  /* per launch */
#define WBX_BRIER_MAX_MEMBERS 256    /* e_k^2 <= (M + 1)^2 fits an int32 */
int wbx_ens_brier_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M, int64_t member_stride,
                          int denom /* M: EnsembleMean; M + 1: Weibull plotting position */, int nthr,
                          const double* thresholds /* DEVICE float64[nthr] */, const void* p, const void* t, const uint8_t* mask,
                          double* partial_out);

/* ---- stage 1: errors of ensemble quantiles (joined ABI 13) ------------------------------------------------------------
 * Error, AbsoluteError and SquaredError (deterministic.py:91-123) of the quantiles of an ensemble against the target, behind
 * EnsembleQuantiles('predictions', quantiles) (wrappers.py:151-211): MAE of the ensemble median, Bias / MSE / RMSE of deciles, in one
 * pass that sorts a point's members once: no float64 [nq][frame] quantile array is formed.  p has a member axis of length M and
 * element stride `member_stride`, which is not part of key / depth / x.  `bounds` is a HOST array of nq wbx_ivl_bound, read during
 * the call; `c_off` is ignored.
 * Per point, with target t:
 *   Members are sorted in the input type (exact).  A flag gathered while they are loaded marks a NaN member (the sort's min / max
 *   drop a NaN: it cannot come from propagation).  Quantile j with the bound (k_j, g_j) -- the host forms h = q (M - 1), k = floor(h),
 *   g = h - k in float64 -- is NumPy's `linear` method in NumPy's order of operations and NumPy's types: with A = x_(k),
 *   B = x_(min(k + 1, M - 1)) and d = B - A formed IN THE INPUT TYPE (np.quantile subtracts the neighbours before the float64 weight
 *   joins: for float32 members d is rounded to float32; wbx_ens_interval_partial widens first and differs there), it is, in float64,
 *       A + d g         where g < 0.5,
 *       B - d (1 - g)   otherwise,
 *   every product and sum rounded on its own, with no shortcut for g == 0 (inf * 0 gives the NaN NumPy gives), and NaN where the flag
 *   is set: np.quantile(members, q) of the members as they are, bit for bit.  Then
 *       e_j = q_j - (double)t
 *       lane ERR * nq + j : e_j      lane ABS * nq + j : |e_j|      lane SQ * nq + j : e_j * e_j
 *   the product rounded before it is added: there is no fused multiply-add between forming a value and accumulating it.
 * Lane order is part of the ABI: WBX_QERR_STATS * nq value lanes, stat * nq + j, stat in (ERR, ABS, SQ) = (0, 1, 2).
 * Sums are float64.  A lane adds its points in the order they come, lanes, waves and blocks are added in fixed orders and nothing is
 * added atomically: a partial is a function of the inputs and the plan only.
 * NaN handling is the deterministic family's: without flags a NaN value poisons its lane of the partial; under WBX_FLAG_MASKED a point
 * adds exactly 0 where the mask is 0 (and poisons where it is not); under WBX_FLAG_SKIPNA a NaN value is counted out of its own lane.
 * Count lanes follow the library's convention (none / one shared under a mask alone / one per value lane under skipna: +-inf members
 * can make one quantile NaN and not another).  partial_out[nkey][nchunk][lanes_total][nj] as for wbx_det_partial:
 * wbx_s1_partial_len with lanes = 3 * nq; wbx_contract, wbx_contract_bits, the accumulators and the chunk records take it unchanged.
 * Refused (WBX_ERR_INVALID, output untouched): M outside 1..WBX_IVL_MAX_MEMBERS, nq outside 1..WBX_QERR_MAX_QUANTILES, a bound with k
 * outside 0..M-1 or g outside [0, 1), NULL `bounds`, an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask,
 * plane_rows != 0 or x_weights, NULL p or t on a non-empty plan.  vec = 4 is accepted and ignored; a block runs block_threads threads
 * up to what its LDS holds (128 for float32, 64 for float64).  nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero the partial. */
#define WBX_QERR_STATS 3           /* ERR, ABS, SQ */
#define WBX_QERR_MAX_QUANTILES 16  /* per launch */
int wbx_ens_quantile_error_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int M,
                                   int64_t member_stride, int nq, const wbx_ivl_bound* bounds /* HOST, nq entries; c_off ignored */,
                                   const void* p, const void* t, const uint8_t* mask, double* partial_out);

/* ---- stage 1: SEEPS from a per-place score table (joined ABI 13) ----------------------------------------------------
 * The stable equitable error in probability space (categorical.py:104-304) of a prediction p against a target t: both are put
 * into a category against the dry threshold and the point's climatological wet threshold, and the pair of categories picks one of
 * nine float64 scores of the PLACE out of a table the host has evaluated, instead of six float64 indicator fields, six products
 * with broadcast coefficient fields, an aligned copy of the wet thresholds and a Boolean mask per chunk.
 * `wet` is input 2 of the plan (key_off[2], depth_off[2], xstride[2], the gather tables; zero strides where it does not vary), in
 * the input type.  `table` is DEVICE float64 and the kernel takes it as opaque numbers: cell (f, o) -- f the category of p, o the
 * category of t -- of the point (key k, depth d, x) is
 *     table[key_off[2][k] + depth_off[2][d] + x * xstride[2] + (3 * f + o) * cell_stride],
 * input 2's address WITHOUT the gather term: the gather selects the time of year, which the table does not depend on.
 * Category of a value v (p or t) against w = the point's `wet`, every comparison in the input type T, the dry threshold rounded
 * to nearest into T first (for float32 inputs that is NOT the float64 comparison: float32(0.00025) > 0.00025, and the value
 * float32(0.00025) is dry here):
 *     0 (dry)    v <= (T)dry_threshold          (tested first)
 *     1 (light)  v >  (T)dry_threshold && v < w
 *     2 (heavy)  v >= w
 *     none       otherwise -- a NaN w with a value that is not dry: the point takes cell (0, 0)
 * so -0.0 and -inf are dry and +inf is heavy unless w is NaN.  PRECONDITION (the caller's, not checked): w > dry_threshold in T, or
 * w is NaN, at every point; a value could otherwise be dry and heavy at once, which the table cannot express.
 * Point value: NaN where p or t is NaN, by an explicit test; the table entry otherwise, handed on as it is (NaN, inf included).
 * ONE value lane.  Count lanes, WBX_FLAG_MASKED, WBX_FLAG_SKIPNA and partial_out[nkey][nchunk][lanes_total][nj] are those of
 * wbx_det_partial with one lane (wbx_s1_partial_len with lanes = 1; wbx_contract and wbx_contract_bits serve it unchanged): a
 * masked-out point contributes exactly 0 whatever its table entry is, a NaN value poisons its partial without flags and under
 * MASKED alone and is counted out under SKIPNA.  Sums are float64 in a fixed order, nothing is added atomically: the partial is a
 * function of the inputs and the plan, bit for bit.
 * Refused (WBX_ERR_INVALID, output untouched): an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask, a
 * NULL p, t, wet or table, plane_rows != 0 or x_weights.  vec = 4 is honoured for the p / t / wet loads where x is summed and ignored
 * where x is kept.  nkey == 0 touches nothing; ndepth == 0 or nx == 0 zero the partial. */
#define WBX_SEEPS_LANES 1
#define WBX_SEEPS_CELLS 9 /* (category of p, category of t), cell 3 * f + o */
int wbx_seeps_partial(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, double dry_threshold, const void* p,
                      const void* t, const void* wet, const double* table /* DEVICE float64 */, int64_t cell_stride,
                      const uint8_t* mask, double* partial_out);

/* ---- stage 1: the three terms of the fractions skill score (joined ABI 13) -------------------------------------------
 * SquaredFractionsError, SquaredPredictionFraction and SquaredTargetFraction (spatial.py:24-277) of a prediction p against a target
 * t at ONE neighbourhood size n, in one sweep over p and t: the n x n neighbourhood means Pf, Tf of both fields are formed from
 * sliding float64 window sums (cost per point independent of n) instead of four whole-array convolutions per size, and the three
 * squares are summed like any other stage-1 statistic.
 * The stencil runs along latitude and longitude, which the stage-1 plan cannot express (latitude is neither key, depth nor x there),
 * so the entry has a plan of its own:
 *   key    k in [0, nkey)     fields that get their own partials
 *   depth  d in [0, ndepth)   fields summed inside the launch, in nchunk chunks of depth_chunk
 *   (y, x) in [0, nlat) x [0, nlon)
 * element address of input i (0 = p, 1 = t, 2 = mask) at (k, d, y, x):
 *     in[i] + key_off[i][k] + depth_off[i][d] + y * lat_stride[i] + x * lon_stride[i]
 * All tables are DEVICE pointers; a NULL table means zeros (a (latitude, longitude)-only mask is two strides and no tables).  Any
 * strides are consumed in place.
 * Per point (y, x), n odd and greater than 1, h = (n - 1) / 2, everything in float64:
 *     S_p = sum of (double)p over the n x n window, NaN members taken as 0;   H_p = the number of NaN members in the window
 *     longitude is cyclic in the window; latitude never has to wrap (every row whose window would is a border row)
 *     Pf = (float)(S_p / (double)(n * n)), or NaN where H_p > 0;   Tf the same from t
 *     border points -- y < h, y >= nlat - h, and x < h or x >= nlon - h unless wrap_longitude -- have Pf = Tf = 0 whatever the
 *     window holds (a NaN included)
 *     value lanes, in float32 arithmetic, then widened:  0 (Pf - Tf)^2,  1 Pf^2,  2 Tf^2          (WBX_FSS_LANES, part of the ABI)
 * n == 1: Pf = p and Tf = t in the INPUT type (float64 stays float64: no float32 rounding), no border; the squares in that type.
 * Count lanes follow the library's convention (none / one shared / one per value lane), exactly as wbx_contingency_partial words it:
 * a NaN lane of a point poisons that lane of its partial without flags; under WBX_FLAG_MASKED alone a point contributes exactly 0
 * where the mask is 0 and poisons where it is not; under WBX_FLAG_SKIPNA a NaN lane of a point is counted out of that lane.  Lane 1
 * does not depend on t's NaNs, nor lane 2 on p's.  The mask is the mask OF THE STATISTIC (what spatial.get_fss_mask returns for this
 * size): the kernel does not erode masks.
 * partial_out[nkey][nlat][nchunk][lanes_total][nj], nj = nlon where x_kept, else 1: the stage-1 partial of a plan with nkey * nlat
 * keys, latitude the fastest key index; wbx_s1_partial_len (with such a plan), wbx_contract and wbx_contract_bits serve it unchanged.
 * Sums: a block of 256 threads owns a (key, chunk, band of B latitudes) and whole circles; a thread owns the columns l + 256 c.  The
 * vertical window sums slide down the band (row y + h enters, row y - h leaves), the horizontal window is a difference of two values
 * of an inclusive prefix over the circle.  The lanes of a row are summed over x as thread -> wave -> the four waves, the fields of a
 * chunk in field order; that order does not depend on B.  No atomics: the result is a function of the inputs, the plan and n, bit for bit.
 * B = WBX_FSS_MAX_BAND_ROWS, halved while B > WBX_FSS_MIN_BAND_ROWS, nkey * nchunk * ceil(nlat / B) < WBX_FSS_TARGET_BLOCKS and
 * B / 2 >= 2 (n - 1) (the halo of n - 1 rows stays at most half a band).
 * Accuracy.  Inputs whose window sums are exact in float64 (0 / 1 indicator fields -- what FSS gets -- and small integers): S is exact
 * in any order, and the fraction is the float32 rounding of the correctly rounded float64 quotient of two integers.  Other inputs,
 * u = 2^-53, M = max |x| over the field: a column sum has seen at most n + 2 B additions of partial sums below n M, a prefix value at
 * most 7 + 6 + 4 + 1 additions of partial sums below nlon n M (its run, the wave scan, the waves in front, the offset; the bound allows
 * 42), and the window is two prefix values, at most two totals and n columns:
 *     |dS| <= u n M (n (n + 2 B) + 84 nlon + 8),     |d(S / n^2)| <= |dS| / n^2 + u |S| / n^2
 * after which the float32 rounding of the fraction (half an ulp of float32; one ulp where dS moves the quotient across a tie)
 * dominates.  +-inf inputs are outside the contract (the host route's running sums turn every later window of such a row into NaN;
 * here inf - inf appears when the value leaves the window).
 * Refused (WBX_ERR_INVALID, output untouched): an even n, n < 1, n > min(nlat, nlon) for n > 1, nlon > WBX_FSS_MAX_NLON (the circle's
 * prefix lives in LDS), an unknown dtype, flags beyond MASKED | SKIPNA, WBX_FLAG_MASKED with a NULL mask.  nkey == 0 touches nothing;
 * ndepth == 0, nlat == 0 or nlon == 0 zero the partial. */
#define WBX_FSS_LANES 3
#define WBX_FSS_MAX_NLON 2048
#define WBX_FSS_MAX_BAND_ROWS 64
#define WBX_FSS_MIN_BAND_ROWS 8
#define WBX_FSS_TARGET_BLOCKS 1024
typedef struct wbx_fss_plan {
  int64_t nkey;
  int64_t ndepth;
  int64_t nlat;
  int64_t nlon;
  int32_t x_kept;         /* 1: keep one partial per longitude (nj = nlon); 0: sum longitude away (nj = 1) */
  int32_t nchunk;         /* depth is cut into nchunk pieces of depth_chunk fields */
  int64_t depth_chunk;
  int64_t lat_stride[3];  /* 0 = p, 1 = t, 2 = mask (uint8) */
  int64_t lon_stride[3];
  const int64_t* key_off[3];   /* [nkey]   or NULL */
  const int64_t* depth_off[3]; /* [ndepth] or NULL */
  uint32_t flags;         /* WBX_FLAG_MASKED | WBX_FLAG_SKIPNA */
  int32_t wrap_longitude; /* 0: the h outermost columns are border points too */
} wbx_fss_plan;
int wbx_fss_partial(wbx_ctx* ctx, const wbx_fss_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int n, const void* p, const void* t,
                    const uint8_t* mask, double* partial_out);

/* ---- stage 1: the FSS terms of thresholded continuous fields (joined ABI 13) -------------------------------------------
 * What FSS is scored on in practice: WrappedMetric(FSS(sizes), [ContinuousToBinary('both', thresholds, dim)]) on a continuous field.
 * The entry takes the CONTINUOUS p and t and the thresholds and forms no indicator field: one call reads p and t once per block of
 * thresholds (see "Launches") instead of once per threshold, and every window sum is an integer count.
 * The plan, its strides, tables and flags, the mask's meaning (the mask of the statistic for this size; it has no threshold axis and
 * serves every threshold), the border rule and wrap_longitude are exactly those of wbx_fss_partial.  The threshold is a LANE, not a
 * plan dim.
 * Per point (y, x) and threshold k, a_k = thresholds[k], n odd and greater than 1:
 *     a member v of a window exceeds a_k where (double)v > a_k -- the host route's float64 comparison.  float32 inputs are compared in
 *     float32 against a_k rounded toward -inf to float32, which is the same predicate (wbx_contingency_partial words it in full);
 *     a NaN threshold is never exceeded; -0.0 > 0.0 is false.  +-inf inputs are ORDINARY numbers here (+inf exceeds every threshold
 *     but +inf and NaN, -inf exceeds none) -- unlike wbx_fss_partial, whose float64 running sums put them outside its contract
 *     C_p,k = the number of members of p's n x n window (longitude cyclic) that exceed a_k;   H_p = the number of NaN members, which
 *     does not depend on k;   C_t,k, H_t the same from t
 *     Pf = (float)((double)C_p,k / (double)(n * n)), or NaN where H_p > 0, and 0 at border points whatever the window holds; Tf alike
 *     value lanes, formed in float32, then widened:  3 k + 0 (Pf - Tf)^2,  3 k + 1 Pf^2,  3 k + 2 Tf^2
 * n == 1: Pf is the indicator itself -- 0, 1, or NaN where the point is NaN -- and there is no border.
 * partial_out[nkey][nlat][nchunk][lanes_total][nj] with 3 * nthr value lanes and the library's count lanes behind them: none; ONE
 * shared lane (3 * nthr) under WBX_FLAG_MASKED alone; one per value lane (3 * nthr + 3 k + l) under WBX_FLAG_SKIPNA.  Hence lanes_total
 * is 3 nthr, 3 nthr + 1 or 6 nthr; wbx_s1_partial_len (lanes = 3 * nthr), wbx_contract and wbx_contract_bits serve it unchanged.
 * Sums.  For every k, lanes 3 k .. 3 k + 2 and their count lanes are BIT FOR BIT what wbx_fss_partial writes under the same plan and
 * n for the float32 fields (p > a_k) and (t > a_k) with NaN kept: the same thread -> wave -> four waves order over x and field order
 * over the depth, independent of the band size.  No atomics.  The two entries are interchangeable.
 * Launches.  A launch carries up to 2 thresholds (the counts of a column and threshold share a 32-bit register, the circle's prefix
 * of a threshold is one 64-bit integer in LDS); the entry cuts nthr into runs of 2 and launches them one after another on the
 * context's stream, each writing its own lane slice of the partial (the shared count lane belongs to the first).
 * Refused (WBX_ERR_INVALID, output untouched): everything wbx_fss_partial refuses, nthr < 1, nthr > WBX_FSS_THR_MAX, a NULL threshold
 * table.  nkey == 0 touches nothing; ndepth == 0, nlat == 0 or nlon == 0 zero the partial. */
#define WBX_FSS_THR_MAX 16
int wbx_fss_threshold_partial(wbx_ctx* ctx, const wbx_fss_plan* plan, int dtype /* WBX_F32 | WBX_F64 */, int n, int nthr,
                              const double* thresholds /* DEVICE, [nthr] */, const void* p, const void* t, const uint8_t* mask,
                              double* partial_out);

/* ---- fused binned reduction (small depth, many boolean bins) -------------------------------------------------
 * Statistic, weight and bin membership in ONE pass over p, t, c -- for chunks where little is reduced before the
 * weight/bin-dependent dims, so that the stage-1 partials would be larger than the inputs (the public benchmark's
 * 1 init x 12 lead chunks with 34 region x land/sea bins, run_benchmark_evaluation.py:97-131,369-382).
 * The plan's keys must be ordered [nA][nBk][nBr] (as for wbx_contract); x is summed; `w_on_x` (WBX_BINNED_* flags) says
 * whether wt / bits are indexed [nBk][nBr][nx] (WBX_BINNED_W_ON_X: W depends on x) or [nBk][nBr][1], and whether the
 * weights come factored: WBX_BINNED_WT_X_ONLY -> wt[nBk][nx] (GridAreaWeighting, weighting.py:62-130, on
 * latitude-fastest chunks), WBX_BINNED_WT_ROW_ONLY -> wt[nBk][nBr] (the same on longitude-fastest chunks); `bits` keeps
 * its full index either way.  out[nA][nBk][lanes_total][nbin], lanes_total and NaN semantics exactly as
 * wbx_det_partial + wbx_contract_bits.  The plan's nchunk / x_kept / vec are ignored.
 * `wt` must not be NULL (WBX_ERR_INVALID; wbx_ens_binned takes NULL as ones, this entry point does not).  An x stride that is
 * negative, or with which a row spans 2^31 bytes or more, in any input sends EVERY patch through the slot kernel (det_binned_kernel:
 * about half the speed; the atom kernel addresses a row as a uniform base plus an unsigned 32-bit lane offset).
 * Non-finite statistics: a NaN statistic under a valid point makes its lane NaN in every bin of its (A, Bk) cell, whatever the
 * point's weight or membership (a zero weight, a point in no bin), as the reference's xr.dot does; so does an INFINITE statistic
 * (+-inf * 0 of the sum it went into is added to every bin), where the reference keeps +-inf in the bins the point belongs to.
 * Accuracy of every output against the float64 restatement of the widened inputs (the lanes above, each term the rounded product
 * lane * wt, summed exactly): |d out| <= (N + 4) eps / 2 * sum |wt_i lane_i| over the N valid points of the cell inside the bin,
 * eps = 2^-52, in any order of the sums (atom or slot kernel, prepared tables or not), count lanes included; integer-valued lanes
 * under unit weights are exact.  tests/test_gpu_det_binned.py holds every output of every mode (DET3 / DET6 / PASS1 x mask modes x
 * weight layouts x float32 / float64), route and edge to that bound, computed per output from the inputs (tests/det_binned_cases.py). */
#define WBX_BINNED_W_ON_X 1
#define WBX_BINNED_WT_X_ONLY 2
#define WBX_BINNED_WT_ROW_ONLY 4
#define WBX_BINNED_TWIN_MASK 16 /* wbx_ens_binned with WBX_FLAG_MASKED: 12 output lanes instead of 6 -- lanes 0-5 with the mask applied,
                                   lanes 6-11 the same statistics over ALL points (mask ignored) from the same pass over the members */
#define WBX_BINNED_ACCUMULATE 32 /* (ABI 12) out[i] += result[i] instead of out[i] = result[i]: `out` is an accumulator of a chunk loop
                                    (the caller's CombinePerKey(CombiningSum()), beam_pipeline.py:509-510) and the launch adds its sums into
                                    it itself -- one thread per element reads, adds and writes, in the kernel that forms the sums, so
                                    there is no wbx_acc_add launch (4 us + a dependency gap) behind a 0.3 ms chunk.  wbx_det_binned and
                                    wbx_ens_binned; an empty reduction (no rows) then leaves `out` as it is */
#define WBX_BINNED_MASK_ON_W 8 /* the validity mask (WBX_FLAG_MASKED) depends on the Bk / Br / x dims only (a (latitude, longitude)
                                  mask under Regions bins): its byte is folded into the atom-id byte, one load less per point.
                                  wbx_ens_binned without this flag: a per-point mask (strides along any dim), see there */
/* `atoms`: NULL, or the tables wbx_binned_atoms wrote for exactly this geometry (plan extents, nA, nBk, nBr, w_on_x) and
 * these `bits`.  The kernel works on a patch's "atoms" (= its distinct membership words: regions are boxes, so a patch
 * of 64 x ~150 rows sees a handful) and needs every point's atom index; the tables depend on the bins and the geometry
 * only, so a chunk loop computes them once.  With NULL they are recomputed inside every call. */
int wbx_det_binned(wbx_ctx* ctx, const wbx_s1_plan* plan, int func, int dtype, const void* p, const void* t,
                   const void* c, const uint8_t* mask, const double* wt, const uint64_t* bits, int64_t nA,
                   int64_t nBk, int64_t nBr, int32_t w_on_x, int32_t nbin, const void* atoms, double* out);
int wbx_binned_atoms_size(const wbx_s1_plan* plan, int64_t nA, int64_t nBk, int64_t nBr, int32_t w_on_x,
                          int64_t* bytes_out);
int wbx_binned_atoms(wbx_ctx* ctx, const wbx_s1_plan* plan, int64_t nA, int64_t nBk, int64_t nBr, int32_t w_on_x,
                     const uint64_t* bits, void* atoms_out /* device, wbx_binned_atoms_size bytes */);

/* ---- fused binned reduction of the ensemble family ---------------------------------------------------------------
 * The public benchmark's probabilistic configuration (public_benchmark/run_benchmark_evaluation.py:341-354, 365-382): CRPS /
 * spread-skill / ensemble-mean RMSE under Regions x land-sea bins, GridAreaWeighting and masked=True.  Replaces
 * probabilistic.py:116-336 + wrappers.py:116-148 + the two xr.dot of aggregation.py:337-366 for every ensemble statistic of a
 * (predictions, targets) pair: the M members of a point are read ONCE (no full-map partial is written), sorted in registers,
 * and the five lanes go straight into the bins.
 *   out[nA][nBk][6][nbin]: lanes 0-4 = the WBX_ENS_LANES of wbx_ens_partial, weighted and binned like wbx_det_binned does;
 *                          lane 5 = the sum of the weights of the valid points of the bin (the count lane, with and without mask).
 * plan / nA / nBk / nBr / bits / nbin / w_on_x as for wbx_det_binned, with these restrictions (WBX_ERR_INVALID otherwise; the
 * two-stage route wbx_ens_partial + wbx_contract_bits covers the rest):
 *   dtype WBX_F32, algo WBX_ENS_SORT (the pair form gives the same number), 2 <= M <= 64, plan->flags within
 *   FAIR | MASKED | SKIPNA;
 *   weights factored: WBX_BINNED_WT_X_ONLY (wt[nBk][nx]) or WBX_BINNED_WT_ROW_ONLY (wt[nBk][nBr]), or wt = NULL (ones);
 *   a mask (WBX_FLAG_MASKED) needs WBX_BINNED_W_ON_X.  It is addressed as input 3 of the plan (key_off[3] / depth_off[3] /
 *   xstride[3], one byte per element).  With WBX_BINNED_MASK_ON_W the caller says that it depends on the Bk / Br / x dims only (a
 *   (latitude, longitude) mask: zero strides along A and the depth dims).  WITHOUT that flag (ABI 11) it may have strides along
 *   any dim -- the per-point mask data_loaders/base.py:25-56 (add_nan_mask_to_data) builds: `mask = ~isnan(data)` over every dim
 *   of the data, which Aggregator(masked=True) consumes (aggregation.py:339-352).  Same single pass over the members; one more
 *   byte per point is read (209 instead of 208 for 51 members).
 * WBX_BINNED_TWIN_MASK (with a mask): out[nA][nBk][12][nbin] -- lanes 0-5 as above with the mask applied, lanes 6-11 the same six over
 * ALL points.  The reference masks the skill / unbiased-MSE / mean-MSE statistics of a variable whose targets carry a `mask`
 * coordinate but not its spread / variance (statistics of the predictions alone, probabilistic.py:165-273, aggregation.py:339-352):
 * both sets come out of ONE pass (masked-out points are accumulated under their atom's twin).
 * WBX_FLAG_SKIPNA (ABI 11; Aggregator(skipna=True), aggregation.py:343-344, 353-355: `mask & ~stat.isnull()` statistic by
 * statistic): out[nA][nBk][10][nbin] = the five value lanes with their NaN points left out, then five count lanes = the sum of the
 * weights of the points each statistic was valid at (the layout of wbx_ens_partial + wbx_contract_bits under SKIPNA).  Skill,
 * unbiased MSE and MSE of the mean are NaN where the target or a member is; spread and variance where a member is (an infinite
 * member counts as NaN here, as in every rank-form kernel of this library).  With WBX_BINNED_TWIN_MASK: out[nA][nBk][20][nbin] --
 * the ten over the valid points of the mask, then the ten over all points; of the first ten the spread / variance lanes (1, 2)
 * and of the second ten the target lanes (0, 3, 4) are NaN: they are not among the sums the pass forms, and the reference's
 * statistics never ask for them (a statistic of the predictions alone carries no mask).
 * `atoms`: NULL, or the tables wbx_ens_binned_atoms wrote for this geometry and these bits (its patches are shorter than
 * wbx_det_binned's, so the tables are its own).  *overflow_out = number of patches with more than 32 distinct membership
 * words (bins that are not boxes): when it is not zero use the two-stage route -- wbx_ens_binned would return NaN for the
 * cells of those patches.  wbx_ens_binned_atoms synchronises when overflow_out is not NULL.
 * Accuracy: as wbx_ens_partial (fp32 chain sums per point for M = 50 / 51, fp64 from the point's values on); lane 3 is formed
 * per (patch, bin) as lane 4 - lane 2 / M from the fp64 sums (the identity holds at every point).  Every output against the float64
 * restatement of the widened inputs: |d out| <= sum_i wt_i b_i + (N + 4) eps / 2 * sum_i |wt_i lane_i| over the N valid points of the
 * cell inside the bin, b_i = the per-point bound of wbx_ens_partial for that M and eps = 2^-52, in any order of the sums (flushes,
 * patches, the three levels, prepared tables or not); lane 3 takes lane 4's bound plus lane 2's / M; count lanes under dyadic weights
 * are exact.  tests/test_gpu_ens_binned.py holds every output of every output mode (6 / 12 / 10 / 20 lanes), mask kind, register
 * bucket, route and edge to that bound, computed per output from the inputs (tests/ens_binned_cases.py). */
int wbx_ens_binned(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride, int algo, const void* p,
                   const void* t, const uint8_t* mask, const double* wt, const uint64_t* bits, int64_t nA, int64_t nBk,
                   int64_t nBr, int32_t w_on_x, int32_t nbin, const void* atoms, double* out);
int wbx_ens_binned_atoms_size(const wbx_s1_plan* plan, int64_t nA, int64_t nBk, int64_t nBr, int32_t w_on_x,
                              int64_t* bytes_out);
int wbx_ens_binned_atoms(wbx_ctx* ctx, const wbx_s1_plan* plan, int64_t nA, int64_t nBk, int64_t nBr, int32_t w_on_x,
                         const uint64_t* bits, void* atoms_out /* device, wbx_ens_binned_atoms_size bytes */,
                         int64_t* overflow_out /* host, or NULL */);

/* ---- materialisation of per-point statistics --------------------------------
 * Statistic.compute()'s full-resolution result (metrics/base.py:135-158) for callers
 * that really want it (unaggregated pipelines, beam_pipeline.py:563-595).
 * Uses the same plan tables with nchunk == 1, writes out[key][depth][x] (C order, fp64)
 * for one lane of the family. */
int wbx_det_map(wbx_ctx* ctx, const wbx_s1_plan* plan, int func, int dtype, int lane,
                const void* p, const void* t, const void* c, double* out);
int wbx_ens_map(wbx_ctx* ctx, const wbx_s1_plan* plan, int dtype, int M, int64_t member_stride,
                int algo, int lane, const void* p, const void* t, double* out);

/* ---- zonal energy spectrum ---------------------------------------------------
 * Not in the reference snapshot (no spectrum metric, no test) -> parity unpinned; definition of the
 * build (WeatherBench-2 lineage): F = rfft(row) / nlon, S_k = |F_k|^2 * (k == 0 ? 1 : 2), k = 0..nlon/2.
 * `field` holds nrows rows consumed IN PLACE: element i of row r is field[r * row_stride + i * lon_stride]
 * (lon-fastest: lon_stride 1, row_stride nlon; latitude-fastest real data: lon_stride nlat, row_stride 1).
 * Contiguous rows with 2/3/5-smooth length: one fused kernel (in-LDS FFT + |.|^2 reduction, the field is read once);
 * otherwise a batched 1-D R2C rocFFT along longitude, then a HIP |.|^2 reduction:
 *   power_out[group[r]][k] (+)= scale[r] * S_k(row r)
 * group[nrows] (int32 in [0, ngroup)) and scale[nrows] (float64, e.g. area weight / count) are device arrays;
 * power_out is float64[ngroup][nlon/2 + 1]; accumulate = 0 overwrites it, 1 adds to it.
 * Order of the sums (round 5; every route, also wbx_det_spectrum / wbx_det_spectrum_slabs): NO atomics on the result path.
 * A team of the transform kernel sums the rows it walks (a fixed share of the launch geometry, in row order) in registers
 * and stores the sums of each run of one group as a RECORD (group, key = (team, sequence number), nlon/2 + 1 values) in a
 * scratch store of the context; a closing kernel on the same stream then adds every group's records in KEY order -- the
 * result is a function of (inputs, launch geometry) only and bit-identical from run to run
 * (tests/test_gpu_round5.py::test_spectra_are_bit_reproducible, ::test_fused_det_spectra_are_bit_reproducible: 20 runs each).  `group` and `scale` are read by this call's
 * kernels in stream order; the number of group changes along `group` is cached per (pointer, nrows) to size the store and
 * the cache entry is dropped by every write this library makes into the table (wbx_memcpy_h2d*, wbx_memset, wbx_memcpy_d2d):
 * a table rewritten by anybody else's kernel must go through one of those calls first (a stale count that is too small does not
 * give wrong sums: the records that do not fit set every value of the call's result to NaN).
 * Cost against round 4's atomics on the same box: +3.1 % (lon-fastest), +2.7 % (lat-fastest), +3.7 % (fused det + spectra);
 * profiles/r05_spectra_records_ab.txt.
 * Accuracy (the one family that is not held to north_star's 1e-6 per value: the transform itself is fp32, only |F|^2 and the
 * sums over rows are fp64).  1440-point rows (0.25 degree grids, both layouts): a row is shifted by an estimate of its mean
 * before the transform and F_0 is restored in fp64, so the error does not scale with the field's mean --
 * |dS_k| <= 2e-6 S_k + 1e-6 sqrt(S'_max S_k), S'_max = max_{k >= 1} S_k, and S_0 to 1e-6, per row against float64 numpy.fft
 * (tests/test_spectra.py::bound_1440).  The relative error of S_k depends on how far S_k sits below S'_max, so it is quoted per
 * kind of row (tests/test_spectra_red.py, profiles/spectrum_accuracy_red_rows.txt; 1440 points, per-row median / area-weighted
 * mean over 200 rows, wavenumbers 1-9 | 10-99 | 100-299 | 300-599 | 600-720):
 *   white rows (280 +- 10):      1.1e-7 / <= 1e-7 in every band -- the 1e-7 after a mean over 200 rows holds for white rows only;
 *   k^-3 rows (temperature-like): 8.5e-8 | 6.3e-7 | 4.3e-6 | 1.5e-5 | 2.8e-5 / 3.4e-8 | 7.1e-7 | 9.0e-6 | 2.0e-5 | 2.2e-5;
 *   k^-5 rows (geopotential-like, 5.4e4 +- 1e3): 1.5e-7 | 1.8e-5 | 4.6e-4 | 3.8e-3 | 1.1e-2 / up to 1.6e-2 (300-599), 0.18 (600-720).
 * That is the fp32 floor of any single-precision transform of those rows (tools/spectrum_fp32_floor.py emulates one on the CPU):
 * per row the one-wave kernels, the generic kernel, the fused det + spectra sweep and the rocFFT route measure 0.5x - 1.6x of
 * it; after a mean over 200 rows 0.1x - 7.4x (the mean of the floor itself varies several-fold from one set of rows to the
 * next).  The |dF|^2 term of a coefficient the row has (almost) none of is up to 5e-15 S'_max.  Every other length the
 * generic fused kernel takes (even, 2/3/5-smooth half length, <= 2048 points: the 64- and 240-point grids of the public
 * configs on one-wave teams, 360 / 720 / 1024 points on teams of two or four waves) is shifted the same way and held to the
 * same bound.  The rocFFT route (odd lengths, prime factors > 5, rows that are not 8-byte aligned, WBX_SPECTRUM_PATH=rocfft)
 * shifts the rows too: a pre-pass (shift_rows_kernel) subtracts each row's mean (fp64 sum, rounded to fp32) into a contiguous
 * scratch tile, rocFFT transforms that, and power_kernel puts X_0 = X'_0 + n m back in fp64: |dS_k| <= 2e-5 S_k + 4e-7
 * sqrt(S_max S_k) with S_max including the mean.  F_0 itself: within 5e-16 of the oracle's S_0 on rows near 280 on every
 * route but the lon-fastest one-wave kernel (8.6e-8, fp32-like, inside its 1e-6; tests/test_spectra_red.py (e)). */
int wbx_zonal_spectrum(wbx_ctx* ctx, const float* field, int64_t lon_stride, int64_t row_stride, int64_t nrows,
                       int32_t nlon, const int32_t* group, const double* scale, int32_t ngroup,
                       int32_t accumulate, double* power_out);

/* The same over `nslab` slabs of `rows_per_slab` uniformly strided rows each: row i of slab o starts at
 * field + h_slab_offsets[o] + i * row_stride (h_slab_offsets is a HOST int64 array of element offsets; group / scale are
 * indexed by o * rows_per_slab + i).  A latitude-fastest field [lead, level, longitude, latitude] is lead x level slabs
 * of `latitude` adjacent rows (row_stride 1, lon_stride = nlat): those are transposed tile by tile into contiguous rows
 * and fed to the fused kernel in one call instead of one strided library batch per slab. */
int wbx_zonal_spectrum_slabs(wbx_ctx* ctx, const float* field, int64_t lon_stride, int64_t row_stride,
                             int64_t rows_per_slab, int64_t nslab, const int64_t* h_slab_offsets, int32_t nlon,
                             const int32_t* group, const double* scale, int32_t ngroup, int32_t accumulate,
                             double* power_out);

/* ---- spectra + deterministic lanes in one sweep ---------------------------------------------------------------------
 * configs[3] / configs[4]: "spectra of p and t + the full deterministic suite in the same sweep".  One launch
 * reads every row of p, t (and c for WBX_DET6) ONCE -- 12 B/point instead of 20 for wbx_det_partial + two wbx_zonal_spectrum
 * launches -- and produces
 *   partial_out[key][lane]      exactly what wbx_det_partial writes for this plan (nchunk = 1): the unweighted per-row sums of
 *                               e, |e|, e^2 (, (p-c)^2, (t-c)^2, (p-c)(t-c)); wbx_contract consumes it unchanged
 *   power_p / power_t[g][k]     what wbx_zonal_spectrum returns for the rows of p resp. t: sum over the rows of group g of
 *                               scale[row] * S_k(row), k = 0 .. 720; overwritten (ordered sums, see wbx_zonal_spectrum)
 * `plan` is the deterministic plan of (p, t[, c]) with x = longitude (nx = 1440, unit x strides, even row offsets), summed,
 * ndepth = 1, nchunk = 1, no mask: a row of the spectra = a key of the plan, group / scale are indexed by key.
 * Spectrum accuracy: as wbx_zonal_spectrum on 1440-point rows (fp32 transform of the mean-shifted rows); the deterministic lanes
 * are fp64 sums of the widened inputs like wbx_det_partial (1e-12).  Parity unpinned for the spectra. */
int wbx_det_spectrum(wbx_ctx* ctx, const wbx_s1_plan* plan, int func /* WBX_DET3 | WBX_DET6 */, int dtype /* WBX_F32 */,
                     const void* p, const void* t, const void* c, const int32_t* group, const double* scale, int64_t ngroup,
                     double* partial_out, double* power_p, double* power_t);

/* The same sweep with stage 2 of the deterministic lanes folded in (round 6).  Where the aggregation's W is a weight per ROW of
 * the plan and the rows of a group are exactly the rows stage 2 would sum into one output -- GridAreaWeighting over
 * (init_time, latitude, longitude), the spectra averaged over (init_time, latitude): configs[3] / configs[4] -- the kernel
 * multiplies every row's sums by det_scale[row] and adds them up with the spectra's records:
 *   det_out[g][lane] = sum over the rows of group g of det_scale[row] * (sum over the row of lane's statistic)
 * = what wbx_contract would make of wbx_det_spectrum's partial_out with that W: [ngroup][3 | 6], overwritten; ordered sums (the
 * records of a group are added in key order), fp64.  It saves the six fp64 wave sums and stores per row (6 % of the kernel) and
 * the 25 MB partial + its contraction.  `group`, `scale`, `det_scale` are device arrays indexed by key. */
int wbx_det_spectrum_folded(wbx_ctx* ctx, const wbx_s1_plan* plan, int func /* WBX_DET3 | WBX_DET6 */, int dtype /* WBX_F32 */,
                            const void* p, const void* t, const void* c, const int32_t* group, const double* scale,
                            const double* det_scale, int64_t ngroup, double* det_out, double* power_p, double* power_t);

/* The same for LATITUDE-FASTEST fields (the layout of the public ERA5 / WeatherBench archives, [.., longitude, latitude];
 * weatherbenchX/data_loaders/xarray_loaders.py:185-188 hands such chunks on as they are stored): `plan` is the deterministic
 * plan of (p, t[, c]) with x = longitude (nx = 1440, summed, ndepth = 1, nchunk = 1, no mask) whose keys are nkey /
 * rows_per_slab slabs of `rows_per_slab` rows each: key o * rows_per_slab + r is row r of slab o, and the rows of a slab are
 * ADJACENT elements of every input (row r + 1 = row r + 1 element; plan->xstride[i] = the longitude stride of input i,
 * >= rows_per_slab).  Outputs and accuracy as wbx_det_spectrum; the deterministic sums of a row are formed in a fixed order
 * (no atomics). */
int wbx_det_spectrum_slabs(wbx_ctx* ctx, const wbx_s1_plan* plan, int func /* WBX_DET3 | WBX_DET6 */, int dtype /* WBX_F32 */,
                           const void* p, const void* t, const void* c, int64_t rows_per_slab, const int32_t* group,
                           const double* scale, int64_t ngroup, double* partial_out, double* power_p, double* power_t);

/* ---- replayable chunk records (ABI 11) ---------------------------------------------------------------------------
 * The body of the reference's per-chunk stage (beam_pipeline.py:161-250: statistics of one chunk -> aggregation states ->
 * CombinePerKey) is, in steady state, the SAME sequence of calls into this library chunk after chunk: same plans, same
 * weights / bins / atom tables, same scratch and accumulator slots; only the inputs' device pointers (and, for statistics
 * against a climatology, the plan variant that carries the chunk's gather table) change.  A caller that has watched one such
 * chunk -- every call with its arguments as 64-bit patterns -- replays the following chunks with ONE call: the host side of
 * a chunk is then a few microseconds whatever the number of metrics, variables and aggregators (a public-benchmark chunk is
 * ~0.35 ms of kernel against 0.3-0.45 ms of Python bookkeeping through the per-call path).
 *   calls[i]   = {fn, nargs, args[]}: entry point WBX_FN_* with its arguments in declaration order, each as the 64-bit pattern
 *                of the value (pointers as addresses, integers sign-extended, a double as its IEEE bits);
 *   relocs[j]  = {call, arg, slot, offset}: before the calls run, calls[call].args[arg] = slots[slot] + offset -- the
 *                arguments that follow the chunk (input pointers, a plan variant);
 *   slots[]    = this chunk's values.
 * The calls run in order, each on the context it names, exactly as if the caller had made them one by one; the first failure
 * stops the replay and is returned (wbx_last_error says which call).  Only entry points that enqueue work and neither allocate
 * nor synchronise can be part of a record (WBX_ERR_INVALID otherwise): */
typedef enum wbx_fn {
  WBX_FN_DET_PARTIAL = 1, WBX_FN_ENS_PARTIAL = 2, WBX_FN_ENS2_PARTIAL = 3, WBX_FN_CAT_PARTIAL = 4, WBX_FN_CAT_EXCEED_FIELD = 5,
  WBX_FN_CONTRACT = 6, WBX_FN_CONTRACT_BITS = 7, WBX_FN_DET_BINNED = 8, WBX_FN_ENS_BINNED = 9, WBX_FN_ZONAL_SPECTRUM = 10,
  WBX_FN_ZONAL_SPECTRUM_SLABS = 11, WBX_FN_DET_SPECTRUM = 12, WBX_FN_DET_SPECTRUM_SLABS = 13, WBX_FN_ACC_ADD = 14,
  WBX_FN_MEMSET = 15, WBX_FN_MEMCPY_D2D = 16, WBX_FN_CTX_WAIT_FENCE = 17, WBX_FN_FENCE_RECORD = 18, WBX_FN_DET_SPECTRUM_FOLDED = 19,
  WBX_FN_CONTINGENCY_PARTIAL = 20, WBX_FN_ENS_RPS_PARTIAL = 21, WBX_FN_ENS_ENERGY_PARTIAL = 22,
  WBX_FN_ENS_VARIOGRAM_PARTIAL = 23, WBX_FN_ENS_WASSERSTEIN_PARTIAL = 24, WBX_FN_ENS_INTERVAL_PARTIAL = 25,
  WBX_FN_ENS_PROB_CONTINGENCY_PARTIAL = 26, WBX_FN_SEEPS_PARTIAL = 27, WBX_FN_FSS_PARTIAL = 28,
  WBX_FN_ENS_BRIER_PARTIAL = 29, WBX_FN_FSS_THRESHOLD_PARTIAL = 30, WBX_FN_ENS_RPS_FIELD_PARTIAL = 31,
  WBX_FN_ENS_QUANTILE_ERROR_PARTIAL = 32
} wbx_fn;
#define WBX_CALL_MAX_ARGS 20
typedef struct wbx_call {
  int32_t fn;     /* wbx_fn */
  int32_t nargs;  /* must equal the entry point's parameter count */
  uint64_t args[WBX_CALL_MAX_ARGS];
} wbx_call;
typedef struct wbx_reloc {
  int32_t call, arg, slot, reserved_;
  int64_t offset; /* bytes */
} wbx_reloc;
/* `calls` is patched in place (it belongs to the caller and is rewritten by every replay). */
int wbx_chunk_replay(wbx_call* calls, int32_t ncalls, const wbx_reloc* relocs, int32_t nrelocs, const uint64_t* slots,
                     int32_t nslots);

#ifdef __cplusplus
}
#endif
#endif /* WBX_H_ */
