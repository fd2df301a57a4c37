// Seasonal (Mondrian) conformal calibration: the offsets of conformal.hip kept per time-of-day bucket (include/stemgnn_hip.h:
// stemgnn_seasonal_* / stemgnn_quantile_store_seasonal).
//
// Every target has an integer time index t; step h of row i has t = o_i + h with o_i the row's origin (a device int64 [count],
// or origin0 + i, or -- the live store -- t_dev[0] + i).  bucket(t) = (u * K) / period with u = (t + phase) mod period in the
// floor sense.  Within a bucket everything is conformal.hip's definition: the key, the rank, the exact MSB-first radix select
// (conformal_select.h, conformal_fit.h), the band widening (conformal_args.h).  Tables are [K, P, Hg, Ng], the bucket slowest,
// so one bucket's slice is exactly a table of stemgnn_conformal_fit and cf_widen is pointed at it.
//
// This file holds the season itself -- the bucket arithmetic and the two policies the shared kernels are instantiated with --
// the streaming apply, and the entries with their checks.
//
// fit:   the kernels and the four passes of conformal_fit.h over K * P tables.  A histogram workgroup owns ONE bucket
//        (blockIdx.z = s * P + p): SsWalk tells it which rows to walk.  It works out the element's u from (i, h) and skips what
//        lies outside the bucket's range [u_lo, u_hi) of u BEFORE target / forecast are loaded, so the memory traffic stays
//        that of the unseasoned fit; the K-fold walk costs integer work only.  With consecutive origins the rows of a bucket
//        come in runs of period / K every `period` rows, and the workgroup enumerates them instead (DIRECT): 1 / K of the walk.
// apply: one streaming launch, a wave per (i, h) row segment: the bucket is worked out once per segment on the scalar unit,
//        the lanes then stream the Q runs of N floats (float4 when N % 4 == 0 and the buffers are 16-byte aligned).
// apply with rearrange / the live store: the column kernel of quantile_column.h, SsSlice choosing the table per (window, h).
// Only vector stores, and integer atomicAdd on LDS / global histogram counters.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/stemgnn_hip.h"
#include "calibration_plan.h"
#include "conformal_args.h"
#include "conformal_fit.h"
#include "conformal_select.h"
#include "devattr.h"
#include "quantile_column.h"
#include "sg_host.h"

namespace {

// SS_THREADS, the choice between the two walks of the fit and the grids of the applies: calibration_plan.h

// where a row's origin comes from, and the season; by value.  origin0 has been reduced into [0, period) by the host (the bucket
// depends on t mod period only), so origin0 + i + h stays far from any overflow.
struct SsTime {
  const long long* origins;                 // int64 [count], or NULL
  const long long* t_dev;                   // int64 [1] (the live store), or NULL
  long long origin0;
  uint32_t period, K, phase;
};

// u = (t + phase) mod period, floor sense; period < 2^31, phase < period
__host__ __device__ inline uint32_t ss_u(long long t, uint32_t period, uint32_t phase) {
  uint32_t r;
  if ((unsigned long long)t < (1ull << 31)) {
    r = (uint32_t)t % period;
  } else {
    long long q = t % (long long)period;
    if (q < 0) q += period;
    r = (uint32_t)q;
  }
  r += phase;                               // < 2^32
  return r >= period ? r - period : r;
}
// bucket of u: (u * K) / period; u * K < 2^47
__host__ __device__ inline uint32_t ss_bucket_of_u(uint32_t u, uint32_t period, uint32_t K) {
  const unsigned long long prod = (unsigned long long)u * K;
  return prod < (1ull << 32) ? (uint32_t)prod / period : (uint32_t)(prod / period);
}
__device__ inline long long ss_origin(const SsTime& tm, long long i) {
  if (tm.origins) return tm.origins[i];
  return (tm.t_dev ? tm.t_dev[0] : tm.origin0) + i;
}
__device__ inline uint32_t ss_bucket(const SsTime& tm, long long i, int h) {
  return ss_bucket_of_u(ss_u(ss_origin(tm, i) + h, tm.period, tm.phase), tm.period, tm.K);
}
// the u of bucket s are [ceil(s * period / K), ceil((s + 1) * period / K)): u K / period == s  <=>  s period <= u K < (s + 1) period
__device__ inline uint32_t ss_u_from(uint32_t s, uint32_t period, uint32_t K) {
  return (uint32_t)(((unsigned long long)s * period + K - 1) / K);
}

// DIRECT (consecutive origins, o_i = origin0 + i): the rows of bucket s at step h are runs of len = u_hi - u_lo rows, one run
// every `period` rows, so they are enumerated instead of found by skipping: virtual row v (run v / len, place v % len) is row
// first(h) - period + run * period + place, with first(h) in [0, period) the first row whose u is u_lo -- the run before it
// may straddle row 0.  Rows outside [0, count) are dropped.  dd = (u_lo - u(0, 0)) mod period.
struct SsDirect {
  int count, runs;                          // runs = count / period + 2 covers every run that meets [0, count)
};
__device__ inline long long ss_direct_row(int v, uint32_t len, uint32_t dd, int h, uint32_t period) {
  const uint32_t run = (uint32_t)v / len, place = (uint32_t)v - run * len;
  const uint32_t first = (dd + period - (uint32_t)h % period) % period;
  return (long long)first - (long long)period + (long long)run * period + place;
}

// the season policy of conformal_fit.h's kernels: blockIdx.z = s * P + p, bucket s walks its own rows.  z and P are not
// negative and are divided as unsigned: the signed division costs the prologue five scalar instructions more, which moved the
// skipping form's loop within its 64-byte line and its time by 2-4 %.
template <bool DIRECT>
struct SsWalk {
  static constexpr bool seasoned = true;
  int N, P;
  SsTime tm;
  SsDirect dr;
  struct Bucket {
    uint32_t u_lo, u_hi, dd;
  };
  __device__ int pair(int z) const { return (int)((uint32_t)z % (uint32_t)P); }
  __device__ Bucket bucket(int z) const {
    const uint32_t s = (uint32_t)z / (uint32_t)P, u_lo = ss_u_from(s, tm.period, tm.K);
    return {u_lo, ss_u_from(s + 1, tm.period, tm.K), (u_lo + tm.period - ss_u(tm.origin0, tm.period, tm.phase)) % tm.period};
  }
  // rows (elements) to walk: `per` for each of the bucket's virtual rows, or all of them
  __device__ int walked(const Bucket& b, int all, int per) const { return DIRECT ? dr.runs * (int)(b.u_hi - b.u_lo) * per : all; }
  __device__ bool window(const Bucket& b, int& i, int h) const {
    if (DIRECT) {
      const long long row = ss_direct_row(i, b.u_hi - b.u_lo, b.dd, h, tm.period);
      if (row < 0 || row >= dr.count) return false;
      i = (int)row;
      return true;
    }
    const uint32_t u = ss_u(ss_origin(tm, i) + h, tm.period, tm.phase);
    return u >= b.u_lo && u < b.u_hi;
  }
};

// the season policy of quantile_column.h's kernel: the tables' slice of step h of window i
struct SsSlice {
  static constexpr bool seasoned = true;
  SsTime tm;
  size_t table;                             // P * Hg * Ng
  __device__ size_t slice(long long i, int h) const { return (size_t)ss_bucket(tm, i, h) * table; }
};

// ---- apply, streaming -----------------------------------------------------------------------------------------------------
// A wave per (i, h) row segment: its Q runs of N floats.  The segment index is made wave-uniform, so the origin load and the
// bucket arithmetic run once per segment on the scalar unit.  forecast and out may be the same buffer: a lane reads its own
// elements before it writes them.
template <int VEC>
__global__ __launch_bounds__(SS_THREADS) void ss_apply(const float* forecast, const float* __restrict__ offsets,
                                                       long long segments, int Q, int H, int N, CfRoles roles, int P, int Hg,
                                                       int Ng, SsTime tm, float* out) {
  const int lane = threadIdx.x & 63;
  const long long w0 = (long long)blockIdx.x * (SS_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long stride = (long long)gridDim.x * (SS_THREADS / 64);
  const int per = N / VEC, items = Q * per;
  const size_t table = (size_t)P * Hg * Ng;
  for (long long seg = w0; seg < segments; seg += stride) {
    const long long i = seg / H;
    const int h = (int)(seg - i * H);
    const float* o = offsets + (size_t)ss_bucket(tm, i, h) * table;
    const size_t base = ((size_t)i * Q * H + h) * (size_t)N;
    for (int it = lane; it < items; it += 64) {
      const int q = it / per, n = (it - q * per) * VEC;
      const size_t e = base + (size_t)q * H * N + n;
      float v[VEC];
      cf_load<VEC>(forecast + e, v);
      cf_widen<VEC>(v, roles.role[q], o, Hg, Ng, h, n);
      cf_store<VEC>(out + e, v);
    }
  }
}

// ---- host checks ----------------------------------------------------------------------------------------------------------
bool ss_season_ok(long long period, int K, long long phase) {
  return period >= 1 && period < (1ll << 31) && K >= 1 && (long long)K <= period && phase >= 0 && phase < period;
}
// the season and the sizes the kernels index with: P K <= 65535 (grid.z), K P G < 2^29 (the pick's int indices)
bool ss_sizes_ok(int H, int N, int P, int K, int per_step, int per_node) {
  if ((long long)P * K > 65535) return false;
  return (long long)K * P * (long long)cf_grouping(per_step, per_node, H, N).groups() < (1ll << 29);
}
long long ss_floor_mod(long long t, long long period) {
  long long r = t % period;
  return r < 0 ? r + period : r;
}
SsTime ss_time(const long long* origins, const long long* t_dev, long long origin0, long long period, int K, long long phase) {
  return {origins, t_dev, ss_floor_mod(origin0, period), (uint32_t)period, (uint32_t)K, (uint32_t)phase};
}

// the column kernel's arguments of both seasonal entries, checked; `gr` gives the table's size
bool ss_column_args(long count, int Q, int H, int N, int rearrange, const float* offsets, int P, const int* lo_rows,
                    const int* hi_rows, int per_step, int per_node, long long period, int K, long long phase, QcArgs* a) {
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &a->roles)) return false;
  if (!ss_season_ok(period, K, phase) || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return false;
  qc_stages(a, Q, H, N, rearrange, offsets, per_step, per_node);
  return true;
}

}  // namespace

extern "C" int stemgnn_season_bucket(long long t, long long period, int K, long long phase) {
  if (!ss_season_ok(period, K, phase)) return -1;
  return (int)ss_bucket_of_u(ss_u(t, (uint32_t)period, (uint32_t)phase), (uint32_t)period, (uint32_t)K);
}

extern "C" size_t stemgnn_seasonal_scratch_bytes(long count, int H, int N, int P, int K, int per_step, int per_node) {
  if (!cf_shapes_ok(count, 1, H, N, P) || K < 1 || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return 0;
  return cf_fit_scratch_bytes((long long)K * P, cf_grouping(per_step, per_node, H, N).groups());
}

extern "C" int stemgnn_seasonal_fit(const float* target, const float* forecast, const long long* origins, long long origin0,
                                    long count, int Q, int H, int N, int P, const int* lo_rows, const int* hi_rows,
                                    const double* coverage, int per_step, int per_node, int masked, long long period, int K,
                                    long long phase, void* scratch, float* offsets, long long* counts, void* stream) {
  if (!target || !forecast || !lo_rows || !hi_rows || !coverage || !scratch || !offsets || !counts) return SG_EINVAL;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, nullptr)) return SG_EINVAL;
  if (!ss_season_ok(period, K, phase) || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return SG_EINVAL;
  if (!sg_aligned16(scratch)) return SG_EINVAL;
  CfPairs pairs;
  if (!cf_fit_pairs(P, lo_rows, hi_rows, coverage, &pairs)) return SG_EINVAL;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  if (!per_node && gr.groups() > 65535) return SG_EINVAL;              // grid.y of the stream form
  const SsTime tm = ss_time(origins, nullptr, origin0, period, K, phase);
  // DIRECT (a bucket's rows enumerated) or skipping through all of them: ss_fit_walk of calibration_plan.h
  const SsFitWalk wk = ss_fit_walk(count, period, K, origins != nullptr);
  const SsDirect dr = {(int)count, wk.runs};
  if (wk.direct)
    return cf_fit_run(target, forecast, count, wk.walk, Q, H, N, P, K * P, pairs, gr, per_node != 0, masked != 0,
                      SsWalk<true>{N, P, tm, dr}, scratch, offsets, counts, (hipStream_t)stream);
  return cf_fit_run(target, forecast, count, count, Q, H, N, P, K * P, pairs, gr, per_node != 0, masked != 0,
                    SsWalk<false>{N, P, tm, dr}, scratch, offsets, counts, (hipStream_t)stream);
}

extern "C" int stemgnn_seasonal_apply(const float* forecast, const float* offsets, const long long* origins,
                                      long long origin0, long count, int Q, int H, int N, int rearrange, int P,
                                      const int* lo_rows, const int* hi_rows, int per_step, int per_node, long long period,
                                      int K, long long phase, float* out, void* stream) {
  if (!forecast || !offsets || !lo_rows || !hi_rows || !out) return SG_EINVAL;
  QcArgs a = {};
  if (!ss_column_args(count, Q, H, N, rearrange, offsets, P, lo_rows, hi_rows, per_step, per_node, period, K, phase, &a))
    return SG_EINVAL;
  const SsTime tm = ss_time(origins, nullptr, origin0, period, K, phase);
  if (rearrange) {
    a.src = forecast;
    a.dst = out;
    return qc_launch(a, count, qc_vec_ok(N, Q, forecast, out), SsSlice{tm, (size_t)P * a.Hg * a.Ng}, (hipStream_t)stream);
  }
  CfApplyPlan pl;                                   // VEC, the grid and its cap: calibration_plan.h
  ss_apply_plan(count, Q, H, N, sg_aligned16(forecast) && sg_aligned16(out), sg_num_cus(), &pl);
  const long long segments = (long long)count * H;
  const unsigned blocks = pl.blocks;
  if (pl.vec == 4)
    hipLaunchKernelGGL(ss_apply<4>, dim3(blocks), dim3(SS_THREADS), 0, (hipStream_t)stream, forecast, offsets, segments, Q, H, N,
                       a.roles, P, a.Hg, a.Ng, tm, out);
  else
    hipLaunchKernelGGL(ss_apply<1>, dim3(blocks), dim3(SS_THREADS), 0, (hipStream_t)stream, forecast, offsets, segments, Q, H, N,
                       a.roles, P, a.Hg, a.Ng, tm, out);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_quantile_store_seasonal(const float* steps, const float* target, const long long* pos,
                                               const long long* t_dev, int B, int Q, int H, int N, int rearrange,
                                               const float* offsets, int P, const int* lo_rows, const int* hi_rows,
                                               int per_step, int per_node, long long period, int K, long long phase,
                                               float* out_forecast, float* out_target, long capacity, void* stream) {
  if (!steps || !target || !pos || !t_dev || !offsets || !lo_rows || !hi_rows || !out_forecast || !out_target || capacity <= 0)
    return SG_EINVAL;
  QcArgs a = {};
  if (!ss_column_args(B, Q, H, N, rearrange, offsets, P, lo_rows, hi_rows, per_step, per_node, period, K, phase, &a))
    return SG_EINVAL;
  a.src = steps;
  a.dst = out_forecast;
  qc_store_to(&a, target, pos, out_target, capacity);
  const SsSlice sn = {ss_time(nullptr, t_dev, 0, period, K, phase), (size_t)P * a.Hg * a.Ng};
  return qc_launch(a, B, qc_vec_ok(N, Q, steps, out_forecast), sn, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------------
// What the launchers of the batch side -- this file's, conformal.hip's and quantile_serve.hip's -- do for a shape
// (include/stemgnn_hip.h: stemgnn_calibration_plan): host only, nothing is launched or read.  Every number comes from the
// function of calibration_plan.h the launcher itself calls, with the compute-unit count the launcher itself asks for.
static inline bool cp_int(long v) { return v >= 0 && v <= 0x7fffffffl; }

extern "C" int stemgnn_calibration_plan(int entry, const long* shape, int nshape, int misaligned, int* out) {
  static const int want[] = {6, 9, 4, 4, 6};
  if (!out || !shape || misaligned < 0 || entry < 0 || entry > SG_CALIBRATION_COLUMN || nshape != want[entry]) return SG_EINVAL;
  for (int i = 1; i < nshape; ++i)
    if (!(cp_int(shape[i]) || (entry == SG_CALIBRATION_SEASONAL_FIT && i == 6))) return SG_EINVAL;
  int w[SG_CALIBRATION_PLAN_WORDS] = {};
  const long count = shape[0];
  const int i1 = (int)shape[1], i2 = (int)shape[2], i3 = (int)shape[3];
  const int cus = sg_num_cus();
  w[6] = cus;
  switch (entry) {
    case SG_CALIBRATION_FIT:
    case SG_CALIBRATION_SEASONAL_FIT: {             // (count, H, N, P, per_step, per_node [, period, K, has_origins])
      const int H = i1, N = i2, P = i3, per_step = shape[4] != 0, per_node = shape[5] != 0;
      if (misaligned || !cf_shapes_ok(count, 1, H, N, P)) return SG_EINVAL;
      const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
      if (!per_node && gr.groups() > 65535) return SG_EINVAL;
      int KP = P;
      long long walked = count;
      if (entry == SG_CALIBRATION_FIT) {
        if ((long long)P * (long long)gr.groups() >= (1ll << 31) / 4) return SG_EINVAL;
        w[28] = 0, w[29] = -1;
      } else {
        const long long period = shape[6];
        const int K = (int)shape[7];
        if (!ss_season_ok(period, K, 0) || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return SG_EINVAL;
        const SsFitWalk wk = ss_fit_walk(count, period, K, shape[8] != 0);
        KP = K * P, walked = wk.walked;
        w[28] = wk.direct, w[29] = wk.why, w[30] = wk.runs, w[31] = (int)std::min<long long>(wk.walk, 0x7fffffff);
      }
      CfFitPlan p;
      cf_fit_plan(walked, KP, gr, per_node != 0, cus, &p);
      w[0] = p.form, w[4] = CF_THREADS, w[3] = KP;
      if (p.form == 0) w[1] = p.tiles, w[2] = p.launched;
      else w[1] = p.launched, w[2] = p.G;
      w[7] = KP, w[8] = p.G, w[9] = gr.Cc, w[10] = gr.Hr, w[11] = gr.L, w[12] = gr.G;
      w[13] = p.tiles, w[14] = p.wd_last, w[15] = p.rpw_full, w[16] = p.rpw_last, w[17] = p.form == 0 ? CF_TILE : 0;
      w[18] = p.chunks, w[19] = p.per_chunk, w[20] = p.bound, w[21] = p.trips, w[22] = p.want, w[23] = p.by_size;
      w[24] = p.blocks_wanted, w[25] = (int)p.pick_blocks, w[26] = p.pick_idle, w[27] = p.rows;
      break;
    }
    case SG_CALIBRATION_APPLY:
    case SG_CALIBRATION_SEASONAL_APPLY: {           // (count, Q, H, N); misaligned: bit 0 forecast, bit 1 out
      if (misaligned > 3 || !cf_shapes_ok(count, i1, i2, i3, 1)) return SG_EINVAL;
      CfApplyPlan p;
      if (entry == SG_CALIBRATION_APPLY) cf_apply_plan(count, i1, i2, i3, misaligned == 0, cus, &p);
      else ss_apply_plan(count, i1, i2, i3, misaligned == 0, cus, &p);
      w[1] = (int)p.blocks, w[2] = w[3] = 1, w[4] = entry == SG_CALIBRATION_APPLY ? CF_THREADS : SS_THREADS, w[5] = p.vec;
      w[7] = (int)std::min<long long>(p.needed, 0x7fffffff), w[8] = (int)p.cap, w[9] = p.capped;
      w[10] = (int)std::min<long long>(p.trips, 0x7fffffff), w[11] = p.lane_trips, w[12] = p.items;
      break;
    }
    case SG_CALIBRATION_COLUMN: {                   // (count, Q, H, N, rearrange, store); misaligned: src, dst, target, out_target
      const int Q = i1, H = i2, N = i3, store = shape[5] != 0;
      if (count <= 0 || !cp_int(count) || Q <= 0 || H <= 0 || N <= 0 || Q > CF_MAX_Q || (long long)H * N >= (1ll << 31)) return SG_EINVAL;
      if (misaligned > (store ? 15 : 3)) return SG_EINVAL;
      QcPlan p;
      qc_plan(count, Q, H * N, shape[4] != 0, qc_vec_shape_ok(N, Q) && (misaligned & 3) == 0, store, cus, &p);
      w[1] = (int)p.gx, w[2] = (int)p.gy, w[3] = 1, w[4] = p.T, w[5] = p.vec;
      w[7] = (int)p.lds, w[8] = p.planes, w[9] = p.cpb, w[10] = p.wpb, w[11] = p.idle, w[12] = p.col_blocks, w[13] = p.cols_last;
      w[14] = p.win_blocks, w[15] = p.capped, w[16] = (int)std::min<long long>(p.win_trips, 0x7fffffff);
      w[17] = store ? ((qc_tvec_shape_ok(H * N) && (misaligned & 12) == 0) ? 4 : 1) : 0;
      w[18] = (int)std::min<long long>(p.target_trips, 0x7fffffff), w[19] = p.per;
      break;
    }
    default: return SG_EINVAL;
  }
  for (int i = 0; i < SG_CALIBRATION_PLAN_WORDS; ++i) out[i] = w[i];
  return 0;
}
