// Streaming conformal anomaly detection for live readings (include/stemgnn_hip.h: stemgnn_anomaly_update).
//
// One call judges ONE arrived row tau: every stored forecast of it (step h of origin tau - h) is scored with the score of
// conformal_select.h, ranked against the rolling window of the scores of the last M - 1 judged rows (every window slot except
// `slot`, which this call overwrites: no thread reads what another writes, so one launch needs no grid-wide synchronisation),
// and the H opinions about a node's reading are combined by Bonferroni.  Counts are integers, the only atomics are integer adds
// (in LDS, and of per-workgroup partial counts into the work buffer), the two divisions are single fp64 operations: the same
// bits on every run.
//
// Two forms, chosen by the grouping (those of aci.hip, for the same reasons; the groups themselves: cf_grouping, conformal_args.h):
//   * columns (per_node): a query meets at most (M - 1) * H scores, strided by N.  A workgroup owns 32 adjacent nodes:
//     consecutive lanes on consecutive nodes (coalesced 128-byte rows), 32 row lanes split the window's rows, up to four
//     queries per node ride one pass over the population, the row lanes meet in integer LDS adds.  With H <= 4 a workgroup
//     owns all steps of its nodes, row lane 0 of a node sees all its p-values and the per-node combination runs in the same
//     launch: ONE launch.  A longer horizon is spread over more workgroups -- (node tiles) x (steps: one each with per_step,
//     four each without) x (parts of the window's rows), about 192 in all -- because eight workgroups alone cannot keep
//     enough loads in flight for a window that no longer fits one L2; their integer partial counts meet in the caller's
//     work buffer and the finishing launch below combines: TWO launches.
//   * pooled (over the nodes): a group's queries (N with per_step, H * N without) meet up to (M - 1) * H * N scores.  Linear
//     in the population instead of queries x population: the queries are sorted in LDS (bitonic, 64-bit key | index), every
//     population key is dropped into the interval between neighbouring queries (binary search, integer LDS add), a suffix
//     sum turns the interval counts into "scores >= query".  The population of a group is dealt over up to 64 workgroups
//     (each sorts the same queries again, which is cheap, and ranks its share); their integer partial counts meet in the
//     caller's work buffer by integer global atomics: TWO launches.  More than 4096 queries go through in batches of 4096,
//     one pass over the share each.
// The finishing launch is ONE workgroup: it turns the totals in the work buffer into p-values, combines per node and leaves
// the buffer zero again.  The two launches are ordered by the launch boundary: no arrival counter, no fence.
// Both run 1024 threads.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "serving_plan.h"
#include "sg_host.h"

namespace {

// (AN_THREADS, AN_TILE, AN_ROWS, AN_QC, AN_BATCH and the caps of the two spreads: serving_plan.h, with the launch geometry)

struct AnIn {
  const float* slab;
  const long long* origins;
  const float* ring_y;
  int S, R, lo, hi, C, H, N;
  long long row;
};

struct AnOut {
  float *scores, *pvalues, *node_p;
  int* alarm;
  long long *counts, *alarm_sum, *judged_sum;
  float* log_row;
};

// (the key of a stored score: cf_score_key of conformal_select.h; NaN = absent is skipped by the caller)

// steps 1 and 2 of element (h, n) of the arrived row: the key of its score, CF_KEY_ABSENT without a target or a forecast
__device__ inline uint32_t an_query(const AnIn& in, int h, int n) {
  const float y = in.ring_y[(size_t)(in.row % in.C) * in.N + n];
  if (y != y) return CF_KEY_ABSENT;
  size_t s = 0;
  if (in.origins) {
    const long long o = in.row - h;
    if (o < 0) return CF_KEY_ABSENT;
    s = (size_t)(o % in.S);
    if (in.origins[s] != o) return CF_KEY_ABSENT;
  }
  const size_t HN = (size_t)in.H * in.N, at = (size_t)h * in.N + n;
  const float* f = in.slab + s * in.R * HN + at;
  return cf_key(f[in.lo * HN], y, f[in.hi * HN]);
}

__device__ inline float an_score(uint32_t key) { return key == CF_KEY_ABSENT ? __uint_as_float(CF_NAN_BITS) : cf_unkey(key); }

// step 4: one fp64 division, rounded once more to fp32
__device__ inline float an_pvalue(bool absent, uint32_t ge, uint32_t m, long long min_scores) {
  if (absent || (long long)m < min_scores) return __uint_as_float(CF_NAN_BITS);
  return (float)((double)(ge + 1u) / (double)(m + 1u));
}

// the per-node combination, by ONE thread per node
__device__ inline void an_node(int n, int v, float pmin, double alpha, const AnOut& out) {
  float np = __uint_as_float(CF_NAN_BITS);
  int al = 0;
  if (v) {
    const double t = (double)v * (double)pmin;
    np = (float)(t < 1.0 ? t : 1.0);
    al = (double)np <= alpha;
  }
  out.node_p[n] = np;
  out.alarm[n] = al;
  out.judged_sum[n] += v > 0;
  out.alarm_sum[n] += al;
  out.log_row[n] = np;
}

// ---- column form ------------------------------------------------------------------------------------------------------
// grid (node tiles, step spans, row parts): the workgroup owns steps [y * hspan, (y + 1) * hspan) of its nodes and every
// gridDim.z-th stretch of 32 population rows.  Alone (one span, one part) it finishes and combines per node; otherwise it adds
// its counts into work ([h * N + n]: scores >= the query; [H * N + group]: m) and part 0 files the scores.
// Thread (lr, lc): node n = tile * 32 + lc, population rows lr + 32 * z, + 32 * parts, ...
__global__ __launch_bounds__(AN_THREADS) void anomaly_columns(AnIn in, int M, int slot, long long min_scores, double alpha,
                                                              int per_step, int hspan, uint32_t* __restrict__ work, AnOut out) {
  __shared__ uint32_t s_ge[AN_QC * AN_TILE], s_m[AN_QC * AN_TILE];
  const int tid = threadIdx.x, lc = tid & (AN_TILE - 1), lr = tid >> 5;
  const int H = in.H, N = in.N, n = blockIdx.x * AN_TILE + lc;
  const size_t HN = (size_t)H * N;
  const bool live = n < N, split = gridDim.y * gridDim.z > 1;
  const int row0 = lr + AN_ROWS * blockIdx.z, row_step = AN_ROWS * gridDim.z;
  int v = 0;                                      // (row lane 0 only) the node's judged steps and their smallest p
  float pmin = INFINITY;
  const int h_begin = blockIdx.y * hspan, h_end = min(H, h_begin + hspan);
  for (int h0 = h_begin; h0 < h_end; h0 += AN_QC) {
    if (tid < AN_QC * AN_TILE) s_ge[tid] = 0u, s_m[tid] = 0u;
    __syncthreads();
    uint32_t q[AN_QC], ge[AN_QC], m[AN_QC];
#pragma unroll
    for (int j = 0; j < AN_QC; ++j) {
      q[j] = (live && h0 + j < h_end) ? an_query(in, h0 + j, n) : CF_KEY_ABSENT;
      ge[j] = m[j] = 0u;
    }
    if (live) {
      if (per_step) {                             // the population of (h, n): scores[i, h, n], i != slot
#pragma unroll
        for (int j = 0; j < AN_QC; ++j) {
          if (h0 + j >= h_end) continue;
          const float* col = out.scores + (size_t)(h0 + j) * N + n;
#pragma unroll 8
          for (int i = row0; i < M; i += row_step) {   // branch-free: the loads of an unrolled round go out together
            const float s = col[(size_t)i * HN];
            const uint32_t ok = (i != slot) & (s == s);
            m[j] += ok;
            ge[j] += ok & (uint32_t)(cf_score_key(s) >= q[j]);
          }
        }
      } else {                                    // the population of node n: scores[i, :, n], i != slot; row r = i * H + h
        const uint32_t rows = (uint32_t)M * H;    // < 2^31: the unsigned counter cannot wrap
        const uint32_t slot0 = (uint32_t)slot * H;  // the slot's rows are [slot0, slot0 + H)
        uint32_t mm = 0u;
#pragma unroll 8
        for (uint32_t r = row0; r < rows; r += row_step) {
          const float s = out.scores[(size_t)r * N + n];
          const uint32_t ok = ((r - slot0) >= (uint32_t)H) & (s == s), k = cf_score_key(s);    // (unsigned: below slot0 wraps high)
          mm += ok;
#pragma unroll
          for (int j = 0; j < AN_QC; ++j) ge[j] += ok & (uint32_t)(k >= q[j]);
        }
#pragma unroll
        for (int j = 0; j < AN_QC; ++j) m[j] = mm;
      }
#pragma unroll
      for (int j = 0; j < AN_QC; ++j) {
        if (ge[j]) atomicAdd(&s_ge[j * AN_TILE + lc], ge[j]);
        if (m[j]) atomicAdd(&s_m[j * AN_TILE + lc], m[j]);
      }
    }
    __syncthreads();
    if (live && lr == 0) {
#pragma unroll
      for (int j = 0; j < AN_QC; ++j) {
        const int h = h0 + j;
        if (h >= h_end) continue;
        const uint32_t mt = s_m[j * AN_TILE + lc];
        const size_t at = (size_t)h * N + n;
        if (split) {
          if (blockIdx.z == 0) out.scores[(size_t)slot * HN + at] = an_score(q[j]);
          if (s_ge[j * AN_TILE + lc]) atomicAdd(&work[at], s_ge[j * AN_TILE + lc]);
          if (mt && (per_step || h == 0)) atomicAdd(&work[HN + (per_step ? at : (size_t)n)], mt);
          continue;
        }
        const float p = an_pvalue(q[j] == CF_KEY_ABSENT, s_ge[j * AN_TILE + lc], mt, min_scores);
        out.scores[(size_t)slot * HN + at] = an_score(q[j]);
        out.pvalues[at] = p;
        if (p == p) {
          ++v;
          pmin = fminf(pmin, p);
        }
        if (per_step)
          out.counts[at] = (long long)mt;
        else if (h == 0)
          out.counts[n] = (long long)mt;
      }
    }
    __syncthreads();                              // the sums are read before the next round clears them
  }
  if (live && lr == 0 && !split) an_node(n, v, pmin, alpha, out);
}

// ---- pooled form ------------------------------------------------------------------------------------------------------
// grid (G, parts).  Group g = the L contiguous floats at offset g * L of every [H * N] slab (L = N with per_step, H * N
// without); part y ranks every parts-th stretch of 1024 * VEC population keys and adds its counts into work: [h * N + n] the
// scores >= the query of (h, n), [H * N + g] the group's m.  VEC = 4: N % 4 == 0 and scores 16-byte aligned, so a float4 of
// the population never leaves a row of N.
template <int VEC>
__global__ __launch_bounds__(AN_THREADS) void anomaly_pooled(AnIn in, int M, int slot, int L, float* __restrict__ scores,
                                                             uint32_t* __restrict__ work) {
  __shared__ unsigned long long s_q[AN_BATCH];    // (key << 32) | index in the batch, ascending after the sort
  __shared__ uint32_t s_cnt[AN_BATCH + 1];        // [j]: population keys with exactly j queries <= them; then its suffix sums
  __shared__ uint32_t s_part[AN_THREADS];
  const int tid = threadIdx.x, g = blockIdx.x, part = blockIdx.y, parts = gridDim.y, N = in.N;
  const size_t HN = (size_t)in.H * N;
  const int base = g * L;
  const uint32_t total = (uint32_t)M * L;         // < 2^31: the unsigned counter below cannot wrap
  for (int b0 = 0; b0 < L; b0 += AN_BATCH) {
    const int nb = min(AN_BATCH, L - b0);
    int P2 = 1;
    while (P2 < nb) P2 <<= 1;
    // 1, 2, 5: the batch's queries; their scores into the window's slot (part 0)
    for (int t = tid; t < P2; t += AN_THREADS) {
      unsigned long long e = ~0ull;
      if (t < nb) {
        const int el = base + b0 + t, h = el / N;
        const uint32_t k = an_query(in, h, el - h * N);
        if (part == 0) scores[(size_t)slot * HN + el] = an_score(k);
        e = ((unsigned long long)k << 32) | (uint32_t)t;
      }
      s_q[t] = e;
    }
    for (int t = tid; t <= nb; t += AN_THREADS) s_cnt[t] = 0u;
    __syncthreads();
    for (int k = 2; k <= P2; k <<= 1) {           // bitonic sort, ascending
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < P2; t += AN_THREADS) {
          const int x = t ^ j;
          if (x > t) {
            const unsigned long long a = s_q[t], b = s_q[x];
            if ((a > b) == ((t & k) == 0)) s_q[t] = b, s_q[x] = a;
          }
        }
        __syncthreads();
      }
    }
    // 3: every population key into the interval j = the number of queries <= it (absent queries sort above every key)
#pragma unroll 2
    for (uint32_t e = (uint32_t)(part * AN_THREADS + tid) * VEC; e < total; e += (uint32_t)parts * AN_THREADS * VEC) {
      const uint32_t i = e / L, t = e - i * L;
      if ((int)i == slot) continue;
      float s[VEC];
      cf_load<VEC>(scores + (size_t)i * HN + base + t, s);
#pragma unroll
      for (int c = 0; c < VEC; ++c) {
        if (s[c] != s[c]) continue;
        const uint32_t key = cf_score_key(s[c]);
        int lo = 0, hi = nb;
        while (lo < hi) {
          const int mid = (lo + hi) >> 1;
          if ((uint32_t)(s_q[mid] >> 32) <= key) lo = mid + 1; else hi = mid;
        }
        atomicAdd(&s_cnt[lo], 1u);
      }
    }
    __syncthreads();
    // suffix sums of s_cnt[0 .. nb]: a thread owns `chunk` adjacent entries
    const int n1 = nb + 1, chunk = (n1 + AN_THREADS - 1) / AN_THREADS;
    const int c0 = min(n1, tid * chunk), c1 = min(n1, c0 + chunk);
    {
      uint32_t own = 0u;
      for (int i = c0; i < c1; ++i) own += s_cnt[i];
      s_part[tid] = own;
    }
    __syncthreads();
    for (int off = 1; off < AN_THREADS; off <<= 1) {
      const uint32_t up = tid + off < AN_THREADS ? s_part[tid + off] : 0u;
      __syncthreads();
      s_part[tid] += up;
      __syncthreads();
    }
    {
      uint32_t run = tid + 1 < AN_THREADS ? s_part[tid + 1] : 0u;
      for (int i = c1 - 1; i >= c0; --i) {
        run += s_cnt[i];
        s_cnt[i] = run;
      }
    }
    __syncthreads();
    // the query at sorted position t has s_cnt[t + 1] of this part's keys >= it (a key below it has at most t queries <= it,
    // a key at or above it at least t + 1, ties among the queries included); this part's share of m = s_cnt[0]
    for (int t = tid; t < nb; t += AN_THREADS) {
      const uint32_t ge = s_cnt[t + 1];
      if (ge) atomicAdd(&work[base + b0 + (int)(uint32_t)s_q[t]], ge);
    }
    if (tid == 0 && b0 == 0 && s_cnt[0]) atomicAdd(&work[HN + g], s_cnt[0]);
    __syncthreads();                              // s_q and s_cnt are read before the next batch overwrites them
  }
}

// ---- finish ------------------------------------------------------------------------------------------------------------
// Step 4 and the per-node combination behind every two-launch form, ONE workgroup (its barrier is what separates "every thread
// has read m" from "clear m"): a thread per node takes the totals of its H elements out of work, which it leaves zero for the
// next call.  An element is absent iff the first launch filed NaN for it.
__global__ __launch_bounds__(AN_THREADS) void anomaly_finish(int H, int N, int slot, long long min_scores, double alpha,
                                                             int per_step, int per_node, uint32_t* __restrict__ work,
                                                             AnOut out) {
  // (the group of (h, n) and the number of groups are CfGrouping::group / groups of conformal_args.h written out: through the
  // struct this kernel compiled to other code that timed slower than the spread allows in two isolated figures)
  const size_t HN = (size_t)H * N;
  for (int n = threadIdx.x; n < N; n += AN_THREADS) {
    int v = 0;
    float pmin = INFINITY;
    for (int h = 0; h < H; ++h) {
      const size_t at = (size_t)h * N + n;
      const size_t g = per_node ? (per_step ? at : (size_t)n) : (per_step ? (size_t)h : 0);
      const float s = out.scores[(size_t)slot * HN + at];
      const float p = an_pvalue(s != s, work[at], work[HN + g], min_scores);
      work[at] = 0u;
      out.pvalues[at] = p;
      if (p == p) {
        ++v;
        pmin = fminf(pmin, p);
      }
    }
    an_node(n, v, pmin, alpha, out);
  }
  __syncthreads();
  const size_t G = (size_t)(per_step ? H : 1) * (per_node ? N : 1);
  for (size_t g = threadIdx.x; g < G; g += AN_THREADS) {
    out.counts[g] = (long long)work[HN + g];
    work[HN + g] = 0u;
  }
}

}  // namespace

extern "C" int stemgnn_anomaly_update(const float* slab, int S, int R, int lo_row, int hi_row, const long long* origins,
                                      long long row, const float* ring_y, int C, int H, int N, int M, int slot,
                                      long long min_scores, double alpha, int per_step, int per_node, float* scores,
                                      float* pvalues, float* node_p, int* alarm, long long* counts, long long* alarm_sum,
                                      long long* judged_sum, float* log_p, int keep, int log_slot, unsigned int* work,
                                      void* stream) {
  if (!slab || !ring_y || !scores || !pvalues || !node_p || !alarm || !counts || !alarm_sum || !judged_sum || !log_p || !work)
    return SG_EINVAL;
  if (S <= 0 || R <= 0 || C <= 0 || H <= 0 || N <= 0 || M <= 0 || keep <= 0 || R > 32) return SG_EINVAL;
  if (lo_row < 0 || lo_row > hi_row || hi_row >= R) return SG_EINVAL;
  if (slot < 0 || slot >= M || log_slot < 0 || log_slot >= keep || row < 0 || min_scores < 0) return SG_EINVAL;
  if (!(alpha > 0.0 && alpha < 1.0)) return SG_EINVAL;                         // NaN fails both
  const long long lim = 1ll << 31, HN = (long long)H * N;
  if (HN >= lim || (long long)M * HN >= lim || (long long)C * N >= lim || (long long)R * HN >= lim ||
      (long long)S * ((long long)R * HN) >= lim || (long long)keep * N >= lim)
    return SG_EINVAL;
  const AnIn in = {slab, origins, ring_y, S, R, lo_row, hi_row, C, H, N, row};
  const AnOut out = {scores, pvalues, node_p, alarm, counts, alarm_sum, judged_sum, log_p + (size_t)log_slot * N};
  hipStream_t s = (hipStream_t)stream;
  AnPlan pl;
  if (!an_plan(H, N, M, per_step, per_node, sg_aligned16(scores), &pl)) return SG_EINVAL;
  const dim3 grid(pl.gx, pl.gy, pl.gz);
  if (pl.form == 0) {
    hipLaunchKernelGGL(anomaly_columns, grid, dim3(AN_THREADS), 0, s, in, M, slot, min_scores, alpha, per_step, pl.hspan, work, out);
    SG_TRY(hipGetLastError());
    if (pl.launches == 2) {
      hipLaunchKernelGGL(anomaly_finish, dim3(1), dim3(AN_THREADS), 0, s, H, N, slot, min_scores, alpha, per_step, 1, work, out);
      SG_TRY(hipGetLastError());
    }
    return 0;
  }
  if (pl.vec == 4)
    hipLaunchKernelGGL(anomaly_pooled<4>, grid, dim3(AN_THREADS), 0, s, in, M, slot, pl.L, scores, work);
  else
    hipLaunchKernelGGL(anomaly_pooled<1>, grid, dim3(AN_THREADS), 0, s, in, M, slot, pl.L, scores, work);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(anomaly_finish, dim3(1), dim3(AN_THREADS), 0, s, H, N, slot, min_scores, alpha, per_step, 0, work, out);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// What the serving launchers -- this file's, aci.hip's and live.hip's -- do for a shape (include/stemgnn_hip.h:
// stemgnn_serving_plan): host only, nothing is launched or read.  Every number comes from the function of serving_plan.h the
// launcher itself calls.
static inline bool sv_int(long v) { return v >= -0x7fffffffl - 1 && v <= 0x7fffffffl; }

extern "C" int stemgnn_serving_plan(int entry, long a0, long a1, long a2, long a3, long a4, long a5, int misaligned, int* out) {
  if (!out || misaligned < 0) return SG_EINVAL;
  int w[SG_SERVING_PLAN_WORDS] = {};
  const int i0 = (int)a0, i1 = (int)a1, i2 = (int)a2, i3 = (int)a3;
  switch (entry) {
    case SG_SERVING_PUSH: {                       // (K, N, C)
      LvPushPlan p;
      if (!(sv_int(a0) && sv_int(a1) && sv_int(a2)) || misaligned || !lv_push_plan(i0, i1, i2, &p)) return SG_EINVAL;
      w[1] = (int)p.blocks, w[2] = w[3] = 1, w[4] = p.threads, w[6] = 1, w[7] = p.k0;
      break;
    }
    case SG_SERVING_GATHER: {                     // (C, N, B, L); misaligned: bit 0 ring, bit 1 out
      LvGatherPlan p;
      if (!(sv_int(a0) && sv_int(a1) && sv_int(a2) && sv_int(a3)) || misaligned > 3) return SG_EINVAL;
      if (!lv_gather_plan(i0, i1, i2, i3, misaligned == 0, &p)) return SG_EINVAL;
      w[1] = i3, w[2] = i2, w[3] = 1, w[4] = p.threads, w[5] = p.vec, w[6] = 1, w[7] = p.trips;
      break;
    }
    case SG_SERVING_ACI: {                        // (H, N, P, M, per_step, per_node); misaligned: issued, raw, ring_y, scores
      AciPlan p;
      if (!(sv_int(a0) && sv_int(a1) && sv_int(a2) && sv_int(a3)) || misaligned > 15) return SG_EINVAL;
      if (i3 <= 0 || !cf_shapes_ok(i3, 1, i0, i1, i2)) return SG_EINVAL;
      aci_plan(i0, i1, i2, i3, a4 != 0, a5 != 0, misaligned == 0, &p);
      w[0] = p.form, w[1] = (int)p.gx, w[2] = (int)p.gy, w[3] = 1, w[4] = ACI_THREADS, w[5] = p.vec, w[6] = 1;
      w[7] = p.gr.Cc, w[8] = p.gr.Hr, w[9] = p.gr.L, w[10] = p.gr.G, w[11] = p.wd_last, w[12] = p.keep;
      w[13] = p.step[0], w[14] = p.step[1], w[15] = p.pass_trips[0], w[16] = p.pass_trips[1];
      w[17] = p.origin_trips[0], w[18] = p.origin_trips[1], w[19] = p.form == 0 ? ACI_TILE : 0;
      break;
    }
    case SG_SERVING_ANOMALY: {                    // (H, N, M, per_step, per_node); misaligned: bit 0 scores
      AnPlan p;
      if (!(sv_int(a0) && sv_int(a1) && sv_int(a2)) || misaligned > 1) return SG_EINVAL;
      if (i0 <= 0 || i1 <= 0 || i2 <= 0 || (long long)i0 * i1 >= (1ll << 31) || (long long)i2 * ((long long)i0 * i1) >= (1ll << 31))
        return SG_EINVAL;
      if (!an_plan(i0, i1, i2, a3 != 0, a4 != 0, misaligned == 0, &p)) return SG_EINVAL;
      w[0] = p.form, w[1] = (int)p.gx, w[2] = (int)p.gy, w[3] = (int)p.gz, w[4] = AN_THREADS, w[5] = p.vec, w[6] = p.launches;
      w[7] = p.hspan, w[8] = p.spans, w[9] = p.rparts, w[10] = p.tiles, w[11] = p.pop_trips, w[12] = (int)p.want;
      w[13] = (int)p.most, w[14] = p.parts, w[15] = p.batches, w[16] = p.nb_last, w[17] = p.p2_last, w[18] = p.L, w[19] = p.G;
      w[20] = p.form == 0 ? AN_TILE : 0, w[21] = p.form == 0 ? AN_ROWS : 0;
      break;
    }
    default: return SG_EINVAL;
  }
  for (int i = 0; i < SG_SERVING_PLAN_WORDS; ++i) out[i] = w[i];
  return 0;
}
