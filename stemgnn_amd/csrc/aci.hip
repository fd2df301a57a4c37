// Adaptive conformal inference for live forecasts (include/stemgnn_hip.h: stemgnn_aci_update).
//
// One call takes ONE matured forecast (one origin), for all P pairs and all groups, in one launch: the origin's scores go into
// slot `slot` of the rolling window scores [M, P, H, N]; every group counts its valid and its missed targets, moves its working
// level alpha by gamma * (target_alpha - miss / valid), and takes the (1 - alpha) quantile of the window's valid scores as its
// new offset -- the exact MSB-first radix select of conformal.hip (its key, rank formula and wave pick: conformal_select.h), but with
// all four 8-bit passes inside the launch: a (pair, group) belongs to ONE workgroup, its histograms live in LDS, and the phases
// are separated by __syncthreads().  No grid-wide synchronisation, no scratch, no floating-point atomics: the only atomics are
// integer adds in LDS, so the result is the same bits on every run.
//
// Two forms, chosen by the grouping (the two of conformal.hip, for the same reasons; their geometry: cf_grouping, conformal_args.h):
//   * columns (per_node): a group's scores are strided by N (or H * N).  The window is a matrix [R, C] whose column is the
//     group (R = M, C = H * N with per_step; R = M * H, C = N without); a workgroup owns 32 adjacent columns and ALL rows,
//     consecutive lanes on consecutive columns, one 256-bin histogram per column in LDS ([bin][column], pitch 33).
//   * stream (pooled over the nodes): a group is M runs of L contiguous floats (L = N with per_step, H * N without); one
//     workgroup per (pair, group), 16 interleaved copies of the histogram ([bin][copy], copy = lane & 15), 16-byte loads when
//     the host found N % 4 == 0 and every buffer 16-byte aligned.  A window of at most 16 loads per thread is read once and
//     kept in registers over the four passes (measured: a third off the launch at 58368 scores per group).
// Both run 1024 threads: the launch is latency-bound (a few dependent passes over a window that sits in L2), so the lever
// is loads in flight per workgroup, not occupancy.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "serving_plan.h"
#include "sg_host.h"

namespace {

// (ACI_THREADS, ACI_WAVES, ACI_TILE = the columns per workgroup of the column form, ACI_KEEP = the loads of the window a thread
// keeps in registers over the passes of the stream form: serving_plan.h, with the launch geometry)
constexpr int ACI_PITCH = ACI_TILE + 1;       // LDS row pitch in words
constexpr int ACI_SEGS = ACI_THREADS / ACI_TILE;   // 32 segments of 8 bins per column in the pick
constexpr int ACI_COPIES = 16;                // histogram copies (stream form)

struct AciPairs {                             // travels by value in the kernel arguments
  int lo[CF_MAX_P], hi[CF_MAX_P];
  double target_alpha[CF_MAX_P];
};

struct AciState {
  float* scores;
  double* alpha;
  float* offsets;
  long long *counts, *miss_sum, *valid_sum;
};

// (the key of a stored score: cf_score_key of conformal_select.h; NaN = absent is skipped by the caller)

// one element of the new origin: its score slot's value, and whether it is valid / missed
__device__ inline float aci_score(float y, float rlo, float rhi, float ilo, float ihi, int& valid, int& miss) {
  if (y != y) return __uint_as_float(CF_NAN_BITS);
  ++valid;
  miss += !(ilo <= y && y <= ihi);
  return cf_unkey(cf_key(rlo, y, rhi));
}

// steps 2-4 of a group, by ONE thread, once m is known: totals, level, and the rank still to be selected (0: the group is
// finished -- nothing moves, or the offset is one of the two infinite branches).
__device__ inline uint32_t aci_level(long long m, int miss, int valid, double target_alpha, double gamma, long long min_scores,
                                     size_t pg, const AciState& st) {
  st.counts[pg] = m;
  st.miss_sum[pg] += miss;
  st.valid_sum[pg] += valid;
  if (valid == 0 || m < min_scores) return 0u;
  // four individually rounded IEEE operations.  The __d*_rn intrinsics are plain operators in this toolchain and carry the
  // translation unit's contraction mode, under which gamma * (..) and the add would fuse into one FMA; the pragma (honoured by
  // hipcc's default -ffp-contract=fast-honor-pragmas) is what keeps the product rounded, so numpy reproduces alpha bit for bit.
  double a, c;
  {
#pragma clang fp contract(off)
    const double err = (double)miss / (double)valid;
    const double dev = target_alpha - err;
    const double move = gamma * dev;
    a = st.alpha[pg] + move;
    c = 1.0 - a;
  }
  st.alpha[pg] = a;
  if (!(c > 0.0)) {                                 // the level left [0, 1] upwards: the empty band
    st.offsets[pg] = __uint_as_float(CF_NINF_BITS);
    return 0u;
  }
  const double kk = cf_rank(m, c);
  if (kk > (double)m) {                             // too few scores for the level (or alpha < 0): the whole line
    st.offsets[pg] = __uint_as_float(CF_PINF_BITS);
    return 0u;
  }
  return (uint32_t)kk;
}

// ---- column form ------------------------------------------------------------------------------------------------------
// grid (column tiles, P).  Cc = columns of the matrix, Hr = its rows per window slot (1 or H); element (r, c) of the window
// is scores[((r / Hr) * P + p) * HN + (r % Hr) * Cc + c]; (r % Hr) * Cc + c is the element's h * N + n.
__global__ __launch_bounds__(ACI_THREADS) void aci_columns(const float* __restrict__ issued, const float* __restrict__ raw,
                                                           const float* __restrict__ ring_y, int C, long long origin, int H,
                                                           int N, int P, AciPairs pairs, double gamma, int M, int slot,
                                                           long long min_scores, int Cc, int Hr, AciState st) {
  __shared__ uint32_t h[256 * ACI_PITCH];
  __shared__ uint32_t part[ACI_SEGS * ACI_PITCH];
  __shared__ int s_valid[ACI_TILE], s_miss[ACI_TILE];
  __shared__ uint32_t s_pre[ACI_TILE], s_k[ACI_TILE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.y;
  const int HN = H * N;
  const int c0 = blockIdx.x * ACI_TILE;
  const int Wd = min(ACI_TILE, Cc - c0);          // columns of this tile
  const int rpw = 64 / Wd;                        // rows one wave covers per iteration (>= 2)
  const int lr = lane / Wd, lc = lane - lr * Wd;
  const bool rows_lane = lr < rpw;
  const int step = ACI_WAVES * rpw;
  for (int i = tid; i < 256 * ACI_PITCH; i += ACI_THREADS) h[i] = 0u;
  if (tid < ACI_TILE) s_valid[tid] = s_miss[tid] = 0, s_pre[tid] = 0u, s_k[tid] = 0u;
  __syncthreads();
  // 1, 2: the origin's scores into the window, valid / miss per column
  if (rows_lane) {
    const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
    int valid = 0, miss = 0;
    for (int r = wave * rpw + lr; r < Hr; r += step) {
      const int e = r * Cc + c0 + lc, hh = e / N, n = e - hh * N;
      const float y = ring_y[(size_t)((origin + hh) % C) * N + n];
      const float s = aci_score(y, raw[lo_off + e], raw[hi_off + e], issued[lo_off + e], issued[hi_off + e], valid, miss);
      st.scores[((size_t)slot * P + p) * HN + e] = s;
    }
    if (valid) atomicAdd(&s_valid[lc], valid);
    if (miss) atomicAdd(&s_miss[lc], miss);
  }
  __syncthreads();                                // the new scores are visible to the whole workgroup from here on
  const uint32_t R = (uint32_t)M * Hr;            // (columns are the groups: [P, Hg, Ng] flattened is [P, Cc])
  for (int d = 0; d < 4; ++d) {
    // 3, 4: one histogram pass over all rows of the tile's columns
    if (rows_lane && (d == 0 || s_k[lc] != 0u)) {
      const uint32_t pre = s_pre[lc];
#pragma unroll 4
      for (uint32_t r = wave * rpw + lr; r < R; r += step) {       // R < 2^31: the unsigned counter cannot wrap
        const uint32_t i = r / Hr;
        const float s = st.scores[((size_t)i * P + p) * HN + (size_t)(r - i * Hr) * Cc + c0 + lc];
        if (s != s) continue;
        const uint32_t key = cf_score_key(s);
        if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * ACI_PITCH + lc], 1u);
      }
    }
    __syncthreads();
    {                                             // 32 segments of 8 bins per column
      const int col = tid & (ACI_TILE - 1), seg = tid >> 5;
      uint32_t v = 0u;
      if (col < Wd) {
#pragma unroll
        for (int b = 0; b < 8; ++b) v += h[(seg * 8 + b) * ACI_PITCH + col];
      }
      part[seg * ACI_PITCH + col] = v;
    }
    __syncthreads();
    if (tid < Wd) {                               // one thread per column: level (pass 0), then the walk to the rank's bin
      const int col = tid;
      const size_t g = (size_t)p * Cc + c0 + col;
      uint32_t k;
      if (d == 0) {
        uint32_t m = 0u;
        for (int sg = 0; sg < ACI_SEGS; ++sg) m += part[sg * ACI_PITCH + col];
        k = aci_level((long long)m, s_miss[col], s_valid[col], pairs.target_alpha[p], gamma, min_scores, g, st);
      } else {
        k = s_k[col];
      }
      if (k != 0u) {
        uint32_t before = 0u;
        int sg = 0;
        while (sg < ACI_SEGS - 1 && before + part[sg * ACI_PITCH + col] < k) before += part[sg++ * ACI_PITCH + col];
        int bin = sg * 8;
        while (bin < sg * 8 + 7 && before + h[bin * ACI_PITCH + col] < k) before += h[bin++ * ACI_PITCH + col];
        const uint32_t pre = s_pre[col] | ((uint32_t)bin << (24 - 8 * d));
        if (d == 3) st.offsets[g] = cf_unkey(pre);
        s_pre[col] = pre;
        k -= before;
      }
      s_k[col] = k;
    }
    __syncthreads();
    if (d < 3) {
      for (int i = tid; i < 256 * ACI_PITCH; i += ACI_THREADS) h[i] = 0u;
      __syncthreads();
    }
  }
}

// ---- stream form ------------------------------------------------------------------------------------------------------
// grid (G, P).  Group g = the L contiguous floats at offset g * L of every [H * N] slab.  VEC = 4: L % 4 == 0, N % 4 == 0 and
// every buffer 16-byte aligned, so a float4 never leaves a row of N.
template <int VEC>
__global__ __launch_bounds__(ACI_THREADS) void aci_stream(const float* __restrict__ issued, const float* __restrict__ raw,
                                                          const float* __restrict__ ring_y, int C, long long origin, int H,
                                                          int N, int P, AciPairs pairs, double gamma, int M, int slot,
                                                          long long min_scores, int L, AciState st) {
  __shared__ uint32_t h[256 * ACI_COPIES];
  __shared__ __attribute__((aligned(16))) uint32_t binsum[256];
  __shared__ int s_valid, s_miss;
  __shared__ uint32_t s_pre, s_k;
  const int tid = threadIdx.x, g = blockIdx.x, p = blockIdx.y, G = gridDim.x;
  const int HN = H * N, base = g * L;
  const size_t pg = (size_t)p * G + g;
  for (int i = tid; i < 256 * ACI_COPIES; i += ACI_THREADS) h[i] = 0u;
  if (tid == 0) s_valid = s_miss = 0, s_pre = 0u, s_k = 0u;
  __syncthreads();
  {  // 1, 2
    const size_t lo_off = (size_t)pairs.lo[p] * HN + base, hi_off = (size_t)pairs.hi[p] * HN + base;
    float* dst = st.scores + ((size_t)slot * P + p) * HN + base;
    int valid = 0, miss = 0;
    for (int t = tid * VEC; t < L; t += ACI_THREADS * VEC) {
      const int e = base + t, hh = e / N, n = e - hh * N;
      float y[VEC], rlo[VEC], rhi[VEC], ilo[VEC], ihi[VEC], s[VEC];
      cf_load<VEC>(ring_y + (size_t)((origin + hh) % C) * N + n, y);
      cf_load<VEC>(raw + lo_off + t, rlo);
      cf_load<VEC>(raw + hi_off + t, rhi);
      cf_load<VEC>(issued + lo_off + t, ilo);
      cf_load<VEC>(issued + hi_off + t, ihi);
#pragma unroll
      for (int j = 0; j < VEC; ++j) s[j] = aci_score(y[j], rlo[j], rhi[j], ilo[j], ihi[j], valid, miss);
      cf_store<VEC>(dst + t, s);
    }
    if (valid) atomicAdd(&s_valid, valid);
    if (miss) atomicAdd(&s_miss, miss);
  }
  __syncthreads();                                // the new scores are visible to the whole workgroup from here on
  const uint32_t total = (uint32_t)M * L;         // < 2^31: the unsigned counter below cannot wrap
  const int copy = tid & (ACI_COPIES - 1);
  const float* win = st.scores + (size_t)p * HN + base;
  const size_t pitch = (size_t)P * HN;            // from one window slot to the next
  // A window of at most ACI_KEEP loads per thread is read ONCE and kept in registers over the four passes (every index below is
  // a compile-time constant after unrolling); a larger one is streamed from L2 again in every pass.  Uniform over the workgroup.
  const bool keep = total <= (uint32_t)(ACI_KEEP * ACI_THREADS * VEC);
  float kept[ACI_KEEP][VEC];
  if (keep) {
#pragma unroll
    for (int q = 0; q < ACI_KEEP; ++q) {
      const uint32_t e = (uint32_t)(tid + q * ACI_THREADS) * VEC;
      if (e < total) {
        const uint32_t i = e / L, t = e - i * L;
        cf_load<VEC>(win + (size_t)i * pitch + t, kept[q]);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j) kept[q][j] = __uint_as_float(CF_NAN_BITS);
      }
    }
  }
  for (int d = 0; d < 4; ++d) {
    const uint32_t pre = s_pre;
    if (keep) {
#pragma unroll
      for (int q = 0; q < ACI_KEEP; ++q) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          const float sc = kept[q][j];
          if (sc != sc) continue;
          const uint32_t key = cf_score_key(sc);
          if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * ACI_COPIES + copy], 1u);
        }
      }
    } else {
#pragma unroll 4
      for (uint32_t e = tid * VEC; e < total; e += ACI_THREADS * VEC) {
        const uint32_t i = e / L, t = e - i * L;
        float s[VEC];
        cf_load<VEC>(win + (size_t)i * pitch + t, s);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
          if (s[j] != s[j]) continue;
          const uint32_t key = cf_score_key(s[j]);
          if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * ACI_COPIES + copy], 1u);
        }
      }
    }
    __syncthreads();
    if (tid < 256) {
      uint32_t v = 0u;
#pragma unroll
      for (int c = 0; c < ACI_COPIES; ++c) {
        const int at = tid * ACI_COPIES + ((c + tid) & (ACI_COPIES - 1));
        v += h[at];
        h[at] = 0u;                               // every pass leaves the copies zero
      }
      binsum[tid] = v;
    }
    __syncthreads();
    if (tid < 64) {                               // wave 0: lane l owns bins 4l .. 4l+3 (the pick of conformal_select.h)
      const uint4 c = reinterpret_cast<const uint4*>(binsum)[tid];
      const uint32_t incl = cf_wave_scan(c, tid);
      uint32_t k = 0u;
      if (d == 0) {
        const long long m = (long long)__shfl(incl, 63, 64);
        if (tid == 0) k = aci_level(m, s_miss, s_valid, pairs.target_alpha[p], gamma, min_scores, pg, st);
        k = __shfl(k, 0, 64);
      } else {
        k = s_k;
      }
      uint32_t bin, before;
      const int at = k != 0u ? cf_wave_pick(c, incl, k, tid, bin, before) : -1;
      if (at < 0) {
        if (tid == 0) s_k = 0u;
      } else if (tid == at) {
        const uint32_t np = pre | (bin << (24 - 8 * d));
        if (d == 3) st.offsets[pg] = cf_unkey(np);
        s_pre = np;
        s_k = k - before;
      }
    }
    __syncthreads();
    if (s_k == 0u) break;                         // uniform: read after the barrier, written before it
  }
}

}  // namespace

extern "C" int stemgnn_aci_update(const float* issued, const float* raw, const float* ring_y, int C, long long origin, int Q,
                                  int H, int N, int P, const int* lo_rows, const int* hi_rows, const double* target_alpha,
                                  double gamma, int M, int slot, long long min_scores, int per_step, int per_node,
                                  float* scores, double* alpha, float* offsets, long long* counts, long long* miss_sum,
                                  long long* valid_sum, void* stream) {
  if (!issued || !raw || !ring_y || !lo_rows || !hi_rows || !target_alpha || !scores || !alpha || !offsets || !counts ||
      !miss_sum || !valid_sum)
    return SG_EINVAL;
  if (M <= 0 || C <= 0 || !cf_shapes_ok(M, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, nullptr)) return SG_EINVAL;
  if (!(gamma >= 0.0) || slot < 0 || slot >= M || origin < 0 || H > C || min_scores < 0) return SG_EINVAL;   // NaN fails >=
  if ((long long)C * N >= (1ll << 31)) return SG_EINVAL;
  AciPairs pairs = {};
  for (int p = 0; p < P; ++p) {
    if (!(target_alpha[p] > 0.0 && target_alpha[p] < 1.0)) return SG_EINVAL;
    pairs.lo[p] = lo_rows[p];
    pairs.hi[p] = hi_rows[p];
    pairs.target_alpha[p] = target_alpha[p];
  }
  const AciState st = {scores, alpha, offsets, counts, miss_sum, valid_sum};
  hipStream_t s = (hipStream_t)stream;
  AciPlan pl;
  aci_plan(H, N, P, M, per_step, per_node, sg_aligned16(issued) && sg_aligned16(raw) && sg_aligned16(ring_y) && sg_aligned16(scores),
           &pl);
  const CfGrouping gr = pl.gr;
  const dim3 grid(pl.gx, pl.gy);
  if (pl.form == 0) {
    hipLaunchKernelGGL(aci_columns, grid, dim3(ACI_THREADS), 0, s, issued, raw, ring_y, C, origin, H, N, P, pairs, gamma, M,
                       slot, min_scores, gr.Cc, gr.Hr, st);
  } else {
    if (pl.vec == 4)
      hipLaunchKernelGGL(aci_stream<4>, grid, dim3(ACI_THREADS), 0, s, issued, raw, ring_y, C, origin, H, N, P, pairs, gamma,
                         M, slot, min_scores, gr.L, st);
    else
      hipLaunchKernelGGL(aci_stream<1>, grid, dim3(ACI_THREADS), 0, s, issued, raw, ring_y, C, origin, H, N, P, pairs, gamma,
                         M, slot, min_scores, gr.L, st);
  }
  SG_TRY(hipGetLastError());
  return 0;
}
