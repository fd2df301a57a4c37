// Scenario reduction by forward selection (Heitsch & Roemisch 2003): pairwise distances of sampled paths and the greedy pick of
// K representatives with redistributed weights (include/stemgnn_hip.h: stemgnn_scenario_distances / stemgnn_scenario_reduce;
// DESIGN.md section 5s).
//
// distances: paths [count, S, L] fp32, a path's trajectory one contiguous run of L floats.  One workgroup per (origin, 32 x 32
//           tile (I, J) of path pairs, I <= J), the energy launch of ensemble.hip with the walk over L instead of over the nodes
//           of one step: L is walked in chunks of 64; the two panels of 32 paths x 64 values (one when I == J) go to LDS as fp64,
//           rows 65 doubles apart (plain coalesced row loads: a wave reads 64 consecutive floats of one path); thread
//           (ti, tj) = (t / 16, t % 16) owns the pairs (2 ti + {0, 1}, 2 tj + {0, 1}) and adds ((x_il - x_jl) * scale_l)^2 into
//           four registers -- DIFFERENCES, never the Gram expansion: two coincident paths give exactly 0.  A half-wave reads two
//           panel-A rows (broadcasts) and sixteen panel-B rows (8-byte reads at banks 4 tj): conflict-free.  The tile is stored
//           where i <= j, and once more, transposed through LDS, where i < j: D[i, j] and D[j, i] are one value's bits, and both
//           stores run along rows of D.
//           A pair's sum is kept as FOUR partial sums, chunk c of L adding into sum c % 4, joined as ((s0 + s1) + s2) + s3: four
//           independent FMA chains per pair in the 256-thread form -- and the split of the wide form, which a call takes when its
//           grid leaves compute units idle (count x tile pairs <= the CUs, e.g. a live query: 3 workgroups at S = 64): 1024
//           threads, wave group g = 0 .. 3 with panels of its own walks the chunks c % 4 = g and owns sum g; the four meet in LDS
//           and group 0 joins them in the same order.  Both forms give the same bits, so batching does not show in the result.
// reduce:   one workgroup per origin, thread u owns candidate u.  D [S, S] is checked (every entry finite and >= 0) while it goes
//           to LDS, rows S | 1 doubles apart, where that fits the 160 KiB of a gfx950 workgroup (S <= 141); beyond, row k is read
//           from memory, contiguous in u.  Per pick: z_u = sum_k min(m_k, D[k, u]) with k = 0, 1, .. in order, one fp64 add after
//           the other (the order is the definition); an argmin over (taken, z, u) -- a wave reduction on pairs, the waves in index
//           order -- that returns the lowest index among equal values; then m_k = min(m_k, D[k, u*]) and, where that lowered
//           m_k strictly, near_k = the pick's position (ties stay with the earlier pick).  counts: thread j counts near == j.
// No floating-point atomics, no allocation, no host synchronisation: the same bits on every run, origin by origin, however the
// origins are batched into calls.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "devattr.h"
#include "sg_host.h"

namespace {

constexpr int RD_THREADS = 256;
constexpr int RD_MAX_S = 1024;
constexpr int RD_PT = 32;                   // distances: paths per panel
constexpr int RD_LC = 64;                   // distances: trajectory values per chunk
constexpr int RD_LD = RD_LC + 1;            // distances: doubles between panel rows
constexpr int RD_TLD = RD_PT + 1;           // distances: doubles between rows of the transposed tile
constexpr int RD_NQ = 4;                    // distances: partial sums per pair, chunk c adding into sum c % 4
constexpr int RD_GROUP_DOUBLES = 2 * RD_PT * RD_LD + RD_LC;   // distances: LDS of one wave group
constexpr size_t RD_LDS_BYTES = 160 * 1024; // reduce: LDS of one workgroup on gfx950

struct RdDistArgs {
  const float* paths;                       // [count, S, L]
  const double* scale;                      // [L] or NULL
  double* D;                                // [count, S, S]
  int S, L, nt, pairs, squared;
};

// NG wave groups of 256 threads: 1, or RD_NQ (one per partial sum)
template <bool SCALED, int NG>
__global__ __launch_bounds__(RD_THREADS * NG) void rd_distance_kernel(const RdDistArgs a) {
  extern __shared__ __align__(16) double rd_dist_lds[];         // per wave group: panel A, panel B, the scale's chunk
  constexpr int NQ = RD_NQ / NG;                                // partial sums a thread keeps
  const int t = threadIdx.x & (RD_THREADS - 1), g = threadIdx.x / RD_THREADS, S = a.S, L = a.L;
  double* pa = rd_dist_lds + (size_t)g * RD_GROUP_DOUBLES;
  double* pb_own = pa + RD_PT * RD_LD;
  double* sc = pb_own + RD_PT * RD_LD;
  const size_t c = blockIdx.x / (unsigned)a.pairs;
  int rem = (int)(blockIdx.x - c * (unsigned)a.pairs), I = 0;
  while (rem >= a.nt - I) {
    rem -= a.nt - I;
    ++I;
  }
  const int J = I + rem;
  const bool diag = I == J;
  const double* pb = diag ? pa : pb_own;
  const float* px = a.paths + c * (size_t)S * L;                // path s: + s * L
  const int ln = t & (RD_LC - 1), lr = t >> 6;                  // the loader's column and first row
  const int ti = t >> 4, tj = t & 15;
  double acc[NQ][2][2];
#pragma unroll
  for (int q = 0; q < NQ; ++q) acc[q][0][0] = acc[q][0][1] = acc[q][1][0] = acc[q][1][1] = 0.0;
  const int chunks = (L + RD_LC - 1) / RD_LC;
  for (int c0 = 0; c0 < chunks; c0 += RD_NQ) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      // chunk c0 + q adds into sum q; the wide form: this group's sum is g.  Past the end (the same for a whole group; the
      // 256-thread form stops there, the groups of the wide one keep the barriers in step) nothing is live and nothing is added
      const long long l0 = (long long)(c0 + (NG == 1 ? q : g)) * RD_LC;
      if (NG == 1 && l0 >= L) break;
      const long long l = l0 + ln;
      const bool live = l < L;
      __syncthreads();                                          // the previous chunk has been read
      for (int r = lr; r < RD_PT; r += RD_THREADS / RD_LC) {
        const int si = I * RD_PT + r, sj = J * RD_PT + r;
        pa[r * RD_LD + ln] = (live && si < S) ? (double)px[(size_t)si * L + l] : 0.0;
        if (!diag) pb_own[r * RD_LD + ln] = (live && sj < S) ? (double)px[(size_t)sj * L + l] : 0.0;
      }
      if (SCALED && t < RD_LC) sc[t] = live ? a.scale[l] : 0.0;
      __syncthreads();
      const int lim = (int)min((long long)RD_LC, L - l0);       // (<= 0 past the end)
      const double* ra = pa + (2 * ti) * RD_LD;
      const double* rb = pb + (2 * tj) * RD_LD;
      for (int k = 0; k < lim; ++k) {
        const double a0 = ra[k], a1 = ra[RD_LD + k], b0 = rb[k], b1 = rb[RD_LD + k];
        const double w = SCALED ? sc[k] : 1.0;
        double d;
        d = a0 - b0; if (SCALED) d = __dmul_rn(d, w); acc[q][0][0] = fma(d, d, acc[q][0][0]);
        d = a0 - b1; if (SCALED) d = __dmul_rn(d, w); acc[q][0][1] = fma(d, d, acc[q][0][1]);
        d = a1 - b0; if (SCALED) d = __dmul_rn(d, w); acc[q][1][0] = fma(d, d, acc[q][1][0]);
        d = a1 - b1; if (SCALED) d = __dmul_rn(d, w); acc[q][1][1] = fma(d, d, acc[q][1][1]);
      }
    }
  }
  __syncthreads();                                              // the panels are read
  double sum[2][2];
  if (NG == 1) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        double s = acc[0][u][v];
#pragma unroll
        for (int q = 1; q < NQ; ++q) s += acc[q][u][v];         // ((s0 + s1) + s2) + s3
        sum[u][v] = s;
      }
  } else {                                                      // the groups' sums meet in their panel A, slot (pair, t)
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) pa[(2 * u + v) * RD_THREADS + t] = acc[0][u][v];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const double* slot = rd_dist_lds + (2 * u + v) * RD_THREADS + t;
        double s = slot[0];
#pragma unroll
        for (int q = 1; q < RD_NQ; ++q) s += slot[(size_t)q * RD_GROUP_DOUBLES];
        sum[u][v] = s;
      }
  }
  // group 0 stores; its panel B becomes the transposed tile (panel A may still be read by the join above)
  double* Dc = a.D + c * (size_t)S * S;
  if (g == 0) {
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        const int ri = 2 * ti + u, rj = 2 * tj + v;
        const int si = I * RD_PT + ri, sj = J * RD_PT + rj;
        const double d = a.squared ? sum[u][v] : sqrt(sum[u][v]);
        pb_own[rj * RD_TLD + ri] = d;
        if (si <= sj && sj < S) Dc[(size_t)si * S + sj] = d;    // (si <= sj < S)
      }
  }
  __syncthreads();
  if (g == 0) {
    const int rj = t >> 3, q0 = (t & 7) * 4;                    // row rj of the transposed tile, four of its columns
    const int sj = J * RD_PT + rj;
    if (sj < S) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int si = I * RD_PT + q0 + q;
        if (si < sj) Dc[(size_t)sj * S + si] = pb_own[rj * RD_TLD + q0 + q];
      }
    }
  }
}

struct RdPickArgs {
  const double* D;                          // [count, S, S]
  int* selected;                            // [count, K]
  int* counts;                              // [count, K]
  int* assign;                              // [count, S]
  double* cost;                             // [count, K]
  int S, K, ld;                             // ld: doubles between rows of the LDS copy
};

// the smaller of two (taken, value, index) candidates: an untaken one first, then the smaller value, then the lower index
__device__ inline void rd_take_min(double& v, int& i, double ov, int oi) {
  const bool ours_taken = i >= RD_MAX_S, theirs_taken = oi >= RD_MAX_S;
  const bool better = ours_taken != theirs_taken ? ours_taken : (ov < v || (ov == v && oi < i));
  if (better) {
    v = ov;
    i = oi;
  }
}

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void rd_pick_kernel(const RdPickArgs a) {
  extern __shared__ double rd_lds[];
  const int S = a.S, K = a.K, t = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
  double* m = rd_lds;                                           // [S]
  double* wv = m + S;                                           // [16]: the waves' candidates
  int* wi = reinterpret_cast<int*>(wv + 16);                    // [16]
  int* near = wi + 16;                                          // [S]
  int* pick = near + S;                                         // [2]: the pick, and (once) the verdict on D
  double* Dl = reinterpret_cast<double*>(near + ((S + 2 + 1) & ~1));   // [S][ld], IN_LDS only
  const size_t c = blockIdx.x;
  const double* Dg = a.D + c * (size_t)S * S;
  const int ld = IN_LDS ? a.ld : S;
  const double* Dr = IN_LDS ? Dl : Dg;                          // what the picks read
  int bad = 0;
  for (int i = t; i < S * S; i += nthr) {
    const double d = Dg[i];
    bad |= (d >= 0.0 && d < INFINITY) ? 0 : 1;                  // a NaN fails both comparisons
    if (IN_LDS) {
      const int k = i / S;
      Dl[k * ld + (i - k * S)] = d;
    }
  }
  for (int k = t; k < S; k += nthr) {
    m[k] = INFINITY;
    near[k] = -1;
  }
  if (__syncthreads_or(bad)) {                                  // refused: this origin alone
    for (int j = t; j < K; j += nthr) {
      a.selected[c * K + j] = -1;
      a.counts[c * K + j] = 0;
      a.cost[c * K + j] = NAN;
    }
    for (int k = t; k < S; k += nthr) a.assign[c * S + k] = -1;
    return;
  }
  bool taken = t >= S;
  for (int p = 0; p < K; ++p) {
    double z = 0.0;
    if (t < S) {
      const double* col = Dr + t;
      for (int k = 0; k < S; ++k) z += fmin(m[k], col[(size_t)k * ld]);
    }
    double v = z;
    int idx = taken ? RD_MAX_S + t : t;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ov = __shfl_down(v, off);
      const int oi = __shfl_down(idx, off);
      rd_take_min(v, idx, ov, oi);
    }
    if ((t & 63) == 0) {
      wv[t >> 6] = v;
      wi[t >> 6] = idx;
    }
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < nw; ++w) rd_take_min(v, idx, wv[w], wi[w]);
      pick[0] = idx;
      a.selected[c * K + p] = idx;
      a.cost[c * K + p] = v / (double)S;
    }
    __syncthreads();
    const int sel = pick[0];
    taken = taken || t == sel;
    for (int k = t; k < S; k += nthr) {
      const double d = Dr[(size_t)k * ld + sel];
      if (d < m[k]) {
        m[k] = d;
        near[k] = p;
      }
    }
    __syncthreads();                                            // m, near and pick are settled for the next pick
  }
  for (int k = t; k < S; k += nthr) a.assign[c * S + k] = near[k];
  for (int j = t; j < K; j += nthr) {
    int n = 0;
    for (int k = 0; k < S; ++k) n += near[k] == j ? 1 : 0;
    a.counts[c * K + j] = n;
  }
}

bool rd_fits_int(long long v) { return v > 0 && v < (1ll << 31); }

size_t rd_pick_lds(int S, int ld, bool in_lds) {
  // m [S] and the waves' 16 values as doubles; 16 + S + 2 ints, rounded to a double; the copy of D
  return ((size_t)S + 16) * 8 + (size_t)((16 + S + 2 + 1) & ~1) * 4 + (in_lds ? (size_t)S * ld * 8 : 0);
}

SgDynLds rd_pick_guard, rd_wide_guard[2];

}  // namespace

extern "C" int stemgnn_scenario_distances(const float* paths, const double* scale, long count, int S, int L, int squared,
                                          double* D, void* stream) {
  if (!paths || !D) return SG_EINVAL;
  if (count <= 0 || S <= 0 || L <= 0 || S > RD_MAX_S || (squared != 0 && squared != 1)) return SG_EINVAL;
  if (!rd_fits_int(count) || !rd_fits_int((long long)S * L) || !rd_fits_int((long long)count * S * S)) return SG_EINVAL;
  RdDistArgs a = {};
  a.paths = paths; a.scale = scale; a.D = D; a.S = S; a.L = L; a.squared = squared;
  a.nt = sg_ceil_div(S, RD_PT);
  a.pairs = a.nt * (a.nt + 1) / 2;
  if (!rd_fits_int((long long)count * a.pairs)) return SG_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  // the wide form where the grid leaves compute units idle and L has chunks to share out; the same bits either way
  const bool wide = (long long)count * a.pairs <= sg_num_cus() && L > RD_LC;
  const dim3 grid((unsigned)(count * a.pairs));
  const size_t lds = (size_t)RD_GROUP_DOUBLES * 8;
  if (wide) {
    if (scale) {
      SG_TRY(sg_ensure_dyn_lds((const void*)rd_distance_kernel<true, RD_NQ>, RD_NQ * lds, rd_wide_guard[1]));
      hipLaunchKernelGGL((rd_distance_kernel<true, RD_NQ>), grid, dim3(RD_THREADS * RD_NQ), RD_NQ * lds, st, a);
    } else {
      SG_TRY(sg_ensure_dyn_lds((const void*)rd_distance_kernel<false, RD_NQ>, RD_NQ * lds, rd_wide_guard[0]));
      hipLaunchKernelGGL((rd_distance_kernel<false, RD_NQ>), grid, dim3(RD_THREADS * RD_NQ), RD_NQ * lds, st, a);
    }
  } else if (scale) {
    hipLaunchKernelGGL((rd_distance_kernel<true, 1>), grid, dim3(RD_THREADS), lds, st, a);
  } else {
    hipLaunchKernelGGL((rd_distance_kernel<false, 1>), grid, dim3(RD_THREADS), lds, st, a);
  }
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_scenario_reduce(const double* D, long count, int S, int K, int* selected, int* counts, int* assign,
                                       double* cost, void* stream) {
  if (!D || !selected || !counts || !assign || !cost) return SG_EINVAL;
  if (count <= 0 || S <= 0 || S > RD_MAX_S || K < 1 || K > S) return SG_EINVAL;
  if (!rd_fits_int(count) || !rd_fits_int((long long)count * S * S)) return SG_EINVAL;
  RdPickArgs a = {};
  a.D = D; a.selected = selected; a.counts = counts; a.assign = assign; a.cost = cost; a.S = S; a.K = K;
  a.ld = S | 1;                             // an odd number of doubles: a column read meets every bank pair once
  const bool in_lds = rd_pick_lds(S, a.ld, true) <= RD_LDS_BYTES;
  const size_t lds = rd_pick_lds(S, a.ld, in_lds);
  int threads = (S + 63) & ~63;             // a thread per candidate; at least four waves to bring D in
  if (threads < RD_THREADS) threads = RD_THREADS;
  hipStream_t st = (hipStream_t)stream;
  if (in_lds) {
    SG_TRY(sg_ensure_dyn_lds((const void*)rd_pick_kernel<true>, lds, rd_pick_guard));
    hipLaunchKernelGGL(rd_pick_kernel<true>, dim3((unsigned)count), dim3(threads), lds, st, a);
  } else {
    hipLaunchKernelGGL(rd_pick_kernel<false>, dim3((unsigned)count), dim3(threads), lds, st, a);
  }
  SG_TRY(hipGetLastError());
  return 0;
}
