// Scenario forecasts: sampled rolling paths and their order statistics (include/stemgnn_hip.h: stemgnn_scenario_roll /
// _roll_given / _bands / _rank).
//
// roll: one round of the roll for Bo origins x S paths.  Path p = b * S + s reads source row p / fan of `inputs` and
// `forecast` (fan == S: round 0, the model ran once per origin; fan == 1: a later round, once per path).  For step j < L and
// node n the draw is the inverse of the piecewise-linear quantile function through (tau_q, v_q), v the column
// forecast[src, :, j, n] in the order of quantile_serve.hip (fp32's with -0 == +0, NaN last, ties in row order), taken at the
// uniform u of a Philox word: see sc_draw.  The draw goes to paths[b, s, step + j, n] and takes the place of the forecast row
// in the window roll of sg_roll_window_kernel (data.hip); round 0 also files the model's own column in bands.
// roll_given: the same kernel template with u read from uniforms[b, s, j, n] (copula.hip makes correlated ones).
//
// A workgroup owns one path; its threads walk the path's (row, node group) items, lanes along n, so every global access of a
// wave is a coalesced run of one row.  The column of a draw item is held in the thread's own LDS words [Q][VEC][threads]
// (Q is a run-time value: a per-thread array indexed at run time would live in scratch memory) -- lane t touches word t of
// every row, conflict-free, and no thread reads another's words: no barrier.  Only the two values that bracket u are needed,
// so nothing is sorted: the ranks are counted as quantile_serve.hip counts them and the values of rank i and i + 1 are kept.
// VEC = 4: four consecutive n per thread, one Philox call, 16-byte accesses (N % 4 == 0, every buffer 16-byte aligned);
// VEC = 1 otherwise: the same call is made by the four threads of a node group, each keeping its word.
//
// bands: row q of bands[b, :, h, n] = the k_q-th smallest of the S values paths[b, :, h, n], h >= step_from, in the same order.
// A workgroup loads a tile of S rows x C columns into LDS (C = 64 .. 8, the tile <= 32 KB), one barrier, then thread (g, c)
// counts, for its rows i = g, g + G, .., how many values of column c come before value i -- rank by counting, the row index
// breaking ties, so the ranks of a column are a permutation and exactly one row answers each k_q.  Lanes of a half-wave read
// word (j, c): distinct c are distinct banks, equal c are one address (a broadcast).  No atomics, no scratch; why counting and
// not a bitonic network or radix passes: DESIGN.md section 5o.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "philox.h"
#include "scenario_draw.h"
#include "sg_host.h"

namespace {

constexpr int SC_THREADS = 256;             // the most; fewer (a multiple of 64) when Q is large: see stemgnn_scenario_roll
constexpr int SC_LDS_BYTES = 32 * 1024;     // per workgroup, either kernel
constexpr int SC_MAX_S = 1024;
constexpr int SC_ROWS = 4;                  // bands: values a thread ranks per walk over its column

struct ScRollArgs {                         // travels by value in the kernel arguments
  const float* inputs;                      // [Bsrc, W, N]
  const float* forecast;                    // [Bsrc, Q, L, N]
  float* inputs_next;                       // [Bo * S, W, N] or NULL
  float* paths;                             // [Bo, S, horizon, N]
  float* bands;                             // [Bo, Q, horizon, N] or NULL
  const float* uniforms;                    // [Bo, S, L, N]: the GIVEN kernels only
  unsigned long long origin0, seed, offset;
  int S, fan, W, L, N, Q, step, horizon, path_coupling, clamp;
  float tau[CF_MAX_Q];
};

struct ScBandArgs {
  const float* paths;                       // [Bo, S, horizon, N]
  float* bands;                             // [Bo, Q, horizon, N]
  int S, Q, HN, from, cols, C, tiles;       // from = step_from * N; cols = HN - from; tiles = ceil(cols / C) per origin
  int rank[CF_MAX_Q];                       // 1-based
};

// The draw at u from the thread's column col[q * stride], q < Q: segment i = the last level <= u within [0, Q - 2],
// wt = (u - tau_i) / (tau_{i+1} - tau_i), y = v_(i) + (v_(i+1) - v_(i)) * wt on the ordered values, every operation rounded
// on its own.  The product and the sum are written as plain operators under `fp contract(off)`: the __fmul_rn / __fadd_rn of
// this toolchain's headers are `x * y` / `x + y` compiled under the default contraction, which fuses them once inlined.
__device__ inline float sc_draw(const ScRollArgs& a, const float* col, int stride, float u) {
#pragma clang fp contract(off)
  const int Q = a.Q;
  int i = 0;
  float t0 = a.tau[0], t1 = a.tau[1];                         // (the levels are read at uniform indices only)
  for (int q = 1; q < Q - 1; ++q) {
    const bool at = a.tau[q] <= u;
    i = at ? q : i;
    t0 = at ? a.tau[q] : t0;
    t1 = at ? a.tau[q + 1] : t1;
  }
  float wt = __fdiv_rn(__fsub_rn(u, t0), __fsub_rn(t1, t0));
  if (a.clamp) wt = fminf(fmaxf(wt, 0.f), 1.f);
  float lo = 0.f, hi = 0.f;
#pragma unroll 1
  for (int q = 0; q < Q; ++q) {
    const float v = col[q * stride];
    int rank = 0;
#pragma clang loop vectorize(disable) unroll_count(4)
    for (int j = 0; j < Q; ++j) {
      const float w = col[j * stride];
      rank += (sc_less(w, v) || (!sc_less(v, w) && j < q)) ? 1 : 0;
    }
    lo = rank == i ? v : lo;
    hi = rank == i + 1 ? v : hi;
  }
  const float d = hi - lo;
  const float m = d * wt;
  return lo + m;
}

// GIVEN: u is read from a.uniforms[b, s, j, n] instead of being made from a Philox word (stemgnn_scenario_roll_given)
template <int VEC, bool GIVEN>
__global__ __launch_bounds__(SC_THREADS) void sc_roll_kernel(const ScRollArgs a) {
  extern __shared__ float4 sc_lds[];
  const int T = blockDim.x, t = threadIdx.x, Q = a.Q, N = a.N, W = a.W, L = a.L;
  const size_t p = blockIdx.x;                                // the path; src = its row of inputs / forecast
  const size_t src = p / (size_t)a.fan;
  const size_t b = p / (size_t)a.S;
  const int s = (int)(p - b * (size_t)a.S);
  const int per = N / VEC;                                    // node groups of a row
  const int take = min(a.horizon - a.step, L);
  const int r0 = a.inputs_next ? 0 : W - L;                   // without a next window only the draw rows are walked
  const int items = (W - r0) * per;
  const int nq = (N + 3) >> 2;                                // Philox calls of a row
  const unsigned long long row0 = ((a.origin0 + b) * (unsigned long long)a.S + (unsigned long long)s) *
                                      (unsigned long long)a.horizon + (unsigned long long)a.step;
  float* col = reinterpret_cast<float*>(sc_lds) + t;          // word (q * VEC + k) * T
  for (int it = t; it < items; it += T) {
    const int rr = it / per, g = it - rr * per;
    const int r = r0 + rr, n = g * VEC;
    if (r < W - L) {                                          // the window moves up by L rows
      float v[VEC];
      cf_load<VEC>(a.inputs + (src * W + r + L) * N + n, v);
      cf_store<VEC>(a.inputs_next + (p * W + r) * N + n, v);
      continue;
    }
    const int j = r - (W - L);
    const float* f = a.forecast + (src * Q * L + j) * N + n;
    for (int q = 0; q < Q; ++q) {
      float v[VEC];
      cf_load<VEC>(f + (size_t)q * L * N, v);
#pragma unroll
      for (int k = 0; k < VEC; ++k) col[(q * VEC + k) * T] = v[k];
      if (a.bands && s == 0 && j < take) cf_store<VEC>(a.bands + ((b * Q + q) * a.horizon + a.step + j) * N + n, v);
    }
    float u[VEC], y[VEC];
    if constexpr (GIVEN) {
      cf_load<VEC>(a.uniforms + ((p * L + j) * N + n), u);
    } else {
      uint32_t w[4];
      sg_philox4(a.seed, a.offset, a.path_coupling ? row0 * nq : (row0 + j) * nq + (n >> 2), w);
#pragma unroll
      for (int k = 0; k < VEC; ++k) u[k] = sc_uniform(a.path_coupling ? w[0] : (VEC == 4 ? w[k] : w[n & 3]));
    }
#pragma unroll
    for (int k = 0; k < VEC; ++k) y[k] = sc_draw(a, col + k * T, VEC * T, u[k]);
    if (j < take) cf_store<VEC>(a.paths + (p * a.horizon + a.step + j) * N + n, y);
    if (a.inputs_next) cf_store<VEC>(a.inputs_next + (p * W + r) * N + n, y);
  }
}

__global__ __launch_bounds__(SC_THREADS) void sc_bands_kernel(const ScBandArgs a) {
  extern __shared__ float4 sc_lds[];
  float* tile = reinterpret_cast<float*>(sc_lds);             // [S][C]
  const int S = a.S, C = a.C, T = blockDim.x, t = threadIdx.x;
  const size_t b = blockIdx.x / (unsigned)a.tiles;
  const int c0 = (int)(blockIdx.x - b * (unsigned)a.tiles) * C;
  const int live = min(C, a.cols - c0);                       // columns of this tile
  const float* src = a.paths + b * S * (size_t)a.HN + a.from + c0;
  for (int e = t; e < S * C; e += T) {
    const int i = e / C, c = e - i * C;
    if (c < live) tile[e] = src[(size_t)i * a.HN + c];
  }
  __syncthreads();
  const int G = T / C, g = t / C, c = t - g * C;
  if (c >= live) return;                                      // (no barrier below)
  float* dst = a.bands + b * a.Q * (size_t)a.HN + a.from + c0 + c;
  for (int i0 = g; i0 < S; i0 += G * SC_ROWS) {
    float v[SC_ROWS];
    int rank[SC_ROWS];
#pragma unroll
    for (int m = 0; m < SC_ROWS; ++m) {
      const int i = i0 + m * G;
      v[m] = tile[(i < S ? i : i0) * C + c];
      rank[m] = 0;
    }
    for (int j = 0; j < S; ++j) {
      const float w = tile[j * C + c];
#pragma unroll
      for (int m = 0; m < SC_ROWS; ++m)
        rank[m] += (sc_less(w, v[m]) || (!sc_less(v[m], w) && j < i0 + m * G)) ? 1 : 0;
    }
#pragma unroll
    for (int m = 0; m < SC_ROWS; ++m) {
      if (i0 + m * G >= S) continue;
      for (int q = 0; q < a.Q; ++q) {
        if (a.rank[q] == rank[m] + 1) dst[(size_t)q * a.HN] = v[m];
      }
    }
  }
}

// the checks and the launch of both roll entries; uniforms == NULL: the Philox draws of `coupling`
template <bool GIVEN>
int sc_roll(const float* inputs, const float* forecast, const float* taus, const float* uniforms, int Bo, int S, int fan, int W,
            int L, int N, int Q, int step, int horizon, long long origin0, unsigned long long seed, unsigned long long offset,
            int coupling, int tails, float* inputs_next, float* paths, float* bands, void* stream) {
  if (!inputs || !forecast || !taus || !paths || inputs == inputs_next || (GIVEN && !uniforms)) return SG_EINVAL;
  if (Bo <= 0 || W <= 0 || N <= 0 || L <= 0 || L > W || step < 0 || step >= horizon) return SG_EINVAL;
  if (Q < 2 || Q > CF_MAX_Q || S < 1 || S > SC_MAX_S || (fan != 1 && fan != S)) return SG_EINVAL;
  if ((coupling != SG_SCENARIO_INDEPENDENT && coupling != SG_SCENARIO_PATH) ||
      (tails != SG_SCENARIO_LINEAR && tails != SG_SCENARIO_CLAMP))
    return SG_EINVAL;
  if (bands && fan != S) return SG_EINVAL;                    // the model's own columns exist in round 0 only
  ScRollArgs a = {};
  for (int q = 0; q < Q; ++q) {
    const float lo = q ? taus[q - 1] : 0.f;
    if (!(taus[q] > lo) || !(taus[q] < 1.f)) return SG_EINVAL;   // strictly increasing inside (0, 1); a NaN fails both
    a.tau[q] = taus[q];
  }
  // what an int carries in the kernel: the path count (grid.x), the items of a path, a column's row stride
  if (!sg_fits_int((long long)Bo * S) || !sg_fits_int((long long)W * N) || !sg_fits_int((long long)Q * L * N) ||
      !sg_fits_int((long long)Q * horizon * N) || !sg_fits_int((long long)S * horizon))
    return SG_EINVAL;
  a.inputs = inputs; a.forecast = forecast; a.inputs_next = inputs_next; a.paths = paths; a.bands = bands;
  a.uniforms = uniforms;
  a.origin0 = (unsigned long long)origin0; a.seed = seed; a.offset = offset;
  a.S = S; a.fan = fan; a.W = W; a.L = L; a.N = N; a.Q = Q; a.step = step; a.horizon = horizon;
  a.path_coupling = coupling == SG_SCENARIO_PATH;
  a.clamp = tails == SG_SCENARIO_CLAMP;
  const bool vec = (N & 3) == 0 && sg_aligned16(inputs) && sg_aligned16(forecast) && sg_aligned16(paths) &&
                   (!inputs_next || sg_aligned16(inputs_next)) && (!bands || sg_aligned16(bands)) &&
                   (!GIVEN || sg_aligned16(uniforms));
  const int VEC = vec ? 4 : 1;
  const long long items = (long long)(inputs_next ? W : L) * (N / VEC);
  int T = SC_THREADS;
  while (T > 64 && ((size_t)T * Q * VEC * 4 > (size_t)SC_LDS_BYTES || T - 64 >= items)) T -= 64;
  const size_t lds = (size_t)T * Q * VEC * 4;                 // <= 32 KB: Q <= 32, VEC <= 4, T >= 64
  const dim3 grid((unsigned)(Bo * S));
  if (vec)
    hipLaunchKernelGGL((sc_roll_kernel<4, GIVEN>), grid, dim3(T), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((sc_roll_kernel<1, GIVEN>), grid, dim3(T), lds, (hipStream_t)stream, a);
  SG_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" long stemgnn_scenario_rank(double tau, long S) {
  if (S < 1) return 0;
  if (!(tau > 0.0)) return 1;
  const double t = tau * (double)S;
  const double k = ceil(t * (1.0 - 1e-12));
  return k < 1.0 ? 1 : (k > (double)S ? S : (long)k);
}

extern "C" int stemgnn_scenario_roll(const float* inputs, const float* forecast, const float* taus, int Bo, int S, int fan, int W,
                                     int L, int N, int Q, int step, int horizon, long long origin0, unsigned long long seed,
                                     unsigned long long offset, int coupling, int tails, float* inputs_next, float* paths,
                                     float* bands, void* stream) {
  return sc_roll<false>(inputs, forecast, taus, nullptr, Bo, S, fan, W, L, N, Q, step, horizon, origin0, seed, offset, coupling,
                        tails, inputs_next, paths, bands, stream);
}

extern "C" int stemgnn_scenario_roll_given(const float* inputs, const float* forecast, const float* taus, const float* uniforms,
                                           int Bo, int S, int fan, int W, int L, int N, int Q, int step, int horizon, int tails,
                                           float* inputs_next, float* paths, float* bands, void* stream) {
  return sc_roll<true>(inputs, forecast, taus, uniforms, Bo, S, fan, W, L, N, Q, step, horizon, 0, 0ull, 0ull,
                       SG_SCENARIO_INDEPENDENT, tails, inputs_next, paths, bands, stream);
}

extern "C" int stemgnn_scenario_bands(const float* paths, int Bo, int S, int horizon, int N, int Q, const int* ranks,
                                      int step_from, float* bands, void* stream) {
  if (!paths || !ranks || !bands || paths == bands) return SG_EINVAL;
  if (Bo <= 0 || horizon <= 0 || N <= 0 || Q < 1 || Q > CF_MAX_Q || S < 1 || S > SC_MAX_S) return SG_EINVAL;
  if (step_from < 0 || step_from > horizon) return SG_EINVAL;
  if (!sg_fits_int((long long)horizon * N) || !sg_fits_int((long long)Bo * S)) return SG_EINVAL;
  ScBandArgs a = {};
  for (int q = 0; q < Q; ++q) {
    if (ranks[q] < 1 || ranks[q] > S) return SG_EINVAL;
    a.rank[q] = ranks[q];
  }
  if (step_from == horizon) return 0;                         // nothing to write
  a.paths = paths; a.bands = bands; a.S = S; a.Q = Q;
  a.HN = horizon * N;
  a.from = step_from * N;
  a.cols = a.HN - a.from;
  int C = 64;                                                 // the widest tile of S rows within the LDS budget, 8 at least
  while (C > 8 && (size_t)S * C * 4 > (size_t)SC_LDS_BYTES) C >>= 1;
  a.C = C;
  a.tiles = sg_ceil_div(a.cols, C);
  if (!sg_fits_int((long long)Bo * a.tiles)) return SG_EINVAL;
  hipLaunchKernelGGL(sc_bands_kernel, dim3((unsigned)(Bo * a.tiles)), dim3(SC_THREADS), (size_t)S * C * 4, (hipStream_t)stream,
                     a);
  SG_TRY(hipGetLastError());
  return 0;
}
