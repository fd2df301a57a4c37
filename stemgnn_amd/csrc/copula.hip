// Gaussian-copula coupling of scenario paths (include/stemgnn_hip.h: stemgnn_copula_pit / _gram / _uniforms; DESIGN.md
// section 5q).  The marginals stay the model's; the uniforms that drive the draws of one (path, step) row are correlated.
//
// pit:      u = F(y), F the piecewise-linear quantile function through (tau_q, v_(q)) that scenario.hip's sc_draw inverts: the
//           same order of the column (scenario_draw.h), the same separately rounded operations.  One thread per (row, node group);
//           the column lives in the thread's own LDS words [Q][VEC][threads] as in sc_roll_kernel, nothing is sorted: the count
//           of values <= y names the segment and the two values of rank i and i + 1 are found by counting.
// gram:     z = normcdfinv((double)u) on load, then for every pair (i, j) the count of rows where both are present and the sums
//           of z_i z_j, z_i and z_i^2 over those rows.  A workgroup owns a 16 x 16 tile of pairs and one chunk of CP_CHUNK rows,
//           walked in stages of 64 rows through two LDS panels; thread (ti, tj) adds its pair's rows in row order.  The finish
//           kernel adds the chunks in chunk order: fixed-order two-level fp64 sums as in ensemble.hip, no atomics.
// uniforms: e = normcdfinvf(uniform of the Philox word `coupling = independent` takes for that draw), z_n = sum_{k <= n}
//           L[n][k] e_k, u_n = normcdff(z_n).  A workgroup owns RT rows with their e in LDS as [k][RT] (one 16-byte read hands a
//           thread e_k of four rows); threads run along n with the rows' sums in registers and read row k of factor_t as a
//           coalesced run (eight rows requested ahead), k ascending from 0: the order of a sum depends on n alone.  Entries
//           with k > n are never used (a select after the load, not a product with 0).
// uniforms_steps: the same kernel body with the steps of a path coupled too.  A tile then holds whole
//           paths, floor(RT / Lsteps) of them, and between the fill and the node sum one thread per (k, path) replaces the path's
//           Lsteps words of LDS row k by A times them, in place.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "philox.h"
#include "scenario_draw.h"
#include "sg_host.h"

namespace {

constexpr int CP_THREADS = 256;
constexpr int CP_LDS_BYTES = 32 * 1024;     // per workgroup, pit and uniforms
constexpr int CP_MAX_S = 1024;
constexpr int CP_TILE = 16;                 // gram: pairs per tile side
constexpr int CP_STAGE = 64;                // gram: rows per LDS stage
constexpr int CP_CHUNK = 1024;              // gram: rows per workgroup; the chunks are added by the finish kernel
constexpr int CP_MAX_N = 2048;              // uniforms: four rows of e within the LDS budget
constexpr int CP_WIDE_N = 512;              // uniforms: sixteen rows up to here
constexpr int CP_KU = 8;                    // uniforms: rows of factor_t in flight per thread
constexpr float CP_U_LO = 5.9604644775390625e-08f;   // 2^-24
constexpr float CP_U_HI = 0.999999940395355224609375f;   // 1 - 2^-24

struct CpPitArgs {                          // travels by value in the kernel arguments
  const float* target;                      // [count, H, N]
  const float* forecast;                    // [count, Q, H, N]
  float* u;                                 // [count, H, N]
  long long items;                          // count * H * (N / VEC)
  int H, N, Q, clamp;
  float tau[CF_MAX_Q];
};

struct CpGramArgs {
  const float* u;                           // [M, N]
  double* part;                             // [chunks][4][N][N]: pair count, sum z_i z_j, sum z_i, sum z_i^2
  long long* pairs;                         // [N, N]
  double* sums;                             // [3][N][N]
  long long M;
  int N, tiles, chunks;
};

struct CpUniArgs {
  const float* factor_t;                    // [N, N], factor_t[k * N + n] = L[n][k]
  float* u;                                 // [rows, N]
  unsigned long long origin0, seed, offset;
  long long rows;                           // Bo * S * Lsteps
  int S, Lsteps, N, step, horizon;
  const float* step_factor;                 // [Lsteps, Lsteps], step_factor[j * Lsteps + i] = A[j][i]; the STEPS kernels only
  int tile_rows;                            // (RT / Lsteps) * Lsteps: the rows of a tile that whole paths fill; STEPS only
};

// keeps a NaN, unlike fminf / fmaxf
__device__ inline float cp_clamp(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The transform of y under the thread's column col[q * stride], q < Q: the inverse of sc_draw, operation by operation.
__device__ inline float cp_pit(const CpPitArgs& a, const float* col, int stride, float y) {
#pragma clang fp contract(off)
  const int Q = a.Q;
  int below = 0;                                              // values <= y: the ordered column has them first
  bool missing = y != y;
  for (int q = 0; q < Q; ++q) {
    const float v = col[q * stride];
    below += v <= y ? 1 : 0;
    missing |= v != v;
  }
  if (missing) return __uint_as_float(CF_NAN_BITS);
  const int i = min(max(below - 1, 0), Q - 2);
  float t0 = a.tau[0], t1 = a.tau[1];                         // (the levels are read at uniform indices only)
  for (int q = 1; q < Q - 1; ++q) {
    t0 = q == i ? a.tau[q] : t0;
    t1 = q == i ? a.tau[q + 1] : t1;
  }
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
  const float d = hi - lo, num = y - lo;
  float wt = __fdiv_rn(num, d);
  if (d == 0.f) wt = num == 0.f ? 0.5f : (num > 0.f ? INFINITY : -INFINITY);
  if (a.clamp) wt = cp_clamp(wt, 0.f, 1.f);
  const float span = t1 - t0;
  const float m = span * wt;
  const float u = t0 + m;
  return cp_clamp(u, CP_U_LO, CP_U_HI);
}

template <int VEC>
__global__ __launch_bounds__(CP_THREADS) void cp_pit_kernel(const CpPitArgs a) {
  extern __shared__ float4 cp_lds[];
  const int T = blockDim.x, t = threadIdx.x, Q = a.Q, N = a.N, H = a.H;
  const long long item = (long long)blockIdx.x * T + t;
  if (item >= a.items) return;                                // (no barrier below)
  const int per = N / VEC;
  const size_t row = (size_t)(item / per);
  const int n = (int)(item - (long long)row * per) * VEC;
  const size_t c = row / (unsigned)H;
  const int h = (int)(row - c * (unsigned)H);
  float* col = reinterpret_cast<float*>(cp_lds) + t;          // word (q * VEC + k) * T
  const float* f = a.forecast + (c * Q * H + h) * N + n;
  for (int q = 0; q < Q; ++q) {
    float v[VEC];
    cf_load<VEC>(f + (size_t)q * H * N, v);
#pragma unroll
    for (int k = 0; k < VEC; ++k) col[(q * VEC + k) * T] = v[k];
  }
  float y[VEC], u[VEC];
  cf_load<VEC>(a.target + row * N + n, y);
#pragma unroll
  for (int k = 0; k < VEC; ++k) u[k] = cp_pit(a, col + k * T, VEC * T, y[k]);
  cf_store<VEC>(a.u + row * N + n, u);
}

__global__ __launch_bounds__(CP_THREADS) void cp_gram_kernel(const CpGramArgs a) {
  __shared__ double zi[CP_STAGE * CP_TILE], zj[CP_STAGE * CP_TILE];
  const int t = threadIdx.x, N = a.N, ti = t >> 4, tj = t & (CP_TILE - 1);
  const int chunk = blockIdx.x / (unsigned)(a.tiles * a.tiles);
  const int rem = blockIdx.x - chunk * (a.tiles * a.tiles);
  const int i0 = (rem / a.tiles) * CP_TILE, j0 = (rem - (rem / a.tiles) * a.tiles) * CP_TILE;
  const long long r0 = (long long)chunk * CP_CHUNK, r1 = min(a.M, r0 + CP_CHUNK);
  const double absent = __longlong_as_double(0x7ff8000000000000ll);
  double s = 0.0, sa = 0.0, sq = 0.0;
  int m = 0;
  for (long long rs = r0; rs < r1; rs += CP_STAGE) {
    __syncthreads();                                           // the previous stage has been read
#pragma unroll 1
    for (int e = t; e < 2 * CP_STAGE * CP_TILE; e += CP_THREADS) {             // both panels in one walk: one copy of normcdfinv
      const bool second = e >= CP_STAGE * CP_TILE;
      const int w = second ? e - CP_STAGE * CP_TILE : e;
      const long long row = rs + (w >> 4);
      const int c = (second ? j0 : i0) + (w & (CP_TILE - 1));
      (second ? zj : zi)[w] = (row < r1 && c < N) ? normcdfinv((double)a.u[(size_t)row * N + c]) : absent;
    }
    __syncthreads();
    const int lim = (int)min((long long)CP_STAGE, r1 - rs);
#pragma unroll 4
    for (int r = 0; r < lim; ++r) {
      const double x = zi[r * CP_TILE + ti], y = zj[r * CP_TILE + tj];
      if (x == x && y == y) {
        s = fma(x, y, s);
        sa += x;
        sq = fma(x, x, sq);
        ++m;
      }
    }
  }
  const int i = i0 + ti, j = j0 + tj;
  if (i < N && j < N) {
    const size_t NN = (size_t)N * N, at = (size_t)chunk * 4 * NN + (size_t)i * N + j;
    a.part[at] = (double)m;
    a.part[at + NN] = s;
    a.part[at + 2 * NN] = sa;
    a.part[at + 3 * NN] = sq;
  }
}

__global__ __launch_bounds__(CP_THREADS) void cp_gram_finish_kernel(const CpGramArgs a) {
  const size_t NN = (size_t)a.N * a.N, e = (size_t)blockIdx.x * CP_THREADS + threadIdx.x;
  if (e >= NN) return;
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < a.chunks; ++c) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += a.part[((size_t)c * 4 + k) * NN + e];
  }
  a.pairs[e] = (long long)v[0];                                // (a sum of counts below 2^31: exact)
  a.sums[e] = v[1];
  a.sums[NN + e] = v[2];
  a.sums[2 * NN + e] = v[3];
}

// RT rows per workgroup (a multiple of 4: e is read four rows at a time); a thread owns the nodes t, t + 256, ..
// STEPS: a tile holds whole paths, a.tile_rows = (RT / Lsteps) * Lsteps live rows (the rest is padding, neither drawn nor stored),
// and the steps of a path are mixed on e in LDS between the fill and the node sum: e[j] <- sum_{i <= j} A[j][i] e[i], i ascending,
// walking j downwards, so that every e[i] a row still needs is the drawn one.
template <int RT, bool STEPS>
__global__ __launch_bounds__(CP_THREADS) void cp_uniforms_kernel(const CpUniArgs a) {
  static_assert(RT % 4 == 0, "e is read as float4 over the rows");
  extern __shared__ float4 cp_lds[];
  float* e = reinterpret_cast<float*>(cp_lds);                // [N][RT]
  const int t = threadIdx.x, N = a.N;
  const int nq = (N + 3) >> 2;                                // Philox calls of a row
  const int used = STEPS ? a.tile_rows : RT;                  // the tile's rows that stand for rows of u
  const long long row0 = (long long)blockIdx.x * used;
  for (int it = t; it < RT * nq; it += CP_THREADS) {
    const int r = it / nq, g = it - r * nq;
    const long long row = row0 + r;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (r < used && row < a.rows) {
      const unsigned long long p = (unsigned long long)(row / a.Lsteps);        // the path b * S + s
      const unsigned long long j = (unsigned long long)(row - (long long)p * a.Lsteps);
      const unsigned long long b = p / (unsigned)a.S, s = p - b * (unsigned)a.S;
      const unsigned long long ctr = (((a.origin0 + b) * (unsigned long long)a.S + s) * (unsigned long long)a.horizon +
                                      (unsigned long long)a.step + j) * (unsigned long long)nq + (unsigned long long)g;
      uint32_t w[4];
      sg_philox4(a.seed, a.offset, ctr, w);
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] = normcdfinvf(sc_uniform(w[k]));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (4 * g + k < N) e[(4 * g + k) * RT + r] = v[k];
  }
  __syncthreads();
  if constexpr (STEPS) {
    // one thread per (node, path of the tile): Lsteps words of one LDS row, in place.  step_factor is read at indices that
    // do not depend on the thread, and only at i <= j.
    const int Ls = a.Lsteps, PT = used / Ls;
    for (int it = t; it < N * PT; it += CP_THREADS) {
      const int k = it / PT, pl = it - k * PT;
      float* ep = e + k * RT + pl * Ls;
      for (int j = Ls - 1; j >= 0; --j) {
        const float* aj = a.step_factor + j * Ls;
        float g = 0.f;
        for (int i = 0; i <= j; ++i) g = fmaf(aj[i], ep[i], g);
        ep[j] = g;
      }
    }
    __syncthreads();
  }
  for (int n0 = 0; n0 < N; n0 += CP_THREADS) {
    const int n = n0 + t;
    const bool live = n < N;
    const float* f = a.factor_t + (live ? n : 0);
    float z[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) z[r] = 0.f;
    const int full = n0, top = min(N, n0 + CP_THREADS);      // k < full: below every n of this pass
    for (int k0 = 0; k0 < top; k0 += CP_KU) {
      // CP_KU rows of factor_t are requested before the first is used (every address is inside the matrix: the row index is
      // held below `top`, the column is a live one); what a thread must not use is replaced by 0 AFTER the load, and
      // fmaf(0, e, z) == z for the finite e
      float l[CP_KU];
#pragma unroll
      for (int i = 0; i < CP_KU; ++i) l[i] = f[(size_t)min(k0 + i, top - 1) * N];
#pragma unroll
      for (int i = 0; i < CP_KU; ++i) {
        const int k = k0 + i;
        const float lk = (k < top && (k < full || (live && k <= n))) ? l[i] : 0.f;
        const float* ek = e + min(k, top - 1) * RT;
#pragma unroll
        for (int r = 0; r < RT; r += 4) {
          const float4 v = *reinterpret_cast<const float4*>(ek + r);
          z[r] = fmaf(lk, v.x, z[r]);
          z[r + 1] = fmaf(lk, v.y, z[r + 1]);
          z[r + 2] = fmaf(lk, v.z, z[r + 2]);
          z[r + 3] = fmaf(lk, v.w, z[r + 3]);
        }
      }
    }
    if (!live) continue;
#pragma unroll
    for (int r = 0; r < RT; ++r)
      if (r < used && row0 + r < a.rows) a.u[(size_t)(row0 + r) * N + n] = cp_clamp(normcdff(z[r]), CP_U_LO, CP_U_HI);
  }
}

// the launch shape of gram; false where the entries answer SG_EINVAL
bool cp_gram_plan(long M, int N, CpGramArgs* a) {
  if (M <= 0 || N <= 0 || !sg_fits_int(M) || !sg_fits_int((long long)N * N)) return false;
  a->M = M; a->N = N;
  a->tiles = sg_ceil_div(N, CP_TILE);
  a->chunks = sg_ceil_div(M, CP_CHUNK);
  return sg_fits_int((long long)a->tiles * a->tiles * a->chunks);
}

}  // namespace

extern "C" int stemgnn_copula_pit(const float* target, const float* forecast, const float* taus, long count, int H, int N, int Q,
                                  int tails, float* u, void* stream) {
  if (!target || !forecast || !taus || !u) return SG_EINVAL;
  if (count <= 0 || H <= 0 || N <= 0 || Q < 2 || Q > CF_MAX_Q) return SG_EINVAL;
  if (tails != SG_SCENARIO_LINEAR && tails != SG_SCENARIO_CLAMP) return SG_EINVAL;
  CpPitArgs a = {};
  for (int q = 0; q < Q; ++q) {
    const float lo = q ? taus[q - 1] : 0.f;
    if (!(taus[q] > lo) || !(taus[q] < 1.f)) return SG_EINVAL;   // strictly increasing inside (0, 1); a NaN fails both
    a.tau[q] = taus[q];
  }
  // what an int carries in the kernel: a row's nodes, a column's row stride, the rows and the grid
  if (!sg_fits_int((long long)H * N) || !sg_fits_int((long long)Q * H * N) || !sg_fits_int((long long)count * H))
    return SG_EINVAL;
  const bool vec = (N & 3) == 0 && sg_aligned16(target) && sg_aligned16(forecast) && sg_aligned16(u);
  const int VEC = vec ? 4 : 1;
  a.target = target; a.forecast = forecast; a.u = u;
  a.items = (long long)count * H * (N / VEC);
  a.H = H; a.N = N; a.Q = Q;
  a.clamp = tails == SG_SCENARIO_CLAMP;
  int T = CP_THREADS;
  while (T > 64 && ((size_t)T * Q * VEC * 4 > (size_t)CP_LDS_BYTES || T - 64 >= a.items)) T -= 64;
  const size_t lds = (size_t)T * Q * VEC * 4;                 // <= 32 KB: Q <= 32, VEC <= 4, T >= 64
  const long long grid = (a.items + T - 1) / T;
  if (!sg_fits_int(grid)) return SG_EINVAL;
  if (vec)
    hipLaunchKernelGGL(cp_pit_kernel<4>, dim3((unsigned)grid), dim3(T), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(cp_pit_kernel<1>, dim3((unsigned)grid), dim3(T), lds, (hipStream_t)stream, a);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t stemgnn_copula_scratch_doubles(long M, int N) {
  CpGramArgs a = {};
  return cp_gram_plan(M, N, &a) ? (size_t)a.chunks * 4 * (size_t)N * N : 0;
}

extern "C" int stemgnn_copula_gram(const float* u, long M, int N, double* scratch, long long* pairs, double* sums,
                                   void* stream) {
  if (!u || !scratch || !pairs || !sums) return SG_EINVAL;
  CpGramArgs a = {};
  if (!cp_gram_plan(M, N, &a)) return SG_EINVAL;
  a.u = u; a.part = scratch; a.pairs = pairs; a.sums = sums;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(cp_gram_kernel, dim3((unsigned)(a.tiles * a.tiles * a.chunks)), dim3(CP_THREADS), 0, st, a);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(cp_gram_finish_kernel, dim3((unsigned)sg_ceil_div((long long)N * N, CP_THREADS)), dim3(CP_THREADS), 0, st,
                     a);
  SG_TRY(hipGetLastError());
  return 0;
}

namespace {

// both uniforms entries: step_factor == nullptr is the entry without a step mix (rows fill the tiles; any Lsteps)
int cp_uniforms(const float* factor_t, const float* step_factor, int Bo, int S, int Lsteps, int N, int step, int horizon,
                long long origin0, unsigned long long seed, unsigned long long offset, float* u, void* stream) {
  if (!factor_t || !u) return SG_EINVAL;
  if (Bo <= 0 || Lsteps <= 0 || N <= 0 || N > CP_MAX_N || S < 1 || S > CP_MAX_S || step < 0 || step >= horizon)
    return SG_EINVAL;
  // what an int carries in the kernel: the rows (the grid is at most that), a path's steps
  if (!sg_fits_int((long long)Bo * S * Lsteps) || !sg_fits_int((long long)S * horizon)) return SG_EINVAL;
  const int RT = N <= CP_WIDE_N ? 16 : 4;                     // N * RT * 4 <= 32 KB
  if (step_factor && Lsteps > RT) return SG_EINVAL;           // a tile holds whole paths
  CpUniArgs a = {};
  a.factor_t = factor_t; a.u = u;
  a.origin0 = (unsigned long long)origin0; a.seed = seed; a.offset = offset;
  a.rows = (long long)Bo * S * Lsteps;
  a.S = S; a.Lsteps = Lsteps; a.N = N; a.step = step; a.horizon = horizon;
  a.step_factor = step_factor;
  a.tile_rows = step_factor ? (RT / Lsteps) * Lsteps : RT;
  const dim3 grid((unsigned)sg_ceil_div(a.rows, a.tile_rows));
  const size_t lds = (size_t)N * RT * 4;
  hipStream_t st = (hipStream_t)stream;
  if (RT == 16) {
    if (step_factor) hipLaunchKernelGGL((cp_uniforms_kernel<16, true>), grid, dim3(CP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((cp_uniforms_kernel<16, false>), grid, dim3(CP_THREADS), lds, st, a);
  } else {
    if (step_factor) hipLaunchKernelGGL((cp_uniforms_kernel<4, true>), grid, dim3(CP_THREADS), lds, st, a);
    else hipLaunchKernelGGL((cp_uniforms_kernel<4, false>), grid, dim3(CP_THREADS), lds, st, a);
  }
  SG_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int stemgnn_copula_uniforms(const float* factor_t, int Bo, int S, int Lsteps, int N, int step, int horizon,
                                       long long origin0, unsigned long long seed, unsigned long long offset, float* u,
                                       void* stream) {
  return cp_uniforms(factor_t, nullptr, Bo, S, Lsteps, N, step, horizon, origin0, seed, offset, u, stream);
}

extern "C" int stemgnn_copula_uniforms_steps(const float* factor_t, const float* step_factor, int Bo, int S, int Lsteps, int N,
                                             int step, int horizon, long long origin0, unsigned long long seed,
                                             unsigned long long offset, float* u, void* stream) {
  if (!step_factor) return SG_EINVAL;
  return cp_uniforms(factor_t, step_factor, Bo, S, Lsteps, N, step, horizon, origin0, seed, offset, u, stream);
}
