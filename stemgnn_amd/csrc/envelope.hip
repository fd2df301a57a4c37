// Simultaneous scenario bands: the studentised sup-norm envelope of sampled paths (include/stemgnn_hip.h:
// stemgnn_scenario_envelope).  Per (origin, column): a centre m_h and a scale s_h per step from the S paths,
// every path's depth d_s = max_h |x[s,h] - m_h| / s_h, the cf_rank(T, coverage)-th smallest depth (in weights) as the ensemble's
// own multiplier, the band m_h -+ q s_h and the depth of the target.  All arithmetic fp64, every sum over s ascending, products
// and sums rounded separately (the whole file is compiled under `fp contract(off)`), so a numpy loop gives the same bits.
//
// One launch, one workgroup of 256 threads per (origin, tile of Ct columns), Ct = 32 .. 4.  A thread owns one column of the tile
// in every phase, so the loads coalesce over n; what it shares the column with changes from phase to phase:
//   load:    the tile's S * H * Ct values go to LDS (float4 or scalar by VEC, ENV_LOADS loads in flight per thread) where they
//            fit beside the rest: `paths` is then read from memory once; beyond that the phases read `paths` themselves with
//            the same indices (IN_LDS = false).
//   moments: thread (g, c) owns the steps g, g + G, .. of column c: two passes over s.
//   depth:   thread (g, c) owns the paths g, g + G, .. of column c, ENV_GROUP of them at a time so that as many divisions are
//            independent: the maximum over h, which no order changes (every term of a present column is a finite number >= 0),
//            walked from step g % H on so that the lanes of a wave meet different LDS banks.
//   select:  thread (g, c) counts, for ENV_GROUP of its paths at a time, the weight of the depths <= their own; the smallest
//            depth that reaches the rank wins (a minimum over exact values: no order changes it).
//   store:   bands, moments, chosen; the target's terms step by step, then their maximum; NaN in an absent column or origin.
// Every phase is a chain of dependent fp64 operations per thread, so the tile is kept narrow enough (ENV_TILE_BYTES) for several
// workgroups to share a compute unit.
// No atomics, no allocation, no host synchronisation: the same bits on every run and for every batching of `count`.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "conformal_select.h"
#include "scenario_math.h"
#include "sg_host.h"

#pragma clang fp contract(off)

namespace {

constexpr int ENV_THREADS = 256;
constexpr int ENV_MAX_S = 1024;
constexpr int ENV_MAX_H = 256;
constexpr int ENV_MAX_T = 1 << 24;          // w x and the cumulative weights are exact
constexpr int ENV_MAX_CT = 32;
constexpr int ENV_LOADS = 8;                // tile loads a thread has in flight
constexpr int ENV_GROUP = 4;                // paths a thread walks side by side in the depth and select phases
constexpr size_t ENV_TILE_BYTES = 40 * 1024;  // the LDS a workgroup should stay within (four per compute unit): decides the
                                              // tile's width, not the result
constexpr size_t ENV_LDS_BYTES = 64 * 1024; // the LDS a workgroup may have

struct EnvArgs {
  const float* paths;                       // [count, S, H, C]
  const int* mult;                          // [count, S] or NULL
  const float* target;                      // [count, H, C] or NULL
  const double* multiplier;                 // NULL, [1] or [C]
  double* moments;                          // [count, 2, H, C]
  double* depth;                            // [count, S, C] or NULL
  double* chosen;                           // [count, C]
  double* truth;                            // [count, C] or NULL
  float* bands;                             // [count, 2, H, C]
  double rank;                              // cf_rank(T, coverage)
  int S, H, C, T, Ct, ct_shift, tiles, ignore_nan, multiplier_n;
};

__host__ __device__ inline size_t env_lds_bytes(int S, int H, int Ct, bool in_lds) {
  return ((size_t)3 * H * Ct + (size_t)S * Ct + ENV_THREADS) * 8 + (in_lds ? (size_t)S * H * Ct * 4 : 0) + (size_t)S * 4 +
         (size_t)Ct * 4;
}

__device__ inline double env_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ inline double env_inf() { return __longlong_as_double(0x7ff0000000000000ll); }
__device__ inline bool env_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <int VEC, bool IN_LDS, bool WEIGHTED>
__global__ __launch_bounds__(ENV_THREADS) void env_kernel(const EnvArgs a) {
  extern __shared__ float4 env_lds4[];
  const int S = a.S, H = a.H, C = a.C, Ct = a.Ct, t = threadIdx.x;
  double* ms = reinterpret_cast<double*>(env_lds4);             // [H][Ct]
  double* ss = ms + H * Ct;                                     // [H][Ct]
  double* ts = ss + H * Ct;                                     // [H][Ct]: the target's terms, NaN where it is missing
  double* dep = ts + H * Ct;                                    // [S][Ct]
  double* red = dep + S * Ct;                                   // [ENV_THREADS]
  float* tile = reinterpret_cast<float*>(red + ENV_THREADS);    // [S * H][Ct] where IN_LDS
  int* wm = reinterpret_cast<int*>(tile + (IN_LDS ? (size_t)S * H * Ct : 0));   // [S]
  int* bad = wm + S;                                            // [Ct]
  const size_t b = blockIdx.x / (unsigned)a.tiles;
  const int c0 = (int)(blockIdx.x - b * (unsigned)a.tiles) * Ct;
  const int live = min(Ct, C - c0);                             // columns of this tile (a multiple of VEC)
  const int c = t & (Ct - 1), g = t >> a.ct_shift, G = ENV_THREADS >> a.ct_shift;
  const bool mine = c < live;
  const size_t n = (size_t)c0 + c;
  const double nan = env_nan(), inf = env_inf(), T = (double)a.T;

  bool ok = true;
  if (WEIGHTED) {
    ok = wt_present(a.mult + b * S, S, a.T, wm);
  } else {
    for (int k = t; k < S; k += ENV_THREADS) wm[k] = 1;
  }
  if (t < Ct) bad[t] = ok ? 0 : 1;
  __syncthreads();

  const float* src = a.paths + b * S * H * (size_t)C + c0;      // value (s, h) of column c: src[(s * H + h) * C + c]
  if (IN_LDS && ok) {
    const int ps = a.ct_shift - (VEC == 4 ? 2 : 0), items = (S * H) << ps;
    for (int e0 = t; e0 < items; e0 += ENV_THREADS * ENV_LOADS) {
      float v[ENV_LOADS][VEC];
      int at[ENV_LOADS];
#pragma unroll
      for (int u = 0; u < ENV_LOADS; ++u) {
        const int e = e0 + u * ENV_THREADS, r = e >> ps, cc = (e - (r << ps)) * VEC;
        at[u] = -1;
        if (e < items && cc < live && (!WEIGHTED || wm[r / H] > 0)) {
          at[u] = r * Ct + cc;
          cf_load<VEC>(src + (size_t)r * C + cc, v[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < ENV_LOADS; ++u) {
        if (at[u] < 0) continue;
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          tile[at[u] + i] = v[u][i];
          if (!env_finite(v[u][i])) bad[(at[u] & (Ct - 1)) + i] = 1;
        }
      }
    }
    __syncthreads();
  }
  auto value = [&](int s, int h) -> double {
    const int r = s * H + h;
    return (double)(IN_LDS ? tile[r * Ct + c] : src[(size_t)r * C + c]);
  };

  // ---- moments: thread (g, c) owns the steps g, g + G, ..
  if (ok && mine) {
    for (int h = g; h < H; h += G) {
      double acc = 0.0;
      bool nf = false;
#pragma unroll 8
      for (int s = 0; s < S; ++s) {
        double w = 1.0;
        if (WEIGHTED) {
          if (wm[s] <= 0) continue;
          w = (double)wm[s];
        }
        const double x = value(s, h);
        if (!IN_LDS) nf |= !env_finite((float)x);
        const double wx = WEIGHTED ? w * x : x;
        acc = acc + wx;
      }
      const double m = acc / T;
      double var = 0.0;
#pragma unroll 8
      for (int s = 0; s < S; ++s) {
        double w = 1.0;
        if (WEIGHTED) {
          if (wm[s] <= 0) continue;
          w = (double)wm[s];
        }
        const double d = value(s, h) - m;
        const double sq = d * d;
        const double wsq = WEIGHTED ? w * sq : sq;
        var = var + wsq;
      }
      ms[h * Ct + c] = m;
      ss[h * Ct + c] = sqrt(var / T);
      if (nf) bad[c] = 1;
    }
  }
  __syncthreads();
  const bool absent = !ok || (mine && bad[c] != 0);

  // ---- depth: thread (g, c) owns the paths g, g + G, .., ENV_GROUP at a time
  if (ok && mine) {
    for (int s0 = g; s0 < S; s0 += ENV_GROUP * G) {
      double d[ENV_GROUP];
      bool on[ENV_GROUP];
#pragma unroll
      for (int u = 0; u < ENV_GROUP; ++u) {
        const int s = s0 + u * G;
        on[u] = s < S && (!WEIGHTED || wm[s] > 0);
        d[u] = on[u] ? 0.0 : nan;
      }
      int h = g % H;
      for (int i = 0; i < H; ++i) {
        const double sd = ss[h * Ct + c], m = ms[h * Ct + c];
        if (sd != 0.0) {
#pragma unroll
          for (int u = 0; u < ENV_GROUP; ++u) {
            if (!on[u]) continue;
            const double r = fabs(value(s0 + u * G, h) - m) / sd;
            d[u] = r > d[u] ? r : d[u];
          }
        }
        h = h + 1 == H ? 0 : h + 1;
      }
#pragma unroll
      for (int u = 0; u < ENV_GROUP; ++u) {
        const int s = s0 + u * G;
        if (s >= S) continue;
        dep[s * Ct + c] = d[u];
        if (a.depth) a.depth[(b * S + s) * (size_t)C + n] = absent ? nan : d[u];
      }
    }
  } else if (a.depth && mine) {
    for (int s = g; s < S; s += G) a.depth[(b * S + s) * (size_t)C + n] = nan;
  }
  __syncthreads();

  // ---- select: the smallest depth whose weight of depths <= it reaches the rank (a member of weight 0 has depth NaN: it is
  // below nothing and adds nothing)
  double best = inf;
  if (ok && mine && !absent && a.rank <= T) {
    for (int s0 = g; s0 < S; s0 += ENV_GROUP * G) {
      double ds[ENV_GROUP];
      int cnt[ENV_GROUP];
#pragma unroll
      for (int u = 0; u < ENV_GROUP; ++u) {
        const int s = s0 + u * G;
        ds[u] = s < S ? dep[s * Ct + c] : nan;
        cnt[u] = 0;
      }
#pragma unroll 4
      for (int j = 0; j < S; ++j) {
        const double dj = dep[j * Ct + c];
        const int wj = WEIGHTED ? wm[j] : 1;
#pragma unroll
        for (int u = 0; u < ENV_GROUP; ++u) cnt[u] += dj <= ds[u] ? wj : 0;
      }
#pragma unroll
      for (int u = 0; u < ENV_GROUP; ++u)
        if ((double)cnt[u] >= a.rank && ds[u] < best) best = ds[u];
    }
  }
  red[t] = best;                                                // [g][c]
  __syncthreads();
  for (int k = 0; k < G; ++k) {
    const double o = red[(k << a.ct_shift) + c];
    best = o < best ? o : best;
  }
  const double q = !mine ? nan : a.multiplier ? a.multiplier[a.multiplier_n == 1 ? 0 : n] : best;

  // ---- store
  const size_t HC = (size_t)H * C;
  if (mine) {
    for (int h = g; h < H; h += G) {
      const double m = ms[h * Ct + c], sd = ss[h * Ct + c];
      double lo, hi;
      if (absent) {
        lo = hi = nan;
      } else if (q == inf) {
        lo = -inf;
        hi = inf;
      } else {
        const double r = q * sd;
        lo = m - r;
        hi = m + r;
      }
      const size_t at = (size_t)h * C + n;
      a.moments[b * 2 * HC + at] = absent ? nan : m;
      a.moments[b * 2 * HC + HC + at] = absent ? nan : sd;
      a.bands[b * 2 * HC + at] = (float)lo;
      a.bands[b * 2 * HC + HC + at] = (float)hi;
      if (a.target) {
        const double y = (double)a.target[b * HC + at];
        ts[h * Ct + c] = y != y ? nan : sd != 0.0 ? fabs(y - m) / sd : (y == m ? 0.0 : inf);
      }
    }
    if (g == 0) a.chosen[b * C + n] = absent ? nan : best;
  }
  if (!a.target) return;
  __syncthreads();
  if (mine && g == G - 1) {
    double tr = 0.0;
    bool any = false, miss = false;
    for (int h = 0; h < H; ++h) {
      const double r = ts[h * Ct + c];
      if (r != r) {
        miss = true;
      } else {
        any = true;
        tr = r > tr ? r : tr;
      }
    }
    a.truth[b * C + n] = (absent || !any || (miss && !a.ignore_nan)) ? nan : tr;
  }
}

template <int VEC, bool IN_LDS>
void env_launch(const EnvArgs& a, unsigned grid, size_t lds, hipStream_t st) {
  if (a.mult)
    hipLaunchKernelGGL((env_kernel<VEC, IN_LDS, true>), dim3(grid), dim3(ENV_THREADS), lds, st, a);
  else
    hipLaunchKernelGGL((env_kernel<VEC, IN_LDS, false>), dim3(grid), dim3(ENV_THREADS), lds, st, a);
}
}  // namespace

extern "C" int stemgnn_scenario_envelope(const float* paths, const int* mult, int total, const float* target, int ignore_nan,
                                         const double* multiplier, int multiplier_n, int count, int S, int H, int C,
                                         double coverage, double* moments, double* depth, double* chosen, double* truth,
                                         float* bands, void* stream) {
  if (!paths || !moments || !chosen || !bands) return SG_EINVAL;
  if ((target == nullptr) != (truth == nullptr)) return SG_EINVAL;
  if (S < 1 || S > ENV_MAX_S || H < 1 || H > ENV_MAX_H || count <= 0 || C <= 0) return SG_EINVAL;
  if (!(coverage > 0.0 && coverage < 1.0)) return SG_EINVAL;
  if (multiplier && multiplier_n != 1 && multiplier_n != C) return SG_EINVAL;
  if (mult && (total < 1 || total > ENV_MAX_T)) return SG_EINVAL;
  if (!sg_fits_int((long long)count * S * C) || !sg_fits_int((long long)count * H * C) || !sg_fits_int((long long)S * H * C))
    return SG_EINVAL;
  EnvArgs a = {};
  a.paths = paths; a.mult = mult; a.target = target; a.multiplier = multiplier; a.moments = moments; a.depth = depth;
  a.chosen = chosen; a.truth = truth; a.bands = bands;
  a.S = S; a.H = H; a.C = C; a.ignore_nan = ignore_nan ? 1 : 0; a.multiplier_n = multiplier_n;
  a.T = mult ? total : S;
  a.rank = cf_rank(a.T, coverage);
  int cap = 4;                                                  // the widest tile: no wider than the columns need
  while (cap < C && cap < ENV_MAX_CT) cap <<= 1;
  bool in_lds = true;
  int Ct = cap;                                                 // the widest that leaves room for other workgroups
  while (Ct > 4 && env_lds_bytes(S, H, Ct, true) > ENV_TILE_BYTES) Ct >>= 1;
  if (env_lds_bytes(S, H, Ct, true) > ENV_LDS_BYTES) {          // the values stay in memory: the widest tile of the rest
    in_lds = false;
    Ct = cap;
    while (Ct > 4 && env_lds_bytes(S, H, Ct, false) > ENV_TILE_BYTES) Ct >>= 1;
  }
  a.Ct = Ct;
  a.ct_shift = Ct == 32 ? 5 : Ct == 16 ? 4 : Ct == 8 ? 3 : 2;
  a.tiles = sg_ceil_div(C, Ct);
  if (!sg_fits_int((long long)count * a.tiles)) return SG_EINVAL;
  const size_t lds = env_lds_bytes(S, H, Ct, in_lds);
  const unsigned grid = (unsigned)count * (unsigned)a.tiles;
  hipStream_t st = (hipStream_t)stream;
  const bool vec = C % 4 == 0 && sg_aligned16(paths);
  if (in_lds) {
    if (vec) env_launch<4, true>(a, grid, lds, st);
    else env_launch<1, true>(a, grid, lds, st);
  } else {                                                      // (no tile loads: VEC has nothing to decide)
    env_launch<1, false>(a, grid, lds, st);
  }
  SG_TRY(hipGetLastError());
  return 0;
}
