// The distance tile of sampled paths: the one body behind rd_distance_kernel (reduce.hip: the whole trajectory) and
// tr_distance_kernel (tree.hip: the prefixes at every stage boundary), and the launcher both entries use.
//
// paths [count, S, L] fp32, a path's trajectory one contiguous run of L floats.  One workgroup per (origin, 32 x 32 tile (I, J)
// of path pairs, I <= J), the energy launch of ensemble.hip with the walk over L instead of over the nodes of one step: the
// columns are walked in chunks of 64; the two panels of 32 paths x 64 values (one when I == J) go to LDS as fp64, rows 65 doubles
// apart (plain coalesced row loads: a wave reads 64 consecutive floats of one path); thread (ti, tj) = (t / 16, t % 16) owns the
// pairs (2 ti + {0, 1}, 2 tj + {0, 1}) and adds ((x_il - x_jl) * scale_l)^2 into four registers -- DIFFERENCES, never the Gram
// expansion: two coincident paths give exactly 0.  A half-wave reads two panel-A rows (broadcasts) and sixteen panel-B rows
// (8-byte reads at banks 4 tj): conflict-free.  The tile is stored where i <= j, and once more, transposed through LDS, where
// i < j: D[i, j] and D[j, i] are one value's bits, and both stores run along rows of D.
// A pair's sum is kept as FOUR partial sums, chunk c adding into sum c % 4, joined as ((s0 + s1) + s2) + s3: four independent
// FMA chains per pair in the 256-thread form -- and the split of the wide form, which a call takes when its grid leaves compute
// units idle (count x tile pairs <= the CUs, e.g. a live query: 3 workgroups at S = 64): 1024 threads, wave group g = 0 .. 3
// with panels of its own walks the chunks c % 4 = g and owns sum g; the four meet in LDS and group 0 joins them in the same
// order and stores.  Both forms give the same bits, so batching does not show in the result.
// STAGED cuts the walk at the stage boundaries end[0] < .. < end[T - 1] = L: stage t walks its own columns in chunks of 64
// counted from the stage's first column (the last one partial); at the boundary the stage's sum Q_t = ((s0 + s1) + s2) + s3 is
// added to the running prefix and the tile of D_t goes out.  The paths are read once for all T tiles.  One stage ending at L
// is the unstaged walk, operation for operation; the unstaged form knows that when it is compiled, so it carries no stage loop,
// no prefix and no bounds (the prefix and the loop cost 8 to 16 registers, and a wave per SIMD or two of occupancy).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/stemgnn_hip.h"
#include "devattr.h"
#include "sg_host.h"

constexpr int PD_THREADS = 256;
constexpr int PD_MAX_T = 16;
constexpr int PD_PT = 32;                   // paths per panel
constexpr int PD_LC = 64;                   // trajectory values per chunk
constexpr int PD_LD = PD_LC + 1;            // doubles between panel rows
constexpr int PD_TLD = PD_PT + 1;           // doubles between rows of the transposed tile
constexpr int PD_NQ = 4;                    // partial sums per pair (and stage), chunk c adding into sum c % 4
constexpr int PD_GROUP_DOUBLES = 2 * PD_PT * PD_LD + PD_LC;   // LDS of one wave group: panel A, panel B, the scale's chunk

struct PdArgs {
  const float* paths;                       // [count, S, L]
  const double* scale;                      // [L] or NULL
  double* D;                                // [count, S, S]; staged: [count, T, S, S]
  int S, L, nt, pairs, squared;
};

struct PdStagedArgs : PdArgs {
  int T;
  int end[PD_MAX_T];                        // the stages' last column + 1
};

// NG wave groups of 256 threads: 1, or PD_NQ (one per partial sum).  T and end are read where STAGED alone.
template <bool SCALED, int NG, bool STAGED>
__device__ __forceinline__ void pd_tile(const PdArgs& a, int T, const int* end) {
  extern __shared__ __align__(16) double pd_lds[];              // per wave group: panel A, panel B, the scale's chunk
  constexpr int NQ = PD_NQ / NG;                                // partial sums a thread keeps
  const int t = threadIdx.x & (PD_THREADS - 1), g = threadIdx.x / PD_THREADS, S = a.S, L = a.L;
  const int stages = STAGED ? T : 1;
  double* pa = pd_lds + (size_t)g * PD_GROUP_DOUBLES;
  double* pb_own = pa + PD_PT * PD_LD;
  double* sc = pb_own + PD_PT * PD_LD;
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
  const int ln = t & (PD_LC - 1), lr = t >> 6;                  // the loader's column and first row
  const int ti = t >> 4, tj = t & 15;
  double pre[2][2] = {{0.0, 0.0}, {0.0, 0.0}};                  // D_t^2 so far
  int lo = 0;
  for (int st = 0; st < stages; ++st) {
    const int hi = STAGED ? end[st] : L;                        // (lo < hi <= L)
    double acc[NQ][2][2];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q][0][0] = acc[q][0][1] = acc[q][1][0] = acc[q][1][1] = 0.0;
    for (long long c0 = lo; c0 < hi; c0 += PD_NQ * PD_LC) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        // chunk (c0 - lo) / 64 + q of the stage adds into sum q; the wide form: this group's sum is g.  Past the stage's end
        // (the same for a whole group; the 256-thread form stops there, the groups of the wide one keep the barriers in step)
        // nothing is live and nothing is added
        const long long l0 = c0 + (NG == 1 ? q : g) * PD_LC;
        if (NG == 1 && l0 >= hi) break;
        const long long l = l0 + ln;
        const bool live = l < hi;
        __syncthreads();                                        // the previous chunk, or the previous stage's tile, has been read
        for (int r = lr; r < PD_PT; r += PD_THREADS / PD_LC) {
          const int si = I * PD_PT + r, sj = J * PD_PT + r;
          pa[r * PD_LD + ln] = (live && si < S) ? (double)px[(size_t)si * L + l] : 0.0;
          if (!diag) pb_own[r * PD_LD + ln] = (live && sj < S) ? (double)px[(size_t)sj * L + l] : 0.0;
        }
        if (SCALED && t < PD_LC) sc[t] = live ? a.scale[l] : 0.0;
        __syncthreads();
        const int lim = (int)min((long long)PD_LC, hi - l0);    // (<= 0 past the end)
        const double* ra = pa + (2 * ti) * PD_LD;
        const double* rb = pb + (2 * tj) * PD_LD;
        for (int k = 0; k < lim; ++k) {
          const double a0 = ra[k], a1 = ra[PD_LD + k], b0 = rb[k], b1 = rb[PD_LD + k];
          const double w = SCALED ? sc[k] : 1.0;
          double d;
          d = a0 - b0; if (SCALED) d = __dmul_rn(d, w); acc[q][0][0] = fma(d, d, acc[q][0][0]);
          d = a0 - b1; if (SCALED) d = __dmul_rn(d, w); acc[q][0][1] = fma(d, d, acc[q][0][1]);
          d = a1 - b0; if (SCALED) d = __dmul_rn(d, w); acc[q][1][0] = fma(d, d, acc[q][1][0]);
          d = a1 - b1; if (SCALED) d = __dmul_rn(d, w); acc[q][1][1] = fma(d, d, acc[q][1][1]);
        }
      }
    }
    lo = hi;
    __syncthreads();                                            // the panels are read
    double sum[2][2];                                           // Q_t = ((s0 + s1) + s2) + s3
    if (NG == 1) {
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          double s = acc[0][u][v];
#pragma unroll
          for (int q = 1; q < NQ; ++q) s += acc[q][u][v];
          sum[u][v] = s;
        }
    } else {                                                    // the groups' sums meet in their panel A, slot (pair, t)
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) pa[(2 * u + v) * PD_THREADS + t] = acc[0][u][v];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const double* slot = pd_lds + (2 * u + v) * PD_THREADS + t;
          double s = slot[0];
#pragma unroll
          for (int q = 1; q < PD_NQ; ++q) s += slot[(size_t)q * PD_GROUP_DOUBLES];
          sum[u][v] = s;
        }
    }
    // group 0 stores; its panel B becomes the transposed tile (panel A may still be read by the join above)
    double* Dc = a.D + (c * stages + st) * (size_t)S * S;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        pre[u][v] = st == 0 ? sum[u][v] : pre[u][v] + sum[u][v];   // D_t^2 = ((Q_1 + Q_2) + ..) + Q_t
        if (g == 0) {
          const int ri = 2 * ti + u, rj = 2 * tj + v;
          const int si = I * PD_PT + ri, sj = J * PD_PT + rj;
          const double d = a.squared ? pre[u][v] : sqrt(pre[u][v]);
          pb_own[rj * PD_TLD + ri] = d;
          if (si <= sj && sj < S) Dc[(size_t)si * S + sj] = d;  // (si <= sj < S)
        }
      }
    __syncthreads();
    if (g == 0) {
      const int rj = t >> 3, q0 = (t & 7) * 4;                  // row rj of the transposed tile, four of its columns
      const int sj = J * PD_PT + rj;
      if (sj < S) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int si = I * PD_PT + q0 + q;
          if (si < sj) Dc[(size_t)sj * S + si] = pb_own[rj * PD_TLD + q0 + q];
        }
      }
    }
  }
}

// Fills a's tile counts and launches kern[scale given][wide]: the wide form where the grid leaves compute units idle and the
// walk has chunks to share out; the same bits either way.  The guards of the wide kernels' 132 KiB of LDS are per Args, that
// is per kernel family.
template <class Args>
int pd_launch(Args& a, long count, void (*const (&kern)[2][2])(Args), hipStream_t st) {
  static SgDynLds guard[2];
  a.nt = sg_ceil_div(a.S, PD_PT);
  a.pairs = a.nt * (a.nt + 1) / 2;
  if (!sg_fits_int((long long)count * a.pairs)) return SG_EINVAL;
  const int scaled = a.scale ? 1 : 0;
  const bool wide = (long long)count * a.pairs <= sg_num_cus() && a.L > PD_LC;
  const int ng = wide ? PD_NQ : 1;
  const size_t lds = (size_t)ng * PD_GROUP_DOUBLES * 8;
  SG_TRY(sg_ensure_dyn_lds((const void*)kern[scaled][wide], lds, guard[scaled]));   // (a no-op for the 256-thread form)
  hipLaunchKernelGGL(kern[scaled][wide], dim3((unsigned)(count * a.pairs)), dim3(PD_THREADS * ng), lds, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}
