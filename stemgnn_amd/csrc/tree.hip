// Scenario trees by staged forward selection (Heitsch & Roemisch 2009): the prefix distances of sampled paths at every stage
// boundary, and the tree of representative paths with integer counts (include/stemgnn_hip.h: stemgnn_scenario_stage_distances /
// stemgnn_scenario_tree).
//
// stage distances: paths [count, S, H, M] fp32.  The distance launch of reduce.hip -- one workgroup per (origin, 32 x 32 tile
//           (I, J) of path pairs, I <= J), the two panels of 32 paths x 64 values in LDS as fp64, thread (ti, tj) owning the
//           pairs (2 ti + {0, 1}, 2 tj + {0, 1}), DIFFERENCES and one fp64 FMA per value -- with the walk over L = H M cut at
//           the stage boundaries: stage t walks its own columns [b_{t-1} M, b_t M) in chunks of 64 counted from the stage's
//           first column (the last one partial), chunk c of the stage adding into sum c % 4; at the boundary the stage's sum
//           Q_t = ((s0 + s1) + s2) + s3 is added to the running prefix and the tile of D_t goes out, where i <= j directly and
//           where i < j transposed through LDS, so D_t[i, j] and D_t[j, i] are one value's bits.  The paths are read once for
//           all T tiles.  The split depends on M and the bounds alone.  As in reduce.hip a call whose grid leaves compute
//           units idle (count x tile pairs <= the CUs: a live query) takes the wide form: 1024 threads, wave group g = 0 .. 3
//           with panels of its own walks the stage's chunks c % 4 = g and owns sum g; at every boundary the four meet in LDS
//           and group 0 joins them in the same order and stores.  Both forms give the same bits.
// tree:     one workgroup per origin, thread u owns candidate u; the pick kernel of weighted.hip run stage by stage.  A
//           stage's D_t [S, S] is checked (every entry between two members of positive multiplicity finite and >= 0) while it
//           goes to LDS, rows S | 1 doubles apart, where that fits 160 KiB (S <= 141); beyond, rows are read from memory.  par
//           (the member's node of the previous stage), m, near and the multiplicities are in LDS.  Phase A gives every parent
//           its first child (the sums run over the parent's members), phase B adds the remaining nodes (the sums run over all
//           members, a member only ever moved onto a path of its own parent); the argmin is on (taken, z, u).  A refusal found
//           at a later stage overwrites what the earlier stages stored.
// No floating-point atomics, no allocation, no memset, no host synchronisation: the same bits on every run, origin by origin,
// however the origins are batched into calls.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "devattr.h"
#include "sg_host.h"

namespace {

constexpr int TR_THREADS = 256;
constexpr int TR_MAX_S = 1024;
constexpr int TR_MAX_T = 16;
constexpr int TR_MAX_W = 1 << 24;
constexpr int TR_PT = 32;                   // distances: paths per panel
constexpr int TR_LC = 64;                   // distances: trajectory values per chunk
constexpr int TR_LD = TR_LC + 1;            // distances: doubles between panel rows
constexpr int TR_TLD = TR_PT + 1;           // distances: doubles between rows of the transposed tile
constexpr int TR_NQ = 4;                    // distances: partial sums per pair and stage, chunk c adding into sum c % 4
constexpr int TR_DIST_DOUBLES = 2 * TR_PT * TR_LD + TR_LC;
constexpr size_t TR_LDS_BYTES = 160 * 1024; // tree: LDS of one workgroup on gfx950

struct TrDistArgs {
  const float* paths;                       // [count, S, L]
  const double* scale;                      // [L] or NULL
  double* D;                                // [count, T, S, S]
  int S, L, T, nt, pairs, squared;
  int end[TR_MAX_T];                        // the stages' last column + 1: b_t * M
};

// NG wave groups of 256 threads: 1, or TR_NQ (one per partial sum)
template <bool SCALED, int NG>
__global__ __launch_bounds__(TR_THREADS * NG) void tr_distance_kernel(const TrDistArgs a) {
  extern __shared__ __align__(16) double tr_dist_lds[];         // per wave group: panel A, panel B, the scale's chunk
  constexpr int NQ = TR_NQ / NG;                                // partial sums a thread keeps
  const int t = threadIdx.x & (TR_THREADS - 1), g = threadIdx.x / TR_THREADS, S = a.S, L = a.L;
  double* pa = tr_dist_lds + (size_t)g * TR_DIST_DOUBLES;
  double* pb_own = pa + TR_PT * TR_LD;
  double* sc = pb_own + TR_PT * TR_LD;
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
  const int ln = t & (TR_LC - 1), lr = t >> 6;                  // the loader's column and first row
  const int ti = t >> 4, tj = t & 15;
  double pre[2][2] = {{0.0, 0.0}, {0.0, 0.0}};                  // D_t^2 so far
  int lo = 0;
  for (int st = 0; st < a.T; ++st) {
    const int hi = a.end[st];                                   // (lo < hi <= L)
    double acc[NQ][2][2];
#pragma unroll
    for (int q = 0; q < NQ; ++q) acc[q][0][0] = acc[q][0][1] = acc[q][1][0] = acc[q][1][1] = 0.0;
    for (long long c0 = lo; c0 < hi; c0 += TR_NQ * TR_LC) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        // chunk (c0 - lo) / 64 + q of the stage adds into sum q; the wide form: this group's sum is g.  Past the stage's end
        // (the same for a whole group; the 256-thread form stops there, the groups of the wide one keep the barriers in step)
        // nothing is live and nothing is added
        const long long l0 = c0 + (NG == 1 ? q : g) * TR_LC;
        if (NG == 1 && l0 >= hi) break;
        const long long l = l0 + ln;
        const bool live = l < hi;
        __syncthreads();                                        // the previous chunk, or the previous stage's tile, has been read
        for (int r = lr; r < TR_PT; r += TR_THREADS / TR_LC) {
          const int si = I * TR_PT + r, sj = J * TR_PT + r;
          pa[r * TR_LD + ln] = (live && si < S) ? (double)px[(size_t)si * L + l] : 0.0;
          if (!diag) pb_own[r * TR_LD + ln] = (live && sj < S) ? (double)px[(size_t)sj * L + l] : 0.0;
        }
        if (SCALED && t < TR_LC) sc[t] = live ? a.scale[l] : 0.0;
        __syncthreads();
        const int lim = (int)min((long long)TR_LC, hi - l0);    // (<= 0 past the end)
        const double* ra = pa + (2 * ti) * TR_LD;
        const double* rb = pb + (2 * tj) * TR_LD;
        for (int k = 0; k < lim; ++k) {
          const double a0 = ra[k], a1 = ra[TR_LD + k], b0 = rb[k], b1 = rb[TR_LD + k];
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
        for (int v = 0; v < 2; ++v) pa[(2 * u + v) * TR_THREADS + t] = acc[0][u][v];
      __syncthreads();
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) {
          const double* slot = tr_dist_lds + (2 * u + v) * TR_THREADS + t;
          double s = slot[0];
#pragma unroll
          for (int q = 1; q < TR_NQ; ++q) s += slot[(size_t)q * TR_DIST_DOUBLES];
          sum[u][v] = s;
        }
    }
    // group 0 stores; its panel B becomes the transposed tile (panel A may still be read by the join above)
    double* Dc = a.D + (c * a.T + st) * (size_t)S * S;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int v = 0; v < 2; ++v) {
        pre[u][v] = st == 0 ? sum[u][v] : pre[u][v] + sum[u][v];   // D_t^2 = ((Q_1 + Q_2) + ..) + Q_t
        if (g == 0) {
          const int ri = 2 * ti + u, rj = 2 * tj + v;
          const int si = I * TR_PT + ri, sj = J * TR_PT + rj;
          const double d = a.squared ? pre[u][v] : sqrt(pre[u][v]);
          pb_own[rj * TR_TLD + ri] = d;
          if (si <= sj && sj < S) Dc[(size_t)si * S + sj] = d;  // (si <= sj < S)
        }
      }
    __syncthreads();
    if (g == 0) {
      const int rj = t >> 3, q0 = (t & 7) * 4;                  // row rj of the transposed tile, four of its columns
      const int sj = J * TR_PT + rj;
      if (sj < S) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int si = I * TR_PT + q0 + q;
          if (si < sj) Dc[(size_t)sj * S + si] = pb_own[rj * TR_TLD + q0 + q];
        }
      }
    }
  }
}

struct TrTreeArgs {
  const double* D;                          // [count, T, S, S]
  const int* mult;                          // [count, S] or NULL (all ones)
  int* node_path;                           // [count, T, nT]
  int* node_parent;                         // [count, T, nT]
  int* node_count;                          // [count, T, nT]
  int* assign;                              // [count, T, S]
  double* cost;                             // [count, T]
  int S, T, nT, ld, W;                      // ld: doubles between rows of the LDS copy
  int n[TR_MAX_T];                          // nodes per stage
};

// the smaller of two (taken, value, index) candidates: an untaken one first, then the smaller value, then the lower index
__device__ inline void tr_take_min(double& v, int& i, double ov, int oi) {
  const bool ours_taken = i >= TR_MAX_S, theirs_taken = oi >= TR_MAX_S;
  const bool better = ours_taken != theirs_taken ? ours_taken : (ov < v || (ov == v && oi < i));
  if (better) {
    v = ov;
    i = oi;
  }
}

// z + p * d with the product and the sum rounded separately: plain operators under `fp contract(off)` (weighted.hip: the
// __dmul_rn / __dadd_rn of this toolchain's headers fuse once inlined)
__device__ inline double tr_add_product(double z, double p, double d) {
#pragma clang fp contract(off)
  const double term = p * d;
  return z + term;
}

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void tr_tree_kernel(const TrTreeArgs a) {
  extern __shared__ double tr_tree_mem[];
  const int S = a.S, T = a.T, nT = a.nT, t = threadIdx.x, nthr = blockDim.x, nw = nthr >> 6;
  double* m = tr_tree_mem;                                      // [S]
  double* wv = m + S;                                           // [16]: the waves' candidates
  int* wi = reinterpret_cast<int*>(wv + 16);                    // [16]
  int* near = wi + 16;                                          // [S]: the member's node of this stage
  int* par = near + S;                                          // [S]: the member's node of the previous stage
  int* mu = par + S;                                            // [S]: the multiplicities
  int* pick = mu + S;                                           // [2]
  double* Dl = reinterpret_cast<double*>(wi + ((3 * S + 18 + 1) & ~1));   // [S][ld], IN_LDS only
  const size_t c = blockIdx.x;
  const int ld = IN_LDS ? a.ld : S;
  for (int k = t; k < S; k += nthr) {
    mu[k] = a.mult ? a.mult[c * S + k] : 1;
    par[k] = 0;
  }
  __syncthreads();
  long long sum = 0;
  int neg = 0, pos = 0;
  for (int k = 0; k < S; ++k) {
    const int w = mu[k];
    neg |= w < 0 ? 1 : 0;
    pos += w > 0 ? 1 : 0;
    sum += w;
  }
  bool refused = neg || sum != (long long)a.W || nT > pos;      // (the same in every thread)
  const bool candidate = !refused && t < S && mu[t] > 0;
  int n_prev = 1;
  for (int st = 0; st < T && !refused; ++st) {
    const double* Dg = a.D + (c * T + st) * (size_t)S * S;
    const double* Dr = IN_LDS ? Dl : Dg;                        // what the picks read
    int bad = 0;
    for (int i = t; i < S * S; i += nthr) {
      const int k = i / S, u = i - k * S;
      if (mu[k] <= 0 || mu[u] <= 0) continue;                   // a row or column of multiplicity 0 is not read
      const double d = Dg[i];
      bad |= (d >= 0.0 && d < INFINITY) ? 0 : 1;                // a NaN fails both comparisons
      if (IN_LDS) Dl[k * ld + u] = d;
    }
    for (int k = t; k < S; k += nthr) {
      m[k] = INFINITY;
      near[k] = -1;
    }
    if (__syncthreads_or(bad)) {
      refused = true;
      break;
    }
    const int n_t = a.n[st];
    const int pu = candidate ? par[t] : -1;
    bool taken = !candidate;
    for (int i = 0; i < n_t; ++i) {
      const bool first = i < n_prev;                            // phase A: parent i's first child
      const bool cand = !taken && (!first || pu == i);
      double z = 0.0;
      if (cand) {
        const double* col = Dr + t;
        for (int k = 0; k < S; ++k) {
          const int w = mu[k];
          if (w <= 0) continue;
          const int pk = par[k];
          if (first && pk != i) continue;
          const double d = pk == pu ? col[(size_t)k * ld] : INFINITY;
          z = tr_add_product(z, (double)w, fmin(m[k], d));
        }
      }
      double v = z;
      int idx = cand ? t : TR_MAX_S + t;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(v, off);
        const int oi = __shfl_down(idx, off);
        tr_take_min(v, idx, ov, oi);
      }
      if ((t & 63) == 0) {
        wv[t >> 6] = v;
        wi[t >> 6] = idx;
      }
      __syncthreads();
      if (t == 0) {
        for (int w = 1; w < nw; ++w) tr_take_min(v, idx, wv[w], wi[w]);
        const int sel = idx < TR_MAX_S ? idx : -1;              // -1: parent i has no member (a phase A pick only)
        pick[0] = sel;
        a.node_path[(c * T + st) * nT + i] = sel;
        a.node_parent[(c * T + st) * nT + i] = sel < 0 ? i : par[sel];
      }
      __syncthreads();
      const int sel = pick[0];
      if (sel >= 0) {
        taken = taken || t == sel;
        const int ps = par[sel];
        for (int k = t; k < S; k += nthr) {
          if (mu[k] <= 0 || par[k] != ps) continue;
          const double d = Dr[(size_t)k * ld + sel];
          if (d < m[k]) {
            m[k] = d;
            near[k] = i;
          }
        }
      }
      __syncthreads();                                          // m, near and pick are settled for the next pick
    }
    for (int k = t; k < S; k += nthr) a.assign[(c * T + st) * S + k] = near[k];
    for (int j = t; j < nT; j += nthr) {
      int n = 0;
      if (j < n_t) {
        for (int k = 0; k < S; ++k) n += near[k] == j ? mu[k] : 0;
      } else {
        a.node_path[(c * T + st) * nT + j] = -1;
        a.node_parent[(c * T + st) * nT + j] = -1;
      }
      a.node_count[(c * T + st) * nT + j] = n;
    }
    if (t == 0) {
      double s = 0.0;
      for (int k = 0; k < S; ++k)
        if (mu[k] > 0) s = tr_add_product(s, (double)mu[k], m[k]);
      a.cost[c * T + st] = s / (double)a.W;
    }
    __syncthreads();                                            // near and m are read
    for (int k = t; k < S; k += nthr) par[k] = near[k];
    n_prev = n_t;
    __syncthreads();
  }
  if (refused) {                                                // this origin alone, every stage
    for (int j = t; j < T * nT; j += nthr) {
      a.node_path[c * T * nT + j] = -1;
      a.node_parent[c * T * nT + j] = -1;
      a.node_count[c * T * nT + j] = 0;
    }
    for (int k = t; k < T * S; k += nthr) a.assign[c * T * S + k] = -1;
    for (int j = t; j < T; j += nthr) a.cost[c * T + j] = NAN;
  }
}

bool tr_fits_int(long long v) { return v > 0 && v < (1ll << 31); }

size_t tr_tree_lds(int S, int ld, bool in_lds) {
  // m [S] and the waves' 16 values as doubles; 16 + 3 S + 2 ints, rounded to a double; the copy of D_t
  return ((size_t)S + 16) * 8 + (size_t)((3 * S + 18 + 1) & ~1) * 4 + (in_lds ? (size_t)S * ld * 8 : 0);
}

SgDynLds tr_tree_guard, tr_wide_guard[2];

}  // namespace

extern "C" int stemgnn_scenario_stage_distances(const float* paths, const double* scale, long count, int S, int H, int M, int T,
                                                const int* bounds, int squared, double* D, void* stream) {
  if (!paths || !bounds || !D) return SG_EINVAL;
  if (count <= 0 || S <= 0 || H <= 0 || M <= 0 || T <= 0 || S > TR_MAX_S || T > TR_MAX_T || (squared != 0 && squared != 1))
    return SG_EINVAL;
  if (!tr_fits_int(count) || !tr_fits_int((long long)S * H * M) || !tr_fits_int((long long)count * T * S * S)) return SG_EINVAL;
  TrDistArgs a = {};
  int before = 0;
  for (int t = 0; t < T; ++t) {
    if (bounds[t] <= before || bounds[t] > H) return SG_EINVAL;
    before = bounds[t];
    a.end[t] = bounds[t] * M;
  }
  if (before != H) return SG_EINVAL;
  a.paths = paths; a.scale = scale; a.D = D; a.S = S; a.L = H * M; a.T = T; a.squared = squared;
  a.nt = sg_ceil_div(S, TR_PT);
  a.pairs = a.nt * (a.nt + 1) / 2;
  if (!tr_fits_int((long long)count * a.pairs)) return SG_EINVAL;
  const dim3 grid((unsigned)(count * a.pairs));
  const size_t lds = (size_t)TR_DIST_DOUBLES * 8;
  hipStream_t st = (hipStream_t)stream;
  // the wide form where the grid leaves compute units idle and a stage has chunks to share out; the same bits either way
  const bool wide = (long long)count * a.pairs <= sg_num_cus() && a.L > TR_LC;
  if (wide) {
    if (scale) {
      SG_TRY(sg_ensure_dyn_lds((const void*)tr_distance_kernel<true, TR_NQ>, TR_NQ * lds, tr_wide_guard[1]));
      hipLaunchKernelGGL((tr_distance_kernel<true, TR_NQ>), grid, dim3(TR_THREADS * TR_NQ), TR_NQ * lds, st, a);
    } else {
      SG_TRY(sg_ensure_dyn_lds((const void*)tr_distance_kernel<false, TR_NQ>, TR_NQ * lds, tr_wide_guard[0]));
      hipLaunchKernelGGL((tr_distance_kernel<false, TR_NQ>), grid, dim3(TR_THREADS * TR_NQ), TR_NQ * lds, st, a);
    }
  } else if (scale) {
    hipLaunchKernelGGL((tr_distance_kernel<true, 1>), grid, dim3(TR_THREADS), lds, st, a);
  } else {
    hipLaunchKernelGGL((tr_distance_kernel<false, 1>), grid, dim3(TR_THREADS), lds, st, a);
  }
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_scenario_tree(const double* D, const int* mult_in, long count, int S, int T, const int* nodes, int W,
                                     int* node_path, int* node_parent, int* node_count, int* assign, double* cost,
                                     void* stream) {
  if (!D || !nodes || !node_path || !node_parent || !node_count || !assign || !cost) return SG_EINVAL;
  if (count <= 0 || S <= 0 || T <= 0 || S > TR_MAX_S || T > TR_MAX_T || W < 1 || W > TR_MAX_W) return SG_EINVAL;
  if (!mult_in && W != S) return SG_EINVAL;
  if (!tr_fits_int(count) || !tr_fits_int((long long)count * T * S * S)) return SG_EINVAL;
  TrTreeArgs a = {};
  int before = 1;
  for (int t = 0; t < T; ++t) {
    if (nodes[t] < before || nodes[t] > S) return SG_EINVAL;
    before = nodes[t];
    a.n[t] = nodes[t];
  }
  a.D = D; a.mult = mult_in; a.node_path = node_path; a.node_parent = node_parent; a.node_count = node_count;
  a.assign = assign; a.cost = cost; a.S = S; a.T = T; a.nT = before; a.W = W;
  a.ld = S | 1;                             // an odd number of doubles: a column read meets every bank pair once
  const bool in_lds = tr_tree_lds(S, a.ld, true) <= TR_LDS_BYTES;
  const size_t lds = tr_tree_lds(S, a.ld, in_lds);
  int threads = (S + 63) & ~63;             // a thread per candidate; at least four waves to bring D in
  if (threads < TR_THREADS) threads = TR_THREADS;
  hipStream_t st = (hipStream_t)stream;
  if (in_lds) {
    SG_TRY(sg_ensure_dyn_lds((const void*)tr_tree_kernel<true>, lds, tr_tree_guard));
    hipLaunchKernelGGL(tr_tree_kernel<true>, dim3((unsigned)count), dim3(threads), lds, st, a);
  } else {
    hipLaunchKernelGGL(tr_tree_kernel<false>, dim3((unsigned)count), dim3(threads), lds, st, a);
  }
  SG_TRY(hipGetLastError());
  return 0;
}
