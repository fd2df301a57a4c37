// Scenario trees by staged forward selection (Heitsch & Roemisch 2009): the prefix distances of sampled paths at every stage
// boundary, and the tree of representative paths with integer counts (include/stemgnn_hip.h: stemgnn_scenario_stage_distances /
// stemgnn_scenario_tree).
//
// stage distances: paths [count, S, H, M] fp32.  The tile of path_distance.h with the walk over L = H M cut at the stage
//           boundaries b_t M (pd_tile, STAGED): D [count, T, S, S], D_t the distance of the prefixes that end with stage t.  The
//           split of a stage's sum depends on M and the bounds alone.
// tree:     one workgroup per origin, thread u owns candidate u; forward selection run stage by stage on the pieces of
//           forward_select.h (the LDS layout with par and the multiplicities beside near, the check of D_t while it goes to LDS,
//           the weighted sums, the argmin on (taken, z, u), the update of m and near, the refusal).  par is the member's node
//           of the previous stage.  Phase A gives every parent its first child (the sums run over the parent's members), phase B
//           adds the remaining nodes (the sums run over all members, a member only ever moved onto a path of its own parent).
//           A refusal found at a later stage overwrites what the earlier stages stored.
// No floating-point atomics, no allocation, no memset, no host synchronisation: the same bits on every run, origin by origin,
// however the origins are batched into calls.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "forward_select.h"
#include "path_distance.h"
#include "sg_host.h"

namespace {

constexpr int TR_MAX_T = PD_MAX_T;
constexpr int TR_MAX_W = 1 << 24;

// NG wave groups of 256 threads: 1, or PD_NQ (one per partial sum)
template <bool SCALED, int NG>
__global__ __launch_bounds__(PD_THREADS * NG) void tr_distance_kernel(const PdStagedArgs a) {
  pd_tile<SCALED, NG, true>(a, a.T, a.end);
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

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void tr_tree_kernel(const TrTreeArgs a) {
  extern __shared__ double tr_tree_mem[];
  const int S = a.S, T = a.T, nT = a.nT, t = threadIdx.x, nthr = blockDim.x;
  const FsLds l = fs_carve(tr_tree_mem, S, 3);
  double* m = l.m;
  int* near = l.arr;                                            // [S]: the member's node of this stage
  int* par = near + S;                                          // [S]: the member's node of the previous stage
  int* mu = par + S;                                            // [S]: the multiplicities
  const size_t c = blockIdx.x;
  const int ld = IN_LDS ? a.ld : S;
  for (int k = t; k < S; k += nthr) {
    mu[k] = a.mult ? a.mult[c * S + k] : 1;
    par[k] = 0;
  }
  __syncthreads();
  int pos;
  bool refused = !sg_census(mu, S, a.W, &pos) || nT > pos;      // (the same in every thread)
  const bool candidate = !refused && t < S && mu[t] > 0;
  int n_prev = 1;
  for (int st = 0; st < T && !refused; ++st) {
    const double* Dg = a.D + (c * T + st) * (size_t)S * S;
    const double* Dr = IN_LDS ? l.D : Dg;                       // what the picks read
    const int bad = fs_stage<IN_LDS>(Dg, l.D, mu, S, ld);
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
          z = fs_add_product(z, (double)w, fmin(m[k], d));
        }
      }
      double v = z;
      int idx = cand ? t : FS_MAX_S + t;
      fs_argmin(v, idx, l);
      if (t == 0) {
        const int sel = idx < FS_MAX_S ? idx : -1;              // -1: parent i has no member (a phase A pick only)
        l.pick[0] = sel;
        a.node_path[(c * T + st) * nT + i] = sel;
        a.node_parent[(c * T + st) * nT + i] = sel < 0 ? i : par[sel];
      }
      __syncthreads();
      const int sel = l.pick[0];
      if (sel >= 0) {
        taken = taken || t == sel;
        fs_lower(l, near, Dr, ld, S, sel, i, mu, par, par[sel]);
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
        if (mu[k] > 0) s = fs_add_product(s, (double)mu[k], m[k]);
      a.cost[c * T + st] = s / (double)a.W;
    }
    __syncthreads();                                            // near and m are read
    for (int k = t; k < S; k += nthr) par[k] = near[k];
    n_prev = n_t;
    __syncthreads();
  }
  if (refused)                                                  // this origin alone, every stage
    fs_refuse(a.node_path + c * T * nT, a.node_parent + c * T * nT, a.node_count + c * T * nT, T * nT, a.assign + c * T * S,
              T * S, a.cost + c * T, T);
}

}  // namespace

extern "C" int stemgnn_scenario_stage_distances(const float* paths, const double* scale, long count, int S, int H, int M, int T,
                                                const int* bounds, int squared, double* D, void* stream) {
  if (!paths || !bounds || !D) return SG_EINVAL;
  if (count <= 0 || S <= 0 || H <= 0 || M <= 0 || T <= 0 || S > FS_MAX_S || T > TR_MAX_T || (squared != 0 && squared != 1))
    return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)S * H * M) || !sg_fits_int((long long)count * T * S * S)) return SG_EINVAL;
  PdStagedArgs a = {};
  int before = 0;
  for (int t = 0; t < T; ++t) {
    if (bounds[t] <= before || bounds[t] > H) return SG_EINVAL;
    before = bounds[t];
    a.end[t] = bounds[t] * M;
  }
  if (before != H) return SG_EINVAL;
  a.paths = paths; a.scale = scale; a.D = D; a.S = S; a.L = H * M; a.T = T; a.squared = squared;
  static void (*const kern[2][2])(PdStagedArgs) = {{tr_distance_kernel<false, 1>, tr_distance_kernel<false, PD_NQ>},
                                                   {tr_distance_kernel<true, 1>, tr_distance_kernel<true, PD_NQ>}};
  return pd_launch(a, count, kern, (hipStream_t)stream);
}

extern "C" int stemgnn_scenario_tree(const double* D, const int* mult_in, long count, int S, int T, const int* nodes, int W,
                                     int* node_path, int* node_parent, int* node_count, int* assign, double* cost,
                                     void* stream) {
  if (!D || !nodes || !node_path || !node_parent || !node_count || !assign || !cost) return SG_EINVAL;
  if (count <= 0 || S <= 0 || T <= 0 || S > FS_MAX_S || T > TR_MAX_T || W < 1 || W > TR_MAX_W) return SG_EINVAL;
  if (!mult_in && W != S) return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)count * T * S * S)) return SG_EINVAL;
  TrTreeArgs a = {};
  int before = 1;
  for (int t = 0; t < T; ++t) {
    if (nodes[t] < before || nodes[t] > S) return SG_EINVAL;
    before = nodes[t];
    a.n[t] = nodes[t];
  }
  a.D = D; a.mult = mult_in; a.node_path = node_path; a.node_parent = node_parent; a.node_count = node_count;
  a.assign = assign; a.cost = cost; a.S = S; a.T = T; a.nT = before; a.W = W;
  return fs_launch<tr_tree_kernel<true>, tr_tree_kernel<false>>(a, 3, count, (hipStream_t)stream);
}
