// Forward selection on a distance matrix (Heitsch & Roemisch 2003): the pieces that the pick of K representatives
// (rd_pick_kernel in reduce.hip, wt_pick_kernel in weighted.hip: one kernel, fs_pick) and the staged pick of a scenario tree
// (tr_tree_kernel in tree.hip: its own control flow) share, and the launcher of all three.
//
// One workgroup per origin, thread u owns candidate u.  D [S, S] is checked (every entry finite and >= 0; WEIGHTED: between two
// members of positive multiplicity, the others are not read) while it goes to LDS, rows S | 1 doubles apart, where that fits
// (below); beyond, row k is read from memory, contiguous in u.  Per pick: z_u = sum_k p_k min(m_k, D[k, u]) with k = 0, 1, .. in
// order, one fp64 product and one fp64 add after the other (the order is the definition; all p_k = 1 where not WEIGHTED, and
// 1 * x is x, so the sum is written z += x there); an argmin over (taken, z, u) -- a wave reduction on pairs, the waves in
// index order -- that returns the lowest index among equal values; then m_k = min(m_k, D[k, u*]) and, where that lowered m_k
// strictly, near_k = the pick's position (ties stay with the earlier pick).  counts: thread j adds the multiplicities of near == j.
// No floating-point atomics: the same bits on every run, origin by origin, however the origins are batched into calls.
//
// LDS of a workgroup: m [S] and the waves' 16 candidate values as doubles, then 16 + 2 + NI * S ints (the waves' indices, the
// pick, and NI arrays of S: near; WEIGHTED also the multiplicities; the tree also par), rounded to a double, then the copy of D.
// The limit is the 160 KiB a gfx950 workgroup may ask for.  With ld = S | 1 the copy is 141 * 141 * 8 = 159048 bytes at S = 141
// and 142 * 143 * 8 = 162448 at S = 142, the rest 1.9 to 3 KiB for NI = 1 .. 3: every NI holds D in LDS up to S = 141 and reads
// it from memory from S = 142 on, so the three entries change over at the same S.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/stemgnn_hip.h"
#include "devattr.h"
#include "scenario_math.h"
#include "sg_host.h"

constexpr int FS_MAX_S = 1024;
constexpr int FS_MIN_THREADS = 256;
constexpr size_t FS_LDS_BYTES = 160 * 1024;

struct FsLds {
  double* m;                                // [S]: the distance to the nearest pick
  double* wv;                               // [16]: the waves' candidates
  int* wi;                                  // [16]
  int* pick;                                // [2]
  int* arr;                                 // [NI][S]: near, then the caller's
  double* D;                                // [S][ld], IN_LDS only
};

__host__ __device__ inline size_t fs_head_ints(int S, int ni) { return (size_t)((18 + ni * S + 1) & ~1); }

__device__ inline FsLds fs_carve(double* mem, int S, int ni) {
  FsLds l;
  l.m = mem;
  l.wv = mem + S;
  l.wi = reinterpret_cast<int*>(l.wv + 16);
  l.pick = l.wi + 16;
  l.arr = l.pick + 2;
  l.D = reinterpret_cast<double*>(l.wi + fs_head_ints(S, ni));
  return l;
}

// the smaller of two (taken, value, index) candidates: an untaken one first, then the smaller value, then the lower index; a
// taken candidate carries FS_MAX_S + its index
__device__ inline void fs_take_min(double& v, int& i, double ov, int oi) {
  const bool ours_taken = i >= FS_MAX_S, theirs_taken = oi >= FS_MAX_S;
  const bool better = ours_taken != theirs_taken ? ours_taken : (ov < v || (ov == v && oi < i));
  if (better) {
    v = ov;
    i = oi;
  }
}

// z + p * d with the product and the sum rounded separately: plain operators under `fp contract(off)` (the __dmul_rn / __dadd_rn
// of this toolchain's headers are `x * y` / `x + y` under the default contraction, which fuses them once inlined)
__device__ inline double fs_add_product(double z, double p, double d) {
#pragma clang fp contract(off)
  const double term = p * d;
  return z + term;
}

// The workgroup's smallest candidate, in thread 0's (v, idx) after the barrier this ends with: a shuffle tree inside each wave,
// then thread 0 takes the waves in index order.
__device__ inline void fs_argmin(double& v, int& idx, const FsLds& l) {
  const int t = threadIdx.x, nw = blockDim.x >> 6;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const double ov = __shfl_down(v, off);
    const int oi = __shfl_down(idx, off);
    fs_take_min(v, idx, ov, oi);
  }
  if ((t & 63) == 0) {
    l.wv[t >> 6] = v;
    l.wi[t >> 6] = idx;
  }
  __syncthreads();
  if (t == 0)
    for (int w = 1; w < nw; ++w) fs_take_min(v, idx, l.wv[w], l.wi[w]);
}

// D [S, S] from memory, checked and (IN_LDS) copied to Dl; mu: the multiplicities, or NULL for all ones.  Returns this thread's
// verdict, for __syncthreads_or: non-zero where an entry it read is negative, infinite or a NaN.
template <bool IN_LDS>
__device__ inline int fs_stage(const double* Dg, double* Dl, const int* mu, int S, int ld) {
  const int t = threadIdx.x, nthr = blockDim.x;
  int bad = 0;
  for (int i = t; i < S * S; i += nthr) {
    const int k = i / S, u = i - k * S;
    if (mu && (mu[k] <= 0 || mu[u] <= 0)) continue;             // a row or column of multiplicity 0 is not read
    const double d = Dg[i];
    bad |= (d >= 0.0 && d < INFINITY) ? 0 : 1;                  // a NaN fails both comparisons
    if (IN_LDS) Dl[k * ld + u] = d;
  }
  return bad;
}

// after a pick: m_k = min(m_k, D[k, sel]) and near_k = p where that is strictly lower, over the members of positive multiplicity
// (mu, or NULL: all) whose parent is ps (par, or NULL: all)
__device__ inline void fs_lower(const FsLds& l, int* near, const double* Dr, int ld, int S, int sel, int p, const int* mu,
                                const int* par, int ps) {
  const int t = threadIdx.x, nthr = blockDim.x;
  for (int k = t; k < S; k += nthr) {
    if ((mu && mu[k] <= 0) || (par && par[k] != ps)) continue;
    const double d = Dr[(size_t)k * ld + sel];
    if (d < l.m[k]) {
      l.m[k] = d;
      near[k] = p;
    }
  }
}

// a refused origin: n picks of -1 (in both arrays, `second` may be NULL) with count 0, ns assignments of -1, nc costs of NaN
__device__ inline void fs_refuse(int* first, int* second, int* counts, int n, int* assign, int ns, double* cost, int nc) {
  const int t = threadIdx.x, nthr = blockDim.x;
  for (int j = t; j < n; j += nthr) {
    first[j] = -1;
    if (second) second[j] = -1;
    counts[j] = 0;
  }
  for (int k = t; k < ns; k += nthr) assign[k] = -1;
  for (int j = t; j < nc; j += nthr) cost[j] = NAN;
}

// (mult stands behind the outputs: ahead of them, the unweighted kernel's argument loads were split, the later part stayed in
// flight into the pick loop and the loop waited for all its LDS reads at once: 4 % on rd_pick_kernel)
struct FsPickArgs {
  const double* D;                          // [count, S, S]
  int* selected;                            // [count, K]
  int* counts;                              // [count, K]
  int* assign;                              // [count, S]
  double* cost;                             // [count, K]
  const int* mult;                          // [count, S]; WEIGHTED only
  int S, K, ld, W;                         // ld: doubles between rows of the LDS copy; W: the ensemble (S where not WEIGHTED)
};

template <bool WEIGHTED, bool IN_LDS>
__device__ __forceinline__ void fs_pick(const FsPickArgs& a) {
  extern __shared__ double fs_mem[];
  const int S = a.S, K = a.K, t = threadIdx.x, nthr = blockDim.x;
  const FsLds l = fs_carve(fs_mem, S, WEIGHTED ? 2 : 1);
  double* m = l.m;
  int* near = l.arr;                                            // [S]
  int* mu = WEIGHTED ? near + S : nullptr;                      // [S]: the multiplicities
  const size_t c = blockIdx.x;
  const double* Dg = a.D + c * (size_t)S * S;
  const int ld = IN_LDS ? a.ld : S;
  const double* Dr = IN_LDS ? l.D : Dg;                         // what the picks read
  int bad = 0;
  if (WEIGHTED) {
    for (int k = t; k < S; k += nthr) mu[k] = a.mult[c * S + k];
    __syncthreads();
    int pos;
    bad = (!sg_census(mu, S, a.W, &pos) || K > pos) ? 1 : 0;    // (the same in every thread)
  }
  if (!bad) bad = fs_stage<IN_LDS>(Dg, l.D, mu, S, ld);
  for (int k = t; k < S; k += nthr) {
    m[k] = INFINITY;
    near[k] = -1;
  }
  if (__syncthreads_or(bad)) {                                  // refused: this origin alone
    fs_refuse(a.selected + c * K, nullptr, a.counts + c * K, K, a.assign + c * S, S, a.cost + c * K, K);
    return;
  }
  const bool candidate = t < S && (!WEIGHTED || mu[t] > 0);
  bool taken = !candidate;
  for (int p = 0; p < K; ++p) {
    double z = 0.0;
    if (candidate) {
      const double* col = Dr + t;
      for (int k = 0; k < S; ++k) {
        if (WEIGHTED) {
          const int w = mu[k];
          if (w > 0) z = fs_add_product(z, (double)w, fmin(m[k], col[(size_t)k * ld]));
        } else {
          z += fmin(m[k], col[(size_t)k * ld]);
        }
      }
    }
    double v = z;
    int idx = taken ? FS_MAX_S + t : t;
    fs_argmin(v, idx, l);
    if (t == 0) {
      l.pick[0] = idx;
      a.selected[c * K + p] = idx;
      a.cost[c * K + p] = v / (double)a.W;
    }
    __syncthreads();
    const int sel = l.pick[0];
    taken = taken || t == sel;
    fs_lower(l, near, Dr, ld, S, sel, p, mu, nullptr, 0);
    __syncthreads();                                            // m, near and pick are settled for the next pick
  }
  for (int k = t; k < S; k += nthr) a.assign[c * S + k] = near[k];
  for (int j = t; j < K; j += nthr) {
    int n = 0;
    for (int k = 0; k < S; ++k) n += near[k] == j ? (WEIGHTED ? mu[k] : 1) : 0;
    a.counts[c * K + j] = n;
  }
}

// Launches one workgroup per origin: IN_LDS where NI arrays of S ints and the copy of D fit, else FROM_MEMORY; a thread per
// candidate, at least four waves to bring D in.  a.ld is set here.  The guard belongs to the kernel pair.
template <auto IN_LDS, auto FROM_MEMORY, class Args>
int fs_launch(Args& a, int ni, long count, hipStream_t st) {
  static SgDynLds guard;
  const int S = a.S;
  a.ld = S | 1;                             // an odd number of doubles: a column read meets every bank pair once
  const size_t head = ((size_t)S + 16) * 8 + fs_head_ints(S, ni) * 4;
  const bool in_lds = head + (size_t)S * a.ld * 8 <= FS_LDS_BYTES;
  const size_t lds = in_lds ? head + (size_t)S * a.ld * 8 : head;
  int threads = (S + 63) & ~63;
  if (threads < FS_MIN_THREADS) threads = FS_MIN_THREADS;
  if (in_lds) {
    SG_TRY(sg_ensure_dyn_lds((const void*)IN_LDS, lds, guard));
    hipLaunchKernelGGL(IN_LDS, dim3((unsigned)count), dim3(threads), lds, st, a);
  } else {
    hipLaunchKernelGGL(FROM_MEMORY, dim3((unsigned)count), dim3(threads), lds, st, a);
  }
  SG_TRY(hipGetLastError());
  return 0;
}
