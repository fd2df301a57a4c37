// The argument checks, the by-value row table with its band widening, and the grouping geometry shared by the conformal
// entries (conformal.hip, seasonal.hip), the fit and the column kernel they share (conformal_fit.h, quantile_column.h), the
// serving epilogue (quantile_serve.hip), the adaptive update (aci.hip) and the anomaly scores (anomaly.hip): one definition of
// what a valid (shape, pairs) is, of what a calibrated row is, and of what a group is.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

constexpr int CF_MAX_Q = 32, CF_MAX_P = 16;

struct CfRoles {                            // apply: 0 = copy, p + 1 = the low row of pair p, -(p + 1) = its high row
  signed char role[CF_MAX_Q];
};

// apply: the VEC values at (h, n .. n + VEC - 1) of a row with role `role` moved by the offsets [P, Hg, Ng] of the row's pair,
// the low row down and the high row up: one fp32 subtract / add each.  (The caller reads the role: the serving epilogue has
// one only when it is given offsets.)
template <int VEC>
__device__ inline void cf_widen(float (&v)[VEC], int role, const float* offsets, int Hg, int Ng, int h, int n) {
  if (role == 0) return;
  const int p = (role > 0 ? role : -role) - 1;
  const float* o = offsets + ((size_t)p * Hg + (Hg > 1 ? h : 0)) * Ng;
#pragma unroll
  for (int j = 0; j < VEC; ++j) {
    const float off = o[Ng > 1 ? n + j : 0];
    v[j] = role > 0 ? __fsub_rn(v[j], off) : __fadd_rn(v[j], off);
  }
}

// The groups of one pair are a table [Hg, Ng] (H or 1 steps, N or 1 nodes) over the (h, n) positions of an [H, N] slab.
//   column form (per_node): a slab is Hr rows of Cc columns, the column is the group
//   stream form (pooled over the nodes): a slab is G runs of L contiguous floats, the run is the group
struct CfGrouping {
  int Hg, Ng, Cc, Hr, L, G;
  __host__ __device__ size_t groups() const { return (size_t)Hg * (size_t)Ng; }
  __host__ __device__ size_t group(int h, int n) const { return (size_t)(Hg > 1 ? h : 0) * Ng + (Ng > 1 ? n : 0); }
};
__host__ __device__ inline CfGrouping cf_grouping(int per_step, int per_node, int H, int N) {
  const int HN = H * N;
  return {per_step ? H : 1, per_node ? N : 1, per_step ? HN : N, per_step ? 1 : H, per_step ? N : HN, per_step ? H : 1};
}

inline bool cf_shapes_ok(long count, int Q, int H, int N, int P) {
  if (count <= 0 || Q <= 0 || H <= 0 || N <= 0 || P <= 0 || Q > CF_MAX_Q || P > CF_MAX_P) return false;
  return (long long)H * N < (1ll << 31) && (long long)count * ((long long)H * N) < (1ll << 31);
}
// cf_pairs_ok fills `roles` when asked
inline bool cf_pairs_ok(int Q, int P, const int* lo, const int* hi, CfRoles* roles) {
  CfRoles r = {};
  for (int p = 0; p < P; ++p) {
    if (!(0 <= lo[p] && lo[p] < hi[p] && hi[p] < Q)) return false;
    if (r.role[lo[p]] != 0 || r.role[hi[p]] != 0) return false;      // a row named twice
    r.role[lo[p]] = (signed char)(p + 1);
    r.role[hi[p]] = (signed char)-(p + 1);
  }
  if (roles) *roles = r;
  return true;
}
