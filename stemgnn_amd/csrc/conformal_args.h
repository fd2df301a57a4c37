// The argument checks and the by-value row table shared by the conformal entries (conformal.hip) and the serving epilogue
// (quantile_serve.hip): one definition of what a valid (shape, pairs) is.
#pragma once

constexpr int CF_MAX_Q = 32, CF_MAX_P = 16;

struct CfRoles {                            // apply: 0 = copy, p + 1 = the low row of pair p, -(p + 1) = its high row
  signed char role[CF_MAX_Q];
};

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
