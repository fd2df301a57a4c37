// The rank formula and the order-preserving key of the radix select, shared by the split-conformal fit (conformal.hip) and the
// adaptive update (aci.hip): one definition of which score is "the k-th smallest of m".
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

// the rank of the offset among m valid scores: two fp64 multiplies (no FMA can form) and a ceil; the factor keeps an exactly
// integral (m + 1) * c from being pushed to the next rank by the rounding of c.  Never below 1.
__host__ __device__ inline double cf_rank(long long m, double c) {
#ifdef __HIP_DEVICE_COMPILE__
  const double t = __dmul_rn((double)(m + 1), c);
  const double k = ceil(__dmul_rn(t, 1.0 - 1e-12));
#else
  const double t = (double)(m + 1) * c;
  const double k = ceil(t * (1.0 - 1e-12));
#endif
  return k < 1.0 ? 1.0 : k;
}

// order-preserving key of a score: NaN -> +inf, -0 -> +0, then the sign-flip transform
__device__ inline uint32_t cf_key(float lo, float y, float hi) {
  const float a = __fsub_rn(lo, y), b = __fsub_rn(y, hi);
  uint32_t u = __float_as_uint(a > b ? a : b);
  if (a != a || b != b) u = 0x7f800000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float cf_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// does the key belong to what pass `d` still looks at (its bits above the pass's byte equal the prefix), and in which bin
__device__ inline bool cf_match(uint32_t key, int d, uint32_t prefix) {
  return d == 0 || (key >> (32 - 8 * d)) == (prefix >> (32 - 8 * d));
}
__device__ inline uint32_t cf_bin(uint32_t key, int d) { return (key >> (24 - 8 * d)) & 255u; }
