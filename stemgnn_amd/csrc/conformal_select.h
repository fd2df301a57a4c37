// The device primitives of the serving kernels (conformal_fit.h, quantile_column.h, conformal.hip, seasonal.hip, live.hip,
// aci.hip, anomaly.hip): the rank formula, the order-preserving key and the wave pick of the radix select -- one definition of
// which score is "the k-th smallest of m" -- the float4-or-scalar load / store behind every VEC template, and the special bit
// patterns.  The select's kernels themselves are conformal_fit.h.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

constexpr uint32_t CF_NAN_BITS = 0x7fc00000u;     // the quiet NaN torch writes for float("nan"): an absent score or reading
constexpr uint32_t CF_PINF_BITS = 0x7f800000u, CF_NINF_BITS = 0xff800000u;
constexpr uint32_t CF_KEY_ABSENT = 0xffffffffu;   // above every key: key(+inf) = 0xff800000

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

// order-preserving key of a score that is not NaN (a stored NaN means absent and is skipped by the caller): -0 -> +0 (a
// computed score cannot be -0 after cf_unkey, but a loaded state may hold one), then the sign-flip transform
__device__ inline uint32_t cf_score_key(float s) {
  uint32_t u = __float_as_uint(s);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the key of the score of (lo, y, hi): NaN -> +inf
__device__ inline uint32_t cf_key(float lo, float y, float hi) {
  const float a = __fsub_rn(lo, y), b = __fsub_rn(y, hi);
  const float s = a > b ? a : b;
  return cf_score_key((a != a || b != b) ? __uint_as_float(CF_PINF_BITS) : s);
}
__device__ inline float cf_unkey(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }

// does the key belong to what pass `d` still looks at (its bits above the pass's byte equal the prefix), and in which bin
__device__ inline bool cf_match(uint32_t key, int d, uint32_t prefix) {
  return d == 0 || (key >> (32 - 8 * d)) == (prefix >> (32 - 8 * d));
}
__device__ inline uint32_t cf_bin(uint32_t key, int d) { return (key >> (24 - 8 * d)) & 255u; }

// The pick of one pass, by ONE wave: lane l holds the counts c of bins 4l .. 4l+3.  cf_wave_scan gives the lane's inclusive
// sum (lane 63: all 256 bins); cf_wave_pick finds the bin that holds the k-th smallest (k >= 1) and returns the lane that
// owns it, in which `bin` and `before` (the count of the bins below it) are set, or -1 when k is beyond the total.
__device__ inline uint32_t cf_wave_scan(const uint4& c, int lane) {
  uint32_t incl = c.x + c.y + c.z + c.w;
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const uint32_t up = __shfl_up(incl, s, 64);
    if (lane >= s) incl += up;
  }
  return incl;
}
__device__ inline int cf_wave_pick(const uint4& c, uint32_t incl, uint32_t k, int lane, uint32_t& bin, uint32_t& before) {
  const unsigned long long reached = __ballot(incl >= k);
  if (reached == 0ull) return -1;
  const int at = __ffsll((long long)reached) - 1;
  if (lane != at) return at;
  before = incl - (c.x + c.y + c.z + c.w);
  bin = 4u * lane;
  if (before + c.x < k) {
    before += c.x; ++bin;
    if (before + c.y < k) {
      before += c.y; ++bin;
      if (before + c.z < k) { before += c.z; ++bin; }
    }
  }
  return at;
}

// VEC consecutive floats: one 16-byte access (VEC = 4, the host checked the alignment) or a scalar one (VEC = 1)
template <int VEC>
__device__ inline void cf_load(const float* p, float (&v)[VEC]) {
  if constexpr (VEC == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[0];
  }
}
template <int VEC>
__device__ inline void cf_store(float* p, const float (&v)[VEC]) {
  if constexpr (VEC == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    p[0] = v[0];
}
