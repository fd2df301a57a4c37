// The two definitions that the draw of a scenario path (scenario.hip) and its inverse, the probability integral transform of
// the copula fit (copula.hip), must share to be inverses: the order of a forecast column and the uniform of a Philox word.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// v before w in the order of quantile_column.h (qc_less), ties left to the caller
__device__ inline bool sc_less(float v, float w) { return v < w || (v == v && w != w); }

// the uniform of a Philox word: exact in fp32, strictly inside (0, 1)
__device__ inline float sc_uniform(uint32_t w) { return __fmul_rn(__fadd_rn((float)(w >> 9), 0.5f), 1.1920928955078125e-07f); }
