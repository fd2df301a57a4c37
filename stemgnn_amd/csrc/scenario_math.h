// Device helpers that the scenario family (ensemble.hip, events.hip, weighted.hip, forward_select.h, path_events.h) must share
// to compute the same bits: the de-normalisation of a loaded value, the fixed-order workgroup sum and the census of a weighted
// set's multiplicities.
#pragma once
#include <hip/hip_runtime.h>

// v * mul + add in fp64, the product and the sum rounded separately
__device__ inline double sg_dn(float v, bool dn, double mu, double ad) {
  return dn ? __dadd_rn(__dmul_rn((double)v, mu), ad) : (double)v;
}

// v summed over the workgroup in a fixed order (a tree inside each wave, the waves in index order); every thread gets the sum
__device__ inline double sg_block_sum(double v, double* sh) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  const int nw = blockDim.x >> 6;
  __syncthreads();                                              // (sh may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
  for (int w = 0; w < nw; ++w) s += sh[w];
  return s;
}

// The census of n multiplicities in LDS (the same in every thread): true when none is negative and their sum is W; *pos counts
// the positive ones.
__device__ inline bool sg_census(const int* wm, int n, int W, int* pos) {
  long long sum = 0;
  int neg = 0, p = 0;
  for (int k = 0; k < n; ++k) {
    const int w = wm[k];
    neg |= w < 0 ? 1 : 0;
    p += w > 0 ? 1 : 0;
    sum += w;
  }
  *pos = p;
  return !neg && sum == (long long)W;
}

// The origin's K multiplicities go to wm (LDS); true when the origin is present.  Every thread calls it (one barrier).
__device__ inline bool wt_present(const int* mult, int K, int W, int* wm) {
  for (int k = threadIdx.x; k < K; k += blockDim.x) wm[k] = mult[k];
  __syncthreads();
  int pos;
  return sg_census(wm, K, W, &pos);
}
