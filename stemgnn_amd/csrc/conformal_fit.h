// The exact radix-select fit of the conformal offsets, in its only copy: the histogram kernels of both forms, the pick and the
// host loop of four passes.  conformal.hip runs it over every row (CfNoSeason); seasonal.hip runs it once per time-of-day
// bucket by handing it a season policy that says which rows a workgroup's bucket walks (DESIGN.md sections 5i, 5n).
//
// One pass = one histogram launch + one pick launch, for all pairs and all groups (and buckets) at once; the scores are
// recomputed from target / forecast on every pass (three coalesced reads per element), so the scratch holds histograms and the
// per-group state only -- no staged keys.  The per-group state (prefix of the key found so far, remaining rank) lives on the
// device.
//
// The histogram launch has two forms, chosen by the grouping:
//   * columns (per_node): a group's members are strided by N (or H * N).  target is read as a matrix [R, C] whose column is
//     the group (R = count, C = H * N with per_step; R = count * H, C = N without), consecutive lanes on consecutive
//     columns.  A workgroup owns a tile of 32 adjacent columns times a chunk of rows and keeps one 256-bin histogram per
//     column in LDS, laid out [bin][column] with a row pitch of 33 words: the 32 columns of one bin sit on 32 different banks.
//   * stream (pooled over the nodes): a group is count runs of L contiguous floats (L = N with per_step, H * N without).
//     Many workgroups per group, each over a chunk of the group's elements, with 16 interleaved copies of the 256-bin
//     histogram in LDS ([bin][copy], copy = lane & 15) so that the lanes of a wave whose scores share a bin -- the common
//     case: the top byte is sign and exponent -- do not serialise on one LDS address.
// Both add their non-zero LDS bins to the group's global histogram with integer atomics; the pick launch (one wave per
// (bucket, pair, group)) scans the 256 bins, narrows the prefix, and clears the bins again for the next pass.
//
// A season policy travels by value as the LAST kernel argument (empty for CfNoSeason, so the other arguments sit where they
// always sat) and answers, for a workgroup whose blockIdx.z is z:
//   pair(z)               the pair the workgroup counts for (z itself without a season; z mod P with one, z = s * P + p)
//   bucket(z)             whatever window() needs to know about the workgroup's bucket
//   walked(b, all, per)   how many rows (elements) the launch walks: `all` of them, or `per` for each of the bucket's own windows
//   window(b, i, h)       is step h of walked window i the bucket's?  (may replace i by the window it stands for)
// and, with a season, N: the nodes of a step, by which a column or an element of a run tells its step.
// Everything is in an unnamed namespace: each translation unit that includes this gets kernels of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "calibration_plan.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "devattr.h"
#include "sg_host.h"

namespace {

// CF_TILE, CF_PITCH, CF_COPIES, CF_THREADS and the chunk arithmetic of the host loop: calibration_plan.h

struct CfPairs {                            // travels by value in the kernel arguments
  int lo[CF_MAX_P], hi[CF_MAX_P];
  double cov[CF_MAX_P];
};

// no season: every row is walked, all of it is bucket 0, nothing about time is read
struct CfNoSeason {
  static constexpr bool seasoned = false;
  struct Bucket {};
  __device__ int pair(int z) const { return z; }
  __device__ Bucket bucket(int) const { return {}; }
  __device__ int walked(const Bucket&, int all, int) const { return all; }
  __device__ bool window(const Bucket&, int&, int) const { return true; }
};

// ---- column form ------------------------------------------------------------------------------------------------------
// grid (column tiles, row chunks, buckets * P).  Hr = rows of the matrix per window (1 or H); HN = H * N.  With a season a
// column tells the step when Hr == 1 (per_step: C = H * N), otherwise the row does (r mod Hr).
template <bool MASKED, class Season>
__global__ __launch_bounds__(CF_THREADS) void cf_hist_columns(const float* __restrict__ y, const float* __restrict__ f,
                                                              int R, int C, int Hr, int Q, int HN, CfPairs pairs, int d,
                                                              const uint32_t* __restrict__ prefix,
                                                              const uint32_t* __restrict__ krem, uint32_t* __restrict__ hist,
                                                              int rows_per_chunk, const Season sn) {
  __shared__ uint32_t h[256 * CF_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, z = blockIdx.z, p = sn.pair(z);
  const int c0 = blockIdx.x * CF_TILE;
  const int Wd = min(CF_TILE, C - c0);            // columns of this tile
  const int rpw = 64 / Wd;                        // rows one wave covers per iteration (>= 2)
  const int lr = lane / Wd, lc = lane - lr * Wd;
  for (int i = tid; i < 256 * CF_PITCH; i += CF_THREADS) h[i] = 0u;
  __syncthreads();
  const auto bk = sn.bucket(z);
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(sn.walked(bk, R, Hr), r0 + rows_per_chunk);
  const size_t g = (size_t)z * C + (size_t)(c0 + lc);
  bool live = lr < rpw;
  uint32_t pre = 0u;
  if (live && d > 0) {
    pre = prefix[g];
    live = krem[g] != 0u;                          // a group whose rank is beyond its size is finished (+inf)
  }
  if (live) {
    const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
    const int step = (CF_THREADS / 64) * rpw;
    int hcol = 0;
    if constexpr (Season::seasoned) hcol = Hr == 1 ? (c0 + lc) / sn.N : 0;
#pragma unroll 2
    for (int rw = r0 + wave * rpw + lr; rw < r1; rw += step) {
      const int iw = rw / Hr;                      // the walked window; i: the window it stands for
      int i = iw;
      if (!sn.window(bk, i, Hr == 1 ? hcol : rw - iw * Hr)) continue;   // another bucket's row: nothing is loaded
      const int r = rw + (i - iw) * Hr;
      const float yv = y[(size_t)r * C + c0 + lc];
      const size_t fb = (size_t)i * Q * HN + (size_t)(rw - iw * Hr) * C + c0 + lc;
      const float lo = f[fb + lo_off], hi = f[fb + hi_off];
      if (MASKED && yv != yv) continue;
      const uint32_t key = cf_key(lo, yv, hi);
      if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * CF_PITCH + lc], 1u);
    }
  }
  __syncthreads();
  // consecutive lanes take consecutive bins of one column: conflict-free LDS reads (pitch 33), contiguous global addresses
  for (int i = tid; i < 256 * Wd; i += CF_THREADS) {
    const int col = i >> 8, bin = i & 255;
    const uint32_t v = h[bin * CF_PITCH + col];
    if (v) atomicAdd(&hist[((size_t)z * C + c0 + col) * 256 + bin], v);
  }
}

// ---- stream form ------------------------------------------------------------------------------------------------------
// grid (chunks, G, buckets * P).  Group g = the L contiguous floats at offset g * L of every window's [H * N] slab; M =
// count * L.  With L = H * N (steps pooled) a run spans H steps and so several buckets: the step is the element's own.
template <bool MASKED, class Season>
__global__ __launch_bounds__(CF_THREADS) void cf_hist_stream(const float* __restrict__ y, const float* __restrict__ f, int M,
                                                             int L, int G, int Q, int HN, CfPairs pairs, int d,
                                                             const uint32_t* __restrict__ prefix,
                                                             const uint32_t* __restrict__ krem, uint32_t* __restrict__ hist,
                                                             int per_chunk, const Season sn) {
  __shared__ uint32_t h[256 * CF_COPIES];
  const int tid = threadIdx.x, g = blockIdx.y, z = blockIdx.z, p = sn.pair(z);
  const size_t pg = (size_t)z * G + g;
  uint32_t pre = 0u;
  if (d > 0) {
    if (krem[pg] == 0u) return;                    // uniform over the workgroup
    pre = prefix[pg];
  }
  for (int i = tid; i < 256 * CF_COPIES; i += CF_THREADS) h[i] = 0u;
  __syncthreads();
  const auto bk = sn.bucket(z);
  const int e0 = blockIdx.x * per_chunk, e1 = (int)min((long long)sn.walked(bk, M, L), (long long)e0 + per_chunk);
  const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
  const int copy = tid & (CF_COPIES - 1), base = g * L;
#pragma unroll 2
  for (int e = e0 + tid; e < e1; e += CF_THREADS) {
    int i = e / L;
    const int t = e - i * L;
    int hh = 0;
    if constexpr (Season::seasoned) hh = L == sn.N ? g : t / sn.N;   // per_step: the group is the step
    if (!sn.window(bk, i, hh)) continue;           // another bucket's sub-run: nothing is loaded
    const float yv = y[(size_t)i * HN + base + t];
    const size_t fb = (size_t)i * Q * HN + base + t;
    const float lo = f[fb + lo_off], hi = f[fb + hi_off];
    if (MASKED && yv != yv) continue;
    const uint32_t key = cf_key(lo, yv, hi);
    if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * CF_COPIES + copy], 1u);
  }
  __syncthreads();
  uint32_t v = 0u;
#pragma unroll
  for (int c = 0; c < CF_COPIES; ++c) v += h[tid * CF_COPIES + ((c + tid) & (CF_COPIES - 1))];
  if (v) atomicAdd(&hist[pg * 256 + tid], v);
}

// ---- pick: one wave per (bucket, pair, group), pg = (s * P + p) * G + g ---------------------------------------------------
// Lane l owns bins 4l .. 4l+3.  Pass 0 also learns m (the sum of all bins), writes counts and turns the coverage into the rank;
// a rank beyond m finishes the group with +inf.  The last pass writes the offset.  Every pass leaves the bins zero.
__global__ __launch_bounds__(CF_THREADS) void cf_pick(uint32_t* __restrict__ hist, uint32_t* __restrict__ prefix,
                                                      uint32_t* __restrict__ krem, int PG, int G, CfPairs pairs, int d,
                                                      float* __restrict__ offsets, long long* __restrict__ counts, int P) {
  const int lane = threadIdx.x & 63;
  const int pg = blockIdx.x * (CF_THREADS / 64) + (threadIdx.x >> 6);
  if (pg >= PG) return;                            // uniform over the wave
  uint4* bins = reinterpret_cast<uint4*>(hist + (size_t)pg * 256) + lane;
  const uint4 c = *bins;
  *bins = make_uint4(0u, 0u, 0u, 0u);
  const uint32_t incl = cf_wave_scan(c, lane);
  uint32_t k, pre;
  if (d == 0) {
    const long long m = (long long)__shfl(incl, 63, 64);
    const double kk = cf_rank(m, pairs.cov[(pg / G) % P]);
    const bool beyond = kk > (double)m;
    k = beyond ? 0u : (uint32_t)kk;
    pre = 0u;
    if (lane == 0) {
      counts[pg] = m;
      if (beyond) {
        offsets[pg] = __uint_as_float(CF_PINF_BITS);
        krem[pg] = 0u;
        prefix[pg] = 0u;
      }
    }
  } else {
    k = krem[pg];
    pre = prefix[pg];
  }
  if (k == 0u) return;
  uint32_t bin, before;
  if (lane != cf_wave_pick(c, incl, k, lane, bin, before)) return;
  pre |= bin << (24 - 8 * d);
  if (d == 3) {
    offsets[pg] = cf_unkey(pre);
  } else {
    prefix[pg] = pre;
    krem[pg] = k - before;
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------
// scratch: histograms [KP G 256] | prefix [KP G] | remaining rank [KP G], KP = buckets * P
inline size_t cf_fit_scratch_bytes(long long KP, size_t groups) { return (size_t)KP * groups * (256 + 2) * sizeof(uint32_t); }

// the pairs with their coverages, each of which must lie inside (0, 1)
inline bool cf_fit_pairs(int P, const int* lo_rows, const int* hi_rows, const double* coverage, CfPairs* pairs) {
  *pairs = CfPairs{};
  for (int p = 0; p < P; ++p) {
    if (!(coverage[p] > 0.0 && coverage[p] < 1.0)) return false;      // NaN fails both
    pairs->lo[p] = lo_rows[p];
    pairs->hi[p] = hi_rows[p];
    pairs->cov[p] = coverage[p];
  }
  return true;
}

// The zero fill and the four passes over KP = buckets * P tables of gr.groups() groups.  `rows` is the number of windows a
// workgroup walks (count without a season).  The caller has checked the shapes, KP * G < 2^29 (the pick's int indices), KP <=
// 65535 (grid.z) and, for the stream form, G <= 65535 (grid.y).
template <class Season>
int cf_fit_run(const float* target, const float* forecast, long count, long long rows, int Q, int H, int N, int P, int KP,
               const CfPairs& pairs, const CfGrouping& gr, bool per_node, bool masked, const Season& sn, void* scratch,
               float* offsets, long long* counts, hipStream_t st) {
  const int HN = H * N, G = (int)gr.groups();
  const long long PG = (long long)KP * G;
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
  uint32_t* prefix = hist + (size_t)PG * 256;
  uint32_t* krem = prefix + PG;
  SG_TRY(sg_zero_async(hist, (size_t)PG * 256 * sizeof(uint32_t), st));
  CfFitPlan pl;
  cf_fit_plan(rows, KP, gr, per_node, sg_num_cus(), &pl);
  for (int d = 0; d < 4; ++d) {
    if (per_node) {
      const int C = gr.Cc, Hr = gr.Hr, R = (int)(count * Hr);
      const dim3 grid((unsigned)pl.tiles, (unsigned)pl.launched, (unsigned)KP);
      auto kernel = masked ? cf_hist_columns<true, Season> : cf_hist_columns<false, Season>;
      hipLaunchKernelGGL(kernel, grid, dim3(CF_THREADS), 0, st, target, forecast, R, C, Hr, Q, HN, pairs, d, prefix, krem, hist,
                         pl.per_chunk, sn);
    } else {
      const int L = gr.L;
      const int M = (int)(count * L);
      const dim3 grid((unsigned)pl.launched, (unsigned)G, (unsigned)KP);
      auto kernel = masked ? cf_hist_stream<true, Season> : cf_hist_stream<false, Season>;
      hipLaunchKernelGGL(kernel, grid, dim3(CF_THREADS), 0, st, target, forecast, M, L, G, Q, HN, pairs, d, prefix, krem, hist,
                         pl.per_chunk, sn);
    }
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(cf_pick, dim3(pl.pick_blocks), dim3(CF_THREADS), 0, st, hist, prefix, krem,
                       (int)PG, G, pairs, d, offsets, counts, P);
    SG_TRY(hipGetLastError());
  }
  return 0;
}

}  // namespace
