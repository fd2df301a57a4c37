// Split-conformal calibration of quantile bands (include/stemgnn_hip.h: stemgnn_conformal_*).
//
// fit:   for every pair p of quantile rows (lo, hi) and every group g of (h, n) positions, the k-th smallest of the scores
//            s = max(f_lo - y, y - f_hi)                          (fp32; NaN counts as +inf)
//        with k = ceil((m + 1) * c * (1 - 1e-12)) of the group's m valid scores: an exact MSB-first radix SELECT on the
//        order-preserving 32-bit key of s, four passes of 8 bits.  No sort, no floating-point atomics; the only atomics are
//        integer histogram counts, which are exact in any order, so the result is the same bits on every run.
// apply: out_lo = f_lo - off, out_hi = f_hi + off, every other row copied; one streaming kernel.
//
// One pass = one histogram launch + one pick launch, for all P pairs and all groups at once; the scores are recomputed from
// target / forecast on every pass (three coalesced reads per element), so the scratch holds histograms and the per-group state
// only -- no staged keys.  The per-group state (prefix of the key found so far, remaining rank) lives on the device.
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
// (pair, group)) scans the 256 bins, narrows the prefix, and clears the bins again for the next pass.
// The key, the wave pick and the vector load / store live in conformal_select.h, the band widening and the grouping geometry in
// conformal_args.h: aci.hip, anomaly.hip and quantile_serve.hip use the same definitions.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "devattr.h"
#include "sg_host.h"

namespace {

constexpr int CF_TILE = 32;                 // columns per workgroup (column form)
constexpr int CF_PITCH = CF_TILE + 1;       // LDS row pitch in words
constexpr int CF_COPIES = 16;               // histogram copies per workgroup (stream form)
constexpr int CF_THREADS = 256;

struct CfPairs {                            // travels by value in the kernel arguments
  int lo[CF_MAX_P], hi[CF_MAX_P];
  double cov[CF_MAX_P];
};

// (cf_rank, cf_key / cf_unkey, cf_match, cf_bin, the wave pick, cf_load / cf_store: conformal_select.h;
//  cf_widen, cf_grouping: conformal_args.h -- shared with quantile_serve.hip, aci.hip and anomaly.hip)

// ---- column form ------------------------------------------------------------------------------------------------------
// grid (column tiles, row chunks, P).  Hr = rows of the matrix per window (1 or H); HN = H * N.
template <bool MASKED>
__global__ __launch_bounds__(CF_THREADS) void cf_hist_columns(const float* __restrict__ y, const float* __restrict__ f,
                                                              int R, int C, int Hr, int Q, int HN, CfPairs pairs, int d,
                                                              const uint32_t* __restrict__ prefix,
                                                              const uint32_t* __restrict__ krem, uint32_t* __restrict__ hist,
                                                              int rows_per_chunk) {
  __shared__ uint32_t h[256 * CF_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = blockIdx.z;
  const int c0 = blockIdx.x * CF_TILE;
  const int Wd = min(CF_TILE, C - c0);            // columns of this tile
  const int rpw = 64 / Wd;                        // rows one wave covers per iteration (>= 2)
  const int lr = lane / Wd, lc = lane - lr * Wd;
  for (int i = tid; i < 256 * CF_PITCH; i += CF_THREADS) h[i] = 0u;
  __syncthreads();
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(R, r0 + rows_per_chunk);
  const size_t g = (size_t)p * C + (size_t)(c0 + lc);
  bool live = lr < rpw;
  uint32_t pre = 0u;
  if (live && d > 0) {
    pre = prefix[g];
    live = krem[g] != 0u;                          // a group whose rank is beyond its size is finished (+inf)
  }
  if (live) {
    const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
    const int step = (CF_THREADS / 64) * rpw;
#pragma unroll 2
    for (int r = r0 + wave * rpw + lr; r < r1; r += step) {
      const int i = r / Hr;
      const float yv = y[(size_t)r * C + c0 + lc];
      const size_t fb = (size_t)i * Q * HN + (size_t)(r - i * Hr) * C + c0 + lc;
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
    if (v) atomicAdd(&hist[((size_t)p * C + c0 + col) * 256 + bin], v);
  }
}

// ---- stream form ------------------------------------------------------------------------------------------------------
// grid (chunks, G, P).  Group g = the L contiguous floats at offset g * L of every window's [H * N] slab; M = count * L.
template <bool MASKED>
__global__ __launch_bounds__(CF_THREADS) void cf_hist_stream(const float* __restrict__ y, const float* __restrict__ f, int M,
                                                             int L, int G, int Q, int HN, CfPairs pairs, int d,
                                                             const uint32_t* __restrict__ prefix,
                                                             const uint32_t* __restrict__ krem, uint32_t* __restrict__ hist,
                                                             int per_chunk) {
  __shared__ uint32_t h[256 * CF_COPIES];
  const int tid = threadIdx.x, g = blockIdx.y, p = blockIdx.z;
  const size_t pg = (size_t)p * G + g;
  uint32_t pre = 0u;
  if (d > 0) {
    if (krem[pg] == 0u) return;                    // uniform over the workgroup
    pre = prefix[pg];
  }
  for (int i = tid; i < 256 * CF_COPIES; i += CF_THREADS) h[i] = 0u;
  __syncthreads();
  const int e0 = blockIdx.x * per_chunk, e1 = (int)min((long long)M, (long long)e0 + per_chunk);
  const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
  const int copy = tid & (CF_COPIES - 1), base = g * L;
#pragma unroll 2
  for (int e = e0 + tid; e < e1; e += CF_THREADS) {
    const int i = e / L, t = e - i * L;
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

// ---- pick: one wave per (pair, group) -----------------------------------------------------------------------------------
// Lane l owns bins 4l .. 4l+3.  Pass 0 also learns m (the sum of all bins), writes counts and turns the coverage into the rank;
// a rank beyond m finishes the group with +inf.  The last pass writes the offset.  Every pass leaves the bins zero.
__global__ __launch_bounds__(CF_THREADS) void cf_pick(uint32_t* __restrict__ hist, uint32_t* __restrict__ prefix,
                                                      uint32_t* __restrict__ krem, int PG, int G, CfPairs pairs, int d,
                                                      float* __restrict__ offsets, long long* __restrict__ counts) {
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
    const double kk = cf_rank(m, pairs.cov[pg / G]);
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

// ---- apply ------------------------------------------------------------------------------------------------------------
// VEC: four consecutive n per thread (N % 4 == 0, 16-byte aligned pointers).  forecast and out may be the same buffer: every
// thread reads its own elements before it writes them.
template <int VEC>
__global__ __launch_bounds__(CF_THREADS) void cf_apply(const float* forecast, const float* __restrict__ offsets, size_t total,
                                                       int Q, int H, int N, CfRoles roles, int Hg, int Ng, float* out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total / VEC; i += stride) {
    const size_t e = i * VEC, row = e / (size_t)N;
    const int n = (int)(e - row * N), h = (int)(row % (size_t)H), q = (int)((row / (size_t)H) % (size_t)Q);
    float v[VEC];
    cf_load<VEC>(forecast + e, v);
    cf_widen<VEC>(v, roles.role[q], offsets, Hg, Ng, h, n);
    cf_store<VEC>(out + e, v);
  }
}

// (the shape and pair checks shared by fit and apply: conformal_args.h)
}  // namespace

extern "C" long stemgnn_conformal_rank(long m, double coverage) { return (long)cf_rank((long long)m, coverage); }

extern "C" size_t stemgnn_conformal_scratch_bytes(long count, int H, int N, int P, int per_step, int per_node) {
  if (!cf_shapes_ok(count, 1, H, N, P)) return 0;
  return (size_t)P * cf_grouping(per_step, per_node, H, N).groups() * (256 + 2) * sizeof(uint32_t);               // histograms | prefix | remaining rank
}

extern "C" int stemgnn_conformal_fit(const float* target, const float* forecast, long count, int Q, int H, int N, int P,
                                     const int* lo_rows, const int* hi_rows, const double* coverage, int per_step,
                                     int per_node, int masked, void* scratch, float* offsets, long long* counts,
                                     void* stream) {
  if (!target || !forecast || !lo_rows || !hi_rows || !coverage || !scratch || !offsets || !counts) return SG_EINVAL;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, nullptr)) return SG_EINVAL;
  if (!sg_aligned16(scratch)) return SG_EINVAL;
  CfPairs pairs = {};
  for (int p = 0; p < P; ++p) {
    if (!(coverage[p] > 0.0 && coverage[p] < 1.0)) return SG_EINVAL;  // NaN fails both
    pairs.lo[p] = lo_rows[p];
    pairs.hi[p] = hi_rows[p];
    pairs.cov[p] = coverage[p];
  }
  hipStream_t st = (hipStream_t)stream;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  const int HN = H * N, G = (int)gr.groups();
  const long long PG = (long long)P * G;
  if (PG >= (1ll << 31) / 4) return SG_EINVAL;                         // the pick kernel's int indices
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
  uint32_t* prefix = hist + (size_t)PG * 256;
  uint32_t* krem = prefix + PG;
  SG_TRY(sg_zero_async(hist, (size_t)PG * 256 * sizeof(uint32_t), st));
  const int blocks_wanted = 4 * sg_num_cus();
  for (int d = 0; d < 4; ++d) {
    if (per_node) {
      const int C = gr.Cc, Hr = gr.Hr, R = (int)(count * Hr);
      const int tiles = sg_ceil_div(C, CF_TILE);
      int chunks = sg_ceil_div(blocks_wanted, (long long)tiles * P);
      chunks = std::max(1, std::min(std::min(chunks, sg_ceil_div(R, 64)), 65535));
      const int rows_per_chunk = sg_ceil_div(R, chunks);
      const dim3 grid((unsigned)tiles, (unsigned)sg_ceil_div(R, rows_per_chunk), (unsigned)P);
      if (masked)
        hipLaunchKernelGGL(cf_hist_columns<true>, grid, dim3(CF_THREADS), 0, st, target, forecast, R, C, Hr, Q, HN, pairs, d,
                           prefix, krem, hist, rows_per_chunk);
      else
        hipLaunchKernelGGL(cf_hist_columns<false>, grid, dim3(CF_THREADS), 0, st, target, forecast, R, C, Hr, Q, HN, pairs, d,
                           prefix, krem, hist, rows_per_chunk);
    } else {
      const int L = gr.L;
      const int M = (int)(count * L);
      if (G > 65535) return SG_EINVAL;
      int chunks = sg_ceil_div(blocks_wanted, PG);
      chunks = std::max(1, std::min(chunks, sg_ceil_div(M, 4 * CF_THREADS)));
      const int per_chunk = sg_ceil_div(M, chunks);
      const dim3 grid((unsigned)sg_ceil_div(M, per_chunk), (unsigned)G, (unsigned)P);
      if (masked)
        hipLaunchKernelGGL(cf_hist_stream<true>, grid, dim3(CF_THREADS), 0, st, target, forecast, M, L, G, Q, HN, pairs, d,
                           prefix, krem, hist, per_chunk);
      else
        hipLaunchKernelGGL(cf_hist_stream<false>, grid, dim3(CF_THREADS), 0, st, target, forecast, M, L, G, Q, HN, pairs, d,
                           prefix, krem, hist, per_chunk);
    }
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(cf_pick, dim3((unsigned)sg_ceil_div(PG, CF_THREADS / 64)), dim3(CF_THREADS), 0, st, hist, prefix, krem,
                       (int)PG, G, pairs, d, offsets, counts);
    SG_TRY(hipGetLastError());
  }
  return 0;
}

extern "C" int stemgnn_conformal_apply(const float* forecast, const float* offsets, long count, int Q, int H, int N, int P,
                                       const int* lo_rows, const int* hi_rows, int per_step, int per_node, float* out,
                                       void* stream) {
  if (!forecast || !offsets || !lo_rows || !hi_rows || !out) return SG_EINVAL;
  CfRoles roles;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &roles)) return SG_EINVAL;
  const size_t total = (size_t)count * Q * H * N;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  const bool vec = (N & 3) == 0 && sg_aligned16(forecast) && sg_aligned16(out);
  const size_t items = vec ? total / 4 : total;
  const size_t cap = (size_t)sg_num_cus() * 8;
  const unsigned blocks = (unsigned)std::max<size_t>(1, std::min(cap, (items + CF_THREADS - 1) / CF_THREADS));
  if (vec)
    hipLaunchKernelGGL(cf_apply<4>, dim3(blocks), dim3(CF_THREADS), 0, (hipStream_t)stream, forecast, offsets, total, Q, H, N,
                       roles, gr.Hg, gr.Ng, out);
  else
    hipLaunchKernelGGL(cf_apply<1>, dim3(blocks), dim3(CF_THREADS), 0, (hipStream_t)stream, forecast, offsets, total, Q, H, N,
                       roles, gr.Hg, gr.Ng, out);
  SG_TRY(hipGetLastError());
  return 0;
}
