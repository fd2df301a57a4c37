// Seasonal (Mondrian) conformal calibration: the offsets of conformal.hip kept per time-of-day bucket (include/stemgnn_hip.h:
// stemgnn_seasonal_* / stemgnn_quantile_store_seasonal).
//
// Every target has an integer time index t; step h of row i has t = o_i + h with o_i the row's origin (a device int64 [count],
// or origin0 + i, or -- the live store -- t_dev[0] + i).  bucket(t) = (u * K) / period with u = (t + phase) mod period in the
// floor sense.  Within a bucket everything is conformal.hip's definition: the key, the rank, the exact MSB-first radix select
// (conformal_select.h), the band widening (conformal_args.h).  Tables are [K, P, Hg, Ng], the bucket slowest, so one bucket's
// slice is exactly a table of stemgnn_conformal_fit and cf_widen is pointed at it.
//
// fit:   conformal.hip's structure -- a zero fill, then four passes of histogram launch + pick launch, scores recomputed per
//        pass, scratch = histograms [K P G 256] | prefix | remaining rank.  A histogram workgroup owns ONE bucket
//        (blockIdx.z = s * P + p): it walks its chunk of rows exactly as cf_hist_columns / cf_hist_stream do, works out the
//        element's u from (i, h) and skips what lies outside the bucket's range [u_lo, u_hi) of u BEFORE it loads target /
//        forecast, so the memory traffic stays that of the unseasoned fit; the K-fold walk costs integer work only.  With
//        consecutive origins the rows of a bucket come in runs of period / K every `period` rows, and the workgroup enumerates
//        them instead (DIRECT): 1 / K of the walk.  The LDS layouts are the unseasoned ones ([bin][column] pitch 33; 16
//        interleaved copies).  The pick is one wave per (s, p, g).
// apply: one streaming launch, a wave per (i, h) row segment: the bucket is worked out once per segment on the scalar unit,
//        the lanes then stream the Q runs of N floats (float4 when N % 4 == 0 and the buffers are 16-byte aligned).
// apply with rearrange / the live store: a column kernel in the form of quantile_serve.hip's (a thread owns its columns from
//        the first load to the last store, the column held in LDS words of its own, no barrier), the table slice chosen per
//        (window, h).
// Only vector stores, and integer atomicAdd on LDS / global histogram counters.
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

constexpr int SS_TILE = 32;                 // columns per workgroup (column form)
constexpr int SS_PITCH = SS_TILE + 1;       // LDS row pitch in words
constexpr int SS_COPIES = 16;               // histogram copies per workgroup (stream form)
constexpr int SS_THREADS = 256;
constexpr int SS_CHUNK = 4;                 // column kernel: rows whose global loads are in flight together
constexpr int SS_LDS_BYTES = 32 * 1024;     // column kernel: per workgroup, both planes
constexpr int SS_VEC_MAX_Q = 16;

struct SsPairs {                            // travels by value in the kernel arguments
  int lo[CF_MAX_P], hi[CF_MAX_P];
  double cov[CF_MAX_P];
};

// where a row's origin comes from, and the season; by value.  origin0 has been reduced into [0, period) by the host (the bucket
// depends on t mod period only), so origin0 + i + h stays far from any overflow.
struct SsTime {
  const long long* origins;                 // int64 [count], or NULL
  const long long* t_dev;                   // int64 [1] (the live store), or NULL
  long long origin0;
  uint32_t period, K, phase;
};

// u = (t + phase) mod period, floor sense; period < 2^31, phase < period
__host__ __device__ inline uint32_t ss_u(long long t, uint32_t period, uint32_t phase) {
  uint32_t r;
  if ((unsigned long long)t < (1ull << 31)) {
    r = (uint32_t)t % period;
  } else {
    long long q = t % (long long)period;
    if (q < 0) q += period;
    r = (uint32_t)q;
  }
  r += phase;                               // < 2^32
  return r >= period ? r - period : r;
}
// bucket of u: (u * K) / period; u * K < 2^47
__host__ __device__ inline uint32_t ss_bucket_of_u(uint32_t u, uint32_t period, uint32_t K) {
  const unsigned long long prod = (unsigned long long)u * K;
  return prod < (1ull << 32) ? (uint32_t)prod / period : (uint32_t)(prod / period);
}
__device__ inline long long ss_origin(const SsTime& tm, long long i) {
  if (tm.origins) return tm.origins[i];
  return (tm.t_dev ? tm.t_dev[0] : tm.origin0) + i;
}
__device__ inline uint32_t ss_bucket(const SsTime& tm, long long i, int h) {
  return ss_bucket_of_u(ss_u(ss_origin(tm, i) + h, tm.period, tm.phase), tm.period, tm.K);
}
// the u of bucket s are [ceil(s * period / K), ceil((s + 1) * period / K)): u K / period == s  <=>  s period <= u K < (s + 1) period
__device__ inline uint32_t ss_u_from(uint32_t s, uint32_t period, uint32_t K) {
  return (uint32_t)(((unsigned long long)s * period + K - 1) / K);
}

// DIRECT (consecutive origins, o_i = origin0 + i): the rows of bucket s at step h are runs of len = u_hi - u_lo rows, one run
// every `period` rows, so they are enumerated instead of found by skipping: virtual row v (run v / len, place v % len) is row
// first(h) - period + run * period + place, with first(h) in [0, period) the first row whose u is u_lo -- the run before it
// may straddle row 0.  Rows outside [0, count) are dropped.  dd = (u_lo - u(0, 0)) mod period.
struct SsDirect {
  int count, runs;                          // runs = count / period + 2 covers every run that meets [0, count)
};
__device__ inline long long ss_direct_row(int v, uint32_t len, uint32_t dd, int h, uint32_t period) {
  const uint32_t run = (uint32_t)v / len, place = (uint32_t)v - run * len;
  const uint32_t first = (dd + period - (uint32_t)h % period) % period;
  return (long long)first - (long long)period + (long long)run * period + place;
}

// ---- fit, column form ---------------------------------------------------------------------------------------------------
// grid (column tiles, row chunks, K * P), blockIdx.z = s * P + p.  The matrix [R, C] of cf_hist_columns; N tells a column's
// step when Hr == 1 (per_step: C = H * N), otherwise the step is the row's (r mod Hr).
template <bool MASKED, bool DIRECT>
__global__ __launch_bounds__(SS_THREADS) void ss_hist_columns(const float* __restrict__ y, const float* __restrict__ f, int R,
                                                              int C, int Hr, int N, int Q, int HN, int P, SsPairs pairs,
                                                              SsTime tm, SsDirect dr, int d,
                                                              const uint32_t* __restrict__ prefix,
                                                              const uint32_t* __restrict__ krem, uint32_t* __restrict__ hist,
                                                              int rows_per_chunk) {
  __shared__ uint32_t h[256 * SS_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int s = blockIdx.z / P, p = blockIdx.z - s * P;
  const int c0 = blockIdx.x * SS_TILE;
  const int Wd = min(SS_TILE, C - c0);
  const int rpw = 64 / Wd;
  const int lr = lane / Wd, lc = lane - lr * Wd;
  for (int i = tid; i < 256 * SS_PITCH; i += SS_THREADS) h[i] = 0u;
  __syncthreads();
  const uint32_t u_lo = ss_u_from(s, tm.period, tm.K), u_hi = ss_u_from(s + 1, tm.period, tm.K), len = u_hi - u_lo;
  const int Rw = DIRECT ? dr.runs * (int)len * Hr : R;     // rows to walk: the bucket's virtual rows, or all of them
  const int r0 = blockIdx.y * rows_per_chunk, r1 = min(Rw, r0 + rows_per_chunk);
  const size_t g = (size_t)blockIdx.z * C + (size_t)(c0 + lc);
  bool live = lr < rpw;
  uint32_t pre = 0u;
  if (live && d > 0) {
    pre = prefix[g];
    live = krem[g] != 0u;
  }
  if (live) {
    const uint32_t dd = (u_lo + tm.period - ss_u(tm.origin0, tm.period, tm.phase)) % tm.period;
    const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
    const int step = (SS_THREADS / 64) * rpw;
    const int hcol = Hr == 1 ? (c0 + lc) / N : 0;
#pragma unroll 2
    for (int rw = r0 + wave * rpw + lr; rw < r1; rw += step) {
      int i = rw / Hr;
      const int hr = rw - i * Hr;
      if (DIRECT) {
        const long long row = ss_direct_row(i, len, dd, Hr == 1 ? hcol : hr, tm.period);
        if (row < 0 || row >= dr.count) continue;
        i = (int)row;
      } else {
        const uint32_t u = ss_u(ss_origin(tm, i) + (Hr == 1 ? hcol : hr), tm.period, tm.phase);
        if (u < u_lo || u >= u_hi) continue;         // another bucket's row: nothing is loaded
      }
      const int r = i * Hr + hr;
      const float yv = y[(size_t)r * C + c0 + lc];
      const size_t fb = (size_t)i * Q * HN + (size_t)hr * C + c0 + lc;
      const float lo = f[fb + lo_off], hi = f[fb + hi_off];
      if (MASKED && yv != yv) continue;
      const uint32_t key = cf_key(lo, yv, hi);
      if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * SS_PITCH + lc], 1u);
    }
  }
  __syncthreads();
  for (int i = tid; i < 256 * Wd; i += SS_THREADS) {
    const int col = i >> 8, bin = i & 255;
    const uint32_t v = h[bin * SS_PITCH + col];
    if (v) atomicAdd(&hist[((size_t)blockIdx.z * C + c0 + col) * 256 + bin], v);
  }
}

// ---- fit, stream form ---------------------------------------------------------------------------------------------------
// grid (chunks, G, K * P).  Group g = the L contiguous floats at offset g * L of every window's slab; with L = H * N (steps
// pooled) a run spans H steps and so several buckets: the step, hence the bucket, is the element's own (t / N).
template <bool MASKED, bool DIRECT>
__global__ __launch_bounds__(SS_THREADS) void ss_hist_stream(const float* __restrict__ y, const float* __restrict__ f, int M,
                                                             int L, int G, int N, int Q, int HN, int P, SsPairs pairs,
                                                             SsTime tm, SsDirect dr, int d,
                                                             const uint32_t* __restrict__ prefix,
                                                             const uint32_t* __restrict__ krem, uint32_t* __restrict__ hist,
                                                             int per_chunk) {
  __shared__ uint32_t h[256 * SS_COPIES];
  const int tid = threadIdx.x, g = blockIdx.y;
  const int s = blockIdx.z / P, p = blockIdx.z - s * P;
  const size_t pg = (size_t)blockIdx.z * G + g;
  uint32_t pre = 0u;
  if (d > 0) {
    if (krem[pg] == 0u) return;                    // uniform over the workgroup
    pre = prefix[pg];
  }
  for (int i = tid; i < 256 * SS_COPIES; i += SS_THREADS) h[i] = 0u;
  __syncthreads();
  const uint32_t u_lo = ss_u_from(s, tm.period, tm.K), u_hi = ss_u_from(s + 1, tm.period, tm.K), len = u_hi - u_lo;
  const uint32_t dd = (u_lo + tm.period - ss_u(tm.origin0, tm.period, tm.phase)) % tm.period;
  const int Mw = DIRECT ? dr.runs * (int)len * L : M;      // elements to walk: of the bucket's virtual rows, or all
  const int e0 = blockIdx.x * per_chunk, e1 = (int)min((long long)Mw, (long long)e0 + per_chunk);
  const size_t lo_off = (size_t)pairs.lo[p] * HN, hi_off = (size_t)pairs.hi[p] * HN;
  const int copy = tid & (SS_COPIES - 1), base = g * L;
  const bool one_step = L == N;                    // per_step: the group is the step
#pragma unroll 2
  for (int e = e0 + tid; e < e1; e += SS_THREADS) {
    int i = e / L;
    const int t = e - i * L;
    const int hh = one_step ? g : t / N;
    if (DIRECT) {
      const long long row = ss_direct_row(i, len, dd, hh, tm.period);
      if (row < 0 || row >= dr.count) continue;
      i = (int)row;
    } else {
      const uint32_t u = ss_u(ss_origin(tm, i) + hh, tm.period, tm.phase);
      if (u < u_lo || u >= u_hi) continue;         // another bucket's sub-run: nothing is loaded
    }
    const float yv = y[(size_t)i * HN + base + t];
    const size_t fb = (size_t)i * Q * HN + base + t;
    const float lo = f[fb + lo_off], hi = f[fb + hi_off];
    if (MASKED && yv != yv) continue;
    const uint32_t key = cf_key(lo, yv, hi);
    if (cf_match(key, d, pre)) atomicAdd(&h[cf_bin(key, d) * SS_COPIES + copy], 1u);
  }
  __syncthreads();
  uint32_t v = 0u;
#pragma unroll
  for (int c = 0; c < SS_COPIES; ++c) v += h[tid * SS_COPIES + ((c + tid) & (SS_COPIES - 1))];
  if (v) atomicAdd(&hist[pg * 256 + tid], v);
}

// ---- pick: one wave per (bucket, pair, group); cf_pick with the coverage of pair (spg / G) mod P ------------------------------
__global__ __launch_bounds__(SS_THREADS) void ss_pick(uint32_t* __restrict__ hist, uint32_t* __restrict__ prefix,
                                                      uint32_t* __restrict__ krem, int SPG, int G, int P, SsPairs pairs, int d,
                                                      float* __restrict__ offsets, long long* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const int pg = blockIdx.x * (SS_THREADS / 64) + (threadIdx.x >> 6);
  if (pg >= SPG) return;                           // uniform over the wave
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

// ---- apply, streaming -----------------------------------------------------------------------------------------------------
// A wave per (i, h) row segment: its Q runs of N floats.  The segment index is made wave-uniform, so the origin load and the
// bucket arithmetic run once per segment on the scalar unit.  forecast and out may be the same buffer: a lane reads its own
// elements before it writes them.
template <int VEC>
__global__ __launch_bounds__(SS_THREADS) void ss_apply(const float* forecast, const float* __restrict__ offsets,
                                                       long long segments, int Q, int H, int N, CfRoles roles, int P, int Hg,
                                                       int Ng, SsTime tm, float* out) {
  const int lane = threadIdx.x & 63;
  const long long w0 = (long long)blockIdx.x * (SS_THREADS / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long stride = (long long)gridDim.x * (SS_THREADS / 64);
  const int per = N / VEC, items = Q * per;
  const size_t table = (size_t)P * Hg * Ng;
  for (long long seg = w0; seg < segments; seg += stride) {
    const long long i = seg / H;
    const int h = (int)(seg - i * H);
    const float* o = offsets + (size_t)ss_bucket(tm, i, h) * table;
    const size_t base = ((size_t)i * Q * H + h) * (size_t)N;
    for (int it = lane; it < items; it += 64) {
      const int q = it / per, n = (it - q * per) * VEC;
      const size_t e = base + (size_t)q * H * N + n;
      float v[VEC];
      cf_load<VEC>(forecast + e, v);
      cf_widen<VEC>(v, roles.role[q], o, Hg, Ng, h, n);
      cf_store<VEC>(out + e, v);
    }
  }
}

// ---- the column kernel: rearranged apply, and the live store ---------------------------------------------------------------
struct SsColArgs {                          // travels by value in the kernel arguments
  const float* src;                         // [count or B, Q, H, N]
  float* dst;                               // apply: out (may be src); store: out_forecast [capacity, Q, H, N]
  const float* target;                      // store only: [B, H, N]
  float* out_target;                        //             [capacity, H, N]
  const long long* pos;                     // store only: device int64[1]; NULL = apply
  const float* offsets;                     // [K, P, Hg, Ng]
  long long count, capacity;
  int Q, HN, N, rearrange, P, Hg, Ng, tvec;
  int cpb, wpb, col_blocks, win_blocks;     // the workgroup geometry of quantile_serve.hip's kernel
  CfRoles roles;
  SsTime tm;
};

__device__ inline bool ss_less(float v, float w) { return v < w || (v == v && w != w); }

template <int VEC>
__global__ __launch_bounds__(SS_THREADS) void ss_column_kernel(const SsColArgs a) {
  extern __shared__ float4 ss_lds[];
  const int T = blockDim.x, t = threadIdx.x, Q = a.Q, HN = a.HN;
  const bool store = a.pos != nullptr;      // uniform over the launch
  const long long p0 = store ? a.pos[0] : 0;
  if (store && blockIdx.y == 1) {           // the batch's targets, beside the forecast rows
    const int tper = a.tvec ? HN / 4 : HN;
    for (long long b = blockIdx.x; b < a.count; b += gridDim.x) {
      const long long row = p0 + b;
      if (row < 0 || row >= a.capacity) continue;
      const float* src = a.target + (size_t)b * HN;
      float* dst = a.out_target + (size_t)row * HN;
      for (int c = t; c < tper; c += T) {
        if (a.tvec)
          reinterpret_cast<float4*>(dst)[c] = reinterpret_cast<const float4*>(src)[c];
        else
          dst[c] = src[c];
      }
    }
    return;
  }
  const int tw = t / a.cpb, tc = t - tw * a.cpb;
  const int cb = blockIdx.x % a.col_blocks, ib = blockIdx.x / a.col_blocks;
  const int c = (cb * a.cpb + tc) * VEC;                    // h * N + n of the thread's first column, in every window
  if (tw >= a.wpb || c >= HN) return;                       // (no barrier below)
  const int h = c / a.N, n = c - h * a.N;
  float* A = reinterpret_cast<float*>(ss_lds) + t;          // plane A: the column as loaded; word (k * Q + q) * T
  float* B = A + (size_t)VEC * Q * T;                       // plane B: the column in order
  const size_t table = (size_t)a.P * a.Hg * a.Ng;
  const long long stride = (long long)a.win_blocks * a.wpb;
  for (long long i = (long long)ib * a.wpb + tw; i < a.count; i += stride) {
    const long long orow = p0 + i;
    if (store && (orow < 0 || orow >= a.capacity)) continue;
    const float* off = a.offsets + (size_t)ss_bucket(a.tm, i, h) * table;
    const float* s = a.src + (size_t)i * Q * HN + c;
    float* d = a.dst + (size_t)orow * Q * HN + c;
    // every row of the column is loaded before anything is stored (out may be the input)
    for (int q0 = 0; q0 < Q; q0 += SS_CHUNK) {
      float v[SS_CHUNK][VEC] = {};
#pragma unroll
      for (int j = 0; j < SS_CHUNK; ++j) {
        if (q0 + j < Q) cf_load<VEC>(s + (size_t)(q0 + j) * HN, v[j]);
      }
#pragma unroll
      for (int j = 0; j < SS_CHUNK; ++j) {
        if (q0 + j < Q) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) A[(k * Q + q0 + j) * T] = v[j][k];
        }
      }
    }
    const float* R = A;
    if (a.rearrange) {                      // by rank: torch.sort(dim=1, stable=True), the definition of stemgnn_quantile_finish
#pragma unroll 1
      for (int k = 0; k < VEC; ++k) {
        const float* Ak = A + k * Q * T;
        float* Bk = B + k * Q * T;
#pragma unroll 1
        for (int q = 0; q < Q; ++q) {
          const float v = Ak[q * T];
          int rank = 0;
          for (int j = 0; j < Q; ++j) {
            const float u = Ak[j * T];
            rank += (ss_less(u, v) || (!ss_less(v, u) && j < q)) ? 1 : 0;
          }
          Bk[rank * T] = v;
        }
      }
      R = B;
    }
#pragma unroll 1
    for (int r = 0; r < Q; ++r) {
      float v[VEC];
#pragma unroll
      for (int k = 0; k < VEC; ++k) v[k] = R[(k * Q + r) * T];
      cf_widen<VEC>(v, (int)a.roles.role[r], off, a.Hg, a.Ng, h, n);
      cf_store<VEC>(d + (size_t)r * HN, v);
    }
  }
}

int ss_column_launch(SsColArgs& a, long count, bool vec, hipStream_t st) {
  const bool store = a.pos != nullptr;
  const int VEC = vec ? 4 : 1;
  int T = SS_THREADS;
  while (T > 64 && (size_t)T * a.Q * VEC * 4 * 2 > (size_t)SS_LDS_BYTES) T -= 64;
  const size_t lds = (size_t)T * a.Q * VEC * 4 * 2;                      // <= 32 KB: Q <= 32 (VEC 1), Q <= 16 (VEC 4)
  const int per = a.HN / VEC;
  a.count = count;
  a.cpb = std::min(per, T);
  a.wpb = T / a.cpb;
  a.col_blocks = sg_ceil_div(per, a.cpb);
  const long long wins = ((long long)count + a.wpb - 1) / a.wpb;
  const long long cap = (long long)sg_num_cus() * 16;
  a.win_blocks = (int)std::max<long long>(1, std::min(wins, cap / a.col_blocks));
  const dim3 grid((unsigned)a.col_blocks * (unsigned)a.win_blocks, store ? 2 : 1);
  if (vec)
    hipLaunchKernelGGL(ss_column_kernel<4>, grid, dim3(T), lds, st, a);
  else
    hipLaunchKernelGGL(ss_column_kernel<1>, grid, dim3(T), lds, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---- host checks ----------------------------------------------------------------------------------------------------------
bool ss_season_ok(long long period, int K, long long phase) {
  return period >= 1 && period < (1ll << 31) && K >= 1 && (long long)K <= period && phase >= 0 && phase < period;
}
// the season and the sizes the kernels index with: P K <= 65535 (grid.z), K P G < 2^29 (the pick's int indices)
bool ss_sizes_ok(int H, int N, int P, int K, int per_step, int per_node) {
  if ((long long)P * K > 65535) return false;
  return (long long)K * P * (long long)cf_grouping(per_step, per_node, H, N).groups() < (1ll << 29);
}
long long ss_floor_mod(long long t, long long period) {
  long long r = t % period;
  return r < 0 ? r + period : r;
}
SsTime ss_time(const long long* origins, const long long* t_dev, long long origin0, long long period, int K, long long phase) {
  return {origins, t_dev, ss_floor_mod(origin0, period), (uint32_t)period, (uint32_t)K, (uint32_t)phase};
}

}  // namespace

extern "C" int stemgnn_season_bucket(long long t, long long period, int K, long long phase) {
  if (!ss_season_ok(period, K, phase)) return -1;
  return (int)ss_bucket_of_u(ss_u(t, (uint32_t)period, (uint32_t)phase), (uint32_t)period, (uint32_t)K);
}

extern "C" size_t stemgnn_seasonal_scratch_bytes(long count, int H, int N, int P, int K, int per_step, int per_node) {
  if (!cf_shapes_ok(count, 1, H, N, P) || K < 1 || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return 0;
  return (size_t)K * P * cf_grouping(per_step, per_node, H, N).groups() * (256 + 2) * sizeof(uint32_t);
}

extern "C" int stemgnn_seasonal_fit(const float* target, const float* forecast, const long long* origins, long long origin0,
                                    long count, int Q, int H, int N, int P, const int* lo_rows, const int* hi_rows,
                                    const double* coverage, int per_step, int per_node, int masked, long long period, int K,
                                    long long phase, void* scratch, float* offsets, long long* counts, void* stream) {
  if (!target || !forecast || !lo_rows || !hi_rows || !coverage || !scratch || !offsets || !counts) return SG_EINVAL;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, nullptr)) return SG_EINVAL;
  if (!ss_season_ok(period, K, phase) || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return SG_EINVAL;
  if (!sg_aligned16(scratch)) return SG_EINVAL;
  SsPairs pairs = {};
  for (int p = 0; p < P; ++p) {
    if (!(coverage[p] > 0.0 && coverage[p] < 1.0)) return SG_EINVAL;  // NaN fails both
    pairs.lo[p] = lo_rows[p];
    pairs.hi[p] = hi_rows[p];
    pairs.cov[p] = coverage[p];
  }
  hipStream_t st = (hipStream_t)stream;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  const int HN = H * N, G = (int)gr.groups(), KP = K * P;
  if (!per_node && G > 65535) return SG_EINVAL;                        // grid.y of the stream form
  const long long SPG = (long long)KP * G;
  const SsTime tm = ss_time(origins, nullptr, origin0, period, K, phase);
  uint32_t* hist = reinterpret_cast<uint32_t*>(scratch);
  uint32_t* prefix = hist + (size_t)SPG * 256;
  uint32_t* krem = prefix + SPG;
  SG_TRY(sg_zero_async(hist, (size_t)SPG * 256 * sizeof(uint32_t), st));
  const int blocks_wanted = 4 * sg_num_cus();
  // consecutive origins: a bucket's rows are enumerated when that walks fewer rows than skipping through all of them does
  // (runs * the longest bucket against count; measured in DESIGN 5n), otherwise -- and always for an origins tensor -- skipped
  const SsDirect dr = {(int)count, (int)(count / period) + 2};
  const long long walk = (long long)dr.runs * ((period + K - 1) / K);    // virtual rows of the longest bucket
  const bool direct = !origins && K >= 2 && 2 * walk <= (long long)count;
  const long long rows = direct ? walk : (long long)count;
  for (int d = 0; d < 4; ++d) {
    if (per_node) {
      const int C = gr.Cc, Hr = gr.Hr, R = (int)(count * Hr), Rw = (int)(rows * Hr);
      const int tiles = sg_ceil_div(C, SS_TILE);
      int chunks = sg_ceil_div(blocks_wanted, (long long)tiles * KP);
      chunks = std::max(1, std::min(std::min(chunks, sg_ceil_div(Rw, 64)), 65535));
      const int rows_per_chunk = sg_ceil_div(Rw, chunks);
      const dim3 grid((unsigned)tiles, (unsigned)sg_ceil_div(Rw, rows_per_chunk), (unsigned)KP);
      auto kernel = masked ? (direct ? ss_hist_columns<true, true> : ss_hist_columns<true, false>)
                           : (direct ? ss_hist_columns<false, true> : ss_hist_columns<false, false>);
      hipLaunchKernelGGL(kernel, grid, dim3(SS_THREADS), 0, st, target, forecast, R, C, Hr, N, Q, HN, P, pairs, tm, dr, d, prefix,
                         krem, hist, rows_per_chunk);
    } else {
      const int L = gr.L;
      const int M = (int)(count * L), Mw = (int)(rows * L);
      int chunks = sg_ceil_div(blocks_wanted, SPG);
      chunks = std::max(1, std::min(chunks, sg_ceil_div(Mw, 4 * SS_THREADS)));
      const int per_chunk = sg_ceil_div(Mw, chunks);
      const dim3 grid((unsigned)sg_ceil_div(Mw, per_chunk), (unsigned)G, (unsigned)KP);
      auto kernel = masked ? (direct ? ss_hist_stream<true, true> : ss_hist_stream<true, false>)
                           : (direct ? ss_hist_stream<false, true> : ss_hist_stream<false, false>);
      hipLaunchKernelGGL(kernel, grid, dim3(SS_THREADS), 0, st, target, forecast, M, L, G, N, Q, HN, P, pairs, tm, dr, d, prefix,
                         krem, hist, per_chunk);
    }
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(ss_pick, dim3((unsigned)sg_ceil_div(SPG, SS_THREADS / 64)), dim3(SS_THREADS), 0, st, hist, prefix, krem,
                       (int)SPG, G, P, pairs, d, offsets, counts);
    SG_TRY(hipGetLastError());
  }
  return 0;
}

extern "C" int stemgnn_seasonal_apply(const float* forecast, const float* offsets, const long long* origins,
                                      long long origin0, long count, int Q, int H, int N, int rearrange, int P,
                                      const int* lo_rows, const int* hi_rows, int per_step, int per_node, long long period,
                                      int K, long long phase, float* out, void* stream) {
  if (!forecast || !offsets || !lo_rows || !hi_rows || !out) return SG_EINVAL;
  CfRoles roles;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &roles)) return SG_EINVAL;
  if (!ss_season_ok(period, K, phase) || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return SG_EINVAL;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  const SsTime tm = ss_time(origins, nullptr, origin0, period, K, phase);
  const bool aligned = (N & 3) == 0 && sg_aligned16(forecast) && sg_aligned16(out);
  if (rearrange) {
    SsColArgs a = {};
    a.src = forecast;
    a.dst = out;
    a.offsets = offsets;
    a.Q = Q;
    a.HN = H * N;
    a.N = N;
    a.rearrange = 1;
    a.P = P;
    a.Hg = gr.Hg;
    a.Ng = gr.Ng;
    a.roles = roles;
    a.tm = tm;
    return ss_column_launch(a, count, aligned && Q <= SS_VEC_MAX_Q, (hipStream_t)stream);
  }
  const long long segments = (long long)count * H;
  const long long cap = (long long)sg_num_cus() * 8;
  const unsigned blocks = (unsigned)std::max<long long>(1, std::min(cap, (segments + SS_THREADS / 64 - 1) / (SS_THREADS / 64)));
  if (aligned)
    hipLaunchKernelGGL(ss_apply<4>, dim3(blocks), dim3(SS_THREADS), 0, (hipStream_t)stream, forecast, offsets, segments, Q, H, N,
                       roles, P, gr.Hg, gr.Ng, tm, out);
  else
    hipLaunchKernelGGL(ss_apply<1>, dim3(blocks), dim3(SS_THREADS), 0, (hipStream_t)stream, forecast, offsets, segments, Q, H, N,
                       roles, P, gr.Hg, gr.Ng, tm, out);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_quantile_store_seasonal(const float* steps, const float* target, const long long* pos,
                                               const long long* t_dev, int B, int Q, int H, int N, int rearrange,
                                               const float* offsets, int P, const int* lo_rows, const int* hi_rows,
                                               int per_step, int per_node, long long period, int K, long long phase,
                                               float* out_forecast, float* out_target, long capacity, void* stream) {
  if (!steps || !target || !pos || !t_dev || !offsets || !lo_rows || !hi_rows || !out_forecast || !out_target || capacity <= 0)
    return SG_EINVAL;
  CfRoles roles;
  if (!cf_shapes_ok(B, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &roles)) return SG_EINVAL;
  if (!ss_season_ok(period, K, phase) || !ss_sizes_ok(H, N, P, K, per_step, per_node)) return SG_EINVAL;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  SsColArgs a = {};
  a.src = steps;
  a.dst = out_forecast;
  a.target = target;
  a.out_target = out_target;
  a.pos = pos;
  a.offsets = offsets;
  a.capacity = capacity;
  a.Q = Q;
  a.HN = H * N;
  a.N = N;
  a.rearrange = rearrange != 0;
  a.P = P;
  a.Hg = gr.Hg;
  a.Ng = gr.Ng;
  a.tvec = (a.HN & 3) == 0 && sg_aligned16(target) && sg_aligned16(out_target);
  a.roles = roles;
  a.tm = ss_time(nullptr, t_dev, 0, period, K, phase);
  const bool vec = (N & 3) == 0 && Q <= SS_VEC_MAX_Q && sg_aligned16(steps) && sg_aligned16(out_forecast);
  return ss_column_launch(a, B, vec, (hipStream_t)stream);
}
