// The crossing counts of sampled paths: the one kernel behind stemgnn_scenario_events (events.hip) and stemgnn_weighted_events
// (weighted.hip), and its launcher.
//
// paths [count, S, H, M] fp32 -> counts int32 [count, 2 H + 1, M].  One workgroup per (origin, tile of C columns); C = 64 .. 1,
// a power of two: the smallest that covers M, halved until the tile's (2 H + 1) x C counters are within 32 KB.  Thread
// (g, c) = (t / C, t % C) owns the paths g, g + G, .. of column c (G = 256 / C; lanes along m: coalesced) and walks h in order
// with "crossed yet", the current run and the longest run in registers; every count is an integer add into the LDS tile, and
// the workgroup writes its tile's 2 H + 1 rows itself.
// WEIGHTED: path s stands mult[c, s] times in an ensemble of W paths.  The workgroup first brings its origin's S multiplicities
// into LDS (wt_present); a path adds its multiplicity where an unweighted one adds 1, a path of multiplicity 0 is never loaded,
// and the tile of an absent origin is -1.
// One launch, no allocation, no memset, no global atomics, only integer adds: the same bits on every run, capturable.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/stemgnn_hip.h"
#include "scenario_math.h"
#include "sg_host.h"

constexpr int EV_THREADS = 256;
constexpr int EV_MAX_H = 256;
constexpr int EV_LDS_BYTES = 32 * 1024;     // the tile of (2 H + 1) x C counters

struct EvArgs {
  const float* paths;                       // [count, S, H, M]
  const int* mult;                          // [count, S]; WEIGHTED only
  const double* thr;                        // [M]
  const double* mul;                        // [M] or NULL
  const double* add;
  int* counts;                              // [count, 2 H + 1, M]
  int S, H, M, C, tiles, above, min_run, W;
};

template <bool WEIGHTED>
static __global__ __launch_bounds__(EV_THREADS) void ev_kernel(const EvArgs a) {
  extern __shared__ int ev_lds[];                               // [2 H + 1][C]: step | first | run; WEIGHTED: then the multiplicities [S]
  const int S = a.S, H = a.H, M = a.M, C = a.C, t = threadIdx.x;
  const int G = EV_THREADS / C, g = t / C, c = t - g * C, R = 2 * H + 1;
  int* wm = ev_lds + R * C;
  const size_t o = blockIdx.x / (unsigned)a.tiles;
  const int tl = (int)(blockIdx.x - o * (unsigned)a.tiles);
  for (int i = t; i < R * C; i += EV_THREADS) ev_lds[i] = 0;
  bool ok = true;
  if (WEIGHTED) ok = wt_present(a.mult + o * S, S, a.W, wm);    // (its barrier also settles the zeroes)
  else __syncthreads();
  const int m = tl * C + c;
  if (ok && m < M) {
    const bool dn = a.mul != nullptr, above = a.above != 0;
    const double mu = dn ? a.mul[m] : 1.0, ad = dn ? a.add[m] : 0.0, th = a.thr[m];
    const size_t HM = (size_t)H * M;
    const float* src = a.paths + o * S * HM + m;
    for (int s = g; s < S; s += G) {
      const int w = WEIGHTED ? wm[s] : 1;
      if (w <= 0) continue;
      const float* p = src + (size_t)s * HM;
      int crossed = 0, cur = 0, best = 0;
#pragma unroll 4
      for (int h = 0; h < H; ++h) {
        const double v = sg_dn(p[(size_t)h * M], dn, mu, ad);
        const bool e = above ? v > th : v < th;                 // strict, so a NaN on either side is never in the event
        if (e) {
          atomicAdd(&ev_lds[h * C + c], w);
          if (!crossed) atomicAdd(&ev_lds[(H + h) * C + c], w);
        }
        crossed |= e ? 1 : 0;
        cur = e ? cur + 1 : 0;
        best = max(best, cur);
      }
      if (best >= a.min_run) atomicAdd(&ev_lds[2 * H * C + c], w);
    }
  }
  __syncthreads();
  int* dst = a.counts + o * R * M + (size_t)tl * C;
  for (int i = t; i < R * C; i += EV_THREADS) {
    const int k = i / C, cc = i - k * C;
    if (tl * C + cc < M) dst[(size_t)k * M + cc] = ok ? ev_lds[i] : -1;
  }
}

// chooses C, fills a's C and tiles, and launches; the entries have checked the pointers and the other sizes
template <bool WEIGHTED>
int ev_launch(EvArgs& a, long count, hipStream_t st) {
  const int S = a.S, H = a.H, M = a.M;
  if (H > EV_MAX_H || a.min_run < 1 || a.min_run > H || (a.above != 0 && a.above != 1)) return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)S * H * M) || !sg_fits_int((2ll * H + 1) * M)) return SG_EINVAL;
  int C = 1;
  while (C < 64 && C < M) C <<= 1;
  while (C > 1 && (size_t)(2 * H + 1) * C * sizeof(int) > (size_t)EV_LDS_BYTES) C >>= 1;
  a.C = C;
  a.tiles = sg_ceil_div(M, C);
  if (!sg_fits_int((long long)count * a.tiles)) return SG_EINVAL;
  const size_t lds = ((size_t)(2 * H + 1) * C + (WEIGHTED ? (size_t)S : 0)) * sizeof(int);
  hipLaunchKernelGGL(ev_kernel<WEIGHTED>, dim3((unsigned)(count * a.tiles)), dim3(EV_THREADS), lds, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}
