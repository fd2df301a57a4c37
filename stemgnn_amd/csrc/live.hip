// Live forecasting: the ingest side of a stream (include/stemgnn_hip.h: stemgnn_live_push / stemgnn_ring_gather /
// stemgnn_live_head).
//
// A ring is [C, N] fp32; the row with absolute index tau (0 = the first row ever pushed) lives in slot tau mod C.  ring_x holds
// what ForecastDataset.data holds (imputed, normalised), ring_y what ForecastDataset.target holds (NaN at missing readings).
// The number of rows pushed so far is a device word t (int64): captured replays read it from memory.  Nothing here does a
// read-modify-write of it: a push is handed the host's own count t0 by value and one thread stores t0 + K.
//
// push: forward fill is a sequential dependence along time, so one thread owns a column and walks its K rows; lanes run along
// n, every row access of a wave is one coalesced run.  The normalisation is sg_normalize_kernel's expression (csrc/data.hip):
// IEEE fp64 subtract and divide by intrinsics (no contraction), optional clip, one rounding to fp32.
// gather: one workgroup per (row, b), a row is one coalesced N-float copy -- 16-byte accesses when the host found N % 4 == 0
// and both buffers 16-byte aligned (a plain float4 copy: nothing is unpacked, so it does not go through cf_load / cf_store).  A
// window that is not (or no longer) in the ring comes back as NaN rows: CF_NAN_BITS of conformal_select.h, the quiet NaN torch
// writes for float("nan"), as in ring_y.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "conformal_select.h"
#include "serving_plan.h"
#include "sg_host.h"

namespace {

// (LV_PUSH_THREADS and the gather's thread classes: serving_plan.h)
__global__ __launch_bounds__(LV_PUSH_THREADS) void lv_push_kernel(
    const double* __restrict__ raw, int K, int N, long long t0, const double* __restrict__ sub,
    const double* __restrict__ div, int clip01, double missing, int has_missing, double* __restrict__ last,
    float* __restrict__ ring_x, float* __restrict__ ring_y, int C, long long* __restrict__ t_dev) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n < N) {
    const double s = sub[n], d = div[n];
    double lv = last[n];
    const int k0 = K > C ? K - C : 0;               // rows before k0 would be overwritten by this very call: fill state only
    int slot = (int)((t0 + k0) % C);
    const float nanf32 = __uint_as_float(CF_NAN_BITS);
    for (int k = 0; k < K; ++k) {
      const double r = raw[(size_t)k * N + n];
      const bool miss = r != r || (has_missing && r == missing);
      if (!miss) lv = r;
      if (k >= k0) {
        double v = __ddiv_rn(__dsub_rn(lv, s), d);
        if (clip01) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);      // np.clip: NaN passes through
        const float f = (float)v;
        ring_x[(size_t)slot * N + n] = f;
        ring_y[(size_t)slot * N + n] = miss ? nanf32 : f;
        slot = slot + 1 == C ? 0 : slot + 1;
      }
    }
    last[n] = lv;
  }
  if (n == 0) t_dev[0] = t0 + K;                    // a plain store of the host's count: nothing reads the old value
}

// out[b, l, :] = ring[(s_b + l) mod C, :]; s_b = starts[b], or t - back without starts.  Not in the ring (s_b < 0, rows not yet
// pushed, rows already overwritten): NaN rows, bit 0 of *status.
template <bool VEC>
__global__ void lv_gather_kernel(const float* __restrict__ ring, int C, int N, const long long* __restrict__ starts,
                                 const long long* __restrict__ t_dev, int back, int L, float* __restrict__ out,
                                 int* __restrict__ status) {
  const int l = blockIdx.x, b = blockIdx.y;
  const long long t = t_dev[0];
  const long long s = starts ? starts[b] : t - back;
  const bool ok = s >= 0 && s + L <= t && s >= t - C;
  if (!ok && l == 0 && threadIdx.x == 0 && status) status[0] |= 1;      // every writer sets the same bit: no atomic needed
  const int slot = ok ? (int)((s + l) % C) : 0;
  const float* src = ring + (size_t)slot * N;
  float* dst = out + ((size_t)b * L + l) * N;
  const float nanf32 = __uint_as_float(CF_NAN_BITS);
  if (VEC) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = threadIdx.x; i < N / 4; i += blockDim.x) d4[i] = ok ? s4[i] : make_float4(nanf32, nanf32, nanf32, nanf32);
  } else {
    for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = ok ? src[i] : nanf32;
  }
}

__global__ void lv_head_kernel(const long long* __restrict__ t_dev, long long history, long long* __restrict__ pos,
                               long long* __restrict__ origins) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const long long t = t_dev[0];
    long long p = t % history;
    if (p < 0) p += history;                        // (t is a row count: never negative; the slot stays inside the slab anyway)
    pos[0] = p;
    origins[p] = t;
  }
}

}  // namespace

extern "C" int stemgnn_live_push(const double* raw, int K, int N, long long t0, const double* sub, const double* div,
                                 int clip01, double missing, int has_missing, double* last, float* ring_x, float* ring_y,
                                 int C, long long* t_dev, void* stream) {
  if (!raw || !sub || !div || !last || !ring_x || !ring_y || !t_dev) return SG_EINVAL;
  LvPushPlan pl;
  if (t0 < 0 || !lv_push_plan(K, N, C, &pl)) return SG_EINVAL;
  hipLaunchKernelGGL(lv_push_kernel, dim3(pl.blocks), dim3(pl.threads), 0, (hipStream_t)stream, raw, K, N, t0, sub, div,
                     clip01, missing, has_missing, last, ring_x, ring_y, C, t_dev);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_ring_gather(const float* ring, int C, int N, const long long* starts, const long long* t_dev, int back,
                                   int B, int L, float* out, int* status, void* stream) {
  if (!ring || !t_dev || !out) return SG_EINVAL;
  LvGatherPlan pl;
  if (back < 0 || back > C || (!starts && B != 1)) return SG_EINVAL;
  if (!lv_gather_plan(C, N, B, L, sg_aligned16(ring) && sg_aligned16(out), &pl)) return SG_EINVAL;
  const int threads = pl.threads;
  const dim3 grid((unsigned)L, (unsigned)B);
  if (pl.vec == 4)
    hipLaunchKernelGGL(lv_gather_kernel<true>, grid, dim3(threads), 0, (hipStream_t)stream, ring, C, N, starts, t_dev, back, L,
                       out, status);
  else
    hipLaunchKernelGGL(lv_gather_kernel<false>, grid, dim3(threads), 0, (hipStream_t)stream, ring, C, N, starts, t_dev, back,
                       L, out, status);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_live_head(const long long* t_dev, long history, long long* pos, long long* origins, void* stream) {
  if (!t_dev || !pos || !origins || history <= 0) return SG_EINVAL;
  hipLaunchKernelGGL(lv_head_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, t_dev, (long long)history, pos, origins);
  SG_TRY(hipGetLastError());
  return 0;
}
