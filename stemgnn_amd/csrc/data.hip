// Data path either side of the hot path, all HBM-bound copies / reductions:
//   * normalisation of the raw series            data_loader/forecast_dataloader.py:7-22    (fp64 in, fp32 out)
//   * window gather = Dataset.__getitem__ + default collate  forecast_dataloader.py:56-63, models/handler.py:136-138
//   * MSE loss of the driver                     models/handler.py:140,162
//   * rolling-inference window shift             models/handler.py:56-61
//   * de-normalise + MAPE / MAE / RMSE           forecast_dataloader.py:25-38, utils/math_utils.py:24-74   (fp64)
// The series stays resident in HBM as one [T, N] fp32 matrix; a batch is B (W+H)-row slabs of it, so every row is one
// coalesced N-float copy.  Reductions are two-stage with a fixed order (bitwise reproducible).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "sg_host.h"

// ---------------------------------------------------------------------------------------------------------------
// Launch plans.  Every launcher below asks one of the static `*_plan` functions for its geometry and launches exactly that;
// stemgnn_data_plan (the end of this file) hands the same answers to the tests, so a threshold or a cap lives in one place.
// A plan function returns false for a shape its entry refuses.
struct SgDataPlan {
  unsigned gx = 1, gy = 1, gz = 1;                                // the (first) launch's grid
  int threads = 0, vec = 0, rows_per_wg = 0, form = 0, passes = 0, nchunk = 0;
};
constexpr int SG_GRID_YZ_MAX = 65535;                             // HIP's limit on grid.y and grid.z
constexpr int COPY_THREADS = 256;                                 // the flat grid-stride kernels (normalise, MSE backward, store)

static inline int sg_passes(size_t total, size_t per_pass) {     // trips of thread 0 of workgroup 0 through `i < total; i += per_pass`
  const size_t p = (total + per_pass - 1) / per_pass;
  return p > (size_t)0x7fffffff ? 0x7fffffff : (int)p;
}
static inline bool flat_plan(size_t total, unsigned max_blocks, SgDataPlan* p) {
  size_t blocks = (total + COPY_THREADS - 1) / COPY_THREADS;
  if (blocks > max_blocks) blocks = max_blocks;
  p->gx = (unsigned)blocks;
  p->threads = COPY_THREADS;
  p->passes = sg_passes(total, blocks * COPY_THREADS);
  return true;
}
__host__ __device__ static inline bool sg_copy_vec(int N) { return (N & 3) == 0; }   // a row of N floats as float4s

// ---------------------------------------------------------------------------------------------------------------
// out[t,n] = float( clip01?( (raw[t,n] - sub[n]) / div[n] ) ) -- IEEE fp64 subtract and divide, as numpy does
__global__ void sg_normalize_kernel(const double* __restrict__ raw, const double* __restrict__ sub,
                                    const double* __restrict__ div, int clip01, float* __restrict__ out, size_t total,
                                    int N) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (; i < total; i += stride) {
    const int n = (int)(i % (size_t)N);
    double v = __ddiv_rn(__dsub_rn(raw[i], sub[n]), div[n]);
    if (clip01) v = v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v);      // np.clip: NaN passes through
    out[i] = (float)v;
  }
}

static bool normalize_plan(long T, int N, SgDataPlan* p) {
  if (T <= 0 || N <= 0) return false;
  return flat_plan((size_t)T * N, 4096, p);
}

extern "C" int stemgnn_normalize_series(const double* raw, const double* sub, const double* div, int clip01, float* out,
                                        long T, int N, void* stream) {
  SgDataPlan p;
  if (!raw || !sub || !div || !out || !normalize_plan(T, N, &p)) return SG_EINVAL;
  const size_t total = (size_t)T * N;
  hipLaunchKernelGGL(sg_normalize_kernel, dim3(p.gx), dim3(p.threads), 0, (hipStream_t)stream, raw, sub, div, clip01, out,
                     total, N);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// x[b,w,:] = series[hi[b]-W+w,:] (w<W), y[b,h,:] = series[hi[b]+h,:] (h<H).  One workgroup per (row of the slab, b).
// Out-of-range rows (a bad index) set *status and write zeros instead of faulting.  The y rows come from `series_y` (the same
// shape; the series itself, or a copy of it that keeps its missing readings as NaN -- the _pair entries).
__global__ void sg_window_gather_kernel(const float* __restrict__ series, const float* __restrict__ series_y,
                                        const long long* __restrict__ hi,
                                        float* __restrict__ x, float* __restrict__ y, int W, int H, int N, long T,
                                        int* __restrict__ status) {
  const int r = blockIdx.x, b = blockIdx.y;
  const long long h0 = hi[b];
  const long long t = h0 - W + r;
  float* dst = r < W ? x + ((size_t)b * W + r) * N : y + ((size_t)b * H + (r - W)) * N;
  const bool ok = h0 - W >= 0 && h0 + H <= T;
  if (!ok && threadIdx.x == 0 && status) atomicOr(status, 1);
  const float* src = (r < W ? series : series_y) + (size_t)(ok ? t : 0) * N;
  if (sg_copy_vec(N)) {
    const float4* s4 = reinterpret_cast<const float4*>(src);
    float4* d4 = reinterpret_cast<float4*>(dst);
    for (int i = threadIdx.x; i < N / 4; i += blockDim.x) d4[i] = ok ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = ok ? src[i] : 0.f;
  }
}

// B is grid.y of both gathers, the window shifts and the store: above HIP's limit the launch itself would fail
static inline bool gather_shape_ok(int B, int W, int H, int N) {
  return B > 0 && B <= SG_GRID_YZ_MAX && W > 0 && H >= 0 && N > 0;
}
static bool gather_plan(int B, int W, int H, int N, SgDataPlan* p) {
  if (!gather_shape_ok(B, W, H, N)) return false;
  p->gx = (unsigned)(W + H), p->gy = (unsigned)B;
  p->threads = N >= 1024 ? 256 : (N >= 256 ? 128 : 64);
  p->vec = sg_copy_vec(N);
  return true;
}

extern "C" int stemgnn_window_gather_pair(const float* series_x, const float* series_y, const long long* hi, float* x,
                                          float* y, int B, int W, int H, int N, long T, int* status, void* stream) {
  SgDataPlan p;
  if (!series_x || !series_y || !hi || !x || !y || !gather_plan(B, W, H, N, &p) || T < (long)W + H) return SG_EINVAL;
  if (p.vec && ((((uintptr_t)series_x | (uintptr_t)series_y | (uintptr_t)x | (uintptr_t)y) & 15) != 0)) return SG_EINVAL;
  hipLaunchKernelGGL(sg_window_gather_kernel, dim3(p.gx, p.gy), dim3(p.threads), 0, (hipStream_t)stream, series_x, series_y, hi,
                     x, y, W, H, N, T, status);
  SG_TRY(hipGetLastError());
  return 0;
}
extern "C" int stemgnn_window_gather(const float* series, const long long* hi, float* x, float* y, int B, int W, int H,
                                     int N, long T, int* status, void* stream) {
  return stemgnn_window_gather_pair(series, series, hi, x, y, B, W, H, N, T, status, stream);
}

// Queue form of the gather (the DataLoader's iteration over one shuffled epoch, models/handler.py:136-138,157-159): the
// window-end rows of a whole epoch sit in `order` (device), `q` is the device-side iterator {position, arrival ticket,
// count}: every launch takes the next B windows and the LAST workgroup to arrive moves the position on -- so a captured
// hipGraph step replays with no per-step index copy ahead of it (that copy and its launch gap were ~10 us of a 1.26 ms
// step).  A position past `count` writes zeros and sets bit 1 of *status.  q[3] != 0 selects WRAP mode: a position from
// which no further full batch fits goes back to 0 (capture warm-ups and the schedule self-check of engine.TrainStep replay
// the step many times over whatever the order buffer holds; training never sets it).
__global__ void sg_window_gather_queue_kernel(const float* __restrict__ series, const float* __restrict__ series_y,
                                              const long long* __restrict__ order,
                                              long long* __restrict__ q, float* __restrict__ x, float* __restrict__ y,
                                              int W, int H, int N, long T, int rows_per_wg, int* __restrict__ status) {
  // few, larger workgroups (<= ~64: rows_per_wg slab rows of one batch element each), so that the arrival count costs
  // 64 atomics on one word, not one per slab row
  __shared__ long long pos_s;
  if (threadIdx.x == 0) pos_s = __hip_atomic_load(&q[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  const long long pos = pos_s;
  const int b = blockIdx.y, B = gridDim.y;
  const long long count = q[2];
  const bool have = pos >= 0 && pos + b < count;
  const long long h0 = have ? order[pos + b] : 0;
  const bool ok = have && h0 - W >= 0 && h0 + H <= T;
  if (!ok && threadIdx.x == 0 && blockIdx.x == 0 && status) atomicOr(status, have ? 1 : 2);
  const int r0 = blockIdx.x * rows_per_wg, r1 = min(W + H, r0 + rows_per_wg);
  for (int r = r0; r < r1; ++r) {
    float* dst = r < W ? x + ((size_t)b * W + r) * N : y + ((size_t)b * H + (r - W)) * N;
    const float* src = (r < W ? series : series_y) + (size_t)(ok ? h0 - W + r : 0) * N;
    if (sg_copy_vec(N)) {
      const float4* s4 = reinterpret_cast<const float4*>(src);
      float4* d4 = reinterpret_cast<float4*>(dst);
      for (int i = threadIdx.x; i < N / 4; i += blockDim.x) d4[i] = ok ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = ok ? src[i] : 0.f;
    }
  }
  if (threadIdx.x == 0) {
    // thread 0 read the position before it takes its ticket, so the last arriver is the last reader as well
    const long long nblk = (long long)gridDim.x * gridDim.y;
    const long long ticket = __hip_atomic_fetch_add(&q[1], 1ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket == nblk - 1) {
      __hip_atomic_store(&q[1], 0ll, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      long long next = pos + B;
      if (q[3] != 0 && next + B > count) next = 0;
      __hip_atomic_store(&q[0], next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

static bool gather_queue_plan(int B, int W, int H, int N, SgDataPlan* p) {
  if (!gather_shape_ok(B, W, H, N)) return false;
  constexpr int WGS = 64;                                         // about this many workgroups take a ticket
  int rows_per_wg = ((W + H) * B + WGS - 1) / WGS;
  if (rows_per_wg > W + H) rows_per_wg = W + H;
  p->gx = (unsigned)((W + H + rows_per_wg - 1) / rows_per_wg), p->gy = (unsigned)B;
  p->threads = N >= 512 ? 256 : (N >= 128 ? 128 : 64);            // fewer, longer-lived workgroups than the plain gather's
  p->vec = sg_copy_vec(N);
  p->rows_per_wg = rows_per_wg;
  return true;
}

extern "C" int stemgnn_window_gather_queue_pair(const float* series_x, const float* series_y, const long long* order,
                                                long long* queue, float* x, float* y, int B, int W, int H, int N, long T,
                                                int* status, void* stream) {
  SgDataPlan p;
  if (!series_x || !series_y || !order || !queue || !x || !y || !gather_queue_plan(B, W, H, N, &p) || T < (long)W + H)
    return SG_EINVAL;
  if (p.vec && ((((uintptr_t)series_x | (uintptr_t)series_y | (uintptr_t)x | (uintptr_t)y) & 15) != 0)) return SG_EINVAL;
  hipLaunchKernelGGL(sg_window_gather_queue_kernel, dim3(p.gx, p.gy), dim3(p.threads), 0, (hipStream_t)stream, series_x,
                     series_y, order, queue, x, y, W, H, N, T, p.rows_per_wg, status);
  SG_TRY(hipGetLastError());
  return 0;
}
extern "C" int stemgnn_window_gather_queue(const float* series, const long long* order, long long* queue, float* x, float* y,
                                           int B, int W, int H, int N, long T, int* status, void* stream) {
  return stemgnn_window_gather_queue_pair(series, series, order, queue, x, y, B, W, H, N, T, status, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// MSE (nn.MSELoss(reduction='mean'), handler.py:140): loss = sum((f-y)^2)/n; two-stage fixed-order reduction.
constexpr int MSE_BLOCKS = 128;
constexpr int MSE_THREADS = 256;
constexpr int MSE_SMALL_THREADS = 1024;                           // the one-workgroup form
constexpr size_t MSE_SMALL_MAX = (size_t)1 << 16;                 // ... up to this many elements

__device__ __forceinline__ float sg_block_sum(float v, float* sm) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) sm[w] = v;
  __syncthreads();
  float t = 0.f;
  if (threadIdx.x == 0)
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) t += sm[i];
  return t;                                                       // valid on thread 0
}

__global__ __launch_bounds__(MSE_THREADS) void sg_mse_partial_kernel(const float* __restrict__ f,
                                                                     const float* __restrict__ y, size_t n,
                                                                     float* __restrict__ part) {
  __shared__ float sm[MSE_THREADS / 64];
  float acc = 0.f;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const float d = f[i] - y[i];
    acc = fmaf(d, d, acc);
  }
  const float t = sg_block_sum(acc, sm);
  if (threadIdx.x == 0) part[blockIdx.x] = t;
}

__global__ void sg_mse_final_kernel(const float* __restrict__ part, int nparts, size_t n, float* __restrict__ loss,
                                    double* __restrict__ accum) {
  float v = (int)threadIdx.x < nparts ? part[threadIdx.x] : 0.f;
  __shared__ float sm[MSE_BLOCKS / 64];
  const float t = sg_block_sum(v, sm);
  if (threadIdx.x == 0) {
    const float l = t / (float)n;
    loss[0] = l;
    if (accum) accum[0] += (double)l;          // running epoch sum (handler.py:166 without the host sync)
  }
}

// small inputs (one training batch: B*H*N = 21,888 values at PEMS07): ONE workgroup, one launch -- the two-stage
// reduction above costs a second kernel boundary on the critical path for nothing
__global__ __launch_bounds__(MSE_SMALL_THREADS) void sg_mse_small_kernel(const float* __restrict__ f,
                                                                         const float* __restrict__ y, size_t n,
                                                                         float* __restrict__ loss, double* __restrict__ accum) {
  __shared__ float sm[MSE_SMALL_THREADS / 64];
  float acc = 0.f;
  for (size_t i = threadIdx.x; i < n; i += MSE_SMALL_THREADS) {
    const float d = f[i] - y[i];
    acc = fmaf(d, d, acc);
  }
  const float t = sg_block_sum(acc, sm);
  if (threadIdx.x == 0) {
    const float l = t / (float)n;
    loss[0] = l;
    if (accum) accum[0] += (double)l;
  }
}

__global__ void sg_mse_bwd_kernel(const float* __restrict__ f, const float* __restrict__ y, size_t n,
                                  const float* __restrict__ gout, float* __restrict__ df) {
  const float s = 2.f * gout[0] / (float)n;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    df[i] = s * (f[i] - y[i]);
}

extern "C" size_t stemgnn_mse_scratch_floats(void) { return MSE_BLOCKS; }

static bool mse_fwd_plan(size_t n, SgDataPlan* p) {
  if (n == 0) return false;
  p->form = n <= MSE_SMALL_MAX ? 0 : 1;
  p->gx = p->form == 0 ? 1 : MSE_BLOCKS;
  p->threads = p->form == 0 ? MSE_SMALL_THREADS : MSE_THREADS;
  p->passes = sg_passes(n, (size_t)p->gx * p->threads);
  return true;
}
static bool mse_bwd_plan(size_t n, SgDataPlan* p) { return n != 0 && flat_plan(n, 1024, p); }

extern "C" int stemgnn_mse_fwd(const float* forecast, const float* target, size_t n, float* scratch, float* loss,
                               double* loss_accum, void* stream) {
  SgDataPlan p;
  if (!forecast || !target || !scratch || !loss || !mse_fwd_plan(n, &p)) return SG_EINVAL;
  if (p.form == 0) {
    hipLaunchKernelGGL(sg_mse_small_kernel, dim3(p.gx), dim3(p.threads), 0, (hipStream_t)stream, forecast, target, n, loss,
                       loss_accum);
    SG_TRY(hipGetLastError());
    return 0;
  }
  hipLaunchKernelGGL(sg_mse_partial_kernel, dim3(p.gx), dim3(p.threads), 0, (hipStream_t)stream, forecast, target, n, scratch);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(sg_mse_final_kernel, dim3(1), dim3(MSE_BLOCKS), 0, (hipStream_t)stream, scratch, MSE_BLOCKS, n,
                     loss, loss_accum);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_mse_bwd(const float* forecast, const float* target, size_t n, const float* grad_loss,
                               float* dforecast, void* stream) {
  SgDataPlan p;
  if (!forecast || !target || !grad_loss || !dforecast || !mse_bwd_plan(n, &p)) return SG_EINVAL;
  hipLaunchKernelGGL(sg_mse_bwd_kernel, dim3(p.gx), dim3(p.threads), 0, (hipStream_t)stream, forecast, target, n, grad_loss,
                     dforecast);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// handler.py:56-61: inputs_next[b,w,:] = w < W-L ? inputs[b,w+L,:] : forecast[b,w-(W-L),:]   (L = model output length)
// and forecast_steps[b, step+j, :] = forecast[b,j,:] for j < min(horizon-step, L).  Out of place (ping-pong buffers).
__global__ void sg_roll_window_kernel(const float* __restrict__ inputs, const float* __restrict__ forecast,
                                      float* __restrict__ inputs_next, float* __restrict__ forecast_steps, int W, int L,
                                      int N, int step, int horizon) {
  const int r = blockIdx.x, b = blockIdx.y;                       // r < W: window row; r >= W: forecast_steps row
  const int take = min(horizon - step, L);
  const float* src;
  float* dst;
  if (r < W) {
    src = r < W - L ? inputs + ((size_t)b * W + r + L) * N : forecast + ((size_t)b * L + (r - (W - L))) * N;
    dst = inputs_next + ((size_t)b * W + r) * N;
  } else {
    const int j = r - W;
    if (j >= take) return;
    src = forecast + ((size_t)b * L + j) * N;
    dst = forecast_steps + ((size_t)b * horizon + step + j) * N;
  }
  for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = src[i];
}

// both window shifts: W window rows, then Q * L rows of forecast_steps (Q = 1: the point forecast's)
static bool roll_plan(int B, int W, int L, int N, int Q, SgDataPlan* p) {
  if (B <= 0 || B > SG_GRID_YZ_MAX || W <= 0 || N <= 0 || L <= 0 || L > W) return false;
  if (Q <= 0 || (long long)Q * L > (1 << 20)) return false;
  p->gx = (unsigned)(W + Q * L), p->gy = (unsigned)B;
  p->threads = N >= 256 ? 256 : 64;
  return true;
}

extern "C" int stemgnn_roll_window(const float* inputs, const float* forecast, float* inputs_next,
                                   float* forecast_steps, int B, int W, int L, int N, int step, int horizon,
                                   void* stream) {
  SgDataPlan p;
  if (!inputs || !forecast || !inputs_next || !forecast_steps || inputs == inputs_next) return SG_EINVAL;
  if (!roll_plan(B, W, L, N, 1, &p) || step < 0 || step >= horizon) return SG_EINVAL;
  hipLaunchKernelGGL(sg_roll_window_kernel, dim3(p.gx, p.gy), dim3(p.threads), 0, (hipStream_t)stream, inputs, forecast,
                     inputs_next, forecast_steps, W, L, N, step, horizon);
  SG_TRY(hipGetLastError());
  return 0;
}

// The same iteration for a quantile forecast [B,Q,L,N]: the window rows come from the POINT row forecast[b, point] exactly as
// above, and all Q rows go to forecast_steps [B,Q,horizon,N].  r < W: window row; r >= W: row (q, j) = ((r - W) / L, (r - W) % L).
__global__ void sg_roll_window_quantile_kernel(const float* __restrict__ inputs, const float* __restrict__ forecast,
                                               float* __restrict__ inputs_next, float* __restrict__ forecast_steps, int W, int L,
                                               int N, int Q, int point, int step, int horizon) {
  const int r = blockIdx.x, b = blockIdx.y;
  const int take = min(horizon - step, L);
  const float* src;
  float* dst;
  if (r < W) {
    src = r < W - L ? inputs + ((size_t)b * W + r + L) * N
                    : forecast + (((size_t)b * Q + point) * L + (r - (W - L))) * N;
    dst = inputs_next + ((size_t)b * W + r) * N;
  } else {
    const int q = (r - W) / L, j = (r - W) - q * L;
    if (j >= take) return;
    src = forecast + (((size_t)b * Q + q) * L + j) * N;
    dst = forecast_steps + (((size_t)b * Q + q) * horizon + step + j) * N;
  }
  for (int i = threadIdx.x; i < N; i += blockDim.x) dst[i] = src[i];
}

extern "C" int stemgnn_roll_window_quantile(const float* inputs, const float* forecast, float* inputs_next,
                                            float* forecast_steps, int B, int W, int L, int N, int Q, int point, int step,
                                            int horizon, void* stream) {
  SgDataPlan p;
  if (!inputs || !forecast || !inputs_next || !forecast_steps || inputs == inputs_next) return SG_EINVAL;
  if (!roll_plan(B, W, L, N, Q, &p) || step < 0 || step >= horizon || point < 0 || point >= Q) return SG_EINVAL;
  hipLaunchKernelGGL(sg_roll_window_quantile_kernel, dim3(p.gx, p.gy), dim3(p.threads), 0, (hipStream_t)stream, inputs,
                     forecast, inputs_next, forecast_steps, W, L, N, Q, point, step, horizon);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// result slabs of a replayed rolling forecast (engine.ForecastStep): rows pos[0] + b of out_forecast / out_target [capacity, H, N]
// := forecast / target [b] -- the position is the window queue's, read on the device (no per-batch host copy)
__global__ void sg_forecast_store_kernel(const float* __restrict__ forecast, const float* __restrict__ target,
                                         const long long* __restrict__ pos, float* __restrict__ out_f, float* __restrict__ out_t,
                                         int HN, long capacity) {
  const int b = blockIdx.y;
  const long long row = pos[0] + b;
  if (row < 0 || row >= capacity) return;
  const bool tgt = blockIdx.z != 0;
  const float* src = (tgt ? target : forecast) + (size_t)b * HN;
  float* dst = (tgt ? out_t : out_f) + (size_t)row * HN;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HN; i += gridDim.x * blockDim.x) dst[i] = src[i];
}

static bool store_plan(int B, int H, int N, SgDataPlan* p) {
  if (B <= 0 || B > SG_GRID_YZ_MAX || H <= 0 || N <= 0 || (long long)H * N > (1 << 30)) return false;    // the kernel's int index
  flat_plan((size_t)H * N, 64, p);                                // per slab row: at most 64 workgroups
  p->gy = (unsigned)B, p->gz = 2;                                 // z: forecast | target
  return true;
}

extern "C" int stemgnn_forecast_store(const float* forecast, const float* target, const long long* pos, float* out_forecast,
                                      float* out_target, int B, int H, int N, long capacity, void* stream) {
  SgDataPlan p;
  if (!forecast || !target || !pos || !out_forecast || !out_target || !store_plan(B, H, N, &p) || capacity <= 0)
    return SG_EINVAL;
  hipLaunchKernelGGL(sg_forecast_store_kernel, dim3(p.gx, p.gy, p.gz), dim3(p.threads), 0, (hipStream_t)stream, forecast,
                     target, pos, out_forecast, out_target, H * N, capacity);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// evaluate(): target / forecast [count, H, N] fp32 (the reference holds the same values in float64 arrays,
// handler.py:50); optional de-normalisation v*mul[n] + add[n] in fp64 with separate multiply and add roundings
// (numpy: `data * std + mean`).  Per element: ape = min?(|f-t|/|t| + 1e-5, 5) (NaN kept), ae = |f-t|, se = (f-t)^2.
// Stage 1: column c = (h, n) sums over a chunk of `count`; stage 2: fixed-order chunk sum, then every axis variant:
// out = overall[3] | by_node[3][N] | by_step[3][H] | by_step_node[3][H][N]   (each triple = mape, mae, rmse).
// MASKED (stemgnn_eval_metrics_masked): an element whose target is NaN is skipped, a fourth plane of `part` / `colsum` counts
// the elements kept per column, and every mean divides by its slice's count (a slice with none: 0 / 0 = NaN).
constexpr int EVAL_CHUNK_ROWS = 64;
constexpr int METRIC_THREADS = 256;                               // both stages of both metric entries

template <bool MASKED>
__global__ __launch_bounds__(METRIC_THREADS) void sg_eval_partial_kernel(const float* __restrict__ target,
                                                              const float* __restrict__ forecast,
                                                              const double* __restrict__ mul,
                                                              const double* __restrict__ add, long count, int HN, int N,
                                                              double* __restrict__ part) {
  // Plain operators under `fp contract(off)`: __dmul_rn / __dadd_rn are inline functions holding a plain operator each, compiled
  // under the translation unit's contraction mode, so v * mul + add and s_se + d * d written with them fused into one FMA and
  // the de-normalised values were not numpy's `data * std + mean`.  The pragma covers what is written in this body.
#pragma clang fp contract(off)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= HN) return;
  const long r0 = (long)blockIdx.y * EVAL_CHUNK_ROWS;
  const long r1 = min(count, r0 + (long)EVAL_CHUNK_ROWS);
  const int n = c % N;
  const double mu = mul ? mul[n] : 1.0, ad = mul ? add[n] : 0.0;
  double s_ape = 0.0, s_ae = 0.0, s_se = 0.0, s_cnt = 0.0;
  for (long r = r0; r < r1; ++r) {
    double t = (double)target[(size_t)r * HN + c], f = (double)forecast[(size_t)r * HN + c];
    if (MASKED) {
      if (t != t) continue;
      s_cnt += 1.0;                                               // a small integer: exact in fp64
    }
    if (mul) {
      t = t * mu + ad;
      f = f * mu + ad;
    }
    const double d = __dsub_rn(f, t);
    const double ae = fabs(d);
    double ape = __dadd_rn(__ddiv_rn(ae, fabs(t)), 1e-5);
    ape = ape > 5.0 ? 5.0 : ape;
    s_ape += ape;
    s_ae += ae;
    s_se += d * d;
  }
  const size_t nchunk = gridDim.y;
  part[((size_t)0 * nchunk + blockIdx.y) * HN + c] = s_ape;
  part[((size_t)1 * nchunk + blockIdx.y) * HN + c] = s_ae;
  part[((size_t)2 * nchunk + blockIdx.y) * HN + c] = s_se;
  if (MASKED) part[((size_t)3 * nchunk + blockIdx.y) * HN + c] = s_cnt;
}

// one workgroup; thread-per-column chunk sums -> by_step_node sums in LDS-free global scratch (`colsum`), then the
// coarser variants by fixed-order loops (H*N is a few thousand at most: this is a microsecond-scale epilogue)
template <bool MASKED>
__global__ __launch_bounds__(METRIC_THREADS) void sg_eval_final_kernel(const double* __restrict__ part, int nchunk, long count,
                                                            int H, int N, double* __restrict__ colsum,
                                                            double* __restrict__ out) {
  const int HN = H * N;
  constexpr int NQ = MASKED ? 4 : 3;                              // plane 3: the valid counts
  double* nodesum = colsum + (size_t)NQ * HN;                     // [NQ][N]
  for (int q = 0; q < NQ; ++q)
    for (int c = threadIdx.x; c < HN; c += blockDim.x) {
      double s = 0.0;
      for (int k = 0; k < nchunk; ++k) s += part[((size_t)q * nchunk + k) * HN + c];
      colsum[(size_t)q * HN + c] = s;
    }
  __syncthreads();
  double* overall = out;
  double* by_node = out + 3;
  double* by_step = by_node + 3 * (size_t)N;
  double* by_sn = by_step + 3 * (size_t)H;
  const double cnt = (double)count;
  if (MASKED) {                                                   // the count plane's node sums, ahead of their readers
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
      double s = 0.0;
      for (int h = 0; h < H; ++h) s += colsum[(size_t)3 * HN + (size_t)h * N + n];
      nodesum[(size_t)3 * N + n] = s;
    }
    __syncthreads();
  }
  for (int q = 0; q < 3; ++q) {
    for (int c = threadIdx.x; c < HN; c += blockDim.x) {
      const double m = colsum[(size_t)q * HN + c] / (MASKED ? colsum[(size_t)3 * HN + c] : cnt);
      by_sn[(size_t)q * HN + c] = q == 2 ? sqrt(m) : m;
    }
    for (int n = threadIdx.x; n < N; n += blockDim.x) {
      double s = 0.0;
      for (int h = 0; h < H; ++h) s += colsum[(size_t)q * HN + (size_t)h * N + n];
      nodesum[(size_t)q * N + n] = s;
      const double m = s / (MASKED ? nodesum[(size_t)3 * N + n] : cnt * H);
      by_node[(size_t)q * N + n] = q == 2 ? sqrt(m) : m;
    }
    for (int h = threadIdx.x; h < H; h += blockDim.x) {
      double s = 0.0, k = 0.0;
      for (int n = 0; n < N; ++n) s += colsum[(size_t)q * HN + (size_t)h * N + n];
      if (MASKED)
        for (int n = 0; n < N; ++n) k += colsum[(size_t)3 * HN + (size_t)h * N + n];
      const double m = s / (MASKED ? k : cnt * N);
      by_step[(size_t)q * H + h] = q == 2 ? sqrt(m) : m;
    }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int q = threadIdx.x;
    double s = 0.0, k = 0.0;
    for (int n = 0; n < N; ++n) s += nodesum[(size_t)q * N + n];
    if (MASKED)
      for (int n = 0; n < N; ++n) k += nodesum[(size_t)3 * N + n];
    const double m = s / (MASKED ? k : cnt * HN);
    overall[q] = q == 2 ? sqrt(m) : m;
  }
}

static inline int eval_nchunk(long count) { return (int)((count + EVAL_CHUNK_ROWS - 1) / EVAL_CHUNK_ROWS); }
// stage 1 of both metric entries: thread = column (h, n), grid.y = row chunk, grid.z = `planes` (quantile metrics: what to sum)
static bool metrics_plan(long count, int H, int N, int planes, SgDataPlan* p) {
  if (count <= 0 || H <= 0 || N <= 0 || (count + EVAL_CHUNK_ROWS - 1) / EVAL_CHUNK_ROWS > SG_GRID_YZ_MAX) return false;
  p->nchunk = eval_nchunk(count);
  p->threads = METRIC_THREADS;
  p->gx = (unsigned)((H * N + METRIC_THREADS - 1) / METRIC_THREADS), p->gy = (unsigned)p->nchunk, p->gz = (unsigned)planes;
  return true;
}

extern "C" size_t stemgnn_eval_scratch_doubles(long count, int H, int N) {
  if (count <= 0 || H <= 0 || N <= 0) return 0;
  return (size_t)3 * H * N * ((size_t)eval_nchunk(count) + 1) + 3 * (size_t)N;
}
extern "C" size_t stemgnn_eval_out_doubles(int H, int N) {
  if (H <= 0 || N <= 0) return 0;
  return 3 + 3 * (size_t)N + 3 * (size_t)H + 3 * (size_t)H * N;
}

extern "C" size_t stemgnn_eval_scratch_doubles_masked(long count, int H, int N) {
  if (count <= 0 || H <= 0 || N <= 0) return 0;
  return (size_t)4 * H * N * ((size_t)eval_nchunk(count) + 1) + 4 * (size_t)N;
}

template <bool MASKED>
static int eval_metrics_impl(const float* target, const float* forecast, const double* mul, const double* add, long count,
                             int H, int N, double* scratch, double* out, void* stream) {
  SgDataPlan p;
  if (!target || !forecast || !scratch || !out || !metrics_plan(count, H, N, 1, &p)) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  const int HN = H * N, nchunk = p.nchunk;
  double* part = scratch;
  double* colsum = scratch + (size_t)(MASKED ? 4 : 3) * HN * nchunk;
  hipLaunchKernelGGL(sg_eval_partial_kernel<MASKED>, dim3(p.gx, p.gy), dim3(p.threads), 0, (hipStream_t)stream, target,
                     forecast, mul, add, count, HN, N, part);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(sg_eval_final_kernel<MASKED>, dim3(1), dim3(METRIC_THREADS), 0, (hipStream_t)stream, part, nchunk, count,
                     H, N, colsum, out);
  SG_TRY(hipGetLastError());
  return 0;
}
extern "C" int stemgnn_eval_metrics(const float* target, const float* forecast, const double* mul, const double* add,
                                    long count, int H, int N, double* scratch, double* out, void* stream) {
  return eval_metrics_impl<false>(target, forecast, mul, add, count, H, N, scratch, out, stream);
}
extern "C" int stemgnn_eval_metrics_masked(const float* target, const float* forecast, const double* mul, const double* add,
                                           long count, int H, int N, double* scratch, double* out, void* stream) {
  return eval_metrics_impl<true>(target, forecast, mul, add, count, H, N, scratch, out, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// Calibration metrics of a quantile forecast (include/stemgnn_hip.h: stemgnn_quantile_metrics), in the style of the pass above:
// target [count,H,N], forecast [count,Q,H,N]; K = 2Q + 2P + 1 statistics (P = Q / 2) plus one plane that counts the elements
// kept.  Stage 1: thread = column c = (h, n) of one row chunk; blockIdx.z picks what it sums -- z < Q: level z (pinball sum,
// target <= forecast count); Q <= z < Q + P: pair (i, Q-1-i) (inside count, width sum); z = Q + P: the crossing count and the
// kept count.  No thread holds more than two sums, so no per-thread array whatever Q is.  Stage 2 (one workgroup): chunk sums ->
// column sums -> per-step sums over n -> overall sums over h, each a fixed-order loop; every mean = sum / the kept count of its
// slice (0 / 0 = NaN for a slice with nothing valid).
struct SgTausD { double v[32]; };

template <bool MASKED>
__global__ __launch_bounds__(METRIC_THREADS) void sg_quantile_partial_kernel(const float* __restrict__ target,
                                                                  const float* __restrict__ forecast, SgTausD taus,
                                                                  const double* __restrict__ mul,
                                                                  const double* __restrict__ add, long count, int Q, int HN,
                                                                  int N, double* __restrict__ part) {
  // as in sg_eval_partial_kernel: every product and sum rounds on its own
#pragma clang fp contract(off)
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= HN) return;
  const int P = Q / 2, z = blockIdx.z;
  const long r0 = (long)blockIdx.y * EVAL_CHUNK_ROWS;
  const long r1 = min(count, r0 + (long)EVAL_CHUNK_ROWS);
  const int n = c % N;
  const bool dn = mul != nullptr;
  const double mu = dn ? mul[n] : 1.0, ad = dn ? add[n] : 0.0;
  const size_t nchunk = gridDim.y;
  double s0 = 0.0, s1 = 0.0;
  int k0, k1;
  if (z < Q) {
    const double tau = taus.v[z];
    k0 = z, k1 = Q + z;
    for (long r = r0; r < r1; ++r) {
      double t = (double)target[(size_t)r * HN + c], f = (double)forecast[((size_t)r * Q + z) * HN + c];
      if (MASKED && t != t) continue;
      if (dn) {
        t = t * mu + ad;
        f = f * mu + ad;
      }
      const double d = __dsub_rn(f, t);
      s0 += d >= 0.0 ? (1.0 - tau) * d : -tau * d;
      s1 += t <= f ? 1.0 : 0.0;
    }
  } else if (z < Q + P) {
    const int i = z - Q, j = Q - 1 - i;
    k0 = 2 * Q + i, k1 = 2 * Q + P + i;
    for (long r = r0; r < r1; ++r) {
      double t = (double)target[(size_t)r * HN + c];
      double lo = (double)forecast[((size_t)r * Q + i) * HN + c], hi = (double)forecast[((size_t)r * Q + j) * HN + c];
      if (MASKED && t != t) continue;
      if (dn) {
        t = t * mu + ad;
        lo = lo * mu + ad;
        hi = hi * mu + ad;
      }
      s0 += (lo <= t && t <= hi) ? 1.0 : 0.0;
      s1 += __dsub_rn(hi, lo);
    }
  } else {
    k0 = 2 * Q + 2 * P, k1 = k0 + 1;
    for (long r = r0; r < r1; ++r) {
      const double t = (double)target[(size_t)r * HN + c];
      if (MASKED && t != t) continue;
      bool cross = false;
      double prev = 0.0;
      for (int q = 0; q < Q; ++q) {
        double f = (double)forecast[((size_t)r * Q + q) * HN + c];
        if (dn) f = f * mu + ad;
        if (q > 0 && f < prev) cross = true;
        prev = f;
      }
      s0 += cross ? 1.0 : 0.0;
      s1 += 1.0;
    }
  }
  part[((size_t)k0 * nchunk + blockIdx.y) * HN + c] = s0;
  part[((size_t)k1 * nchunk + blockIdx.y) * HN + c] = s1;
}

__global__ __launch_bounds__(METRIC_THREADS) void sg_quantile_final_kernel(const double* __restrict__ part, int nchunk, int K, int H, int N,
                                                                double* __restrict__ colsum, double* __restrict__ out) {
  const int HN = H * N, K1 = K + 1;                                // plane K: the kept counts
  double* stepsum = colsum + (size_t)K1 * HN;                      // [K1][H]
  for (int i = threadIdx.x; i < K1 * HN; i += blockDim.x) {
    const int k = i / HN, c = i - k * HN;
    double s = 0.0;
    for (int j = 0; j < nchunk; ++j) s += part[((size_t)k * nchunk + j) * HN + c];
    colsum[i] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K1 * H; i += blockDim.x) {
    double s = 0.0;
    for (int n = 0; n < N; ++n) s += colsum[(size_t)i * N + n];      // i = k * H + h
    stepsum[i] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i < K * H; i += blockDim.x) out[K + i] = stepsum[i] / stepsum[(size_t)K * H + i % H];
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    double s = 0.0, cnt = 0.0;
    for (int h = 0; h < H; ++h) s += stepsum[(size_t)k * H + h];
    for (int h = 0; h < H; ++h) cnt += stepsum[(size_t)K * H + h];
    out[k] = s / cnt;
  }
}

static inline int quantile_nstat(int Q) { return 2 * Q + 2 * (Q / 2) + 1; }
static bool quantile_metrics_plan(long count, int Q, int H, int N, SgDataPlan* p) {
  if (Q <= 0 || Q > 32 || H <= 0 || N <= 0) return false;
  if ((long long)H * N > (1ll << 30) / (quantile_nstat(Q) + 1)) return false;           // the final kernel's int indices
  return metrics_plan(count, H, N, Q + Q / 2 + 1, p);             // z: Q levels, Q / 2 pairs, crossing + kept counts
}
extern "C" size_t stemgnn_quantile_scratch_doubles(long count, int Q, int H, int N) {
  if (count <= 0 || Q <= 0 || Q > 32 || H <= 0 || N <= 0) return 0;
  const size_t K1 = (size_t)quantile_nstat(Q) + 1;
  return K1 * H * N * ((size_t)eval_nchunk(count) + 1) + K1 * H;
}
extern "C" size_t stemgnn_quantile_out_doubles(int Q, int H) {
  if (Q <= 0 || Q > 32 || H <= 0) return 0;
  return (size_t)quantile_nstat(Q) * ((size_t)H + 1);
}

template <bool MASKED>
static int quantile_metrics_impl(const float* target, const float* forecast, const double* taus, const double* mul,
                                 const double* add, long count, int Q, int H, int N, double* scratch, double* out,
                                 void* stream) {
  SgDataPlan p;
  if (!target || !forecast || !taus || !scratch || !out || !quantile_metrics_plan(count, Q, H, N, &p)) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  SgTausD t;
  for (int q = 0; q < 32; ++q) t.v[q] = 0.5;
  for (int q = 0; q < Q; ++q) {
    if (!(taus[q] > 0.0 && taus[q] < 1.0)) return SG_EINVAL;        // NaN fails both
    t.v[q] = taus[q];
  }
  const int HN = H * N, nchunk = p.nchunk, K = quantile_nstat(Q);
  double* part = scratch;
  double* colsum = scratch + (size_t)(K + 1) * HN * nchunk;
  hipLaunchKernelGGL(sg_quantile_partial_kernel<MASKED>, dim3(p.gx, p.gy, p.gz), dim3(p.threads), 0, (hipStream_t)stream,
                     target, forecast, t, mul, add, count, Q, HN, N, part);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(sg_quantile_final_kernel, dim3(1), dim3(METRIC_THREADS), 0, (hipStream_t)stream, part, nchunk, K, H, N,
                     colsum, out);
  SG_TRY(hipGetLastError());
  return 0;
}
extern "C" int stemgnn_quantile_metrics(const float* target, const float* forecast, const double* taus, const double* mul,
                                        const double* add, long count, int Q, int H, int N, double* scratch, double* out,
                                        void* stream) {
  return quantile_metrics_impl<false>(target, forecast, taus, mul, add, count, Q, H, N, scratch, out, stream);
}
extern "C" int stemgnn_quantile_metrics_masked(const float* target, const float* forecast, const double* taus, const double* mul,
                                               const double* add, long count, int Q, int H, int N, double* scratch, double* out,
                                               void* stream) {
  return quantile_metrics_impl<true>(target, forecast, taus, mul, add, count, Q, H, N, scratch, out, stream);
}

// ---------------------------------------------------------------------------------------------------------------
// What the launchers above do for a shape (include/stemgnn_hip.h: stemgnn_data_plan): host only, nothing is launched or read.
static inline bool fits_int(long v) { return v >= -0x7fffffffl - 1 && v <= 0x7fffffffl; }

extern "C" int stemgnn_data_plan(int entry, long a0, long a1, long a2, long a3, long a4, int* out) {
  if (!out) return SG_EINVAL;
  const bool ints3 = fits_int(a0) && fits_int(a1) && fits_int(a2), ints = ints3 && fits_int(a3);   // a4: the quantile shift's Q alone
  const int i0 = (int)a0, i1 = (int)a1, i2 = (int)a2, i3 = (int)a3, i4 = (int)a4;
  SgDataPlan p;
  bool ok = false;
  switch (entry) {
    case SG_DATA_NORMALIZE: ok = fits_int(a1) && normalize_plan(a0, i1, &p); break;
    case SG_DATA_GATHER: ok = ints && gather_plan(i0, i1, i2, i3, &p); break;
    case SG_DATA_GATHER_QUEUE: ok = ints && gather_queue_plan(i0, i1, i2, i3, &p); break;
    case SG_DATA_MSE_FWD: ok = a0 > 0 && mse_fwd_plan((size_t)a0, &p); break;
    case SG_DATA_MSE_BWD: ok = a0 > 0 && mse_bwd_plan((size_t)a0, &p); break;
    case SG_DATA_ROLL: ok = ints && roll_plan(i0, i1, i2, i3, 1, &p); break;
    case SG_DATA_ROLL_QUANTILE: ok = ints && fits_int(a4) && roll_plan(i0, i1, i2, i3, i4, &p); break;
    case SG_DATA_FORECAST_STORE: ok = ints3 && store_plan(i0, i1, i2, &p); break;
    case SG_DATA_EVAL: ok = fits_int(a1) && fits_int(a2) && metrics_plan(a0, i1, i2, 1, &p); break;
    case SG_DATA_QUANTILE_METRICS: ok = fits_int(a1) && fits_int(a2) && fits_int(a3) && quantile_metrics_plan(a0, i1, i2, i3, &p); break;
    default: break;
  }
  if (!ok) return SG_EINVAL;
  const int words[SG_DATA_PLAN_WORDS] = {(int)p.gx, (int)p.gy, (int)p.gz, p.threads, p.vec, p.rows_per_wg, p.form, p.passes, p.nchunk};
  for (int i = 0; i < SG_DATA_PLAN_WORDS; ++i) out[i] = words[i];
  return 0;
}
