// Opt-in controls of the fused optimizers (stemgnn_amd/optim.py): global gradient-norm clipping, weight decay and the
// skip of a step whose gradient is not finite -- computed on the device, inside the captured step.
//   stemgnn_grad_sqsum         one launch: fp64 partial sums of (g * grad_scale)^2, one per fixed 8192-float chunk
//   stemgnn_rmsprop_step_ext   the RMSprop / Adam step of tail.hip with  g1 = (g * grad_scale) * coef ; g2 = g1 + wd * p
//   stemgnn_adam_step_ext      in front of the unchanged update arithmetic (torch's order: clip_grad_norm_, then the
//                              optimizer adds the decay); decoupled (AdamW): p *= 1 - lr * wd instead.
// No third launch and no grid barrier: EVERY workgroup of the step kernel sums the partials itself (a few KB out of L2), in
// one fixed order, so all workgroups -- and every rank of a data-parallel run, whose reduced gradients are the same bits --
// hold the same norm, the same coefficient and the same skip decision.  The element -> partial mapping depends on n alone
// (never on the CU count) and nothing is accumulated with atomics: the norm is the same bits on any device, eager or replayed.
// stemgnn_rmsprop_step / stemgnn_adam_step (tail.hip) stay what the optimizers call when no control is enabled.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/stemgnn_hip.h"
#include "sg_host.h"

constexpr int OPT_THREADS = 256;
constexpr int OPT_LOADS = 8;                                        // independent 16-byte loads in flight per thread
constexpr size_t OPT_CHUNK = (size_t)OPT_THREADS * OPT_LOADS * 4;   // floats per workgroup of the norm kernel (32 KB)
constexpr unsigned OPT_MAX_BLOCKS = 2048;                           // grid cap of the step kernels (grid-stride beyond)

extern "C" size_t stemgnn_grad_norm_partials(size_t n) { return n == 0 ? 1 : (n + OPT_CHUNK - 1) / OPT_CHUNK; }

// Sum over the 256 threads of a workgroup in a fixed order: xor butterfly inside each wave (both partners add the same two
// numbers, so all 64 lanes end with the same bits), then the four wave sums left to right.  `sh` = 4 doubles of LDS.
__device__ __forceinline__ double opt_block_sum(double v, double* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const double s = ((sh[0] + sh[1]) + sh[2]) + sh[3];
  __syncthreads();
  return s;
}

__device__ __forceinline__ void opt_sq_acc(double& acc, float g, float gscale) {
  const double d = (double)(g * gscale);          // the scaled gradient the step kernel sees (one fp32 rounding)
  acc = fma(d, d, acc);                           // its square is exact in fp64
}

__global__ __launch_bounds__(OPT_THREADS) void sg_grad_sqsum_kernel(const float* __restrict__ g, size_t n, float gscale,
                                                                    double* __restrict__ partials) {
  __shared__ double sh[4];
  const size_t base = (size_t)blockIdx.x * OPT_CHUNK + (size_t)threadIdx.x * 4;
  double acc = 0.0;
  if ((size_t)(blockIdx.x + 1) * OPT_CHUNK <= n) {                  // a whole chunk: eight loads issued before the first use
    float4 v[OPT_LOADS];
#pragma unroll
    for (int k = 0; k < OPT_LOADS; ++k) v[k] = *reinterpret_cast<const float4*>(g + base + (size_t)k * OPT_THREADS * 4);
#pragma unroll
    for (int k = 0; k < OPT_LOADS; ++k) {
      opt_sq_acc(acc, v[k].x, gscale); opt_sq_acc(acc, v[k].y, gscale);
      opt_sq_acc(acc, v[k].z, gscale); opt_sq_acc(acc, v[k].w, gscale);
    }
  } else {                                                          // the last chunk: same element -> thread mapping, bounded
#pragma unroll
    for (int k = 0; k < OPT_LOADS; ++k) {
      const size_t i = base + (size_t)k * OPT_THREADS * 4;
      if (i + 3 < n) {
        const float4 v = *reinterpret_cast<const float4*>(g + i);
        opt_sq_acc(acc, v.x, gscale); opt_sq_acc(acc, v.y, gscale);
        opt_sq_acc(acc, v.z, gscale); opt_sq_acc(acc, v.w, gscale);
      } else {
        for (size_t j = i; j < n; ++j) opt_sq_acc(acc, g[j], gscale);
      }
    }
  }
  const double s = opt_block_sum(acc, sh);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

extern "C" int stemgnn_grad_sqsum(const float* grads, size_t n, float grad_scale, double* partials, void* stream) {
  if (!grads || !partials || n == 0) return SG_EINVAL;
  if ((((uintptr_t)grads) & 15) != 0 || (((uintptr_t)partials) & 7) != 0) return SG_EINVAL;
  const size_t blocks = stemgnn_grad_norm_partials(n);
  if (blocks > 0x7fffffffu) return SG_EINVAL;
  hipLaunchKernelGGL(sg_grad_sqsum_kernel, dim3((unsigned)blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, grads, n,
                     grad_scale, partials);
  SG_TRY(hipGetLastError());
  return 0;
}

// What a step does with its gradient, derived by every workgroup from the same partials in the same order.
struct OptControl {
  float total;   // pre-clip norm of the scaled gradient (NaN: no partials given, no norm taken)
  float coef;    // min(1, max_norm / (total + 1e-6)) in fp32 -- torch.nn.utils.clip_grad_norm_(norm_type=2); NaN stays NaN
  bool skip;     // skip_nonfinite and the norm is inf / NaN
};

__device__ __forceinline__ OptControl opt_control(const double* __restrict__ partials, size_t np, float max_norm,
                                                  int skip_nonfinite, double* sh) {
  OptControl c;
  c.total = __builtin_nanf("");
  c.coef = 1.f;
  c.skip = false;
  if (partials == nullptr) return c;
  double acc = 0.0;
  for (size_t i = threadIdx.x; i < np; i += OPT_THREADS) acc += partials[i];
  c.total = (float)sqrt(opt_block_sum(acc, sh));
  if (max_norm > 0.f) {
    const float r = max_norm / (c.total + 1e-6f);
    c.coef = r < 1.f ? r : (r != r ? r : 1.f);
  }
  c.skip = skip_nonfinite != 0 && !isfinite(c.total);
  return c;
}

// stats[0] norm, [1] coefficient applied (0: skipped), [2] running count of clipped steps, [3] running count of skipped steps
__device__ __forceinline__ void opt_write_stats(double* __restrict__ stats, const OptControl& c) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  stats[0] = (double)c.total;
  stats[1] = c.skip ? 0.0 : (double)c.coef;
  if (!c.skip && c.coef < 1.f) stats[2] += 1.0;
  if (c.skip) stats[3] += 1.0;
}

// ---- RMSprop ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void opt_rmsprop_elem(float& p, float g, float& sq, float lr, float alpha, float oma, float eps,
                                                 float gscale, float coef, float wd) {
  float gv = (g * gscale) * coef;
  if (wd != 0.f) gv = gv + wd * p;
  sq = alpha * sq + oma * gv * gv;                // oma = 1 - alpha (opt_one_minus)
  p -= lr * gv / (sqrtf(sq) + eps);
}

__global__ __launch_bounds__(OPT_THREADS) void sg_rmsprop_ext_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ sq, size_t n, const float* __restrict__ lr_dev,
    float alpha, float oma, float eps, int zero_grad, float gscale, float wd, float max_norm, int skip_nonfinite,
    const double* __restrict__ partials, size_t np, double* __restrict__ stats) {
  __shared__ double sh[4];
  const OptControl c = opt_control(partials, np, max_norm, skip_nonfinite, sh);
  opt_write_stats(stats, c);
  if (c.skip && !zero_grad) return;
  const float lr = lr_dev[0], coef = c.coef;
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (; i + 3 < n; i += stride) {
    if (!c.skip) {
      float4 pv = *reinterpret_cast<float4*>(p + i), sv = *reinterpret_cast<float4*>(sq + i);
      const float4 gv = *reinterpret_cast<float4*>(g + i);
      opt_rmsprop_elem(pv.x, gv.x, sv.x, lr, alpha, oma, eps, gscale, coef, wd);
      opt_rmsprop_elem(pv.y, gv.y, sv.y, lr, alpha, oma, eps, gscale, coef, wd);
      opt_rmsprop_elem(pv.z, gv.z, sv.z, lr, alpha, oma, eps, gscale, coef, wd);
      opt_rmsprop_elem(pv.w, gv.w, sv.w, lr, alpha, oma, eps, gscale, coef, wd);
      *reinterpret_cast<float4*>(p + i) = pv;
      *reinterpret_cast<float4*>(sq + i) = sv;
    }
    if (zero_grad) *reinterpret_cast<float4*>(g + i) = zero4;
  }
  if (i < n) {                          // ragged tail (at most one thread: the one whose vector straddles n)
    for (size_t j = i; j < n; ++j) {
      if (!c.skip) {
        float pv = p[j], sv = sq[j];
        opt_rmsprop_elem(pv, g[j], sv, lr, alpha, oma, eps, gscale, coef, wd);
        p[j] = pv;
        sq[j] = sv;
      }
      if (zero_grad) g[j] = 0.f;
    }
  }
}

static bool opt_bad_controls(float weight_decay, float max_norm, int skip_nonfinite, const double* partials,
                             const double* stats) {
  if (!stats || (((uintptr_t)stats | (uintptr_t)partials) & 7) != 0) return true;
  if (!(weight_decay >= 0.f) || max_norm != max_norm) return true;
  return (max_norm > 0.f || skip_nonfinite) && !partials;
}

// 1 - b as torch forms it.  torch.optim computes `1 - beta` in Python doubles and rounds the result to fp32 (0.999 ->
// 0.001 -> 0.001f); from the fp32 argument alone, 1.f - 0.999f = 0.00099998713 is off by 1.3e-5 -- which the second moment
// inherits in full.  The decimal the caller wrote is recovered as the shortest one that rounds to the given float (what
// printing a float32 shows); for a value that is not a short decimal this is 1 - (double)b rounded once.  Host only.
static float opt_one_minus(float b) {
  char buf[32];
  for (int prec = 1; prec <= 9; ++prec) {
    snprintf(buf, sizeof buf, "%.*g", prec, (double)b);
    const double d = strtod(buf, nullptr);
    if ((float)d == b) return (float)(1.0 - d);
  }
  return (float)(1.0 - (double)b);
}

static unsigned opt_step_blocks(size_t n) {
  const size_t blocks = ((n + 3) / 4 + OPT_THREADS - 1) / OPT_THREADS;
  return blocks > OPT_MAX_BLOCKS ? OPT_MAX_BLOCKS : (unsigned)blocks;
}

extern "C" int stemgnn_rmsprop_step_ext(float* params, float* grads, float* square_avg, size_t n, const float* lr_dev,
                                        float alpha, float eps, int zero_grad, float grad_scale, float weight_decay,
                                        float max_norm, int skip_nonfinite, const double* partials, double* stats,
                                        void* stream) {
  if (!params || !grads || !square_avg || !lr_dev || n == 0) return SG_EINVAL;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)square_avg) & 15) != 0) return SG_EINVAL;
  if (opt_bad_controls(weight_decay, max_norm, skip_nonfinite, partials, stats)) return SG_EINVAL;
  hipLaunchKernelGGL(sg_rmsprop_ext_kernel, dim3(opt_step_blocks(n)), dim3(OPT_THREADS), 0, (hipStream_t)stream, params,
                     grads, square_avg, n, lr_dev, alpha, opt_one_minus(alpha), eps, zero_grad, grad_scale, weight_decay,
                     max_norm, skip_nonfinite, partials, stemgnn_grad_norm_partials(n), stats);
  SG_TRY(hipGetLastError());
  return 0;
}

// ---- Adam / AdamW -------------------------------------------------------------------------------------------------
struct OptAdamConst {
  float b1, b2, omb1, omb2, eps, step_size, rs2, gscale, coef, wd, shrink;   // omb = 1 - beta (opt_one_minus)
};

__device__ __forceinline__ void opt_adam_elem(float& p, float g, float& m, float& v, const OptAdamConst& k) {
  const float b1 = k.b1, b2 = k.b2, eps = k.eps, step_size = k.step_size, rs2 = k.rs2, gscale = k.gscale, coef = k.coef,
              wd = k.wd, shrink = k.shrink;
  float gv = (g * gscale) * coef;
  p *= shrink;                                    // decoupled decay (AdamW): 1 - lr * wd, and wd = 0 here; else exactly 1
  if (wd != 0.f) gv = gv + wd * p;
  m = b1 * m + k.omb1 * gv;
  v = b2 * v + k.omb2 * gv * gv;
  p -= step_size * m / (sqrtf(v) * rs2 + eps);
}

__global__ __launch_bounds__(OPT_THREADS) void sg_adam_ext_kernel(
    float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n,
    const float* __restrict__ lr_dev, const float* __restrict__ step_dev, float b1, float b2, float omb1, float omb2,
    float eps, int zero_grad, float gscale, float weight_decay, int decoupled, float max_norm, int skip_nonfinite,
    const double* __restrict__ partials, size_t np, double* __restrict__ stats) {
  __shared__ double sh[4];
  const OptControl c = opt_control(partials, np, max_norm, skip_nonfinite, sh);
  opt_write_stats(stats, c);
  if (c.skip && !zero_grad) return;
  const float lr = lr_dev[0], coef = c.coef;
  const float t = step_dev[0] + 1.f;                      // this step's index (1-based); the tick launch advances it
  const float bc1 = 1.f - powf(b1, t), bc2 = 1.f - powf(b2, t);
  const float step_size = lr / bc1, rs2 = 1.f / sqrtf(bc2);
  const float shrink = decoupled ? (float)(1.0 - (double)lr * (double)weight_decay) : 1.f;
  const float wd = decoupled ? 0.f : weight_decay;          // the coupled (L2) term of the gradient
  const OptAdamConst k = {b1, b2, omb1, omb2, eps, step_size, rs2, gscale, coef, wd, shrink};
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
  for (; i + 3 < n; i += stride) {
    if (!c.skip) {
      float4 pv = *reinterpret_cast<float4*>(p + i), mv = *reinterpret_cast<float4*>(m + i),
             vv = *reinterpret_cast<float4*>(v + i);
      const float4 gv = *reinterpret_cast<float4*>(g + i);
      opt_adam_elem(pv.x, gv.x, mv.x, vv.x, k);
      opt_adam_elem(pv.y, gv.y, mv.y, vv.y, k);
      opt_adam_elem(pv.z, gv.z, mv.z, vv.z, k);
      opt_adam_elem(pv.w, gv.w, mv.w, vv.w, k);
      *reinterpret_cast<float4*>(p + i) = pv;
      *reinterpret_cast<float4*>(m + i) = mv;
      *reinterpret_cast<float4*>(v + i) = vv;
    }
    if (zero_grad) *reinterpret_cast<float4*>(g + i) = zero4;
  }
  if (i < n) {                          // ragged tail (at most one thread)
    for (size_t j = i; j < n; ++j) {
      if (!c.skip) {
        float pv = p[j], mv = m[j], vv = v[j];
        opt_adam_elem(pv, g[j], mv, vv, k);
        p[j] = pv;
        m[j] = mv;
        v[j] = vv;
      }
      if (zero_grad) g[j] = 0.f;
    }
  }
}

// The step count advances after every workgroup of the step kernel has read it (kernel boundary) -- unless the step was
// skipped: one workgroup takes the same decision from the same partials in the same order.
__global__ __launch_bounds__(OPT_THREADS) void sg_adam_tick_ext_kernel(float* __restrict__ step_dev,
                                                                       const double* __restrict__ partials, size_t np,
                                                                       int skip_nonfinite) {
  __shared__ double sh[4];
  const OptControl c = opt_control(skip_nonfinite ? partials : nullptr, np, 0.f, skip_nonfinite, sh);
  if (threadIdx.x == 0 && !c.skip) step_dev[0] += 1.f;
}

extern "C" int stemgnn_adam_step_ext(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                                     const float* lr_dev, float* step_dev, float beta1, float beta2, float eps, int zero_grad,
                                     float grad_scale, float weight_decay, int decoupled, float max_norm, int skip_nonfinite,
                                     const double* partials, double* stats, void* stream) {
  if (!params || !grads || !exp_avg || !exp_avg_sq || !lr_dev || !step_dev || n == 0) return SG_EINVAL;
  if ((((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) != 0) return SG_EINVAL;
  if (opt_bad_controls(weight_decay, max_norm, skip_nonfinite, partials, stats)) return SG_EINVAL;
  const size_t np = stemgnn_grad_norm_partials(n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(sg_adam_ext_kernel, dim3(opt_step_blocks(n)), dim3(OPT_THREADS), 0, st, params, grads, exp_avg,
                     exp_avg_sq, n, lr_dev, step_dev, beta1, beta2, opt_one_minus(beta1), opt_one_minus(beta2), eps, zero_grad,
                     grad_scale, weight_decay, decoupled, max_norm, skip_nonfinite, partials, np, stats);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(sg_adam_tick_ext_kernel, dim3(1), dim3(OPT_THREADS), 0, st, step_dev, partials, np, skip_nonfinite);
  SG_TRY(hipGetLastError());
  return 0;
}
