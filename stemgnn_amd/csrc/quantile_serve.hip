// The serving epilogue of a quantile forecast (include/stemgnn_hip.h: stemgnn_quantile_finish / _store).
//
// A column is the Q values of one (i, h, n) of a [count, Q, H, N] forecast, H * N floats apart.  Finishing a column:
//   a. rearrange: the column's values in non-decreasing order -- a SELECTION of the inputs, bit patterns kept.  The order is
//      fp32's with -0 == +0, NaN above everything (+inf included), ties (NaNs among themselves too) in row order: what
//      torch.sort(dim=1, stable=True) gives.  By rank: rank_q = #{j : v_j before v_q}, the row index breaking ties, and v_q goes
//      to row rank_q.
//   b. calibrate: stemgnn_conformal_apply on the result of a (one fp32 subtract / add per pair row, same broadcast: the
//      cf_widen of conformal_args.h that conformal.hip calls).
// finish writes the column back where it came from (or to `out`); store writes it to the result slab row pos[0] + b, the
// position read on the device, and copies the batch's target beside it (the contract of stemgnn_forecast_store).
//
// One thread owns its columns from the first load to the last store, lanes run along n: every one of the Q row loads and row
// stores of a wave is one coalesced run.  Q is a run-time value, and a per-thread array indexed at run time would live in
// scratch memory, so the columns of a workgroup are held in LDS instead, component-major [component][Q][threads] in 4-byte
// words: lane t touches word t of every row, so every LDS access is conflict-free, and a thread only ever touches its own
// words -- no barrier anywhere.  The rank pass reads the column from one LDS plane and writes the ordered column to a second
// one; the output pass then walks the rows in order, so the global stores stay coalesced whatever the ranks are.
// VEC = 4: four consecutive n per thread, 16-byte global accesses (N % 4 == 0, every buffer 16-byte aligned, Q <= 16 so that
// the two planes of 64 threads fit 32 KB); VEC = 1 otherwise.  Two instantiations in all.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "conformal_select.h"
#include "devattr.h"
#include "sg_host.h"

namespace {

constexpr int QS_THREADS = 256;             // the most; fewer (a multiple of 64) when Q is large: see qs_launch
constexpr int QS_CHUNK = 4;                 // rows whose global loads are in flight together
constexpr int QS_LDS_BYTES = 32 * 1024;     // per workgroup, both planes
constexpr int QS_VEC_MAX_Q = 16;

struct QsArgs {                             // travels by value in the kernel arguments
  const float* src;                         // [count or B, Q, H, N]
  float* dst;                               // finish: out (may be src); store: out_forecast [capacity, Q, H, N]
  const float* target;                      // store only: [B, H, N]
  float* out_target;                        //             [capacity, H, N]
  const long long* pos;                     // store only: device int64[1]; NULL = finish
  const float* offsets;                     // [P, Hg, Ng] or NULL
  long long count;                          // windows (count or B)
  long long capacity;
  int Q, HN, N, rearrange, Hg, Ng, tvec;
  int cpb, wpb;                             // a workgroup = wpb windows x cpb column groups (cpb * wpb <= threads)
  int col_blocks, win_blocks;               // grid.x = col_blocks * win_blocks; a workgroup strides over the windows
  CfRoles roles;
};

// v before w in the order of stage a, ties left to the caller
__device__ inline bool qs_less(float v, float w) { return v < w || (v == v && w != w); }

template <int VEC>
__global__ __launch_bounds__(QS_THREADS) void qs_finish_kernel(const QsArgs a) {
  extern __shared__ float4 qs_lds[];
  const int T = blockDim.x, t = threadIdx.x, Q = a.Q, HN = a.HN;
  const bool store = a.pos != nullptr;     // uniform over the launch
  const long long p0 = store ? a.pos[0] : 0;
  if (store && blockIdx.y == 1) {           // the batch's targets, beside the forecast rows: a workgroup per window
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
  float* A = reinterpret_cast<float*>(qs_lds) + t;          // plane A: the column as loaded; word (k * Q + q) * T
  float* B = A + (size_t)VEC * Q * T;                       // plane B: the column in order (rearrange only)
  const long long stride = (long long)a.win_blocks * a.wpb;
  for (long long i = (long long)ib * a.wpb + tw; i < a.count; i += stride) {
    const long long orow = p0 + i;
    if (store && (orow < 0 || orow >= a.capacity)) continue;
    const float* s = a.src + (size_t)i * Q * HN + c;
    float* d = a.dst + (size_t)orow * Q * HN + c;
    // every row of the column is loaded before anything is stored (out may be the input), QS_CHUNK loads in flight
    for (int q0 = 0; q0 < Q; q0 += QS_CHUNK) {
      float v[QS_CHUNK][VEC] = {};
#pragma unroll
      for (int j = 0; j < QS_CHUNK; ++j) {
        if (q0 + j < Q) cf_load<VEC>(s + (size_t)(q0 + j) * HN, v[j]);
      }
#pragma unroll
      for (int j = 0; j < QS_CHUNK; ++j) {
        if (q0 + j < Q) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) A[(k * Q + q0 + j) * T] = v[j][k];
        }
      }
    }
    const float* R = A;
    if (a.rearrange) {
#pragma unroll 1
      for (int k = 0; k < VEC; ++k) {
        const float* Ak = A + k * Q * T;
        float* Bk = B + k * Q * T;
#pragma unroll 1
        for (int q = 0; q < Q; ++q) {
          const float v = Ak[q * T];
          int rank = 0;
#pragma clang loop vectorize(disable) unroll_count(4)
          for (int j = 0; j < Q; ++j) {
            const float u = Ak[j * T];
            rank += (qs_less(u, v) || (!qs_less(v, u) && j < q)) ? 1 : 0;
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
      cf_widen<VEC>(v, a.offsets ? (int)a.roles.role[r] : 0, a.offsets, a.Hg, a.Ng, h, n);
      cf_store<VEC>(d + (size_t)r * HN, v);
    }
  }
}

// the stage arguments both entries share; fills Q .. roles of `a`
bool qs_stages_ok(long count, int Q, int H, int N, int rearrange, const float* offsets, int P, const int* lo_rows,
                  const int* hi_rows, int per_step, int per_node, QsArgs* a) {
  if (count <= 0 || Q <= 0 || H <= 0 || N <= 0 || Q > CF_MAX_Q || (long long)H * N >= (1ll << 31)) return false;
  a->roles = CfRoles{};
  if (offsets) {
    if (!lo_rows || !hi_rows) return false;
    if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &a->roles)) return false;
  }
  a->offsets = offsets;
  a->Q = Q;
  a->HN = H * N;
  a->N = N;
  a->rearrange = rearrange != 0;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  a->Hg = gr.Hg;
  a->Ng = gr.Ng;
  return true;
}

int qs_launch(QsArgs& a, long count, bool vec, hipStream_t st) {
  const bool store = a.pos != nullptr;
  const int VEC = vec ? 4 : 1, planes = a.rearrange ? 2 : 1;
  int T = QS_THREADS;
  while (T > 64 && (size_t)T * a.Q * VEC * 4 * planes > (size_t)QS_LDS_BYTES) T -= 64;
  const size_t lds = (size_t)T * a.Q * VEC * 4 * planes;                 // <= 32 KB: Q <= 32 (VEC 1), Q <= 16 (VEC 4)
  const int per = a.HN / VEC;                                            // column groups per window
  a.count = count;
  a.cpb = std::min(per, T);
  a.wpb = T / a.cpb;
  a.col_blocks = sg_ceil_div(per, a.cpb);
  const long long wins = ((long long)count + a.wpb - 1) / a.wpb;
  const long long cap = (long long)sg_num_cus() * 16;
  a.win_blocks = (int)std::max<long long>(1, std::min(wins, cap / a.col_blocks));
  const dim3 grid((unsigned)a.col_blocks * (unsigned)a.win_blocks, store ? 2 : 1);
  if (vec)
    hipLaunchKernelGGL(qs_finish_kernel<4>, grid, dim3(T), lds, st, a);
  else
    hipLaunchKernelGGL(qs_finish_kernel<1>, grid, dim3(T), lds, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int stemgnn_quantile_finish(const float* forecast, long count, int Q, int H, int N, int rearrange,
                                       const float* offsets, int P, const int* lo_rows, const int* hi_rows, int per_step,
                                       int per_node, float* out, void* stream) {
  if (!forecast || !out) return SG_EINVAL;
  QsArgs a = {};
  if (!qs_stages_ok(count, Q, H, N, rearrange, offsets, P, lo_rows, hi_rows, per_step, per_node, &a)) return SG_EINVAL;
  a.src = forecast;
  a.dst = out;
  const bool vec = (N & 3) == 0 && Q <= QS_VEC_MAX_Q && sg_aligned16(forecast) && sg_aligned16(out);
  return qs_launch(a, count, vec, (hipStream_t)stream);
}

extern "C" int stemgnn_quantile_store(const float* steps, const float* target, const long long* pos, int B, int Q, int H,
                                      int N, int rearrange, const float* offsets, int P, const int* lo_rows,
                                      const int* hi_rows, int per_step, int per_node, float* out_forecast, float* out_target,
                                      long capacity, void* stream) {
  if (!steps || !target || !pos || !out_forecast || !out_target || capacity <= 0) return SG_EINVAL;
  QsArgs a = {};
  if (!qs_stages_ok(B, Q, H, N, rearrange, offsets, P, lo_rows, hi_rows, per_step, per_node, &a)) return SG_EINVAL;
  a.src = steps;
  a.dst = out_forecast;
  a.target = target;
  a.out_target = out_target;
  a.pos = pos;
  a.capacity = capacity;
  a.tvec = (a.HN & 3) == 0 && sg_aligned16(target) && sg_aligned16(out_target);
  const bool vec = (N & 3) == 0 && Q <= QS_VEC_MAX_Q && sg_aligned16(steps) && sg_aligned16(out_forecast);
  return qs_launch(a, B, vec, (hipStream_t)stream);
}
