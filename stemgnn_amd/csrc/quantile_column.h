// The column kernel of the serving epilogue, in its only copy: quantile_serve.hip launches it with one table of offsets (or
// none), seasonal.hip with a season policy that picks the table per (window, h) (DESIGN.md sections 5j, 5n).
//
// A column is the Q values of one (i, h, n) of a [count, Q, H, N] forecast, H * N floats apart.  Finishing a column:
//   a. rearrange: the column's values in non-decreasing order -- a SELECTION of the inputs, bit patterns kept.  The order is
//      fp32's with -0 == +0, NaN above everything (+inf included), ties (NaNs among themselves too) in row order: what
//      torch.sort(dim=1, stable=True) gives.  By rank: rank_q = #{j : v_j before v_q}, the row index breaking ties, and v_q goes
//      to row rank_q.
//   b. calibrate: stemgnn_conformal_apply on the result of a (one fp32 subtract / add per pair row, same broadcast: the
//      cf_widen of conformal_args.h that conformal.hip calls).
// The column goes back where it came from (or to `out`), or -- the store -- to the result slab row pos[0] + b, the position
// read on the device, with the batch's target copied beside it (the contract of stemgnn_forecast_store).
//
// One thread owns its columns from the first load to the last store, lanes run along n: every one of the Q row loads and row
// stores of a wave is one coalesced run.  Q is a run-time value, and a per-thread array indexed at run time would live in
// scratch memory, so the columns of a workgroup are held in LDS instead, component-major [component][Q][threads] in 4-byte
// words: lane t touches word t of every row, so every LDS access is conflict-free, and a thread only ever touches its own
// words -- no barrier anywhere.  The rank pass reads the column from one LDS plane and writes the ordered column to a second
// one (there is no second plane without rearrange); the output pass then walks the rows in order, so the global stores stay
// coalesced whatever the ranks are.
// VEC = 4: four consecutive n per thread, 16-byte global accesses (N % 4 == 0, every buffer 16-byte aligned, Q <= 16 so that
// the two planes of 64 threads fit 32 KB); VEC = 1 otherwise.
//
// A season policy travels by value as the LAST kernel argument (empty for QcNoSeason) and answers slice(i, h): how many floats
// into `offsets` the table of step h of window i begins.  Without a season `offsets` may be NULL (no calibration).
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

// QC_THREADS, QC_CHUNK, QC_LDS_BYTES, QC_VEC_MAX_Q and the workgroup geometry of qc_launch: calibration_plan.h

struct QcArgs {                             // travels by value in the kernel arguments
  const float* src;                         // [count or B, Q, H, N]
  float* dst;                               // finish / apply: out (may be src); store: out_forecast [capacity, Q, H, N]
  const float* target;                      // store only: [B, H, N]
  float* out_target;                        //             [capacity, H, N]
  const long long* pos;                     // store only: device int64[1]; NULL = finish / apply
  const float* offsets;                     // [P, Hg, Ng] or NULL; with a season [K, P, Hg, Ng]
  long long count;                          // windows (count or B)
  long long capacity;
  int Q, HN, N, rearrange, Hg, Ng, tvec;
  int cpb, wpb;                             // a workgroup = wpb windows x cpb column groups (cpb * wpb <= threads)
  int col_blocks, win_blocks;               // grid.x = col_blocks * win_blocks; a workgroup strides over the windows
  CfRoles roles;
};

struct QcNoSeason {                         // one table for every window and step
  static constexpr bool seasoned = false;
  __device__ size_t slice(long long, int) const { return 0; }
};

// v before w in the order of stage a, ties left to the caller
__device__ inline bool qc_less(float v, float w) { return v < w || (v == v && w != w); }

template <int VEC, class Season>
__global__ __launch_bounds__(QC_THREADS) void qc_kernel(const QcArgs a, const Season sn) {
  extern __shared__ float4 qc_lds[];
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
  float* A = reinterpret_cast<float*>(qc_lds) + t;          // plane A: the column as loaded; word (k * Q + q) * T
  float* B = A + (size_t)VEC * Q * T;                       // plane B: the column in order (rearrange only)
  const long long stride = (long long)a.win_blocks * a.wpb;
  for (long long i = (long long)ib * a.wpb + tw; i < a.count; i += stride) {
    const long long orow = p0 + i;
    if (store && (orow < 0 || orow >= a.capacity)) continue;
    const float* off = a.offsets + sn.slice(i, h);
    const float* s = a.src + (size_t)i * Q * HN + c;
    float* d = a.dst + (size_t)orow * Q * HN + c;
    // every row of the column is loaded before anything is stored (out may be the input), QC_CHUNK loads in flight
    for (int q0 = 0; q0 < Q; q0 += QC_CHUNK) {
      float v[QC_CHUNK][VEC] = {};
#pragma unroll
      for (int j = 0; j < QC_CHUNK; ++j) {
        if (q0 + j < Q) cf_load<VEC>(s + (size_t)(q0 + j) * HN, v[j]);
      }
#pragma unroll
      for (int j = 0; j < QC_CHUNK; ++j) {
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
            rank += (qc_less(u, v) || (!qc_less(v, u) && j < q)) ? 1 : 0;
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
      cf_widen<VEC>(v, Season::seasoned || a.offsets ? (int)a.roles.role[r] : 0, off, a.Hg, a.Ng, h, n);
      cf_store<VEC>(d + (size_t)r * HN, v);
    }
  }
}

// the vector form needs N % 4 == 0, Q <= 16 and both buffers 16-byte aligned
inline bool qc_vec_ok(int N, int Q, const void* src, const void* dst) {
  return qc_vec_shape_ok(N, Q) && sg_aligned16(src) && sg_aligned16(dst);
}

// the two stages of a column: fills offsets and Q .. Ng of `a`; the roles are the caller's (cf_pairs_ok)
inline void qc_stages(QcArgs* a, int Q, int H, int N, int rearrange, const float* offsets, int per_step, int per_node) {
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  a->offsets = offsets;
  a->Q = Q;
  a->HN = H * N;
  a->N = N;
  a->rearrange = rearrange != 0;
  a->Hg = gr.Hg;
  a->Ng = gr.Ng;
}
// makes `a` (after qc_stages) a store to slab rows pos[0] + b
inline void qc_store_to(QcArgs* a, const float* target, const long long* pos, float* out_target, long capacity) {
  a->target = target;
  a->out_target = out_target;
  a->pos = pos;
  a->capacity = capacity;
  a->tvec = qc_tvec_shape_ok(a->HN) && sg_aligned16(target) && sg_aligned16(out_target);
}

// fills the workgroup geometry of `a` and launches; `a` is a store when it has pos
template <class Season>
int qc_launch(QcArgs& a, long count, bool vec, const Season& sn, hipStream_t st) {
  QcPlan pl;                                        // threads, LDS, the workgroup's shape and the grid: calibration_plan.h
  qc_plan(count, a.Q, a.HN, a.rearrange != 0, vec, a.pos != nullptr, sg_num_cus(), &pl);
  a.count = count;
  a.cpb = pl.cpb;
  a.wpb = pl.wpb;
  a.col_blocks = pl.col_blocks;
  a.win_blocks = pl.win_blocks;
  const dim3 grid(pl.gx, pl.gy);
  auto kernel = vec ? qc_kernel<4, Season> : qc_kernel<1, Season>;
  hipLaunchKernelGGL(kernel, grid, dim3(pl.T), pl.lds, st, a, sn);
  SG_TRY(hipGetLastError());
  return 0;
}

}  // namespace
