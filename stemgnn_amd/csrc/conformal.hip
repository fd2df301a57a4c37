// Split-conformal calibration of quantile bands (include/stemgnn_hip.h: stemgnn_conformal_*).
//
// fit:   for every pair p of quantile rows (lo, hi) and every group g of (h, n) positions, the k-th smallest of the scores
//            s = max(f_lo - y, y - f_hi)                          (fp32; NaN counts as +inf)
//        with k = ceil((m + 1) * c * (1 - 1e-12)) of the group's m valid scores: an exact MSB-first radix SELECT on the
//        order-preserving 32-bit key of s, four passes of 8 bits.  No sort, no floating-point atomics; the only atomics are
//        integer histogram counts, which are exact in any order, so the result is the same bits on every run.
//        The kernels and the host loop of the passes are conformal_fit.h (shared with seasonal.hip), run here without a season.
// apply: out_lo = f_lo - off, out_hi = f_hi + off, every other row copied; one streaming kernel, defined here.
//
// The key, the wave pick and the vector load / store live in conformal_select.h, the band widening, the argument checks and
// the grouping geometry in conformal_args.h: quantile_column.h, aci.hip, anomaly.hip and seasonal.hip use the same definitions.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/stemgnn_hip.h"
#include "calibration_plan.h"
#include "conformal_args.h"
#include "conformal_fit.h"
#include "conformal_select.h"
#include "devattr.h"
#include "sg_host.h"

namespace {

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

}  // namespace

extern "C" long stemgnn_conformal_rank(long m, double coverage) { return (long)cf_rank((long long)m, coverage); }

extern "C" size_t stemgnn_conformal_scratch_bytes(long count, int H, int N, int P, int per_step, int per_node) {
  if (!cf_shapes_ok(count, 1, H, N, P)) return 0;
  return cf_fit_scratch_bytes(P, cf_grouping(per_step, per_node, H, N).groups());
}

extern "C" int stemgnn_conformal_fit(const float* target, const float* forecast, long count, int Q, int H, int N, int P,
                                     const int* lo_rows, const int* hi_rows, const double* coverage, int per_step,
                                     int per_node, int masked, void* scratch, float* offsets, long long* counts,
                                     void* stream) {
  if (!target || !forecast || !lo_rows || !hi_rows || !coverage || !scratch || !offsets || !counts) return SG_EINVAL;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, nullptr)) return SG_EINVAL;
  if (!sg_aligned16(scratch)) return SG_EINVAL;
  CfPairs pairs;
  if (!cf_fit_pairs(P, lo_rows, hi_rows, coverage, &pairs)) return SG_EINVAL;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  if ((long long)P * (long long)gr.groups() >= (1ll << 31) / 4) return SG_EINVAL;   // the pick kernel's int indices
  if (!per_node && gr.groups() > 65535) return SG_EINVAL;                           // grid.y of the stream form
  return cf_fit_run(target, forecast, count, count, Q, H, N, P, P, pairs, gr, per_node != 0, masked != 0, CfNoSeason{}, scratch,
                    offsets, counts, (hipStream_t)stream);
}

extern "C" int stemgnn_conformal_apply(const float* forecast, const float* offsets, long count, int Q, int H, int N, int P,
                                       const int* lo_rows, const int* hi_rows, int per_step, int per_node, float* out,
                                       void* stream) {
  if (!forecast || !offsets || !lo_rows || !hi_rows || !out) return SG_EINVAL;
  CfRoles roles;
  if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &roles)) return SG_EINVAL;
  const size_t total = (size_t)count * Q * H * N;
  const CfGrouping gr = cf_grouping(per_step, per_node, H, N);
  CfApplyPlan pl;                                   // VEC, the grid and its cap: calibration_plan.h
  cf_apply_plan(count, Q, H, N, sg_aligned16(forecast) && sg_aligned16(out), sg_num_cus(), &pl);
  const unsigned blocks = pl.blocks;
  if (pl.vec == 4)
    hipLaunchKernelGGL(cf_apply<4>, dim3(blocks), dim3(CF_THREADS), 0, (hipStream_t)stream, forecast, offsets, total, Q, H, N,
                       roles, gr.Hg, gr.Ng, out);
  else
    hipLaunchKernelGGL(cf_apply<1>, dim3(blocks), dim3(CF_THREADS), 0, (hipStream_t)stream, forecast, offsets, total, Q, H, N,
                       roles, gr.Hg, gr.Ng, out);
  SG_TRY(hipGetLastError());
  return 0;
}
