// The serving epilogue of a quantile forecast (include/stemgnn_hip.h: stemgnn_quantile_finish / _store):
// a column's Q values put in order and widened by the conformal offsets, in one launch.  finish writes the column back where
// it came from (or to `out`); store writes it to the result slab row pos[0] + b and copies the batch's target beside it.
// The kernel, its argument struct and its launch are quantile_column.h (shared with seasonal.hip), run here without a season;
// this file holds the two entries and their checks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "conformal_args.h"
#include "quantile_column.h"
#include "sg_host.h"

namespace {

// the stage arguments both entries share; fills offsets and Q .. roles of `a`
bool qs_stages_ok(long count, int Q, int H, int N, int rearrange, const float* offsets, int P, const int* lo_rows,
                  const int* hi_rows, int per_step, int per_node, QcArgs* a) {
  if (count <= 0 || Q <= 0 || H <= 0 || N <= 0 || Q > CF_MAX_Q || (long long)H * N >= (1ll << 31)) return false;
  a->roles = CfRoles{};
  if (offsets) {
    if (!lo_rows || !hi_rows) return false;
    if (!cf_shapes_ok(count, Q, H, N, P) || !cf_pairs_ok(Q, P, lo_rows, hi_rows, &a->roles)) return false;
  }
  qc_stages(a, Q, H, N, rearrange, offsets, per_step, per_node);
  return true;
}

}  // namespace

extern "C" int stemgnn_quantile_finish(const float* forecast, long count, int Q, int H, int N, int rearrange,
                                       const float* offsets, int P, const int* lo_rows, const int* hi_rows, int per_step,
                                       int per_node, float* out, void* stream) {
  if (!forecast || !out) return SG_EINVAL;
  QcArgs a = {};
  if (!qs_stages_ok(count, Q, H, N, rearrange, offsets, P, lo_rows, hi_rows, per_step, per_node, &a)) return SG_EINVAL;
  a.src = forecast;
  a.dst = out;
  return qc_launch(a, count, qc_vec_ok(N, Q, forecast, out), QcNoSeason{}, (hipStream_t)stream);
}

extern "C" int stemgnn_quantile_store(const float* steps, const float* target, const long long* pos, int B, int Q, int H,
                                      int N, int rearrange, const float* offsets, int P, const int* lo_rows,
                                      const int* hi_rows, int per_step, int per_node, float* out_forecast, float* out_target,
                                      long capacity, void* stream) {
  if (!steps || !target || !pos || !out_forecast || !out_target || capacity <= 0) return SG_EINVAL;
  QcArgs a = {};
  if (!qs_stages_ok(B, Q, H, N, rearrange, offsets, P, lo_rows, hi_rows, per_step, per_node, &a)) return SG_EINVAL;
  a.src = steps;
  a.dst = out_forecast;
  qc_store_to(&a, target, pos, out_target, capacity);
  return qc_launch(a, B, qc_vec_ok(N, Q, steps, out_forecast), QcNoSeason{}, (hipStream_t)stream);
}
