// Scenario reduction by forward selection (Heitsch & Roemisch 2003): pairwise distances of sampled paths and the greedy pick of
// K representatives with redistributed weights (include/stemgnn_hip.h: stemgnn_scenario_distances / stemgnn_scenario_reduce;
// DESIGN.md section 5s).
//
// distances: the tile of path_distance.h over the whole trajectory (pd_tile, unstaged): D [count, S, S] from paths [count, S, L].
// reduce:    the pick of forward_select.h with every path counting once (fs_pick, not WEIGHTED): no multiplicities are read or
//            kept, the costs are over S.
// The two entries here are the kernels' names, for the profiles and the timing tools, and the argument checks.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "forward_select.h"
#include "path_distance.h"
#include "sg_host.h"

namespace {

// NG wave groups of 256 threads: 1, or PD_NQ (one per partial sum)
template <bool SCALED, int NG>
__global__ __launch_bounds__(PD_THREADS * NG) void rd_distance_kernel(const PdArgs a) {
  pd_tile<SCALED, NG, false>(a, 1, nullptr);
}

template <bool IN_LDS>
__global__ __launch_bounds__(1024) void rd_pick_kernel(const FsPickArgs a) {
  fs_pick<false, IN_LDS>(a);
}

}  // namespace

extern "C" int stemgnn_scenario_distances(const float* paths, const double* scale, long count, int S, int L, int squared,
                                          double* D, void* stream) {
  if (!paths || !D) return SG_EINVAL;
  if (count <= 0 || S <= 0 || L <= 0 || S > FS_MAX_S || (squared != 0 && squared != 1)) return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)S * L) || !sg_fits_int((long long)count * S * S)) return SG_EINVAL;
  PdArgs a = {};
  a.paths = paths; a.scale = scale; a.D = D; a.S = S; a.L = L; a.squared = squared;
  static void (*const kern[2][2])(PdArgs) = {{rd_distance_kernel<false, 1>, rd_distance_kernel<false, PD_NQ>},
                                             {rd_distance_kernel<true, 1>, rd_distance_kernel<true, PD_NQ>}};
  return pd_launch(a, count, kern, (hipStream_t)stream);
}

extern "C" int stemgnn_scenario_reduce(const double* D, long count, int S, int K, int* selected, int* counts, int* assign,
                                       double* cost, void* stream) {
  if (!D || !selected || !counts || !assign || !cost) return SG_EINVAL;
  if (count <= 0 || S <= 0 || S > FS_MAX_S || K < 1 || K > S) return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)count * S * S)) return SG_EINVAL;
  FsPickArgs a = {};
  a.D = D; a.selected = selected; a.counts = counts; a.assign = assign; a.cost = cost; a.S = S; a.K = K; a.W = S;
  return fs_launch<rd_pick_kernel<true>, rd_pick_kernel<false>>(a, 1, count, (hipStream_t)stream);
}
