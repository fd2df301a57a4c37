// Scenario events: weighted aggregates over node sets and the crossing counts of sampled paths
// (include/stemgnn_hip.h: stemgnn_scenario_aggregate / stemgnn_scenario_events).
//
// aggregate: x [rows, N] fp32 -> out [rows, R] fp32, out[row, r] = sum_n weights[r, n] * v_n over the nodes with a non-zero
//            weight, v_n the value de-normalised to fp64 where it is loaded.  One wave owns a row at a time and a workgroup of
//            four waves walks rows b * 4 + w, + 4 * grid, ..: x is streamed once (lane l reads the nodes 4 l .. 4 l + 3 of every
//            256-node pass with one 16-byte load, or node l of every 64-node pass on the scalar path; the next row's first load
//            is issued ahead of the current row's arithmetic).  The weights, mul and add of a lane's nodes are loaded once per
//            workgroup, into one of three places (RB = R rounded up to a power of two, the groups beyond R weigh zero):
//            the lane's own registers when a row is one pass and a lane has at most 32 weights (N <= 256, R <= 8 on the 16-byte
//            path: PEMS07 with 8 groups); else LDS as [RB + 2][Np] doubles (Np = N rounded up to 4), where a lane reads its four
//            consecutive doubles of a row with two 16-byte reads, consecutive lanes consecutive addresses; else, where that
//            table is beyond 64 KB, global memory (the three arrays stay in L2).  A pass whose values are all finite in the
//            wave takes plain FMAs -- a zero weight then leaves its node out by itself, bit for bit -- and only a pass that
//            holds a NaN or an infinity takes the select on the weight.
//            Every lane keeps RB fp64 partials over its passes in pass order; the lanes meet in a fixed butterfly: while
//            more than one partial is left a lane keeps one half of its partials and hands the other to the lane `mask` away
//            (masks 32, 16, ..), then the lanes that hold the same r add up over the remaining masks.  RB - 1 + 6 - log2(RB)
//            exchanges instead of 6 RB; the order is a function of N and R alone.
// events:    the kernel of path_events.h (ev_kernel<false>: every path counts once), shared with weighted.hip.
// One launch each, no allocation, no memset, no global atomics, nothing floating-point that depends on arrival order: the same
// bits on every run, capturable.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "path_events.h"
#include "scenario_math.h"
#include "sg_host.h"

namespace {

constexpr int AG_THREADS = 256;
constexpr int AG_WAVES = AG_THREADS / 64;
constexpr int AG_MAX_R = 32;
constexpr int AG_MAX_N = 4096;
constexpr int AG_LDS_BYTES = 64 * 1024;     // the table of weights, mul and add; beyond it they are read from global memory
constexpr int AG_MAX_BLOCKS = 2048;         // 256 CUs x 8 workgroups: the rows beyond are walked
constexpr int EV_MAX_S = 1024;

struct AgArgs {
  const float* x;                           // [rows, N]
  const double* w;                          // [R, N]
  const double* mul;                        // [N] or NULL
  const double* add;
  float* out;                               // [rows, R]
  long long rows;
  int N, R, Np;
};

template <int VEC>
struct AgVec {
  float v[VEC];
};

template <int VEC>
__device__ inline AgVec<VEC> ag_load(const float* p) {
  AgVec<VEC> r;
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
  } else {
    r.v[0] = *p;
  }
  return r;
}

// The RB partials of the 64 lanes summed in a fixed butterfly; returns the sum of group *r in the lanes whose low
// log2(64 / RB) bits are anything (every lane of a group holds it).
template <int RB>
__device__ inline double ag_tree(double (&acc)[RB], int lane, int* r) {
  int which = 0;
#pragma unroll
  for (int half = RB / 2, mask = 32; half >= 1; half >>= 1, mask >>= 1) {
    const bool up = (lane & mask) != 0;
#pragma unroll
    for (int i = 0; i < half; ++i) {
      const double lo = acc[i], hi = acc[i + half];
      acc[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, mask);
    }
    which += up ? half : 0;
  }
  double s = acc[0];
#pragma unroll
  for (int mask = 32 / RB; mask >= 1; mask >>= 1) s += __shfl_xor(s, mask);
  *r = which;
  return s;
}

// where the weights, mul and add of a lane's nodes live: in its registers (one pass over the row and at most 32 weights per
// lane), in the LDS table, or in global memory
enum { AG_REG = 0, AG_LDS = 1, AG_GLOBAL = 2 };

template <int RB, int VEC, int SRC>
__global__ __launch_bounds__(AG_THREADS) void ag_kernel(const AgArgs a) {
  extern __shared__ double ag_lds[];                           // AG_LDS: [RB + 2][Np]
  const int N = a.N, R = a.R, Np = a.Np, t = threadIdx.x, lane = t & 63;
  const bool dn = a.mul != nullptr;
  const int first = lane * VEC;
  double wr[RB][VEC], mur[VEC], adr[VEC];                      // AG_REG
  if constexpr (SRC == AG_REG) {
#pragma unroll
    for (int k = 0; k < VEC; ++k) {
      const int n = first + k;
      const bool live = n < N;
      mur[k] = (dn && live) ? a.mul[n] : 1.0;
      adr[k] = (dn && live) ? a.add[n] : 0.0;
#pragma unroll
      for (int r = 0; r < RB; ++r) wr[r][k] = (r < R && live) ? a.w[(size_t)r * N + n] : 0.0;
    }
  }
  if constexpr (SRC == AG_LDS) {
    for (int i = t; i < (RB + 2) * Np; i += AG_THREADS) {
      const int r = i / Np, n = i - r * Np;
      double v = 0.0;
      if (n < N) {
        if (r < RB) v = r < R ? a.w[(size_t)r * N + n] : 0.0;
        else if (r == RB) v = dn ? a.mul[n] : 1.0;
        else v = dn ? a.add[n] : 0.0;
      }
      ag_lds[i] = v;
    }
    __syncthreads();
  }
  const long long stride = (long long)gridDim.x * AG_WAVES;
  long long row = (long long)blockIdx.x * AG_WAVES + (t >> 6);
  AgVec<VEC> cur = {};
  if (row < a.rows && first < N) cur = ag_load<VEC>(a.x + (size_t)row * N + first);
  for (; row < a.rows; row += stride) {
    const float* xr = a.x + (size_t)row * N;
    AgVec<VEC> nxt = {};
    if (row + stride < a.rows && first < N) nxt = ag_load<VEC>(a.x + (size_t)(row + stride) * N + first);
    double acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.0;
    for (int n0 = first; n0 < N; n0 += 64 * VEC) {
      const AgVec<VEC> xv = n0 == first ? cur : ag_load<VEC>(xr + n0);
      double v[VEC];
      bool finite = true;
#pragma unroll
      for (int k = 0; k < VEC; ++k) {
        double mu, ad;
        if constexpr (SRC == AG_REG) {
          mu = mur[k]; ad = adr[k];
        } else if constexpr (SRC == AG_LDS) {
          mu = ag_lds[RB * Np + n0 + k]; ad = ag_lds[(RB + 1) * Np + n0 + k];
        } else {
          mu = dn ? a.mul[n0 + k] : 1.0; ad = dn ? a.add[n0 + k] : 0.0;
        }
        v[k] = sg_dn(xv.v[k], dn, mu, ad);
        finite = finite && fabs(v[k]) < __builtin_inf();       // false for a NaN too
      }
      // A weight of exactly 0 leaves its node out.  Where every value of the wave's pass is finite the plain FMA does that by
      // itself (0 * v = +-0, and acc is never -0), bit for bit; the select is for the pass that holds a NaN or an infinity.
      const bool plain = __all(finite) != 0;
#pragma unroll
      for (int r = 0; r < RB; ++r) {
        double w[VEC];
        if constexpr (SRC == AG_REG) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) w[k] = wr[r][k];
        } else if constexpr (SRC == AG_LDS) {
          if constexpr (VEC == 4) {
            const double2 w0 = *reinterpret_cast<const double2*>(&ag_lds[r * Np + n0]);
            const double2 w1 = *reinterpret_cast<const double2*>(&ag_lds[r * Np + n0 + 2]);
            w[0] = w0.x; w[1] = w0.y; w[2] = w1.x; w[3] = w1.y;
          } else {
            w[0] = ag_lds[r * Np + n0];
          }
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) w[k] = r < R ? a.w[(size_t)r * N + n0 + k] : 0.0;
        }
        if (plain) {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[r] = fma(w[k], v[k], acc[r]);
        } else {
#pragma unroll
          for (int k = 0; k < VEC; ++k) acc[r] = w[k] != 0.0 ? fma(w[k], v[k], acc[r]) : acc[r];
        }
      }
    }
    int r;
    const double s = ag_tree<RB>(acc, lane, &r);
    if ((lane & (64 / RB - 1)) == 0 && r < R) a.out[(size_t)row * R + r] = (float)s;
    cur = nxt;
  }
}

template <int RB>
int ag_launch(const AgArgs& a, int grid, bool vec, hipStream_t st) {
  const size_t lds = (size_t)(RB + 2) * a.Np * sizeof(double);
  const int per = vec ? 4 : 1;
  const bool in_regs = a.N <= 64 * per && RB * per <= 32, in_lds = lds <= (size_t)AG_LDS_BYTES;
  const dim3 g(grid), b(AG_THREADS);
  if (in_regs && vec) hipLaunchKernelGGL((ag_kernel<RB, 4, AG_REG>), g, b, 0, st, a);
  else if (in_regs) hipLaunchKernelGGL((ag_kernel<RB, 1, AG_REG>), g, b, 0, st, a);
  else if (in_lds && vec) hipLaunchKernelGGL((ag_kernel<RB, 4, AG_LDS>), g, b, lds, st, a);
  else if (in_lds) hipLaunchKernelGGL((ag_kernel<RB, 1, AG_LDS>), g, b, lds, st, a);
  else if (vec) hipLaunchKernelGGL((ag_kernel<RB, 4, AG_GLOBAL>), g, b, 0, st, a);
  else hipLaunchKernelGGL((ag_kernel<RB, 1, AG_GLOBAL>), g, b, 0, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" int stemgnn_scenario_aggregate(const float* x, const double* weights, const double* mul, const double* add,
                                          long long rows, int N, int R, float* out, void* stream) {
  if (!x || !weights || !out) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  if (rows <= 0 || N <= 0 || R <= 0 || R > AG_MAX_R || N > AG_MAX_N) return SG_EINVAL;
  if (rows >= (1ll << 31) || !sg_fits_int(rows * R)) return SG_EINVAL;
  AgArgs a = {};
  a.x = x; a.w = weights; a.mul = mul; a.add = add; a.out = out;
  a.rows = rows; a.N = N; a.R = R; a.Np = (N + 3) & ~3;
  const long long want = (rows + AG_WAVES - 1) / AG_WAVES;
  const int grid = (int)(want < AG_MAX_BLOCKS ? want : AG_MAX_BLOCKS);
  const bool vec = N % 4 == 0 && sg_aligned16(x);
  hipStream_t st = (hipStream_t)stream;
  if (R == 1) return ag_launch<1>(a, grid, vec, st);
  if (R == 2) return ag_launch<2>(a, grid, vec, st);
  if (R <= 4) return ag_launch<4>(a, grid, vec, st);
  if (R <= 8) return ag_launch<8>(a, grid, vec, st);
  if (R <= 16) return ag_launch<16>(a, grid, vec, st);
  return ag_launch<32>(a, grid, vec, st);
}

extern "C" int stemgnn_scenario_events(const float* paths, const double* thr, const double* mul, const double* add, long count,
                                       int S, int H, int M, int above, int min_run, int* counts, void* stream) {
  if (!paths || !thr || !counts) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  if (count <= 0 || S <= 0 || H <= 0 || M <= 0 || S > EV_MAX_S) return SG_EINVAL;
  EvArgs a = {};
  a.paths = paths; a.thr = thr; a.mul = mul; a.add = add; a.counts = counts;
  a.S = S; a.H = H; a.M = M; a.above = above; a.min_run = min_run;
  return ev_launch<false>(a, count, (hipStream_t)stream);
}
