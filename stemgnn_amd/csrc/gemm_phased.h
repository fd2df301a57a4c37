// Phased form of the small-product kernel (gemm_core.h, 32 x 32 tiles, TWO_LEVEL): the same MFMA stream on the same LDS
// values -- hence the same bits -- with the operand loads following each operand's contiguous axis.
//
// sg_gemm_f32 has ONE compile-time walk order per operand for the whole launch.  Several graph products serve two
// differently laid-out problems through it (ChebBwd1: z = 0 / z = 1; ChebBwd2: k < N / k >= N; the two-block dT product:
// block 0's [B, W, N] window / block 1's [B, N, W] backcast), so one of the two is loaded against the grain: every lane
// of a wave on another row.  Here an op describes its problem as a static list of PHASES, pieces (z, K range) in each of
// which both operands have one layout (users: ChebBwd1, GFT forward / dX / two-block dT; ChebBwd2 measured slower in
// this form and stays on the core):
//   * blockIdx.z picks a fully specialised body (a wave-uniform switch), the K phases are a compile-time unrolled outer
//     loop around the tile loop: no per-element or per-tile run-time choice of map.
//   * per phase each operand is walked k-fastest or i / j-fastest.  A wave's ds_write_b32 is served in two groups of 32
//     lanes on 32 banks (MI355X_MICROARCH.md, LDS table).  BM = BN = 32, so an i / j-fastest group is the 32 consecutive
//     words of one LDS row: conflict-free at any row stride.  A k-fastest group is 32 rows at one column: conflict-free
//     iff the stride is odd.  Hence per operand: stride 32 + 17 if any of its phases (of this z) walks k fastest, else
//     32 + 16 -- the core's rule, and one stride per operand so that a tile staged by two phases is one LDS image.
//   * operand addresses are separable, off = row(i) + col(k): the ops hand out the two parts, so an index decomposition
//     (the (kq, n) / (b, t) divmods of the dG and X operands) is done once per thread and tile row / column, not per
//     element, and in 32-bit arithmetic (the launchers check the extents).
//   * a K tile that straddles a phase boundary is staged as two pieces, one per phase, each through its own walk with the
//     other phase's rows masked; the MFMA loop and the TWO_LEVEL flush run once per tile, after the same k as in the core.
//   * edge handling and prefetch as in the core: loads from clamped (always valid) indices, then select; tile t+1 (or the
//     next piece) is loaded into registers before the MFMA loop of tile t, also across a phase change.
//
// Op interface (Z = blockIdx.z, P = K phase; K starts at 0):
//   static constexpr int NZ, NPH (<= 2);
//   template <int Z, int P> static constexpr bool akf(), bkf();      // walk k fastest?
//   bool setup(int z, int& M, int& N, int& K) const;   int pend() const;   // end of K phase 0 when NPH == 2
//   template <int Z, int P> int arow(int i), acol(int k), brow(int k), bcol(int j) const;   // k: index in the whole K range
//   template <int Z, int P> float aval(int off), bval(int off) const;
//   void epi(int z, int i, int j, float v) const;
#pragma once
#include <stdlib.h>

#include "gemm_core.h"

template <int I>
struct sg_ic {
  static constexpr int value = I;
};

template <class Op, int BK, int Z>
__device__ __forceinline__ void sg_phased_body(const Op& op, float* lds) {
  constexpr int NPH = Op::NPH;
  static_assert(NPH == 1 || NPH == 2, "phases");
  static_assert(BK % 16 == 0 && (BK & (BK - 1)) == 0, "BK");
  constexpr bool LAST_AKF = Op::template akf<Z, NPH - 1>(), LAST_BKF = Op::template bkf<Z, NPH - 1>();
  constexpr int SA = 32 + ((Op::template akf<Z, 0>() || LAST_AKF) ? 17 : 16);
  constexpr int SB = 32 + ((Op::template bkf<Z, 0>() || LAST_BKF) ? 17 : 16);
  constexpr int R = 32 * BK / 256;      // staged elements per thread and operand
  float* As = lds;
  float* Bs = lds + BK * 49;

  int M, N, K;
  if (!op.setup(Z, M, N, K)) return;
  const int m0 = blockIdx.x * 32;
  const int n0 = blockIdx.y * 32;
  if (m0 >= M || n0 >= N) return;
  int pb[NPH + 1];                      // phase p covers k in [pb[p], pb[p + 1])
  pb[0] = 0;
  pb[NPH] = K;
  if constexpr (NPH == 2) pb[1] = op.pend();

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;

  sg_f32x4 acc = (sg_f32x4){0.f, 0.f, 0.f, 0.f}, acc2 = (sg_f32x4){0.f, 0.f, 0.f, 0.f};
  float ra[R], rb[R];

  // one piece: the rows of K tile kb that lie in phase P (the last phase also owns the zero padding behind K); loads from
  // clamped (always valid) indices, then select, as in the core
  auto gload = [&](auto pc, int kb) {
    constexpr int P = decltype(pc)::value;
    const int lo = pb[P], hi = pb[P + 1];
    auto ck = [&](int gk) { return gk < lo ? lo : (gk < hi ? gk : hi - 1); };
    if constexpr (Op::template akf<Z, P>()) {
      const int gk = kb + tid % BK;
      const int co = op.template acol<Z, P>(ck(gk));
      const bool kin = gk >= lo && gk < hi;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int gi = m0 + tid / BK + (256 / BK) * r;
        const float v = op.template aval<Z, P>(op.template arow<Z, P>(gi < M ? gi : M - 1) + co);
        ra[r] = (gi < M && kin) ? v : 0.f;
      }
    } else {
      const int gi = m0 + (tid & 31);
      const int ro = op.template arow<Z, P>(gi < M ? gi : M - 1);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int gk = kb + (tid >> 5) + 8 * r;
        const float v = op.template aval<Z, P>(ro + op.template acol<Z, P>(ck(gk)));
        ra[r] = (gi < M && gk >= lo && gk < hi) ? v : 0.f;
      }
    }
    if constexpr (Op::template bkf<Z, P>()) {
      const int gk = kb + tid % BK;
      const int ro = op.template brow<Z, P>(ck(gk));
      const bool kin = gk >= lo && gk < hi;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int gj = n0 + tid / BK + (256 / BK) * r;
        const float v = op.template bval<Z, P>(ro + op.template bcol<Z, P>(gj < N ? gj : N - 1));
        rb[r] = (gj < N && kin) ? v : 0.f;
      }
    } else {
      const int gj = n0 + (tid & 31);
      const int co = op.template bcol<Z, P>(gj < N ? gj : N - 1);
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int gk = kb + (tid >> 5) + 8 * r;
        const float v = op.template bval<Z, P>(op.template brow<Z, P>(ck(gk)) + co);
        rb[r] = (gj < N && gk >= lo && gk < hi) ? v : 0.f;
      }
    }
  };
  // a row of the tile is written by the phase that owns it; with one phase the mask is compile-time true
  auto lstore = [&](auto pc, int kb) {
    constexpr int P = decltype(pc)::value;
    const int lo = pb[P], hi = pb[P + 1];
    auto mine = [&](int gk) { return (P == 0 || gk >= lo) && (P == NPH - 1 || gk < hi); };
    if constexpr (Op::template akf<Z, P>()) {
      const int k = tid % BK;
      if (mine(kb + k)) {
#pragma unroll
        for (int r = 0; r < R; ++r) As[k * SA + tid / BK + (256 / BK) * r] = ra[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = (tid >> 5) + 8 * r;
        if (mine(kb + k)) As[k * SA + (tid & 31)] = ra[r];
      }
    }
    if constexpr (Op::template bkf<Z, P>()) {
      const int k = tid % BK;
      if (mine(kb + k)) {
#pragma unroll
        for (int r = 0; r < R; ++r) Bs[k * SB + tid / BK + (256 / BK) * r] = rb[r];
      }
    } else {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int k = (tid >> 5) + 8 * r;
        if (mine(kb + k)) Bs[k * SB + (tid & 31)] = rb[r];
      }
    }
  };

  const int fi = lane & 15;       // fragment row (A) / col (B)
  const int fk = lane >> 4;       // fragment k within the k-step of 4

  // the tiles of phase P; a tile that straddles the end of the phase gets its second piece from the next phase's
  // loader and is finished (MFMA loop, flush) at the top of the next phase's loop
  auto phase = [&](auto pc) {
    constexpr int P = decltype(pc)::value;
    constexpr bool LAST = P == NPH - 1;
    using Next = sg_ic<LAST ? P : P + 1>;
    const int hi = pb[P + 1];
    for (int kb = pb[P] & ~(BK - 1); kb < hi; kb += BK) {
      lstore(pc, kb);
      if constexpr (!LAST) {
        if (kb + BK > hi) {
          gload(Next{}, kb);
          break;
        }
      }
      __syncthreads();
      if (kb + BK < hi) gload(pc, kb + BK);
      else if constexpr (!LAST) gload(Next{}, kb + BK);
#pragma unroll
      for (int ks = 0; ks < BK; ks += 4) {
        const float af = As[(ks + fk) * SA + wm * 16 + fi];
        const float bf = Bs[(ks + fk) * SB + wn * 16 + fi];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, acc, 0, 0, 0);
      }
      acc2 += acc;
      acc = (sg_f32x4){0.f, 0.f, 0.f, 0.f};
      __syncthreads();
    }
  };

  gload(sg_ic<0>{}, 0);
  phase(sg_ic<0>{});
  if constexpr (NPH == 2) phase(sg_ic<1>{});

  // epilogue: D layout of 16x16 MFMA: col = lane & 15, row = (lane >> 4) * 4 + reg
  const int gj = n0 + wn * 16 + fi;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int gi = m0 + wm * 16 + fk * 4 + reg;
    if (gi < M && gj < N) op.epi(Z, gi, gj, acc2[reg]);
  }
}

template <class Op, int BK>
__global__ __launch_bounds__(256) void sg_gemm_phased_f32(const Op op) {
  static_assert(Op::NZ == 1 || Op::NZ == 2, "z");
  __builtin_amdgcn_s_setprio(SG_CHAIN_PRIO);      // as in the core: these launches share CUs with the weight-gradient launch
  __shared__ float lds[2 * BK * 49];
  if constexpr (Op::NZ == 2) {
    if (blockIdx.z == 1) {
      sg_phased_body<Op, BK, 1>(op, lds);
      return;
    }
  }
  sg_phased_body<Op, BK, 0>(op, lds);
}

template <class Op, int BK = 128>
static inline hipError_t sg_launch_phased(const Op& op, int maxM, int maxN, hipStream_t stream) {
  dim3 grid((maxM + 31) / 32, (maxN + 31) / 32, Op::NZ);
  if (grid.x == 0 || grid.y == 0) return hipSuccess;
  hipLaunchKernelGGL((sg_gemm_phased_f32<Op, BK>), grid, dim3(256), 0, stream, op);
  return hipGetLastError();
}

// STEMGNN_GRAPH_PHASED=0 selects the generic launches; read per call so that both forms can be compared in one process
static inline bool sg_graph_phased() {
  const char* e = getenv("STEMGNN_GRAPH_PHASED");
  return !(e && e[0] == '0' && e[1] == '\0');
}
