// Fused forward of the three GLU layers of a StockBlock on the bf16 matrix pipe (round 5): the csrc/glu_fused.h design with
// split-bf16 arithmetic inside (STEMGNN_DTYPE=bf16x2; BASELINE.json configs[1] names "bf16/fp32").
//
// v_mfma_f32_32x32x2_f32 runs at 1/16 of the rate of v_mfma_f32_32x32x16_bf16.  An fp32 number is hi + lo (two bf16 numbers)
// to 2^-17, so   a b ~ a_hi b_hi + a_hi b_lo + a_lo b_hi   (fp32 accumulation; ~2^-16 relative, csrc/gemm2s.h's S = 2) costs
// 3 x 32 cycles per 16 k where the exact product costs 8 x 64: 5.3 x less matrix time.  The round-4 split kernels were
// per-layer launches and lost to the fused fp32 kernel (1.25 vs 1.24 ms per step); this kernel keeps the fusion:
//   * a workgroup owns 64 series rows of one branch and walks all three layers; the row block's activations are resident in
//     LDS as TWO bf16 PLANES [plane][row][k] (k contiguous, row stride K + 8 elements = 4 * odd words: the 16-byte fragment
//     reads of a lane group of ds_read_b128 touch all 64 banks once), split when they are produced: G in the prologue,
//     every layer's `out` by the epilogue that forms it (in place: the K loop of a layer is over before its output exists);
//   * the weights arrive PRE-SPLIT (sg_pack_fused_bf16_kernel, once per step on the side stream) as one continuous stream of
//     16 KB stages in exactly the LDS image the fragment reads want -- stage = (16 k) x (256 pair columns: 4 waves x
//     {left, right} x 32 channels) x 2 planes, element order [plane][k half][wave][left|right][channel][8 k] -- moved by
//     global_load_lds_dwordx4 into the same 5-stage ring, one counted vmcnt wait and one raw barrier per stage;
//   * a wave owns all 64 rows x 32 HP channels, left and right map of a channel in the same lane: per stage 2 row tiles x
//     2 maps x 3 products = 12 MFMAs from 4 A + 4 B fragment reads (the A fragments of a k step are kept in registers
//     across its HP stages);
//   * epilogue = the fp32 kernel's (bias, sigmoid gate, saved fp32 `out` / `gate` in 128-byte row pieces) + the split of
//     `out` into the two planes of the next layer's operand.
// The saved tensors are fp32 as before, so the data-gradient chain, the weight gradients and the heads are unchanged.
// Applies where the fp32 fused kernel applies (padded channel count <= 256).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gemm2s.h"
#include "glu_fused.h"
#include "layout.h"

constexpr int GB_BM = 64;                 // series rows per workgroup
constexpr int GB_STAGE_E = 8192;          // bf16 elements per ring stage (16 KB = GF_STAGE floats)
constexpr int GB_STAGES = 5;
#ifndef GB_STORE_AUX
#define GB_STORE_AUX 2                    // cache policy of the saved-tensor / d(pre-activation) stores: nt.  They are 82 / 148 MB per
#endif                                    // launch that nobody reads before the backward pass; as streaming stores they stop evicting what
                                          // the step is about to use (measured A/B, same box: 1.1009 -> 1.0853 ms per step; 0 = default policy)
#ifndef GB_ABL
#define GB_ABL 0                          // timing-probe ablation bits (tools/build_variant.sh -DGB_ABL=n; results wrong by design):
#endif                                    // 1 no epilogue HBM stores, 2 no MFMA, 4 no DMA in the K loop, 8 no operand-plane writes, 16 no sigmoid

struct GbGeom {
  int hp[3];        // channel groups of 32 per wave, per layer
  int kp[3];        // K padded to the MFMA's 16
  int nst[3];       // stages per layer: kp / 16 * hp
  int ns;           // stages per branch
  int LDK;          // row stride of an activation plane (elements): max kp + 8
  size_t lds_bytes;
  bool ok;
};
SG_HD GbGeom gb_geom(const SgDims& d) {
  GbGeom g;
  const GfGeom f = gf_geom(d);
  int ka = 0;
  g.ns = 0;
  for (int l = 0; l < 3; ++l) {
    g.hp[l] = f.hp[l] < 1 ? 1 : (f.hp[l] > 2 ? 2 : f.hp[l]);
    const int K = l == 0 ? d.KG : d.CP;
    g.kp[l] = (K + 15) & ~15;
    g.nst[l] = g.kp[l] / 16 * g.hp[l];
    g.ns += g.nst[l];
    if (g.kp[l] > ka) ka = g.kp[l];
  }
  g.LDK = ka + 8;
  g.lds_bytes = (size_t)2 * GB_BM * g.LDK * 2 + (size_t)GB_STAGES * GB_STAGE_E * 2;
  g.ok = f.ok && d.CP <= 256 && g.lds_bytes <= (size_t)160 * 1024;
  return g;
}
// bf16 elements of the pre-split weight stream of one block (both branches)
SG_HD size_t gb_stream_elems(const SgDims& d) {
  const GbGeom g = gb_geom(d);
  return g.ok ? (size_t)2 * g.ns * GB_STAGE_E : 0;
}

// ---- weight stream ------------------------------------------------------------------------------------------------------
// element e of branch r: stage s = e / 8192 -> (layer l, k step ks = s / hp, channel group h = s % hp); inside the stage
// w = ((((plane * 2 + kh) * 4 + wave) * 2 + t) * 32 + fi) * 8 + j  ->  k = 16 ks + 8 kh + j, channel c = wave 32 hp + 32 h + fi,
// t = 0 linear_left / 1 linear_right.  Source: the K-major pair panel Wp[k][q], q = (c / 16) * 32 + c % 16 + 16 t (layout.h).
struct GbPackArgs {
  const float* wp[2][3];
  unsigned short* wf[2];
  int K[3], np[2][3], cp[2][3];
  GbGeom g;
};
static __global__ __launch_bounds__(256) void sg_pack_fused_bf16_kernel(const GbPackArgs a) {
  const int r = blockIdx.y;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.g.ns * GB_STAGE_E) return;
  int s = (int)(e / GB_STAGE_E), l = 0;
  while (l < 2 && s >= a.g.nst[l]) { s -= a.g.nst[l]; ++l; }
  const int hp = a.g.hp[l], ks = s / hp, h = s - ks * hp;
  const int w = (int)(e % GB_STAGE_E);
  const int j = w & 7, fi = (w >> 3) & 31, t = (w >> 8) & 1, wave = (w >> 9) & 3, kh = (w >> 11) & 1, plane = (w >> 12) & 1;
  const int k = 16 * ks + 8 * kh + j, c = wave * 32 * hp + 32 * h + fi;
  float v = 0.f;
  if (k < a.K[l] && c < a.cp[r][l]) v = a.wp[r][l][(size_t)k * a.np[r][l] + ((c >> 4) << 5) + (c & 15) + 16 * t];
  unsigned p[2];
  g2s_split<2>(v, p);
  a.wf[r][e] = (unsigned short)p[plane];
}

// ---- kernel -----------------------------------------------------------------------------------------------------------
struct GbArgs {
  const float* G;                   // [M][KG]
  const unsigned short* wf[2];      // pre-split weight stream per branch
  const float* bias[2][3];          // packed pair-order bias (left at q, right at q + 16)
  float* out[2][3];
  float* gate[2][3];
  int cp[2][3];                     // padded channel counts = row strides of out / gate
  int nst[3], kp[3];
  int KG, LDK, M, nrb, ns;
};

typedef __bf16 gb_bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 gb_bf2 __attribute__((ext_vector_type(2)));

// sigmoid on the hardware transcendentals (v_exp_f32, v_rcp_f32: ~1 ulp each).  csrc/glu_fused.h's gf_sigmoid uses the
// correctly-rounded reciprocal (a ~10-instruction division sequence) because the fp32 kernels must reproduce the per-layer
// kernels bit for bit; here the split products carry 2^-16 already and the epilogues are what bounds the kernel
__device__ __forceinline__ float gb_sigmoid(float v) {
  return __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(-1.44269504088896340736f * v));
}

// split of a PAIR of fp32 values into their bf16 hi / lo parts on the hardware converter (v_cvt_pk_bf16_f32, round to nearest
// even like csrc/gemm2s.h's g2s_split<2>): hi = {bf16(a), bf16(b)} packed a | b << 16, lo likewise of the remainders --
// 6 VALU instructions per pair against ~20 for two integer-arithmetic splits
__device__ __forceinline__ void gb_split_pair(float a, float b, unsigned& hi, unsigned& lo) {
  gb_bf2 h;
  h[0] = (__bf16)a; h[1] = (__bf16)b;
  hi = __builtin_bit_cast(unsigned, h);
  const float ra = a - __uint_as_float(hi << 16), rb = b - __uint_as_float(hi & 0xffff0000u);
  gb_bf2 l;
  l[0] = (__bf16)ra; l[1] = (__bf16)rb;
  lo = __builtin_bit_cast(unsigned, l);
}

// fragment reads live in __restrict__-parameter functions (alias-scope metadata: without it hipcc's waitcnt pass assumes an
// LDS read may alias the LDS-DMA in flight and drains the ring per read -- csrc/glu_fused.h)
__device__ __forceinline__ void gb_read_a(const unsigned short* __restrict__ Ap, int plane_stride, int tile_stride,
                                          gb_bf8 (&a)[2][2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int p = 0; p < 2; ++p)
      a[i][p] = __builtin_bit_cast(gb_bf8, *reinterpret_cast<const uint4*>(Ap + p * plane_stride + i * tile_stride));
}
__device__ __forceinline__ void gb_read_b(const unsigned short* __restrict__ Bp, gb_bf8 (&b)[2][2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int p = 0; p < 2; ++p)
      b[t][p] = __builtin_bit_cast(gb_bf8, *reinterpret_cast<const uint4*>(Bp + p * (GB_STAGE_E / 2) + t * 256));
}

// saved tensors of a layer as its epilogue forms them, stored through BUFFER stores: one per-lane offset, a scalar offset per
// (register, tile), rows >= M and dead channels fall outside num_records and are dropped -- no exec-mask branch per store.
// Row tiles here are block rows 32 i .. 32 i + 31.
// (Measured and NOT kept, round 5: issuing these stores from inside the NEXT layer's K loop, Q per ring stage, with the
// counted waits widened to "all but the youngest pieces + stores".  The stores of all workgroups hit the HBM as one burst that
// the next K loop's waits sit out -- with the stores ablated this kernel drops from 41 to 29 us -- but vmcnt counts loads and
// stores together and they do NOT retire in order relative to each other: under a chip-wide launch younger stores were
// acknowledged before older LDS-DMA pieces had landed, the wait returned early and the stage-level test read stale weights
// (small launches passed).  Only a wait that leaves no more than the younger LOADS outstanding is safe, i.e. the stores are
// waited for -- which is the original schedule.  De-phasing the two branches' workgroups by 2.5 / 6 us at kernel start, so
// that only half of them burst at a time: 43.0 / 44.8 us against 41.8 -- no gain either.)
template <int HP>
struct GbPend {
  float o[HP][2][16], gs[HP][2][16];
  __amdgpu_buffer_rsrc_t ro, rg;
  int voff[HP];
  int cp4;
  static constexpr int N = 2 * HP * 2 * 16;
  __device__ __forceinline__ void init(float* outp, float* gatep, int cp, int M, int m0, int lane, int wave) {
    const int fi = lane & 31, fk = lane >> 5;
    const unsigned bytes = (unsigned)((size_t)M * cp * 4);
    ro = __builtin_amdgcn_make_buffer_rsrc(outp, 0, bytes, 0x00020000);
    rg = __builtin_amdgcn_make_buffer_rsrc(gatep, 0, bytes, 0x00020000);
    cp4 = cp * 4;
#pragma unroll
    for (int h = 0; h < HP; ++h) {
      const int c = wave * 32 * HP + h * 32 + fi;
      voff[h] = ((m0 + 4 * fk) * cp + c) * 4 | (c < cp ? 0 : 0x7fffffff);      // dead channel / row >= M: outside num_records
    }
  }
  __device__ __forceinline__ void store(int e) const {
    const int t = e & 1, idx = e >> 1, h = idx / 32, rem = idx % 32, i = rem / 16, reg = rem % 16;
    const int so = __builtin_amdgcn_readfirstlane((32 * i + (reg & 3) + 8 * (reg >> 2)) * cp4);
    const float v = t ? gs[h][i][reg] : o[h][i][reg];
    if (!(GB_ABL & 1)) __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, v), t ? rg : ro, voff[h], so, GB_STORE_AUX);
  }
};

// One ring stage = one (k step, channel group h): 12 MFMAs, the next ring stage's four DMA pieces issued from inside.
// Products smallest first (a_lo b_hi, a_hi b_lo, a_hi b_hi), as csrc/gemm2s.h.
template <int H>
__device__ __forceinline__ void gb_stage(const gb_bf8 (&a)[2][2], const unsigned short* __restrict__ Bp,
                                         sg_f32x16 (&acc)[2][2][2], GfRing& rg) {
  gb_bf8 b[2][2];
  gb_read_b(Bp, b);
  int piece = 0;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      __builtin_amdgcn_sched_barrier(0);
      if (!(GB_ABL & 2)) acc[i][H][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[t][0], acc[i][H][t], 0, 0, 0);
      if (!(GB_ABL & 4)) rg.issue(piece);
      ++piece;
      __builtin_amdgcn_sched_barrier(0);
      if (!(GB_ABL & 2)) {
        acc[i][H][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[t][1], acc[i][H][t], 0, 0, 0);
        acc[i][H][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[t][0], acc[i][H][t], 0, 0, 0);
      } else {
        acc[i][H][t][0] += __builtin_bit_cast(float, __builtin_bit_cast(uint4, a[i][0]).x ^ __builtin_bit_cast(uint4, b[t][1]).y ^ __builtin_bit_cast(uint4, a[i][1]).z ^ __builtin_bit_cast(uint4, b[t][0]).w);
      }
    }
}

// operand planes of the next layer: this lane's channel column, rows of both tiles (through a __restrict__ pointer, see
// gf_write_operand)
__device__ __forceinline__ void gb_write_operand(unsigned short* __restrict__ a0, int plane_stride, int LDK, const float (&o)[2][16],
                                                 int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; reg += 2) {
      const int r0 = 32 * i + g2_row_of(reg, lane), r1 = 32 * i + g2_row_of(reg + 1, lane);
      unsigned hi, lo;
      gb_split_pair(o[i][reg], o[i][reg + 1], hi, lo);
      a0[r0 * LDK] = (unsigned short)hi;
      a0[r1 * LDK] = (unsigned short)(hi >> 16);
      a0[plane_stride + r0 * LDK] = (unsigned short)lo;
      a0[plane_stride + r1 * LDK] = (unsigned short)(lo >> 16);
    }
}

// INF: the inference forward (stemgnn_spectral_glu_fwd_split_infer) -- only the last layer's `out` is stored
template <int HP, bool LAST, bool INF = false>
__device__ __forceinline__ void gb_layer(unsigned short* Ab, int LDK, GfRing& rg, int& rbuf, int nk, int lane, int wave,
                                         const float (&bl)[2], const float (&br)[2], GbPend<HP>& next, int kcap) {
  const int fi = lane & 31, fk = (lane >> 5) << 3;
  sg_f32x16 acc[2][2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][h][t][e] = 0.f;
  const int plane_stride = GB_BM * LDK, tile_stride = 32 * LDK;
  const unsigned short* Ap = Ab + fi * LDK + fk;
  // this lane's B fragment inside a stage: [plane][kh = lane >> 5][wave][t][fi][8]
  const int boff = ((((lane >> 5) * 4 + wave) * 2) * 32 + fi) * 8;
  const unsigned short* ring = reinterpret_cast<const unsigned short*>(rg.ring);
  gb_bf8 a[2][2];
  for (int ks = 0; ks < nk; ++ks) {
#pragma unroll
    for (int h = 0; h < HP; ++h) {
      gf_wait_vm<(GB_STAGES - 2) * GF_NI>();             // my pieces of this stage have landed
      __builtin_amdgcn_s_barrier();                      // everybody's have; the buffer read last stage is free
      if (h == 0) gb_read_a(Ap + ks * 16, plane_stride, tile_stride, a);
      if (h == 0) gb_stage<0>(a, ring + (size_t)rbuf * GB_STAGE_E + boff, acc, rg);
      else gb_stage<1>(a, ring + (size_t)rbuf * GB_STAGE_E + boff, acc, rg);
      rg.advance();
      rbuf = rbuf + 1 == GB_STAGES ? 0 : rbuf + 1;
    }
  }
  // ---- epilogue: bias, GLU gating, next layer's operand planes, saved tensors -----------------------------------------------
  if constexpr (!LAST) __builtin_amdgcn_s_barrier();     // every wave is done reading the activation planes
#pragma unroll
  for (int h = 0; h < HP; ++h) {
    const int c = wave * 32 * HP + h * 32 + fi;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const float u = acc[i][h][0][reg] + bl[h], v = acc[i][h][1][reg] + br[h];
        next.gs[h][i][reg] = (GB_ABL & 16) ? v : gb_sigmoid(v);
        next.o[h][i][reg] = u * next.gs[h][i][reg];
        // INF: with its store gone, hipcc would contract the product into the operand split's remainder o - bf16(o) (an FMA
        // with a different rounding than the training kernel's multiply then subtract): keep the rounded product
        if constexpr (INF) asm volatile("" : "+v"(next.o[h][i][reg]));
      }
    if constexpr (!LAST) {
      if (c < kcap && !(GB_ABL & 8)) gb_write_operand(Ab + c, plane_stride, LDK, next.o[h], lane);   // (columns beyond the next K: never read)
    }
  }
#pragma unroll
  for (int e = 0; e < GbPend<HP>::N; ++e)
    if (!INF || (LAST && (e & 1) == 0)) next.store(e);        // (e & 1: the gate half of the pending values)
  if constexpr (!LAST) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // published by the next layer's first barrier
  if (GB_ABL & 1) {
    if (acc[0][0][0][0] + acc[1][HP - 1][1][7] == 1.2345e-30f) Ab[0] = 1;    // keep the accumulators alive
  }
}

template <int HP01, int HP2, bool INF = false>
static __global__ __launch_bounds__(256, 1) void sg_glu_fused_fwd_bf16_kernel(const GbArgs g) {
  extern __shared__ __attribute__((aligned(16))) float gb_lds[];   // ONE array: the two activation planes, then the ring
  unsigned short* Ab = reinterpret_cast<unsigned short*>(gb_lds);
  const int L = blockIdx.x, xcd = L & 7;
  const int r = (xcd >> 2) & 1, rb = (L >> 3) * 4 + (xcd & 3);      // XCDs 0-3 stream branch 0's weights, 4-7 branch 1's
  if (rb >= g.nrb) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fi = lane & 31;
  const int m0 = rb * GB_BM, M = g.M, LDK = g.LDK;

  GfRing rg;
  rg.ring = gb_lds + (size_t)GB_BM * LDK;                // 2 planes x 64 rows x LDK elements = 64 LDK floats
  rg.wave = wave;
  rg.nstages = GB_STAGES;
  rg.src = reinterpret_cast<const float*>(g.wf[r]) + (size_t)wave * GF_NI * 256 + lane * 4;
  rg.next = 0; rg.last = g.ns - 1; rg.wbuf = 0;
#pragma unroll
  for (int p = 0; p < GB_STAGES - 1; ++p) {
#pragma unroll
    for (int q = 0; q < GF_NI; ++q) rg.issue(q);
    rg.advance();
  }
  float bl[3][2], br[3][2];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    const int hp = l < 2 ? HP01 : HP2;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = wave * 32 * hp + h * 32 + fi;
      const bool ok = h < hp && c < g.cp[r][l];
      const int q = ((c >> 4) << 5) + (c & 15);
      const float* b = g.bias[r][l];
      const float x = b[ok ? q : 0], y = b[ok ? q + 16 : 0];
      bl[l][h] = ok ? x : 0.f;
      br[l][h] = ok ? y : 0.f;
    }
  }
  {  // layer-0 operand: the G rows of this block, split into the two planes; k = KG .. kp[0]-1 and rows beyond M are zero
    const int KG = g.KG, KP0 = g.kp[0];
    const float* Gp = g.G + (size_t)m0 * KG;
    const int nrow = M - m0 < GB_BM ? M - m0 : GB_BM;
    for (int idx = tid; idx < GB_BM * KP0; idx += 256) {
      const int i = idx / KP0, k = idx - i * KP0;
      const bool ok = i < nrow && k < KG;
      const float v = Gp[ok ? i * KG + k : 0];
      unsigned p[2];
      g2s_split<2>(ok ? v : 0.f, p);
      Ab[i * LDK + k] = (unsigned short)p[0];
      Ab[GB_BM * LDK + i * LDK + k] = (unsigned short)p[1];
    }
  }
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(bl[l][h]), "+v"(br[l][h]));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (the first stage's barrier publishes the planes)
  int rbuf = 0;
  GbPend<HP01> p0, p1;
  GbPend<HP2> p2;
  p0.init(g.out[r][0], g.gate[r][0], g.cp[r][0], M, m0, lane, wave);
  p1.init(g.out[r][1], g.gate[r][1], g.cp[r][1], M, m0, lane, wave);
  p2.init(g.out[r][2], g.gate[r][2], g.cp[r][2], M, m0, lane, wave);
  gb_layer<HP01, false, INF>(Ab, LDK, rg, rbuf, g.kp[0] / 16, lane, wave, bl[0], br[0], p0, g.kp[1]);
  gb_layer<HP01, false, INF>(Ab, LDK, rg, rbuf, g.kp[1] / 16, lane, wave, bl[1], br[1], p1, g.kp[2]);
  gb_layer<HP2, true, INF>(Ab, LDK, rg, rbuf, g.kp[2] / 16, lane, wave, bl[2], br[2], p2, 0);
  gf_wait_vm<0>();                                         // the run-ahead DMA pieces must not outlive the workgroup's LDS
}

// =======================================================================================================================
// Fused data-gradient chain of the GLU stack on the bf16 matrix pipe (round 5): csrc/glu_fused.h's sg_glu_fused_dgrad_kernel
// with split-bf16 products inside -- d(pre-activation) of layer 2 (from the heads' backward) -> layer 1 -> layer 0 -> dG in ONE
// launch per block.  Same structure as the fp32 chain:
//   * a workgroup owns 64 series rows of one branch; the operand of the running product is resident in LDS, here as two bf16
//     planes [plane][row][k] like the forward's: the d(pre-activation) rows of layer 2 are copied in from HBM (split on the
//     way), those of layers 1 / 0 are written there by the epilogue that forms them -- a lane's left / right pair of a
//     channel is two neighbouring k, i.e. ONE 4-byte LDS write per plane -- and stored to HBM once (fp32, pair order) for
//     the weight-gradient kernel;
//   * a wave owns 32 NT channels of the layer whose d(out) is being formed, for all 64 rows; the second product accumulates
//     into a second set while the first set is still being turned into its operand; the reduction of the second / third
//     product runs in NT phases of 256 rows (phase p = the left / right values of every wave's p-th channel group);
//   * GLU backward in the epilogue: left = d gate, right = d out (1 - gate), the saved fp32 out / gate of
//     the layer below requested with buffer loads from inside the last stages of the preceding K loop;
//   * the pre-split weight stream (sg_pack_dgrad_bf16_kernel) is laid out in exactly the order the phases consume it:
//     stages of 16 KB = [plane][k eighth][wave][column tile][channel][8 k] for the first two products (32 / NT k per stage),
//     [plane][k eighth][64 columns][8 k] (64 k per stage) for the third (-> the 3 W <= 64 columns of dG).
// 12 MFMAs (v_mfma_f32_32x32x16_bf16) per ring stage and wave in every product.
struct GqGeom {
  int nt;               // MFMA column tiles per wave
  int ks;               // k per ring stage of the first two products: 32 / nt
  int nstA[2];          // stages of the first product (layer-2 weights), per branch
  int nstB[2];          // stages of each phase of the second product (layer-1 weights)
  int nstC[2];          // stages (64 k) of each phase of the third product (layer 0 -> dG)
  int ns[2];            // stages per branch
  int LDK;              // row stride of an operand plane (elements)
  size_t lds_bytes;
  bool ok;
};
SG_HD GqGeom gq_geom(const SgDims& d) {
  GqGeom g;
  g.nt = d.CP > 128 ? 2 : 1;
  g.ks = 32 / g.nt;
  g.ok = d.CP <= 256 && d.KG <= 64;
  for (int r = 0; r < 2; ++r) g.nstA[r] = (2 * d.CP2[r] + g.ks - 1) / g.ks;
  for (int p = 0; p < 2; ++p) {
    int live = 0;                                   // (wave, lane) pairs of phase p whose channel exists
    for (int w = 0; w < 4; ++w)
      for (int fi = 0; fi < 32; ++fi)
        if (p < g.nt && w * 32 * g.nt + 32 * p + fi < d.CP) ++live;
    g.nstB[p] = (2 * live + g.ks - 1) / g.ks;
    g.nstC[p] = (2 * live + 63) / 64;
  }
  for (int r = 0; r < 2; ++r) g.ns[r] = g.nstA[r] + g.nstB[0] + g.nstB[1] + g.nstC[0] + g.nstC[1];
  g.LDK = 256 + 8;
  g.lds_bytes = (size_t)2 * GB_BM * g.LDK * 2 + (size_t)GB_STAGES * GB_STAGE_E * 2;
  g.ok = g.ok && g.lds_bytes <= (size_t)160 * 1024 && 2 * d.CP2[0] <= 256 && 2 * d.CP2[1] <= 256;
  return g;
}
SG_HD size_t gq_stream_elems(const SgDims& d, int r) {
  const GqGeom g = gq_geom(d);
  return g.ok ? (size_t)g.ns[r] * GB_STAGE_E : 0;
}

struct GqPackArgs {
  const float* wp[2][3];        // pair panels [K_in][NP] of layers 0, 1, 2
  unsigned short* wd[2];
  int np[2][3];
  int CP, KG;
  GqGeom g;
};
static __global__ __launch_bounds__(256) void sg_pack_dgrad_bf16_kernel(const GqPackArgs a) {
  const int r = blockIdx.y;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.g.ns[r] * GB_STAGE_E) return;
  int s = (int)(e / GB_STAGE_E);
  const int w = (int)(e % GB_STAGE_E);
  const int plane = w >> 12, wi = w & 4095;
  const int nt = a.g.nt, ks = a.g.ks;
  const int sAB = a.g.nstA[r] + a.g.nstB[0] + a.g.nstB[1];
  float v = 0.f;
  if (s >= sAB) {                                    // third product: [k eighth < 8][col < 64][8]
    s -= sAB;
    int ph = 0;
    if (s >= a.g.nstC[0]) { s -= a.g.nstC[0]; ph = 1; }
    const int kq = wi >> 9, col = (wi >> 3) & 63, j8 = wi & 7;
    const int k2 = s * 64 + 8 * kq + j8;             // row of the phase: 2 (wave' 32 + lane') + t
    const int t = k2 & 1, wf = k2 >> 1, w2 = wf >> 5, f2 = wf & 31;
    const int c2 = w2 * 32 * nt + 32 * ph + f2;      // layer-0 channel whose left / right value the row holds
    if (w2 < 4 && c2 < a.CP && col < a.KG) v = a.wp[r][0][(size_t)col * a.np[r][0] + ((c2 >> 4) << 5) + (c2 & 15) + 16 * t];
  } else {                                           // first / second product: [k eighth < ks / 8][wave][j < nt][fi][8]
    const int j8 = wi & 7, fi = (wi >> 3) & 31;
    const int rest = wi >> 8;                        // (kq * 4 + wave) * nt + j
    const int j = rest % nt, wave = (rest / nt) & 3, kq = rest / (4 * nt);
    const int c = wave * 32 * nt + 32 * j + fi;      // output column of the product = input channel of the layer
    const int kk = 8 * kq + j8;
    if (s < a.g.nstA[r]) {                           // layer 2: reduction row = natural pair column
      const int q = s * ks + kk;
      if (q < a.np[r][2] && c < a.CP) v = a.wp[r][2][(size_t)c * a.np[r][2] + q];
    } else {                                         // layer 1: reduction rows in phase order
      s -= a.g.nstA[r];
      int ph = 0;
      if (s >= a.g.nstB[0]) { s -= a.g.nstB[0]; ph = 1; }
      const int k2 = s * ks + kk;
      const int t = k2 & 1, wf = k2 >> 1, w2 = wf >> 5, f2 = wf & 31;
      const int c2 = w2 * 32 * nt + 32 * ph + f2;
      if (w2 < 4 && c2 < a.CP && c < a.CP) v = a.wp[r][1][(size_t)c * a.np[r][1] + ((c2 >> 4) << 5) + (c2 & 15) + 16 * t];
    }
  }
  unsigned p[2];
  g2s_split<2>(v, p);
  a.wd[r][e] = (unsigned short)p[plane];
}

struct GqArgs {
  const float* dact2[2];        // [M][np2[r]]   d(pre-activation) of layer 2, pair order
  const unsigned short* wd[2];  // pre-split weight stream
  const float* out1[2];         // saved out / gate of layers 1 and 0, [M][CP]
  const float* gate1[2];
  const float* out0[2];
  const float* gate0[2];
  float* dact1[2];              // [M][2 CP]  d(pre-activation) of layers 1 and 0, pair order
  float* dact0[2];
  float* dG[2];                 // [M][KG]
  int np2[2], nstA[2], ns[2];
  int nstB[2], nstC[2];
  int CP, KG, M, nrb, LDK;
};

// saved out / gate values one epilogue tile needs (64 rows x 1 channel per lane and tensor), requested in GQ_NB batches from
// inside the last stages of the K loop that precedes the epilogue (csrc/glu_fused.h, gd_load_batch)
constexpr int GQ_NB = 8;
struct GqSaved {
  float y[2][16], g[2][16];
};
template <int NT, int J>
__device__ __forceinline__ void gq_load_batch(GqSaved& sv, int b, const float* __restrict__ y, const float* __restrict__ gt,
                                              int CP, int M, int m0, int lane, int wave) {
  const int fi = lane & 31, fk = lane >> 5;
  const int c = wave * 32 * NT + 32 * J + fi;
  const unsigned bytes = (unsigned)((size_t)M * CP * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(y), 0, bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gt), 0, bytes, 0x00020000);
  const int voff = ((m0 + 4 * fk) * CP + c) * 4 | (c < CP ? 0 : 0x7fffffff);      // dead channel / row >= M: reads 0
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    if (reg / (16 / GQ_NB) != b) continue;           // (b is a compile-time constant at every call site)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int so = __builtin_amdgcn_readfirstlane((32 * i + (reg & 3) + 8 * (reg >> 2)) * CP * 4);
      sv.y[i][reg] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, voff, so, 0));
      sv.g[i][reg] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, voff, so, 0));
    }
  }
}

// fragment reads of the first two products: A = operand rows (both row tiles, both planes) at k0; B = the wave's NT column
// tiles of k-step u inside the stage
__device__ __forceinline__ void gq_read_a(const unsigned short* __restrict__ Ap, int plane_stride, int tile_stride,
                                          gb_bf8 (&a)[2][2]) {
  gb_read_a(Ap, plane_stride, tile_stride, a);
}
template <int NT>
__device__ __forceinline__ void gq_read_b(const unsigned short* __restrict__ Bp, gb_bf8 (&b)[NT][2]) {
#pragma unroll
  for (int j = 0; j < NT; ++j)
#pragma unroll
    for (int p = 0; p < 2; ++p)
      b[j][p] = __builtin_bit_cast(gb_bf8, *reinterpret_cast<const uint4*>(Bp + p * (GB_STAGE_E / 2) + j * 256));
}
// one ring stage of the first / second product: 32 / NT k = 2 / NT k-steps of 16, 12 MFMAs, 4 DMA pieces
template <int NT>
__device__ __forceinline__ void gq_stage(const unsigned short* Ap, int plane_stride, int tile_stride, const unsigned short* Bst,
                                         int boff, sg_f32x16 (&acc)[2][NT], GfRing& rg) {
  constexpr int NU = 2 / NT;                         // k-steps per stage
  int piece = 0;
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    gb_bf8 a[2][2], b[NT][2];
    gq_read_a(Ap + 16 * u, plane_stride, tile_stride, a);
    gq_read_b<NT>(Bst + boff + u * (2 * 4 * NT * 32 * 8), b);
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        __builtin_amdgcn_sched_barrier(0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][0], acc[i][j], 0, 0, 0);
        if (piece < GF_NI) rg.issue(piece);
        ++piece;
        __builtin_amdgcn_sched_barrier(0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][1], acc[i][j], 0, 0, 0);
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
      }
  }
}

// K loop of one product (phase).  PJ >= 0: the saved out / gate values of column tile PJ (tensors y / gt) are requested from
// inside the last GQ_NB stages, one batch right behind each stage's barrier (P2 >= 0: a second tile into sv2 likewise).
template <int NT, int PJ, int P2>
__device__ __forceinline__ void gq_kloop(const unsigned short* Ab, int LDK, GfRing& rg, int& rbuf, int nst, int lane, int wave,
                                         sg_f32x16 (&acc)[2][NT], GqSaved& sv, GqSaved& sv2, const float* __restrict__ y,
                                         const float* __restrict__ gt, int CP, int M, int m0) {
  constexpr int KS = 32 / NT;
  const int fi = lane & 31, fk = (lane >> 5) << 3;
  const int plane_stride = GB_BM * LDK, tile_stride = 32 * LDK;
  const unsigned short* Ap = Ab + fi * LDK + fk;
  // this lane's B fragment inside a stage: [plane][k eighth = 2 u + (lane >> 5)][wave][j][fi][8]
  const int boff = ((((lane >> 5) * 4 + wave) * NT) * 32 + fi) * 8;
  const unsigned short* ring = reinterpret_cast<const unsigned short*>(rg.ring);
  const int nhead = (PJ >= 0 && nst > GQ_NB) ? nst - GQ_NB : (PJ >= 0 ? 0 : nst);
  int s = 0;
  for (; s < nhead; ++s) {
    gf_wait_vm<(GB_STAGES - 2) * GF_NI>();
    __builtin_amdgcn_s_barrier();
    gq_stage<NT>(Ap + s * KS, plane_stride, tile_stride, ring + (size_t)rbuf * GB_STAGE_E, boff, acc, rg);
    rg.advance();
    rbuf = rbuf + 1 == GB_STAGES ? 0 : rbuf + 1;
  }
  if constexpr (PJ >= 0) {
    const int first = nst < GQ_NB ? GQ_NB - nst : 0;
#pragma unroll
    for (int b = 0; b < GQ_NB; ++b) {
      if (b >= first) {
        gf_wait_vm<(GB_STAGES - 2) * GF_NI>();
        __builtin_amdgcn_s_barrier();
      }
      gq_load_batch<NT, PJ>(sv, b, y, gt, CP, M, m0, lane, wave);
      if constexpr (P2 >= 0) gq_load_batch<NT, P2>(sv2, b, y, gt, CP, M, m0, lane, wave);
      if (b >= first) {
        gq_stage<NT>(Ap + s * KS, plane_stride, tile_stride, ring + (size_t)rbuf * GB_STAGE_E, boff, acc, rg);
        rg.advance();
        rbuf = rbuf + 1 == GB_STAGES ? 0 : rbuf + 1;
        ++s;
      }
    }
  }
}

// third product (-> dG, 3 W <= 64 columns): the four waves split the 2 x 2 output tiles of the [64 x 64] result; a ring stage
// holds 64 k x 64 columns = 4 k-steps of 16: 12 MFMAs per wave
__device__ __forceinline__ void gq_read_c(const unsigned short* __restrict__ Ap, const unsigned short* __restrict__ Bp,
                                          int plane_stride, gb_bf8 (&a)[2], gb_bf8 (&b)[2]) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    a[p] = __builtin_bit_cast(gb_bf8, *reinterpret_cast<const uint4*>(Ap + p * plane_stride));
    b[p] = __builtin_bit_cast(gb_bf8, *reinterpret_cast<const uint4*>(Bp + p * (GB_STAGE_E / 2)));
  }
}
__device__ __forceinline__ void gq_kloop_c(const unsigned short* Ab, int LDK, GfRing& rg, int& rbuf, int nst, int lane, int wave,
                                           sg_f32x16& acc) {
  const int fi = lane & 31, fk = (lane >> 5) << 3, mi = wave >> 1, nj = wave & 1;
  const int plane_stride = GB_BM * LDK;
  const unsigned short* Ap = Ab + (32 * mi + fi) * LDK + fk;
  const int boff = ((lane >> 5) * 64 + 32 * nj + fi) * 8;      // [plane][k eighth = 2 u + (lane >> 5)][col][8]
  const unsigned short* ring = reinterpret_cast<const unsigned short*>(rg.ring);
  for (int s = 0; s < nst; ++s) {
    gf_wait_vm<(GB_STAGES - 2) * GF_NI>();
    __builtin_amdgcn_s_barrier();
    const unsigned short* Bst = ring + (size_t)rbuf * GB_STAGE_E + boff;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      gb_bf8 a[2], b[2];
      gq_read_c(Ap + s * 64 + 16 * u, Bst + u * (2 * 64 * 8), plane_stride, a, b);
      __builtin_amdgcn_sched_barrier(0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], acc, 0, 0, 0);
      rg.issue(u);
      __builtin_amdgcn_sched_barrier(0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], acc, 0, 0, 0);
    }
    rg.advance();
    rbuf = rbuf + 1 == GB_STAGES ? 0 : rbuf + 1;
  }
}

// operand rows of the coming phase: this lane's channel = k pair (k0, k0 + 1) = (left, right), rows of both tiles; one 4-byte
// write per plane and element (through a __restrict__ pointer, see gf_write_operand)
__device__ __forceinline__ void gq_write_operand(unsigned short* __restrict__ a0, int plane_stride, int LDK, const float (&l)[2][16],
                                                 const float (&r)[2][16], int lane) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rl = 32 * i + g2_row_of(reg, lane);
      unsigned hi, lo;
      gb_split_pair(l[i][reg], r[i][reg], hi, lo);
      *reinterpret_cast<unsigned*>(a0 + rl * LDK) = hi;
      *reinterpret_cast<unsigned*>(a0 + plane_stride + rl * LDK) = lo;
    }
}

// GLU backward of column tile J of the accumulators: -> d(pre-activation) of the layer below in HBM (pair order, buffer
// stores: rows >= M and dead channels are dropped) and into the operand planes as k = 2 (wave 32 + lane) + t of the coming phase
template <int NT, int J>
__device__ __forceinline__ void gq_epilogue(const sg_f32x16 (&acc)[2][NT], unsigned short* Ab, int LDK, const GqSaved& sv,
                                            float* dpre, int CP, int M, int m0, int lane, int wave) {
  const int fi = lane & 31, fk = lane >> 5;
  const int c = wave * 32 * NT + 32 * J + fi;
  const int q = ((c >> 4) << 5) + (c & 15);
  float l[2][16], r[2][16];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const float d = acc[i][J][reg];
      l[i][reg] = d * sv.g[i][reg];
      r[i][reg] = d * sv.y[i][reg] * (1.f - sv.g[i][reg]);
    }
  gq_write_operand(Ab + 2 * (wave * 32 + fi), GB_BM * LDK, LDK, l, r, lane);
  const unsigned bytes = (unsigned)((size_t)M * 2 * CP * 4);
  const __amdgpu_buffer_rsrc_t rd = __builtin_amdgcn_make_buffer_rsrc(dpre, 0, bytes, 0x00020000);
  const int voff = ((m0 + 4 * fk) * 2 * CP + q) * 4 | (c < CP ? 0 : 0x7fffffff);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int so = __builtin_amdgcn_readfirstlane((32 * i + (reg & 3) + 8 * (reg >> 2)) * 2 * CP * 4);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, l[i][reg]), rd, voff, so, GB_STORE_AUX);
      __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(int, r[i][reg]), rd, voff, so + 64, GB_STORE_AUX);
    }
}

template <int NT>
static __global__ __launch_bounds__(256, 1) void sg_glu_fused_dgrad_bf16_kernel(const GqArgs g) {
  extern __shared__ __attribute__((aligned(16))) float gb_lds[];   // ONE array: the two operand planes, then the ring
  unsigned short* Ab = reinterpret_cast<unsigned short*>(gb_lds);
  const int L = blockIdx.x, xcd = L & 7;
  const int r = (xcd >> 2) & 1, rb = (L >> 3) * 4 + (xcd & 3);
  if (rb >= g.nrb) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = rb * GB_BM, M = g.M, CP = g.CP, LDK = g.LDK;
  constexpr int KS = 32 / NT;

  GfRing rg;
  rg.ring = gb_lds + (size_t)GB_BM * LDK;
  rg.wave = wave;
  rg.nstages = GB_STAGES;
  rg.src = reinterpret_cast<const float*>(g.wd[r]) + (size_t)wave * GF_NI * 256 + lane * 4;
  rg.next = 0; rg.last = g.ns[r] - 1; rg.wbuf = 0;
#pragma unroll
  for (int p = 0; p < GB_STAGES - 1; ++p) {
#pragma unroll
    for (int q = 0; q < GF_NI; ++q) rg.issue(q);
    rg.advance();
  }
  {  // operand of the first product: the block's d(pre-activation) rows of layer 2, split into the two planes; k beyond np2
     // (up to the stage boundary) and rows beyond M are zero.  A thread moves four consecutive k of one row.
    const int np2 = g.np2[r], kend = g.nstA[r] * KS, nq = kend >> 2;
    const float* src = g.dact2[r] + (size_t)m0 * np2;
    const int rows = M - m0 < GB_BM ? M - m0 : GB_BM;
    for (int idx = tid; idx < GB_BM * nq; idx += 256) {
      const int i = idx / nq, kq = idx - i * nq;
      const bool ok = i < rows && 4 * kq < np2;                    // (np2 is a multiple of 4)
      const float4 v = *reinterpret_cast<const float4*>(src + (ok ? (size_t)i * np2 + 4 * kq : 0));
      unsigned h01, l01, h23, l23;
      gb_split_pair(ok ? v.x : 0.f, ok ? v.y : 0.f, h01, l01);
      gb_split_pair(ok ? v.z : 0.f, ok ? v.w : 0.f, h23, l23);
      *reinterpret_cast<uint2*>(Ab + i * LDK + 4 * kq) = make_uint2(h01, h23);
      *reinterpret_cast<uint2*>(Ab + GB_BM * LDK + i * LDK + 4 * kq) = make_uint2(l01, l23);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int rbuf = 0;
  sg_f32x16 acc1[2][NT], acc0[2][NT];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc1[i][j][e] = 0.f; acc0[i][j][e] = 0.f; }
  GqSaved sva, svb;
  gq_kloop<NT, 0, -1>(Ab, LDK, rg, rbuf, g.nstA[r], lane, wave, acc1, sva, svb, g.out1[r], g.gate1[r], CP, M, m0);   // d(out of layer 1)
  __builtin_amdgcn_s_barrier();                                      // every wave is done reading the operand planes
  gq_epilogue<NT, 0>(acc1, Ab, LDK, sva, g.dact1[r], CP, M, m0, lane, wave);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (NT == 2) {
    gq_kloop<NT, 1, -1>(Ab, LDK, rg, rbuf, g.nstB[0], lane, wave, acc0, sva, svb, g.out1[r], g.gate1[r], CP, M, m0);  // phase 0
    __builtin_amdgcn_s_barrier();
    gq_epilogue<NT, 1>(acc1, Ab, LDK, sva, g.dact1[r], CP, M, m0, lane, wave);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gq_kloop<NT, 0, 1>(Ab, LDK, rg, rbuf, g.nstB[1], lane, wave, acc0, sva, svb, g.out0[r], g.gate0[r], CP, M, m0);
  } else {
    gq_kloop<NT, 0, -1>(Ab, LDK, rg, rbuf, g.nstB[0], lane, wave, acc0, sva, svb, g.out0[r], g.gate0[r], CP, M, m0);
  }
  // third product: d(pre-activation) of layer 0 (stored for the weight gradients, kept in LDS phase by phase) -> dG slab
  sg_f32x16 accg;
#pragma unroll
  for (int e = 0; e < 16; ++e) accg[e] = 0.f;
  __builtin_amdgcn_s_barrier();
  gq_epilogue<NT, 0>(acc0, Ab, LDK, sva, g.dact0[r], CP, M, m0, lane, wave);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  gq_kloop_c(Ab, LDK, rg, rbuf, g.nstC[0], lane, wave, accg);
  if constexpr (NT == 2) {
    __builtin_amdgcn_s_barrier();
    gq_epilogue<NT, 1>(acc0, Ab, LDK, svb, g.dact0[r], CP, M, m0, lane, wave);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gq_kloop_c(Ab, LDK, rg, rbuf, g.nstC[1], lane, wave, accg);
  }
  {
    const int kin = (wave & 1) * 32 + (lane & 31), mi = wave >> 1;
    float* pg = g.dG[r] + (size_t)m0 * g.KG + kin;
    if (kin < g.KG) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int rl = 32 * mi + g2_row_of(reg, lane);
        if (m0 + rl < M) pg[(size_t)rl * g.KG] = accg[reg];
      }
    }
  }
  gf_wait_vm<0>();
}
