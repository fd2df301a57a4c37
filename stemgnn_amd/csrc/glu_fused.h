// Fused forward of the three GLU layers of a StockBlock (reference models/base_model.py:52-54 with :12-13) for gfx950,
// round 4: ONE launch per block instead of three.
//
// The layers are row-local (out_l[m] depends on out_{l-1}[m] only), so a workgroup owns 64 series rows of ONE branch
// (Re / Im) and walks all three layers:
//   * the layer input of the row block stays in LDS, K-major (As[k][row], row stride 66 floats): the GFT output G for
//     layer 0, then every layer's `out` is written back into the same buffer by the epilogue (the K loop of a layer is
//     finished before its output exists, so the buffer is reused in place) -- no activation re-read from HBM / L2;
//   * a wave owns ALL 64 rows x 32 HP channels (HP = 1 or 2 groups of 32), left and right linear maps of a channel in the
//     same lane (no cross-lane exchange in the GLU epilogue): 2 x HP x 2 MFMA tiles of 32 x 32 = up to 128 accumulator
//     registers; the whole layer output lives in the accumulators of the four waves;
//   * the weights of the three layers are ONE contiguous stream of 16 KB stages (pre-packed by sg_pack_fused_kernel in
//     exactly the LDS image the fragment reads want), moved L2 -> LDS by `global_load_lds_dwordx4` into a 5-stage ring
//     that never drains: the first stages of layer l+1 land while layer l's epilogue runs; one counted `s_waitcnt vmcnt`
//     per stage and -- a stage being stored wave-major, every wave requesting exactly the slice it reads (GF_PRIVATE_RING)
//     -- no barrier inside a layer's K loop (the csrc/wgrad.h ring, here with the A operand resident);
//   * per k-step one 8-byte A fragment read + HP 8-byte B fragment reads feed 4 HP MFMAs (v_mfma_f32_32x32x2_f32, exact
//     fp32: every accumulator sums k = 0, 1, 2, .. in order, as the per-layer kernels do -- same bits);
//   * the epilogue adds the bias, forms out = u * sigmoid(v), stores `out` and `gate` for the backward pass (128
//     contiguous bytes per row and store instruction, fire and forget) and drops `out` into the activation buffer.
// Launch, first-tile latency and the store tail are paid once per block instead of three times, and layers 1 / 2 no
// longer read their 14 MB inputs back.  Applies when the padded channel count is <= 256 (W * multi <= 64: every BASELINE
// configuration except configs[4], whose K = 960 layers run the per-layer kernels at 0.8 of peak anyway).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "gemm2.h"
#include "layout.h"

constexpr int GF_NI = 4;             // DMA pieces (1 KB each) per wave and stage  (GF_BM, GF_LDA, GF_STAGE, GF_STAGES: layout.h)
#ifndef GF_PF
#define GF_PF 2                      // fragment prefetch distance in k-steps
#endif
#ifndef GF_ABL
#define GF_ABL 0                     // timing-probe ablation bits (tools/probe/glu_fused_probe): 1 no epilogue stores,
#endif                               // 2 no MFMA, 4 no DMA in the K loop, 8 no sigmoid.  Results wrong by design.
// Wave-private weight ring.  A wave owns all rows of the block times its own channel slice, so of a weight stage it reads
// only its own CW = NC / 4 columns.  With the stage stored wave-major ([wave][RS rows][CW columns]: a wave's slice is 4 KB =
// exactly its GF_NI pieces of 1 KB) every wave requests precisely the bytes it will read: its own counted `s_waitcnt vmcnt`
// orders its fragment reads behind its own DMA and no barrier is needed inside a K loop.  The first fragments of stage s + 1
// are then read under the last MFMAs of stage s (GF_XPF) -- the K loop of a layer is one uninterrupted MFMA stream.  The
// pack kernels emit the wave-major order (route "repack": the DMA source stays one contiguous run and the producer side of
// the ring does not change at all; nothing outside this file knows the element order inside a stage).
// -DGF_PRIVATE_RING=0 restores the shared ring (pieces dealt by position, one s_barrier per stage); -DGF_XPF=0 keeps the
// private ring but starts every stage with its own fragment reads (A/B: tools/build_variant.sh, STEMGNN_HIP_LIB).
#ifndef GF_PRIVATE_RING
#define GF_PRIVATE_RING 1
#endif
#ifndef GF_XPF
#define GF_XPF 1
#endif
#define GF_CARRY (GF_PRIVATE_RING && GF_XPF)
// prologue copies (G -> LDS in the forward, d(pre-activation) of layer 2 -> LDS in the chain): loads in flight per thread
// before the first LDS write; 0 = the one-load-one-write loops
#ifndef GF_G_BATCH
#define GF_G_BATCH 8
#endif
constexpr int GF_WSLICE = 1024;      // floats of a wave's slice of a stage (GF_STAGE / 4 = GF_NI pieces of 256)

__device__ __forceinline__ float gf_sigmoid(float v) { return __frcp_rn(1.f + __expf(-v)); }
// saved out / gate and d(pre-activation) stores: 82 / 148 MB per launch that nobody reads before the backward pass -- as
// non-temporal (streaming) stores they stop evicting what the step is about to use (round 5, measured on the bf16 kernels:
// 1.1009 -> 1.0853 ms per step; -DGF_NT_STORES=0 restores the default policy)
#ifndef GF_NT_STORES
#define GF_NT_STORES 1
#endif
#if GF_NT_STORES
#define GF_ST(p, v) __builtin_nontemporal_store((v), (p))
#else
#define GF_ST(p, v) (*(p) = (v))
#endif

// ---- weight stream in LDS-image order ---------------------------------------------------------------------------------
// stage s of layer l, element (kk, p): kk < rs weight rows, p < 256 hp columns; column p = wave * 64 hp + h * 64 + 2 fi + t
// holds linear_left (t = 0) / linear_right (t = 1) of channel c = wave * 32 hp + h * 32 + fi, input k = s * rs + kk.
// Source: the K-major "pair" panel Wp[k][q], q = (c / 16) * 32 + c % 16 + 16 t (layout.h).  Padding rows / channels = 0.
// Position inside the stage: private ring  wave * 1024 + kk * 64 hp + (p - wave * 64 hp)   (wave-major, a wave's columns
// contiguous per row);  shared ring  kk * 256 hp + p.
struct GfPackArgs {
  const float* wp[2][3];
  float* wf[2];
  int K[3], np[2][3], cp[2][3];
  GfGeom g;
};
static __global__ __launch_bounds__(256) void sg_pack_fused_kernel(const GfPackArgs a) {
  const int r = blockIdx.y;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.g.ns * GF_STAGE) return;
  int s = (int)(e / GF_STAGE), l = 0;
  while (l < 2 && s >= a.g.nst[l]) { s -= a.g.nst[l]; ++l; }
  const int hp = 16 / a.g.rs[l], nc = 256 * hp;
  const int w = (int)(e % GF_STAGE);
#if GF_PRIVATE_RING
  // wave-major stage image: [wave][rs rows][64 hp columns]; the column inside the wave's slice as before
  const int wave = w / GF_WSLICE, kk = (w % GF_WSLICE) / (64 * hp), rem = w % (64 * hp);
  (void)nc;
#else
  const int kk = w / nc, p = w % nc;
  const int wave = p / (64 * hp), rem = p % (64 * hp);
#endif
  const int h = rem >> 6, fi = (rem & 63) >> 1, t = rem & 1;
  const int c = wave * 32 * hp + h * 32 + fi, k = s * a.g.rs[l] + kk;
  float v = 0.f;
  if (k < a.K[l] && c < a.cp[r][l]) v = a.wp[r][l][(size_t)k * a.np[r][l] + ((c >> 4) << 5) + (c & 15) + 16 * t];
  a.wf[r][e] = v;
}

// ---- kernel -----------------------------------------------------------------------------------------------------------
struct GfArgs {
  const float* G;               // [M][KG]
  const float* wf[2];           // fused-order weight stream per branch
  const float* bias[2][3];      // packed pair-order bias (left at q, right at q + 16)
  float* out[2][3];
  float* gate[2][3];
  int cp[2][3];                 // padded channel counts = row strides of out / gate
  int nst[3];
  int KG, KP0, KA, M, nrb, ns;
};

template <int N>
__device__ __forceinline__ void gf_wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// the ring's producer side: this lane's source pointer of the NEXT stage to request and the buffer it goes to
struct GfRing {
  const float* src;
  float* ring;
  int next, last, wbuf, wave, nstages;
  __device__ __forceinline__ void issue(int q) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + q * 256),
                                     (__attribute__((address_space(3))) void*)(ring + wbuf * GF_STAGE + (wave * GF_NI + q) * 256),
                                     16, 0, 0);
  }
  // stages past the end re-request the last one (never read): the ring stays full, the counted wait stays one constant
  __device__ __forceinline__ void advance() {
    if (next < last) src += GF_STAGE;
    ++next;
    wbuf = wbuf + 1 == nstages ? 0 : wbuf + 1;
  }
};

// Row tiles of a workgroup (MT = 2: 64 rows, MT = 3: 96 rows -- the latter when 64-row blocks would need a second, mostly
// empty round of workgroups, e.g. M = 11456 at PEMS03: 358 blocks on 256 CUs -> 240 blocks of 96).  Tiles 0 and 1 are
// interleaved in block rows 0..63 (tile i, tile row r = block row 2 r + i: one 8-byte LDS read feeds both), tile 2 is block
// rows 64..95.  LDS row stride of the K-major operand buffer: 32 MT + 2 floats (conflict-free 8-byte epilogue writes).
template <int MT>
struct GfTile {
  static constexpr int BM = 32 * MT, LDA = 32 * MT + 2;
  static constexpr int STAGES = MT == 3 ? 4 : 5;        // ring depth the LDS leaves room for (MT = 3: 94 KB of operand)
  static __device__ __forceinline__ int row(int i, int reg, int lane) {
    return i < 2 ? 2 * g2_row_of(reg, lane) + i : 64 + g2_row_of(reg, lane);
  }
};
// One ring stage of MFMA work (16 / HP weight rows = 8 / HP k-steps) with the next ring stage's DMA pieces issued from
// inside it.  The fragment reads go through __restrict__ pointers: that gives them alias-scope metadata, without which
// hipcc's waitcnt pass assumes every LDS read may alias the LDS-DMA in flight and drains the ring (vmcnt(0)) per k-step.
// Aq points at (row k0 + fk, column 2 fi) of the operand buffer; A2 at (row k0 + fk, column 64 + fi) (MT = 3 only).
// Row stride of a weight stage as a wave's fragment reads see it: the wave's own CW columns (private ring) or all NC.
#if GF_PRIVATE_RING
#define GF_BSTRIDE(NC_) ((NC_) / 4)
#else
#define GF_BSTRIDE(NC_) (NC_)
#endif
// The first fragments of a stage (k-steps 0 .. PF - 1), carried from the stage before it (GF_XPF)
template <int HP>
struct GfFrag {
  float2 a[GF_PF], b[GF_PF][HP];
  float c[GF_PF];
};
// NEXT (GF_XPF): this stage is not the K loop's last -- behind the request of its last DMA piece it waits for this wave's
// pieces of the next stage (same counted constant: STAGES - 2 newer stages may still be in flight) and reads that stage's
// first fragments (operand rows + RS, weights at Bn) into pf, under the MFMAs that are left.  Those reads touch the buffer of
// stage s + 1 only; the pieces requested from inside this stage go to the buffer of stage s - 1, whose fragment reads -- this
// wave's own, nobody else reads its slice -- had all returned before its last MFMA issued (per-wave write-after-read).
// FIRST: the K loop's first stage reads its own first fragments (nothing was carried to it).  All fragment reads, the
// carried ones too, are on this function's __restrict__ parameters and land in locals first: they must keep the alias
// scopes that the DMA requests issued from here are marked not to alias, or hipcc puts a `vmcnt(0)` ahead of them
// (compiler facts (i) and (iii) of DESIGN 4).
template <int MT, int HP, bool FIRST, bool NEXT>
__device__ __forceinline__ void gf_stage(const float* __restrict__ Aq, const float* __restrict__ A2,
                                         const float* __restrict__ Bs, const float* __restrict__ Bn,
                                         sg_f32x16 (&acc)[MT][HP][2], GfRing& rg, GfFrag<HP>& pf) {
  constexpr int NC = 256 * HP, RS = 16 / HP, STEPS = RS / 2, LDA = GfTile<MT>::LDA, BST = GF_BSTRIDE(NC);
  constexpr int EVERY = STEPS / GF_NI;                 // one DMA piece every EVERY k-steps (1 or 2)
  float2 fa[STEPS], fb[STEPS][HP];
  float fc[STEPS];
  auto rd = [&](int st) {
    fa[st] = *reinterpret_cast<const float2*>(Aq + 2 * st * LDA);
    if constexpr (MT == 3) fc[st] = A2[2 * st * LDA];
#pragma unroll
    for (int h = 0; h < HP; ++h) fb[st][h] = *reinterpret_cast<const float2*>(Bs + 2 * st * BST + h * 64);
  };
#pragma unroll
  for (int st = 0; st < GF_PF && st < STEPS; ++st) {
    if constexpr (GF_CARRY && !FIRST) {
      fa[st] = pf.a[st]; fc[st] = MT == 3 ? pf.c[st] : 0.f;
#pragma unroll
      for (int h = 0; h < HP; ++h) fb[st][h] = pf.b[st][h];
    } else {
      rd(st);
    }
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    float a[3];
    a[0] = fa[st].x; a[1] = fa[st].y; a[2] = MT == 3 ? fc[st] : 0.f;
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) acc[0][0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], fb[st][0].x, acc[0][0][0], 0, 0, 0);
    if (st + GF_PF < STEPS) rd(st + GF_PF);
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) acc[0][0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], fb[st][0].y, acc[0][0][1], 0, 0, 0);
    if (!(GF_ABL & 4) && st % EVERY == 0 && st / EVERY < GF_NI) rg.issue(st / EVERY);
#if GF_CARRY
    if constexpr (NEXT) {
      if (st == (GF_NI - 1) * EVERY) {                 // the stage's last piece is out
        gf_wait_vm<(GfTile<MT>::STAGES - 2) * GF_NI>();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int pn = 0; pn < GF_PF && pn < STEPS; ++pn) {
          // (through locals: a float2 copied straight into pf is a memcpy at the time the alias scopes are handed out,
          // and the load it becomes later has none)
          const float2 va = *reinterpret_cast<const float2*>(Aq + (RS + 2 * pn) * LDA);
          pf.a[pn].x = va.x; pf.a[pn].y = va.y;
          if constexpr (MT == 3) pf.c[pn] = A2[(RS + 2 * pn) * LDA];
#pragma unroll
          for (int h = 0; h < HP; ++h) {
            const float2 vb = *reinterpret_cast<const float2*>(Bn + 2 * pn * BST + h * 64);
            pf.b[pn][h].x = vb.x; pf.b[pn][h].y = vb.y;
          }
        }
      }
    }
#endif
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) {
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int h = 0; h < HP; ++h) {
          if (i == 0 && h == 0) continue;
          acc[i][h][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], fb[st][h].x, acc[i][h][0], 0, 0, 0);
          acc[i][h][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], fb[st][h].y, acc[i][h][1], 0, 0, 0);
        }
    }
  }
}

// INF: the inference forward (stemgnn_spectral_glu_fwd_infer) -- the same arithmetic with only the last layer's `out` stored
// (no gate at all; layers 0 / 1 live in LDS only)
template <int MT, int HP, bool LAST, bool INF = false>
__device__ __forceinline__ void gf_layer(float* As, GfRing& rg, int& rbuf, int nst, int lane, int wave,
                                         const float (&bl)[2], const float (&br)[2], float* __restrict__ outp,
                                         float* __restrict__ gatep, int cp, int M, int m0, int KA) {
  using T = GfTile<MT>;
  constexpr int NC = 256 * HP, RS = 16 / HP, LDA = T::LDA;
  const int fi = lane & 31, fk = lane >> 5;
  sg_f32x16 acc[MT][HP][2];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int h = 0; h < HP; ++h)
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][h][t][e] = 0.f;
  const float* Ap = As + fk * LDA + 2 * fi;
  const float* Ap2 = As + fk * LDA + 64 + fi;
  GfFrag<HP> pf;
#if GF_PRIVATE_RING
  // Private ring: NO barrier inside the K loop.  What orders the LDS traffic instead:
  //   * weights, read-after-write: a wave reads only the slice its own pieces filled, behind its own counted vmcnt wait
  //     (in-order retirement: with STAGES - 2 stages' pieces allowed in flight the oldest requested stage has landed);
  //   * weights, write-after-read, per wave: the pieces requested from inside stage s go to the buffer of stage s - 1; this
  //     wave's fragment reads of that buffer have returned (its MFMAs consumed them), and no other wave reads the slice;
  //   * activation buffer: ONE barrier here, after the prologue copy's / the previous layer's epilogue LDS writes (each
  //     wave has waited lgkmcnt(0) behind its own) and before the K loop's first read of it.  It does not change during
  //     the K loop; the barrier ahead of the epilogue (below) keeps the epilogue from overwriting it under a reader.
  const int boff = wave * GF_WSLICE + fk * (NC / 4) + 2 * fi;
  const float* Bw = rg.ring + boff;
  gf_wait_vm<(T::STAGES - 2) * GF_NI>();               // my pieces of the layer's first stage have landed
  __builtin_amdgcn_s_barrier();                        // the layer input in LDS is complete
  // every stage but the last waits for and reads the start of the next one from inside (gf_stage<.., NEXT>); the first and
  // the last stage are peeled off the loop (straight-line code: no join at which hipcc would wait for the ring)
  auto stage = [&](int s, auto first, auto next) __attribute__((always_inline)) {
    const int nbuf = rbuf + 1 == T::STAGES ? 0 : rbuf + 1;
    gf_stage<MT, HP, decltype(first)::value, decltype(next)::value>(Ap + (size_t)s * RS * LDA, Ap2 + (size_t)s * RS * LDA,
                                            Bw + rbuf * GF_STAGE, Bw + nbuf * GF_STAGE, acc, rg, pf);
    rg.advance();
    rbuf = nbuf;
  };
#if GF_XPF
  constexpr std::true_type yes{};
  constexpr std::false_type no{};
  if (nst == 1) {
    stage(0, yes, no);
  } else {
    stage(0, yes, yes);
    for (int s = 1; s + 1 < nst; ++s) stage(s, no, yes);
    stage(nst - 1, no, no);
  }
#else
  for (int s = 0; s < nst; ++s) {
    if (s) gf_wait_vm<(T::STAGES - 2) * GF_NI>();      // my pieces of this stage have landed
    stage(s, std::true_type{}, std::false_type{});
  }
#endif
#else
  const int boff = fk * NC + wave * (64 * HP) + 2 * fi;
  for (int s = 0; s < nst; ++s) {
    gf_wait_vm<(T::STAGES - 2) * GF_NI>();             // my pieces of this stage have landed
    __builtin_amdgcn_s_barrier();                      // everybody's have; the buffer read last stage is free
    const float* Bs = rg.ring + rbuf * GF_STAGE + boff;
    gf_stage<MT, HP, true, false>(Ap + (size_t)s * RS * LDA, Ap2 + (size_t)s * RS * LDA, Bs, Bs, acc, rg, pf);
    rg.advance();
    rbuf = rbuf + 1 == T::STAGES ? 0 : rbuf + 1;
  }
#endif
  // ---- epilogue: bias, GLU gating, saved tensors, next layer's input ----------------------------------------------------
  if constexpr (!LAST) __builtin_amdgcn_s_barrier();     // every wave is done reading the activation buffer
  const bool full = m0 + T::BM <= M;                     // wave-uniform: only the last row block of a launch is ragged
#pragma unroll
  for (int h = 0; h < HP; ++h) {
    const int c = wave * 32 * HP + h * 32 + fi;
    const bool live = c < cp;
    float o[16][MT], gs[16][MT];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
#pragma unroll
      for (int i = 0; i < MT; ++i) {
        const float u = acc[i][h][0][reg] + bl[h], v = acc[i][h][1][reg] + br[h];
        gs[reg][i] = (GF_ABL & 8) ? v : gf_sigmoid(v);
        o[reg][i] = u * gs[reg][i];
      }
      if constexpr (!LAST) {
        if (c < KA) {
          *reinterpret_cast<float2*>(As + c * LDA + 2 * g2_row_of(reg, lane)) = make_float2(o[reg][0], o[reg][1]);
          if constexpr (MT == 3) As[c * LDA + 64 + g2_row_of(reg, lane)] = o[reg][2];
        }
      }
    }
    // saved tensors: ONE lane predicate around the whole store loop (a per-store `row < M` test costs an exec-mask branch
    // per store pair); the ragged last block takes the predicated form
    float* po = outp + (size_t)m0 * cp + c;
    float* pg = gatep + (size_t)m0 * cp + c;
    if (!(GF_ABL & 1) && (!INF || LAST) && live) {
      if (full) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            const size_t off = (size_t)T::row(i, reg, lane) * cp;
            GF_ST(&po[off], o[reg][i]);
            if constexpr (!INF) GF_ST(&pg[off], gs[reg][i]);
          }
      } else {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
#pragma unroll
          for (int i = 0; i < MT; ++i) {
            const int rl = T::row(i, reg, lane);
            if (m0 + rl < M) {
              GF_ST(&po[(size_t)rl * cp], o[reg][i]);
              if constexpr (!INF) GF_ST(&pg[(size_t)rl * cp], gs[reg][i]);
            }
          }
      }
    }
  }
  if constexpr (!LAST) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // published by the barrier at the next K loop's entry
  if (GF_ABL & 1) {
    if (acc[0][0][0][0] + acc[MT - 1][HP - 1][1][7] == 1.2345e-30f) As[0] = 1.f;   // keep the accumulators alive
  }
}

template <int MT, int HP01, int HP2, bool INF = false>
static __global__ __launch_bounds__(256, 1) void sg_glu_fused_fwd_kernel(const GfArgs g) {
  using T = GfTile<MT>;
  extern __shared__ __attribute__((aligned(16))) float gf_lds[];   // ONE array: As[KA][LDA] then the ring
  float* As = gf_lds;
  const int L = blockIdx.x, xcd = L & 7;
  const int r = (xcd >> 2) & 1, rb = (L >> 3) * 4 + (xcd & 3);      // XCDs 0-3 stream branch 0's weights, 4-7 branch 1's
  if (rb >= g.nrb) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int fi = lane & 31;
  const int m0 = rb * T::BM, M = g.M;

  GfRing rg;
  rg.ring = gf_lds + (size_t)g.KA * T::LDA;
  rg.wave = wave;
  rg.nstages = T::STAGES;
  rg.src = g.wf[r] + (size_t)wave * GF_NI * 256 + lane * 4;
  rg.next = 0; rg.last = g.ns - 1; rg.wbuf = 0;
#pragma unroll
  for (int p = 0; p < T::STAGES - 1; ++p) {
#pragma unroll
    for (int q = 0; q < GF_NI; ++q) rg.issue(q);
    rg.advance();
  }
  // biases of this lane's channels (layer, group): loaded once -- an ordinary load inside the ring would drain it
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
  {  // layer-0 input: the G rows of this block, K-major, rows KG .. KP0-1 zero (they meet zero weight rows).  Block row i of
     // the buffer is series row m0 + i for tiles 0 / 1 interleaved (i < 64) and tile 2 (i >= 64) alike: the MFMA row <-> block
     // row mapping lives in the fragment reads and the epilogue only
    const int KG = g.KG;
    const float* Gp = g.G + (size_t)m0 * KG;
    const int nlive = (M - m0 < T::BM ? M - m0 : T::BM) * KG;
#if GF_G_BATCH
    // a thread's elements GF_G_BATCH at a time: all of a batch's loads requested before the first LDS write waits for one
    // (the one-load-one-write loop paid an L2 round trip per iteration, 9 of them at 64 rows x 36 columns)
    for (int base = tid; base < T::BM * KG; base += 256 * GF_G_BATCH) {
      float v[GF_G_BATCH];
#pragma unroll
      for (int j = 0; j < GF_G_BATCH; ++j) {
        const int idx = base + 256 * j;
        v[j] = Gp[idx < nlive ? idx : 0];
      }
#pragma unroll
      for (int j = 0; j < GF_G_BATCH; ++j) {
        const int idx = base + 256 * j;
        const int i = idx / KG, k = idx - i * KG;
        if (idx < T::BM * KG) As[k * T::LDA + i] = idx < nlive ? v[j] : 0.f;
      }
    }
#else
    for (int idx = tid; idx < T::BM * KG; idx += 256) {
      const int i = idx / KG, k = idx - i * KG;
      const float v = Gp[idx < nlive ? idx : 0];
      As[k * T::LDA + i] = idx < nlive ? v : 0.f;
    }
#endif
    for (int idx = tid; idx < (g.KP0 - KG) * T::BM; idx += 256) As[(KG + idx / T::BM) * T::LDA + (idx % T::BM)] = 0.f;
  }
  // materialise the biases HERE (the copy loop above has drained the loads anyway): left to the compiler their selects
  // sink to the first epilogue, where the wait for these ordinary loads would drain the ring
#pragma unroll
  for (int l = 0; l < 3; ++l)
#pragma unroll
    for (int h = 0; h < 2; ++h) asm volatile("" : "+v"(bl[l][h]), "+v"(br[l][h]));
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");       // (the barrier at the K loop's entry publishes the buffer)
  int rbuf = 0;
  gf_layer<MT, HP01, false, INF>(As, rg, rbuf, g.nst[0], lane, wave, bl[0], br[0], g.out[r][0], g.gate[r][0], g.cp[r][0], M, m0, g.KA);
  gf_layer<MT, HP01, false, INF>(As, rg, rbuf, g.nst[1], lane, wave, bl[1], br[1], g.out[r][1], g.gate[r][1], g.cp[r][1], M, m0, g.KA);
  gf_layer<MT, HP2, true, INF>(As, rg, rbuf, g.nst[2], lane, wave, bl[2], br[2], g.out[r][2], g.gate[r][2], g.cp[r][2], M, m0, g.KA);
  gf_wait_vm<0>();                                         // the run-ahead DMA pieces must not outlive the workgroup's LDS
}

// =======================================================================================================================
// Fused data-gradient chain of the GLU stack (autograd of models/base_model.py:52-54 with :12-13 through
// models/handler.py:164), round 4: d(pre-activation) of layer 2 (from the heads' backward) -> layer 1 -> layer 0 in ONE
// launch per block instead of three.  Mirror of the forward kernel:
//   * a workgroup owns 64 series rows of one branch; the operand of the running product is resident in LDS, K-major: the
//     d(pre-activation) rows of layer 2 are copied in from HBM, those of layer 1 are written there by the epilogue that
//     forms them (and stored to HBM once, for the weight-gradient kernel) -- they are never read back;
//   * a wave owns 32 NT channels of the layer whose d(out) is being formed, for all 64 rows: 2 x NT accumulator tiles; the
//     second product accumulates into a second set while the first set is still being turned into its operand;
//   * that operand (2 CP = 480 rows at PEMS07) does not fit the LDS beside the ring, so the reduction runs in NT phases of
//     256 rows: phase p = the left / right values of every wave's p-th channel group.  The reduction order of a product is
//     free -- the weight stream (sg_pack_dgrad_kernel) is laid out in exactly the order the phases produce the rows;
//   * GLU backward in the epilogue: d = d(out)[row][c]; left = d * gate; right = d * out * (1 - gate), with
//     the saved out / gate of the layer below loaded per lane (all loads of a tile in flight before the first use).
//   * the layer-0 product (K = 2 CP -> the 3 W columns of dG) runs the same way behind it: its operand, the
//     d(pre-activation) of layer 0, is stored once for the weight gradients and consumed from LDS; the four waves split the
//     2 x 2 output tiles of the [64 x 64] result (one MFMA per k-step -- 7 us of a 60 us workgroup instead of a launch).
// fp32 MFMA throughout; the first product sums its reduction in the per-layer kernels' order, the others in phase order
// (fp32 re-association: parity bar, not bitwise).
struct GdPackArgs {
  const float* wp[2][3];        // pair panels [K_in][NP] of layers 1, 2 (index 0 unused)
  float* wd[2];
  int np[2][3];
  int CP, KG;
  GdGeom g;
};
static __global__ __launch_bounds__(256) void sg_pack_dgrad_kernel(const GdPackArgs a) {
  const int r = blockIdx.y;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)a.g.ns[r] * GF_STAGE) return;
  int s = (int)(e / GF_STAGE);
  const int nt = a.g.nt, rs = a.g.rs, nc = 128 * nt;
  const int wi = (int)(e % GF_STAGE);
  const int sAB = a.g.nstA[r] + a.g.nstB[0] + a.g.nstB[1];
  if (s >= sAB) {                                    // third product: layer 0, 64 rows x 64 columns per stage
    s -= sAB;
    int ph = 0;
    if (s >= a.g.nstC[0]) { s -= a.g.nstC[0]; ph = 1; }
    const int kk = wi >> 6, kin = wi & 63;           // column = input index of layer 0 (3 W of them)
    const int k2 = s * 64 + kk;
    const int t = k2 & 1, wf = k2 >> 1, w2 = wf >> 5, f2 = wf & 31;
    const int c2 = w2 * 32 * nt + 32 * ph + f2;      // layer-0 channel whose left / right value the row holds
    float v = 0.f;
    if (w2 < 4 && c2 < a.CP && kin < a.KG) v = a.wp[r][0][(size_t)kin * a.np[r][0] + ((c2 >> 4) << 5) + (c2 & 15) + 16 * t];
    a.wd[r][e] = v;
    return;
  }
  // first / second product: a wave's 32 nt columns of a weight row are  wave * 32 nt + (nt == 2 ? 2 fi + j : fi).
  // Position inside the stage: private ring  wave * 1024 + kk * 32 nt + column in the slice  (wave-major, as the forward's
  // stream);  shared ring  kk * 128 nt + column.  The third product's stages (above) are shared by wave pairs and keep
  // their order in both forms.
#if GF_PRIVATE_RING
  const int kk = (wi % GF_WSLICE) / (32 * nt), p = (wi / GF_WSLICE) * (32 * nt) + wi % (32 * nt);
  (void)nc;
#else
  const int kk = wi / nc, p = wi % nc;
#endif
  int wave, fi, j;
  if (nt == 2) { wave = p >> 6; fi = (p & 63) >> 1; j = p & 1; }
  else { wave = p >> 5; fi = p & 31; j = 0; }
  const int c = wave * 32 * nt + 32 * j + fi;        // output column of the product = input channel of the layer
  float v = 0.f;
  if (s < a.g.nstA[r]) {                             // first product: layer 2, reduction row = natural pair column
    const int q = s * rs + kk;
    if (q < a.np[r][2] && c < a.CP) v = a.wp[r][2][(size_t)c * a.np[r][2] + q];
  } else {                                           // second product: layer 1, reduction rows in phase order
    s -= a.g.nstA[r];
    int ph = 0;
    if (s >= a.g.nstB[0]) { s -= a.g.nstB[0]; ph = 1; }
    const int k2 = s * rs + kk;                      // row of the phase: 2 (wave' 32 + lane') + t
    const int t = k2 & 1, wf = k2 >> 1, w2 = wf >> 5, f2 = wf & 31;
    const int c2 = w2 * 32 * nt + 32 * ph + f2;      // layer-1 channel whose left (t = 0) / right (t = 1) value the row holds
    if (w2 < 4 && c2 < a.CP && c < a.CP) v = a.wp[r][1][(size_t)c * a.np[r][1] + ((c2 >> 4) << 5) + (c2 & 15) + 16 * t];
  }
  a.wd[r][e] = v;
}

struct GdArgs {
  const float* dact2[2];        // [M][np2[r]]   d(pre-activation) of layer 2, pair order
  const float* wd[2];           // weight stream (sg_pack_dgrad_kernel)
  const float* out1[2];         // saved out / gate of layers 1 and 0, [M][CP]
  const float* gate1[2];
  const float* out0[2];
  const float* gate0[2];
  float* dact1[2];              // [M][2 CP]  d(pre-activation) of layers 1 and 0, pair order
  float* dact0[2];
  float* dG[2];                 // [M][KG]    layer-0 data gradient, one slab per branch (summed by the GFT backward)
  int np2[2], nstA[2], ns[2];
  int nstB[2], nstC[2];
  int CP, KG, M, nrb, KA;
};

// row-tile geometry of the data-gradient kernel: as GfTile, but the 96-row form leaves room for 3 ring stages only (its
// operand buffer is 256 x 98 floats = 100 KB)
template <int MT>
struct GdTile {
  static constexpr int BM = 32 * MT, LDA = 32 * MT + 2;
  static constexpr int STAGES = MT == 3 ? 3 : 5;
};

// first fragments of a stage of the first / second product, carried from the stage before it (GF_XPF; as GfFrag)
struct GdFrag {
  float2 a[GF_PF];
  float c[GF_PF], b[GF_PF][2];
};
template <int MT, int NT>
__device__ __forceinline__ void gd_frag_load(const float* __restrict__ Aq, const float* __restrict__ A2,
                                             const float* __restrict__ Bs, GdFrag& pf) {
  constexpr int RS = 32 / NT, STEPS = RS / 2, LDA = GdTile<MT>::LDA, BST = GF_BSTRIDE(128 * NT);
#pragma unroll
  for (int st = 0; st < GF_PF && st < STEPS; ++st) {
    const float2 va = *reinterpret_cast<const float2*>(Aq + 2 * st * LDA);   // (through locals: see gf_stage)
    pf.a[st].x = va.x; pf.a[st].y = va.y;
    if constexpr (MT == 3) pf.c[st] = A2[2 * st * LDA];
    if constexpr (NT == 2) {
      const float2 b = *reinterpret_cast<const float2*>(Bs + 2 * st * BST);
      pf.b[st][0] = b.x; pf.b[st][1] = b.y;
    } else {
      pf.b[st][0] = Bs[2 * st * BST]; pf.b[st][1] = 0.f;
    }
  }
}
// NEXT: as in gf_stage -- behind the stage's last DMA piece, wait for this wave's pieces of the next stage and read its
// first fragments (operand rows + RS, weights at Bn) into pf under the MFMAs that are left.  The saved out / gate loads of
// the loop's tail (gd_load_batch) are ordinary loads on the same counter: they only make the counted wait cover more.
template <int MT, int NT, bool NEXT>
__device__ __forceinline__ void gd_stage(const float* __restrict__ Aq, const float* __restrict__ A2,
                                         const float* __restrict__ Bs, const float* __restrict__ Bn,
                                         sg_f32x16 (&acc)[MT][NT], GfRing& rg, GdFrag& pf) {
  constexpr int NC = 128 * NT, RS = 32 / NT, STEPS = RS / 2, LDA = GdTile<MT>::LDA, BST = GF_BSTRIDE(NC);
  constexpr int EVERY = STEPS / GF_NI;                 // one DMA piece every EVERY k-steps (2 or 4)
  float2 fa[STEPS];
  float fc[STEPS];
  float fb[STEPS][2];
  auto rd = [&](int st) {
    fa[st] = *reinterpret_cast<const float2*>(Aq + 2 * st * LDA);
    if constexpr (MT == 3) fc[st] = A2[2 * st * LDA];
    if constexpr (NT == 2) {
      const float2 b = *reinterpret_cast<const float2*>(Bs + 2 * st * BST);
      fb[st][0] = b.x; fb[st][1] = b.y;
    } else {
      fb[st][0] = Bs[2 * st * BST]; fb[st][1] = 0.f;
    }
  };
#pragma unroll
  for (int st = 0; st < GF_PF && st < STEPS; ++st) {
#if GF_CARRY
    fa[st] = pf.a[st]; fc[st] = MT == 3 ? pf.c[st] : 0.f;
    fb[st][0] = pf.b[st][0]; fb[st][1] = pf.b[st][1];
#else
    rd(st);
#endif
  }
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    float a[3];
    a[0] = fa[st].x; a[1] = fa[st].y; a[2] = MT == 3 ? fc[st] : 0.f;
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], fb[st][0], acc[0][0], 0, 0, 0);
    if (st + GF_PF < STEPS) rd(st + GF_PF);
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], fb[st][0], acc[1][0], 0, 0, 0);
    if (!(GF_ABL & 4) && st % EVERY == 0 && st / EVERY < GF_NI) rg.issue(st / EVERY);
#if GF_CARRY
    if constexpr (NEXT) {
      if (st == (GF_NI - 1) * EVERY) {                 // the stage's last piece is out
        gf_wait_vm<(GdTile<MT>::STAGES - 2) * GF_NI>();
        __builtin_amdgcn_sched_barrier(0);
        gd_frag_load<MT, NT>(Aq + RS * LDA, A2 + RS * LDA, Bn, pf);
      }
    }
#endif
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) {
      if constexpr (MT == 3) acc[2][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], fb[st][0], acc[2][0], 0, 0, 0);
      if constexpr (NT == 2) {
#pragma unroll
        for (int i = 0; i < MT; ++i) acc[i][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], fb[st][1], acc[i][1], 0, 0, 0);
      }
    }
  }
}

// third product (-> dG, 3 W <= 64 columns): the four waves split the 2 x 2 output tiles of block rows 0..63, one MFMA per
// k-step; with 96-row blocks waves 0 / 1 also take the two tiles of rows 64..95.  A ring stage holds 64 weight rows x 64
// columns = 32 k-steps
template <int MT>
__device__ __forceinline__ void gd_stage_c(const float* __restrict__ Aq, const float* __restrict__ A2,
                                           const float* __restrict__ Bs, sg_f32x16& acc, sg_f32x16& acc2, bool extra,
                                           GfRing& rg) {
  constexpr int STEPS = 32, EVERY = STEPS / GF_NI, PF = 4, LDA = GdTile<MT>::LDA;
  float fa[STEPS], fb[STEPS], fc[STEPS];
  auto rd = [&](int st) {
    fa[st] = Aq[2 * st * LDA];
    fb[st] = Bs[2 * st * 64];
    if constexpr (MT == 3) fc[st] = A2[2 * st * LDA];
  };
#pragma unroll
  for (int st = 0; st < PF; ++st) rd(st);
#pragma unroll
  for (int st = 0; st < STEPS; ++st) {
    __builtin_amdgcn_sched_barrier(0);
    if (!(GF_ABL & 2)) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[st], fb[st], acc, 0, 0, 0);
    if constexpr (MT == 3) {
      if (extra && !(GF_ABL & 2)) acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(fc[st], fb[st], acc2, 0, 0, 0);   // wave-uniform
    }
    if (st + PF < STEPS) rd(st + PF);
    if (!(GF_ABL & 4) && st % EVERY == 0 && st / EVERY < GF_NI) rg.issue(st / EVERY);
  }
}
template <int MT>
__device__ __forceinline__ void gd_kloop_c(const float* As, GfRing& rg, int& rbuf, int nst, int lane, int wave, sg_f32x16& acc,
                                           sg_f32x16& acc2) {
  using T = GdTile<MT>;
  const int fi = lane & 31, fk = lane >> 5, mi = wave >> 1, nj = wave & 1;
  const float* Ap = As + fk * T::LDA + 2 * fi + mi;          // row tile mi = block rows 2 r + mi (interleaved, as everywhere)
  const float* Ap2 = As + fk * T::LDA + 64 + fi;             // row tile 2 = block rows 64 + r
  const int boff = fk * 64 + nj * 32 + fi;
  for (int s = 0; s < nst; ++s) {
    gf_wait_vm<(T::STAGES - 2) * GF_NI>();
    __builtin_amdgcn_s_barrier();
    gd_stage_c<MT>(Ap + (size_t)s * 64 * T::LDA, Ap2 + (size_t)s * 64 * T::LDA, rg.ring + rbuf * GF_STAGE + boff, acc, acc2,
                   mi == 0, rg);
    rg.advance();
    rbuf = rbuf + 1 == T::STAGES ? 0 : rbuf + 1;
  }
}

// Saved out / gate values one epilogue tile needs: 32 MT rows x 1 channel per lane and tensor.  They are requested in GD_NB
// batches from inside the LAST GD_NB stages of the K loop that precedes the epilogue (gd_kloop), so their HBM latency hides
// under MFMA work instead of standing in front of every epilogue (measured: ~3 us per tile, 4 tiles per workgroup).  A batch
// must have landed by the next stage's counted wait (vmcnt retires in order), which a stage's 2048 MFMA cycles cover.
constexpr int GD_NB = 8;              // batches (= stages) a tile's loads are spread over
template <int MT>
struct GdSaved {
  float y[16][MT], g[16][MT];
};
// Buffer loads: ONE per-lane byte offset (row part that depends on the lane + channel) and a SCALAR offset per (register,
// tile) -- 64-bit per-element addresses cost two VGPRs each and, hoisted over a batch, pushed the 96-row kernel into
// scratch (every scratch reload drains the ring).  Rows >= M and dead channels fall outside num_records and read 0.
template <int MT, int NT, int J>
__device__ __forceinline__ void gd_load_batch(GdSaved<MT>& sv, int b, const float* __restrict__ y, const float* __restrict__ gt,
                                              int CP, int M, int m0, int lane, int wave) {
  const int fi = lane & 31, fk = lane >> 5;
  const int c = wave * 32 * NT + 32 * J + fi;
  const unsigned bytes = (unsigned)((size_t)M * CP * 4);
  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(y), 0, bytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gt), 0, bytes, 0x00020000);
  const int dead = c < CP ? 0 : 0x7fffffff;                                 // out of range -> 0
  const int v01 = ((m0 + 8 * fk) * CP + c) * 4 | dead, v2 = ((m0 + 64 + 4 * fk) * CP + c) * 4 | dead;
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    if (reg / (16 / GD_NB) != b) continue;           // (b is a compile-time constant at every call site)
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      // block row = [constant part] + [lane part]: tiles 0 / 1: 2 (reg & 3) + 16 (reg >> 2) + i  (+ 8 fk);  tile 2: (reg & 3) + 8 (reg >> 2)  (+ 64 + 4 fk)
      const int crow = i < 2 ? 2 * (reg & 3) + 16 * (reg >> 2) + i : (reg & 3) + 8 * (reg >> 2);
      const int so = __builtin_amdgcn_readfirstlane(crow * CP * 4);
      sv.y[reg][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(ry, i < 2 ? v01 : v2, so, 0));
      sv.g[reg][i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, i < 2 ? v01 : v2, so, 0));
    }
  }
}

// K loop of one product (phase).  PJ >= 0: the saved out / gate values of column tile PJ (tensors y / gt) are requested from
// inside the last GD_NB stages, one batch right behind each stage's barrier (P2 >= 0: a second tile into sv2 likewise).
template <int MT, int NT, int PJ, int P2>
__device__ __forceinline__ void gd_kloop(const float* As, GfRing& rg, int& rbuf, int nst, int lane, int wave,
                                         sg_f32x16 (&acc)[MT][NT], GdSaved<MT>& sv, GdSaved<MT>& sv2,
                                         const float* __restrict__ y, const float* __restrict__ gt, int CP, int M, int m0) {
  using T = GdTile<MT>;
  constexpr int NC = 128 * NT, RS = 32 / NT;
  const int fi = lane & 31, fk = lane >> 5;
  const float* Ap = As + fk * T::LDA + 2 * fi;
  const float* Ap2 = As + fk * T::LDA + 64 + fi;
  const int nhead = (PJ >= 0 && nst > GD_NB) ? nst - GD_NB : (PJ >= 0 ? 0 : nst);
  int s = 0;
  GdFrag pf;
#if GF_PRIVATE_RING
  // Private ring: NO barrier inside the K loop (gf_layer has the argument in full).  A wave reads only the weight slice its
  // own pieces filled, behind its own counted vmcnt wait; it re-requests into the buffer of stage s - 1 only from inside
  // stage s, when its own fragment reads of that buffer have returned (per-wave write-after-read).  ONE barrier at the
  // entry: the operand buffer (the prologue copy / the LDS rows of the epilogue before this loop, each wave behind its own
  // lgkmcnt(0)) is complete before the loop's first read of it; the barrier ahead of every epilogue (in the kernel body)
  // keeps the epilogue from overwriting it under a reader.  The third product (gd_kloop_c) stays on the barrier form: two
  // waves share a column tile of its weights; its first stage barrier also covers the hand-over from this form.
  const int boff = wave * GF_WSLICE + fk * (NC / 4) + (NT == 2 ? 2 * fi : fi);
  gf_wait_vm<(T::STAGES - 2) * GF_NI>();               // my pieces of the loop's first stage have landed
  __builtin_amdgcn_s_barrier();                        // the operand in LDS is complete
#if GF_XPF
  gd_frag_load<MT, NT>(Ap, Ap2, rg.ring + rbuf * GF_STAGE + boff, pf);
#endif
  // every stage but the loop's last waits for and reads the start of the next one from inside (gd_stage<.., NEXT>)
  auto top = [&]() __attribute__((always_inline)) {    // GF_XPF=0: a stage's own wait, where the shared form has it
#if !GF_XPF
    if (s) gf_wait_vm<(T::STAGES - 2) * GF_NI>();
#endif
  };
  auto stage = [&](auto next) __attribute__((always_inline)) {
    const int nbuf = rbuf + 1 == T::STAGES ? 0 : rbuf + 1;
    gd_stage<MT, NT, decltype(next)::value>(Ap + (size_t)s * RS * T::LDA, Ap2 + (size_t)s * RS * T::LDA,
                                            rg.ring + rbuf * GF_STAGE + boff, rg.ring + nbuf * GF_STAGE + boff, acc, rg, pf);
    rg.advance();
    rbuf = nbuf;
    ++s;
  };
  if constexpr (PJ >= 0) {
    while (s < nhead) { top(); stage(std::true_type{}); }   // (nhead > 0 only with the full tail behind it)
    // tail: stage s of the last min(nst, GD_NB) carries batch (GD_NB - (nst - s)); batches a short loop has no stage
    // for go out ahead of it.  The last batch's stage is the loop's last (peeled: NEXT is a compile-time property)
    const int first = nst < GD_NB ? GD_NB - nst : 0;
    auto tail = [&](int b, auto next) __attribute__((always_inline)) {
      if (b >= first) top();
      gd_load_batch<MT, NT, PJ>(sv, b, y, gt, CP, M, m0, lane, wave);
      if constexpr (P2 >= 0) gd_load_batch<MT, NT, P2>(sv2, b, y, gt, CP, M, m0, lane, wave);
      if (b >= first) stage(next);
    };
#pragma unroll
    for (int b = 0; b < GD_NB - 1; ++b) tail(b, std::true_type{});
    tail(GD_NB - 1, std::false_type{});
  } else {
    while (s + 1 < nhead) { top(); stage(std::true_type{}); }
    if (s < nhead) { top(); stage(std::false_type{}); }
  }
#else
  const int boff = fk * NC + (NT == 2 ? wave * 64 + 2 * fi : wave * 32 + fi);
  for (; s < nhead; ++s) {
    gf_wait_vm<(T::STAGES - 2) * GF_NI>();
    __builtin_amdgcn_s_barrier();
    const float* Bs = rg.ring + rbuf * GF_STAGE + boff;
    gd_stage<MT, NT, false>(Ap + (size_t)s * RS * T::LDA, Ap2 + (size_t)s * RS * T::LDA, Bs, Bs, acc, rg, pf);
    rg.advance();
    rbuf = rbuf + 1 == T::STAGES ? 0 : rbuf + 1;
  }
  if constexpr (PJ >= 0) {
    // tail: stage s of the last min(nst, GD_NB) carries batch (GD_NB - (nst - s)); batches a short loop has no stage
    // for go out ahead of it
    const int first = nst < GD_NB ? GD_NB - nst : 0;
#pragma unroll
    for (int b = 0; b < GD_NB; ++b) {
      if (b >= first) {
        gf_wait_vm<(T::STAGES - 2) * GF_NI>();
        __builtin_amdgcn_s_barrier();
      }
      gd_load_batch<MT, NT, PJ>(sv, b, y, gt, CP, M, m0, lane, wave);
      if constexpr (P2 >= 0) gd_load_batch<MT, NT, P2>(sv2, b, y, gt, CP, M, m0, lane, wave);
      if (b >= first) {
        const float* Bs = rg.ring + rbuf * GF_STAGE + boff;
        gd_stage<MT, NT, false>(Ap + (size_t)s * RS * T::LDA, Ap2 + (size_t)s * RS * T::LDA, Bs, Bs, acc, rg, pf);
        rg.advance();
        rbuf = rbuf + 1 == T::STAGES ? 0 : rbuf + 1;
        ++s;
      }
    }
  }
#endif
}

// GLU backward of column tile J of the accumulators: -> d(pre-activation) of the layer below in HBM (pair order) and, when
// TO_LDS, into the operand buffer as rows 2 (wave 32 + lane) + t of the coming phase
template <int MT, int NT, int J, bool TO_LDS>
__device__ __forceinline__ void gd_epilogue(const sg_f32x16 (&acc)[MT][NT], float* As, const GdSaved<MT>& sv,
                                            float* __restrict__ dpre, int CP, int M, int m0, int lane, int wave) {
  using T = GdTile<MT>;
  const int fi = lane & 31;
  const int c = wave * 32 * NT + 32 * J + fi;
  const bool live = c < CP;
  const int q = ((c >> 4) << 5) + (c & 15);
  const int k0 = 2 * (wave * 32 + fi);
  // the three products per value are formed twice -- for the LDS rows (every lane) and again inside the store loop (live
  // lanes) -- rather than kept in 2 x 16 x MT registers across both
  auto lr = [&](int reg, int i, float& left, float& right) {
    const float d = acc[i][J][reg];
    left = d * sv.g[reg][i];
    right = d * sv.y[reg][i] * (1.f - sv.g[reg][i]);
  };
  if constexpr (TO_LDS) {
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
      const int rl = 2 * g2_row_of(reg, lane);
      float l[3], r[3];
#pragma unroll
      for (int i = 0; i < MT; ++i) lr(reg, i, l[i], r[i]);
      *reinterpret_cast<float2*>(As + k0 * T::LDA + rl) = make_float2(l[0], l[1]);
      *reinterpret_cast<float2*>(As + (k0 + 1) * T::LDA + rl) = make_float2(r[0], r[1]);
      if constexpr (MT == 3) {
        As[k0 * T::LDA + 64 + g2_row_of(reg, lane)] = l[2];
        As[(k0 + 1) * T::LDA + 64 + g2_row_of(reg, lane)] = r[2];
      }
    }
  }
  // ONE lane predicate around the whole store loop: a per-store test puts every store pair into its own basic block, and
  // hipcc then waits vmcnt(0) in each (the prefetched operands look pending at every join) -- the stores serialise
  float* dp = dpre + (size_t)m0 * 2 * CP + q;
  const bool full = m0 + T::BM <= M;
  if (!(GF_ABL & 1) && live) {
    if (full) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const size_t off = (size_t)GfTile<MT>::row(i, reg, lane) * 2 * CP;
          float l, r;
          lr(reg, i, l, r);
          GF_ST(&dp[off], l);
          GF_ST(&dp[off + 16], r);
        }
    } else {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg)
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          const int rl = GfTile<MT>::row(i, reg, lane);
          float l, r;
          lr(reg, i, l, r);
          if (m0 + rl < M) {
            GF_ST(&dp[(size_t)rl * 2 * CP], l);
            GF_ST(&dp[(size_t)rl * 2 * CP + 16], r);
          }
        }
    }
  }
}

template <int MT, int NT>
static __global__ __launch_bounds__(256, 1) void sg_glu_fused_dgrad_kernel(const GdArgs g) {
  using T = GdTile<MT>;
  extern __shared__ __attribute__((aligned(16))) float gf_lds[];   // ONE array: As[KA][LDA] then the ring
  float* As = gf_lds;
  const int L = blockIdx.x, xcd = L & 7;
  const int r = (xcd >> 2) & 1, rb = (L >> 3) * 4 + (xcd & 3);
  if (rb >= g.nrb) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int m0 = rb * T::BM, M = g.M, CP = g.CP;
  constexpr int RS = 32 / NT;

  GfRing rg;
  rg.ring = gf_lds + (size_t)g.KA * T::LDA;
  rg.wave = wave;
  rg.nstages = T::STAGES;
  rg.src = g.wd[r] + (size_t)wave * GF_NI * 256 + lane * 4;
  rg.next = 0; rg.last = g.ns[r] - 1; rg.wbuf = 0;
#pragma unroll
  for (int p = 0; p < T::STAGES - 1; ++p) {
#pragma unroll
    for (int q = 0; q < GF_NI; ++q) rg.issue(q);
    rg.advance();
  }
  {  // operand of the first product: the block's d(pre-activation) rows of layer 2, K-major; rows np2 .. nstA * RS - 1 zero
    // a wave moves 16 rows x 4 k-quads per step, the quads 2 apart: the four ds_write_b32 of a lane's float4 then land in
    // rows 8 apart = 16 banks apart per quad, 64 distinct banks per instruction (the row-per-wave mapping was 8-way
    // conflicted); the other parity of the quads is the next step, so every 128-byte line is still used in full
    const int np2 = g.np2[r], nq = np2 >> 2;
    const float* src = g.dact2[r] + (size_t)m0 * np2;
    const int rows = M - m0 < T::BM ? M - m0 : T::BM;
    const int r16 = lane & 15, a4 = lane >> 4;
    const int nkc = (nq + 7) >> 3;                      // chunks of 8 k-quads
    const int nitem = (T::BM / 16) * nkc * 2;
#if GF_G_BATCH
    // as the forward's G copy: a wave's float4 loads GF_G_BATCH at a time, all requested before the first LDS write
    for (int base = wave; base < nitem; base += 4 * GF_G_BATCH) {
      float4 v[GF_G_BATCH];
#pragma unroll
      for (int j = 0; j < GF_G_BATCH; ++j) {
        const int item = base + 4 * j;
        const int par = item & 1, kc = (item >> 1) % nkc, rblk = (item >> 1) / nkc;
        const int i = 16 * rblk + r16, kq = kc * 8 + 2 * a4 + par;
        const bool ok = item < nitem && i < rows && kq < nq;
        v[j] = *reinterpret_cast<const float4*>(src + (ok ? (size_t)i * np2 + 4 * kq : 0));
      }
#pragma unroll
      for (int j = 0; j < GF_G_BATCH; ++j) {
        const int item = base + 4 * j;
        const int par = item & 1, kc = (item >> 1) % nkc, rblk = (item >> 1) / nkc;
        const int i = 16 * rblk + r16, kq = kc * 8 + 2 * a4 + par;
        const bool ok = i < rows && kq < nq;
        if (item < nitem && kq < nq) {
          float* d = As + (4 * kq) * T::LDA + i;
          d[0] = ok ? v[j].x : 0.f;
          d[T::LDA] = ok ? v[j].y : 0.f;
          d[2 * T::LDA] = ok ? v[j].z : 0.f;
          d[3 * T::LDA] = ok ? v[j].w : 0.f;
        }
      }
    }
#else
    for (int item = wave; item < nitem; item += 4) {
      const int par = item & 1, kc = (item >> 1) % nkc, rblk = (item >> 1) / nkc;
      const int i = 16 * rblk + r16, kq = kc * 8 + 2 * a4 + par;
      const bool ok = i < rows && kq < nq;
      const float4 v = *reinterpret_cast<const float4*>(src + (ok ? (size_t)i * np2 + 4 * kq : 0));
      if (kq < nq) {
        float* d = As + (4 * kq) * T::LDA + i;
        d[0] = ok ? v.x : 0.f;
        d[T::LDA] = ok ? v.y : 0.f;
        d[2 * T::LDA] = ok ? v.z : 0.f;
        d[3 * T::LDA] = ok ? v.w : 0.f;
      }
    }
#endif
    const int kend = g.nstA[r] * RS;
    for (int idx = tid; idx < (kend - np2) * T::BM; idx += 256) As[(np2 + idx / T::BM) * T::LDA + (idx % T::BM)] = 0.f;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  int rbuf = 0;
  sg_f32x16 acc1[MT][NT], acc0[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) { acc1[i][j][e] = 0.f; acc0[i][j][e] = 0.f; }
  // The saved out / gate values of the coming epilogue are requested from inside the last stages of the K loop before it
  // (PRE; `load_now` is the unpipelined form, kept for A/B: ~3 us exposed per epilogue tile).  With buffer loads (one
  // VGPR of addressing) both forms fit the register file without scratch at 64- and at 96-row blocks.
  constexpr bool PRE = true;
  GdSaved<MT> sva, svb;
  auto load_now = [&](GdSaved<MT>& sv, auto jtag, const float* y, const float* gt) {
    constexpr int J = decltype(jtag)::value;
#pragma unroll
    for (int b = 0; b < GD_NB; ++b) gd_load_batch<MT, NT, J>(sv, b, y, gt, CP, M, m0, lane, wave);
  };
  using J0 = std::integral_constant<int, 0>;
  using J1 = std::integral_constant<int, 1>;
  gd_kloop<MT, NT, (PRE ? 0 : -1), -1>(As, rg, rbuf, g.nstA[r], lane, wave, acc1, sva, svb, g.out1[r], g.gate1[r], CP, M, m0);   // d(out of layer 1)
  if constexpr (!PRE) load_now(sva, J0{}, g.out1[r], g.gate1[r]);
  __builtin_amdgcn_s_barrier();                                      // every wave is done reading the operand buffer
  gd_epilogue<MT, NT, 0, true>(acc1, As, sva, g.dact1[r], CP, M, m0, lane, wave);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if constexpr (NT == 2) {
    gd_kloop<MT, NT, (PRE ? 1 : -1), -1>(As, rg, rbuf, g.nstB[0], lane, wave, acc0, sva, svb, g.out1[r], g.gate1[r], CP, M, m0);  // phase 0
    if constexpr (!PRE) load_now(sva, J1{}, g.out1[r], g.gate1[r]);
    __builtin_amdgcn_s_barrier();
    gd_epilogue<MT, NT, 1, true>(acc1, As, sva, g.dact1[r], CP, M, m0, lane, wave);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gd_kloop<MT, NT, (PRE ? 0 : -1), (PRE ? 1 : -1)>(As, rg, rbuf, g.nstB[1], lane, wave, acc0, sva, svb, g.out0[r], g.gate0[r], CP, M, m0);
  } else {
    gd_kloop<MT, NT, (PRE ? 0 : -1), -1>(As, rg, rbuf, g.nstB[0], lane, wave, acc0, sva, svb, g.out0[r], g.gate0[r], CP, M, m0);
  }
  // third product: d(pre-activation) of layer 0 (stored for the weight gradients, kept in LDS phase by phase) -> dG slab
  sg_f32x16 accg, accg2;
#pragma unroll
  for (int e = 0; e < 16; ++e) { accg[e] = 0.f; accg2[e] = 0.f; }
  if constexpr (!PRE) load_now(sva, J0{}, g.out0[r], g.gate0[r]);
  __builtin_amdgcn_s_barrier();
  gd_epilogue<MT, NT, 0, true>(acc0, As, sva, g.dact0[r], CP, M, m0, lane, wave);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  gd_kloop_c<MT>(As, rg, rbuf, g.nstC[0], lane, wave, accg, accg2);
  if constexpr (NT == 2) {
    if constexpr (!PRE) load_now(sva, J1{}, g.out0[r], g.gate0[r]);
    __builtin_amdgcn_s_barrier();
    gd_epilogue<MT, NT, 1, true>(acc0, As, (PRE ? svb : sva), g.dact0[r], CP, M, m0, lane, wave);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    gd_kloop_c<MT>(As, rg, rbuf, g.nstC[1], lane, wave, accg, accg2);
  }
  {
    const int kin = (wave & 1) * 32 + (lane & 31), mi = wave >> 1;
    float* pg = g.dG[r] + (size_t)m0 * g.KG + kin;
    if (!(GF_ABL & 1) && kin < g.KG) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int rl = 2 * g2_row_of(reg, lane) + mi;
        if (m0 + rl < M) pg[(size_t)rl * g.KG] = accg[reg];
        if constexpr (MT == 3) {
          const int r2 = 64 + g2_row_of(reg, lane);
          if (mi == 0 && m0 + r2 < M) pg[(size_t)r2 * g.KG] = accg2[reg];
        }
      }
    }
  }
  gf_wait_vm<0>();
}
