// Cluster recurrence v4 (U = ceil(Hd/P) <= 64; forward: any P <= 8, backward: P <= 4 and P = 6): WAVE SPECIALISATION.
//
// What bounds a recurrence step is not FLOPs or bytes but the number of instructions the busiest wave has to ISSUE (a wave
// issues one instruction every ~4-5 cycles whatever its kind; measured with -DGRU_PROF, profiles/r02_gru_phase_cycles.txt,
// profiles/r02_gru_wave_specialisation.md): in the v2 / v3 kernels wave 0 ran the gate phase (LDS partial sums, gate math,
// granule stores), the global loads of the next step's inputs with their 64-bit address arithmetic, the global stores of
// the saved gates AND its own mat-vec slice -- 800-930 cycles of gate phase plus a 1100-cycle mat-vec, the whole critical
// path of the step, while the other waves sat in their poll loops.  Here the waves of a workgroup have roles:
//   * the MAT-VEC waves -- forward: P of them, owner slice q for all three gates (one broadcast of h_k serves three
//     v_pk_fma); backward: 3P, (gate g, owner slice q) -- poll their slice's granules (the workgroup's own units included:
//     every slice arrives through the exchange), multiply, leave a partial sum in LDS.  Nothing else: a global store or
//     load issued ahead of a poll would hold the poll back (vmcnt retires in order).
//     Lane maps of the multiply (the poll is always lane = k of the slice).  Forward, slices of 33..40 units: lane l of
//     lane set t holds output 64 t + l = gate * U + unit, every k (GRU_FWD_PACK); otherwise lane = unit for three gates.
//     Backward, one slice per wave and KU > 32: lanes l and 32 + l hold the units 2 l and 2 l + 1, the lower half of the
//     wave the k pairs (4i, 4i+1), the upper half (4i+2, 4i+3); lane l ends with the sum of unit 2 l, lane 32 + l with
//     that of 2 l + 1 (GRU_BWD_FOLD); KU = 32 and two slices per wave (P = 6): lane = unit, every k.
//   * ONE GATE wave: barrier -> partial sums and inputs from LDS -> gate math -> granule stores -> results into an LDS
//     stash.  No global loads, no global data stores, no mat-vec.
//   * ONE CHORE wave: it fetches the next step's gate inputs from global memory into LDS (one step ahead), moves the
//     previous step's stash to global memory and, in the backward, accumulates dW_ih | db_ih from the gate gradients
//     passing through it.  It never polls, so it may wait for its memory operations at leisure.
//   * Timing: the chore wave and the pollers SLEEP through the gate phase.  The CU's vector-memory pipeline is in order; a
//     granule store queued behind HBM loads or behind a dozen waves' poll loads reaches the L2 late and every partner of
//     the cluster waits for it.  The sleep lengths (GRU_CHORE_SLEEP_*, GRU_POLL_PRE_*) are tuned on MI355X and only
//     affect speed, never the result.
// The arithmetic (mat-vec chains, order of the partial sums, gate formulas) is that of the v2 kernels: with the same P the
// hidden states are bit-identical, the gradients agree to rounding (the compiler contracts the gate-gradient products
// differently in the two kernels) (tests/test_hip_gru_eigh.py).  LDS buffers are double buffered by step parity; the
// hand-offs (who writes / reads which parity between which two barriers) are spelled out at each kernel below.
#pragma once

// A/B hook (-DGRU_PUB_PUSH=n): what the gate wave does right after its granule stores.  0: nothing; 1: wait for their
// acknowledgement; 2: a dummy L2 load behind them; 3: the stores carry sc0 (gru_publish_x)
#ifndef GRU_PUB_PUSH
#define GRU_PUB_PUSH 0
#endif
__device__ __forceinline__ void gru4_after_publish(const gru_u64* g) {
#if GRU_PUB_PUSH == 1
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#elif GRU_PUB_PUSH == 2
  gru_u64 x;
  asm volatile("global_load_dwordx2 %0, %1, off sc1" : "=v"(x) : "v"(g) : "memory");
  asm volatile("" :: "v"(x));
#else
  (void)g;
#endif
}
// Poll of one granule per lane in the mat-vec waves.  GRU_POLL_MODE bit 0: two loads in flight, half a round trip apart
// (the expected wait for the NEXT look at the granule after it lands is a quarter of a round trip instead of a half);
// PRE (x 64 cycles): sleep first -- nothing can arrive before the gate phase of the producers is over, and an idle
// memory pipeline lets their granule stores through sooner.
#ifndef GRU_POLL_MODE
#define GRU_POLL_MODE 0
#endif
#ifndef GRU_POLL_PRE_F
#define GRU_POLL_PRE_F 9      // (12 with the libm gate math of rounds 2-3; 10 with GRU_FAST_GATES in round 4; 9 with the packed mat-vec
                              //  and the vector partial-sum reads, together with GRU_CHORE_SLEEP_F: profiles/gru_packed_ab.txt)
#endif
#ifndef GRU_POLL_PRE_B
#define GRU_POLL_PRE_B 9
#endif
#ifndef GRU_POLL_LOOP_SLEEP
#define GRU_POLL_LOOP_SLEEP 1
#endif
#include "gru_math.h"

template <int PRE>
__device__ __forceinline__ float gru4_poll(const gru_u64* g, unsigned tag, bool active, int* status) {
  if (PRE > 0) __builtin_amdgcn_s_sleep(PRE);
#if (GRU_POLL_MODE & 1)
  float v = 0.f;
  if (active) {
    gru_u64 a = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __builtin_amdgcn_s_sleep(2);
    gru_u64 b = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    for (;;) {
      if ((unsigned)(a >> 32) == tag) { v = __uint_as_float((unsigned)a); break; }
      a = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((unsigned)(b >> 32) == tag) { v = __uint_as_float((unsigned)b); break; }
      b = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (++spins > (1u << 22)) { atomicExch(status, 1); break; }
    }
  }
  return v;
#else
  float v = 0.f;
  if (active) {
    gru_u64 x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    unsigned spins = 0;
    while ((unsigned)(x >> 32) != tag) {
      if (GRU_POLL_LOOP_SLEEP > 0) __builtin_amdgcn_s_sleep(GRU_POLL_LOOP_SLEEP);
      x = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (++spins > (1u << 22)) { atomicExch(status, 1); break; }   // partner not resident / lost: give up, flag it
    }
    v = __uint_as_float((unsigned)x);
  }
  return v;
#endif
}
// two granules per lane (the two owner slices of an OW = 2 mat-vec wave): both loads go out before the first spin
template <int PRE>
__device__ __forceinline__ void gru4_poll2(const gru_u64* g0, const gru_u64* g1, unsigned tag, bool act0, bool act1,
                                           int* status, float (&v)[2]) {
  if (PRE > 0) __builtin_amdgcn_s_sleep(PRE);
  gru_u64 x0 = __hip_atomic_load(g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (inactive lanes read a valid granule
  gru_u64 x1 = __hip_atomic_load(g1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     //  of the slice and ignore it)
  unsigned spins = 0;
  while (act0 && (unsigned)(x0 >> 32) != tag) {
    if (GRU_POLL_LOOP_SLEEP > 0) __builtin_amdgcn_s_sleep(GRU_POLL_LOOP_SLEEP);
    x0 = __hip_atomic_load(g0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (++spins > (1u << 22)) { atomicExch(status, 1); break; }
  }
  spins = 0;
  while (act1 && (unsigned)(x1 >> 32) != tag) {
    if (GRU_POLL_LOOP_SLEEP > 0) __builtin_amdgcn_s_sleep(GRU_POLL_LOOP_SLEEP);
    x1 = __hip_atomic_load(g1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (++spins > (1u << 22)) { atomicExch(status, 1); break; }
  }
  v[0] = act0 ? __uint_as_float((unsigned)x0) : 0.f;
  v[1] = act1 ? __uint_as_float((unsigned)x1) : 0.f;
}
// A/B hooks, default on; 0 restores the instruction streams they replaced (csrc/Makefile: libstemgnn_hip_gruref.so has
// all three off).  None changes a bit of the results (tests/test_hip_gru_packed.py, tests/test_hip_gru_bwd_fold.py).
// GRU_FWD_PACK: forward mat-vec waves of the KU = 34 and 40 instantiations (slices of 33..40 units) hold lane -> (gate,
//   unit) over two lane sets instead of lane -> unit for three gates: two v_pk_fma per k-pair instead of three
//   (gru_matvec2).  KU = 32 (slices of <= 32 units: hidden <= 224, the small models) stays unpacked: nothing was measured
//   to pay there, and the packed kernel's footprint moved the timing of those few-microsecond steps enough to flip the
//   train step's overlapped-or-serialised schedule decision from run to run.
// GRU_PART_VEC: the partial sums lie with the slice index contiguous per output, so the gate wave fetches them with
//   ds_read_b128 (forward P = 7: six instead of 21 ds_read_b32; backward P = 4: three instead of 12).
// GRU_BWD_FOLD: backward mat-vec waves of the OW = 1 instantiations (P = 1, 2, 4) with KU = 48, 58, 64 hold lane -> two
//   units (2 l, 2 l + 1 in lanes l and 32 + l) and split the k pairs over the two lane halves instead of lane -> unit for
//   every k (gru_matvec_fold): a lane needs half of the polled values, read from the wave's LDS row with ds_read_b64, and
//   no v_readlane; three v_permlane32_swap + add rounds form each unit's sum in gru_matvec's association.  OW = 2 (P = 6)
//   keeps the readlane mat-vec: folded, the two slices' 128 weight registers and 32 values in flight leave <6,64,2> at 168
//   registers with 64 bytes of scratch (spills) under its 170-register bound.  KU = 32 (reached with P = 1 only: hidden
//   <= 32, the small models) keeps it too, for the forward's reason: nothing to gain in those few-microsecond steps, and
//   the folded kernel moved their timing enough to flip the train step's schedule decision.
#ifndef GRU_FWD_PACK
#define GRU_FWD_PACK 1
#endif
#ifndef GRU_BWD_FOLD
#define GRU_BWD_FOLD 1
#endif
#ifndef GRU_PART_VEC
#define GRU_PART_VEC 1
#endif
// Row stride (floats) of n contiguous partial sums: whole float4s, an ODD number of them -- the 16 lanes of a ds_read_b128
// group then fall on 16 different 16-byte slots of the 256-byte bank row (the writers' ds_write_b32 are 4-way, off the
// gate wave).  n <= 4: 4, n <= 12: 12.
constexpr int gru4_part_stride(int n) { return 4 * (((n + 3) / 4) | 1); }
// Partial sums of one step parity as rows x slices.  at(row, q): VEC row-major with the padded stride, else slice-major
// (the unpacked forward and the backward then keep the [gate * P + q][lane] / [wave][lane] image they always had).
template <int ROWS, int N, int P = 0>           // P > 0: the unpacked forward, row = 64 gate + lane
struct Gru4Part {
  static constexpr int PS = gru4_part_stride(N);
  static constexpr int FLOATS = GRU_PART_VEC ? ROWS * PS : ROWS * N;
  static __device__ __forceinline__ int at(int row, int q) {
#if GRU_PART_VEC
    return row * PS + q;
#else
    return P > 0 ? ((row >> 6) * P + q) * 64 + (row & 63) : q * ROWS + row;
#endif
  }
  // acc + the N partial sums of `row`, added in slice order
  static __device__ __forceinline__ float sum(const float* part, int row, float acc) {
#if GRU_PART_VEC
    float4 v[PS / 4];
#pragma unroll
    for (int i = 0; i < (N + 3) / 4; ++i) v[i] = *reinterpret_cast<const float4*>(part + row * PS + 4 * i);
#pragma unroll
    for (int q = 0; q < N; ++q) {
      const float4 t = v[q >> 2];
      acc += (q & 3) == 0 ? t.x : ((q & 3) == 1 ? t.y : ((q & 3) == 2 ? t.z : t.w));
    }
#else
#pragma unroll
    for (int q = 0; q < N; ++q) acc += part[at(row, q)];
#endif
    return acc;
  }
};
// upper bound of the static LDS of the backward kernel (its `part` is 64 rows of up to 3 P partial sums)
constexpr int gru4_static_lds_floats(int P, int nin, int nout) {
  return 2 * 64 * (GRU_PART_VEC ? gru4_part_stride(3 * P) : 3 * P) + 3 * P * 64 + 2 * nin * 64 + 2 * nout * 64;
}

// dynamic LDS the PACKED forward instantiations reserve without using it (see the launcher): what is left of 156 KiB
// beside their static part[2][128 rows] + lrow + gin + stash; 0 = the instantiation does not pack
constexpr bool gru4_fwd_packs(int KU) { return GRU_FWD_PACK != 0 && KU > 32 && KU <= 40; }
constexpr bool gru4_bwd_folds(int KU, int OW) { return GRU_BWD_FOLD != 0 && OW == 1 && KU > 32; }
constexpr size_t gru4_fwd_hog_bytes(int P, int KU) {
  return gru4_fwd_packs(KU)
             ? (size_t)156 * 1024 - sizeof(float) * (2 * 128 * (GRU_PART_VEC ? gru4_part_stride(P) : P) + P * 64 + 2 * 3 * 64 + 2 * 5 * 64)
             : 0;
}
// ---- forward ------------------------------------------------------------------------------------------------------
// Waves 0 .. P-1: mat-vec of owner slice q for all three gates (one broadcast per k serves three v_pk_fma, as in the v3
// kernel: 4 polling waves instead of 12), wave P: gates, wave P+1: chores.
// barrier #s closes the mat-vec of step s.  part[s&1]: written by the mat-vec waves before barrier #s, read by the gate
// wave between #s and #s+1, rewritten before #s+2.  gin[s&1] (the gi values of step s): written by the chore wave right
// after #s-1 from registers it loaded a step earlier, read by the gate wave after #s.  stash[s&1]: written by the gate
// wave between #s and #s+1, moved to global memory by the chore wave between #s+1 and #s+2, rewritten after #s+2.
// The chore wave issues its global loads / stores only after a pause that lets the gate wave's granule stores go first:
// the CU's memory pipeline is in order, and a granule store queued behind HBM loads costs the whole cluster a step time.
constexpr int GRU4_WMAX = 16;            // window lengths up to this have dW_ih accumulated inside the backward recurrence
// x 64 cycles after the barrier (the forward gate phase takes ~600).  The chore wave is IN the step's barrier: with the
// packed mat-vec its pause of 20, not the mat-vec waves, closed the step.  Forward in the step at PEMS07, pause 24 / 20 / 18 /
// 17 / 16 / 15 / 14: 242 / 220 / 210 / 206 / 202 / 201 / 217 us (profiles/gru_packed_ab.txt): below 15 its loads and stores
// get in front of the granule stores; 16 keeps two notches from that edge.
#ifndef GRU_CHORE_SLEEP_F
#define GRU_CHORE_SLEEP_F 16
#endif
#ifndef GRU_SW_MODE
#define GRU_SW_MODE 0                    // store wave of the backward (progress-publishing launches): 0 = write-through stores
#endif
#ifndef GRU_SW_SLEEP
#define GRU_SW_SLEEP 30                  // ... issued this long (x 64 clocks) behind the step's barrier: AFTER the gate wave's granule
#endif                                   // stores (measured, backward recurrence at PEMS07: sleep 0 / 10: 304 / 300 us, 30: 268; plain stores 268, none 259)
// x 64 cycles after the barrier (the backward gate phase takes ~450).  As in the forward, the chore wave is in the step's
// barrier: behind the folded mat-vec its pause of 10 closed the step.  Backward in the step at PEMS07, pause 14 / 12 / 10 / 9 /
// 8 / 7 / 6 / 5 / 4: 263 / 254 / 244 / 241 / 237 / 236 / 239 / 252 / 254 us (profiles/gru_bwd_fold_ab.txt): at 5 and below its
// loads and stores get in front of the granule stores; 7 keeps two notches from that edge.  The instantiations that do not
// fold (two slices per wave, KU = 32, or GRU_BWD_FOLD = 0) keep the 10 tuned for the readlane mat-vec (GRU_CHORE_SLEEP_B_RL).
#ifndef GRU_CHORE_SLEEP_B
#define GRU_CHORE_SLEEP_B 7
#endif
#ifndef GRU_CHORE_SLEEP_B_RL
#define GRU_CHORE_SLEEP_B_RL 10
#endif
template <int P, int KU, bool RS = true>     // RS = false: no `reserve` stores (stemgnn_gru_fwd_infer)
__global__ __launch_bounds__((P + 2) * 64) void gru_fwd_cluster4_kernel(const float* __restrict__ gi, const float* __restrict__ w_hh,
                                                                        const float* __restrict__ b_hh, int B, int S, int Hd,
                                                                        gru_u64* __restrict__ xbuf, int* __restrict__ status,
                                                                        float* __restrict__ h_all, float* __restrict__ reserve,
                                                                        gru_u64* __restrict__ xid, int allow_fast) {
  // PACK: the mat-vec waves' outputs are o = 64 set + lane = gate * U + unit (U by the cluster, the same in every
  // workgroup); outputs with unit >= un or o >= 3 U hold zero weights.  Otherwise row 64 gate + lane, lane = unit.
  constexpr bool PACK = gru4_fwd_packs(KU);
  typedef Gru4Part<PACK ? 128 : 192, P, PACK ? 0 : P> Part;
  __shared__ __attribute__((aligned(16))) float part[2][Part::FLOATS];
  __shared__ __attribute__((aligned(16))) float lrow[P][64];
  __shared__ float gin[2][3][64];
  __shared__ float stash[2][5][64];                      // r, z, n, W_hn h + b_hn, h
  __shared__ int s_fast;
  int b, p;
  gru_cluster_ids(B, P, b, p);
  if (b >= B) return;
  const bool fast = P > 1 && gru_same_xcd(xid + (size_t)b * P, p, P, allow_fast, status, &s_fast, threadIdx.x);
  const int U = (Hd + P - 1) / P;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = gru_uniform(tid >> 6);
  const int u0 = p * U, un = max(0, min(Hd, u0 + U) - u0);
  const int H3 = 3 * Hd;
  const bool lane_ok = lane < un;
  const int gu = u0 + (lane_ok ? lane : 0);
  // A workgroup that owns no unit (the last ones of a cluster whose slices overshoot Hd: Hd = 16 on seven workgroups)
  // has nothing to publish or to store, so no partner ever waits for it -- and then nothing keeps it in step either: two
  // steps late (waves of another kernel on its CU; with the packed kernels' 100 registers they fit) it misses a granule
  // for good and spins into the time-out.  It has taken part in the XCD check above, which its partners wait for.
  if (un == 0) return;

  if (wave < P) {
    // ---------------- mat-vec wave: owner slot q (rotated by p), gates r, z, n ----------------
    const int q = wave;
    const int k0 = ((q + p) % P) * U, kn = max(0, min(Hd, k0 + U) - k0);
    gru_f2 wr[3][32];                                    // lane = unit, three gates
    gru_f2 wp[2][GRU_PACK_KMAX / 2];                     // PACK: lane = (gate, unit), two lane sets
    if constexpr (PACK) {
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int o = 64 * t + lane, g = o / U, u = o - g * U;
        const bool live = o < 3 * U && u < un;
        const float* wrow = w_hh + (live ? ((size_t)g * Hd + u0 + u) * Hd : (size_t)0) + (kn > 0 ? k0 : 0);
#pragma unroll
        for (int kk = 0; kk < KU; ++kk) {
          const float v = wrow[kk < kn ? kk : 0];
          wp[t][kk >> 1][kk & 1] = (live && kk < kn) ? v : 0.f;
        }
      }
    } else {
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const float* wrow = w_hh + ((size_t)g * Hd + gu) * Hd + (kn > 0 ? k0 : 0);
#pragma unroll
        for (int kk = 0; kk < KU; ++kk) {
          const float v = wrow[kk < kn ? kk : 0];
          wr[g][kk >> 1][kk & 1] = (lane_ok && kk < kn) ? v : 0.f;
        }
      }
    }
    const gru_u64* pollp = xbuf + (size_t)b * Hd + k0 + (lane < kn ? lane : 0);      // parity 0; parity 1 is B*Hd further
    const size_t par = (size_t)B * Hd;
#ifdef GRU_PROF
    long long c_a = 0, c_b = 0, c_c = 0;
#endif
    for (int s = 0; s < S; ++s) {
      GRU_T(t0);
      float hv = 0.f;
      if (s > 0) hv = gru4_poll<GRU_POLL_PRE_F>(pollp + (s & 1) * par, (unsigned)s, lane < kn, status);
      GRU_T(t1);
      GRU_ACC(c_a, t1, t0);
      float* pw = part[s & 1];
      if constexpr (PACK) {
        float o0, o1;
        gru_matvec2<KU, GRU_NR3(KU)>(wp[0], wp[1], hv, lrow[q], lane, o0, o1);
        pw[Part::at(lane, q)] = o0;
        pw[Part::at(64 + lane, q)] = o1;
      } else {
        float o0, o1, o2;
        gru_matvec3<KU, GRU_NR3(KU)>(wr[0], wr[1], wr[2], hv, lrow[q], lane, o0, o1, o2);
        pw[Part::at(lane, q)] = o0;
        pw[Part::at(64 + lane, q)] = o1;
        pw[Part::at(128 + lane, q)] = o2;
      }
      GRU_T(t2);
      GRU_ACC(c_b, t2, t1);
      gru_lds_barrier();                                 // #s
      GRU_T(t3);
      GRU_ACC(c_c, t3, t2);
    }
    gru_lds_barrier();                                   // the gate wave has finished step S - 1
#ifdef GRU_PROF
    if (blockIdx.x == 0 && lane == 0)
      printf("gru fwd4 mat-vec wave %d: per step cycles: poll %lld  matvec %lld  barrier wait %lld\n", wave, c_a / S, c_b / S, c_c / S);
#endif
  } else if (wave == P + 1) {
    // ---------------- chore wave ----------------
    const float* gip = gi + (size_t)b * H3 + gu;         // row (s, b) is s * B * H3 further
    const size_t grow = (size_t)B * H3;
    float v0 = gip[0], v1 = gip[Hd], v2 = gip[2 * Hd];  // gi values of step 0
    for (int s = 0; s < S; ++s) {
      gin[s & 1][0][lane] = v0;                          // (gate(s-2), the last reader of this parity, finished before #s-1)
      gin[s & 1][1][lane] = v1;
      gin[s & 1][2][lane] = v2;
      float r = 0.f, z = 0.f, n = 0.f, g2 = 0.f, hn = 0.f;
      if (s >= 2) {
        r = stash[s & 1][0][lane]; z = stash[s & 1][1][lane]; n = stash[s & 1][2][lane];
        g2 = stash[s & 1][3][lane]; hn = stash[s & 1][4][lane];
      }
      if (s > 0) __builtin_amdgcn_s_sleep(GRU_CHORE_SLEEP_F);   // let the granule stores of gate(s-1) go first
      if (s + 1 < S) {
        const float* gn = gip + (size_t)(s + 1) * grow;
        v0 = gn[0]; v1 = gn[Hd]; v2 = gn[2 * Hd];
      }
      if (s >= 2 && lane_ok) {
        const size_t rw = (size_t)(s - 2) * B + b;
        if constexpr (RS) {
          float* rs = reserve + rw * 4 * Hd + gu;
          rs[0] = r; rs[Hd] = z; rs[2 * Hd] = n; rs[3 * Hd] = g2;
        }
        h_all[rw * Hd + gu] = hn;
      }
      gru_lds_barrier();                                 // #s
    }
    gru_lds_barrier();                                   // the gate wave has finished step S - 1 (stash[(S-1)&1] is complete)
    for (int t = (S >= 2 ? S - 2 : S - 1); t < S; ++t) {
      const size_t rw = (size_t)t * B + b;
      if (lane_ok) {
        if constexpr (RS) {
          float* rs = reserve + rw * 4 * Hd + gu;
          rs[0] = stash[t & 1][0][lane]; rs[Hd] = stash[t & 1][1][lane]; rs[2 * Hd] = stash[t & 1][2][lane];
          rs[3 * Hd] = stash[t & 1][3][lane];
        }
        h_all[rw * Hd + gu] = stash[t & 1][4][lane];
      }
    }
  } else {
    // ---------------- gate wave ----------------
    const float bh0 = b_hh[gu], bh1 = b_hh[Hd + gu], bh2 = b_hh[2 * Hd + gu];
    float hown = 0.f;
    // partial-sum rows of this lane's unit, gates r, z, n (PACK: lanes beyond the slice read unit 0's and are never stored)
    const int row0 = PACK ? (lane < U ? lane : 0) : lane, rstep = PACK ? U : 64;
    gru_u64* pub = xbuf + (size_t)b * Hd + gu;           // parity 0
    const size_t par = (size_t)B * Hd;
#ifdef GRU_PROF
    long long c_a = 0, c_b = 0, c_c = 0;
#endif
    for (int s = 0; s < S; ++s) {
      GRU_T(t0);
      gru_lds_barrier();                                 // #s
      GRU_T(t1);
      GRU_ACC(c_a, t1, t0);
      const float* pr = part[s & 1];
      const float g0 = Part::sum(pr, row0, bh0), g1 = Part::sum(pr, row0 + rstep, bh1), g2 = Part::sum(pr, row0 + 2 * rstep, bh2);
      const float gp0 = gin[s & 1][0][lane], gp1 = gin[s & 1][1][lane], gp2 = gin[s & 1][2][lane];
      const float r = gru4_sigmoid(gp0 + g0);
      const float z = gru4_sigmoid(gp1 + g1);
      const float n = gru4_tanh(gp2 + r * g2);
      const float hn = (1.f - z) * n + z * hown;
      hown = hn;
      if (s + 1 < S && lane_ok) gru_publish_x(pub + ((s + 1) & 1) * par, (unsigned)(s + 1), hn, fast);
      gru4_after_publish(pub);
      GRU_T(t2);
      GRU_ACC(c_b, t2, t1);
      stash[s & 1][0][lane] = r;
      stash[s & 1][1][lane] = z;
      stash[s & 1][2][lane] = n;
      stash[s & 1][3][lane] = g2;
      stash[s & 1][4][lane] = hn;
      GRU_T(t3);
      GRU_ACC(c_c, t3, t2);
    }
    gru_lds_barrier();
#ifdef GRU_PROF
    if (blockIdx.x == 0 && lane == 0)
      printf("gru fwd4 gate wave: per step cycles: barrier wait %lld  gate phase to publish %lld  stash %lld\n", c_a / S, c_b / S, c_c / S);
#endif
  }
}

// ---- backward -----------------------------------------------------------------------------------------------------
// Barriers: B_init, then B_s (s = S-1 .. 1) closing the mat-vec of step s, then B_fin.  gate(s) runs between B_{s+1}
// and B_s.  part[tag&1] (tag = S-s): written by mat-vec(s) before B_s, read by gate(s-1).  bin[(s-1)&1]: inputs of
// gate(s-1), fetched by the chore wave during step s+1 and written at the top of step s (before B_s).  bout[s&1]: written by gate(s) before
// B_s, moved to global memory by the chore wave during step s-1 (before B_{s-1}), rewritten by gate(s-2) after that.
// OW = owner slices per mat-vec wave.  OW = 1 (P <= 4): 3P mat-vec waves.  OW = 2 (P = 6: hidden sizes 321..384, PEMS03's
// N = 358): 3P/2 waves that poll and multiply two slices per step, so that the workgroup stays inside 1024 threads with
// the gate and chore waves on top (3*6/2 + 2 = 11 waves: three per SIMD, 170 registers per lane -- the two slices' 128
// weight registers fit only with the all-readlane broadcast, NR = 64).  Both granule loads of a step are in flight
// before the first spin.
template <int P, int KU, int OW = 1, bool SW = false>     // SW: the progress-publishing launch (one more wave, the store wave)
__global__ __launch_bounds__((3 * P / OW + 2 + (SW ? 1 : 0)) * 64) void gru_bwd_cluster4_kernel(const float* __restrict__ dout, const float* __restrict__ w_hh,
                                                                            const float* __restrict__ h_all,
                                                                            const float* __restrict__ reserve, int B, int S, int Hd,
                                                                            gru_u64* __restrict__ xbuf, int* __restrict__ status,
                                                                            float* __restrict__ dgi, float* __restrict__ dghn,
                                                                            gru_u64* __restrict__ xid, int allow_fast,
                                                                            const float* __restrict__ x, float* __restrict__ ih_slab,
                                                                            int W, const float* __restrict__ dkey,
                                                                            const float* __restrict__ dquery,
                                                                            const float* __restrict__ wk, const float* __restrict__ wq,
                                                                            unsigned* __restrict__ prog, int prog_ts) {
  // prog != nullptr (round 5): the dW_hh product runs on another stream WHILE this kernel does (wgrad.h, WgArgs::phase).  The
  // chore wave then stores the gate gradients write-through (sc1: they leave this XCD's L2 for the fabric) and counts
  // prog[j] once per workgroup when its row of time step j * prog_ts -- the last of the chunk [j ts, (j+1) ts), the steps
  // run downwards -- has been stored AND drained (vmcnt(0)): a reader that sees prog[j] == B * P may load every row of a
  // time step >= j * prog_ts after one agent-scope acquire.
  // dkey != nullptr (round 4): the output gradient arrives FACTORED -- in the model dh[s][b][i] = dkey[b][i] wk[s] +
  // dquery[b][i] wq[s] (adjoint of key = sum_s h[s] wk[s], models/base_model.py:154-155), so the [S, B, Hd] tensor is never
  // written or read and the kernel that formed it leaves the backward's critical chain; `dout` is unused then
  static_assert(P % OW == 0 && (OW == 1 || OW == 2), "owner slices per wave");
  constexpr int NMV = 3 * P / OW;
  constexpr bool FOLD = gru4_bwd_folds(KU, OW);          // (else the readlane mat-vec: see GRU_BWD_FOLD)
  typedef Gru4Part<64, NMV> Part;                        // row = unit, one partial sum per mat-vec wave
  __shared__ __attribute__((aligned(16))) float part[2][Part::FLOATS];
  __shared__ __attribute__((aligned(16))) float lrow[NMV][64];
  __shared__ float bin[2][6][64];                        // dh_out, r, z, n, W_hn h + b_hn, h_prev
  __shared__ float bout[2][4][64];                       // dr, dz, dn, dn * r
  __shared__ int s_fast;
  int b, p;
  gru_cluster_ids(B, P, b, p);
  if (b >= B) return;
  const bool fast = P > 1 && gru_same_xcd(xid + (size_t)b * P, p, P, allow_fast, status, &s_fast, threadIdx.x);
  const int U = (Hd + P - 1) / P;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = gru_uniform(tid >> 6);
  const int u0 = p * U, un = max(0, min(Hd, u0 + U) - u0);
  const int H3 = 3 * Hd;
  const bool lane_ok = lane < un;
  const int gu = u0 + (lane_ok ? lane : 0);
  for (int i = tid; i < 2 * Part::FLOATS; i += (int)blockDim.x) (&part[0][0])[i] = 0.f;      // (the padding of the rows too)

  if (wave < NMV) {
    // ---------------- mat-vec wave (gate g, owner slot q rotated by p): reduction slice j = g*Hd + units of that owner
    const int g = wave / (P / OW), q0 = (wave - g * (P / OW)) * OW;
    gru_f2 wr[OW][32];                                   // lane = unit, every k
    gru_f2 wf[2][GRU_FOLD_PMAX];                         // FOLD: lane -> units 2 (lane & 31) + t, the k pairs of its half
    int kn[OW];
    const gru_u64* pollp[OW];                            // parity 0
#pragma unroll
    for (int o = 0; o < OW; ++o) {
      const int k0 = ((q0 + o + p) % P) * U;
      kn[o] = max(0, min(Hd, k0 + U) - k0);
      if constexpr (FOLD) {
        const int half = lane >> 5;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          const int j = 2 * (lane & 31) + t;
          const bool live = j < un;
          const float* wcol = w_hh + ((size_t)g * Hd + (kn[o] > 0 ? k0 : 0)) * Hd + u0 + (live ? j : 0);
#pragma unroll
          for (int i = 0; i < gru_fold_pairs(KU); ++i)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
              const int kk = 4 * i + 2 * half + c;
              const float v = wcol[(size_t)(kk < kn[o] ? kk : 0) * Hd];
              wf[t][i][c] = (live && kk < kn[o]) ? v : (kk < KU ? 0.f : -0.f);     // (kk >= KU: gru_matvec_fold)
            }
        }
      } else {
        const float* wcol = w_hh + ((size_t)g * Hd + (kn[o] > 0 ? k0 : 0)) * Hd + gu;
#pragma unroll
        for (int kk = 0; kk < KU; ++kk) {
          const float v = wcol[(size_t)(kk < kn[o] ? kk : 0) * Hd];
          wr[o][kk >> 1][kk & 1] = (lane_ok && kk < kn[o]) ? v : 0.f;
        }
      }
      pollp[o] = xbuf + (size_t)b * H3 + (size_t)g * Hd + k0 + (lane < kn[o] ? lane : 0);
    }
    // where this lane's partial sum goes: FOLD leaves pv(2 l) in lane l and pv(2 l + 1) in lane 32 + l
    const int prow = FOLD ? 2 * (lane & 31) + (lane >> 5) : lane;
    const size_t par = (size_t)B * H3;
#ifdef GRU_PROF
    long long c_a = 0, c_b = 0, c_c = 0;
#endif
    gru_lds_barrier();                                   // B_init (also publishes the zeroed partial sums)
    for (int s = S - 1; s >= 1; --s) {
      const unsigned tag = (unsigned)(S - s);
      GRU_T(t0);
      float pv;
      if constexpr (OW == 1) {
        const float dv = gru4_poll<GRU_POLL_PRE_B>(pollp[0] + (tag & 1) * par, tag, lane < kn[0], status);
        if constexpr (FOLD) pv = gru_matvec_fold<KU>(wf, dv, lrow[wave], lane);
        else pv = gru_matvec<KU, (KU <= 58 ? GRU_NR4 : (GRU_NR4 > 24 ? GRU_NR4 : 24))>(wr[0], dv, lrow[wave], lane);
      } else {
        float dv[2];
        gru4_poll2<GRU_POLL_PRE_B>(pollp[0] + (tag & 1) * par, pollp[1] + (tag & 1) * par, tag, lane < kn[0], lane < kn[1],
                                   status, dv);
        pv = gru_matvec<KU, 64>(wr[0], dv[0], lrow[wave], lane);
        pv += gru_matvec<KU, 64>(wr[OW - 1], dv[1], lrow[wave], lane);
      }
      part[tag & 1][Part::at(prow, wave)] = pv;
      GRU_T(t2);
      GRU_ACC(c_b, t2, t0);                              // (poll + mat-vec together: the poll's end is inside the if constexpr)
      gru_lds_barrier();                                 // B_s
      GRU_T(t3);
      GRU_ACC(c_c, t3, t2);
    }
    gru_lds_barrier();                                   // B_fin: gate(0) is done
#ifdef GRU_PROF
    if (blockIdx.x == 0 && lane == 0)
      printf("gru bwd4 mat-vec wave %d: per step cycles: poll %lld  matvec %lld  barrier wait %lld\n", wave, c_a / S, c_b / S, c_c / S);
#endif
  } else if (wave == NMV + 1) {
    // ---------------- chore wave: inputs of gate(s-1) into bin[(s-1)&1] before B_s; outputs of gate(s+1) to global ----
    const bool factored = dkey != nullptr;
    const float dk_own = factored ? dkey[(size_t)b * Hd + gu] : 0.f, dq_own = factored ? dquery[(size_t)b * Hd + gu] : 0.f;
    auto fetch = [&](int t, float (&val)[6]) {
      const size_t rw = (size_t)t * B + b;
      const float* rs = reserve + rw * 4 * Hd + gu;
      val[0] = factored ? dk_own * wk[t] + dq_own * wq[t] : dout[rw * Hd + gu];      // (wk[t], wq[t]: wave-uniform scalar loads)
      val[1] = rs[0]; val[2] = rs[Hd]; val[3] = rs[2 * Hd]; val[4] = rs[3 * Hd];
      val[5] = t > 0 ? h_all[(rw - B) * Hd + gu] : 0.f;
    };
    auto stage = [&](int t, const float (&val)[6]) {
#pragma unroll
      for (int v = 0; v < 6; ++v) bin[t & 1][v][lane] = val[v];
    };
    constexpr bool wt = SW;                              // the store wave (below) moves the gate gradients out instead
    auto put = [&](size_t rw, float dr, float dz, float dn, float dnr) {
      if (wt) return;
      float* go = dgi + rw * H3 + gu;
      go[0] = dr; go[Hd] = dz; go[2 * Hd] = dn;
      dghn[rw * Hd + gu] = dnr;
    };
    auto flush = [&](int t) {
      const size_t rw = (size_t)t * B + b;
      const float dr = bout[t & 1][0][lane], dz = bout[t & 1][1][lane], dn = bout[t & 1][2][lane], dnr = bout[t & 1][3][lane];
      if (lane_ok) put(rw, dr, dz, dn, dnr);
    };
    // dW_ih | db_ih of this workgroup's units and batch row, accumulated over the steps as the gate gradients pass through
    // on their way to global memory (ih_slab != nullptr, W <= GRU4_WMAX): acc[g][w] += d_g(t) * x[b][w][t].  x is read
    // with wave-uniform (scalar) loads.  The slab row (b, gate row) is reduced over b by gru_reduce_grad_kernel.
    float acc[3][GRU4_WMAX], accb[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int w = 0; w < GRU4_WMAX; ++w) acc[g][w] = 0.f;
    const float* xrow = x + (size_t)b * W * S;           // x[b][w][t] = xrow[w * S + t]
    auto wih_x = [&](int t, float (&xv)[GRU4_WMAX]) {     // the W window values of step t: independent scalar loads, no branches
      if (!ih_slab) return;
#pragma unroll
      for (int w = 0; w < GRU4_WMAX; ++w) xv[w] = xrow[(size_t)(w < W ? w : 0) * S + t];
    };
    auto wih = [&](const float (&xv)[GRU4_WMAX], float dr, float dz, float dn) {
      if (!ih_slab) return;
      accb[0] += dr; accb[1] += dz; accb[2] += dn;
#pragma unroll
      for (int w = 0; w < GRU4_WMAX; ++w) {              // (columns w >= W accumulate a copy of column 0 and are never stored)
        acc[0][w] = fmaf(dr, xv[w], acc[0][w]);
        acc[1][w] = fmaf(dz, xv[w], acc[1][w]);
        acc[2][w] = fmaf(dn, xv[w], acc[2][w]);
      }
    };
    float val[6];
    fetch(S - 1, val);
    stage(S - 1, val);
    if (S >= 2) fetch(S - 2, val);                       // inputs of gate(S-2): staged at the top of step S-1
    gru_lds_barrier();                                   // B_init
    for (int s = S - 1; s >= 1; --s) {
      stage(s - 1, val);                                 // (gate(s+1), the last reader of this parity, finished before B_{s+1})
      float dr = 0.f, dz = 0.f, dn = 0.f, dnr = 0.f;
      const bool have = s + 1 <= S - 1;
      if (have) { dr = bout[(s + 1) & 1][0][lane]; dz = bout[(s + 1) & 1][1][lane]; dn = bout[(s + 1) & 1][2][lane]; dnr = bout[(s + 1) & 1][3][lane]; }
      float xv[GRU4_WMAX];
      if (have) wih_x(s + 1, xv);                        // scalar-cache loads: not in the vector memory pipeline's way
      __builtin_amdgcn_s_sleep(FOLD ? GRU_CHORE_SLEEP_B : GRU_CHORE_SLEEP_B_RL);      // the granule stores of gate(s) go first
      if (s >= 2) fetch(s - 2, val);
      if (have && lane_ok) put((size_t)(s + 1) * B + b, dr, dz, dn, dnr);
      if (have) wih(xv, dr, dz, dn);
      gru_lds_barrier();                                 // B_s
    }
    gru_lds_barrier();                                   // B_fin: gate(0) is done
    float xv[GRU4_WMAX];
    if (S >= 2) { flush(1); wih_x(1, xv); wih(xv, bout[1][0][lane], bout[1][1][lane], bout[1][2][lane]); }
    flush(0);
    wih_x(0, xv);
    wih(xv, bout[0][0][lane], bout[0][1][lane], bout[0][2][lane]);
    if (ih_slab && lane_ok) {
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        float* o = ih_slab + ((size_t)b * H3 + (size_t)g * Hd + gu) * (W + 1);
#pragma unroll
        for (int w = 0; w < GRU4_WMAX; ++w)
          if (w < W) o[w] = acc[g][w];
        o[W] = accb[g];
      }
    }
  } else if (SW && wave == NMV + 2) {
    // ---------------- store wave (SW launches, prog != nullptr: one more wave) ----------------
    // bout[(s+1)&1] -> global memory during step s like the chore wave does otherwise, but WRITE-THROUGH, and from a wave
    // that has no loads in flight: the chore wave waits for its loads at the top of every step and vmcnt cannot tell loads
    // from the stores behind them, so it would sit out every write-through acknowledgement there (measured: 270 -> 313 us
    // per backward).  Here the only waits are counted ones at chunk boundaries: stores complete in issue order, so with at
    // most the last two steps' 8 stores in flight every row of a step >= s + 3 is in memory.
    auto put = [&](int t) {
      const size_t rw = (size_t)t * B + b;
      const float dr = bout[t & 1][0][lane], dz = bout[t & 1][1][lane], dn = bout[t & 1][2][lane], dnr = bout[t & 1][3][lane];
      if (lane_ok) {
        float* go = dgi + rw * H3 + gu;
#if GRU_SW_MODE == 0
        __hip_atomic_store(go, dr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(go + Hd, dz, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(go + 2 * Hd, dn, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(dghn + rw * Hd + gu, dnr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#elif GRU_SW_MODE == 2      // timing probes: plain / non-temporal stores (not visible to the reader in time: results wrong)
        go[0] = dr; go[Hd] = dz; go[2 * Hd] = dn; dghn[rw * Hd + gu] = dnr;
#elif GRU_SW_MODE == 3
        __builtin_nontemporal_store(dr, go); __builtin_nontemporal_store(dz, go + Hd);
        __builtin_nontemporal_store(dn, go + 2 * Hd); __builtin_nontemporal_store(dnr, dghn + rw * Hd + gu);
#else
        if (dr + dz + dn + dnr == 1.2345e-30f) go[0] = dr;                  // mode 1: no stores at all
#endif
      }
    };
    auto count = [&](int t) {                            // chunk t / prog_ts is complete for this workgroup
      if (lane == 0) __hip_atomic_fetch_add(prog + t / prog_ts, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    gru_lds_barrier();                                   // B_init
    for (int s = S - 1; s >= 1; --s) {
      __builtin_amdgcn_s_sleep(GRU_SW_SLEEP);            // let the granule stores of gate(s) go first
      if (s + 1 <= S - 1) put(s + 1);
      if (s + 3 <= S - 1 && (s + 3) % prog_ts == 0) {
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        count(s + 3);
      }
      gru_lds_barrier();                                 // B_s
    }
    gru_lds_barrier();                                   // B_fin: gate(0) is done
    if (S >= 2) put(1);
    put(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    for (int t = (S - 1 < 3 ? S - 1 : 3); t >= 0; --t)
      if (t % prog_ts == 0) count(t);
  } else {
    // ---------------- gate wave ----------------
    float dhz = 0.f;
    gru_u64* pub = xbuf + (size_t)b * H3 + gu;           // parity 0, gate r; gates z / n are Hd / 2 Hd granules further
    const size_t par = (size_t)B * H3;
#ifdef GRU_PROF
    long long c_a = 0, c_b = 0, c_c = 0;
#endif
    gru_lds_barrier();                                   // B_init
    for (int s = S - 1; s >= 0; --s) {
      const unsigned tag = (unsigned)(S - s);
      GRU_T(t1);
      const float dh = Part::sum(part[(tag + 1) & 1], lane, bin[s & 1][0][lane] + dhz);      // partials of the step after this one
      const float r = bin[s & 1][1][lane], z = bin[s & 1][2][lane], n = bin[s & 1][3][lane], ghn = bin[s & 1][4][lane];
      const float hprev = s > 0 ? bin[s & 1][5][lane] : 0.f;
      const float dn = dh * (1.f - z) * (1.f - n * n);
      const float dz = dh * (hprev - n) * z * (1.f - z);
      const float dr = dn * ghn * r * (1.f - r);
      const float dnr = dn * r;
      dhz = dh * z;
      if (s > 0 && lane_ok) {
        gru_u64* xb = pub + (tag & 1) * par;
        gru_publish_x(xb, tag, dr, fast);
        gru_publish_x(xb + Hd, tag, dz, fast);
        gru_publish_x(xb + 2 * Hd, tag, dnr, fast);
      }
      gru4_after_publish(pub);
      GRU_T(t2);
      GRU_ACC(c_b, t2, t1);
      bout[s & 1][0][lane] = dr;
      bout[s & 1][1][lane] = dz;
      bout[s & 1][2][lane] = dn;
      bout[s & 1][3][lane] = dnr;
      GRU_T(t3);
      GRU_ACC(c_c, t3, t2);
      if (s > 0) gru_lds_barrier();                      // B_s
      GRU_T(t4);
      GRU_ACC(c_a, t4, t3);
    }
    gru_lds_barrier();                                   // B_fin
#ifdef GRU_PROF
    if (blockIdx.x == 0 && lane == 0)
      printf("gru bwd4 gate wave: per step cycles: barrier wait %lld  gate phase to publish %lld  stash %lld\n", c_a / S, c_b / S, c_c / S);
#endif
  }
}
