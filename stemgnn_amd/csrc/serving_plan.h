// The launch geometry of the per-arrival serving entries -- stemgnn_live_push / stemgnn_ring_gather (live.hip),
// stemgnn_aci_update (aci.hip), stemgnn_anomaly_update (anomaly.hip) -- as host functions of the shape alone: every tile width,
// thread class, cap and threshold of the three files is defined HERE, once; the launchers take their grids, forms and spans from
// these functions, the kernels their constants, and stemgnn_serving_plan (the end of anomaly.hip) hands the same answers to the
// tests (tests/test_serving_cases.py), so what it reports is what runs.  Alignment enters as a flag: no function reads a buffer.
#pragma once
#include <stdint.h>

#include "conformal_args.h"
#include "sg_host.h"

// ---- live.hip ---------------------------------------------------------------------------------------------------------------
constexpr int LV_PUSH_THREADS = 64;
constexpr int LV_GATHER_MID_N = 256, LV_GATHER_WIDE_N = 1024;     // the N from which a row is copied by 128 / by 256 threads

struct LvPushPlan {
  unsigned blocks;
  int threads, k0;                                // k0: the first of the K rows that is stored (K > C: the rows before it only fill)
};
static inline bool lv_push_plan(int K, int N, int C, LvPushPlan* p) {
  if (K <= 0 || N <= 0 || C <= 0) return false;
  if ((long long)C * N >= (1ll << 31)) return false;
  p->blocks = (unsigned)sg_ceil_div(N, LV_PUSH_THREADS);
  p->threads = LV_PUSH_THREADS;
  p->k0 = K > C ? K - C : 0;
  return true;
}

struct LvGatherPlan {
  int threads, vec, trips;                        // vec: 4 = float4 copies, 1 = scalar; trips of thread 0 through the copy loop
};
static inline bool lv_gather_plan(int C, int N, int B, int L, bool aligned, LvGatherPlan* p) {
  if (C <= 0 || N <= 0 || B <= 0 || L <= 0 || L > C || B > 65535) return false;
  if ((long long)C * N >= (1ll << 31)) return false;
  p->threads = N >= LV_GATHER_WIDE_N ? 256 : (N >= LV_GATHER_MID_N ? 128 : 64);
  p->vec = ((N & 3) == 0 && aligned) ? 4 : 1;
  p->trips = sg_ceil_div(N / p->vec, p->threads);
  return true;
}

// ---- aci.hip ----------------------------------------------------------------------------------------------------------------
constexpr int ACI_THREADS = 1024;
constexpr int ACI_WAVES = ACI_THREADS / 64;
constexpr int ACI_TILE = 32;                  // columns per workgroup (column form)
constexpr int ACI_KEEP = 16;                  // loads of the window a thread keeps in registers over the passes (stream form)

struct AciPlan {
  int form;                                   // 0 = columns, 1 = stream
  unsigned gx, gy;
  int vec;                                    // stream: 4 or 1; columns: 0
  CfGrouping gr;
  int wd_last, keep;                          // columns: the last tile's width; stream: the window stays in registers
  // [0] the fullest tile (tile 0), [1] the last tile; stream: both the one workgroup shape
  int step[2];                                // rows a workgroup covers per trip (stream: elements, threads * VEC)
  int pass_trips[2];                          // trips of the first row lane (thread) through one histogram pass
  int origin_trips[2];                        // ... through the origin-scoring loop
};
// (shapes: M > 0 and cf_shapes_ok, checked by the callers)
static inline void aci_plan(int H, int N, int P, int M, int per_step, int per_node, bool aligned, AciPlan* p) {
  p->gr = cf_grouping(per_step, per_node, H, N);
  p->gy = (unsigned)P;
  if (per_node) {
    const int tiles = sg_ceil_div(p->gr.Cc, ACI_TILE);
    const long long R = (long long)M * p->gr.Hr;
    p->form = 0, p->gx = (unsigned)tiles, p->vec = 0, p->keep = 0;
    p->wd_last = p->gr.Cc - (tiles - 1) * ACI_TILE;
    const int wd[2] = {p->gr.Cc < ACI_TILE ? p->gr.Cc : ACI_TILE, p->wd_last};
    for (int i = 0; i < 2; ++i) {
      p->step[i] = ACI_WAVES * (64 / wd[i]);
      p->pass_trips[i] = sg_ceil_div(R, p->step[i]);
      p->origin_trips[i] = sg_ceil_div(p->gr.Hr, p->step[i]);
    }
  } else {
    const long long total = (long long)M * p->gr.L;
    p->form = 1, p->gx = (unsigned)p->gr.G, p->vec = ((N & 3) == 0 && aligned) ? 4 : 1, p->wd_last = 0;
    p->keep = total <= (long long)ACI_KEEP * ACI_THREADS * p->vec;
    for (int i = 0; i < 2; ++i) {
      p->step[i] = ACI_THREADS * p->vec;
      p->pass_trips[i] = sg_ceil_div(total, p->step[i]);
      p->origin_trips[i] = sg_ceil_div(p->gr.L, p->step[i]);
    }
  }
}

// ---- anomaly.hip ------------------------------------------------------------------------------------------------------------
constexpr int AN_THREADS = 1024;
constexpr int AN_TILE = 32;                       // nodes per workgroup (column form)
constexpr int AN_ROWS = AN_THREADS / AN_TILE;     // row lanes per node
constexpr int AN_QC = 4;                          // queries per node that share one pass over the population
constexpr int AN_BATCH = 4096;                    // queries sorted at a time (pooled form)
constexpr int AN_COL_BLOCKS = 192;                // workgroups the column form of a long horizon aims at
constexpr int AN_MAX_RPARTS = 16;
constexpr int AN_PART_KEYS = 8192;                // population keys per workgroup the pooled form aims at
constexpr int AN_MAX_PARTS = 64;

struct AnPlan {
  int form;                                       // 0 = columns, 2 = pooled
  unsigned gx, gy, gz;
  int vec, launches;                              // vec: pooled 4 or 1; columns 0
  int hspan, spans, rparts, tiles, pop_trips;     // columns; pop_trips: trips of row lane 0 of part 0 over the population's rows
  long long want, most;                           // columns with spans > 1: rparts before its clamps, and the parts that still get rows
  int parts, batches, nb_last, p2_last, L, G;     // pooled
};
// false: a grid the launch cannot have (spans > 65535).  (shapes: checked by the callers)
static inline bool an_plan(int H, int N, int M, int per_step, int per_node, bool aligned, AnPlan* p) {
  *p = AnPlan{};
  if (per_node) {
    p->hspan = H <= AN_QC ? H : (per_step ? 1 : AN_QC);
    p->spans = (H + p->hspan - 1) / p->hspan;
    p->tiles = sg_ceil_div(N, AN_TILE);
    if (p->spans > 65535) return false;
    const long long rows = per_step ? M : (long long)M * H;
    p->rparts = 1;
    if (p->spans > 1) {                           // a long horizon: enough workgroups, none without rows
      p->most = (rows + AN_ROWS - 1) / AN_ROWS;
      p->want = AN_COL_BLOCKS / ((long long)p->tiles * p->spans);
      p->rparts = (int)(p->want < 1 ? 1 : (p->want > AN_MAX_RPARTS ? AN_MAX_RPARTS : p->want));
      if (p->rparts > p->most) p->rparts = (int)p->most;
    }
    p->form = 0, p->gx = (unsigned)p->tiles, p->gy = (unsigned)p->spans, p->gz = (unsigned)p->rparts;
    p->launches = p->spans > 1 ? 2 : 1;
    p->pop_trips = sg_ceil_div(rows, (long long)AN_ROWS * p->rparts);
    return true;
  }
  const CfGrouping gr = cf_grouping(per_step, 0, H, N);
  p->L = gr.L, p->G = gr.G;
  p->parts = sg_ceil_div((long long)M * gr.L, AN_PART_KEYS);
  if (p->parts > AN_MAX_PARTS) p->parts = AN_MAX_PARTS;
  p->form = 2, p->gx = (unsigned)gr.G, p->gy = (unsigned)p->parts, p->gz = 1u;
  p->vec = ((N & 3) == 0 && aligned) ? 4 : 1;
  p->launches = 2;
  p->batches = sg_ceil_div(gr.L, AN_BATCH);
  p->nb_last = gr.L - (p->batches - 1) * AN_BATCH;
  p->p2_last = 1;
  while (p->p2_last < p->nb_last) p->p2_last <<= 1;
  return true;
}
