// The launch geometry of the batch side of the conformal family -- stemgnn_conformal_fit / _apply (conformal.hip, conformal_fit.h),
// stemgnn_seasonal_fit / _apply (seasonal.hip) and the column kernel behind stemgnn_quantile_finish / _store, stemgnn_seasonal_apply
// with rearrange and stemgnn_quantile_store_seasonal (quantile_column.h) -- as host functions of the shape and the compute-unit
// count alone: every tile width, thread count, LDS budget, cap and threshold of these files is defined HERE, once; the launchers
// take their grids, forms and chunk sizes from these functions, the kernels their constants, and stemgnn_calibration_plan (the end
// of seasonal.hip) hands the same answers to the tests (tests/test_calibration_cases.py), so what it reports is what runs.
// Alignment enters as a flag: no function reads a buffer.  The counterpart of serving_plan.h.
#pragma once
#include <stdint.h>

#include "conformal_args.h"
#include "sg_host.h"

// ---- conformal_fit.h: the histogram launches of the fit and its pick ----------------------------------------------------------
constexpr int CF_TILE = 32;                 // columns per workgroup (column form)
constexpr int CF_PITCH = CF_TILE + 1;       // LDS row pitch in words
constexpr int CF_COPIES = 16;               // histogram copies per workgroup (stream form)
constexpr int CF_THREADS = 256;
constexpr int CF_WAVES = CF_THREADS / 64;
constexpr int CF_BLOCKS_PER_CU = 4;         // histogram workgroups the fit aims at, per compute unit
constexpr int CF_CHUNK_MIN_ROWS = 64;       // column form: no chunk shorter than this many rows ...
constexpr int CF_CHUNK_MIN_ELEMS = 4 * CF_THREADS;   // ... stream form: than this many elements
constexpr int CF_MAX_CHUNKS = 65535;        // grid.y of the column form

enum { CF_BOUND_WANTED = 0, CF_BOUND_SIZE = 1, CF_BOUND_GRID = 2 };   // what set the chunk count

struct CfFitPlan {
  int form;                                 // 0 = columns, 1 = stream
  int KP, G;                                // tables (buckets * P), groups of a table
  long long PG;
  int blocks_wanted;
  int tiles, wd_last, rpw_full, rpw_last;   // columns: tiles, columns of the last one, rows a wave covers per trip on tile 0 / the last
  int rows;                                 // what the chunk formula divides: rows (columns) or elements (stream) a workgroup row walks
  int want, by_size;                        // the chunk count each bound asks for: blocks wanted / (tiles * KP or KP * G), rows / 64 or elements / 1024
  int chunks, per_chunk, launched, bound;   // the count chosen, rows (elements) per chunk, chunks that get any, CF_BOUND_*
  int trips;                                // of the first row lane of tile 0 (stream: thread 0) through chunk 0
  unsigned pick_blocks;
  int pick_idle;                            // waves of the last pick workgroup without a (table, group)
};
// `walked` = the windows a workgroup walks (count, or the virtual rows of the longest bucket: ss_fit_walk).  (shapes: checked by
// the callers, KP * G < 2^29)
static inline void cf_fit_plan(long long walked, int KP, const CfGrouping& gr, bool per_node, int cus, CfFitPlan* p) {
  *p = CfFitPlan{};
  p->KP = KP, p->G = (int)gr.groups(), p->PG = (long long)KP * p->G;
  p->blocks_wanted = CF_BLOCKS_PER_CU * cus;
  int step;
  if (per_node) {
    const int C = gr.Cc;
    p->form = 0, p->rows = (int)(walked * gr.Hr);
    p->tiles = sg_ceil_div(C, CF_TILE);
    p->wd_last = C - (p->tiles - 1) * CF_TILE;
    p->rpw_full = 64 / (C < CF_TILE ? C : CF_TILE), p->rpw_last = 64 / p->wd_last;
    p->want = sg_ceil_div(p->blocks_wanted, (long long)p->tiles * KP);
    p->by_size = sg_ceil_div(p->rows, CF_CHUNK_MIN_ROWS);
    step = CF_WAVES * p->rpw_full;
  } else {
    p->form = 1, p->rows = (int)(walked * gr.L);
    p->want = sg_ceil_div(p->blocks_wanted, p->PG);
    p->by_size = sg_ceil_div(p->rows, CF_CHUNK_MIN_ELEMS);
    step = CF_THREADS;
  }
  int chunks = p->want;
  p->bound = CF_BOUND_WANTED;
  if (p->by_size < chunks) chunks = p->by_size, p->bound = CF_BOUND_SIZE;
  if (per_node && CF_MAX_CHUNKS < chunks) chunks = CF_MAX_CHUNKS, p->bound = CF_BOUND_GRID;
  p->chunks = chunks < 1 ? 1 : chunks;
  p->per_chunk = sg_ceil_div(p->rows, p->chunks);
  p->launched = sg_ceil_div(p->rows, p->per_chunk);
  p->trips = sg_ceil_div(p->rows < p->per_chunk ? p->rows : p->per_chunk, step);
  p->pick_blocks = (unsigned)sg_ceil_div(p->PG, CF_WAVES);
  p->pick_idle = (int)((long long)p->pick_blocks * CF_WAVES - p->PG);
}

// ---- seasonal.hip: which walk the seasonal fit takes ------------------------------------------------------------------------------
enum { SS_WALK_DIRECT = 0, SS_WALK_ORIGINS = 1, SS_WALK_ONE_BUCKET = 2, SS_WALK_LONG = 3 };   // DIRECT, or why the fit skips instead

struct SsFitWalk {
  int direct, why;                          // why: SS_WALK_*
  int runs;                                 // count / period + 2 covers every run that meets [0, count)
  long long walk;                           // virtual rows of the longest bucket: runs * ceil(period / K)
  long long walked;                         // what goes into cf_fit_plan: walk (DIRECT) or count
};
// consecutive origins: a bucket's rows are enumerated (DIRECT) when that walks fewer rows than skipping through all of them does
// (runs * the longest bucket against count; measured in DESIGN 5n), otherwise -- and always for an origins tensor -- skipped
static inline SsFitWalk ss_fit_walk(long count, long long period, int K, bool has_origins) {
  SsFitWalk w;
  w.runs = (int)(count / period) + 2;
  w.walk = (long long)w.runs * ((period + K - 1) / K);
  w.why = has_origins ? SS_WALK_ORIGINS : (K < 2 ? SS_WALK_ONE_BUCKET : (2 * w.walk > (long long)count ? SS_WALK_LONG : SS_WALK_DIRECT));
  w.direct = w.why == SS_WALK_DIRECT;
  w.walked = w.direct ? w.walk : (long long)count;
  return w;
}

// ---- conformal.hip / seasonal.hip: the streaming applies --------------------------------------------------------------------------
constexpr int SS_THREADS = 256;
constexpr int SS_WAVES = SS_THREADS / 64;
constexpr int CF_APPLY_BLOCKS_PER_CU = 8;   // the cap of both applies' grids, per compute unit

struct CfApplyPlan {
  int vec;                                  // 4 = float4, 1 = scalar
  unsigned blocks;
  long long needed, cap;                    // workgroups that give every item a thread (segment a wave) of its own; the cap
  int capped;
  long long trips;                          // of thread 0 over the items (seasonal: of wave 0 over the segments)
  int items, lane_trips;                    // seasonal: Q * N / VEC items of a segment, trips of lane 0 over them
};
// one thread per VEC elements of [count, Q, H, N], striding
static inline void cf_apply_plan(long count, int Q, int H, int N, bool aligned, int cus, CfApplyPlan* p) {
  *p = CfApplyPlan{};
  const size_t total = (size_t)count * Q * H * N;
  p->vec = ((N & 3) == 0 && aligned) ? 4 : 1;
  const size_t items = total / (size_t)p->vec;
  p->cap = (long long)cus * CF_APPLY_BLOCKS_PER_CU;
  p->needed = (long long)((items + CF_THREADS - 1) / CF_THREADS);
  p->capped = p->needed > p->cap;
  const long long b = p->capped ? p->cap : p->needed;
  p->blocks = (unsigned)(b < 1 ? 1 : b);
  p->trips = (long long)((items + (size_t)p->blocks * CF_THREADS - 1) / ((size_t)p->blocks * CF_THREADS));
}
// one wave per (window, step) segment, striding; its lanes over the segment's Q runs of N / VEC items
static inline void ss_apply_plan(long count, int Q, int H, int N, bool aligned, int cus, CfApplyPlan* p) {
  *p = CfApplyPlan{};
  const long long segments = (long long)count * H;
  p->vec = ((N & 3) == 0 && aligned) ? 4 : 1;
  p->cap = (long long)cus * CF_APPLY_BLOCKS_PER_CU;
  p->needed = (segments + SS_WAVES - 1) / SS_WAVES;
  p->capped = p->needed > p->cap;
  const long long b = p->capped ? p->cap : p->needed;
  p->blocks = (unsigned)(b < 1 ? 1 : b);
  p->trips = (segments + (long long)p->blocks * SS_WAVES - 1) / ((long long)p->blocks * SS_WAVES);
  p->items = Q * (N / p->vec);
  p->lane_trips = sg_ceil_div(p->items, 64);
}

// ---- quantile_column.h: the column kernel ---------------------------------------------------------------------------------------
constexpr int QC_THREADS = 256;             // the most; fewer (a multiple of 64) when Q is large: see qc_plan
constexpr int QC_CHUNK = 4;                 // rows whose global loads are in flight together
constexpr int QC_LDS_BYTES = 32 * 1024;     // per workgroup, both planes
constexpr int QC_VEC_MAX_Q = 16;
constexpr int QC_BLOCKS_PER_CU = 16;        // the cap of the grid, per compute unit

struct QcPlan {
  int vec, T, planes;
  size_t lds;                               // <= 32 KB: Q <= 32 (VEC 1), Q <= 16 (VEC 4)
  int per;                                  // column groups (of VEC columns) per window
  int cpb, wpb, idle;                       // a workgroup = wpb windows x cpb column groups; T - cpb * wpb threads have neither
  int col_blocks, cols_last;                // cols_last: columns (not groups) of the last column block
  int win_blocks, capped;                   // capped: the cap (16 CUs / col_blocks), not the windows, set win_blocks
  long long win_trips;                      // of a workgroup's first window lane over the windows it strides through
  unsigned gx, gy;
  long long target_trips;                   // store: of target workgroup 0 over the batch's windows
};
// the vector form needs N % 4 == 0, Q <= 16 and both buffers 16-byte aligned
static inline bool qc_vec_shape_ok(int N, int Q) { return (N & 3) == 0 && Q <= QC_VEC_MAX_Q; }
// the batch's target is copied by float4 when H * N % 4 == 0 and both of its buffers are 16-byte aligned
static inline bool qc_tvec_shape_ok(int HN) { return (HN & 3) == 0; }

static inline void qc_plan(long count, int Q, int HN, bool rearrange, bool vec, bool store, int cus, QcPlan* p) {
  *p = QcPlan{};
  p->vec = vec ? 4 : 1, p->planes = rearrange ? 2 : 1;
  int T = QC_THREADS;
  while (T > 64 && (size_t)T * Q * p->vec * 4 * p->planes > (size_t)QC_LDS_BYTES) T -= 64;
  p->T = T;
  p->lds = (size_t)T * Q * p->vec * 4 * p->planes;
  p->per = HN / p->vec;
  p->cpb = p->per < T ? p->per : T;
  p->wpb = T / p->cpb;
  p->idle = T - p->cpb * p->wpb;
  p->col_blocks = sg_ceil_div(p->per, p->cpb);
  p->cols_last = (p->per - (p->col_blocks - 1) * p->cpb) * p->vec;
  const long long wins = ((long long)count + p->wpb - 1) / p->wpb;
  const long long cap = (long long)cus * QC_BLOCKS_PER_CU / p->col_blocks;
  p->capped = cap < wins;
  const long long wb = wins < cap ? wins : cap;
  p->win_blocks = (int)(wb < 1 ? 1 : wb);
  const long long stride = (long long)p->win_blocks * p->wpb;
  p->win_trips = ((long long)count + stride - 1) / stride;
  p->gx = (unsigned)p->col_blocks * (unsigned)p->win_blocks, p->gy = store ? 2u : 1u;
  p->target_trips = store ? ((long long)count + p->gx - 1) / p->gx : 0;
}
