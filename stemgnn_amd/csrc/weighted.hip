// Weighted scenario sets: bands, scores, event counts and a further reduction of K kept paths that carry integer
// multiplicities (include/stemgnn_hip.h: stemgnn_weighted_bands / _scores / _events, stemgnn_scenario_reduce_weighted;
// DESIGN.md section 5t).  Member k of origin c stands mult[c, k] times in an ensemble of W paths; every entry computes what
// its unweighted parent (scenario.hip, ensemble.hip, events.hip, reduce.hip) computes on that replicated ensemble, from the K
// members alone.
//
// Every workgroup first brings its origin's K multiplicities into LDS and decides, the same way in every kernel, whether the
// origin is PRESENT (none negative, their sum W).  A member of multiplicity 0 is never loaded.
// bands:   one workgroup per (origin, tile of C columns of the H * N), the tile of K x C values in LDS (C = 64 .. 8, <= 32 KB).
//          Thread (g, c) owns members g, g + G, .. of column c: `before` = the multiplicities of the values ahead of its own in
//          the order of sc_less (-0 == +0, NaN last, the member index breaking ties); the member answers every rank in
//          (before, before + w].  The answers meet in an LDS tile [Q][C] that the workgroup stores (NaN for an absent origin).
// events:  the kernel of path_events.h (ev_kernel<true>): `+= w` for `+= 1`; an absent origin's tile is -1.
// scores:  the three launches of ensemble.hip on the live members (those of positive multiplicity, compacted in index order):
//          the pair tiles of the energy score weigh a pair distance by w w' and a target distance by w; the marginal launch,
//          one workgroup per row (c, h) walking the row's node tiles in order, weighs |x - y| and x by w, |x - x'| by w w'
//          and counts ranks in multiplicities; the row's ranks meet in an LDS histogram where W + 1 <= 4096 and go to `hist`
//          with one 64-bit integer add per non-empty bin (beyond: one add per element); the finish, one workgroup per step and one for the
//          overall statistics, adds the partials in index order.  An absent origin contributes zeros and
//          is counted in slot 6.
// reduce:  the pick of forward_select.h (fs_pick, WEIGHTED): z_u = sum_k p_k min(m_k, D[k, u]), the product and the sum rounded
//          separately; a member of multiplicity 0 is no candidate and its row and column of D are not read.
// No floating-point atomics, no allocation, no memset, no host synchronisation: the same bits on every run, origin by origin.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "forward_select.h"
#include "path_events.h"
#include "scenario_draw.h"
#include "scenario_math.h"
#include "sg_host.h"

namespace {

constexpr int WT_THREADS = 256;
constexpr int WT_MAX_K = 256;               // bands, scores, events: members of a set
constexpr int WT_MAX_Q = 32;
constexpr int WT_MAX_W = 1 << 24;           // w w' and W^2 are exact in fp64
constexpr int WT_TILE_BYTES = 32 * 1024;    // bands, marginal: the LDS tile
constexpr int WT_PT = 32;                   // energy: members per panel
constexpr int WT_NC = 64;                   // energy: nodes per chunk
constexpr int WT_LD = WT_NC + 1;            // energy: doubles between panel rows
constexpr int WT_FIN_THREADS = 1024;
constexpr int WT_OUT_K = 7;
constexpr int WT_HIST_BINS = 4096;          // marginal: a row's ranks meet in LDS where W + 1 bins are within 16 KB

// wt_present (scenario_math.h), and the members of positive multiplicity compacted in index order: idx[i] the member, wl[i]
// its multiplicity, i < *n.  K <= blockDim.x.  Two barriers.
__device__ inline bool wt_live(const int* mult, int K, int W, int* wm, int* idx, int* wl, int* n) {
  const int t = threadIdx.x;
  const bool ok = wt_present(mult, K, W, wm);
  int pos = 0, all = 0;
  for (int k = 0; k < K; ++k) {
    const int on = wm[k] > 0 ? 1 : 0;
    all += on;
    pos += k < t ? on : 0;
  }
  if (ok && t < K && wm[t] > 0) {
    idx[pos] = t;
    wl[pos] = wm[t];
  }
  __syncthreads();
  *n = ok ? all : 0;
  return ok;
}

template <int VEC>
__device__ inline void wt_load(const float* p, float* v) {
  if constexpr (VEC == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int VEC>
__device__ inline void wt_store(float* p, const float* v) {
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    *p = v[0];
  }
}

// ---- bands ---------------------------------------------------------------------------------------------------------------------
struct WtBandArgs {
  const float* paths;                       // [count, K, HN]
  const int* mult;                          // [count, K]
  float* bands;                             // [count, Q, HN]
  int K, Q, HN, C, tiles, W;
  int rank[WT_MAX_Q];                       // 1-based
};

template <int VEC>
__global__ __launch_bounds__(WT_THREADS) void wt_bands_kernel(const WtBandArgs a) {
  extern __shared__ float4 wt_lds4[];
  const int K = a.K, Q = a.Q, C = a.C, t = threadIdx.x;
  float* tile = reinterpret_cast<float*>(wt_lds4);              // [K][C]
  float* res = tile + K * C;                                    // [Q][C]
  int* wm = reinterpret_cast<int*>(res + Q * C);                // [K]
  const size_t b = blockIdx.x / (unsigned)a.tiles;
  const int c0 = (int)(blockIdx.x - b * (unsigned)a.tiles) * C;
  const int live = min(C, a.HN - c0);                           // columns of this tile (a multiple of VEC)
  const bool ok = wt_present(a.mult + b * K, K, a.W, wm);
  const int per = C / VEC;
  if (ok) {
    const float* src = a.paths + b * K * (size_t)a.HN + c0;
    for (int e = t; e < K * per; e += WT_THREADS) {
      const int i = e / per, c = (e - i * per) * VEC;
      if (wm[i] > 0 && c < live) wt_load<VEC>(src + (size_t)i * a.HN + c, tile + i * C + c);
    }
  } else {
    for (int e = t; e < Q * C; e += WT_THREADS) res[e] = __uint_as_float(0x7fc00000u);
  }
  __syncthreads();
  if (ok) {
    const int G = WT_THREADS / C, g = t / C, c = t - g * C;
    if (c < live) {
      for (int i = g; i < K; i += G) {
        const int wi = wm[i];
        if (wi <= 0) continue;
        const float v = tile[i * C + c];
        int before = 0;
        for (int j = 0; j < K; ++j) {
          const int wj = wm[j];
          if (wj <= 0) continue;                                // (uniform over the workgroup)
          const float w = tile[j * C + c];
          before += (sc_less(w, v) || (!sc_less(v, w) && j < i)) ? wj : 0;
        }
        for (int q = 0; q < Q; ++q) {
          const int r = a.rank[q];
          if (r > before && r <= before + wi) res[q * C + c] = v;
        }
      }
    }
  }
  __syncthreads();
  float* dst = a.bands + b * Q * (size_t)a.HN + c0;
  for (int e = t; e < Q * per; e += WT_THREADS) {
    const int q = e / per, c = (e - q * per) * VEC;
    if (c < live) wt_store<VEC>(dst + (size_t)q * a.HN + c, res + q * C + c);
  }
}

// ---- scores --------------------------------------------------------------------------------------------------------------------
struct WtScoreArgs {
  const float* target;                      // [count, H, N]
  const float* paths;                       // [count, K, H, N]
  const int* mult;                          // [count, K]
  const double* mul;                        // [N] or NULL
  const double* add;
  // partials, step-major: [5][H][count]: sum w |x - y|, pair sum, se, var, valid elements of a row;
  // [2][H][count][pairs]: pair sum, sum w ||x - y||; then [H][count]: the row has a node; then [count]: the origin is absent
  double* mpart;
  double* epart;
  double* out;
  unsigned long long* hist;                 // [H][W + 1]
  long long rows, count;                    // rows = count * H
  int K, H, N, C, tn, nt, pairs, fair, W, lds_hist;
};

template <bool MASKED>
__global__ __launch_bounds__(WT_THREADS) void wt_energy_kernel(const WtScoreArgs a) {
  __shared__ double pa[WT_PT * WT_LD], pb_own[WT_PT * WT_LD], ys[WT_NC], red[WT_THREADS / 64];
  __shared__ int wm[WT_MAX_K], idx[WT_MAX_K], wl[WT_MAX_K];
  const int t = threadIdx.x, K = a.K, N = a.N;
  {                                                             // hist = 0 ahead of the marginal launch
    const size_t bins = (size_t)a.H * ((size_t)a.W + 1);
    for (size_t i = (size_t)blockIdx.x * WT_THREADS + t; i < bins; i += (size_t)gridDim.x * WT_THREADS) a.hist[i] = 0ull;
  }
  const size_t row = blockIdx.x / (unsigned)a.pairs;
  int rem = (int)(blockIdx.x - row * (unsigned)a.pairs), I = 0;
  while (rem >= a.nt - I) {
    rem -= a.nt - I;
    ++I;
  }
  const int J = I + rem;
  const bool diag = I == J;
  const double* pb = diag ? pa : pb_own;
  const size_t b = row / (unsigned)a.H;
  const int h = (int)(row - b * (unsigned)a.H);
  int kk;
  const bool ok = wt_live(a.mult + b * K, K, a.W, wm, idx, wl, &kk);
  const size_t HN = (size_t)a.H * N;
  const float* tg = a.target + row * N;
  const float* px = a.paths + (b * K * a.H + h) * (size_t)N;    // member k: + k * HN
  const bool dn = a.mul != nullptr;
  const int ln = t & (WT_NC - 1), lr = t >> 6;                  // the loader's column and first row
  const int ti = t >> 4, tj = t & 15;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, e0 = 0.0, e1 = 0.0;
  int any = 0;
  // the panel rows that hold live members, rounded up to a thread's two; the threads and waves that own none skip the walk
  const int nra = min(WT_PT, (kk - I * WT_PT + 1) & ~1), nrb = diag ? nra : min(WT_PT, (kk - J * WT_PT + 1) & ~1);
  const bool work = 2 * ti < nra && 2 * tj < nrb;
  if (J * WT_PT < kk) {                                         // (J >= I: a tile past the live members adds nothing)
    for (int n0 = 0; n0 < N; n0 += WT_NC) {
      const int n = n0 + ln;
      const bool live = n < N;
      const float y = live ? tg[n] : 0.f;
      const bool valid = live && (!MASKED || y == y);
      const double mu = (dn && live) ? a.mul[n] : 1.0, ad = (dn && live) ? a.add[n] : 0.0;
      any |= valid ? 1 : 0;
      __syncthreads();                                          // the previous chunk has been read
      for (int r = lr; r < nra; r += WT_THREADS / WT_NC) {
        const int si = I * WT_PT + r;
        pa[r * WT_LD + ln] = (valid && si < kk) ? sg_dn(px[(size_t)idx[si] * HN + n], dn, mu, ad) : 0.0;
      }
      if (!diag) {
        for (int r = lr; r < nrb; r += WT_THREADS / WT_NC) {
          const int sj = J * WT_PT + r;
          pb_own[r * WT_LD + ln] = (valid && sj < kk) ? sg_dn(px[(size_t)idx[sj] * HN + n], dn, mu, ad) : 0.0;
        }
      }
      if (t < WT_NC) ys[t] = valid ? sg_dn(y, dn, mu, ad) : 0.0;
      __syncthreads();
      const int lim = min(WT_NC, N - n0);
      const double* ra = pa + (2 * ti) * WT_LD;
      const double* rb = pb + (2 * tj) * WT_LD;
      for (int k = 0; work && k < lim; ++k) {
        const double a0 = ra[k], a1 = ra[WT_LD + k], b0 = rb[k], b1 = rb[WT_LD + k], yk = ys[k];
        double d;
        d = a0 - b0; acc[0][0] = fma(d, d, acc[0][0]);
        d = a0 - b1; acc[0][1] = fma(d, d, acc[0][1]);
        d = a1 - b0; acc[1][0] = fma(d, d, acc[1][0]);
        d = a1 - b1; acc[1][1] = fma(d, d, acc[1][1]);
        d = a0 - yk; e0 = fma(d, d, e0);
        d = a1 - yk; e1 = fma(d, d, e1);
      }
    }
  }
  double p = 0.0, e = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int si = I * WT_PT + 2 * ti + u, sj = J * WT_PT + 2 * tj + v;
      if (si < sj && sj < kk) p += (double)wl[si] * (double)wl[sj] * sqrt(acc[u][v]);
    }
  if (diag && tj == 0) {
    const int si = I * WT_PT + 2 * ti;
    if (si < kk) e += (double)wl[si] * sqrt(e0);
    if (si + 1 < kk) e += (double)wl[si + 1] * sqrt(e1);
  }
  p = sg_block_sum(p, red);
  e = sg_block_sum(e, red);
  const int has = __syncthreads_or(any);
  if (t == 0) {
    const size_t np = (size_t)a.rows * a.pairs, r = (size_t)h * a.count + b;
    const size_t at = r * a.pairs + (blockIdx.x - row * (unsigned)a.pairs);
    a.epart[at] = p;
    a.epart[np + at] = e;
    if (I == 0 && J == 0) {
      a.epart[2 * np + r] = (ok && has) ? 1.0 : 0.0;
      if (h == 0) a.epart[2 * np + (size_t)a.rows + b] = ok ? 0.0 : 1.0;
    }
  }
}

template <bool MASKED>
__global__ __launch_bounds__(WT_THREADS) void wt_marginal_kernel(const WtScoreArgs a) {
  extern __shared__ double wt_lds[];
  __shared__ int wm[WT_MAX_K], idx[WT_MAX_K], wl[WT_MAX_K];
  const int K = a.K, C = a.C, N = a.N, W = a.W, t = threadIdx.x;
  const int G = WT_THREADS / C, g = t / C, c = t - g * C;
  double* tile = wt_lds;                                        // [K][C], the live members first
  double* rd = tile + (size_t)K * C;                            // [2][256]: per-thread sums, [g][c]
  double* rc = rd + 2 * WT_THREADS;                             // [5][64]: per-column results
  int* ri = reinterpret_cast<int*>(rc + 5 * 64);                // [2][256]
  int* lh = ri + 2 * WT_THREADS;                                // [W + 1] where a.lds_hist: the row's ranks
  const size_t row = blockIdx.x;
  const size_t b = row / (unsigned)a.H;
  const int h = (int)(row - b * (unsigned)a.H);
  if (a.lds_hist)
    for (int i = t; i <= W; i += WT_THREADS) lh[i] = 0;
  int kk;
  const bool ok = wt_live(a.mult + b * K, K, W, wm, idx, wl, &kk);   // (its barriers settle lh too)
  const size_t HN = (size_t)a.H * N;
  const bool dn = a.mul != nullptr;
  unsigned long long* hist = a.hist + (size_t)h * ((size_t)W + 1);
  double total = 0.0;                                           // thread t < 5: statistic t over the tiles, in tile order
  for (int tl = 0; tl < a.tn; ++tl) {
    const int n = tl * C + c;
    const bool live = n < N;
    const float y = live ? a.target[row * N + n] : 0.f;
    const bool valid = ok && live && (!MASKED || y == y);
    const double mu = (dn && live) ? a.mul[n] : 1.0, ad = (dn && live) ? a.add[n] : 0.0;
    const double yd = sg_dn(y, dn, mu, ad);
    const float* src = a.paths + (b * K * a.H + h) * (size_t)N + n;
    int lt = 0, eq = 0;
    double sa = 0.0, sx = 0.0;
    __syncthreads();                                            // the previous tile has been read
    for (int i = g; i < kk; i += G) {
      const float x = live ? src[(size_t)idx[i] * HN] : 0.f;
      const double xd = sg_dn(x, dn, mu, ad), w = (double)wl[i];
      tile[i * C + c] = xd;
      lt += x < y ? wl[i] : 0;
      eq += x == y ? wl[i] : 0;
      sa = fma(w, fabs(xd - yd), sa);
      sx = fma(w, xd, sx);
    }
    rd[t] = sa;
    rd[WT_THREADS + t] = sx;
    ri[t] = lt;
    ri[WT_THREADS + t] = eq;
    __syncthreads();
    double A = 0.0, SX = 0.0;
    int LT = 0, EQ = 0;
    for (int k = 0; k < G; ++k) {
      A += rd[k * C + c];
      SX += rd[WT_THREADS + k * C + c];
      LT += ri[k * C + c];
      EQ += ri[WT_THREADS + k * C + c];
    }
    const double mean = SX / (double)W;
    __syncthreads();                                            // rd is written again below
    double sv = 0.0, sp = 0.0;
    for (int i = g; i < kk; i += G) {
      const double xi = tile[i * C + c], wi = (double)wl[i], d = xi - mean;
      sv = fma(wi, d * d, sv);
      double p = 0.0;
      for (int j = 0; j < i; ++j) p = fma((double)wl[j], fabs(xi - tile[j * C + c]), p);
      sp = fma(wi, p, sp);
    }
    rd[t] = sv;
    rd[WT_THREADS + t] = sp;
    __syncthreads();
    if (g == 0) {
      double V = 0.0, P = 0.0;
      for (int k = 0; k < G; ++k) {
        V += rd[k * C + c];
        P += rd[WT_THREADS + k * C + c];
      }
      const double dm = mean - yd;
      rc[0 * 64 + c] = valid ? A : 0.0;
      rc[1 * 64 + c] = valid ? P : 0.0;
      rc[2 * 64 + c] = valid ? dm * dm : 0.0;
      rc[3 * 64 + c] = valid ? V / (double)(W - 1) : 0.0;       // W == 1: 0 / 0
      rc[4 * 64 + c] = valid ? 1.0 : 0.0;
      if (valid && y == y) {                                    // (valid: LT + EQ <= W)
        if (a.lds_hist) atomicAdd(&lh[LT + EQ / 2], 1);
        else atomicAdd(&hist[LT + EQ / 2], 1ull);
      }
    }
    __syncthreads();
    if (t < 5) {
      double s = 0.0;
      for (int k = 0; k < C; ++k) s += rc[t * 64 + k];
      total += s;
    }
  }
  if (t < 5) a.mpart[(size_t)t * a.rows + (size_t)h * a.count + b] = total;
  if (a.lds_hist) {
    __syncthreads();
    for (int i = t; i <= W; i += WT_THREADS)
      if (lh[i]) atomicAdd(&hist[i], (unsigned long long)lh[i]);
  }
}

// workgroup h < H: the statistics of step h; workgroup H: the overall ones, every step's partials added thread by thread
__global__ __launch_bounds__(WT_FIN_THREADS) void wt_finish_kernel(const WtScoreArgs a) {
  __shared__ double red[WT_FIN_THREADS / 64];
  const int t = threadIdx.x, H = a.H, hb = blockIdx.x;
  const long long count = a.count;
  const double W = (double)a.W, D = a.fair ? W * (W - 1.0) : W * W;
  const size_t nm = (size_t)a.rows, np = (size_t)a.rows * a.pairs;
  const int h0 = hb < H ? hb : 0, h1 = hb < H ? hb + 1 : H;
  // sum w |x - y|, pairs, se, var, elements; energy pairs, sum w ||x - y||, rows; absent origins
  double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, v[9];
  for (int h = h0; h < h1; ++h) {
    // a step's partials are one run per statistic: thread t adds the items t, t + 1024, .. (coalesced, independent loads)
    const size_t m0 = (size_t)h * count, e0 = (size_t)h * count * a.pairs;
    for (size_t i = t; i < (size_t)count; i += WT_FIN_THREADS) {
#pragma unroll
      for (int k = 0; k < 5; ++k) s[k] += a.mpart[k * nm + m0 + i];
      s[7] += a.epart[2 * np + m0 + i];
    }
    for (size_t i = t; i < (size_t)count * a.pairs; i += WT_FIN_THREADS) {
      s[5] += a.epart[e0 + i];
      s[6] += a.epart[np + e0 + i];
    }
  }
  for (size_t i = t; i < (size_t)count; i += WT_FIN_THREADS) s[8] += a.epart[2 * np + (size_t)a.rows + i];
#pragma unroll
  for (int k = 0; k < 9; ++k) v[k] = sg_block_sum(s[k], red);
  if (t == 0) {
    double* o = hb < H ? a.out + WT_OUT_K + hb : a.out;         // statistic k of step h: out[7 + k * H + h]
    const size_t ld = hb < H ? (size_t)H : 1;
    o[0 * ld] = (v[0] / W - v[1] / D) / v[4];
    o[1 * ld] = (v[6] / W - v[5] / D) / v[7];
    o[2 * ld] = sqrt(v[2] / v[4]);
    o[3 * ld] = sqrt(v[3] / v[4]);
    o[4 * ld] = v[4];
    o[5 * ld] = v[7];
    o[6 * ld] = v[8];
  }
}

// ---- reduce --------------------------------------------------------------------------------------------------------------------
template <bool IN_LDS>
__global__ __launch_bounds__(1024) void wt_pick_kernel(const FsPickArgs a) {
  fs_pick<true, IN_LDS>(a);
}

bool wt_sizes_ok(long count, int K, int W) { return count > 0 && K > 0 && K <= WT_MAX_K && W >= 1 && W <= WT_MAX_W; }

// the launch shape of the scores at (count, K, H, N); false where the entries answer SG_EINVAL
bool wt_plan(long count, int K, int H, int N, WtScoreArgs* a) {
  if (count <= 0 || K <= 0 || H <= 0 || N <= 0 || K > WT_MAX_K || !sg_fits_int(count)) return false;
  int C = 4;
  while (C < 64 && C < N) C <<= 1;
  while (C > 4 && (size_t)K * C * 8 > (size_t)WT_TILE_BYTES) C >>= 1;
  const int nt = sg_ceil_div(K, WT_PT);
  a->K = K; a->H = H; a->N = N; a->C = C;
  a->tn = sg_ceil_div(N, C);
  a->nt = nt;
  a->pairs = nt * (nt + 1) / 2;
  if (!sg_fits_int((long long)count * H) || !sg_fits_int((long long)H * N) || !sg_fits_int((long long)K * H * N)) return false;
  a->rows = (long long)count * H;
  a->count = count;
  return sg_fits_int(a->rows * a->pairs);
}
}  // namespace

extern "C" int stemgnn_weighted_bands(const float* paths, const int* mult, long count, int K, int H, int N, int W, int Q,
                                      const int* ranks, float* bands, void* stream) {
  if (!paths || !mult || !ranks || !bands || paths == bands) return SG_EINVAL;
  if (!wt_sizes_ok(count, K, W) || H <= 0 || N <= 0 || Q < 1 || Q > WT_MAX_Q) return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)H * N) || !sg_fits_int((long long)K * H * N) ||
      !sg_fits_int((long long)Q * H * N))
    return SG_EINVAL;
  WtBandArgs a = {};
  for (int q = 0; q < Q; ++q) {
    if (ranks[q] < 1 || ranks[q] > W) return SG_EINVAL;
    a.rank[q] = ranks[q];
  }
  a.paths = paths; a.mult = mult; a.bands = bands; a.K = K; a.Q = Q; a.W = W;
  a.HN = H * N;
  int C = 64;                                                   // the widest tile of K rows within the LDS budget, 8 at least
  while (C > 8 && (size_t)K * C * 4 > (size_t)WT_TILE_BYTES) C >>= 1;
  a.C = C;
  a.tiles = sg_ceil_div(a.HN, C);
  if (!sg_fits_int((long long)count * a.tiles)) return SG_EINVAL;
  const size_t lds = ((size_t)K * C + (size_t)Q * C + (size_t)K) * 4;
  const dim3 grid((unsigned)(count * a.tiles));
  const bool vec = N % 4 == 0 && sg_aligned16(paths) && sg_aligned16(bands);
  if (vec)
    hipLaunchKernelGGL(wt_bands_kernel<4>, grid, dim3(WT_THREADS), lds, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(wt_bands_kernel<1>, grid, dim3(WT_THREADS), lds, (hipStream_t)stream, a);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" size_t stemgnn_weighted_scratch_doubles(long count, int K, int H, int N) {
  WtScoreArgs a = {};
  if (!wt_plan(count, K, H, N, &a)) return 0;
  return (size_t)a.rows * (5 + 2 * (size_t)a.pairs + 1) + (size_t)count;
}

extern "C" size_t stemgnn_weighted_out_doubles(int H) { return H > 0 ? (size_t)WT_OUT_K * ((size_t)H + 1) : 0; }

extern "C" int stemgnn_weighted_scores(const float* target, const float* paths, const int* mult, const double* mul,
                                       const double* add, long count, int K, int H, int N, int W, int fair, int masked,
                                       double* scratch, double* out, long long* hist, void* stream) {
  if (!target || !paths || !mult || !scratch || !out || !hist) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  WtScoreArgs a = {};
  if (!wt_plan(count, K, H, N, &a) || W < 1 || W > WT_MAX_W || (fair && W < 2)) return SG_EINVAL;
  if (!sg_fits_int((long long)H * ((long long)W + 1))) return SG_EINVAL;
  a.target = target; a.paths = paths; a.mult = mult; a.mul = mul; a.add = add; a.out = out;
  a.hist = reinterpret_cast<unsigned long long*>(hist);
  a.fair = fair ? 1 : 0;
  a.W = W;
  a.mpart = scratch;
  a.epart = scratch + 5 * (size_t)a.rows;
  a.lds_hist = W + 1 <= WT_HIST_BINS ? 1 : 0;
  hipStream_t st = (hipStream_t)stream;
  const dim3 ge((unsigned)(a.rows * a.pairs)), gm((unsigned)a.rows), b(WT_THREADS);
  const size_t lds = ((size_t)K * a.C + 2 * WT_THREADS + 5 * 64) * 8 + ((size_t)2 * WT_THREADS + (a.lds_hist ? W + 1 : 0)) * 4;
  if (masked) {
    hipLaunchKernelGGL(wt_energy_kernel<true>, ge, b, 0, st, a);
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(wt_marginal_kernel<true>, gm, b, lds, st, a);
  } else {
    hipLaunchKernelGGL(wt_energy_kernel<false>, ge, b, 0, st, a);
    SG_TRY(hipGetLastError());
    hipLaunchKernelGGL(wt_marginal_kernel<false>, gm, b, lds, st, a);
  }
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(wt_finish_kernel, dim3((unsigned)H + 1), dim3(WT_FIN_THREADS), 0, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}

extern "C" int stemgnn_weighted_events(const float* paths, const int* mult, const double* thr, const double* mul,
                                       const double* add, long count, int K, int H, int M, int W, int above, int min_run,
                                       int* counts, void* stream) {
  if (!paths || !mult || !thr || !counts) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  if (!wt_sizes_ok(count, K, W) || H <= 0 || M <= 0) return SG_EINVAL;
  EvArgs a = {};
  a.paths = paths; a.mult = mult; a.thr = thr; a.mul = mul; a.add = add; a.counts = counts;
  a.S = K; a.H = H; a.M = M; a.above = above; a.min_run = min_run; a.W = W;
  return ev_launch<true>(a, count, (hipStream_t)stream);
}

extern "C" int stemgnn_scenario_reduce_weighted(const double* D, const int* mult_in, long count, int S, int K, int W,
                                                int* selected, int* counts, int* assign, double* cost, void* stream) {
  if (!D || !mult_in || !selected || !counts || !assign || !cost) return SG_EINVAL;
  if (count <= 0 || S <= 0 || S > FS_MAX_S || K < 1 || K > S || W < 1 || W > WT_MAX_W) return SG_EINVAL;
  if (!sg_fits_int(count) || !sg_fits_int((long long)count * S * S)) return SG_EINVAL;
  FsPickArgs a = {};
  a.D = D; a.mult = mult_in; a.selected = selected; a.counts = counts; a.assign = assign; a.cost = cost;
  a.S = S; a.K = K; a.W = W;
  return fs_launch<wt_pick_kernel<true>, wt_pick_kernel<false>>(a, 2, count, (hipStream_t)stream);
}
