// Ensemble scores of sampled scenario paths: CRPS, energy score, spread / skill and the rank histogram
// (include/stemgnn_hip.h: stemgnn_ensemble_scores / _masked).
//
// target [count, H, N], paths [count, S, H, N] fp32; every value is de-normalised to fp64 (v * mul[n] + add[n], the product
// and the sum rounded separately) where it is loaded and all arithmetic is fp64 from there.  Three launches:
//
// energy:   one workgroup per (row (c, h), 32 x 32 tile (I, J) of path pairs, I <= J).  N is walked in chunks of 64 nodes: the
//           two panels of 32 paths x 64 nodes (one when I == J) and the target chunk go to LDS as fp64, rows 65 doubles apart;
//           thread (ti, tj) = (t / 16, t % 16) owns the pairs (2 ti + {0, 1}, 2 tj + {0, 1}) and adds (x_sn - x_s'n)^2 into four
//           registers -- DIFFERENCES, never |x|^2 + |x'|^2 - 2 x.x' (coupling="path": nearly coincident paths).  A half-wave reads
//           two panel-A rows (broadcasts, 260 words apart: banks 4 apart) and sixteen panel-B rows (8-byte reads at banks 4 tj):
//           conflict-free.  The diagonal tiles also form sum_n (x_sn - y_n)^2.  Then the square roots, each pair s < s' counted
//           once (the finish doubles it), a fixed-order block sum, and one partial per workgroup.  A node left out (masked, NaN
//           target) is stored as 0 on both sides.  This launch also zeroes `hist`, which the next one adds into.
// marginal: one workgroup per (row, tile of C nodes); C = 64 .. 4, a power of two: the smallest that covers N, halved until
//           the tile of S x C doubles is within 32 KB.  Thread (g, c) = (t / C, t % C) owns rows g, g + G, .. of column c
//           (G = 256 / C): it loads them (lanes along n: coalesced), counts x < y and x == y on the raw fp32 values, adds
//           |x - y| and x, and files the fp64 value in LDS.  After one barrier every thread knows its column's mean; the second
//           walk adds (x - mean)^2 and, four own rows at a time, |x_i - x_j| over j < i straight from LDS (one 8-byte read feeds
//           four sums; lanes of a half-wave read consecutive words or one address).  Columns meet in LDS in g order, the
//           tile's columns in c order, one partial per workgroup and statistic; ranks go to an LDS histogram and from there
//           to `hist` with one 64-bit integer add per non-empty bin.
// finish:   one workgroup adds the partials of every step in index order (thread-strided, then a fixed tree), writes the
//           per-step statistics and, summing the steps in order, the overall ones.
// No floating-point atomics, no allocation, no host synchronisation: the same bits on every run.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/stemgnn_hip.h"
#include "scenario_math.h"
#include "sg_host.h"

namespace {

constexpr int EN_THREADS = 256;
constexpr int EN_MAX_S = 1024;
constexpr int EN_TILE_BYTES = 32 * 1024;    // marginal: the S x C tile of doubles
constexpr int EN_ROWS = 4;                  // marginal: own rows per walk over the column
constexpr int EN_PT = 32;                   // energy: paths per panel
constexpr int EN_NC = 64;                   // energy: nodes per chunk
constexpr int EN_LD = EN_NC + 1;            // energy: doubles between panel rows
constexpr int EN_FIN_THREADS = 1024;
constexpr int EN_K = 6;

struct EnArgs {
  const float* target;                      // [count, H, N]
  const float* paths;                       // [count, S, H, N]
  const double* mul;                        // [N] or NULL
  const double* add;
  // partials, step-major so that a step's are one run: [5][H][count][tn]: sum |x - y|, pair sum, se, var, valid elements;
  // [2][H][count][pairs]: pair sum, sum ||x - y||; then [H][count]: the row has a node
  double* mpart;
  double* epart;
  double* out;
  unsigned long long* hist;                 // [H][S + 1]
  long long rows, count;                    // rows = count * H
  int S, H, N, C, tn, nt, pairs, fair;
};

template <bool MASKED>
__global__ __launch_bounds__(EN_THREADS) void en_energy_kernel(const EnArgs a) {
  __shared__ double pa[EN_PT * EN_LD], pb_own[EN_PT * EN_LD], ys[EN_NC], red[EN_THREADS / 64];
  const int t = threadIdx.x, S = a.S, N = a.N;
  {                                                            // hist = 0 ahead of the marginal launch
    const size_t bins = (size_t)a.H * (S + 1);
    for (size_t i = (size_t)blockIdx.x * EN_THREADS + t; i < bins; i += (size_t)gridDim.x * EN_THREADS) a.hist[i] = 0ull;
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
  const size_t HN = (size_t)a.H * N;
  const float* tg = a.target + row * N;
  const float* px = a.paths + (b * S * a.H + h) * (size_t)N;   // path s: + s * HN
  const bool dn = a.mul != nullptr;
  const int ln = t & (EN_NC - 1), lr = t >> 6;                 // the loader's column and first row
  const int ti = t >> 4, tj = t & 15;
  double acc[2][2] = {{0.0, 0.0}, {0.0, 0.0}}, e0 = 0.0, e1 = 0.0;
  int any = 0;
  for (int n0 = 0; n0 < N; n0 += EN_NC) {
    const int n = n0 + ln;
    const bool live = n < N;
    const float y = live ? tg[n] : 0.f;
    const bool valid = live && (!MASKED || y == y);
    const double mu = (dn && live) ? a.mul[n] : 1.0, ad = (dn && live) ? a.add[n] : 0.0;
    any |= valid ? 1 : 0;
    __syncthreads();                                           // the previous chunk has been read
    for (int r = lr; r < EN_PT; r += EN_THREADS / EN_NC) {
      const int si = I * EN_PT + r, sj = J * EN_PT + r;
      pa[r * EN_LD + ln] = (valid && si < S) ? sg_dn(px[(size_t)si * HN + n], dn, mu, ad) : 0.0;
      if (!diag) pb_own[r * EN_LD + ln] = (valid && sj < S) ? sg_dn(px[(size_t)sj * HN + n], dn, mu, ad) : 0.0;
    }
    if (t < EN_NC) ys[t] = valid ? sg_dn(y, dn, mu, ad) : 0.0;
    __syncthreads();
    const int lim = min(EN_NC, N - n0);
    const double* ra = pa + (2 * ti) * EN_LD;
    const double* rb = pb + (2 * tj) * EN_LD;
    if (diag) {
      for (int k = 0; k < lim; ++k) {
        const double a0 = ra[k], a1 = ra[EN_LD + k], b0 = rb[k], b1 = rb[EN_LD + k], yk = ys[k];
        double d;
        d = a0 - b0; acc[0][0] = fma(d, d, acc[0][0]);
        d = a0 - b1; acc[0][1] = fma(d, d, acc[0][1]);
        d = a1 - b0; acc[1][0] = fma(d, d, acc[1][0]);
        d = a1 - b1; acc[1][1] = fma(d, d, acc[1][1]);
        d = a0 - yk; e0 = fma(d, d, e0);
        d = a1 - yk; e1 = fma(d, d, e1);
      }
    } else {
      for (int k = 0; k < lim; ++k) {
        const double a0 = ra[k], a1 = ra[EN_LD + k], b0 = rb[k], b1 = rb[EN_LD + k];
        double d;
        d = a0 - b0; acc[0][0] = fma(d, d, acc[0][0]);
        d = a0 - b1; acc[0][1] = fma(d, d, acc[0][1]);
        d = a1 - b0; acc[1][0] = fma(d, d, acc[1][0]);
        d = a1 - b1; acc[1][1] = fma(d, d, acc[1][1]);
      }
    }
  }
  double p = 0.0, e = 0.0;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) {
      const int si = I * EN_PT + 2 * ti + u, sj = J * EN_PT + 2 * tj + v;
      if (si < sj && sj < S) p += sqrt(acc[u][v]);
    }
  if (diag && tj == 0) {
    const int si = I * EN_PT + 2 * ti;
    if (si < S) e += sqrt(e0);
    if (si + 1 < S) e += sqrt(e1);
  }
  p = sg_block_sum(p, red);
  e = sg_block_sum(e, red);
  const int has = __syncthreads_or(any);
  if (t == 0) {
    const size_t np = (size_t)a.rows * a.pairs, r = (size_t)h * a.count + b;
    const size_t at = r * a.pairs + (blockIdx.x - row * (unsigned)a.pairs);
    a.epart[at] = p;
    a.epart[np + at] = e;
    if (I == 0 && J == 0) a.epart[2 * np + r] = has ? 1.0 : 0.0;
  }
}

template <bool MASKED>
__global__ __launch_bounds__(EN_THREADS) void en_marginal_kernel(const EnArgs a) {
  extern __shared__ double en_lds[];
  const int S = a.S, C = a.C, N = a.N, t = threadIdx.x;
  const int G = EN_THREADS / C, g = t / C, c = t - g * C;
  double* tile = en_lds;                                       // [S][C]
  double* rd = tile + (size_t)S * C;                           // [2][256]: per-thread sums, [g][c]
  double* rc = rd + 2 * EN_THREADS;                            // [5][64]: per-column results
  int* ri = reinterpret_cast<int*>(rc + 5 * 64);               // [2][256]
  int* lh = ri + 2 * EN_THREADS;                               // [S + 1]
  for (int i = t; i <= S; i += EN_THREADS) lh[i] = 0;
  const size_t row = blockIdx.x / (unsigned)a.tn;
  const int tl = (int)(blockIdx.x - row * (unsigned)a.tn);
  const size_t b = row / (unsigned)a.H;
  const int h = (int)(row - b * (unsigned)a.H);
  const size_t HN = (size_t)a.H * N;
  const int n = tl * C + c;
  const bool live = n < N;
  const bool dn = a.mul != nullptr;
  const float y = live ? a.target[row * N + n] : 0.f;
  const bool valid = live && (!MASKED || y == y);
  const double mu = (dn && live) ? a.mul[n] : 1.0, ad = (dn && live) ? a.add[n] : 0.0;
  const double yd = sg_dn(y, dn, mu, ad);
  const float* src = a.paths + (b * S * a.H + h) * (size_t)N + n;
  int lt = 0, eq = 0;
  double sa = 0.0, sx = 0.0;
  for (int i = g; i < S; i += G) {
    const float x = live ? src[(size_t)i * HN] : 0.f;
    const double xd = sg_dn(x, dn, mu, ad);
    tile[i * C + c] = xd;
    lt += x < y ? 1 : 0;
    eq += x == y ? 1 : 0;
    sa += fabs(xd - yd);
    sx += xd;
  }
  rd[t] = sa;
  rd[EN_THREADS + t] = sx;
  ri[t] = lt;
  ri[EN_THREADS + t] = eq;
  __syncthreads();
  double A = 0.0, SX = 0.0;
  int LT = 0, EQ = 0;
  for (int k = 0; k < G; ++k) {
    A += rd[k * C + c];
    SX += rd[EN_THREADS + k * C + c];
    LT += ri[k * C + c];
    EQ += ri[EN_THREADS + k * C + c];
  }
  const double mean = SX / (double)S;
  __syncthreads();                                             // rd is written again below
  double sv = 0.0, sp = 0.0;
  for (int i0 = g; i0 < S; i0 += G * EN_ROWS) {
    double xi[EN_ROWS], p[EN_ROWS];
    int top[EN_ROWS], last = 0;                                // row m meets the rows j < top[m]
#pragma unroll
    for (int m = 0; m < EN_ROWS; ++m) {
      const int i = i0 + m * G;
      top[m] = i < S ? i : 0;
      last = max(last, top[m]);
      xi[m] = tile[(i < S ? i : i0) * C + c];
      p[m] = 0.0;
      if (i < S) {
        const double d = xi[m] - mean;
        sv += d * d;
      }
    }
    // the rows below the first own row meet all four (when all four exist); only the last 3 G rows need the comparison
    const int common = i0 + (EN_ROWS - 1) * G < S ? i0 : 0;
    for (int j = 0; j < common; ++j) {
      const double w = tile[j * C + c];
#pragma unroll
      for (int m = 0; m < EN_ROWS; ++m) p[m] += fabs(xi[m] - w);
    }
    for (int j = common; j < last; ++j) {
      const double w = tile[j * C + c];
#pragma unroll
      for (int m = 0; m < EN_ROWS; ++m) p[m] += j < top[m] ? fabs(xi[m] - w) : 0.0;
    }
#pragma unroll
    for (int m = 0; m < EN_ROWS; ++m) sp += p[m];
  }
  rd[t] = sv;
  rd[EN_THREADS + t] = sp;
  __syncthreads();
  if (g == 0) {
    double V = 0.0, P = 0.0;
    for (int k = 0; k < G; ++k) {
      V += rd[k * C + c];
      P += rd[EN_THREADS + k * C + c];
    }
    const double dm = mean - yd;
    rc[0 * 64 + c] = valid ? A : 0.0;
    rc[1 * 64 + c] = valid ? P : 0.0;
    rc[2 * 64 + c] = valid ? dm * dm : 0.0;
    rc[3 * 64 + c] = valid ? V / (double)(S - 1) : 0.0;        // S == 1: 0 / 0
    rc[4 * 64 + c] = valid ? 1.0 : 0.0;
    if (valid && y == y) atomicAdd(&lh[LT + EQ / 2], 1);
  }
  __syncthreads();
  if (t < 5) {
    double s = 0.0;
    for (int k = 0; k < C; ++k) s += rc[t * 64 + k];
    a.mpart[((size_t)t * a.rows + (size_t)h * a.count + b) * a.tn + tl] = s;
  }
  for (int i = t; i <= S; i += EN_THREADS)
    if (lh[i]) atomicAdd(&a.hist[(size_t)h * (S + 1) + i], (unsigned long long)lh[i]);
}

__global__ __launch_bounds__(EN_FIN_THREADS) void en_finish_kernel(const EnArgs a) {
  __shared__ double red[EN_FIN_THREADS / 64];
  const int t = threadIdx.x, H = a.H;
  const long long count = a.count;
  const double S = (double)a.S, D = a.fair ? S * (S - 1.0) : S * S;
  const size_t nm = (size_t)a.rows * a.tn, np = (size_t)a.rows * a.pairs;
  double all[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int h = 0; h <= H; ++h) {
    double v[8];                                               // sum |x - y|, pairs, se, var, elements; energy pairs, sum ||x - y||, rows
    if (h < H) {
      // a step's partials are one run per statistic: thread t adds the items t, t + 1024, .. (coalesced, independent loads)
      double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      const size_t m0 = (size_t)h * count * a.tn, e0 = (size_t)h * count * a.pairs;
      for (size_t i = t; i < (size_t)count * a.tn; i += EN_FIN_THREADS) {
#pragma unroll
        for (int k = 0; k < 5; ++k) s[k] += a.mpart[k * nm + m0 + i];
      }
      for (size_t i = t; i < (size_t)count * a.pairs; i += EN_FIN_THREADS) {
        s[5] += a.epart[e0 + i];
        s[6] += a.epart[np + e0 + i];
      }
      for (size_t i = t; i < (size_t)count; i += EN_FIN_THREADS) s[7] += a.epart[2 * np + (size_t)h * count + i];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        v[k] = sg_block_sum(s[k], red);
        all[k] += v[k];
      }
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = all[k];
    }
    if (t == 0) {
      double* o = h < H ? a.out + EN_K + h : a.out;            // statistic k of step h: out[K + k * H + h]
      const size_t ld = h < H ? (size_t)H : 1;
      o[0 * ld] = (v[0] / S - v[1] / D) / v[4];
      o[1 * ld] = (v[6] / S - v[5] / D) / v[7];
      o[2 * ld] = sqrt(v[2] / v[4]);
      o[3 * ld] = sqrt(v[3] / v[4]);
      o[4 * ld] = v[4];
      o[5 * ld] = v[7];
    }
  }
}

// the launch shape of (count, S, H, N); false where the entries answer SG_EINVAL
bool en_plan(long count, int S, int H, int N, EnArgs* a) {
  if (count <= 0 || S <= 0 || H <= 0 || N <= 0 || S > EN_MAX_S || !sg_fits_int(count)) return false;
  int C = 4;
  while (C < 64 && C < N) C <<= 1;
  while (C > 4 && (size_t)S * C * 8 > (size_t)EN_TILE_BYTES) C >>= 1;
  const int nt = sg_ceil_div(S, EN_PT);
  a->S = S; a->H = H; a->N = N; a->C = C;
  a->tn = sg_ceil_div(N, C);
  a->nt = nt;
  a->pairs = nt * (nt + 1) / 2;
  // what an int carries in the kernels: the grids, a row's nodes, the histogram's bins, one origin's path values
  if (!sg_fits_int((long long)count * H) || !sg_fits_int((long long)H * N) || !sg_fits_int((long long)H * (S + 1)) ||
      !sg_fits_int((long long)S * H * N))
    return false;
  a->rows = (long long)count * H;
  a->count = count;
  return sg_fits_int(a->rows * a->tn) && sg_fits_int(a->rows * a->pairs);
}

size_t en_scratch(const EnArgs& a) { return (size_t)a.rows * (5 * (size_t)a.tn + 2 * (size_t)a.pairs + 1); }

template <bool MASKED>
int en_scores(const float* target, const float* paths, const double* mul, const double* add, long count, int S, int H, int N,
              int fair, double* scratch, double* out, long long* hist, void* stream) {
  if (!target || !paths || !scratch || !out || !hist) return SG_EINVAL;
  if ((mul == nullptr) != (add == nullptr)) return SG_EINVAL;
  EnArgs a = {};
  if (!en_plan(count, S, H, N, &a) || (fair && S < 2)) return SG_EINVAL;
  a.target = target; a.paths = paths; a.mul = mul; a.add = add; a.out = out;
  a.hist = reinterpret_cast<unsigned long long*>(hist);
  a.fair = fair ? 1 : 0;
  a.mpart = scratch;
  a.epart = scratch + 5 * (size_t)a.rows * a.tn;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(en_energy_kernel<MASKED>, dim3((unsigned)(a.rows * a.pairs)), dim3(EN_THREADS), 0, st, a);
  SG_TRY(hipGetLastError());
  const size_t lds = ((size_t)S * a.C + 2 * EN_THREADS + 5 * 64) * 8 + (2 * EN_THREADS + (size_t)S + 1) * 4;
  hipLaunchKernelGGL(en_marginal_kernel<MASKED>, dim3((unsigned)(a.rows * a.tn)), dim3(EN_THREADS), lds, st, a);
  SG_TRY(hipGetLastError());
  hipLaunchKernelGGL(en_finish_kernel, dim3(1), dim3(EN_FIN_THREADS), 0, st, a);
  SG_TRY(hipGetLastError());
  return 0;
}

}  // namespace

extern "C" size_t stemgnn_ensemble_scratch_doubles(long count, int S, int H, int N) {
  EnArgs a = {};
  return en_plan(count, S, H, N, &a) ? en_scratch(a) : 0;
}

extern "C" size_t stemgnn_ensemble_out_doubles(int H) { return H > 0 ? (size_t)EN_K * ((size_t)H + 1) : 0; }

extern "C" int stemgnn_ensemble_scores(const float* target, const float* paths, const double* mul, const double* add, long count,
                                       int S, int H, int N, int fair, double* scratch, double* out, long long* hist,
                                       void* stream) {
  return en_scores<false>(target, paths, mul, add, count, S, H, N, fair, scratch, out, hist, stream);
}

extern "C" int stemgnn_ensemble_scores_masked(const float* target, const float* paths, const double* mul, const double* add,
                                              long count, int S, int H, int N, int fair, double* scratch, double* out,
                                              long long* hist, void* stream) {
  return en_scores<true>(target, paths, mul, add, count, S, H, N, fair, scratch, out, hist, stream);
}
