/* stemgnn_hip.h -- C ABI of libstemgnn_hip.so: the MI355X (gfx950) implementation of StemGNN's
 * spectral hot path (latent-correlation attention -> Laplacian -> Chebyshev/eigen basis -> GFT ->
 * DFT/GLU/iDFT spe_seq_cell -> IGFT + forecast/backcast heads), forward and backward.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to contiguous row-major fp32 unless the name ends in _host;
 *   - all buffers (inputs, outputs, saved activations, workspaces) are owned by the caller; the
 *     library never allocates, frees or synchronises; every launch goes to `stream` (a hipStream_t
 *     passed as void*), so the calls are stream-ordered and graph-capturable;
 *   - a block's `packed`, `split`, `saved`, `scratch`, `gradpart` and the inference workspace need no initialisation by the caller:
 *     the library writes every float of them it later reads, padding columns and ragged row blocks included, and writes nothing
 *     beyond the size its stemgnn_*_floats function returns (tests/test_hip_block.py runs every entry on NaN-filled, guarded buffers);
 *   - return value: 0 on success, a negative hipError_t (-(int)err) on a launch failure, or
 *     SG_EINVAL (-10001) for a bad argument.  No exception crosses this boundary.
 *   - shapes: B batch, N nodes (units), W window (time_step), multi, H horizon, Wm = W*multi,
 *     M = B*N rows.
 *
 * Each entry point names the reference code it replaces (paths relative to microsoft/StemGNN).
 */
#ifndef STEMGNN_HIP_H
#define STEMGNN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SG_EINVAL (-10001)

/* number of per-StockBlock parameter tensors, in state_dict order of one block:
 * 0 weight[1,4,1,Wm,Wm]; 1,2 forecast.{w,b}; 3,4 forecast_result.{w,b}; 5,6 backcast.{w,b} (NULL for
 * stack_cnt>0); 7,8 backcast_short_cut.{w,b}; then GLUs.g.linear_left.{w,b}, GLUs.g.linear_right.{w,b}
 * for g=0..5 (9 + 4*g + {0,1,2,3}).   (models/base_model.py:23-44) */
#define SG_BLOCK_NPARAMS 33

/* library / build identification: returns a static string "stemgnn_hip <version> gfx950". */
const char* stemgnn_version(void);
/* compute units of the current HIP device (256 on MI355X): the launch-sizing formulas use it, never a constant */
int stemgnn_num_cus(void);

/* ---- sizes (in floats) of the caller-allocated buffers ----------------------------------------- */
size_t stemgnn_table_floats(int W, int multi);                       /* DFT / C2R tables            */
size_t stemgnn_packed_floats(int W, int multi);                      /* packed weights of one block */
size_t stemgnn_saved_floats(int B, int N, int W, int multi);         /* saved activations, one block fwd */
size_t stemgnn_scratch_floats(int B, int N, int W, int multi);       /* backward scratch, one block */
size_t stemgnn_gradpart_floats(int W, int multi, int nsplit);        /* split-M weight-grad partials */
size_t stemgnn_attn_saved_floats(int B, int N);                      /* key,query,rowsum,A,deg      */
size_t stemgnn_attn_scratch_floats(int B, int N, int nchunk);        /* attention backward scratch  */
size_t stemgnn_scratch_offset_dG(int B, int N, int W, int multi);    /* float offset of dG [M,3W] inside the backward scratch */

/* Fill the constant DFT tables (double-precision trig rounded to fp32) into a HOST buffer of
 * stemgnn_table_floats() floats; the caller copies it to the device once per (W, multi).
 * Replaces the library FFT plans behind torch.rfft/irfft (models/base_model.py:49,58). */
int stemgnn_make_tables_host(int W, int multi, float* tables_host);

/* ---- latent-correlation attention + Laplacian  (models/base_model.py:139-147, 151-162) --------
 * h        [N, B, N]  GRU output exactly as nn.GRU returns it (seq-major; :137), h[s,b,i]
 * wk, wq   [N]        weight_key / weight_query
 * seed     device uint64[2] = {seed, offset} for the dropout Philox stream (ignored if !training or p==0)
 * saved    stemgnn_attn_saved_floats(): key[B,N] | query[B,N] | rowsum[B,N] | A[N,N] (batch-mean, un-symmetrised) | deg[N]
 * attention_out [N,N] = 0.5(A+A^T)  (the tensor Model.forward returns)
 * mul_L    [4,N,N]: slot 0 := 0 (T0 is zeros, :129) and slot 1 := L are written here
 * parts    bit 0: attention (-> A | deg, contiguous N*N + N floats at saved + 3*B*N), bit 1: Laplacian from (A, deg);
 *          3 = both.  The batch mean (:140) is the ONE cross-sample reduction of the path: a data-parallel caller that
 *          wants single-process semantics for a split batch runs part 1, averages A | deg over the ranks, runs part 2.
 * Limits:  0 <= drop_p < 1 (forward and backward), and the attention part keeps four rows of N floats plus one float per
 *          batch of a chunk in 64 KiB of LDS: ceil(B / min(B, 8)) + 4 N <= 16384, i.e. N <= 4095 for B <= 32 (N <= 4094 up to
 *          B = 64).  A larger N returns SG_EINVAL before anything is launched.
 */
int stemgnn_attn_laplacian_fwd(const float* h, const float* wk, const float* wq, float alpha,
                               float drop_p, int training, const uint64_t* seed,
                               int B, int N, float* saved, float* attention_out, float* mul_L,
                               int parts, void* stream);
/* dL [N,N] = gradient w.r.t. mul_L slot 1 (total).  Outputs dh [N,B,N], dwk [N], dwq [N].
 * scratch: stemgnn_attn_scratch_floats(B,N,nchunk).  parts bit 0: Laplacian backward -> dA / B in scratch[0 .. N*N)
 * (averaged over the ranks by an exact-mode data-parallel caller), bit 1: softmax / key / query backward; 3 = both.
 * parts bit 2 (with bit 1): FACTORED output -- stop at dkey | dquery ([B,N] each, left in scratch behind the [N,N] dA:
 * scratch + N*N and scratch + N*N + B*N); dh / dwk / dwq are not touched (may be NULL).  In the model
 * dh[s][b][i] = dkey[b][i] wk[s] + dquery[b][i] wq[s] (models/base_model.py:154-155): stemgnn_gru_bwd_rank2 consumes the two
 * factors directly, stemgnn_keyquery_wgrad forms dwk / dwq from them off the critical chain. */
int stemgnn_attn_laplacian_bwd(const float* dL, const float* h, const float* wk, const float* wq,
                               float alpha, float drop_p, int training, const uint64_t* seed,
                               int B, int N, const float* saved, float* scratch, int nchunk,
                               float* dh, float* dwk, float* dwq, int parts, void* stream);
/* The same with an external gradient for the RETURNED attention: dA_ext [N,N] fp32 row-major = d(loss)/d(attention_out)
 * (a penalty on the learned graph, an edge's saliency).  Its adjoint through the symmetrisation (:143) and the batch mean (:140)
 * joins inside the Laplacian backward's own launch:
 *     dA / B = ((dd_i - dq_ij / 2) + (dA_ext[i][j] + dA_ext[j][i]) / 2) / B
 * -- no extra launch on the chain; with dA_ext all zeros the outputs have the bits of stemgnn_attn_laplacian_bwd's.
 * dL == NULL: attention-only backward (nothing reached mul_L): a small seed kernel writes dA / B = (dA_ext + dA_ext^T) / 2 / B
 * in place of the Laplacian backward.  dA_ext == NULL: exactly stemgnn_attn_laplacian_bwd.  Both NULL: SG_EINVAL.
 * parts, the scratch layout (stemgnn_attn_scratch_floats) and every other argument: as stemgnn_attn_laplacian_bwd. */
int stemgnn_attn_laplacian_bwd_ext(const float* dL, const float* dA_ext, const float* h, const float* wk, const float* wq,
                                   float alpha, float drop_p, int training, const uint64_t* seed,
                                   int B, int N, const float* saved, float* scratch, int nchunk,
                                   float* dh, float* dwk, float* dwq, int parts, void* stream);
/* test hook: write the 0/1 keep-mask [B,N,N] the kernels above generate for `seed`. */
int stemgnn_dropout_mask(float drop_p, const uint64_t* seed, int B, int N, float* mask, void* stream);
/* One step of a model's dropout stream (nn.Dropout draws a fresh mask per forward, models/base_model.py:101,142): used[0..1] :=
 * seed[0..1] (the {key, offset} the coming forward / backward pair reads), then seed[1] += 1 -- one launch, graph-capturable. */
int stemgnn_dropout_seed_next(uint64_t* seed, uint64_t* used, void* stream);

/* ---- Chebyshev basis  (models/base_model.py:121-134) --------------------------------------------
 * in: mul_L slot 1 = L;  out: slot 2 = 2LL, slot 3 = 2L(2LL) - L  (fp32 MFMA GEMMs). */
int stemgnn_cheb_fwd(float* mul_L, int N, void* stream);
/* dmul_L [4,N,N] gradient of all four slots (slot 0 ignored) -> dL [N,N]; scratch 2*N*N floats. */
int stemgnn_cheb_bwd(const float* mul_L, const float* dmul_L, float* dL, float* scratch, int N, void* stream);

/* ---- frozen / user-supplied graphs: the spectral basis from a given adjacency, without the GRU + attention front --------
 * A        [N,N]  un-symmetrised adjacency (what the model has after the batch mean, models/base_model.py:140), fp32 row-major
 * deg      [N]    its degrees (:141).  A graph taken from the model carries the degrees the model computed (the fused front sums
 *                 them in another order than a row sum of A); a free adjacency gets them from stemgnn_graph_degree.
 * All entries: one launch each (stemgnn_graph_basis_bwd: one), no memset node, no host sync -- graph-capturable; SG_EINVAL
 * before anything is launched for a NULL pointer or N <= 0 (n == 0, w <= 0, wsum <= 0).
 *
 * stemgnn_graph_degree: deg[i] = sum_j A[i][j], one wave per row, fixed order (independent of the launch geometry). */
int stemgnn_graph_degree(const float* A, int N, float* deg, void* stream);
/* (A, deg) -> attention_out [N,N] = 0.5 (A + A^T) and mul_L slots 0 (zeros) and 1 (L, :144-147): part 2 of
 * stemgnn_attn_laplacian_fwd as a call of its own (the same kernel, the same bits).  The caller runs stemgnn_cheb_fwd or
 * stemgnn_eigh_fwd on mul_L afterwards, as behind stemgnn_attn_laplacian_fwd. */
int stemgnn_graph_basis_fwd(const float* A, const float* deg, float* attention_out, float* mul_L, int N, void* stream);
/* Adjoint of the above w.r.t. A for deg = row sums of A: dL [N,N] = gradient of mul_L slot 1 (total, from stemgnn_cheb_bwd),
 * dA_ext [N,N] = gradient of attention_out; dA [N,N] out.  The degree term is always on (a free adjacency has no softmax behind
 * it to annihilate a row-constant gradient).  dL == NULL: dA = (dA_ext + dA_ext^T) / 2; dA_ext == NULL: the Laplacian's share
 * alone; both NULL: SG_EINVAL (the semantics of stemgnn_attn_laplacian_bwd_ext with B = 1).  For a STORED degree (a constant
 * of the graph) this is not the gradient: the caller decides. */
int stemgnn_graph_basis_bwd(const float* dL, const float* dA_ext, const float* A, const float* deg, float* dA, int N,
                            void* stream);
/* Running weighted mean of n floats (A | deg of one batch's graph) in fp64: acc[e] += w * v[e] (init != 0: acc[e] = w * v[e],
 * acc need not be cleared), then out[e] = (float)(acc[e] / wsum).  One thread per element and no atomics: the result depends
 * on the order of the calls alone. */
int stemgnn_graph_accumulate(const float* v, double w, double* acc, size_t n, int init, void* stream);
int stemgnn_graph_finish(const double* acc, double wsum, float* out, size_t n, void* stream);

/* ---- Laplacian eigendecomposition route (north-star; same function of L as stemgnn_cheb_fwd) --------
 * Symmetric N x N eigensolver L = U^T diag(lam) U, then slot k := sum_e p_k(lam_e) u_e u_e^T for k = 2,3 with
 * p = (2 l^2, 4 l^3 - l) (slot 0 = zeros and slot 1 = L are left as attn_laplacian_fwd wrote them).
 *   nsweeps <= 0 : direct solver, 7 launches, 3 <= N <= 2048: Householder tridiagonalisation as ONE persistent cluster
 *                  kernel (pending rank-2 update fused with the next symmetric mat-vec, one grid barrier per column) ->
 *                  multisection (Sturm counts, one wave per eigenvalue: 3 fp32 + 6 fp64 rounds of 65 points) -> fp64 inverse iteration (pivoted
 *                  tridiagonal LU) -> cluster pass (eigenvalues closer than 1e-9 |T|, repeated ones included, are
 *                  re-orthogonalised and re-iterated as LAPACK dstein does) -> reflector back-transform -> rebuild on
 *                  the MFMA GEMM core;
 *   nsweeps  > 0 : parallel one-sided Jacobi (one launch per tournament round, fp64 rotation parameters), one
 *                  Newton-Schulz re-orthogonalisation and Rayleigh quotients on MFMA.
 * lam [N] (ascending for the direct solver); U [N,N] with the eigenvectors in ROWS; scratch:
 * stemgnn_eigh_scratch_floats(N) (16-byte aligned).  stemgnn_eigh_status(): host-synchronous read-and-clear of the
 * solver's status word of the CURRENT device (0 ok, 2 = a grid-barrier wait of the tridiagonalisation timed out, 3 = a cluster
 * re-solve broke down).  stemgnn_eigh_cluster_fixes(): host-synchronous read-and-clear of the number of eigenvectors the
 * cluster pass re-orthogonalised on the current device (diagnostic; 0 for a spectrum without clusters). */
size_t stemgnn_eigh_scratch_floats(int N);
int stemgnn_eigh_fwd(float* mul_L, float* lam, float* U, float* scratch, int N, int nsweeps, void* stream);
/* The batched form north_star names (round 5; direct solver): `batch` matrices in ONE call, matrix m at mul_L + m 4 N^2
 * (slot 1 = L_m; slots 2 / 3 receive its rebuilt basis), lam + m N, U + m N^2, scratch + m stemgnn_eigh_scratch_floats(N).
 * N <= 256: every stage takes the batch as a grid dimension -- 7 launches whatever the batch, one workgroup per matrix in the
 * tridiagonalisation -- so 8 Laplacians of the PEMS07 size cost what one does; N > 256: the multi-workgroup
 * tridiagonalisation runs matrix by matrix, the other stages batched.  Results per matrix are bitwise those of stemgnn_eigh_fwd. */
int stemgnn_eigh_batched(float* mul_L, float* lam, float* U, float* scratch, int N, int batch, void* stream);
int stemgnn_eigh_status(void);
int stemgnn_eigh_cluster_fixes(void);

/* ---- split-bf16 GLU GEMM (experiment; BASELINE configs[1] "bf16/fp32", SURVEY 8b `_bf16` entry points) -----------
 * C[M,N] = A[M,K] B[N,K]^T -- the shape of one GLU layer (models/base_model.py:12-13, x W^T) -- with every fp32 operand
 * taken as the sum of `splits` bf16 numbers and the cross products evaluated on the bf16 MFMA pipe with fp32
 * accumulation: splits = 3 -> 6 products (~2^-24 relative, fp32 class), 2 -> 3 products (~2^-16), 1 -> plain bf16.
 * B is pre-split by stemgnn_split_weights_bf16 into `planes` (stemgnn_split_planes_floats floats, 16-byte aligned);
 * A is split on the fly.  K % 4 == 0 and A 16-byte aligned (SG_EINVAL otherwise).  Operands of the `_bf16` entries must
 * be finite and smaller in magnitude than bf16's largest finite value (0x7f7f0000, ~3.39e38): the split rounds to nearest
 * even on the bit pattern (sp_bf16_rne), which carries a larger value up to infinity and mangles NaN / Inf.
 * stemgnn_glu_gemm_f32 is the same product on the exact-fp32 MFMA core (any K, no alignment rule). */
size_t stemgnn_split_planes_floats(int N, int K, int splits);
int stemgnn_split_weights_bf16(const float* B, int N, int K, int splits, void* planes, void* stream);
int stemgnn_glu_gemm_bf16(const float* A, const void* planes, float* C, int M, int N, int K, int splits, void* stream);
int stemgnn_glu_gemm_f32(const float* A, const float* B, float* C, int M, int N, int K, void* stream);

/* ---- stand-alone GLU (models/base_model.py:6-13) and the general fp32 GEMM it is composed from ---------------------
 * stemgnn_sgemm_f32: C[M,N] (+)= A B on the exact-fp32 MFMA core; element (i,k) of A at A[i*lda+k] (a_kcontig) or
 * A[k*lda+i]; element (k,j) of B at B[j*ldb+k] (b_kcontig) or B[k*ldb+j]; accumulate != 0 adds to C.
 * Required (SG_EINVAL otherwise): lda >= (a_kcontig ? K : M), ldb >= (b_kcontig ? K : N), ldc >= N, positive sizes,
 * non-NULL pointers.  No alignment is required of any pointer or leading dimension: operands whose base pointers are
 * 16-byte aligned and whose lda, ldb (and K where an operand is k-contiguous, M where A is not, N where B is not) are
 * multiples of 4 take the vector loaders (16-byte loads), every other call the scalar, fully predicated loaders -- same
 * values either way.  Only [M, N] of C is written; the ldc - N gap columns are left alone.
 * stemgnn_sgemm_paths: which of the two a call takes, host only (launches nothing, dereferences nothing; same operand
 * checks): out = {vec (1 vector loaders, 0 scalar), nx = row tiles of 64, ny = column tiles of 128, blocks = the 1-D
 * grid, nx rounded up to 8 times ny (block L -> row tile L % 8 + 8 * (L / 8 / ny), column tile L / 8 % ny)}.  It asks
 * the launch's own plan (g2_plan, csrc/gemm2.h); tests use it to prove which loaders and tile orders their cases ran.
 * stemgnn_glu_combine_fwd: out = (U + bl) * sigmoid(V + br), saving gate = sigmoid(.) and lin = U + bl ([M,C] each);
 * stemgnn_glu_combine_bwd: dU = dout * gate, dV = dout * lin * gate * (1 - gate);  stemgnn_colsum: out[c] = sum_m X[m][c]
 * in a fixed order (bias gradients). */
int stemgnn_sgemm_f32(const float* A, int lda, int a_kcontig, const float* B, int ldb, int b_kcontig, float* C, int ldc,
                      int M, int N, int K, int accumulate, void* stream);
int stemgnn_sgemm_paths(const void* A, int lda, int a_kcontig, const void* B, int ldb, int b_kcontig, int M, int N, int K,
                        int* out /* [4] */);
int stemgnn_glu_combine_fwd(const float* U, const float* V, const float* bl, const float* br, float* out, float* gate,
                            float* lin, int M, int C, void* stream);
int stemgnn_glu_combine_bwd(const float* dout, const float* lin, const float* gate, float* dU, float* dV, int M, int C,
                            void* stream);
int stemgnn_colsum(const float* X, int M, int C, float* out, void* stream);

/* ---- GRU front (models/base_model.py:92,137: nn.GRU(time_step, units) over the node axis) ------------
 * seq_len S (= N nodes), batch B, input size W, hidden size Hd (= N).  PyTorch gate order (r,z,n).
 * x [B,W,S] is the model input read in place (x_s[b,t] = x[b,t,s]); w_ih [3Hd,W], w_hh [3Hd,Hd],
 * b_ih, b_hh [3Hd]; h_ext [S+1,B,Hd]: slab 0 is set to zero (h_{-1}) and slabs 1..S are exactly nn.GRU's output
 * (so h_ext + B*Hd is the [S,B,Hd] tensor, and h_ext itself is "h of the previous step" row for row -- the
 * operand of the dW_hh GEMM); reserve keeps r,z,n,gh_n for backward.
 * Recurrence: P = 1..8 persistent workgroups per batch row keep their slice of w_hh resident in registers
 * for all S steps and exchange h (forward) / the gate gradients (backward) once per step through tagged
 * 8-byte granules (bounded spins; a timeout sets *status = 1, a device int the caller owns and zeroes);
 * hidden sizes beyond 512 run on ONE cluster of <= 224 workgroups that holds w_hh as MFMA A operands for up to 16
 * batch rows at a time (csrc/gru_wide.h; flags + write-through stores instead of granules). */
size_t stemgnn_gru_reserve_floats(int B, int S, int Hd);
size_t stemgnn_gru_fwd_scratch_floats(int B, int S, int Hd);
size_t stemgnn_gru_bwd_scratch_floats(int B, int S, int Hd, int W);
/* CUs (one workgroup each) the backward recurrence occupies for its whole run at this shape: a caller that overlaps other
 * kernels with it on another stream sizes them for the remaining CUs. */
int stemgnn_gru_bwd_cus(int B, int Hd);
/* The launch plan of the GRU front at a shape (host only, no GPU work): the one function stemgnn_gru_fwd / _fwd_infer,
 * every stemgnn_gru_bwd* entry, stemgnn_gru_bwd_rank2_ok and stemgnn_gru_bwd_cus take their decisions from, written out as
 * SG_GRU_PATH_WORDS ints.  cus > 0: the plan for a device with that many CUs; cus <= 0: the current device.  Parts that
 * look at pointers (16-byte alignment of the projection's output, the fused weight-gradient kernel's operand rules) are
 * answered for buffers that are each their own 256-byte aligned allocation, as the model's are.  Environment switches
 * count as the launchers read them.  SG_EINVAL for a bad argument.  Tests use it to prove that their shapes reach every
 * kernel family and instantiation (a moved threshold fails on the CPU instead of silently dropping coverage). */
#define SG_GRU_PATH_WORDS 16
#define SG_GRU_FWD_FAMILY   0    /* SG_GRU_FAM_*                                                                          */
#define SG_GRU_FWD_P        1    /* workgroups per batch row of the forward cluster (0: wide / streaming)                 */
#define SG_GRU_FWD_K        2    /* unrolled mat-vec length KF of gru_fwd_cluster4_kernel (0 elsewhere)                   */
#define SG_GRU_GI_STREAM    3    /* input projection: 1 the streaming kernel (W == 12, Hd % 4 == 0), 0 the GEMM           */
#define SG_GRU_BWD_FAMILY   4    /* SG_GRU_FAM_*                                                                          */
#define SG_GRU_BWD_P        5    /* workgroups per batch row of the backward cluster (0: wide / streaming)                */
#define SG_GRU_BWD_KU       6    /* unrolled mat-vec length KU of gru_bwd_cluster4 / cluster2_kernel (0 elsewhere)        */
#define SG_GRU_BWD_SLICES   7    /* owner slices per mat-vec wave (1 or 2; 0 outside the wave-level clusters)             */
#define SG_GRU_IH_FOLDED    8    /* dW_ih | db_ih accumulated inside the recurrence (else the split-K GEMM)               */
#define SG_GRU_HH_FORM      9    /* SG_GRU_HH_*                                                                           */
#define SG_GRU_IH_SLABS     10   /* slabs the dW_ih | db_ih sum adds up: B when folded, else the split count 32           */
#define SG_GRU_RANK2_OK     11   /* == stemgnn_gru_bwd_rank2_ok(B, Hd)                                                    */
#define SG_GRU_WIDE_PASSES  12   /* wide cluster: 16-row passes over the batch, ceil(B / 16) (0: not wide)                */
#define SG_GRU_WIDE_MT      13   /* wide cluster: 16-row MFMA tiles of a workgroup's 3 U gate rows                        */
#define SG_GRU_WIDE_GWF     14   /* wide cluster: forward instantiation, 16-unit groups per wave (8 or 16)                */
#define SG_GRU_WIDE_GWB     15   /* wide cluster: backward instantiation (24 or 48)                                       */
#define SG_GRU_FAM_STREAM   0    /* one workgroup per batch row, W_hh streamed from L2 every step                         */
#define SG_GRU_FAM_CLUSTER1 1    /* round-1 cluster (LDS staging), STEMGNN_GRU_CLUSTER=1 and hidden < 64                  */
#define SG_GRU_FAM_CLUSTER2 2    /* backward only: gru_bwd_cluster2_kernel (P = 5, 8)                                     */
#define SG_GRU_FAM_CLUSTER4 3    /* wave-specialised per-row cluster (gru_cluster4.h)                                     */
#define SG_GRU_FAM_WIDE     4    /* one MFMA cluster for all batch rows (gru_wide.h)                                      */
#define SG_GRU_HH_SLABS     0    /* dW_hh | db_hh as 32 split-K slabs + the fixed-order reduce                            */
#define SG_GRU_HH_TILES     1    /* fused weight-gradient kernel, tile list (<= 64 output tiles)                          */
#define SG_GRU_HH_FLAT      2    /* fused weight-gradient kernel, flat work list (> 64 output tiles)                      */
int stemgnn_gru_paths(int B, int S, int Hd, int W, int cus, int* out /* [SG_GRU_PATH_WORDS] */);
int stemgnn_gru_fwd(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                    int B, int S, int Hd, int W, float* scratch, float* h_ext, float* reserve, int* status,
                    void* stream);
/* dh_all [S,B,Hd] = gradient of every output step -> dw_ih, dw_hh, db_ih, db_hh (x's gradient: stemgnn_gru_input_grad behind
 * it); everything is ordered on `stream` (the side-stream schedules of round 2 were measured slower and removed in round 4). */
int stemgnn_gru_bwd(const float* dh_all, const float* x, const float* w_hh, const float* h_ext,
                    const float* reserve, int B, int S, int Hd, int W, float* scratch,
                    float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int* status, void* stream);

/* dwk[s] = sum_{b,i} dkey[b,i] h[s,b,i] (dwq likewise) from the factors a parts | 4 call of stemgnn_attn_laplacian_bwd left
 * in `attn_scratch`. */
int stemgnn_keyquery_wgrad(const float* h, const float* attn_scratch, float* dwk, float* dwq, int B, int N, void* stream);
/* parts bit 3 (value 8, with bit 2) of stemgnn_attn_laplacian_bwd leaves dquery as per-chunk partials; this sums them (same fixed
 * order) into `out` [B, N], or into the scratch's own dquery slot when out == NULL.  stemgnn_keyquery_wgrad2: the key / query
 * weight gradients from explicit dkey / dquery buffers. */
int stemgnn_attn_dquery_reduce(float* attn_scratch, int B, int N, int nchunk, float* out, void* stream);
int stemgnn_keyquery_wgrad2(const float* h, const float* dkey, const float* dquery, float* dwk, float* dwq, int B, int N,
                            void* stream);
/* stemgnn_gru_bwd with the output gradient given as the rank-2 form dh[s][b][i] = dkey[b][i] wk[s] + dquery[b][i] wq[s]
 * (dkey, dquery [B,Hd]; wk, wq [S]); only where stemgnn_gru_bwd_rank2_ok(B, Hd) (the wave-specialised per-row clusters). */
int stemgnn_gru_bwd_rank2_ok(int B, int Hd);
int stemgnn_gru_bwd_rank2(const float* dkey, const float* dquery, const float* wk, const float* wq, const float* x,
                          const float* w_hh, const float* h_ext, const float* reserve, int B, int S, int Hd, int W,
                          float* scratch, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int* status, void* stream);
/* The same with dquery still in the attention backward's per-chunk partials (stemgnn_attn_laplacian_bwd with parts bit 3 set):
 * `dquery` [B, Hd] is followed by the partials [B][nchunk][Hd], as in the attention scratch; the chunk sum (fixed order: the
 * bits of stemgnn_attn_laplacian_bwd's own reduction) runs inside the zero-fill launch ahead of the recurrence.
 * flags bit 0: the dW_hh product as three-term split-bf16 on the bf16 matrix pipe (STEMGNN_DTYPE=bf16x2; ~2^-16 relative per
 * product, fp32 accumulation, same fixed-order split reduction); 0: exact fp32. */
int stemgnn_gru_bwd_rank2_dq(const float* dkey, float* dquery, int nchunk, int flags, const float* wk, const float* wq, const float* x,
                             const float* w_hh, const float* h_ext, const float* reserve, int B, int S, int Hd, int W,
                             float* scratch, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int* status, void* stream);
/* stemgnn_gru_bwd_rank2 as two calls, with the dW_hh product running BESIDE the recurrence instead of behind it (round 5):
 *   _begin  (stream):              the fill of the control words, the fork point, the recurrence -- which now stores the gate
 *                                  gradients write-through and counts finished chunks of 4 time steps per workgroup;
 *   _finish (side_stream, stream): on `side_stream`, ordered behind the fill, persistent workgroups (at most the CUs the
 *                                  recurrence leaves free) that take the weight-gradient work items in the order their rows
 *                                  become final, wait (BOUNDED) for the recurrence to get there, claim and compute them; on
 *                                  `stream`, behind the recurrence, the closing launch: the items of the last few time steps,
 *                                  anything the side launch did not claim, the fixed-order sums, dW_ih | db_ih.
 * The caller joins `side_stream` into `stream` afterwards.  Same arguments as stemgnn_gru_bwd_rank2 for both; dW_hh has the
 * SAME BITS as from the single call (one K partition, one summation order, whoever computes which item); a side launch that
 * cannot run beside the recurrence (a serialising graph executor) times out and the closing launch does everything.
 * Only where stemgnn_gru_bwd_overlap_ok (the rank-2 kernels, W <= 16, S >= 32, >= 32 free CUs, STEMGNN_GRU_WHH_OVERLAP=1 --
 * OFF by default: measured 1.102 against 1.105 ms per step at the headline shape, see csrc/gru.hip).
 * ctl: NULL -- the progress counters / claims / arrival counters live inside `scratch`, `_begin` zeroes them and `_finish`
 * makes `side_stream` wait for that fill through an event.  Inside a captured hipGraph that edge is NOT enough: the ROCm
 * executor makes a node with a parent on another branch wait for everything that branch has queued by then -- the recurrence
 * included (measured, profiles/r05_gru_whh_overlap.md).  So a graph caller passes its own buffer of
 * stemgnn_gru_bwd_ctl_words(S) zeroed words, zeroed (every step) at a point that is ordered ahead of both streams' use by
 * edges the step has anyway, and the side launch gets no parent on `stream` at all. */
int stemgnn_gru_bwd_overlap_ok(int B, int S, int Hd, int W);
size_t stemgnn_gru_bwd_ctl_words(int S);
int stemgnn_gru_bwd_rank2_begin(const float* dkey, const float* dquery, const float* wk, const float* wq, const float* x,
                                const float* w_hh, const float* h_ext, const float* reserve, int B, int S, int Hd, int W,
                                float* scratch, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int* status,
                                unsigned* ctl, void* stream);
int stemgnn_gru_bwd_rank2_finish(const float* dkey, const float* dquery, const float* wk, const float* wq, const float* x,
                                 const float* w_hh, const float* h_ext, const float* reserve, int B, int S, int Hd, int W,
                                 float* scratch, float* dw_ih, float* dw_hh, float* db_ih, float* db_hh, int* status,
                                 unsigned* ctl, void* side_stream, void* stream);
/* Weights-off backward (no GRU parameter needs a gradient): the recurrence alone, on the plain kernels -- no dW_hh product, no
 * dW_ih accumulation, no reduce launch.  Same arguments as stemgnn_gru_bwd / stemgnn_gru_bwd_rank2_dq without the four weight
 * outputs (and without the dW_hh flags); the gate gradients in `scratch` carry the same bits as from those calls.
 * stemgnn_gru_bwd_rank2_recur: nchunk > 0 -- dquery is followed by the attention backward's per-chunk partials, summed in the
 * fill launch as in stemgnn_gru_bwd_rank2_dq; nchunk == 0 -- dquery is already summed. */
int stemgnn_gru_bwd_recur(const float* dh_all, const float* x, const float* w_hh, const float* h_ext, const float* reserve,
                          int B, int S, int Hd, int W, float* scratch, int* status, void* stream);
int stemgnn_gru_bwd_rank2_recur(const float* dkey, float* dquery, int nchunk, const float* wk, const float* wq, const float* x,
                                const float* w_hh, const float* h_ext, const float* reserve, int B, int S, int Hd, int W,
                                float* scratch, int* status, void* stream);
/* Gradient of the GRU's input (gi = x W_ih^T + b_ih): dx[b][t][s] = sum_j dgi[s*B + b][j] W_ih[j][t], x's own [B, W, S] layout
 * (written, not accumulated).  `scratch` is the scratch of an earlier stemgnn_gru_bwd, _rank2, _rank2_dq, _rank2_begin (+ its
 * _finish), _recur or _rank2_recur call on the same stream, whose gate gradients dgi [S*B, 3 Hd] sit at its offset 0.  Exact
 * fp32 on the MFMA core, one fixed summation order: bit-identical from launch to launch. */
int stemgnn_gru_input_grad(const float* scratch, const float* w_ih, int B, int S, int Hd, int W, float* dx, void* stream);

/* ---- weight packing (per StockBlock, once per optimizer step) -----------------------------------
 * Folds the length-W DFT (:49-51) into the first GLU layer, drops the dead C2R bins,
 * folds the C2R inverse DFT (:58) into the graph-conv weight (:66-67), and lays the GLU weights out
 * as K-major "pair" panels for the MFMA kernels.  params_host: SG_BLOCK_NPARAMS device pointers
 * (host array). */
int stemgnn_block_pack(const float* const* params_host, const float* tables, float* packed,
                       int W, int multi, void* stream);
/* The pair panels, biases and the folded graph-conv weight only -- without the two fp32 stage streams of the fused fp32
 * kernels (stemgnn_glu_fused_repack writes those).  For a caller whose GLU forward / data gradients run on the split-bf16
 * kernels (stemgnn_glu_split_panels packs THEIR streams from the panels): nothing would read the fp32 streams. */
int stemgnn_block_pack_panels(const float* const* params_host, const float* tables, float* packed, int W, int multi,
                              void* stream);
/* The GLU weights of `packed` once more as the stage stream of the fused three-layer forward (csrc/glu_fused.h), written
 * behind the panels inside the same buffer; stemgnn_block_pack calls it (exported for callers that fill the panels
 * themselves).  No-op for (W, multi) the fused kernel does not cover (padded channel count 4 W multi > 256). */
int stemgnn_glu_fused_repack(float* packed, int W, int multi, void* stream);
/* adjoint of the above: scatter the weight gradients (slab 0 of every gradpart region, left complete by
 * stemgnn_block_wgrad or by the parts & 2 calls of stemgnn_igft_heads_bwd / stemgnn_spectral_glu_bwd) into the parameter
 * gradients grads_host[SG_BLOCK_NPARAMS] (entries may be NULL to skip).  nsplit = the value gradpart was sized with.
 * has_backcast == 0: entries 5..8 (the backcast head and the short-cut the block then never evaluates, :73-74) are not written. */
int stemgnn_block_unpack_grads(const float* gradpart, int nsplit, const float* tables,
                               float* const* grads_host, int W, int multi, int has_backcast, void* stream);

/* ---- GFT  (models/base_model.py:62-64)  G[b,n,(k-1)W+t] = sum_m T_k[n,m] X[b,m,t], k=1..3 -----
 * X is addressed as X[b*xs_b + m*xs_n + t*xs_t]: block 0 reads the model input x[B,W,N] in place
 * (xs = W*N, 1, N), block 1 reads the backcast [B,N,W] (xs = N*W, W, 1).  G [M, 3W]. */
int stemgnn_gft_fwd(const float* mul_L, const float* X, long xs_b, long xs_n, long xs_t,
                    float* G, int B, int N, int W, void* stream);
/* dG [2][M,3W]: the two per-branch partial slabs stemgnn_spectral_glu_bwd leaves at stemgnn_scratch_offset_dG (their
 * sum is the gradient; added while loading) -> dX [B,N,W] (may be NULL) and dmul_L[1..3] (+= if accumulate; may be NULL: a
 * caller can run the two products of a block on different streams -- only the data gradient is on the backward's chain). */
int stemgnn_gft_bwd(const float* mul_L, const float* X, long xs_b, long xs_n, long xs_t,
                    const float* dG, float* dX, float* dmul_L, int accumulate,
                    int B, int N, int W, void* stream);
/* d(mul_L)[1..3] of BOTH blocks as one product (written, not accumulated): the reduction runs over block 0's (b, t) range,
 * then block 1's.  X0 / X1, dG0 / dG1 as in stemgnn_gft_bwd (reference: autograd of models/base_model.py:64, mul_L is shared
 * by the two blocks, :172). */
int stemgnn_gft_bwd_dt2(const float* X0, long xs0_b, long xs0_n, long xs0_t, const float* dG0, const float* X1, long xs1_b,
                        long xs1_n, long xs1_t, const float* dG1, float* dmul_L, int B, int N, int W, void* stream);

/* ---- spe_seq_cell: DFT -> 3x GLU on Re and Im (models/base_model.py:46-54, GLU :12-13) ----------
 * G = saved + offset(G) is read; GLU outputs and gates are written into `saved`. */
int stemgnn_spectral_glu_fwd(const float* packed, float* saved, int B, int N, int W, int multi, void* stream);
/* needs d(pre-activation) of the last GLU layer in scratch (written by igft_heads_bwd); produces dG in
 * scratch.dG and the GLU weight-gradient partials in gradpart.
 * parts: bit 0 = data-gradient chain (layer 2 -> 1 -> 0 -> dG), bit 1 = the weight-gradient GEMMs.  The two parts
 * only share read-only inputs once the chain has run, so a caller may issue part 2 later or on another stream
 * (it is off the critical path of the backward pass); 3 = both, in order.  bit 2 (with bit 1): the fused weight-gradient
 * launch's products as three-term split-bf16 (see stemgnn_block_wgrad_split). */
int stemgnn_spectral_glu_bwd(const float* packed, const float* saved, float* scratch, float* gradpart,
                             int nsplit, int parts, int B, int N, int W, int multi, void* stream);
/* Split-bf16 arithmetic for the same layers (BASELINE.json configs[1] "bf16/fp32"; reference data and weights are fp32,
 * models/base_model.py:12-13, 52-54): every fp32 operand is the exact sum of `splits` bf16 numbers (3: fp32-class
 * products from 6 bf16 MFMAs, 2: ~2^-16 relative from 3) with fp32 accumulation on v_mfma_f32_32x32x16_bf16.
 * stemgnn_glu_split_panels turns the packed fp32 panels of layers 1, 2 (both branches) into the bf16 plane sets the two
 * entry points read (`split`: caller-owned, 16-byte aligned, stemgnn_glu_split_floats floats; once per step, after
 * stemgnn_block_pack).  _fwd_split == stemgnn_spectral_glu_fwd, _dgrad_split == stemgnn_spectral_glu_bwd with parts = 1,
 * with layers 1, 2 on the split kernel (layer 0 and its data gradient stay exact fp32: K = 3W, traffic-bound); saved
 * activations, scratch layout and every downstream stage are unchanged.  Shapes that break the 16-byte rules of the
 * split kernel run the fp32 kernels. */
size_t stemgnn_glu_split_floats(int W, int multi, int splits);
int stemgnn_glu_split_panels(const float* packed, float* split, int W, int multi, int splits, void* stream);
int stemgnn_spectral_glu_fwd_split(const float* packed, const float* split, float* saved, int B, int N, int W, int multi,
                                   int splits, void* stream);
/* Warm-up of the fused forward: the same kernel instance the real launch of a [B, N] batch gets, over four row blocks (eight
 * workgroups, one per XCD and branch), writing into a caller-owned dummy `saved` of stemgnn_glu_warm_saved_floats floats whose
 * G region holds any finite values.  splits = 0: the fp32 kernel (`split` ignored), 2: the split-bf16 kernel.  Brings the
 * kernel's code and block's weight stream into the XCDs' L2 ahead of the first real launch of a step (-10 us at PEMS07); a
 * no-op returning 0 where the fused kernels do not apply. */
size_t stemgnn_glu_warm_saved_floats(int W, int multi);
int stemgnn_spectral_glu_fwd_warm(const float* packed, const float* split, float* saved, int B, int N, int W, int multi,
                                  int splits, void* stream);
int stemgnn_spectral_glu_dgrad_split(const float* packed, const float* split, const float* saved, float* scratch,
                                     int B, int N, int W, int multi, int splits, void* stream);
/* Round 5: with splits == 2 and a padded channel count 4 W multi <= 256 (every BASELINE configuration but configs[4])
 * stemgnn_spectral_glu_fwd_split is ONE launch for the three layers with the split-bf16 products inside
 * (csrc/glu_fused_bf16.h: the row block's activations resident in LDS as two bf16 planes, the pre-split weights -- written
 * by stemgnn_glu_split_panels into the same `split` buffer -- on a direct-to-LDS ring; layer 0 is split too), and
 * stemgnn_spectral_glu_dgrad_split is ONE launch for d(pre-activation) of layer 2 -> 1 -> 0 -> dG likewise (its layer-0 product
 * included).  The saved out / gate and every d(pre-activation) stay fp32, so weight gradients, heads and the rest are
 * unchanged.  stemgnn_glu_fused_bf16_ok tells (1 / 0) whether those forms apply (STEMGNN_GLU_FUSED=0 turns them off). */
int stemgnn_glu_fused_bf16_ok(int W, int multi, int splits);

/* ---- C2R iDFT + graph-conv weight + forecast / backcast heads (models/base_model.py:55-58, 65-74)
 * forecast [M,W]: written (accumulate=0) or added to (accumulate=1: result[0]+result[1], :174 -- old + the finished forecast, one
 * rounding away from the sum of the two).
 * backcast [M,W] (block 0 only, else NULL); X as in gft_fwd (short-cut input, :71). */
int stemgnn_igft_heads_fwd(const float* const* params_host, const float* packed, float* saved,
                           const float* X, long xs_b, long xs_n, long xs_t,
                           float* forecast, int accumulate, float* backcast,
                           int B, int N, int W, int multi, void* stream);
/* dforecast [M,W], dbackcast [M,W] or NULL, backcast = forward output (for sigmoid').  parts bit 0: data path
 * (dpF, dpB, dig and d(pre-activation) of the last GLU layer into scratch); bit 1: the heads' / graph-conv
 * weight-gradient partials (needs bit 0's results). */
int stemgnn_igft_heads_bwd(const float* const* params_host, const float* packed, const float* saved,
                           const float* X, long xs_b, long xs_n, long xs_t,
                           const float* dforecast, const float* dbackcast, const float* backcast,
                           float* scratch, float* gradpart, int nsplit, int parts,
                           int B, int N, int W, int multi, void* stream);

/* Stand-alone block with a differentiable input only: the short-cut head's direct term (models/base_model.py:71-72),
 * dX [M,W] -= dpB BS_w, with dpB taken from the scratch the data part (parts & 1) of stemgnn_igft_heads_bwd filled. */
int stemgnn_shortcut_dx(const float* scratch, const float* bs_w, float* dX, int B, int N, int W, int multi, void* stream);

/* ALL weight gradients of one StockBlock (autograd of models/base_model.py:12-13, 66-74 via models/handler.py:164): the
 * six GLU products and the heads' FR / F / BC / graph-conv products in ONE launch of the fused weight-gradient kernel
 * (direct-to-LDS operand ring, in-kernel fixed-order split reduction), the short-cut head BS beside it.  Needs the data
 * parts (parts & 1) of stemgnn_igft_heads_bwd and stemgnn_spectral_glu_bwd; leaves complete gradients in slab 0 of every
 * gradpart region (-> stemgnn_block_unpack_grads).  has_bc: block 0 (backcast heads present).  cu_percent (10..100):
 * share of the CUs the big launch should fill -- lower it when latency-critical kernels run beside it on another stream. */
int stemgnn_block_wgrad(const float* const* params_host, const float* packed, const float* saved,
                        const float* X, long xs_b, long xs_n, long xs_t, const float* dforecast, int has_bc,
                        float* scratch, float* gradpart, int nsplit, int cu_percent,
                        int B, int N, int W, int multi, void* stream);
/* The same launch with the fused kernel's products as three-term split-bf16 (a_hi b_hi + a_hi b_lo + a_lo b_hi, fp32
 * accumulation) on v_mfma_f32_32x32x16_bf16 when splits == 2 (STEMGNN_DTYPE=bf16x2; ~2^-16 relative per product); splits == 0
 * is stemgnn_block_wgrad.  Reference: the weight gradients autograd forms for models/base_model.py:12-13, 66-72. */
int stemgnn_block_wgrad_split(const float* const* params_host, const float* packed, const float* saved,
                              const float* X, long xs_b, long xs_n, long xs_t, const float* dforecast, int has_bc,
                              float* scratch, float* gradpart, int nsplit, int cu_percent, int B, int N, int W,
                              int multi, int splits, void* stream);

/* Which launch path each stage of one StockBlock takes at a shape (host only, no GPU work): a bitmask of SG_PATH_*, asked
 * through the same predicates the launchers use, for buffers allocated the way the model allocates them (each its own
 * 256-byte aligned allocation).  splits: 0 exact fp32, 2 / 3 the split-bf16 GLU forms (STEMGNN_DTYPE=bf16x2 / bf16x3).
 * Environment switches count as the launchers read them.  SG_EINVAL for a bad argument.  Tests use it to prove that their
 * shapes reach every path (a moved threshold fails on the CPU instead of silently dropping coverage). */
#define SG_PATH_GLU_FWD_FUSED   1    /* GLU forward: one fused three-layer launch (else per-layer launches)            */
#define SG_PATH_GLU_DGRAD_FUSED 2    /* GLU data-gradient chain: one fused launch (else per-layer launches)           */
#define SG_PATH_HEADS_FWD_FUSED 4    /* IGFT + heads forward: one fused kernel (else the per-stage GEMMs)             */
#define SG_PATH_HEADS_BWD_FUSED 8    /* heads backward, data part: one fused kernel (else the per-stage GEMMs)        */
#define SG_PATH_HEADS_BWD_16W   16   /* ... that kernel at 16 waves per workgroup (KF > 128; else 4)                  */
#define SG_PATH_LONG_K          32   /* K of the folded IGFT GEMM > 640: the long-K (two-level) instantiations        */
#define SG_PATH_WGRAD_FUSED     64   /* block 0's weight gradients in one fused launch (else the per-stage slab path) */
#define SG_PATH_GLU_WGRAD_FUSED 128  /* the six GLU products alone fit that kernel (what the slab path's GLU part asks) */
int stemgnn_block_paths(int B, int N, int W, int multi, int splits);

/* ---- inference forward (no saved activations; Model.predict / engine.ForecastStep) ----------------------------------
 * The _infer entries run the same kernels and arithmetic as their training counterparts -- bit-identical outputs -- without the
 * stores only the backward pass reads: no GRU `reserve`, no GLU gates, no layer-0 / layer-1 GLU outputs where the fused kernels
 * keep them in LDS, no ig / fs of the heads.  One block's intermediate tensors live in a caller-owned workspace `ws` of
 * ws_floats floats (layout: G [M,3W] | layer-2 GLU outputs [M,CP2[0]] | [M,CP2[1]] | optional ping-pong slabs 4 x [M,CP]);
 * it is reusable for block 1 once block 0's heads have run (stream order).
 * stemgnn_infer_workspace_floats: the size for the exact-fp32 and the bf16x2 forms (the ping-pong slabs are included where a
 * per-layer GLU launch or the per-stage heads path runs at this shape, or STEMGNN_GLU_FUSED=0);
 * stemgnn_infer_workspace_split_floats: the same for one arithmetic (splits 0, 2, 3 as stemgnn_spectral_glu_fwd_split; 3
 * always needs the slabs).  A workspace smaller than the path the call takes needs returns SG_EINVAL.
 * stemgnn_gru_fwd_infer      == stemgnn_gru_fwd without `reserve` (h_ext is written as ever: the attention reads it)
 * stemgnn_spectral_glu_fwd_infer / _split_infer == stemgnn_spectral_glu_fwd / _split, reading G from ws and writing the
 *                               layer-2 outputs into ws
 * stemgnn_igft_heads_fwd_infer == stemgnn_igft_heads_fwd reading the layer-2 outputs from ws
 * The GFT writes G with stemgnn_gft_fwd(..., G = ws, ...) (offset 0 of the workspace). */
size_t stemgnn_infer_workspace_floats(int B, int N, int W, int multi);
size_t stemgnn_infer_workspace_split_floats(int B, int N, int W, int multi, int splits);
int stemgnn_gru_fwd_infer(const float* x, const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh,
                          int B, int S, int Hd, int W, float* scratch, float* h_ext, int* status, void* stream);
int stemgnn_spectral_glu_fwd_infer(const float* packed, float* ws, size_t ws_floats, int B, int N, int W, int multi,
                                   void* stream);
int stemgnn_spectral_glu_fwd_split_infer(const float* packed, const float* split, float* ws, size_t ws_floats, int B, int N,
                                         int W, int multi, int splits, void* stream);
int stemgnn_igft_heads_fwd_infer(const float* const* params_host, const float* packed, float* ws, size_t ws_floats,
                                 const float* X, long xs_b, long xs_n, long xs_t, float* forecast, int accumulate,
                                 float* backcast, int B, int N, int W, int multi, void* stream);

/* ---- callers on either side of the blocks, fused ------------------------------------------------
 * fc tail (models/base_model.py:97-101,174-179): fsum [B*N, W] (block forecast sum) ->
 * forecast [B,H,N] = Linear(W,H)(LeakyReLU_0.01(Linear(W,W)(fsum))) permuted.  stemgnn_fc_tail_supported(W,H)
 * tells whether the fused kernels cover (W,H) (registers / LDS); otherwise the caller keeps its own fc. */
int stemgnn_fc_tail_supported(int W, int H);
size_t stemgnn_fc_tail_scratch_floats(int B, int N, int W, int H);
/* stemgnn_fc_tail_plan: how the fc-tail entries launch for (B, N, W, H), host only (launches nothing).  It is computed from what the
 * launchers use themselves -- the block-size constants, the LDS-size functions, both `*_scratch_floats` functions -- except [6] and
 * [7], which mirror the partial-sum kernels' text (csrc/tail.hip says where); the launchers do not read it.  Tests use it to
 * prove which block counts, ragged blocks and partial-sum trips their cases reach.  out = 12 ints for the 64-row entries
 * (stemgnn_fc_tail_fwd / _bwd) followed by 12 for the 32-row training entries (`_train*`, H = Q * H for a quantile head):
 *   [0] rows per block   [1] threads per row   [2] row blocks = ceil(B N / rows)   [3] nacc = (W + 1)(W + H) gradient elements
 *   [4] floats per block in `scratch` (nacc; training: nacc + 1, the block's loss sum at index nacc)
 *   [5] grid of the partial-sum launch = ceil([4] / 64)   [6] its block lanes   [7] blocks it sums per trip of all lanes
 *   [8] dynamic LDS bytes of the first kernel (fwd; training: the row kernel)   [9] 1 if that exceeds the 64 KB default (the
 *   launcher then raises the kernel's limit first)   [10], [11] the same for the second kernel (bwd; training: 0, 0).
 * SG_EINVAL where stemgnn_fc_tail_supported(W, H) is 0, B or N <= 0, B N beyond int, or out is NULL. */
enum { SG_TAIL_PLAN_WORDS = 24 };
int stemgnn_fc_tail_plan(int B, int N, int W, int H, int* out /* [SG_TAIL_PLAN_WORDS] */);
int stemgnn_fc_tail_fwd(const float* fsum, const float* w0, const float* b0, const float* w2, const float* b2,
                        int B, int N, int W, int H, float* forecast, void* stream);
int stemgnn_fc_tail_bwd(const float* dforecast, const float* fsum, const float* w0, const float* b0, const float* w2,
                        int B, int N, int W, int H, float* scratch, float* dfsum, float* dw0, float* db0,
                        float* dw2, float* db2, void* stream);
/* training tail in two launches: fc forward -> nn.MSELoss(reduction='mean') against target [B,H,N] -> d(loss)/d(forecast)
 * (upstream gradient taken as 1: loss.backward(), models/handler.py:162-164) -> fc backward.  Writes the loss (float, and
 * += into *loss_accum, double, if given), dfsum [B*N, W] and the four fc parameter gradients; forecast [B,H,N] is also
 * written when non-NULL.  Same arithmetic as stemgnn_fc_tail_fwd + stemgnn_mse_fwd/_bwd + stemgnn_fc_tail_bwd. */
size_t stemgnn_fc_tail_train_scratch_floats(int B, int N, int W, int H);
int stemgnn_fc_tail_train(const float* fsum, const float* target, const float* w0, const float* b0, const float* w2,
                          const float* b2, int B, int N, int W, int H, float* scratch, float* forecast,
                          float* loss, double* loss_accum, float* dfsum, float* dw0, float* db0, float* dw2,
                          float* db2, void* stream);
/* The same two launches as separate calls: `_rows` = the per-row part (forecast, d(fsum), per-row-block partial sums in
 * `scratch`), `_finish` = the fixed-order sum of the partials into loss / loss_accum / the fc gradients.  Nothing on the
 * backward's chain reads what `_finish` writes, so a step driver may queue it on another stream; same bits as the one call. */
int stemgnn_fc_tail_train_rows(const float* fsum, const float* target, const float* w0, const float* b0, const float* w2,
                               const float* b2, int B, int N, int W, int H, float* scratch, float* forecast, float* dfsum,
                               void* stream);
int stemgnn_fc_tail_train_finish(const float* scratch, int B, int N, int W, int H, float* loss, double* loss_accum,
                                 float* dw0, float* db0, float* dw2, float* db2, void* stream);
/* The same tail with a choice of loss and with missing targets (csrc/tail.hip; one kernel template, the three entries above
 * are its <MSE, unmasked> instantiation).  With d = forecast - target, `kind` picks the element loss:
 *   SG_LOSS_MSE   d^2
 *   SG_LOSS_MAE   |d|, derivative sign(d) with sign(0) = 0 (torch.nn.L1Loss)
 *   SG_LOSS_HUBER torch.nn.HuberLoss(delta = param): d^2 / 2 for |d| <= param, else param (|d| - param / 2); derivative
 *                 clamp(d, -param, param).  param must be finite and > 0 (ignored by the other kinds).
 * norm == NULL: loss = sum / (B H N) and a NaN target propagates, as in the entries above.  norm != NULL: a NaN target is a
 * MISSING target -- it is selected out (never multiplied by 0), so it reaches neither the loss nor any gradient whatever the
 * forecast holds there, and loss = (sum over the valid targets) * norm[1], with norm = the two floats
 * stemgnn_target_valid_count wrote for this target: norm[0] = (float)count of non-NaN values, norm[1] = (float)(1.0 / count),
 * or 0 when count == 0 (loss and every gradient are then exactly 0).  +-inf is a value, not a missing one; a NaN forecast on a
 * valid target still propagates.  What selection protects: the loss, dfsum, db0 and db2 whatever the forecast holds on a missing
 * target (NaN or inf included), and dw0 / dw2 as long as the row's activations are finite -- the weight-gradient partials form
 * dz * x and dy * a per row, so a row whose targets are ALL missing (dz = dy = 0) but whose fsum or activations are not finite gives
 * 0 * inf = NaN in dw0 / dw2, as torch's matmul backward does.  `_rows_loss` and `_finish_loss` read norm[1] from device memory when they run; `_finish_loss`
 * must get the norm (or NULL) its `_rows_loss` got.  stemgnn_target_valid_count is ONE launch of one workgroup with no
 * host sync (capturable in a hipGraph); its count is an integer sum: exact, order-independent, independent of what norm held.
 * Scratch: stemgnn_fc_tail_train_scratch_floats.  SG_EINVAL (nothing launched) on a NULL pointer other than norm / forecast /
 * loss_accum, n == 0, an unknown kind, a Huber param that is not finite or <= 0, or a shape outside the fc tail's range. */
enum { SG_LOSS_MSE = 0, SG_LOSS_MAE = 1, SG_LOSS_HUBER = 2, SG_LOSS_PINBALL = 3 };
int stemgnn_target_valid_count(const float* target, size_t n, float* norm, void* stream);
int stemgnn_fc_tail_train_loss(const float* fsum, const float* target, const float* w0, const float* b0, const float* w2,
                               const float* b2, int B, int N, int W, int H, int kind, float param, const float* norm,
                               float* scratch, float* forecast, float* loss, double* loss_accum, float* dfsum, float* dw0,
                               float* db0, float* dw2, float* db2, void* stream);
int stemgnn_fc_tail_train_rows_loss(const float* fsum, const float* target, const float* w0, const float* b0, const float* w2,
                                    const float* b2, int B, int N, int W, int H, int kind, float param, const float* norm,
                                    float* scratch, float* forecast, float* dfsum, void* stream);
int stemgnn_fc_tail_train_finish_loss(const float* scratch, int B, int N, int W, int H, const float* norm, float* loss,
                                      double* loss_accum, float* dw0, float* db0, float* dw2, float* db2, void* stream);
/* The same tail for a QUANTILE head trained by the pinball loss (SG_LOSS_PINBALL: one more instantiation of the same kernel
 * template; the `_loss` entries above keep refusing kind 3 -- this loss needs Q and the levels).  fc.2 has Q * H output rows, row
 * j = q * H + h being quantile level taus[q] of horizon step h; forecast (optional) and the fc.2 gradients are [B, Q * H, N] /
 * [Q * H, W] / [Q * H].  The target stays [B, H, N]: row j reads target[b, j % H, n], nobody replicates it Q times.  With
 * d = forecast - target and t = taus[j / H]:   l = d >= 0 ? (1 - t) d : -t d ;   dl/dd = 1 - t (d > 0), -t (d < 0), 0 (d == 0);
 * a NaN d on a valid target stays NaN in both.  loss = sum / (B Q H N) = torch.maximum(t (y - f), (t - 1) (y - f)).mean() with y
 * broadcast over q.  norm != NULL (stemgnn_target_valid_count of the [B, H, N] target): a NaN target is missing for all Q of its
 * rows (selected out, never multiplied) and the normaliser is norm[1] / Q; with no valid target the loss and every gradient are
 * exactly 0.  taus: Q floats in HOST memory, read by the call itself and handed to the kernel by value (nothing to allocate or
 * keep alive; a captured step carries them in its kernel node).  Same launch count as the `_loss` entries (rows + finish), the
 * partial-sum kernel is theirs; scratch: stemgnn_fc_tail_train_scratch_floats(B, N, W, Q * H).  `_finish_quantile` needs Q for the
 * loss scale only.  SG_EINVAL (nothing launched) on a NULL pointer other than norm / forecast / loss_accum, B, N, W, H or Q <= 0,
 * Q * H or W outside the fc tail's range (stemgnn_fc_tail_supported(W, Q * H)), or a level that is NaN, <= 0 or >= 1. */
int stemgnn_fc_tail_train_quantile(const float* fsum, const float* target, const float* w0, const float* b0, const float* w2,
                                   const float* b2, int B, int N, int W, int H, int Q, const float* taus, const float* norm,
                                   float* scratch, float* forecast, float* loss, double* loss_accum, float* dfsum, float* dw0,
                                   float* db0, float* dw2, float* db2, void* stream);
int stemgnn_fc_tail_train_rows_quantile(const float* fsum, const float* target, const float* w0, const float* b0,
                                        const float* w2, const float* b2, int B, int N, int W, int H, int Q, const float* taus,
                                        const float* norm, float* scratch, float* forecast, float* dfsum, void* stream);
int stemgnn_fc_tail_train_finish_quantile(const float* scratch, int B, int N, int W, int H, int Q, const float* norm,
                                          float* loss, double* loss_accum, float* dw0, float* db0, float* dw2, float* db2,
                                          void* stream);
/* Zero `bytes` bytes at `ptr` in stream order, as a KERNEL launch (the reference's zero_grad, models/handler.py:160, when it is
 * not fused into the optimizer kernel; control words).  The step path never uses hipMemsetAsync: inside a captured hipGraph
 * a memset node was seen to run into the kernel node that follows it. */
int stemgnn_fill_zero(void* ptr, size_t bytes, void* stream);
/* RMSprop step of the reference driver (models/handler.py:127,165; torch defaults alpha=0.99, momentum 0, not
 * centered) over flat, 16-byte aligned parameter / gradient / square_avg buffers of n floats; lr is read from
 * device memory; zero_grad != 0 also clears the gradients for the next step (handler.py:160); every gradient is
 * multiplied by grad_scale first (1 / world_size after a SUM all-reduce of the flat bucket: no separate averaging pass). */
int stemgnn_rmsprop_step(float* params, float* grads, float* square_avg, size_t n, const float* lr_dev,
                         float alpha, float eps, int zero_grad, float grad_scale, void* stream);

/* Adam step of the driver's other optimizer branch (models/handler.py:128-129; torch defaults weight_decay 0,
 * amsgrad off) over flat buffers of n floats; lr and the step count (step_dev[0], a float, incremented by the call) are
 * read from device memory, so the call is replayable inside a hipGraph; zero_grad / grad_scale as in rmsprop_step. */
int stemgnn_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, const float* lr_dev,
                      float* step_dev, float beta1, float beta2, float eps, int zero_grad, float grad_scale,
                      void* stream);

/* ---- opt-in controls of the two fused optimizers (csrc/optim.hip): gradient-norm clipping, weight decay, non-finite skip.
 * The two entries above stay what the optimizers call when no control is enabled.
 * Number of fp64 partial sums grad_sqsum writes for a bucket of n floats: one per fixed chunk of 8192 floats.  Host only; a
 * function of n alone (never of the device), so the norm is the same bits on any device, eager or replayed. */
size_t stemgnn_grad_norm_partials(size_t n);
/* partials[c] = sum over chunk c of (grads[i] * grad_scale)^2, accumulated in fp64 in a fixed order (no atomics); one
 * launch.  grads 16-byte aligned, any n > 0.  SG_EINVAL (nothing launched) on NULL, n == 0 or a misaligned pointer. */
int stemgnn_grad_sqsum(const float* grads, size_t n, float grad_scale, double* partials, void* stream);
/* rmsprop_step / adam_step with, per element,  g1 = (g * grad_scale) * coef ;  g2 = g1 + weight_decay * p  in front of
 * the unchanged update (torch's order: clip_grad_norm_, then the optimizer adds the L2 term).  Every workgroup sums the
 * stemgnn_grad_norm_partials(n) partials of a grad_sqsum call with the same grad_scale itself, in one fixed order:
 * total = (float)sqrt(sum), coef = min(1, max_norm / (total + 1e-6f)) in fp32 (max_norm <= 0: no clipping, coef = 1).
 * decoupled (Adam only; AdamW): p *= 1 - lr * weight_decay before the update and no decay term in the gradient.
 * skip_nonfinite != 0 and total not finite: parameters, moments and Adam's step count are not written, gradients are
 * still zeroed when zero_grad is set; otherwise NaN propagates as in torch.  partials may be NULL when max_norm <= 0 and
 * skip_nonfinite == 0 (no norm is taken; stats[0] = NaN).  stats = 4 doubles on the device, written by one workgroup:
 * [0] the pre-clip norm of this step, [1] the coefficient applied (1 not clipped, 0 skipped), [2] / [3] running counts of
 * steps with coef < 1 / of skipped steps.  All flat buffers 16-byte aligned; SG_EINVAL (nothing launched) otherwise, on
 * NULL, n == 0, a negative weight_decay, or missing partials.  1 - alpha / 1 - beta are formed as torch forms them (from
 * the decimal the float argument stands for, in fp64, rounded once), so the moments track torch's to fp32 rounding. */
int stemgnn_rmsprop_step_ext(float* params, float* grads, float* square_avg, size_t n, const float* lr_dev, float alpha,
                             float eps, int zero_grad, float grad_scale, float weight_decay, float max_norm,
                             int skip_nonfinite, const double* partials, double* stats, void* stream);
int stemgnn_adam_step_ext(float* params, float* grads, float* exp_avg, float* exp_avg_sq, size_t n, const float* lr_dev,
                          float* step_dev, float beta1, float beta2, float eps, int zero_grad, float grad_scale,
                          float weight_decay, int decoupled, float max_norm, int skip_nonfinite, const double* partials,
                          double* stats, void* stream);

/* ---- data path either side of the hot path ---------------------------------------------
 * normalized() (data_loader/forecast_dataloader.py:7-22): out[t,n] = (float)clip01?((raw[t,n]-sub[n])/div[n]) in IEEE
 * fp64 (z_score: sub=mean, div=std with 0->1; min_max: sub=min, div=max-min+1e-5, clip01=1).  raw [T,N] fp64. */
int stemgnn_normalize_series(const double* raw, const double* sub, const double* div, int clip01, float* out,
                             long T, int N, void* stream);
/* ForecastDataset.__getitem__ + default collate (forecast_dataloader.py:56-63, models/handler.py:136-138,158-159):
 * x[b,w,:] = series[hi[b]-W+w,:], y[b,h,:] = series[hi[b]+h,:]; series [T,N] fp32 resident, hi [B] int64 (device).
 * A window outside [0,T] is written as zeros and sets bit 0 of *status (device int, may be NULL); the other windows of the batch
 * are gathered.  H = 0 is allowed (y is not touched).  B is a grid extent: B > 65535 returns SG_EINVAL, nothing launched (both
 * gathers, their `_pair` forms, stemgnn_roll_window, stemgnn_roll_window_quantile and stemgnn_forecast_store). */
int stemgnn_window_gather(const float* series, const long long* hi, float* x, float* y, int B, int W, int H, int N,
                          long T, int* status, void* stream);
/* The same gather as an ITERATOR over one shuffled epoch (the DataLoader loop of models/handler.py:157-159): order [count]
 * int64 window-end rows (device), queue = device long long[4] {position, 0, count, wrap}, set by the caller when an epoch
 * is loaded (wrap != 0: a position from which no full batch is left goes back to 0 instead of running past the end --
 * start-up replays only).  Every call gathers windows order[position .. position+B) and advances position by B ON THE DEVICE, so a
 * captured hipGraph step needs no per-step index copy.  Row b of a call is window order[position + b] while 0 <= position and
 * position + b < count; a row past the end (or at a negative position) is zeros and sets bit 1 of *status, so a ragged last batch
 * holds its first count - position windows followed by zero rows.  A window of `order` outside [0,T] is zeros + bit 0, as above.
 * The position always moves: to position + B, or with wrap to 0 when position + 2 B > count.  queue[1] is the call's own
 * arrival counter and is 0 again after every call. */
int stemgnn_window_gather_queue(const float* series, const long long* order, long long* queue, float* x, float* y, int B,
                                int W, int H, int N, long T, int* status, void* stream);
/* Both gathers with the y rows taken from a second series of the same shape (x from series_x, y from series_y): the
 * targets of a data set that keeps its missing readings as NaN while the inputs stay imputed.  Same kernels -- the two
 * entries above pass their series twice; for N % 4 == 0 both series must be 16-byte aligned. */
int stemgnn_window_gather_pair(const float* series_x, const float* series_y, const long long* hi, float* x, float* y, int B,
                               int W, int H, int N, long T, int* status, void* stream);
int stemgnn_window_gather_queue_pair(const float* series_x, const float* series_y, const long long* order, long long* queue,
                                     float* x, float* y, int B, int W, int H, int N, long T, int* status, void* stream);
/* nn.MSELoss(reduction='mean') of the driver (models/handler.py:140,162): loss[0] = mean((forecast-target)^2) with
 * a fixed-order two-stage reduction; bwd: dforecast = grad_loss[0] * 2 (forecast-target)/n. */
size_t stemgnn_mse_scratch_floats(void);
int stemgnn_mse_fwd(const float* forecast, const float* target, size_t n, float* scratch, float* loss,
                    double* loss_accum, void* stream);   /* loss_accum (may be NULL): device double, += (double)loss[0] */
int stemgnn_mse_bwd(const float* forecast, const float* target, size_t n, const float* grad_loss, float* dforecast,
                    void* stream);
/* one iteration of the rolling inference (models/handler.py:56-61), out of place: inputs_next = inputs shifted left
 * by L with forecast [B,L,N] appended; forecast_steps[b, step + j, :] = forecast[b,j,:] for j < min(horizon-step, L).
 * Rows of forecast_steps outside [step, step + min(horizon-step, L)) are not written.  L > W (which the reference fails on with a
 * shape error), step outside [0, horizon) or B > 65535 returns SG_EINVAL. */
int stemgnn_roll_window(const float* inputs, const float* forecast, float* inputs_next, float* forecast_steps,
                        int B, int W, int L, int N, int step, int horizon, void* stream);
/* engine.ForecastStep's result slabs: out_forecast / out_target [capacity, H, N] rows pos[0] + b := forecast / target [B, H, N]
 * row b, with pos (int64[1]) read on the device -- the window queue's position before the batch's gather; rows outside
 * [0, capacity) are dropped and no other row of the slabs is written.  B > 65535 or H N > 2^30: SG_EINVAL. */
int stemgnn_forecast_store(const float* forecast, const float* target, const long long* pos, float* out_forecast,
                           float* out_target, int B, int H, int N, long capacity, void* stream);
/* evaluate() (utils/math_utils.py:24-74) with the optional de_normalized() (forecast_dataloader.py:25-38) in front:
 * target / forecast [count,H,N] fp32, v -> v*mul[n] + add[n] in fp64 when mul != NULL (z_score: std, mean; min_max:
 * max-min+1e-8, min).  out (fp64) = overall[3] | by_node[3][N] | by_step[3][H] | by_step_node[3][H][N], each triple
 * (MAPE with its +1e-5 and clip at 5, MAE, RMSE). */
size_t stemgnn_eval_scratch_doubles(long count, int H, int N);
size_t stemgnn_eval_out_doubles(int H, int N);
int stemgnn_eval_metrics(const float* target, const float* forecast, const double* mul, const double* add,
                         long count, int H, int N, double* scratch, double* out, void* stream);
/* The same metrics over the elements whose TARGET is not NaN (missing readings): same per-element formulas, output layout
 * and fixed-order fp64 reduction, plus one plane that counts the elements kept; every mean divides by the valid count of its
 * slice, and a slice with no valid element yields NaN.  Scratch: stemgnn_eval_scratch_doubles_masked (>= the unmasked size). */
size_t stemgnn_eval_scratch_doubles_masked(long count, int H, int N);
int stemgnn_eval_metrics_masked(const float* target, const float* forecast, const double* mul, const double* add,
                                long count, int H, int N, double* scratch, double* out, void* stream);
/* stemgnn_data_plan: how one entry of csrc/data.hip launches for a shape, host only: it launches nothing and reads no buffer.
 * Every launcher of that file takes its geometry from the static function this entry calls for it, so what it reports is what
 * runs; tests use it to prove which thread counts, copy forms, grid-stride passes and chunk counts their cases reach
 * (tests/test_data_cases.py).  `entry` is one of SG_DATA_* and a0..a4 are its shape (unused ones are ignored):
 *   SG_DATA_NORMALIZE (T, N) | SG_DATA_GATHER, SG_DATA_GATHER_QUEUE (B, W, H, N) | SG_DATA_MSE_FWD, SG_DATA_MSE_BWD (n)
 *   SG_DATA_ROLL (B, W, L, N) | SG_DATA_ROLL_QUANTILE (B, W, L, N, Q) | SG_DATA_FORECAST_STORE (B, H, N)
 *   SG_DATA_EVAL (count, H, N; the masked entry launches the same) | SG_DATA_QUANTILE_METRICS (count, Q, H, N; likewise).
 * out = SG_DATA_PLAN_WORDS ints, 0 where a word does not apply:
 *   [0] [1] [2] the grid of the entry's first (or only) launch   [3] its threads per workgroup
 *   [4] the gathers: 1 = float4 copies (N % 4 == 0), 0 = scalar   [5] queue gather: slab rows per workgroup
 *   [6] MSE forward: 0 = one workgroup, 1 = two-stage (partial sums, then one workgroup over them)
 *   [7] normalise, MSE (both), forecast store: trips of the busiest thread through its grid-stride loop
 *   [8] eval and quantile metrics: row chunks of `count` (= grid.y).
 * SG_EINVAL for an unknown entry, out == NULL, or a shape the entry itself refuses (its checks on sizes, not on pointers, T,
 * step, horizon or point). */
enum { SG_DATA_NORMALIZE = 0, SG_DATA_GATHER = 1, SG_DATA_GATHER_QUEUE = 2, SG_DATA_MSE_FWD = 3, SG_DATA_MSE_BWD = 4, SG_DATA_ROLL = 5,
       SG_DATA_ROLL_QUANTILE = 6, SG_DATA_FORECAST_STORE = 7, SG_DATA_EVAL = 8, SG_DATA_QUANTILE_METRICS = 9 };
enum { SG_DATA_PLAN_WORDS = 9 };
int stemgnn_data_plan(int entry, long a0, long a1, long a2, long a3, long a4, int* out /* [SG_DATA_PLAN_WORDS] */);

/* ---- quantile forecasts (a model with Q output rows per horizon step; csrc/data.hip) ---------------------------------
 * stemgnn_roll_window for a quantile forecast [B, Q, L, N]: inputs_next is built from the POINT row (forecast[b, point]) exactly
 * as stemgnn_roll_window builds it, and forecast_steps [B, Q, horizon, N] receives all Q rows:
 * forecast_steps[b, q, step + j, :] = forecast[b, q, j, :] for j < min(horizon - step, L).  The argument checks of
 * stemgnn_roll_window, plus Q > 0 and 0 <= point < Q. */
int stemgnn_roll_window_quantile(const float* inputs, const float* forecast, float* inputs_next, float* forecast_steps, int B,
                                 int W, int L, int N, int Q, int point, int step, int horizon, void* stream);
/* Calibration metrics of a quantile forecast: target [count, H, N], forecast [count, Q, H, N], both fp32; taus = Q doubles in
 * HOST memory (levels in (0, 1), Q <= 32); optional de-normalisation v * mul[n] + add[n] in fp64 ahead of everything else, as in
 * stemgnn_eval_metrics.  One fp64 pass with fixed-order two-level sums (no atomics).  With P = Q / 2 and K = 2 Q + 2 P + 1,
 * out (fp64) = overall[K] | by_step[K][H], where the K statistics are
 *   [0, Q)            mean pinball loss of level q (l as in stemgnn_fc_tail_train_quantile, in fp64)
 *   [Q, 2Q)           empirical coverage of level q: the share of target <= forecast_q
 *   [2Q, 2Q + P)      interval coverage of the pair (i, Q - 1 - i): the share of forecast_i <= target <= forecast_{Q-1-i}
 *   [2Q + P, 2Q + 2P) mean width forecast_{Q-1-i} - forecast_i of that pair
 *   2Q + 2P           crossing rate: the share of elements whose Q forecasts are not non-decreasing in q.
 * `_masked`: an element whose target is NaN is left out everywhere and every mean divides by its slice's valid count; a slice
 * with nothing valid is NaN.  SG_EINVAL (nothing launched) on a NULL pointer other than mul / add, mul without add, count, Q, H
 * or N <= 0, Q > 32, or a level that is NaN, <= 0 or >= 1; the size entries return 0 for such shapes. */
size_t stemgnn_quantile_scratch_doubles(long count, int Q, int H, int N);
size_t stemgnn_quantile_out_doubles(int Q, int H);
int stemgnn_quantile_metrics(const float* target, const float* forecast, const double* taus, const double* mul,
                             const double* add, long count, int Q, int H, int N, double* scratch, double* out, void* stream);
int stemgnn_quantile_metrics_masked(const float* target, const float* forecast, const double* taus, const double* mul,
                                    const double* add, long count, int Q, int H, int N, double* scratch, double* out,
                                    void* stream);

/* ---- conformal calibration of quantile bands (split-conformal CQR; csrc/conformal.hip) -----------
 * target [count, H, N], forecast [count, Q, H, N], fp32 and contiguous; P pairs of rows (lo_rows[p], hi_rows[p]) with nominal
 * coverage coverage[p] in (0, 1).  lo_rows, hi_rows and coverage are P values each in HOST memory, read by the call itself and
 * passed on by value (as the levels of stemgnn_fc_tail_train_quantile are).
 * Score of element (i, h, n) for pair p, in fp32: s = max(f[i, lo, h, n] - y[i, h, n], y[i, h, n] - f[i, hi, h, n]); a NaN
 * score counts as +inf.  masked: an element whose target is NaN is left out and does not count (without it the NaN target
 * gives a NaN score, hence +inf, and counts).
 * Groups: a group keeps its own h if per_step, else pools all H; likewise n and per_node.  offsets (fp32) and counts (int64) are
 * [P, Hg, Ng] with Hg = per_step ? H : 1, Ng = per_node ? N : 1.  counts = m, the group's valid scores.
 * Rank, in fp64: k = max(1, ceil(((m + 1) * coverage) * (1 - 1e-12))) -- two multiplies and a ceil; stemgnn_conformal_rank is
 * that formula on the host, and the device uses the same operations.
 * offsets = the k-th smallest (1-based) of the group's m scores in the total order of fp32 with -0 == +0, +inf if k > m: an
 * exact MSB-first radix select over integer histograms (no sort, no floating-point atomics), so the same bits on every run and
 * whatever the scratch held before.  No host synchronisation, no allocation; 9 launches whatever count and P are.
 * scratch: stemgnn_conformal_scratch_bytes bytes, 16-byte aligned (histograms and per-group state only).
 * SG_EINVAL (nothing launched; the size entry returns 0) on a NULL pointer, count, Q, H, N or P <= 0, Q > 32, P > 16, a pair
 * outside 0 <= lo < hi < Q, a row named twice, a coverage that is NaN, <= 0 or >= 1, or count * H * N >= 2^31; fit alone also
 * on a misaligned scratch and on H > 65535 pooled over the nodes per step. */
long stemgnn_conformal_rank(long m, double coverage);
size_t stemgnn_conformal_scratch_bytes(long count, int H, int N, int P, int per_step, int per_node);
int stemgnn_conformal_fit(const float* target, const float* forecast, long count, int Q, int H, int N, int P,
                          const int* lo_rows, const int* hi_rows, const double* coverage, int per_step, int per_node,
                          int masked, void* scratch, float* offsets, long long* counts, void* stream);
/* out[i, lo_p] = forecast[i, lo_p] - offsets[p, ..], out[i, hi_p] = forecast[i, hi_p] + offsets[p, ..] (one fp32 operation each,
 * the group's offset broadcast over a pooled axis); rows in no pair are copied bit for bit.  out may be forecast itself.  One
 * streaming launch, 16-byte accesses when N % 4 == 0 and both buffers are 16-byte aligned.  The shape and pair checks of fit. */
int stemgnn_conformal_apply(const float* forecast, const float* offsets, long count, int Q, int H, int N, int P,
                            const int* lo_rows, const int* hi_rows, int per_step, int per_node, float* out, void* stream);

/* ---- serving epilogue of a quantile forecast (csrc/quantile_serve.hip) ---------------------------
 * forecast / steps / out are [count or B, Q, H, N], target is [B, H, N], fp32 and contiguous.  A column is the Q values of one
 * (i, h, n).  Finishing a column is two stages, in this order:
 *   a. rearrange != 0: the column's values in non-decreasing order -- torch.sort(dim=1, stable=True) bit for bit: fp32's order
 *      with -0 == +0, NaN above everything (+inf included), ties (NaNs among themselves too) in row order; a selection of the
 *      inputs, so the sign of a zero and a NaN's payload survive.
 *   b. offsets != NULL: stemgnn_conformal_apply on the result of a (same pairs, groups, broadcast and fp32 operation; rows in no
 *      pair untouched).  P, lo_rows and hi_rows are ignored when offsets is NULL.
 * With neither stage both entries are plain copies.
 * finish: out[i] = the finished forecast[i]; out may be forecast itself (a thread reads its whole column before it writes).
 * store:  out_forecast[pos[0] + b] = the finished steps[b] and out_target[pos[0] + b] = target[b], with pos (int64[1]) read on
 *         the device and rows outside [0, capacity) dropped: stemgnn_forecast_store for [capacity, Q, H, N] / [capacity, H, N].
 * One launch each, no scratch, no allocation, no host synchronisation.  16-byte accesses when N % 4 == 0, Q <= 16 and every
 * buffer is 16-byte aligned, a scalar path otherwise (a misaligned view included).
 * SG_EINVAL (nothing launched) on a NULL pointer other than offsets, count / B, Q, H or N <= 0, Q > 32, H * N >= 2^31,
 * capacity <= 0, and -- with offsets -- everything stemgnn_conformal_apply refuses. */
int stemgnn_quantile_finish(const float* forecast, long count, int Q, int H, int N, int rearrange, const float* offsets,
                            int P, const int* lo_rows, const int* hi_rows, int per_step, int per_node, float* out,
                            void* stream);
int stemgnn_quantile_store(const float* steps, const float* target, const long long* pos, int B, int Q, int H, int N,
                           int rearrange, const float* offsets, int P, const int* lo_rows, const int* hi_rows, int per_step,
                           int per_node, float* out_forecast, float* out_target, long capacity, void* stream);

/* ---- seasonal conformal calibration: offsets per time-of-day bucket (csrc/seasonal.hip) -----------
 * Mondrian (category-conditional) split-conformal calibration with a bucket of the target's time as the category.
 * Time: every target has an integer time index t.  Row i of target [count, H, N] / forecast [count, Q, H, N] has an origin o_i,
 * the time index of its step-0 target; step h has t = o_i + h.  o_i = origins[i] (int64 [count] on the device: any order,
 * repeats and gaps allowed, negative values too) or, with origins == NULL, origin0 + i.
 * Bucket: u = (t + phase) mod period in the floor sense (0 <= u < period for negative t too), bucket = (u * K) / period in
 * integer division; period >= 1, 1 <= K <= period, 0 <= phase < period.  stemgnn_season_bucket is that formula on the host
 * (-1 on a bad period / K / phase); the device uses the same integer operations.  The bucket is the TARGET's: step h of row i
 * is scored in, and widened with, bucket(o_i + h), so the steps of one row may fall into different buckets.
 * offsets (fp32) and counts (int64) are [K, P, Hg, Ng], the bucket slowest: slice s is a table of stemgnn_conformal_fit.
 * fit:   within a bucket everything is stemgnn_conformal_fit's definition -- score, NaN -> +inf, masked, the rank, the k-th
 *        smallest in fp32's total order with -0 == +0, +inf when k > m (an empty bucket: count 0, +inf) -- by the same exact
 *        radix select: the same bits on every run, under any permutation of the rows and whatever the scratch held before.
 *        period == K == 1 gives stemgnn_conformal_fit's offsets and counts bit for bit.  No host synchronisation, no
 *        allocation, 9 launches; scratch: stemgnn_seasonal_scratch_bytes bytes, 16-byte aligned, K times the unseasoned one.
 * apply: out[i, lo_p, h, n] = forecast - offsets[bucket(o_i + h), p, ..], out[i, hi_p, h, n] = forecast + ... (one fp32
 *        operation each); rows in no pair are copied bit for bit; out may be forecast itself.  rearrange != 0: the column is
 *        first put in non-decreasing order exactly as stemgnn_quantile_finish does it.  One launch; 16-byte accesses when
 *        N % 4 == 0 and both buffers are 16-byte aligned (with rearrange also Q <= 16).
 * store: stemgnn_quantile_store with the table slice chosen on the device: batch row b has origin t_dev[0] + b (t_dev: the
 *        int64[1] row count of the live ring), step h is widened with slice bucket(t_dev[0] + b + h).  One launch, no scratch.
 * SG_EINVAL (nothing launched; the size entry returns 0) on everything the unseasoned entries refuse, a NULL offsets / t_dev,
 * period < 1 or >= 2^31, K < 1, K > period, phase outside [0, period), P * K > 65535, K * P * Hg * Ng >= 2^29. */
int stemgnn_season_bucket(long long t, long long period, int K, long long phase);
size_t stemgnn_seasonal_scratch_bytes(long count, int H, int N, int P, int K, int per_step, int per_node);
int stemgnn_seasonal_fit(const float* target, const float* forecast, const long long* origins, long long origin0, long count,
                         int Q, int H, int N, int P, const int* lo_rows, const int* hi_rows, const double* coverage,
                         int per_step, int per_node, int masked, long long period, int K, long long phase, void* scratch,
                         float* offsets, long long* counts, void* stream);
int stemgnn_seasonal_apply(const float* forecast, const float* offsets, const long long* origins, long long origin0,
                           long count, int Q, int H, int N, int rearrange, int P, const int* lo_rows, const int* hi_rows,
                           int per_step, int per_node, long long period, int K, long long phase, float* out, void* stream);
int stemgnn_quantile_store_seasonal(const float* steps, const float* target, const long long* pos, const long long* t_dev,
                                    int B, int Q, int H, int N, int rearrange, const float* offsets, int P,
                                    const int* lo_rows, const int* hi_rows, int per_step, int per_node, long long period,
                                    int K, long long phase, float* out_forecast, float* out_target, long capacity,
                                    void* stream);

/* ---- live forecasting: a stream of readings in a device ring (csrc/live.hip) ----------------------
 * A ring is [C, N] fp32: the row with absolute index tau (0 = the first row ever pushed) lives in slot tau mod C.  ring_x holds
 * the imputed, normalised rows (ForecastDataset.data), ring_y the same values with NaN at missing readings
 * (ForecastDataset.target).  t_dev (int64[1], device) is the number of rows pushed so far.
 * push:   raw [K, N] fp64 (device), rows in time order.  Per column n: a reading is missing when it is NaN or
 *         (has_missing && raw == missing); a missing reading is replaced by last[n] (fp64 [N], the column's last valid RAW
 *         reading; the caller sets it to the column's fill value before the first push), a valid one updates last[n].  The value
 *         is normalised as stemgnn_normalize_series does -- (float)clip01?((v - sub[n]) / div[n]), IEEE fp64, one rounding --
 *         and written to ring_x[(t0 + k) mod C]; ring_y gets the same value, or NaN where the reading was missing.  K > C: only
 *         the last C rows are stored, every row still updates last.  Then t_dev[0] = t0 + K: t0 is the HOST's count of the rows
 *         pushed before, nothing reads the old device value.
 * gather: out[b, l, :] = ring[(s_b + l) mod C, :] for l < L, out [B, L, N]; s_b = starts[b] (int64 [B], device), or, with
 *         starts == NULL, t_dev[0] - back with B == 1 (the current window: back = L = W).  A window that starts below 0, reaches
 *         past the rows pushed (s_b + L > t) or into rows already overwritten (s_b < t - C) comes back as NaN rows and sets bit 0
 *         of *status (int32, device; may be NULL).  16-byte accesses when N % 4 == 0 and ring and out are 16-byte aligned, a
 *         scalar path otherwise.
 * head:   pos[0] = t_dev[0] mod history and origins[pos[0]] = t_dev[0] (all int64, device; origins [history]): the position at
 *         which stemgnn_forecast_store / stemgnn_quantile_store file the forecast made now.
 * One launch each, no atomics, no scratch, no allocation, no host synchronisation.
 * SG_EINVAL (nothing launched) on a NULL pointer other than starts / status, K, N, C, B or L <= 0, L > C, back < 0 or > C,
 * t0 < 0, history <= 0, B > 65535, B != 1 without starts, C * N >= 2^31. */
int stemgnn_live_push(const double* raw, int K, int N, long long t0, const double* sub, const double* div, int clip01,
                      double missing, int has_missing, double* last, float* ring_x, float* ring_y, int C, long long* t_dev,
                      void* stream);
int stemgnn_ring_gather(const float* ring, int C, int N, const long long* starts, const long long* t_dev, int back, int B,
                        int L, float* out, int* status, void* stream);
int stemgnn_live_head(const long long* t_dev, long history, long long* pos, long long* origins, void* stream);

/* ---- adaptive conformal inference for live forecasts (Gibbs & Candes 2021; csrc/aci.hip) -----------
 * One call processes ONE matured forecast (one origin) for all P pairs and all groups; pairs and groups are those of
 * stemgnn_conformal_fit (per_step / per_node, state [P, Hg, Ng]).  issued [Q, H, N] = the finished rows that were served,
 * raw [Q, H, N] = the same forecast ahead of calibration, fp32 and contiguous.  The targets are a ring [C, N]: target row h sits
 * in slot (origin + h) mod C (a plain [H, N] tensor is C = H, origin = 0).  lo_rows, hi_rows and target_alpha (= 1 - coverage,
 * in (0, 1)) are P values each in HOST memory, read by the call itself and passed on by value.
 * Device state, owned by the caller and persistent between calls: scores [M, P, H, N] fp32 (NaN = absent; a new window is all
 * NaN), alpha fp64 (initialised to target_alpha[p]), offsets fp32 (the buffer stemgnn_quantile_store reads), counts, miss_sum,
 * valid_sum int64, the last five [P, Hg, Ng].
 * Per pair p and group g, in this order:
 *   1. score: for every (h, n) of the group s = max(raw_lo - y, y - raw_hi) as stemgnn_conformal_fit computes it (fp32, one
 *      rounding each, a NaN from the forecast gives +inf, -0 becomes +0); a NaN target makes the element invalid: its score
 *      slot gets NaN and it counts nowhere.  The origin's scores overwrite slot `slot` (= the host's n_done mod M) of the window.
 *   2. error: valid = the group's valid elements of this origin, miss = those with !(issued_lo <= y && y <= issued_hi) (a NaN
 *      band is a miss, an infinite one covers); miss_sum += miss, valid_sum += valid.
 *   3. level: m = the group's non-NaN scores in the whole window after step 1; counts = m.  If valid == 0 or m < min_scores,
 *      alpha and the offset stay exactly as they are.  Otherwise alpha = alpha + gamma * (target_alpha - miss / valid), four
 *      individually rounded IEEE fp64 operations (divide, subtract, multiply, add; no FMA).  alpha is NOT clamped.
 *   4. offset: c = 1 - alpha.  !(c > 0): -inf (the empty band).  Otherwise k = stemgnn_conformal_rank(m, c); k > m: +inf; else
 *      the k-th smallest of the m scores in the total order of fp32 with -0 == +0: an exact MSB-first radix select, four 8-bit
 *      passes over integer histograms in LDS inside the one launch.  No sort, no floating-point atomics: the same bits on
 *      every run.
 * gamma == 0 is a rolling-window split-conformal refit at the nominal level.  One launch, no scratch, no allocation, no host
 * synchronisation; 16-byte accesses pooled over the nodes when N % 4 == 0 and issued, raw, ring_y and scores are 16-byte aligned.
 * SG_EINVAL (nothing launched) on a NULL pointer, Q, H, N, P, M or C <= 0, Q > 32, P > 16, a pair outside 0 <= lo < hi < Q, a row
 * named twice, gamma NaN or < 0, a target_alpha that is NaN, <= 0 or >= 1, slot outside [0, M), origin < 0, H > C,
 * M * H * N >= 2^31, C * N >= 2^31, min_scores < 0. */
int stemgnn_aci_update(const float* issued, const float* raw, const float* ring_y, int C, long long origin, int Q, int H, int N,
                       int P, const int* lo_rows, const int* hi_rows, const double* target_alpha, double gamma, int M, int slot,
                       long long min_scores, int per_step, int per_node, float* scores, double* alpha, float* offsets,
                       long long* counts, long long* miss_sum, long long* valid_sum, void* stream);

/* ---- conformal anomaly p-values for live readings (csrc/anomaly.hip) ---------------------------------
 * One call judges ONE arrived row `row` (= tau): every stored forecast of it -- step h of origin tau - h, h < H -- is scored and
 * ranked against a rolling window of the scores of earlier rows.
 * slab [S, R, H, N] fp32 is the forecast slab (R rows per forecast: 1 for a point model, Q for a quantile model), origins [S]
 * int64 on the device the origin filed in every slot; ring_y [C, N] the targets, row tau in slot tau mod C, NaN = missing.
 * lo_row == hi_row scores the absolute residual of that row, lo_row < hi_row the band's conformity score.
 * Device state, owned by the caller and persistent between calls: scores [M, H, N] fp32 (NaN = absent; a new window is all
 * NaN), alarm_sum / judged_sum int64 [N] (initialised to 0), log_p [keep, N] fp32.  Written in full by every call: pvalues
 * [H, N] fp32, node_p [N] fp32, alarm [N] int32, counts int64 [H if per_step else 1, N if per_node else 1], row log_slot of log_p,
 * slot `slot` of scores.
 * Per element (h, n), in this order:
 *   1. forecast: o = tau - h, s = o mod S; present iff o >= 0 and origins[s] == o.  origins == NULL: the slab is [1, R, H, N]
 *      (S is not used) and every step is present.  f_lo = slab[s, lo_row, h, n], f_hi = slab[s, hi_row, h, n].
 *   2. score: y = ring_y[tau mod C, n].  A NaN y or an absent forecast makes the element absent: its score slot gets NaN, its
 *      p-value is NaN and it counts nowhere.  Otherwise score = max(f_lo - y, y - f_hi) as stemgnn_conformal_fit computes it
 *      (fp32, one rounding each, a NaN from the forecast gives +inf, -0 becomes +0).
 *   3. population: the group's non-NaN scores in every window slot EXCEPT `slot` (= the host's n_done mod M), i.e. the last
 *      M - 1 judged rows; the group is step h alone with per_step, all H steps without, node n alone with per_node, all nodes
 *      without.  m = its size; counts[g] = m.  (Leaving `slot` out is what makes one pass possible: nothing reads what the call
 *      writes, and a row's own elements are never in its population.)
 *   4. p-value: ge = the population's scores >= score in the total order of fp32 with -0 == +0 and +inf largest;
 *      p = (float)((double)(ge + 1) / (double)(m + 1)), or NaN if m < min_scores.  pvalues[h, n] = p.
 *   5. file: scores[slot, h, n] = score, or NaN when absent.
 * Per node: v = the number of non-NaN p over h, pmin = the smallest; node_p[n] = v ? (float)min(1.0, (double)v * (double)pmin)
 * : NaN (Bonferroni over the opinions about one reading, valid under any dependence between them); alarm[n] = v &&
 * (double)node_p[n] <= alpha; judged_sum[n] += (v > 0); alarm_sum[n] += alarm[n]; log_p[log_slot, n] = node_p[n].
 * work: 2 * H * N uint32 on the device, owned by the caller, ZERO before the first call; every call leaves it zero again.
 * Where a group's window is dealt over several workgroups (pooled over the nodes: up to 64 per group; per_node with H > 4:
 * node tiles x steps x parts of the rows), their integer partial counts -- scores >= the query of (h, n) at [h * N + n], the
 * m of group g at [H * N + g] -- meet there by integer atomic adds; the second launch reads the totals and clears them.
 * per_node with H <= 4 never touches it.
 * Integer counts, integer atomics only, no floating-point atomics: the same bits on every run.  No allocation, no host
 * synchronisation.  Launches: per_node with H <= 4: one; otherwise two (the ranking, then p-values and the per-node
 * combination in one workgroup).  16-byte loads of the window pooled over the nodes when N % 4 == 0 and scores is 16-byte
 * aligned.
 * SG_EINVAL (nothing launched) on a NULL pointer other than origins, S, R, C, H, N, M or keep <= 0, R > 32, rows outside
 * 0 <= lo_row <= hi_row < R, slot outside [0, M), log_slot outside [0, keep), row < 0, alpha NaN or outside (0, 1),
 * min_scores < 0, M * H * N, C * N, S * R * H * N or keep * N >= 2^31. */
int stemgnn_anomaly_update(const float* slab, int S, int R, int lo_row, int hi_row, const long long* origins, long long row,
                           const float* ring_y, int C, int H, int N, int M, int slot, long long min_scores, double alpha,
                           int per_step, int per_node, float* scores, float* pvalues, float* node_p, int* alarm,
                           long long* counts, long long* alarm_sum, long long* judged_sum, float* log_p, int keep, int log_slot,
                           unsigned int* work, void* stream);

/* stemgnn_serving_plan: how one of the four per-arrival serving entries above launches for a shape, host only: it launches
 * nothing and reads no buffer.  The launchers take their geometry from the static functions this entry calls
 * (csrc/serving_plan.h), so what it reports is what runs; tests use it to prove which forms, tiles, trips, parts and batches
 * their cases reach (tests/test_serving_cases.py).  `entry` is one of SG_SERVING_* and a0..a5 are its shape (unused ones are
 * ignored); `misaligned` has one bit per buffer whose address decides the form, set = NOT 16-byte aligned:
 *   SG_SERVING_PUSH (K, N, C), no bits | SG_SERVING_GATHER (C, N, B, L), bit 0 ring, bit 1 out
 *   SG_SERVING_ACI (H, N, P, M, per_step, per_node), bits 0..3 issued, raw, ring_y, scores
 *   SG_SERVING_ANOMALY (H, N, M, per_step, per_node), bit 0 scores.
 * out = SG_SERVING_PLAN_WORDS ints, 0 where a word does not apply:
 *   [0] form: 0 = columns (and push, gather), 1 = stream, 2 = pooled   [1] [2] [3] the grid of the first (or only) launch
 *   [4] its threads per workgroup   [5] VEC: 4 = 16-byte accesses, 1 = scalar, 0 = the form has no choice   [6] launches
 *   push:    [7] k0, the first of the K rows that is stored (K - C when K > C)
 *   gather:  [7] trips of a thread through the copy loop of one row
 *   ACI:     [7] Cc [8] Hr [9] L [10] G (the grouping: columns and rows per slot of the column form, run length and runs of the
 *            stream form)   [11] columns of the last tile   [12] stream: 1 = the window is kept in registers, 0 = streamed
 *            [13] [14] rows one trip of a workgroup covers, on the fullest (first) and on the last tile (stream: elements)
 *            [15] [16] trips of the first row lane through one histogram pass over the window, likewise
 *            [17] [18] its trips through the scoring of the origin, likewise   [19] columns of a full tile (column form)
 *   anomaly: [7] hspan [8] spans [9] rparts [10] node tiles   [11] trips of a row lane over the population's rows
 *            [12] rparts before its clamps (192 / (tiles * spans))   [13] the most parts that still get rows   (both: spans > 1)
 *            [14] pooled: parts   [15] batches of queries   [16] [17] the last batch's queries and their power of two
 *            [18] L [19] G (pooled)   [20] nodes of a full tile   [21] row lanes of a workgroup (both: column form).
 * SG_EINVAL for an unknown entry, out == NULL, a bit that names no buffer, or a shape the entry itself refuses (its checks on the
 * sizes given here, not on pointers, C of the target ring, S, R, keep or the slots). */
enum { SG_SERVING_PUSH = 0, SG_SERVING_GATHER = 1, SG_SERVING_ACI = 2, SG_SERVING_ANOMALY = 3 };
enum { SG_SERVING_PLAN_WORDS = 22 };
int stemgnn_serving_plan(int entry, long a0, long a1, long a2, long a3, long a4, long a5, int misaligned,
                         int* out /* [SG_SERVING_PLAN_WORDS] */);

/* stemgnn_calibration_plan: how the batch side of the conformal family launches for a shape -- stemgnn_conformal_fit / _apply,
 * stemgnn_seasonal_fit / _apply and the column kernel behind stemgnn_quantile_finish / _store, stemgnn_seasonal_apply with
 * rearrange and stemgnn_quantile_store_seasonal -- host only: it launches nothing and reads no buffer.  The launchers take their
 * geometry from the static functions this entry calls (csrc/calibration_plan.h) with the compute-unit count this entry reports,
 * so what it reports is what runs; tests use it to prove which forms, tiles, chunks, trips, thread counts and column blocks their
 * cases reach (tests/test_calibration_cases.py).  `entry` is one of SG_CALIBRATION_*, `shape` its nshape values in HOST memory
 * (nshape must be the entry's own number); `misaligned` has one bit per buffer whose address decides a form, set = NOT 16-byte
 * aligned:
 *   SG_CALIBRATION_FIT            (count, H, N, P, per_step, per_node), no bits
 *   SG_CALIBRATION_SEASONAL_FIT   (count, H, N, P, per_step, per_node, period, K, has_origins), no bits; has_origins != 0: the
 *                                 origins are a tensor, not origin0 + i
 *   SG_CALIBRATION_APPLY          (count, Q, H, N), bit 0 forecast, bit 1 out
 *   SG_CALIBRATION_SEASONAL_APPLY (count, Q, H, N), the same bits; rearrange == 0 (with rearrange: SG_CALIBRATION_COLUMN)
 *   SG_CALIBRATION_COLUMN         (count or B, Q, H, N, rearrange, store), bit 0 src (forecast / steps), bit 1 dst (out /
 *                                 out_forecast) and, store != 0 only, bit 2 target, bit 3 out_target.
 * out = SG_CALIBRATION_PLAN_WORDS ints, 0 where a word does not apply:
 *   [0] form: 0 = columns (and the applies, the column kernel), 1 = stream   [1] [2] [3] the grid of the first launch (the fit:
 *   of a histogram launch)   [4] its threads per workgroup   [5] VEC: 4 = 16-byte accesses, 1 = scalar, 0 = no choice
 *   [6] the compute units the caps below were worked out with (stemgnn_num_cus())
 *   fit, seasonal fit:
 *     [7] KP, the tables (P, or K * P)   [8] groups of a table   [9] Cc [10] Hr [11] L [12] G (the grouping: columns and rows per
 *     window of the column form, run length and runs of the stream form)
 *     [13] column tiles   [14] columns of the last tile   [15] [16] rows a wave covers per trip (rpw = 64 / width) on the first
 *     and on the last tile   [17] columns of a full tile   ([13] .. [17]: column form)
 *     [18] chunks chosen   [19] rows (stream: elements) per chunk   [20] what set [18]: 0 = the blocks wanted ([22]), 1 = the
 *     rows / elements ([23]), 2 = the 65535 of grid.y; the first of them in this order that gives the minimum
 *     [21] trips of the first row lane of the first tile (stream: of thread 0) through chunk 0
 *     [22] ceil([24] / (tiles * KP)) (stream: / (KP * groups))   [23] ceil([27] / 64) (stream: / 1024)
 *     [24] histogram workgroups aimed at: 4 per compute unit   [25] workgroups of the pick launch, a wave per (table, group)
 *     [26] waves of the last pick workgroup that have none   [27] the rows (stream: elements) [23] divides: count * Hr
 *     (count * L), or with DIRECT the virtual rows of the longest bucket in place of count
 *     [28] seasonal: 1 = DIRECT (a bucket's rows are enumerated), 0 = skipping   [29] why: 0 = DIRECT, 1 = an origins tensor,
 *     2 = K == 1, 3 = 2 * walk > count; -1 without a season   [30] runs = count / period + 2   [31] walk = runs * ceil(period / K)
 *   apply, seasonal apply:
 *     [7] workgroups that give every item a thread (seasonal: every (window, step) segment a wave) of its own
 *     [8] the cap, 8 per compute unit   [9] 1 = the cap set the grid   [10] trips of thread 0 over the items (seasonal: of wave 0
 *     over the segments)   [11] seasonal: trips of lane 0 over a segment's items   [12] seasonal: those items, Q * N / VEC
 *   column kernel ([4] = T):
 *     [7] LDS bytes   [8] planes (2 with rearrange)   [9] cpb [10] wpb: a workgroup holds wpb windows of cpb column groups
 *     [11] threads with neither, T - cpb * wpb   [12] column blocks   [13] columns of the last column block
 *     [14] window blocks   [15] 1 = their cap (16 per compute unit / [12]) set [14]   [16] trips of a workgroup's first window
 *     lane over the windows   [17] store: 4 = the target is copied by float4, 1 = by scalar; 0 = not a store
 *     [18] store: trips of target workgroup 0 over the batch's windows   [19] column groups (of VEC columns) per window.
 * SG_EINVAL for an unknown entry, out == NULL, shape == NULL, an nshape that is not the entry's, a negative value, a bit that
 * names no buffer of the entry, or a shape the entry itself refuses (its checks on the sizes given here, not on pointers, pairs,
 * coverages, phase or capacity; the column kernel: those of stemgnn_quantile_finish without offsets). */
enum { SG_CALIBRATION_FIT = 0, SG_CALIBRATION_SEASONAL_FIT = 1, SG_CALIBRATION_APPLY = 2, SG_CALIBRATION_SEASONAL_APPLY = 3,
       SG_CALIBRATION_COLUMN = 4 };
enum { SG_CALIBRATION_PLAN_WORDS = 32 };
int stemgnn_calibration_plan(int entry, const long* shape, int nshape, int misaligned,
                             int* out /* [SG_CALIBRATION_PLAN_WORDS] */);

/* ---- scenario forecasts: sampled rolling paths and their order statistics (csrc/scenario.hip) --------
 * roll:  one round of a roll that feeds SAMPLED rows back instead of the point row, for Bo origins x S paths.  inputs
 *        [Bsrc, W, N], forecast [Bsrc, Q, L, N], fp32 and contiguous; taus = the Q levels as fp32 in HOST memory, read by the call
 *        itself and passed on by value.  Path p = b * S + s reads source row p / fan: fan == S is round 0 (Bsrc == Bo, the model
 *        ran once per origin), fan == 1 a later round (Bsrc == Bo * S).  For every path, step j < L and node n:
 *          1. v_(0) <= .. <= v_(Q-1): the column forecast[src, :, j, n] in the order of stemgnn_quantile_finish's rearrange
 *             (-0 == +0, NaN last, ties in row order; a selection, bit patterns kept).
 *          2. u = ((w >> 9) + 0.5f) * 2^-23, exact in fp32 and strictly inside (0, 1); w is a Philox4x32-10 word under key
 *             seed with `offset` as the counter's high 64 bits.  coupling == SG_SCENARIO_INDEPENDENT: word n & 3 of counter
 *             ((((origin0 + b) * S + s) * horizon + (step + j)) * ceil(N / 4) + (n >> 2)) (64-bit, wrapping).
 *             SG_SCENARIO_PATH: word 0 of the counter of (j = 0, n = 0), for every j and n of the round.
 *          3. i = the largest index in [0, Q - 2] with taus[i] <= u, 0 when there is none.
 *          4. wt = (u - taus[i]) / (taus[i + 1] - taus[i]), two fp32 subtractions and one correctly rounded division;
 *             tails == SG_SCENARIO_CLAMP clamps wt to [0, 1], SG_SCENARIO_LINEAR extends the outermost segments.
 *          5. y = v_(i) + (v_(i+1) - v_(i)) * wt, the subtraction, the product and the sum rounded separately (no FMA).
 *        NaN and infinite values follow from this arithmetic.  Outputs: paths[b, s, step + j, n] = y for j < min(L, horizon -
 *        step) (paths [Bo, S, horizon, N]); inputs_next [Bo * S, W, N] (may be NULL: the last round) = the window of
 *        stemgnn_roll_window with y where that takes the forecast row; bands [Bo, Q, horizon, N] (round 0 only, else NULL):
 *        bands[b, :, step + j, n] = the model's own column, unsorted, bit for bit.
 * bands: bands[b, q, h, n] = the ranks[q]-th smallest (1-based) of the S values paths[b, :, h, n] in the same order, for every
 *        h >= step_from; the steps below step_from are not written.  ranks = Q ints in HOST memory, passed on by value.
 * rank:  k = min(S, max(1, ceil((tau * S) * (1 - 1e-12)))) in fp64 -- two multiplies and a ceil -- on the host.
 * One launch each, no scratch, no atomics, no allocation, no host synchronisation.  roll uses 16-byte accesses when N % 4 == 0
 * and every buffer is 16-byte aligned, a scalar path otherwise.
 * SG_EINVAL (nothing launched): a NULL pointer other than inputs_next / bands of roll; Bo, W, L, N <= 0, L > W, step outside
 * [0, horizon), inputs_next == inputs; Q < 2 or Q > 32 (bands: Q < 1); levels not strictly increasing inside (0, 1); S outside
 * [1, 1024]; fan not in {1, S}; bands with fan != S; an unknown coupling / tails; Bo * S, W * N, Q * L * N, Q * horizon * N or
 * S * horizon >= 2^31; bands: step_from outside [0, horizon], a rank outside [1, S], horizon * N >= 2^31. */
#define SG_SCENARIO_INDEPENDENT 0
#define SG_SCENARIO_PATH 1
#define SG_SCENARIO_LINEAR 0
#define SG_SCENARIO_CLAMP 1
long stemgnn_scenario_rank(double tau, long S);
int stemgnn_scenario_roll(const float* inputs, const float* forecast, const float* taus, int Bo, int S, int fan, int W, int L,
                          int N, int Q, int step, int horizon, long long origin0, unsigned long long seed,
                          unsigned long long offset, int coupling, int tails, float* inputs_next, float* paths, float* bands,
                          void* stream);
int stemgnn_scenario_bands(const float* paths, int Bo, int S, int horizon, int N, int Q, const int* ranks, int step_from,
                           float* bands, void* stream);
/* roll_given: stemgnn_scenario_roll with step 2 replaced by u = uniforms[b, s, j, n] (uniforms [Bo, S, L, N], fp32 and
 * contiguous, on the device): the same kernel with a third source for u, so steps 1 and 3 to 5, the outputs and every refusal
 * above hold as they stand (coupling, seed, offset and origin0 do not exist here; uniforms == NULL is refused too).  The 16-byte
 * path also needs uniforms 16-byte aligned.  A value outside (0, 1) or a NaN follows from the arithmetic of steps 3 to 5;
 * keeping u inside is the caller's contract (stemgnn_copula_uniforms does; antithetic or user-defined dependence may not). */
int stemgnn_scenario_roll_given(const float* inputs, const float* forecast, const float* taus, const float* uniforms, int Bo,
                                int S, int fan, int W, int L, int N, int Q, int step, int horizon, int tails, float* inputs_next,
                                float* paths, float* bands, void* stream);

/* ---- Gaussian-copula coupling of scenario paths (csrc/copula.hip) ---------------------------------------
 * The marginals stay the model's quantile functions; the uniforms of one (path, step) row are u_n = Phi(z_n), z = L e with e
 * i.i.d. N(0, 1) and L L^T = R a correlation matrix over the nodes, estimated from the normal scores of held-out targets.
 * pit:      u[c, h, n] = F(target[c, h, n]), F the quantile function of stemgnn_scenario_roll's steps 1 and 3 to 5 read the other
 *           way.  target [count, H, N], forecast [count, Q, H, N], u [count, H, N], fp32 and contiguous; taus = the Q levels as
 *           fp32 in HOST memory.  With v_(0) <= .. <= v_(Q-1) the column in that order and y the target:
 *             i  = the largest index in [0, Q - 2] with v_(i) <= y, 0 when there is none
 *             d  = v_(i+1) - v_(i);  wt = (y - v_(i)) / d, fp32, a correctly rounded division;
 *                  where d == 0: wt = 0.5 when y == v_(i), else +inf / -inf by the sign of y - v_(i)
 *             tails == SG_SCENARIO_CLAMP clamps wt to [0, 1]
 *             u  = taus[i] + (taus[i + 1] - taus[i]) * wt, the subtraction, the product and the sum rounded separately (no FMA),
 *                  then clamped to [2^-24, 1 - 2^-24].
 *           Both clamps are comparisons that keep a NaN.  A NaN target or a NaN anywhere in the column gives u = NaN (bits
 *           0x7fc00000), "missing"; an infinite column value follows from the arithmetic.  One launch; 16-byte accesses when
 *           N % 4 == 0 and target, forecast and u are 16-byte aligned, a scalar path otherwise.
 * gram:     u [M, N] fp32 (M = count * H rows); z = normcdfinv((double)u) in fp64, a NaN z (a NaN u, a u outside [0, 1]) is
 *           absent.  For every (i, j), over the rows where z_i and z_j are both present:
 *             pairs[i, j] = their number (int64, exact)
 *             sums[0][i, j] = sum z_i z_j    sums[1][i, j] = sum z_i    sums[2][i, j] = sum z_i^2     (fp64 [3][N][N])
 *           Two launches: rows in chunks of 1024 added in row order, then the chunks in chunk order; no atomics, the same bits on
 *           every run.  scratch: stemgnn_copula_scratch_doubles(M, N) doubles on the device (0 for a refused shape).
 * uniforms: u [Bo, S, Lsteps, N] fp32.  factor_t [N, N] fp32, factor_t[k * N + n] = L[n][k], L lower triangular; the entries
 *           with k > n are never used.  For path (b, s), step j < Lsteps and node k:
 *             e_k = normcdfinvf(((w >> 9) + 0.5f) * 2^-23), w the Philox word of stemgnn_scenario_roll's step 2 under
 *                   SG_SCENARIO_INDEPENDENT for (origin0 + b, s, step + j, k): a draw is named by global origin, path, step, node
 *             z_n = sum_{k <= n} L[n][k] * e_k, fp32 FMAs with k ascending from 0 (the order depends on n alone)
 *             u_n = normcdff(z_n) clamped to [2^-24, 1 - 2^-24].
 *           One launch, no scratch.  N <= 2048 (the rows of e a workgroup holds: 16 up to N = 512, 4 beyond).
 * No allocation, no host synchronisation, no atomics; capturable.
 * SG_EINVAL (nothing launched): a NULL pointer; count, H, N, M, Bo, Lsteps <= 0; Q < 2 or Q > 32; levels not strictly increasing
 * inside (0, 1); an unknown tails; S outside [1, 1024]; step outside [0, horizon); uniforms: N > 2048; pit: H * N, Q * H * N,
 * count * H or the grid ceil(count * H * (N / VEC) / threads) >= 2^31; gram: M, N * N or the grid ceil(N / 16)^2 *
 * ceil(M / 1024) >= 2^31; uniforms: Bo * S * Lsteps or S * horizon >= 2^31. */
int stemgnn_copula_pit(const float* target, const float* forecast, const float* taus, long count, int H, int N, int Q, int tails,
                       float* u, void* stream);
size_t stemgnn_copula_scratch_doubles(long M, int N);
int stemgnn_copula_gram(const float* u, long M, int N, double* scratch, long long* pairs, double* sums, void* stream);
int stemgnn_copula_uniforms(const float* factor_t, int Bo, int S, int Lsteps, int N, int step, int horizon, long long origin0,
                            unsigned long long seed, unsigned long long offset, float* u, void* stream);
/* uniforms_steps: the same with the steps of one round coupled as well, a separable Gaussian copula
 * over (step, node): the normal scores of a path's round have correlation T[j][j'] * R[n][n'].  step_factor [Lsteps, Lsteps]
 * fp32 row-major, step_factor[j * Lsteps + i] = A[j][i], A the lower Cholesky factor of T; the entries with i > j are never
 * read.  For path (b, s):
 *   e[j][k] = the e_k of stemgnn_copula_uniforms for (origin0 + b, s, step + j, k): the same Philox word, the same counter map
 *   g[j][k] = sum_{i <= j} A[j][i] * e[i][k], fp32 FMAs with i ascending from 0, the sum starting at 0.f
 *   z[j][n] = sum_{k <= n} L[n][k] * g[j][k], in stemgnn_copula_uniforms' order
 *   u[b, s, j, n] = normcdff(z[j][n]) clamped to [2^-24, 1 - 2^-24].
 * With A the identity the result is stemgnn_copula_uniforms', bit for bit.  A workgroup owns whole paths: Lsteps <= 16 for
 * N <= 512 and Lsteps <= 4 for 512 < N <= 2048; anything else, a NULL step_factor and whatever stemgnn_copula_uniforms refuses
 * is SG_EINVAL with nothing launched.  One launch, no scratch, no atomics; capturable. */
int stemgnn_copula_uniforms_steps(const float* factor_t, const float* step_factor, int Bo, int S, int Lsteps, int N, int step,
                                  int horizon, long long origin0, unsigned long long seed, unsigned long long offset, float* u,
                                  void* stream);

/* ---- ensemble scores of scenario paths: CRPS, energy score, rank histogram (csrc/ensemble.hip) --------
 * target [count, H, N] and paths [count, S, H, N] (stemgnn_scenario_roll's layout), fp32 and contiguous, 1 <= S <= 1024; optional
 * de-normalisation v * mul[n] + add[n] in fp64 ahead of everything else, as in stemgnn_eval_metrics (mul > 0 is the caller's
 * contract).  All arithmetic is fp64 from the fp32 inputs.  D = S^2, or S (S - 1) with fair != 0 (the estimator that is unbiased
 * in S; needs S >= 2).
 * Per element (c, h, n), with x_s = paths[c, s, h, n] and y = target[c, h, n]:
 *   crps = (1 / S) sum_s |x_s - y| - (1 / (2 D)) sum_s sum_s' |x_s - x_s'|
 *   mean = (1 / S) sum_s x_s;  se = (mean - y)^2;  var = sum_s (x_s - mean)^2 / (S - 1), NaN when S == 1
 *   rank = #{s : x_s < y} + #{s : x_s == y} / 2 (integer division), compared on the raw fp32 values (-0 == +0; a NaN path
 *          value is in neither set), so 0 <= rank <= S.
 * Per row (c, h), over its node set V (every n; `_masked`: those whose target is not NaN):
 *   energy = (1 / S) sum_s ||x_s - y|| - (1 / (2 D)) sum_s sum_s' ||x_s - x_s'||, Euclidean norms over n in V of the
 *            de-normalised values; a pair distance is sqrt(sum_n (x_sn - x_s'n)^2), formed from the differences.
 * out (fp64) = overall[6] | by_step[6][H]:
 *   0 mean crps over the valid elements     1 mean energy over the valid rows
 *   2 sqrt(mean se), the RMSE of the ensemble mean     3 sqrt(mean var), the spread ([3] / [2] near 1: spread matches skill)
 *   4 the number of valid elements          5 the number of valid rows
 * hist (int64 [H][S + 1]) = the count of every rank per step over the valid elements; the call zeroes it itself.
 * Plain entry: every element and row is valid; a NaN target makes the statistics of its slices NaN and is left out of hist (it
 * has no rank).  `_masked`: a NaN target is missing: left out of [0], [2], [3], [4], hist and the V of its row; a row with empty
 * V is left out of [1] and [5]; a slice with nothing valid is NaN in [0..3].  Both: a NaN path value on a valid target
 * propagates.
 * Fixed-order two-level fp64 sums; integer atomics for hist only, no floating-point atomics: the same bits on every run.  No
 * allocation, no host synchronisation, three launches.  scratch: stemgnn_ensemble_scratch_doubles doubles on the device.
 * SG_EINVAL (nothing launched) on a NULL pointer other than mul / add, mul without add, count, S, H or N <= 0, S > 1024, fair
 * with S < 2, or one of the kernels' int products >= 2^31: the two grids count * H * ceil(N / C) (C the node tile, 4 .. 64) and
 * count * H * T (T + 1) / 2 (T = ceil(S / 32)), H * (S + 1), S * H * N; the size entries return 0 for such shapes. */
size_t stemgnn_ensemble_scratch_doubles(long count, int S, int H, int N);
size_t stemgnn_ensemble_out_doubles(int H);
int stemgnn_ensemble_scores(const float* target, const float* paths, const double* mul, const double* add, long count, int S,
                            int H, int N, int fair, double* scratch, double* out, long long* hist, void* stream);
int stemgnn_ensemble_scores_masked(const float* target, const float* paths, const double* mul, const double* add, long count,
                                   int S, int H, int N, int fair, double* scratch, double* out, long long* hist, void* stream);

/* ---- scenario events: aggregates over node sets and crossing counts of sampled paths (csrc/events.hip) --
 * De-normalisation, both entries: v = (double)x * mul[j] + add[j] in fp64, the product and the sum rounded separately (as in
 * stemgnn_ensemble_scores), j the node (aggregate) or the column (events); mul == add == NULL: v = (double)x.
 * aggregate: x [rows, N] fp32 and contiguous (paths: rows = count * S * H; targets: rows = count * H), weights [R, N] fp64 on the
 *            device, out [rows, R] fp32:
 *              out[row, r] = (float) sum over the nodes n with weights[r, n] != 0 of weights[r, n] * v_n
 *            accumulated in fp64 (fused multiply-adds) in an order that depends on N and R alone, never on the row or on rows: a
 *            pass computed batch by batch is the whole pass bit for bit.  A node whose weight is exactly 0 is not part of the
 *            sum (a NaN there does not reach the group); a NaN inside a group propagates.  16-byte loads when N % 4 == 0 and x is
 *            16-byte aligned, a scalar path otherwise.  R <= 32, N <= 4096.
 * events:    paths [count, S, H, M] fp32 and contiguous (M: the node axis or an aggregated group axis), thr [M] fp64 on the
 *            device, counts int32 [count, 2 H + 1, M].  E(s, h) = v > thr[m] when above == 1, v < thr[m] when above == 0, strict
 *            fp64 comparisons: a NaN value or threshold is never in the event.  For origin c and column m:
 *              counts[c, h, m]      = #{s : E(s, h)}                                            h < H   ("step")
 *              counts[c, H + h, m]  = #{s : E(s, h) and no E(s, h') for h' < h}                 h < H   ("first")
 *              counts[c, 2 H, m]    = #{s : the longest run of consecutive steps with E is >= min_run}  ("run")
 *            A NaN breaks a run and is not a crossing.  Integers only: exact.  1 <= S <= 1024, 1 <= H <= 256.
 * One launch each; no allocation, no host synchronisation, no memset, no global atomics (integer LDS adds in events only): the
 * same bits on every run, capturable.
 * SG_EINVAL (nothing launched): a NULL pointer other than mul / add; mul without add (or add without mul);
 * aggregate: rows, N or R <= 0, R > 32, N > 4096, rows * R >= 2^31 (the grid is min(ceil(rows / 4), 2048));
 * events: count, S, H or M <= 0, S > 1024, H > 256, min_run outside [1, H], above not 0 / 1, S * H * M, (2 H + 1) * M or the
 * grid count * ceil(M / C) >= 2^31 (C the column tile, 1 .. 64). */
int stemgnn_scenario_aggregate(const float* x, const double* weights, const double* mul, const double* add, long long rows,
                               int N, int R, float* out, void* stream);
int stemgnn_scenario_events(const float* paths, const double* thr, const double* mul, const double* add, long count, int S,
                            int H, int M, int above, int min_run, int* counts, void* stream);

/* ---- scenario reduction: K representative paths with weights, by forward selection (csrc/reduce.hip) ---
 * distances: paths [count, S, L] fp32 and contiguous, a path's trajectory flattened (L = H * M); scale [L] fp64 on the device or
 *            NULL (all ones); D [count, S, S] fp64:
 *              D[c, i, j] = sqrt( sum_l (((double)x_il - (double)x_jl) * scale_l)^2 ),  l = 0, 1, .. L - 1 in that order
 *            each difference formed first, then multiplied by scale_l, then accumulated by one fp64 fused multiply-add; with
 *            squared != 0 there is no square root.  The sum is over DIFFERENCES, never |x|^2 + |x'|^2 - 2 x.x': two coincident
 *            paths are at exactly 0 (paths of coupling = "path" nearly coincide).  The upper triangle is computed and stored
 *            twice: D[c, i, j] and D[c, j, i] are the same bits, and the diagonal of a finite path is +0.  Nothing is masked: a
 *            NaN or an infinity in a path reaches its row and its column, the diagonal included, as the arithmetic gives it.
 *            One launch, one workgroup per (origin, 32 x 32 tile of pairs on or above the diagonal).
 * reduce:    D [count, S, S] fp64, from the entry above or any cost of the caller's: D[k, u] is the cost of moving path k onto
 *            path u; symmetry is neither needed nor checked.  Per origin, with m_k = +inf, for pick i = 0 .. K - 1:
 *              z_u         = sum_k min(m_k, D[k, u]),  k = 0, 1, .. S - 1 in that order, one fp64 add after the other
 *              selected[i] = the u not yet selected with the smallest z_u, the lowest index among equals
 *              cost[i]     = z_u / S: the Kantorovich distance between the uniform ensemble and the kept set with optimally
 *                            redistributed weights
 *              m_k         = min(m_k, D[k, selected[i]])
 *            and after the last pick assign[k] = the position j in 0 .. K - 1 of the kept path nearest to k (D[k, selected[j]]
 *            smallest; among equals the one selected earliest) and counts[j] = #{k : assign[k] = j}: the weights are
 *            counts / S, and the counts add up to S.  selected, counts int32 [count, K]; assign int32 [count, S]; cost fp64
 *            [count, K].  An origin whose D holds an entry that is not a finite number >= 0 is refused: its selected and assign
 *            are -1, its counts 0, its cost NaN; the other origins of the call are not affected.
 *            One launch, one workgroup per origin; D is held in LDS where S (S | 1) doubles fit 160 KiB (S <= 141).
 * Both: no floating-point atomics, no allocation, no host synchronisation; the same bits on every run, and an origin's results do
 * not depend on which other origins share the call.
 * SG_EINVAL (nothing launched): a NULL pointer other than scale; count or S <= 0; S > 1024; count * S * S >= 2^31;
 * distances: L <= 0, squared not 0 / 1, S * L or the grid count * T (T + 1) / 2 (T = ceil(S / 32)) >= 2^31;
 * reduce: K < 1 or K > S. */
int stemgnn_scenario_distances(const float* paths, const double* scale, long count, int S, int L, int squared, double* D,
                               void* stream);
int stemgnn_scenario_reduce(const double* D, long count, int S, int K, int* selected, int* counts, int* assign, double* cost,
                            void* stream);

/* ---- weighted scenario sets: bands, scores, event counts and a further reduction of kept paths (csrc/weighted.hip, DESIGN.md
 * section 5t) ---------------------------------------------------------------------------------------------------------------
 * A set is K members per origin with integer multiplicities mult int32 [count, K] (a ScenarioSet's counts): member k stands
 * mult[c, k] times in an ensemble of W paths, 1 <= W <= 2^24, so every product w w' and W^2 is exact in fp64.  K <= 256 for
 * bands, scores and events.  A member of multiplicity 0 is not read: a NaN there reaches nothing.  An origin is ABSENT when one
 * of its multiplicities is negative or they do not add up to W (a refused origin of stemgnn_scenario_reduce has counts 0); an
 * absent origin does not affect any other.
 * bands:  paths [count, K, H, N], bands [count, Q, H, N] fp32; ranks = Q ints in HOST memory (stemgnn_scenario_rank(tau, W)),
 *         passed on by value.  bands[c, q, h, n] = the first value, in the order of stemgnn_scenario_bands (-0 == +0, NaN last,
 *         stable in k), whose cumulative multiplicity reaches ranks[q]: what stemgnn_scenario_bands returns for the W paths in
 *         which member k stands mult[c, k] times in a row, bit for bit.  An absent origin is NaN (0x7fc00000) everywhere.  One
 *         launch; 16-byte accesses when N % 4 == 0 and paths and bands are 16-byte aligned, a scalar path otherwise.
 * scores: the definitions of stemgnn_ensemble_scores (`masked` != 0: of stemgnn_ensemble_scores_masked) with w_k = mult[c, k]:
 *           crps = (1 / W) sum_k w_k |x_k - y| - (1 / (2 D)) sum_k sum_k' w_k w_k' |x_k - x_k'|,  D = W^2 or W (W - 1) with fair
 *           mean = (1 / W) sum_k w_k x_k;  var = sum_k w_k (x_k - mean)^2 / (W - 1), NaN when W == 1
 *           rank = sum{w_k : x_k < y} + (sum{w_k : x_k == y}) / 2 (integer division), on the raw fp32 values
 *           energy: the same with Euclidean norms over the row's node set, formed from differences
 *         out (fp64) = overall[7] | by_step[7][H]: slots 0 .. 5 as in stemgnn_ensemble_scores over the present origins, slot 6 the
 *         number of absent origins (the same number in every by-step slot).  hist int64 [H][W + 1]; the call zeroes it itself.
 *         De-normalisation, masking and NaN propagation as there.  Fixed-order two-level fp64 sums, integer atomics for hist
 *         only (a row's ranks meet in LDS first where W + 1 <= 4096); three launches.  scratch: stemgnn_weighted_scratch_doubles doubles on the device.
 * events: paths [count, K, H, M], counts int32 [count, 2 H + 1, M]: the three counts of stemgnn_scenario_events with every
 *         member counted mult[c, k] times -- exact integers, equal to that entry's on the replicated ensemble.  An absent
 *         origin is -1 everywhere.  One launch.  H <= 256.
 * reduce_weighted: the forward selection of stemgnn_scenario_reduce on an ensemble of S members with probabilities
 *         mult_in[c, k] / W (mult_in int32 [count, S], S <= 1024).  With p_k = (double)mult_in[c, k]:
 *           z_u = sum_k p_k * min(m_k, D[k, u]) over the k with p_k > 0 in index order, the product and the add rounded
 *                 separately (no FMA);  cost[i] = z_u / W;  counts[j] = the sum of mult_in[k] over the members assigned to j
 *         A member of multiplicity 0 is no candidate, has assign = -1, and its row and column of D are not read.  Refused as
 *         there (-1 / 0 / -1 / NaN), also when the origin is absent or K exceeds the number of members of positive multiplicity.
 *         With mult_in all ones and W == S every output equals stemgnn_scenario_reduce's bit for bit.  One launch; D in LDS
 *         where it fits (S <= 141).
 * All: no allocation, no host synchronisation, no memset, no floating-point atomics; the same bits on every run, and an origin's
 * results do not depend on which other origins share the call; capturable.
 * SG_EINVAL (nothing launched): a NULL pointer other than mul / add; mul without add; count, K, S, H, N, M or Q <= 0; K > 256;
 * Q > 32; S > 1024; W outside [1, 2^24]; a rank outside [1, W]; fair with W < 2; events: H > 256, min_run outside [1, H], above
 * not 0 / 1; reduce_weighted: K outside [1, S]; an int product >= 2^31: count, count * H, H * N, K * H * N (K * H * M), Q * H * N,
 * (2 H + 1) * M, H * (W + 1), count * S * S, or a grid (bands: count * ceil(H N / C); scores: count * H * T (T + 1) / 2,
 * T = ceil(K / 32); events: count * ceil(M / C)); the size entries return 0 for such shapes. */
int stemgnn_weighted_bands(const float* paths, const int* mult, long count, int K, int H, int N, int W, int Q, const int* ranks,
                           float* bands, void* stream);
size_t stemgnn_weighted_scratch_doubles(long count, int K, int H, int N);
size_t stemgnn_weighted_out_doubles(int H);
int stemgnn_weighted_scores(const float* target, const float* paths, const int* mult, const double* mul, const double* add,
                            long count, int K, int H, int N, int W, int fair, int masked, double* scratch, double* out,
                            long long* hist, void* stream);
int stemgnn_weighted_events(const float* paths, const int* mult, const double* thr, const double* mul, const double* add,
                            long count, int K, int H, int M, int W, int above, int min_run, int* counts, void* stream);
int stemgnn_scenario_reduce_weighted(const double* D, const int* mult_in, long count, int S, int K, int W, int* selected,
                                     int* counts, int* assign, double* cost, void* stream);

/* ---- scenario trees: staged forward selection of sampled paths (csrc/tree.hip) -----------------------
 * Paths x [count, S, H, M] fp32 and contiguous.  bounds = T ints in HOST memory, 0 < b_1 < b_2 < .. < b_T = H, passed on by
 * value: stage t = 1 .. T owns the steps [b_{t-1}, b_t), b_0 = 0.  nodes = T ints in HOST memory, 1 <= n_1 <= .. <= n_T <= S,
 * passed on by value.  mult_in int32 [count, S] with common total W, or NULL: all ones and W = S; the conventions are those
 * of the weighted sets above (1 <= W <= 2^24; an origin with a negative multiplicity or a wrong sum is absent).  T <= 16.
 * stage_distances: D [count, T, S, S] fp64, prefix form.  With scale [H * M] fp64 on the device or NULL (all ones):
 *              Q_t[i, j] = sum over the columns (h, m) of stage t, in order, of (((double)x_i - (double)x_j) * scale)^2
 *            the difference formed first, then multiplied by the scale, then accumulated by one fp64 fused multiply-add;
 *              D_t^2 = ((Q_1 + Q_2) + ..) + Q_t, summed in stage order;   D_t = sqrt(D_t^2), or D_t^2 itself with squared != 0
 *            DIFFERENCES, never the Gram expansion: D_t[i, j] and D_t[j, i] are the same bits, a finite path is at exactly +0
 *            from itself, and a NaN or an infinity reaches its row and its column from its stage on and not before.  A
 *            stage's own sum is kept as four partial sums: the stage's columns are walked in chunks of 64 counted from the
 *            stage's first column, chunk c adding into sum c % 4, joined as ((s0 + s1) + s2) + s3 -- a function of M and the
 *            bounds alone.  One launch that reads the paths once and stores all T tiles; one workgroup per (origin, 32 x 32
 *            tile of pairs on or above the diagonal), of 256 threads or, where the grid leaves compute units idle, of 1024 (a
 *            wave group per partial sum): the same bits either way.
 * tree:      D [count, T, S, S] fp64, from the entry above or any cost of the caller's (D_t[k, u]: moving member k onto member
 *            u in the metric of stage t; symmetry is neither needed nor checked).  Per origin, with p_k = (double)mult_in[k];
 *            a member with p_k = 0 is never a candidate, is never read and keeps assign = -1 (the LIVE members are the others):
 *              par_0(k) = 0 for all k.  For stage t = 1 .. T: m_k = +inf, then n_t picks, node i of the stage the i-th pick:
 *              phase A, i = 0 .. n_{t-1} - 1 (n_0 = 1), one child for every parent in parent order: the candidates are the
 *                unselected u with par_{t-1}(u) = i;  z_u = sum over the k with par_{t-1}(k) = i, in index order, of
 *                p_k * D_t[k, u], the product and the add rounded separately (no FMA); the pick u* is the smallest z_u, the
 *                lowest index among equals; then m_k = D_t[k, u*] for the k of that parent.  A parent without members (its
 *                representative coincides with an earlier pick's, which took every member) has no candidate: that child is
 *                EMPTY, node_path = -1, node_parent = i, node_count = 0, and nothing else changes.
 *              phase B, i = n_{t-1} .. n_t - 1: the candidates are every unselected live u;  z_u = sum over all live k, in
 *                index order, of p_k * min(m_k, E[k, u]),  E[k, u] = D_t[k, u] where par_{t-1}(k) = par_{t-1}(u), +inf
 *                elsewhere (a path is only ever moved onto a path of its own parent); pick and ties as in phase A; then
 *                m_k = min(m_k, D_t[k, u*]) for the k of u*'s parent.
 *              after the stage's last pick: assign_t[k] = the node of stage t whose representative is nearest to k among the
 *                nodes with k's parent, among equals the earliest pick;  par_t = assign_t;  node_path[t, i] = the pick;
 *                node_parent[t, i] = par_{t-1}(pick), so node_parent[t, i] = i for i < n_{t-1};  node_count[t, i] = the sum of
 *                mult_in over the members assigned to i;  cost[t] = (sum over live k, in index order, of p_k * m_k) / W, the
 *                product and the add rounded separately: the Kantorovich distance, in the stage's prefix metric, between the
 *                ensemble and the stage's nodes under the tree constraint.
 *            With T = 1 every output equals stemgnn_scenario_reduce_weighted's bit for bit (node_path = selected, node_count =
 *            counts, assign, cost[0] = its cost[K - 1]); with mult_in = NULL, stemgnn_scenario_reduce's.
 *            Refused origin (node_path = node_parent = -1, node_count = 0, assign = -1, cost = NaN, ALL stages): the origin is
 *            absent; n_T exceeds the members of positive multiplicity; an entry of any stage between two live members is not a
 *            finite number >= 0.  The other origins of the call are not affected.
 *            Outputs, padded to n_T per stage: node_path, node_parent, node_count int32 [count, T, n_T] with -1 / -1 / 0 beyond
 *            n_t; assign int32 [count, T, S]; cost fp64 [count, T].  One launch, one workgroup per origin; a stage's D_t is held
 *            in LDS where it fits (S <= 141), beyond that rows are read from memory.
 * Both: no allocation, no host synchronisation, no memset, no floating-point atomics; the same bits on every run, and an
 * origin's results do not depend on which other origins share the call; capturable.
 * SG_EINVAL (nothing launched): a NULL pointer other than scale / mult_in; count, S, H, M or T <= 0; S > 1024; T > 16; bounds
 * not strictly increasing from above 0 or not ending at H; nodes decreasing or outside [1, S]; W outside [1, 2^24], or W != S
 * with mult_in NULL; squared not 0 / 1; count, count * T * S * S, S * H * M or the grid count * P (P + 1) / 2 (P = ceil(S / 32))
 * >= 2^31. */
int stemgnn_scenario_stage_distances(const float* paths, const double* scale, long count, int S, int H, int M, int T,
                                     const int* bounds, int squared, double* D, void* stream);
int stemgnn_scenario_tree(const double* D, const int* mult_in, long count, int S, int T, const int* nodes, int W, int* node_path,
                          int* node_parent, int* node_count, int* assign, double* cost, void* stream);

/* ---- simultaneous scenario bands: the studentised sup-norm envelope of sampled paths (csrc/envelope.hip, DESIGN.md section
 * 5v) --------------------------------------------------------------------------------------------------------------------------
 * paths [count, S, H, C] fp32 and contiguous (C: nodes, or the groups of stemgnn_scenario_aggregate).  mult int32 [count, S]
 * with common sum `total`, or NULL: all ones (total is then not looked at).  The conventions are those of the weighted sets
 * above: w_s = mult[c, s], T = total (without mult: w_s = 1, T = S); a member of weight 0 is never read.  Per (origin c, column
 * n), all in fp64, every sum over s ascending, every product and every sum rounded on its own (no FMA):
 *   centre   m_h = (sum_s w_s x[s, h]) / T
 *   scale    s_h = sqrt((sum_s w_s (x[s, h] - m_h)^2) / T): the square rounded, then its product with w_s, then the add; the
 *            division and the root correctly rounded.      moments[c, 0, h, n] = m_h, moments[c, 1, h, n] = s_h
 *   depth    d_s = max_h |x[s, h] - m_h| / s_h, a step with s_h == 0 contributing 0;  depth[c, s, n] = d_s, NaN for a member
 *            of weight 0 (depth may be NULL)
 *   chosen   with k = the rank of stemgnn_conformal_rank(T, coverage): the smallest d_s whose members j with d_j <= d_s carry
 *            weight at least k; +inf when k > T.  It is the multiplier that holds `coverage` of the ensemble's own paths.
 *   q        chosen[c, n] when multiplier is NULL, else multiplier[multiplier_n == 1 ? 0 : n] (fp64, on the device)
 *   bands    bands[c, 0, h, n] = (float)(m_h - q s_h), bands[c, 1, h, n] = (float)(m_h + q s_h); q = +inf: -inf / +inf
 *            whatever s_h is
 *   truth    with target [count, H, C] fp32: truth[c, n] = max_h |y_h - m_h| / s_h; where s_h == 0 the term is 0 if y_h == m_h
 *            and +inf otherwise.  ignore_nan != 0: NaN steps of the target are skipped, NaN when every step is NaN;
 *            ignore_nan == 0: NaN when any step is.  The band with multiplier q holds the whole target exactly when
 *            truth <= q.  target and truth are both given or both NULL.
 * ABSENT: a column with a non-finite value in a path of positive weight; every column of an origin whose weights are negative
 * or do not sum to total.  An absent column is NaN in every output; no other column is affected.
 * One launch, one workgroup per (origin, tile of 32 .. 4 columns); the tile's S * H values are held in LDS where they fit (64 KB
 * with the depths and moments), so `paths` is read once, else read from memory by every phase; 16-byte loads when C % 4 == 0 and
 * paths is 16-byte aligned, scalar ones otherwise.  No allocation, no host synchronisation, no memset, no atomics; the same
 * bits on every run, and an origin's results do not depend on which other origins share the call; capturable.
 * SG_EINVAL (nothing launched): paths, moments, chosen or bands NULL; one of target / truth without the other; S outside
 * [1, 1024]; H outside [1, 256]; count or C <= 0; coverage not inside (0, 1) (NaN included); multiplier given with multiplier_n
 * neither 1 nor C; mult given with total outside [1, 2^24]; count * S * C, count * H * C or S * H * C >= 2^31. */
int stemgnn_scenario_envelope(const float* paths, const int* mult, int total, const float* target, int ignore_nan,
                              const double* multiplier, int multiplier_n, int count, int S, int H, int C, double coverage,
                              double* moments, double* depth, double* chosen, double* truth, float* bands, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* STEMGNN_HIP_H */
