"""GPU: the StockBlock stage (csrc/block.hip, glu_fused.h, glu_fused_bf16.h, heads.h, wgrad.h, pack.hip, gemm*.h) through the
C ABI against fp64, one case per launch-path decision -- the block's counterpart of tests/test_hip_front.py.

BLOCK_CASES is (B, N, W, multi); tests/test_block_cases.py proves on the CPU that the list reaches both values of every SG_PATH_*
bit of stemgnn_block_paths (exact fp32 and bf16x2), both answers of stemgnn_glu_fused_bf16_ok, both sides of M mod 32 / 64 / 96,
and shapes with CP > C, CP2[r] > U[r], WmP > Wm and nf[1] = 0.

Inputs (seeded fp32 draws): X = randn(B, N, W); mul_L = cheb_polynomial(L) for L = I - (A + A^T) / (2 N), A = rand(N, N), as in
test_stock_block_layer_standalone; the 33 parameters from oracle.det_state_dict; upstream gradients wf = randn (forecast) and an
independent wb = randn (backcast): the loss is sum(forecast * wf) + sum(backcast * wb), so block 0's backcast gradient is not the
one an MSE loss leaves.

Hygiene: packed, split, saved, scratch, gradpart, the inference workspace, forecast, backcast, dX, dmul_L and every parameter
gradient are NaN before each call and sized exactly by their stemgnn_*_floats function; every buffer, the inputs' guarded copies
included, carries a guard band of 256 floats that must read back unchanged after each call; `saved` and `packed` must have the
bits after the backward they had before it; the whole forward + backward of a case is repeated on re-poisoned buffers (same bits).

Reference: oracle.stemgnn_oracle.stock_block with autograd in fp64 on the device, on the same fp32 values, for forecast,
backcast, dX, dmul_L[1..3] and the 33 parameter gradients (each under its own norm).  The intermediates (G, the useful columns of
out[r][l] / gate[r][l], ig, fs in `saved`; dpF, dpB, dig and dG = the sum of its two slabs in `scratch`) come from
_traced_block, the same expressions line by line with the intermediates kept, whose forecast / backcast must equal
stock_block's.  Where the reference gradient is identically zero (the dead C2R bins of GLUs.4 / GLUs.5, the order-0 columns of
GLUs.0 / GLUs.1, the f = 0 sine column) the kernel's must be exactly zero.

Forms: both arithmetics (splits 0: stemgnn_block_pack, _spectral_glu_fwd, _spectral_glu_bwd parts 1, _block_wgrad; splits 2:
_block_pack_panels, _glu_split_panels, _fwd_split, _dgrad_split, _block_wgrad_split), both input layouts of X on every case
([B,W,N] read in place and [B,N,W]; compared with each other within the bound), both backcast states (has_backcast 0: backcast /
dbackcast NULL, parameters 5, 6 NULL, guarded gradient buffers for 7, 8 come back all NaN), accumulate = 1 of the heads forward,
parts 1 then 2 against 3 of the two backward entries (no bits promised: both within the bound, the test prints whether the
bits matched), stemgnn_block_wgrad against the parts & 2 slab path, cu_percent 100 / 10, nsplit 1 / 3 / 32, STEMGNN_GLU_FUSED
0..3 (forward: same bits in every setting; the 64- and 96-row data-gradient chains: same bits; each setting against fp64 on its
own), _block_pack_panels + _glu_fused_repack against _block_pack (bits), the warm-up launch, the inference entries (bits of the
training forward).

Tolerances.  Hard bar: relerr < 1e-4 (max-norm relative, tests/util.relerr) against fp64 for both arithmetics (BASELINE.json).
Rounding-class bar: with e_ref the relerr of torch's fp32 evaluation of the same oracle functions against the fp64 run,
e_kernel <= K * max(e_ref, floor); floor = 2^-22 for exact fp32 and 2^-16 for bf16x2 (the per-product error include/stemgnn_hip.h
states for splits == 2).  Why a factor at all: the kernels sum on MFMA trees and in split-M partials where torch sums in its own
order, and the DFT / C2R tables are folded into the weights (one more rounding per folded weight).

K = 4 in both arithmetics: the worst ratio e_kernel / max(e_ref, floor) measured on an MI355X (256 CUs) over the 21 cases and every
form above is 3.33 in exact fp32 and 2.44 in bf16x2, rounded up to the next power of two.  Worst ratio per quantity, the case and
form that gave it (bc1 / bc0: with / without the backcast heads; bnw / bwn: X as [B,N,W] / [B,W,N]; "block cu10": stemgnn_block_wgrad
at cu_percent 10; FUSED=: STEMGNN_GLU_FUSED; out[r][l] / gate[r][l] and d GLUs.*: the worst over the branches / the six GLUs and
their two sides):

exact fp32 (splits 0), floor 2^-22:
    quantity                     ratio   case (B, N, W, multi)   form                     e_kernel   e_ref
    forecast                      2.54   (2, 6, 64, 5)           bc1 bnw                  1.01e-06   3.98e-07
    backcast                      0.42   (3, 43, 12, 5)          bc1 bnw                  1.00e-07   1.25e-07
    G                             1.00   (1, 31, 12, 5)          bc1 bnw                  2.44e-07   2.44e-07
    out[r][0]                     0.35   (1, 2, 2, 1)            bc1 bnw                  8.30e-08   7.55e-08
    gate[r][0]                    0.36   (2, 3, 1, 3)            bc1 bnw                  8.61e-08   5.94e-08
    out[r][1]                     0.54   (3, 20, 7, 3)           bc1 bnw                  3.93e-07   7.34e-07
    gate[r][1]                    0.42   (2, 3, 1, 3)            bc1 bnw                  9.97e-08   9.97e-08
    out[r][2]                     0.58   (2, 3, 1, 3)            bc1 bnw                  1.38e-07   1.38e-07
    gate[r][2]                    0.40   (3, 20, 7, 3)           bc1 bnw                  1.36e-07   3.39e-07
    ig                            0.55   (2, 3, 1, 3)            bc1 bnw                  1.30e-07   8.08e-08
    fs                            0.49   (1, 97, 12, 5)          bc1 bnw                  1.19e-07   2.42e-07
    dpF                           1.55   (2, 7, 64, 9)           bc1 bnw                  3.70e-07   1.39e-07
    dpB                           0.89   (3, 5, 64, 1)           bc1 bnw                  2.13e-07   1.89e-07
    dig                           3.33   (2, 7, 64, 9)           bc0 bnw                  8.89e-07   2.67e-07
    dG                            1.70   (1, 1, 1, 1)            bc1 bnw                  4.06e-07   2.26e-07
    dX                            1.40   (2, 3, 1, 3)            bc0 bnw                  3.34e-07   1.28e-07
    dmul_L                        2.74   (1, 2, 2, 1)            splits 0 FUSED=0         6.53e-07   1.48e-07
    d weight                      1.17   (2, 3, 1, 3)            bc1 bnw                  2.80e-07   1.27e-07
    d forecast.weight             0.73   (1, 2, 2, 1)            bc1 bnw                  1.74e-07   1.54e-07
    d forecast.bias               2.62   (3, 43, 12, 5)          bc1 bnw                  6.24e-07   1.63e-07
    d forecast_result.weight      3.18   (3, 43, 12, 5)          bc1 bnw                  7.59e-07   2.08e-07
    d forecast_result.bias        1.90   (8, 12, 12, 5)          bc1 bnw                  4.54e-07   1.40e-07
    d backcast.weight             1.71   (2, 3, 1, 3)            bc1 bnw                  4.08e-07   6.27e-08
    d backcast.bias               1.59   (4, 228, 12, 5)         block cu10 nsplit32      3.79e-07   1.19e-07
    d backcast_short_cut.weight   1.02   (3, 5, 64, 1)           bc1 bnw                  2.44e-07   1.52e-07
    d backcast_short_cut.bias     0.78   (2, 7, 64, 9)           bc1 bnw                  1.86e-07   1.89e-07
    d GLUs.*.weight               2.00   (2, 3, 1, 3)            bc0 bnw                  4.97e-07   2.48e-07
    d GLUs.*.bias                 1.97   (2, 3, 1, 3)            splits 0 FUSED=0         4.70e-07   1.53e-07

bf16x2 (splits 2), floor 2^-16:
    quantity                     ratio   case (B, N, W, multi)   form                     e_kernel   e_ref
    forecast                      0.07   (2, 6, 64, 5)           bc1 bnw                  1.10e-06   3.98e-07
    backcast                      0.03   (3, 5, 64, 1)           bc1 bnw                  4.78e-07   4.59e-07
    G                             0.04   (4, 228, 12, 5)         bc1 bnw                  6.10e-07   8.29e-07
    out[r][0]                     0.69   (3, 11, 12, 5)          bc1 bnw                  1.05e-05   2.01e-06
    gate[r][0]                    1.22   (8, 8, 12, 5)           bc1 bnw                  1.86e-05   5.04e-06
    out[r][1]                     0.71   (5, 19, 12, 5)          bc1 bnw                  1.09e-05   4.14e-06
    gate[r][1]                    0.87   (3, 5, 64, 1)           bc1 bnw                  1.67e-05   1.92e-05
    out[r][2]                     1.02   (3, 20, 7, 3)           bc1 bnw                  1.56e-05   1.19e-06
    gate[r][2]                    0.54   (2, 5, 64, 11)          bc1 bnw                  8.24e-06   7.57e-06
    ig                            0.88   (8, 8, 12, 5)           bc1 bnw                  1.34e-05   7.52e-06
    fs                            0.04   (3, 5, 64, 1)           bc1 bnw                  6.70e-07   6.47e-07
    dpF                           0.02   (2, 7, 64, 9)           bc1 bnw                  3.70e-07   1.39e-07
    dpB                           0.04   (1, 2, 2, 1)            bc1 bnw                  5.86e-07   9.05e-08
    dig                           0.06   (2, 5, 64, 11)          bc0 bnw                  8.64e-07   3.05e-07
    dG                            1.02   (3, 5, 64, 1)           bc1 bnw                  1.55e-05   1.45e-05
    dX                            0.84   (3, 20, 7, 3)           bc0 bnw                  1.28e-05   1.93e-06
    dmul_L                        1.06   (7, 9, 12, 5)           bc1 bnw                  1.62e-05   7.12e-06
    d weight                      0.79   (8, 8, 12, 5)           bc1 bnw                  1.20e-05   1.10e-05
    d forecast.weight             1.03   (8, 12, 12, 5)          bc1 bnw                  1.57e-05   7.49e-06
    d forecast.bias               0.36   (1, 31, 12, 5)          splits 2 FUSED=0         5.49e-06   1.53e-07
    d forecast_result.weight      0.83   (1, 31, 12, 5)          bc1 bnw                  1.26e-05   2.19e-07
    d forecast_result.bias        0.20   (4, 228, 12, 5)         bc1 bnw                  2.98e-06   1.65e-07
    d backcast.weight             0.93   (1, 31, 12, 5)          splits 2 FUSED=0         1.42e-05   8.40e-06
    d backcast.bias               0.23   (3, 11, 12, 5)          bc1 bnw                  3.51e-06   9.30e-08
    d backcast_short_cut.weight   0.02   (1, 2, 2, 1)            bc1 bnw                  3.14e-07   7.26e-08
    d backcast_short_cut.bias     0.02   (1, 2, 2, 1)            bc1 bnw                  2.59e-07   4.81e-08
    d GLUs.*.weight               2.44   (1, 2, 2, 1)            bc0 bnw                  3.72e-05   6.26e-07
    d GLUs.*.bias                 1.53   (8, 12, 12, 5)          bc1 bnw                  2.33e-05   9.66e-06

(dig, the largest in fp32: the per-stage heads backward of (2, 7, 64, 9) sums W multi + W = 640 products per element on the MFMA
tree.  d GLUs.*.weight in bf16x2: at (1, 2, 2, 1) e_ref is 6e-7 and the floor decides.  The two layouts of X gave the same bits in
every case and quantity: ratio 0.  Nothing needs more than 4.)
"""
import ctypes
import functools
import math

import pytest
import torch

from tests.util import DEV, SENTINEL, _all_nan, _bits, _Buf, _relerr, dims, l2_channels, saved_layout, scratch_layout

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = {0: 4, 2: 4}                         # per arithmetic (splits): the measured worst ratio, rounded up (the table above)
FLOOR = {0: 2.0 ** -22, 2: 2.0 ** -16}
NSPLIT = 32                              # ops.py's _NSPLIT
NPARAMS = 33

M_SWEEP = [(1, 31), (4, 8), (3, 11), (7, 9), (8, 8), (5, 13), (5, 19), (8, 12), (1, 97), (3, 43)]     # M = 31 .. 129 at W 12, multi 5
BLOCK_CASES = [
    # (B, N, W, multi)
    (1, 1, 1, 1), (1, 2, 2, 1), (2, 3, 1, 3),      # Wm <= 3: no imaginary bins, slab weight gradients, 4-wave heads backward
    (3, 5, 64, 1),                                 # CP = 256: the fused forward's limit; per-layer data-gradient chain (3 W > 64)
    (1, 17, 13, 5),                                # CP = 272: just past it
    (2, 6, 64, 5),                                 # long K, per-stage heads forward, fused heads backward
    (4, 40, 64, 3),                                # KF = 784
    (2, 7, 64, 9), (2, 5, 64, 11),                 # per-stage heads backward: by the LDS limit, by the Wm limit
] + [(B, N, 12, 5) for B, N in M_SWEEP] + [
    (3, 20, 7, 3),                                 # CP <= 128: the data-gradient chain with nt = 1
    (4, 228, 12, 5),                               # PEMS07 anchor
]
PARAM_NAMES = (["weight", "forecast.weight", "forecast.bias", "forecast_result.weight", "forecast_result.bias", "backcast.weight",
                "backcast.bias", "backcast_short_cut.weight", "backcast_short_cut.bias"]
               + [f"GLUs.{g}.linear_{side}.{wb}" for g in range(6) for side in ("left", "right") for wb in ("weight", "bias")])


def _ids(cases):
    return ["-".join(f"{k}{v}" for k, v in zip("BNWm", c)) for c in cases]


# ---- inputs and the reference ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _draws(case):
    from oracle import stemgnn_oracle as O

    B, N, W, multi = case
    g = torch.Generator().manual_seed(7919 * B + 104729 * N + 31 * W + multi)
    X = torch.randn(B, N, W, generator=g)
    A = torch.rand(N, N, generator=g)
    L = torch.eye(N) - 0.5 * (A + A.T) / N
    sd = O.det_state_dict(N, W, multi, 1, seed=11 + W + multi, stack_cnt=1)
    params = [sd["stock_block.0." + k].contiguous() for k in PARAM_NAMES]
    return dict(X=X, mul_L=O.cheb_polynomial(L).contiguous(), params=params, wf=torch.randn(B, N, W, generator=g),
                wb=torch.randn(B, N, W, generator=g), old=torch.randn(B, N, W, generator=g))


def _traced_block(X, mul_L, sd, s):
    """oracle.stock_block with spe_seq_cell's device branch inlined, expression by expression, keeping the intermediates"""
    import torch.nn.functional as F

    p = f"stock_block.{s}."
    B, _, N, W = X.shape
    t = {}
    gfted = torch.matmul(mul_L.unsqueeze(1), X.unsqueeze(1))
    t["gfted"] = gfted
    x = gfted.reshape(B, -1, N, W)
    tt = torch.arange(W, dtype=x.dtype, device=x.device)
    ang = 2.0 * math.pi * torch.outer(tt, tt) / W
    ff_real, ff_imag = x @ torch.cos(ang), -(x @ torch.sin(ang))
    br = [ff_real.permute(0, 2, 1, 3).reshape(B, N, -1), ff_imag.permute(0, 2, 1, 3).reshape(B, N, -1)]
    for i in range(3):
        for r in range(2):
            pre = p + f"GLUs.{2 * i + r}."
            left = F.linear(br[r], sd[pre + "linear_left.weight"], sd[pre + "linear_left.bias"])
            gate = torch.sigmoid(F.linear(br[r], sd[pre + "linear_right.weight"], sd[pre + "linear_right.bias"]))
            br[r] = left * gate
            t[f"out{r}{i}"], t[f"gate{r}{i}"] = br[r], gate
    real = br[0].reshape(B, N, 4, -1).permute(0, 2, 1, 3)
    img = br[1].reshape(B, N, 4, -1).permute(0, 2, 1, 3)
    n = real.shape[-1]
    h = n // 2
    f = torch.arange(h + 1, dtype=x.dtype, device=x.device)
    tau = torch.arange(n, dtype=x.dtype, device=x.device)
    ang = 2.0 * math.pi * torch.outer(f, tau) / n
    c = torch.full((h + 1,), 2.0, dtype=x.dtype, device=x.device)
    c[0] = 1.0
    sfac = c.clone()
    sfac[0] = 0.0
    if n % 2 == 0:
        c[h] = 1.0
        sfac[h] = 0.0
    gconv_input = ((real[..., : h + 1] @ (c[:, None] * torch.cos(ang)) - img[..., : h + 1] @ (sfac[:, None] * torch.sin(ang))) / n).unsqueeze(2)
    igfted = torch.matmul(gconv_input, sd[p + "weight"]).sum(dim=1)
    preF = F.linear(igfted, sd[p + "forecast.weight"], sd[p + "forecast.bias"]).squeeze(1)
    fsrc = torch.sigmoid(preF)
    forecast = F.linear(fsrc, sd[p + "forecast_result.weight"], sd[p + "forecast_result.bias"])
    t.update(ig=igfted, preF=preF, fs=fsrc)
    back = None
    if s == 0:
        short = F.linear(X, sd[p + "backcast_short_cut.weight"], sd[p + "backcast_short_cut.bias"])
        preB = F.linear(igfted, sd[p + "backcast.weight"], sd[p + "backcast.bias"]) - short
        back = torch.sigmoid(preB)
        t["preB"] = preB
    return forecast, back, t


def _evaluate(case, has_bc, dt):
    """every compared quantity in `dt` on the device: outputs and gradients by oracle.stock_block, intermediates by _traced_block"""
    from oracle import stemgnn_oracle as O

    B, N, W, multi = case
    d, dr = dims(*case), _draws(case)
    s = 0 if has_bc else 1
    wf, wb = dr["wf"].to(DEV, dt), dr["wb"].to(DEV, dt)

    def leaves():
        leaf = lambda v: v.to(DEV, dt, copy=True).requires_grad_(True)
        sd = {f"stock_block.{s}.{k}": leaf(v) for i, (k, v) in enumerate(zip(PARAM_NAMES, dr["params"])) if has_bc or i not in (5, 6)}
        return leaf(dr["X"].unsqueeze(1)), leaf(dr["mul_L"]), sd

    def loss(fo, bc):
        return (fo * wf).sum() + ((bc.squeeze(1) * wb).sum() if bc is not None else 0.0)

    X, mul_L, sd = leaves()
    fo, bc = O.stock_block(X, mul_L, sd, s)
    assert (bc is not None) == bool(has_bc)
    loss(fo, bc).backward()
    r = dict(forecast=fo.detach().reshape(d.M, W), dX=X.grad.reshape(d.M, W), dmul_L=mul_L.grad[1:])
    if has_bc:
        r["backcast"] = bc.detach().reshape(d.M, W)
    for i, k in enumerate(PARAM_NAMES):
        g = sd.get(f"stock_block.{s}.{k}")
        r["d " + k] = None if g is None or g.grad is None else g.grad
    assert [k for k in PARAM_NAMES if r["d " + k] is None] == ([] if has_bc else PARAM_NAMES[5:9]), "which gradients the oracle leaves None"
    del X, mul_L, sd
    X, mul_L, sd = leaves()
    fo2, bc2, t = _traced_block(X, mul_L, sd, s)
    tie = 1e-12 if dt == torch.float64 else 1e-5
    assert _relerr(fo2.detach().reshape(d.M, W), r["forecast"]) < tie and (bc2 is None or _relerr(bc2.detach().reshape(d.M, W), r["backcast"]) < tie), \
        "_traced_block is not oracle.stock_block"
    keep = ["gfted", "ig", "preF"] + (["preB"] if has_bc else [])
    for k in keep:
        t[k].retain_grad()
    loss(fo2, bc2).backward()
    r["G"] = t["gfted"].detach()[:, 1:4, 0].permute(0, 2, 1, 3).reshape(d.M, d.KG)
    r["dG"] = t["gfted"].grad[:, 1:4, 0].permute(0, 2, 1, 3).reshape(d.M, d.KG)
    for rr in range(2):
        idx = torch.tensor(l2_channels(d, rr), dtype=torch.long, device=DEV)
        for l in range(3):
            for q in ("out", "gate"):
                v = t[f"{q}{rr}{l}"].detach().reshape(d.M, d.C)
                r[f"{q}{rr}{l}"] = v if l < 2 else v[:, idx]
    r["ig"], r["fs"] = t["ig"].detach().reshape(d.M, d.Wm), t["fs"].detach().reshape(d.M, d.Wm)
    r["dig"], r["dpF"] = t["ig"].grad.reshape(d.M, d.Wm), t["preF"].grad.reshape(d.M, d.Wm)
    if has_bc:
        r["dpB"] = t["preB"].grad.reshape(d.M, W)
    return r


@functools.lru_cache(maxsize=None)
def _reference(case, has_bc):
    return _evaluate(case, has_bc, torch.float64), _evaluate(case, has_bc, torch.float32)


FWD_Q = ["forecast", "backcast", "G"] + [f"{q}{r}{l}" for r in range(2) for l in range(3) for q in ("out", "gate")] + ["ig", "fs"]
DATA_Q = ["dpF", "dpB", "dig", "dG"]
GRAD_Q = ["dX", "dmul_L"] + ["d " + k for k in PARAM_NAMES]


def _rows(got, ref, names, tag=""):
    """(quantity, e_kernel, e_ref) per name present on both sides; exact zeros where the reference is identically zero"""
    r64, r32 = ref
    rows = []
    for q in names:
        if r64.get(q) is None or r64[q].numel() == 0:          # what the reference lacks: None gradients, backcast without its head,
            continue                                           # the imaginary branch's last layer at nf[1] = 0
        assert q in got, f"{tag}{q}: the harness returned no such quantity"
        g = got[q].reshape(r64[q].shape)
        dead = (r64[q] == 0) & (r32[q] == 0)
        assert bool((g[dead] == 0).all()), f"{tag}{q}: not exactly zero where the reference gradient is identically zero"
        rows.append((tag + q, _relerr(g, r64[q]), _relerr(r32[q], r64[q])))
    return rows


def _judge(title, rows, splits):
    """Prints every figure, then asserts both bars."""
    k, floor = K[splits], FLOOR[splits]
    ratio = lambda r: (r[1] / max(r[2], floor)) if r[1] == r[1] else float("inf")
    worst = max(rows, key=ratio)
    print(f"{title}: worst ratio {ratio(worst):.2f} ({worst[0]}: e_kernel {worst[1]:.2e}, e_ref {worst[2]:.2e})")
    for r in rows:
        print(f"    {r[0]:44s} e_kernel {r[1]:.2e} e_ref {r[2]:.2e} ratio {ratio(r):.2f}")
    bad = [r for r in rows if not (r[1] < TOL and r[1] <= k * max(r[2], floor))]
    assert not bad, bad


# ---- the harness ------------------------------------------------------------------------------------------------------------------
class _Block:
    """One block's tensors in guarded buffers and the entries of the C ABI on them, as ops.StockBlockFn / ops.SpectralHotPath call them."""

    def __init__(self, case, has_bc, layout="bnw", splits=0, nsplit=NSPLIT):
        from stemgnn_amd import _lib, ops

        self.lib, self.case, self.has_bc, self.layout, self.splits, self.nsplit = _lib.load(), case, int(has_bc), layout, splits, nsplit
        B, N, W, multi = case
        self.d, self.dims4 = dims(*case), (B, N, W, multi)
        self.st = torch.cuda.current_stream().cuda_stream
        dr = _draws(case)
        if layout == "bwn":          # the model input x[B,W,N] read in place
            xm, self.xs = dr["X"].permute(0, 2, 1).contiguous(), (W * N, 1, N)
        else:                        # a backcast [B,N,W]
            xm, self.xs = dr["X"], (N * W, W, 1)
        self.inp, self.w = {}, {}
        self._put("X", xm)
        self._put("mul_L", dr["mul_L"])
        self._put("dforecast", dr["wf"])
        if has_bc:
            self._put("dbackcast", dr["wb"])
        self._put("tables", ops.dft_tables(W, multi, torch.device(DEV)))
        assert self.inp["tables"].n == self.lib.stemgnn_table_floats(W, multi)
        self.params = [None if (not has_bc and i in (5, 6)) else self._put(f"param{i}", t) for i, t in enumerate(dr["params"])]
        self.parr = self._ptrs(self.params)

    def _put(self, name, t):
        b = _Buf(t.numel())
        b.t.copy_(t.reshape(-1))
        self.inp[name] = b
        return b

    @staticmethod
    def _ptrs(bufs):
        arr = (ctypes.c_void_p * NPARAMS)()
        for i, b in enumerate(bufs):
            arr[i] = None if b is None else b.ptr()
        return arr

    def fresh(self, name, n, fill=float("nan")):
        self.w[name] = _Buf(n, fill)
        return self.w[name]

    def done(self, rc, what):
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        allb = {**self.inp, **self.w}
        ok = torch.stack([(b.full[b.n:] == SENTINEL).all() for b in allb.values()])
        if not bool(ok.all()):
            raise AssertionError(f"{what}: wrote behind the end of {[k for k, b in allb.items() if not b.intact()]}")

    # ---- packing
    def pack(self, how=None):
        lib, (B, N, W, multi), st = self.lib, self.dims4, self.st
        how = how or ("panels" if self.splits else "pack")
        pk = self.fresh("packed", lib.stemgnn_packed_floats(W, multi))
        tab = self.inp["tables"].ptr()
        if how == "pack":
            self.done(lib.stemgnn_block_pack(self.parr, tab, pk.ptr(), W, multi, st), "block_pack")
        else:
            self.done(lib.stemgnn_block_pack_panels(self.parr, tab, pk.ptr(), W, multi, st), "block_pack_panels")
            if how == "panels+repack":
                self.done(lib.stemgnn_glu_fused_repack(pk.ptr(), W, multi, st), "glu_fused_repack")
        if self.splits:
            self.split_panels()
        return pk

    def split_panels(self):
        lib, (B, N, W, multi), st = self.lib, self.dims4, self.st
        sp = self.fresh("split", lib.stemgnn_glu_split_floats(W, multi, self.splits))
        self.done(lib.stemgnn_glu_split_panels(self.w["packed"].ptr(), sp.ptr(), W, multi, self.splits, st), "glu_split_panels")

    # ---- forward
    def gft_fwd(self, dst):
        B, N, W, multi = self.dims4
        self.done(self.lib.stemgnn_gft_fwd(self.inp["mul_L"].ptr(), self.inp["X"].ptr(), *self.xs, dst.ptr(), B, N, W, self.st), "gft_fwd")

    def glu_fwd(self):
        lib, (B, N, W, multi), w = self.lib, self.dims4, self.w
        if self.splits:
            rc = lib.stemgnn_spectral_glu_fwd_split(w["packed"].ptr(), w["split"].ptr(), w["saved"].ptr(), B, N, W, multi, self.splits, self.st)
        else:
            rc = lib.stemgnn_spectral_glu_fwd(w["packed"].ptr(), w["saved"].ptr(), B, N, W, multi, self.st)
        self.done(rc, "spectral_glu_fwd" + ("_split" if self.splits else ""))

    def out_bufs(self, accumulate):
        d = self.d
        fo = self.fresh("forecast", d.M * d.W)
        if accumulate:
            fo.t.copy_(_draws(self.case)["old"].reshape(-1))
        bc = self.fresh("backcast", d.M * d.W) if self.has_bc else None
        return fo, bc

    def forward(self, accumulate=0):
        lib, (B, N, W, multi), w = self.lib, self.dims4, self.w
        sv = self.fresh("saved", lib.stemgnn_saved_floats(B, N, W, multi))
        fo, bc = self.out_bufs(accumulate)
        self.gft_fwd(sv)
        self.glu_fwd()
        rc = lib.stemgnn_igft_heads_fwd(self.parr, w["packed"].ptr(), sv.ptr(), self.inp["X"].ptr(), *self.xs, fo.ptr(), accumulate,
                                        bc.ptr() if bc else None, B, N, W, multi, self.st)
        self.done(rc, "igft_heads_fwd")
        return self.forward_views()

    def forward_views(self):
        d, w = self.d, self.w
        got = dict(forecast=w["forecast"].t.view(d.M, d.W))
        if self.has_bc:
            got["backcast"] = w["backcast"].t.view(d.M, d.W)
        if "saved" in w:
            L = saved_layout(d)
            for q in FWD_Q[2:]:
                off, rows, ld, cu = L[q]
                got[q] = w["saved"].t[off: off + rows * ld].view(rows, ld)[:, :cu]
        return got

    def forward_infer(self):
        lib, (B, N, W, multi), w = self.lib, self.dims4, self.w
        n_ws = lib.stemgnn_infer_workspace_split_floats(B, N, W, multi, self.splits)
        ws = self.fresh("ws", n_ws)
        w.pop("saved", None)
        fo, bc = self.out_bufs(0)
        self.gft_fwd(ws)
        if self.splits:
            rc = lib.stemgnn_spectral_glu_fwd_split_infer(w["packed"].ptr(), w["split"].ptr(), ws.ptr(), n_ws, B, N, W, multi, self.splits, self.st)
        else:
            rc = lib.stemgnn_spectral_glu_fwd_infer(w["packed"].ptr(), ws.ptr(), n_ws, B, N, W, multi, self.st)
        self.done(rc, "spectral_glu_fwd_infer")
        rc = lib.stemgnn_igft_heads_fwd_infer(self.parr, w["packed"].ptr(), ws.ptr(), n_ws, self.inp["X"].ptr(), *self.xs, fo.ptr(), 0,
                                              bc.ptr() if bc else None, B, N, W, multi, self.st)
        self.done(rc, "igft_heads_fwd_infer")
        return self.forward_views()

    # ---- backward
    def heads_bwd(self, parts):
        lib, (B, N, W, multi), w, inp = self.lib, self.dims4, self.w, self.inp
        rc = lib.stemgnn_igft_heads_bwd(self.parr, w["packed"].ptr(), w["saved"].ptr(), inp["X"].ptr(), *self.xs, inp["dforecast"].ptr(),
                                        inp["dbackcast"].ptr() if self.has_bc else None, w["backcast"].ptr() if self.has_bc else None,
                                        w["scratch"].ptr(), w["gradpart"].ptr(), self.nsplit, parts, B, N, W, multi, self.st)
        self.done(rc, f"igft_heads_bwd parts {parts}")

    def glu_bwd(self, parts):
        """parts 1 in bf16x2: stemgnn_spectral_glu_dgrad_split; weight-gradient parts in bf16x2 carry bit 2"""
        lib, (B, N, W, multi), w = self.lib, self.dims4, self.w
        if self.splits and parts == 1:
            rc = lib.stemgnn_spectral_glu_dgrad_split(w["packed"].ptr(), w["split"].ptr(), w["saved"].ptr(), w["scratch"].ptr(), B, N, W, multi,
                                                      self.splits, self.st)
            return self.done(rc, "spectral_glu_dgrad_split")
        if self.splits and parts & 2:
            parts |= 4
        rc = lib.stemgnn_spectral_glu_bwd(w["packed"].ptr(), w["saved"].ptr(), w["scratch"].ptr(), w["gradpart"].ptr(), self.nsplit, parts, B, N,
                                          W, multi, self.st)
        self.done(rc, f"spectral_glu_bwd parts {parts}")

    def block_wgrad(self, cu_percent=100):
        lib, (B, N, W, multi), w, inp = self.lib, self.dims4, self.w, self.inp
        a = (self.parr, w["packed"].ptr(), w["saved"].ptr(), inp["X"].ptr(), *self.xs, inp["dforecast"].ptr(), self.has_bc, w["scratch"].ptr(),
             w["gradpart"].ptr(), self.nsplit, cu_percent, B, N, W, multi)
        if self.splits:
            self.done(lib.stemgnn_block_wgrad_split(*a, self.splits, self.st), f"block_wgrad_split cu {cu_percent}")
        else:
            self.done(lib.stemgnn_block_wgrad(*a, self.st), f"block_wgrad cu {cu_percent}")

    def backward(self, form="block", cu_percent=100):
        """form: "block" = data parts, then stemgnn_block_wgrad(_split); "3" = both entries with parts 3; "1,2" = the data parts, then
        the weight-gradient parts (the slab path of the heads, the GLU products alone)"""
        lib, (B, N, W, multi), w, inp, d = self.lib, self.dims4, self.w, self.inp, self.d
        before = (w["saved"].full.clone(), w["packed"].full.clone())
        self.fresh("scratch", lib.stemgnn_scratch_floats(B, N, W, multi))
        self.fresh("gradpart", lib.stemgnn_gradpart_floats(W, multi, self.nsplit))
        dX, dT = self.fresh("dX", d.M * W), self.fresh("dmul_L", 4 * N * N)
        assert lib.stemgnn_scratch_offset_dG(B, N, W, multi) == scratch_layout(d)["dG"][0]
        if form == "3":
            self.heads_bwd(3)
            self.glu_bwd(3)
        else:
            self.heads_bwd(1)
            self.glu_bwd(1)
            if form == "block":
                self.block_wgrad(cu_percent)
            else:
                self.heads_bwd(2)
                self.glu_bwd(2)
        dG = w["scratch"].full[scratch_layout(d)["dG"][0]:]
        rc = lib.stemgnn_gft_bwd(inp["mul_L"].ptr(), inp["X"].ptr(), *self.xs, dG.data_ptr(), dX.ptr(), dT.ptr(), 0, B, N, W, self.st)
        self.done(rc, "gft_bwd")
        grads = [self.fresh(f"grad{i}", t.numel()) if (self.has_bc or i not in (5, 6)) else None for i, t in enumerate(_draws(self.case)["params"])]
        rc = lib.stemgnn_block_unpack_grads(w["gradpart"].ptr(), self.nsplit, inp["tables"].ptr(), self._ptrs(grads), W, multi, self.has_bc, self.st)
        self.done(rc, "block_unpack_grads")
        if self.has_bc:
            self.done(lib.stemgnn_shortcut_dx(w["scratch"].ptr(), self.params[7].ptr(), dX.ptr(), B, N, W, multi, self.st), "shortcut_dx")
        else:
            assert _all_nan(grads[7].t) and _all_nan(grads[8].t), "has_backcast = 0: the short-cut head's gradient buffers were written"
        assert _bits(w["saved"].full, before[0]), "the backward wrote into `saved`"
        assert _bits(w["packed"].full, before[1]), "the backward wrote into `packed`"
        got = dict(dX=dX.t.view(d.M, W), dmul_L=dT.t.view(4, N, N)[1:])
        for q in DATA_Q:
            if q == "dpB" and not self.has_bc:
                continue
            off, rows, ld, _ = scratch_layout(d)[q]
            v = w["scratch"].t[off: off + rows * ld].view(rows, ld)
            got[q] = v if q != "dG" else v[: d.M] + v[d.M:]
        for i, k in enumerate(PARAM_NAMES):
            if grads[i] is not None and (self.has_bc or i not in (7, 8)):
                got["d " + k] = grads[i].t
        return got

    def run(self, pack=None, form="block", accumulate=0, cu_percent=100):
        self.w.clear()
        self.pack(pack)
        got = self.forward(accumulate)
        got.update(self.backward(form, cu_percent))
        return got

    def raw(self, names=("saved", "scratch", "forecast", "backcast", "dX", "dmul_L") + tuple(f"grad{i}" for i in range(NPARAMS))):
        return {k: self.w[k].t.clone() for k in names if k in self.w}


def _same(a, b):
    return [k for k in a if not _bits(a[k], b[k])]


def _cross(tag, a, b, ref, names):
    """rows that hold form a against form b to the bound the reference's own error sets (e_ref of that quantity)"""
    r64, r32 = ref
    return [(f"{tag} {q}", _relerr(a[q], b[q]), _relerr(r32[q], r64[q])) for q in names if r64.get(q) is not None and r64[q].numel()]


ARITH = [0, 2]


@pytest.mark.parametrize("splits", ARITH, ids=["f32", "bf16x2"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_block_case_vs_fp64(case, splits):
    """Both backcast states, both input layouts, accumulate = 1 and the repeat, everything against fp64."""
    rows = []
    for has_bc in (1, 0):
        ref = _reference(case, has_bc)
        blk = _Block(case, has_bc, "bnw", splits)
        got = blk.run()
        raw = blk.raw()
        names = FWD_Q + DATA_Q + GRAD_Q
        rows += _rows(got, ref, names, f"bc{has_bc} bnw ")
        blk.run()
        assert not _same(raw, blk.raw()), f"has_backcast {has_bc}: differs from launch to launch: {_same(raw, blk.raw())}"
        # the other layout of X: the same values, another addressing -- against fp64 and against the first layout
        alt = _Block(case, has_bc, "bwn", splits)
        got2 = alt.run()
        rows += _rows(got2, ref, names, f"bc{has_bc} bwn ") + _cross(f"bc{has_bc} bwn vs bnw", got2, got, ref, names)
        # accumulate = 1: old + fresh within one rounding (round to nearest: half an ulp of the sum), everything else untouched
        alt.w.clear()
        alt.pack()
        acc = alt.forward(accumulate=1)
        old = _draws(case)["old"].to(DEV).reshape(got2["forecast"].shape).double()
        want = old + got2["forecast"].double()
        assert bool(((acc["forecast"].double() - want).abs() <= 2.0 ** -24 * want.abs()).all()), \
            f"has_backcast {has_bc}: accumulate = 1 is not old + fresh within one rounding"
        rest = [k for k in acc if k != "forecast"]
        assert not _same({k: acc[k] for k in rest}, {k: got2[k] for k in rest}), "accumulate = 1 changed something beside the forecast"
    _judge(f"BLOCK {case} splits {splits}", rows, splits)


@pytest.mark.parametrize("splits", ARITH, ids=["f32", "bf16x2"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_block_parts_and_wgrad_forms(case, splits):
    """parts 3 against 1 then 2 of stemgnn_igft_heads_bwd / stemgnn_spectral_glu_bwd (the slab path of the heads' weight gradients),
    stemgnn_block_wgrad at cu_percent 100 and 10 and with nsplit 1 / 3 / 32: every form within the bound of fp64.  Neither the header
    nor DESIGN.md promises bits between these forms: whether they matched is printed."""
    ref = _reference(case, 1)
    names = DATA_Q + GRAD_Q
    rows, raws = [], {}
    for form, cu, nsplit in (("3", 100, NSPLIT), ("1,2", 100, NSPLIT), ("block", 100, NSPLIT), ("block", 10, NSPLIT), ("block", 100, 1),
                             ("block", 100, 3)):
        blk = _Block(case, 1, "bwn", splits, nsplit)
        tag = f"{form} cu{cu} nsplit{nsplit}"
        got = blk.run(pack="pack", form=form, cu_percent=cu)      # the fp32 streams too: parts 3 runs the fp32 chain in either arithmetic
        rows += _rows(got, ref, names, tag + " ")
        raws[tag] = blk.raw(("scratch", "dX", "dmul_L") + tuple(f"grad{i}" for i in range(NPARAMS)))
    base = f"3 cu100 nsplit{NSPLIT}"
    for tag, raw in raws.items():
        if tag != base and not (splits and tag.startswith("block")):      # (bf16x2: the block form runs another data-gradient chain)
            diff = _same(raws[base], raw)
            print(f"BLOCK parts {case} splits {splits}: {tag} against parts 3: " + ("same bits" if not diff else f"other bits in {diff}"))
    _judge(f"BLOCK parts {case} splits {splits}", rows, splits)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_block_glu_fused_settings(case, monkeypatch):
    """STEMGNN_GLU_FUSED 0..3 (read per call).  Exact fp32: the forward has the same bits in every setting, the 64- and
    96-row data-gradient chains have each other's bits, every setting is within the bound of fp64 on its own.  bf16x2: 0 (per-layer
    split launches) and 1 against fp64 (the fused bf16 kernels split layer 0 too: no bits between them)."""
    ref = _reference(case, 1)
    names = FWD_Q + DATA_Q + GRAD_Q
    rows, raws = [], {}
    for splits, modes in ((0, "0123"), (2, "01")):
        for mode in modes:
            monkeypatch.setenv("STEMGNN_GLU_FUSED", mode)
            blk = _Block(case, 1, "bwn", splits)
            rows_m = _rows(blk.run(), ref, names, f"splits {splits} FUSED={mode} ")
            if splits == 0:
                rows += rows_m
                raws[mode] = blk.raw()
            else:
                _judge(f"BLOCK fused {case} splits 2 FUSED={mode}", rows_m, 2)
    monkeypatch.delenv("STEMGNN_GLU_FUSED")
    fwd = ("saved", "forecast", "backcast")
    for mode in "123":
        diff = _same({k: raws["0"][k] for k in fwd}, {k: raws[mode][k] for k in fwd})
        assert not diff, f"STEMGNN_GLU_FUSED={mode}: other bits in the forward's {diff} than with 0"
    assert not _same(raws["2"], raws["3"]), f"the 64- and 96-row forms differ in {_same(raws['2'], raws['3'])}"
    _judge(f"BLOCK fused {case} splits 0", rows, 0)


@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_block_pack_panels_repack_is_pack(case):
    a, b = _Block(case, 1), _Block(case, 1)
    pa, pb = a.pack("pack"), b.pack("panels+repack")
    assert pa.n == pb.n == a.lib.stemgnn_packed_floats(case[2], case[3])
    assert _bits(pa.t, pb.t), "stemgnn_block_pack_panels + stemgnn_glu_fused_repack: other bits than stemgnn_block_pack"
    # has_backcast = 0 (parameters 5, 6 NULL) packs the same panels: the backcast heads are not part of `packed`
    c = _Block(case, 0)
    assert _bits(c.pack("pack").t, pa.t)


@pytest.mark.parametrize("splits", ARITH, ids=["f32", "bf16x2"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_block_warm_up(case, splits):
    """stemgnn_spectral_glu_fwd_warm on a guarded dummy `saved` (NaN but for a finite G region): guards intact, and a real forward
    after it has the bits of one without it."""
    B, N, W, multi = case
    blk = _Block(case, 1, "bwn", splits)
    blk.pack("pack")
    plain = blk.forward()
    raw = blk.raw(("saved", "forecast", "backcast"))
    n = blk.lib.stemgnn_glu_warm_saved_floats(W, multi)
    assert n == blk.lib.stemgnn_saved_floats(1, 4 * 96, W, multi)
    dummy = blk.fresh("warm", n)
    g = torch.Generator(device=DEV).manual_seed(5)
    dummy.t[: 4 * 96 * 3 * W] = torch.randn(4 * 96 * 3 * W, device=DEV, generator=g)     # covers the G region of every warm-up shape
    rc = blk.lib.stemgnn_spectral_glu_fwd_warm(blk.w["packed"].ptr(), blk.w["split"].ptr() if splits else None, dummy.ptr(), B, N, W, multi,
                                               splits, blk.st)
    blk.done(rc, "spectral_glu_fwd_warm")
    assert not _same(raw, blk.raw(("saved", "forecast", "backcast"))), "the warm-up wrote into the real buffers"
    blk.forward()
    assert not _same(raw, blk.raw(("saved", "forecast", "backcast"))), "a forward behind the warm-up has other bits"
    assert plain["forecast"].shape == (B * N, W)


@pytest.mark.parametrize("splits", ARITH, ids=["f32", "bf16x2"])
@pytest.mark.parametrize("case", BLOCK_CASES, ids=_ids(BLOCK_CASES))
def test_block_inference_entries(case, splits):
    """_fwd_infer / _split_infer / stemgnn_igft_heads_fwd_infer on a NaN workspace of exactly stemgnn_infer_workspace_split_floats:
    the bits of the training forward (include/stemgnn_hip.h), in both backcast states and both layouts."""
    for has_bc, layout in ((1, "bwn"), (0, "bnw")):
        blk = _Block(case, has_bc, layout, splits)
        blk.pack()
        blk.forward()
        train = blk.raw(("forecast", "backcast"))
        blk.forward_infer()
        assert not _same(train, blk.raw(("forecast", "backcast"))), f"has_backcast {has_bc}: the inference entries have other bits"
