"""GPU: the attention / Laplacian / Chebyshev stage (csrc/front.hip) through the C ABI against fp64, one case per form.

FRONT_CASES is (N, B, drop_p, dL mode, nchunk); tests/test_front_cases.py proves on the CPU that the list reaches both sides of
every decision the stage takes by shape (register / LDS forms at N = 256, the 64-lane and 32 / 4 tile edges, N < nchunk, the
batch-chunk shapes of the forward, dropout on both sides of N = 256) and that the host model of the dropout map
(tests/helpers/philox_ref.py) is Philox4x32-10.

Inputs (seeded fp32 draws): h = tanh(randn(N, B, N)), wk, wq = randn(N, 1) * 2 / sqrt(N) (logits with a spread of 1.5 to 1.8:
max(att) * N is between 2 and 18, not the 1.04 of initial weights), dL = randn ("rand") or 1e-3 randn + randn row-constant +
randn column-constant parts ("struct": stresses the dp - dot cancellation of the softmax backward).

Hygiene: saved, scratch, attention_out, mul_L and every output are NaN before each call, every buffer carries a guard band
behind the size its stemgnn_*_floats function returns (must read back unchanged), one call per case is repeated (same bits).

Reference: oracle.self_graph_attention / laplacian_from_attention / cheb_polynomial with autograd in fp64 on the same fp32
values, on the device.  key / query are formed by the oracle's own line (matmul(inp, w)) and handed to self_graph_attention as
a two-step sequence with unit weights (1 * key + 0 * query is exact), which makes d key / d query leaves of the graph.  Both
the fp64 and the fp32 run get kink_pos = (key32 + query32 > 0) from the key / query the kernel saved (an fp32 add, as in the
kernels); tests/util.kink_audit checks those decisions against the fp64 logits.  Under dropout the oracle gets the mask the
HOST model predicts, and stemgnn_dropout_mask must equal it bit for bit.  Without dropout the Laplacian backward drops the
row-constant degree term (the softmax backward annihilates it), so dA / B is compared after subtracting each row's mean from
both sides -- exactly the freedom that leaves.

Forms compared with each other (bits where the code or the header promises them): forward parts 3 against 1 then 2 (A,
attention_out, key, query, rowsum: bits; deg, mul_L[1]: each within the bound of fp64 -- the fused kernel sums per-chunk
degrees, the split one the reduced row); backward parts 3 against 1 then 2 (all bits); parts 3|4 (dkey | dquery bits, dh / dwk /
dwq untouched); parts 3|4|8 then stemgnn_attn_dquery_reduce with out = NULL and with a buffer (bits); stemgnn_keyquery_wgrad
against stemgnn_keyquery_wgrad2 (bits), both within the rounding bound of fp64 AND of the dwk / dwq of the materialised call;
nchunk in {1, 3, 16, N, N + 5}: dkey bits, dquery within the bound.

Tolerances.  Hard bar: relerr < 1e-4 (max-norm relative, tests/util.relerr) against fp64.  Rounding-class bar: with e_ref the
relerr of torch's fp32 evaluation of the same functions against the fp64 run, e_kernel <= K * max(e_ref, 2^-22), the floor and
form of tests/test_hip_gru_paths.py.  Why a factor at all: the kernels sum rows in 64-lane trees and the batch in up to 8
chunks where torch sums linearly, and evaluate exp with the device's expf -- a small factor, not orders.  The Chebyshev
products take the same form with their own K_CHEB, capped by the 1e-5 the stage tests of tests/test_hip_graph_phased.py hold.

K = 8 and K_CHEB = 2: the worst ratio e_kernel / max(e_ref, 2^-22) measured on an MI355X (256 CUs) over the 29 cases, the 4
nchunk sweeps (5 values each) and the 15 Chebyshev runs, rounded up to the next power of two.  Worst ratio per quantity (the
case that gave it):

    quantity               ratio   case (N, B, p, dL, nchunk)            e_kernel   e_ref
    key                    1.30    (257, 9, 0.5, rand, 16)               3.10e-07   2.00e-07
    query                  1.14    (300, 17, 0.2, struct, 305)           2.77e-07   2.44e-07
    A                      2.35    (129, 2, 0, rand, 129)                7.09e-07   3.02e-07
    deg                    0.90    (257, 9, 0.5, rand, 16)               2.16e-07   1.23e-07
    attention_out          2.61    (2048, 7, 0, struct, 16)              1.82e-06   6.98e-07
    mul_L[1]               1.31    (255, 7, 0.2, struct, 16)             3.12e-07   2.26e-07
    deg, parts 1 then 2    1.00    (2048, 7, 0, struct, 16)              2.38e-07   1.19e-07
    mul_L[1], 1 then 2     1.05    (300, 17, 0.2, struct, 305)           2.52e-07   2.40e-07
    dA / B                 1.57    (33, 7, 0.5, struct, 16)              3.74e-07   2.24e-07
    dkey                   5.12    (228, 33, 0, struct, 16)              3.76e-06   7.35e-07
    dquery                 3.08    (256, 8, 0, rand, 16)                 7.96e-07   2.58e-07
    dh                     2.93    (256, 8, 0, rand, 16)                 7.94e-07   2.71e-07
    dwk                    2.50    (2048, 7, 0, struct, 16)              6.84e-06   2.73e-06
    dwq                    0.89    (257, 1, 0, struct, 16)               3.55e-07   3.99e-07
    dwk, dwq (wgrad)       2.50    as dwk / dwq; against the materialised call's: 0 in every case (asserted: the bound)
    T2 / T3                1.11 / 1.17   N = 32 / 127                    2.65e-07 / 5.08e-07   2.16e-07 / 4.32e-07
    dLp / dT2p / dL        1.13 / 1.00 / 1.14   N = 128 / 33 / 127       4.23e-07 / 2.61e-07 / 3.28e-07

(dkey, the largest: in "struct" mode dA / B carries O(1) row- and column-constant parts that the softmax backward's dp - dot
cancels down to the 1e-3 part; the kernel's dot is a 64-lane tree over a row of p * dp, torch's a linear sum, and every "rand"
case stays below 3.1.  Nothing needs more than 16.)

attention_out's symmetry and its equality with the two-part form hold for every B because sg_laplacian_fused_kernel forms
0.5 (own / B + partner / B) without contracting the first product into the add (17 of the 29 cases have 1 / B not a power of
two, where a contracted form is off by an ulp).
"""
import math

import numpy as np
import pytest
import torch

from tests.helpers import philox_ref
from tests.util import DEV, GUARD, SENTINEL, _all_nan, _bits, _Buf, _relerr, kink_audit      # noqa: F401 (GUARD, SENTINEL: the guard band of _Buf)

pytestmark = pytest.mark.gpu
TOL = 1e-4
TOL_CHEB = 1e-5
K = 8
K_CHEB = 2
FLOOR = 2.0 ** -22
ALPHA = 0.2
SG_EINVAL = -10001
SEED, OFFSET = 0x9E3779B97F4A7C15, (1 << 32) + 0xFFFFFFF0      # high words set; the offset above 2^32

NS = [1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 129, 228, 255, 256, 257, 300, 511, 513, 1024, 2048]
BS = [1, 2, 7, 8, 9, 15, 17, 33, 64]


def NCHUNKS(N):
    return [1, 3, 16, N, N + 5]


FRONT_CASES = [
    # (N, B, drop_p, dL mode, nchunk)
    (1, 1, 0.0, "rand", 16), (1, 7, 0.0, "struct", 1), (2, 2, 0.0, "rand", 16), (3, 9, 0.0, "struct", 3), (5, 15, 0.0, "rand", 16),
    (31, 8, 0.0, "struct", 16), (32, 17, 0.0, "rand", 37), (33, 7, 0.5, "struct", 16), (63, 33, 0.0, "rand", 16),
    (64, 64, 0.2, "rand", 16), (65, 15, 0.5, "struct", 3), (127, 9, 0.0, "struct", 16), (129, 2, 0.0, "rand", 129),
    (228, 33, 0.0, "struct", 16), (228, 33, 0.5, "rand", 16), (255, 7, 0.2, "struct", 16), (256, 8, 0.0, "rand", 16),
    (256, 8, 0.5, "struct", 1), (257, 9, 0.5, "rand", 16), (257, 1, 0.0, "struct", 16), (300, 17, 0.0, "rand", 16),
    (300, 17, 0.2, "struct", 305), (511, 64, 0.0, "struct", 16), (513, 8, 0.5, "struct", 16), (513, 2, 0.0, "rand", 3),
    (1024, 9, 0.5, "rand", 16), (1024, 17, 0.0, "struct", 16), (2048, 9, 0.0, "rand", 16), (2048, 7, 0.0, "struct", 16),
]
NCHUNK_CASES = [(5, 7, 0.0, "rand"), (33, 9, 0.5, "struct"), (228, 8, 0.0, "struct"), (300, 17, 0.5, "rand")]
MASK_NS = [1, 63, 64, 65, 255, 256, 257, 300, 512, 513, 1024]
MASK_PS = [0.0, 0.2, 0.5, 0.9]
MASK_SEEDS = [(SEED, OFFSET), (0xFFFFFFFF00000001, 1 << 32), ((1 << 63) + 12345, (1 << 40) + 7)]
CHEB_NS = [1, 2, 3, 31, 32, 33, 127, 128, 129, 511, 512, 513, 640]
CHEB_GENERIC_N = 129             # also with STEMGNN_GRAPH_PHASED=0 (the generic launch of the first backward product)


def _seed_tensor(seed, offset):
    return torch.from_numpy(np.array([seed, offset], dtype=np.uint64).view(np.int64)).to(DEV)


def _draws(N, B, mode):
    g = torch.Generator().manual_seed(1000003 * N + 1009 * B + (mode == "struct"))
    h = torch.tanh(torch.randn(N, B, N, generator=g))
    wk = torch.randn(N, 1, generator=g) * 2 / math.sqrt(N)
    wq = torch.randn(N, 1, generator=g) * 2 / math.sqrt(N)
    if mode == "struct":
        dL = 1e-3 * torch.randn(N, N, generator=g) + torch.randn(N, 1, generator=g) + torch.randn(1, N, generator=g)
    else:
        dL = torch.randn(N, N, generator=g)
    return {k: v.contiguous().to(DEV) for k, v in dict(h=h, wk=wk, wq=wq, dL=dL).items()}


class _Stage:
    """The front's entries of the C ABI on NaN-filled, guarded buffers."""

    def __init__(self, d, N, B, p, seed=None):
        from stemgnn_amd import _lib

        self.lib, self.d, self.N, self.B, self.p = _lib.load(), d, N, B, p
        self.seed = _seed_tensor(*seed) if seed is not None else None
        self.st = torch.cuda.current_stream().cuda_stream
        self.bufs = [_Buf(t.numel()) for t in d.values()]     # the inputs live in guarded copies too (nothing may write near them)
        for b, t in zip(self.bufs, d.values()):
            b.t.copy_(t.reshape(-1))
        self.h, self.wk, self.wq, self.dL = self.bufs

    def done(self, rc, what, bufs):
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        for name, b in bufs.items():
            assert b.intact(), f"{what}: wrote behind the end of {name}"
        for name, b in zip(("h", "wk", "wq", "dL"), self.bufs):
            assert b.intact(), f"{what}: wrote behind the end of {name}"

    def _seedp(self):
        return self.seed.data_ptr() if self.seed is not None else None

    def fwd(self, parts_seq=(3,)):
        N, B, lib = self.N, self.B, self.lib
        bufs = dict(saved=_Buf(lib.stemgnn_attn_saved_floats(B, N)), att=_Buf(N * N), mul_L=_Buf(4 * N * N))
        for parts in parts_seq:
            rc = lib.stemgnn_attn_laplacian_fwd(self.h.ptr(), self.wk.ptr(), self.wq.ptr(), ALPHA, self.p, 1, self._seedp(), B, N,
                                                bufs["saved"].ptr(), bufs["att"].ptr(), bufs["mul_L"].ptr(), parts, self.st)
            self.done(rc, f"attn_laplacian_fwd parts {parts}", bufs)
            if parts == 1:
                assert _all_nan(bufs["att"].t) and _all_nan(bufs["mul_L"].t), "forward part 1 touched attention_out / mul_L"
        s = bufs["saved"].t
        bn = B * N
        out = dict(saved=bufs["saved"], key=s[:bn].view(B, N), query=s[bn:2 * bn].view(B, N), rowsum=s[2 * bn:3 * bn].view(B, N),
                   A=s[3 * bn:3 * bn + N * N].view(N, N), deg=s[3 * bn + N * N:3 * bn + N * N + N],
                   att=bufs["att"].t.view(N, N), mul_L=bufs["mul_L"].t.view(4, N, N))
        return out

    def bwd(self, saved, nchunk, parts_seq=(3,), null_out=False):
        N, B, lib = self.N, self.B, self.lib
        bufs = dict(scratch=_Buf(lib.stemgnn_attn_scratch_floats(B, N, nchunk)), dh=_Buf(N * B * N), dwk=_Buf(N), dwq=_Buf(N))
        before = saved.full.clone()
        for parts in parts_seq:
            outs = (None, None, None) if null_out else (bufs["dh"].ptr(), bufs["dwk"].ptr(), bufs["dwq"].ptr())
            rc = lib.stemgnn_attn_laplacian_bwd(self.dL.ptr(), self.h.ptr(), self.wk.ptr(), self.wq.ptr(), ALPHA, self.p, 1,
                                                self._seedp(), B, N, saved.ptr(), bufs["scratch"].ptr(), nchunk, *outs, parts, self.st)
            self.done(rc, f"attn_laplacian_bwd parts {parts} nchunk {nchunk}", bufs)
        assert _bits(saved.full, before), "the backward wrote into `saved`"
        s = bufs["scratch"].t
        nn, bn = N * N, B * N
        return dict(scratch=bufs["scratch"], dAB=s[:nn].view(N, N), dkey=s[nn:nn + bn].view(B, N), dquery=s[nn + bn:nn + 2 * bn].view(B, N),
                    dqpart=s[nn + 2 * bn:].view(B, nchunk, N), dh=bufs["dh"].t.view(N, B, N), dwk=bufs["dwk"].t, dwq=bufs["dwq"].t)

    def dquery_reduce(self, scratch, nchunk, to_buffer):
        out = _Buf(self.B * self.N)
        rc = self.lib.stemgnn_attn_dquery_reduce(scratch.ptr(), self.B, self.N, nchunk, out.ptr() if to_buffer else None, self.st)
        self.done(rc, "attn_dquery_reduce", dict(scratch=scratch, out=out))
        return out.t.view(self.B, self.N)

    def wgrad(self, scratch=None, dkey=None, dquery=None):
        N, B = self.N, self.B
        bufs = dict(dwk=_Buf(N), dwq=_Buf(N))
        if scratch is not None:
            rc = self.lib.stemgnn_keyquery_wgrad(self.h.ptr(), scratch.ptr(), bufs["dwk"].ptr(), bufs["dwq"].ptr(), B, N, self.st)
            bufs["scratch"] = scratch
        else:
            kq = [_Buf(B * N), _Buf(B * N)]
            kq[0].t.copy_(dkey.reshape(-1))
            kq[1].t.copy_(dquery.reshape(-1))
            rc = self.lib.stemgnn_keyquery_wgrad2(self.h.ptr(), kq[0].ptr(), kq[1].ptr(), bufs["dwk"].ptr(), bufs["dwq"].ptr(), B, N, self.st)
            bufs.update(dkey=kq[0], dquery=kq[1])
        self.done(rc, "keyquery_wgrad" + ("" if scratch is not None else "2"), bufs)
        return bufs["dwk"].t, bufs["dwq"].t

    def mask(self, p=None):
        N, B = self.N, self.B
        m = _Buf(B * N * N)
        rc = self.lib.stemgnn_dropout_mask(self.p if p is None else p, self.seed.data_ptr(), B, N, m.ptr(), self.st)
        self.done(rc, "dropout_mask", dict(mask=m))
        return m.t.view(B, N, N)


def _reference(d, N, B, p, mask, key32, query32, dt):
    """every compared quantity of the stage in `dt` on the device, by the oracle's functions and autograd"""
    from oracle import stemgnn_oracle as O

    h = d["h"].to(dt).requires_grad_(True)
    wk = d["wk"].to(dt).requires_grad_(True)
    wq = d["wq"].to(dt).requires_grad_(True)
    inp = h.permute(1, 2, 0)                                  # [B, i, s]: self_graph_attention's own `inp` for gru_out = h[s, b, i]
    key, query = torch.matmul(inp, wk), torch.matmul(inp, wq)  # its lines :154-155
    key.retain_grad()
    query.retain_grad()
    unit = torch.eye(2, dtype=dt, device=h.device)
    kink = (key32[:, :, None] + query32[:, None, :]) > 0       # fp32 add, as in the kernels
    p32 = float(np.float32(p))
    att = O.self_graph_attention(torch.cat([key, query], 2).permute(0, 2, 1), unit[:, :1], unit[:, 1:], ALPHA,
                                 drop_mask=mask.to(dt) if p > 0 else None, drop_p=p32, kink_pos=kink)
    att.retain_grad()
    L, A_s = O.laplacian_from_attention(att)
    (L * d["dL"].to(dt)).sum().backward()
    A = att.detach().mean(0)
    r = dict(key=key.detach()[..., 0], query=query.detach()[..., 0], A=A, deg=A.sum(1), att=A_s.detach(), L=L.detach(),
             dAB=att.grad[0], dkey=key.grad[..., 0], dquery=query.grad[..., 0], dh=h.grad, dwk=wk.grad[:, 0], dwq=wq.grad[:, 0])
    if dt == torch.float64:
        r["logits"] = (key.detach() + query.detach().transpose(1, 2))
    return r


def _centre(x, p):
    """without dropout dA / B is defined up to a constant per row: take each row's mean out"""
    x = x.double()
    return x if p > 0 else x - x.mean(1, keepdim=True)


def _judge(title, rows, k=K, tol=TOL):
    """rows: (quantity, e_kernel, e_ref).  Prints every figure, then asserts both bars."""
    worst = max(rows, key=lambda r: (r[1] / max(r[2], FLOOR)) if r[1] == r[1] else float("inf"))
    print(f"{title}: worst ratio {worst[1] / max(worst[2], FLOOR):.2f} ({worst[0]}: e_kernel {worst[1]:.2e}, e_ref {worst[2]:.2e})")
    for q, ek, er in rows:
        print(f"    {q:16s} e_kernel {ek:.2e} e_ref {er:.2e} ratio {ek / max(er, FLOOR):.2f}")
    bad = [(q, ek, er) for q, ek, er in rows if not (ek < tol and ek <= k * max(er, FLOOR))]
    assert not bad, bad


def _host_mask(N, B, p, seed):
    m = philox_ref.dropout_mask(p, seed[0], seed[1], B, N)
    assert (m.reshape(B, N, N).mean(0).sum(1) > 0).all(), "a row of the batch-mean attention is dropped whole: the reference is NaN there"
    return torch.from_numpy(m).to(DEV)


def _forward_and_reference(N, B, p, mode):
    d = _draws(N, B, mode)
    seed = (SEED + N, OFFSET + B) if p > 0 else None
    stg = _Stage(d, N, B, p, seed)
    mask = None
    if p > 0:
        mask = _host_mask(N, B, p, seed)
        assert _bits(stg.mask(), mask), "stemgnn_dropout_mask is not the host model's Philox4x32-10 map"
    F = stg.fwd()
    r64 = _reference(d, N, B, p, mask, F["key"], F["query"], torch.float64)
    r32 = _reference(d, N, B, p, mask, F["key"], F["query"], torch.float32)
    ek = float((F["key"].double() - r64["key"]).abs().max())
    eq = float((F["query"].double() - r64["query"]).abs().max())
    pos = (F["key"][:, :, None] + F["query"][:, None, :]) > 0
    kink_audit(pos, r64.pop("logits"), ek + eq, f"front N={N} B={B}: key/query fp32 error {ek:.2e}/{eq:.2e}")
    return d, stg, F, r64, r32


def _fwd_rows(F, r64, r32, tag=""):
    return [(tag + q, _relerr(F[m], r64[r]), _relerr(r32[r], r64[r]))
            for q, m, r in (("key", "key", "key"), ("query", "query", "query"), ("A", "A", "A"), ("deg", "deg", "deg"),
                            ("attention_out", "att", "att"))] + \
           [(tag + "mul_L[1]", _relerr(F["mul_L"][1], r64["L"]), _relerr(r32["L"], r64["L"]))]


def _bwd_rows(Bw, r64, r32, p, tag="", names=("dAB", "dkey", "dquery", "dh", "dwk", "dwq")):
    rows = []
    for q in names:
        if q == "dAB":
            rows.append((tag + "dA/B", _relerr(_centre(Bw[q], p), _centre(r64[q], p)), _relerr(_centre(r32[q], p), _centre(r64[q], p))))
        else:
            rows.append((tag + q, _relerr(Bw[q], r64[q]), _relerr(r32[q], r64[q])))
    return rows


def _ids(cases):
    return ["-".join(f"{k}{v}" for k, v in zip("NBpmc", c)) for c in cases]


@pytest.mark.parametrize("N,B,p,mode,nchunk", FRONT_CASES, ids=_ids(FRONT_CASES))
def test_front_case_vs_fp64(N, B, p, mode, nchunk):
    d, stg, F, r64, r32 = _forward_and_reference(N, B, p, mode)
    # ---- forward: exact facts, the repeat, the two-part form
    assert bool((F["mul_L"][0] == 0).all()), "mul_L[0] is not exactly 0"
    assert _all_nan(F["mul_L"][2:]), "the forward touched mul_L slots 2 / 3"
    assert torch.equal(F["att"], F["att"].T), "attention_out is not bitwise symmetric"
    F2 = stg.fwd()
    assert _bits(F2["saved"].t, F["saved"].t) and _bits(F2["att"], F["att"]) and _bits(F2["mul_L"], F["mul_L"]), \
        "forward differs from launch to launch"
    Fs = stg.fwd((1, 2))
    for q in ("key", "query", "rowsum", "A", "att"):
        assert _bits(Fs[q], F[q]), f"forward parts 1 then 2: other bits of {q} than parts 3"
    assert bool((Fs["mul_L"][0] == 0).all()) and _all_nan(Fs["mul_L"][2:])
    rows = _fwd_rows(F, r64, r32) + [r for r in _fwd_rows(Fs, r64, r32, "split ") if r[0] in ("split deg", "split mul_L[1]")]
    if N == 1:
        assert bool((F["A"] == 1).all()) and bool((F["att"] == 1).all()), "N = 1: the attention is not exactly 1"
        assert bool((F["mul_L"][1] == 0).all()), "N = 1: L is not exactly 0"
    # ---- backward: parts 3, the repeat, 1 then 2
    Bw = stg.bwd(F["saved"], nchunk)
    Bw2 = stg.bwd(F["saved"], nchunk)
    keys = ("scratch", "dh", "dwk", "dwq")
    same = lambda a, b, ks: all(_bits(a[k].t if k == "scratch" else a[k], b[k].t if k == "scratch" else b[k]) for k in ks)
    assert same(Bw2, Bw, keys), "backward differs from launch to launch"
    Bs = stg.bwd(F["saved"], nchunk, (1, 2))
    assert same(Bs, Bw, keys), "backward parts 1 then 2: other bits than parts 3"
    rows += _bwd_rows(Bw, r64, r32, p)
    if N == 1:
        assert all(bool((Bw[q] == 0).all()) for q in ("dkey", "dquery", "dh", "dwk", "dwq")), "N = 1: a gradient is not exactly 0"
    # ---- factored: parts 3|4 leaves dkey | dquery, touches no output
    Bf = stg.bwd(F["saved"], nchunk, (3 | 4,))
    assert same(Bf, Bw, ("scratch",)), "parts 3|4: other bits in the scratch (dA / B | dkey | dquery | partials) than the materialised form"
    assert _all_nan(Bf["dh"]) and _all_nan(Bf["dwk"]) and _all_nan(Bf["dwq"]), "parts 3|4 touched dh / dwk / dwq"
    # ---- partial: parts 3|4|8 leaves the per-chunk partials; stemgnn_attn_dquery_reduce sums them
    Bp = stg.bwd(F["saved"], nchunk, (3 | 4 | 8,), null_out=True)
    assert _bits(Bp["dAB"], Bw["dAB"]) and _bits(Bp["dkey"], Bw["dkey"]) and _bits(Bp["dqpart"], Bw["dqpart"]), \
        "parts 3|4|8: other bits of dA / B, dkey or the partials"
    assert _all_nan(Bp["dquery"]), "parts 3|4|8 reduced dquery"
    out = stg.dquery_reduce(Bp["scratch"], nchunk, to_buffer=True)
    assert _bits(out, Bw["dquery"]), "stemgnn_attn_dquery_reduce(out): other bits than the inline reduction"
    assert _all_nan(Bp["dquery"]), "stemgnn_attn_dquery_reduce(out) wrote the scratch's dquery slot"
    stg.dquery_reduce(Bp["scratch"], nchunk, to_buffer=False)
    assert _bits(Bp["dquery"], Bw["dquery"]), "stemgnn_attn_dquery_reduce(NULL): other bits than the inline reduction"
    # ---- weight gradients from the factors
    dwk1, dwq1 = stg.wgrad(scratch=Bf["scratch"])
    dwk2, dwq2 = stg.wgrad(dkey=Bw["dkey"], dquery=Bw["dquery"])
    assert _bits(dwk1, dwk2) and _bits(dwq1, dwq2), "stemgnn_keyquery_wgrad and _wgrad2 differ"
    rows += _bwd_rows(dict(dwk=dwk1, dwq=dwq1), r64, r32, p, "wgrad ", ("dwk", "dwq"))
    # ... and against the dwk / dwq of the materialised call (sg_keyquery_bwd_kernel), held to the same bound
    rows += [("wgrad dwk vs mat.", _relerr(dwk1, Bw["dwk"]), rows[-2][2]), ("wgrad dwq vs mat.", _relerr(dwq1, Bw["dwq"]), rows[-1][2])]
    _judge(f"FRONT {(N, B, p, mode, nchunk)}", rows)


@pytest.mark.parametrize("N,B,p,mode", NCHUNK_CASES, ids=_ids(NCHUNK_CASES))
def test_front_nchunk(N, B, p, mode):
    """One wave does a row whichever chunk owns it: dkey has the same bits for every nchunk; dquery is a sum in chunk order."""
    d, stg, F, r64, r32 = _forward_and_reference(N, B, p, mode)
    rows, first = [], None
    for nchunk in NCHUNKS(N):
        Bw = stg.bwd(F["saved"], nchunk)
        if first is None:
            first = Bw
        assert _bits(Bw["dAB"], first["dAB"]) and _bits(Bw["dkey"], first["dkey"]), f"nchunk {nchunk}: other bits of dA / B or dkey than nchunk 1"
        rows += _bwd_rows(Bw, r64, r32, p, f"nchunk {nchunk} ", ("dkey", "dquery", "dh", "dwk", "dwq"))
    _judge(f"FRONT nchunk {(N, B, p, mode)}", rows)


@pytest.mark.parametrize("N", MASK_NS)
def test_dropout_mask_is_the_host_philox_map(N):
    from stemgnn_amd import _lib

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    B = 3 if N <= 512 else 2
    for seed in MASK_SEEDS:
        seedt = _seed_tensor(*seed)
        for p in MASK_PS:
            m = _Buf(B * N * N)
            assert lib.stemgnn_dropout_mask(p, seedt.data_ptr(), B, N, m.ptr(), st) == 0
            torch.cuda.synchronize()
            assert m.intact(), "dropout_mask wrote behind the mask"
            got = m.t.view(B, N, N)
            want = torch.from_numpy(philox_ref.dropout_mask(p, seed[0], seed[1], B, N)).to(DEV)
            assert _bits(got, want), (N, hex(seed[0]), hex(seed[1]), p, int((got != want).sum()))
            if p == 0.0:
                assert bool((got == 1).all())


def test_dropout_seed_next():
    from stemgnn_amd import _lib

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for key, off in ((SEED, 5), (SEED, 0xFFFFFFFF), (0xFFFFFFFF00000001, (1 << 32) + 0xFFFFFFFF)):
        seed = _seed_tensor(key, off)
        used = torch.full((2,), -1, dtype=torch.int64, device=DEV)
        assert lib.stemgnn_dropout_seed_next(seed.data_ptr(), used.data_ptr(), st) == 0
        torch.cuda.synchronize()
        as_u64 = lambda t: [int(v) for v in t.cpu().numpy().view(np.uint64)]
        assert as_u64(used) == [key, off], "used != the old seed"
        assert as_u64(seed) == [key, off + 1], "the offset did not increment (carry out of the low word included)"
        # the pair the forward would read draws the mask of the OLD offset
        got = torch.empty(2 * 65 * 65, device=DEV)
        assert lib.stemgnn_dropout_mask(0.5, used.data_ptr(), 2, 65, got.data_ptr(), st) == 0
        torch.cuda.synchronize()
        assert _bits(got.view(2, 65, 65), torch.from_numpy(philox_ref.dropout_mask(0.5, key, off, 2, 65)).to(DEV))


def _cheb(N, monkeypatch, phased):
    from oracle import stemgnn_oracle as O
    from stemgnn_amd import _lib

    lib = _lib.load()
    if phased:
        monkeypatch.delenv("STEMGNN_GRAPH_PHASED", raising=False)
    else:
        monkeypatch.setenv("STEMGNN_GRAPH_PHASED", "0")
    st = torch.cuda.current_stream().cuda_stream
    g = torch.Generator().manual_seed(N)
    nn = N * N
    L = (torch.randn(N, N, generator=g) / N ** 0.5).to(DEV)
    mul_L_b = (torch.randn(4, N, N, generator=g) / N ** 0.5).to(DEV)
    dmul_L = torch.randn(4, N, N, generator=g).to(DEV)

    def fwd():
        m = _Buf(4 * nn)
        m.t[nn:2 * nn] = L.reshape(-1)
        assert lib.stemgnn_cheb_fwd(m.ptr(), N, st) == 0
        torch.cuda.synchronize()
        assert m.intact(), "cheb_fwd wrote behind mul_L"
        return m.t.view(4, N, N)

    def bwd():
        mb, db, dL, scr = _Buf(4 * nn), _Buf(4 * nn), _Buf(nn), _Buf(2 * nn)
        mb.t.copy_(mul_L_b.reshape(-1))
        db.t.copy_(dmul_L.reshape(-1))
        mb.t[:nn] = float("nan")                 # slot 0 of either input is never read
        db.t[:nn] = float("nan")
        assert lib.stemgnn_cheb_bwd(mb.ptr(), db.ptr(), dL.ptr(), scr.ptr(), N, st) == 0
        torch.cuda.synchronize()
        assert all(b.intact() for b in (mb, db, dL, scr)), "cheb_bwd wrote behind a buffer"
        return dL.t.view(N, N), scr.t.view(2, N, N)

    T = fwd()
    assert _all_nan(T[0]) and _bits(T[1], L), "cheb_fwd touched slot 0 or slot 1"
    assert _bits(fwd(), T), "cheb_fwd differs from launch to launch"
    dL, scr = bwd()
    dL2, scr2 = bwd()
    assert _bits(dL2, dL) and _bits(scr2, scr), "cheb_bwd differs from launch to launch"
    ref = {}
    for dt in (torch.float64, torch.float32):
        T_ref = O.cheb_polynomial(L.to(dt))
        Lb, T2 = mul_L_b[1].to(dt), mul_L_b[2].to(dt)
        dT1, dT2, dT3 = (dmul_L[k].to(dt) for k in (1, 2, 3))
        dLp = dT1 - dT3 + 2 * dT3 @ T2.T
        dT2p = dT2 + 2 * Lb.T @ dT3
        ref[dt] = dict(T2=T_ref[2], T3=T_ref[3], dLp=dLp, dT2p=dT2p, dL=dLp + 2 * (dT2p @ Lb.T + Lb.T @ dT2p))
    r64, r32 = ref[torch.float64], ref[torch.float32]
    got = dict(T2=T[2], T3=T[3], dLp=scr[0], dT2p=scr[1], dL=dL)
    rows = [(q, _relerr(got[q], r64[q]), _relerr(r32[q], r64[q])) for q in got]
    _judge(f"CHEB N={N} phased={int(phased)}", rows, K_CHEB, TOL_CHEB)
    return T, dL, scr


@pytest.mark.parametrize("N", CHEB_NS)
def test_cheb_vs_fp64(N, monkeypatch):
    _cheb(N, monkeypatch, True)


def test_cheb_generic_launch_vs_fp64(monkeypatch):
    """STEMGNN_GRAPH_PHASED=0: the generic launch of the first backward product, below N = 512 where the switch applies"""
    on = _cheb(CHEB_GENERIC_N, monkeypatch, True)
    off = _cheb(CHEB_GENERIC_N, monkeypatch, False)
    assert all(_bits(a, b) for a, b in zip(on, off)), "STEMGNN_GRAPH_PHASED=0: other bits (same MFMA stream promised)"


def test_front_abi_errors():
    """Return codes only: every refused call comes back before anything is launched (all buffers are real and large enough)."""
    N, B, nchunk = 5, 3, 4
    d = _draws(N, B, "rand")
    stg = _Stage(d, N, B, 0.5, (SEED, OFFSET))
    lib, st, sp = stg.lib, stg.st, stg.seed.data_ptr()
    saved, att, mul_L = _Buf(lib.stemgnn_attn_saved_floats(B, N)), _Buf(N * N), _Buf(4 * N * N)
    scr, dh, dwk, dwq, bn = _Buf(lib.stemgnn_attn_scratch_floats(B, N, nchunk)), _Buf(N * B * N), _Buf(N), _Buf(N), _Buf(B * N)

    def fwd(**kw):
        a = dict(h=stg.h.ptr(), wk=stg.wk.ptr(), wq=stg.wq.ptr(), alpha=ALPHA, p=0.5, training=1, seed=sp, B=B, N=N,
                 saved=saved.ptr(), att=att.ptr(), mul_L=mul_L.ptr(), parts=3)
        a.update(kw)
        return lib.stemgnn_attn_laplacian_fwd(*a.values(), st)

    def bwd(**kw):
        a = dict(dL=stg.dL.ptr(), h=stg.h.ptr(), wk=stg.wk.ptr(), wq=stg.wq.ptr(), alpha=ALPHA, p=0.5, training=1, seed=sp, B=B,
                 N=N, saved=saved.ptr(), scr=scr.ptr(), nchunk=nchunk, dh=dh.ptr(), dwk=dwk.ptr(), dwq=dwq.ptr(), parts=3)
        a.update(kw)
        return lib.stemgnn_attn_laplacian_bwd(*a.values(), st)

    bad_fwd = [dict(h=None), dict(wk=None), dict(wq=None), dict(saved=None), dict(att=None), dict(mul_L=None), dict(B=0), dict(N=0),
               dict(parts=0), dict(parts=4), dict(seed=None), dict(p=-0.1), dict(p=1.0), dict(p=1.5), dict(p=float("nan"))]
    for kw in bad_fwd:
        assert fwd(**kw) == SG_EINVAL, ("fwd", kw)
    bad_bwd = [dict(dL=None), dict(h=None), dict(wk=None), dict(wq=None), dict(saved=None), dict(scr=None), dict(dh=None),
               dict(dwk=None), dict(dwq=None), dict(B=0), dict(N=0), dict(nchunk=0), dict(nchunk=-1), dict(parts=0), dict(parts=4),
               dict(parts=12), dict(seed=None), dict(p=-0.1), dict(p=1.0), dict(p=1.5), dict(p=float("nan"))]
    for kw in bad_bwd:
        assert bwd(**kw) == SG_EINVAL, ("bwd", kw)
    torch.cuda.synchronize()
    for b in (saved, att, mul_L, scr, dh, dwk, dwq):
        assert _all_nan(b.t) and b.intact(), "a refused call wrote"
    # the same arguments are accepted once they are good (the refusals above are not an accident of the base call)
    assert fwd() == 0 and bwd() == 0 and fwd(seed=None, p=0.0) == 0 and fwd(seed=None, training=0) == 0
    assert bwd(parts=3 | 4, dh=None, dwk=None, dwq=None) == 0
    torch.cuda.synchronize()
    one = lambda f, *a: f(*a, st)
    assert one(lib.stemgnn_attn_dquery_reduce, None, B, N, nchunk, bn.ptr()) == SG_EINVAL
    assert one(lib.stemgnn_attn_dquery_reduce, scr.ptr(), B, N, 0, bn.ptr()) == SG_EINVAL
    assert one(lib.stemgnn_attn_dquery_reduce, scr.ptr(), 0, N, nchunk, bn.ptr()) == SG_EINVAL
    for a in ((None, scr.ptr(), dwk.ptr(), dwq.ptr()), (stg.h.ptr(), None, dwk.ptr(), dwq.ptr()), (stg.h.ptr(), scr.ptr(), None, dwq.ptr()),
              (stg.h.ptr(), scr.ptr(), dwk.ptr(), None)):
        assert one(lib.stemgnn_keyquery_wgrad, *a, B, N) == SG_EINVAL
    assert one(lib.stemgnn_keyquery_wgrad, stg.h.ptr(), scr.ptr(), dwk.ptr(), dwq.ptr(), B, 0) == SG_EINVAL
    for i in range(5):
        a = [stg.h.ptr(), bn.ptr(), bn.ptr(), dwk.ptr(), dwq.ptr()]
        a[i] = None
        assert one(lib.stemgnn_keyquery_wgrad2, *a, B, N) == SG_EINVAL
    assert one(lib.stemgnn_dropout_seed_next, sp, sp) == SG_EINVAL, "seed == used"
    assert one(lib.stemgnn_dropout_seed_next, None, sp) == SG_EINVAL and one(lib.stemgnn_dropout_seed_next, sp, None) == SG_EINVAL
    assert one(lib.stemgnn_dropout_mask, 0.5, None, B, N, att.ptr()) == SG_EINVAL
    assert one(lib.stemgnn_dropout_mask, 0.5, sp, B, N, None) == SG_EINVAL
    assert one(lib.stemgnn_cheb_fwd, None, N) == SG_EINVAL and one(lib.stemgnn_cheb_fwd, mul_L.ptr(), 0) == SG_EINVAL
    for i in range(4):
        a = [mul_L.ptr(), mul_L.ptr(), att.ptr(), scr.ptr()]
        a[i] = None
        assert one(lib.stemgnn_cheb_bwd, *a, N) == SG_EINVAL
    assert one(lib.stemgnn_cheb_bwd, mul_L.ptr(), mul_L.ptr(), att.ptr(), scr.ptr(), 0) == SG_EINVAL


def test_front_refuses_an_n_whose_lds_does_not_fit():
    """include/stemgnn_hip.h: ceil(B / min(B, 8)) + 4 N <= 16384.  The refusal comes before the key / query launch: `saved`
    (sized for the refused shape, so that nothing is out of bounds whatever the call does) stays NaN."""
    from stemgnn_amd import _lib

    lib = _lib.load()
    st = torch.cuda.current_stream().cuda_stream
    for N, B in ((4096, 1), (4095, 33)):
        h, w = torch.zeros(N * B * N, device=DEV), torch.zeros(N, device=DEV)
        saved, att, mul_L = _Buf(lib.stemgnn_attn_saved_floats(B, N)), _Buf(N * N), _Buf(4 * N * N)
        for parts in (1, 3):
            rc = lib.stemgnn_attn_laplacian_fwd(h.data_ptr(), w.data_ptr(), w.data_ptr(), ALPHA, 0.0, 1, None, B, N, saved.ptr(),
                                                att.ptr(), mul_L.ptr(), parts, st)
            assert rc == SG_EINVAL, (N, B, parts, rc)
        torch.cuda.synchronize()
        assert _all_nan(saved.t[: 3 * B * N]) and _all_nan(att.t) and saved.intact(), "the refused forward had launched already"
        del h, saved, att, mul_L
    # the largest allowed shape of four batches per chunk (4 + 4 * 4095 floats = 64 KiB exactly) is accepted and runs: every row
    # of A sums to 1 without dropout
    N, B = 4095, 25
    g = torch.Generator(device=DEV).manual_seed(4095)
    h = _Buf(N * B * N)
    torch.randn(N * B * N, generator=g, device=DEV, out=h.t)
    h.t.tanh_()
    w = torch.randn(2, N, generator=g, device=DEV) * 2 / math.sqrt(N)
    saved, att, mul_L = _Buf(lib.stemgnn_attn_saved_floats(B, N)), _Buf(N * N), _Buf(4 * N * N)
    rc = lib.stemgnn_attn_laplacian_fwd(h.ptr(), w[0].data_ptr(), w[1].data_ptr(), ALPHA, 0.0, 1, None, B, N, saved.ptr(), att.ptr(),
                                        mul_L.ptr(), 3, st)
    assert rc == 0, ("the largest allowed N is refused", N, B, rc)
    torch.cuda.synchronize()
    assert saved.intact() and att.intact() and mul_L.intact() and h.intact()
    deg = saved.t[3 * B * N + N * N: 3 * B * N + N * N + N]
    a = att.t.view(N, N)
    assert float((deg - 1).abs().max()) < 1e-5 and torch.equal(a, a.T) and bool(torch.isfinite(mul_L.t[N * N:2 * N * N]).all())
