"""GPU: every launch path of the GRU front (csrc/gru.hip) against the fp64 cell, one case per kernel instantiation.

GRU_CASES is (B, Hd, W) with S = Hd, as the model runs it; tests/test_gru_paths.py proves on the CPU (stemgnn_gru_paths,
the launchers' own plan) that the list reaches every reachable forward (family, PF, KF), every backward (family, P, KU,
slices), both input projections, folded / GEMM dW_ih, the three dW_hh forms, per-row dW_ih slabs beyond 32, the wide
cluster's pass shapes and the residency edge B * P == 224.  GRU_STEP_CASES is (B, S, Hd, W) with fewer steps than one
progress chunk of four, which only the C ABI can ask for.

Per case: fp32 draws of x, the four parameters and dh from a seeded generator; reference = oracle.gru_manual in fp64 on
the same values, on the device (pinned to ATen's GRU by tests/test_oracle_golden.py).  Every call goes through the C ABI
with h_ext, reserve, both scratch buffers and every output filled with NaN beforehand, and the device status word must
be 0 behind each.

Tolerances.  Hard bar: relerr < 1e-4 (max-norm relative, tests/util.relerr) against fp64.  Rounding-class bar: with e_ref
the relerr of an fp32 evaluation of the same cell (torch's CPU nn.GRU, or the fp32 gru_manual on the device where the CPU
would need minutes) against the fp64 run, e_kernel <= K * max(e_ref, 2^-22); the floor is four fp32 ulps of the largest
element, so a lucky e_ref cannot ask for more than fp32 holds.  Why a factor at all: the kernels sum each Hd-long mat-vec
in P slices x waves instead of one dot product and evaluate the gates with compensated hardware transcendentals -- a small
factor, not orders; a wrong slice, a missing column, a stale tag or a wrong slab count is O(1e-3) and up.

K = 8: the worst ratio e_kernel / max(e_ref, 2^-22) measured on an MI355X (256 CUs) over all 51 cases, rounded up to the
next power of two.  Worst ratio per quantity (the case that gave it):

    quantity   materialised dh           rank2 / rank2_dq (flags 0)    rank2_dq flags 1 (split-bf16 dW_hh | db_hh)
    h          1.06 (5, 321, 16)
    dx         1.71 (64, 228, 12)        1.52 (33, 66, 12)             1.52
    dW_ih      1.41 (5, 321, 16)         1.31 (40, 200, 12)            1.31
    dW_hh      5.04 (225, 40, 4)         3.45 (224, 64, 3)             0.78 of 2^-16 (1, 64, 3): 1.2e-5
    db_ih      2.14 (32, 358, 12)        3.55 (37, 384, 12)            3.55
    db_hh      5.20 (225, 40, 4)         4.41 (224, 64, 3)             0.35 of 2^-16 (1, 64, 3): 5.4e-6
    dquery sum                           0.37 (5, 33, 7)

(the two largest, 5.0 / 5.2, are the streaming kernels' 225-row weight-gradient sums; every per-row cluster and the wide
cluster stay below 4.5.)  The split-bf16 product (flags 1) takes 2^-16 as its floor for BOTH of its outputs: dW_hh | db_hh
is one product, db_hh its ones column, and csrc/wgrad.h splits every operand value into bf16 hi + lo (16 mantissa bits) and
drops lo x lo -- a 2^-16-class error per product whatever the other operand is (against 2^-22, db_hh measures up to 21).
Everything else of that call is exact fp32 and takes the fp32 floor.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
TOL = 1e-4
K = 8
FLOOR = 2.0 ** -22
FLOOR_BF16 = 2.0 ** -16
NCHUNK = 3
DEV = "cuda:0"

GRU_CASES = [
    # new ground: P = 8 kernels, B > 32 forward clusters, per-row slabs beyond 32, the residency rule's fallbacks and edge
    (3, 385, 12), (2, 448, 20), (4, 512, 16), (28, 512, 12), (40, 60, 5), (33, 30, 12), (48, 100, 12), (36, 97, 3),
    (40, 200, 12), (40, 201, 12), (37, 256, 7), (56, 228, 12), (57, 228, 12), (64, 228, 12), (44, 320, 9), (37, 384, 12),
    (224, 64, 3), (225, 40, 4), (120, 100, 12),
    # the remaining forward (PF, KF) of B > 32 (PF = 1, 2, 4: the backward's P) and of 239 <= Hd <= 290 (PF = 7 at 40
    # columns, PF = 5), the backward (P, KU) they bring, and 112 * 2 == 224
    (35, 34, 4), (50, 40, 12), (34, 45, 16), (33, 55, 8), (33, 66, 12), (64, 80, 12), (40, 90, 17), (112, 128, 12),
    (33, 130, 6), (36, 150, 12), (50, 192, 12), (34, 270, 12), (8, 260, 12),
    # the shapes of test_gru_fwd_bwd_vs_torch_cpu, the six-workgroup and the wide test (tests/test_hip_gru_eigh.py)
    (32, 228, 12), (5, 33, 7), (3, 140, 12), (2, 300, 4), (9, 358, 12), (1, 64, 3), (4, 307, 12),
    (32, 358, 12), (3, 384, 5), (2, 330, 20), (5, 321, 16),
    (8, 1024, 12), (16, 2048, 48), (20, 600, 12), (2, 1500, 4), (16, 513, 3),
]
GRU_STEP_CASES = [(5, 1, 96, 12), (5, 3, 228, 12), (40, 7, 200, 5)]
ALL_CASES = [(B, Hd, Hd, W) for B, Hd, W in GRU_CASES] + GRU_STEP_CASES


def _relerr(got, ref):
    """tests/util.relerr on the device: max|got - ref| / max|ref| (NaN if got holds one)."""
    ref = ref.double()
    d = (got.double() - ref).abs().max().item()
    den = ref.abs().max().item()
    return d / den if den > 0 else d


def _draws(B, S, Hd, W):
    g = torch.Generator().manual_seed(1000003 * B + 1009 * S + 31 * Hd + W)
    k = 1.0 / math.sqrt(Hd)                                  # nn.GRU's own initial range
    u = lambda *s: (torch.rand(*s, generator=g) * 2 - 1) * k
    t = dict(x=torch.randn(B, W, S, generator=g), w_ih=u(3 * Hd, W), w_hh=u(3 * Hd, Hd), b_ih=u(3 * Hd), b_hh=u(3 * Hd),
             dh=torch.randn(S, B, Hd, generator=g), dkey=torch.randn(B, Hd, generator=g),
             dqpart=torch.randn(B, NCHUNK, Hd, generator=g), wk=torch.randn(S, generator=g), wq=torch.randn(S, generator=g))
    return {k_: v.contiguous() for k_, v in t.items()}


def _cell(t, dhs, dtype, where):
    """h and, per output gradient in `dhs`, (dx, dw_ih, dw_hh, db_ih, db_hh) of the written-out cell in `dtype` on `where`."""
    from oracle import stemgnn_oracle as O

    x = t["x"].to(where, dtype).requires_grad_(True)
    prm = [t[n].to(where, dtype).requires_grad_(True) for n in ("w_ih", "w_hh", "b_ih", "b_hh")]
    out = O.gru_manual(x.permute(2, 0, 1), *prm)
    grads = [torch.autograd.grad(out, [x] + prm, dh.to(where, dtype), retain_graph=True) for dh in dhs]
    return out.detach(), grads


def _aten_cpu(t, dhs):
    """the same through torch's own fp32 CPU nn.GRU."""
    B, W, S = t["x"].shape
    Hd = t["w_hh"].shape[1]
    gru = torch.nn.GRU(W, Hd)
    with torch.no_grad():
        for n in ("w_ih", "w_hh", "b_ih", "b_hh"):
            getattr(gru, {"w_ih": "weight_ih_l0", "w_hh": "weight_hh_l0", "b_ih": "bias_ih_l0", "b_hh": "bias_hh_l0"}[n]).copy_(t[n])
    x = t["x"].clone().requires_grad_(True)
    out, _ = gru(x.permute(2, 0, 1).contiguous())
    prm = [gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0]
    grads = [torch.autograd.grad(out, [x] + prm, dh.cpu().float(), retain_graph=True) for dh in dhs]
    return out.detach(), grads


class _Abi:
    """The GRU entries of the C ABI on NaN-filled buffers, the status word checked behind every call."""

    def __init__(self, t, B, S, Hd, W):
        from stemgnn_amd import _lib
        from stemgnn_amd.ops import gru_status

        self.lib, self.B, self.S, self.Hd, self.W = _lib.load(), B, S, Hd, W
        self.d = {k: v.to(DEV) for k, v in t.items()}
        self.status = gru_status(torch.device(DEV))
        self.st = torch.cuda.current_stream().cuda_stream
        self.ngate = 4 * S * B * Hd                          # dgi [S*B, 3 Hd] | dghn [S*B, Hd] at offset 0 of the scratch

    def nan(self, n):
        return torch.full((int(n),), float("nan"), device=DEV)

    def done(self, rc, what):
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        assert int(self.status.item()) == 0, f"{what}: device status word {int(self.status.item())}"

    def fwd(self, infer=False):
        B, S, Hd, W, d, lib = self.B, self.S, self.Hd, self.W, self.d, self.lib
        h_ext = self.nan((S + 1) * B * Hd).view(S + 1, B, Hd)
        scr = self.nan(lib.stemgnn_gru_fwd_scratch_floats(B, S, Hd))
        head = (d["x"].data_ptr(), d["w_ih"].data_ptr(), d["w_hh"].data_ptr(), d["b_ih"].data_ptr(), d["b_hh"].data_ptr(),
                B, S, Hd, W, scr.data_ptr(), h_ext.data_ptr())
        if infer:
            self.done(lib.stemgnn_gru_fwd_infer(*head, self.status.data_ptr(), self.st), "gru_fwd_infer")
            return h_ext, None
        reserve = self.nan(lib.stemgnn_gru_reserve_floats(B, S, Hd))
        self.done(lib.stemgnn_gru_fwd(*head, reserve.data_ptr(), self.status.data_ptr(), self.st), "gru_fwd")
        return h_ext, reserve

    def bwd(self, how, h_ext, reserve, dq=None, flags=0):
        """how: 'dh' | 'rank2' | 'rank2_dq' | 'recur' | 'rank2_recur' -> (gate gradients, dx, [dw_ih, dw_hh, db_ih, db_hh] or None)"""
        B, S, Hd, W, d, lib = self.B, self.S, self.Hd, self.W, self.d, self.lib
        scr = self.nan(lib.stemgnn_gru_bwd_scratch_floats(B, S, Hd, W))
        out = [self.nan(3 * Hd * W).view(3 * Hd, W), self.nan(3 * Hd * Hd).view(3 * Hd, Hd), self.nan(3 * Hd), self.nan(3 * Hd)]
        mid = (d["x"].data_ptr(), d["w_hh"].data_ptr(), h_ext.data_ptr(), reserve.data_ptr(), B, S, Hd, W, scr.data_ptr())
        outs = tuple(o.data_ptr() for o in out)
        tail = (self.status.data_ptr(), self.st)
        fac = (d["wk"].data_ptr(), d["wq"].data_ptr())
        if how == "dh":
            rc = lib.stemgnn_gru_bwd(d["dh"].data_ptr(), *mid, *outs, *tail)
        elif how == "recur":
            rc = lib.stemgnn_gru_bwd_recur(d["dh"].data_ptr(), *mid, *tail)
        elif how == "rank2":
            rc = lib.stemgnn_gru_bwd_rank2(d["dkey"].data_ptr(), dq.data_ptr(), *fac, *mid, *outs, *tail)
        elif how == "rank2_dq":
            rc = lib.stemgnn_gru_bwd_rank2_dq(d["dkey"].data_ptr(), dq.data_ptr(), NCHUNK, flags, *fac, *mid, *outs, *tail)
        elif how == "rank2_recur":
            rc = lib.stemgnn_gru_bwd_rank2_recur(d["dkey"].data_ptr(), dq.data_ptr(), NCHUNK, *fac, *mid, *tail)
        else:
            raise ValueError(how)
        self.done(rc, "gru_bwd " + how)
        dx = self.nan(B * W * S).view(B, W, S)
        rc = lib.stemgnn_gru_input_grad(scr.data_ptr(), d["w_ih"].data_ptr(), B, S, Hd, W, dx.data_ptr(), self.st)
        self.done(rc, "gru_input_grad")
        return scr[: self.ngate].clone(), dx, (None if "recur" in how else out)


def _plan_text(p):
    from stemgnn_amd._lib import SG_GRU_FAM, SG_GRU_HH

    fam = {v: k for k, v in SG_GRU_FAM.items()}
    hh = {v: k for k, v in SG_GRU_HH.items()}
    s = f"fwd {fam[p['fwd_family']]}"
    if p["fwd_P"]:
        s += f" P{p['fwd_P']} K{p['fwd_K']}"
    s += f" gi {'stream' if p['gi_stream'] else 'gemm'} | bwd {fam[p['bwd_family']]}"
    if p["bwd_P"]:
        s += f" P{p['bwd_P']} KU{p['bwd_KU']} x{p['bwd_slices']}"
    if p["wide_passes"]:
        s += f" passes {p['wide_passes']} MT{p['wide_MT']} GW {p['wide_GWf']}/{p['wide_GWb']}"
    return s + f" dW_ih {'folded' if p['ih_folded'] else 'gemm'} {p['ih_slabs']} slabs, dW_hh {hh[p['hh_form']]}, rank2 {p['rank2_ok']}"


@pytest.mark.parametrize("B,S,Hd,W", ALL_CASES, ids=[f"B{B}-S{S}-Hd{Hd}-W{W}" for B, S, Hd, W in ALL_CASES])
def test_gru_path_vs_fp64_cell(B, S, Hd, W, monkeypatch):
    from stemgnn_amd import _lib

    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE", "STEMGNN_GRU_WHH_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    # 1. this device plans what the case list was proved against (256 CUs): another CU count reports the lost path by name
    plan = _lib.gru_paths(B, S, Hd, W, 0)
    at256 = _lib.gru_paths(B, S, Hd, W, 256)
    assert plan == at256, f"this device no longer proves the path of {(B, S, Hd, W)}: {_plan_text(plan)} != {_plan_text(at256)}"
    rank2 = bool(plan["rank2_ok"])
    assert rank2 == bool(_lib.load().stemgnn_gru_bwd_rank2_ok(B, Hd))

    t = _draws(B, S, Hd, W)
    abi = _Abi(t, B, S, Hd, W)
    # 2. forward, inference forward
    h_ext, reserve = abi.fwd()
    assert float(h_ext[0].abs().max()) == 0.0, "slab 0 (h_{-1}) is not zero behind the forward"
    h = h_ext[1:]
    h_inf, _ = abi.fwd(infer=True)
    assert torch.equal(h_inf, h_ext), "stemgnn_gru_fwd_infer: other bits than stemgnn_gru_fwd"
    # 3. materialised dh; 5. the recurrence alone leaves the same bits
    gates, dx, grads = abi.bwd("dh", h_ext, reserve)
    gates_r, dx_r, _ = abi.bwd("recur", h_ext, reserve)
    assert torch.equal(gates_r, gates) and torch.equal(dx_r, dx), "stemgnn_gru_bwd_recur: other gate gradients / dx"
    got = {"dh": (h, dx, grads)}
    dhs = [t["dh"]]
    dq_sum = None
    if rank2:
        # 4. the factored output gradient; dquery as NCHUNK partials first, so that the other calls see the kernel's own sum
        dq = torch.cat([abi.nan(B * Hd), abi.d["dqpart"].reshape(-1)])
        g_dq, dx_dq, grads_dq = abi.bwd("rank2_dq", h_ext, reserve, dq=dq)
        dq_sum = dq[: B * Hd].clone().view(B, Hd)
        g_rr, dx_rr, _ = abi.bwd("rank2_recur", h_ext, reserve, dq=dq)
        assert torch.equal(g_rr, g_dq) and torch.equal(dx_rr, dx_dq), "stemgnn_gru_bwd_rank2_recur: other gate gradients / dx"
        _, dx_2, grads_2 = abi.bwd("rank2", h_ext, reserve, dq=dq_sum)
        _, dx_b, grads_b = abi.bwd("rank2_dq", h_ext, reserve, dq=dq, flags=1)
        got.update(rank2_dq=(h, dx_dq, grads_dq), rank2=(h, dx_2, grads_2), rank2_bf16=(h, dx_b, grads_b))
        dhs.append(t["dkey"].double()[None] * t["wk"].double()[:, None, None]
                   + dq_sum.cpu().double()[None] * t["wq"].double()[:, None, None])
    # 6. a second run has the same bits
    h_ext2, reserve2 = abi.fwd()
    assert torch.equal(h_ext2, h_ext) and torch.equal(reserve2.view(torch.int32), reserve.view(torch.int32)), \
        "forward differs from launch to launch"
    _, dx2, grads2 = abi.bwd("dh", h_ext2, reserve2)
    assert torch.equal(dx2, dx) and all(torch.equal(a, b) for a, b in zip(grads2, grads)), "backward differs from launch to launch"

    # references: fp64 cell on the device; fp32: ATen's CPU GRU where that takes seconds, else the fp32 cell on the device
    dhs = [dh.to(DEV) for dh in dhs[1:]]
    dhs.insert(0, abi.d["dh"])
    h64, g64 = _cell(abi.d, dhs, torch.float64, DEV)                 # (the draws are on the device already)
    if S * B * Hd * Hd <= 4e8:
        h32, g32 = _aten_cpu(t, dhs)
    else:
        h32, g32 = _cell(abi.d, dhs, torch.float32, DEV)
    names = ("dx", "dW_ih", "dW_hh", "db_ih", "db_hh")
    rows = []            # (label, quantity, e_kernel, e_ref, floor)
    rows.append(("fwd", "h", _relerr(h, h64), _relerr(h32.to(DEV), h64), FLOOR))
    if dq_sum is not None:
        ref = t["dqpart"].double().sum(1)
        rows.append(("rank2_dq", "dquery", _relerr(dq_sum.cpu(), ref), _relerr(t["dqpart"].sum(1), ref), FLOOR))
    for label, (_, dxk, gk) in got.items():
        i = 0 if label == "dh" else 1
        for q, mine, r64, r32 in zip(names, [dxk] + gk, g64[i], g32[i]):
            floor = FLOOR_BF16 if (label == "rank2_bf16" and q in ("dW_hh", "db_hh")) else FLOOR
            rows.append((label, q, _relerr(mine, r64), _relerr(r32.to(DEV), r64), floor))
    worst = max(rows, key=lambda r: (r[2] / max(r[3], r[4])) if r[2] == r[2] else float("inf"))
    line = (f"GRU {(B, S, Hd, W)}: {_plan_text(plan)} | worst ratio {worst[2] / max(worst[3], worst[4]):.2f} "
            f"({worst[0]} {worst[1]}: e_kernel {worst[2]:.2e}, e_ref {worst[3]:.2e})")
    print(line)
    for label, q, ek, er, floor in rows:
        print(f"    {label:10s} {q:6s} e_kernel {ek:.2e} e_ref {er:.2e} ratio {ek / max(er, floor):.2f}")
    bad = [(label, q, ek, er) for label, q, ek, er, floor in rows if not (ek < TOL and ek <= K * max(er, floor))]
    assert not bad, bad
