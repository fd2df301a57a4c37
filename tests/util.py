"""Shared helpers for the test-suite (test infrastructure)."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def hash_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 9973


def load_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    N, W, m, H, B, mode = (int(v) for v in z["cfg"])
    cfg = dict(N=N, W=W, multi=m, H=H, B=B, mode={0: "eval", 1: "train", 2: "mask"}[mode])
    return z, cfg


def relerr(got, ref):
    """norm-relative error used throughout: max|got-ref| / max|ref|."""
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    den = ref.abs().max().item()
    num = (got - ref).abs().max().item()
    return num / den if den > 0 else num


def sign_sketch(a, k=64, seed=7):
    """k random +-1 projections of a flattened tensor (float64), the signs from oracle/detrand.py.  For a difference d
    of two tensors, mean(sketch(d)^2) estimates ||d||_2^2 without bias, and with k = 64 it falls below a quarter of it
    with negligible probability -- so a fixture can pin a large tensor through k numbers (||d||_inf <= ||d||_2)."""
    from oracle.detrand import det_uniform
    flat = torch.as_tensor(a).double().reshape(-1).numpy()
    signs = np.where(det_uniform((k, flat.size), seed) >= 0, 1.0, -1.0)
    return signs @ flat


def synthetic_series(T, N, seed):
    """sin(2 pi t / p_n + phi_n) * a_n + c_n + noise (SURVEY 8d shape), float64, from the deterministic generators of
    oracle/detrand.py (so a fixture can name a seed instead of carrying the series)."""
    from oracle.detrand import det_normalish, det_uniform
    t = np.arange(T, dtype=np.float64)[:, None]
    p = det_uniform((N,), seed, 6.0, 30.0).astype(np.float64)
    phi = det_uniform((N,), seed + 1, 0.0, 6.28).astype(np.float64)
    a = det_uniform((N,), seed + 2, 0.5, 3.0).astype(np.float64)
    c = det_uniform((N,), seed + 3, -2.0, 8.0).astype(np.float64)
    return np.sin(2 * np.pi * t / p + phi) * a + c + 0.1 * det_normalish((T, N), seed + 4).astype(np.float64)


def kink_audit(pos_impl, ref64, err, what):
    """LeakyReLU-kink audit of one set of pre-activations: `pos_impl` the implementation's decisions (which side of 0 it took
    each value to be on), `ref64` the fp64 oracle's values, `err` the implementation's measured (rounding-class) evaluation
    error of them.  A value is "near the kink" when it is smaller than twice that error; the decisions may differ from the
    fp64 ones on at most a handful of values, and only near the kink.  Returns the flips (where they differ)."""
    ref64 = ref64.double().cpu()
    pos_impl = pos_impl.cpu()
    near = ref64.abs() <= 2 * err
    flips = pos_impl != (ref64 > 0)
    n_near, n_flip = int(near.sum()), int(flips.sum())
    print(f"kink audit ({what}): fp32 error {err:.2e}; {n_near} of {ref64.numel()} values within twice that of 0, "
          f"{n_flip} decision flips")
    assert n_near <= max(16, int(2e-5 * ref64.numel())), n_near
    assert n_flip <= max(8, int(5e-7 * ref64.numel())) and bool((flips & ~near).sum() == 0), (n_flip, int((flips & ~near).sum()))
    return flips


# ---- stage suites through the C ABI (tests/test_hip_front.py, tests/test_hip_block.py): NaN-filled, guarded buffers --------------
GUARD = 256                      # floats behind every buffer
SENTINEL = -7777.25
DEV = "cuda:0"


def _relerr(got, ref):
    """tests/util.relerr on the device: max|got - ref| / max|ref| (absolute where the reference is all zero; NaN if got holds one)."""
    ref = ref.double()
    d = (got.double() - ref).abs().max().item()
    den = ref.abs().max().item()
    return d / den if den > 0 else d


def _bits(a, b):
    """same bits, NaN included"""
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _all_nan(t):
    return bool(torch.isnan(t).all())


class _Buf:
    """n floats of NaN with a guard band behind them"""

    def __init__(self, n, fill=float("nan")):
        self.n = int(n)
        self.full = torch.full((self.n + GUARD,), fill, device=DEV)
        self.full[self.n:] = SENTINEL
        self.t = self.full[: self.n]

    def ptr(self):
        return self.full.data_ptr()

    def intact(self):
        return bool((self.full[self.n:] == SENTINEL).all())


class _BufD(_Buf):
    """_Buf of doubles"""

    def __init__(self, n, fill=float("nan")):
        self.n = int(n)
        self.full = torch.full((self.n + GUARD,), fill, device=DEV, dtype=torch.float64)
        self.full[self.n:] = SENTINEL
        self.t = self.full[: self.n]


POISON_I64 = -0x0DEAD0BAD0C0FFEE          # what an int64 / int32 buffer holds before a call: no position, count or status looks like it
POISON_I32 = -0x0BADC0DE
SENTINEL_I = -77772525


class _BufI(_Buf):
    """_Buf of int64 (or int32) words: a recognisable poison in place of NaN, an integer sentinel behind them"""

    def __init__(self, n, fill=None, dtype=torch.int64):
        self.n = int(n)
        fill = (POISON_I64 if dtype == torch.int64 else POISON_I32) if fill is None else fill
        self.full = torch.full((self.n + GUARD,), fill, device=DEV, dtype=dtype)
        self.full[self.n:] = SENTINEL_I
        self.t = self.full[: self.n]

    def intact(self):
        return bool((self.full[self.n:] == SENTINEL_I).all())


# ---- csrc/layout.h in Python (tests/test_block_cases.py checks it against the stemgnn_*_floats functions) ----
def dims(B, N, W, multi):
    c16 = lambda v: (v + 15) & ~15
    Wm = W * multi
    nf = (Wm // 2 + 1, (Wm + 1) // 2 - 1)
    U = (4 * nf[0], 4 * nf[1])
    CP2 = tuple(c16(u if u > 0 else 1) for u in U)
    return SimpleNamespace(B=B, N=N, W=W, multi=multi, Wm=Wm, WmP=c16(Wm), C=4 * Wm, CP=c16(4 * Wm), KG=3 * W, M=B * N, nf=nf, U=U,
                           CP2=CP2, KF=CP2[0] + CP2[1])


def saved_layout(d):
    """name -> (offset, rows, row stride, useful columns); the order of SgSavedLayout"""
    L, off = {}, 0

    def add(name, ld, useful):
        nonlocal off
        L[name] = (off, d.M, ld, useful)
        off += d.M * ld

    add("G", d.KG, d.KG)
    for r in range(2):
        for l in range(3):
            cp, cu = (d.CP, d.C) if l < 2 else (d.CP2[r], d.U[r])
            add(f"out{r}{l}", cp, cu)
            add(f"gate{r}{l}", cp, cu)
    add("ig", d.Wm, d.Wm)
    add("fs", d.Wm, d.Wm)
    L["total"] = off
    return L


def scratch_layout(d):
    L, off = {}, 0
    for name, ld in (("dpF", d.Wm), ("dpB", d.W), ("dig", d.Wm)):
        L[name] = (off, d.M, ld, ld)
        off += d.M * ld
    off += 6 * d.M * 2 * d.CP                                   # d(pre-activation) of the six GLU layers, pair order
    L["dG"] = (off, 2 * d.M, d.KG, d.KG)
    L["total"] = off + 2 * d.M * d.KG
    return L


def l2_channels(d, r):
    """useful channel c of the last GLU layer -> channel kq * Wm + f of GLUs[4 + r] (sg_l2_orig_channel)"""
    return [(c // d.nf[r]) * d.Wm + c % d.nf[r] + (1 if r == 1 else 0) for c in range(d.U[r])]
