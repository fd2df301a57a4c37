"""GPU: the per-arrival serving entries -- stemgnn_live_push and stemgnn_ring_gather (stemgnn_amd/csrc/live.hip), stemgnn_aci_update
(csrc/aci.hip) and stemgnn_anomaly_update (csrc/anomaly.hip) -- through the C ABI on NaN-filled, guarded buffers, at the widths and
windows at which their launchers take another decision: the serving counterpart of tests/test_hip_data_stage.py.

Cases, inputs and references are in tests/test_serving_cases.py (the case table is in its docstring), which proves on the CPU, through
stemgnn_serving_plan, that the cases reach every form, tile count, tile width, row trip, span, row part, part, batch, thread class
and copy form of the launchers, and that every further trip, tile, part and batch changes the expected outputs.  The references are
tests/helpers/aci_ref.AciRef, tests/helpers/anomaly_ref.AnomalyRefFast (proved equal to AnomalyRef's loop there) and the header's
push and gather contracts in numpy; none is code under test.

Hygiene, for every call: every input and every state buffer is a guarded copy (tests/util._Buf and its kin: sentinels behind the
payload, and in front of it where the buffer sits at a 4-byte offset); outputs an entry writes in full -- pvalues, node_p, alarm,
counts and log_p[log_slot] of the anomaly entry, the gathered windows, the ring rows a push covers, t_dev -- are NaN or a junk
integer before the call; afterwards every guard is unchanged, every input has its bits, and the WHOLE of every state buffer is
compared with the reference, so the other M - 1 score slots, the other log_p rows, the ring rows outside a push, offsets and alpha
of held groups and the words of `work` beyond H N + G must be what they were; `work` is zero where a call may use it.  Every case
runs twice from the same preloaded state and both runs must agree bit for bit; a case with a buffer at a 4-byte offset must agree
bit for bit with its aligned twin.

No tolerance anywhere: k-th smallest fp32 values, integer counts, fp64 expressions of individually rounded operations and copies.
Scores, p-values, node_p, log_p and ring_y are compared as bit patterns where either side holds a number and must be NaN in the
same places (NaN = absent); offsets, ring_x and the gathered rows as bit patterns; alpha as fp64 bits; counts and sums as integers.

Findings: none.  Every case agrees with its reference on the first run, no guard was touched, and the second tile, the one-column
tile, the second and third row trips, the split spans and row parts, 64 parts and three sorted batches hold the same contract as
the toy shapes of the semantic suites."""
import ctypes

import numpy as np
import pytest
import torch

from tests import test_serving_cases as S
from tests.util import SENTINEL, SENTINEL_I, _all_nan, _Buf, _BufD, _BufI

pytestmark = pytest.mark.gpu
F32 = np.float32
JUNK_I = -0x0BADC0DE


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    return _lib.load()


class G:
    """a guarded device copy of a numpy array, `off` elements inside its allocation (fp32, off = 1: a 4-byte offset); the
    elements in front of it are sentinels like the band behind"""

    def __init__(self, a, off=0):
        a = np.ascontiguousarray(a)
        if a.dtype == np.uint32:
            a = a.view(np.int32)
        self.shape, self.dtype, self.off, self.n = a.shape, a.dtype, int(off), a.size
        n = self.n + self.off
        if a.dtype == np.float32:
            self.buf, self.sentinel = _Buf(n), SENTINEL
        elif a.dtype == np.float64:
            self.buf, self.sentinel = _BufD(n), SENTINEL
        else:
            self.buf, self.sentinel = _BufI(n, dtype={8: torch.int64, 4: torch.int32}[a.dtype.itemsize]), SENTINEL_I
        self.buf.full[:self.off] = self.sentinel
        self.view = self.buf.full[self.off:n]
        self.ptr = self.buf.full.data_ptr() + self.off * a.dtype.itemsize
        assert (self.ptr % 16 == 0) == (self.off * a.dtype.itemsize % 16 == 0)
        self.write(a)

    def write(self, a):
        a = np.ascontiguousarray(a)
        a = a.view(np.int32) if a.dtype == np.uint32 else a
        assert a.size == self.n and a.dtype == self.dtype
        self.view.copy_(torch.from_numpy(a.reshape(-1).copy()))
        self.host = a.reshape(self.shape).copy()

    def read(self, what):
        """the payload, after checking the bands around it"""
        full = self.buf.full.cpu().numpy()
        assert (full[:self.off] == self.sentinel).all() and (full[self.off + self.n:] == self.sentinel).all(), f"{what}: a guard element changed"
        return full[self.off:self.off + self.n].reshape(self.shape).copy()

    def unchanged(self, what):
        assert S.same_bits(self.read(what), self.host), f"{what}: an input changed"


def _ptr(g):
    return None if g is None else g.ptr


def _ok(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


def _check(got, want, what, nan_aware):
    want = np.asarray(want)
    if want.dtype.kind in "iu":
        assert got.dtype.kind in "iu" and np.array_equal(got.astype(np.int64), want.astype(np.int64)), what
        return
    assert got.dtype == want.dtype, what
    if not (S.same_nan_aware if nan_aware else S.same_bits)(got, want):
        bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1))
        raise AssertionError(f"{what}: {bad.size} of {got.size} differ, first at {bad[:5].tolist()}: "
                             f"{got.reshape(-1)[bad[:5]].tolist()} != {want.reshape(-1)[bad[:5]].tolist()}")


def _pair(run, c):
    """twice from the same preloaded state; a case with a misaligned buffer also against its aligned twin"""
    first, second = run(c), run(c)
    if getattr(c, "mis", 0):
        second = run(c._replace(mis=0))
    assert len(first) == len(second) > 0
    for i, (a, b) in enumerate(zip(first, second)):
        assert S.same_bits(a, b), f"{c}: buffer {i} differs between the two runs"


# ---- push ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.PUSH_CASES, ids=str)
def test_live_push(lib, c):
    d = S.push_data(c)
    want = S.push_ref(c, d)
    covered = S.push_covered(c)

    def run(c):
        ins = [G(d[k]) for k in ("raw", "sub", "div")]
        before_x, before_y = d["ring_x"].copy(), d["ring_y"].copy()
        before_x[covered], before_y[covered] = np.nan, np.nan            # what the push covers is written in full
        last, rx, ry = G(d["last"]), G(before_x), G(before_y)
        t = G(np.array([JUNK_I], dtype=np.int64))
        assert _all_nan(rx.view.view(c.C, c.N)[covered]) and _all_nan(ry.view.view(c.C, c.N)[covered])
        _ok(lib.stemgnn_live_push(ins[0].ptr, c.K, c.N, c.t0, ins[1].ptr, ins[2].ptr, c.clip01, S.MISSING, c.has_missing, last.ptr,
                                  rx.ptr, ry.ptr, c.C, t.ptr, None))
        got = dict(ring_x=rx.read("ring_x"), ring_y=ry.read("ring_y"), last=last.read("last"), t=t.read("t_dev"))
        _check(got["ring_x"], want["ring_x"], f"{c}: ring_x", False)
        _check(got["ring_y"], want["ring_y"], f"{c}: ring_y", True)
        _check(got["last"], want["last"], f"{c}: last", False)
        _check(got["t"], want["t"], f"{c}: t_dev", False)
        for k, g in zip(("raw", "sub", "div"), ins):
            g.unchanged(k)
        return list(got.values())
    _pair(run, c)


# ---- gather -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.GATHER_CASES, ids=str)
def test_ring_gather(lib, c):
    d = S.gather_data(c)
    want = S.gather_ref(c, d)

    def run(c):
        ring = G(d["ring"], off=c.mis & 1)
        starts = None if c.starts is None else G(np.asarray(c.starts, dtype=np.int64))
        t = G(np.array([c.t], dtype=np.int64))
        out = G(np.full((c.B, c.L, c.N), np.nan, dtype=F32), off=(c.mis >> 1) & 1)
        status = G(np.zeros(1, dtype=np.int32)) if c.status else None
        assert _all_nan(out.view)
        _ok(lib.stemgnn_ring_gather(ring.ptr, c.C, c.N, _ptr(starts), t.ptr, c.back, c.B, c.L, out.ptr, _ptr(status), None))
        got = out.read("out")
        _check(got, want["out"], f"{c}: out", False)
        if status is not None:
            assert int(status.read("status")[0]) == want["status"], c
        ring.unchanged("ring")
        t.unchanged("t_dev")
        if starts is not None:
            starts.unchanged("starts")
        return [got]
    _pair(run, c)


# ---- ACI ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.ACI_CASES, ids=str)
def test_aci_update(lib, c):
    d = S.aci_data(c)
    states, branches = S.aci_ref_run(c, d)
    Q, pairs, ta = S.aci_pairs(c)
    assert "select" in branches
    if c.per_node:                                                      # node 1 never has a target: its groups hold, bit for bit
        assert S.same_bits(states[-1]["alpha"][..., 1], d["alpha"][..., 1]) and S.same_bits(states[-1]["offsets"][..., 1], d["offsets"][..., 1])
    lo, hi = (ctypes.c_int * c.P)(*[p[0] for p in pairs]), (ctypes.c_int * c.P)(*[p[1] for p in pairs])
    alphas = (ctypes.c_double * c.P)(*ta)

    def run(c):
        st = dict(scores=G(d["window"], off=(c.mis >> 3) & 1), alpha=G(d["alpha"]), offsets=G(d["offsets"]),
                  counts=G(d["counts"].astype(np.int64)), miss_sum=G(d["miss_sum"].astype(np.int64)), valid_sum=G(d["valid_sum"].astype(np.int64)))
        got = []
        for k, (call, want) in enumerate(zip(d["calls"], states)):
            issued, raw, ring = G(call["issued"], off=c.mis & 1), G(call["raw"], off=(c.mis >> 1) & 1), G(call["ring"], off=(c.mis >> 2) & 1)
            slot = (d["slot0"] + k) % c.M
            _ok(lib.stemgnn_aci_update(issued.ptr, raw.ptr, ring.ptr, d["C"], call["origin"], Q, c.H, c.N, c.P, lo, hi, alphas, S.GAMMA,
                                       c.M, slot, S.MIN_SCORES, c.per_step, c.per_node, st["scores"].ptr, st["alpha"].ptr,
                                       st["offsets"].ptr, st["counts"].ptr, st["miss_sum"].ptr, st["valid_sum"].ptr, None))
            for name in S.ACI_STATE:
                g = st[name].read(name)
                _check(g, want[name], f"{c}, call {k}: {name}", name == "scores")
                got.append(g)
            issued.unchanged("issued"), raw.unchanged("raw"), ring.unchanged("ring_y")
        return got
    _pair(run, c)


# ---- anomaly ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.ANOMALY_CASES, ids=str)
def test_anomaly_update(lib, c):
    d = S.anomaly_data(c)
    states = S.anomaly_ref_run(c, d)
    words, used = S.work_words(c)
    work0 = np.zeros(words, dtype=np.int32)
    work0[used:] = S.WORK_JUNK

    def run(c):
        slab, origins = G(d["slab"]), (G(d["origins"]) if c.origins else None)
        st = dict(scores=G(d["window"], off=c.mis & 1), alarm_sum=G(d["alarm_sum"].astype(np.int64)),
                  judged_sum=G(d["judged_sum"].astype(np.int64)), log_p=G(d["log_p"]))
        work = G(work0)
        got = []
        for k, (call, want) in enumerate(zip(d["calls"], states)):
            ring = G(call["ring"])
            slot, log_slot = S.anomaly_slots(c, d, k)
            st.update(pvalues=G(np.full((c.H, c.N), np.nan, dtype=F32)), node_p=G(np.full(c.N, np.nan, dtype=F32)),
                      alarm=G(np.full(c.N, JUNK_I, dtype=np.int32)), counts=G(np.full(want["counts"].shape, JUNK_I, dtype=np.int64)))
            log = st["log_p"].read("log_p")
            log[log_slot] = np.nan
            st["log_p"].write(log)
            assert _all_nan(st["pvalues"].view) and _all_nan(st["node_p"].view) and _all_nan(st["log_p"].view.view(S.KEEP, c.N)[log_slot])
            _ok(lib.stemgnn_anomaly_update(slab.ptr, d["S"], S.AN_R, S.AN_LO, S.AN_HI, _ptr(origins), call["row"], ring.ptr, S.AN_C, c.H,
                                           c.N, c.M, slot, S.AN_MIN_SCORES, S.AN_ALPHA, c.per_step, c.per_node, st["scores"].ptr,
                                           st["pvalues"].ptr, st["node_p"].ptr, st["alarm"].ptr, st["counts"].ptr, st["alarm_sum"].ptr,
                                           st["judged_sum"].ptr, st["log_p"].ptr, S.KEEP, log_slot, work.ptr, None))
            for name in S.AN_STATE:
                g = st[name].read(name)
                _check(g, want[name], f"{c}, call {k}: {name}", True)
                got.append(g)
            assert S.same_bits(work.read("work"), work0), f"{c}, call {k}: work is not zero again, or a word beyond H N + G changed"
            ring.unchanged("ring_y"), slab.unchanged("slab")
            if origins is not None:
                origins.unchanged("origins")
        return got
    _pair(run, c)
