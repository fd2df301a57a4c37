"""CPU: the case lists of tests/test_hip_serving_stage.py (the per-arrival serving entries: stemgnn_live_push and stemgnn_ring_gather
of csrc/live.hip, stemgnn_aci_update of csrc/aci.hip, stemgnn_anomaly_update of csrc/anomaly.hip), their inputs and references, and
proof that they reach what they claim.

stemgnn_serving_plan reports, host only, what each launcher does for a shape: the form (columns, stream, pooled), the grid, the
threads, VEC, and per entry the tile widths, row trips, spans, row parts, parts and batches (include/stemgnn_hip.h).  The launchers
take their geometry from the same static functions (csrc/serving_plan.h), so every class below is decided by what the plan says,
none by a threshold copied into this file.  CLASSES names every launch decision the device suite must reach; test_class_is_reached
is parametrised over it, so taking the cases of any one class out of the lists fails that class's test.

Cases (the smallest shapes that reach a class; the largest input of the suite is 2.1 MB):
  push     (K, N, C, t0, clip01, has_missing)
             (3, 11, 8, 5, 0, 1)      one block, K < C            (8, 64, 8, 3, 1, 0)     one full block, K = C, clip, no `missing`
             (13, 150, 5, 7, 1, 1)    three blocks, ragged, K > C with t0 % C != 0
             (4, 65, 6, 0, 0, 0)      two blocks, one live lane in the last
  gather   (C, N, B, L, starts, back, t, status, misaligned)
             N = 11, 255 (64 threads), 256, 300 (128), 1024, 1027, 2052 (256); float4 and scalar, by N and by the address of
             ring / out alone; several copy trips in both forms; starts == NULL; B = 5 with held windows and a negative, a not yet
             pushed and an overwritten one; status == NULL with a window the ring does not hold
  aci      (H, N, P, M, per_step, per_node, calls, misaligned)
             columns: (2, 11, 2, 5) one ragged tile of 22 (64 mod 22 != 0) | (1, 32, 1, 40) a full tile, two row trips |
             (3, 32, 1, 22, per_step = 0) a full tile, three trips, Hr = H | (1, 33, 1, 2050) a last tile of one column, three
             trips of its 1024-row step | (1, 70, 1, 4) three tiles, ragged | (33, 32, 1, 2, per_step = 0) two trips of the origin's
             scoring.   stream: float4 / scalar by N, scalar by the address of each of the four buffers alone, kept and streamed
             windows in both, L below one trip with a streamed window, L over three trips
  anomaly  (H, N, M, per_step, per_node, origins, calls, misaligned)
             columns: one launch with three population trips for both per_step, N = 32, N = 33, three ragged tiles; split with
             hspan 1 (H = 193: want < 1; H = 5, M = 520: the cap of 16; H = 5, M = 40: cut to `most`; H = 6, N = 70: inside the
             clamps), split with hspan 4 over spans of 4, 4, 2.   pooled: parts 1, 4 and 64, one batch, three batches with a last
             one of 600 queries, a last batch of one query, scalar by N and by the address of scores
Every window is PRELOADED (quarter-grid values with ties, +-inf, +-0 and about 10 % NaN in all M slots), then one to three calls
run; the first call writes the last slot, so the slot index wraps.

Sensitivity: a class that says "a further trip, tile, part, batch or block" must matter.  For each such class the reference is
computed twice here -- in full, and with that class's share of the work left out (window rows beyond the first trip or of the
parts above 0 set absent; the last tile's, block's or batch's outputs left as they were) -- and the expected outputs must differ.

The file also proves tests/helpers/anomaly_ref.AnomalyRefFast (sort + searchsorted per group) equal to AnomalyRef's per-element loop
on the small cases, and holds the host-only refusals of the four entries that tests/test_live_abi.py, tests/test_aci_abi.py and
tests/test_anomaly_abi.py do not have, and the plan's own.

Findings: none on the CPU side.  Moving the launch arithmetic of the three files into csrc/serving_plan.h changed no decision (the
pre-existing serving suites pass with the same bits); what the device suite found is in its own docstring."""
import ctypes
import functools
import os
from collections import namedtuple

import numpy as np
import pytest

from tests.helpers import aci_ref, anomaly_ref

EINVAL = -10001
F32 = np.float32
SEED = 20261021
NAN_BITS = 0x7FC00000                                                   # the quiet NaN the kernels write (CF_NAN_BITS)

Push = namedtuple("Push", "K N C t0 clip01 has_missing")
Gather = namedtuple("Gather", "C N B L starts back t status mis")
Aci = namedtuple("Aci", "H N P M per_step per_node calls mis")
An = namedtuple("An", "H N M per_step per_node origins calls mis")

PUSH_CASES = [Push(3, 11, 8, 5, 0, 1), Push(8, 64, 8, 3, 1, 0), Push(13, 150, 5, 7, 1, 1), Push(4, 65, 6, 0, 0, 0)]
GATHER_CASES = [
    Gather(6, 11, 1, 4, None, 4, 9, 1, 0),
    Gather(6, 12, 5, 4, (5, -1, 6, 2, 3), 0, 9, 1, 0),                  # held, negative, not yet pushed, overwritten, held
    Gather(4, 255, 1, 4, None, 4, 4, 1, 0),
    Gather(5, 256, 2, 3, (4, 9), 0, 7, 0, 0),                          # status == NULL, the second window not held
    Gather(4, 300, 2, 2, (4, 1), 0, 6, 1, 0),
    Gather(4, 300, 2, 2, (4, 1), 0, 6, 1, 1),                          # ring at a 4-byte offset
    Gather(4, 300, 2, 2, (4, 1), 0, 6, 1, 2),                          # out at a 4-byte offset
    Gather(4, 1024, 1, 2, None, 2, 6, 1, 0),
    Gather(4, 1027, 2, 3, (3, 0), 0, 6, 1, 0),
    Gather(3, 2052, 2, 2, (4, 7), 0, 6, 1, 0),
]
ACI_CASES = [
    Aci(2, 11, 2, 5, 1, 1, 3, 0), Aci(1, 32, 1, 40, 1, 1, 2, 0), Aci(3, 32, 1, 22, 0, 1, 2, 0), Aci(1, 33, 1, 2050, 1, 1, 1, 0),
    Aci(1, 70, 1, 4, 1, 1, 2, 0), Aci(33, 32, 1, 2, 0, 1, 3, 0),
    Aci(2, 12, 1, 5, 1, 0, 3, 0), Aci(2, 11, 2, 5, 0, 0, 3, 0),
    Aci(2, 12, 1, 5, 1, 0, 2, 1), Aci(2, 12, 1, 5, 1, 0, 2, 2), Aci(2, 12, 1, 5, 1, 0, 2, 4), Aci(2, 12, 1, 5, 1, 0, 2, 8),
    Aci(3, 3000, 1, 8, 0, 0, 1, 0), Aci(2, 1501, 1, 6, 0, 0, 1, 0), Aci(1, 501, 1, 40, 1, 0, 2, 0), Aci(1, 1000, 1, 70, 1, 0, 2, 0),
]
ANOMALY_CASES = [
    An(2, 11, 70, 1, 1, 1, 3, 0), An(3, 32, 30, 0, 1, 0, 2, 0), An(4, 33, 5, 1, 1, 0, 2, 0), An(2, 70, 6, 0, 1, 0, 2, 0),
    An(193, 8, 3, 1, 1, 0, 1, 0), An(5, 8, 520, 1, 1, 0, 1, 0), An(5, 8, 40, 1, 1, 1, 2, 0), An(10, 33, 7, 0, 1, 0, 2, 0),
    An(6, 70, 330, 1, 1, 0, 1, 0),
    An(2, 12, 5, 1, 0, 1, 3, 0), An(2, 11, 5, 0, 0, 0, 2, 0), An(2, 12, 5, 1, 0, 1, 3, 1), An(2, 500, 30, 0, 0, 0, 1, 0),
    An(1, 8792, 59, 1, 0, 0, 1, 0), An(1, 4097, 3, 1, 0, 0, 2, 0),
]
CASES = {"push": PUSH_CASES, "gather": GATHER_CASES, "aci": ACI_CASES, "anomaly": ANOMALY_CASES}
GAMMA, MIN_SCORES, AN_ALPHA, AN_MIN_SCORES, KEEP = 0.05, 3, 0.2, 2, 3
MISSING = 0.0
WORK_JUNK = 0x5A5A5A5A                                                  # in the words of `work` no call may touch


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def plan_args(entry, c):
    return {"push": lambda: (c.K, c.N, c.C), "gather": lambda: (c.C, c.N, c.B, c.L),
            "aci": lambda: (c.H, c.N, c.P, c.M, c.per_step, c.per_node), "anomaly": lambda: (c.H, c.N, c.M, c.per_step, c.per_node)}[entry]()


def plan(entry, c, mis=None):
    from stemgnn_amd import _lib

    return _lib.serving_plan(entry, *plan_args(entry, c), misaligned=getattr(c, "mis", 0) if mis is None else mis)


@functools.lru_cache(maxsize=None)
def _gather_threads():
    """the thread classes of the ring gather, found by asking the plan over N = 1 .. 2048"""
    from stemgnn_amd import _lib

    return sorted({_lib.serving_plan("gather", 4, N, 1, 2)["threads"] for N in range(1, 2049)})


def _held(c):
    """per window of the call: does the ring hold it (the header's three conditions)"""
    return [0 <= s and s + c.L <= c.t and s >= c.t - c.C for s in (c.starts if c.starts is not None else (c.t - c.back,))]


def _form(p):
    from stemgnn_amd import _lib

    return {v: k for k, v in _lib.SG_SERVING_FORM.items()}[p["form"]]


def _by_address(entry, c, p, bit):
    """scalar because of ONE buffer's address: that bit alone is set, and without it the same shape runs float4"""
    return c.mis == bit and p["vec"] == 1 and plan(entry, c, 0)["vec"] == 4


# class name -> (entry, predicate(case, plan)); `lambda c, p, k=k` binds the loop value
CLASSES = {
    # ---- push
    "push/one block": ("push", lambda c, p: p["grid_x"] == 1),
    "push/two or more blocks, ragged last": ("push", lambda c, p: p["grid_x"] >= 2 and c.N % p["threads"] != 0),
    "push/K < C": ("push", lambda c, p: c.K < c.C and p["k0"] == 0),
    "push/K = C": ("push", lambda c, p: c.K == c.C and p["k0"] == 0),
    "push/K > C with t0 % C != 0, several blocks": ("push", lambda c, p: p["k0"] > 0 and c.t0 % c.C != 0 and p["grid_x"] > 1),
    "push/clip on": ("push", lambda c, p: c.clip01 == 1), "push/clip off": ("push", lambda c, p: c.clip01 == 0),
    "push/has_missing on": ("push", lambda c, p: c.has_missing == 1), "push/has_missing off": ("push", lambda c, p: c.has_missing == 0),
    # ---- gather
    "gather/two or more copy trips, float4": ("gather", lambda c, p: p["trips"] >= 2 and p["vec"] == 4),
    "gather/two or more copy trips, scalar": ("gather", lambda c, p: p["trips"] >= 2 and p["vec"] == 1),
    "gather/float4": ("gather", lambda c, p: p["vec"] == 4),
    "gather/scalar by N": ("gather", lambda c, p: p["vec"] == 1 and c.mis == 0),
    "gather/scalar by the address of ring": ("gather", lambda c, p: _by_address("gather", c, p, 1)),
    "gather/scalar by the address of out": ("gather", lambda c, p: _by_address("gather", c, p, 2)),
    "gather/starts == NULL": ("gather", lambda c, p: c.starts is None and p["grid_y"] == 1),
    "gather/held and not held windows in one call": ("gather", lambda c, p: p["grid_y"] > 1 and True in _held(c) and any(
        s < 0 for s in c.starts) and any(s >= 0 and s + c.L > c.t for s in c.starts) and any(0 <= s < c.t - c.C for s in c.starts)),
    "gather/status == NULL, a window not held": ("gather", lambda c, p: not c.status and False in _held(c)),
    # ---- ACI, column form
    "aci columns/one tile, ragged": ("aci", lambda c, p: _form(p) == "columns" and p["grid_x"] == 1 and p["Cc"] < p["tile"]),
    "aci columns/a full tile": ("aci", lambda c, p: _form(p) == "columns" and p["Cc"] >= p["tile"]),
    "aci columns/three or more tiles, ragged last": ("aci", lambda c, p: _form(p) == "columns" and p["grid_x"] >= 3 and 1 < p["wd_last"] < p["tile"]),
    "aci columns/a last tile of one column": ("aci", lambda c, p: _form(p) == "columns" and p["grid_x"] >= 2 and p["wd_last"] == 1),
    "aci columns/a tile width that does not divide 64": ("aci", lambda c, p: _form(p) == "columns" and 64 % p["wd_last"] != 0),
    "aci columns/two origin-scoring trips": ("aci", lambda c, p: _form(p) == "columns" and p["origin_trips_full"] >= 2),
    "aci columns/Hr = 1": ("aci", lambda c, p: _form(p) == "columns" and p["Hr"] == 1 < c.H),
    "aci columns/Hr = H": ("aci", lambda c, p: _form(p) == "columns" and p["Hr"] == c.H > 1),
    # ---- ACI, stream form
    "aci stream/float4": ("aci", lambda c, p: _form(p) == "stream" and p["vec"] == 4),
    "aci stream/scalar by N": ("aci", lambda c, p: _form(p) == "stream" and p["vec"] == 1 and c.mis == 0),
    "aci stream/L below one trip": ("aci", lambda c, p: _form(p) == "stream" and p["L"] < p["step_full"]),
    "aci stream/L below one trip, window streamed": ("aci", lambda c, p: _form(p) == "stream" and p["L"] < p["step_full"] and not p["keep"]),
    "aci stream/L over several scoring trips": ("aci", lambda c, p: _form(p) == "stream" and p["origin_trips_full"] >= 3),
    # ---- anomaly, column form
    "anomaly columns/N = one full tile": ("anomaly", lambda c, p: _form(p) == "columns" and c.N == p["tile"]),
    "anomaly columns/N = one tile and one node": ("anomaly", lambda c, p: _form(p) == "columns" and c.N == p["tile"] + 1),
    "anomaly columns/three or more tiles, ragged": ("anomaly", lambda c, p: _form(p) == "columns" and p["tiles"] >= 3 and c.N % p["tile"] != 0),
    "anomaly columns/split, hspan 1": ("anomaly", lambda c, p: _form(p) == "columns" and p["launches"] == 2 and p["hspan"] == 1),
    "anomaly columns/split, hspan 4, H mod 4 != 0, three spans": ("anomaly", lambda c, p: _form(p) == "columns" and p["launches"] == 2 and p["hspan"] == 4 and c.H % 4 != 0 and p["spans"] >= 3),
    "anomaly columns/rparts = 1 because want < 1": ("anomaly", lambda c, p: p["launches"] == 2 and _form(p) == "columns" and p["want"] < 1 and p["rparts"] == 1),
    "anomaly columns/rparts at its cap": ("anomaly", lambda c, p: _form(p) == "columns" and 1 < p["rparts"] < min(p["want"], p["most"])),
    "anomaly columns/rparts cut to most": ("anomaly", lambda c, p: _form(p) == "columns" and 1 < p["rparts"] == p["most"] < plan("anomaly", c._replace(M=c.M * 64))["rparts"]),
    "anomaly columns/rparts = want, inside the clamps": ("anomaly", lambda c, p: _form(p) == "columns" and 1 < p["rparts"] == p["want"] < p["most"]),
    # ---- anomaly, pooled form
    "anomaly pooled/parts = 1": ("anomaly", lambda c, p: _form(p) == "pooled" and p["parts"] == 1),
    "anomaly pooled/1 < parts < cap": ("anomaly", lambda c, p: _form(p) == "pooled" and 1 < p["parts"] < plan("anomaly", c._replace(M=c.M * 64))["parts"]),
    "anomaly pooled/parts at its cap": ("anomaly", lambda c, p: _form(p) == "pooled" and p["parts"] > 1 and p["parts"] == plan("anomaly", c._replace(M=c.M * 2))["parts"] == p["grid_y"]),
    "anomaly pooled/one batch": ("anomaly", lambda c, p: _form(p) == "pooled" and p["batches"] == 1),
    "anomaly pooled/three batches, a last one that is no power of two": ("anomaly", lambda c, p: _form(p) == "pooled" and p["batches"] == 3 and 4 * p["nb_last"] < 3 * p["p2_last"]),
    "anomaly pooled/a last batch of one query": ("anomaly", lambda c, p: _form(p) == "pooled" and p["batches"] >= 2 and p["nb_last"] == 1),
    "anomaly pooled/float4": ("anomaly", lambda c, p: _form(p) == "pooled" and p["vec"] == 4),
    "anomaly pooled/scalar by N": ("anomaly", lambda c, p: _form(p) == "pooled" and p["vec"] == 1 and c.mis == 0),
    "anomaly pooled/scalar by the address of scores": ("anomaly", lambda c, p: _form(p) == "pooled" and _by_address("anomaly", c, p, 1)),
    "anomaly/stored origins, a step without a forecast": ("anomaly", lambda c, p: c.origins == 1),
    "anomaly/origins == NULL": ("anomaly", lambda c, p: c.origins == 0),
}
for _k in (2, 3):
    CLASSES[f"aci columns/{_k} or more row trips on a full tile"] = (
        "aci", lambda c, p, k=_k: _form(p) == "columns" and p["Cc"] >= p["tile"] and p["pass_trips_full"] >= k)
    CLASSES[f"aci columns/{_k} or more row trips on a one-column tile"] = (
        "aci", lambda c, p, k=_k: _form(p) == "columns" and p["grid_x"] >= 2 and p["wd_last"] == 1 and p["pass_trips_last"] >= k)
for _b, _name in enumerate(("issued", "raw", "ring_y", "scores")):
    CLASSES[f"aci stream/scalar by the address of {_name}"] = ("aci", lambda c, p, b=1 << _b: _form(p) == "stream" and _by_address("aci", c, p, b))
for _v in (4, 1):
    CLASSES[f"aci stream/window kept, VEC {_v}"] = ("aci", lambda c, p, v=_v: _form(p) == "stream" and p["vec"] == v and p["keep"] == 1 and c.mis == 0)
    CLASSES[f"aci stream/window streamed, VEC {_v}"] = ("aci", lambda c, p, v=_v: _form(p) == "stream" and p["vec"] == v and p["keep"] == 0)
for _s in (0, 1):
    CLASSES[f"anomaly columns/one launch, two or more population trips, per_step = {_s}"] = (
        "anomaly", lambda c, p, s=_s: _form(p) == "columns" and p["launches"] == 1 and p["pop_trips"] >= 2 and c.per_step == s)


for _i, _name in enumerate(("smallest", "middle", "largest")):
    CLASSES[f"gather/the {_name} thread class"] = ("gather", lambda c, p, i=_i: p["threads"] == _gather_threads()[i])


def reached(name, cases=None):
    entry, pred = CLASSES[name]
    return [c for c in (CASES[entry] if cases is None else cases) if pred(c, plan(entry, c))]


@pytest.mark.parametrize("name", list(CLASSES))
def test_class_is_reached(lib, name):
    """at least one case of the entry's list is in the class, according to stemgnn_serving_plan; without those cases none is"""
    hit = reached(name)
    assert hit, f"no case of {CLASSES[name][0]} reaches `{name}`"
    rest = [c for c in CASES[CLASSES[name][0]] if c not in hit]
    assert not reached(name, rest)


def test_lists_are_small_distinct_and_cover_every_entry(lib):
    from stemgnn_amd import _lib

    assert set(CASES) == set(_lib.SG_SERVING_ENTRY) == {CLASSES[k][0] for k in CLASSES}
    assert len(_gather_threads()) == 3
    for entry, cases in CASES.items():
        assert len(set(cases)) == len(cases) <= 16, entry
    assert max(c.M * c.P * c.H * c.N for c in ACI_CASES) * 4 < 3e6 and max(c.M * c.H * c.N for c in ANOMALY_CASES) * 4 < 3e6
    assert max(c.C * c.N for c in GATHER_CASES + PUSH_CASES) * 8 < 1e5
    for c in ACI_CASES + ANOMALY_CASES:
        assert 1 <= c.calls <= 3
    # every misaligned case has its aligned twin in the list: the device suite compares the two runs bit for bit
    for entry in ("gather", "aci", "anomaly"):
        for c in CASES[entry]:
            assert c.mis == 0 or any(o._replace(mis=c.mis, calls=c.calls) == c if hasattr(c, "calls") else o._replace(mis=c.mis) == c
                                     for o in CASES[entry] if o.mis == 0), c


def test_thresholds_have_a_case_on_either_side(lib):
    """the gather's thread classes and the tile, keep, part and batch thresholds, found by asking the plan"""
    from stemgnn_amd import _lib

    t = [_lib.serving_plan("gather", 4, N, 1, 2)["threads"] for N in range(1, 2049)]
    edges = [N for N in range(2, 2049) if t[N - 1] != t[N - 2]]
    have = {c.N for c in GATHER_CASES}
    assert len(edges) == 2 and all(N in have and any(n < N and t[n - 1] == t[N - 2] for n in have) for N in edges), edges
    tiles = [_lib.serving_plan("anomaly", 2, N, 5, 1, 1)["tiles"] for N in range(1, 100)]
    edge = next(N for N in range(2, 100) if tiles[N - 1] == 2)
    assert {edge - 1, edge} <= {c.N for c in ANOMALY_CASES if c.per_node}
    cols = [_lib.serving_plan("aci", 1, N, 1, 5, 1, 1)["grid_x"] for N in range(1, 100)]
    edge = next(N for N in range(2, 100) if cols[N - 1] == 2)
    assert {edge - 1, edge} <= {c.N * (c.H if c.per_step else 1) for c in ACI_CASES if c.per_node}
    assert [_lib.serving_plan("anomaly", 5, 8, M, 1, 1)["launches"] for M in (3, 40)] == [2, 2]
    assert [_lib.serving_plan("anomaly", H, 8, 9, 1, 1)["launches"] for H in (1, 4, 5)] == [1, 1, 2]
    assert [_lib.serving_plan("anomaly", H, 8, 9, 0, 1)["hspan"] for H in (1, 3, 4, 5, 9)] == [1, 3, 4, 4, 4]


# ---- inputs: generated once per case, numpy only -----------------------------------------------------------------------------------
def _rng(c, salt=0):
    return np.random.default_rng(SEED + salt + sum((i + 1) * int(v) for i, v in enumerate(c) if isinstance(v, (int, np.integer))))


def grid(rng, shape, nan=0.10, lo=-12, hi=13):
    """fp32 values on a quarter grid (many ties) with +-inf, +0, -0 and NaN"""
    v = (rng.integers(lo, hi, size=shape) / 4).astype(F32)
    u = rng.random(size=shape)
    edge = nan
    for share, value in ((0.02, np.inf), (0.01, -np.inf), (0.03, 0.0), (0.02, -0.0)):
        v[(u >= edge) & (u < edge + share)] = F32(value)
        edge += share
    v[u < nan] = F32(np.nan)
    return v


def window(rng, shape):
    """a preloaded window [M, ...]: grid() plus a quarter-grid drift over the slots (eight levels, the first exactly as drawn, so
    -0 survives), so that the rows of a later trip or part hold other values than the first ones and leaving them out shows"""
    w = grid(rng, shape)
    drift = ((np.arange(shape[0]) * 8 // shape[0]) / 4).astype(F32).reshape((-1,) + (1,) * (len(shape) - 1))
    return np.where(drift > 0, w + drift, w).astype(F32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_nan_aware(a, b):
    """the same bits wherever either holds a number, NaN in the same places (NaN = absent: its payload is not part of the contract)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool((na == nb).all()) and bool((a.view(u)[~na] == b.view(u)[~nb]).all())


def differ(a, b):
    return not same_nan_aware(np.asarray(a), np.asarray(b))


# ---- push ---------------------------------------------------------------------------------------------------------------------------
def push_data(c):
    rng = _rng(c, 1)
    raw = rng.normal(3.0, 2.0, size=(c.K, c.N))
    u = rng.random(size=raw.shape)
    raw[u < 0.12] = np.nan
    raw[(u >= 0.12) & (u < 0.24)] = MISSING                             # a reading only when has_missing is off
    raw[0, :2] = np.nan, MISSING                                        # the first row falls back on `last`
    sub, div = rng.normal(3.0, 0.5, size=c.N), rng.uniform(0.5, 3.0, size=c.N)
    if c.clip01:
        sub, div = rng.uniform(2.0, 3.0, size=c.N), rng.uniform(1.0, 2.0, size=c.N)     # narrower than the data: both sides clip
    last = rng.normal(3.0, 2.0, size=c.N)
    ring_x = (100 + np.arange(c.C * c.N).reshape(c.C, c.N) / 4).astype(F32)
    ring_y = ring_x.copy()
    ring_y[rng.random(size=ring_y.shape) < 0.2] = np.nan
    return dict(raw=raw, sub=sub, div=div, last=last, ring_x=ring_x, ring_y=ring_y)


def push_covered(c):
    """the ring slots the call writes"""
    return sorted({(c.t0 + k) % c.C for k in range(max(0, c.K - c.C), c.K)})


def push_ref(c, d):
    """the header's contract in numpy: forward fill from `last`, IEEE fp64 subtract and divide, the clip of stemgnn_normalize_series
    (NaN and -0 pass), one rounding to fp32; K > C stores only the last C rows"""
    lv, rx, ry = d["last"].copy(), d["ring_x"].copy(), d["ring_y"].copy()
    for k in range(c.K):
        r = d["raw"][k]
        miss = np.isnan(r) | ((r == MISSING) if c.has_missing else False)
        lv = np.where(miss, lv, r)
        if k >= c.K - c.C:
            v = (lv - d["sub"]) / d["div"]
            if c.clip01:
                v = np.where(v < 0.0, 0.0, np.where(v > 1.0, 1.0, v))
            f = v.astype(F32)
            rx[(c.t0 + k) % c.C] = f
            ry[(c.t0 + k) % c.C] = np.where(miss, F32(np.nan), f)
    return dict(ring_x=rx, ring_y=ry, last=lv, t=np.array([c.t0 + c.K], dtype=np.int64))


# ---- gather -------------------------------------------------------------------------------------------------------------------------
def gather_data(c):
    ring = grid(_rng(c, 2), (c.C, c.N))
    ring[:, 0] = np.arange(c.C, dtype=F32) + 50                          # every slot recognisable
    return dict(ring=ring)


def gather_ref(c, d):
    starts = c.starts if c.starts is not None else (c.t - c.back,)
    out = np.empty((c.B, c.L, c.N), dtype=F32)
    status = 0
    for b, s in enumerate(starts):
        if 0 <= s and s + c.L <= c.t and s >= c.t - c.C:
            out[b] = d["ring"][(s + np.arange(c.L)) % c.C]
        else:
            out[b] = np.array([NAN_BITS], dtype=np.uint32).view(F32)[0]
            status |= 1
    return dict(out=out, status=status)


# ---- ACI ----------------------------------------------------------------------------------------------------------------------------
def aci_pairs(c):
    Q = 2 * c.P + 1
    return Q, [(p, Q - 1 - p) for p in range(c.P)], [0.2, 0.4][:c.P]


def aci_data(c):
    """the preloaded state and, per call, (origin, ring_y [C, N], issued, raw [Q, H, N]); node 1 has no target at all (its
    groups hold), and pooled over the nodes per step neither has the last step"""
    rng = _rng(c._replace(mis=0, calls=0), 3)
    Q, pairs, _ = aci_pairs(c)
    shape = (c.P, c.H if c.per_step else 1, c.N if c.per_node else 1)
    C = c.H + 2
    alpha = rng.choice([0.2, 0.05, 0.5, 0.9], size=shape)
    if alpha.size >= 8:                                                 # two groups outside [0, 1]: the empty band and the whole line
        alpha.reshape(-1)[[2, 5]] = 1.25, -0.125
    d = dict(window=window(rng, (c.M, c.P, c.H, c.N)), alpha=alpha,
             offsets=(rng.integers(-8, 9, size=shape) / 4 + 100).astype(F32), counts=rng.integers(0, 1000, size=shape),
             miss_sum=rng.integers(0, 1000, size=shape), valid_sum=rng.integers(1000, 2000, size=shape), C=C, slot0=c.M - 1, calls=[])
    for k in range(3):                                                  # all three drawn whatever c.calls is: a twin shares them
        origin = 3 + k
        ring = grid(rng, (C, c.N), lo=-6, hi=7)
        ring[:, 1] = np.nan
        if c.per_step and not c.per_node and c.H > 1:
            ring[(origin + c.H - 1) % C] = np.nan
        raw = grid(rng, (Q, c.H, c.N), nan=0.02, lo=-4, hi=5)
        issued = grid(rng, (Q, c.H, c.N), nan=0.02, lo=-4, hi=5)
        for lo, hi in pairs:                                            # mostly a band: lo below hi
            raw[lo], raw[hi] = raw[lo] - F32(1), raw[hi] + F32(1)
            issued[lo], issued[hi] = issued[lo] - F32(2), issued[hi] + F32(2)
        d["calls"].append(dict(origin=origin, ring=ring, raw=raw, issued=issued))
    d["calls"] = d["calls"][:c.calls]
    return d


ACI_STATE = ("scores", "alpha", "offsets", "counts", "miss_sum", "valid_sum")


def aci_ref_run(c, d, window=None):
    """the state after every call: [{scores, alpha, offsets, counts, miss_sum, valid_sum}], by tests/helpers/aci_ref.AciRef"""
    _, pairs, ta = aci_pairs(c)
    ref = aci_ref.AciRef(pairs, ta, GAMMA, c.M, c.per_step, c.per_node, MIN_SCORES, c.H, c.N)
    ref.scores[:] = d["window"] if window is None else window
    ref.alpha[:], ref.offsets[:], ref.counts[:], ref.miss_sum[:], ref.valid_sum[:] = d["alpha"], d["offsets"], d["counts"], d["miss_sum"], d["valid_sum"]
    ref.n_done = d["slot0"]
    states = []
    for call in d["calls"]:
        y = call["ring"][(call["origin"] + np.arange(c.H)) % d["C"]]
        ref.update(y, call["issued"], call["raw"])
        states.append({k: getattr(ref, k).copy() for k in ACI_STATE})
    return states, ref.branches


# ---- anomaly ------------------------------------------------------------------------------------------------------------------------
AN_R, AN_LO, AN_HI, AN_C, AN_ROW0 = 3, 0, 2, 3, 40


def anomaly_data(c):
    rng = _rng(c._replace(mis=0, calls=0), 4)
    S = c.H + 2 if c.origins else 1
    d = dict(window=window(rng, (c.M, c.H, c.N)), slab=grid(rng, (S, AN_R, c.H, c.N), nan=0.02, lo=-4, hi=5), S=S,
             alarm_sum=rng.integers(0, 50, size=c.N), judged_sum=rng.integers(50, 100, size=c.N),
             log_p=(rng.integers(0, 5, size=(KEEP, c.N)) / 4).astype(F32), slot0=c.M - 1, origins=None, calls=[])
    d["slab"][:, AN_LO] -= F32(1)
    d["slab"][:, AN_HI] += F32(1)
    top = AN_ROW0 + 2
    if c.origins:                                                       # slot s holds the origin in (top - S, top] that is s mod S ...
        o = np.array([top - ((top - s) % S) for s in range(S)], dtype=np.int64)
        o[(top - 1) % S] = -5                                           # ... but one slot was never filed: step h = tau - (top - 1) is absent
        d["origins"] = o
    for k in range(3):
        ring = grid(rng, (AN_C, c.N), lo=-6, hi=7)
        ring[:, 0], ring[:, c.N - 1] = np.nan, F32(0.25)               # node 0 never has a reading, the last node always
        d["calls"].append(dict(row=AN_ROW0 + k, ring=ring))
    d["calls"] = d["calls"][:c.calls]
    return d


AN_STATE = ("scores", "pvalues", "node_p", "alarm", "counts", "alarm_sum", "judged_sum", "log_p")


def anomaly_ref_run(c, d, window=None, cls=None):
    cls = cls or anomaly_ref.AnomalyRefFast
    ref = cls(AN_ALPHA, c.M, c.per_step, c.per_node, AN_MIN_SCORES, c.H, c.N, keep=KEEP)
    ref.scores[:] = d["window"] if window is None else window
    ref.alarm_sum[:], ref.judged_sum[:], ref.log_p[:] = d["alarm_sum"], d["judged_sum"], d["log_p"]
    ref.n_done = d["slot0"]
    states = []
    for call in d["calls"]:
        tau = call["row"]
        y = call["ring"][tau % AN_C]
        if c.origins:
            o = tau - np.arange(c.H)
            s = o % d["S"]
            present = (o >= 0) & (d["origins"][s] == o)
            f_lo, f_hi = d["slab"][s, AN_LO, np.arange(c.H)], d["slab"][s, AN_HI, np.arange(c.H)]
        else:
            present, f_lo, f_hi = None, d["slab"][0, AN_LO], d["slab"][0, AN_HI]
        ref.update(y, f_lo, f_hi, present=present, row=tau)
        states.append({k: np.array(getattr(ref, k)).copy() for k in AN_STATE})
    return states


def anomaly_slots(c, d, k):
    """(slot, log_slot) of call k: the host's n_done mod M and mod keep"""
    return (d["slot0"] + k) % c.M, (d["slot0"] + k) % KEEP


def work_words(c):
    """(words of `work`, the words a call may use: H N counts and one m per group)"""
    G = (c.H if c.per_step else 1) * (c.N if c.per_node else 1)
    return 2 * c.H * c.N, c.H * c.N + G


# ---- the references' own checks -----------------------------------------------------------------------------------------------------
def test_inputs_hold_the_edges_they_claim():
    w = grid(np.random.default_rng(0), (4000,))
    share = np.isnan(w).mean()
    assert 0.07 < share < 0.13 and np.isposinf(w).any() and np.isneginf(w).any()
    assert ((w == 0) & np.signbit(w)).any() and ((w == 0) & ~np.signbit(w)).any()
    assert len(np.unique(w[np.isfinite(w)])) < 60                       # a quarter grid: ties everywhere
    for c in PUSH_CASES:
        d = push_data(c)
        assert np.isnan(d["raw"]).any() and (d["raw"] == MISSING).any()
        r = push_ref(c, d)
        cov = push_covered(c)
        assert len(cov) == min(c.K, c.C) and np.isnan(r["ring_y"][cov]).any() and not np.isnan(r["ring_x"][cov]).any()
        if c.clip01:
            assert (r["ring_x"][cov] == 0).any() and (r["ring_x"][cov] == 1).any()
        if c.K < c.C:
            rest = [s for s in range(c.C) if s not in cov]
            assert same_bits(r["ring_x"][rest], d["ring_x"][rest])
    for c in ACI_CASES:
        states, branches = aci_ref_run(c, aci_data(c))
        assert "select" in branches and ("hold" in branches or not (c.per_node or (c.per_step and c.H > 1))), (c, branches)
    assert {"-inf", "+inf"} <= aci_ref_run(ACI_CASES[0], aci_data(ACI_CASES[0]))[1]
    for c in ANOMALY_CASES:
        if c.M * c.H * c.N > 40000:
            continue
        s = anomaly_ref_run(c, anomaly_data(c))[-1]
        assert np.isnan(s["pvalues"]).any() and not np.isnan(s["pvalues"]).all() and not s["alarm"].all(), c
        if c.origins:
            assert np.isnan(s["pvalues"]).all(axis=1).any(), c          # a whole step without a forecast


@pytest.mark.parametrize("c", [c for c in ANOMALY_CASES if c.M * c.H * c.N <= 12000], ids=str)
def test_fast_anomaly_reference_equals_the_loop(c):
    d = anomaly_data(c)
    fast, loop = anomaly_ref_run(c, d), anomaly_ref_run(c, d, cls=anomaly_ref.AnomalyRef)
    assert len(fast) == len(loop) == c.calls
    for a, b in zip(fast, loop):
        for k in AN_STATE:
            assert a[k].dtype == b[k].dtype and same_nan_aware(a[k], b[k]) if a[k].dtype.kind == "f" else np.array_equal(a[k], b[k]), (c, k)


# ---- sensitivity: what a class adds must change the expected outputs ----------------------------------------------------------------
def _aci_rows(c, p):
    """the window's row index (column form: r = i * Hr + h') of every element [M, P, H, N], and its column"""
    i, _, h, n = np.meshgrid(np.arange(c.M), np.arange(c.P), np.arange(c.H), np.arange(c.N), indexing="ij")
    return (i * p["Hr"] + (0 if c.per_step else h)), (h * c.N + n if c.per_step else n)


def _an_rows(c):
    i, h, n = np.meshgrid(np.arange(c.M), np.arange(c.H), np.arange(c.N), indexing="ij")
    return (i if c.per_step else i * c.H + h), h, n


def _aci_window_without(name, c, p):
    r, col = _aci_rows(c, p)
    if "full tile" in name:                                              # tile 0: rows beyond its first trip
        return (col < p["tile"]) & (r >= p["step_full"])
    return (col >= (p["grid_x"] - 1) * p["tile"]) & (r >= p["step_last"])


def _an_window_without(name, c, p):
    r, h, n = _an_rows(c)
    if _form(p) == "columns":
        if "population trips" in name:
            return r >= p["row_lanes"] * p["rparts"]
        return (r // p["row_lanes"]) % p["rparts"] != 0                 # the rows of the parts above 0
    i = np.arange(c.M)[:, None, None]
    t = (h * c.N + n) % p["L"]
    e = i * p["L"] + t
    return (e // (p["threads"] * p["vec"])) % p["parts"] != 0


WINDOW_SENSITIVE = {name: fn for name, fn in (
    [(k, _aci_window_without) for k in CLASSES if "row trips on" in k] +
    [(k, _an_window_without) for k in CLASSES if "population trips" in k or k in (
        "anomaly columns/rparts at its cap", "anomaly columns/rparts cut to most", "anomaly columns/rparts = want, inside the clamps",
        "anomaly pooled/1 < parts < cap", "anomaly pooled/parts at its cap")])}


@pytest.mark.parametrize("name", list(WINDOW_SENSITIVE))
def test_further_trips_and_parts_matter(lib, name):
    """with the window rows of the class's further trips (or parts above 0) absent, the reference gives other offsets / p-values"""
    entry, _ = CLASSES[name]
    hit = reached(name)
    assert hit
    for c in hit:
        p = plan(entry, c)
        without = WINDOW_SENSITIVE[name](name, c, p)
        d = aci_data(c) if entry == "aci" else anomaly_data(c)
        assert without.shape == d["window"].shape and without.any() and not without.all(), c
        assert (~np.isnan(d["window"][without])).any(), c
        less = np.where(without, F32(np.nan), d["window"])
        if entry == "aci":
            full, part = aci_ref_run(c, d)[0][0], aci_ref_run(c, d, window=less)[0][0]
            assert differ(full["offsets"], part["offsets"]) and differ(full["counts"], part["counts"]), c
        else:
            full, part = anomaly_ref_run(c, d)[0], anomaly_ref_run(c, d, window=less)[0]
            assert differ(full["pvalues"], part["pvalues"]) and differ(full["counts"], part["counts"]), c


def _aci_outputs_without(name, c, p, d, full):
    """(output name, mask of the elements the class's share writes)"""
    r, col = _aci_rows(c, p)
    if "origin-scoring" in name or "scoring trips" in name:             # the origin's rows (stream: elements) beyond the first trip
        h, n = np.meshgrid(np.arange(c.H), np.arange(c.N), indexing="ij")
        at = (h if _form(p) == "columns" else (h * c.N + n) % p["L"]) >= p["step_full"]
        m = np.zeros(d["window"].shape, bool)
        m[d["slot0"]] = at[None]
        return "scores", m
    shape = full["offsets"].shape                                        # the last tile's groups
    g = np.arange(shape[1] * shape[2]).reshape(shape[1:])
    return "offsets", np.broadcast_to(g >= (p["grid_x"] - 1) * p["tile"], shape)


def _an_outputs_without(name, c, p, d, full):
    h, n = np.meshgrid(np.arange(c.H), np.arange(c.N), indexing="ij")
    if _form(p) == "columns":
        return "pvalues", n >= (p["tiles"] - 1) * p["tile"]
    batch = (p["L"] - p["nb_last"]) // (p["batches"] - 1)               # queries per full batch, from the plan
    t = (h * c.N + n) % p["L"]
    return "pvalues", t >= batch                                        # every batch after the first


def _push_outputs_without(name, c, p, d, full):
    m = np.zeros((c.C, c.N), bool)
    m[push_covered(c), (p["grid_x"] - 1) * p["threads"]:] = True
    return "ring_x", m


def _gather_outputs_without(name, c, p, d, full):
    m = np.zeros((c.B, c.L, c.N), bool)
    m[:, :, p["threads"] * p["vec"]:] = True
    return "out", m


OUTPUT_SENSITIVE = {
    "push/two or more blocks, ragged last": _push_outputs_without,
    "push/K > C with t0 % C != 0, several blocks": _push_outputs_without,
    "gather/two or more copy trips, float4": _gather_outputs_without,
    "gather/two or more copy trips, scalar": _gather_outputs_without,
    "aci columns/three or more tiles, ragged last": _aci_outputs_without,
    "aci columns/a last tile of one column": _aci_outputs_without,
    "aci columns/two origin-scoring trips": _aci_outputs_without,
    "aci stream/L over several scoring trips": _aci_outputs_without,
    "anomaly columns/N = one tile and one node": _an_outputs_without,
    "anomaly columns/three or more tiles, ragged": _an_outputs_without,
    "anomaly pooled/three batches, a last one that is no power of two": _an_outputs_without,
    "anomaly pooled/a last batch of one query": _an_outputs_without,
}


def before_and_after(entry, c):
    """(what the outputs hold before the first call, what the reference says they hold after it)"""
    if entry == "push":
        d = push_data(c)
        before = dict(d)
        before["ring_x"], before["ring_y"] = d["ring_x"].copy(), d["ring_y"].copy()
        before["ring_x"][push_covered(c)] = np.nan
        before["ring_y"][push_covered(c)] = np.nan
        return d, before, push_ref(c, d)
    if entry == "gather":
        d = gather_data(c)
        return d, dict(out=np.full((c.B, c.L, c.N), np.nan, dtype=F32)), gather_ref(c, d)
    if entry == "aci":
        d = aci_data(c)
        return d, dict(scores=d["window"], offsets=d["offsets"]), aci_ref_run(c, d)[0][0]
    d = anomaly_data(c)
    return d, dict(pvalues=np.full((c.H, c.N), np.nan, dtype=F32)), anomaly_ref_run(c, d)[0]


@pytest.mark.parametrize("name", list(OUTPUT_SENSITIVE))
def test_further_tiles_blocks_and_batches_matter(lib, name):
    """leaving the outputs of the class's last tile / block / batch / further trips as they were gives other expected outputs"""
    entry, _ = CLASSES[name]
    hit = reached(name)
    assert hit
    for c in hit:
        p = plan(entry, c)
        d, before, full = before_and_after(entry, c)
        key, mask = OUTPUT_SENSITIVE[name](name, c, p, d, full)
        assert mask.shape == full[key].shape and mask.any() and not mask.all(), (c, key)
        part = np.where(mask, before[key], full[key])
        assert differ(part, full[key]), (c, key)


def test_comparisons_fail_on_one_wrong_element():
    """the device suite's comparisons, handed wrong results: one ulp, a NaN lost, a NaN made, the sign of a zero"""
    w = window(np.random.default_rng(1), (6, 2, 9))
    assert same_bits(w, w.copy()) and same_nan_aware(w, w.copy()) and not differ(w, w.copy())
    flat = w.reshape(-1)
    k_num, k_nan = int(np.flatnonzero(np.isfinite(flat))[3]), int(np.flatnonzero(np.isnan(flat))[0])
    k_zero = int(np.flatnonzero(flat == 0)[0])
    for k, v in ((k_num, np.nextafter(flat[k_num], F32(99))), (k_nan, F32(0.5)), (k_num, F32(np.nan)), (k_zero, -flat[k_zero])):
        wrong = w.copy()
        wrong.reshape(-1)[k] = v
        assert not same_bits(wrong, w) and not same_nan_aware(wrong, w) and differ(wrong, w), (k, v)
    other = w.copy()
    other.view(np.uint32).reshape(-1)[k_nan] = 0x7FC00001               # another NaN payload: absent all the same, other bits
    assert same_nan_aware(other, w) and not same_bits(other, w)
    a = np.array([0.2, 0.5])
    assert not same_bits(a, np.nextafter(a, 9.0)) and not same_bits(a, a.astype(F32)) and not same_nan_aware(a, a[:1])


# ---- refusals, host only: fake pointers, nothing is launched ------------------------------------------------------------------------
P = 4096
ACI_OK = dict(issued=P, raw=P, ring_y=P, C=7, origin=3, Q=3, H=2, N=11, P=1, lo=None, hi=None, ta=None, gamma=0.05, M=5, slot=4,
              min_scores=0, per_step=1, per_node=0, scores=P, alpha=P, offsets=P, counts=P, miss_sum=P, valid_sum=P)
AN_OK = dict(slab=P, S=4, R=3, lo=0, hi=2, origins=P, row=9, ring_y=P, C=7, H=2, N=11, M=5, slot=4, min_scores=0, alpha=0.1,
             per_step=1, per_node=0, scores=P, pvalues=P, node_p=P, alarm=P, counts=P, alarm_sum=P, judged_sum=P, log_p=P, keep=3,
             log_slot=2, work=P)
PUSH_OK = dict(raw=P, K=1, N=11, t0=0, sub=P, div=P, clip01=0, missing=0.0, has_missing=1, last=P, ring_x=P, ring_y=P, C=12, t_dev=P)
GATHER_OK = dict(ring=P, C=12, N=11, starts=P, t_dev=P, back=0, B=3, L=5, out=P, status=P)


def _aci(lib, **change):
    a = {**ACI_OK, **change}
    a["lo"], a["hi"], a["ta"] = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(2), (ctypes.c_double * 1)(0.2)
    return lib.stemgnn_aci_update(*a.values(), None)


def _call(f, ok, **change):
    return f(*{**ok, **change}.values(), None)


def test_entries_refuse_what_the_abi_files_leave(lib):
    an, push, gather = lib.stemgnn_anomaly_update, lib.stemgnn_live_push, lib.stemgnn_ring_gather
    # spans > 65535: per_node and per_step, one span per step
    assert _call(an, AN_OK, per_node=1, H=65536, N=1, slot=0, M=1) == EINVAL
    assert _call(an, AN_OK, per_node=1, per_step=0, H=4 * 65535 + 1, N=1, slot=0, M=1) == EINVAL
    # every 2^31 limit of the anomaly entry, each alone
    for change in (dict(H=2 ** 16, N=2 ** 15, M=1, slot=0, S=1, R=1, hi=0),             # H N
                   dict(M=2 ** 20, H=2 ** 4, N=2 ** 7, slot=0, S=1, R=1, hi=0),         # M H N
                   dict(C=2 ** 20, N=2 ** 11, H=1, M=1, slot=0, S=1, R=1, hi=0),        # C N
                   dict(R=32, hi=31, H=2 ** 13, N=2 ** 13, M=1, slot=0, S=1),           # R H N
                   dict(S=2 ** 10, R=2, hi=1, H=2 ** 10, N=2 ** 10, M=1, slot=0),       # S R H N
                   dict(keep=2 ** 20, N=2 ** 11, H=1, M=1, slot=0, S=1, R=1, hi=0, C=1)):   # keep N
        assert _call(an, AN_OK, **change) == EINVAL, change
        assert _call(an, AN_OK, per_node=1, **change) == EINVAL, change
    # ... and of the adaptive update (fake pointers: only refused calls are ever made)
    for change in (dict(H=2 ** 16, N=2 ** 15, M=1, slot=0, C=2 ** 16), dict(M=2 ** 20, H=2 ** 4, N=2 ** 7, slot=0, C=16),
                   dict(C=2 ** 20, N=2 ** 11, H=1, M=1, slot=0), dict(H=8, C=7), dict(M=0, slot=0), dict(C=0)):
        assert _aci(lib, **change) == EINVAL, change
        assert _aci(lib, per_node=1, **change) == EINVAL, change
    # the ring entries
    assert _call(push, PUSH_OK, C=2 ** 20, N=2 ** 11) == EINVAL and _call(push, PUSH_OK, C=2 ** 16, N=2 ** 15) == EINVAL
    for ok in (GATHER_OK, {**GATHER_OK, **dict(starts=None, back=4, B=1, L=4)}):
        assert _call(gather, ok, L=13) == EINVAL                        # L > C
        assert _call(gather, ok, back=13) == EINVAL                     # back > C
        assert _call(gather, ok, L=12, back=12, C=11) == EINVAL
        assert _call(gather, ok, C=2 ** 20, N=2 ** 11) == EINVAL
    assert _call(gather, GATHER_OK, B=65536) == EINVAL and _call(gather, GATHER_OK, B=2 ** 20) == EINVAL


def test_plan_refusals(lib):
    from stemgnn_amd import _lib

    out = (ctypes.c_int * _lib.SG_SERVING_PLAN_WORDS)()
    E = _lib.SG_SERVING_ENTRY
    f = lib.stemgnn_serving_plan
    assert f(E["push"], 3, 11, 8, 0, 0, 0, 0, out) == 0 and list(out)[:8] == [0, 1, 1, 1, 64, 0, 1, 0]
    assert f(E["push"], 3, 11, 8, 0, 0, 0, 0, None) == EINVAL
    assert f(E["push"], 3, 11, 8, -1 << 40, 1 << 40, 7, 0, out) == 0     # arguments an entry does not use
    for entry in (-1, len(E), 1 << 20):
        assert f(entry, 3, 11, 8, 2, 1, 1, 0, out) == EINVAL
    bad = {"push": [(0, 11, 8), (3, 0, 8), (3, 11, 0), (-1, 11, 8), (3, 2 ** 15, 2 ** 16), (1 << 32, 11, 8)],
           "gather": [(0, 11, 3, 5), (12, 0, 3, 5), (12, 11, 0, 5), (12, 11, 3, 0), (12, 11, 3, 13), (12, 11, 65536, 5), (2 ** 16, 2 ** 15, 3, 5)],
           "aci": [(0, 11, 1, 5, 1, 1), (2, 0, 1, 5, 1, 1), (2, 11, 0, 5, 1, 1), (2, 11, 17, 5, 1, 1), (2, 11, 1, 0, 1, 1),
                   (2 ** 16, 2 ** 15, 1, 1, 1, 0), (2 ** 4, 2 ** 7, 1, 2 ** 20, 0, 1), (1 << 32, 11, 1, 5, 1, 1)],
           "anomaly": [(0, 11, 5, 1, 1), (2, 0, 5, 1, 1), (2, 11, 0, 1, 1), (65536, 1, 1, 1, 1), (4 * 65535 + 1, 1, 1, 0, 1),
                       (2 ** 16, 2 ** 15, 1, 1, 0), (2 ** 4, 2 ** 7, 2 ** 20, 0, 0)]}
    assert set(bad) == set(E)
    for entry, shapes in bad.items():
        for s in shapes:
            assert f(E[entry], *(list(s) + [0] * (6 - len(s))), 0, out) == EINVAL, (entry, s)
    assert f(E["anomaly"], 65535, 1, 1, 1, 1, 0, 0, out) == 0 and out[2] == 65535
    assert f(E["anomaly"], 65536, 1, 1, 1, 0, 0, 0, out) == 0            # pooled: no span limit
    # a bit that names no buffer of the entry
    for entry, first_bad in (("push", 1), ("gather", 4), ("aci", 16), ("anomaly", 2)):
        shape = {"push": (3, 11, 8), "gather": (12, 12, 3, 5), "aci": (2, 12, 1, 5, 1, 0), "anomaly": (2, 12, 5, 1, 0)}[entry]
        args = list(shape) + [0] * (6 - len(shape))
        assert f(E[entry], *args, first_bad, out) == EINVAL and f(E[entry], *args, -1, out) == EINVAL, entry
        for m in range(first_bad):
            assert f(E[entry], *args, m, out) == 0 and (out[5] == 4) == (m == 0 and entry != "push"), (entry, m)
