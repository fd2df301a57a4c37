"""CPU: the shapes of tests/test_hip_gru_paths.py reach every reachable launch path of csrc/gru.hip.

stemgnn_gru_paths is the launchers' own plan (host only); `cus = 256` asks it for an MI355X without a device.  "Reachable"
is derived here by brute force over the shape range, not typed in: if a threshold of the plan moves (the forward's
preferred 7 workgroups per row, its 40-column bound, the 64-lane slice, the residency rule cus - cus / 8, GRU4_WMAX), an
instantiation appears or disappears, a pinned anchor moves, or the case list loses a path -- and this fails on a machine
without a GPU, naming what was lost."""
import itertools
from ctypes import c_int

import pytest

from tests.test_hip_gru_paths import GRU_CASES, GRU_STEP_CASES

CUS = 256
LIMIT = CUS - CUS // 8                       # the residency rule: workgroups that must all be resident at once
WS = (1, 3, 12, 16, 17, 20, 64)
FWD = ("fwd_family", "fwd_P", "fwd_K")
BWD = ("bwd_family", "bwd_P", "bwd_KU", "bwd_slices")


@pytest.fixture(scope="module")
def lib():
    import os

    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(autouse=True)
def _default_switches(monkeypatch):
    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE"):
        monkeypatch.delenv(name, raising=False)


def _plan(lib, B, Hd, W, S=None, cus=CUS):
    from stemgnn_amd._lib import SG_GRU_PATH_WORDS, SG_GRU_WORD

    out = (c_int * SG_GRU_PATH_WORDS)()
    rc = lib.stemgnn_gru_paths(B, Hd if S is None else S, Hd, W, cus, out)
    assert rc == 0, ((B, S, Hd, W), rc)
    return {k: int(out[i]) for k, i in SG_GRU_WORD.items()}


def _last_pass(B):
    return B - 16 * ((B + 15) // 16 - 1)


def _features(p, B, Hd):
    """what one shape proves, as a set of named values"""
    f = {("fwd",) + tuple(p[k] for k in FWD), ("bwd",) + tuple(p[k] for k in BWD),
         ("gi_stream", p["gi_stream"]), ("ih_folded", p["ih_folded"]), ("rank2_ok", p["rank2_ok"]), ("hh_form", p["hh_form"]),
         ("wide_MT", p["wide_MT"]), ("wide_GWf", p["wide_GWf"]), ("wide_GWb", p["wide_GWb"])}
    if p["ih_slabs"] > 32:
        f.add(("ih_slabs > 32, Hd % 4 == 0", Hd % 4 == 0))
    if p["wide_passes"]:
        f.add(("wide passes", min(p["wide_passes"], 3)))                        # 1, 2, >= 3
        f.add(("wide last pass rows", "<= 8" if _last_pass(B) <= 8 else ("9..15" if _last_pass(B) < 16 else "16")))
    return f


@pytest.fixture(scope="module")
def reachable(lib):
    hds = list(range(1, 601)) + list(range(608, 2049, 16)) + [1023, 1025, 2047]
    seen = set()
    for B, Hd, W in itertools.product(range(1, 301), hds, WS):
        seen |= _features(_plan(lib, B, Hd, W), B, Hd)
    return seen


def test_cases_are_distinct_and_in_range():
    assert len(set(GRU_CASES)) == len(GRU_CASES) and len(set(GRU_STEP_CASES)) == len(GRU_STEP_CASES)
    for B, Hd, W in GRU_CASES:
        assert 1 <= B <= 300 and 1 <= Hd <= 2048 and 1 <= W <= 64, (B, Hd, W)
    for B, S, Hd, W in GRU_STEP_CASES:
        assert 1 <= S < 4 * 2 and S != Hd, (B, S, Hd, W)       # fewer steps than two progress chunks, one below a single one
    assert any(S < 4 for _, S, _, _ in GRU_STEP_CASES)


def test_case_list_reaches_everything_reachable(lib, reachable):
    from stemgnn_amd._lib import SG_GRU_FAM, SG_GRU_HH

    got = set()
    for B, Hd, W in GRU_CASES:
        got |= _features(_plan(lib, B, Hd, W), B, Hd)
    missing = sorted(reachable - got, key=str)
    assert not missing, f"reachable at {CUS} CUs, run by no case of GRU_CASES: {missing}"
    assert got <= reachable, sorted(got - reachable, key=str)          # (the enumeration covers the cases' own range)
    # the enumeration itself found every family and both sides of every decision (a plan that lost one shows here)
    fams = {f[1] for f in reachable if f[0] == "fwd"}
    assert fams == {SG_GRU_FAM["stream"], SG_GRU_FAM["cluster4"], SG_GRU_FAM["wide"]}, fams
    fams = {f[1] for f in reachable if f[0] == "bwd"}
    assert fams == {SG_GRU_FAM["stream"], SG_GRU_FAM["cluster2"], SG_GRU_FAM["cluster4"], SG_GRU_FAM["wide"]}, fams
    for k in ("gi_stream", "ih_folded", "rank2_ok"):
        assert {(k, 0), (k, 1)} <= reachable, k
    assert {("hh_form", v) for v in SG_GRU_HH.values()} <= reachable
    assert {("ih_slabs > 32, Hd % 4 == 0", True), ("ih_slabs > 32, Hd % 4 == 0", False)} <= reachable
    assert {("wide passes", 1), ("wide passes", 3), ("wide last pass rows", "<= 8"), ("wide last pass rows", "9..15")} <= reachable
    assert {("wide_GWf", 8), ("wide_GWf", 16), ("wide_GWb", 24), ("wide_GWb", 48)} <= reachable
    # the instantiations of the wave-level clusters: what exists against what a 256-CU device can be made to run
    fwd = {(f[2], f[3]) for f in reachable if f[0] == "fwd" and f[1] == SG_GRU_FAM["cluster4"]}
    assert fwd == ({(1, k) for k in (32, 34, 40, 48, 58, 64)} | {(p, k) for p in (2, 4) for k in (34, 40, 48, 58, 64)}
                   | {(p, k) for p in (5, 6, 8) for k in (58, 64)} | {(7, 32), (7, 34), (7, 40)}), sorted(fwd)
    bwd = {f[1:] for f in reachable if f[0] == "bwd" and f[1] in (SG_GRU_FAM["cluster2"], SG_GRU_FAM["cluster4"])}
    c2, c4 = SG_GRU_FAM["cluster2"], SG_GRU_FAM["cluster4"]
    assert bwd == ({(c4, 1, k, 1) for k in (32, 48, 58, 64)} | {(c4, p, k, 1) for p in (2, 4) for k in (48, 58, 64)}
                   | {(c4, 6, k, 2) for k in (58, 64)} | {(c2, 5, k, 1) for k in (58, 64)} | {(c2, 8, k, 2) for k in (58, 64)}), sorted(bwd)


def test_residency_edge_is_run_at_three_shapes(lib):
    """B * P exactly at the limit (one more batch row and the launcher must choose another kernel)"""
    at_edge = []
    for B, Hd, W in GRU_CASES:
        p, q = _plan(lib, B, Hd, W), _plan(lib, B + 1, Hd, W)
        if p["bwd_P"] and B * p["bwd_P"] == LIMIT:
            assert (q["bwd_family"], q["bwd_P"]) != (p["bwd_family"], p["bwd_P"]), (B, Hd, W)
            at_edge.append((B, Hd, W))
    assert len(at_edge) >= 3, at_edge
    assert {(56, 228, 12), (28, 512, 12), (224, 64, 3)} <= set(at_edge)
    # ... and the forward's own edge: 7 workgroups per row at batch 32, the backward's P from 33 on
    assert _plan(lib, 32, 228, 12)["fwd_P"] == 7 and _plan(lib, 33, 228, 12)["fwd_P"] == 4 and 32 * 7 == LIMIT
    assert any(B * _plan(lib, B, Hd, W)["fwd_P"] == LIMIT and _plan(lib, B, Hd, W)["fwd_P"] == 7 for B, Hd, W in GRU_CASES)


def test_pinned_anchors(lib):
    from stemgnn_amd._lib import SG_GRU_FAM as F, SG_GRU_HH as HH

    def sub(p, **kw):
        got = {k: p[k] for k in kw}
        assert got == kw, f"plan moved: {sorted(set(got.items()) - set(kw.items()))} where the code stood at {sorted(set(kw.items()) - set(got.items()))}"
        return True

    p = _plan(lib, 32, 228, 12)                      # PEMS07
    assert sub(p, fwd_family=F["cluster4"], fwd_P=7, fwd_K=34, gi_stream=1, bwd_family=F["cluster4"], bwd_P=4, bwd_KU=58,
               bwd_slices=1, ih_folded=1, hh_form=HH["tiles"], ih_slabs=32, rank2_ok=1, wide_passes=0), p
    p = _plan(lib, 56, 228, 12)                      # 56 * 4 == 224: the last batch size on the per-row clusters at N = 228
    assert sub(p, fwd_family=F["cluster4"], fwd_P=4, fwd_K=58, bwd_family=F["cluster4"], bwd_P=4, bwd_KU=58, ih_folded=1,
               ih_slabs=56, rank2_ok=1), p
    p = _plan(lib, 57, 228, 12)                      # one more: the wide cluster in passes of 16, 16, 16, 9 rows
    assert sub(p, fwd_family=F["wide"], bwd_family=F["wide"], fwd_P=0, bwd_P=0, wide_passes=4, rank2_ok=0, ih_folded=0,
               gi_stream=0, wide_MT=1, wide_GWf=8, wide_GWb=24) and _last_pass(57) == 9, p
    p = _plan(lib, 3, 385, 12)
    assert sub(p, fwd_family=F["cluster4"], fwd_P=8, fwd_K=58, bwd_family=F["cluster2"], bwd_P=8, bwd_KU=58, bwd_slices=2,
               rank2_ok=0, ih_folded=0, hh_form=HH["slabs"], ih_slabs=32), p
    p = _plan(lib, 32, 358, 12)                      # PEMS03
    assert sub(p, bwd_family=F["cluster4"], bwd_P=6, bwd_slices=2, rank2_ok=1, ih_folded=1, hh_form=HH["slabs"]), p
    p = _plan(lib, 225, 40, 4)                       # more rows than resident workgroups, hidden < 64: streaming both ways
    assert sub(p, fwd_family=F["stream"], bwd_family=F["stream"], fwd_P=0, bwd_P=0, rank2_ok=0, wide_passes=0), p
    assert sub(_plan(lib, 4, 512, 16), hh_form=HH["tiles"], ih_folded=0, bwd_KU=64)      # 64 output tiles: still the tile list
    assert sub(_plan(lib, 16, 513, 3), hh_form=HH["slabs"], fwd_family=F["wide"])
    assert sub(_plan(lib, 8, 1024, 12), hh_form=HH["flat"], fwd_family=F["wide"], wide_GWf=8, wide_GWb=24)
    assert sub(_plan(lib, 16, 2048, 48), hh_form=HH["flat"], wide_MT=2, wide_GWf=16, wide_GWb=48)
    assert sub(_plan(lib, 5, 321, 16), ih_folded=1) and sub(_plan(lib, 5, 321, 17), ih_folded=0)
    # the sequence length is no part of any kernel choice
    for B, S, Hd, W in GRU_STEP_CASES:
        assert _plan(lib, B, Hd, W, S=S) == _plan(lib, B, Hd, W), (B, S, Hd, W)
    # the plan is what stemgnn_gru_bwd_rank2_ok / stemgnn_gru_bwd_cus answer from (no device here: their limit is 0, as
    # cus <= 0 asks; with a GPU the current device's)
    for B, Hd in ((32, 228), (57, 228), (3, 385), (225, 40)):
        p = _plan(lib, B, Hd, 12, cus=0)
        assert lib.stemgnn_gru_bwd_rank2_ok(B, Hd) == p["rank2_ok"]


def test_model_level_fallback_cases_take_the_fallbacks(lib):
    from stemgnn_amd._lib import SG_GRU_FAM as F
    from tests.test_hip_shape_domain import GRU_FALLBACK_CASES

    plans = {c: _plan(lib, c[4], c[0], c[1]) for c in GRU_FALLBACK_CASES}            # (N, W, multi, H, B)
    p = plans[(228, 12, 5, 3, 64)]
    assert (p["fwd_family"], p["bwd_family"], p["wide_passes"], p["rank2_ok"]) == (F["wide"], F["wide"], 4, 0), p
    p = plans[(400, 12, 5, 3, 4)]
    assert (p["fwd_P"], p["bwd_family"], p["bwd_P"], p["bwd_slices"], p["rank2_ok"]) == (8, F["cluster2"], 8, 2, 0), p
    p = plans[(60, 12, 5, 3, 40)]
    assert (p["fwd_family"], p["fwd_P"], p["ih_folded"], p["ih_slabs"], p["rank2_ok"]) == (F["cluster4"], 1, 1, 40, 1), p
    p = plans[(40, 8, 2, 4, 225)]
    assert (p["fwd_family"], p["bwd_family"], p["rank2_ok"]) == (F["stream"], F["stream"], 0), p


def test_gru_paths_rejects_bad_arguments(lib):
    from stemgnn_amd._lib import SG_EINVAL, SG_GRU_PATH_WORDS

    out = (c_int * SG_GRU_PATH_WORDS)()
    for args in ((0, 5, 5, 12), (2, 0, 5, 12), (2, 5, 0, 12), (2, 5, 5, 0), (-1, 5, 5, 12)):
        assert lib.stemgnn_gru_paths(*args, CUS, out) == SG_EINVAL, args
    assert lib.stemgnn_gru_paths(2, 5, 5, 12, CUS, None) == SG_EINVAL


def test_environment_switches_count_as_the_launchers_read_them(lib, monkeypatch):
    from stemgnn_amd._lib import SG_GRU_FAM as F

    fam = lambda B, Hd: (_plan(lib, B, Hd, 12)["fwd_family"], _plan(lib, B, Hd, 12)["bwd_family"])
    assert fam(32, 228) == (F["cluster4"], F["cluster4"]) and fam(5, 33) == (F["cluster4"], F["cluster4"])
    monkeypatch.setenv("STEMGNN_GRU_CLUSTER", "0")                # streaming kernels, also where the wide cluster would fit
    assert fam(32, 228) == fam(5, 33) == fam(8, 1024) == (F["stream"], F["stream"])
    assert _plan(lib, 32, 228, 12)["rank2_ok"] == 0
    monkeypatch.setenv("STEMGNN_GRU_CLUSTER", "1")                # the round-1 cluster -- below hidden 64 only: from there on the
    assert fam(5, 33) == (F["cluster1"], F["cluster1"])           # wide cluster takes what the wave-level clusters leave
    assert _plan(lib, 5, 33, 12)["bwd_P"] == 1 and _plan(lib, 5, 33, 12)["rank2_ok"] == 0
    assert fam(32, 228) == (F["wide"], F["wide"])
    assert fam(225, 40) == (F["stream"], F["stream"])             # 225 rows are not resident for it either
    monkeypatch.setenv("STEMGNN_GRU_WIDE", "0")
    assert fam(32, 228) == (F["cluster1"], F["cluster1"]) and _plan(lib, 32, 228, 12)["bwd_P"] == 4
    monkeypatch.setenv("STEMGNN_GRU_CLUSTER", "2")
    assert fam(57, 228) == (F["stream"], F["stream"])             # 57 * 4 > 224: no cluster of either kind
    assert fam(8, 1024) == (F["stream"], F["stream"])
    monkeypatch.setenv("STEMGNN_GRU_WIDE", "1")                   # forced: the small hidden sizes of the wide test
    p = _plan(lib, 3, 228, 12)
    assert (p["fwd_family"], p["bwd_family"], p["wide_passes"], p["rank2_ok"]) == (F["wide"], F["wide"], 1, 0)
    assert fam(5, 33) == (F["cluster4"], F["cluster4"])           # ... which starts at hidden 64
