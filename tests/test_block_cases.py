"""CPU: BLOCK_CASES of tests/test_hip_block.py reaches both sides of every decision the StockBlock stage takes by shape
(stemgnn_block_paths and stemgnn_glu_fused_bf16_ok ask the launchers' own predicates, host only; the padding classes follow from
csrc/layout.h), every case is inside the constructor's range, and the Python transcription of csrc/layout.h the GPU suite views the
buffers through agrees with the library's size functions.  A threshold that moves fails here instead of silently dropping a path
from the GPU suite."""
import pytest

from tests.test_hip_block import BLOCK_CASES, M_SWEEP
from tests.util import dims, l2_channels, saved_layout, scratch_layout

WANT_M = {31, 32, 33, 63, 64, 65, 95, 96, 97, 129}
WANT_NAMED = [(1, 1, 1, 1), (1, 2, 2, 1), (2, 3, 1, 3), (3, 5, 64, 1), (1, 17, 13, 5), (2, 6, 64, 5), (4, 40, 64, 3), (2, 7, 64, 9),
              (2, 5, 64, 11), (4, 228, 12, 5)]


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
    monkeypatch.delenv("STEMGNN_GLU_FUSED", raising=False)


def _paths(lib, case, splits=0):
    from stemgnn_amd._lib import SG_PATH

    B, N, W, multi = case
    v = lib.stemgnn_block_paths(B, N, W, multi, splits)
    assert v >= 0, (case, v)
    return {k: bool(v & bit) for k, bit in SG_PATH.items()}


def _padding_classes(case):
    d = dims(*case)
    f = set()
    for mod in (32, 64, 96):
        f.add(f"M % {mod} {'==' if d.M % mod == 0 else '!='} 0")
    if d.CP > d.C:
        f.add("CP > C")
    if any(d.CP2[r] > d.U[r] > 0 for r in range(2)):
        f.add("CP2[r] > U[r]")
    if d.WmP > d.Wm:
        f.add("WmP > Wm")
    if d.nf[1] == 0:
        f.add("nf[1] == 0")
    return f


PADDING_CLASSES = {f"M % {mod} {op} 0" for mod in (32, 64, 96) for op in ("==", "!=")} | {"CP > C", "CP2[r] > U[r]", "WmP > Wm", "nf[1] == 0"}


def _missing_paths(lib, cases):
    from stemgnn_amd._lib import SG_PATH

    missing = []
    for splits in (0, 2):
        seen = {k: set() for k in SG_PATH}
        for c in cases:
            for k, v in _paths(lib, c, splits).items():
                seen[k].add(v)
        missing += [(splits, k, v) for k, s in seen.items() for v in sorted({True, False} - s)]
    ok = {bool(lib.stemgnn_glu_fused_bf16_ok(c[2], c[3], 2)) for c in cases}
    missing += [("glu_fused_bf16_ok", v) for v in sorted({True, False} - ok)]
    return missing


def test_cases_are_in_the_constructor_range(lib):
    for B, N, W, multi in BLOCK_CASES:
        assert B >= 1 and N >= 1 and multi >= 1 and W >= 1 and lib.stemgnn_fc_tail_supported(W, 1) == 1, (B, N, W, multi)
    assert len(set(BLOCK_CASES)) == len(BLOCK_CASES)


def test_the_named_cases_and_the_m_sweep_are_there():
    assert all(c in BLOCK_CASES for c in WANT_NAMED), [c for c in WANT_NAMED if c not in BLOCK_CASES]
    assert {B * N for B, N in M_SWEEP} == WANT_M and all((B, N, 12, 5) in BLOCK_CASES for B, N in M_SWEEP)
    assert all(max(B, N) <= 97 and B * N in WANT_M for B, N in M_SWEEP)


def test_every_path_bit_is_reached_both_ways(lib):
    assert not _missing_paths(lib, BLOCK_CASES), _missing_paths(lib, BLOCK_CASES)


def test_every_padding_class_is_reached():
    have = set().union(*(_padding_classes(c) for c in BLOCK_CASES))
    assert have == PADDING_CLASSES, sorted(PADDING_CLASSES ^ have)


@pytest.mark.parametrize("lost", sorted(PADDING_CLASSES))
def test_a_list_trimmed_of_a_padding_class_fails(lost):
    kept = [c for c in BLOCK_CASES if lost not in _padding_classes(c)]
    assert len(kept) < len(BLOCK_CASES), f"no case shows {lost!r}"
    assert lost not in set().union(*(_padding_classes(c) for c in kept))


def test_pinned_decisions(lib):
    """what the comment beside each case of BLOCK_CASES says it is there for"""
    for c in [(1, 1, 1, 1), (1, 2, 2, 1), (2, 3, 1, 3)]:
        p, d = _paths(lib, c), dims(*c)
        assert d.Wm <= 3 and p["heads_bwd_fused"] and not p["heads_bwd_16w"] and not p["wgrad_fused"], (c, p)
    assert dims(1, 1, 1, 1).nf[1] == 0 and dims(1, 2, 2, 1).nf[1] == 0 and dims(2, 3, 1, 3).nf[1] == 1
    p = _paths(lib, (3, 5, 64, 1))
    assert dims(3, 5, 64, 1).CP == 256 and p["glu_fwd_fused"] and not p["glu_dgrad_fused"], p
    assert dims(1, 17, 13, 5).CP == 272 and not _paths(lib, (1, 17, 13, 5))["glu_fwd_fused"]
    p = _paths(lib, (2, 6, 64, 5))
    assert p["long_k"] and not p["heads_fwd_fused"] and p["heads_bwd_fused"], p
    p = _paths(lib, (4, 40, 64, 3))
    assert dims(4, 40, 64, 3).KF == 784 and p["long_k"] and not p["heads_fwd_fused"], p
    for c in [(2, 7, 64, 9), (2, 5, 64, 11)]:
        assert not _paths(lib, c)["heads_bwd_fused"], c
    assert dims(2, 7, 64, 9).Wm <= 640 < dims(2, 5, 64, 11).Wm            # the LDS limit; the Wm limit (SG_LONG_K)
    c = next(c for c in BLOCK_CASES if dims(*c).CP <= 128 and dims(*c).Wm > 3)
    assert _paths(lib, c)["glu_dgrad_fused"] and _paths(lib, c, 2)["glu_dgrad_fused"], c       # the chain with nt = 1
    pems = _paths(lib, (4, 228, 12, 5))
    assert not pems.pop("long_k") and all(pems.values()), pems
    for B, N in M_SWEEP:                                                  # the ragged sizes run the fused forms (64- and 96-row blocks)
        p = _paths(lib, (B, N, 12, 5))
        assert p["glu_fwd_fused"] and p["glu_dgrad_fused"] and p["wgrad_fused"], (B, N, p)


def test_python_layout_is_the_librarys(lib):
    for case in BLOCK_CASES:
        B, N, W, multi = case
        d = dims(*case)
        assert saved_layout(d)["total"] == lib.stemgnn_saved_floats(B, N, W, multi), case
        assert scratch_layout(d)["total"] == lib.stemgnn_scratch_floats(B, N, W, multi), case
        assert scratch_layout(d)["dG"][0] == lib.stemgnn_scratch_offset_dG(B, N, W, multi), case
        for r in range(2):
            ch = l2_channels(d, r)
            assert len(ch) == d.U[r] == 4 * d.nf[r] and len(set(ch)) == len(ch) and all(0 <= c < d.C for c in ch)
            # the live bins of branch r: f = 0 .. Wm / 2 (Re), 1 .. ceil(Wm / 2) - 1 (Im), in each of the four orders
            assert sorted(ch) == sorted(k * d.Wm + f for k in range(4) for f in range(r, r + d.nf[r]))
