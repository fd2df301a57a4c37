"""CPU: the shapes of tests/test_hip_shape_domain.py reach both sides of every launch-path decision of csrc/block.hip
(stemgnn_block_paths asks the launchers' own predicates, host only).  If a threshold moves, this fails here instead of the
GPU suite quietly losing a path."""
import pytest

from tests.test_hip_shape_domain import EDGE_CASES, SWEEP_CASES, sweep_cases

CASES = EDGE_CASES + SWEEP_CASES


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

    N, W, multi, H, B = case
    v = lib.stemgnn_block_paths(B, N, W, multi, splits)
    assert v >= 0, (case, v)
    return {k: bool(v & bit) for k, bit in SG_PATH.items()}


def test_sweep_literals_are_the_seeded_draw():
    assert SWEEP_CASES == sweep_cases()


def test_cases_are_in_the_constructor_range():
    for N, W, multi, H, B in CASES:
        assert 1 <= N and 1 <= W <= 64 and 1 <= multi and 1 <= H <= 32 and 1 <= B, (N, W, multi, H, B)
    assert len(set(CASES)) == len(CASES)


def test_every_path_bit_is_reached_both_ways(lib):
    from stemgnn_amd._lib import SG_PATH

    seen = {k: set() for k in SG_PATH}
    for c in CASES:
        for k, v in _paths(lib, c).items():
            seen[k].add(v)
    missing = {k: sorted({True, False} - s) for k, s in seen.items() if s != {True, False}}
    assert not missing, missing
    # the bf16x2 forms (STEMGNN_DTYPE=bf16x2): fused split-bf16 GLU forward / data-gradient chain or the per-layer launches
    ok = {bool(lib.stemgnn_glu_fused_bf16_ok(W, multi, 2)) for N, W, multi, H, B in CASES}
    assert ok == {True, False}
    for k in ("glu_fwd_fused", "glu_dgrad_fused"):
        assert {_paths(lib, c, 2)[k] for c in CASES} == {True, False}, k


def test_pinned_anchors(lib):
    pems = _paths(lib, (228, 12, 5, 3, 32))
    assert not pems.pop("long_k") and all(pems.values()), pems        # PEMS07: every fused path, 16-wave heads backward
    p = _paths(lib, (7, 64, 9, 4, 2))
    assert not p["heads_bwd_fused"] and not p["heads_fwd_fused"]      # per-stage heads backward (and forward)
    p = _paths(lib, (6, 64, 5, 32, 2))
    assert not p["heads_fwd_fused"] and p["long_k"] and p["heads_bwd_fused"] and not p["glu_fwd_fused"]
    p = _paths(lib, (40, 64, 3, 8, 4))
    assert not p["heads_fwd_fused"] and p["long_k"]                   # the per-stage inference heads of test_hip_predict
    p = _paths(lib, (5, 64, 1, 1, 3))
    assert p["glu_fwd_fused"] and not p["glu_dgrad_fused"]            # CP = 256 exactly: fused forward (dgrad: 3 W > 64)
    assert not _paths(lib, (17, 13, 5, 7, 1))["glu_fwd_fused"]        # CP = 272
    for c in [(1, 1, 1, 1, 1), (2, 2, 1, 1, 1), (3, 1, 3, 2, 2)]:     # W*multi <= 3: 4 waves (KF <= 128), slab weight gradients
        p = _paths(lib, c)
        assert p["heads_bwd_fused"] and not p["heads_bwd_16w"] and not p["wgrad_fused"], (c, p)


def test_block_paths_rejects_bad_arguments(lib):
    from stemgnn_amd._lib import SG_EINVAL

    for args in ((0, 5, 12, 5, 0), (2, 0, 12, 5, 0), (2, 5, 0, 5, 0), (2, 5, 12, 0, 0), (2, 5, 12, 5, 1)):
        assert lib.stemgnn_block_paths(*args) == SG_EINVAL, args
