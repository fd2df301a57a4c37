"""CPU: the lane map of the packed forward mat-vec waves (csrc/gru_cluster4.h, GRU_FWD_PACK), stated in Python.

A mat-vec wave of the forward instantiations with KF = 34 and 40 (slices of 33..40 units; KF = 32 stays unpacked) holds
the rows of the three gates over TWO lane sets: lane l of
set t owns output o = 64 t + l, which is (gate, unit) = divmod(o, U) with U = ceil(Hd / P) -- the cluster's slice length,
the same in every workgroup, so that the gate wave finds gate g of unit u in row g U + u whatever `un` (the units this
workgroup really owns) is.  An output with unit >= un or o >= 3 U carries zero weights.  Checked exhaustively here:
every live (gate, unit) has exactly one owner, no (set, lane) owns two, and the plan (stemgnn_gru_paths over the range of
tests/test_gru_paths.py) never hands the packed kernels a slice whose 3 U outputs exceed the 128 places."""
import itertools
from ctypes import c_int

import pytest

CUS = 256
SETS, LANES = 2, 64
KF_PACKED = (34, 40)                         # the forward instantiations that pack (gru4_fwd_packs: 32 < KF <= 40)
KF_MAPPED = (32, 34, 40)                     # every KF <= 40 fits the map; the issue's bound is checked for all of them


def owner(gate, unit, U):
    """(set, lane) that holds the weight row of (gate, unit)"""
    return divmod(gate * U + unit, LANES)


def output(t, lane, U, un):
    """(gate, unit) of lane `lane` of set `t`, or None where the lane holds zero weights"""
    o = LANES * t + lane
    gate, unit = divmod(o, U)
    return (gate, unit) if o < 3 * U and unit < un else None


def gate_row(gate, lane, U):
    """the partial-sum row the gate wave's lane `lane` (= unit, < U) reads for `gate`"""
    return gate * U + lane


@pytest.mark.parametrize("U", range(1, 43))
def test_lane_map_is_a_bijection_onto_the_live_outputs(U):
    assert 3 * U <= SETS * LANES                 # (42 is the last U the map has places for; the kernels stop at 40)
    for un in range(0, U + 1):
        live = [(t, lane, output(t, lane, U, un)) for t, lane in itertools.product(range(SETS), range(LANES))]
        got = [x[2] for x in live if x[2] is not None]
        want = [(g, u) for g in range(3) for u in range(un)]
        assert sorted(got) == want, (U, un)                       # every live (gate, unit) exactly once, nothing else
        assert len(set(got)) == len(got)
        for t, lane, gu in live:
            if gu is not None:
                assert owner(*gu, U) == (t, lane), (U, un, t, lane)   # the two directions agree
        for g, u in want:
            t, lane = owner(g, u, U)
            assert 0 <= t < SETS and 0 <= lane < LANES
            assert gate_row(g, u, U) == LANES * t + lane          # where the gate wave looks is where it was written
        # rows the gate wave reads for its dead lanes (un <= lane < U) exist and are zero-weight outputs
        for g, lane in itertools.product(range(3), range(un, U)):
            row = gate_row(g, lane, U)
            assert row < SETS * LANES and output(*divmod(row, LANES), U, un) is None


def test_second_lane_set_edges():
    assert all(owner(g, u, 21)[0] == 0 for g in range(3) for u in range(21))                   # 63 outputs: set 1 empty
    assert [owner(2, u, 22) for u in (19, 20, 21)] == [(0, 63), (1, 0), (1, 1)]                # 66: two lanes in set 1
    assert owner(2, 39, 40) == (1, 55) and owner(2, 32, 33) == (1, 34)                          # 120 and 99 outputs
    assert output(0, 0, 1, 0) is None and output(0, 2, 1, 1) == (2, 0) and output(0, 3, 1, 1) is None


@pytest.fixture(scope="module")
def lib():
    import os

    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_every_packed_plan_fits_two_lane_sets(lib, monkeypatch):
    from stemgnn_amd._lib import SG_GRU_FAM, SG_GRU_PATH_WORDS, SG_GRU_WORD

    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE"):
        monkeypatch.delenv(name, raising=False)
    out = (c_int * SG_GRU_PATH_WORDS)()
    fam, fp, fk = (SG_GRU_WORD[k] for k in ("fwd_family", "fwd_P", "fwd_K"))
    hds = list(range(1, 601)) + list(range(608, 2049, 16)) + [1023, 1025, 2047]
    seen = set()
    for B, Hd in itertools.product(range(1, 301), hds):           # (the forward's plan does not depend on S and W)
        assert lib.stemgnn_gru_paths(B, Hd, Hd, 12, CUS, out) == 0
        if out[fam] != SG_GRU_FAM["cluster4"] or out[fk] > max(KF_MAPPED):
            continue
        P, K = int(out[fp]), int(out[fk])
        U = -(-Hd // P)
        assert K in KF_MAPPED and U <= K and 3 * U <= SETS * LANES, (B, Hd, P, K, U)
        if K in KF_PACKED:
            assert 32 < U <= 40, (B, Hd, P, K, U)                 # what the packed kernels really get: both lane sets in use
            seen.add((P, K))
    # the instantiations that pack: the seven-workgroup kernels and the B > 32 ones at slices of 33..40 units
    assert seen == {(7, 34), (7, 40), (1, 34), (1, 40), (2, 34), (2, 40), (4, 34), (4, 40)}, sorted(seen)
