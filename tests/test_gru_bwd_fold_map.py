"""CPU: the lane map of the folded backward mat-vec waves (csrc/gru_cluster4.h GRU_BWD_FOLD, csrc/gru.hip gru_matvec_fold),
stated in Python.

A mat-vec wave of the backward's OW = 1 instantiations (slices of U <= KU units; the kernels fold at KU = 48 / 58 / 64 and
keep KU = 32 unfolded, the map holds for all four) gives lanes l and 32 + l the two units 2 l and 2 l + 1.  The lower half of the wave (lanes 0..31) walks the k pairs (4 i, 4 i + 1), the upper
half the pairs (4 i + 2, 4 i + 3), i < ceil(KU / 4); a unit >= un or a k >= kn carries a zero weight.  The unfolded form
(gru_matvec: lane = unit, every k) sums k = 0 mod 4 in chain a0.x, 1 in a0.y, 2 in a1.x, 3 in a1.y, each in ascending k,
the tail pair of KU % 4 == 2 in a0, and returns (a0.x + a1.x) + (a0.y + a1.y).  Checked here, with the sums kept as
symbols: every live (unit, k) is multiplied exactly once, every product sits in gru_matvec's chain at gru_matvec's place,
and the three v_permlane32_swap + add rounds leave gru_matvec's association of unit 2 l in lane l and of 2 l + 1 in lane
32 + l, which is the partial-sum row the lane writes."""
import pytest

LANES, HALF = 64, 32
KUS = (32, 48, 58, 64)                       # the backward's instantiations
US = (1, 2, 31, 32, 33, 45, 57, 58, 63, 64)


def ku_of(U):
    return min(k for k in KUS if k >= U)


def pairs(KU):
    return (KU + 3) // 4


def units(lane):
    return 2 * (lane % HALF), 2 * (lane % HALF) + 1


def k_of(lane, i, c):
    """the k of component c of this lane's i-th weight pair"""
    return 4 * i + 2 * (lane // HALF) + c


def out_row(lane):
    """the partial-sum row (= unit) the lane writes"""
    return 2 * (lane % HALF) + lane // HALF


def fold_chains(KU, un, kn):
    """per lane: [[x chain, y chain] of unit 2 l, the same of 2 l + 1]; a chain is the tuple of its live (unit, k) in order"""
    out = []
    for lane in range(LANES):
        per_unit = []
        for u in units(lane):
            per_unit.append([tuple((u, k_of(lane, i, c)) for i in range(pairs(KU)) if u < un and k_of(lane, i, c) < kn)
                             for c in range(2)])
        out.append(per_unit)
    return out


def ref_chains(KU, un, kn):
    """gru_matvec: {unit: {'a0.x': chain, ...}}, written as the loop in csrc/gru.hip runs"""
    out = {}
    for u in range(LANES):
        ch = {"a0.x": [], "a0.y": [], "a1.x": [], "a1.y": []}
        kk = 0
        while kk + 3 < KU:
            ch["a0.x"].append(kk), ch["a0.y"].append(kk + 1), ch["a1.x"].append(kk + 2), ch["a1.y"].append(kk + 3)
            kk += 4
        if KU & 3:
            ch["a0.x"].append(KU - 2), ch["a0.y"].append(KU - 1)
        out[u] = {name: tuple((u, k) for k in ks if u < un and k < kn) for name, ks in ch.items()}
    return out


def permlane32_swap(a, b):
    """v_permlane32_swap a, b: the upper half of a changes places with the lower half of b"""
    return a[:HALF] + b[:HALF], a[HALF:] + b[HALF:]


def add(x, y):
    """a float add as a symbol: it commutes, it does not associate"""
    return ("+",) + tuple(sorted((x, y), key=repr))


def swap_add(a, b):
    a, b = permlane32_swap(a, b)
    return [add(x, y) for x, y in zip(a, b)]


def combine(chains):
    """the three rounds of gru_matvec_fold on the four chains of every lane"""
    c = [[chains[lane][t][comp] for lane in range(LANES)] for t in range(2) for comp in range(2)]
    return swap_add(swap_add(c[0], c[1]), swap_add(c[2], c[3]))


def _cases():
    for U in US:
        for kn in sorted({k for k in (1, 2, 3, 4, 5, U - 1, U) if 1 <= k <= U}):
            for un in sorted({kn, U}):
                yield U, kn, un


@pytest.mark.parametrize("U,kn,un", list(_cases()), ids=lambda v: str(v))
def test_fold_map(U, kn, un):
    KU = ku_of(U)
    assert U <= KU <= LANES and 2 * HALF == LANES and 4 * pairs(KU) <= LANES          # the broadcast row holds every k read
    got, ref = fold_chains(KU, un, kn), ref_chains(KU, un, kn)
    # every live (unit, k) exactly once, nothing else
    seen = [p for lane in got for per_unit in lane for chain in per_unit for p in chain]
    assert sorted(seen) == [(u, k) for u in range(un) for k in range(kn)]
    assert len(set(seen)) == len(seen)
    # every product in gru_matvec's chain, in gru_matvec's order; the tail pair in a0
    for lane in range(LANES):
        acc = "a0" if lane < HALF else "a1"
        for t, u in enumerate(units(lane)):
            assert got[lane][t][0] == ref[u][acc + ".x"], (lane, u)
            assert got[lane][t][1] == ref[u][acc + ".y"], (lane, u)
    if KU & 3:
        assert all((u, k) in ref[u]["a0.x" if k % 2 == 0 else "a0.y"] for u in range(un) for k in (KU - 2, KU - 1) if k < kn)
        # the upper half's last pair does not exist: its k are beyond every slice (weights -0, values +0 there)
        assert k_of(HALF, pairs(KU) - 1, 0) == KU and KU >= U >= kn
    # the combine: (a0.x + a1.x) + (a0.y + a1.y) of the unit the lane writes
    pv = combine(got)
    for lane in range(LANES):
        u = out_row(lane)
        assert u in units(lane) and u == (lane % HALF) * 2 + lane // HALF
        r = ref[u]
        assert pv[lane] == add(add(r["a0.x"], r["a1.x"]), add(r["a0.y"], r["a1.y"])), (lane, u)
    assert sorted(out_row(lane) for lane in range(LANES)) == list(range(LANES))       # one writer per row


def test_swap_semantics_and_edges():
    a, b = permlane32_swap(list(range(64)), list(range(100, 164)))
    assert a == list(range(32)) + list(range(100, 132)) and b == list(range(32, 64)) + list(range(132, 164))
    assert [ku_of(U) for U in US] == [32, 32, 32, 32, 48, 48, 58, 58, 64, 64]
    assert [pairs(k) for k in KUS] == [8, 12, 15, 16]
    assert units(0) == (0, 1) and units(31) == (62, 63) and units(32) == (0, 1) and units(63) == (62, 63)
    assert [k_of(0, 14, c) for c in (0, 1)] == [56, 57] and [k_of(32, 13, c) for c in (0, 1)] == [54, 55]     # KU 58: the last live pairs
    assert (out_row(0), out_row(32), out_row(31), out_row(63)) == (0, 1, 62, 63)
