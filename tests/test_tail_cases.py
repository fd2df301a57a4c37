"""CPU: the case tables of tests/test_hip_tail_stage.py (the fc tail and its losses, csrc/tail.hip), and proof that they reach what
they claim.

stemgnn_fc_tail_plan reports, host only, what the fc-tail launchers do (csrc/tail.hip): rows per block, threads per row, row blocks,
the nacc = (W + 1)(W + H) gradient elements, the partial-sum launch's grid, its block lanes and the blocks it sums per trip, and the
dynamic LDS of each kernel.  It is computed from the block-size constants, the LDS-size functions and the `*_scratch_floats`
functions the launchers use themselves; only the partial-sum kernels' lanes and loads per lane are numbers that mirror the kernels'
text.  Every property below is read from that plan, none from a constant copied into this file -- a block size or an LDS layout
that moves fails here instead of silently dropping an edge from the GPU suite.  Nothing is launched.

What the kernels decide on, and where the tables put a case:
  * sg_fc_tail_train_reduce_kernel walks the row blocks in trips of `reduce_trip` (4 lanes x 8 clamped loads in flight): fewer blocks
    than lanes, exactly one trip, one trip plus a block, a trip plus one block per lane, plus one more;
  * the loss slot i == nacc of the training partials: in a reduce workgroup of its own when nacc is a multiple of 64, and on
    thread 0's second trip through the row kernel's `e < nacc + 1` loop when nacc is a multiple of 256;
  * the `m < M` masks: a last block of 1 row, of rows - 1 rows, and a full one, with more than one block, in both families;
  * the `t = q; t < W; t += row_threads` maps: W and H below, at and one above the threads per row of both families;
  * `m / N`: N = 1, a block that straddles batch elements, N equal to the block and above it;
  * sg_ensure_dyn_lds: only the 64-row backward crosses the 64 KB default, at W >= 63 here."""
import ctypes
import os
import re

import pytest

EINVAL = -10001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_C = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}


def header_signature(name):
    """(restype, argtypes) of `name` as include/stemgnn_hip.h declares it: pointers -> c_void_p, scalars by their C type"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stemgnn_hip.h")).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/stemgnn_hip.h"
    return _C[m.group(1)], [ctypes.c_void_p if "*" in a else _C[a.split()[-2]] for a in m.group(2).split(",")]


TAIL_CASES = [(1, 1, 1, 1), (2, 3, 2, 5), (1, 31, 3, 13), (1, 32, 7, 1), (3, 11, 4, 4), (1, 63, 5, 3), (2, 32, 8, 8), (5, 13, 9, 9),
              (1, 97, 15, 1), (4, 32, 7, 25), (3, 43, 12, 3), (5, 51, 1, 32), (1, 257, 2, 31), (31, 32, 3, 2), (16, 64, 5, 2),
              (5, 205, 5, 2), (9, 128, 4, 1), (5, 231, 6, 2), (2, 7, 64, 32), (4, 3, 64, 1), (3, 5, 1, 32), (3, 5, 63, 31),
              (32, 228, 12, 3)]
QUANTILE_CASES = [(1, 1, 1, 1, 1), (2, 7, 5, 2, 3), (1, 33, 3, 1, 9), (3, 11, 8, 8, 4), (2, 5, 4, 1, 32), (1, 40, 6, 32, 1),
                  (5, 231, 6, 1, 2)]                                  # (B, N, W, HT, Q), the tail's rows H = Q * HT <= 32
ENTRIES = ["stemgnn_fc_tail_supported", "stemgnn_fc_tail_scratch_floats", "stemgnn_fc_tail_plan", "stemgnn_fc_tail_fwd",
           "stemgnn_fc_tail_bwd", "stemgnn_fc_tail_train_scratch_floats", "stemgnn_fc_tail_train", "stemgnn_fc_tail_train_rows",
           "stemgnn_fc_tail_train_finish", "stemgnn_target_valid_count", "stemgnn_fc_tail_train_loss",
           "stemgnn_fc_tail_train_rows_loss", "stemgnn_fc_tail_train_finish_loss", "stemgnn_fc_tail_train_quantile",
           "stemgnn_fc_tail_train_rows_quantile", "stemgnn_fc_tail_train_finish_quantile", "stemgnn_mse_fwd", "stemgnn_mse_bwd"]


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


@pytest.fixture(scope="module")
def plans(lib):
    from stemgnn_amd import _lib

    return {c: _lib.fc_tail_plan(*c) for c in TAIL_CASES}


def quantile_plans():
    from stemgnn_amd import _lib

    return {c: _lib.fc_tail_plan(c[0], c[1], c[2], c[3] * c[4]) for c in QUANTILE_CASES}


def test_tables_are_small_and_distinct():
    assert len(set(TAIL_CASES)) == len(TAIL_CASES) <= 24 and len(set(QUANTILE_CASES)) == len(QUANTILE_CASES) <= 8
    assert max(B * N for B, N, _, _ in TAIL_CASES) == 32 * 228          # nothing above the PEMS07 anchor
    assert all(Q * HT <= 32 for _, _, _, HT, Q in QUANTILE_CASES)


def test_the_plan_is_what_the_scratch_functions_return(lib, plans):
    for (B, N, W, H), p in list(plans.items()) + [((c[0], c[1], c[2], c[3] * c[4]), p) for c, p in quantile_plans().items()]:
        for fam, fn in (("plain", lib.stemgnn_fc_tail_scratch_floats), ("train", lib.stemgnn_fc_tail_train_scratch_floats)):
            f = p[fam]
            assert f["rows"] * f["row_threads"] == 256
            assert f["nblocks"] == -(-B * N // f["rows"])
            assert f["nacc"] == (W + 1) * (W + H)
            assert fn(B, N, W, H) == f["nblocks"] * f["slots"]
            assert f["reduce_grid"] == -(-f["slots"] // 64)
            assert f["reduce_trip"] % f["reduce_lanes"] == 0
            assert [f["lds0_raised"], f["lds1_raised"]] == [int(f["lds0"] > 65536), int(f["lds1"] > 65536)]
        assert p["plain"]["slots"] == p["plain"]["nacc"] and p["train"]["slots"] == p["train"]["nacc"] + 1
        assert p["plain"]["rows"] != p["train"]["rows"]                 # two families, two block sizes


def test_training_block_counts_walk_the_reduce_trips(plans):
    t = [p["train"] for p in plans.values()]
    lanes, trip = t[0]["reduce_lanes"], t[0]["reduce_trip"]
    assert all((f["reduce_lanes"], f["reduce_trip"]) == (lanes, trip) for f in t)
    counts = {f["nblocks"] for f in t}
    assert counts == {1, 2, 3, 4, 5, 8, 9, 31, 32, 33, 36, 37, 228}
    assert any(n < lanes for n in counts)                               # lanes with no block at all
    assert {lanes, lanes + 1} <= counts                                 # one block per lane, and a lane with two
    assert {trip - 1, trip, trip + 1, trip + lanes, trip + lanes + 1} <= counts      # clamped loads: 1 short, none, 1 block over, ...
    assert any(n > 2 * trip and n % trip for n in counts)               # several trips and a ragged last one


def _tail_rows(case, fam):
    return case[0] * case[1] % fam["rows"]


def test_ragged_last_blocks(plans):
    for famname in ("train", "plain"):
        rows = plans[TAIL_CASES[0]][famname]["rows"]
        multi = {_tail_rows(c, p[famname]) for c, p in plans.items() if p[famname]["nblocks"] > 1}
        assert {0, 1, rows - 1} <= multi, (famname, sorted(multi))
        single = {c[0] * c[1] for c, p in plans.items() if p[famname]["nblocks"] == 1}
        assert {1, rows - 1, rows} <= single, (famname, sorted(single))
    plain = {p["plain"]["nblocks"] for p in plans.values()}
    assert {1, 2, 3, 4, 5} <= plain and any(n >= 16 for n in plain)
    assert {c[0] * c[1] % 64 for c in TAIL_CASES} >= {0, 1, 63}


def test_w_and_h_sit_on_the_stride_boundaries(lib, plans):
    Ws, Hs = {c[2] for c in TAIL_CASES}, {c[3] for c in TAIL_CASES}
    for famname in ("plain", "train"):
        T = plans[TAIL_CASES[0]][famname]["row_threads"]
        assert {T - 1, T, T + 1} <= Ws, (famname, T)
        assert {T, T + 1} <= Hs and any(h < T for h in Hs), (famname, T)    # below / at / one above
    assert {plans[TAIL_CASES[0]][f]["row_threads"] for f in ("plain", "train")} == {4, 8}
    # the range limits, found by asking, and one below them
    Wmax = max(w for w in range(1, 200) if lib.stemgnn_fc_tail_supported(w, 1))
    Hmax = max(h for h in range(1, 200) if lib.stemgnn_fc_tail_supported(1, h))
    assert (Wmax, Hmax) == (64, 32) and lib.stemgnn_fc_tail_supported(Wmax, Hmax)
    assert {Wmax, Wmax - 1, 1} <= Ws and {Hmax, Hmax - 1, 1} <= Hs
    assert (Wmax, Hmax) in {(c[2], c[3]) for c in TAIL_CASES} and (Wmax - 1, Hmax - 1) in {(c[2], c[3]) for c in TAIL_CASES}
    qrows = {c[3] * c[4] for c in QUANTILE_CASES}
    assert {1, Hmax} <= qrows and any(c[4] == Hmax for c in QUANTILE_CASES) and any(c[3] == Hmax for c in QUANTILE_CASES)
    assert any(c[3] > 1 and c[4] > 1 for c in QUANTILE_CASES)           # j % HT and j / HT both non-trivial


def test_the_loss_slot_lands_everywhere(plans):
    by_wh = {(c[2], c[3]): p["train"] for c, p in plans.items()}
    nacc = {wh: f["nacc"] for wh, f in by_wh.items()}
    assert any(n < 64 for n in nacc.values()) and any(n > 256 for n in nacc.values())
    own_group = {wh for wh, f in by_wh.items() if f["slots"] % 64 == 1}            # i == nacc is lane 0 of a workgroup of its own
    assert {(3, 13), (7, 1), (63, 31)} <= own_group
    for wh in own_group:
        assert by_wh[wh]["reduce_grid"] == nacc[wh] // 64 + 1
    second_trip = {wh for wh, n in nacc.items() if n % 256 == 0}                  # e == nacc is thread 0's second (or later) element
    assert {(15, 1), (7, 25)} <= second_trip
    assert any(f["slots"] % 64 not in (0, 1) for f in by_wh.values())
    assert second_trip <= own_group                                               # 256 is a multiple of 64
    several = lambda group: {p["train"]["nblocks"] > 1 for c, p in plans.items() if (c[2], c[3]) in group}
    assert several(own_group) == {False, True} and several(second_trip) == {True}   # the slot as one block's sum and as a sum of several


def test_n_against_the_block(plans):
    assert any(c[1] == 1 for c in TAIL_CASES)
    for famname in ("plain", "train"):
        rows = plans[TAIL_CASES[0]][famname]["rows"]
        assert any(c[0] > 1 and c[1] % rows and c[1] < rows for c in TAIL_CASES)      # a block holds rows of several batch elements
        assert any(c[0] > 1 and c[1] % rows and c[1] > rows for c in TAIL_CASES)      # a block straddles two of them
        assert any(c[0] > 1 and c[1] == rows for c in TAIL_CASES), famname            # N is the block
        assert any(c[1] > rows for c in TAIL_CASES)


def test_dynamic_lds_on_both_sides_of_the_default(plans):
    raised = [bool(p["plain"]["lds1_raised"]) for p in plans.values()]            # table order is run order
    assert any(raised) and not all(raised)
    first, last = raised.index(True), len(raised) - 1 - raised[::-1].index(True)
    assert not any(raised[:first]) and first > 0 and last < len(raised) - 1 and not raised[-1]
    assert False in raised[first:last]                                           # a small case between two raised ones
    # today only the 64-row backward needs it; the assertion is on what the plan says, for every kernel
    for p in list(plans.values()) + list(quantile_plans().values()):
        for fam in ("plain", "train"):
            for k in ("lds0", "lds1"):
                assert p[fam][k] <= 150 * 1024
        assert p["plain"]["lds0"] > 0 and p["plain"]["lds1"] > 0 and p["train"]["lds0"] > 0 and p["train"]["lds1"] == 0


def test_refusals(lib):
    out = (ctypes.c_int * 24)()
    assert lib.stemgnn_fc_tail_plan(2, 3, 4, 5, out) == 0
    assert lib.stemgnn_fc_tail_plan(2, 3, 4, 5, None) == EINVAL
    for W in range(-1, 70):
        for H in range(-1, 36):
            ok = bool(lib.stemgnn_fc_tail_supported(W, H))
            assert (lib.stemgnn_fc_tail_plan(2, 3, W, H, out) == 0) == ok, (W, H)
    p = 4096                                                          # a non-NULL pointer value: every call below is refused first
    for B, N, W, H in ((2, 3, 65, 1), (2, 3, 1, 33), (0, 3, 4, 5), (2, 0, 4, 5), (2, 3, 0, 5), (2, 3, 4, 0), (-1, 3, 4, 5),
                       (2, -3, 4, 5), (2, 3, -4, 5), (2, 3, 4, -5)):
        assert lib.stemgnn_fc_tail_plan(B, N, W, H, out) == EINVAL, (B, N, W, H)
        assert lib.stemgnn_fc_tail_fwd(p, p, p, p, p, B, N, W, H, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_bwd(p, p, p, p, p, B, N, W, H, p, p, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train(p, p, p, p, p, p, B, N, W, H, p, p, p, p, p, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train_rows(p, p, p, p, p, p, B, N, W, H, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train_finish(p, B, N, W, H, p, p, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train_loss(p, p, p, p, p, p, B, N, W, H, 1, 0.0, p, p, p, p, p, p, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train_finish_loss(p, B, N, W, H, p, p, p, p, p, p, p, None) == EINVAL
    taus = (ctypes.c_float * 33)(*[(q + 1) / 34 for q in range(33)])
    for HT, Q in ((1, 33), (33, 1), (3, 11), (11, 3), (0, 3), (3, 0), (-3, -11)):                # Q HT = 33, or not positive
        assert lib.stemgnn_fc_tail_train_quantile(p, p, p, p, p, p, 2, 3, 4, HT, Q, taus, p, p, p, p, p, p, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train_rows_quantile(p, p, p, p, p, p, 2, 3, 4, HT, Q, taus, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_train_finish_quantile(p, 2, 3, 4, HT, Q, p, p, p, p, p, p, p, None) == EINVAL
        assert lib.stemgnn_fc_tail_plan(2, 3, 4, HT * Q if HT * Q > 0 else 0, out) == EINVAL
    assert lib.stemgnn_fc_tail_plan(2, 3, 4, 32, out) == 0
    assert lib.stemgnn_fc_tail_plan(1 << 16, 1 << 15, 4, 5, out) == EINVAL          # B N beyond int
    assert lib.stemgnn_mse_fwd(None, p, 8, p, p, None, None) == EINVAL and lib.stemgnn_mse_fwd(p, p, 0, p, p, None, None) == EINVAL
    assert lib.stemgnn_mse_bwd(p, p, 8, None, p, None) == EINVAL and lib.stemgnn_mse_bwd(p, p, 0, p, p, None) == EINVAL


@pytest.mark.parametrize("case", TAIL_CASES, ids=str)
def test_inputs_keep_clear_of_every_kink(case):
    """the seed search and the band asserts of tests/test_hip_loss_tail.case succeed on the CPU; the mask has a whole (b, h) plane
    and, from two training blocks on, a whole row block missing"""
    import torch

    from tests.test_hip_loss_tail import DELTA, case as tail_case, fc64

    B, N, W, H = case
    c = tail_case(B, N, W, H)
    z64, f64 = fc64(c["fsum"].double(), *(p.double() for p in c["prm"]))
    d = (f64 - c["y"].double()).abs()
    assert float(z64.abs().min()) > 1e-5
    assert float(d.min()) >= 0.05 and float((d - DELTA).abs().min()) >= 0.05
    assert bool(c["miss"][B - 1, H - 1].all()) and bool(torch.isnan(c["y_nan"]).eq(c["miss"]).all())
    if B * N >= 64:
        assert bool(c["miss"].permute(0, 2, 1).reshape(B * N, H)[:32].all())


@pytest.mark.parametrize("case", QUANTILE_CASES, ids=str)
def test_quantile_inputs_keep_clear_of_every_kink(case):
    from tests.test_hip_loss_tail import fc64
    from tests.test_hip_quantile_tail import BAND, case as quantile_case

    B, N, W, HT, Q = case
    c = quantile_case(B, N, W, HT, Q)
    z64, f64 = fc64(c["fsum"].double(), *(p.double() for p in c["prm"]))
    assert float(z64.abs().min()) > 1e-5
    dist = (f64.reshape(B, Q, HT, N) - c["y"].double().unsqueeze(1)).abs().min()
    assert float(dist) >= BAND and len(c["taus"]) == Q and bool(c["miss"][B - 1, HT - 1].all())


@pytest.mark.parametrize("name", ENTRIES)
def test_symbol_has_the_headers_signature(lib, name):
    from stemgnn_amd import _lib

    res, args = _lib.SIGNATURES[name]
    args = [ctypes.c_void_p if isinstance(a, type) and issubclass(a, ctypes._Pointer) else a for a in args]     # host arrays
    assert hasattr(lib, name)
    assert (res, args) == header_signature(name)
