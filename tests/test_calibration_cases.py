"""CPU: the case lists of tests/test_hip_calibration_stage.py (the batch side of the conformal family: stemgnn_conformal_fit / _apply
of csrc/conformal.hip, stemgnn_seasonal_fit / _apply and stemgnn_quantile_store_seasonal of csrc/seasonal.hip, stemgnn_quantile_finish
/ _store of csrc/quantile_serve.hip, with the fit and the column kernel they share, csrc/conformal_fit.h and csrc/quantile_column.h),
their inputs and references, and proof that they reach what they claim.

stemgnn_calibration_plan reports, host only, what each launcher does for a shape (include/stemgnn_hip.h): the fit's form, grouping,
tiles, rows per wave, chunk count with the bound that set it, row trips, pick workgroups and -- with a season -- the walk; the
applies' VEC, grid, cap and trips; the column kernel's VEC, threads, LDS, planes, workgroup shape, column and window blocks, window
trips and the store's target copy.  The launchers take their geometry from the same static functions (csrc/calibration_plan.h), so
every class below is decided by what the plan says, none by a threshold copied into this file.  CLASSES names every launch decision
the device suite must reach; test_class_is_reached is parametrised over it, so taking the cases of any one class out of the lists
fails that class's test.  The plan is asked with the compute units of the current device, 256 where there is none; the device suite
asks again on the device.

Cases (the smallest shapes that reach a class at 256 compute units; the largest buffer of the suite is 16.9 MB):
  fit            (count, H, N, P, Q, per_step, per_node), each run masked and unmasked
                   columns: (1408, 3, 7) one tile of 21 over three steps, 22 chunks set by the rows | (2, 32, 1024) 1 024 full tiles,
                   one chunk because tiles KP >= 4 CUs | (300, 3, 37) four tiles, the last of 15, for both per_step | (70, 1, 33) a last
                   tile of one column | (1537, 3, 228) 22 tiles, 24 chunks set by the blocks wanted
                   stream: (5, 2, 12) one chunk, L = N and L = H N | (2100, 1, 8, P = 16) 17 chunks set by the elements |
                   (19, 3, 1200, P = 16) 64 chunks set by the blocks wanted, 5 trips
  seasonal_fit   (count, H, N, P, Q, per_step, per_node, period, K, phase, origin), origin an int (origin0), "consecutive" (the same
                   origins as a tensor) or "scattered"
                   DIRECT in both forms with a negative origin0 and its "consecutive" twin, which skips; K = 1; 2 walk > count;
                   period 48 > count 40 (runs = 2, buckets without a row); K = 4 over a period of 10; a scattered int64 tensor
  apply          (count, Q, H, N, mis, in_place): float4 and scalar by N and by each address, 2 048 capped workgroups with a second trip
  seasonal_apply (count, Q, H, N, mis, in_place, origin): the same, a second wave trip over 8 193 segments, three lane trips (N = 228)
  column         (count, Q, H, N, rearrange, caller, mis, pos, capacity), caller one of finish_in_place, finish_out, store,
                   seasonal_apply, seasonal_store
                   (4097, 2, 1, 257) two column blocks, the last of one column, 2 048 capped window blocks, three window trips |
                   (2049, 2, 1, 1028) the same in the vector form, two trips | (1030, 3, 1, 301) a ragged last block of 45, one plane |
                   T = 64, 128, 192, 256 | scalar by N, by Q = 17 and by the address of src and of dst | wpb = 1 with 85 idle threads |
                   the store with pos[0] = -3 and pos[0] + B > capacity, target by float4, by scalar (H N = 21) and by each address
Inputs: quarter-grid values with many ties, +-inf, +-0 and NaN; about 10 % NaN targets; NaN forecasts on valid targets; the (H - 1,
N / 2) position without any valid target; with P >= 2 a last pair whose coverage puts its rank beyond every group's size (+inf).
The column kernel's columns are drawn from nine values (both zeros, both infinities, two NaN payloads), most put in descending order.

Sensitivity: a class that says "a further trip, tile, chunk, column block or window trip" must matter.  For each such class the
reference is computed twice here -- in full, and with that class's share of the work left out (fit: the target rows beyond the first
chunk or the first trip of every chunk set absent; apply and column kernel: the outputs of the last tile, block or further trips left
as the buffer was) -- and the expected outputs must differ.

The file also holds the plan's own refusals, the host-only refusals of the entries that tests/test_conformal_abi.py,
tests/test_seasonal_abi.py and tests/test_quantile_serve_abi.py do not have, and the check that the plan's CU word is stemgnn_num_cus().

Findings: none on the CPU side.  Moving the launch arithmetic of the five launch sites into csrc/calibration_plan.h changed no decision
(the pre-existing suites pass with the same bits).  The plan agrees with the issue's starting points; one was replaced by a smaller
shape: (4100, 3, 1, 300, 0) takes its two column blocks and three window trips only with a misaligned buffer (14.8 MB), and
(4097, 2, 1, 257, 1), scalar by N, takes them at 8.4 MB, while (1030, 3, 1, 301, 0) has the ragged last block on one plane.
What the device suite found is in its own docstring."""
import ctypes
from collections import namedtuple

import numpy as np
import pytest

from tests.helpers import conformal_ref as CR
from tests.helpers import seasonal_ref as SR
from tests.test_serving_cases import differ, grid, lib, same_bits, same_nan_aware  # noqa: F401  (lib: the module fixture)

EINVAL = -10001
F32 = np.float32
SEED = 20261021

Fit = namedtuple("Fit", "count H N P Q per_step per_node")
SFit = namedtuple("SFit", "count H N P Q per_step per_node period K phase origin")
Apply = namedtuple("Apply", "count Q H N mis in_place")
SApply = namedtuple("SApply", "count Q H N mis in_place origin")
Col = namedtuple("Col", "count Q H N rearrange caller mis pos capacity")

FIT_CASES = [
    Fit(1408, 3, 7, 2, 5, 1, 1), Fit(2, 32, 1024, 1, 3, 1, 1), Fit(300, 3, 37, 2, 5, 1, 1), Fit(300, 3, 37, 2, 5, 0, 1),
    Fit(70, 1, 33, 1, 3, 1, 1), Fit(1537, 3, 228, 2, 4, 1, 1),
    Fit(5, 2, 12, 1, 3, 1, 0), Fit(5, 2, 12, 1, 3, 0, 0), Fit(2100, 1, 8, 16, 32, 1, 0), Fit(19, 3, 1200, 16, 32, 0, 0),
]
SFIT_CASES = [
    SFit(1408, 3, 7, 2, 5, 1, 1, 48, 24, 5, -5), SFit(1408, 3, 7, 2, 5, 1, 1, 48, 24, 5, "consecutive"),
    SFit(2100, 1, 8, 16, 32, 1, 0, 48, 24, 0, 7), SFit(2100, 1, 8, 16, 32, 1, 0, 48, 24, 0, "consecutive"),
    SFit(300, 3, 37, 1, 3, 1, 1, 7, 1, 0, 3), SFit(70, 3, 11, 1, 3, 1, 0, 48, 4, 9, 11),
    SFit(40, 2, 5, 1, 3, 1, 1, 48, 24, 0, -7), SFit(40, 2, 5, 1, 3, 1, 1, 48, 24, 0, "consecutive"),
    SFit(300, 3, 37, 2, 5, 0, 1, 10, 4, 3, 2), SFit(300, 3, 37, 2, 5, 0, 1, 10, 4, 3, "consecutive"),
    SFit(257, 2, 9, 1, 3, 0, 0, 12, 4, 1, "scattered"),
]
APPLY_CASES = [
    Apply(9, 3, 3, 65, 0, 0), Apply(9, 3, 3, 68, 0, 0), Apply(9, 3, 3, 68, 0, 1), Apply(9, 3, 3, 68, 1, 0), Apply(9, 3, 3, 68, 2, 0),
    Apply(130, 3, 3, 449, 0, 0), Apply(260, 3, 3, 900, 0, 1),
]
SAPPLY_CASES = [
    SApply(9, 3, 3, 65, 0, 0, -4), SApply(9, 3, 3, 68, 0, 0, "scattered"), SApply(9, 3, 3, 68, 0, 1, "scattered"),
    SApply(9, 3, 3, 68, 1, 0, "scattered"), SApply(9, 3, 3, 68, 2, 0, "scattered"),
    SApply(2731, 3, 3, 5, 0, 0, 5), SApply(2731, 3, 3, 8, 0, 1, 5), SApply(37, 3, 3, 228, 0, 0, -4),
]
COLUMN_CASES = [
    Col(4097, 2, 1, 257, 1, "finish_out", 0, 0, 0), Col(2049, 2, 1, 1028, 1, "finish_in_place", 0, 0, 0),
    Col(1030, 3, 1, 301, 0, "finish_out", 0, 0, 0),
    Col(5, 16, 1, 8, 1, "finish_out", 0, 0, 0), Col(5, 16, 1, 8, 0, "finish_in_place", 0, 0, 0),
    Col(5, 5, 3, 8, 1, "finish_out", 0, 0, 0), Col(5, 5, 3, 8, 1, "finish_out", 1, 0, 0), Col(5, 5, 3, 8, 1, "finish_out", 2, 0, 0),
    Col(5, 17, 1, 8, 1, "finish_in_place", 0, 0, 0), Col(5, 32, 3, 5, 1, "finish_out", 0, 0, 0),
    Col(3, 3, 3, 228, 1, "seasonal_apply", 0, 0, 0), Col(3, 9, 3, 228, 1, "seasonal_apply", 0, 0, 0),
    Col(7, 3, 2, 20, 1, "store", 0, 2, 20), Col(7, 3, 2, 20, 1, "store", 4, 2, 20), Col(7, 3, 2, 20, 1, "store", 8, 2, 20),
    Col(7, 3, 2, 20, 1, "store", 0, -3, 20), Col(7, 3, 2, 20, 0, "store", 0, 16, 20), Col(7, 3, 1, 21, 1, "store", 0, 2, 20),
    Col(7, 3, 2, 20, 1, "seasonal_store", 0, 2, 20), Col(7, 3, 2, 20, 1, "seasonal_store", 0, -3, 3),
]
CASES = {"fit": FIT_CASES, "seasonal_fit": SFIT_CASES, "apply": APPLY_CASES, "seasonal_apply": SAPPLY_CASES, "column": COLUMN_CASES}
SEASON = (12, 4, 5)                                                     # (period, K, phase) of the seasonal applies and stores
T0 = 31                                                                 # t_dev[0] of the seasonal store


def _is_store(c):
    return c.caller in ("store", "seasonal_store")


def plan_shape(entry, c):
    return {"fit": lambda: (c.count, c.H, c.N, c.P, c.per_step, c.per_node),
            "seasonal_fit": lambda: (c.count, c.H, c.N, c.P, c.per_step, c.per_node, c.period, c.K, int(isinstance(c.origin, str))),
            "apply": lambda: (c.count, c.Q, c.H, c.N), "seasonal_apply": lambda: (c.count, c.Q, c.H, c.N),
            "column": lambda: (c.count, c.Q, c.H, c.N, c.rearrange, int(_is_store(c)))}[entry]()


def plan(entry, c, mis=None):
    from stemgnn_amd import _lib

    return _lib.calibration_plan(entry, *plan_shape(entry, c), misaligned=getattr(c, "mis", 0) if mis is None else mis)


def _name(table, value):
    return {v: k for k, v in table.items()}[value]


def _form(p):
    from stemgnn_amd import _lib

    return _name(_lib.SG_CALIBRATION_FORM, p["form"])


def _bound(p):
    from stemgnn_amd import _lib

    return _name(_lib.SG_CALIBRATION_BOUND, p["bound"])


def _why(p):
    from stemgnn_amd import _lib

    return _name(_lib.SG_CALIBRATION_WALK, p["why"])


def _by_address(entry, c, p, bit, word="vec"):
    """scalar because of ONE buffer's address: that bit alone is set, and without it the same shape runs float4"""
    return c.mis == bit and p[word] == 1 and plan(entry, c, 0)[word] == 4


def _cols(p):
    return _form(p) == "columns"


def _empty_buckets(c):
    """seasonal fit: buckets no (row, step) falls into, by the numpy bucket formula"""
    return set(range(c.K)) - set(SR.buckets_of(sfit_origins(c), c.H, (c.period, c.K, c.phase)).reshape(-1).tolist())


# class name -> (entry, predicate(case, plan)); `lambda c, p, k=k` binds the loop value
CLASSES = {
    # ---- fit, column form
    "fit columns/one tile": ("fit", lambda c, p: _cols(p) and p["tiles"] == 1),
    "fit columns/several tiles, ragged last": ("fit", lambda c, p: _cols(p) and p["tiles"] >= 2 and 1 < p["wd_last"] < p["tile"]),
    "fit columns/a last tile of one column": ("fit", lambda c, p: _cols(p) and p["tiles"] >= 2 and p["wd_last"] == 1),
    "fit columns/a full tile, rpw = 2": ("fit", lambda c, p: _cols(p) and p["Cc"] >= p["tile"] and p["rpw_full"] == 2),
    "fit columns/chunks set by the rows": ("fit", lambda c, p: _cols(p) and _bound(p) == "size" and 1 < p["chunks"] == p["by_size"] < p["want"]),
    "fit columns/chunks set by the blocks wanted": ("fit", lambda c, p: _cols(p) and _bound(p) == "wanted" and 1 < p["chunks"] == p["want"] < p["by_size"]),
    "fit columns/one chunk because tiles KP >= 4 CUs": ("fit", lambda c, p: _cols(p) and p["want"] == 1 == p["chunks"] and p["tiles"] * p["KP"] >= p["blocks_wanted"]),
    "fit columns/two or more row trips inside a chunk": ("fit", lambda c, p: _cols(p) and p["trips"] >= 2 and p["chunks"] >= 2),
    "fit columns/Hr = 1": ("fit", lambda c, p: _cols(p) and p["Hr"] == 1 < c.H),
    "fit columns/Hr = H": ("fit", lambda c, p: _cols(p) and p["Hr"] == c.H > 1),
    "fit columns/a tile that spans two steps": ("fit", lambda c, p: _cols(p) and c.per_step and c.N < p["tile"] and p["Cc"] > c.N),
    # ---- fit, stream form
    "fit stream/one chunk": ("fit", lambda c, p: _form(p) == "stream" and p["chunks"] == 1 == p["grid_x"]),
    "fit stream/chunks set by the elements": ("fit", lambda c, p: _form(p) == "stream" and _bound(p) == "size" and 1 < p["chunks"] == p["by_size"] < p["want"]),
    "fit stream/chunks set by the blocks wanted": ("fit", lambda c, p: _form(p) == "stream" and _bound(p) == "wanted" and 1 < p["chunks"] == p["want"] < p["by_size"]),
    "fit stream/two or more trips of thread 0": ("fit", lambda c, p: _form(p) == "stream" and p["trips"] >= 2 and p["chunks"] >= 2),
    "fit stream/L = N": ("fit", lambda c, p: _form(p) == "stream" and p["L"] == c.N < c.H * c.N),
    "fit stream/L = H N": ("fit", lambda c, p: _form(p) == "stream" and p["L"] == c.H * c.N > c.N),
    # ---- fit, pick
    "fit pick/idle waves in the last workgroup": ("fit", lambda c, p: p["pick_idle"] > 0),
    "fit pick/several workgroups, none idle": ("fit", lambda c, p: p["pick_idle"] == 0 and p["pick_blocks"] > 1),
    # ---- seasonal fit
    "seasonal fit/DIRECT, columns": ("seasonal_fit", lambda c, p: p["direct"] == 1 and _why(p) == "direct" and _cols(p)),
    "seasonal fit/DIRECT, stream": ("seasonal_fit", lambda c, p: p["direct"] == 1 and _form(p) == "stream"),
    "seasonal fit/skipping, an origins tensor": ("seasonal_fit", lambda c, p: p["direct"] == 0 and _why(p) == "origins"),
    "seasonal fit/skipping, a scattered origins tensor": ("seasonal_fit", lambda c, p: _why(p) == "origins" and c.origin == "scattered"),
    "seasonal fit/skipping, K = 1": ("seasonal_fit", lambda c, p: p["direct"] == 0 and _why(p) == "one_bucket"),
    "seasonal fit/skipping, 2 walk > count": ("seasonal_fit", lambda c, p: p["direct"] == 0 and _why(p) == "long" and 2 * p["walk"] > c.count),
    "seasonal fit/DIRECT, period > count, runs = 2": ("seasonal_fit", lambda c, p: p["direct"] == 1 and p["runs"] == 2 and c.period > c.count),
    "seasonal fit/DIRECT, K does not divide the period": ("seasonal_fit", lambda c, p: p["direct"] == 1 and c.period % c.K != 0),
    "seasonal fit/DIRECT, origin0 negative": ("seasonal_fit", lambda c, p: p["direct"] == 1 and c.origin < 0),
    "seasonal fit/a bucket that no row falls into": ("seasonal_fit", lambda c, p: p["direct"] == 1 and len(_empty_buckets(c)) > 0),
    "seasonal fit/DIRECT, Hr = H": ("seasonal_fit", lambda c, p: p["direct"] == 1 and _cols(p) and p["Hr"] == c.H > 1),
    # ---- the column kernel's callers and the store
    "column/T = 256": ("column", lambda c, p: p["threads"] == 256), "column/T = 192": ("column", lambda c, p: p["threads"] == 192),
    "column/T = 128": ("column", lambda c, p: p["threads"] == 128), "column/T = 64": ("column", lambda c, p: p["threads"] == 64),
    "column/one plane": ("column", lambda c, p: p["planes"] == 1 and not c.rearrange),
    "column/two planes": ("column", lambda c, p: p["planes"] == 2 and c.rearrange),
    "column/float4": ("column", lambda c, p: p["vec"] == 4),
    "column/scalar by N": ("column", lambda c, p: p["vec"] == 1 and c.mis == 0 and plan("column", c._replace(N=(c.N + 3) // 4 * 4))["vec"] == 4),
    "column/scalar by Q > 16": ("column", lambda c, p: p["vec"] == 1 and c.mis == 0 and plan("column", c._replace(Q=2))["vec"] == 4),
    "column/scalar by the address of src": ("column", lambda c, p: _by_address("column", c, p, 1)),
    "column/scalar by the address of dst": ("column", lambda c, p: _by_address("column", c, p, 2)),
    "column/wpb > 1": ("column", lambda c, p: p["wpb"] > 1), "column/wpb = 1": ("column", lambda c, p: p["wpb"] == 1 == p["col_blocks"]),
    "column/idle threads, wpb > 1": ("column", lambda c, p: p["idle"] > 0 and p["wpb"] > 1),
    "column/idle threads, wpb = 1": ("column", lambda c, p: p["idle"] > 0 and p["wpb"] == 1),
    "column/two or more column blocks, ragged last": ("column", lambda c, p: p["col_blocks"] >= 2 and p["vec"] < p["cols_last"] < p["cpb"] * p["vec"]),
    "column/a last column block of one column": ("column", lambda c, p: p["col_blocks"] >= 2 and p["cols_last"] == 1),
    "column/a last column block of one float4": ("column", lambda c, p: p["col_blocks"] >= 2 and p["cols_last"] == 4 == p["vec"]),
    "column/win_blocks capped, a second window trip": ("column", lambda c, p: p["capped"] == 1 and p["win_trips"] >= 2),
    "column/win_blocks capped, a third window trip": ("column", lambda c, p: p["capped"] == 1 and p["win_trips"] >= 3),
    "column/win_blocks not capped": ("column", lambda c, p: p["capped"] == 0 and p["win_blocks"] > 1 and p["win_trips"] == 1),
    "column/store, target by float4": ("column", lambda c, p: p["grid_y"] == 2 and p["tvec"] == 4),
    "column/store, target scalar by H N": ("column", lambda c, p: p["grid_y"] == 2 and p["tvec"] == 1 and c.mis == 0),
    "column/store, target scalar by the address of target": ("column", lambda c, p: p["grid_y"] == 2 and _by_address("column", c, p, 4, "tvec")),
    "column/store, target scalar by the address of out_target": ("column", lambda c, p: p["grid_y"] == 2 and _by_address("column", c, p, 8, "tvec")),
    "column/store, pos[0] negative": ("column", lambda c, p: p["grid_y"] == 2 and c.pos < 0 < c.pos + c.count),
    "column/store, pos[0] + B > capacity": ("column", lambda c, p: p["grid_y"] == 2 and c.pos < c.capacity < c.pos + c.count),
    "column/store, more windows than target workgroups": ("column", lambda c, p: p["grid_y"] == 2 and p["target_trips"] >= 2),
    "column/seasonal store, rows dropped at both ends": ("column", lambda c, p: c.caller == "seasonal_store" and c.pos < 0 and c.pos + c.count > c.capacity),
}
for _caller in ("finish_in_place", "finish_out", "store", "seasonal_apply", "seasonal_store"):
    CLASSES[f"column/caller {_caller}"] = ("column", lambda c, p, k=_caller: c.caller == k and p["grid_y"] == (2 if _is_store(c) else 1))
for _e, _what in (("apply", "thread 0"), ("seasonal_apply", "wave 0")):
    CLASSES.update({
        f"{_e}/float4": (_e, lambda c, p: p["vec"] == 4),
        f"{_e}/scalar by N": (_e, lambda c, p: p["vec"] == 1 and c.mis == 0),
        f"{_e}/scalar by the address of forecast": (_e, lambda c, p, e=_e: _by_address(e, c, p, 1)),
        f"{_e}/scalar by the address of out": (_e, lambda c, p, e=_e: _by_address(e, c, p, 2)),
        f"{_e}/cap not binding": (_e, lambda c, p: p["capped"] == 0 and p["trips"] == 1 and p["grid_x"] > 1),
        f"{_e}/cap binding, a second trip of {_what}, float4": (_e, lambda c, p: p["capped"] == 1 and p["trips"] >= 2 and p["vec"] == 4),
        f"{_e}/cap binding, a second trip of {_what}, scalar": (_e, lambda c, p: p["capped"] == 1 and p["trips"] >= 2 and p["vec"] == 1),
        f"{_e}/in place": (_e, lambda c, p: c.in_place == 1), f"{_e}/out of place": (_e, lambda c, p: c.in_place == 0),
    })
CLASSES["seasonal_apply/three or more lane trips over a segment"] = ("seasonal_apply", lambda c, p: p["lane_trips"] >= 3)
CLASSES["seasonal_apply/a scattered origins tensor"] = ("seasonal_apply", lambda c, p: c.origin == "scattered")
CLASSES["seasonal_apply/origin0 negative"] = ("seasonal_apply", lambda c, p: c.origin != "scattered" and c.origin < 0)


def reached(name, cases=None):
    entry, pred = CLASSES[name]
    return [c for c in (CASES[entry] if cases is None else cases) if pred(c, plan(entry, c))]


@pytest.mark.parametrize("name", list(CLASSES))
def test_class_is_reached(lib, name):
    """at least one case of the entry's list is in the class, according to stemgnn_calibration_plan; without those cases none is"""
    hit = reached(name)
    assert hit, f"no case of {CLASSES[name][0]} reaches `{name}`"
    rest = [c for c in CASES[CLASSES[name][0]] if c not in hit]
    assert not reached(name, rest)


def largest_buffer_bytes(entry, c):
    Q = c.Q
    return 4 * c.count * Q * c.H * c.N


def test_lists_are_small_distinct_and_cover_every_entry(lib):
    from stemgnn_amd import _lib

    assert set(CASES) == set(_lib.SG_CALIBRATION_ENTRY) == {CLASSES[k][0] for k in CLASSES}
    for entry, cases in CASES.items():
        assert len(set(cases)) == len(cases) <= 20, entry
        assert max(largest_buffer_bytes(entry, c) for c in cases) < 20e6, entry
    # every misaligned case has its aligned twin in the list, every "consecutive" seasonal fit the DIRECT run of the same rows
    for entry in ("apply", "seasonal_apply", "column"):
        for c in CASES[entry]:
            assert c.mis == 0 or c._replace(mis=0) in CASES[entry], c
    for c in SFIT_CASES:
        if c.origin == "consecutive":
            twin = sfit_twin(c)
            assert plan("seasonal_fit", twin)["direct"] == 1 and plan("seasonal_fit", c)["direct"] == 0, c


def test_the_plan_uses_the_devices_compute_units(lib):
    cus = lib.stemgnn_num_cus()
    assert cus > 0
    for entry, cases in CASES.items():
        p = plan(entry, cases[0])
        assert p["cus"] == cus, entry
    p = plan("fit", FIT_CASES[0])
    assert p["blocks_wanted"] % cus == 0 and plan("apply", APPLY_CASES[0])["cap"] % cus == 0


# ---- inputs: generated once per case, numpy only -------------------------------------------------------------------------------------
def _rng(c, salt=0):
    return np.random.default_rng(SEED + salt + sum((i + 1) * int(v) for i, v in enumerate(c) if isinstance(v, (int, np.integer))))


def pairs_of(P, Q):
    return tuple((p, Q - 1 - p) for p in range(P))


def coverages(P):
    """the last pair of several asks for a rank beyond every group's size: its offsets are +inf"""
    cov = [0.8, 0.4, 0.6, 0.2][:P] if P <= 4 else [0.05 + 0.9 * p / P for p in range(P)]
    if P >= 2:
        cov[-1] = 1 - 1e-9
    return cov


def fit_data(c):
    """(target [count, H, N], forecast [count, Q, H, N]); the same for a seasonal case and its twin"""
    key = Fit(c.count, c.H, c.N, c.P, c.Q, c.per_step, c.per_node)
    rng = _rng(key, 11)
    y = grid(rng, (c.count, c.H, c.N), nan=0.10)
    f = grid(rng, (c.count, c.Q, c.H, c.N), nan=0.02, lo=-8, hi=9)
    for lo, hi in pairs_of(c.P, c.Q):
        f[:, lo] -= F32(1)
        f[:, hi] += F32(1)
    drift = ((np.arange(c.count) * 8 // c.count) / 4).astype(F32).reshape(-1, 1, 1)      # later rows hold other values
    y = np.where(drift > 0, y + drift, y).astype(F32)
    y[:, c.H - 1, c.N // 2] = np.nan                                   # one position without any valid target
    return y, f


def sfit_twin(c):
    """the DIRECT run of a "consecutive" case: the list's case with the same shape and an int origin"""
    return next(o for o in SFIT_CASES if not isinstance(o.origin, str) and o._replace(origin="consecutive") == c)


def sfit_origins(c):
    if c.origin == "consecutive":
        return SR.origins_of(sfit_twin(c).origin, c.count)
    if c.origin == "scattered":
        return SR.scattered_origins(c.count, _rng(c, 12))
    return SR.origins_of(c.origin, c.count)


def fit_ref(c, masked, y=None):
    yy, f = fit_data(c)
    y = yy if y is None else y
    if isinstance(c, SFit):
        return SR.fit_np(y, f, sfit_origins(c), pairs_of(c.P, c.Q), coverages(c.P), (c.period, c.K, c.phase), c.per_step, c.per_node, masked)
    return CR.fit_np(y, f, pairs_of(c.P, c.Q), coverages(c.P), c.per_step, c.per_node, masked)


def origins_of(c):
    """the origins of a seasonal apply (or seasonal column) case"""
    o = getattr(c, "origin", -4)
    return SR.scattered_origins(c.count, _rng((c.count, c.Q, c.H, c.N), 13)) if o == "scattered" else SR.origins_of(o, c.count)


def apply_data(c):
    """(forecast [count, Q, H, N], offsets [(K,) 1, H, N]) with one pair (0, Q - 1), per step and per node"""
    seasonal = isinstance(c, SApply)
    rng = _rng(c._replace(mis=0, in_place=0), 14)
    f = grid(rng, (c.count, c.Q, c.H, c.N), nan=0.03)
    shape = ((SEASON[1],) if seasonal else ()) + (1, c.H, c.N)
    off = (rng.integers(-6, 7, size=shape) / 4).astype(F32)
    off.reshape(-1)[:3] = np.inf, -0.0, 0.25
    return f, off


def apply_ref(c):
    f, off = apply_data(c)
    pairs = ((0, c.Q - 1),)
    if isinstance(c, SApply):
        return SR.apply_np(f, off, origins_of(c), pairs, SEASON)
    return CR.apply_np(f, off, pairs, True, True)


# ---- the column kernel -------------------------------------------------------------------------------------------------------------
POOL = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc01234, 0xffc00001], np.uint32).view(F32)
POOL = np.concatenate([POOL, np.array([-1.5, 0.5, 2.0], F32)])
FILL = F32(-555.5)                                                      # what the result slabs of a store hold before the call


def stable_sort(x):
    """the order of stage a along axis 1: fp32's with -0 == +0, NaN above everything, ties (NaNs too) in row order; a selection"""
    nan = np.isnan(x)
    order = np.lexsort((np.where(nan, F32(0), x), nan), axis=1)         # the last key is the primary one; lexsort is stable
    return np.take_along_axis(x, order, axis=1)


def column_data(c):
    key = c._replace(mis=0, caller="", pos=0, capacity=0)
    rng = _rng(key, 15)
    x = POOL[rng.integers(0, POOL.size, size=(c.count, c.Q, c.H, c.N))]
    col = np.arange(c.count * c.H * c.N).reshape(c.count, 1, c.H, c.N)
    x = np.where(col % 4 != 3, stable_sort(x)[:, ::-1], x).astype(F32)  # three columns in four descending: most have to move
    x = np.ascontiguousarray(x)
    seasonal = c.caller.startswith("seasonal")
    shape = ((SEASON[1],) if seasonal else ()) + (1, c.H, 1)            # one pair, per step, nodes pooled
    off = (rng.integers(-6, 7, size=shape) / 4).astype(F32)
    off.reshape(-1)[0] = 0.75
    target = grid(rng, (c.count, c.H, c.N))
    return x, off, target


def column_ref(c):
    """(rows [count, Q, H, N], ordered: the columns after stage a) -- stage a, then the apply reference"""
    x, off, _ = column_data(c)
    ordered = stable_sort(x) if c.rearrange else x
    pairs = ((0, c.Q - 1),)
    if c.caller.startswith("seasonal"):
        o = SR.origins_of(T0, c.count) if c.caller == "seasonal_store" else origins_of(c)      # the store: t_dev[0] + b
        return SR.apply_np(ordered, off, o, pairs, SEASON), ordered
    return CR.apply_np(ordered, off, pairs, True, False), ordered


def store_ref(c, rows):
    """the stemgnn_forecast_store contract: slab row pos + b takes batch row b where 0 <= pos + b < capacity, the rest keep the fill"""
    _, _, target = column_data(c)
    slab = np.full((c.capacity, c.Q, c.H, c.N), FILL, F32)
    tslab = np.full((c.capacity, c.H, c.N), FILL, F32)
    for b in range(c.count):
        if 0 <= c.pos + b < c.capacity:
            slab[c.pos + b], tslab[c.pos + b] = rows[b], target[b]
    return slab, tslab


def same_rows(got, want, ordered, paired):
    """applied rows: NaN in the same places, the same bits wherever the reference holds a number (a NaN that inf - inf makes only has
    to be a NaN), and the rows in no pair bit for bit what stage a selected"""
    if got.shape != want.shape or got.dtype != want.dtype or not same_nan_aware(got, want):
        return False
    free = [q for q in range(got.shape[1]) if q not in paired]
    return same_bits(got[:, free], ordered[:, free])


# ---- the references' own checks -----------------------------------------------------------------------------------------------------
def test_inputs_hold_the_edges_they_claim():
    for c in (FIT_CASES[2], SFIT_CASES[0]):
        y, f = fit_data(c)
        assert 0.07 < np.isnan(y).mean() < 0.17 and np.isnan(y[:, c.H - 1, c.N // 2]).all()
        assert np.isnan(f[~np.isnan(y)[:, None].repeat(c.Q, 1)]).any()  # NaN forecasts on valid targets
        assert np.isinf(y).any() and ((y == 0) & np.signbit(y)).any() and len(np.unique(y[np.isfinite(y)])) < 80
        off, cnt = fit_ref(c, True)
        assert np.isposinf(off[..., -1, :, :]).all() and (cnt[..., 0, c.H - 1, c.N // 2] == 0).all()       # rank beyond the size; no valid target
        assert np.isfinite(off[..., 0, :, :]).any()
        off_u, cnt_u = fit_ref(c, False)
        assert (cnt_u >= cnt).all() and (cnt_u > cnt).any()
    x, off, _ = column_data(COLUMN_CASES[5])
    moved = (x.view(np.uint32) != stable_sort(x).view(np.uint32)).any(axis=1).mean()
    assert moved >= 0.5 and all((x.view(np.uint32) == v).any() for v in POOL.view(np.uint32))
    s = stable_sort(np.array([np.nan, np.inf, -0.0, 0.0, -1.0, 0.0], F32).reshape(1, 6, 1, 1)).reshape(-1)
    assert s.view(np.uint32).tolist() == np.array([-1.0, -0.0, 0.0, 0.0, np.inf, np.nan], F32).view(np.uint32).tolist()
    two = np.array([0xffc00001, 0x7fc01234, 0x7f800000], np.uint32).view(F32).reshape(1, 3, 1, 1)
    assert stable_sort(two).view(np.uint32).reshape(-1).tolist() == [0x7f800000, 0xffc00001, 0x7fc01234]  # NaNs keep their row order
    assert len(_empty_buckets(SFIT_CASES[6])) > 0 and not _empty_buckets(SFIT_CASES[0])


def test_seasonal_twins_share_rows_and_origins():
    for c in SFIT_CASES:
        if c.origin == "consecutive":
            t = sfit_twin(c)
            assert np.array_equal(sfit_origins(c), sfit_origins(t)) and same_bits(fit_data(c)[0], fit_data(t)[0])
            a, b = fit_ref(c, True), fit_ref(t, True)
            assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- sensitivity: what a class adds must change the expected outputs ----------------------------------------------------------------
def _fit_rows(c, p):
    """[count, H, N]: the matrix row (column form) or the element index within its group (stream form) of every target"""
    i, h, n = np.meshgrid(np.arange(c.count), np.arange(c.H), np.arange(c.N), indexing="ij")
    if _cols(p):
        return i * p["Hr"] + (0 if c.per_step else h)
    return i * p["L"] + (h * c.N + n) % p["L"]


def _fit_without(name, c, p):
    r = _fit_rows(c, p)
    step = (p["threads"] // 64) * p["rpw_full"] if _cols(p) else p["threads"]
    if "trips" in name:                                                 # the rows beyond the first trip of every chunk
        return r % p["per_chunk"] >= step
    return r >= p["per_chunk"]                                          # the rows of the chunks above 0


FIT_SENSITIVE = ["fit columns/chunks set by the rows", "fit columns/chunks set by the blocks wanted",
                 "fit columns/two or more row trips inside a chunk", "fit stream/chunks set by the elements",
                 "fit stream/chunks set by the blocks wanted", "fit stream/two or more trips of thread 0"]


@pytest.mark.parametrize("name", FIT_SENSITIVE)
def test_further_chunks_and_trips_matter(lib, name):
    """with the target rows of the class's further chunks (or trips) absent, the reference gives other offsets and counts"""
    hit = reached(name)
    assert hit
    for c in hit:
        p = plan("fit", c)
        without = _fit_without(name, c, p)
        y, _ = fit_data(c)
        assert without.shape == y.shape and without.any() and not without.all() and (~np.isnan(y[without])).any(), c
        full, part = fit_ref(c, True), fit_ref(c, True, y=np.where(without, F32(np.nan), y))
        assert differ(full[0], part[0]) and not np.array_equal(full[1], part[1]), c


def _fit_outputs_without(name, c, p):
    g = np.arange(p["groups"]).reshape((c.H if c.per_step else 1), -1)
    return "offsets", np.broadcast_to(g >= (p["tiles"] - 1) * p["tile"], (c.P,) + g.shape)


def _apply_outputs_without(name, c, p):
    e = np.arange(c.count * c.Q * c.H * c.N).reshape(c.count, c.Q, c.H, c.N)
    if c.__class__ is Apply:
        return "out", e // p["vec"] >= p["grid_x"] * p["threads"]
    i, q, h, n = np.meshgrid(np.arange(c.count), np.arange(c.Q), np.arange(c.H), np.arange(c.N), indexing="ij")
    if "lane trips" in name:
        return "out", q * (c.N // p["vec"]) + n // p["vec"] >= 64
    return "out", i * c.H + h >= p["grid_x"] * (p["threads"] // 64)


def _column_outputs_without(name, c, p):
    i, q, h, n = np.meshgrid(np.arange(c.count), np.arange(c.Q), np.arange(c.H), np.arange(c.N), indexing="ij")
    if "column block" in name:
        return "out", h * c.N + n >= (p["col_blocks"] - 1) * p["cpb"] * p["vec"]
    if "target workgroups" in name:
        b = np.arange(c.capacity) - c.pos                                # the batch row a slab row takes
        return "out_target", np.broadcast_to(((b >= p["grid_x"]) & (b < c.count)).reshape(-1, 1, 1), (c.capacity, c.H, c.N))
    return "out", i >= (2 if "third" in name else 1) * p["win_blocks"] * p["wpb"]


OUTPUT_SENSITIVE = {
    "fit columns/several tiles, ragged last": _fit_outputs_without, "fit columns/a last tile of one column": _fit_outputs_without,
    "column/two or more column blocks, ragged last": _column_outputs_without, "column/a last column block of one column": _column_outputs_without,
    "column/a last column block of one float4": _column_outputs_without,
    "column/win_blocks capped, a second window trip": _column_outputs_without, "column/win_blocks capped, a third window trip": _column_outputs_without,
    "column/store, more windows than target workgroups": _column_outputs_without,
    "seasonal_apply/three or more lane trips over a segment": _apply_outputs_without,
}
OUTPUT_SENSITIVE.update({k: _apply_outputs_without for k in CLASSES if "a second trip of" in k})


def before_and_after(entry, c):
    """(what the outputs hold before the call, what the reference says they hold after it)"""
    if entry == "fit":
        off, _ = fit_ref(c, True)
        return dict(offsets=np.full(off.shape, np.nan, F32)), dict(offsets=off)
    if entry in ("apply", "seasonal_apply"):
        f, _ = apply_data(c)
        return dict(out=f if c.in_place else np.full(f.shape, np.nan, F32)), dict(out=apply_ref(c))
    x, _, _ = column_data(c)
    rows, _ = column_ref(c)
    if _is_store(c):
        slab, tslab = store_ref(c, rows)
        return dict(out=np.full(slab.shape, FILL), out_target=np.full(tslab.shape, FILL)), dict(out=slab, out_target=tslab)
    return dict(out=x if c.caller == "finish_in_place" else np.full(x.shape, np.nan, F32)), dict(out=rows)


@pytest.mark.parametrize("name", list(OUTPUT_SENSITIVE))
def test_further_tiles_blocks_and_trips_matter(lib, name):
    """leaving the outputs of the class's last tile / column block / further trips as they were gives other expected outputs"""
    entry, _ = CLASSES[name]
    hit = reached(name)
    assert hit
    for c in hit:
        p = plan(entry, c)
        before, full = before_and_after(entry, c)
        key, mask = OUTPUT_SENSITIVE[name](name, c, p)
        assert mask.shape == full[key].shape and mask.any(), (c, key)   # (a store may drop every row of the first trip: all)
        assert not mask.all() or (entry == "column" and _is_store(c)), (c, key)
        assert differ(np.where(mask, before[key], full[key]), full[key]), (c, key)


def test_every_further_share_class_has_its_sensitivity_check():
    words = ("trip", "tiles", "last tile", "chunks set", "column block", "target workgroups")
    named = {k for k in CLASSES if any(w in k for w in words) and "one chunk" not in k}
    assert named <= set(FIT_SENSITIVE) | set(OUTPUT_SENSITIVE), sorted(named - set(FIT_SENSITIVE) - set(OUTPUT_SENSITIVE))


def test_comparisons_fail_on_one_wrong_element():
    c = COLUMN_CASES[5]
    rows, ordered = column_ref(c)
    paired = (0, c.Q - 1)
    assert same_rows(rows.copy(), rows, ordered, paired)
    for q, v in ((0, None), (2, None), (2, F32(np.nan))):
        k = int(np.flatnonzero(np.isfinite(rows[:, q]).reshape(-1))[2])
        wrong = rows.copy()
        flat = wrong[:, q].reshape(-1).copy()
        flat[k] = np.nextafter(flat[k], F32(99)) if v is None else v
        wrong[:, q] = flat.reshape(wrong[:, q].shape)
        assert not same_rows(wrong, rows, ordered, paired), q
    other = rows.copy()
    nan_at = np.flatnonzero(np.isnan(other[:, 2]).reshape(-1))
    flat = other[:, 2].reshape(-1).copy()
    flat.view(np.uint32)[nan_at[0]] = 0x7fc00001                         # a row in no pair keeps its NaN payload
    other[:, 2] = flat.reshape(other[:, 2].shape)
    assert not same_rows(other, rows, ordered, paired)


# ---- refusals, host only: fake pointers, nothing is launched ------------------------------------------------------------------------
PTR = 4096


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def doubles(*v):
    return (ctypes.c_double * len(v))(*v)


FIT_OK = dict(target=PTR, forecast=PTR, count=70, Q=5, H=3, N=11, P=2, lo=ints(0, 1), hi=ints(4, 3), cov=doubles(0.8, 0.4),
              per_step=1, per_node=0, masked=0, scratch=PTR, offsets=PTR, counts=PTR)
APPLY_OK = dict(forecast=PTR, offsets=PTR, count=70, Q=5, H=3, N=11, P=2, lo=ints(0, 1), hi=ints(4, 3), per_step=1, per_node=0, out=PTR)
SAPPLY_OK = dict(forecast=PTR, offsets=PTR, origins=None, origin0=7, count=70, Q=5, H=3, N=11, rearrange=0, P=2, lo=ints(0, 1),
                 hi=ints(4, 3), per_step=1, per_node=0, period=288, K=24, phase=100, out=PTR)
SSTORE_OK = dict(steps=PTR, target=PTR, pos=PTR, t_dev=PTR, B=4, Q=5, H=3, N=11, rearrange=1, offsets=PTR, P=2, lo=ints(0, 1),
                 hi=ints(4, 3), per_step=1, per_node=0, period=288, K=24, phase=100, out_forecast=PTR, out_target=PTR, capacity=9)
FINISH_OK = dict(forecast=PTR, count=70, Q=5, H=3, N=11, rearrange=1, offsets=None, P=0, lo=None, hi=None, per_step=1, per_node=0, out=PTR)
STORE_OK = dict(steps=PTR, target=PTR, pos=PTR, B=7, Q=5, H=3, N=11, rearrange=1, offsets=None, P=0, lo=None, hi=None, per_step=1,
                per_node=0, out_forecast=PTR, out_target=PTR, capacity=9)


def _refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == EINVAL


def test_entries_refuse_what_the_abi_files_leave(lib):
    one = dict(P=1, lo=ints(0), hi=ints(4))
    # the unseasoned fit: P G >= 2^29 (the pick's int indices) and G > 65535 in the stream form (grid.y), every factor being fine
    assert _refused(lib.stemgnn_conformal_fit, FIT_OK, count=1, H=2 ** 10, N=2 ** 19, per_step=1, per_node=1, cov=doubles(0.8), **one)
    assert _refused(lib.stemgnn_conformal_fit, FIT_OK, count=2, H=65536, N=1, per_step=1, per_node=0)
    assert lib.stemgnn_conformal_scratch_bytes(2, 65535, 1, 2, 1, 0) == 2 * 65535 * 258 * 4
    # H N >= 2^31 on its own (count = 1), and a count beyond a long's 32 bits, for the applies and the seasonal store
    for f, ok, count in ((lib.stemgnn_conformal_apply, APPLY_OK, "count"), (lib.stemgnn_seasonal_apply, SAPPLY_OK, "count"),
                         (lib.stemgnn_seasonal_apply, dict(SAPPLY_OK, rearrange=1), "count"),
                         (lib.stemgnn_quantile_store_seasonal, SSTORE_OK, "B")):
        assert _refused(f, ok, **{count: 1}, H=2 ** 16, N=2 ** 15), f.__name__
        assert _refused(f, ok, **{count: 2 ** 31 // 33 + 1}), f.__name__
    assert _refused(lib.stemgnn_conformal_apply, APPLY_OK, count=2 ** 40) and _refused(lib.stemgnn_seasonal_apply, SAPPLY_OK, count=2 ** 40)
    # the epilogue without offsets: Q > 32, and pairs are not looked at
    for f, ok in ((lib.stemgnn_quantile_finish, FINISH_OK), (lib.stemgnn_quantile_store, STORE_OK)):
        assert _refused(f, ok, Q=33) and _refused(f, ok, Q=0) and _refused(f, ok, N=-1), f.__name__
        assert _refused(f, ok, offsets=PTR, P=2, lo=None, hi=ints(4, 3)) and _refused(f, ok, offsets=PTR, P=2, lo=ints(0, 1), hi=None)


SHAPES_OK = {"fit": (70, 3, 11, 2, 1, 0), "seasonal_fit": (70, 3, 11, 2, 1, 0, 288, 24, 0), "apply": (70, 5, 3, 12),
             "seasonal_apply": (70, 5, 3, 12), "column": (70, 5, 3, 12, 1, 0)}


def _plan_rc(lib, entry, shape, mis=0, out=True, nshape=None):
    from stemgnn_amd import _lib

    buf = (ctypes.c_int * _lib.SG_CALIBRATION_PLAN_WORDS)()
    arr = (ctypes.c_long * max(1, len(shape)))(*shape)
    rc = lib.stemgnn_calibration_plan(entry, arr, len(shape) if nshape is None else nshape, mis, buf if out else None)
    return rc, list(buf)


def test_plan_refusals(lib):
    from stemgnn_amd import _lib

    E = _lib.SG_CALIBRATION_ENTRY
    assert set(SHAPES_OK) == set(E) and _lib.SG_CALIBRATION_NSHAPE == {k: len(v) for k, v in SHAPES_OK.items()}
    for entry, shape in SHAPES_OK.items():
        rc, w = _plan_rc(lib, E[entry], shape)
        assert rc == 0 and w[4] in (64, 128, 192, 256) and w[6] == lib.stemgnn_num_cus(), entry
        assert _plan_rc(lib, E[entry], shape, out=False)[0] == EINVAL
        assert _plan_rc(lib, E[entry], shape + (0,))[0] == EINVAL and _plan_rc(lib, E[entry], shape[:-1])[0] == EINVAL
        assert _plan_rc(lib, E[entry], shape, mis=-1)[0] == EINVAL
        for i in range(4):                                              # a zero or a negative size
            for v in (0, -1):
                assert _plan_rc(lib, E[entry], shape[:i] + (v,) + shape[i + 1:])[0] == EINVAL, (entry, i, v)
        assert _plan_rc(lib, E[entry], (2 ** 40,) + shape[1:])[0] == EINVAL, entry
    assert lib.stemgnn_calibration_plan(E["fit"], None, 6, 0, (ctypes.c_int * 32)()) == EINVAL
    for entry in (-1, len(E), 1 << 20):
        assert _plan_rc(lib, entry, SHAPES_OK["fit"])[0] == EINVAL
    # a bit that names no buffer of the entry
    for entry, first_bad in (("fit", 1), ("seasonal_fit", 1), ("apply", 4), ("seasonal_apply", 4), ("column", 4)):
        assert _plan_rc(lib, E[entry], SHAPES_OK[entry], mis=first_bad)[0] == EINVAL, entry
        for m in range(first_bad):
            rc, w = _plan_rc(lib, E[entry], SHAPES_OK[entry], mis=m)
            assert rc == 0 and (w[5] == 4) == (m == 0 and "fit" not in entry), (entry, m)
    store = SHAPES_OK["column"][:5] + (1,)
    assert _plan_rc(lib, E["column"], store, mis=16)[0] == EINVAL
    for m in range(16):
        rc, w = _plan_rc(lib, E["column"], store, mis=m)
        assert rc == 0 and (w[5] == 4) == (m & 3 == 0) and (w[17] == 4) == (m & 12 == 0) and w[2] == 2, m
    # the shapes the entries themselves refuse
    bad = {"fit": [(70, 3, 11, 17, 1, 0), (2 ** 31 // 33 + 1, 3, 11, 2, 1, 0), (1, 2 ** 10, 2 ** 19, 1, 1, 1), (2, 65536, 1, 2, 1, 0)],
           "seasonal_fit": [(70, 3, 11, 2, 1, 0, 0, 24, 0), (70, 3, 11, 2, 1, 0, 2 ** 31, 24, 0), (70, 3, 11, 2, 1, 0, 288, 0, 0),
                            (70, 3, 11, 2, 1, 0, 288, 289, 0), (70, 3, 11, 2, 1, 0, 2 ** 20, 32768, 0), (70, 3, 11, 2, 1, 0, -288, 24, 0),
                            (1, 300, 1000, 1, 1, 1, 4096, 2048, 0), (2, 65536, 1, 1, 1, 0, 288, 1, 0)],
           "apply": [(70, 33, 3, 12), (2 ** 31 // 36 + 1, 5, 3, 12), (1, 5, 2 ** 16, 2 ** 15)],
           "seasonal_apply": [(70, 33, 3, 12), (2 ** 31 // 36 + 1, 5, 3, 12), (1, 5, 2 ** 16, 2 ** 15)],
           "column": [(70, 33, 3, 12, 1, 0), (1, 5, 2 ** 16, 2 ** 15, 1, 0), (2 ** 31, 5, 3, 12, 1, 1)]}
    assert set(bad) == set(E)
    for entry, shapes in bad.items():
        for s in shapes:
            assert _plan_rc(lib, E[entry], s)[0] == EINVAL, (entry, s)
    assert _plan_rc(lib, E["fit"], (2, 65535, 1, 2, 1, 0))[0] == 0 and _plan_rc(lib, E["column"], (70, 32, 3, 12, 1, 0))[0] == 0
    assert _plan_rc(lib, E["seasonal_fit"], (70, 3, 11, 1, 1, 0, 2 ** 31 - 1, 65535, 1))[0] == 0
