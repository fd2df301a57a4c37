"""CPU: the case lists of tests/test_hip_data_stage.py (the data stage, stemgnn_amd/csrc/data.hip; cases and references in
tests/helpers/data_ref.py), and proof that they reach what they claim.

stemgnn_data_plan reports, host only, what each launcher of data.hip does for a shape: the grid, the threads per workgroup, float4
or scalar copies, the queue gather's slab rows per workgroup, the MSE form, the grid-stride passes and the metric entries' row
chunks.  The launchers take their geometry from the same static functions, so every class below is decided by what the plan says,
none by a threshold copied into this file: a threshold that moves fails here instead of silently dropping an edge from the device
suite.  CLASSES names every launch decision and input edge the suite must reach; test_class_is_reached is parametrised over it, so
taking the cases of any one class out of the lists fails that class's test.

The file also holds the host-only argument checks (fake pointers: every call is refused before anything is launched), the size
functions against the layouts the references assume, and the comparison helpers of the device suite handed wrong results -- they
stand in for mutation runs on the device."""
import ctypes
import os

import numpy as np
import pytest

from tests.helpers import data_ref as R

EINVAL = -10001


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def plan(entry, case):
    from stemgnn_amd import _lib

    return _lib.data_plan(entry, *R.plan_args(entry, case))


def _thr(entry):
    """the thread classes of an entry, found by asking the plan over N = 1 .. 2048 (smallest first)"""
    from stemgnn_amd import _lib

    shape = {"gather": lambda N: (3, 5, 2, N), "gather_queue": lambda N: (3, 5, 2, N), "roll": lambda N: (2, 5, 2, N),
             "roll_quantile": lambda N: (2, 5, 2, N, 3)}[entry]
    return sorted({_lib.data_plan(entry, *shape(N))["threads"] for N in range(1, 2049)})


def _q(case):
    return R.QUEUE_CASES[case]


def _take(c):                                                           # (B, W, L, N, step, horizon, ...)
    return min(c[5] - c[4], c[2])


# class name -> (entry, predicate(case, plan)); `lambda c, p, k=k` binds the loop value
CLASSES = {
    "normalize/one pass": ("normalize", lambda c, p: p["passes"] == 1),
    "normalize/two passes, N not dividing the stride": ("normalize", lambda c, p: p["passes"] == 2 and (p["grid_x"] * p["threads"]) % c[1] != 0),
    "normalize/clip01 off": ("normalize", lambda c, p: c[2] == 0),
    "normalize/clip01 on": ("normalize", lambda c, p: c[2] == 1),
    "normalize/N = 1": ("normalize", lambda c, p: c[1] == 1),
    "normalize/two passes with clip01": ("normalize", lambda c, p: p["passes"] == 2 and c[2] == 1),
    "gather/H = 0": ("gather", lambda c, p: c[1] == 0 and p["grid_x"] == R.GATHER_W),
    "gather/H > 0": ("gather", lambda c, p: c[1] > 0),
    "gather/all rows good": ("gather", lambda c, p: not R.gather_ref(*R.series_pair(R.GATHER_T, c[0]), c[2], R.GATHER_W, c[1])[3]),
    "gather/H = 0, a window ending at T": ("gather", lambda c, p: c[1] == 0 and R.GATHER_T in c[2]),
    "gather_queue/rows_per_wg = 1": ("gather_queue", lambda c, p: p["rows_per_wg"] == 1 and p["grid_x"] == _q(c)["W"] + _q(c)["H"] > 1),
    "gather_queue/ragged last row group": ("gather_queue", lambda c, p: p["rows_per_wg"] > 1 and (_q(c)["W"] + _q(c)["H"]) % p["rows_per_wg"] != 0),
    "gather_queue/rows_per_wg = W + H, grid.x = 1": ("gather_queue", lambda c, p: p["grid_x"] == 1 and p["grid_y"] >= 64 and p["rows_per_wg"] > 1),
    "gather_queue/one workgroup": ("gather_queue", lambda c, p: p["grid_x"] * p["grid_y"] == 1),
    "gather_queue/one workgroup, wrap": ("gather_queue", lambda c, p: p["grid_x"] * p["grid_y"] == 1 and _q(c)["wrap"]),
    "gather_queue/walk past the end, ragged batch": ("gather_queue", lambda c, p: not _q(c)["wrap"] and _q(c)["count"] % _q(c)["B"] != 0
                                                     and _q(c)["calls"] == -(-_q(c)["count"] // _q(c)["B"]) + 1 and _q(c)["B"] > 1),
    "gather_queue/wrap": ("gather_queue", lambda c, p: _q(c)["wrap"] and _q(c)["B"] > 1 and _q(c)["calls"] >= 4),
    "gather_queue/bad window inside order": ("gather_queue", lambda c, p: any(0 < i < _q(c)["B"] - 1 for i in _q(c)["bad"])),
    "gather_queue/negative start": ("gather_queue", lambda c, p: _q(c)["start"] < 0),
    "gather_queue/pair, float4": ("gather_queue", lambda c, p: _q(c)["pair"] and p["vec"] == 1),
    "gather_queue/pair, scalar": ("gather_queue", lambda c, p: _q(c)["pair"] and p["vec"] == 0),
    "mse_fwd/n = 1": ("mse_fwd", lambda c, p: c == 1),
    "mse_fwd/one workgroup, one pass, ragged": ("mse_fwd", lambda c, p: p["form"] == 0 and p["passes"] == 1 and c == p["threads"] - 1),
    "mse_fwd/one workgroup, second pass of one element": ("mse_fwd", lambda c, p: p["form"] == 0 and c == p["threads"] + 1),
    "mse_fwd/largest one-workgroup size": ("mse_fwd", lambda c, p: p["form"] == 0 and _form("mse_fwd", c + 1) == 1),
    "mse_fwd/smallest two-stage size": ("mse_fwd", lambda c, p: p["form"] == 1 and _form("mse_fwd", c - 1) == 0),
    "mse_fwd/two-stage, ragged last pass": ("mse_fwd", lambda c, p: p["form"] == 1 and p["passes"] > 1 and c % (p["grid_x"] * p["threads"]) not in (0, 1)),
    "mse_bwd/n = 1": ("mse_bwd", lambda c, p: c == 1),
    "mse_bwd/one pass, several workgroups": ("mse_bwd", lambda c, p: p["passes"] == 1 and p["grid_x"] > 1),
    "mse_bwd/two passes": ("mse_bwd", lambda c, p: p["passes"] == 2 and c % (p["grid_x"] * p["threads"]) != 0),
    "forecast_store/H N below one workgroup": ("forecast_store", lambda c, p: c[0] * c[1] < p["threads"] and p["grid_x"] == 1),
    "forecast_store/H N one above a workgroup": ("forecast_store", lambda c, p: c[0] * c[1] == p["threads"] + 1 and p["grid_x"] == 2),
    "forecast_store/two passes": ("forecast_store", lambda c, p: p["passes"] == 2 and c[0] * c[1] % (p["grid_x"] * p["threads"]) != 0),
}
for _e in ("gather", "gather_queue"):
    for _t in (64, 128, 256):
        for _v in (0, 1):
            CLASSES[f"{_e}/{_t} threads, {'float4' if _v else 'scalar'}"] = (_e, lambda c, p, t=_t, v=_v: (p["threads"], p["vec"]) == (t, v))
for _N in (1, 7, 8, 255, 256, 257, 1023, 1024, 1027):
    CLASSES[f"gather/N = {_N}"] = ("gather", lambda c, p, N=_N: c[0] == N)
for _N in (127, 128, 511, 512):
    CLASSES[f"gather_queue/N = {_N}"] = ("gather_queue", lambda c, p, N=_N: _q(c)["N"] == N)
for _v in (0, 1):
    for _y in (0, 2):
        CLASSES[f"gather/good and bad rows mixed, {'float4' if _v else 'scalar'}, H = {_y}"] = (
            "gather", lambda c, p, v=_v, y=_y: p["vec"] == v and c[1] == y and
            0 < len(R.gather_ref(*R.series_pair(R.GATHER_T, c[0]), c[2], R.GATHER_W, c[1])[3]) < len(c[2]))
for _name, _f in (("window before the start", lambda c: any(0 <= e < R.GATHER_W for e in c[2])), ("negative row", lambda c: any(e < 0 for e in c[2])),
                  ("window past the end", lambda c: any(e + c[1] > R.GATHER_T for e in c[2]))):
    CLASSES[f"gather/{_name}"] = ("gather", lambda c, p, f=_f: f(c))
for _e in ("roll", "roll_quantile"):
    CLASSES.update({
        f"{_e}/L = 1": (_e, lambda c, p: c[2] == 1 < c[1]),
        f"{_e}/1 < L < W": (_e, lambda c, p: 1 < c[2] < c[1]),
        f"{_e}/L = W": (_e, lambda c, p: c[2] == c[1] > 1),
        f"{_e}/64 threads": (_e, lambda c, p: p["threads"] == 64),
        f"{_e}/256 threads": (_e, lambda c, p: p["threads"] == 256 and c[3] % 256 != 0),
        f"{_e}/take = L": (_e, lambda c, p: _take(c) == c[2]),
        f"{_e}/take < L": (_e, lambda c, p: _take(c) < c[2]),
        f"{_e}/step = 0": (_e, lambda c, p: c[4] == 0),
        f"{_e}/step > 0": (_e, lambda c, p: c[4] > 0),
        f"{_e}/rows of forecast_steps on both sides stay": (_e, lambda c, p: c[4] > 0 and c[4] + _take(c) < c[5]),
    })
CLASSES["roll/rows of forecast_steps on both sides stay"] = ("roll", lambda c, p: c[4] + _take(c) < c[5])    # after them: (2, 5, 2, 300, 0, 4)
CLASSES["roll_quantile/rows of forecast_steps on both sides stay"] = ("roll_quantile", lambda c, p: c[4] + _take(c) < c[5])
CLASSES["roll_quantile/Q = 1"] = ("roll_quantile", lambda c, p: c[6] == 1 and p["grid_x"] == c[1] + c[2])
for _name, _f in (("first", lambda c: c[7] == 0), ("middle", lambda c: 0 < c[7] < c[6] - 1), ("last", lambda c: c[7] == c[6] - 1)):
    CLASSES[f"roll_quantile/Q = 3, point {_name}"] = ("roll_quantile", lambda c, p, f=_f: c[6] == 3 and p["grid_x"] == c[1] + 3 * c[2] and f(c))
for _pos, _name in ((0, "0"), (R.STORE_CAPACITY - R.STORE_B, "capacity - B"), (R.STORE_CAPACITY - 1, "capacity - 1"), (-1, "-1"),
                    (-R.STORE_B, "-B"), (R.STORE_CAPACITY, "capacity")):
    for _hn in ("below", "two passes"):
        CLASSES[f"forecast_store/pos = {_name}, {_hn}"] = (
            "forecast_store", lambda c, p, pos=_pos, two=_hn == "two passes": c[2] == pos and (p["passes"] == 2) == two)
for _m in (0, 1):
    _form_name = "masked" if _m else "plain"
    for _cnt in R.EVAL_COUNTS:
        CLASSES[f"eval {_form_name}/count = {_cnt}"] = ("eval", lambda c, p, m=_m, n=_cnt: c[3] == m and c[0] == n and p["nchunk"] == -(-n // 64))
    for _H, _N in R.EVAL_SHAPES:
        CLASSES[f"eval {_form_name}/(H, N) = ({_H}, {_N})"] = ("eval", lambda c, p, m=_m, H=_H, N=_N: c[3] == m and c[1:3] == (H, N))
    for _d in (0, 1):
        CLASSES[f"eval {_form_name}/{'with' if _d else 'without'} mul, add"] = ("eval", lambda c, p, m=_m, d=_d: c[3:5] == (m, d))
    CLASSES[f"eval {_form_name}/two column workgroups and three chunks"] = ("eval", lambda c, p, m=_m: c[3] == m and p["grid_x"] == 2 and p["nchunk"] == 3)
    CLASSES[f"eval {_form_name}/N beyond the epilogue's threads"] = ("eval", lambda c, p, m=_m: c[3] == m and c[2] > p["threads"])
    CLASSES[f"eval {_form_name}/H beyond the epilogue's threads"] = ("eval", lambda c, p, m=_m: c[3] == m and c[1] > p["threads"])
    for _Q in (1, 2, 3, 32):
        CLASSES[f"quantile {_form_name}/Q = {_Q}"] = ("quantile_metrics", lambda c, p, m=_m, Q=_Q: c[4] == m and c[1] == Q and p["grid_z"] == Q + Q // 2 + 1)
    for _cnt in (1, 65):
        CLASSES[f"quantile {_form_name}/count = {_cnt}"] = ("quantile_metrics", lambda c, p, m=_m, n=_cnt: c[4] == m and c[0] == n and p["nchunk"] == -(-n // 64))
    for _H, _N in ((1, 1), (3, 86)):
        CLASSES[f"quantile {_form_name}/(H, N) = ({_H}, {_N})"] = ("quantile_metrics", lambda c, p, m=_m, H=_H, N=_N: c[4] == m and c[2:4] == (H, N))
    CLASSES[f"quantile {_form_name}/Q = 32, two chunks, two column workgroups"] = (
        "quantile_metrics", lambda c, p, m=_m: c[4] == m and c[1] == 32 and p["nchunk"] == 2 and p["grid_x"] == 2)
    for _d in (0, 1):
        CLASSES[f"quantile {_form_name}/{'with' if _d else 'without'} mul, add"] = ("quantile_metrics", lambda c, p, m=_m, d=_d: c[4:6] == (m, d))


def _form(entry, n):
    from stemgnn_amd import _lib

    return _lib.data_plan(entry, n)["form"]


def reached(name, cases=None):
    entry, pred = CLASSES[name]
    return [c for c in (R.CASES[entry] if cases is None else cases) if pred(c, plan(entry, c))]


@pytest.mark.parametrize("name", list(CLASSES))
def test_class_is_reached(lib, name):
    """at least one case of the entry's list is in the class, according to stemgnn_data_plan; without those cases none is"""
    hit = reached(name)
    assert hit, f"no case of {CLASSES[name][0]} reaches `{name}`"
    rest = [c for c in R.CASES[CLASSES[name][0]] if c not in hit]
    assert not reached(name, rest)


def test_lists_are_small_distinct_and_cover_every_entry(lib):
    from stemgnn_amd import _lib

    assert set(R.CASES) == set(_lib.SG_DATA_ENTRY) == {CLASSES[k][0] for k in CLASSES}
    for entry, cases in R.CASES.items():
        assert len(set(cases)) == len(cases) <= 24, entry
    assert max(T * N for T, N, _ in R.NORMALIZE_CASES) * 8 < 8.5e6          # the largest input of the suite: 8.4 MB of fp64
    assert max(R.MSE_FWD_CASES + R.MSE_BWD_CASES) < 300000
    assert max(c * Q * H * N for c, Q, H, N, _, _ in R.QUANTILE_CASES) < 600000


def test_thread_classes_are_the_ones_the_tables_name(lib):
    """the thresholds themselves, found by asking: every N at which an entry's thread count changes has a case on either side"""
    from stemgnn_amd import _lib

    assert _thr("gather") == [64, 128, 256] == _thr("gather_queue") and _thr("roll") == [64, 256] == _thr("roll_quantile")
    for entry, shape, have in (("gather", lambda N: (3, 5, 2, N), {c[0] for c in R.GATHER_CASES}),
                               ("gather_queue", lambda N: (3, 5, 2, N), {c["N"] for c in R.QUEUE_CASES.values()}),
                               ("roll", lambda N: (2, 5, 2, N), {c[3] for c in R.ROLL_CASES})):
        t = [_lib.data_plan(entry, *shape(N))["threads"] for N in range(1, 2049)]
        edges = [N for N in range(2, 2049) if t[N - 1] != t[N - 2]]       # the first N of a new class
        for N in edges:
            assert any(n >= N and t[n - 1] == t[N - 1] for n in have) and any(n < N and t[n - 1] == t[N - 2] for n in have), (entry, N)
        if entry != "roll":
            assert all(N in have and N - 1 in have for N in edges), (entry, edges)
    # the MSE switch and the pass counts, likewise
    n0 = next(n for n in range(65000, 66000) if _form("mse_fwd", n) == 1)
    assert {n0 - 1, n0} <= set(R.MSE_FWD_CASES)
    p = _lib.data_plan("normalize", 1 << 20, 1)
    assert p["passes"] == 1 and _lib.data_plan("normalize", (1 << 20) + 1, 1)["passes"] == 2 and p["grid_x"] * p["threads"] == 1 << 20
    p = _lib.data_plan("forecast_store", 1, 1, 1 << 14)
    assert p["passes"] == 1 and _lib.data_plan("forecast_store", 1, 1, (1 << 14) + 1)["passes"] == 2
    p = _lib.data_plan("mse_bwd", 1 << 18)
    assert p["passes"] == 1 and _lib.data_plan("mse_bwd", (1 << 18) + 1)["passes"] == 2
    assert [_lib.data_plan("eval", c, 1, 1)["nchunk"] for c in (1, 63, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]


def test_queue_model_walks_as_the_issue_states(lib):
    """count = 20, B = 8: the third call is ragged (rows 16 .. 19, then zeros, bit 1), the fourth is all zeros; with wrap the
    positions are 0, 8, 0, 8; a negative position gathers nothing"""
    sx, sy = R.series_pair(R.GATHER_T, 7)
    for name, positions in (("walk", [0, 8, 16, 24, 32]), ("wrap", [0, 8, 0, 8, 0])):
        c = R.QUEUE_CASES[name]
        m = R.QueueModel(R.queue_order(c), c["count"], c["wrap"], c["start"])
        for k in range(c["calls"]):
            assert m.q[0] == positions[k]
            x, y, status, zero = m.call(sx, sx, c["B"], c["W"], c["H"])
            want = ([4, 5, 6, 7], 2) if positions[k] == 16 else (list(range(8)), 2) if positions[k] == 24 else ([], 0)
            assert (zero, status) == want, (name, k)
            assert not x[zero].any() and not y[zero].any() and all(x[b].any() for b in range(8) if b not in zero)
        assert m.q == [positions[c["calls"]], 0, c["count"], c["wrap"]]
    c = R.QUEUE_CASES["bad_window"]
    m = R.QueueModel(R.queue_order(c), c["count"], 0)
    sx, _ = R.series_pair(R.GATHER_T, c["N"])
    assert [m.call(sx, sx, 3, 5, 2)[2:] for _ in range(2)] == [(1, [1]), (1, [1])]      # order[1] and order[4]: the middle row, bit 0
    c = R.QUEUE_CASES["negative_start"]
    m = R.QueueModel(R.queue_order(c), c["count"], 0, c["start"])
    sx, _ = R.series_pair(R.GATHER_T, c["N"])
    assert m.call(sx, sx, 3, 5, 2)[2:] == (2, [0, 1, 2]) and m.q[0] == 1 and m.call(sx, sx, 3, 5, 2)[2:] == (0, [])
    for c in R.QUEUE_CASES.values():                                               # every good window is inside the series
        assert all(c["W"] <= e <= R.GATHER_T - c["H"] for i, e in enumerate(R.queue_order(c)) if i not in c["bad"])


def test_inputs_hold_the_edges_they_claim():
    raw, sub, div = R.normalize_case(40, 7, 1)
    v = (raw - sub) / div
    assert np.isnan(v[0]).all() and np.isposinf(v[1]).all() and np.isneginf(v[2]).all()
    assert (v[3] == 0).all() and (v[4] == 1).all() and (v[5] < 0).all() and (v[6] > 1).all() and ((v[7] < 1) & (v[8] > 0)).all()
    assert np.signbit(v[10, 6]) and v[10, 6] == 0 and np.isinf(R.normalize_ref(raw, sub, div, 0)[9]).all()
    clipped = R.normalize_ref(raw, sub, div, 1)
    assert (clipped[5] == 0).all() and (clipped[6] == 1).all() and (clipped[2] == 0).all() and np.isnan(clipped[0]).all()
    assert R.normalize_ref(raw, sub, div, 0)[5].max() < 0                      # just beyond 0 survives without the clip
    for case in R.EVAL_CASES:
        t, f, mul, add = R.eval_case(*case)
        count, H, N, masked, denorm = case
        assert (mul is not None) == bool(denorm)
        h0, n0 = R.eval_zero_at(H, N)
        if count >= 63:
            assert t[5, h0, n0] == 0 and f[5, h0, n0] != 0 and not np.isnan(t[:5, h0, n0]).all()
        if count == 65:
            assert t[64, h0, n0] == 0 and f[64, h0, n0] == 0
        if masked and H > 1 and N > 1:
            assert np.isnan(t[:, H - 1]).all() and np.isnan(t[:, :, 0]).all() and np.isnan(t[:, 0, N - 1]).all()
            assert not np.isnan(t[:, 0, 1:N - 1]).all()
        if not masked:
            assert not np.isnan(t).any()
    t, f, _, _ = R.eval_case(65, 2, 300, 0, 0)
    m = R.plain_metrics_numpy(t, f)
    assert np.isnan(m["overall"][0]) and np.isfinite(m["overall"][1]) and np.isnan(m["by_node"][0][150]) and np.isfinite(np.delete(m["by_node"][0], 150)).all()
    t, f, _, _ = R.eval_case(64, 3, 86, 0, 0)
    assert R.plain_metrics_numpy(t, f)["by_step_node"][0][1, 43] > 5 / 64       # the clipped percentage error is in that mean
    for case in R.QUANTILE_CASES:
        C, Q, H, N, masked, denorm = case
        t, f, _, _ = R.quantile_case(*case)
        assert (t[:, None] == f).any(), case                                  # a tie
        if Q > 1 and C * H * N > 100:
            assert (np.diff(f, axis=1) < 0).any() and (np.diff(f, axis=1) == 0).any(), case
        if masked and H > 1:
            assert np.isnan(t[:, H - 1]).all()


def test_unmasked_reference_is_the_oracles_evaluate():
    from oracle import data_oracle as do

    t, f, _, _ = R.eval_case(64, 3, 86, 0, 0)
    m = R.masked_metrics_numpy(t, f)
    p = R.plain_metrics_numpy(t, f)
    for name, kw in (("overall", {}), ("by_node", dict(by_node=True)), ("by_step", dict(by_step=True)),
                     ("by_step_node", dict(by_step=True, by_node=True))):
        want = do.evaluate(t.astype(np.float64), f.astype(np.float64), **kw)
        for a, b, w in zip(m[name], p[name], want):
            np.testing.assert_allclose(a, w, rtol=1e-13, atol=0)
            np.testing.assert_allclose(b, w, rtol=1e-13, atol=0)


def test_size_functions_match_the_layouts_of_the_references(lib):
    from stemgnn_amd import _lib

    assert lib.stemgnn_mse_scratch_floats() == _lib.data_plan("mse_fwd", max(R.MSE_FWD_CASES))["grid_x"]      # one partial per workgroup
    for count, H, N, masked, denorm in R.EVAL_CASES:
        nchunk = plan("eval", (count, H, N))["nchunk"]
        t, f, mul, add = R.eval_case(count, H, N, masked, denorm)
        want, _ = R.eval_ref(t, f, mul, add, masked)
        assert lib.stemgnn_eval_out_doubles(H, N) == want.size == 3 * (1 + N + H + H * N)
        planes = 4 if masked else 3                                           # sums per chunk and column, their totals, node sums
        size = (lib.stemgnn_eval_scratch_doubles_masked if masked else lib.stemgnn_eval_scratch_doubles)(count, H, N)
        assert size == planes * (H * N * (nchunk + 1) + N)
    for case in R.QUANTILE_CASES:
        count, Q, H, N, masked, denorm = case
        nchunk = plan("quantile_metrics", case)["nchunk"]
        t, f, mul, add = R.quantile_case(*case)
        want, exact = R.quantile_ref(t, f, R.levels(Q), mul, add, masked)
        K = 2 * Q + 2 * (Q // 2) + 1
        assert lib.stemgnn_quantile_out_doubles(Q, H) == want.size == exact.size == K * (H + 1)
        assert lib.stemgnn_quantile_scratch_doubles(count, Q, H, N) == (K + 1) * (H * N * (nchunk + 1) + H)
        assert int(exact.sum()) == ((Q + Q // 2 + 1) * (H + 1) if count * N > 1 else exact.size)     # a single term: everything
    assert lib.stemgnn_eval_scratch_doubles(0, 3, 4) == 0 and lib.stemgnn_quantile_out_doubles(33, 2) == 0


def test_plan_and_grid_limit_refusals(lib):
    from stemgnn_amd import _lib

    out = (ctypes.c_int * _lib.SG_DATA_PLAN_WORDS)()
    E = _lib.SG_DATA_ENTRY
    assert lib.stemgnn_data_plan(E["gather"], 3, 5, 2, 7, 0, out) == 0 and list(out)[:4] == [7, 3, 1, 64]
    assert lib.stemgnn_data_plan(E["gather"], 3, 5, 2, 7, 0, None) == EINVAL
    assert lib.stemgnn_data_plan(E["gather"], 3, 5, 2, 7, -1 << 40, out) == 0 and lib.stemgnn_data_plan(E["mse_bwd"], 9, -1, 1 << 40, 0, -7, out) == 0
    assert lib.stemgnn_data_plan(E["forecast_store"], 4, 3, 7, 1 << 40, 1 << 40, out) == 0          # arguments an entry does not use
    for entry in (-1, len(E), 1 << 20):
        assert lib.stemgnn_data_plan(entry, 3, 5, 2, 7, 1, out) == EINVAL
    bad = {"normalize": [(0, 3), (5, 0), (-1, 3), (5, 1 << 31)],
           "gather": [(0, 5, 2, 7), (65536, 5, 2, 7), (3, 0, 2, 7), (3, 5, -1, 7), (3, 5, 2, 0), (1 << 32, 5, 2, 7)],
           "gather_queue": [(0, 5, 2, 7), (65536, 5, 2, 7), (3, 0, 2, 7), (3, 5, -1, 7), (3, 5, 2, 0)],
           "mse_fwd": [(0,), (-4,)], "mse_bwd": [(0,), (-4,)],
           "roll": [(0, 5, 2, 7), (65536, 5, 2, 7), (2, 5, 6, 7), (2, 5, 0, 7), (2, 0, 0, 7), (2, 5, 2, 0)],
           "roll_quantile": [(65536, 5, 2, 7, 3), (2, 5, 6, 7, 3), (2, 5, 2, 7, 0), (2, 5, 2, 0, 3)],
           "forecast_store": [(0, 3, 7), (65536, 3, 7), (4, 0, 7), (4, 3, 0), (4, 1 << 16, 1 << 16)],
           "eval": [(0, 3, 7), (5, 0, 7), (5, 3, 0), (64 * 65535 + 1, 3, 7)],
           "quantile_metrics": [(0, 3, 3, 7), (5, 0, 3, 7), (5, 33, 3, 7), (5, 3, 0, 7), (5, 3, 3, 0), (64 * 65535 + 1, 3, 3, 7)]}
    assert set(bad) == set(E)
    for entry, shapes in bad.items():
        for s in shapes:
            assert lib.stemgnn_data_plan(E[entry], *(list(s) + [0] * (5 - len(s))), out) == EINVAL, (entry, s)
    good = {"gather": (65535, 5, 0, 7), "gather_queue": (65535, 5, 2, 7), "roll": (65535, 5, 5, 7), "roll_quantile": (65535, 5, 2, 7, 32),
            "forecast_store": (65535, 3, 7), "eval": (64 * 65535, 3, 7)}
    for entry, s in good.items():
        assert _lib.data_plan(entry, *s)["grid_y"] == 65535, entry
    # the entries themselves, with fake non-NULL pointers (16-byte aligned): refused before anything is launched
    p = 4096
    for B, rc in ((65536, EINVAL), (1 << 20, EINVAL), (0, EINVAL), (-1, EINVAL)):
        assert lib.stemgnn_window_gather(p, p, p, p, B, 5, 2, 7, 40, None, None) == rc
        assert lib.stemgnn_window_gather_pair(p, p, p, p, p, B, 5, 2, 7, 40, None, None) == rc
        assert lib.stemgnn_window_gather_queue(p, p, p, p, p, B, 5, 2, 7, 40, None, None) == rc
        assert lib.stemgnn_window_gather_queue_pair(p, p, p, p, p, p, B, 5, 2, 7, 40, None, None) == rc
        assert lib.stemgnn_roll_window(p, p + 64, p + 128, p + 192, B, 5, 2, 7, 0, 3, None) == rc
        assert lib.stemgnn_roll_window_quantile(p, p + 64, p + 128, p + 192, B, 5, 2, 7, 3, 1, 0, 3, None) == rc
        assert lib.stemgnn_forecast_store(p, p, p, p, p, B, 3, 7, 10, None) == rc
    assert lib.stemgnn_forecast_store(p, p, p, p, p, 4, 3, 7, 0, None) == EINVAL                        # capacity
    assert lib.stemgnn_roll_window(p, p + 64, p + 128, p + 192, 2, 5, 2, 7, 3, 3, None) == EINVAL       # step = horizon
    assert lib.stemgnn_roll_window_quantile(p, p + 64, p + 128, p + 192, 2, 5, 2, 7, 3, 3, 0, 3, None) == EINVAL    # point = Q
    assert lib.stemgnn_window_gather(p, p, p, p, 3, 5, 0, 7, 4, None, None) == EINVAL                  # T < W with H = 0
    assert lib.stemgnn_window_gather(p + 4, p, p, p, 3, 5, 2, 8, 40, None, None) == EINVAL             # float4 rows, unaligned series


# ---- the checker checked -------------------------------------------------------------------------------------------------------
def _buffer(payload, dtype=np.float32):
    payload = np.asarray(payload, dtype=dtype).reshape(-1)
    return np.concatenate([payload, np.full(R.GUARD, R.SENTINEL if np.dtype(dtype).kind == "f" else R.SENTINEL_I, dtype=dtype)])


def test_helpers_agree_with_tests_util():
    from tests import util

    assert (R.GUARD, R.SENTINEL, R.SENTINEL_I) == (util.GUARD, util.SENTINEL, util.SENTINEL_I)
    assert np.float32(R.SENTINEL) == R.SENTINEL                               # exact in fp32, so `==` on a guard is a bit test


def test_checker_fails_on_one_wrong_element():
    sx, sy = R.series_pair(R.GATHER_T, 8)
    x, y, status, _ = R.gather_ref(sx, sy, (9, 20, 31), 5, 2)
    R.check_buffer(_buffer(x), x, "x")
    R.check_buffer(_buffer(y), y, "y (NaN and all)")
    for k in (0, x.size // 2, x.size - 1):
        wrong = x.copy()
        wrong.reshape(-1)[k] = np.nextafter(wrong.reshape(-1)[k], np.float32(9))     # one ulp
        with pytest.raises(AssertionError, match="1 of"):
            R.check_buffer(_buffer(wrong), x, "x")
    wrong = y.copy()
    k = int(np.flatnonzero(np.isnan(y.reshape(-1)))[0])
    wrong.reshape(-1)[k] = 0.0                                                   # a NaN of series_y replaced by a number
    with pytest.raises(AssertionError):
        R.check_buffer(_buffer(wrong), y, "y")
    z = np.zeros(4, np.float32)
    with pytest.raises(AssertionError):
        R.check_buffer(_buffer(-z), z, "the sign of zero")
    want = R.normalize_ref(*R.normalize_case(40, 7, 1), 1)
    R.check_normalized(_buffer(want), want, "normalise")
    for k, v in ((0, 0.5), (7 * 3 + 2, np.nan), (7 * 12 + 1, np.nextafter(want[12, 1], np.float32(9)))):  # a NaN lost, a NaN made, one ulp
        wrong = want.copy()
        wrong.reshape(-1)[k] = v
        with pytest.raises(AssertionError):
            R.check_normalized(_buffer(wrong), want, "normalise")
    t, f, mul, add = R.quantile_case(65, 3, 3, 86, 1, 0)
    want, exact = R.quantile_ref(t, f, R.levels(3), mul, add, 1)
    R.check_metrics(_buffer(want, np.float64), want, exact, "metrics")
    for k, v in ((0, want[0] * (1 + 1e-11)), (int(np.flatnonzero(exact)[0]), np.nextafter(want[np.flatnonzero(exact)[0]], 9.0)),
                 (int(np.flatnonzero(np.isnan(want))[0]), 0.0), (1, np.nan)):
        wrong = want.copy()
        wrong[k] = v
        with pytest.raises(AssertionError):
            R.check_metrics(_buffer(wrong, np.float64), want, exact, "metrics")
    t1, f1, mul1, add1 = R.eval_case(1, 3, 7, 0, 1)                                # count = 1: a single-term mean is off by one ulp
    want1, exact1 = R.eval_ref(t1, f1, mul1, add1, 0)
    assert int(exact1.sum()) == 2 * 3 * 7 and not exact1[:3 + 3 * 7 + 3 * 3].any() and not exact1[-3 * 7:].any()
    R.check_metrics(_buffer(want1, np.float64), want1, exact1, "eval, count = 1")
    wrong = want1.copy()
    k = int(np.flatnonzero(exact1)[-1])
    wrong[k] = np.nextafter(wrong[k], 9.0)
    with pytest.raises(AssertionError, match="must be equal"):
        R.check_metrics(_buffer(wrong, np.float64), want1, exact1, "eval, count = 1")
    ok = want.copy()
    ok[0] *= 1 + 1e-13                                                         # inside the bound on a sum of reals
    R.check_metrics(_buffer(ok, np.float64), want, exact, "metrics")


def test_checker_fails_on_a_row_that_should_have_stayed_poisoned():
    B, L, N, horizon, step = 2, 2, 7, 5, 1
    g = np.random.default_rng(0)
    inputs, forecast = g.normal(size=(B, 4, N)).astype(np.float32), g.normal(size=(B, L, N)).astype(np.float32)
    poison = np.full((B, horizon, N), np.nan, np.float32)
    nxt, steps = R.roll_ref(inputs, forecast, poison, step, horizon)
    assert np.isnan(poison).all() and np.isnan(steps[:, 0]).all() and np.isnan(steps[:, 3:]).all() and not np.isnan(steps[:, 1:3]).any()
    R.check_buffer(_buffer(steps), steps, "forecast_steps")
    for row in (0, 3, 4):
        wrong = steps.copy()
        wrong[1, row] = forecast[1, 0]                                            # written where nothing may be
        with pytest.raises(AssertionError):
            R.check_buffer(_buffer(wrong), steps, "forecast_steps")
    out = np.full((R.STORE_CAPACITY, 3, N), np.nan, np.float32)
    fc, tg = g.normal(size=(4, 3, N)).astype(np.float32), g.normal(size=(4, 3, N)).astype(np.float32)
    for pos, rows in ((0, [0, 1, 2, 3]), (8, [8, 9]), (-1, [0, 1, 2]), (-4, []), (10, [])):
        of, ot = R.store_ref(fc, tg, pos, out, out)
        assert np.flatnonzero(~np.isnan(of[:, 0, 0])).tolist() == rows == np.flatnonzero(~np.isnan(ot[:, 0, 0])).tolist()
        wrong = of.copy()
        wrong[5] = 0.0                                                            # row 5 is never a target here
        with pytest.raises(AssertionError):
            R.check_buffer(_buffer(wrong), of, "out_forecast")


def test_checker_fails_on_one_altered_guard_element():
    x = np.arange(12, dtype=np.float32)
    for dtype in (np.float32, np.float64, np.int64, np.int32):
        for k in (0, 100, R.GUARD - 1):
            full = _buffer(x, dtype)
            R.check_buffer(full, x.astype(dtype), "buffer")
            full[12 + k] = 0
            with pytest.raises(AssertionError, match="guard"):
                R.check_buffer(full, x.astype(dtype), "buffer")
            with pytest.raises(AssertionError, match="guard"):
                R.assert_guard(full, 12, "buffer")
    full = _buffer(x)
    full[12] = np.nan                                                             # NaN in the guard: `!=` sees it
    with pytest.raises(AssertionError, match="guard"):
        R.assert_guard(full, 12, "buffer")
    with pytest.raises(AssertionError):
        R.assert_guard(full[:-1], 12, "a short buffer")


def test_checker_fails_on_a_wrong_status_bit():
    R.check_status(0, 0, "status")
    R.check_status(3, 3, "status")
    for got, want in ((0, 1), (1, 0), (2, 1), (1, 2), (3, 1), (3, 2), (1, 3), (0, 2)):
        with pytest.raises(AssertionError, match="status"):
            R.check_status(got, want, "status")
