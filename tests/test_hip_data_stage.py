"""GPU: the data stage (stemgnn_amd/csrc/data.hip: normalisation, both window gathers, MSE, the window shifts, the forecast store,
evaluate() and the quantile metrics) through the C ABI on NaN-filled, guarded buffers -- the data path's counterpart of
tests/test_hip_front.py, tests/test_hip_block.py, tests/test_hip_gru_paths.py, tests/test_hip_tail_stage.py, tests/test_hip_gemm.py
and tests/test_hip_eigh.py.

Cases, references and the comparison helpers are in tests/helpers/data_ref.py (plain numpy, fp64 where there is arithmetic, written
from include/stemgnn_hip.h); tests/test_data_cases.py proves on the CPU, through stemgnn_data_plan, that the cases reach every thread
class, copy form, grid-stride pass count, MSE form and chunk count of the launchers, and that the helpers fail on one wrong element,
one row that should have stayed poisoned, one altered guard element and one wrong status bit.

Hygiene, for every call: every input is a guarded copy and has its bits compared afterwards; every output and scratch buffer is NaN
(integers: a recognisable poison) before the call, sized exactly by the entry's own size function or the documented shape, with
tests/util.GUARD sentinels behind it; the whole case runs twice on fresh buffers and both runs must agree bit for bit.  The gather
status word starts at 0, is compared with the model's bits after every call and cleared.  Windows outside the series, positions
past `count` and negative positions are defined behaviour: such a row is zeros, and nothing is loaded for it.

Bounds (all the project's own): copies -- the same bits over the whole destination, the elements a call must leave alone included;
normalise -- numpy's bits, NaN where numpy has NaN; MSE -- 1e-6 relative to fp64 (tests/test_hip_data.py), loss_accum exact;
metrics -- rtol 1e-12 per element on sums of reals, equality on count-over-count statistics, NaN exactly where the reference has it."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import data_ref as R
from tests.util import DEV, _Buf, _BufD, _BufI

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    return _lib.load()


def _new(n, dtype, fill=None):
    dtype = np.dtype(dtype)
    kw = {} if fill is None else dict(fill=fill)
    if dtype == np.float32:
        return _Buf(n, **kw)
    if dtype == np.float64:
        return _BufD(n, **kw)
    return _BufI(n, dtype={8: torch.int64, 4: torch.int32}[dtype.itemsize], **kw)


def _in(a):
    """a guarded device copy of a numpy array; `host` keeps what it must still hold after the call"""
    a = np.ascontiguousarray(a)
    b = _new(a.size, a.dtype)
    b.t.copy_(torch.from_numpy(a.reshape(-1)))
    b.host = _back(b)
    return b


def _back(b):
    return b.full.cpu().numpy()


def _unchanged(*inputs):
    for i, b in enumerate(inputs):
        if b is not None:
            R.assert_same_bits(_back(b), b.host, f"input {i}")


def _ptr(b):
    return None if b is None else b.ptr()


def _ok(rc):
    assert rc == 0, rc
    torch.cuda.synchronize()


def _twice(run):
    """`run()` allocates fresh poisoned buffers, calls, checks against the reference and returns what it read back"""
    first, second = run(), run()
    assert len(first) == len(second) > 0
    for i, (a, b) in enumerate(zip(first, second)):
        R.assert_same_bits(b, a, f"second run, buffer {i}")


@pytest.mark.parametrize("case", R.NORMALIZE_CASES, ids=str)
def test_normalize(lib, case):
    T, N, clip01 = case
    raw, sub, div = R.normalize_case(*case)
    want = R.normalize_ref(raw, sub, div, clip01)
    assert np.isnan(want).any() and (want == 0).any() and np.isinf(want).any() != bool(clip01)
    ins = [_in(raw), _in(sub), _in(div)]

    def run():
        out = _Buf(T * N)
        _ok(lib.stemgnn_normalize_series(ins[0].ptr(), ins[1].ptr(), ins[2].ptr(), clip01, out.ptr(), T, N, None))
        R.check_normalized(_back(out), want, f"normalise {case}")
        _unchanged(*ins)
        return [_back(out)]
    _twice(run)


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=str)
def test_window_gather(lib, case):
    N, H, hi = case
    T, W, B = R.GATHER_T, R.GATHER_W, len(hi)
    sx, sy = R.series_pair(T, N)
    dsx, dsy, dhi = _in(sx), _in(sy), _in(np.asarray(hi, dtype=np.int64))
    status = _new(1, np.int32, fill=0)

    def run():
        got = []
        for pair in (False, True):
            x, y = _Buf(B * W * N), _Buf(B * H * N)
            if pair:
                rc = lib.stemgnn_window_gather_pair(dsx.ptr(), dsy.ptr(), dhi.ptr(), x.ptr(), y.ptr(), B, W, H, N, T, status.ptr(), None)
            else:
                rc = lib.stemgnn_window_gather(dsx.ptr(), dhi.ptr(), x.ptr(), y.ptr(), B, W, H, N, T, status.ptr(), None)
            _ok(rc)
            wx, wy, wstatus, zero = R.gather_ref(sx, sy if pair else sx, hi, W, H)
            R.check_buffer(_back(x), wx, f"x {case} pair={pair}")
            R.check_buffer(_back(y), wy, f"y {case} pair={pair}")
            R.assert_guard(_back(status), 1, "status")
            R.check_status(_back(status)[0], wstatus, f"{case} pair={pair}")
            status.t.zero_()
            _unchanged(dsx, dsy, dhi)
            got += [_back(x), _back(y)]
        return got
    _twice(run)


@pytest.mark.parametrize("name", list(R.QUEUE_CASES))
def test_window_gather_queue(lib, name):
    c = R.QUEUE_CASES[name]
    B, W, H, N, T = c["B"], c["W"], c["H"], c["N"], R.GATHER_T
    sx, sy = R.series_pair(T, N)
    if not c["pair"]:
        sy = sx
    order = R.queue_order(c)
    dsx, dsy, dorder = _in(sx), _in(sy), _in(np.asarray(order, dtype=np.int64))
    status = _new(1, np.int32, fill=0)

    def run():
        model = R.QueueModel(order, c["count"], c["wrap"], c["start"])
        queue = _in(np.asarray(model.q, dtype=np.int64))
        got, seen = [], 0
        for k in range(c["calls"]):
            x, y = _Buf(B * W * N), _Buf(B * H * N)
            if c["pair"]:
                rc = lib.stemgnn_window_gather_queue_pair(dsx.ptr(), dsy.ptr(), dorder.ptr(), queue.ptr(), x.ptr(), y.ptr(), B, W, H, N, T,
                                                          status.ptr(), None)
            else:
                rc = lib.stemgnn_window_gather_queue(dsx.ptr(), dorder.ptr(), queue.ptr(), x.ptr(), y.ptr(), B, W, H, N, T, status.ptr(), None)
            _ok(rc)
            wx, wy, wstatus, zero = model.call(sx, sy, B, W, H)
            R.check_buffer(_back(x), wx, f"{name} call {k}: x")
            R.check_buffer(_back(y), wy, f"{name} call {k}: y")
            R.check_buffer(_back(queue), np.asarray(model.q, dtype=np.int64), f"{name} call {k}: queue (position, ticket, count, wrap)")
            R.assert_guard(_back(status), 1, "status")
            R.check_status(_back(status)[0], wstatus, f"{name} call {k}")
            status.t.zero_()
            _unchanged(dsx, dsy, dorder)
            seen |= wstatus
            got += [_back(x), _back(y), _back(queue)]
        if c["bad"]:
            assert seen & 1
        if c["pair"]:
            assert any(np.isnan(g).any() for g in got[1::3])                   # the second series' NaN reached y
        return got
    _twice(run)


@pytest.mark.parametrize("n", R.MSE_FWD_CASES)
def test_mse_fwd(lib, n):
    f, y = R.mse_case(n)
    want, _ = R.mse_ref(f, y)
    df, dy = _in(f), _in(y)
    nscratch = lib.stemgnn_mse_scratch_floats()
    accum = _new(1, np.float64, fill=0.0)
    losses = []
    for k in range(2):                                                       # the second call on re-poisoned buffers, the same accumulator
        scratch, loss = _Buf(nscratch), _Buf(1)
        _ok(lib.stemgnn_mse_fwd(df.ptr(), dy.ptr(), n, scratch.ptr(), loss.ptr(), accum.ptr(), None))
        R.assert_guard(_back(scratch), nscratch, "scratch")
        R.assert_guard(_back(loss), 1, "loss")
        R.assert_guard(_back(accum), 1, "loss_accum")
        _unchanged(df, dy)
        losses.append(_back(loss)[:1].copy())
        err = abs(float(losses[-1][0]) - want) / want
        print(f"mse_fwd n = {n}: loss {float(losses[-1][0])!r}, fp64 {want!r}, relative error {err:.2e}")
        assert err <= R.MSE_RTOL
    R.assert_same_bits(losses[1], losses[0], "second call")
    assert _back(accum)[0] == np.float64(losses[0][0]) + np.float64(losses[1][0])      # exactly: two widened fp32 values, fp64 adds
    scratch, loss = _Buf(nscratch), _Buf(1)                                   # without an accumulator: the same loss
    _ok(lib.stemgnn_mse_fwd(df.ptr(), dy.ptr(), n, scratch.ptr(), loss.ptr(), None, None))
    R.check_buffer(_back(loss), losses[0], "loss with loss_accum = NULL")


@pytest.mark.parametrize("n", R.MSE_BWD_CASES)
def test_mse_bwd(lib, n):
    f, y = R.mse_case(n)
    g = np.asarray([3.0], dtype=np.float32)
    _, want = R.mse_ref(f, y, 3.0)
    df, dy, dg = _in(f), _in(y), _in(g)

    def run():
        out = _Buf(n)
        _ok(lib.stemgnn_mse_bwd(df.ptr(), dy.ptr(), n, dg.ptr(), out.ptr(), None))
        full = _back(out)
        R.assert_guard(full, n, "dforecast")
        assert not np.isnan(full[:n]).any()
        err = float(np.abs(full[:n].astype(np.float64) - want).max() / np.abs(want).max())
        print(f"mse_bwd n = {n}: max-norm relative error {err:.2e}")
        assert err <= R.MSE_RTOL
        _unchanged(df, dy, dg)
        return [full]
    _twice(run)


def _roll(lib, case, quantile):
    B, W, L, N, step, horizon = case[:6]
    Q, point = case[6:] if quantile else (1, None)
    g = np.random.default_rng(sum(case))
    inputs = g.normal(size=(B, W, N)).astype(np.float32)
    forecast = g.normal(size=(B, Q, L, N) if quantile else (B, L, N)).astype(np.float32)
    poison = np.full((B, Q, horizon, N) if quantile else (B, horizon, N), np.nan, dtype=np.float32)
    wnext, wsteps = R.roll_ref(inputs, forecast, poison, step, horizon, point)
    assert np.isnan(wsteps).sum() == B * Q * N * (horizon - min(horizon - step, L)) and not np.isnan(wnext).any()
    di, df = _in(inputs), _in(forecast)

    def run():
        nxt, steps = _Buf(B * W * N), _Buf(poison.size)
        if quantile:
            rc = lib.stemgnn_roll_window_quantile(di.ptr(), df.ptr(), nxt.ptr(), steps.ptr(), B, W, L, N, Q, point, step, horizon, None)
        else:
            rc = lib.stemgnn_roll_window(di.ptr(), df.ptr(), nxt.ptr(), steps.ptr(), B, W, L, N, step, horizon, None)
        _ok(rc)
        R.check_buffer(_back(nxt), wnext, f"inputs_next {case}")
        R.check_buffer(_back(steps), wsteps, f"forecast_steps {case}")
        _unchanged(di, df)
        return [_back(nxt), _back(steps)]
    _twice(run)


@pytest.mark.parametrize("case", R.ROLL_CASES, ids=str)
def test_roll_window(lib, case):
    _roll(lib, case, False)


@pytest.mark.parametrize("case", R.ROLL_QUANTILE_CASES, ids=str)
def test_roll_window_quantile(lib, case):
    _roll(lib, case, True)


@pytest.mark.parametrize("case", R.STORE_CASES, ids=str)
def test_forecast_store(lib, case):
    H, N, pos = case
    B, cap = R.STORE_B, R.STORE_CAPACITY
    g = np.random.default_rng(H * N)
    forecast, target = g.normal(size=(B, H, N)).astype(np.float32), g.normal(size=(B, H, N)).astype(np.float32)
    poison = np.full((cap, H, N), np.nan, dtype=np.float32)
    wf, wt = R.store_ref(forecast, target, pos, poison, poison)
    df, dt, dpos = _in(forecast), _in(target), _in(np.asarray([pos], dtype=np.int64))

    def run():
        of, ot = _Buf(poison.size), _Buf(poison.size)
        _ok(lib.stemgnn_forecast_store(df.ptr(), dt.ptr(), dpos.ptr(), of.ptr(), ot.ptr(), B, H, N, cap, None))
        R.check_buffer(_back(of), wf, f"out_forecast {case}")
        R.check_buffer(_back(ot), wt, f"out_target {case}")
        _unchanged(df, dt, dpos)
        return [_back(of), _back(ot)]
    _twice(run)


@pytest.mark.parametrize("case", R.EVAL_CASES, ids=str)
def test_eval_metrics(lib, case):
    count, H, N, masked, denorm = case
    t, f, mul, add = R.eval_case(*case)
    want, exact = R.eval_ref(t, f, mul, add, masked)
    assert np.isfinite(want).any() or count * H * N == 1
    dt, df = _in(t), _in(f)
    dmul, dadd = (_in(mul), _in(add)) if denorm else (None, None)
    fn, size = (lib.stemgnn_eval_metrics_masked, lib.stemgnn_eval_scratch_doubles_masked) if masked else \
               (lib.stemgnn_eval_metrics, lib.stemgnn_eval_scratch_doubles)

    def run():
        scratch, out = _BufD(size(count, H, N)), _BufD(lib.stemgnn_eval_out_doubles(H, N))
        _ok(fn(dt.ptr(), df.ptr(), _ptr(dmul), _ptr(dadd), count, H, N, scratch.ptr(), out.ptr(), None))
        R.check_metrics(_back(out), want, exact, f"eval {case}")
        R.assert_guard(_back(scratch), scratch.n, "scratch")
        _unchanged(dt, df, dmul, dadd)
        return [_back(out)]
    _twice(run)


@pytest.mark.parametrize("case", R.QUANTILE_CASES, ids=str)
def test_quantile_metrics(lib, case):
    count, Q, H, N, masked, denorm = case
    t, f, mul, add = R.quantile_case(*case)
    taus = R.levels(Q)
    want, exact = R.quantile_ref(t, f, taus, mul, add, masked)
    dt, df = _in(t), _in(f)
    dmul, dadd = (_in(mul), _in(add)) if denorm else (None, None)
    htaus = (ctypes.c_double * Q)(*taus)
    fn = lib.stemgnn_quantile_metrics_masked if masked else lib.stemgnn_quantile_metrics

    def run():
        scratch, out = _BufD(lib.stemgnn_quantile_scratch_doubles(count, Q, H, N)), _BufD(lib.stemgnn_quantile_out_doubles(Q, H))
        _ok(fn(dt.ptr(), df.ptr(), htaus, _ptr(dmul), _ptr(dadd), count, Q, H, N, scratch.ptr(), out.ptr(), None))
        R.check_metrics(_back(out), want, exact, f"quantile metrics {case}")
        R.assert_guard(_back(scratch), scratch.n, "scratch")
        _unchanged(dt, df, dmul, dadd)
        return [_back(out)]
    _twice(run)
