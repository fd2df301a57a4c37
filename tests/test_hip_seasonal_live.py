"""GPU: a seasonal calibrator in the live forecaster -- engine.LiveForecaster.set_calibrator(cal, t_offset) and the seasonal store
of csrc/seasonal.hip inside the replayed graph.

The reference is the project's eager path on the same inputs: Model.predict / ops.roll_window_quantile at batch 1, torch.sort
over the levels, then SeasonalConformalCalibrator.apply with the row's time index (itself checked against numpy in
tests/test_hip_seasonal.py).  Both sides run the same fp32 operations on the same values, so every comparison is one of bit
patterns.  The set-up is that of tests/test_hip_live.py: W = 4, multi_layer 2, H = 2, horizon 5 (three rolling rounds), units 12
(16-byte rows) and 11 (scalar rows); history 8 >= horizon so that forecasts mature; period 6, 3 buckets, t_offset 4."""
import numpy as np
import pytest
import torch

from tests.helpers import seasonal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261020
W, MULTI, H, HORIZON, HISTORY, T = 4, 2, 2, 5, 8, 24
TAUS = (0.1, 0.5, 0.9)
PERIOD, BUCKETS, PHASE, T_OFFSET = 6, 3, 1, 4
assert T >= 2 * PERIOD + W


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


_series, _models, _wants, _cals = {}, {}, {}, {}


def series_of(N):
    """[T, N] float64 readings without gaps; no normalisation, so the ring holds float32(series)"""
    if N not in _series:
        _series[N] = np.random.default_rng(SEED + N).normal(size=(T, N))
    return _series[N]


def data_of(N):
    return torch.from_numpy(series_of(N)).float().to(DEV)


def model_of(N, quant=True):
    key = (N, quant)
    if key not in _models:
        from stemgnn_amd import Model
        torch.manual_seed(SEED + N)
        _models[key] = Model(N, 2, W, MULTI, horizon=H, **(dict(quantiles=TAUS) if quant else {})).to(DEV).eval()
    return _models[key]


def make_live(N, quant=True, **kw):
    from stemgnn_amd import LiveForecaster
    return LiveForecaster(model_of(N, quant), W, HORIZON, history=HISTORY, **kw)


def eager_roll(model, x):
    """trainer.rolling_forecast's inner loop at batch 1: [Q, horizon, N]"""
    from stemgnn_amd import ops
    steps = torch.empty(1, len(TAUS), HORIZON, x.shape[2], device=DEV)
    window, done = x, 0
    while done < HORIZON:
        out, _ = model.predict(window)
        window = ops.roll_window_quantile(window, out, steps, done, HORIZON, model.point_index)
        done += min(HORIZON - done, out.shape[-2])
    return steps[0]


def wanted(N):
    """{t: the eager rolling forecast of the window that ends at row t, levels in order}, computed once and never changed"""
    if N not in _wants:
        data, model = data_of(N), model_of(N)
        _wants[N] = {t: torch.sort(eager_roll(model, data[t - W:t][None].contiguous()), dim=0, stable=True).values.clone()
                     for t in range(W, T + 1)}
    return _wants[N]


def backtest(N):
    """(forecasts [m, Q, horizon, N] in order, targets [m, horizon, N], origins [m]) of every window whose targets exist"""
    ts = list(range(W, T - HORIZON + 1))
    fc = torch.stack([wanted(N)[t] for t in ts])
    tg = torch.stack([data_of(N)[t:t + HORIZON] for t in ts])
    return fc, tg, torch.tensor(ts, dtype=torch.int64, device=DEV)


def seasonal_of(N, season=(PERIOD, BUCKETS, PHASE), shift=0.0, t_offset=T_OFFSET):
    """fitted on the rearranged backtest forecasts, on the user's clock (row tau has t = tau + t_offset); every entry finite"""
    key = (N, season, shift, t_offset)
    if key not in _cals:
        from stemgnn_amd.math_utils import SeasonalConformalCalibrator
        fc, tg, origins = backtest(N)
        cal = SeasonalConformalCalibrator(TAUS, *season).fit(tg, fc, origins + t_offset)
        assert tuple(cal.offsets.shape) == (season[1], 1, HORIZON, 1) and bool(torch.isfinite(cal.offsets).all())
        assert len({float(v) for v in cal.offsets[:, 0, 0, 0]}) == season[1]            # the buckets differ: the slice matters
        if shift:
            cal = SeasonalConformalCalibrator(TAUS, *season).load_state_dict(dict(cal.state_dict(), offsets=cal.offsets + shift))
        _cals[key] = cal
    return _cals[key]


def static_of(N):
    from stemgnn_amd.math_utils import ConformalCalibrator
    fc, tg, _ = backtest(N)
    return ConformalCalibrator(TAUS).fit(tg, fc)


def finished(N, t, cal, t_offset=T_OFFSET):
    """what forecast() must return at `t` rows pushed: the eager rows, widened with the buckets of t + t_offset + h"""
    return cal.apply(wanted(N)[t][None], origin=t + t_offset)[0]


def run(live, N, rows, cal, t_offset=T_OFFSET):
    """push rows one by one, forecast wherever a window exists, compare"""
    series = series_of(N)
    for t in rows:
        assert live.push(series[t]) == t + 1
        if live.ready:
            assert same_bits(live.forecast(), finished(N, t + 1, cal, t_offset)), t


# ---- bit-for-bit serving ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", (True, False), ids=("graph", "eager"))
@pytest.mark.parametrize("N", (12, 11))
def test_live_forecast_equals_the_eager_loop_and_apply(N, graph):
    cal = seasonal_of(N)
    live = make_live(N, rearrange=True, graph=graph)
    live.set_calibrator(cal, t_offset=T_OFFSET)
    run(live, N, range(T), cal)
    assert (live._replay is not None) == graph
    used = {cal.bucket_of(t + T_OFFSET + h) for t in range(W, T + 1) for h in range(HORIZON)}
    assert used == set(range(BUCKETS))
    # the slices are really chosen per step: one forecast's steps fall into more than one bucket, and a static table differs
    assert len({cal.bucket_of(T + T_OFFSET + h) for h in range(HORIZON)}) > 1
    flat = R.apply_np(wanted(N)[T][None].cpu().numpy(), cal.offsets.cpu().numpy(), T + T_OFFSET, cal.pairs, cal.season)
    assert np.array_equal(flat.view(np.int32), bits(finished(N, T, cal)[None]).numpy())


def test_constructor_takes_a_seasonal_calibrator():
    cal = seasonal_of(12)
    live = make_live(12, rearrange=True, calibrator=cal)          # the clock starts at 0 until set_calibrator names another
    run(live, 12, range(W + 3), cal, t_offset=0)
    live.set_calibrator(cal, t_offset=T_OFFSET)
    assert live._replay is None
    run(live, 12, range(W + 3, W + 6), cal)


# ---- refit, changed season ------------------------------------------------------------------------------------------------------
def test_refit_of_the_same_shape_is_seen_without_a_new_capture():
    N = 12
    cal, refit = seasonal_of(N), seasonal_of(N, shift=0.375)
    live = make_live(N, rearrange=True)
    live.set_calibrator(cal, t_offset=T_OFFSET)
    run(live, N, range(10), cal)
    replay, buffer = live._replay, live._offsets
    assert replay is not None
    live.set_calibrator(refit, t_offset=T_OFFSET)
    assert live._replay is replay and live._offsets is buffer and live._armed
    run(live, N, range(10, 14), refit)
    assert live._replay is replay
    assert not same_bits(finished(N, 12, refit), finished(N, 12, cal))


def test_a_changed_season_or_clock_captures_again_and_is_right():
    N = 12
    cal = seasonal_of(N)
    other = seasonal_of(N, season=(4, 2, 0))
    live = make_live(N, rearrange=True)
    live.set_calibrator(cal, t_offset=T_OFFSET)
    run(live, N, range(8), cal)
    replay = live._replay
    live.set_calibrator(other, t_offset=T_OFFSET)
    assert live._replay is None and not live._armed
    run(live, N, range(8, 12), other)
    second = live._replay
    assert second is not None and second is not replay
    # the same tables on another clock: the folded phase changes
    live.set_calibrator(other, t_offset=T_OFFSET + 1)
    assert live._replay is None
    run(live, N, range(12, 16), other, t_offset=T_OFFSET + 1)
    # seasonal -> static -> none
    static = static_of(N)
    live.set_calibrator(static)
    assert live._replay is None
    live.push(series_of(N)[16])
    assert same_bits(live.forecast(), static.apply(wanted(N)[17][None])[0])
    live.set_calibrator(None)
    live.push(series_of(N)[17])
    assert same_bits(live.forecast(), wanted(N)[18])


# ---- matured() -> fit -> set_calibrator -----------------------------------------------------------------------------------------
def test_matured_round_trip():
    from stemgnn_amd.math_utils import SeasonalConformalCalibrator
    N = 11
    live = make_live(N, rearrange=True)
    series = series_of(N)
    for t in range(T - 4):
        live.push(series[t])
        if live.ready:
            live.forecast()
    fc, tg, origins = live.matured()
    assert origins.dtype == torch.int64 and origins.numel() >= 3
    for o, f in zip(origins.tolist(), fc):
        assert same_bits(f, wanted(N)[o])
    assert same_bits(tg, torch.stack([data_of(N)[o:o + HORIZON] for o in origins.tolist()]))
    cal = SeasonalConformalCalibrator(TAUS, PERIOD, BUCKETS, PHASE, fallback="inf").fit(tg, fc, origins + T_OFFSET,
                                                                                       ignore_nan=True)
    pairs, coverage = R.pairs_of(TAUS)
    want, counts = R.fit_np(tg.cpu().numpy(), fc.cpu().numpy(), (origins + T_OFFSET).cpu().numpy(), pairs, coverage,
                            (PERIOD, BUCKETS, PHASE), True, False, True)
    assert np.array_equal(cal.offsets.cpu().numpy(), want) and np.array_equal(cal.counts.cpu().numpy(), counts)
    pooled = SeasonalConformalCalibrator(TAUS, PERIOD, BUCKETS, PHASE).fit(tg, fc, origins + T_OFFSET, ignore_nan=True)
    live.set_calibrator(pooled, t_offset=T_OFFSET)
    run(live, N, range(T - 4, T), pooled)


# ---- restart ------------------------------------------------------------------------------------------------------------------
def test_state_round_trip_continues_with_identical_forecasts():
    N = 12
    cal = seasonal_of(N)
    live = make_live(N, rearrange=True)
    live.set_calibrator(cal, t_offset=T_OFFSET)
    run(live, N, range(13), cal)
    state = live.state_dict()
    assert state["calibrator_kind"] == "seasonal" and state["t_offset"] == T_OFFSET
    fresh = make_live(N, rearrange=True, calibrator=cal).load_state_dict(state)
    late = make_live(N, rearrange=True)
    late.set_calibrator(cal)                                      # the clock comes with the state
    late.load_state_dict(state)
    assert late.t_offset == T_OFFSET
    series = series_of(N)
    for t in range(13, T):
        got = []
        for one in (live, fresh, late):
            assert one.push(series[t]) == t + 1
            got.append(one.forecast())
        assert same_bits(got[0], got[1]) and same_bits(got[0], got[2]) and same_bits(got[0], finished(N, t + 1, cal))
    assert same_bits(fresh.out_forecast, live.out_forecast) and fresh._origins == live._origins
    with pytest.raises(ValueError, match="seasonal"):
        make_live(N, rearrange=True).load_state_dict(state)
    assert make_live(N, rearrange=True, calibrator=static_of(N)).state_dict()["calibrator_kind"] == "static"
    assert make_live(N, rearrange=True).state_dict()["calibrator_kind"] is None


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    from stemgnn_amd.engine import QuantileForecastStep
    from stemgnn_amd.math_utils import AdaptiveConformal
    N = 12
    cal = seasonal_of(N)
    live = make_live(N, rearrange=True)
    live.set_calibrator(cal, t_offset=T_OFFSET)
    with pytest.raises(ValueError, match="seasonal"):
        live.set_adaptive(AdaptiveConformal(TAUS))
    run(live, N, range(6), cal)                                   # and it goes on serving
    with pytest.raises(ValueError, match="seasonal"):
        live.set_adaptive(AdaptiveConformal(TAUS))
    adaptive = make_live(N, rearrange=True)
    adaptive.set_adaptive(AdaptiveConformal(TAUS))
    with pytest.raises(ValueError, match="adaptive"):
        adaptive.set_calibrator(cal, t_offset=T_OFFSET)
    with pytest.raises(ValueError, match="seasonal"):
        QuantileForecastStep(model_of(N), 2, W, HORIZON, data_of(N), 8, calibrator=cal)
    with pytest.raises(ValueError, match="point model"):
        make_live(N, quant=False, calibrator=cal)
    with pytest.raises(ValueError, match="quantile model"):
        make_live(N, quant=False).set_calibrator(cal, t_offset=T_OFFSET)
    with pytest.raises(ValueError, match="point model"):
        make_live(N, quant=False, calibrator=static_of(N))        # as for the static one


# ---- the static paths are untouched -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", (True, False), ids=("graph", "eager"))
def test_static_calibrator_paths_are_untouched(graph):
    from stemgnn_amd import ops
    N = 12
    static = static_of(N)
    live = make_live(N, rearrange=True, calibrator=static, graph=graph)
    series = series_of(N)
    for t in range(10):
        live.push(series[t])
        if live.ready:
            assert same_bits(live.forecast(), static.apply(wanted(N)[t + 1][None])[0])
    assert "seasonal" not in live._finish_kw and live.state_dict()["t_offset"] == 0
    # the unseasoned store entry itself, against finish + apply
    steps = torch.randn(3, 3, HORIZON, N, device=DEV)
    slab, targets = torch.zeros(5, 3, HORIZON, N, device=DEV), torch.zeros(5, HORIZON, N, device=DEV)
    pos = torch.tensor([1], dtype=torch.int64, device=DEV)
    ops.quantile_store(steps, torch.ones(3, HORIZON, N, device=DEV), pos, slab, targets, rearrange=True, offsets=static.offsets,
                       pairs=static.pairs)
    assert same_bits(slab[1:4], static.apply(torch.sort(steps, dim=1, stable=True).values))
    assert bool((slab[0] == 0).all()) and bool((slab[4] == 0).all()) and bool((targets[1:4] == 1).all())


def test_seasonal_store_entry_on_a_batch():
    """the store on its own, B = 3 rows whose origins are t_dev + b: rows beyond the capacity are dropped, targets copied"""
    from stemgnn_amd import ops
    for N in (12, 11):
        cal = seasonal_of(N)
        steps = torch.randn(3, 3, HORIZON, N, device=DEV)
        slab, targets = torch.zeros(4, 3, HORIZON, N, device=DEV), torch.zeros(4, HORIZON, N, device=DEV)
        pos = torch.tensor([2], dtype=torch.int64, device=DEV)
        t_dev = torch.tensor([-9], dtype=torch.int64, device=DEV)
        season = (PERIOD, BUCKETS, (PHASE + T_OFFSET) % PERIOD)
        ops.quantile_store_seasonal(steps, torch.ones(3, HORIZON, N, device=DEV), pos, slab, targets, rearrange=True,
                                    offsets=cal.offsets, pairs=cal.pairs, seasonal=season, t_dev=t_dev)
        want = cal.apply(torch.sort(steps, dim=1, stable=True).values, origin=-9 + T_OFFSET)
        assert same_bits(slab[2:4], want[:2])                     # the third row is beyond the capacity
        assert bool((slab[:2] == 0).all()) and bool((targets[2:4] == 1).all()) and bool((targets[:2] == 0).all())


@pytest.mark.parametrize("N", (4, 5), ids=("float4", "scalar"))
@pytest.mark.parametrize("Q", (3, 17, 32))
@pytest.mark.parametrize("rearrange", (False, True), ids=("as-is", "rearrange"))
def test_seasonal_store_column_kernel_paths(rearrange, Q, N):
    """the seasonal store through every path of the shared column kernel, against numpy bit for bit: one LDS plane (as-is) and
    two (rearrange); Q = 17 is the first value past the float4 form's limit of 16, Q = 32 shrinks the workgroup to 128 threads
    whose two planes fill 32 KB exactly; N = 4 takes the float4 form, N = 5 the scalar one with a ragged last column block.
    B = 3 rows at pos = 2 of capacity 4: the third row is dropped.  Season (7, 3, 2) with t_dev = -11: the stored rows' steps
    fall in buckets (2, 2) and (2, 0)."""
    from stemgnn_amd import ops
    B, Hs, cap, season, t0 = 3, 2, 4, (7, 3, 2), -11
    assert [[R.bucket(t0 + b + h, *season) for h in range(Hs)] for b in range(2)] == [[2, 2], [2, 0]]
    rng = np.random.default_rng(SEED + 64 * Q + 2 * N + int(rearrange))
    pairs = tuple((i, Q - 1 - i) for i in range(Q // 2))
    steps = rng.normal(size=(B, Q, Hs, N)).astype(np.float32)
    target = rng.normal(size=(B, Hs, N)).astype(np.float32)
    offsets = np.abs(rng.normal(size=(season[1], len(pairs), Hs, N))).astype(np.float32)
    slab, targets = torch.zeros(cap, Q, Hs, N, device=DEV), torch.zeros(cap, Hs, N, device=DEV)
    ops.quantile_store_seasonal(torch.from_numpy(steps).to(DEV), torch.from_numpy(target).to(DEV),
                                torch.tensor([2], dtype=torch.int64, device=DEV), slab, targets, rearrange=rearrange,
                                offsets=torch.from_numpy(offsets).to(DEV), pairs=pairs, per_step=True, per_node=True,
                                seasonal=season, t_dev=torch.tensor([t0], dtype=torch.int64, device=DEV))
    ordered = np.sort(steps, axis=1, kind="stable") if rearrange else steps
    want = R.apply_np(ordered, offsets, t0, pairs, season)
    assert same_bits(slab[2:], torch.from_numpy(want[:2]))
    assert same_bits(targets[2:], torch.from_numpy(target[:2]))
    assert bool((slab[:2] == 0).all()) and bool((targets[:2] == 0).all())
