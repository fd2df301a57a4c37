"""GPU: live forecasting -- the ingest kernels of csrc/live.hip and engine.LiveForecaster on top of them.

Every reference is one of the project's earlier paths on the same inputs (ForecastDataset's normalisation and imputation, the eager
Model.predict / ops.roll_window loop, torch.sort + ConformalCalibrator.apply), never the code under test; both sides run the same
kernels on the same values, so every comparison is torch.equal or one of bit patterns -- there is no tolerance in this file.

Shapes: units 11 (scalar row copies) and 12 (16-byte row copies), W = 4, multi_layer 2, H = 2, horizon 5 (three rolling rounds, the
last one partial), history 3, so the ring has C = 12 slots and the 40-row series wraps it three times.  One fixed seed.

Two remarks on the cases.  (i) A window that ends at row t > T - H cannot be asked of ops.window_gather (it wants H target rows
behind the window): the reference window is the slice ds.data[t - W:t], checked to BE window_gather's result wherever that exists.
(ii) With history 3 < horizon 5 a forecast made at every row is overwritten before it matures, so the every-row pass can only
show that matured() stays empty; a second pass forecasts every fourth row, where two stored forecasts are matured at a time."""
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261019
W, MULTI, H, HORIZON, HISTORY, T = 4, 2, 2, 5, 3, 40
C = W + HORIZON + HISTORY
TAUS = (0.1, 0.5, 0.9)
GAP_COL = 7                                  # units 12: the column whose first three readings are missing
METHODS = ("z_score", "min_max", None)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def same_nan_aware(a, b):
    """equal shapes, NaN at the same places, equal bit patterns everywhere else"""
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def raw_series(N):
    """[T, N] float64 raw readings: missing = 0.0 and NaN entries in several rows after row 0 (the last row included)."""
    rng = np.random.default_rng(SEED + N)
    s = rng.normal(loc=3.0, scale=2.0, size=(T, N))
    s[s == 0.0] = 1.0
    for t, n, v in ((5, 1, 0.0), (6, 1, 0.0), (9, 3, np.nan), (17, 0, 0.0), (18, 0, np.nan), (19, 0, 0.0), (23, 5, np.nan),
                    (30, N - 1, 0.0), (38, 2, 0.0), (39, 2, np.nan), (39, N - 1, 0.0)):
        s[t, n] = v
    if N == 12:
        s[0, GAP_COL], s[1, GAP_COL], s[2, GAP_COL] = 0.0, np.nan, 0.0
    return s


def statistics(N, method):
    rng = np.random.default_rng(SEED + 100 + N)
    if method == "z_score":
        return dict(mean=rng.normal(3.0, 0.5, size=N), std=rng.uniform(1.0, 3.0, size=N))
    if method == "min_max":                   # narrower than the data: the clip is live on both sides
        return dict(min=rng.uniform(0.5, 1.5, size=N), max=rng.uniform(4.0, 5.0, size=N))
    return None


_refs = {}


def reference(N, method):
    """The dataset a backtest would hold for this stream, computed once: .data / .target [T, N] on the device.  For the column
    with leading gaps (units 12) those readings are set to `fill` first -- a stream cannot back-fill from the future -- and are
    NaN in the target, as every missing reading is."""
    key = (N, method)
    if key in _refs:
        return _refs[key]
    from stemgnn_amd.forecast_dataloader import ForecastDataset
    series = raw_series(N)
    stat = statistics(N, method)
    if method == "z_score":
        fill, fill_arg = np.asarray(stat["mean"], dtype=np.float64), None          # the default: the `sub` statistic
    elif method == "min_max":
        fill, fill_arg = np.asarray(stat["min"], dtype=np.float64), None
    else:
        fill = fill_arg = np.full(N, 1.25)                                          # (the default 0.0 is `missing` itself)
    filled = series.copy()
    if N == 12:
        filled[:3, GAP_COL] = fill[GAP_COL]
    ds = ForecastDataset(filled, W, H, method, None if stat is None else dict(stat), missing=0.0, device=DEV)
    target = ds.target.clone()
    if N == 12:
        target[:3, GAP_COL] = float("nan")
        if method in ("z_score", "min_max"):
            assert bool((ds.data[:3, GAP_COL] == 0).all())                          # the default fill normalises to exactly 0
    missing = np.isnan(series) | (series == 0.0)
    assert missing[1:].any(axis=1).sum() >= 8 and not missing[0, [c for c in range(N) if c != GAP_COL or N != 12]].any()
    assert torch.equal(torch.isnan(target).cpu(), torch.from_numpy(missing))
    assert not bool(torch.isnan(ds.data).any())
    _refs[key] = types.SimpleNamespace(series=series, stat=stat, fill_arg=fill_arg, data=ds.data, target=target, N=N,
                                       method=method)
    return _refs[key]


_models = {}


def model_of(N, quant):
    key = (N, quant)
    if key not in _models:
        from stemgnn_amd import Model
        torch.manual_seed(SEED + N + (1000 if quant else 0))
        _models[key] = Model(N, 2, W, MULTI, horizon=H, **(dict(quantiles=TAUS) if quant else {})).to(DEV).eval()
    return _models[key]


def make_live(ref, quant=False, **kw):
    from stemgnn_amd import LiveForecaster
    return LiveForecaster(model_of(ref.N, quant), W, HORIZON, normalize_method=ref.method,
                          norm_statistic=None if ref.stat is None else dict(ref.stat), missing=0.0, fill=ref.fill_arg,
                          history=HISTORY, **kw)


def window_at(ref, t):
    """the window that ends at row t: rows t - W .. t - 1 of the dataset, [1, W, N]"""
    from stemgnn_amd import ops
    x = ref.data[t - W:t][None].contiguous()
    if t + H <= T:
        got, _ = ops.window_gather(ref.data, torch.tensor([t], dtype=torch.int64, device=DEV), W, H)
        assert same_bits(got, x)
    return x


def eager_roll(model, x, **kw):
    """trainer.rolling_forecast's inner loop at batch 1: [horizon, N] / [Q, horizon, N]"""
    from stemgnn_amd import ops
    quant = model.quantiles is not None
    steps = torch.empty((1,) + ((len(TAUS),) if quant else ()) + (HORIZON, x.shape[2]), device=DEV)
    window, done, rounds = x, 0, 0
    while done < HORIZON:
        out, _ = model.predict(window, **kw)
        if quant:
            window = ops.roll_window_quantile(window, out, steps, done, HORIZON, model.point_index)
        else:
            window = ops.roll_window(window, out, steps, done, HORIZON)
        done += min(HORIZON - done, out.shape[-2])
        rounds += 1
    assert rounds == 3
    return steps[0]


_wants = {}


def wanted(N, quant, adjacency=None):
    """{t: the eager rolling forecast of the window that ends at row t} for t = W .. T, computed once and never changed"""
    key = (N, quant, adjacency is not None)
    if key not in _wants:
        ref, model = reference(N, "z_score"), model_of(N, quant)
        kw = {} if adjacency is None else dict(adjacency=adjacency)
        _wants[key] = {t: eager_roll(model, window_at(ref, t), **kw).clone() for t in range(W, T + 1)}
    return _wants[key]


_graphs = {}


def prior_graph(N):
    if N not in _graphs:
        from stemgnn_amd import LatentGraph
        A = np.random.default_rng(SEED + 7 + N).uniform(0.1, 1.0, size=(N, N)).astype(np.float32)
        _graphs[N] = LatentGraph.from_adjacency(torch.from_numpy(A), device=DEV)
    return _graphs[N]


def sort_q(raw):
    return torch.sort(raw, dim=0, stable=True).values


_cals = {}


def calibrator_of(N, shift=0.0):
    """fitted on the REARRANGED backtest forecasts of every window whose targets exist (the rule of rearrange + calibrate)"""
    key = (N, shift)
    if key not in _cals:
        from stemgnn_amd.math_utils import ConformalCalibrator
        ref, raw = reference(N, "z_score"), wanted(N, True)
        ts = [t for t in range(W, T - HORIZON + 1)]
        fc = torch.stack([sort_q(raw[t]) for t in ts])
        tg = torch.stack([ref.target[t:t + HORIZON] for t in ts])
        cal = ConformalCalibrator(TAUS).fit(tg, fc, ignore_nan=True)
        assert tuple(cal.offsets.shape) == (1, HORIZON, 1) and bool(torch.isfinite(cal.offsets).all())
        if shift:
            cal = ConformalCalibrator(TAUS).load_state_dict(dict(cal.state_dict(), offsets=cal.offsets + shift))
        _cals[key] = cal
    return _cals[key]


def finished(N, t, cal):
    return cal.apply(sort_q(wanted(N, True)[t])[None])[0]


# ---- 1. ingest equals the dataset ---------------------------------------------------------------------------------------------
def chronological(ring, rows):
    """the last C rows pushed, oldest first"""
    idx = torch.tensor([tau % C for tau in range(rows - C, rows)], dtype=torch.int64, device=ring.device)
    return ring.index_select(0, idx)


def push_row_by_row(live, series):
    for t in range(T):
        assert live.push(series[t]) == t + 1                      # numpy [N]


def push_mixed_chunks(live, series):
    t, sizes = 0, (1, 3, 7)
    i = 0
    while t < T:
        k = min(sizes[i % 3], T - t)
        live.push(torch.from_numpy(series[t:t + k].copy()))        # host tensor [K, N]
        t, i = t + k, i + 1
    assert i > 9


def push_bulk(live, series):
    live.push(torch.from_numpy(series).to(DEV))                    # device tensor, K = 40 > C: only the last C rows are stored


@pytest.mark.parametrize("method", METHODS, ids=lambda m: str(m))
@pytest.mark.parametrize("N", (11, 12))
def test_ingest_equals_the_dataset(N, method):
    ref = reference(N, method)
    want_x, want_y = ref.data[T - C:], ref.target[T - C:]
    lasts = []
    for way in (push_row_by_row, push_mixed_chunks, push_bulk):
        live = make_live(ref)
        assert (live.rows, live.ready, live.C) == (0, False, C)
        way(live, ref.series)
        torch.cuda.synchronize()
        assert live.rows == T and live.ready and int(live.t_dev.item()) == T
        assert (live.ring_x.data_ptr() % 16 == 0) and (N % 4 == 0) == (N == 12)
        assert same_bits(chronological(live.ring_x, T), want_x), (way.__name__, N, method)
        assert same_nan_aware(chronological(live.ring_y, T), want_y), (way.__name__, N, method)
        lasts.append(live.last.clone())
    # the fill state: every column's last valid raw reading, whatever the chunking
    marked = np.where(np.isnan(ref.series) | (ref.series == 0.0), np.nan, ref.series)
    last_valid = np.array([col[~np.isnan(col)][-1] for col in marked.T])
    for last in lasts:
        assert torch.equal(last.cpu(), torch.from_numpy(last_valid))


def test_ring_wraps_and_partial_fill():
    """fewer rows than slots: the rows pushed sit in slots 0 .. rows - 1, the rest of ring_y is still NaN; then past one wrap"""
    ref = reference(12, "z_score")
    live = make_live(ref)
    live.push(ref.series[:5])
    torch.cuda.synchronize()
    assert same_bits(live.ring_x[:5], ref.data[:5]) and same_nan_aware(live.ring_y[:5], ref.target[:5])
    assert bool(torch.isnan(live.ring_y[5:]).all())
    live.push(ref.series[5:15])                                    # rows 12, 13, 14 land in slots 0, 1, 2
    torch.cuda.synchronize()
    assert same_bits(live.ring_x[:3], ref.data[12:15]) and same_bits(live.ring_x[3:], ref.data[3:12])


@pytest.mark.parametrize("N", (11, 12))
def test_ring_gather_returns_nan_rows_for_windows_the_ring_does_not_hold(N):
    from stemgnn_amd import ops
    ref = reference(N, "z_score")
    live = make_live(ref)
    live.push(ref.series[:30])
    starts = torch.tensor([30 - C, 25, -1, 30 - C - 1, 26, 7], dtype=torch.int64, device=DEV)   # L = 5: 26 reaches row 30
    ops.ring_status_word(DEV).zero_()
    got = ops.ring_gather(live.ring_y, live.t_dev, HORIZON, starts=starts)
    torch.cuda.synchronize()
    for b, s in enumerate(starts.tolist()):
        if s in (30 - C, 25):
            assert same_nan_aware(got[b], ref.target[s:s + HORIZON]), s
        else:
            assert bool(torch.isnan(got[b]).all()), s
    with pytest.raises(IndexError):
        ops.check_ring_status(DEV)
    ops.check_ring_status(DEV)                                     # the word was cleared
    # the current window, at the device-side head
    x = ops.ring_gather(live.ring_x, live.t_dev, W, back=W)
    assert same_bits(x, ref.data[26:30][None])
    ops.check_ring_status(DEV)


# ---- 2. forecast equals predict ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (11, 12))
def test_forecast_equals_the_eager_predict_loop(N):
    ref, want, G = reference(N, "z_score"), wanted(N, False), prior_graph(N)
    want_adj = wanted(N, False, adjacency=G)
    replayed, eager, fixed = make_live(ref), make_live(ref, graph=False), make_live(ref, adjacency=G)
    for t in range(1, T + 1):
        for live in (replayed, eager, fixed):
            live.push(ref.series[t - 1])
        if t < W:
            assert not replayed.ready
            with pytest.raises(RuntimeError):
                replayed.forecast()
            continue
        f, e, a = replayed.forecast(), eager.forecast(), fixed.forecast()
        assert tuple(f.shape) == (HORIZON, N)
        assert same_bits(f, want[t]) and same_bits(e, want[t]) and same_bits(f, e), t
        assert same_bits(a, want_adj[t]), t
        assert same_bits(replayed.forecast(), f)                   # twice at the same t: the same slot, the same rows
    assert replayed._replay is not None and fixed._replay is not None and eager._replay is None
    assert not same_bits(want[T], want_adj[T])
    assert replayed._origins == [T - (T - s) % HISTORY for s in range(HISTORY)] == replayed.origins.tolist()


@pytest.mark.parametrize("N", (11, 12))
def test_quantile_forecast_raw_and_finished(N):
    ref, raw, cal = reference(N, "z_score"), wanted(N, True), calibrator_of(N)
    plain = make_live(ref, quant=True)
    served = make_live(ref, quant=True, rearrange=True, calibrator=cal)
    served_eager = make_live(ref, quant=True, rearrange=True, calibrator=cal, graph=False)
    crossed = 0
    for t in range(1, T + 1):
        for live in (plain, served, served_eager):
            live.push(ref.series[t - 1])
        if t < W:
            continue
        f = plain.forecast()
        assert tuple(f.shape) == (len(TAUS), HORIZON, N) and same_bits(f, raw[t]), t
        want = finished(N, t, cal)
        assert same_bits(served.forecast(), want) and same_bits(served_eager.forecast(), want), t
        crossed += int(not same_bits(sort_q(raw[t]), raw[t]))
    assert crossed > 10, "the untrained heads cross: without it rearrangement would show nothing"
    assert served._replay is not None and served_eager._replay is None


# ---- 3. matured pairs ---------------------------------------------------------------------------------------------------------------
def expected_origins(slots, rows):
    return sorted(o for o in slots.values() if o + HORIZON <= rows and o >= rows - C)


def test_matured_stays_empty_when_every_row_forecasts_into_three_slots():
    """history 3 < horizon 5: a forecast made at every row is overwritten before its targets are complete"""
    N = 11
    ref, want = reference(N, "z_score"), wanted(N, False)
    live = make_live(ref)
    slots = {}
    for t in range(1, T + 1):
        live.push(ref.series[t - 1])
        fc, tg, origins = live.matured()
        assert expected_origins(slots, t) == [] == origins.tolist()
        assert tuple(fc.shape) == (0, HORIZON, N) and tuple(tg.shape) == (0, HORIZON, N) and origins.dtype == torch.int64
        if t >= W:
            assert same_bits(live.forecast(), want[t])
            slots[t % HISTORY] = t
    assert live.origins.tolist() == live._origins


@pytest.mark.parametrize("N", (11, 12))
def test_matured_pairs_of_a_forecast_every_fourth_row(N):
    from stemgnn_amd.math_utils import ConformalCalibrator
    ref, raw = reference(N, "z_score"), wanted(N, True)
    live = make_live(ref, quant=True)
    slots, seen, most = {}, set(), None
    fc, tg, origins = live.matured()                               # before anything was pushed
    assert tuple(fc.shape) == (0, len(TAUS), HORIZON, N) and tuple(tg.shape) == (0, HORIZON, N) and origins.numel() == 0
    for t in range(1, T + 1):
        live.push(ref.series[t - 1])
        exp = expected_origins(slots, t)
        fc, tg, origins = live.matured()
        assert origins.tolist() == exp, t
        if t < W + HORIZON:
            assert exp == [], "empty before the first maturity"
        assert tuple(fc.shape) == (len(exp), len(TAUS), HORIZON, N) and tuple(tg.shape) == (len(exp), HORIZON, N)
        for i, o in enumerate(exp):
            assert same_bits(fc[i], raw[o]), (t, o)                # the stored forecast, unchanged
            assert same_nan_aware(tg[i], ref.target[o:o + HORIZON]), (t, o)
            seen.add(o)
        if len(exp) == 2:
            most = (fc.clone(), tg.clone(), list(exp))
        if t >= W and t % 4 == 0:
            assert same_bits(live.forecast(), raw[t])
            slots[t % HISTORY] = t
    assert seen == set(range(W, T - HORIZON + 1, 4)) and most is not None
    assert bool(torch.isnan(torch.cat([ref.target[o:o + HORIZON] for o in seen])).any()), "targets with missing readings"
    # the pairs feed the calibrator as they are, and give what the backtest rows give
    fc, tg, exp = most
    a = ConformalCalibrator(TAUS).fit(tg, fc, ignore_nan=True)
    b = ConformalCalibrator(TAUS).fit(torch.stack([ref.target[o:o + HORIZON] for o in exp]),
                                      torch.stack([raw[o] for o in exp]), ignore_nan=True)
    assert same_bits(a.offsets, b.offsets) and torch.equal(a.counts, b.counts)
    assert int(a.counts.sum()) < 2 * HORIZON * N or not bool(torch.isnan(tg).any())


# ---- 4. set_calibrator without re-capture --------------------------------------------------------------------------------------------
def test_set_calibrator_reuses_the_captured_graph():
    N = 12
    ref, raw = reference(N, "z_score"), wanted(N, True)
    cal, cal2 = calibrator_of(N), calibrator_of(N, shift=0.375)
    live = make_live(ref, quant=True, rearrange=True, calibrator=cal)
    live.push(ref.series[:W + 1])
    assert same_bits(live.forecast(), finished(N, W + 1, cal))
    rep = live._replay
    assert rep is not None
    live.set_calibrator(cal2)
    live.push(ref.series[W + 1])
    got = live.forecast()
    assert same_bits(got, finished(N, W + 2, cal2)) and not same_bits(got, finished(N, W + 2, cal))
    assert live._replay is rep, "same per_step / per_node shape: the offsets are copied into the buffer the graph reads"
    # the calibrator's own tensor was copied, not adopted
    assert live._offsets.data_ptr() != cal2.offsets.data_ptr()
    # present -> absent changes the store's arguments: captured again, at the next forecast
    live.set_calibrator(None)
    live.push(ref.series[W + 2])
    assert same_bits(live.forecast(), sort_q(raw[W + 3]))
    assert live._replay is not None and live._replay is not rep


# ---- 5. restart ---------------------------------------------------------------------------------------------------------------------
def test_restart_from_a_state_dict_continues_bit_for_bit():
    N, cut = 12, 22
    ref, cal = reference(N, "z_score"), calibrator_of(N)
    kw = dict(quant=True, rearrange=True, calibrator=cal)
    whole, resumed, nonempty = make_live(ref, **kw), None, 0
    for t in range(1, T + 1):
        whole.push(ref.series[t - 1])
        if resumed is not None:
            resumed.push(ref.series[t - 1])
            assert resumed.rows == whole.rows == t
            pairs = list(zip(whole.matured(), resumed.matured()))
            for a, b in pairs[:2]:
                assert same_nan_aware(a, b) and a.dtype == b.dtype == torch.float32, t
            assert torch.equal(pairs[2][0], pairs[2][1]) and pairs[2][0].dtype == torch.int64, t
            nonempty += int(pairs[2][0].numel() > 0)
        if t >= W and t % 2 == 0:
            f = whole.forecast()
            assert same_bits(f, finished(N, t, cal)), t
            if resumed is not None:
                assert same_bits(resumed.forecast(), f), t
        if t == cut:
            state = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in whole.state_dict().items()}   # as if read from disk
            resumed = make_live(ref, **kw).load_state_dict(state)
            assert resumed.rows == cut and resumed._origins == whole._origins
    torch.cuda.synchronize()
    assert same_bits(resumed.ring_x, whole.ring_x) and same_nan_aware(resumed.ring_y, whole.ring_y)
    assert torch.equal(resumed.last, whole.last) and same_bits(resumed.out_forecast, whole.out_forecast)
    assert int(resumed.t_dev.item()) == T and nonempty > 5
    with pytest.raises(ValueError, match="history"):
        make_live(ref, **kw).load_state_dict(dict(state, history=HISTORY + 1))


# ---- 6. denormalize ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ("z_score", "min_max"))
def test_denormalized_forecast(method):
    from stemgnn_amd.forecast_dataloader import de_normalized
    N = 11
    ref = reference(N, method)
    live = make_live(ref)
    live.push(ref.series[:W + 3])
    f = live.forecast()
    d = live.forecast(denormalize=True)
    want = de_normalized(f, method, dict(ref.stat))
    assert d.dtype == torch.float64 and tuple(d.shape) == (HORIZON, N) and torch.equal(d, want)
    assert not torch.equal(d, f.double())
