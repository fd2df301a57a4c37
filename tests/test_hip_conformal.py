"""GPU: conformal calibration of quantile bands (csrc/conformal.hip, math_utils.ConformalCalibrator, the trainer plumbing)
against the numpy restatement of its definition (tests/helpers/conformal_ref.py).  The offset is a k-th smallest fp32 value, so
every offset comparison is equality as numbers (np.array_equal: inf == inf, -0 == +0) and the counts are equal -- no tolerance
anywhere."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests.helpers.conformal_ref import apply_np, fit_np, rank, scores_np  # the definition, in numpy

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = np.float32(np.inf)
GROUPINGS = ((True, False), (False, False), (True, True), (False, True))          # (per_step, per_node)
LEVELS = {2: (0.1, 0.9), 3: (0.1, 0.5, 0.9), 5: (0.05, 0.25, 0.5, 0.75, 0.95)}


def pairs_of(quantiles):
    Q = len(quantiles)
    pairs = tuple((i, Q - 1 - i) for i in range(Q // 2))
    return pairs, [float(quantiles[hi]) - float(quantiles[lo]) for lo, hi in pairs]


# ---- helpers ----------------------------------------------------------------------------------------------------------------
def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def fit_gpu(y, f, pairs, coverage, per_step, per_node, masked):
    from stemgnn_amd import ops
    off, cnt = ops.conformal_fit(dev(y), dev(f), pairs, coverage, per_step, per_node, ignore_nan=masked)
    assert off.dtype == torch.float32 and cnt.dtype == torch.int64
    return off.cpu().numpy(), cnt.cpu().numpy()


def check_fit(y, f, pairs, coverage, per_step, per_node, masked, what=""):
    want_off, want_cnt = fit_np(y, f, pairs, coverage, per_step, per_node, masked)
    off, cnt = fit_gpu(y, f, pairs, coverage, per_step, per_node, masked)
    tag = (what, y.shape, per_step, per_node, masked)
    assert off.shape == want_off.shape and cnt.shape == want_cnt.shape, tag
    assert np.array_equal(cnt, want_cnt), tag
    assert not np.isnan(off).any(), tag
    assert np.array_equal(off, want_off), (tag, off.ravel()[:8], want_off.ravel()[:8])
    return off, cnt


def random_case(count, H, N, Q, seed, nan_share=0.0):
    rng = np.random.default_rng(seed)
    y = rng.normal(size=(count, H, N)).astype(np.float32) * (1 + np.arange(H, dtype=np.float32))[None, :, None]
    centre = (0.5 * y + rng.normal(size=y.shape).astype(np.float32) * 0.5)[:, None]
    half = np.sort(np.abs(rng.normal(size=(count, Q, H, N))).astype(np.float32), axis=1)
    f = (centre + half - half.mean(axis=1, keepdims=True)).astype(np.float32)      # Q rows, non-decreasing in q
    if nan_share:
        y[rng.random(y.shape) < nan_share] = np.nan
        y[:, H - 1, N // 2] = np.nan                              # one (h, n) column with no valid target at all
    return y, f


# ---- 1. random data -------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1, 1), (5, 2, 3), (257, 3, 7), (1000, 1, 33), (64, 3, 65), (2049, 2, 5))


@pytest.mark.parametrize("Q", (2, 3, 5))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fit_on_random_data_equals_numpy(shape, Q):
    count, H, N = shape
    pairs, coverage = pairs_of(LEVELS[Q])
    for masked in (False, True):
        y, f = random_case(count, H, N, Q, seed=count + 7 * Q, nan_share=0.1 if masked else 0.0)
        for per_step, per_node in GROUPINGS:
            off, cnt = check_fit(y, f, pairs, coverage, per_step, per_node, masked, f"Q{Q}")
            if masked and per_step and per_node:                  # the all-NaN column is a group of its own: empty, +inf
                assert (cnt[:, H - 1, N // 2] == 0).all() and np.isposinf(off[:, H - 1, N // 2]).all()
        if not masked and count > 1:
            # unmasked NaN targets count, as +inf
            y2 = y.copy()
            y2[0] = np.nan
            check_fit(y2, f, pairs, coverage, True, False, False, "nan targets counted")


# ---- 2. chosen scores -------------------------------------------------------------------------------------------------------
def key_sets(m, rng):
    """with f_lo = -inf and f_hi = 0 the score is the target itself (y - 0), so these ARE the scores"""
    sets = {
        "top24": (1.0 + np.arange(m, dtype=np.float64) * 2.0 ** -23).astype(np.float32)[rng.permutation(m)],
        "three": rng.choice(np.array([-2.5, 0.75, 3.0], np.float32), m),
        "zeros": rng.choice(np.array([0.0, -0.0], np.float32), m),
        "zeros_mixed": rng.choice(np.array([0.0, -0.0, -1.0, 1.0], np.float32), m),
        "subnormal": rng.choice(np.array([1e-40, -1e-40, 0.0], np.float32), m),
        "inf": rng.choice(np.array([np.inf, -np.inf, 0.5, -0.5], np.float32), m),
        "posinf": rng.choice(np.array([np.inf, 0.5, -0.5], np.float32), m),
        "negative": (-1e30 * (1.0 + rng.random(m))).astype(np.float32),
    }
    sets["negative"][0] = np.float32(-3e38)
    return sets


@pytest.mark.parametrize("m", (1, 2, 255, 256, 257, 4097))
def test_fit_on_chosen_scores(m):
    rng = np.random.default_rng(m)
    sets = key_sets(m, rng)
    # three pairs of a Q = 6 forecast, all (-inf, 0): one call selects rank 1, rank m and rank m + 1 (= +inf)
    pairs = ((0, 5), (1, 4), (2, 3))
    coverage = [1e-6, (m - 0.5) / (m + 1), 1 - 1e-9]
    assert [rank(m, c) for c in coverage] == [1, m, m + 1]
    names = list(sets)
    cols = np.stack([sets[k] for k in names], axis=1)             # [m, sets]: every key set is one node
    S = cols.shape[1]

    def forecast(count, H, N):
        f = np.zeros((count, 6, H, N), np.float32)
        f[:, :3] = -np.inf
        return f

    # per group: every key set a group of exactly m (node groups; the same with the sets laid along the horizon axis)
    y = cols.reshape(m, 1, S)
    off, cnt = check_fit(y, forecast(m, 1, S), pairs, coverage, False, True, False, "sets as nodes")
    assert (cnt == m).all() and np.isposinf(off[2]).all()
    check_fit(y, forecast(m, 1, S), pairs, coverage, True, True, False, "sets as nodes, per step")
    yh = cols.reshape(m, S, 1)
    check_fit(yh, forecast(m, S, 1), pairs, coverage, True, False, False, "sets as steps")
    check_fit(yh, forecast(m, S, 1), pairs, coverage, True, True, False, "sets as steps and nodes")
    # pooled: one group of exactly m per key set, through the streaming form; and folded [m / 1, 1, 1] vs [1, 1, m]
    for k in names:
        for shape in ((m, 1, 1), (1, 1, m), (1, m, 1)):
            yk = sets[k].reshape(shape)
            off, cnt = check_fit(yk, forecast(*shape), pairs, coverage, False, False, False, k)
            assert cnt.ravel().tolist() == [m, m, m]
    # and everything pooled into one group of S * m, ranks 1, S*m, S*m + 1
    M = S * m
    pooled_cov = [1e-6, (M - 0.5) / (M + 1), 1 - 1e-9]
    assert [rank(M, c) for c in pooled_cov] == [1, M, M + 1]
    check_fit(y, forecast(m, 1, S), pairs, pooled_cov, False, False, False, "all sets pooled")
    check_fit(y, forecast(m, 1, S), pairs, pooled_cov, True, False, False, "all sets pooled per step")


# ---- 3. NaN rules -----------------------------------------------------------------------------------------------------------
def test_nan_rules():
    pairs, coverage = ((0, 1),), [0.5]
    y = np.array([0.0, 1.0, 2.0, 3.0, 4.0], np.float32).reshape(5, 1, 1)
    f = np.zeros((5, 2, 1, 1), np.float32)
    f[:, 0] = -np.inf                                             # scores 0 .. 4; k = ceil(6 * .5) = 3 -> 2.0
    for grouping in GROUPINGS:
        off, cnt = check_fit(y, f, pairs, coverage, *grouping, False)
        assert off.item() == 2.0 and cnt.item() == 5
    # a NaN forecast on a valid target counts and sorts last: scores 0, inf, 2, 3, 4 -> third smallest is 3.0
    f1 = f.copy()
    f1[1, 1] = np.nan
    for masked in (False, True):
        for grouping in GROUPINGS:
            off, cnt = check_fit(y, f1, pairs, coverage, *grouping, masked)
            assert off.item() == 3.0 and cnt.item() == 5
    f2 = f1.copy()
    f2[0, 0] = np.nan                                             # the low row as well: scores inf, inf, 2, 3, 4 -> 4.0
    off, cnt = check_fit(y, f2, pairs, coverage, True, False, False)
    assert off.item() == 4.0 and cnt.item() == 5
    # a NaN target: left out under masked (scores 1, 2, 3, 4; k = ceil(5 * .5) = 3 -> 3.0), +inf and counted without
    y1 = y.copy()
    y1[0] = np.nan
    for grouping in GROUPINGS:
        off, cnt = check_fit(y1, f, pairs, coverage, *grouping, True)
        assert off.item() == 3.0 and cnt.item() == 4
        off, cnt = check_fit(y1, f, pairs, coverage, *grouping, False)
        assert off.item() == 3.0 and cnt.item() == 5              # 1, 2, 3, 4, inf -> the third is 3.0
    y2 = np.full((5, 1, 1), np.nan, np.float32)
    for grouping in GROUPINGS:
        off, cnt = check_fit(y2, f, pairs, coverage, *grouping, True)
        assert np.isposinf(off).all() and cnt.item() == 0         # m = 0: the band becomes the whole line
        off, cnt = check_fit(y2, f, pairs, coverage, *grouping, False)
        assert np.isposinf(off).all() and cnt.item() == 5


# ---- 4 / 5. the C entry itself: scratch garbage, repeatability, guarded buffers ---------------------------------------------
GUARD = 64                                                        # sentinel elements either side


def raw_fit(y, f, pairs, coverage, per_step, per_node, masked, scratch_byte):
    """stemgnn_conformal_fit on caller-made buffers: the scratch pre-filled with one byte value, offsets and counts inside
    sentinel-filled allocations.  Returns (offsets, counts) after checking the sentinels."""
    from stemgnn_amd import _lib
    lib = _lib.load()
    C, H, N = y.shape
    Q, P = f.shape[1], len(pairs)
    shape = (P, H if per_step else 1, N if per_node else 1)
    n = int(np.prod(shape))
    nbytes = lib.stemgnn_conformal_scratch_bytes(C, H, N, P, int(per_step), int(per_node))
    assert nbytes > 0
    scratch = torch.full((nbytes + 2 * GUARD,), scratch_byte, dtype=torch.uint8, device=DEV)
    off_buf = torch.full((n + 2 * GUARD,), -777.25, dtype=torch.float32, device=DEV)
    cnt_buf = torch.full((n + 2 * GUARD,), -777, dtype=torch.int64, device=DEV)
    yd, fd = dev(y), dev(f)
    lo = (ctypes.c_int * P)(*[p[0] for p in pairs])
    hi = (ctypes.c_int * P)(*[p[1] for p in pairs])
    cov = (ctypes.c_double * P)(*coverage)
    rc = lib.stemgnn_conformal_fit(yd.data_ptr(), fd.data_ptr(), C, Q, H, N, P, lo, hi, cov, int(per_step), int(per_node),
                                   int(masked), scratch.data_ptr() + GUARD, off_buf.data_ptr() + 4 * GUARD,
                                   cnt_buf.data_ptr() + 8 * GUARD, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for buf, fill in ((off_buf, -777.25), (cnt_buf, -777), (scratch, scratch_byte)):
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[-GUARD:] == fill).all())
    return off_buf[GUARD:GUARD + n].reshape(shape).cpu().numpy(), cnt_buf[GUARD:GUARD + n].reshape(shape).cpu().numpy()


@pytest.mark.parametrize("grouping", GROUPINGS, ids=lambda g: f"step{int(g[0])}node{int(g[1])}")
def test_scratch_garbage_repeatability_and_guards(grouping):
    count, H, N, Q = 300, 3, 37, 5
    pairs, coverage = pairs_of(LEVELS[Q])
    for masked in (False, True):
        y, f = random_case(count, H, N, Q, seed=99, nan_share=0.1 if masked else 0.0)
        want = fit_np(y, f, pairs, coverage, *grouping, masked)
        runs = [raw_fit(y, f, pairs, coverage, *grouping, masked, fill) for fill in (0xFF, 0x00, 0xFF)]
        for off, cnt in runs:
            assert np.array_equal(off, want[0]) and np.array_equal(cnt, want[1])
            assert off.tobytes() == runs[0][0].tobytes() and cnt.tobytes() == runs[0][1].tobytes()


# ---- 6. apply -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", (1, 3, 4, 65, 68))
def test_apply_equals_numpy_bit_for_bit(N):
    from stemgnn_amd import ops
    count, H = 9, 3
    for Q in (2, 3, 5):
        pairs, _ = pairs_of(LEVELS[Q])
        rng = np.random.default_rng(N * 10 + Q)
        f = rng.normal(size=(count, Q, H, N)).astype(np.float32)
        f[0, 0, 0, 0] = np.nan                                    # NaN forecasts stay NaN
        f[1, Q - 1, H - 1, N - 1] = np.nan
        f.view(np.uint32)[2, Q // 2, 1, 0] = 0x7fc01234           # a NaN payload in a row that (for odd Q) is only copied
        for per_step, per_node in GROUPINGS:
            shape = (len(pairs), H if per_step else 1, N if per_node else 1)
            offsets = rng.normal(size=shape).astype(np.float32)   # negative ones shrink the band
            offsets[0, 0, 0] = np.inf
            want = apply_np(f, offsets, pairs, per_step, per_node)
            fd, od = dev(f), dev(offsets)
            got = ops.conformal_apply(fd, od, pairs, per_step, per_node)
            assert got.data_ptr() != fd.data_ptr() and torch.equal(fd.cpu().view(torch.int32), torch.from_numpy(f.view(np.int32)))
            g = got.cpu().numpy()
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(g), nan)
            assert g.view(np.uint32)[~nan].tobytes() == want.view(np.uint32)[~nan].tobytes()
            assert np.isneginf(g[1:, 0, 0, 0]).all() and np.isposinf(g[:, Q - 1, 0, 0]).all()      # the +inf offset
            paired = {r for pr in pairs for r in pr}
            for q in range(Q):
                if q not in paired:                               # rows in no pair: identical bits, payloads included
                    assert g[:, q].tobytes() == f[:, q].tobytes()
            # in place equals out of place, bit for bit
            same = ops.conformal_apply(fd, od, pairs, per_step, per_node, out=fd)
            assert same.data_ptr() == fd.data_ptr()
            assert torch.equal(fd.view(torch.int32), got.view(torch.int32))
            # an unaligned view of a guarded buffer: the scalar path, and nothing written outside
            total = f.size
            buf = torch.full((total + 2 * GUARD + 1,), -777.25, dtype=torch.float32, device=DEV)
            for shift in (0, 1):
                buf.fill_(-777.25)
                out = buf[GUARD + shift:GUARD + shift + total].view(count, Q, H, N)
                ops.conformal_apply(dev(f), od, pairs, per_step, per_node, out=out)
                torch.cuda.synchronize()
                assert torch.equal(out.view(torch.int32), got.view(torch.int32))
                assert bool((buf[:GUARD + shift] == -777.25).all()) and bool((buf[GUARD + shift + total:] == -777.25).all())


# ---- 7. coverage on fresh data ----------------------------------------------------------------------------------------------
def test_coverage_on_fresh_data_and_why_per_step_is_the_default():
    from stemgnn_amd.math_utils import ConformalCalibrator
    from stemgnn_amd.trainer import score_forecast
    taus = (0.1, 0.5, 0.9)
    rng = np.random.default_rng(0)
    count, H, N = 1500, 3, 7
    scale = (1.0 + np.arange(H))[None, :, None]

    def draw():
        return (rng.normal(size=(count, H, N)) * scale).astype(np.float32)

    y_cal, y_new = dev(draw()), dev(draw())
    bands = torch.zeros(count, 3, H, N, device=DEV)
    bands[:, 0], bands[:, 2] = -0.5, 0.5
    per_step = ConformalCalibrator(taus, per_step=True, per_node=False).fit(y_cal, bands)
    assert tuple(per_step.offsets.shape) == (1, H, 1) and per_step.counts.flatten().tolist() == [count * N] * H
    m = score_forecast(bands, y_new, quantiles=taus, calibrator=per_step)
    plain = score_forecast(bands, y_new, quantiles=taus)
    print("raw", m["interval_coverage_raw"], "calibrated", m["interval_coverage"], "offsets", per_step.offsets.flatten().tolist())
    assert float(m["interval_coverage_raw"][0]) < 0.6
    assert np.array_equal(m["interval_coverage_raw"], plain["interval_coverage"])
    assert np.array_equal(m["interval_width_raw"], plain["interval_width"])
    for k in ("mae", "mape", "rmse", "mae_norm", "mae_node", "rmse_node"):          # the point row is untouched
        assert np.array_equal(np.asarray(m[k]), np.asarray(plain[k])), k
    from stemgnn_amd.math_utils import QuantileScores
    by_step = QuantileScores(y_new, per_step.apply(bands), taus).interval_coverage_step[0]
    print("per-step calibrated coverage", by_step)
    assert (np.abs(by_step - 0.8) < 0.03).all(), by_step
    pooled = ConformalCalibrator(taus, per_step=False, per_node=False).fit(y_cal, bands)
    assert tuple(pooled.offsets.shape) == (1, 1, 1) and pooled.counts.item() == count * H * N
    spread = QuantileScores(y_new, pooled.apply(bands), taus).interval_coverage_step[0]
    print("pooled-over-steps calibrated coverage per step", spread)
    assert spread.max() - spread.min() > 0.3, spread


# ---- 8. the in-sample guarantee ---------------------------------------------------------------------------------------------
def on_grid(a):
    """multiples of 2^-6 (all far below 2^10): every fp32 difference and sum of such values is exact"""
    return (np.round(a * 64.0) / 64.0).astype(np.float32)


@pytest.mark.parametrize("grouping", GROUPINGS, ids=lambda g: f"step{int(g[0])}node{int(g[1])}")
def test_in_sample_coverage_is_at_least_nominal(grouping):
    """Calibrating the calibration set itself covers at least nominal in every group with k <= m: at least k elements have
    s <= off, and k / m >= c.  That argument is one of exact arithmetic, so the assertion is made on data whose fp32
    differences are exact (a 2^-6 grid).  On general fp32 data an element whose score TIES with the offset can fall just outside
    its own calibrated band, by the rounding of the round trip f - fl(f - y) (s < off still implies covered: rounding is
    monotone); the numpy restatement shows the same -- 2 of the 128 (grouping, mask, group, pair) cases below lose exactly one
    such element and land at 128/257 and 385/771 of a nominal 0.5.  On such data the test asserts what the kernels owe: every
    element with s < off is covered, and those are at least k minus the ties."""
    from stemgnn_amd.math_utils import ConformalCalibrator, QuantileScores
    per_step, per_node = grouping
    count, H, N, Q = 257, 3, 7, 5
    taus = LEVELS[Q]
    for masked in (False, True):
        for exact in (True, False):
            y, f = random_case(count, H, N, Q, seed=5, nan_share=0.1 if masked else 0.0)
            if masked:
                y[:3, H - 1, N // 2] = [0.125, -0.25, 0.375]      # a group of m = 3: the outer level needs k = 4 > m
            if exact:
                y, f = on_grid(y), on_grid(f)
            yd, fd = dev(y), dev(f)
            cal = ConformalCalibrator(taus, per_step, per_node).fit(yd, fd, ignore_nan=masked)
            out = cal.apply(fd)
            offsets, counts = cal.offsets.cpu().numpy(), cal.counts.cpu().numpy()
            keep = ~np.isnan(y) if masked else np.ones(y.shape, bool)
            checked = 0
            for hg in range(offsets.shape[1]):
                hs = slice(hg, hg + 1) if per_step else slice(None)
                for ng in range(offsets.shape[2]):
                    ns = slice(ng, ng + 1) if per_node else slice(None)
                    qs = QuantileScores(yd[:, hs, ns].contiguous(), out[:, :, hs, ns].contiguous(), taus, ignore_nan=masked)
                    for p, c in enumerate(cal.interval_nominal):
                        m = int(counts[p, hg, ng])
                        k = rank(m, c)
                        tag = (exact, masked, hg, ng, p, m, k, qs.interval_coverage[p])
                        if k > m:
                            assert np.isposinf(offsets[p, hg, ng]) and qs.interval_coverage[p] == 1.0, tag
                            continue
                        assert np.isfinite(offsets[p, hg, ng]) and k / m >= c, tag
                        if exact:
                            assert qs.interval_coverage[p] >= c, tag
                        else:
                            s = scores_np(y, f, *cal.pairs[p])[:, hs, ns][keep[:, hs, ns]]
                            inside = int((s < offsets[p, hg, ng]).sum())
                            assert inside >= k - int((s == offsets[p, hg, ng]).sum()), tag
                            assert round(qs.interval_coverage[p] * m) >= inside, tag
                        checked += 1
            assert checked > 0


# ---- 9. the trainer ---------------------------------------------------------------------------------------------------------
def test_trainer_calibrates_from_the_best_validation_pass(tmp_path):
    from stemgnn_amd import trainer as T
    from stemgnn_amd.forecast_dataloader import ForecastDataset, WindowLoader
    from stemgnn_amd.math_utils import ConformalCalibrator
    taus = (0.1, 0.5, 0.9)
    rng = np.random.default_rng(2024)
    length, N = 400, 16
    t = np.arange(length, dtype=np.float64)[:, None]
    series = np.sin(2 * np.pi * t / rng.uniform(8.0, 30.0, N) + rng.uniform(0.0, 6.28, N)) * rng.uniform(0.5, 3.0, N) \
        + rng.uniform(-2.0, 8.0, N) + 0.3 * rng.normal(size=(length, N))

    def run(out_dir, **kw):
        torch.manual_seed(77)
        tr = T.DeviceTrainer(16, 8, 2, 2, quantiles=taus, batch_size=16, **kw)
        metrics, statistic = tr.fit(series[:300], series[300:], 2, out_dir=out_dir, log=lambda s: None)
        return tr, metrics, statistic

    plain, plain_metrics, _ = run(tmp_path / "plain")
    assert plain.calibrator is None and not (tmp_path / "plain" / "conformal.pt").exists()
    tr, metrics, statistic = run(tmp_path / "cal", calibrate=True)
    assert sorted(metrics) == sorted(plain_metrics)                # validate keeps its return value
    assert "interval_coverage_raw" not in plain_metrics
    cal = tr.calibrator
    assert isinstance(cal, ConformalCalibrator) and cal.per_step and not cal.per_node
    assert tuple(cal.offsets.shape) == (1, 2, 1) and cal.offsets.is_cuda and bool(torch.isfinite(cal.offsets).all())
    assert (tmp_path / "cal" / "conformal.pt").is_file()
    back = T.load_calibrator(tmp_path / "cal", DEV)
    assert torch.equal(back.offsets, cal.offsets) and torch.equal(back.counts, cal.counts)
    assert back.pairs == cal.pairs and back.quantiles == cal.quantiles and (back.per_step, back.per_node) == (True, False)
    assert np.array_equal(back.interval_nominal, cal.interval_nominal)
    # the validation set, forecast by the best model: its calibrated interval coverage is at least nominal
    best = T.load_checkpoint(tmp_path / "cal")
    ds = ForecastDataset(series[300:], window_size=8, horizon=2, normalize_method="z_score", norm_statistic=statistic, device=DEV)
    forecast, target = T.rolling_forecast(best, WindowLoader(ds, batch_size=16), 2)
    refit = ConformalCalibrator(taus).fit(target, forecast)
    assert torch.equal(refit.offsets, cal.offsets) and torch.equal(refit.counts, cal.counts)
    scored = T.score_forecast(forecast, target, "z_score", statistic, quantiles=taus, calibrator=back)
    print("validation: raw", scored["interval_coverage_raw"], "calibrated", scored["interval_coverage"])
    assert float(scored["interval_coverage"][0]) >= float(scored["interval_nominal"][0])
    # trainer.test picks conformal.pt up and reports both; without the file it reports what it always did
    args = types.SimpleNamespace(window_size=8, horizon=2, norm_method="z_score", device=DEV, batch_size=16)
    tested = T.test(series[300:], args, str(tmp_path / "cal"), str(tmp_path / "cal" / "test"))
    assert np.array_equal(tested["interval_coverage"], scored["interval_coverage"])
    assert np.array_equal(tested["interval_coverage_raw"], scored["interval_coverage_raw"])
    untouched = T.test(series[300:], args, str(tmp_path / "plain"), str(tmp_path / "plain" / "test"))
    assert sorted(untouched) == sorted(plain_metrics) and "interval_coverage_raw" not in untouched
    with pytest.raises(ValueError, match="quantile"):
        T.DeviceTrainer(16, 8, 2, 2, calibrate=True)
