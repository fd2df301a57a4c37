"""GPU: stemgnn_scenario_envelope (csrc/envelope.hip) against the numpy restatement (tests/helpers/envelope_ref.py), bit for bit,
on NaN-filled guarded buffers through the C ABI: the float4 and the scalar path, the tile in LDS and in memory, every optional
argument; edge values, weights, batching; the statistical case of a driftless random walk; and the Python layers end to end on
a tiny quantile model."""
import numpy as np
import pytest
import torch

from tests.helpers import envelope_ref as E
from tests.test_hip_scenario import DEV, GUARD, device_copy, guarded, same_draws, tsame

pytestmark = pytest.mark.gpu
SEED = 20261021
NAN, INF = np.nan, np.inf
KEYS = ("moments", "depth", "chosen", "truth", "bands")


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib
    return _lib.load()


def same64(a, b):
    """float64 arrays: NaN in the same places, the same bits elsewhere"""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def same_outputs(got, want):
    for k in KEYS:
        if (got[k] is None) != (want[k] is None):
            return False
        if got[k] is not None and not (same_draws if k == "bands" else same64)(got[k], want[k]):
            return False
    return True


def guarded64(shape):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), NAN, device=DEV, dtype=torch.float64)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def guards_intact(whole, view):
    lo = (view.data_ptr() - whole.data_ptr()) // whole.element_size()
    return bool(torch.isnan(whole[:lo]).all()) and bool(torch.isnan(whole[lo + view.numel():]).all())


def run_entry(lib, x, coverage, target=None, mult=None, total=0, multiplier=None, ignore_nan=False, depth=True, misalign=False):
    """the C entry on guarded buffers; paths (and bands) start one float off a 16-byte boundary with misalign"""
    count, S, H, C = x.shape
    keep = [device_copy(x, misalign)]
    d_target = d_mult = d_q = None
    if target is not None:
        keep.append(device_copy(target, misalign))
        d_target = keep[-1][1]
    if mult is not None:
        d_mult = torch.from_numpy(np.asarray(mult, np.int32)).to(DEV).contiguous()
    if multiplier is not None:
        d_q = torch.from_numpy(np.asarray(multiplier, np.float64)).to(DEV).contiguous()
    out = dict(moments=guarded64((count, 2, H, C)), depth=guarded64((count, S, C)) if depth else None,
               chosen=guarded64((count, C)), truth=guarded64((count, C)) if target is not None else None,
               bands=guarded((count, 2, H, C), misalign))

    def ptr(v):
        return None if v is None else v.data_ptr()

    def view(k):
        return None if out[k] is None else out[k][1]

    rc = lib.stemgnn_scenario_envelope(keep[0][1].data_ptr(), ptr(d_mult), int(total), ptr(d_target), int(ignore_nan), ptr(d_q),
                                       0 if d_q is None else d_q.numel(), count, S, H, C, float(coverage), ptr(view("moments")),
                                       ptr(view("depth")), ptr(view("chosen")), ptr(view("truth")), ptr(view("bands")),
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    for k in KEYS:
        assert out[k] is None or guards_intact(*out[k]), k
    return {k: None if out[k] is None else out[k][1].cpu().numpy() for k in KEYS}


def without_depth(want):
    return {**want, "depth": None}


# (count, S, H, C): tiles of 4, 8, 8 (five tiles, the last one a single column), 16, 16 (seventeen tiles, the last one part full),
# 4 and 32 (two tiles) columns held in LDS, S beyond a wave and at the limit, and two whose S * H values stay in memory (48 KB
# per column), on the scalar and on the aligned launch
SHAPES = [(1, 1, 1, 1), (3, 5, 4, 7), (2, 64, 12, 33), (2, 65, 3, 32), (1, 130, 2, 260), (1, 1024, 1, 4), (2, 9, 2, 40),
          (1, 300, 40, 5), (2, 300, 40, 8)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_the_entry_matches_the_restatement_bit_for_bit(lib, shape):
    count, S, H, C = shape
    rng = np.random.default_rng(SEED + S * H + C)
    x = (rng.normal(size=shape) * rng.uniform(0.5, 20.0, size=(1, 1, 1, C)) + rng.normal(size=(count, 1, H, C))).astype(np.float32)
    y = (x[:, 0] + rng.normal(size=(count, H, C))).astype(np.float32)
    y[rng.random(y.shape) < 0.2] = NAN                                             # missing readings
    one, each = [1.75], rng.uniform(0.5, 4.0, size=C)
    coverage = 0.4 if S == 1 else 0.7
    # (misaligned, target, ignore_nan, multiplier, depth): every option on either load path
    for mis, tg, ign, q, dep in ((0, None, 0, None, 1), (1, None, 0, None, 0), (0, y, 0, None, 0), (1, y, 1, None, 1),
                                 (0, y, 1, one, 1), (1, y, 0, each, 0), (0, None, 0, each, 1), (1, None, 0, one, 0)):
        want = E.envelope(x, coverage, target=tg, multiplier=q, ignore_nan=bool(ign))
        got = run_entry(lib, x, coverage, target=tg, multiplier=q, ignore_nan=ign, depth=bool(dep), misalign=bool(mis))
        assert same_outputs(got, want if dep else without_depth(want)), (mis, tg is not None, ign, q is not None, dep)
    assert np.isfinite(want["chosen"]).all()
    want = E.envelope(x, 0.9, target=y)                                            # another rank; k > T at S <= 8
    assert same_outputs(run_entry(lib, x, 0.9, target=y), want)


def test_edge_values(lib):
    count, S, H, C = 2, 6, 3, 8
    rng = np.random.default_rng(SEED + 1)
    x = rng.normal(size=(count, S, H, C)).astype(np.float32)
    y = rng.normal(size=(count, H, C)).astype(np.float32)
    x[:, :, 1, :4] = x[:, :1, 1, :4]                                               # step 1 of columns 0 .. 3: all paths equal
    y[:, 1, :2] = x[:, 0, 1, :2]                                                   # the truth on the centre, and off it (2, 3)
    x[0, 2, 0, 5] = NAN                                                            # one NaN, one +inf: that column alone
    x[1, 4, 2, 6] = INF
    y[0, 0, 4] = y[1, 2, 4] = NAN                                                  # some steps missing, and all
    y[:, :, 7] = NAN
    for ign in (False, True):
        want = E.envelope(x, 0.7, target=y, ignore_nan=ign)
        for mis in (False, True):
            got = run_entry(lib, x, 0.7, target=y, ignore_nan=ign, misalign=mis)
            assert same_outputs(got, want)
        assert (got["moments"][:, 1, 1, :4] == 0.0).all()
        assert np.isfinite(got["truth"][:, :2]).all() and (got["truth"][:, 2:4] == INF).all()
        gone = np.zeros((count, C), bool)
        gone[0, 5] = gone[1, 6] = True
        for k in ("moments", "bands"):
            assert np.array_equal(np.isnan(got[k]).all(axis=(1, 2)), gone) and np.array_equal(np.isnan(got[k]).any(axis=(1, 2)), gone)
        assert np.array_equal(np.isnan(got["depth"]).any(axis=1), gone) and np.array_equal(np.isnan(got["chosen"]), gone)
        missing = gone.copy()
        missing[:, 7] = True
        if not ign:
            missing[:, 4] = True
        assert np.array_equal(np.isnan(got["truth"]), missing)
    # S = 1: every scale is 0, the one path has depth 0 and is its own band; the truth is inside only where it is the path
    x, y = x[:, :1, :, :4].copy(), y[:, :, :4].copy()
    y[0, :, 0] = x[0, 0, :, 0]
    got = run_entry(lib, x, 0.4, target=y)
    assert same_outputs(got, E.envelope(x, 0.4, target=y))
    assert (got["moments"][:, 1] == 0.0).all() and (got["depth"] == 0.0).all() and (got["chosen"] == 0.0).all()
    assert np.array_equal(got["bands"][:, 0], x[:, 0]) and np.array_equal(got["bands"][:, 1], x[:, 0])
    assert got["truth"][0, 0] == 0.0 and (got["truth"].ravel()[1:] == INF).all()
    got = run_entry(lib, x, 0.9)                                                   # k = 2 > 1: the whole line
    assert (got["chosen"] == INF).all() and (got["bands"][:, 0] == -INF).all() and (got["bands"][:, 1] == INF).all()
    want = E.envelope(x, 0.9, multiplier=[INF])                                    # a calibrator's +inf over a scale of 0
    assert same_outputs(run_entry(lib, x, 0.9, multiplier=[INF]), want) and (want["bands"][:, 1] == INF).all()


def envelope_np(paths, coverage, **kw):
    """ops.scenario_envelope on host arrays -> numpy outputs"""
    from stemgnn_amd import ops
    dev = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v)).to(DEV)) for k, v in kw.items()
           if k in ("target", "mult", "multiplier")}
    rest = {k: v for k, v in kw.items() if k not in dev}
    out = ops.scenario_envelope(torch.from_numpy(paths).to(DEV), coverage, return_depth=True, **dev, **rest)
    return {k: None if out[k] is None else out[k].cpu().numpy() for k in KEYS}


def test_weights(lib):
    rng = np.random.default_rng(SEED + 2)
    count, K, H, C = 3, 9, 4, 7
    x = rng.normal(size=(count, K, H, C)).astype(np.float32)
    y = rng.normal(size=(count, H, C)).astype(np.float32)
    mult = rng.integers(0, 9, size=(count, K)).astype(np.int32)
    mult[:, 0] += 100 - mult.sum(axis=1).astype(np.int32)
    mult[1, 3] = 0
    mult[1, 0] += 100 - mult[1].sum()
    for mis in (False, True):
        got = run_entry(lib, x, 0.8, target=y, mult=mult, total=100, misalign=mis)
        assert same_outputs(got, E.envelope(x, 0.8, target=y, mult=mult, total=100))
    assert np.isnan(got["depth"][1, 3]).all() and not np.isnan(got["depth"][1, :3]).any()
    # weights where the S * H values stay in memory (48 KB per column): a member of weight 0, NaN-filled, is skipped by every
    # phase; a non-finite value in a member of positive weight makes its column alone absent
    for shape in ((1, 300, 40, 5), (2, 300, 40, 8)):
        xs = rng.normal(size=shape).astype(np.float32)
        ys = rng.normal(size=(shape[0], 40, shape[3])).astype(np.float32)
        ms = rng.integers(0, 4, size=(shape[0], 300)).astype(np.int32)
        ms[:, 7], ms[:, 11], ms[:, 0] = 0, 2, 0
        ms[:, 0] = (1000 - ms.sum(axis=1)).astype(np.int32)
        xs[:, 7] = NAN
        xs[0, 11, 3, 2] = INF
        assert (ms.sum(axis=1) == 1000).all() and (ms[:, 0] > 0).all()
        want = E.envelope(xs, 0.8, target=ys, mult=ms, total=1000)
        for mis in (False, True):
            assert same_outputs(run_entry(lib, xs, 0.8, target=ys, mult=ms, total=1000, misalign=mis), want)
        assert np.isnan(want["chosen"][0, 2]) and np.isnan(want["chosen"]).sum() == 1
    # integer-valued paths, total 64: every sum is exact, so the weighted call is the unweighted call on the replicated ensemble
    K = 10
    xi = rng.integers(-8, 9, size=(2, K, H, 8)).astype(np.float32)
    yi = rng.integers(-8, 9, size=(2, H, 8)).astype(np.float32)
    mi = np.array([[6, 0, 7, 9, 1, 13, 8, 5, 4, 11], [1, 1, 1, 1, 1, 1, 1, 1, 55, 1]], np.int32)
    assert (mi.sum(axis=1) == 64).all()
    full = np.stack([np.repeat(xi[c], mi[c], axis=0) for c in range(2)])
    for q in (None, [2.5]):
        weighted = envelope_np(xi, 0.9, target=yi, mult=mi, total=64, multiplier=q)
        assert same_outputs(weighted, E.envelope(xi, 0.9, target=yi, mult=mi, total=64, multiplier=q))
        replicated = envelope_np(full, 0.9, target=yi, multiplier=q)
        for k in ("moments", "chosen", "truth"):
            assert same64(weighted[k], replicated[k]), k
        assert same_draws(weighted["bands"], replicated["bands"])
        for c in range(2):
            first = np.concatenate([[0], np.cumsum(mi[c])[:-1]])
            live = mi[c] > 0
            assert same64(weighted["depth"][c][live], replicated["depth"][c][first[live]])
    # a member of weight 0 is never read
    ok = envelope_np(xi, 0.9, target=yi, mult=mi, total=64)
    poisoned = xi.copy()
    poisoned[0, 1] = NAN
    assert mi[0, 1] == 0 and same_outputs(envelope_np(poisoned, 0.9, target=yi, mult=mi, total=64), ok)
    # negative weights, or a wrong sum: that origin is absent, the other as it was
    for change in ((0, -1), (9, 12)):
        bad = mi.copy()
        bad[0, change[0]] = change[1]
        if change[1] < 0:
            bad[0, 2] += 1 + mi[0, 0]                                              # the sum is still 64
            assert bad[0].sum() == 64
        got = envelope_np(xi, 0.9, target=yi, mult=bad, total=64)
        assert same_outputs(got, E.envelope(xi, 0.9, target=yi, mult=bad, total=64))
        for k in KEYS:
            assert np.isnan(got[k][0]).all() and (same_draws if k == "bands" else same64)(got[k][1], ok[k][1]), k


def test_batches_join_to_the_whole():
    rng = np.random.default_rng(SEED + 3)
    x = rng.normal(size=(6, 33, 5, 12)).astype(np.float32)
    y = rng.normal(size=(6, 5, 12)).astype(np.float32)
    whole = envelope_np(x, 0.9, target=y)
    again = envelope_np(x, 0.9, target=y)
    parts = [envelope_np(x[lo:hi], 0.9, target=y[lo:hi]) for lo, hi in ((0, 3), (3, 6))]
    joined = {k: np.concatenate([p[k] for p in parts]) for k in KEYS}
    assert same_outputs(joined, whole) and same_outputs(again, whole)
    assert same_outputs(whole, E.envelope(x, 0.9, target=y))


def test_the_statistical_case():
    """A driftless random walk, 4096 origins of 32 exchangeable paths over 8 steps, one column, coverage 0.9.  Every figure is
    the restatement's exactly; the conditions were fixed on the restatement alone, over six seeds: the pointwise band
    between ranks 2 and 31 holds the whole trajectory < 0.70 of the time (0.609-0.619); the ensemble's own multiplier holds it
    in [0.82, 0.895] (0.860-0.876); the multiplier fitted on the first half holds it within 0.025 of 0.9 on the second half
    (0.884-0.903; 3.8 binomial standard deviations at 2048 rows) and >= 0.95 at every single step (0.966-0.978)."""
    from stemgnn_amd import math_utils, ops
    paths, y = E.random_walk_case(SEED)
    want = E.statistical_figures(paths, y)
    d_paths, d_y = torch.from_numpy(paths).to(DEV), torch.from_numpy(y).to(DEV)
    ordered = ops.scenario_bands(d_paths, [2 / 32, 31 / 32], 0, torch.empty(4096, 2, 8, 1, device=DEV))
    assert ops.scenario_rank(2 / 32, 32) == 2 and ops.scenario_rank(31 / 32, 32) == 31
    pointwise = math_utils.joint_coverage(d_y, ordered[:, 0], ordered[:, 1])
    own = math_utils.simultaneous_bands(d_paths, 0.9, target=d_y)
    ensemble = own.joint_coverage()[0]
    half = 2048
    cal = math_utils.EnvelopeCalibrator(0.9).fit(own.truth[:half])
    fresh = math_utils.simultaneous_bands(d_paths[half:], 0.9, target=d_y[half:], calibrator=cal)
    calibrated, column = fresh.joint_coverage()
    inside = (d_y[half:] >= fresh.bands[:, 0]) & (d_y[half:] <= fresh.bands[:, 1])
    per_step = float(inside.double().mean(dim=(0, 2)).min())
    got = (pointwise, ensemble, calibrated, per_step, float(cal.multiplier))
    print(f"pointwise {pointwise:.4f}, ensemble {ensemble:.4f}, calibrated {calibrated:.4f}, lowest step {per_step:.4f}, "
          f"multiplier {got[4]:.4f}; restatement {want}")
    assert got == want and column.tolist() == [calibrated]
    assert calibrated == math_utils.joint_coverage(d_y[half:], fresh.bands[:, 0], fresh.bands[:, 1])
    assert pointwise < 0.70 and 0.82 <= ensemble <= 0.895 and abs(calibrated - 0.9) <= 0.025 and per_step >= 0.95
    assert fresh.width().shape == (8,) and bool((fresh.width()[1:] > fresh.width()[:-1]).all())


def same_envelopes(a, b):
    names = ("bands", "moments", "chosen", "multiplier", "truth", "depth")
    return all((getattr(a, n) is None) == (getattr(b, n) is None) for n in names) and \
        all(getattr(a, n) is None or tsame(getattr(a, n), getattr(b, n)) for n in names)


def test_envelopes_of_a_model_end_to_end():
    from stemgnn_amd import (EnvelopeCalibrator, EventSpec, LiveForecaster, Model, PathEnvelope, ScenarioSet, reduce_scenarios,
                             simultaneous_bands, trainer)
    N, W, L, TAUS, HOR = 7, 4, 2, (0.1, 0.5, 0.9), 4
    torch.manual_seed(SEED)
    model = Model(N, 2, W, 2, horizon=L, quantiles=TAUS).to(DEV).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(5, W, N, generator=g).to(DEV)
    y = torch.randn(5, HOR, N, generator=g).to(DEV)
    graph = model.latent_graph(x)
    whole, split = [(x, y)], [(x[:2], y[:2]), (x[2:], y[2:])]
    kw = dict(paths=8, seed=11, adjacency=graph)
    bands0, target0, paths0 = trainer.rolling_scenarios(model, whole, HOR, return_paths=True, **kw)
    spec = EventSpec(0.0, groups=[[0, 1, 2], [3, 4, 5, 6]])
    fitted = EnvelopeCalibrator(0.8).fit(simultaneous_bands(paths0, 0.8, target=target0))
    assert bool(torch.isfinite(fitted.multiplier).all())
    for how in (dict(), dict(on=spec), dict(calibrator=fitted), dict(ignore_nan=True)):
        want = simultaneous_bands(paths0, 0.8, target=target0, **how)
        assert isinstance(want, PathEnvelope) and want.count == 5 and want.C == (2 if "on" in how else N)
        for loader in (whole, split):                                            # 5 windows at once == 2 + 3
            b, t, got = trainer.scenario_envelopes(model, loader, HOR, 0.8, **kw, **how)
            assert tsame(b, bands0) and tsame(t, target0) and same_envelopes(got, want)
    # on=spec: the band of the corridor means, of the paths and of the target
    want = simultaneous_bands(spec.aggregate(paths0), 0.8, target=spec.aggregate(target0))
    assert same_envelopes(simultaneous_bands(paths0, 0.8, on=spec, target=target0), want)
    assert same_envelopes(simultaneous_bands(paths0, 0.8, on=spec.aggregate(paths0), target=spec.aggregate(target0)), want)
    # a ScenarioSet enters with its counts as weights
    kept = reduce_scenarios(paths0, 3)
    assert isinstance(kept, ScenarioSet)
    got = kept.envelope(0.8, target=target0, return_depth=True)
    full = torch.stack([torch.repeat_interleave(kept.paths[c], kept.counts[c].long(), dim=0) for c in range(5)])
    want = simultaneous_bands(full, 0.8, target=target0)
    assert got.depth.shape == (5, 3, N) and torch.allclose(got.center, want.center, rtol=1e-12, atol=1e-12)
    assert torch.allclose(got.truth, want.truth, rtol=1e-9, atol=1e-9)
    # the live forecaster: the same call on its own paths, and nothing of the serving state moves
    live = LiveForecaster(model, W, HOR, history=4, adjacency=graph)
    live.push(np.random.default_rng(SEED + 3).normal(size=(W + 2, N)))
    live.seed = 21
    before = live.forecast()
    for how in (dict(), dict(on=spec), dict(calibrator=fitted)):
        got = live.envelope(0.8, paths=8, **how)
        want = simultaneous_bands(live.scenarios(paths=8, return_paths=True)[1][None], 0.8, **how)
        assert got.count == 1 and got.truth is None and same_envelopes(got, want)
    assert tsame(live.forecast(), before)
    # score_forecast: exactly three more keys
    plain = trainer.score_forecast(bands0, target0, quantiles=TAUS, paths=paths0)
    for envelope in (0.8, fitted):
        scored = trainer.score_forecast(bands0, target0, quantiles=TAUS, paths=paths0, envelope=envelope)
        assert set(scored) - set(plain) == {"joint_coverage", "joint_coverage_pointwise", "envelope_width"}
        assert set(plain) <= set(scored)
        env = simultaneous_bands(paths0, 0.8, target=target0, calibrator=None if envelope == 0.8 else fitted)
        assert scored["joint_coverage"] == env.joint_coverage()[0]
        assert np.array_equal(scored["envelope_width"], env.width().cpu().numpy()) and scored["envelope_width"].shape == (HOR,)
        lo, hi = bands0[:, 0], bands0[:, 2]
        want = float(((target0 >= lo) & (target0 <= hi)).all(dim=1).double().mean())
        assert scored["joint_coverage_pointwise"] == want
    # missing readings: both shares are taken over the same pairs, whichever way the NaN steps are treated
    holed = target0.clone()
    holed[0, 1, 2] = holed[3, 0, 5] = float("nan")
    holed[4, :, 6] = float("nan")
    for ign in (False, True):
        scored = trainer.score_forecast(bands0, holed, quantiles=TAUS, paths=paths0, envelope=0.8, ignore_nan=ign)
        env = simultaneous_bands(paths0, 0.8, target=holed, ignore_nan=ign)
        judged = ~torch.isnan(env.truth)
        assert int(judged.sum()) == 5 * N - (1 if ign else 3)
        assert scored["joint_coverage"] == float((env.inside & judged).sum()) / float(judged.sum())
        step_in = ((holed >= bands0[:, 0]) & (holed <= bands0[:, 2])) | torch.isnan(holed)
        assert scored["joint_coverage_pointwise"] == float((step_in.all(dim=1) & judged).sum()) / float(judged.sum())
