"""GPU: the ensemble scores of csrc/ensemble.hip (CRPS, energy score, spread / skill, rank histogram) against the numpy fp64
restatement of their definition (tests/helpers/ensemble_ref.py), and math_utils.EnsembleScores / trainer.score_forecast on top.

Outputs lie inside guarded buffers -- `out` NaN-filled, `hist` sentinel-filled -- and are compared whole.  hist and the counts
[4], [5] are integers and compared exactly.  The bound on [0..3] is derived, not measured: every sum of the definition adds
non-negative terms, so its relative error is at most (n - 1) 2^-53 for n terms; n <= 2^23 at these shapes, 9.4e-10 -- so each
of the two terms of [0] and [1] is within 1e-9 of itself and the statistic within 1e-9 (|first| + |second|); [2] and [3] are
a square root (one more rounding) of one such sum: 1e-9 relative."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import ensemble_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261020
GUARD = 64
SENTINEL = -0x0123456789ABCDEF
RTOL = 1e-9
K = 6


def device_f32(a, misalign):
    """a on the device, 16-byte aligned or 4 bytes off"""
    a = np.ascontiguousarray(a, np.float32)
    whole = torch.zeros(a.size + 8, device=DEV)
    lo = 4 + (1 if misalign else 0)
    view = whole[lo:lo + a.size].view(*a.shape)
    view.copy_(torch.from_numpy(a))
    assert (view.data_ptr() % 16 != 0) == bool(misalign)
    return view


def run_entry(target, paths, mul=None, add=None, masked=False, fair=False, misalign=False):
    """the C entry on guarded buffers -> (out whole, hist whole) as numpy"""
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, S, H, N = paths.shape
    d_t, d_p = device_f32(target, misalign), device_f32(paths, misalign)
    n_out = lib.stemgnn_ensemble_out_doubles(H)
    assert n_out == K * (1 + H)
    out = torch.full((n_out + 2 * GUARD,), float("nan"), dtype=torch.float64, device=DEV)
    hist = torch.full((H * (S + 1) + 2 * GUARD,), SENTINEL, dtype=torch.int64, device=DEV)
    scratch = torch.full((lib.stemgnn_ensemble_scratch_doubles(count, S, H, N),), float("nan"), dtype=torch.float64, device=DEV)
    d_mul = d_add = None
    if mul is not None:
        d_mul, d_add = torch.from_numpy(mul).to(DEV), torch.from_numpy(add).to(DEV)
    entry = lib.stemgnn_ensemble_scores_masked if masked else lib.stemgnn_ensemble_scores
    rc = entry(d_t.data_ptr(), d_p.data_ptr(), d_mul.data_ptr() if mul is not None else None,
               d_add.data_ptr() if mul is not None else None, count, S, H, N, int(fair), scratch.data_ptr(),
               out[GUARD:].data_ptr(), hist[GUARD:].data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_t.cpu().numpy().view(np.uint32), np.ascontiguousarray(target, np.float32).view(np.uint32))
    return out.cpu().numpy(), hist.cpu().numpy()


def check(got_out, got_hist, ref, H, S):
    """the whole buffers against the restatement; prints the worst error over its bound"""
    exp_hist = np.full(got_hist.size, SENTINEL, np.int64)
    exp_hist[GUARD:GUARD + H * (S + 1)] = ref["hist"].reshape(-1)
    assert np.array_equal(got_hist, exp_hist)
    n_out = K * (1 + H)
    assert np.isnan(got_out[:GUARD]).all() and np.isnan(got_out[GUARD + n_out:]).all()
    got, exp = got_out[GUARD:GUARD + n_out], ref["out"]
    worst = 0.0
    for at in range(1 + H):                                                  # 0: overall, 1 + h: step h
        idx = [k if at == 0 else K + k * H + (at - 1) for k in range(K)]
        assert got[idx[4]] == exp[idx[4]] and got[idx[5]] == exp[idx[5]], (at, got[idx], exp[idx])
        for k in range(4):
            g, e = got[idx[k]], exp[idx[k]]
            if np.isnan(e) or np.isinf(e):
                assert (np.isnan(g) and np.isnan(e)) or g == e, (at, k, g, e)
                continue
            bound = RTOL * (abs(ref["first"][k, at]) + abs(ref["second"][k, at])) if k < 2 else RTOL * abs(e)
            assert abs(g - e) <= bound, (at, k, g, e, abs(g - e), bound)
            if bound > 0:
                worst = max(worst, abs(g - e) / bound)
    print(f"worst |error| / bound: {worst:.3e}")
    return got


# (count, S, H, N): count * H * N * S^2 <= 2^23
CASES = [(1, 1, 1, 1), (3, 2, 2, 5), (7, 33, 3, 70), (2, 100, 1, 64), (5, 64, 3, 12), (1, 1024, 1, 8)]
_data, _refs = {}, {}


def case_data(case, masked):
    key = (case, masked)
    if key not in _data:
        count, S, H, N = case
        assert count * H * N * S * S <= 2 ** 23
        rng = np.random.default_rng(SEED + 17 * S + N + (1 if masked else 0))
        target = rng.normal(size=(count, H, N)).astype(np.float32)
        paths = (rng.normal(size=(count, S, H, N)) * 0.8 + 0.1).astype(np.float32)
        if masked and target.size > 1:
            target[rng.random(target.shape) < 0.15] = np.nan
            target.reshape(-1)[0] = np.nan
        mul = rng.uniform(0.5, 40.0, size=N)
        add = rng.normal(size=N) * 100.0
        _data[key] = (target, paths, mul, add)
    return _data[key]


def case_ref(case, masked, fair, denorm):
    key = (case, masked, fair, denorm)
    if key not in _refs:
        target, paths, mul, add = case_data(case, masked)
        _refs[key] = R.scores(target, paths, mul if denorm else None, add if denorm else None, masked=masked, fair=fair)
    return _refs[key]


@pytest.mark.parametrize("denorm", (False, True), ids=("raw", "denorm"))
@pytest.mark.parametrize("fair", (False, True), ids=("biased", "fair"))
@pytest.mark.parametrize("masked", (False, True), ids=("plain", "masked"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_scores_match_the_restatement(case, masked, fair, denorm):
    count, S, H, N = case
    if fair and S < 2:
        from stemgnn_amd import _lib
        target, paths, _, _ = case_data(case, masked)
        entry = _lib.load().stemgnn_ensemble_scores_masked if masked else _lib.load().stemgnn_ensemble_scores
        assert entry(64, 64, None, None, count, S, H, N, 1, 64, 64, 64, None) == -10001     # refused: nothing to compare
        return
    target, paths, mul, add = case_data(case, masked)
    ref = case_ref(case, masked, fair, denorm)
    if S == 1:
        assert np.isnan(ref["out"][3]) and (ref["second"] == 0).all()       # no spread, no pair term
    if masked and target.size > 1:
        assert 0 < ref["out"][4] < target.size
    for misalign in (False, True):
        out, hist = run_entry(target, paths, mul if denorm else None, add if denorm else None, masked, fair, misalign)
        check(out, hist, ref, H, S)


def special_inputs():
    """(target, paths) [4, 5, 3, 6] with ties of the target with one, two and all path values and +0 / -0 ties"""
    rng = np.random.default_rng(SEED + 1)
    count, S, H, N = 4, 5, 3, 6
    target = rng.normal(size=(count, H, N)).astype(np.float32)
    paths = rng.normal(size=(count, S, H, N)).astype(np.float32)
    target[0, 0, 0] = paths[0, 2, 0, 0]                                      # equal to one
    paths[0, 1, 0, 1] = paths[0, 3, 0, 1]
    target[0, 0, 1] = paths[0, 1, 0, 1]                                      # equal to two
    paths[0, :, 0, 2] = 0.75
    target[0, 0, 2] = 0.75                                                   # equal to all
    paths[1, :, 1, 0] = (0.0, -0.0, 0.0, -0.0, 1.0)
    target[1, 1, 0] = -0.0                                                   # four zero ties of both signs
    paths[1, :, 1, 1] = (-0.0, -0.0, -1.0, 2.0, 3.0)
    target[1, 1, 1] = 0.0
    paths[2, :, 2, 3] = paths[2, 0, 2, 3]                                    # all tied, the target elsewhere
    return target, paths


def test_ties_take_the_midrank():
    target, paths = special_inputs()

    def rank(c, h, n):                                                       # what the rule says, by hand
        x, y = paths[c, :, h, n], target[c, h, n]
        return int((x < y).sum() + (x == y).sum() // 2)
    lt = int((paths[0, :, 0, 1] < target[0, 0, 1]).sum())
    assert rank(0, 0, 1) == lt + 1 and rank(0, 0, 2) == 2 and rank(1, 1, 0) == 2 and rank(1, 1, 1) == 2
    for masked in (False, True):
        ref = R.scores(target, paths, masked=masked)
        out, hist = run_entry(target, paths, masked=masked)
        check(out, hist, ref, 3, 5)
        assert ref["hist"].sum() == target.size


def test_missing_targets():
    target, paths = special_inputs()
    target[0, 1, 2] = target[3, 0, 5] = np.nan                               # single nodes
    target[1, 0, :] = np.nan                                                 # every node of one row
    target[:, 2, :] = np.nan                                                 # every element of one step
    mul, add = np.linspace(0.5, 3.0, 6), np.linspace(-5.0, 5.0, 6)
    for fair in (False, True):
        ref = R.scores(target, paths, mul, add, masked=True, fair=fair)
        o = ref["out"]
        assert o[5] == 4 * 2 - 1 and o[4] == 4 * 2 * 6 - 2 - 6               # the row and the step are out
        assert np.isnan(o[K + np.arange(4) * 3 + 2]).all() and o[K + 4 * 3 + 2] == 0 and o[K + 5 * 3 + 2] == 0
        assert np.isfinite(o[:4]).all() and (ref["hist"][2] == 0).all()
        out, hist = run_entry(target, paths, mul, add, masked=True, fair=fair)
        check(out, hist, ref, 3, 5)
    # the plain entry on the same tensors: NaN wherever the definition involves a NaN target, and those have no rank
    ref = R.scores(target, paths, mul, add)
    assert np.isnan(ref["out"][:3]).all() and ref["out"][4] == target.size and ref["hist"].sum() == np.isfinite(target).sum()
    out, hist = run_entry(target, paths, mul, add)
    check(out, hist, ref, 3, 5)


@pytest.mark.parametrize("masked", (False, True), ids=("plain", "masked"))
def test_nan_and_inf_path_values_propagate(masked):
    target, paths = special_inputs()
    paths[0, 3, 0, 4] = np.nan                                               # step 0
    paths[2, 1, 1, 2] = np.inf                                               # step 1; step 2 stays finite
    ref = R.scores(target, paths, masked=masked)
    o = ref["out"]
    assert np.isnan(o[0]) and np.isnan(o[1]) and np.isnan(o[K + 0]) and np.isnan(o[K + 1]) and np.isnan(o[K + 3 + 1])
    assert np.isfinite(o[K + np.arange(4) * 3 + 2]).all()
    assert ref["hist"].sum() == target.size                                  # a rank all the same
    out, hist = run_entry(target, paths, masked=masked)
    check(out, hist, ref, 3, 5)


def test_two_runs_give_the_same_bits():
    case = (7, 33, 3, 70)
    target, paths, mul, add = case_data(case, True)
    a = run_entry(target, paths, mul, add, masked=True, fair=True)
    b = run_entry(target, paths, mul, add, masked=True, fair=True)
    assert np.array_equal(a[0].view(np.uint64), b[0].view(np.uint64)) and np.array_equal(a[1], b[1])


def on_device(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def against_ref(es, ref, H, S):
    """an EnsembleScores object against the restatement, by the rules of check"""
    got = np.concatenate([[es.crps, es.energy, es.rmse, es.spread, es.valid, es.valid_rows],
                          np.concatenate([es.crps_step, es.energy_step, es.rmse_step, es.spread_step,
                                          es.valid_step.astype(np.float64), es.valid_rows_step.astype(np.float64)])])
    whole = np.full(got.size + 2 * GUARD, np.nan)
    whole[GUARD:GUARD + got.size] = got
    hist = np.full(H * (S + 1) + 2 * GUARD, SENTINEL, np.int64)
    hist[GUARD:GUARD + H * (S + 1)] = es.rank_histogram_step.reshape(-1)
    check(whole, hist, ref, H, S)
    assert np.array_equal(es.rank_histogram, ref["hist"].sum(axis=0)) and es.rank_histogram.dtype == np.int64


def test_rank_histogram_of_a_calibrated_and_of_a_narrow_ensemble():
    """3200 ranks over 16 bins; 37.7 = the 0.999 quantile of chi-square with 15 degrees of freedom.  Seed SEED + 2: the
    restatement gives 12.13 for the calibrated ensemble and 2380 for the half-scale one (outer bins 638 and 656, flat 200)."""
    from stemgnn_amd.math_utils import EnsembleScores
    rng = np.random.default_rng(SEED + 2)
    count, S, H, N = 64, 15, 2, 25
    target = rng.normal(size=(count, H, N)).astype(np.float32)
    paths = rng.normal(size=(count, S, H, N)).astype(np.float32)
    narrow = (paths * np.float32(0.5)).astype(np.float32)
    es = EnsembleScores(on_device(target), on_device(paths))
    against_ref(es, R.scores(target, paths), H, S)
    assert es.rank_histogram.sum() == 3200 and es.rank_uniformity_dof == 15
    assert es.rank_uniformity == pytest.approx(R.rank_uniformity(es.rank_histogram), rel=1e-12)
    print(f"calibrated: chi-square {es.rank_uniformity:.2f}, spread / rmse {es.spread / es.rmse:.3f}")
    assert es.rank_uniformity < 37.7
    es = EnsembleScores(on_device(target), on_device(narrow))
    against_ref(es, R.scores(target, narrow), H, S)
    print(f"half scale: chi-square {es.rank_uniformity:.2f}, outer bins {es.rank_histogram[0]}, {es.rank_histogram[-1]}")
    assert es.rank_uniformity > 37.7
    assert es.rank_histogram[0] > 2 * 200 and es.rank_histogram[-1] > 2 * 200


def test_the_energy_score_tells_the_couplings_apart_and_the_crps_does_not():
    """Truth A: one shock per row, repeated over the nodes; truth B: iid per node.  Ensemble P: one normal per path, repeated;
    ensemble I: iid.  Seed SEED + 3, by the restatement: energy(I | A) - energy(P | A) = 0.2078, energy(P | B) -
    energy(I | B) = 0.1975 (the issue's numpy check found 0.20 - 0.24, standard errors at most 0.022; the bound is 0.1), and
    |crps(P | A) - crps(I | A)| = 0.0039, within the issue's 0.05 as it stands."""
    from stemgnn_amd.math_utils import EnsembleScores
    rng = np.random.default_rng(SEED + 3)
    count, S, H, N = 256, 32, 1, 8
    truth_a = np.repeat(rng.normal(size=(count, H, 1)), N, axis=2).astype(np.float32)
    truth_b = rng.normal(size=(count, H, N)).astype(np.float32)
    ens_p = np.repeat(rng.normal(size=(count, S, H, 1)), N, axis=3).astype(np.float32)
    ens_i = rng.normal(size=(count, S, H, N)).astype(np.float32)
    got = {}
    for tn, truth in (("A", truth_a), ("B", truth_b)):
        for en, ens in (("P", ens_p), ("I", ens_i)):
            es = EnsembleScores(on_device(truth), on_device(ens))
            against_ref(es, R.scores(truth, ens), H, S)
            got[en + tn] = es
    margin_a = got["IA"].energy - got["PA"].energy
    margin_b = got["PB"].energy - got["IB"].energy
    crps_gap = abs(got["PA"].crps - got["IA"].crps)
    print(f"energy margins: A {margin_a:.4f}, B {margin_b:.4f}; crps gap on A {crps_gap:.4f}")
    assert got["PA"].energy < got["IA"].energy and margin_a > 0.1
    assert got["IB"].energy < got["PB"].energy and margin_b > 0.1
    assert crps_gap < 0.05


# ---- end to end: a real small quantile model (the one tests/test_hip_scenario.py builds) ----------------------------------
N_E, W_E, H_E, TAUS_E = 9, 12, 3, (0.1, 0.5, 0.9)
OLD_KEYS = {"mae", "mape", "rmse", "mae_node", "mape_node", "rmse_node", "mape_norm", "mae_norm", "rmse_norm", "pinball",
            "pinball_q", "coverage_q", "interval_coverage", "interval_width", "interval_nominal", "crossing"}
NEW_KEYS = {k + s + n for k in ("crps", "energy_score", "ensemble_rmse", "spread") for s in ("", "_step") for n in ("", "_norm")} | \
    {"rank_histogram", "rank_histogram_step"}


def test_scenario_paths_of_a_model_are_scored_end_to_end():
    from stemgnn_amd import Model, trainer
    from stemgnn_amd.math_utils import EnsembleScores
    torch.manual_seed(SEED)
    model = Model(N_E, 2, W_E, 2, horizon=H_E, quantiles=TAUS_E).to(DEV).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(5, W_E, N_E, generator=g).to(DEV)
    y = torch.randn(5, 7, N_E, generator=g).to(DEV)
    graph = model.latent_graph(x)
    bands, target, paths = trainer.rolling_scenarios(model, [(x, y)], 7, paths=16, seed=11, adjacency=graph, return_paths=True)
    t_np, p_np = target.cpu().numpy(), paths.cpu().numpy()
    ref = R.scores(t_np, p_np)
    es = EnsembleScores(target, paths)
    against_ref(es, ref, 7, 16)
    assert np.isfinite(ref["out"]).all() and es.valid == 5 * 7 * N_E and es.valid_rows == 5 * 7
    plain = trainer.score_forecast(bands, target, quantiles=TAUS_E)
    assert set(plain) == OLD_KEYS
    scored = trainer.score_forecast(bands, target, quantiles=TAUS_E, paths=paths)
    assert set(scored) == OLD_KEYS | NEW_KEYS
    for k in OLD_KEYS:
        assert np.array_equal(np.asarray(scored[k]), np.asarray(plain[k])), k
    for key, name in (("crps", "crps"), ("energy_score", "energy"), ("ensemble_rmse", "rmse"), ("spread", "spread")):
        for norm in ("", "_norm"):                                           # no statistic given: raw units are the normalised ones
            assert scored[key + norm] == getattr(es, name)
            assert np.array_equal(scored[key + "_step" + norm], getattr(es, name + "_step"))
    assert np.array_equal(scored["rank_histogram"], es.rank_histogram)
    assert np.array_equal(scored["rank_histogram_step"], es.rank_histogram_step)
    # with a statistic the raw keys are those of the de-normalised values, the *_norm keys stay
    stat = dict(mean=np.linspace(10, 50, N_E).tolist(), std=np.linspace(1, 9, N_E).tolist())
    raw = trainer.score_forecast(bands, target, "z_score", stat, quantiles=TAUS_E, paths=paths, fair=True)
    ref_raw = R.scores(t_np, p_np, np.asarray(stat["std"]), np.asarray(stat["mean"]), fair=True)
    ref_fair = R.scores(t_np, p_np, fair=True)
    for k, key in enumerate(("crps", "energy_score", "ensemble_rmse", "spread")):
        tol = RTOL * (abs(ref_raw["first"][k, 0]) + abs(ref_raw["second"][k, 0])) if k < 2 else RTOL * abs(ref_raw["out"][k])
        assert abs(raw[key] - ref_raw["out"][k]) <= tol, key
        tol = RTOL * (abs(ref_fair["first"][k, 0]) + abs(ref_fair["second"][k, 0])) if k < 2 else RTOL * abs(ref_fair["out"][k])
        assert abs(raw[key + "_norm"] - ref_fair["out"][k]) <= tol, key
    assert np.array_equal(raw["rank_histogram"], es.rank_histogram)
