"""GPU: the step coupling of scenario paths -- stemgnn_copula_uniforms_steps (csrc/copula.hip) against the numpy restatement of
its definition (tests/helpers/steps_copula_ref.py), and math_utils.SpaceTimeCopula / path_energy_score through
ops.scenario_roll, trainer.rolling_scenarios and LiveForecaster.scenarios.

Every output lies inside a NaN-filled buffer with guard words on both sides, compared whole; bit comparisons are
test_hip_scenario.py's same_bits.  The fp64 comparison carries the issue's bound, stated where it is used."""
import numpy as np
import pytest
import torch

from tests.helpers import copula_ref as C
from tests.helpers import steps_copula_ref as T
from tests.test_hip_scenario import DEV, GUARD, KEY, LEVELS, OFFSET, ORIGIN0, SEED, guarded, same_bits, tsame

pytestmark = pytest.mark.gpu
SG_EINVAL = -10001
ALLOW = 16                                   # ulps of allowance for normcdfinvf / normcdff
STEP = 3
STAT_SEED = 7                                # tests/test_steps_copula_ref.py clears the same conditions by numpy at this seed

# (N, Bo, S, L): the smallest shapes that reach every tile form
CASES = [
    (1, 4, 3, 2),                            # 8 paths per tile of 16 rows
    (5, 3, 3, 3),                            # 5 per tile, a pad row, a partial second tile
    (64, 2, 3, 5),                           # 3 per tile
    (257, 2, 2, 16),                         # one path fills the tile; n crosses the 256 threads
    (512, 1, 3, 7),                          # 2 per tile, partial
    (513, 2, 1, 4),                          # the tile of 4 rows: one path per tile
    (2048, 1, 3, 2),                         # the tile of 4 rows: two per tile, partial
    (64, 2, 3, 1),                           # L = 1
]
IDS = ["-".join(str(v) for v in c) for c in CASES]


def nan_above(lower):
    """a float32 copy of a lower triangular matrix with NaN above its diagonal"""
    out = np.array(lower, np.float32)
    out[np.triu_indices(out.shape[0], 1)] = np.nan
    return out


def operands(N, L):
    """(factor [N, N] lower, factor_t on the device with NaN where k > n, step_factor [L, L] with NaN where i > j, on the device)"""
    factor = C.factor_of(T.decay(N, 0.7))
    step_factor = C.factor_of(T.decay(L, 0.8))
    d_f = torch.from_numpy(np.ascontiguousarray(nan_above(factor).T)).to(DEV)
    d_a = torch.from_numpy(nan_above(step_factor)).to(DEV)
    return factor, d_f, step_factor, d_a


def run_steps(lib, d_f, d_a, Bo, S, L, N, origin0=ORIGIN0):
    """the whole guarded buffer after one call of the new entry (d_a None: the existing entry)"""
    step, horizon = STEP, STEP + L + 1
    whole, d_u = guarded((Bo, S, L, N), False)
    if d_a is None:
        rc = lib.stemgnn_copula_uniforms(d_f.data_ptr(), Bo, S, L, N, step, horizon, origin0, KEY, OFFSET, d_u.data_ptr(), None)
    else:
        rc = lib.stemgnn_copula_uniforms_steps(d_f.data_ptr(), d_a.data_ptr(), Bo, S, L, N, step, horizon, origin0, KEY, OFFSET,
                                               d_u.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return whole.cpu().numpy()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_uniforms_steps_match_fp64(case):
    """|u - u*| <= 0.4 (N + L + 16) 2^-24 (|A| |e*| |L|^T) + 4 * 2^-24: the bound of stemgnn_copula_uniforms with the step sum's
    L more roundings -- sequential fp32 sums, max phi = 0.399, 16 ulps for normcdfinvf / normcdff, and u's own rounding."""
    from stemgnn_amd import _lib
    N, Bo, S, L = case
    lib = _lib.load()
    factor, d_f, step_factor, d_a = operands(N, L)
    want, mag = T.uniforms_steps(factor, step_factor, ORIGIN0, Bo, S, STEP + L + 1, STEP, L, KEY, OFFSET)
    got = run_steps(lib, d_f, d_a, Bo, S, L, N)
    inner = got[GUARD:GUARD + want.size].reshape(want.shape)
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + want.size:]).all()      # every guard word is intact
    assert not np.isnan(inner).any() and inner.min() >= C.U_LO and inner.max() <= C.U_HI
    err = np.abs(inner.astype(np.float64) - want)
    bound = 0.4 * (N + L + ALLOW) * 2.0 ** -24 * mag + 4 * 2.0 ** -24
    print(f"N {N} L {L}: worst error / bound {float((err / bound).max()):.4f}, max error {float(err.max()):.3e}")
    assert (err <= bound).all()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_uniforms_steps_bits_do_not_depend_on_the_run_or_the_tile(case):
    from stemgnn_amd import _lib
    N, Bo, S, L = case
    lib = _lib.load()
    _, d_f, _, d_a = operands(N, L)
    got = run_steps(lib, d_f, d_a, Bo, S, L, N)
    assert same_bits(run_steps(lib, d_f, d_a, Bo, S, L, N), got)                 # two runs, the same bits
    size = Bo * S * L * N
    first = Bo // 2 if Bo > 1 else 0                                             # the loader's batching cannot move a draw
    parts = [run_steps(lib, d_f, d_a, b, S, L, N, origin0=ORIGIN0 + at)[GUARD:GUARD + b * S * L * N]
             for at, b in ((0, first), (first, Bo - first)) if b]
    assert same_bits(np.concatenate(parts), got[GUARD:GUARD + size])
    # behind one more origin the same paths land in other rows of other tiles
    two = run_steps(lib, d_f, d_a, Bo + 1, S, L, N, origin0=ORIGIN0 - 1)
    assert same_bits(two[GUARD + S * L * N:GUARD + S * L * N + size], got[GUARD:GUARD + size])


@pytest.mark.parametrize("case", [CASES[1], CASES[3], CASES[5], CASES[7]], ids=[IDS[1], IDS[3], IDS[5], IDS[7]])
def test_identity_steps_give_the_bits_of_the_existing_entry(case):
    from stemgnn_amd import _lib
    N, Bo, S, L = case
    lib = _lib.load()
    _, d_f, _, _ = operands(N, L)
    d_eye = torch.from_numpy(nan_above(np.eye(L))).to(DEV)
    got = run_steps(lib, d_f, d_eye, Bo, S, L, N)
    assert same_bits(got, run_steps(lib, d_f, None, Bo, S, L, N))
    assert not np.isnan(got[GUARD:GUARD + Bo * S * L * N]).any()


def test_refusals_leave_the_output_untouched():
    from stemgnn_amd import _lib
    lib = _lib.load()
    untouched = None
    for N, L, kw in ((64, 17, {}), (513, 5, {}), (2049, 2, {}), (64, 3, dict(null=True)), (64, 3, dict(step=7, horizon=7)),
                     (64, 3, dict(step=8, horizon=7))):
        d_f = torch.zeros(N, N, device=DEV)
        d_a = torch.eye(L, device=DEV)
        null = kw.pop("null", False)
        whole, d_u = guarded((2, 3, L, N), False)
        rc = lib.stemgnn_copula_uniforms_steps(d_f.data_ptr(), None if null else d_a.data_ptr(), 2, 3, L, N, kw.get("step", STEP),
                                               kw.get("horizon", STEP + L + 1), ORIGIN0, KEY, OFFSET, d_u.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == SG_EINVAL, (N, L, kw, null)
        untouched = whole.cpu().numpy()
        assert np.isnan(untouched).all(), (N, L, kw, null)
    assert untouched is not None


def test_ops_copula_uniforms_takes_the_step_factor():
    from stemgnn_amd import _lib, ops
    N, Bo, S, L = CASES[1]
    lib = _lib.load()
    factor, _, step_factor, _ = operands(N, L)
    d_f = torch.from_numpy(np.ascontiguousarray(factor.T)).to(DEV)
    d_a = torch.from_numpy(step_factor).to(DEV)
    u = ops.copula_uniforms(d_f, Bo, S, L, STEP, STEP + L + 1, origin0=ORIGIN0, seed=KEY, offset=OFFSET, step_factor=d_a)
    want = run_steps(lib, d_f, d_a, Bo, S, L, N)[GUARD:GUARD + u.numel()].reshape(u.shape)
    assert same_bits(u.cpu().numpy(), want)
    plain = ops.copula_uniforms(d_f, Bo, S, L, STEP, STEP + L + 1, origin0=ORIGIN0, seed=KEY, offset=OFFSET)
    assert same_bits(plain.cpu().numpy(), run_steps(lib, d_f, None, Bo, S, L, N)[GUARD:GUARD + u.numel()].reshape(u.shape))
    for bad in (d_a[:2, :2].contiguous(), d_a.double(), d_a.cpu(), d_a.T, torch.eye(L + 1, device=DEV)):
        with pytest.raises(_lib.StemGNNHipError, match="step_factor"):
            ops.copula_uniforms(d_f, Bo, S, L, STEP, STEP + L + 1, step_factor=bad)


def test_the_dependence_is_the_one_asked_for():
    from stemgnn_amd.math_utils import SpaceTimeCopula
    r, t = C.block_correlation(16, 8, 0.9), T.decay(3, 0.8)
    cop = SpaceTimeCopula.from_correlations(r, t, LEVELS[3], device=DEV)
    u = cop.uniforms(16, 256, 3, 0, 3, ORIGIN0, KEY).cpu().numpy().reshape(4096, 3, 16)
    assert u.min() >= C.U_LO and u.max() <= C.U_HI
    mean_err = float(np.abs(u.reshape(4096, -1).mean(axis=0) - 0.5).max())
    corr_err = float(np.abs(T.kron_correlation(C.ndtri(u.astype(np.float64))) - np.kron(t, r)).max())
    print(f"max |mean u - 0.5| = {mean_err:.4f} (bound 0.0226), max |corr - T (x) R| = {corr_err:.4f} (bound 0.078)")
    assert mean_err <= 5 * np.sqrt(1 / (12 * 4096))
    assert corr_err <= 5 / np.sqrt(4096)


def test_the_step_coupling_shows_in_the_scores():
    """Truth over 4 steps x 16 nodes with normal scores correlated 0.8^|i-j| (x) (blocks of 8 at 0.9); every forecast is the
    exact N(0, 1) quantile function at seven levels, so only the dependence differs between the two ensembles: the node copula
    alone ("space") and SpaceTimeCopula ("steps"), both fitted on the same 512 rows.  The event: node 0 above 0.5 at all 4 steps.
    The conditions are the issue's, half the smallest margin of its five numpy seeds; by the restatement alone at this seed
    (tests/test_steps_copula_ref.py): whole-trajectory energy 5.5938 / 5.5051, per-step energy 2.6581 / 2.6562, CRPS 0.5808 /
    0.5807, mean odds 0.0098 / 0.1075 at a base rate of 0.1436, Brier 0.1412 / 0.1268, max |T_raw - T_true| 0.0776.  The
    device's figures are printed."""
    from stemgnn_amd import ops
    from stemgnn_amd.math_utils import EnsembleScores, EventSpec, GaussianCopula, SpaceTimeCopula, path_energy_score
    case = T.steps_case(STAT_SEED)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in case.items() if k not in ("R_true", "T_true")}
    count, S, N, L = T.STEPS_NEW, T.STEPS_S, T.STEPS_N, T.STEPS_L
    cops = dict(space=GaussianCopula(T.STEPS_TAUS, shrinkage=0.05).fit(dev["y_fit"], dev["f_fit"]),
                steps=SpaceTimeCopula(T.STEPS_TAUS, shrinkage=0.05).fit(dev["y_fit"], dev["f_fit"]))
    assert tsame(cops["space"].factor_t, cops["steps"].factor_t)                 # the node part is GaussianCopula.fit's
    assert tsame(cops["space"].correlation, cops["steps"].correlation)
    cop = cops["steps"]
    assert cop.steps == L and tuple(cop.step_factor.shape) == (L, L) and int(cop.step_pairs.min()) == T.STEPS_FIT * N
    t_raw = cop.step_correlation_raw.cpu().numpy()
    t_err = float(np.abs(t_raw - case["T_true"]).max())
    assert np.array_equal(cop.step_correlation.cpu().numpy(), t_raw)             # step_shrinkage = 0
    window = torch.zeros(count, L, N, device=DEV)
    spec = EventSpec(T.STEPS_THRESHOLD, min_run=L)
    realised = spec.realised(dev["y_new"])
    whole, score, odds, brier = {}, {}, {}, {}
    for name, c in cops.items():
        paths = torch.full((count, S, L, N), float("nan"), device=DEV)
        u = c.uniforms(count, S, L, 0, L, T.STEPS_ORIGIN0, T.STEPS_KEY)
        ops.scenario_roll(window, dev["f_new"], T.STEPS_TAUS, paths, 0, last=True, uniforms=u)
        assert bool(torch.isfinite(paths).all())
        whole[name] = float(path_energy_score(dev["y_new"], paths))
        score[name] = EnsembleScores(dev["y_new"], paths)
        events = spec.count(paths)
        odds[name] = float(events.p_run[:, 0].mean())
        brier[name] = float(events.score(realised).brier_run_column[0])
    print(f"whole-trajectory energy {whole}; per-step energy {[float(s.energy) for s in score.values()]}; crps "
          f"{[float(s.crps) for s in score.values()]}; mean odds {odds}; brier {brier}; max |T_raw - T_true| {t_err:.4f}")
    assert whole["space"] - whole["steps"] > 0.035
    assert abs(score["space"].energy - score["steps"].energy) < 0.02
    assert abs(score["space"].crps - score["steps"].crps) < 0.005
    assert odds["space"] <= 0.02 and odds["steps"] >= 0.08
    assert brier["space"] - brier["steps"] > 0.003
    assert t_err < 0.15


def test_path_energy_score_is_the_energy_of_the_flattened_rows():
    from stemgnn_amd.math_utils import EnsembleScores, path_energy_score
    g = torch.Generator().manual_seed(SEED + 5)
    y = torch.randn(6, 3, 5, generator=g).to(DEV)
    paths = torch.randn(6, 4, 3, 5, generator=g).to(DEV)
    got = float(path_energy_score(y, paths))
    want = T.path_energy(y.cpu().numpy(), paths.cpu().numpy())
    assert abs(got - want) <= 1e-12 * abs(want) + 1e-12
    flat = EnsembleScores(y.reshape(6, 1, 15), paths.reshape(6, 4, 1, 15))
    assert got == float(flat.energy)
    mul, add = torch.linspace(0.5, 2.0, 5), torch.linspace(-1.0, 1.0, 5)
    scaled = float(path_energy_score(y, paths, mul=mul, add=add, fair=True))
    yd = y.cpu().double() * mul.double() + add.double()
    pd = paths.cpu().double() * mul.double() + add.double()
    x = pd.reshape(6, 4, 15).numpy()
    first = np.sqrt(((x - yd.reshape(6, 1, 15).numpy()) ** 2).sum(axis=-1)).mean(axis=1)
    second = np.sqrt(((x[:, :, None] - x[:, None]) ** 2).sum(axis=-1)).sum(axis=(1, 2)) / (2.0 * 4 * 3)
    assert abs(scaled - float((first - second).mean())) <= 1e-9


# ---- end to end: the small quantile model of tests/test_hip_copula.py ---------------------------------------------------------
N_E, W_E, H_E, TAUS_E = 9, 12, 3, (0.1, 0.5, 0.9)


def test_space_time_scenarios_of_a_model_end_to_end():
    from stemgnn_amd import LiveForecaster, Model, trainer
    from stemgnn_amd.math_utils import GaussianCopula, SpaceTimeCopula
    torch.manual_seed(SEED)
    model = Model(N_E, 2, W_E, 2, horizon=H_E, quantiles=TAUS_E).to(DEV).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(5, W_E, N_E, generator=g).to(DEV)
    y = torch.randn(5, 7, N_E, generator=g).to(DEV)
    graph = model.latent_graph(x)
    xv = torch.randn(40, W_E, N_E, generator=g).to(DEV)
    yv = torch.randn(40, H_E, N_E, generator=g).to(DEV)
    fc, tg = trainer.rolling_forecast(model, [(xv, yv)], H_E, adjacency=graph)
    cop = SpaceTimeCopula(TAUS_E, step_shrinkage=0.1).fit(tg, fc)
    plain = GaussianCopula(TAUS_E).fit(tg, fc)
    assert cop.steps == H_E and cop.nodes == N_E and int(cop.step_pairs.min()) == 40 * N_E
    assert tsame(cop.factor_t, plain.factor_t) and int(cop.pairs.min()) == 40 * H_E
    raw, shrunk = cop.step_correlation_raw.cpu().numpy(), cop.step_correlation.cpu().numpy()
    assert np.allclose(shrunk, 0.9 * raw + 0.1 * np.eye(H_E), rtol=0, atol=1e-15)
    assert np.array_equal(cop.step_factor.cpu().numpy(), np.linalg.cholesky(shrunk).astype(np.float32))
    whole = [(x, y)]
    want, _ = trainer.rolling_forecast(model, whole, 7, adjacency=graph)
    kw = dict(paths=16, seed=11, adjacency=graph, return_paths=True)
    bands, target, paths = trainer.rolling_scenarios(model, whole, 7, coupling=cop, **kw)
    assert bands.shape == (5, 3, 7, N_E) and paths.shape == (5, 16, 7, N_E) and tsame(target, y)
    assert tsame(bands[:, :, :3], want[:, :, :3])                              # round 0: rolling_forecast's bits
    assert bool(torch.isfinite(bands).all()) and bool(torch.isfinite(paths).all())
    b2, _, p2 = trainer.rolling_scenarios(model, whole, 7, coupling=cop, **kw)
    assert tsame(b2, bands) and tsame(p2, paths)                               # two calls, the same bits
    split = [(x[:2], y[:2]), (x[2:], y[2:])]
    b3, t3, p3 = trainer.rolling_scenarios(model, split, 7, coupling=cop, **kw)
    assert tsame(b3, bands) and tsame(t3, target) and tsame(p3, paths)         # 5 at once == 2 + 3
    _, _, other = trainer.rolling_scenarios(model, whole, 7, coupling=plain, **kw)
    assert not tsame(other, paths)                                             # the step coupling moves the paths
    # identity steps: the paths of the node copula, bit for bit
    R = plain.correlation.cpu().numpy()
    same = SpaceTimeCopula.from_correlations(R, np.eye(H_E), TAUS_E, device=DEV)
    _, _, p5 = trainer.rolling_scenarios(model, whole, 7, coupling=same, **kw)
    _, _, p6 = trainer.rolling_scenarios(model, whole, 7, coupling=GaussianCopula.from_correlation(R, TAUS_E, device=DEV), **kw)
    assert tsame(p5, p6)
    # a state_dict round trip gives the same uniforms
    again = SpaceTimeCopula.from_state_dict(cop.state_dict())
    assert tsame(again.uniforms(3, 4, H_E, 3, 7, 5, 11), cop.uniforms(3, 4, H_E, 3, 7, 5, 11))
    assert tsame(again.uniforms(3, 4, 1, 6, 7, 5, 11), cop.uniforms(3, 4, 1, 6, 7, 5, 11))      # the leading 1 x 1 block
    live = LiveForecaster(model, W_E, 7, history=4, adjacency=graph)
    live.push(np.random.default_rng(SEED + 3).normal(size=(W_E + 2, N_E)))
    live.seed = 21
    lb, lp = live.scenarios(paths=8, coupling=cop, return_paths=True)
    assert tuple(lp.shape) == (8, 7, N_E) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lb).all())
    # a copula of fewer steps than a round is refused before predict is called
    short = SpaceTimeCopula.from_correlations(R, T.decay(2, 0.8), TAUS_E, device=DEV)
    calls = []
    predict = model.predict
    model.predict = lambda *a, **k: (calls.append(1), predict(*a, **k))[1]
    with pytest.raises(ValueError, match="couples 2 steps, a round of the model has 3"):
        trainer.rolling_scenarios(model, whole, 7, coupling=short, **kw)
    assert not calls
    del model.predict
