"""GPU: the Gaussian-copula coupling of scenario paths -- the kernels of csrc/copula.hip and stemgnn_scenario_roll_given against
the numpy restatement of their definitions (tests/helpers/copula_ref.py, scenario_ref.py), and math_utils.GaussianCopula through
trainer.rolling_scenarios / LiveForecaster.scenarios.

Comparisons of float32 results are of bit patterns, with test_hip_scenario.py's one remark: a value that is ARITHMETIC is
compared as "the same bits, or NaN on both sides" (same_draws: IEEE leaves the sign and payload of an invalid operation's NaN to
the implementation), a SELECTION strictly (same_bits).  Every float32 output lies inside a NaN-filled buffer with guard words on
both sides, compared whole.  The fp64 comparisons carry the bounds of the issue, stated where they are used."""
import numpy as np
import pytest
import torch

from tests.helpers import copula_ref as C
from tests.helpers import scenario_ref as R
from tests.test_hip_scenario import (DEV, GUARD, KEY, LEVELS, OFFSET, ORIGIN0, SEED, device_copy, guarded, same_bits, same_draws,
                                     special_columns, tbits, tsame, u32)

pytestmark = pytest.mark.gpu
NAN_BITS = 0x7fc00000


def whole_of(ref, misalign):
    lo = GUARD + (1 if misalign else 0)
    out = np.full(ref.size + 2 * GUARD + 1, np.nan, np.float32)
    out[lo:lo + ref.size] = ref.reshape(-1)
    return out, lo


def special_uniforms(shape, taus, rng):
    """float32 uniforms on the draw's grid with, by flat index, the two ends of the clamp and values exactly at a level"""
    u = R.uniform(rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64).astype(np.uint32)).reshape(-1)
    idx = np.arange(u.size)
    u[idx % 13 == 1] = C.U_LO
    u[idx % 13 == 2] = C.U_HI
    for q, t in enumerate(taus):
        u[idx % 41 == 3 + q] = np.float32(t)
    return u.reshape(shape)


# (N, Q, S, W, L, round0, tails, step, horizon, misalign, last)
GIVEN_CASES = [
    (1, 2, 1, 4, 1, True, "linear", 0, 7, False, False),
    (1, 3, 7, 4, 1, False, "clamp", 6, 7, False, True),
    (5, 3, 2, 3, 3, True, "clamp", 0, 7, False, False),
    (5, 9, 64, 12, 3, False, "linear", 6, 7, False, False),         # the last round, cut short, window still made
    (5, 32, 2, 12, 3, True, "linear", 0, 7, False, False),
    (64, 3, 64, 12, 3, True, "linear", 0, 7, False, False),         # 16-byte path, round 0
    (64, 9, 7, 12, 3, False, "clamp", 3, 7, False, False),          # 16-byte path, fewer threads (Q = 9)
    (64, 32, 2, 3, 3, False, "linear", 3, 7, False, False),         # 16-byte path, 64 threads (Q = 32)
    (64, 2, 2, 4, 1, False, "linear", 5, 7, True, False),           # N % 4 == 0 off a 16-byte boundary: scalar
    (64, 3, 7, 12, 3, True, "clamp", 0, 2, True, True),             # horizon below L
    (257, 3, 64, 12, 3, False, "linear", 6, 7, False, True),        # cut short, no next window
    (257, 9, 7, 3, 3, True, "linear", 0, 7, False, False),
    (257, 2, 2, 12, 3, False, "clamp", 3, 7, True, False),
    (64, 3, 1, 12, 3, True, "clamp", 0, 7, False, False),           # S = 1: fan == 1 == S
]


def run_given(lib, _lib, d_in, d_fc, taus, d_u, Bo, S, fan, W, L, N, Q, step, horizon, tails, d_next, d_paths, d_bands):
    rc = lib.stemgnn_scenario_roll_given(d_in.data_ptr(), d_fc.data_ptr(), _lib.host_floats(taus), d_u.data_ptr(), Bo, S, fan, W,
                                         L, N, Q, step, horizon, _lib.SG_SCENARIO_TAILS[tails],
                                         None if d_next is None else d_next.data_ptr(), d_paths.data_ptr(),
                                         None if d_bands is None else d_bands.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", GIVEN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_roll_given_matches_the_draw_and_the_window_roll(case):
    from stemgnn_amd import _lib
    N, Q, S, W, L, round0, tails, step, horizon, misalign, last = case
    lib = _lib.load()
    taus = LEVELS[Q]
    Bo = 2 if S >= 64 else 3
    fan = S if round0 else 1
    Bsrc = Bo if round0 else Bo * S
    rng = np.random.default_rng(SEED + N + 7 * Q + 13 * S)
    inputs = rng.normal(size=(Bsrc, W, N)).astype(np.float32)
    forecast = special_columns(rng.normal(size=(Bsrc, Q, L, N)).astype(np.float32), rng)
    u = special_uniforms((Bo, S, L, N), taus, rng)
    ref_paths = np.full((Bo, S, horizon, N), np.nan, np.float32)
    ref_next = None if last else np.full((Bo * S, W, N), np.nan, np.float32)
    ref_bands = np.full((Bo, Q, horizon, N), np.nan, np.float32) if round0 else None
    C.roll_given(inputs, forecast, taus, u, Bo, S, fan, step, horizon, tails, ref_paths, ref_bands, ref_next)
    _, d_in = device_copy(inputs, misalign)
    _, d_fc = device_copy(forecast, misalign)
    _, d_u = device_copy(u, misalign)
    w_paths, d_paths = guarded(ref_paths.shape, misalign)
    w_next, d_next = (None, None) if last else guarded(ref_next.shape, misalign)
    w_bands, d_bands = guarded(ref_bands.shape, misalign) if round0 else (None, None)
    run_given(lib, _lib, d_in, d_fc, taus, d_u, Bo, S, fan, W, L, N, Q, step, horizon, tails, d_next, d_paths, d_bands)
    got_paths = w_paths.cpu().numpy()
    exp_paths, lo = whole_of(ref_paths, misalign)
    written = np.zeros(ref_paths.shape, bool)
    written[:, :, step:step + min(L, horizon - step)] = True
    wmask = np.zeros(exp_paths.size, bool)
    wmask[lo:lo + ref_paths.size] = written.reshape(-1)
    assert same_draws(got_paths[wmask], exp_paths[wmask])
    assert same_bits(got_paths[~wmask], exp_paths[~wmask])                   # the guards and every unwritten step
    assert np.isfinite(ref_paths[written]).mean() > 0.5
    if not last:
        got, (exp, _) = w_next.cpu().numpy(), whole_of(ref_next, misalign)
        drawn = np.zeros(ref_next.shape, bool)
        drawn[:, W - L:] = True
        dmask = np.zeros(exp.size, bool)
        dmask[lo:lo + ref_next.size] = drawn.reshape(-1)
        assert same_draws(got[dmask], exp[dmask])
        assert same_bits(got[~dmask], exp[~dmask])                           # the rows that move up, and the guards
    if round0:
        assert same_bits(w_bands.cpu().numpy(), whole_of(ref_bands, misalign)[0])
    assert same_bits(d_in.cpu().numpy(), inputs) and same_bits(d_fc.cpu().numpy(), forecast) and same_bits(d_u.cpu().numpy(), u)


@pytest.mark.parametrize("N", (64, 5))                                       # the 16-byte path and the scalar one
def test_roll_given_with_the_independent_uniforms_is_the_existing_entry(N):
    from stemgnn_amd import _lib
    lib = _lib.load()
    Q, S, W, L, step, horizon, Bo = 3, 7, 12, 3, 3, 7, 3
    taus = LEVELS[Q]
    rng = np.random.default_rng(SEED + 100 + N)
    inputs = rng.normal(size=(Bo * S, W, N)).astype(np.float32)
    forecast = special_columns(rng.normal(size=(Bo * S, Q, L, N)).astype(np.float32), rng)
    u = R.uniform(R.words(ORIGIN0, Bo, S, horizon, step, L, N, KEY, OFFSET, "independent"))
    _, d_in = device_copy(inputs, False)
    _, d_fc = device_copy(forecast, False)
    _, d_u = device_copy(u, False)
    outs = []
    for given in (False, True):
        w_paths, d_paths = guarded((Bo, S, horizon, N), False)
        w_next, d_next = guarded((Bo * S, W, N), False)
        if given:
            run_given(lib, _lib, d_in, d_fc, taus, d_u, Bo, S, 1, W, L, N, Q, step, horizon, "linear", d_next, d_paths, None)
        else:
            rc = lib.stemgnn_scenario_roll(d_in.data_ptr(), d_fc.data_ptr(), _lib.host_floats(taus), Bo, S, 1, W, L, N, Q, step,
                                           horizon, ORIGIN0, KEY, OFFSET, _lib.SG_SCENARIO_COUPLING["independent"],
                                           _lib.SG_SCENARIO_TAILS["linear"], d_next.data_ptr(), d_paths.data_ptr(), None, None)
            assert rc == 0
            torch.cuda.synchronize()
        outs.append((w_paths.cpu().numpy(), w_next.cpu().numpy()))
    assert same_bits(outs[0][0], outs[1][0]) and same_bits(outs[0][1], outs[1][1])
    assert np.isfinite(outs[0][0][GUARD:-GUARD - 1].reshape(Bo, S, horizon, N)[:, :, step:step + L]).mean() > 0.5


# (N, Q, H, tails, misalign)
PIT_CASES = [
    (1, 2, 1, "linear", False), (1, 9, 3, "clamp", False), (5, 3, 3, "linear", False), (5, 32, 1, "clamp", False),
    (64, 3, 3, "linear", False), (64, 9, 1, "clamp", False), (64, 32, 3, "linear", False), (64, 2, 3, "clamp", True),
    (257, 3, 1, "clamp", False), (257, 9, 3, "linear", True), (257, 2, 3, "linear", False), (257, 32, 1, "clamp", False),
]


@pytest.mark.parametrize("case", PIT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_pit_matches_the_restatement(case):
    from stemgnn_amd import _lib
    N, Q, H, tails, misalign = case
    lib = _lib.load()
    taus = LEVELS[Q]
    count = 7
    rng = np.random.default_rng(SEED + 200 + N + 7 * Q + H)
    forecast = special_columns(rng.normal(size=(count, Q, H, N)).astype(np.float32), rng)
    y = rng.normal(size=(count, H, N)).astype(np.float32)
    flat, idx = y.reshape(-1), np.arange(y.size)
    at_a_value = forecast.transpose(0, 2, 3, 1).reshape(-1, Q)[idx, idx % Q]
    flat[idx % 5 == 1] = at_a_value[idx % 5 == 1]                               # exactly at a value of its column
    flat[idx % 17 == 2] = np.nan
    flat[idx % 19 == 3] = 1e6                                                   # beyond both ends
    flat[idx % 19 == 4] = -1e6
    ref = C.pit(forecast, taus, y, tails)
    _, d_y = device_copy(y, misalign)
    _, d_fc = device_copy(forecast, misalign)
    whole, d_u = guarded(ref.shape, misalign)
    rc = lib.stemgnn_copula_pit(d_y.data_ptr(), d_fc.data_ptr(), _lib.host_floats(taus), count, H, N, Q,
                                _lib.SG_SCENARIO_TAILS[tails], d_u.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    exp, lo = whole_of(ref, misalign)
    inside = np.zeros(exp.size, bool)
    inside[lo:lo + ref.size] = True
    assert same_draws(got[inside], exp[inside])
    assert same_bits(got[~inside], exp[~inside])
    missing = (np.isnan(y) | np.isnan(forecast).any(axis=1)).reshape(-1)
    assert (u32(got[inside])[missing] == NAN_BITS).all() and missing.any()
    fin = got[inside][~np.isnan(got[inside])]
    assert fin.size > 0.5 * ref.size and fin.min() >= C.U_LO and fin.max() <= C.U_HI
    ends = (C.U_LO, C.U_HI) if tails == "linear" else (np.float32(taus[0]), np.float32(taus[-1]))
    assert (fin == ends[0]).any() and (fin == ends[1]).any()                    # the far targets reach both ends
    assert tails == "linear" or (fin.min() == ends[0] and fin.max() == ends[1])
    assert same_bits(d_y.cpu().numpy(), y) and same_bits(d_fc.cpu().numpy(), forecast)


def guarded_typed(n, dtype, fill):
    whole = torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dtype)
    return whole, whole[GUARD:GUARD + n]


GRAM_M = (1, 7, 300, C.CHUNK + 6)            # the last spans the kernel's row-chunk edge: CP_CHUNK = 1024 rows per workgroup
GRAM_N = (1, 5, 17, 64, 257)


@pytest.mark.parametrize("N", GRAM_N)
@pytest.mark.parametrize("M", GRAM_M)
def test_gram_matches_fp64(M, N):
    """pairs exactly; each sum within (M + 64) 2^-53 times the same sum over the absolute values of its terms -- for sum z_i z_j
    that is (|Z|^T |Z|)_ij, the bound of an M-term fp64 sum plus a few ulps for the inverse CDF; for sum z_i and sum z_i^2 the
    yardstick is their own absolute sum over the pair's rows."""
    from stemgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(SEED + 300 + 1000 * N + M)
    u = np.clip(rng.random(size=(M, N)).astype(np.float32), C.U_LO, C.U_HI)
    u[rng.random(size=u.shape) < 0.1] = np.nan
    u.reshape(-1)[:3] = (C.U_LO, C.U_HI, 0.5)[:min(3, u.size)]
    if N > 1:
        u[:, N - 2] = np.nan                                                    # a column that is absent throughout
    pairs, sums, mags = C.gram(u)
    _, d_u = device_copy(u, False)
    words = lib.stemgnn_copula_scratch_doubles(M, N)
    assert words == -(-M // C.CHUNK) * 4 * N * N
    runs = []
    for _ in range(2):
        scratch = torch.full((words,), float("nan"), device=DEV, dtype=torch.float64)
        w_pairs, d_pairs = guarded_typed(N * N, torch.int64, -7)
        w_sums, d_sums = guarded_typed(3 * N * N, torch.float64, float("nan"))
        assert lib.stemgnn_copula_gram(d_u.data_ptr(), M, N, scratch.data_ptr(), d_pairs.data_ptr(), d_sums.data_ptr(), None) == 0
        torch.cuda.synchronize()
        runs.append((w_pairs.cpu().numpy(), w_sums.cpu().numpy()))
    (got_pairs, got_sums), again = runs
    assert np.array_equal(got_pairs, again[0]) and np.array_equal(got_sums.view(np.int64), again[1].view(np.int64))
    assert (got_pairs[:GUARD] == -7).all() and (got_pairs[-GUARD:] == -7).all()
    assert np.isnan(got_sums[:GUARD]).all() and np.isnan(got_sums[-GUARD:]).all()
    assert np.array_equal(got_pairs[GUARD:-GUARD].reshape(N, N), pairs)
    err = np.abs(got_sums[GUARD:-GUARD].reshape(3, N, N) - sums)
    bound = (M + 64) * 2.0 ** -53 * mags
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.nanmax(np.where(bound > 0, err / bound, 0.0)))
    print(f"M {M} N {N}: worst error / bound {worst:.4f}")
    assert (err <= bound).all()
    assert same_bits(d_u.cpu().numpy(), u)


# (N, Bo, S, L): 24 rows, a partial tile of 16; the largest N of the 16-row configuration; the largest of the 4-row one, 6 rows
UNIFORM_CASES = [(1, 4, 3, 2), (5, 4, 3, 2), (64, 4, 3, 2), (257, 4, 3, 2), (512, 2, 3, 3), (2048, 2, 1, 3)]
ALLOW = 16                                   # ulps of allowance for normcdfinvf / normcdff (the issue's figure)


@pytest.mark.parametrize("case", UNIFORM_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_uniforms_match_fp64(case):
    """|u - u*| <= 0.4 (N + 16) 2^-24 (|L| |e*|)_n + 4 * 2^-24: the sequential fp32 summation bound times max phi = 0.399, 16 ulps
    for normcdfinvf / normcdff, and u's own rounding."""
    from stemgnn_amd import _lib
    N, Bo, S, L = case
    lib = _lib.load()
    step, horizon = 3, 7
    ij = np.arange(N)
    factor = C.factor_of(0.7 ** np.abs(ij[:, None] - ij[None, :]))
    factor_t = np.ascontiguousarray(factor.T)
    factor_t[np.tril_indices(N, -1)] = np.nan                                   # k > n: must not influence the result
    want, mag = C.uniforms(factor, ORIGIN0, Bo, S, horizon, step, L, KEY, OFFSET)
    d_f = torch.from_numpy(factor_t).to(DEV)

    def run(origin0, bo):
        whole, d_u = guarded((bo, S, L, N), False)
        rc = lib.stemgnn_copula_uniforms(d_f.data_ptr(), bo, S, L, N, step, horizon, origin0, KEY, OFFSET, d_u.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        return whole.cpu().numpy()

    got = run(ORIGIN0, Bo)
    inner = got[GUARD:GUARD + want.size].reshape(want.shape)
    assert np.isnan(got[:GUARD]).all() and np.isnan(got[GUARD + want.size:]).all()      # every guard word is intact
    assert not np.isnan(inner).any() and inner.min() >= C.U_LO and inner.max() <= C.U_HI
    err = np.abs(inner.astype(np.float64) - want)
    bound = 0.4 * (N + ALLOW) * 2.0 ** -24 * mag + 4 * 2.0 ** -24
    print(f"N {N}: worst error / bound {float((err / bound).max()):.4f}, max error {float(err.max()):.3e}")
    assert (err <= bound).all()
    assert same_bits(run(ORIGIN0, Bo), got)                                     # two runs, the same bits
    half = Bo // 2                                                              # the loader's batching cannot move a draw
    parts = [run(ORIGIN0, half)[GUARD:GUARD + want.size // 2], run(ORIGIN0 + half, half)[GUARD:GUARD + want.size // 2]]
    assert same_bits(np.concatenate(parts), got[GUARD:GUARD + want.size])


def test_the_dependence_is_the_one_asked_for():
    from stemgnn_amd.math_utils import GaussianCopula
    r = C.block_correlation(16, 8, 0.9)
    cop = GaussianCopula.from_correlation(r, LEVELS[3], device=DEV)
    u = cop.uniforms(8, 256, 2, 0, 2, ORIGIN0, KEY).cpu().numpy().reshape(-1, 16)
    assert u.shape[0] == 4096 and u.min() >= C.U_LO and u.max() <= C.U_HI
    mean_err = float(np.abs(u.mean(axis=0) - 0.5).max())
    lower = np.tril(cop.factor_t.cpu().numpy().T.astype(np.float64))
    corr_err = float(np.abs(np.corrcoef(C.ndtri(u.astype(np.float64)), rowvar=False) - lower @ lower.T).max())
    print(f"max |mean u - 0.5| = {mean_err:.4f} (bound 0.0226), max |corr - L L^T| = {corr_err:.4f} (bound 0.078)")
    assert mean_err <= 5 * np.sqrt(1 / (12 * 4096))
    assert corr_err <= 5 / np.sqrt(4096)
    assert np.abs(lower @ lower.T - r).max() < 1e-6


def test_the_energy_score_prefers_the_fitted_copula():
    """Truth y = chol(R_true) e, two blocks of 8 nodes at 0.9; the forecast is the exact N(0, 1) quantile function at seven levels
    for every row, so only the dependence differs between the ensembles.  By the restatement alone at this seed
    (tests/test_copula_abi.py): energy(independent) - energy(copula) = 0.1179, energy(path) - energy(copula) = 0.1756 (the
    issue's numpy check over 8 seeds: 0.080 - 0.129 and 0.110 - 0.183; the bound 0.04 is half the smallest), CRPS within 0.0003
    of one another (bound 0.05: the marginals are kept), max |correlation_raw - R_true| = 0.0903 (bound 0.25: sampling error at
    512 rows plus the attenuation of seven linearly interpolated levels).  The device's figures are printed."""
    from stemgnn_amd import ops
    from stemgnn_amd.math_utils import EnsembleScores, GaussianCopula
    case = C.energy_case(SEED + 7)
    dev = {k: torch.from_numpy(v).to(DEV) for k, v in case.items() if k != "R_true"}
    cop = GaussianCopula(C.ENERGY_TAUS, shrinkage=0.05).fit(dev["y_fit"], dev["f_fit"])
    raw = cop.correlation_raw.cpu().numpy()
    raw_err = float(np.abs(raw - case["R_true"]).max())
    count, S, N = C.ENERGY_NEW, C.ENERGY_S, C.ENERGY_N
    window = torch.zeros(count, 1, N, device=DEV)
    score = {}
    for name in ("independent", "path", "copula"):
        paths = torch.full((count, S, 1, N), float("nan"), device=DEV)
        kw = dict(uniforms=cop.uniforms(count, S, 1, 0, 1, C.ENERGY_ORIGIN0, C.ENERGY_KEY)) if name == "copula" else \
            dict(coupling=name)
        ops.scenario_roll(window, dev["f_new"], C.ENERGY_TAUS, paths, 0, origin0=C.ENERGY_ORIGIN0, seed=C.ENERGY_KEY, last=True,
                          **kw)
        score[name] = EnsembleScores(dev["y_new"], paths)
    m_ind = score["independent"].energy - score["copula"].energy
    m_path = score["path"].energy - score["copula"].energy
    crps = [float(s.crps) for s in score.values()]
    print(f"energy margins: independent {m_ind:.4f}, path {m_path:.4f}; crps {crps}; raw correlation error {raw_err:.4f}")
    assert m_ind > 0.04 and m_path > 0.04
    assert max(crps) - min(crps) < 0.05
    assert raw_err < 0.25
    assert tuple(cop.pairs.shape) == (N, N) and int(cop.pairs.min()) == C.ENERGY_FIT and cop.nodes == N
    shrunk = cop.correlation.cpu().numpy()
    assert np.allclose(shrunk, 0.95 * raw + 0.05 * np.eye(N), rtol=0, atol=1e-15)


# ---- end to end: the small quantile model of tests/test_hip_ensemble.py --------------------------------------------------------
N_E, W_E, H_E, TAUS_E = 9, 12, 3, (0.1, 0.5, 0.9)


def test_copula_scenarios_of_a_model_end_to_end():
    from stemgnn_amd import LiveForecaster, Model, trainer
    from stemgnn_amd.math_utils import GaussianCopula
    torch.manual_seed(SEED)
    model = Model(N_E, 2, W_E, 2, horizon=H_E, quantiles=TAUS_E).to(DEV).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(5, W_E, N_E, generator=g).to(DEV)
    y = torch.randn(5, 7, N_E, generator=g).to(DEV)
    graph = model.latent_graph(x)
    # held-out residuals at the model's own horizon: 40 windows, pooled over the 3 steps
    xv = torch.randn(40, W_E, N_E, generator=g).to(DEV)
    yv = torch.randn(40, H_E, N_E, generator=g).to(DEV)
    fc, tg = trainer.rolling_forecast(model, [(xv, yv)], H_E, adjacency=graph)
    cop = GaussianCopula(TAUS_E).fit(tg, fc)
    assert cop.nodes == N_E and int(cop.pairs.min()) == 40 * H_E and tuple(cop.factor_t.shape) == (N_E, N_E)
    u = cop.pit(tg, fc)
    assert tuple(u.shape) == (40, H_E, N_E) and float(u.min()) >= C.U_LO and float(u.max()) <= C.U_HI
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
    _, _, free = trainer.rolling_scenarios(model, whole, 7, coupling="independent", **kw)
    assert not tsame(free, paths)
    # a state_dict round trip gives the same paths
    again = GaussianCopula.from_state_dict(cop.state_dict())
    _, _, p4 = trainer.rolling_scenarios(model, whole, 7, coupling=again, **kw)
    assert tsame(p4, paths)
    # LiveForecaster.scenarios on the same window is the corresponding row
    live = LiveForecaster(model, W_E, 7, history=4, adjacency=graph)
    rng = np.random.default_rng(SEED + 3)
    live.push(rng.normal(size=(W_E + 2, N_E)))
    live.seed = 21
    lb, lp = live.scenarios(paths=8, coupling=cop, return_paths=True)
    window = torch.cat([live.ring_x[(live.rows - W_E + i) % live.C][None] for i in range(W_E)])[None].contiguous()
    wb, _, wp = trainer.rolling_scenarios(model, [(window, torch.zeros(1, 7, N_E, device=DEV))], 7, paths=8, seed=21,
                                          origin=live.rows, return_paths=True, adjacency=graph, coupling=cop)
    assert tsame(lb, wb[0]) and tsame(lp, wp[0])
    scored = trainer.score_forecast(bands, target, quantiles=TAUS_E, paths=paths)
    assert np.isfinite(scored["energy_score"]) and np.isfinite(scored["crps"])
    assert tbits(paths).shape == (5, 16, 7, N_E)
