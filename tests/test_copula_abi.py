"""CPU: the copula entries of include/stemgnn_hip.h (csrc/copula.hip, stemgnn_scenario_roll_given in csrc/scenario.hip) are
exported, declared and bound; every bad argument is refused before any launch; math_utils.GaussianCopula and
engine.scenario_rounds refuse what they must on the host; the numpy restatement (tests/helpers/copula_ref.py) checks itself:
the transform inverts the draw, and the restatement alone clears the statistical margins of the GPU test.  Nothing is launched."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import copula_ref as C
from tests.helpers import scenario_ref as R

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
SEED = 20261020
NEW = ("stemgnn_copula_pit", "stemgnn_copula_gram", "stemgnn_copula_scratch_doubles", "stemgnn_copula_uniforms",
       "stemgnn_scenario_roll_given")
TAUS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def floats(*v):
    return (ctypes.c_float * len(v))(*v)


def refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == SG_EINVAL


def test_symbols_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib, engine, math_utils, ops, trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_scenario_roll_given"][1]) == 18 and len(sig["stemgnn_copula_pit"][1]) == 10
    assert len(sig["stemgnn_copula_gram"][1]) == 7 and len(sig["stemgnn_copula_uniforms"][1]) == 12
    assert sig["stemgnn_copula_uniforms"][1][7] is ctypes.c_longlong                    # origin0
    assert sig["stemgnn_copula_uniforms"][1][8] is ctypes.c_ulonglong and sig["stemgnn_copula_uniforms"][1][9] is ctypes.c_ulonglong
    assert sig["stemgnn_copula_scratch_doubles"] == (ctypes.c_size_t, [ctypes.c_long, ctypes.c_int])
    assert _lib.SG_SCENARIO_COUPLING == {"independent": 0, "path": 1}                   # the copula is no third code
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "copula.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    assert "scenario_draw.h" in makefile.split("HDRS =")[1].splitlines()[0]
    # one definition of the column's order and of the uniform, in the header both users include
    for user in ("copula.hip", "scenario.hip"):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "scenario_draw.h"' in text and "bool sc_less(" not in text and "float sc_uniform(" not in text, user
    for name in ("copula_pit", "copula_gram", "copula_uniforms"):
        assert callable(getattr(ops, name)), name
    par = inspect.signature(ops.scenario_roll).parameters
    assert tuple(par)[-1] == "uniforms" and par["uniforms"].default is None
    par = inspect.signature(math_utils.GaussianCopula.__init__).parameters
    assert tuple(par) == ("self", "quantiles", "shrinkage", "tails", "min_pairs")
    assert (par["shrinkage"].default, par["tails"].default, par["min_pairs"].default) == (0.05, "linear", 8)
    assert tuple(inspect.signature(math_utils.GaussianCopula.uniforms).parameters) == (
        "self", "Bo", "S", "L", "step", "horizon", "origin0", "seed", "offset")
    # the scenario signatures are where they were
    assert tuple(inspect.signature(trainer.rolling_scenarios).parameters)[:9] == (
        "model", "loader", "horizon", "paths", "seed", "adjacency", "coupling", "tails", "return_paths")
    assert tuple(inspect.signature(engine.LiveForecaster.scenarios).parameters) == (
        "self", "paths", "horizon", "seed", "coupling", "tails", "return_paths")
    assert lib.stemgnn_copula_scratch_doubles(7560, 228) == 8 * 4 * 228 * 228         # chunks of 1024 rows
    assert C.CHUNK == 1024 and lib.stemgnn_copula_scratch_doubles(C.CHUNK, 5) == 100
    assert lib.stemgnn_copula_scratch_doubles(C.CHUNK + 1, 5) == 200
    for m, n in ((0, 5), (5, 0), (-1, 5), (2 ** 31, 5), (5, 2 ** 16)):
        assert lib.stemgnn_copula_scratch_doubles(m, n) == 0, (m, n)


# the arguments of the entries, in order (the stream follows)
GIVEN_OK = dict(inputs=P, forecast=2 * P, taus=floats(*TAUS), uniforms=6 * P, Bo=4, S=8, fan=8, W=12, L=3, N=11, Q=3, step=0,
                horizon=7, tails=0, inputs_next=3 * P, paths=4 * P, bands=5 * P)
PIT_OK = dict(target=P, forecast=2 * P, taus=floats(*TAUS), count=5, H=3, N=11, Q=3, tails=0, u=3 * P)
GRAM_OK = dict(u=P, M=15, N=11, scratch=2 * P, pairs=3 * P, sums=4 * P)
UNI_OK = dict(factor_t=P, Bo=4, S=8, Lsteps=3, N=11, step=0, horizon=7, origin0=5, seed=1, offset=0, u=2 * P)
BAD_LEVELS = ((0.1, 0.1, 0.9), (0.5, 0.1, 0.9), (0.0, 0.5, 0.9), (0.1, 0.5, 1.0), (-0.1, 0.5, 0.9), (0.1, 0.5, 1.5),
              (0.1, float("nan"), 0.9), (float("nan"), 0.5, 0.9), (0.1, 0.5, float("nan")), (0.1, 0.9, 0.5))


def test_roll_given_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_scenario_roll_given, GIVEN_OK
    for k in ("inputs", "forecast", "taus", "uniforms", "paths"):
        assert refused(f, ok, **{k: None}), k
    assert refused(f, ok, inputs_next=P)                                        # the window cannot be rolled in place
    for k in ("Bo", "W", "L", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, L=13)                                                 # L > W
    for v in (-1, 7, 8):
        assert refused(f, ok, step=v), v
    assert refused(f, ok, horizon=0)
    for q in (1, 0, -1):
        assert refused(f, ok, Q=q, taus=floats(0.5)), q
    assert refused(f, ok, Q=33, taus=floats(*[(i + 1) / 40 for i in range(33)]))
    for bad in BAD_LEVELS:
        assert refused(f, ok, taus=floats(*bad)), bad
    for s in (0, -1, 1025):
        assert refused(f, ok, S=s, fan=s), s
        assert refused(f, ok, S=s, fan=1), s
    for fan in (0, 2, 4, 9, -1):
        assert refused(f, ok, fan=fan), fan
    assert refused(f, ok, fan=1)                                                # round-0 bands with a later round's fan
    for v in (-1, 2):
        assert refused(f, ok, tails=v), v
    assert refused(f, ok, Bo=2 ** 21, S=1024, fan=1024)                         # Bo * S
    assert refused(f, ok, W=2 ** 16, N=2 ** 15)                                 # W * N
    assert refused(f, ok, W=2 ** 12, L=2 ** 12, N=2 ** 18)                      # Q * L * N
    assert refused(f, ok, horizon=2 ** 20, N=2 ** 10)                           # Q * horizon * N
    assert refused(f, ok, S=1024, fan=1024, horizon=2 ** 21, N=1)               # S * horizon


def test_scenario_roll_still_refuses_a_third_coupling(lib):
    ok = dict(inputs=P, forecast=2 * P, taus=floats(*TAUS), Bo=4, S=8, fan=8, W=12, L=3, N=11, Q=3, step=0, horizon=7, origin0=5,
              seed=1, offset=0, coupling=0, tails=0, inputs_next=3 * P, paths=4 * P, bands=5 * P)
    for v in (2, 3, -1):
        assert refused(lib.stemgnn_scenario_roll, ok, coupling=v), v


def test_pit_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_copula_pit, PIT_OK
    for k in ("target", "forecast", "taus", "u"):
        assert refused(f, ok, **{k: None}), k
    for k in ("count", "H", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    for q in (1, 0, -1):
        assert refused(f, ok, Q=q, taus=floats(0.5)), q
    assert refused(f, ok, Q=33, taus=floats(*[(i + 1) / 40 for i in range(33)]))
    for bad in BAD_LEVELS:
        assert refused(f, ok, taus=floats(*bad)), bad
    for v in (-1, 2):
        assert refused(f, ok, tails=v), v
    assert refused(f, ok, H=2 ** 16, N=2 ** 15)                                 # H * N
    assert refused(f, ok, H=2 ** 15, N=2 ** 15)                                 # Q * H * N
    assert refused(f, ok, count=2 ** 20, H=2 ** 11, N=1)                        # count * H
    assert refused(f, ok, count=2 ** 30, H=1, N=2 ** 9 + 1)                     # the grid: 2^30 * 513 / 256 blocks


def test_gram_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_copula_gram, GRAM_OK
    for k in ("u", "scratch", "pairs", "sums"):
        assert refused(f, ok, **{k: None}), k
    for k in ("M", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, M=2 ** 31)                                            # M
    assert refused(f, ok, N=2 ** 16)                                            # N * N
    assert refused(f, ok, M=2 ** 30, N=2 ** 12)                                 # the grid: 256^2 tiles * 2^20 chunks


def test_uniforms_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_copula_uniforms, UNI_OK
    for k in ("factor_t", "u"):
        assert refused(f, ok, **{k: None}), k
    for k in ("Bo", "Lsteps", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, N=2049)                                               # beyond the LDS tile of four rows
    for s in (0, -1, 1025):
        assert refused(f, ok, S=s), s
    for v in (-1, 7, 8):
        assert refused(f, ok, step=v), v
    assert refused(f, ok, horizon=0)
    assert refused(f, ok, Bo=2 ** 19, S=1024, Lsteps=4)                         # Bo * S * Lsteps
    assert refused(f, ok, S=1024, horizon=2 ** 21)                              # S * horizon


def test_from_correlation_refuses_what_is_no_correlation_matrix():
    from stemgnn_amd.math_utils import GaussianCopula
    good = C.block_correlation(4, 2, 0.5)
    cop = GaussianCopula.from_correlation(good, TAUS, device="cpu")
    assert cop.nodes == 4 and cop.tails == "linear" and cop.pairs is None and cop.factor_t.dtype == torch.float32
    lower = np.linalg.cholesky(good)
    assert np.array_equal(cop.factor_t.numpy(), lower.astype(np.float32).T)      # factor_t[k, n] = L[n, k]
    with pytest.raises(ValueError, match="square"):
        GaussianCopula.from_correlation(np.ones((3, 4)), TAUS)
    bad = good.copy()
    bad[0, 1] = bad[1, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        GaussianCopula.from_correlation(bad, TAUS)
    bad = good.copy()
    bad[0, 1] += 1e-3
    with pytest.raises(ValueError, match="not symmetric"):
        GaussianCopula.from_correlation(bad, TAUS)
    bad = good.copy()
    bad[2, 2] = 1.001
    with pytest.raises(ValueError, match="diagonal is not 1"):
        GaussianCopula.from_correlation(bad, TAUS)
    bad = np.array([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]])
    with pytest.raises(ValueError, match="not positive definite .smallest eigenvalue -.*larger shrinkage"):
        GaussianCopula.from_correlation(bad, TAUS)
    for kw in (dict(quantiles=(0.5,)), dict(quantiles=(0.5, 0.1)), dict(quantiles=TAUS, shrinkage=1.5),
               dict(quantiles=TAUS, tails="flat"), dict(quantiles=TAUS, min_pairs=1)):
        with pytest.raises(ValueError):
            GaussianCopula(**kw)
    with pytest.raises(ValueError, match="not fitted"):
        GaussianCopula(TAUS).uniforms(1, 1, 1, 0, 1, 0, 0)
    # the state round trip needs no device
    again = GaussianCopula.from_state_dict(cop.state_dict())
    assert torch.equal(again.factor_t, cop.factor_t) and torch.equal(again.correlation, cop.correlation) and again.nodes == 4
    with pytest.raises(ValueError, match="saved for levels"):
        GaussianCopula(TAUS, tails="clamp").load_state_dict(cop.state_dict())


def test_scenario_rounds_refuses_a_copula_that_does_not_fit():
    from stemgnn_amd import Model, trainer
    from stemgnn_amd.engine import scenario_rounds
    from stemgnn_amd.math_utils import GaussianCopula
    model = Model(6, 2, 4, 2, horizon=2, quantiles=TAUS)
    loader = [(torch.zeros(2, 4, 6), torch.zeros(2, 5, 6))]
    four = GaussianCopula.from_correlation(np.eye(4), TAUS, device="cpu")
    clamped = GaussianCopula.from_correlation(np.eye(6), TAUS, tails="clamp", device="cpu")
    assert model.training
    for cop, what in ((four, "fitted on 4 nodes, the window has 6"), (clamped, "tails are 'clamp', the call's 'linear'"),
                      (GaussianCopula(TAUS), "fitted GaussianCopula")):
        with pytest.raises(ValueError, match=what):
            scenario_rounds(model, loader[0][0], 5, 4, 0, 0, cop, "linear", {})
        with pytest.raises(ValueError, match=what):
            trainer.rolling_scenarios(model, loader, 5, paths=4, coupling=cop)
        assert model.training                                                   # as it was
    model.eval()
    with pytest.raises(ValueError, match="fitted on 4 nodes"):
        scenario_rounds(model, loader[0][0], 5, 4, 0, 0, four, "linear", {})
    assert not model.training
    model.train()


def test_ops_wrappers_have_no_cpu_fallback():
    from stemgnn_amd import ops
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import GaussianCopula
    with pytest.raises(StemGNNHipError):
        ops.copula_pit(torch.zeros(2, 3, 4), torch.zeros(2, 3, 3, 4), TAUS)
    with pytest.raises(StemGNNHipError):
        ops.copula_gram(torch.full((6, 4), 0.5))
    with pytest.raises(StemGNNHipError):
        ops.copula_uniforms(torch.eye(4), 2, 3, 1, 0, 5)
    with pytest.raises(StemGNNHipError):
        ops.scenario_roll(torch.zeros(2, 4, 6), torch.zeros(2, 3, 2, 6), TAUS, torch.zeros(2, 4, 5, 6), 0,
                          uniforms=torch.full((2, 4, 2, 6), 0.5))
    cop = GaussianCopula.from_correlation(np.eye(4), TAUS, device="cpu")
    with pytest.raises(StemGNNHipError):
        cop.uniforms(2, 3, 1, 0, 5, 0, 0)
    with pytest.raises(StemGNNHipError):
        GaussianCopula(TAUS).fit(torch.zeros(2, 3, 4), torch.zeros(2, 3, 3, 4))


def test_the_counter_map_of_the_restatement():
    a = R.words(2 ** 33 + 5, 2, 3, 7, 3, 3, 9, 0x9E3779B97F4A7C15, 0x100000003, "independent")
    b = C.words(2 ** 33 + 5, 2, 3, 7, 3, 3, 9, 0x9E3779B97F4A7C15, 0x100000003)
    assert a.dtype == b.dtype == np.uint32 and np.array_equal(a, b)
    a = R.words(2 ** 64 - 1, 2, 2, 5, 4, 1, 5, 7, 0, "independent")               # the counter wraps
    assert np.array_equal(a, C.words(2 ** 64 - 1, 2, 2, 5, 4, 1, 5, 7, 0))


@pytest.mark.parametrize("tails", ("linear", "clamp"))
@pytest.mark.parametrize("Q", (2, 3, 9))
def test_the_transform_inverts_the_draw(Q, tails):
    """pit(draw(u)) against u, u on the draw's grid, strictly increasing columns.  With eps = 2^-24, s = tau_(i+1) - tau_i,
    d = v_(i+1) - v_(i) and wt = (u - tau_i) / s, every operation of the two definitions rounded once:
      - the draw rounds u - tau_i, the division, d * wt; the transform rounds y - v_(i), its division and s * wt': six factors
        (1 + delta) on a quantity of size s |wt|, and the draw's last sum y = fl(v_(i) + m) leaves an absolute error eps |y| in
        y - v_(i), which the division by d turns into eps |y| / d on wt' -- the error the division inherits where the segment is
        short against the magnitude of its values.  Together, times s: s (6 eps |wt| + eps |y| / d), taken with 8 and 2 for the
        second-order terms;
      - the last sum tau_i + s wt' rounds once more: one ulp of u at most; 4 ulps are allowed.
    Where y rounds onto v_(i+1) the transform answers tau_(i+1) from the next segment, within the same bound.  With clamped tails
    the draw stops at the outer levels, so the transform returns u clipped to [tau_0, tau_(Q-1)]."""
    LEVELS = {2: (0.1, 0.9), 3: (0.1, 0.5, 0.9), 9: (0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95)}
    taus = np.asarray(LEVELS[Q], np.float32)
    rng = np.random.default_rng(SEED + Q)
    count = 4096
    col = np.sort(rng.normal(size=(count, Q, 1, 1)), axis=1).astype(np.float32)
    col = col[(np.diff(col, axis=1) > 0).all(axis=1)[:, 0, 0]]                   # strictly increasing in float32
    count = col.shape[0]
    assert count > 4000
    u = R.uniform(rng.integers(0, 2 ** 32, size=(count, 1, 1), dtype=np.uint64).astype(np.uint32))
    y = R.draw(col, taus, u, tails)
    back = C.pit(col, taus, y, tails)
    want = np.clip(u, taus[0], taus[-1]) if tails == "clamp" else u
    i = np.zeros(u.shape, np.int64)
    for q in range(1, Q - 1):
        i = np.where(taus[q] <= u, q, i)
    s = (taus[i + 1] - taus[i]).astype(np.float64)
    d = (np.take_along_axis(col, i[:, None] + 1, axis=1) - np.take_along_axis(col, i[:, None], axis=1))[:, 0].astype(np.float64)
    wt = np.abs(want.astype(np.float64) - taus[i]) / s
    eps = 2.0 ** -24
    bound = 4 * np.spacing(want).astype(np.float64) + s * (8 * eps * wt + 2 * eps * np.abs(y).astype(np.float64) / d)
    err = np.abs(back.astype(np.float64) - want.astype(np.float64))
    print(f"Q {Q} {tails}: max error / bound {float((err / bound).max()):.3f}, max error {float(err.max()):.3e}")
    assert (err <= bound).all()
    assert (back >= C.U_LO).all() and (back <= C.U_HI).all()


def test_the_restatement_clears_the_margins_of_the_energy_test():
    """The configuration of tests/test_hip_copula.py::test_the_energy_score_prefers_the_fitted_copula at its seed, by numpy
    alone: energy(independent) - energy(copula) = 0.1179, energy(path) - energy(copula) = 0.1756 (bound 0.04), the CRPS of the
    three ensembles within 0.0003 of one another (bound 0.05), max |correlation_raw - R_true| = 0.0903 (bound 0.25)."""
    case = C.energy_case(SEED + 7)
    out = C.energy_case_restated(case)
    score = {k: C.crps_and_energy(case["y_new"], out[k]) for k in ("independent", "path", "copula")}
    m_ind = score["independent"][1] - score["copula"][1]
    m_path = score["path"][1] - score["copula"][1]
    crps = [v[0] for v in score.values()]
    raw_err = float(np.abs(out["correlation_raw"] - case["R_true"]).max())
    print(f"energy margins: independent {m_ind:.4f}, path {m_path:.4f}; crps {crps}; raw correlation error {raw_err:.4f}")
    assert m_ind > 0.04 and m_path > 0.04
    assert max(crps) - min(crps) < 0.05
    assert raw_err < 0.25
