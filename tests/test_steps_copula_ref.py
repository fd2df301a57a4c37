"""CPU: the step coupling of the copula (stemgnn_copula_uniforms_steps, math_utils.SpaceTimeCopula) -- the numpy restatement
(tests/helpers/steps_copula_ref.py) checks itself, the entry is exported, declared and bound and refuses bad arguments before
any launch, SpaceTimeCopula and engine.scenario_rounds refuse on the host what they must, and the restatement alone clears
the statistical conditions the device is held to in tests/test_hip_steps_copula.py.  Nothing is launched."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import copula_ref as C
from tests.helpers import steps_copula_ref as T

SG_EINVAL = -10001
P = 64                          # a stand-in device address: every call below is refused before any use
TAUS = (0.1, 0.5, 0.9)
KEY, OFFSET, ORIGIN0 = 0x9E3779B97F4A7C15, 0x100000003, 2 ** 33 + 12345
STAT_SEED = 7                   # the first of the issue's five seeds; tests/test_hip_steps_copula.py uses the same


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_identity_steps_are_the_node_copula_exactly():
    for N, L in ((5, 3), (9, 1), (6, 16)):
        factor = C.factor_of(T.decay(N, 0.7))
        eye = np.eye(L, dtype=np.float32)
        eye[np.triu_indices(L, 1)] = np.nan                                      # above the diagonal: not read
        got, mag = T.uniforms_steps(factor, eye, ORIGIN0, 2, 3, 3 + L + 1, 3, L, KEY, OFFSET)
        want, want_mag = C.uniforms(factor, ORIGIN0, 2, 3, 3 + L + 1, 3, L, KEY, OFFSET)
        assert np.array_equal(got, want) and np.array_equal(mag, want_mag)
        assert got.shape == (2, 3, L, N) and np.isfinite(got).all()


def test_the_restated_dependence_is_separable():
    """4096 paths, L 3, N 6: the empirical correlation of the normal scores is within 5 / sqrt(4096) of T (x) R"""
    N, L = 6, 3
    r, t = T.decay(N, 0.7), T.decay(L, 0.8)
    factor, step_factor = C.factor_of(r), C.factor_of(t)
    u, _ = T.uniforms_steps(factor, step_factor, ORIGIN0, 16, 256, L, 0, L, KEY, OFFSET)
    z = C.ndtri(u).reshape(4096, L, N)
    err = float(np.abs(T.kron_correlation(z) - np.kron(t, r)).max())
    print(f"max |corr - T (x) R| = {err:.4f} (bound {5 / 64:.4f})")
    assert err <= 5 / np.sqrt(4096)
    assert abs(float(u.mean()) - 0.5) <= 5 * np.sqrt(1 / (12 * u.size))


def test_symbol_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib, math_utils, ops
    name = "stemgnn_copula_uniforms_steps"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    assert hasattr(lib, name) and name + "(" in header
    res, args = _lib.SIGNATURES[name]
    assert res is ctypes.c_int and len(args) == 13
    assert args[8] is ctypes.c_longlong and args[9] is ctypes.c_ulonglong and args[10] is ctypes.c_ulonglong   # origin0, seed, offset
    assert all(a is ctypes.c_int for a in args[2:8]) and all(a is ctypes.c_void_p for a in args[:2] + args[11:])
    assert len(_lib.SIGNATURES["stemgnn_copula_uniforms"][1]) == 12              # the existing entry stays
    par = inspect.signature(ops.copula_uniforms).parameters
    assert tuple(par)[-1] == "step_factor" and par["step_factor"].default is None
    assert issubclass(math_utils.SpaceTimeCopula, math_utils.GaussianCopula)
    par = inspect.signature(math_utils.SpaceTimeCopula.__init__).parameters
    assert tuple(par) == ("self", "quantiles", "shrinkage", "step_shrinkage", "tails", "min_pairs")
    assert (par["shrinkage"].default, par["step_shrinkage"].default, par["tails"].default, par["min_pairs"].default) == \
        (0.05, 0.0, "linear", 8)
    assert tuple(inspect.signature(math_utils.path_energy_score).parameters) == (
        "target", "paths", "mul", "add", "ignore_nan", "fair")


UNI_OK = dict(factor_t=P, step_factor=3 * P, Bo=4, S=8, Lsteps=3, N=11, step=0, horizon=7, origin0=5, seed=1, offset=0, u=2 * P)


def refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == SG_EINVAL


def test_the_entry_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_copula_uniforms_steps, UNI_OK
    for k in ("factor_t", "step_factor", "u"):
        assert refused(f, ok, **{k: None}), k
    for k in ("Bo", "Lsteps", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, Lsteps=17, horizon=40)                                # a tile of 16 rows holds no such path
    assert refused(f, ok, N=513, Lsteps=5)                                      # nor a tile of 4 rows this one
    assert refused(f, ok, N=2048, Lsteps=5) and refused(f, ok, N=2049, Lsteps=2)
    for s in (0, -1, 1025):
        assert refused(f, ok, S=s), s
    for v in (-1, 7, 8):
        assert refused(f, ok, step=v), v
    assert refused(f, ok, horizon=0)
    assert refused(f, ok, Bo=2 ** 19, S=1024, Lsteps=4)                         # Bo * S * Lsteps
    assert refused(f, ok, S=1024, horizon=2 ** 21)                              # S * horizon


def test_space_time_copula_refuses_on_the_host():
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import GaussianCopula, SpaceTimeCopula
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="step_shrinkage"):
            SpaceTimeCopula(TAUS, step_shrinkage=bad)
    r, t = C.block_correlation(4, 2, 0.5), T.decay(3, 0.8)
    cop = SpaceTimeCopula.from_correlations(r, t, TAUS, device="cpu")
    assert cop.nodes == 4 and cop.steps == 3 and cop.pairs is None and cop.step_pairs is None
    assert cop.step_factor.dtype == torch.float32 and tuple(cop.step_factor.shape) == (3, 3)
    assert np.array_equal(cop.step_factor.numpy(), np.linalg.cholesky(t).astype(np.float32))      # row-major, lower
    assert np.array_equal(cop.factor_t.numpy(), np.linalg.cholesky(r).astype(np.float32).T)
    assert np.array_equal(cop.step_correlation.numpy(), t) and cop.step_correlation.dtype == torch.float64
    not_pd = np.array([[1.0, 0.9, -0.9], [0.9, 1.0, 0.9], [-0.9, 0.9, 1.0]])
    with pytest.raises(ValueError, match="step matrix: .*not positive definite .smallest eigenvalue -"):
        SpaceTimeCopula.from_correlations(r, not_pd, TAUS, device="cpu")
    with pytest.raises(ValueError, match="not positive definite .smallest eigenvalue -"):
        SpaceTimeCopula.from_correlations(not_pd, t, TAUS, device="cpu")
    bad = t.copy()
    bad[0, 1] += 1e-3
    with pytest.raises(ValueError, match="step matrix: the matrix is not symmetric"):
        SpaceTimeCopula.from_correlations(r, bad, TAUS, device="cpu")
    with pytest.raises(ValueError, match="step matrix: a square matrix"):
        SpaceTimeCopula.from_correlations(r, np.ones((3, 4)), TAUS, device="cpu")
    with pytest.raises(TypeError, match="from_correlations"):
        SpaceTimeCopula.from_correlation(r, TAUS, device="cpu")
    with pytest.raises(ValueError, match="4 steps in a round, the copula couples 3"):          # L > steps, before any launch
        cop.uniforms(2, 3, 4, 0, 9, 0, 0)
    with pytest.raises(ValueError, match="not fitted"):
        SpaceTimeCopula(TAUS).uniforms(1, 1, 1, 0, 1, 0, 0)
    with pytest.raises(StemGNNHipError):                                        # no CPU fallback
        cop.uniforms(2, 3, 3, 0, 9, 0, 0)
    # the state round trip needs no device; a state of the other class is refused by both, and says why
    again = SpaceTimeCopula.from_state_dict(cop.state_dict())
    assert torch.equal(again.step_factor, cop.step_factor) and torch.equal(again.factor_t, cop.factor_t)
    assert torch.equal(again.step_correlation, cop.step_correlation) and again.steps == 3 and again.nodes == 4
    assert again.step_shrinkage == 0.0 and again.step_pairs is None
    foreign = GaussianCopula.from_correlation(r, TAUS, device="cpu").state_dict()
    with pytest.raises(ValueError, match="no step_shrinkage.*GaussianCopula"):
        SpaceTimeCopula.from_state_dict(foreign)
    with pytest.raises(ValueError, match="no step_shrinkage, steps, step_correlation, .*step_factor.*GaussianCopula"):
        SpaceTimeCopula(TAUS).load_state_dict(foreign)
    with pytest.raises(ValueError, match="saved by a SpaceTimeCopula"):
        GaussianCopula.from_state_dict(cop.state_dict())
    with pytest.raises(ValueError, match="saved for levels"):
        SpaceTimeCopula(TAUS, tails="clamp").load_state_dict(cop.state_dict())


def test_copula_uniforms_refuses_a_step_factor_that_does_not_fit():
    from stemgnn_amd import ops
    from stemgnn_amd._lib import StemGNNHipError
    with pytest.raises(StemGNNHipError):                                        # the device check comes first: nothing runs on a CPU
        ops.copula_uniforms(torch.eye(4), 2, 3, 2, 0, 5, step_factor=torch.eye(2))


def test_scenario_rounds_refuses_a_copula_of_fewer_steps():
    from stemgnn_amd import Model, trainer
    from stemgnn_amd.engine import scenario_rounds
    from stemgnn_amd.math_utils import SpaceTimeCopula
    model = Model(6, 2, 4, 2, horizon=3, quantiles=TAUS)
    loader = [(torch.zeros(2, 4, 6), torch.zeros(2, 5, 6))]
    short = SpaceTimeCopula.from_correlations(np.eye(6), T.decay(2, 0.8), TAUS, device="cpu")
    called = []
    model.predict = lambda *a, **k: called.append(1)                            # the model must not be touched
    for _ in range(2):
        with pytest.raises(ValueError, match="couples 2 steps, a round of the model has 3"):
            scenario_rounds(model, loader[0][0], 5, 4, 0, 0, short, "linear", {})
        with pytest.raises(ValueError, match="couples 2 steps"):
            trainer.rolling_scenarios(model, loader, 5, paths=4, coupling=short)
        assert model.training and not called


def test_the_restatement_clears_the_statistical_conditions():
    """The case of tests/test_hip_steps_copula.py::test_the_step_coupling_shows_in_the_scores at its seed, by numpy alone, under
    the same conditions (the issue's: half the smallest margin of its five seeds).  The figures are printed."""
    case = T.steps_case(STAT_SEED)
    out = T.steps_case_restated(case)
    y = case["y_new"]
    whole = {k: T.path_energy(y, out[k]) for k in ("space", "steps")}
    marg = {k: T.crps_and_energy(y, out[k]) for k in ("space", "steps")}
    event = {k: T.run_event(y, out[k]) for k in ("space", "steps")}
    t_err = float(np.abs(out["step_correlation_raw"] - case["T_true"]).max())
    print(f"whole-trajectory energy {whole}; (crps, per-step energy) {marg}; (odds, brier, base rate) {event}; "
          f"max |T_raw - T_true| {t_err:.4f}")
    assert whole["space"] - whole["steps"] > 0.035
    assert abs(marg["space"][1] - marg["steps"][1]) < 0.02 and abs(marg["space"][0] - marg["steps"][0]) < 0.005
    assert event["space"][0] <= 0.02 and event["steps"][0] >= 0.08
    assert event["space"][1] - event["steps"][1] > 0.003
    assert t_err < 0.15
    assert int(out["step_pairs"].min()) == T.STEPS_FIT * T.STEPS_N
