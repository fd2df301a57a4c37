"""CPU: the simultaneous-band entry of include/stemgnn_hip.h (csrc/envelope.hip) is exported, declared and bound; every bad
argument is refused before any launch; the Python layers refuse what they cannot run before anything reaches a GPU;
EnvelopeCalibrator picks the rank it says and round-trips through its state_dict; the numpy restatement
(tests/helpers/envelope_ref.py) agrees with hand-worked values and alone meets the conditions of the statistical case of
tests/test_hip_envelope.py at that test's seed.  Nothing is launched."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import envelope_ref as E

SG_EINVAL = -10001
SEED = 20261021
P = 64                          # stand-in device addresses: every call below is refused before any use
ENV = dict(paths=P, mult=None, total=0, target=2 * P, ignore_nan=0, multiplier=None, multiplier_n=0, count=5, S=33, H=12, C=70,
           coverage=0.9, moments=3 * P, depth=4 * P, chosen=5 * P, truth=6 * P, bands=7 * P)


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def refused(f, **change):
    return f(*{**ENV, **change}.values(), None) == SG_EINVAL


def test_symbol_exported_declared_and_bound(lib):
    import stemgnn_amd
    from stemgnn_amd import _lib, engine, math_utils, ops, trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    name = "stemgnn_scenario_envelope"
    assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in header
    assert len(_lib.SIGNATURES[name][1]) == 18 == len(ENV) + 1
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "envelope.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    assert tuple(inspect.signature(ops.scenario_envelope).parameters) == (
        "paths", "coverage", "target", "mult", "total", "multiplier", "ignore_nan", "return_depth")
    assert tuple(inspect.signature(math_utils.simultaneous_bands).parameters) == (
        "paths", "coverage", "on", "target", "calibrator", "ignore_nan", "return_depth")
    assert tuple(inspect.signature(math_utils.ScenarioSet.envelope).parameters)[1:] == (
        "coverage", "on", "target", "calibrator", "ignore_nan", "return_depth")
    assert tuple(inspect.signature(math_utils.EnvelopeCalibrator.__init__).parameters)[1:] == ("coverage", "per_column")
    assert tuple(inspect.signature(math_utils.joint_coverage).parameters) == ("y", "lo", "hi", "ignore_nan")
    assert tuple(inspect.signature(trainer.scenario_envelopes).parameters) == (
        "model", "loader", "horizon", "coverage", "paths", "seed", "adjacency", "coupling", "tails", "origin", "on", "calibrator",
        "ignore_nan")
    assert tuple(inspect.signature(engine.LiveForecaster.envelope).parameters)[1:] == (
        "coverage", "paths", "horizon", "seed", "coupling", "tails", "on", "calibrator")
    assert inspect.signature(trainer.score_forecast).parameters["envelope"].default is None
    for n in ("PathEnvelope", "EnvelopeCalibrator", "simultaneous_bands", "joint_coverage"):
        assert getattr(stemgnn_amd, n) is getattr(math_utils, n) and n in stemgnn_amd.__all__


def test_the_entry_rejects_bad_arguments(lib):
    f = lib.stemgnn_scenario_envelope
    for k in ("paths", "moments", "chosen", "bands"):
        assert refused(f, **{k: None}), k
    assert refused(f, target=None) and refused(f, truth=None)                     # one without the other
    for k in ("count", "S", "H", "C"):
        for v in (0, -1):
            assert refused(f, **{k: v}), (k, v)
    assert refused(f, S=1025) and refused(f, H=257)
    for c in (0.0, 1.0, -0.1, 1.5, float("nan"), float("inf")):
        assert refused(f, coverage=c), c
    for n in (0, 2, 69, 71, -1):
        assert refused(f, multiplier=8 * P, multiplier_n=n), n
    for t in (0, -1, 2 ** 24 + 1):
        assert refused(f, mult=9 * P, total=t), t
    assert refused(f, count=2 ** 20, S=1024, H=1, C=2)                             # count * S * C
    assert refused(f, count=2 ** 20, S=1, H=256, C=8)                              # count * H * C
    assert refused(f, count=1, S=1024, H=256, C=2 ** 13)                           # S * H * C
    assert refused(f, count=2 ** 31 - 1, S=1, H=1, C=2)


def test_ops_refuse_before_touching_the_library(monkeypatch):
    from stemgnn_amd import _lib, ops
    from stemgnn_amd._lib import StemGNNHipError

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    x, y = torch.zeros(2, 5, 3, 4), torch.zeros(2, 3, 4)
    for bad in (x[0], torch.zeros(2, 5, 3, 0), np.zeros((2, 5, 3, 4), np.float32)):
        with pytest.raises(StemGNNHipError, match=r"non-empty \[count,S,H,C\]"):
            ops.scenario_envelope(bad, 0.9)
    for bad in (x.double(), x.transpose(1, 2)):
        with pytest.raises(StemGNNHipError, match="contiguous float32"):
            ops.scenario_envelope(bad, 0.9)
    for bad in (torch.zeros(1, 1025, 1, 1), torch.zeros(1, 1, 257, 1)):
        with pytest.raises(StemGNNHipError, match="at most 1024 paths"):
            ops.scenario_envelope(bad, 0.9)
    for c in (0.0, 1.0, -0.5, 2, float("nan"), True, "0.9", None):
        with pytest.raises(StemGNNHipError, match=r"coverage must be a number inside \(0, 1\)"):
            ops.scenario_envelope(x, c)
    for m in (torch.ones(3), torch.ones(5), torch.ones(2, 4), [1.0, 2.0]):
        with pytest.raises(StemGNNHipError, match=r"multiplier must be a scalar, \[1\] or \[4\]"):
            ops.scenario_envelope(x, 0.9, multiplier=m)
    with pytest.raises(StemGNNHipError, match="mult and total go together"):
        ops.scenario_envelope(x, 0.9, mult=torch.ones(2, 5, dtype=torch.int32))
    for m in (torch.ones(2, 5), torch.ones(2, 4, dtype=torch.int32)):
        with pytest.raises(StemGNNHipError, match="mult must be a contiguous int32"):
            ops.scenario_envelope(x, 0.9, mult=m, total=5)
    for t in (0, 2 ** 24 + 1, 5.0, True):
        with pytest.raises(StemGNNHipError, match="total must be an integer"):
            ops.scenario_envelope(x, 0.9, mult=torch.ones(2, 5, dtype=torch.int32), total=t)
    for t in (y[0], y.double(), torch.zeros(2, 4, 3).transpose(1, 2)):
        with pytest.raises(StemGNNHipError, match="target must be a contiguous float32"):
            ops.scenario_envelope(x, 0.9, target=t)
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):                 # a host tensor: no fallback
        ops.scenario_envelope(x, 0.9, target=y, multiplier=torch.ones(4), return_depth=True)


def test_python_layers_have_no_cpu_fallback_and_check_their_arguments():
    from stemgnn_amd import math_utils, trainer
    from stemgnn_amd._lib import StemGNNHipError
    y, p = torch.zeros(2, 3, 4), torch.zeros(2, 5, 3, 4)
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        math_utils.simultaneous_bands(p, target=y)
    with pytest.raises(StemGNNHipError, match=r"\[count,S,H,N\]"):
        math_utils.simultaneous_bands(y)
    with pytest.raises(StemGNNHipError, match="coverage must be"):
        math_utils.simultaneous_bands(p, coverage=1.0)
    with pytest.raises(ValueError, match="no groups"):
        math_utils.simultaneous_bands(p, on=math_utils.EventSpec(0.5))
    with pytest.raises(ValueError, match="fitted EnvelopeCalibrator"):
        math_utils.simultaneous_bands(p, calibrator=math_utils.EnvelopeCalibrator())
    with pytest.raises(ValueError, match="fitted EnvelopeCalibrator"):
        math_utils.simultaneous_bands(p, calibrator=2.0)
    per_column = math_utils.EnvelopeCalibrator(0.9, per_column=True).fit(torch.rand(20, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="fitted per column on 3 columns, the paths have 4"):
        math_utils.simultaneous_bands(p, calibrator=per_column)
    for c in (0.0, 1.0, float("nan"), True, None):
        with pytest.raises(ValueError, match="coverage must be"):
            math_utils.EnvelopeCalibrator(c)
    with pytest.raises(ValueError, match="truth"):
        math_utils.EnvelopeCalibrator().fit(torch.zeros(3))
    with pytest.raises(ValueError, match="goes with paths="):
        trainer.score_forecast(torch.zeros(2, 3, 3, 4), y, quantiles=(0.1, 0.5, 0.9), envelope=0.9)
    with pytest.raises(ValueError, match="goes with paths="):
        trainer.score_forecast(y, y, paths=p, envelope=0.9)
    with pytest.raises(ValueError, match="needs a quantile model"):
        trainer.scenario_envelopes(torch.nn.Linear(1, 1), [], 3)
    a = math_utils.PathEnvelope(torch.zeros(2, 2, 3, 4), torch.zeros(2, 2, 3, 4, dtype=torch.float64),
                                torch.ones(2, 4, dtype=torch.float64), torch.ones(2, 4, dtype=torch.float64),
                                torch.tensor([[0.5, 1.0, 1.5, float("nan")]] * 2, dtype=torch.float64))
    assert a.inside.tolist() == [[True, True, False, False]] * 2                   # NaN: absent, not inside
    overall, column = a.joint_coverage()
    assert overall == 4 / 6 and column[:3].tolist() == [1.0, 1.0, 0.0] and np.isnan(column[3])
    assert a.width().tolist() == [0.0, 0.0, 0.0] and a.center.shape == a.scale.shape == (2, 3, 4)
    both = math_utils.PathEnvelope.cat([a, a])
    assert both.count == 4 and both.truth.shape == (4, 4) and both.multiplier.shape == (4, 4) and both.depth is None
    with pytest.raises(ValueError, match="share H and C"):
        math_utils.PathEnvelope.cat([a, math_utils.PathEnvelope(torch.zeros(2, 2, 3, 5), torch.zeros(2, 2, 3, 5),
                                                                torch.ones(2, 5), torch.ones(2, 5))])
    with pytest.raises(ValueError, match="without a target"):
        math_utils.PathEnvelope(a.bands, a.moments, a.chosen, a.multiplier).inside


def test_joint_coverage_of_any_band():
    from stemgnn_amd.math_utils import joint_coverage
    nan = float("nan")
    y = torch.tensor([[[0.0, 0.0], [0.0, 2.0]], [[1.0, nan], [nan, nan]], [[0.5, 0.0], [-1.0, 0.0]]])   # [3, 2, 2]
    lo, hi = -torch.ones(3, 2, 2), torch.ones(3, 2, 2)
    # pairs (origin, column): (0,0) in, (0,1) out at step 1, (1,0) a NaN step, (1,1) all NaN, (2,0) in (on the edge), (2,1) in
    assert joint_coverage(y, lo, hi) == 3 / 6
    assert joint_coverage(y, lo, hi, ignore_nan=True) == 4 / 5
    assert np.isnan(joint_coverage(y[1:2, :, 1:], lo[1:2, :, 1:], hi[1:2, :, 1:], ignore_nan=True))


def test_the_calibrator_picks_the_rank_it_says():
    from stemgnn_amd.math_utils import EnvelopeCalibrator
    inf, nan = float("inf"), float("nan")
    # c = 0.9: m = 0 -> k = 1 > 0; m = 8 -> k = ceil(8.1) = 9 > 8; m = 9 -> k = 9, the largest; m = 10 -> k = ceil(9.9) = 10
    for m, want in ((0, inf), (8, inf), (9, 9.0), (10, 10.0)):
        assert E.rank(m, 0.9) == (1 if m == 0 else m if m >= 9 else 9)
        d = torch.arange(m, 0, -1, dtype=torch.float64).reshape(m, 1)              # m .. 1, so the k-th smallest is k
        cal = EnvelopeCalibrator(0.9).fit(d)
        assert cal.multiplier.dtype == torch.float64 and cal.multiplier.tolist() == [want] and cal.counts.tolist() == [m]
        padded = torch.cat([d, torch.full((3, 1), nan, dtype=torch.float64)])      # NaN depths are no depths
        assert EnvelopeCalibrator(0.9).fit(padded).multiplier.tolist() == [want]
        assert E.calibrated_multiplier(padded.numpy(), 0.9) == want
    assert E.rank(19, 0.5) == 10 and E.rank(9, 0.9) == 9                           # an integral (m + 1) c is not pushed up
    assert EnvelopeCalibrator(0.5).fit(torch.arange(19.0).reshape(19, 1)).multiplier.tolist() == [9.0]
    assert np.isnan(EnvelopeCalibrator(0.9).fit(padded, ignore_nan=False).multiplier.item())
    # per column, and pooled over the columns
    t = torch.tensor([[1.0, 30.0], [2.0, 10.0], [3.0, nan], [4.0, 20.0]], dtype=torch.float64)
    cal = EnvelopeCalibrator(0.5, per_column=True).fit(t)                          # k = ceil(2.5) = 3 of 4; k = 2 of 3
    assert cal.multiplier.tolist() == [3.0, 20.0] and cal.counts.tolist() == [4, 3]
    assert EnvelopeCalibrator(0.5).fit(t).multiplier.tolist() == [4.0]             # k = 4 of 7
    rng = np.random.default_rng(SEED)
    d = rng.random((257, 3))
    d[rng.random(d.shape) < 0.1] = np.nan
    for c in (0.5, 0.8, 0.9, 0.99, 0.999):
        got = EnvelopeCalibrator(c, per_column=True).fit(torch.from_numpy(d)).multiplier.tolist()
        assert got == [E.calibrated_multiplier(d[:, j], c) for j in range(3)]
        assert EnvelopeCalibrator(c).fit(torch.from_numpy(d)).multiplier.tolist() == [E.calibrated_multiplier(d, c)]


def test_state_dict_round_trip():
    from stemgnn_amd.math_utils import EnvelopeCalibrator, PathEnvelope
    truth = torch.rand(50, 3, dtype=torch.float64)
    env = PathEnvelope(torch.zeros(50, 2, 1, 3), torch.zeros(50, 2, 1, 3, dtype=torch.float64), truth.clone(), truth.clone(), truth)
    for per_column in (False, True):
        cal = EnvelopeCalibrator(0.8, per_column).fit(env)                         # an envelope stands for its truth
        assert cal.multiplier.shape == ((3,) if per_column else (1,))
        state = cal.state_dict()
        assert set(state) == {"coverage", "per_column", "multiplier", "counts"}
        new = EnvelopeCalibrator.from_state_dict(state)
        assert (new.coverage, new.per_column) == (0.8, per_column)
        assert torch.equal(new.multiplier, cal.multiplier) and torch.equal(new.counts, cal.counts)
        assert new.multiplier.dtype == torch.float64 and new.counts.dtype == torch.int64
        with pytest.raises(ValueError, match="saved for coverage"):
            EnvelopeCalibrator(0.8, not per_column).load_state_dict(state)
        with pytest.raises(ValueError, match="saved for coverage"):
            EnvelopeCalibrator(0.9, per_column).load_state_dict(state)
    unfitted = EnvelopeCalibrator.from_state_dict(EnvelopeCalibrator(0.7).state_dict())
    assert unfitted.multiplier is None and unfitted.counts is None
    with pytest.raises(ValueError, match="do not fit"):
        EnvelopeCalibrator(0.8).load_state_dict(dict(coverage=0.8, per_column=False, multiplier=torch.ones(3),
                                                     counts=torch.ones(3)))


def test_the_restatement_on_hand_worked_values():
    nan, inf = np.nan, np.inf
    # one origin, one column, S = 4, H = 2: step 0 holds 1, 2, 3, 6 (m = 3, v = 3.5), step 1 is constant (s = 0)
    x = np.array([[1, 5], [2, 5], [3, 5], [6, 5]], np.float32).reshape(1, 4, 2, 1)
    y = np.array([4.0, 5.0], np.float32).reshape(1, 2, 1)
    out = E.envelope(x, 0.5, target=y)
    s = np.sqrt(3.5)
    assert out["moments"][0, :, :, 0].tolist() == [[3.0, 5.0], [s, 0.0]]
    assert out["depth"][0, :, 0].tolist() == [2.0 / s, 1.0 / s, 0.0, 3.0 / s]
    assert out["chosen"][0, 0] == 2.0 / s                                          # k = ceil(2.5) = 3: the third smallest depth
    assert out["truth"][0, 0] == 1.0 / s
    lo, hi = 3.0 - (2.0 / s) * s, 3.0 + (2.0 / s) * s
    assert out["bands"][0, :, :, 0].tolist() == [[np.float32(lo), 5.0], [np.float32(hi), 5.0]]
    # off the centre of the constant step the truth is outside every finite band
    y[0, 1, 0] = 5.5
    assert E.envelope(x, 0.5, target=y)["truth"][0, 0] == inf
    y[0, 1, 0] = nan
    assert np.isnan(E.envelope(x, 0.5, target=y)["truth"][0, 0])
    assert E.envelope(x, 0.5, target=y, ignore_nan=True)["truth"][0, 0] == 1.0 / s
    # k > T: the band is the whole line, whatever the scale
    out = E.envelope(x, 0.9)
    assert out["chosen"][0, 0] == inf and out["bands"][0, :, :, 0].tolist() == [[-inf, -inf], [inf, inf]] and out["truth"] is None
    # a given multiplier; weights: member 3 counted twice, member 0 not read
    out = E.envelope(x, 0.5, multiplier=[2.0])
    assert out["bands"][0, :, 0, 0].tolist() == [np.float32(3.0 - 2.0 * s), np.float32(3.0 + 2.0 * s)]
    x[0, 0] = nan
    out = E.envelope(x, 0.5, mult=[[0, 1, 1, 2]], total=4)
    same = E.envelope(np.array([[2, 5], [3, 5], [6, 5], [6, 5]], np.float32).reshape(1, 4, 2, 1), 0.5)
    assert np.array_equal(out["moments"], same["moments"]) and out["chosen"][0, 0] == same["chosen"][0, 0]
    assert np.isnan(out["depth"][0, 0, 0]) and out["depth"][0, 1:, 0].tolist() == same["depth"][0, :3, 0].tolist()
    for mult, total in (([[0, 1, 1, 1]], 4), ([[-1, 2, 2, 1]], 4)):                # a wrong sum, a negative weight
        out = E.envelope(x, 0.5, mult=mult, total=total)
        assert all(np.isnan(out[k]).all() for k in ("moments", "depth", "chosen", "bands"))
    assert np.isnan(E.envelope(x, 0.5)["chosen"][0, 0])                            # the NaN member counts again: absent


def test_the_statistical_case_by_the_restatement_alone():
    """The conditions of test_hip_envelope.test_the_statistical_case at its seed, by numpy alone (figures printed): a
    driftless random walk, 4096 origins of 32 exchangeable paths over 8 steps, coverage 0.9: the pointwise band between ranks 2
    and 31 holds the whole trajectory < 0.70 of the time; the ensemble's own multiplier in [0.82, 0.895]; the multiplier
    calibrated on the first half within 0.025 of 0.9 on the second, and >= 0.95 at every single step."""
    paths, y = E.random_walk_case(SEED)
    pointwise, ensemble, calibrated, per_step, q = E.statistical_figures(paths, y)
    print(f"restatement: pointwise {pointwise:.4f}, ensemble {ensemble:.4f}, calibrated {calibrated:.4f}, lowest step "
          f"{per_step:.4f}, multiplier {q:.4f}")
    assert pointwise < 0.70 and 0.82 <= ensemble <= 0.895 and abs(calibrated - 0.9) <= 0.025 and per_step >= 0.95
