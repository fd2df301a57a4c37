"""CPU: the scenario-event entries of include/stemgnn_hip.h (csrc/events.hip) are exported, declared and bound; every bad
argument is refused before any launch; the Python layers refuse what they cannot run before anything reaches a GPU;
group_weights has its values; the numpy restatement (tests/helpers/events_ref.py) agrees with hand-worked cases, and alone meets
the conditions of the statistical case of tests/test_hip_events.py at that test's seed.  Nothing is launched."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import copula_ref as C
from tests.helpers import events_ref as E

SG_EINVAL = -10001
SEED = 20261020
P = 64                          # stand-in device addresses: every call below is refused before any use
NEW = ("stemgnn_scenario_aggregate", "stemgnn_scenario_events")
AGG = dict(x=P, weights=2 * P, mul=3 * P, add=4 * P, rows=70, N=228, R=8, out=5 * P)
EVT = dict(paths=P, thr=2 * P, mul=3 * P, add=4 * P, count=5, S=33, H=12, M=70, above=1, min_run=3, counts=5 * P)


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == SG_EINVAL


def test_symbols_exported_declared_and_bound(lib):
    import stemgnn_amd
    from stemgnn_amd import _lib, engine, math_utils, ops, trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert len(_lib.SIGNATURES["stemgnn_scenario_aggregate"][1]) == 9
    assert len(_lib.SIGNATURES["stemgnn_scenario_events"][1]) == 12
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "events.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    assert tuple(inspect.signature(ops.scenario_aggregate).parameters) == ("x", "weights", "mul", "add")
    assert tuple(inspect.signature(ops.scenario_events).parameters) == ("paths", "threshold", "above", "min_run", "mul", "add")
    assert tuple(inspect.signature(math_utils.EventSpec.__init__).parameters)[1:] == \
        ("threshold", "above", "min_run", "groups", "reduce", "mul", "add")
    assert tuple(inspect.signature(math_utils.group_weights).parameters) == ("groups", "N", "reduce")
    for name in ("EventSpec", "ScenarioEvents", "EventScores", "group_weights"):
        assert getattr(stemgnn_amd, name) is getattr(math_utils, name) and name in stemgnn_amd.__all__
    par = inspect.signature(trainer.rolling_scenarios).parameters
    assert tuple(par)[-2:] == ("origin", "events") and par["events"].default is None
    par = inspect.signature(trainer.score_forecast).parameters
    assert tuple(par)[-1] == "events" and par["events"].default is None
    assert tuple(inspect.signature(engine.LiveForecaster.event_odds).parameters)[1:] == \
        ("spec", "paths", "horizon", "seed", "coupling", "tails")


def test_aggregate_rejects_bad_arguments(lib):
    f = lib.stemgnn_scenario_aggregate
    for k in ("x", "weights", "out"):
        assert refused(f, AGG, **{k: None}), k
    assert refused(f, AGG, add=None) and refused(f, AGG, mul=None)                # one without the other
    for k in ("rows", "N", "R"):
        for v in (0, -1):
            assert refused(f, AGG, **{k: v}), (k, v)
    assert refused(f, AGG, R=33) and refused(f, AGG, N=4097)
    assert refused(f, AGG, rows=2 ** 31, R=1) and refused(f, AGG, rows=2 ** 26, R=32)   # rows * R
    assert refused(f, AGG, rows=2 ** 40)


def test_events_reject_bad_arguments(lib):
    f = lib.stemgnn_scenario_events
    for k in ("paths", "thr", "counts"):
        assert refused(f, EVT, **{k: None}), k
    assert refused(f, EVT, add=None) and refused(f, EVT, mul=None)
    for k in ("count", "S", "H", "M"):
        for v in (0, -1):
            assert refused(f, EVT, **{k: v}), (k, v)
    assert refused(f, EVT, S=1025) and refused(f, EVT, H=257)
    assert refused(f, EVT, min_run=0) and refused(f, EVT, min_run=13) and refused(f, EVT, min_run=-1)
    assert refused(f, EVT, above=2) and refused(f, EVT, above=-1)
    assert refused(f, EVT, S=1024, H=256, M=2 ** 13, min_run=1)                   # S * H * M
    assert refused(f, EVT, S=1, H=256, M=2 ** 22, min_run=1)                      # (2 H + 1) * M
    assert refused(f, EVT, count=2 ** 31, S=1, H=1, M=1, min_run=1)               # the grid
    assert refused(f, EVT, count=2 ** 26, S=1, H=1, M=64 * 32 + 1, min_run=1)     # count * ceil(M / 64)


def test_ops_refuse_before_touching_the_library(monkeypatch):
    from stemgnn_amd import _lib, ops
    from stemgnn_amd._lib import StemGNNHipError

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    x, w = torch.zeros(2, 5, 3, 4), torch.ones(2, 4, dtype=torch.float64)
    for bad_w in (torch.ones(4), torch.ones(2, 5), torch.ones(0, 4), torch.ones(2, 3, 4), [[1, 1, 1, 1]]):
        with pytest.raises(StemGNNHipError, match=r"weights must be a \[R,4\]"):
            ops.scenario_aggregate(x, bad_w)
    with pytest.raises(StemGNNHipError, match="at most 32 groups"):
        ops.scenario_aggregate(x, torch.ones(33, 4))
    with pytest.raises(StemGNNHipError, match="at most 32 groups"):
        ops.scenario_aggregate(torch.zeros(2, 4097), torch.ones(1, 4097))
    for bad_x in (x.double(), x.half(), x.long(), torch.zeros(2, 5, 4, 3).transpose(2, 3), torch.zeros(2, 8)[:, ::2]):
        with pytest.raises(StemGNNHipError, match="contiguous float32"):
            ops.scenario_aggregate(bad_x, w)
    for bad_x in (torch.zeros(()), torch.zeros(0, 4), np.zeros((2, 4), np.float32)):
        with pytest.raises(StemGNNHipError, match="non-empty"):
            ops.scenario_aggregate(bad_x, w)
    with pytest.raises(StemGNNHipError, match="mul and add go together"):
        ops.scenario_aggregate(x, w, mul=torch.ones(4))
    with pytest.raises(StemGNNHipError, match="mul must be a scalar or 4 values"):
        ops.scenario_aggregate(x, w, mul=torch.ones(3), add=torch.ones(4))
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):                 # a host tensor: no fallback
        ops.scenario_aggregate(x, w)
    for bad_p in (x[0], torch.zeros(2, 5, 3, 0), torch.zeros(2, 5, 3, 4, 1)):
        with pytest.raises(StemGNNHipError, match=r"non-empty \[count,S,H,M\]"):
            ops.scenario_events(bad_p, 0.0)
    for bad_p in (x.double(), x.int(), x.transpose(1, 2)):
        with pytest.raises(StemGNNHipError, match="contiguous float32"):
            ops.scenario_events(bad_p, 0.0)
    with pytest.raises(StemGNNHipError, match="at most 1024 paths"):
        ops.scenario_events(torch.zeros(1, 1025, 1, 1), 0.0)
    with pytest.raises(StemGNNHipError, match="at most 1024 paths"):
        ops.scenario_events(torch.zeros(1, 1, 257, 1), 0.0)
    for bad_run in (0, 4, -1, 1.5, True):
        with pytest.raises(StemGNNHipError, match="min_run must be an integer within"):
            ops.scenario_events(x, 0.0, min_run=bad_run)
    for bad_thr in (torch.zeros(3), np.zeros((4, 1)), [0.0, 1.0]):
        with pytest.raises(StemGNNHipError, match="threshold must be a scalar or 4 values"):
            ops.scenario_events(x, bad_thr)
    with pytest.raises(StemGNNHipError, match="mul and add go together"):
        ops.scenario_events(x, 0.0, add=torch.ones(4))
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        ops.scenario_events(x, 0.0)


def test_python_layers_have_no_cpu_fallback_and_check_their_arguments():
    from stemgnn_amd import math_utils, trainer
    from stemgnn_amd._lib import StemGNNHipError
    y, p = torch.zeros(2, 3, 4), torch.zeros(2, 5, 3, 4)
    spec = math_utils.EventSpec(0.5, groups=[[0, 1], [2, 3]])
    for call in (lambda: spec.count(p), lambda: spec.aggregate(p), lambda: spec.realised(y),
                 lambda: math_utils.EventSpec(0.5).count(p), lambda: math_utils.EventSpec(0.5).realised(y)):
        with pytest.raises(StemGNNHipError, match="no CPU fallback"):
            call()
    with pytest.raises(StemGNNHipError):
        spec.count(y)
    with pytest.raises(ValueError, match="no groups"):
        math_utils.EventSpec(0.5).aggregate(p)
    with pytest.raises(ValueError, match="index outside"):
        math_utils.EventSpec(0.5, groups=[[0, 4]]).count(p)
    for kw in (dict(min_run=0), dict(min_run=1.5), dict(reduce="max"), dict(mul=torch.ones(4))):
        with pytest.raises(ValueError):
            math_utils.EventSpec(0.5, **kw)
    with pytest.raises(ValueError, match="goes with paths="):
        trainer.score_forecast(torch.zeros(2, 3, 3, 4), y, quantiles=(0.1, 0.5, 0.9), events=spec)
    with pytest.raises(ValueError, match="int32"):
        math_utils.ScenarioEvents(torch.zeros(2, 7, 4), 5)
    a = math_utils.ScenarioEvents(torch.zeros(2, 7, 4, dtype=torch.int32), 5)
    with pytest.raises(ValueError, match="share S, H and M"):
        math_utils.ScenarioEvents.cat([a, math_utils.ScenarioEvents(torch.zeros(2, 7, 4, dtype=torch.int32), 6)])
    with pytest.raises(ValueError, match="realised must be"):
        a.score(a)


def test_group_weights_values():
    from stemgnn_amd.math_utils import group_weights
    w = group_weights([[0, 2, 3], [1], range(5)], 5)
    assert w.dtype == torch.float64 and tuple(w.shape) == (3, 5)
    assert w.tolist() == [[1 / 3, 0, 1 / 3, 1 / 3, 0], [0, 1, 0, 0, 0], [0.2] * 5]
    assert group_weights([[0, 2, 3], [1]], 5, reduce="sum").tolist() == [[1, 0, 1, 1, 0], [0, 1, 0, 0, 0]]
    given = np.array([[0.25, 0.75, 0.0], [0.0, -1.0, 2.0]])
    assert np.array_equal(group_weights(given, 3).numpy(), given)                  # a matrix is used as it is
    assert np.array_equal(group_weights(torch.from_numpy(given).float(), 3).numpy(), given.astype(np.float32))
    assert tuple(group_weights([[i] for i in range(32)], 40).shape) == (32, 40)
    for bad, n in (([[0, 5]], 5), ([[-1]], 5), ([[]], 5), ([[1, 1]], 5), ([], 5), ([[i] for i in range(33)], 40), ([[0.5]], 5),
                   (np.ones((2, 4)), 5), (np.ones((33, 5)), 5), (np.ones(5), 5), ([[0]], 0)):
        with pytest.raises(ValueError):
            group_weights(bad, n)
    with pytest.raises(ValueError):
        group_weights([[0]], 5, reduce="median")


def counts_of(values, thr, above, min_run):
    """one origin, one column: values [S][H] -> (step [H], first [H], run) by both restatements"""
    x = np.array(values, np.float32)[None, :, :, None]
    slow, fast = E.events(x, [thr], above, min_run), E.events_fast(x, [thr], above, min_run)
    assert np.array_equal(slow, fast)
    H = x.shape[2]
    return slow[0, :H, 0].tolist(), slow[0, H:2 * H, 0].tolist(), int(slow[0, 2 * H, 0])


def test_the_restatement_on_hand_worked_values():
    nan, inf = np.nan, np.inf
    # a value equal to the threshold is on neither side
    assert counts_of([[1.0, 2.0, 3.0]], 2.0, True, 1) == ([0, 0, 1], [0, 0, 1], 1)
    assert counts_of([[1.0, 2.0, 3.0]], 2.0, False, 1) == ([1, 0, 0], [1, 0, 0], 1)
    # -0.0 against +0.0: equal, so in neither event
    assert counts_of([[-0.0, 0.0]], 0.0, True, 1) == ([0, 0], [0, 0], 0)
    assert counts_of([[-0.0, 0.0]], -0.0, False, 1) == ([0, 0], [0, 0], 0)
    # a NaN breaks a run and is not a crossing; a NaN threshold admits nothing; infinities compare as numbers
    assert counts_of([[5, 5, nan, 5, 5]], 1.0, True, 3) == ([1, 1, 0, 1, 1], [1, 0, 0, 0, 0], 0)
    assert counts_of([[5, 5, nan, 5, 5]], 1.0, True, 2) == ([1, 1, 0, 1, 1], [1, 0, 0, 0, 0], 1)
    assert counts_of([[nan, nan]], 1.0, False, 1) == ([0, 0], [0, 0], 0)
    assert counts_of([[5, -5]], nan, True, 1) == ([0, 0], [0, 0], 0)
    assert counts_of([[inf, -inf, 0]], inf, True, 1) == ([0, 0, 0], [0, 0, 0], 0)
    assert counts_of([[inf, -inf, 0]], -inf, True, 1) == ([1, 0, 1], [1, 0, 0], 1)
    assert counts_of([[inf, -inf, 0]], inf, False, 2) == ([0, 1, 1], [0, 1, 0], 1)
    # min_run = H: only the path that is in the event throughout
    three = [[2, 2, 2, 2], [2, 2, 2, 0], [0, 2, 2, 2]]
    assert counts_of(three, 1.0, True, 4) == ([2, 3, 3, 2], [2, 1, 0, 0], 1)
    # a run at either end
    assert counts_of(three, 1.0, True, 3) == ([2, 3, 3, 2], [2, 1, 0, 0], 3)
    assert counts_of([[2, 2, 0, 0, 0], [0, 0, 0, 2, 2], [2, 0, 2, 0, 2]], 1.0, True, 2) == ([2, 1, 1, 1, 2], [2, 0, 0, 1, 0], 2)
    # above both ways on the same values
    assert counts_of([[1, 3, 1, 3]], 2.0, True, 1) == ([0, 1, 0, 1], [0, 1, 0, 0], 1)
    assert counts_of([[1, 3, 1, 3]], 2.0, False, 2) == ([1, 0, 1, 0], [1, 0, 0, 0], 0)
    # de-normalisation: 2 * x + 1 against a raw threshold
    x = np.array([0.0, 0.5, 1.0], np.float32).reshape(1, 3, 1, 1)
    assert E.events(x, [2.0], True, 1, mul=[2.0], add=[1.0])[0, :, 0].tolist() == [1, 1, 1]
    assert E.events(x, [2.0], False, 1, mul=[2.0], add=[1.0])[0, :, 0].tolist() == [1, 1, 1]
    # the aggregate: a zero weight keeps a NaN out, a NaN inside a group propagates
    ref, mag = E.aggregate(np.array([[1, nan, 3, 4]], np.float32), np.array([[0.5, 0, 0.5, 0], [0, 1, 0, 1], [0, 0, 0, -2.0]]),
                           mul=[2, 2, 2, 2], add=[1, 1, 1, 1])
    assert ref[0, 0] == 5.0 and np.isnan(ref[0, 1]) and ref[0, 2] == -18.0 and mag[0, 2] == 18.0 and mag[0, 0] == 5.0


def test_brier_from_a_hand_made_table():
    from stemgnn_amd.math_utils import EventScores
    # S = 2; forecasts 0, 1/2, 1 with (n, o) = (4, 1), (2, 1), (4, 3):
    # brier = [1 * 1 + 3 * 0 + 1 * 1/4 + 1 * 1/4 + 3 * 0 + 1 * 1] / 10 = 0.25; base rate 5 / 10; skill = 1 - 0.25 / 0.25 = 0
    t = np.array([[4, 1], [2, 1], [4, 3]], np.int64)
    assert E.brier(t, 2) == (0.25, 0.5, 0.0)
    # a perfect forecast; a constant base rate has no skill to measure
    assert E.brier(np.array([[3, 0], [0, 0], [2, 2]]), 2) == (0.0, 0.4, 1.0)
    b, base, skill = E.brier(np.array([[3, 0], [0, 0], [0, 0]]), 2)
    assert (b, base) == (0.0, 0.0) and np.isnan(skill)
    assert all(np.isnan(v) for v in E.brier(np.zeros((3, 2), np.int64), 2))
    # the table from counts: S = 2, H = 2, M = 1, three origins; forecast counts of "any" = 0, 1, 2; it occurred in the last two
    counts = np.array([[[0], [0], [0], [0], [0]], [[1], [0], [1], [0], [1]], [[2], [1], [2], [0], [1]]], np.int32)
    real = np.array([[[0], [0], [0], [0], [0]], [[0], [1], [0], [1], [0]], [[1], [1], [1], [0], [1]]], np.int32)
    table = E.reliability(counts, 2, real)
    assert table.shape == (4, 1, 3, 2)
    assert table[0, 0].tolist() == [[1, 0], [1, 1], [1, 1]]                        # any
    assert table[1, 0].tolist() == [[1, 0], [2, 1], [0, 0]]                        # run
    assert table[2, 0].tolist() == [[1, 0], [1, 0], [1, 1]] and table[3, 0].tolist() == [[2, 1], [1, 1], [0, 0]]
    missing = np.zeros((3, 2, 1), bool)
    missing[1, 1, 0] = True                                                        # origin 1, step 1: out of any, run and step 1
    masked = E.reliability(counts, 2, real, missing)
    assert masked[0, 0].tolist() == [[1, 0], [0, 0], [1, 1]] and masked[2, 0].tolist() == table[2, 0].tolist()
    assert masked[3, 0].tolist() == [[1, 0], [1, 1], [0, 0]]
    # math_utils.EventScores reads the same figures off the same table
    sc = EventScores(table, 2)
    for k, suffix in ((0, ""), (1, "_run")):
        want = E.brier(table[k, 0], 2)
        got = (getattr(sc, "brier" + suffix), getattr(sc, "base_rate" + suffix), getattr(sc, "skill" + suffix))
        assert np.array_equal(np.array(got), np.array(want), equal_nan=True)
        assert np.array_equal(getattr(sc, "brier" + suffix + "_column"), np.array([want[0]]))
    assert sc.brier_step.tolist() == [E.brier(table[2, 0], 2)[0], E.brier(table[3, 0], 2)[0]]
    assert sc.reliability.shape == (1, 3, 2) and sc.reliability_step.shape == (2, 1, 3, 2) and sc.valid == 3


def test_the_statistical_case_by_the_restatement_alone():
    """The conditions of test_hip_events.test_the_statistical_case at its seed, by numpy alone (figures printed): coverage of the
    truth's 16-node mean by the band between ranks 4 and 29 of the paths' mean: independent < 0.45, path > 0.85,
    |copula - 25/33| <= 0.067; Brier score of "mean > 0.8": independent - copula > 0.004 and path - copula > 0.004."""
    case = C.energy_case(SEED + 7)
    ens = C.energy_case_restated(case)
    fig = E.statistical_figures(case["y_new"], {k: ens[k] for k in ("independent", "path", "copula")})
    print("restatement: " + "; ".join(f"{k}: coverage {c:.4f}, brier {b:.4f}" for k, (c, b) in fig.items()))
    assert fig["independent"][0] < 0.45 and fig["path"][0] > 0.85 and abs(fig["copula"][0] - 25 / 33) <= 0.067
    assert fig["independent"][1] - fig["copula"][1] > 0.004 and fig["path"][1] - fig["copula"][1] > 0.004
