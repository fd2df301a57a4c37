"""CPU: the scenario-reduction entries of include/stemgnn_hip.h (csrc/reduce.hip) are exported, declared and bound; every bad
argument is refused before any launch; the Python layers refuse what they cannot run before anything reaches a GPU; the numpy
restatement (tests/helpers/reduce_ref.py) agrees with hand-worked cases and with brute force over all subsets, and alone meets
the conditions of the two statistical cases of tests/test_hip_reduce.py at that test's seed.  Nothing is launched."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import reduce_ref as R

SG_EINVAL = -10001
SEED = 20261020
P = 64                          # stand-in device addresses: every call below is refused before any use
NEW = ("stemgnn_scenario_distances", "stemgnn_scenario_reduce")
DST = dict(paths=P, scale=2 * P, count=5, S=33, L=70, squared=0, D=3 * P)
RED = dict(D=P, count=5, S=33, K=8, selected=2 * P, counts=3 * P, assign=4 * P, cost=5 * P)


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
    assert len(_lib.SIGNATURES["stemgnn_scenario_distances"][1]) == 8
    assert len(_lib.SIGNATURES["stemgnn_scenario_reduce"][1]) == 9
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "reduce.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    sig = inspect.signature
    assert str(sig(ops.scenario_distances)) == "(paths, scale=None, squared=False)"
    assert str(sig(ops.scenario_reduce)) == \
        "(paths, keep, scale=None, squared=False, distances=None, max_scratch_bytes=268435456)"
    assert str(sig(math_utils.reduce_scenarios)) == "(paths, keep, on=None, scale=None, squared=False)"
    assert str(sig(trainer.reduced_scenarios)) == \
        "(model, loader, horizon, keep, paths=64, seed=0, adjacency=None, coupling='independent', tails='linear', origin=0, " \
        "on=None, scale=None, squared=False)"
    assert str(sig(engine.LiveForecaster.scenario_set)) == \
        "(self, keep, paths=64, horizon=None, seed=None, coupling='independent', tails='linear', on=None, scale=None, " \
        "squared=False)"
    for name in ("expect", "keep_for", "head", "cat"):
        assert callable(getattr(math_utils.ScenarioSet, name)), name
    assert isinstance(math_utils.ScenarioSet.weights, property)
    for name in ("ScenarioSet", "reduce_scenarios"):
        assert getattr(stemgnn_amd, name) is getattr(math_utils, name) and name in stemgnn_amd.__all__
    # the pinned signatures still hold
    par = sig(trainer.rolling_scenarios).parameters
    assert tuple(par) == ("model", "loader", "horizon", "paths", "seed", "adjacency", "coupling", "tails", "return_paths", "origin",
                          "events") and par["events"].default is None
    assert tuple(sig(trainer.score_forecast).parameters)[-1] == "events"
    assert tuple(sig(engine.LiveForecaster.scenarios).parameters)[1:] == \
        ("paths", "horizon", "seed", "coupling", "tails", "return_paths")
    assert tuple(sig(engine.LiveForecaster.event_odds).parameters)[1:] == ("spec", "paths", "horizon", "seed", "coupling", "tails")


def test_distances_reject_bad_arguments(lib):
    f = lib.stemgnn_scenario_distances
    for k in ("paths", "D"):
        assert refused(f, DST, **{k: None}), k
    for k in ("count", "S", "L"):
        for v in (0, -1):
            assert refused(f, DST, **{k: v}), (k, v)
    assert refused(f, DST, S=1025)
    assert refused(f, DST, squared=2) and refused(f, DST, squared=-1)
    assert refused(f, DST, S=1024, L=2 ** 21)                                     # S * L
    assert refused(f, DST, count=2 ** 11, S=1024, L=1)                            # count * S * S
    assert refused(f, DST, count=2 ** 31, S=1, L=1) and refused(f, DST, count=2 ** 40, S=1, L=1)   # count, and the grid


def test_reduce_rejects_bad_arguments(lib):
    f = lib.stemgnn_scenario_reduce
    for k in ("D", "selected", "counts", "assign", "cost"):
        assert refused(f, RED, **{k: None}), k
    for k in ("count", "S"):
        for v in (0, -1):
            assert refused(f, RED, **{k: v}), (k, v)
    assert refused(f, RED, S=1025, K=1)
    for v in (0, -1, 34):
        assert refused(f, RED, K=v), v
    assert refused(f, RED, count=2 ** 11, S=1024) and refused(f, RED, count=2 ** 31, S=1, K=1)   # count * S * S


def test_ops_refuse_before_touching_the_library(monkeypatch):
    from stemgnn_amd import _lib, ops
    from stemgnn_amd._lib import StemGNNHipError

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    x = torch.zeros(2, 5, 3, 4)
    calls = (lambda p, **kw: ops.scenario_distances(p, **kw), lambda p, **kw: ops.scenario_reduce(p, 2, **kw))
    for call in calls:
        for bad_p in (x[0], torch.zeros(2, 5, 3, 0), torch.zeros(2, 5, 3, 4, 1), np.zeros((2, 5, 3, 4), np.float32), None):
            with pytest.raises(StemGNNHipError, match=r"non-empty \[count,S,H,M\]"):
                call(bad_p)
        for bad_p in (x.double(), x.int(), x.transpose(1, 2)):
            with pytest.raises(StemGNNHipError, match="contiguous float32"):
                call(bad_p)
        with pytest.raises(StemGNNHipError, match="at most 1024 paths"):
            call(torch.zeros(1, 1025, 1, 1))
        for bad_s in (torch.ones(3), torch.ones(4, 3), torch.ones(1, 3, 4), np.ones((2, 4)), [1.0, 2.0]):
            with pytest.raises(StemGNNHipError, match=r"scale must be a scalar, \[4\] or \[3,4\]"):
                call(x, scale=bad_s)
        for bad_q in (2, -1, "yes", None, 0.5):
            with pytest.raises(StemGNNHipError, match="squared must be True or False"):
                call(x, squared=bad_q)
        for good in (dict(), dict(scale=2.0), dict(scale=torch.ones(4)), dict(scale=np.ones((3, 4))), dict(squared=True)):
            with pytest.raises(StemGNNHipError, match="no CPU fallback"):         # a host tensor: no fallback
                call(x, **good)
    for bad_k in (0, 6, -1, 1.5, True, None):
        with pytest.raises(StemGNNHipError, match=r"keep must be an integer within \[1, 5\]"):
            ops.scenario_reduce(x, bad_k)
    for bad_b in (0, 5 * 5 * 8 - 1, 1.5, True):
        with pytest.raises(StemGNNHipError, match="max_scratch_bytes must hold one origin's"):
            ops.scenario_reduce(x, 2, max_scratch_bytes=bad_b)
    d = torch.zeros(2, 5, 5, dtype=torch.float64)
    for bad_d in (d[0], torch.zeros(2, 5, 4, dtype=torch.float64), torch.zeros(0, 5, 5, dtype=torch.float64), d.numpy()):
        with pytest.raises(StemGNNHipError, match=r"distances must be a non-empty \[count,S,S\]"):
            ops.scenario_reduce(None, 2, distances=bad_d)
    for bad_d in (d.float(), d.transpose(1, 2)):
        with pytest.raises(StemGNNHipError, match="contiguous float64"):
            ops.scenario_reduce(None, 2, distances=bad_d)
    with pytest.raises(StemGNNHipError, match="at most 1024 paths"):
        ops.scenario_reduce(None, 2, distances=torch.zeros(1, 1025, 1025, dtype=torch.float64))
    with pytest.raises(StemGNNHipError, match="with the distances' count = 2 and S = 5"):
        ops.scenario_reduce(torch.zeros(2, 6, 3, 4), 2, distances=d)
    with pytest.raises(StemGNNHipError, match=r"keep must be an integer within \[1, 5\]"):
        ops.scenario_reduce(None, 6, distances=d)
    for p in (None, x):
        with pytest.raises(StemGNNHipError, match="distances is on cpu.*no CPU fallback"):
            ops.scenario_reduce(p, 2, distances=d)


def test_python_layers_have_no_cpu_fallback_and_check_their_arguments(monkeypatch):
    from stemgnn_amd import _lib, math_utils, trainer
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import EventSpec, ScenarioSet, reduce_scenarios

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    p = torch.zeros(2, 5, 3, 4)
    spec = EventSpec(0.5, groups=[[0, 1], [2, 3]])
    for call in (lambda: reduce_scenarios(p, 2), lambda: reduce_scenarios(p, 2, on=spec),
                 lambda: reduce_scenarios(p, 2, on=torch.zeros(2, 5, 3, 2)),
                 lambda: reduce_scenarios(p, 2, scale=0.5, squared=True)):
        with pytest.raises(StemGNNHipError, match="no CPU fallback"):
            call()
    with pytest.raises(StemGNNHipError, match=r"paths must be \[count,S,H,N\]"):
        reduce_scenarios(p[0], 2)
    for bad_on in (torch.zeros(2, 5, 3), torch.zeros(2, 4, 3, 2), torch.zeros(3, 5, 3, 2), torch.zeros(2, 5, 2, 4)):
        with pytest.raises(StemGNNHipError, match=r"on must be \[count,S,H,R\]"):
            reduce_scenarios(p, 2, on=bad_on)
    with pytest.raises(ValueError, match="no groups="):
        reduce_scenarios(p, 2, on=EventSpec(0.5))
    with pytest.raises(StemGNNHipError, match="keep must be an integer within"):
        reduce_scenarios(p, 6)
    with pytest.raises(StemGNNHipError, match=r"scale must be a scalar, \[2\] or \[3,2\]"):    # the scale is the aggregate's
        reduce_scenarios(p, 2, on=torch.zeros(2, 5, 3, 2), scale=torch.ones(4))
    with pytest.raises(ValueError, match="needs a quantile model"):
        trainer.reduced_scenarios(object(), [], 3, 2)

    def a_set(S=5, K=2, H=3, N=4, **kw):
        return ScenarioSet(torch.zeros(2, K, dtype=torch.int64), torch.ones(2, K, dtype=torch.int32),
                           torch.zeros(2, S, dtype=torch.int32), torch.zeros(2, K, dtype=torch.float64), S, torch.zeros(2, K, H, N),
                           **kw)

    with pytest.raises(ValueError, match="index must be int64"):
        ScenarioSet(torch.zeros(2, 2, dtype=torch.int32), torch.ones(2, 2, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32),
                    torch.zeros(2, 2, dtype=torch.float64), 5, torch.zeros(2, 2, 3, 4))
    for other in (a_set(S=6), a_set(K=3), a_set(H=2), a_set(N=5)):
        with pytest.raises(ValueError, match="share S, K, H and N"):
            ScenarioSet.cat([a_set(), other])
    with pytest.raises(ValueError, match="share S, K, H and N"):
        ScenarioSet.cat([])
    with pytest.raises(ValueError, match=r"needs `distances` .* or `source` .* holds neither"):
        a_set().head(1)
    for bad_k in (0, 3, 1.5, True):
        with pytest.raises(ValueError, match=r"k must be an integer within \[1, 2\]"):
            a_set().head(bad_k)
    with pytest.raises(ValueError, match=r"values must be \[count, S, ...\]"):
        a_set().expect(torch.zeros(2, 4))
    # what needs no kernel runs on the host as it stands: head from retained distances, weights, expect, keep_for
    D = torch.tensor([[0.0, 1.0, 3.0], [1.0, 0.0, 2.0], [3.0, 2.0, 0.0]], dtype=torch.float64)[None]
    full = ScenarioSet(torch.tensor([[1, 2]]), torch.tensor([[2, 1]], dtype=torch.int32),
                       torch.tensor([[0, 0, 1]], dtype=torch.int32),
                       torch.tensor([[1.0, 1.0 / 3.0]], dtype=torch.float64), 3, torch.zeros(1, 2, 1, 1), distances=D)
    one = full.head(1)
    assert one.index.tolist() == [[1]] and one.counts.tolist() == [[3]] and one.assign.tolist() == [[0, 0, 0]]
    assert one.cost.tolist() == [[1.0]] and one.K == 1 and tuple(one.paths.shape) == (1, 1, 1, 1)
    two = full.head(2)
    assert two.counts.tolist() == [[2, 1]] and two.assign.tolist() == [[0, 0, 1]]
    assert full.weights.tolist() == [[2 / 3, 1 / 3]]
    assert full.expect(torch.tensor([[10.0, 20.0, 50.0]])).tolist() == [2 / 3 * 20.0 + 1 / 3 * 50.0]
    assert full.keep_for(1.0).tolist() == [1] and full.keep_for(0.5).tolist() == [2] and full.keep_for(0.0).tolist() == [2]
    gone = ScenarioSet(torch.tensor([[-1, -1]]), torch.zeros(1, 2, dtype=torch.int32), torch.full((1, 3), -1, dtype=torch.int32),
                       torch.full((1, 2), float("nan"), dtype=torch.float64), 3, torch.full((1, 2, 1, 1), float("nan")),
                       distances=D)
    assert bool(torch.isnan(gone.weights).all()) and bool(torch.isnan(gone.expect(torch.ones(1, 3))).all())
    assert gone.head(1).assign.tolist() == [[-1, -1, -1]] and gone.head(1).counts.tolist() == [[0]]
    assert math_utils.ScenarioSet.cat([full, gone]).count == 2


def line(points):
    """the distance matrix of points on a line, [1, S, S] float64"""
    x = np.asarray(points, np.float32).reshape(1, -1, 1)
    return R.distances(x).astype(np.float64)


def test_the_restatement_on_hand_worked_values():
    # three collinear points at 0, 1, 3: the column sums are 4, 3, 5 -> index 1 at cost 3 / 3; then z = (1 + 0 + 2, ., 1 + 0 + 0):
    # index 2 at cost 1 / 3; 0 and 1 go to the first pick, 2 to itself
    D = line([0.0, 1.0, 3.0])
    assert D[0].tolist() == [[0, 1, 3], [1, 0, 2], [3, 2, 0]]
    sel, cnt, asg, cost = R.forward(D, 1)
    assert sel.tolist() == [[1]] and cost.tolist() == [[1.0]] and cnt.tolist() == [[3]] and asg.tolist() == [[0, 0, 0]]
    sel, cnt, asg, cost = R.forward(D, 2)
    assert sel.tolist() == [[1, 2]] and cnt.tolist() == [[2, 1]] and asg.tolist() == [[0, 0, 1]]
    assert cost.tolist() == [[1.0, 1.0 / 3.0]] and R.subset_cost(D[0], [1, 2]) == 1.0 / 3.0
    assert sel.dtype == np.int32 and cnt.dtype == np.int32 and asg.dtype == np.int32 and cost.dtype == np.float64
    # two identical paths: exactly 0 apart, the lowest index wins, the duplicate is assigned to it
    x = np.array([[1.5, -2.0, 0.25], [1.5, -2.0, 0.25]], np.float32)[None]
    D = R.distances(x)
    assert D.dtype == np.longdouble and (D == 0).all()
    sel, cnt, asg, cost = R.forward(D.astype(np.float64), 2)
    assert sel.tolist() == [[0, 1]] and asg.tolist() == [[0, 0]] and cnt.tolist() == [[2, 0]] and cost.tolist() == [[0.0, 0.0]]
    D = line([5.0, 0.0, 5.0, 1.0])                                               # a duplicate of the medoid's neighbour
    sel, cnt, asg, cost = R.forward(D, 2)
    assert sel.tolist() == [[0, 1]] and asg.tolist() == [[0, 1, 0, 1]] and cnt.tolist() == [[2, 2]]
    # K = S on distinct paths: everything kept, nothing moved
    D = line([0.0, 1.0, 3.0, 7.0, 15.0])
    sel, cnt, asg, cost = R.forward(D, 5)
    assert sorted(sel[0].tolist()) == [0, 1, 2, 3, 4] and cnt.tolist() == [[1] * 5] and cost[0, -1] == 0.0
    assert (np.diff(cost[0]) <= 0).all() and [sel[0, j] for j in asg[0]] == [0, 1, 2, 3, 4]
    # the scale multiplies the difference; squared leaves the root out
    x = np.array([[0.0, 0.0], [3.0, 2.0]], np.float32)[None]
    assert R.distances(x, scale=[1.0, 2.0])[0, 0, 1] == 5.0 and R.distances(x, scale=[1.0, 2.0], squared=True)[0, 1, 0] == 25.0
    # a NaN, an infinity or a negative entry: that origin alone is refused
    D = np.concatenate([line([0.0, 1.0, 3.0])] * 4)
    D[1, 0, 2], D[2, 1, 1], D[3, 2, 0] = np.nan, np.inf, -1.0
    sel, cnt, asg, cost = R.forward(D, 2)
    assert sel.tolist() == [[1, 2]] + [[-1, -1]] * 3 and cnt.tolist() == [[2, 1]] + [[0, 0]] * 3
    assert asg.tolist() == [[0, 0, 1]] + [[-1] * 3] * 3 and cost[0].tolist() == [1.0, 1.0 / 3.0] and np.isnan(cost[1:]).all()
    # an asymmetric D reads D[k, u] as "k onto u": column 0 is cheap to reach, row 0 is dear to leave
    D = np.array([[[0.0, 9.0, 9.0], [1.0, 0.0, 5.0], [1.0, 5.0, 0.0]]])
    sel, cnt, asg, cost = R.forward(D, 2)
    assert sel.tolist() == [[0, 1]] and cost.tolist() == [[2.0 / 3.0, 1.0 / 3.0]] and asg.tolist() == [[0, 1, 0]]
    assert R.forward(np.transpose(D, (0, 2, 1)).copy(), 1)[0].tolist() == [[1]]     # the transpose: 14 / 3 at 1 or 2, 18 / 3 at 0


def test_the_restatement_against_brute_force():
    """S = 10, L = 6, 200 seeds: the first pick is the medoid (the exact optimum at K = 1); for K <= 3 the greedy cost is at least
    the optimum's (relative 1e-12: the brute-force sums run in another order).  Greedy carries no guarantee to assert: the worst
    ratio is printed."""
    worst = 1.0
    for seed in range(200):
        rng = np.random.default_rng(SEED + seed)
        D = R.distances(rng.normal(size=(1, 10, 6)).astype(np.float32)).astype(np.float64)
        sel, cnt, asg, cost = R.forward(D, 3)
        sums = np.zeros(10)
        for k in range(10):
            sums = sums + D[0, k]
        assert sel[0, 0] == int(np.argmin(sums)) and cost[0, 0] == sums.min() / 10
        assert cnt.sum() == 10 and (np.diff(cost[0]) <= 0).all()
        for K in (1, 2, 3):
            best = R.best_subset_cost(D[0], K)
            assert cost[0, K - 1] >= best * (1 - 1e-12), (seed, K)
            assert abs(cost[0, K - 1] - R.subset_cost(D[0], sel[0, :K])) <= 1e-13 * cost[0, K - 1]
            worst = max(worst, cost[0, K - 1] / best)
        assert abs(cost[0, 0] - R.best_subset_cost(D[0], 1)) <= 1e-12 * cost[0, 0]
    print(f"greedy / optimum, worst over 200 seeds and K <= 3: {worst:.4f}")


def test_the_statistical_cases_by_the_restatement_alone():
    """The conditions of test_hip_reduce's cluster case and value case at its seeds, by numpy alone (figures printed)."""
    x, labels = R.cluster_case(SEED + 1)
    D = R.distances(x.reshape(1, R.CLUSTER_S, -1)).astype(np.float64)
    sel, cnt, asg, cost = R.forward(D, 3)
    print(f"cluster case: counts {cnt[0].tolist()}, cost {cost[0].tolist()}")
    assert R.cluster_conditions(labels, cnt[0], asg[0], cost[0])
    paths = R.walk_case(SEED + 2)
    D = R.distances(paths.reshape(R.WALK_COUNT, R.WALK_S, -1)).astype(np.float64)
    sel, cnt, asg, cost = R.forward(D, R.WALK_K)
    fig = R.value_figures(R.peak_of_mean(paths), D, sel, cnt, cost)
    print(f"value case: error ratio {fig[0]:.4f}, share {fig[1]:.4f}, cost ratio {fig[2]:.4f}")
    assert R.value_conditions(fig)
