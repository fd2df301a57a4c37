"""CPU: the weighted scenario-set entries of include/stemgnn_hip.h (csrc/weighted.hip) are exported, declared and bound; every bad
argument is refused before any launch; the Python layers refuse what they cannot run before anything reaches a GPU; the numpy
restatement (tests/helpers/weighted_ref.py) agrees with hand-worked cases and with the project's unweighted helpers on the
replicated ensemble; from_weights, merge and the reading of negative counts run on the host; the walk-case figures of
tests/test_hip_weighted.py are computed by the restatement alone at that test's seed.  Nothing is launched."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import ensemble_ref, events_ref, reduce_ref, scenario_ref
from tests.helpers import weighted_ref as W

SG_EINVAL = -10001
SEED = 20261023
P = 64                          # stand-in device addresses: every call below is refused before any use
RANKS = (ctypes.c_int * 3)(1, 4, 7)             # host memory: the entry reads it
NEW = ("stemgnn_weighted_bands", "stemgnn_weighted_scratch_doubles", "stemgnn_weighted_out_doubles", "stemgnn_weighted_scores",
       "stemgnn_weighted_events", "stemgnn_scenario_reduce_weighted")
BND = dict(paths=P, mult=2 * P, count=5, K=8, H=3, N=70, W=7, Q=3, ranks=RANKS, bands=3 * P)
SCO = dict(target=P, paths=2 * P, mult=3 * P, mul=None, add=None, count=5, K=8, H=3, N=70, W=64, fair=0, masked=0,
           scratch=4 * P, out=5 * P, hist=6 * P)
EVT = dict(paths=P, mult=2 * P, thr=3 * P, mul=None, add=None, count=5, K=8, H=3, M=70, W=64, above=1, min_run=1, counts=4 * P)
RED = dict(D=P, mult_in=2 * P, count=5, S=33, K=8, W=100, selected=3 * P, counts=4 * P, assign=5 * P, cost=6 * P)


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
    from stemgnn_amd import _lib, engine, math_utils, ops, trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    for name, n in zip(NEW, (11, 4, 1, 16, 14, 11)):
        assert len(_lib.SIGNATURES[name][1]) == n, name
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "weighted.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    assert lib.stemgnn_weighted_out_doubles(12) == 7 * 13 and lib.stemgnn_weighted_out_doubles(0) == 0
    assert lib.stemgnn_weighted_scratch_doubles(5, 8, 3, 70) > 0
    for bad in ((0, 8, 3, 70), (5, 0, 3, 70), (5, 257, 3, 70), (5, 8, 0, 70), (5, 8, 3, 0), (2 ** 31, 8, 3, 70)):
        assert lib.stemgnn_weighted_scratch_doubles(*bad) == 0, bad
    sig = inspect.signature
    for name in ("weighted_bands", "weighted_scores", "weighted_events", "scenario_reduce_weighted"):
        assert callable(getattr(ops, name)), name
    for name in ("bands", "scores", "events", "reduce", "merge", "from_weights"):
        assert callable(getattr(math_utils.ScenarioSet, name)), name
    assert sig(math_utils.ScenarioSet.__init__).parameters["total"].default is None
    assert str(sig(math_utils.ScenarioSet.bands)) == "(self, quantiles, out=None)"
    assert str(sig(math_utils.ScenarioSet.scores)) == "(self, y, mul=None, add=None, ignore_nan=False, fair=False)"
    assert str(sig(math_utils.ScenarioSet.reduce)) == "(self, keep, on=None, scale=None, squared=False)"
    assert str(sig(math_utils.ScenarioSet.from_weights)) == "(paths, weights, total=65536)"
    # the pinned signatures still hold
    assert str(sig(math_utils.reduce_scenarios)) == "(paths, keep, on=None, scale=None, squared=False)"
    assert str(sig(ops.scenario_reduce)) == \
        "(paths, keep, scale=None, squared=False, distances=None, max_scratch_bytes=268435456)"
    assert str(sig(ops.scenario_events)) == "(paths, threshold, above=True, min_run=1, mul=None, add=None)"
    assert str(sig(ops.ensemble_scores)) == "(y, paths, mul=None, add=None, ignore_nan=False, fair=False)"
    assert str(sig(math_utils.EnsembleScores.__init__)) == "(self, y, paths, mul=None, add=None, ignore_nan=False, fair=False)"
    assert str(sig(math_utils.EventSpec.__init__)) == \
        "(self, threshold, above=True, min_run=1, groups=None, reduce='mean', mul=None, add=None)"
    assert str(sig(trainer.reduced_scenarios)) == \
        "(model, loader, horizon, keep, paths=64, seed=0, adjacency=None, coupling='independent', tails='linear', origin=0, " \
        "on=None, scale=None, squared=False)"
    assert str(sig(engine.LiveForecaster.scenario_set)) == \
        "(self, keep, paths=64, horizon=None, seed=None, coupling='independent', tails='linear', on=None, scale=None, " \
        "squared=False)"
    par = sig(trainer.rolling_scenarios).parameters
    assert tuple(par) == ("model", "loader", "horizon", "paths", "seed", "adjacency", "coupling", "tails", "return_paths", "origin",
                          "events")
    assert tuple(sig(trainer.score_forecast).parameters)[-1] == "events"


def test_bands_reject_bad_arguments(lib):
    f = lib.stemgnn_weighted_bands
    for k in ("paths", "mult", "ranks", "bands"):
        assert refused(f, BND, **{k: None}), k
    assert refused(f, BND, bands=P)                                              # in place
    for k in ("count", "K", "H", "N", "W", "Q"):
        for v in (0, -1):
            assert refused(f, BND, **{k: v}), (k, v)
    assert refused(f, BND, K=257) and refused(f, BND, Q=33) and refused(f, BND, W=2 ** 24 + 1)
    for bad in ((0, 4, 7), (1, 8, 7), (1, 4, -1)):
        assert refused(f, BND, ranks=(ctypes.c_int * 3)(*bad)), bad
    assert refused(f, BND, W=3)                                                  # ranks 4 and 7 are beyond W
    assert refused(f, BND, H=2 ** 16, N=2 ** 15)                                 # H * N
    assert refused(f, BND, K=256, H=2 ** 12, N=2 ** 11)                          # K * H * N
    assert refused(f, BND, K=1, Q=32, H=2 ** 13, N=2 ** 13)                      # Q * H * N
    assert refused(f, BND, count=2 ** 31) and refused(f, BND, count=2 ** 28, H=1, N=512)   # count, and the grid


def test_scores_reject_bad_arguments(lib):
    f = lib.stemgnn_weighted_scores
    for k in ("target", "paths", "mult", "scratch", "out", "hist"):
        assert refused(f, SCO, **{k: None}), k
    assert refused(f, SCO, mul=P) and refused(f, SCO, add=P)
    for k in ("count", "K", "H", "N", "W"):
        for v in (0, -1):
            assert refused(f, SCO, **{k: v}), (k, v)
    assert refused(f, SCO, K=257) and refused(f, SCO, W=2 ** 24 + 1)
    assert refused(f, SCO, W=1, fair=1)
    assert refused(f, SCO, H=128, W=2 ** 24)                                     # H * (W + 1)
    assert refused(f, SCO, H=2 ** 16, N=2 ** 15) and refused(f, SCO, K=256, H=2 ** 12, N=2 ** 11)
    assert refused(f, SCO, count=2 ** 31) and refused(f, SCO, count=2 ** 30, H=2, N=1)     # count, count * H
    assert refused(f, SCO, count=2 ** 26, K=256, H=1, N=1)                       # the pair grid: 36 tiles a row


def test_events_reject_bad_arguments(lib):
    f = lib.stemgnn_weighted_events
    for k in ("paths", "mult", "thr", "counts"):
        assert refused(f, EVT, **{k: None}), k
    assert refused(f, EVT, mul=P) and refused(f, EVT, add=P)
    for k in ("count", "K", "H", "M", "W"):
        for v in (0, -1):
            assert refused(f, EVT, **{k: v}), (k, v)
    assert refused(f, EVT, K=257) and refused(f, EVT, H=257, min_run=1) and refused(f, EVT, W=2 ** 24 + 1)
    for v in (0, 4, -1):
        assert refused(f, EVT, min_run=v), v
    assert refused(f, EVT, above=2) and refused(f, EVT, above=-1)
    assert refused(f, EVT, K=256, H=256, M=2 ** 15)                              # K * H * M
    assert refused(f, EVT, K=1, H=256, M=2 ** 22)                                # (2 H + 1) * M
    assert refused(f, EVT, count=2 ** 31) and refused(f, EVT, count=2 ** 30, K=1, H=1, M=128)   # count, and the grid


def test_reduce_weighted_rejects_bad_arguments(lib):
    f = lib.stemgnn_scenario_reduce_weighted
    for k in ("D", "mult_in", "selected", "counts", "assign", "cost"):
        assert refused(f, RED, **{k: None}), k
    for k in ("count", "S", "W"):
        for v in (0, -1):
            assert refused(f, RED, **{k: v}), (k, v)
    assert refused(f, RED, S=1025, K=1) and refused(f, RED, W=2 ** 24 + 1)
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
    m = torch.ones(2, 5, dtype=torch.int32)
    y = torch.zeros(2, 3, 4)
    calls = (lambda p, mu=m, t=5, **kw: ops.weighted_bands(p, mu, t, (0.1, 0.9), **kw),
             lambda p, mu=m, t=5, **kw: ops.weighted_scores(y, p, mu, t, **kw),
             lambda p, mu=m, t=5, **kw: ops.weighted_events(p, mu, t, 0.5, **kw))
    for call in calls:
        for bad_p in (x[0], torch.zeros(2, 5, 3, 0), np.zeros((2, 5, 3, 4), np.float32), None):
            with pytest.raises(StemGNNHipError, match=r"non-empty \[count,K,H,N\]"):
                call(bad_p)
        for bad_p in (x.double(), x.transpose(2, 3)):
            with pytest.raises(StemGNNHipError, match="contiguous float32"):
                call(bad_p)
        with pytest.raises(StemGNNHipError, match="at most 256 weighted members"):
            call(torch.zeros(1, 257, 1, 1), mu=torch.ones(1, 257, dtype=torch.int32))
        for bad_m in (m.long(), m[:, :4], m[0], m.t(), [[1] * 5] * 2, None):
            with pytest.raises(StemGNNHipError, match="mult must be a contiguous int32"):
                call(x, mu=bad_m)
        for bad_t in (0, -1, 2 ** 24 + 1, 5.0, True, None):
            with pytest.raises(StemGNNHipError, match=r"total must be an integer within \[1, 2\^24\]"):
                call(x, t=bad_t)
        with pytest.raises(StemGNNHipError, match="no CPU fallback"):            # a host tensor: no fallback
            call(x)
    with pytest.raises(StemGNNHipError, match="1 to 32 levels"):
        ops.weighted_bands(x, m, 5, ())
    with pytest.raises(StemGNNHipError, match="out must be a contiguous float32"):
        ops.weighted_bands(x, m, 5, (0.1, 0.9), out=torch.zeros(2, 3, 3, 4))
    for bad_y in (y[0], y.double(), torch.zeros(2, 3, 5), None):
        with pytest.raises(StemGNNHipError, match=r"y must be a contiguous float32 \[count,H,N\]"):
            ops.weighted_scores(bad_y, x, m, 5)
    with pytest.raises(StemGNNHipError, match="mul and add go together"):
        ops.weighted_scores(y, x, m, 5, mul=torch.ones(4))
    with pytest.raises(StemGNNHipError, match="fair=True needs total >= 2"):
        ops.weighted_scores(y, x, m, 1, fair=True)
    with pytest.raises(StemGNNHipError, match="histogram"):
        ops.weighted_scores(torch.zeros(1, 200, 1), torch.zeros(1, 2, 200, 1), torch.ones(1, 2, dtype=torch.int32), 2 ** 24)
    for bad_r in (0, 4, 1.5, True):
        with pytest.raises(StemGNNHipError, match=r"min_run must be an integer within \[1, 3\]"):
            ops.weighted_events(x, m, 5, 0.5, min_run=bad_r)
    with pytest.raises(StemGNNHipError, match="threshold must be a scalar or 4 values"):
        ops.weighted_events(x, m, 5, torch.zeros(3))
    d = torch.zeros(2, 5, 5, dtype=torch.float64)
    for bad_d in (d[0], torch.zeros(2, 5, 4, dtype=torch.float64), d.numpy()):
        with pytest.raises(StemGNNHipError, match=r"distances must be a non-empty \[count,S,S\]"):
            ops.scenario_reduce_weighted(bad_d, m, 5, 2)
    for bad_d in (d.float(), d.transpose(1, 2)):
        with pytest.raises(StemGNNHipError, match="contiguous float64"):
            ops.scenario_reduce_weighted(bad_d, m, 5, 2)
    with pytest.raises(StemGNNHipError, match="at most 1024 members"):
        ops.scenario_reduce_weighted(torch.zeros(1, 1025, 1025, dtype=torch.float64), torch.ones(1, 1025, dtype=torch.int32), 5, 2)
    with pytest.raises(StemGNNHipError, match="mult must be a contiguous int32"):
        ops.scenario_reduce_weighted(d, m[:, :4], 5, 2)
    for bad_k in (0, 6, 1.5, True):
        with pytest.raises(StemGNNHipError, match=r"keep must be an integer within \[1, 5\]"):
            ops.scenario_reduce_weighted(d, m, 5, bad_k)
    with pytest.raises(StemGNNHipError, match="distances is on cpu.*no CPU fallback"):
        ops.scenario_reduce_weighted(d, m, 5, 2)


def a_set(S=5, K=2, H=3, N=4, counts=None, **kw):
    from stemgnn_amd.math_utils import ScenarioSet
    counts = torch.ones(2, K, dtype=torch.int32) if counts is None else counts
    return ScenarioSet(torch.zeros(2, K, dtype=torch.int64), counts, torch.zeros(2, S, dtype=torch.int32),
                       torch.zeros(2, K, dtype=torch.float64), S, torch.zeros(2, K, H, N), **kw)


def test_python_layers_have_no_cpu_fallback_and_check_their_arguments(monkeypatch):
    from stemgnn_amd import _lib
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import EventSpec, ScenarioSet

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    s = a_set(total=2)
    assert s.total == 2 and a_set().total == 5 and s.weights.tolist() == [[0.5, 0.5]] * 2
    y = torch.zeros(2, 3, 4)
    spec, grouped = EventSpec(0.5), EventSpec(0.5, groups=[[0, 1], [2, 3]])
    for call in (lambda: s.bands((0.1, 0.9)), lambda: s.scores(y), lambda: s.scores(y, fair=True, ignore_nan=True),
                 lambda: s.events(spec), lambda: spec.count(s), lambda: grouped.count(s), lambda: s.reduce(1),
                 lambda: s.reduce(1, on=grouped), lambda: s.reduce(1, on=torch.zeros(2, 2, 3, 2), scale=0.5, squared=True)):
        with pytest.raises(StemGNNHipError, match="no CPU fallback"):
            call()
    for bad_t in (0, 2 ** 24 + 1, 1.5, True):
        with pytest.raises(ValueError, match=r"total must be an integer within \[1, 2\^24\]"):
            a_set(total=bad_t)
    with pytest.raises(ValueError, match="spec must be an EventSpec"):
        s.events(0.5)
    for bad_k in (0, 3, 1.5, True):
        with pytest.raises(StemGNNHipError, match=r"keep must be an integer within \[1, 2\]"):
            s.reduce(bad_k)
    with pytest.raises(ValueError, match="no groups="):
        s.reduce(1, on=spec)
    for bad_on in (torch.zeros(2, 2, 3), torch.zeros(2, 3, 3, 2), torch.zeros(3, 2, 3, 2)):
        with pytest.raises(StemGNNHipError, match=r"on must be \[count,K,H,R\]"):
            s.reduce(1, on=bad_on)
    child = a_set(S=2, K=1, total=2)
    child._parent = s                                                            # what reduce() leaves behind
    with pytest.raises(ValueError, match=r"parent\.reduce\(k\)"):
        child.head(1)
    with pytest.raises(ValueError, match="share total"):
        ScenarioSet.cat([a_set(), a_set(total=7)])
    assert ScenarioSet.cat([s, s]).total == 2


def test_merge_and_from_weights_on_the_host():
    from stemgnn_amd.math_utils import ScenarioSet
    a = ScenarioSet(torch.tensor([[3, 1], [-1, -1]]), torch.tensor([[3, 1], [0, 0]], dtype=torch.int32),
                    torch.tensor([[1, 1, 0, 0], [-1, -1, -1, -1]], dtype=torch.int32), torch.zeros(2, 2, dtype=torch.float64), 4,
                    torch.arange(2 * 2 * 1 * 2, dtype=torch.float32).reshape(2, 2, 1, 2))
    b = ScenarioSet(torch.tensor([[0], [2]]), torch.tensor([[6], [6]], dtype=torch.int32),
                    torch.zeros(2, 6, dtype=torch.int32), torch.zeros(2, 1, dtype=torch.float64), 6,
                    100 + torch.arange(2 * 1 * 1 * 2, dtype=torch.float32).reshape(2, 1, 1, 2))
    mrg = ScenarioSet.merge([a, b])
    assert (mrg.count, mrg.K, mrg.S, mrg.total, mrg.H, mrg.N) == (2, 3, 10, 10, 1, 2)
    assert mrg.index.tolist() == [[3, 1, 4], [-1, -1, 6]] and mrg.counts.tolist() == [[3, 1, 6], [0, 0, 6]]
    assert mrg.assign.tolist() == [[1, 1, 0, 0, 2, 2, 2, 2, 2, 2], [-1, -1, -1, -1, 2, 2, 2, 2, 2, 2]]
    assert bool(torch.isnan(mrg.cost).all()) and mrg.distances is None and mrg.source is None
    assert mrg.paths[0, :, 0, 0].tolist() == [0.0, 2.0, 100.0]
    assert mrg.weights[0].tolist() == [0.3, 0.1, 0.6] and bool(torch.isnan(mrg.weights[1]).all())   # a refused part: absent
    assert not W.present(mrg.counts.numpy(), mrg.total)[1] and W.present(mrg.counts.numpy(), mrg.total)[0]
    for bad in ([], [a, a_set()], [a, 3]):
        with pytest.raises(ValueError, match="ScenarioSets of the same origins"):
            ScenarioSet.merge(bad)
    with pytest.raises(ValueError, match="beyond 2\\^24"):
        ScenarioSet.merge([a_set(total=2 ** 24), a_set(total=1)])
    with pytest.raises(ValueError, match="needs `distances`"):
        mrg.head(1)
    # largest remainders by hand: 0.5 / 0.25 / 0.25 of 4 is exact; thirds of 4 leave one unit for the lowest index; 0.45 / 0.45 /
    # 0.1 of 10 is 4.5, 4.5, 1: one unit short, equal remainders 0.5, index 0 takes it; 1 / 2 / 3 of 7: 1.17, 2.33, 3.5 -> 1, 2, 4
    p = torch.zeros(8, 3, 1, 1)
    rows = [[0.5, 0.25, 0.25], [1.0, 1.0, 1.0], [0.0, 2.0, 0.0], [1.0, -1.0, 1.0], [0.0, 0.0, 0.0], [1.0, float("nan"), 1.0],
            [1.0, float("inf"), 1.0], [3.0, 0.0, 1.0]]
    fw = ScenarioSet.from_weights(p, torch.tensor(rows), total=4)
    assert fw.counts.tolist() == [[2, 1, 1], [2, 1, 1], [0, 4, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0], [3, 0, 1]]
    assert (fw.total, fw.S, fw.K) == (4, 3, 3) and fw.index.tolist() == [[0, 1, 2]] * 8 and fw.counts.dtype == torch.int32
    assert W.present(fw.counts.numpy(), 4).tolist() == [True, True, True, False, False, False, False, True]
    assert ScenarioSet.from_weights(p[:2], [[0.45, 0.45, 0.1], [1, 2, 3]], total=10).counts.tolist() == [[5, 4, 1], [2, 3, 5]]
    assert ScenarioSet.from_weights(p[:1], [[1, 2, 3]], total=7).counts.tolist() == [[1, 2, 4]]
    rng = np.random.default_rng(SEED)
    w = rng.random((50, 9))
    for total in (1, 64, 65536, 2 ** 24):
        got = ScenarioSet.from_weights(torch.zeros(50, 9, 1, 1), torch.tensor(w), total=total).counts.tolist()
        assert got == [W.round_weights(r, total) for r in w] and all(sum(r) == total for r in got)
    assert ScenarioSet.from_weights(p[:1], [[1, 1, 1]]).total == 65536
    for bad_t in (0, 2 ** 24 + 1, 2.5, True):
        with pytest.raises(ValueError, match="total must be an integer"):
            ScenarioSet.from_weights(p, torch.tensor(rows), total=bad_t)
    with pytest.raises(ValueError, match=r"weights must be real and \[count, K\]"):
        ScenarioSet.from_weights(p, torch.ones(8, 2))
    with pytest.raises(ValueError, match=r"paths must be \[count,K,H,N\]"):
        ScenarioSet.from_weights(p[0], torch.ones(3))


def test_negative_counts_read_as_nan_and_are_left_out_of_the_score():
    from stemgnn_amd.math_utils import ScenarioEvents
    H, M, S = 2, 1, 4
    counts = torch.tensor([[[4], [1], [4], [0], [3]], [[-1]] * 5, [[0], [2], [0], [2], [1]]], dtype=torch.int32)
    ev = ScenarioEvents(counts, S)
    assert ev.p_any[:, 0].tolist()[::2] == [1.0, 0.5] and bool(torch.isnan(ev.p_any[1]).all())
    for name in ("p_step", "p_by", "p_run", "duration"):
        v = getattr(ev, name)
        assert bool(torch.isnan(v[1]).all()) and not bool(torch.isnan(v[0]).any()) and not bool(torch.isnan(v[2]).any()), name
    real = ScenarioEvents(torch.tensor([[[1], [0], [1], [0], [1]]] * 3, dtype=torch.int32), 1,
                          torch.zeros(3, H, M, dtype=torch.bool))
    sc = ev.score(real)
    assert sc.valid == 2 and sc.reliability[0, :, 0].tolist() == [0, 0, 1, 0, 1]
    whole = ScenarioEvents(counts[::2].contiguous(), S).score(ScenarioEvents(real.counts[::2].contiguous(), 1, real.missing[::2]))
    assert (whole.reliability == sc.reliability).all() and (whole.reliability_step == sc.reliability_step).all()
    assert whole.brier == sc.brier and whole.brier_run == sc.brier_run


def test_the_restatement_on_hand_worked_values():
    # two members, 0 with weight 3 and 4 with weight 1, the truth at 1:
    #   crps = (3 * 1 + 1 * 3) / 4 - (2 * 3 * 1 * 4) / (2 * 16) = 1.5 - 0.75; fair: 1.5 - 24 / 24
    #   mean = 1, var = (3 * 1 + 1 * 9) / 3 = 4, rank = 3
    paths = np.array([0.0, 4.0], np.float32).reshape(1, 2, 1, 1)
    mult = np.array([[3, 1]])
    y = np.ones((1, 1, 1), np.float32)
    r = W.scores(y, paths, mult, 4)
    assert r["out"][:7].tolist() == [0.75, 0.75, 0.0, 2.0, 1.0, 1.0, 0.0] and r["out"][7:].tolist() == r["out"][:7].tolist()
    assert r["hist"].tolist() == [[0, 0, 0, 1, 0]]
    assert r["first"][:, 0].tolist() == [1.5, 1.5] and r["second"][:, 0].tolist() == [0.75, 0.75]
    assert W.scores(y, paths, mult, 4, fair=True)["out"][:2].tolist() == [0.5, 0.5]
    assert W.scores(y, paths, mult, 4, mul=[2.0], add=[1.0])["out"][:4].tolist() == [1.5, 1.5, 0.0, 4.0]
    assert W.bands(paths, mult, 4, [1, 2, 3, 4])[0, :, 0, 0].tolist() == [0.0, 0.0, 0.0, 4.0]
    assert [W.rank(t, 4) for t in (0.0, 0.25, 0.5, 0.75, 0.76, 1.0)] == [1, 1, 2, 3, 4, 4]
    assert W.events(paths, mult, 4, [2.0], True, 1)[0, :, 0].tolist() == [1, 1, 1]
    assert W.events(paths, mult, 4, [2.0], False, 1)[0, :, 0].tolist() == [3, 3, 3]
    # a tie at the target: 3 // 2 = 1; with the weights the other way round 1 // 2 = 0
    tie = np.array([1.0, 4.0], np.float32).reshape(1, 2, 1, 1)
    assert W.scores(y, tie, mult, 4)["hist"].tolist() == [[0, 1, 0, 0, 0]]
    assert W.scores(y, tie, np.array([[1, 3]]), 4)["hist"].tolist() == [[1, 0, 0, 0, 0]]
    # a member of multiplicity 0 that holds NaN reaches nothing
    p3 = np.array([0.0, np.nan, 4.0], np.float32).reshape(1, 3, 1, 1)
    m3 = np.array([[3, 0, 1]])
    r3 = W.scores(y, p3, m3, 4)
    assert r3["out"].tolist() == r["out"].tolist() and r3["hist"].tolist() == r["hist"].tolist()
    assert W.bands(p3, m3, 4, [3, 4])[0, :, 0, 0].tolist() == [0.0, 4.0]
    assert W.events(p3, m3, 4, [2.0], True, 1)[0, :, 0].tolist() == [1, 1, 1]
    # with a positive multiplicity it propagates: NaN last in the order, NaN scores, no event
    m3n = np.array([[2, 1, 1]])
    assert np.isnan(W.scores(y, p3, m3n, 4)["out"][:4]).all()
    b = W.bands(p3, m3n, 4, [2, 3, 4])[0, :, 0, 0]
    assert b[:2].tolist() == [0.0, 4.0] and np.isnan(b[2])
    assert W.events(p3, m3n, 4, [2.0], True, 1)[0, :, 0].tolist() == [1, 1, 1]
    # an absent origin (a wrong sum, a negative multiplicity) beside a present one
    p2 = np.concatenate([paths, paths, paths])
    m2 = np.array([[3, 2], [3, 1], [5, -1]])
    y2 = np.ones((3, 1, 1), np.float32)
    r2 = W.scores(y2, p2, m2, 4)
    assert r2["out"][:7].tolist() == [0.75, 0.75, 0.0, 2.0, 1.0, 1.0, 2.0] and r2["hist"].tolist() == r["hist"].tolist()
    bb = W.bands(p2, m2, 4, [1, 4])
    assert (bb[[0, 2]].view(np.uint32) == 0x7FC00000).all() and bb[1, :, 0, 0].tolist() == [0.0, 4.0]
    ee = W.events(p2, m2, 4, [2.0], True, 1)
    assert (ee[[0, 2]] == -1).all() and ee[1, :, 0].tolist() == [1, 1, 1]
    only = W.scores(y2[:1], p2[:1], m2[:1], 4)["out"]
    assert np.isnan(only[:4]).all() and only[4:7].tolist() == [0.0, 0.0, 1.0]
    # W = 1: the variance is 0 / 0
    assert np.isnan(W.scores(y, paths[:, :1], np.array([[1]]), 1)["out"][3])
    # a run: the member in the event at steps 0 and 1 only
    walk = np.array([[3.0, 3.0, 0.0], [0.0, 3.0, 3.0]], np.float32).reshape(1, 2, 3, 1)
    e = W.events(walk, np.array([[5, 2]]), 7, [2.0], True, 2)[0, :, 0].tolist()
    assert e == [5, 7, 2, 5, 2, 0, 7]
    # forward selection: points at 0, 1, 3 with multiplicities 1, 1, 2 of 4: z = (7, 5, 5) -> index 1 at 5 / 4; then
    # z_0 = 0 + 0 + 2 * 2, z_2 = 1 + 0 + 0 -> index 2 at 1 / 4; 0 and 1 go to the first pick
    x = np.array([0.0, 1.0, 3.0], np.float32).reshape(1, 3, 1)
    D = reduce_ref.distances(x).astype(np.float64)
    sel, cnt, asg, cost = W.forward(D, np.array([[1, 1, 2]]), 4, 2)
    assert sel.tolist() == [[1, 2]] and cnt.tolist() == [[2, 2]] and asg.tolist() == [[0, 0, 1]] and cost.tolist() == [[1.25, 0.25]]
    # a member of multiplicity 0 is no candidate, is assigned nowhere, and its NaN distances are not read
    D0 = D.copy()
    D0[0, 1, :], D0[0, :, 1] = np.nan, np.nan
    sel, cnt, asg, cost = W.forward(D0, np.array([[2, 0, 2]]), 4, 2)
    assert sel.tolist() == [[0, 2]] and cnt.tolist() == [[2, 2]] and asg.tolist() == [[0, -1, 1]] and cost.tolist() == [[1.5, 0.0]]
    # refused: too few positive members, a wrong sum, a negative multiplicity, a NaN between two positive members
    for m, d in (([2, 0, 2], D0), ([1, 1, 1], D), ([3, -1, 2], D), ([1, 1, 2], D0)):
        sel, cnt, asg, cost = W.forward(d, np.array([m]), 4, 3 if m == [2, 0, 2] else 2)
        assert (sel == -1).all() and (cnt == 0).all() and (asg == -1).all() and np.isnan(cost).all(), m


CASES = ((1, 1, 1, 1, 1), (3, 2, 2, 5, 7), (4, 8, 3, 7, 64), (2, 33, 1, 6, 100), (2, 5, 4, 3, 12))


@pytest.mark.parametrize("shape", CASES)
def test_the_restatement_against_the_existing_helpers_on_the_replicated_ensemble(shape):
    count, K, H, N, Wt = shape
    rng = np.random.default_rng(SEED + sum(shape))
    paths, target, mult = W.random_set(rng, count, K, H, N, Wt)
    paths[0, :, 0, 0] = np.where(np.isnan(paths[0, :, 0, 0]), np.nan, target[0, 0, 0])     # ties at the target, and among members
    if N > 1:
        paths[-1, :, -1, 1] = np.float32(-0.0) * np.sign(paths[-1, :, -1, 1])              # +0 and -0 are one value
    rep = W.replicate(paths, mult)
    taus = (0.05, 0.5, 0.95, 1.0)
    want = np.empty((count, len(taus), H, N), np.float32)
    scenario_ref.bands_of(rep, taus, 0, want)
    got = W.bands(paths, mult, Wt, [W.rank(t, Wt) for t in taus])
    assert [W.rank(t, Wt) for t in taus] == [scenario_ref.rank(t, Wt) for t in taus]
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    mul, add = rng.uniform(0.5, 2.0, N), rng.normal(size=N)
    thr = rng.normal(size=N) * 0.5
    for above, run, dn in ((True, 1, False), (False, min(2, H), True)):
        kw = dict(mul=mul, add=add) if dn else {}
        assert (W.events(paths, mult, Wt, thr, above, run, **kw) == events_ref.events_fast(rep, thr, above, run, **kw)).all()
    target[0, 0, -1] = np.nan
    for masked, fair, dn in ((False, False, False), (True, Wt > 1, True)):
        kw = dict(mul=mul, add=add) if dn else {}
        a = W.scores(target, paths, mult, Wt, masked=masked, fair=fair, **kw)
        b = ensemble_ref.scores(target, rep, masked=masked, fair=fair, **kw)
        assert (a["hist"] == b["hist"]).all()
        for h in range(1 + H):
            at7 = (lambda k: k) if h == 0 else (lambda k: 7 + k * H + h - 1)
            at6 = (lambda k: k) if h == 0 else (lambda k: 6 + k * H + h - 1)
            for k in (4, 5):
                assert a["out"][at7(k)] == b["out"][at6(k)]
            assert a["out"][at7(6)] == 0.0
            for k in (0, 1):
                x, z = a["out"][at7(k)], b["out"][at6(k)]
                bound = 2e-9 * (abs(b["first"][k, h]) + abs(b["second"][k, h]))
                assert (np.isnan(x) and np.isnan(z)) or abs(x - z) <= bound, (h, k, x, z)
            for k in (2, 3):
                x, z = a["out"][at7(k)], b["out"][at6(k)]
                assert (np.isnan(x) and np.isnan(z)) or abs(x - z) <= 2e-9 * abs(z), (h, k, x, z)


def test_forward_with_all_ones_weights_is_the_parent_restatement():
    rng = np.random.default_rng(SEED + 5)
    for S, K in ((5, 2), (33, 8), (64, 8)):
        D = reduce_ref.distances(rng.normal(size=(4, S, 7)).astype(np.float32)).astype(np.float64)
        D[1, 2, 3] = np.nan
        D[2, S - 1, 0] = -1.0
        a = W.forward(D, np.ones((4, S), np.int32), S, K)
        b = reduce_ref.forward(D, K)
        for x, z in zip(a, b):
            assert x.dtype == z.dtype and x.tobytes() == z.tobytes()
        assert (a[0][1:3] == -1).all() and (a[1][[0, 3]].sum(axis=1) == S).all()
    # weighted: the counts add up to W, the cost does not rise, the kept members are positive ones
    D = reduce_ref.distances(rng.normal(size=(6, 20, 7)).astype(np.float32)).astype(np.float64)
    mult = W.random_set(rng, 6, 20, 1, 1, 50)[2]
    sel, cnt, asg, cost = W.forward(D, mult, 50, 6)
    assert (cnt.sum(axis=1) == 50).all() and (np.diff(cost, axis=1) <= 0).all()
    assert (np.take_along_axis(mult, sel.astype(np.int64), axis=1) > 0).all() and ((asg == -1) == (mult == 0)).all()


WALK_N, WALK_KEEP, EVENT_LEVEL = 128, 8, 2.0


def node_mean(x):
    """[..., N] float32 -> [..., 1] float32: the mean over the nodes as the aggregate entry returns it (fp64 sum, rounded once)"""
    w = np.full((1, x.shape[-1]), 1.0 / x.shape[-1])
    return events_ref.aggregate(x.reshape(-1, x.shape[-1]), w)[0].astype(np.float32).reshape(x.shape[:-1] + (1,))


def walk_figures(count=WALK_N):
    """the table of DESIGN.md 5t by the restatement alone: the full 64, the weighted 8 and the first 8 of the walk case against one
    more draw from the same law; the event is "the mean of the 16 nodes above 2.0 at some step" -> {name: dict}"""
    paths = reduce_ref.walk_case(SEED, count)
    truth = reduce_ref.walk_case(SEED + 1, count)[:, 0]
    S = paths.shape[1]
    D = reduce_ref.distances(paths.reshape(count, S, -1)).astype(np.float64)
    ones = np.ones((count, S), np.int32)
    sel, cnt, asg, cost = W.forward(D, ones, S, WALK_KEEP)
    kept = np.take_along_axis(paths, sel.astype(np.int64)[:, :, None, None], axis=1)
    sets = {"full 64": (paths, ones, S), "weighted 8": (kept, cnt, S),
            "first 8": (paths[:, :WALK_KEEP], ones[:, :WALK_KEEP], WALK_KEEP)}
    H = paths.shape[2]
    real = W.events(node_mean(truth)[:, None], np.ones((count, 1), np.int32), 1, [EVENT_LEVEL], True, 1)
    o = real[:, H:2 * H, 0].sum(axis=1).astype(np.float64)
    out = {}
    for name, (x, m, total) in sets.items():
        r = W.scores(truth, x, m, total)["out"]
        ev = W.events(node_mean(x), m, total, [EVENT_LEVEL], True, 1)
        p = ev[:, H:2 * H, 0].sum(axis=1) / float(total)
        out[name] = dict(energy=r[1], crps=r[0], spread=r[3], rmse=r[2], brier=float(((p - o) ** 2).mean()), p=float(p.mean()),
                         base=float(o.mean()), sets=(x, m, total), any=ev[:, H:2 * H, 0].sum(axis=1))
    return out, truth


def test_the_walk_case_figures_by_the_restatement_alone():
    """The figures of the issue's table, printed; asserted is only what must hold: the weighted 8 score as their replication to
    64 scores (the existing helper), their multiplicities sum to 64, and the "any" count is the sum of the multiplicities of the
    members in the event.  The direction of reduced / first 8 / full is printed, not asserted."""
    fig, truth = walk_figures()
    for name, f in fig.items():
        print(f"{name:11s} energy {f['energy']:.3f} crps {f['crps']:.3f} spread {f['spread']:.3f} rmse {f['rmse']:.3f} "
              f"brier {f['brier']:.4f} mean p {f['p']:.3f} base rate {f['base']:.4f}")
    x, m, total = fig["weighted 8"]["sets"]
    assert (m.sum(axis=1) == 64).all() and total == 64
    a = W.scores(truth, x, m, total)
    b = ensemble_ref.scores(truth, W.replicate(x, m))
    assert (a["hist"] == b["hist"]).all()
    for k in (0, 1):
        assert abs(a["out"][k] - b["out"][k]) <= 2e-9 * (abs(b["first"][k, 0]) + abs(b["second"][k, 0]))
    for k in (2, 3):
        assert abs(a["out"][k] - b["out"][k]) <= 2e-9 * abs(b["out"][k])
    inside = (node_mean(x)[..., 0] > EVENT_LEVEL).any(axis=2)                    # [count, 8]: the member is in the event
    assert (fig["weighted 8"]["any"] == (m * inside).sum(axis=1)).all()
