"""CPU: the scenario-tree entries of include/stemgnn_hip.h (csrc/tree.hip) are exported, declared and bound; every bad argument is
refused before any launch; the Python layers refuse what they cannot run before anything reaches a GPU; the numpy restatement
(tests/helpers/tree_ref.py) agrees with hand-worked cases, with the weighted forward selection at one stage bit for bit and
with brute force over all admissible trees, and alone meets the conditions of the planted case of tests/test_hip_tree.py at
that test's seed.  Nothing is launched."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import tree_ref as TR
from tests.helpers import weighted_ref as W

SG_EINVAL = -10001
SEED = 20261021
P = 64                          # stand-in device addresses: every call below is refused before any use
NEW = ("stemgnn_scenario_stage_distances", "stemgnn_scenario_tree")


def ints(*v):
    return (ctypes.c_int * len(v))(*v)                                           # host memory: the entries read it


DST = dict(paths=P, scale=2 * P, count=5, S=33, H=7, M=23, T=3, bounds=ints(1, 4, 7), squared=0, D=3 * P)
TRE = dict(D=P, mult_in=2 * P, count=5, S=33, T=3, nodes=ints(2, 4, 8), W=100, node_path=3 * P, node_parent=4 * P,
           node_count=5 * P, assign=6 * P, cost=7 * P)


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
    for name, n in zip(NEW, (11, 13)):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n, name
        assert name + "(" in header, name
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "tree.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    sig = inspect.signature
    assert str(sig(ops.scenario_stage_distances)) == "(paths, stages, scale=None, squared=False)"
    assert str(sig(ops.scenario_tree)) == \
        "(paths, stages, nodes, scale=None, squared=False, distances=None, mult=None, total=None, max_scratch_bytes=268435456)"
    assert str(sig(math_utils.scenario_tree)) == "(paths, stages, nodes, on=None, scale=None, squared=False)"
    assert str(sig(math_utils.ScenarioSet.tree)) == "(self, stages, nodes, on=None, scale=None, squared=False)"
    assert str(sig(trainer.scenario_trees)) == \
        "(model, loader, horizon, stages, nodes, paths=64, seed=0, adjacency=None, coupling='independent', tails='linear', " \
        "origin=0, on=None, scale=None, squared=False)"
    assert str(sig(engine.LiveForecaster.scenario_tree)) == \
        "(self, stages, nodes, paths=64, horizon=None, seed=None, coupling='independent', tails='linear', on=None, scale=None, " \
        "squared=False)"
    for name in ("scenarios", "values", "probabilities", "conditional", "expect", "cat", "export"):
        assert callable(getattr(math_utils.ScenarioTree, name)), name
    for name in ("ScenarioTree", "scenario_tree"):
        assert getattr(stemgnn_amd, name) is getattr(math_utils, name) and name in stemgnn_amd.__all__
    # the pinned signatures still hold
    assert str(sig(ops.scenario_distances)) == "(paths, scale=None, squared=False)"
    assert str(sig(ops.scenario_reduce)) == \
        "(paths, keep, scale=None, squared=False, distances=None, max_scratch_bytes=268435456)"
    assert str(sig(math_utils.reduce_scenarios)) == "(paths, keep, on=None, scale=None, squared=False)"
    assert str(sig(math_utils.ScenarioSet.reduce)) == "(self, keep, on=None, scale=None, squared=False)"
    assert str(sig(math_utils.ScenarioSet.__init__)) == \
        "(self, index, counts, assign, cost, S, paths, distances=None, source=None, total=None)"
    assert str(sig(trainer.reduced_scenarios)) == \
        "(model, loader, horizon, keep, paths=64, seed=0, adjacency=None, coupling='independent', tails='linear', origin=0, " \
        "on=None, scale=None, squared=False)"
    assert str(sig(engine.LiveForecaster.scenario_set)) == \
        "(self, keep, paths=64, horizon=None, seed=None, coupling='independent', tails='linear', on=None, scale=None, " \
        "squared=False)"
    assert tuple(sig(engine.LiveForecaster.scenarios).parameters)[1:] == \
        ("paths", "horizon", "seed", "coupling", "tails", "return_paths")
    assert len(_lib.SIGNATURES["stemgnn_scenario_distances"][1]) == 8 and len(_lib.SIGNATURES["stemgnn_scenario_reduce"][1]) == 9
    assert len(_lib.SIGNATURES["stemgnn_scenario_reduce_weighted"][1]) == 11


def test_stage_distances_reject_bad_arguments(lib):
    f = lib.stemgnn_scenario_stage_distances
    for k in ("paths", "bounds", "D"):
        assert refused(f, DST, **{k: None}), k
    for k in ("count", "S", "H", "M", "T"):
        for v in (0, -1):
            assert refused(f, DST, **{k: v}), (k, v)
    assert refused(f, DST, S=1025)
    assert refused(f, DST, T=17, H=17, bounds=ints(*range(1, 18)))
    for bad in ((0, 4, 7), (1, 1, 7), (4, 1, 7), (1, 4, 6), (1, 4, 8), (-1, 4, 7)):   # not strictly increasing, not ending at H
        assert refused(f, DST, bounds=ints(*bad)), bad
    assert refused(f, DST, squared=2) and refused(f, DST, squared=-1)
    assert refused(f, DST, S=1024, H=2 ** 11, M=2 ** 10, bounds=ints(1, 4, 2 ** 11))             # S * H * M
    assert refused(f, DST, count=2 ** 10, S=1024, H=7, M=1)                      # count * T * S * S
    assert refused(f, DST, count=2 ** 31, S=1) and refused(f, DST, count=2 ** 40, S=1)           # count, and the grid


def test_tree_rejects_bad_arguments(lib):
    f = lib.stemgnn_scenario_tree
    for k in ("D", "nodes", "node_path", "node_parent", "node_count", "assign", "cost"):
        assert refused(f, TRE, **{k: None}), k
    for k in ("count", "S", "T"):
        for v in (0, -1):
            assert refused(f, TRE, **{k: v}), (k, v)
    assert refused(f, TRE, S=1025) and refused(f, TRE, T=17, nodes=ints(*[1] * 17))
    for bad in ((0, 4, 8), (2, 1, 8), (2, 4, 3), (2, 4, 34), (-1, 4, 8)):        # decreasing, or outside [1, S]
        assert refused(f, TRE, nodes=ints(*bad)), bad
    for v in (0, -1, 2 ** 24 + 1):
        assert refused(f, TRE, W=v), v
    assert refused(f, TRE, mult_in=None, W=100) and refused(f, TRE, mult_in=None, W=32)          # NULL: W must be S
    assert refused(f, TRE, count=2 ** 10, S=1024)                                # count * T * S * S
    assert refused(f, TRE, count=2 ** 31, S=1, nodes=ints(1, 1, 1))


def test_ops_refuse_before_touching_the_library(monkeypatch):
    from stemgnn_amd import _lib, ops
    from stemgnn_amd._lib import StemGNNHipError

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    x = torch.zeros(2, 5, 3, 4)
    calls = (lambda p, st=(1, 3), **kw: ops.scenario_stage_distances(p, st, **kw),
             lambda p, st=(1, 3), **kw: ops.scenario_tree(p, st, (1, 2), **kw))
    for call in calls:
        for bad_p in (x[0], torch.zeros(2, 5, 3, 0), np.zeros((2, 5, 3, 4), np.float32), None):
            with pytest.raises(StemGNNHipError, match=r"non-empty \[count,S,H,M\]"):
                call(bad_p)
        for bad_p in (x.double(), x.transpose(1, 2)):
            with pytest.raises(StemGNNHipError, match="contiguous float32"):
                call(bad_p)
        for bad_st in ((), (0, 3), (1, 1, 3), (2, 1, 3), (1, 2), (1, 4), (1.0, 3), (True, 3), 3, None, tuple(range(1, 18))):
            with pytest.raises(StemGNNHipError, match="stages must be 1 to 16 strictly increasing step bounds that end at H = 3"):
                call(x, bad_st)
        with pytest.raises(StemGNNHipError, match=r"scale must be a scalar, \[4\] or \[3,4\]"):
            call(x, scale=torch.ones(3))
        with pytest.raises(StemGNNHipError, match="squared must be True or False"):
            call(x, squared=2)
        for good in (dict(), dict(scale=2.0), dict(squared=True), dict(st=(3,)), dict(st=[1, 2, 3])):
            if call is calls[1] and "st" in good:
                continue                                                         # (its two node counts go with two stages)
            with pytest.raises(StemGNNHipError, match="no CPU fallback"):         # a host tensor: no fallback
                call(x, **good)
    for bad_n in ((), (1,), (0, 2), (2, 1), (1, 6), (1, 2, 3), (1.0, 2), (True, 2), 2, None):
        with pytest.raises(StemGNNHipError, match=r"nodes must be 2 non-decreasing node counts within \[1, 5\]"):
            ops.scenario_tree(x, (1, 3), bad_n)
    for bad_b in (0, 2 * 5 * 5 * 8 - 1, 1.5, True):
        with pytest.raises(StemGNNHipError, match="max_scratch_bytes must hold one origin's"):
            ops.scenario_tree(x, (1, 3), (1, 2), max_scratch_bytes=bad_b)
    m = torch.ones(2, 5, dtype=torch.int32)
    for bad_m in (m.long(), m[:1], m.t().contiguous().t(), m.numpy()):
        with pytest.raises(StemGNNHipError, match="mult must be a contiguous int32"):
            ops.scenario_tree(x, (1, 3), (1, 2), mult=bad_m, total=5)
    for bad_total in (None, 0, 2 ** 24 + 1, 5.0, True):
        with pytest.raises(StemGNNHipError, match="total must be an integer within"):
            ops.scenario_tree(x, (1, 3), (1, 2), mult=m, total=bad_total)
    with pytest.raises(StemGNNHipError, match="without mult every path counts once"):
        ops.scenario_tree(x, (1, 3), (1, 2), total=7)
    d = torch.zeros(2, 2, 5, 5, dtype=torch.float64)
    for bad_d in (d[0], torch.zeros(2, 2, 5, 4, dtype=torch.float64), torch.zeros(0, 2, 5, 5, dtype=torch.float64), d.numpy()):
        with pytest.raises(StemGNNHipError, match=r"distances must be a non-empty \[count,T,S,S\]"):
            ops.scenario_tree(None, None, (1, 2), distances=bad_d)
    for bad_d in (d.float(), d.transpose(2, 3)):
        with pytest.raises(StemGNNHipError, match="contiguous float64"):
            ops.scenario_tree(None, None, (1, 2), distances=bad_d)
    with pytest.raises(StemGNNHipError, match="at most 1024 paths and 16 stages"):
        ops.scenario_tree(None, None, (1,) * 17, distances=torch.zeros(1, 17, 1, 1, dtype=torch.float64))
    with pytest.raises(StemGNNHipError, match="with the distances' count = 2 and S = 5"):
        ops.scenario_tree(torch.zeros(2, 6, 3, 4), None, (1, 2), distances=d)
    with pytest.raises(StemGNNHipError, match="3 stages, but the distances hold T = 2"):
        ops.scenario_tree(None, (1, 2, 3), (1, 2), distances=d)
    for p in (None, x):
        with pytest.raises(StemGNNHipError, match="distances is on cpu.*no CPU fallback"):
            ops.scenario_tree(p, None, (1, 2), distances=d)


def a_tree(count=2, S=5, N=4, total=5):
    """a hand-made tree on the host: stages (1, 3), nodes (1, 2); node 0 of stage 1 holds paths {0, 1, 2}, node 1 holds {3, 4}"""
    from stemgnn_amd.math_utils import ScenarioTree
    index = torch.tensor([[[0, -1], [1, 3]]] * count)
    parent = torch.tensor([[[0, -1], [0, 0]]] * count, dtype=torch.int32)
    counts = torch.tensor([[[total, 0], [total - 2, 2]]] * count, dtype=torch.int32)
    assign = torch.tensor([[[0] * S, [0, 0, 0, 1, 1] + [1] * (S - 5)]] * count, dtype=torch.int32)
    cost = torch.tensor([[2.0, 1.0]] * count, dtype=torch.float64)
    values = [torch.zeros(count, 1, 1, N), torch.ones(count, 2, 2, N)]
    return ScenarioTree((1, 3), (1, 2), index, parent, counts, assign, cost, S, total, values, torch.ones(count, 2, 3, N))


def test_python_layers_have_no_cpu_fallback_and_check_their_arguments(monkeypatch):
    from stemgnn_amd import _lib, trainer
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import EventSpec, ScenarioSet, ScenarioTree, scenario_tree

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    p = torch.zeros(2, 5, 3, 4)
    spec = EventSpec(0.5, groups=[[0, 1], [2, 3]])
    for call in (lambda: scenario_tree(p, (1, 3), (1, 2)), lambda: scenario_tree(p, (1, 3), (1, 2), on=spec),
                 lambda: scenario_tree(p, (1, 3), (1, 2), on=torch.zeros(2, 5, 3, 2)),
                 lambda: scenario_tree(p, (3,), (5,), scale=0.5, squared=True)):
        with pytest.raises(StemGNNHipError, match="no CPU fallback"):
            call()
    with pytest.raises(StemGNNHipError, match=r"paths must be \[count,S,H,N\]"):
        scenario_tree(p[0], (1, 3), (1, 2))
    for bad_on in (torch.zeros(2, 5, 3), torch.zeros(2, 4, 3, 2), torch.zeros(2, 5, 2, 4)):
        with pytest.raises(StemGNNHipError, match=r"on must be \[count,S,H,R\]"):
            scenario_tree(p, (1, 3), (1, 2), on=bad_on)
    with pytest.raises(ValueError, match="no groups="):
        scenario_tree(p, (1, 3), (1, 2), on=EventSpec(0.5))
    with pytest.raises(StemGNNHipError, match="stages must be 1 to 16 strictly increasing"):
        scenario_tree(p, (1, 2), (1, 2))
    with pytest.raises(StemGNNHipError, match="nodes must be 2 non-decreasing"):
        scenario_tree(p, (1, 3), (2, 1))
    with pytest.raises(ValueError, match="needs a quantile model"):
        trainer.scenario_trees(object(), [], 3, (1, 3), (1, 2))
    kept = ScenarioSet(torch.zeros(2, 3, dtype=torch.int64), torch.ones(2, 3, dtype=torch.int32), torch.zeros(2, 5, dtype=torch.int32),
                       torch.zeros(2, 3, dtype=torch.float64), 5, torch.zeros(2, 3, 3, 4))
    with pytest.raises(StemGNNHipError, match=r"nodes must be 2 non-decreasing node counts within \[1, 3\]"):
        kept.tree((1, 3), (1, 4))
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        kept.tree((1, 3), (1, 2))
    # what needs no kernel runs on the host as it stands
    tree = a_tree()
    assert (tree.count, tree.T, tree.H, tree.N, tree.S, tree.total) == (2, 2, 3, 4, 5, 5)
    assert tree.probabilities(0).tolist() == [[1.0]] * 2 and tree.probabilities(1).tolist() == [[0.6, 0.4]] * 2
    assert tree.conditional(0).tolist() == [[1.0]] * 2 and tree.conditional(1).tolist() == [[0.6, 0.4]] * 2
    assert tuple(tree.values(1).shape) == (2, 2, 2, 4)
    leaves = tree.scenarios()
    assert isinstance(leaves, ScenarioSet) and (leaves.K, leaves.S, leaves.total) == (2, 5, 5)
    assert leaves.index.tolist() == [[1, 3]] * 2 and leaves.counts.tolist() == [[3, 2]] * 2
    assert tree.expect(torch.tensor([[1.0, 10.0, 2.0, 20.0, 3.0]] * 2)).tolist() == [0.6 * 10.0 + 0.4 * 20.0] * 2
    out = tree.export(1)
    assert out["stages"] == (1, 3) and out["nodes"] == (1, 2) and out["total"] == 5
    assert out["parent"][1].tolist() == [0, 0] and out["probability"][1].tolist() == [0.6, 0.4]
    assert out["conditional"][0].tolist() == [1.0] and out["values"][1].shape == (2, 2, 4)
    both = ScenarioTree.cat([tree, a_tree(count=1)])
    assert both.count == 3 and tuple(both.values(0).shape) == (3, 1, 1, 4) and tuple(both.paths.shape) == (3, 2, 3, 4)
    for other in (a_tree(S=6), a_tree(N=3), a_tree(total=7)):
        with pytest.raises(ValueError, match="share stages, nodes, S, total and N"):
            ScenarioTree.cat([tree, other])
    with pytest.raises(ValueError, match="share stages"):
        ScenarioTree.cat([])
    for bad_t in (-1, 2, 0.5, True):
        with pytest.raises(ValueError, match=r"t must be a stage within \[0, 1\]"):
            tree.values(bad_t)
    with pytest.raises(ValueError, match=r"c must be an origin within \[0, 1\]"):
        tree.export(2)
    with pytest.raises(ValueError, match="node_index must be int64"):
        ScenarioTree((1, 3), (1, 2), tree.node_index.int(), tree.parent, tree.counts, tree.assign, tree.cost, 5, 5,
                     [tree.values(0), tree.values(1)], tree.paths)


def line(points, T=1):
    """the stage distances of points on a line, the same at every stage: [1, T, S, S] float64"""
    x = np.asarray(points, np.float64)
    return np.broadcast_to(np.abs(x[:, None] - x[None, :]), (1, T, len(x), len(x))).copy()


def test_the_restatement_on_hand_worked_values():
    # S = 1: the path is every stage's only node
    path, parent, count, assign, cost = TR.tree(line([2.0], 3), None, 1, (1, 1, 1))
    assert path.tolist() == [[[0]] * 3] and parent.tolist() == [[[0]] * 3] and count.tolist() == [[[1]] * 3]
    assert assign.tolist() == [[[0]] * 3] and cost.tolist() == [[0.0] * 3]
    assert path.dtype == np.int32 and assign.dtype == np.int32 and cost.dtype == np.float64
    # S = 2, T = 2, nodes (1, 2): stage 1 keeps index 0 (equal sums, the lower index) at cost (0 + 3) / 2; stage 2: phase A picks
    # the parent's child 0 again (z = 4 each), phase B adds 1; both nodes are children of node 0
    D = np.array([[[[0.0, 3.0], [3.0, 0.0]], [[0.0, 4.0], [4.0, 0.0]]]])
    path, parent, count, assign, cost = TR.tree(D, None, 2, (1, 2))
    assert path.tolist() == [[[0, -1], [0, 1]]] and parent.tolist() == [[[0, -1], [0, 0]]]
    assert count.tolist() == [[[2, 0], [1, 1]]] and assign.tolist() == [[[0, 0], [0, 1]]] and cost.tolist() == [[1.5, 0.0]]
    # the same with multiplicities (1, 3): index 1 is the medoid (z = 3 * 3 at 0, 1 * 3 at 1)
    path, parent, count, assign, cost = TR.tree(D, [[1, 3]], 4, (1, 2))
    assert path.tolist() == [[[1, -1], [1, 0]]] and count.tolist() == [[[4, 0], [3, 1]]] and cost.tolist() == [[0.75, 0.0]]
    # nodes (2, 2): stage 2 is phase A alone, one child per parent, and a path never moves to the other parent's child although
    # it is nearer: points 0, 1 | 10, 11 at stage 1; at stage 2 path 1 sits on path 2
    D1 = line([0.0, 1.0, 10.0, 11.0])[0, 0]
    D2 = D1.copy()
    D2[1, 2] = D2[2, 1] = 0.0
    path, parent, count, assign, cost = TR.tree(np.stack([D1, D2])[None], None, 4, (2, 2))
    assert path.tolist() == [[[1, 2], [0, 2]]] and parent.tolist() == [[[0, 0], [0, 1]]]     # (sums 22, 20, 20, 22: index 1)
    assert assign.tolist() == [[[0, 0, 1, 1], [0, 0, 1, 1]]] and count.tolist() == [[[2, 2], [2, 2]]]
    assert cost.tolist() == [[0.5, 0.5]]
    # a member of multiplicity 0 is never read; a refused origin is refused at every stage and alone
    D = np.concatenate([line([0.0, 1.0, 3.0], 2)] * 5)
    D[0, :, 2, :] = D[0, :, :, 2] = np.nan
    D[2, 1, 0, 1] = -1.0
    D[3, 0, 2, 2] = np.inf
    mult = [[2, 1, 0], [1, 1, 1], [1, 1, 1], [1, 1, 1], [3, 0, 0]]
    path, parent, count, assign, cost = TR.tree(D, mult, 3, (1, 2))
    assert path[0].tolist() == [[0, -1], [0, 1]] and assign[0].tolist() == [[0, 0, -1], [0, 1, -1]] and count[0].tolist() == [[3, 0], [2, 1]]
    assert path[1].tolist() == [[1, -1], [1, 2]] and cost[1].tolist() == [1.0, 1.0 / 3.0]
    for c in (2, 3, 4):                                                          # a negative entry, an infinity, n_T above the live
        assert (path[c] == -1).all() and (parent[c] == -1).all() and (count[c] == 0).all() and (assign[c] == -1).all()
        assert np.isnan(cost[c]).all()
    # a duplicated path that is picked: its node is empty, and so is that node's child
    D = line([0.0, 0.0, 5.0], 2)
    path, parent, count, assign, cost = TR.tree(D, None, 3, (3, 3))
    assert path.tolist() == [[[0, 2, 1], [0, 2, -1]]] and parent.tolist() == [[[0, 0, 0], [0, 1, 2]]]
    assert count.tolist() == [[[2, 1, 0], [2, 1, 0]]] and assign.tolist() == [[[0, 0, 1], [0, 0, 1]]]
    # the composed leaves: leaf j's steps of stage t are its ancestor's representative's
    x = np.arange(4 * 3 * 1, dtype=np.float32).reshape(1, 4, 3, 1)
    got = TR.leaves(x, (1, 3), np.array([[[0, -1], [1, 3]]]), np.array([[[0, 0, 0, 0], [0, 0, 1, 1]]]))
    assert got[0, :, :, 0].tolist() == [[0.0, 4.0, 5.0], [0.0, 10.0, 11.0]]
    # the distances: the scale multiplies the difference, squared leaves the root out, the prefix grows with the stage
    x = np.array([[[0.0, 0.0], [0.0, 0.0]], [[3.0, 2.0], [4.0, 0.0]]], np.float32)[None]      # [1, 2, H = 2, M = 2]
    got = TR.stage_distances(x, (1, 2), scale=[1.0, 2.0])
    assert got.dtype == np.longdouble and got[0, :, 0, 1].tolist() == [5.0, np.sqrt(np.longdouble(41.0))]
    assert TR.stage_distances(x, (1, 2), squared=True, dtype=np.float64)[0, :, 1, 0].tolist() == [13.0, 29.0]


@pytest.mark.parametrize("S,K", [(5, 2), (33, 8), (12, 12)])
def test_one_stage_is_the_weighted_forward_selection_bit_for_bit(S, K):
    rng = np.random.default_rng(SEED + S)
    x = rng.normal(size=(3, S, 4, 3)).astype(np.float32)
    x[:, S - 1] = x[:, 0]
    D = TR.stage_distances(x, (4,), dtype=np.float64)
    for mult, Wt in ((TR.random_mult(rng, 3, S, 2 * S, zeros=K < S), 2 * S), (np.ones((3, S), np.int32), S)):
        path, parent, count, assign, cost = TR.tree(D, mult, Wt, (K,))
        sel, cnt, asg, cst = W.forward(D[:, 0], mult, Wt, K)
        assert np.array_equal(path[:, 0], sel) and np.array_equal(count[:, 0], cnt) and np.array_equal(assign[:, 0], asg)
        ok = ~np.isnan(cst[:, K - 1])
        assert np.array_equal(cost[ok, 0].view(np.int64), cst[ok, K - 1].view(np.int64))
        assert np.array_equal(np.isnan(cost[:, 0]), ~ok) and (parent[ok, 0] == 0).all()
    assert np.array_equal(TR.tree(D, None, S, (K,))[4].view(np.int64), cost.view(np.int64))       # NULL is all ones


def test_the_restatement_against_brute_force():
    """S <= 6, T = 2, 60 seeds: at each stage the greedy cost is at least the optimum over all admissible node sets given the
    stage before (relative 1e-12: the brute-force sums run in another order), and equal where n_t = n_{t-1} (phase A alone: every
    parent's best child).  Greedy carries no further guarantee to assert: the worst ratio is printed."""
    worst = 1.0
    for seed in range(60):
        rng = np.random.default_rng(SEED + seed)
        S = int(rng.integers(3, 7))
        x = rng.normal(size=(1, S, 4, 2)).astype(np.float32)
        D = TR.stage_distances(x, (2, 4), dtype=np.float64)
        mult = TR.random_mult(rng, 1, S, S + 3, zeros=seed % 2 == 1)
        live = int((mult[0] > 0).sum())
        n1 = int(rng.integers(1, live + 1))
        n2 = int(rng.integers(n1, live + 1))
        path, parent, count, assign, cost = TR.tree(D, mult, S + 3, (n1, n2))
        assert count[0].sum(axis=1).tolist() == [S + 3] * 2
        best1 = TR.best_subset_cost(D[0, 0], mult[0], S + 3, np.zeros(S, np.int64), n1)
        best2 = TR.best_subset_cost(D[0, 1], mult[0], S + 3, assign[0, 0], n2)
        for got, best, same in ((cost[0, 0], best1, n1 == 1), (cost[0, 1], best2, n2 == n1)):
            assert got >= best * (1 - 1e-12), (seed, got, best)
            if same:
                assert abs(got - best) <= 1e-12 * max(best, 1e-300), (seed, got, best)
            if best > 0:
                worst = max(worst, got / best)
        reps = [u for u in path[0, 1] if u >= 0]
        own = TR.subset_cost(D[0, 1], mult[0], S + 3, assign[0, 0], reps)
        assert abs(own - cost[0, 1]) <= 1e-12 * max(own, 1e-300)
    print(f"greedy / optimum per stage, worst over 60 seeds: {worst:.4f}")


def test_the_planted_case_by_the_restatement_alone():
    """The conditions of test_hip_tree's planted case at its seed, by numpy alone (figures printed)."""
    x, labels = TR.planted_case(SEED)
    D = TR.stage_distances(x[None], TR.PLANT_BOUNDS, dtype=np.float64)
    path, parent, count, assign, cost = TR.tree(D, None, TR.PLANT_S, TR.PLANT_NODES)
    print(f"planted case: counts {count[0].tolist()}, cost {cost[0].tolist()}")
    assert TR.planted_conditions(labels, assign[0], count[0])
    assert count[0, 0, :2].tolist() == [32, 32] and count[0, 1, :4].tolist() == [16] * 4
    assert sorted(count[0, 2].tolist()) == sorted(TR.PLANT_SIZES)
