"""GPU: scenario trees -- the two kernels of csrc/tree.hip against the numpy restatement of their definition
(tests/helpers/tree_ref.py), and math_utils.scenario_tree / ScenarioTree through ScenarioSet.tree, trainer.scenario_trees and
LiveForecaster.scenario_tree.

Every output of the entries lies inside a guarded buffer (NaN for the fp64 ones, -7 for the int32 ones), compared whole.  The stage
distances carry the issue's bound, derived and not measured: |got - ref| <= (L_t + T + 8) 2^-53 ref against the longdouble
restatement, L_t the prefix length -- one rounding per difference, per scaling and per fused multiply-add (any grouping of the
L_t terms into partial sums adds at most as many roundings to a term as the sequential sum does), at most T + 3 joins of partial
and stage sums, halved by the root, plus the root's own -- and twice that without the root.  The tree is compared bit for bit:
the restatement adds in the definition's order."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import tree_ref as TR
from tests.helpers import weighted_ref as W
from tests.test_hip_scenario import DEV, device_copy, same_bits, tsame
from tests.test_hip_weighted import check_scores, dev_mult, guarded_as, inside, is_guard

pytestmark = pytest.mark.gpu
SEED = 20261021
NAN = np.nan
STAGES = [(7, 23, (1, 4, 7)),            # stages longer than a 64-chunk that end mid-chunk
          (5, 3, (1, 2, 3, 4, 5)),       # one step per stage
          (4, 64, (2, 4))]               # boundaries on chunk edges


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def ints(n, *v):
    return (ctypes.c_int * n)(*v)


def run_stage_distances(lib, d_x, d_scale, bounds, squared):
    count, S, H, M = d_x.shape
    T = len(bounds)
    whole, d_D = guarded_as((count, T, S, S), torch.float64, NAN)
    rc = lib.stemgnn_scenario_stage_distances(d_x.data_ptr(), None if d_scale is None else d_scale.data_ptr(), count, S, H, M, T,
                                              ints(T, *bounds), squared, d_D.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return inside(whole, (count, T, S, S), np.isnan)


def run_tree(lib, d_D, d_mult, Wt, nodes):
    count, T, S, _ = d_D.shape
    nT = nodes[-1]
    outs = [guarded_as((count, T, nT), torch.int32, -7), guarded_as((count, T, nT), torch.int32, -7),
            guarded_as((count, T, nT), torch.int32, -7), guarded_as((count, T, S), torch.int32, -7),
            guarded_as((count, T), torch.float64, NAN)]
    rc = lib.stemgnn_scenario_tree(d_D.data_ptr(), None if d_mult is None else d_mult.data_ptr(), count, S, T, ints(T, *nodes),
                                   Wt, *(view.data_ptr() for _, view in outs), None)
    assert rc == 0
    torch.cuda.synchronize()
    return tuple(inside(outs[i][0], (count, T, nT), is_guard) for i in range(3)) + \
        (inside(outs[3][0], (count, T, S), is_guard), inside(outs[4][0], (count, T), np.isnan))


def same_tree(got, want):
    ok = ~np.isnan(want[4])
    return all(np.array_equal(g, w) for g, w in zip(got[:4], want[:4])) and got[4].shape == want[4].shape and \
        np.array_equal(np.isnan(got[4]), ~ok) and np.array_equal(bits64(got[4])[ok], bits64(want[4])[ok])


def check_distances(lib, x, bounds, worst):
    count, S, H, M = x.shape
    T = len(bounds)
    rng = np.random.default_rng(SEED + S + H)
    scale = rng.uniform(0.25, 4.0, size=(H, M))
    d_scale = torch.from_numpy(scale.reshape(-1)).to(DEV)
    lt = np.asarray(bounds, np.longdouble)[None, :, None, None] * M              # the prefix length of every stage
    for sc in (None, scale):
        for squared in (0, 1):
            ref = TR.stage_distances(x, bounds, sc, bool(squared))
            bound = (2 if squared else 1) * (lt + T + 8) * np.longdouble(2.0) ** -53 * ref
            _, d_x = device_copy(x, misalign=bool(squared))                      # the base pointer one float off 16 bytes
            got = run_stage_distances(lib, d_x, None if sc is None else d_scale, bounds, squared)
            err = np.abs(got.astype(np.longdouble) - ref)
            assert (err <= bound).all(), (sc is not None, squared, float((err - bound).max()))
            if (bound > 0).any():
                worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
            diag = got[:, :, np.arange(S), np.arange(S)]
            assert (diag == 0).all() and not np.signbit(diag).any()               # exactly +0
            assert np.array_equal(bits64(got), bits64(np.transpose(got, (0, 1, 3, 2))))
            if S >= 2:
                assert (got[:, :, 0, S - 1] == 0).all()                           # the duplicated path
            assert (np.diff(got, axis=1) >= 0).all()                              # a prefix only grows
            again = run_stage_distances(lib, d_x, None if sc is None else d_scale, bounds, squared)
            assert np.array_equal(bits64(again), bits64(got))
            assert same_bits(d_x.cpu().numpy(), x)
            if count > 1:                                                        # the origins over two calls: the whole
                a = run_stage_distances(lib, d_x[:1], None if sc is None else d_scale, bounds, squared)
                b = run_stage_distances(lib, d_x[1:], None if sc is None else d_scale, bounds, squared)
                assert np.array_equal(bits64(np.concatenate([a, b])), bits64(got))
    return worst


def paths_case(rng, count, S, H, M):
    x = rng.normal(size=(count, S, H, M)).astype(np.float32)
    if S >= 2:
        x[:, S - 1] = x[:, 0]                                                    # a duplicated path
    if S >= 4:
        x[:, 2] = x[:, 1] + np.float32(2.0 ** -20) * rng.normal(size=(count, H, M)).astype(np.float32)   # nearly coincident
    return x


@pytest.mark.parametrize("S", [1, 2, 31, 33, 64, 65])
def test_stage_distances_match_the_longdouble_restatement(S):
    from stemgnn_amd import _lib
    lib = _lib.load()
    worst = 0.0
    for H, M, bounds in STAGES:
        rng = np.random.default_rng(SEED + 11 * S + 13 * H)
        worst = check_distances(lib, paths_case(rng, 2, S, H, M), bounds, worst)
    print(f"S = {S}: worst error / bound {worst:.4f}")


def test_stage_distances_on_more_workgroups_than_compute_units():
    from stemgnn_amd import _lib
    H, M, bounds = STAGES[0]
    worst = check_distances(_lib.load(), paths_case(np.random.default_rng(SEED + 1), 300, 8, H, M), bounds, 0.0)
    print(f"count = 300: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("count,S,H,M", [pytest.param(2, 33, 5, 13, id="33-5-13"), pytest.param(2, 8, 2, 200, id="8-2-200"),
                                         pytest.param(2, 65, 3, 64, id="65-3-64"), pytest.param(300, 5, 3, 110, id="300-5-3-110")])
def test_one_stage_is_the_distance_entry(count, S, H, M):
    """T = 1 against ops.scenario_distances: the same bits (one tile body behind both entries), and both within the bound of the
    longdouble restatement.  300 origins are more workgroups than compute units: the 256-thread form, six chunks, the four
    partial sums getting 2, 2, 1, 1; the other cases take the wide form"""
    from stemgnn_amd import ops
    x = paths_case(np.random.default_rng(SEED + S), count, S, H, M)
    d_x = torch.from_numpy(x).to(DEV)
    L = H * M
    for squared in (False, True):
        ref = TR.stage_distances(x, (H,), None, squared)[:, 0]
        bound = (2 if squared else 1) * (L + 1 + 8) * np.longdouble(2.0) ** -53 * ref
        got = ops.scenario_stage_distances(d_x, (H,), squared=squared).cpu().numpy()[:, 0]
        other = ops.scenario_distances(d_x, squared=squared).cpu().numpy()
        assert (np.abs(got.astype(np.longdouble) - ref) <= bound).all()
        assert (np.abs(got.astype(np.longdouble) - other.astype(np.longdouble)) <= bound).all()
        assert np.array_equal(bits64(got), bits64(other))


def test_a_nan_reaches_its_row_and_column_from_its_stage_on():
    from stemgnn_amd import ops
    H, M, bounds = STAGES[0]
    x = np.random.default_rng(SEED + 2).normal(size=(2, 33, H, M)).astype(np.float32)
    x[0, 5, 2, 7] = np.nan                                                       # stage 2 (steps 1 .. 3) of origin 0
    x[1, 32, 6, 0] = np.inf                                                      # the last stage of origin 1
    got = ops.scenario_stage_distances(torch.from_numpy(x).to(DEV), bounds).cpu().numpy()
    want = np.zeros(got.shape, bool)
    want[0, 1:, 5, :] = want[0, 1:, :, 5] = True
    assert np.array_equal(np.isnan(got[0]), want[0]) and np.isfinite(got[0, 0]).all()
    assert np.isfinite(got[1, :2]).all() and np.isnan(got[1, 2, 32, 32])         # inf - inf on the diagonal
    off = np.arange(33) != 32
    assert np.isposinf(got[1, 2, 32, off]).all() and np.isposinf(got[1, 2, off, 32]).all()
    assert np.isfinite(got[1, 2][np.ix_(off, off)]).all()


def tree_inputs(S, T, count, seed):
    """device stage distances [count, T, S, S] of random paths with a duplicate and a near-duplicate among them"""
    from stemgnn_amd import ops
    rng = np.random.default_rng(seed)
    x = paths_case(rng, count, S, 2 * T, 3)
    d_D = ops.scenario_stage_distances(torch.from_numpy(x).to(DEV), tuple(range(2, 2 * T + 1, 2)))
    return rng, d_D, d_D.cpu().numpy()


TREE_CASES = [(S, nodes) for S in (1, 2, 33, 64, 142) for nodes in ((1, 1, 1), (2, 4, 8), ("S", "S", "S"), (1, "S"))]


@pytest.mark.parametrize("S,nodes", TREE_CASES, ids=lambda v: str(v).replace(" ", "").replace("'", ""))
def test_tree_matches_the_restatement_bit_for_bit(S, nodes):
    """the LDS path and (S = 142) the read-from-memory path; uniform multiplicities (NULL), random ones, and random ones
    with zeros (a tree with n_T above the live members is refused, by both)"""
    from stemgnn_amd import _lib
    lib = _lib.load()
    nodes = tuple(min(S, S if n == "S" else n) for n in nodes)
    count = 1 if S == 142 else 2
    rng, d_D, D = tree_inputs(S, len(nodes), count, SEED + 17 * S + sum(nodes))
    Wt = 3 * S + 1
    cases = [(None, S), (TR.random_mult(rng, count, S, Wt, zeros=False), Wt), (TR.random_mult(rng, count, S, Wt), Wt)]
    for mult, total in cases:
        got = run_tree(lib, d_D, None if mult is None else dev_mult(mult), total, nodes)
        want = TR.tree(D, mult, total, nodes)
        assert same_tree(got, want), (mult is None, [np.array_equal(g, w) for g, w in zip(got, want)])
        assert same_tree(run_tree(lib, d_D, None if mult is None else dev_mult(mult), total, nodes), got)
        if count > 1:                                                            # the origins over two calls: the whole
            parts = [run_tree(lib, d_D[c:c + 1], None if mult is None else dev_mult(mult[c:c + 1]), total, nodes)
                     for c in range(count)]
            assert same_tree(tuple(np.concatenate([p[i] for p in parts]) for i in range(5)), got)


@pytest.mark.parametrize("S", [33, 142])
def test_refused_origins_leave_the_others_alone(S):
    from stemgnn_amd import _lib
    lib = _lib.load()
    nodes = (2, 4, 8)
    rng, d_D, D = tree_inputs(S, 3, 6, SEED + S)
    Wt = 2 * S
    mult = TR.random_mult(rng, 6, S, Wt, zeros=False)
    mult[1, 3] += 1                                                              # a wrong sum: absent
    mult[2, 4] = -1                                                              # a negative multiplicity: absent
    mult[2, 5] += Wt - mult[2].sum()                                             # (the sum is right again)
    mult[4] = 0                                                                  # seven live members: n_T = 8 exceeds them
    mult[4, :7] = [Wt - 6, 1, 1, 1, 1, 1, 1]
    D[3, 1, 7, 9] = -1.0                                                         # a negative distance in stage 2
    D[5, 2, 0, 1] = np.nan                                                       # a NaN in the last stage: the stored stages are taken back
    mult[0, 6] += mult[0, 2]                                                     # origin 0: a zero whose row and column hold NaN
    mult[0, 2] = 0
    D[0, :, 2, :] = D[0, :, :, 2] = np.nan
    d_D = torch.from_numpy(D).to(DEV)
    got = run_tree(lib, d_D, dev_mult(mult), Wt, nodes)
    want = TR.tree(D, mult, Wt, nodes)
    assert same_tree(got, want)
    assert (got[0][1:] == -1).all() and (got[1][1:] == -1).all() and (got[2][1:] == 0).all() and (got[3][1:] == -1).all()
    assert np.isnan(got[4][1:]).all() and (got[0][0, 2] >= 0).all() and (got[2][0].sum(axis=1) == Wt).all()
    assert (got[3][0, :, 2] == -1).all()
    alone = run_tree(lib, d_D[:1], dev_mult(mult[:1]), Wt, nodes)
    assert same_tree(alone, tuple(g[:1] for g in got))


@pytest.mark.parametrize("S,K", [(5, 2), (33, 8), (64, 8), (142, 5), (12, 12)])
def test_one_stage_is_the_forward_selection(S, K):
    from stemgnn_amd import ops
    rng = np.random.default_rng(SEED + 3 * S + K)
    d_x = torch.from_numpy(paths_case(rng, 3, S, 4, 5)).to(DEV)
    D = ops.scenario_distances(d_x)
    sel, cnt, asg, cost = ops.scenario_reduce(d_x, K)
    for got in (ops.scenario_tree(d_x, (4,), (K,)), ops.scenario_tree(None, (4,), (K,), distances=D[:, None].contiguous())):
        assert tsame(got[0][:, 0], sel) and tsame(got[2][:, 0], cnt) and tsame(got[3][:, 0], asg)
        assert tsame(got[4][:, 0], cost[:, K - 1]) and bool((got[1] == 0).all())
    Wt = 2 * S + 3
    mult = dev_mult(TR.random_mult(rng, 3, S, Wt, zeros=K < S))
    sel, cnt, asg, cost = ops.scenario_reduce_weighted(D, mult, Wt, K)
    got = ops.scenario_tree(d_x, (4,), (K,), mult=mult, total=Wt)
    assert tsame(got[0][:, 0], sel) and tsame(got[2][:, 0], cnt) and tsame(got[3][:, 0], asg)
    assert tsame(got[4][:, 0], cost[:, K - 1])


def test_the_callers_own_asymmetric_distances_and_the_batches():
    from stemgnn_amd import ops
    rng = np.random.default_rng(SEED + 4)
    D = np.cumsum(rng.uniform(0.1, 2.0, size=(7, 3, 20, 20)), axis=1)            # asymmetric, growing with the stage
    d_D = torch.from_numpy(D).to(DEV)
    mult = TR.random_mult(rng, 7, 20, 50)
    want = TR.tree(D, mult, 50, (2, 3, 6))
    got = ops.scenario_tree(None, None, (2, 3, 6), distances=d_D, mult=dev_mult(mult), total=50)
    assert same_tree(tuple(g.cpu().numpy() for g in got), want)
    x = torch.from_numpy(paths_case(rng, 7, 20, 6, 5)).to(DEV)
    scale = torch.linspace(0.5, 2.0, 5)
    whole = ops.scenario_tree(x, (1, 3, 6), (2, 3, 6), scale=scale, squared=True)
    parts = ops.scenario_tree(x, (1, 3, 6), (2, 3, 6), scale=scale, squared=True, max_scratch_bytes=2 * 3 * 20 * 20 * 8)
    assert all(tsame(a, b) for a, b in zip(whole, parts))
    D = ops.scenario_stage_distances(x, (1, 3, 6), scale, True)
    assert same_tree(tuple(g.cpu().numpy() for g in whole), TR.tree(D.cpu().numpy(), None, 20, (2, 3, 6)))


def test_the_structure_of_a_tree():
    from stemgnn_amd import scenario_tree
    rng = np.random.default_rng(SEED + 5)
    S, H, N, bounds, nodes = 24, 7, 5, (2, 4, 7), (2, 5, 9)
    x = rng.normal(size=(4, S, H, N)).astype(np.float32)
    d_x = torch.from_numpy(x).to(DEV)
    tree = scenario_tree(d_x, bounds, nodes)
    parent, counts, assign = tree.parent.cpu().numpy(), tree.counts.cpu().numpy(), tree.assign.cpu().numpy()
    leaves = tree.scenarios().paths.cpu().numpy()
    index = tree.node_index.cpu().numpy()
    assert same_bits(leaves, TR.leaves(x, bounds, index, assign))
    for c in range(4):
        for t in range(3):
            assert counts[c, t].sum() == S == tree.total
            if t:                                                                # the children's counts add up to their parent's
                for i in range(nodes[t - 1]):
                    assert counts[c, t, :nodes[t]][parent[c, t, :nodes[t]] == i].sum() == counts[c, t - 1, i]
                assert (parent[c, t, :nodes[t - 1]] == np.arange(nodes[t - 1])).all()
            anc = assign[c, t, index[c, 2]]                                      # the leaves' ancestors at stage t
            for a in range(9):
                for b in range(a):
                    if anc[a] == anc[b]:                                         # a shared ancestor: the same bits before b_t
                        assert same_bits(leaves[c, a, :bounds[t]], leaves[c, b, :bounds[t]])
            prefixes = {leaves[c, j, :bounds[t]].tobytes() for j in range(9)}
            assert len(prefixes) == nodes[t]
    every = scenario_tree(d_x, bounds, (S, S, S))
    assert bool((every.counts == 1).all()) and bool((every.cost == 0).all())
    assert sorted(every.node_index[0, 2].tolist()) == list(range(S))
    assert tsame(every.scenarios().paths, torch.gather(d_x, 1, every.node_index[:, 2][:, :, None, None].expand(-1, -1, H, N)))


def test_the_planted_tree():
    """S = 64, bounds (2, 4, 6), nodes (2, 4, 8), leaf sizes 12, 4, 9, 7, 10, 6, 11, 5 in shuffled order: every stage's
    assignment reproduces the planted labels up to renaming, and the counts are the planted sizes"""
    from stemgnn_amd import scenario_tree
    x, labels = TR.planted_case(SEED)
    tree = scenario_tree(torch.from_numpy(x[None]).to(DEV), TR.PLANT_BOUNDS, TR.PLANT_NODES)
    counts, assign = tree.counts[0].cpu().numpy(), tree.assign[0].cpu().numpy()
    print(f"planted case: counts {counts.tolist()}, cost {tree.cost[0].tolist()}")
    assert TR.planted_conditions(labels, assign, counts)
    assert counts[0, :2].tolist() == [32, 32] and counts[1, :4].tolist() == [16] * 4
    assert sorted(counts[2].tolist()) == sorted(TR.PLANT_SIZES)


def test_a_tree_answers_what_a_scenario_set_is_asked():
    from stemgnn_amd import EventSpec, ScenarioSet, ScenarioTree, reduce_scenarios, scenario_tree
    rng = np.random.default_rng(SEED + 6)
    S, H, N, bounds, nodes = 32, 6, 8, (2, 4, 6), (2, 4, 6)
    x = np.cumsum(rng.normal(size=(5, S, H, N)), axis=2).astype(np.float32)
    x[3, 7, 5, 1] = np.nan                                                       # origin 3 is refused (its last stage)
    truth = np.cumsum(rng.normal(size=(5, H, N)), axis=1).astype(np.float32)
    d_x, d_y = torch.from_numpy(x).to(DEV), torch.from_numpy(truth).to(DEV)
    tree = scenario_tree(d_x, bounds, nodes)
    assert isinstance(tree, ScenarioTree) and (tree.count, tree.T, tree.S, tree.total, tree.H, tree.N) == (5, 3, S, S, H, N)
    assert bool((tree.node_index[3] == -1).all()) and bool(torch.isnan(tree.cost[3]).all())
    leaves = tree.scenarios()
    assert isinstance(leaves, ScenarioSet) and (leaves.K, leaves.S, leaves.total) == (6, S, S)
    lx, lm = leaves.paths.cpu().numpy(), leaves.counts.cpu().numpy()
    assert same_bits(lx, TR.leaves(x, bounds, tree.node_index.cpu().numpy(), tree.assign.cpu().numpy()))
    assert np.isnan(lx[3]).all() and (lm[3] == 0).all() and (lm[[0, 1, 2, 4]].sum(axis=1) == S).all()
    taus = (0.05, 0.5, 0.95)
    assert same_bits(leaves.bands(taus).cpu().numpy(), W.bands(lx, lm, S, [W.rank(t, S) for t in taus]))
    sc = leaves.scores(d_y)
    from stemgnn_amd import ops
    o, h = ops.weighted_scores(d_y, leaves.paths, leaves.counts, S)
    check_scores((o.cpu().numpy(), h.cpu().numpy()), W.scores(truth, lx, lm, S), H)
    assert sc.absent == 1 and sc.crps == float(o[0])
    spec = EventSpec(1.0, min_run=2)
    ev = leaves.events(spec)
    assert np.array_equal(ev.counts.cpu().numpy(), W.events(lx, lm, S, np.full(N, 1.0), True, 2))
    # values, probabilities, conditional, expect
    for t in range(3):
        lo = (0,) + bounds
        v = tree.values(t)
        assert tuple(v.shape) == (5, nodes[t], bounds[t] - lo[t], N)
        assert tsame(v[0], d_x[0, tree.node_index[0, t, :nodes[t]], lo[t]:bounds[t]])
        p, q = tree.probabilities(t), tree.conditional(t)
        assert bool(torch.isnan(p[3]).all()) and bool(torch.isnan(q[3]).all())
        assert p[0].tolist() == [n / S for n in tree.counts[0, t, :nodes[t]].tolist()]
        above = [S] * nodes[t] if t == 0 else tree.counts[0, t - 1][tree.parent[0, t, :nodes[t]].long()].tolist()
        assert q[0].tolist() == [n / a for n, a in zip(tree.counts[0, t, :nodes[t]].tolist(), above)]
    const = torch.full((5, S, H), 3.5, device=DEV)
    assert bool((tree.expect(const)[[0, 1, 2, 4]] == 3.5).all())
    # the grouped metric is another tree; cat of two batches is the whole pass
    spec = EventSpec(0.0, groups=[[0, 1, 2, 3], [4, 5, 6, 7]])
    grouped = scenario_tree(d_x, bounds, nodes, on=spec, scale=0.5)
    assert not tsame(grouped.cost, tree.cost) and tuple(grouped.scenarios().paths.shape) == (5, 6, H, N)
    both = ScenarioTree.cat([scenario_tree(d_x[:2], bounds, nodes), scenario_tree(d_x[2:], bounds, nodes)])
    for name in ("node_index", "parent", "counts", "assign", "cost", "paths"):
        assert tsame(getattr(both, name), getattr(tree, name)), name
    assert all(tsame(both.values(t), tree.values(t)) for t in range(3)) and both.count == 5
    # export round-trips to the tensors
    out = tree.export(0)
    assert out["stages"] == bounds and out["nodes"] == nodes and out["total"] == S
    for t in range(3):
        assert np.array_equal(out["parent"][t], tree.parent[0, t, :nodes[t]].cpu().numpy())
        assert np.array_equal(out["probability"][t] * S, tree.counts[0, t, :nodes[t]].cpu().numpy())
        assert np.array_equal(out["conditional"][t], tree.conditional(t)[0].cpu().numpy())
        assert same_bits(out["values"][t], tree.values(t)[0].cpu().numpy())
    # a merged set's tree: the restatement with the merged counts
    ok = [0, 1, 2, 4]
    merged = ScenarioSet.merge([reduce_scenarios(d_x[:, :16].contiguous(), 6), reduce_scenarios(d_x[:, 16:].contiguous(), 6)])
    mt = merged.tree(bounds, (2, 3, 4))
    mx, mm = merged.paths.cpu().numpy(), merged.counts.cpu().numpy()
    Dm = ops.scenario_stage_distances(merged.paths[ok].contiguous(), bounds).cpu().numpy()
    want = TR.tree(Dm, mm[ok], S, (2, 3, 4))
    got = (mt.node_index.int(), mt.parent, mt.counts, mt.assign, mt.cost)
    assert same_tree(tuple(g[ok].cpu().numpy() for g in got), want) and (mt.S, mt.total) == (12, S)
    assert bool((mt.node_index[3] == -1).all())                                  # origin 3's NaN member refused one half
    assert same_bits(mt.paths[ok].cpu().numpy(), TR.leaves(mx[ok], bounds, want[0], want[3]))


def same_trees(a, b):
    return (a.stages, a.nodes, a.S, a.total) == (b.stages, b.nodes, b.S, b.total) and \
        all(tsame(getattr(a, n), getattr(b, n)) for n in ("node_index", "parent", "counts", "assign", "cost", "paths")) and \
        all(tsame(a.values(t), b.values(t)) for t in range(a.T))


def test_trees_of_a_model_end_to_end():
    from stemgnn_amd import EventSpec, LiveForecaster, Model, scenario_tree, trainer
    from tests.test_hip_reduce import H_E, N_E, TAUS_E, W_E
    torch.manual_seed(SEED)
    model = Model(N_E, 2, W_E, 2, horizon=H_E, quantiles=TAUS_E).to(DEV).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(5, W_E, N_E, generator=g).to(DEV)
    y = torch.randn(5, 7, N_E, generator=g).to(DEV)
    graph = model.latent_graph(x)
    whole, split = [(x, y)], [(x[:2], y[:2]), (x[2:], y[2:])]
    kw = dict(paths=16, seed=11, adjacency=graph)
    bands0, target0, paths0 = trainer.rolling_scenarios(model, whole, 7, return_paths=True, **kw)
    spec = EventSpec(0.0, groups=[[0, 1, 2, 3], [4, 5, 6, 7, 8]])
    for red in (dict(), dict(on=spec), dict(scale=torch.linspace(0.5, 2.0, N_E), squared=True)):
        want = scenario_tree(paths0, (2, 4, 7), (2, 3, 5), **red)
        assert bool((want.counts.sum(dim=2) == 16).all())
        for loader in (whole, split):                                            # 5 windows at once == 2 + 3
            b, t, got = trainer.scenario_trees(model, loader, 7, (2, 4, 7), (2, 3, 5), **kw, **red)
            assert tsame(b, bands0) and tsame(t, target0) and same_trees(got, want)
    live = LiveForecaster(model, W_E, 7, history=4, adjacency=graph)
    live.push(np.random.default_rng(SEED + 3).normal(size=(W_E + 2, N_E)))
    live.seed = 21
    before = live.forecast()
    for red in (dict(), dict(on=spec, scale=2.0)):
        got = live.scenario_tree((3, 7), (2, 4), paths=8, **red)
        want = scenario_tree(live.scenarios(paths=8, return_paths=True)[1][None], (3, 7), (2, 4), **red)
        assert got.count == 1 and got.S == 8 and same_trees(got, want)
    assert tsame(live.forecast(), before)
