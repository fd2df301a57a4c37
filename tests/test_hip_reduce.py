"""GPU: scenario reduction -- the two kernels of csrc/reduce.hip against the numpy restatement of their definition
(tests/helpers/reduce_ref.py), and math_utils.reduce_scenarios / ScenarioSet through trainer.reduced_scenarios and
LiveForecaster.scenario_set.

Every output lies inside a guarded buffer (NaN for the fp64 ones, -7 for the int32 ones), compared whole: what the definition does
not write must still hold the guard.  The distances carry the issue's bound, derived and not measured:
|got - ref| <= (L + 8) 2^-53 ref against the longdouble restatement -- one rounding per difference, per scaling and per fused
multiply-add, halved by the root, plus the root's own -- and twice that without the root.  The reduction is compared bit for
bit: the restatement adds in the definition's order."""
import numpy as np
import pytest
import torch

from tests.helpers import reduce_ref as R
from tests.test_hip_scenario import DEV, GUARD, SEED, device_copy, same_bits, tsame

pytestmark = pytest.mark.gpu
NAN, INF = np.nan, np.inf


def guarded64(shape):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), NAN, device=DEV, dtype=torch.float64)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def guarded32(shape):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), -7, device=DEV, dtype=torch.int32)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def inside(whole, shape, guard_ok):
    """the view of `shape` inside a guarded host copy, after checking that both guards still hold"""
    n = int(np.prod(shape))
    got = whole.cpu().numpy()
    assert guard_ok(got[:GUARD]).all() and guard_ok(got[GUARD + n:]).all()
    return got[GUARD:GUARD + n].reshape(shape)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def run_distances(lib, d_x, d_scale, squared):
    count, S, L = d_x.shape
    whole, d_D = guarded64((count, S, S))
    rc = lib.stemgnn_scenario_distances(d_x.data_ptr(), None if d_scale is None else d_scale.data_ptr(), count, S, L, squared,
                                        d_D.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return inside(whole, (count, S, S), np.isnan)


def run_reduce(lib, d_D, K):
    count, S, _ = d_D.shape
    outs = [guarded32((count, K)), guarded32((count, K)), guarded32((count, S)), guarded64((count, K))]
    rc = lib.stemgnn_scenario_reduce(d_D.data_ptr(), count, S, K, *(view.data_ptr() for _, view in outs), None)
    assert rc == 0
    torch.cuda.synchronize()
    is_guard = lambda v: v == -7                                                 # noqa: E731
    return (inside(outs[0][0], (count, K), is_guard), inside(outs[1][0], (count, K), is_guard),
            inside(outs[2][0], (count, S), is_guard), inside(outs[3][0], (count, K), np.isnan))


def same_reduction(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3].shape == want[3].shape and \
        np.array_equal(bits64(got[3])[~np.isnan(want[3])], bits64(want[3])[~np.isnan(want[3])]) and \
        np.array_equal(np.isnan(got[3]), np.isnan(want[3]))


# one path; a ragged tile; one past a tile; exactly two tiles and 42 full chunks + 48; one past two tiles; the most tiles; L = 1;
# exactly one chunk of L (64: the largest L the wide form, which shares the chunks out over four wave groups, is not taken at;
# 65 above is the smallest it is); 300 origins of one tile pair: more workgroups than compute units, so the whole call takes the
# 256-thread form and the one-origin call of the split below the wide one -- the two forms must give the same bits (6 chunks: the
# four partial sums get 2, 2, 1 and 1); the same with off-diagonal tiles
DIST_SHAPES = [(1, 1, 1), (3, 5, 7), (2, 33, 65), (1, 64, 2736), (2, 65, 130), (1, 1024, 3), (1, 97, 1), (2, 4, 64),
               (300, 5, 330), (100, 33, 130)]


@pytest.mark.parametrize("shape", DIST_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_distances_match_the_longdouble_restatement(shape):
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, S, L = shape
    rng = np.random.default_rng(SEED + 7 * count + 11 * S + 13 * L)
    x = rng.normal(size=shape).astype(np.float32)
    if S >= 2:
        x[:, S - 1] = x[:, 0]                                                    # a duplicated path
    if S >= 4:
        x[:, 2] = x[:, 1] + np.float32(2.0 ** -20) * rng.normal(size=(count, L)).astype(np.float32)   # nearly coincident paths
    scale = rng.uniform(0.25, 4.0, size=L)
    d_scale = torch.from_numpy(scale).to(DEV)
    worst = 0.0
    for sc in (None, scale):
        for squared in (0, 1):
            ref = R.distances(x, sc, bool(squared))
            bound = (2 if squared else 1) * (L + 8) * np.longdouble(2.0) ** -53 * ref
            for misalign in (False, True):
                _, d_x = device_copy(x, misalign)
                got = run_distances(lib, d_x, None if sc is None else d_scale, squared)
                err = np.abs(got.astype(np.longdouble) - ref)
                assert (err <= bound).all(), (sc is not None, squared, misalign, float((err - bound).max()))
                if (bound > 0).any():
                    worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()))
                diag = got[:, np.arange(S), np.arange(S)]
                assert (diag == 0).all() and not np.signbit(diag).any()           # exactly +0
                assert np.array_equal(bits64(got), bits64(np.transpose(got, (0, 2, 1))))
                if S >= 2:
                    assert (got[:, 0, S - 1] == 0).all() and (got[:, S - 1, 0] == 0).all()
                assert np.array_equal(bits64(run_distances(lib, d_x, None if sc is None else d_scale, squared)), bits64(got))
                assert same_bits(d_x.cpu().numpy(), x)
                if count > 1:                                                    # the origins over two calls: the whole
                    a = run_distances(lib, d_x[:1], None if sc is None else d_scale, squared)
                    b = run_distances(lib, d_x[1:], None if sc is None else d_scale, squared)
                    assert np.array_equal(bits64(np.concatenate([a, b])), bits64(got))
    print(f"{shape}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("shape", [(2, 33, 65), (1, 65, 3)], ids=lambda s: "-".join(str(v) for v in s))
def test_a_nan_reaches_its_row_and_column_only(shape):
    from stemgnn_amd import _lib, ops
    lib = _lib.load()
    count, S, L = shape
    x = np.random.default_rng(SEED + 5).normal(size=shape).astype(np.float32)
    bad = S - 2
    x[0, bad, L // 2] = NAN
    _, d_x = device_copy(x, False)
    for squared in (0, 1):
        got = run_distances(lib, d_x, None, squared)
        want = np.zeros((count, S, S), bool)
        want[0, bad, :] = want[0, :, bad] = True                                 # the diagonal entry too: NaN - NaN
        assert np.array_equal(np.isnan(got), want)
    # ops on the same values: the same bits, and that origin alone is refused downstream
    D = ops.scenario_distances(d_x.view(count, S, 1, L))
    assert np.array_equal(np.isnan(D.cpu().numpy()), want)
    sel, cnt, asg, cost = ops.scenario_reduce(d_x.view(count, S, 1, L), 3)
    assert (sel[0] == -1).all() and (cnt[0] == 0).all() and (asg[0] == -1).all() and bool(torch.isnan(cost[0]).all())
    if count > 1:
        assert (sel[1] >= 0).all() and int(cnt[1].sum()) == S


# one path; K = S; a ragged wave; the flagship shape; K = S at 64; one past a wave; the most paths (D read from memory);
# K above a wave's worth of picks; the last S whose D is held in LDS and the first that is not
RED_SHAPES = [(1, 1, 1), (3, 5, 5), (2, 33, 8), (4, 64, 8), (1, 64, 64), (2, 65, 3), (1, 1024, 4), (1, 200, 17), (2, 141, 5),
              (2, 142, 5)]


def check_reduction(lib, D, K):
    """the device on D [count, S, S] float64 (host) against the restatement; returns the device's results"""
    count, S, _ = D.shape
    d_D = torch.from_numpy(np.ascontiguousarray(D)).to(DEV)
    got = run_reduce(lib, d_D, K)
    want = R.forward(D, K)
    assert same_reduction(got, want), (count, S, K)
    sel, cnt, asg, cost = got
    ok = sel[:, 0] >= 0
    assert (np.diff(cost[ok], axis=1) <= 0).all() and (cnt[ok].sum(axis=1) == S).all()
    for c in np.nonzero(ok)[0]:
        assert len(set(sel[c].tolist())) == K and (np.bincount(asg[c], minlength=K) == cnt[c]).all()
        want_cost = R.subset_cost(D[c], sel[c])
        assert abs(cost[c, K - 1] - want_cost) <= 1e-13 * want_cost
    assert np.array_equal(bits64(d_D.cpu().numpy()), bits64(D))                  # the input is unchanged
    again = run_reduce(lib, d_D, K)
    assert all(np.array_equal(a, b) for a, b in zip(again[:3], got[:3])) and \
        np.array_equal(bits64(again[3]), bits64(got[3]))                         # two runs
    return got


@pytest.mark.parametrize("shape", RED_SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_reduce_matches_the_restatement_bit_for_bit(shape):
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, S, K = shape
    rng = np.random.default_rng(SEED + 3 * count + 5 * S + 7 * K)
    # the device's own distances of random paths
    x = rng.normal(size=(count, S, 6)).astype(np.float32)
    _, d_x = device_copy(x, False)
    D = run_distances(lib, d_x, None, 0)
    sel, cnt, asg, cost = check_reduction(lib, D, K)
    # the first k picks at K are the picks at K = k
    for k in sorted({1, (K + 1) // 2}):
        d_D = torch.from_numpy(D).to(DEV)
        part = run_reduce(lib, d_D, k)
        assert np.array_equal(part[0], sel[:, :k]) and np.array_equal(bits64(part[3]), bits64(cost[:, :k]))
    # blocks of duplicated paths: many exact ties, at zero and elsewhere
    dup = x[:, rng.integers(0, max(1, S // 4), size=S)]
    _, d_dup = device_copy(np.ascontiguousarray(dup), False)
    check_reduction(lib, run_distances(lib, d_dup, None, 1), K)
    # small integers, not symmetric, a non-zero diagonal: many equal z, the lowest index must win
    check_reduction(lib, rng.integers(0, 3, size=(count, S, S)).astype(np.float64), K)
    check_reduction(lib, np.ones((count, S, S)), K)
    # an asymmetric cost of the caller's
    check_reduction(lib, rng.uniform(0.0, 1.0, size=(count, S, S)) * rng.uniform(0.1, 10.0, size=(count, 1, S)), K)


@pytest.mark.parametrize("S", [33, 200])
def test_one_refused_origin_leaves_the_others_alone(S):
    from stemgnn_amd import _lib
    lib = _lib.load()
    rng = np.random.default_rng(SEED + S)
    K = 4
    for poison in (INF, NAN, -1.0, -INF):
        D = rng.uniform(0.5, 2.0, size=(4, S, S))
        D[2, S - 1, 1] = poison
        sel, cnt, asg, cost = check_reduction(lib, D, K)
        assert (sel[2] == -1).all() and (cnt[2] == 0).all() and (asg[2] == -1).all() and np.isnan(cost[2]).all()
        for c in (0, 1, 3):                                                      # as when they are alone in the call
            alone = run_reduce(lib, torch.from_numpy(D[c:c + 1]).to(DEV), K)
            assert np.array_equal(alone[0][0], sel[c]) and np.array_equal(alone[1][0], cnt[c])
            assert np.array_equal(alone[2][0], asg[c]) and np.array_equal(bits64(alone[3][0]), bits64(cost[c]))


def test_ops_batches_equal_the_one_call():
    from stemgnn_amd import ops
    count, S, H, M, K = 7, 33, 3, 5, 6
    x = torch.from_numpy(np.random.default_rng(SEED + 9).normal(size=(count, S, H, M)).astype(np.float32)).to(DEV)
    scale = torch.linspace(0.5, 2.0, M)
    for kw in (dict(), dict(scale=scale), dict(scale=scale[None].expand(H, M) * torch.arange(1, H + 1)[:, None], squared=True),
               dict(scale=0.5)):
        whole = ops.scenario_reduce(x, K, **kw)
        three = ops.scenario_reduce(x, K, max_scratch_bytes=3 * S * S * 8, **kw)  # 3 + 3 + 1 origins
        one = ops.scenario_reduce(x, K, max_scratch_bytes=S * S * 8, **kw)
        D = ops.scenario_distances(x, **kw)
        given = ops.scenario_reduce(None, K, distances=D, max_scratch_bytes=3 * S * S * 8)
        for other in (three, one, given):
            assert all(tsame(a, b) for a, b in zip(whole, other))
        assert whole[0].dtype == torch.int32 and whole[3].dtype == torch.float64 and tuple(whole[2].shape) == (count, S)
        want = R.forward(D.cpu().numpy(), K)
        assert same_reduction(tuple(t.cpu().numpy() for t in whole), want)
        sc = None if "scale" not in kw else (torch.as_tensor(kw["scale"], dtype=torch.float64).expand(H, M).reshape(-1).numpy())
        ref = R.distances(x.cpu().numpy().reshape(count, S, H * M), sc, kw.get("squared", False))
        err = np.abs(D.cpu().numpy().astype(np.longdouble) - ref)
        assert (err <= (2 if kw.get("squared") else 1) * (H * M + 8) * np.longdouble(2.0) ** -53 * ref).all()


def test_the_cluster_case():
    """Three clusters of 32, 20 and 12 paths (64 paths, H = 12, M = 5; centres N(0, 10^2) per coordinate, unit noise).  The issue's
    conditions, exact: at keep = 3 the sorted counts are [12, 20, 32], assign reproduces the cluster labels, and
    cost[2] < 0.5 cost[1] (numpy, six seeds: 9.4 - 10.1 against 25.2 - 31.4; at this seed 9.60 against 31.36)."""
    from stemgnn_amd import reduce_scenarios
    x, labels = R.cluster_case(SEED + 1)
    kept = reduce_scenarios(torch.from_numpy(x).to(DEV), 3)
    counts, assign, cost = kept.counts[0].cpu().numpy(), kept.assign[0].cpu().numpy(), kept.cost[0].cpu().numpy()
    print(f"device: counts {counts.tolist()}, cost {cost.tolist()}")
    assert R.cluster_conditions(labels, counts, assign, cost)
    assert kept.weights[0].tolist() == [c / 64 for c in counts.tolist()] and kept.S == 64
    assert tsame(kept.paths[0], torch.from_numpy(x[0][kept.index[0].cpu().numpy()]).to(DEV))


def test_the_value_case():
    """The block-correlated walk (correlation 0.9 inside two blocks of 8 nodes; 256 origins, 64 paths, 12 steps, keep = 8),
    functional = the peak over the steps of the 16-node mean; reduce_scenarios against the first 8 paths at equal weights.  The
    issue's conditions, each about half the margin seen in numpy on other seeds: the mean absolute error of the expectation
    against the full ensemble's at most 0.8 x the first eight's (seen 0.55 - 0.65); cost[7] <= subset_cost(first 8) at 0.99 of
    the origins at least (seen 1.00); mean cost[7] <= 0.95 x mean subset_cost(first 8) (seen 0.872 - 0.882).  The restatement
    alone, at this seed (tests/test_reduce_abi.py): 0.6451, 1.0000, 0.8754.  The device's are printed."""
    from stemgnn_amd import ops, reduce_scenarios
    paths = R.walk_case(SEED + 2)
    d_paths = torch.from_numpy(paths).to(DEV)
    kept = reduce_scenarios(d_paths, R.WALK_K)
    peak = R.peak_of_mean(paths)
    D = ops.scenario_distances(d_paths).cpu().numpy()
    fig = R.value_figures(peak, D, kept.index.cpu().numpy(), kept.counts.cpu().numpy(), kept.cost.cpu().numpy())
    print(f"device: error ratio {fig[0]:.4f}, share {fig[1]:.4f}, cost ratio {fig[2]:.4f}")
    assert R.value_conditions(fig)
    # expect() is that weighted sum
    want = (np.take_along_axis(peak, kept.index.cpu().numpy(), axis=1) * kept.weights.cpu().numpy()).sum(axis=1)
    got = kept.expect(torch.from_numpy(peak).to(DEV)).cpu().numpy()
    assert np.abs(got - want).max() <= 1e-14 * np.abs(want).max()
    # and the device's reduction is the restatement's of the device's distances
    assert same_reduction((kept.index.cpu().numpy(), kept.counts.cpu().numpy(), kept.assign.cpu().numpy(), kept.cost.cpu().numpy()),
                          R.forward(D, R.WALK_K))


# ---- through the layers: the small quantile model of tests/test_hip_events.py --------------------------------------------------
N_E, W_E, H_E, TAUS_E = 9, 12, 3, (0.1, 0.5, 0.9)


def same_set(a, b, paths=True):
    return a.S == b.S and tsame(a.index, b.index) and tsame(a.counts, b.counts) and tsame(a.assign, b.assign) and \
        tsame(a.cost, b.cost) and (not paths or tsame(a.paths, b.paths))


def test_reduction_of_a_model_end_to_end():
    from stemgnn_amd import EventSpec, LiveForecaster, Model, ScenarioSet, reduce_scenarios, trainer
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
    scale = torch.linspace(0.5, 2.0, N_E)
    for red in (dict(), dict(on=spec), dict(scale=scale, squared=True)):
        want = reduce_scenarios(paths0, 4, **red)
        assert isinstance(want, ScenarioSet) and (want.count, want.K, want.S, want.H, want.N) == (5, 4, 16, 7, N_E)
        assert want.index.dtype == torch.int64 and int(want.index.min()) >= 0 and bool((want.counts.sum(1) == 16).all())
        for loader in (whole, split):                                            # 5 windows at once == 2 + 3
            b, t, got = trainer.reduced_scenarios(model, loader, 7, 4, **kw, **red)
            assert tsame(b, bands0) and tsame(t, target0) and same_set(got, want)
            assert got.source is None and got.distances is None                  # the pass keeps count * keep paths
        # the kept paths are the paths at the kept indices
        assert tsame(want.paths, torch.stack([paths0[c, want.index[c]] for c in range(5)]))
        # head(k) is the reduction at keep = k (from the paths the set still refers to)
        for k in (1, 3):
            assert same_set(want.head(k), reduce_scenarios(paths0, k, **red))
    want = reduce_scenarios(paths0, 4)
    on = spec.aggregate(paths0)
    assert same_set(reduce_scenarios(paths0, 4, on=spec), reduce_scenarios(paths0, 4, on=on))
    assert not tsame(reduce_scenarios(paths0, 4, on=on).cost, want.cost)          # the aggregate is another distance
    # cat of two halves is the whole
    halves = ScenarioSet.cat([reduce_scenarios(paths0[:2], 4), reduce_scenarios(paths0[2:], 4)])
    assert same_set(halves, want) and halves.count == 5
    # keep_for
    assert want.keep_for(1.0).tolist() == [1] * 5 and want.keep_for(1.0).dtype == torch.int64
    cost = want.cost.cpu().numpy()
    zero = [int(np.argmax(row == 0)) + 1 if (row == 0).any() else 4 for row in cost]
    assert want.keep_for(0.0).tolist() == zero
    every = reduce_scenarios(paths0, 16)
    assert bool((every.cost[:, -1] == 0).all()) and every.keep_for(0.0).tolist() == \
        [int(np.argmax(row == 0)) + 1 for row in every.cost.cpu().numpy()]
    loose = want.keep_for(0.8).cpu().numpy()
    assert all(k == 4 or cost[c, k - 1] <= 0.8 * cost[c, 0] for c, k in enumerate(loose)) and \
        all(k == 1 or cost[c, k - 2] > 0.8 * cost[c, 0] for c, k in enumerate(loose))
    # expect of a constant is that constant, exactly (S = 16, a power of two); of the paths themselves: the weighted kept paths
    const = torch.full((5, 16, 7), 3.7, device=DEV)
    assert bool((want.expect(const) == float(np.float32(3.7))).all()) and want.expect(const).dtype == torch.float64
    mean = want.expect(paths0)
    assert tuple(mean.shape) == (5, 7, N_E)
    ref = (want.paths.double() * want.weights[:, :, None, None]).sum(dim=1)
    assert float((mean - ref).abs().max()) <= 1e-14 * float(ref.abs().max())
    # LiveForecaster.scenario_set on the head window, and forecast() is left as it was
    live = LiveForecaster(model, W_E, 7, history=4, adjacency=graph)
    live.push(np.random.default_rng(SEED + 3).normal(size=(W_E + 2, N_E)))
    live.seed = 21
    before = live.forecast()
    for red in (dict(), dict(on=spec, scale=2.0)):
        got = live.scenario_set(3, paths=8, **red)
        want = reduce_scenarios(live.scenarios(paths=8, return_paths=True)[1][None], 3, **red)
        assert got.count == 1 and got.S == 8 and got.K == 3 and same_set(got, want)
    assert tsame(live.forecast(), before)
