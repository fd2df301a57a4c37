"""GPU: the weighted scenario-set entries of csrc/weighted.hip against the numpy restatement of their definitions
(tests/helpers/weighted_ref.py, the primary reference) and against the project's unweighted entries on the replicated ensemble
(the second one), then math_utils.ScenarioSet's bands / scores / events / reduce / merge through the layers.

Every output lies inside a guarded buffer (NaN for fp32 and fp64, -7 for the integers) and is compared whole; the inputs are
checked unchanged; every case runs 16-byte aligned and 4 bytes off.  Bands are compared bit for bit, event counts, `hist` and
out[4..6] exactly.  The bound on out[0..3] is the one of tests/test_hip_ensemble.py, derived and not measured: every sum of the
definition adds non-negative terms (the weight products are exact), so its relative error is at most (n - 1) 2^-53 for n
terms; n <= 2^23 at these shapes, 9.4e-10 -- each of the two terms of [0] and [1] is within 1e-9 of itself and the statistic
within 1e-9 (|first| + |second|); [2] and [3] are a square root of one such sum: 1e-9 relative.  Against the unweighted entry,
which carries the same bound against the same exact value, twice that.  (The walk case at keep = S adds 2^27.6 pair terms in
all, beyond 2^23; the bound is kept as it is: neither side adds them in one chain -- the kernels' longest chain is a thread's
walk over at most 256 members, then fixed trees, and numpy sums pairwise -- so the (n - 1) 2^-53 of a single chain is far from
reached; the worst error seen is 4e-7 of the bound.)  The reduction is compared bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

from tests.helpers import reduce_ref as R
from tests.helpers import weighted_ref as W
from tests.test_hip_scenario import DEV, GUARD, SEED, device_copy, guarded, same_bits, tsame

pytestmark = pytest.mark.gpu
RTOL = 1e-9
TAUS = (0.05, 0.5, 0.95, 1.0)
WSEED = 20261023                 # the walk case of tests/test_weighted_abi.py


def guarded_as(shape, dtype, fill):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), fill, device=DEV, dtype=dtype)
    return whole, whole[GUARD:GUARD + n].view(*shape)


def inside(whole, shape, guard_ok, lead=GUARD):
    """the view of `shape` inside a guarded host copy, after checking that both guards still hold"""
    n = int(np.prod(shape))
    got = whole.cpu().numpy()
    assert guard_ok(got[:lead]).all() and guard_ok(got[lead + n:]).all()
    return got[lead:lead + n].reshape(shape)


def is_guard(v):
    return v == -7


def dev_mult(mult):
    return torch.from_numpy(np.ascontiguousarray(mult, np.int32)).to(DEV)


def run_bands(lib, d_paths, d_mult, Wt, ranks, misalign):
    count, K, H, N = d_paths.shape
    Q = len(ranks)
    whole, d_b = guarded((count, Q, H, N), misalign)
    rc = lib.stemgnn_weighted_bands(d_paths.data_ptr(), d_mult.data_ptr(), count, K, H, N, Wt, Q, (ctypes.c_int * Q)(*ranks),
                                    d_b.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    lead = int((d_b.data_ptr() - whole.data_ptr()) // 4)
    return inside(whole, (count, Q, H, N), np.isnan, lead)


def run_events(lib, d_paths, d_mult, Wt, d_thr, above, min_run, d_mul=None, d_add=None):
    count, K, H, M = d_paths.shape
    whole, d_c = guarded_as((count, 2 * H + 1, M), torch.int32, -7)
    rc = lib.stemgnn_weighted_events(d_paths.data_ptr(), d_mult.data_ptr(), d_thr.data_ptr(),
                                     None if d_mul is None else d_mul.data_ptr(), None if d_add is None else d_add.data_ptr(),
                                     count, K, H, M, Wt, int(above), min_run, d_c.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return inside(whole, (count, 2 * H + 1, M), is_guard)


def run_scores(lib, d_y, d_paths, d_mult, Wt, d_mul=None, d_add=None, masked=False, fair=False):
    count, K, H, N = d_paths.shape
    n_out = lib.stemgnn_weighted_out_doubles(H)
    assert n_out == 7 * (1 + H)
    scratch = torch.full((lib.stemgnn_weighted_scratch_doubles(count, K, H, N),), np.nan, device=DEV, dtype=torch.float64)
    w_out, d_out = guarded_as((n_out,), torch.float64, np.nan)
    w_hist, d_hist = guarded_as((H, Wt + 1), torch.int64, -7)
    rc = lib.stemgnn_weighted_scores(d_y.data_ptr(), d_paths.data_ptr(), d_mult.data_ptr(),
                                     None if d_mul is None else d_mul.data_ptr(), None if d_add is None else d_add.data_ptr(),
                                     count, K, H, N, Wt, int(fair), int(masked), scratch.data_ptr(), d_out.data_ptr(),
                                     d_hist.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return inside(w_out, (n_out,), np.isnan), inside(w_hist, (H, Wt + 1), is_guard)


def run_parent_scores(lib, d_y, d_rep, d_mul=None, d_add=None, masked=False, fair=False):
    count, S, H, N = d_rep.shape
    entry = lib.stemgnn_ensemble_scores_masked if masked else lib.stemgnn_ensemble_scores
    scratch = torch.empty(lib.stemgnn_ensemble_scratch_doubles(count, S, H, N), device=DEV, dtype=torch.float64)
    out = torch.empty(6 * (1 + H), device=DEV, dtype=torch.float64)
    hist = torch.empty(H, S + 1, device=DEV, dtype=torch.int64)
    rc = entry(d_y.data_ptr(), d_rep.data_ptr(), None if d_mul is None else d_mul.data_ptr(),
               None if d_add is None else d_add.data_ptr(), count, S, H, N, int(fair), scratch.data_ptr(), out.data_ptr(),
               hist.data_ptr(), None)
    assert rc == 0
    torch.cuda.synchronize()
    return out.cpu().numpy(), hist.cpu().numpy()


def check_scores(got, ref, H, scale=1.0, width=7):
    """out (width 7) against a reference dict or a parent's out (width 6); returns the worst error over its bound"""
    out, hist = got
    assert np.array_equal(hist, ref["hist"])
    worst = 0.0
    for at in range(1 + H):
        for k in range(width):
            g = out[k if at == 0 else 7 + k * H + at - 1]
            e = ref["out"][k if at == 0 else width + k * H + at - 1]
            if k >= 4:
                assert g == e, (at, k, g, e)
                continue
            if np.isnan(e):
                assert np.isnan(g), (at, k, g)
                continue
            bound = scale * RTOL * ((abs(ref["first"][k, at]) + abs(ref["second"][k, at])) if k < 2 else abs(e))
            assert abs(g - e) <= bound, (at, k, g, e, abs(g - e), bound)
            if bound > 0:
                worst = max(worst, abs(g - e) / bound)
    return worst


def make_case(shape):
    count, K, H, N, Wt = shape
    rng = np.random.default_rng(SEED + 3 * count + 5 * K + 7 * H + 11 * N + 13 * Wt)
    paths, target, mult = W.random_set(rng, count, K, H, N, Wt)
    live = np.nonzero(mult[0] > 0)[0]
    paths[0, live[0], 0, 0] = target[0, 0, 0]                                    # a tie at the target
    if live.size > 1:
        paths[0, live[1], 0, 0] = target[0, 0, 0]
        paths[count - 1, live[0], H - 1, N - 1] = np.float32(-0.0)              # -0 and +0 are one value, the lower index first
        paths[count - 1, live[1], H - 1, N - 1] = np.float32(0.0)
    if count >= 3:
        mult[1, 0] += 1                                                          # a wrong sum
        mult[2, 0] = -1 - mult[2, 0]                                             # a negative multiplicity
        if K > 1:
            mult[2, 1] += Wt - mult[2].sum()                                     # .. whose sum is still W
    return rng, paths, target, mult


# the smallest case; the scalar path; the real reduced shape with a ragged node tile; the walk shape; one past a 32-member tile;
# the largest K; more workgroups than compute units
SHAPES = [(1, 1, 1, 1, 1), (3, 2, 2, 5, 7), (4, 8, 3, 70, 64), (5, 8, 12, 16, 64), (2, 33, 1, 64, 100), (2, 256, 1, 8, 1000),
          (300, 3, 2, 4, 5)]
IDS = lambda s: "-".join(str(v) for v in s)                                      # noqa: E731


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bands_match_the_restatement_and_the_replicated_ensemble(shape):
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, K, H, N, Wt = shape
    rng, paths, target, mult = make_case(shape)
    ranks = [W.rank(t, Wt) for t in TAUS]
    assert ranks == [int(lib.stemgnn_scenario_rank(t, Wt)) for t in TAUS]
    want = W.bands(paths, mult, Wt, ranks)
    ok = W.present(mult, Wt)
    assert (want[~ok].view(np.uint32) == 0x7FC00000).all() and ok.sum() >= count - 2
    d_mult = dev_mult(mult)
    d_ranks = (ctypes.c_int * len(ranks))(*ranks)
    for misalign in (False, True):
        _, d_paths = device_copy(paths, misalign)
        got = run_bands(lib, d_paths, d_mult, Wt, ranks, misalign)
        assert same_bits(got, want)
        assert same_bits(run_bands(lib, d_paths, d_mult, Wt, ranks, misalign), got)            # the same bits on every run
        assert same_bits(d_paths.cpu().numpy(), paths) and np.array_equal(d_mult.cpu().numpy(), mult)
        if count > 1:                                                            # the origins over two calls: the whole
            a = run_bands(lib, d_paths[:1], d_mult[:1], Wt, ranks, misalign)
            b = run_bands(lib, d_paths[1:], d_mult[1:], Wt, ranks, misalign)
            assert same_bits(np.concatenate([a, b]), got)
        # the second reference: the project's own bands of the replicated ensemble (the present origins)
        rep = W.replicate(paths[ok], mult[ok])
        _, d_rep = device_copy(rep, misalign)
        whole, d_b = guarded((int(ok.sum()), len(ranks), H, N), misalign)
        assert lib.stemgnn_scenario_bands(d_rep.data_ptr(), int(ok.sum()), Wt, H, N, len(ranks), d_ranks, 0, d_b.data_ptr(),
                                          None) == 0
        torch.cuda.synchronize()
        assert same_bits(d_b.cpu().numpy(), got[ok])


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_events_match_the_restatement_and_the_replicated_ensemble(shape):
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, K, H, M, Wt = shape
    rng, paths, target, mult = make_case(shape)
    ok = W.present(mult, Wt)
    mul, add = rng.uniform(0.5, 2.0, M), rng.normal(size=M)
    thr = rng.normal(size=M) * 0.5
    thr[0] = target[0, 0, 0]                                                     # a value on the threshold: strict, not in the event
    d_thr, d_mul, d_add = (torch.from_numpy(v).to(DEV) for v in (thr, mul, add))
    d_mult = dev_mult(mult)
    rep = W.replicate(paths[ok], mult[ok])
    n_ok = int(ok.sum())
    for misalign in (False, True):
        _, d_paths = device_copy(paths, misalign)
        _, d_rep = device_copy(rep, misalign)
        for above in (0, 1):
            for min_run in sorted({1, min(2, H), H}):
                for dn in (False, True):
                    kw = dict(mul=mul, add=add) if dn else {}
                    dkw = dict(d_mul=d_mul, d_add=d_add) if dn else {}
                    want = W.events(paths, mult, Wt, thr, bool(above), min_run, **kw)
                    got = run_events(lib, d_paths, d_mult, Wt, d_thr, above, min_run, **dkw)
                    assert np.array_equal(got, want), (above, min_run, dn)
                    assert (got[~ok] == -1).all()
                    assert np.array_equal(run_events(lib, d_paths, d_mult, Wt, d_thr, above, min_run, **dkw), got)
                    parent = torch.full((n_ok, 2 * H + 1, M), -7, device=DEV, dtype=torch.int32)
                    assert lib.stemgnn_scenario_events(d_rep.data_ptr(), d_thr.data_ptr(), d_mul.data_ptr() if dn else None,
                                                       d_add.data_ptr() if dn else None, n_ok, Wt, H, M, above, min_run,
                                                       parent.data_ptr(), None) == 0
                    assert np.array_equal(parent.cpu().numpy(), got[ok])
        if count > 1:
            a = run_events(lib, d_paths[:1], d_mult[:1], Wt, d_thr, 1, 1)
            b = run_events(lib, d_paths[1:], d_mult[1:], Wt, d_thr, 1, 1)
            assert np.array_equal(np.concatenate([a, b]), run_events(lib, d_paths, d_mult, Wt, d_thr, 1, 1))
        assert same_bits(d_paths.cpu().numpy(), paths) and np.array_equal(d_mult.cpu().numpy(), mult)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_scores_match_the_restatement_and_the_replicated_ensemble(shape):
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, K, H, N, Wt = shape
    rng, paths, target, mult = make_case(shape)
    ok = W.present(mult, Wt)
    mul, add = rng.uniform(0.5, 2.0, N), rng.normal(size=N)
    d_mul, d_add = torch.from_numpy(mul).to(DEV), torch.from_numpy(add).to(DEV)
    d_mult = dev_mult(mult)
    holes = target.copy()
    holes[count - 1, H - 1, N - 1] = np.nan                                      # a missing reading
    if N > 1:
        holes[0, 0, :] = np.nan                                                  # a row with none
    rep = W.replicate(paths[ok], mult[ok])
    variants = [dict(), dict(dn=True), dict(masked=True), dict(dn=True, masked=True)] + ([dict(fair=True)] if Wt > 1 else [])
    worst = [0.0, 0.0]
    for v in variants:
        dn, masked, fair = v.get("dn", False), v.get("masked", False), v.get("fair", False)
        y = holes if (masked or dn) else target                                  # unmasked with mul / add: the NaN propagates
        kw = dict(mul=mul, add=add) if dn else {}
        dkw = dict(d_mul=d_mul, d_add=d_add) if dn else {}
        ref = W.scores(y, paths, mult, Wt, masked=masked, fair=fair, **kw)
        assert ref["out"][6] == float((~ok).sum())
        for misalign in (False, True):
            _, d_paths = device_copy(paths, misalign)
            _, d_y = device_copy(y, misalign)
            got = run_scores(lib, d_y, d_paths, d_mult, Wt, masked=masked, fair=fair, **dkw)
            worst[0] = max(worst[0], check_scores(got, ref, H))
            again = run_scores(lib, d_y, d_paths, d_mult, Wt, masked=masked, fair=fair, **dkw)
            assert np.array_equal(got[0].view(np.int64), again[0].view(np.int64)) and np.array_equal(got[1], again[1])
            assert same_bits(d_paths.cpu().numpy(), paths) and same_bits(d_y.cpu().numpy(), y)
            # the second reference: the project's own scores of the replicated ensemble of the present origins
            _, d_rep = device_copy(rep, misalign)
            _, d_yok = device_copy(y[ok], misalign)
            p_out, p_hist = run_parent_scores(lib, d_yok, d_rep, masked=masked, fair=fair, **dkw)
            second = dict(out=p_out, hist=p_hist, first=ref["first"], second=ref["second"])
            worst[1] = max(worst[1], check_scores(got, second, H, scale=2.0, width=6))
            if count > 1 and not v:                                              # two calls: each against its own restatement
                hist = np.zeros_like(got[1])
                for sl in (slice(0, 1), slice(1, None)):
                    part = run_scores(lib, d_y[sl], d_paths[sl], d_mult[sl], Wt)
                    check_scores(part, W.scores(y[sl], paths[sl], mult[sl], Wt), H)
                    hist += part[1]
                assert np.array_equal(hist, got[1])
    print(f"{shape}: worst |error| / bound {worst[0]:.3e} (restatement), {worst[1]:.3e} of twice it (unweighted entry)")


def run_reduce_weighted(lib, d_D, d_mult, Wt, K):
    count, S, _ = d_D.shape
    outs = [guarded_as((count, K), torch.int32, -7), guarded_as((count, K), torch.int32, -7),
            guarded_as((count, S), torch.int32, -7), guarded_as((count, K), torch.float64, np.nan)]
    rc = lib.stemgnn_scenario_reduce_weighted(d_D.data_ptr(), d_mult.data_ptr(), count, S, K, Wt,
                                              *(view.data_ptr() for _, view in outs), None)
    assert rc == 0
    torch.cuda.synchronize()
    return (inside(outs[0][0], (count, K), is_guard), inside(outs[1][0], (count, K), is_guard),
            inside(outs[2][0], (count, S), is_guard), inside(outs[3][0], (count, K), np.isnan))


def same_reduction(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got[:3], want[:3])) and got[3].shape == want[3].shape and \
        np.array_equal(np.isnan(got[3]), np.isnan(want[3])) and \
        np.array_equal(got[3].view(np.int64)[~np.isnan(want[3])], want[3].view(np.int64)[~np.isnan(want[3])])


# a small set; one past a 32-thread..64-thread wave boundary; the real size; the LDS limit and one past it; beyond one wave group
@pytest.mark.parametrize("S,K", [(5, 2), (33, 8), (64, 8), (141, 8), (142, 3), (300, 4)])
def test_reduce_weighted_matches_the_restatement_bit_for_bit(S, K):
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, Wt = 5, 3 * S + 1
    rng = np.random.default_rng(SEED + 17 * S + K)
    x = rng.normal(size=(count, S, 9)).astype(np.float32)
    x[:, S - 1] = x[:, 0]                                                        # a duplicated member: equal z, the lower index wins
    D = R.distances(x).astype(np.float64)

    def weights(zeros):
        """multiplicities that sum to Wt: 0 at `zeros` of the inner members, at least 1 elsewhere"""
        off = rng.choice(np.arange(1, S - 1), size=zeros, replace=False)
        on = np.setdiff1d(np.arange(S), off)
        m = np.zeros(S, np.int32)
        m[on] = 1 + rng.multinomial(Wt - on.size, np.ones(on.size) / on.size)
        return m, off

    mult = np.zeros((count, S), np.int32)
    mult[0], off = weights(max(1, S // 5))                                       # zeros among the weights
    D[0, off, :], D[0, :, off] = np.nan, np.inf                                  # not read: those members have multiplicity 0
    mult[1] = weights(1)[0]
    mult[1, 0] += 1                                                              # absent: a wrong sum
    mult[2, :K - 1] = 1
    mult[2, 0] = Wt - (K - 2)                                                    # K - 1 positive members: K is one too many
    mult[3] = weights(1)[0]
    D[3, 0, S - 1] = np.nan                                                      # a NaN between two positive members IS read
    mult[4] = weights(0)[0]                                                      # every member positive
    assert (mult[[0, 2, 3, 4]].sum(axis=1) == Wt).all() and (mult >= 0).all()
    want = W.forward(D, mult, Wt, K)
    assert (want[0][1:4] == -1).all() and (want[0][[0, 4]] >= 0).all()
    assert (want[1][[0, 4]].sum(axis=1) == Wt).all()
    d_D, d_mult = torch.from_numpy(D).to(DEV), dev_mult(mult)
    got = run_reduce_weighted(lib, d_D, d_mult, Wt, K)
    assert same_reduction(got, want)
    assert same_reduction(run_reduce_weighted(lib, d_D, d_mult, Wt, K), got)
    parts = [run_reduce_weighted(lib, d_D[sl], d_mult[sl], Wt, K) for sl in (slice(0, 2), slice(2, None))]
    assert same_reduction(tuple(np.concatenate([a, b]) for a, b in zip(*parts)), got)
    assert np.array_equal(d_mult.cpu().numpy(), mult) and np.array_equal(d_D.cpu().numpy().view(np.int64), D.view(np.int64))
    # all-ones weights and W = S: the unweighted entry on the same D, bit for bit (its refusals included)
    D1 = R.distances(x).astype(np.float64)
    D1[1, 2, 3] = np.nan
    d_D1 = torch.from_numpy(D1).to(DEV)
    ones = torch.ones(count, S, device=DEV, dtype=torch.int32)
    mine = run_reduce_weighted(lib, d_D1, ones, S, K)
    theirs = [torch.full(s, -7, device=DEV, dtype=t) for s, t in (((count, K), torch.int32), ((count, K), torch.int32),
                                                                  ((count, S), torch.int32), ((count, K), torch.float64))]
    assert lib.stemgnn_scenario_reduce(d_D1.data_ptr(), count, S, K, *(t.data_ptr() for t in theirs), None) == 0
    torch.cuda.synchronize()
    assert same_reduction(mine, tuple(t.cpu().numpy() for t in theirs)) and (mine[0][1] == -1).all()
    assert same_reduction(mine, W.forward(D1, np.ones((count, S), np.int32), S, K))


def test_a_total_beyond_any_replication():
    """W = 65536 (from_weights' default) and 2^24, the largest: no replicated ensemble to compare with, the restatement alone
    (the scores at 65536 only: a histogram of 2^24 + 1 bins per step is no test's size)."""
    from stemgnn_amd import _lib
    lib = _lib.load()
    for Wt in (65536, 2 ** 24):
        rng = np.random.default_rng(SEED + Wt)
        paths, target, mult = W.random_set(rng, 2, 6, 2, 5, 6)
        mult = mult * (Wt // 6)
        for c in range(2):                                                       # the remainder of W / 6 goes to the first member
            mult[c, np.nonzero(mult[c] > 0)[0][0]] += Wt - mult[c].sum()
        d_mult = dev_mult(mult)
        _, d_paths = device_copy(paths, False)
        _, d_y = device_copy(target, False)
        ranks = [W.rank(t, Wt) for t in TAUS]
        assert same_bits(run_bands(lib, d_paths, d_mult, Wt, ranks, False), W.bands(paths, mult, Wt, ranks))
        if Wt == 65536:
            check_scores(run_scores(lib, d_y, d_paths, d_mult, Wt, fair=True), W.scores(target, paths, mult, Wt, fair=True), 2)
        thr = torch.zeros(5, device=DEV, dtype=torch.float64)
        assert np.array_equal(run_events(lib, d_paths, d_mult, Wt, thr, 1, 2), W.events(paths, mult, Wt, np.zeros(5), True, 2))


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def set_numpy(kept):
    return kept.paths.cpu().numpy(), kept.counts.cpu().numpy(), kept.total


def test_a_scenario_set_answers_what_the_ensemble_was_asked():
    from stemgnn_amd import EventSpec, ScenarioSet, ops, reduce_scenarios, trainer
    from stemgnn_amd.math_utils import EnsembleScores
    walk = R.walk_case(WSEED, 5)
    walk[3, 7, 2, 1] = np.nan                                                    # origin 3 is refused by the reduction
    truth = R.walk_case(WSEED + 1, 5)[:, 0].copy()
    d_walk, d_y = torch.from_numpy(walk).to(DEV), torch.from_numpy(truth).to(DEV)
    kept = reduce_scenarios(d_walk, 8)
    assert kept.total == 64 and kept.counts[3].tolist() == [0] * 8
    x, m, total = set_numpy(kept)
    # bands
    got = kept.bands(TAUS)
    assert tsame(got, ops.weighted_bands(kept.paths, kept.counts, 64, TAUS)) and tuple(got.shape) == (5, 4, 12, 16)
    assert same_bits(got.cpu().numpy(), W.bands(x, m, 64, [W.rank(t, 64) for t in TAUS]))
    assert bool(torch.isnan(got[3]).all()) and not bool(torch.isnan(got[[0, 1, 2, 4]]).any())
    out = torch.full_like(got, 5.0)
    assert kept.bands(TAUS, out=out) is out and tsame(out, got)
    ok = [0, 1, 2, 4]
    rep = torch.from_numpy(W.replicate(x[ok], m[ok])).to(DEV)                    # the only route there was: [4, 64, 12, 16]
    want = ops.scenario_bands(rep, TAUS, 0, torch.empty(4, 4, 12, 16, device=DEV))
    assert tsame(got[ok], want)
    # scores: the attributes are the entry's numbers, and those are the restatement's and the replicated ensemble's
    mul, add = torch.linspace(0.5, 2.0, 16), torch.linspace(-1.0, 1.0, 16)
    for kw in (dict(), dict(mul=mul, add=add, fair=True), dict(ignore_nan=True)):
        sc = kept.scores(d_y, **kw)
        o, h = ops.weighted_scores(d_y, kept.paths, kept.counts, 64, **kw)
        o, h = o.cpu().numpy(), h.cpu().numpy()
        assert isinstance(sc, EnsembleScores) and sc.absent == 1 and o[6] == 1.0
        for k, name in enumerate(("crps", "energy", "rmse", "spread", "valid", "valid_rows")):
            assert getattr(sc, name) == o[k] and np.array_equal(getattr(sc, name + "_step"), o[7 + k * 12:7 + (k + 1) * 12])
        assert sc.valid == 4 * 12 * 16 and sc.valid_rows == 4 * 12
        assert np.array_equal(sc.rank_histogram_step, h) and sc.rank_histogram.shape == (65,) and sc.rank_uniformity_dof == 64
        nkw = dict(masked=kw.get("ignore_nan", False), fair=kw.get("fair", False))
        if "mul" in kw:
            nkw.update(mul=mul.double().numpy(), add=add.double().numpy())
        ref = W.scores(truth, x, m, 64, **nkw)
        check_scores((o, h), ref, 12)
        po, ph = ops.ensemble_scores(d_y[ok].contiguous(), rep, kw.get("mul"), kw.get("add"),
                                     ignore_nan=kw.get("ignore_nan", False), fair=kw.get("fair", False))
        check_scores((o, h), dict(out=po.cpu().numpy(), hist=ph.cpu().numpy(), first=ref["first"], second=ref["second"]), 12,
                     scale=2.0, width=6)
    # events, per node and per group
    for spec in (EventSpec(1.0, mul=mul, add=add, min_run=2), EventSpec(2.0, groups=[list(range(16))]),
                 EventSpec(-1.0, above=False, groups=[list(range(8)), list(range(8, 16))], reduce="sum")):
        ev = spec.count(kept)
        assert ev.S == 64 and tsame(ev.counts, kept.events(spec).counts)
        src = kept.paths if spec.groups is None else spec.aggregate(kept.paths)
        direct = ops.weighted_events(src, kept.counts, 64, spec.threshold, spec.above, spec.min_run,
                                     *((spec.mul, spec.add) if spec.groups is None else ()))
        assert tsame(ev.counts, direct) and bool((ev.counts[3] == -1).all())
        assert tsame(ev.counts[ok], spec.count(rep).counts)
        assert bool(torch.isnan(ev.p_any[3]).all()) and bool(torch.isnan(ev.p_step[3]).all())
        assert not bool(torch.isnan(ev.p_any[ok]).any())
        real = spec.realised(d_y)
        a, b = ev.score(real), spec.count(rep).score(spec.realised(d_y[ok]))
        assert np.array_equal(a.reliability, b.reliability) and np.array_equal(a.reliability_step, b.reliability_step)
        assert a.valid == b.valid and (a.brier == b.brier or (np.isnan(a.brier) and np.isnan(b.brier)))
    # score_forecast dispatches on the set
    spec = EventSpec(2.0, groups=[list(range(16))])
    res = trainer.score_forecast(d_y, d_y, paths=kept, events=spec)
    sc, es = kept.scores(d_y), spec.count(kept).score(spec.realised(d_y))
    assert res["crps"] == sc.crps and res["energy_score"] == sc.energy and res["spread"] == sc.spread
    assert np.array_equal(res["rank_histogram"], sc.rank_histogram) and res["rank_histogram"].shape == (65,)
    assert res["event_brier"] == es.brier and np.array_equal(res["event_reliability"], es.reliability)
    # reduce again: the restatement on the kept paths' distances, and the entry itself
    again = kept.reduce(3)
    D = ops.scenario_distances(kept.paths)
    direct = ops.scenario_reduce_weighted(D, kept.counts, 64, 3)
    assert (again.S, again.K, again.total, again.count) == (8, 3, 64, 5)
    assert tsame(again.index, direct[0].long()) and all(tsame(a, b) for a, b in zip((again.counts, again.assign, again.cost),
                                                                                    direct[1:]))
    assert same_reduction((direct[0].cpu().numpy(), direct[1].cpu().numpy(), direct[2].cpu().numpy(), direct[3].cpu().numpy()),
                          W.forward(D.cpu().numpy(), m, 64, 3))
    assert again.counts[ok].sum(dim=1).tolist() == [64] * 4 and again.index[3].tolist() == [-1] * 3
    assert tsame(again.paths[0], kept.paths[0][again.index[0]]) and bool(torch.isnan(again.paths[3]).all())
    assert again.scores(d_y).absent == 1 and tuple(again.bands(TAUS).shape) == (5, 4, 12, 16)
    with pytest.raises(ValueError, match=r"parent\.reduce\(k\)"):
        again.head(2)
    grouped = kept.reduce(3, on=EventSpec(0.0, groups=[list(range(8)), list(range(8, 16))]), scale=0.5)
    assert grouped.counts[ok].sum(dim=1).tolist() == [64] * 4 and not tsame(grouped.cost, again.cost)
    # merge: two halves of the 64 paths, each reduced to 8, then to 8 again
    halves = ScenarioSet.merge([reduce_scenarios(d_walk[:, :32].contiguous(), 8), reduce_scenarios(d_walk[:, 32:].contiguous(), 8)])
    assert (halves.K, halves.S, halves.total) == (16, 64, 64) and halves.counts[ok].sum(dim=1).tolist() == [64] * 4
    two = halves.reduce(8)
    assert (two.K, two.S, two.total) == (8, 16, 64) and two.counts[ok].sum(dim=1).tolist() == [64] * 4
    assert bool((two.counts[3] == 0).all()) and two.scores(d_y).absent == 1      # origin 3's NaN sits in the first half
    first = halves.index[:, :8]
    assert tsame(halves.paths[0, :8], d_walk[0, first[0]]) and tsame(halves.paths[0, 8:], d_walk[0, halves.index[0, 8:]])
    # from_weights on the device: uniform weights over 64 are the full ensemble
    uni = ScenarioSet.from_weights(d_walk[ok], torch.ones(4, 64), total=64)
    assert uni.counts.tolist() == [[1] * 64] * 4
    assert tsame(uni.bands(TAUS), ops.scenario_bands(d_walk[ok].contiguous(), TAUS, 0, torch.empty(4, 4, 12, 16, device=DEV)))


def test_the_walk_case():
    """256 origins of the block-correlated walk, the truth one more draw from the same law; keep = 8.  Asserted: the kernels give
    the restatement's figures within the bound; kept.scores equals the scores of the replicated set; the "any" counts of
    spec.count(kept) are the multiplicities of the members in the event; at keep = S the weighted scores are EnsembleScores of
    the full paths.  The direction of reduced / first 8 / full is printed, not asserted.  The restatement alone, 128 origins
    (tests/test_weighted_abi.py): energy 6.640 / 7.084 / 7.379, crps 1.458 / 1.552 / 1.621, spread 2.551 / 2.187 / 2.571 for
    full 64 / weighted 8 / first 8."""
    from stemgnn_amd import EventSpec, ScenarioSet, ops, reduce_scenarios
    from stemgnn_amd.math_utils import EnsembleScores
    walk, truth = R.walk_case(WSEED), R.walk_case(WSEED + 1)[:, 0].copy()
    d_walk, d_y = torch.from_numpy(walk).to(DEV), torch.from_numpy(truth).to(DEV)
    kept = reduce_scenarios(d_walk, 8)
    x, m, total = set_numpy(kept)
    assert (m.sum(axis=1) == 64).all()
    sc = kept.scores(d_y)
    ref = W.scores(truth, x, m, 64)
    o, h = (t.cpu().numpy() for t in ops.weighted_scores(d_y, kept.paths, kept.counts, 64))
    worst = check_scores((o, h), ref, 12)
    assert sc.crps == o[0] and sc.energy == o[1] and sc.absent == 0
    rep = torch.from_numpy(W.replicate(x, m)).to(DEV)

    def parent(paths, like):
        po, ph = ops.ensemble_scores(d_y, paths)
        return dict(out=po.cpu().numpy(), hist=ph.cpu().numpy(), first=like["first"], second=like["second"])

    check_scores((o, h), parent(rep, ref), 12, scale=2.0, width=6)               # kept.scores equals the replicated set's
    spec = EventSpec(2.0, groups=[list(range(16))])
    ev = spec.count(kept)
    member_in = (spec.aggregate(kept.paths)[..., 0] > 2.0).any(dim=2)            # [count, 8]
    assert torch.equal(ev.first.sum(dim=1)[:, 0].long(), (kept.counts.long() * member_in).sum(dim=1))
    every = reduce_scenarios(d_walk, 64)                                         # keep = S: every path, each once
    assert bool((every.counts == 1).all())
    ref64 = W.scores(truth, walk, np.ones((256, 64), np.int32), 64)
    o64 = tuple(t.cpu().numpy() for t in ops.weighted_scores(d_y, every.paths, every.counts, 64))
    worst = max(worst, check_scores(o64, ref64, 12))
    check_scores(o64, parent(d_walk, ref64), 12, scale=2.0, width=6)
    direct = EnsembleScores(d_y, d_walk)
    first = ScenarioSet.from_weights(d_walk[:, :8].contiguous(), torch.ones(256, 8), total=8).scores(d_y)
    real = spec.realised(d_y)
    for name, s, e in (("full 64", direct, spec.count(d_walk)), ("weighted 8", sc, ev),
                       ("first 8", first, spec.count(d_walk[:, :8].contiguous()))):
        print(f"{name:11s} energy {s.energy:.3f} crps {s.crps:.3f} spread {s.spread:.3f} rmse {s.rmse:.3f} "
              f"brier {e.score(real).brier:.4f} mean p {float(e.p_any.mean()):.3f}")
    print(f"worst |error| / bound against the restatement: {worst:.3e}")


def test_sets_of_a_model_expose_the_methods():
    from stemgnn_amd import LiveForecaster, Model, ops, trainer
    n, w, hz = 9, 12, 3
    torch.manual_seed(SEED)
    model = Model(n, 2, w, 2, horizon=hz, quantiles=(0.1, 0.5, 0.9)).to(DEV).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x, y = torch.randn(5, w, n, generator=g).to(DEV), torch.randn(5, 7, n, generator=g).to(DEV)
    graph = model.latent_graph(x)
    kw = dict(paths=16, seed=11, adjacency=graph)
    _, target, paths = trainer.rolling_scenarios(model, [(x, y)], 7, return_paths=True, **kw)
    _, _, kept = trainer.reduced_scenarios(model, [(x[:2], y[:2]), (x[2:], y[2:])], 7, 4, **kw)
    assert kept.total == 16 and kept.count == 5
    rep = torch.stack([torch.repeat_interleave(kept.paths[c], kept.counts[c].long(), dim=0) for c in range(5)])
    assert tsame(kept.bands((0.1, 0.9)), ops.scenario_bands(rep, (0.1, 0.9), 0, torch.empty(5, 2, 7, n, device=DEV)))
    sc = kept.scores(target)
    assert sc.absent == 0 and sc.valid == 5 * 7 * n and sc.rank_histogram.shape == (17,)
    live = LiveForecaster(model, w, 7, history=4, adjacency=graph)
    live.push(np.random.default_rng(SEED + 3).normal(size=(w + 2, n)))
    live.seed = 21
    one = live.scenario_set(3, paths=8)
    assert one.total == 8 and tuple(one.bands((0.5,)).shape) == (1, 1, 7, n) and int(one.reduce(2).counts.sum()) == 8
