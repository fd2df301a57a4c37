"""GPU: seasonal conformal calibration (csrc/seasonal.hip, math_utils.SeasonalConformalCalibrator) against the numpy restatement
of its definition in tests/helpers/seasonal_ref.py.  An offset is a k-th smallest fp32 value and an applied row one fp32
operation, so every comparison is equality (np.array_equal on numbers for offsets: inf == inf, -0 == +0; bit patterns for
applied rows, a NaN that the operation itself makes -- inf - inf -- only has to be a NaN) and the counts are equal -- no tolerance anywhere except the binomial margin of the coverage test, which is
computed from the group sizes."""
import math

import numpy as np
import pytest
import torch

from tests.helpers import seasonal_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 1, 1), (5, 2, 3), (257, 3, 7), (1000, 1, 33), (64, 3, 65), (2049, 2, 5))
SEASONS = ((1, 1, 0), (12, 4, 5), (7, 7, 0), (288, 24, 100))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_values(a, b):
    """NaN at the same places (the payload of a NaN that an operation makes is the machine's), equal bits everywhere else"""
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def fit_gpu(y, f, origin, pairs, coverage, season, per_step, per_node, masked):
    from stemgnn_amd import ops
    origin = dev(origin) if isinstance(origin, np.ndarray) else origin
    off, cnt = ops.seasonal_fit(dev(y), dev(f), origin, pairs, coverage, season, per_step, per_node, ignore_nan=masked)
    assert off.dtype == torch.float32 and cnt.dtype == torch.int64
    return off.cpu().numpy(), cnt.cpu().numpy()


def check_fit(y, f, origin, pairs, coverage, season, per_step, per_node, masked, what=""):
    want_off, want_cnt = R.fit_np(y, f, origin, pairs, coverage, season, per_step, per_node, masked)
    off, cnt = fit_gpu(y, f, origin, pairs, coverage, season, per_step, per_node, masked)
    tag = (what, y.shape, season, per_step, per_node, masked)
    assert off.shape == want_off.shape and cnt.shape == want_cnt.shape, tag
    assert np.array_equal(cnt, want_cnt), tag
    assert not np.isnan(off).any(), tag
    assert np.array_equal(off, want_off), (tag, off.ravel()[:8], want_off.ravel()[:8])
    return off, cnt


# ---- 1. the fit equals numpy ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", (3, 5))
@pytest.mark.parametrize("season", SEASONS, ids=str)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fit_equals_numpy(shape, season, Q):
    count, H, N = shape
    pairs, coverage = R.pairs_of(R.LEVELS[Q])
    rng = np.random.default_rng(count + 13 * Q + season[0])
    forms = (-5, 3 * season[0] + 2, R.scattered_origins(count, rng))
    empty = 0
    for masked in (False, True):
        y, f = R.random_case(count, H, N, Q, seed=count + 7 * Q, nan_share=0.1 if masked else 0.0)
        for g, (per_step, per_node) in enumerate(R.GROUPINGS):
            # every grouping with the tensor form and one of the two origin0 forms; all three forms on the first grouping
            for origin in (forms if g == 0 else (forms[g % 2], forms[2])):
                off, cnt = check_fit(y, f, origin, pairs, coverage, season, per_step, per_node, masked, f"Q{Q}")
                empty += int((cnt == 0).sum())
                assert np.isposinf(off[cnt == 0]).all()
    if season[1] == 24 and count <= 5:
        assert empty > 0                                          # buckets nothing falls into: +inf, count 0


@pytest.mark.parametrize("fallback", ("pooled", "inf"))
@pytest.mark.parametrize("min_scores", (0, 10))
def test_calibrator_fallback_equals_numpy(fallback, min_scores):
    from stemgnn_amd.math_utils import SeasonalConformalCalibrator
    count, H, N, Q = 257, 3, 7, 5
    taus = R.LEVELS[Q]
    pairs, coverage = R.pairs_of(taus)
    season = (288, 24, 100)                                       # t = -5 .. 253: u = 95 .. 287, 0 .. 65 -- bucket 6 is empty
    y, f = R.random_case(count, H, N, Q, seed=99, nan_share=0.1)
    for per_step, per_node in R.GROUPINGS:
        cal = SeasonalConformalCalibrator(taus, *season, per_step=per_step, per_node=per_node, min_scores=min_scores,
                                          fallback=fallback).fit(dev(y), dev(f), -5, ignore_nan=True)
        raw, cnt = R.fit_np(y, f, -5, pairs, coverage, season, per_step, per_node, True)
        assert np.array_equal(cal.counts.cpu().numpy(), cnt)
        assert np.array_equal(cal.offsets_seasonal.cpu().numpy(), raw)
        if fallback == "inf":
            assert cal.pooled_offsets is None and np.array_equal(cal.offsets.cpu().numpy(), raw)
            continue
        pooled, _ = R.pooled_fit_np(y, f, pairs, coverage, per_step, per_node, True)
        want = R.fallback_np(raw, cnt, pooled, coverage, min_scores)
        assert np.array_equal(cal.pooled_offsets.cpu().numpy(), pooled)
        assert np.array_equal(cal.offsets.cpu().numpy(), want)
        thin = cnt < np.array(cal.thresholds()).reshape(1, -1, 1, 1)
        assert thin.any() and not thin.all()
        if not (per_step and per_node):                           # (the all-NaN column has no pooled score either)
            assert np.isfinite(cal.offsets.cpu().numpy()).all() and np.isposinf(raw).any()


# ---- 2. one bucket is ConformalCalibrator -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((257, 3, 7), (64, 3, 8)), ids=lambda s: "x".join(map(str, s)))
def test_one_bucket_equals_the_unseasoned_calibrator(shape):
    from stemgnn_amd.math_utils import ConformalCalibrator, SeasonalConformalCalibrator
    count, H, N = shape
    taus = R.LEVELS[5]
    rng = np.random.default_rng(5)
    for masked in (False, True):
        y, f = R.random_case(count, H, N, 5, seed=count, nan_share=0.1 if masked else 0.0)
        for per_step, per_node in R.GROUPINGS:
            base = ConformalCalibrator(taus, per_step, per_node).fit(dev(y), dev(f), ignore_nan=masked)
            want = base.apply(dev(f))
            for origin in (0, -17, dev(R.scattered_origins(count, rng))):
                for fallback in ("pooled", "inf"):
                    cal = SeasonalConformalCalibrator(taus, 1, 1, 0, per_step, per_node, fallback=fallback)
                    cal.fit(dev(y), dev(f), origin, ignore_nan=masked)
                    assert tuple(cal.offsets.shape) == (1,) + tuple(base.offsets.shape)
                    assert torch.equal(cal.offsets[0].view(torch.int32), base.offsets.view(torch.int32))
                    assert torch.equal(cal.counts[0], base.counts)
                    assert torch.equal(cal.apply(dev(f), origin).view(torch.int32), want.view(torch.int32))


# ---- 3. / 4. permutations, scratch, repeats -----------------------------------------------------------------------------------
def test_permuting_the_rows_with_their_origins_keeps_the_bits():
    count, H, N, Q = 1000, 3, 7, 3
    pairs, coverage = R.pairs_of(R.LEVELS[Q])
    rng = np.random.default_rng(3)
    y, f = R.random_case(count, H, N, Q, seed=11, nan_share=0.1)
    origins = R.scattered_origins(count, rng)
    perm = rng.permutation(count)
    for per_step, per_node in R.GROUPINGS:
        a = fit_gpu(y, f, origins, pairs, coverage, (12, 4, 5), per_step, per_node, True)
        b = fit_gpu(y[perm], f[perm], origins[perm], pairs, coverage, (12, 4, 5), per_step, per_node, True)
        assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
        # consecutive origins, handed over as a shuffled tensor
        c = fit_gpu(y, f, 7, pairs, coverage, (12, 4, 5), per_step, per_node, True)
        d = fit_gpu(y[perm], f[perm], (np.arange(count, dtype=np.int64) + 7)[perm], pairs, coverage, (12, 4, 5), per_step,
                    per_node, True)
        assert np.array_equal(bits(c[0]), bits(d[0])) and np.array_equal(c[1], d[1])


def test_the_result_does_not_depend_on_what_the_scratch_held():
    from stemgnn_amd import _lib
    lib = _lib.load()
    count, H, N, Q = 257, 3, 7, 3
    P, season = 1, (12, 4, 5)
    y, f = R.random_case(count, H, N, Q, seed=21)
    ty, tf = dev(y), dev(f)
    lo, hi, cov = (ctypes_ints(0)), (ctypes_ints(2)), (_lib.c_double * 1)(0.8)
    stream = torch.cuda.current_stream().cuda_stream
    for per_step, per_node in R.GROUPINGS:
        want_off, want_cnt = R.fit_np(y, f, -5, ((0, 2),), [0.8], season, per_step, per_node, False)
        nbytes = lib.stemgnn_seasonal_scratch_bytes(count, H, N, P, season[1], int(per_step), int(per_node))
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        results = []
        for fill in (0x00, 0xFF, None, None):                     # None: whatever the previous fit left (no re-zeroing)
            if fill is not None:
                scratch.fill_(fill)
            off = torch.full(want_off.shape, float("nan"), device=DEV)
            cnt = torch.full(want_cnt.shape, -1, dtype=torch.int64, device=DEV)
            rc = lib.stemgnn_seasonal_fit(ty.data_ptr(), tf.data_ptr(), None, -5, count, Q, H, N, P, lo, hi, cov, int(per_step),
                                          int(per_node), 0, *season, scratch.data_ptr(), off.data_ptr(), cnt.data_ptr(), stream)
            assert rc == 0
            results.append((off.cpu().numpy(), cnt.cpu().numpy()))
        for off, cnt in results:
            assert np.array_equal(bits(off), bits(want_off)) and np.array_equal(cnt, want_cnt)


def ctypes_ints(*v):
    import ctypes
    return (ctypes.c_int * len(v))(*v)


# ---- 5. apply -----------------------------------------------------------------------------------------------------------------
def apply_cases(N):
    rng = np.random.default_rng(N)
    count, Q, H = 37, 5, 3
    f = rng.normal(size=(count, Q, H, N)).astype(np.float32)
    f[3, 0, 1, 0], f[4, 4, 2, N - 1], f[5, 1, 0, 0], f[6, 2, 1, 0] = np.inf, -np.inf, np.nan, np.nan
    f[7, :, 0, 0] = (0.0, -0.0, 0.0, -0.0, 1.0)
    return f


@pytest.mark.parametrize("N", (8, 7, 228, 1), ids=lambda n: f"N{n}")
def test_apply_equals_numpy(N):
    from stemgnn_amd import ops
    f = apply_cases(N)
    count, Q, H, _ = f.shape
    pairs, _ = R.pairs_of(R.LEVELS[Q])
    rng = np.random.default_rng(17 + N)
    season = (12, 4, 5)
    for per_step, per_node in R.GROUPINGS:
        off = rng.normal(size=(4, 2, H if per_step else 1, N if per_node else 1)).astype(np.float32)
        off.reshape(-1)[:3] = (np.inf, -np.inf, np.nan)
        for origin in (-5, R.scattered_origins(count, rng)):
            want = R.apply_np(f, off, origin, pairs, season)
            o = dev(origin) if isinstance(origin, np.ndarray) else origin
            got = ops.seasonal_apply(dev(f), dev(off), o, pairs, season, per_step, per_node)
            assert same_values(got.cpu().numpy(), want), (N, per_step, per_node)
            # in place
            buf = dev(f)
            assert ops.seasonal_apply(buf, dev(off), o, pairs, season, per_step, per_node, out=buf) is buf
            assert same_values(buf.cpu().numpy(), want)
            # a view one float off the allocation's alignment: the scalar path
            store = torch.empty(f.size + 1, device=DEV)
            view = store[1:].view(f.shape)
            view.copy_(dev(f))
            assert view.data_ptr() % 16 == 4
            out = torch.empty(f.size + 1, device=DEV)[1:].view(f.shape)
            ops.seasonal_apply(view, dev(off), o, pairs, season, per_step, per_node, out=out)
            assert same_values(out.cpu().numpy(), want)
            # rearrange: torch.sort(dim=1, stable=True), then the unarranged apply; also in place
            ordered = torch.sort(dev(f), dim=1, stable=True).values
            want_r = ops.seasonal_apply(ordered, dev(off), o, pairs, season, per_step, per_node)
            got_r = ops.seasonal_apply(dev(f), dev(off), o, pairs, season, per_step, per_node, rearrange=True)
            assert torch.equal(got_r.view(torch.int32), want_r.view(torch.int32))
            assert same_values(want_r.cpu().numpy(), R.apply_np(ordered.cpu().numpy(), off, origin, pairs, season))
            buf = dev(f)
            ops.seasonal_apply(buf, dev(off), o, pairs, season, per_step, per_node, rearrange=True, out=buf)
            assert torch.equal(buf.view(torch.int32), want_r.view(torch.int32))
            ops.seasonal_apply(view, dev(off), o, pairs, season, per_step, per_node, rearrange=True, out=out)
            assert torch.equal(out.contiguous().view(torch.int32), want_r.view(torch.int32))


def test_apply_rearranged_with_many_levels():
    """Q = 20 > 16: the rearranged apply takes its scalar path whatever N is"""
    from stemgnn_amd import ops
    rng = np.random.default_rng(20)
    f = rng.normal(size=(9, 20, 2, 8)).astype(np.float32)
    pairs = tuple((i, 19 - i) for i in range(10))
    off = rng.normal(size=(3, 10, 2, 1)).astype(np.float32)
    ordered = torch.sort(dev(f), dim=1, stable=True).values
    want = R.apply_np(ordered.cpu().numpy(), off, 4, pairs, (7, 3, 2))
    got = ops.seasonal_apply(dev(f), dev(off), 4, pairs, (7, 3, 2), True, False, rearrange=True)
    assert same_values(got.cpu().numpy(), want)


# ---- 6. chosen scores, inside one bucket ----------------------------------------------------------------------------------------
def key_sets(m, rng):
    """with f_lo = -inf and f_hi = 0 the score is the target itself (y - 0), so these ARE the scores"""
    return {
        "low_byte": (1.0 + np.arange(m, dtype=np.float64) % 256 * 2.0 ** -23).astype(np.float32)[rng.permutation(m)],
        "top24": (1.0 + np.arange(m, dtype=np.float64) * 2.0 ** -23).astype(np.float32)[rng.permutation(m)],
        "zeros": rng.choice(np.array([0.0, -0.0], np.float32), m),
        "zeros_mixed": rng.choice(np.array([0.0, -0.0, -1.0, 1.0], np.float32), m),
        "inf": rng.choice(np.array([np.inf, -np.inf, 0.5, -0.5], np.float32), m),
        "posinf": rng.choice(np.array([np.inf, 0.5, -0.5], np.float32), m),
    }


@pytest.mark.parametrize("m", (1, 2, 255, 257, 1030))
def test_fit_on_chosen_scores_within_one_bucket(m):
    """period 4, K 2: rows with origin 0, 1 (mod 4) are bucket 0 -- the chosen keys -- the others bucket 1, filled with noise
    that must not leak in.  Three pairs select rank 1, rank m and rank m + 1 (= +inf) of bucket 0's m scores."""
    rng = np.random.default_rng(m)
    sets = key_sets(m, rng)
    pairs = ((0, 5), (1, 4), (2, 3))
    coverage = [1e-6, (m - 0.5) / (m + 1), 1 - 1e-9]
    assert [R.rank(m, c) for c in coverage] == [1, m, m + 1]
    names = list(sets)
    S = len(names)
    count = 2 * m
    origins = np.empty(count, np.int64)
    origins[0::2] = 4 * np.arange(m) + (np.arange(m) % 2)        # bucket 0
    origins[1::2] = 4 * np.arange(m) + 2 + (np.arange(m) % 2)    # bucket 1
    origins -= 4 * (m // 2)                                       # half of them negative
    order = rng.permutation(count)
    y = np.empty((count, 1, S), np.float32)
    y[0::2, 0] = np.stack([sets[k] for k in names], axis=1)
    y[1::2, 0] = rng.normal(size=(m, S)).astype(np.float32) * 100
    f = np.zeros((count, 6, 1, S), np.float32)
    f[:, :3] = -np.inf
    y, f, origins = y[order], f[order], origins[order]
    for per_step in (False, True):
        off, cnt = check_fit(y, f, origins, pairs, coverage, (4, 2, 0), per_step, True, False, "sets as nodes")
        assert (cnt == m).all() and np.isposinf(off[:, 2]).all()
        for j, k in enumerate(names):
            # (a target of -inf under f_lo = -inf scores -inf - -inf = NaN, which counts as +inf)
            v = np.sort(np.where(np.isneginf(sets[k]), np.float32(np.inf), np.where(sets[k] == 0, np.float32(0), sets[k])))
            assert off[0, 0, 0, j] == v[0] and off[0, 1, 0, j] == v[m - 1], k
    # pooled over the nodes (the streaming form): one set at a time
    for k in names:
        yk = y[:, :, names.index(k):names.index(k) + 1].copy()
        check_fit(yk, f[:, :, :, :1], origins, pairs, coverage, (4, 2, 0), True, False, False, k)


# ---- 7. coverage: what the feature is for -----------------------------------------------------------------------------------------
def test_coverage_per_bucket_where_a_pooled_calibrator_fails():
    from stemgnn_amd.math_utils import ConformalCalibrator, SeasonalConformalCalibrator
    taus, season, K = (0.1, 0.5, 0.9), R.COVERAGE_SEASON, R.COVERAGE_SEASON[1]
    H, N, c = 3, 7, 0.9 - 0.1
    y_cal, f_cal, bk_cal = R.coverage_case(1600, 11, H, N, seed=2026)
    y_new, f_new, bk_new = R.coverage_case(1600, 5, H, N, seed=2027)
    seasonal = SeasonalConformalCalibrator(taus, *season, per_step=True, per_node=False).fit(dev(y_cal), dev(f_cal), 11)
    pooled = ConformalCalibrator(taus, per_step=True, per_node=False).fit(dev(y_cal), dev(f_cal))
    # the calibrators are the numpy ones
    pairs, coverage = R.pairs_of(taus)
    want, _ = R.fit_np(y_cal, f_cal, 11, pairs, coverage, season, True, False, False)
    assert np.array_equal(seasonal.offsets.cpu().numpy(), want) and np.isfinite(want).all()
    _, m_cal = R.coverage_by_bucket_step(y_cal, f_cal, bk_cal, K)
    cov_s, m_new = R.coverage_by_bucket_step(y_new, seasonal.apply(dev(f_new), 5).cpu().numpy(), bk_new, K)
    cov_p, _ = R.coverage_by_bucket_step(y_new, pooled.apply(dev(f_new)).cpu().numpy(), bk_new, K)
    margin = 5 * np.sqrt(c * (1 - c) * (1.0 / m_cal + 1.0 / m_new))
    print("seasonal coverage", cov_s.round(4).tolist(), "margin", margin.round(4).tolist(), "pooled", cov_p.round(4).tolist())
    assert (m_cal > 0).all() and (m_new > 0).all() and (margin < 0.06).all()
    assert (np.abs(cov_s - c) <= margin).all(), (cov_s, margin)
    assert (cov_p[0] >= 0.95).all() and (cov_p[3] <= 0.6).all(), cov_p
    assert math.isclose(c, 0.8)
