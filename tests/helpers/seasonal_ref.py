"""The definition of seasonal (per time-of-day bucket) conformal calibration, restated in numpy: the bucket formula, the
per-bucket fit (rank, fp32 score, k-th smallest), the thin-bucket fallback, and the apply.  Nothing here touches the code
under test."""
import math

import numpy as np

INF = np.float32(np.inf)
GROUPINGS = ((True, False), (False, False), (True, True), (False, True))          # (per_step, per_node)
LEVELS = {2: (0.1, 0.9), 3: (0.1, 0.5, 0.9), 5: (0.05, 0.25, 0.5, 0.75, 0.95)}


def bucket(t, period, K, phase):
    """Python's % is the floor mod and // on non-negative ints the integer division of the definition"""
    return ((int(t) + phase) % period) * K // period


def buckets_of(origins, H, season):
    """[count, H] the bucket of step h of row i: bucket(o_i + h)"""
    period, K, phase = season
    return np.array([[bucket(int(o) + h, period, K, phase) for h in range(H)] for o in origins], np.int64).reshape(len(origins), H)


def origins_of(origin, count):
    return np.arange(count, dtype=np.int64) + int(origin) if np.isscalar(origin) else np.asarray(origin, np.int64)


def pairs_of(quantiles):
    Q = len(quantiles)
    pairs = tuple((i, Q - 1 - i) for i in range(Q // 2))
    return pairs, [float(quantiles[hi]) - float(quantiles[lo]) for lo, hi in pairs]


def rank(m, c):
    """the definition: two fp64 multiplies and a ceil"""
    t = (m + 1) * c
    return math.ceil(t * (1 - 1e-12))


def min_count(c):
    """m_min(c): the smallest m with rank(m, c) <= m"""
    m = 0
    while max(1, rank(m, c)) > m:
        m += 1
    return m


def scores_np(y, f, lo, hi):
    """fp32: two rounded subtractions and a max; a NaN score counts as +inf"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.maximum(f[:, lo] - y, y - f[:, hi])               # np.maximum propagates NaN
    assert s.dtype == np.float32
    return np.where(np.isnan(s), INF, s)


def fit_np(y, f, origin, pairs, coverage, season, per_step, per_node, masked):
    """(offsets fp32, counts int64) [K, P, Hg, Ng]: per bucket, pair and group the k-th smallest score, +inf when k > m"""
    C, H, N = y.shape
    K = season[1]
    Hg, Ng = (H if per_step else 1), (N if per_node else 1)
    offsets = np.empty((K, len(pairs), Hg, Ng), np.float32)
    counts = np.empty((K, len(pairs), Hg, Ng), np.int64)
    keep = ~np.isnan(y) if masked else np.ones(y.shape, bool)
    bk = buckets_of(origins_of(origin, C), H, season)           # [C, H]
    for s in range(K):
        mine = keep & (bk == s)[:, :, None]
        for p, (lo, hi) in enumerate(pairs):
            sc = scores_np(y, f, lo, hi)
            for hg in range(Hg):
                hs = slice(hg, hg + 1) if per_step else slice(None)
                for ng in range(Ng):
                    ns = slice(ng, ng + 1) if per_node else slice(None)
                    v = np.sort(sc[:, hs, ns][mine[:, hs, ns]])
                    k = max(1, rank(v.size, coverage[p]))
                    counts[s, p, hg, ng] = v.size
                    offsets[s, p, hg, ng] = INF if k > v.size else v[k - 1]
    return offsets, counts


def pooled_fit_np(y, f, pairs, coverage, per_step, per_node, masked):
    """the unseasoned fit: one bucket"""
    off, cnt = fit_np(y, f, 0, pairs, coverage, (1, 1, 0), per_step, per_node, masked)
    return off[0], cnt[0]


def fallback_np(offsets, counts, pooled, coverage, min_scores):
    """fallback="pooled": every entry whose count is below max(min_scores, m_min(c_p)) takes the pooled entry"""
    need = np.array([max(int(min_scores), min_count(c)) for c in coverage], np.int64).reshape(1, -1, 1, 1)
    return np.where(counts < need, pooled[None], offsets).astype(np.float32)


def apply_np(f, offsets, origin, pairs, season):
    """out[i, lo_p, h, n] = f - offsets[bucket(o_i + h), p, ..], hi_p: f + ...; one fp32 operation each"""
    C, Q, H, N = f.shape
    bk = buckets_of(origins_of(origin, C), H, season)
    out = f.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p, (lo, hi) in enumerate(pairs):
            off = np.broadcast_to(offsets[:, p], (offsets.shape[0], offsets.shape[2], offsets.shape[3]))
            Hg = off.shape[1]
            sel = off[bk, np.arange(H)[None, :] if Hg > 1 else 0]          # [C, H, Ng]
            out[:, lo] = f[:, lo] - sel
            out[:, hi] = f[:, hi] + sel
    assert out.dtype == np.float32
    return out


def random_case(count, H, N, Q, seed, nan_share=0.0):
    rng = np.random.default_rng(seed)
    y = rng.normal(size=(count, H, N)).astype(np.float32) * (1 + np.arange(H, dtype=np.float32))[None, :, None]
    centre = (0.5 * y + rng.normal(size=y.shape).astype(np.float32) * 0.5)[:, None]
    half = np.sort(np.abs(rng.normal(size=(count, Q, H, N))).astype(np.float32), axis=1)
    f = (centre + half - half.mean(axis=1, keepdims=True)).astype(np.float32)      # Q rows, non-decreasing in q
    if nan_share:
        y[rng.random(y.shape) < nan_share] = np.nan
        y[:, H - 1, N // 2] = np.nan                              # one (h, n) column with no valid target at all
    return y, f


def scattered_origins(count, rng):
    """a shuffled range with repeats and gaps, some of it negative"""
    o = rng.permutation(np.arange(count, dtype=np.int64) * 2 - count // 3)
    o[rng.random(count) < 0.2] = o[0]
    return o


# ---- the coverage experiment of the issue: noise scale by bucket ------------------------------------------------------------
COVERAGE_SEASON = (8, 4, 3)
SIGMA = (0.5, 1.0, 2.0, 4.0)


def coverage_case(count, origin0, H, N, seed):
    """forecast rows fixed at -1 / 0 / +1, target sigma[bucket(t)] * normal"""
    rng = np.random.default_rng(seed)
    bk = buckets_of(origins_of(origin0, count), H, COVERAGE_SEASON)
    y = (np.asarray(SIGMA)[bk][:, :, None] * rng.normal(size=(count, H, N))).astype(np.float32)
    f = np.empty((count, 3, H, N), np.float32)
    f[:, 0], f[:, 1], f[:, 2] = -1.0, 0.0, 1.0
    return y, f, bk


def coverage_by_bucket_step(y, banded, bk, K):
    """(coverage [K, H], group sizes [K, H]) of lo <= y <= hi per (bucket, step), nodes pooled"""
    inside = (banded[:, 0] <= y) & (y <= banded[:, 2])
    H = y.shape[1]
    cov, size = np.full((K, H), np.nan), np.zeros((K, H), np.int64)
    for s in range(K):
        for h in range(H):
            rows = bk[:, h] == s
            size[s, h] = rows.sum() * y.shape[2]
            if size[s, h]:
                cov[s, h] = inside[rows, h].mean()
    return cov, size
