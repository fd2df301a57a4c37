"""numpy restatement of stemgnn_scenario_envelope (include/stemgnn_hip.h): the simultaneous band of sampled
paths.  Every sum is a plain loop over s in float64 (numpy rounds every product and every sum on its own), vectorised over the
origins, steps and columns only, so the bits are the kernel's.  Nothing is imported from the code under test."""
import math

import numpy as np


def rank(m, c):
    """cf_rank of csrc/conformal_select.h: ceil(((m + 1) * c) * (1 - 1e-12)), never below 1"""
    return max(1, int(math.ceil((float(m + 1) * float(c)) * (1.0 - 1e-12))))


def envelope(paths, coverage, target=None, mult=None, total=None, multiplier=None, ignore_nan=False):
    """paths [count,S,H,C] float32; mult int [count,S] with `total`, or None; target [count,H,C] float32 or None; multiplier
    None, [1] or [C] float64 -> dict(moments [count,2,H,C] f64, depth [count,S,C] f64, chosen [count,C] f64, truth [count,C]
    f64 or None, bands [count,2,H,C] f32)"""
    x = np.asarray(paths, np.float32)
    count, S, H, C = x.shape
    if mult is None:
        w, T = np.ones((count, S), np.int64), S
    else:
        w, T = np.asarray(mult).astype(np.int64), int(total)
    present = (w >= 0).all(axis=1) & (w.sum(axis=1) == T)                          # [count]
    live = w > 0                                                                   # [count,S]
    X = x.astype(np.float64)
    wd = w.astype(np.float64)
    nan, inf = np.nan, np.inf
    with np.errstate(all="ignore"):
        acc = np.zeros((count, H, C))
        for s in range(S):
            term = wd[:, s, None, None] * X[:, s]
            acc = np.where(live[:, s, None, None], acc + term, acc)
        m = acc / float(T)
        var = np.zeros((count, H, C))
        for s in range(S):
            d = X[:, s] - m
            sq = d * d
            term = wd[:, s, None, None] * sq
            var = np.where(live[:, s, None, None], var + term, var)
        sd = np.sqrt(var / float(T))
        depth = np.full((count, S, C), nan)
        for s in range(S):
            r = np.abs(X[:, s] - m) / sd
            r = np.where(sd == 0.0, 0.0, r)
            depth[:, s] = np.where(live[:, s, None], r.max(axis=1), nan)
        bad = (~np.isfinite(x) & live[:, :, None, None]).any(axis=(1, 2)) | ~present[:, None]   # [count,C]
        k = rank(T, coverage)
        chosen = np.full((count, C), inf)
        if k <= T:
            for c in range(count):
                dc = depth[c]                                                      # [S,C]
                cnt = ((dc[None, :, :] <= dc[:, None, :]) * w[c][None, :, None]).sum(axis=1)   # [S,C]: weight of d_j <= d_s
                chosen[c] = np.where((cnt >= k) & live[c][:, None], dc, inf).min(axis=0)
        q = chosen if multiplier is None else np.broadcast_to(np.asarray(multiplier, np.float64).reshape(1, -1), (count, C))
        qb = q[:, None, :]
        r = qb * sd
        lo, hi = m - r, m + r
        lo, hi = np.where(qb == inf, -inf, lo), np.where(qb == inf, inf, hi)
        truth = None
        if target is not None:
            y = np.asarray(target, np.float32).astype(np.float64)
            r = np.abs(y - m) / sd
            r = np.where(sd == 0.0, np.where(y == m, 0.0, inf), r)
            miss = np.isnan(y)
            tr = np.where(miss, 0.0, r).max(axis=1)
            gone = miss.all(axis=1) | (miss.any(axis=1) & (not ignore_nan))
            truth = np.where(gone | bad, nan, tr)
        gone = bad[:, None, :]
        moments = np.stack([np.where(gone, nan, m), np.where(gone, nan, sd)], axis=1)
        bands = np.stack([np.where(gone, nan, lo), np.where(gone, nan, hi)], axis=1).astype(np.float32)
        depth = np.where(bad[:, None, :], nan, depth)
        chosen = np.where(bad, nan, chosen)
    return dict(moments=moments, depth=depth, chosen=chosen, truth=truth, bands=bands)


def calibrated_multiplier(truth, coverage):
    """the split-conformal multiplier of the depths that are not NaN: the rank(m, coverage)-th smallest, +inf beyond m"""
    d = np.sort(np.asarray(truth, np.float64).ravel())
    d = d[~np.isnan(d)]
    k = rank(d.size, coverage)
    return float("inf") if k > d.size else float(d[k - 1])


def joint(y, lo, hi):
    """share of (origin, column) pairs with y [count,H,C] inside lo .. hi at every step"""
    return float(((y >= lo) & (y <= hi)).all(axis=1).mean())


def random_walk_case(seed, count=4096, S=32, H=8):
    """the statistical case: paths [count,S,H,1] and the truth [count,H,1], cumulative sums of standard normals (exchangeable)"""
    rng = np.random.default_rng(seed)
    walks = rng.standard_normal((count, S + 1, H, 1)).cumsum(axis=2).astype(np.float32)
    return np.ascontiguousarray(walks[:, :S]), np.ascontiguousarray(walks[:, S])


def statistical_figures(paths, y, coverage=0.9):
    """the four figures of the statistical case by the restatement alone, and the calibrated multiplier:
    (pointwise joint coverage by ranks 2 and S - 1, the ensemble multiplier's joint coverage, the calibrated multiplier's joint
    coverage on the second half, its lowest per-step coverage there, the multiplier)"""
    count, S = paths.shape[:2]
    half = count // 2
    ordered = np.sort(paths, axis=1)
    pointwise = joint(y, ordered[:, 1], ordered[:, S - 2])
    own = envelope(paths, coverage, target=y)
    ensemble = float((own["truth"] <= own["chosen"]).mean())
    q = calibrated_multiplier(own["truth"][:half], coverage)
    cal = envelope(paths[half:], coverage, target=y[half:], multiplier=[q])
    calibrated = float((cal["truth"] <= q).mean())
    lo, hi = cal["bands"][:, 0], cal["bands"][:, 1]
    per_step = float(((y[half:] >= lo) & (y[half:] <= hi)).mean(axis=(0, 2)).min())
    return pointwise, ensemble, calibrated, per_step, q
