"""The definition of the scenario-event entries (include/stemgnn_hip.h: stemgnn_scenario_aggregate / stemgnn_scenario_events) and
of math_utils.EventScores, restated in numpy: plain loops in float64.  Nothing here touches the code under test."""
import numpy as np


def denorm(x, mul=None, add=None):
    """float32 [..., n] -> float64, the product and the sum rounded separately (numpy does not fuse them)"""
    v = np.asarray(x, np.float32).astype(np.float64)
    if mul is None:
        return v
    with np.errstate(all="ignore"):
        return v * np.asarray(mul, np.float64) + np.asarray(add, np.float64)


def aggregate(x, weights, mul=None, add=None):
    """x float32 [rows, N], weights float64 [R, N] -> (ref float64 [rows, R], mag float64 [rows, R] = sum_n |w_n v_n| over the
    same nodes: the yardstick of the re-association bound).  A node of weight 0 is not part of either sum."""
    v = denorm(x, mul, add)
    w = np.asarray(weights, np.float64)
    rows, R = v.shape[0], w.shape[0]
    ref, mag = np.zeros((rows, R)), np.zeros((rows, R))
    with np.errstate(all="ignore"):
        for r in range(R):
            on = np.nonzero(w[r] != 0)[0]
            terms = v[:, on] * w[r, on]
            ref[:, r] = terms.sum(axis=1)
            mag[:, r] = np.abs(terms).sum(axis=1)
    return ref, mag


def events(paths, thr, above, min_run, mul=None, add=None):
    """paths float32 [count, S, H, M], thr float64 [M] -> counts int32 [count, 2 H + 1, M]"""
    v = denorm(paths, mul, add)
    count, S, H, M = v.shape
    thr = np.broadcast_to(np.asarray(thr, np.float64), (M,))
    counts = np.zeros((count, 2 * H + 1, M), np.int32)
    with np.errstate(invalid="ignore"):
        e = (v > thr) if above else (v < thr)                   # [count, S, H, M]; a NaN on either side is False
    for c in range(count):
        for m in range(M):
            for s in range(S):
                crossed, cur, best = False, 0, 0
                for h in range(H):
                    if e[c, s, h, m]:
                        counts[c, h, m] += 1
                        if not crossed:
                            counts[c, H + h, m] += 1
                            crossed = True
                        cur += 1
                        best = max(best, cur)
                    else:
                        cur = 0
                if best >= min_run:
                    counts[c, 2 * H, m] += 1
    return counts


def events_fast(paths, thr, above, min_run, mul=None, add=None):
    """events() with the loops over (origin, path, column) vectorised; the walk over h is kept (the tests hold the two against
    each other on small shapes)"""
    v = denorm(paths, mul, add)
    count, S, H, M = v.shape
    thr = np.broadcast_to(np.asarray(thr, np.float64), (M,))
    with np.errstate(invalid="ignore"):
        e = (v > thr) if above else (v < thr)
    counts = np.zeros((count, 2 * H + 1, M), np.int32)
    crossed = np.zeros((count, S, M), bool)
    cur = np.zeros((count, S, M), np.int64)
    best = np.zeros((count, S, M), np.int64)
    for h in range(H):
        eh = e[:, :, h]
        counts[:, h] = eh.sum(axis=1)
        counts[:, H + h] = (eh & ~crossed).sum(axis=1)
        crossed |= eh
        cur = np.where(eh, cur + 1, 0)
        best = np.maximum(best, cur)
    counts[:, 2 * H] = (best >= min_run).sum(axis=1)
    return counts


def reliability(counts, S, real, missing=None):
    """counts [count, 2 H + 1, M] of S paths, real the same of the one path that happened, missing bool [count, H, M] or None
    -> int64 [2 + H, M, S + 1, 2] of (n_j, o_j) for any | run | step 0 .. H - 1"""
    count, K, M = counts.shape
    H = K // 2
    table = np.zeros((2 + H, M, S + 1, 2), np.int64)
    for c in range(count):
        for m in range(M):
            gone = missing is not None and bool(missing[c, :, m].any())
            kinds = [(counts[c, H:2 * H, m].sum(), real[c, H:2 * H, m].sum(), gone), (counts[c, 2 * H, m], real[c, 2 * H, m], gone)]
            kinds += [(counts[c, h, m], real[c, h, m], missing is not None and bool(missing[c, h, m])) for h in range(H)]
            for k, (j, o, skip) in enumerate(kinds):
                if not skip:
                    table[k, m, int(j), 0] += 1
                    table[k, m, int(j), 1] += int(o)
    return table


def brier(table, S):
    """(brier, base_rate, skill) of one table [S + 1, 2] of (n_j, o_j), python floats"""
    V = float(table[:, 0].sum())
    if V == 0:
        return float("nan"), float("nan"), float("nan")
    b = sum(float(o) * (1.0 - j / S) ** 2 + float(n - o) * (j / S) ** 2 for j, (n, o) in enumerate(table)) / V
    base = float(table[:, 1].sum()) / V
    skill = 1.0 - b / (base * (1.0 - base)) if 0.0 < base < 1.0 else float("nan")
    return b, base, skill


def order_statistic(x, rank, axis):
    """the rank-th smallest (1-based) along axis"""
    return np.take(np.sort(x, axis=axis), rank - 1, axis=axis)


def scenario_rank(tau, S):
    """stemgnn_scenario_rank: min(S, max(1, ceil(tau * S * (1 - 1e-12))))"""
    return int(min(S, max(1, np.ceil(tau * S * (1.0 - 1e-12)))))


def statistical_figures(y, ensembles, threshold=0.8, levels=(0.1, 0.9)):
    """The issue's statistical case by numpy alone: y float32 [count, 1, N], ensembles {name: float32 [count, S, 1, N]} ->
    {name: (coverage of the truth by the band between the two ranks of the mean over all nodes, Brier score of "mean >
    threshold")}; the mean is the float32 rounding of the float64 weighted sum, as the aggregate entry returns it"""
    N = y.shape[-1]
    w = np.full((1, N), 1.0 / N)
    out = {}
    ty = aggregate(y.reshape(-1, N), w)[0].astype(np.float32).reshape(-1)            # [count]
    for name, x in ensembles.items():
        count, S = x.shape[:2]
        ax = aggregate(x.reshape(-1, N), w)[0].astype(np.float32).reshape(count, S)
        lo = order_statistic(ax, scenario_rank(levels[0], S), 1)
        hi = order_statistic(ax, scenario_rank(levels[1], S), 1)
        cover = float(((lo <= ty) & (ty <= hi)).mean())
        c = events_fast(ax[:, :, None, None], [threshold], True, 1)
        r = events_fast(ty[:, None, None, None], [threshold], True, 1)
        b = brier(reliability(c, S, r)[0, 0], S)[0]
        out[name] = (cover, b)
    return out
