"""numpy fp64 restatement of the ensemble scores of include/stemgnn_hip.h (stemgnn_ensemble_scores / _masked): broadcasting over
one origin at a time, the double sums over (s, s') written out as they are defined.  Shares no code with the ops."""
import numpy as np

K = 6


def scores(target, paths, mul=None, add=None, masked=False, fair=False):
    """target [count, H, N], paths [count, S, H, N] float32 -> dict of
    out [6 * (1 + H)] float64 (overall | by_step[6][H]), hist [H, S + 1] int64, and first / second [2, 1 + H]: the two terms of
    statistics 0 and 1 (their difference is the statistic), the tolerance's yardstick."""
    target, paths = np.asarray(target, np.float32), np.asarray(paths, np.float32)
    count, S, H, N = paths.shape
    assert target.shape == (count, H, N)
    D = float(S * (S - 1)) if fair else float(S * S)
    t64, p64 = target.astype(np.float64), paths.astype(np.float64)
    if mul is not None:
        mul, add = np.asarray(mul, np.float64), np.asarray(add, np.float64)
        t64, p64 = t64 * mul + add, p64 * mul + add
    is_nan = np.isnan(target)
    valid = ~is_nan if masked else np.ones_like(is_nan)                      # [count, H, N]
    c_first, c_second, se, var = (np.zeros((count, H, N)) for _ in range(4))
    e_first, e_second = np.zeros((count, H)), np.zeros((count, H))
    rank = np.zeros((count, H, N), np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(count):
            x, y = p64[c], t64[c]                                            # [S, H, N], [H, N]
            c_first[c] = np.abs(x - y).sum(axis=0) / S
            c_second[c] = np.abs(x[:, None] - x[None, :]).sum(axis=(0, 1)) / (2.0 * D)
            mean = x.sum(axis=0) / S
            se[c] = (mean - y) ** 2
            var[c] = ((x - mean) ** 2).sum(axis=0) / (S - 1) if S > 1 else np.nan
            raw, ry = paths[c], target[c]
            rank[c] = (raw < ry).sum(axis=0) + (raw == ry).sum(axis=0) // 2
            v = valid[c]                                                     # [H, N]: the node set of every row
            dy = np.where(v, x - y, 0.0)                                     # a node outside V takes no part
            e_first[c] = np.sqrt((dy ** 2).sum(axis=-1)).sum(axis=0) / S
            dx = np.where(v, x[:, None] - x[None, :], 0.0)                   # [S, S, H, N]
            e_second[c] = np.sqrt((dx ** 2).sum(axis=-1)).sum(axis=(0, 1)) / (2.0 * D)
    row_valid = valid.any(axis=-1)                                           # [count, H]
    out = np.full(K * (1 + H), np.nan)
    first, second = np.full((2, 1 + H), np.nan), np.full((2, 1 + H), np.nan)
    hist = np.zeros((H, S + 1), np.int64)
    with np.errstate(invalid="ignore", divide="ignore"):
        for h in [None] + list(range(H)):
            sl = slice(None) if h is None else slice(h, h + 1)
            v, rv = valid[:, sl], row_valid[:, sl]
            n_el, n_row = int(v.sum()), int(rv.sum())
            f0 = np.where(v, c_first[:, sl], 0.0).sum() / n_el if n_el else np.nan
            s0 = np.where(v, c_second[:, sl], 0.0).sum() / n_el if n_el else np.nan
            f1 = np.where(rv, e_first[:, sl], 0.0).sum() / n_row if n_row else np.nan
            s1 = np.where(rv, e_second[:, sl], 0.0).sum() / n_row if n_row else np.nan
            rmse = np.sqrt(np.where(v, se[:, sl], 0.0).sum() / n_el) if n_el else np.nan
            spread = np.sqrt(np.where(v, var[:, sl], 0.0).sum() / n_el) if n_el else np.nan
            vals = (f0 - s0, f1 - s1, rmse, spread, float(n_el), float(n_row))
            at = 0 if h is None else 1 + h
            first[:, at], second[:, at] = (f0, f1), (s0, s1)
            for k, val in enumerate(vals):
                out[k if h is None else K + k * H + h] = val
    for h in range(H):
        ranked = valid[:, h] & ~is_nan[:, h]                                 # a NaN target has no rank
        hist[h] = np.bincount(rank[:, h][ranked], minlength=S + 1)
    return dict(out=out, hist=hist, first=first, second=second)


def rank_uniformity(hist):
    """chi-square of the pooled histogram [S + 1] against flat"""
    hist = np.asarray(hist, np.float64)
    expect = hist.sum() / hist.size
    return float(((hist - expect) ** 2).sum() / expect)
