"""numpy restatement of the weighted scenario-set entries of include/stemgnn_hip.h (stemgnn_weighted_bands / _scores / _events,
stemgnn_scenario_reduce_weighted), written from the definitions: member k of origin c carries the multiplicity mult[c, k] among
W paths, and nothing here forms the replicated ensemble.  Sums are fp64; `forward` adds in the definition's order (k sequential,
the product and the add rounded separately), so its results are the device's bit for bit.  Shares no code with the ops."""
import numpy as np

K_OUT = 7
NAN_BITS = np.uint32(0x7FC00000)


def present(mult, W):
    """mult int [count, K] -> bool [count]: no negative multiplicity and the sum is W"""
    mult = np.asarray(mult, np.int64)
    return (mult >= 0).all(axis=1) & (mult.sum(axis=1) == int(W))


def rank(tau, W):
    """stemgnn_scenario_rank: min(W, max(1, ceil(tau * W * (1 - 1e-12))))"""
    return int(min(W, max(1, np.ceil(float(tau) * int(W) * (1.0 - 1e-12)))))


def _order_key(v):
    """float32 -> a float64 key whose ascending stable sort is the definition's order: -0 == +0, NaN last"""
    v = np.asarray(v, np.float32)
    k = v.astype(np.float64) + 0.0
    k[v == 0] = 0.0
    k[np.isposinf(v)] = 1e300
    k[np.isnan(v)] = np.inf
    return k


def denorm(x, mul=None, add=None):
    v = np.asarray(x, np.float32).astype(np.float64)
    if mul is None:
        return v
    with np.errstate(all="ignore"):
        return v * np.asarray(mul, np.float64) + np.asarray(add, np.float64)


def bands(paths, mult, W, ranks):
    """paths float32 [count, K, H, N], ranks: Q 1-based ranks within [1, W] -> float32 [count, Q, H, N]: the first value in the
    order whose cumulative multiplicity reaches the rank; an absent origin is NaN (0x7fc00000)"""
    paths, mult = np.asarray(paths, np.float32), np.asarray(mult, np.int64)
    count, K, H, N = paths.shape
    out = np.empty((count, len(ranks), H, N), np.float32)
    out.view(np.uint32)[...] = NAN_BITS
    ok = present(mult, W)
    for c in range(count):
        if not ok[c]:
            continue
        live = np.nonzero(mult[c] > 0)[0]                                        # a member of multiplicity 0 is not read
        x, w = paths[c, live], mult[c, live]
        order = np.argsort(_order_key(x), axis=0, kind="stable")
        v = np.take_along_axis(x, order, axis=0)
        cum = np.cumsum(w[order], axis=0)                                        # [k, H, N]
        for q, r in enumerate(ranks):
            at = (cum >= int(r)).argmax(axis=0)
            out[c, q] = np.take_along_axis(v, at[None], axis=0)[0]
    return out


def events(paths, mult, W, thr, above, min_run, mul=None, add=None):
    """paths float32 [count, K, H, M], thr float64 [M] -> int32 [count, 2 H + 1, M]: step | first | run counts in
    multiplicities; an absent origin is -1"""
    v = denorm(paths, mul, add)
    mult = np.asarray(mult, np.int64)
    count, K, H, M = v.shape
    thr = np.broadcast_to(np.asarray(thr, np.float64), (M,))
    with np.errstate(invalid="ignore"):
        e = (v > thr) if above else (v < thr)
    w = np.where(mult > 0, mult, 0)[:, :, None]                                  # [count, K, 1]
    e = e & (mult > 0)[:, :, None, None]
    out = np.zeros((count, 2 * H + 1, M), np.int64)
    crossed = np.zeros((count, K, M), bool)
    cur = np.zeros((count, K, M), np.int64)
    best = np.zeros((count, K, M), np.int64)
    for h in range(H):
        eh = e[:, :, h]
        out[:, h] = (eh * w).sum(axis=1)
        out[:, H + h] = ((eh & ~crossed) * w).sum(axis=1)
        crossed |= eh
        cur = np.where(eh, cur + 1, 0)
        best = np.maximum(best, cur)
    out[:, 2 * H] = ((best >= min_run) * w).sum(axis=1)
    out[~present(mult, W)] = -1
    return out.astype(np.int32)


def scores(target, paths, mult, W, mul=None, add=None, masked=False, fair=False):
    """target [count, H, N], paths [count, K, H, N] float32, mult [count, K] -> dict of out [7 * (1 + H)] float64 (overall |
    by_step[7][H]), hist [H, W + 1] int64, and first / second [2, 1 + H]: the two terms of statistics 0 and 1"""
    target, paths = np.asarray(target, np.float32), np.asarray(paths, np.float32)
    mult = np.asarray(mult, np.int64)
    count, K, H, N = paths.shape
    W = int(W)
    D = float(W) * float(W - 1) if fair else float(W) * float(W)
    t64, p64 = denorm(target, mul, add), denorm(paths, mul, add)
    ok = present(mult, W)
    is_nan = np.isnan(target)
    valid = (~is_nan if masked else np.ones_like(is_nan)) & ok[:, None, None]
    c_first, c_second, se, var = (np.zeros((count, H, N)) for _ in range(4))
    e_first, e_second = np.zeros((count, H)), np.zeros((count, H))
    rk = np.zeros((count, H, N), np.int64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for c in range(count):
            if not ok[c]:
                continue
            live = np.nonzero(mult[c] > 0)[0]
            x, y = p64[c, live], t64[c]                                          # [k, H, N], [H, N]
            wi = mult[c, live]
            w = wi.astype(np.float64)[:, None, None]
            ww = (wi[:, None] * wi[None, :]).astype(np.float64)                  # exact: W <= 2^24
            c_first[c] = (w * np.abs(x - y)).sum(axis=0) / W
            c_second[c] = (ww[:, :, None, None] * np.abs(x[:, None] - x[None, :])).sum(axis=(0, 1)) / (2.0 * D)
            mean = (w * x).sum(axis=0) / W
            se[c] = (mean - y) ** 2
            var[c] = (w * (x - mean) ** 2).sum(axis=0) / (W - 1) if W > 1 else np.nan
            raw, ry = paths[c, live], target[c]
            wk = wi[:, None, None]
            rk[c] = (wk * (raw < ry)).sum(axis=0) + (wk * (raw == ry)).sum(axis=0) // 2
            v = valid[c]
            dy = np.where(v, x - y, 0.0)
            e_first[c] = (w[:, :, 0] * np.sqrt((dy ** 2).sum(axis=-1))).sum(axis=0) / W
            dx = np.where(v, x[:, None] - x[None, :], 0.0)
            e_second[c] = (ww[:, :, None] * np.sqrt((dx ** 2).sum(axis=-1))).sum(axis=(0, 1)) / (2.0 * D)
    row_valid = valid.any(axis=-1)
    out = np.full(K_OUT * (1 + H), np.nan)
    first, second = np.full((2, 1 + H), np.nan), np.full((2, 1 + H), np.nan)
    hist = np.zeros((H, W + 1), np.int64)
    gone = float((~ok).sum())
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
            vals = (f0 - s0, f1 - s1, rmse, spread, float(n_el), float(n_row), gone)
            at = 0 if h is None else 1 + h
            first[:, at], second[:, at] = (f0, f1), (s0, s1)
            for k, val in enumerate(vals):
                out[k if h is None else K_OUT + k * H + h] = val
    for h in range(H):
        ranked = valid[:, h] & ~is_nan[:, h]                                     # a NaN target has no rank
        hist[h] = np.bincount(rk[:, h][ranked], minlength=W + 1)
    return dict(out=out, hist=hist, first=first, second=second)


def forward(D, mult, W, K):
    """D float64 [count, S, S] (D[c, k, u]: member k onto member u), mult int [count, S] -> selected int32 [count, K], counts
    int32 [count, K], assign int32 [count, S], cost float64 [count, K].  Refused (-1, 0, -1, NaN): an absent origin, fewer than
    K members of positive multiplicity, or an entry between two such members that is not a finite number >= 0."""
    D, mult = np.asarray(D, np.float64), np.asarray(mult, np.int64)
    count, S, _ = D.shape
    live = mult > 0                                                              # [count, S]
    read = live[:, :, None] & live[:, None, :]                                   # the entries that are read at all
    with np.errstate(invalid="ignore"):
        bad = (read & ~(np.isfinite(D) & (D >= 0))).any(axis=(1, 2))
    refused = ~present(mult, W) | (live.sum(axis=1) < K) | bad
    Dw = np.where(read & ~refused[:, None, None], D, 0.0)
    p = np.where(live, mult, 0).astype(np.float64)
    m = np.full((count, S), np.inf)
    taken = ~live
    selected = np.zeros((count, K), np.int32)
    cost = np.empty((count, K), np.float64)
    rows = np.arange(count)
    for i in range(K):
        z = np.zeros((count, S), np.float64)
        for k in range(S):                                                       # sequential in k: the definition's order
            term = p[:, k, None] * np.minimum(m[:, k, None], Dw[:, k, :])        # the product, rounded
            z = np.where(live[:, k, None], z + term, z)                          # then the add, rounded
        u = np.argmin(np.where(taken, np.inf, z), axis=1)                        # the lowest index among equals
        selected[:, i] = u
        cost[:, i] = z[rows, u] / float(W)
        taken = taken.copy()
        taken[rows, u] = True
        m = np.minimum(m, Dw[rows, :, u])
    near = np.take_along_axis(Dw, selected[:, None, :].astype(np.int64), axis=2)  # [count, S, K]: D[k, selected[j]]
    assign = np.where(live, np.argmin(near, axis=2), -1).astype(np.int32)        # the earliest pick among equals
    counts = ((assign[:, :, None] == np.arange(K)) * np.where(live, mult, 0)[:, :, None]).sum(axis=1).astype(np.int32)
    selected[refused], counts[refused], assign[refused], cost[refused] = -1, 0, -1, np.nan
    return selected, counts, assign, cost


def replicate(paths, mult):
    """the ensemble the definitions speak of, member k mult[k] times in a row: for the SECOND reference only (the project's
    unweighted entries and helpers); every origin must be present.  paths [count, K, ...] -> [count, W, ...]"""
    mult = np.asarray(mult, np.int64)
    return np.stack([np.repeat(paths[c], mult[c], axis=0) for c in range(paths.shape[0])])


def round_weights(weights, total):
    """largest-remainder rounding of one row of probabilities to multiplicities that sum to total, the lower index first among
    equal remainders; plain Python on float64"""
    w = [float(v) for v in weights]
    s = sum(w)
    q = [v / s * total for v in w]
    base = [int(np.floor(v)) for v in q]
    short = total - sum(base)
    order = sorted(range(len(w)), key=lambda i: (-(q[i] - base[i]), i))
    for i in order[:short]:
        base[i] += 1
    return base


def random_set(rng, count, K, H, N, W, zeros=True):
    """-> (paths float32 [count, K, H, N], target float32 [count, H, N], mult int32 [count, K]): standard normal values; the
    multiplicities sum to W with a few zeros among them (where K > 1), and one multiplicity-0 member per origin is NaN-filled"""
    paths = rng.normal(size=(count, K, H, N)).astype(np.float32)
    target = rng.normal(size=(count, H, N)).astype(np.float32)
    mult = np.zeros((count, K), np.int64)
    for c in range(count):
        on = np.nonzero(rng.random(K) < 0.8)[0] if (zeros and K > 1) else np.arange(K)
        on = (on if on.size else np.array([0]))[:W]
        mult[c, on] = 1
        np.add.at(mult[c], rng.choice(on, size=W - on.size), 1)
        off = np.nonzero(mult[c] == 0)[0]
        if off.size:
            paths[c, off[0]] = np.nan
    assert (mult.sum(axis=1) == W).all()
    return paths, target, mult.astype(np.int32)
