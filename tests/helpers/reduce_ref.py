"""numpy restatement of scenario reduction by forward selection (include/stemgnn_hip.h: stemgnn_scenario_distances /
stemgnn_scenario_reduce), and the two statistical cases of tests/test_hip_reduce.py.

distances: in np.longdouble, returned as longdouble -- the reference the device's fp64 distances are bounded against.
forward:   the definition itself, in fp64 and in the definition's order (the k loop is sequential, vectorised over the
           candidates u and over the origins), so its results are the device's bit for bit."""
import itertools

import numpy as np


def distances(x, scale=None, squared=False):
    """x [count, S, L] float32, scale [L] or None -> D [count, S, S] longdouble: sqrt(sum_l ((x_il - x_jl) * scale_l)^2)"""
    x = np.asarray(x, np.float32).astype(np.longdouble)
    count, S, L = x.shape
    w = np.ones(L, np.longdouble) if scale is None else np.asarray(scale, np.float64).astype(np.longdouble)
    D = np.empty((count, S, S), np.longdouble)
    with np.errstate(invalid="ignore", over="ignore"):
        step = max(1, (1 << 21) // (S * L))                                      # rows i per pass: bounded memory
        for c in range(count):
            for i in range(0, S, step):
                d = (x[c, i:i + step, None, :] - x[c][None, :, :]) * w
                D[c, i:i + step] = (d * d).sum(axis=2)
        return D if squared else np.sqrt(D)


def forward(D, K):
    """D [count, S, S] float64 (D[c, k, u]: path k onto path u) -> selected int32 [count, K], counts int32 [count, K],
    assign int32 [count, S], cost float64 [count, K].  An origin with an entry that is not a finite number >= 0 is refused:
    -1, 0, -1, NaN."""
    D = np.asarray(D, np.float64)
    count, S, _ = D.shape
    with np.errstate(invalid="ignore"):
        refused = ~(np.isfinite(D) & (D >= 0)).all(axis=(1, 2))
    Dw = np.where(refused[:, None, None], 0.0, D)
    m = np.full((count, S), np.inf)
    taken = np.zeros((count, S), bool)
    selected = np.empty((count, K), np.int32)
    cost = np.empty((count, K), np.float64)
    rows = np.arange(count)
    for i in range(K):
        z = np.zeros((count, S), np.float64)
        for k in range(S):                                                       # sequential in k: the definition's order
            z = z + np.minimum(m[:, k, None], Dw[:, k, :])
        u = np.argmin(np.where(taken, np.inf, z), axis=1)                        # the lowest index among equals
        selected[:, i] = u
        cost[:, i] = z[rows, u] / S
        taken[rows, u] = True
        m = np.minimum(m, Dw[rows, :, u])
    near = np.take_along_axis(Dw, selected[:, None, :].astype(np.int64), axis=2)  # [count, S, K]: D[k, selected[j]]
    assign = np.argmin(near, axis=2).astype(np.int32)                            # the earliest pick among equals
    counts = (assign[:, :, None] == np.arange(K)).sum(axis=1).astype(np.int32)
    selected[refused], counts[refused], assign[refused], cost[refused] = -1, 0, -1, np.nan
    return selected, counts, assign, cost


def subset_cost(D, sel):
    """D [S, S], sel: kept indices -> (1 / S) sum_k min_j D[k, sel_j]: the Kantorovich distance between the uniform ensemble
    and the kept set with optimally redistributed weights"""
    D = np.asarray(D, np.float64)
    return float(D[:, np.asarray(sel, np.int64)].min(axis=1).sum() / D.shape[0])


def best_subset_cost(D, K):
    """the optimum over all subsets of K paths, by brute force (small S only)"""
    S = D.shape[0]
    return min(subset_cost(D, sel) for sel in itertools.combinations(range(S), K))


# ---- the cluster case: three well separated clusters of 32, 20 and 12 paths ----------------------------------------------------
CLUSTER_S, CLUSTER_H, CLUSTER_M, CLUSTER_SIZES = 64, 12, 5, (32, 20, 12)


def cluster_case(seed):
    """-> (paths [1, 64, 12, 5] float32, labels [64]): centres N(0, 10^2) per coordinate, unit noise, the paths shuffled"""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(3, CLUSTER_H, CLUSTER_M)) * 10.0
    labels = rng.permutation(np.repeat(np.arange(3), CLUSTER_SIZES))
    x = centres[labels] + rng.normal(size=(CLUSTER_S, CLUSTER_H, CLUSTER_M))
    return x.astype(np.float32)[None], labels


def cluster_conditions(labels, counts, assign, cost):
    """the issue's: the sorted counts are [12, 20, 32], assign reproduces the labels, cost[2] < 0.5 cost[1]"""
    same = all(len(set(assign[labels == g].tolist())) == 1 for g in range(3)) and len(set(assign.tolist())) == 3
    return sorted(counts.tolist()) == [12, 20, 32] and same and bool(cost[2] < 0.5 * cost[1])


# ---- the value case: a block-correlated random walk ----------------------------------------------------------------------------
WALK_COUNT, WALK_S, WALK_H, WALK_M, WALK_K, WALK_RHO = 256, 64, 12, 16, 8, 0.9


def walk_case(seed, count=WALK_COUNT):
    """-> paths [count, 64, 12, 16] float32: random walks over 12 steps whose unit-variance increments have correlation 0.9
    inside each of two blocks of 8 nodes and none between them"""
    rng = np.random.default_rng(seed)
    common = rng.normal(size=(count, WALK_S, WALK_H, 2, 1))
    own = rng.normal(size=(count, WALK_S, WALK_H, 2, WALK_M // 2))
    inc = np.sqrt(WALK_RHO) * common + np.sqrt(1.0 - WALK_RHO) * own
    return np.cumsum(inc.reshape(count, WALK_S, WALK_H, WALK_M), axis=2).astype(np.float32)


def peak_of_mean(paths):
    """the functional: the peak over the steps of the mean over the nodes; paths [count, S, H, M] -> [count, S] float64"""
    return np.asarray(paths, np.float64).mean(axis=3).max(axis=2)


def value_figures(peak, D, selected, counts, cost):
    """-> (MAE of the weighted reduced set's expectation / MAE of the first K paths', both against the full ensemble's;
    the share of origins with cost[K - 1] <= subset_cost(first K); mean cost[K - 1] / mean subset_cost(first K))"""
    count, S = peak.shape
    K = selected.shape[1]
    full = peak.mean(axis=1)
    kept = (np.take_along_axis(peak, selected.astype(np.int64), axis=1) * (counts / S)).sum(axis=1)
    first = peak[:, :K].mean(axis=1)
    head = np.array([subset_cost(D[c], range(K)) for c in range(count)])
    return (float(np.abs(kept - full).mean() / np.abs(first - full).mean()), float((cost[:, K - 1] <= head).mean()),
            float(cost[:, K - 1].mean() / head.mean()))


def value_conditions(fig):
    """the issue's: the error ratio at most 0.8, the share at least 0.99, the cost ratio at most 0.95"""
    return fig[0] <= 0.8 and fig[1] >= 0.99 and fig[2] <= 0.95
