"""numpy restatement of the scenario-tree entries of include/stemgnn_hip.h (stemgnn_scenario_stage_distances /
stemgnn_scenario_tree), written from the definitions.  `tree` adds in the definition's order (k sequential, the product and the
add rounded separately, fp64), so on the same D its results are the device's bit for bit; `stage_distances` sums sequentially
in the column order, in longdouble by default (the reference of the derived bound) or in fp64.  Shares no code with the ops."""
import itertools

import numpy as np


def stage_distances(x, bounds, scale=None, squared=False, dtype=np.longdouble):
    """x float32 [count, S, H, M], bounds (b_1 < .. < b_T = H) -> D [count, T, S, S] of `dtype`: Q_t summed over the stage's
    columns (h, m) in order from the differences times the scale, D_t^2 = ((Q_1 + Q_2) + ..) + Q_t, the root unless squared"""
    x = np.asarray(x, np.float32)
    count, S, H, M = x.shape
    v = x.astype(np.float64).astype(dtype).reshape(count, S, H * M)
    sc = np.ones(H * M, dtype) if scale is None else np.broadcast_to(np.asarray(scale, np.float64), (H, M)).reshape(-1).astype(dtype)
    out = np.empty((count, len(bounds), S, S), dtype)
    pre = np.zeros((count, S, S), dtype)
    lo = 0
    with np.errstate(invalid="ignore", over="ignore"):
        for t, b in enumerate(bounds):
            q = np.zeros((count, S, S), dtype)
            for l in range(lo * M, b * M):                                       # sequential in the column order
                d = (v[:, :, None, l] - v[:, None, :, l]) * sc[l]
                q = q + d * d
            pre = q if t == 0 else pre + q
            out[:, t] = pre if squared else np.sqrt(pre)
            lo = b
    return out


def present(mult, W):
    mult = np.asarray(mult, np.int64)
    return (mult >= 0).all(axis=1) & (mult.sum(axis=1) == int(W))


def _one(D, mult, W, nodes):
    """one origin: D float64 [T, S, S], mult int64 [S] -> None (refused) or (node_path, node_parent, node_count [T, n_T],
    assign [T, S], cost [T])"""
    T, S, _ = D.shape
    nT = nodes[-1]
    live = mult > 0
    members = np.nonzero(live)[0]
    if (mult < 0).any() or mult.sum() != W or nT > members.size:
        return None
    sub = D[:, members][:, :, members]
    with np.errstate(invalid="ignore"):
        if not (np.isfinite(sub) & (sub >= 0)).all():
            return None
    p = mult.astype(np.float64)
    node_path = np.full((T, nT), -1, np.int32)
    node_parent = np.full((T, nT), -1, np.int32)
    node_count = np.zeros((T, nT), np.int32)
    assign = np.full((T, S), -1, np.int32)
    cost = np.empty(T, np.float64)
    par = np.zeros(S, np.int64)
    n_prev = 1
    for t in range(T):
        Dt = D[t]
        m = np.full(S, np.inf)
        near = np.full(S, -1, np.int64)
        taken = ~live
        for i in range(nodes[t]):
            first = i < n_prev
            cand = ~taken & ((par == i) if first else True)
            z = np.zeros(S, np.float64)
            for k in members:                                                    # sequential in k: the definition's order
                if first and par[k] != i:
                    continue
                e = np.where(par == par[k], Dt[k], np.inf)                       # only onto a path of k's own parent
                term = p[k] * np.minimum(m[k], e)                                # the product, rounded
                z = z + term                                                     # then the add, rounded
            if not cand.any():                                                   # a parent without members: an empty child
                node_parent[t, i] = i
                continue
            u = int(np.argmin(np.where(cand, z, np.inf)))                        # the lowest index among equals
            if not cand[u]:                                                      # every candidate at +inf cannot happen: z is finite
                raise AssertionError("no finite candidate")
            node_path[t, i], node_parent[t, i] = u, par[u]
            taken = taken.copy()
            taken[u] = True
            for k in members:
                if par[k] == par[u] and Dt[k, u] < m[k]:                         # ties stay with the earlier pick
                    m[k], near[k] = Dt[k, u], i
        assign[t] = np.where(live, near, -1)
        for i in range(nodes[t]):
            node_count[t, i] = mult[live & (near == i)].sum()
        s = 0.0
        for k in members:
            term = p[k] * m[k]
            s = s + term
        cost[t] = s / float(W)
        par = near.copy()
        n_prev = nodes[t]
    return node_path, node_parent, node_count, assign, cost


def tree(D, mult, W, nodes):
    """D float64 [count, T, S, S] (D[c, t, k, u]: member k onto member u in stage t), mult int [count, S] or None (all ones),
    nodes (n_1 <= .. <= n_T) -> node_path, node_parent, node_count int32 [count, T, n_T], assign int32 [count, T, S], cost float64
    [count, T].  Refused (-1, -1, 0, -1, NaN at every stage): an absent origin, fewer than n_T members of positive
    multiplicity, or an entry of any stage between two such members that is not a finite number >= 0."""
    D = np.asarray(D, np.float64)
    count, T, S, _ = D.shape
    mult = np.ones((count, S), np.int64) if mult is None else np.asarray(mult, np.int64)
    nodes = tuple(int(v) for v in nodes)
    nT = nodes[-1]
    node_path = np.full((count, T, nT), -1, np.int32)
    node_parent = np.full((count, T, nT), -1, np.int32)
    node_count = np.zeros((count, T, nT), np.int32)
    assign = np.full((count, T, S), -1, np.int32)
    cost = np.full((count, T), np.nan, np.float64)
    for c in range(count):
        got = _one(D[c], mult[c], int(W), nodes)
        if got is not None:
            node_path[c], node_parent[c], node_count[c], assign[c], cost[c] = got
    return node_path, node_parent, node_count, assign, cost


def leaves(x, bounds, node_path, assign):
    """the composed leaf trajectories: x [count, S, H, N], node_path [count, T, n], assign [count, T, S] -> float32
    [count, n, H, N]; leaf j's steps of stage t are those of node_path[t, assign[t, node_path[T - 1, j]]]; NaN where there is none"""
    x = np.asarray(x, np.float32)
    count, T, n = node_path.shape
    out = np.full((count, n) + x.shape[2:], np.nan, np.float32)
    lo = (0,) + tuple(bounds[:-1])
    for c in range(count):
        for j in range(n):
            leaf = node_path[c, T - 1, j]
            if leaf < 0:
                continue
            for t in range(T):
                out[c, j, lo[t]:bounds[t]] = x[c, node_path[c, t, assign[c, t, leaf]], lo[t]:bounds[t]]
    return out


def subset_cost(Dt, mult, W, par, reps):
    """the cost of ONE stage given its representatives: every live member goes to the nearest representative among those of
    its own parent (par: the members' nodes of the stage before) -> the cost, or None where a live member's parent has none"""
    live = np.nonzero(np.asarray(mult) > 0)[0]
    total = 0.0
    for k in live:
        own = [Dt[k, u] for u in reps if par[u] == par[k]]
        if not own:
            return None
        total += float(mult[k]) * min(own)
    return total / W


def best_subset_cost(Dt, mult, W, par, n):
    """brute force: the smallest subset_cost over all n representatives among the live members that leave no parent childless"""
    live = [k for k in range(Dt.shape[0]) if mult[k] > 0]
    best = np.inf
    for reps in itertools.combinations(live, n):
        c = subset_cost(Dt, mult, W, par, reps)
        if c is not None:
            best = min(best, c)
    return best


PLANT_S, PLANT_H, PLANT_M = 64, 6, 4
PLANT_BOUNDS, PLANT_NODES = (2, 4, 6), (2, 4, 8)
PLANT_SIZES = (12, 4, 9, 7, 10, 6, 11, 5)


def planted_case(seed):
    """-> (x float32 [64, 6, 4], labels int [3, 64]): a binary tree of depth 3; the centre of a node's two steps is
    4 * N(0, 1) per level, the noise 0.05; leaf l has PLANT_SIZES[l] members and the labels (l >> 2, l >> 1, l) at the three
    stages; the members are in shuffled order"""
    rng = np.random.default_rng(seed)
    centres = [4.0 * rng.normal(size=(2 << t, 2, PLANT_M)) for t in range(3)]
    leaf = np.repeat(np.arange(8), PLANT_SIZES)
    leaf = leaf[rng.permutation(PLANT_S)]
    x = np.empty((PLANT_S, PLANT_H, PLANT_M))
    labels = np.empty((3, PLANT_S), np.int64)
    for t in range(3):
        labels[t] = leaf >> (2 - t)
        x[:, 2 * t:2 * t + 2] = centres[t][labels[t]]
    x = x + 0.05 * rng.normal(size=x.shape)
    return x.astype(np.float32), labels


def planted_conditions(labels, assign, node_count):
    """assign [3, S] reproduces the planted labels up to renaming at all three stages, and the counts are the planted sizes"""
    for t in range(3):
        pairs = set(zip(labels[t].tolist(), assign[t].tolist()))
        if len(pairs) != (2 << t) or len({a for a, _ in pairs}) != (2 << t) or len({b for _, b in pairs}) != (2 << t):
            return False
        want = sorted(np.bincount(labels[t], minlength=2 << t).tolist())
        if sorted(node_count[t, :2 << t].tolist()) != want:
            return False
    return True


def random_mult(rng, count, S, W, zeros=True):
    """int32 [count, S]: multiplicities that sum to W, a few zeros among them where S > 1"""
    mult = np.zeros((count, S), np.int64)
    for c in range(count):
        on = np.nonzero(rng.random(S) < 0.8)[0] if (zeros and S > 1) else np.arange(S)
        on = (on if on.size else np.array([0]))[:W]
        mult[c, on] = 1
        np.add.at(mult[c], rng.choice(on, size=W - on.size), 1)
    return mult.astype(np.int32)
