"""Device mirror of the reference's ``utils/math_utils.py``: MAPE / MAE / RMSE / evaluate on
[count, time_step, node] tensors that stay on the GPU; one fused fp64 kernel pass (`stemgnn_eval_metrics`) yields
every axis variant, and only the few result numbers come back to the host.

Quirks kept (utils/math_utils.py:32-33): MAPE adds 1e-5 to each ratio and clips at 5; a 0/0 stays NaN.
"""
import numpy as np
import torch

from . import ops


def _as_f32(t, like=None):
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
        if like is not None:
            t = t.to(like.device)
    return t.float() if t.dtype != torch.float32 else t


class Scores:
    """All axis variants of (MAPE, MAE, RMSE) from one kernel pass.  ignore_nan: elements whose ground truth is NaN (missing
    readings) are left out of every mean (`stemgnn_eval_metrics_masked`); a slice with none left is NaN."""

    def __init__(self, y, y_hat, mul=None, add=None, ignore_nan=False):
        y_hat = _as_f32(y_hat)
        y = _as_f32(y, like=y_hat)
        C, H, N = y.shape
        v = ops.eval_metrics(y, y_hat, mul, add, ignore_nan=bool(ignore_nan)).cpu().numpy()
        self.overall = v[:3]
        o = 3
        self.by_node = v[o:o + 3 * N].reshape(3, N); o += 3 * N
        self.by_step = v[o:o + 3 * H].reshape(3, H); o += 3 * H
        self.by_step_node = v[o:o + 3 * H * N].reshape(3, H, N)

    def get(self, by_step=False, by_node=False):
        if by_step and by_node:
            m = self.by_step_node
        elif by_step:
            m = self.by_step
        elif by_node:
            m = self.by_node
        else:
            return tuple(np.float64(x) for x in self.overall)
        return m[0].copy(), m[1].copy(), m[2].copy()


class QuantileScores:
    """Calibration of a quantile forecast from one kernel pass (`stemgnn_quantile_metrics`): y [count, H, N] ground truth,
    y_hat [count, Q, H, N], quantiles = the Q levels.  Attributes (numpy float64; `*_step` = the same per horizon step, a
    trailing axis of H), with P = Q // 2 pairs (i, Q-1-i):
      pinball [Q]            mean pinball loss per level        coverage [Q]          share of y <= y_hat_q (nominal: the level)
      interval_coverage [P]  share of y_hat_i <= y <= y_hat_{Q-1-i}   interval_width [P]    mean y_hat_{Q-1-i} - y_hat_i
      interval_nominal [P]   tau_{Q-1-i} - tau_i                crossing              share of elements whose Q forecasts are
                                                                                      not non-decreasing in q
    mul / add: per-node de-normalisation, applied in fp64 ahead of everything.  ignore_nan: elements whose ground truth is NaN
    are left out everywhere (`stemgnn_quantile_metrics_masked`); a slice with none left is NaN."""

    def __init__(self, y, y_hat, quantiles, mul=None, add=None, ignore_nan=False):
        y_hat = _as_f32(y_hat)
        y = _as_f32(y, like=y_hat)
        q = tuple(float(t) for t in quantiles)
        Q, P, H = len(q), len(q) // 2, y.shape[1]
        K = 2 * Q + 2 * P + 1
        v = ops.quantile_metrics(y, y_hat, q, mul, add, ignore_nan=bool(ignore_nan)).cpu().numpy()
        self.quantiles = q
        self.interval_nominal = np.array([q[Q - 1 - i] - q[i] for i in range(P)], dtype=np.float64)
        for suffix, m in (("", v[:K]), ("_step", v[K:].reshape(K, H))):
            setattr(self, "pinball" + suffix, m[:Q].copy())
            setattr(self, "coverage" + suffix, m[Q:2 * Q].copy())
            setattr(self, "interval_coverage" + suffix, m[2 * Q:2 * Q + P].copy())
            setattr(self, "interval_width" + suffix, m[2 * Q + P:2 * Q + 2 * P].copy())
            setattr(self, "crossing" + suffix, m[2 * Q + 2 * P].copy() if suffix else np.float64(m[2 * Q + 2 * P]))


class EnsembleScores:
    """Proper scores of sampled paths from one call (`stemgnn_ensemble_scores`): y [count, H, N] ground truth, paths
    [count, S, H, N] (`trainer.rolling_scenarios(..., return_paths=True)`).  Attributes (numpy; `*_step` = the same per horizon
    step [H]):
      crps     mean continuous ranked probability score over the elements: marginal, per (step, node)
      energy   mean energy score over the (origin, step) rows: multivariate over the nodes of a row, so it sees the dependence
               between nodes -- the score that compares `coupling=` choices (their marginals, hence their crps, are the same)
      rmse     RMSE of the ensemble mean           spread   sqrt(mean ensemble variance); spread / rmse near 1: spread matches skill
      valid    elements scored                     valid_rows   rows scored
      rank_histogram [S + 1] (the sum over steps) and rank_histogram_step [H, S + 1], int64: where the truth falls among the S
               sorted path values (ties at the midrank); flat when calibrated, U-shaped when the paths are too narrow
      rank_uniformity   the chi-square statistic of rank_histogram against flat, rank_uniformity_dof = S its degrees of freedom
    mul / add: per-node de-normalisation in fp64 ahead of everything.  ignore_nan: NaN targets are missing readings
    (`stemgnn_ensemble_scores_masked`); a slice with nothing valid is NaN.  fair: the pair terms of crps and energy are divided by
    S (S - 1) instead of S^2, unbiased in S: for comparing runs with different `paths=`.  One host sync."""

    def __init__(self, y, paths, mul=None, add=None, ignore_nan=False, fair=False):
        paths = _as_f32(paths)
        y = _as_f32(y, like=paths)
        out, hist = ops.ensemble_scores(y, paths, mul, add, ignore_nan=bool(ignore_nan), fair=bool(fair))
        self._fill(out, hist, 6)

    @classmethod
    def _weighted(cls, y, paths, mult, total, mul=None, add=None, ignore_nan=False, fair=False):
        """The scores of a weighted set (`stemgnn_weighted_scores`, through `ScenarioSet.scores`): the same attributes, the
        histograms over total + 1 bins, and `absent`, the number of origins left out (refused by the reduction, or with
        multiplicities that do not sum to total).  One host sync."""
        paths = _as_f32(paths)
        y = _as_f32(y, like=paths)
        self = cls.__new__(cls)
        out, hist = ops.weighted_scores(y, paths, mult, total, mul, add, ignore_nan=bool(ignore_nan), fair=bool(fair))
        v = self._fill(out, hist, 7)
        self.absent = int(v[6])
        return self

    def _fill(self, out, hist, K):
        """the attributes from out [K * (1 + H)] and hist [H, S + 1] (device): the one sync"""
        H, S = int(hist.shape[0]), int(hist.shape[1]) - 1
        flat = torch.cat([out, hist.reshape(-1).double()]).cpu().numpy()         # (counts below 2^53: exact as doubles)
        v, h = flat[:out.numel()], flat[out.numel():].astype(np.int64).reshape(H, S + 1)
        names = ("crps", "energy", "rmse", "spread", "valid", "valid_rows")
        for k, name in enumerate(names):
            kind = np.float64 if k < 4 else np.int64                         # the two counts are integers
            setattr(self, name, kind(v[k]))
            setattr(self, name + "_step", v[K + k * H:K + (k + 1) * H].astype(kind))
        self.rank_histogram_step = h.copy()
        self.rank_histogram = h.sum(axis=0)
        total = int(self.rank_histogram.sum())
        expect = total / (S + 1.0)
        self.rank_uniformity_dof = S
        self.rank_uniformity = np.float64(((self.rank_histogram - expect) ** 2).sum() / expect) if total else np.float64("nan")
        return v


MAX_GROUPS = 32                              # R of stemgnn_scenario_aggregate


def group_weights(groups, N, reduce="mean"):
    """The [R, N] float64 weight matrix of node groups (host tensor; `ops.scenario_aggregate` takes it).  groups: a [R, N]
    tensor / array, used as it is, or a sequence of index sequences: 1 / len(g) ("mean") or 1 ("sum") on the members of g, 0
    elsewhere.  Validated on the host: indices within [0, N), no empty group, no index twice in a group, R <= 32."""
    if reduce not in ("mean", "sum"):
        raise ValueError(f"group_weights: reduce is 'mean' or 'sum', got {reduce!r}")
    N = int(N)
    if N < 1:
        raise ValueError(f"group_weights: N must be at least 1, got {N}")
    if torch.is_tensor(groups) or isinstance(groups, np.ndarray):
        w = groups.detach().cpu() if torch.is_tensor(groups) else torch.as_tensor(groups)
        if w.dim() != 2 or w.shape[1] != N or w.shape[0] < 1 or w.is_complex() or w.dtype == torch.bool:
            raise ValueError(f"group_weights: a weight matrix must be real and [R, {N}], got {w.dtype} {tuple(w.shape)}")
        if w.shape[0] > MAX_GROUPS:
            raise ValueError(f"group_weights: at most {MAX_GROUPS} groups, got {w.shape[0]}")
        return w.to(torch.float64).contiguous()
    groups = [list(g) for g in groups]
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError(f"group_weights: 1 to {MAX_GROUPS} groups, got {len(groups)}")
    w = torch.zeros(len(groups), N, dtype=torch.float64)
    for r, g in enumerate(groups):
        if not g:
            raise ValueError(f"group_weights: group {r} is empty")
        idx = [int(i) for i in g]
        if any(i != j for i, j in zip(idx, g)) or min(idx) < 0 or max(idx) >= N:
            raise ValueError(f"group_weights: group {r} has an index outside [0, {N})")
        if len(set(idx)) != len(idx):
            raise ValueError(f"group_weights: group {r} names an index twice")
        w[r, idx] = 1.0 / len(idx) if reduce == "mean" else 1.0
    return w


def _brier(table, S):
    """(brier, base_rate, skill) of a reliability table [..., S + 1, 2] of (n_j, o_j), fp64 on the host"""
    n, o = table[..., 0].astype(np.float64), table[..., 1].astype(np.float64)
    p = np.arange(S + 1, dtype=np.float64) / S
    with np.errstate(divide="ignore", invalid="ignore"):
        V = n.sum(axis=-1)
        brier = (o * (1.0 - p) ** 2 + (n - o) * p ** 2).sum(axis=-1) / V
        base = o.sum(axis=-1) / V
        skill = np.where((base > 0) & (base < 1), 1.0 - brier / (base * (1.0 - base)), np.nan)
    return brier, base, skill


class EventScores:
    """Verification of event probabilities against what happened, from one integer table (`ScenarioEvents.score`).
    A forecast probability is j / S, j the number of paths in the event.  For each of "any" (the event at some step), "run" (at
    least min_run steps in a row) and every single step:
      reliability        int64 [M, S + 1, 2] = (n_j, o_j): the valid (origin, column) pairs whose forecast count was j, and those
                         of them where the event occurred            (reliability_run; reliability_step [H, M, S + 1, 2])
      brier              (1 / V) sum_j [o_j (1 - j / S)^2 + (n_j - o_j) (j / S)^2], V = sum_j n_j
      base_rate          sum_j o_j / V
      skill              1 - brier / (base_rate (1 - base_rate)), NaN when the base rate is 0 or 1 (or nothing is valid)
    each overall (brier, brier_run, brier_step [H]) and per column (brier_column [M], brier_run_column, brier_step_column
    [H, M]), numpy float64 computed on the host from the table: exact functions of integers.  valid: V of "any"."""

    def __init__(self, table, S):
        table = np.asarray(table, dtype=np.int64)                                # [2 + H, M, S + 1, 2]
        self.S = int(S)
        self.reliability, self.reliability_run, self.reliability_step = table[0], table[1], table[2:]
        for suffix, t in (("", table[0]), ("_run", table[1]), ("_step", table[2:])):
            pooled = t.sum(axis=-3)
            for column, tab in (("", pooled), ("_column", t)):
                b, r, s = _brier(tab, self.S)
                whole = suffix != "_step" and not column
                setattr(self, "brier" + suffix + column, np.float64(b) if whole else b)
                setattr(self, "base_rate" + suffix + column, np.float64(r) if whole else r)
                setattr(self, "skill" + suffix + column, np.float64(s) if whole else s)
        self.valid = int(table[0][..., 0].sum())


class ScenarioEvents:
    """The counts of `ops.scenario_events` (int32 [count, 2H + 1, M], device) of S paths, read as probabilities (float64 device
    tensors, no sync):
      p_step [count, H, M]  the event at step h              p_by [count, H, M]   the event at some step <= h (first passage)
      p_any [count, M]      the event at some step           p_run [count, M]     at least min_run steps in a row
      duration [count, M]   the expected number of steps in the event
    cat(parts) joins batches along the origins.  score(realised, ignore_nan=False) -> EventScores: `realised` is
    `EventSpec.realised(target)`, the same counts of the one path that happened (S = 1) with `missing` [count, H, M].
    ignore_nan: an (origin, column) with a missing (NaN) target at ANY step is left out of "any" and "run", a missing step out of
    that step alone; without it a NaN target is "not in the event" (the strict comparison's answer) and everything is valid."""

    def __init__(self, counts, S, missing=None):
        if counts.dim() != 3 or counts.shape[1] % 2 != 1 or counts.dtype != torch.int32:
            raise ValueError(f"ScenarioEvents: counts must be int32 [count, 2H + 1, M], got {counts.dtype} {tuple(counts.shape)}")
        self.counts, self.S, self.missing = counts, int(S), missing
        self.count, self.H, self.M = int(counts.shape[0]), int(counts.shape[1]) // 2, int(counts.shape[2])

    @property
    def step(self):
        return self.counts[:, :self.H]

    @property
    def first(self):
        return self.counts[:, self.H:2 * self.H]

    @property
    def run(self):
        return self.counts[:, 2 * self.H]

    def _p(self, n):
        """n / S; NaN where the counts are negative (an absent origin of a weighted set: `ops.weighted_events` files -1)"""
        p = n.double() / self.S
        return torch.where(n < 0, torch.full_like(p, float("nan")), p)

    @property
    def p_step(self):
        return self._p(self.step)

    @property
    def p_by(self):
        return self._p(self.first.cumsum(dim=1))

    @property
    def p_any(self):
        return self._p(self.first.sum(dim=1))

    @property
    def p_run(self):
        return self._p(self.run)

    @property
    def duration(self):
        return self._p(self.step.sum(dim=1))

    @staticmethod
    def cat(parts):
        parts = list(parts)
        if not parts or any(p.S != parts[0].S or p.counts.shape[1:] != parts[0].counts.shape[1:] for p in parts):
            raise ValueError("ScenarioEvents.cat: the parts must share S, H and M")
        missing = None if parts[0].missing is None else torch.cat([p.missing for p in parts])
        return ScenarioEvents(torch.cat([p.counts for p in parts]), parts[0].S, missing)

    def score(self, realised, ignore_nan=False):
        if not isinstance(realised, ScenarioEvents) or realised.S != 1 or realised.counts.shape != self.counts.shape:
            raise ValueError("ScenarioEvents.score: realised must be EventSpec.realised(target) of the same origins, steps and "
                             "columns")
        H, M, S = self.H, self.M, self.S
        # kinds: any | run | step 0 .. H - 1; forecast count j and occurrence o of every (kind, origin, column)
        j = torch.cat([self.first.sum(dim=1, keepdim=True), self.run[:, None], self.step], dim=1).long()
        o = torch.cat([realised.first.sum(dim=1, keepdim=True), realised.run[:, None], realised.step], dim=1).long()
        kinds = H + 2
        k = torch.arange(kinds, device=j.device)[None, :, None]
        m = torch.arange(M, device=j.device)[None, None, :]
        key = ((k * M + m) * (S + 1) + j) * 2 + o
        bins = kinds * M * (S + 1) * 2
        key = torch.where(j < 0, torch.full_like(key, bins), key)               # an absent origin of a weighted set is left out
        if ignore_nan and realised.missing is not None:
            gone = realised.missing.any(dim=1, keepdim=True)
            key = torch.where(torch.cat([gone, gone, realised.missing], dim=1), torch.full_like(key, bins), key)
        table = torch.bincount(key.reshape(-1), minlength=bins + 1)[:bins].reshape(kinds, M, S + 1, 2).cpu().numpy()   # the sync
        out = np.empty_like(table)
        out[..., 0] = table.sum(axis=-1)
        out[..., 1] = table[..., 1]
        return EventScores(out, S)


class EventSpec:
    """The definition of an event on scenario paths: value > threshold (above=True) or value < threshold, for at least `min_run`
    consecutive steps where a run is asked for, per node or per GROUP of nodes.
    threshold: a scalar or one value per column (node, or group with groups=), in raw units when mul / add are given.
    groups / reduce: `group_weights`' arguments: the event is about the mean (or sum) over each group's nodes -- the one
    product where the `coupling=` of the paths changes the answer.  mul / add: per-node de-normalisation, fp64.
      count(paths [count,S,H,N]) -> ScenarioEvents; with groups the paths are aggregated first (`ops.scenario_aggregate`, which
                                  de-normalises), then counted with no further de-normalisation (`ops.scenario_events`)
                                  paths a ScenarioSet: its kept paths, every member counted with its multiplicity
                                  (`ops.weighted_events`) -> ScenarioEvents(counts, set.total); an absent origin is -1 / NaN
      aggregate(x [..., N])      -> [..., R] float32, the aggregated (de-normalised) paths or target: rolling_scenarios' layout
                                  with N = R, so ops.scenario_bands, EnsembleScores and QuantileScores take it as it is
      realised(target [count,H,N]) -> ScenarioEvents of the one path that happened (S = 1) with `missing` [count,H,M]: the
                                  (aggregated) target is NaN there"""

    def __init__(self, threshold, above=True, min_run=1, groups=None, reduce="mean", mul=None, add=None):
        if isinstance(min_run, bool) or int(min_run) != min_run or int(min_run) < 1:
            raise ValueError(f"EventSpec: min_run must be an integer of at least 1, got {min_run!r}")
        if reduce not in ("mean", "sum"):
            raise ValueError(f"EventSpec: reduce is 'mean' or 'sum', got {reduce!r}")
        if (mul is None) != (add is None):
            raise ValueError("EventSpec: mul and add go together")
        if groups is not None and not (torch.is_tensor(groups) or isinstance(groups, np.ndarray)):
            groups = [list(g) for g in groups]
        self.threshold, self.above, self.min_run = threshold, bool(above), int(min_run)
        self.groups, self.reduce, self.mul, self.add = groups, reduce, mul, add
        self._weights = {}

    def weights(self, N, device):
        key = (int(N), str(device))
        if key not in self._weights:
            self._weights[key] = group_weights(self.groups, N, self.reduce).to(device)
        return self._weights[key]

    def aggregate(self, x):
        if self.groups is None:
            raise ValueError("EventSpec.aggregate: the spec has no groups=")
        x = _as_f32(x)
        return ops.scenario_aggregate(x, self.weights(x.shape[-1], x.device), self.mul, self.add)

    def _count(self, paths):
        paths = _as_f32(paths)
        if paths.dim() != 4:
            raise ops._lib.StemGNNHipError(f"EventSpec: paths must be [count,S,H,N], got {tuple(paths.shape)}")
        if self.groups is not None:
            return ops.scenario_events(self.aggregate(paths), self.threshold, self.above, self.min_run), paths.shape[1]
        return ops.scenario_events(paths, self.threshold, self.above, self.min_run, self.mul, self.add), paths.shape[1]

    def count(self, paths):
        if isinstance(paths, ScenarioSet):                                       # the kept paths, counted with their multiplicities
            kept = paths.paths
            if self.groups is not None:
                counts = ops.weighted_events(self.aggregate(kept), paths.counts, paths.total, self.threshold, self.above,
                                             self.min_run)
            else:
                counts = ops.weighted_events(kept, paths.counts, paths.total, self.threshold, self.above, self.min_run,
                                             self.mul, self.add)
            return ScenarioEvents(counts, paths.total)
        counts, S = self._count(paths)
        return ScenarioEvents(counts, S)

    def realised(self, target):
        target = _as_f32(target)
        if target.dim() != 3:
            raise ops._lib.StemGNNHipError(f"EventSpec.realised: target must be [count,H,N], got {tuple(target.shape)}")
        if self.groups is not None:
            value = self.aggregate(target)
            counts = ops.scenario_events(value[:, None], self.threshold, self.above, self.min_run)
        else:
            value = target
            counts = ops.scenario_events(target[:, None], self.threshold, self.above, self.min_run, self.mul, self.add)
        return ScenarioEvents(counts, 1, torch.isnan(value))


def _first_min(values):
    """the lowest position of the minimum along the last axis (torch.argmin leaves the choice among equals open)"""
    k = values.shape[-1]
    pos = torch.arange(k, device=values.device).expand_as(values)
    return torch.where(values == values.amin(dim=-1, keepdim=True), pos, torch.full_like(pos, k)).amin(dim=-1)


class ScenarioSet:
    """K representative paths per origin with weights: the result of `reduce_scenarios` (scenario reduction by forward
    selection, `ops.scenario_reduce`).  Device tensors, no sync:
      index   int64 [count, K]    the kept paths' indices among the S, in the order they were picked
      counts  int32 [count, K]    the paths whose nearest kept path each is       weights  float64 [count, K] = counts / S
      assign  int32 [count, S]    the position in 0 .. K-1 every path went to
      cost    float64 [count, K]  the Kantorovich distance between the full ensemble and the first i + 1 picks with their
                                  optimal weights: non-increasing in i, so K can be chosen by tolerance (keep_for)
      paths   float32 [count, K, H, N]  the kept trajectories                      S  the size of the ensemble
    A refused origin (a NaN or an infinity among its distances): index and assign -1, counts 0, cost NaN, and its `paths` rows and
    `weights` are NaN, so nothing computed from them passes for a number.
      expect(values [count, S, ...]) -> float64 [count, ...]: the weighted sum over the kept members of any functional
                    evaluated on all S paths -- what the full ensemble's mean of it is replaced by
      keep_for(tol) -> int64 [count]: the smallest number of members whose cost is at most tol * cost[:, 0]
      head(k)       -> the ScenarioSet of the first k picks (forward selection is nested: they ARE the picks at keep = k); its
                    counts and assign are re-derived from the distances, so the set must still hold `distances` [count, S, S]
                    or `source` = (the [count, S, H, R] tensor the distances were taken on, scale, squared): reduce_scenarios
                    keeps a reference to the latter, trainer.reduced_scenarios drops it with the batch's paths
      cat(parts)    joins batches along the origins
    The set as a weighted ensemble: member k stands counts[c, k] times among `total` paths (total = S
    unless the set was reduced again, merged or made from_weights; weights = counts / total).  An origin is ABSENT when a count
    is negative or the counts do not sum to total (a refused origin's are 0): NaN bands, NaN probabilities, left out of scores.
      bands(quantiles, out=None) -> float32 [count, Q, H, N], `ops.scenario_bands` of the replicated ensemble, bit for bit
      scores(y, mul=None, add=None, ignore_nan=False, fair=False) -> EnsembleScores with rank histograms over total + 1 bins
                    and `absent`, the number of absent origins; one host sync
      events(spec)  -> spec.count(self): ScenarioEvents(counts, total)
      reduce(keep, on=None, scale=None, squared=False) -> the ScenarioSet of `keep` of the K members, by forward selection with
                    the counts as input probabilities (`ops.scenario_reduce_weighted`) on the distances between the kept paths,
                    or between their on= aggregates (reduce_scenarios' on / scale / squared); its S is this set's K, its index
                    and assign are positions among this set's members, its total this set's total
      merge(parts)  (static) the members of several sets of the same origins side by side, the totals added: two seeds, two
                    models, or chunks of an ensemble too large to hold -- merge(chunks).reduce(8) is a two-stage reduction;
                    cost NaN, no distances
      tree(stages, nodes, on=None, scale=None, squared=False) -> the ScenarioTree of the set's K members with the counts as
                    input probabilities (`scenario_tree`'s arguments): merge(chunks).tree(..) builds a
                    tree from an ensemble too large to hold; its S is this set's K, its total this set's
      envelope(coverage=0.9, on=None, target=None, calibrator=None, ignore_nan=False, return_depth=False) ->
                    `simultaneous_bands` of the set: the PathEnvelope of the kept paths with their counts as weights
      from_weights(paths, weights, total=65536)  (static, pure torch) user-supplied probabilities rounded to multiplicities
                    that sum to total by largest remainders (the lower index first among equal remainders); a row that is
                    negative, non-finite or all zero becomes an absent origin"""

    def __init__(self, index, counts, assign, cost, S, paths, distances=None, source=None, total=None):
        if index.dim() != 2 or index.dtype != torch.int64 or counts.dtype != torch.int32 or counts.shape != index.shape or \
                cost.shape != index.shape or assign.dim() != 2 or assign.shape[0] != index.shape[0] or \
                paths.dim() != 4 or paths.shape[:2] != index.shape:
            raise ValueError(f"ScenarioSet: index must be int64 [count, K] with int32 counts, cost [count, K], assign [count, S] "
                             f"and paths [count, K, H, N], got {index.dtype} {tuple(index.shape)}, {counts.dtype} "
                             f"{tuple(counts.shape)}, {tuple(cost.shape)}, {tuple(assign.shape)}, {tuple(paths.shape)}")
        self.index, self.counts, self.assign, self.cost, self.S, self.paths = index, counts, assign, cost, int(S), paths
        self.distances, self.source = distances, source
        self.count, self.K = int(index.shape[0]), int(index.shape[1])
        self.H, self.N = int(paths.shape[2]), int(paths.shape[3])
        if total is not None and (isinstance(total, bool) or int(total) != total or not 1 <= int(total) <= 2 ** 24):
            raise ValueError(f"ScenarioSet: total must be an integer within [1, 2^24], got {total!r}")
        self.total = self.S if total is None else int(total)
        self._parent = None                                                      # the set this one was reduced from (reduce)

    @property
    def weights(self):
        w = self.counts.double() / self.total
        return torch.where(self.index[:, :1] < 0, torch.full_like(w, float("nan")), w)

    def bands(self, quantiles, out=None):
        return ops.weighted_bands(self.paths, self.counts, self.total, quantiles, out)

    def scores(self, y, mul=None, add=None, ignore_nan=False, fair=False):
        return EnsembleScores._weighted(y, self.paths, self.counts, self.total, mul, add, ignore_nan=ignore_nan, fair=fair)

    def events(self, spec):
        if not isinstance(spec, EventSpec):
            raise ValueError(f"ScenarioSet.events: spec must be an EventSpec, got {type(spec).__name__}")
        return spec.count(self)

    def envelope(self, coverage=0.9, on=None, target=None, calibrator=None, ignore_nan=False, return_depth=False):
        return simultaneous_bands(self, coverage, on=on, target=target, calibrator=calibrator, ignore_nan=ignore_nan,
                                  return_depth=return_depth)

    def reduce(self, keep, on=None, scale=None, squared=False):
        if isinstance(on, EventSpec):
            if on.groups is None:
                raise ValueError("ScenarioSet.reduce: on= an EventSpec stands for its aggregate(paths); the spec has no groups=")
            on = on.aggregate(self.paths)
        elif on is None:
            on = self.paths
        else:
            on = _as_f32(on, like=self.paths)
            if on.dim() != 4 or tuple(on.shape[:3]) != (self.count, self.K, self.H):
                raise ops._lib.StemGNNHipError(f"ScenarioSet.reduce: on must be [count,K,H,R] with the set's count, K and H "
                                               f"{(self.count, self.K, self.H)}, got {tuple(on.shape)}")
        keep = ops._reduce_keep("ScenarioSet.reduce", keep, self.K)
        D = ops.scenario_distances(on.contiguous(), scale, squared)
        selected, counts, assign, cost = ops.scenario_reduce_weighted(D, self.counts, self.total, keep)
        index = selected.long()
        kept = torch.gather(self.paths, 1, index.clamp(min=0)[:, :, None, None].expand(-1, -1, self.H, self.N))
        kept = torch.where((index < 0)[:, :, None, None], torch.full_like(kept, float("nan")), kept)
        out = ScenarioSet(index, counts, assign, cost, self.K, kept, total=self.total)
        out._parent = self
        return out

    def tree(self, stages, nodes, on=None, scale=None, squared=False):
        on = _on_paths("ScenarioSet.tree", self.paths, on).contiguous()
        out = ops.scenario_tree(on, stages, nodes, scale, squared, mult=self.counts, total=self.total)
        return ScenarioTree._build(self.paths, ops._tree_stages("ScenarioSet.tree", stages, self.H),
                                   ops._tree_nodes("ScenarioSet.tree", nodes, len(tuple(stages)), self.K), out, self.total)

    @staticmethod
    def merge(parts):
        parts = list(parts)
        if not parts or any(not isinstance(p, ScenarioSet) or (p.count, p.H, p.N) != (parts[0].count, parts[0].H, parts[0].N)
                            for p in parts):
            raise ValueError("ScenarioSet.merge: the parts must be ScenarioSets of the same origins: one count, H and N")
        total = sum(p.total for p in parts)
        if total > 2 ** 24:
            raise ValueError(f"ScenarioSet.merge: the totals add up to {total}, beyond 2^24")
        index, assign, s0, k0 = [], [], 0, 0
        for p in parts:                                                          # indices among the joined S, positions among the joined K
            index.append(torch.where(p.index < 0, p.index, p.index + s0))
            assign.append(torch.where(p.assign < 0, p.assign, p.assign + k0))
            s0, k0 = s0 + p.S, k0 + p.K
        counts = torch.cat([p.counts for p in parts], dim=1)
        cost = torch.full(counts.shape, float("nan"), dtype=torch.float64, device=counts.device)
        return ScenarioSet(torch.cat(index, dim=1), counts, torch.cat(assign, dim=1), cost, s0,
                           torch.cat([p.paths for p in parts], dim=1), total=total)

    @staticmethod
    def from_weights(paths, weights, total=65536):
        paths = _as_f32(paths)
        if paths.dim() != 4:
            raise ValueError(f"ScenarioSet.from_weights: paths must be [count,K,H,N], got {tuple(paths.shape)}")
        if isinstance(total, bool) or int(total) != total or not 1 <= int(total) <= 2 ** 24:
            raise ValueError(f"ScenarioSet.from_weights: total must be an integer within [1, 2^24], got {total!r}")
        total = int(total)
        count, K = int(paths.shape[0]), int(paths.shape[1])
        w = weights if torch.is_tensor(weights) else torch.as_tensor(np.asarray(weights, dtype=np.float64))
        if tuple(w.shape) != (count, K) or w.is_complex():
            raise ValueError(f"ScenarioSet.from_weights: weights must be real and [count, K] = [{count}, {K}], got "
                             f"{tuple(w.shape)}")
        w = w.detach().to(device=paths.device, dtype=torch.float64)
        good = (torch.isfinite(w) & (w >= 0)).all(dim=1) & (w.sum(dim=1) > 0) & torch.isfinite(w.sum(dim=1))
        w = torch.where(good[:, None], w, torch.ones_like(w))
        q = w / w.sum(dim=1, keepdim=True) * total
        base = torch.floor(q)
        short = total - base.sum(dim=1, keepdim=True)                            # how many members are rounded up
        order = torch.sort(q - base, dim=1, descending=True, stable=True).indices   # the lower index first among equals
        place = torch.empty_like(order).scatter_(1, order, torch.arange(K, device=w.device).expand(count, K))
        counts = (base + (place < short).double()).to(torch.int32)
        counts = torch.where(good[:, None], counts, torch.zeros_like(counts))
        each = torch.arange(K, device=paths.device).expand(count, K)
        cost = torch.full((count, K), float("nan"), dtype=torch.float64, device=paths.device)
        return ScenarioSet(each.contiguous(), counts.contiguous(), each.to(torch.int32).contiguous(), cost, K, paths.contiguous(),
                           total=total)

    def expect(self, values):
        if not torch.is_tensor(values) or values.dim() < 2 or tuple(values.shape[:2]) != (self.count, self.S):
            raise ValueError(f"ScenarioSet.expect: values must be [count, S, ...] = [{self.count}, {self.S}, ...], got "
                             f"{tuple(values.shape) if torch.is_tensor(values) else type(values).__name__}")
        tail = values.shape[2:]
        idx = self.index.clamp(min=0).reshape(self.count, self.K, *([1] * len(tail))).expand(self.count, self.K, *tail)
        kept = torch.gather(values.double(), 1, idx)
        return (kept * self.weights.reshape(self.count, self.K, *([1] * len(tail)))).sum(dim=1)

    def keep_for(self, tol):
        ok = self.cost <= float(tol) * self.cost[:, :1]
        first = torch.arange(1, self.K + 1, device=ok.device).expand_as(ok)
        return torch.where(ok, first, torch.full_like(first, self.K)).amin(dim=1)

    def _distances(self, lo, hi):
        if self.distances is not None:
            return self.distances[lo:hi]
        on, scale, squared = self.source
        return ops.scenario_distances(on[lo:hi], scale, squared)

    def head(self, k):
        if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= self.K:
            raise ValueError(f"ScenarioSet.head: k must be an integer within [1, {self.K}], got {k!r}")
        if self._parent is not None:
            raise ValueError("ScenarioSet.head: this set was reduced from a weighted set, whose counts a head cannot re-derive; "
                             "forward selection is nested, so parent.reduce(k) is the same set")
        if self.distances is None and self.source is None:
            raise ValueError("ScenarioSet.head: counts and assign of the first k picks are re-derived from the distances: the "
                             "set needs `distances` ([count, S, S], ops.scenario_distances) or `source` (the full [count, S, H, R] "
                             "paths the distances were taken on, with scale and squared), and holds neither")
        k, S = int(k), self.S
        index = self.index[:, :k]
        refused = index[:, :1] < 0
        assign = torch.empty_like(self.assign)
        step = max(1, (256 << 20) // (S * S * 8))
        for lo in range(0, self.count, step):
            D = self._distances(lo, lo + step)                                   # [n, S, S]: D[k, u], path k onto path u
            cols = index[lo:lo + step].clamp(min=0)[:, None, :].expand(-1, S, -1)
            assign[lo:lo + step] = _first_min(torch.gather(D, 2, cols)).to(assign.dtype)
        assign = torch.where(refused, torch.full_like(assign, -1), assign)
        counts = (assign[:, :, None] == torch.arange(k, device=assign.device)).sum(dim=1).to(torch.int32)
        return ScenarioSet(index.contiguous(), counts, assign, self.cost[:, :k].contiguous(), S, self.paths[:, :k].contiguous(),
                           self.distances, self.source, total=self.total)

    @staticmethod
    def cat(parts):
        parts = list(parts)
        if not parts or any((p.S, p.K, p.H, p.N) != (parts[0].S, parts[0].K, parts[0].H, parts[0].N) for p in parts):
            raise ValueError("ScenarioSet.cat: the parts must share S, K, H and N")
        if any(p.total != parts[0].total for p in parts):
            raise ValueError("ScenarioSet.cat: the parts must share total")
        distances = torch.cat([p.distances for p in parts]) if all(p.distances is not None for p in parts) else None
        return ScenarioSet(*(torch.cat([getattr(p, name) for p in parts]) for name in ("index", "counts", "assign", "cost")),
                           parts[0].S, torch.cat([p.paths for p in parts]), distances, total=parts[0].total)


def reduce_scenarios(paths, keep, on=None, scale=None, squared=False):
    """Scenario reduction: of the S sampled paths of every origin (paths [count, S, H, N] float32 on the device,
    `trainer.rolling_scenarios(..., return_paths=True)`), the `keep` that represent the ensemble best, with probabilities -- what a
    stochastic program or a dispatcher can take where they cannot take S equally likely paths.  Forward selection (Heitsch &
    Roemisch 2003) on the Euclidean distance between whole trajectories (`ops.scenario_reduce`): each pick is the path that most
    lowers the Kantorovich distance between the ensemble and the kept set, and every dropped path's probability 1 / S goes to its
    nearest kept path, so the weights are integer counts over S.  Returns a ScenarioSet.
    on: the [count, S, H, R] float32 tensor the distances are taken on instead of `paths` -- typically
    `EventSpec.aggregate(paths)`, a reduction by corridor means whose kept members are still the full node paths; an EventSpec
    with groups= stands for its `aggregate(paths)`.  scale (a scalar, [R] or [H, R]; R = N without on=): multiplies every
    difference, e.g. 1 / std per column or a discount per step; squared: squared Euclidean distances."""
    paths = _as_f32(paths)
    if paths.dim() != 4:
        raise ops._lib.StemGNNHipError(f"reduce_scenarios: paths must be [count,S,H,N], got {tuple(paths.shape)}")
    on = _on_paths("reduce_scenarios", paths, on).contiguous()
    selected, counts, assign, cost = ops.scenario_reduce(on, keep, scale, squared)
    index = selected.long()
    C, S, H, N = paths.shape
    kept = torch.gather(paths, 1, index.clamp(min=0)[:, :, None, None].expand(-1, -1, H, N))
    kept = torch.where((index < 0)[:, :, None, None], torch.full_like(kept, float("nan")), kept)
    return ScenarioSet(index, counts, assign, cost, S, kept, source=(on, scale, bool(squared)))


def _take_paths(paths, index, lo, hi):
    """paths [count, S, H, N], index int64 [count, n] -> [count, n, hi - lo, N]: the steps [lo, hi) of the indexed paths, NaN
    where the index is negative"""
    n, N = index.shape[1], paths.shape[3]
    got = torch.gather(paths[:, :, lo:hi], 1, index.clamp(min=0)[:, :, None, None].expand(-1, n, hi - lo, N))
    return torch.where((index < 0)[:, :, None, None], torch.full_like(got, float("nan")), got)


class ScenarioTree:
    """A scenario tree per origin: the result of `scenario_tree` (staged forward selection, `ops.scenario_tree`; DESIGN.md
    section 5u).  Stage t = 0 .. T - 1 owns the steps [stages[t - 1], stages[t]) (from 0 for t = 0) and has nodes[t] nodes;
    every node is a sampled path's steps of that stage, a child of one node of the stage before, with an integer count.  The
    members of a node share its ancestors' steps: what a multi-stage program needs (non-anticipativity).  Device tensors, no
    sync, the node axis padded to n = nodes[-1]:
      node_index int64 [count, T, n]  the path each node is represented by (-1: padding, a refused origin, an empty node)
      parent     int32 [count, T, n]  the node's parent among the nodes of stage t - 1 (0 at t = 0; -1: padding, refused)
      counts     int32 [count, T, n]  the multiplicities the node gathers; at every stage they add up to `total`
      assign     int32 [count, T, S]  the node of stage t every path went to        cost  float64 [count, T]  the Kantorovich
                                      distance between the ensemble and the stage's nodes, in the stage's prefix metric
      paths      float32 [count, n, H, N]  the LEAVES' trajectories: leaf j's steps of stage t are those of the representative of
                                      its ancestor at that stage      S, total  the ensemble's size and the multiplicities' sum
    A refused origin: -1 / -1 / 0 / -1 / NaN and NaN trajectories.
      scenarios()      -> the ScenarioSet of the leaves with counts[:, T - 1] and total: bands, scores, events,
                          EventSpec.count and trainer.score_forecast(paths=) take a tree through it
      values(t)        -> float32 [count, nodes[t], stages[t] - stages[t - 1], N], the nodes' own steps
      probabilities(t) -> float64 [count, nodes[t]] = counts / total      conditional(t) -> counts / the parent's count
      expect(values [count, S, ...]) -> float64 [count, ...], the leaf-weighted mean, as ScenarioSet.expect
      cat(parts)       joins batches along the origins
      export(c)        -> one origin on the host as a plain dict: stages, nodes, total, and per stage the lists parent,
                          probability, conditional, values (numpy arrays): the node list tree-based solvers read; one sync"""

    def __init__(self, stages, nodes, node_index, parent, counts, assign, cost, S, total, stage_values, paths):
        stages, nodes = tuple(int(v) for v in stages), tuple(int(v) for v in nodes)
        T, n = len(stages), nodes[-1]
        if len(nodes) != T or node_index.dtype != torch.int64 or node_index.dim() != 3 or \
                tuple(node_index.shape[1:]) != (T, n) or parent.shape != node_index.shape or counts.shape != node_index.shape or \
                counts.dtype != torch.int32 or assign.dim() != 3 or tuple(assign.shape[:2]) != tuple(node_index.shape[:2]) or \
                tuple(cost.shape) != tuple(node_index.shape[:2]) or len(stage_values) != T or paths.dim() != 4 or \
                tuple(paths.shape[:3]) != (node_index.shape[0], n, stages[-1]):
            raise ValueError(f"ScenarioTree: node_index must be int64 [count, T, n_T] with int32 parent and counts, assign "
                             f"[count, T, S], cost [count, T], T stage values and paths [count, n_T, H, N]; got "
                             f"{node_index.dtype} {tuple(node_index.shape)}, {tuple(parent.shape)}, {counts.dtype} "
                             f"{tuple(counts.shape)}, {tuple(assign.shape)}, {tuple(cost.shape)}, {len(stage_values)}, "
                             f"{tuple(paths.shape)} at stages {stages}, nodes {nodes}")
        self.stages, self.nodes, self.T = stages, nodes, T
        self.node_index, self.parent, self.counts, self.assign, self.cost = node_index, parent, counts, assign, cost
        self.S, self.total, self.paths = int(S), int(total), paths
        self._values = list(stage_values)
        self.count, self.H, self.N = int(node_index.shape[0]), stages[-1], int(paths.shape[3])

    @staticmethod
    def _build(paths, stages, nodes, out, total):
        """the tree of ops.scenario_tree's outputs `out` on paths [count, S, H, N]: gathers, no kernel"""
        node_path, node_parent, node_count, assign, cost = out
        T, S = len(stages), int(paths.shape[1])
        index = node_path.long()
        lo = (0,) + tuple(stages[:-1])
        values = [_take_paths(paths, index[:, t, :nodes[t]], lo[t], stages[t]) for t in range(T)]
        leaf = index[:, T - 1]                                                   # [count, n]
        parts = []
        for t in range(T):                                                       # the ancestor of every leaf at stage t, its path
            anc = torch.gather(assign[:, t].long(), 1, leaf.clamp(min=0))
            rep = torch.gather(index[:, t], 1, anc.clamp(min=0))
            rep = torch.where((leaf < 0) | (anc < 0), torch.full_like(rep, -1), rep)
            parts.append(_take_paths(paths, rep, lo[t], stages[t]))
        return ScenarioTree(stages, nodes, index, node_parent, node_count, assign, cost, S, total, values,
                            torch.cat(parts, dim=2).contiguous())

    def _stage(self, who, t):
        if isinstance(t, bool) or int(t) != t or not 0 <= int(t) < self.T:
            raise ValueError(f"ScenarioTree.{who}: t must be a stage within [0, {self.T - 1}], got {t!r}")
        return int(t)

    def scenarios(self):
        last = self.T - 1
        cost = torch.full((self.count, self.nodes[-1]), float("nan"), dtype=torch.float64, device=self.cost.device)
        cost[:, -1] = self.cost[:, last]
        return ScenarioSet(self.node_index[:, last].contiguous(), self.counts[:, last].contiguous(),
                           self.assign[:, last].contiguous(), cost, self.S, self.paths, total=self.total)

    def values(self, t):
        return self._values[self._stage("values", t)]

    def probabilities(self, t):
        t = self._stage("probabilities", t)
        p = self.counts[:, t, :self.nodes[t]].double() / self.total
        return torch.where(self.parent[:, t, :1] < 0, torch.full_like(p, float("nan")), p)

    def conditional(self, t):
        t = self._stage("conditional", t)
        own = self.counts[:, t, :self.nodes[t]].double()
        if t == 0:
            above = torch.full_like(own, float(self.total))
        else:
            above = torch.gather(self.counts[:, t - 1].double(), 1, self.parent[:, t, :self.nodes[t]].long().clamp(min=0))
        return torch.where(self.parent[:, t, :1] < 0, torch.full_like(own, float("nan")), own / above)

    def expect(self, values):
        return self.scenarios().expect(values)

    @staticmethod
    def cat(parts):
        parts = list(parts)
        if not parts or any(not isinstance(p, ScenarioTree) or
                            (p.stages, p.nodes, p.S, p.total, p.N) != (parts[0].stages, parts[0].nodes, parts[0].S,
                                                                       parts[0].total, parts[0].N) for p in parts):
            raise ValueError("ScenarioTree.cat: the parts must be ScenarioTrees that share stages, nodes, S, total and N")
        a = parts[0]
        return ScenarioTree(a.stages, a.nodes,
                            *(torch.cat([getattr(p, name) for p in parts]) for name in ("node_index", "parent", "counts",
                                                                                        "assign", "cost")),
                            a.S, a.total, [torch.cat([p._values[t] for p in parts]) for t in range(a.T)],
                            torch.cat([p.paths for p in parts]))

    def export(self, c):
        if isinstance(c, bool) or int(c) != c or not 0 <= int(c) < self.count:
            raise ValueError(f"ScenarioTree.export: c must be an origin within [0, {self.count - 1}], got {c!r}")
        c = int(c)
        out = dict(stages=self.stages, nodes=self.nodes, total=self.total, parent=[], probability=[], conditional=[], values=[])
        for t in range(self.T):
            out["parent"].append(self.parent[c, t, :self.nodes[t]].cpu().numpy())
            out["probability"].append(self.probabilities(t)[c].cpu().numpy())
            out["conditional"].append(self.conditional(t)[c].cpu().numpy())
            out["values"].append(self._values[t][c].cpu().numpy())
        return out


def _on_paths(who, paths, on):
    """the tensor the distances are taken on (on= of reduce_scenarios and scenario_tree): the paths, a [count,S,H,R] tensor, or
    an EventSpec with groups= standing for its aggregate of the paths"""
    if isinstance(on, EventSpec):
        if on.groups is None:
            raise ValueError(f"{who}: on= an EventSpec stands for its aggregate(paths); the spec has no groups=")
        return on.aggregate(paths)
    if on is None:
        return paths
    on = _as_f32(on, like=paths)
    if on.dim() != 4 or tuple(on.shape[:3]) != tuple(paths.shape[:3]):
        raise ops._lib.StemGNNHipError(f"{who}: on must be [count,S,H,R] with the paths' count, S and H "
                                       f"{tuple(paths.shape[:3])}, got {tuple(on.shape)}")
    return on


def scenario_tree(paths, stages, nodes, on=None, scale=None, squared=False):
    """A scenario tree of the S sampled paths of every origin (paths [count, S, H, N] float32 on the device): where
    `reduce_scenarios` returns a fan -- K members that differ from the first step on, valid for two-stage decisions only --
    the tree's members share their history up to a stage and branch afterwards, with conditional probabilities on the
    branches: what dispatch, signal plans and rerouting, which decide again every few steps, need.  Forward tree construction
    (Heitsch & Roemisch 2009; `ops.scenario_tree`): stage t, the steps [stages[t - 1], stages[t]), keeps nodes[t] paths; first
    one child for every node of the stage before, then the rest where they most lower the Kantorovich distance in the metric of
    the steps before stages[t]; a path only ever moves to a node of its own parent.  stages: strictly increasing step bounds
    that end at H; nodes: non-decreasing counts within [1, S].  on / scale / squared: reduce_scenarios'.  Returns a
    ScenarioTree; with one stage its leaves are `reduce_scenarios(paths, nodes[0])`."""
    paths = _as_f32(paths)
    if paths.dim() != 4:
        raise ops._lib.StemGNNHipError(f"scenario_tree: paths must be [count,S,H,N], got {tuple(paths.shape)}")
    on = _on_paths("scenario_tree", paths, on).contiguous()
    out = ops.scenario_tree(on, stages, nodes, scale, squared)
    return ScenarioTree._build(paths, ops._tree_stages("scenario_tree", stages, int(paths.shape[2])),
                               ops._tree_nodes("scenario_tree", nodes, len(tuple(stages)), int(paths.shape[1])), out,
                               int(paths.shape[1]))


class PathEnvelope:
    """A simultaneous band of sampled paths: the result of `simultaneous_bands` (`ops.scenario_envelope`).
    Where every other band of the library covers the target step by step, this one is sized so that the WHOLE trajectory of a
    column stays inside it.  Device tensors, no sync:
      bands      float32 [count, 2, H, C]  lower and upper: center -+ multiplier * scale
      center     float64 [count, H, C]     the paths' (weighted) mean per step      scale  float64 [count, H, C] their deviation
      chosen     float64 [count, C]        the multiplier that holds `coverage` of the ensemble's own whole paths
      multiplier float64                   the one in use: `chosen`, or a calibrator's [1] or [C]
      truth      float64 [count, C]        the target's depth max_h |y - center| / scale, or None without a target
      depth      float64 [count, S, C]     every path's depth, on request, else None
      inside     bool [count, C]           truth <= multiplier: the band holds the whole target; False where absent (NaN)
    joint_coverage() -> (overall, per column [C]) over the pairs with a truth, one sync;  width() -> float64 [H] on the
    device, the mean upper - lower per step;  cat(parts) joins batches along the origins."""

    def __init__(self, bands, moments, chosen, multiplier, truth=None, depth=None, coverage=None):
        if bands.dim() != 4 or bands.shape[1] != 2 or moments.shape != bands.shape or \
                tuple(chosen.shape) != (bands.shape[0], bands.shape[3]):
            raise ValueError(f"PathEnvelope: bands and moments must be [count, 2, H, C] with chosen [count, C], got "
                             f"{tuple(bands.shape)}, {tuple(moments.shape)}, {tuple(chosen.shape)}")
        self.bands, self.moments, self.chosen, self.multiplier = bands, moments, chosen, multiplier
        self.truth, self.depth, self.coverage = truth, depth, coverage
        self.count, self.H, self.C = int(bands.shape[0]), int(bands.shape[2]), int(bands.shape[3])

    @property
    def center(self):
        return self.moments[:, 0]

    @property
    def scale(self):
        return self.moments[:, 1]

    @property
    def inside(self):
        if self.truth is None:
            raise ValueError("PathEnvelope.inside: the envelope was made without a target")
        return self.truth <= self.multiplier

    def joint_coverage(self):
        inside = self.inside
        valid = ~torch.isnan(self.truth)
        hit = (inside & valid).sum(dim=0).double()
        n = valid.sum(dim=0).double()
        both = torch.stack([hit, n]).cpu().numpy()                               # the one sync
        with np.errstate(divide="ignore", invalid="ignore"):
            return float(both[0].sum() / both[1].sum()), both[0] / both[1]

    def width(self):
        w = self.bands[:, 1].double() - self.bands[:, 0].double()
        return torch.nanmean(w.transpose(0, 1).reshape(self.H, -1), dim=1)

    @staticmethod
    def cat(parts):
        parts = list(parts)
        if not parts or any(not isinstance(p, PathEnvelope) or (p.H, p.C) != (parts[0].H, parts[0].C) for p in parts):
            raise ValueError("PathEnvelope.cat: the parts must be PathEnvelopes that share H and C")
        first = parts[0]
        if any((p.truth is None) != (first.truth is None) or (p.depth is None) != (first.depth is None) or
               p.multiplier.dim() != first.multiplier.dim() for p in parts):
            raise ValueError("PathEnvelope.cat: the parts must all have, or all lack, truth, depth and a calibrator's multiplier")
        if first.depth is not None and any(p.depth.shape[1] != first.depth.shape[1] for p in parts):
            raise ValueError("PathEnvelope.cat: the parts must share S")

        def join(name):
            return None if getattr(first, name) is None else torch.cat([getattr(p, name) for p in parts])

        multiplier = join("multiplier") if first.multiplier.dim() == 2 else first.multiplier
        return PathEnvelope(join("bands"), join("moments"), join("chosen"), multiplier, join("truth"), join("depth"),
                            first.coverage)


class EnvelopeCalibrator:
    """Split-conformal calibration of the simultaneous band's multiplier: what gives "the whole trajectory stays inside with
    probability `coverage`" its guarantee (the ensemble's own multiplier only holds that share of its own paths).
    fit(envelope_or_truth, ignore_nan=True): the held-out truth depths (a PathEnvelope made with target=, or its `truth`
    [count, C]), pooled or, with per_column, column by column; the multiplier is the k-th smallest of the m depths that are not
    NaN, k = ceil((m + 1) coverage (1 - 1e-12)), +inf when k > m.  ignore_nan=False: a NaN depth makes its group's multiplier
    NaN.  torch.sort on the tensor's own device, no sync.  multiplier: float64 [1] or [C]; counts: int64, the m of every group.
    Passed as calibrator= to simultaneous_bands (ScenarioSet.envelope, trainer.scenario_envelopes, LiveForecaster.envelope),
    its multiplier replaces the ensemble's own.  On exchangeable fresh origins the band then holds the whole trajectory with
    probability at least `coverage`."""

    def __init__(self, coverage=0.9, per_column=False):
        if isinstance(coverage, bool) or not isinstance(coverage, (int, float, np.floating)) or not 0.0 < float(coverage) < 1.0:
            raise ValueError(f"EnvelopeCalibrator: coverage must be a number inside (0, 1), got {coverage!r}")
        self.coverage, self.per_column = float(coverage), bool(per_column)
        self.multiplier = self.counts = None

    def fit(self, envelope_or_truth, ignore_nan=True):
        truth = envelope_or_truth.truth if isinstance(envelope_or_truth, PathEnvelope) else envelope_or_truth
        if not torch.is_tensor(truth) or truth.dim() != 2:
            raise ValueError("EnvelopeCalibrator.fit: a PathEnvelope made with target=, or its truth [count, C], is needed, got "
                             f"{tuple(truth.shape) if torch.is_tensor(truth) else type(truth).__name__}")
        d = truth.detach().double()
        d = d.transpose(0, 1) if self.per_column else d.reshape(1, -1)           # [groups, n]
        nan = torch.isnan(d)
        m = (~nan).sum(dim=1)
        n = d.shape[1]
        if n == 0:
            q = torch.full((d.shape[0],), float("inf"), dtype=torch.float64, device=d.device)
        else:
            ordered = torch.sort(d, dim=1).values                                # NaN last
            k = torch.ceil(((m + 1).double() * self.coverage) * (1.0 - 1e-12)).clamp(min=1.0).long()
            q = torch.gather(ordered, 1, (k - 1).clamp(max=n - 1)[:, None])[:, 0]
            q = torch.where(k > m, torch.full_like(q, float("inf")), q)
            if not ignore_nan:
                q = torch.where(nan.any(dim=1), torch.full_like(q, float("nan")), q)
        self.multiplier, self.counts = q.contiguous(), m
        return self

    def state_dict(self):
        return dict(coverage=self.coverage, per_column=self.per_column, multiplier=self.multiplier, counts=self.counts)

    def load_state_dict(self, state, device=None):
        if float(state["coverage"]) != self.coverage or bool(state["per_column"]) != self.per_column:
            raise ValueError(f"EnvelopeCalibrator.load_state_dict: saved for coverage {state['coverage']}, "
                             f"per_column={state['per_column']}; this one has {self.coverage}, {self.per_column}")
        multiplier, counts = state["multiplier"], state["counts"]
        if multiplier is not None:
            if multiplier.dim() != 1 or counts.shape != multiplier.shape or (not self.per_column and multiplier.shape[0] != 1):
                raise ValueError(f"EnvelopeCalibrator.load_state_dict: multiplier {tuple(multiplier.shape)} / counts "
                                 f"{tuple(counts.shape)} do not fit per_column={self.per_column}")
            if device is not None:
                multiplier, counts = multiplier.to(device), counts.to(device)
            multiplier, counts = multiplier.double().contiguous(), counts.long().contiguous()
        self.multiplier, self.counts = multiplier, counts
        return self

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(state["coverage"], state["per_column"]).load_state_dict(state, device)


def simultaneous_bands(paths, coverage=0.9, on=None, target=None, calibrator=None, ignore_nan=False, return_depth=False):
    """The band that holds whole trajectories (`ops.scenario_envelope`): per origin and column, the
    paths' mean and deviation per step and ONE multiplier for all steps, center -+ multiplier * scale.  Returns a PathEnvelope.
    paths: [count, S, H, N] float32 on the device (rolling_scenarios(..., return_paths=True)), or a ScenarioSet, whose kept
    paths enter with their counts as weights.  coverage: the share of the ensemble's own whole paths the band holds (`chosen`).
    target [count, H, N]: what happened; the envelope's `truth` and `inside` say whether the band held it, and `truth` is what
    EnvelopeCalibrator.fit takes.  calibrator (a fitted EnvelopeCalibrator): its multiplier is used instead of the ensemble's.
    on: an EventSpec with groups=, whose aggregate of the paths AND of the target the band is made for (corridor means), or a
    [count, S, H, R] tensor standing for the paths (the target is then [count, H, R])."""
    mult = total = None
    if isinstance(paths, ScenarioSet):
        mult, total, paths = paths.counts, paths.total, paths.paths
    paths = _as_f32(paths)
    if paths.dim() != 4:
        raise ops._lib.StemGNNHipError(f"simultaneous_bands: paths must be [count,S,H,N], got {tuple(paths.shape)}")
    if target is not None:
        target = _as_f32(target, like=paths)
        if isinstance(on, EventSpec) and on.groups is not None:
            target = on.aggregate(target)
    on = _on_paths("simultaneous_bands", paths, on).contiguous()
    multiplier = None
    if calibrator is not None:
        if not isinstance(calibrator, EnvelopeCalibrator) or calibrator.multiplier is None:
            raise ValueError("simultaneous_bands: calibrator= takes a fitted EnvelopeCalibrator")
        if calibrator.per_column and calibrator.multiplier.shape[0] != on.shape[3]:
            raise ValueError(f"simultaneous_bands: the calibrator was fitted per column on {calibrator.multiplier.shape[0]} "
                             f"columns, the paths have {on.shape[3]}")
        multiplier = calibrator.multiplier
    out = ops.scenario_envelope(on, coverage, None if target is None else target.contiguous(), mult, total, multiplier,
                                ignore_nan, return_depth)
    in_use = out["chosen"] if multiplier is None else multiplier.to(device=on.device, dtype=torch.float64)
    return PathEnvelope(out["bands"], out["moments"], out["chosen"], in_use, out["truth"], out["depth"], float(coverage))


def joint_coverage(y, lo, hi, ignore_nan=False):
    """The share of (origin, column) pairs whose whole trajectory y [count, H, N] lies inside the band lo .. hi (both
    [count, H, N]): what any band, pointwise ones included, is worth to a plan that assumes all steps hold at once.  A torch
    composition; returns a float (one sync).  ignore_nan: NaN steps of y are skipped and a pair without a step is left out;
    otherwise a NaN step counts as outside."""
    y = y.double()
    held = (y >= lo.double()) & (y <= hi.double())
    if ignore_nan:
        missing = torch.isnan(y)
        held, valid = (held | missing).all(dim=1), ~missing.all(dim=1)
    else:
        held = held.all(dim=1)
        valid = torch.ones_like(held)
    both = torch.stack([(held & valid).sum(), valid.sum()]).cpu()
    return float(both[0]) / float(both[1]) if int(both[1]) else float("nan")


class GaussianCopula:
    """The dependence BETWEEN NODES of sampled scenario paths: a Gaussian copula over the model's own marginals, on the device.

    `coupling="independent"` and `coupling="path"` are the two ends of the range; a network's residuals are correlated in blocks.
    Here the uniforms that drive the draws of one (path, step) row are u = Phi(L e), e i.i.d. standard normal and L L^T = R a
    correlation matrix over the nodes, so every node keeps exactly the predicted quantile function as its marginal and only the
    joint behaviour changes.  Pass the fitted object as `coupling=` to trainer.rolling_scenarios / LiveForecaster.scenarios;
    `EnsembleScores.energy` is the score that ranks it against the two strings.

    fit(y, y_hat): y [count, H, N] held-out ground truth, y_hat [count, Q, H, N], normalised units, as a validation pass leaves
    them at the model's own horizon (`trainer.rolling_forecast(model, loader, model.horizon)`); all H steps are pooled.
      u = pit(y, y_hat)                 the transform of each target under its forecast (`ops.copula_pit`), NaN = missing
      pairs, sums = ops.copula_gram(u)  pairwise-complete moments of z = Phi^-1(u), fp64, m_ij = pairs
      mean_i|j = a_ij / m_ij,  cov_ij = s_ij / m_ij - mean_i|j mean_j|i,  var_i|j = q_ij / m_ij - mean_i|j^2
      R_ij = cov_ij / sqrt(var_i|j var_j|i), 0 where m_ij < min_pairs or a variance is not positive; unit diagonal; (R + R^T) / 2
      correlation = (1 - shrinkage) R + shrinkage I
    elementwise in fp64 on the device; the Cholesky factor of that one N x N matrix is taken on the host in fp64 (a ValueError
    names the smallest eigenvalue when it fails: pairwise-complete estimates need not be positive definite, a larger shrinkage
    makes them so), cast to fp32, transposed and copied to the device.
    from_correlation(R, quantiles, tails): a prior matrix instead of a fit, validated once on the host.
    pit(y, y_hat) -> u [count, H, N]: its histogram per node is a calibration diagnostic in its own right (flat when calibrated).
    uniforms(Bo, S, L, step, horizon, origin0, seed, offset=0) -> u [Bo, S, L, N] (`ops.copula_uniforms`), what
    `ops.scenario_roll(..., uniforms=u)` takes; a draw is named by global origin, path, step and node as for "independent".
    tails must be the `tails=` of the scenario call: the transform of the fit and the draw are inverses only then.
    Attributes: correlation (fp64 [N, N], device, the shrunk matrix), correlation_raw, pairs (int64 [N, N]; None from a prior),
    factor_t (fp32 [N, N], factor_t[k, n] = L[n, k]), nodes."""

    def __init__(self, quantiles, shrinkage=0.05, tails="linear", min_pairs=8):
        q = tuple(float(t) for t in quantiles)
        if len(q) < 2 or not all(0.0 < a < b < 1.0 for a, b in zip(q, q[1:])):
            raise ValueError(f"GaussianCopula: at least two levels, strictly increasing inside (0, 1), are needed; got {q}")
        if not 0.0 <= float(shrinkage) <= 1.0:
            raise ValueError(f"GaussianCopula: shrinkage must be within [0, 1], got {shrinkage}")
        if tails not in ("linear", "clamp"):
            raise ValueError(f"GaussianCopula: tails must be 'linear' or 'clamp', got {tails!r}")
        if int(min_pairs) < 2:
            raise ValueError(f"GaussianCopula: min_pairs must be at least 2 (a variance needs two rows), got {min_pairs}")
        self.quantiles, self.shrinkage, self.tails, self.min_pairs = q, float(shrinkage), tails, int(min_pairs)
        self.correlation = self.correlation_raw = self.pairs = self.factor_t = self.nodes = None

    def pit(self, y, y_hat):
        y_hat = _as_f32(y_hat)
        y = _as_f32(y, like=y_hat)
        if y_hat.dim() != 4 or y_hat.shape[1] != len(self.quantiles):
            raise ValueError(f"GaussianCopula.pit: y_hat must be [count, {len(self.quantiles)}, H, N], got {tuple(y_hat.shape)}")
        return ops.copula_pit(y.contiguous(), y_hat.contiguous(), self.quantiles, self.tails)

    def fit(self, y, y_hat):
        shrunk, R, pairs, factor = self._estimate(self.pit(y, y_hat), self.shrinkage, "GaussianCopula.fit")
        self._take(shrunk, R, pairs, factor, R.device)
        return self

    def _estimate(self, u, shrinkage, who):
        """(shrunk, raw, pairs, fp64 host factor) over the columns of u [.., K]: the estimator of the class docstring"""
        pairs, (s, a, q) = ops.copula_gram(u)
        m = pairs.double()
        mean = a / m                                                    # mean_i|j; its transpose is mean_j|i (m is symmetric)
        var = q / m - mean * mean
        R = (s / m - mean * mean.T) / torch.sqrt(var * var.T)
        R = torch.where((pairs < self.min_pairs) | ~(var > 0) | ~(var.T > 0), torch.zeros_like(R), R)
        R.fill_diagonal_(1.0)
        R = (R + R.T) / 2
        eye = torch.eye(R.shape[0], dtype=R.dtype, device=R.device)
        shrunk = (1.0 - shrinkage) * R + shrinkage * eye
        return shrunk, R, pairs, self._factor(shrunk.cpu().numpy(), who)

    @staticmethod
    def _factor(R, who):
        """The lower Cholesky factor of the host matrix R in fp64, or the ValueError that says why there is none."""
        if not np.isfinite(R).all():
            raise ValueError(f"{who}: the correlation matrix has entries that are not finite")
        try:
            return np.linalg.cholesky(R)
        except np.linalg.LinAlgError:
            low = float(np.linalg.eigvalsh((R + R.T) / 2).min())
            raise ValueError(f"{who}: the correlation matrix is not positive definite (smallest eigenvalue {low:.3e}); a larger "
                             "shrinkage is needed") from None

    def _take(self, correlation, raw, pairs, factor, device):
        self.correlation, self.correlation_raw, self.pairs = correlation, raw, pairs
        self.factor_t = torch.from_numpy(np.ascontiguousarray(factor.astype(np.float32).T)).to(device)
        self.nodes = int(factor.shape[0])

    @classmethod
    def from_correlation(cls, R, quantiles, tails="linear", device=None):
        """A copula from a prior correlation matrix (numpy or tensor): square, finite, symmetric and of unit diagonal to 1e-6,
        positive definite.  device: where factor_t goes (default: R's when it is a device tensor, else the current HIP device)."""
        R, factor, device = cls._prior(R, "GaussianCopula.from_correlation", device)
        self = cls(quantiles, shrinkage=0.0, tails=tails)
        dev_R = torch.from_numpy(R.copy()).to(device)
        self._take(dev_R, dev_R.clone(), None, factor, device)
        return self

    @classmethod
    def _prior(cls, R, who, device):
        """A prior correlation matrix validated on the host -> (fp64 numpy matrix, its fp64 factor, the device to use)"""
        if torch.is_tensor(R):
            device = R.device if device is None and R.is_cuda else device
            R = R.detach().cpu().numpy()
        R = np.asarray(R, dtype=np.float64)
        if R.ndim != 2 or R.shape[0] != R.shape[1] or R.shape[0] < 1:
            raise ValueError(f"{who}: a square matrix is needed, got shape {R.shape}")
        if not np.isfinite(R).all():
            raise ValueError(f"{who}: the matrix has entries that are not finite")
        if np.abs(R - R.T).max() > 1e-6:
            raise ValueError(f"{who}: the matrix is not symmetric (max |R - R^T| = {np.abs(R - R.T).max():.3e})")
        if np.abs(np.diag(R) - 1.0).max() > 1e-6:
            raise ValueError(f"{who}: the diagonal is not 1 (max |R_ii - 1| = {np.abs(np.diag(R) - 1.0).max():.3e})")
        factor = cls._factor(R, who)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        return R, factor, device

    def uniforms(self, Bo, S, L, step, horizon, origin0, seed, offset=0):
        if self.factor_t is None:
            raise ValueError("GaussianCopula.uniforms: not fitted (call fit, from_correlation or load_state_dict first)")
        return ops.copula_uniforms(self.factor_t, Bo, S, L, step, horizon, origin0=origin0, seed=seed, offset=offset)

    def state_dict(self):
        return dict(quantiles=self.quantiles, shrinkage=self.shrinkage, tails=self.tails, min_pairs=self.min_pairs,
                    nodes=self.nodes, correlation=self.correlation, correlation_raw=self.correlation_raw, pairs=self.pairs,
                    factor_t=self.factor_t)

    def load_state_dict(self, state, device=None):
        if "step_factor" in state:
            raise ValueError("GaussianCopula.load_state_dict: the state was saved by a SpaceTimeCopula (it holds step_factor); "
                             "loading it here would drop the step coupling")
        q = tuple(float(t) for t in state["quantiles"])
        if q != self.quantiles or state["tails"] != self.tails:
            raise ValueError(f"GaussianCopula.load_state_dict: saved for levels {q}, tails={state['tails']!r}; this one has "
                             f"{self.quantiles}, {self.tails!r}")
        f = state["factor_t"]
        if f is not None and (f.dim() != 2 or f.shape[0] != f.shape[1] or tuple(state["correlation"].shape) != tuple(f.shape)):
            raise ValueError(f"GaussianCopula.load_state_dict: factor_t {tuple(f.shape)} / correlation "
                             f"{tuple(state['correlation'].shape)} are not one square shape")

        def put(t, dtype):
            if t is None:
                return None
            return t.detach().to(device=t.device if device is None else device, dtype=dtype).contiguous().clone()

        self.correlation, self.correlation_raw = put(state["correlation"], torch.float64), put(state["correlation_raw"], torch.float64)
        self.pairs, self.factor_t = put(state["pairs"], torch.int64), put(f, torch.float32)
        self.nodes = None if f is None else int(f.shape[0])
        return self

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(state["quantiles"], state["shrinkage"], state["tails"], state["min_pairs"]).load_state_dict(state, device)


class SpaceTimeCopula(GaussianCopula):
    """The dependence between nodes AND between the steps of one round: a separable Gaussian copula over (step, node).

    `GaussianCopula` couples the nodes of one (path, step) row; the H = model.horizon steps a path draws in one round are still
    independent of one another, although real h-step errors from one origin are strongly correlated.  Here the normal scores of
    one round of one path have correlation T[j, j'] * R[n, n']: R the node matrix of `GaussianCopula`, T an H x H matrix over the
    steps.  Every (step, node) keeps exactly the predicted marginal.  Between rounds the dependence stays what the roll creates
    (the next round is conditioned on the drawn window).  It goes wherever a `GaussianCopula` goes as `coupling=`;
    `path_energy_score` is the score that ranks it (CRPS and the per-step `EnsembleScores.energy` do not see steps).

    fit(y, y_hat): the node part is `GaussianCopula.fit`'s, bit for bit.  The step part takes the same u = pit(y, y_hat)
    [count, H, N] with rows (origin, node) and columns h -- `ops.copula_gram(u.transpose(1, 2))` -- through the same
    elementwise estimator; step_correlation = (1 - step_shrinkage) T + step_shrinkage I, its fp64 Cholesky factor taken on the
    host and cast to fp32 as step_factor [H, H].
    from_correlations(R, T, quantiles, tails): prior matrices instead of a fit, both validated on the host.
    uniforms(Bo, S, L, ...): L <= steps; the leading L x L block of step_factor (the factor of T's leading block) goes to
    `ops.copula_uniforms(..., step_factor=)`.
    New attributes: step_correlation (fp64 [H, H], device), step_correlation_raw, step_pairs (int64; None from a prior),
    step_factor (fp32 [H, H], lower triangular), steps (= H)."""

    def __init__(self, quantiles, shrinkage=0.05, step_shrinkage=0.0, tails="linear", min_pairs=8):
        super().__init__(quantiles, shrinkage=shrinkage, tails=tails, min_pairs=min_pairs)
        if not 0.0 <= float(step_shrinkage) <= 1.0:
            raise ValueError(f"SpaceTimeCopula: step_shrinkage must be within [0, 1], got {step_shrinkage}")
        self.step_shrinkage = float(step_shrinkage)
        self.step_correlation = self.step_correlation_raw = self.step_pairs = self.step_factor = self.steps = None
        self._blocks = {}

    def fit(self, y, y_hat):
        u = self.pit(y, y_hat)
        shrunk, R, pairs, factor = self._estimate(u, self.shrinkage, "SpaceTimeCopula.fit")
        steps = self._estimate(u.transpose(1, 2).contiguous(), self.step_shrinkage, "SpaceTimeCopula.fit, the step matrix")
        self._take(shrunk, R, pairs, factor, R.device)
        self._take_steps(*steps, R.device)
        return self

    def _take_steps(self, correlation, raw, pairs, factor, device):
        self.step_correlation, self.step_correlation_raw, self.step_pairs = correlation, raw, pairs
        self.step_factor = torch.from_numpy(np.ascontiguousarray(factor.astype(np.float32))).to(device)
        self.steps = int(factor.shape[0])
        self._blocks = {}

    @classmethod
    def from_correlation(cls, R, quantiles, tails="linear", device=None):
        raise TypeError("SpaceTimeCopula.from_correlation: a step matrix is needed too; call from_correlations(R, T, ...)")

    @classmethod
    def from_correlations(cls, R, T, quantiles, tails="linear", device=None):
        """A copula from prior matrices (numpy or tensor): R over the nodes, T over the steps, each square, finite, symmetric
        and of unit diagonal to 1e-6, positive definite.  device: as for `GaussianCopula.from_correlation`."""
        R, factor, device = cls._prior(R, "SpaceTimeCopula.from_correlations", device)
        T, step_factor, _ = cls._prior(T, "SpaceTimeCopula.from_correlations, the step matrix", device)
        self = cls(quantiles, shrinkage=0.0, step_shrinkage=0.0, tails=tails)
        dev_R, dev_T = torch.from_numpy(R.copy()).to(device), torch.from_numpy(T.copy()).to(device)
        self._take(dev_R, dev_R.clone(), None, factor, device)
        self._take_steps(dev_T, dev_T.clone(), None, step_factor, device)
        return self

    def uniforms(self, Bo, S, L, step, horizon, origin0, seed, offset=0):
        if self.factor_t is None or self.step_factor is None:
            raise ValueError("SpaceTimeCopula.uniforms: not fitted (call fit, from_correlations or load_state_dict first)")
        L = int(L)
        if not 1 <= L <= self.steps:
            raise ValueError(f"SpaceTimeCopula.uniforms: {L} steps in a round, the copula couples {self.steps}")
        block = self._blocks.get(L)
        if block is None:                                               # the factor of T's leading block
            block = self._blocks[L] = self.step_factor[:L, :L].contiguous()
        return ops.copula_uniforms(self.factor_t, Bo, S, L, step, horizon, origin0=origin0, seed=seed, offset=offset,
                                   step_factor=block)

    def state_dict(self):
        return dict(super().state_dict(), step_shrinkage=self.step_shrinkage, steps=self.steps,
                    step_correlation=self.step_correlation, step_correlation_raw=self.step_correlation_raw,
                    step_pairs=self.step_pairs, step_factor=self.step_factor)

    STEP_KEYS = ("step_shrinkage", "steps", "step_correlation", "step_correlation_raw", "step_pairs", "step_factor")

    def load_state_dict(self, state, device=None):
        missing = [k for k in self.STEP_KEYS if k not in state]
        if missing:
            raise ValueError(f"SpaceTimeCopula.load_state_dict: the state has no {', '.join(missing)}: it was saved by a "
                             "GaussianCopula, which couples no steps")
        f = state["step_factor"]
        if f is not None and (f.dim() != 2 or f.shape[0] != f.shape[1] or
                              tuple(state["step_correlation"].shape) != tuple(f.shape)):
            raise ValueError(f"SpaceTimeCopula.load_state_dict: step_factor {tuple(f.shape)} / step_correlation "
                             f"{tuple(state['step_correlation'].shape)} are not one square shape")
        GaussianCopula.load_state_dict(self, {k: v for k, v in state.items() if k not in self.STEP_KEYS}, device)

        def put(t, dtype):
            if t is None:
                return None
            return t.detach().to(device=t.device if device is None else device, dtype=dtype).contiguous().clone()

        self.step_correlation = put(state["step_correlation"], torch.float64)
        self.step_correlation_raw = put(state["step_correlation_raw"], torch.float64)
        self.step_pairs, self.step_factor = put(state["step_pairs"], torch.int64), put(f, torch.float32)
        self.steps = None if f is None else int(f.shape[0])
        self._blocks = {}
        return self

    @classmethod
    def from_state_dict(cls, state, device=None):
        if "step_shrinkage" not in state:
            raise ValueError("SpaceTimeCopula.from_state_dict: the state has no step_shrinkage: it was saved by a "
                             "GaussianCopula, which couples no steps")
        return cls(state["quantiles"], state["shrinkage"], state["step_shrinkage"], state["tails"],
                   state["min_pairs"]).load_state_dict(state, device)


def path_energy_score(target, paths, mul=None, add=None, ignore_nan=False, fair=False):
    """The energy score of whole trajectories: target [count, H, N] and paths [count, S, H, N] scored as count rows of H * N
    values, so that the dependence across steps counts as the dependence across nodes does in `EnsembleScores.energy` -- the
    one score that ranks step couplings (`SpaceTimeCopula` against `GaussianCopula`).  `ops.ensemble_scores` on the views
    [count, 1, H * N] and [count, S, 1, H * N]; mul / add [N] are repeated for every step.  Returns the mean over the origins
    as a numpy float64 (one sync).  ignore_nan, fair: as for `EnsembleScores`."""
    paths = _as_f32(paths)
    target = _as_f32(target, like=paths)
    if target.dim() != 3 or paths.dim() != 4 or (paths.shape[0],) + tuple(paths.shape[2:]) != tuple(target.shape):
        raise ValueError(f"path_energy_score: target must be [count, H, N] and paths [count, S, H, N], got "
                         f"{tuple(target.shape)} / {tuple(paths.shape)}")
    count, S, H, N = paths.shape
    if (mul is None) != (add is None):
        raise ValueError("path_energy_score: mul and add go together")
    if mul is not None:
        mul, add = (torch.as_tensor(v).reshape(-1).repeat(H) for v in (mul, add))
        if mul.numel() != H * N or add.numel() != H * N:
            raise ValueError(f"path_energy_score: mul and add must hold {N} values")
    out, _ = ops.ensemble_scores(target.contiguous().view(count, 1, H * N), paths.contiguous().view(count, S, 1, H * N), mul, add,
                                 ignore_nan=bool(ignore_nan), fair=bool(fair))
    return np.float64(out[1].item())


class ConformalCalibrator:
    """Split-conformal calibration of the bands of a quantile forecast (conformalized quantile regression), on the device.

    quantiles = the Q levels (at least two); the pairs are (i, Q-1-i), i < Q // 2, with nominal coverage
    tau_{Q-1-i} - tau_i (`QuantileScores.interval_nominal`); for odd Q the middle row belongs to no pair and is never touched.
    per_step / per_node: one offset per horizon step / per node, or pooled over that axis (the flags of `Scores.get`).

    fit(y, y_hat): y [count, H, N] held-out ground truth, y_hat [count, Q, H, N]; per pair and group the offset is the k-th
    smallest score max(y_hat_lo - y, y - y_hat_hi), k = ceil((m + 1) c (1 - 1e-12)) of the group's m scores (`ops.conformal_fit`);
    +inf where the group holds too few scores for the level (k > m: the band becomes the whole line).  A negative offset narrows
    the band.  ignore_nan: NaN targets are missing readings and are left out.
    apply(y_hat): the pairs' rows moved outwards by their offsets, every other row unchanged; any [count, Q, H, N], a [B, Q, H, N]
    straight from `Model.predict` included.

    Calibration works in the forecast's own (normalised) units: apply it AHEAD of de-normalising.  A pooled-over-nodes offset
    is then one number in z-score units, which is the sensible thing to share between nodes of different scale.
    On the calibration data itself every group with k <= m is covered at least k / m >= c; on exchangeable fresh data the
    coverage is at least c in expectation.  Attributes: offsets (device fp32 [P, Hg, Ng]), counts (int64, the m of every group),
    pairs, interval_nominal, per_step, per_node."""

    def __init__(self, quantiles, per_step=True, per_node=False):
        q = tuple(float(t) for t in quantiles)
        if len(q) < 2:
            raise ValueError(f"ConformalCalibrator: {len(q)} quantile level(s) form no pair; at least two are needed")
        Q = len(q)
        self.quantiles = q
        self.pairs = tuple((i, Q - 1 - i) for i in range(Q // 2))
        self.interval_nominal = np.array([q[hi] - q[lo] for lo, hi in self.pairs], dtype=np.float64)
        if not bool(((self.interval_nominal > 0) & (self.interval_nominal < 1)).all()):
            raise ValueError(f"ConformalCalibrator: levels {q} must be increasing inside (0, 1)")
        self.per_step, self.per_node = bool(per_step), bool(per_node)
        self.offsets = self.counts = None

    def fit(self, y, y_hat, ignore_nan=False):
        y_hat = _as_f32(y_hat)
        y = _as_f32(y, like=y_hat)
        if y_hat.dim() != 4 or y_hat.shape[1] != len(self.quantiles):
            raise ValueError(f"ConformalCalibrator.fit: y_hat must be [count, {len(self.quantiles)}, H, N], got "
                             f"{tuple(y_hat.shape)}")
        self.offsets, self.counts = ops.conformal_fit(y, y_hat, self.pairs, [float(c) for c in self.interval_nominal],
                                                      self.per_step, self.per_node, ignore_nan=bool(ignore_nan))
        return self

    def apply(self, y_hat, out=None):
        if self.offsets is None:
            raise ValueError("ConformalCalibrator.apply: not fitted (call fit or load_state_dict first)")
        y_hat = _as_f32(y_hat)
        _, Hg, Ng = self.offsets.shape
        if y_hat.dim() != 4 or y_hat.shape[1] != len(self.quantiles) or (self.per_step and y_hat.shape[2] != Hg) or \
                (self.per_node and y_hat.shape[3] != Ng):
            raise ValueError(f"ConformalCalibrator.apply: y_hat must be [count, {len(self.quantiles)}, "
                             f"{Hg if self.per_step else 'H'}, {Ng if self.per_node else 'N'}], got {tuple(y_hat.shape)}")
        offsets = self.offsets if self.offsets.device == y_hat.device or not y_hat.is_cuda else self.offsets.to(y_hat.device)
        return ops.conformal_apply(y_hat, offsets, self.pairs, self.per_step, self.per_node, out=out)

    def state_dict(self):
        return dict(quantiles=self.quantiles, pairs=self.pairs, per_step=self.per_step, per_node=self.per_node,
                    interval_nominal=torch.from_numpy(self.interval_nominal.copy()), offsets=self.offsets, counts=self.counts)

    def load_state_dict(self, state, device=None):
        q = tuple(float(t) for t in state["quantiles"])
        if q != self.quantiles or bool(state["per_step"]) != self.per_step or bool(state["per_node"]) != self.per_node:
            raise ValueError(f"ConformalCalibrator.load_state_dict: saved for levels {q}, per_step={state['per_step']}, "
                             f"per_node={state['per_node']}; this one has {self.quantiles}, {self.per_step}, {self.per_node}")
        offsets, counts = state["offsets"], state["counts"]
        if offsets is not None:
            if offsets.dim() != 3 or offsets.shape[0] != len(self.pairs) or counts.shape != offsets.shape:
                raise ValueError(f"ConformalCalibrator.load_state_dict: offsets {tuple(offsets.shape)} / counts "
                                 f"{tuple(counts.shape)} do not fit {len(self.pairs)} pairs")
            if device is not None:
                offsets, counts = offsets.to(device), counts.to(device)
            offsets, counts = offsets.float().contiguous(), counts.long().contiguous()
        self.offsets, self.counts = offsets, counts
        return self

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(state["quantiles"], state["per_step"], state["per_node"]).load_state_dict(state, device)


class SeasonalConformalCalibrator:
    """`ConformalCalibrator` per time-of-day bucket (Mondrian / category-conditional split-conformal calibration), on the device.

    A traffic model's residuals at 8 am are several times those at 3 am; offsets pooled over the day cover the nominal level on
    average but over-cover the quiet hours and under-cover the busy ones.  Here every target has an integer time index t on the
    user's clock (e.g. minutes / 5 since some midnight) and is calibrated within its bucket
        bucket(t) = ((t + phase) mod period) * buckets // period          (floor mod; `bucket_of` is this formula on the host)
    e.g. period=288, buckets=24 for hourly offsets of 5-minute data.  The bucket is the TARGET's: row i has an origin o_i, the
    time index of its step-0 target, and its step h is scored in, and widened with, bucket(o_i + h).

    fit(y, y_hat, origin): y [count, H, N], y_hat [count, Q, H, N]; origin an int (row i has origin + i: the rows of a
    validation pass) or an int64 tensor [count] (any order, repeats and gaps allowed; a host tensor is moved to the device
    once).  Within a bucket everything is `ConformalCalibrator.fit`'s definition (`ops.seasonal_fit`); period = buckets = 1 is
    `ConformalCalibrator` bit for bit.
    apply(y_hat, origin, out=None, rearrange=False): the pairs' rows moved by their bucket's offsets (`ops.seasonal_apply`);
    rearrange: the levels are first put in non-decreasing order (`rearrange_quantiles`), in the same launch.

    Thin buckets.  A bucket may hold too few scores for the level, and +inf (the whole line) is a poor band to serve.  With
    fallback="pooled" fit also runs the pooled `ops.conformal_fit` on the same tensors and every entry (s, p, g) whose count is
    below max(min_scores, m_min(c_p)) -- m_min(c) the smallest m whose rank ceil((m + 1) c (1 - 1e-12)) is <= m -- takes the
    pooled entry (on the device, no sync).  `offsets_seasonal` keeps the untouched tables and `pooled_offsets` the pooled one.
    fallback="inf" keeps the raw definition.

    Attributes: offsets (device fp32 [K, P, Hg, Ng], what apply and the live store use), counts (int64, the m of every bucket's
    group), pairs, interval_nominal, per_step, per_node, period, buckets, phase."""

    kind = "seasonal"

    def __init__(self, quantiles, period, buckets, phase=0, per_step=True, per_node=False, min_scores=0, fallback="pooled"):
        base = ConformalCalibrator(quantiles, per_step, per_node)          # its refusals: two levels, increasing in (0, 1)
        self.quantiles, self.pairs, self.interval_nominal = base.quantiles, base.pairs, base.interval_nominal
        self.per_step, self.per_node = base.per_step, base.per_node
        self.period, self.buckets, self.phase = int(period), int(buckets), int(phase)
        self.season = ops._season("SeasonalConformalCalibrator", (period, buckets, phase))
        if fallback not in ("pooled", "inf"):
            raise ValueError(f"SeasonalConformalCalibrator: fallback must be 'pooled' or 'inf', got {fallback!r}")
        if int(min_scores) < 0:
            raise ValueError(f"SeasonalConformalCalibrator: min_scores must be >= 0, got {min_scores}")
        self.min_scores, self.fallback = int(min_scores), fallback
        self.offsets = self.counts = self.offsets_seasonal = self.pooled_offsets = None

    def bucket_of(self, t):
        period, K, phase = self.season
        return ((int(t) + phase) % period) * K // period

    @staticmethod
    def min_count(c):
        """m_min(c): the smallest m whose rank is within the group, i.e. the fewest scores that give a finite offset."""
        import math
        m = 0
        while max(1, math.ceil(((m + 1) * float(c)) * (1 - 1e-12))) > m:
            m += 1
        return m

    def thresholds(self):
        """max(min_scores, m_min(c_p)) per pair: below it an entry falls back to the pooled one (fallback="pooled")."""
        return [max(self.min_scores, self.min_count(c)) for c in self.interval_nominal]

    def fit(self, y, y_hat, origin, ignore_nan=False):
        y_hat = _as_f32(y_hat)
        y = _as_f32(y, like=y_hat)
        if y_hat.dim() != 4 or y_hat.shape[1] != len(self.quantiles):
            raise ValueError(f"SeasonalConformalCalibrator.fit: y_hat must be [count, {len(self.quantiles)}, H, N], got "
                             f"{tuple(y_hat.shape)}")
        cov = [float(c) for c in self.interval_nominal]
        seasonal, self.counts = ops.seasonal_fit(y, y_hat, origin, self.pairs, cov, self.season, self.per_step,
                                                 self.per_node, ignore_nan=bool(ignore_nan))
        self.offsets_seasonal, self.pooled_offsets = seasonal, None
        self.offsets = seasonal
        if self.fallback == "pooled":
            self.pooled_offsets, _ = ops.conformal_fit(y, y_hat, self.pairs, cov, self.per_step, self.per_node,
                                                       ignore_nan=bool(ignore_nan))
            need = torch.tensor(self.thresholds(), dtype=torch.int64, device=seasonal.device).view(1, -1, 1, 1)
            self.offsets = torch.where(self.counts < need, self.pooled_offsets[None], seasonal).contiguous()
        return self

    def apply(self, y_hat, origin, out=None, rearrange=False):
        if self.offsets is None:
            raise ValueError("SeasonalConformalCalibrator.apply: not fitted (call fit or load_state_dict first)")
        y_hat = _as_f32(y_hat)
        _, _, Hg, Ng = self.offsets.shape
        if y_hat.dim() != 4 or y_hat.shape[1] != len(self.quantiles) or (self.per_step and y_hat.shape[2] != Hg) or \
                (self.per_node and y_hat.shape[3] != Ng):
            raise ValueError(f"SeasonalConformalCalibrator.apply: y_hat must be [count, {len(self.quantiles)}, "
                             f"{Hg if self.per_step else 'H'}, {Ng if self.per_node else 'N'}], got {tuple(y_hat.shape)}")
        offsets = self.offsets if self.offsets.device == y_hat.device or not y_hat.is_cuda else self.offsets.to(y_hat.device)
        return ops.seasonal_apply(y_hat, offsets, origin, self.pairs, self.season, self.per_step, self.per_node,
                                  rearrange=rearrange, out=out)

    def state_dict(self):
        return dict(kind=self.kind, quantiles=self.quantiles, pairs=self.pairs, per_step=self.per_step, per_node=self.per_node,
                    period=self.period, buckets=self.buckets, phase=self.phase, min_scores=self.min_scores,
                    fallback=self.fallback, interval_nominal=torch.from_numpy(self.interval_nominal.copy()),
                    offsets=self.offsets, counts=self.counts, offsets_seasonal=self.offsets_seasonal,
                    pooled_offsets=self.pooled_offsets)

    def load_state_dict(self, state, device=None):
        if state.get("kind") != self.kind:
            raise ValueError(f"SeasonalConformalCalibrator.load_state_dict: the state's kind is {state.get('kind')!r}, not "
                             f"{self.kind!r}")
        q = tuple(float(t) for t in state["quantiles"])
        mine = (self.quantiles, self.per_step, self.per_node, self.period, self.buckets, self.phase)
        saved = (q, bool(state["per_step"]), bool(state["per_node"]), int(state["period"]), int(state["buckets"]),
                 int(state["phase"]))
        if saved != mine:
            raise ValueError(f"SeasonalConformalCalibrator.load_state_dict: saved for (levels, per_step, per_node, period, "
                             f"buckets, phase) = {saved}; this one has {mine}")
        offsets, counts = state["offsets"], state["counts"]
        extra = [state.get("offsets_seasonal"), state.get("pooled_offsets")]
        if offsets is not None:
            if offsets.dim() != 4 or tuple(offsets.shape[:2]) != (self.buckets, len(self.pairs)) or \
                    counts.shape != offsets.shape:
                raise ValueError(f"SeasonalConformalCalibrator.load_state_dict: offsets {tuple(offsets.shape)} / counts "
                                 f"{tuple(counts.shape)} do not fit {self.buckets} buckets of {len(self.pairs)} pairs")
            if device is not None:
                offsets, counts = offsets.to(device), counts.to(device)
                extra = [None if t is None else t.to(device) for t in extra]
            offsets, counts = offsets.float().contiguous(), counts.long().contiguous()
            extra = [None if t is None else t.float().contiguous() for t in extra]
        self.offsets, self.counts = offsets, counts
        self.offsets_seasonal, self.pooled_offsets = extra
        return self

    @classmethod
    def from_state_dict(cls, state, device=None):
        return cls(state["quantiles"], state["period"], state["buckets"], state["phase"], state["per_step"], state["per_node"],
                   state.get("min_scores", 0), state.get("fallback", "pooled")).load_state_dict(state, device)


class _DeviceState:
    """The device tensors a streaming object owns: `_STATE` names them (all None until the state is made), `_TYPES` gives the
    dtypes that are not `_DTYPE`.  One definition of how they are saved, loaded and restored in place."""
    _STATE, _TYPES, _DTYPE = (), {}, torch.float32

    def _save_state(self):
        return {k: None if getattr(self, k) is None else getattr(self, k).clone() for k in self._STATE}

    def _drop_state(self):
        for k in self._STATE:
            setattr(self, k, None)

    def _take_state(self, state, shapes, device, in_place):
        """state[k] of shape shapes[k] for every k: a typed clone on `device`, or (in_place) copied into the tensor already
        owned, which a captured graph may read.  Nothing is written before every shape has passed."""
        for k in self._STATE:
            if tuple(state[k].shape) != tuple(shapes[k]):
                raise ValueError(f"{type(self).__name__}.load_state_dict: {k} is {tuple(state[k].shape)}, expected "
                                 f"{tuple(shapes[k])}")
        for k in self._STATE:
            if in_place:
                getattr(self, k).copy_(state[k])
            else:
                setattr(self, k, state[k].detach().to(device=device, dtype=self._TYPES.get(k, self._DTYPE)).contiguous().clone())

    def load_state_dict(self, state, device=None):
        return self._load(state, device, False)

    def restore_(self, state, device=None):
        """load_state_dict into the buffers already owned (same checks, same host counters): their addresses stay, so a
        captured graph that reads them goes on without re-capture.  Without device state yet it is load_state_dict; a state
        saved without device state leaves the buffers as they are."""
        return self._load(state, device, self.scores is not None)


class AdaptiveConformal(_DeviceState):
    """Adaptive conformal inference (ACI, Gibbs & Candes 2021) for the bands of a live quantile forecast, on the device.

    A `ConformalCalibrator` fitted once covers "in expectation on exchangeable new data"; a stream whose regime changes is not
    exchangeable.  This object keeps, per pair and group, a working miscoverage level alpha_t and a rolling window of the last
    `window` forecasts' scores, and after every realised target (`update`, one launch of ``ops.aci_update``)
        alpha <- alpha + gamma * (alpha* - miss / valid)            alpha* = 1 - interval_nominal
        offset <- the (1 - alpha) quantile of the window's valid scores (the calibrator's rank formula and exact select)
    alpha is not clamped: 1 - alpha <= 0 gives the offset -inf (an empty band, every target missed), a rank beyond the window's
    scores +inf (the whole line) -- those two excursions are what makes the long-run miscoverage of the ISSUED bands approach
    alpha* whatever the stream does: |miss rate - alpha*| <= (max(alpha_1, 1 - alpha_1) + gamma) / (gamma T) after T updates.
    gamma = 0 never moves alpha: a rolling-window split-conformal refit at the nominal level.  min_scores: a group's alpha and
    offset stay as they are until its window holds that many valid scores.

    The pairs, interval_nominal, per_step and per_node are `ConformalCalibrator`'s.  update(y, issued, raw): y [H, N] the realised
    targets (NaN = missing, left out), issued [Q, H, N] the rows that were served (the miss is counted on them), raw [Q, H, N] the
    same forecast ahead of calibration, rearranged if the server rearranges (the scores are taken on them); or
    update(None, issued, raw, ring=ring_y, origin=o) with the targets in a [C, N] ring at slots (o + h) mod C.
    `offsets` (device fp32 [P, Hg, Ng]) is the live buffer: a captured graph that reads it sees every update without re-capture;
    apply(y_hat) moves a [count, Q, H, N] forecast by it.  report() -> dict of numpy arrays alpha, offsets, counts, miss_sum,
    valid_sum, miscoverage (= miss_sum / valid_sum, NaN where nothing was valid), with one host sync.  The device state is made
    at the first update (or load_state_dict); state_dict() carries all of it, n_done included."""

    def __init__(self, quantiles, gamma=0.005, window=256, per_step=True, per_node=False, min_scores=0):
        base = ConformalCalibrator(quantiles, per_step, per_node)          # its refusals: two levels, increasing in (0, 1)
        self.quantiles, self.pairs, self.interval_nominal = base.quantiles, base.pairs, base.interval_nominal
        self.per_step, self.per_node = base.per_step, base.per_node
        gamma = float(gamma)
        if not gamma >= 0.0:
            raise ValueError(f"AdaptiveConformal: gamma must be >= 0, got {gamma}")
        if int(window) < 1:
            raise ValueError(f"AdaptiveConformal: window must be at least 1, got {window}")
        if int(min_scores) < 0:
            raise ValueError(f"AdaptiveConformal: min_scores must be >= 0, got {min_scores}")
        self.gamma, self.window, self.min_scores = gamma, int(window), int(min_scores)
        self.target_alpha = [1.0 - float(c) for c in self.interval_nominal]          # fp64, on the host
        self.n_done = 0
        self.scores = self.alpha = self.offsets = self.counts = self.miss_sum = self.valid_sum = None

    _STATE = ("scores", "alpha", "offsets", "counts", "miss_sum", "valid_sum")
    _TYPES, _DTYPE = dict(scores=torch.float32, alpha=torch.float64, offsets=torch.float32), torch.int64

    def group_shape(self, H, N):
        return (len(self.pairs), int(H) if self.per_step else 1, int(N) if self.per_node else 1)

    def init_state(self, H, N, device, offsets=None):
        """Make the device state for forecasts [Q, H, N] (update does it by itself; a caller that wants other initial offsets
        than 0, or the offsets buffer ahead of the first update, calls it first).  Fill kernels, never inside a capture.  With
        the state already there nothing changes."""
        if self.offsets is not None:
            if tuple(self.scores.shape[2:]) != (int(H), int(N)):
                raise ValueError(f"AdaptiveConformal: the state is for forecasts [Q, {self.scores.shape[2]}, "
                                 f"{self.scores.shape[3]}], got [Q, {H}, {N}]")
            return self
        shape = self.group_shape(H, N)
        self.scores = torch.full((self.window, shape[0], int(H), int(N)), float("nan"), device=device)
        ta = torch.tensor(self.target_alpha, dtype=torch.float64).reshape(-1, 1, 1)
        self.alpha = ta.expand(shape).contiguous().to(device)
        self.offsets = torch.zeros(shape, device=device) if offsets is None else \
            offsets.detach().to(device=device, dtype=torch.float32).reshape(shape).clone()
        self.counts, self.miss_sum, self.valid_sum = (torch.zeros(shape, dtype=torch.int64, device=device) for _ in range(3))
        return self

    def update(self, y, issued, raw, *, ring=None, origin=0):
        issued, raw = _as_f32(issued), _as_f32(raw)
        if issued.dim() != 3 or issued.shape[0] != len(self.quantiles) or raw.shape != issued.shape:
            raise ValueError(f"AdaptiveConformal.update: issued and raw must be [{len(self.quantiles)}, H, N], got "
                             f"{tuple(issued.shape)} / {tuple(raw.shape)}")
        if ring is None:
            ring, origin = _as_f32(y, like=issued).contiguous(), 0
            if tuple(ring.shape) != tuple(issued.shape[1:]):
                raise ValueError(f"AdaptiveConformal.update: y must be {tuple(issued.shape[1:])}, got {tuple(ring.shape)}")
        _, H, N = issued.shape
        self.init_state(H, N, issued.device)
        ops.aci_update(issued.contiguous(), raw.contiguous(), ring, origin, self.pairs, self.target_alpha, self.gamma,
                       self.n_done % self.window, self.min_scores, self.per_step, self.per_node, self.scores, self.alpha,
                       self.offsets, self.counts, self.miss_sum, self.valid_sum)
        self.n_done += 1
        return self

    def apply(self, y_hat, out=None):
        if self.offsets is None:
            raise ValueError("AdaptiveConformal.apply: no state yet (call update or load_state_dict first)")
        return ops.conformal_apply(_as_f32(y_hat), self.offsets, self.pairs, self.per_step, self.per_node, out=out)

    def report(self):
        if self.offsets is None:
            raise ValueError("AdaptiveConformal.report: no state yet (call update or load_state_dict first)")
        shape, n = tuple(self.offsets.shape), self.offsets.numel()
        flat = torch.cat([self.alpha.reshape(-1), self.offsets.double().reshape(-1)] +
                         [t.double().reshape(-1) for t in (self.counts, self.miss_sum, self.valid_sum)]).cpu().numpy()
        alpha, offsets, counts, miss, valid = (flat[i * n:(i + 1) * n].reshape(shape) for i in range(5))
        with np.errstate(divide="ignore", invalid="ignore"):
            rate = np.where(valid > 0, miss / valid, np.nan)
        return dict(alpha=alpha.copy(), offsets=offsets.astype(np.float32), counts=counts.astype(np.int64),
                    miss_sum=miss.astype(np.int64), valid_sum=valid.astype(np.int64), miscoverage=rate)

    def state_dict(self):
        state = dict(quantiles=self.quantiles, pairs=self.pairs, per_step=self.per_step, per_node=self.per_node,
                     gamma=self.gamma, window=self.window, min_scores=self.min_scores, n_done=int(self.n_done))
        state.update(self._save_state())
        return state

    def _load(self, state, device, in_place):
        q = tuple(float(t) for t in state["quantiles"])
        if q != self.quantiles or bool(state["per_step"]) != self.per_step or bool(state["per_node"]) != self.per_node or \
                int(state["window"]) != self.window:
            raise ValueError(f"AdaptiveConformal.load_state_dict: saved for levels {q}, per_step={state['per_step']}, "
                             f"per_node={state['per_node']}, window={state['window']}; this one has {self.quantiles}, "
                             f"{self.per_step}, {self.per_node}, {self.window}")
        sc = state["scores"]
        if sc is None:
            if not in_place:
                self._drop_state()
        else:
            if sc.dim() != 4 or sc.shape[0] != self.window or sc.shape[1] != len(self.pairs):
                raise ValueError(f"AdaptiveConformal.load_state_dict: scores {tuple(sc.shape)} do not fit window {self.window} / "
                                 f"{len(self.pairs)} pairs")
            own = self.scores if in_place else sc
            shapes = dict(dict.fromkeys(self._STATE, self.group_shape(own.shape[2], own.shape[3])), scores=tuple(own.shape))
            self._take_state(state, shapes, sc.device if device is None else device, in_place)
        self.n_done = int(state["n_done"])
        return self


class ConformalAnomaly(_DeviceState):
    """Streaming conformal anomaly detection: is the reading that just arrived normal?  On the device, one call per row.

    When row tau arrives, every stored forecast of it -- step h of the forecast made at origin tau - h, h < H -- is scored
    (score="point": |forecast - y| of one row; "band": max(lo - y, y - hi) of a quantile pair, the calibrator's score) and ranked
    against a rolling window of the scores of the last `window - 1` judged rows, grouped as `ConformalCalibrator` groups
    (per_step: against step h only; per_node: against node n only):
        p[h, n]   = (#{window scores >= score} + 1) / (m + 1)       the exact conformal p-value, NaN until m >= min_scores
        node_p[n] = min(1, v * min_h p[h, n])                       Bonferroni over the v judged steps: valid under any dependence
        alarm[n]  = node_p[n] <= alpha
    On an exchangeable stream P(p <= a) <= a, so the false-alarm rate per judged reading is at most alpha.  A missing reading
    (NaN) or a step with no stored forecast is absent: NaN p-value, counted nowhere.  The row's own scores enter the window only
    after it is judged, so a row is never compared with itself.

    update(y, forecasts): y [N], forecasts [H, N] or [R, H, N] (step h = the forecast of THIS row made h rows ago), rows=(lo, hi)
    the rows scored (default (0, 0) for "point", (0, R - 1) for "band"); or update(None, None, slab=out_forecast,
    origins=origins, row=tau, ring=ring_y, rows=(lo, hi)) on a forecast slab [S, (R,) H, N] with its device-side origins and the
    target ring, which is what LiveForecaster.set_anomaly issues.  One ``ops.anomaly_update``, no sync.
    Attributes (live device buffers of the last row): pvalues [H, N], node_p [N], alarm int32 [N]; counts (int64, the m of every
    group), alarm_sum / judged_sum (int64 [N]), n_done, last_row.  recent() -> (node_p [k, N], rows int64 [k]) ascending from the
    log of the last `keep` rows (the rows from a host mirror: no sync).  report() -> dict of numpy arrays with one sync,
    alarm_rate = alarm_sum / judged_sum and resolution = 1 / (counts + 1) (the smallest p a group can give) included.  The device
    state is made at the first update (or load_state_dict); state_dict() carries all of it."""

    def __init__(self, alpha=0.01, window=1024, per_step=True, per_node=True, min_scores=32, score="point", keep=64):
        alpha = float(alpha)
        if not (alpha > 0.0 and alpha < 1.0):
            raise ValueError(f"ConformalAnomaly: alpha must be inside (0, 1), got {alpha}")
        if int(window) < 2:
            raise ValueError(f"ConformalAnomaly: window must be at least 2 (the arriving row's own slot is left out, so a window "
                             f"of 1 has an empty population for ever), got {window}")
        if int(min_scores) < 0:
            raise ValueError(f"ConformalAnomaly: min_scores must be >= 0, got {min_scores}")
        if int(keep) < 1:
            raise ValueError(f"ConformalAnomaly: keep must be at least 1, got {keep}")
        if score not in ("point", "band"):
            raise ValueError(f"ConformalAnomaly: score must be 'point' or 'band', got {score!r}")
        self.alpha, self.window, self.min_scores, self.keep, self.score = alpha, int(window), int(min_scores), int(keep), score
        self.per_step, self.per_node = bool(per_step), bool(per_node)
        self.n_done, self.last_row = 0, -1
        self._log_rows = [-1] * self.keep
        self._work = None                                          # the entry's work buffer: zero between calls, no state
        self._drop_state()

    _STATE = ("scores", "pvalues", "node_p", "alarm", "counts", "alarm_sum", "judged_sum", "log_p")
    _TYPES = dict(alarm=torch.int32, counts=torch.int64, alarm_sum=torch.int64, judged_sum=torch.int64)

    def group_shape(self, H, N):
        return (int(H) if self.per_step else 1, int(N) if self.per_node else 1)

    def check_shape(self, H, N):
        """Refuse a configuration that can never raise an alarm: the smallest node_p is H / (m + 1), and m is at most
        (window - 1) * (group's steps) * (group's nodes).  Nothing touches the device."""
        import math
        per_row = (1 if self.per_step else int(H)) * (1 if self.per_node else int(N))
        need = math.ceil(int(H) / self.alpha * (1.0 - 1e-12))                    # m + 1 must reach this
        if (self.window - 1) * per_row + 1 < need:
            raise ValueError(f"ConformalAnomaly: window {self.window} can never alarm at alpha {self.alpha} with horizon {H}: "
                             f"the smallest p-value is {H} / {(self.window - 1) * per_row + 1}; window >= "
                             f"{-(-(need - 1) // per_row) + 1} would do")
        return self

    def _shapes(self, H, N):
        H, N = int(H), int(N)
        return dict(scores=(self.window, H, N), pvalues=(H, N), node_p=(N,), alarm=(N,), counts=self.group_shape(H, N),
                    alarm_sum=(N,), judged_sum=(N,), log_p=(self.keep, N))

    def init_state(self, H, N, R, device):
        """Make the device state for forecasts [R, H, N] (update does it by itself).  Fill kernels, never inside a capture.  With
        the state already there nothing changes."""
        if self.scores is not None:
            if tuple(self.scores.shape[1:]) != (int(H), int(N)):
                raise ValueError(f"ConformalAnomaly: the state is for forecasts [R, {self.scores.shape[1]}, "
                                 f"{self.scores.shape[2]}], got [R, {H}, {N}]")
            return self
        if not 1 <= int(R) <= 32:
            raise ValueError(f"ConformalAnomaly: forecasts of {R} rows (1 to 32 are served)")
        if self.score == "band" and int(R) < 2:
            raise ValueError("ConformalAnomaly: score='band' needs a forecast of at least two rows (a point forecast has no band)")
        self.check_shape(H, N)
        for k, shape in self._shapes(H, N).items():
            dt = self._TYPES.get(k, torch.float32)
            fill = float("nan") if dt == torch.float32 else 0
            setattr(self, k, torch.full(shape, fill, dtype=dt, device=device))
        return self

    def update(self, y, forecasts, *, slab=None, origins=None, row=None, ring=None, rows=None):
        if slab is None:
            f = _as_f32(forecasts)
            if f.dim() == 2:
                f = f[None]
            if f.dim() != 3:
                raise ValueError(f"ConformalAnomaly.update: forecasts must be [H, N] or [R, H, N], got {tuple(f.shape)}")
            slab, origins = f.contiguous()[None], None
            ring = _as_f32(y, like=f).contiguous()
            if tuple(ring.shape) != (f.shape[2],):
                raise ValueError(f"ConformalAnomaly.update: y must be [{f.shape[2]}], got {tuple(ring.shape)}")
            ring = ring[None]
            row = self.n_done if row is None else int(row)
        else:
            if ring is None or row is None:
                raise ValueError("ConformalAnomaly.update: the slab form needs ring= and row=")
            if slab.dim() == 3:                                    # a point model's slab [S, H, N]
                slab = slab[:, None]
            if slab.dim() != 4:
                raise ValueError(f"ConformalAnomaly.update: slab must be [S, H, N] or [S, R, H, N], got {tuple(slab.shape)}")
        _, R, H, N = slab.shape
        if rows is None:
            rows = (0, 0) if self.score == "point" else (0, R - 1)
        lo, hi = int(rows[0]), int(rows[1])
        if not 0 <= lo <= hi < R or (self.score == "band") != (lo < hi):
            raise ValueError(f"ConformalAnomaly.update: rows {(lo, hi)} do not name a {self.score} score of a forecast of {R} rows")
        self.init_state(H, N, R, slab.device)
        if self._work is None or self._work.device != self.scores.device:
            self._work = torch.zeros(2 * H * N, dtype=torch.int32, device=self.scores.device)
        log_slot = self.n_done % self.keep
        ops.anomaly_update(slab, origins, int(row), ring, (lo, hi), self.n_done % self.window, self.min_scores, self.alpha,
                           self.per_step, self.per_node, self.scores, self.pvalues, self.node_p, self.alarm, self.counts,
                           self.alarm_sum, self.judged_sum, self.log_p, log_slot, self._work)
        self._log_rows[log_slot] = int(row)
        self.n_done += 1
        self.last_row = int(row)
        return self

    def recent(self):
        """(node_p [k, N], rows int64 [k]) of the last k = min(n_done, keep) judged rows, oldest first."""
        if self.scores is None:
            raise ValueError("ConformalAnomaly.recent: no state yet (call update or load_state_dict first)")
        k = min(self.n_done, self.keep)
        first = (self.n_done - k) % self.keep
        order = [(first + i) % self.keep for i in range(k)]
        parts = [self.log_p[first:first + k]] if first + k <= self.keep else [self.log_p[first:], self.log_p[:first + k - self.keep]]
        return torch.cat(parts).clone(), torch.tensor([self._log_rows[s] for s in order], dtype=torch.int64)

    def report(self):
        if self.scores is None:
            raise ValueError("ConformalAnomaly.report: no state yet (call update or load_state_dict first)")
        names = ("pvalues", "node_p", "alarm", "counts", "alarm_sum", "judged_sum")
        flat = torch.cat([getattr(self, k).double().reshape(-1) for k in names]).cpu().numpy()
        out, at = {}, 0
        for k in names:
            t = getattr(self, k)
            out[k] = flat[at:at + t.numel()].reshape(tuple(t.shape)).astype(
                {torch.float32: np.float32, torch.int32: np.int32, torch.int64: np.int64}[t.dtype])
            at += t.numel()
        with np.errstate(divide="ignore", invalid="ignore"):
            out["alarm_rate"] = np.where(out["judged_sum"] > 0, out["alarm_sum"] / out["judged_sum"], np.nan)
        out["resolution"] = 1.0 / (out["counts"] + 1.0)
        out["n_done"], out["row"] = int(self.n_done), int(self.last_row)
        return out

    def _config(self):
        return dict(alpha=self.alpha, window=self.window, per_step=self.per_step, per_node=self.per_node,
                    min_scores=self.min_scores, score=self.score, keep=self.keep)

    def state_dict(self):
        return dict(self._config(), n_done=int(self.n_done), last_row=int(self.last_row), log_rows=list(self._log_rows),
                    **self._save_state())

    def _load(self, state, device, in_place):
        saved = {k: state[k] for k in self._config()}
        saved.update(alpha=float(saved["alpha"]), per_step=bool(saved["per_step"]), per_node=bool(saved["per_node"]))
        if saved != self._config():
            raise ValueError(f"ConformalAnomaly.load_state_dict: saved with {saved}; this one has {self._config()}")
        sc = state["scores"]
        if sc is None:
            if not in_place:
                self._drop_state()
        else:
            if sc.dim() != 3 or sc.shape[0] != self.window:
                raise ValueError(f"ConformalAnomaly.load_state_dict: scores {tuple(sc.shape)} do not fit window {self.window}")
            own = self.scores if in_place else sc
            self._take_state(state, self._shapes(own.shape[1], own.shape[2]), sc.device if device is None else device, in_place)
        self.n_done, self.last_row = int(state["n_done"]), int(state["last_row"])
        self._log_rows = [int(v) for v in state["log_rows"]]
        return self


def rearrange_quantiles(y_hat, out=None):
    """The monotone rearrangement of a quantile forecast [count, Q, H, N]: the Q values of every (window, step, node) in
    non-decreasing order (``ops.quantile_finish``; ``torch.sort(y_hat, dim=1, stable=True).values`` bit for bit), so no two levels
    cross and ``QuantileScores.crossing`` is 0 (swapping two crossed levels never raises their summed pinball loss).  out: as in
    ``ConformalCalibrator.apply`` (y_hat itself: in place).
    The one rule when it is combined with calibration: rearrange FIRST, and fit the calibrator on rearranged forecasts -- its
    offsets are quantiles of the scores of the rows it will be applied to.  Nothing is sorted again after calibration (that
    would move a nested inner band below its guarantee); nested pairs that still cross then are left alone and counted under
    ``crossing``."""
    return ops.quantile_finish(_as_f32(y_hat), rearrange=True, out=out)


def evaluate(y, y_hat, by_step=False, by_node=False, ignore_nan=False):
    """utils/math_utils.py:59-74.  y: ground truth, y_hat: prediction, both [count, time_step, node] on the GPU.
    ignore_nan: leave the elements whose ground truth is NaN out of every mean."""
    return Scores(y, y_hat, ignore_nan=ignore_nan).get(by_step, by_node)


_AXES = {None: (False, False), 0: (True, True), (0, 2): (True, False), (0, 1): (False, True)}


def _one(which, v, v_, axis):
    if axis not in _AXES:
        raise ValueError(f"axis {axis!r}: the device metrics cover the variants evaluate() uses: {list(_AXES)}")
    return Scores(v, v_).get(*_AXES[axis])[which]


def MAPE(v, v_, axis=None):
    return _one(0, v, v_, axis)


def MAE(v, v_, axis=None):
    return _one(1, v, v_, axis)


def RMSE(v, v_, axis=None):
    return _one(2, v, v_, axis)
