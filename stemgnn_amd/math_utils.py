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
