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
