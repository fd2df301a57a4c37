"""The definition of split-conformal calibration of quantile bands, restated in numpy: the rank, the fp32 score, the k-th smallest
score per group, and the apply.  Nothing here touches the code under test.  (tests/test_hip_conformal.py and
tests/test_calibration_cases.py compare csrc/conformal.hip with it.)"""
import math

import numpy as np

INF = np.float32(np.inf)


def rank(m, c):
    t = (m + 1) * c
    return math.ceil(t * (1 - 1e-12))


def scores_np(y, f, lo, hi):
    """fp32: two rounded subtractions and a max; a NaN score counts as +inf"""
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.maximum(f[:, lo] - y, y - f[:, hi])               # np.maximum propagates NaN
    assert s.dtype == np.float32
    return np.where(np.isnan(s), INF, s)


def fit_np(y, f, pairs, coverage, per_step, per_node, masked):
    C, H, N = y.shape
    Hg, Ng = (H if per_step else 1), (N if per_node else 1)
    offsets = np.empty((len(pairs), Hg, Ng), np.float32)
    counts = np.empty((len(pairs), Hg, Ng), np.int64)
    keep = ~np.isnan(y) if masked else np.ones(y.shape, bool)
    for p, (lo, hi) in enumerate(pairs):
        s = scores_np(y, f, lo, hi)
        for hg in range(Hg):
            hs = slice(hg, hg + 1) if per_step else slice(None)
            for ng in range(Ng):
                ns = slice(ng, ng + 1) if per_node else slice(None)
                v = np.sort(s[:, hs, ns][keep[:, hs, ns]])
                k = rank(v.size, coverage[p])
                counts[p, hg, ng] = v.size
                offsets[p, hg, ng] = INF if k > v.size else v[k - 1]
    return offsets, counts


def apply_np(f, offsets, pairs, per_step, per_node):
    out = f.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p, (lo, hi) in enumerate(pairs):
            off = offsets[p][None]                                # [1, Hg, Ng] broadcasts over the pooled axes
            out[:, lo] = f[:, lo] - off
            out[:, hi] = f[:, hi] + off
    assert out.dtype == np.float32
    return out
