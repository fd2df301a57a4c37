"""The definition of the copula entries (include/stemgnn_hip.h: stemgnn_copula_pit / _gram / _uniforms) and of
math_utils.GaussianCopula.fit, restated in numpy: the transform in float32 with every operation rounded on its own (the inverse
of scenario_ref.draw, operation by operation), the pairwise-complete moments and the uniforms in float64.  The order of a column,
the Philox counter map and the uniform of a word are scenario_ref's.  Nothing here touches the code under test."""
import numpy as np
import torch

from tests.helpers import scenario_ref as R
from tests.helpers.philox_ref import philox4x32_10

F = np.float32
U_LO, U_HI = F(2.0 ** -24), F(1.0 - 2.0 ** -24)
CHUNK = 1024                                 # rows per workgroup of the gram kernel (CP_CHUNK in csrc/copula.hip)


def ndtri(p):
    return torch.special.ndtri(torch.from_numpy(np.ascontiguousarray(p, np.float64))).numpy()


def ndtr(z):
    return torch.special.ndtr(torch.from_numpy(np.ascontiguousarray(z, np.float64))).numpy()


def keep_nan_clamp(v, lo, hi):
    return np.where(v < lo, lo, np.where(v > hi, hi, v)).astype(F)


def pit(column, taus, y, tails):
    """column float32 [P, Q, L, N], y float32 [P, L, N] -> u float32 [P, L, N]"""
    taus = np.asarray(taus, F)
    Q = taus.size
    column, y = np.asarray(column, F), np.asarray(y, F)
    v = np.take_along_axis(column, R.stable_order(column, 1), axis=1)
    with np.errstate(all="ignore"):
        below = (v <= y[:, None]).sum(axis=1)
        i = np.clip(below - 1, 0, Q - 2)
        t0, t1 = taus[i], taus[i + 1]
        lo = np.take_along_axis(v, i[:, None], axis=1)[:, 0]
        hi = np.take_along_axis(v, i[:, None] + 1, axis=1)[:, 0]
        d, num = (hi - lo).astype(F), (y - lo).astype(F)
        wt = (num / d).astype(F)
        flat = np.where(num == 0, F(0.5), np.where(num > 0, F(np.inf), F(-np.inf))).astype(F)
        wt = np.where(d == 0, flat, wt).astype(F)
        if tails == "clamp":
            wt = keep_nan_clamp(wt, F(0), F(1))
        span = (t1 - t0).astype(F)
        u = (t0 + (span * wt).astype(F)).astype(F)
        u = keep_nan_clamp(u, U_LO, U_HI)
    missing = np.isnan(y) | np.isnan(column).any(axis=1)
    return np.where(missing, F(np.nan), u).astype(F)


def roll_given(inputs, forecast, taus, u, Bo, S, fan, step, horizon, tails, paths, bands=None, inputs_next=None):
    """scenario_ref.roll with the uniforms u float32 [Bo, S, L, N] given instead of drawn, in place on paths / bands /
    inputs_next"""
    _, W, N = inputs.shape
    L = forecast.shape[2]
    src = np.arange(Bo * S) // fan
    y = R.draw(forecast[src], taus, np.asarray(u, F).reshape(Bo * S, L, N), tails)
    take = min(L, horizon - step)
    paths.reshape(Bo * S, horizon, N)[:, step:step + take] = y[:, :take]
    if inputs_next is not None:
        inputs_next[:, :W - L] = inputs[src][:, L:]
        inputs_next[:, W - L:] = y
    if bands is not None:
        bands[:, :, step:step + take] = forecast[:, :, :take]


def gram(u):
    """u float32 [M, N] -> pairs int64 [N, N], sums float64 [3, N, N], absolute sums float64 [3, N, N] (the yardstick of the
    tolerance: the same three sums over the absolute values of their terms)"""
    z = ndtri(np.asarray(u, F).astype(np.float64))
    present = ~np.isnan(z)
    p = present.astype(np.float64)
    z0 = np.where(present, z, 0.0)
    pairs = present.astype(np.int64).T @ present.astype(np.int64)
    sums = np.stack([z0.T @ z0, z0.T @ p, (z0 * z0).T @ p])
    mags = np.stack([np.abs(z0).T @ np.abs(z0), np.abs(z0).T @ p, (z0 * z0).T @ p])
    return pairs, sums, mags


def correlation(pairs, sums, min_pairs):
    """GaussianCopula.fit's elementwise step: the raw correlation matrix of the pairwise-complete moments"""
    s, a, q = sums
    with np.errstate(all="ignore"):
        m = pairs.astype(np.float64)
        mean = a / m
        var = q / m - mean * mean
        r = (s / m - mean * mean.T) / np.sqrt(var * var.T)
    r = np.where((pairs < min_pairs) | ~(var > 0) | ~(var.T > 0), 0.0, r)
    np.fill_diagonal(r, 1.0)
    return (r + r.T) / 2


def factor_of(corr):
    """the float32 lower Cholesky factor of a float64 correlation matrix, as GaussianCopula stores it (before the transpose)"""
    return np.linalg.cholesky(np.asarray(corr, np.float64)).astype(F)


def words(origin0, Bo, S, horizon, step, L, N, seed, offset):
    """scenario_ref.words(..., "independent") with the 64-bit wrapping counter in numpy uint64 arithmetic (the CPU test holds
    the two against each other)"""
    nq = np.uint64((N + 3) // 4)
    b, s, j, n = np.meshgrid(np.arange(Bo, dtype=np.uint64), np.arange(S, dtype=np.uint64), np.arange(L, dtype=np.uint64),
                             np.arange(N, dtype=np.uint64), indexing="ij")
    with np.errstate(over="ignore"):
        o = np.uint64(int(origin0) & ((1 << 64) - 1))
        ctr = (((o + b) * np.uint64(S) + s) * np.uint64(horizon) + np.uint64(step) + j) * nq + (n >> np.uint64(2))
    w = philox4x32_10((ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return np.take_along_axis(np.stack(w, axis=-1), (n & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def uniforms(factor, origin0, Bo, S, horizon, step, L, seed, offset):
    """factor float32 [N, N] lower triangular -> (u* float64 [Bo, S, L, N] = clip(ndtr(factor e*)), (|factor| |e*|) of the same
    shape: the yardstick of the summation bound)"""
    N = factor.shape[0]
    e = ndtri(R.uniform(words(origin0, Bo, S, horizon, step, L, N, seed, offset)).astype(np.float64))
    lower = np.tril(np.asarray(factor, np.float64))
    u = np.clip(ndtr(e @ lower.T), float(U_LO), float(U_HI))
    return u, np.abs(e) @ np.abs(lower).T


# ---- the configuration of the energy-score test: a block-correlated truth under exact N(0, 1) marginals --------------------------
ENERGY_TAUS = (0.02, 0.1, 0.25, 0.5, 0.75, 0.9, 0.98)
ENERGY_N, ENERGY_FIT, ENERGY_NEW, ENERGY_S = 16, 512, 1024, 32
ENERGY_KEY, ENERGY_ORIGIN0 = 0x5DEECE66D, 2 ** 33 + 99


def block_correlation(n=ENERGY_N, block=8, rho=0.9):
    r = np.zeros((n, n))
    for at in range(0, n, block):
        r[at:at + block, at:at + block] = rho
    np.fill_diagonal(r, 1.0)
    return r


def energy_case(seed):
    """dict(R_true, y_fit [512, 1, 16], f_fit [512, 7, 1, 16], y_new [1024, 1, 16], f_new [1024, 7, 1, 16]), float32"""
    rng = np.random.default_rng(seed)
    r_true = block_correlation()
    chol = np.linalg.cholesky(r_true)
    z = ndtri(np.asarray(ENERGY_TAUS)).astype(F)

    def rows(count):
        y = (rng.normal(size=(count, ENERGY_N)) @ chol.T).astype(F)[:, None]
        return y, np.ascontiguousarray(np.broadcast_to(z[None, :, None, None], (count, len(z), 1, ENERGY_N)))

    y_fit, f_fit = rows(ENERGY_FIT)
    y_new, f_new = rows(ENERGY_NEW)
    return dict(R_true=r_true, y_fit=y_fit, f_fit=f_fit, y_new=y_new, f_new=f_new)


def energy_case_restated(case, shrinkage=0.05, min_pairs=8):
    """The three ensembles [1024, 32, 1, 16] of the case and the raw correlation, by the restatement alone"""
    N, S, count = ENERGY_N, ENERGY_S, ENERGY_NEW
    u_fit = pit(case["f_fit"], ENERGY_TAUS, case["y_fit"], "linear")
    pairs, sums, _ = gram(u_fit.reshape(-1, N))
    raw = correlation(pairs, sums, min_pairs)
    factor = factor_of((1 - shrinkage) * raw + shrinkage * np.eye(N))
    out = dict(correlation_raw=raw)
    column = np.repeat(case["f_new"], S, axis=0)                                   # fan = S: every path reads its origin's column
    for name in ("independent", "path"):
        u = R.uniform(R.words(ENERGY_ORIGIN0, count, S, 1, 0, 1, N, ENERGY_KEY, 0, name)) if name == "path" else \
            R.uniform(words(ENERGY_ORIGIN0, count, S, 1, 0, 1, N, ENERGY_KEY, 0))
        out[name] = R.draw(column, ENERGY_TAUS, u.reshape(count * S, 1, N), "linear").reshape(count, S, 1, N)
    u, _ = uniforms(factor, ENERGY_ORIGIN0, count, S, 1, 0, 1, ENERGY_KEY, 0)
    out["copula"] = R.draw(column, ENERGY_TAUS, u.astype(F).reshape(count * S, 1, N), "linear").reshape(count, S, 1, N)
    return out


def crps_and_energy(target, paths):
    """(mean CRPS, mean energy score) of paths [count, S, H, N] against target [count, H, N], float64, D = S^2"""
    x, y = np.asarray(paths, np.float64), np.asarray(target, np.float64)
    S = x.shape[1]
    crps = np.abs(x - y[:, None]).mean(axis=1) - np.abs(x[:, :, None] - x[:, None]).sum(axis=(1, 2)) / (2.0 * S * S)
    first = np.sqrt(((x - y[:, None]) ** 2).sum(axis=-1)).mean(axis=1)
    second = np.sqrt(((x[:, :, None] - x[:, None]) ** 2).sum(axis=-1)).sum(axis=(1, 2)) / (2.0 * S * S)
    return float(crps.mean()), float((first - second).mean())
