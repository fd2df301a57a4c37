"""The definition of stemgnn_copula_uniforms_steps (include/stemgnn_hip.h) and of math_utils.SpaceTimeCopula.fit, restated in
numpy on top of tests/helpers/copula_ref.py: the Philox words, the inverse and the forward normal CDF are that file's, the step
mix and the node sum are float64 products.  It also holds the statistical case of the step coupling: a truth whose normal scores
are correlated T (x) R over (step, node) under exact N(0, 1) marginals, and its ensembles by the restatement alone.  Nothing
here touches the code under test."""
import numpy as np

from tests.helpers import copula_ref as C
from tests.helpers import scenario_ref as R

F = np.float32


def uniforms_steps(factor, step_factor, origin0, Bo, S, horizon, step, L, seed, offset):
    """factor float32 [N, N] and step_factor float32 [L, L], lower triangular (what lies above the diagonals is not read) ->
    (u* float64 [Bo, S, L, N] = clip(ndtr(A e* factor^T)) with A applied along the steps, and |A| |e*| |factor|^T of the same
    shape: the yardstick of the summation bound)"""
    N = factor.shape[0]
    e = C.ndtri(R.uniform(C.words(origin0, Bo, S, horizon, step, L, N, seed, offset)).astype(np.float64))
    lower = np.tril(np.asarray(factor, np.float64))
    A = np.tril(np.asarray(step_factor, np.float64))
    assert A.shape == (L, L)
    g = np.einsum("ji,bsin->bsjn", A, e)
    u = np.clip(C.ndtr(g @ lower.T), float(C.U_LO), float(C.U_HI))
    return u, np.einsum("ji,bsin->bsjn", np.abs(A), np.abs(e)) @ np.abs(lower).T


def decay(n, rho):
    ij = np.arange(n)
    return rho ** np.abs(ij[:, None] - ij[None, :]).astype(np.float64)


def kron_correlation(z):
    """z [rows, L, N] normal scores -> their empirical correlation [L * N, L * N], (step, node) flattened step-major"""
    return np.corrcoef(z.reshape(z.shape[0], -1), rowvar=False)


# ---- the statistical case: 4 steps x 16 nodes, node blocks of 8 at 0.9, steps at 0.8^|i - j| -----------------------------------
STEPS_L, STEPS_RHO, STEPS_THRESHOLD = 4, 0.8, 0.5
STEPS_N, STEPS_FIT, STEPS_NEW, STEPS_S = C.ENERGY_N, C.ENERGY_FIT, C.ENERGY_NEW, C.ENERGY_S
STEPS_TAUS, STEPS_KEY, STEPS_ORIGIN0 = C.ENERGY_TAUS, C.ENERGY_KEY, C.ENERGY_ORIGIN0


def steps_case(seed):
    """dict(R_true [16, 16], T_true [4, 4], y_fit [512, 4, 16], f_fit [512, 7, 4, 16], y_new [1024, 4, 16], f_new
    [1024, 7, 4, 16]), float32: y = A_T e chol(R)^T with e i.i.d. N(0, 1); every forecast is the exact N(0, 1) quantile function"""
    rng = np.random.default_rng(seed)
    r_true, t_true = C.block_correlation(STEPS_N, 8, 0.9), decay(STEPS_L, STEPS_RHO)
    chol_r, chol_t = np.linalg.cholesky(r_true), np.linalg.cholesky(t_true)
    z = C.ndtri(np.asarray(STEPS_TAUS)).astype(F)

    def rows(count):
        e = rng.normal(size=(count, STEPS_L, STEPS_N))
        y = (np.einsum("ji,cin->cjn", chol_t, e) @ chol_r.T).astype(F)
        return y, np.ascontiguousarray(np.broadcast_to(z[None, :, None, None], (count, len(z), STEPS_L, STEPS_N)))

    y_fit, f_fit = rows(STEPS_FIT)
    y_new, f_new = rows(STEPS_NEW)
    return dict(R_true=r_true, T_true=t_true, y_fit=y_fit, f_fit=f_fit, y_new=y_new, f_new=f_new)


def steps_case_restated(case, shrinkage=0.05, step_shrinkage=0.0, min_pairs=8):
    """The two ensembles [1024, 32, 4, 16] of the case -- "space" (the node copula alone) and "steps" (node and step) -- and the
    raw step correlation, by the restatement alone"""
    N, L, S, count = STEPS_N, STEPS_L, STEPS_S, STEPS_NEW
    u_fit = C.pit(case["f_fit"], STEPS_TAUS, case["y_fit"], "linear")
    pairs, sums, _ = C.gram(u_fit.reshape(-1, N))
    raw = C.correlation(pairs, sums, min_pairs)
    factor = C.factor_of((1 - shrinkage) * raw + shrinkage * np.eye(N))
    s_pairs, s_sums, _ = C.gram(np.ascontiguousarray(u_fit.transpose(0, 2, 1)).reshape(-1, L))
    s_raw = C.correlation(s_pairs, s_sums, min_pairs)
    step_factor = C.factor_of((1 - step_shrinkage) * s_raw + step_shrinkage * np.eye(L))
    column = np.broadcast_to(case["f_new"][:1], (count * S,) + case["f_new"].shape[1:])       # every row holds the same column
    out = dict(correlation_raw=raw, step_correlation_raw=s_raw, step_pairs=s_pairs)
    u, _ = C.uniforms(factor, STEPS_ORIGIN0, count, S, L, 0, L, STEPS_KEY, 0)
    out["space"] = R.draw(column, STEPS_TAUS, u.astype(F).reshape(count * S, L, N), "linear").reshape(count, S, L, N)
    u, _ = uniforms_steps(factor, step_factor, STEPS_ORIGIN0, count, S, L, 0, L, STEPS_KEY, 0)
    out["steps"] = R.draw(column, STEPS_TAUS, u.astype(F).reshape(count * S, L, N), "linear").reshape(count, S, L, N)
    return out


def path_energy(target, paths, chunk=128):
    """the mean energy score of whole trajectories: paths [count, S, H, N] against target [count, H, N] as count rows of H * N
    values, float64, D = S^2"""
    count, S = paths.shape[:2]
    x, y = np.asarray(paths, np.float64).reshape(count, S, -1), np.asarray(target, np.float64).reshape(count, 1, -1)
    total = 0.0
    for at in range(0, count, chunk):
        xc, yc = x[at:at + chunk], y[at:at + chunk]
        first = np.sqrt(((xc - yc) ** 2).sum(axis=-1)).mean(axis=1)
        second = np.sqrt(((xc[:, :, None] - xc[:, None]) ** 2).sum(axis=-1)).sum(axis=(1, 2)) / (2.0 * S * S)
        total += float((first - second).sum())
    return total / count


def crps_and_energy(target, paths, chunk=128):
    """copula_ref.crps_and_energy (marginal CRPS, per-step energy score) over chunks of origins of one size"""
    count = paths.shape[0]
    assert count % chunk == 0
    parts = [C.crps_and_energy(target[at:at + chunk], paths[at:at + chunk]) for at in range(0, count, chunk)]
    return float(np.mean([p[0] for p in parts])), float(np.mean([p[1] for p in parts]))


def run_event(target, paths, node=0, threshold=STEPS_THRESHOLD):
    """(mean odds, Brier score, base rate) of "node above threshold at every step": the odds are the share of paths in the event"""
    odds = (np.asarray(paths)[:, :, :, node] > threshold).all(axis=2).mean(axis=1)
    happened = (np.asarray(target)[:, :, node] > threshold).all(axis=1).astype(np.float64)
    return float(odds.mean()), float(((odds - happened) ** 2).mean()), float(happened.mean())
