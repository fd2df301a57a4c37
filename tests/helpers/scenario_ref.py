"""The definition of the scenario kernels (include/stemgnn_hip.h: stemgnn_scenario_roll / _bands / _rank), restated in numpy:
the order of a column, the Philox counter map, the uniform, the segment, the weight and the draw in float32 with every operation
rounded on its own, the window roll and the order statistics of the paths.  Nothing here touches the code under test."""
import math

import numpy as np

from tests.helpers.philox_ref import philox4x32_10

F = np.float32
_M64 = (1 << 64) - 1


def rank(tau, S):
    """the definition: two fp64 multiplies, a ceil, clamped to [1, S]"""
    return min(int(S), max(1, math.ceil(float(tau) * int(S) * (1 - 1e-12))))


def order_key(v):
    """float32 array -> a float64 key whose ascending stable sort is the order of the definition: fp32's order with
    -0 == +0 (both map to 0.0) and NaN above +inf (a key beyond every float32)"""
    v = np.asarray(v, F)
    k = v.astype(np.float64) + 0.0
    k[v == 0] = 0.0
    k[np.isnan(v)] = np.inf
    k[np.isposinf(v)] = 1e300
    return k


def stable_order(v, axis):
    """indices that put `v` in the definition's order along `axis`, ties in index order"""
    return np.argsort(order_key(v), axis=axis, kind="stable")


def words(origin0, Bo, S, horizon, step, L, N, seed, offset, coupling):
    """uint32 [Bo, S, L, N]: the Philox word of every draw of the round"""
    nq = (N + 3) // 4
    b, s, j, n = np.meshgrid(np.arange(Bo), np.arange(S), np.arange(L), np.arange(N), indexing="ij")
    out = np.empty(b.shape, np.uint32)
    flat = out.reshape(-1)
    bf, sf, jf, nf = (a.reshape(-1) for a in (b, s, j, n))
    ctr = np.empty(flat.size, np.uint64)
    for e in range(flat.size):                                  # Python ints: 64-bit wrapping arithmetic, stated once
        row0 = ((int(origin0) + int(bf[e])) * S + int(sf[e])) * horizon + step
        c = row0 * nq if coupling == "path" else (row0 + int(jf[e])) * nq + (int(nf[e]) >> 2)
        ctr[e] = c & _M64
    w = philox4x32_10((ctr & np.uint64(0xFFFFFFFF), ctr >> np.uint64(32), offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    w = np.stack(w, axis=-1)
    flat[:] = w[:, 0] if coupling == "path" else w[np.arange(flat.size), nf & 3]
    return out


def uniform(w):
    return (((w >> np.uint32(9)).astype(F) + F(0.5)) * F(2.0 ** -23)).astype(F)


def draw(column, taus, u, tails):
    """column float32 [P, Q, L, N], u float32 [P, L, N] -> y float32 [P, L, N]"""
    taus = np.asarray(taus, F)
    Q = taus.size
    v = np.take_along_axis(column, stable_order(column, 1), axis=1)
    i = np.zeros(u.shape, np.int64)
    for q in range(1, Q - 1):
        i = np.where(taus[q] <= u, q, i)
    t0, t1 = taus[i], taus[i + 1]
    with np.errstate(all="ignore"):
        wt = ((u - t0).astype(F) / (t1 - t0).astype(F)).astype(F)
        if tails == "clamp":
            wt = np.minimum(np.maximum(wt, F(0)), F(1))
        lo = np.take_along_axis(v, i[:, None], axis=1)[:, 0]
        hi = np.take_along_axis(v, i[:, None] + 1, axis=1)[:, 0]
        d = (hi - lo).astype(F)
        return (lo + (d * wt).astype(F)).astype(F)


def roll(inputs, forecast, taus, Bo, S, fan, step, horizon, origin0, seed, offset, coupling, tails, paths, bands=None,
         inputs_next=None):
    """One round, in place on paths / bands / inputs_next (numpy float32 arrays of the entry's shapes; the last two may be
    None)."""
    _, W, N = inputs.shape
    Q, L = forecast.shape[1:3]
    src = np.arange(Bo * S) // fan
    u = uniform(words(origin0, Bo, S, horizon, step, L, N, seed, offset, coupling)).reshape(Bo * S, L, N)
    y = draw(forecast[src], taus, u, tails)                    # [Bo * S, L, N]
    take = min(L, horizon - step)
    paths.reshape(Bo * S, horizon, N)[:, step:step + take] = y[:, :take]
    if inputs_next is not None:
        inputs_next[:, :W - L] = inputs[src][:, L:]
        inputs_next[:, W - L:] = y
    if bands is not None:
        bands[:, :, step:step + take] = forecast[:, :, :take]


def bands_of(paths, taus, step_from, bands):
    """bands[b, q, h, n] = the rank(taus[q], S)-th smallest of paths[b, :, h, n] for h >= step_from, in place"""
    S = paths.shape[1]
    v = np.take_along_axis(paths, stable_order(paths, 1), axis=1)
    for q, t in enumerate(taus):
        bands[:, q, step_from:] = v[:, rank(t, S) - 1, step_from:]
