"""numpy restatement of stemgnn_aci_update (include/stemgnn_hip.h): the reference of tests/test_aci_abi.py and
tests/test_hip_aci.py, never the code under test.  fp32 scores, fp64 alpha with one numpy operation per IEEE operation in the
kernel's order, np.sort for the k-th value, the rank formula of stemgnn_conformal_rank."""
import math

import numpy as np

F32 = np.float32


def rank(m, c):
    """stemgnn_conformal_rank: max(1, ceil(((m + 1) * c) * (1 - 1e-12))), two fp64 multiplies"""
    t = np.float64(m + 1) * np.float64(c)
    return max(1.0, math.ceil(t * np.float64(1.0 - 1e-12)))


def scores_of(y, lo, hi):
    """s = max(lo - y, y - hi) in fp32 as cf_key orders it: NaN from the forecast -> +inf, -0 -> +0; NaN target -> NaN"""
    y, lo, hi = (np.asarray(v, dtype=F32) for v in (y, lo, hi))
    with np.errstate(invalid="ignore"):
        a, b = lo - y, y - hi
        s = np.where(a > b, a, b).astype(F32)
    s[np.isnan(a) | np.isnan(b)] = F32(np.inf)
    s[s == 0] = F32(0.0)
    s[np.isnan(y)] = F32(np.nan)
    return s


class AciRef:
    def __init__(self, pairs, target_alpha, gamma, window, per_step, per_node, min_scores, H, N, offsets=None):
        self.pairs, self.ta = [tuple(p) for p in pairs], [np.float64(a) for a in target_alpha]
        self.gamma, self.M, self.min_scores = np.float64(gamma), int(window), int(min_scores)
        self.per_step, self.per_node, self.H, self.N = bool(per_step), bool(per_node), H, N
        P = len(self.pairs)
        self.shape = (P, H if per_step else 1, N if per_node else 1)
        self.scores = np.full((self.M, P, H, N), np.nan, dtype=F32)
        self.alpha = np.empty(self.shape, dtype=np.float64)
        for p in range(P):
            self.alpha[p] = self.ta[p]
        self.offsets = np.zeros(self.shape, dtype=F32) if offsets is None else np.array(offsets, dtype=F32).reshape(self.shape)
        self.counts, self.miss_sum, self.valid_sum = (np.zeros(self.shape, dtype=np.int64) for _ in range(3))
        self.n_done = 0
        self.branches = set()                       # which of the offset's branches have occurred: "-inf", "+inf", "select", "hold"

    def _slices(self, hg, ng):
        return (slice(hg, hg + 1) if self.per_step else slice(None)), (slice(ng, ng + 1) if self.per_node else slice(None))

    def update(self, y, issued, raw):
        y, issued, raw = (np.asarray(v, dtype=F32) for v in (y, issued, raw))
        slot = self.n_done % self.M
        valid_el = ~np.isnan(y)
        for p, (lo, hi) in enumerate(self.pairs):
            self.scores[slot, p] = scores_of(y, raw[lo], raw[hi])
            with np.errstate(invalid="ignore"):
                miss_el = valid_el & ~((issued[lo] <= y) & (y <= issued[hi]))
            for hg in range(self.shape[1]):
                for ng in range(self.shape[2]):
                    hs, ns = self._slices(hg, ng)
                    valid, miss = int(valid_el[hs, ns].sum()), int(miss_el[hs, ns].sum())
                    g = (p, hg, ng)
                    self.miss_sum[g] += miss
                    self.valid_sum[g] += valid
                    w = self.scores[:, p, hs, ns].reshape(-1)
                    w = w[~np.isnan(w)]
                    w = np.where(w == 0, F32(0.0), w)          # a loaded window may hold -0: it orders, and comes back, as +0
                    m = int(w.size)
                    self.counts[g] = m
                    if valid == 0 or m < self.min_scores:
                        self.branches.add("hold")
                        continue
                    err = np.float64(miss) / np.float64(valid)
                    a = self.alpha[g] + self.gamma * (self.ta[p] - err)
                    self.alpha[g] = a
                    c = np.float64(1.0) - a
                    if not c > 0.0:
                        self.offsets[g] = F32(-np.inf)
                        self.branches.add("-inf")
                        continue
                    k = rank(m, c)
                    if k > m:
                        self.offsets[g] = F32(np.inf)
                        self.branches.add("+inf")
                        continue
                    self.offsets[g] = np.sort(w)[int(k) - 1]
                    self.branches.add("select")
        self.n_done += 1

    def apply(self, forecast):
        """conformal_apply on one [Q, H, N] forecast: lo - offset, hi + offset, one fp32 operation each"""
        out = np.array(forecast, dtype=F32)
        off = np.broadcast_to(self.offsets, (len(self.pairs), self.H, self.N))
        with np.errstate(invalid="ignore"):
            for p, (lo, hi) in enumerate(self.pairs):
                out[lo] = out[lo] - off[p]
                out[hi] = out[hi] + off[p]
        return out


# ---- the long-run stream of both test files ----------------------------------------------------------------------------------
LONG = dict(T=400, N=8, taus=(0.1, 0.9), target_alpha=0.2, gamma=0.05, window=50, switch=200, nan_share=0.05)


def long_run_stream(seed):
    """(y [T, 1, N] fp32 with 5 % NaN, raw [2, 1, N] fp32): a Gaussian stream whose sigma goes 1 -> 3 at update 200, under the
    fixed band of the sigma = 1 regime's 0.1 / 0.9 quantiles"""
    L = LONG
    rng = np.random.default_rng(seed)
    sigma = np.where(np.arange(L["T"]) < L["switch"], 1.0, 3.0)[:, None, None]
    y = (rng.normal(size=(L["T"], 1, L["N"])) * sigma).astype(F32)
    y[rng.random(size=y.shape) < L["nan_share"]] = np.nan
    raw = np.empty((2, 1, L["N"]), dtype=F32)
    raw[0], raw[1] = -1.2815516, 1.2815516
    return y, raw


def long_run_bound(T_valid):
    """the theorem's bound on |miss rate - alpha*|: (max(alpha_1, 1 - alpha_1) + gamma) / (gamma T)"""
    a1, g = LONG["target_alpha"], LONG["gamma"]
    return (max(a1, 1.0 - a1) + g) / (g * T_valid)


def long_run_reference(seed):
    """The no-delay protocol on the helper: apply the current offsets, observe, update.  Returns (helper, second-half miss rate
    of the offsets frozen at the switch, number of updates with a valid target)."""
    L = LONG
    y, raw = long_run_stream(seed)
    ref = AciRef([(0, 1)], [1.0 - (L["taus"][1] - L["taus"][0])], L["gamma"], L["window"], True, False, 0, 1, L["N"])
    frozen, fm, fv, t_valid = None, 0, 0, 0
    for t in range(L["T"]):
        if t == L["switch"]:
            frozen = ref.offsets.copy()
        ref.update(y[t], ref.apply(raw), raw)
        ok = ~np.isnan(y[t])
        t_valid += int(ok.any())
        if frozen is not None:
            lo, hi = raw[0] - frozen[0], raw[1] + frozen[0]
            fm += int((ok & ~((lo <= y[t]) & (y[t] <= hi))).sum())
            fv += int(ok.sum())
    return ref, fm / fv, t_valid
