"""numpy restatement of stemgnn_anomaly_update (include/stemgnn_hip.h): the reference of tests/test_anomaly_abi.py and
tests/test_hip_anomaly.py, never the code under test.  fp32 scores in the kernel's operation order, integer counts, the two fp64
expressions (p = (ge + 1) / (m + 1), node_p = min(1, v * pmin)), each rounded once more to fp32."""
import numpy as np

F32 = np.float32


def scores_of(y, lo, hi):
    """s = max(lo - y, y - hi) in fp32, one rounding each: NaN from the forecast -> +inf, -0 -> +0; NaN target -> NaN"""
    y, lo, hi = (np.asarray(v, dtype=F32) for v in (y, lo, hi))
    with np.errstate(invalid="ignore"):
        a, b = (lo - y).astype(F32), (y - hi).astype(F32)
        s = np.where(a > b, a, b).astype(F32)
    s[np.isnan(a) | np.isnan(b)] = F32(np.inf)
    s[s == 0] = F32(0.0)
    s[np.isnan(np.broadcast_to(y, s.shape))] = F32(np.nan)
    return s


class AnomalyRef:
    def __init__(self, alpha, window, per_step, per_node, min_scores, H, N, keep=64):
        self.alpha, self.M, self.min_scores, self.keep = np.float64(alpha), int(window), int(min_scores), int(keep)
        self.per_step, self.per_node, self.H, self.N = bool(per_step), bool(per_node), int(H), int(N)
        self.scores = np.full((self.M, H, N), np.nan, dtype=F32)
        self.pvalues = np.full((H, N), np.nan, dtype=F32)
        self.node_p = np.full(N, np.nan, dtype=F32)
        self.alarm = np.zeros(N, dtype=np.int32)
        self.counts = np.zeros((H if per_step else 1, N if per_node else 1), dtype=np.int64)
        self.alarm_sum, self.judged_sum = np.zeros(N, dtype=np.int64), np.zeros(N, dtype=np.int64)
        self.log_p = np.full((self.keep, N), np.nan, dtype=F32)
        self.log_rows = [-1] * self.keep
        self.n_done = 0

    def update(self, y, f_lo, f_hi=None, present=None, row=None):
        """y [N]; f_lo / f_hi [H, N] the two scored rows of the forecasts of this reading, step h made h rows ago (f_hi None: the
        same row, the absolute residual); present [H] bool: which steps have a stored forecast (default all)."""
        H, N = self.H, self.N
        f_hi = f_lo if f_hi is None else f_hi
        y = np.asarray(y, dtype=F32).reshape(N)
        score = scores_of(y[None, :], np.asarray(f_lo, dtype=F32).reshape(H, N), np.asarray(f_hi, dtype=F32).reshape(H, N))
        if present is not None:
            score[~np.asarray(present, dtype=bool)] = F32(np.nan)
        slot = self.n_done % self.M
        others = np.delete(self.scores, slot, axis=0)                 # the last M - 1 judged rows
        p = np.full((H, N), np.nan, dtype=F32)
        for h in range(H):
            for n in range(N):
                hs = slice(h, h + 1) if self.per_step else slice(None)
                ns = slice(n, n + 1) if self.per_node else slice(None)
                pop = others[:, hs, ns].reshape(-1)
                pop = pop[~np.isnan(pop)]
                m = int(pop.size)
                self.counts[h if self.per_step else 0, n if self.per_node else 0] = m
                if np.isnan(score[h, n]) or m < self.min_scores:
                    continue
                ge = int((pop >= score[h, n]).sum())                  # IEEE: -0 == +0, +inf largest
                p[h, n] = F32(np.float64(ge + 1) / np.float64(m + 1))
        self.scores[slot] = score
        self.pvalues = p
        for n in range(N):
            ok = p[:, n][~np.isnan(p[:, n])]
            v = int(ok.size)
            if v:
                self.node_p[n] = F32(min(np.float64(1.0), np.float64(v) * np.float64(ok.min())))
                self.alarm[n] = int(np.float64(self.node_p[n]) <= self.alpha)
            else:
                self.node_p[n], self.alarm[n] = F32(np.nan), 0
            self.judged_sum[n] += int(v > 0)
            self.alarm_sum[n] += int(self.alarm[n])
        self.log_p[self.n_done % self.keep] = self.node_p
        self.log_rows[self.n_done % self.keep] = self.n_done if row is None else int(row)
        self.n_done += 1

    def recent(self):
        k = min(self.n_done, self.keep)
        order = [(self.n_done - k + i) % self.keep for i in range(k)]
        return self.log_p[order].copy(), np.array([self.log_rows[s] for s in order], dtype=np.int64)


class AnomalyRefFast(AnomalyRef):
    """AnomalyRef with update() restated per GROUP instead of per element, for the wide cases of the serving stage suite
    (tests/test_serving_cases.py proves it equal to the loop on the small cases): a group's population is sorted once and every
    query of the group meets it through np.searchsorted -- `side="left"` counts the scores below the query in IEEE order
    (-0 == +0, +inf largest), the rest are >= it.  The per-node combination is the same fp64 expression on whole rows."""

    def update(self, y, f_lo, f_hi=None, present=None, row=None):
        H, N, M = self.H, self.N, self.M
        f_hi = f_lo if f_hi is None else f_hi
        y = np.asarray(y, dtype=F32).reshape(N)
        score = scores_of(y[None, :], np.asarray(f_lo, dtype=F32).reshape(H, N), np.asarray(f_hi, dtype=F32).reshape(H, N))
        if present is not None:
            score[~np.asarray(present, dtype=bool)] = F32(np.nan)
        slot = self.n_done % M
        others = np.delete(self.scores, slot, axis=0)                 # [M - 1, H, N]
        Hg, Ng = self.counts.shape
        # [Hg, Ng, population of the group] and [Hg, Ng, queries of the group], the queries with their (h, n)
        pop = others.transpose(1, 2, 0) if self.per_step else others.transpose(2, 0, 1).reshape(1, N, -1)
        pop = pop if self.per_node else pop.reshape(Hg, 1, -1)
        hh, nn = np.meshgrid(np.arange(H), np.arange(N), indexing="ij")
        p = np.full((H, N), np.nan, dtype=F32)
        for hg in range(Hg):
            for ng in range(Ng):
                s = np.sort(pop[hg, ng])                              # NaN last
                m = int(s.size - np.isnan(s).sum())
                self.counts[hg, ng] = m
                if m < self.min_scores:
                    continue
                sel = (hh == hg if self.per_step else np.ones((H, N), bool)) & (nn == ng if self.per_node else np.ones((H, N), bool))
                q = score[sel]
                ge = m - np.searchsorted(s[:m], q, side="left")
                with np.errstate(invalid="ignore"):
                    pv = (np.float64(1) + ge.astype(np.float64)) / np.float64(m + 1)
                p[sel] = np.where(np.isnan(q), np.nan, pv).astype(F32)
        self.scores[slot] = score
        self.pvalues = p
        ok = ~np.isnan(p)
        v = ok.sum(axis=0)
        pmin = np.where(ok, p, F32(np.inf)).min(axis=0).astype(np.float64)
        with np.errstate(invalid="ignore"):                           # v = 0: 0 * inf, replaced below
            node = np.minimum(np.float64(1.0), v.astype(np.float64) * pmin).astype(F32)
        self.node_p = np.where(v > 0, node, F32(np.nan)).astype(F32)
        self.alarm = ((v > 0) & (self.node_p.astype(np.float64) <= self.alpha)).astype(np.int32)
        self.judged_sum += (v > 0)
        self.alarm_sum += self.alarm
        self.log_p[self.n_done % self.keep] = self.node_p
        self.log_rows[self.n_done % self.keep] = self.n_done if row is None else int(row)
        self.n_done += 1


# ---- the validity / power stream of both test files ----------------------------------------------------------------------------
VALID = dict(T=1500, N=8, H=2, window=64, min_scores=32, alpha=0.1, spikes=((700, 3), (701, 3), (1200, 5)), spike=8.0)


def validity_stream(seed):
    """y [T, N] fp32 iid normal with +8 spikes; the forecast is 0 at both steps"""
    V = VALID
    y = np.random.default_rng(seed).normal(size=(V["T"], V["N"])).astype(F32)
    for t, n in V["spikes"]:
        y[t, n] += F32(V["spike"])
    return y


def validity_reference(seed):
    """(helper after the whole stream, the alarm flags [T, N] it raised)"""
    V = VALID
    y = validity_stream(seed)
    ref = AnomalyRef(V["alpha"], V["window"], True, True, V["min_scores"], V["H"], V["N"])
    zero, flags = np.zeros((V["H"], V["N"]), dtype=F32), np.zeros((V["T"], V["N"]), dtype=np.int32)
    for t in range(V["T"]):
        ref.update(y[t], zero)
        flags[t] = ref.alarm
    return ref, flags
