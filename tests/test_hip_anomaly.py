"""GPU: conformal anomaly p-values for live readings -- the kernel of csrc/anomaly.hip, math_utils.ConformalAnomaly and
LiveForecaster.set_anomaly on top of it.

The reference of everything is tests/helpers/anomaly_ref.py (numpy: fp32 scores, integer counts, the two fp64 expressions), never
the code under test; every comparison is one of bit patterns (NaN-aware where NaN means "absent").  There is no tolerance in this
file; the one inequality is alpha / 4 <= false-alarm rate <= alpha on the helper's own stream (derived: with both steps equal the
rate at a full window is floor(0.05 * 64) / 64 = 3 / 64).  One fixed seed."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import anomaly_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261020
GROUPINGS = ((True, False), (True, True), (False, False), (False, True))       # (per_step, per_node)
CASES = ((1, 2, 11, (0, 0)), (3, 3, 12, (1, 1)), (3, 3, 12, (0, 2)))            # (R, H, N, rows): scalar path, 16-byte path
M, ROWS, S, RING, KEEP, MIN_SCORES, ALPHA = 5, 17, 4, 7, 3, 3, 0.625
SKIPPED, ALL_NAN = 9, 6                       # the origin never stored (its slot keeps a stale one) / the row without a target
LONG = ((1, 5, 11, (0, 0)),)                  # H > 4: the column form spreads the steps over workgroups; S < H: step 4 is overwritten
STATE = ("scores", "pvalues", "node_p", "alarm", "counts", "alarm_sum", "judged_sum")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def same_nan_aware(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def state_matches(ref, st, what, log_slot=None):
    for k in STATE:
        got, want = getattr(st, k), torch.from_numpy(getattr(ref, k))
        ok = same_nan_aware(got, want) if got.dtype == torch.float32 else (got.dtype == want.dtype and torch.equal(got.cpu(), want))
        assert ok, (what, k, got, want)
    if log_slot is not None:
        assert same_nan_aware(st.log_p[log_slot], torch.from_numpy(ref.log_p[log_slot])), (what, "log_p")


_streams = {}


def stream(R, H, N, full):
    """Readings y [T, N] and forecasts F[o] [R, H, N] (origin o, step h = the forecast of row o + h) on a grid of quarters: exact
    ties in and across window slots, scores of exactly 0.  full=False: rows 0 .. 16 (tau < h at the start), origin SKIPPED never
    stored, scattered NaN targets, one row without any, a NaN forecast on a valid target, (y, f) = (+0, -0).  full=True: rows
    3 .. 19 with every origin stored, so every step is present (the form without origins can say the same)."""
    key = (R, H, N, full)
    if key in _streams:
        return _streams[key]
    rng = np.random.default_rng(SEED + 10 * R + N + (1 if full else 0))
    first = 3 if full else 0
    taus = list(range(first, first + ROWS))
    T = taus[-1] + 1
    y = (np.round(rng.normal(size=(T, N)) * 4) / 4).astype(np.float32)
    centre = np.round(rng.normal(size=(T, 1, H, N)) * 2) / 4
    half = np.linspace(0.25, 1.0, R // 2)[::-1].reshape(1, -1, 1, 1)
    F = np.concatenate([centre - half] + ([centre] if R % 2 else []) + [centre + half[:, ::-1]], axis=1).astype(np.float32)
    y[rng.random(size=y.shape) < 0.12] = np.nan
    store = {tau: [tau] for tau in taus}
    if full:
        store[first] = [1, 2, 3]
    else:
        store[SKIPPED] = []
        y[ALL_NAN] = np.nan
    # (late rows: their scores are still in the window when the sequence ends)
    t0 = taus[-1]
    y[t0 - 2, 4], F[t0 - 3, :, 1, 4] = 0.5, np.nan                   # row t0-2, step 1 (origin t0-3): NaN forecast, valid target
    y[t0 - 1, 2], F[t0 - 1, R - 1, 0, 2] = -0.25, np.nan             # row t0-1, step 0: the upper (or only) row is NaN
    y[t0 - 3, 1], F[t0 - 3, :, 0, 1] = 0.0, 1.0
    F[t0 - 3, : max(1, R - 1), 0, 1] = -0.0                          # (y, f_lo) = (+0, -0): the score -0 is stored as +0
    y[t0, 0], F[t0 - 1, :, 1, 0] = 0.75, 0.75                        # a score of exactly +0
    _streams[key] = types.SimpleNamespace(y=y, F=F, taus=taus, store=store)
    return _streams[key]


def opinions(st, tau, H, rows, stored):
    """what the helper is fed for row tau: f_lo / f_hi [H, N] and which steps have a stored forecast"""
    N = st.y.shape[1]
    f_lo, f_hi, present = np.zeros((H, N), np.float32), np.zeros((H, N), np.float32), np.zeros(H, bool)
    for h in range(H):
        o = tau - h
        if o >= 0 and o in stored:
            f_lo[h], f_hi[h], present[h] = st.F[o, rows[0], h], st.F[o, rows[1], h], True
    return f_lo, f_hi, present


def fresh_state(H, N, per_step, per_node, st=None):
    """the entry's buffers: new and full of junk, or re-initialised in place (what is written in full stays dirty)"""
    if st is None:
        shapes = dict(scores=(M, H, N), pvalues=(H, N), node_p=(N,), alarm=(N,), counts=(H if per_step else 1, N if per_node else 1),
                      alarm_sum=(N,), judged_sum=(N,), log_p=(KEEP, N), work=(2 * H * N,))
        types_ = dict(alarm=torch.int32, counts=torch.int64, alarm_sum=torch.int64, judged_sum=torch.int64, work=torch.int32)
        st = types.SimpleNamespace(**{k: torch.full(s, 77, dtype=types_.get(k, torch.float32), device=DEV) for k, s in shapes.items()})
    st.scores.fill_(float("nan"))
    st.alarm_sum.zero_()
    st.judged_sum.zero_()
    st.work.zero_()
    return st


# ---- 1. the kernel against the helper, update by update ------------------------------------------------------------------------
@pytest.mark.parametrize("per_step,per_node", GROUPINGS)
@pytest.mark.parametrize("R,H,N,rows", CASES + LONG)
def test_kernel_equals_the_helper_update_by_update(R, H, N, rows, per_step, per_node):
    from stemgnn_amd import ops
    inp = stream(R, H, N, False)
    st, finals = None, []
    for run in range(2):
        st = fresh_state(H, N, per_step, per_node, st)               # the second run: dirty buffers, re-initialised
        ref = anomaly_ref.AnomalyRef(ALPHA, M, per_step, per_node, MIN_SCORES, H, N, keep=KEEP)
        rng = np.random.default_rng(SEED + run)
        slab = dev(rng.normal(size=(S, R, H, N)).astype(np.float32))
        origins = torch.full((S,), -1, dtype=torch.int64, device=DEV)
        ring = dev(rng.normal(size=(RING, N)).astype(np.float32))
        stored = set()
        for u, tau in enumerate(inp.taus):
            for o in inp.store[tau]:
                slab[o % S].copy_(dev(inp.F[o]))
                origins[o % S] = o
                stored = {p for p in stored if p % S != o % S} | {o}
            ring[tau % RING].copy_(dev(inp.y[tau]))
            f_lo, f_hi, present = opinions(inp, tau, H, rows, stored)
            ref.update(inp.y[tau], f_lo, f_hi, present, row=tau)
            assert all(t.data_ptr() % 16 == 0 for t in (slab, ring, st.scores))         # N % 4 alone picks the path
            ops.anomaly_update(slab, origins, tau, ring, rows, u % M, MIN_SCORES, ALPHA, per_step, per_node, st.scores,
                               st.pvalues, st.node_p, st.alarm, st.counts, st.alarm_sum, st.judged_sum, st.log_p, u % KEEP, st.work)
            state_matches(ref, st, (run, tau), log_slot=u % KEEP)
            if tau == 0:
                assert not present[1:].any() and np.isnan(ref.pvalues).all()          # tau < h, and the window is empty
            if tau == SKIPPED + 1:
                assert not present[1] and present[0], "a stale origin in the slot"
            if tau == ALL_NAN:
                assert np.isnan(ref.node_p).all() and not ref.alarm.any()
            if u < MIN_SCORES and per_step and per_node:
                assert np.isnan(ref.pvalues).all(), "held until min_scores"
        finals.append({k: getattr(st, k).clone() for k in STATE})
        # the inputs held what they promise
        s = ref.scores
        assert np.isinf(s).any() and (s == 0).any() and not (s.view(np.uint32) == 0x80000000).any()
        flat = s[~np.isnan(s)]
        assert flat.size - np.unique(flat).size > 10, "exact ties across the window"
        assert ref.alarm_sum.sum() > 0 and (ref.judged_sum < ROWS).all() and ref.judged_sum.sum() > 0
    for k, v in finals[0].items():
        assert same_nan_aware(v, finals[1][k]) if v.dtype == torch.float32 else torch.equal(v, finals[1][k]), k


@pytest.mark.parametrize("per_step,per_node", GROUPINGS)
@pytest.mark.parametrize("R,H,N,rows", CASES)
def test_without_origins_equals_the_slab_form(R, H, N, rows, per_step, per_node):
    """origins = NULL with the diagonal gathered by the caller into [1, R, H, N]: the slab form's bits, and the helper's"""
    from stemgnn_amd import ops
    inp = stream(R, H, N, True)
    a, b = fresh_state(H, N, per_step, per_node), fresh_state(H, N, per_step, per_node)
    ref = anomaly_ref.AnomalyRef(ALPHA, M, per_step, per_node, MIN_SCORES, H, N, keep=KEEP)
    slab = torch.zeros(S, R, H, N, device=DEV)
    origins = torch.full((S,), -1, dtype=torch.int64, device=DEV)
    ring = torch.zeros(RING, N, device=DEV)
    for u, tau in enumerate(inp.taus):
        for o in inp.store[tau]:
            slab[o % S].copy_(dev(inp.F[o]))
            origins[o % S] = o
        ring[tau % RING].copy_(dev(inp.y[tau]))
        diag = np.stack([inp.F[tau - h, :, h] for h in range(H)], axis=1)             # [R, H, N]
        ref.update(inp.y[tau], diag[rows[0]], diag[rows[1]], row=tau)
        for st, args in ((a, (slab, origins, tau, ring)), (b, (dev(diag)[None], None, tau, dev(inp.y[tau])[None]))):
            ops.anomaly_update(*args, rows, u % M, MIN_SCORES, ALPHA, per_step, per_node, st.scores, st.pvalues, st.node_p,
                               st.alarm, st.counts, st.alarm_sum, st.judged_sum, st.log_p, u % KEEP, st.work)
            state_matches(ref, st, tau, log_slot=u % KEEP)
    assert ref.alarm_sum.sum() > 0


@pytest.mark.parametrize("per_step", (False, True), ids=("all", "step"))
@pytest.mark.parametrize("N", (2050, 2052, 4100), ids=("scalar", "16-byte", "wide"))
def test_pooled_beyond_one_sorted_batch_and_one_workgroup(N, per_step):
    """pooled over the nodes with more than 4096 queries in a group (H * N = 4100 / 4104 over everything, N = 4100 per step: two
    sorted batches) and a window of more than 8192 keys (dealt over several workgroups, which meet in the work buffer)"""
    from stemgnn_amd import ops
    H, U = 2, 4
    rng = np.random.default_rng(SEED + 7)
    y = (np.round(rng.normal(size=(U, N)) * 4) / 4).astype(np.float32)
    y[rng.random(size=y.shape) < 0.1] = np.nan
    f = (np.round(rng.normal(size=(U, H, N)) * 2) / 4).astype(np.float32)
    st = fresh_state(H, N, per_step, False)
    for u in range(U):
        ops.anomaly_update(dev(f[u])[None, None], None, u, dev(y[u])[None], (0, 0), u % M, MIN_SCORES, ALPHA, per_step, False,
                           st.scores, st.pvalues, st.node_p, st.alarm, st.counts, st.alarm_sum, st.judged_sum, st.log_p, u % KEEP,
                           st.work)
    torch.cuda.synchronize()
    scores = np.full((M, H, N), np.nan, dtype=np.float32)            # (the helper's loop, vectorised: np.sort + searchsorted)
    for u in range(U):
        score = anomaly_ref.scores_of(y[u][None], f[u], f[u])
        others = np.delete(scores, u % M, axis=0)
        p, counts = np.full((H, N), np.nan, dtype=np.float32), []
        for hs in ([slice(h, h + 1) for h in range(H)] if per_step else [slice(None)]):
            pop = others[:, hs].reshape(-1)
            pop = np.sort(pop[~np.isnan(pop)])
            ge = pop.size - np.searchsorted(pop, score[hs], side="left")
            p[hs] = ((ge + 1).astype(np.float64) / np.float64(pop.size + 1)).astype(np.float32)
            if pop.size < MIN_SCORES:
                p[hs] = np.nan
            counts.append(pop.size)
        p[np.isnan(score)] = np.nan
        scores[u % M] = score
    assert same_nan_aware(st.scores, torch.from_numpy(scores)) and same_nan_aware(st.pvalues, torch.from_numpy(p))
    assert st.counts.reshape(-1).tolist() == counts and M * N * (1 if per_step else H) > 8192 and min(counts) > 4096
    with np.errstate(invalid="ignore"):
        v, pmin = (~np.isnan(p)).sum(axis=0), np.where(np.isnan(p), np.inf, p).min(axis=0)
        want = np.where(v > 0, np.minimum(1.0, v * pmin.astype(np.float64)), np.nan).astype(np.float32)
    assert same_nan_aware(st.node_p, torch.from_numpy(want))
    assert torch.equal(st.alarm.cpu(), torch.from_numpy((want.astype(np.float64) <= ALPHA).astype(np.int32)))
    assert not bool(st.work.any()), "the work buffer is left zero"


@pytest.mark.parametrize("per_step", (True, False), ids=("step_node", "node"))
def test_long_horizon_rows_dealt_over_workgroups(per_step):
    """per_node with H = 5 > 4 and a window of 70 slots: the column form deals the window's rows over several workgroups (3 of 32
    rows per step, 11 with the steps pooled), which meet in the work buffer; the window wraps once"""
    from stemgnn_amd import ops
    H, N, MW, U = 5, 11, 70, 75
    rng = np.random.default_rng(SEED + 11)
    y = (np.round(rng.normal(size=(U, N)) * 4) / 4).astype(np.float32)
    y[rng.random(size=y.shape) < 0.1] = np.nan
    f = (np.round(rng.normal(size=(U, H, N)) * 2) / 4).astype(np.float32)
    ref = anomaly_ref.AnomalyRef(ALPHA, MW, per_step, True, MIN_SCORES, H, N, keep=KEEP)
    st = fresh_state(H, N, per_step, True)
    st.scores = torch.full((MW, H, N), float("nan"), device=DEV)
    y_d, f_d = dev(y), dev(f)
    for u in range(U):
        ops.anomaly_update(f_d[u][None, None], None, u, y_d[u][None], (0, 0), u % MW, MIN_SCORES, ALPHA, per_step, True, st.scores,
                           st.pvalues, st.node_p, st.alarm, st.counts, st.alarm_sum, st.judged_sum, st.log_p, u % KEEP, st.work)
        ref.update(y[u], f[u])
        if u % 9 == 0 or u >= U - 3:
            state_matches(ref, st, u, log_slot=u % KEEP)
    assert int(ref.counts.max()) > 32 * (1 if per_step else H) and ref.alarm_sum.sum() > 0
    assert not bool(st.work.any()), "the work buffer is left zero"


# ---- 2. ConformalAnomaly against the helper ------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_step,per_node", ((True, True), (False, False)))
def test_conformal_anomaly_both_update_forms_recent_report_and_state(per_step, per_node):
    from stemgnn_amd.math_utils import ConformalAnomaly
    R, H, N, rows = 3, 3, 12, (0, 2)
    kw = dict(alpha=ALPHA, window=M, per_step=per_step, per_node=per_node, min_scores=MIN_SCORES, score="band", keep=KEEP)
    # the slab form, with a restart through CPU tensors in mid-sequence
    inp = stream(R, H, N, False)
    det, again = ConformalAnomaly(**kw), None
    ref = anomaly_ref.AnomalyRef(ALPHA, M, per_step, per_node, MIN_SCORES, H, N, keep=KEEP)
    slab, origins = torch.zeros(S, R, H, N, device=DEV), torch.full((S,), -1, dtype=torch.int64, device=DEV)
    ring, stored = torch.zeros(RING, N, device=DEV), set()
    for u, tau in enumerate(inp.taus):
        for o in inp.store[tau]:
            slab[o % S].copy_(dev(inp.F[o]))
            origins[o % S] = o
            stored = {p for p in stored if p % S != o % S} | {o}
        ring[tau % RING].copy_(dev(inp.y[tau]))
        ref.update(inp.y[tau], *opinions(inp, tau, H, rows, stored), row=tau)
        for d in (det, again):
            if d is not None:
                d.update(None, None, slab=slab, origins=origins, row=tau, ring=ring, rows=rows)
                state_matches(ref, d, (tau, d is again), log_slot=u % KEEP)
                got, got_rows = d.recent()
                want, want_rows = ref.recent()
                assert same_nan_aware(got, torch.from_numpy(want)) and got_rows.tolist() == want_rows.tolist()
                assert d.n_done == u + 1 and d.last_row == tau
        if u == 8:
            state = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in det.state_dict().items()}
            again = ConformalAnomaly(**kw).load_state_dict(state, device=DEV)
            assert again.n_done == 9 and again.scores.device.type == "cuda"
    rep = det.report()
    for k in ("pvalues", "node_p", "alarm", "counts", "alarm_sum", "judged_sum"):
        want = getattr(ref, k)
        assert rep[k].dtype == want.dtype and np.array_equal(rep[k], want, equal_nan=rep[k].dtype == np.float32), k
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(rep["alarm_rate"], np.where(ref.judged_sum > 0, ref.alarm_sum / ref.judged_sum, np.nan), equal_nan=True)
    assert np.array_equal(rep["resolution"], 1.0 / (ref.counts + 1.0)) and rep["n_done"] == ROWS and rep["row"] == inp.taus[-1]
    # the plain form: y [N] and the gathered forecasts [R, H, N] / [H, N]
    inp = stream(R, H, N, True)
    band, point = ConformalAnomaly(**kw), ConformalAnomaly(**dict(kw, score="point"))
    rb = anomaly_ref.AnomalyRef(ALPHA, M, per_step, per_node, MIN_SCORES, H, N, keep=KEEP)
    rp = anomaly_ref.AnomalyRef(ALPHA, M, per_step, per_node, MIN_SCORES, H, N, keep=KEEP)
    for u, tau in enumerate(inp.taus):
        diag = np.stack([inp.F[tau - h, :, h] for h in range(H)], axis=1)
        rb.update(inp.y[tau], diag[0], diag[2])
        rp.update(inp.y[tau], diag[1])
        band.update(dev(inp.y[tau]), dev(diag))
        point.update(dev(inp.y[tau]), dev(diag[1]))
        state_matches(rb, band, ("band", tau), log_slot=u % KEEP)
        state_matches(rp, point, ("point", tau), log_slot=u % KEEP)
    assert band.recent()[1].tolist() == [ROWS - 3, ROWS - 2, ROWS - 1]


# ---- 3. LiveForecaster end to end ----------------------------------------------------------------------------------------------
W, MULTI, H_MODEL, HORIZON, HISTORY, UNITS, T = 4, 2, 2, 5, 8, 6, 64
C_LIVE = W + HORIZON + HISTORY
LIVE_TAUS = (0.1, 0.5, 0.9)
_live = {}


def live_reference():
    """the raw series [T, 6] with missing readings, its statistics, and the dataset's target rows [T, 6] (NaN = missing)"""
    if not _live:
        from stemgnn_amd.forecast_dataloader import ForecastDataset
        rng = np.random.default_rng(SEED + 300)
        series = rng.normal(loc=3.0, scale=2.0, size=(T, UNITS))
        series[series == 0.0] = 1.0
        for t, n, v in ((5, 1, 0.0), (6, 1, 0.0), (9, 3, np.nan), (17, 0, 0.0), (18, 0, np.nan), (23, 5, np.nan), (30, 5, 0.0),
                        (58, 2, 0.0), (61, 4, np.nan)):
            series[t, n] = v
        stat = dict(mean=rng.normal(3.0, 0.5, size=UNITS), std=rng.uniform(1.0, 3.0, size=UNITS))
        ds = ForecastDataset(series, W, H_MODEL, "z_score", dict(stat), missing=0.0, device=DEV)
        _live.update(series=series, stat=stat, target=ds.target.cpu().numpy())
        assert np.isnan(_live["target"]).sum() == 9
    return _live


def model_of(quant):
    key = ("model", quant)
    if key not in _live:
        from stemgnn_amd import Model
        torch.manual_seed(SEED + (1000 if quant else 0))
        _live[key] = Model(UNITS, 2, W, MULTI, horizon=H_MODEL, **(dict(quantiles=LIVE_TAUS) if quant else {})).to(DEV).eval()
    return _live[key]


def make_live(quant, graph):
    from stemgnn_amd import LiveForecaster
    return LiveForecaster(model_of(quant), W, HORIZON, normalize_method="z_score", norm_statistic=dict(live_reference()["stat"]),
                          missing=0.0, history=HISTORY, graph=graph)


LIVE_CASES = ((False, "point", True, True, 0.875), (True, "band", False, False, 0.25), (True, "point", True, False, 0.5))


@pytest.mark.parametrize("graph", (True, False), ids=("graph", "eager"))
@pytest.mark.parametrize("quant,score,per_step,per_node,alpha", LIVE_CASES)
def test_live_forecaster_with_a_detector(quant, score, per_step, per_node, alpha, graph):
    from stemgnn_amd.math_utils import ConformalAnomaly
    L = live_reference()
    series, target = L["series"], L["target"]
    kw = dict(alpha=alpha, window=6, per_step=per_step, per_node=per_node, min_scores=2, score=score, keep=4)
    rows = (0, 0) if not quant else ((0, 2) if score == "band" else (1, 1))
    twin, live, det = make_live(quant, graph), make_live(quant, graph), ConformalAnomaly(**kw)
    live.set_anomaly(det)
    ref = anomaly_ref.AnomalyRef(alpha, 6, per_step, per_node, 2, HORIZON, UNITS, keep=4)
    kept, resumed, replay = {}, None, None

    def judge(first, count):
        """the helper's side of a push of rows first .. first + count - 1"""
        for tau in range(max(first, first + count - C_LIVE), first + count):
            f_lo, f_hi = np.zeros((HORIZON, UNITS), np.float32), np.zeros((HORIZON, UNITS), np.float32)
            present = np.zeros(HORIZON, bool)
            for h in range(HORIZON):
                f = kept.get(tau - h)
                if f is not None:
                    f = f.reshape(-1, HORIZON, UNITS)
                    f_lo[h], f_hi[h], present[h] = f[rows[0], h], f[rows[1], h], True
            if present.any():
                ref.update(target[tau], f_lo, f_hi, present, row=tau)

    def check(what):
        for lv in (live,) + ((resumed,) if resumed is not None else ()):
            d = lv.anomaly
            node_p, alarm, row = lv.anomalies()
            assert d.n_done == ref.n_done and row == (ref.recent()[1][-1] if ref.n_done else -1), what
            assert node_p is d.node_p and alarm is d.alarm
            state_matches(ref, d, what)
            got, got_rows = d.recent()
            want, want_rows = ref.recent()
            assert same_nan_aware(got, torch.from_numpy(want)) and got_rows.tolist() == want_rows.tolist(), what

    t = W
    for lv in (twin, live):
        assert lv.push(series[:W]) == W                              # the bulk load of history: nothing to judge
    assert det.n_done == 0 and det.last_row == -1
    check("bulk")
    plan = {12: 2, 20: "off", 26: "save", 30: C_LIVE + HORIZON}     # rows pushed after the forecast at t (default 1)
    while t < T:
        want = twin.forecast()
        assert same_bits(live.forecast(), want), t                   # the detector changes nothing the forecast returns
        if resumed is not None:
            assert same_bits(resumed.forecast(), want), t
        kept[t] = want.cpu().numpy()
        for o in [o for o in kept if o <= t - HISTORY]:
            del kept[o]                                              # overwritten in the slab
        if replay is None:
            replay = live._replay
            assert (replay is not None) == graph
        step = plan.get(t, 1)
        if step == "off":                                            # the detector off for one row, then on again: it continues
            live.set_anomaly(None)
            for lv in (twin, live):
                lv.push(series[t])
            assert det.n_done == ref.n_done and "anomaly" not in live.state_dict()
            live.set_anomaly(det)
            t += 1
            continue
        if step == "save":                                           # a restart in mid-stream, as if read from disk
            state = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in live.state_dict().items()}
            state["anomaly"] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in state["anomaly"].items()}
            resumed = make_live(quant, graph)
            resumed.set_anomaly(ConformalAnomaly(**kw))
            resumed.load_state_dict(state)
            assert resumed.rows == t and resumed.anomaly.n_done == det.n_done
            step = 1
        step = min(step, T - t)
        before = det.n_done
        for lv in (twin, live) + ((resumed,) if resumed is not None else ()):
            assert lv.push(series[t:t + step]) == t + step
        if step > C_LIVE:                                            # no row still in the ring has a stored forecast
            assert det.n_done == before
        else:
            assert det.n_done == before + step                       # two rows in one push: two updates, in order
        judge(t, step)
        check(t)
        t += step
    assert live._replay is replay, "never captured again"
    assert ref.n_done > 6 * 4 and np.isnan(ref.scores).any() and ref.judged_sum.sum() > 0
    assert "anomaly" not in twin.state_dict() and twin.anomaly is None


# ---- 4. validity and power ------------------------------------------------------------------------------------------------------
def test_false_alarm_rate_is_bounded_and_spikes_are_flagged():
    from stemgnn_amd.math_utils import ConformalAnomaly
    V = anomaly_ref.VALID
    y = anomaly_ref.validity_stream(SEED)
    ref, ref_flags = anomaly_ref.validity_reference(SEED)
    det = ConformalAnomaly(alpha=V["alpha"], window=V["window"], min_scores=V["min_scores"])
    y_d, zero = dev(y), torch.zeros(V["H"], V["N"], device=DEV)
    flags = torch.zeros(V["T"], V["N"], dtype=torch.int32, device=DEV)
    for t in range(V["T"]):                                          # on the device throughout: no sync inside the loop
        det.update(y_d[t], zero)
        flags[t].copy_(det.alarm)
    rep = det.report()                                               # the one sync
    assert np.array_equal(rep["alarm_sum"], ref.alarm_sum) and np.array_equal(rep["judged_sum"], ref.judged_sum)
    assert np.array_equal(flags.cpu().numpy(), ref_flags)
    rate = ref.alarm_sum.sum() / ref.judged_sum.sum()
    print(f"validity: false-alarm rate {rate:.4f} at alpha {V['alpha']}, {int(ref.judged_sum.sum())} judged")
    assert int(ref.judged_sum.sum()) == 11744 and V["alpha"] / 4 <= rate <= V["alpha"]
    for t, n in V["spikes"]:
        assert ref_flags[t, n] == 1, (t, n)
    state_matches(ref, det, "validity")
