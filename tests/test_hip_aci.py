"""GPU: adaptive conformal bands -- the update kernel of csrc/aci.hip, math_utils.AdaptiveConformal and
LiveForecaster.set_adaptive on top of it.

The reference of everything is tests/helpers/aci_ref.py (numpy: fp32 scores, fp64 alpha in the kernel's operation order, np.sort
for the k-th value), never the code under test; every comparison is one of bit patterns (NaN-aware where NaN means "absent").
There is no tolerance in this file; the one inequality is the theorem's long-run bound, (max(alpha_1, 1 - alpha_1) + gamma) /
(gamma T) = 0.0425 for the stream used, derived, not measured.  One fixed seed.

A remark on case 2 (gamma = 0 against ConformalCalibrator.fit).  A group with no valid target in the newest forecast keeps its
offset (step 3 of the entry's contract), while a fit of the window would recompute it; with per_step and per_node a group has ONE
element per forecast, so every NaN target is such a hold.  The expected offset is therefore the fit's wherever the group had a
valid target in the newest forecast, and the offset before otherwise; counts are the fit's everywhere."""
import types

import numpy as np
import pytest
import torch

from tests.helpers import aci_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261019
GROUPINGS = ((True, False), (True, True), (False, False), (False, True))       # (per_step, per_node)
SHAPES = ((3, 2, 11), (5, 3, 12))                                               # (Q, H, N): scalar path, 16-byte path
TAUS = {3: (0.1, 0.5, 0.9), 5: (0.05, 0.25, 0.5, 0.75, 0.95)}
M, UPDATES, RING = 5, 17, 7
NO_VALID_ROW, NO_VALID_ALL = 6, 9             # updates whose row h = 0 and column 3 / whose whole target are NaN


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def same_nan_aware(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pairs_of(Q):
    return tuple((i, Q - 1 - i) for i in range(Q // 2))


def alphas_of(Q):
    t = TAUS[Q]
    return [1.0 - float(np.float64(t[hi]) - np.float64(t[lo])) for lo, hi in pairs_of(Q)]


def state_matches(ref, st, what):
    assert same_nan_aware(st.scores, torch.from_numpy(ref.scores)), what
    assert same_bits(st.alpha, torch.from_numpy(ref.alpha)), what
    assert same_bits(st.offsets, torch.from_numpy(ref.offsets)), what
    for k in ("counts", "miss_sum", "valid_sum"):
        assert torch.equal(getattr(st, k).cpu(), torch.from_numpy(getattr(ref, k))), (what, k)


_inputs = {}


def inputs(Q, H, N, holes=True):
    """UPDATES forecasts on a grid of quarters (exact ties across window slots, scores of exactly 0): y [U,H,N] with scattered NaN,
    raw [U,Q,H,N], the origins (they wrap the ring of RING slots).  holes: the two updates in which whole groups have no valid
    target.  Also: a NaN forecast row on a valid target, and (y, lo) = (+0, -0), whose score -0 must be stored as +0."""
    key = (Q, H, N, holes)
    if key in _inputs:
        return _inputs[key]
    rng = np.random.default_rng(SEED + 10 * Q + N + (1 if holes else 0))
    y = (np.round(rng.normal(size=(UPDATES, H, N)) * 4) / 4).astype(np.float32)
    centre = np.round(rng.normal(size=(UPDATES, 1, H, N)) * 2) / 4
    half = np.linspace(0.25, 1.5, Q // 2)[::-1].reshape(1, -1, 1, 1)
    raw = np.concatenate([centre - half] + ([centre] if Q % 2 else []) + [centre + half[:, ::-1]], axis=1).astype(np.float32)
    y[rng.random(size=y.shape) < 0.12] = np.nan
    # (late updates: their scores are still in the window when the sequence ends)
    y[14, 1, 4], raw[14, 0, 1, 4] = 0.5, np.nan                     # a NaN forecast on a valid target: score +inf, a miss
    y[15, 0, 2], raw[15, Q - 1, 0, 2] = -0.25, np.nan
    y[13, 0, 1], raw[13, 0, 0, 1], raw[13, Q - 1, 0, 1] = 0.0, -0.0, 1.0         # max(-0 - 0, 0 - 1) = -0
    y[16, 1, 0], raw[16, 0, 1, 0], raw[16, Q - 1, 1, 0] = 0.75, 0.75, 2.0        # max(+0, ..) = +0
    if holes:
        y[NO_VALID_ROW, 0, :], y[NO_VALID_ROW, :, 3] = np.nan, np.nan
        y[NO_VALID_ALL] = np.nan
    else:
        y[1, 0, 0] = y[7, 1, 5] = np.nan
    origins = [3 + 2 * u for u in range(UPDATES)]
    assert max(o % RING + H for o in origins) > RING, "some origin's targets wrap the ring"
    _inputs[key] = types.SimpleNamespace(y=y, raw=raw, origins=origins)
    return _inputs[key]


def ring_of(y, origin, N, rng):
    """a [RING, N] ring of junk with target row h at slot (origin + h) mod RING"""
    ring = rng.normal(size=(RING, N)).astype(np.float32)
    for h in range(y.shape[0]):
        ring[(origin + h) % RING] = y[h]
    return ring


def fresh_state(Q, H, N, per_step, per_node, st=None):
    """the entry's state buffers, new or re-initialised in place"""
    P = Q // 2
    shape = (P, H if per_step else 1, N if per_node else 1)
    if st is None:
        st = types.SimpleNamespace(scores=torch.empty(M, P, H, N, device=DEV), alpha=torch.empty(shape, dtype=torch.float64, device=DEV),
                                   offsets=torch.empty(shape, device=DEV),
                                   **{k: torch.empty(shape, dtype=torch.int64, device=DEV) for k in ("counts", "miss_sum", "valid_sum")})
    st.scores.fill_(float("nan"))
    st.alpha.copy_(torch.tensor(alphas_of(Q), dtype=torch.float64).reshape(P, 1, 1).expand(shape))
    st.offsets.zero_()
    for k in ("counts", "miss_sum", "valid_sum"):
        getattr(st, k).zero_()
    return st


# ---- 1. the kernel against the helper, update by update ------------------------------------------------------------------------
def update_sequence(Q, H, N, per_step, per_node):
    from stemgnn_amd import ops
    inp, pairs, ta = inputs(Q, H, N), pairs_of(Q), alphas_of(Q)
    st, finals = None, []
    for run in range(2):
        st = fresh_state(Q, H, N, per_step, per_node, st)            # the second run: dirty buffers, re-initialised
        ref = aci_ref.AciRef(pairs, ta, 0.1, M, per_step, per_node, 0, H, N)
        rng = np.random.default_rng(SEED + run)
        for u in range(UPDATES):
            issued = ref.apply(inp.raw[u])                           # what the offsets in force would have served
            before = (ref.alpha.copy(), ref.offsets.copy())
            ref.update(inp.y[u], issued, inp.raw[u])
            ring = dev(ring_of(inp.y[u], inp.origins[u], N, rng))
            i_d, r_d = dev(issued), dev(inp.raw[u])
            assert all(t.data_ptr() % 16 == 0 for t in (i_d, r_d, ring, st.scores))     # N % 4 alone picks the path
            ops.aci_update(i_d, r_d, ring, inp.origins[u], pairs, ta, 0.1, u % M, 0, per_step, per_node, st.scores, st.alpha,
                           st.offsets, st.counts, st.miss_sum, st.valid_sum)
            state_matches(ref, st, (run, u))
            if u == NO_VALID_ALL:                                    # nothing valid anywhere: nothing moved, in any grouping
                assert np.array_equal(ref.alpha, before[0]) and np.array_equal(ref.offsets.view(np.int32), before[1].view(np.int32))
            if u == NO_VALID_ROW and (per_step or per_node):         # the groups of row 0 / column 3 held
                held = (slice(None), 0 if per_step else slice(None), 3 if per_node else slice(None))
                assert np.array_equal(ref.alpha[held], before[0][held])
                if per_step != per_node:
                    assert not np.array_equal(ref.alpha, before[0]), "the other groups moved"
        assert {"hold", "select"} <= ref.branches and (("+inf" in ref.branches) or not per_node)
        finals.append({k: getattr(st, k).clone() for k in ("scores", "alpha", "offsets", "counts", "miss_sum", "valid_sum")})
    for k, v in finals[0].items():
        assert same_nan_aware(v, finals[1][k]) if v.dtype == torch.float32 else torch.equal(v, finals[1][k]), k
    # the inputs held what they promise
    s = ref.scores
    assert np.isinf(s).any() and (s == 0).any() and not (s.view(np.uint32) == 0x80000000).any()
    flat = s[~np.isnan(s)]
    assert flat.size - np.unique(flat).size > 10, "exact ties across the window"


@pytest.mark.parametrize("per_step,per_node", GROUPINGS)
@pytest.mark.parametrize("Q,H,N", SHAPES)
def test_kernel_equals_the_helper_update_by_update(Q, H, N, per_step, per_node):
    update_sequence(Q, H, N, per_step, per_node)


@pytest.mark.parametrize("N", (1639, 6556), ids=("scalar", "16-byte"))
def test_pooled_window_beyond_the_register_budget_is_streamed(N):
    """A pooled group's window of at most 16 loads per thread (16384 floats, 65536 with 16-byte loads) is kept in registers over
    the four passes; a larger one is read again in every pass.  M * H * N = 16390 / 65560 is just beyond either threshold."""
    assert M * 2 * N > 16 * 1024 * (4 if N % 4 == 0 else 1) > M * 2 * (N - 4)
    update_sequence(3, 2, N, False, False)


# ---- 2. gamma = 0 is the existing calibrator on a rolling window ---------------------------------------------------------------
@pytest.mark.parametrize("per_step,per_node", GROUPINGS)
@pytest.mark.parametrize("Q,H,N", SHAPES)
def test_gamma_zero_equals_the_calibrator_on_the_window(Q, H, N, per_step, per_node):
    from stemgnn_amd.math_utils import AdaptiveConformal, ConformalCalibrator
    inp = inputs(Q, H, N, holes=False)
    ad = AdaptiveConformal(TAUS[Q], gamma=0.0, window=M, per_step=per_step, per_node=per_node)
    y_d, raw_d = dev(inp.y), dev(inp.raw)
    fits = held = 0
    for u in range(UPDATES):
        prev = None if ad.offsets is None else ad.offsets.clone()
        ad.update(y_d[u], raw_d[u], raw_d[u])
        lo = max(0, u + 1 - M)
        cal = ConformalCalibrator(TAUS[Q], per_step, per_node).fit(y_d[lo:u + 1], raw_d[lo:u + 1], ignore_nan=True)
        ok = ~torch.isnan(y_d[u])                                    # which groups had a valid target in the newest forecast
        ok = ok if per_step else ok.any(dim=0, keepdim=True)
        ok = (ok if per_node else ok.any(dim=1, keepdim=True))[None].expand_as(cal.offsets)
        prev = torch.zeros_like(cal.offsets) if prev is None else prev
        want = torch.where(ok, cal.offsets, prev)
        assert same_bits(ad.offsets, want), u
        assert torch.equal(ad.counts, cal.counts), u
        fits, held = fits + int(ok.sum()), held + int((~ok).sum())
    assert fits > 0 and (held > 0 or not (per_step and per_node))
    assert same_bits(ad.alpha, torch.tensor(alphas_of(Q), dtype=torch.float64).reshape(-1, 1, 1).expand_as(ad.alpha).contiguous())
    assert ad.n_done == UPDATES


# ---- 3. both excursions, and min_scores ------------------------------------------------------------------------------------------
def test_both_excursions_match_the_helper():
    from stemgnn_amd.math_utils import AdaptiveConformal
    Q, H, N = 3, 2, 5
    raw = np.zeros((Q, H, N), dtype=np.float32)
    raw[0], raw[2] = -1.0, 1.0
    centre, far = np.zeros((H, N), dtype=np.float32), np.full((H, N), 100.0, dtype=np.float32)
    ad = AdaptiveConformal(TAUS[Q], gamma=0.5, window=4).init_state(H, N, DEV)
    ref = aci_ref.AciRef(pairs_of(Q), alphas_of(Q), 0.5, 4, True, False, 0, H, N)
    raw_d, trace = dev(raw), []
    for t, y in enumerate([centre] * 10 + [far] * 6 + [centre] * 4):
        issued = ad.apply(raw_d[None])[0]                            # no delay: the offsets in force, then observe, then update
        assert same_bits(issued, torch.from_numpy(ref.apply(raw))), t
        ref.update(y, ref.apply(raw), raw)
        ad.update(dev(y), issued, raw_d)
        state_matches(ref, ad, t)
        trace.append((float(ref.alpha[0, 0, 0]), float(ref.offsets[0, 0, 0])))
    a, o = np.array(trace).T
    up = int(np.argmax(o == -np.inf))
    assert o[up] == -np.inf and a[up] >= 1.0 and up < 10, "alpha climbed past 1: the empty band"
    assert a[up + 1] < a[up] and o[up + 1] > -np.inf, "the empty band missed everything and alpha came back"
    down = int(np.argmax(o == np.inf))
    assert o[down] == np.inf and a[down] < 0.0 and 10 <= down < 16, "alpha fell below 0: the whole line"
    assert a[down + 1] > a[down], "the whole line covered and alpha came back"
    assert {"-inf", "+inf", "select"} <= ref.branches


def test_min_scores_holds_alpha_and_the_initial_offsets():
    from stemgnn_amd.math_utils import AdaptiveConformal
    Q, H, N = 3, 2, 11
    inp = inputs(Q, H, N, holes=False)
    first = np.full((1, H, N), 0.375, dtype=np.float32)
    ad = AdaptiveConformal(TAUS[Q], gamma=0.5, window=M, per_step=True, per_node=True, min_scores=4)
    ad.init_state(H, N, DEV, offsets=torch.from_numpy(first))
    ref = aci_ref.AciRef(pairs_of(Q), alphas_of(Q), 0.5, M, True, True, 4, H, N, offsets=first)
    for u in range(8):
        issued = ref.apply(inp.raw[u])
        ref.update(inp.y[u], issued, inp.raw[u])
        ad.update(dev(inp.y[u]), dev(issued), dev(inp.raw[u]))
        state_matches(ref, ad, u)
        if u < 3:                                                    # one score per group and update: m <= 3 < 4
            assert bool((ad.offsets == 0.375).all()) and bool((ad.alpha == alphas_of(Q)[0]).all()), u
            assert int(ad.counts.max()) == u + 1
    assert not bool((ad.offsets == 0.375).all()) and "select" in ref.branches
    rep = ad.report()
    assert np.array_equal(rep["alpha"], ref.alpha) and np.array_equal(rep["counts"], ref.counts)
    assert np.array_equal(rep["offsets"].view(np.int32), ref.offsets.view(np.int32))
    assert np.array_equal(rep["miscoverage"], ref.miss_sum / ref.valid_sum)
    # the state survives a save / load, n_done included
    again = AdaptiveConformal(TAUS[Q], gamma=0.5, window=M, per_step=True, per_node=True, min_scores=4)
    again.load_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in ad.state_dict().items()}, device=DEV)
    issued = ref.apply(inp.raw[8])
    ref.update(inp.y[8], issued, inp.raw[8])
    again.update(dev(inp.y[8]), dev(issued), dev(inp.raw[8]))
    assert again.n_done == 9
    state_matches(ref, again, "reloaded")


# ---- 4. the long-run guarantee ------------------------------------------------------------------------------------------------------
def test_long_run_miscoverage_meets_the_bound_where_frozen_offsets_fail():
    from stemgnn_amd.math_utils import AdaptiveConformal
    L = aci_ref.LONG
    y, raw = aci_ref.long_run_stream(SEED)
    ref, ref_frozen, t_valid = aci_ref.long_run_reference(SEED)
    y_d, raw_d = dev(y), dev(raw)
    ad = AdaptiveConformal(L["taus"], gamma=L["gamma"], window=L["window"]).init_state(1, L["N"], DEV)
    frozen, tally = None, torch.zeros(2, dtype=torch.int64, device=DEV)
    for t in range(L["T"]):                                          # on the device throughout: no sync inside the loop
        if t == L["switch"]:
            frozen = ad.offsets.clone()
        ad.update(y_d[t], ad.apply(raw_d[None])[0], raw_d)
        if frozen is not None:
            ok = ~torch.isnan(y_d[t])
            miss = ok & ~((raw_d[0] - frozen[0] <= y_d[t]) & (y_d[t] <= raw_d[1] + frozen[0]))
            tally += torch.stack([miss.sum(), ok.sum()])
    rep = ad.report()                                                # the one sync
    fm, fv = tally.tolist()
    rate = float(rep["miscoverage"][0, 0, 0])
    bound = aci_ref.long_run_bound(t_valid)
    print(f"long run: miscoverage {rate:.6f} (nominal {L['target_alpha']}), bound {bound:.4f}, frozen second half {fm / fv:.4f}")
    assert t_valid == L["T"] and abs(bound - 0.0425) < 1e-12
    assert abs(rate - L["target_alpha"]) <= bound
    assert fm / fv > 2 * L["target_alpha"] and fm / fv == ref_frozen
    state_matches(ref, ad, "long run")


# ---- 5. LiveForecaster end to end ----------------------------------------------------------------------------------------------
W, MULTI, H_MODEL, HORIZON, HISTORY, T = 4, 2, 2, 5, 8, 40
LIVE_TAUS = TAUS[3]


def raw_series(N):
    """[T, N] float64 raw readings with missing = 0.0 and NaN entries (the recipe of tests/test_hip_live.py)"""
    rng = np.random.default_rng(SEED + N)
    s = rng.normal(loc=3.0, scale=2.0, size=(T, N))
    s[s == 0.0] = 1.0
    for t, n, v in ((5, 1, 0.0), (6, 1, 0.0), (9, 3, np.nan), (17, 0, 0.0), (18, 0, np.nan), (19, 0, 0.0), (23, 5, np.nan),
                    (30, N - 1, 0.0), (38, 2, 0.0), (39, 2, np.nan), (39, N - 1, 0.0)):
        s[t, n] = v
    return s


_models = {}


def model_of(N):
    if N not in _models:
        from stemgnn_amd import Model
        torch.manual_seed(SEED + N + 1000)
        _models[N] = Model(N, 2, W, MULTI, horizon=H_MODEL, quantiles=LIVE_TAUS).to(DEV).eval()
    return _models[N]


def make_live(N, **kw):
    from stemgnn_amd import LiveForecaster
    rng = np.random.default_rng(SEED + 100 + N)
    stat = dict(mean=rng.normal(3.0, 0.5, size=N), std=rng.uniform(1.0, 3.0, size=N))
    return LiveForecaster(model_of(N), W, HORIZON, normalize_method="z_score", norm_statistic=stat, missing=0.0, history=HISTORY,
                          **kw)


def static_calibrator(per_step, per_node, N):
    from stemgnn_amd.math_utils import ConformalCalibrator
    cal = ConformalCalibrator(LIVE_TAUS, per_step, per_node)
    shape = (1, HORIZON if per_step else 1, N if per_node else 1)
    off = (0.25 + 0.125 * torch.arange(shape[1] * shape[2], dtype=torch.float32).reshape(shape) / (shape[1] * shape[2])).to(DEV)
    return cal.load_state_dict(dict(cal.state_dict(), offsets=off, counts=torch.ones(shape, dtype=torch.int64, device=DEV)))


@pytest.mark.parametrize("graph", (True, False), ids=("graph", "eager"))
@pytest.mark.parametrize("rearrange", (True, False), ids=("rearranged", "as_is"))
@pytest.mark.parametrize("N", (11, 12))
def test_live_forecaster_with_adaptive_bands(N, rearrange, graph):
    from stemgnn_amd import ops
    from stemgnn_amd.math_utils import AdaptiveConformal
    per_step, per_node = True, N == 12
    series, cut = raw_series(N), 22
    cal = static_calibrator(per_step, per_node, N)
    kw = dict(gamma=0.1, window=6, per_step=per_step, per_node=per_node)
    twin = make_live(N, rearrange=rearrange, graph=graph)            # the raw rows, and the matured pairs
    live = make_live(N, rearrange=rearrange, graph=graph, calibrator=cal)
    ad = AdaptiveConformal(LIVE_TAUS, **kw)
    live.set_adaptive(ad)
    assert live.adaptive is ad and live.calibrator is None
    with pytest.raises(ValueError, match=r"set_adaptive\(None\)"):
        live.set_calibrator(cal)
    ref = aci_ref.AciRef(ad.pairs, ad.target_alpha, 0.1, 6, per_step, per_node, 0, HORIZON, N, offsets=cal.offsets.cpu().numpy())
    issued_at, done, resumed, rep, before_first, updates = {}, -1, None, None, 0, 0
    for t in range(1, T + 1):
        for lv in (twin, live) + ((resumed,) if resumed is not None else ()):
            lv.push(series[t - 1])
        if t < W:
            continue
        fc, tg, origins = twin.matured()                             # ahead of twin.forecast(), which may reuse a slot
        for i, o in enumerate(origins.tolist()):
            if o > done:
                ref.update(tg[i].cpu().numpy(), issued_at[o], fc[i].cpu().numpy())
                done, updates = o, updates + 1
        raw_t = twin.forecast()
        want = ops.conformal_apply(raw_t[None], dev(ref.offsets), ad.pairs, per_step, per_node)[0]
        got = live.forecast()
        assert same_bits(got, want), t
        assert same_bits(ad.offsets, torch.from_numpy(ref.offsets)) and same_bits(ad.alpha, torch.from_numpy(ref.alpha)), t
        issued_at[t] = want.cpu().numpy()
        if updates == 0:
            before_first += 1
            assert same_bits(ad.offsets, cal.offsets)               # the static calibrator's offsets until the first update
        if rep is None:
            rep = live._replay
            assert (rep is not None) == graph
        if resumed is not None:
            assert same_bits(resumed.forecast(), want), t
            assert same_bits(resumed.adaptive.offsets, ad.offsets) and same_bits(resumed.adaptive.alpha, ad.alpha), t
            assert resumed.adaptive.n_done == ad.n_done and resumed.done == live.done
        if t == cut:                                                 # a restart in mid-stream, as if read from disk
            state = live.state_dict()
            state = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in state.items()}
            state["adaptive"] = {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in state["adaptive"].items()}
            resumed = make_live(N, rearrange=rearrange, graph=graph)
            resumed.set_adaptive(AdaptiveConformal(LIVE_TAUS, **kw))
            resumed.load_state_dict(state)
            assert resumed.rows == cut and resumed.done == live.done and resumed.adaptive.n_done == ad.n_done
    assert live._replay is rep, "never captured again"
    assert before_first == HORIZON and updates == T - HORIZON - W + 1 == ad.n_done and live.done == T - HORIZON
    assert {"select"} <= ref.branches and updates > 6 * 4, "the window wrapped"
    assert bool(torch.isnan(live.ring_y).any()), "targets with missing readings"
    assert same_nan_aware(ad.scores, torch.from_numpy(ref.scores))
    assert torch.equal(ad.counts.cpu(), torch.from_numpy(ref.counts)) and torch.equal(ad.miss_sum.cpu(), torch.from_numpy(ref.miss_sum))
    # a state saved without adaptive bands still loads into a forecaster without them
    plain_state = {k: v for k, v in twin.state_dict().items()}
    assert "adaptive" not in plain_state and "history_raw" not in plain_state
    assert same_bits(make_live(N, rearrange=rearrange, graph=graph).load_state_dict(plain_state).forecast(), raw_t)
    live.set_adaptive(None)                                          # back to the raw bands
    assert live.adaptive is None and same_bits(live.forecast(), raw_t)


def test_a_forecaster_without_adaptive_bands_launches_what_it_did():
    """set_adaptive never called: no raw slab, the one store, and the captured body issues the same calls as before"""
    from stemgnn_amd import ops
    live = make_live(11, rearrange=True, graph=False)
    live.push(raw_series(11)[:W])
    calls = []
    real = ops.quantile_store, ops.aci_update
    ops.quantile_store = lambda *a, **k: (calls.append("store"), real[0](*a, **k))[1]
    ops.aci_update = lambda *a, **k: (calls.append("aci"), real[1](*a, **k))[1]
    try:
        live.forecast()
    finally:
        ops.quantile_store, ops.aci_update = real
    assert calls == ["store"] and live.out_raw is None and live.adaptive is None
