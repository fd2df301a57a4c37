"""GPU: what a LOADED state does to the serving kernels -- the one key of a stored score (csrc/conformal_select.h:
cf_score_key) and the in-place restore of math_utils.AdaptiveConformal / ConformalAnomaly under a captured LiveForecaster.

1. A stored -0.  The other suites reach -0 only as a freshly computed score, which is stored as +0; a loaded window may hold the
   bit pattern itself.  It must order as +0 (for the anomaly count: a stored -0 is >= a query of +0) and come back as +0 (for the
   adaptive offset).  The references are tests/helpers/aci_ref.py and tests/helpers/anomaly_ref.py on the same bits; every
   comparison is one of bit patterns (NaN-aware where NaN means "absent").
2. LiveForecaster.load_state_dict on a forecaster whose graph is captured: the buffers the graph reads keep their addresses,
   nothing is captured again, and the forecaster goes on bit for bit like the one that was never interrupted.
There is no tolerance in this file.  One fixed seed."""
import numpy as np
import pytest
import torch

from tests.helpers import aci_ref, anomaly_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261021
F32 = np.float32
H, WINDOW = 2, 4
SHAPES = (5, 8)                               # N: scalar path, 16-byte path
GROUPINGS = ((True, False), (True, True), (False, False), (False, True))       # (per_step, per_node)
SPECIAL = np.array([-0.0, 0.0, np.nan, np.inf, -np.inf], dtype=F32)
POOL = np.concatenate([SPECIAL, np.array([-0.0, -0.0, -0.0, -0.5, -0.25], dtype=F32)])      # mostly <= 0: zeros get selected


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def same_nan_aware(a, b):
    a, b = a.detach().cpu(), b.detach().cpu()
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(na, nb) and torch.equal(bits(a)[~na], bits(b)[~nb])


def window_of(N, rng):
    """[WINDOW, H, N] fp32 drawn from POOL; every special bit pattern is in every slot the update reads (1 .. WINDOW - 1)"""
    w = rng.choice(POOL, size=(WINDOW, H, N))
    for slot in range(1, WINDOW):
        w[slot].reshape(-1)[rng.permutation(H * N)[:SPECIAL.size]] = SPECIAL
    for v in SPECIAL[:2]:
        assert (w[1:].view(np.uint32) == v.view(np.uint32)).any()
    return w


# ---- 1. a stored -0 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_step,per_node", GROUPINGS)
@pytest.mark.parametrize("N", SHAPES)
def test_adaptive_update_on_a_loaded_window_with_negative_zero(N, per_step, per_node):
    from stemgnn_amd.math_utils import AdaptiveConformal
    rng = np.random.default_rng(SEED + N)
    window = window_of(N, rng)[:, None]                              # [WINDOW, P = 1, H, N]
    y = (rng.integers(-4, 5, size=(H, N)) / 4).astype(F32)           # inside [-1, 1]: scores <= 0, exactly +0 at the ends
    y[0, 1], y[1, 3] = np.nan, np.nan
    raw = np.stack([np.full((H, N), -1.0, F32), np.full((H, N), 1.0, F32)])
    ad = AdaptiveConformal((0.1, 0.9), gamma=0.1, window=WINDOW, per_step=per_step, per_node=per_node, min_scores=0)
    ref = aci_ref.AciRef(ad.pairs, ad.target_alpha, 0.1, WINDOW, per_step, per_node, 0, H, N)
    ref.scores[:], ref.n_done = window, WINDOW                       # a full window: the update overwrites slot 0
    state = dict(ad.init_state(H, N, DEV).state_dict(), scores=torch.from_numpy(window.copy()), n_done=WINDOW)
    ad.load_state_dict(state, device=DEV)
    assert same_nan_aware(ad.scores, torch.from_numpy(window)) and ad.scores.data_ptr() % 16 == 0
    ref.update(y, raw, raw)
    ad.update(torch.from_numpy(y).to(DEV), torch.from_numpy(raw).to(DEV), torch.from_numpy(raw).to(DEV))
    assert same_bits(ad.offsets, torch.from_numpy(ref.offsets)), (ad.offsets, ref.offsets)
    assert same_bits(ad.alpha, torch.from_numpy(ref.alpha))
    for k in ("counts", "miss_sum", "valid_sum"):
        assert torch.equal(getattr(ad, k).cpu(), torch.from_numpy(getattr(ref, k))), k
    assert same_nan_aware(ad.scores, torch.from_numpy(ref.scores))   # the loaded slots keep their bits, -0 included
    # the inputs held what they promise: some group's offset IS a zero of the window, and it came back as +0
    zero = ref.offsets == 0
    assert zero.any() and not np.signbit(ref.offsets[zero]).any() and "select" in ref.branches


@pytest.mark.parametrize("per_step,per_node", GROUPINGS)
@pytest.mark.parametrize("N", SHAPES)
def test_anomaly_update_on_a_loaded_window_with_negative_zero(N, per_step, per_node):
    from stemgnn_amd.math_utils import ConformalAnomaly
    rng = np.random.default_rng(SEED + 100 + N)
    window = window_of(N, rng)
    y = (rng.integers(-2, 3, size=N) / 4).astype(F32)
    f = np.stack([y.copy(), y + F32(0.25)]).astype(F32)              # step 0: |f - y| = +0 exactly, the query a stored -0 must meet
    y[2] = np.nan
    det = ConformalAnomaly(alpha=0.5, window=WINDOW, per_step=per_step, per_node=per_node, min_scores=0, keep=WINDOW)
    ref = anomaly_ref.AnomalyRef(0.5, WINDOW, per_step, per_node, 0, H, N, keep=WINDOW)
    ref.scores[:], ref.n_done = window, WINDOW
    state = dict(det.init_state(H, N, 1, DEV).state_dict(), scores=torch.from_numpy(window.copy()), n_done=WINDOW)
    det.load_state_dict(state, device=DEV)
    ref.update(y, f)
    det.update(torch.from_numpy(y).to(DEV), torch.from_numpy(f).to(DEV))
    for k in ("pvalues", "node_p", "scores"):
        assert same_nan_aware(getattr(det, k), torch.from_numpy(getattr(ref, k))), (k, getattr(det, k), getattr(ref, k))
    for k in ("alarm", "counts", "judged_sum", "alarm_sum"):
        got, want = getattr(det, k).cpu(), torch.from_numpy(getattr(ref, k))
        assert got.dtype == want.dtype and torch.equal(got, want), k
    # the inputs held what they promise: a query of +0 whose population holds a -0, counted as >= it
    def population(n):                                               # of step 0 of node n
        return window[1:, 0 if per_step else slice(None), n if per_node else slice(None)].reshape(-1)
    met = [n for n in range(N) if not np.isnan(y[n]) and np.signbit(population(n)[population(n) == 0]).any()]
    assert met and not np.isnan(ref.pvalues[0, met]).any() and (f[0, met] == y[met]).all()


# ---- 2. restore in place under a captured graph ---------------------------------------------------------------------------------------
W, HORIZON, HISTORY, T, CUT, N_LIVE = 4, 2, 6, 26, 14, 11
TAUS = (0.1, 0.5, 0.9)


def raw_series():
    rng = np.random.default_rng(SEED + 7)
    s = rng.normal(loc=3.0, scale=2.0, size=(T, N_LIVE))
    s[s == 0.0] = 1.0
    for t, n, v in ((5, 1, 0.0), (9, 3, np.nan), (16, 0, 0.0), (17, 0, np.nan), (21, N_LIVE - 1, 0.0)):
        s[t, n] = v
    return s


def make_live(model):
    from stemgnn_amd import LiveForecaster
    from stemgnn_amd.math_utils import AdaptiveConformal, ConformalAnomaly
    rng = np.random.default_rng(SEED + 8)
    stat = dict(mean=rng.normal(3.0, 0.5, size=N_LIVE), std=rng.uniform(1.0, 3.0, size=N_LIVE))
    live = LiveForecaster(model, W, HORIZON, normalize_method="z_score", norm_statistic=stat, missing=0.0, history=HISTORY,
                          rearrange=True, graph=True)
    live.set_adaptive(AdaptiveConformal(TAUS, gamma=0.1, window=5, per_step=True, per_node=False))
    live.set_anomaly(ConformalAnomaly(alpha=0.5, window=6, per_step=True, per_node=True, min_scores=2, keep=4))
    return live


def test_load_state_dict_restores_a_captured_forecaster_in_place():
    from stemgnn_amd import Model
    torch.manual_seed(SEED)
    model = Model(N_LIVE, 2, W, 2, horizon=HORIZON, quantiles=TAUS).to(DEV).eval()
    series = raw_series()
    whole, other = make_live(model), make_live(model)
    for t in range(1, T + 1):                                        # `other` runs to the end once: captured, another state
        other.push(series[t - 1])
        if t >= W:
            other.forecast()
    owned = lambda lv: dict(offsets=lv.adaptive.offsets, ad_scores=lv.adaptive.scores, det_scores=lv.anomaly.scores,
                            node_p=lv.anomaly.node_p)
    before = {k: v.data_ptr() for k, v in owned(other).items()}
    replay = other._replay
    assert replay is not None
    for t in range(1, T + 1):
        whole.push(series[t - 1])
        if t > CUT:
            other.push(series[t - 1])
        if t < W:
            continue
        want = whole.forecast()
        if t == CUT:                                                 # as if read from disk
            state = whole.state_dict()
            cpu = lambda d: {k: (v.cpu() if torch.is_tensor(v) else v) for k, v in d.items()}
            state = dict(cpu(state), adaptive=cpu(state["adaptive"]), anomaly=cpu(state["anomaly"]))
            assert other.load_state_dict(state) is other
            assert {k: v.data_ptr() for k, v in owned(other).items()} == before and other._replay is replay
            assert other.rows == CUT and other.adaptive.n_done == whole.adaptive.n_done
            assert (other.anomaly.n_done, other.anomaly.last_row) == (whole.anomaly.n_done, whole.anomaly.last_row)
            assert same_bits(other.adaptive.offsets, whole.adaptive.offsets)
            assert same_nan_aware(other.anomaly.scores, whole.anomaly.scores)
        if t > CUT:
            assert same_bits(other.forecast(), want), t
            (p_o, a_o, r_o), (p_w, a_w, r_w) = other.anomalies(), whole.anomalies()
            assert same_nan_aware(p_o, p_w) and torch.equal(a_o, a_w) and r_o == r_w, t
            assert same_bits(other.adaptive.offsets, whole.adaptive.offsets) and same_bits(other.adaptive.alpha, whole.adaptive.alpha), t
    assert other._replay is replay and {k: v.data_ptr() for k, v in owned(other).items()} == before, "never captured again"
    assert whole.adaptive.n_done > 5 and whole.anomaly.n_done > 6, "both windows wrapped after the restore"
    rec_o, rec_w = other.anomaly.recent(), whole.anomaly.recent()
    assert same_nan_aware(rec_o[0], rec_w[0]) and torch.equal(rec_o[1], rec_w[1])
    assert bool((~torch.isnan(whole.anomaly.node_p)).any()), "some node was judged"
