"""CPU: the adaptive-conformal entry of include/stemgnn_hip.h (csrc/aci.hip) is exported, declared and bound; every bad argument
is refused before any launch; math_utils.AdaptiveConformal and LiveForecaster.set_adaptive refuse what they cannot serve before
they touch the device; the numpy helper (tests/helpers/aci_ref.py) alone meets the long-run bound of tests/test_hip_aci.py on
that test's stream, so the condition is known to be reachable before a GPU sees it.  Nothing is launched."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import aci_ref

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NAME = "stemgnn_aci_update"
TAUS = (0.1, 0.5, 0.9)
SEED = 20261019


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_symbol_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib, engine, math_utils, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    assert hasattr(lib, NAME) and NAME in _lib.SIGNATURES and NAME + "(" in header
    res, args = _lib.SIGNATURES[NAME]
    assert res is ctypes.c_int and len(args) == 25
    assert args[4] is ctypes.c_longlong and "long long origin" in header           # origin
    assert args[12] is ctypes.c_double and "double gamma" in header                # gamma
    assert args[15] is ctypes.c_longlong and "long long min_scores" in header      # min_scores
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "aci.hip" in makefile.split("SRCS =")[1].splitlines()[0].split()
    assert tuple(inspect.signature(ops.aci_update).parameters) == (
        "issued", "raw", "ring_y", "origin", "pairs", "target_alpha", "gamma", "slot", "min_scores", "per_step", "per_node",
        "scores", "alpha", "offsets", "counts", "miss_sum", "valid_sum")
    par = inspect.signature(math_utils.AdaptiveConformal.__init__).parameters
    assert tuple(par) == ("self", "quantiles", "gamma", "window", "per_step", "per_node", "min_scores")
    assert (par["gamma"].default, par["window"].default, par["per_step"].default, par["per_node"].default,
            par["min_scores"].default) == (0.005, 256, True, False, 0)
    par = inspect.signature(math_utils.AdaptiveConformal.update).parameters
    assert tuple(par) == ("self", "y", "issued", "raw", "ring", "origin")
    assert par["ring"].kind is inspect.Parameter.KEYWORD_ONLY and par["origin"].default == 0
    assert tuple(inspect.signature(engine.LiveForecaster.set_adaptive).parameters) == ("self", "adaptive")


def test_live_forecaster_constructor_is_unchanged():
    from stemgnn_amd import engine
    par = inspect.signature(engine.LiveForecaster.__init__).parameters
    assert tuple(par) == ("self", "model", "window", "horizon", "normalize_method", "norm_statistic", "missing", "fill",
                          "history", "adjacency", "rearrange", "calibrator", "graph", "device")
    assert par["history"].default == 64 and par["graph"].default is True and par["calibrator"].default is None
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(par)[4:])


LO, HI = (ctypes.c_int * 1)(0), (ctypes.c_int * 1)(2)
TA = (ctypes.c_double * 1)(0.2)
OK = dict(issued=P, raw=P, ring_y=P, C=7, origin=3, Q=3, H=2, N=11, P=1, lo=LO, hi=HI, ta=TA, gamma=0.1, M=5, slot=4,
          min_scores=0, per_step=1, per_node=0, scores=P, alpha=P, offsets=P, counts=P, miss_sum=P, valid_sum=P)


def refused(f, **change):
    return f(*{**OK, **change}.values(), None) == SG_EINVAL


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def doubles(*v):
    return (ctypes.c_double * len(v))(*v)


def test_update_rejects_bad_arguments(lib):
    f = getattr(lib, NAME)
    for grouping in (dict(per_step=1, per_node=0), dict(per_step=0, per_node=1)):
        for k in ("issued", "raw", "ring_y", "lo", "hi", "ta", "scores", "alpha", "offsets", "counts", "miss_sum", "valid_sum"):
            assert refused(f, **grouping, **{k: None}), k
        for k in ("C", "Q", "H", "N", "P", "M"):
            for v in (0, -1):
                assert refused(f, **grouping, **{k: v}), (k, v)
    assert refused(f, Q=33, hi=ints(32))                                          # Q > 32
    assert refused(f, Q=40, P=17, lo=ints(*range(17)), hi=ints(*range(20, 37)), ta=doubles(*[0.2] * 17))      # P > 16
    for lo, hi in ((0, 3), (-1, 2), (2, 2), (2, 1)):                               # a pair outside 0 <= lo < hi < Q
        assert refused(f, lo=ints(lo), hi=ints(hi)), (lo, hi)
    assert refused(f, Q=4, P=2, lo=ints(0, 0), hi=ints(3, 2), ta=doubles(0.2, 0.4))                            # a row named twice
    assert refused(f, Q=4, P=2, lo=ints(0, 1), hi=ints(3, 3), ta=doubles(0.2, 0.4))
    for g in (float("nan"), -0.5, -1e-300):
        assert refused(f, gamma=g), g
    for a in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert refused(f, ta=doubles(a)), a
    assert refused(f, Q=4, P=2, lo=ints(0, 1), hi=ints(3, 2), ta=doubles(0.2, 1.0))                            # the second level
    for s in (-1, 5, 6):
        assert refused(f, slot=s), s
    for o in (-1, -2 ** 40):
        assert refused(f, origin=o), o
    assert refused(f, C=1)                                                         # H > C
    assert refused(f, M=2 ** 15, H=2 ** 4, C=2 ** 4, N=2 ** 12, slot=0)            # M * H * N >= 2^31
    assert refused(f, C=2 ** 16, N=2 ** 15, H=1, M=1, slot=0)                      # C * N >= 2^31
    for v in (-1, -2 ** 40):
        assert refused(f, min_scores=v), v


def test_adaptive_conformal_refuses_before_touching_the_device():
    from stemgnn_amd.math_utils import AdaptiveConformal
    for taus in ((0.5,), ()):
        with pytest.raises(ValueError, match="at least two"):
            AdaptiveConformal(taus)
    for taus in ((0.9, 0.5, 0.1), (0.5, 0.5), (0.1, 0.9, 0.5, 0.4)):
        with pytest.raises(ValueError, match="increasing"):
            AdaptiveConformal(taus)
    for g in (-0.1, float("nan")):
        with pytest.raises(ValueError, match="gamma"):
            AdaptiveConformal(TAUS, gamma=g)
    for w in (0, -3):
        with pytest.raises(ValueError, match="window"):
            AdaptiveConformal(TAUS, window=w)
    with pytest.raises(ValueError, match="min_scores"):
        AdaptiveConformal(TAUS, min_scores=-1)
    ad = AdaptiveConformal((0.05, 0.25, 0.5, 0.75, 0.95), gamma=0.0, window=3, per_step=False, per_node=True, min_scores=2)
    assert ad.pairs == ((0, 4), (1, 3)) and ad.n_done == 0 and ad.offsets is None and ad.scores is None
    assert ad.target_alpha == [1.0 - (0.95 - 0.05), 1.0 - (0.75 - 0.25)]
    assert ad.group_shape(5, 7) == (2, 1, 7)
    for call in (ad.report, lambda: ad.apply(torch.zeros(1, 5, 2, 7))):
        with pytest.raises(ValueError, match="no state yet"):
            call()
    assert ad.state_dict()["scores"] is None and ad.state_dict()["n_done"] == 0


def fitted(taus, shape, **kw):
    from stemgnn_amd.math_utils import ConformalCalibrator
    cal = ConformalCalibrator(taus, **kw)
    return cal.load_state_dict(dict(cal.state_dict(), offsets=torch.zeros(shape), counts=torch.zeros(shape, dtype=torch.int64)))


def test_set_adaptive_refuses_before_touching_the_device():
    from stemgnn_amd import LiveForecaster, Model
    from stemgnn_amd.math_utils import AdaptiveConformal
    plain, quant = Model(6, 2, 4, 2, horizon=2), Model(6, 2, 4, 2, horizon=2, quantiles=TAUS)
    with pytest.raises(ValueError, match="quantile model"):
        LiveForecaster(plain, 4, 5, history=8).set_adaptive(AdaptiveConformal(TAUS))
    live = LiveForecaster(quant, 4, 5, history=8)
    for taus in ((0.2, 0.5, 0.8), (0.1, 0.9)):
        with pytest.raises(ValueError, match="levels"):
            live.set_adaptive(AdaptiveConformal(taus))
    stale = AdaptiveConformal(TAUS)                                 # carries the state of another horizon
    stale.load_state_dict(dict(stale.state_dict(), scores=torch.zeros(256, 1, 2, 6), alpha=torch.zeros(1, 2, 1, dtype=torch.float64),
                               offsets=torch.zeros(1, 2, 1), counts=torch.zeros(1, 2, 1, dtype=torch.int64),
                               miss_sum=torch.zeros(1, 2, 1, dtype=torch.int64),
                               valid_sum=torch.zeros(1, 2, 1, dtype=torch.int64)))
    with pytest.raises(ValueError, match="do not fit horizon 5"):
        live.set_adaptive(stale)
    short = LiveForecaster(quant, 4, 5, history=3)
    with pytest.raises(ValueError, match="history 3 < horizon 5"):
        short.set_adaptive(AdaptiveConformal(TAUS))
    pooled = LiveForecaster(quant, 4, 5, history=8, calibrator=fitted(TAUS, (1, 5, 1)))
    with pytest.raises(ValueError, match="per_step=True, per_node=False"):       # the static calibrator's grouping differs
        pooled.set_adaptive(AdaptiveConformal(TAUS, per_step=False, per_node=True))
    assert pooled.adaptive is None and pooled.calibrator is not None
    ad = AdaptiveConformal(TAUS)
    pooled.set_adaptive(ad)                                         # the take-over: still nothing on the device
    assert pooled.adaptive is ad and pooled.calibrator is None and ad.offsets is None
    with pytest.raises(ValueError, match=r"set_adaptive\(None\)"):
        pooled.set_calibrator(fitted(TAUS, (1, 5, 1)))
    pooled.set_adaptive(None)
    assert pooled.adaptive is None and pooled.calibrator is None
    pooled.set_calibrator(fitted(TAUS, (1, 5, 1)))
    for lv in (live, short, pooled):
        assert lv.rows == 0 and not lv._ready_buffers


def test_helper_alone_meets_the_long_run_bound():
    L = aci_ref.LONG
    for seed in (SEED, SEED + 1, SEED + 2):
        ref, frozen_rate, t_valid = aci_ref.long_run_reference(seed)
        rate = ref.miss_sum[0, 0, 0] / ref.valid_sum[0, 0, 0]
        bound = aci_ref.long_run_bound(t_valid)
        assert t_valid == L["T"] and abs(bound - 0.0425) < 1e-12
        assert abs(rate - L["target_alpha"]) <= bound, (seed, rate)
        assert frozen_rate > 2 * L["target_alpha"], (seed, frozen_rate)
        assert ref.n_done == L["T"] and int(ref.counts[0, 0, 0]) <= L["window"] * L["N"]


def test_helper_branches_and_gamma_zero_is_a_rolling_refit():
    """the helper's own two excursions and holds, on hand-made inputs; with gamma = 0 its offset is the k-th smallest of the
    window at the nominal level (the formula of ConformalCalibrator.fit), whatever was issued"""
    raw = np.array([[[-1.0, -1.0]], [[1.0, 1.0]]], dtype=np.float32)              # [2, 1, 2]
    ref = aci_ref.AciRef([(0, 1)], [0.2], 0.5, 4, True, False, 0, 1, 2)
    for _ in range(4):                                              # always covered: alpha climbs by 0.1 a step
        ref.update(np.zeros((1, 2), dtype=np.float32), ref.apply(raw), raw)
    assert "select" in ref.branches and ref.alpha[0, 0, 0] == 0.2 + 0.1 + 0.1 + 0.1 + 0.1
    hold = aci_ref.AciRef([(0, 1)], [0.2], 0.5, 4, True, False, 3, 1, 2)
    hold.update(np.array([[np.nan, 0.0]], dtype=np.float32), raw, raw)            # m = 1 < min_scores
    hold.update(np.full((1, 2), np.nan, dtype=np.float32), raw, raw)              # nothing valid
    assert hold.branches == {"hold"} and hold.alpha[0, 0, 0] == 0.2 and hold.offsets[0, 0, 0] == 0.0
    assert hold.counts[0, 0, 0] == 1 and hold.valid_sum[0, 0, 0] == 1 and np.isnan(hold.scores[1]).all()
    z = aci_ref.AciRef([(0, 1)], [0.5], 0.0, 3, True, False, 0, 1, 2)
    rng = np.random.default_rng(SEED)
    ys = rng.normal(size=(7, 1, 2)).astype(np.float32)
    for t in range(7):
        z.update(ys[t], raw, raw)
        w = np.sort(aci_ref.scores_of(ys[max(0, t - 2):t + 1], raw[0], raw[1]).reshape(-1))
        k = aci_ref.rank(w.size, 0.5)
        want = np.float32(np.inf) if k > w.size else w[int(k) - 1]
        assert z.offsets[0, 0, 0] == want and z.alpha[0, 0, 0] == 0.5, t
    assert aci_ref.scores_of(np.float32(1.0), np.float32(1.0), np.float32(1.0)).view(np.uint32) == 0   # -0 -> +0
    assert aci_ref.scores_of(np.float32(0.0), np.float32(np.nan), np.float32(1.0)) == np.inf
