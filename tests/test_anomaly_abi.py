"""CPU: the anomaly entry of include/stemgnn_hip.h (csrc/anomaly.hip) is exported, declared and bound; every bad argument is
refused before any launch; math_utils.ConformalAnomaly and LiveForecaster.set_anomaly refuse what they cannot serve before they
touch the device; the numpy helper (tests/helpers/anomaly_ref.py) alone meets the statistical condition of
tests/test_hip_anomaly.py on that test's stream, so the condition is known to be reachable before a GPU sees it.  Nothing is
launched."""
import ctypes
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import anomaly_ref

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NAME = "stemgnn_anomaly_update"
SEED = 20261020


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
    assert res is ctypes.c_int and len(args) == 29
    assert args[6] is ctypes.c_longlong and "long long row" in header              # row
    assert args[13] is ctypes.c_longlong and "long long min_scores" in header      # min_scores
    assert args[14] is ctypes.c_double and "double alpha" in header                # alpha
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "anomaly.hip" in makefile.split("SRCS =")[1].splitlines()[0].split()
    assert tuple(inspect.signature(ops.anomaly_update).parameters) == (
        "slab", "origins", "row", "ring_y", "rows", "slot", "min_scores", "alpha", "per_step", "per_node", "scores", "pvalues",
        "node_p", "alarm", "counts", "alarm_sum", "judged_sum", "log_p", "log_slot", "work")
    par = inspect.signature(math_utils.ConformalAnomaly.__init__).parameters
    assert tuple(par) == ("self", "alpha", "window", "per_step", "per_node", "min_scores", "score", "keep")
    assert tuple(par[k].default for k in list(par)[1:]) == (0.01, 1024, True, True, 32, "point", 64)
    par = inspect.signature(math_utils.ConformalAnomaly.update).parameters
    assert tuple(par) == ("self", "y", "forecasts", "slab", "origins", "row", "ring", "rows")
    assert all(par[k].kind is inspect.Parameter.KEYWORD_ONLY and par[k].default is None for k in list(par)[3:])
    assert tuple(inspect.signature(math_utils.ConformalAnomaly.init_state).parameters) == ("self", "H", "N", "R", "device")
    assert tuple(inspect.signature(engine.LiveForecaster.set_anomaly).parameters) == ("self", "detector")
    assert tuple(inspect.signature(engine.LiveForecaster.anomalies).parameters) == ("self",)
    for k in ("recent", "report", "state_dict", "load_state_dict"):
        assert callable(getattr(math_utils.ConformalAnomaly, k))


OK = dict(slab=P, S=4, R=3, lo=0, hi=2, origins=P, row=9, ring_y=P, C=7, H=2, N=11, M=5, slot=4, min_scores=0, alpha=0.1,
          per_step=1, per_node=0, scores=P, pvalues=P, node_p=P, alarm=P, counts=P, alarm_sum=P, judged_sum=P, log_p=P, keep=3,
          log_slot=2, work=P)


def refused(f, **change):
    return f(*{**OK, **change}.values(), None) == SG_EINVAL


def test_update_rejects_bad_arguments(lib):
    f = getattr(lib, NAME)
    for grouping in (dict(per_step=1, per_node=0), dict(per_step=0, per_node=1), dict(per_step=1, per_node=1),
                     dict(per_step=0, per_node=0)):
        for k in ("slab", "ring_y", "scores", "pvalues", "node_p", "alarm", "counts", "alarm_sum", "judged_sum", "log_p", "work"):
            assert refused(f, **grouping, **{k: None}), k
        assert refused(f, **grouping, origins=None, slab=None)                    # origins may be NULL, nothing else
        for k in ("S", "R", "C", "H", "N", "M", "keep"):
            for v in (0, -1):
                assert refused(f, **grouping, **{k: v}), (k, v)
    assert refused(f, R=33, hi=32)                                                # R > 32
    for lo, hi in ((0, 3), (-1, 2), (2, 1), (3, 3), (-1, -1)):                     # rows outside 0 <= lo <= hi < R
        assert refused(f, lo=lo, hi=hi), (lo, hi)
    for s in (-1, 5, 6):
        assert refused(f, slot=s), s
    for s in (-1, 3):
        assert refused(f, log_slot=s), s
    for r in (-1, -2 ** 40):
        assert refused(f, row=r), r
    for a in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert refused(f, alpha=a), a
    for v in (-1, -2 ** 40):
        assert refused(f, min_scores=v), v
    assert refused(f, M=2 ** 15, H=2 ** 4, N=2 ** 12, slot=0)                      # M * H * N >= 2^31
    assert refused(f, C=2 ** 16, N=2 ** 15, H=1, M=1, slot=0)                      # C * N >= 2^31
    assert refused(f, S=2 ** 15, R=1, hi=0, H=2 ** 4, N=2 ** 12, M=1, slot=0)      # S * R * H * N >= 2^31
    assert refused(f, S=2 ** 11, R=32, hi=31, H=2 ** 4, N=2 ** 11, M=1, slot=0)
    assert refused(f, S=2 ** 30, R=32, hi=31, H=2 ** 15, N=2 ** 15, M=1, slot=0)   # the product leaves 64 bits


def test_conformal_anomaly_refuses_before_touching_the_device():
    from stemgnn_amd.math_utils import ConformalAnomaly
    for a in (0.0, 1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            ConformalAnomaly(alpha=a)
    for w in (1, 0, -3):
        with pytest.raises(ValueError, match="window"):
            ConformalAnomaly(window=w)
    with pytest.raises(ValueError, match="min_scores"):
        ConformalAnomaly(min_scores=-1)
    for k in (0, -2):
        with pytest.raises(ValueError, match="keep"):
            ConformalAnomaly(keep=k)
    with pytest.raises(ValueError, match="score"):
        ConformalAnomaly(score="interval")
    det = ConformalAnomaly(window=299)
    assert det.n_done == 0 and det.scores is None and det.node_p is None and det.state_dict()["scores"] is None
    for call in (det.report, det.recent):
        with pytest.raises(ValueError, match="no state yet"):
            call()
    # once H and N are known: the defaults at horizon 3 need window >= 300
    with pytest.raises(ValueError, match=r"can never alarm.*window >= 300 would do"):
        det.init_state(3, 7, 1, "cuda:0")
    with pytest.raises(ValueError, match=r"can never alarm.*window >= 300 would do"):
        det.update(torch.zeros(7), torch.zeros(3, 7))
    assert det.scores is None
    ConformalAnomaly(window=300).check_shape(3, 7)
    ConformalAnomaly(window=44, per_step=False, per_node=False).check_shape(3, 7)          # 43 * 21 + 1 = 904 >= 300
    with pytest.raises(ValueError, match=r"window >= 16 would do"):                          # 14 * 21 + 1 = 295 < 300
        ConformalAnomaly(window=15, per_step=False, per_node=False).check_shape(3, 7)
    with pytest.raises(ValueError, match=r"window >= 44 would do"):                          # pooled over 7 nodes: 42 * 7 + 1 = 295 < 300
        ConformalAnomaly(window=43, per_step=True, per_node=False).check_shape(3, 7)
    with pytest.raises(ValueError, match="band"):                                           # a band of a point forecast
        ConformalAnomaly(alpha=0.5, window=8, score="band").update(torch.zeros(7), torch.zeros(3, 7))
    with pytest.raises(ValueError, match="rows"):
        ConformalAnomaly(alpha=0.5, window=8).update(torch.zeros(7), torch.zeros(3, 3, 7), rows=(0, 2))
    with pytest.raises(ValueError, match="saved with"):
        ConformalAnomaly(window=300).load_state_dict(ConformalAnomaly(window=301).state_dict())


def test_set_anomaly_refuses_before_touching_the_device():
    from stemgnn_amd import LiveForecaster, Model
    from stemgnn_amd.math_utils import ConformalAnomaly
    plain, quant = Model(6, 2, 4, 2, horizon=2), Model(6, 2, 4, 2, horizon=2, quantiles=(0.1, 0.5, 0.9))
    live = LiveForecaster(plain, 4, 5, history=8)
    with pytest.raises(ValueError, match="point model has no bands"):
        live.set_anomaly(ConformalAnomaly(alpha=0.5, window=16, score="band"))
    with pytest.raises(ValueError, match=r"can never alarm.*window >= 500 would do"):
        live.set_anomaly(ConformalAnomaly(window=400))                              # horizon 5 at alpha 0.01
    short = LiveForecaster(quant, 4, 5, history=3)
    with pytest.raises(ValueError, match="history 3 < horizon 5"):
        short.set_anomaly(ConformalAnomaly(alpha=0.5, window=16))
    with pytest.raises(RuntimeError, match="no detector"):
        live.anomalies()
    det = ConformalAnomaly(alpha=0.5, window=16)
    live.set_anomaly(det)
    assert live.anomaly is det and live._anomaly_rows == (0, 0) and det.scores is None
    live.set_anomaly(None)
    assert live.anomaly is None
    qlive = LiveForecaster(quant, 4, 5, history=8)
    qlive.set_anomaly(ConformalAnomaly(alpha=0.5, window=16))
    assert qlive._anomaly_rows == (quant.point_index, quant.point_index) == (1, 1)
    qlive.set_anomaly(ConformalAnomaly(alpha=0.5, window=16, score="band"))
    assert qlive._anomaly_rows == (0, 2)
    for lv in (live, short, qlive):
        assert lv.rows == 0 and not lv._ready_buffers


def test_helper_alone_meets_the_validity_and_power_condition():
    V = anomaly_ref.VALID
    for seed in (SEED, SEED + 1, SEED + 2):
        ref, flags = anomaly_ref.validity_reference(seed)
        judged, alarms = int(ref.judged_sum.sum()), int(ref.alarm_sum.sum())
        rate = alarms / judged
        assert judged == (V["T"] - V["min_scores"]) * V["N"] == 11744 and alarms == int(flags.sum())
        assert V["alpha"] / 4 <= rate <= V["alpha"], (seed, rate)
        for t, n in V["spikes"]:
            assert flags[t, n] == 1, (seed, t, n)
        assert int(ref.counts.max()) == V["window"] - 1 and ref.n_done == V["T"]


def test_helper_on_hand_made_inputs():
    """the helper's own arithmetic: ties count, +inf is largest, -0 == +0, the row's own slot is left out, Bonferroni"""
    ref = anomaly_ref.AnomalyRef(0.5, 3, True, True, 1, 2, 2)
    f = np.zeros((2, 2), dtype=np.float32)
    ref.update(np.array([1.0, np.nan], dtype=np.float32), f)
    assert np.isnan(ref.pvalues).all() and np.isnan(ref.node_p).all() and ref.judged_sum.sum() == 0          # m = 0 < 1
    ref.update(np.array([1.0, 2.0], dtype=np.float32), f)                        # a tie with the one score: ge = 1
    assert ref.pvalues[0, 0] == 1.0 and np.isnan(ref.pvalues[0, 1]) and ref.counts[0, 0] == 1 and ref.counts[0, 1] == 0
    ref.update(np.array([3.0, 1.0], dtype=np.float32), np.array([[0, 0], [np.nan, 0]], dtype=np.float32))
    assert ref.pvalues[0, 0] == np.float32(1 / 3) and ref.pvalues[1, 0] == np.float32(1 / 3) and ref.scores[2, 1, 0] == np.inf
    assert ref.node_p[0] == np.float32(2 * np.float64(np.float32(1 / 3))) and ref.alarm[0] == 0
    assert ref.pvalues[0, 1] == 1.0 and ref.node_p[1] == 1.0                     # 1.0 below the one score 2.0: ge = 1 of m = 1
    ref.update(np.array([0.5, 9.0], dtype=np.float32), f)                        # slot 0 is left out: the population is rows 1, 2
    assert ref.counts[0, 0] == 2 and ref.pvalues[0, 0] == 1.0 and ref.pvalues[1, 0] == 1.0
    assert ref.pvalues[0, 1] == np.float32(1 / 3) and ref.node_p[1] == np.float32(2 * np.float64(np.float32(1 / 3)))
    assert anomaly_ref.scores_of(np.float32(0.0), np.float32(-0.0), np.float32(1.0)).view(np.uint32) == 0   # -0 -> +0
    assert anomaly_ref.scores_of(np.float32(0.0), np.float32(np.nan), np.float32(1.0)) == np.inf
    rec, rows = ref.recent()
    assert rows.tolist() == [0, 1, 2, 3] and rec.shape == (4, 2)
