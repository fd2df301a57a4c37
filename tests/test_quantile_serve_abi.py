"""CPU: the serving-epilogue entries of include/stemgnn_hip.h (csrc/quantile_serve.hip) are exported, declared and bound; every
bad argument is refused before any launch; the Python layers refuse what they cannot serve.  Nothing is launched."""
import ctypes
import inspect
import os

import pytest
import torch

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NEW = ("stemgnn_quantile_finish", "stemgnn_quantile_store")
TAUS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_quantile_finish"][1]) == 14 and len(sig["stemgnn_quantile_store"][1]) == 18
    assert sig["stemgnn_quantile_finish"][1][1] is ctypes.c_long and sig["stemgnn_quantile_store"][1][16] is ctypes.c_long
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "quantile_serve.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    for fn, names in ((ops.quantile_finish, ("forecast", "rearrange", "offsets", "pairs", "per_step", "per_node", "out")),
                      (ops.quantile_store, ("steps", "target", "pos", "out_forecast", "out_target", "rearrange", "offsets",
                                            "pairs", "per_step", "per_node"))):
        assert tuple(inspect.signature(fn).parameters) == names
    par = inspect.signature(ops.quantile_finish).parameters
    assert par["rearrange"].default is False and par["offsets"].default is None and par["per_step"].default is True
    assert par["per_node"].default is False and par["out"].default is None


# the arguments of the two entries, in order (the stream follows); offsets given, so the pair checks are live
FINISH_OK = dict(forecast=P, count=70, Q=5, H=3, N=11, rearrange=1, offsets=P, P=2, lo=ints(0, 1), hi=ints(4, 3), per_step=1,
                 per_node=0, out=P)
STORE_OK = dict(steps=P, target=P, pos=P, B=7, Q=5, H=3, N=11, rearrange=1, offsets=P, P=2, lo=ints(0, 1), hi=ints(4, 3),
                per_step=1, per_node=0, out_forecast=P, out_target=P, capacity=70)
BAD_PAIRS = [((0, 1), (5, 3)), ((-1, 1), (4, 3)), ((4, 1), (0, 3)), ((2, 1), (2, 3)), ((0, 0), (4, 3)), ((0, 1), (4, 4)),
             ((0, 3), (4, 4)), ((0, 1), (3, 3)), ((0, 1), (1, 3))]


def refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == SG_EINVAL


@pytest.mark.parametrize("entry", NEW)
def test_entries_reject_bad_arguments(lib, entry):
    f = getattr(lib, entry)
    finish = entry.endswith("finish")
    ok = FINISH_OK if finish else STORE_OK
    count = "count" if finish else "B"
    pointers = ("forecast", "out") if finish else ("steps", "target", "pos", "out_forecast", "out_target")
    for k in pointers + ("lo", "hi"):
        assert refused(f, ok, **{k: None}), k
    for k in (count, "Q", "H", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
            assert refused(f, ok, **{k: v, "offsets": None}), (k, v)          # a bad dimension is one with either stage
    assert refused(f, ok, Q=33, hi=ints(32, 31))
    assert refused(f, ok, Q=33, offsets=None)
    assert refused(f, ok, Q=33, offsets=None, rearrange=0)
    assert refused(f, ok, H=2 ** 16, N=2 ** 15, offsets=None)                 # H * N >= 2^31
    if not finish:
        for v in (0, -1):
            assert refused(f, ok, capacity=v), v
            assert refused(f, ok, capacity=v, offsets=None, rearrange=0), v
    # with offsets: everything stemgnn_conformal_apply refuses
    for v in (0, -1, 17):
        assert refused(f, ok, P=v), v
    for lo, hi in BAD_PAIRS:
        assert refused(f, ok, lo=ints(*lo), hi=ints(*hi)), (lo, hi)
    assert refused(f, ok, Q=32, P=17, lo=ints(*range(17)), hi=ints(*range(31, 14, -1)))
    assert refused(f, ok, **{count: 2 ** 31 // 33 + 1})                       # count * H * N >= 2^31


def test_python_layers_refuse_what_they_cannot_serve():
    from stemgnn_amd import Model, trainer
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.engine import ForecastStep, QuantileForecastStep
    from stemgnn_amd.math_utils import ConformalCalibrator, rearrange_quantiles
    series = torch.zeros(40, 6)
    plain, quant = Model(6, 2, 4, 2, horizon=2), Model(6, 2, 4, 2, horizon=2, quantiles=TAUS)
    with pytest.raises(ValueError, match="needs a quantile model"):
        QuantileForecastStep(plain, 4, 4, 2, series, 8)
    with pytest.raises(ValueError, match="quantile model"):                    # ... and the point class keeps refusing the other
        ForecastStep(quant, 4, 4, 2, series, 8)
    with pytest.raises(ValueError, match="not fitted"):
        QuantileForecastStep(quant, 4, 4, 2, series, 8, calibrator=ConformalCalibrator(TAUS))

    def fitted(taus, shape, **kw):
        cal = ConformalCalibrator(taus, **kw)
        return cal.load_state_dict(dict(cal.state_dict(), offsets=torch.zeros(shape), counts=torch.zeros(shape, dtype=torch.int64)))

    with pytest.raises(ValueError, match="levels"):
        QuantileForecastStep(quant, 4, 4, 2, series, 8, calibrator=fitted((0.2, 0.5, 0.8), (1, 2, 1)))
    with pytest.raises(ValueError, match="levels"):
        QuantileForecastStep(quant, 4, 4, 2, series, 8, calibrator=fitted((0.1, 0.9), (1, 2, 1)))
    with pytest.raises(ValueError, match="do not fit horizon 5"):             # a per-step calibrator fitted on 2 steps
        QuantileForecastStep(quant, 4, 4, 5, series, 8, calibrator=fitted(TAUS, (1, 2, 1)))
    with pytest.raises(ValueError, match="do not fit"):                       # a per-node calibrator of another width
        QuantileForecastStep(quant, 4, 4, 2, series, 8, calibrator=fitted(TAUS, (1, 1, 7), per_step=False, per_node=True))
    # the trainer's entry refuses the same, and a dataset of another horizon
    ds = type("D", (), dict(horizon=2, window_size=4, data=series, hi_all=torch.arange(4, 12), __len__=lambda self: 8))()
    with pytest.raises(ValueError, match="needs a quantile model"):
        trainer.rolling_quantile_forecast_graph(plain, ds, 2, 4)
    with pytest.raises(ValueError, match="not fitted"):
        trainer.rolling_quantile_forecast_graph(quant, ds, 2, 4, calibrator=ConformalCalibrator(TAUS))
    with pytest.raises(ValueError, match="dataset horizon"):
        trainer.rolling_quantile_forecast_graph(quant, ds, 5, 4)
    # the ops wrappers: no CPU fallback, and the shapes of their neighbours
    y_hat = torch.zeros(4, 3, 2, 6)
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        rearrange_quantiles(y_hat)
    par = inspect.signature(trainer.rolling_quantile_forecast_graph).parameters
    assert par["rearrange"].default is False and par["calibrator"].default is None and par["adjacency"].default is None
