"""CPU: the seasonal conformal entries of include/stemgnn_hip.h (csrc/seasonal.hip) are exported, declared and bound; the host
bucket formula equals its Python restatement; the scratch size; every bad argument is refused before any launch; the Python
layers refuse what they cannot serve.  Nothing is launched."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from tests.helpers import seasonal_ref as R

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NEW = ("stemgnn_season_bucket", "stemgnn_seasonal_scratch_bytes", "stemgnn_seasonal_fit", "stemgnn_seasonal_apply",
       "stemgnn_quantile_store_seasonal")
NAN = float("nan")
SEASONS = ((1, 1, 0), (7, 7, 0), (12, 4, 5), (288, 24, 100), (10, 3, 9))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def doubles(*v):
    return (ctypes.c_double * len(v))(*v)


# ---- declarations ---------------------------------------------------------------------------------------------------------
C_TYPES = {"int": ctypes.c_int, "long": ctypes.c_long, "long long": ctypes.c_longlong, "size_t": ctypes.c_size_t,
           "double": ctypes.c_double, "const int*": ctypes.POINTER(ctypes.c_int), "const double*": ctypes.POINTER(ctypes.c_double)}


def header_signature(name):
    """(restype, argtypes) of a declaration of include/stemgnn_hip.h; device pointers are void pointers in the binding"""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "stemgnn_hip.h")).read(), flags=re.S)
    res, args = re.search(r"(\w[\w ]*?)\s+" + name + r"\s*\(([^)]*)\)\s*;", src).groups()
    types = []
    for a in args.split(","):
        kind = re.sub(r"\s+", " ", a.strip()).rsplit(" ", 1)[0].replace(" *", "*")
        types.append(C_TYPES.get(kind, ctypes.c_void_p))
    return C_TYPES[res.strip()], types


def test_symbols_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        res, args = header_signature(name)
        assert _lib.SIGNATURES[name][0] is res, name
        assert list(_lib.SIGNATURES[name][1]) == args, name
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_seasonal_fit"][1]) == 22 and len(sig["stemgnn_seasonal_apply"][1]) == 19
    assert len(sig["stemgnn_quantile_store_seasonal"][1]) == 22
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "seasonal.hip" in makefile.split("SRCS =")[1].splitlines()[0]


# ---- the bucket formula -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("season", SEASONS, ids=str)
def test_bucket_equals_the_python_formula(lib, season):
    period, K, phase = season
    ts = list(range(-3 * period, 3 * period + 1))
    for centre in (2 ** 40, -2 ** 40):
        ts += list(range(centre - period - 2, centre + period + 3))
    for t in ts:
        got = lib.stemgnn_season_bucket(t, period, K, phase)
        assert got == R.bucket(t, period, K, phase) == ((t + phase) % period) * K // period, (t, season)
        assert 0 <= got < K
    # in u = (t + phase) mod period: non-decreasing, and every bucket is hit
    by_u = [lib.stemgnn_season_bucket(u - phase, period, K, phase) for u in range(period)]
    assert by_u == sorted(by_u) and set(by_u) == set(range(K)), season
    assert by_u == [u * K // period for u in range(period)]


def test_bucket_refuses_a_bad_season(lib):
    for bad in ((0, 1, 0), (-3, 1, 0), (5, 0, 0), (5, -1, 0), (5, 6, 0), (5, 2, -1), (5, 2, 5), (2 ** 31, 4, 0)):
        assert lib.stemgnn_season_bucket(7, *bad) == -1, bad
    assert lib.stemgnn_season_bucket(7, 2 ** 31 - 1, 4, 0) == 0


def test_calibrator_bucket_of_is_the_formula():
    from stemgnn_amd.math_utils import SeasonalConformalCalibrator
    for period, K, phase in SEASONS:
        cal = SeasonalConformalCalibrator((0.1, 0.9), period, K, phase)
        for t in (-2 ** 40, -period - 1, -1, 0, 1, period - 1, period, 3 * period + 2, 2 ** 40 + 3):
            assert cal.bucket_of(t) == R.bucket(t, period, K, phase)


# ---- scratch ----------------------------------------------------------------------------------------------------------------
def test_scratch_size(lib):
    size, unseasoned = lib.stemgnn_seasonal_scratch_bytes, lib.stemgnn_conformal_scratch_bytes
    for per_step in (0, 1):
        for per_node in (0, 1):
            groups = (3 if per_step else 1) * (11 if per_node else 1)
            for pairs in (1, 2, 16):
                for K in (1, 4, 24):
                    assert size(70, 3, 11, pairs, K, per_step, per_node) == K * pairs * groups * (256 + 2) * 4
                    assert size(70, 3, 11, pairs, K, per_step, per_node) == K * unseasoned(70, 3, 11, pairs, per_step, per_node)
                    # histograms and state only: the size does not grow with count
                    assert size(70000, 3, 11, pairs, K, per_step, per_node) == size(70, 3, 11, pairs, K, per_step, per_node)
    for bad in ((0, 3, 11, 2, 4), (70, 0, 11, 2, 4), (70, 3, 0, 2, 4), (70, 3, 11, 0, 4), (70, 3, 11, 17, 4), (-1, 3, 11, 2, 4),
                (2 ** 31 // 33 + 1, 3, 11, 2, 4), (70, 3, 11, 2, 0), (70, 3, 11, 2, -1), (70, 3, 11, 2, 32768),
                (70, 3, 11, 16, 4096)):
        assert size(*bad, 1, 0) == 0, bad
    assert size(70, 3, 11, 1, 65535, 1, 0) == 65535 * 3 * 258 * 4                    # P * K == 65535 is served
    assert size(70, 300, 1000, 1, 2048, 1, 1) == 0                                   # K P G = 2048 * 300000 >= 2^29
    assert size(70, 300, 1000, 1, 1024, 1, 1) == 1024 * 300000 * 258 * 4


# ---- refusals, each with one bad argument among otherwise valid ones ------------------------------------------------------------
BAD_PAIRS = [((0, 1), (5, 3)), ((-1, 1), (4, 3)), ((4, 1), (0, 3)), ((2, 1), (2, 3)), ((0, 0), (4, 3)), ((0, 1), (4, 4)),
             ((0, 3), (4, 4)), ((0, 1), (3, 3)), ((0, 1), (1, 3))]
BAD_SHAPES = (("count", 0), ("Q", 0), ("H", 0), ("N", 0), ("P", 0), ("count", -1), ("Q", -5), ("H", -1), ("N", -2), ("P", -1))
BAD_SEASONS = (("period", 0), ("period", -288), ("period", 2 ** 31), ("K", 0), ("K", -1), ("K", 289), ("phase", -1),
               ("phase", 288), ("phase", 2 ** 40), ("K", 32768))               # the last: P * K = 65536 > 65535
FIT_OK = dict(target=P, forecast=P, origins=None, origin0=-5, count=70, Q=5, H=3, N=11, P=2, lo=ints(0, 1), hi=ints(4, 3),
              cov=doubles(0.8, 0.4), per_step=1, per_node=0, masked=0, period=288, K=24, phase=100, scratch=P, offsets=P,
              counts=P)
APPLY_OK = dict(forecast=P, offsets=P, origins=None, origin0=7, count=70, Q=5, H=3, N=11, rearrange=0, P=2, lo=ints(0, 1),
                hi=ints(4, 3), per_step=1, per_node=0, period=288, K=24, phase=100, out=P)
STORE_OK = dict(steps=P, target=P, pos=P, t_dev=P, B=4, Q=5, H=3, N=11, rearrange=1, offsets=P, P=2, lo=ints(0, 1),
                hi=ints(4, 3), per_step=1, per_node=0, period=288, K=24, phase=100, out_forecast=P, out_target=P, capacity=9)


def refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == SG_EINVAL


def common_refusals(f, ok, count_key):
    for k, v in BAD_SHAPES:
        k = count_key if k == "count" else k
        assert refused(f, ok, **{k: v}), (k, v)
    for lo, hi in BAD_PAIRS:
        assert refused(f, ok, lo=ints(*lo), hi=ints(*hi)), (lo, hi)
    for k, v in BAD_SEASONS:
        if k == "K" and v == 32768:
            assert refused(f, ok, K=v, period=2 ** 20), (k, v)
        else:
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, Q=33, hi=ints(32, 31))
    assert refused(f, ok, Q=32, P=17, lo=ints(*range(17)), hi=ints(*range(31, 14, -1)), cov=doubles(*([0.5] * 17))) \
        if "cov" in ok else refused(f, ok, Q=32, P=17, lo=ints(*range(17)), hi=ints(*range(31, 14, -1)))
    # K P G >= 2^29, every single factor being fine
    assert refused(f, ok, **{count_key: 1}, H=300, N=1000, per_step=1, per_node=1, K=2048, period=4096, P=1, lo=ints(0),
                   hi=ints(4), **({"cov": doubles(0.8)} if "cov" in ok else {}))


def test_fit_rejects_bad_arguments(lib):
    f = lib.stemgnn_seasonal_fit
    for k in ("target", "forecast", "lo", "hi", "cov", "scratch", "offsets", "counts"):
        assert refused(f, FIT_OK, **{k: None}), k
    common_refusals(f, FIT_OK, "count")
    for bad in ((NAN, 0.4), (0.8, 0.0), (1.0, 0.4), (0.8, -0.1), (1.5, 0.4), (0.8, NAN)):
        assert refused(f, FIT_OK, cov=doubles(*bad)), bad
    assert refused(f, FIT_OK, count=2 ** 31 // 33 + 1) and refused(f, FIT_OK, count=2 ** 40)     # count * H * N >= 2^31
    assert refused(f, FIT_OK, scratch=P + 4)                                                       # 16-byte aligned
    assert refused(f, FIT_OK, origins=P, period=0)                                                 # the tensor form too
    assert refused(f, FIT_OK, count=2, H=65536, N=1, per_step=1, per_node=0, K=1)                   # grid.y of the stream form


def test_apply_rejects_bad_arguments(lib):
    f = lib.stemgnn_seasonal_apply
    for k in ("forecast", "offsets", "lo", "hi", "out"):
        assert refused(f, APPLY_OK, **{k: None}), k
    for rearrange in (0, 1):
        common_refusals(f, dict(APPLY_OK, rearrange=rearrange), "count")
    assert refused(f, APPLY_OK, count=2 ** 31 // 33 + 1)


def test_store_rejects_bad_arguments(lib):
    f = lib.stemgnn_quantile_store_seasonal
    for k in ("steps", "target", "pos", "t_dev", "offsets", "lo", "hi", "out_forecast", "out_target"):
        assert refused(f, STORE_OK, **{k: None}), k
    common_refusals(f, STORE_OK, "B")
    for capacity in (0, -3):
        assert refused(f, STORE_OK, capacity=capacity)


# ---- the Python layers ------------------------------------------------------------------------------------------------------
def test_calibrator_refusals_and_state_round_trip(tmp_path):
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import ConformalCalibrator, SeasonalConformalCalibrator
    for bad in ((0, 1, 0), (288, 0, 0), (288, 289, 0), (288, 24, 288), (288, 24, -1), (2 ** 31, 24, 0)):
        with pytest.raises(ValueError, match="season"):
            SeasonalConformalCalibrator((0.1, 0.5, 0.9), *bad)
    with pytest.raises(ValueError, match="pair"):
        SeasonalConformalCalibrator((0.5,), 288, 24)
    with pytest.raises(ValueError, match="fallback"):
        SeasonalConformalCalibrator((0.1, 0.9), 288, 24, fallback="zero")
    with pytest.raises(ValueError, match="min_scores"):
        SeasonalConformalCalibrator((0.1, 0.9), 288, 24, min_scores=-1)
    cal = SeasonalConformalCalibrator((0.1, 0.5, 0.9), 12, 4, phase=5)
    assert cal.kind == "seasonal" and cal.pairs == ((0, 2),) and (cal.per_step, cal.per_node) == (True, False)
    assert cal.interval_nominal.tolist() == [0.9 - 0.1] and (cal.min_scores, cal.fallback) == (0, "pooled")
    # m_min: rank(m, c) <= m first holds at m = 4 for c = 0.8 (ranks 1, 2, 3, 4, 4 of m = 0 .. 4)
    assert [R.rank(m, 0.9 - 0.1) for m in range(5)] == [1, 2, 3, 4, 4]
    assert cal.thresholds() == [4] == [R.min_count(0.9 - 0.1)] and cal.min_count(0.5) == 1 == R.min_count(0.5)
    assert SeasonalConformalCalibrator((0.1, 0.9), 12, 4, min_scores=30).thresholds() == [30]
    y, y_hat = torch.zeros(4, 2, 3), torch.zeros(4, 3, 2, 3)
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        cal.fit(y, y_hat, 0)
    with pytest.raises(ValueError, match="not fitted"):
        cal.apply(y_hat, 0)
    offsets = torch.arange(8, dtype=torch.float32).reshape(4, 1, 2, 1)
    offsets[1, 0, 1, 0] = float("inf")
    counts = torch.arange(8).reshape(4, 1, 2, 1)
    cal.load_state_dict(dict(cal.state_dict(), offsets=offsets, counts=counts))
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        cal.apply(y_hat, 0)
    with pytest.raises(ValueError):
        cal.apply(torch.zeros(4, 3, 5, 3), 0)                                          # per_step: the fitted H
    torch.save(cal.state_dict(), tmp_path / "s.pt")
    state = torch.load(tmp_path / "s.pt", weights_only=False)
    assert state["kind"] == "seasonal" and (state["period"], state["buckets"], state["phase"]) == (12, 4, 5)
    back = SeasonalConformalCalibrator.from_state_dict(state)
    assert torch.equal(back.offsets, offsets) and torch.equal(back.counts, counts)
    assert (back.period, back.buckets, back.phase, back.pairs, back.quantiles) == (12, 4, 5, cal.pairs, cal.quantiles)
    with pytest.raises(ValueError):
        SeasonalConformalCalibrator((0.1, 0.5, 0.9), 12, 3, phase=5).load_state_dict(state)        # other buckets
    with pytest.raises(ValueError, match="kind"):
        cal.load_state_dict(ConformalCalibrator((0.1, 0.5, 0.9)).state_dict())                     # a static state


def test_keywords_are_optional_and_absent_by_default():
    from stemgnn_amd import LiveForecaster, ops, trainer
    assert inspect.signature(trainer.score_forecast).parameters["origin"].default is None
    assert inspect.signature(LiveForecaster.set_calibrator).parameters["t_offset"].default == 0
    assert "seasonal" not in inspect.signature(ops.quantile_store).parameters          # the unseasoned store is as it was
    assert "t_offset" not in inspect.signature(LiveForecaster.__init__).parameters
    sig = inspect.signature(ops.quantile_store_seasonal).parameters
    assert tuple(sig)[:10] == tuple(inspect.signature(ops.quantile_store).parameters) and tuple(sig)[10:] == ("seasonal", "t_dev")


def test_serving_layers_refuse_what_they_cannot_serve():
    from stemgnn_amd import LiveForecaster, Model, trainer
    from stemgnn_amd.engine import QuantileForecastStep
    from stemgnn_amd.math_utils import AdaptiveConformal, SeasonalConformalCalibrator
    taus = (0.1, 0.5, 0.9)
    cal = SeasonalConformalCalibrator(taus, 6, 3)
    fitted = SeasonalConformalCalibrator(taus, 6, 3)
    fitted.load_state_dict(dict(fitted.state_dict(), offsets=torch.zeros(3, 1, 5, 1), counts=torch.zeros(3, 1, 5, 1).long()))
    quant, point = Model(6, 2, 4, 2, horizon=2, quantiles=taus), Model(6, 2, 4, 2, horizon=2)
    with pytest.raises(ValueError, match="seasonal"):
        QuantileForecastStep(quant, 2, 4, 5, None, 8, calibrator=fitted)
    with pytest.raises(ValueError, match="not fitted"):
        LiveForecaster(quant, 4, 5, calibrator=cal)
    with pytest.raises(ValueError, match="point model"):
        LiveForecaster(point, 4, 5, calibrator=fitted)
    with pytest.raises(ValueError, match="quantile model"):
        LiveForecaster(point, 4, 5).set_calibrator(fitted, t_offset=4)
    with pytest.raises(ValueError, match="horizon"):
        LiveForecaster(quant, 4, 3).set_calibrator(fitted)
    live = LiveForecaster(quant, 4, 5, history=8)
    live.set_calibrator(fitted, t_offset=4)
    assert live.t_offset == 4 and live._season(fitted) == (6, 3, 4)
    with pytest.raises(ValueError, match="seasonal"):
        live.set_adaptive(AdaptiveConformal(taus))
    other = LiveForecaster(quant, 4, 5, history=8)
    other.set_adaptive(AdaptiveConformal(taus))
    with pytest.raises(ValueError, match="adaptive"):
        other.set_calibrator(fitted)
    f, y = torch.zeros(4, 3, 5, 6), torch.zeros(4, 5, 6)
    with pytest.raises(ValueError, match="origin"):
        trainer.score_forecast(f, y, quantiles=taus, calibrator=fitted)
