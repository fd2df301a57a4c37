"""CPU: the conformal entries of include/stemgnn_hip.h (csrc/conformal.hip) are exported, declared and bound; the host rank
formula equals its Python restatement; every bad argument is refused before any launch; the Python layers refuse what they
cannot calibrate.  Nothing is launched."""
import ctypes
import inspect
import math
import os

import pytest
import torch

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NEW = ("stemgnn_conformal_rank", "stemgnn_conformal_scratch_bytes", "stemgnn_conformal_fit", "stemgnn_conformal_apply")
NAN = float("nan")


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


def rank(m, c):
    """the definition: two fp64 multiplies and a ceil"""
    t = (m + 1) * c
    return math.ceil(t * (1 - 1e-12))


def test_symbols_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_conformal_fit"][1]) == 17 and len(sig["stemgnn_conformal_apply"][1]) == 13
    assert sig["stemgnn_conformal_rank"] == (ctypes.c_long, [ctypes.c_long, ctypes.c_double])
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "conformal.hip" in makefile.split("SRCS =")[1].splitlines()[0]


def test_rank_equals_the_python_formula(lib):
    assert 0.9 - 0.1 == 0.8
    for m, c, want in ((99, 0.8, 80), (9, 0.8, 8), (4, 0.8, 4), (3, 0.8, 4)):
        assert rank(m, c) == want
        assert lib.stemgnn_conformal_rank(m, c) == want, (m, c)
    for c in (1e-6, 0.5, 0.8, 0.9 - 0.1, 0.98, 1 - 1e-9):
        assert lib.stemgnn_conformal_rank(0, c) == 1 == rank(0, c), c
    for c in (0.5, 0.8, 0.9, 0.98):
        for m in range(5000):
            assert lib.stemgnn_conformal_rank(m, c) == rank(m, c), (m, c)
    for m, c in ((2 ** 31 - 2, 0.98), (123456789, 0.9 - 0.1), (4097, (4097 - 0.5) / 4098), (257, 1 - 1e-9), (256, 1e-6)):
        assert lib.stemgnn_conformal_rank(m, c) == rank(m, c), (m, c)


FIT_OK = dict(target=P, forecast=P, count=70, Q=5, H=3, N=11, P=2, lo=ints(0, 1), hi=ints(4, 3), cov=doubles(0.8, 0.4),
              per_step=1, per_node=0, masked=0, scratch=P, offsets=P, counts=P)
BAD_PAIRS = [((0, 1), (5, 3)), ((-1, 1), (4, 3)), ((4, 1), (0, 3)), ((2, 1), (2, 3)), ((0, 0), (4, 3)), ((0, 1), (4, 4)),
             ((0, 3), (4, 4)), ((0, 1), (3, 3)), ((0, 1), (1, 3))]
BAD_SHAPES = (("count", 0), ("Q", 0), ("H", 0), ("N", 0), ("P", 0), ("count", -1), ("Q", -5), ("H", -1), ("N", -2), ("P", -1))


def test_fit_rejects_bad_arguments(lib):
    f = lib.stemgnn_conformal_fit
    for k in ("target", "forecast", "lo", "hi", "cov", "scratch", "offsets", "counts"):
        assert f(*{**FIT_OK, k: None}.values(), None) == SG_EINVAL, k
    for k, v in BAD_SHAPES:
        assert f(*{**FIT_OK, k: v}.values(), None) == SG_EINVAL, (k, v)
    for lo, hi in BAD_PAIRS:
        assert f(*{**FIT_OK, "lo": ints(*lo), "hi": ints(*hi)}.values(), None) == SG_EINVAL, (lo, hi)
    for bad in ((NAN, 0.4), (0.8, 0.0), (1.0, 0.4), (0.8, -0.1), (1.5, 0.4), (0.8, NAN)):
        assert f(*{**FIT_OK, "cov": doubles(*bad)}.values(), None) == SG_EINVAL, bad
    # Q > 32; P > 16 (17 valid, distinct pairs need Q >= 34, so it is the Q limit or the P limit that refuses: both named)
    rows33 = dict(FIT_OK, Q=33, lo=ints(0, 1), hi=ints(32, 31))
    assert f(*rows33.values(), None) == SG_EINVAL
    lo17, hi17, cov17 = ints(*range(17)), ints(*range(31, 14, -1)), doubles(*([0.5] * 17))
    assert f(*dict(FIT_OK, Q=32, P=17, lo=lo17, hi=hi17, cov=cov17).values(), None) == SG_EINVAL
    assert f(*dict(FIT_OK, Q=32, P=16, lo=lo17, hi=hi17, cov=cov17, target=None).values(), None) == SG_EINVAL
    # count * H * N >= 2^31
    assert f(*dict(FIT_OK, count=2 ** 31 // 33 + 1).values(), None) == SG_EINVAL
    assert f(*dict(FIT_OK, count=2 ** 40).values(), None) == SG_EINVAL
    assert f(*dict(FIT_OK, scratch=P + 4).values(), None) == SG_EINVAL              # the scratch is 16-byte aligned


def test_apply_rejects_bad_arguments(lib):
    ok = dict(forecast=P, offsets=P, count=70, Q=5, H=3, N=11, P=2, lo=ints(0, 1), hi=ints(4, 3), per_step=1, per_node=0,
              out=P)
    f = lib.stemgnn_conformal_apply
    for k in ("forecast", "offsets", "lo", "hi", "out"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k, v in BAD_SHAPES:
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)
    for lo, hi in BAD_PAIRS:
        assert f(*{**ok, "lo": ints(*lo), "hi": ints(*hi)}.values(), None) == SG_EINVAL, (lo, hi)
    assert f(*dict(ok, Q=33, hi=ints(32, 31)).values(), None) == SG_EINVAL
    assert f(*dict(ok, Q=32, P=17, lo=ints(*range(17)), hi=ints(*range(31, 14, -1))).values(), None) == SG_EINVAL
    assert f(*dict(ok, count=2 ** 31 // 33 + 1).values(), None) == SG_EINVAL


def test_scratch_size(lib):
    size = lib.stemgnn_conformal_scratch_bytes
    for per_step in (0, 1):
        for per_node in (0, 1):
            groups = (3 if per_step else 1) * (11 if per_node else 1)
            for pairs in (1, 2, 16):
                assert size(70, 3, 11, pairs, per_step, per_node) == pairs * groups * (256 + 2) * 4
                # histograms and state only: the size does not grow with count (no staged keys, no P copies of anything)
                assert size(70000, 3, 11, pairs, per_step, per_node) == size(70, 3, 11, pairs, per_step, per_node)
    for bad in ((0, 3, 11, 2), (70, 0, 11, 2), (70, 3, 0, 2), (70, 3, 11, 0), (70, 3, 11, 17), (-1, 3, 11, 2),
                (2 ** 31 // 33 + 1, 3, 11, 2)):
        assert size(*bad, 1, 0) == 0, bad


def test_calibrator_refuses_one_level_and_cpu_tensors():
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.math_utils import ConformalCalibrator
    for bad in ((0.5,), ()):
        with pytest.raises(ValueError, match="pair"):
            ConformalCalibrator(bad)
    cal = ConformalCalibrator((0.1, 0.5, 0.9))
    assert cal.pairs == ((0, 2),) and cal.per_step is True and cal.per_node is False
    assert cal.interval_nominal.tolist() == [0.9 - 0.1]
    assert ConformalCalibrator((0.05, 0.25, 0.5, 0.75, 0.95), per_step=False, per_node=True).pairs == ((0, 4), (1, 3))
    y, y_hat = torch.zeros(4, 2, 3), torch.zeros(4, 3, 2, 3)
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        cal.fit(y, y_hat)
    with pytest.raises(ValueError, match="not fitted"):
        cal.apply(y_hat)
    cal.load_state_dict(dict(cal.state_dict(), offsets=torch.zeros(1, 2, 1), counts=torch.zeros(1, 2, 1, dtype=torch.int64)))
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):
        cal.apply(y_hat)
    with pytest.raises(ValueError):
        cal.apply(torch.zeros(4, 3, 5, 3))                                             # per_step: the fitted H


def test_calibrator_state_round_trip(tmp_path):
    from stemgnn_amd.math_utils import ConformalCalibrator
    cal = ConformalCalibrator((0.1, 0.5, 0.9), per_step=True, per_node=False)
    offsets = torch.tensor([[[0.25], [float("inf")], [-0.5]]])
    counts = torch.tensor([[[7], [0], [9]]])
    cal.load_state_dict(dict(cal.state_dict(), offsets=offsets, counts=counts))
    torch.save(cal.state_dict(), tmp_path / "c.pt")
    back = ConformalCalibrator.from_state_dict(torch.load(tmp_path / "c.pt", weights_only=False))
    assert torch.equal(back.offsets, offsets) and torch.equal(back.counts, counts)
    assert back.pairs == cal.pairs and back.quantiles == cal.quantiles and (back.per_step, back.per_node) == (True, False)
    with pytest.raises(ValueError):
        ConformalCalibrator((0.1, 0.9)).load_state_dict(cal.state_dict())


def test_trainer_keywords():
    from stemgnn_amd import trainer
    sig = inspect.signature(trainer.DeviceTrainer.__init__).parameters
    assert sig["calibrate"].default is False and sig["calibrate_per_step"].default is True
    assert sig["calibrate_per_node"].default is False
    assert inspect.signature(trainer.score_forecast).parameters["calibrator"].default is None
    with pytest.raises(ValueError, match="quantile"):
        trainer.DeviceTrainer(6, 4, 2, 2, calibrate=True, device="cpu")
    with pytest.raises(ValueError, match="quantile"):
        trainer.DeviceTrainer(6, 4, 2, 2, calibrate=True, quantiles=(0.5,), device="cpu")
