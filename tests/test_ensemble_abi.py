"""CPU: the ensemble-score entries of include/stemgnn_hip.h (csrc/ensemble.hip) are exported, declared and bound; every bad
argument is refused before any launch; the size entries have their values; the Python layers refuse what they cannot run and
the numpy restatement (tests/helpers/ensemble_ref.py) agrees with hand-worked values.  Nothing is launched."""
import inspect
import os

import numpy as np
import pytest
import torch

from tests.helpers import ensemble_ref as R

SG_EINVAL = -10001
P = 64                          # stand-in device addresses: every call below is refused before any use
NEW = ("stemgnn_ensemble_scratch_doubles", "stemgnn_ensemble_out_doubles", "stemgnn_ensemble_scores",
       "stemgnn_ensemble_scores_masked")
# the arguments of the two entries, in order (the stream follows)
OK = dict(target=P, paths=2 * P, mul=3 * P, add=4 * P, count=5, S=33, H=3, N=70, fair=0, scratch=5 * P, out=6 * P, hist=7 * P)


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def refused(f, **change):
    return f(*{**OK, **change}.values(), None) == SG_EINVAL


def test_symbols_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib, math_utils, ops, trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    sig = _lib.SIGNATURES
    assert sig["stemgnn_ensemble_scores_masked"] == sig["stemgnn_ensemble_scores"]
    assert len(sig["stemgnn_ensemble_scores"][1]) == 13
    makefile = open(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "Makefile")).read()
    assert "ensemble.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    par = inspect.signature(ops.ensemble_scores).parameters
    assert tuple(par) == ("y", "paths", "mul", "add", "ignore_nan", "fair")
    assert tuple(inspect.signature(math_utils.EnsembleScores.__init__).parameters)[1:] == tuple(par)
    par = inspect.signature(trainer.score_forecast).parameters
    assert par["paths"].default is None and par["fair"].default is False


def test_scores_reject_bad_arguments(lib):
    for f in (lib.stemgnn_ensemble_scores, lib.stemgnn_ensemble_scores_masked):
        for k in ("target", "paths", "scratch", "out", "hist"):
            assert refused(f, **{k: None}), k
        assert refused(f, mul=None) and refused(f, add=None)                   # one without the other
        for k in ("count", "S", "H", "N"):
            for v in (0, -1):
                assert refused(f, **{k: v}), (k, v)
        assert refused(f, S=1025)
        assert refused(f, S=1, fair=1)
        # products that do not fit the kernels' ints
        assert refused(f, count=2 ** 31)                                       # count itself
        assert refused(f, count=2 ** 30, H=2)                                  # count * H
        assert refused(f, count=2 ** 28, S=1, H=1, N=1024)                     # the marginal grid: count * H * ceil(N / 64)
        assert refused(f, count=2 ** 22, S=1024, H=1, N=1)                     # the energy grid: count * H * 528
        assert refused(f, count=1, S=1, H=2 ** 16, N=2 ** 15)                  # H * N
        assert refused(f, count=1, S=1024, H=2 ** 21, N=1)                     # H * (S + 1), S * H * N


def test_size_entries(lib):
    scratch, out = lib.stemgnn_ensemble_scratch_doubles, lib.stemgnn_ensemble_out_doubles
    for H in (1, 3, 12, 288):
        assert out(H) == 6 * (1 + H)
    assert out(0) == 0 and out(-1) == 0
    for shape in ((1, 1, 1, 1), (3, 2, 2, 5), (7, 33, 3, 70), (2, 100, 1, 64), (5, 64, 3, 12), (1, 1024, 1, 8),
                  (2520, 64, 12, 228)):
        count, S, H, N = shape
        n = scratch(*shape)
        assert n > 0, shape
        # at least one partial per statistic, row and kernel; a small multiple of the rows, far below the input itself
        assert 8 * count * H <= n <= count * H * (5 * ((N + 3) // 4) + 2 * 528 + 1), shape
    assert scratch(2520, 64, 12, 228) < 2520 * 12 * 228                        # PEMS07: the scratch is below the target's size
    for bad in ((0, 8, 3, 4), (-1, 8, 3, 4), (5, 0, 3, 4), (5, 1025, 3, 4), (5, 8, 0, 4), (5, 8, 3, 0), (5, 8, -3, 4),
                (2 ** 31, 1, 1, 1), (2 ** 30, 1, 2, 1), (2 ** 22, 1024, 1, 1), (1, 1, 2 ** 16, 2 ** 15)):
        assert scratch(*bad) == 0, bad


def test_ops_refuse_before_touching_the_library(monkeypatch):
    from stemgnn_amd import _lib, ops
    from stemgnn_amd._lib import StemGNNHipError

    def no_load():
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_load)
    y, p = torch.zeros(2, 3, 4), torch.zeros(2, 5, 3, 4)
    for bad_y, bad_p in ((y[0], p), (y, p[0]), (y, torch.zeros(2, 5, 3, 5)), (y, torch.zeros(3, 5, 3, 4)),
                         (torch.zeros(2, 4, 3), p)):
        with pytest.raises(StemGNNHipError, match=r"y must be \[count,H,N\] and paths \[count,S,H,N\]"):
            ops.ensemble_scores(bad_y, bad_p)
    for bad_y, bad_p in ((y.double(), p), (y, p.double()), (y, p.half()), (y.long(), p)):
        with pytest.raises(StemGNNHipError, match="contiguous float32"):
            ops.ensemble_scores(bad_y, bad_p)
    with pytest.raises(StemGNNHipError, match="contiguous float32"):
        ops.ensemble_scores(y, torch.zeros(2, 3, 5, 4).transpose(1, 2))
    with pytest.raises(StemGNNHipError, match="contiguous float32"):
        ops.ensemble_scores(torch.zeros(2, 3, 8)[:, :, ::2], p)
    with pytest.raises(StemGNNHipError, match="mul and add go together"):
        ops.ensemble_scores(y, p, mul=torch.ones(4))
    with pytest.raises(StemGNNHipError, match="1 to 1024"):
        ops.ensemble_scores(y, torch.zeros(2, 1025, 3, 4))
    with pytest.raises(StemGNNHipError, match="fair=True needs at least 2"):
        ops.ensemble_scores(y, torch.zeros(2, 1, 3, 4), fair=True)
    with pytest.raises(StemGNNHipError, match="no CPU fallback"):               # a host tensor: no fallback
        ops.ensemble_scores(y, p)


def test_python_layers_have_no_cpu_fallback():
    from stemgnn_amd import math_utils, trainer
    from stemgnn_amd._lib import StemGNNHipError
    y, p = torch.zeros(2, 3, 4), torch.zeros(2, 5, 3, 4)
    with pytest.raises(StemGNNHipError):
        math_utils.EnsembleScores(y, p)
    with pytest.raises(StemGNNHipError):
        trainer.score_forecast(torch.zeros(2, 3, 3, 4), y, quantiles=(0.1, 0.5, 0.9), paths=p)


def test_the_restatement_on_hand_worked_values():
    # one element, S = 2: x = (1, 3), y = 2: crps = 1 - 2 / (2 * 4) * 2 = 0.5; fair: 1 - 2 * 2 / (2 * 2) = 0
    y = np.array([[[2.0]]], np.float32)
    x = np.array([[[[1.0]], [[3.0]]]], np.float32)
    r = R.scores(y, x)
    assert r["out"][0] == 0.5 and r["out"][1] == 0.5                             # one node: the energy score is the crps
    assert r["out"][2] == 0.0 and r["out"][3] == np.sqrt(2.0) and r["out"][4] == 1 and r["out"][5] == 1
    assert r["hist"].tolist() == [[0, 1, 0]]
    assert R.scores(y, x, fair=True)["out"][0] == 0.0
    # de-normalisation scales crps, energy, rmse and spread by mul; the ranks do not move
    r2 = R.scores(y, x, mul=np.array([4.0]), add=np.array([-7.0]))
    assert np.array_equal(r2["out"][:4], 4 * r["out"][:4]) and np.array_equal(r2["hist"], r["hist"])
    # the midrank rule: y equal to one, two and all of three values; -0 == +0
    for vals, yv, want in (((1, 2, 3), 2, 1), ((2, 2, 3), 2, 1), ((1, 2, 2), 2, 2), ((2, 2, 2), 2, 1), ((0.0, -0.0, 5), -0.0, 1),
                           ((1, 2, 3), 0, 0), ((1, 2, 3), 4, 3), ((np.nan, 2, 3), 2.5, 1)):
        x = np.array(vals, np.float32).reshape(1, 3, 1, 1)
        h = R.scores(np.full((1, 1, 1), yv, np.float32), x)["hist"][0]
        assert h[want] == 1 and h.sum() == 1, (vals, yv, h)
    # two nodes, S = 2, paths (0, 0) and (3, 4), y = (0, 0): energy = (0 + 5) / 2 - (2 * 5) / 8 = 1.25
    y = np.zeros((1, 1, 2), np.float32)
    x = np.array([[[[0, 0]], [[3, 4]]]], np.float32)
    r = R.scores(y, x)
    assert r["out"][1] == 1.25 and r["out"][0] == ((1.5 - 0.75) + (2 - 1)) / 2
    # masked: the NaN node leaves V; a row of NaN only leaves [1] and [5]
    y = np.array([[[0, np.nan]], [[np.nan, np.nan]]], np.float32)
    x = np.concatenate([x, x])
    r = R.scores(y, x, masked=True)
    assert r["out"][1] == 1.5 - 0.75 and r["out"][4] == 1 and r["out"][5] == 1 and r["hist"].sum() == 1
    plain = R.scores(y, x)
    assert np.isnan(plain["out"][:3]).all() and plain["out"][4] == 4 and plain["out"][5] == 2 and plain["hist"].sum() == 1
    assert plain["out"][3] == 2.5                                                # the spread does not involve the target
