"""CPU: the loss / missing-value entries of include/stemgnn_hip.h (csrc/tail.hip, csrc/data.hip) are exported and declared,
refuse bad arguments before any launch, and the Python layers expose the new options behind defaults.  Nothing is launched."""
import inspect
import os

import numpy as np
import pytest

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NEW = ("stemgnn_target_valid_count", "stemgnn_fc_tail_train_loss", "stemgnn_fc_tail_train_rows_loss",
       "stemgnn_fc_tail_train_finish_loss", "stemgnn_window_gather_pair", "stemgnn_window_gather_queue_pair",
       "stemgnn_eval_metrics_masked", "stemgnn_eval_scratch_doubles_masked")
MSE, MAE, HUBER = 0, 1, 2


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_new_symbols_exported_and_declared(lib):
    from stemgnn_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert "SG_LOSS_MSE = 0, SG_LOSS_MAE = 1, SG_LOSS_HUBER = 2" in header
    assert _lib.SG_LOSS == {"mse": MSE, "mae": MAE, "huber": HUBER}
    # the entries every default call goes through are still there, with their signatures
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_fc_tail_train"][1]) == 20 and len(sig["stemgnn_fc_tail_train_rows"][1]) == 14
    assert len(sig["stemgnn_fc_tail_train_finish"][1]) == 12
    assert len(sig["stemgnn_fc_tail_train_loss"][1]) == 23 and len(sig["stemgnn_fc_tail_train_rows_loss"][1]) == 17
    assert len(sig["stemgnn_fc_tail_train_finish_loss"][1]) == 13
    assert len(sig["stemgnn_window_gather_pair"][1]) == len(sig["stemgnn_window_gather"][1]) + 1
    assert len(sig["stemgnn_window_gather_queue_pair"][1]) == len(sig["stemgnn_window_gather_queue"][1]) + 1
    assert sig["stemgnn_eval_metrics_masked"] == sig["stemgnn_eval_metrics"]


def test_target_valid_count_rejects_bad_arguments(lib):
    f = lib.stemgnn_target_valid_count
    assert f(None, 10, P, None) == SG_EINVAL
    assert f(P, 10, None, None) == SG_EINVAL
    assert f(P, 0, P, None) == SG_EINVAL


BAD_DELTAS = (0.0, -1.0, float("nan"), float("inf"))      # "finite and > 0": 0, -1, NaN as the issue lists, and +inf


def test_train_loss_rejects_bad_arguments(lib):
    ok = dict(fsum=P, target=P, w0=P, b0=P, w2=P, b2=P, B=2, N=7, W=5, H=2, kind=HUBER, param=0.5, norm=P, scratch=P,
              forecast=None, loss=P, accum=None, dfsum=P, dw0=P, db0=P, dw2=P, db2=P)
    f = lib.stemgnn_fc_tail_train_loss
    for k in ("fsum", "target", "w0", "b0", "w2", "b2", "scratch", "loss", "dfsum", "dw0", "db0", "dw2", "db2"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "kind": 3}.values(), None) == SG_EINVAL
    assert f(*{**ok, "kind": -1}.values(), None) == SG_EINVAL
    for d in BAD_DELTAS:
        assert f(*{**ok, "param": d}.values(), None) == SG_EINVAL, d
    for k, v in (("B", 0), ("N", 0), ("W", 0), ("H", 0), ("W", 65), ("H", 33)):       # the existing shape checks
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)


def test_rows_loss_rejects_bad_arguments(lib):
    ok = dict(fsum=P, target=P, w0=P, b0=P, w2=P, b2=P, B=2, N=7, W=5, H=2, kind=MAE, param=0.0, norm=None, scratch=P,
              forecast=None, dfsum=P)
    f = lib.stemgnn_fc_tail_train_rows_loss
    for k in ("fsum", "target", "w0", "b0", "w2", "b2", "scratch", "dfsum"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "kind": 3}.values(), None) == SG_EINVAL
    for d in BAD_DELTAS:
        assert f(*{**ok, "kind": HUBER, "param": d}.values(), None) == SG_EINVAL, d
    for k, v in (("B", 0), ("N", 0), ("W", 65), ("H", 33)):
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)


def test_finish_loss_rejects_bad_arguments(lib):
    ok = dict(scratch=P, B=2, N=7, W=5, H=2, norm=P, loss=P, accum=None, dw0=P, db0=P, dw2=P, db2=P)
    f = lib.stemgnn_fc_tail_train_finish_loss
    for k in ("scratch", "loss", "dw0", "db0", "dw2", "db2"):                         # `scratch`: finish without scratch
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k, v in (("B", 0), ("N", 0), ("W", 65), ("H", 33)):
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)


def test_pair_gathers_reject_bad_arguments(lib):
    ok = dict(sx=P, sy=P, hi=P, x=P, y=P, B=4, W=12, H=3, N=8, T=100, status=None)
    f = lib.stemgnn_window_gather_pair
    for k in ("sx", "sy", "hi", "x", "y"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "T": 14}.values(), None) == SG_EINVAL                             # shorter than one window
    assert f(*{**ok, "sy": P + 4}.values(), None) == SG_EINVAL                         # the alignment check covers both series
    assert f(*{**ok, "sx": P + 4}.values(), None) == SG_EINVAL
    okq = dict(sx=P, sy=P, order=P, queue=P, x=P, y=P, B=4, W=12, H=3, N=8, T=100, status=None)
    g = lib.stemgnn_window_gather_queue_pair
    for k in ("sx", "sy", "order", "queue", "x", "y"):
        assert g(*{**okq, k: None}.values(), None) == SG_EINVAL, k
    assert g(*{**okq, "sy": P + 8}.values(), None) == SG_EINVAL
    assert g(*{**okq, "B": 0}.values(), None) == SG_EINVAL


def test_masked_metrics_reject_bad_arguments_and_size_their_scratch(lib):
    ok = dict(target=P, forecast=P, mul=None, add=None, count=70, H=3, N=11, scratch=P, out=P)
    f = lib.stemgnn_eval_metrics_masked
    for k in ("target", "forecast", "scratch", "out"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "mul": P}.values(), None) == SG_EINVAL                            # mul without add
    assert f(*{**ok, "count": 0}.values(), None) == SG_EINVAL
    size, plain = lib.stemgnn_eval_scratch_doubles_masked, lib.stemgnn_eval_scratch_doubles
    for shape in ((1, 1, 1), (70, 3, 11), (64, 3, 228), (65, 12, 7), (1000, 3, 228)):
        assert size(*shape) >= plain(*shape) > 0, shape
    for shape in ((0, 3, 11), (70, 0, 11), (70, 3, 0), (-1, 3, 11)):
        assert size(*shape) == 0, shape


def test_python_layers_expose_the_options_with_their_defaults():
    from stemgnn_amd import Model, engine, forecast_dataloader, math_utils, ops, trainer
    sig = inspect.signature(Model.loss).parameters
    assert sig["kind"].default == "mse" and sig["huber_delta"].default == 1.0 and sig["ignore_nan"].default is False
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("kind", "huber_delta", "ignore_nan"))
    sig = inspect.signature(engine.TrainStep.__init__).parameters
    assert sig["loss"].default == "mse" and sig["huber_delta"].default == 1.0 and sig["ignore_nan"].default is False
    assert sig["target_series"].default is None
    assert inspect.signature(engine.ForecastStep.__init__).parameters["target_series"].default is None
    sig = inspect.signature(trainer.DeviceTrainer.__init__).parameters
    assert sig["loss"].default == "mse" and sig["huber_delta"].default == 1.0 and sig["missing"].default is None
    assert inspect.signature(trainer.column_statistics).parameters["missing"].default is None
    assert inspect.signature(trainer.score_forecast).parameters["ignore_nan"].default is False
    assert inspect.signature(forecast_dataloader.ForecastDataset.__init__).parameters["missing"].default is None
    assert inspect.signature(math_utils.Scores.__init__).parameters["ignore_nan"].default is False
    assert inspect.signature(math_utils.evaluate).parameters["ignore_nan"].default is False
    for fn in (ops.window_gather, ops.window_gather_queue):
        assert inspect.signature(fn).parameters["target_series"].default is None
    # appended behind the existing arguments: positional calls of FcTailMse keep their meaning
    names = list(inspect.signature(ops.FcTailMse.forward).parameters)
    assert names == ["ctx", "fsum", "target", "w0", "b0", "w2", "b2", "state", "loss_out", "accum", "unit_grad", "kind", "param",
                     "ignore_nan"]
    sig = inspect.signature(ops.FcTailMse.forward).parameters
    assert sig["kind"].default == "mse" and sig["param"].default == 0.0 and sig["ignore_nan"].default is False
    assert callable(ops.target_valid_count)


def test_unknown_loss_kind_raises_value_error():
    import torch

    from stemgnn_amd import Model
    m = Model(6, 2, 4, 2, horizon=2)
    with pytest.raises(ValueError, match="quantile"):
        m.loss(torch.zeros(2, 4, 6), torch.zeros(2, 2, 6), kind="quantile")


def test_mark_missing_host_logic():
    """The marking ForecastDataset(missing=...) applies ahead of `_fill_na`, on a 6 x 3 array with NaN and 0 entries."""
    from stemgnn_amd.forecast_dataloader import _fill_na, mark_missing
    nan = np.nan
    raw = np.array([[1.0, 0.0, 3.0],
                    [nan, 2.0, 0.0],
                    [0.0, 2.5, 3.5],
                    [4.0, nan, 0.0],
                    [4.5, 0.0, nan],
                    [5.0, 3.0, 4.0]])
    keep = raw.copy()
    same, mask = mark_missing(raw, None)                       # missing=None: the identity, no mask
    assert mask is None and same.dtype == np.float64 and same is not raw
    np.testing.assert_array_equal(same, keep)
    assert np.array_equal(_fill_na(same), _fill_na(keep), equal_nan=True)
    marked, mask = mark_missing(raw, 0.0)
    np.testing.assert_array_equal(raw, keep)                   # the caller's array is left alone
    expect = np.array([[0, 1, 0], [1, 0, 1], [1, 0, 0], [0, 1, 1], [0, 1, 1], [0, 0, 0]], dtype=bool)
    np.testing.assert_array_equal(mask, expect)
    assert np.isnan(marked[expect]).all()
    np.testing.assert_array_equal(marked[~expect], keep[~expect])
    filled = _fill_na(marked)                                   # ffill, then bfill for a leading gap -- zeros imputed too
    np.testing.assert_array_equal(filled, np.array([[1.0, 2.0, 3.0],
                                                    [1.0, 2.0, 3.0],
                                                    [1.0, 2.5, 3.5],
                                                    [4.0, 2.5, 3.5],
                                                    [4.5, 2.5, 3.5],
                                                    [5.0, 3.0, 4.0]]))
    marked2, mask2 = mark_missing(raw, -1.0)                   # another marker: only the raw NaN entries
    np.testing.assert_array_equal(mask2, np.isnan(keep))
    one_d, m1 = mark_missing(np.array([0.0, 1.0, nan]), 0.0)   # a single series becomes one column, as in `_fill_na`
    assert one_d.shape == (3, 1) and m1[:, 0].tolist() == [True, False, True]
