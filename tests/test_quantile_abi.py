"""CPU: the quantile entries of include/stemgnn_hip.h (csrc/tail.hip, csrc/data.hip) are exported and declared and refuse bad
arguments before any launch; the quantile head of Model leaves every other parameter alone; the pins of the existing ABI
(tests/test_loss_abi.py) still hold.  Nothing is launched."""
import inspect
import os

import pytest
import torch

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NEW = ("stemgnn_fc_tail_train_quantile", "stemgnn_fc_tail_train_rows_quantile", "stemgnn_fc_tail_train_finish_quantile",
       "stemgnn_roll_window_quantile", "stemgnn_quantile_metrics", "stemgnn_quantile_metrics_masked",
       "stemgnn_quantile_scratch_doubles", "stemgnn_quantile_out_doubles")
NAN = float("nan")


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def taus(*v):
    from stemgnn_amd import _lib
    return _lib.host_floats(v)


def taus64(*v):
    from stemgnn_amd import _lib
    return _lib.host_floats(v, _lib.c_double)


def test_new_symbols_exported_and_declared_and_the_old_pins_hold(lib):
    from stemgnn_amd import _lib, ops
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_fc_tail_train_quantile"][1]) == 23 and len(sig["stemgnn_fc_tail_train_rows_quantile"][1]) == 17
    assert len(sig["stemgnn_fc_tail_train_finish_quantile"][1]) == 14
    assert sig["stemgnn_quantile_metrics_masked"] == sig["stemgnn_quantile_metrics"]
    # the pins of tests/test_loss_abi.py, re-asserted: the enum grew at its end, SG_LOSS and FcTailMse did not change
    assert "SG_LOSS_MSE = 0, SG_LOSS_MAE = 1, SG_LOSS_HUBER = 2" in header
    assert "SG_LOSS_HUBER = 2, SG_LOSS_PINBALL = 3 }" in header
    assert _lib.SG_LOSS == {"mse": 0, "mae": 1, "huber": 2}
    assert _lib.SG_LOSS_PINBALL == 3
    names = list(inspect.signature(ops.FcTailMse.forward).parameters)
    assert names == ["ctx", "fsum", "target", "w0", "b0", "w2", "b2", "state", "loss_out", "accum", "unit_grad", "kind", "param",
                     "ignore_nan"]
    names = list(inspect.signature(ops.FcTailQuantile.forward).parameters)
    assert names == ["ctx", "fsum", "target", "w0", "b0", "w2", "b2", "state", "loss_out", "accum", "unit_grad", "taus",
                     "ignore_nan"]


def test_loss_entries_keep_rejecting_kind_3(lib):
    ok = dict(fsum=P, target=P, w0=P, b0=P, w2=P, b2=P, B=2, N=7, W=5, H=2, kind=3, param=0.5, norm=None, scratch=P,
              forecast=None, loss=P, accum=None, dfsum=P, dw0=P, db0=P, dw2=P, db2=P)
    assert lib.stemgnn_fc_tail_train_loss(*ok.values(), None) == SG_EINVAL
    rows = dict(fsum=P, target=P, w0=P, b0=P, w2=P, b2=P, B=2, N=7, W=5, H=2, kind=3, param=0.0, norm=None, scratch=P,
                forecast=None, dfsum=P)
    assert lib.stemgnn_fc_tail_train_rows_loss(*rows.values(), None) == SG_EINVAL
    # the fc tail's range
    assert lib.stemgnn_fc_tail_supported(64, 32) == 1
    assert lib.stemgnn_fc_tail_supported(65, 3) == 0 and lib.stemgnn_fc_tail_supported(12, 33) == 0


BAD_TAUS = [(0.0, 0.5, 0.9), (0.1, 1.0, 0.9), (0.1, 0.5, NAN), (-0.5, 0.5, 0.9), (0.1, 0.5, 1.5)]
BAD_SHAPES = (("B", 0), ("N", 0), ("W", 0), ("H", 0), ("Q", 0), ("B", -1), ("Q", -3), ("W", 65))


def test_train_quantile_rejects_bad_arguments(lib):
    ok = dict(fsum=P, target=P, w0=P, b0=P, w2=P, b2=P, B=2, N=7, W=5, H=2, Q=3, taus=taus(0.1, 0.5, 0.9), norm=P, scratch=P,
              forecast=None, loss=P, accum=None, dfsum=P, dw0=P, db0=P, dw2=P, db2=P)
    f = lib.stemgnn_fc_tail_train_quantile
    for k in ("fsum", "target", "w0", "b0", "w2", "b2", "taus", "scratch", "loss", "dfsum", "dw0", "db0", "dw2", "db2"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k, v in BAD_SHAPES:
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)
    eleven = taus(*[(i + 1) / 12 for i in range(11)])
    assert f(*{**ok, "H": 3, "Q": 11, "taus": eleven}.values(), None) == SG_EINVAL          # Q * H = 33
    assert f(*{**ok, "H": 33, "Q": 1, "taus": taus(0.5)}.values(), None) == SG_EINVAL
    for bad in BAD_TAUS:
        assert f(*{**ok, "taus": taus(*bad)}.values(), None) == SG_EINVAL, bad


def test_rows_quantile_rejects_bad_arguments(lib):
    ok = dict(fsum=P, target=P, w0=P, b0=P, w2=P, b2=P, B=2, N=7, W=5, H=2, Q=3, taus=taus(0.1, 0.5, 0.9), norm=None,
              scratch=P, forecast=None, dfsum=P)
    f = lib.stemgnn_fc_tail_train_rows_quantile
    for k in ("fsum", "target", "w0", "b0", "w2", "b2", "taus", "scratch", "dfsum"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k, v in BAD_SHAPES:
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)
    eleven = taus(*[(i + 1) / 12 for i in range(11)])
    assert f(*{**ok, "H": 3, "Q": 11, "taus": eleven}.values(), None) == SG_EINVAL
    for bad in BAD_TAUS:
        assert f(*{**ok, "taus": taus(*bad)}.values(), None) == SG_EINVAL, bad


def test_finish_quantile_rejects_bad_arguments(lib):
    ok = dict(scratch=P, B=2, N=7, W=5, H=2, Q=3, norm=P, loss=P, accum=None, dw0=P, db0=P, dw2=P, db2=P)
    f = lib.stemgnn_fc_tail_train_finish_quantile
    for k in ("scratch", "loss", "dw0", "db0", "dw2", "db2"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k, v in BAD_SHAPES:
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)
    assert f(*{**ok, "H": 3, "Q": 11}.values(), None) == SG_EINVAL


def test_roll_window_quantile_rejects_bad_arguments(lib):
    ok = dict(inputs=P, forecast=P, nxt=2 * P, steps=P, B=2, W=5, L=2, N=7, Q=3, point=1, step=0, horizon=5)
    f = lib.stemgnn_roll_window_quantile
    for k in ("inputs", "forecast", "nxt", "steps"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "nxt": P}.values(), None) == SG_EINVAL                            # in place
    for k, v in (("B", 0), ("W", 0), ("N", 0), ("L", 0), ("L", 6), ("step", -1), ("step", 5), ("Q", 0), ("point", -1),
                 ("point", 3)):
        assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)


def test_quantile_metrics_reject_bad_arguments_and_size_their_buffers(lib):
    ok = dict(target=P, forecast=P, taus=taus64(0.1, 0.5, 0.9), mul=None, add=None, count=70, Q=3, H=3, N=11, scratch=P, out=P)
    for f in (lib.stemgnn_quantile_metrics, lib.stemgnn_quantile_metrics_masked):
        for k in ("target", "forecast", "taus", "scratch", "out"):
            assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
        assert f(*{**ok, "mul": P}.values(), None) == SG_EINVAL                        # mul without add
        for k, v in (("count", 0), ("Q", 0), ("H", 0), ("N", 0), ("Q", 33)):
            assert f(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)
        for bad in ((0.0, 0.5, 0.9), (0.1, 1.0, 0.9), (0.1, NAN, 0.9)):
            assert f(*{**ok, "taus": taus64(*bad)}.values(), None) == SG_EINVAL, bad
    for Q, H in ((1, 1), (3, 3), (4, 2), (9, 1)):
        K = 2 * Q + 2 * (Q // 2) + 1
        assert lib.stemgnn_quantile_out_doubles(Q, H) == K * (H + 1)
        for count, N in ((1, 1), (70, 11), (65, 7)):
            chunks = (count + 63) // 64
            assert lib.stemgnn_quantile_scratch_doubles(count, Q, H, N) == (K + 1) * H * N * (chunks + 1) + (K + 1) * H
    assert lib.stemgnn_quantile_out_doubles(0, 3) == 0 and lib.stemgnn_quantile_scratch_doubles(0, 3, 3, 11) == 0


def test_quantile_head_leaves_every_other_parameter_alone():
    from stemgnn_amd import Model
    torch.manual_seed(11)
    plain = Model(6, 2, 4, 2, horizon=2)
    torch.manual_seed(11)
    none = Model(6, 2, 4, 2, horizon=2, quantiles=None)
    torch.manual_seed(11)
    quant = Model(6, 2, 4, 2, horizon=2, quantiles=(0.1, 0.5, 0.9))
    sd, sn, sq = plain.state_dict(), none.state_dict(), quant.state_dict()
    assert list(sd) == list(sn) == list(sq)
    for k in sd:
        assert torch.equal(sd[k], sn[k]), k
        if not k.startswith("fc.2."):
            assert torch.equal(sd[k], sq[k]), k
    assert tuple(quant.fc[2].weight.shape) == (6, 4) and tuple(quant.fc[2].bias.shape) == (6,)
    assert list(quant.state_dict())[-2:] == ["fc.2.weight", "fc.2.bias"]               # the last parameters created
    assert quant.horizon == 2 and quant.quantiles == (0.1, 0.5, 0.9) and isinstance(quant.quantiles, tuple)
    assert plain.quantiles is None and none.quantiles is None
    assert inspect.signature(Model.__init__).parameters["quantiles"].kind is inspect.Parameter.KEYWORD_ONLY


def test_whole_module_pickling_carries_the_quantiles(tmp_path):
    from stemgnn_amd import Model
    from stemgnn_amd.trainer import load_checkpoint, save_checkpoint
    quant = Model(6, 2, 4, 2, horizon=2, quantiles=(0.25, 0.75))
    save_checkpoint(quant, tmp_path)
    back = load_checkpoint(tmp_path)
    assert back.quantiles == (0.25, 0.75) and back.point_index == 0 and back.horizon == 2
    assert all(torch.equal(v, back.state_dict()[k]) for k, v in quant.state_dict().items())
    save_checkpoint(Model(6, 2, 4, 2, horizon=2), tmp_path, 1)
    assert load_checkpoint(tmp_path, 1).quantiles is None


def test_bad_quantile_tuples_and_the_range():
    from stemgnn_amd import Model
    from stemgnn_amd._lib import StemGNNHipError
    for bad in ((0.5, 0.1), (0.1, 0.1, 0.9), (0.0, 0.5), (0.5, 1.0), (), (0.1, NAN)):
        with pytest.raises(ValueError):
            Model(6, 2, 4, 2, horizon=2, quantiles=bad)
    with pytest.raises(StemGNNHipError, match="fc tail"):
        Model(6, 2, 4, 2, horizon=3, quantiles=tuple((i + 1) / 12 for i in range(11)))
    Model(6, 2, 4, 2, horizon=4, quantiles=tuple((i + 1) / 9 for i in range(8)))     # Q * H = 32: the limit itself


def test_point_index():
    from stemgnn_amd import Model
    for q, want in (((0.1, 0.5, 0.9), 1), ((0.25, 0.75), 0), ((0.05,), 0), ((0.1, 0.4, 0.7), 1)):
        assert Model(6, 2, 4, 2, horizon=2, quantiles=q).point_index == want, q


def test_loss_kinds_by_model_type():
    from stemgnn_amd import Model
    x, y = torch.zeros(2, 4, 6), torch.zeros(2, 2, 6)
    plain, quant = Model(6, 2, 4, 2, horizon=2), Model(6, 2, 4, 2, horizon=2, quantiles=(0.1, 0.5, 0.9))
    with pytest.raises(ValueError, match="pinball"):
        plain.loss(x, y, kind="pinball")
    for kind in ("mse", "mae", "huber"):
        with pytest.raises(ValueError, match="quantile model"):
            quant.loss(x, y, kind=kind)
    for m in (plain, quant):
        with pytest.raises(ValueError, match="quantile"):
            m.loss(x, y, kind="quantile")


def test_python_layers_expose_the_keyword_behind_defaults():
    from stemgnn_amd import engine, math_utils, ops, trainer
    assert inspect.signature(trainer.DeviceTrainer.__init__).parameters["quantiles"].default is None
    assert inspect.signature(trainer.DeviceTrainer.__init__).parameters["loss"].default == "mse"
    assert inspect.signature(trainer.score_forecast).parameters["quantiles"].default is None
    sig = inspect.signature(math_utils.QuantileScores.__init__).parameters
    assert list(sig) == ["self", "y", "y_hat", "quantiles", "mul", "add", "ignore_nan"]
    assert sig["mul"].default is None and sig["add"].default is None and sig["ignore_nan"].default is False
    assert callable(ops.roll_window_quantile) and callable(ops.quantile_metrics)
    assert inspect.signature(engine.TrainStep.__init__).parameters["loss"].default == "mse"
