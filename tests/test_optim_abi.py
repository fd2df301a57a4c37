"""CPU: the optimizer-control entries of include/stemgnn_hip.h (csrc/optim.hip) are exported, size their partial sums from n
alone, and refuse bad arguments before any launch; the Python optimizers refuse negative controls.  Nothing is launched."""
import os

import pytest
import torch

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
NEW = ("stemgnn_grad_norm_partials", "stemgnn_grad_sqsum", "stemgnn_rmsprop_step_ext", "stemgnn_adam_step_ext")


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
    # the entries the optimizers call with every control at its default are still there, with their signatures
    assert len(_lib.SIGNATURES["stemgnn_rmsprop_step"][1]) == 10 and len(_lib.SIGNATURES["stemgnn_adam_step"][1]) == 13


def test_partials_count_depends_on_n_alone_and_is_monotone(lib):
    f = lib.stemgnn_grad_norm_partials
    assert f(0) >= 1 and f(1) == 1
    sizes = [1, 2, 3, 4, 5, 255, 1023, 1024, 1025, 4096, 8191, 8192, 8193, 100000, 1 << 20, 2048 * 1024 + 5, 1 << 31, (1 << 33) + 7]
    counts = [f(n) for n in sizes]
    assert all(c >= 1 for c in counts)
    assert counts == sorted(counts)
    assert counts == [f(n) for n in sizes]                      # a pure function of n
    # one partial per fixed chunk: the last n with one partial, the first with two, and the count grows by one per chunk
    c = 1
    while f(c + 1) == 1:
        c += 1
    assert f(c) == 1 and f(c + 1) == 2 and f(2 * c) == 2 and f(2 * c + 1) == 3 and f(2 * c + 3) == 3
    assert f(1 << 40) == ((1 << 40) + c - 1) // c


def test_grad_sqsum_rejects_bad_arguments(lib):
    ok = dict(grads=P, n=100, scale=1.0, partials=P)
    assert lib.stemgnn_grad_sqsum(*{**ok, "grads": None}.values(), None) == SG_EINVAL
    assert lib.stemgnn_grad_sqsum(*{**ok, "partials": None}.values(), None) == SG_EINVAL
    assert lib.stemgnn_grad_sqsum(*{**ok, "n": 0}.values(), None) == SG_EINVAL
    for mis in (P + 4, P + 8, P + 1):
        assert lib.stemgnn_grad_sqsum(*{**ok, "grads": mis}.values(), None) == SG_EINVAL, mis
    assert lib.stemgnn_grad_sqsum(*{**ok, "partials": P + 4}.values(), None) == SG_EINVAL


def test_rmsprop_step_ext_rejects_bad_arguments(lib):
    ok = dict(params=P, grads=P, sq=P, n=100, lr=P, alpha=0.99, eps=1e-8, zero=1, scale=1.0, wd=0.01, max_norm=1.0, skip=1,
              partials=P, stats=P)
    f = lib.stemgnn_rmsprop_step_ext
    for k in ("params", "grads", "sq", "lr", "stats", "partials"):      # partials: required by max_norm > 0 / skip
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "partials": None, "max_norm": 0.0}.values(), None) == SG_EINVAL       # skip still needs the norm
    assert f(*{**ok, "partials": None, "skip": 0}.values(), None) == SG_EINVAL             # clipping needs the norm
    assert f(*{**ok, "n": 0}.values(), None) == SG_EINVAL
    for k in ("params", "grads", "sq"):
        assert f(*{**ok, k: P + 4}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "wd": -0.01}.values(), None) == SG_EINVAL


def test_adam_step_ext_rejects_bad_arguments(lib):
    ok = dict(params=P, grads=P, m=P, v=P, n=100, lr=P, step=P, b1=0.9, b2=0.999, eps=1e-8, zero=1, scale=1.0, wd=0.01,
              decoupled=1, max_norm=1.0, skip=1, partials=P, stats=P)
    f = lib.stemgnn_adam_step_ext
    for k in ("params", "grads", "m", "v", "lr", "step", "stats", "partials"):
        assert f(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "partials": None, "max_norm": -1.0}.values(), None) == SG_EINVAL
    assert f(*{**ok, "partials": None, "skip": 0}.values(), None) == SG_EINVAL
    assert f(*{**ok, "n": 0}.values(), None) == SG_EINVAL
    for k in ("params", "grads", "m", "v"):
        assert f(*{**ok, k: P + 8}.values(), None) == SG_EINVAL, k
    assert f(*{**ok, "wd": -1.0}.values(), None) == SG_EINVAL


@pytest.mark.parametrize("cls", ["FusedRMSprop", "FusedAdam"])
def test_optimizers_reject_negative_controls(cls):
    from stemgnn_amd import optim
    make = getattr(optim, cls)
    params = [torch.nn.Parameter(torch.zeros(8))]
    with pytest.raises(ValueError, match="weight_decay"):
        make(params, weight_decay=-1e-2)
    with pytest.raises(ValueError, match="max_grad_norm"):
        make(params, max_grad_norm=-1.0)
    with pytest.raises(ValueError, match="max_grad_norm"):
        make(params, max_grad_norm=0.0)                       # "clip everything away": None is the way to say no clipping


def test_device_trainer_and_train_adapter_take_the_controls():
    import inspect

    from stemgnn_amd import optim, trainer
    sig = inspect.signature(trainer.DeviceTrainer.__init__).parameters
    assert sig["weight_decay"].default == 0.0 and sig["max_grad_norm"].default is None and sig["skip_nonfinite"].default is False
    for cls, extra in ((optim.FusedRMSprop, ()), (optim.FusedAdam, ("decoupled_weight_decay",))):
        sig = inspect.signature(cls.__init__).parameters
        assert sig["weight_decay"].default == 0.0 and sig["max_grad_norm"].default is None
        assert sig["skip_nonfinite"].default is False
        for name in extra:
            assert sig[name].default is False
