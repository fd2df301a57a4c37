"""CPU: the scenario entries of include/stemgnn_hip.h (csrc/scenario.hip) are exported, declared and bound; every bad argument
is refused before any launch; the rank function is the formula; the Python layers refuse a point model.  Nothing is launched."""
import ctypes
import inspect
import os

import pytest
import torch

from tests.helpers import scenario_ref as R

SG_EINVAL = -10001
P = 64                          # a stand-in device address (16-byte aligned): every call below is refused before any use
P2 = 128
NEW = ("stemgnn_scenario_roll", "stemgnn_scenario_bands", "stemgnn_scenario_rank")
TAUS = (0.1, 0.5, 0.9)


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def floats(*v):
    return (ctypes.c_float * len(v))(*v)


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_symbols_exported_declared_and_bound(lib):
    from stemgnn_amd import _lib, engine, ops, trainer
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "stemgnn_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    sig = _lib.SIGNATURES
    assert len(sig["stemgnn_scenario_roll"][1]) == 21 and len(sig["stemgnn_scenario_bands"][1]) == 10
    assert sig["stemgnn_scenario_roll"][1][12] is ctypes.c_longlong                      # origin0
    assert sig["stemgnn_scenario_roll"][1][13] is ctypes.c_ulonglong and sig["stemgnn_scenario_roll"][1][14] is ctypes.c_ulonglong
    assert sig["stemgnn_scenario_rank"] == (ctypes.c_long, [ctypes.c_double, ctypes.c_long])
    csrc = os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc")
    makefile = open(os.path.join(csrc, "Makefile")).read()
    assert "scenario.hip" in makefile.split("SRCS =")[1].splitlines()[0]
    assert "philox.h" in makefile.split("HDRS =")[1].splitlines()[0]
    # one definition of the generator, in the header both users include
    for user in ("front.hip", "scenario.hip"):
        text = open(os.path.join(csrc, user)).read()
        assert '#include "philox.h"' in text and "void sg_philox4(" not in text, user
    assert "void sg_philox4(" in open(os.path.join(csrc, "philox.h")).read()
    assert tuple(inspect.signature(trainer.rolling_scenarios).parameters)[:9] == (
        "model", "loader", "horizon", "paths", "seed", "adjacency", "coupling", "tails", "return_paths")
    par = inspect.signature(trainer.rolling_scenarios).parameters
    assert par["paths"].default == 64 and par["seed"].default == 0 and par["adjacency"].default is None
    assert par["coupling"].default == "independent" and par["tails"].default == "linear" and par["return_paths"].default is False
    par = inspect.signature(engine.LiveForecaster.scenarios).parameters
    assert tuple(par) == ("self", "paths", "horizon", "seed", "coupling", "tails", "return_paths")
    assert par["paths"].default == 64 and par["horizon"].default is None and par["seed"].default is None
    assert callable(ops.scenario_roll) and callable(ops.scenario_bands) and callable(ops.scenario_rank)


# the arguments of the two entries, in order (the stream follows)
ROLL_OK = dict(inputs=P, forecast=P2, taus=floats(*TAUS), Bo=4, S=8, fan=8, W=12, L=3, N=11, Q=3, step=0, horizon=7, origin0=5,
               seed=1, offset=0, coupling=0, tails=0, inputs_next=3 * P, paths=4 * P, bands=5 * P)
BANDS_OK = dict(paths=P, Bo=4, S=8, horizon=7, N=11, Q=3, ranks=ints(1, 4, 8), step_from=3, bands=P2)


def refused(f, ok, **change):
    return f(*{**ok, **change}.values(), None) == SG_EINVAL


def test_roll_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_scenario_roll, ROLL_OK
    for k in ("inputs", "forecast", "taus", "paths"):
        assert refused(f, ok, **{k: None}), k
    assert refused(f, ok, inputs_next=P)                                        # the window cannot be rolled in place
    for k in ("Bo", "W", "L", "N"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, L=13)                                                 # L > W
    for v in (-1, 7, 8):
        assert refused(f, ok, step=v), v
    assert refused(f, ok, horizon=0)
    # Q < 2 or Q > 32
    for q in (1, 0, -1):
        assert refused(f, ok, Q=q, taus=floats(0.5)), q
    assert refused(f, ok, Q=33, taus=floats(*[(i + 1) / 40 for i in range(33)]))
    # levels that are not strictly increasing inside (0, 1)
    for bad in ((0.1, 0.1, 0.9), (0.5, 0.1, 0.9), (0.0, 0.5, 0.9), (0.1, 0.5, 1.0), (-0.1, 0.5, 0.9), (0.1, 0.5, 1.5),
                (0.1, float("nan"), 0.9), (float("nan"), 0.5, 0.9), (0.1, 0.5, float("nan")), (0.1, 0.9, 0.5)):
        assert refused(f, ok, taus=floats(*bad)), bad
    # S outside [1, 1024]
    for s in (0, -1, 1025):
        assert refused(f, ok, S=s, fan=s), s
        assert refused(f, ok, S=s, fan=1), s
    # fan not in {1, S}
    for fan in (0, 2, 4, 9, -1):
        assert refused(f, ok, fan=fan), fan
    assert refused(f, ok, fan=1)                                                # round-0 bands with a later round's fan
    for k in ("coupling", "tails"):
        for v in (-1, 2):
            assert refused(f, ok, **{k: v}), (k, v)
    # index products that reach 2^31 where an int carries them
    assert refused(f, ok, Bo=2 ** 21, S=1024, fan=1024)                         # Bo * S
    assert refused(f, ok, W=2 ** 16, N=2 ** 15)                                 # W * N
    assert refused(f, ok, W=2 ** 12, L=2 ** 12, N=2 ** 18)                      # Q * L * N
    assert refused(f, ok, horizon=2 ** 20, N=2 ** 10)                           # Q * horizon * N
    assert refused(f, ok, S=1024, fan=1024, horizon=2 ** 21, N=1)               # S * horizon


def test_bands_rejects_bad_arguments(lib):
    f, ok = lib.stemgnn_scenario_bands, BANDS_OK
    for k in ("paths", "ranks", "bands"):
        assert refused(f, ok, **{k: None}), k
    assert refused(f, ok, bands=P)
    for k in ("Bo", "horizon", "N", "Q"):
        for v in (0, -1):
            assert refused(f, ok, **{k: v}), (k, v)
    assert refused(f, ok, Q=33, ranks=ints(*([1] * 33)))
    for s in (0, -1, 1025):
        assert refused(f, ok, S=s), s
    for v in (-1, 8):
        assert refused(f, ok, step_from=v), v
    for bad in ((0, 4, 8), (1, 4, 9), (1, -3, 8)):
        assert refused(f, ok, ranks=ints(*bad)), bad
    assert refused(f, ok, horizon=2 ** 16, N=2 ** 15, step_from=0)             # horizon * N
    assert refused(f, ok, Bo=2 ** 21, S=1024, ranks=ints(1, 4, 8))             # Bo * S
    # step_from == horizon: nothing to write, nothing launched, no error
    assert f(*{**ok, "step_from": 7}.values(), None) == 0


def test_rank_is_the_formula(lib):
    from stemgnn_amd import ops
    for tau in (0.05, 0.1, 0.25, 0.5, 0.9, 0.95, 1 / 3):
        for S in range(1, 1025):
            k = lib.stemgnn_scenario_rank(tau, S)
            assert k == R.rank(tau, S), (tau, S, k)
            assert 1 <= k <= S
    assert ops.scenario_rank(0.5, 64) == 32 and ops.scenario_rank(0.9, 10) == 9 and ops.scenario_rank(1 / 3, 3) == 1
    assert ops.scenario_rank(0.05, 7) == 1 and ops.scenario_rank(0.95, 1) == 1


def test_python_layers_refuse_a_point_model():
    from stemgnn_amd import Model, trainer
    from stemgnn_amd._lib import StemGNNHipError
    from stemgnn_amd.engine import LiveForecaster
    plain, single = Model(6, 2, 4, 2, horizon=2), Model(6, 2, 4, 2, horizon=2, quantiles=(0.5,))
    loader = [(torch.zeros(2, 4, 6), torch.zeros(2, 5, 6))]
    for model in (plain, single):
        with pytest.raises(ValueError, match="needs a quantile model"):
            trainer.rolling_scenarios(model, loader, 5)
        with pytest.raises(ValueError, match="needs a quantile model"):
            LiveForecaster(model, 4, 5).scenarios()
        assert model.training                                                   # refused before the model is touched
    quant = Model(6, 2, 4, 2, horizon=2, quantiles=TAUS)
    for paths in (0, 1025):
        with pytest.raises(ValueError, match="paths within"):
            trainer.rolling_scenarios(quant, loader, 5, paths=paths)
        with pytest.raises(ValueError, match="paths within"):
            LiveForecaster(quant, 4, 5).scenarios(paths=paths)
    with pytest.raises(RuntimeError, match="a window needs 4"):
        LiveForecaster(quant, 4, 5).scenarios()                                 # nothing pushed yet: refused on the host
    # the ops wrappers: no CPU fallback
    with pytest.raises(StemGNNHipError):
        trainer.rolling_scenarios(quant, loader, 5)
    assert quant.training                                                       # the training state is restored on the way out
    with pytest.raises(StemGNNHipError):
        from stemgnn_amd import ops
        ops.scenario_bands(torch.zeros(1, 4, 5, 6), TAUS, 2, torch.zeros(1, 3, 5, 6))
