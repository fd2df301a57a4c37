"""CPU: the C entries and the Python surface of the frozen / user-supplied graph path (``adjacency=``).  Nothing is launched:
every call here is refused before it reaches the device."""
import inspect
import os
import re
from ctypes import c_double, c_int, c_size_t, c_void_p

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stemgnn_hip.h")
EINVAL = -10001
_C = {"int": c_int, "size_t": c_size_t, "double": c_double}
ENTRIES = ["stemgnn_graph_degree", "stemgnn_graph_basis_fwd", "stemgnn_graph_basis_bwd", "stemgnn_graph_accumulate",
           "stemgnn_graph_finish"]


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def header_signature(name):
    """(restype, argtypes) of `name` as include/stemgnn_hip.h declares it: pointers -> c_void_p, scalars by their C type."""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, f"{name} is not declared in include/stemgnn_hip.h"
    args = []
    for a in m.group(2).split(","):
        a = a.strip()
        args.append(c_void_p if "*" in a else _C[a.split()[-2]])
    return _C[m.group(1)], args


@pytest.mark.parametrize("name", ENTRIES)
def test_symbol_has_the_headers_signature(lib, name):
    from stemgnn_amd import _lib

    assert hasattr(lib, name)
    assert _lib.SIGNATURES[name] == header_signature(name)


def test_einval_for_null_and_empty(lib):
    p = 4096                                             # a non-NULL pointer value; nothing dereferences it: every call is refused
    assert lib.stemgnn_graph_degree(None, 8, p, None) == EINVAL
    assert lib.stemgnn_graph_degree(p, 8, None, None) == EINVAL
    for n in (0, -3):
        assert lib.stemgnn_graph_degree(p, n, p, None) == EINVAL
        assert lib.stemgnn_graph_basis_fwd(p, p, p, p, n, None) == EINVAL
        assert lib.stemgnn_graph_basis_bwd(p, p, p, p, p, n, None) == EINVAL
    for hole in range(4):
        args = [p, p, p, p]
        args[hole] = None
        assert lib.stemgnn_graph_basis_fwd(*args, 8, None) == EINVAL
    assert lib.stemgnn_graph_basis_bwd(None, None, p, p, p, 8, None) == EINVAL      # neither gradient
    for hole in (2, 3, 4):
        args = [p, p, p, p, p]
        args[hole] = None
        assert lib.stemgnn_graph_basis_bwd(*args, 8, None) == EINVAL
    assert lib.stemgnn_graph_accumulate(None, 1.0, p, 8, 1, None) == EINVAL
    assert lib.stemgnn_graph_accumulate(p, 1.0, None, 8, 1, None) == EINVAL
    assert lib.stemgnn_graph_accumulate(p, 1.0, p, 0, 1, None) == EINVAL
    assert lib.stemgnn_graph_accumulate(p, 0.0, p, 8, 1, None) == EINVAL
    assert lib.stemgnn_graph_finish(None, 1.0, p, 8, None) == EINVAL
    assert lib.stemgnn_graph_finish(p, 1.0, None, 8, None) == EINVAL
    assert lib.stemgnn_graph_finish(p, 1.0, p, 0, None) == EINVAL
    assert lib.stemgnn_graph_finish(p, 0.0, p, 8, None) == EINVAL


def test_from_adjacency_validates_on_the_host():
    from stemgnn_amd import LatentGraph

    ok = torch.rand(6, 6) + 0.1
    bad = {
        "square": torch.rand(6, 5),
        "square ": torch.rand(6),
        "float32": torch.rand(6, 6) > 0.5,
        "float32 ": torch.complex(ok, ok),
        "tensor": [[1.0, "x"], [0.0, 1.0]],
        "non-finite": ok.clone().index_put_((torch.tensor(2), torch.tensor(3)), torch.tensor(float("nan"))),
        "non-finite ": ok.clone().index_put_((torch.tensor(0), torch.tensor(0)), torch.tensor(float("inf"))),
        "negative": ok.clone().index_put_((torch.tensor(1), torch.tensor(4)), torch.tensor(-1e-3)),
        "not positive": ok.clone().index_put_((torch.tensor(3),), torch.zeros(6)),
    }
    for what, A in bad.items():
        with pytest.raises(ValueError, match=what.strip()):
            LatentGraph.from_adjacency(A)
    with pytest.raises(ValueError, match="degree"):
        LatentGraph.from_adjacency(ok, degree=torch.ones(5))
    with pytest.raises(ValueError, match="degree"):
        LatentGraph.from_adjacency(ok, degree=torch.tensor([1.0, 1.0, 0.0, 1.0, 1.0, 1.0]))
    # float64 / integer input converts; it is the device that a CPU-only process then lacks
    if not torch.cuda.is_available():
        from stemgnn_amd._lib import StemGNNHipError
        for A in (ok.double(), torch.ones(4, 4, dtype=torch.int64)):
            with pytest.raises(StemGNNHipError, match="no CPU fallback"):
                LatentGraph.from_adjacency(A)


def test_latent_graph_refuses_mismatched_parts():
    from stemgnn_amd import LatentGraph

    with pytest.raises(ValueError):
        LatentGraph(torch.rand(4, 3), torch.rand(4))
    with pytest.raises(ValueError):
        LatentGraph(torch.rand(4, 4), torch.rand(3))
    with pytest.raises(ValueError):
        LatentGraph(torch.rand(4, 4).double(), torch.rand(4))


def test_model_accepts_adjacency_keyword_and_still_refuses_the_cpu():
    from stemgnn_amd import LatentGraph, Model, engine, ops, trainer
    from stemgnn_amd._lib import StemGNNHipError

    m = Model(6, 2, 4, 2, horizon=2)
    x, y = torch.randn(2, 4, 6), torch.randn(2, 2, 6)
    for call in (lambda: m(x, adjacency=None), lambda: m.loss(x, y, adjacency=None), lambda: m.predict(x, adjacency=None),
                 lambda: m(x, adjacency=torch.rand(6, 6)), lambda: m.loss(x, y, adjacency=torch.rand(6, 6)),
                 lambda: m.predict(x, adjacency=torch.rand(6, 6)), lambda: m.latent_graph(x), lambda: m.average_graph([x])):
        with pytest.raises(StemGNNHipError, match="no CPU fallback"):
            call()
    for fn in (Model.forward, Model.loss, Model.predict, ops.forecast_forward, engine.TrainStep.__init__,
               engine.ForecastStep.__init__, trainer.rolling_forecast, trainer.rolling_forecast_graph):
        assert inspect.signature(fn).parameters["adjacency"].default is None, fn
    assert LatentGraph is __import__("stemgnn_amd.graph", fromlist=["LatentGraph"]).LatentGraph
