"""stemgnn_amd -- MI355X-native (gfx950) implementation of StemGNN's spectral hot path.

The product path is hand-written HIP behind a C ABI (``include/stemgnn_hip.h`` ->
``stemgnn_amd/libstemgnn_hip.so``); this package is the host-side mirror of the reference's
``models.base_model`` interface (``Model``, ``StockBlockLayer``, ``GLU``).  There is no CPU
fallback: calling the model without the HIP library or on a non-GPU tensor raises.
"""
from .base_model import GLU, Model, StockBlockLayer  # noqa: F401
from .graph import LatentGraph  # noqa: F401

from .math_utils import (EventScores, EventSpec, ScenarioEvents, ScenarioSet, ScenarioTree, group_weights,  # noqa: F401
                         reduce_scenarios, scenario_tree)

__all__ = ["Model", "StockBlockLayer", "GLU", "LatentGraph", "LiveForecaster", "EventSpec", "ScenarioEvents", "EventScores",
           "group_weights", "ScenarioSet", "reduce_scenarios", "ScenarioTree", "scenario_tree"]
__version__ = "0.1.0"


def __getattr__(name):
    # engine pulls in torch.distributed: loaded when the serving class is first asked for, not with the package
    if name == "LiveForecaster":
        from .engine import LiveForecaster
        return LiveForecaster
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
