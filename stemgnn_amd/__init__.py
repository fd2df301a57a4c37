"""stemgnn_amd -- MI355X-native (gfx950) implementation of StemGNN's spectral hot path.

The product path is hand-written HIP behind a C ABI (``include/stemgnn_hip.h`` ->
``stemgnn_amd/libstemgnn_hip.so``); this package is the host-side mirror of the reference's
``models.base_model`` interface (``Model``, ``StockBlockLayer``, ``GLU``).  There is no CPU
fallback: calling the model without the HIP library or on a non-GPU tensor raises.
"""
from .base_model import GLU, Model, StockBlockLayer  # noqa: F401
from .graph import LatentGraph  # noqa: F401

from .math_utils import (EnvelopeCalibrator, EventScores, EventSpec, PathEnvelope, ScenarioEvents,  # noqa: F401
                         ScenarioSet, ScenarioTree, group_weights, joint_coverage, reduce_scenarios, scenario_tree,
                         simultaneous_bands)

__all__ = ["Model", "StockBlockLayer", "GLU", "LatentGraph", "LiveForecaster", "EventSpec", "ScenarioEvents", "EventScores",
           "group_weights", "ScenarioSet", "reduce_scenarios", "ScenarioTree", "scenario_tree", "PathEnvelope",
           "EnvelopeCalibrator", "simultaneous_bands", "joint_coverage"]
__version__ = "0.1.0"


def __getattr__(name):
    # engine pulls in torch.distributed: loaded when the serving class is first asked for, not with the package
    if name == "LiveForecaster":
        from .engine import LiveForecaster
        return LiveForecaster
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
