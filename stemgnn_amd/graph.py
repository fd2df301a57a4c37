"""Frozen and user-supplied graphs: the model run from a given adjacency, without the GRU + attention front.

The reference recomputes its latent-correlation graph from every batch (models/base_model.py:137-148): the attention is
the mean over the batch (:140), so a forecast depends on the other windows of its batch, and the GRU behind it is most of
the step.  A :class:`LatentGraph` holds the point of that computation behind the batch mean -- the un-symmetrised
adjacency ``A`` and its degrees -- and everything from there on (symmetrisation, normalised Laplacian, Chebyshev basis; the
eigen route under STEMGNN_SPECTRAL=eig) is built by the kernels the model's own front launches.

Three sources:
    ``Model.latent_graph(x)``            the graph the model computes for the batch x in eval mode
    ``Model.average_graph(batches)``     its batch-size-weighted mean over a data set (fp64 sums on the device)
    ``LatentGraph.from_adjacency(A)``    a prior graph, e.g. a road-distance adjacency

and one consumer keyword, ``adjacency=``, on Model.forward / loss / predict, engine.TrainStep / ForecastStep and
trainer.rolling_forecast / rolling_forecast_graph.
"""
import torch

from . import _lib, ops


class LatentGraph:
    """``A`` [N,N] fp32 (un-symmetrised adjacency, what the reference has after models/base_model.py:140) and ``degree`` [N] on
    the device, plus the lazily built ``mul_L`` [4,N,N] and symmetrised ``attention`` [N,N], cached per spectral route
    (STEMGNN_SPECTRAL) and dropped when ``A`` or ``degree`` is replaced.  A frozen object: nothing here is differentiable
    (hand Model.forward a raw [N,N] tensor with ``requires_grad`` for a learnable adjacency).

    The degree is STORED, not recomputed from A: the fused front sums it in another order than a row sum of A would, and
    ``model.predict(x, adjacency=model.latent_graph(x))`` returns the bits of ``model.predict(x)``."""

    def __init__(self, A, degree):
        self._cache = {}
        self._set(A, degree)

    def _set(self, A, degree):
        A, degree = A.detach(), degree.detach()
        if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] == 0:
            raise ValueError(f"adjacency must be a square [N,N] matrix, got {tuple(A.shape)}")
        if degree.shape != (A.shape[0],):
            raise ValueError(f"degree must be [{A.shape[0]}], got {tuple(degree.shape)}")
        if A.dtype != torch.float32 or degree.dtype != torch.float32:
            raise ValueError("adjacency and degree must be float32")
        if degree.device != A.device:
            raise ValueError("adjacency and degree must be on one device")
        self._A, self._degree = A.contiguous(), degree.contiguous()
        self._cache.clear()

    @property
    def A(self):
        return self._A

    @A.setter
    def A(self, value):
        self._set(value, self._degree)

    @property
    def degree(self):
        return self._degree

    @degree.setter
    def degree(self, value):
        self._set(self._A, value)

    @property
    def N(self):
        return self._A.shape[0]

    @property
    def device(self):
        return self._A.device

    def to(self, device):
        """A LatentGraph on `device` (this one if it is there already)."""
        device = torch.device(device)
        if device == self.device or (device.type == self.device.type and device.index is None):
            return self
        return LatentGraph(self._A.to(device), self._degree.to(device))

    def basis(self):
        """(attention [N,N], mul_L [4,N,N]) for the current spectral route, built once (ops.graph_basis)."""
        route = ops.spectral_route()
        hit = self._cache.get(route)
        if hit is None:
            with torch.no_grad():
                hit = self._cache[route] = ops.graph_basis(self._A, self._degree)
        return hit

    @property
    def attention(self):
        return self.basis()[0]

    @property
    def mul_L(self):
        return self.basis()[1]

    @classmethod
    def from_adjacency(cls, A, degree=None, device=None):
        """A prior graph.  A: square, non-negative, finite, float32 or convertible to it (anything torch.as_tensor takes);
        degree None: deg_i = sum_j A[i][j], taken BEFORE the symmetrisation as the reference does (:141-143), by the device
        kernel ``stemgnn_graph_degree``.  Validated once on the host (one sync here, none later): ValueError for a non-square
        input, a dtype that is not real-valued, a non-finite or negative entry, or a row sum / degree that is not positive --
        a zero degree would put 1 / 1e-7 into the Laplacian, silently, as it would in the reference.
        device: where the graph lives (default: A's own device when it is on a HIP device, else the current one)."""
        try:
            A = torch.as_tensor(A)
        except Exception as e:  # noqa: BLE001
            raise ValueError(f"adjacency is not convertible to a tensor: {e}") from None
        if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] == 0:
            raise ValueError(f"adjacency must be a square [N,N] matrix, got {tuple(A.shape)}")
        if A.dtype == torch.bool or A.is_complex():
            raise ValueError(f"adjacency must be float32 or convertible to float32, got {A.dtype}")
        A = A.detach().to(torch.float32)
        if not bool(torch.isfinite(A).all()):
            raise ValueError("adjacency has a non-finite entry")
        if bool((A < 0).any()):
            raise ValueError("adjacency has a negative entry")
        # the row sums on the host side of the check are fp64 (is the degree positive at all); the degree the graph carries
        # comes from the device kernel
        if degree is None and not bool((A.double().sum(dim=1) > 0).all()):
            raise ValueError("adjacency has a row whose sum is not positive (an isolated node has no normalised Laplacian)")
        if degree is not None:
            degree = torch.as_tensor(degree).detach().to(torch.float32).reshape(-1)
            if degree.shape != (A.shape[0],):
                raise ValueError(f"degree must have {A.shape[0]} entries, got {tuple(degree.shape)}")
            if not bool(torch.isfinite(degree).all()) or not bool((degree > 0).all()):
                raise ValueError("degree must be finite and positive")
        if device is None:
            if not A.is_cuda and not torch.cuda.is_available():
                raise _lib.StemGNNHipError(
                    f"adjacency is on {A.device}: stemgnn_amd runs only on a HIP device (no CPU fallback)")
            device = A.device if A.is_cuda else torch.device("cuda", torch.cuda.current_device())
        A = A.to(device).contiguous()
        if degree is None:
            with torch.no_grad():
                degree = ops.graph_degree(A)
            if not bool((degree > 0).all()):
                raise ValueError("adjacency has a row whose sum is not positive")
        return cls(A, degree.to(device))


def prepare(adjacency, device):
    """What a step driver keeps of its ``adjacency=`` argument: a LatentGraph on `device` with its basis built (nothing of it
    is left for the captured step), a tensor as it is, None as None."""
    if isinstance(adjacency, LatentGraph):
        adjacency = adjacency.to(device)
        adjacency.basis()
    return adjacency


def resolve_basis(adjacency, device):
    """(attention, mul_L) of what a caller passed as ``adjacency=``: a LatentGraph (cached, constant) or a raw [N,N] float32
    tensor on the device (= from_adjacency without the host validation; differentiable through ops.GraphBasisFn when it
    requires a gradient)."""
    if isinstance(adjacency, LatentGraph):
        return adjacency.to(device).basis()
    if not torch.is_tensor(adjacency):
        raise TypeError(f"adjacency must be a LatentGraph or an [N,N] tensor, got {type(adjacency).__name__}")
    if adjacency.dim() != 2 or adjacency.shape[0] != adjacency.shape[1]:
        raise ValueError(f"adjacency must be a square [N,N] matrix, got {tuple(adjacency.shape)}")
    return ops.GraphBasisFn.apply(adjacency, None)
