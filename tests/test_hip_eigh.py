"""GPU: the direct eigensolver (csrc/eigh.hip) on prior-graph spectra and on every launch path, through the C ABI on
NaN-filled, guarded buffers, against fp64.

The solver was written for the latent Laplacian (dense, N - 1 eigenvalues in [0.99, 1.01]); ``LatentGraph.from_adjacency``
under STEMGNN_SPECTRAL=eig hands it rings, grids, stars, hypercubes, k-NN graphs, disconnected and self-loop-only graphs
(tests/helpers/eigh_cases.py; tests/test_eigh_cases.py pins their spectra on the CPU).  Buffers: mul_L slot 0 holds a
sentinel, slot 1 the matrix, slots 2 / 3, lam, U and the scratch NaN; the scratch is exactly stemgnn_eigh_scratch_floats(N)
floats; a guard band behind each.  After every call: rc 0 and a clean status word, slots 0 / 1 bit-identical to what went in,
no NaN / inf in lam, U, slots 2 / 3, all guards intact.

Bounds (fp64 metrics of tests/helpers/eigh_cases.metrics): ev, orth < 1e-5 (2e-5 where the spectrum is repeated by
construction, as test_eigh_repeated_eigenvalues_keep_an_orthonormal_basis has it), rec < 2e-5, slots 2 / 3 against the fp64
polynomials < 1e-4.  The per-vector residual `res` is bounded by 8 x the residual of the float32 LAPACK solution of the same
matrix, floor 1e-6, cap 2e-5 (eigh_cases.res_limit).

Measured on an MI355X, test_eigh_prior_graph_spectra (the LAPACK column is the host's own BLAS: it moves a little from one
machine to the next, the limit with it):

    case           device res   float32 LAPACK res   limit     device ev / orth / rec
    ring64         3.96e-07     1.08e-06             8.7e-06   1.5e-07 / 1.8e-07 / 4.2e-07
    ring257        8.97e-07     1.35e-06             1.1e-05   7.5e-07 / 2.7e-07 / 4.3e-07
    path65         6.49e-08     5.40e-07             4.3e-06   5.5e-08 / 3.3e-08 / 2.6e-08
    star96         8.34e-07     5.93e-06             2.0e-05   8.3e-07 / 8.9e-07 / 9.2e-07
    bipartite      8.34e-07     4.83e-06             2.0e-05   8.3e-07 / 8.9e-07 / 9.0e-07
    hypercube64    6.59e-07     1.48e-06             1.2e-05   4.8e-07 / 4.4e-07 / 8.6e-07
    hypercube256   9.95e-07     2.05e-06             1.6e-05   7.9e-07 / 5.9e-07 / 7.6e-07
    grid16x20      8.60e-07     1.38e-06             1.1e-05   3.8e-07 / 5.0e-07 / 7.5e-07
    grid17x19      7.96e-07     1.50e-06             1.2e-05   4.5e-07 / 3.3e-07 / 9.1e-07
    copies         6.95e-07     9.75e-07             7.8e-06   4.2e-07 / 6.4e-07 / 5.9e-07
    knn            1.07e-06     1.86e-06             1.5e-05   5.6e-07 / 5.4e-07 / 1.3e-06
    selfmix        5.39e-07     9.00e-07             7.2e-06   2.8e-07 / 2.5e-07 / 6.1e-07
    identity       0            0                    1.0e-06   0 / 0 / 0

The device stays below the float32 LAPACK residual on every case (its eigenvalues and inverse iteration are fp64).  Launch-path
edges: worst res 1.43e-06 (N = 1025, LAPACK 5.99e-06); Jacobi edges: worst 6.62e-07 (N = 65).  Forecasts of the two spectral
routes (test_prior_graph_basis_eig_route_vs_cheb_route): worst relerr 2.1e-07 against the bound 1e-3.  Before the fix of the
zero Laplacian the two `identity` cases and the zero matrix of the batched test ended with status 3 (cluster re-solve broke
down on NaN vectors).
"""
import functools

import pytest
import torch

from oracle import stemgnn_oracle as O
from tests.helpers import eigh_cases as E
from tests.util import DEV, SENTINEL, _Buf, _all_nan, _bits, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-4


def _lib():
    from stemgnn_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


class _Call:
    """The buffers of one call for `mats` ([batch] of [N,N] float32): sentinel / matrix / NaN / NaN slots per matrix."""

    def __init__(self, mats, scratch_floats=None):
        self.N = N = mats[0].shape[0]
        self.batch = len(mats)
        nn = N * N
        self.S = _lib().stemgnn_eigh_scratch_floats(N) if scratch_floats is None else scratch_floats
        self.mul = _Buf(self.batch * 4 * nn)
        view = self.mul.t.view(self.batch, 4, nn)
        view[:, 0] = SENTINEL
        for m, L in enumerate(mats):
            view[m, 1] = L.reshape(-1).to(DEV)
        self.lam, self.U, self.scr = _Buf(self.batch * N), _Buf(self.batch * nn), _Buf(self.batch * self.S)
        self.before = self.mul.t.clone()

    def ptrs(self):
        return self.mul.ptr(), self.lam.ptr(), self.U.ptr(), self.scr.ptr()

    def guards(self):
        return all(b.intact() for b in (self.mul, self.lam, self.U, self.scr))

    def untouched(self):
        return (_bits(self.mul.t, self.before) and _all_nan(self.lam.t) and _all_nan(self.U.t) and _all_nan(self.scr.t)
                and self.guards())

    def done(self, rc, what):
        from stemgnn_amd import ops
        torch.cuda.synchronize()
        assert rc == 0, (what, rc)
        ops.check_eigh_status()
        N, nn = self.N, self.N * self.N
        got, was = self.mul.t.view(self.batch, 4, nn), self.before.view(self.batch, 4, nn)
        assert _bits(got[:, :2], was[:, :2]), f"{what}: slot 0 / 1 changed"
        for name, t in (("lam", self.lam.t), ("U", self.U.t), ("slots 2 / 3", got[:, 2:])):
            assert bool(torch.isfinite(t).all()), f"{what}: {name} holds a NaN or inf"
        assert self.guards(), f"{what}: a guard band was written"
        return self.mul.t.view(self.batch, 4, N, N), self.lam.t.view(self.batch, N), self.U.t.view(self.batch, N, N)


def _solve(L, sweeps=0, scratch_floats=None):
    c = _Call([L], scratch_floats)
    rc = _lib().stemgnn_eigh_fwd(*c.ptrs(), c.N, sweeps, _stream())
    mul, lam, U = c.done(rc, f"eigh_fwd N {c.N} sweeps {sweeps}")
    return mul[0], lam[0], U[0]


def _check(what, L, ref, mul, lam, U, rep):
    """all metrics of one solution against fp64; returns them"""
    m = E.metrics(L, lam, U, ref["ev"])
    m["T2"], m["T3"] = relerr(mul[2], ref["T2"]), relerr(mul[3], ref["T3"])
    lim = E.res_limit(ref["lapack"]["res"])
    print(f"{what}: ev {m['ev']:.2e} orth {m['orth']:.2e} rec {m['rec']:.2e} T2 {m['T2']:.2e} T3 {m['T3']:.2e} | "
          f"res {m['res']:.2e} | LAPACK {ref['lapack']['res']:.2e} | limit {lim:.1e}")
    eo = 2e-5 if rep else 1e-5
    assert m["ev"] < eo and m["orth"] < eo, (what, m)
    assert m["rec"] < 2e-5, (what, m)
    assert m["T2"] < TOL and m["T3"] < TOL, (what, m)
    assert m["res"] < lim, (what, m["res"], lim)
    return m


@functools.lru_cache(maxsize=None)
def _oracle(N, seed=0):
    """(L, reference) of the oracle's latent Laplacian, B = 2 windows beyond N = 256 as in test_hip_gru_eigh.py; shared"""
    L = E.oracle_laplacian(N, B=6 if N <= 256 else 2, seed=seed).contiguous()
    return L, E.reference(L)


@functools.lru_cache(maxsize=None)
def _split_pairs(N):
    from tests.test_hip_gru_eigh import _degenerate
    L = _degenerate("split_pairs", N).contiguous()
    return L, E.reference(L)


# ---- a. prior-graph spectra -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(E.CASES))
def test_eigh_prior_graph_spectra(name):
    A, L, ref = E.case(name)
    lib = _lib()
    lib.stemgnn_eigh_cluster_fixes()
    mul, lam, U = _solve(L)
    print(f"{name}: {lib.stemgnn_eigh_cluster_fixes()} eigenvectors re-orthogonalised by the cluster pass")
    m = _check(name, L, ref, mul, lam, U, E.repeated(name))
    if name == "identity":
        assert float(lam.abs().max()) <= 1e-30
        assert bool((mul[2] == 0).all()) and bool((mul[3] == 0).all())
        assert m["orth"] < 1e-5


# ---- b. launch-path edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 63, 65, 255, 256, 257, 300, 320, 1025])
def test_eigh_launch_path_edges(N):
    """The oracle's Laplacian at the smallest accepted sizes (one reflector; N - 3 = 0 in the back-transform), around a lane
    chunk, on both sides of the register / general tridiagonalisation boundary, in the one-workgroup general kernel with
    real reflectors (257, 300, 320) and at the smallest size of the <32,4> back-transform."""
    L, ref = _oracle(N)
    mul, lam, U = _solve(L)
    _check(f"oracle N {N}", L, ref, mul, lam, U, False)


@pytest.mark.parametrize("entry,N,arg", [("fwd", 2, 0), ("fwd", 2049, 0), ("batched", 2, 1), ("fwd", 33, 65)])
def test_eigh_refusals_leave_the_buffers_alone(entry, N, arg):
    lib = _lib()
    c = _Call([torch.eye(N) * 0.5])
    if entry == "fwd":
        rc = lib.stemgnn_eigh_fwd(*c.ptrs(), N, arg, _stream())
    else:
        rc = lib.stemgnn_eigh_batched(*c.ptrs(), N, arg, _stream())
    torch.cuda.synchronize()
    assert rc != 0
    assert c.untouched()


# ---- c. the batched entry on matrices of different kinds ------------------------------------------------------------------------
def _batch_run(items):
    """items: [(label, L, ref, repeated)] of one N.  One batched call; per matrix the bits of a single call and the metrics.
    Returns the per-matrix (lam, U, mul_L)."""
    lib = _lib()
    c = _Call([it[1] for it in items])
    rc = lib.stemgnn_eigh_batched(*c.ptrs(), c.N, c.batch, _stream())
    mul, lam, U = c.done(rc, f"eigh_batched N {c.N} batch {c.batch}")
    for m, (label, L, ref, rep) in enumerate(items):
        one = _Call([L])
        rc = lib.stemgnn_eigh_fwd(*one.ptrs(), one.N, 0, _stream())
        mul1, lam1, U1 = one.done(rc, f"eigh_fwd for {label}")
        assert _bits(lam[m], lam1[0]) and _bits(U[m], U1[0]) and _bits(mul[m], mul1[0]), (label, m)
        _check(f"batched[{m}] {label}", L, ref, mul[m], lam[m], U[m], rep)
    return [(lam[m].clone(), U[m].clone(), mul[m].clone()) for m in range(c.batch)]


def test_eigh_batched_mixed_kinds():
    """Matrices of different kinds side by side in one batched call (N = 64: the batch is a grid dimension of every stage;
    N = 257: the general tridiagonalisation looped per matrix): a clustered spectrum, a zero matrix or a split tridiagonal
    next to a latent Laplacian must not change its neighbours' bits, in either order."""
    zero = torch.zeros(64, 64)
    items = [("ring64",) + E.case("ring64")[1:] + (True,), ("hypercube64",) + E.case("hypercube64")[1:] + (True,),
             ("zero", zero, E.reference(zero), True), ("oracle",) + _oracle(64) + (False,),
             ("split_pairs",) + _split_pairs(64) + (True,)]
    fwd = _batch_run(items)
    rev = _batch_run(items[::-1])[::-1]
    for (label, *_), a, b in zip(items, fwd, rev):
        assert all(_bits(x, y) for x, y in zip(a, b)), f"{label}: bits depend on the neighbours"
    _batch_run([("ring257",) + E.case("ring257")[1:] + (True,), ("oracle",) + _oracle(257) + (False,)])


# ---- d. the Jacobi route below one block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 65])
def test_eigh_jacobi_edges(N):
    """nsweeps = 9 at the odd / even tournament sizes below one block, on 3 N^2 floats of scratch."""
    L, ref = _oracle(N)
    mul, lam, U = _solve(L, sweeps=9, scratch_floats=3 * N * N)
    _check(f"jacobi N {N}", L, ref, mul, lam, U, False)


# ---- e. prior graphs through LatentGraph and the model --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ring64", "star96", "grid17x19", "selfmix", "identity"])
def test_prior_graph_basis_eig_route_vs_cheb_route(name, monkeypatch):
    """LatentGraph.from_adjacency(A).basis() on both spectral routes against the fp64 polynomials of the fp64 Laplacian, and
    one forecast from each.  Forecast bound: relerr(eig, cheb) < 1e-3, ten times the basis tolerance (two blocks' GFT products
    amplify the basis error)."""
    from stemgnn_amd import LatentGraph, Model, ops

    A = E.case(name)[0]
    N = A.shape[0]
    L64 = O.laplacian_from_attention(A[None].double())[0]
    ref = O.cheb_polynomial(L64)
    sd = O.det_state_dict(N, 12, 5, 3)
    model = Model(N, 2, 12, 5, horizon=3, dropout_rate=0.0)
    model.load_state_dict(sd)
    model.to(DEV).eval()
    x = torch.randn(3, 12, N, generator=torch.Generator().manual_seed(N)).to(DEV)
    out = {}
    for route in ("cheb", "eig"):
        monkeypatch.setenv("STEMGNN_SPECTRAL", route)
        graph = LatentGraph.from_adjacency(A.to(DEV))
        att, mul = graph.basis()
        forecast, _ = model.predict(x, adjacency=graph)
        torch.cuda.synchronize()
        ops.check_eigh_status(DEV)
        errs = [relerr(mul[k], ref[k]) for k in (1, 2, 3)]
        print(f"{name} {route}: L {errs[0]:.2e} T2 {errs[1]:.2e} T3 {errs[2]:.2e}")
        assert bool(torch.isfinite(mul).all()) and all(e < TOL for e in errs), (route, errs)
        assert bool(torch.isfinite(forecast).all()), route
        out[route] = (att.clone(), mul.clone(), forecast.clone())
    assert _bits(out["eig"][0], out["cheb"][0])
    assert _bits(out["eig"][1][:2], out["cheb"][1][:2])
    e = relerr(out["eig"][2], out["cheb"][2])
    print(f"{name}: forecast eig vs cheb {e:.2e}")
    assert e < 1e-3, e
