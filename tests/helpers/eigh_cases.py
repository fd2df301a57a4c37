"""Prior-graph adjacencies, the float32 Laplacian the device forms from them, and the fp64 reference and metrics of the
eigensolver suites (tests/test_eigh_cases.py on the CPU, tests/test_hip_eigh.py on the device).  CPU only: nothing here
touches the library.

The latent Laplacian the solver was written for is dense with N - 1 eigenvalues packed into [0.99, 1.01].  The graphs below
are what ``LatentGraph.from_adjacency`` feeds it instead: eigenvalues spread over [0, 2], structurally exact multiplicities,
disconnected components, zero rows, and tridiagonals that split.  Every generator is deterministic (torch.Generator seeds)
and returns the un-symmetrised float32 adjacency."""
import functools
import itertools

import torch

from oracle import stemgnn_oracle as O
from tests.util import relerr


# ---- adjacencies ---------------------------------------------------------------------------------------------------------
def ring(N):
    """cycle C_N: eigenvalues 1 - cos(2 pi k / N), every one but 0 (and 2, N even) exactly double"""
    A = torch.zeros(N, N)
    i = torch.arange(N)
    A[i, (i + 1) % N] = 1.0
    A[i, (i - 1) % N] = 1.0
    return A


def path(N):
    """path P_N: L is tridiagonal already, every reflector is skipped"""
    A = torch.zeros(N, N)
    i = torch.arange(N - 1)
    A[i, i + 1] = 1.0
    A[i + 1, i] = 1.0
    return A


def star(N):
    """K_{1,N-1}: eigenvalue 1 with multiplicity N - 2, plus 0 and 2"""
    A = torch.zeros(N, N)
    A[0, 1:] = 1.0
    A[1:, 0] = 1.0
    return A


def bipartite(p, q):
    """K_{p,q}: eigenvalue 1 with multiplicity p + q - 2, plus the paired extremes 0 and 2"""
    A = torch.zeros(p + q, p + q)
    A[:p, p:] = 1.0
    A[p:, :p] = 1.0
    return A


def hypercube(d):
    """Q_d: eigenvalues 2 k / d with multiplicity C(d, k)"""
    N = 1 << d
    A = torch.zeros(N, N)
    i = torch.arange(N)
    for b in range(d):
        A[i, i ^ (1 << b)] = 1.0
    return A


def grid(r, c):
    """r x c four-neighbour grid: sparse, degrees 2 / 3 / 4"""
    A = torch.zeros(r * c, r * c)
    for y, x in itertools.product(range(r), range(c)):
        for yy, xx in ((y + 1, x), (y, x + 1)):
            if yy < r and xx < c:
                A[y * c + x, yy * c + xx] = 1.0
                A[yy * c + xx, y * c + x] = 1.0
    return A


def copies(k, n, seed=21):
    """k identical dense random components: block diagonal, T splits, every eigenvalue k-fold up to fp32 rounding"""
    blk = torch.rand(n, n, generator=torch.Generator().manual_seed(seed)) + 0.05
    return torch.block_diag(*([blk] * k)).contiguous()


def knn(N, k, seed=22):
    """k nearest neighbours of N random points of the unit square, weight exp(-4 dist): sparse and asymmetric"""
    pts = torch.rand(N, 2, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    dist = torch.cdist(pts, pts)
    dist.fill_diagonal_(float("inf"))
    d, idx = torch.topk(dist, k, dim=1, largest=False)
    A = torch.zeros(N, N, dtype=torch.float64)
    A.scatter_(1, idx, torch.exp(-4.0 * d))
    return A.float()


def selfmix(N=140, seed=23):
    """10 %-dense random weights + 0.5 I; nodes 0..4 keep their self-loop only: L has five zero rows and T splits"""
    g = torch.Generator().manual_seed(seed)
    A = torch.rand(N, N, generator=g) * (torch.rand(N, N, generator=g) < 0.1) + 0.5 * torch.eye(N)
    A[:5] = 0.0
    A[:, :5] = 0.0
    A[torch.arange(5), torch.arange(5)] = 0.5
    return A.contiguous()


def identity(N):
    """A = 2 I: L = 0 exactly"""
    return 2.0 * torch.eye(N)


# name -> (generator, its arguments, repeated eigenvalues by construction, gaps below 1e-9 |L| in the fp64 spectrum or None
# where the count is not structural)
CASES = {
    "ring64": (ring, (64,), True, 31),
    "ring257": (ring, (257,), True, 128),
    "path65": (path, (65,), False, 0),
    "star96": (star, (96,), True, 93),
    "bipartite": (bipartite, (40, 88), True, 125),
    "hypercube64": (hypercube, (6,), True, 57),
    "hypercube256": (hypercube, (8,), True, 247),
    "grid16x20": (grid, (16, 20), False, 0),
    "grid17x19": (grid, (17, 19), False, 0),
    "copies": (copies, (4, 60), True, None),
    "knn": (knn, (300, 6), False, 0),
    "selfmix": (selfmix, (), False, None),
    "identity": (identity, (33,), True, None),
}


def adjacency(name):
    fn, args, _, _ = CASES[name]
    return fn(*args)


def repeated(name):
    return CASES[name][2]


def close_gaps(ev, scale):
    """neighbouring fp64 eigenvalues closer than 1e-9 of `scale` (the solver's cluster threshold)"""
    return int((ev[1:] - ev[:-1] < 1e-9 * scale).sum())


# ---- Laplacians ----------------------------------------------------------------------------------------------------------
def laplacian_fp(A):
    """The float32 Laplacian as sg_laplacian_fwd_kernel forms it: deg = rowsum(A) before the symmetrisation,
    S = (A + A^T) / 2, dh = 1 / (sqrt(deg) + 1e-7), L_ij = dh_i ((delta_ij deg_i - S_ij) dh_j)."""
    A = A.float()
    deg = A.sum(dim=1)
    S = 0.5 * (A + A.T)
    dh = 1.0 / (torch.sqrt(deg) + torch.tensor(1e-7))
    return (dh[:, None] * ((torch.diag(deg) - S) * dh[None, :])).contiguous()


def oracle_laplacian(N, B=6, seed=0):
    """The latent Laplacian of the oracle's front for B random windows (models/base_model.py:137-147)."""
    sd = O.det_state_dict(N, 12, 5, 3, seed=seed)
    torch.manual_seed(seed)
    x = torch.randn(B, 12, N)
    att = O.self_graph_attention(O.gru_front(x, sd), sd["weight_key"], sd["weight_query"])
    return O.laplacian_from_attention(att)[0]


@functools.lru_cache(maxsize=None)
def case(name):
    """(A, L, reference(L)) of a table row, computed once per process and shared: treat as read-only"""
    A = adjacency(name)
    L = laplacian_fp(A)
    return A, L, reference(L)


# ---- reference and metrics -------------------------------------------------------------------------------------------------
def metrics(L, lam, U, ev=None):
    """fp64 metrics of an eigen-decomposition with the eigenvectors in the ROWS of U (the device's layout):
    ev max |sort(lam) - eigvalsh(L)|, orth max |U U^T - I|, rec relerr(U^T diag(lam) U, L), res max_e |L u_e - lam_e u_e|_2."""
    Ld, lam, U = L.double().cpu(), lam.double().cpu(), U.double().cpu()
    N = Ld.shape[0]
    if ev is None:
        ev = torch.linalg.eigvalsh(Ld)
    return {"ev": float((torch.sort(lam).values - ev).abs().max()),
            "orth": float((U @ U.T - torch.eye(N, dtype=torch.float64)).abs().max()),
            "rec": relerr((U.T * lam) @ U, Ld),
            "res": float((U @ Ld - lam[:, None] * U).norm(dim=1).max())}


def reference(L):
    """fp64 eigenvalues, fp64 2 L^2 and 4 L^3 - L, and the float32 LAPACK solution (torch.linalg.eigh on the CPU) with its
    own four metrics."""
    Ld = L.double()
    ev = torch.linalg.eigvalsh(Ld)
    T2 = 2.0 * Ld @ Ld
    T3 = 2.0 * Ld @ T2 - Ld
    lam32, Q32 = torch.linalg.eigh(L.float())
    U32 = Q32.T.contiguous()
    return {"ev": ev, "T2": T2, "T3": T3, "lapack_lam": lam32, "lapack_U": U32, "lapack": metrics(L, lam32, U32, ev)}


def res_limit(lapack_res):
    """Bound on the device's per-vector residual: 8 x the float32 LAPACK residual of the same matrix (the device reduces in
    the same precision with unblocked fp32 dot products: a small constant over LAPACK), floor 1e-6, cap 2e-5."""
    return min(max(8.0 * lapack_res, 1e-6), 2e-5)
