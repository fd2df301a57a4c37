"""CPU: the prior-graph cases of tests/helpers/eigh_cases.py are what their table claims -- valid adjacencies for
LatentGraph.from_adjacency, symmetric Laplacians, the stated multiplicities in the fp64 spectrum -- and the float32 LAPACK
solution of every one of them is inside the bounds the device suite (tests/test_hip_eigh.py) asks of the HIP solver, so
those bounds are attainable in the solver's own precision."""
import pytest
import torch

from tests.helpers import eigh_cases as E


@pytest.mark.parametrize("name", list(E.CASES))
def test_case_is_a_valid_prior_graph_with_the_claimed_spectrum(name):
    A, L, ref = E.case(name)
    N = A.shape[0]
    assert A.dtype == torch.float32 and A.shape == (N, N) and L.shape == (N, N)
    assert bool((A >= 0).all())
    assert bool((A.double().sum(dim=1) > 0).all()) and bool((A.sum(dim=1) > 0).all())
    assert float((L - L.T).abs().max()) <= 1e-7
    ev = ref["ev"]
    gaps = E.close_gaps(ev, float(L.double().abs().max()))
    want = E.CASES[name][3]
    print(f"{name}: N = {N}, spectrum [{float(ev.min()):.2e}, {float(ev.max()):.6f}], {gaps} gaps below 1e-9 |L|")
    if name == "identity":
        assert bool((L == 0).all()) and bool((ev == 0).all())
    if want is not None:
        assert gaps == want, (gaps, want)
    if name == "selfmix":
        assert bool((L[:5] == 0).all()) and bool((L[:, :5] == 0).all())
    if name == "copies":                                                        # four-fold up to fp32 rounding
        assert float((ev.view(60, 4).max(dim=1).values - ev.view(60, 4).min(dim=1).values).max()) < 1e-6
    if name == "knn":
        assert not torch.equal(A, A.T) and int((A > 0).sum()) == 6 * N


@pytest.mark.parametrize("name", list(E.CASES))
def test_float32_lapack_meets_the_device_bounds(name):
    A, L, ref = E.case(name)
    m = ref["lapack"]
    print(f"{name}: float32 LAPACK ev {m['ev']:.2e} orth {m['orth']:.2e} rec {m['rec']:.2e} res {m['res']:.2e}")
    assert m["ev"] < 1e-5 and m["orth"] < 1e-5 and m["rec"] < 1e-5 and m["res"] < 1e-5, m


def test_metrics_see_one_bad_eigenvector():
    """`res` is per vector: eigenvector 7 with 1e-3 of eigenvector 150 mixed in has the residual 1e-3 |lam_150 - lam_7|."""
    L = E.case("knn")[1].double()
    L = 0.5 * (L + L.T)                                   # (the float32 Laplacian is symmetric to 1e-7 only)
    ev, Q = torch.linalg.eigh(L)
    lam, U = ev, Q.T.contiguous()
    good = E.metrics(L, lam, U, ev)
    assert good["res"] < 1e-12 and good["orth"] < 1e-12
    U[7] = U[7] + 1e-3 * U[150]
    bad = E.metrics(L, lam, U, ev)
    gap = float((ev[150] - ev[7]).abs())
    assert abs(bad["res"] - 1e-3 * gap) < 1e-9 and bad["orth"] > 9e-4


def test_res_limit_floor_and_cap():
    assert E.res_limit(0.0) == 1e-6 and E.res_limit(5e-7) == 4e-6 and E.res_limit(1e-5) == 2e-5
