"""CPU: the input-gradient entries of include/stemgnn_hip.h refuse bad arguments, and the fp64 oracle's x-gradient matches
the real reference's (tests/golden/input_grad/*.npz, written by tests/golden/make_golden_input_grad.py)."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import stemgnn_oracle as O
from tests.util import GOLDEN_DIR, hash_seed, relerr

SG_EINVAL = -10001
TOL64 = 2e-5                    # tests/test_oracle_golden.py: fp64 oracle vs the reference's fp32 round-off
INPUT_GRAD_DIR = os.path.join(GOLDEN_DIR, "input_grad")
P = 64                          # a stand-in device address: every call below is refused before anything is read


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_gru_input_grad_rejects_bad_arguments(lib):
    ok = dict(scratch=P, w_ih=P, B=2, S=5, Hd=5, W=3, dx=P)
    for k in ("scratch", "w_ih", "dx"):
        assert lib.stemgnn_gru_input_grad(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k in ("B", "S", "Hd", "W"):
        for v in (0, -1):
            assert lib.stemgnn_gru_input_grad(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)


def test_gru_bwd_recur_rejects_bad_arguments(lib):
    ok = dict(dh_all=P, x=P, w_hh=P, h_ext=P, reserve=P, B=2, S=5, Hd=5, W=3, scratch=P, status=P)
    for k in ("dh_all", "x", "w_hh", "h_ext", "reserve", "scratch", "status"):
        assert lib.stemgnn_gru_bwd_recur(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k in ("B", "S", "Hd", "W"):
        for v in (0, -1):
            assert lib.stemgnn_gru_bwd_recur(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)


def test_gru_bwd_rank2_recur_rejects_bad_arguments(lib):
    ok = dict(dkey=P, dquery=P, nchunk=16, wk=P, wq=P, x=P, w_hh=P, h_ext=P, reserve=P, B=2, S=5, Hd=5, W=3, scratch=P,
              status=P)
    for k in ("dkey", "dquery", "wk", "wq", "x", "w_hh", "h_ext", "reserve", "scratch", "status"):
        assert lib.stemgnn_gru_bwd_rank2_recur(*{**ok, k: None}.values(), None) == SG_EINVAL, k
    for k in ("B", "S", "Hd", "W"):
        for v in (0, -1):
            assert lib.stemgnn_gru_bwd_rank2_recur(*{**ok, k: v}.values(), None) == SG_EINVAL, (k, v)
    assert lib.stemgnn_gru_bwd_rank2_recur(*{**ok, "nchunk": -1}.values(), None) == SG_EINVAL


def input_grad_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(INPUT_GRAD_DIR, "*.npz")))


def oracle_x_grad(z, name, dtype=torch.float64):
    """d(MSE loss)/dx of the oracle (autograd through O.model_forward) on a fixture's inputs, weights and dropout mask."""
    N, W, m, H, B, mode = (int(v) for v in z["cfg"])
    sd = O.det_state_dict(N, W, m, H, seed=hash_seed(name), dtype=dtype)
    x = torch.from_numpy(z["x"]).to(dtype).requires_grad_(True)
    kw = dict(drop_mask=torch.from_numpy(z["drop_mask"]).to(dtype), drop_p=0.5) if mode == 2 else {}
    forecast, _ = O.model_forward(x, sd, **kw)
    loss = torch.nn.functional.mse_loss(forecast, torch.from_numpy(z["y"]).to(dtype))
    return torch.autograd.grad(loss, x)[0], loss.detach()


def test_all_golden_cases_have_an_input_grad_fixture():
    from tests.golden.make_golden import CASES

    assert input_grad_cases() == sorted(CASES)


@pytest.mark.parametrize("name", input_grad_cases())
def test_oracle_x_grad_matches_reference_fixture(name):
    z = np.load(os.path.join(INPUT_GRAD_DIR, name + ".npz"))
    g, loss = oracle_x_grad(z, name)
    assert g.shape == z["x_grad"].shape
    assert float(np.abs(z["x_grad"]).max()) > 0.0
    assert abs(float(loss) - float(z["loss"])) < TOL64 * max(1.0, abs(float(z["loss"])))
    assert relerr(g, z["x_grad"]) < 5 * TOL64, relerr(g, z["x_grad"])
