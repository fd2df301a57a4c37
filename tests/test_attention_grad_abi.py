"""CPU: the attention-gradient entry of include/stemgnn_hip.h is declared, exported and refuses bad arguments before
anything is launched; the public interface carries the new arguments; the oracle's penalty gradients behave as the tests of
tests/test_hip_attention_grad.py assume (a row-constant gradient for the attention is annihilated, the penalties used there
are not)."""
import inspect
import os
import re

import pytest
import torch

from oracle import stemgnn_oracle as O

SG_EINVAL = -10001
P = 64                          # a stand-in device address: every call below is refused before anything is read
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_ext_entry_is_declared_and_exported(lib):
    from stemgnn_amd import _lib

    header = open(os.path.join(ROOT, "include", "stemgnn_hip.h")).read()
    assert re.search(r"\bint\s+stemgnn_attn_laplacian_bwd_ext\s*\(", header)
    plain, ext = (_lib.SIGNATURES[n] for n in ("stemgnn_attn_laplacian_bwd", "stemgnn_attn_laplacian_bwd_ext"))
    assert ext[0] is plain[0] and len(ext[1]) == len(plain[1]) + 1          # the plain entry's arguments plus dA_ext
    assert ext[1][:1] + ext[1][2:] == plain[1]
    assert hasattr(lib, "stemgnn_attn_laplacian_bwd_ext")


def _ok():
    return dict(dL=P, dA_ext=P, h=P, wk=P, wq=P, alpha=0.2, drop_p=0.0, training=1, seed=None, B=2, N=5, saved=P, scratch=P,
                nchunk=16, dh=P, dwk=P, dwq=P, parts=3)


def test_ext_entry_rejects_bad_arguments(lib):
    ok = _ok()
    call = lambda **kw: lib.stemgnn_attn_laplacian_bwd_ext(*{**ok, **kw}.values(), None)
    assert call(dL=None, dA_ext=None) == SG_EINVAL, "no gradient at all"
    for k in ("h", "wk", "wq", "saved", "scratch"):
        assert call(**{k: None}) == SG_EINVAL, k
        assert call(**{k: None}, dL=None) == SG_EINVAL, (k, "attention-only")
    for k in ("dh", "dwk", "dwq"):                           # outputs of the materialised form; the factored form takes NULL
        assert call(**{k: None}) == SG_EINVAL, k
    for k in ("B", "N", "nchunk"):
        for v in (0, -1):
            assert call(**{k: v}) == SG_EINVAL, (k, v)
    assert call(parts=0) == SG_EINVAL and call(parts=4) == SG_EINVAL
    assert call(drop_p=0.5) == SG_EINVAL, "dropout without a seed"
    assert call(drop_p=1.0, seed=P) == SG_EINVAL and call(drop_p=-0.1, seed=P) == SG_EINVAL


def test_plain_entry_still_requires_dL(lib):
    ok = _ok()
    del ok["dA_ext"]
    assert lib.stemgnn_attn_laplacian_bwd(*{**ok, "dL": None}.values(), None) == SG_EINVAL


def test_public_interface_carries_the_new_arguments():
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep

    p = inspect.signature(Model.loss).parameters
    assert "return_attention" in p and p["return_attention"].default is False
    p = inspect.signature(TrainStep.__init__).parameters
    assert "attention_penalty" in p and p["attention_penalty"].default is None


def test_oracle_row_constant_attention_gradient_is_annihilated():
    """Why the GPU tests use a Frobenius prior and a random linear form, not A.sum(): without dropout the rows of the softmax
    sum to 1, so a penalty whose gradient is constant along the rows of the symmetrised attention has an analytically zero
    gradient -- a relative error against it would measure rounding noise."""
    N, W, multi, H, B = 20, 12, 5, 3, 4
    sd = {k: v.double().requires_grad_(True) for k, v in O.det_state_dict(N, W, multi, H, seed=1).items()}
    x = torch.randn(B, W, N, generator=torch.Generator().manual_seed(0)).double()
    _, A = O.model_forward(x, sd)
    names = ("weight_key", "weight_query")
    g_sum = torch.autograd.grad(A.sum(), [sd[k] for k in names], retain_graph=True)
    prior = torch.rand(N, N, generator=torch.Generator().manual_seed(1)).double() / N
    g_fro = torch.autograd.grad(((A - prior) ** 2).sum(), [sd[k] for k in names])
    for gs, gf in zip(g_sum, g_fro):
        assert float(gs.abs().max()) < 1e-12 < 1e-6 < float(gf.abs().max())
