"""CPU: the inference-forward entry points of the C ABI (Model.predict / engine.ForecastStep) are exported, reject bad
arguments without launching anything, and size a workspace far smaller than the training forward's saved activations."""
import os

import pytest

from stemgnn_amd import _lib

INFER = ["stemgnn_gru_fwd_infer", "stemgnn_spectral_glu_fwd_infer", "stemgnn_spectral_glu_fwd_split_infer",
         "stemgnn_igft_heads_fwd_infer", "stemgnn_infer_workspace_floats", "stemgnn_infer_workspace_split_floats",
         "stemgnn_forecast_store"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_infer_symbols_exported_with_signatures(lib):
    for n in INFER:
        assert hasattr(lib, n), n
        assert n in _lib.SIGNATURES, n


def test_infer_entries_reject_null_and_bad_shapes(lib):
    E = _lib.SG_EINVAL
    fake = 1 << 20                       # never dereferenced: every call below fails its argument check first
    assert lib.stemgnn_gru_fwd_infer(None, None, None, None, None, 2, 8, 8, 4, None, None, None, None) == E
    assert lib.stemgnn_gru_fwd_infer(fake, fake, fake, fake, fake, 0, 8, 8, 4, fake, fake, fake, None) == E
    # the training entry still refuses a NULL reserve
    assert lib.stemgnn_gru_fwd(fake, fake, fake, fake, fake, 2, 8, 8, 4, fake, fake, None, fake, None) == E
    n_ws = lib.stemgnn_infer_workspace_floats(2, 8, 4, 2)
    assert lib.stemgnn_spectral_glu_fwd_infer(None, fake, n_ws, 2, 8, 4, 2, None) == E
    assert lib.stemgnn_spectral_glu_fwd_infer(fake, None, n_ws, 2, 8, 4, 2, None) == E
    assert lib.stemgnn_spectral_glu_fwd_infer(fake, fake, n_ws, 2, 8, 4, 0, None) == E
    assert lib.stemgnn_spectral_glu_fwd_infer(fake, fake, 16, 2, 8, 4, 2, None) == E          # workspace too small
    assert lib.stemgnn_spectral_glu_fwd_split_infer(fake, None, fake, n_ws, 2, 8, 4, 2, 2, None) == E
    assert lib.stemgnn_spectral_glu_fwd_split_infer(fake, fake, fake, n_ws, 2, 8, 4, 2, 1, None) == E
    assert lib.stemgnn_spectral_glu_fwd_split_infer(fake, fake, fake, 16, 2, 8, 4, 2, 2, None) == E
    parr = _lib.ptr_array([None] * _lib.SG_BLOCK_NPARAMS)
    assert lib.stemgnn_igft_heads_fwd_infer(None, fake, fake, n_ws, fake, 32, 1, 8, fake, 0, None, 2, 8, 4, 2, None) == E
    assert lib.stemgnn_igft_heads_fwd_infer(parr, fake, fake, 16, fake, 32, 1, 8, fake, 0, None, 2, 8, 4, 2, None) == E
    assert lib.stemgnn_igft_heads_fwd_infer(parr, fake, None, n_ws, fake, 32, 1, 8, fake, 0, None, 2, 8, 4, 2, None) == E
    assert lib.stemgnn_forecast_store(None, fake, fake, fake, fake, 2, 3, 8, 10, None) == E
    assert lib.stemgnn_forecast_store(fake, fake, fake, fake, fake, 2, 3, 8, 0, None) == E
    assert lib.stemgnn_infer_workspace_floats(0, 8, 4, 2) == 0
    assert lib.stemgnn_infer_workspace_split_floats(2, 8, 4, 2, 1) == 0


def test_infer_workspace_size_pems07(lib):
    # G [M, 3W] + the two layer-2 GLU outputs [M, CP2 = 128] each; the fused kernels keep layers 0 / 1 in LDS
    M = 32 * 228
    n = lib.stemgnn_infer_workspace_floats(32, 228, 12, 5)
    assert n == M * (36 + 2 * 128)
    assert n < lib.stemgnn_saved_floats(32, 228, 12, 5) // 8
    assert lib.stemgnn_infer_workspace_split_floats(32, 228, 12, 5, 0) == n
    assert lib.stemgnn_infer_workspace_split_floats(32, 228, 12, 5, 2) == n
    # bf16x3 always runs the per-layer launches: + two ping-pong slabs [M, CP = 240] per branch
    assert lib.stemgnn_infer_workspace_split_floats(32, 228, 12, 5, 3) == M * (36 + 2 * 128 + 4 * 240)


def test_infer_workspace_size_per_layer_shapes(lib):
    # 4 W multi > 256 (COVID W = 28): no fused GLU kernel, the ping-pong slabs are part of the workspace
    M, W, multi = 32 * 25, 28, 5
    Wm = W * multi
    cp = -(-4 * Wm // 16) * 16
    cp2 = [-(-4 * (Wm // 2 + 1) // 16) * 16, -(-4 * ((Wm + 1) // 2 - 1) // 16) * 16]
    n = lib.stemgnn_infer_workspace_floats(32, 25, W, multi)
    assert n == M * (3 * W + cp2[0] + cp2[1] + 4 * cp)
    assert n < lib.stemgnn_saved_floats(32, 25, W, multi)
