"""CPU: the C-ABI library builds for gfx950, loads, and exports every symbol include/stemgnn_hip.h declares.
No compute is launched (there is no GPU in the build container)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "stemgnn_hip.h")
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def declared_symbols():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(stemgnn_[a-zA-Z0-9_]+)\s*\(", src)))


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


def test_header_symbols_exported(lib):
    from stemgnn_amd import _lib

    names = declared_symbols()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/stemgnn_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in stemgnn_amd/_lib.py"
    assert set(_lib.SIGNATURES) == set(names)


def test_version_and_sizes(lib):
    assert b"gfx950" in lib.stemgnn_version()
    # PEMS07 shape: W=12, multi=5 -> GLU panels 36x480, 240x480, 240x480, 240x256 ... (layout.h)
    n = lib.stemgnn_packed_floats(12, 5)
    panels = 2 * (36 * 480 + 480 + 240 * 480 + 480) + (240 * 256 + 256) * 2 + 256 * 64
    # + the same weights as the 16 KB-stage streams of the fused kernels (csrc/glu_fused.h), 4096 floats per stage:
    # forward: per branch 5 (K 36 -> 40, 8 rows) + 30 (K 240, 8 rows) + 15 (K 240, 16 rows) stages;
    # data-gradient chain: per branch 16 (256 rows / 16) + 16 + 14 (two phases of 256 / 224 live rows) + 4 + 4 (64-row stages)
    expect = panels + 2 * (5 + 30 + 15) * 4096 + 2 * (16 + 16 + 14 + 4 + 4) * 4096
    assert n == expect
    assert lib.stemgnn_table_floats(12, 5) == 2 * 144 + 31 * 60 + 29 * 60
    assert lib.stemgnn_saved_floats(32, 228, 12, 5) == 7296 * (36 + 2 * 2 * (240 + 240 + 128) + 120)


def test_tables_host_math(lib):
    import numpy as np
    import torch

    W, multi = 12, 5
    Wm = W * multi
    n = lib.stemgnn_table_floats(W, multi)
    buf = torch.empty(n, dtype=torch.float32)
    assert lib.stemgnn_make_tables_host(W, multi, buf.data_ptr()) == 0
    t = buf.numpy().astype(np.float64)
    cosW = t[: W * W].reshape(W, W)
    sinW = t[W * W: 2 * W * W].reshape(W, W)
    cinvR = t[2 * W * W: 2 * W * W + 31 * Wm].reshape(31, Wm)
    cinvI = t[2 * W * W + 31 * Wm:].reshape(29, Wm)
    # forward DFT == torch.fft.fft on a random real signal
    g = torch.randn(5, W, dtype=torch.float64)
    ff = torch.fft.fft(g, dim=-1)
    assert np.abs(g.numpy() @ cosW - ff.real.numpy()).max() < 1e-6
    assert np.abs(-(g.numpy() @ sinW) - ff.imag.numpy()).max() < 1e-6
    # C2R inverse == torch.fft.irfft on the first Wm/2+1 bins of an arbitrary (non-Hermitian) spectrum
    re, im = torch.randn(3, Wm, dtype=torch.float64), torch.randn(3, Wm, dtype=torch.float64)
    y = torch.fft.irfft(torch.complex(re, im)[..., : Wm // 2 + 1], n=Wm, dim=-1).numpy()
    mine = re.numpy()[:, :31] @ cinvR + im.numpy()[:, 1:30] @ cinvI
    assert np.abs(mine - y).max() < 1e-6
    assert sinW[:, 0].max() == 0.0 and np.abs(sinW[:, W // 2]).max() == 0.0   # exact zeros at DC / Nyquist


def test_invalid_args_return_einval(lib):
    assert lib.stemgnn_cheb_fwd(None, 8, None) == -10001
    assert lib.stemgnn_make_tables_host(0, 5, None) == -10001
    # the data-path entries refuse NULL buffers and series shorter than one window before any HIP call
    assert lib.stemgnn_window_gather(None, None, None, None, 4, 12, 3, 8, 100, None, None) == -10001
    assert lib.stemgnn_window_gather_queue(None, None, None, None, None, 4, 12, 3, 8, 100, None, None) == -10001
    assert lib.stemgnn_gru_bwd_rank2_ok(0, 228) == 0       # (what it answers for a real shape depends on the device's CU count)


def test_model_refuses_cpu():
    import torch

    from stemgnn_amd import Model
    from stemgnn_amd._lib import StemGNNHipError

    m = Model(6, 2, 4, 2, horizon=2)
    with pytest.raises(StemGNNHipError):
        m(torch.randn(2, 4, 6))


def test_state_dict_contract_matches_reference_order():
    import torch

    from oracle import stemgnn_oracle as O
    from stemgnn_amd import Model

    m = Model(10, 2, 12, 5, horizon=3)
    shapes = O.param_shapes(10, 12, 5, 3)
    got = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    assert got == list(shapes.items())
    assert [k for k, _ in m.named_parameters()] == list(shapes.keys())


@pytest.mark.parametrize("stack_cnt", [1, 3])
def test_constructor_accepts_any_stack_count_like_the_reference(stack_cnt):
    """reference :93-95 builds `stack_cnt` blocks; only block 0 owns `backcast` (:29-30); train()/eval() on a CPU model
    (never ran a kernel) must not touch the device."""
    from stemgnn_amd import Model

    m = Model(6, stack_cnt, 4, 2, horizon=2)
    assert len(m.stock_block) == stack_cnt and hasattr(m.stock_block[0], "backcast")
    assert all(not hasattr(b, "backcast") for b in m.stock_block[1:])
    keys = list(m.state_dict().keys())
    assert sum(k.startswith(f"stock_block.{stack_cnt - 1}.") for k in keys) > 0
    m.eval(); m.train()
    # the reference's own state_dict for the same constructor call (tests/golden/make_golden.py run_stack_case)
    z = np.load(os.path.join(GOLDEN_DIR, "ref_init", f"stack{stack_cnt}.npz"))
    assert [(k, tuple(z["shape." + k])) for k in z["keys"].tolist()] == \
           [(k, tuple(v.shape)) for k, v in m.state_dict().items()]


def test_model_constructor_rejects_shapes_outside_the_fc_tail_range(lib):
    """The reference takes any window / horizon (nn.Sequential fc, models/base_model.py:97-101); the HIP fc tail covers
    time_step <= 64, horizon <= 32 and there is no torch fallback -- the constructor says so immediately."""
    from stemgnn_amd import Model
    from stemgnn_amd._lib import StemGNNHipError
    Model(6, 2, 64, 1, horizon=32)
    for w, h in ((65, 3), (12, 33)):
        with pytest.raises(StemGNNHipError, match="fc tail"):
            Model(6, 2, w, 1, horizon=h)
    assert lib.stemgnn_fc_tail_supported(64, 32) == 1 and lib.stemgnn_fc_tail_supported(65, 3) == 0
