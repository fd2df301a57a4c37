"""Phased small-product kernel (csrc/gemm_phased.h) against the generic launches it replaces: the five graph-product entry
points through the C ABI, STEMGNN_GRAPH_PHASED on (default) and =0, must agree BIT FOR BIT (same MFMA stream, same flush
points), at ragged and N % 4 != 0 sizes and with both layouts of X; and both agree with an fp64 product within the bounds
the stage tests of test_hip_parity.py use: 2e-6 norm-relative for one product (test_both_blocks_dT_as_one_product_...),
1e-5 for the Chebyshev stage (test_stage_cheb_large_n_and_abi_errors), whose outputs chain two products."""
import pytest
import torch

from tests.util import relerr

pytestmark = pytest.mark.gpu

NS = [24, 140, 228, 300, 358]
BATCH = {24: 3, 140: 7, 228: 32, 300: 5, 358: 4}      # B W = 384 (tile-aligned phase boundary) at 228, ragged elsewhere
W = 12
LAYOUTS = ["bwn", "bnw"]


def _x(layout, B, N, g, dev):
    """X[b, n, t] stored as [B, W, N] (the model's input window) or [B, N, W] (a block's backcast): tensor, strides
    (b, n, t), and the fp64 [B, N, W] view."""
    if layout == "bwn":
        x = torch.randn(B, W, N, generator=g).to(dev)
        return x, (W * N, 1, N), x.double().permute(0, 2, 1)
    x = torch.randn(B, N, W, generator=g).to(dev)
    return x, (N * W, W, 1), x.double()


def _both(monkeypatch, run):
    """run() with the phased launches and with the generic ones"""
    monkeypatch.delenv("STEMGNN_GRAPH_PHASED", raising=False)
    on = run()
    monkeypatch.setenv("STEMGNN_GRAPH_PHASED", "0")
    off = run()
    monkeypatch.delenv("STEMGNN_GRAPH_PHASED", raising=False)
    return on, off


@pytest.mark.parametrize("N", NS)
def test_cheb_fwd(N, monkeypatch):
    from stemgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N)
    L = (torch.randn(N, N, generator=g) / N ** 0.5).to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        mul_L = torch.zeros(4, N, N, device=dev)
        mul_L[1] = L
        _lib.check(lib.stemgnn_cheb_fwd(mul_L.data_ptr(), N, st), "cheb_fwd")
        torch.cuda.synchronize()
        return mul_L

    on, off = _both(monkeypatch, run)
    assert torch.equal(on, off)
    Ld = L.double()
    T2 = 2 * Ld @ Ld
    e2, e3 = relerr(on[2], T2), relerr(on[3], 2 * Ld @ on[2].double() - Ld)
    print(f"cheb_fwd N={N}: T2 {e2:.2e} T3 {e3:.2e}")
    assert e2 < 1e-5 and e3 < 1e-5


@pytest.mark.parametrize("N", NS)
def test_cheb_bwd(N, monkeypatch):
    from stemgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N + 1)
    mul_L = (torch.randn(4, N, N, generator=g) / N ** 0.5).to(dev)
    dmul_L = torch.randn(4, N, N, generator=g).to(dev)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        dL = torch.zeros(N, N, device=dev)
        scratch = torch.zeros(2, N, N, device=dev)
        _lib.check(lib.stemgnn_cheb_bwd(mul_L.data_ptr(), dmul_L.data_ptr(), dL.data_ptr(), scratch.data_ptr(), N, st), "cheb_bwd")
        torch.cuda.synchronize()
        return dL, scratch

    (dL_on, s_on), (dL_off, s_off) = _both(monkeypatch, run)
    assert torch.equal(s_on, s_off) and torch.equal(dL_on, dL_off)
    L, T2 = mul_L[1].double(), mul_L[2].double()
    dT1, dT2, dT3 = dmul_L[1].double(), dmul_L[2].double(), dmul_L[3].double()
    dLp = dT1 - dT3 + 2 * dT3 @ T2.T
    dT2p = dT2 + 2 * L.T @ dT3
    dL = dLp + 2 * (dT2p @ L.T + L.T @ dT2p)
    errs = (relerr(s_on[0], dLp), relerr(s_on[1], dT2p), relerr(dL_on, dL))
    print(f"cheb_bwd N={N}: dLp {errs[0]:.2e} dT2p {errs[1]:.2e} dL {errs[2]:.2e}")
    assert max(errs) < 1e-5


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", NS)
def test_gft_fwd(N, layout, monkeypatch):
    from stemgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = BATCH[N]
    g = torch.Generator().manual_seed(N + 2)
    mul_L = (torch.randn(4, N, N, generator=g) / N ** 0.5).to(dev)
    x, (sb, sn, stt), xd = _x(layout, B, N, g, dev)
    st = torch.cuda.current_stream().cuda_stream

    def run():
        G = torch.zeros(B * N, 3 * W, device=dev)
        _lib.check(lib.stemgnn_gft_fwd(mul_L.data_ptr(), x.data_ptr(), sb, sn, stt, G.data_ptr(), B, N, W, st), "gft_fwd")
        torch.cuda.synchronize()
        return G

    on, off = _both(monkeypatch, run)
    assert torch.equal(on, off)
    ref = torch.einsum("knm,bmt->bnkt", mul_L[1:].double(), xd).reshape(B * N, 3 * W)
    e = relerr(on, ref)
    print(f"gft_fwd N={N} {layout}: {e:.2e}")
    assert e < 2e-6


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("N", NS)
def test_gft_bwd(N, layout, monkeypatch):
    from stemgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = BATCH[N]
    g = torch.Generator().manual_seed(N + 3)
    mul_L = (torch.randn(4, N, N, generator=g) / N ** 0.5).to(dev)
    x, (sb, sn, stt), xd = _x(layout, B, N, g, dev)
    dG = (torch.randn(2, B * N, 3 * W, generator=g) * 0.1).to(dev)          # two partial slabs
    st = torch.cuda.current_stream().cuda_stream

    def run():
        dX = torch.zeros(B, N, W, device=dev)
        dmul_L = torch.zeros(4, N, N, device=dev)
        _lib.check(lib.stemgnn_gft_bwd(mul_L.data_ptr(), x.data_ptr(), sb, sn, stt, dG.data_ptr(), dX.data_ptr(), dmul_L.data_ptr(),
                                       0, B, N, W, st), "gft_bwd")
        torch.cuda.synchronize()
        return dX, dmul_L

    (dX_on, dT_on), (dX_off, dT_off) = _both(monkeypatch, run)
    assert torch.equal(dX_on, dX_off) and torch.equal(dT_on, dT_off)
    dsum = (dG[0] + dG[1]).double().view(B, N, 3, W)
    ex = relerr(dX_on, torch.einsum("knm,bnkt->bmt", mul_L[1:].double(), dsum))
    et = relerr(dT_on[1:], torch.einsum("bnkt,bmt->knm", dsum, xd))
    print(f"gft_bwd N={N} {layout}: dX {ex:.2e} dT {et:.2e}")
    assert ex < 2e-6 and et < 2e-6


@pytest.mark.parametrize("layouts", [("bwn", "bnw"), ("bnw", "bwn"), ("bwn", "bwn"), ("bnw", "bnw")])
@pytest.mark.parametrize("N", NS)
def test_gft_bwd_dt2(N, layouts, monkeypatch):
    from stemgnn_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    B = BATCH[N]
    g = torch.Generator().manual_seed(N + 4)
    xs = [_x(lay, B, N, g, dev) for lay in layouts]
    dG = [(torch.randn(2, B * N, 3 * W, generator=g) * 0.1).to(dev) for _ in range(2)]
    st = torch.cuda.current_stream().cuda_stream

    def run():
        dmul_L = torch.zeros(4, N, N, device=dev)
        (x0, s0, _), (x1, s1, _) = xs
        _lib.check(lib.stemgnn_gft_bwd_dt2(x0.data_ptr(), *s0, dG[0].data_ptr(), x1.data_ptr(), *s1, dG[1].data_ptr(),
                                           dmul_L.data_ptr(), B, N, W, st), "dt2")
        torch.cuda.synchronize()
        return dmul_L

    on, off = _both(monkeypatch, run)
    assert torch.equal(on, off)
    ref = torch.zeros(3, N, N, dtype=torch.float64, device=dev)
    for (_, _, xd), d in zip(xs, dG):
        ref += torch.einsum("bnkt,bmt->knm", (d[0] + d[1]).double().view(B, N, 3, W), xd)
    e = relerr(on[1:], ref)
    print(f"gft_bwd_dt2 N={N} {layouts}: {e:.2e}")
    assert bool((on[0] == 0).all()) and e < 2e-6
