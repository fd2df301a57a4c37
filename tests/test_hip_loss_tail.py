"""GPU: the fused training tail with a choice of loss (MSE / MAE / Huber) and missing-value masking (csrc/tail.hip, the
`_loss` entries of include/stemgnn_hip.h) against an fp64 restatement, against the entries it was templated from, and the
valid-target count kernel."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests.util import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DELTA = 0.5
KINDS = ("mse", "mae", "huber")
# the smallest shapes that reach every branch of the 32-row, 8-threads-per-row kernel: smallest case | fewer rows than one block |
# ragged last block, H = 1 | H and W beyond the 8-thread stride | range limit | PEMS07
SHAPES = [(1, 1, 1, 1), (2, 7, 5, 2), (5, 33, 12, 1), (3, 50, 28, 28), (2, 7, 64, 32), (32, 228, 12, 3)]
TOL = 1e-5              # the bound test_fc_tail_fwd_bwd_vs_torch uses for these kernels


def fc64(fsum, w0, b0, w2, b2):
    """fc tail in the tensors' dtype: (pre-activations z [B,N,W], forecast [B,H,N])."""
    z = fsum @ w0.T + b0
    a = torch.where(z > 0, z, 0.01 * z)
    return z, (a @ w2.T + b2).permute(0, 2, 1).contiguous()


def loss64(f, y, kind, ignore_nan):
    """The issue's semantics restated in torch: sum of l(f - y) over the valid targets / their count (B H N unmasked)."""
    valid = ~torch.isnan(y) if ignore_nan else torch.ones_like(y, dtype=torch.bool)
    d = torch.where(valid, f - torch.where(valid, y, torch.zeros_like(y)), torch.zeros_like(f))
    if kind == "mse":
        ell = d * d
    elif kind == "mae":
        ell = d.abs()
    else:
        ell = torch.where(d.abs() <= DELTA, 0.5 * d * d, DELTA * (d.abs() - 0.5 * DELTA))
    ell = torch.where(valid, ell, torch.zeros_like(ell))
    cnt = int(valid.sum())
    return ell.sum() / cnt if cnt else ell.sum() * 0.0


@functools.lru_cache(maxsize=None)
def case(B, N, W, H):
    """Inputs (fp32, CPU), the fp64 forecast and the two targets of one shape, built once and left unchanged.
    Targets y = f64 - e with a random sign and |e| in [0.05, 0.4] u [0.6, 1.5] (delta = 0.5), so that no element sits within
    0.05 of the MAE kink at 0 or of the Huber kinks at +-delta: fp32 forecast error (~1e-6) cannot move an element across one
    and no element has to be excluded from a comparison.  The seed is the first whose fc pre-activations also keep clear
    of LeakyReLU's kink (|z| > 1e-5 in fp64), for the same reason."""
    for seed in itertools.count(1000 * B + 10 * N + H):
        g = torch.Generator().manual_seed(seed)
        fsum = torch.randn(B, N, W, generator=g)
        prm = [torch.randn(W, W, generator=g) * 0.3, torch.randn(W, generator=g) * 0.1,
               torch.randn(H, W, generator=g) * 0.3, torch.randn(H, generator=g) * 0.1]
        z64, f64 = fc64(fsum.double(), *(p.double() for p in prm))
        if float(z64.abs().min()) > 1e-5:
            break
    u = torch.rand(B, H, N, generator=g, dtype=torch.float64)
    mag = torch.where(u < 0.5, 0.0501 + (0.4 - 0.0501) * (u / 0.5), 0.6 + (1.5 - 0.6) * ((u - 0.5) / 0.5))
    sign = torch.where(torch.rand(B, H, N, generator=g) < 0.5, -1.0, 1.0).double()
    y = (f64 - sign * mag).float()
    d = (f64 - y.double()).abs()                                  # the band property, on the fp64 values
    assert float(d.min()) >= 0.05 and float((d - DELTA).abs().min()) >= 0.05 and float(d.max()) <= 1.5001
    # deterministic mask, ~30 % missing: scattered + one whole (b, h) plane + (B N >= 64) every target of rows 0..31, so that
    # one workgroup of the 32-row kernel has nothing valid
    miss = torch.rand(B, H, N, generator=g) < 0.3
    miss[B - 1, H - 1, :] = True
    if B * N >= 64:
        rows = torch.arange(B * N).reshape(B, 1, N).expand(B, H, N)
        miss |= rows < 32
    y_nan = y.clone()
    y_nan[miss] = float("nan")
    return dict(fsum=fsum, prm=prm, y=y, y_nan=y_nan, miss=miss)


@functools.lru_cache(maxsize=None)
def reference(B, N, W, H, kind, ignore_nan):
    """fp64 CPU: (loss, d fsum, four fc gradients) for an upstream gradient of 1."""
    c = case(B, N, W, H)
    fsum = c["fsum"].double().requires_grad_(True)
    prm = [p.double().requires_grad_(True) for p in c["prm"]]
    y = (c["y_nan"] if ignore_nan else c["y"]).double()
    loss = loss64(fc64(fsum, *prm)[1], y, kind, ignore_nan)
    grads = torch.autograd.grad(loss, [fsum] + prm)
    return loss.detach(), grads[0], list(grads[1:])


@pytest.mark.parametrize("ignore_nan", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("B,N,W,H", SHAPES)
def test_loss_kinds_and_masking_vs_fp64(B, N, W, H, kind, ignore_nan):
    from stemgnn_amd import ops
    c = case(B, N, W, H)
    ref_loss, ref_df, ref_g = reference(B, N, W, H, kind, ignore_nan)
    y = (c["y_nan"] if ignore_nan else c["y"]).to(DEV)
    everything_missing = ignore_nan and bool(c["miss"].all())
    assert everything_missing == (ignore_nan and (B, N, W, H) == (1, 1, 1, 1))
    for scale in (1.0, 2.5):
        f = c["fsum"].to(DEV).requires_grad_(True)
        ps = [p.to(DEV).requires_grad_(True) for p in c["prm"]]
        loss = ops.FcTailMse.apply(f, y, *ps, None, None, None, False, kind, DELTA if kind == "huber" else 0.0, ignore_nan)
        (scale * loss).backward()
        torch.cuda.synchronize()
        outs = [loss.detach(), f.grad] + [p.grad for p in ps]
        refs = [ref_loss, scale * ref_df] + [scale * g for g in ref_g]
        errs = [relerr(o, r) for o, r in zip(outs, refs)]
        print(f"{(B, N, W, H)} {kind} ignore_nan={ignore_nan} upstream {scale}: loss {float(loss.detach()):.6f} (fp64 {float(ref_loss):.6f}) "
              f"relerr loss/dfsum/dw0/db0/dw2/db2 = " + " ".join(f"{e:.1e}" for e in errs))
        for o in outs:
            assert bool(torch.isfinite(o).all())
        for e in errs:
            assert e < TOL, errs
        if everything_missing:
            assert float(ref_loss) == 0.0
            for o in outs:
                assert bool((o == 0).all()), o


def _tail_buffers(lib, B, N, W, H, prm, fsum):
    return dict(scratch=torch.empty(lib.stemgnn_fc_tail_train_scratch_floats(B, N, W, H), device=DEV),
                forecast=torch.zeros(B, H, N, device=DEV),
                loss=torch.zeros((), device=DEV), acc=torch.full((), 0.5, device=DEV, dtype=torch.float64),
                dfsum=torch.empty_like(fsum), dw0=torch.empty_like(prm[0]), db0=torch.empty_like(prm[1]),
                dw2=torch.empty_like(prm[2]), db2=torch.empty_like(prm[3]))


@pytest.mark.parametrize("B,N,W,H", SHAPES)
def test_unmasked_mse_loss_entry_is_the_old_entry(B, N, W, H):
    """stemgnn_fc_tail_train_loss(SG_LOSS_MSE, norm = NULL) is the same instantiation as stemgnn_fc_tail_train: every output
    bit for bit."""
    from stemgnn_amd import _lib
    lib = _lib.load()
    c = case(B, N, W, H)
    fsum, y = c["fsum"].to(DEV), c["y"].to(DEV)
    prm = [p.to(DEV) for p in c["prm"]]
    st = torch.cuda.current_stream().cuda_stream
    old, new = _tail_buffers(lib, B, N, W, H, prm, fsum), _tail_buffers(lib, B, N, W, H, prm, fsum)
    head = [fsum.data_ptr(), y.data_ptr()] + [p.data_ptr() for p in prm] + [B, N, W, H]

    def tail(b):
        return [b[k].data_ptr() for k in ("scratch", "forecast", "loss", "acc", "dfsum", "dw0", "db0", "dw2", "db2")] + [st]
    _lib.check(lib.stemgnn_fc_tail_train(*head, *tail(old)), "old entry")
    _lib.check(lib.stemgnn_fc_tail_train_loss(*head, _lib.SG_LOSS["mse"], 0.0, None, *tail(new)), "loss entry")
    torch.cuda.synchronize()
    for k in ("forecast", "loss", "acc", "dfsum", "dw0", "db0", "dw2", "db2"):
        assert torch.equal(old[k], new[k]), k
    assert float(old["loss"]) > 0


@pytest.mark.parametrize("B,N,W,H", [(5, 33, 12, 1), (3, 50, 28, 28), (32, 228, 12, 3)])
def test_rows_loss_then_finish_loss_equal_the_one_call(B, N, W, H):
    """(huber, masked): `_rows_loss` then `_finish_loss` on a side stream == the one call, bit for bit."""
    from stemgnn_amd import _lib, ops
    lib = _lib.load()
    c = case(B, N, W, H)
    fsum, y = c["fsum"].to(DEV), c["y_nan"].to(DEV)
    prm = [p.to(DEV) for p in c["prm"]]
    norm = ops.target_valid_count(y)
    st = torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    one, two = _tail_buffers(lib, B, N, W, H, prm, fsum), _tail_buffers(lib, B, N, W, H, prm, fsum)
    head = [fsum.data_ptr(), y.data_ptr()] + [p.data_ptr() for p in prm] + [B, N, W, H, _lib.SG_LOSS["huber"], DELTA,
                                                                           norm.data_ptr()]
    grads = ("dw0", "db0", "dw2", "db2")
    _lib.check(lib.stemgnn_fc_tail_train_loss(*head, one["scratch"].data_ptr(), one["forecast"].data_ptr(), one["loss"].data_ptr(),
                                              one["acc"].data_ptr(), one["dfsum"].data_ptr(), *(one[k].data_ptr() for k in grads),
                                              st), "one call")
    _lib.check(lib.stemgnn_fc_tail_train_rows_loss(*head, two["scratch"].data_ptr(), two["forecast"].data_ptr(),
                                                   two["dfsum"].data_ptr(), st), "rows")
    side.wait_stream(torch.cuda.current_stream())
    _lib.check(lib.stemgnn_fc_tail_train_finish_loss(two["scratch"].data_ptr(), B, N, W, H, norm.data_ptr(), two["loss"].data_ptr(),
                                                     two["acc"].data_ptr(), *(two[k].data_ptr() for k in grads),
                                                     side.cuda_stream), "finish")
    torch.cuda.synchronize()
    for k in ("forecast", "loss", "acc", "dfsum") + grads:
        assert torch.equal(one[k], two[k]), k
    ref_loss = reference(B, N, W, H, "huber", True)[0]
    assert abs(float(one["loss"]) - float(ref_loss)) < TOL * float(ref_loss)
    assert abs(float(one["acc"]) - 0.5 - float(one["loss"])) < 1e-6


@pytest.mark.parametrize("pattern", ["none", "all", "random"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 21888, 100003])
def test_target_valid_count(n, pattern):
    """norm = {count, float32(1 / count)} (0, 0 when nothing is valid), whatever the buffer held before."""
    from stemgnn_amd import _lib
    lib = _lib.load()
    g = torch.Generator().manual_seed(n)
    y = torch.randn(n, generator=g)
    y[::7] = float("inf")                                          # +-inf is a value, not a missing one
    if pattern == "all":
        y[:] = float("nan")
    elif pattern == "random":
        y[torch.rand(n, generator=g) < 0.3] = float("nan")
    count = int((~torch.isnan(y)).sum())
    norm = torch.tensor([float("nan"), -7.5e30], device=DEV)       # garbage
    y_dev = y.to(DEV)
    _lib.check(lib.stemgnn_target_valid_count(y_dev.data_ptr(), n, norm.data_ptr(), torch.cuda.current_stream().cuda_stream),
               "target_valid_count")
    got = norm.cpu().numpy()
    assert got[0] == np.float32(count)
    assert got[1] == (np.float32(1.0 / np.float64(count)) if count else np.float32(0.0))
    if pattern == "all":
        assert got.tolist() == [0.0, 0.0]
    if pattern == "none":
        assert count == n
