"""GPU: the fused training tail of a quantile head (pinball loss over Q * H rows against the [B,H,N] target; csrc/tail.hip, the
`_quantile` entries of include/stemgnn_hip.h) against an fp64 restatement, against its own rows + finish pair and against the MAE
entry it must reduce to at Q = 1, tau = 0.5; the quantile window shift and the calibration metrics of csrc/data.hip."""
import functools
import itertools

import numpy as np
import pytest
import torch

from tests.helpers.data_ref import scores64
from tests.test_hip_loss_tail import TOL, fc64
from tests.test_hip_loss_tail import case as mae_case
from tests.util import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, N, W, H, Q): smallest case | fewer rows than one 32-row block | ragged last block, H = 1, Q beyond the eight-thread stride |
# Q H = 28, j % H and j / H both non-trivial | both range limits | PEMS07
SHAPES = [(1, 1, 1, 1, 1), (2, 7, 5, 2, 3), (5, 33, 12, 1, 9), (3, 50, 28, 4, 7), (2, 7, 64, 8, 4), (32, 228, 12, 3, 3)]
BAND = 0.05


def levels(Q):
    """Q levels evenly spaced in (0, 1)."""
    return tuple((q + 1) / (Q + 1) for q in range(Q))


def pinball64(f, y, taus, ignore_nan):
    """The issue's semantics restated in torch: f [B,Q*H,N] (row q * H + h), y [B,H,N]; the mean over B Q H N of
    max(tau (y - f), (tau - 1) (y - f)), a NaN target missing for all Q of its rows (normaliser: valid targets * Q)."""
    B, H, N = y.shape
    Q = len(taus)
    f = f.reshape(B, Q, H, N)
    valid = (~torch.isnan(y) if ignore_nan else torch.ones_like(y, dtype=torch.bool)).unsqueeze(1).expand(B, Q, H, N)
    yb = torch.where(valid, y.unsqueeze(1).expand(B, Q, H, N), torch.zeros_like(f))
    tau = torch.tensor(taus, dtype=f.dtype).reshape(1, Q, 1, 1)
    d = torch.where(valid, f - yb, torch.zeros_like(f))
    ell = torch.where(valid, torch.where(d >= 0, (1 - tau) * d, -tau * d), torch.zeros_like(f))
    cnt = int(valid.sum())
    return ell.sum() / cnt if cnt else ell.sum() * 0.0


def place_targets(f64, Q, g):
    """f64 [B,Q*H,N] (fp64 forecasts, row q * H + h) -> fp32 targets [B,H,N] that keep clear of the pinball kink of all Q rows:
    per (b, h, n) one of  lowest forecast - m | highest forecast + m | the midpoint of a gap between neighbouring (sorted)
    forecasts wider than 0.1,  drawn at random, m in [0.0501, 1.5].  Asserts min_q |f64_q - y| >= 0.05 on what it returns."""
    B, QH, N = f64.shape
    H = QH // Q
    fq = f64.reshape(B, Q, H, N).permute(0, 2, 3, 1)                       # [B,H,N,Q]
    s = fq.sort(dim=-1).values
    m = 0.0501 + (1.5 - 0.0501) * torch.rand(B, H, N, generator=g, dtype=torch.float64)
    cand = torch.cat([(s[..., :1] - m.unsqueeze(-1)), (s[..., -1:] + m.unsqueeze(-1)), 0.5 * (s[..., 1:] + s[..., :-1])], dim=-1)
    ok = torch.cat([torch.ones(B, H, N, 2, dtype=torch.bool), (s[..., 1:] - s[..., :-1]) > 0.1], dim=-1)
    score = torch.where(ok, torch.rand(B, H, N, Q + 1, generator=g, dtype=torch.float64), torch.full_like(cand, -1.0))
    y = cand.gather(-1, score.argmax(dim=-1, keepdim=True)).squeeze(-1).float()
    dist = (fq - y.double().unsqueeze(-1)).abs().min()
    assert float(dist) >= BAND, float(dist)
    return y


@functools.lru_cache(maxsize=None)
def case(B, N, W, H, Q):
    """Inputs (fp32, CPU) and the two targets of one shape, built once and left unchanged.  The seed is the first whose fc
    pre-activations keep clear of LeakyReLU's kink (|z| > 1e-5 in fp64).  Every target keeps clear of the pinball kink of all Q of
    its rows: per (b, h, n), y is drawn among  lowest forecast - m | highest forecast + m | the midpoint of any gap between
    neighbouring (sorted) forecasts wider than 0.1,  m in [0.0501, 1.5] -- asserted below on the fp64 forecasts and the fp32 target:
    min_q |f64_q - y| >= 0.05, so fp32 forecast error (~1e-6) moves no element across a kink and none is excluded anywhere."""
    for seed in itertools.count(1000 * B + 10 * N + H + 100 * Q):
        g = torch.Generator().manual_seed(seed)
        fsum = torch.randn(B, N, W, generator=g)
        prm = [torch.randn(W, W, generator=g) * 0.3, torch.randn(W, generator=g) * 0.1,
               torch.randn(Q * H, W, generator=g) * 0.3, torch.randn(Q * H, generator=g) * 0.1]
        z64, f64 = fc64(fsum.double(), *(p.double() for p in prm))
        if float(z64.abs().min()) > 1e-5:
            break
    y = place_targets(f64, Q, g)
    # deterministic mask, ~30 % missing: scattered + one whole (b, h) plane + (B N >= 64) every target of rows 0..31, so that
    # one workgroup of the 32-row kernel has nothing valid; at (1,1,1,1,1) the plane is everything
    miss = torch.rand(B, H, N, generator=g) < 0.3
    miss[B - 1, H - 1, :] = True
    if B * N >= 64:
        rows = torch.arange(B * N).reshape(B, 1, N).expand(B, H, N)
        miss = miss | (rows < 32)
    y_nan = y.clone()
    y_nan[miss] = float("nan")
    return dict(fsum=fsum, prm=prm, y=y, y_nan=y_nan, miss=miss, taus=levels(Q))


@functools.lru_cache(maxsize=None)
def reference(B, N, W, H, Q, ignore_nan):
    """fp64 CPU: (loss, d fsum, four fc gradients) for an upstream gradient of 1."""
    c = case(B, N, W, H, Q)
    fsum = c["fsum"].double().requires_grad_(True)
    prm = [p.double().requires_grad_(True) for p in c["prm"]]
    y = (c["y_nan"] if ignore_nan else c["y"]).double()
    loss = pinball64(fc64(fsum, *prm)[1], y, c["taus"], ignore_nan)
    grads = torch.autograd.grad(loss, [fsum] + prm)
    return loss.detach(), grads[0], list(grads[1:])


@pytest.mark.parametrize("ignore_nan", [False, True])
@pytest.mark.parametrize("B,N,W,H,Q", SHAPES)
def test_pinball_tail_vs_fp64(B, N, W, H, Q, ignore_nan):
    c = case(B, N, W, H, Q)
    ref_loss, ref_df, ref_g = reference(B, N, W, H, Q, ignore_nan)         # on the CPU, before anything runs on the GPU
    from stemgnn_amd import ops
    y = (c["y_nan"] if ignore_nan else c["y"]).to(DEV)
    everything_missing = ignore_nan and bool(c["miss"].all())
    assert everything_missing == (ignore_nan and (B, N, W, H, Q) == (1, 1, 1, 1, 1))
    for scale in (1.0, 2.5):
        f = c["fsum"].to(DEV).requires_grad_(True)
        ps = [p.to(DEV).requires_grad_(True) for p in c["prm"]]
        loss = ops.FcTailQuantile.apply(f, y, *ps, None, None, None, False, c["taus"], ignore_nan)
        (scale * loss).backward()
        torch.cuda.synchronize()
        outs = [loss.detach(), f.grad] + [p.grad for p in ps]
        refs = [ref_loss, scale * ref_df] + [scale * g for g in ref_g]
        errs = [relerr(o, r) for o, r in zip(outs, refs)]
        print(f"{(B, N, W, H, Q)} ignore_nan={ignore_nan} upstream {scale}: loss {float(loss.detach()):.6f} (fp64 {float(ref_loss):.6f}) "
              f"relerr loss/dfsum/dw0/db0/dw2/db2 = " + " ".join(f"{e:.1e}" for e in errs))
        for o in outs:
            assert bool(torch.isfinite(o).all())
        for e in errs:
            assert e < TOL, errs
        if everything_missing:
            assert float(ref_loss) == 0.0
            for o in outs:
                assert bool((o == 0).all()), o


def _tail_buffers(lib, B, N, W, rows, prm, fsum):
    return dict(scratch=torch.empty(lib.stemgnn_fc_tail_train_scratch_floats(B, N, W, rows), device=DEV),
                forecast=torch.zeros(B, rows, N, device=DEV),
                loss=torch.zeros((), device=DEV), acc=torch.full((), 0.5, device=DEV, dtype=torch.float64),
                dfsum=torch.empty_like(fsum), dw0=torch.empty_like(prm[0]), db0=torch.empty_like(prm[1]),
                dw2=torch.empty_like(prm[2]), db2=torch.empty_like(prm[3]))


GRADS = ("dw0", "db0", "dw2", "db2")


@pytest.mark.parametrize("ignore_nan", [False, True])
@pytest.mark.parametrize("B,N,W,H,Q", SHAPES)
def test_rows_then_finish_equal_the_one_call(B, N, W, H, Q, ignore_nan):
    """`_rows_quantile` then `_finish_quantile` on a side stream == the one call, bit for bit; accum receives += loss; the
    forecast the tail writes is the fp64 one."""
    c = case(B, N, W, H, Q)
    ref_loss = reference(B, N, W, H, Q, ignore_nan)[0]
    from stemgnn_amd import _lib, ops
    lib = _lib.load()
    fsum, y = c["fsum"].to(DEV), (c["y_nan"] if ignore_nan else c["y"]).to(DEV)
    prm = [p.to(DEV) for p in c["prm"]]
    norm = ops.target_valid_count(y) if ignore_nan else None
    norm_ptr = norm.data_ptr() if norm is not None else None
    tau = _lib.host_floats(c["taus"])
    st = torch.cuda.current_stream().cuda_stream
    side = torch.cuda.Stream()
    one, two = _tail_buffers(lib, B, N, W, Q * H, prm, fsum), _tail_buffers(lib, B, N, W, Q * H, prm, fsum)
    head = [fsum.data_ptr(), y.data_ptr()] + [p.data_ptr() for p in prm] + [B, N, W, H, Q, tau, norm_ptr]
    _lib.check(lib.stemgnn_fc_tail_train_quantile(*head, one["scratch"].data_ptr(), one["forecast"].data_ptr(),
                                                  one["loss"].data_ptr(), one["acc"].data_ptr(), one["dfsum"].data_ptr(),
                                                  *(one[k].data_ptr() for k in GRADS), st), "one call")
    _lib.check(lib.stemgnn_fc_tail_train_rows_quantile(*head, two["scratch"].data_ptr(), two["forecast"].data_ptr(),
                                                       two["dfsum"].data_ptr(), st), "rows")
    side.wait_stream(torch.cuda.current_stream())
    _lib.check(lib.stemgnn_fc_tail_train_finish_quantile(two["scratch"].data_ptr(), B, N, W, H, Q, norm_ptr, two["loss"].data_ptr(),
                                                         two["acc"].data_ptr(), *(two[k].data_ptr() for k in GRADS),
                                                         side.cuda_stream), "finish")
    torch.cuda.synchronize()
    for k in ("forecast", "loss", "acc", "dfsum") + GRADS:
        assert torch.equal(one[k], two[k]), k
    assert abs(float(one["loss"]) - float(ref_loss)) <= TOL * float(ref_loss)
    assert abs(float(one["acc"]) - 0.5 - float(one["loss"])) < 1e-6
    f64 = fc64(c["fsum"].double(), *(p.double() for p in c["prm"]))[1]
    assert relerr(one["forecast"], f64) < TOL


@pytest.mark.parametrize("ignore_nan", [False, True])
@pytest.mark.parametrize("B,N,W,H", [(2, 7, 5, 2), (5, 33, 12, 1), (32, 228, 12, 3)])
def test_one_level_at_the_median_is_half_the_mae_entry(B, N, W, H, ignore_nan):
    """Replication identity: Q = 1, tau = 0.5 is 0.5 |d| -- every output is half of what the (already verified) MAE `_loss`
    entry gives on the same inputs."""
    from stemgnn_amd import _lib, ops
    lib = _lib.load()
    c = mae_case(B, N, W, H)
    fsum, y = c["fsum"].to(DEV), (c["y_nan"] if ignore_nan else c["y"]).to(DEV)
    prm = [p.to(DEV) for p in c["prm"]]
    norm = ops.target_valid_count(y) if ignore_nan else None
    norm_ptr = norm.data_ptr() if norm is not None else None
    st = torch.cuda.current_stream().cuda_stream
    mae, pin = _tail_buffers(lib, B, N, W, H, prm, fsum), _tail_buffers(lib, B, N, W, H, prm, fsum)
    head = [fsum.data_ptr(), y.data_ptr()] + [p.data_ptr() for p in prm] + [B, N, W, H]

    def tail(b):
        return [b[k].data_ptr() for k in ("scratch", "forecast", "loss", "acc", "dfsum") + GRADS] + [st]
    _lib.check(lib.stemgnn_fc_tail_train_loss(*head, _lib.SG_LOSS["mae"], 0.0, norm_ptr, *tail(mae)), "mae entry")
    _lib.check(lib.stemgnn_fc_tail_train_quantile(*head, 1, _lib.host_floats((0.5,)), norm_ptr, *tail(pin)), "pinball entry")
    torch.cuda.synchronize()
    assert torch.equal(mae["forecast"], pin["forecast"])
    assert float(mae["loss"]) > 0
    for k in ("loss", "dfsum") + GRADS:
        e = relerr(pin[k], 0.5 * mae[k])
        print(f"{(B, N, W, H)} ignore_nan={ignore_nan} {k}: relerr against 0.5 x MAE {e:.1e}")
        assert e < 1e-6, (k, e)


@pytest.mark.parametrize("B,W,L,N,Q,horizon,steps", [(2, 5, 2, 7, 3, 5, (0, 2, 4)), (1, 1, 1, 1, 1, 1, (0,))])
def test_roll_window_quantile_is_the_indexing_it_stands_for(B, W, L, N, Q, horizon, steps):
    from stemgnn_amd import ops
    g = torch.Generator().manual_seed(17 * B + Q)
    inputs = torch.randn(B, W, N, generator=g).to(DEV)
    forecast = torch.randn(B, Q, L, N, generator=g).to(DEV)
    for point in sorted({0, Q // 2, Q - 1}):
        for step in steps:
            got_steps = torch.full((B, Q, horizon, N), -7.25, device=DEV)
            want_steps = got_steps.clone()
            nxt = ops.roll_window_quantile(inputs, forecast, got_steps, step, horizon, point)
            take = min(horizon - step, L)
            want_steps[:, :, step:step + take] = forecast[:, :, :take]
            want = torch.cat([inputs[:, L:], forecast[:, point]], dim=1)
            torch.cuda.synchronize()
            assert torch.equal(nxt, want), (point, step)
            assert torch.equal(got_steps, want_steps), (point, step)


@functools.lru_cache(maxsize=None)
def metric_case(C, Q, H, N, with_nan):
    g = np.random.default_rng(100 * C + Q)
    t = g.normal(size=(C, H, N)).astype(np.float32)
    f = (t[:, None] + np.sort(g.normal(size=(C, Q, H, N)), axis=1)).astype(np.float32)
    if Q > 1:                                           # built to have crossings: about one element in ten swaps two levels
        swap = g.random(size=(C, H, N)) < 0.1
        a, b = f[:, 0].copy(), f[:, Q - 1].copy()
        f[:, 0], f[:, Q - 1] = np.where(swap, b, a), np.where(swap, a, b)
    if with_nan:
        t[g.random(size=t.shape) < 0.25] = np.nan
        t[:, H - 1, :] = np.nan                         # one whole step with nothing valid: NaN there, not elsewhere
    mul = g.uniform(0.5, 3.0, size=N)
    add = g.uniform(-2.0, 8.0, size=N)
    return t, f, mul, add


@pytest.mark.parametrize("with_nan", [False, True])
@pytest.mark.parametrize("denorm", [False, True])
@pytest.mark.parametrize("C,Q,H,N", [(70, 3, 3, 11), (1, 1, 1, 1)])
def test_quantile_scores_vs_numpy_fp64(C, Q, H, N, denorm, with_nan):
    from stemgnn_amd.math_utils import QuantileScores
    t, f, mul, add = metric_case(C, Q, H, N, with_nan)
    taus = levels(Q)
    m, a = (mul, add) if denorm else (None, None)
    ref = scores64(t, f, taus, m, a, ignore_nan=with_nan)
    tm, ta = (torch.from_numpy(mul), torch.from_numpy(add)) if denorm else (None, None)
    got = QuantileScores(torch.from_numpy(t).to(DEV), torch.from_numpy(f).to(DEV), taus, tm, ta, ignore_nan=with_nan)
    if not with_nan:                                    # nothing to leave out: the masked entry is the plain one
        again = QuantileScores(torch.from_numpy(t).to(DEV), torch.from_numpy(f).to(DEV), taus, tm, ta, ignore_nan=True)
        for k in ("pinball", "coverage", "interval_coverage", "interval_width", "crossing"):
            assert np.array_equal(getattr(again, k), getattr(got, k)) and \
                np.array_equal(getattr(again, k + "_step"), getattr(got, k + "_step")), k
    assert np.allclose(got.interval_nominal, [taus[Q - 1 - i] - taus[i] for i in range(Q // 2)], rtol=0, atol=0)
    for k in ("pinball", "interval_width"):             # sums of real numbers: the project's metric bound
        for g_, r_ in ((getattr(got, k), ref[k][0]), (getattr(got, k + "_step"), ref[k][1])):
            assert g_.shape == r_.shape, k
            assert np.array_equal(np.isnan(g_), np.isnan(r_)), k
            keep = ~np.isnan(r_)
            if keep.any():
                e = np.abs(g_[keep] - r_[keep]).max() / np.abs(r_[keep]).max()
                print(f"{(C, Q, H, N)} denorm={denorm} nan={with_nan} {k}: relerr {e:.1e}")
                assert e < 1e-12, (k, e)
    for k in ("coverage", "interval_coverage", "crossing"):      # counts over counts: the same fp64 quotient
        assert np.array_equal(np.asarray(getattr(got, k)), np.asarray(ref[k][0]), equal_nan=True), k
        assert np.array_equal(np.asarray(getattr(got, k + "_step")).reshape(ref[k][1].shape), ref[k][1], equal_nan=True), k
    if with_nan:
        assert np.isnan(got.pinball_step[:, H - 1]).all() and np.isnan(got.coverage_step[:, H - 1]).all()
        assert np.isnan(got.crossing_step[H - 1])
        if H > 1:
            assert np.isfinite(got.pinball).all() and np.isfinite(got.pinball_step[:, :H - 1]).all()
        else:
            assert np.isnan(got.pinball).all()
    elif Q > 1:
        assert 0.0 < float(got.crossing) < 0.5
