"""GPU: the loss options through the model and the step driver -- Model.loss(kind, huber_delta, ignore_nan) against the fp64
oracle, engine.TrainStep(loss, ignore_nan, target_series) eager / captured / queue, and the default step unchanged."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import stemgnn_oracle as O
from tests.test_hip_loss_tail import DELTA, KINDS, loss64
from tests.util import GOLDEN_DIR, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4              # norm-relative, the project's bar for the model against the fp64 oracle


@functools.lru_cache(maxsize=None)
def oracle_case(N, W, multi, H, B):
    """The reference's own initialisation (tests/golden/ref_init: the constructor regenerates it from the seed), its input
    window, the fp64 oracle forecast and targets y = forecast - e by the band construction of tests/test_hip_loss_tail.py
    (|e| in [0.05, 0.4] u [0.6, 1.5], delta = 0.5), ~30 % of them missing incl. one whole (b, h) plane."""
    from stemgnn_amd import Model
    z = np.load(os.path.join(GOLDEN_DIR, "ref_init", f"n{N}_w{W}_m{multi}_h{H}_b{B}.npz"))
    torch.manual_seed(123)
    sd = {k: v.detach().clone() for k, v in Model(N, 2, W, multi, horizon=H, dropout_rate=0.0).state_dict().items()}
    x = torch.from_numpy(z["x"])
    with torch.no_grad():
        f64, _ = O.model_forward(x.double(), {k: v.double() for k, v in sd.items()})
    g = torch.Generator().manual_seed(N * 100 + H)
    u = torch.rand(B, H, N, generator=g, dtype=torch.float64)
    mag = torch.where(u < 0.5, 0.0501 + (0.4 - 0.0501) * (u / 0.5), 0.6 + (1.5 - 0.6) * ((u - 0.5) / 0.5))
    sign = torch.where(torch.rand(B, H, N, generator=g) < 0.5, -1.0, 1.0).double()
    y = (f64 - sign * mag).float()
    d = (f64 - y.double()).abs()
    assert float(d.min()) >= 0.05 and float((d - DELTA).abs().min()) >= 0.05
    miss = torch.rand(B, H, N, generator=g) < 0.3
    miss[B - 1, H - 1, :] = True
    y[miss] = float("nan")
    return sd, x, y


@functools.lru_cache(maxsize=None)
def oracle_grads(N, W, multi, H, B, kind):
    sd, x, y = oracle_case(N, W, multi, H, B)
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    f, _ = O.model_forward(x64, leaves)
    loss = loss64(f, y.double(), kind, True)
    keys = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in keys] + [x64], allow_unused=True)
    return loss.detach(), dict(zip(keys, grads[:-1])), grads[-1]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("N,W,multi,H,B", [(11, 12, 5, 3, 3), (16, 8, 2, 1, 6)])
def test_model_loss_masked_vs_fp64_oracle(N, W, multi, H, B, kind):
    from stemgnn_amd import Model, ops
    sd, x, y = oracle_case(N, W, multi, H, B)
    ref_loss, ref_grads, ref_xgrad = oracle_grads(N, W, multi, H, B, kind)
    model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0)
    model.load_state_dict(sd)
    model.to(DEV).train()
    xd = x.to(DEV).requires_grad_(True)
    loss = model.loss(xd, y.to(DEV), kind=kind, huber_delta=DELTA, ignore_nan=True)
    loss.backward()
    torch.cuda.synchronize()
    ops.check_gru_status(DEV)
    loss = loss.detach()
    errs = {"loss": abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)), "x.grad": relerr(xd.grad, ref_xgrad)}
    for k, p in model.named_parameters():
        if ref_grads[k] is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            errs["grad." + k] = relerr(p.grad, ref_grads[k])
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{(N, W, multi, H, B)} {kind}: loss {float(loss):.6f} (fp64 {float(ref_loss):.6f}), worst relerr {worst[0]} = {worst[1]:.2e}")
    assert bool(torch.isfinite(xd.grad).all()) and all(bool(torch.isfinite(p.grad).all()) for p in model.parameters()
                                                       if p.grad is not None)
    assert worst[1] < TOL, errs


def _step_setup():
    N, W, H, multi, B, T = 20, 12, 3, 5, 4, 120
    g = torch.Generator().manual_seed(11)
    series = torch.randn(T, N, generator=g)
    target = series.clone()
    target[torch.rand(T, N, generator=g) < 0.2] = float("nan")
    hi = torch.randint(0, T - W - H, (6, B), generator=g) + W
    return (N, W, H, multi, B, T), series.to(DEV), target.to(DEV), hi.to(DEV)


def _run_steps(series, hi, dims, graph=True, queue=False, **kw):
    from stemgnn_amd import Model, ops
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop
    N, W, H, multi, B, T = dims
    torch.manual_seed(7)
    model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0).to(DEV).train()
    opt = FusedRMSprop(model.parameters(), lr=1e-3)
    step = TrainStep(model, opt, B, W, H, N, series=series, graph=graph, order_capacity=hi.numel() if queue else 0, **kw)
    if queue:
        step.load_order(hi)
        for _ in range(hi.shape[0]):
            step.run_next()
    else:
        for i in range(hi.shape[0]):
            step.run_indices(hi[i])
    torch.cuda.synchronize()
    ops.check_gather_status(DEV)                          # the gather status is clean
    ops.check_gru_status(DEV)
    return step, opt.flat_p.clone(), float(step.epoch_loss_sum())


def test_train_step_huber_masked_eager_graph_and_queue_agree():
    dims, series, target, hi = _step_setup()
    kw = dict(loss="huber", huber_delta=DELTA, ignore_nan=True, target_series=target)
    step_g, p_graph, l_graph = _run_steps(series, hi, dims, graph=True, **kw)
    step_e, p_eager, l_eager = _run_steps(series, hi, dims, graph=False, **kw)
    step_q, p_queue, l_queue = _run_steps(series, hi, dims, graph=True, queue=True, **kw)
    assert step_g.mode.startswith("hipgraph") and step_q.mode.startswith("hipgraph"), (step_g.mode, step_q.mode)
    assert step_e.mode == "eager"
    for p in (p_graph, p_eager, p_queue):
        assert bool(torch.isfinite(p).all())
    assert np.isfinite(l_graph) and l_graph > 0
    print(f"graph vs eager parameters relerr {relerr(p_graph, p_eager):.2e}; loss sums {l_graph} {l_eager} {l_queue}")
    assert relerr(p_graph, p_eager) < 1e-6
    assert torch.equal(p_queue, p_graph) and l_queue == l_graph
    assert bool(torch.isnan(step_g.y).any())              # the targets really came from target_series


def test_default_train_step_is_unchanged_by_spelling_the_defaults():
    dims, series, _, hi = _step_setup()
    _, p_default, l_default = _run_steps(series, hi, dims, graph=True)
    _, p_spelled, l_spelled = _run_steps(series, hi, dims, graph=True, loss="mse", ignore_nan=False, target_series=None)
    assert torch.equal(p_default, p_spelled) and l_default == l_spelled
