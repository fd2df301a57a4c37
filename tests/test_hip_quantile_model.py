"""GPU: the quantile head of Model end to end -- the same bits as the plain model of Q * H outputs, Model.loss(kind="pinball")
against the fp64 oracle, the captured TrainStep(loss="pinball") against the eager one, and a short DeviceTrainer run with the
rolling forecast and the calibration metrics."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import stemgnn_oracle as O
from tests.test_hip_input_grad import _kink_overrides
from tests.test_hip_quantile_tail import pinball64, place_targets
from tests.util import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4                      # BASELINE.json's bar for the model against the fp64 oracle
TAUS = (0.1, 0.5, 0.9)


def _pair(seed=3):
    """The quantile model (H = 3, Q = 3) and the plain horizon-9 model on the oracle's deterministic horizon-9 weights."""
    from stemgnn_amd import Model
    N, W, multi = 11, 12, 5
    sd = O.det_state_dict(N, W, multi, 9, seed=seed)
    quant = Model(N, 2, W, multi, horizon=3, dropout_rate=0.0, quantiles=TAUS)
    plain = Model(N, 2, W, multi, horizon=9, dropout_rate=0.0)
    quant.load_state_dict(sd)
    plain.load_state_dict(sd)
    return quant.to(DEV), plain.to(DEV), sd


def test_quantile_model_has_the_bits_of_the_wide_plain_model():
    quant, plain, _ = _pair()
    x = torch.randn(3, 12, 11, generator=torch.Generator().manual_seed(5)).to(DEV)
    quant.eval(), plain.eval()
    with torch.no_grad():
        fq, aq = quant(x)
        fp, ap = plain(x)
    pq, paq = quant.predict(x)
    torch.cuda.synchronize()
    assert tuple(fq.shape) == (3, 3, 3, 11) and tuple(pq.shape) == (3, 3, 3, 11)
    assert torch.equal(fq.reshape(3, 9, 11), fp) and torch.equal(aq, ap)
    assert torch.equal(pq, fq) and torch.equal(paq, aq)
    G = quant.latent_graph(x)
    pg, _ = quant.predict(x, adjacency=G)
    assert tuple(pg.shape) == (3, 3, 3, 11) and torch.equal(pg, pq)
    # a user-written loss on the forecast back-propagates through the existing fc tail backward
    quant.train()
    xg = x.clone().requires_grad_(True)
    quant(xg)[0][:, quant.point_index].square().mean().backward()
    torch.cuda.synchronize()
    assert xg.grad is not None and bool(torch.isfinite(xg.grad).all()) and float(xg.grad.abs().max()) > 0
    assert float(quant.fc[2].weight.grad[:3].abs().max()) == 0.0 and float(quant.fc[2].weight.grad[3:6].abs().max()) > 0


def _oracle_pinball(x, y, sd, over, ignore_nan, frozen_graph):
    """fp64: gru_front + hot_path of the oracle, the fc tail and the pinball loss restated here.  frozen_graph: the spectral basis
    is a constant (Model.loss(..., adjacency=model.latent_graph(x))): block 0 and 1 run on the detached mul_L, so the GRU, key and
    query get no gradient and x gets its gradient through block 0 alone."""
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    if frozen_graph:
        with torch.no_grad():
            mul_L = O.hot_path(O.gru_front(x64, leaves), x64, leaves, kink_pos=over.get("kink_pos"))[2]
        f0, X1 = O.stock_block(x64.unsqueeze(1).permute(0, 1, 3, 2), mul_L, leaves, 0)
        fsum = f0 + O.stock_block(X1, mul_L, leaves, 1)[0]
    else:
        fsum = O.hot_path(O.gru_front(x64, leaves), x64, leaves, kink_pos=over.get("kink_pos"))[0]
    z = F.linear(fsum, leaves["fc.0.weight"], leaves["fc.0.bias"])
    a = F.leaky_relu(z, 0.01) if "fc_kink_pos" not in over else torch.where(over["fc_kink_pos"], z, 0.01 * z)
    f = F.linear(a, leaves["fc.2.weight"], leaves["fc.2.bias"]).permute(0, 2, 1)       # [B,Q*H,N]
    loss = pinball64(f, y.double(), TAUS, ignore_nan)
    keys = list(leaves)
    grads = torch.autograd.grad(loss, [x64] + [leaves[k] for k in keys], allow_unused=True)
    return loss.detach(), grads[0], dict(zip(keys, grads[1:])), f.detach()


@pytest.mark.parametrize("variant", ["plain", "ignore_nan", "adjacency"])
def test_pinball_loss_and_gradients_vs_fp64(variant):
    quant, _, sd = _pair(seed=7)
    quant.train()
    g = torch.Generator().manual_seed(21)
    x = torch.randn(3, 12, 11, generator=g)
    xd = x.to(DEV).requires_grad_(True)
    over = _kink_overrides(quant, xd, x, sd, "cpu", {})
    frozen = variant == "adjacency"
    f64 = _oracle_pinball(x, torch.zeros(3, 3, 11), sd, over, False, frozen)[3]
    y = place_targets(f64, len(TAUS), g)                       # asserts min_q |f64_q - y| >= 0.05, on the CPU
    if variant == "ignore_nan":
        y[torch.rand(y.shape, generator=g) < 0.3] = float("nan")
    ref_loss, ref_dx, ref_g, _ = _oracle_pinball(x, y, sd, over, variant == "ignore_nan", frozen)
    kw = dict(ignore_nan=True) if variant == "ignore_nan" else {}
    if frozen:
        kw["adjacency"] = quant.latent_graph(xd.detach())
    loss = quant.loss(xd, y.to(DEV), kind="pinball", **kw)
    loss.backward()
    torch.cuda.synchronize()
    errs = {"loss": relerr(loss.detach(), ref_loss), "x.grad": relerr(xd.grad, ref_dx)}
    for k, p in quant.named_parameters():
        if ref_g[k] is None or float(ref_g[k].abs().max()) == 0.0:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
        else:
            assert p.grad is not None, k
            errs["grad." + k] = relerr(p.grad, ref_g[k])
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{variant}: loss {float(loss.detach()):.6f} (fp64 {float(ref_loss):.6f}); {len(errs)} comparisons, worst {worst[0]} = {worst[1]:.2e}")
    if frozen:
        assert all(ref_g[k] is None for k in ref_g if k.startswith("GRU.") or k.startswith("weight_"))
    assert all(np.isfinite(e) for e in errs.values()), errs
    assert worst[1] < TOL, errs


def _stepper(graph, series=None, **kw):
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop
    N, W, multi, H, B = 16, 8, 2, 2, 6
    torch.manual_seed(1234)
    model = Model(N, 2, W, multi, horizon=H, quantiles=TAUS).to(DEV)
    model.set_dropout_seed(99)
    opt = FusedRMSprop(model.parameters(), lr=1e-3, eps=1e-8)
    step = TrainStep(model, opt, B, W, H, N, series=series, graph=graph, schedule_check=False, loss="pinball", **kw)
    return model, opt, step


def test_captured_pinball_step_equals_the_eager_one():
    g = torch.Generator().manual_seed(8)
    batches = [(torch.randn(6, 8, 16, generator=g).to(DEV), torch.randn(6, 2, 16, generator=g).to(DEV)) for _ in range(3)]
    trace = {}
    for graph in (False, True):
        model, opt, step = _stepper(graph)
        assert tuple(step.y.shape) == (6, 2, 16)                    # the step's target stays [B,H,N]
        assert step.state.direct and step.state.overlap
        trace[graph] = []
        for x, y in batches:
            step.run_batch(x, y)
            torch.cuda.synchronize()
            trace[graph].append((opt.flat_p.clone(), step.loss.clone()))
        assert step.mode.startswith("hipgraph") == graph, step.mode
        assert step.state.tail_finish is None
    for i, ((pe, le), (pg, lg)) in enumerate(zip(trace[False], trace[True])):
        assert torch.equal(le, lg) and float(le) > 0, (i, float(le), float(lg))
        assert torch.equal(pe, pg), i
    assert not torch.equal(trace[True][0][0], trace[True][2][0])
    # the loss of step 1 is Model.loss on that batch (same initial weights, same dropout key)
    model, _, _ = _stepper(False)
    model.train()
    with torch.no_grad():
        ref = float(model.loss(*batches[0], kind="pinball"))
    got = float(trace[True][0][1])
    print(f"step 1: loss {got:.7f}, Model.loss {ref:.7f}")
    assert abs(got - ref) <= 1e-6 * abs(ref)


def test_captured_pinball_step_with_missing_targets_from_a_target_series():
    g = torch.Generator().manual_seed(9)
    series = torch.randn(60, 16, generator=g)
    target_series = series.clone()
    target_series[torch.rand(series.shape, generator=g) < 0.3] = float("nan")
    series, target_series = series.to(DEV), target_series.to(DEV)
    his = [torch.randint(8, 58, (6,), generator=g).to(DEV) for _ in range(3)]
    trace = {}
    for graph in (False, True):
        model, opt, step = _stepper(graph, series=series, ignore_nan=True, target_series=target_series)
        trace[graph] = []
        for hi in his:
            step.run_indices(hi)
            torch.cuda.synchronize()
            assert bool(torch.isnan(step.y).any()) and not bool(torch.isnan(step.x).any())
            trace[graph].append((opt.flat_p.clone(), step.loss.clone()))
        assert step.mode.startswith("hipgraph") == graph, step.mode
    for i, ((pe, le), (pg, lg)) in enumerate(zip(trace[False], trace[True])):
        assert torch.equal(le, lg) and float(le) > 0 and bool(torch.isfinite(pe).all()), (i, float(le), float(lg))
        assert torch.equal(pe, pg), i


def test_train_step_refuses_a_loss_that_does_not_fit_the_model():
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop
    for quantiles, loss in ((None, "pinball"), (TAUS, "mse")):
        model = Model(16, 2, 8, 2, horizon=2, quantiles=quantiles).to(DEV)
        with pytest.raises(ValueError, match="pinball"):
            TrainStep(model, FusedRMSprop(model.parameters(), lr=1e-3), 6, 8, 2, 16, loss=loss)


def test_short_training_run_with_rolling_forecast_and_calibration():
    from stemgnn_amd.engine import ForecastStep
    from stemgnn_amd.forecast_dataloader import ForecastDataset, WindowLoader
    from stemgnn_amd.trainer import DeviceTrainer, rolling_forecast, rolling_forecast_graph, score_forecast
    rng = np.random.default_rng(2024)
    T, N = 400, 16
    t = np.arange(T, dtype=np.float64)[:, None]
    series = np.sin(2 * np.pi * t / rng.uniform(8.0, 30.0, N) + rng.uniform(0.0, 6.28, N)) * rng.uniform(0.5, 3.0, N) \
        + rng.uniform(-2.0, 8.0, N) + 0.3 * rng.normal(size=(T, N))
    torch.manual_seed(77)
    trainer = DeviceTrainer(16, 8, 2, 2, quantiles=TAUS, batch_size=16)
    assert trainer.loss == "pinball" and trainer.model.quantiles == TAUS
    lines = []
    metrics, statistic = trainer.fit(series[:300], series[300:], 2, log=lines.append)
    print("\n".join(lines))
    assert any("quantiles: pinball" in ln for ln in lines)
    new = ("pinball", "pinball_q", "coverage_q", "interval_coverage", "interval_width", "interval_nominal", "crossing")
    for k in ("mae", "mape", "rmse", "mae_node", "mape_node", "rmse_node", "mae_norm", "mape_norm", "rmse_norm") + new:
        assert k in metrics and bool(np.isfinite(np.asarray(metrics[k], dtype=np.float64)).all()), k
    assert len(metrics["pinball_q"]) == 3 and len(metrics["coverage_q"]) == 3 and len(metrics["interval_coverage"]) == 1
    assert abs(float(metrics["interval_nominal"][0]) - 0.8) < 1e-12
    print("coverage against nominal: " + ", ".join(f"{t_:g} -> {c:.3f}" for t_, c in zip(TAUS, metrics["coverage_q"]))
          + f"; 10-90 % band {float(metrics['interval_coverage'][0]):.3f} of 0.8, crossing {metrics['crossing']:.3f}")
    ds = ForecastDataset(series[300:], window_size=8, horizon=2, normalize_method="z_score", norm_statistic=statistic, device=DEV)
    forecast, target = rolling_forecast(trainer.model, WindowLoader(ds, batch_size=16), 2)
    assert tuple(forecast.shape) == (len(ds), 3, 2, 16) and tuple(target.shape) == (len(ds), 2, 16)
    again = score_forecast(forecast, target, "z_score", statistic, quantiles=TAUS)
    assert again["mae"] == metrics["mae"] and again["pinball"] == metrics["pinball"]
    point = score_forecast(forecast[:, trainer.model.point_index].contiguous(), target, "z_score", statistic)
    assert all(np.array_equal(np.asarray(point[k]), np.asarray(again[k])) for k in point)      # the 3-D path, unchanged
    # beyond the model's own horizon the point row is what rolls: [count, Q, 5, N], the first round's rows unchanged
    ds5 = ForecastDataset(series[300:], window_size=8, horizon=5, normalize_method="z_score", norm_statistic=statistic, device=DEV)
    f5, t5 = rolling_forecast(trainer.model, WindowLoader(ds5, batch_size=16), 5)
    assert tuple(f5.shape) == (len(ds5), 3, 5, 16) and bool(torch.isfinite(f5).all())
    assert torch.equal(f5[:16, :, :2], forecast[:16])
    with pytest.raises(ValueError, match="quantile model"):
        ForecastStep(trainer.model, 16, 8, 2, ds.data, len(ds))
    with pytest.raises(ValueError, match="quantile model"):
        rolling_forecast_graph(trainer.model, ds, 2, 16)
