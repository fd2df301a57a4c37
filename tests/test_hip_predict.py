"""GPU: the inference forward (Model.predict, engine.ForecastStep, trainer.rolling_forecast_graph) against the training
forward in eval mode -- bit for bit -- and against the reference's golden eval-mode forecast."""
import numpy as np
import pytest
import torch

from oracle import stemgnn_oracle as O
from tests.util import hash_seed, load_golden, relerr, synthetic_series

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _model(N, W, multi, H, seed=1, train=False, dropout=0.5):
    from stemgnn_amd import Model

    model = Model(N, 2, W, multi, horizon=H, dropout_rate=dropout)
    model.load_state_dict(O.det_state_dict(N, W, multi, H, seed=seed))
    return model.to(DEV).train(train)


def _check_equal(N, W, multi, H, B, seed=1):
    model = _model(N, W, multi, H, seed=seed)
    torch.manual_seed(seed)
    x = torch.randn(B, W, N, device=DEV)
    f_p, a_p = model.predict(x)
    with torch.no_grad():
        f_r, a_r = model(x)
    torch.cuda.synchronize()
    from stemgnn_amd.ops import check_gru_status
    check_gru_status(DEV)
    assert f_p.shape == (B, H, N) and a_p.shape == (N, N)
    assert torch.equal(f_p, f_r), relerr(f_p, f_r)
    assert torch.equal(a_p, a_r), relerr(a_p, a_r)


@pytest.mark.parametrize("dtype", ["f32", "bf16x2"])
@pytest.mark.parametrize("N,W,multi,H,B", [(228, 12, 5, 3, 32),      # PEMS07: cluster4 GRU, fused GLU and heads
                                           (25, 28, 5, 28, 8)])      # COVID: per-layer GLU fallback
def test_predict_equals_eval_forward(N, W, multi, H, B, dtype, monkeypatch):
    monkeypatch.setenv("STEMGNN_DTYPE", dtype)
    _check_equal(N, W, multi, H, B)


@pytest.mark.parametrize("N,W,multi,H,B", [(140, 12, 5, 3, 16),      # ECG
                                           (2048, 48, 2, 3, 2)])     # wide GRU, per-layer GLU (KF = 400: fused heads)
def test_predict_equals_eval_forward_more_shapes(N, W, multi, H, B):
    _check_equal(N, W, multi, H, B)


@pytest.mark.parametrize("dtype", ["f32", "bf16x2"])
@pytest.mark.parametrize("N,W,multi,H,B", [(40, 64, 3, 8, 4),        # KF = 784 > 640: per-stage inference heads, long K
                                           (7, 64, 9, 4, 2)])        # per-stage heads forward and backward
def test_predict_equals_eval_forward_per_stage_heads(N, W, multi, H, B, dtype, monkeypatch):
    """The per-stage heads of the inference forward keep ig / fs in branch 0's ping-pong slabs of the workspace
    (stemgnn_igft_heads_fwd_infer); the training forward keeps them in the saved activations."""
    from stemgnn_amd import _lib

    assert not _lib.load().stemgnn_block_paths(B, N, W, multi, 0) & _lib.SG_PATH["heads_fwd_fused"]
    monkeypatch.setenv("STEMGNN_DTYPE", dtype)
    _check_equal(N, W, multi, H, B)


@pytest.mark.parametrize("cluster", ["2", "1", "0"])
@pytest.mark.parametrize("B,S,W", [(32, 228, 12), (5, 33, 7), (3, 140, 12), (2, 300, 4), (9, 358, 12), (1, 64, 3), (4, 307, 12)])
def test_predict_equals_eval_forward_gru_forms(B, S, W, cluster, monkeypatch):
    """The GRU shapes and cluster switches of test_gru_fwd_bwd_vs_torch_cpu: every forward form of the recurrence."""
    monkeypatch.setenv("STEMGNN_GRU_CLUSTER", cluster)
    _check_equal(S, W, 2, 2, B, seed=S + B)


def test_predict_golden_eval():
    name = "tiny_eval_h1"
    z, cfg = load_golden(name)
    model = _model(cfg["N"], cfg["W"], cfg["multi"], cfg["H"], seed=hash_seed(name), dropout=0.0)
    f, a = model.predict(torch.from_numpy(z["x"]).to(DEV))
    assert relerr(f, z["forecast"]) < 1e-4
    assert relerr(a, z["attention"]) < 1e-4


def test_predict_no_grad_state_and_memory():
    N, W, multi, H, B = 228, 12, 5, 3, 32
    model = _model(N, W, multi, H, train=True)
    torch.manual_seed(0)
    x = torch.randn(B, W, N, device=DEV)
    f, a = model.predict(x)                       # also warms the lazy per-device state (tables, status words)
    assert f.grad_fn is None and a.grad_fn is None and not f.requires_grad
    assert model.training
    with torch.enable_grad():
        f2, _ = model.predict(x)
    assert f2.grad_fn is None and model.training

    def peak(fn):
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        rise = torch.cuda.max_memory_allocated() - before
        del out
        return rise

    model.eval()
    with torch.no_grad():
        model(x)
        p_fwd = peak(lambda: model(x))
    model.train()
    p_pred = peak(lambda: model.predict(x))
    assert p_pred <= 0.4 * p_fwd, (p_pred, p_fwd)


def _dataset(T, N, W, H):
    from stemgnn_amd.forecast_dataloader import ForecastDataset

    return ForecastDataset(synthetic_series(T, N, seed=5), W, H, normalize_method="z_score", device=DEV)


def test_forecast_step_equals_rolling_forecast():
    from stemgnn_amd.forecast_dataloader import WindowLoader
    from stemgnn_amd.trainer import rolling_forecast, rolling_forecast_graph, score_forecast

    N, W, multi, H, B, horizon = 40, 12, 3, 3, 8, 7          # three rounds per batch; 12 + 7 + ... -> ragged last batch
    model = _model(N, W, multi, H, train=True)
    ds = _dataset(12 + 7 + 8 * 5 + 3, N, W, horizon)
    assert len(ds) % B != 0 and len(ds) > 2 * B
    f_ref, t_ref = rolling_forecast(model, WindowLoader(ds, batch_size=B), horizon)
    model.train()
    f_g, t_g = rolling_forecast_graph(model, ds, horizon, B)
    torch.cuda.synchronize()
    assert model.training
    assert f_g.shape == f_ref.shape == (len(ds), horizon, N)
    assert torch.equal(t_g, t_ref)
    assert torch.equal(f_g, f_ref), relerr(f_g, f_ref)
    s_ref = score_forecast(f_ref, t_ref)
    s_g = score_forecast(f_g, t_g)
    assert s_ref.keys() == s_g.keys()
    for k in s_ref:
        assert np.array_equal(np.asarray(s_ref[k]), np.asarray(s_g[k]), equal_nan=True), k


def _train_with(interleave):
    """6 TrainStep replays (queue mode, graph, FusedRMSprop) after the eager first step; with `interleave`, a predict and a
    ForecastStep pass after replays 2 and 4."""
    from stemgnn_amd import ops
    from stemgnn_amd.engine import ForecastStep, TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    N, W, multi, H, B, T = 48, 12, 3, 3, 8, 120
    torch.manual_seed(0)
    model = _model(N, W, multi, H, train=True)
    model.set_dropout_seed(99)
    opt = FusedRMSprop(model.parameters(), lr=1e-3, eps=1e-8)
    g = torch.Generator().manual_seed(7)
    series = torch.randn(T, N, generator=g).to(DEV)
    total = 7
    hi = (torch.randint(0, T - W - H, (total * B,), generator=g) + W).to(DEV)
    step = TrainStep(model, opt, B, W, H, N, series=series, order_capacity=total * B, schedule_check=False)
    step.load_order(hi)
    fs = ForecastStep(model, B, W, H, series, order_capacity=3 * B + 3) if interleave else None
    losses = []
    for i in range(total):
        step.run_next()
        losses.append(float(step.loss))
        if interleave and i in (2, 4):
            model.predict(series[None, :W].contiguous())
            fs.load_order(hi[:3 * B + 3])
            while fs.remaining:
                fs.run_next()
            fs.result()[0].sum().item()
    torch.cuda.synchronize()
    ops.check_gru_status(DEV)
    ops.check_gather_status(DEV)
    assert step.mode.startswith("hipgraph"), step.mode
    return opt.flat_p.clone(), losses


def test_predict_between_train_steps_leaves_training_unchanged():
    p_plain, l_plain = _train_with(False)
    p_mix, l_mix = _train_with(True)
    assert l_plain == l_mix
    assert torch.equal(p_plain, p_mix)
