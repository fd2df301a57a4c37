"""GPU: the model run from a frozen or user-supplied graph (``adjacency=``) -- no GRU, no attention.

Bit-identity of ``predict(x, adjacency=latent_graph(x))`` with ``predict(x)``; a free adjacency (forward, two losses, every
gradient including x's and the adjacency's own) against an fp64 composition of the oracle's functions; batch independence;
``average_graph``; the captured inference and training steps against their eager forms.

SHAPES (N, W, multi, H, B) are the smallest that reach each branch of the kernels involved: one ragged 32 x 32 Laplacian
tile with H = 1; one row short of a full tile; a second tile holding one row; the first N past the register-resident
(N <= 256) branch of the Laplacian backward / degree kernels and past the single-workgroup front.  Tolerance: BASELINE's
1e-4 norm-relative against fp64.  At the seeds used, the oracle evaluated in fp32 is itself within 1e-5 of fp64 in every
compared quantity (worst 7.8e-6, checked on the CPU when the seeds were fixed), so the instances are well conditioned."""
import pytest
import torch
import torch.nn.functional as F

from oracle import stemgnn_oracle as O
from tests.util import kink_audit, relerr, synthetic_series

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = torch.device("cuda:0")
SHAPES = [(5, 4, 1, 1, 1), (31, 12, 5, 3, 1), (33, 12, 5, 3, 3), (257, 12, 2, 3, 2)]
DELTA = 0.7             # Huber delta: inside the spread of the residuals, so both branches of the loss are taken
_FRONT = ("GRU.weight_ih_l0", "GRU.weight_hh_l0", "GRU.bias_ih_l0", "GRU.bias_hh_l0", "weight_key", "weight_query")


def case_data(case):
    """Weights, inputs, targets (one copy with NaNs) and a random non-negative, asymmetric adjacency whose row sums are
    positive (uniform + a small floor) for one shape; seeds derived from the shape."""
    N, W, multi, H, B = case
    sd = O.det_state_dict(N, W, multi, H, seed=N + 3 * W + 7 * multi + B)
    g = torch.Generator().manual_seed(N * 7 + B * 131 + W)
    x, y = torch.randn(B, W, N, generator=g), torch.randn(B, H, N, generator=g)
    A = torch.rand(N, N, generator=g) + 0.05
    y_nan = y.clone()
    y_nan.view(-1)[torch.randperm(y.numel(), generator=g)[:max(1, y.numel() // 5)]] = float("nan")
    return sd, x, y, y_nan, A


def oracle_forward(x, A, sd, fc_kink_pos=None):
    """The reference from the point behind the batch mean (models/base_model.py:141-148, 169-179) for a given A [N,N]:
    composed from the oracle's own functions.  Returns (forecast [B,H,N], attention, fc tail pre-activation z)."""
    L, A_s = O.laplacian_from_attention(A[None])
    mul_L = O.cheb_polynomial(L)
    X = x.unsqueeze(1).permute(0, 1, 3, 2)
    f0, X1 = O.stock_block(X, mul_L, sd, 0)
    f1, _ = O.stock_block(X1, mul_L, sd, 1)
    z = F.linear(f0 + f1, sd["fc.0.weight"], sd["fc.0.bias"])                       # the fc lines of O.model_forward
    v = F.leaky_relu(z, 0.01) if fc_kink_pos is None else torch.where(fc_kink_pos, z, 0.01 * z)
    v = F.linear(v, sd["fc.2.weight"], sd["fc.2.bias"])
    forecast = v.unsqueeze(1).squeeze(-1) if v.shape[-1] == 1 else v.permute(0, 2, 1).contiguous()
    return forecast, A_s, z


def oracle_loss(forecast, target, kind):
    if kind == "mse":
        return F.mse_loss(forecast, target)
    valid = ~torch.isnan(target)                                                    # huber over the valid targets
    return F.huber_loss(forecast[valid], target[valid], delta=DELTA)


def oracle_run(case, kind, dtype=torch.float64, fc_kink_pos=None):
    """loss, forecast, attention, z and the gradients of every parameter, of x and of A, in `dtype`."""
    sd, x, y, y_nan, A = case_data(case)
    leaves = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    xl, Al = x.to(dtype).requires_grad_(True), A.to(dtype).requires_grad_(True)
    forecast, att, z = oracle_forward(xl, Al, leaves, fc_kink_pos)
    loss = oracle_loss(forecast, (y if kind == "mse" else y_nan).to(dtype), kind)
    keys = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[k] for k in keys] + [xl, Al], allow_unused=True)
    out = dict(zip(keys, grads[:-2]))
    out["x"], out["A"] = grads[-2], grads[-1]
    return loss.detach(), forecast.detach(), att.detach(), z.detach(), out


def _model(case, train=True, dropout=0.5):
    from stemgnn_amd import Model

    N, W, multi, H, B = case
    model = Model(N, 2, W, multi, horizon=H, dropout_rate=dropout)
    model.load_state_dict(case_data(case)[0])
    return model.to(DEV).train(train)


# ---- 1. bit-identity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype,spectral", [(c, "f32", "cheb") for c in SHAPES] +
                         [(SHAPES[2], "bf16x2", "cheb"), (SHAPES[3], "f32", "eig")])
def test_predict_from_latent_graph_has_the_bits_of_predict(case, dtype, spectral, monkeypatch):
    from stemgnn_amd import LatentGraph, ops

    monkeypatch.setenv("STEMGNN_DTYPE", dtype)
    monkeypatch.setenv("STEMGNN_SPECTRAL", spectral)
    model = _model(case)
    x = case_data(case)[1].to(DEV)
    f_ref, a_ref = model.predict(x)
    G = model.latent_graph(x)
    assert isinstance(G, LatentGraph) and G.A.shape == (case[0], case[0]) and G.degree.shape == (case[0],)
    f, a = model.predict(x, adjacency=G)
    torch.cuda.synchronize()
    ops.check_gru_status(DEV)
    if spectral == "eig":
        ops.check_eigh_status(DEV)
    assert torch.equal(a, a_ref), relerr(a, a_ref)
    assert torch.equal(f, f_ref), relerr(f, f_ref)
    assert model.training and f.grad_fn is None
    # the basis is cached per spectral route and dropped when A is replaced
    assert G.mul_L is G.mul_L
    G.A = G.A.clone()
    f2, _ = model.predict(x, adjacency=G)
    assert torch.equal(f2, f_ref)


# ---- 2. prior graph: forward and backward against fp64 ---------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "huber_nan"])
@pytest.mark.parametrize("case", SHAPES)
def test_free_adjacency_matches_fp64(case, kind):
    N, W, multi, H, B = case
    sd, x, y, y_nan, A = case_data(case)
    o_loss, o_forecast, o_att, z64, o_grads = oracle_run(case, kind)
    model = _model(case)
    xd, Ad = x.to(DEV).requires_grad_(True), A.to(DEV).requires_grad_(True)
    yd = (y if kind == "mse" else y_nan).to(DEV)
    if kind == "mse":
        loss = model.loss(xd, yd, adjacency=Ad)
    else:
        loss = model.loss(xd, yd, kind="huber", huber_delta=DELTA, ignore_nan=True, adjacency=Ad)
    loss.backward()
    with torch.no_grad():
        forecast, att = model(xd, adjacency=Ad)
        z = F.linear(model.graph_path(xd, Ad)[0], model.fc[0].weight, model.fc[0].bias).cpu()
    torch.cuda.synchronize()
    assert forecast.shape == o_forecast.shape == (B, H, N)
    errs = {"forecast": relerr(forecast, o_forecast), "attention": relerr(att, o_att),
            "loss": abs(float(loss.detach()) - float(o_loss)) / abs(float(o_loss))}
    # the fc tail's LeakyReLU kink, audited as in tests/test_hip_shape_domain.py
    ez = float((z.double() - z64).abs().max())
    assert relerr(z, z64) < 2e-5, relerr(z, z64)
    flips = kink_audit(z > 0, z64, ez, "fc tail pre-activations")
    g_ref = o_grads
    if int(flips.sum()):
        g_ref = oracle_run(case, kind, fc_kink_pos=torch.where(flips, z > 0, z64 > 0))[4]
    for k, p in model.named_parameters():
        if k in _FRONT:
            assert p.grad is None and g_ref[k] is None, k          # the front takes no part
        elif g_ref[k] is None:
            assert p.grad is None, k
        else:
            assert p.grad is not None, k
            errs["grad." + k] = relerr(p.grad, g_ref[k])
    errs["grad.x"] = relerr(xd.grad, g_ref["x"])
    errs["grad.A"] = relerr(Ad.grad, g_ref["A"])
    worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{case} {kind}: worst norm-relative error {worst[1]:.2e} ({worst[0]}); grad.A {errs['grad.A']:.2e} grad.x {errs['grad.x']:.2e}")
    bad = [(k, f"{e:.2e}") for k, e in errs.items() if not e < TOL]
    assert not bad, bad


# ---- 3. a gradient for the attention alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", [SHAPES[2], SHAPES[3]])
def test_attention_gradient_alone(case):
    sd, x, y, y_nan, A = case_data(case)
    model = _model(case)
    xd, Ad = x.to(DEV).requires_grad_(True), A.to(DEV).requires_grad_(True)
    forecast, att = model(xd, adjacency=Ad)
    assert torch.equal(att, 0.5 * (Ad.detach() + Ad.detach().T))
    att.sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(Ad.grad, torch.ones_like(Ad))               # (G + G^T) / 2 with G = 1
    assert xd.grad is None
    assert all(p.grad is None for p in model.parameters())


# ---- 4. batch independence -----------------------------------------------------------------------------------------------
def test_frozen_graph_makes_the_forecast_batch_independent():
    case = N, W, multi, H, B = SHAPES[2]
    # seeds chosen (on the CPU, among 60 x 5) so that the property is not an accident of the instance: on the reference's own
    # path (fp64 oracle) window 0's forecast moves by 7.0e-3 with the company it keeps; at most seeds the softmax is close
    # to uniform and the batch mean changes little
    sd = O.det_state_dict(N, W, multi, H, seed=15)
    x = torch.randn(B, W, N, generator=torch.Generator().manual_seed(5))
    sd64 = {k: v.double() for k, v in sd.items()}
    alone, batch = O.model_forward(x[:1].double(), sd64)[0], O.model_forward(x.double(), sd64)[0][:1]
    assert relerr(alone, batch) > 1e-3, relerr(alone, batch)
    model = _model(case, train=False)
    model.load_state_dict(sd)
    xd = x.to(DEV)
    assert relerr(model.predict(xd[:1])[0], model.predict(xd)[0][:1]) > 1e-3
    G = model.latent_graph(xd)
    f_alone, _ = model.predict(xd[:1].contiguous(), adjacency=G)
    f_batch, _ = model.predict(xd, adjacency=G)
    torch.cuda.synchronize()
    assert relerr(f_alone, f_batch[:1]) < TOL, relerr(f_alone, f_batch[:1])


# ---- 5. average_graph -----------------------------------------------------------------------------------------------------
def test_average_graph_is_the_fp64_weighted_mean():
    case = SHAPES[2]
    N, W = case[0], case[1]
    model = _model(case)
    g = torch.Generator().manual_seed(11)
    batches = [torch.randn(b, W, N, generator=g).to(DEV) for b in (3, 3, 1)]
    G = model.average_graph(batches)
    G2 = model.average_graph((xb, None) for xb in batches)          # loader-style items; a second run
    flat = lambda q: torch.cat([q.A.reshape(-1), q.degree]).cpu()   # noqa: E731
    parts = [flat(model.latent_graph(xb)).double() for xb in batches]
    expect = ((3.0 * parts[0] + 3.0 * parts[1] + 1.0 * parts[2]) / 7.0).float()
    torch.cuda.synchronize()
    assert torch.equal(flat(G), expect), relerr(flat(G), expect)
    assert torch.equal(flat(G), flat(G2))
    assert not torch.equal(flat(G), parts[0].float())


# ---- 6. ForecastStep ---------------------------------------------------------------------------------------------------------
def test_forecast_step_with_adjacency_equals_rolling_forecast():
    from stemgnn_amd.forecast_dataloader import ForecastDataset, WindowLoader
    from stemgnn_amd.trainer import rolling_forecast, rolling_forecast_graph

    N, W, multi, H, B, horizon = 33, 12, 5, 3, 4, 7                # horizon > H: three rounds, the window rolls
    case = (N, W, multi, H, 3)
    model = _model(case)
    ds = ForecastDataset(synthetic_series(W + horizon + 4 * 2 + 1, N, seed=5), W, horizon, normalize_method="z_score", device=DEV)
    assert len(ds) % B != 0 and len(ds) > 2 * B
    G = model.latent_graph(ds.data[None, :W].contiguous())
    f_ref, t_ref = rolling_forecast(model, WindowLoader(ds, batch_size=B), horizon, adjacency=G)
    model.train()
    f_g, t_g = rolling_forecast_graph(model, ds, horizon, B, adjacency=G)
    torch.cuda.synchronize()
    assert f_g.shape == f_ref.shape == (len(ds), horizon, N)
    assert torch.equal(t_g, t_ref)
    assert torch.equal(f_g, f_ref), relerr(f_g, f_ref)
    # and it is the frozen graph that was used: the default pass gives another forecast
    f_def, _ = rolling_forecast_graph(model, ds, horizon, B)
    assert not torch.equal(f_def, f_g)


# ---- 7. TrainStep ------------------------------------------------------------------------------------------------------------
def _stepper(case, graph, adjacency_of=None):
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    N, W, multi, H, B = case
    model = _model(case)
    model.set_dropout_seed(99)
    opt = FusedRMSprop(model.parameters(), lr=1e-3, eps=1e-8)
    kw = {} if adjacency_of is None else dict(adjacency=adjacency_of(model))
    step = TrainStep(model, opt, B, W, H, N, graph=graph, schedule_check=False, **kw)
    return model, opt, step


def test_train_step_with_adjacency_captured_equals_eager_and_leaves_no_thunk():
    from stemgnn_amd import LatentGraph

    case = SHAPES[2]
    sd, x, y, y_nan, A = case_data(case)
    xd, yd = x.to(DEV), y.to(DEV)
    make = lambda model: LatentGraph.from_adjacency(A.to(DEV))     # noqa: E731
    out = {}
    for graph in (False, True):
        model, opt, step = _stepper(case, graph, make)
        assert step.state.direct and step.state.overlap            # direct + overlap mode, FusedRMSprop
        p0 = opt.flat_p.clone()
        step.run_batch(xd, yd)                                     # eager first step (arms the capture)
        step.run_batch(xd, yd)                                     # graph=True: a replay
        torch.cuda.synchronize()
        assert step.mode.startswith("hipgraph") == graph, step.mode
        assert step.state.tail_finish is None and step.state.prepacked is None and step.state.pending is None
        assert step.state.exact_group is None
        out[graph] = (opt.flat_p.clone(), float(step.loss), model, opt, step, p0)
    assert out[True][1] == out[False][1] and out[True][1] > 0
    assert torch.equal(out[True][0], out[False][0])
    model, opt, step, p0 = out[True][2:]
    # the front's parameters took no step (weight decay off)
    for k, p in model.named_parameters():
        off = opt.bucket.offset_of(p)
        moved = not torch.equal(opt.flat_p[off:off + p.numel()], p0[off:off + p.numel()])
        unused = k in ("stock_block.1.backcast_short_cut.weight", "stock_block.1.backcast_short_cut.bias")
        assert moved == (k not in _FRONT and not unused), k
    # a default step on the model that took the adjacency path == the same step on a model that never did
    ref_model, ref_opt, ref_step = _stepper(case, False)
    ref_step.run_batch(xd, yd)
    again_model, again_opt, again_step = _stepper(case, False, make)
    again_step.run_batch(xd, yd)
    again_opt.flat_p.copy_(p0)
    again_opt.square_avg.zero_()
    from stemgnn_amd.engine import TrainStep
    plain = TrainStep(again_model, again_opt, case[4], case[1], case[3], case[0], graph=False, schedule_check=False)
    plain.run_batch(xd, yd)
    torch.cuda.synchronize()
    assert float(plain.loss) == float(ref_step.loss)
    assert torch.equal(again_opt.flat_p, ref_opt.flat_p)
    assert plain.state.tail_finish is None


# ---- the failures the default path states, stated the same way -----------------------------------------------------------
@pytest.mark.parametrize("stack_cnt,exc", [(1, IndexError), (3, AttributeError)])
def test_stack_count_failures_as_on_the_default_path(stack_cnt, exc):
    from stemgnn_amd import Model

    m = Model(6, stack_cnt, 4, 2, horizon=2).to(DEV)
    x, A = torch.randn(2, 4, 6, device=DEV), torch.rand(6, 6, device=DEV) + 0.1
    for call in (lambda: m(x, adjacency=A), lambda: m.predict(x, adjacency=A), lambda: m.loss(x, x[:, :2], adjacency=A)):
        with pytest.raises(exc):
            call()


def test_adjacency_of_another_size_is_refused():
    from stemgnn_amd._lib import StemGNNHipError

    model = _model(SHAPES[0])
    x = case_data(SHAPES[0])[1].to(DEV)
    for call in (lambda: model(x, adjacency=torch.rand(7, 7, device=DEV)), lambda: model.predict(x, adjacency=torch.rand(7, 7, device=DEV))):
        with pytest.raises(StemGNNHipError, match="nodes"):
            call()
