"""GPU: x.grad of the HIP backward -- the GRU's input projection (stemgnn_gru_input_grad behind the recurrence) plus block 0's
GFT adjoint and short-cut term (SpectralHotPath) -- against torch's CPU nn.GRU, the fp64 oracle and the real reference's
fixtures; invariance of everything else; frozen weights (the weights-off GRU backward, no weight-gradient launches)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import stemgnn_oracle as O
from tests.test_hip_shape_domain import EDGE_CASES, EIG_CASES, SEEDS
from tests.util import GOLDEN_DIR, hash_seed, kink_audit, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
GRU_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


# ---- 1. GRU level ---------------------------------------------------------------------------------------------------------
def _gru_case(B, S, W):
    torch.manual_seed(S + B)
    gru = torch.nn.GRU(W, S)
    x = torch.randn(B, W, S)
    dh = torch.randn(S, B, S)
    return gru, x, dh


def _hip_gru_x_grad(gru, x, dh, trainable=True):
    from stemgnn_amd.ops import GruFront, check_gru_status

    params = [getattr(gru, n).detach().clone().cuda().requires_grad_(trainable) for n in GRU_PARAMS]
    xd = x.cuda().requires_grad_(True)
    GruFront.apply(xd, *params).backward(dh.cuda())
    torch.cuda.synchronize()
    check_gru_status(torch.device(DEV))
    return xd.grad.clone(), [p.grad for p in params]


def _check_gru_x_grad(B, S, W, ref=None):
    gru, x, dh = _gru_case(B, S, W)
    if ref is None:
        xr = x.clone().requires_grad_(True)
        out, _ = gru(xr.permute(2, 0, 1).contiguous())
        out.backward(dh)
        ref = xr.grad
    g1, pg = _hip_gru_x_grad(gru, x, dh)
    assert all(g is not None for g in pg)
    assert relerr(g1, ref) < TOL, relerr(g1, ref)
    g2, _ = _hip_gru_x_grad(gru, x, dh)
    assert torch.equal(g1, g2), "x.grad differs from launch to launch"
    g3, pg3 = _hip_gru_x_grad(gru, x, dh, trainable=False)        # weights-off backward (stemgnn_gru_bwd_recur)
    assert all(g is None for g in pg3)
    assert torch.equal(g1, g3), float((g1 - g3).abs().max())


@pytest.mark.parametrize("cluster", ["2", "1", "0"])
@pytest.mark.parametrize("B,S,W", [(32, 228, 12), (5, 33, 7), (3, 140, 12), (2, 300, 4), (9, 358, 12), (1, 64, 3), (4, 307, 12)])
def test_gru_x_grad_vs_torch_cpu(B, S, W, cluster, monkeypatch):
    monkeypatch.setenv("STEMGNN_GRU_CLUSTER", cluster)
    _check_gru_x_grad(B, S, W)


@pytest.mark.parametrize("B,S,W", [(32, 358, 12), (3, 384, 5), (2, 330, 20), (5, 321, 16)])
def test_gru_x_grad_six_workgroup_cluster(B, S, W):
    _check_gru_x_grad(B, S, W)


def test_gru_x_grad_wide_cluster():
    """Hidden 1024 (csrc/gru_wide.h) against the fp64 GRU cell of the oracle, evaluated on the device."""
    B, S, W = 8, 1024, 12
    gru, x, dh = _gru_case(B, S, W)
    rp = [getattr(gru, n).detach().double().cuda() for n in GRU_PARAMS]
    x64 = x.double().cuda().requires_grad_(True)
    out = O.gru_manual(x64.permute(2, 0, 1), *rp)
    out.backward(dh.double().cuda())
    _check_gru_x_grad(B, S, W, ref=x64.grad)


# ---- 2. model level -------------------------------------------------------------------------------------------------------
def _model(N, W, multi, H, sd, p=0.0):
    from stemgnn_amd import Model

    model = Model(N, 2, W, multi, horizon=H, dropout_rate=p)
    model.load_state_dict(sd)
    return model.to(DEV)


def _oracle_x_grad(x, y, sd, where="cpu", use_loss=True, **kw):
    sd64 = {k: v.double().to(where) for k, v in sd.items()}
    x64 = x.double().to(where).requires_grad_(True)
    f, _ = O.model_forward(x64, sd64, **kw)
    out = F.mse_loss(f, y.double().to(where)) if use_loss else f.sum()
    return torch.autograd.grad(out, x64)[0].cpu()


def _kink_overrides(model, xd, x, sd, where, kw, seed=None):
    """tests/util.kink_audit on the attention logits and the fc tail's pre-activations; returns the kink_pos / fc_kink_pos
    overrides for the decisions the implementation took differently from fp64 (empty when none did)."""
    from stemgnn_amd import ops

    if seed is not None:
        model.set_dropout_seed(*seed)
    ops.capture_attention_state(True)
    try:
        with torch.no_grad():
            fsum = model.hot_path(xd)[0]
            z = F.linear(fsum, model.fc[0].weight, model.fc[0].bias).cpu()
        key, query = (t.cpu() for t in ops.last_attention_state(DEV))
    finally:
        ops.capture_attention_state(False)
    sd64 = {k: v.double().to(where) for k, v in sd.items()}
    x64 = x.double().to(where)
    inp64 = O.gru_front(x64, sd64).permute(0, 2, 1)
    key64 = torch.matmul(inp64, sd64["weight_key"]).squeeze(-1).cpu()
    query64 = torch.matmul(inp64, sd64["weight_query"]).squeeze(-1).cpu()
    del inp64
    ek, eq = float((key.double() - key64).abs().max()), float((query.double() - query64).abs().max())
    logit64 = key64.unsqueeze(2) + query64.unsqueeze(1)
    pos = (key.unsqueeze(2) + query.unsqueeze(1)) > 0
    flips = kink_audit(pos, logit64, ek + eq, "attention logits")
    hk = {k: v for k, v in kw.items() if k in ("drop_mask", "drop_p")}
    z64 = F.linear(O.hot_path(O.gru_front(x64, sd64), x64, sd64, **hk)[0], sd64["fc.0.weight"], sd64["fc.0.bias"]).cpu()
    fflips = kink_audit(z > 0, z64, float((z.double() - z64).abs().max()), "fc tail pre-activations")
    over = {}
    if int(flips.sum()):
        over["kink_pos"] = torch.where(flips, pos, logit64 > 0).to(where)
    if int(fflips.sum()):
        over["fc_kink_pos"] = torch.where(fflips, z > 0, z64 > 0).to(where)
    return over


def _check_model_x_grad(N, W, multi, H, B, sd, x, y, dtype="f32", spectral="cheb", monkeypatch=None, where="cpu", p=0.0,
                        use_loss_method=False, train=True):
    from stemgnn_amd import ops

    monkeypatch.setenv("STEMGNN_DTYPE", dtype)
    monkeypatch.setenv("STEMGNN_SPECTRAL", spectral)
    model = _model(N, W, multi, H, sd, p=p)
    model.train(train)
    kw, seed = {}, None
    if p > 0.0:
        seed = (424242, 17)
        model.set_dropout_seed(*seed)
        kw = dict(drop_mask=ops.dropout_mask(p, model._seed.clone(), B, N).to(where).double(), drop_p=p)
    xd = x.to(DEV).requires_grad_(True)
    if use_loss_method:
        model.loss(xd, y.to(DEV)).backward()
    else:
        f, _ = model(xd)
        F.mse_loss(f, y.to(DEV)).backward()
    torch.cuda.synchronize()
    ops.check_gru_status(DEV)
    g = xd.grad.detach().cpu()
    ref = _oracle_x_grad(x, y, sd, where, **kw)
    err = relerr(g, ref)
    if not err < TOL:
        # a LeakyReLU decision the fp32 run took on the other side of 0 moves x.grad with every other gradient upstream of it
        over = _kink_overrides(model, x.to(DEV), x, sd, where, kw, seed)
        if over:
            ref = _oracle_x_grad(x, y, sd, where, **kw, **over)
            print(f"kink flips: x.grad {err:.2e} against the un-overridden fp64 run, {relerr(g, ref):.2e} with the overrides")
            err = relerr(g, ref)
    print(f"{dtype} {spectral} {(N, W, multi, H, B)}: x.grad relerr {err:.2e}")
    assert err < TOL, err
    return g


GOLDEN = ["tiny_eval_h1", "small_train_p0", "odd_wm_train", "pems_shape_n20"]    # small_dropmask: test_train_mode_dropout


@pytest.mark.parametrize("name", GOLDEN)
def test_golden_x_grad(name, monkeypatch):
    z = np.load(os.path.join(GOLDEN_DIR, "input_grad", name + ".npz"))
    N, W, m, H, B, mode = (int(v) for v in z["cfg"])
    sd = O.det_state_dict(N, W, m, H, seed=hash_seed(name))
    x, y = torch.from_numpy(z["x"]), torch.from_numpy(z["y"])
    g = _check_model_x_grad(N, W, m, H, B, sd, x, y, monkeypatch=monkeypatch, train=mode != 0)
    assert relerr(g, z["x_grad"]) < TOL, relerr(g, z["x_grad"])


def _edge_inputs(case):
    N, W, multi, H, B = case
    s_w, s_x = SEEDS.get(case, (N + 3 * W + 7 * multi + B, N * 7 + B * 131 + W))
    sd = O.det_state_dict(N, W, multi, H, seed=s_w)
    g = torch.Generator().manual_seed(s_x)
    return sd, torch.randn(B, W, N, generator=g), torch.randn(B, H, N, generator=g)


@pytest.mark.parametrize("dtype", ["f32", "bf16x2"])
@pytest.mark.parametrize("N,W,multi,H,B", EDGE_CASES)
def test_edge_shape_x_grad(N, W, multi, H, B, dtype, monkeypatch):
    sd, x, y = _edge_inputs((N, W, multi, H, B))
    _check_model_x_grad(N, W, multi, H, B, sd, x, y, dtype=dtype, monkeypatch=monkeypatch)


@pytest.mark.parametrize("N,W,multi,H,B", EIG_CASES)
def test_eig_route_x_grad(N, W, multi, H, B, monkeypatch):
    sd, x, y = _edge_inputs((N, W, multi, H, B))
    _check_model_x_grad(N, W, multi, H, B, sd, x, y, spectral="eig", monkeypatch=monkeypatch)


def test_train_mode_dropout_x_grad(monkeypatch):
    N, W, multi, H, B = 10, 4, 2, 2, 4
    sd = O.det_state_dict(N, W, multi, H, seed=5)
    torch.manual_seed(3)
    x, y = torch.randn(B, W, N), torch.randn(B, H, N)
    _check_model_x_grad(N, W, multi, H, B, sd, x, y, monkeypatch=monkeypatch, p=0.5)


def test_loss_method_x_grad(monkeypatch):
    N, W, multi, H, B = 20, 12, 5, 3, 4
    sd = O.det_state_dict(N, W, multi, H, seed=1)
    torch.manual_seed(0)
    x, y = torch.randn(B, W, N), torch.randn(B, H, N)
    _check_model_x_grad(N, W, multi, H, B, sd, x, y, monkeypatch=monkeypatch, use_loss_method=True)


def test_configs3_shard_x_grad(monkeypatch):
    N, W, multi, H, B = 1024, 12, 5, 3, 8
    sd = O.det_state_dict(N, W, multi, H, seed=N)
    torch.manual_seed(N)
    x, y = torch.randn(B, W, N), torch.randn(B, H, N)
    _check_model_x_grad(N, W, multi, H, B, sd, x, y, monkeypatch=monkeypatch, where=DEV)


# ---- 3. invariance / 4. frozen weights --------------------------------------------------------------------------------------
SHAPE = (20, 12, 5, 3, 4)


def _step(model, x, y, need_x, overlap):
    """One train-mode forward + MSE backward; returns (forecast, attention, loss, {name: grad}, x.grad)."""
    from stemgnn_amd import ops

    if overlap:
        model.hot_state.set(direct=True, overlap=True)
        for p in model.parameters():
            p.grad = torch.zeros_like(p) if p.requires_grad else None
    else:
        model.hot_state.set(direct=False)
        model.zero_grad(set_to_none=True)
    xd = x.to(DEV).requires_grad_(need_x)
    f, a = model(xd)
    loss = F.mse_loss(f, y.to(DEV))
    loss.backward()
    ops.join_side_streams()
    torch.cuda.synchronize()
    ops.check_gru_status(DEV)
    grads = {k: (None if p.grad is None else p.grad.clone()) for k, p in model.named_parameters()}
    return f.detach().clone(), a.clone(), loss.detach().clone(), grads, (xd.grad.clone() if need_x else None)


def _setup():
    N, W, multi, H, B = SHAPE
    sd = O.det_state_dict(N, W, multi, H, seed=1)
    torch.manual_seed(0)
    return _model(N, W, multi, H, sd).train(), torch.randn(B, W, N), torch.randn(B, H, N)


@pytest.mark.parametrize("overlap", [False, True])
def test_everything_else_is_unchanged_by_x_requires_grad(overlap):
    model, x, y = _setup()
    f0, a0, l0, g0, _ = _step(model, x, y, False, overlap)
    f1, a1, l1, g1, gx = _step(model, x, y, True, overlap)
    assert gx is not None and float(gx.abs().max()) > 0.0
    assert torch.equal(f0, f1) and torch.equal(a0, a1) and torch.equal(l0, l1)
    for k in g0:
        assert (g0[k] is None) == (g1[k] is None), k
        assert g0[k] is None or torch.equal(g0[k], g1[k]), k
    if overlap:
        _, _, _, _, gx_plain = _step(model, x, y, True, False)
        assert relerr(gx, gx_plain) < 1e-5, relerr(gx, gx_plain)


def test_x_grad_accumulates_and_autograd_grad_leaves_params_alone():
    model, x, y = _setup()
    xd = x.to(DEV).requires_grad_(True)
    for it in range(2):
        f, _ = model(xd)
        F.mse_loss(f, y.to(DEV)).backward()
        if it == 0:
            g1 = xd.grad.clone()
    torch.cuda.synchronize()
    assert torch.equal(xd.grad, 2 * g1)
    model.zero_grad(set_to_none=True)
    xe = x.to(DEV).requires_grad_(True)
    f, _ = model(xe)
    (gx,) = torch.autograd.grad(f.sum(), xe)
    torch.cuda.synchronize()
    assert all(p.grad is None for p in model.parameters())
    N, W, multi, H, B = SHAPE
    sd = O.det_state_dict(N, W, multi, H, seed=1)
    ref = _oracle_x_grad(x, y, sd, use_loss=False)
    assert relerr(gx, ref) < TOL, relerr(gx, ref)


@pytest.mark.parametrize("overlap", [False, True])
def test_frozen_weights_x_grad(overlap):
    """With every weight frozen there is no weight-gradient work to overlap, so both schedules run the plain one: x.grad must
    be the plain trainable run's bit for bit (the overlap schedule's trainable x.grad is within 1e-5 of it, see above)."""
    model, x, y = _setup()
    *_, gx = _step(model, x, y, True, False)
    model.requires_grad_(False)
    f, a, l, grads, gx_frozen = _step(model, x, y, True, overlap)
    assert all(g is None for g in grads.values())
    assert all(p.grad is None for p in model.parameters())
    assert model.hot_state.pending is None
    assert torch.equal(gx, gx_frozen), float((gx - gx_frozen).abs().max())
    # eval-mode attribution pass
    model.eval()
    xe = x.to(DEV).requires_grad_(True)
    model(xe)[0].backward(torch.ones(SHAPE[4], SHAPE[3], SHAPE[0], device=DEV))
    torch.cuda.synchronize()
    N, W, multi, H, B = SHAPE
    ref = _oracle_x_grad(x, y, O.det_state_dict(N, W, multi, H, seed=1), use_loss=False)
    assert relerr(xe.grad, ref) < TOL, relerr(xe.grad, ref)


def test_frozen_weights_x_grad_under_library_gru(monkeypatch):
    model, x, y = _setup()
    *_, gx = _step(model, x, y, True, False)
    monkeypatch.setenv("STEMGNN_GRU", "miopen")
    model.requires_grad_(False)
    *_, gx_lib = _step(model, x, y, True, False)
    assert relerr(gx_lib, gx) < TOL, relerr(gx_lib, gx)
