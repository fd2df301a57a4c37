"""GPU: gradients through the returned attention (stemgnn_attn_laplacian_bwd_ext, SpectralHotPath.backward's `datt`) against
the fp64 oracle -- the stage through the C ABI, the model with an MSE + graph-prior loss, the attention-only backward, edge
saliency with frozen weights, engine.TrainStep(attention_penalty=...) as a hipGraph, and the unchanged plain backward.

Yardstick: the fp64 oracle (oracle.stemgnn_oracle), max-norm relative error < 1e-4 (tests/util.relerr), the LeakyReLU-kink
audit of tests/util.kink_audit unchanged.

Penalties.  Without dropout the rows of the softmax sum to 1, so a penalty whose gradient is constant along the rows of the
symmetrised attention (A.sum(), A.abs().sum()) has an analytically zero gradient (tests/test_attention_grad_abi.py shows it on
the oracle) and a relative error against it measures rounding noise.  The tests use a Frobenius prior
lam * ((A - P) ** 2).sum(), P = rand(N, N) / N, and a linear form (Wt * A).sum(), Wt = randn(N, N).
lam for the MSE + prior loss: the fp64 oracle gives max|d weight_key| = 3.7e-6 / 1.0e-5 / 1.3e-7 / 1.8e-8 from the MSE and
1.9e-2 / 1.4e-2 / 1.6e-4 / 9.9e-5 from the prior at lam = 1 for the four shapes below (the weights and inputs of _inputs below);
lam = 1e-3 puts the prior's share of d weight_key / d weight_query / d GRU at 1 to 5 times the MSE's, so an error in either
share shows in the sum.  The attention-only and TrainStep tests use lam = 1.
Stage-level dropout rate: 0.2 (at N = 5, B = 1 a rate of 0.5 drops a whole row of the batch-mean attention with
probability 1 / 32 per row, where the Laplacian's 1 / sqrt(degree) has no meaning; the test asserts that no row is)."""
import functools
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import stemgnn_oracle as O
from tests.test_hip_front import ALPHA, OFFSET, SEED, _bits, _Buf, _draws, _Stage
from tests.test_hip_input_grad import _kink_overrides, _model
from tests.util import kink_audit, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-4
DEV = "cuda:0"
NCHUNK = 16


# ---- 1. stage level, through the C ABI ----------------------------------------------------------------------------------------
def _bwd_ext(stg, saved, G, nchunk, parts, with_dL=True):
    """stemgnn_attn_laplacian_bwd_ext on NaN-filled, guarded buffers (the layout of tests/test_hip_front._Stage.bwd)."""
    N, B, lib = stg.N, stg.B, stg.lib
    bufs = dict(scratch=_Buf(lib.stemgnn_attn_scratch_floats(B, N, nchunk)), dh=_Buf(N * B * N), dwk=_Buf(N), dwq=_Buf(N))
    before = saved.full.clone()
    outs = (None, None, None) if parts & 4 else (bufs["dh"].ptr(), bufs["dwk"].ptr(), bufs["dwq"].ptr())
    rc = lib.stemgnn_attn_laplacian_bwd_ext(stg.dL.ptr() if with_dL else None, G.ptr(), stg.h.ptr(), stg.wk.ptr(), stg.wq.ptr(),
                                            ALPHA, stg.p, 1, stg._seedp(), B, N, saved.ptr(), bufs["scratch"].ptr(), nchunk,
                                            *outs, parts, stg.st)
    stg.done(rc, f"attn_laplacian_bwd_ext parts {parts} dL {with_dL}", dict(bufs, G=G))
    assert _bits(saved.full, before), "the backward wrote into `saved`"
    s = bufs["scratch"].t
    nn, bn = N * N, B * N
    return dict(scratch=bufs["scratch"], dAB=s[:nn].view(N, N), dkey=s[nn:nn + bn].view(B, N), dquery=s[nn + bn:nn + 2 * bn].view(B, N),
                dh=bufs["dh"].t.view(N, B, N), dwk=bufs["dwk"].t, dwq=bufs["dwq"].t)


def _stage_reference(d, G, N, B, p, mask, key32, query32, with_dL):
    """fp64 autograd of sum(dL * L) + sum(G * A_s) (the first term only with_dL) by the oracle's functions, on the device; the
    LeakyReLU decisions are the kernel's (fp32 add of its saved key / query), as in tests/test_hip_front._reference."""
    dt = torch.float64
    h = d["h"].to(dt).requires_grad_(True)
    wk = d["wk"].to(dt).requires_grad_(True)
    wq = d["wq"].to(dt).requires_grad_(True)
    inp = h.permute(1, 2, 0)
    key, query = torch.matmul(inp, wk), torch.matmul(inp, wq)
    unit = torch.eye(2, dtype=dt, device=h.device)
    kink = (key32[:, :, None] + query32[:, None, :]) > 0
    att = O.self_graph_attention(torch.cat([key, query], 2).permute(0, 2, 1), unit[:, :1], unit[:, 1:], ALPHA,
                                 drop_mask=mask.to(dt) if p > 0 else None, drop_p=float(torch.tensor(p, dtype=torch.float32)),
                                 kink_pos=kink)
    L, A_s = O.laplacian_from_attention(att)
    loss = (A_s * G.to(dt)).sum()
    if with_dL:
        loss = loss + (L * d["dL"].to(dt)).sum()
    loss.backward()
    return dict(dh=h.grad, dwk=wk.grad[:, 0], dwq=wq.grad[:, 0], key=key.detach()[..., 0], query=query.detach()[..., 0])


STAGE_CASES = list(itertools.product([5, 40, 256, 257, 300], [1, 3], [0.0, 0.2]))


@pytest.mark.parametrize("N,B,p", STAGE_CASES, ids=[f"N{n}-B{b}-p{p}" for n, b, p in STAGE_CASES])
def test_stage_ext_vs_fp64(N, B, p):
    d = _draws(N, B, "rand")
    stg = _Stage(d, N, B, p, (SEED + N, OFFSET + B) if p > 0 else None)
    mask = None
    if p > 0:
        mask = stg.mask().clone()
        assert bool((mask.mean(0).sum(1) > 0).all()), "a row of the batch-mean attention is dropped whole"
    Fw = stg.fwd()
    Gt = torch.randn(N, N, generator=torch.Generator().manual_seed(77 * N + B)).to(DEV)
    G = _Buf(N * N)
    G.t.copy_(Gt.reshape(-1))
    wk64, wq64 = d["wk"].double()[:, 0], d["wq"].double()[:, 0]
    audited = False
    for with_dL in (True, False):
        ref = _stage_reference(d, Gt, N, B, p, mask, Fw["key"], Fw["query"], with_dL)
        if not audited:
            ek = float((Fw["key"].double() - ref["key"]).abs().max())
            eq = float((Fw["query"].double() - ref["query"]).abs().max())
            pos = (Fw["key"][:, :, None] + Fw["query"][:, None, :]) > 0
            kink_audit(pos, ref["key"][:, :, None] + ref["query"][:, None, :], ek + eq, f"stage N={N} B={B}")
            audited = True
        mat = _bwd_ext(stg, Fw["saved"], G, NCHUNK, 3, with_dL)
        fac = _bwd_ext(stg, Fw["saved"], G, NCHUNK, 3 | 4, with_dL)
        assert _bits(fac["scratch"].t, mat["scratch"].t), "parts 3|4: other bits in the scratch than the materialised form"
        assert all(bool(torch.isnan(fac[q]).all()) for q in ("dh", "dwk", "dwq")), "parts 3|4 touched dh / dwk / dwq"
        dwk_f, dwq_f = stg.wgrad(scratch=fac["scratch"])
        dh_f = fac["dkey"].double()[None] * wk64[:, None, None] + fac["dquery"].double()[None] * wq64[:, None, None]
        errs = {"dh": relerr(mat["dh"], ref["dh"]), "dwk": relerr(mat["dwk"], ref["dwk"]), "dwq": relerr(mat["dwq"], ref["dwq"]),
                "factored dh": relerr(dh_f, ref["dh"]), "factored dwk": relerr(dwk_f, ref["dwk"]),
                "factored dwq": relerr(dwq_f, ref["dwq"])}
        print(f"stage {(N, B, p)} dL {'given' if with_dL else 'NULL'}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        assert float(ref["dh"].abs().max()) > 0.0
        assert all(v < TOL for v in errs.values()), errs
    # a zero external gradient leaves the plain entry's result
    Z = _Buf(N * N, fill=0.0)
    zero = _bwd_ext(stg, Fw["saved"], Z, NCHUNK, 3)
    plain = stg.bwd(Fw["saved"], NCHUNK)
    for q in ("dAB", "dkey", "dquery", "dh", "dwk", "dwq"):
        assert torch.equal(zero[q], plain[q]), f"zero G: {q} differs from stemgnn_attn_laplacian_bwd's"
    # parts 1 then 2 (the exact-mode caller's form) gives the bits of parts 3
    N_, B_, lib = stg.N, stg.B, stg.lib
    split = _Buf(lib.stemgnn_attn_scratch_floats(B_, N_, NCHUNK))
    for parts in (1, 2 | 4):
        rc = lib.stemgnn_attn_laplacian_bwd_ext(stg.dL.ptr(), G.ptr(), stg.h.ptr(), stg.wk.ptr(), stg.wq.ptr(), ALPHA, stg.p, 1,
                                                stg._seedp(), B_, N_, Fw["saved"].ptr(), split.ptr(), NCHUNK, None, None, None,
                                                parts, stg.st)
        stg.done(rc, f"attn_laplacian_bwd_ext parts {parts}", dict(scratch=split))
    whole = _bwd_ext(stg, Fw["saved"], G, NCHUNK, 3 | 4)
    assert _bits(split.t, whole["scratch"].t), "parts 1 then 2|4: other bits than parts 3|4"


# ---- 2. model level: MSE + Frobenius prior ----------------------------------------------------------------------------------
MODEL_CASES = [(20, 12, 5, 3, 4), (228, 12, 5, 3, 32), (257, 12, 5, 3, 2), (17, 13, 5, 7, 1)]
MODES = ["eval", "train_p0", "train_mask"]
LAM = 1e-3
DROP_P = 0.5
DROP_SEED = (424242, 17)


@functools.lru_cache(maxsize=None)
def _inputs(case):
    N, W, multi, H, B = case
    sd = O.det_state_dict(N, W, multi, H, seed=1)
    g = torch.Generator().manual_seed(N)
    x, y = torch.randn(B, W, N, generator=g), torch.randn(B, H, N, generator=g)
    prior = torch.rand(N, N, generator=g) / N
    wt = torch.randn(N, N, generator=g)
    return sd, x, y, prior, wt


def _frob(prior, lam):
    return lambda A: lam * ((A - prior.to(device=A.device, dtype=A.dtype)) ** 2).sum()


def _linear(wt):
    return lambda A: (wt.to(device=A.device, dtype=A.dtype) * A).sum()


def _oracle_grads(case, penalty, with_mse, kw, root=None):
    """fp64 gradients of [MSE +] penalty(A_s) (root: of A_s[root] instead) for every weight and x: ({name: grad | None}, x.grad)"""
    sd, x, y = _inputs(case)[:3]
    leaves = {k: v.double().requires_grad_(True) for k, v in sd.items()}
    x64 = x.double().requires_grad_(True)
    f, A = O.model_forward(x64, leaves, **kw)
    loss = A[root] if root is not None else penalty(A)
    if with_mse:
        loss = loss + F.mse_loss(f, y.double())
    grads = torch.autograd.grad(loss, list(leaves.values()) + [x64], allow_unused=True)
    return dict(zip(leaves, grads[:-1])), grads[-1]


_oracle_cache = {}


def _setup_model(case, mode, monkeypatch, dtype="f32", spectral="cheb"):
    """(model, oracle kwargs, dropout seed | None) for one mode; the dropout mask is the one the kernels will regenerate"""
    from stemgnn_amd import ops

    N, W, multi, H, B = case
    monkeypatch.setenv("STEMGNN_DTYPE", dtype)
    monkeypatch.setenv("STEMGNN_SPECTRAL", spectral)
    p = DROP_P if mode == "train_mask" else 0.0
    model = _model(N, W, multi, H, _inputs(case)[0], p=p)
    model.train(mode != "eval")
    kw, seed = {}, None
    if p > 0.0:
        seed = DROP_SEED
        model.set_dropout_seed(*seed)
        mask = ops.dropout_mask(p, model._seed.clone(), B, N)
        assert bool((mask.mean(0).sum(1) > 0).all()), "a row of the batch-mean attention is dropped whole"
        kw = dict(drop_mask=mask.cpu().double(), drop_p=p)
    return model, kw, seed


def _compare(model, xd, case, penalty, with_mse, kw, seed, names=None, root=None, cache_key=None):
    """every parameter gradient (of `names`, default all) and x.grad against the oracle; on a miss, once more with the kink
    decisions of the implementation (tests/test_hip_input_grad._kink_overrides audits them).  Prints every figure."""
    from stemgnn_amd import ops

    torch.cuda.synchronize()
    ops.check_gru_status(DEV)
    sd, x = _inputs(case)[:2]

    def errors(ref, ref_x):
        errs = {}
        for k, p in model.named_parameters():
            if names is not None and not k.startswith(names):
                continue
            if ref[k] is None:
                continue
            assert p.grad is not None, f"{k}: no gradient"
            errs[k] = relerr(p.grad, ref[k])
        if xd.grad is not None:
            errs["x"] = relerr(xd.grad, ref_x)
        return errs

    if cache_key is None or cache_key not in _oracle_cache:
        got = _oracle_grads(case, penalty, with_mse, kw, root)
        if cache_key is not None:
            _oracle_cache.clear()                  # the last reference is kept: the dtype / path parametrisation reuses it
            _oracle_cache[cache_key] = got
    else:
        got = _oracle_cache[cache_key]
    errs = errors(*got)
    worst = max(errs.items(), key=lambda kv: kv[1])
    if not worst[1] < TOL:
        over = _kink_overrides(model, xd.detach(), x, sd, "cpu", kw, seed)
        if over:
            errs2 = errors(*_oracle_grads(case, penalty, with_mse, dict(kw, **over), root))
            print(f"kink flips: worst {worst[0]} {worst[1]:.2e} against the un-overridden fp64 run")
            errs = errs2
            worst = max(errs.items(), key=lambda kv: kv[1])
    print(f"{case}: worst {worst[0]} {worst[1]:.2e}; x {errs.get('x', float('nan')):.2e}, weight_key "
          f"{errs.get('weight_key', float('nan')):.2e}, weight_query {errs.get('weight_query', float('nan')):.2e}")
    assert worst[1] < TOL, {k: v for k, v in errs.items() if not v < TOL}
    return errs


@pytest.mark.parametrize("path", ["forward", "loss"])
@pytest.mark.parametrize("dtype", ["f32", "bf16x2"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("N,W,multi,H,B", MODEL_CASES)
def test_model_mse_plus_prior_vs_oracle(N, W, multi, H, B, mode, dtype, path, monkeypatch):
    case = (N, W, multi, H, B)
    _, x, y, prior, _ = _inputs(case)
    model, kw, seed = _setup_model(case, mode, monkeypatch, dtype)
    pen = _frob(prior, LAM)
    xd = x.to(DEV).requires_grad_(True)
    if path == "loss":
        loss, att = model.loss(xd, y.to(DEV), return_attention=True)
    else:
        f, att = model(xd)
        loss = F.mse_loss(f, y.to(DEV))
    assert att.requires_grad
    (loss + pen(att)).backward()
    errs = _compare(model, xd, case, pen, True, kw, seed, cache_key=(case, mode))
    assert {"weight_key", "weight_query", "x", "GRU.weight_hh_l0", "stock_block.0.weight", "fc.0.weight"} <= set(errs)


# ---- 3. attention-only ------------------------------------------------------------------------------------------------------
FRONT = ("GRU.", "weight_key", "weight_query")


def _attention_only(model, case, xd=None, root=None):
    _, x, _, _, wt = _inputs(case)
    xd = x.to(DEV).requires_grad_(True) if xd is None else xd
    _, att = model(xd)
    (att[root] if root is not None else _linear(wt)(att)).backward()
    return xd


@pytest.mark.parametrize("case,mode,spectral", [((20, 12, 5, 3, 4), "train_p0", "cheb"), ((20, 12, 5, 3, 4), "eval", "cheb"),
                                                ((257, 12, 5, 3, 2), "train_mask", "cheb"), ((228, 12, 5, 3, 32), "train_p0", "cheb"),
                                                ((256, 12, 5, 3, 2), "train_p0", "eig")])
def test_attention_only_backward(case, mode, spectral, monkeypatch):
    from stemgnn_amd import ops

    model, kw, seed = _setup_model(case, mode, monkeypatch, spectral=spectral)
    wt = _inputs(case)[4]
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        if seed is not None:
            model.set_dropout_seed(*seed)
        xd = _attention_only(model, case)
        torch.cuda.synchronize()
        runs.append(({k: None if p.grad is None else p.grad.clone() for k, p in model.named_parameters()}, xd.grad.clone()))
    _compare(model, xd, case, _linear(wt), False, kw, seed, names=FRONT)
    if spectral == "eig":
        ops.check_eigh_status(DEV)
    for k, g in runs[0][0].items():
        if k.startswith(("stock_block.", "fc.")):
            assert g is None, f"{k} received a gradient from the attention alone"
        else:
            assert g is not None and float(g.abs().max()) > 0.0, k
            assert torch.equal(g, runs[1][0][k]), f"{k} differs from run to run"
    assert torch.equal(runs[0][1], runs[1][1]), "x.grad differs from run to run"
    assert model.hot_state.pending is None and model.hot_state.tail_finish is None


def test_attention_only_in_direct_overlap_mode_leaves_block_gradients_alone():
    """direct-gradient + side-stream mode (what engine.TrainStep sets): the attention-only backward writes no block / fc
    p.grad, queues nothing on the side stream, and gives the front's gradients of the plain mode."""
    from stemgnn_amd import ops

    case = (20, 12, 5, 3, 4)
    N, W, multi, H, B = case
    model = _model(N, W, multi, H, _inputs(case)[0]).train()
    xp = _attention_only(model, case)
    torch.cuda.synchronize()
    plain = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    model.hot_state.set(direct=True, overlap=True)
    for p in model.parameters():
        p.grad = torch.full_like(p, 3.0)
    xo = _attention_only(model, case)
    ops.join_side_streams()
    torch.cuda.synchronize()
    assert model.hot_state.pending is None
    for k, p in model.named_parameters():
        if k.startswith(("stock_block.", "fc.")):
            assert bool((p.grad == 3.0).all()), f"{k}: p.grad was written"
        else:
            assert relerr(p.grad, plain[k]) < 1e-5, (k, relerr(p.grad, plain[k]))
    assert relerr(xo.grad, xp.grad) < 1e-5


def test_attention_only_with_a_pending_fused_tail_runs_the_whole_backward():
    """Model.loss(unit_grad=True) in direct + side-stream mode defers the fc tail's partial-sum launch to
    SpectralHotPath.backward; a backward from the attention alone must still run it (no shortcut): the loss value and the fc
    gradients appear, the front's gradients are the attention-only ones."""
    from stemgnn_amd import ops

    case = (20, 12, 5, 3, 4)
    N, W, multi, H, B = case
    _, x, y, _, wt = _inputs(case)
    model = _model(N, W, multi, H, _inputs(case)[0]).train()
    _attention_only(model, case)
    torch.cuda.synchronize()
    alone = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    with torch.no_grad():
        want = float(model.loss(x.to(DEV), y.to(DEV)))
    model.hot_state.set(direct=True, overlap=True)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    loss, att = model.loss(x.to(DEV), y.to(DEV), unit_grad=True, return_attention=True)
    assert model.hot_state.tail_finish is not None, "the fused tail did not defer its second launch: nothing to test"
    _linear(wt)(att).backward()
    ops.join_side_streams()
    torch.cuda.synchronize()
    assert model.hot_state.tail_finish is None
    assert abs(float(loss) - want) <= 1e-6 * abs(want), (float(loss), want)
    assert float(model.fc[0].weight.grad.abs().max()) > 0.0
    for k in alone:
        g = dict(model.named_parameters())[k].grad
        assert relerr(g, alone[k]) < 1e-5, (k, relerr(g, alone[k]))


# ---- 4. frozen weights: saliency of one edge ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case,mode,root", [((20, 12, 5, 3, 4), "eval", (3, 7)), ((20, 12, 5, 3, 4), "train_p0", (11, 11)),
                                            ((257, 12, 5, 3, 2), "eval", (256, 0))])
def test_edge_saliency_with_frozen_weights(case, mode, root, monkeypatch):
    model, kw, seed = _setup_model(case, mode, monkeypatch)
    model.requires_grad_(False)
    xd = _attention_only(model, case, root=root)
    assert all(p.grad is None for p in model.parameters())
    assert xd.grad is not None and float(xd.grad.abs().max()) > 0.0
    _compare(model, xd, case, None, False, kw, seed, names=("no parameter",), root=root)


# ---- 5. engine.TrainStep(attention_penalty=...) -------------------------------------------------------------------------------
def test_train_step_with_attention_penalty_captures_a_graph_and_matches_eager():
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    N, W, H, multi, B, T, K = 20, 12, 3, 5, 4, 120, 6
    dev = torch.device(DEV)
    g = torch.Generator().manual_seed(2)
    series = torch.randn(T, N, generator=g).to(dev)
    hi = (torch.randint(0, T - W - H, (K, B), generator=g) + W).to(dev)
    prior = (torch.rand(N, N, generator=g) / N).to(dev)
    pen = _frob(prior, 1.0)
    outs = {}
    for name, graph, penalty in (("graph", True, pen), ("eager", False, pen), ("plain", True, None)):
        torch.manual_seed(7)
        model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0).to(dev).train()
        opt = FusedRMSprop(model.parameters(), lr=1e-3)
        step = TrainStep(model, opt, B, W, H, N, series=series, graph=graph, attention_penalty=penalty)
        for i in range(K):
            if i == K - 1:
                before = opt.flat_p.clone()
            step.run_indices(hi[i])
        torch.cuda.synchronize()
        assert step.mode.startswith("hipgraph") == graph, step.mode
        outs[name] = opt.flat_p.clone()
        if penalty is None:
            assert step.penalty is None
            continue
        # the static scalar holds the penalty of the last step's forward: the callable on the attention of the parameters
        # that step started from (dropout 0: train and eval forward are the same function)
        after = opt.flat_p.clone()
        opt.flat_p.copy_(before)
        model.eval()
        with torch.no_grad():
            want = pen(model(step.x)[1])
        opt.flat_p.copy_(after)
        print(f"{name}: step.penalty {float(step.penalty):.9e}, callable {float(want):.9e}, loss {float(step.loss):.6e}")
        assert float(want) > 0.0 and torch.equal(step.penalty, want), (float(step.penalty), float(want))
    assert relerr(outs["graph"], outs["eager"]) < 1e-6, relerr(outs["graph"], outs["eager"])
    assert not torch.equal(outs["graph"], outs["plain"]), "the penalty did not change the training"


def test_train_step_with_attention_penalty_in_exact_mode_graph_equals_eager():
    """Exact data-parallel mode with the data-changing stand-in collective of tests/test_hip_schedule.py: the two [N,N]
    collectives (the second now carries the attention's gradient too) captured inside the one graph give the eager step."""
    from stemgnn_amd import Model, ops
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop
    from tests.test_hip_schedule import SHAPE, _double

    c = dict(SHAPE, T=800)
    dev = torch.device(DEV)
    steps = 6
    res = {}
    for name, kwargs in (("eager", dict(graph=False)), ("graph", dict(one_graph=True)), ("graph, no penalty", dict(one_graph=True))):
        torch.manual_seed(0)
        model = Model(c["N"], 2, c["W"], c["multi"], horizon=c["H"]).to(dev).train()        # dropout 0.5
        model.set_dropout_seed(99)
        opt = FusedRMSprop(model.parameters(), lr=1e-4, eps=1e-8)
        g = torch.Generator().manual_seed(7)
        series = torch.randn(c["T"], c["N"], generator=g).to(dev)
        total = steps + 1
        hi = (torch.randint(0, c["T"] - c["W"] - c["H"], (total * c["B"],), generator=g) + c["W"]).to(dev)
        prior = (torch.rand(c["N"], c["N"], generator=g) / c["N"]).to(dev)
        step = TrainStep(model, opt, c["B"], c["W"], c["H"], c["N"], series=series, world=2, exact=True, collective_fn=_double,
                         order_capacity=total * c["B"], schedule_check=False,
                         attention_penalty=None if "no penalty" in name else _frob(prior, 1.0), **kwargs)
        step.load_order(hi)
        for _ in range(total):
            step.run_next()
        torch.cuda.synchronize()
        ops.check_gru_status(dev)
        ops.check_gather_status(dev)
        res[name] = (opt.flat_p.clone(), step)
    assert res["eager"][1].mode == "eager"
    s_graph = res["graph"][1]
    assert s_graph.mode.startswith("hipgraph(whole step incl. the exact-mode"), (s_graph.mode, s_graph.schedule)
    assert s_graph.schedule["one_graph_verified"]["ok"], s_graph.schedule
    assert torch.equal(res["graph"][0], res["eager"][0]), float((res["graph"][0] - res["eager"][0]).abs().max())
    assert not torch.equal(res["graph"][0], res["graph, no penalty"][0])


# ---- 6. unchanged behaviour ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("overlap", [False, True])
def test_plain_backward_is_unchanged_by_a_live_attention_output(overlap):
    from stemgnn_amd import ops

    case = (20, 12, 5, 3, 4)
    N, W, multi, H, B = case
    _, x, y = _inputs(case)[:3]
    model = _model(N, W, multi, H, _inputs(case)[0]).train()
    got = []
    for keep in (True, False):
        if overlap:
            model.hot_state.set(direct=True, overlap=True)
            for p in model.parameters():
                p.grad = torch.zeros_like(p)
        else:
            model.zero_grad(set_to_none=True)
        xd = x.to(DEV).requires_grad_(True)
        out = model(xd)
        f, kept = (out[0], out[1]) if keep else (out[0], None)
        del out
        F.mse_loss(f, y.to(DEV)).backward()
        ops.join_side_streams()
        torch.cuda.synchronize()
        assert kept is None or kept.requires_grad
        got.append(({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, xd.grad.clone()))
    assert got[0][0].keys() == got[1][0].keys()
    for k in got[0][0]:
        assert torch.equal(got[0][0][k], got[1][0][k]), k
    assert torch.equal(got[0][1], got[1][1])
