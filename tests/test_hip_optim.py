"""GPU: the fused optimizers' opt-in controls (csrc/optim.hip, stemgnn_amd/optim.py) -- gradient-norm clipping, weight decay,
non-finite skip -- against torch's own CPU optimizers and torch.nn.utils.clip_grad_norm_, alone and inside engine.TrainStep
(eager, hipGraph, the data-parallel forms), plus state_dict resume and the trainer's log line.

The optimizer comparisons use the set-up of tests/test_hip_tail.py::test_fused_rmsprop_matches_torch_rmsprop: five shapes
(4194 floats: not a multiple of 4, so the one-thread ragged tail runs), 6 steps, an ExponentialLR step after the third, one
shape that never gets a gradient.  Bars: that file's (parameters relerr < 1e-6 RMSprop, < 2e-6 Adam) and 2e-6 on the moments --
the moments are what show a wrong coefficient (RMSprop's update is almost scale-free)."""
import functools
import re
import types

import numpy as np
import pytest
import torch

from tests.util import relerr, synthetic_series

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(7, 5), (13,), (1, 4, 1, 6, 6), (3,), (129, 31)]
NO_GRAD = 3                       # the shape that never receives a gradient
P_BAR = {"rmsprop": 1e-6, "adam": 2e-6}
M_BAR = 2e-6


# ---- 1. the norm kernel ------------------------------------------------------------------------------------------------
def _chunk(lib):
    c = 1
    while lib.stemgnn_grad_norm_partials(c + 1) == 1:
        c += 1
    return c


@pytest.mark.parametrize("scale", [1.0, 0.25])
def test_grad_norm_kernel_vs_fp64_numpy(scale):
    """stats[0] of a step (sqsum launch + step kernel, lr = 0) against sqrt(sum((g * scale)^2)) in fp64 numpy.  Bar 1e-6:
    the scaling is one fp32 rounding per element (the square and the sum are fp64), <= 6e-8 on the root, the final fp32
    rounding of the norm another 6e-8; the bar is several times that.  The same input twice gives the same bits, and the
    kernel writes exactly stemgnn_grad_norm_partials(n) partial sums (a guard word behind them stays untouched)."""
    from stemgnn_amd import _lib
    lib = _lib.load()
    C = _chunk(lib)
    sizes = [1, 3, 4, 5, 1023, 1024, 1025, C, C + 1, 2 * C + 3, 2048 * 1024 + 5]
    gen = torch.Generator().manual_seed(11)
    stream = torch.cuda.current_stream().cuda_stream
    lr = torch.zeros(1, device=DEV)
    for n in sizes:
        g_host = torch.randn(n, generator=gen)
        ref = float(np.sqrt(np.sum((g_host.numpy().astype(np.float64) * scale) ** 2)))
        g = g_host.to(DEV)
        p, sq = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        np_ = int(lib.stemgnn_grad_norm_partials(n))
        assert np_ == (n + C - 1) // C
        partials = torch.full((np_ + 1,), -7.0, device=DEV, dtype=torch.float64)
        got = []
        for _ in range(2):
            stats = torch.zeros(4, device=DEV, dtype=torch.float64)
            _lib.check(lib.stemgnn_grad_sqsum(g.data_ptr(), n, scale, partials.data_ptr(), stream), "grad_sqsum")
            _lib.check(lib.stemgnn_rmsprop_step_ext(p.data_ptr(), g.data_ptr(), sq.data_ptr(), n, lr.data_ptr(), 0.99, 1e-8, 0,
                                                    scale, 0.0, 1e30, 0, partials.data_ptr(), stats.data_ptr(), stream),
                       "rmsprop_step_ext")
            got.append(stats.cpu())
        part = partials.cpu().numpy()
        err = abs(float(got[0][0]) - ref) / ref
        err_parts = abs(float(np.sqrt(part[:np_].sum())) - ref) / ref
        print(f"n={n} scale={scale}: norm {float(got[0][0]):.9g} fp64 {ref:.9g} relerr {err:.2e} (partials alone {err_parts:.2e})")
        assert part[np_] == -7.0, "the norm kernel wrote past its partial sums"
        assert err <= 1e-6 and err_parts <= 1e-6, (n, err, err_parts)
        assert got[0][0].view(torch.int64) == got[1][0].view(torch.int64), "two runs of one input differ in stats[0]"
        assert got[0].tolist()[1:] == [1.0, 0.0, 0.0]                 # not clipped, nothing counted
        assert float(p.abs().max()) == 0.0 and torch.equal(g.cpu(), g_host)   # lr = 0, zero_grad = 0: nothing else written


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_step_kernels_past_the_grid_cap_and_ragged_tail(kind):
    """One clipped step over 2048 * 1024 + 5 floats: past the step kernels' 2048-block grid (the grid-stride loop
    runs twice for some threads) with a one-element ragged tail, against torch's optimizer on one tensor.  The reference
    clips with clip_grad_norm_'s formula on a norm taken in fp64: torch's own fp32 sum over 2M squares carries more error
    than the bars below allow, and the norm is what this test is about."""
    n = 2048 * 1024 + 5
    torch.manual_seed(3)
    ref_p = [torch.randn(n, requires_grad=True)]
    grad = torch.randn(n)
    ref_opt, my_opt, my_p = _optimizers(kind, ref_p, {}, dict(max_grad_norm=700.0))
    ref_p[0].grad = grad.clone()
    my_opt.bucket.views[0].copy_(grad.to(DEV))
    total = np.float32(np.sqrt(np.sum(grad.numpy().astype(np.float64) ** 2)))
    assert total > 1400.0                                             # sqrt(n) = 1448: the step is clipped to about half
    ref_p[0].grad.mul_(float(min(np.float32(1.0), np.float32(700.0) / (total + np.float32(1e-6)))))
    ref_opt.step()
    my_opt.step()
    rep = my_opt.grad_report()
    assert abs(rep["norm"] - float(total)) <= 1e-6 * float(total) and rep["clipped_steps"] == 1, rep
    assert relerr(my_p[0].detach(), ref_p[0].detach()) < P_BAR[kind]
    for name, mine in _my_moments(kind, my_opt).items():
        assert relerr(mine, ref_opt.state[ref_p[0]][name]) < M_BAR, name
    assert float(my_opt.bucket.flat.abs().max()) == 0.0


# ---- 2.-5. against torch's optimizers ----------------------------------------------------------------------------------------
def _optimizers(kind, ref_p, ref_kw, my_kw, ref_cls=None):
    from stemgnn_amd.optim import FusedAdam, FusedRMSprop
    my_p = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in ref_p]
    if kind == "rmsprop":
        ref_opt = torch.optim.RMSprop(ref_p, lr=1e-3, eps=1e-8, **ref_kw)
        my_opt = FusedRMSprop(my_p, lr=1e-3, alpha=0.99, eps=1e-8, **my_kw)
    else:
        ref_opt = (ref_cls or torch.optim.Adam)(ref_p, lr=1e-3, betas=(0.9, 0.999), **ref_kw)
        my_opt = FusedAdam(my_p, lr=1e-3, betas=(0.9, 0.999), **my_kw)
    return ref_opt, my_opt, my_p


def _my_moments(kind, opt):
    if kind == "rmsprop":
        return {"square_avg": opt.square_avg}
    return {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}


def _state_clone(kind, opt):
    names = ("flat_p", "square_avg") if kind == "rmsprop" else ("flat_p", "square_avg", "exp_avg", "_step_dev")
    return {k: getattr(opt, k).clone() for k in names}


def _run(kind, ref_kw, my_kw, ref_cls=None, max_norm=None, poison=None, all_grads=False, steps=6, seed=0):
    """6 steps of both optimizers on the same gradients: randn (total norm ~ 65), halved on odd steps (~ 32).  poison =
    (step, shape index, flat index, value): that gradient element of that step is replaced, torch OMITS the step (what
    skip_nonfinite promises) and the fused state must not move by a bit.  Returns what the assertions need."""
    torch.manual_seed(seed)
    ref_p = [torch.randn(s, requires_grad=True) for s in SHAPES]
    ref_opt, my_opt, my_p = _optimizers(kind, ref_p, ref_kw, my_kw, ref_cls)
    sched_r = torch.optim.lr_scheduler.ExponentialLR(ref_opt, gamma=0.5)
    sched_m = torch.optim.lr_scheduler.ExponentialLR(my_opt, gamma=0.5)
    untouched = my_p[NO_GRAD].detach().clone()
    decays = my_kw.get("weight_decay", 0.0) != 0.0
    for it in range(steps):
        grads = [torch.randn(s) * (0.5 if it % 2 else 1.0) for s in SHAPES]
        poisoned = poison is not None and it == poison[0]
        if poisoned:
            grads[poison[1]].view(-1)[poison[2]] = poison[3]
        for p, g in zip(ref_p, grads):
            p.grad = g.clone()
        for view, g in zip(my_opt.bucket.views, grads):
            view.copy_(g.to(DEV))
        if not all_grads:
            # the shape that never receives a gradient: an all-zero slot of the flat bucket.  torch skips a parameter whose
            # .grad is None -- the same outcome without weight decay; WITH it the fused kernel decays the slot like any
            # zero gradient, so torch is handed the zero gradient the kernel sees
            ref_p[NO_GRAD].grad = torch.zeros(SHAPES[NO_GRAD]) if decays else None
            my_opt.bucket.views[NO_GRAD].zero_()
        before = _state_clone(kind, my_opt)
        if not (poisoned and my_kw.get("skip_nonfinite")):
            if max_norm is not None:
                torch.nn.utils.clip_grad_norm_([p for p in ref_p if p.grad is not None], max_norm)
            ref_opt.step()
        my_opt.step()
        if poisoned and my_kw.get("skip_nonfinite"):
            for k, v in before.items():
                assert torch.equal(getattr(my_opt, k), v), f"skipped step moved {k}"
            rep = my_opt.grad_report()
            assert rep["coef"] == 0.0 and not np.isfinite(rep["norm"]), rep
        if it == 2:
            sched_r.step(); sched_m.step()
        assert float(my_opt.bucket.flat.abs().max()) == 0.0, "gradients not cleared by the fused kernel"
    torch.cuda.synchronize()
    if not all_grads and not decays:
        assert torch.equal(my_p[NO_GRAD].detach(), untouched)
    return ref_p, ref_opt, my_p, my_opt


def _assert_matches(kind, ref_p, ref_opt, my_p, my_opt):
    for mine, theirs in zip(my_p, ref_p):
        assert mine.data_ptr() >= my_opt.flat_p.data_ptr()
        assert relerr(mine.detach(), theirs.detach()) < P_BAR[kind]
    off = 0
    for p in ref_p:                                                  # the flat moments against torch's per-parameter state
        n = p.numel()
        for name, flat in _my_moments(kind, my_opt).items():
            theirs = ref_opt.state[p][name] if name in ref_opt.state.get(p, {}) else torch.zeros_like(p)
            assert relerr(flat[off:off + n].view_as(p), theirs) < M_BAR, (name, tuple(p.shape))
        off += n


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_max_grad_norm_matches_clip_grad_norm(kind):
    out = _run(kind, {}, dict(max_grad_norm=50.0), max_norm=50.0)
    _assert_matches(kind, *out)
    rep = out[3].grad_report()
    assert rep["clipped_steps"] == 3 and rep["skipped_steps"] == 0, rep       # the even steps (norm ~ 65), not the odd (~ 32)
    assert 25.0 < rep["norm"] < 40.0 and rep["coef"] == 1.0, rep               # the last step is an odd one


@pytest.mark.parametrize("kind,ref_cls,my_kw", [
    ("rmsprop", None, {}), ("adam", None, {}), ("adam", torch.optim.AdamW, dict(decoupled_weight_decay=True))])
def test_weight_decay_matches_torch(kind, ref_cls, my_kw):
    out = _run(kind, dict(weight_decay=1e-2), dict(weight_decay=1e-2, **my_kw), ref_cls=ref_cls, seed=1)
    _assert_matches(kind, *out)
    rep = out[3].grad_report()
    assert np.isnan(rep["norm"]) and rep["coef"] == 1.0 and rep["clipped_steps"] == 0, rep   # no norm taken: one launch as before


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_clip_then_decay_order(kind):
    """weight decay 0.5 (large, so that the order matters far above the bar) with clipping: torch clips the raw gradient and
    the optimizer then adds wd * p; decaying first would change the clipped norm."""
    out = _run(kind, dict(weight_decay=0.5), dict(weight_decay=0.5, max_grad_norm=50.0), max_norm=50.0, seed=2)
    _assert_matches(kind, *out)
    assert out[3].grad_report()["clipped_steps"] == 3


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
@pytest.mark.parametrize("value,where", [(float("inf"), (4, 129 * 31 - 1)), (float("nan"), (0, 0))])
def test_skip_nonfinite_leaves_the_state_untouched(kind, value, where):
    """Step 3 of 6 carries one inf (the last element of the bucket: the ragged tail) or one NaN (the first): nothing moves by a
    bit (_run checks it), the gradients are zeroed, and the end equals a torch run that omits the step."""
    out = _run(kind, {}, dict(skip_nonfinite=True), poison=(2, where[0], where[1], value), seed=4)
    _assert_matches(kind, *out)
    rep = out[3].grad_report()
    assert rep["skipped_steps"] == 1 and rep["clipped_steps"] == 0, rep
    if kind == "adam":
        assert float(out[3]._step_dev) == 5.0                       # the skipped step did not advance the count


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
@pytest.mark.parametrize("value", [float("inf"), float("nan")])
def test_without_skip_nonfinite_nan_propagates_as_in_torch(kind, value):
    """max_grad_norm without skip_nonfinite: torch's behaviour -- a NaN norm makes every parameter NaN, an inf norm gives the
    coefficient 0 and inf * 0 = NaN in that one element.  Every shape gets a gradient here (torch leaves a parameter without
    one alone; the flat bucket cannot tell it from a zero gradient)."""
    ref_p, ref_opt, my_p, my_opt = _run(kind, {}, dict(max_grad_norm=50.0), max_norm=50.0, poison=(2, 4, 77, value),
                                        all_grads=True, steps=3, seed=5)
    n_nan = 0
    for mine, theirs in zip(my_p, ref_p):
        assert torch.equal(torch.isnan(mine.detach()).cpu(), torch.isnan(theirs.detach()))
        n_nan += int(torch.isnan(theirs).sum())
    assert n_nan == (1 if value == float("inf") else sum(p.numel() for p in ref_p))
    assert my_opt.grad_report()["skipped_steps"] == 0


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_explicit_defaults_are_the_default_path_bit_for_bit(kind):
    a = _run(kind, {}, {})[3]
    b = _run(kind, {}, dict(weight_decay=0.0, max_grad_norm=None, skip_nonfinite=False))[3]
    assert not a.controls_enabled and not b.controls_enabled
    assert torch.equal(a.flat_p, b.flat_p)
    for name in _my_moments(kind, a):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert a.stats.tolist() == [0.0, 0.0, 0.0, 0.0]                 # the old entry points do not know the buffer


# ---- 6.-8. inside the train step ---------------------------------------------------------------------------------------
N, W, H, MULTI, B, T = 20, 12, 3, 5, 4, 120


def _quadruple(view):              # three more ranks holding identical gradients (tests/test_hip_schedule.py)
    view.mul_(4.0)


_quadruple.world = 4


def _model_and_opt(kind, controls):
    from stemgnn_amd import Model
    from stemgnn_amd.optim import FusedAdam, FusedRMSprop
    torch.manual_seed(7)
    model = Model(N, 2, W, MULTI, horizon=H, dropout_rate=0.0).to(DEV).train()
    opt = (FusedAdam if kind == "adam" else FusedRMSprop)(model.parameters(), lr=1e-3, **controls)
    return model, opt


def _train(kind, controls, graph, steps=range(6), collective_fn=None, one_graph=None, pair=None, per_step=None):
    from stemgnn_amd.engine import TrainStep
    g = torch.Generator().manual_seed(2)
    series = torch.randn(T, N, generator=g).to(DEV)
    hi = (torch.randint(0, T - W - H, (6, B), generator=g) + W).to(DEV)
    model, opt = pair if pair is not None else _model_and_opt(kind, controls)
    world = int(getattr(collective_fn, "world", 1)) if collective_fn is not None else 1
    step = TrainStep(model, opt, B, W, H, N, series=series, world=world, graph=graph, collective_fn=collective_fn,
                     one_graph=one_graph, schedule_check=False)
    for i in steps:
        step.run_indices(hi[i])
        if per_step is not None:
            per_step(opt)
    torch.cuda.synchronize()
    return model, opt, step


@functools.lru_cache(maxsize=None)
def _median_norm(kind):
    """The median of the 6 gradient norms of an eager run that takes the norm but never clips (max_grad_norm = 1e30)."""
    norms = []
    _train(kind, dict(max_grad_norm=1e30), graph=False, per_step=lambda opt: norms.append(opt.grad_report()["norm"]))
    assert len(norms) == 6 and all(np.isfinite(v) and v > 0 for v in norms), norms
    s = sorted(norms)
    return 0.5 * (s[2] + s[3])


@pytest.mark.parametrize("kind", ["adam", "rmsprop"])
def test_train_step_clips_inside_the_graph_and_matches_eager(kind):
    """TrainStep with max_grad_norm at the median norm of the unclipped run, so that some steps clip and some do not: the
    captured step gives the eager step's parameters, and the SAME clipped count -- the capture's warm-up steps are rolled back
    out of the counters too."""
    bound = _median_norm(kind)
    outs = []
    for graph in (True, False):
        _, opt, step = _train(kind, dict(max_grad_norm=bound), graph=graph)
        assert step.mode.startswith("hipgraph") == graph, step.mode
        outs.append((opt.flat_p.clone(), opt.grad_report()))
    print(kind, "bound", bound, "reports", outs[0][1], outs[1][1])
    assert relerr(outs[0][0], outs[1][0]) < 1e-6
    assert outs[0][1]["clipped_steps"] == outs[1][1]["clipped_steps"]
    assert 0 < outs[1][1]["clipped_steps"] < 6, outs[1][1]
    assert outs[0][1]["skipped_steps"] == 0 and outs[1][1]["skipped_steps"] == 0


DP_SHAPE = dict(N=228, W=12, H=3, multi=5, B=32, T=800)        # tests/test_hip_schedule.py's, where every form is exercised


def _train_dp(controls, collective_fn=None, one_graph=None, graph=True, per_step=None, steps=6):
    """tests/test_hip_schedule.py::_train with the controls: the headline shape, real dropout, the device-side window queue."""
    from stemgnn_amd import Model, ops
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop
    c = DP_SHAPE
    torch.manual_seed(0)
    model = Model(c["N"], 2, c["W"], c["multi"], horizon=c["H"]).to(DEV).train()        # dropout 0.5
    model.set_dropout_seed(99)
    opt = FusedRMSprop(model.parameters(), lr=1e-4, eps=1e-8, **controls)
    g = torch.Generator().manual_seed(7)
    series = torch.randn(c["T"], c["N"], generator=g).to(DEV)
    total = steps + 1
    hi = (torch.randint(0, c["T"] - c["W"] - c["H"], (total * c["B"],), generator=g) + c["W"]).to(DEV)
    world = int(getattr(collective_fn, "world", 2)) if collective_fn is not None else 1
    step = TrainStep(model, opt, c["B"], c["W"], c["H"], c["N"], series=series, world=world, graph=graph,
                     collective_fn=collective_fn, one_graph=one_graph, order_capacity=total * c["B"], schedule_check=False)
    step.load_order(hi)
    for _ in range(total):
        step.run_next()
        if per_step is not None:
            per_step(opt)
    torch.cuda.synchronize()
    ops.check_gru_status(torch.device(DEV))
    ops.check_gather_status(torch.device(DEV))
    return opt, step


def test_clipping_sees_the_averaged_gradient_in_every_data_parallel_form():
    """A stand-in collective that multiplies the gradients by 4 with world = 4 (x 4 and x 1/4 are exact): the one-graph
    two-range form, the two-graph form and the plain single-rank step must give the same bits.  A norm taken before grad_scale
    would clip four times harder.  The bound is the median norm of an unclipped eager run of the same 7 steps."""
    norms = []
    _train_dp(dict(max_grad_norm=1e30), graph=False, per_step=lambda opt: norms.append(opt.grad_report()["norm"]))
    assert len(norms) == 7 and all(np.isfinite(v) and v > 0 for v in norms), norms
    bound = sorted(norms)[3]
    controls = dict(max_grad_norm=bound, weight_decay=1e-2)
    o_plain, s_plain = _train_dp(controls)
    o_one, s_one = _train_dp(controls, _quadruple, one_graph=True)
    o_two, s_two = _train_dp(controls, _quadruple, one_graph=False)
    o_eager, s_eager = _train_dp(controls, _quadruple, graph=False)
    assert s_plain.mode == "hipgraph(whole step)", s_plain.mode
    assert s_one.mode == "hipgraph(whole step incl. rccl all-reduce)", (s_one.mode, s_one.schedule)
    assert s_two.mode.startswith("hipgraph(fwd+bwd)"), s_two.mode
    assert s_eager.mode == "eager"
    reports = [o.grad_report() for o in (o_plain, o_one, o_two, o_eager)]
    print("norms", norms, "bound", bound, reports)
    assert 0 < reports[0]["clipped_steps"] < 7, reports[0]
    for o, rep in zip((o_one, o_two), reports[1:3]):
        assert torch.equal(o.flat_p, o_plain.flat_p), float((o.flat_p - o_plain.flat_p).abs().max())
        assert torch.equal(o.square_avg, o_plain.square_avg)
        assert rep == reports[0]
    # the eager collective form against the captured ones: the bar of the graph-vs-eager comparisons (tests/test_hip_tail.py)
    assert relerr(o_eager.flat_p, o_plain.flat_p) < 1e-6
    assert reports[3]["clipped_steps"] == reports[0]["clipped_steps"] and reports[3]["skipped_steps"] == 0


@pytest.mark.parametrize("kind", ["rmsprop", "adam"])
def test_state_dict_resumes_bit_for_bit(kind):
    """3 eager steps, state_dict() of model and optimizer into a fresh model and optimizer, 3 more steps == 6 uninterrupted
    steps, bit for bit, on the parameters, the moments, Adam's step count and the controls' counters; the learning rate (halved
    after step 2 by a scheduler the resumed run does not have) travels with the state."""
    from stemgnn_amd import Model
    controls = dict(max_grad_norm=_median_norm(kind), weight_decay=1e-2, skip_nonfinite=True)

    def halve_lr_after_step_2():
        seen = []

        def hook(opt):
            seen.append(1)
            if len(seen) == 2:
                opt.param_groups[0]["lr"] *= 0.5
        return hook

    _, whole, _ = _train(kind, controls, graph=False, per_step=halve_lr_after_step_2())
    model_a, opt_a, _ = _train(kind, controls, graph=False, steps=range(3), per_step=halve_lr_after_step_2())
    sd_model = {k: v.detach().clone() for k, v in model_a.state_dict().items()}
    sd_opt = opt_a.state_dict()
    assert set(sd_opt["flat"]) >= {"square_avg", "stats", "lr"} and sd_opt["flat"]["lr"] == 5e-4
    if kind == "adam":
        assert float(sd_opt["flat"]["_step_dev"]) == 3.0 and "exp_avg" in sd_opt["flat"]
    torch.manual_seed(123)                                        # other initial weights: everything must come from the state
    model_b = Model(N, 2, W, MULTI, horizon=H, dropout_rate=0.0)
    model_b.load_state_dict(sd_model)
    model_b.to(DEV).train()
    opt_b = type(opt_a)(model_b.parameters(), lr=1e-3)            # default controls: they come back with the param group
    opt_b.load_state_dict(sd_opt)
    assert opt_b.param_groups[0]["lr"] == 5e-4 and float(opt_b._lr_dev) == np.float32(5e-4)
    assert opt_b.param_groups[0]["max_grad_norm"] == controls["max_grad_norm"] and opt_b.controls_enabled
    for p in model_b.parameters():                                # parameters stay views of flat_p, gradients bucket views
        assert opt_b.flat_p.data_ptr() <= p.data_ptr() < opt_b.flat_p.data_ptr() + 4 * opt_b.numel
    opt_b._check_grad_views()
    _train(kind, controls, graph=False, steps=range(3, 6), pair=(model_b, opt_b))
    assert torch.equal(opt_b.flat_p, whole.flat_p), float((opt_b.flat_p - whole.flat_p).abs().max())
    for name in ("square_avg", "stats") + (("exp_avg", "_step_dev") if kind == "adam" else ()):
        assert torch.equal(getattr(opt_b, name), getattr(whole, name)), name
    assert opt_b.grad_report() == whole.grad_report()
    if kind == "adam":
        assert float(opt_b._step_dev) == 6.0


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def test_train_adapter_hands_the_controls_on_and_logs_the_counts(tmp_path, capsys):
    from stemgnn_amd import Model, trainer
    n, w, h, multi, bs, ntrain = N, W, H, MULTI, 8, 100
    raw = synthetic_series(140, n, 5)
    base = dict(window_size=w, horizon=h, multi_layer=multi, device=DEV, norm_method="z_score", optimizer="RMSProp", lr=1e-3,
                decay_rate=0.5, exponential_decay_step=5, batch_size=bs, epoch=1, validate_freq=1, early_stop=False,
                hipgraph=True)
    factory = lambda *a, **k: Model(*a, dropout_rate=0.0, **k)                      # noqa: E731
    steps = -(-(ntrain - w - h + 1) // bs)

    torch.manual_seed(0)
    args = types.SimpleNamespace(**base, max_grad_norm=1e-3, weight_decay=1e-2, skip_nonfinite=True)
    trainer.train(raw[:ntrain], raw[ntrain:], args, str(tmp_path / "a"), model_factory=factory)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch 0:")]
    assert len(line) == 1, line
    m = re.fullmatch(r"epoch 0: [\d.]+s  mean train loss [\d.]+  clipped (\d+)/(\d+), skipped (\d+)  \[.+\]", line[0])
    assert m is not None, line[0]
    # a bound of 1e-3 is far below any gradient norm of an untrained model: every step of the epoch clips -- and only those
    # (the capture's warm-up steps are not counted)
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (steps, steps, 0), line[0]

    torch.manual_seed(0)
    trainer.train(raw[:ntrain], raw[ntrain:], types.SimpleNamespace(**base), str(tmp_path / "b"), model_factory=factory)
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("epoch 0:")]
    assert len(line) == 1 and re.fullmatch(r"epoch 0: [\d.]+s  mean train loss [\d.]+  \[.+\]", line[0]), line
