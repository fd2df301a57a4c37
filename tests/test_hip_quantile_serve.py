"""GPU: the serving epilogue of quantile forecasts (csrc/quantile_serve.hip) and the replayed rolling forecast built on it
(engine.QuantileForecastStep, trainer.rolling_quantile_forecast_graph).

Every reference is torch on the CPU or one of the project's earlier entries (ops.conformal_apply, ops.forecast_store,
trainer.rolling_forecast), never the code under test.  The epilogue selects, copies and does one fp32 operation that
stemgnn_conformal_apply does as well, so every comparison is one of bit patterns (int32 views: NaN payloads and the sign of
zero included) -- there is no tolerance in this file except the one named in test 4 for a forecast computed at two batch sizes."""
import types

import numpy as np
import pytest
import torch

from tests.util import relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TAUS = (0.1, 0.5, 0.9)
GROUPINGS = ((True, False), (False, False), (True, True), (False, True))          # (per_step, per_node)
GUARD = 64
SENTINEL = -777.25
# the values a column is drawn from: few, so ties are frequent; both zeros, both infinities, two NaNs of different payload
PLANTED = np.array([0x00000000, 0x80000000, 0x7f800000, 0xff800000, 0x7fc01234, 0xffc00001], np.uint32)
ORDINARY = np.array([-1.5, 0.5, 2.0], np.float32).view(np.uint32)
SHAPES = ((3, 1, 16), (2, 3, 5), (5, 2, 20), (1, 1, 1), (7, 3, 260))             # (count, H, N)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def sort_cpu(x):
    return torch.sort(x.detach().cpu(), dim=1, stable=True).values


def tied_columns(count, Q, H, N, seed):
    """[count, Q, H, N] fp32 on the CPU drawn from PLANTED + ORDINARY.  Three columns in four are then put in DESCENDING order
    (a random draw of Q = 2 values is in order half the time), so that most columns have to move."""
    rng = np.random.default_rng(seed)
    pool = np.concatenate([PLANTED, ORDINARY])
    x = torch.from_numpy(pool[rng.integers(0, pool.size, size=(count, Q, H, N))].view(np.float32).copy())
    return mostly_descending(x)


def mostly_descending(x):
    """three columns in four put in descending order: most columns of the result have to move"""
    count, _, H, N = x.shape
    col = torch.arange(count * H * N).reshape(count, 1, H, N)
    return torch.where((col % 4 != 3).expand_as(x), torch.flip(sort_cpu(x), dims=(1,)), x).contiguous()


def unsorted_share(x):
    """share of the columns that are not their own stable sort, bit for bit"""
    moved = (bits(x) != bits(sort_cpu(x))).any(dim=1)
    return float(moved.float().mean())


# ---- 1. rearrangement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", (1, 2, 3, 5, 8, 32))
def test_rearrangement_equals_stable_torch_sort_bit_for_bit(Q):
    from stemgnn_amd import ops
    from stemgnn_amd.math_utils import rearrange_quantiles
    for count, H, N in SHAPES:
        x = tied_columns(count, Q, H, N, seed=1000 * Q + N)
        want = sort_cpu(x)
        if Q > 1:                                  # (a column of one value is its own order: nothing can be asked of Q = 1)
            share = unsorted_share(x)
            assert share >= 0.5, (Q, count, H, N, share)
            assert x.numel() < 64 * Q or all(bool((x.numpy().view(np.uint32) == p).any()) for p in PLANTED)
        xd = x.to(DEV)
        got = ops.quantile_finish(xd, rearrange=True)
        assert got.data_ptr() != xd.data_ptr() and same_bits(xd, x), "out of place: the input is left alone"
        assert same_bits(got, want), (Q, count, H, N)
        same = rearrange_quantiles(xd, out=xd)     # in place: a thread reads its whole column before it writes
        assert same.data_ptr() == xd.data_ptr() and same_bits(xd, want), (Q, count, H, N)
        # idempotent, and without a stage a plain copy
        assert same_bits(ops.quantile_finish(xd, rearrange=True), want)
        assert same_bits(ops.quantile_finish(x.to(DEV)), x)


def test_rearrangement_of_a_misaligned_view_takes_the_scalar_path():
    """N % 4 == 0 but the base pointer is 4 bytes off 16-byte alignment: no 16-byte access may be made.  Input and output views
    sit inside sentinel-filled buffers; nothing outside them may change."""
    from stemgnn_amd import ops
    count, Q, H, N = 5, 3, 2, 20
    x = tied_columns(count, Q, H, N, seed=77)
    assert unsorted_share(x) >= 0.5
    want = sort_cpu(x)
    total = x.numel()

    def view(buf, shift):
        return buf[GUARD + shift:GUARD + shift + total].view(count, Q, H, N)

    for shift_in, shift_out in ((1, 0), (0, 1), (1, 1), (1, 3)):
        src = torch.full((total + 2 * GUARD + 4,), SENTINEL, device=DEV)
        dst = torch.full((total + 2 * GUARD + 4,), SENTINEL, device=DEV)
        xin, out = view(src, shift_in), view(dst, shift_out)
        assert xin.data_ptr() % 16 == 4 * shift_in and out.data_ptr() % 16 == 4 * shift_out
        xin.copy_(x)
        ops.quantile_finish(xin, rearrange=True, out=out)
        torch.cuda.synchronize()
        assert same_bits(out, want) and same_bits(xin, x), (shift_in, shift_out)
        for buf, shift in ((src, shift_in), (dst, shift_out)):
            assert bool((buf[:GUARD + shift] == SENTINEL).all()) and bool((buf[GUARD + shift + total:] == SENTINEL).all())
    # in place on the misaligned view
    src = torch.full((total + 2 * GUARD + 4,), SENTINEL, device=DEV)
    xin = view(src, 1)
    xin.copy_(x)
    ops.quantile_finish(xin, rearrange=True, out=xin)
    torch.cuda.synchronize()
    assert same_bits(xin, want)
    assert bool((src[:GUARD + 1] == SENTINEL).all()) and bool((src[GUARD + 1 + total:] == SENTINEL).all())


# ---- 2. the calibration stage ---------------------------------------------------------------------------------------------------
def pairs_of(Q):
    return tuple((i, Q - 1 - i) for i in range(Q // 2))


@pytest.mark.parametrize("N", (5, 8))
@pytest.mark.parametrize("Q", (2, 5))
def test_calibration_stage_equals_conformal_apply_bit_for_bit(Q, N):
    from stemgnn_amd import ops
    count, H = 9, 3
    pairs = pairs_of(Q)
    rng = np.random.default_rng(10 * N + Q)
    x = mostly_descending(torch.from_numpy(rng.normal(size=(count, Q, H, N)).astype(np.float32)))
    x[0, 0, 0, 0], x[1, Q - 1, H - 1, N - 1] = float("nan"), float("inf")
    assert unsorted_share(x) >= 0.5
    xd, sorted_d = x.to(DEV), sort_cpu(x).to(DEV)
    for per_step, per_node in GROUPINGS:
        shape = (len(pairs), H if per_step else 1, N if per_node else 1)
        offsets = rng.normal(size=shape).astype(np.float32)
        offsets.flat[0] = np.inf
        if offsets.size > 1:
            offsets.flat[-1] = -0.375                              # a negative offset narrows the band
        assert (offsets < 0).any() or offsets.size == 1
        od = torch.from_numpy(offsets).to(DEV)
        tag = (Q, N, per_step, per_node)
        # stage b alone
        want = ops.conformal_apply(xd, od, pairs, per_step, per_node)
        got = ops.quantile_finish(xd, offsets=od, pairs=pairs, per_step=per_step, per_node=per_node)
        assert same_bits(got, want) and same_bits(xd, x), tag
        if Q % 2:                                                  # the middle row is in no pair: untouched
            assert same_bits(got[:, Q // 2], x[:, Q // 2]), tag
        assert bool(torch.isinf(got[2:, 0, 0, 0]).all()), tag      # the +inf offset reached the low row
        # both stages: calibration acts on the REARRANGED column
        want2 = ops.conformal_apply(sorted_d, od, pairs, per_step, per_node)
        got2 = ops.quantile_finish(xd, rearrange=True, offsets=od, pairs=pairs, per_step=per_step, per_node=per_node)
        assert same_bits(got2, want2), tag
        assert not same_bits(got2, want), tag
        inplace = xd.clone()
        ops.quantile_finish(inplace, rearrange=True, offsets=od, pairs=pairs, per_step=per_step, per_node=per_node, out=inplace)
        assert same_bits(inplace, want2), tag


# ---- 3. quantile_store ----------------------------------------------------------------------------------------------------------
class Slab:
    """a slab of `shape` inside a NaN-filled guard region; untouched rows hold SENTINEL"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.full = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
        self.t = self.full[GUARD:GUARD + n].view(shape)
        self.t.fill_(SENTINEL)

    def guards_intact(self):
        return bool(torch.isnan(self.full[:GUARD]).all()) and bool(torch.isnan(self.full[-GUARD:]).all())


@pytest.mark.parametrize("HN", ((2, 20), (3, 5)), ids=("vec", "scalar"))
@pytest.mark.parametrize("start", (7, -2, 0))
def test_store_equals_forecast_store_per_quantile_row(HN, start):
    from stemgnn_amd import ops
    H, N = HN
    B, Q, cap = 6, 3, 10                                           # start 7: rows 7, 8, 9 land, three fall off the end
    steps = tied_columns(B, Q, H, N, seed=5 + N).to(DEV)
    target = torch.from_numpy(np.random.default_rng(N).normal(size=(B, H, N)).astype(np.float32)).to(DEV)
    target[1, 0, 0] = float("nan")
    pos = torch.tensor([start], dtype=torch.int64, device=DEV)
    inside = [b for b in range(B) if 0 <= start + b < cap]
    assert 0 < len(inside) < B or start == 0
    # reference: the existing point entry, one quantile row at a time
    ref_t, ref_q = Slab((cap, H, N)), [Slab((cap, H, N)) for _ in range(Q)]
    for q in range(Q):
        ops.forecast_store(steps[:, q].contiguous(), target, pos, ref_q[q].t, ref_t.t)
    out_f, out_t = Slab((cap, Q, H, N)), Slab((cap, H, N))
    ops.quantile_store(steps, target, pos, out_f.t, out_t.t)
    torch.cuda.synchronize()
    assert int(pos.item()) == start
    for q in range(Q):
        assert same_bits(out_f.t[:, q], ref_q[q].t), (q, start)
    assert same_bits(out_t.t, ref_t.t)
    assert out_f.guards_intact() and out_t.guards_intact()
    for b in range(B):
        row = start + b
        if b in inside:
            assert same_bits(out_f.t[row], steps[b]) and same_bits(out_t.t[row], target[b])
    untouched = [r for r in range(cap) if r - start not in range(B)]
    for r in untouched:
        assert bool((out_f.t[r] == SENTINEL).all()) and bool((out_t.t[r] == SENTINEL).all()), r
    # with both stages: the rows that land are quantile_finish's
    pairs, od = pairs_of(Q), torch.tensor([[[0.25]] * H], device=DEV)
    finished = ops.quantile_finish(steps, rearrange=True, offsets=od, pairs=pairs)
    out_f2, out_t2 = Slab((cap, Q, H, N)), Slab((cap, H, N))
    ops.quantile_store(steps, target, pos, out_f2.t, out_t2.t, rearrange=True, offsets=od, pairs=pairs)
    torch.cuda.synchronize()
    for b in inside:
        assert same_bits(out_f2.t[start + b], finished[b])
    for r in untouched:
        assert bool((out_f2.t[r] == SENTINEL).all()), r
    assert same_bits(out_t2.t, ref_t.t) and out_f2.guards_intact() and out_t2.guards_intact() and int(pos.item()) == start


# ---- 4. the model level -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def served():
    """An untrained quantile model on a resident random series, its eager rolling forecast (horizon 5 = three rounds of a
    horizon-2 model; batches of 6 with a ragged last one), computed once."""
    from stemgnn_amd import Model
    from stemgnn_amd.forecast_dataloader import ForecastDataset, WindowLoader
    from stemgnn_amd.trainer import rolling_forecast
    torch.manual_seed(4321)
    model = Model(16, 2, 8, 2, horizon=2, quantiles=TAUS).to(DEV)
    series = np.random.default_rng(11).normal(size=(64, 16))
    ds = ForecastDataset(series, window_size=8, horizon=5, device=DEV)
    B = 6
    assert len(ds) % B != 0 and len(ds) > 3 * B
    raw, target = rolling_forecast(model, WindowLoader(ds, batch_size=B), 5)
    torch.cuda.synchronize()
    assert tuple(raw.shape) == (len(ds), 3, 5, 16) and tuple(target.shape) == (len(ds), 5, 16)
    return types.SimpleNamespace(model=model, ds=ds, B=B, raw=raw.clone(), target=target.clone(),
                                 sorted=sort_cpu(raw).to(DEV))


def test_untrained_heads_cross_often(served):
    """The head rows are independent at initialisation: without this the tests below would show nothing."""
    from stemgnn_amd.math_utils import QuantileScores
    crossing = float(QuantileScores(served.target, served.raw, TAUS).crossing)
    print(f"crossing rate of the raw forecast: {crossing:.3f}")
    assert crossing > 0.1, crossing
    assert not same_bits(served.raw, served.sorted)


def test_replayed_pass_equals_the_eager_rolling_forecast(served):
    from stemgnn_amd.trainer import rolling_quantile_forecast_graph, score_forecast
    f, t = rolling_quantile_forecast_graph(served.model, served.ds, 5, served.B)
    torch.cuda.synchronize()
    assert same_bits(f, served.raw) and same_bits(t, served.target)
    a, b = score_forecast(f, t, quantiles=TAUS), score_forecast(served.raw, served.target, quantiles=TAUS)
    for k in ("mae", "mape", "rmse", "mae_node", "mape_node", "rmse_node", "mae_norm", "mape_norm", "rmse_norm"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_replayed_pass_rearranges_and_calibrates(served):
    from stemgnn_amd.math_utils import ConformalCalibrator, QuantileScores
    from stemgnn_amd.trainer import rolling_quantile_forecast_graph
    f, t = rolling_quantile_forecast_graph(served.model, served.ds, 5, served.B, rearrange=True)
    torch.cuda.synchronize()
    assert same_bits(f, served.sorted) and same_bits(t, served.target)
    assert float(QuantileScores(t, f, TAUS).crossing) == 0.0
    cal = ConformalCalibrator(TAUS).fit(served.target, served.sorted)           # fitted on REARRANGED forecasts: the rule
    assert tuple(cal.offsets.shape) == (1, 5, 1) and bool(torch.isfinite(cal.offsets).all())
    want = cal.apply(served.sorted)
    f, t = rolling_quantile_forecast_graph(served.model, served.ds, 5, served.B, rearrange=True, calibrator=cal)
    torch.cuda.synchronize()
    assert same_bits(f, want) and same_bits(t, served.target)
    assert not same_bits(f, served.sorted)
    # the calibrator alone acts on the raw rows
    f, _ = rolling_quantile_forecast_graph(served.model, served.ds, 5, served.B, calibrator=cal)
    assert same_bits(f, cal.apply(served.raw))


def test_eager_step_second_pass_and_capture(served):
    from stemgnn_amd.engine import QuantileForecastStep
    from stemgnn_amd.math_utils import ConformalCalibrator
    cal = ConformalCalibrator(TAUS).fit(served.target, served.sorted)
    want = cal.apply(served.sorted)
    out = {}
    for graph in (False, True):
        step = QuantileForecastStep(served.model, served.B, 8, 5, served.ds.data, len(served.ds), graph=graph, rearrange=True,
                                    calibrator=cal)
        for again in range(2):                                      # a second pass after load_order reuses the capture
            step.load_order(served.ds.hi_all)
            assert step.remaining == len(served.ds)
            while step.remaining > 0:
                step.run_next()
            torch.cuda.synchronize()
            f, t = step.result()
            assert same_bits(f, want) and same_bits(t, served.target), (graph, again)
        assert (step._replay is not None) == graph
        out[graph] = f.clone()
    assert same_bits(out[False], out[True])


def test_pass_from_a_fixed_graph(served):
    """adjacency=: every window is forecast from the same graph, so its forecast does not depend on the batch it is in.  Two batch
    sizes may take different launch paths inside the blocks (another summation order), so across batch sizes the comparison is
    2e-4 of the largest forecast -- twice the 1e-4 the model is held to against the fp64 oracle (BASELINE.json), each pass
    being within that of the same exact value; at one batch size the replayed pass equals the eager one bit for bit."""
    from stemgnn_amd.forecast_dataloader import WindowLoader
    from stemgnn_amd.trainer import rolling_forecast, rolling_quantile_forecast_graph
    G = served.model.latent_graph(served.ds.data[None, :8].contiguous())
    ref, _ = rolling_forecast(served.model, WindowLoader(served.ds, batch_size=served.B), 5, adjacency=G)
    f6, t6 = rolling_quantile_forecast_graph(served.model, served.ds, 5, served.B, adjacency=G)
    f4, t4 = rolling_quantile_forecast_graph(served.model, served.ds, 5, 4, adjacency=G)
    torch.cuda.synchronize()
    assert same_bits(f6, ref) and same_bits(t6, served.target) and same_bits(t4, served.target)
    assert not same_bits(f6, served.raw)
    err = relerr(f4, f6)
    print(f"adjacency: batch 4 against batch 6, relative difference {err:.2e} (bit-equal: {same_bits(f4, f6)})")
    assert err < 2e-4, err
