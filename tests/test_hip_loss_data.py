"""GPU: the data path of the missing-value feature -- targets gathered from a second series (`_pair` gathers),
ForecastDataset(missing=...), the masked metrics against numpy fp64, and a small DeviceTrainer fit with a robust loss."""
import numpy as np
import pytest
import torch

from tests.helpers.data_ref import masked_metrics_numpy
from tests.util import synthetic_series

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("N", [20, 7])                # the float4 and the scalar copy path
def test_pair_gather_eager_and_queue(N):
    from stemgnn_amd import ops
    T, W, H, B = 90, 12, 3, 4
    g = torch.Generator().manual_seed(N)
    sx = torch.randn(T, N, generator=g)
    sy = torch.randn(T, N, generator=g)
    sy[torch.rand(T, N, generator=g) < 0.25] = float("nan")
    order = torch.randperm(T - W - H + 1, generator=g)[:3 * B] + W
    want_x = torch.stack([sx[h - W:h] for h in order.tolist()])
    want_y = torch.stack([sy[h:h + H] for h in order.tolist()])
    assert bool(torch.isnan(want_y).any())
    sx, sy, order = sx.to(DEV), sy.to(DEV), order.to(DEV)
    x, y = ops.window_gather(sx, order, W, H, target_series=sy)
    assert torch.equal(x.cpu(), want_x)                              # x bitwise from series_x
    assert torch.equal(bits(y).cpu(), bits(want_y))                  # y bitwise from series_y, NaN included
    queue = torch.tensor([0, 0, 3 * B, 0], dtype=torch.int64, device=DEV)
    xq, yq = torch.empty(B, W, N, device=DEV), torch.empty(B, H, N, device=DEV)
    for k in range(3):
        ops.window_gather_queue(sx, order, queue, B, W, H, xq, yq, target_series=sy)
        assert torch.equal(xq.cpu(), want_x[k * B:(k + 1) * B])
        assert torch.equal(bits(yq).cpu(), bits(want_y[k * B:(k + 1) * B]))
    assert queue.tolist()[:3] == [3 * B, 0, 3 * B]
    # _pair(s, s) is the old entry
    x0, y0 = ops.window_gather(sx, order, W, H)
    x1, y1 = ops.window_gather(sx, order, W, H, target_series=sx)
    assert torch.equal(x0, x1) and torch.equal(y0, y1) and torch.equal(x0, x)
    queue.copy_(torch.tensor([0, 0, 3 * B, 0]))
    xa, ya = ops.window_gather_queue(sx, order, queue, B, W, H, torch.empty_like(xq), torch.empty_like(yq))
    queue.copy_(torch.tensor([0, 0, 3 * B, 0]))
    xb, yb = ops.window_gather_queue(sx, order, queue, B, W, H, torch.empty_like(xq), torch.empty_like(yq), target_series=sx)
    assert torch.equal(xa, xb) and torch.equal(ya, yb) and torch.equal(ya, y0[:B])
    ops.check_gather_status(sx.device)
    with pytest.raises(Exception, match="target_series"):
        ops.window_gather(sx, order, W, H, target_series=sy[:-1])


@pytest.mark.parametrize("method", ["z_score", "min_max"])
def test_forecast_dataset_missing_marks_targets_and_keeps_inputs_imputed(method):
    from stemgnn_amd.forecast_dataloader import ForecastDataset, _fill_na, mark_missing
    T, N, W, H = 40, 5, 8, 3
    raw = synthetic_series(T, N, seed=5)
    rng = np.random.RandomState(3)
    raw[rng.rand(T, N) < 0.12] = 0.0
    raw[rng.rand(T, N) < 0.08] = np.nan
    raw[0, 1] = 0.0                                                   # a leading gap (back-filled)
    marked, mask = mark_missing(raw, 0.0)
    assert mask.sum() > 20 and np.isnan(raw).any() and (raw == 0.0).any()
    ds = ForecastDataset(raw, W, H, normalize_method=method, missing=0.0, device=DEV)
    plain = ForecastDataset(_fill_na(marked), W, H, normalize_method=method, device=DEV)   # missing=None on the filled array
    assert plain.target is None and ds.target is not None
    assert torch.equal(ds.data, plain.data)
    idx = list(range(len(ds)))
    x, y = ds.gather(idx)
    x0, y0 = plain.gather(idx)
    assert torch.equal(x, x0) and not bool(torch.isnan(x).any())     # inputs imputed exactly as without the argument
    miss = torch.stack([torch.from_numpy(mask[h:h + H]) for h in ds.x_end_idx]).to(DEV)
    assert torch.equal(torch.isnan(y), miss)                          # NaN exactly at the marked positions
    assert torch.equal(bits(y)[~miss], bits(y0)[~miss])               # bitwise equal elsewhere
    xi, yi = ds[3]
    assert torch.equal(xi, x[3]) and torch.equal(torch.isnan(yi), miss[3])


@pytest.mark.parametrize("denorm", [False, True])
def test_masked_metrics_vs_numpy_fp64(denorm):
    from stemgnn_amd import math_utils
    count, H, N = 70, 3, 11                                           # crosses the 64-row chunk
    g = torch.Generator().manual_seed(9)
    t = torch.randn(count, H, N, generator=g) + 3.0
    f = t + 0.3 * torch.randn(count, H, N, generator=g)
    full = t.clone()
    t[torch.rand(count, H, N, generator=g) < 0.3] = float("nan")
    t[:, 1, 4] = float("nan")                                         # one (h, n) column entirely missing
    mul = add = None
    if denorm:
        mul, add = torch.rand(N, generator=g, dtype=torch.float64) + 0.5, torch.randn(N, generator=g, dtype=torch.float64)
    sc = math_utils.Scores(t.to(DEV), f.to(DEV), mul, add, ignore_nan=True)
    want = masked_metrics_numpy(t.numpy(), f.numpy(), None if mul is None else mul.numpy(), None if add is None else add.numpy())
    got = dict(overall=sc.get(), by_node=sc.get(by_node=True), by_step=sc.get(by_step=True),
               by_step_node=sc.get(by_step=True, by_node=True))
    for name in want:
        for nm, a, b in zip(("mape", "mae", "rmse"), got[name], want[name]):
            a, b = np.asarray(a), np.asarray(b)
            assert np.array_equal(np.isnan(a), np.isnan(b)), (name, nm)
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0, err_msg=f"{name} {nm}")
    for q in range(3):                                                # NaN there, finite everywhere else
        m = got["by_step_node"][q]
        assert np.isnan(m[1, 4]) and np.isfinite(np.delete(m.reshape(-1), 1 * N + 4)).all()
        assert np.isfinite(got["by_node"][q]).all() and np.isfinite(got["by_step"][q]).all() and np.isfinite(got["overall"][q])
    # with no NaN target the masked metrics are the unmasked ones
    a = math_utils.Scores(full.to(DEV), f.to(DEV), mul, add, ignore_nan=True)
    b = math_utils.Scores(full.to(DEV), f.to(DEV), mul, add)
    for kw in (dict(), dict(by_node=True), dict(by_step=True), dict(by_step=True, by_node=True)):
        for u, v in zip(a.get(**kw), b.get(**kw)):
            np.testing.assert_allclose(u, v, rtol=1e-12, atol=0)
    u = math_utils.evaluate(t.to(DEV), f.to(DEV), ignore_nan=True)
    if not denorm:
        np.testing.assert_allclose(u, [float(v) for v in want["overall"]], rtol=1e-12)


def test_small_fit_with_mae_and_missing_readings():
    from stemgnn_amd.trainer import DeviceTrainer
    rng = np.random.RandomState(0)
    series = synthetic_series(280, 6, seed=21)
    series[rng.rand(*series.shape) < 0.10] = 0.0                      # 10 % dead-sensor readings
    train, valid = series[:200], series[200:]
    torch.manual_seed(3)
    trainer = DeviceTrainer(6, 12, 3, 2, batch_size=16, lr=1e-3, loss="mae", missing=0.0, device=DEV)
    losses = {}

    def on_step(epoch, i, stepper):
        losses.setdefault(epoch, []).append(stepper.loss.clone())
    metrics, stat = trainer.fit(train, valid, 2, on_step=on_step, log=lambda *_: None)
    torch.cuda.synchronize()
    per_epoch = [float(torch.stack(losses[e]).double().mean()) for e in (0, 1)]
    print("mean train loss per epoch", per_epoch, {k: v for k, v in metrics.items() if not k.endswith("_node")})
    assert trainer.stepper.loss_kw == dict(kind="mae", huber_delta=1.0, ignore_nan=True)
    assert trainer.stepper.target_series is not None and bool(torch.isnan(trainer.stepper.target_series).any())
    for k in ("mae", "mape", "rmse", "mae_norm", "mape_norm", "rmse_norm"):
        assert np.isfinite(metrics[k]), (k, metrics[k])
    assert all(np.isfinite(v) for v in per_epoch)
    assert per_epoch[1] < per_epoch[0], per_epoch
    assert np.isfinite(stat["mean"]).all() and np.isfinite(stat["std"]).all()
