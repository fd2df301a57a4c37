"""Inference-forward timing at the PEMS07 shape (N=228, W=12, H=3, multi=5, B=32): eager Model.forward under no_grad in eval
mode (GPU time and wall time), eager Model.predict, one engine.ForecastStep replay, and one validation pass over a 0.2 T split
(trainer.rolling_forecast against trainer.rolling_forecast_graph), each with the peak memory it allocates.  Prints one JSON
line.  Usage: python tools/infer_time.py [--reps 50]   (STEMGNN_DTYPE selects fp32 / bf16x2 as everywhere)."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--T", type=int, default=12672)          # PEMS07's length; the validation split is 0.2 T
    a = ap.parse_args()
    from oracle import stemgnn_oracle as O
    from stemgnn_amd import Model
    from stemgnn_amd.engine import ForecastStep
    from stemgnn_amd.forecast_dataloader import ForecastDataset, WindowLoader
    from stemgnn_amd.trainer import rolling_forecast, rolling_forecast_graph
    from tests.util import synthetic_series

    N, W, multi, H, B = 228, 12, 5, 3, 32
    dev = torch.device("cuda:0")
    model = Model(N, 2, W, multi, horizon=H)
    model.load_state_dict(O.det_state_dict(N, W, multi, H, seed=1))
    model.to(dev).eval()
    x = torch.randn(B, W, N, device=dev)
    res = {"shape": dict(N=N, W=W, H=H, multi=multi, B=B), "dtype": os.environ.get("STEMGNN_DTYPE", "f32")}

    def measure(fn, reps):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / reps * 1e6
        return dict(gpu_us=e0.elapsed_time(e1) / reps * 1e3, wall_us=wall,
                    peak_mb=(torch.cuda.max_memory_allocated() - before) / 2**20)

    def fwd():
        with torch.no_grad():
            model(x)

    res["forward_no_grad"] = measure(fwd, a.reps)
    res["predict"] = measure(lambda: model.predict(x), a.reps)
    series = torch.randn(1024, N, device=dev)
    fs = ForecastStep(model, B, W, H, series, order_capacity=B)
    hi = torch.full((B,), W, dtype=torch.int64, device=dev)

    def replay():
        fs.load_order(hi)
        fs.run_next()
    res["forecast_step_replay"] = measure(replay, a.reps)
    ds = ForecastDataset(synthetic_series(int(0.2 * a.T), N, seed=3), W, H, normalize_method="z_score", device=dev)
    res["validation_windows"] = len(ds)
    res["validation_eager"] = measure(lambda: rolling_forecast(model, WindowLoader(ds, batch_size=B), H), 3)
    res["validation_graph"] = measure(lambda: rolling_forecast_graph(model, ds, H, B), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
