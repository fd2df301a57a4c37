"""Serving time of a quantile model at the PEMS07 shape (N=228, W=12, H=3, multi=5, B=32, Q=3) over a 0.2 T validation split,
for a pass horizon of 3 (one round) and of 12 (four rolling rounds).  Per horizon, for the SAME result (rearranged, calibrated
rows [count, Q, horizon, N]):
  graph_call     trainer.rolling_quantile_forecast_graph(rearrange=True, calibrator=cal): one call, its capture included
  graph_pass     a kept engine.QuantileForecastStep: load_order + the replays of one pass (the steady state of a server)
  eager_compose  what there was before: trainer.rolling_forecast, then torch.sort(dim=1), then calibrator.apply
  graph_raw_pass the kept step with both stages off (what the epilogue's two stages cost inside the replay)
  point_pass     a kept engine.ForecastStep on a point model of the same shape (what the Q rows cost)
  epilogue       on the whole result at once: ops.quantile_finish(rearrange, offsets) against torch.sort + ops.conformal_apply,
                 with the bytes the former has to move (one read and one write of the result) over its time
Every figure is the median of `--rounds` windows of `--reps` repetitions, GPU time by events around work that ends in a
synchronise; the windows of the compared variants alternate.  Prints one JSON line.
Usage: python tools/quantile_serve_time.py [--reps 3] [--rounds 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAUS = (0.1, 0.5, 0.9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--T", type=int, default=12672)          # PEMS07's length; the validation split is 0.2 T
    a = ap.parse_args()
    from stemgnn_amd import Model, ops
    from stemgnn_amd.engine import ForecastStep, QuantileForecastStep
    from stemgnn_amd.forecast_dataloader import ForecastDataset, WindowLoader
    from stemgnn_amd.math_utils import ConformalCalibrator
    from stemgnn_amd.trainer import rolling_forecast, rolling_quantile_forecast_graph
    from tests.util import synthetic_series

    if not torch.cuda.is_available():
        raise SystemExit("quantile_serve_time.py measures on the GPU; none found")
    N, W, multi, H, B = 228, 12, 5, 3, 32
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    quant = Model(N, 2, W, multi, horizon=H, quantiles=TAUS).to(dev).eval()
    point = Model(N, 2, W, multi, horizon=H).to(dev).eval()
    series = synthetic_series(int(0.2 * a.T), N, seed=3)
    res = {"shape": dict(N=N, W=W, H=H, multi=multi, B=B, Q=len(TAUS)), "reps": a.reps, "epilogue_reps": 50,
           "rounds": a.rounds, "horizons": {}}

    def window(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def measure(variants, reps):
        """median ms per call of every variant; the variants' windows alternate"""
        for fn in variants.values():
            fn()
        torch.cuda.synchronize()
        windows = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                windows[k].append(window(fn, reps))
        return {k: dict(ms=round(statistics.median(v), 3), windows_ms=[round(t, 3) for t in v]) for k, v in windows.items()}

    def run_pass(step, hi_all):
        step.load_order(hi_all)
        while step.remaining > 0:
            step.run_next()

    for horizon in (3, 12):
        ds = ForecastDataset(series, W, horizon, normalize_method="z_score", device=dev)
        raw, target = rolling_forecast(quant, WindowLoader(ds, batch_size=B), horizon)
        ordered = torch.sort(raw, dim=1, stable=True).values
        cal = ConformalCalibrator(TAUS).fit(target, ordered)
        want = cal.apply(ordered)
        n = len(ds)
        kept = QuantileForecastStep(quant, B, W, horizon, ds.data, n, rearrange=True, calibrator=cal)
        kept_raw = QuantileForecastStep(quant, B, W, horizon, ds.data, n)
        kept_point = ForecastStep(point, B, W, horizon, ds.data, n)
        for step in (kept, kept_raw, kept_point):
            run_pass(step, ds.hi_all)
        torch.cuda.synchronize()
        same = bool(torch.equal(kept.result()[0].view(torch.int32), want.view(torch.int32)))

        def eager_compose():
            f, _ = rolling_forecast(quant, WindowLoader(ds, batch_size=B), horizon)
            return cal.apply(torch.sort(f, dim=1).values)

        out = measure({
            "graph_call": lambda: rolling_quantile_forecast_graph(quant, ds, horizon, B, rearrange=True, calibrator=cal),
            "eager_compose": eager_compose,
            "graph_pass": lambda: run_pass(kept, ds.hi_all),
            "graph_raw_pass": lambda: run_pass(kept_raw, ds.hi_all),
            "point_pass": lambda: run_pass(kept_point, ds.hi_all),
        }, a.reps)
        epi = measure({
            "quantile_finish": lambda: ops.quantile_finish(raw, rearrange=True, offsets=cal.offsets, pairs=cal.pairs),
            "sort_then_apply": lambda: ops.conformal_apply(torch.sort(raw, dim=1).values, cal.offsets, cal.pairs),
        }, 50)
        nbytes = 2 * raw.numel() * 4
        epi["bytes"] = nbytes
        epi["quantile_finish_gb_per_s"] = round(nbytes / (epi["quantile_finish"]["ms"] * 1e-3) / 1e9, 1)
        res["horizons"][str(horizon)] = dict(windows=n, batches=(n + B - 1) // B, replayed_equals_eager_composition=same,
                                             **out, epilogue=epi)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
