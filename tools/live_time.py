"""Latency of live forecasting at the PEMS07 shape (N=228, W=12, H=3, multi=5) at batch 1, for a pass horizon of 3 (one round)
and of 12 (four rolling rounds), a point model and a Q=3 quantile model (rearranged + calibrated rows).  Per case, for the SAME
forecast of the window that ends at the newest row:
  live_replayed   LiveForecaster.push(one row) + forecast(), graph=True: one ingest launch and one hipGraph replay
  live_eager      the same with graph=False: the same kernels launched one by one
  composed        what there was before: the normalised row appended on the host into a resident fp32 series tensor (one row
                  copy), ops.window_gather of the newest window, the eager Model.predict / ops.roll_window loop at batch 1, and for
                  the quantile model torch.sort(dim=1) + calibrator.apply on the result.  The host-side imputation and fp64
                  normalisation of the raw row, which a user of that composition must also do, are NOT in its figure.
Every call ends in the forecast tensor.  Two modes: `isolated` synchronises the device after every call -- the latency a server
sees that forecasts once per arriving row -- and `back_to_back` only at the end of a window (throughput: the host runs ahead of
the device).  A window of `--reps` calls is timed by a host clock around work that ends in a device synchronise (the host's
launch work is part of a batch-1 call, so device events alone would miss it) and reported per call; the figure is the median
of `--rounds` windows, the variants' windows alternate, spread = (max - min) / median.
Writes profiles/live_time.txt-style text to stdout after one JSON line.
Usage: python tools/live_time.py [--reps 200] [--rounds 7]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAUS = (0.1, 0.5, 0.9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the text report here")
    a = ap.parse_args()
    from stemgnn_amd import LiveForecaster, Model, ops
    from stemgnn_amd.forecast_dataloader import ForecastDataset
    from stemgnn_amd.math_utils import ConformalCalibrator
    from tests.util import synthetic_series

    if not torch.cuda.is_available():
        raise SystemExit("live_time.py measures on the GPU; none found")
    N, W, multi, H = 228, 12, 5, 3
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    models = {"point": Model(N, 2, W, multi, horizon=H).to(dev).eval(),
              "quantile": Model(N, 2, W, multi, horizon=H, quantiles=TAUS).to(dev).eval()}
    T = 512
    series = np.asarray(synthetic_series(T, N, seed=3), dtype=np.float64)
    stat = dict(mean=series.mean(axis=0), std=series.std(axis=0))
    res = {"shape": dict(N=N, W=W, H=H, multi=multi, B=1, Q=len(TAUS)), "reps": a.reps, "rounds": a.rounds, "cases": {}}

    def window(fn, reps, isolated):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
            if isolated:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / reps

    def measure(variants, isolated):
        for fn in variants.values():
            for _ in range(20):
                fn()
        torch.cuda.synchronize()
        windows = {k: [] for k in variants}
        for _ in range(a.rounds):
            for k, fn in variants.items():
                windows[k].append(window(fn, a.reps, isolated))
        out = {}
        for k, v in windows.items():
            med = statistics.median(v)
            out[k] = dict(ms=round(med, 4), spread=round((max(v) - min(v)) / med, 3), windows_ms=[round(t, 4) for t in v])
        return out

    for kind, model in models.items():
        quant = kind == "quantile"
        for horizon in (3, 12):
            ds = ForecastDataset(series, W, horizon, normalize_method="z_score", norm_statistic=dict(stat), device=dev)
            rows = [np.ascontiguousarray(series[t]) for t in range(T)]
            norm_rows = [ds.data[t].cpu().clone() for t in range(T)]         # what the host-side composition appends
            cal = None
            if quant:                                                          # any fitted calibrator of the right shape
                cal = ConformalCalibrator(TAUS)
                shape = (1, horizon, 1)
                cal.load_state_dict(dict(cal.state_dict(), offsets=torch.full(shape, 0.125),
                                         counts=torch.full(shape, 100, dtype=torch.int64)), device=dev)
            kw = dict(normalize_method="z_score", norm_statistic=dict(stat), history=64)
            if quant:
                kw.update(rearrange=True, calibrator=cal)
            lives = {"live_replayed": LiveForecaster(model, W, horizon, graph=True, **kw),
                     "live_eager": LiveForecaster(model, W, horizon, graph=False, **kw)}
            for live in lives.values():
                live.push(series[:W])
            resident = torch.zeros(T + 8, N, device=dev)
            resident[:W].copy_(ds.data[:W])
            state = {"t": W}
            hi = torch.zeros(1, dtype=torch.int64, device=dev)
            y_unused = torch.zeros(1, 1, N, device=dev)
            steps_shape = (1,) + ((len(TAUS),) if quant else ()) + (horizon, N)

            def composed():
                t = state["t"]
                if t >= T:                                                    # wrap: the series is replayed from its start
                    t = W
                resident[t].copy_(norm_rows[t])                               # the append: one row, host to device
                t += 1
                state["t"] = t
                hi.fill_(t)
                x, _ = ops.window_gather(resident, hi, W, 1, y=y_unused)     # (the entry wants a target row: one spare row)
                steps = torch.empty(steps_shape, device=dev)
                done, win = 0, x
                while done < horizon:
                    out, _ = model.predict(win)
                    if quant:
                        win = ops.roll_window_quantile(win, out, steps, done, horizon, model.point_index)
                    else:
                        win = ops.roll_window(win, out, steps, done, horizon)
                    done += min(horizon - done, out.shape[-2])
                if quant:
                    steps = cal.apply(torch.sort(steps, dim=1).values)
                return steps[0]

            def live_call(live):
                def call():
                    live.push(rows[live.rows % T])
                    return live.forecast()
                return call

            # the three give the same forecast for the same window (checked once, on the first window after the warm start)
            want = composed()
            same = {k: bool(torch.equal(live_call(live)().view(torch.int32), want.view(torch.int32))) for k, live in lives.items()}
            variants = {"composed": composed, **{k: live_call(live) for k, live in lives.items()}}
            for mode, isolated in (("isolated", True), ("back_to_back", False)):
                out = measure(variants, isolated)
                out["same_bits_as_composed"] = same
                out["replayed_over_composed"] = round(out["live_replayed"]["ms"] / out["composed"]["ms"], 3)
                out["replayed_over_eager"] = round(out["live_replayed"]["ms"] / out["live_eager"]["ms"], 3)
                res["cases"][f"{kind}_h{horizon}_{mode}"] = out
    print(json.dumps(res))
    lines = [f"live forecasting latency, PEMS07 shape N={N} W={W} H={H} multi={multi}, batch 1; ms per push(one row) + forecast(),",
             f"median of {a.rounds} windows of {a.reps} calls (host clock around work ending in a device synchronise), "
             "(max - min) / median in brackets",
             f"{'case':<28}{'composed':>18}{'live eager':>18}{'live replayed':>18}{'replay/composed':>17}{'replay/eager':>14}  same bits"]
    for name, c in res["cases"].items():
        cell = lambda k: f"{c[k]['ms']:.4f} [{c[k]['spread']:.2f}]"      # noqa: E731
        lines.append(f"{name:<28}{cell('composed'):>18}{cell('live_eager'):>18}{cell('live_replayed'):>18}"
                     f"{c['replayed_over_composed']:>17.3f}{c['replayed_over_eager']:>14.3f}  {c['same_bits_as_composed']}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
