"""Cost of adaptive conformal bands on a live forecast, at the PEMS07 shape (N=228, W=12, H=3, multi=5), batch 1, Q=3, a pass
horizon of 3 (one round) and of 12 (four rolling rounds), score window 256, for offsets per step pooled over the nodes
(`pooled`) and per step and node (`per_node`).  Per case, one call = LiveForecaster.push(one row) + forecast() (graph=True,
rearrange on), ending in the forecast tensor:
  static     a fitted ConformalCalibrator in force, never refitted (what a forecast costs without adapting bands)
  adaptive   the same forecaster after set_adaptive(AdaptiveConformal(window=256)): one ops.aci_update launch ahead of the replay,
             and the replay's second store (the raw slab)
  refit      the only way to adapting bands before: matured() + ConformalCalibrator.fit(ignore_nan=True) + set_calibrator ahead
             of every forecast (history 256, so that the refit sees the window the adaptive object keeps)
  update     the ops.aci_update launch alone (AdaptiveConformal.update), on a copy of the adaptive forecaster's full window
Every forecaster is first run for window + horizon + W rows, so the adaptive window is full and `refit` fits 256 - horizon
forecasts.  Two modes, as tools/live_time.py has them: `isolated` synchronises the device after every call, `back_to_back` only
at the end of a window of `--reps` calls; a window is timed by a host clock around work that ends in a device synchronise and
reported per call; the figure is the median of `--rounds` windows, the variants' windows alternate, spread = (max - min) / median.
Writes profiles/aci_time.txt-style text to stdout after one JSON line.
Usage: python tools/aci_time.py [--reps 100] [--rounds 7]"""
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
WINDOW = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the text report here")
    a = ap.parse_args()
    from stemgnn_amd import LiveForecaster, Model
    from stemgnn_amd.math_utils import AdaptiveConformal, ConformalCalibrator
    from tests.util import synthetic_series

    if not torch.cuda.is_available():
        raise SystemExit("aci_time.py measures on the GPU; none found")
    N, W, multi, H = 228, 12, 5, 3
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = Model(N, 2, W, multi, horizon=H, quantiles=TAUS).to(dev).eval()
    T = 1024
    series = np.asarray(synthetic_series(T, N, seed=3), dtype=np.float64)
    stat = dict(mean=series.mean(axis=0), std=series.std(axis=0))
    rows = [np.ascontiguousarray(series[t]) for t in range(T)]
    res = {"shape": dict(N=N, W=W, H=H, multi=multi, B=1, Q=len(TAUS), window=WINDOW), "reps": a.reps, "rounds": a.rounds,
           "cases": {}}

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
            for _ in range(10):
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

    for horizon in (3, 12):
        for grouping, per_node in (("pooled", False), ("per_node", True)):
            shape = (1, horizon, N if per_node else 1)

            def fitted():
                cal = ConformalCalibrator(TAUS, True, per_node)
                return cal.load_state_dict(dict(cal.state_dict(), offsets=torch.full(shape, 0.125),
                                                counts=torch.full(shape, 100, dtype=torch.int64)), device=dev)

            def live():
                return LiveForecaster(model, W, horizon, normalize_method="z_score", norm_statistic=dict(stat), history=WINDOW,
                                      rearrange=True, calibrator=fitted(), graph=True)

            static, adaptive, refit = live(), live(), live()
            ad = AdaptiveConformal(TAUS, window=WINDOW, per_step=True, per_node=per_node)
            adaptive.set_adaptive(ad)
            cal = ConformalCalibrator(TAUS, True, per_node)

            def call(lv):
                def fn():
                    lv.push(rows[lv.rows % T])
                    return lv.forecast()
                return fn

            def refit_call():
                refit.push(rows[refit.rows % T])
                fc, tg, _ = refit.matured()
                if fc.shape[0]:
                    refit.set_calibrator(cal.fit(tg, fc, ignore_nan=True))
                return refit.forecast()

            variants = {"static": call(static), "adaptive": call(adaptive), "refit": refit_call}
            for lv in (static, adaptive, refit):
                lv.push(series[:W])
            for _ in range(WINDOW + horizon + W):                            # fill the score window and the history slab
                for fn in variants.values():
                    fn()
            torch.cuda.synchronize()
            assert ad.n_done >= WINDOW and refit.matured()[0].shape[0] >= WINDOW - horizon
            slot = (adaptive.done % adaptive.history)
            # a copy of the full window with gamma = 0 (the same launch; alpha stays put however often the one origin is fed, so
            # every call runs the whole select and never one of the two early-out branches)
            alone = AdaptiveConformal(TAUS, gamma=0.0, window=WINDOW, per_step=True, per_node=per_node)
            alone.load_state_dict(ad.state_dict())
            issued, raw_rows, ring, origin = adaptive.out_forecast[slot].clone(), adaptive.out_raw[slot].clone(), \
                adaptive.ring_y.clone(), adaptive.done

            def update_alone():
                alone.update(None, issued, raw_rows, ring=ring, origin=origin)

            variants["update"] = update_alone
            for mode, isolated in (("isolated", True), ("back_to_back", False)):
                out = measure(variants, isolated)
                out["overhead_ms"] = round(out["adaptive"]["ms"] - out["static"]["ms"], 4)
                out["overhead_share"] = round(out["overhead_ms"] / out["static"]["ms"], 3)
                out["refit_overhead_ms"] = round(out["refit"]["ms"] - out["static"]["ms"], 4)
                out["replay_is_the_first"] = adaptive._replay is not None
                res["cases"][f"h{horizon}_{grouping}_{mode}"] = out
    print(json.dumps(res))
    lines = [f"adaptive conformal bands on a live forecast, PEMS07 shape N={N} W={W} H={H} multi={multi}, batch 1, Q=3, window "
             f"{WINDOW}; ms per call,",
             f"median of {a.rounds} windows of {a.reps} calls (host clock around work ending in a device synchronise), "
             "(max - min) / median in brackets",
             f"{'case':<28}{'static':>17}{'adaptive':>17}{'refit':>17}{'update alone':>17}{'adaptive-static':>17}{'share':>8}"
             f"{'refit-static':>14}"]
    for name, c in res["cases"].items():
        cell = lambda k: f"{c[k]['ms']:.4f} [{c[k]['spread']:.2f}]"      # noqa: E731
        lines.append(f"{name:<28}{cell('static'):>17}{cell('adaptive'):>17}{cell('refit'):>17}{cell('update'):>17}"
                     f"{c['overhead_ms']:>17.4f}{c['overhead_share']:>8.3f}{c['refit_overhead_ms']:>14.4f}")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
