"""Cost of seasonal conformal calibration, by the protocol of tools/conformal_time.py and tools/live_time.py:
same process, results checked equal first, alternating windows, medians and the spread (max - min) / median.
  fit    PEMS07 validation shape count 2520, Q 3, H 3, N 228, period 288, 24 buckets, consecutive origins; all four groupings,
         masked (about 10 % NaN targets) and not:
           seasonal     ops.seasonal_fit, origin an int: a bucket's rows are enumerated
           seasonal_tensor  the same origins as an int64 tensor: a bucket's rows are found by skipping the others'
           composition  what a user writes today: 24 x (index_select of a bucket's rows + ops.conformal_fit).  The rows are
                        chosen by the bucket of their ORIGIN, which is the definition at step 0 only (later steps would
                        need a selection of their own: three times the work); it is timed as written and checked equal
                        to the seasonal fit at H = 1, where it is the definition
           unseasoned   ops.conformal_fit on the same tensors: the floor
  apply  [2520, 3, 3, 228]: ops.seasonal_apply against ops.conformal_apply and against 24 masked applies (torch.where)
  live   PEMS07, batch 1, Q 3, horizons 3 and 12: push(one row) + forecast() with a seasonal calibrator against the same with a
         static one, isolated (a synchronise after every call) and back to back; host clock around work ending in a synchronise.
         --sections live_static measures the static forecaster alone through the API that predates the feature, so the same
         file can be pointed at an older tree with --root.
One JSON line, then a text report.
Usage: python tools/seasonal_time.py [--sections fit,apply,live] [--root DIR] [--reps 50] [--rounds 9] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

COUNT, Q, H, N = 2520, 3, 3, 228
PERIOD, K, PHASE, ORIGIN0 = 288, 24, 100, 7
TAUS = (0.1, 0.5, 0.9)
PAIRS, COVERAGE = ((0, 2),), [0.9 - 0.1]
GROUPINGS = ((True, False), (False, False), (True, True), (False, True))


def event_window_us(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def host_window_ms(run, reps, isolated):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
        if isolated:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(runs, window, reps, rounds, warm):
    names = list(runs)
    for v in names:
        window(runs[v], warm)
    got = {v: [] for v in names}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            got[v].append(window(runs[v], reps))
    return {v: dict(median=round(statistics.median(got[v]), 3),
                    spread=round((max(got[v]) - min(got[v])) / statistics.median(got[v]), 3)) for v in names}


def fit_section(ops, args, dev):
    g = torch.Generator().manual_seed(3)
    y = torch.randn(COUNT, H, N, generator=g)
    f = (0.5 * y + 0.5 * torch.randn(COUNT, H, N, generator=g)).unsqueeze(1) + torch.tensor([-0.6, 0.0, 0.6]).view(1, Q, 1, 1)
    y_nan = y.clone()
    y_nan[torch.rand(y.shape, generator=g) < 0.1] = float("nan")
    y, y_nan, f = y.to(dev), y_nan.to(dev), f.contiguous().to(dev)
    season = (PERIOD, K, PHASE)
    bucket = (torch.arange(COUNT) + ORIGIN0 + PHASE) % PERIOD * K // PERIOD
    rows = [torch.nonzero(bucket == s).flatten().to(dev) for s in range(K)]
    assert all(r.numel() > 0 for r in rows)

    def composition(t, per_step, per_node, masked, tt=None, ff=None):
        tt, ff = (t, f) if tt is None else (tt, ff)
        return [ops.conformal_fit(tt.index_select(0, r), ff.index_select(0, r), PAIRS, COVERAGE, per_step, per_node,
                                  ignore_nan=masked) for r in rows]

    # equal first: at H = 1 a bucket's rows are the rows whose origin falls into it, so the composition IS the definition
    y1, f1 = y[:, :1].contiguous(), f[:, :, :1].contiguous()
    for per_step, per_node in GROUPINGS:
        got = ops.seasonal_fit(y1, f1, ORIGIN0, PAIRS, COVERAGE, season, per_step, per_node)
        want = composition(y1, per_step, per_node, False, y1, f1)
        assert torch.equal(got[0], torch.stack([w[0] for w in want])) and torch.equal(got[1], torch.stack([w[1] for w in want]))
    origins = (torch.arange(COUNT) + ORIGIN0).to(dev)              # the same origins as a tensor: the skipping form
    for per_step, per_node in GROUPINGS:
        a = ops.seasonal_fit(y_nan, f, ORIGIN0, PAIRS, COVERAGE, season, per_step, per_node, ignore_nan=True)
        b = ops.seasonal_fit(y_nan, f, origins, PAIRS, COVERAGE, season, per_step, per_node, ignore_nan=True)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    one = ops.seasonal_fit(y, f, ORIGIN0, PAIRS, COVERAGE, (1, 1, 0))
    base = ops.conformal_fit(y, f, PAIRS, COVERAGE)
    assert torch.equal(one[0][0], base[0]) and torch.equal(one[1][0], base[1])
    out = {}
    for per_step, per_node in GROUPINGS:
        for masked in (False, True):
            name = f"step{int(per_step)}_node{int(per_node)}" + ("_masked" if masked else "")
            t = y_nan if masked else y
            runs = {"seasonal": lambda: ops.seasonal_fit(t, f, ORIGIN0, PAIRS, COVERAGE, season, per_step, per_node,
                                                         ignore_nan=masked),
                    "seasonal_tensor": lambda: ops.seasonal_fit(t, f, origins, PAIRS, COVERAGE, season, per_step, per_node,
                                                                ignore_nan=masked),
                    "composition": lambda: composition(t, per_step, per_node, masked),
                    "unseasoned": lambda: ops.conformal_fit(t, f, PAIRS, COVERAGE, per_step, per_node, ignore_nan=masked)}
            r = alternate(runs, event_window_us, args.reps, args.rounds, 5)
            r["seasonal_over_composition"] = round(r["seasonal"]["median"] / r["composition"]["median"], 3)
            r["seasonal_over_unseasoned"] = round(r["seasonal"]["median"] / r["unseasoned"]["median"], 3)
            out[name] = r
    return out


def apply_section(ops, args, dev):
    g = torch.Generator().manual_seed(4)
    f = torch.randn(COUNT, Q, H, N, generator=g).to(dev)
    season = (PERIOD, K, PHASE)
    bucket = ((torch.arange(COUNT)[:, None] + torch.arange(H)[None, :] + ORIGIN0 + PHASE) % PERIOD * K // PERIOD).to(dev)
    masks = [(bucket == s)[:, None, :, None] for s in range(K)]
    out = {}
    for per_step, per_node in GROUPINGS:
        shape = (K, 1, H if per_step else 1, N if per_node else 1)
        offsets = torch.randn(shape, generator=g).to(dev)

        def masked_applies():
            res = f
            for s in range(K):
                res = torch.where(masks[s], ops.conformal_apply(f, offsets[s], PAIRS, per_step, per_node), res)
            return res

        got = ops.seasonal_apply(f, offsets, ORIGIN0, PAIRS, season, per_step, per_node)
        assert torch.equal(got.view(torch.int32), masked_applies().view(torch.int32))
        runs = {"seasonal": lambda: ops.seasonal_apply(f, offsets, ORIGIN0, PAIRS, season, per_step, per_node),
                "unseasoned": lambda: ops.conformal_apply(f, offsets[0], PAIRS, per_step, per_node),
                "masked_x24": masked_applies,
                "seasonal_rearranged": lambda: ops.seasonal_apply(f, offsets, ORIGIN0, PAIRS, season, per_step, per_node,
                                                                  rearrange=True),
                "finish_rearranged": lambda: ops.quantile_finish(f, rearrange=True, offsets=offsets[0], pairs=PAIRS,
                                                                 per_step=per_step, per_node=per_node)}
        r = alternate(runs, event_window_us, args.reps, args.rounds, 5)
        r["seasonal_over_unseasoned"] = round(r["seasonal"]["median"] / r["unseasoned"]["median"], 3)
        r["seasonal_over_masked_x24"] = round(r["seasonal"]["median"] / r["masked_x24"]["median"], 3)
        out[f"step{int(per_step)}_node{int(per_node)}"] = r
    return out


def live_section(args, dev, seasonal):
    from stemgnn_amd import LiveForecaster, Model
    from stemgnn_amd.math_utils import ConformalCalibrator
    from tests.util import synthetic_series
    Wn, multi = 12, 5
    torch.manual_seed(0)
    model = Model(N, 2, Wn, multi, horizon=H, quantiles=TAUS).to(dev).eval()
    T = 512
    series = np.asarray(synthetic_series(T, N, seed=3), dtype=np.float64)
    stat = dict(mean=series.mean(axis=0), std=series.std(axis=0))
    rows = [np.ascontiguousarray(series[t]) for t in range(T)]
    out = {}
    for horizon in (3, 12):
        static = ConformalCalibrator(TAUS)
        static.load_state_dict(dict(static.state_dict(), offsets=torch.full((1, horizon, 1), 0.125),
                                    counts=torch.full((1, horizon, 1), 100, dtype=torch.int64)), device=dev)
        kw = dict(normalize_method="z_score", norm_statistic=dict(stat), history=64, rearrange=True, graph=True)
        lives = {"static": LiveForecaster(model, Wn, horizon, calibrator=static, **kw)}
        if seasonal:
            from stemgnn_amd.math_utils import SeasonalConformalCalibrator
            cal = SeasonalConformalCalibrator(TAUS, PERIOD, K, PHASE)
            shape = (K, 1, horizon, 1)
            cal.load_state_dict(dict(cal.state_dict(), offsets=torch.full(shape, 0.125),
                                     counts=torch.full(shape, 100, dtype=torch.int64)), device=dev)
            lives["seasonal"] = LiveForecaster(model, Wn, horizon, **kw)
            lives["seasonal"].set_calibrator(cal, t_offset=ORIGIN0)
        for live in lives.values():
            live.push(series[:Wn])

        def call_of(live):
            def call():
                live.push(rows[live.rows % T])
                return live.forecast()
            return call

        calls = {k: call_of(v) for k, v in lives.items()}
        first = {k: c() for k, c in calls.items()}
        if seasonal:                                            # equal tables: the same rows whichever slice is taken
            assert torch.equal(first["static"].view(torch.int32), first["seasonal"].view(torch.int32))
        for mode, isolated in (("isolated", True), ("back_to_back", False)):
            r = alternate(calls, lambda fn, reps: host_window_ms(fn, reps, isolated), args.live_reps, args.rounds, 20)
            if seasonal:
                r["seasonal_over_static"] = round(r["seasonal"]["median"] / r["static"]["median"], 3)
            out[f"h{horizon}_{mode}"] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="fit,apply,live")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the tree whose stemgnn_amd is measured (default: this one)")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--live-reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="append the report to this file")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    if not torch.cuda.is_available():
        raise SystemExit("seasonal_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    sections = args.sections.split(",")
    res = {"root": os.path.relpath(os.path.abspath(args.root)), "shape": dict(count=COUNT, Q=Q, H=H, N=N, period=PERIOD, K=K),
           "reps": args.reps, "live_reps": args.live_reps, "rounds": args.rounds}
    if "fit" in sections or "apply" in sections:
        from stemgnn_amd import ops
    if "fit" in sections:
        res["fit_us"] = fit_section(ops, args, dev)
    if "apply" in sections:
        res["apply_us"] = apply_section(ops, args, dev)
    if "live" in sections:
        res["live_ms"] = live_section(args, dev, True)
    if "live_static" in sections:
        res["live_static_ms"] = live_section(args, dev, False)
    line = json.dumps(res)
    print(line)
    lines = []
    for key, unit in (("fit_us", "us"), ("apply_us", "us"), ("live_ms", "ms"), ("live_static_ms", "ms")):
        if key not in res:
            continue
        lines.append(f"[{key}] tree {res['root']}: median of {args.rounds} alternating windows, {unit} per call, "
                     "[(max - min) / median]")
        for name, r in res[key].items():
            cells = "  ".join(f"{k} {v['median']:.3f} [{v['spread']:.2f}]" if isinstance(v, dict) else f"{k} {v:.3f}"
                              for k, v in r.items())
            lines.append(f"  {name:<22} {cells}")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
