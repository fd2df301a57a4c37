"""Cost of the scenario-event kernels, by the protocol of tools/ensemble_time.py: same process, results
checked equal first, alternating windows of device events, medians and the spread (max - min) / median.
Setting: the PEMS07 pass (N 228, horizon 12, S 64 paths, 2520 origins; --origins: fewer), 8 groups of mean speed, per-node
de-normalisation to mph.
  aggregate  ops.scenario_aggregate against the torch composition a user would write, (paths.double() * mul + add) @ W.T,
             origin chunk by origin chunk (--chunk) to bound its temporaries
  events     ops.scenario_events ("below 30 mph", min_run 3) on the 228 node columns (de-normalising) and on the 8 group columns,
             against comparisons, cumsum for the first passage, a run-length scan over the steps and sum(1), chunked the same way
  live       the same two event forms at count = 1 (LiveForecaster.event_odds' shape), M in {228, 8}
  bytes/s    the bytes each kernel has to move (its input once, its output once) over its call time, beside a `copy_` in the same
             process that reads and writes the same number of bytes in all
One JSON line, then a text report written to --out.
Usage: python tools/events_time.py [--origins 2520] [--chunk 252] [--reps 3] [--rounds 5] [--out profiles/events_time.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

N, H, S, R = 228, 12, 64, 8
SEED = 7
THRESHOLD, MIN_RUN = 30.0, 3


def event_window_ms(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def alternate(runs, reps, rounds, warm):
    names = list(runs)
    for v in names:
        event_window_ms(runs[v], warm)
    got = {v: [] for v in names}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            got[v].append(event_window_ms(runs[v], reps))
    return {v: dict(median=round(statistics.median(got[v]), 4),
                    spread=round((max(got[v]) - min(got[v])) / statistics.median(got[v]), 3)) for v in names}


def torch_aggregate(x, w, mul, add, chunk):
    out = torch.empty(x.shape[:-1] + (w.shape[0],), device=x.device, dtype=torch.float32)
    wt = w.t().contiguous()
    for c0 in range(0, x.shape[0], chunk):
        out[c0:c0 + chunk] = ((x[c0:c0 + chunk].double() * mul + add) @ wt).float()
    return out


def torch_events(x, thr, above, min_run, mul, add, chunk):
    count, s, h, m = x.shape
    counts = torch.empty(count, 2 * h + 1, m, device=x.device, dtype=torch.int32)
    for c0 in range(0, count, chunk):
        v = x[c0:c0 + chunk].double()
        if mul is not None:
            v = v * mul + add
        e = v > thr if above else v < thr                                        # [c, S, H, M]
        first = e & (e.cumsum(dim=2) == 1)
        cur = torch.zeros_like(e[:, :, 0], dtype=torch.int32)
        best = torch.zeros_like(cur)
        for k in range(h):                                                       # the run-length scan
            cur = (cur + 1) * e[:, :, k]
            best = torch.maximum(best, cur)
        counts[c0:c0 + chunk, :h] = e.sum(dim=1)
        counts[c0:c0 + chunk, h:2 * h] = first.sum(dim=1)
        counts[c0:c0 + chunk, 2 * h] = (best >= min_run).sum(dim=1)
    return counts


def kernel_times_us(run, reps, names):
    """device time per call of the named kernels of `run`, from torch.profiler; {} when it reports none"""
    from torch.profiler import ProfilerActivity, profile
    run()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(reps):
            run()
        torch.cuda.synchronize()
    out = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = getattr(ev, "cuda_time_total", 0.0)
        for name in names:
            if t and name in ev.key:
                out[name] = round(out.get(name, 0.0) + t / reps, 2)
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--origins", type=int, default=2520)
    ap.add_argument("--chunk", type=int, default=252)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "events_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("events_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import ops
    from stemgnn_amd.math_utils import group_weights
    g = torch.Generator().manual_seed(SEED)
    count = args.origins
    x = torch.randn(count, S, H, N, generator=g).to(dev)
    mul = (torch.rand(N, generator=g, dtype=torch.float64) * 10.0 + 8.0).to(dev)      # mph per normalised unit
    add = (torch.rand(N, generator=g, dtype=torch.float64) * 25.0 + 30.0).to(dev)
    w = group_weights([list(map(int, c)) for c in torch.arange(N).chunk(R)], N).to(dev)
    thr_n = torch.full((N,), THRESHOLD, dtype=torch.float64, device=dev)
    thr_r = torch.full((R,), THRESHOLD + 10.0, dtype=torch.float64, device=dev)
    res = {"shape": dict(N=N, horizon=H, S=S, origins=count, groups=R, chunk=args.chunk), "reps": args.reps, "rounds": args.rounds}

    # equality first, at the timed shape
    agg = ops.scenario_aggregate(x, w, mul, add)
    t_agg = torch_aggregate(x, w, mul, add, args.chunk)
    agg_diff = float(((agg - t_agg).abs() / t_agg.abs().clamp_min(1.0)).max())
    c_nodes = ops.scenario_events(x, thr_n, False, MIN_RUN, mul, add)
    c_groups = ops.scenario_events(agg, thr_r, False, MIN_RUN)
    equal = dict(nodes=bool(torch.equal(c_nodes, torch_events(x, thr_n, False, MIN_RUN, mul, add, args.chunk))),
                 groups=bool(torch.equal(c_groups, torch_events(agg, thr_r, False, MIN_RUN, None, None, args.chunk))))
    res["aggregate_max_relative_difference"] = agg_diff
    res["event_counts_equal"] = equal
    res["event_rates"] = dict(nodes=float(c_nodes[:, :H].double().mean() / S), groups=float(c_groups[:, :H].double().mean() / S))
    # one fp32 rounding on either side; a larger gap is a wrong result, not a time
    if agg_diff > 2.0 ** -22 or not all(equal.values()):
        raise SystemExit(f"the two sides disagree: aggregate {agg_diff}, counts equal {equal}")

    x1, agg1 = x[:1].contiguous(), agg[:1].contiguous()
    forms = {
        "aggregate": (lambda: ops.scenario_aggregate(x, w, mul, add), lambda: torch_aggregate(x, w, mul, add, args.chunk),
                      x.numel() * 4 + agg.numel() * 4),
        "events_nodes": (lambda: ops.scenario_events(x, thr_n, False, MIN_RUN, mul, add),
                         lambda: torch_events(x, thr_n, False, MIN_RUN, mul, add, args.chunk), x.numel() * 4 + c_nodes.numel() * 4),
        "events_groups": (lambda: ops.scenario_events(agg, thr_r, False, MIN_RUN),
                          lambda: torch_events(agg, thr_r, False, MIN_RUN, None, None, args.chunk),
                          agg.numel() * 4 + c_groups.numel() * 4),
        "live_nodes": (lambda: ops.scenario_events(x1, thr_n, False, MIN_RUN, mul, add),
                       lambda: torch_events(x1, thr_n, False, MIN_RUN, mul, add, 1), None),
        "live_groups": (lambda: ops.scenario_events(agg1, thr_r, False, MIN_RUN),
                        lambda: torch_events(agg1, thr_r, False, MIN_RUN, None, None, 1), None),
    }
    res["call_ms"], res["bandwidth"] = {}, {}
    for name, (hip, ref, nbytes) in forms.items():
        runs = {"hip": hip, "torch": ref}
        if nbytes is not None:
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            runs["copy"] = lambda s=src, d=dst: d.copy_(s)
        reps = args.reps if nbytes is not None else 20 * args.reps
        r = alternate(runs, reps, args.rounds, 1)
        r["hip_over_torch"] = round(r["hip"]["median"] / r["torch"]["median"], 4)
        res["call_ms"][name] = r
        if nbytes is not None:
            hip_bw, copy_bw = nbytes / r["hip"]["median"] / 1e6, 2 * (nbytes // 2) / r["copy"]["median"] / 1e6
            res["bandwidth"][name] = dict(bytes=nbytes, hip_GBps=round(hip_bw, 1), copy_GBps=round(copy_bw, 1),
                                          hip_over_copy=round(hip_bw / copy_bw, 3))
            del src, dst
    try:
        kern = kernel_times_us(lambda: (forms["aggregate"][0](), forms["events_nodes"][0]()), args.reps, ("ag_kernel", "ev_kernel"))
    except Exception as e:                                                       # the profiler is an extra: the report says so
        kern = {"error": repr(e)[:200]}
    res["hip_kernels_us"] = kern
    print(json.dumps(res))
    lines = [f"scenario events, N {N}, horizon {H}, S {S}, {count} origins, {R} groups of mean speed (torch composition in fp64, "
             f"{args.chunk} origins per chunk)",
             f"[call_ms] median of {args.rounds} alternating windows of {args.reps} calls (live forms: {20 * args.reps}), ms per "
             "call, [(max - min) / median]"]
    for name, r in res["call_ms"].items():
        lines.append(f"  {name}")
        for k, v in r.items():
            lines.append(f"    {k:<18} " + (f"{v['median']:.4f} [{v['spread']:.2f}]" if isinstance(v, dict) else f"{v:.4f}"))
    lines.append("[bandwidth] input once + output once over the call time, beside a copy_ of the same total bytes (GB/s)")
    for name, b in res["bandwidth"].items():
        lines.append(f"  {name:<16} {b['bytes'] / 1e6:10.1f} MB   hip {b['hip_GBps']:8.1f}   copy {b['copy_GBps']:8.1f}   "
                     f"hip / copy {b['hip_over_copy']:.3f}")
    lines.append("[hip_kernels_us] device time per call of the kernels at the full pass (torch.profiler, a run of its own)")
    if not kern or "error" in kern:
        lines.append(f"  not measured: the profiler reported no kernel ({kern.get('error', 'none listed')})")
    for name, v in kern.items():
        if name != "error":
            lines.append(f"  {name:<18} {v:.2f}")
    lines.append(f"[agreement] aggregate: max |hip - torch| / max(|torch|, 1) = {agg_diff:.2e}; counts equal: nodes "
                 f"{equal['nodes']}, groups {equal['groups']}; share of (path, step) pairs in the event: nodes "
                 f"{res['event_rates']['nodes']:.3f}, groups {res['event_rates']['groups']:.3f}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
