"""Cost of the scenario-reduction kernels, by the protocol of tools/ensemble_time.py: same process, results
compared first, alternating windows of device events, medians and the spread (max - min) / median.
Shapes: the PEMS07 pass (2520 origins, 64 paths, 12 steps, 228 nodes, keep 8; --origins: fewer), the same pass on 8 group
aggregates (L = 96 instead of 2736), and a live query at count = 1 on either.
  distances  stemgnn_scenario_distances alone, against torch.cdist on the paths in fp64 (origin chunk by origin chunk, --chunk, to
             bound the fp64 copy)
  reduce     stemgnn_scenario_reduce alone on those distances, against the greedy loop written in torch: vectorised over origins
             and candidates, no host decision per pick, `keep` x (minimum, sum, argmin, gather, minimum)
  both       ops.scenario_reduce (distances in scratch, then the picks) against cdist + loop
The torch side sums in another order, so it need not pick the same paths where two candidates are within rounding: the share of
origins with the same picks is reported; the distances, and the costs of the origins with the same picks, must agree to rounding.
One JSON line, then a text report written to --out.
Usage: python tools/reduce_time.py [--origins 2520] [--chunk 252] [--reps 3] [--rounds 5] [--out profiles/reduce_time.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

N, H, S, R, K = 228, 12, 64, 8, 8
SEED = 7


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


def torch_distances(x, chunk):
    count, s = x.shape[:2]
    D = torch.empty(count, s, s, device=x.device, dtype=torch.float64)
    for c0 in range(0, count, chunk):
        v = x[c0:c0 + chunk].double().flatten(2)
        D[c0:c0 + chunk] = torch.cdist(v, v)
    return D


def torch_greedy(D, keep):
    count, s, _ = D.shape
    m = torch.full((count, s), float("inf"), device=D.device, dtype=torch.float64)
    taken = torch.zeros(count, s, device=D.device, dtype=torch.bool)
    selected = torch.empty(count, keep, device=D.device, dtype=torch.int64)
    cost = torch.empty(count, keep, device=D.device, dtype=torch.float64)
    for i in range(keep):
        z = torch.minimum(m[:, :, None], D).sum(dim=1).masked_fill(taken, float("inf"))
        best, u = z.min(dim=1)
        selected[:, i], cost[:, i] = u, best / s
        taken.scatter_(1, u[:, None], True)
        m = torch.minimum(m, D.gather(2, u[:, None, None].expand(-1, s, 1)).squeeze(2))
    assign = D.gather(2, selected[:, None, :].expand(-1, s, -1)).argmin(dim=2)
    counts = torch.zeros(count, keep, device=D.device, dtype=torch.int64).scatter_add_(1, assign, torch.ones_like(assign))
    return selected, counts, assign, cost


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
    ap.add_argument("--out", default=os.path.join(root, "profiles", "reduce_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("reduce_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import _lib, ops
    from stemgnn_amd.math_utils import group_weights
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream                     # noqa: E731
    g = torch.Generator().manual_seed(SEED)
    count = args.origins
    x = torch.randn(count, S, H, N, generator=g).cumsum(dim=2).to(dev)            # random walks over the steps
    w = group_weights([list(map(int, c)) for c in torch.arange(N).chunk(R)], N).to(dev)
    agg = ops.scenario_aggregate(x, w)
    res = {"shape": dict(N=N, horizon=H, S=S, origins=count, groups=R, keep=K, chunk=args.chunk), "reps": args.reps,
           "rounds": args.rounds, "call_ms": {}, "agreement": {}}

    def hip_distances(v, out):
        _lib.check(lib.stemgnn_scenario_distances(v.data_ptr(), None, v.shape[0], S, v.shape[2] * v.shape[3], 0, out.data_ptr(),
                                                  stream()), "scenario_distances")

    def hip_reduce(D, outs):
        _lib.check(lib.stemgnn_scenario_reduce(D.data_ptr(), D.shape[0], S, K, *(o.data_ptr() for o in outs), stream()),
                   "scenario_reduce")

    shapes = {"pass_nodes": (x, False), "pass_groups": (agg, False), "live_nodes": (x[:1].contiguous(), True),
              "live_groups": (agg[:1].contiguous(), True)}
    for name, (v, live) in shapes.items():
        c = v.shape[0]
        D = torch.empty(c, S, S, device=dev, dtype=torch.float64)
        outs = (torch.empty(c, K, device=dev, dtype=torch.int32), torch.empty(c, K, device=dev, dtype=torch.int32),
                torch.empty(c, S, device=dev, dtype=torch.int32), torch.empty(c, K, device=dev, dtype=torch.float64))
        hip_distances(v, D)
        hip_reduce(D, outs)
        t_D = torch_distances(v, args.chunk)
        t_sel, t_counts, _, t_cost = torch_greedy(t_D, K)
        off = ~torch.eye(S, device=dev, dtype=torch.bool)                        # (cdist's diagonal is not exactly 0)
        d_diff = float(((D - t_D).abs() / D.clamp_min(1e-30))[:, off].max())
        alike = (outs[0].long() == t_sel).all(dim=1)
        same = float(alike.double().mean())
        c_diff = float(((outs[3] - t_cost).abs() / t_cost)[alike].max()) if bool(alike.any()) else 0.0
        res["agreement"][name] = dict(distance_max_relative_difference=d_diff, origins_with_the_same_picks=same,
                                      cost_max_relative_difference=c_diff)
        # the sums run in another order, so the picks may part where two candidates tie within rounding (the costs of such an
        # origin then differ by what the other pick is worth); where the picks are the same the costs differ by rounding and by
        # cdist's diagonal: its Gram expansion leaves a kept path about 1e-6 away from itself where the kernel has exactly 0
        if d_diff > 1e-9 or c_diff > 1e-6:
            raise SystemExit(f"{name}: the two sides disagree: distances {d_diff}, costs at equal picks {c_diff}")
        reps = 20 * args.reps if live else args.reps
        r = {}
        for part, runs in (("distances", {"hip": lambda: hip_distances(v, D), "torch": lambda: torch_distances(v, args.chunk)}),
                           ("reduce", {"hip": lambda: hip_reduce(D, outs), "torch": lambda: torch_greedy(t_D, K)}),
                           ("both", {"hip": lambda: ops.scenario_reduce(v, K),
                                     "torch": lambda: torch_greedy(torch_distances(v, args.chunk), K)})):
            t = alternate(runs, reps, args.rounds, 1)
            t["hip_over_torch"] = round(t["hip"]["median"] / t["torch"]["median"], 4)
            r[part] = t
        res["call_ms"][name] = r
        try:
            kern = kernel_times_us(lambda: (hip_distances(v, D), hip_reduce(D, outs)), args.reps,
                                   ("rd_distance_kernel", "rd_pick_kernel"))
        except Exception as e:                                                   # the profiler is an extra: the report says so
            kern = {"error": repr(e)[:200]}
        r["hip_kernels_us"] = kern
        del D, t_D
    print(json.dumps(res))
    lines = [f"scenario reduction, S {S}, horizon {H}, keep {K}; pass: {count} origins on N {N} nodes (L {H * N}) and on {R} group "
             f"means (L {H * R}); live: count 1 (torch: cdist in fp64, {args.chunk} origins per chunk, and a greedy loop)",
             f"[call_ms] median of {args.rounds} alternating windows of {args.reps} calls (live shapes: {20 * args.reps}), ms per "
             "call, [(max - min) / median]"]
    for name, r in res["call_ms"].items():
        lines.append(f"  {name}")
        for part in ("distances", "reduce", "both"):
            t = r[part]
            lines.append(f"    {part:<10} hip {t['hip']['median']:9.4f} [{t['hip']['spread']:.2f}]   torch "
                         f"{t['torch']['median']:9.4f} [{t['torch']['spread']:.2f}]   hip / torch {t['hip_over_torch']:.4f}")
        kern = r["hip_kernels_us"]
        if not kern or "error" in kern:
            lines.append(f"    kernels    not measured: the profiler reported no kernel ({kern.get('error', 'none listed')})")
        else:
            lines.append("    kernels    " + "   ".join(f"{k} {v:.2f} us" for k, v in kern.items())
                         + "   (torch.profiler, a run of its own)")
    lines.append("[agreement] hip against torch: max relative difference of the distances, share of origins with the same picks, "
                 "max relative difference of the costs where the picks are the same")
    for name, a in res["agreement"].items():
        lines.append(f"  {name:<12} {a['distance_max_relative_difference']:.2e}   {a['origins_with_the_same_picks']:.4f}   "
                     f"{a['cost_max_relative_difference']:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
