"""Cost of the weighted scenario-set kernels, by the protocol of tools/reduce_time.py: same process, results
compared first, alternating windows of device events, medians and the spread (max - min) / median.
Shapes: the PEMS07 pass (2520 origins, K = 8 kept paths with multiplicities over W = 64, 12 steps, 228 nodes; --origins: fewer),
the same pass on 8 group aggregates, and a live query at count = 1.  For each of the four entries, three ways to the same result:
  hip    the weighted entry on the K members (the reduction: distances of the K members, then stemgnn_scenario_reduce_weighted,
         8 -> 3)
  (a)    the only way there was: repeat_interleave to 64 equally likely paths, then the unweighted entry
  (b)    the weighted definition composed in torch (fp64, origin chunk by origin chunk, --chunk, to bound the pair tensors)
Bands and event counts must be equal; the scores agree to rounding; the reductions agree in cost to rounding wherever they pick
the same members ((a) picks among 64 paths of which many coincide, so its picks are mapped back to members).
One JSON line, then a text report written to --out.
Usage: python tools/weighted_time.py [--origins 2520] [--chunk 126] [--reps 3] [--rounds 5] [--out profiles/weighted_time.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

N, H, S, R, K, KEEP = 228, 12, 64, 8, 8, 3
TAUS = (0.05, 0.25, 0.5, 0.75, 0.95)
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


def replicate(x, mult):
    """[count, K, ...] with multiplicities [count, K] that sum to S -> [count, S, ...]: member k mult[k] times in a row"""
    count = x.shape[0]
    flat = torch.repeat_interleave(x.reshape((count * x.shape[1],) + tuple(x.shape[2:])), mult.reshape(-1).long(), dim=0)
    return flat.reshape((count, -1) + tuple(x.shape[2:]))


# ---- (b): the weighted definitions composed in torch ---------------------------------------------------------------------------
def torch_bands(x, mult, ranks):
    v, order = x.sort(dim=1, stable=True)
    cum = mult.long()[:, :, None, None].expand_as(x).gather(1, order).cumsum(dim=1)
    out = []
    for r in ranks:
        at = (cum >= r).int().argmax(dim=1, keepdim=True)
        out.append(v.gather(1, at))
    return torch.cat(out, dim=1)


def torch_events(x, mult, thr, min_run):
    e = x.double() > thr
    w = mult.long()[:, :, None, None]
    before = (e.cumsum(dim=2) - e.long()) > 0
    best = e.clone()
    run = e.clone()
    for _ in range(min_run - 1):                                                 # run[h]: min_run steps in a row ending at h
        run = torch.cat([torch.zeros_like(run[:, :, :1]), run[:, :, :-1]], dim=2) & e
        best = run
    return torch.cat([(e * w).sum(dim=1), ((e & ~before) * w).sum(dim=1), (best.any(dim=2, keepdim=True) * w).sum(dim=1)],
                     dim=1).to(torch.int32)


def torch_scores(y, x, mult, total, chunk):
    """-> (crps, energy, rmse, spread) overall, and hist [H, total + 1]"""
    count, k, h, n = x.shape
    sums = torch.zeros(4, device=x.device, dtype=torch.float64)
    hist = torch.zeros(h, total + 1, device=x.device, dtype=torch.int64)
    steps = torch.arange(h, device=x.device)[None, :, None]
    for c0 in range(0, count, chunk):
        v, t = x[c0:c0 + chunk].double(), y[c0:c0 + chunk].double()
        w = mult[c0:c0 + chunk].double()
        w1, ww = w[:, :, None, None], (w[:, :, None] * w[:, None, :])
        d = v[:, :, None] - v[:, None, :]                                        # [c, K, K, H, N]
        crps = (w1 * (v - t[:, None]).abs()).sum(dim=1) / total - (ww[:, :, :, None, None] * d.abs()).sum(dim=(1, 2)) / (2.0 * total ** 2)
        en = (w[:, :, None] * (v - t[:, None]).square().sum(dim=-1).sqrt()).sum(dim=1) / total \
            - (ww[:, :, :, None] * d.square().sum(dim=-1).sqrt()).sum(dim=(1, 2)) / (2.0 * total ** 2)
        mean = (w1 * v).sum(dim=1) / total
        var = (w1 * (v - mean[:, None]).square()).sum(dim=1) / (total - 1)
        sums += torch.stack([crps.sum(), en.sum(), (mean - t).square().sum(), var.sum()])
        wi = mult[c0:c0 + chunk].long()[:, :, None, None]
        raw, ry = x[c0:c0 + chunk], y[c0:c0 + chunk][:, None]
        rank = (wi * (raw < ry)).sum(dim=1) + (wi * (raw == ry)).sum(dim=1) // 2
        hist += torch.bincount((steps * (total + 1) + rank).reshape(-1), minlength=h * (total + 1)).reshape(h, total + 1)
    el = count * h * n
    return torch.stack([sums[0] / el, sums[1] / (count * h), (sums[2] / el).sqrt(), (sums[3] / el).sqrt()]), hist


def torch_greedy(D, mult, total, keep):
    count, s, _ = D.shape
    p = mult.double()
    m = torch.full((count, s), float("inf"), device=D.device, dtype=torch.float64)
    taken = mult <= 0
    selected = torch.empty(count, keep, device=D.device, dtype=torch.int64)
    cost = torch.empty(count, keep, device=D.device, dtype=torch.float64)
    for i in range(keep):
        z = (p[:, :, None] * torch.minimum(m[:, :, None], D)).sum(dim=1).masked_fill(taken, float("inf"))
        best, u = z.min(dim=1)
        selected[:, i], cost[:, i] = u, best / total
        taken = taken.scatter(1, u[:, None], True)
        m = torch.minimum(m, D.gather(2, u[:, None, None].expand(-1, s, 1)).squeeze(2))
    return selected, cost


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
    ap.add_argument("--chunk", type=int, default=126)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "weighted_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("weighted_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import ops, reduce_scenarios
    from stemgnn_amd.math_utils import group_weights
    g = torch.Generator().manual_seed(SEED)
    count = args.origins
    weights = group_weights([list(map(int, c)) for c in torch.arange(N).chunk(R)], N).to(dev)
    kept_parts, y_parts = [], []
    for c0 in range(0, count, args.chunk):                                       # the kept sets of a real reduction, batch by batch
        n = min(args.chunk, count - c0)
        full = torch.randn(n, S + 1, H, N, generator=g).cumsum(dim=2).to(dev)     # random walks; the last one is the truth
        kept_parts.append(reduce_scenarios(full[:, :S].contiguous(), K))
        y_parts.append(full[:, S].contiguous())
        del full
    x = torch.cat([k.paths for k in kept_parts]).contiguous()
    mult = torch.cat([k.counts for k in kept_parts]).contiguous()
    y = torch.cat(y_parts).contiguous()
    del kept_parts, y_parts
    assert bool((mult.sum(dim=1) == S).all())
    res = {"shape": dict(N=N, horizon=H, W=S, K=K, origins=count, groups=R, keep=KEEP, chunk=args.chunk), "reps": args.reps,
           "rounds": args.rounds, "call_ms": {}, "kernels_us": {}, "agreement": {}}
    shapes = {"pass_nodes": (x, y, mult, False), "pass_groups": (ops.scenario_aggregate(x, weights), ops.scenario_aggregate(y, weights),
                                                                 mult, False),
              "live_nodes": (x[:1].contiguous(), y[:1].contiguous(), mult[:1].contiguous(), True)}
    ranks = [ops.scenario_rank(t, S) for t in TAUS]
    for name, (v, t, m, live) in shapes.items():
        c, n = v.shape[0], v.shape[3]
        thr = v.double().mean(dim=(0, 1, 2)) + v.double().std(dim=(0, 1, 2))
        chunk = max(1, min(args.chunk, c))
        bands = lambda p: ops.scenario_bands(p, TAUS, 0, torch.empty(c, len(TAUS), H, n, device=dev))   # noqa: E731
        dist_reduce = lambda: ops.scenario_reduce_weighted(ops.scenario_distances(v), m, S, KEEP)       # noqa: E731
        rep_reduce = lambda: ops.scenario_reduce(replicate(v, m), KEEP)                                  # noqa: E731
        tor_reduce = lambda: torch_greedy(torch.cdist(v.double().flatten(2), v.double().flatten(2)), m, S, KEEP)   # noqa: E731
        parts = {
            "bands": {"hip": lambda: ops.weighted_bands(v, m, S, TAUS), "a": lambda: bands(replicate(v, m)),
                      "b": lambda: torch_bands(v, m, ranks)},
            "scores": {"hip": lambda: ops.weighted_scores(t, v, m, S), "a": lambda: ops.ensemble_scores(t, replicate(v, m)),
                       "b": lambda: torch_scores(t, v, m, S, chunk)},
            "events": {"hip": lambda: ops.weighted_events(v, m, S, thr, True, 2),
                       "a": lambda: ops.scenario_events(replicate(v, m), thr, True, 2), "b": lambda: torch_events(v, m, thr, 2)},
            "reduce": {"hip": dist_reduce, "a": rep_reduce, "b": tor_reduce},
        }
        # results first
        agree = {}
        b_hip, b_a, b_b = (parts["bands"][k]() for k in ("hip", "a", "b"))
        agree["bands_equal"] = [bool(torch.equal(b_hip, b_a)), bool(torch.equal(b_hip, b_b))]
        e_hip, e_a, e_b = (parts["events"][k]() for k in ("hip", "a", "b"))
        agree["events_equal"] = [bool(torch.equal(e_hip, e_a)), bool(torch.equal(e_hip, e_b))]
        (o_hip, h_hip), (o_a, h_a), (o_b, h_b) = (parts["scores"][k]() for k in ("hip", "a", "b"))
        agree["scores_max_relative_difference"] = [float(((o_hip[:4] - o_a[:4]).abs() / o_a[:4].abs()).max()),
                                                   float(((o_hip[:4] - o_b).abs() / o_b.abs()).max())]
        agree["hist_equal"] = [bool(torch.equal(h_hip, h_a)), bool(torch.equal(h_hip, h_b))]
        r_hip, r_a, r_b = dist_reduce(), rep_reduce(), tor_reduce()
        member = torch.arange(K, device=dev)[None].expand(c, K)
        of_path = replicate(member, m)                                           # the member every replicated path is
        a_sel = of_path.gather(1, r_a[0].long())
        same_a, same_b = (r_hip[0].long() == a_sel).all(dim=1), (r_hip[0].long() == r_b[0]).all(dim=1)
        agree["reduce_same_picks"] = [float(same_a.double().mean()), float(same_b.double().mean())]
        rel = lambda got, ok: float(((r_hip[3] - got).abs() / got.clamp_min(1e-300))[ok].max()) if bool(ok.any()) \
            else 0.0                                                             # noqa: E731
        agree["reduce_cost_max_relative_difference"] = [rel(r_a[3], same_a), rel(r_b[1], same_b)]
        res["agreement"][name] = agree
        if not all(agree["bands_equal"] + agree["events_equal"] + agree["hist_equal"]) or \
                max(agree["scores_max_relative_difference"]) > 1e-9 or max(agree["reduce_cost_max_relative_difference"]) > 1e-6:
            print(json.dumps(res))
            raise SystemExit(f"{name}: the three ways disagree: {agree}")
        reps = 20 * args.reps if live else args.reps
        r = {}
        for part, runs in parts.items():
            tm = alternate(runs, reps, args.rounds, 1)
            tm["hip_over_a"] = round(tm["hip"]["median"] / tm["a"]["median"], 4)
            tm["hip_over_b"] = round(tm["hip"]["median"] / tm["b"]["median"], 4)
            r[part] = tm
        try:
            kern = kernel_times_us(lambda: (parts["scores"]["hip"](), parts["reduce"]["hip"]()), args.reps,
                                   ("wt_energy_kernel", "wt_marginal_kernel", "wt_finish_kernel", "rd_distance_kernel",
                                    "wt_pick_kernel"))
        except Exception as e:                                                   # the profiler is an extra: the report says so
            kern = {"error": repr(e)[:200]}
        res["kernels_us"][name] = kern
        res["call_ms"][name] = r
    print(json.dumps(res))
    lines = [f"weighted scenario sets, K {K} kept paths with multiplicities over W {S}, horizon {H}; pass: {count} origins on N {N} "
             f"nodes and on {R} group means; live: count 1.  hip: the weighted entry; (a): repeat_interleave to {S} paths + the "
             f"unweighted entry; (b): the weighted definition in torch (fp64, {args.chunk} origins per chunk).  reduce: {K} -> {KEEP}, "
             "distances included on every side",
             f"[call_ms] median of {args.rounds} alternating windows of {args.reps} calls (live: {20 * args.reps}), ms per call, "
             "[(max - min) / median]"]
    for name, r in res["call_ms"].items():
        lines.append(f"  {name}")
        for part, tm in r.items():
            lines.append(f"    {part:<7} hip {tm['hip']['median']:9.4f} [{tm['hip']['spread']:.2f}]   (a) {tm['a']['median']:9.4f} "
                         f"[{tm['a']['spread']:.2f}]   (b) {tm['b']['median']:9.4f} [{tm['b']['spread']:.2f}]   hip / (a) "
                         f"{tm['hip_over_a']:.4f}   hip / (b) {tm['hip_over_b']:.4f}")
        kern = res["kernels_us"][name]
        if not kern or "error" in kern:
            lines.append(f"    kernels not measured: the profiler reported no kernel ({kern.get('error', 'none listed')})")
        else:
            lines.append("    kernels of scores and reduce: " + "   ".join(f"{k} {v:.2f} us" for k, v in kern.items())
                         + "   (torch.profiler, a run of its own)")
    lines.append("[agreement] hip against (a), (b): bands equal, event counts equal, histograms equal, max relative difference of "
                 "crps / energy / rmse / spread, share of origins with the same picks, max relative cost difference there")
    for name, a in res["agreement"].items():
        lines.append(f"  {name:<12} {a['bands_equal']} {a['events_equal']} {a['hist_equal']} "
                     f"{['%.1e' % v for v in a['scores_max_relative_difference']]} {['%.4f' % v for v in a['reduce_same_picks']]} "
                     f"{['%.1e' % v for v in a['reduce_cost_max_relative_difference']]}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
