"""Cost of the ensemble scores, by the protocol of tools/scenario_time.py: same process, results checked
equal first, alternating windows of device events, medians and the spread (max - min) / median.
Setting: the PEMS07 shape (N 228, horizon 12), S 64 paths, 2520 origins (--origins: fewer if the torch side runs out of memory;
the report says which).
  call     ops.ensemble_scores (three launches) against the torch composition of the same numbers in fp64, the one a user would
           write: the energy pair term by paths.permute(0, 2, 1, 3) -> torch.cdist (timed in both compute modes: the default
           takes the Gram form |x|^2 + |x'|^2 - 2 x.x' at S > 25, `donot_use_mm` forms differences as the kernel does), the CRPS
           pair term through a sort over the paths and the rank identity, the ranks by comparisons + bincount, mean and variance
           by torch.mean / torch.var.  The composition runs origin chunk by origin chunk (--chunk) to bound its temporaries.
  parts    the composition's parts alone, and the kernels of the call alone from torch.profiler's device times (a run of its
           own, after the timed windows).
One JSON line, then a text report written to --out.
Usage: python tools/ensemble_time.py [--origins 2520] [--chunk 252] [--reps 3] [--rounds 5] [--out profiles/ensemble_time.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

N, H, S = 228, 12, 64
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


def torch_energy(y, x, mode):
    """sums over the chunk's rows of (sum_s ||x_s - y||, sum_s sum_s' ||x_s - x_s'||), fp64"""
    rows = x.permute(0, 2, 1, 3).reshape(-1, x.shape[1], x.shape[3])        # [c * H, S, N]
    pair = torch.cdist(rows, rows, compute_mode=mode).sum()
    first = torch.linalg.vector_norm(rows - y.reshape(-1, 1, y.shape[2]), dim=2).sum()
    return first, pair


def torch_crps(y, x):
    """sums over the chunk's elements of (sum_s |x_s - y|, sum_s sum_s' |x_s - x_s'|): sort + the rank identity"""
    s = x.shape[1]
    first = (x - y[:, None]).abs().sum()
    v = torch.sort(x, dim=1).values
    w = (2.0 * torch.arange(1, s + 1, device=x.device, dtype=x.dtype) - s - 1.0).view(1, s, 1, 1)
    return first, 2.0 * (v * w).sum()


def torch_ranks(y32, x32, hist):
    y = y32[:, None]
    rank = (x32 < y).sum(dim=1) + (x32 == y).sum(dim=1) // 2                 # [c, H, N]
    s1 = x32.shape[1] + 1
    step = torch.arange(rank.shape[1], device=rank.device).view(1, -1, 1)
    hist += torch.bincount((rank + step * s1).reshape(-1), minlength=hist.numel()).view_as(hist)


def torch_moments(y, x):
    mean = x.mean(dim=1)
    return ((mean - y) ** 2).sum(), x.var(dim=1, unbiased=True).sum()


def torch_scores(y32, x32, chunk, mode, parts=("energy", "crps", "ranks", "moments")):
    """the composition over origin chunks -> (out[6] overall, hist [H, S + 1]); parts: which of it runs (timing of one alone)"""
    count, s, h, n = x32.shape
    acc = torch.zeros(6, dtype=torch.float64, device=x32.device)
    hist = torch.zeros(h, s + 1, dtype=torch.int64, device=x32.device)
    for c0 in range(0, count, chunk):
        ys, xs = y32[c0:c0 + chunk], x32[c0:c0 + chunk]
        y, x = ys.double(), xs.double()
        if "energy" in parts:
            f, p = torch_energy(y, x, mode)
            acc[0] += f
            acc[1] += p
        if "crps" in parts:
            f, p = torch_crps(y, x)
            acc[2] += f
            acc[3] += p
        if "moments" in parts:
            se, var = torch_moments(y, x)
            acc[4] += se
            acc[5] += var
        if "ranks" in parts:
            torch_ranks(ys, xs, hist)
    el, rows, d = count * h * n, count * h, 2.0 * s * s
    out = torch.stack([(acc[2] / s - acc[3] / d) / el, (acc[0] / s - acc[1] / d) / rows, (acc[4] / el).sqrt(),
                       (acc[5] / el).sqrt()])
    return out, hist


def kernel_times_us(run, reps):
    """device time per call of every kernel of `run`, from torch.profiler; {} when it reports none"""
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
        if t and "en_" in ev.key:
            name = [p for p in ("en_energy_kernel", "en_marginal_kernel", "en_finish_kernel") if p in ev.key]
            if name:
                out[name[0]] = round(t / reps, 2)
    return out


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--origins", type=int, default=2520)
    ap.add_argument("--chunk", type=int, default=252)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "ensemble_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("ensemble_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import ops
    g = torch.Generator().manual_seed(SEED)
    count = args.origins
    y = torch.randn(count, H, N, generator=g).to(dev)
    x = (torch.randn(count, S, H, N, generator=g) * 0.8 + 0.1).to(dev)
    # equality first, at the timed shape
    out, hist = ops.ensemble_scores(y, x)
    res = {"shape": dict(N=N, horizon=H, S=S, origins=count, chunk=args.chunk), "reps": args.reps, "rounds": args.rounds}
    agree = {}
    for mode in ("donot_use_mm_for_euclid_dist", "use_mm_for_euclid_dist"):
        t_out, t_hist = torch_scores(y, x, args.chunk, mode)
        agree[mode] = [float(v) for v in ((t_out - out[:4]).abs() / out[:4].abs())]
        hist_equal = bool(torch.equal(t_hist, hist))
    res["relative_difference_hip_vs_torch"] = agree
    res["rank_histograms_equal"] = hist_equal
    # differences formed as the kernel forms them agree to the rounding of fp64 sums; a larger gap is a wrong result, not a time
    if not hist_equal or max(agree["donot_use_mm_for_euclid_dist"]) > 1e-9:
        raise SystemExit(f"the two sides disagree: histograms equal {hist_equal}, relative differences {agree}")
    runs = {"hip": lambda: ops.ensemble_scores(y, x),
            "torch": lambda: torch_scores(y, x, args.chunk, "donot_use_mm_for_euclid_dist"),
            "torch_gram": lambda: torch_scores(y, x, args.chunk, "use_mm_for_euclid_dist")}
    res["call_ms"] = alternate(runs, args.reps, args.rounds, 1)
    for k in ("torch", "torch_gram"):
        res["call_ms"]["hip_over_" + k] = round(res["call_ms"]["hip"]["median"] / res["call_ms"][k]["median"], 4)
    parts = {"torch_energy_diff": (("energy",), "donot_use_mm_for_euclid_dist"),
             "torch_energy_gram": (("energy",), "use_mm_for_euclid_dist"),
             "torch_crps": (("crps",), "donot_use_mm_for_euclid_dist"),
             "torch_ranks": (("ranks",), "donot_use_mm_for_euclid_dist"),
             "torch_moments": (("moments",), "donot_use_mm_for_euclid_dist")}
    res["parts_ms"] = alternate({k: (lambda p=p, m=m: torch_scores(y, x, args.chunk, m, p)) for k, (p, m) in parts.items()},
                                args.reps, args.rounds, 1)
    try:
        kern = kernel_times_us(lambda: ops.ensemble_scores(y, x), args.reps)
    except Exception as e:                                                   # the profiler is an extra: the report says so
        kern = {"error": repr(e)[:200]}
    res["hip_kernels_us"] = kern
    print(json.dumps(res))
    lines = [f"ensemble scores, N {N}, horizon {H}, S {S}, {count} origins (torch composition in fp64, {args.chunk} origins per chunk)",
             f"[call_ms] median of {args.rounds} alternating windows of {args.reps} calls, ms per call, [(max - min) / median]"]
    for name, r in res["call_ms"].items():
        lines.append(f"  {name:<22} " + (f"{r['median']:.4f} [{r['spread']:.2f}]" if isinstance(r, dict) else f"{r:.4f}"))
    lines.append("[parts_ms] the composition's parts alone, same protocol")
    for name, r in res["parts_ms"].items():
        lines.append(f"  {name:<22} {r['median']:.4f} [{r['spread']:.2f}]")
    lines.append("[hip_kernels_us] device time per call of the call's kernels (torch.profiler, a run of its own)")
    if not kern or "error" in kern:
        lines.append(f"  not measured: the profiler reported no kernel ({kern.get('error', 'none listed')})")
    for name, v in kern.items():
        if name != "error":
            lines.append(f"  {name:<22} {v:.2f}")
    lines.append(f"[agreement] |hip - torch| / |hip| of crps, energy, rmse, spread (rank histograms equal: {hist_equal})")
    for mode, v in agree.items():
        lines.append(f"  {mode:<30} " + "  ".join(f"{e:.2e}" for e in v))
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
