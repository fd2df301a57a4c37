"""Cost of the simultaneous-band kernel, by the protocol of tools/reduce_time.py: same process, results
compared first, alternating windows of device events, medians and the spread (max - min) / median.
Shapes: the PEMS07 pass (2520 origins, 64 paths, 12 steps, 228 nodes; --origins: fewer), the same pass on 8 group aggregates,
and a live query at count = 1 on either.
  hip    ops.scenario_envelope with a target (one launch; the allocation of its outputs included)
  torch  the same numbers as a torch composition in fp64: mean, var, abs, amax over the steps, kthvalue over the paths, the
         band and the target's depth (origin chunk by origin chunk, --chunk, to bound the fp64 copy)
The achieved bandwidth counts `paths` once (the kernel reads it once where the tile fits in LDS); the kernel's own time is
taken from torch.profiler in a run of its own.  torch sums in another order: the results must agree to rounding.
One JSON line, then a text report written to --out.
Usage: python tools/envelope_time.py [--origins 2520] [--chunk 252] [--reps 3] [--rounds 5] [--out profiles/envelope_time.txt]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reduce_time import alternate, kernel_times_us  # noqa: E402

N, H, S, R = 228, 12, 64, 8
COVERAGE = 0.9
SEED = 7


def torch_envelope(x, y, k, chunk):
    count, s, h, c = x.shape
    f64 = dict(device=x.device, dtype=torch.float64)
    moments, chosen, truth = torch.empty(count, 2, h, c, **f64), torch.empty(count, c, **f64), torch.empty(count, c, **f64)
    bands = torch.empty(count, 2, h, c, device=x.device)
    for c0 in range(0, count, chunk):
        X = x[c0:c0 + chunk].double()
        m = X.mean(dim=1)
        sd = X.var(dim=1, unbiased=False).sqrt()
        depth = ((X - m[:, None]).abs() / sd[:, None]).amax(dim=2)                # [chunk, S, C]
        q = depth.kthvalue(k, dim=1).values
        moments[c0:c0 + chunk, 0], moments[c0:c0 + chunk, 1], chosen[c0:c0 + chunk] = m, sd, q
        bands[c0:c0 + chunk, 0], bands[c0:c0 + chunk, 1] = (m - q[:, None] * sd).float(), (m + q[:, None] * sd).float()
        truth[c0:c0 + chunk] = ((y[c0:c0 + chunk].double() - m).abs() / sd).amax(dim=1)
    return dict(moments=moments, chosen=chosen, truth=truth, bands=bands)


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--origins", type=int, default=2520)
    ap.add_argument("--chunk", type=int, default=252)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "envelope_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("envelope_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import _lib, ops
    from stemgnn_amd.math_utils import group_weights
    lib = _lib.load()
    g = torch.Generator().manual_seed(SEED)
    count = args.origins
    walks = torch.randn(count, S + 1, H, N, generator=g).cumsum(dim=2).to(dev)    # random walks over the steps
    x, y = walks[:, :S].contiguous(), walks[:, S].contiguous()
    del walks
    w = group_weights([list(map(int, c)) for c in torch.arange(N).chunk(R)], N).to(dev)
    ax, ay = ops.scenario_aggregate(x, w), ops.scenario_aggregate(y, w)
    k = int(lib.stemgnn_conformal_rank(S, COVERAGE))
    res = {"shape": dict(N=N, horizon=H, S=S, origins=count, groups=R, coverage=COVERAGE, rank=k, chunk=args.chunk),
           "reps": args.reps, "rounds": args.rounds, "call_ms": {}, "agreement": {}}
    shapes = {"pass_nodes": (x, y, False), "pass_groups": (ax, ay, False), "live_nodes": (x[:1].contiguous(), y[:1].contiguous(), True),
              "live_groups": (ax[:1].contiguous(), ay[:1].contiguous(), True)}
    for name, (v, t, live) in shapes.items():
        hip = ops.scenario_envelope(v, COVERAGE, target=t)
        ref = torch_envelope(v, t, k, args.chunk)
        diff = {key: float(((hip[key].double() - ref[key].double()).abs() / ref[key].double().abs().clamp_min(1e-30)).max())
                for key in ("moments", "chosen", "truth")}
        diff["bands"] = float((hip["bands"] - ref["bands"]).abs().max() / ref["bands"].abs().max())
        res["agreement"][name] = diff
        if max(diff["moments"], diff["chosen"], diff["truth"]) > 1e-9 or diff["bands"] > 1e-6:
            raise SystemExit(f"{name}: the sides disagree: {diff}")
        reps = 20 * args.reps if live else args.reps
        r = alternate({"hip": lambda: ops.scenario_envelope(v, COVERAGE, target=t),
                       "torch": lambda: torch_envelope(v, t, k, args.chunk)}, reps, args.rounds, 1)
        try:
            kern = kernel_times_us(lambda: ops.scenario_envelope(v, COVERAGE, target=t), reps, ("env_kernel",))
        except Exception as e:                                                   # the profiler is an extra: the report says so
            kern = {"error": repr(e)[:200]}
        r["hip_kernels_us"] = kern
        r["paths_bytes"] = v.numel() * 4
        res["call_ms"][name] = r
        del hip, ref
    print(json.dumps(res))
    lines = [f"simultaneous bands, S {S}, horizon {H}, coverage {COVERAGE} (rank {k}); pass: {count} origins on N {N} nodes and on "
             f"{R} group means; live: count 1.  hip: ops.scenario_envelope with a target; torch: fp64 mean, var, abs, amax, "
             f"kthvalue, {args.chunk} origins per chunk",
             f"[call_ms] median of {args.rounds} alternating windows of {args.reps} calls (live shapes: {20 * args.reps}), ms per "
             "call, [(max - min) / median]; GB/s: the bytes of `paths`, counted once, over the time"]
    for name, r in res["call_ms"].items():
        gb = r["paths_bytes"] / 1e9
        kern = r["hip_kernels_us"]
        line = (f"  {name:<12} hip {r['hip']['median']:9.4f} [{r['hip']['spread']:.2f}]   torch {r['torch']['median']:9.4f} "
                f"[{r['torch']['spread']:.2f}]   hip / torch {r['hip']['median'] / r['torch']['median']:.4f}   paths {gb:.4f} GB   "
                f"call {gb / (r['hip']['median'] * 1e-3):8.1f} GB/s")
        if kern and "error" not in kern:
            us = kern["env_kernel"]
            line += f"   env_kernel {us:.2f} us, {gb / (us * 1e-6):8.1f} GB/s (torch.profiler, a run of its own)"
        else:
            line += f"   kernel not measured ({kern.get('error', 'the profiler listed none')})"
        lines.append(line)
    lines.append("[agreement] hip against torch: max relative difference of moments, chosen, truth; of the bands relative to the "
                 "largest band value")
    for name, a in res["agreement"].items():
        lines.append(f"  {name:<12} {a['moments']:.2e}   {a['chosen']:.2e}   {a['truth']:.2e}   {a['bands']:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
