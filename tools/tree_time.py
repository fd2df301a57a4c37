"""Cost of the scenario-tree kernels, by the protocol of tools/reduce_time.py: same process, results compared
first, alternating windows of device events, medians and the spread (max - min) / median.
Shapes: the PEMS07 pass (2520 origins, 64 paths, 12 steps, 228 nodes; stages (3, 6, 12), nodes (2, 4, 8); --origins: fewer), the
same pass on 8 group aggregates, and a live query at count = 1 on either.
  distances  stemgnn_scenario_stage_distances alone, against what existed before it:
               prefix  T calls of ops.scenario_distances on .contiguous() prefix slices of the paths
               torch   torch.cdist in fp64 on the same slices (origin chunk by origin chunk, --chunk, to bound the fp64 copy)
  tree       stemgnn_scenario_tree alone on those distances, against the staged greedy loop written in torch: vectorised over
             origins and candidates, no host decision per pick, the parent constraint as a mask
  both       ops.scenario_tree (distances in scratch, then the tree) against cdist + loop
The torch side sums in another order, so it need not pick the same paths where two candidates are within rounding: the share of
origins with the same nodes is reported; the distances, and the costs of the origins with the same nodes, must agree to rounding.
One JSON line, then a text report written to --out.
Usage: python tools/tree_time.py [--origins 2520] [--chunk 252] [--reps 3] [--rounds 5] [--out profiles/tree_time.txt]"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from reduce_time import alternate, kernel_times_us  # noqa: E402

N, H, S, R = 228, 12, 64, 8
STAGES, NODES = (3, 6, 12), (2, 4, 8)
SEED = 7


def prefix_distances(ops, x):
    return torch.stack([ops.scenario_distances(x[:, :, :b].contiguous()) for b in STAGES], dim=1)


def torch_distances(x, chunk):
    count, s = x.shape[:2]
    D = torch.empty(count, len(STAGES), s, s, device=x.device, dtype=torch.float64)
    for c0 in range(0, count, chunk):
        for t, b in enumerate(STAGES):
            v = x[c0:c0 + chunk, :, :b].double().flatten(2)
            D[c0:c0 + chunk, t] = torch.cdist(v, v)
    return D


def torch_tree(D, nodes):
    count, T, s, _ = D.shape
    dev = D.device
    par = torch.zeros(count, s, device=dev, dtype=torch.int64)
    path = torch.full((count, T, nodes[-1]), -1, device=dev, dtype=torch.int64)
    cost = torch.empty(count, T, device=dev, dtype=torch.float64)
    n_prev = 1
    for t in range(T):
        Dt = D[:, t]
        E = Dt.masked_fill(par[:, :, None] != par[:, None, :], float("inf"))     # only onto a path of the own parent
        m = torch.full((count, s), float("inf"), device=dev, dtype=torch.float64)
        near = torch.full((count, s), -1, device=dev, dtype=torch.int64)
        taken = torch.zeros(count, s, device=dev, dtype=torch.bool)
        for i in range(nodes[t]):
            if i < n_prev:
                mine = par == i
                z = Dt.masked_fill(~mine[:, :, None], 0.0).sum(dim=1).masked_fill(taken | ~mine, float("inf"))
            else:
                z = torch.minimum(m[:, :, None], E).sum(dim=1).masked_fill(taken, float("inf"))
            u = z.argmin(dim=1)
            path[:, t, i] = u
            taken.scatter_(1, u[:, None], True)
            d = E.gather(2, u[:, None, None].expand(-1, s, 1)).squeeze(2)
            lower = d < m
            m = torch.where(lower, d, m)
            near = torch.where(lower, torch.full_like(near, i), near)
        cost[:, t] = m.sum(dim=1) / s
        par, n_prev = near, nodes[t]
    return path, cost


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--origins", type=int, default=2520)
    ap.add_argument("--chunk", type=int, default=252)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "tree_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("tree_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import _lib, ops
    from stemgnn_amd.math_utils import group_weights
    lib = _lib.load()
    stream = lambda: torch.cuda.current_stream().cuda_stream                     # noqa: E731
    g = torch.Generator().manual_seed(SEED)
    count, T, nT = args.origins, len(STAGES), NODES[-1]
    x = torch.randn(count, S, H, N, generator=g).cumsum(dim=2).to(dev)            # random walks over the steps
    w = group_weights([list(map(int, c)) for c in torch.arange(N).chunk(R)], N).to(dev)
    agg = ops.scenario_aggregate(x, w)
    bounds, nodes = (ctypes.c_int * T)(*STAGES), (ctypes.c_int * T)(*NODES)
    res = {"shape": dict(N=N, horizon=H, S=S, origins=count, groups=R, stages=STAGES, nodes=NODES, chunk=args.chunk),
           "reps": args.reps, "rounds": args.rounds, "call_ms": {}, "agreement": {}}

    def hip_distances(v, out):
        _lib.check(lib.stemgnn_scenario_stage_distances(v.data_ptr(), None, v.shape[0], S, H, v.shape[3], T, bounds, 0,
                                                        out.data_ptr(), stream()), "scenario_stage_distances")

    def hip_tree(D, outs):
        _lib.check(lib.stemgnn_scenario_tree(D.data_ptr(), None, D.shape[0], S, T, nodes, S, *(o.data_ptr() for o in outs),
                                             stream()), "scenario_tree")

    shapes = {"pass_nodes": (x, False), "pass_groups": (agg, False), "live_nodes": (x[:1].contiguous(), True),
              "live_groups": (agg[:1].contiguous(), True)}
    for name, (v, live) in shapes.items():
        c = v.shape[0]
        D = torch.empty(c, T, S, S, device=dev, dtype=torch.float64)
        outs = tuple(torch.empty(c, T, nT, device=dev, dtype=torch.int32) for _ in range(3)) + \
            (torch.empty(c, T, S, device=dev, dtype=torch.int32), torch.empty(c, T, device=dev, dtype=torch.float64))
        hip_distances(v, D)
        hip_tree(D, outs)
        p_D = prefix_distances(ops, v)
        t_D = torch_distances(v, args.chunk)
        t_path, t_cost = torch_tree(t_D, NODES)
        off = ~torch.eye(S, device=dev, dtype=torch.bool)                        # (cdist's diagonal is not exactly 0)
        p_diff = float(((D - p_D).abs() / D.clamp_min(1e-30))[:, :, off].max())
        d_diff = float(((D - t_D).abs() / D.clamp_min(1e-30))[:, :, off].max())
        alike = (outs[0].long() == t_path).flatten(1).all(dim=1)
        same = float(alike.double().mean())
        c_diff = float(((outs[4] - t_cost).abs() / t_cost)[alike].max()) if bool(alike.any()) else 0.0
        res["agreement"][name] = dict(prefix_max_relative_difference=p_diff, distance_max_relative_difference=d_diff,
                                      origins_with_the_same_nodes=same, cost_max_relative_difference=c_diff)
        if p_diff > 1e-12 or d_diff > 1e-9 or c_diff > 1e-6:
            raise SystemExit(f"{name}: the sides disagree: prefix {p_diff}, distances {d_diff}, costs at equal nodes {c_diff}")
        reps = 20 * args.reps if live else args.reps
        r = {}
        for part, runs in (("distances", {"hip": lambda: hip_distances(v, D), "prefix": lambda: prefix_distances(ops, v),
                                          "torch": lambda: torch_distances(v, args.chunk)}),
                           ("tree", {"hip": lambda: hip_tree(D, outs), "torch": lambda: torch_tree(t_D, NODES)}),
                           ("both", {"hip": lambda: ops.scenario_tree(v, STAGES, NODES),
                                     "torch": lambda: torch_tree(torch_distances(v, args.chunk), NODES)})):
            r[part] = alternate(runs, reps, args.rounds, 1)
        res["call_ms"][name] = r
        try:
            kern = kernel_times_us(lambda: (hip_distances(v, D), hip_tree(D, outs)), args.reps,
                                   ("tr_distance_kernel", "tr_tree_kernel"))
        except Exception as e:                                                   # the profiler is an extra: the report says so
            kern = {"error": repr(e)[:200]}
        r["hip_kernels_us"] = kern
        del D, t_D, p_D
    print(json.dumps(res))
    lines = [f"scenario trees, S {S}, horizon {H}, stages {STAGES}, nodes {NODES}; pass: {count} origins on N {N} nodes and on {R} "
             f"group means; live: count 1 (prefix: {T} calls of scenario_distances on contiguous prefix copies; torch: cdist in "
             f"fp64 on the same slices, {args.chunk} origins per chunk, and a masked greedy loop)",
             f"[call_ms] median of {args.rounds} alternating windows of {args.reps} calls (live shapes: {20 * args.reps}), ms per "
             "call, [(max - min) / median]"]
    for name, r in res["call_ms"].items():
        lines.append(f"  {name}")
        for part in ("distances", "tree", "both"):
            t = r[part]
            lines.append(f"    {part:<10} " + "   ".join(f"{k} {t[k]['median']:9.4f} [{t[k]['spread']:.2f}]" for k in t) + "   "
                         + "   ".join(f"hip / {k} {t['hip']['median'] / t[k]['median']:.4f}" for k in t if k != "hip"))
        kern = r["hip_kernels_us"]
        if not kern or "error" in kern:
            lines.append(f"    kernels    not measured: the profiler reported no kernel ({kern.get('error', 'none listed')})")
        else:
            lines.append("    kernels    " + "   ".join(f"{k} {v:.2f} us" for k, v in kern.items())
                         + "   (torch.profiler, a run of its own)")
    lines.append("[agreement] hip against the others: max relative difference of the distances against the prefix calls and "
                 "against cdist, share of origins with the same nodes, max relative difference of the costs where the nodes are the same")
    for name, a in res["agreement"].items():
        lines.append(f"  {name:<12} {a['prefix_max_relative_difference']:.2e}   {a['distance_max_relative_difference']:.2e}   "
                     f"{a['origins_with_the_same_nodes']:.4f}   {a['cost_max_relative_difference']:.2e}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
