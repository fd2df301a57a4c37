"""Cost of conformal calibration at a PEMS07 validation pass.  One JSON line.
  shape: count = 2520 windows (the 20 % split of a 12672-row series, window 12, horizon 3), Q = 3, H = 3, N = 228; all four
  groupings (per_step, per_node), masked (about 10 % NaN targets) and not.
  fit     ops.conformal_fit on resident tensors (scratch and outputs allocated by the call, as a user gets it)
  torch   what a user would write today, same GPU, same process: the scores as tensors, the group axis moved last, torch.sort
          along it (NaN scores as +inf; masked: the masked-out scores as +inf too, so that they sort last), the rank computed
          ON THE DEVICE from the per-group valid count in fp64, and a gather of the k-th value -- no host round trip
  apply   ops.conformal_apply, out of place;  torch_apply: clone + two broadcast row updates
  us per call: events around `reps` back-to-back calls ending in a synchronise, `rounds` such windows per variant, fit and torch
  ALTERNATING window by window (the order flips every round), median per variant after warm-up calls.  The two fits are
  checked for equal offsets and counts before anything is timed.
Usage: python tools/conformal_time.py [--reps 50] [--rounds 9] [--out profiles/conformal_time.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COUNT, Q, H, N = 2520, 3, 3, 228
TAUS = (0.1, 0.5, 0.9)
PAIRS, COVERAGE = ((0, 2),), [0.9 - 0.1]
GROUPINGS = ((True, False), (False, False), (True, True), (False, True))


def torch_fit(y, f, per_step, per_node, masked):
    """the torch formulation of ops.conformal_fit for the pairs above: (offsets, counts) [P, Hg, Ng]"""
    inf = torch.tensor(float("inf"), device=y.device)
    offsets, counts = [], []
    for (lo, hi), c in zip(PAIRS, COVERAGE):
        s = torch.maximum(f[:, lo] - y, y - f[:, hi])
        s = torch.where(torch.isnan(s), inf, s)
        valid = ~torch.isnan(y) if masked else torch.ones_like(y, dtype=torch.bool)
        if masked:
            s = torch.where(valid, s, inf)
        # [count, H, N] -> [Hg, Ng, members]
        if per_step and per_node:
            g, v = s.permute(1, 2, 0), valid.permute(1, 2, 0)
        elif per_step:
            g, v = s.permute(1, 0, 2).reshape(H, 1, -1), valid.permute(1, 0, 2).reshape(H, 1, -1)
        elif per_node:
            g, v = s.permute(2, 0, 1).reshape(1, N, -1), valid.permute(2, 0, 1).reshape(1, N, -1)
        else:
            g, v = s.reshape(1, 1, -1), valid.reshape(1, 1, -1)
        m = v.sum(-1)
        k = torch.ceil(((m + 1).double() * c) * (1 - 1e-12)).long()
        ordered = torch.sort(g, dim=-1).values
        kth = ordered.gather(-1, (k.clamp(max=g.shape[-1]) - 1).unsqueeze(-1)).squeeze(-1)
        offsets.append(torch.where(k > m, inf, kth))
        counts.append(m)
    return torch.stack(offsets), torch.stack(counts)


def torch_apply(f, offsets):
    out = f.clone()
    for p, (lo, hi) in enumerate(PAIRS):
        out[:, lo] -= offsets[p]
        out[:, hi] += offsets[p]
    return out


def window_us(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(runs, reps, rounds, warm):
    names = list(runs)
    for v in names:
        window_us(runs[v], warm)
    us = {v: [] for v in names}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            us[v].append(window_us(runs[v], reps))
    return {v: round(statistics.median(us[v]), 2) for v in names}, {v: [round(x, 2) for x in us[v]] for v in names}


def main():
    from stemgnn_amd import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(3)
    y = torch.randn(COUNT, H, N, generator=g)
    f = (0.5 * y + 0.5 * torch.randn(COUNT, H, N, generator=g)).unsqueeze(1) + torch.tensor([-0.6, 0.0, 0.6]).view(1, Q, 1, 1)
    y_nan = y.clone()
    y_nan[torch.rand(y.shape, generator=g) < 0.1] = float("nan")
    y, y_nan, f = y.to(dev), y_nan.to(dev), f.contiguous().to(dev)
    out = {"shape": dict(count=COUNT, Q=Q, H=H, N=N, P=len(PAIRS)), "reps": args.reps, "rounds": args.rounds, "fit_us": {},
           "fit_us_windows": {}, "apply_us": {}, "apply_us_windows": {}}
    for per_step, per_node in GROUPINGS:
        for masked in (False, True):
            name = f"step{int(per_step)}_node{int(per_node)}" + ("_masked" if masked else "")
            t = y_nan if masked else y
            got, want = ops.conformal_fit(t, f, PAIRS, COVERAGE, per_step, per_node, ignore_nan=masked), \
                torch_fit(t, f, per_step, per_node, masked)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), name
            med, windows = alternate({"fit": lambda: ops.conformal_fit(t, f, PAIRS, COVERAGE, per_step, per_node, ignore_nan=masked),
                                      "torch": lambda: torch_fit(t, f, per_step, per_node, masked)},
                                     args.reps, args.rounds, 10)
            out["fit_us"][name] = med
            out["fit_us_windows"][name] = windows
        offsets = got[0]
        med, windows = alternate({"apply": lambda: ops.conformal_apply(f, offsets, PAIRS, per_step, per_node),
                                  "torch_apply": lambda: torch_apply(f, offsets)}, args.reps, args.rounds, 10)
        out["apply_us"][f"step{int(per_step)}_node{int(per_node)}"] = med
        out["apply_us_windows"][f"step{int(per_step)}_node{int(per_node)}"] = windows
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
