"""Cost of a robust, missing-value-aware loss inside the captured step at the PEMS07 shape.  One JSON line:
  engine.TrainStep (FusedRMSprop, hipGraph replay), two steppers built side by side:
    default   the step with every loss argument at its default (stemgnn_fc_tail_train_rows / _finish)
    masked    loss="mae", ignore_nan=True, targets from a target_series with 10 % NaN: one more launch on the chain
              (stemgnn_target_valid_count), the `_loss` entries of the same tail kernels, the `_pair` gather
  us per step: events around `reps` back-to-back replays ending in a synchronise, `rounds` such windows per variant, the
  variants ALTERNATING window by window (the order flips every round), median per variant after warm-up replays.
  --variant NAME: only replays of that variant, for a run under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/loss_time.py [--reps 200] [--rounds 9] [--variant masked]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, W, MULTI, H, B, T = 228, 12, 5, 3, 32, 3000
VARIANTS = ("default", "masked")


def make_step(dev, variant):
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    torch.manual_seed(0)
    model = Model(N, 2, W, MULTI, horizon=H).to(dev).train()              # dropout 0.5, as the benchmark's step
    model.set_dropout_seed(99)
    opt = FusedRMSprop(model.parameters(), lr=1e-4, eps=1e-8)
    g = torch.Generator().manual_seed(7)
    series = torch.randn(T, N, generator=g).to(dev)
    kw = {}
    if variant == "masked":
        target = series.clone()
        target[torch.rand(T, N, generator=g).to(dev) < 0.1] = float("nan")
        kw = dict(loss="mae", ignore_nan=True, target_series=target)
    step = TrainStep(model, opt, B, W, H, N, series=series, order_capacity=64 * B, **kw)
    order = (torch.randint(0, T - W - H, (64 * B,), generator=g) + W).to(dev)

    def run():
        if step._q_left < B:
            step.load_order(order)
        step.run_next()
    for _ in range(4):                  # eager first step, capture, first replays
        run()
    torch.cuda.synchronize()
    return step, run


def window_us(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--variant", choices=VARIANTS, default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    names = VARIANTS if args.variant is None else (args.variant,)
    steps = {v: make_step(dev, v) for v in names}
    for v in names:                     # warm-up replays
        window_us(steps[v][1], 50)
    us = {v: [] for v in names}
    for r in range(args.rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            us[v].append(window_us(steps[v][1], args.reps))
    out = {"shape": dict(N=N, W=W, multi=MULTI, H=H, B=B), "reps": args.reps, "rounds": args.rounds,
           "modes": {v: steps[v][0].mode for v in names},
           "us_per_step_median": {v: round(statistics.median(us[v]), 2) for v in names},
           "us_per_step_windows": {v: [round(x, 2) for x in us[v]] for v in names},
           "loss": {v: float(steps[v][0].loss) for v in names}}
    if len(names) == 2:
        out["extra_us"] = round(out["us_per_step_median"]["masked"] - out["us_per_step_median"]["default"], 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
