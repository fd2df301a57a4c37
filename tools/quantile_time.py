"""Cost of the quantile head inside the captured step at the PEMS07 shape with Q = 3 levels.  One JSON line:
  engine.TrainStep (FusedRMSprop, hipGraph replay), two steppers built side by side:
    default   the plain model's step with every loss argument at its default (stemgnn_fc_tail_train_rows / _finish)
    pinball   Model(..., quantiles=(0.1, 0.5, 0.9)), loss="pinball": the same launches, the `_quantile` entries of the same tail
              kernels over Q * H = 9 output rows
  us per step: events around `reps` back-to-back replays ending in a synchronise, `rounds` such windows per variant, the
  variants ALTERNATING window by window (the order flips every round), median per variant after warm-up replays.
  rows launch alone: a hipGraph of `chain` back-to-back launches of stemgnn_fc_tail_train_rows (H = 3) and of
  stemgnn_fc_tail_train_rows_quantile (H = 3, Q = 3) on the same fsum / target, replayed and timed the same alternating way;
  us per launch = window / (reps * chain).
  --variant NAME: only replays of that variant's step, for a run under `rocprofv3 --kernel-trace --stats`.
Usage: python tools/quantile_time.py [--reps 200] [--rounds 9] [--variant pinball] [--out profiles/quantile_tail_time.txt]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, W, MULTI, H, B, T = 228, 12, 5, 3, 32, 3000
TAUS = (0.1, 0.5, 0.9)
VARIANTS = ("default", "pinball")
CHAIN = 20


def make_step(dev, variant):
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    torch.manual_seed(0)
    head = dict(quantiles=TAUS) if variant == "pinball" else {}
    model = Model(N, 2, W, MULTI, horizon=H, **head).to(dev).train()      # dropout 0.5, as the benchmark's step
    model.set_dropout_seed(99)
    opt = FusedRMSprop(model.parameters(), lr=1e-4, eps=1e-8)
    g = torch.Generator().manual_seed(7)
    series = torch.randn(T, N, generator=g).to(dev)
    kw = dict(loss="pinball") if variant == "pinball" else {}
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


def make_rows(dev, variant):
    """A captured chain of CHAIN rows launches on fixed buffers; returns the replay callable."""
    from stemgnn_amd import _lib
    from stemgnn_amd.engine import capture
    lib = _lib.load()
    Q = len(TAUS) if variant == "pinball" else 1
    g = torch.Generator().manual_seed(11)
    fsum = torch.randn(B, N, W, generator=g).to(dev)
    y = torch.randn(B, H, N, generator=g).to(dev)
    prm = [t.to(dev) for t in (torch.randn(W, W, generator=g) * 0.3, torch.randn(W, generator=g) * 0.1,
                               torch.randn(Q * H, W, generator=g) * 0.3, torch.randn(Q * H, generator=g) * 0.1)]
    scratch = torch.empty(lib.stemgnn_fc_tail_train_scratch_floats(B, N, W, Q * H), device=dev)
    dfsum = torch.empty_like(fsum)
    head = [fsum.data_ptr(), y.data_ptr()] + [p.data_ptr() for p in prm] + [B, N, W, H]
    taus = _lib.host_floats(TAUS)

    def chain():
        st = torch.cuda.current_stream().cuda_stream
        for _ in range(CHAIN):
            if variant == "pinball":
                _lib.check(lib.stemgnn_fc_tail_train_rows_quantile(*head, Q, taus, None, scratch.data_ptr(), None,
                                                                   dfsum.data_ptr(), st), "rows_quantile")
            else:
                _lib.check(lib.stemgnn_fc_tail_train_rows(*head, scratch.data_ptr(), None, dfsum.data_ptr(), st), "rows")
    rep = capture(chain, warmups=2)
    if rep is None:
        raise RuntimeError("graph capture of the rows chain failed")
    keep = (fsum, y, prm, scratch, dfsum, taus)
    return (lambda: rep()), keep


def window_us(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def alternate(runs, names, reps, rounds, warm):
    for v in names:
        window_us(runs[v], warm)
    us = {v: [] for v in names}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            us[v].append(window_us(runs[v], reps))
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--variant", choices=VARIANTS, default=None)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    names = VARIANTS if args.variant is None else (args.variant,)
    steps = {v: make_step(dev, v) for v in names}
    us = alternate({v: steps[v][1] for v in names}, names, args.reps, args.rounds, 50)
    out = {"shape": dict(N=N, W=W, multi=MULTI, H=H, B=B, Q=len(TAUS)), "reps": args.reps, "rounds": args.rounds,
           "modes": {v: steps[v][0].mode for v in names},
           "us_per_step_median": {v: round(statistics.median(us[v]), 2) for v in names},
           "us_per_step_windows": {v: [round(x, 2) for x in us[v]] for v in names},
           "loss": {v: float(steps[v][0].loss) for v in names}}
    if len(names) == 2:
        out["extra_us"] = round(out["us_per_step_median"]["pinball"] - out["us_per_step_median"]["default"], 2)
        rows = {v: make_rows(dev, v) for v in names}
        rus = alternate({v: rows[v][0] for v in names}, names, max(args.reps // 4, 10), args.rounds, 10)
        out["rows_launch_chain"] = CHAIN
        out["rows_launch_us_median"] = {v: round(statistics.median(rus[v]) / CHAIN, 2) for v in names}
        out["rows_launch_us_windows"] = {v: [round(x / CHAIN, 2) for x in rus[v]] for v in names}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
