"""Cost of gradient-norm clipping inside the fused step at the PEMS07 shape.  One JSON line per part:
  step    engine.TrainStep (FusedRMSprop or FusedAdam, hipGraph replay), three steppers built side by side:
            default    the step with every control at its default (the old entry points)
            clip       max_grad_norm set: stemgnn_grad_sqsum + stemgnn_*_step_ext
            torch      the default step with torch.nn.utils.clip_grad_norm_(parameters, max_norm) captured in front of
                       step() -- what a user would write without the control
          us per step: events around `reps` back-to-back replays ending in a synchronise, `rounds` such windows per variant,
          the variants ALTERNATING window by window (the order rotates every round), median per variant after warm-up replays
  trace   only replays of ONE variant (--variant), nothing else on the device: the run to put under
          `rocprofv3 --kernel-trace --stats` for the kernel times of the sqsum launch and of the step kernels
Usage: python tools/optim_time.py --part step|trace [--optimizer RMSProp|Adam] [--reps 200] [--rounds 9] [--variant clip]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, W, MULTI, H, B, T = 228, 12, 5, 3, 32, 3000
MAX_NORM = 1.0
VARIANTS = ("default", "clip", "torch")


def make_step(dev, variant, optimizer):
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedAdam, FusedRMSprop

    base = FusedRMSprop if optimizer == "RMSProp" else FusedAdam

    class TorchClipped(base):          # clip_grad_norm_ over the ~70 bucket views, then the default fused step
        def step(self, closure=None):
            torch.nn.utils.clip_grad_norm_(self._params, MAX_NORM)
            return super().step(closure)

    torch.manual_seed(0)
    model = Model(N, 2, W, MULTI, horizon=H).to(dev).train()              # dropout 0.5, as the benchmark's step
    model.set_dropout_seed(99)
    cls = TorchClipped if variant == "torch" else base
    kw = dict(max_grad_norm=MAX_NORM) if variant == "clip" else {}
    opt = cls(model.parameters(), lr=1e-4, eps=1e-8, **kw)
    g = torch.Generator().manual_seed(7)
    series = torch.randn(T, N, generator=g).to(dev)
    step = TrainStep(model, opt, B, W, H, N, series=series, order_capacity=64 * B)
    order = (torch.randint(0, T - W - H, (64 * B,), generator=g) + W).to(dev)

    def run():
        if step._q_left < B:
            step.load_order(order)
        step.run_next()
    for _ in range(4):                  # eager first step, capture, first replays
        run()
    torch.cuda.synchronize()
    return step, opt, run


def window_us(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["step", "trace"])
    ap.add_argument("--optimizer", default="RMSProp", choices=["RMSProp", "Adam"])
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--variant", default="clip", choices=VARIANTS)
    ap.add_argument("--steps", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    res = {"part": a.part, "optimizer": a.optimizer, "shape": [N, W, MULTI, H, B], "max_norm": MAX_NORM}
    if a.part == "trace":
        step, opt, run = make_step(dev, a.variant, a.optimizer)
        for _ in range(a.steps):
            run()
        torch.cuda.synchronize()
        res.update(variant=a.variant, mode=step.mode, steps=a.steps + 4, numel=opt.numel)
        print(json.dumps(res))
        return
    built = {v: make_step(dev, v, a.optimizer) for v in VARIANTS}
    for v in VARIANTS:                  # warm-up: every variant's replay path, before any timed window
        window_us(built[v][2], 50)
    runs = {v: [] for v in VARIANTS}
    for r in range(a.rounds):
        for k in range(len(VARIANTS)):
            v = VARIANTS[(k + r) % len(VARIANTS)]
            runs[v].append(window_us(built[v][2], a.reps))
    for v in VARIANTS:
        step, opt, _ = built[v]
        res[v + "_us"] = round(statistics.median(runs[v]), 2)
        res[v + "_min_max_us"] = [round(min(runs[v]), 2), round(max(runs[v]), 2)]
        res[v + "_mode"] = step.mode
    res["numel"] = built["clip"][1].numel
    res["clip_report"] = built["clip"][1].grad_report()
    res["clip_minus_default_us"] = round(res["clip_us"] - res["default_us"], 2)
    res["torch_minus_default_us"] = round(res["torch_us"] - res["default_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
