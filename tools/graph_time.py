"""Frozen-graph timing at the PEMS07 shape (N=228, W=12, H=3, multi=5, B=32): Model.predict with and without a frozen graph
(``adjacency=model.latent_graph(x)``), and one captured training step (engine.TrainStep, FusedRMSprop) with and without.
Each figure is the median of --reps samples after a warm-up; a sample is HIP-event time over --inner back-to-back calls
divided by --inner (the calls are 0.2 - 1.5 ms long: one event pair around a single one would measure the launch gaps).
Prints one JSON line and writes the table to profiles/graph_adjacency_time.txt.
Usage: python tools/graph_time.py [--reps 30] [--inner 10]   (STEMGNN_DTYPE selects fp32 / bf16x2 as everywhere; the training
step from an adjacency runs its GLU layers in exact fp32 either way)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_adjacency_time.txt"))
    a = ap.parse_args()
    from oracle import stemgnn_oracle as O
    from stemgnn_amd import Model
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    N, W, multi, H, B = 228, 12, 5, 3, 32
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    x, y = torch.randn(B, W, N, device=dev), torch.randn(B, H, N, device=dev)

    def median_us(fn):
        for _ in range(3 * a.inner):
            fn()
        torch.cuda.synchronize()
        samples = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                fn()
            e1.record()
            e1.synchronize()
            samples.append(e0.elapsed_time(e1) / a.inner * 1e3)
        return dict(median_us=statistics.median(samples), min_us=min(samples), max_us=max(samples))

    def fresh():
        model = Model(N, 2, W, multi, horizon=H)
        model.load_state_dict(O.det_state_dict(N, W, multi, H, seed=1))
        return model.to(dev)

    res = {"shape": dict(N=N, W=W, H=H, multi=multi, B=B), "dtype": os.environ.get("STEMGNN_DTYPE", "f32"),
           "reps": a.reps, "inner": a.inner}
    model = fresh().eval()
    G = model.latent_graph(x)
    G.basis()                                   # built once; every later call takes it from the cache
    res["predict"] = median_us(lambda: model.predict(x))
    res["predict_adjacency"] = median_us(lambda: model.predict(x, adjacency=G))
    # interleaved once more the other way round, so a drift of the clocks cannot decide the comparison
    res["predict_adjacency_2"] = median_us(lambda: model.predict(x, adjacency=G))
    res["predict_2"] = median_us(lambda: model.predict(x))

    def train_step(adjacency):
        m = fresh().train()
        m.set_dropout_seed(1)
        opt = FusedRMSprop(m.parameters(), lr=1e-4, eps=1e-8)
        kw = {} if adjacency is None else dict(adjacency=adjacency)
        step = TrainStep(m, opt, B, W, H, N, **kw)
        step.run_batch(x, y)                    # eager first step, then the capture
        out = median_us(lambda: step.run_batch())
        out["mode"] = step.mode
        return out

    res["train_step"] = train_step(None)
    res["train_step_adjacency"] = train_step(G)
    p = min(res["predict"]["median_us"], res["predict_2"]["median_us"])
    pa = max(res["predict_adjacency"]["median_us"], res["predict_adjacency_2"]["median_us"])
    res["predict_ratio"] = pa / p               # the slower frozen-graph figure over the faster default one
    res["train_step_ratio"] = res["train_step_adjacency"]["median_us"] / res["train_step"]["median_us"]
    lines = [f"frozen-graph timing, PEMS07 shape N={N} W={W} H={H} multi={multi} B={B}, STEMGNN_DTYPE={res['dtype']}",
             f"median of {a.reps} samples, each {a.inner} back-to-back calls between two HIP events (us per call)", ""]
    for k in ("predict", "predict_adjacency", "predict_adjacency_2", "predict_2", "train_step", "train_step_adjacency"):
        v = res[k]
        lines.append(f"{k:24s} median {v['median_us']:9.1f}   min {v['min_us']:9.1f}   max {v['max_us']:9.1f}   {v.get('mode', '')}")
    lines += ["", f"predict(x, adjacency=G) / predict(x)            {res['predict_ratio']:.3f}   (slower frozen run over faster default run)",
              f"train step with adjacency / default train step  {res['train_step_ratio']:.3f}"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
