"""Cost of the input gradient (x.grad) at the PEMS07 shape and the configs[3] / configs[4] per-GPU shards:
  (a) a training step (Model.loss + backward, overlap schedule as the step driver runs it) with and without x.requires_grad;
  (b) a frozen-weights attribution pass (eval forward + backward to x) against the same pass with trainable weights;
  (c) stemgnn_gru_input_grad alone, against its roofline (fp32 MFMA peak / HBM bandwidth).
GPU time per call from events around `reps` back-to-back calls (median of 5 such runs).  Prints one JSON line per shape.
Usage: python tools/input_grad_time.py [--reps 20] [--shapes pems07,c3,c4]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {"pems07": (228, 12, 5, 3, 32), "c3": (1024, 12, 5, 3, 8), "c4": (2048, 48, 5, 12, 16)}
PEAK_FLOPS, PEAK_BW = 157.3e12, 6.3e12


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        runs.append(a.elapsed_time(b) * 1e3 / reps)
    return round(statistics.median(runs), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="pems07,c3,c4")
    ap.add_argument("--parts", default="a,b,c", help="a, b, c, or b_train / b_frozen alone (kernel traces)")
    a = ap.parse_args()
    from oracle import stemgnn_oracle as O
    from stemgnn_amd import Model, _lib, ops

    dev = torch.device("cuda:0")
    lib = _lib.load()
    for name in a.shapes.split(","):
        N, W, multi, H, B = SHAPES[name]
        res = {"shape": name, "N": N, "W": W, "multi": multi, "H": H, "B": B, "dtype": os.environ.get("STEMGNN_DTYPE", "f32")}
        sd = O.det_state_dict(N, W, multi, H, seed=1)
        model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0)
        model.load_state_dict(sd)
        model.to(dev)
        x, y = torch.randn(B, W, N, device=dev), torch.randn(B, H, N, device=dev)

        parts = a.parts.split(",")
        # (a) training step
        model.train()
        model.hot_state.set(direct=True, overlap=True)
        for p in model.parameters():
            p.grad = torch.zeros_like(p)

        def train_step(need_x):
            xd = x.detach().requires_grad_(need_x)
            model.loss(xd, y, unit_grad=True).backward()
            ops.join_side_streams()
        if "a" in parts:
            res["train_step_us"] = timed(lambda: train_step(False), a.reps)
            res["train_step_xgrad_us"] = timed(lambda: train_step(True), a.reps)

        # (b) attribution pass: eval forward + backward to x (plain schedule)
        model.hot_state.set(direct=False)
        model.eval()
        g = torch.ones(B, H, N, device=dev)

        def attribution():
            model.zero_grad(set_to_none=True)
            xd = x.detach().requires_grad_(True)
            model(xd)[0].backward(g)
        if "b" in parts or "b_train" in parts:
            res["attr_trainable_us"] = timed(attribution, a.reps)
        if "b" in parts or "b_frozen" in parts:
            model.requires_grad_(False)
            res["attr_frozen_us"] = timed(attribution, a.reps)
            model.requires_grad_(True)
        if "c" not in parts:
            print(json.dumps(res), flush=True)
            continue

        # (c) the product alone: dgi [S*B, 3 Hd] (a random stand-in at offset 0 of the scratch) x W_ih [3 Hd, W] -> dx [B, W, S]
        S, Hd = N, N
        scratch = torch.randn(S * B * 3 * Hd, device=dev)
        w_ih = model.GRU.weight_ih_l0.detach().contiguous()
        dx = torch.empty(B, W, S, device=dev)

        def product():
            _lib.check(lib.stemgnn_gru_input_grad(scratch.data_ptr(), w_ih.data_ptr(), B, S, Hd, W, dx.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream), "gru_input_grad")
        res["product_us"] = timed(product, a.reps * 5)
        flops = 2.0 * S * B * 3 * Hd * W
        nbytes = 4.0 * (S * B * 3 * Hd + 3 * Hd * W + B * W * S)
        res["product_roofline_us"] = round(max(flops / PEAK_FLOPS, nbytes / PEAK_BW) * 1e6, 2)
        res["product_GBps"] = round(nbytes / (res["product_us"] * 1e-6) / 1e9, 1)
        del scratch
        print(json.dumps(res), flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
