"""Cost of scenario forecasts, by the protocol of tools/seasonal_time.py: same process, results checked equal
first, alternating windows, medians and the spread (max - min) / median.
Setting: the PEMS07 shape (N 228, W 12, multi 5), Q 3, model horizon 3, horizon 12 (4 rounds), S 64 paths, a loader batch of 32
origins, a frozen graph (adjacency=model.latent_graph(x)).
  kernels  ops.scenario_roll and ops.scenario_bands alone against their torch counterparts, the composition of the same
           definition a user would write: per round torch.sort over the levels, a uniform tensor, searchsorted, gather, the
           interpolation, cat; the bands torch.sort over the paths + index_select.  Round 0 (32 source rows fanned out to 2048
           paths) and a later round (2048 source rows) are timed apart.  Equality first: with the kernel's own uniforms (the
           numpy Philox of tests/helpers) handed to the composition, both give the same bits.
  pass     one batch through all four rounds: the new kernels around Model.predict, the torch composition around the same
           predict calls, trainer.rolling_forecast at the same horizon (the point-path roll: what the paths cost on top), and
           the predict calls alone (one at batch 32 + three at batch 2048).  Host clock around work that ends in a synchronise.
One JSON line, then a text report written to --out.
Usage: python tools/scenario_time.py [--sections kernels,pass] [--reps 20] [--rounds 7] [--out profiles/scenario_time.txt]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

N, W, MULTI, L, HORIZON, S, BO = 228, 12, 5, 3, 12, 64, 32
TAUS = (0.1, 0.5, 0.9)
Q = len(TAUS)
SEED = 7


def event_window_us(run, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        run()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def host_window_ms(run, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        run()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def alternate(runs, window, reps, rounds, warm):
    names = list(runs)
    for v in names:
        window(runs[v], warm)
    got = {v: [] for v in names}
    for r in range(rounds):
        for v in (names if r % 2 == 0 else names[::-1]):
            got[v].append(window(runs[v], reps))
    return {v: dict(median=round(statistics.median(got[v]), 3),
                    spread=round((max(got[v]) - min(got[v])) / statistics.median(got[v]), 3)) for v in names}


def torch_round(window, out, taus_t, fan, step, horizon, steps, bands, u=None):
    """One round of the definition in eager torch; window [Bsrc,W,N], out [Bsrc,Q,L,N] -> the next windows [P,W,N]."""
    P, n_l = window.shape[0] * fan, out.shape[2]
    v = torch.sort(out, dim=1, stable=True).values
    if fan > 1:
        v, window = v.repeat_interleave(fan, dim=0), window.repeat_interleave(fan, dim=0)
    if u is None:
        u = torch.rand(P, n_l, window.shape[2], device=window.device)
    i = (torch.searchsorted(taus_t, u, right=True) - 1).clamp_(0, taus_t.numel() - 2)
    t0, t1 = taus_t[i], taus_t[i + 1]
    wt = (u - t0) / (t1 - t0)
    lo, hi = v.gather(1, i[:, None]).squeeze(1), v.gather(1, (i + 1)[:, None]).squeeze(1)
    y = lo + (hi - lo) * wt
    take = min(n_l, horizon - step)
    steps.view(P, horizon, -1)[:, step:step + take] = y[:, :take]
    if bands is not None:
        bands[:, :, step:step + take] = out[:, :, :take]
    return torch.cat([window[:, n_l:], y], dim=1)


def torch_bands(steps, ranks_t, step_from, bands):
    bands[:, :, step_from:] = torch.sort(steps, dim=1).values.index_select(1, ranks_t)[:, :, step_from:]
    return bands


def kernels_section(ops, args, dev):
    from tests.helpers import scenario_ref as R
    g = torch.Generator().manual_seed(SEED)
    taus_t = torch.tensor(TAUS, device=dev)
    ranks_t = torch.tensor([ops.scenario_rank(t, S) - 1 for t in TAUS], device=dev)
    # equality first, at a small shape: the composition fed the kernel's own uniforms gives the kernel's bits
    bo, s, n = 2, 5, 12
    bit_equal = True
    for fan in (s, 1):
        src = bo if fan == s else bo * s
        x, out = torch.randn(src, W, n, generator=g).to(dev), torch.randn(src, Q, L, n, generator=g).to(dev)
        steps, bands = torch.zeros(bo, s, HORIZON, n, device=dev), torch.zeros(bo, Q, HORIZON, n, device=dev)
        nxt = ops.scenario_roll(x, out, TAUS, steps, 3, origin0=11, seed=SEED, bands=bands if fan == s else None)
        u = torch.from_numpy(R.uniform(R.words(11, bo, s, HORIZON, 3, L, n, SEED, 0, "independent")).reshape(bo * s, L, n))
        steps_t, bands_t = torch.zeros_like(steps), torch.zeros_like(bands)
        nxt_t = torch_round(x, out, taus_t, fan, 3, HORIZON, steps_t, bands_t if fan == s else None, u=u.to(dev))
        # (torch's own fp32 divide decides whether the composition's bits are the kernel's: reported, not required)
        assert torch.allclose(nxt, nxt_t, rtol=1e-6, atol=1e-7) and torch.allclose(steps, steps_t, rtol=1e-6, atol=1e-7)
        assert torch.equal(bands, bands_t) and torch.equal(nxt[:, :W - L], nxt_t[:, :W - L])
        bit_equal = bit_equal and torch.equal(nxt.view(torch.int32), nxt_t.view(torch.int32)) and torch.equal(steps, steps_t)
    paths = torch.randn(BO, S, HORIZON, N, generator=g).to(dev)
    b_hip = ops.scenario_bands(paths, TAUS, L, torch.zeros(BO, Q, HORIZON, N, device=dev))
    b_t = torch_bands(paths, ranks_t, L, torch.zeros(BO, Q, HORIZON, N, device=dev))
    assert torch.equal(b_hip, b_t)
    # timing at the setting's shape
    x0, out0 = torch.randn(BO, W, N, generator=g).to(dev), torch.randn(BO, Q, L, N, generator=g).to(dev)
    x1, out1 = torch.randn(BO * S, W, N, generator=g).to(dev), torch.randn(BO * S, Q, L, N, generator=g).to(dev)
    steps, bands = torch.zeros(BO, S, HORIZON, N, device=dev), torch.zeros(BO, Q, HORIZON, N, device=dev)
    res = {}
    res["roll_round0"] = alternate(
        {"hip": lambda: ops.scenario_roll(x0, out0, TAUS, steps, 0, seed=SEED, bands=bands),
         "torch": lambda: torch_round(x0, out0, taus_t, S, 0, HORIZON, steps, bands)}, event_window_us, args.reps, args.rounds, 5)
    res["roll_later"] = alternate(
        {"hip": lambda: ops.scenario_roll(x1, out1, TAUS, steps, 3, seed=SEED),
         "torch": lambda: torch_round(x1, out1, taus_t, 1, 3, HORIZON, steps, None)}, event_window_us, args.reps, args.rounds, 5)
    res["roll_last"] = alternate(
        {"hip": lambda: ops.scenario_roll(x1, out1, TAUS, steps, 9, seed=SEED, last=True),
         "torch": lambda: torch_round(x1, out1, taus_t, 1, 9, HORIZON, steps, None)}, event_window_us, args.reps, args.rounds, 5)
    res["bands"] = alternate(
        {"hip": lambda: ops.scenario_bands(steps, TAUS, L, bands),
         "torch": lambda: torch_bands(steps, ranks_t, L, bands)}, event_window_us, args.reps, args.rounds, 5)
    for r in res.values():
        r["hip_over_torch"] = round(r["hip"]["median"] / r["torch"]["median"], 3)
    res["roll_round0"]["composition_bit_equal"] = float(bit_equal)
    return res


def pass_section(ops, args, dev):
    from stemgnn_amd import Model, trainer
    from stemgnn_amd.engine import scenario_rounds
    torch.manual_seed(0)
    model = Model(N, 2, W, MULTI, horizon=L, quantiles=TAUS).to(dev).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x, y = torch.randn(BO, W, N, generator=g).to(dev), torch.randn(BO, HORIZON, N, generator=g).to(dev)
    graph = model.latent_graph(x)
    kw = dict(adjacency=graph)
    taus_t = torch.tensor(TAUS, device=dev)
    ranks_t = torch.tensor([ops.scenario_rank(t, S) - 1 for t in TAUS], device=dev)
    xs = torch.randn(BO * S, W, N, generator=g).to(dev)

    def hip_pass():
        with torch.no_grad():
            return scenario_rounds(model, x, HORIZON, S, 0, SEED, "independent", "linear", kw)

    def torch_pass():
        with torch.no_grad():
            steps, bands = torch.empty(BO, S, HORIZON, N, device=dev), torch.empty(BO, Q, HORIZON, N, device=dev)
            window, done = x, 0
            while done < HORIZON:
                out, _ = model.predict(window, **kw)
                window = torch_round(window, out, taus_t, S if done == 0 else 1, done, HORIZON, steps, bands if done == 0 else None)
                done += L
            return torch_bands(steps, ranks_t, L, bands), steps

    def predict_only():
        model.predict(x, **kw)
        for _ in range(HORIZON // L - 1):
            model.predict(xs, **kw)

    # the two passes agree where no random number is involved, and in distribution beyond (different generators)
    (b_hip, _), (b_t, _) = hip_pass(), torch_pass()
    assert torch.equal(b_hip[:, :, :L], b_t[:, :, :L])
    width = lambda b: float((b[:, -1, L:] - b[:, 0, L:]).mean())
    assert abs(width(b_hip) / width(b_t) - 1) < 0.1, (width(b_hip), width(b_t))
    res = {"pass": alternate({"scenarios_hip": hip_pass, "scenarios_torch": torch_pass,
                              "rolling_forecast": lambda: trainer.rolling_forecast(model, [(x, y)], HORIZON, **kw),
                              "predict_only": predict_only}, host_window_ms, args.pass_reps, args.rounds, 3)}
    p = res["pass"]
    p["hip_over_torch"] = round(p["scenarios_hip"]["median"] / p["scenarios_torch"]["median"], 3)
    p["hip_over_rolling_forecast"] = round(p["scenarios_hip"]["median"] / p["rolling_forecast"]["median"], 3)
    p["predict_share_of_hip"] = round(p["predict_only"]["median"] / p["scenarios_hip"]["median"], 3)
    p["band_width_hip_over_torch"] = round(width(b_hip) / width(b_t), 4)
    return res


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernels,pass")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "scenario_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    if not torch.cuda.is_available():
        raise SystemExit("scenario_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    from stemgnn_amd import ops
    res = {"shape": dict(N=N, W=W, Q=Q, L=L, horizon=HORIZON, S=S, Bo=BO), "reps": args.reps, "pass_reps": args.pass_reps,
           "rounds": args.rounds}
    sections = args.sections.split(",")
    if "kernels" in sections:
        res["kernels_us"] = kernels_section(ops, args, dev)
    if "pass" in sections:
        res["pass_ms"] = pass_section(ops, args, dev)
    print(json.dumps(res))
    lines = [f"scenario forecasts, N {N}, W {W}, Q {Q}, model horizon {L}, horizon {HORIZON}, S {S}, {BO} origins per batch, "
             "frozen graph"]
    for key, unit in (("kernels_us", "us"), ("pass_ms", "ms")):
        if key not in res:
            continue
        lines.append(f"[{key}] median of {args.rounds} alternating windows, {unit} per call, [(max - min) / median]")
        for name, r in res[key].items():
            cells = "  ".join(f"{k} {v['median']:.3f} [{v['spread']:.2f}]" if isinstance(v, dict) else f"{k} {v:.3f}"
                              for k, v in r.items())
            lines.append(f"  {name:<12} {cells}")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
