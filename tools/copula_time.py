"""Cost of the Gaussian-copula coupling, by the protocol of tools/scenario_time.py: same process, results
checked against each other first, alternating windows, medians and the spread (max - min) / median.
Setting: the PEMS07 shape (N 228, W 12, multi 5), Q 3, model horizon 3, horizon 12 (4 rounds), S 64 paths, a loader batch of 32
origins, a frozen graph; the fit on 2520 held-out windows x 3 steps.
  kernels  ops.copula_uniforms against its torch composition (randn, a matmul with the factor, special.ndtr) at the 6144 rows of
           one round; ops.scenario_roll(uniforms=) against ops.scenario_roll (a later round, 2048 source rows).
  pass     one batch through all four rounds: engine.scenario_rounds with the copula against coupling="independent".
  fit      GaussianCopula.fit (pit, gram, the elementwise step, the host Cholesky) against the torch composition of the same
           moments (sort + compare + gather for the transform, special.ndtri, four fp64 matmuls over the masked scores, the same
           elementwise step and host Cholesky), and the two device parts of each alone.
  device   torch.profiler's device time of every kernel above, per launch, in a run of its own.
One JSON line, then a text report written to --out; --append FILE adds that file's lines (the bench.py figures of the parent and
of this commit, which another process measures) to the report.
Usage: python tools/copula_time.py [--sections kernels,pass,fit,device] [--reps 20] [--rounds 7] [--out profiles/copula_time.txt]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

N, W, MULTI, L, HORIZON, S, BO = 228, 12, 5, 3, 12, 64, 32
TAUS = (0.1, 0.5, 0.9)
Q = len(TAUS)
SEED = 7
FIT_COUNT = 2520


def block_matrix(n, block, rho):
    r = np.zeros((n, n))
    for at in range(0, n, block):
        r[at:at + block, at:at + block] = rho
    np.fill_diagonal(r, 1.0)
    return r


def torch_uniforms(factor_t, rows):
    return torch.special.ndtr(torch.randn(rows, factor_t.shape[0], device=factor_t.device) @ factor_t)


def torch_pit(y, y_hat, taus_t):
    v = torch.sort(y_hat, dim=1, stable=True).values
    i = ((v <= y[:, None]).sum(dim=1) - 1).clamp_(0, taus_t.numel() - 2)
    lo, hi = v.gather(1, i[:, None]).squeeze(1), v.gather(1, (i + 1)[:, None]).squeeze(1)
    t0, t1 = taus_t[i], taus_t[i + 1]
    u = t0 + (t1 - t0) * ((y - lo) / (hi - lo))
    return u.clamp_(2.0 ** -24, 1 - 2.0 ** -24)


def torch_gram(u):
    z = torch.special.ndtri(u.reshape(-1, u.shape[-1]).double())
    present = ~torch.isnan(z)
    p, z0 = present.double(), torch.where(present, z, torch.zeros_like(z))
    return (p.T @ p).long(), torch.stack([z0.T @ z0, z0.T @ p, (z0 * z0).T @ p])


def correlation_of(pairs, sums, shrinkage, min_pairs):
    s, a, q = sums
    m = pairs.double()
    mean = a / m
    var = q / m - mean * mean
    r = (s / m - mean * mean.T) / torch.sqrt(var * var.T)
    r = torch.where((pairs < min_pairs) | ~(var > 0) | ~(var.T > 0), torch.zeros_like(r), r)
    r.fill_diagonal_(1.0)
    r = (r + r.T) / 2
    return (1 - shrinkage) * r + shrinkage * torch.eye(r.shape[0], dtype=r.dtype, device=r.device)


def kernels_section(ops, T, args, dev):
    from stemgnn_amd.math_utils import GaussianCopula
    from tests.helpers import copula_ref as C
    cop = GaussianCopula.from_correlation(block_matrix(N, 12, 0.6), TAUS, device=dev)
    rows = BO * S * L
    # first: the kernel against the composition fed the kernel's own normals, at a small shape
    small = GaussianCopula.from_correlation(block_matrix(12, 4, 0.6), TAUS, device=dev)
    u_hip = small.uniforms(2, 5, L, 3, HORIZON, 11, SEED)
    want, _ = C.uniforms(small.factor_t.cpu().numpy().T, 11, 2, 5, HORIZON, 3, L, SEED, 0)
    assert float((u_hip.cpu().double() - torch.from_numpy(want)).abs().max()) < 1e-6
    g = torch.Generator().manual_seed(SEED)
    x1, out1 = torch.randn(BO * S, W, N, generator=g).to(dev), torch.randn(BO * S, Q, L, N, generator=g).to(dev)
    steps = torch.zeros(BO, S, HORIZON, N, device=dev)
    u = cop.uniforms(BO, S, L, 3, HORIZON, 0, SEED)
    res = {}
    res["uniforms"] = T.alternate(
        {"hip": lambda: ops.copula_uniforms(cop.factor_t, BO, S, L, 3, HORIZON, seed=SEED),
         "torch": lambda: torch_uniforms(cop.factor_t, rows)}, T.event_window_us, args.reps, args.rounds, 5)
    res["uniforms"]["hip_over_torch"] = round(res["uniforms"]["hip"]["median"] / res["uniforms"]["torch"]["median"], 3)
    res["roll_later"] = T.alternate(
        {"given": lambda: ops.scenario_roll(x1, out1, TAUS, steps, 3, uniforms=u),
         "philox": lambda: ops.scenario_roll(x1, out1, TAUS, steps, 3, seed=SEED)}, T.event_window_us, args.reps, args.rounds, 5)
    res["roll_later"]["given_over_philox"] = round(res["roll_later"]["given"]["median"] / res["roll_later"]["philox"]["median"], 3)
    return res


def pass_section(ops, T, args, dev):
    from stemgnn_amd import Model
    from stemgnn_amd.engine import scenario_rounds
    from stemgnn_amd.math_utils import GaussianCopula
    torch.manual_seed(0)
    model = Model(N, 2, W, MULTI, horizon=L, quantiles=TAUS).to(dev).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(BO, W, N, generator=g).to(dev)
    kw = dict(adjacency=model.latent_graph(x))
    cop = GaussianCopula.from_correlation(block_matrix(N, 12, 0.6), TAUS, device=dev)

    def run(coupling):
        with torch.no_grad():
            return scenario_rounds(model, x, HORIZON, S, 0, SEED, coupling, "linear", kw)

    (b_c, _), (b_i, _) = run(cop), run("independent")
    assert torch.equal(b_c[:, :, :L], b_i[:, :, :L])                             # round 0: the model's own rows either way
    res = {"pass": T.alternate({"copula": lambda: run(cop), "independent": lambda: run("independent")}, T.host_window_ms,
                               args.pass_reps, args.rounds, 3)}
    res["pass"]["copula_over_independent"] = round(res["pass"]["copula"]["median"] / res["pass"]["independent"]["median"], 4)
    return res


def fit_section(ops, T, args, dev):
    from stemgnn_amd.math_utils import GaussianCopula
    g = torch.Generator().manual_seed(SEED + 2)
    chol = torch.from_numpy(np.linalg.cholesky(block_matrix(N, 12, 0.6))).float()
    y = (torch.randn(FIT_COUNT, L, N, generator=g) @ chol.T).to(dev)
    y[torch.rand(y.shape, generator=g).to(dev) < 0.02] = float("nan")             # 2 % missing readings
    y_hat = (torch.tensor([-1.2816, 0.0, 1.2816]).view(1, Q, 1, 1) + 0.1 * torch.randn(FIT_COUNT, Q, L, N, generator=g)).to(dev)
    taus_t = torch.tensor(TAUS, device=dev)
    cop = GaussianCopula(TAUS)

    def torch_fit():
        pairs, sums = torch_gram(torch_pit(y, y_hat, taus_t))
        return np.linalg.cholesky(correlation_of(pairs, sums, cop.shrinkage, cop.min_pairs).cpu().numpy())

    cop.fit(y, y_hat)
    u = cop.pit(y, y_hat)
    pairs_t, sums_t = torch_gram(u)
    pairs_h, sums_h = ops.copula_gram(u)
    assert torch.equal(pairs_t, pairs_h) and float((sums_t - sums_h).abs().max() / sums_t.abs().max()) < 1e-12
    lower = torch_fit()
    assert float(np.abs(lower.astype(np.float32).T - cop.factor_t.cpu().numpy()).max()) < 1e-4
    res = {}
    res["fit"] = T.alternate({"hip": lambda: cop.fit(y, y_hat), "torch": torch_fit}, T.host_window_ms, args.pass_reps,
                             args.rounds, 2)
    res["pit"] = T.alternate({"hip": lambda: ops.copula_pit(y, y_hat, TAUS), "torch": lambda: torch_pit(y, y_hat, taus_t)},
                             T.host_window_ms, args.reps, args.rounds, 3)
    res["gram"] = T.alternate({"hip": lambda: ops.copula_gram(u), "torch": lambda: torch_gram(u)}, T.host_window_ms,
                              args.pass_reps, args.rounds, 2)
    for r in res.values():
        r["hip_over_torch"] = round(r["hip"]["median"] / r["torch"]["median"], 3)
    return res


def device_section(ops, T, args, dev):
    """torch.profiler's device time per kernel, in a run of its own (the windows above also hold the host's cost of a call)"""
    from torch.profiler import ProfilerActivity, profile
    from stemgnn_amd.math_utils import GaussianCopula
    cop = GaussianCopula.from_correlation(block_matrix(N, 12, 0.6), TAUS, device=dev)
    g = torch.Generator().manual_seed(SEED)
    x1, out1 = torch.randn(BO * S, W, N, generator=g).to(dev), torch.randn(BO * S, Q, L, N, generator=g).to(dev)
    y, y_hat = torch.randn(FIT_COUNT, L, N, generator=g).to(dev), torch.randn(FIT_COUNT, Q, L, N, generator=g).to(dev)
    steps = torch.zeros(BO, S, HORIZON, N, device=dev)
    u = cop.uniforms(BO, S, L, 3, HORIZON, 0, SEED)
    uf = ops.copula_pit(y, y_hat, TAUS)

    def calls():
        ops.copula_uniforms(cop.factor_t, BO, S, L, 3, HORIZON, seed=SEED)
        torch_uniforms(cop.factor_t, BO * S * L)
        ops.scenario_roll(x1, out1, TAUS, steps, 3, uniforms=u)
        ops.scenario_roll(x1, out1, TAUS, steps, 3, seed=SEED)
        ops.copula_pit(y, y_hat, TAUS)
        ops.copula_gram(uf)

    for _ in range(3):
        calls()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(args.reps):
            calls()
        torch.cuda.synchronize()
    res = {}
    for ev in prof.key_averages():
        t = getattr(ev, "device_time_total", None) or getattr(ev, "cuda_time_total", 0)
        if t and ev.count:
            res[ev.key[:70]] = round(t / ev.count, 2)
    return {"per_launch": dict(sorted(res.items(), key=lambda kv: -kv[1]))}


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="kernels,pass,fit,device")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--append", default=None)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "copula_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    if not torch.cuda.is_available():
        raise SystemExit("copula_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    import scenario_time as T                                                    # the protocol: windows, alternation, medians
    from stemgnn_amd import ops
    res = {"shape": dict(N=N, W=W, Q=Q, L=L, horizon=HORIZON, S=S, Bo=BO, fit_rows=FIT_COUNT * L), "reps": args.reps,
           "pass_reps": args.pass_reps, "rounds": args.rounds}
    sections = args.sections.split(",")
    for name, key, fn in (("kernels", "kernels_us", kernels_section), ("pass", "pass_ms", pass_section),
                          ("fit", "fit_ms", fit_section), ("device", "device_us", device_section)):
        if name in sections:
            res[key] = fn(ops, T, args, dev)
    print(json.dumps(res))
    lines = [f"Gaussian-copula coupling, N {N}, W {W}, Q {Q}, model horizon {L}, horizon {HORIZON}, S {S}, {BO} origins per batch, "
             f"frozen graph; fit on {FIT_COUNT} x {L} rows"]
    for key, unit in (("kernels_us", "us"), ("pass_ms", "ms"), ("fit_ms", "ms")):
        if key not in res:
            continue
        lines.append(f"[{key}] median of {args.rounds} alternating windows, {unit} per call, [(max - min) / median]")
        for name, r in res[key].items():
            cells = "  ".join(f"{k} {v['median']:.3f} [{v['spread']:.2f}]" if isinstance(v, dict) else f"{k} {v:.3f}"
                              for k, v in r.items())
            lines.append(f"  {name:<12} {cells}")
    if "device_us" in res:
        lines.append(f"[device_us] torch.profiler, device time per launch, us, mean of {args.reps} launches")
        lines += [f"  {v:10.2f}  {k}" for k, v in res["device_us"]["per_launch"].items()]
    if args.append:
        with open(args.append) as fh:
            lines += [ln.rstrip("\n") for ln in fh if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
