"""Cost of the step coupling of the copula, by the protocol of tools/copula_time.py: same process, results
checked against each other first, alternating windows, medians and the spread (max - min) / median.
Setting: the PEMS07 shape (N 228, W 12, multi 5), Q 3, model horizon 3, horizon 12 (4 rounds), S 64 paths, a loader batch of 32
origins, a frozen graph; the fit on 2520 held-out windows x 3 steps.
  launch   ops.copula_uniforms(step_factor=) (stemgnn_copula_uniforms_steps) against ops.copula_uniforms
           (stemgnn_copula_uniforms) at the 6144 rows of one round.
  pass     one batch through all four rounds: engine.scenario_rounds with a SpaceTimeCopula against a GaussianCopula of the same
           node matrix.  The condition of the issue: steps <= space * (1 + space's own spread + 0.01).
  fit      SpaceTimeCopula.fit against GaussianCopula.fit on the same rows.
One JSON line, then a text report written to --out; --append FILE adds that file's lines (the bench.py figures of the parent and
of this commit, which another process measures) to the report.
Usage: python tools/steps_copula_time.py [--sections launch,pass,fit] [--reps 20] [--rounds 7] [--out profiles/steps_copula_time.txt]"""
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
STEP_RHO = 0.8


def step_matrix(n, rho):
    ij = np.arange(n)
    return rho ** np.abs(ij[:, None] - ij[None, :]).astype(np.float64)


def copulas(C, dev):
    from stemgnn_amd.math_utils import GaussianCopula, SpaceTimeCopula
    r = C.block_matrix(N, 12, 0.6)
    return GaussianCopula.from_correlation(r, TAUS, device=dev), \
        SpaceTimeCopula.from_correlations(r, step_matrix(L, STEP_RHO), TAUS, device=dev)


def launch_section(ops, C, T, args, dev):
    from stemgnn_amd.math_utils import SpaceTimeCopula
    space, steps = copulas(C, dev)
    # first: identity steps give the existing entry's bits, at the shape that is timed
    same = SpaceTimeCopula.from_correlations(C.block_matrix(N, 12, 0.6), np.eye(L), TAUS, device=dev)
    assert torch.equal(same.uniforms(BO, S, L, 3, HORIZON, 0, SEED), space.uniforms(BO, S, L, 3, HORIZON, 0, SEED))
    assert not torch.equal(steps.uniforms(BO, S, L, 3, HORIZON, 0, SEED), space.uniforms(BO, S, L, 3, HORIZON, 0, SEED))
    block = steps.step_factor
    res = {"uniforms": T.alternate(
        {"steps": lambda: ops.copula_uniforms(steps.factor_t, BO, S, L, 3, HORIZON, seed=SEED, step_factor=block),
         "space": lambda: ops.copula_uniforms(space.factor_t, BO, S, L, 3, HORIZON, seed=SEED)},
        T.event_window_us, args.reps, args.rounds, 5)}
    res["uniforms"]["steps_over_space"] = round(res["uniforms"]["steps"]["median"] / res["uniforms"]["space"]["median"], 3)
    return res


def pass_section(ops, C, T, args, dev):
    from stemgnn_amd import Model
    from stemgnn_amd.engine import scenario_rounds
    torch.manual_seed(0)
    model = Model(N, 2, W, MULTI, horizon=L, quantiles=TAUS).to(dev).eval()
    g = torch.Generator().manual_seed(SEED + 1)
    x = torch.randn(BO, W, N, generator=g).to(dev)
    kw = dict(adjacency=model.latent_graph(x))
    space, steps = copulas(C, dev)

    def run(coupling):
        with torch.no_grad():
            return scenario_rounds(model, x, HORIZON, S, 0, SEED, coupling, "linear", kw)

    (b_t, _), (b_s, _) = run(steps), run(space)
    assert torch.equal(b_t[:, :, :L], b_s[:, :, :L])                             # round 0: the model's own rows either way
    res = {"pass": T.alternate({"steps": lambda: run(steps), "space": lambda: run(space)}, T.host_window_ms, args.pass_reps,
                               args.rounds, 3)}
    p = res["pass"]
    p["steps_over_space"] = round(p["steps"]["median"] / p["space"]["median"], 4)
    p["allowed"] = round(1.0 + p["space"]["spread"] + 0.01, 4)
    return res


def fit_section(ops, C, T, args, dev):
    from stemgnn_amd.math_utils import GaussianCopula, SpaceTimeCopula
    g = torch.Generator().manual_seed(SEED + 2)
    chol = torch.from_numpy(np.linalg.cholesky(C.block_matrix(N, 12, 0.6))).float()
    chol_t = torch.from_numpy(np.linalg.cholesky(step_matrix(L, STEP_RHO))).float()
    y = (torch.einsum("ji,cin->cjn", chol_t, torch.randn(FIT_COUNT, L, N, generator=g)) @ chol.T).to(dev)
    y[torch.rand(y.shape, generator=g).to(dev) < 0.02] = float("nan")             # 2 % missing readings
    y_hat = (torch.tensor([-1.2816, 0.0, 1.2816]).view(1, Q, 1, 1) + 0.1 * torch.randn(FIT_COUNT, Q, L, N, generator=g)).to(dev)
    space, steps = GaussianCopula(TAUS), SpaceTimeCopula(TAUS)
    space.fit(y, y_hat)
    steps.fit(y, y_hat)
    assert torch.equal(space.factor_t, steps.factor_t)                           # the node part is the same fit
    res = {"fit": T.alternate({"steps": lambda: steps.fit(y, y_hat), "space": lambda: space.fit(y, y_hat)}, T.host_window_ms,
                              args.pass_reps, args.rounds, 2)}
    res["fit"]["steps_over_space"] = round(res["fit"]["steps"]["median"] / res["fit"]["space"]["median"], 3)
    res["fit"]["max_abs_T_error"] = round(float((steps.step_correlation_raw.cpu() -
                                                 torch.from_numpy(step_matrix(L, STEP_RHO))).abs().max()), 3)
    return res


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    ap = argparse.ArgumentParser()
    ap.add_argument("--sections", default="launch,pass,fit")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pass-reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--append", default=None)
    ap.add_argument("--out", default=os.path.join(root, "profiles", "steps_copula_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "tools"))
    if not torch.cuda.is_available():
        raise SystemExit("steps_copula_time.py measures on the GPU; none found")
    dev = torch.device("cuda:0")
    import copula_time as C                                                      # the setting: shapes and the node matrix
    import scenario_time as T                                                    # the protocol: windows, alternation, medians
    from stemgnn_amd import ops
    assert (C.N, C.W, C.L, C.HORIZON, C.S, C.BO, C.FIT_COUNT) == (N, W, L, HORIZON, S, BO, FIT_COUNT)
    res = {"shape": dict(N=N, W=W, Q=Q, L=L, horizon=HORIZON, S=S, Bo=BO, fit_rows=FIT_COUNT * L), "reps": args.reps,
           "pass_reps": args.pass_reps, "rounds": args.rounds}
    sections = args.sections.split(",")
    for name, key, fn in (("launch", "launch_us", launch_section), ("pass", "pass_ms", pass_section),
                          ("fit", "fit_ms", fit_section)):
        if name in sections:
            res[key] = fn(ops, C, T, args, dev)
    print(json.dumps(res))
    lines = [f"Step coupling of the copula, N {N}, W {W}, Q {Q}, model horizon {L}, horizon {HORIZON}, S {S}, {BO} origins per "
             f"batch, frozen graph; fit on {FIT_COUNT} x {L} rows; steps = SpaceTimeCopula, space = GaussianCopula"]
    for key, unit in (("launch_us", "us"), ("pass_ms", "ms"), ("fit_ms", "ms")):
        if key not in res:
            continue
        lines.append(f"[{key}] median of {args.rounds} alternating windows, {unit} per call, [(max - min) / median]")
        for name, r in res[key].items():
            cells = "  ".join(f"{k} {v['median']:.3f} [{v['spread']:.2f}]" if isinstance(v, dict) else f"{k} {v:.4f}"
                              for k, v in r.items())
            lines.append(f"  {name:<12} {cells}")
        if key == "pass_ms":
            p = res[key]["pass"]
            lines.append(f"  condition    steps_over_space {p['steps_over_space']:.4f} <= allowed {p['allowed']:.4f} (1 + space's "
                         f"spread + 0.01): {'met' if p['steps_over_space'] <= p['allowed'] else 'NOT met'}")
    if args.append:
        with open(args.append) as fh:
            lines += [ln.rstrip("\n") for ln in fh if ln.strip()]
    text = "\n".join(lines) + "\n"
    print(text)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
