"""GPU: the folded backward mat-vec of the wave-specialised GRU recurrence (csrc/gru_cluster4.h GRU_BWD_FOLD, csrc/gru.hip
gru_matvec_fold): two units per lane, the k pairs split over the two lane halves, three v_permlane32_swap + add rounds.
The backward instantiations with one owner slice per wave and KU = 48 / 58 / 64 fold (P = 1, 2, 4); KU = 32 (hidden <= 32)
and P = 6 (two slices per wave) keep the unfolded mat-vec.

The fold keeps every chain, every chain's order and the final association (tests/test_gru_bwd_fold_map.py states the map),
so it may not move a bit:
1. against libstemgnn_hip_gruref.so (csrc/Makefile: gru.hip with the switch off, the instruction stream it replaced) every
   gradient of tests/helpers/gru_probe.py has the same SHA-256, once per folded KU and per P (one process per build for all shapes:
   tests/helpers/gru_probe_many.py);
2. against the fp64 cell on NaN-filled buffers with the bound of tests/test_hip_gru_paths.py (its draws, its cell, its
   error measure: e_kernel <= 8 max(e_ref, 2^-22) and < 1e-4), at shapes that reach every folded KU, ragged last slices with an odd
   and an even number of units and kn = 1, 2, 3 mod 4; the sequence length is a free argument of the C ABI, so 3..5 steps do;
3. two launches on the same inputs give the same bits, the factored-output-gradient entry (stemgnn_gru_bwd_rank2) included.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.test_hip_gru_packed import REF_LIB, ROOT
from tests.test_hip_gru_paths import FLOOR, K, TOL, _Abi, _aten_cpu, _cell, _draws, _plan_text, _relerr

pytestmark = pytest.mark.gpu

# gru_probe.py takes (B, W, S = Hd) -> the backward (P, KU) the plan must give
PROBES = [
    ((3, 12, 226), (4, 58), "U 57, the last workgroup owns 55 units / the last slice 55 k"),
    ((3, 12, 255), (4, 64), "U 64, last 63"),
    ((2, 3, 180), (4, 48), "U 45"),
    ((2, 12, 100), (2, 58), "P 2, U 50"),
    ((2, 3, 40), (1, 48), "P 1, U 40"),
]
# (B, S, Hd, W) -> the backward (P, KU)
CASES = [
    ((2, 4, 228, 12), (4, 58), "the headline's instantiation: U 57, nothing ragged"),
    ((3, 4, 226, 12), (4, 58), "U 57, last slice 55: the last lane pair owns one unit, kn = 3 mod 4"),
    ((3, 4, 255, 12), (4, 64), "U 64, last slice 63"),
    ((1, 3, 5, 3), (1, 32), "U 5, KU 32: not folded, beside the folded ones on the same buffers"),
    ((33, 4, 132, 3), (4, 48), "U 33, B beyond one cluster row"),
    ((2, 5, 100, 12), (2, 58), "P 2, U 50: six partial sums, kn = 2 mod 4 on every slice"),
    ((2, 5, 40, 3), (1, 48), "P 1, U 40"),
    ((2, 4, 231, 12), (4, 58), "U 58 (even), last slice 57: kn = 1 mod 4"),
    ((2, 4, 190, 12), (4, 48), "U 48 (even), last slice 46: kn = 2 mod 4"),
    ((2, 4, 229, 12), (4, 58), "U 58 (even), last slice 55: kn = 3 mod 4"),
]
IDS = ["B%d-S%d-Hd%d-W%d" % c[0] for c in CASES]


def _check_plan(B, S, Hd, W, want):
    from stemgnn_amd import _lib

    plan = _lib.gru_paths(B, S, Hd, W, 0)
    assert plan == _lib.gru_paths(B, S, Hd, W, 256), f"this device plans another path for {(B, S, Hd, W)}: {_plan_text(plan)}"
    assert plan["bwd_family"] == _lib.SG_GRU_FAM["cluster4"], _plan_text(plan)
    assert (plan["bwd_P"], plan["bwd_KU"], plan["bwd_slices"]) == want + (1,), _plan_text(plan)
    return plan


def _probe_many(lib_name):
    """{shape: gru_probe's JSON} of every PROBES shape from one process with `lib_name` loaded"""
    env = dict(os.environ)
    env["STEMGNN_HIP_LIB"] = os.path.join(ROOT, "stemgnn_amd", lib_name)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "gru_probe_many.py")]
                       + ["%d,%d,%d" % c[0] for c in PROBES], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])      # (the probe raises on a set time-out status word)
    rows = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(rows) == len(PROBES) and all(r["lib"] == lib_name for r in rows), p.stdout[-1500:]
    return {c[0]: r for c, r in zip(PROBES, rows)}


@pytest.fixture(scope="module")
def probes():
    """both builds' digests, computed once: two processes for all shapes (the library is chosen at import time)"""
    if not os.path.isfile(os.path.join(ROOT, "stemgnn_amd", REF_LIB)):
        pytest.skip(REF_LIB + " not built (python __graft_entry__.py builds it)")
    return _probe_many("libstemgnn_hip.so"), _probe_many(REF_LIB)


@pytest.mark.parametrize("shape,want,why", PROBES, ids=["B%d-W%d-Hd%d" % p[0] for p in PROBES])
def test_same_bits_as_the_unfolded_stream(shape, want, why, probes):
    B, W, Hd = shape
    _check_plan(B, Hd, Hd, W, want)
    new, ref = probes[0][shape], probes[1][shape]
    print(f"GRU {shape} ({why}): folded bwd {new['bwd_us']:.0f} us | switch off bwd {ref['bwd_us']:.0f} us")
    assert len(new["grads"]) == 4
    assert new["h"] == ref["h"], "hidden states differ from the reference build"
    assert new["grads"] == ref["grads"], "gradients differ from the unfolded build"


@pytest.mark.parametrize("shape,want,why", CASES, ids=IDS)
def test_folded_paths_vs_fp64_cell(shape, want, why, monkeypatch):
    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE", "STEMGNN_GRU_WHH_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    B, S, Hd, W = shape
    plan = _check_plan(B, S, Hd, W, want)
    t = _draws(B, S, Hd, W)
    abi = _Abi(t, B, S, Hd, W)
    h_ext, reserve = abi.fwd()
    _, dx, grads = abi.bwd("dh", h_ext, reserve)
    got = {"dh": (dx, grads)}
    dhs = [abi.d["dh"]]
    if plan["rank2_ok"]:
        dq = torch.cat([abi.nan(B * Hd), abi.d["dqpart"].reshape(-1)])
        _, dx_dq, grads_dq = abi.bwd("rank2_dq", h_ext, reserve, dq=dq)       # the progress-publishing launch of the model's step
        dq_sum = dq[: B * Hd].view(B, Hd).double()
        got["rank2_dq"] = (dx_dq, grads_dq)
        dhs.append(abi.d["dkey"].double()[None] * abi.d["wk"].double()[:, None, None]
                   + dq_sum[None] * abi.d["wq"].double()[:, None, None])
    _, g64 = _cell(abi.d, dhs, torch.float64, "cuda:0")
    _, g32 = _aten_cpu(t, dhs)
    rows = []
    for i, (label, (dxk, gk)) in enumerate(got.items()):
        for q, mine, r64, r32 in zip(("dx", "dW_ih", "dW_hh", "db_ih", "db_hh"), [dxk] + gk, g64[i], g32[i]):
            rows.append((label, q, _relerr(mine, r64), _relerr(r32.to("cuda:0"), r64)))
    print(f"GRU {shape} ({why}): {_plan_text(plan)}")
    for label, q, ek, er in rows:
        print(f"    {label:10s} {q:6s} e_kernel {ek:.2e} e_ref {er:.2e} ratio {ek / max(er, FLOOR):.2f}")
    bad = [r for r in rows if not (r[2] < TOL and r[2] <= K * max(r[3], FLOOR))]
    assert not bad, bad


@pytest.mark.parametrize("shape,want", [(CASES[1][0], CASES[1][1]), (CASES[5][0], CASES[5][1])], ids=[IDS[1], IDS[5]])
def test_folded_paths_launch_to_launch(shape, want, monkeypatch):
    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE", "STEMGNN_GRU_WHH_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    B, S, Hd, W = shape
    plan = _check_plan(B, S, Hd, W, want)
    assert plan["rank2_ok"]
    abi = _Abi(_draws(B, S, Hd, W), B, S, Hd, W)
    h_ext, reserve = abi.fwd()
    dq_sum = abi.d["dqpart"].sum(1).contiguous()
    runs = []
    for _ in range(2):
        gates, dx, grads = abi.bwd("dh", h_ext, reserve)
        gates2, dx2, grads2 = abi.bwd("rank2", h_ext, reserve, dq=dq_sum)
        runs.append([gates.view(torch.int32), dx] + grads + [gates2.view(torch.int32), dx2] + grads2)
    assert not any(torch.isnan(a.float()).any() for a in runs[0][1:6] + runs[0][7:])
    for a, b in zip(*runs):
        assert torch.equal(a, b), "backward differs from launch to launch"
