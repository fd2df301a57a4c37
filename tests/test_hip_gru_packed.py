"""GPU: the packed forward mat-vec and the vector partial-sum reads of the wave-specialised GRU recurrence
(csrc/gru_cluster4.h: GRU_FWD_PACK, GRU_PART_VEC).  The forward packs at KF = 34 and 40 (slices of 33..40 units); the KF = 32
shapes below run the unpacked mat-vec on the vector partial-sum layout.

Both keep the order of every sum, so they may not move a bit:
1. against libstemgnn_hip_gruref.so (csrc/Makefile: gru.hip with both switches off, the instruction streams they replaced)
   the hidden states and every gradient of tests/helpers/gru_probe.py have the same SHA-256, at the PEMS07 shape and at a
   small shape whose last slice is ragged in both directions;
2. against the fp64 cell on NaN-filled buffers with the bound of tests/test_hip_gru_paths.py (its draws, its cell, its
   error measure: e_kernel <= 8 max(e_ref, 2^-22) and < 1e-4), at shapes that reach every edge of the lane map
   (tests/test_gru_packed_map.py states the map) and every partial-sum row length of the backward; the sequence length is
   a free argument of the C ABI, so 3..5 steps do;
3. two launches on the same inputs give the same bits.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests.test_hip_gru_paths import FLOOR, K, TOL, _Abi, _aten_cpu, _cell, _draws, _plan_text, _relerr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = "libstemgnn_hip_gruref.so"

# (B, S, Hd, W) -> (forward P, forward K, backward P) the plan must give, and what the shape is there for
CASES = [
    ((2, 5, 228, 12), (7, 34, 4), "U 33: 99 outputs, the last workgroup owns 30 units"),
    ((2, 5, 224, 12), (7, 32, 4), "U 32, K 32: unpacked mat-vec on the vector layout, nothing ragged"),
    ((2, 5, 280, 12), (7, 40, 5), "U 40: 120 outputs, the upper limit"),
    ((3, 4, 147, 12), (7, 32, 4), "U 21, K 32: unpacked, ragged last slice"),
    ((3, 4, 154, 12), (7, 32, 4), "U 22, K 32: unpacked, nothing ragged"),
    ((1, 3, 5, 3), (7, 32, 1), "U 1, K 32: workgroups that own no unit (they leave behind the XCD check)"),
    ((33, 4, 40, 3), (1, 40, 1), "PF 1, U 40: packed without an exchange"),
    ((33, 4, 80, 3), (2, 40, 2), "PF 2, U 40"),
    ((33, 4, 132, 3), (4, 34, 4), "P 4, U 33: forward packed, 12 partial sums in the backward"),
    ((2, 5, 100, 12), (7, 32, 2), "backward P 2: 6 partial sums"),
    ((2, 5, 358, 12), (6, 64, 6), "backward P 6, two slices per wave: 9 partial sums; forward not packed (K 64)"),
    ((2, 5, 40, 3), (7, 32, 1), "backward P 1: 3 partial sums"),
]
IDS = ["B%d-S%d-Hd%d-W%d" % c[0] for c in CASES]


def _probe(lib_name, shape):
    env = dict(os.environ)
    env["STEMGNN_HIP_LIB"] = os.path.join(ROOT, "stemgnn_amd", lib_name)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "gru_probe.py")] + [str(v) for v in shape],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])      # (the probe raises on a set time-out status word)
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


# gru_probe.py takes (B, W, S = Hd).  (3, 12, 255): forward P 7, U 37, K 40 (packed), the last workgroup owns 33 units;
# backward P 4, U 64, the last workgroup owns 63
@pytest.mark.parametrize("shape", [(32, 12, 228), (3, 12, 255)], ids=["pems07", "ragged"])
def test_same_bits_as_the_unpacked_streams(shape):
    if not os.path.isfile(os.path.join(ROOT, "stemgnn_amd", REF_LIB)):
        pytest.skip(REF_LIB + " not built (python __graft_entry__.py builds it)")
    new = _probe("libstemgnn_hip.so", shape)
    ref = _probe(REF_LIB, shape)
    assert new["lib"] == "libstemgnn_hip.so" and ref["lib"] == REF_LIB
    print(f"GRU {shape}: packed fwd {new['fwd_us']:.0f} us bwd {new['bwd_us']:.0f} us | "
          f"switches off fwd {ref['fwd_us']:.0f} us bwd {ref['bwd_us']:.0f} us")
    assert new["h"] == ref["h"], "hidden states differ from the unpacked build"
    assert new["grads"] == ref["grads"], "gradients differ from the unpacked build"


def _check_plan(B, S, Hd, W, want):
    from stemgnn_amd import _lib

    plan = _lib.gru_paths(B, S, Hd, W, 0)
    assert plan == _lib.gru_paths(B, S, Hd, W, 256), f"this device plans another path for {(B, S, Hd, W)}: {_plan_text(plan)}"
    assert (plan["fwd_P"], plan["fwd_K"], plan["bwd_P"]) == want, _plan_text(plan)
    assert plan["fwd_family"] == _lib.SG_GRU_FAM["cluster4"]
    return plan


@pytest.mark.parametrize("shape,want,why", CASES, ids=IDS)
def test_packed_paths_vs_fp64_cell(shape, want, why, monkeypatch):
    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE", "STEMGNN_GRU_WHH_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    B, S, Hd, W = shape
    plan = _check_plan(B, S, Hd, W, want)
    t = _draws(B, S, Hd, W)
    abi = _Abi(t, B, S, Hd, W)
    h_ext, reserve = abi.fwd()
    assert float(h_ext[0].abs().max()) == 0.0
    h_inf, _ = abi.fwd(infer=True)
    assert torch.equal(h_inf, h_ext), "stemgnn_gru_fwd_infer: other bits than stemgnn_gru_fwd"
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
    h64, g64 = _cell(abi.d, dhs, torch.float64, "cuda:0")
    h32, g32 = _aten_cpu(t, dhs)
    rows = [("fwd", "h", _relerr(h_ext[1:], h64), _relerr(h32.to("cuda:0"), h64))]
    for i, (label, (dxk, gk)) in enumerate(got.items()):
        for q, mine, r64, r32 in zip(("dx", "dW_ih", "dW_hh", "db_ih", "db_hh"), [dxk] + gk, g64[i], g32[i]):
            rows.append((label, q, _relerr(mine, r64), _relerr(r32.to("cuda:0"), r64)))
    print(f"GRU {shape} ({why}): {_plan_text(plan)}")
    for label, q, ek, er in rows:
        print(f"    {label:10s} {q:6s} e_kernel {ek:.2e} e_ref {er:.2e} ratio {ek / max(er, FLOOR):.2f}")
    bad = [r for r in rows if not (r[2] < TOL and r[2] <= K * max(r[3], FLOOR))]
    assert not bad, bad


@pytest.mark.parametrize("shape,want", [(CASES[0][0], CASES[0][1]), (CASES[7][0], CASES[7][1])], ids=[IDS[0], IDS[7]])
def test_packed_paths_launch_to_launch(shape, want, monkeypatch):
    for name in ("STEMGNN_GRU_CLUSTER", "STEMGNN_GRU_WIDE", "STEMGNN_GRU_WHH_OVERLAP"):
        monkeypatch.delenv(name, raising=False)
    B, S, Hd, W = shape
    _check_plan(B, S, Hd, W, want)
    abi = _Abi(_draws(B, S, Hd, W), B, S, Hd, W)
    runs = []
    for _ in range(2):
        h_ext, reserve = abi.fwd()
        gates, dx, grads = abi.bwd("dh", h_ext, reserve)
        runs.append([h_ext, reserve.view(torch.int32), gates.view(torch.int32), dx] + grads)
    assert not torch.isnan(runs[0][0]).any()
    for a, b in zip(*runs):
        assert torch.equal(a, b), "forward + backward differ from launch to launch"
