"""GPU parity of the two stages added around the spectral blocks: the persistent-kernel GRU front
(reference nn.GRU, models/base_model.py:92,137) and the Laplacian eigensolver route (north-star a-4)."""
import os

import pytest
import torch

from oracle import stemgnn_oracle as O
from tests.helpers.eigh_cases import oracle_laplacian as _laplacian
from tests.util import relerr

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.mark.parametrize("cluster", ["2", "1", "0"])
@pytest.mark.parametrize("B,S,W", [(32, 228, 12), (5, 33, 7), (3, 140, 12), (2, 300, 4), (9, 358, 12), (1, 64, 3), (4, 307, 12)])
def test_gru_fwd_bwd_vs_torch_cpu(B, S, W, cluster, monkeypatch):
    monkeypatch.setenv("STEMGNN_GRU_CLUSTER", cluster)      # 2: cluster v2 (wave-level exchange), 1: cluster v1, 0: streaming
    from stemgnn_amd.ops import GruFront

    torch.manual_seed(S + B)
    gru = torch.nn.GRU(W, S)                              # hidden size = number of nodes = sequence length
    x = torch.randn(B, W, S)
    dh = torch.randn(S, B, S)
    out, _ = gru(x.permute(2, 0, 1).contiguous())
    out.backward(dh)
    params = [p.detach().clone().cuda().requires_grad_(True)
              for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    h = GruFront.apply(x.cuda(), *params)
    h.backward(dh.cuda())
    torch.cuda.synchronize()
    from stemgnn_amd.ops import check_gru_status
    check_gru_status(torch.device("cuda:0"))
    assert relerr(h, out.detach()) < TOL
    for mine, ref in zip(params, (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)):
        assert relerr(mine.grad, ref.grad) < TOL


@pytest.mark.parametrize("B,S,W", [(32, 358, 12), (3, 384, 5), (2, 330, 20), (5, 321, 16)])
def test_gru_six_workgroup_cluster_backward_vs_torch_cpu(B, S, W, monkeypatch):
    """Hidden sizes 321..384 (PEMS03's N = 358): six workgroups per batch row, the wave-specialised backward with two owner
    slices per mat-vec wave (round 3), against torch's CPU GRU and for launch-to-launch bit reproducibility (W = 20 exceeds
    the in-recurrence dW_ih accumulation and takes the GEMM path)."""
    from stemgnn_amd.ops import GruFront, check_gru_status

    torch.manual_seed(S + B)
    gru = torch.nn.GRU(W, S)
    x = torch.randn(B, W, S)
    dh = torch.randn(S, B, S)
    out, _ = gru(x.permute(2, 0, 1).contiguous())
    out.backward(dh)
    params = [p.detach().clone().cuda().requires_grad_(True)
              for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)]
    h = GruFront.apply(x.cuda(), *params)
    h.backward(dh.cuda())
    torch.cuda.synchronize()
    check_gru_status(torch.device("cuda:0"))
    assert relerr(h, out.detach()) < TOL
    for mine, ref in zip(params, (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)):
        assert relerr(mine.grad, ref.grad) < TOL
    g1 = [p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    GruFront.apply(x.cuda(), *params).backward(dh.cuda())      # bitwise reproducible from launch to launch
    torch.cuda.synchronize()
    for a, p in zip(g1, params):
        assert torch.equal(a, p.grad)


def _rank2_backward(lib, t, side=None, poison=False, own_ctl=False):
    """dW_ih, dW_hh, db_ih, db_hh of the factored backward: the single call, or (side) _begin / _finish with the dW_hh product
    beside the recurrence."""
    from stemgnn_amd.ops import gru_status
    B, W, S = t["x"].shape
    dev = t["x"].device
    scratch = torch.empty(lib.stemgnn_gru_bwd_scratch_floats(B, S, S, W), device=dev)
    if poison:
        scratch.fill_(float("nan"))
    out = [torch.full_like(t["w_ih"], 7.0), torch.full_like(t["w_hh"], 7.0), torch.full((3 * S,), 7.0, device=dev),
           torch.full((3 * S,), 7.0, device=dev)]
    args = (t["dkey"].data_ptr(), t["dquery"].data_ptr(), t["wk"].data_ptr(), t["wq"].data_ptr(), t["x"].data_ptr(),
            t["w_hh"].data_ptr(), t["h_ext"].data_ptr(), t["reserve"].data_ptr(), B, S, S, W, scratch.data_ptr(),
            out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), gru_status(dev).data_ptr())
    main = torch.cuda.current_stream()
    if side is None:
        assert lib.stemgnn_gru_bwd_rank2(*args, main.cuda_stream) == 0
    else:
        side.wait_stream(main)
        ctl = None
        if own_ctl:                      # the graph caller's form: control words in a buffer of its own, zeroed on the side stream
            with torch.cuda.stream(side):
                ctl_t = torch.full((lib.stemgnn_gru_bwd_ctl_words(S),), -1 if poison else 0, device=dev, dtype=torch.int32)
                ctl_t.zero_()
            main.wait_stream(side)
            ctl = ctl_t.data_ptr()
        assert lib.stemgnn_gru_bwd_rank2_begin(*args, ctl, main.cuda_stream) == 0
        assert lib.stemgnn_gru_bwd_rank2_finish(*args, ctl, side.cuda_stream, main.cuda_stream) == 0
        main.wait_stream(side)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("B,S,W", [(32, 228, 12), (8, 140, 12), (16, 256, 7), (12, 96, 9), (32, 172, 16)])
def test_gru_dwhh_beside_the_recurrence_has_the_bits_of_the_single_call(B, S, W, monkeypatch):
    """Round 5: stemgnn_gru_bwd_rank2_begin / _finish run the dW_hh product on a second stream WHILE the backward recurrence
    produces its operand (progress counters, bounded waits, claims; csrc/wgrad.h WgArgs::phase).  One K partition and one
    summation order whoever computes which work item: the gradients must equal the single call's BIT FOR BIT
      * with the side launch following the recurrence (it starts beside it and polls from the first chunk on),
      * with a side launch that gives up at once (STEMGNN_GRU_WHH_TIMEOUT=0: the closing launch computes what is left),
      * with NaNs in every scratch word the calls do not write themselves,
    and match torch's CPU GRU under the factored output gradient dh[s,b,i] = dkey[b,i] wk[s] + dquery[b,i] wq[s]."""
    from stemgnn_amd import _lib
    from stemgnn_amd.ops import check_gru_status, gru_status
    lib = _lib.load()
    dev = torch.device("cuda:0")
    monkeypatch.delenv("STEMGNN_GRU_WHH_OVERLAP", raising=False)
    assert lib.stemgnn_gru_bwd_overlap_ok(B, S, S, W) == 0          # opt-in (measured neutral at the headline shape)
    monkeypatch.setenv("STEMGNN_GRU_WHH_OVERLAP", "1")               # also selects the two-level K partition of the single call
    if not lib.stemgnn_gru_bwd_overlap_ok(B, S, S, W):
        pytest.skip("shape outside the overlapped form on this device")
    torch.manual_seed(S + B)
    gru = torch.nn.GRU(W, S)
    x = torch.randn(B, W, S)
    dkey, dquery, wk, wq = torch.randn(B, S), torch.randn(B, S), torch.randn(S), torch.randn(S)
    out, _ = gru(x.permute(2, 0, 1).contiguous())
    dh = dkey[None] * wk[:, None, None] + dquery[None] * wq[:, None, None]
    out.backward(dh)
    ref = [gru.weight_ih_l0.grad, gru.weight_hh_l0.grad, gru.bias_ih_l0.grad, gru.bias_hh_l0.grad]
    t = dict(x=x.to(dev), dkey=dkey.to(dev), dquery=dquery.to(dev), wk=wk.to(dev), wq=wq.to(dev))
    w_ih, w_hh, b_ih, b_hh = (p.detach().to(dev).contiguous() for p in (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0,
                                                                         gru.bias_hh_l0))
    t.update(w_ih=w_ih, w_hh=w_hh)
    t["h_ext"] = torch.empty(S + 1, B, S, device=dev)
    t["reserve"] = torch.empty(lib.stemgnn_gru_reserve_floats(B, S, S), device=dev)
    fscr = torch.empty(lib.stemgnn_gru_fwd_scratch_floats(B, S, S), device=dev)
    assert lib.stemgnn_gru_fwd(t["x"].data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(), B, S, S, W,
                               fscr.data_ptr(), t["h_ext"].data_ptr(), t["reserve"].data_ptr(), gru_status(dev).data_ptr(),
                               torch.cuda.current_stream().cuda_stream) == 0
    single = _rank2_backward(lib, t)
    for mine, r in zip(single, ref):
        assert relerr(mine, r.to(dev)) < TOL
    side = torch.cuda.Stream()
    for label, tmo in (("following", None), ("gives up at once", "0"), ("following, poisoned scratch", None)):
        if tmo is None:
            monkeypatch.delenv("STEMGNN_GRU_WHH_TIMEOUT", raising=False)
        else:
            monkeypatch.setenv("STEMGNN_GRU_WHH_TIMEOUT", tmo)
        for rep in range(4):
            got = _rank2_backward(lib, t, side=side, poison="poisoned" in label, own_ctl=bool(rep & 1))
            for name, a, b in zip(("dw_ih", "dw_hh", "db_ih", "db_hh"), got, single):
                assert torch.equal(a, b), (label, rep, name, float((a - b).abs().max()))
    check_gru_status(dev)


@pytest.mark.parametrize("B,S,W,force", [(8, 1024, 12, False), (16, 2048, 48, False), (5, 100, 7, True), (3, 228, 12, True),
                                          (20, 600, 12, False), (2, 1500, 4, False), (16, 513, 3, False)])
def test_wide_cluster_gru_vs_torch_cpu(B, S, W, force, monkeypatch):
    """csrc/gru_wide.h: one cluster of workgroups holding W_hh as MFMA A operands for all batch rows (hidden sizes beyond
    the per-row clusters; the per-GPU shards of BASELINE configs[3] / [4] are the first two cases; B > 16 runs as
    16-column passes; `force` runs small hidden sizes through it) against torch's CPU nn.GRU, forward and every gradient."""
    if force:
        monkeypatch.setenv("STEMGNN_GRU_WIDE", "1")
    from stemgnn_amd.ops import GruFront, check_gru_status

    torch.manual_seed(S + B)
    gru = torch.nn.GRU(W, S)
    x = torch.randn(B, W, S)
    dh = torch.randn(S, B, S)
    ref_params = (gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    if S >= 1500:       # torch's CPU GRU needs minutes here (50 MB of W_hh per step): written-out fp64 cell on the device,
        rp = [p.detach().double().cuda().requires_grad_(True) for p in ref_params]   # pinned to ATen's GRU by a CPU test
        out = O.gru_manual(x.permute(2, 0, 1).contiguous().double().cuda(), *rp)
        out.backward(dh.double().cuda())
        ref_grads = [p.grad for p in rp]
        del rp
    else:
        out, _ = gru(x.permute(2, 0, 1).contiguous())
        out.backward(dh)
        ref_grads = [p.grad for p in ref_params]
    params = [p.detach().clone().cuda().requires_grad_(True) for p in ref_params]
    h = GruFront.apply(x.cuda(), *params)
    h.backward(dh.cuda())
    torch.cuda.synchronize()
    check_gru_status(torch.device("cuda:0"))
    assert relerr(h, out.detach()) < TOL
    for mine, ref in zip(params, ref_grads):
        assert relerr(mine.grad, ref) < TOL


def _gru_probe(lib_name, shape=(32, 12, 228)):
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env["STEMGNN_HIP_LIB"] = os.path.join(root, "stemgnn_amd", lib_name)
    p = subprocess.run([sys.executable, os.path.join(root, "tests", "helpers", "gru_probe.py")] + [str(v) for v in shape],
                       env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-1500:], p.stderr[-3000:])
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


def test_gru_gate_math_propagates_nan():
    """the compensated hardware-transcendental gate math clamped its arguments with fmaxf / fminf, which return
    the non-NaN operand -- a NaN pre-activation (diverged weights, bad data) came out as sigma = 0 / tanh = +-1 and the hidden
    state stayed finite.  With compare-selects a NaN in the input reaches every later hidden state, as in torch's GRU."""
    from stemgnn_amd import ops
    B, S, W = 4, 40, 6
    torch.manual_seed(0)
    gru = torch.nn.GRU(W, S).cuda()
    x = torch.randn(B, W, S, device="cuda")
    x[1, 2, 7] = float("nan")                         # batch row 1, recurrence step 7
    with torch.no_grad():
        h = ops.GruFront.apply(x, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    torch.cuda.synchronize()
    assert torch.isfinite(h[:7]).all() and torch.isfinite(h[:, [0, 2, 3]]).all()       # before it, and the other rows
    assert torch.isnan(h[7:, 1]).all()                                                  # from step 7 on, the whole row


def test_gru_hand_tuned_pauses_only_change_the_time():
    """The wave-specialised recurrence carries five s_sleep constants calibrated on one MI355X (csrc/gru_cluster4.h).  They
    only move memory traffic in time: the build with every pause set to 0 (libstemgnn_hip_untuned.so, made by
    __graft_entry__.build()) must return bit-identical hidden states and gradients, never trip the exchange time-out --
    and the test prints both timings, so a box on which the calibration no longer pays shows up in the log."""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not os.path.isfile(os.path.join(root, "stemgnn_amd", "libstemgnn_hip_untuned.so")):
        pytest.skip("libstemgnn_hip_untuned.so not built (python __graft_entry__.py builds it)")
    tuned = _gru_probe("libstemgnn_hip.so")
    untuned = _gru_probe("libstemgnn_hip_untuned.so")
    assert untuned["lib"] == "libstemgnn_hip_untuned.so"
    print(f"GRU PEMS07 shape: tuned fwd {tuned['fwd_us']:.0f} us bwd {tuned['bwd_us']:.0f} us | "
          f"no pauses fwd {untuned['fwd_us']:.0f} us bwd {untuned['bwd_us']:.0f} us")
    assert tuned["h"] == untuned["h"] and tuned["grads"] == untuned["grads"]
    # a mis-tuned pause may cost time, not correctness; the calibrated build must not be the slower one by a margin
    assert tuned["fwd_us"] + tuned["bwd_us"] < 1.3 * (untuned["fwd_us"] + untuned["bwd_us"])


@pytest.mark.parametrize("N,sweeps", [(228, 0), (33, 0), (64, 0), (140, 0), (5, 0), (321, 0), (1024, 0), (2048, 0),
                                      (228, 9), (33, 9), (64, 9), (140, 9)])
def test_eigh_stage_reproduces_chebyshev_basis(N, sweeps):
    """stemgnn_eigh_fwd at the sizes of every BASELINE config: sweeps = 0 is the direct solver (Householder cluster
    kernel -> fp64 multisection -> fp64 inverse iteration -> back-transform; N = 321 / 1024 / 2048 use several
    workgroups with the grid barrier), sweeps = 9 the one-sided Jacobi of round 1."""
    from stemgnn_amd import _lib, ops

    lib = _lib.load()
    L = _laplacian(N, B=6 if N <= 256 else 2)
    mul_L = torch.zeros(4, N, N, device="cuda")
    mul_L[1] = L.cuda()
    lam = torch.empty(N, device="cuda")
    U = torch.empty(N, N, device="cuda")
    scratch = torch.empty(lib.stemgnn_eigh_scratch_floats(N), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.stemgnn_eigh_fwd(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), scratch.data_ptr(), N, sweeps, st) == 0
    torch.cuda.synchronize()
    ops.check_eigh_status()
    ref = O.cheb_polynomial(L.double())
    assert relerr(mul_L[2], ref[2]) < TOL and relerr(mul_L[3], ref[3]) < TOL
    assert torch.equal(mul_L[1].cpu(), L) and float(mul_L[0].abs().max()) == 0.0
    Ud = U.cpu().double()
    assert float((Ud @ Ud.T - torch.eye(N, dtype=torch.float64)).abs().max()) < 1e-5            # orthogonality
    assert relerr((Ud.T * lam.cpu().double()) @ Ud, L.double()) < 1e-5                           # L = U^T diag(lam) U
    ev = torch.linalg.eigvalsh(L.double())
    assert float((torch.sort(lam.cpu().double()).values - ev).abs().max()) < 1e-5


@pytest.mark.parametrize("N,batch", [(228, 8), (64, 5), (140, 3), (321, 2)])
def test_eigh_batched_equals_one_call_per_matrix(N, batch):
    """stemgnn_eigh_batched (north_star: "a batched N x N symmetric eigensolver"): `batch` different Laplacians in one call
    (the batch is a grid dimension of every stage; N = 321 runs the multi-workgroup tridiagonalisation matrix by matrix) give,
    matrix by matrix, bit for bit what stemgnn_eigh_fwd gives -- eigenvalues, eigenvectors and the rebuilt T2 / T3 slots."""
    from stemgnn_amd import _lib, ops

    lib = _lib.load()
    dev = torch.device("cuda")
    S = lib.stemgnn_eigh_scratch_floats(N)
    assert S % 4 == 0
    mats = [_laplacian(N, B=3, seed=10 + m) for m in range(batch)]
    mul_L = torch.zeros(batch, 4, N, N, device=dev)
    for m in range(batch):
        mul_L[m, 1] = mats[m].to(dev)
    lam = torch.empty(batch, N, device=dev)
    U = torch.empty(batch, N, N, device=dev)
    scratch = torch.empty(batch * S, device=dev)
    st = torch.cuda.current_stream().cuda_stream
    assert lib.stemgnn_eigh_batched(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), scratch.data_ptr(), N, batch, st) == 0
    torch.cuda.synchronize()
    ops.check_eigh_status()
    for m in range(batch):
        one = torch.zeros(4, N, N, device=dev)
        one[1] = mats[m].to(dev)
        lam1, U1 = torch.empty(N, device=dev), torch.empty(N, N, device=dev)
        scr1 = torch.empty(S, device=dev)
        assert lib.stemgnn_eigh_fwd(one.data_ptr(), lam1.data_ptr(), U1.data_ptr(), scr1.data_ptr(), N, 0, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(lam[m], lam1) and torch.equal(U[m], U1) and torch.equal(mul_L[m], one), m
        ev = torch.linalg.eigvalsh(mats[m].double())
        assert float((torch.sort(lam[m].cpu().double()).values - ev).abs().max()) < 1e-5
    assert lib.stemgnn_eigh_batched(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), scratch.data_ptr(), N, 0, st) != 0


def _degenerate(kind, N):
    g = torch.Generator().manual_seed(3)
    if kind == "rank_one":            # I - 11^T/N: eigenvalue 1 with multiplicity N - 1 (constant series give this Laplacian)
        return torch.eye(N) - torch.ones(N, N) / N
    if kind == "twin_blocks":         # two identical diagonal blocks: EVERY eigenvalue is double (duplicated series)
        a = torch.randn(N // 2, N // 2, generator=g) * 0.2
        a = (a + a.T) / 2
        z = torch.zeros_like(a)
        return torch.cat([torch.cat([a, z], 1), torch.cat([z, a], 1)], 0)
    if kind == "tight":               # distinct eigenvalues 1e-12 apart inside groups of five (fp64 cannot separate them)
        q, _ = torch.linalg.qr(torch.randn(N, N, generator=g, dtype=torch.float64))
        lam = torch.linspace(-1, 1, N // 5, dtype=torch.float64).repeat_interleave(5)[:N]
        lam = lam + 1e-12 * torch.arange(N, dtype=torch.float64)
        return ((q * lam) @ q.T).float()
    if kind == "split_pairs":         # already tridiagonal and split: T = L exactly, two eigenvalues of multiplicity N / 2
        return torch.kron(torch.eye(N // 2), torch.tensor([[0.3, 0.2], [0.2, 0.3]]))
    raise ValueError(kind)


@pytest.mark.parametrize("kind,N", [("split_pairs", 64), ("split_pairs", 300), ("rank_one", 96), ("twin_blocks", 128),
                                    ("tight", 100), ("twin_blocks", 512)])
def test_eigh_repeated_eigenvalues_keep_an_orthonormal_basis(kind, N):
    """Exactly repeated / numerically coincident eigenvalues: independent inverse iteration would return
    parallel vectors and a rank-deficient U; the cluster pass must hand back an orthonormal basis so that the rebuilt
    slots are still the polynomials of L."""
    from stemgnn_amd import _lib, ops

    lib = _lib.load()
    L = _degenerate(kind, N)
    L = ((L + L.T) / 2).contiguous()
    mul_L = torch.zeros(4, N, N, device="cuda")
    mul_L[1] = L.cuda()
    lam = torch.empty(N, device="cuda")
    U = torch.empty(N, N, device="cuda")
    scratch = torch.empty(lib.stemgnn_eigh_scratch_floats(N), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    lib.stemgnn_eigh_cluster_fixes()                                  # clear the diagnostic counter
    assert lib.stemgnn_eigh_fwd(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), scratch.data_ptr(), N, 0, st) == 0
    torch.cuda.synchronize()
    ops.check_eigh_status()
    fixes = lib.stemgnn_eigh_cluster_fixes()
    print(f"{kind} N={N}: {fixes} eigenvectors re-orthogonalised by the cluster pass")
    if kind == "split_pairs":         # every reflector is the identity here, so the clusters are exact by construction
        assert fixes == N - 2, "the cluster pass did not run on a clustered spectrum"
    Ud = U.cpu().double()
    assert float((Ud @ Ud.T - torch.eye(N, dtype=torch.float64)).abs().max()) < 2e-5
    Ld = L.double()
    assert relerr((Ud.T * lam.cpu().double()) @ Ud, Ld) < 2e-5
    ref2 = 2 * Ld @ Ld
    ref3 = 2 * Ld @ ref2 - Ld
    assert relerr(mul_L[2], ref2) < TOL and relerr(mul_L[3], ref3) < TOL
    ev = torch.linalg.eigvalsh(Ld)
    assert float((torch.sort(lam.cpu().double()).values - ev).abs().max()) < 1e-5


def test_eigh_without_clusters_skips_the_cluster_pass():
    from stemgnn_amd import _lib

    lib = _lib.load()
    N = 140
    mul_L = torch.zeros(4, N, N, device="cuda")
    mul_L[1] = _laplacian(N).cuda()
    lam, U = torch.empty(N, device="cuda"), torch.empty(N, N, device="cuda")
    scratch = torch.empty(lib.stemgnn_eigh_scratch_floats(N), device="cuda")
    lib.stemgnn_eigh_cluster_fixes()
    assert lib.stemgnn_eigh_fwd(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), scratch.data_ptr(), N, 0,
                                torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert lib.stemgnn_eigh_cluster_fixes() == 0


def test_model_eig_route_matches_oracle(monkeypatch):
    from stemgnn_amd import Model

    monkeypatch.setenv("STEMGNN_SPECTRAL", "eig")
    N, W, multi, H, B = 60, 12, 5, 3, 8
    sd = O.det_state_dict(N, W, multi, H, seed=4)
    model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0)
    model.load_state_dict(sd)
    model.cuda().train()
    torch.manual_seed(5)
    x, y = torch.randn(B, W, N), torch.randn(B, H, N)
    forecast, att = model(x.cuda())
    torch.nn.functional.mse_loss(forecast, y.cuda()).backward()
    o_loss, o_forecast, o_att, o_grads = O.loss_and_grads(x, y, sd)
    assert relerr(forecast, o_forecast) < TOL and relerr(att, o_att) < TOL
    for k, p in model.named_parameters():
        if o_grads[k] is not None:
            assert relerr(p.grad, o_grads[k]) < TOL, k


def test_model_eig_route_train_mode_with_dropout(monkeypatch):
    """The eigen route in TRAIN mode with the kernels' own Philox dropout: same seed -> the eig and the Chebyshev
    routes see the same mask, so forecast, attention and every gradient must agree (the basis is the same function of
    L; the backward is the polynomial one either way) -- and the Chebyshev route is pinned to the oracle with the
    exported mask by test_train_mode_dropout_matches_oracle_with_exported_mask."""
    from stemgnn_amd import Model

    N, W, multi, H, B = 60, 12, 5, 3, 8
    sd = O.det_state_dict(N, W, multi, H, seed=9)
    torch.manual_seed(6)
    x, y = torch.randn(B, W, N).cuda(), torch.randn(B, H, N).cuda()
    res = {}
    for route in ("cheb", "eig"):
        monkeypatch.setenv("STEMGNN_SPECTRAL", route)
        model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.5)
        model.load_state_dict(sd)
        model.cuda().train()
        model.set_dropout_seed(1234, 7)
        forecast, att = model(x)
        torch.nn.functional.mse_loss(forecast, y).backward()
        res[route] = (forecast.detach(), att.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    assert relerr(res["eig"][0], res["cheb"][0]) < TOL and relerr(res["eig"][1], res["cheb"][1]) < TOL
    for k, g in res["cheb"][2].items():
        assert relerr(res["eig"][2][k], g) < TOL, k


@pytest.mark.parametrize("N,B", [(228, 8), (358, 4), (1024, 2)])
def test_model_eig_route_at_real_sizes(N, B, monkeypatch):
    """The eigen route INSIDE the model at the sizes of BASELINE configs[1], [2], [3] (only N = 60, the
    one-workgroup register-resident kernel, was covered): N = 228 runs the register-resident tridiagonalisation, N = 358 and
    1024 the multi-workgroup grid-barrier kernel.  T_k(L) = U p_k(Lambda) U^T is the same function of L as the two Chebyshev
    products, so forecast, attention and every parameter gradient of the two routes must agree; the Chebyshev route is
    pinned to the oracle at these shapes by test_hip_parity."""
    from stemgnn_amd import Model, ops

    W, multi, H = 12, 5, 3
    sd = O.det_state_dict(N, W, multi, H, seed=11)
    torch.manual_seed(N)
    x, y = torch.randn(B, W, N).cuda(), torch.randn(B, H, N).cuda()
    res = {}
    for route in ("cheb", "eig"):
        monkeypatch.setenv("STEMGNN_SPECTRAL", route)
        model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0)
        model.load_state_dict(sd)
        model.cuda().train()
        forecast, att = model(x)
        torch.nn.functional.mse_loss(forecast, y).backward()
        torch.cuda.synchronize()
        res[route] = (forecast.detach(), att.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    ops.check_eigh_status(torch.device("cuda:0"))
    ops.check_gru_status(torch.device("cuda:0"))
    assert relerr(res["eig"][0], res["cheb"][0]) < TOL and relerr(res["eig"][1], res["cheb"][1]) < TOL
    for k, g in res["cheb"][2].items():
        assert relerr(res["eig"][2][k], g) < TOL, (k, relerr(res["eig"][2][k], g))


def test_eig_route_inside_the_hipgraph_train_step(monkeypatch):
    """STEMGNN_SPECTRAL=eig through engine.TrainStep at the headline shape: the seven launches of the direct solver are
    captured with the rest of the step (one hipGraph replay per batch) and the training losses track the Chebyshev
    route's (same seeds, same dropout stream)."""
    from stemgnn_amd import Model, ops
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    N, W, multi, H, B, T = 228, 12, 5, 3, 32, 600
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(2)
    series = torch.randn(T, N, generator=g).to(dev)
    hi = (torch.randperm(T - W - H, generator=g)[: 6 * B] + W).view(6, B).to(dev)
    losses, modes = {}, {}
    for route in ("cheb", "eig"):
        monkeypatch.setenv("STEMGNN_SPECTRAL", route)
        torch.manual_seed(0)
        model = Model(N, 2, W, multi, horizon=H).to(dev).train()
        model.set_dropout_seed(77, 0)
        opt = FusedRMSprop(model.parameters(), lr=1e-4, eps=1e-8)
        step = TrainStep(model, opt, B, W, H, N, series=series)
        out = []
        for i in range(6):
            step.run_indices(hi[i])
            out.append(float(step.loss.item()))
        losses[route], modes[route] = out, step.mode
    ops.check_eigh_status(dev)
    assert modes["eig"] == "hipgraph(whole step)", modes
    assert all(abs(a - b) <= 2e-4 * abs(b) for a, b in zip(losses["eig"], losses["cheb"])), losses


def test_miopen_gru_switch_gives_same_result(monkeypatch):
    from stemgnn_amd import Model

    N, W, multi, H, B = 40, 12, 5, 3, 4
    sd = O.det_state_dict(N, W, multi, H, seed=6)
    model = Model(N, 2, W, multi, horizon=H, dropout_rate=0.0)
    model.load_state_dict(sd)
    model.cuda().train()
    x = torch.randn(B, W, N).cuda()
    f_hip, _ = model(x)
    monkeypatch.setenv("STEMGNN_GRU", "miopen")
    f_lib, _ = model(x)
    assert relerr(f_hip, f_lib.detach().cpu()) < TOL
