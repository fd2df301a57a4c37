"""GPU: the fused fp32 GLU kernels on the wave-private weight ring (csrc/glu_fused.h, GF_PRIVATE_RING) through the C ABI:
stemgnn_block_pack -> stemgnn_spectral_glu_fwd, then stemgnn_spectral_glu_bwd with parts = 1, as tests/test_hip_block.py
drives them.  STEMGNN_GLU_FUSED is read per call: 0 = per-layer launches, 2 / 3 = fused with 64- / 96-row workgroups forced.

What is asserted, per shape and width:
  * forward: the whole `saved` buffer (out / gate of all three layers, both branches) of the fused launch has the bits of the
    per-layer launches, and the 64- and 96-row forms have each other's bits (the kernel header's "same bits");
  * data-gradient chain: the whole `scratch` of the 64-row form has the bits of the 96-row form; dG (the sum of its two
    slabs) of every setting is judged as tests/test_hip_block.py judges it -- max-norm relative error against an fp64
    evaluation of the same chain on the same fp32 values, below 1e-4 and below K = 4 times max(e_ref, 2^-22), e_ref the
    error of torch's fp32 evaluation (the constants and their derivation: that file's docstring);
  * determinism: every call is made twice back to back on one stream, on two sets of buffers, and the two have the same bits;
  * the guard bands behind every buffer read back unchanged.

Shapes (M = B N rows): one ragged block (M = 7); a ragged last block behind full ones (M = 129 = 2 x 64 + 1, and M = 197 =
2 x 96 + 5 for the 96-row form); more workgroups than the chip has CUs (M = 8448: 264 workgroups of 64 rows -- the later
ones start on a CU whose LDS ring still holds another workgroup's stages).  Widths: (W, multi) = (12, 5), two channel groups
per wave in layers 0 / 1 and one in the last (HP / NT = 2, then 1), and (7, 3), CP = 96, where every layer takes the
one-group form.  Random weights and inputs from fixed seeds.
"""
import ctypes

import pytest
import torch

from tests.util import DEV, _Buf, _bits, _relerr, dims, saved_layout, scratch_layout

pytestmark = pytest.mark.gpu
TOL, K, FLOOR = 1e-4, 4, 2.0 ** -22          # tests/test_hip_block.py: TOL, K[0], FLOOR[0] (exact fp32)
NSPLIT = 32
PARAM_NAMES = (["weight", "forecast.weight", "forecast.bias", "forecast_result.weight", "forecast_result.bias", "backcast.weight",
                "backcast.bias", "backcast_short_cut.weight", "backcast_short_cut.bias"]
               + [f"GLUs.{g}.linear_{side}.{wb}" for g in range(6) for side in ("left", "right") for wb in ("weight", "bias")])
SHAPES = [(1, 7), (3, 43), (1, 197), (32, 264)]
WIDTHS = [(12, 5), (7, 3)]
CASES = [(B, N, W, multi) for W, multi in WIDTHS for B, N in SHAPES]
MODES = ("0", "2", "3")


def _params(W, multi):
    """the 33 parameters of a StockBlock in the shapes of the reference model, values ~ N(0, 1 / fan_in) from a fixed seed"""
    from oracle import stemgnn_oracle as O

    sd = O.det_state_dict(2, W, multi, 1, seed=1, stack_cnt=1)
    g = torch.Generator().manual_seed(4099 * W + multi)
    out = []
    for k in PARAM_NAMES:
        t = sd["stock_block.0." + k]
        fan = t.shape[-1] if t.dim() > 1 else t.numel()
        out.append((torch.randn(t.shape, generator=g) / fan ** 0.5).contiguous())
    return out


class _Run:
    """packed weights + one (saved, scratch) pair per STEMGNN_GLU_FUSED setting and repetition"""

    def __init__(self, case, monkeypatch):
        from stemgnn_amd import _lib, ops

        self.lib = lib = _lib.load()
        B, N, W, multi = self.case = case
        self.d = d = dims(*case)
        st = torch.cuda.current_stream().cuda_stream
        assert lib.stemgnn_block_paths(B, N, W, multi, 0) & 3 == 3, "the fused GLU kernels do not apply to this shape"
        self.bufs = {}
        prm = [self._put(f"param{i}", t) for i, t in enumerate(_params(W, multi))]
        arr = (ctypes.c_void_p * len(prm))(*[b.ptr() for b in prm])
        tab = self._put("tables", ops.dft_tables(W, multi, torch.device(DEV)))
        self.packed = pk = self._new("packed", lib.stemgnn_packed_floats(W, multi))
        self._done(lib.stemgnn_block_pack(arr, tab.ptr(), pk.ptr(), W, multi, st), "block_pack")
        g = torch.Generator(device=DEV).manual_seed(7919 * B + 104729 * N + 31 * W + multi)
        G = torch.randn(d.M * d.KG, device=DEV, generator=g)
        n_scr = lib.stemgnn_scratch_floats(B, N, W, multi)
        self.scr0 = scr0 = 0.1 * torch.randn(n_scr, device=DEV, generator=g)   # holds d(pre-activation) of layer 2, the chain's input
        self.saved, self.scratch = {}, {}
        for mode in MODES:
            monkeypatch.setenv("STEMGNN_GLU_FUSED", mode)
            sv = [self._new(f"saved{mode}{i}", lib.stemgnn_saved_floats(B, N, W, multi)) for i in range(2)]
            sc = [self._new(f"scratch{mode}{i}", n_scr) for i in range(2)]
            gp = self._new(f"gradpart{mode}", lib.stemgnn_gradpart_floats(W, multi, NSPLIT))
            for b in sv:
                b.t[: d.M * d.KG] = G
            for b in sc:
                b.t.copy_(scr0)
            for b in sv:                                                  # twice back to back, no synchronisation between
                rc = lib.stemgnn_spectral_glu_fwd(pk.ptr(), b.ptr(), B, N, W, multi, st)
                assert rc == 0, ("spectral_glu_fwd", mode, rc)
            for i in range(2):
                rc = lib.stemgnn_spectral_glu_bwd(pk.ptr(), sv[i].ptr(), sc[i].ptr(), gp.ptr(), NSPLIT, 1, B, N, W, multi, st)
                assert rc == 0, ("spectral_glu_bwd", mode, rc)
            self._done(0, f"STEMGNN_GLU_FUSED={mode}")
            self.saved[mode], self.scratch[mode] = sv, sc
        monkeypatch.delenv("STEMGNN_GLU_FUSED")

    def _new(self, name, n):
        self.bufs[name] = _Buf(n)
        return self.bufs[name]

    def _put(self, name, t):
        b = self._new(name, t.numel())
        b.t.copy_(t.reshape(-1))
        return b

    def _done(self, rc, what):
        assert rc == 0, (what, rc)
        torch.cuda.synchronize()
        bad = [k for k, b in self.bufs.items() if not b.intact()]
        assert not bad, f"{what}: wrote behind the end of {bad}"

    # ---- the chain in torch, from the pair panels in `packed` and the saved out / gate of the per-layer forward
    def chain(self, dt):
        d, pk = self.d, self.packed.t
        sv = self.saved["0"][0].t
        SL, M, CP, KG = saved_layout(d), d.M, d.CP, d.KG
        base = M * (d.Wm + d.W + d.Wm)                                    # dpF, dpB, dig lead the scratch
        c = torch.arange(CP, device=DEV)
        ql = (c // 16) * 32 + c % 16
        off, dG = 0, torch.zeros(M, KG, device=DEV, dtype=dt)
        for r in range(2):
            wp = []
            for l in range(3):
                kin, np_ = (KG if l == 0 else CP), 2 * (CP if l < 2 else d.CP2[r])
                wp.append(pk[off: off + kin * np_].view(kin, np_).to(dt))
                off += kin * np_ + np_
            np2 = 2 * d.CP2[r]
            o2 = base + (r * 3 + 2) * M * 2 * CP
            dpre = self.scr0[o2: o2 + M * np2].view(M, np2).to(dt)
            for l in (1, 0):
                dout = dpre @ wp[l + 1].T                                   # [M, CP]
                o, rows, ld, _ = SL[f"out{r}{l}"]
                y = sv[o: o + rows * ld].view(rows, ld).to(dt)
                o, rows, ld, _ = SL[f"gate{r}{l}"]
                gt = sv[o: o + rows * ld].view(rows, ld).to(dt)
                dpre = torch.zeros(M, 2 * CP, device=DEV, dtype=dt)
                dpre[:, ql] = dout * gt
                dpre[:, ql + 16] = dout * y * (1 - gt)
            dG += dpre @ wp[0].T
        return dG

    def dG(self, mode, i=0):
        off, rows, ld, _ = scratch_layout(self.d)["dG"]
        s = self.scratch[mode][i].t[off: off + rows * ld].view(2, self.d.M, ld)
        return s[0] + s[1]


def _ids(cases):
    return ["-".join(f"{k}{v}" for k, v in zip("BNWm", c)) for c in cases]


@pytest.mark.parametrize("case", CASES, ids=_ids(CASES))
def test_glu_private_ring(case, monkeypatch):
    run = _Run(case, monkeypatch)
    # determinism: two launches back to back
    for mode in MODES:
        assert _bits(run.saved[mode][0].t, run.saved[mode][1].t), f"STEMGNN_GLU_FUSED={mode}: two forwards back to back differ"
        assert _bits(run.scratch[mode][0].t, run.scratch[mode][1].t), f"STEMGNN_GLU_FUSED={mode}: two chains back to back differ"
    # forward: same bits as the per-layer launches, 64- and 96-row forms alike
    assert not bool(torch.isnan(run.saved["0"][0].t[: saved_layout(run.d)["ig"][0]]).any()), "the forward left NaN in out / gate"
    for mode in "23":
        assert _bits(run.saved["0"][0].t, run.saved[mode][0].t), f"STEMGNN_GLU_FUSED={mode}: other bits in `saved` than the per-layer launches"
    # chain: 64- against 96-row form bitwise; every setting against fp64 under the block suite's bars
    assert _bits(run.scratch["2"][0].t, run.scratch["3"][0].t), "the 64- and 96-row data-gradient chains differ"
    r64, r32 = run.chain(torch.float64), run.chain(torch.float32)
    e_ref = _relerr(r32, r64)
    for mode in MODES:
        e = _relerr(run.dG(mode), r64)
        print(f"GLU private ring {case} FUSED={mode}: dG e_kernel {e:.2e} e_ref {e_ref:.2e} ratio {e / max(e_ref, FLOOR):.2f}")
        assert e < TOL and e <= K * max(e_ref, FLOOR), (mode, e, e_ref)
