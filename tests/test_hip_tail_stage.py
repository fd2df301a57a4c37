"""GPU: the last stage of the training step -- the fc tail and its losses (the 15 entries of csrc/tail.hip and the un-fused MSE
entries of csrc/data.hip) -- through the C ABI on NaN-filled, guarded buffers against fp64: the tail's counterpart of
tests/test_hip_gru_paths.py, tests/test_hip_front.py, tests/test_hip_block.py and tests/test_hip_gemm.py.

The cases come from tests/test_tail_cases.py, which proves on the CPU (stemgnn_fc_tail_plan) that they
reach every trip count of the partial-sum kernel, the loss slot in a workgroup of its own and on a second trip, ragged last blocks
of 1 and rows - 1 rows in both kernel families, W and H on the stride boundaries of the 4- and 8-thread row maps, both range limits,
and the dynamic-LDS line of the 64-row backward.

Hygiene (_train_call, _plain_call): every input sits in a guarded copy; scratch (exactly stemgnn_fc_tail_scratch_floats /
stemgnn_fc_tail_train_scratch_floats), forecast, dfsum, the four gradients, loss and norm are NaN before the call; after it every
guard band and every input bit is compared, every output element must have been written, and a repeat on re-poisoned buffers must
give the same bits.  An optional output that is not asked for (forecast = NULL, loss_accum = NULL) must stay as it was.

Inputs are those of tests/test_hip_loss_tail.case / tests/test_hip_quantile_tail.case (imported, not copied): targets at a band
distance from every kink of the loss, pre-activations away from LeakyReLU's kink, ~30 % of the targets missing with one whole (b, h)
plane and one whole row block among them -- so no element is excluded from any comparison.  The edge tests then walk ONTO the kinks on
purpose, where the header states a convention: d == 0 (targets overwritten with the forecast's own bits), z == 0 (a zero row of w0).

Reference: fp64 autograd on the CPU of the same fp32 values, for forecast, loss, dfsum and the four gradients, each under its own
max-norm (tests/util._relerr).  Two bars, both asserted for every quantity of every form and case:
    hard bar             relerr < 1e-5                                  (what tests/test_hip_tail.py holds these kernels to)
    rounding-class bar   e_kernel <= K * max(e_ref, 2^-22)              e_ref: torch's fp32 evaluation of the same reference functions
                                                                        on the device, against the same fp64 run
Bit-for-bit assertions (rows + finish == one call, `_train_loss(MSE, NULL)` == `_train`, optional outputs, loss_accum) take no
tolerance.

K = 16: the worst ratio e_kernel / max(e_ref, 2^-22) measured on an MI355X over the 2704 (quantity, form, case) comparisons of this
file, 8.91, rounded up to the next power of two.  Worst per quantity (the tests print every line, prefixed RATIO):

    quantity    ratio   case (B, N, W, H)   form            e_kernel   e_ref
    forecast     1.10   (3, 5, 63, 31)      z==0 train      2.62e-07   2.19e-07
    loss         2.40   (4, 3, 64, 1)       mse norm        5.71e-07   3.14e-08
    dfsum        2.10   (4, 3, 64, 1)       huber null      3.02e-06   1.44e-06
    dw0          3.77   (1, 257, 2, 31)     z==0 fwd+bwd    9.07e-07   2.41e-07
    db0          8.91   (1, 257, 2, 31)     fwd+bwd         2.12e-06   5.93e-08
    db2          3.80   (9, 128, 4, 1)      huber norm      6.83e-06   1.80e-06
    dw2          2.08   (4, 3, 64, 1)       huber norm      9.33e-07   4.49e-07
    dforecast    0.46   (1, 97, 15, 1)      mse_fwd/_bwd    1.11e-07   1.11e-07

One comparison is above 4 and 18 are above 2.  The 8.91 is db0 of stemgnn_fc_tail_bwd at (1, 257, 2, 31): with W = 2 the max-norm
rests on two numbers, each the sum over 257 rows of d(z) values that cancel to 1.4 % of their absolute sum (-3.00 of 177.7, -1.81 of
134.0).  The kernel adds them in a fixed order -- 64 rows per block one by one, five blocks on four lanes -- and that order alone,
replayed on the host in fp32 on correctly rounded d(z), is 8.5e-07 off; the kernel's own 31-term d(z) carry the rest.  torch's
tree-shaped sum of the same terms happens to land within 5.9e-08.  That is what fixed-order fp32 sums of M rows explain (a
running-sum bound would allow 68 * 2^-24 * 177.7 / 3.0 = 2.4e-04); a wrong block count or a dropped partial shows as 1e-3 and up, and
did in the mutants below.  The largest e_kernel anywhere is 6.83e-06 (db2 at H = 1, Huber: one number, the same kind of sum),
under the hard bar; its e_ref is 1.80e-06.

Measured, not promised: on all 23 cases the training entries' forecast equals stemgnn_fc_tail_fwd's bit for bit, and the masked
form on a target without NaN equals the unmasked form bit for bit in every output (float(1.0 / count) and 1 / (float(B) float(H)
float(N)) round alike at these sizes).  Both are asserted only to the hard bar.

What the suite found: no wrong value and no write outside a buffer, in either source file.  Mutants of csrc/tail.hip (its kernels
are the text they were before this suite) that only
change numbers (every address stays in bounds) were run against it, and each failed it: the partial-sum kernel without the
`bb < nblocks` zeroing (241 of 540 tests fail), with `i < nacc` for `i <= nacc` (290), the row kernel without `m < M` on d in the
unmasked (123) and in the masked (117) instantiation, stemgnn_fc_tail_bwd without `m < M` on its upstream gradient (33), MAE with
derivative +-scale at d == 0 (97) and pinball likewise (27).  The `m < M` guards of the stores and of the fsum loads were not
mutated: without them the kernel leaves its buffers.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_hip_loss_tail import DELTA, case as tail_case, fc64, loss64
from tests.test_hip_quantile_tail import case as quantile_case, pinball64
from tests.test_tail_cases import QUANTILE_CASES, TAIL_CASES
from tests.util import DEV, GUARD, SENTINEL, _all_nan, _bits, _Buf, _relerr, hash_seed

pytestmark = pytest.mark.gpu
TOL = 1e-5
K, FLOOR = 16, 2.0 ** -22
ACC0 = 0.5                                                       # what loss_accum holds before a call
QUANT = ("forecast", "loss", "dfsum", "dw0", "db0", "dw2", "db2")
GRADS = ("dw0", "db0", "dw2", "db2")
LOSS_FORMS = [(k, m) for k in ("mse", "mae", "huber") for m in (False, True)]
NAN, INF = float("nan"), float("inf")


def _libs():
    from stemgnn_amd import _lib

    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _filled(t):
    buf = _Buf(t.numel())
    buf.t.copy_(t.reshape(-1).to(DEV))
    return buf


def _gen(*key):
    return torch.Generator().manual_seed(hash_seed("/".join(str(k) for k in key)))


def _id(c):
    return "x".join(str(v) for v in c)


# =====================================================================================================================
# the reference: fp64 on the CPU, and the same functions in fp32 on the device
# =====================================================================================================================
def _reference(fsum, prm, y, kind, masked, taus=None, zero=None, gout=None, dtype=torch.float64, device="cpu"):
    """{forecast, loss, dfsum, dw0, db0, dw2, db2} by autograd in `dtype` on `device` from fp32 inputs.  kind "plain": no loss, the
    gradients of sum(forecast * gout).  zero: elements of the forecast [B, rows, N] whose d is exactly 0 (the forecast is replaced by
    the target there: no loss, no gradient, still counted in the normaliser)."""
    f = fsum.to(device=device, dtype=dtype).requires_grad_(True)
    ps = [p.to(device=device, dtype=dtype).requires_grad_(True) for p in prm]
    fc = fc64(f, *ps)[1]
    if kind == "plain":
        loss = (fc * gout.to(device=device, dtype=dtype)).sum()
    else:
        yy = y.to(device=device, dtype=dtype)
        fe = fc
        if zero is not None:
            B, HT, N = yy.shape
            ye = torch.nan_to_num(yy).unsqueeze(1).expand(B, fc.shape[1] // HT, HT, N).reshape(fc.shape)
            fe = torch.where(zero.to(device), ye, fc)
        with torch.device(device):                               # pinball64 builds its level tensor with torch.tensor(...)
            loss = pinball64(fe, yy, taus, masked) if kind == "pinball" else loss64(fe, yy, "mse" if kind == "train" else kind, masked)
    g = torch.autograd.grad(loss, [f] + ps)
    out = dict(zip(("dfsum",) + GRADS, (t.detach().reshape(-1) for t in g)))
    out["forecast"] = fc.detach().reshape(-1)
    out["loss"] = loss.detach().reshape(1)
    return out


def _both(fsum, prm, y, kind, masked, **kw):
    return _reference(fsum, prm, y, kind, masked, **kw), _reference(fsum, prm, y, kind, masked, dtype=torch.float32, device=DEV, **kw)


@functools.lru_cache(maxsize=None)
def _case_refs(case, kind, masked):
    c = tail_case(*case)
    return _both(c["fsum"], c["prm"], c["y_nan"] if masked else c["y"], kind, masked)


def _taus32(c):
    """the levels as the fp32 numbers the kernel gets"""
    return tuple(float(np.float32(t)) for t in c["taus"])


@functools.lru_cache(maxsize=None)
def _quantile_refs(case, masked):
    c = quantile_case(*case)
    return _both(c["fsum"], c["prm"], c["y_nan"] if masked else c["y"], "pinball", masked, taus=_taus32(c))


def _hold(title, got, ref64, ref32, names=QUANT):
    """both bars for every quantity; prints one line per quantity that the K table is collected from"""
    bad = []
    for k in names:
        assert not torch.isnan(got[k]).any(), f"{title}: {k} holds {int(torch.isnan(got[k]).sum())} NaN of {got[k].numel()}"
        e_k, e_r = _relerr(got[k].cpu(), ref64[k]), _relerr(ref32[k].cpu(), ref64[k])
        ratio = e_k / max(e_r, FLOOR)
        print(f"RATIO {k:8s} {ratio:6.2f}  {title:44s} e_kernel {e_k:.2e} e_ref {e_r:.2e}")
        if not (e_k < TOL and e_k <= K * max(e_r, FLOOR)):
            bad.append((k, e_k, e_r, ratio))
    assert not bad, (title, bad)


# =====================================================================================================================
# the calls
# =====================================================================================================================
def _accum():
    acc = torch.full((1 + GUARD // 2,), SENTINEL, dtype=torch.float64, device=DEV)
    acc[0] = ACC0
    return acc


def _train_call(dims, fsum, y, prm, kind, masked, Q=0, taus=None, want_forecast=True, want_acc=True, split=False):
    """one training-tail call (kind "train": the MSE-only entries; "mse" | "mae" | "huber": the `_loss` entries; "pinball": the
    `_quantile` entries, dims = (B, N, W, HT)) on poisoned, guarded buffers; split: `_rows*` on the current stream, `_finish*` on
    another.  Checks guards, inputs and the optional outputs; returns the outputs on the CPU (NaNs and all) + "acc", "norm",
    "scratch"."""
    _lib, lib = _libs()
    B, N, W, HT = dims
    H = HT * max(Q, 1)
    st = _stream()
    ins = [_filled(t) for t in (fsum, y, *prm)]
    before = [b.full.clone() for b in ins]
    norm = None
    if masked:
        norm = _Buf(2)
        _lib.check(lib.stemgnn_target_valid_count(ins[1].ptr(), y.numel(), norm.ptr(), st), "stemgnn_target_valid_count")
    nptr = norm.ptr() if masked else None
    sizes = dict(scratch=lib.stemgnn_fc_tail_train_scratch_floats(B, N, W, H), forecast=B * H * N, dfsum=B * N * W, dw0=W * W,
                 db0=W, dw2=H * W, db2=H, loss=1)
    assert sizes["scratch"] == _lib.fc_tail_plan(B, N, W, H)["train"]["nblocks"] * ((W + 1) * (W + H) + 1)
    o = {k: _Buf(n) for k, n in sizes.items()}
    acc = _accum()
    fptr = o["forecast"].ptr() if want_forecast else None
    aptr = acc.data_ptr() if want_acc else None
    head = [b.ptr() for b in ins] + [B, N, W, HT]
    grads = [o[k].ptr() for k in GRADS]
    if kind == "train":
        assert not masked
        one, rows, finish, mid, fin_mid = lib.stemgnn_fc_tail_train, lib.stemgnn_fc_tail_train_rows, lib.stemgnn_fc_tail_train_finish, [], []
    elif kind == "pinball":
        tarr = _lib.host_floats(taus)
        one, rows, finish = (lib.stemgnn_fc_tail_train_quantile, lib.stemgnn_fc_tail_train_rows_quantile,
                             lib.stemgnn_fc_tail_train_finish_quantile)
        mid, fin_mid = [Q, tarr, nptr], [Q, nptr]
    else:
        one, rows, finish = lib.stemgnn_fc_tail_train_loss, lib.stemgnn_fc_tail_train_rows_loss, lib.stemgnn_fc_tail_train_finish_loss
        mid, fin_mid = [_lib.SG_LOSS[kind], DELTA if kind == "huber" else 0.0, nptr], [nptr]
    if not split:
        _lib.check(one(*head, *mid, o["scratch"].ptr(), fptr, o["loss"].ptr(), aptr, o["dfsum"].ptr(), *grads, st), f"{kind} one call")
    else:
        side = torch.cuda.Stream()
        _lib.check(rows(*head, *mid, o["scratch"].ptr(), fptr, o["dfsum"].ptr(), st), f"{kind} rows")
        assert _all_nan(o["loss"].t) and all(_all_nan(o[k].t) for k in GRADS)          # `_rows` leaves them to `_finish`
        side.wait_stream(torch.cuda.current_stream())
        _lib.check(finish(o["scratch"].ptr(), B, N, W, HT, *fin_mid, o["loss"].ptr(), aptr, *grads, side.cuda_stream), f"{kind} finish")
    torch.cuda.synchronize()
    for name, b in list(zip(("fsum", "target", "w0", "b0", "w2", "b2"), ins)) + list(o.items()) + ([("norm", norm)] if masked else []):
        assert b.intact(), f"{kind}: written behind {name}"
    assert bool((acc[1:] == SENTINEL).all()), "written behind loss_accum"
    for name, b, b0 in zip(("fsum", "target", "w0", "b0", "w2", "b2"), ins, before):
        assert _bits(b.full, b0), f"{kind}: input {name} changed"
    if not want_forecast:
        assert _all_nan(o["forecast"].t), "forecast = NULL, yet the buffer was written"
    if not want_acc:
        assert float(acc[0]) == ACC0
    out = {k: b.t.cpu() for k, b in o.items()}
    out["acc"] = float(acc[0])
    out["norm"] = norm.t.cpu() if masked else None
    return out


def _written(out, names=QUANT + ("scratch",)):
    for k in names:
        assert not torch.isnan(out[k]).any(), f"{k}: {int(torch.isnan(out[k]).sum())} of {out[k].numel()} elements left NaN"


def _same(a, b, names=QUANT):
    return [k for k in names if not _bits(a[k], b[k])]


def _plain_call(dims, fsum, prm, gout=None):
    """stemgnn_fc_tail_fwd, then (gout given) stemgnn_fc_tail_bwd on poisoned, guarded buffers"""
    _lib, lib = _libs()
    B, N, W, H = dims
    st = _stream()
    ins = [_filled(t) for t in (fsum, *prm)]
    before = [b.full.clone() for b in ins]
    o = dict(forecast=_Buf(B * H * N))
    _lib.check(lib.stemgnn_fc_tail_fwd(*[b.ptr() for b in ins], B, N, W, H, o["forecast"].ptr(), st), "stemgnn_fc_tail_fwd")
    if gout is not None:
        g = _filled(gout)
        ins.append(g)
        before.append(g.full.clone())
        o.update(scratch=_Buf(lib.stemgnn_fc_tail_scratch_floats(B, N, W, H)), dfsum=_Buf(B * N * W), dw0=_Buf(W * W), db0=_Buf(W),
                 dw2=_Buf(H * W), db2=_Buf(H))
        assert o["scratch"].n == _lib.fc_tail_plan(B, N, W, H)["plain"]["nblocks"] * (W + 1) * (W + H)
        _lib.check(lib.stemgnn_fc_tail_bwd(g.ptr(), *[b.ptr() for b in ins[:4]], B, N, W, H, o["scratch"].ptr(), o["dfsum"].ptr(),
                                           *[o[k].ptr() for k in GRADS], st), "stemgnn_fc_tail_bwd")
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins) and all(b.intact() for b in o.values())
    assert all(_bits(b.full, b0) for b, b0 in zip(ins, before))
    return {k: b.t.cpu() for k, b in o.items()}


@functools.lru_cache(maxsize=None)
def _clean(case, kind, masked):
    """the one call of a form on the case's own inputs, run once and shared (outputs on the CPU, never modified)"""
    c = tail_case(*case)
    return _train_call(case, c["fsum"], c["y_nan"] if masked else c["y"], c["prm"], kind, masked)


@functools.lru_cache(maxsize=None)
def _clean_quantile(case, masked):
    B, N, W, HT, Q = case
    c = quantile_case(*case)
    return _train_call((B, N, W, HT), c["fsum"], c["y_nan"] if masked else c["y"], c["prm"], "pinball", masked, Q=Q, taus=c["taus"])


# =====================================================================================================================
# every form against fp64
# =====================================================================================================================
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_fwd_and_bwd_vs_fp64(case):
    B, N, W, H = case
    c = tail_case(*case)
    gout = torch.randn(B, H, N, generator=_gen("gout", case))
    ref64, ref32 = _both(c["fsum"], c["prm"], None, "plain", False, gout=gout)
    got = _plain_call(case, c["fsum"], c["prm"], gout)
    _written(got, ("forecast", "scratch", "dfsum") + GRADS)
    _hold(f"{case} fwd+bwd", got, ref64, ref32, ("forecast", "dfsum") + GRADS)
    again = _plain_call(case, c["fsum"], c["prm"], gout)
    assert not _same(got, again, ("forecast", "scratch", "dfsum") + GRADS)
    only_fwd = _plain_call(case, c["fsum"], c["prm"])
    assert _bits(only_fwd["forecast"], got["forecast"])


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_train_vs_fp64(case):
    got = _clean(case, "train", False)
    _written(got)
    _hold(f"{case} train", got, *_case_refs(case, "train", False))
    c = tail_case(*case)
    again = _train_call(case, c["fsum"], c["y"], c["prm"], "train", False)
    assert not _same(got, again, QUANT + ("scratch",)) and again["acc"] == got["acc"]


@pytest.mark.parametrize("kind,masked", LOSS_FORMS, ids=lambda v: {True: "norm", False: "null"}.get(v, v))
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_train_loss_vs_fp64(case, kind, masked):
    got = _clean(case, kind, masked)
    _written(got)
    c = tail_case(*case)
    if masked:
        count = int((~c["miss"]).sum())
        assert got["norm"].tolist() == [float(count), float(np.float32(1.0 / count)) if count else 0.0]
    _hold(f"{case} {kind} {'norm' if masked else 'null'}", got, *_case_refs(case, kind, masked))
    again = _train_call(case, c["fsum"], c["y_nan"] if masked else c["y"], c["prm"], kind, masked)
    assert not _same(got, again, QUANT + ("scratch",))


@pytest.mark.parametrize("masked", (False, True), ids=("null", "norm"))
@pytest.mark.parametrize("case", QUANTILE_CASES, ids=_id)
def test_train_quantile_vs_fp64(case, masked):
    B, N, W, HT, Q = case
    got = _clean_quantile(case, masked)
    _written(got)
    _hold(f"{case} pinball {'norm' if masked else 'null'}", got, *_quantile_refs(case, masked))
    c = quantile_case(*case)
    again = _train_call((B, N, W, HT), c["fsum"], c["y_nan"] if masked else c["y"], c["prm"], "pinball", masked, Q=Q, taus=c["taus"])
    assert not _same(got, again, QUANT + ("scratch",))


def _mse_calls(f, y, gl):
    """stemgnn_mse_fwd + stemgnn_mse_bwd on flat fp32 CPU tensors: (loss [1], dforecast, loss_accum)"""
    _lib, lib = _libs()
    n, st = f.numel(), _stream()
    ins = [_filled(f), _filled(y), _filled(gl)]
    before = [b.full.clone() for b in ins]
    scratch, loss, df, acc = _Buf(lib.stemgnn_mse_scratch_floats()), _Buf(1), _Buf(n), _accum()
    _lib.check(lib.stemgnn_mse_fwd(ins[0].ptr(), ins[1].ptr(), n, scratch.ptr(), loss.ptr(), acc.data_ptr(), st), "stemgnn_mse_fwd")
    _lib.check(lib.stemgnn_mse_bwd(ins[0].ptr(), ins[1].ptr(), n, ins[2].ptr(), df.ptr(), st), "stemgnn_mse_bwd")
    torch.cuda.synchronize()
    assert all(b.intact() for b in ins + [scratch, loss, df]) and bool((acc[1:] == SENTINEL).all())
    assert all(_bits(b.full, b0) for b, b0 in zip(ins, before))
    return loss.t.cpu(), df.t.cpu(), float(acc[0]), scratch.t.cpu()


def _mse_refs(f, y, gl):
    out = []
    for dtype, device in ((torch.float64, "cpu"), (torch.float32, DEV)):
        ff = f.to(device=device, dtype=dtype).requires_grad_(True)
        loss = ((ff - y.to(device=device, dtype=dtype)) ** 2).mean()
        (g,) = torch.autograd.grad(loss, ff, gl.to(device=device, dtype=dtype).reshape(()))
        out.append(dict(loss=loss.detach().reshape(1), dforecast=g.detach()))
    return out


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_mse_entries_on_the_forwards_output(case):
    c = tail_case(*case)
    f = _plain_call(case, c["fsum"], c["prm"])["forecast"]
    gl = torch.tensor([1.75])
    loss, df, acc, _ = _mse_calls(f, c["y"].reshape(-1), gl)
    _hold(f"{case} mse_fwd/_bwd", dict(loss=loss, dforecast=df), *_mse_refs(f, c["y"].reshape(-1), gl), ("loss", "dforecast"))
    assert acc == ACC0 + float(loss)


MSE_ONE_WORKGROUP = 1 << 16           # csrc/data.hip, stemgnn_mse_fwd: `n <= (size_t)1 << 16` takes the one-workgroup kernel


@pytest.mark.parametrize("n", (MSE_ONE_WORKGROUP - 1, MSE_ONE_WORKGROUP, MSE_ONE_WORKGROUP + 1, MSE_ONE_WORKGROUP + 4465))
def test_mse_fwd_on_both_sides_of_its_one_workgroup_threshold(n):
    from stemgnn_amd import _lib
    forms = [_lib.data_plan("mse_fwd", MSE_ONE_WORKGROUP + k)["form"] for k in (0, 1)]     # what the launcher itself goes by
    assert forms == [0, 1], "the threshold moved: move the sizes of this test with it"
    assert (MSE_ONE_WORKGROUP + 4465) % 256 != 0
    g = _gen("mse", n)
    f, y, gl = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.tensor([-0.625])
    loss, df, acc, scratch = _mse_calls(f, y, gl)
    two_stage = n > MSE_ONE_WORKGROUP
    assert _all_nan(scratch) != two_stage and (not two_stage or not torch.isnan(scratch).any())    # all of scratch, or none of it
    _hold(f"mse n={n}", dict(loss=loss, dforecast=df), *_mse_refs(f, y, gl), ("loss", "dforecast"))
    assert acc == ACC0 + float(loss)
    again = _mse_calls(f, y, gl)
    assert _bits(loss, again[0]) and _bits(df, again[1])


# =====================================================================================================================
# bits where the header promises them
# =====================================================================================================================
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_rows_then_finish_on_another_stream_is_the_one_call(case):
    c = tail_case(*case)
    for kind, masked in [("train", False)] + LOSS_FORMS:
        one = _clean(case, kind, masked)
        two = _train_call(case, c["fsum"], c["y_nan"] if masked else c["y"], c["prm"], kind, masked, split=True)
        assert not _same(one, two, QUANT + ("scratch",)), (kind, masked, _same(one, two, QUANT + ("scratch",)))
        assert one["acc"] == two["acc"] == ACC0 + float(one["loss"])              # exactly old + (double)loss


@pytest.mark.parametrize("masked", (False, True), ids=("null", "norm"))
@pytest.mark.parametrize("case", QUANTILE_CASES, ids=_id)
def test_quantile_rows_then_finish_and_the_optional_outputs(case, masked):
    B, N, W, HT, Q = case
    c = quantile_case(*case)
    one = _clean_quantile(case, masked)
    args = ((B, N, W, HT), c["fsum"], c["y_nan"] if masked else c["y"], c["prm"], "pinball", masked)
    two = _train_call(*args, Q=Q, taus=c["taus"], split=True)
    assert not _same(one, two, QUANT + ("scratch",))
    assert one["acc"] == two["acc"] == ACC0 + float(one["loss"])
    bare = _train_call(*args, Q=Q, taus=c["taus"], want_forecast=False, want_acc=False)
    assert not _same(one, bare, QUANT[1:] + ("scratch",))


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_unmasked_mse_loss_entry_is_the_train_entry(case):
    assert not _same(_clean(case, "train", False), _clean(case, "mse", False), QUANT + ("scratch",))
    assert _clean(case, "train", False)["acc"] == _clean(case, "mse", False)["acc"]


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_optional_outputs_change_nothing_else(case):
    c = tail_case(*case)
    for kind, masked in (("train", False), ("huber", True), ("mae", False)):
        one = _clean(case, kind, masked)
        y = c["y_nan"] if masked else c["y"]
        no_f = _train_call(case, c["fsum"], y, c["prm"], kind, masked, want_forecast=False)
        no_a = _train_call(case, c["fsum"], y, c["prm"], kind, masked, want_acc=False)
        assert not _same(one, no_f, QUANT[1:] + ("scratch",)) and no_f["acc"] == one["acc"]
        assert not _same(one, no_a, QUANT + ("scratch",))
        split = _train_call(case, c["fsum"], y, c["prm"], kind, masked, want_forecast=False, want_acc=False, split=True)
        assert not _same(one, split, QUANT[1:] + ("scratch",))


# =====================================================================================================================
# measured, not promised
# =====================================================================================================================
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_the_training_forecast_against_fwd_and_masked_against_unmasked(case):
    """Two kernels (64-row / 32-row) evaluate the same fmaf chains in the same order: the forecasts are measured against each other
    and held to the hard bar.  The masked form on a target without NaN differs from the unmasked one only in the normaliser
    (float(1.0 / count) against 1 / (float(B) float(H) float(N))): same forecast bits, everything else to the hard bar."""
    c = tail_case(*case)
    fwd = _plain_call(case, c["fsum"], c["prm"])["forecast"]
    train = _clean(case, "train", False)
    e = _relerr(train["forecast"], fwd)
    print(f"{case}: `_train` forecast == `_fwd` forecast bit for bit: {_bits(train['forecast'], fwd)} (relerr {e:.1e})")
    assert e < TOL
    for kind in ("mse", "mae", "huber"):
        un = _clean(case, kind, False)
        ma = _train_call(case, c["fsum"], c["y"], c["prm"], kind, True)
        _written(ma)
        assert ma["norm"].tolist() == [float(c["y"].numel()), float(np.float32(1.0 / c["y"].numel()))]
        assert _bits(un["forecast"], ma["forecast"])
        errs = {k: _relerr(ma[k], un[k]) for k in QUANT[1:]}
        print(f"{case} {kind}: masked on a full target == unmasked bit for bit: {not _same(un, ma)}; relerr " +
              " ".join(f"{k} {v:.1e}" for k, v in errs.items()))
        assert max(errs.values()) < TOL, errs


# =====================================================================================================================
# the edges nobody asserted
# =====================================================================================================================
def _plant_zero_d(valid, g):
    """~10 % of the valid targets (at least one, if any is valid)"""
    plant = (torch.rand(valid.shape, generator=g) < 0.1) & valid
    if valid.any() and not plant.any():
        plant.view(-1)[int(valid.reshape(-1).nonzero()[0])] = True
    return plant


@pytest.mark.parametrize("masked", (False, True), ids=("null", "norm"))
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_mae_at_d_equal_zero(case, masked):
    """sign(0) = 0: targets overwritten with the forecast's own bits have d == 0 exactly; they add nothing to the loss or to any
    gradient and still count in the normaliser.  A derivative of +-scale there would be an O(0.1) error in dfsum."""
    B, N, W, H = case
    c = tail_case(*case)
    first = _clean(case, "mae", masked)
    y = (c["y_nan"] if masked else c["y"]).clone()
    plant = _plant_zero_d(~torch.isnan(y), _gen("d0", case, masked))
    if not plant.any():
        assert masked and bool(c["miss"].all()) and B == H == 1                 # the missing (b, h) plane is the whole target: nothing
        return                                                                  # to plant; the unmasked run plants
    y[plant] = first["forecast"].reshape(B, H, N)[plant]
    got = _train_call(case, c["fsum"], y, c["prm"], "mae", masked)
    assert _bits(got["forecast"], first["forecast"])                  # so those d are exactly 0
    if masked:
        assert _bits(got["norm"], first["norm"])
    ref64, ref32 = _both(c["fsum"], c["prm"], y, "mae", masked, zero=plant)
    _hold(f"{case} mae d==0 {'norm' if masked else 'null'} ({int(plant.sum())} planted)", got, ref64, ref32)


@pytest.mark.parametrize("masked", (False, True), ids=("null", "norm"))
@pytest.mark.parametrize("case", QUANTILE_CASES, ids=_id)
def test_pinball_at_d_equal_zero(case, masked):
    """per planted target the bits of ONE level's forecast: that row's d is exactly 0 (derivative 0, the MAE convention), the
    target's other Q - 1 rows keep a real d -- only targets whose other levels stay 1e-3 away in fp64 are planted"""
    B, N, W, HT, Q = case
    c = quantile_case(*case)
    first = _clean_quantile(case, masked)
    y = (c["y_nan"] if masked else c["y"]).clone()
    g = _gen("d0 pinball", case, masked)
    f64 = fc64(c["fsum"].double(), *(p.double() for p in c["prm"]))[1].reshape(B, Q, HT, N)
    q0 = torch.randint(0, Q, (B, 1, HT, N), generator=g)
    gap = (f64 - f64.gather(1, q0)).abs()
    gap.scatter_(1, q0, INF)
    ok = (gap.min(dim=1).values > 1e-3) & ~torch.isnan(y)
    plant = _plant_zero_d(ok, g)
    if not plant.any():
        assert masked and bool(c["miss"].all()) and B == HT == 1                 # the missing (b, h) plane is the whole target
        return
    f32 = first["forecast"].reshape(B, Q, HT, N)
    y[plant] = f32.gather(1, q0).squeeze(1)[plant]
    zero = torch.zeros(B, Q, HT, N, dtype=torch.bool).scatter_(1, q0, plant.unsqueeze(1)).reshape(B, Q * HT, N)
    assert int(zero.sum()) == int(plant.sum())
    got = _train_call((B, N, W, HT), c["fsum"], y, c["prm"], "pinball", masked, Q=Q, taus=c["taus"])
    assert _bits(got["forecast"], first["forecast"])
    d = got["forecast"].reshape(B, Q, HT, N) - y.unsqueeze(1)
    assert bool((d[zero.reshape(B, Q, HT, N)] == 0).all())
    ref64, ref32 = _both(c["fsum"], c["prm"], y, "pinball", masked, taus=_taus32(c), zero=zero)
    _hold(f"{case} pinball d==0 {'norm' if masked else 'null'} ({int(plant.sum())} planted)", got, ref64, ref32)


@pytest.mark.parametrize("case", [c for c in TAIL_CASES if c[2] >= 2], ids=_id)
def test_leaky_relu_at_z_equal_zero(case):
    """a zero row t0 of w0 with b0[t0] = 0: z[:, t0] is exactly 0 in fp32 and in fp64, and both take slope 0.01 (z > 0 fails).  MSE
    forms only: the forecast moves, so the targets' distance from the MAE / Huber kinks is no longer known."""
    B, N, W, H = case
    c = tail_case(*case)
    t0 = hash_seed(_id(case)) % W
    prm = [p.clone() for p in c["prm"]]
    prm[0][t0, :] = 0.0
    prm[1][t0] = 0.0
    gout = torch.randn(B, H, N, generator=_gen("gout z0", case))
    got = _plain_call(case, c["fsum"], prm, gout)
    _hold(f"{case} z==0 fwd+bwd", got, *_both(c["fsum"], prm, None, "plain", False, gout=gout), ("forecast", "dfsum") + GRADS)
    ref64 = _reference(c["fsum"], prm, c["y"], "train", False)
    assert float(ref64["dw0"].reshape(W, W)[t0].abs().max()) > 0 and float(ref64["db0"][t0].abs()) > 0     # slope 0.01, not 0
    got = _train_call(case, c["fsum"], c["y"], prm, "train", False)
    _hold(f"{case} z==0 train", got, ref64, _reference(c["fsum"], prm, c["y"], "train", False, dtype=torch.float32, device=DEV))
    got = _train_call(case, c["fsum"], c["y_nan"], prm, "mse", True)
    _hold(f"{case} z==0 mse norm", got, *_both(c["fsum"], prm, c["y_nan"], "mse", True))


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_a_missing_target_is_selected_out_whatever_the_forecast_holds(case):
    """horizon step h0 entirely missing and b2[h0] = NaN: the forecast is NaN exactly on those rows, and nothing else notices --
    loss, dfsum and the four gradients are those of the fp64 reference with the finite b2.  (dw2's row h0 is dy * a with dy = 0 and
    a finite: the finite half of the weight-gradient caveat of include/stemgnn_hip.h.)  With norm = NULL the same input is a NaN loss."""
    B, N, W, H = case
    c = tail_case(*case)
    h0 = H - 1
    y = c["y_nan"].clone()
    y[:, h0, :] = NAN
    prm = [p.clone() for p in c["prm"]]
    prm[3][h0] = NAN
    expect = torch.zeros(B, H, N, dtype=torch.bool)
    expect[:, h0, :] = True
    for kind in ("mse", "mae", "huber"):
        got = _train_call(case, c["fsum"], y, prm, kind, True)
        assert torch.equal(torch.isnan(got["forecast"]).reshape(B, H, N), expect), kind
        for k in QUANT[1:]:
            assert bool(torch.isfinite(got[k]).all()), (kind, k)
        ref64, ref32 = _both(c["fsum"], c["prm"], y, kind, True)
        keep = ~expect.reshape(-1)
        got["forecast"], ref64["forecast"], ref32["forecast"] = got["forecast"][keep], ref64["forecast"][keep], ref32["forecast"][keep.to(DEV)]
        _hold(f"{case} {kind} b2[h0] = NaN", got, ref64, ref32, QUANT if H > 1 else QUANT[1:])
        if H == 1:
            assert all(bool((got[k] == 0).all()) for k in QUANT[1:])            # nothing valid is left
    null = _train_call(case, c["fsum"], y, prm, "mae", False)
    assert bool(torch.isnan(null["loss"]).all())


@pytest.mark.parametrize("case", QUANTILE_CASES, ids=_id)
def test_quantile_missing_step_is_selected_out(case):
    B, N, W, HT, Q = case
    c = quantile_case(*case)
    h0 = HT - 1
    y = c["y_nan"].clone()
    y[:, h0, :] = NAN
    prm = [p.clone() for p in c["prm"]]
    prm[3][[q * HT + h0 for q in range(Q)]] = NAN
    expect = torch.zeros(B, Q, HT, N, dtype=torch.bool)
    expect[:, :, h0, :] = True
    got = _train_call((B, N, W, HT), c["fsum"], y, prm, "pinball", True, Q=Q, taus=c["taus"])
    assert torch.equal(torch.isnan(got["forecast"]).reshape(B, Q, HT, N), expect)
    for k in QUANT[1:]:
        assert bool(torch.isfinite(got[k]).all()), k
    ref64, ref32 = _both(c["fsum"], c["prm"], y, "pinball", True, taus=_taus32(c))
    _hold(f"{case} pinball b2[h0] = NaN", got, ref64, ref32, QUANT[1:])
    null = _train_call((B, N, W, HT), c["fsum"], y, prm, "pinball", False, Q=Q, taus=c["taus"])
    assert bool(torch.isnan(null["loss"]).all())


@pytest.mark.parametrize("where", ("first", "last"))
@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_a_nan_row_of_fsum_stays_in_its_row(case, where):
    """row m* = (b*, n*) of fsum poisons exactly forecast[b*, :, n*] and dfsum[m*, :]; every other element of both keeps the bits of
    the clean run.  m* = 0 sits in the first block, m* = M - 1 in the last (ragged) one, next to the rows the `m < M` masks drop.
    (`_bwd` takes its upstream gradient as given, and LeakyReLU's backward selects on z: its dfsum row m* is whatever 0.01 da is, as in
    torch; the other rows are held to their bits.)"""
    B, N, W, H = case
    M = B * N
    c = tail_case(*case)
    m = 0 if where == "first" else M - 1
    b, n = divmod(m, N)
    fsum = c["fsum"].clone()
    fsum.reshape(M, W)[m, W // 2] = NAN
    in_f = torch.zeros(B, H, N, dtype=torch.bool)
    in_f[b, :, n] = True
    in_d = torch.zeros(M, W, dtype=torch.bool)
    in_d[m] = True
    clean = _clean(case, "train", False)
    got = _train_call(case, fsum, c["y"], c["prm"], "train", False)
    assert torch.equal(torch.isnan(got["forecast"]), in_f.reshape(-1)) and torch.equal(torch.isnan(got["dfsum"]), in_d.reshape(-1))
    assert _bits(got["forecast"][~in_f.reshape(-1)], clean["forecast"][~in_f.reshape(-1)])
    assert _bits(got["dfsum"][~in_d.reshape(-1)], clean["dfsum"][~in_d.reshape(-1)])
    gout = torch.randn(B, H, N, generator=_gen("gout", case))
    clean, got = _plain_call(case, c["fsum"], c["prm"], gout), _plain_call(case, fsum, c["prm"], gout)
    assert torch.equal(torch.isnan(got["forecast"]), in_f.reshape(-1))
    assert _bits(got["forecast"][~in_f.reshape(-1)], clean["forecast"][~in_f.reshape(-1)])
    assert _bits(got["dfsum"][~in_d.reshape(-1)], clean["dfsum"][~in_d.reshape(-1)])


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_all_targets_missing(case):
    c = tail_case(*case)
    y = torch.full_like(c["y"], NAN)
    for kind in ("mse", "mae", "huber"):
        got = _train_call(case, c["fsum"], y, c["prm"], kind, True)
        assert got["norm"].tolist() == [0.0, 0.0]
        assert _bits(got["forecast"], _clean(case, kind, True)["forecast"])
        for k in QUANT[1:]:
            assert bool((got[k] == 0).all()), (kind, k)
        assert got["acc"] == ACC0


@pytest.mark.parametrize("case", QUANTILE_CASES, ids=_id)
def test_quantile_all_targets_missing(case):
    B, N, W, HT, Q = case
    c = quantile_case(*case)
    got = _train_call((B, N, W, HT), c["fsum"], torch.full_like(c["y"], NAN), c["prm"], "pinball", True, Q=Q, taus=c["taus"])
    assert _bits(got["forecast"], _clean_quantile(case, True)["forecast"])
    for k in QUANT[1:]:
        assert bool((got[k] == 0).all()), k


@pytest.mark.parametrize("case", TAIL_CASES, ids=_id)
def test_an_infinite_target_under_a_mask_is_a_value(case):
    """+-inf is not a missing target: it counts in norm, the loss is +inf, and (MSE) its row of dfsum is not finite; the other rows
    keep the clean run's bits"""
    B, N, W, H = case
    M = B * N
    c = tail_case(*case)
    valid = (~c["miss"]).reshape(-1).nonzero().reshape(-1)
    y = c["y_nan"].clone()
    if len(valid) == 0:                                          # B = H = 1: the missing plane is the whole target -- give one a value
        assert B == H == 1
        valid = torch.tensor([M // 2])
        y.view(-1)[M // 2] = 0.25
        base = y.clone()
        clean_of = lambda kind: _train_call(case, c["fsum"], base, c["prm"], kind, True)
    else:
        clean_of = lambda kind: _clean(case, kind, True)
    at = int(valid[len(valid) // 2])
    b, rest = divmod(at, H * N)
    m = b * N + rest % N
    y.view(-1)[at] = -INF if at % 2 else INF
    other = torch.ones(M, W, dtype=torch.bool)
    other[m] = False
    for kind in ("mse", "mae", "huber"):
        clean, got = clean_of(kind), _train_call(case, c["fsum"], y, c["prm"], kind, True)
        assert _bits(got["norm"], clean["norm"]) and _bits(got["forecast"], clean["forecast"])
        assert float(got["loss"]) == INF, (kind, float(got["loss"]))
        assert _bits(got["dfsum"][other.reshape(-1)], clean["dfsum"][other.reshape(-1)])
        if kind == "mse":
            assert not bool(torch.isfinite(got["dfsum"].reshape(M, W)[m]).any())
        else:                                                    # the derivative is clamped: +-scale, finite
            assert bool(torch.isfinite(got["dfsum"]).all())
