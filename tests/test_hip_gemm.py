"""GPU: the seven entries of csrc/splitgemm.hip through the C ABI on NaN-filled, guarded buffers against fp64 -- the GEMM counterpart
of tests/test_hip_front.py and tests/test_hip_block.py, and the one direct window onto sg_gemm2 (csrc/gemm2.h).

The cases come from tests/test_gemm_cases.py, which proves on the CPU (stemgnn_sgemm_paths, the launch's own plan) that they reach
every orientation of stemgnn_sgemm_f32 on both loader pairs, every reason for the scalar pair, and the wrap of the XCD tile
grouping (nx = 9 row tiles, ny = 3 column tiles).  Each GEMM call here asks the query again with the pointers it really passes and
fails if the launch would not take the loaders the table names.

Hygiene: every input sits in a _Buf of exactly its layout's footprint, (rows - 1) * ld + extent floats plus the one-float offset
where the case has one, NaN outside the logical elements (a loader that uses a gap element poisons the product); every output is NaN
before the call, or holds known values for accumulate = 1; guard bands, the inputs' bits and the ldc - N gap columns of C are
compared after every call.  The planes of the split-bf16 entries are prefilled with bf16 NaNs in both halves of every float.

Checks.  Integer operands from [-8, 8] (K <= 68: every partial sum is an integer below 2^24) must give the fp64 product bit for bit,
on every case and for accumulate 0 and 1 -- no tolerance to hide a misplaced, missing or doubled term.  (Only the sign of a zero
is not compared: it depends on the order of the sum.)  Real operands are bounded element by element, with u = 2^-24 and
g(n) = n u / (1 - n u):
    stemgnn_sgemm_f32, stemgnn_glu_gemm_f32   |C - ref| <= g(2 K + 2) (|A| |B| + |C_old|)       at most two roundings per term
    stemgnn_glu_gemm_bf16                     |C - ref| <= (t_s + g(T_s Kp + 1)) |A| |B|          Kp = K rounded up to 32
        splits 1: T = 1, t = 2^-7 (two operand roundings of 2^-8); 2: T = 3, t = 3 * 2^-16 (mid * mid and the two residuals);
        3: T = 6, t = 2^-22 (the three dropped products)
    stemgnn_colsum                            |out - ref| <= g(M) sum |x|
all derived, none measured.  Worst ratio of the error to its bound on an MI355X, per test (the tests print it per case):

    test                                           worst ratio   case
    sgemm (1,1) vector / scalar                    0.321 / 0.041   516x260x4 ldc+3, accumulate / 63x129x52 offA
    sgemm (1,0) vector / scalar                    0.034 / 0.318   132x128x52 / 516x260x3, accumulate
    sgemm (0,1) vector / scalar                    0.305 / 0.349   516x260x4, accumulate / 516x260x2 offB, accumulate
    sgemm (0,0) vector / scalar                    0.309 / 0.273   516x260x3 / 516x260x4 offA
    glu_gemm_f32                                   0.250           (130, 127, 3)
    glu_gemm_bf16 splits 1 / 2 / 3                 0.665 / 0.195 / 0.014   (130, 1, 4) / (63, 127, 28) / (63, 127, 28)
    colsum                                         0.517           (3, 65)
(the short sums sit closest to their bound: at K = 52 the running-sum bound allows 106 roundings and the errors cancel; the
planted-NaN test holds every untouched element to the same bound.)  Both loader pairs of every orientation ran, form (0,1) --
which nothing else in the repository executes -- included.

stemgnn_glu_combine_fwd / _bwd are bounded as the block suite bounds its stages: with e the max-norm relative error against the fp64
formula, e_kernel <= COMBINE_K * max(e_ref, 2^-23), e_ref the error of the same formula evaluated in fp32 by torch on the CPU from
the same inputs and 2^-23 the spacing of fp32 (e_ref is 0 where torch and the kernel round alike, as for lin = U + bl).

Measured on an MI355X over the five shapes: e_kernel equals e_ref to the digits printed for every output (the kernel and torch
round alike at the element that decides the max-norm), every e_ref is below 2^-23, so the worst e_kernel / max(e_ref, 2^-23) is
    out 0.98   gate 0.75   lin 0.37   dU 0.35   dV 0.81      (all at (4100, 257); e_kernel 1.16e-07, 9.00e-08, 4.44e-08, 4.15e-08,
                                                              9.64e-08)
and the largest e_kernel / e_ref is 1.00: COMBINE_K = 4, the block suite's factor, has room to spare and nothing calls for another.
"""
import math

import pytest
import torch

from tests.test_gemm_cases import GEMM_CASES, GLU_CASES, GLU_CASES_F32, nan_cases, query, real_cases
from tests.util import _all_nan, _bits, _Buf, hash_seed

pytestmark = pytest.mark.gpu
U32 = 2.0 ** -24
COMBINE_K, COMBINE_FLOOR = 4, 2.0 ** -23
SPLIT_T = {1: 1, 2: 3, 3: 6}                                    # bf16 products per term
SPLIT_TRUNC = {1: 2.0 ** -7, 2: 3 * 2.0 ** -16, 3: 2.0 ** -22}
BF16_NAN_PAIR = 0x7FC07FC0                                       # a float32 NaN whose two halves are bf16 NaNs


def gamma(n):
    return n * U32 / (1 - n * U32)


def _libs():
    from stemgnn_amd import _lib

    return _lib, _lib.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync():
    torch.cuda.synchronize()


def _gen(*key):
    return torch.Generator().manual_seed(hash_seed("/".join(str(k) for k in key)))


def _ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


def _same_numbers(got, ref64):
    """got (fp32) holds the fp64 values bit for bit; ref64 must be exact in fp32; +0 and -0 count as the same number"""
    ref32 = ref64.float()
    assert torch.equal(ref32.double(), ref64)
    return _bits(got + 0.0, ref32 + 0.0)


def _mismatch(got, ref64):
    bad = (got.double() != ref64) | torch.isnan(got)
    idx = bad.nonzero()
    return f"{int(bad.sum())} of {bad.numel()} elements differ, first at {idx[0].tolist() if len(idx) else None}"


def _worst(err, bound):
    """max of err / bound over the elements (an error where the bound is 0 counts as inf)"""
    return float(torch.nan_to_num(err / bound, nan=0.0, posinf=math.inf).max())


# =====================================================================================================================
# stemgnn_sgemm_f32
# =====================================================================================================================
def _operand(logical, kcontig, ld, off):
    """logical[i, k] (CPU fp32) -> a guarded device buffer of exactly its footprint that holds it k-contiguous (element (i, k) at
    i * ld + k) or not (at k * ld + i), `off` floats behind the buffer's start; everything else in the buffer is NaN"""
    I, K = logical.shape
    rows, extent = (I, K) if kcontig else (K, I)
    buf = _Buf((rows - 1) * ld + extent + off)
    torch.as_strided(buf.t, (I, K), (ld, 1) if kcontig else (1, ld), off).copy_(logical.to(buf.t.device))
    return buf, buf.ptr() + 4 * off


def _sgemm(c, A, B, acc, prefill=None):
    """run one case: A [M, K], B [N, K] logical (B[j, k] = element (k, j) of the right operand), prefill the c_floats of C or None
    (NaN).  Returns C's [M, N] on the CPU after checking the plan, the guards, the inputs' bits and the gap columns."""
    _lib, lib = _libs()
    a_buf, a_ptr = _operand(A, c.akc, c.lda, c.offA)
    b_buf, b_ptr = _operand(B, c.bkc, c.ldb, c.offB)
    assert a_buf.n == c.a_floats + c.offA and b_buf.n == c.b_floats + c.offB
    c_buf = _Buf(c.c_floats)
    if prefill is not None:
        c_buf.t.copy_(prefill.to(c_buf.t.device))
    a0, b0, c0 = a_buf.full.clone(), b_buf.full.clone(), c_buf.t.clone()
    vec, nx, ny, _ = query(lib, c, a_ptr, b_ptr)
    assert vec == c.vec and (nx, ny) == (c.nx, c.ny), (c, vec, nx, ny)         # the launch takes the loaders the table names
    _lib.check(lib.stemgnn_sgemm_f32(a_ptr, c.lda, c.akc, b_ptr, c.ldb, c.bkc, c_buf.ptr(), c.ldc, c.M, c.N, c.K, acc, _stream()),
               "stemgnn_sgemm_f32")
    _sync()
    assert a_buf.intact() and b_buf.intact() and c_buf.intact(), c
    assert _bits(a_buf.full, a0) and _bits(b_buf.full, b0), c
    inside = torch.zeros(c.c_floats, dtype=torch.bool)
    torch.as_strided(inside, (c.M, c.N), (c.ldc, 1)).fill_(True)
    assert int((~inside).sum()) == (c.M - 1) * c.dldc
    assert _bits(c_buf.t.cpu()[~inside], c0.cpu()[~inside]), f"{c}: a gap column of C changed"
    return torch.as_strided(c_buf.t, (c.M, c.N), (c.ldc, 1)).cpu()


def _old(c, prefill):
    return torch.as_strided(prefill, (c.M, c.N), (c.ldc, 1)).double()


@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("c", GEMM_CASES, ids=lambda c: c.id)
def test_sgemm_integer_operands_give_the_fp64_product_bit_for_bit(c, acc):
    g = _gen(c.id, acc)
    A, B = _ints(g, c.M, c.K), _ints(g, c.N, c.K)
    prefill = _ints(g, c.c_floats) if acc else None
    ref = A.double() @ B.double().T
    if acc:
        ref = ref + _old(c, prefill)
    got = _sgemm(c, A, B, acc, prefill)
    assert not torch.isnan(got).any(), f"{c}: {int(torch.isnan(got).sum())} elements of [M, N] were left NaN"
    assert _same_numbers(got, ref), f"{c}: {_mismatch(got, ref)}"


@pytest.mark.parametrize("acc", (0, 1))
@pytest.mark.parametrize("c", real_cases(), ids=lambda c: c.id)
def test_sgemm_real_operands_stay_within_the_running_sum_bound(c, acc):
    g = _gen(c.id, acc, "real")
    A, B = torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g)
    prefill = torch.randn(c.c_floats, generator=g) if acc else None
    ref, mag = A.double() @ B.double().T, A.double().abs() @ B.double().abs().T
    if acc:
        ref, mag = ref + _old(c, prefill), mag + _old(c, prefill).abs()
    got = _sgemm(c, A, B, acc, prefill)
    assert not torch.isnan(got).any()
    err, bound = (got.double() - ref).abs(), gamma(2 * c.K + 2) * mag
    print(f"sgemm {c.id} acc={acc} ({'vector' if c.vec else 'scalar'}): worst |C - ref| / bound {_worst(err, bound):.3f}")
    assert bool((err <= bound).all()), f"{c}: worst ratio {_worst(err, bound):.3f}"


@pytest.mark.parametrize("where", ("first", "last"))
@pytest.mark.parametrize("c", nan_cases(), ids=lambda c: c.id)
def test_sgemm_a_planted_nan_poisons_its_row_or_column_only(c, where):
    """A NaN at A(i0, k0) must make exactly row i0 of C NaN, one at B(k0, j0) exactly column j0: element (0, 0) is what every
    out-of-range lane of the loaders clamps to and must then discard; the last row / column / k sit in the ragged tile."""
    i0, j0, k0 = (0, 0, 0) if where == "first" else (c.M - 1, c.N - 1, c.K - 1)
    g = _gen(c.id, where)
    A, B = torch.randn(c.M, c.K, generator=g), torch.randn(c.N, c.K, generator=g)
    ref, mag = A.double() @ B.double().T, A.double().abs() @ B.double().abs().T
    bound = gamma(2 * c.K + 2) * mag
    for operand in ("A", "B"):
        An, Bn, expect = A.clone(), B.clone(), torch.zeros(c.M, c.N, dtype=torch.bool)
        if operand == "A":
            An[i0, k0] = float("nan")
            expect[i0, :] = True
        else:
            Bn[j0, k0] = float("nan")
            expect[:, j0] = True
        got = _sgemm(c, An, Bn, 0)
        assert torch.equal(torch.isnan(got), expect), (c, operand, int(torch.isnan(got).sum()), int(expect.sum()))
        err = (got.double() - ref).abs()
        assert bool((err <= bound)[~expect].all()), (c, operand)


# =====================================================================================================================
# stemgnn_glu_gemm_f32, stemgnn_split_weights_bf16, stemgnn_glu_gemm_bf16: C[M, N] = A[M, K] B[N, K]^T
# =====================================================================================================================
def _filled(t):
    buf = _Buf(t.numel())
    buf.t.copy_(t.reshape(-1).to(buf.t.device))
    return buf


def _glu_f32(A, B):
    _lib, lib = _libs()
    (M, K), N = A.shape, B.shape[0]
    a, b, c = _filled(A), _filled(B), _Buf(M * N)
    _lib.check(lib.stemgnn_glu_gemm_f32(a.ptr(), b.ptr(), c.ptr(), M, N, K, _stream()), "stemgnn_glu_gemm_f32")
    _sync()
    assert a.intact() and b.intact() and c.intact()
    assert _bits(a.t.cpu(), A.reshape(-1)) and _bits(b.t.cpu(), B.reshape(-1))
    return c.t.cpu().reshape(M, N)


def _split(B, s):
    """stemgnn_split_weights_bf16 into bf16-NaN-filled planes of exactly stemgnn_split_planes_floats: (the guarded buffer, the
    planes [s, N, Kp] as bf16 on the CPU); nothing behind the s * N * Kp numbers may have been written"""
    _lib, lib = _libs()
    N, K = B.shape
    Kp = (K + 31) // 32 * 32
    b = _filled(B)
    planes = _Buf(lib.stemgnn_split_planes_floats(N, K, s))
    planes.t.view(torch.int32).fill_(BF16_NAN_PAIR)
    assert 2 * planes.n >= s * N * Kp and _all_nan(planes.t.view(torch.bfloat16).float())
    _lib.check(lib.stemgnn_split_weights_bf16(b.ptr(), N, K, s, planes.ptr(), _stream()), "stemgnn_split_weights_bf16")
    _sync()
    assert b.intact() and planes.intact() and _bits(b.t.cpu(), B.reshape(-1))
    flat = planes.t.view(torch.bfloat16).cpu()
    assert _all_nan(flat[s * N * Kp:].float()), "written behind the planes"
    return planes, flat[: s * N * Kp].reshape(s, N, Kp)


def _glu_bf16(A, planes, N, s):
    _lib, lib = _libs()
    M, K = A.shape
    a, c = _filled(A), _Buf(M * N)
    p0 = planes.full.clone()
    _lib.check(lib.stemgnn_glu_gemm_bf16(a.ptr(), planes.ptr(), c.ptr(), M, N, K, s, _stream()), "stemgnn_glu_gemm_bf16")
    _sync()
    assert a.intact() and c.intact() and _bits(a.t.cpu(), A.reshape(-1))
    assert torch.equal(planes.full.view(torch.int32), p0.view(torch.int32))
    return c.t.cpu().reshape(M, N)


@pytest.mark.parametrize("M,N,K", GLU_CASES + GLU_CASES_F32)
def test_glu_gemms_integer_operands_give_the_fp64_product_bit_for_bit(M, N, K):
    """integers up to 8 are bf16 numbers: hi carries them, mid and lo are 0, so all three split counts are exact too"""
    g = _gen("glu", M, N, K)
    A, B = _ints(g, M, K), _ints(g, N, K)
    ref = A.double() @ B.double().T
    got = _glu_f32(A, B)
    assert _same_numbers(got, ref), f"fp32 entry: {_mismatch(got, ref)}"
    if K % 4:
        return                                                   # the bf16 entries refuse it (tests/test_gemm_cases.py)
    for s in (1, 2, 3):
        planes, _ = _split(B, s)
        got = _glu_bf16(A, planes, N, s)
        assert _same_numbers(got, ref), f"splits {s}: {_mismatch(got, ref)}"


@pytest.mark.parametrize("M,N,K", GLU_CASES + GLU_CASES_F32)
def test_glu_gemms_real_operands_stay_within_the_derived_bounds(M, N, K):
    g = _gen("glu real", M, N, K)
    A, B = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * 0.05
    ref, mag = A.double() @ B.double().T, A.double().abs() @ B.double().abs().T
    got = _glu_f32(A, B)
    err, bound = (got.double() - ref).abs(), gamma(2 * K + 2) * mag
    line = f"glu ({M}, {N}, {K}): worst |C - ref| / bound: fp32 {_worst(err, bound):.3f}"
    assert bool((err <= bound).all()), line
    Kp = (K + 31) // 32 * 32
    for s in (() if K % 4 else (1, 2, 3)):
        planes, _ = _split(B, s)
        got = _glu_bf16(A, planes, N, s)
        assert not torch.isnan(got).any(), s
        err, bound = (got.double() - ref).abs(), (SPLIT_TRUNC[s] + gamma(SPLIT_T[s] * Kp + 1)) * mag
        line += f" | bf16x{s} {_worst(err, bound):.3f}"
        assert bool((err <= bound).all()), line
    print(line)


@pytest.mark.parametrize("N,K", sorted({(n, k) for _, n, k in GLU_CASES}))
def test_split_planes_hold_the_weights(N, K):
    """read back as bf16: three planes sum to B exactly (in fp32 arithmetic), two to within 2^-16 |B|, one is B rounded to nearest
    even; the Kp - K padding columns are zero in every plane"""
    B = torch.randn(N, K, generator=_gen("planes", N, K)) * 0.05
    for s in (1, 2, 3):
        _, p = _split(B, s)
        assert not torch.isnan(p.float()).any(), f"splits {s}: unwritten numbers inside the planes"
        assert bool((p[:, :, K:].float() == 0).all()), f"splits {s}: padding not zero"
        p = p[:, :, :K].float()
        if s == 1:
            assert _bits(p[0], B.bfloat16().float())
        elif s == 2:
            d = ((p[0].double() + p[1].double()) - B.double()).abs()
            assert bool((d <= 2.0 ** -16 * B.double().abs()).all()), float((d / B.double().abs()).max())
        else:
            assert _bits((p[0] + p[1]) + p[2], B)


# =====================================================================================================================
# stemgnn_glu_combine_fwd / _bwd
# =====================================================================================================================
COMBINE_SHAPES = [(1, 1), (3, 65), (7, 64), (5, 200), (4100, 257)]        # the last: M * C > 4096 * 256, a second grid-stride trip
PLANTED = (88.0, -88.0, 0.0, -104.0, 104.0)         # gate arguments; expf(-104) = 0 and expf(104) = inf: gate exactly 1 and exactly 0


def _relerr(got, ref):
    den = float(ref.abs().max())
    num = float((got.double() - ref).abs().max())
    return num / den if den > 0 else num


def _spread(n, count):
    """`count` distinct positions over n elements (fewer where n is smaller)"""
    return sorted({(t * n) // count + (n // count) // 2 for t in range(count)} & set(range(n)))


def _run_fwd(U, V, bl, br, M, C):
    _lib, lib = _libs()
    ins = [_filled(t) for t in (U, V, bl, br)]
    outs = [_Buf(M * C) for _ in range(3)]
    _lib.check(lib.stemgnn_glu_combine_fwd(*[b.ptr() for b in ins + outs], M, C, _stream()), "stemgnn_glu_combine_fwd")
    _sync()
    assert all(b.intact() for b in ins + outs)
    assert all(_bits(b.t.cpu(), t) for b, t in zip(ins, (U, V, bl, br)))
    return [b.t.cpu() for b in outs]                             # out, gate, lin


@pytest.mark.parametrize("M,C", COMBINE_SHAPES)
def test_glu_combine_fwd(M, C):
    g, n = _gen("combine fwd", M, C), M * C
    U, V = torch.randn(n, generator=g), torch.rand(n, generator=g) * 60 - 30
    bl, br = torch.randn(C, generator=g) * 0.5, torch.randn(C, generator=g) * 0.5
    col = torch.arange(n) % C
    for pos, x in zip(_spread(n, len(PLANTED)), PLANTED[len(PLANTED) - min(n, len(PLANTED)):]):
        V[pos] = x - float(br[pos % C])
    x32 = V + br[col]
    u64, x64 = U.double() + bl.double()[col], V.double() + br.double()[col]
    ref = dict(out=u64 * torch.sigmoid(x64), gate=torch.sigmoid(x64), lin=u64)
    g32 = 1.0 / (1.0 + torch.exp(-x32))
    cpu32 = dict(out=(U + bl[col]) * g32, gate=g32, lin=U + bl[col])
    got = dict(zip(("out", "gate", "lin"), _run_fwd(U, V, bl, br, M, C)))
    line = f"combine fwd ({M}, {C}):"
    for k in ("out", "gate", "lin"):
        assert not torch.isnan(got[k]).any(), k
        e_k, e_ref = _relerr(got[k], ref[k]), _relerr(cpu32[k], ref[k])
        line += f" {k} {e_k:.2e} / {e_ref:.2e} = {e_k / max(e_ref, COMBINE_FLOOR):.2f}"
        assert e_k <= COMBINE_K * max(e_ref, COMBINE_FLOOR), line
    print(line)
    one, zero = x32 >= 80, x32 <= -100                           # 1 + expf(-80) rounds to 1, expf(100) is inf
    assert n < len(PLANTED) or (int(one.sum()) == 2 and int(zero.sum()) == 1)
    assert bool((got["gate"][one] == 1).all()) and _bits(got["out"][one], got["lin"][one])
    assert bool((got["gate"][zero] == 0).all()) and bool((got["out"][zero] == 0).all())
    assert bool((got["gate"] >= 0).all()) and bool((got["gate"] <= 1).all())
    # a NaN stays in its own element
    if n >= 2:
        iu, iv = _spread(n, 2)
        Un, Vn = U.clone(), V.clone()
        Un[iu], Vn[iv] = float("nan"), float("nan")
        out, gate, lin = _run_fwd(Un, Vn, bl, br, M, C)
        idx = torch.arange(n)
        assert torch.equal(torch.isnan(out), (idx == iu) | (idx == iv))
        assert torch.equal(torch.isnan(gate), idx == iv) and torch.equal(torch.isnan(lin), idx == iu)
        keep = ~torch.isnan(out)
        assert _bits(out[keep], got["out"][keep]) and _bits(gate[idx != iv], got["gate"][idx != iv])


def _run_bwd(dout, lin, gate, M, C):
    _lib, lib = _libs()
    ins = [_filled(t) for t in (dout, lin, gate)]
    outs = [_Buf(M * C) for _ in range(2)]
    _lib.check(lib.stemgnn_glu_combine_bwd(*[b.ptr() for b in ins + outs], M, C, _stream()), "stemgnn_glu_combine_bwd")
    _sync()
    assert all(b.intact() for b in ins + outs)
    assert all(_bits(b.t.cpu(), t) for b, t in zip(ins, (dout, lin, gate)))
    return [b.t.cpu() for b in outs]                             # dU, dV


@pytest.mark.parametrize("M,C", COMBINE_SHAPES)
def test_glu_combine_bwd(M, C):
    g, n = _gen("combine bwd", M, C), M * C
    dout, lin = torch.randn(n, generator=g), torch.randn(n, generator=g)
    gate = torch.sigmoid(torch.rand(n, generator=g) * 60 - 30)
    sat = _spread(n, 4)
    for pos, v in zip(sat, (1.0, 0.0, 1.0, 0.0)[4 - len(sat):]):
        gate[pos] = v
    d64, l64, g64 = dout.double(), lin.double(), gate.double()
    ref = dict(dU=d64 * g64, dV=d64 * l64 * g64 * (1 - g64))
    cpu32 = dict(dU=dout * gate, dV=dout * lin * gate * (1.0 - gate))
    got = dict(zip(("dU", "dV"), _run_bwd(dout, lin, gate, M, C)))
    line = f"combine bwd ({M}, {C}):"
    for k in ("dU", "dV"):
        assert not torch.isnan(got[k]).any(), k
        e_k, e_ref = _relerr(got[k], ref[k]), _relerr(cpu32[k], ref[k])
        line += f" {k} {e_k:.2e} / {e_ref:.2e} = {e_k / max(e_ref, COMBINE_FLOOR):.2f}"
        assert e_k <= COMBINE_K * max(e_ref, COMBINE_FLOOR), line
    print(line)
    one, zero = gate == 1, gate == 0
    assert _bits(got["dU"][one], dout[one]) and bool((got["dV"][one] == 0).all())
    assert bool((got["dU"][zero] == 0).all()) and bool((got["dV"][zero] == 0).all())
    if n >= 3:
        i_d, i_l, i_g = _spread(n, 3)
        dn, ln, gn = dout.clone(), lin.clone(), gate.clone()
        dn[i_d], ln[i_l], gn[i_g] = float("nan"), float("nan"), float("nan")
        dU, dV = _run_bwd(dn, ln, gn, M, C)
        idx = torch.arange(n)
        assert torch.equal(torch.isnan(dU), (idx == i_d) | (idx == i_g))
        assert torch.equal(torch.isnan(dV), (idx == i_d) | (idx == i_l) | (idx == i_g))
        assert _bits(dU[~torch.isnan(dU)], got["dU"][~torch.isnan(dU)]) and _bits(dV[~torch.isnan(dV)], got["dV"][~torch.isnan(dV)])


# =====================================================================================================================
# stemgnn_colsum
# =====================================================================================================================
def _colsum(X):
    _lib, lib = _libs()
    M, C = X.shape
    x, out = _filled(X), _Buf(C)
    _lib.check(lib.stemgnn_colsum(x.ptr(), M, C, out.ptr(), _stream()), "stemgnn_colsum")
    _sync()
    assert x.intact() and out.intact() and _bits(x.t.cpu(), X.reshape(-1))
    return out.t.cpu()


@pytest.mark.parametrize("C", (1, 63, 64, 65, 200))
@pytest.mark.parametrize("M", (1, 2, 3, 4, 5, 1000))
def test_colsum(M, C):
    g = _gen("colsum", M, C)
    X = _ints(g, M, C)
    got = _colsum(X)
    assert _same_numbers(got, X.double().sum(0)), _mismatch(got, X.double().sum(0))
    X = torch.randn(M, C, generator=g)
    got, again = _colsum(X), _colsum(X)
    assert not torch.isnan(got).any() and _bits(got, again)
    err, bound = (got.double() - X.double().sum(0)).abs(), gamma(M) * X.double().abs().sum(0)
    print(f"colsum ({M}, {C}): worst |out - ref| / bound {_worst(err, bound):.3f}")
    assert bool((err <= bound).all()), _worst(err, bound)
