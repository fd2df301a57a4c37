"""CPU: the case table of tests/test_hip_gemm.py (the GEMM entries of csrc/splitgemm.hip), and proof that it reaches what it claims.

stemgnn_sgemm_f32 runs one of four instantiations of sg_gemm2 (csrc/gemm2.h) by operand orientation (A k-contiguous or not, B
k-contiguous or not), each with a vector loader pair (16-byte loads) or a scalar, fully predicated pair; g2_launch picks the pair
from pointer alignment, ld % 4, K % 4, M % 4 and N % 4.  stemgnn_sgemm_paths asks the launch's own plan (g2_plan), host only, so
this file can prove on the CPU which loaders and which tile order every case of the table takes -- a condition that moves fails here
instead of silently dropping a path from the GPU suite.  Nothing is launched and no pointer is dereferenced.

The table is built from the tile constants of the instantiations stemgnn_sgemm_f32 launches -- BM = 64 rows, BN = 128 columns,
BK = 16 per LDS stage, MFMA k-step 2 -- and kept to the smallest sizes that reach each class: M one below / at / one above a tile
and at the vector width, N likewise, K below an MFMA step, below / at / above the float4 width, one below / at / one above a stage,
and three stages with a ragged last one (36 = 2 * 16 + 4, 52 = 3 * 16 + 4).  Cases with nx >= 8 row tiles use K <= 8."""
import ctypes
import os
from collections import namedtuple

import pytest

from tests.test_graph_abi import header_signature

BM, BN, BK, KSTEP = 64, 128, 16, 2
M_SIZES = {1, 3, 4, 63, 64, 65, 132, 512, 516}
N_SIZES = {1, 4, 127, 128, 129, 260}
K_SIZES = {1, 2, 3, 4, 15, 16, 17, 36, 52}
ORIENTATIONS = [(1, 1), (1, 0), (0, 1), (0, 0)]
EINVAL = -10001
ENTRIES = ["stemgnn_sgemm_f32", "stemgnn_glu_gemm_f32", "stemgnn_split_weights_bf16", "stemgnn_glu_gemm_bf16",
           "stemgnn_glu_combine_fwd", "stemgnn_glu_combine_bwd", "stemgnn_colsum", "stemgnn_sgemm_paths"]


class GemmCase(namedtuple("GemmCase", "akc bkc M N K dlda dldb offA offB dldc")):
    """One call of stemgnn_sgemm_f32: orientation, sizes, leading dimensions as natural + d (d in 0, 4, 1; ldc = N + 0 or 3),
    base pointers one float (offA / offB = 1) into a 16-byte aligned allocation or at its start."""
    __slots__ = ()

    @property
    def lda(self):
        return (self.K if self.akc else self.M) + self.dlda

    @property
    def ldb(self):
        return (self.K if self.bkc else self.N) + self.dldb

    @property
    def ldc(self):
        return self.N + self.dldc

    @property
    def a_floats(self):
        """footprint of A behind its base pointer: (rows - 1) * ld + extent"""
        rows, extent = (self.M, self.K) if self.akc else (self.K, self.M)
        return (rows - 1) * self.lda + extent

    @property
    def b_floats(self):
        rows, extent = (self.N, self.K) if self.bkc else (self.K, self.N)
        return (rows - 1) * self.ldb + extent

    @property
    def c_floats(self):
        return (self.M - 1) * self.ldc + self.N

    @property
    def nx(self):
        return -(-self.M // BM)

    @property
    def ny(self):
        return -(-self.N // BN)

    @property
    def scalar_reasons(self):
        """why g2_launch takes the scalar loaders (empty: the vector loaders); only the reasons that apply to the orientation"""
        r = set()
        if self.offA:
            r.add("A base")
        if self.offB:
            r.add("B base")
        if self.lda % 4:
            r.add("lda % 4")
        if self.ldb % 4:
            r.add("ldb % 4")
        if (self.akc or self.bkc) and self.K % 4:
            r.add("K % 4")
        if not self.akc and self.M % 4:
            r.add("M % 4")
        if not self.bkc and self.N % 4:
            r.add("N % 4")
        return r

    @property
    def vec(self):
        return not self.scalar_reasons

    @property
    def id(self):
        s = f"a{self.akc}b{self.bkc}-{self.M}x{self.N}x{self.K}"
        for tag, v in (("lda+", self.dlda), ("ldb+", self.dldb), ("ldc+", self.dldc)):
            if v:
                s += f"-{tag}{v}"
        return s + ("-offA" if self.offA else "") + ("-offB" if self.offB else "")


def applicable_reasons(akc, bkc):
    r = {"A base", "B base", "lda % 4", "ldb % 4"}
    if akc or bkc:
        r.add("K % 4")
    if not akc:
        r.add("M % 4")
    if not bkc:
        r.add("N % 4")
    return r


def _c(M, N, K, dlda=0, dldb=0, offA=0, offB=0, dldc=0):
    return (M, N, K, dlda, dldb, offA, offB, dldc)


# per orientation: vector-path cases first, then one case per reason for the scalar path with that reason alone (a leading
# dimension of natural + 1 brings a ragged extent back to a multiple of 4), then crossings
_TABLE = {
    (1, 1): [   # A[i*lda+k], B[j*ldb+k]: vector needs K % 4 == 0
        _c(64, 128, 16), _c(65, 129, 36, dlda=4, dldb=4, dldc=3), _c(1, 1, 4), _c(132, 260, 52, dldb=4),
        _c(516, 260, 4, dldc=3), _c(512, 4, 4),
        _c(63, 127, 16, offA=1), _c(64, 128, 16, offB=1, dldc=3), _c(4, 4, 16, dlda=1), _c(3, 129, 4, dldb=1),
        _c(65, 4, 15, dlda=1, dldb=1),
        _c(64, 127, 17), _c(1, 1, 1), _c(3, 4, 2), _c(4, 1, 3, dldc=3), _c(63, 129, 52, offA=1), _c(512, 1, 3),
    ],
    (1, 0): [   # A[i*lda+k], B[k*ldb+j]: vector needs K % 4 == 0 and N % 4 == 0
        _c(64, 128, 16), _c(65, 260, 36, dlda=4, dldb=4, dldc=3), _c(1, 4, 4), _c(132, 128, 52), _c(3, 4, 4, dldc=3),
        _c(512, 4, 4),
        _c(63, 128, 16, offA=1), _c(64, 128, 16, offB=1, dldc=3), _c(4, 4, 16, dlda=1), _c(3, 128, 4, dldb=1),
        _c(65, 4, 15, dlda=1), _c(64, 127, 16, dldb=1),
        _c(64, 129, 17), _c(1, 1, 1), _c(4, 1, 2, dldc=3), _c(63, 129, 52), _c(516, 260, 3),
    ],
    (0, 1): [   # A[k*lda+i], B[j*ldb+k]: vector needs K % 4 == 0 and M % 4 == 0
        _c(64, 128, 16), _c(132, 129, 36, dlda=4, dldb=4, dldc=3), _c(4, 1, 4), _c(64, 260, 52), _c(516, 260, 4),
        _c(512, 4, 4, dldc=3),
        _c(64, 127, 16, offA=1), _c(64, 128, 16, offB=1, dldc=3), _c(4, 4, 16, dlda=1), _c(4, 129, 4, dldb=1),
        _c(4, 4, 15, dldb=1), _c(63, 128, 16, dlda=1),
        _c(65, 129, 17), _c(1, 1, 1), _c(3, 4, 2, dldc=3), _c(65, 127, 52), _c(516, 260, 2, offB=1), _c(512, 1, 3),
    ],
    (0, 0): [   # A[k*lda+i], B[k*ldb+j]: vector needs M % 4 == 0 and N % 4 == 0, whatever K
        _c(64, 128, 16), _c(132, 260, 36, dlda=4, dldb=4, dldc=3), _c(4, 4, 1), _c(64, 128, 17), _c(4, 128, 15, dldc=3),
        _c(64, 260, 52), _c(516, 260, 3), _c(512, 4, 1),
        _c(64, 128, 16, offA=1), _c(64, 128, 16, offB=1, dldc=3), _c(4, 4, 16, dlda=1), _c(4, 4, 4, dldb=1),
        _c(63, 128, 16, dlda=1), _c(64, 127, 16, dldb=1),
        _c(65, 129, 17), _c(1, 1, 1), _c(3, 1, 2, dldc=3), _c(63, 129, 52), _c(516, 260, 4, offA=1), _c(512, 1, 2),
    ],
}
GEMM_CASES = [GemmCase(akc, bkc, *row) for (akc, bkc) in ORIENTATIONS for row in _TABLE[(akc, bkc)]]


def _of(akc, bkc, vec=None):
    return [c for c in GEMM_CASES if (c.akc, c.bkc) == (akc, bkc) and (vec is None or c.vec == vec)]


def real_cases():
    """cases that also run with real-valued operands: per orientation and loader path the (first) one with the largest K, and every
    case with nx = 9, ny = 3"""
    out = []
    for akc, bkc in ORIENTATIONS:
        for vec in (True, False):
            cs = _of(akc, bkc, vec)
            out.append(max(cs, key=lambda c: c.K))          # max keeps the first of equals
    out += [c for c in GEMM_CASES if (c.nx, c.ny) == (9, 3) and c not in out]
    return out


def nan_cases():
    """cases of the planted-NaN test: per orientation the first vector and the first scalar case with a ragged last tile and at
    least one LDS stage of K"""
    out = []
    for akc, bkc in ORIENTATIONS:
        for vec in (True, False):
            out.append(next(c for c in _of(akc, bkc, vec) if c.M >= 63 and c.N >= 127 and (c.M % BM or c.N % BN) and c.K >= 16))
    return out


# ---- the GLU-shaped entries: C[M,N] = A[M,K] B[N,K]^T; K = 4 one ragged stage of the bf16 kernel (32 per stage), 32 no padding,
# 36 / 68 a padded last stage; 3 and 17 (fp32 entry only: the bf16 entries need K % 4 == 0) take the scalar loaders
GLU_M, GLU_N, GLU_K, GLU_K_F32 = {1, 63, 64, 65, 130}, {1, 127, 128, 129, 260}, {4, 28, 32, 36, 68}, {3, 17}
GLU_CASES = [(1, 1, 4), (63, 127, 28), (64, 128, 32), (65, 129, 36), (130, 260, 68), (1, 260, 32), (130, 1, 4), (64, 127, 36),
             (65, 128, 28)]
GLU_CASES_F32 = [(65, 129, 3), (63, 1, 17), (1, 128, 17), (130, 127, 3)]


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__

        __graft_entry__.build()
    return _lib.load()


BASE_A, BASE_B = 1 << 20, 1 << 21           # 16-byte aligned pointer values; nothing dereferences them


def query(lib, c, A=None, B=None):
    """stemgnn_sgemm_paths of a case as (vec, nx, ny, blocks); A / B default to the stand-in pointers"""
    out = (ctypes.c_int * 4)()
    A = BASE_A + 4 * c.offA if A is None else A
    B = BASE_B + 4 * c.offB if B is None else B
    rc = lib.stemgnn_sgemm_paths(A, c.lda, c.akc, B, c.ldb, c.bkc, c.M, c.N, c.K, out)
    assert rc == 0, (c, rc)
    return bool(out[0]), out[1], out[2], out[3]


def test_sizes_come_from_the_tile_constants():
    assert M_SIZES == {1, 3, 4, BM - 1, BM, BM + 1, 2 * BM + 4, 8 * BM, 8 * BM + 4}
    assert N_SIZES == {1, 4, BN - 1, BN, BN + 1, 2 * BN + 4}
    assert K_SIZES == {1, KSTEP, 3, 4, BK - 1, BK, BK + 1, 2 * BK + 4, 3 * BK + 4}
    assert {c.M for c in GEMM_CASES} == M_SIZES
    assert {c.N for c in GEMM_CASES} == N_SIZES
    assert {c.K for c in GEMM_CASES} == K_SIZES
    assert {c.dlda for c in GEMM_CASES} == {0, 4, 1} == {c.dldb for c in GEMM_CASES}
    assert {c.dldc for c in GEMM_CASES} == {0, 3}
    assert len({c.id for c in GEMM_CASES}) == len(GEMM_CASES)
    for o in ORIENTATIONS:
        assert 12 <= len(_of(*o)) <= 20, (o, len(_of(*o)))
        assert {c.dldc for c in _of(*o)} == {0, 3}
        assert {c.dlda for c in _of(*o)} == {0, 4, 1} == {c.dldb for c in _of(*o)}, o
    for c in GEMM_CASES:
        assert c.K <= 64                                             # integer operands from [-8, 8] sum exactly in fp32
        assert c.nx < 8 or c.K <= 8, c


def test_the_launch_plan_is_what_the_table_says(lib):
    for c in GEMM_CASES:
        vec, nx, ny, blocks = query(lib, c)
        assert vec == c.vec, (c, c.scalar_reasons)
        assert (nx, ny) == (c.nx, c.ny), c
        assert blocks == 8 * -(-nx // 8) * ny, c                     # whole rounds of the 8 XCDs


def test_each_orientation_has_both_loader_paths_and_every_scalar_reason(lib):
    for o in ORIENTATIONS:
        assert len(_of(*o, vec=True)) >= 3 and len(_of(*o, vec=False)) >= 3, o
        alone = {next(iter(c.scalar_reasons)) for c in _of(*o) if len(c.scalar_reasons) == 1}
        assert alone == applicable_reasons(*o), (o, applicable_reasons(*o) - alone)
        # each of those cases is one change away from the vector path: the reason is what the launch reads
        for c in _of(*o):
            if len(c.scalar_reasons) == 1:
                assert not query(lib, c)[0]
                if c.offA or c.offB:
                    assert query(lib, c, A=BASE_A, B=BASE_B)[0], c
                elif "lda % 4" in c.scalar_reasons or "ldb % 4" in c.scalar_reasons:
                    up = c._replace(dlda=c.dlda + (-c.lda) % 4, dldb=c.dldb + (-c.ldb) % 4)
                    assert query(lib, up)[0], c
    assert any(c.vec and c.K % 2 for c in _of(0, 0))                 # no K rule where neither operand is k-contiguous
    assert any(len(c.scalar_reasons) > 1 for c in GEMM_CASES)


def test_tile_counts_wrap_the_xcd_grouping():
    assert {1, 8, 9} <= {c.nx for c in GEMM_CASES}
    assert {1, 3} <= {c.ny for c in GEMM_CASES}
    wrap = [c for c in GEMM_CASES if (c.nx, c.ny) == (9, 3)]
    assert wrap and {c.vec for c in wrap} == {True, False}
    assert {(c.akc, c.bkc) for c in wrap} == set(ORIENTATIONS)
    for o in ORIENTATIONS:
        assert any(c.nx >= 8 for c in _of(*o)), o


def test_real_and_nan_selections():
    real = real_cases()
    for o in ORIENTATIONS:
        for vec in (True, False):
            got = [c for c in real if (c.akc, c.bkc) == o and c.vec == vec]
            assert got and max(c.K for c in got) == max(c.K for c in _of(*o, vec=vec)) == 52, (o, vec)
    assert all(c in real for c in GEMM_CASES if (c.nx, c.ny) == (9, 3))
    nan = nan_cases()
    assert len(nan) == 8 and {(c.akc, c.bkc, c.vec) for c in nan} == {(a, b, v) for a, b in ORIENTATIONS for v in (True, False)}
    for c in nan:
        assert c.M % BM or c.N % BN                                  # the last tile is ragged


def test_glu_shapes():
    assert {m for m, _, _ in GLU_CASES} == GLU_M and {n for _, n, _ in GLU_CASES} == GLU_N
    assert {k for _, _, k in GLU_CASES} == GLU_K and {k for _, _, k in GLU_CASES_F32} == GLU_K_F32
    assert all(k % 4 == 0 and k <= 68 for _, _, k in GLU_CASES)
    assert GLU_M == {1, BM - 1, BM, BM + 1, 2 * BM + 2} and GLU_N == {1, BN - 1, BN, BN + 1, 2 * BN + 4}


def test_sgemm_refusals(lib):
    p, out = 4096, (ctypes.c_int * 4)()

    def sgemm(A=p, lda=16, akc=1, B=p, ldb=16, bkc=1, C=p, ldc=8, M=8, N=8, K=16, acc=0):
        return lib.stemgnn_sgemm_f32(A, lda, akc, B, ldb, bkc, C, ldc, M, N, K, acc, None)

    def paths(A=p, lda=16, akc=1, B=p, ldb=16, bkc=1, M=8, N=8, K=16, o=out):
        return lib.stemgnn_sgemm_paths(A, lda, akc, B, ldb, bkc, M, N, K, o)

    assert paths() == 0
    for f in (sgemm, paths):
        for kw in (dict(A=None), dict(B=None), dict(M=0), dict(N=-1), dict(K=0), dict(lda=0), dict(ldb=-4),
                   dict(lda=15), dict(ldb=15),                                  # k-contiguous: below K
                   dict(akc=0, lda=7), dict(bkc=0, ldb=7),                      # not k-contiguous: below M / N
                   dict(akc=0, M=17, lda=16)):                                  # ... where K would have passed
            assert f(**kw) == EINVAL, (f.__name__, kw)
    assert sgemm(bkc=0, N=17, ldb=16, ldc=17) == EINVAL and paths(bkc=0, N=17, ldb=16) == EINVAL
    assert sgemm(C=None) == EINVAL and sgemm(ldc=7) == EINVAL
    assert paths(o=None) == EINVAL
    # the minima themselves pass the check (the query launches nothing)
    assert paths(lda=16, ldb=16) == 0 and paths(akc=0, lda=8, bkc=0, ldb=8) == 0


def test_glu_and_elementwise_refusals(lib):
    p = 4096
    assert lib.stemgnn_glu_gemm_f32(None, p, p, 8, 8, 8, None) == EINVAL
    assert lib.stemgnn_glu_gemm_f32(p, None, p, 8, 8, 8, None) == EINVAL
    assert lib.stemgnn_glu_gemm_f32(p, p, None, 8, 8, 8, None) == EINVAL
    for dims3 in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (-1, 8, 8)):
        assert lib.stemgnn_glu_gemm_f32(p, p, p, *dims3, None) == EINVAL
        assert lib.stemgnn_glu_gemm_bf16(p, p, p, *dims3, 2, None) == EINVAL
    for hole in range(3):
        args = [p, p, p]
        args[hole] = None
        assert lib.stemgnn_glu_gemm_bf16(*args, 8, 8, 8, 2, None) == EINVAL
    for K in (1, 2, 3, 5, 6, 7, 30):
        assert lib.stemgnn_glu_gemm_bf16(p, p, p, 8, 8, K, 2, None) == EINVAL, K
    for off in (4, 8, 12):
        assert lib.stemgnn_glu_gemm_bf16(p + off, p, p, 8, 8, 8, 2, None) == EINVAL          # misaligned A
        assert lib.stemgnn_glu_gemm_bf16(p, p + off, p, 8, 8, 8, 2, None) == EINVAL          # misaligned planes
        assert lib.stemgnn_split_weights_bf16(p, 8, 8, 2, p + off, None) == EINVAL
    for s in (0, 4, -1):
        assert lib.stemgnn_glu_gemm_bf16(p, p, p, 8, 8, 8, s, None) == EINVAL
        assert lib.stemgnn_split_weights_bf16(p, 8, 8, s, p, None) == EINVAL
    assert lib.stemgnn_split_weights_bf16(None, 8, 8, 2, p, None) == EINVAL
    assert lib.stemgnn_split_weights_bf16(p, 8, 8, 2, None, None) == EINVAL
    assert lib.stemgnn_split_weights_bf16(p, 0, 8, 2, p, None) == EINVAL
    assert lib.stemgnn_split_weights_bf16(p, 8, 0, 2, p, None) == EINVAL
    for hole in range(7):
        args = [p] * 7
        args[hole] = None
        assert lib.stemgnn_glu_combine_fwd(*args, 4, 4, None) == EINVAL
    for hole in range(5):
        args = [p] * 5
        args[hole] = None
        assert lib.stemgnn_glu_combine_bwd(*args, 4, 4, None) == EINVAL
    for M, C in ((0, 4), (4, 0), (-2, 4)):
        assert lib.stemgnn_glu_combine_fwd(*[p] * 7, M, C, None) == EINVAL
        assert lib.stemgnn_glu_combine_bwd(*[p] * 5, M, C, None) == EINVAL
        assert lib.stemgnn_colsum(p, M, C, p, None) == EINVAL
    assert lib.stemgnn_colsum(None, 4, 4, p, None) == EINVAL
    assert lib.stemgnn_colsum(p, 4, 4, None, None) == EINVAL


def test_plane_sizes(lib):
    """stemgnn_split_planes_floats holds splits * N * Kp bf16 numbers, Kp = K rounded up to 32 (the GPU suite views the planes so)"""
    for N, K, s in ((1, 4, 1), (127, 28, 3), (129, 36, 2), (260, 68, 3), (1, 1, 1)):
        Kp = (K + 31) // 32 * 32
        assert 2 * lib.stemgnn_split_planes_floats(N, K, s) >= s * N * Kp
        assert lib.stemgnn_split_planes_floats(N, K, s) == (s * N * Kp + 1) // 2 + 8


@pytest.mark.parametrize("name", ENTRIES)
def test_symbol_has_the_headers_signature(lib, name):
    from stemgnn_amd import _lib

    assert hasattr(lib, name)
    assert _lib.SIGNATURES[name] == header_signature(name)
