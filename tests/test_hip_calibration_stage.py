"""GPU: the batch side of the conformal family -- stemgnn_conformal_fit / _apply (stemgnn_amd/csrc/conformal.hip), stemgnn_seasonal_fit /
_apply and stemgnn_quantile_store_seasonal (csrc/seasonal.hip), stemgnn_quantile_finish / _store (csrc/quantile_serve.hip), with the fit
and the column kernel they share (csrc/conformal_fit.h, csrc/quantile_column.h) -- through the C ABI on NaN-filled, guarded buffers, at
the widths and window counts at which their launchers take another decision: the counterpart of tests/test_hip_serving_stage.py.

Cases, inputs and references are in tests/test_calibration_cases.py (the case table is in its docstring), which proves on the CPU,
through stemgnn_calibration_plan, that the cases reach every form, tile count, tile width, chunk bound, row trip, walk, VEC, cap,
thread count, plane count, workgroup shape, column block and window trip of the launchers, and that every further chunk, trip, tile,
block and window trip changes the expected outputs.  That proof ran with the 256 compute units the plan falls back on without a
device; this module asks the plan again on the device when it is imported and every test fails if a class is no longer reached.
The references are tests/helpers/conformal_ref.py, tests/helpers/seasonal_ref.py, a stable numpy sort (-0 == +0, NaN last) and the
stemgnn_forecast_store contract for the slab rows; none is code under test.

Hygiene, for every call: every input and output is a guarded copy (tests/util._Buf and its kin: sentinels behind the payload, and in
front of it where the buffer sits at a 4-byte offset); offsets and an out-of-place `out` are NaN, counts a junk integer, the fit's
scratch 0xFF and the result slabs of a store a recognisable fill before the call; afterwards every guard is unchanged, every input
has its bits (in place: the rows in no pair, where nothing is rearranged), and the WHOLE of every output buffer is compared with the
reference, so slab rows outside [pos, pos + B) and [0, capacity) must hold the fill.  Every case runs twice and both runs must agree
bit for bit; a case with a buffer at a 4-byte offset must agree bit for bit with its aligned twin; a seasonal fit whose consecutive
origins are handed over as a tensor (the skipping walk) must agree bit for bit with the DIRECT run of the same rows.

No tolerance anywhere: offsets are k-th smallest fp32 values, compared as numbers (inf == inf, -0 == +0) and never NaN; counts are
integers; applied and rearranged rows are bit patterns, except that a NaN the operation itself makes only has to be a NaN.

Findings: none.  Every case agrees with its reference on the first run and no guard was touched: the second and third window trips
of the column kernel, its second column block (of one column, of one float4, ragged), the capped grids of both applies with their
second trips, 24 chunks of 22 tiles and 64 stream chunks of the fit, and the DIRECT walk with runs = 2 hold the same contract as the
toy shapes of the semantic suites."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import test_calibration_cases as S
from tests.test_hip_serving_stage import G, _ok, _ptr

pytestmark = pytest.mark.gpu
F32 = np.float32
JUNK_I = -0x0BADC0DE
NAN = F32(np.nan)


def _unreached():
    """the classes of the CPU proof that no case reaches with THIS device's compute units (None: the library is not built yet)"""
    from stemgnn_amd import _lib

    if not os.path.isfile(_lib.LIB_PATH):
        return None
    return [k for k in S.CLASSES if not S.reached(k)]


UNREACHED = _unreached()


@pytest.fixture(scope="module")
def lib():
    from stemgnn_amd import _lib

    return _lib.load()


@pytest.fixture(autouse=True)
def every_class_is_reached_on_this_device(lib):
    missing = _unreached() if UNREACHED is None else UNREACHED
    assert not missing, f"with {lib.stemgnn_num_cus()} compute units no case reaches {missing}"


def test_classes_are_reached_on_the_device(lib):
    assert lib.stemgnn_num_cus() == S.plan("fit", S.FIT_CASES[0])["cus"] and torch.cuda.is_available()


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def _pair_args(pairs):
    return _ints([p[0] for p in pairs]), _ints([p[1] for p in pairs])


def _twice(run, c, twin=None):
    """twice from the same inputs; a misaligned case (or a seasonal fit with its origins as a tensor) also against its twin"""
    first, second = run(c), run(c)
    for other in ([second] + ([run(twin)] if twin is not None else [])):
        assert len(first) == len(other) > 0
        for i, (a, b) in enumerate(zip(first, other)):
            assert S.same_bits(a, b), f"{c}: buffer {i} differs between two runs"


# ---- fit ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.FIT_CASES + S.SFIT_CASES, ids=str)
def test_fit(lib, c):
    seasonal = isinstance(c, S.SFit)
    y, f = S.fit_data(c)
    pairs, cov = S.pairs_of(c.P, c.Q), S.coverages(c.P)
    lo, hi = _pair_args(pairs)
    covs = (ctypes.c_double * c.P)(*cov)
    Hg, Ng = (c.H if c.per_step else 1), (c.N if c.per_node else 1)
    shape = ((c.K,) if seasonal else ()) + (c.P, Hg, Ng)
    if seasonal:
        nbytes = lib.stemgnn_seasonal_scratch_bytes(c.count, c.H, c.N, c.P, c.K, c.per_step, c.per_node)
    else:
        nbytes = lib.stemgnn_conformal_scratch_bytes(c.count, c.H, c.N, c.P, c.per_step, c.per_node)
    assert nbytes == int(np.prod(shape)) * 258 * 4

    for masked in (0, 1):
        want_off, want_cnt = S.fit_ref(c, bool(masked))
        assert want_off.shape == shape and not np.isnan(want_off).any()

        def run(c):
            yb, fb = G(y), G(f)
            scratch = G(np.full(nbytes // 4, -1, dtype=np.int32))       # 0xFF in every byte
            off, cnt = G(np.full(shape, NAN, dtype=F32)), G(np.full(shape, JUNK_I, dtype=np.int64))
            origins = G(S.sfit_origins(c)) if seasonal and isinstance(c.origin, str) else None
            if seasonal:
                _ok(lib.stemgnn_seasonal_fit(yb.ptr, fb.ptr, _ptr(origins), 0 if origins is not None else c.origin, c.count, c.Q, c.H,
                                             c.N, c.P, lo, hi, covs, c.per_step, c.per_node, masked, c.period, c.K, c.phase,
                                             scratch.ptr, off.ptr, cnt.ptr, None))
            else:
                _ok(lib.stemgnn_conformal_fit(yb.ptr, fb.ptr, c.count, c.Q, c.H, c.N, c.P, lo, hi, covs, c.per_step, c.per_node,
                                              masked, scratch.ptr, off.ptr, cnt.ptr, None))
            got_off, got_cnt = off.read("offsets"), cnt.read("counts")
            scratch.read("scratch")
            yb.unchanged("target"), fb.unchanged("forecast")
            if origins is not None:
                origins.unchanged("origins")
            assert np.array_equal(got_cnt, want_cnt), (c, masked, np.flatnonzero((got_cnt != want_cnt).reshape(-1))[:5].tolist())
            assert not np.isnan(got_off).any(), (c, masked)
            bad = np.flatnonzero((got_off != want_off).reshape(-1))
            assert bad.size == 0, (c, masked, bad[:5].tolist(), got_off.reshape(-1)[bad[:5]].tolist(), want_off.reshape(-1)[bad[:5]].tolist())
            return [got_off, got_cnt]
        _twice(run, c, S.sfit_twin(c) if seasonal and c.origin == "consecutive" else None)


# ---- the streaming applies ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.APPLY_CASES + S.SAPPLY_CASES, ids=str)
def test_apply(lib, c):
    seasonal = isinstance(c, S.SApply)
    f, offsets = S.apply_data(c)
    want = S.apply_ref(c)
    paired = (0, c.Q - 1)
    lo, hi = _pair_args((paired,))
    assert np.isnan(want).any() and np.isinf(want).any()

    def run(c):
        fb = G(f, off=c.mis & 1)
        ob = fb if c.in_place else G(np.full(f.shape, NAN, dtype=F32), off=(c.mis >> 1) & 1)
        offb = G(offsets)
        origins = G(S.origins_of(c)) if seasonal and c.origin == "scattered" else None
        if seasonal:
            period, K, phase = S.SEASON
            _ok(lib.stemgnn_seasonal_apply(fb.ptr, offb.ptr, _ptr(origins), 0 if origins is not None else c.origin, c.count, c.Q, c.H,
                                           c.N, 0, 1, lo, hi, 1, 1, period, K, phase, ob.ptr, None))
        else:
            _ok(lib.stemgnn_conformal_apply(fb.ptr, offb.ptr, c.count, c.Q, c.H, c.N, 1, lo, hi, 1, 1, ob.ptr, None))
        got = ob.read("out")
        assert S.same_rows(got, want, f, paired), _first_difference(c, got, want)
        offb.unchanged("offsets")
        if not c.in_place:
            fb.unchanged("forecast")
        if origins is not None:
            origins.unchanged("origins")
        return [got]
    _twice(run, c, c._replace(mis=0) if c.mis else None)


def _first_difference(c, got, want):
    bad = np.flatnonzero(~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).reshape(-1))
    return f"{c}: {bad.size} of {got.size} differ, first at {bad[:5].tolist()}: {got.reshape(-1)[bad[:5]].tolist()} != {want.reshape(-1)[bad[:5]].tolist()}"


# ---- the column kernel, by each of its callers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", S.COLUMN_CASES, ids=str)
def test_column(lib, c):
    x, offsets, target = S.column_data(c)
    rows, ordered = S.column_ref(c)
    paired = (0, c.Q - 1)
    lo, hi = _pair_args((paired,))
    period, K, phase = S.SEASON
    store = S._is_store(c)
    if c.rearrange:
        assert (ordered.view(np.uint32) != x.view(np.uint32)).any(axis=1).mean() >= 0.5
    if store:
        want, want_t = S.store_ref(c, rows)
        kept, _ = S.store_ref(c, ordered)
        inside = [r for r in range(c.capacity) if 0 <= r - c.pos < c.count]
        assert 0 < len(inside) and (len(inside) < c.count) == (c.pos < 0 or c.pos + c.count > c.capacity)

    def run(c):
        src, offb = G(x, off=c.mis & 1), G(offsets)
        if not store:
            in_place = c.caller == "finish_in_place"
            dst = src if in_place else G(np.full(x.shape, NAN, dtype=F32), off=(c.mis >> 1) & 1)
            if c.caller == "seasonal_apply":
                _ok(lib.stemgnn_seasonal_apply(src.ptr, offb.ptr, None, int(S.origins_of(c)[0]), c.count, c.Q, c.H, c.N, c.rearrange, 1, lo, hi,
                                               1, 0, period, K, phase, dst.ptr, None))
            else:
                _ok(lib.stemgnn_quantile_finish(src.ptr, c.count, c.Q, c.H, c.N, c.rearrange, offb.ptr, 1, lo, hi, 1, 0, dst.ptr, None))
            got = dst.read("out")
            assert S.same_rows(got, rows, ordered, paired), _first_difference(c, got, rows)
            if not in_place:
                src.unchanged("forecast")
            offb.unchanged("offsets")
            return [got]
        tgt = G(target, off=(c.mis >> 2) & 1)
        slab = G(np.full(want.shape, S.FILL, dtype=F32), off=(c.mis >> 1) & 1)
        tslab = G(np.full(want_t.shape, S.FILL, dtype=F32), off=(c.mis >> 3) & 1)
        pos = G(np.array([c.pos], dtype=np.int64))
        if c.caller == "seasonal_store":
            t_dev = G(np.array([S.T0], dtype=np.int64))
            _ok(lib.stemgnn_quantile_store_seasonal(src.ptr, tgt.ptr, pos.ptr, t_dev.ptr, c.count, c.Q, c.H, c.N, c.rearrange, offb.ptr, 1,
                                                    lo, hi, 1, 0, period, K, phase, slab.ptr, tslab.ptr, c.capacity, None))
            t_dev.unchanged("t_dev")
        else:
            _ok(lib.stemgnn_quantile_store(src.ptr, tgt.ptr, pos.ptr, c.count, c.Q, c.H, c.N, c.rearrange, offb.ptr, 1, lo, hi, 1, 0,
                                           slab.ptr, tslab.ptr, c.capacity, None))
        got, got_t = slab.read("out_forecast"), tslab.read("out_target")
        assert S.same_rows(got, want, kept, paired), _first_difference(c, got, want)
        assert S.same_bits(got_t, want_t), f"{c}: out_target"
        outside = [r for r in range(c.capacity) if r not in inside]
        assert (got[outside] == S.FILL).all() and (got_t[outside] == S.FILL).all()
        src.unchanged("steps"), tgt.unchanged("target"), pos.unchanged("pos"), offb.unchanged("offsets")
        return [got, got_t]
    _twice(run, c, c._replace(mis=0) if c.mis else None)
