"""CPU: (1) tests/helpers/philox_ref.py, the host model of the attention dropout map, is Philox4x32-10 (Random123's known-answer
vectors) and maps element (b, i, j) to word (j >> 6) & 3 of counter (b N + i) NQ + (j >> 8) 64 + (j & 63); (2) the literal case
lists of tests/test_hip_front.py reach both sides of every decision csrc/front.hip takes by shape.  A trimmed list fails here,
on a machine without a GPU, naming what was lost -- and test_a_trimmed_list_fails proves that of this file's own check."""
import numpy as np
import pytest

from tests.helpers import philox_ref
from tests.test_hip_front import (BS, CHEB_GENERIC_N, CHEB_NS, FRONT_CASES, MASK_NS, MASK_PS, MASK_SEEDS, NCHUNK_CASES, NCHUNKS,
                                  NS)

# Random123 kat_vectors, philox4x32 10 rounds: counter; key; result
KAT = [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
]
# what the stage-level net was asked to cover
WANT_NS = {1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 127, 129, 228, 255, 256, 257, 300, 511, 513, 1024, 2048}
WANT_BS = {1, 2, 7, 8, 9, 15, 17, 33, 64}
WANT_MASK_NS = {1, 63, 64, 65, 255, 256, 257, 300, 512, 513, 1024}
WANT_MASK_PS = {0.0, 0.2, 0.5, 0.9}
WANT_CHEB_NS = {1, 2, 3, 31, 32, 33, 127, 128, 129, 511, 512, 513, 640}
ATTN_NBC = 8                     # batch chunks of the attention forward (csrc/front.hip)


def _words(text):
    return [int(w, 16) for w in text.split()]


@pytest.mark.parametrize("counter,key,result", KAT)
def test_philox4x32_10_known_answers(counter, key, result):
    got = philox_ref.philox4x32_10(_words(counter), _words(key))
    assert [int(w) for w in got] == _words(result)
    # ... and as one element of an array call (the form the mask model uses)
    c = [np.array([0, w, 1], dtype=np.uint64) for w in _words(counter)]
    got = philox_ref.philox4x32_10(c, _words(key))
    assert [int(w[1]) for w in got] == _words(result)


def _philox_int(ctr, key):
    """the same ten rounds on Python integers (an independent transcription for the map test below)"""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0, c1, c2, c3


def test_philox_int_known_answers():
    for counter, key, result in KAT:
        assert list(_philox_int(_words(counter), _words(key))) == _words(result)


@pytest.mark.parametrize("N", [1, 63, 65, 256, 257, 300, 513, 1024])
def test_mask_model_column_map(N):
    """word (j >> 6) & 3 of counter (b N + i) NQ + (j >> 8) 64 + (j & 63); c2 | c3 = offset; key = seed -- element by element"""
    B = 3
    seed, offset = 0xFFFFFFFF00000001, (1 << 32) + 0xFFFFFFFF
    nq = 64 * ((N + 255) // 256)
    assert philox_ref.drop_nq(N) == nq
    rng = np.random.default_rng(N)
    words = philox_ref.mask_words(seed, offset, B, N)
    assert words.shape == (B * N, N) and words.dtype == np.uint32
    picks = {(0, 0, 0), (B - 1, N - 1, N - 1), (1, N // 2, min(N - 1, 256)), (1, 0, min(N - 1, 255)), (2, N - 1, min(N - 1, 64)),
             (0, N - 1, min(N - 1, 63)), (2, 0, min(N - 1, 320)), (1, N - 1, min(N - 1, 512))}
    picks |= {(int(rng.integers(B)), int(rng.integers(N)), int(rng.integers(N))) for _ in range(40)}
    for b, i, j in picks:
        idx = (b * N + i) * nq + (j >> 8) * 64 + (j & 63)
        w = _philox_int((idx & 0xFFFFFFFF, idx >> 32, offset & 0xFFFFFFFF, offset >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(words[b * N + i, j]) == w[(j >> 6) & 3], (b, i, j)
    # a subset of rows is the same rows
    rows = [0, B * N - 1]
    assert np.array_equal(philox_ref.mask_words(seed, offset, B, N, rows), words[rows])


def test_mask_model_keep_rule():
    """keep when float32(word) * 2^-32 >= float32(p), the conversion rounding to nearest"""
    # float32(0.2) = 13421773 * 2^-26: the threshold word is 13421773 * 64 = 0x33333340, and words round to multiples of 64 there
    # (0x33333320 is the tie, to even = down; 0x33333321 rounds up to the threshold).  Below 2^31 words round to multiples of
    # 128: 0x7FFFFFC0 is the tie, to even = up to 2^31.  0xFFFFFF7F rounds down to 2^32 - 256 (u = 1 - 2^-24), 0xFFFFFF80 up to 2^32.
    w = np.array([0, 1, 0x33333320, 0x33333321, 0x7FFFFFBF, 0x7FFFFFC0, 0x80000000, 0xFFFFFF7F, 0xFFFFFF80, 0xFFFFFFFF], dtype=np.uint32)
    assert philox_ref.keep(w, 0.0).all()
    assert list(philox_ref.keep(w, 0.2)) == [False] * 3 + [True] * 7
    assert list(philox_ref.keep(w, 0.5)) == [False] * 5 + [True] * 5
    assert list(philox_ref.keep(w, np.float32(1.0) - np.float32(2.0 ** -24))) == [False] * 7 + [True] * 3
    m = philox_ref.dropout_mask(0.0, 1, 2, 2, 70)
    assert m.shape == (2, 70, 70) and m.dtype == np.float32 and (m == 1).all()
    for p in (0.2, 0.5, 0.9):
        m = philox_ref.dropout_mask(p, 0x9E3779B97F4A7C15, 1 << 32, 4, 300)
        assert set(np.unique(m)) == {0.0, 1.0}
        n = m.size
        assert abs(m.mean() - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5, (p, m.mean())       # five sigma of the binomial
    # another offset, another seed: another mask
    a, b, c = (philox_ref.dropout_mask(0.5, s, o, 1, 64) for s, o in ((1, 1 << 32), (1, (1 << 32) + 1), (2, 1 << 32)))
    assert (a != b).any() and (a != c).any()


# ---- the case lists ----------------------------------------------------------------------------------------------------
def _n_features(N, nchunk):
    f = {"N <= 256" if N <= 256 else "N > 256"}
    if N % 64 in (0, 1, 63):
        f.add(f"N % 64 == {N % 64}")
    if N % 32:
        f.add("N % 32 != 0")
    if N % 4:
        f.add("N % 4 != 0")
    if N < nchunk:
        f.add("N < nchunk")
    return f


def _b_features(B):
    nbc = min(B, ATTN_NBC)
    bn = -(-B // nbc)                         # batches per chunk of sg_attention_fwd_kernel
    chunks = -(-B // bn)
    if B < 8:
        return {"B < 8"}
    if B == 8:
        return {"B == 8"}
    f = set()
    if chunks < ATTN_NBC:
        f.add("B > 8, fewer than 8 chunks")
    if B % bn:
        f.add("B > 8, ragged last chunk")
    return f


N_CLASSES = {"N <= 256", "N > 256", "N % 64 == 0", "N % 64 == 1", "N % 64 == 63", "N % 32 != 0", "N % 4 != 0", "N < nchunk"}
B_CLASSES = {"B < 8", "B == 8", "B > 8, fewer than 8 chunks", "B > 8, ragged last chunk"}
DROP_CLASSES = {f"dropout {on} at N {side} 256" for on in ("on", "off") for side in ("<=", ">")}
CHEB_CLASSES = {"cheb N <= 512", "cheb N > 512", "cheb N % 32 == 0", "cheb N % 32 != 0"}


def _case_features(case):
    N, B, p, mode, nchunk = case
    return _n_features(N, nchunk) | _b_features(B) | {f"dropout {'on' if p > 0 else 'off'} at N {'<=' if N <= 256 else '>'} 256"}


def _cheb_features(N):
    return {"cheb N <= 512" if N <= 512 else "cheb N > 512", "cheb N % 32 == 0" if N % 32 == 0 else "cheb N % 32 != 0"}


def _missing(front_cases, cheb_ns):
    have = set()
    for c in front_cases:
        have |= _case_features(c)
    for N in cheb_ns:
        have |= _cheb_features(N)
    return (N_CLASSES | B_CLASSES | DROP_CLASSES | CHEB_CLASSES) - have


def test_case_lists_reach_every_decision():
    assert not _missing(FRONT_CASES, CHEB_NS), _missing(FRONT_CASES, CHEB_NS)
    assert {c[0] for c in FRONT_CASES} == WANT_NS == set(NS), sorted(WANT_NS ^ {c[0] for c in FRONT_CASES})
    assert {c[1] for c in FRONT_CASES} == WANT_BS == set(BS), sorted(WANT_BS ^ {c[1] for c in FRONT_CASES})
    assert len(set(FRONT_CASES)) == len(FRONT_CASES)
    assert {c[2] for c in FRONT_CASES} == {0.0, 0.2, 0.5} and {c[3] for c in FRONT_CASES} == {"rand", "struct"}
    # both dL modes and both dropout rates on both sides of N = 256
    for side in (lambda N: N <= 256, lambda N: N > 256):
        assert {(c[2], c[3]) for c in FRONT_CASES if side(c[0]) and c[0] > 1} >= {(0.0, "rand"), (0.0, "struct"), (0.5, "rand"),
                                                                                   (0.5, "struct")}
        assert any(c[2] == 0.2 for c in FRONT_CASES if side(c[0]))
    assert set(CHEB_NS) == WANT_CHEB_NS and CHEB_GENERIC_N in CHEB_NS and CHEB_GENERIC_N < 512
    assert set(MASK_NS) == WANT_MASK_NS and set(MASK_PS) == WANT_MASK_PS
    assert all(s >> 32 and o >= 1 << 32 for s, o in MASK_SEEDS), "a mask seed without high bits, or an offset below 2^32"
    assert any(s >> 63 for s, o in MASK_SEEDS), "no seed with bit 63 set"


def test_nchunk_lists():
    for N in (5, 33, 300):
        assert NCHUNKS(N) == [1, 3, 16, N, N + 5]
    # the per-case nchunk of FRONT_CASES: the model's 16, 1, 3, N and beyond N all occur
    per_case = {("16" if c == 16 else "1" if c == 1 else "3" if c == 3 else "N" if c == N else "> N" if c > N else "?")
                for N, _, _, _, c in FRONT_CASES}
    assert per_case == {"16", "1", "3", "N", "> N"}, per_case
    # the nchunk sweep: both kernel forms, dropout on and off, N < 16 (chunks without a row), both dL modes
    assert {N <= 256 for N, _, _, _ in NCHUNK_CASES} == {True, False}
    assert {p > 0 for _, _, p, _ in NCHUNK_CASES} == {True, False}
    assert any(N < 16 for N, _, _, _ in NCHUNK_CASES) and {m for _, _, _, m in NCHUNK_CASES} == {"rand", "struct"}
    assert all(N in WANT_NS and B in WANT_BS for N, B, _, _ in NCHUNK_CASES)


@pytest.mark.parametrize("lost", sorted(N_CLASSES | B_CLASSES | DROP_CLASSES | CHEB_CLASSES))
def test_a_trimmed_list_fails(lost):
    """drop every case that shows one class: the check above names exactly that class as missing"""
    front = [c for c in FRONT_CASES if lost not in _case_features(c)]
    cheb = [N for N in CHEB_NS if lost not in _cheb_features(N)]
    assert len(front) + len(cheb) < len(FRONT_CASES) + len(CHEB_NS), f"no case shows {lost!r}"
    assert lost in _missing(front, cheb)


def test_b_features_are_the_launchers_chunking():
    """the forward's nbc = min(B, 8), bn = ceil(B / nbc), ceil(B / bn) chunks -- the figures the classes above stand on"""
    shapes = {B: (-(-B // min(B, 8)), -(-B // -(-B // min(B, 8)))) for B in sorted(WANT_BS)}
    assert shapes == {1: (1, 1), 2: (1, 2), 7: (1, 7), 8: (1, 8), 9: (2, 5), 15: (2, 8), 17: (3, 6), 33: (5, 7), 64: (8, 8)}
    assert _b_features(9) == {"B > 8, fewer than 8 chunks", "B > 8, ragged last chunk"} and _b_features(15) == {"B > 8, ragged last chunk"}
    assert _b_features(64) == set() and _b_features(16) == set()
