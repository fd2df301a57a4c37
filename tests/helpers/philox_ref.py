"""Host model of the attention dropout map of csrc/front.hip: plain numpy Philox4x32-10 (Salmon et al., "Parallel random
numbers: as easy as 1, 2, 3", SC'11; the Random123 known-answer vectors pin it in tests/test_front_cases.py) and the
library's element -> (counter, word) map on top of it.

Element (b, i, j) of the [B, N, N] keep mask takes word (j >> 6) & 3 of the call with
    counter  c0 | c1 = (b N + i) * NQ + (j >> 8) * 64 + (j & 63)   (64-bit, low word first),   NQ = 64 * ceil(N / 256)
             c2 | c3 = offset                                       (64-bit, low word first)
    key      k0 | k1 = seed
and is kept when float32(word) * float32(2^-32) >= float32(p) (uint32 -> float32 round-to-nearest)."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # the two round multipliers
W0, W1 = 0x9E3779B9, 0xBB67AE85          # the key schedule's Weyl increments
_U32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) c0..c3, key: two k0, k1 (uint32 values) -> four uint32 arrays (broadcast shape)."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & _U32 for c in counter)
    k0, k1 = (np.asarray(k, dtype=np.uint64) & _U32 for k in key)
    for _ in range(10):
        p0 = np.uint64(M0) * c0                  # 32 x 32 -> 64 bit: never wraps a uint64
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _U32, (p0 >> _S32) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + np.uint64(W0)) & _U32, (k1 + np.uint64(W1)) & _U32
    return tuple(np.asarray(c).astype(np.uint32) for c in (c0, c1, c2, c3))


def drop_nq(N):
    return 64 * ((N + 255) // 256)


def mask_words(seed, offset, B, N, rows=None):
    """uint32 [rows, N]: the Philox word of every element of the rows `rows` (flat b N + i; default all B N of them)."""
    seed, offset = int(seed), int(offset)
    rows = np.arange(B * N, dtype=np.uint64) if rows is None else np.asarray(rows, dtype=np.uint64)
    nq = drop_nq(N)
    ctr = rows[:, None] * np.uint64(nq) + np.arange(nq, dtype=np.uint64)[None, :]       # every call of these rows, once
    w = philox4x32_10((ctr & _U32, ctr >> _S32, offset & 0xFFFFFFFF, (offset >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    j = np.arange(N)
    return np.stack(w, axis=-1)[:, (j >> 8) * 64 + (j & 63), (j >> 6) & 3]


def keep(words, p):
    return words.astype(np.float32) * np.float32(2.0 ** -32) >= np.float32(p)


def dropout_mask(p, seed, offset, B, N):
    """float32 [B, N, N] of 0 / 1: what stemgnn_dropout_mask must write for device seed words {seed, offset}."""
    out = np.empty((B * N, N), dtype=np.float32)
    chunk_rows = max(1, (1 << 21) // N)
    for r0 in range(0, B * N, chunk_rows):
        rows = np.arange(r0, min(B * N, r0 + chunk_rows), dtype=np.uint64)
        out[r0:r0 + rows.size] = keep(mask_words(seed, offset, B, N, rows), p)
    return out.reshape(B, N, N)
