"""References, case lists and comparison helpers of the data stage suite (stemgnn_amd/csrc/data.hip): tests/test_hip_data_stage.py
runs the cases on the device, tests/test_data_cases.py proves on the CPU that they reach every launch decision and that the
comparison helpers fail when they should.

Every reference is plain numpy / Python written from the description of its entry in include/stemgnn_hip.h -- slicing and indexing
for the copies, fp64 for everything with arithmetic -- and none looks at how the kernels split their work.  The copies are applied
to a COPY OF THE POISONED DESTINATION, so the elements a call must leave alone are part of what is compared."""
import functools

import numpy as np

GUARD = 256                        # tests/util.GUARD, SENTINEL and SENTINEL_I (tests/test_data_cases.py checks they agree)
SENTINEL = -7777.25
SENTINEL_I = -77772525


# ---- comparison helpers (numpy in, AssertionError out; the device suite hands them whole buffers read back, guard included) ------
def _uint(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def assert_same_bits(got, want, what):
    """same shape, dtype and bits -- NaN payloads and the sign of zero included"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.flatnonzero(_uint(got).reshape(-1) != _uint(want).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {want.size} elements differ, first at flat index {int(bad[0])}: " \
                          f"{got.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}"


def assert_guard(full, n, what):
    """`full` = a buffer of n elements and the GUARD sentinels behind them, as read back"""
    full = np.asarray(full)
    assert full.shape == (n + GUARD,), (what, full.shape, n)
    sentinel = SENTINEL if full.dtype.kind == "f" else SENTINEL_I
    bad = np.flatnonzero(full[n:] != sentinel)
    assert bad.size == 0, f"{what}: guard element {int(bad[0])} behind {n} elements reads {full[n + bad[0]]!r}"


def check_buffer(full, want, what):
    """the guard is intact and the payload has exactly the bits of `want` (which holds the poison wherever nothing may be written)"""
    want = np.asarray(want)
    assert_guard(full, want.size, what)
    assert_same_bits(np.asarray(full)[: want.size].reshape(want.shape), want, what)


def check_status(got, want, what):
    """the gather status word: bit 0 = a window outside the series, bit 1 = a row past the end of `order`"""
    assert int(got) == int(want), f"{what}: status {int(got):#x}, expected {int(want):#x}"


def check_normalized(full, want, what):
    """normalise: the reference's bits where it is not NaN, NaN where it is"""
    want = np.asarray(want)
    assert_guard(full, want.size, what)
    got = np.asarray(full)[: want.size].reshape(want.shape)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at other places than the reference"
    assert_same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), want), what)


def check_metrics(full, want, exact, what, rtol=1e-12):
    """fp64 metrics: NaN exactly where the reference has NaN; `exact` (bool per element) marks the count-over-count and the
    single-term statistics, which must be equal; every other element within rtol of the reference, element by element"""
    want = np.asarray(want, dtype=np.float64)
    assert_guard(full, want.size, what)
    got = np.asarray(full)[: want.size]
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN at {np.flatnonzero(np.isnan(got)).tolist()[:8]}, " \
                                                f"the reference at {np.flatnonzero(nan).tolist()[:8]}"
    ex = np.asarray(exact, dtype=bool) & ~nan
    assert np.array_equal(got[ex], want[ex]), f"{what}: a statistic that must be equal differs at {np.flatnonzero(ex & (got != want))[:8]}"
    rest = ~ex & ~nan
    err = np.abs(got[rest] - want[rest])
    worst = float((err / np.abs(want[rest])).max()) if rest.any() and bool((want[rest] != 0).all()) else float(err.max(initial=0.0))
    print(f"{what}: worst relative error {worst:.2e} over {int(rest.sum())} sums, {int(ex.sum())} exact, {int(nan.sum())} NaN")
    assert bool((err <= rtol * np.abs(want[rest])).all()), (what, worst)
    return worst


# ---- normalise ------------------------------------------------------------------------------------------------------------------
# (T, N, clip01): one grid-stride pass and two (T N just above 2^20 with an N that does not divide the stride), clip on / off, N = 1
NORMALIZE_CASES = [(40, 7, 0), (40, 7, 1), (33, 1, 1), (33, 1, 0), (349600, 3, 1), (349600, 3, 0)]


@functools.lru_cache(maxsize=None)
def normalize_case(T, N, clip01):
    """raw [T, N] fp64, sub, div [N].  Column n has div = 2^(n % 3 - 1) and sub a multiple of 0.25, so raw = sub + k div lands on
    0 and 1 exactly; rows 0..9 hold NaN, +-inf, the values on and just beyond 0 and 1, both zeros and a value that leaves fp32."""
    g = np.random.default_rng(1000 * N + clip01 + T)
    sub = np.round(g.normal(size=N) * 4) / 4
    sub[N - 1] = 0.0
    div = 2.0 ** (np.arange(N) % 3 - 1)
    raw = sub + div * g.uniform(-0.5, 1.5, size=(T, N))
    eps = 2.0 ** -40
    special = [np.full(N, np.nan), np.full(N, np.inf), np.full(N, -np.inf), sub.copy(), sub + div, sub - div * eps,
               sub + div * (1 + eps), sub + div * (1 - eps), sub + div * eps, np.full(N, 1e300)]
    for r, v in enumerate(special):
        raw[r] = v
    raw[10, N - 1] = -0.0                                               # sub is 0 there: (-0.0 - 0.0) / div = -0.0
    raw[T - 1] = sub + div * (1 + eps)                                  # the last row as well: the tail of the last pass
    return raw, sub, div


def normalize_ref(raw, sub, div, clip01):
    with np.errstate(over="ignore", invalid="ignore"):
        v = (raw - sub) / div
        if clip01:
            v = np.clip(v, 0.0, 1.0)
        return v.astype(np.float32)


# ---- the gathers ----------------------------------------------------------------------------------------------------------------
GATHER_T, GATHER_W, GATHER_B = 40, 5, 3
_T, _W = GATHER_T, GATHER_W
# (N, H, hi): every thread class x copy form with all windows good (the first and the last window of the series among them), then
# batches that mix good rows with windows past the end, before the start and at a negative row, in both copy forms and all three
# thread classes, and H = 0 (hi = T is then a good window)
GATHER_CASES = [(N, 2, (_W, 17, _T - 2)) for N in (1, 7, 8, 255, 256, 257, 1023, 1024, 1027)] + \
               [(N, 2, (9, _T - 1, 4)) for N in (7, 8, 256, 1027)] + \
               [(N, 2, (-3, 20, _T + 7)) for N in (8, 257, 1024)] + \
               [(7, 0, (_W, _T, 20)), (8, 0, (_T + 1, _T, _W - 1)), (256, 0, (_T, _W, 11)), (255, 0, (_T + 3, 12, 0))]


@functools.lru_cache(maxsize=None)
def series_pair(T, N, seed=0):
    """series_x: finite; series_y: the same shape with a quarter of its readings NaN (the `_pair` entries' target series)"""
    g = np.random.default_rng(7 * N + T + seed)
    sx = g.normal(size=(T, N)).astype(np.float32)
    sy = g.normal(size=(T, N)).astype(np.float32)
    sy[g.random(size=(T, N)) < 0.25] = np.nan
    return sx, sy


def gather_ref(sx, sy, ends, W, H):
    """ends[b]: the window-end row of batch row b, or None for a row past the end of an epoch's order (queue form).  Returns
    x [B,W,N], y [B,H,N], the status bits and the rows that are zero.  x[b] = sx[end - W : end], y[b] = sy[end : end + H]."""
    T, N = sx.shape
    x, y = np.zeros((len(ends), W, N), np.float32), np.zeros((len(ends), H, N), np.float32)
    status, zero = 0, []
    for b, e in enumerate(ends):
        if e is None:
            status |= 2
            zero.append(b)
        elif e - W < 0 or e + H > T:
            status |= 1
            zero.append(b)
        else:
            x[b], y[b] = sx[e - W:e], sy[e:e + H]
    return x, y, status, zero


class QueueModel:
    """the iterator {position, ticket, count, wrap} of stemgnn_window_gather_queue as the header describes it"""

    def __init__(self, order, count, wrap, start=0):
        self.order, self.q = list(order), [start, 0, count, wrap]

    def call(self, sx, sy, B, W, H):
        pos, _, count, wrap = self.q
        ends = [self.order[pos + b] if pos >= 0 and pos + b < count else None for b in range(B)]
        out = gather_ref(sx, sy, ends, W, H)
        nxt = pos + B
        if wrap and nxt + B > count:                                     # no further full batch from there
            nxt = 0
        self.q = [nxt, 0, count, wrap]
        return out


# name -> B, W, H, N, count, wrap, start, calls, pair, bad {index in order: window-end row}
QUEUE_CASES = {
    "walk": dict(B=8, W=5, H=2, N=7, count=20, wrap=0, start=0, calls=4, pair=False, bad={}),
    "wrap": dict(B=8, W=5, H=2, N=7, count=20, wrap=1, start=0, calls=4, pair=False, bad={}),
    "bad_window": dict(B=3, W=5, H=2, N=127, count=6, wrap=0, start=0, calls=2, pair=False, bad={1: _T, 4: 2}),
    "negative_start": dict(B=3, W=5, H=2, N=128, count=6, wrap=0, start=-2, calls=2, pair=False, bad={}),
    "ragged_row_group": dict(B=20, W=5, H=2, N=511, count=45, wrap=0, start=0, calls=3, pair=False, bad={}),
    "one_row_group": dict(B=64, W=5, H=2, N=512, count=74, wrap=0, start=0, calls=2, pair=False, bad={70: _T - 1}),
    "one_workgroup": dict(B=1, W=1, H=0, N=5, count=3, wrap=0, start=0, calls=4, pair=False, bad={}),
    "one_workgroup_wrap": dict(B=1, W=1, H=0, N=4, count=3, wrap=1, start=0, calls=4, pair=False, bad={}),
    "wide_scalar": dict(B=3, W=5, H=2, N=513, count=5, wrap=0, start=0, calls=2, pair=False, bad={}),
    "pair_nan": dict(B=8, W=5, H=2, N=8, count=20, wrap=0, start=0, calls=3, pair=True, bad={}),
    "pair_nan_scalar": dict(B=3, W=5, H=2, N=7, count=7, wrap=1, start=0, calls=3, pair=True, bad={}),
}


def queue_order(c):
    g = np.random.default_rng(c["count"] + c["N"])
    order = g.integers(c["W"], _T - c["H"] + 1, size=c["count"]).tolist()
    for i, e in c["bad"].items():
        order[i] = e
    return order


# ---- MSE ------------------------------------------------------------------------------------------------------------------------
MSE_FWD_CASES = [1, 1023, 1025, 65536, 65537, 100003]
MSE_BWD_CASES = [1, 1025, 262144 + 77]
MSE_RTOL = 1e-6                                                          # the bound tests/test_hip_data.py::test_mse_loss_matches_torch holds


@functools.lru_cache(maxsize=None)
def mse_case(n):
    import torch

    g = torch.Generator().manual_seed(n)
    return torch.randn(n, generator=g).numpy(), torch.randn(n, generator=g).numpy()


def mse_ref(f, y, g=1.0):
    """the fp64 mean of (f - y)^2 and its gradient 2 g (f - y) / n"""
    d = f.astype(np.float64) - y.astype(np.float64)
    return float(np.mean(d * d)), 2.0 * float(g) * d / d.size


# ---- window shift ---------------------------------------------------------------------------------------------------------------
# (B, W, L, N, step, horizon): L = 1, in between, = W | 64 and 256 threads | take = L and the last call's take < L | step 0 and later
ROLL_CASES = [(2, 5, 1, 7, 0, 3), (2, 5, 2, 7, 2, 3), (2, 5, 5, 300, 0, 7), (3, 4, 3, 300, 3, 5), (2, 5, 2, 300, 0, 4), (1, 1, 1, 7, 4, 5)]
# the same with (Q, point): one row, and three with the point row first, in the middle and last
ROLL_QUANTILE_CASES = [c + qp for c, qp in zip(ROLL_CASES, [(1, 0), (3, 0), (3, 1), (3, 2), (3, 1), (3, 2)])] + [(2, 5, 5, 7, 1, 3, 1, 0)]


def roll_ref(inputs, forecast, steps, step, horizon, point=None):
    """inputs [B,W,N]; forecast [B,L,N] (or [B,Q,L,N] with `point`); steps: the poisoned forecast_steps [B,(Q,)horizon,N], not
    modified.  Returns inputs_next and the forecast_steps expected after the call."""
    L = forecast.shape[-2]
    take = min(horizon - step, L)
    steps = steps.copy()
    if point is None:
        steps[:, step:step + take] = forecast[:, :take]
        fp = forecast
    else:
        steps[:, :, step:step + take] = forecast[:, :, :take]
        fp = forecast[:, point]
    return np.concatenate([inputs[:, L:], fp], axis=1), steps


# ---- forecast store -------------------------------------------------------------------------------------------------------------
STORE_B, STORE_CAPACITY = 4, 10
# (H, N, pos): H N below one workgroup, one over a workgroup, two grid-stride passes | pos: every edge of [0, capacity)
STORE_CASES = [(H, N, pos) for H, N in ((3, 7), (1, 257), (3, 5463))
               for pos in (0, STORE_CAPACITY - STORE_B, STORE_CAPACITY - 1, -1, -STORE_B, STORE_CAPACITY)]


def store_ref(forecast, target, pos, out_f, out_t):
    """out_f / out_t: the poisoned slabs [capacity, H, N], not modified; rows pos + b outside them are dropped"""
    out_f, out_t = out_f.copy(), out_t.copy()
    for b in range(forecast.shape[0]):
        if 0 <= pos + b < out_f.shape[0]:
            out_f[pos + b], out_t[pos + b] = forecast[b], target[b]
    return out_f, out_t


# ---- evaluate() -----------------------------------------------------------------------------------------------------------------
def masked_metrics_numpy(t32, f32, mul=None, add=None):
    """evaluate()'s formulas over the elements whose target is not NaN, fp64: dict axis-variant -> (mape, mae, rmse)."""
    t, f = t32.astype(np.float64), f32.astype(np.float64)
    if mul is not None:
        t, f = t * mul + add, f * mul + add
    valid = ~np.isnan(t)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = f - t
        ape = np.abs(d) / np.abs(t) + 1e-5
        ape = np.where(ape > 5, 5, ape)
    out = {}
    for name, axis in (("overall", None), ("by_node", (0, 1)), ("by_step", (0, 2)), ("by_step_node", 0)):
        cnt = valid.sum(axis=axis).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = [np.where(valid, v, 0.0).sum(axis=axis) / cnt for v in (ape, np.abs(d), d * d)]
        out[name] = (mean[0], mean[1], np.sqrt(mean[2]))
    return out


def plain_metrics_numpy(t32, f32, mul=None, add=None):
    """the same with nothing left out: a NaN (a missing target, or 0 / 0 in the percentage error) spoils every mean it is part of"""
    t, f = t32.astype(np.float64), f32.astype(np.float64)
    if mul is not None:
        t, f = t * mul + add, f * mul + add
    with np.errstate(divide="ignore", invalid="ignore"):
        d = f - t
        ape = np.abs(d) / np.abs(t) + 1e-5
        ape = np.where(ape > 5, 5, ape)
        out = {}
        for name, axis in (("overall", None), ("by_node", (0, 1)), ("by_step", (0, 2)), ("by_step_node", 0)):
            out[name] = (np.mean(ape, axis=axis), np.mean(np.abs(d), axis=axis), np.sqrt(np.mean(d * d, axis=axis)))
    return out


def eval_pack(m):
    """the dict of either function above in the layout of `out`: overall[3] | by_node[3][N] | by_step[3][H] | by_step_node[3][H][N]"""
    return np.concatenate([np.asarray(v, dtype=np.float64).reshape(-1) for name in ("overall", "by_node", "by_step", "by_step_node")
                           for v in m[name]])


EVAL_COUNTS = (1, 63, 64, 65, 129)
EVAL_SHAPES = ((1, 1), (3, 7), (3, 86), (2, 300), (257, 1))
# (count, H, N, masked, denorm): every count and every (H, N) in both forms, each form with and without mul / add; (129, 3, 86) has
# three chunks and H N = 258 columns, one workgroup and two columns
EVAL_CASES = [(EVAL_COUNTS[i], *EVAL_SHAPES[(i + 2 * m) % 5], m, (i + m) % 2) for m in (0, 1) for i in range(5)] + \
             [(129, 3, 86, 0, 1), (129, 3, 86, 1, 0), (65, 2, 300, 0, 0), (65, 3, 7, 1, 1), (1, 3, 7, 0, 1)]


def eval_zero_at(H, N):
    """the column (h, n) that holds the zero targets: one the masked cases do not blank as a whole"""
    return (H // 2 if H > 2 else 0), (N // 2 if N > 2 else N - 1)


@functools.lru_cache(maxsize=None)
def eval_case(count, H, N, masked, denorm):
    """target, forecast [count, H, N] fp32, mul, add [N] fp64 (None without `denorm`).  From 63 rows on, one target is exactly 0 with
    an error (its percentage error is clipped to 5), and at count = 65 another is 0 with no error (0 / 0: NaN in every unmasked
    MAPE it belongs to).  Masked: a quarter of the targets NaN, plus a whole step, a whole node and one whole column where there
    is more than one of them."""
    g = np.random.default_rng(count + 1000 * H + 7 * N + masked)
    t = (g.normal(size=(count, H, N)) + 3.0).astype(np.float32)
    f = (t + 0.3 * g.normal(size=(count, H, N))).astype(np.float32)
    if masked:
        t[g.random(size=t.shape) < 0.25] = np.nan
        if H > 1:
            t[:, H - 1, :] = np.nan
        if N > 1:
            t[:, :, 0] = np.nan
        if H * N > 2:
            t[:, 0, N - 1] = np.nan
    h0, n0 = eval_zero_at(H, N)
    if count >= 63:
        t[5, h0, n0] = 0.0
    if count == 65:
        t[64, h0, n0], f[64, h0, n0] = 0.0, 0.0
    mul, add = (g.uniform(0.5, 3.0, size=N), g.uniform(-2.0, 8.0, size=N)) if denorm else (None, None)
    return t, f, mul, add


def eval_ref(t, f, mul, add, masked):
    """the expected `out` and which of its elements must be EQUAL.  Every statistic is a sum of reals, so normally none -- but with
    count = 1 a by_step_node MAPE or MAE is a single term: no order to differ in, every operation on the way (the widening, the
    multiply and the add of the de-normalisation, subtract, divide, + 1e-5, / 1) a correctly rounded IEEE one on both sides.  A
    kernel that fuses v * mul + add into one FMA fails there.  (RMSE goes through sqrt and keeps the rtol.)"""
    want = eval_pack((masked_metrics_numpy if masked else plain_metrics_numpy)(t, f, mul, add))
    exact = np.zeros(want.size, dtype=bool)
    count, H, N = t.shape
    if count == 1:
        sn = 3 + 3 * N + 3 * H                                           # by_step_node[3][H][N] starts here
        exact[sn: sn + 2 * H * N] = True
    return want, exact


# ---- quantile metrics -----------------------------------------------------------------------------------------------------------
def scores64(t, f, taus, mul, add, ignore_nan):
    """numpy fp64 restatement of stemgnn_quantile_metrics: dict name -> (overall, per step [.., H])."""
    t, f = t.astype(np.float64), f.astype(np.float64)
    C, Q, H, N = f.shape
    if mul is not None:
        t, f = t * mul + add, f * mul + add
    valid = ~np.isnan(t) if ignore_nan else np.ones_like(t, dtype=bool)
    P = Q // 2

    def mean(v, h):                                     # v [C,H,N] -> mean over the valid elements of step h (None: all steps)
        sel = valid if h is None else valid[:, h]
        vv = v if h is None else v[:, h]
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.float64(vv[sel].sum()) / np.float64(sel.sum())

    def both(v):
        return mean(v, None), np.array([mean(v, h) for h in range(H)])
    out = {k: ([], []) for k in ("pinball", "coverage", "interval_coverage", "interval_width")}

    def push(k, v):
        o, s = both(v)
        out[k][0].append(o)
        out[k][1].append(s)
    for q in range(Q):
        d = f[:, q] - t
        push("pinball", np.where(d >= 0, (1 - taus[q]) * d, -taus[q] * d))
        push("coverage", (t <= f[:, q]).astype(np.float64))
    for i in range(P):
        lo, hi = f[:, i], f[:, Q - 1 - i]
        push("interval_coverage", ((lo <= t) & (t <= hi)).astype(np.float64))
        push("interval_width", hi - lo)
    res = {k: (np.array(o), np.array(s).reshape(len(o), H)) for k, (o, s) in out.items()}
    cross = (np.diff(f, axis=1) < 0).any(axis=1).astype(np.float64) if Q > 1 else np.zeros_like(t)
    res["crossing"] = both(cross)
    return res


def levels(Q):
    return tuple((q + 1) / (Q + 1) for q in range(Q))


# (count, Q, H, N, masked, denorm): Q odd, even (a pair straddling the middle), 1 and the limit 32 | one chunk and two | one column and
# 258 of them, in both forms
QUANTILE_CASES = [(1, 1, 1, 1), (65, 2, 3, 86), (65, 3, 1, 1), (1, 32, 3, 86), (65, 32, 3, 86), (65, 3, 3, 86), (1, 2, 1, 1)]
QUANTILE_CASES = [c + (m, (i + m) % 2) for m in (0, 1) for i, c in enumerate(QUANTILE_CASES)]


@functools.lru_cache(maxsize=None)
def quantile_case(C, Q, H, N, masked, denorm):
    """as tests/test_hip_quantile_tail.metric_case -- sorted levels around the target, one element in ten with its outer levels swapped
    (crossings) -- plus ties target == forecast_q and equal adjacent levels (which are no crossing)"""
    g = np.random.default_rng(100 * C + Q + 7 * N + masked)
    t = g.normal(size=(C, H, N)).astype(np.float32)
    f = (t[:, None] + np.sort(g.normal(size=(C, Q, H, N)), axis=1)).astype(np.float32)
    if Q > 1:
        swap = g.random(size=(C, H, N)) < 0.1
        a, b = f[:, 0].copy(), f[:, Q - 1].copy()
        f[:, 0], f[:, Q - 1] = np.where(swap, b, a), np.where(swap, a, b)
        same = g.random(size=(C, H, N)) < 0.1
        f[:, Q // 2] = np.where(same, f[:, Q // 2 - 1], f[:, Q // 2])
    tie = g.random(size=(C, H, N)) < 0.1
    f[:, Q // 2] = np.where(tie, t, f[:, Q // 2])
    if C == 1:
        f[0, Q // 2, 0, 0] = t[0, 0, 0]                                  # the smallest cases hold a tie for certain
    if masked:
        if t.size > 1:                                                  # (a single element stays: the tie)
            t[g.random(size=t.shape) < 0.25] = np.nan
        if H > 1:
            t[:, H - 1, :] = np.nan                                     # one whole step with nothing valid
    mul, add = (g.uniform(0.5, 3.0, size=N), g.uniform(-2.0, 8.0, size=N)) if denorm else (None, None)
    return t, f, mul, add


def quantile_pack(res, Q, H):
    """scores64's dict in the layout of `out` (overall[K] | by_step[K][H]) and the mask of its count-over-count statistics"""
    names = ("pinball", "coverage", "interval_coverage", "interval_width", "crossing")
    overall = np.concatenate([np.asarray(res[k][0], dtype=np.float64).reshape(-1) for k in names])
    steps = np.concatenate([np.asarray(res[k][1], dtype=np.float64).reshape(-1, H) for k in names])
    exact1 = np.concatenate([np.full(np.asarray(res[k][0]).size, k in ("coverage", "interval_coverage", "crossing")) for k in names])
    K = 2 * Q + 2 * (Q // 2) + 1
    assert overall.shape == (K,) and steps.shape == (K, H)
    return np.concatenate([overall, steps.reshape(-1)]), np.concatenate([exact1, np.repeat(exact1, H)])


def quantile_ref(t, f, taus, mul, add, masked):
    """the expected `out` and which elements must be EQUAL: the count-over-count statistics, and every statistic that is a single
    term (count N = 1: the per-step ones; count H N = 1: all), as in eval_ref"""
    C, Q, H, N = f.shape
    want, exact = quantile_pack(scores64(t, f, taus, mul, add, ignore_nan=bool(masked)), Q, H)
    K = want.size // (H + 1)
    if C * N == 1:
        exact[K:] = True
    if C * H * N == 1:
        exact[:K] = True
    return want, exact


# ---- what stemgnn_data_plan is asked for each case -------------------------------------------------------------------------------
def plan_args(entry, case):
    if entry == "normalize":
        return case[:2]
    if entry == "gather":
        return (GATHER_B, GATHER_W, case[1], case[0])
    if entry == "gather_queue":
        c = QUEUE_CASES[case]
        return (c["B"], c["W"], c["H"], c["N"])
    if entry in ("mse_fwd", "mse_bwd"):
        return (case,)
    if entry == "roll":
        return case[:4]
    if entry == "roll_quantile":
        return case[:4] + (case[6],)
    if entry == "forecast_store":
        return (STORE_B, case[0], case[1])
    if entry == "eval":
        return case[:3]
    if entry == "quantile_metrics":
        return case[:4]
    raise KeyError(entry)


CASES = {"normalize": NORMALIZE_CASES, "gather": GATHER_CASES, "gather_queue": list(QUEUE_CASES), "mse_fwd": MSE_FWD_CASES,
         "mse_bwd": MSE_BWD_CASES, "roll": ROLL_CASES, "roll_quantile": ROLL_QUANTILE_CASES, "forecast_store": STORE_CASES,
         "eval": EVAL_CASES, "quantile_metrics": QUANTILE_CASES}
