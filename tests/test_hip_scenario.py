"""GPU: scenario forecasts -- the two kernels of csrc/scenario.hip against the numpy restatement of their definition
(tests/helpers/scenario_ref.py), and trainer.rolling_scenarios / LiveForecaster.scenarios on top of them.

Comparisons are of bit patterns.  One remark: a draw is ARITHMETIC (a subtraction, a product, a sum), and where that arithmetic
is invalid (inf - inf, 0 * inf, a NaN operand) IEEE leaves the NaN's sign and payload to the implementation -- the host
produces 0xffc00000 where the device produces 0x7fc00000 -- so a drawn value is compared as "the same bits, or NaN on both
sides" (same_draws).  Everything that is a SELECTION -- the round-0 bands, the window rows that move up, the order statistics of
scenario_bands -- keeps its input's bits, NaN payloads included, and is compared strictly (same_bits).

Every output lies inside a NaN-filled buffer with guard words on both sides, compared whole: what the definition does not write
must still hold the guard.  Statistical bounds (coverage) are the issue's: nominal 0.9, minus about 0.02 for interpolating seven
levels linearly, plus or minus four binomial standard deviations over 1600 walks (0.03), rounded outwards to [0.84, 0.96]; the
point-path roll, which the numpy check of the issue put at 0.43 - 0.46, must stay below 0.6."""
import ctypes
import statistics

import numpy as np
import pytest
import torch

from tests.helpers import scenario_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 20261020
GUARD = 64                                   # floats either side of every output
ORIGIN0 = 2 ** 33 + 12345                    # above 2^32 / (S * horizon) for every case: the counter's high word is live
KEY, OFFSET = 0x9E3779B97F4A7C15, 0x100000003
LEVELS = {2: (0.1, 0.9), 3: (0.1, 0.5, 0.9), 9: (0.05, 0.1, 0.25, 0.4, 0.5, 0.6, 0.75, 0.9, 0.95),
          32: tuple((i + 1) / 33 for i in range(32))}
NAN_PAYLOAD = np.array([0x7fc00123], np.uint32).view(np.float32)[0]


def u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(u32(a), u32(b))


def same_draws(a, b):
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(u32(a)[~na], u32(b)[~nb])


def guarded(shape, misalign):
    """(whole buffer on the device, the view of `shape` inside it): NaN everywhere; misalign: the view starts 4 bytes off a
    16-byte boundary"""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD + 1,), float("nan"), device=DEV)
    lo = GUARD + (1 if misalign else 0)
    view = whole[lo:lo + n].view(*shape)
    assert (view.data_ptr() % 16 != 0) == bool(misalign)
    return whole, view


def device_copy(a, misalign):
    whole, view = guarded(a.shape, misalign)
    view.copy_(torch.from_numpy(a))
    return whole, view


def special_columns(f, rng):
    """forecast [B, Q, L, N] float32 with, by flat column index, ties, a crossing (descending) column, +-0, infinities and NaN"""
    B, Q, L, N = f.shape
    cols = f.transpose(0, 2, 3, 1).reshape(-1, Q)             # a copy: [B * L * N, Q]
    for c in range(cols.shape[0]):
        kind = c % 11
        if kind == 1:
            cols[c] = cols[c, 0]                              # all tied
        elif kind == 2:
            cols[c] = -np.sort(-cols[c])                      # crossing: descending
        elif kind == 3:
            cols[c, ::2], cols[c, 1::2] = 0.0, -0.0
        elif kind == 4:
            cols[c, -1] = np.inf
        elif kind == 5:
            cols[c, 0], cols[c, -1] = np.inf, -np.inf
        elif kind == 6:
            cols[c, rng.integers(Q)] = NAN_PAYLOAD
        elif kind == 7:
            cols[c, :2] = cols[c, 1]                          # a tie of two, then a crossing pair
            cols[c, -1] = cols[c, 0] - 1
        elif kind == 8:
            cols[c, 0], cols[c, -1] = -0.0, 0.0
    return np.ascontiguousarray(cols.reshape(B, L, N, Q).transpose(0, 3, 1, 2))


# (N, Q, S, W, L, round0, coupling, tails, step, horizon, misalign, last)
ROLL_CASES = [
    (1, 2, 1, 4, 1, True, "independent", "linear", 0, 7, False, False),
    (1, 3, 7, 4, 1, False, "path", "clamp", 6, 7, False, True),
    (5, 3, 2, 3, 3, True, "path", "clamp", 0, 7, False, False),
    (5, 9, 64, 12, 3, False, "independent", "linear", 6, 7, False, False),       # the last round, cut short, window still made
    (5, 32, 2, 12, 3, True, "independent", "linear", 0, 7, False, False),
    (64, 3, 64, 12, 3, True, "independent", "linear", 0, 7, False, False),       # 16-byte path, round 0
    (64, 9, 7, 12, 3, False, "independent", "clamp", 3, 7, False, False),        # 16-byte path, fewer threads (Q = 9)
    (64, 32, 2, 3, 3, False, "path", "linear", 3, 7, False, False),              # 16-byte path, 64 threads (Q = 32)
    (64, 2, 2, 4, 1, False, "path", "linear", 5, 7, True, False),                # N % 4 == 0 off a 16-byte boundary: scalar
    (64, 3, 7, 12, 3, True, "path", "clamp", 0, 2, True, True),                  # horizon below L
    (257, 3, 64, 12, 3, False, "independent", "linear", 6, 7, False, True),      # cut short, no next window
    (257, 9, 7, 3, 3, True, "path", "linear", 0, 7, False, False),
    (257, 2, 2, 12, 3, False, "independent", "clamp", 3, 7, True, False),
    (64, 3, 1, 12, 3, True, "independent", "clamp", 0, 7, False, False),         # S = 1: fan == 1 == S
]


@pytest.mark.parametrize("case", ROLL_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_scenario_roll_matches_the_restatement(case):
    from stemgnn_amd import _lib
    N, Q, S, W, L, round0, coupling, tails, step, horizon, misalign, last = case
    lib = _lib.load()
    taus = LEVELS[Q]
    Bo = 2 if S >= 64 else 3
    fan = S if round0 else 1
    Bsrc = Bo if round0 else Bo * S
    rng = np.random.default_rng(SEED + N + 7 * Q + 13 * S)
    inputs = rng.normal(size=(Bsrc, W, N)).astype(np.float32)
    forecast = special_columns(rng.normal(size=(Bsrc, Q, L, N)).astype(np.float32), rng)
    # the restatement, in place on NaN-filled arrays
    ref_paths = np.full((Bo, S, horizon, N), np.nan, np.float32)
    ref_next = None if last else np.full((Bo * S, W, N), np.nan, np.float32)
    ref_bands = np.full((Bo, Q, horizon, N), np.nan, np.float32) if round0 else None
    R.roll(inputs, forecast, taus, Bo, S, fan, step, horizon, ORIGIN0, KEY, OFFSET, coupling, tails, ref_paths, ref_bands,
           ref_next)
    _, d_in = device_copy(inputs, misalign)
    _, d_fc = device_copy(forecast, misalign)
    w_paths, d_paths = guarded(ref_paths.shape, misalign)
    w_next, d_next = (None, None) if last else guarded(ref_next.shape, misalign)
    w_bands, d_bands = guarded(ref_bands.shape, misalign) if round0 else (None, None)
    rc = lib.stemgnn_scenario_roll(d_in.data_ptr(), d_fc.data_ptr(), _lib.host_floats(taus), Bo, S, fan, W, L, N, Q, step,
                                   horizon, ORIGIN0, KEY, OFFSET, _lib.SG_SCENARIO_COUPLING[coupling],
                                   _lib.SG_SCENARIO_TAILS[tails], None if last else d_next.data_ptr(), d_paths.data_ptr(),
                                   d_bands.data_ptr() if round0 else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    lo = GUARD + (1 if misalign else 0)

    def whole_of(ref):
        out = np.full(ref.size + 2 * GUARD + 1, np.nan, np.float32)
        out[lo:lo + ref.size] = ref.reshape(-1)
        return out

    got_paths = w_paths.cpu().numpy()
    exp_paths = whole_of(ref_paths)
    # the guards and every unwritten step hold the fill's NaN (one bit pattern); the drawn rows compare as draws
    written = np.zeros(ref_paths.shape, bool)
    written[:, :, step:step + min(L, horizon - step)] = True
    wmask = np.zeros(exp_paths.size, bool)
    wmask[lo:lo + ref_paths.size] = written.reshape(-1)
    assert same_draws(got_paths[wmask], exp_paths[wmask])
    assert same_bits(got_paths[~wmask], exp_paths[~wmask])
    assert np.isfinite(ref_paths[written]).mean() > 0.5                     # (the special columns are a minority)
    if not last:
        got, exp = w_next.cpu().numpy(), whole_of(ref_next)
        drawn = np.zeros(ref_next.shape, bool)
        drawn[:, W - L:] = True
        dmask = np.zeros(exp.size, bool)
        dmask[lo:lo + ref_next.size] = drawn.reshape(-1)
        assert same_draws(got[dmask], exp[dmask])
        assert same_bits(got[~dmask], exp[~dmask])                          # the rows that move up, and the guards
        assert not np.isnan(got[lo:lo + ref_next.size].reshape(ref_next.shape)[:, :W - L]).any()
    if round0:
        assert same_bits(w_bands.cpu().numpy(), whole_of(ref_bands))        # the model's own columns: payloads and signs kept
    # the inputs were only read
    assert same_bits(d_in.cpu().numpy(), inputs) and same_bits(d_fc.cpu().numpy(), forecast)


def test_the_draw_lies_on_the_quantile_function():
    """A property of the definition itself, on the restatement's side of the comparison above: with clamped tails every draw of
    a finite column lies within [min, max] of the column -- up to the two roundings of v_i + (v_{i+1} - v_i) * wt at a magnitude
    below 8, 2 * 2^-24 * 8 < 1e-6 -- and with linear tails the draws at u outside [0.1, 0.9], a fifth of them, may leave it."""
    rng = np.random.default_rng(SEED)
    col = rng.normal(size=(1, 3, 1, 4096)).astype(np.float32)
    assert np.abs(col).max() < 8
    u = R.uniform(rng.integers(0, 2 ** 32, size=(1, 1, 4096), dtype=np.uint64).astype(np.uint32))
    assert u.min() > 0 and u.max() < 1
    y = R.draw(col, LEVELS[3], u, "clamp")
    assert (y >= col.min(axis=1) - 1e-6).all() and (y <= col.max(axis=1) + 1e-6).all()
    y = R.draw(col, LEVELS[3], u, "linear")
    assert ((y < col.min(axis=1)) | (y > col.max(axis=1))).mean() > 0.1      # u outside [0.1, 0.9]: 0.2 of the draws


BANDS_S = (1, 2, 7, 64, 200, 300, 1024)      # tiles of 64, 64, 64, 64, 32, 16 and 8 columns


@pytest.mark.parametrize("S", BANDS_S)
def test_scenario_bands_match_a_stable_sort(S):
    from stemgnn_amd import _lib
    lib = _lib.load()
    Bo, horizon, N, L = 2, 5, 37, 3                              # 185 / 74 columns per origin: several tiles, the last partial
    taus = LEVELS[9] if S >= 7 else LEVELS[3]
    Q = len(taus)
    rng = np.random.default_rng(SEED + S)
    paths = np.round(rng.normal(size=(Bo, S, horizon, N)), 1).astype(np.float32)            # one decimal: many ties
    paths[rng.random(paths.shape) < 0.05] = np.nan
    paths[rng.random(paths.shape) < 0.02] = NAN_PAYLOAD
    paths[rng.random(paths.shape) < 0.02] = -0.0
    paths[rng.random(paths.shape) < 0.02] = np.inf
    paths[rng.random(paths.shape) < 0.02] = -np.inf
    paths[0, :, 4, 3] = np.nan                                   # a column of NaN only
    paths[1, :, 4, 5] = 0.25                                     # a column of one value
    ranks = [R.rank(t, S) for t in taus]
    assert ranks == [lib.stemgnn_scenario_rank(t, S) for t in taus]
    _, d_paths = device_copy(paths, False)
    for step_from in (0, L, horizon):
        ref = np.full((Bo, Q, horizon, N), np.nan, np.float32)
        R.bands_of(paths, taus, step_from, ref)
        whole, d_bands = guarded(ref.shape, False)
        rc = lib.stemgnn_scenario_bands(d_paths.data_ptr(), Bo, S, horizon, N, Q, (ctypes.c_int * Q)(*ranks), step_from,
                                        d_bands.data_ptr(), None)
        assert rc == 0
        torch.cuda.synchronize()
        exp = np.full(ref.size + 2 * GUARD + 1, np.nan, np.float32)
        exp[GUARD:GUARD + ref.size] = ref.reshape(-1)
        assert same_bits(whole.cpu().numpy(), exp), step_from     # the steps below step_from and the guards: untouched
    # the reference is numpy's stable sort: against plain np.sort the values agree wherever no NaN / zero sign is involved
    v = np.sort(paths, axis=1, kind="stable")
    ref = np.full((Bo, Q, horizon, N), np.nan, np.float32)
    R.bands_of(paths, taus, 0, ref)
    for q, k in enumerate(ranks):
        np.testing.assert_array_equal(ref[:, q], v[:, k - 1])     # (== : NaN equals NaN here, -0 equals +0)
    assert same_bits(d_paths.cpu().numpy(), paths)


# ---- end to end: a real small quantile model -----------------------------------------------------------------------------
N_E, W_E, H_E, TAUS_E = 9, 12, 3, (0.1, 0.5, 0.9)
_e2e = {}


def e2e():
    """The model, five windows and their graph, made once and never changed."""
    if not _e2e:
        from stemgnn_amd import Model
        torch.manual_seed(SEED)
        model = Model(N_E, 2, W_E, 2, horizon=H_E, quantiles=TAUS_E).to(DEV).eval()
        g = torch.Generator().manual_seed(SEED + 1)
        x = torch.randn(5, W_E, N_E, generator=g).to(DEV)
        y = torch.randn(5, 7, N_E, generator=g).to(DEV)
        _e2e.update(model=model, x=x, y=y, graph=model.latent_graph(x))
    return _e2e["model"], _e2e["x"], _e2e["y"], _e2e["graph"]


def tbits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def tsame(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(tbits(a), tbits(b))


def test_within_the_model_horizon_the_bands_are_rolling_forecasts():
    from stemgnn_amd import trainer
    model, x, y, graph = e2e()
    loader = [(x, y[:, :3].contiguous())]
    for kw in ({}, dict(adjacency=graph)):
        want, wt = trainer.rolling_forecast(model, loader, 3, **kw)
        got, gt = trainer.rolling_scenarios(model, loader, 3, paths=7, seed=5, **kw)
        assert tsame(got, want) and tsame(gt, wt)
    assert not model.training
    model.train()
    trainer.rolling_scenarios(model, loader, 3, paths=2)
    assert model.training                                         # the training state is restored
    model.eval()


def test_rolling_scenarios_beyond_the_model_horizon():
    from stemgnn_amd import ops, trainer
    model, x, y, graph = e2e()
    whole = [(x, y)]
    want, _ = trainer.rolling_forecast(model, whole, 7, adjacency=graph)
    bands, target, paths = trainer.rolling_scenarios(model, whole, 7, paths=16, seed=11, adjacency=graph, return_paths=True)
    assert bands.shape == (5, 3, 7, N_E) and paths.shape == (5, 16, 7, N_E) and tsame(target, y)
    assert tsame(bands[:, :, :3], want[:, :, :3])                 # the first round: the model's own rows
    assert not tsame(bands[:, :, 3:], want[:, :, 3:])
    assert bool(torch.isfinite(bands).all()) and bool(torch.isfinite(paths).all())
    # the loader's batching does not matter: 5 windows at once == 2 + 3
    split = [(x[:2], y[:2]), (x[2:], y[2:])]
    b2, t2, p2 = trainer.rolling_scenarios(model, split, 7, paths=16, seed=11, adjacency=graph, return_paths=True)
    assert tsame(b2, bands) and tsame(t2, target) and tsame(p2, paths)
    # one seed, one result; another seed, another
    b3 = trainer.rolling_scenarios(model, whole, 7, paths=16, seed=11, adjacency=graph)[0]
    b4 = trainer.rolling_scenarios(model, whole, 7, paths=16, seed=12, adjacency=graph)[0]
    assert tsame(b3, bands) and not tsame(b4[:, :, 3:], bands[:, :, 3:]) and tsame(b4[:, :, :3], bands[:, :, :3])
    # the bands beyond the first round are the order statistics of exactly the returned paths
    again = bands.clone()
    again[:, :, 3:] = float("nan")
    ops.scenario_bands(paths, TAUS_E, 3, again)
    assert tsame(again, bands)
    ref = np.full(tuple(bands.shape), np.nan, np.float32)
    R.bands_of(paths.cpu().numpy(), TAUS_E, 3, ref)
    assert same_bits(bands[:, :, 3:].cpu().numpy(), ref[:, :, 3:])
    # without adjacency= it runs too (the graph of a round is then the mean over the batch's paths)
    b5 = trainer.rolling_scenarios(model, whole, 7, paths=4, seed=11)[0]
    assert b5.shape == bands.shape and bool(torch.isfinite(b5).all())


Z7 = (0.05, 0.1, 0.25, 0.5, 0.75, 0.9, 0.95)


class Walk:
    """A stand-in model whose one-step quantiles are exact for a driftless random walk with unit steps:
    predict(x) = last row + z_tau, L = 1."""
    quantiles, point_index, training = Z7, 3, False

    def __init__(self):
        self.z = torch.tensor([statistics.NormalDist().inv_cdf(t) for t in Z7], dtype=torch.float32, device=DEV)

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def predict(self, x, adjacency=None):
        return (x[:, None, -1:, :] + self.z[None, :, None, None]).contiguous(), None

    __call__ = predict


def test_path_coupling_moves_the_whole_network_together():
    from stemgnn_amd import trainer
    x, y = torch.zeros(3, 4, 6, device=DEV), torch.zeros(3, 5, 6, device=DEV)
    _, _, paths = trainer.rolling_scenarios(Walk(), [(x, y)], 5, paths=8, seed=3, coupling="path", return_paths=True)
    assert tsame(paths, paths[..., :1].expand_as(paths).contiguous())
    assert len(set(paths[0, :, 4, 0].tolist())) > 1               # ... while the paths differ from one another
    _, _, free = trainer.rolling_scenarios(Walk(), [(x, y)], 5, paths=8, seed=3, return_paths=True)
    assert not tsame(free, free[..., :1].expand_as(free).contiguous())


def test_coverage_at_step_eight_of_a_random_walk():
    from stemgnn_amd import trainer
    g = torch.Generator().manual_seed(SEED + 2)
    target = torch.randn(200, 8, 8, generator=g).cumsum(dim=1).to(DEV)
    loader = [(torch.zeros(200, 4, 8, device=DEV), target)]
    bands, tg = trainer.rolling_scenarios(Walk(), loader, 8, paths=256, seed=1)
    covered = ((bands[:, 0, 7] <= tg[:, 7]) & (tg[:, 7] <= bands[:, 6, 7])).float().mean().item()
    point, _ = trainer.rolling_forecast(Walk(), loader, 8)
    point_covered = ((point[:, 0, 7] <= tg[:, 7]) & (tg[:, 7] <= point[:, 6, 7])).float().mean().item()
    print(f"coverage of the nominal 0.9 band at step 8: sampled paths {covered:.4f}, point path {point_covered:.4f}")
    assert 0.84 <= covered <= 0.96
    assert point_covered < 0.6


@pytest.mark.parametrize("frozen", (False, True))
def test_live_scenarios_are_rolling_scenarios_of_the_head_window(frozen):
    from stemgnn_amd import LiveForecaster, trainer
    model, x, _, graph = e2e()
    kw = dict(adjacency=graph) if frozen else {}
    live = LiveForecaster(model, W_E, 7, history=4, **kw)
    rng = np.random.default_rng(SEED + 3)
    live.push(rng.normal(size=(W_E + 2, N_E)))
    before = live.forecast()
    slab, origins = live.out_forecast.clone(), list(live._origins)
    live.seed = 21
    bands, paths = live.scenarios(paths=8, return_paths=True)
    assert bands.shape == (3, 7, N_E) and paths.shape == (8, 7, N_E)
    window = torch.cat([live.ring_x[(live.rows - W_E + i) % live.C][None] for i in range(W_E)])[None].contiguous()
    want_b, _, want_p = trainer.rolling_scenarios(model, [(window, torch.zeros(1, 7, N_E, device=DEV))], 7, paths=8, seed=21,
                                                  origin=live.rows, return_paths=True, **kw)
    assert tsame(bands, want_b[0]) and tsame(paths, want_p[0])
    assert tsame(live.scenarios(paths=8, seed=21), bands) and not tsame(live.scenarios(paths=8, seed=22), bands)
    short = live.scenarios(paths=8, horizon=3)                    # another horizon than the forecaster's: the model's own rows
    assert tsame(short, before[:, :3])
    # nothing of the serving state moved
    assert tsame(live.out_forecast, slab) and live._origins == origins
    assert tsame(live.forecast(), before)
