"""Shared helpers for the test-suite (test infrastructure)."""
import glob
import os

import numpy as np
import torch

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def hash_seed(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 9973


def load_golden(name):
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    N, W, m, H, B, mode = (int(v) for v in z["cfg"])
    cfg = dict(N=N, W=W, multi=m, H=H, B=B, mode={0: "eval", 1: "train", 2: "mask"}[mode])
    return z, cfg


def relerr(got, ref):
    """norm-relative error used throughout: max|got-ref| / max|ref|."""
    got = torch.as_tensor(got).double().cpu()
    ref = torch.as_tensor(ref).double().cpu()
    den = ref.abs().max().item()
    num = (got - ref).abs().max().item()
    return num / den if den > 0 else num


def sign_sketch(a, k=64, seed=7):
    """k random +-1 projections of a flattened tensor (float64), the signs from oracle/detrand.py.  For a difference d
    of two tensors, mean(sketch(d)^2) estimates ||d||_2^2 without bias, and with k = 64 it falls below a quarter of it
    with negligible probability -- so a fixture can pin a large tensor through k numbers (||d||_inf <= ||d||_2)."""
    from oracle.detrand import det_uniform
    flat = torch.as_tensor(a).double().reshape(-1).numpy()
    signs = np.where(det_uniform((k, flat.size), seed) >= 0, 1.0, -1.0)
    return signs @ flat


def synthetic_series(T, N, seed):
    """sin(2 pi t / p_n + phi_n) * a_n + c_n + noise (SURVEY 8d shape), float64, from the deterministic generators of
    oracle/detrand.py (so a fixture can name a seed instead of carrying the series)."""
    from oracle.detrand import det_normalish, det_uniform
    t = np.arange(T, dtype=np.float64)[:, None]
    p = det_uniform((N,), seed, 6.0, 30.0).astype(np.float64)
    phi = det_uniform((N,), seed + 1, 0.0, 6.28).astype(np.float64)
    a = det_uniform((N,), seed + 2, 0.5, 3.0).astype(np.float64)
    c = det_uniform((N,), seed + 3, -2.0, 8.0).astype(np.float64)
    return np.sin(2 * np.pi * t / p + phi) * a + c + 0.1 * det_normalish((T, N), seed + 4).astype(np.float64)


def kink_audit(pos_impl, ref64, err, what):
    """LeakyReLU-kink audit of one set of pre-activations: `pos_impl` the implementation's decisions (which side of 0 it took
    each value to be on), `ref64` the fp64 oracle's values, `err` the implementation's measured (rounding-class) evaluation
    error of them.  A value is "near the kink" when it is smaller than twice that error; the decisions may differ from the
    fp64 ones on at most a handful of values, and only near the kink.  Returns the flips (where they differ)."""
    ref64 = ref64.double().cpu()
    pos_impl = pos_impl.cpu()
    near = ref64.abs() <= 2 * err
    flips = pos_impl != (ref64 > 0)
    n_near, n_flip = int(near.sum()), int(flips.sum())
    print(f"kink audit ({what}): fp32 error {err:.2e}; {n_near} of {ref64.numel()} values within twice that of 0, "
          f"{n_flip} decision flips")
    assert n_near <= max(16, int(2e-5 * ref64.numel())), n_near
    assert n_flip <= max(8, int(5e-7 * ref64.numel())) and bool((flips & ~near).sum() == 0), (n_flip, int((flips & ~near).sum()))
    return flips
