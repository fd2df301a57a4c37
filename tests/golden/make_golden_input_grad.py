"""Generate the input-gradient fixtures from the REAL reference (run where the reference exists).

    python tests/golden/make_golden_input_grad.py

For every case of tests/golden/make_golden.py (same inputs, deterministic weights and fixed dropout mask), runs the
reference's forward + MSE backward with ``x.requires_grad_(True)`` and writes tests/golden/input_grad/<case>.npz:
x, y, cfg and ``x_grad`` -- the gradient plain autograd leaves in ``x.grad`` (models/base_model.py: the GRU input at :137,
block 0's input at :169).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle.detrand import det_normalish, det_uniform  # noqa: E402
from oracle.ref_shim import load_reference_model_module  # noqa: E402
from oracle.stemgnn_oracle import det_state_dict  # noqa: E402
from tests.golden.make_golden import CASES, hash_seed  # noqa: E402

OUT = os.path.join(HERE, "input_grad")


def run_case(name, c, ref):
    torch.manual_seed(0)
    N, W, m, H, B = c["N"], c["W"], c["multi"], c["H"], c["B"]
    p = 0.5 if c["mode"] == "mask" else 0.0
    model = ref.Model(N, 2, W, m, horizon=H, dropout_rate=p)
    missing = model.load_state_dict(det_state_dict(N, W, m, H, seed=hash_seed(name)), strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    x = torch.from_numpy(det_normalish((B, W, N), 7 + hash_seed(name)))
    y = torch.from_numpy(det_normalish((B, H, N), 11 + hash_seed(name)))
    out = {"x": x.numpy().copy(), "y": y.numpy()}
    model.eval() if c["mode"] == "eval" else model.train()
    if c["mode"] == "mask":
        mask = (det_uniform((B, N, N), 13 + hash_seed(name), 0.0, 1.0) >= p).astype(np.float32)
        out["drop_mask"] = mask
        tm = torch.from_numpy(mask)

        class FixedMask(torch.nn.Module):                  # stands in for nn.Dropout's Bernoulli draw (:161)
            def forward(self, t):
                return t * tm / (1.0 - p)

        model.dropout = FixedMask()
    x.requires_grad_(True)
    forecast, _ = model(x)
    loss = torch.nn.functional.mse_loss(forecast, y)
    loss.backward()
    out["x_grad"] = x.grad.detach().numpy()
    out["loss"] = np.float64(loss.item())
    out["cfg"] = np.array([N, W, m, H, B, {"eval": 0, "train": 1, "mask": 2}[c["mode"]]], np.int64)
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: loss={loss.item():.6f} |x.grad|max={x.grad.abs().max():.3e} size={os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    ref = load_reference_model_module()
    for name, c in CASES.items():
        run_case(name, c, ref)
