"""Model at the PEMS07 shape on fixed inputs, for the switches the library reads once per process (static ... getenv): run as
a fresh subprocess per switch value by tests/test_hip_shape_domain.py.  One forward + backward through Model, then two
TrainStep steps (the second a replay of the captured graph); saves x, y, forecast, attention, every gradient and the updated
parameters to the .npz named by argv[1], and prints one JSON line with SHA-256 digests of the same arrays."""
import hashlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

N, W, MULTI, H, B = 228, 12, 5, 3, 32


def main():
    from oracle import stemgnn_oracle as O
    from stemgnn_amd import Model, ops
    from stemgnn_amd.engine import TrainStep
    from stemgnn_amd.optim import FusedRMSprop

    dev = torch.device("cuda:0")
    sd = O.det_state_dict(N, W, MULTI, H, seed=1)
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(B, W, N, generator=g), torch.randn(B, H, N, generator=g)
    model = Model(N, 2, W, MULTI, horizon=H, dropout_rate=0.0)
    model.load_state_dict(sd)
    model.to(dev).train()
    forecast, att = model(x.to(dev))
    torch.nn.functional.mse_loss(forecast, y.to(dev)).backward()
    torch.cuda.synchronize()
    ops.check_gru_status(dev)
    arrays = {"x": x.numpy(), "y": y.numpy(), "forecast": forecast.detach().cpu().numpy(),
              "attention": att.detach().cpu().numpy()}
    for k, p in model.named_parameters():
        if p.grad is not None:
            arrays["grad." + k] = p.grad.cpu().numpy()
    # one captured train step: the eager first step captures, the second replays the graph
    model.zero_grad(set_to_none=True)
    opt = FusedRMSprop(model.parameters(), lr=1e-3, eps=1e-8)
    T = 120
    series = torch.randn(T, N, generator=g).to(dev)
    hi = (torch.randint(0, T - W - H, (2 * B,), generator=g) + W).to(dev)
    step = TrainStep(model, opt, B, W, H, N, series=series, order_capacity=2 * B, schedule_check=False)
    step.load_order(hi)
    losses = []
    for _ in range(2):
        step.run_next()
        losses.append(float(step.loss))
    torch.cuda.synchronize()
    ops.check_gru_status(dev)
    assert step.mode.startswith("hipgraph"), step.mode
    arrays["losses"] = np.asarray(losses, dtype=np.float32)
    for k, p in model.named_parameters():
        arrays["param." + k] = p.detach().cpu().numpy()
    np.savez(sys.argv[1], **arrays)
    digests = {k: hashlib.sha256(np.ascontiguousarray(v).tobytes()).hexdigest() for k, v in arrays.items()}
    print(json.dumps({"mode": step.mode, "digests": digests}))


if __name__ == "__main__":
    main()
