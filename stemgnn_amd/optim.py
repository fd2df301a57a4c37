"""Fused optimizer step for the reference driver's training loop.

The reference trains with ``torch.optim.RMSprop(params, lr, eps=1e-8)`` (models/handler.py:127) and calls
``model.zero_grad()`` / ``optim.step()`` every batch (:160,:165): ~70 small tensors, i.e. a launch-bound cloud of
tiny kernels.  ``FusedRMSprop`` keeps ALL parameters, gradients and the running square average in three flat
buffers and performs the step -- and the zeroing of the gradients for the next step -- in ONE HIP kernel
(``stemgnn_rmsprop_step``).  Same arithmetic as torch.optim.RMSprop(momentum=0, centered=False, weight_decay=0).

Three opt-in controls, computed on the device inside the (captured) step -- between backward and update there is no host
code that could look at a gradient:
  ``max_grad_norm``   ``torch.nn.utils.clip_grad_norm_(params, max_grad_norm)`` on the gradient the kernel applies, i.e. AFTER
                      ``grad_scale`` (the averaged gradient of a data-parallel run): one extra launch (``stemgnn_grad_sqsum``)
  ``weight_decay``    torch's coupled L2 term, added after the clipping; ``decoupled_weight_decay`` (FusedAdam) = AdamW
  ``skip_nonfinite``  a step whose gradient norm is inf / NaN leaves parameters, moments and Adam's step count untouched
With all three at their defaults ``step()`` calls the same entry points as before (same launches, same bits); otherwise
``stemgnn_*_step_ext`` (csrc/optim.hip).  ``grad_report()`` reads the norm / coefficient / counters the kernel keeps;
``state_dict()`` / ``load_state_dict()`` carry the flat state (moments, step count, counters, lr) for a resumed run.
"""
import torch

from . import _lib
from .distributed import FlatGradBucket


class FusedRMSprop(torch.optim.Optimizer):
    _flat_state = ("square_avg", "stats")     # device buffers state_dict() carries besides the param group

    def __init__(self, params, lr=1e-2, alpha=0.99, eps=1e-8, bucket=None, fuse_zero_grad=True, weight_decay=0.0,
                 max_grad_norm=None, skip_nonfinite=False):
        params = [p for p in params if p.requires_grad]
        if not float(weight_decay) >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if max_grad_norm is not None and not float(max_grad_norm) > 0.0:
            raise ValueError(f"Invalid max_grad_norm value: {max_grad_norm} (a positive norm, or None for no clipping)")
        super().__init__(params, dict(lr=lr, alpha=alpha, eps=eps, weight_decay=float(weight_decay),
                                      max_grad_norm=None if max_grad_norm is None else float(max_grad_norm),
                                      skip_nonfinite=bool(skip_nonfinite)))
        if not params or not params[0].is_cuda:
            raise _lib.StemGNNHipError("FusedRMSprop needs parameters on a HIP device (move the model first)")
        dev = params[0].device
        self._params = params
        self.numel = sum(p.numel() for p in params)
        self.flat_p = torch.empty(self.numel, device=dev, dtype=torch.float32)
        off = 0
        for p in params:                      # re-point every parameter at its slice of the flat buffer
            n = p.numel()
            view = self.flat_p[off:off + n].view_as(p)
            view.copy_(p.data)
            p.data = view
            off += n
        self.bucket = bucket if bucket is not None else FlatGradBucket(params)
        if self.bucket.numel != self.numel:
            raise ValueError("gradient bucket and parameter list differ")
        self.square_avg = torch.zeros_like(self.flat_p)
        self._lr_host = float(lr)
        self._lr_dev = torch.tensor([lr], device=dev, dtype=torch.float32)
        self.fuse_zero_grad = bool(fuse_zero_grad)
        self.grad_scale = 1.0      # applied to every gradient inside the kernel (1 / world after a SUM all-reduce)
        # the controls' device state, allocated here so that step() is capture-safe: the norm kernel's fp64 partial sums and
        # {norm, coefficient, clipped steps, skipped steps} of include/stemgnn_hip.h
        self._partials = torch.zeros(int(_lib.load().stemgnn_grad_norm_partials(self.numel)), device=dev, dtype=torch.float64)
        self.stats = torch.zeros(4, device=dev, dtype=torch.float64)

    def _controls(self):
        """(weight_decay, max_norm for the kernel (<= 0: none), skip_nonfinite, a norm is needed, any control enabled)"""
        group = self.param_groups[0]
        wd = float(group.get("weight_decay", 0.0))
        mn = group.get("max_grad_norm")
        mn = 0.0 if mn is None else float(mn)
        if not wd >= 0.0 or (group.get("max_grad_norm") is not None and not mn > 0.0):
            raise ValueError("weight_decay must not be negative and max_grad_norm must be positive (None: no clipping)")
        skip = bool(group.get("skip_nonfinite", False))
        need_norm = mn > 0.0 or skip
        return wd, mn, skip, need_norm, (need_norm or wd != 0.0)

    @property
    def controls_enabled(self):
        return self._controls()[4]

    def _grad_sqsum(self, lib, stream):
        _lib.check(lib.stemgnn_grad_sqsum(self.bucket.flat.data_ptr(), self.numel, float(self.grad_scale),
                                          self._partials.data_ptr(), stream), "grad_sqsum")

    def grad_report(self, reset=False):
        """What the controls did, with one host sync: the last step's pre-clip gradient norm (NaN when no norm is taken:
        weight decay alone) and coefficient (1 not clipped, 0 skipped), and the running counts of clipped and of skipped
        steps (reset=True zeroes the two counts)."""
        norm, coef, clipped, skipped = self.stats.tolist()
        if reset:
            self.stats[2:].zero_()
        return {"norm": norm, "coef": coef, "clipped_steps": int(clipped), "skipped_steps": int(skipped)}

    def state_dict(self):
        """torch's dict (the param group with the controls and the current lr; per-parameter state is empty: the moments
        are flat) plus ``flat``: copies of the flat state buffers, so a resumed run continues the moments, Adam's step count
        and the counters instead of restarting them at zero."""
        sd = super().state_dict()
        sd["flat"] = {name: getattr(self, name).detach().clone() for name in self._flat_state}
        sd["flat"]["lr"] = float(self.param_groups[0]["lr"])
        return sd

    def load_state_dict(self, state_dict):
        flat = state_dict.get("flat")
        if flat is None:
            raise _lib.StemGNNHipError(f"{type(self).__name__}.load_state_dict: no 'flat' state (not a state_dict of a fused "
                                       "optimizer)")
        for name in self._flat_state:
            if name not in flat or flat[name].shape != getattr(self, name).shape:
                raise ValueError(f"{type(self).__name__}.load_state_dict: flat state '{name}' is missing or has another size")
        super().load_state_dict({k: v for k, v in state_dict.items() if k != "flat"})
        with torch.no_grad():
            for name in self._flat_state:       # into the existing buffers: parameters stay views of flat_p, graphs stay valid
                getattr(self, name).copy_(flat[name])
        self.param_groups[0]["lr"] = float(flat["lr"])
        self.sync_lr()

    def zero_grad(self, set_to_none=False):   # gradients live in the flat bucket; never drop the views
        self.bucket.zero()

    def _check_grad_views(self):
        """The step reads the FLAT gradient buffer: every p.grad must still be its view (torch's default
        model.zero_grad(set_to_none=True) drops them -> backward would fill fresh tensors and the step would see zeros).
        Object identity first (what attach() stored; a handful of ns per parameter on the launch-bound eager path), the
        device-pointer comparison only for a .grad someone replaced."""
        for p, view in zip(self.bucket.params, self.bucket.views):
            g = p.grad
            if g is view:
                continue
            if g is None or g.data_ptr() != view.data_ptr():
                raise _lib.StemGNNHipError(
                    f"{type(self).__name__}: a parameter's .grad is no longer the flat-bucket view (model.zero_grad() with "
                    "set_to_none=True?).  Use optimizer.zero_grad() / model.zero_grad(set_to_none=False), or call "
                    "optimizer.bucket.attach() before backward.")

    def sync_lr(self):
        """Push a learning rate an LR scheduler changed (host side) to the device word the kernel reads.  step() calls
        it; a hipGraph replay does not run step()'s Python, so engine.TrainStep calls it before every replay."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_host:
            self._lr_host = lr
            self._lr_dev.fill_(lr)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        group = self.param_groups[0]
        self.sync_lr()
        from .ops import join_side_streams
        join_side_streams(self.flat_p.device)
        self._check_grad_views()
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        wd, max_norm, skip, need_norm, enabled = self._controls()
        if not enabled:
            _lib.check(lib.stemgnn_rmsprop_step(
                self.flat_p.data_ptr(), self.bucket.flat.data_ptr(), self.square_avg.data_ptr(), self.numel,
                self._lr_dev.data_ptr(), float(group["alpha"]), float(group["eps"]), int(self.fuse_zero_grad),
                float(self.grad_scale), stream), "rmsprop_step")
            return loss
        if need_norm:
            self._grad_sqsum(lib, stream)
        _lib.check(lib.stemgnn_rmsprop_step_ext(
            self.flat_p.data_ptr(), self.bucket.flat.data_ptr(), self.square_avg.data_ptr(), self.numel,
            self._lr_dev.data_ptr(), float(group["alpha"]), float(group["eps"]), int(self.fuse_zero_grad),
            float(self.grad_scale), wd, max_norm, int(skip), self._partials.data_ptr() if need_norm else None,
            self.stats.data_ptr(), stream), "rmsprop_step_ext")
        return loss


class FusedAdam(FusedRMSprop):
    """``torch.optim.Adam(params, lr, betas=(0.9, 0.999))`` of the driver's other optimizer branch (models/handler.py:128-129)
    over the same flat buffers as FusedRMSprop: one kernel (+ a one-thread step-count tick), gradient zeroing fused in,
    lr and the step count in device memory -- so an Adam run keeps the hipGraph train step too."""

    _flat_state = ("square_avg", "exp_avg", "_step_dev", "stats")     # square_avg is exp_avg_sq

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, bucket=None, fuse_zero_grad=True, weight_decay=0.0,
                 decoupled_weight_decay=False, max_grad_norm=None, skip_nonfinite=False):
        params = [p for p in params if p.requires_grad]
        FusedRMSprop.__init__(self, params, lr=lr, alpha=0.0, eps=eps, bucket=bucket, fuse_zero_grad=fuse_zero_grad,
                              weight_decay=weight_decay, max_grad_norm=max_grad_norm, skip_nonfinite=skip_nonfinite)
        self.param_groups[0]["betas"] = tuple(betas)
        self.param_groups[0]["decoupled_weight_decay"] = bool(decoupled_weight_decay)
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = self.square_avg                       # reuse the second flat state buffer
        self._step_dev = torch.zeros(1, device=self.flat_p.device, dtype=torch.float32)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        group = self.param_groups[0]
        self.sync_lr()
        from .ops import join_side_streams
        join_side_streams(self.flat_p.device)
        self._check_grad_views()
        b1, b2 = group["betas"]
        lib = _lib.load()
        stream = torch.cuda.current_stream().cuda_stream
        wd, max_norm, skip, need_norm, enabled = self._controls()
        if not enabled:
            _lib.check(lib.stemgnn_adam_step(
                self.flat_p.data_ptr(), self.bucket.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                self.numel, self._lr_dev.data_ptr(), self._step_dev.data_ptr(), float(b1), float(b2), float(group["eps"]),
                int(self.fuse_zero_grad), float(self.grad_scale), stream), "adam_step")
            return loss
        if need_norm:
            self._grad_sqsum(lib, stream)
        _lib.check(lib.stemgnn_adam_step_ext(
            self.flat_p.data_ptr(), self.bucket.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
            self.numel, self._lr_dev.data_ptr(), self._step_dev.data_ptr(), float(b1), float(b2), float(group["eps"]),
            int(self.fuse_zero_grad), float(self.grad_scale), wd, int(bool(group.get("decoupled_weight_decay", False))),
            max_norm, int(skip), self._partials.data_ptr() if need_norm else None, self.stats.data_ptr(), stream),
            "adam_step_ext")
        return loss
