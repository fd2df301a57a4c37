"""Host-side composition of the HIP stages into one autograd function.

PyTorch is plumbing here: it owns device memory (torch.empty), the current HIP stream and the
autograd graph; every number on the hot path is produced by libstemgnn_hip.so.

Stage order (reference models/base_model.py): attention+Laplacian (:139-147) -> Chebyshev (:148)
-> per StockBlock: pack, GFT (:62-64), spectral GLU (:46-54), IGFT+heads (:55-58, :65-74).
"""
import ctypes
import os
import weakref

import numpy as np
import torch

from . import _lib

_NSPLIT = 32      # split-M factor of the slab weight-gradient GEMMs (heads' BS product; GLU only on the fallback path)
_side_streams = {}


def _side_stream(device, index=0):
    key = (str(device), index)
    st = _side_streams.get(key)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _side_streams[key] = st
    return st


def fresh_side_stream(device, index=0):
    """Replace the side stream of `device` by a newly created one (engine.TrainStep's schedule self-check: a re-capture
    after a lost branch overlap gives the runtime another stream -> hardware-queue mapping to work with).  The caller
    guarantees that nothing is pending on the old one (device synchronised)."""
    _side_streams.pop((str(device), index), None)
    return _side_stream(device, index)


class HotPathState:
    """Per-model scheduling state of the hot path (one instance per ``stemgnn_amd.Model``; nothing process-global).

    direct : backward WRITES the hot-path / GRU / fc parameter gradients straight into existing ``p.grad`` buffers
             (e.g. the views of a FlatGradBucket) instead of returning them to autograd, which would launch one
             accumulate kernel per parameter (~70 tiny launches per step).  Semantics: overwrite, i.e. equivalent to
             ``zero_grad(); backward()`` -- not for accumulating gradients over several backward passes.
    overlap: additionally queue the spectral blocks' weight-gradient GEMMs (and the weight packing / dropout-stream
             bookkeeping of the forward) on a side HIP stream so they overlap the rest of the step (notably the
             latency-bound GRU recurrence).  Gradients are then complete only after ``join_side_streams()``;
             FusedRMSprop.step, FlatGradBucket.all_reduce_mean and GruFront.backward call it -- any other reader of
             ``.grad`` must call it first.
    """

    def __init__(self):
        self.direct = False
        self.overlap = False
        self.prepacked = None        # (packed panels, side stream, blocks) queued by prepack_blocks
        self.preseed = None          # dropout key of the coming forward, cloned on the side stream (Model.prefetch_side)
        self.fork_event = None       # optional event the next prepack_blocks forks the side stream from
        self.pending = None          # (side stream, keep-alive objects) of weight-gradient work not yet joined
        self.exact_group = None      # data-parallel "exact mode" (SURVEY 8e-ii): (process group, world size) or None
        self.gru_front_live = False  # set by Model.hot_path when the GRU output it hands to SpectralHotPath came from GruFront
        self.dh_factors = None       # (attn scratch, B, N, wk, wq): the factored d(loss)/d(GRU output) SpectralHotPath.backward left
                                     # for GruFront.backward (stemgnn_gru_bwd_rank2) instead of a materialised [N,B,N] tensor
        self.block_grads_hook = None # callable run on the side stream right behind block 1's un-packing (overlap mode): the
                                     # step driver's all-reduce of the block / fc gradient range (engine.TrainStep)
        self.gru_ctl = None          # int32 control words of the GRU's dW_hh product beside the recurrence (stemgnn_gru_bwd_rank2_begin
        self.gru_ctl_zeroed = False  # / _finish); True: zeroed on the side stream by this backward pass, ahead of both streams' use
        self.warm_saved = None       # dummy saved-activation buffer of the fused forward's warm-up launch (prepack_blocks)
        self.tail_finish = None      # thunk(stream): the fc tail's partial-sum launch (loss, fc gradients) FcTailMse.forward left for
                                     # SpectralHotPath.backward to queue on the side branch (nothing on the chain reads its output)
        self.tail_may_defer = True   # False while Model.loss runs from a given adjacency: no SpectralHotPath.backward will come
                                     # for the thunk, FcTailMse.forward runs both launches itself
        self.side_probe = None       # a list: every kernel the step would put on the SIDE branch is also appended as a
                                     # re-issuable thunk(stream) -- engine.TrainStep's schedule self-check replays them alone to
                                     # measure the side branch's kernel-time sum (collectives and the dropout key step excluded)
        _states.add(self)

    def set(self, direct=True, overlap=False):
        self.direct = bool(direct)
        self.overlap = bool(direct) and bool(overlap)
        return self

    def join(self):
        item, self.pending = self.pending, None
        if item is not None:
            side, keep = item
            torch.cuda.current_stream().wait_stream(side)
            del keep

    def reset(self):
        """Drop queued side-stream work after a failed capture / aborted step (engine.capture)."""
        for item in (self.prepacked, self.pending):
            if item is not None:
                try:        # the stream may have been forked into the capture that just failed (invalidated capture)
                    (item[1] if item is self.prepacked else item[0]).synchronize()
                except RuntimeError:
                    pass    # engine.capture synchronizes the device afterwards anyway
        self.prepacked = None
        self.preseed = None
        self.fork_event = None
        self.pending = None
        self.dh_factors = None
        self.gru_ctl_zeroed = False
        self.tail_finish = None


_states = weakref.WeakSet()
_NO_STATE = None


def _state(state):
    """Functions called without a model (stand-alone use, tests): a shared inert state (no direct writes, no overlap)."""
    global _NO_STATE
    if state is not None:
        return state
    if _NO_STATE is None:
        _NO_STATE = HotPathState()
    return _NO_STATE


def join_side_streams(device=None):
    """Make the current stream wait for weight-gradient work any model queued on a side stream (see
    SpectralHotPath.backward).  Called by every consumer of the gradients; cheap no-op when nothing is pending."""
    for st in list(_states):
        if st.pending is not None and (device is None or str(st.pending[0].device) == str(torch.device(device))):
            st.join()


def _all_reduce_mean(t, group_world):
    """Mean of `t` over the ranks of (group, world[, stand-in]) on the current stream.  The optional third entry is an
    in-stream stand-in fn(view) for the SUM all-reduce (schedule tests on a 1-GPU box, see FlatGradBucket.reduce_fn)."""
    group, world = group_world[0], group_world[1]
    fn = group_world[2] if len(group_world) > 2 else None
    if fn is not None:
        fn(t)
    else:
        import torch.distributed as dist
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    t.div_(world)


def set_direct_grad(model, flag=True, overlap=False):
    """Switch ``model`` (a stemgnn_amd.Model) to direct-gradient mode, see HotPathState."""
    return model.hot_state.set(flag, overlap)


_NCHUNK = 16      # row chunks of the attention backward


def _wg_cu(which, B, N):
    """CU share (percent) of the side stream's first / second fused weight-gradient launch.  The first runs beside the
    Chebyshev / attention backward chain and is sized for (nearly) the whole chip (round 4: 80 / 65 % measured 0 / +18 us per
    step; round 5: see below); the second
    runs under the GRU backward recurrence, which pins stemgnn_gru_bwd_cus(B, N) CUs for its whole run, and is sized for
    what is left (50 % at PEMS07 where 4 workgroups serve a batch row, 25 % at N = 358 with 6; hidden sizes of the wide
    cluster keep 50)."""
    if which == 0:
        # round 5, with the 256 x 64 tiles (33 instead of 37 tiles per launch): 100 % would give 7 splits = 231 workgroups and
        # starves the backward chain beside it (ChebBwd 17 + 21 -> 30 + 42 us; step 1.142 ms against 1.122 at 90 % = 6 splits,
        # 198 workgroups; 80 % 1.122; the 128 x 128-only build 1.125 -- same box, profiles/r05_wgrad_tiles_ab.txt)
        return 90
    if N > 512:          # wide cluster (hidden > 512): the weight-gradient work there exceeds what the idle CUs could do in
        return 50        # the recurrence's time -- the round-2/3 setting (half of the chip, sharing CUs with the cluster) stays
    lib = _lib.load()
    cus = lib.stemgnn_num_cus()
    busy = lib.stemgnn_gru_bwd_cus(B, N)
    return max(10, min(100, (cus - busy) * 100 // cus))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def glu_splits():
    """Arithmetic of the GLU forward / data-gradient layers inside the model (STEMGNN_DTYPE): 0 = exact fp32 MFMA (default,
    the reference's arithmetic), 3 / 2 = split-bf16 products (bf16x3: fp32-class; bf16x2: ~2^-16 relative) on the bf16
    matrix instructions with fp32 accumulation (csrc/gemm2s.h).  Read per call, so a test can switch it."""
    v = os.environ.get("STEMGNN_DTYPE", "f32").lower()
    if v in ("f32", "fp32", ""):
        return 0
    if v == "bf16x3":
        return 3
    if v == "bf16x2":
        return 2
    raise _lib.StemGNNHipError(f"STEMGNN_DTYPE={v!r}: expected f32, bf16x3 or bf16x2")


def _pack_block(lib, parr, tables, pk, W, multi, splits, stream):
    """Pack one block's weights for the arithmetic the GLU products will run in: exact fp32 -> panels + the fp32 stage streams of
    the fused kernels (stemgnn_block_pack); split-bf16 -> the panels only (stemgnn_block_pack_panels; _split_panels packs the
    bf16 streams from them and nothing reads the fp32 streams: two dead launches and ~35 MB of writes per step in round 5)."""
    if splits:
        _lib.check(lib.stemgnn_block_pack_panels(parr, tables.data_ptr(), pk.data_ptr(), W, multi, stream), "block_pack_panels")
    else:
        _lib.check(lib.stemgnn_block_pack(parr, tables.data_ptr(), pk.data_ptr(), W, multi, stream), "block_pack")


def _split_panels(lib, pk, W, multi, splits, device, stream):
    sp = torch.empty(lib.stemgnn_glu_split_floats(W, multi, splits), device=device, dtype=torch.float32)
    _lib.check(lib.stemgnn_glu_split_panels(pk.data_ptr(), sp.data_ptr(), W, multi, splits, stream), "glu_split_panels")
    return sp


def _require_gpu(t, name):
    if not t.is_cuda:
        raise _lib.StemGNNHipError(
            f"{name} is on {t.device}: stemgnn_amd runs only on a HIP device (no CPU fallback)")
    if t.dtype != torch.float32:
        raise _lib.StemGNNHipError(f"{name} must be float32, got {t.dtype}")


_table_cache = {}


def dft_tables(W, multi, device):
    """Constant DFT / C2R tables for (W, multi), built once on the host by the library."""
    key = (W, multi, str(device))
    t = _table_cache.get(key)
    if t is None:
        lib = _lib.load()
        n = lib.stemgnn_table_floats(W, multi)
        host = torch.empty(n, dtype=torch.float32)
        _lib.check(lib.stemgnn_make_tables_host(W, multi, host.data_ptr()), "make_tables_host")
        t = host.to(device)
        _table_cache[key] = t
    return t


def dropout_mask(drop_p, seed, B, N):
    """Test hook: the 0/1 keep mask [B,N,N] the attention kernels regenerate from `seed` (uint64[2])."""
    lib = _lib.load()
    mask = torch.empty(B, N, N, device=seed.device, dtype=torch.float32)
    _lib.check(lib.stemgnn_dropout_mask(float(drop_p), seed.data_ptr(), B, N, mask.data_ptr(), _stream()),
               "dropout_mask")
    return mask


_gru_status = {}


def gru_status(device):
    """Device int32 the cluster GRU kernels set to 1 if an inter-workgroup wait timed out (never expected)."""
    key = str(device)
    t = _gru_status.get(key)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=device)
        _gru_status[key] = t
    return t


def gru_status_exists(device):
    """True once a GRU kernel has been launched on `device` (the status word is created by the first launch)."""
    return str(device) in _gru_status


def check_eigh_status(device=None):
    """Host sync + raise if the direct eigensolver flagged a run on `device` (STEMGNN_SPECTRAL=eig only).  The library
    keeps one status word per device and clears it when it is read, so an event is reported once."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        rc = _lib.load().stemgnn_eigh_status()
    if rc == 2:
        raise _lib.StemGNNHipError(f"eigensolver status 2 on {dev}: a grid-barrier wait of the tridiagonalisation timed "
                                   "out (a workgroup of its cluster was not resident)")
    if rc == 3:
        raise _lib.StemGNNHipError(f"eigensolver status 3 on {dev}: the re-solve of an eigenvalue cluster broke down "
                                   "(no independent start vector left)")
    if rc != 0:
        raise _lib.StemGNNHipError(f"eigensolver status {rc} on {dev}")


def check_gru_status(device):
    """Host sync + raise if a GRU exchange timed out (call outside timed regions / in tests)."""
    st = gru_status(device)
    if int(st.item()) != 0:
        st.zero_()                               # report once; the next check sees only new time-outs
        raise _lib.StemGNNHipError("GRU cluster exchange timed out (partner workgroup not resident?); "
                                   "set STEMGNN_GRU_CLUSTER=0 to use the single-workgroup kernels")


class GruFront(torch.autograd.Function):
    """nn.GRU(time_step, units) over the node axis (reference models/base_model.py:137) as two persistent HIP
    recurrence kernels.  (x [B,W,N], weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0) -> h [N,B,N]."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, state=None):
        lib = _lib.load()
        ctx.state = _state(state)
        gru_params = (w_ih, w_hh, b_ih, b_hh)
        for name, t in (("x", x), ("GRU.weight_ih_l0", w_ih), ("GRU.weight_hh_l0", w_hh)):
            _require_gpu(t, name)
        x = x.contiguous()
        B, W, S = x.shape
        Hd = w_hh.shape[1]
        dev, f32 = x.device, torch.float32
        w_ih, w_hh, b_ih, b_hh = (t.contiguous() for t in (w_ih, w_hh, b_ih, b_hh))
        h_ext = torch.empty(S + 1, B, Hd, device=dev, dtype=f32)     # slab 0 = h_{-1} = 0 (set by the library)
        h_all = h_ext[1:]                                             # exactly nn.GRU's output, a contiguous view
        reserve = torch.empty(lib.stemgnn_gru_reserve_floats(B, S, Hd), device=dev, dtype=f32)
        scratch = torch.empty(lib.stemgnn_gru_fwd_scratch_floats(B, S, Hd), device=dev, dtype=f32)
        _lib.check(lib.stemgnn_gru_fwd(x.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(),
                                       B, S, Hd, W, scratch.data_ptr(), h_ext.data_ptr(), reserve.data_ptr(),
                                       gru_status(dev).data_ptr(), _stream()), "gru_fwd")
        # save_for_backward (not ctx attributes): h_all is an OUTPUT -- holding it on ctx would form a
        # ctx <-> grad_fn reference cycle that never frees the step's buffers
        ctx.save_for_backward(x, w_ih, w_hh, h_ext, reserve)
        ctx.gru_params = gru_params
        return h_all

    @staticmethod
    def backward(ctx, dh_all):
        lib = _lib.load()
        x, w_ih, w_hh, h_ext, reserve = ctx.saved_tensors
        B, W, S = x.shape
        Hd = w_hh.shape[1]
        dev, f32 = x.device, torch.float32
        factors, ctx.state.dh_factors = ctx.state.dh_factors, None
        if factors is None:
            dh_all = dh_all.contiguous()
        scratch = torch.empty(lib.stemgnn_gru_bwd_scratch_floats(B, S, Hd, W), device=dev, dtype=f32)
        prm = ctx.gru_params
        # frozen GRU (no parameter needs a gradient): the recurrence alone (stemgnn_gru_bwd_recur / _rank2_recur) -- its gate
        # gradients are all the input gradient below needs
        frozen = not any(ctx.needs_input_grad[1:5])
        direct = not frozen and ctx.state.direct and all(p.grad is not None and p.grad.is_contiguous() for p in prm)
        if direct:
            dw_ih, dw_hh, db_ih, db_hh = (p.grad for p in prm)
        elif not frozen:
            dw_ih, dw_hh = torch.empty_like(w_ih), torch.empty_like(w_hh)
            db_ih = torch.empty(3 * Hd, device=dev, dtype=f32)
            db_hh = torch.empty(3 * Hd, device=dev, dtype=f32)
        if frozen:
            if factors is not None:
                attn_scratch, fb, fn, wk, wq, after, dq_chunks = factors
                base = attn_scratch.data_ptr() + 4 * fn * fn
                ctx.state.gru_ctl_zeroed = False
                _lib.check(lib.stemgnn_gru_bwd_rank2_recur(base, base + 4 * fb * fn, dq_chunks, wk.data_ptr(), wq.data_ptr(),
                                                           x.data_ptr(), w_hh.data_ptr(), h_ext.data_ptr(), reserve.data_ptr(),
                                                           B, S, Hd, W, scratch.data_ptr(), gru_status(dev).data_ptr(),
                                                           _stream()), "gru_bwd_rank2_recur")
                if after is not None:
                    after()             # dwk / dwq on the side stream
            else:
                _lib.check(lib.stemgnn_gru_bwd_recur(dh_all.data_ptr(), x.data_ptr(), w_hh.data_ptr(), h_ext.data_ptr(),
                                                     reserve.data_ptr(), B, S, Hd, W, scratch.data_ptr(),
                                                     gru_status(dev).data_ptr(), _stream()), "gru_bwd_recur")
        elif factors is not None:
            # SpectralHotPath.backward stopped at dkey | dquery: dh[s,b,i] = dkey[b,i] wk[s] + dquery[b,i] wq[s] is formed
            # inside the recurrence (the [N,B,N] gradient tensor is never written; `dh_all` is a zero-stride placeholder)
            attn_scratch, fb, fn, wk, wq, after, dq_chunks = factors
            base = attn_scratch.data_ptr() + 4 * fn * fn
            tail = (x.data_ptr(), w_hh.data_ptr(), h_ext.data_ptr(), reserve.data_ptr(), B, S, Hd, W, scratch.data_ptr(),
                    dw_ih.data_ptr(), dw_hh.data_ptr(), db_ih.data_ptr(), db_hh.data_ptr(), gru_status(dev).data_ptr())
            args = (base, base + 4 * fb * fn, wk.data_ptr(), wq.data_ptr()) + tail
            # overlap mode: the dW_hh product runs on the side stream BESIDE the recurrence (persistent workgroups that follow
            # its progress counters) and only the last few time steps' share + the fixed-order sums stay behind it
            # (include/stemgnn_hip.h: stemgnn_gru_bwd_rank2_begin / _finish; same bits as the single call)
            beside = (ctx.state.overlap and ctx.state.pending is not None and ctx.state.gru_ctl_zeroed
                      and bool(lib.stemgnn_gru_bwd_overlap_ok(B, S, Hd, W))
                      and ctx.state.gru_ctl.numel() == lib.stemgnn_gru_bwd_ctl_words(S))
            ctx.state.gru_ctl_zeroed = False
            ctl = ctx.state.gru_ctl.data_ptr() if beside else None
            if beside:
                _lib.check(lib.stemgnn_gru_bwd_rank2_begin(*args, ctl, _stream()), "gru_bwd_rank2_begin")
            elif dq_chunks:
                # dquery is still the attention backward's per-chunk partials: summed inside this call's zero-fill launch
                # (bf16x2: the dW_hh product on the bf16 matrix pipe as well, like the blocks' weight gradients)
                wg_split = 1 if glu_splits() == 2 and os.environ.get("STEMGNN_WGRAD_BF16", "1") != "0" else 0
                _lib.check(lib.stemgnn_gru_bwd_rank2_dq(base, base + 4 * fb * fn, dq_chunks, wg_split, wk.data_ptr(), wq.data_ptr(),
                                                        *tail, _stream()), "gru_bwd_rank2_dq")
            else:
                _lib.check(lib.stemgnn_gru_bwd_rank2(*args, _stream()), "gru_bwd_rank2")
            if after is not None:
                after()                 # dwk / dwq on the side stream (needs dkey | dquery only)
            if beside:
                # behind dwk / dwq on the side stream (its only parent inside a captured graph: a parent on the main branch
                # would make it wait for the recurrence itself, include/stemgnn_hip.h).  A third stream that starts the
                # followers WITH the recurrence was measured too: they take CUs from block 1's weight gradients, which then
                # end behind the recurrence (+26 us per step; profiles/r05_gru_whh_overlap.md)
                side = ctx.state.pending[0]
                _lib.check(lib.stemgnn_gru_bwd_rank2_finish(*args, ctl, side.cuda_stream, _stream()), "gru_bwd_rank2_finish")
        else:
            _lib.check(lib.stemgnn_gru_bwd(dh_all.data_ptr(), x.data_ptr(), w_hh.data_ptr(), h_ext.data_ptr(),
                                           reserve.data_ptr(), B, S, Hd, W, scratch.data_ptr(), dw_ih.data_ptr(),
                                           dw_hh.data_ptr(), db_ih.data_ptr(), db_hh.data_ptr(),
                                           gru_status(dev).data_ptr(), _stream()), "gru_bwd")
        dx = None
        if ctx.needs_input_grad[0]:
            # x [B,W,S] through the input projection, from the gate gradients the call above left at offset 0 of `scratch`
            dx = torch.empty(B, W, S, device=dev, dtype=f32)
            _lib.check(lib.stemgnn_gru_input_grad(scratch.data_ptr(), w_ih.data_ptr(), B, S, Hd, W, dx.data_ptr(), _stream()),
                       "gru_input_grad")
        ctx.state.join()                # the spectral blocks' weight gradients (side stream) overlapped this recurrence
        if direct or frozen:
            return dx, None, None, None, None, None
        return dx, dw_ih, dw_hh, db_ih, db_hh, None


class FcTail(torch.autograd.Function):
    """fc tail of Model.forward (reference models/base_model.py:175-179): fsum [B,N,W] -> forecast [B,H,N]."""

    @staticmethod
    def forward(ctx, fsum, w0, b0, w2, b2, state=None):
        lib = _lib.load()
        ctx.state = _state(state)
        fsum = fsum.contiguous()
        B, N, W = fsum.shape
        H = w2.shape[0]
        forecast = torch.empty(B, H, N, device=fsum.device, dtype=torch.float32)
        w0, b0, w2, b2 = (t.contiguous() for t in (w0, b0, w2, b2))
        _lib.check(lib.stemgnn_fc_tail_fwd(fsum.data_ptr(), w0.data_ptr(), b0.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                           B, N, W, H, forecast.data_ptr(), _stream()), "fc_tail_fwd")
        ctx.save_for_backward(fsum, w0, b0, w2)
        ctx.fc_params = (w0, b0, w2, b2)
        return forecast

    @staticmethod
    def backward(ctx, dforecast):
        lib = _lib.load()
        fsum, w0, b0, w2 = ctx.saved_tensors
        B, N, W = fsum.shape
        H = w2.shape[0]
        dev, f32 = fsum.device, torch.float32
        dforecast = dforecast.contiguous()
        prm = ctx.fc_params
        direct = ctx.state.direct and all(p.grad is not None and p.grad.is_contiguous() for p in prm)
        if direct:
            dw0, db0, dw2, db2 = (p.grad for p in prm)
        else:
            dw0, db0, dw2, db2 = (torch.empty_like(p) for p in prm)
        dfsum = torch.empty_like(fsum)
        scratch = torch.empty(lib.stemgnn_fc_tail_scratch_floats(B, N, W, H), device=dev, dtype=f32)
        _lib.check(lib.stemgnn_fc_tail_bwd(dforecast.data_ptr(), fsum.data_ptr(), w0.data_ptr(), b0.data_ptr(),
                                           w2.data_ptr(), B, N, W, H, scratch.data_ptr(), dfsum.data_ptr(),
                                           dw0.data_ptr(), db0.data_ptr(), dw2.data_ptr(), db2.data_ptr(), _stream()),
                   "fc_tail_bwd")
        if direct:
            return dfsum, None, None, None, None, None
        return dfsum, dw0, db0, dw2, db2, None


def _fc_tail_train_forward(ctx, fsum, target, prm, H, state, loss_out, accum, unit_grad, ignore_nan, entries):
    """The fused training tail's forward, shared by FcTailMse and FcTailQuantile: the direct / deferred logic exists once.
    prm = (fc.0.weight, fc.0.bias, fc.2.weight, fc.2.bias); H = the target's horizon ([B,H,N]; fc.2 has H rows, or Q * H for a
    quantile head -- the scratch is sized by fc.2's rows).  entries(norm) -> (rows_call, finish_call, both_call, sel, fin_sel):
    the three library entries and the arguments they take between `B, N, W, H` and the scratch (rows / both) or the loss
    (finish); norm = the valid-target count buffer (ignore_nan) or None."""
    lib = _lib.load()
    ctx.state = _state(state)
    _require_gpu(fsum, "fsum")
    _require_gpu(target, "target")
    fsum, target = fsum.contiguous(), target.contiguous()
    B, N, W = fsum.shape
    w0, b0, w2, b2 = prm
    if tuple(target.shape) != (B, H, N):
        raise _lib.StemGNNHipError(f"target must be [B,H,N]=({B},{H},{N}), got {tuple(target.shape)}")
    dev, f32 = fsum.device, torch.float32
    w0c, b0c, w2c, b2c = (t.contiguous() for t in prm)
    # direct writes into p.grad only for a call that WILL be back-propagated with an upstream gradient of 1
    # (unit_grad: the step driver's promise): a logging call under no_grad, or a scaled loss, must not clobber the
    # flat gradient bucket -- those use temporaries that backward scales and returns
    wanted = any(ctx.needs_input_grad[i] for i in (0, 2, 3, 4, 5))
    direct = ctx.state.direct and bool(unit_grad) and wanted and \
        all(p.grad is not None and p.grad.is_contiguous() for p in prm)
    grads = [p.grad for p in prm] if direct else [torch.empty_like(p) for p in prm]
    dfsum = torch.empty_like(fsum)
    loss = loss_out if loss_out is not None else torch.empty((), device=dev, dtype=f32)
    if accum is not None and (accum.dtype != torch.float64 or accum.device != dev):
        raise _lib.StemGNNHipError("accum must be a float64 scalar on the forecast's device")
    scratch = torch.empty(lib.stemgnn_fc_tail_train_scratch_floats(B, N, W, w2.shape[0]), device=dev, dtype=f32)

    acc_ptr = accum.data_ptr() if accum is not None else None
    norm = target_valid_count(target) if ignore_nan else None
    # one shared direct / deferred logic; only the three library calls differ between the plain, the `_loss` and the
    # `_quantile` form
    rows_call, finish_call, both_call, sel, fin_sel = entries(norm)
    # direct + unit_grad + side-stream mode: the step driver promises an immediate backward with an upstream gradient of 1
    # (engine.TrainStep) -> only the per-row launch runs here; the partial-sum launch (loss, fc gradients: no consumer
    # before the optimizer) is left for SpectralHotPath.backward to queue on the side branch (-10 us on the chain)
    # (state.tail_may_defer False: a caller whose backward has no SpectralHotPath node -- Model.loss with an adjacency --
    # nobody would run the thunk, so both launches run here)
    defer = direct and ctx.state.overlap and ctx.state.tail_finish is None and ctx.state.tail_may_defer
    if defer:
        _lib.check(rows_call(
            fsum.data_ptr(), target.data_ptr(), w0c.data_ptr(), b0c.data_ptr(), w2c.data_ptr(), b2c.data_ptr(), B, N, W, H,
            *sel, scratch.data_ptr(), None, dfsum.data_ptr(), _stream()), "fc_tail_train_rows")
        g0, g1, g2, g3 = grads

        def finish(stream, scratch=scratch, loss=loss, g0=g0, g1=g1, g2=g2, g3=g3, norm=norm):   # norm: kept alive
            _lib.check(finish_call(scratch.data_ptr(), B, N, W, H, *fin_sel, loss.data_ptr(), acc_ptr, g0.data_ptr(),
                                   g1.data_ptr(), g2.data_ptr(), g3.data_ptr(), stream),
                       "fc_tail_train_finish")
        ctx.state.tail_finish = finish
    else:
        _lib.check(both_call(
            fsum.data_ptr(), target.data_ptr(), w0c.data_ptr(), b0c.data_ptr(), w2c.data_ptr(), b2c.data_ptr(), B, N, W, H,
            *sel, scratch.data_ptr(), None, loss.data_ptr(), acc_ptr, dfsum.data_ptr(),
            grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), grads[3].data_ptr(), _stream()), "fc_tail_train")
    # (the reduction of the per-block partials -- loss, fc gradients -- stays a launch of its own on this stream.  Measured
    # in round 4: on the side stream no gain (the cross-queue edge costs what the 9 us launch returns); as the job of the
    # LAST workgroup to arrive of the first launch, 40 us instead of 12 + 10 -- one workgroup summing 114 partials that
    # other XCDs just wrote is a serial chain of fabric round trips)
    ctx.direct, ctx.unit_grad = direct, bool(unit_grad)
    ctx.held = (dfsum, None if direct else grads)
    ctx.set_materialize_grads(False)
    if loss_out is not None:
        ctx.mark_dirty(loss_out)
    return loss


def _fc_tail_train_backward(ctx, grad_loss, n_inputs):
    """Hands out what _fc_tail_train_forward holds; `n_inputs`: the Function's forward arguments (fsum, target, the four fc
    parameters in slots 0..5, then non-differentiable ones)."""
    dfsum, grads = ctx.held
    ctx.held = None
    if ctx.state.tail_finish is not None and not ctx.state.overlap:      # the mode changed between forward and backward
        fin, ctx.state.tail_finish = ctx.state.tail_finish, None
        fin(_stream())
    if not ctx.unit_grad:
        dfsum = dfsum * grad_loss
        if grads is not None:
            grads = [g * grad_loss for g in grads]
    if grads is None:
        return (dfsum,) + (None,) * (n_inputs - 1)
    return (dfsum, None, grads[0], grads[1], grads[2], grads[3]) + (None,) * (n_inputs - 6)


class FcTailMse(torch.autograd.Function):
    """Training tail as one node: fc tail (reference models/base_model.py:175-179) + nn.MSELoss(reduction='mean')
    (models/handler.py:140,162) + both backwards, two launches (``stemgnn_fc_tail_train``).  forward returns the loss
    and already holds d(loss)/d(fsum) and the fc parameter gradients for an upstream gradient of 1 (``loss.backward()``,
    handler.py:164); backward hands them out (scaled by the upstream gradient unless ``unit_grad``).
    (fsum [B,N,W], target [B,H,N], fc.0.weight, fc.0.bias, fc.2.weight, fc.2.bias) -> loss [].
    kind "mse" | "mae" | "huber" (param: Huber's delta) and ignore_nan (a NaN target is a missing one; the loss is the mean
    over the valid targets, ``target_valid_count`` being one more launch ahead of the tail) go through the ``_loss`` entries
    of the same kernels; with all three at their defaults the calls are the ones named above."""

    @staticmethod
    def forward(ctx, fsum, target, w0, b0, w2, b2, state=None, loss_out=None, accum=None, unit_grad=False, kind="mse",
                param=0.0, ignore_nan=False):
        lib = _lib.load()
        if kind not in _lib.SG_LOSS:
            raise ValueError(f"unknown loss kind {kind!r}: one of {sorted(_lib.SG_LOSS)}")
        plain = kind == "mse" and not ignore_nan           # today's entries

        def entries(norm):
            if plain:
                return (lib.stemgnn_fc_tail_train_rows, lib.stemgnn_fc_tail_train_finish, lib.stemgnn_fc_tail_train, (), ())
            norm_ptr = norm.data_ptr() if norm is not None else None
            return (lib.stemgnn_fc_tail_train_rows_loss, lib.stemgnn_fc_tail_train_finish_loss,
                    lib.stemgnn_fc_tail_train_loss, (_lib.SG_LOSS[kind], float(param), norm_ptr), (norm_ptr,))
        return _fc_tail_train_forward(ctx, fsum, target, (w0, b0, w2, b2), w2.shape[0], state, loss_out, accum, unit_grad,
                                      ignore_nan, entries)

    @staticmethod
    def backward(ctx, grad_loss):
        return _fc_tail_train_backward(ctx, grad_loss, 13)


class FcTailQuantile(torch.autograd.Function):
    """FcTailMse for a quantile head: fc.2 has Q * H rows (row q * H + h = level taus[q] of step h) and the loss is the pinball
    loss against the [B,H,N] target, mean over B Q H N (``stemgnn_fc_tail_train_quantile`` and its rows / finish pair: the same
    kernels, the same two launches, the same direct / deferred handling).
    (fsum [B,N,W], target [B,H,N], fc.0.weight, fc.0.bias, fc.2.weight [Q*H,W], fc.2.bias [Q*H], state, loss_out, accum,
    unit_grad, taus, ignore_nan) -> loss [].  taus: Q floats, strictly inside (0, 1); ignore_nan: a NaN target is missing for
    all Q of its rows and the normaliser is (valid targets) * Q."""

    @staticmethod
    def forward(ctx, fsum, target, w0, b0, w2, b2, state=None, loss_out=None, accum=None, unit_grad=False, taus=(0.5,),
                ignore_nan=False):
        lib = _lib.load()
        Q = len(taus)
        if Q < 1 or w2.shape[0] % Q != 0:
            raise _lib.StemGNNHipError(f"fc.2 has {w2.shape[0]} rows: not a multiple of the {Q} quantile levels")
        tau_arr = _lib.host_floats(taus)

        def entries(norm):
            norm_ptr = norm.data_ptr() if norm is not None else None
            return (lib.stemgnn_fc_tail_train_rows_quantile, lib.stemgnn_fc_tail_train_finish_quantile,
                    lib.stemgnn_fc_tail_train_quantile, (Q, tau_arr, norm_ptr), (Q, norm_ptr))
        return _fc_tail_train_forward(ctx, fsum, target, (w0, b0, w2, b2), w2.shape[0] // Q, state, loss_out, accum, unit_grad,
                                      ignore_nan, entries)

    @staticmethod
    def backward(ctx, grad_loss):
        return _fc_tail_train_backward(ctx, grad_loss, 12)


def target_valid_count(y):
    """``stemgnn_target_valid_count``: float32[2] = {count, 1 / count (0 when count is 0)} of the non-NaN values of `y`, one
    launch on the current stream, no host sync -- the normaliser the masked ``_loss`` entries read on the device."""
    lib = _lib.load()
    _require_gpu(y, "target")
    y = y.contiguous()
    norm = torch.empty(2, device=y.device, dtype=torch.float32)
    _lib.check(lib.stemgnn_target_valid_count(y.data_ptr(), y.numel(), norm.data_ptr(), _stream()), "target_valid_count")
    return norm


class GluFn(torch.autograd.Function):
    """Stand-alone GLU (reference models/base_model.py:6-13): x [M,K] -> (x Wl^T + bl) * sigmoid(x Wr^T + br) [M,C].
    Inside the model the GLU is the epilogue of the fused spectral GEMMs; this composition (general fp32 GEMM entry +
    elementwise kernels) only backs ``stemgnn_amd.GLU.forward`` for callers that use the module on its own."""

    @staticmethod
    def forward(ctx, x, wl, bl, wr, br):
        lib = _lib.load()
        for name, t in (("x", x), ("linear_left.weight", wl), ("linear_right.weight", wr)):
            _require_gpu(t, name)
        x, wl, bl, wr, br = (t.contiguous() for t in (x, wl, bl, wr, br))
        M, K = x.shape
        C = wl.shape[0]
        dev, st = x.device, _stream()
        U = torch.empty(M, C, device=dev)
        V = torch.empty(M, C, device=dev)
        for w, o in ((wl, U), (wr, V)):                 # x W^T: both operands k-contiguous
            _lib.check(lib.stemgnn_sgemm_f32(x.data_ptr(), K, 1, w.data_ptr(), K, 1, o.data_ptr(), C, M, C, K, 0, st), "sgemm")
        out, gate, lin = (torch.empty(M, C, device=dev) for _ in range(3))
        _lib.check(lib.stemgnn_glu_combine_fwd(U.data_ptr(), V.data_ptr(), bl.data_ptr(), br.data_ptr(), out.data_ptr(),
                                               gate.data_ptr(), lin.data_ptr(), M, C, st), "glu_combine_fwd")
        ctx.save_for_backward(x, wl, wr, lin, gate)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        x, wl, wr, lin, gate = ctx.saved_tensors
        M, K = x.shape
        C = wl.shape[0]
        dev, st = x.device, _stream()
        dout = dout.contiguous()
        dU, dV = torch.empty(M, C, device=dev), torch.empty(M, C, device=dev)
        _lib.check(lib.stemgnn_glu_combine_bwd(dout.data_ptr(), lin.data_ptr(), gate.data_ptr(), dU.data_ptr(),
                                               dV.data_ptr(), M, C, st), "glu_combine_bwd")
        dx = torch.empty(M, K, device=dev)
        dwl, dwr = torch.empty_like(wl), torch.empty_like(wr)
        dbl, dbr = torch.empty(C, device=dev), torch.empty(C, device=dev)
        for i, (d, w, dw, db) in enumerate(((dU, wl, dwl, dbl), (dV, wr, dwr, dbr))):
            # dx (+)= d W : A = d [M,C] k-contiguous, B(k=c, j) = W[c*K + j] (j-contiguous)
            _lib.check(lib.stemgnn_sgemm_f32(d.data_ptr(), C, 1, w.data_ptr(), K, 0, dx.data_ptr(), K, M, K, C, int(i > 0), st), "sgemm")
            # dW = d^T x : A(i=c, k=m) = d[m*C + c], B(k=m, j) = x[m*K + j]
            _lib.check(lib.stemgnn_sgemm_f32(d.data_ptr(), C, 0, x.data_ptr(), K, 0, dw.data_ptr(), K, C, K, M, 0, st), "sgemm")
            _lib.check(lib.stemgnn_colsum(d.data_ptr(), M, C, db.data_ptr(), st), "colsum")
        return dx, dwl, dbl, dwr, dbr


class StockBlockFn(torch.autograd.Function):
    """One StockBlockLayer (reference models/base_model.py:61-75) as a stand-alone autograd node:
    (X [B,N,W] contiguous, mul_L [4,N,N], multi, has_backcast, 33 block params) -> (forecast [B,N,W], backcast [B,N,W]).
    Model.forward uses the fused two-block node (SpectralHotPath); this one backs StockBlockLayer.forward and the model run
    from a given adjacency (Model.forward(x, adjacency=...)).  The GLU layers run in exact fp32 here whatever STEMGNN_DTYPE
    says (no split-bf16 form of this node).  A mul_L that needs no gradient (a frozen graph) gets none: the d(mul_L) product
    of stemgnn_gft_bwd is not launched."""

    @staticmethod
    def forward(ctx, X, mul_L, multi, has_bc, *params):
        lib = _lib.load()
        _require_gpu(X, "x")
        _require_gpu(mul_L, "mul_L")
        X = X.contiguous()
        mul_L = mul_L.contiguous()
        B, N, W = X.shape
        dev, f32 = X.device, torch.float32
        st = _stream()
        params = [None if p is None else p.contiguous() for p in params]
        tables = dft_tables(W, multi, dev)
        pk = torch.empty(lib.stemgnn_packed_floats(W, multi), device=dev, dtype=f32)
        sv = torch.empty(lib.stemgnn_saved_floats(B, N, W, multi), device=dev, dtype=f32)
        forecast = torch.empty(B, N, W, device=dev, dtype=f32)
        backcast = torch.empty(B, N, W, device=dev, dtype=f32) if has_bc else None
        parr = _lib.ptr_array(params)
        sb, sn, stt = N * W, W, 1
        _lib.check(lib.stemgnn_block_pack(parr, tables.data_ptr(), pk.data_ptr(), W, multi, st), "block_pack")
        _lib.check(lib.stemgnn_gft_fwd(mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, sv.data_ptr(), B, N, W, st), "gft_fwd")
        _lib.check(lib.stemgnn_spectral_glu_fwd(pk.data_ptr(), sv.data_ptr(), B, N, W, multi, st), "spectral_glu_fwd")
        _lib.check(lib.stemgnn_igft_heads_fwd(parr, pk.data_ptr(), sv.data_ptr(), X.data_ptr(), sb, sn, stt,
                                              forecast.data_ptr(), 0, backcast.data_ptr() if has_bc else None,
                                              B, N, W, multi, st), "igft_heads_fwd")
        ctx.dims = (B, N, W, multi, bool(has_bc))
        ctx.params = params
        ctx.aux = (X, mul_L, tables, pk, sv, backcast.detach() if has_bc else None)
        if has_bc:
            return forecast, backcast
        return forecast, None

    @staticmethod
    def backward(ctx, dforecast, dbackcast):
        lib = _lib.load()
        B, N, W, multi, has_bc = ctx.dims
        X, mul_L, tables, pk, sv, backcast = ctx.aux
        params = ctx.params
        dev, f32 = X.device, torch.float32
        st = _stream()
        nsplit = _NSPLIT
        if dforecast is None:
            dforecast = torch.zeros(B, N, W, device=dev, dtype=f32)
        dforecast = dforecast.contiguous()
        use_bc = has_bc and dbackcast is not None
        if has_bc and not use_bc:
            dbackcast = torch.zeros(B, N, W, device=dev, dtype=f32)
            use_bc = True
        scratch = torch.empty(lib.stemgnn_scratch_floats(B, N, W, multi), device=dev, dtype=f32)
        dG = scratch[lib.stemgnn_scratch_offset_dG(B, N, W, multi):]
        gradpart = torch.empty(lib.stemgnn_gradpart_floats(W, multi, nsplit), device=dev, dtype=f32)
        dmul_L = torch.zeros(4, N, N, device=dev, dtype=f32) if ctx.needs_input_grad[1] else None
        dX = torch.empty(B, N, W, device=dev, dtype=f32)
        parr = _lib.ptr_array(params)
        sb, sn, stt = N * W, W, 1
        _lib.check(lib.stemgnn_igft_heads_bwd(
            parr, pk.data_ptr(), sv.data_ptr(), X.data_ptr(), sb, sn, stt, dforecast.data_ptr(),
            dbackcast.contiguous().data_ptr() if use_bc else None, backcast.data_ptr() if use_bc else None,
            scratch.data_ptr(), gradpart.data_ptr(), nsplit, 1, B, N, W, multi, st), "igft_heads_bwd")
        _lib.check(lib.stemgnn_spectral_glu_bwd(pk.data_ptr(), sv.data_ptr(), scratch.data_ptr(), gradpart.data_ptr(),
                                                nsplit, 1, B, N, W, multi, st), "spectral_glu_bwd")
        _lib.check(lib.stemgnn_block_wgrad(parr, pk.data_ptr(), sv.data_ptr(), X.data_ptr(), sb, sn, stt,
                                           dforecast.data_ptr(), int(use_bc), scratch.data_ptr(), gradpart.data_ptr(),
                                           nsplit, 100, B, N, W, multi, st), "block_wgrad")
        _lib.check(lib.stemgnn_gft_bwd(mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, dG.data_ptr(), dX.data_ptr(),
                                       dmul_L.data_ptr() if dmul_L is not None else None, 0, B, N, W, st), "gft_bwd")
        grads = [None] * 33
        for i, p in enumerate(params):
            if p is None or (not has_bc and i in (7, 8)):
                continue
            grads[i] = torch.empty_like(p)
        _lib.check(lib.stemgnn_block_unpack_grads(gradpart.data_ptr(), nsplit, tables.data_ptr(), _lib.ptr_array(grads),
                                                  W, multi, int(has_bc), st), "block_unpack_grads")
        if use_bc and ctx.needs_input_grad[0]:
            # short-cut input of the backcast head (:71-72): backcast = sigmoid(BC(ig) - BS(x)) also depends on x directly.
            # Model.forward never needs this term (x is data); only a stand-alone block with a differentiable input does.
            _lib.check(lib.stemgnn_shortcut_dx(scratch.data_ptr(), params[7].data_ptr(), dX.data_ptr(), B, N, W, multi, st),
                       "shortcut_dx")
        return (dX, dmul_L, None, None, *grads)


def graph_degree(A):
    """``stemgnn_graph_degree``: deg [N] = row sums of the adjacency A [N,N] (reference models/base_model.py:141, before the
    symmetrisation), one wave per row in a fixed order."""
    lib = _lib.load()
    _require_gpu(A, "adjacency")
    A = A.contiguous()
    N = A.shape[0]
    deg = torch.empty(N, device=A.device, dtype=torch.float32)
    _lib.check(lib.stemgnn_graph_degree(A.data_ptr(), N, deg.data_ptr(), _stream()), "graph_degree")
    return deg


def spectral_route():
    """STEMGNN_SPECTRAL: "cheb" (default) or "eig", read per call."""
    return "eig" if os.environ.get("STEMGNN_SPECTRAL", "cheb") == "eig" else "cheb"


def graph_basis(A, deg):
    """(A [N,N], deg [N]) -> (attention [N,N] = 0.5 (A + A^T), mul_L [4,N,N]): the Laplacian kernel of the model's own front
    (``stemgnn_graph_basis_fwd``) and then the Chebyshev products, or the eigen route under STEMGNN_SPECTRAL=eig -- the launches
    SpectralHotPath.forward makes behind its attention, on the same values: the same bits."""
    lib = _lib.load()
    _require_gpu(A, "adjacency")
    _require_gpu(deg, "degree")
    A, deg = A.contiguous(), deg.contiguous()
    N = A.shape[0]
    if A.dim() != 2 or A.shape[1] != N or deg.numel() != N:
        raise _lib.StemGNNHipError(f"adjacency must be [N,N] with a degree of N entries, got {tuple(A.shape)} / {tuple(deg.shape)}")
    dev, f32, st = A.device, torch.float32, _stream()
    mul_L = torch.empty(4, N, N, device=dev, dtype=f32)
    attention = torch.empty(N, N, device=dev, dtype=f32)
    _lib.check(lib.stemgnn_graph_basis_fwd(A.data_ptr(), deg.data_ptr(), attention.data_ptr(), mul_L.data_ptr(), N, st),
               "graph_basis_fwd")
    if spectral_route() == "eig":
        lam = torch.empty(N, device=dev, dtype=f32)
        U = torch.empty(N, N, device=dev, dtype=f32)
        escr = torch.empty(lib.stemgnn_eigh_scratch_floats(N), device=dev, dtype=f32)
        _lib.check(lib.stemgnn_eigh_fwd(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), escr.data_ptr(), N, 0, st), "eigh_fwd")
    else:
        _lib.check(lib.stemgnn_cheb_fwd(mul_L.data_ptr(), N, st), "cheb_fwd")
    return attention, mul_L


class GraphBasisFn(torch.autograd.Function):
    """(A [N,N], degree [N] | None) -> (attention [N,N] = 0.5 (A + A^T), mul_L [4,N,N]): the spectral basis of a GIVEN adjacency
    (reference models/base_model.py:141-148 from the point behind the batch mean of :140).  degree None: the row sums of A
    (``stemgnn_graph_degree``), and A is differentiable -- both outputs are, mul_L too (unlike SpectralHotPath's): backward is
    d(mul_L) -> ``stemgnn_cheb_bwd`` -> ``stemgnn_graph_basis_bwd`` (degree term on), a gradient of the attention joining in
    that launch; with a gradient for the attention alone a seed kernel writes (G + G^T) / 2.  A stored degree is a constant of
    the graph and A then gets no gradient (None)."""

    @staticmethod
    def forward(ctx, A, degree=None):
        _require_gpu(A, "adjacency")
        A = A.contiguous()
        ctx.derived = degree is None
        deg = graph_degree(A) if degree is None else degree.contiguous()
        attention, mul_L = graph_basis(A, deg)
        ctx.save_for_backward(A, deg)
        ctx.mul_L = mul_L.detach() if ctx.derived and ctx.needs_input_grad[0] else None
        ctx.set_materialize_grads(False)
        return attention, mul_L

    @staticmethod
    def backward(ctx, datt, dmul_L):
        if not (ctx.derived and ctx.needs_input_grad[0]) or (datt is None and dmul_L is None):
            return None, None
        lib = _lib.load()
        A, deg = ctx.saved_tensors
        N = A.shape[0]
        dev, f32, st = A.device, torch.float32, _stream()
        dL = None
        if dmul_L is not None:
            dL = torch.empty(N, N, device=dev, dtype=f32)
            scratch = torch.empty(2 * N * N, device=dev, dtype=f32)
            _lib.check(lib.stemgnn_cheb_bwd(ctx.mul_L.data_ptr(), dmul_L.contiguous().data_ptr(), dL.data_ptr(),
                                            scratch.data_ptr(), N, st), "cheb_bwd")
        if datt is not None:
            datt = datt.contiguous()
        dA = torch.empty(N, N, device=dev, dtype=f32)
        _lib.check(lib.stemgnn_graph_basis_bwd(dL.data_ptr() if dL is not None else None,
                                               datt.data_ptr() if datt is not None else None, A.data_ptr(), deg.data_ptr(),
                                               dA.data_ptr(), N, st), "graph_basis_bwd")
        return dA, None


_keep_attention_state = False
_last_attention_state = {}


def capture_attention_state(flag=True):
    """Test hook: keep the key / query vectors ([B,N] each) of the last SpectralHotPath.forward per device, so a
    reference computed at higher precision can take the same LeakyReLU-kink decisions (key_i + query_j > 0)."""
    global _keep_attention_state
    _keep_attention_state = bool(flag)
    if not flag:
        _last_attention_state.clear()


def last_attention_state(device):
    return _last_attention_state.get(str(torch.device(device)))


def prepack_blocks(state, block_params, W, multi, device, batch_shape=None):
    """Pack both blocks' weights (stemgnn_block_pack) on the side stream now, so that they overlap whatever the
    caller queues next on the current stream (Model.hot_path: the GRU recurrence).  The next SpectralHotPath.forward
    on this device picks the packed panels up and joins the side stream.  batch_shape = (B, N) of the coming forward, when the
    caller knows it: the fused forward is warmed for that shape behind the packing."""
    lib = _lib.load()
    side, main = _side_stream(device), torch.cuda.current_stream()
    tables = dft_tables(W, multi, device)
    n_packed = lib.stemgnn_packed_floats(W, multi)
    blocks = [[None if p is None else p.contiguous() for p in blk] for blk in block_params]
    packed = [torch.empty(n_packed, device=device, dtype=torch.float32) for _ in blocks]
    ev, state.fork_event = state.fork_event, None
    if ev is not None:
        side.wait_event(ev)          # fork point chosen by the step driver (engine.TrainStep: ahead of the window gather)
    else:
        side.wait_stream(main)
    splits = glu_splits()
    split = []
    for blk, pk in zip(blocks, packed):
        parr = _lib.ptr_array(blk)

        def pack(stream, parr=parr, pk=pk, blk=blk):
            _pack_block(lib, parr, tables, pk, W, multi, splits, stream)
        pack(side.cuda_stream)
        if state.side_probe is not None:
            state.side_probe.append(pack)
        if splits:      # (allocated on the current stream like the packed panels; the side stream only runs the kernel)
            split.append(_split_panels(lib, pk, W, multi, splits, device, side.cuda_stream))
    # control words of the GRU's dW_hh product beside the backward recurrence (opt-in, STEMGNN_GRU_WHH_OVERLAP=1): zeroed HERE,
    # on the side branch under the GRU forward -- ordered ahead of the recurrence through the join that precedes the attention
    # kernels, and ahead of the side launch that reads them by stream order (round 6: the backward's schedule has no side ->
    # main edge ahead of the recurrence any more)
    if batch_shape is not None and bool(lib.stemgnn_gru_bwd_overlap_ok(batch_shape[0], batch_shape[1], batch_shape[1], W)):
        nctl = lib.stemgnn_gru_bwd_ctl_words(batch_shape[1])
        if state.gru_ctl is None or state.gru_ctl.numel() != nctl or state.gru_ctl.device != torch.device(device):
            state.gru_ctl = torch.zeros(nctl, device=device, dtype=torch.int32)
        _lib.check(lib.stemgnn_fill_zero(state.gru_ctl.data_ptr(), 4 * nctl, side.cuda_stream), "fill_zero")
        state.gru_ctl_zeroed = True
    # warm-up of the fused GLU forward (stemgnn_spectral_glu_fwd_warm): the kernel's code and block 0's weight stream into the
    # XCDs' L2 on eight CUs the GRU recurrence leaves idle; the first real launch of the step is ~10 us shorter for it
    # (exact fp32 only: the split-bf16 kernel is a third of the size and shows no first-launch penalty -- 38.1 / 37.6 us for the
    # two blocks -- while every extra launch beside the GRU forward costs that recurrence time: 219 -> 231 us with eight more)
    if batch_shape is not None and splits == 0 and os.environ.get("STEMGNN_GLU_WARM", "1") != "0":
        nwarm = lib.stemgnn_glu_warm_saved_floats(W, multi)
        if state.warm_saved is None or state.warm_saved.numel() != nwarm or state.warm_saved.device != torch.device(device):
            state.warm_saved = torch.zeros(nwarm, device=device, dtype=torch.float32)
        _lib.check(lib.stemgnn_spectral_glu_fwd_warm(packed[0].data_ptr(), split[0].data_ptr() if splits else None,
                                                     state.warm_saved.data_ptr(), batch_shape[0], batch_shape[1], W, multi,
                                                     splits, side.cuda_stream), "spectral_glu_fwd_warm")
    state.prepacked = (packed, side, blocks, (splits, split))


class SpectralHotPath(torch.autograd.Function):
    """(h, x, weight_key, weight_query, 33 params of block 0, 33 params of block 1) ->
    (sum of the two block forecasts [B,N,W], attention [N,N], mul_L [4,N,N]).

    h is the GRU output [N_seq, B, N_hid] exactly as nn.GRU returns it; x is the model input [B,W,N].

    Both the forecast sum and `attention` are differentiable (mul_L is not).  A gradient G for `attention` joins the backward
    inside the Laplacian backward's launch (stemgnn_attn_laplacian_bwd_ext): dA / B gets (G + G^T) / 2 / B added, everything
    behind it -- softmax backward, factored or materialised dh, GruFront.backward -- is the chain of the plain backward.
    With G alone (nothing flows into the forecast sum) the blocks' backward is skipped altogether: a seed kernel writes
    dA / B, no block tensor gets a gradient (None, not zeros) and x receives the GRU's share only.
    """

    @staticmethod
    def forward(ctx, h, x, wk, wq, multi, alpha, drop_p, training, seed, state, *block_params):
        lib = _lib.load()
        state = ctx.state = _state(state)
        # `h` came from ops.GruFront of the same model (Model.hot_path says so through the state): the backward may hand
        # the GRU its output gradient in factored form instead of materialising [N,B,N]
        ctx.factored, state.gru_front_live = bool(getattr(state, "gru_front_live", False)), False
        for name, t in (("gru output", h), ("x", x), ("weight_key", wk), ("weight_query", wq)):
            _require_gpu(t, name)
        assert len(block_params) == 2 * _lib.SG_BLOCK_NPARAMS
        h = h.contiguous()
        x = x.contiguous()
        B, W, N = x.shape
        if h.shape != (N, B, N):
            raise _lib.StemGNNHipError(f"gru output must be [N,B,N]=({N},{B},{N}), got {tuple(h.shape)}")
        dev, f32 = x.device, torch.float32
        st = _stream()
        M = B * N
        blocks = [list(block_params[:33]), list(block_params[33:])]
        blocks = [[None if p is None else p.contiguous() for p in blk] for blk in blocks]
        tables = dft_tables(W, multi, dev)

        mul_L = torch.empty(4, N, N, device=dev, dtype=f32)
        attention = torch.empty(N, N, device=dev, dtype=f32)
        attn_saved = torch.empty(lib.stemgnn_attn_saved_floats(B, N), device=dev, dtype=f32)
        use_drop = bool(training) and drop_p > 0.0
        # join the side stream BEFORE the first kernel that reads `seed`: in overlap mode the dropout stream's clone /
        # increment (Model._next_seed) and the weight packing were queued there (ordering edge clone -> attention)
        pre, state.prepacked = state.prepacked, None
        if pre is not None:
            torch.cuda.current_stream().wait_stream(pre[1])
        # exact data-parallel mode: the batch mean of the attention (:140) is the one cross-sample reduction of the path;
        # averaging A | deg over the ranks between the two parts restores single-process semantics for a split batch
        exact = state.exact_group
        for part in ((3,) if exact is None else (1, 2)):
            _lib.check(lib.stemgnn_attn_laplacian_fwd(
                h.data_ptr(), wk.data_ptr(), wq.data_ptr(), float(alpha), float(drop_p), int(bool(training)),
                seed.data_ptr() if use_drop else None, B, N, attn_saved.data_ptr(), attention.data_ptr(),
                mul_L.data_ptr(), part, st), "attn_laplacian_fwd")
            if exact is not None and part == 1:
                _all_reduce_mean(attn_saved[3 * B * N:3 * B * N + N * N + N], exact)
        if _keep_attention_state:
            _last_attention_state[str(dev)] = (attn_saved[:B * N].view(B, N).clone(),
                                               attn_saved[B * N:2 * B * N].view(B, N).clone())
        if os.environ.get("STEMGNN_SPECTRAL", "cheb") == "eig":
            # north-star eigen route: L = U^T diag(lam) U, T_k = sum_e p_k(lam_e) u_e u_e^T (same function of L;
            # the backward below is the polynomial one either way -- never differentiates through eigenvectors)
            lam = torch.empty(N, device=dev, dtype=f32)
            U = torch.empty(N, N, device=dev, dtype=f32)
            escr = torch.empty(lib.stemgnn_eigh_scratch_floats(N), device=dev, dtype=f32)
            _lib.check(lib.stemgnn_eigh_fwd(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), escr.data_ptr(), N,
                                            0, st), "eigh_fwd")
        else:
            _lib.check(lib.stemgnn_cheb_fwd(mul_L.data_ptr(), N, st), "cheb_fwd")

        fsum = torch.empty(B, N, W, device=dev, dtype=f32)
        backcast = torch.empty(B, N, W, device=dev, dtype=f32)
        packed, saved, split = [], [], []
        splits = pre[3][0] if pre is not None else glu_splits()
        n_packed = lib.stemgnn_packed_floats(W, multi)
        n_saved = lib.stemgnn_saved_floats(B, N, W, multi)
        xviews = [(x, W * N, 1, N), (backcast, N * W, W, 1)]   # X[b,n,t] strides of block 0 / block 1
        for s in range(2):
            sv = torch.empty(n_saved, device=dev, dtype=f32)
            parr = _lib.ptr_array(blocks[s])
            X, sb, sn, stt = xviews[s]
            sp = None
            if pre is not None:
                pk = pre[0][s]
                sp = pre[3][1][s] if splits else None
            else:
                pk = torch.empty(n_packed, device=dev, dtype=f32)
                _pack_block(lib, parr, tables, pk, W, multi, splits, st)
                if splits:
                    sp = _split_panels(lib, pk, W, multi, splits, dev, st)
            _lib.check(lib.stemgnn_gft_fwd(mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, sv.data_ptr(), B, N, W, st),
                       "gft_fwd")
            if splits:
                _lib.check(lib.stemgnn_spectral_glu_fwd_split(pk.data_ptr(), sp.data_ptr(), sv.data_ptr(), B, N, W, multi,
                                                              splits, st), "spectral_glu_fwd_split")
            else:
                _lib.check(lib.stemgnn_spectral_glu_fwd(pk.data_ptr(), sv.data_ptr(), B, N, W, multi, st),
                           "spectral_glu_fwd")
            split.append(sp)
            _lib.check(lib.stemgnn_igft_heads_fwd(
                parr, pk.data_ptr(), sv.data_ptr(), X.data_ptr(), sb, sn, stt, fsum.data_ptr(), int(s == 1),
                backcast.data_ptr() if s == 0 else None, B, N, W, multi, st), "igft_heads_fwd")
            packed.append(pk)
            saved.append(sv)

        ctx.dims = (B, N, W, multi, float(alpha), float(drop_p), bool(training))
        ctx.blocks = blocks
        ctx.aux = (h, x, wk, wq, seed, tables, mul_L, attn_saved, backcast, packed, saved)
        ctx.split = (splits, split)
        ctx.mark_non_differentiable(mul_L)
        ctx.set_materialize_grads(False)
        return fsum, attention, mul_L

    @staticmethod
    def backward(ctx, dfsum, datt, _dmulL):
        if dfsum is None and datt is None:
            return (None,) * (10 + 2 * _lib.SG_BLOCK_NPARAMS)
        lib = _lib.load()
        B, N, W, multi, alpha, drop_p, training = ctx.dims
        h, x, wk, wq, seed, tables, mul_L, attn_saved, backcast, packed, saved = ctx.aux
        blocks = ctx.blocks
        state = ctx.state
        splits, split = ctx.split
        dev, f32 = x.device, torch.float32
        st = _stream()
        tail_finish, state.tail_finish = state.tail_finish, None     # FcTailMse.forward's deferred partial-sum launch
        if dfsum is None and tail_finish is not None:
            # a gradient for the attention alone while the fused tail's deferred launch is pending (Model.loss whose loss was
            # left out of this backward): no shortcut -- the whole backward with a zero forecast gradient queues the thunk
            # where it always goes
            dfsum = torch.zeros(B, N, W, device=dev, dtype=f32)
        # attention-only: no gradient reaches the forecast sum, hence none reaches mul_L or any block tensor -- both blocks'
        # heads / GLU / GFT backward, the d(mul_L) product and the Chebyshev backward are skipped and none of their buffers
        # exists; the frozen-group machinery below (live -> no block gradient -> overlap off) does the rest
        attn_only = dfsum is None
        if not attn_only:
            dfsum = dfsum.contiguous()
        if datt is not None:
            datt = datt.contiguous()        # (autograd has checked shape and dtype against the output)
        nsplit = _NSPLIT
        n_scratch = lib.stemgnn_scratch_floats(B, N, W, multi)
        off_dG = lib.stemgnn_scratch_offset_dG(B, N, W, multi)
        n_gradpart = lib.stemgnn_gradpart_floats(W, multi, nsplit)
        dmul_L = None if attn_only else torch.empty(4, N, N, device=dev, dtype=f32)
        dbackcast = None if attn_only else torch.empty(B, N, W, device=dev, dtype=f32)
        xviews = [(x, W * N, 1, N), (backcast, N * W, W, 1)]
        grads = [[None] * 33, [None] * 33]
        direct_idx = set()
        # frozen parameter groups (no tensor of the group needs a gradient) get no buffers and no weight-gradient launches
        nig = ctx.needs_input_grad
        live = [not attn_only and any(nig[10 + 33 * s + i] for i, p in enumerate(blocks[s]) if p is not None) for s in (0, 1)]
        kq_live = nig[2] or nig[3]
        for s in (1, 0):
            for i, p in enumerate(blocks[s]):
                if p is None or (s == 1 and i in (7, 8)) or not live[s]:   # block 1's short-cut is unused (:73-74) -> grad None
                    continue
                if state.direct and p.grad is not None and p.grad.is_contiguous():
                    grads[s][i] = p.grad          # written in place by the unpack kernel
                    direct_idx.add((s, i))
                else:
                    grads[s][i] = torch.empty_like(p)
        # The weight-gradient GEMMs + un-packing feed nothing downstream in the backward pass.  When every block
        # gradient is written in place (direct-grad mode) they run on a side stream, overlapping the rest of the
        # chain -- in particular the latency-bound GRU recurrence, which leaves half of the CUs idle; whoever
        # consumes the gradients (optimizer / all-reduce, or GruFront.backward at the latest) joins the stream.
        n_block_grads = sum(g is not None for blk in grads for g in blk)
        overlap = state.overlap and n_block_grads > 0 and len(direct_idx) == n_block_grads
        side = _side_stream(dev) if overlap else None
        main = torch.cuda.current_stream()
        keep = []
        if tail_finish is not None and not overlap:
            tail_finish(st)
            tail_finish = None
        # Scheduling of the weight-gradient work (heads + GLU weight-gradient GEMMs + un-packing), which feeds nothing
        # downstream in the backward pass.  overlap: both blocks' weight gradients go to the side stream, block 0's
        # first (it overlaps the cheb / attention chain), then block 1's, which then runs under the GRU recurrence
        # (that kernel is latency-bound on half of the CUs and reserves its CUs' LDS, so the GEMMs land on the idle
        # CUs); block 1 therefore keeps its own scratch / partial buffers until the join.
        defer_b1 = overlap
        scratch0 = None if attn_only else torch.empty(n_scratch, device=dev, dtype=f32)
        gradpart0 = None if attn_only else torch.empty(n_gradpart, device=dev, dtype=f32)
        bufs = {0: (scratch0, gradpart0), 1: (scratch0, gradpart0)}
        if defer_b1:
            bufs[1] = (torch.empty(n_scratch, device=dev, dtype=f32), torch.empty(n_gradpart, device=dev, dtype=f32))

        def stage_fns(s):
            scratch, gradpart = bufs[s]
            parr = _lib.ptr_array(blocks[s])
            X, sb, sn, stt = xviews[s]
            has_bc = s == 0
            garr = _lib.ptr_array(grads[s])
            keep.append((parr, garr))

            def heads(stream):                  # data part: dpF, dpB, dig, d(pre-activation) of the last GLU layer
                _lib.check(lib.stemgnn_igft_heads_bwd(
                    parr, packed[s].data_ptr(), saved[s].data_ptr(), X.data_ptr(), sb, sn, stt, dfsum.data_ptr(),
                    dbackcast.data_ptr() if has_bc else None, backcast.data_ptr() if has_bc else None,
                    scratch.data_ptr(), gradpart.data_ptr(), nsplit, 1, B, N, W, multi, stream), "igft_heads_bwd")

            def glu(stream):                    # data-gradient chain of the three GLU layers -> dG
                # (bf16x2 with 4 W multi <= 256: one fused launch on the bf16 matrix pipe, csrc/glu_fused_bf16.h -- the entry
                # point decides; measured in round 5: the per-layer split launches cost +31 us per step against the fused fp32
                # chain, the fused bf16 chain is the one that beats it)
                if splits:
                    _lib.check(lib.stemgnn_spectral_glu_dgrad_split(
                        packed[s].data_ptr(), split[s].data_ptr(), saved[s].data_ptr(), scratch.data_ptr(),
                        B, N, W, multi, splits, stream), "spectral_glu_dgrad_split")
                    return
                _lib.check(lib.stemgnn_spectral_glu_bwd(
                    packed[s].data_ptr(), saved[s].data_ptr(), scratch.data_ptr(), gradpart.data_ptr(), nsplit, 1,
                    B, N, W, multi, stream), "spectral_glu_bwd")

            def wgrad(stream, cu_percent):      # every weight gradient of the block (fused kernel + the BS head)
                # bf16x2: the fused launch's products as split-bf16 too (round 6, csrc/wgrad.h wg_stage_bf16)
                _lib.check(lib.stemgnn_block_wgrad_split(
                    parr, packed[s].data_ptr(), saved[s].data_ptr(), X.data_ptr(), sb, sn, stt, dfsum.data_ptr(),
                    int(has_bc), scratch.data_ptr(), gradpart.data_ptr(), nsplit, cu_percent, B, N, W, multi,
                    2 if splits == 2 and os.environ.get("STEMGNN_WGRAD_BF16", "1") != "0" else 0, stream), "block_wgrad")

            def unpack(stream):
                _lib.check(lib.stemgnn_block_unpack_grads(
                    gradpart.data_ptr(), nsplit, tables.data_ptr(), garr, W, multi, int(has_bc), stream),
                    "block_unpack_grads")

            return heads, glu, wgrad, unpack

        # side-stream schedule: both weight-gradient launches fork right behind block 0's data-gradient chain -- block 0's
        # runs beside the Chebyshev / attention backward chain, block 1's (sized for the CUs the GRU leaves free) under the
        # GRU recurrence.  Measured alternatives (round 3, removed in round 4): forking block 1's right behind its own chain,
        # beside block 0's MFMA-bound data-gradient kernels, +170 us per step (two GEMM streams on one chip are zero-sum);
        # forking only behind the Chebyshev backward +32 us; block 0's GFT backward ahead of the fork +9 us.  Round 5, with the
        # faster bf16 chain and weight-gradient kernels: both launches forked at the GRU backward (under the recurrence) +29 us.
        # Capture order matters inside the hipGraph step: at a fork the FIRST captured successor of a node stays on its
        # queue, every later one moves to another queue behind a cross-queue edge (~10 us).  So at every fork the main
        # stream's next kernel (the critical chain) is queued before the side stream's work that forks at the same node.
        # Both blocks' shares of d(mul_L): round 6 -- ONE product behind block 0's data-gradient chain (stemgnn_gft_bwd_dt2, K =
        # the two blocks' (b, t) ranges back to back) instead of block 1's product on the side branch + block 0's accumulating
        # product on the chain: the fork behind block 1's dX product and the join ahead of block 0's product were ~15 us of
        # cross-queue latency on the critical chain.
        dt1 = None
        for s in (() if attn_only else (1, 0)):
            scratch = bufs[s][0]
            dG = scratch[off_dG:]
            X, sb, sn, stt = xviews[s]
            heads, glu, wgrad, unpack = stage_fns(s)
            heads(st)
            glu(st)
            if not overlap:
                if live[s]:
                    wgrad(st, 100)
                    unpack(st)
                _lib.check(lib.stemgnn_gft_bwd(
                    mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, dG.data_ptr(),
                    dbackcast.data_ptr() if s == 1 else None, dmul_L.data_ptr(), int(s == 0), B, N, W, st), "gft_bwd")
            elif s == 1:
                # block 1: only its data gradient (-> dbackcast) feeds block 0's backward
                _lib.check(lib.stemgnn_gft_bwd(mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, dG.data_ptr(),
                                               dbackcast.data_ptr(), None, 0, B, N, W, st), "gft_bwd dX")
                dt1 = (X, sb, sn, stt, dG)
            else:
                fork = torch.cuda.Event()                # every data-gradient chain is queued
                fork.record(main)
                X1, sb1, sn1, stt1, dG1 = dt1
                _lib.check(lib.stemgnn_gft_bwd_dt2(X.data_ptr(), sb, sn, stt, dG.data_ptr(), X1.data_ptr(), sb1, sn1, stt1,
                                                   dG1.data_ptr(), dmul_L.data_ptr(), B, N, W, st), "gft_bwd_dt2")
                side.wait_event(fork)
                with torch.cuda.stream(side):
                    sst = side.cuda_stream
                    for ss in (0, 1):
                        if not live[ss]:
                            continue
                        _h, _g, w2, u2 = (heads, glu, wgrad, unpack) if ss == 0 else stage_fns(1)
                        w2(sst, _wg_cu(ss, B, N))
                        u2(sst)
                        if state.side_probe is not None:
                            state.side_probe.append(lambda stream, w2=w2, pc=_wg_cu(ss, B, N): w2(stream, pc))
                            state.side_probe.append(u2)
                    if tail_finish is not None:          # loss + fc gradients: ahead of the hook (fc is part of its range)
                        tail_finish(sst)
                        keep.append(tail_finish)         # its buffers stay alive until the join
                        if state.side_probe is not None:
                            state.side_probe.append(tail_finish)
                    if state.block_grads_hook is not None:
                        state.block_grads_hook()         # data-parallel: reduce the finished range under the GRU recurrence
                keep.append(bufs)                        # alive until the join
        dX0 = None
        if nig[1] and not attn_only:
            # d(loss)/dx through block 0 (x is its input X, :169): the GFT adjoint sum_k T_k^T dG0_k (:63) minus the short-cut
            # head's direct term (:70-71), from block 0's heads data part still in scratch0 -- written [B,N,W], handed out as
            # x's [B,W,N] view.  The GRU's share comes from GruFront.backward; autograd adds the two.
            X, sb, sn, stt = xviews[0]
            dX0 = torch.empty(B, N, W, device=dev, dtype=f32)
            _lib.check(lib.stemgnn_gft_bwd(mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, scratch0[off_dG:].data_ptr(),
                                           dX0.data_ptr(), None, 0, B, N, W, st), "gft_bwd dX")
            _lib.check(lib.stemgnn_shortcut_dx(scratch0.data_ptr(), blocks[0][7].data_ptr(), dX0.data_ptr(), B, N, W, multi, st),
                       "shortcut_dx")
        if overlap:
            state.pending = (side, (keep, packed, saved, split, backcast, dfsum, dbackcast))
        dL = None
        if not attn_only:
            dL = torch.empty(N, N, device=dev, dtype=f32)
            cheb_scratch = torch.empty(2 * N * N, device=dev, dtype=f32)
            _lib.check(lib.stemgnn_cheb_bwd(mul_L.data_ptr(), dmul_L.data_ptr(), dL.data_ptr(), cheb_scratch.data_ptr(),
                                            N, st), "cheb_bwd")
        # factored: dh[s,b,i] = dkey[b,i] wk[s] + dquery[b,i] wq[s] goes to the GRU backward as its two [B,N] factors
        # (stemgnn_gru_bwd_rank2); the kernel that would materialise the 6.6 MB tensor (and form dwk / dwq on the way) leaves
        # the critical chain, dwk / dwq come from a small kernel of their own on the side stream
        factored = ctx.factored and ctx.needs_input_grad[0] and bool(lib.stemgnn_gru_bwd_rank2_ok(B, N))
        dh = torch.empty(1, device=dev, dtype=f32).expand(N, B, N) if factored else torch.empty_like(h)   # placeholder: never read
        kq_direct = kq_live and state.direct and wk.grad is not None and wq.grad is not None
        if kq_live:
            dwk = wk.grad if kq_direct else torch.empty_like(wk)
            dwq = wq.grad if kq_direct else torch.empty_like(wq)
        elif factored:
            dwk = dwq = None            # frozen key / query: the factored attention backward forms neither
        else:
            dwk, dwq = torch.empty(2, N, device=dev, dtype=f32)       # written on the way to dh, never read
        _ptr = lambda t: None if t is None else t.data_ptr()
        attn_scratch = torch.empty(lib.stemgnn_attn_scratch_floats(B, N, _NCHUNK), device=dev, dtype=f32)
        use_drop = training and drop_p > 0.0
        # exact mode: d(loss_global)/dA = mean over ranks of the local dA, and the flat gradient bucket is AVERAGED later,
        # so every rank back-propagates the rank-mean of dA / B through its own samples
        exact = state.exact_group
        # round 6: with the factored form on the side-stream schedule the chunk sum of dquery is not a launch of its own on the
        # chain -- the GRU backward's zero-fill launch carries it (stemgnn_gru_bwd_rank2_dq), the key / query weight gradients
        # on the side branch sum their own copy (same fixed order, same bits)
        follower = bool(overlap and ctx.factored and state.gru_ctl_zeroed and lib.stemgnn_gru_bwd_overlap_ok(B, N, N, W))
        dq_parts = bool(factored and overlap and kq_direct and not follower)      # (the follower's _begin call takes dquery reduced)
        if not kq_live:                 # frozen key / query: nothing else reads dquery -- the GRU backward's fill launch sums it
            dq_parts = bool(factored and not follower)
        # a gradient for the returned attention: the _ext entry's Laplacian backward carries it in the same launch (dL None:
        # its seed kernel).  Exact mode: G belongs to the rank-AVERAGED attention and is the same on every rank, so adding it in
        # part 1, ahead of the rank mean, is right -- mean_r(dA_r + G) = mean_r(dA_r) + G
        if datt is None:
            bwd_entry, head = lib.stemgnn_attn_laplacian_bwd, (dL.data_ptr(),)
        else:
            bwd_entry, head = lib.stemgnn_attn_laplacian_bwd_ext, (_ptr(dL), datt.data_ptr())
        for part in ((3,) if exact is None else (1, 2)):
            _lib.check(bwd_entry(
                *head, h.data_ptr(), wk.data_ptr(), wq.data_ptr(), alpha, drop_p, int(training),
                seed.data_ptr() if use_drop else None, B, N, attn_saved.data_ptr(), attn_scratch.data_ptr(), _NCHUNK,
                None if factored else dh.data_ptr(), _ptr(dwk), _ptr(dwq),
                part | ((4 | (8 if dq_parts else 0)) if factored and part != 1 else 0), st), "attn_laplacian_bwd")
            if exact is not None and part == 1:
                _all_reduce_mean(attn_scratch[:N * N], exact)
        if factored:
            after = None
            if overlap and kq_direct:       # behind block 1's weight gradients on the side stream, under the GRU recurrence;
                kq_ready = torch.cuda.Event()                         # queued by GruFront.backward BEHIND its own launches
                kq_ready.record(main)                                 # (capture order, see above)
                pend, hh, kdwk, kdwq = state.pending, h, dwk, dwq
                dq2 = torch.empty(B, N, device=dev, dtype=f32) if dq_parts else None

                def kq_wgrad(stream):
                    if dq2 is not None:
                        _lib.check(lib.stemgnn_attn_dquery_reduce(attn_scratch.data_ptr(), B, N, _NCHUNK, dq2.data_ptr(), stream),
                                   "attn_dquery_reduce")
                        _lib.check(lib.stemgnn_keyquery_wgrad2(hh.data_ptr(), attn_scratch.data_ptr() + 4 * N * N, dq2.data_ptr(),
                                                               kdwk.data_ptr(), kdwq.data_ptr(), B, N, stream), "keyquery_wgrad2")
                        return
                    _lib.check(lib.stemgnn_keyquery_wgrad(hh.data_ptr(), attn_scratch.data_ptr(), kdwk.data_ptr(),
                                                          kdwq.data_ptr(), B, N, stream), "keyquery_wgrad")

                def after():
                    side.wait_event(kq_ready)
                    with torch.cuda.stream(side):
                        kq_wgrad(side.cuda_stream)
                    pend[1][0].append((attn_scratch, hh, dq2))
                if state.side_probe is not None:
                    state.side_probe.append(kq_wgrad)
            state.dh_factors = (attn_scratch, B, N, wk, wq, after, _NCHUNK if dq_parts else 0)
            if after is None and kq_live:
                _lib.check(lib.stemgnn_keyquery_wgrad(h.data_ptr(), attn_scratch.data_ptr(), dwk.data_ptr(), dwq.data_ptr(),
                                                      B, N, st), "keyquery_wgrad")
        for s_, i_ in direct_idx:
            grads[s_][i_] = None                  # already in p.grad: nothing for autograd to accumulate
        if kq_direct or not kq_live:
            dwk = dwq = None
        dx = dX0.permute(0, 2, 1) if dX0 is not None else None
        return (dh, dx, dwk, dwq, None, None, None, None, None, None, *grads[0], *grads[1])


# ---------------------------------------------------------------------------------------------------------------
# data path either side of the hot path: thin wrappers over csrc/data.hip

def latent_adjacency(x, gru_params, wk, wq, alpha, drop_p):
    """The model's own graph for the batch x [B,W,N] in eval mode: the GRU recurrence (stemgnn_gru_fwd_infer) and the attention /
    Laplacian launches of forecast_forward, of which A [N,N] | deg [N] -- the batch-mean attention ahead of the symmetrisation
    and the degrees the fused front summed for it -- are returned as one contiguous view of N*N + N floats."""
    lib = _lib.load()
    w_ih, w_hh, b_ih, b_hh = (t.contiguous() for t in gru_params)
    for name, t in (("x", x), ("GRU.weight_ih_l0", w_ih), ("GRU.weight_hh_l0", w_hh), ("weight_key", wk),
                    ("weight_query", wq)):
        _require_gpu(t, name)
    x = x.contiguous()
    B, W, N = x.shape
    Hd = w_hh.shape[1]
    if Hd != N:
        raise _lib.StemGNNHipError(f"GRU hidden size {Hd} != units {N}")
    dev, f32, st = x.device, torch.float32, _stream()
    h_ext = torch.empty(N + 1, B, Hd, device=dev, dtype=f32)
    gscr = torch.empty(lib.stemgnn_gru_fwd_scratch_floats(B, N, Hd), device=dev, dtype=f32)
    _lib.check(lib.stemgnn_gru_fwd_infer(x.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(),
                                         B, N, Hd, W, gscr.data_ptr(), h_ext.data_ptr(), gru_status(dev).data_ptr(), st),
               "gru_fwd_infer")
    mul_L = torch.empty(4, N, N, device=dev, dtype=f32)
    attention = torch.empty(N, N, device=dev, dtype=f32)
    attn_saved = torch.empty(lib.stemgnn_attn_saved_floats(B, N), device=dev, dtype=f32)
    # parts = 3, the call forecast_forward makes: its fused kernel takes the degrees from the per-chunk row sums (another order
    # than the separate reduction of parts = 1), and those are the degrees a frozen graph must carry to reproduce its bits
    _lib.check(lib.stemgnn_attn_laplacian_fwd(h_ext[1:].data_ptr(), wk.data_ptr(), wq.data_ptr(), float(alpha), float(drop_p),
                                              0, None, B, N, attn_saved.data_ptr(), attention.data_ptr(), mul_L.data_ptr(), 3,
                                              st), "attn_laplacian_fwd")
    return attn_saved[3 * B * N:3 * B * N + N * N + N]


def forecast_forward(x, gru_params, wk, wq, multi, alpha, drop_p, block_params, fc_params, adjacency=None):
    """Inference forward of Model (reference models/base_model.py:136-179 in eval mode) without autograd and without the
    tensors only a backward pass reads: the GRU recurrence without its gate reserve (stemgnn_gru_fwd_infer), attention /
    Laplacian with training = 0, Chebyshev basis (eigen route under STEMGNN_SPECTRAL=eig), both StockBlocks on the _infer
    entries (one workspace of stemgnn_infer_workspace_split_floats floats, reused by block 1), then the fc tail kernel.
    Same kernels and arithmetic as SpectralHotPath.forward in eval mode: bit-identical outputs.  The weights are packed
    on every call, as in training.  x [B,W,N]; gru_params = (weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0);
    block_params = 2 x 33 block tensors; fc_params = (fc.0.weight, fc.0.bias, fc.2.weight, fc.2.bias).
    adjacency (a graph.LatentGraph or an [N,N] tensor): the GRU and the attention are skipped, mul_L and the symmetrised
    attention come from the graph (a LatentGraph caches them); everything from the blocks on is unchanged.
    Returns (forecast [B,H,N], attention [N,N])."""
    lib = _lib.load()
    if adjacency is not None:
        return _forecast_forward_graph(x, adjacency, multi, block_params, fc_params)
    w_ih, w_hh, b_ih, b_hh = (t.contiguous() for t in gru_params)
    for name, t in (("x", x), ("GRU.weight_ih_l0", w_ih), ("GRU.weight_hh_l0", w_hh), ("weight_key", wk),
                    ("weight_query", wq)):
        _require_gpu(t, name)
    assert len(block_params) == 2 * _lib.SG_BLOCK_NPARAMS
    x = x.contiguous()
    B, W, N = x.shape
    Hd = w_hh.shape[1]
    if Hd != N:
        raise _lib.StemGNNHipError(f"GRU hidden size {Hd} != units {N}")
    dev, f32 = x.device, torch.float32
    st = _stream()
    # GRU (reference :137) -> h [N,B,N] = h_ext[1:]
    h_ext = torch.empty(N + 1, B, Hd, device=dev, dtype=f32)
    gscr = torch.empty(lib.stemgnn_gru_fwd_scratch_floats(B, N, Hd), device=dev, dtype=f32)
    _lib.check(lib.stemgnn_gru_fwd_infer(x.data_ptr(), w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(), b_hh.data_ptr(),
                                         B, N, Hd, W, gscr.data_ptr(), h_ext.data_ptr(), gru_status(dev).data_ptr(), st),
               "gru_fwd_infer")
    del gscr                        # (stream-ordered reuse by the caching allocator: lowers the call's peak)
    # attention + Laplacian (eval: no dropout) and the spectral basis
    mul_L = torch.empty(4, N, N, device=dev, dtype=f32)
    attention = torch.empty(N, N, device=dev, dtype=f32)
    attn_saved = torch.empty(lib.stemgnn_attn_saved_floats(B, N), device=dev, dtype=f32)
    _lib.check(lib.stemgnn_attn_laplacian_fwd(h_ext[1:].data_ptr(), wk.data_ptr(), wq.data_ptr(), float(alpha), float(drop_p),
                                              0, None, B, N, attn_saved.data_ptr(), attention.data_ptr(), mul_L.data_ptr(), 3,
                                              st), "attn_laplacian_fwd")
    if os.environ.get("STEMGNN_SPECTRAL", "cheb") == "eig":
        lam = torch.empty(N, device=dev, dtype=f32)
        U = torch.empty(N, N, device=dev, dtype=f32)
        escr = torch.empty(lib.stemgnn_eigh_scratch_floats(N), device=dev, dtype=f32)
        _lib.check(lib.stemgnn_eigh_fwd(mul_L.data_ptr(), lam.data_ptr(), U.data_ptr(), escr.data_ptr(), N, 0, st), "eigh_fwd")
    else:
        _lib.check(lib.stemgnn_cheb_fwd(mul_L.data_ptr(), N, st), "cheb_fwd")
    del attn_saved
    return _forecast_blocks(x, mul_L, multi, block_params, fc_params), attention


def _forecast_forward_graph(x, adjacency, multi, block_params, fc_params):
    from .graph import resolve_basis
    _require_gpu(x, "x")
    assert len(block_params) == 2 * _lib.SG_BLOCK_NPARAMS
    x = x.contiguous()
    attention, mul_L = resolve_basis(adjacency, x.device)
    if mul_L.shape[1] != x.shape[2]:
        raise _lib.StemGNNHipError(f"adjacency is [{mul_L.shape[1]},{mul_L.shape[1]}] but x has {x.shape[2]} nodes")
    return _forecast_blocks(x, mul_L.detach(), multi, block_params, fc_params), attention.detach()


def _forecast_blocks(x, mul_L, multi, block_params, fc_params):
    """Both StockBlocks on the _infer entries and the fc tail: x [B,W,N] contiguous, mul_L [4,N,N] -> forecast [B,H,N]."""
    lib = _lib.load()
    B, W, N = x.shape
    dev, f32 = x.device, torch.float32
    st = _stream()
    # both StockBlocks through one inference workspace (G | layer-2 GLU outputs | ping-pong slabs where needed)
    splits = glu_splits()
    tables = dft_tables(W, multi, dev)
    n_ws = lib.stemgnn_infer_workspace_split_floats(B, N, W, multi, splits)
    ws = torch.empty(n_ws, device=dev, dtype=f32)
    fsum = torch.empty(B, N, W, device=dev, dtype=f32)
    backcast = torch.empty(B, N, W, device=dev, dtype=f32)
    n_packed = lib.stemgnn_packed_floats(W, multi)
    blocks = [list(block_params[:33]), list(block_params[33:])]
    xviews = [(x, W * N, 1, N), (backcast, N * W, W, 1)]   # X[b,n,t] strides of block 0 / block 1
    for s in range(2):
        blk = [None if p is None else p.contiguous() for p in blocks[s]]
        parr = _lib.ptr_array(blk)
        X, sb, sn, stt = xviews[s]
        pk = torch.empty(n_packed, device=dev, dtype=f32)
        _pack_block(lib, parr, tables, pk, W, multi, splits, st)
        _lib.check(lib.stemgnn_gft_fwd(mul_L.data_ptr(), X.data_ptr(), sb, sn, stt, ws.data_ptr(), B, N, W, st), "gft_fwd")
        if splits:
            sp = _split_panels(lib, pk, W, multi, splits, dev, st)
            _lib.check(lib.stemgnn_spectral_glu_fwd_split_infer(pk.data_ptr(), sp.data_ptr(), ws.data_ptr(), n_ws, B, N, W,
                                                                multi, splits, st), "spectral_glu_fwd_split_infer")
        else:
            _lib.check(lib.stemgnn_spectral_glu_fwd_infer(pk.data_ptr(), ws.data_ptr(), n_ws, B, N, W, multi, st),
                       "spectral_glu_fwd_infer")
        _lib.check(lib.stemgnn_igft_heads_fwd_infer(parr, pk.data_ptr(), ws.data_ptr(), n_ws, X.data_ptr(), sb, sn, stt,
                                                    fsum.data_ptr(), int(s == 1), backcast.data_ptr() if s == 0 else None,
                                                    B, N, W, multi, st), "igft_heads_fwd_infer")
    # fc tail (:175-179) -> [B,H,N]
    w0, b0, w2, b2 = (t.contiguous() for t in fc_params)
    H = w2.shape[0]
    forecast = torch.empty(B, H, N, device=dev, dtype=f32)
    _lib.check(lib.stemgnn_fc_tail_fwd(fsum.data_ptr(), w0.data_ptr(), b0.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                                       B, N, W, H, forecast.data_ptr(), st), "fc_tail_fwd")
    return forecast


def forecast_store(forecast, target, pos, out_forecast, out_target):
    """Result slabs of engine.ForecastStep: out_*[pos + b] = forecast / target[b] with the row position read on the device
    (pos: int64[1]); rows at or beyond the slabs' capacity are dropped."""
    lib = _lib.load()
    B, H, N = forecast.shape
    if target.shape != forecast.shape or out_forecast.shape[1:] != (H, N) or out_target.shape != out_forecast.shape:
        raise _lib.StemGNNHipError("forecast_store: shape mismatch")
    if pos.dtype != torch.int64 or pos.device != forecast.device:
        raise _lib.StemGNNHipError("forecast_store: pos must be an int64 tensor on the forecast's device")
    _lib.check(lib.stemgnn_forecast_store(forecast.data_ptr(), target.data_ptr(), pos.data_ptr(), out_forecast.data_ptr(),
                                          out_target.data_ptr(), B, H, N, out_forecast.shape[0], _stream()), "forecast_store")


class MSELossFn(torch.autograd.Function):
    """nn.MSELoss(reduction='mean') of the driver (reference models/handler.py:140,162) as two fixed-order kernels."""

    @staticmethod
    def forward(ctx, forecast, target, loss_out=None, accum=None):
        """loss_out: optional float32 scalar to write the loss into (a static buffer); accum: optional float64 device
        scalar that receives `+= loss` inside the reduction kernel (epoch loss sum without extra launches)."""
        lib = _lib.load()
        _require_gpu(forecast, "forecast")
        _require_gpu(target, "target")
        if forecast.shape != target.shape:
            raise _lib.StemGNNHipError(f"MSE: shapes differ {tuple(forecast.shape)} vs {tuple(target.shape)}")
        forecast, target = forecast.contiguous(), target.contiguous()
        scratch = torch.empty(lib.stemgnn_mse_scratch_floats(), device=forecast.device, dtype=torch.float32)
        loss = loss_out if loss_out is not None else torch.empty((), device=forecast.device, dtype=torch.float32)
        if accum is not None and (accum.dtype != torch.float64 or accum.device != forecast.device):
            raise _lib.StemGNNHipError("MSE: accum must be a float64 scalar on the forecast's device")
        _lib.check(lib.stemgnn_mse_fwd(forecast.data_ptr(), target.data_ptr(), forecast.numel(), scratch.data_ptr(),
                                       loss.data_ptr(), accum.data_ptr() if accum is not None else None, _stream()),
                   "mse_fwd")
        ctx.save_for_backward(forecast, target)
        ctx.set_materialize_grads(False)
        if loss_out is not None:
            ctx.mark_dirty(loss_out)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        lib = _lib.load()
        forecast, target = ctx.saved_tensors
        grad_loss = grad_loss.contiguous()
        dforecast = torch.empty_like(forecast)
        _lib.check(lib.stemgnn_mse_bwd(forecast.data_ptr(), target.data_ptr(), forecast.numel(), grad_loss.data_ptr(),
                                       dforecast.data_ptr(), _stream()), "mse_bwd")
        return dforecast, None, None, None


def mse_loss(forecast, target, loss_out=None, accum=None):
    return MSELossFn.apply(forecast, target, loss_out, accum)


class MSELoss(torch.nn.Module):
    """Drop-in for ``nn.MSELoss(reduction='mean')`` at models/handler.py:140."""

    def __init__(self, reduction="mean"):
        super().__init__()
        if reduction != "mean":
            raise ValueError("stemgnn_amd.ops.MSELoss implements reduction='mean' only (the reference's setting)")

    def forward(self, forecast, target):
        return MSELossFn.apply(forecast, target)


def normalize_series(raw, sub, div, clip01):
    """raw [T,N] float64 (device) -> float32 [T,N]: (raw - sub[n]) / div[n] in fp64, optional clip to [0,1]."""
    lib = _lib.load()
    if not raw.is_cuda or raw.dtype != torch.float64:
        raise _lib.StemGNNHipError("normalize_series: raw must be a float64 tensor on a HIP device")
    raw, sub, div = raw.contiguous(), sub.contiguous(), div.contiguous()
    T, N = raw.shape
    out = torch.empty(T, N, device=raw.device, dtype=torch.float32)
    _lib.check(lib.stemgnn_normalize_series(raw.data_ptr(), sub.data_ptr(), div.data_ptr(), int(bool(clip01)),
                                            out.data_ptr(), T, N, _stream()), "normalize_series")
    return out


_gather_status = {}


def _check_target_series(series, target_series, what):
    _require_gpu(target_series, "target_series")
    if target_series.shape != series.shape or target_series.device != series.device or not target_series.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: target_series must be a contiguous [T,N] tensor of the series' shape and device")


def window_gather(series, hi, W, H, x=None, y=None, target_series=None):
    """series [T,N] fp32 resident, hi [B] int64 (device): x[b] = series[hi-W:hi], y[b] = series[hi:hi+H]; with
    `target_series` (same shape) y[b] = target_series[hi:hi+H] instead (stemgnn_window_gather_pair)."""
    lib = _lib.load()
    _require_gpu(series, "series")
    if hi.dtype != torch.int64 or hi.device != series.device:
        raise _lib.StemGNNHipError("window_gather: hi must be an int64 tensor on the series' device")
    T, N = series.shape
    B = hi.numel()
    if x is None:
        x = torch.empty(B, W, N, device=series.device, dtype=torch.float32)
    if y is None:
        y = torch.empty(B, H, N, device=series.device, dtype=torch.float32)
    key = str(series.device)
    st = _gather_status.get(key)
    if st is None:
        st = _gather_status[key] = torch.zeros(1, dtype=torch.int32, device=series.device)
    if target_series is not None:
        _check_target_series(series, target_series, "window_gather")
        _lib.check(lib.stemgnn_window_gather_pair(series.data_ptr(), target_series.data_ptr(), hi.data_ptr(), x.data_ptr(),
                                                  y.data_ptr(), B, W, H, N, T, st.data_ptr(), _stream()), "window_gather")
        return x, y
    _lib.check(lib.stemgnn_window_gather(series.data_ptr(), hi.data_ptr(), x.data_ptr(), y.data_ptr(), B, W, H, N, T,
                                         st.data_ptr(), _stream()), "window_gather")
    return x, y


def window_gather_queue(series, order, queue, B, W, H, x, y, target_series=None):
    """Iterator form (stemgnn_window_gather_queue): the next B windows of `order` (int64, device) at the device-side
    position queue[0]; the kernel advances the position itself.  queue: int64[4] = {position, 0, count, -}.
    `target_series`: as in window_gather (stemgnn_window_gather_queue_pair)."""
    lib = _lib.load()
    _require_gpu(series, "series")
    for t, n in ((order, "order"), (queue, "queue")):
        if t.dtype != torch.int64 or t.device != series.device or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"window_gather_queue: {n} must be a contiguous int64 tensor on the series' device")
    T, N = series.shape
    key = str(series.device)
    st = _gather_status.get(key)
    if st is None:
        st = _gather_status[key] = torch.zeros(1, dtype=torch.int32, device=series.device)
    if target_series is not None:
        _check_target_series(series, target_series, "window_gather_queue")
        _lib.check(lib.stemgnn_window_gather_queue_pair(series.data_ptr(), target_series.data_ptr(), order.data_ptr(),
                                                        queue.data_ptr(), x.data_ptr(), y.data_ptr(), B, W, H, N, T,
                                                        st.data_ptr(), _stream()), "window_gather_queue")
        return x, y
    _lib.check(lib.stemgnn_window_gather_queue(series.data_ptr(), order.data_ptr(), queue.data_ptr(), x.data_ptr(),
                                               y.data_ptr(), B, W, H, N, T, st.data_ptr(), _stream()), "window_gather_queue")
    return x, y


def check_gather_status(device):
    """Raise if any window_gather since the last check saw an out-of-range index (one sync; call per epoch)."""
    st = _gather_status.get(str(device))
    if st is not None:
        v = int(st.item())
        if v != 0:
            st.zero_()
            raise IndexError("window_gather: window index outside the series" if v & 1 else
                             "window_gather_queue: stepped past the end of the loaded order")


def roll_window(inputs, forecast, forecast_steps, step, horizon):
    """One iteration of the reference's rolling inference (models/handler.py:56-61); returns the next inputs."""
    lib = _lib.load()
    _require_gpu(inputs, "inputs")
    _require_gpu(forecast, "forecast")
    B, W, N = inputs.shape
    L = forecast.shape[1]
    if L == 0:
        raise Exception("Get blank inference result")                    # handler.py:54-55
    inputs, forecast = inputs.contiguous(), forecast.contiguous()
    nxt = torch.empty_like(inputs)
    _lib.check(lib.stemgnn_roll_window(inputs.data_ptr(), forecast.data_ptr(), nxt.data_ptr(),
                                       forecast_steps.data_ptr(), B, W, L, N, int(step), int(horizon), _stream()),
               "roll_window")
    return nxt


def roll_window_quantile(inputs, forecast, forecast_steps, step, horizon, point):
    """roll_window for a quantile forecast [B,Q,L,N] (``stemgnn_roll_window_quantile``): the next inputs are built from the point
    row forecast[:, point] exactly as roll_window builds them, and all Q rows go to forecast_steps [B,Q,horizon,N]."""
    lib = _lib.load()
    _require_gpu(inputs, "inputs")
    _require_gpu(forecast, "forecast")
    B, W, N = inputs.shape
    if forecast.dim() != 4 or forecast.shape[0] != B or forecast.shape[3] != N:
        raise _lib.StemGNNHipError(f"roll_window_quantile: forecast must be [B,Q,L,N], got {tuple(forecast.shape)}")
    Q, L = forecast.shape[1], forecast.shape[2]
    if L == 0:
        raise Exception("Get blank inference result")                    # handler.py:54-55
    if tuple(forecast_steps.shape) != (B, Q, int(horizon), N) or not forecast_steps.is_contiguous():
        raise _lib.StemGNNHipError(f"roll_window_quantile: forecast_steps must be a contiguous [B,Q,horizon,N] tensor, got "
                                   f"{tuple(forecast_steps.shape)}")
    inputs, forecast = inputs.contiguous(), forecast.contiguous()
    nxt = torch.empty_like(inputs)
    _lib.check(lib.stemgnn_roll_window_quantile(inputs.data_ptr(), forecast.data_ptr(), nxt.data_ptr(),
                                                forecast_steps.data_ptr(), B, W, L, N, Q, int(point), int(step), int(horizon),
                                                _stream()), "roll_window_quantile")
    return nxt


def quantile_metrics(target, forecast, quantiles, mul=None, add=None, ignore_nan=False):
    """target [count,H,N], forecast [count,Q,H,N] fp32 -> float64 device vector overall[K] | by_step[K][H] with P = Q // 2,
    K = 2 Q + 2 P + 1: pinball[Q] | coverage[Q] | interval coverage[P] | interval width[P] | crossing rate
    (``stemgnn_quantile_metrics``; ignore_nan: the ``_masked`` entry, NaN targets left out everywhere)."""
    lib = _lib.load()
    _require_gpu(target, "target")
    _require_gpu(forecast, "forecast")
    Q = len(quantiles)
    if target.dim() != 3 or forecast.dim() != 4 or forecast.shape[1] != Q or \
            (forecast.shape[0],) + tuple(forecast.shape[2:]) != tuple(target.shape):
        raise _lib.StemGNNHipError(f"quantile_metrics: target must be [count,H,N] and forecast [count,{Q},H,N], got "
                                   f"{tuple(target.shape)} / {tuple(forecast.shape)}")
    target, forecast = target.contiguous(), forecast.contiguous()
    C, H, N = target.shape
    dev = target.device
    entry = lib.stemgnn_quantile_metrics_masked if ignore_nan else lib.stemgnn_quantile_metrics
    scratch = torch.empty(lib.stemgnn_quantile_scratch_doubles(C, Q, H, N), device=dev, dtype=torch.float64)
    out = torch.empty(lib.stemgnn_quantile_out_doubles(Q, H), device=dev, dtype=torch.float64)
    if mul is not None:
        mul = mul.to(device=dev, dtype=torch.float64).contiguous()
        add = add.to(device=dev, dtype=torch.float64).contiguous()
    _lib.check(entry(target.data_ptr(), forecast.data_ptr(), _lib.host_floats(quantiles, _lib.c_double),
                     mul.data_ptr() if mul is not None else None, add.data_ptr() if add is not None else None, C, Q, H, N,
                     scratch.data_ptr(), out.data_ptr(), _stream()), "quantile_metrics")
    return out


def _conformal_pairs(pairs, Q):
    pairs = [(int(lo), int(hi)) for lo, hi in pairs]
    if not pairs:
        raise ValueError("conformal: no pair of quantile rows")
    lo = (_lib.c_int * len(pairs))(*[p[0] for p in pairs])
    hi = (_lib.c_int * len(pairs))(*[p[1] for p in pairs])
    return len(pairs), lo, hi


def _fit_inputs(what, target, forecast, pairs, coverage):
    """The calibration set of a fit, checked: target [count,H,N] and forecast [count,Q,H,N] on one device, one coverage per
    pair.  Returns (target, forecast), contiguous, and (P, lo, hi)."""
    _require_gpu(target, "target")
    _require_gpu(forecast, "forecast")
    if target.dim() != 3 or forecast.dim() != 4 or (forecast.shape[0],) + tuple(forecast.shape[2:]) != tuple(target.shape):
        raise _lib.StemGNNHipError(f"{what}: target must be [count,H,N] and forecast [count,Q,H,N], got "
                                   f"{tuple(target.shape)} / {tuple(forecast.shape)}")
    if target.device != forecast.device:
        raise _lib.StemGNNHipError(f"{what}: target is on {target.device}, forecast on {forecast.device}")
    P, lo, hi = _conformal_pairs(pairs, forecast.shape[1])
    if len(coverage) != P:
        raise ValueError(f"{what}: {P} pairs but {len(coverage)} coverages")
    return target.contiguous(), forecast.contiguous(), P, lo, hi


def _tables(lead, H, N, per_step, per_node):
    """The shape of offsets / counts: the tables of `lead` = (P,) or (K, P) over the groups [Hg, Ng]."""
    return tuple(lead) + (H if per_step else 1, N if per_node else 1)


def _fit_outputs(nbytes, shape, device):
    """(scratch, offsets, counts) of a fit whose tables have `shape`."""
    return (torch.empty(max(nbytes, 16), device=device, dtype=torch.uint8),
            torch.empty(shape, device=device, dtype=torch.float32), torch.empty(shape, device=device, dtype=torch.int64))


def _offsets_ok(what, offsets, shape, device, float32=True, contiguous=False):
    """offsets must be the tables `shape` on `device`; float32 / contiguous: whether the entry also insists on that.  Returns
    them contiguous."""
    if tuple(offsets.shape) != shape or offsets.device != device or (float32 and offsets.dtype != torch.float32) or \
            (contiguous and not offsets.is_contiguous()):
        want = ("contiguous " if contiguous else "") + ("float32 " if float32 else "")
        got = f"{offsets.dtype} " if float32 else ""
        raise _lib.StemGNNHipError(f"{what}: offsets must be {want}{shape} on {device}, got {got}{tuple(offsets.shape)} "
                                   f"on {offsets.device}")
    return offsets.contiguous()


def _out_like(what, forecast, out, float32=True):
    """out=None: a new tensor (and forecast made contiguous); otherwise forecast and out must be contiguous tensors of one
    shape on one device already (float32: whether the entry also insists on out's dtype).  Returns (forecast, out)."""
    if out is None:
        forecast = forecast.contiguous()
        return forecast, torch.empty_like(forecast)
    _require_gpu(out, "out")
    if not forecast.is_contiguous() or not out.is_contiguous() or out.shape != forecast.shape or \
            out.device != forecast.device or (float32 and out.dtype != torch.float32):
        raise _lib.StemGNNHipError(f"{what}: with out=, forecast and out must be contiguous {'float32 ' if float32 else ''}"
                                   f"tensors of one shape on one device")
    return forecast, out


def conformal_fit(target, forecast, pairs, coverage, per_step=True, per_node=False, ignore_nan=False):
    """Split-conformal offsets of the quantile pairs (``stemgnn_conformal_fit``): target [count,H,N], forecast [count,Q,H,N] fp32,
    pairs = P (lo, hi) rows, coverage = their P nominal coverages.  Returns (offsets fp32, counts int64), both device tensors
    [P, H if per_step else 1, N if per_node else 1]: per group the k-th smallest score max(f_lo - y, y - f_hi),
    k = ceil((m + 1) coverage (1 - 1e-12)) of its m scores, +inf where k > m.  ignore_nan: NaN targets are left out (otherwise
    they count as +inf)."""
    lib = _lib.load()
    target, forecast, P, lo, hi = _fit_inputs("conformal_fit", target, forecast, pairs, coverage)
    C, Q, H, N = forecast.shape
    nbytes = lib.stemgnn_conformal_scratch_bytes(C, H, N, P, int(bool(per_step)), int(bool(per_node)))
    scratch, offsets, counts = _fit_outputs(nbytes, _tables((P,), H, N, per_step, per_node), target.device)
    _lib.check(lib.stemgnn_conformal_fit(target.data_ptr(), forecast.data_ptr(), C, Q, H, N, P, lo, hi,
                                         _lib.host_floats(coverage, _lib.c_double), int(bool(per_step)), int(bool(per_node)),
                                         int(bool(ignore_nan)), scratch.data_ptr(), offsets.data_ptr(), counts.data_ptr(),
                                         _stream()), "conformal_fit")
    return offsets, counts


def conformal_apply(forecast, offsets, pairs, per_step=True, per_node=False, out=None):
    """forecast [count,Q,H,N] with the pairs' rows moved by the offsets of conformal_fit (``stemgnn_conformal_apply``): the low
    row minus, the high row plus, every other row copied.  out: a contiguous tensor of forecast's shape, or forecast itself
    (in place); a new tensor by default."""
    lib = _lib.load()
    _require_gpu(forecast, "forecast")
    _require_gpu(offsets, "offsets")
    if forecast.dim() != 4:
        raise _lib.StemGNNHipError(f"conformal_apply: forecast must be [count,Q,H,N], got {tuple(forecast.shape)}")
    C, Q, H, N = forecast.shape
    P, lo, hi = _conformal_pairs(pairs, Q)
    offsets = _offsets_ok("conformal_apply", offsets, _tables((P,), H, N, per_step, per_node), forecast.device, float32=False)
    forecast, out = _out_like("conformal_apply", forecast, out, float32=False)
    _lib.check(lib.stemgnn_conformal_apply(forecast.data_ptr(), offsets.data_ptr(), C, Q, H, N, P, lo, hi,
                                           int(bool(per_step)), int(bool(per_node)), out.data_ptr(), _stream()),
               "conformal_apply")
    return out


def _season(what, season):
    """(period, buckets, phase) as ints, refused here when it names no bucketing (so that the error names the reason)."""
    period, K, phase = (int(v) for v in season)
    if not (1 <= period < 2 ** 31 and 1 <= K <= period and 0 <= phase < period):
        raise ValueError(f"{what}: season (period, buckets, phase) = {(period, K, phase)} needs 1 <= buckets <= period < 2^31 "
                         f"and 0 <= phase < period")
    return period, K, phase


def _origins(what, origin, count, device):
    """origin: an int (row i has origin + i) or an int64 tensor [count] (a host tensor is moved to the device once);
    returns (device pointer or None, origin0, keep-alive)."""
    if torch.is_tensor(origin):
        if origin.dim() != 1 or origin.shape[0] != count or origin.dtype != torch.int64:
            raise _lib.StemGNNHipError(f"{what}: origin must be an int or an int64 tensor [{count}], got {origin.dtype} "
                                       f"{tuple(origin.shape)}")
        origin = origin.to(device).contiguous()
        return origin.data_ptr(), 0, origin
    return None, int(origin), None


def seasonal_fit(target, forecast, origin, pairs, coverage, season, per_step=True, per_node=False, ignore_nan=False):
    """conformal_fit per time-of-day bucket (``stemgnn_seasonal_fit``): step h of row i belongs to bucket
    ((o_i + h + phase) mod period) * K // period with o_i = origin + i (an int) or origin[i] (int64 [count]); season =
    (period, K, phase).  Returns (offsets fp32, counts int64) [K, P, Hg, Ng]: slice s is conformal_fit over the bucket's
    elements (+inf / 0 for an empty bucket)."""
    lib = _lib.load()
    target, forecast, P, lo, hi = _fit_inputs("seasonal_fit", target, forecast, pairs, coverage)
    C, Q, H, N = forecast.shape
    period, K, phase = _season("seasonal_fit", season)
    optr, origin0, keep = _origins("seasonal_fit", origin, C, target.device)
    nbytes = lib.stemgnn_seasonal_scratch_bytes(C, H, N, P, K, int(bool(per_step)), int(bool(per_node)))
    scratch, offsets, counts = _fit_outputs(nbytes, _tables((K, P), H, N, per_step, per_node), target.device)
    _lib.check(lib.stemgnn_seasonal_fit(target.data_ptr(), forecast.data_ptr(), optr, origin0, C, Q, H, N, P, lo, hi,
                                        _lib.host_floats(coverage, _lib.c_double), int(bool(per_step)), int(bool(per_node)),
                                        int(bool(ignore_nan)), period, K, phase, scratch.data_ptr(), offsets.data_ptr(),
                                        counts.data_ptr(), _stream()), "seasonal_fit")
    return offsets, counts


def seasonal_apply(forecast, offsets, origin, pairs, season, per_step=True, per_node=False, rearrange=False, out=None):
    """forecast [count,Q,H,N] with the pairs' rows of step h of row i moved by the offsets of bucket(o_i + h)
    (``stemgnn_seasonal_apply``); offsets [K,P,Hg,Ng] of seasonal_fit, origin and season as there.  rearrange: every column's
    Q values are first put in non-decreasing order (quantile_finish's stage a).  out: a contiguous tensor of forecast's shape,
    or forecast itself (in place); a new tensor by default."""
    lib = _lib.load()
    _require_gpu(forecast, "forecast")
    _require_gpu(offsets, "offsets")
    if forecast.dim() != 4 or forecast.dtype != torch.float32:
        raise _lib.StemGNNHipError(f"seasonal_apply: forecast must be float32 [count,Q,H,N], got {forecast.dtype} "
                                   f"{tuple(forecast.shape)}")
    C, Q, H, N = forecast.shape
    P, lo, hi = _conformal_pairs(pairs, Q)
    period, K, phase = _season("seasonal_apply", season)
    offsets = _offsets_ok("seasonal_apply", offsets, _tables((K, P), H, N, per_step, per_node), forecast.device)
    forecast, out = _out_like("seasonal_apply", forecast, out)
    optr, origin0, keep = _origins("seasonal_apply", origin, C, forecast.device)
    _lib.check(lib.stemgnn_seasonal_apply(forecast.data_ptr(), offsets.data_ptr(), optr, origin0, C, Q, H, N,
                                          int(bool(rearrange)), P, lo, hi, int(bool(per_step)), int(bool(per_node)), period, K,
                                          phase, out.data_ptr(), _stream()), "seasonal_apply")
    return out


def _finish_stages(what, forecast, offsets, pairs, per_step, per_node):
    """The calibration stage's arguments of quantile_finish / quantile_store, checked as conformal_apply checks them; returns
    (offsets pointer or None, P, lo, hi, keep-alive)."""
    if offsets is None:
        return None, 0, None, None, None
    _require_gpu(offsets, "offsets")
    if pairs is None:
        raise ValueError(f"{what}: offsets= needs pairs= (the (lo, hi) rows they belong to)")
    _, Q, H, N = forecast.shape
    P, lo, hi = _conformal_pairs(pairs, Q)
    offsets = _offsets_ok(what, offsets, _tables((P,), H, N, per_step, per_node), forecast.device)
    return offsets.data_ptr(), P, lo, hi, offsets


def quantile_finish(forecast, rearrange=False, offsets=None, pairs=None, per_step=True, per_node=False, out=None):
    """The finished rows of a quantile forecast [count,Q,H,N] (``stemgnn_quantile_finish``), one launch:
    rearrange: every column's Q values in non-decreasing order (``torch.sort(forecast, dim=1, stable=True).values`` bit for bit);
    offsets / pairs / per_step / per_node: then conformal_apply on that.  With neither, a copy.  out: a contiguous tensor of
    forecast's shape, or forecast itself (in place); a new tensor by default."""
    lib = _lib.load()
    _require_gpu(forecast, "forecast")
    if forecast.dim() != 4 or forecast.dtype != torch.float32:
        raise _lib.StemGNNHipError(f"quantile_finish: forecast must be float32 [count,Q,H,N], got {forecast.dtype} "
                                   f"{tuple(forecast.shape)}")
    optr, P, lo, hi, keep = _finish_stages("quantile_finish", forecast, offsets, pairs, per_step, per_node)
    forecast, out = _out_like("quantile_finish", forecast, out)
    C, Q, H, N = forecast.shape
    _lib.check(lib.stemgnn_quantile_finish(forecast.data_ptr(), C, Q, H, N, int(bool(rearrange)), optr, P, lo, hi,
                                           int(bool(per_step)), int(bool(per_node)), out.data_ptr(), _stream()),
               "quantile_finish")
    return out


def _store_shapes(what, steps, target, pos, out_forecast, out_target):
    _require_gpu(steps, "steps")
    if steps.dim() != 4:
        raise _lib.StemGNNHipError(f"{what}: steps must be [B,Q,H,N], got {tuple(steps.shape)}")
    B, Q, H, N = steps.shape
    if tuple(target.shape) != (B, H, N) or tuple(out_forecast.shape[1:]) != (Q, H, N) or out_forecast.dim() != 4 or \
            tuple(out_target.shape) != (out_forecast.shape[0], H, N):
        raise _lib.StemGNNHipError(f"{what}: shape mismatch")
    for t, name in ((steps, "steps"), (target, "target"), (out_forecast, "out_forecast"), (out_target, "out_target")):
        if t.device != steps.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"{what}: {name} must be a contiguous float32 tensor on the steps' device")
    if pos.dtype != torch.int64 or pos.device != steps.device:
        raise _lib.StemGNNHipError(f"{what}: pos must be an int64 tensor on the steps' device")
    return B, Q, H, N


def quantile_store(steps, target, pos, out_forecast, out_target, rearrange=False, offsets=None, pairs=None, per_step=True,
                   per_node=False):
    """Result slabs of engine.QuantileForecastStep (``stemgnn_quantile_store``): out_forecast[pos + b] = the finished steps[b]
    (quantile_finish's two stages) and out_target[pos + b] = target[b], with the row position read on the device (pos: int64[1]);
    rows at or beyond the slabs' capacity are dropped.  steps [B,Q,H,N], target [B,H,N], slabs [capacity,Q,H,N] / [capacity,H,N]."""
    lib = _lib.load()
    B, Q, H, N = _store_shapes("quantile_store", steps, target, pos, out_forecast, out_target)
    optr, P, lo, hi, keep = _finish_stages("quantile_store", steps, offsets, pairs, per_step, per_node)
    _lib.check(lib.stemgnn_quantile_store(steps.data_ptr(), target.data_ptr(), pos.data_ptr(), B, Q, H, N,
                                          int(bool(rearrange)), optr, P, lo, hi, int(bool(per_step)), int(bool(per_node)),
                                          out_forecast.data_ptr(), out_target.data_ptr(), out_forecast.shape[0], _stream()),
               "quantile_store")


def quantile_store_seasonal(steps, target, pos, out_forecast, out_target, rearrange=False, offsets=None, pairs=None,
                            per_step=True, per_node=False, seasonal=None, t_dev=None):
    """quantile_store with the offsets of a seasonal calibrator (``stemgnn_quantile_store_seasonal``): offsets are the [K,P,Hg,Ng]
    tables of seasonal_fit, seasonal = (period, K, phase), t_dev int64[1] on the device; batch row b has origin t_dev[0] + b and
    its step h is widened with the tables' slice bucket(t_dev[0] + b + h), worked out on the device."""
    lib = _lib.load()
    B, Q, H, N = _store_shapes("quantile_store_seasonal", steps, target, pos, out_forecast, out_target)
    if seasonal is None or offsets is None or pairs is None:
        raise ValueError("quantile_store_seasonal: needs seasonal= (period, K, phase), offsets= (the [K,P,Hg,Ng] tables) and pairs=")
    period, K, phase = _season("quantile_store_seasonal", seasonal)
    if t_dev is None or t_dev.dtype != torch.int64 or t_dev.device != steps.device or t_dev.numel() < 1:
        raise _lib.StemGNNHipError("quantile_store_seasonal: t_dev must be an int64 tensor on the steps' device")
    P, lo, hi = _conformal_pairs(pairs, Q)
    _offsets_ok("quantile_store_seasonal", offsets, _tables((K, P), H, N, per_step, per_node), steps.device, contiguous=True)
    _lib.check(lib.stemgnn_quantile_store_seasonal(steps.data_ptr(), target.data_ptr(), pos.data_ptr(), t_dev.data_ptr(),
                                                   B, Q, H, N, int(bool(rearrange)), offsets.data_ptr(), P, lo, hi,
                                                   int(bool(per_step)), int(bool(per_node)), period, K, phase,
                                                   out_forecast.data_ptr(), out_target.data_ptr(), out_forecast.shape[0],
                                                   _stream()), "quantile_store_seasonal")


def scenario_rank(tau, S):
    """The 1-based rank of level `tau` among S path values (``stemgnn_scenario_rank``):
    min(S, max(1, ceil(tau * S * (1 - 1e-12)))) in fp64."""
    return int(_lib.load().stemgnn_scenario_rank(float(tau), int(S)))


def scenario_roll(inputs, forecast, quantiles, paths, step, origin0=0, seed=0, offset=0, coupling="independent",
                  tails="linear", bands=None, last=False, uniforms=None):
    """One round of a sampled roll (``stemgnn_scenario_roll``): every path draws its next window rows from the quantile
    function through (quantiles, forecast column) -- the definition in include/stemgnn_hip.h -- instead of taking the point row.
    inputs [Bsrc,W,N], forecast [Bsrc,Q,L,N], paths [Bo,S,horizon,N] (rows step .. step + L - 1 are written).  Bsrc == Bo is
    round 0 (fan = S: every path of an origin reads the origin's one forecast) and takes bands [Bo,Q,horizon,N], which receives
    the model's own rows of those steps; Bsrc == Bo * S is a later round (fan = 1, no bands).  origin0: the global index of
    the batch's first origin; seed / offset: the Philox key and the counter's high words.  uniforms: a float32 tensor
    [Bo,S,L,N] whose values take the place of the Philox uniforms (``stemgnn_scenario_roll_given``; `copula_uniforms` makes
    correlated ones); coupling, origin0, seed and offset are then ignored, and values inside (0, 1) are the caller's contract.
    Returns the next inputs [Bo * S,W,N], or None with last=True (the round whose windows nobody reads)."""
    lib = _lib.load()
    _require_gpu(inputs, "inputs")
    _require_gpu(forecast, "forecast")
    _require_gpu(paths, "paths")
    if inputs.dim() != 3 or forecast.dim() != 4 or paths.dim() != 4:
        raise _lib.StemGNNHipError(f"scenario_roll: inputs [Bsrc,W,N], forecast [Bsrc,Q,L,N] and paths [Bo,S,horizon,N] wanted, "
                                   f"got {tuple(inputs.shape)}, {tuple(forecast.shape)}, {tuple(paths.shape)}")
    Bsrc, W, N = inputs.shape
    Q, L = forecast.shape[1], forecast.shape[2]
    Bo, S, horizon = paths.shape[:3]
    if L == 0:
        raise Exception("Get blank inference result")                    # handler.py:54-55
    if forecast.shape[0] != Bsrc or forecast.shape[3] != N or paths.shape[3] != N or len(quantiles) != Q:
        raise _lib.StemGNNHipError(f"scenario_roll: shape mismatch: inputs {tuple(inputs.shape)}, forecast "
                                   f"{tuple(forecast.shape)}, paths {tuple(paths.shape)}, {len(quantiles)} levels")
    if Bsrc == Bo * S and (S > 1 or bands is None):
        fan = 1
    elif Bsrc == Bo:
        fan = S
    else:
        raise _lib.StemGNNHipError(f"scenario_roll: {Bsrc} source windows fit neither {Bo} origins nor {Bo} x {S} paths")
    for t, name in ((inputs, "inputs"), (forecast, "forecast"), (paths, "paths")) + (() if bands is None else ((bands, "bands"),)):
        if t.device != inputs.device or t.dtype != torch.float32:
            raise _lib.StemGNNHipError(f"scenario_roll: {name} must be a float32 tensor on the inputs' device")
    if not paths.is_contiguous():
        raise _lib.StemGNNHipError("scenario_roll: paths must be contiguous")
    if bands is not None and (tuple(bands.shape) != (Bo, Q, horizon, N) or not bands.is_contiguous()):
        raise _lib.StemGNNHipError(f"scenario_roll: bands must be a contiguous [Bo,Q,horizon,N] tensor, got {tuple(bands.shape)}")
    if (uniforms is None and coupling not in _lib.SG_SCENARIO_COUPLING) or tails not in _lib.SG_SCENARIO_TAILS:
        raise ValueError(f"scenario_roll: coupling is one of {tuple(_lib.SG_SCENARIO_COUPLING)}, tails one of "
                         f"{tuple(_lib.SG_SCENARIO_TAILS)}, got {coupling!r}, {tails!r}")
    inputs, forecast = inputs.contiguous(), forecast.contiguous()
    nxt = None if last else torch.empty(Bo * S, W, N, device=inputs.device, dtype=torch.float32)
    if uniforms is not None:
        if tuple(uniforms.shape) != (Bo, S, L, N) or uniforms.dtype != torch.float32 or uniforms.device != inputs.device or \
                not uniforms.is_contiguous():
            raise _lib.StemGNNHipError(f"scenario_roll: uniforms must be a contiguous float32 {(Bo, S, L, N)} tensor on the "
                                       f"inputs' device, got {uniforms.dtype} {tuple(uniforms.shape)} on {uniforms.device}")
        _lib.check(lib.stemgnn_scenario_roll_given(inputs.data_ptr(), forecast.data_ptr(), _lib.host_floats(quantiles),
                                                   uniforms.data_ptr(), Bo, S, fan, W, L, N, Q, int(step), horizon,
                                                   _lib.SG_SCENARIO_TAILS[tails], None if nxt is None else nxt.data_ptr(),
                                                   paths.data_ptr(), None if bands is None else bands.data_ptr(), _stream()),
                   "scenario_roll")
        return nxt
    mask = (1 << 64) - 1
    _lib.check(lib.stemgnn_scenario_roll(inputs.data_ptr(), forecast.data_ptr(), _lib.host_floats(quantiles), Bo, S, fan, W, L,
                                         N, Q, int(step), horizon, int(origin0), int(seed) & mask, int(offset) & mask,
                                         _lib.SG_SCENARIO_COUPLING[coupling], _lib.SG_SCENARIO_TAILS[tails],
                                         None if nxt is None else nxt.data_ptr(), paths.data_ptr(),
                                         None if bands is None else bands.data_ptr(), _stream()), "scenario_roll")
    return nxt


def scenario_bands(paths, quantiles, step_from, bands):
    """The bands of sampled paths (``stemgnn_scenario_bands``): bands[b, q, h, n] = the scenario_rank(quantiles[q], S)-th
    smallest of paths[b, :, h, n] for every step h >= step_from (NaN last: a selection, bit patterns kept); the steps below
    step_from are left as they are.  paths [Bo,S,horizon,N], bands [Bo,Q,horizon,N], contiguous float32; returns bands."""
    lib = _lib.load()
    _require_gpu(paths, "paths")
    _require_gpu(bands, "bands")
    if paths.dim() != 4 or bands.dim() != 4:
        raise _lib.StemGNNHipError(f"scenario_bands: paths [Bo,S,horizon,N] and bands [Bo,Q,horizon,N] wanted, got "
                                   f"{tuple(paths.shape)}, {tuple(bands.shape)}")
    Bo, S, horizon, N = paths.shape
    Q = len(quantiles)
    if tuple(bands.shape) != (Bo, Q, horizon, N):
        raise _lib.StemGNNHipError(f"scenario_bands: bands must be {(Bo, Q, horizon, N)}, got {tuple(bands.shape)}")
    for t, name in ((paths, "paths"), (bands, "bands")):
        if t.device != paths.device or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"scenario_bands: {name} must be a contiguous float32 tensor on the paths' device")
    ranks = (ctypes.c_int * Q)(*[scenario_rank(t, S) for t in quantiles])
    _lib.check(lib.stemgnn_scenario_bands(paths.data_ptr(), Bo, S, horizon, N, Q, ranks, int(step_from), bands.data_ptr(),
                                          _stream()), "scenario_bands")
    return bands


def copula_pit(y, y_hat, quantiles, tails="linear"):
    """The probability integral transform of y under the forecast's quantile function (``stemgnn_copula_pit``; the exact
    inverse of scenario_roll's draw, defined in include/stemgnn_hip.h): y [count,H,N], y_hat [count,Q,H,N], contiguous float32
    on one device -> u [count,H,N] in [2^-24, 1 - 2^-24]; NaN where y or a value of its column is NaN (missing)."""
    lib = _lib.load()
    _require_gpu(y, "y")
    _require_gpu(y_hat, "y_hat")
    if y.dim() != 3 or y_hat.dim() != 4 or (y_hat.shape[0],) + tuple(y_hat.shape[2:]) != tuple(y.shape) or \
            y_hat.shape[1] != len(quantiles):
        raise _lib.StemGNNHipError(f"copula_pit: y must be [count,H,N] and y_hat [count,{len(quantiles)},H,N], got "
                                   f"{tuple(y.shape)} / {tuple(y_hat.shape)}")
    if y.device != y_hat.device or not y.is_contiguous() or not y_hat.is_contiguous():
        raise _lib.StemGNNHipError("copula_pit: y and y_hat must be contiguous tensors on one device")
    if tails not in _lib.SG_SCENARIO_TAILS:
        raise ValueError(f"copula_pit: tails is one of {tuple(_lib.SG_SCENARIO_TAILS)}, got {tails!r}")
    C, Q, H, N = y_hat.shape
    u = torch.empty_like(y)
    _lib.check(lib.stemgnn_copula_pit(y.data_ptr(), y_hat.data_ptr(), _lib.host_floats(quantiles), C, H, N, Q,
                                      _lib.SG_SCENARIO_TAILS[tails], u.data_ptr(), _stream()), "copula_pit")
    return u


def copula_gram(u):
    """Pairwise-complete second moments of the normal scores z = normcdfinv(u) (``stemgnn_copula_gram``): u [M,N] (or
    [count,H,N], pooled over its leading axes), contiguous float32, NaN = absent -> (pairs int64 [N,N], sums float64 [3,N,N] =
    sum z_i z_j | sum z_i | sum z_i^2 over the rows where i and j are both present), on the device, no sync."""
    lib = _lib.load()
    _require_gpu(u, "u")
    if u.dim() < 2 or not u.is_contiguous():
        raise _lib.StemGNNHipError(f"copula_gram: u must be a contiguous [M,N] or [count,H,N] tensor, got {tuple(u.shape)}")
    N = u.shape[-1]
    M = u.numel() // max(N, 1)
    words = lib.stemgnn_copula_scratch_doubles(M, N)
    if words == 0:
        raise _lib.StemGNNHipError(f"copula_gram: {M} rows of {N} nodes are outside the entry's range (SG_EINVAL)")
    scratch = torch.empty(words, device=u.device, dtype=torch.float64)
    pairs = torch.empty(N, N, device=u.device, dtype=torch.int64)
    sums = torch.empty(3, N, N, device=u.device, dtype=torch.float64)
    _lib.check(lib.stemgnn_copula_gram(u.data_ptr(), M, N, scratch.data_ptr(), pairs.data_ptr(), sums.data_ptr(), _stream()),
               "copula_gram")
    return pairs, sums


def copula_uniforms(factor_t, Bo, S, L, step, horizon, origin0=0, seed=0, offset=0, step_factor=None):
    """The correlated uniforms of one round (``stemgnn_copula_uniforms``): factor_t [N,N] float32 with factor_t[k, n] = L[n, k],
    L the lower Cholesky factor of the nodes' correlation matrix (the entries with k > n are never read into the result) ->
    u [Bo,S,L,N] = normcdf(L e) clamped to [2^-24, 1 - 2^-24], e the standard normal of the Philox word that
    coupling="independent" takes for that (global origin, path, step, node).  step_factor: a contiguous float32 [L,L] tensor on
    factor_t's device, the lower Cholesky factor A of a correlation over the round's steps (entries above the diagonal are never
    read); the L steps of a path are then coupled as well, e <- A e along the steps ahead of the node sum
    (``stemgnn_copula_uniforms_steps``; L <= 16 for N <= 512, L <= 4 beyond)."""
    lib = _lib.load()
    _require_gpu(factor_t, "factor_t")
    if factor_t.dim() != 2 or factor_t.shape[0] != factor_t.shape[1] or not factor_t.is_contiguous():
        raise _lib.StemGNNHipError(f"copula_uniforms: factor_t must be a contiguous [N,N] tensor, got {tuple(factor_t.shape)}")
    N = factor_t.shape[0]
    if step_factor is not None and (not torch.is_tensor(step_factor) or tuple(step_factor.shape) != (int(L), int(L)) or
                                    step_factor.dtype != torch.float32 or step_factor.device != factor_t.device or
                                    not step_factor.is_contiguous()):
        got = f"{step_factor.dtype} {tuple(step_factor.shape)} on {step_factor.device}" if torch.is_tensor(step_factor) else \
            type(step_factor).__name__
        raise _lib.StemGNNHipError(f"copula_uniforms: step_factor must be a contiguous float32 {(int(L), int(L))} tensor on "
                                   f"factor_t's device, got {got}")
    u = torch.empty(int(Bo), int(S), int(L), N, device=factor_t.device, dtype=torch.float32)
    mask = (1 << 64) - 1
    if step_factor is None:
        _lib.check(lib.stemgnn_copula_uniforms(factor_t.data_ptr(), int(Bo), int(S), int(L), N, int(step), int(horizon),
                                               int(origin0), int(seed) & mask, int(offset) & mask, u.data_ptr(), _stream()),
                   "copula_uniforms")
    else:
        _lib.check(lib.stemgnn_copula_uniforms_steps(factor_t.data_ptr(), step_factor.data_ptr(), int(Bo), int(S), int(L), N,
                                                     int(step), int(horizon), int(origin0), int(seed) & mask, int(offset) & mask,
                                                     u.data_ptr(), _stream()), "copula_uniforms")
    return u


def ensemble_scores(y, paths, mul=None, add=None, ignore_nan=False, fair=False):
    """Scores of sampled paths against what happened (``stemgnn_ensemble_scores``; the definitions are in include/stemgnn_hip.h):
    y [count,H,N], paths [count,S,H,N] (rolling_scenarios' layout), contiguous float32 on one device ->
    (out float64 [6 * (1 + H)] = overall | by_step[6][H] of mean CRPS, mean energy score, RMSE of the ensemble mean, spread,
    valid elements, valid rows; hist int64 [H, S + 1], the rank histogram per step), both on the device, no sync.
    mul / add: per-node de-normalisation in fp64 ahead of everything.  ignore_nan: the ``_masked`` entry, NaN targets are missing.
    fair: the pair terms are divided by S (S - 1) instead of S^2 (unbiased in S; needs S >= 2)."""
    if y.dim() != 3 or paths.dim() != 4 or (paths.shape[0],) + tuple(paths.shape[2:]) != tuple(y.shape):
        raise _lib.StemGNNHipError(f"ensemble_scores: y must be [count,H,N] and paths [count,S,H,N], got "
                                   f"{tuple(y.shape)} / {tuple(paths.shape)}")
    for t, name in ((y, "y"), (paths, "paths")):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"ensemble_scores: {name} must be a contiguous float32 tensor, got {t.dtype}, "
                                       f"strides {tuple(t.stride())}")
    if (mul is None) != (add is None):
        raise _lib.StemGNNHipError("ensemble_scores: mul and add go together")
    C, S, H, N = paths.shape
    if not 1 <= S <= 1024 or (fair and S < 2):
        raise _lib.StemGNNHipError(f"ensemble_scores: {S} paths (1 to 1024 are scored; fair=True needs at least 2)")
    _require_gpu(y, "y")
    _require_gpu(paths, "paths")
    if paths.device != y.device:
        raise _lib.StemGNNHipError(f"ensemble_scores: y is on {y.device}, paths on {paths.device}")
    lib = _lib.load()
    dev = y.device
    entry = lib.stemgnn_ensemble_scores_masked if ignore_nan else lib.stemgnn_ensemble_scores
    scratch = torch.empty(lib.stemgnn_ensemble_scratch_doubles(C, S, H, N), device=dev, dtype=torch.float64)
    out = torch.empty(lib.stemgnn_ensemble_out_doubles(H), device=dev, dtype=torch.float64)
    hist = torch.empty(H, S + 1, device=dev, dtype=torch.int64)
    if mul is not None:
        mul = mul.to(device=dev, dtype=torch.float64).contiguous()
        add = add.to(device=dev, dtype=torch.float64).contiguous()
    _lib.check(entry(y.data_ptr(), paths.data_ptr(), mul.data_ptr() if mul is not None else None,
                     add.data_ptr() if add is not None else None, C, S, H, N, int(bool(fair)), scratch.data_ptr(),
                     out.data_ptr(), hist.data_ptr(), _stream()), "ensemble_scores")
    return out, hist


def _per_column(what, name, v, n):
    """a scalar or n values -> a float64 host-or-device tensor [n] (not yet moved); refuses any other shape"""
    v = v.detach() if torch.is_tensor(v) else torch.as_tensor(np.asarray(v, dtype=np.float64))
    if v.dim() == 0:
        v = v.reshape(1).expand(n)
    if v.dim() != 1 or v.shape[0] != n or v.is_complex():
        raise _lib.StemGNNHipError(f"{what}: {name} must be a scalar or {n} values, got shape {tuple(v.shape)}")
    return v


def _denorm_pair(what, mul, add, n):
    if (mul is None) != (add is None):
        raise _lib.StemGNNHipError(f"{what}: mul and add go together")
    if mul is None:
        return None, None
    return _per_column(what, "mul", mul, n), _per_column(what, "add", add, n)


def _f64_on(v, device):
    return None if v is None else v.to(device=device, dtype=torch.float64).contiguous()


def scenario_aggregate(x, weights, mul=None, add=None):
    """Weighted aggregates over node sets (``stemgnn_scenario_aggregate``; the definition is in include/stemgnn_hip.h):
    x [..., N] contiguous float32 on the device (paths [count,S,H,N], targets [count,H,N], ..), weights [R,N] (any real dtype,
    used as float64; math_utils.group_weights makes them), R <= 32, N <= 4096 -> out [..., R] float32 with
    out[.., r] = sum over the nodes with a non-zero weight of weights[r, n] * (x[.., n] * mul[n] + add[n]), in fp64.
    A node of weight 0 is not read into the sum (its NaN stays out); the same bits however the leading axes are batched."""
    what = "scenario_aggregate"
    if not torch.is_tensor(x) or x.dim() < 1 or x.shape[-1] < 1 or x.numel() == 0:
        raise _lib.StemGNNHipError(f"{what}: x must be a non-empty [..., N] tensor, got "
                                   f"{tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    N = int(x.shape[-1])
    if not torch.is_tensor(weights) or weights.dim() != 2 or weights.shape[1] != N or weights.shape[0] < 1 or \
            weights.is_complex():
        raise _lib.StemGNNHipError(f"{what}: weights must be a [R,{N}] tensor, got "
                                   f"{tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__}")
    R = int(weights.shape[0])
    if R > 32 or N > 4096:
        raise _lib.StemGNNHipError(f"{what}: at most 32 groups over at most 4096 nodes, got R = {R}, N = {N}")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: x must be a contiguous float32 tensor, got {x.dtype}, strides {tuple(x.stride())}")
    mul, add = _denorm_pair(what, mul, add, N)
    rows = x.numel() // N
    if rows * R >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {rows} rows x {R} groups do not fit the entry's range (2^31)")
    _require_gpu(x, "x")
    lib = _lib.load()
    dev = x.device
    weights, mul, add = _f64_on(weights.detach(), dev), _f64_on(mul, dev), _f64_on(add, dev)
    out = torch.empty(tuple(x.shape[:-1]) + (R,), device=dev, dtype=torch.float32)
    _lib.check(lib.stemgnn_scenario_aggregate(x.data_ptr(), weights.data_ptr(), None if mul is None else mul.data_ptr(),
                                              None if add is None else add.data_ptr(), rows, N, R, out.data_ptr(), _stream()),
               what)
    return out


def scenario_events(paths, threshold, above=True, min_run=1, mul=None, add=None):
    """Crossing counts of sampled paths (``stemgnn_scenario_events``; the definition is in include/stemgnn_hip.h):
    paths [count,S,H,M] contiguous float32 on the device (M: nodes, or the groups of scenario_aggregate), threshold a scalar or
    M values (float64, in the units of paths * mul + add) -> counts int32 [count, 2H+1, M]: rows 0..H-1 the paths in the event
    per step, rows H..2H-1 the paths whose FIRST step in the event it is, row 2H the paths with at least `min_run` consecutive
    steps in it.  above: the event is value > threshold (True) or value < threshold (False), strict, never true of a NaN."""
    what = "scenario_events"
    if not torch.is_tensor(paths) or paths.dim() != 4 or paths.numel() == 0:
        raise _lib.StemGNNHipError(f"{what}: paths must be a non-empty [count,S,H,M] tensor, got "
                                   f"{tuple(paths.shape) if torch.is_tensor(paths) else type(paths).__name__}")
    if paths.dtype != torch.float32 or not paths.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: paths must be a contiguous float32 tensor, got {paths.dtype}, strides "
                                   f"{tuple(paths.stride())}")
    C, S, H, M = (int(v) for v in paths.shape)
    if S > 1024 or H > 256:
        raise _lib.StemGNNHipError(f"{what}: at most 1024 paths of at most 256 steps, got S = {S}, H = {H}")
    if isinstance(min_run, bool) or int(min_run) != min_run or not 1 <= int(min_run) <= H:
        raise _lib.StemGNNHipError(f"{what}: min_run must be an integer within [1, {H}], got {min_run!r}")
    threshold = _per_column(what, "threshold", threshold, M)
    mul, add = _denorm_pair(what, mul, add, M)
    _require_gpu(paths, "paths")
    lib = _lib.load()
    dev = paths.device
    threshold, mul, add = _f64_on(threshold, dev), _f64_on(mul, dev), _f64_on(add, dev)
    counts = torch.empty(C, 2 * H + 1, M, device=dev, dtype=torch.int32)
    _lib.check(lib.stemgnn_scenario_events(paths.data_ptr(), threshold.data_ptr(), None if mul is None else mul.data_ptr(),
                                           None if add is None else add.data_ptr(), C, S, H, M, int(bool(above)), int(min_run),
                                           counts.data_ptr(), _stream()), what)
    return counts


def _reduce_paths(what, paths):
    """paths [count,S,H,M] contiguous float32 (checked on the host, the device last) -> (count, S, H, M)"""
    if not torch.is_tensor(paths) or paths.dim() != 4 or paths.numel() == 0:
        raise _lib.StemGNNHipError(f"{what}: paths must be a non-empty [count,S,H,M] tensor, got "
                                   f"{tuple(paths.shape) if torch.is_tensor(paths) else type(paths).__name__}")
    if paths.dtype != torch.float32 or not paths.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: paths must be a contiguous float32 tensor, got {paths.dtype}, strides "
                                   f"{tuple(paths.stride())}")
    C, S, H, M = (int(v) for v in paths.shape)
    if S > 1024:
        raise _lib.StemGNNHipError(f"{what}: at most 1024 paths, got S = {S}")
    if S * H * M >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {S} paths of {H} x {M} values do not fit the entry's range (2^31)")
    return C, S, H, M


def _reduce_scale(what, scale, H, M):
    """scale: None, a scalar, [M] or [H,M] -> None or a float64 tensor [H * M] (not yet moved)"""
    if scale is None:
        return None
    v = scale.detach() if torch.is_tensor(scale) else torch.as_tensor(np.asarray(scale, dtype=np.float64))
    if v.is_complex() or v.dim() > 2 or (v.dim() == 1 and v.shape[0] != M) or (v.dim() == 2 and tuple(v.shape) != (H, M)):
        raise _lib.StemGNNHipError(f"{what}: scale must be a scalar, [{M}] or [{H},{M}], got shape {tuple(v.shape)}")
    return v.to(torch.float64).expand(H, M).reshape(H * M)


def _reduce_flag(what, squared):
    if not isinstance(squared, (bool, np.bool_, int)) or squared not in (0, 1):
        raise _lib.StemGNNHipError(f"{what}: squared must be True or False, got {squared!r}")
    return int(bool(squared))


def _reduce_keep(what, keep, S):
    if isinstance(keep, bool) or not isinstance(keep, (int, np.integer)) or not 1 <= int(keep) <= S:
        raise _lib.StemGNNHipError(f"{what}: keep must be an integer within [1, {S}] (S = {S} paths), got {keep!r}")
    return int(keep)


def _reduce_batch(what, S, max_scratch_bytes):
    """origins per call: D [batch,S,S] float64 within max_scratch_bytes and within the entries' range (2^31 elements)"""
    if isinstance(max_scratch_bytes, bool) or int(max_scratch_bytes) != max_scratch_bytes or int(max_scratch_bytes) < S * S * 8:
        raise _lib.StemGNNHipError(f"{what}: max_scratch_bytes must hold one origin's [S,S] float64 distances "
                                   f"({S * S * 8} bytes), got {max_scratch_bytes!r}")
    return max(1, min(int(max_scratch_bytes) // (S * S * 8), (2 ** 31 - 1) // (S * S)))


def _reduce_distances(what, distances, staged=False):
    """a caller's distances: a non-empty contiguous float64 [count,S,S] (staged: [count,T,S,S]) -> (count, S) ((count, T, S))"""
    dims, layout = (4, "[count,T,S,S]") if staged else (3, "[count,S,S]")
    if not torch.is_tensor(distances) or distances.dim() != dims or distances.shape[-2] != distances.shape[-1] or \
            distances.numel() == 0:
        raise _lib.StemGNNHipError(f"{what}: distances must be a non-empty {layout} tensor, got "
                                   f"{tuple(distances.shape) if torch.is_tensor(distances) else type(distances).__name__}")
    if distances.dtype != torch.float64 or not distances.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: distances must be a contiguous float64 tensor, got {distances.dtype}, strides "
                                   f"{tuple(distances.stride())}")
    return tuple(int(v) for v in distances.shape[:-1])


def _reduce_outputs(C, S, K, dev):
    """selected [C,K], counts [C,K], assign [C,S] int32 and cost [C,K] float64, uninitialised on dev"""
    return (torch.empty(C, K, device=dev, dtype=torch.int32), torch.empty(C, K, device=dev, dtype=torch.int32),
            torch.empty(C, S, device=dev, dtype=torch.int32), torch.empty(C, K, device=dev, dtype=torch.float64))


def scenario_distances(paths, scale=None, squared=False):
    """Pairwise distances of sampled paths (``stemgnn_scenario_distances``; the definition is in include/stemgnn_hip.h):
    paths [count,S,H,M] contiguous float32 on the device (M: nodes, or the groups of scenario_aggregate) ->
    D [count,S,S] float64, D[c,i,j] = sqrt(sum over (h, m) of ((x_i - x_j) * scale)^2) in fp64 from the differences; squared:
    without the root.  scale: a scalar, [M] or [H,M] (any real dtype, used as float64), e.g. 1 / std per node or a discount per
    step.  D equals its transpose bit for bit; coincident paths are at exactly 0; a NaN in a path reaches its row and column."""
    what = "scenario_distances"
    C, S, H, M = _reduce_paths(what, paths)
    scale = _reduce_scale(what, scale, H, M)
    squared = _reduce_flag(what, squared)
    if C * S * S >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {C} origins x {S} x {S} distances do not fit the entry's range (2^31); "
                                   "scenario_reduce walks the origins in batches")
    _require_gpu(paths, "paths")
    lib = _lib.load()
    scale = _f64_on(scale, paths.device)
    D = torch.empty(C, S, S, device=paths.device, dtype=torch.float64)
    _lib.check(lib.stemgnn_scenario_distances(paths.data_ptr(), None if scale is None else scale.data_ptr(), C, S, H * M,
                                              squared, D.data_ptr(), _stream()), what)
    return D


def scenario_reduce(paths, keep, scale=None, squared=False, distances=None, max_scratch_bytes=256 << 20):
    """Scenario reduction by forward selection (``stemgnn_scenario_distances`` + ``stemgnn_scenario_reduce``; the definition is
    in include/stemgnn_hip.h): of the S paths of every origin, `keep` representatives are picked greedily, each pick the one that
    most lowers the Kantorovich distance between the uniform ensemble and the kept set, and every path is assigned to its nearest
    kept one.  paths [count,S,H,M] contiguous float32 on the device; scale / squared: scenario_distances'.  Returns
      selected int32 [count,keep]  path indices in the order they were picked       counts int32 [count,keep]  paths assigned to each
      assign   int32 [count,S]     the position in 0 .. keep-1 every path went to   cost   float64 [count,keep]  the distance after
                                                                                   every pick (non-increasing)
    all on the device, no sync; the weights are counts / S.  An origin with a NaN or an infinity among its distances is refused:
    -1 / 0 / -1 / NaN, the others are not affected.  The origins are walked in batches whose [batch,S,S] float64 distances stay
    within max_scratch_bytes; the result is that of one call, bit for bit.
    distances [count,S,S] float64 (contiguous, on the device): any cost of the caller's, D[k,u] = moving path k onto path u;
    only the second entry runs, and paths may be None."""
    what = "scenario_reduce"
    if distances is None:
        C, S, H, M = _reduce_paths(what, paths)
        scale = _reduce_scale(what, scale, H, M)
        squared = _reduce_flag(what, squared)
        source = paths
    else:
        C, S = _reduce_distances(what, distances)
        if S > 1024:
            raise _lib.StemGNNHipError(f"{what}: at most 1024 paths, got S = {S}")
        if paths is not None and (not torch.is_tensor(paths) or paths.dim() != 4 or tuple(paths.shape[:2]) != (C, S)):
            raise _lib.StemGNNHipError(f"{what}: paths must be [count,S,H,M] with the distances' count = {C} and S = {S}, got "
                                       f"{tuple(paths.shape) if torch.is_tensor(paths) else type(paths).__name__}")
        source = distances
    K = _reduce_keep(what, keep, S)
    batch = _reduce_batch(what, S, max_scratch_bytes)
    if not source.is_cuda:
        raise _lib.StemGNNHipError(f"{what}: {'paths' if distances is None else 'distances'} is on {source.device}: "
                                   "stemgnn_amd runs only on a HIP device (no CPU fallback)")
    lib = _lib.load()
    dev = source.device
    selected, counts, assign, cost = _reduce_outputs(C, S, K, dev)
    if distances is None:
        scale = _f64_on(scale, dev)
        D = torch.empty(min(batch, C), S, S, device=dev, dtype=torch.float64)
    for lo in range(0, C, batch):
        n = min(batch, C - lo)
        if distances is None:
            _lib.check(lib.stemgnn_scenario_distances(paths[lo:lo + n].data_ptr(), None if scale is None else scale.data_ptr(),
                                                      n, S, H * M, squared, D.data_ptr(), _stream()), "scenario_distances")
            d_ptr = D.data_ptr()
        else:
            d_ptr = distances[lo:lo + n].data_ptr()
        _lib.check(lib.stemgnn_scenario_reduce(d_ptr, n, S, K, selected[lo:lo + n].data_ptr(), counts[lo:lo + n].data_ptr(),
                                               assign[lo:lo + n].data_ptr(), cost[lo:lo + n].data_ptr(), _stream()), what)
    return selected, counts, assign, cost


def _weighted_set(what, paths, mult, total, most=256):
    """paths [count,K,H,M] contiguous float32, mult int32 [count,K] contiguous, total the common sum W in [1, 2^24] (checked on
    the host, the device last) -> (count, K, H, M, W)"""
    if not torch.is_tensor(paths) or paths.dim() != 4 or paths.numel() == 0:
        raise _lib.StemGNNHipError(f"{what}: paths must be a non-empty [count,K,H,N] tensor, got "
                                   f"{tuple(paths.shape) if torch.is_tensor(paths) else type(paths).__name__}")
    if paths.dtype != torch.float32 or not paths.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: paths must be a contiguous float32 tensor, got {paths.dtype}, strides "
                                   f"{tuple(paths.stride())}")
    C, K, H, M = (int(v) for v in paths.shape)
    if K > most:
        raise _lib.StemGNNHipError(f"{what}: at most {most} weighted members, got K = {K}")
    if K * H * M >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {K} members of {H} x {M} values do not fit the entry's range (2^31)")
    W = _weighted_mult(what, mult, total, C, K)
    if mult.device != paths.device:
        raise _lib.StemGNNHipError(f"{what}: paths is on {paths.device}, mult on {mult.device}")
    return C, K, H, M, W


def _weighted_mult(what, mult, total, C, K):
    if not torch.is_tensor(mult) or tuple(mult.shape) != (C, K) or mult.dtype != torch.int32 or not mult.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: mult must be a contiguous int32 [{C},{K}] tensor of multiplicities, got "
                                   f"{(str(mult.dtype) + ' ' + str(tuple(mult.shape))) if torch.is_tensor(mult) else type(mult).__name__}")
    if isinstance(total, bool) or not isinstance(total, (int, np.integer)) or not 1 <= int(total) <= 2 ** 24:
        raise _lib.StemGNNHipError(f"{what}: total must be an integer within [1, 2^24] (the multiplicities' common sum), got "
                                   f"{total!r}")
    return int(total)


def weighted_bands(paths, mult, total, quantiles, out=None):
    """The bands of a weighted scenario set (``stemgnn_weighted_bands``; the definition is in include/stemgnn_hip.h): paths
    [count,K,H,N] contiguous float32 on the device, mult int32 [count,K] the members' multiplicities with common sum `total` ->
    bands [count,Q,H,N] float32: bands[c,q,h,n] = the scenario_rank(quantiles[q], total)-th smallest of the ensemble in which member
    k stands mult[c,k] times -- `scenario_bands` of the replicated ensemble, bit for bit, without forming it.  A member of
    multiplicity 0 is not read; an origin whose multiplicities are negative or do not sum to total is NaN.  K <= 256."""
    what = "weighted_bands"
    C, K, H, N, W = _weighted_set(what, paths, mult, total)
    quantiles = [float(t) for t in quantiles]
    Q = len(quantiles)
    if not 1 <= Q <= 32:
        raise _lib.StemGNNHipError(f"{what}: 1 to 32 levels, got {Q}")
    if out is not None and (not torch.is_tensor(out) or tuple(out.shape) != (C, Q, H, N) or out.dtype != torch.float32 or
                            not out.is_contiguous() or out.device != paths.device):
        raise _lib.StemGNNHipError(f"{what}: out must be a contiguous float32 {(C, Q, H, N)} tensor on the paths' device")
    _require_gpu(paths, "paths")
    lib = _lib.load()
    bands = torch.empty(C, Q, H, N, device=paths.device, dtype=torch.float32) if out is None else out
    ranks = (ctypes.c_int * Q)(*[scenario_rank(t, W) for t in quantiles])
    _lib.check(lib.stemgnn_weighted_bands(paths.data_ptr(), mult.data_ptr(), C, K, H, N, W, Q, ranks, bands.data_ptr(), _stream()),
               what)
    return bands


def weighted_scores(y, paths, mult, total, mul=None, add=None, ignore_nan=False, fair=False):
    """Scores of a weighted scenario set against what happened (``stemgnn_weighted_scores``; the definitions are in
    include/stemgnn_hip.h): y [count,H,N], paths [count,K,H,N], mult int32 [count,K] with common sum `total` ->
    (out float64 [7 * (1 + H)] = overall | by_step[7][H]: the six statistics of `ensemble_scores` with every member weighted by
    its multiplicity, then the number of absent origins; hist int64 [H, total + 1]), both on the device, no sync.
    mul / add, ignore_nan, fair: `ensemble_scores`' (fair needs total >= 2)."""
    what = "weighted_scores"
    C, K, H, N, W = _weighted_set(what, paths, mult, total)
    if not torch.is_tensor(y) or tuple(y.shape) != (C, H, N) or y.dtype != torch.float32 or not y.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: y must be a contiguous float32 [count,H,N] = {(C, H, N)} tensor, got "
                                   f"{(str(y.dtype) + ' ' + str(tuple(y.shape))) if torch.is_tensor(y) else type(y).__name__}")
    mul, add = _denorm_pair(what, mul, add, N)
    if fair and W < 2:
        raise _lib.StemGNNHipError(f"{what}: fair=True needs total >= 2, got {W}")
    if H * (W + 1) >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: a histogram of {H} x {W + 1} bins does not fit the entry's range (2^31)")
    _require_gpu(paths, "paths")
    _require_gpu(y, "y")
    if y.device != paths.device:
        raise _lib.StemGNNHipError(f"{what}: y is on {y.device}, paths on {paths.device}")
    lib = _lib.load()
    dev = paths.device
    mul, add = _f64_on(mul, dev), _f64_on(add, dev)
    scratch = torch.empty(lib.stemgnn_weighted_scratch_doubles(C, K, H, N), device=dev, dtype=torch.float64)
    out = torch.empty(lib.stemgnn_weighted_out_doubles(H), device=dev, dtype=torch.float64)
    hist = torch.empty(H, W + 1, device=dev, dtype=torch.int64)
    _lib.check(lib.stemgnn_weighted_scores(y.data_ptr(), paths.data_ptr(), mult.data_ptr(),
                                           None if mul is None else mul.data_ptr(), None if add is None else add.data_ptr(),
                                           C, K, H, N, W, int(bool(fair)), int(bool(ignore_nan)), scratch.data_ptr(),
                                           out.data_ptr(), hist.data_ptr(), _stream()), what)
    return out, hist


def weighted_events(paths, mult, total, threshold, above=True, min_run=1, mul=None, add=None):
    """Crossing counts of a weighted scenario set (``stemgnn_weighted_events``): `scenario_events` with every member counted
    mult[c,k] times -- the counts of the replicated ensemble of `total` paths, exactly.  paths [count,K,H,M], mult int32
    [count,K] -> counts int32 [count, 2H+1, M]; an origin whose multiplicities are negative or do not sum to total is -1."""
    what = "weighted_events"
    C, K, H, M, W = _weighted_set(what, paths, mult, total)
    if H > 256:
        raise _lib.StemGNNHipError(f"{what}: at most 256 steps, got H = {H}")
    if isinstance(min_run, bool) or int(min_run) != min_run or not 1 <= int(min_run) <= H:
        raise _lib.StemGNNHipError(f"{what}: min_run must be an integer within [1, {H}], got {min_run!r}")
    threshold = _per_column(what, "threshold", threshold, M)
    mul, add = _denorm_pair(what, mul, add, M)
    _require_gpu(paths, "paths")
    lib = _lib.load()
    dev = paths.device
    threshold, mul, add = _f64_on(threshold, dev), _f64_on(mul, dev), _f64_on(add, dev)
    counts = torch.empty(C, 2 * H + 1, M, device=dev, dtype=torch.int32)
    _lib.check(lib.stemgnn_weighted_events(paths.data_ptr(), mult.data_ptr(), threshold.data_ptr(),
                                           None if mul is None else mul.data_ptr(), None if add is None else add.data_ptr(),
                                           C, K, H, M, W, int(bool(above)), int(min_run), counts.data_ptr(), _stream()), what)
    return counts


def scenario_reduce_weighted(distances, mult, total, keep):
    """Forward selection on an ensemble with probabilities mult / total (``stemgnn_scenario_reduce_weighted``; the definition is
    in include/stemgnn_hip.h): distances float64 [count,S,S] contiguous on the device (`scenario_distances`, or any cost
    D[k,u] of moving member k onto member u), mult int32 [count,S] with common sum `total` -> (selected int32 [count,keep],
    counts int32 [count,keep] = the multiplicities gathered by each kept member, assign int32 [count,S], cost float64
    [count,keep]), on the device, no sync.  A member of multiplicity 0 is no candidate and its distances are not read.  Refused
    origins (-1 / 0 / -1 / NaN): a distance that is not a finite number >= 0, multiplicities that are negative or do not sum
    to total, fewer than `keep` members of positive multiplicity.  All-ones mult and total = S: `scenario_reduce`, bit for bit."""
    what = "scenario_reduce_weighted"
    C, S = _reduce_distances(what, distances)
    if S > 1024:
        raise _lib.StemGNNHipError(f"{what}: at most 1024 members, got S = {S}")
    if C * S * S >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {C} origins x {S} x {S} distances do not fit the entry's range (2^31)")
    W = _weighted_mult(what, mult, total, C, S)
    K = _reduce_keep(what, keep, S)
    if not distances.is_cuda:
        raise _lib.StemGNNHipError(f"{what}: distances is on {distances.device}: stemgnn_amd runs only on a HIP device "
                                   "(no CPU fallback)")
    if mult.device != distances.device:
        raise _lib.StemGNNHipError(f"{what}: distances is on {distances.device}, mult on {mult.device}")
    lib = _lib.load()
    selected, counts, assign, cost = _reduce_outputs(C, S, K, distances.device)
    _lib.check(lib.stemgnn_scenario_reduce_weighted(distances.data_ptr(), mult.data_ptr(), C, S, K, W, selected.data_ptr(),
                                                    counts.data_ptr(), assign.data_ptr(), cost.data_ptr(), _stream()), what)
    return selected, counts, assign, cost


def _envelope_coverage(what, coverage):
    if isinstance(coverage, bool) or not isinstance(coverage, (int, float, np.floating)) or not 0.0 < float(coverage) < 1.0:
        raise _lib.StemGNNHipError(f"{what}: coverage must be a number inside (0, 1), got {coverage!r}")
    return float(coverage)


def scenario_envelope(paths, coverage, target=None, mult=None, total=None, multiplier=None, ignore_nan=False,
                      return_depth=False):
    """The simultaneous band of sampled paths (``stemgnn_scenario_envelope``; the definition is in include/stemgnn_hip.h): per
    (origin, column) a centre and a scale per step from the S paths, every path's depth max_h |x - centre| / scale, the
    multiplier `chosen` that holds `coverage` of the ensemble's own whole paths, and the band centre -+ q * scale with
    q = chosen, or q = `multiplier` (a scalar or C values, fp64: an EnvelopeCalibrator's) when one is given.
    paths [count,S,H,C] contiguous float32 on the device; mult int32 [count,S] with common sum `total`: a weighted set's
    multiplicities; target [count,H,C] float32: what happened, whose depth `truth` the band with multiplier q holds exactly when
    truth <= q (ignore_nan: NaN steps are skipped).  Returns a dict of device tensors, no sync:
      bands float32 [count,2,H,C], moments float64 [count,2,H,C] (centre, scale), chosen float64 [count,C],
      truth float64 [count,C] or None, depth float64 [count,S,C] or None (return_depth).
    A column with a non-finite path value, and every column of an origin whose multiplicities are negative or do not sum to
    total, is NaN everywhere.  S <= 1024, H <= 256.  One launch."""
    what = "scenario_envelope"
    if not torch.is_tensor(paths) or paths.dim() != 4 or paths.numel() == 0:
        raise _lib.StemGNNHipError(f"{what}: paths must be a non-empty [count,S,H,C] tensor, got "
                                   f"{tuple(paths.shape) if torch.is_tensor(paths) else type(paths).__name__}")
    if paths.dtype != torch.float32 or not paths.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: paths must be a contiguous float32 tensor, got {paths.dtype}, strides "
                                   f"{tuple(paths.stride())}")
    count, S, H, C = (int(v) for v in paths.shape)
    if S > 1024 or H > 256:
        raise _lib.StemGNNHipError(f"{what}: at most 1024 paths of at most 256 steps, got S = {S}, H = {H}")
    if max(count * S * C, count * H * C, S * H * C) >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {count} origins of {S} paths of {H} x {C} values do not fit the entry's range "
                                   "(2^31); walk the origins in batches")
    coverage = _envelope_coverage(what, coverage)
    if (mult is None) != (total is None):
        raise _lib.StemGNNHipError(f"{what}: mult and total go together")
    W = 0 if mult is None else _weighted_mult(what, mult, total, count, S)
    if mult is not None and mult.device != paths.device:
        raise _lib.StemGNNHipError(f"{what}: paths is on {paths.device}, mult on {mult.device}")
    if target is not None and (not torch.is_tensor(target) or tuple(target.shape) != (count, H, C) or
                               target.dtype != torch.float32 or not target.is_contiguous()):
        raise _lib.StemGNNHipError(
            f"{what}: target must be a contiguous float32 [count,H,C] = {(count, H, C)} tensor, got "
            f"{(str(target.dtype) + ' ' + str(tuple(target.shape))) if torch.is_tensor(target) else type(target).__name__}")
    if multiplier is not None:
        multiplier = multiplier.detach() if torch.is_tensor(multiplier) else \
            torch.as_tensor(np.asarray(multiplier, dtype=np.float64))
        if multiplier.dim() == 0:
            multiplier = multiplier.reshape(1)
        if multiplier.dim() != 1 or multiplier.shape[0] not in (1, C) or multiplier.is_complex():
            raise _lib.StemGNNHipError(f"{what}: multiplier must be a scalar, [1] or [{C}] (one per column), got shape "
                                       f"{tuple(multiplier.shape)}")
    _require_gpu(paths, "paths")
    if target is not None:
        _require_gpu(target, "target")
        if target.device != paths.device:
            raise _lib.StemGNNHipError(f"{what}: target is on {target.device}, paths on {paths.device}")
    lib = _lib.load()
    dev = paths.device
    multiplier = _f64_on(multiplier, dev)
    f64 = dict(device=dev, dtype=torch.float64)
    moments, chosen = torch.empty(count, 2, H, C, **f64), torch.empty(count, C, **f64)
    truth = None if target is None else torch.empty(count, C, **f64)
    depth = torch.empty(count, S, C, **f64) if return_depth else None
    bands = torch.empty(count, 2, H, C, device=dev, dtype=torch.float32)

    def ptr(v):
        return None if v is None else v.data_ptr()

    _lib.check(lib.stemgnn_scenario_envelope(paths.data_ptr(), ptr(mult), W, ptr(target), int(bool(ignore_nan)), ptr(multiplier),
                                             0 if multiplier is None else int(multiplier.shape[0]), count, S, H, C, coverage,
                                             moments.data_ptr(), ptr(depth), chosen.data_ptr(), ptr(truth), bands.data_ptr(),
                                             _stream()), what)
    return dict(bands=bands, moments=moments, chosen=chosen, truth=truth, depth=depth)


def _tree_stages(what, stages, H):
    """stage bounds 0 < b_1 < .. < b_T = H (T <= 16) -> a tuple of ints"""
    try:
        b = tuple(stages)
    except TypeError:
        b = None
    if not b or len(b) > 16 or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in b) or \
            any(int(v) <= int(u) for u, v in zip((0,) + b[:-1], b)) or int(b[-1]) != H:
        raise _lib.StemGNNHipError(f"{what}: stages must be 1 to 16 strictly increasing step bounds that end at H = {H} "
                                   f"(stage t owns the steps [b_(t-1), b_t)), got {stages!r}")
    return tuple(int(v) for v in b)


def _tree_nodes(what, nodes, T, S):
    """node counts 1 <= n_1 <= .. <= n_T <= S, one per stage -> a tuple of ints"""
    try:
        n = tuple(nodes)
    except TypeError:
        n = None
    if not n or len(n) != T or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in n) or \
            any(int(v) < int(u) for u, v in zip((1,) + n[:-1], n)) or int(n[-1]) > S:
        raise _lib.StemGNNHipError(f"{what}: nodes must be {T} non-decreasing node counts within [1, {S}], one per stage "
                                   f"(S = {S} paths), got {nodes!r}")
    return tuple(int(v) for v in n)


def scenario_stage_distances(paths, stages, scale=None, squared=False):
    """Prefix distances of sampled paths at every stage boundary (``stemgnn_scenario_stage_distances``; the definition is in
    include/stemgnn_hip.h): paths [count,S,H,M] contiguous float32 on the device, stages = the bounds 0 < b_1 < .. < b_T = H ->
    D [count,T,S,S] float64, D[c,t,i,j] = sqrt(sum over the steps before b_t and all m of ((x_i - x_j) * scale)^2) in fp64 from
    the differences, the stages' sums added in stage order; squared: without the root.  scale: scenario_distances'.  One
    launch reads the paths once for all T tiles.  Every D[c,t] equals its transpose bit for bit; a NaN in a path reaches its row
    and column from its stage on."""
    what = "scenario_stage_distances"
    C, S, H, M = _reduce_paths(what, paths)
    bounds = _tree_stages(what, stages, H)
    scale = _reduce_scale(what, scale, H, M)
    squared = _reduce_flag(what, squared)
    T = len(bounds)
    if C * T * S * S >= 2 ** 31:
        raise _lib.StemGNNHipError(f"{what}: {C} origins x {T} x {S} x {S} distances do not fit the entry's range (2^31); "
                                   "scenario_tree walks the origins in batches")
    _require_gpu(paths, "paths")
    lib = _lib.load()
    scale = _f64_on(scale, paths.device)
    D = torch.empty(C, T, S, S, device=paths.device, dtype=torch.float64)
    _lib.check(lib.stemgnn_scenario_stage_distances(paths.data_ptr(), None if scale is None else scale.data_ptr(), C, S, H, M, T,
                                                    (ctypes.c_int * T)(*bounds), squared, D.data_ptr(), _stream()), what)
    return D


def scenario_tree(paths, stages, nodes, scale=None, squared=False, distances=None, mult=None, total=None,
                  max_scratch_bytes=256 << 20):
    """A scenario tree by staged forward selection (``stemgnn_scenario_stage_distances`` + ``stemgnn_scenario_tree``; the
    definition is in include/stemgnn_hip.h): per origin, stage t keeps nodes[t] representative paths, every node a child of
    one node of the stage before (the members of a node share their representative up to the stage's bound), every path
    assigned to the nearest node among its parent's children in the prefix metric of the stage.  paths [count,S,H,M]
    contiguous float32 on the device; stages / scale / squared: scenario_stage_distances'; nodes: 1 <= n_1 <= .. <= n_T <= S.
    mult int32 [count,S] with common sum `total`: the paths' multiplicities (None: one each).  Returns
      node_path   int32 [count,T,n_T]  the path each node is represented by      node_parent int32 [count,T,n_T]  its parent node
      node_count  int32 [count,T,n_T]  the multiplicities it gathers              assign      int32 [count,T,S]    every path's node
      cost        float64 [count,T]    the Kantorovich distance of the stage, in its prefix metric
    on the device, no sync; beyond n_t the node entries are -1 / -1 / 0.  A refused origin (absent, n_T above its members of
    positive multiplicity, or a distance between two such members that is not a finite number >= 0) is -1 / -1 / 0 / -1 / NaN at
    every stage; the others are not affected.  The origins are walked in batches whose [batch,T,S,S] float64 distances stay
    within max_scratch_bytes; the result is that of one call, bit for bit.
    distances [count,T,S,S] float64 (contiguous, on the device): any cost of the caller's, D[t,k,u] = moving path k onto path u
    in stage t; only the second entry runs, paths may be None, and `stages` is only checked for its length."""
    what = "scenario_tree"
    if distances is None:
        C, S, H, M = _reduce_paths(what, paths)
        bounds = _tree_stages(what, stages, H)
        T = len(bounds)
        scale = _reduce_scale(what, scale, H, M)
        squared = _reduce_flag(what, squared)
        source = paths
    else:
        C, T, S = _reduce_distances(what, distances, staged=True)
        if S > 1024 or T > 16:
            raise _lib.StemGNNHipError(f"{what}: at most 1024 paths and 16 stages, got S = {S}, T = {T}")
        if paths is not None and (not torch.is_tensor(paths) or paths.dim() != 4 or tuple(paths.shape[:2]) != (C, S)):
            raise _lib.StemGNNHipError(f"{what}: paths must be [count,S,H,M] with the distances' count = {C} and S = {S}, got "
                                       f"{tuple(paths.shape) if torch.is_tensor(paths) else type(paths).__name__}")
        if stages is not None and len(tuple(stages)) != T:
            raise _lib.StemGNNHipError(f"{what}: {len(tuple(stages))} stages, but the distances hold T = {T}")
        source = distances
    n = _tree_nodes(what, nodes, T, S)
    if mult is None:
        if total is not None and total != S:
            raise _lib.StemGNNHipError(f"{what}: without mult every path counts once and total is S = {S}, got {total!r}")
        W = S
    else:
        W = _weighted_mult(what, mult, total, C, S)
        if mult.device != source.device:
            raise _lib.StemGNNHipError(f"{what}: mult is on {mult.device}, the {'paths' if distances is None else 'distances'} "
                                       f"on {source.device}")
    one = T * S * S * 8
    if isinstance(max_scratch_bytes, bool) or int(max_scratch_bytes) != max_scratch_bytes or int(max_scratch_bytes) < one:
        raise _lib.StemGNNHipError(f"{what}: max_scratch_bytes must hold one origin's [T,S,S] float64 distances ({one} bytes), "
                                   f"got {max_scratch_bytes!r}")
    batch = max(1, min(int(max_scratch_bytes) // one, (2 ** 31 - 1) // (T * S * S)))
    if not source.is_cuda:
        raise _lib.StemGNNHipError(f"{what}: {'paths' if distances is None else 'distances'} is on {source.device}: "
                                   "stemgnn_amd runs only on a HIP device (no CPU fallback)")
    lib = _lib.load()
    dev = source.device
    nT = n[-1]
    node_path = torch.empty(C, T, nT, device=dev, dtype=torch.int32)
    node_parent = torch.empty(C, T, nT, device=dev, dtype=torch.int32)
    node_count = torch.empty(C, T, nT, device=dev, dtype=torch.int32)
    assign = torch.empty(C, T, S, device=dev, dtype=torch.int32)
    cost = torch.empty(C, T, device=dev, dtype=torch.float64)
    n_host = (ctypes.c_int * T)(*n)
    if distances is None:
        scale = _f64_on(scale, dev)
        b_host = (ctypes.c_int * T)(*bounds)
        D = torch.empty(min(batch, C), T, S, S, device=dev, dtype=torch.float64)
    for lo in range(0, C, batch):
        k = min(batch, C - lo)
        if distances is None:
            _lib.check(lib.stemgnn_scenario_stage_distances(paths[lo:lo + k].data_ptr(),
                                                            None if scale is None else scale.data_ptr(), k, S, H, M, T, b_host,
                                                            squared, D.data_ptr(), _stream()), "scenario_stage_distances")
            d_ptr = D.data_ptr()
        else:
            d_ptr = distances[lo:lo + k].data_ptr()
        _lib.check(lib.stemgnn_scenario_tree(d_ptr, None if mult is None else mult[lo:lo + k].data_ptr(), k, S, T, n_host, W,
                                             node_path[lo:lo + k].data_ptr(), node_parent[lo:lo + k].data_ptr(),
                                             node_count[lo:lo + k].data_ptr(), assign[lo:lo + k].data_ptr(),
                                             cost[lo:lo + k].data_ptr(), _stream()), what)
    return node_path, node_parent, node_count, assign, cost


def _ring_ok(what, ring, t_dev):
    _require_gpu(ring, "ring")
    if ring.dim() != 2 or ring.dtype != torch.float32 or not ring.is_contiguous():
        raise _lib.StemGNNHipError(f"{what}: a ring must be a contiguous float32 [C,N] tensor, got {ring.dtype} "
                                   f"{tuple(ring.shape)}")
    if t_dev.dtype != torch.int64 or t_dev.device != ring.device or t_dev.numel() < 1:
        raise _lib.StemGNNHipError(f"{what}: t_dev must be an int64 tensor on the ring's device")


def live_push(raw, t0, sub, div, clip01, missing, last, ring_x, ring_y, t_dev):
    """K new rows of a stream into the rings (``stemgnn_live_push``): raw [K,N] float64 on the device, t0 the HOST's count of the
    rows pushed before.  Forward fill from `last` (float64 [N], updated), the normalisation of normalize_series, ring_x the
    imputed rows, ring_y the same with NaN at the missing readings (NaN, or `missing` when it is not None); then
    t_dev[0] = t0 + K.  One launch, nothing synchronises."""
    lib = _lib.load()
    _ring_ok("live_push", ring_x, t_dev)
    _ring_ok("live_push", ring_y, t_dev)
    C, N = ring_x.shape
    if ring_y.shape != ring_x.shape or ring_y.device != ring_x.device:
        raise _lib.StemGNNHipError("live_push: ring_x and ring_y must have one shape and device")
    if raw.dim() != 2 or raw.shape[1] != N or raw.dtype != torch.float64 or raw.device != ring_x.device or \
            not raw.is_contiguous():
        raise _lib.StemGNNHipError(f"live_push: raw must be a contiguous float64 [K,{N}] tensor on the rings' device")
    for t, name in ((sub, "sub"), (div, "div"), (last, "last")):
        if t.dtype != torch.float64 or t.device != ring_x.device or t.numel() != N or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"live_push: {name} must be a contiguous float64 [{N}] tensor on the rings' device")
    _lib.check(lib.stemgnn_live_push(raw.data_ptr(), raw.shape[0], N, int(t0), sub.data_ptr(), div.data_ptr(),
                                     int(bool(clip01)), 0.0 if missing is None else float(missing), int(missing is not None),
                                     last.data_ptr(), ring_x.data_ptr(), ring_y.data_ptr(), C, t_dev.data_ptr(), _stream()),
               "live_push")


_ring_status = {}


def ring_status_word(device):
    """The device's int32 status word of ring_gather (created on first use: a caller that captures a ring_gather into a hipGraph
    asks for it once ahead of the capture, so that its zero fill is not a node of the graph)."""
    key = str(device)
    st = _ring_status.get(key)
    if st is None:
        st = _ring_status[key] = torch.zeros(1, dtype=torch.int32, device=device)
    return st


def ring_gather(ring, t_dev, L, starts=None, back=0, out=None):
    """out[b, l] = ring[(s_b + l) mod C] for l < L (``stemgnn_ring_gather``): s_b = starts[b] (int64 [B], device), or the one
    window that starts `back` rows behind the device-side head t_dev[0] when starts is None.  A window that is not (or no longer)
    in the ring comes back as NaN rows (and sets bit 0 of the device's ring status word: check_ring_status)."""
    lib = _lib.load()
    _ring_ok("ring_gather", ring, t_dev)
    C, N = ring.shape
    if starts is not None:
        if starts.dtype != torch.int64 or starts.device != ring.device or starts.dim() != 1 or not starts.is_contiguous():
            raise _lib.StemGNNHipError("ring_gather: starts must be a contiguous int64 [B] tensor on the ring's device")
        B = starts.numel()
    else:
        B = 1
    if out is None:
        out = torch.empty(B, int(L), N, device=ring.device, dtype=torch.float32)
    elif tuple(out.shape) != (B, int(L), N) or out.dtype != torch.float32 or out.device != ring.device or \
            not out.is_contiguous():
        raise _lib.StemGNNHipError(f"ring_gather: out must be a contiguous float32 {(B, int(L), N)} tensor on the ring's device")
    st = ring_status_word(ring.device)
    _lib.check(lib.stemgnn_ring_gather(ring.data_ptr(), C, N, starts.data_ptr() if starts is not None else None,
                                       t_dev.data_ptr(), int(back), B, int(L), out.data_ptr(), st.data_ptr(), _stream()),
               "ring_gather")
    return out


def check_ring_status(device):
    """Raise if any ring_gather since the last check asked for rows the ring does not hold (one sync)."""
    st = _ring_status.get(str(device))
    if st is not None and int(st.item()) != 0:
        st.zero_()
        raise IndexError("ring_gather: a window outside the rows the ring holds (NaN rows were returned)")


def live_head(t_dev, history, pos, origins):
    """pos[0] = t_dev[0] mod history and origins[pos[0]] = t_dev[0] on the device (``stemgnn_live_head``): the slab position of
    the forecast made now, for forecast_store / quantile_store."""
    lib = _lib.load()
    for t, name in ((t_dev, "t_dev"), (pos, "pos"), (origins, "origins")):
        if not t.is_cuda or t.dtype != torch.int64 or t.device != t_dev.device or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"live_head: {name} must be a contiguous int64 tensor on one HIP device")
    if origins.numel() != int(history):
        raise _lib.StemGNNHipError(f"live_head: origins must hold history = {history} entries, got {origins.numel()}")
    _lib.check(lib.stemgnn_live_head(t_dev.data_ptr(), int(history), pos.data_ptr(), origins.data_ptr(), _stream()),
               "live_head")


def aci_update(issued, raw, ring_y, origin, pairs, target_alpha, gamma, slot, min_scores, per_step, per_node, scores, alpha,
               offsets, counts, miss_sum, valid_sum):
    """One adaptive-conformal update from ONE matured forecast (``stemgnn_aci_update``): issued / raw [Q,H,N] (the served rows and
    the same forecast ahead of calibration), the targets in the ring ring_y [C,N] at slots (origin + h) mod C, pairs = P (lo, hi)
    rows with target_alpha = 1 - coverage each.  State, updated in place: scores [M,P,H,N] fp32 (NaN = absent; slot `slot` is
    overwritten), alpha fp64, offsets fp32, counts / miss_sum / valid_sum int64, all [P, H if per_step else 1, N if per_node
    else 1].  One launch, nothing synchronises."""
    lib = _lib.load()
    _require_gpu(issued, "issued")
    dev = issued.device
    if issued.dim() != 3 or raw.shape != issued.shape:
        raise _lib.StemGNNHipError(f"aci_update: issued and raw must be [Q,H,N], got {tuple(issued.shape)} / {tuple(raw.shape)}")
    Q, H, N = issued.shape
    P, lo, hi = _conformal_pairs(pairs, Q)
    if len(target_alpha) != P:
        raise ValueError(f"aci_update: {P} pairs but {len(target_alpha)} target levels")
    if ring_y.dim() != 2 or ring_y.shape[1] != N:
        raise _lib.StemGNNHipError(f"aci_update: ring_y must be [C,{N}], got {tuple(ring_y.shape)}")
    if scores.dim() != 4 or tuple(scores.shape[1:]) != (P, H, N):
        raise _lib.StemGNNHipError(f"aci_update: scores must be [M,{P},{H},{N}], got {tuple(scores.shape)}")
    for t, name in ((issued, "issued"), (raw, "raw"), (ring_y, "ring_y"), (scores, "scores")):
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"aci_update: {name} must be a contiguous float32 tensor on {dev}")
    shape = (P, H if per_step else 1, N if per_node else 1)
    for t, name, dt in ((alpha, "alpha", torch.float64), (offsets, "offsets", torch.float32), (counts, "counts", torch.int64),
                        (miss_sum, "miss_sum", torch.int64), (valid_sum, "valid_sum", torch.int64)):
        if tuple(t.shape) != shape or t.device != dev or t.dtype != dt or not t.is_contiguous():
            raise _lib.StemGNNHipError(f"aci_update: {name} must be a contiguous {dt} {shape} tensor on {dev}")
    _lib.check(lib.stemgnn_aci_update(issued.data_ptr(), raw.data_ptr(), ring_y.data_ptr(), ring_y.shape[0], int(origin), Q, H, N,
                                      P, lo, hi, _lib.host_floats(target_alpha, _lib.c_double), float(gamma), scores.shape[0],
                                      int(slot), int(min_scores), int(bool(per_step)), int(bool(per_node)), scores.data_ptr(),
                                      alpha.data_ptr(), offsets.data_ptr(), counts.data_ptr(), miss_sum.data_ptr(),
                                      valid_sum.data_ptr(), _stream()), "aci_update")


def anomaly_update(slab, origins, row, ring_y, rows, slot, min_scores, alpha, per_step, per_node, scores, pvalues, node_p, alarm,
                   counts, alarm_sum, judged_sum, log_p, log_slot, work):
    """Conformal anomaly p-values of ONE arrived row (``stemgnn_anomaly_update``): slab [S,R,H,N] the stored forecasts with their
    origins (int64 [S] on the device; None: slab [1,R,H,N] holds the row's forecasts, step h at [0,:,h]), row = the arrived row's
    absolute index, its targets in the ring ring_y [C,N] at slot row mod C, rows = (lo, hi) the slab rows scored (lo == hi: the
    absolute residual).  State, updated in place: scores [M,H,N] fp32 (NaN = absent; slot `slot` is overwritten), alarm_sum /
    judged_sum int64 [N], row log_slot of log_p [keep,N]; written in full: pvalues [H,N], node_p [N], alarm int32 [N], counts
    int64 [H if per_step else 1, N if per_node else 1].  work: int32 [2 * H * N], zero before the first call and left zero by
    every call (where the workgroups of the two-launch forms meet).  One or two launches; nothing synchronises."""
    lib = _lib.load()
    _require_gpu(slab, "slab")
    dev = slab.device
    if slab.dim() != 4:
        raise _lib.StemGNNHipError(f"anomaly_update: slab must be [S,R,H,N], got {tuple(slab.shape)}")
    S, R, H, N = slab.shape
    lo, hi = (int(v) for v in rows)
    if origins is None:
        if S != 1:
            raise _lib.StemGNNHipError(f"anomaly_update: without origins the slab is [1,R,H,N], got {tuple(slab.shape)}")
    elif origins.dtype != torch.int64 or origins.device != dev or tuple(origins.shape) != (S,) or not origins.is_contiguous():
        raise _lib.StemGNNHipError(f"anomaly_update: origins must be a contiguous int64 [{S}] tensor on {dev}")
    if ring_y.dim() != 2 or ring_y.shape[1] != N:
        raise _lib.StemGNNHipError(f"anomaly_update: ring_y must be [C,{N}], got {tuple(ring_y.shape)}")
    if scores.dim() != 3 or tuple(scores.shape[1:]) != (H, N):
        raise _lib.StemGNNHipError(f"anomaly_update: scores must be [M,{H},{N}], got {tuple(scores.shape)}")
    if log_p.dim() != 2 or log_p.shape[1] != N:
        raise _lib.StemGNNHipError(f"anomaly_update: log_p must be [keep,{N}], got {tuple(log_p.shape)}")
    gshape = (H if per_step else 1, N if per_node else 1)
    for t, name, dt, shape in ((slab, "slab", torch.float32, None), (ring_y, "ring_y", torch.float32, None),
                               (scores, "scores", torch.float32, None), (log_p, "log_p", torch.float32, None),
                               (pvalues, "pvalues", torch.float32, (H, N)), (node_p, "node_p", torch.float32, (N,)),
                               (alarm, "alarm", torch.int32, (N,)), (counts, "counts", torch.int64, gshape),
                               (alarm_sum, "alarm_sum", torch.int64, (N,)), (judged_sum, "judged_sum", torch.int64, (N,)),
                               (work, "work", torch.int32, (2 * H * N,))):
        if t.device != dev or t.dtype != dt or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
            raise _lib.StemGNNHipError(f"anomaly_update: {name} must be a contiguous {dt} {shape or ''} tensor on {dev}")
    _lib.check(lib.stemgnn_anomaly_update(slab.data_ptr(), S, R, lo, hi, None if origins is None else origins.data_ptr(), int(row),
                                          ring_y.data_ptr(), ring_y.shape[0], H, N, scores.shape[0], int(slot), int(min_scores),
                                          float(alpha), int(bool(per_step)), int(bool(per_node)), scores.data_ptr(),
                                          pvalues.data_ptr(), node_p.data_ptr(), alarm.data_ptr(), counts.data_ptr(),
                                          alarm_sum.data_ptr(), judged_sum.data_ptr(), log_p.data_ptr(), log_p.shape[0],
                                          int(log_slot), work.data_ptr(), _stream()), "anomaly_update")


def eval_metrics(target, forecast, mul=None, add=None, ignore_nan=False):
    """target / forecast [count,H,N] fp32 -> float64 device vector
    overall[3] | by_node[3][N] | by_step[3][H] | by_step_node[3][H][N]  (MAPE, MAE, RMSE each).
    ignore_nan: elements whose target is NaN are left out and every mean divides by its slice's valid count
    (stemgnn_eval_metrics_masked; a slice with no valid element is NaN)."""
    lib = _lib.load()
    _require_gpu(target, "target")
    _require_gpu(forecast, "forecast")
    if target.shape != forecast.shape or target.dim() != 3:
        raise _lib.StemGNNHipError("eval_metrics: target/forecast must both be [count, time_step, node]")
    target, forecast = target.contiguous(), forecast.contiguous()
    C, H, N = target.shape
    dev = target.device
    sizer, entry = (lib.stemgnn_eval_scratch_doubles_masked, lib.stemgnn_eval_metrics_masked) if ignore_nan else \
        (lib.stemgnn_eval_scratch_doubles, lib.stemgnn_eval_metrics)
    scratch = torch.empty(sizer(C, H, N), device=dev, dtype=torch.float64)
    out = torch.empty(lib.stemgnn_eval_out_doubles(H, N), device=dev, dtype=torch.float64)
    if mul is not None:
        mul = mul.to(device=dev, dtype=torch.float64).contiguous()
        add = add.to(device=dev, dtype=torch.float64).contiguous()
    _lib.check(entry(target.data_ptr(), forecast.data_ptr(), mul.data_ptr() if mul is not None else None,
                     add.data_ptr() if add is not None else None, C, H, N, scratch.data_ptr(), out.data_ptr(), _stream()),
               "eval_metrics")
    return out
