"""Optimizer / training-step plumbing for the HIP MAE path (host-side counterpart of run_swin_mae3d.py:588-598,644-669).

FusedAdamW: clip_grad_norm_(max_norm) + AdamW over the model's flat fp32 parameter/gradient buffers in three kernel
launches (norm reduction, clip coefficient, update); hyper-parameters live in a small device tensor so the step is
hipGraph-replayable.  OneCycle: the reference's OneCycleLR defaults (pct_start .3, cos, div 25, final_div 1e4,
beta1 cycling .95->.85->.95), stepped every iteration."""
from __future__ import annotations

import math
import time

import numpy as np

import torch

from . import ops


class OneCycle:
    def __init__(self, max_lr: float, total_steps: int, pct_start=0.3, div_factor=25.0, final_div_factor=1e4, base_m=0.85, max_m=0.95):
        self.max_lr, self.total = max_lr, total_steps
        self.init_lr, self.min_lr = max_lr / div_factor, max_lr / div_factor / final_div_factor
        self.up_end = float(pct_start * total_steps) - 1
        self.base_m, self.max_m = base_m, max_m

    @staticmethod
    def _cos(a, b, pct):
        return b + (a - b) / 2.0 * (math.cos(math.pi * pct) + 1)

    def at(self, step: int):
        """(lr, beta1) used for optimizer step number `step` (0-based), same as torch OneCycleLR(two-phase, cos)."""
        if step <= self.up_end:
            pct = step / self.up_end if self.up_end > 0 else 1.0
            return self._cos(self.init_lr, self.max_lr, pct), self._cos(self.max_m, self.base_m, pct)
        pct = (step - self.up_end) / (self.total - 1 - self.up_end)
        return self._cos(self.max_lr, self.min_lr, pct), self._cos(self.base_m, self.max_m, pct)


class PinnedRing:
    """Ring of pinned host slots for small per-step uploads (hyper-parameters, token mask, extents).  `upload(src, dst)` copies
    src -> next slot -> dst (non-blocking, stream-ordered) and records an event; a slot is only rewritten after the event of its
    previous upload has completed, so the host can run ahead of the device without corrupting a copy that has not executed yet."""

    def __init__(self, shape, dtype, depth: int = 8, pinned: bool = True):
        self.buf = torch.empty((depth,) + tuple(shape), dtype=dtype)
        if pinned:
            self.buf = self.buf.pin_memory()
        self.events = [None] * depth
        self.i, self.pinned = 0, pinned

    def upload(self, src: torch.Tensor, dst: torch.Tensor):
        k = self.i % len(self.events)
        self.i += 1
        if self.events[k] is not None:
            # polled, not hipEventSynchronize: on this runtime a blocking wait on an (already complete) event was measured to return
            # only when the stream had drained (~100 ms per step in Trainer.fit, the device idle meanwhile)
            while not self.events[k].query():
                time.sleep(1e-4)
        slot = self.buf[k]
        slot.copy_(src.reshape(slot.shape))
        dst.copy_(slot.view(dst.shape), non_blocking=True)
        if self.pinned and dst.is_cuda:
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream())
            self.events[k] = ev


class FusedAdamW:
    """ranges: a finetune.param_ranges table over `model`'s flat layout, or None.  With a table the step runs the *_ranges kernels: range r steps with
    lr * lr_scale[r] and weight_decay * wd_scale[r], a range with lr_scale 0 is frozen (parameters and moments not written, outside the clip norm), and `norm` is
    the norm over the ranges that train.  The table is fixed here, on the device, so launch() stays graph-capturable; the scheduled lr of set_hyper() times the
    fixed scale is what OneCycleLR does with a list of max_lr.  None: the one-setting kernels, exactly as without the keyword.

    accumulate: k micro-batches per optimizer step.  With k > 1 -- asked for here, or by the step object that drives the optimizer
    (GraphedTrainStep(accumulate=k), FinetuneStep.accumulate) -- the gradient buffer holds the SUM of the micro-gradients when launch() runs, and the middle launch
    is ops.clip_coef_mean: clip and update act on the mean, weight `grad_scale` = 1 / (micro-batches of this step) each, set by set_grad_scale(); `norm` is the
    mean gradient's norm.  With 1 the launches are the three of before.  k is part of a checkpoint's resume section; a resume under another k is refused."""

    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-3, max_grad_norm=0.1, ranges=None, accumulate: int = 1):
        if int(accumulate) < 1:
            raise ValueError(f"FusedAdamW: accumulate >= 1, got {accumulate}")
        if model._flat is None:
            model.flatten_parameters()
        self.model, self.lr, self.betas, self.eps, self.wd, self.max_norm = model, lr, tuple(betas), eps, weight_decay, max_grad_norm
        flat = model._flat
        self.m, self.v = torch.zeros_like(flat), torch.zeros_like(flat)
        self.acc = torch.zeros(1, dtype=torch.float64, device=flat.device)
        self.coef = torch.ones(1, device=flat.device)
        self.norm = torch.zeros(1, device=flat.device)
        # {lr, b1, b2, eps, wd, 1-b1^t, 1-b2^t}: lr 0 and unit bias corrections until update_hyper() => a launch is a no-op
        self.hyper = torch.tensor([0.0, betas[0], betas[1], eps, 0.0, 1.0, 1.0, 0.0], device=flat.device)
        self.t = 0
        self.zero_grads_after_step = False   # the AdamW kernel also clears the flat gradient buffer (GraphedTrainStep turns it on)
        self.accumulate = int(accumulate)    # micro-batches per optimizer step, as the checkpoints record it
        self.mean_clip = self.accumulate > 1  # launch() clips the mean of an accumulated sum (a step object may turn it on)
        self.inv_k = torch.ones(1, device=flat.device)   # 1 / (micro-batches of this step), read by ops.clip_coef_mean
        self.grad_scale = 1.0                # ... and the value last sent
        self.ranges, self.range_record = None, None
        if ranges is not None:
            bounds, scale, record = ranges
            if int(record["bounds"][-1]) != flat.numel() or bounds.device != flat.device or scale.device != flat.device:
                raise ValueError(f"FusedAdamW: the range table ends at {record['bounds'][-1]} on {bounds.device}, the flat buffer has {flat.numel()} elements on "
                                 f"{flat.device}: build it with finetune.param_ranges over the same object")
            self.ranges, self.range_record = (bounds, scale), range_record(record)
            if flat.is_cuda:
                # the entries check a table on the host except inside a graph capture: once here, so a table they refuse never reaches a captured launch
                ops.grad_sqnorm_ranges(model._flat_grad, bounds, scale, self.acc)

    def set_hyper(self, lr=None, beta1=None):
        if lr is not None:
            self.lr = lr
        if beta1 is not None:
            self.betas = (beta1, self.betas[1])

    def set_grad_scale(self, inv_k: float):
        """the weight of each micro-gradient in this step's mean, 1 / (number of micro-batches): sent when it changes (NOT graph-capturable: a kernel argument
        of a tiny launch, as update_hyper's values; a captured launch() reads it on every replay)"""
        inv_k = float(inv_k)
        if not 0.0 < inv_k <= 1.0:
            raise ValueError(f"FusedAdamW.set_grad_scale: 1 / k of k >= 1 micro-batches, got {inv_k}")
        if inv_k != self.grad_scale:
            if self.inv_k.is_cuda:
                ops.grad_scale(inv_k, self.inv_k)
            else:
                self.inv_k.fill_(inv_k)
            self.grad_scale = inv_k

    def _clip(self):
        if self.mean_clip:
            ops.clip_coef_mean(self.acc, float(self.max_norm or 0.0), self.inv_k, self.coef, self.norm)
        else:
            ops.clip_coef(self.acc, float(self.max_norm or 0.0), self.coef, self.norm)

    def update_hyper(self, upload: bool = True):
        """advance the step counter and hand {lr, betas, eps, wd, bias corrections} to the device (NOT graph-capturable: the values are
        kernel arguments of a tiny launch, ops.step_params -- no host-to-device copy, so the host never waits for the stream).
        upload=False: only compute `self.hyper_host` (GraphedTrainStep sends it together with the mask and the extents)."""
        self.t += 1
        b1, b2 = self.betas
        # torch.optim.AdamW semantics under OneCycleLR momentum cycling: bias corrections from the CURRENT betas, 1 - beta^t
        # (not the running product of the per-step beta1 values, which differs by ~20 % a few steps into a cycled schedule)
        self.hyper_host = [self.lr, b1, b2, self.eps, self.wd, 1.0 - b1 ** self.t, 1.0 - b2 ** self.t, 1.0 if self.zero_grads_after_step else 0.0]
        if upload:
            if self.hyper.is_cuda:
                ops.step_params(hyper=self.hyper_host, hyper_dev=self.hyper)
            else:
                self.hyper.copy_(torch.tensor(self.hyper_host, dtype=torch.float32))

    def launch(self):
        """the three device-side launches (graph-capturable): grad norm, clip coefficient (of the mean, under accumulation), AdamW update"""
        g = self.model._flat_grad
        if self.ranges is not None:
            bounds, scale = self.ranges
            ops.grad_sqnorm_ranges(g, bounds, scale, self.acc)
            self._clip()
            ops.adamw_step_ranges(self.model._flat, g, self.m, self.v, self.hyper, bounds, scale, self.coef)
            return
        ops.grad_sqnorm(g, self.acc)
        self._clip()
        ops.adamw_step(self.model._flat, g, self.m, self.v, self.hyper, self.coef)

    def step(self):
        self.update_hyper()
        self.launch()


# thread-local capture mode: HIP calls made meanwhile by OTHER threads (the input prefetcher's pinned allocations and copies, the RCCL
# watchdog's event queries) must not invalidate the capture of the training thread
_CAPTURE_MODE = "thread_local"


class GraphedTrainStep:
    """One pre-training step (zero_grad, forward, backward, [all-reduce], clip+AdamW) replayed from HIP graphs.

    The step issues ~1.5k kernel launches; at 1 grid/GPU the eager Python/ctypes launch path costs as much wall time as the
    kernels, so the launch-bound loop is captured once (torch.cuda.CUDAGraph on the capture stream our C ABI launches on)
    and replayed.  Per-step inputs live in static device buffers refreshed before each replay: the padded batch, the valid
    extents, the token mask (host python `random`, as the reference) and the optimizer hyper-parameters.  Stochastic-depth
    noise is drawn inside the graph by torch's graph-safe Philox generator.
    With data parallelism the gradient exchange is ONE flat all-reduce between the backward graph and the optimizer graph
    (RCCL collectives are kept out of the captured region).

    accumulate = k > 1: k micro-batches of `batch` grids per optimizer step, each with its own block mask and its own loss normalisation, the
    mean of their gradients stepped -- by definition the k-rank data-parallel step, not the step of one batch of k * batch grids.  Two graphs in one pool: forward +
    backward, which adds into the gradient buffer (the AdamW kernel of the previous step cleared it) and adds its three losses into a device accumulator; and
    clip-of-the-mean + AdamW, which also turns the accumulator into the mean losses.  __call__(micro_batches, masks) replays the first once per micro-batch and the
    second once; begin(masks) / micro(j) / finish() are the same step in pieces, for a caller that fills `x` itself.  Fewer than k micro-batches (the ragged last step
    of an epoch) weigh 1 / k' each.  Data-parallel: the pieces of the split step without any collective for all but the last micro-step, whose replay is the step of
    before, so every gradient range is exchanged once per optimizer step; the collectives inside the graph (NMH_DP_CAPTURE_COMM=1) would run k times and are refused.
    accumulate = 1 is the step of before: the same graphs, the same launches."""

    MAX_EXT_ROWS, MAX_MASK_BITS = 16, 4096   # capacity of one nmh_step_params launch (csrc/misc.hip: ext[48], bits[128])

    def __init__(self, model, opt: FusedAdamW, batch: int, reducer=None, warmup: int = 2, accumulate: int = 1):
        import os
        if int(accumulate) < 1:
            raise ValueError(f"GraphedTrainStep: accumulate >= 1, got {accumulate}")
        if accumulate > 1 and reducer is not None and os.environ.get("NMH_DP_CAPTURE_COMM", "0") == "1":
            raise ValueError("GraphedTrainStep: NMH_DP_CAPTURE_COMM=1 puts the collectives inside the backward graph, which accumulate > 1 replays once per "
                             "micro-batch; gradient accumulation exchanges each range once per optimizer step, between the replays (unset the variable)")
        if opt.accumulate not in (1, int(accumulate)):
            raise ValueError(f"GraphedTrainStep: accumulate = {accumulate}, but the optimizer was built with accumulate = {opt.accumulate}")
        model.refuse_frozen_stages("GraphedTrainStep")
        self.model, self.opt, self.reducer = model, opt, reducer
        self.accumulate = int(accumulate)
        if self.accumulate > 1:
            opt.accumulate, opt.mean_clip = self.accumulate, True
        dev = model.mask_token.device
        R, g = model.resolution, model.resolution // 4
        self.x = torch.zeros((batch, 4, R, R, R), device=dev)
        self.ext = torch.full((batch, 3), R, dtype=torch.int32, device=dev)
        self.mask = torch.zeros(g ** 3, dtype=torch.uint8, device=dev)
        # what the step is captured for (model.EmbedBound): rows per sample of the compact patch embed of the kept tokens, from the mask distribution, and masks
        # that are constant on every 4^3 window, as the block masks are (stage 0's first block on the kept windows only, ops.BLOCK0_KEPT).  Every mask is checked
        # against it in __call__ / begin (_fit_capture): one that keeps more tokens, or cuts through windows, re-captures the step with the widened bound
        from .model import EmbedBound, embed_capacity_rows
        self.bound = EmbedBound(embed_capacity_rows(g, p_remove=model.masking_prob), bool(ops.BLOCK0_KEPT and g % 4 == 0))
        self.losses = None
        if self.accumulate > 1:
            # outside the graphs' pool: the sum of the micro-batches' three losses, and their mean (the optimizer graph writes it and clears the sum)
            self._loss_sum, self.losses = torch.zeros(3, device=dev), torch.zeros(3, device=dev)
            self._n_micro = self._done = 0
        self._ext_host = None
        self._g1 = self._g2 = None
        self._gb, self._ranges = [], []
        self._warm = warmup
        self.overlap = True    # False: every collective on the main stream (A/B measurement of what the overlap hides)
        if reducer is not None and reducer.world > 1 and len(reducer.stage_bounds) != 7:
            raise ValueError("GraphedTrainStep: the data-parallel step expects the gradient segments of a 4-stage encoder + decoder")
        self.comm_captured = False

    def __del__(self):
        st = getattr(self, "_capture_stream", None)
        if st is not None:   # workspaces keyed by this step's capture stream go with it (ops.swin_mlp_split_ws)
            try:
                ops.swin_mlp_split_ws_drop_stream(st.cuda_stream)
            except Exception:  # noqa: BLE001  (interpreter shutdown)
                pass

    def set_extents(self, ext):
        """valid extents [B][3] of the batch now in `self.x` (host list / tensor) -> static device buffer, through a pinned ring"""
        self._ext_host = [[int(v) for v in row] for row in (ext.tolist() if hasattr(ext, "tolist") else ext)]   # sent with the next step's parameters

    def _fwd_bwd(self, zero=True):
        if zero:
            self.model.zero_grad()
        out = self.model.forward_static(self.x, self.ext, self.mask, self.bound)
        out[0].backward()
        return out

    def _capture(self):
        import os
        import torch.distributed as tdist
        ops.side_stream.auto(self.x.shape[0])
        # NMH_DP_FORCE_SPLIT=1 / NMH_DP_FORCE=1: the data-parallel step also with a one-rank group (tools/bench_dp_overhead.py: what the machinery costs)
        dp = self.reducer is not None and (self.reducer.active or os.environ.get("NMH_DP_FORCE_SPLIT") == "1")
        # RCCL collectives CAN be captured into a HIP graph on this stack (tools/probe_rccl_capture.py: replay == eager).  With
        # NMH_DP_CAPTURE_COMM=1 the whole step -- forward, backward with the range all-reduces launched by the autograd triggers on the comm
        # stream, join, clip + AdamW -- is ONE graph without host-side replay boundaries.  Measured over a one-rank RCCL group
        # (tools/bench_dp_overhead.py, ms/step at 1 / 8 grids): single process 12.38 / 58.93, split graphs 13.07 / 60.20, one graph with the
        # collectives inside 13.41 / 60.67 -- no gain on one GPU (what both pay is the bf16 bucket casts and the joins of the weight-gradient
        # side stream in front of every exchange), and plain collectives between graph replays are the more conservative use of RCCL for a
        # first multi-GPU run, so the DEFAULT keeps the collectives outside: the step is cut into pieces at the gradient-range boundaries.
        self.comm_captured = (dp and self.reducer.active and self.reducer.on_gpu and tdist.is_initialized() and tdist.get_backend(self.reducer.group) == "nccl"
                              and os.environ.get("NMH_DP_CAPTURE_COMM", "0") == "1" and os.environ.get("NMH_DP_FORCE_SPLIT") != "1")
        split = dp and not self.comm_captured
        # split mode: the eager path's autograd triggers would issue collectives on the comm stream inside the capture, graph mode owns the
        # exchange (see __call__); captured mode: the triggers ARE the exchange
        self.model._reducer = self.reducer if self.comm_captured else None
        # ONE stream for the warm-up and for every capture below: workspaces that are keyed by the launch stream (ops.swin_mlp_split_ws) are then
        # allocated eagerly by the warm-up, never from a graph's private pool, and their arrival counters are cleared before the capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        ops.swin_mlp_split_ws_reset()
        self._capture_stream = s
        with torch.cuda.stream(s):
            for _ in range(self._warm):
                # warm-up touches no optimizer state (lazy kernel attributes / allocator pools only)
                if split:
                    self._split_a(zero=True)
                    for j in range(len(self._pieces["back"])):
                        self._split_back(j)
                    self._pieces = None
                else:
                    self._fwd_bwd()
                    if self.comm_captured:
                        self.reducer.finish()
        torch.cuda.current_stream().wait_stream(s)
        # inside the replayed step the gradient buffer is cleared by the optimizer kernel of the previous step (hyper[7]); only the
        # first replay needs it cleared here
        self.opt.zero_grads_after_step = True
        self.model.zero_grad()
        torch.cuda.synchronize()
        self._g1 = torch.cuda.CUDAGraph()
        if not split:
            with torch.cuda.graph(self._g1, stream=s, capture_error_mode=_CAPTURE_MODE):
                out = self._fwd_bwd(zero=False)
                if self.comm_captured:
                    self.reducer.finish()      # ranges whose trigger did not fire (the embed tail) + join of the comm stream
                self._keep_losses(out)
                if self.accumulate == 1:
                    self.opt.launch()
            if self.accumulate > 1:
                self._g2 = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self._g2, pool=self._g1.pool(), stream=s, capture_error_mode=_CAPTURE_MODE):
                    self._optimizer_piece()
            return
        # data parallel, collectives outside the graphs: the step is cut where gradient ranges complete, and the collectives run BETWEEN the replays on the comm
        # stream (RCCL stays outside the captured regions), overlapping the next piece of the backward:
        #   g1  = forward + decoder backward                              -> all-reduce [decoders, head]
        #   gb[0] = backward of stage 3 and the LAST third of stage 2     -> all-reduce [stage 2 blocks 12.., stage 3]
        #   gb[1], gb[2] = backward of the middle / first third of stage 2 -> all-reduce of that third (the first exchange of the 48.9 M
        #                  stage-2/3 parameters is in flight while two thirds of stage 2 are still in backward)
        #   gb[3] = backward of stages 1, 0, the embed                    -> all-reduce [mask token, embed, stage 0, stage 1]
        #   g2 = clip + AdamW
        with torch.cuda.graph(self._g1, stream=s, capture_error_mode=_CAPTURE_MODE):
            out = self._split_a(zero=False)
            self._keep_losses(out)
        pool = self._g1.pool()
        self._gb = []
        for k in range(len(self._pieces["back"])):
            gk = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gk, pool=pool, stream=s, capture_error_mode=_CAPTURE_MODE):
                self._split_back(k)
            self._gb.append(gk)
        self._g2 = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._g2, pool=pool, stream=s, capture_error_mode=_CAPTURE_MODE):
            self._optimizer_piece()
        self._pieces = None

    def _keep_losses(self, out):
        """inside a capture, after the forward: the step's three losses; under accumulation added to the sum over the micro-batches"""
        losses = torch.stack([o.detach() for o in out[:3]])
        if self.accumulate > 1:
            self._loss_sum += losses
        else:
            self.losses = losses

    def _optimizer_piece(self):
        """inside a capture: clip + AdamW; under accumulation also the mean of the micro-batches' losses, and their sum cleared for the next step"""
        self.opt.launch()
        if self.accumulate > 1:
            torch.mul(self._loss_sum, self.opt.inv_k, out=self.losses)
            self._loss_sum.zero_()

    # ---- the step in autograd pieces (data-parallel graph mode) ----------------------------------------------------------------------
    def _stage2_chunks(self):
        """block groups of the chunked encoder stage (dist.GradReducer.chunk_groups: stage 2 in three groups of six blocks for swin_s)"""
        from .dist import stage_chunk_groups
        if self.reducer is not None and self.reducer.chunk_groups:
            return self.reducer.chunk_groups
        return stage_chunk_groups(self.model, 2, 3)

    def _split_a(self, zero=True):
        """forward + decoder backward.  The encoder features enter the decoder (and every later piece enters the next) through detached
        leaves, so each piece is its own autograd graph whose incoming gradients are the `.grad` of those leaves."""
        from .model import _StageFlushFn, SwinBlock3D, wgrad_queue_for
        m = self.model
        if zero:
            m.zero_grad()
        B, R = self.x.shape[0], m.resolution
        g = R // 4
        m._packer.run(late_split=False)   # the stages are captured into separate graphs
        tok, b0 = m._embed(self.x, self.mask, self.bound)
        sd = m._draw_sd_noise(B, tok.device)
        m._wq.sync_after_flush = False
        f0, bi = m._run_stage(0, tok, sd, 0, b0=b0)
        f1, bi = m._run_stage(1, f0, sd, bi)
        e1 = f1.detach().requires_grad_()
        groups = self._stage2_chunks()
        q = wgrad_queue_for(m, m.compute_dtype)
        x, ins, outs = e1, [], []
        for k, grp in enumerate(groups):
            ins.append(x)
            y = _StageFlushFn.apply(x, q) if q is not None else x     # backward of the group ends by issuing its queued weight gradients
            for mod in grp:
                if isinstance(mod, SwinBlock3D):
                    y = mod(y.contiguous(), None if sd is None else sd[bi])
                    bi += 1
                else:
                    y = mod(y.contiguous())
            outs.append(y)
            x = y.detach().requires_grad_() if k + 1 < len(groups) else y
        f2 = outs[-1]
        f3, bi = m._run_stage(3, f2, sd, bi)
        d = [f.detach().requires_grad_() for f in (f0, f1, f2, f3)]
        losses = m._decode_and_loss(d, self.x, self.ext, self.mask, None)
        losses[0].backward()
        # gradient ranges of the pieces (element offsets into the flat buffers; parameters lie in module order)
        off = m._offsets
        first = lambda mod: min(off[id(p)] for p in mod.parameters() if p.requires_grad)  # noqa: E731
        b = self.reducer.stage_bounds if self.reducer is not None else None
        s2_lo, s3_hi = (b[3], b[5]) if b is not None else (first(m.stages[2]), first(m.decoder4))
        starts = [s2_lo] + [first(grp[0]) for grp in groups[1:]]
        back = []
        n = len(groups)
        for k in range(n - 1, -1, -1):       # backward order: last group (together with stage 3) first
            hi = s3_hi if k == n - 1 else starts[k + 1]
            back.append({"kind": "s2", "k": k, "lo": starts[k], "hi": hi})
        back.append({"kind": "s01", "lo": 0, "hi": s2_lo})
        self._pieces = {"f": (f0, f1, f2, f3), "e1": e1, "d": d, "ins": ins, "outs": outs, "back": back}
        self._ranges = [(p["lo"], p["hi"]) for p in back]
        return losses[0], losses[1], losses[2]

    def _split_back(self, j: int):
        """piece j of the encoder backward (see _capture)"""
        P = self._pieces
        pc = P["back"][j]
        f0, f1, f2, f3 = P["f"]
        d, ins, outs = P["d"], P["ins"], P["outs"]
        if pc["kind"] == "s2":
            k = pc["k"]
            if k == len(outs) - 1:
                torch.autograd.backward([f3, f2], [d[3].grad, d[2].grad])
            else:
                torch.autograd.backward([outs[k]], [ins[k + 1].grad])
        else:
            e1 = P["e1"]
            ops.add_inplace(e1.grad, d[1].grad)     # stage 1's output feeds stage 2 and decoder3's skip connection
            torch.autograd.backward([f1, f0], [e1.grad, d[0].grad])

    def _load(self, grids):
        """a list of (4,a0,a1,a2) tensors -> the static batch and its extents"""
        self.x.zero_()
        ext = []
        for i, t in enumerate(grids):
            a0, a1, a2 = t.shape[1:]
            self.x[i, :, :a0, :a1, :a2].copy_(t, non_blocking=True)
            ext.append([a0, a1, a2])
        self.set_extents(ext)

    def _mask_bits(self, block_mask, upload: bool = True):
        """the block bits that travel as kernel arguments, or None for a mask that has to be uploaded whole -- which happens here unless upload=False"""
        from .model import block_bits_of_mask
        g = self.model.resolution // 4
        bits = block_mask if isinstance(block_mask, np.ndarray) and block_mask.shape != (g, g, g) else block_bits_of_mask(block_mask)
        if bits is None:   # an arbitrary (not block-structured) token mask: uploaded through the event-guarded pinned ring
            if upload:
                if getattr(self, "_pin_mask", None) is None:
                    self._pin_mask = PinnedRing((self.mask.numel(),), torch.uint8)
                self._pin_mask.upload(torch.as_tensor(block_mask).to(torch.uint8), self.mask)
        elif bits.shape[0] ** 3 > self.MAX_MASK_BITS:   # more blocks than the launch's argument struct holds (resolution > 256): full mask upload
            if upload:
                full = np.zeros((g, g, g), dtype=np.uint8)
                blk = np.asarray(bits, dtype=np.uint8).repeat(4, 0).repeat(4, 1).repeat(4, 2)
                full[:blk.shape[0], :blk.shape[1], :blk.shape[2]] = blk
                if getattr(self, "_pin_mask", None) is None:
                    self._pin_mask = PinnedRing((self.mask.numel(),), torch.uint8)
                self._pin_mask.upload(torch.from_numpy(full), self.mask)
            bits = None
        return bits

    def _fit_capture(self, block_mask, bits):
        """capture the step again where `block_mask` does not fit what was captured: a mask that cuts through 4^3 windows, or keeps more tokens than the embed has
        rows for.  The warm-up of a capture clears the gradient buffer, so under accumulation this runs for every mask of a step before its first replay."""
        from .model import mask_kept_aligned, refit_bound
        g = self.model.resolution // 4
        new = refit_bound(self.bound, g, *mask_kept_aligned(g, block_mask, bits))
        if new is not None:
            self.bound = new
            torch.cuda.synchronize()
            self._capture()

    def _send(self, bits, hyper):
        """mask bits + optimizer hyper-parameters + extents as kernel arguments of one launch: nothing in the step waits on a copy.
        The argument struct holds 16 samples' extents (nmh_step_params): larger batches send the rest in further launches."""
        g = self.model.resolution // 4
        ext, self._ext_host = self._ext_host, None
        first = ext[:self.MAX_EXT_ROWS] if ext is not None else None
        ops.step_params(tokmask=self.mask if bits is not None else None, block_bits=bits, nb=0 if bits is None else bits.shape[0], g=g,
                        hyper=hyper, hyper_dev=self.opt.hyper if hyper is not None else None, extents=first, extents_dev=self.ext if ext is not None else None)
        if ext is not None:
            for i0 in range(self.MAX_EXT_ROWS, len(ext), self.MAX_EXT_ROWS):
                ops.step_params(extents=ext[i0:i0 + self.MAX_EXT_ROWS], extents_dev=self.ext[i0:i0 + self.MAX_EXT_ROWS])

    def _replay_dp(self, exchange: bool):
        """the pieces of the data-parallel step after g1, up to the optimizer graph; exchange=False: a micro-step that only accumulates, no collective"""
        red, b = self.reducer, self.reducer.stage_bounds
        if exchange:
            red.allreduce_range(b[5], b[6], overlap=self.overlap)
        for gk, (lo, hi) in zip(self._gb, self._ranges):
            gk.replay()
            if exchange:
                red.allreduce_range(lo, hi, overlap=self.overlap)
        if exchange:
            red.wait()

    def __call__(self, grids=None, block_mask=None):
        """grids: optional list of (4,a0,a1,a2) tensors (copied into the static batch); block_mask: uint8 (g,g,g) host tensor.
        accumulate > 1: `grids` is the list of the step's micro-batches, each such a list, and `block_mask` the list of their masks, one per micro-batch;
        1 <= len <= accumulate.  Returns the mean of the micro-batches' losses."""
        if self.accumulate > 1:
            if grids is None or block_mask is None or len(grids) != len(block_mask):
                raise ValueError("GraphedTrainStep(accumulate > 1): one list of grids and one block mask per micro-batch")
            self._load(grids[0])       # (a capture in begin() warms up on the static batch)
            self.begin(block_mask)
            for j, mb in enumerate(grids):
                if j > 0:
                    self._load(mb)
                self.micro(j)
            return self.finish()
        if grids is not None:
            self._load(grids)
        if self._g1 is None:
            self._capture()
        self.opt.update_hyper(upload=False)
        bits = None
        if block_mask is not None:
            bits = self._mask_bits(block_mask)
            self._fit_capture(block_mask, bits)
        self._send(bits, self.opt.hyper_host)
        self._g1.replay()
        if self._g2 is not None:
            self._replay_dp(exchange=True)
            self._g2.replay()
        return self.losses

    # ---- accumulate > 1: the optimizer step in pieces ---------------------------------------------------------------------------------------
    def begin(self, masks):
        """start an optimizer step of len(masks) micro-batches: advance the optimizer's step count, set the micro-gradients' weight 1 / len(masks), and make
        the captured step fit EVERY mask of the step before its first replay (a later capture would clear the gradients accumulated so far)"""
        if self.accumulate == 1:
            raise RuntimeError("GraphedTrainStep.begin: the step was built without accumulation; call it")
        if not 1 <= len(masks) <= self.accumulate:
            raise ValueError(f"GraphedTrainStep.begin: 1 .. {self.accumulate} micro-batches, got {len(masks)}")
        if self._done != self._n_micro:
            raise RuntimeError(f"GraphedTrainStep.begin: the step before has run {self._done} of its {self._n_micro} micro-batches")
        if self._g1 is None:
            self._capture()
        for bm in masks:
            self._fit_capture(bm, self._mask_bits(bm, upload=False))
        self.opt.update_hyper(upload=False)
        self.opt.set_grad_scale(1.0 / len(masks))
        self._masks, self._n_micro, self._done = list(masks), len(masks), 0

    def micro(self, j: int):
        """micro-batch j of the step, now in `x` with its extents set: forward + backward added to the gradient buffer.  Data-parallel: the last one exchanges."""
        if j != self._done or j >= self._n_micro:
            raise RuntimeError(f"GraphedTrainStep.micro: micro-batch {j} after {self._done} of {self._n_micro}")
        self._send(self._mask_bits(self._masks[j]), self.opt.hyper_host if j == 0 else None)
        self._g1.replay()
        if self._gb:
            self._replay_dp(exchange=j == self._n_micro - 1)
        self._done += 1

    def finish(self):
        """clip + AdamW on the mean gradient -> the mean of the micro-batches' losses (device tensor; valid until the next step's finish())"""
        if self._n_micro == 0 or self._done != self._n_micro:
            raise RuntimeError(f"GraphedTrainStep.finish: {self._done} of {self._n_micro} micro-batches have run")
        self._g2.replay()
        self._n_micro = self._done = 0
        return self.losses


# --------------------------------------------------------------------------------------------------
# Trainer parity extras: metrics, checkpoints, epoch loop
# --------------------------------------------------------------------------------------------------
def mse(pred_rgb: torch.Tensor, target_rgb: torch.Tensor, valid_mask: torch.Tensor) -> torch.Tensor:
    """mean squared error over the RGB entries of the voxels selected by valid_mask (nerf_rpn/model/metrics.py:69-75);
    evaluation-only bookkeeping on the eval tuple (stock tensor ops, not part of the training step)"""
    err = (pred_rgb - target_rgb) ** 2
    return err[valid_mask.expand_as(err)].mean()


def psnr(pred_rgb: torch.Tensor, target_rgb: torch.Tensor, valid_mask: torch.Tensor) -> torch.Tensor:
    """-10 log10(mse) (metrics.py:78-79)"""
    return -10.0 * torch.log10(mse(pred_rgb, target_rgb, valid_mask))


def eval_metrics(eval_out) -> tuple:
    """(psnr, mse) of one `model(x, is_eval=True)` 6-tuple exactly as the reference's eval loop computes them
    (run_swin_mae3d.py:747-760).  Both also follow from the fused loss: mse == loss_rgb / 3, because loss_rgb divides the same
    masked sum by the voxel count instead of the entry count (swin_mae3d.py:1535)."""
    _, _, _, pred, mask, target = eval_out
    m = mask.bool()
    return psnr(pred[..., :3], target[..., :3], m), mse(pred[..., :3], target[..., :3], m)


def _unwrapped(model):
    """the model inside a DDP-style wrapper, or the model itself"""
    return getattr(model, "module", model)


def _write_checkpoint(path: str, sections: dict, epoch: int, train_args: dict, opt=None, step: int = None, flat=None):
    """the one writer behind the four save_*_checkpoint: {"epoch", one entry per section in the order given (a state dict copied to the host, or None),
    "train_args" (stored as passed)} and, with `opt`, the "resume" section (resume_section) over `flat`, the owner of the flat buffers: opt.model unless given."""
    ck = {"epoch": epoch}
    for name, sd in sections.items():
        ck[name] = None if sd is None else {k: v.detach().cpu() for k, v in sd.items()}
    ck["train_args"] = train_args
    if opt is not None:
        ck["resume"] = resume_section(opt.model if flat is None else flat, opt, step)
    torch.save(ck, path)


def _read_checkpoint(path: str, parts, opt=None, who: str = "", strict: bool = True) -> dict:
    """the one reader behind the four load_*_checkpoint.  parts: (section, module, required) triples, loaded in that order; a section that is not required is
    skipped where the file has none (or None).  With `opt` and a "resume" section the optimizer continues where it stopped (restore_resume over opt.model).
    Returns the checkpoint dict."""
    # tensors, numbers, strings, dicts/lists/tuples only: nothing in any checkpoint format needs unpickling of arbitrary objects
    ck = torch.load(path, map_location="cpu", weights_only=True)
    for section, module, required in parts:
        if required or ck.get(section) is not None:
            module.load_state_dict(ck[section], strict=strict)
    if opt is not None and "resume" in ck:
        restore_resume(ck["resume"], opt.model, opt, who)
    return ck


def save_checkpoint(path: str, model, epoch: int, train_args: dict, opt: "FusedAdamW" = None, step: int = None):
    """the reference's checkpoint (run_swin_mae3d.py:471-489): {"epoch", "state_dict", "train_args"}; state_dict keys/shapes are the
    reference's, so nerf_rpn loads it unchanged.  With `opt` the file additionally carries what a TRUE resume needs (the reference
    cannot resume its optimizer): AdamW moments over the flat buffer, step count, beta powers, schedule position."""
    _write_checkpoint(path, {"state_dict": model.state_dict()}, epoch, dict(train_args), opt, step, flat=model)


def flat_layout(model) -> dict:
    """{parameter name: [offset, numel]} of the model's flat fp32 parameter / gradient / moment buffers"""
    return {n: [int(model._offsets[id(p)]), int(p.numel())] for n, p in model.named_parameters() if id(p) in model._offsets}


def resume_section(model, opt, step=None) -> dict:
    """what a TRUE resume needs, as save_checkpoint and save_detection_checkpoint store it under "resume": the AdamW moments over the flat buffer, step count,
    learning rate, betas, schedule position.  The moments are flat buffers in the model's parameter order: the layout (name -> offset, numel) travels with
    them, so a file written under another flat layout (e.g. the 4-element granule of earlier builds) is remapped by name instead of misaligned"""
    r = {"m": opt.m.detach().cpu(), "v": opt.v.detach().cpu(), "t": opt.t, "lr": opt.lr, "betas": tuple(opt.betas), "step": step, "layout": flat_layout(model)}
    if getattr(opt, "range_record", None) is not None:     # FusedAdamW(ranges=): the table the moments were kept under; without one the section is as before
        r["ranges"] = opt.range_record
    if getattr(opt, "accumulate", 1) != 1:                 # FusedAdamW(accumulate=k): the micro-batches per optimizer step the run was scheduled under
        r["accumulate"] = int(opt.accumulate)
    return r


def range_record(rec) -> dict:
    """a range table's host record (finetune.ParamRanges.record, or a resume section's "ranges") in the one form that compares: ints and floats in lists"""
    return {"bounds": [int(b) for b in rec["bounds"]], "scale": [[float(ls), float(ws)] for ls, ws in rec["scale"]]}


def restore_resume(r: dict, model, opt, who: str):
    """the inverse of resume_section: the moments into opt.m / opt.v (remapped by parameter name when the file's flat layout is not this build's), then
    t, lr and betas.  `model` is whatever flat_layout takes (an MAE model or a finetune.FlatParameters)."""
    tab_ck, tab_now = r.get("ranges"), getattr(opt, "range_record", None)
    if (None if tab_ck is None else range_record(tab_ck)) != tab_now:
        # the frozen ranges' moments in the file are whatever they were when freezing began (zero from the start): stepping them under another table, or
        # freezing ranges whose moments are live, would be silent
        raise RuntimeError(f"{who}: the file's optimizer state was kept {'without a range table' if tab_ck is None else 'under a range table of ' + str(len(tab_ck['scale'])) + ' ranges'}"
                           f", this optimizer has {'none' if tab_now is None else ('one' if tab_ck is None else 'another one') + ' of ' + str(len(tab_now['scale'])) + ' ranges'}: build FusedAdamW with the "
                           "same ranges= (the same layer_decay / no_decay / freeze)")
    k_ck, k_now = int(r.get("accumulate", 1)), int(getattr(opt, "accumulate", 1))
    if k_ck != k_now:
        # the file's step count, schedule position and moments belong to optimizer steps of k_ck micro-batches: under another k the same epochs hold another
        # number of steps, and the OneCycle schedule built for them is another one
        raise RuntimeError(f"{who}: the file's run took optimizer steps of {k_ck} micro-batch{'es' if k_ck != 1 else ''} (accumulate = {k_ck}), this one is set up "
                           f"with accumulate = {k_now}: resume with the same accumulate=")
    lay_now, lay_ck = flat_layout(model), r.get("layout")
    if lay_ck is None or {k: list(v) for k, v in lay_ck.items()} == lay_now:
        if r["m"].numel() != opt.m.numel():
            raise RuntimeError(f"{who}: the optimizer state has {r['m'].numel()} elements, this build's flat layout {opt.m.numel()} "
                               "(a file without a 'layout' section written under another parameter granule cannot be remapped)")
        opt.m.copy_(r["m"]); opt.v.copy_(r["v"])
    else:   # another flat layout: remap every parameter's moments by name
        if set(lay_ck) != set(lay_now) or any(lay_ck[k][1] != lay_now[k][1] for k in lay_now):
            raise RuntimeError(f"{who}: the optimizer state belongs to a different parameter set")
        opt.m.zero_(); opt.v.zero_()
        for k, (off, n) in lay_now.items():
            o2 = lay_ck[k][0]
            opt.m[off:off + n].copy_(r["m"][o2:o2 + n]); opt.v[off:off + n].copy_(r["v"][o2:o2 + n])
    opt.t, opt.lr, opt.betas = r["t"], r["lr"], tuple(r["betas"])


def load_checkpoint(path: str, model, opt: "FusedAdamW" = None, strict: bool = True) -> dict:
    """loads a reference-format checkpoint (also one written by the reference itself); returns the checkpoint dict.  With `opt` and
    a "resume" section the optimizer continues where it stopped."""
    ck = _read_checkpoint(path, [("state_dict", model, True)], strict=strict)
    if opt is not None and "resume" in ck:      # (its own tail: the moments lie over the model itself, which must be on the device by now)
        if model._flat is None or not model._flat.is_cuda:
            raise RuntimeError("load_checkpoint: move the model to the HIP device before restoring the optimizer")
        restore_resume(ck["resume"], model, opt, "load_checkpoint")
    return ck


def _eval_epoch(val_scenes, epoch: int, eval_interval: int, epochs: int) -> bool:
    """is `epoch` evaluated: there are validation scenes, and it is a multiple of eval_interval or the last one (from arguments alone: the same on every rank)"""
    return bool(val_scenes) and (epoch % eval_interval == 0 or epoch == epochs)


def _format_record(rec: dict) -> str:
    """one history record as the log line"""
    return " ".join(f"{k}={v:.5g}" if isinstance(v, float) else f"{k}={v}" for k, v in rec.items())


def accum_epoch_plan(batches, k: int):
    """the optimizer steps of one epoch under gradient accumulation: the epoch's batches, in order, in groups of k -- every step has k micro-batches but the last,
    which has what is left (1 .. k; its micro-gradients weigh 1 / that many).  k = 1: one batch per step.  Raises on k < 1."""
    if int(k) != k or k < 1:
        raise ValueError(f"accum_epoch_plan: k >= 1 micro-batches per optimizer step, got {k}")
    batches = list(batches)
    return [batches[i:i + k] for i in range(0, len(batches), k)]


class Trainer:
    """Epoch loop of run_swin_mae3d.py:600-709 without wandb: OneCycle schedule stepped every iteration, HIP-graph train step,
    evaluation every `eval_interval` epochs, `model_best.pt` by validation PSNR (:620-629) and `epoch_{k}.pt`; rank 0 writes.
    `train_scenes` / `val_scenes`: sequences of stored scenes ((W,L,H,4) arrays or paths); sharded across ranks with
    DistributedSampler semantics (dist.shard_indices).

    accumulate = k: an optimizer step takes k consecutive batches of the epoch as micro-batches (accum_epoch_plan; the last step of an epoch
    takes what is left), each with its own mask, and steps on the mean of their gradients: the reference's recipe of batch_size * world * k grids on fewer GPUs.
    steps_per_epoch, global_step, the optimizer's step count and the OneCycle schedule count OPTIMIZER steps; the logged loss is the mean over them of the
    per-step mean; train_args["batch_size"] = batch_size * world * k and train_args["accumulate"] = k.  resume(path) continues after the file's epoch, at an
    optimizer-step boundary; a file written under another k is refused.  INVARIANT (data-parallel): every rank runs the same number of optimizer steps with the
    same number of micro-steps in each, because dist.shard_indices pads the shards to equal length -- the last micro-step of each optimizer step holds the
    collectives, and a rank that ran one fewer would hang the others."""

    def __init__(self, model, train_scenes, val_scenes=None, batch_size: int = 4, num_epochs: int = 1, lr: float = 1e-4, weight_decay: float = 1e-3,
                 clip_grad_norm: float = 0.1, eval_interval: int = 1, save_path: str = None, normalize_density: bool = True, flip_prob: float = 0.0,
                 rotate_prob: float = 0.0, rank: int = 0, world: int = 1, reducer=None, log=print, train_args: dict = None, seed: int = 0, no_decay: bool = False, freeze=(),
                 accumulate: int = 1):
        from . import data, dist as _dist
        from .finetune import param_ranges, recipe_rules, selector_names
        self.model, self.train_scenes, self.val_scenes = model, train_scenes, val_scenes
        self.batch, self.epochs, self.eval_interval, self.save_path = batch_size, num_epochs, eval_interval, save_path
        self.rank, self.world, self.log, self.seed = rank, world, log, seed
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"Trainer: accumulate >= 1, got {accumulate}")
        model.refuse_frozen_stages("Trainer")
        self.accumulate = int(accumulate)
        self.args = dict(train_args or {}, lr=lr, weight_decay=weight_decay, clip_grad_norm=clip_grad_norm, batch_size=batch_size * world * self.accumulate,
                         accumulate=self.accumulate, num_epochs=num_epochs, normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob,
                         no_decay=bool(no_decay), freeze=selector_names(model, freeze))
        self._shard = _dist.shard_indices
        dev = model.mask_token.device
        self.batcher = data.GridBatcher(model.resolution, dev, normalize_density, flip_prob, rotate_prob)
        self.val_batcher = data.GridBatcher(model.resolution, dev, normalize_density)
        rules = recipe_rules(model, None, no_decay, freeze)     # per-range settings; none: the one-setting step
        self.opt = FusedAdamW(model, lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm, ranges=param_ranges(model, rules) if rules else None,
                              accumulate=self.accumulate)
        # the reference's DataLoader has no drop_last: len(train_loader) is the ceiling, and it sizes OneCycleLR (run_swin_mae3d.py:594-598); under accumulation
        # the scheduler is stepped once per optimizer step, so it is sized by those
        self.micro_per_epoch = -(-len(self._shard(len(train_scenes), rank, world, 0)) // batch_size)
        if self.micro_per_epoch < 1:
            raise ValueError("Trainer: empty training shard")
        self.steps_per_epoch = len(accum_epoch_plan(range(self.micro_per_epoch), self.accumulate))
        if world > 1:
            _dist.broadcast_parameters(model)   # DDP's initial broadcast: every rank starts from rank 0's weights
        self.sched = OneCycle(lr, num_epochs * self.steps_per_epoch)
        self.step_fn = GraphedTrainStep(model, self.opt, batch_size, reducer=reducer, accumulate=self.accumulate)
        self.global_step, self.start_epoch, self.best_metric, self.history = 0, 1, None, []

    def _scene(self, s):
        from . import data
        return data.load_scene(s) if isinstance(s, str) else s

    def train_epoch(self, epoch: int):
        import random
        from . import data
        from .model import draw_block_mask
        self.model.train()
        idx = self._shard(len(self.train_scenes), self.rank, self.world, epoch, seed=self.seed)
        g = self.model.resolution // 4
        batches = [[self.train_scenes[i] for i in idx[b * self.batch:(b + 1) * self.batch]] for b in range(self.micro_per_epoch)]
        sizes = [len(step) for step in accum_epoch_plan(range(len(batches)), self.accumulate)]     # micro-batches of every optimizer step
        si = mi = 0
        # input pipeline: batch k+1 is loaded, staged through pinned rings, copied and prepared on a copy stream by a background thread
        # while step k runs (the reference's DataLoader workers); the losses are read back once per epoch, not per step, so the host
        # keeps queueing replays ahead of the device
        if self.step_fn._g1 is None:
            self.step_fn._capture()    # before the producer thread exists: its allocations / copies would invalidate a global-mode capture
        pf = data.Prefetcher(self.batcher, batches, self.batch, load=self._scene, seed=1000003 * self.seed + 7919 * epoch + self.rank)
        main = torch.cuda.current_stream()
        loss_acc = torch.zeros((), device=self.step_fn.x.device)
        for j, xb, ext, ev in pf:
            main.wait_event(ev)
            n = xb.shape[0]
            self.step_fn.x[:n].copy_(xb, non_blocking=True)          # device-to-device into the graph's static input
            pf.done(j, main)
            if n < self.batch:
                # ragged last batch of the epoch (no drop_last in the reference): the unused slots of the static batch become empty
                # grids with zero valid extent -- no voxel of them enters either loss mask, so losses and gradients equal those of
                # the smaller batch
                self.step_fn.x[n:].zero_()
                ext = ext + [[0, 0, 0]] * (self.batch - n)
            self.step_fn.set_extents(ext)
            if self.accumulate > 1:
                if mi == 0:
                    lr, b1 = self.sched.at(self.global_step)
                    self.opt.set_hyper(lr=lr, beta1=b1)
                    # one mask per micro-batch, as every DDP rank draws its own; all of them now: begin() fits the captured step to every one before the first replay
                    self.step_fn.begin([draw_block_mask((g, g, g), self.model.masking_prob, rng=random) for _ in range(sizes[si])])
                self.step_fn.micro(mi)
                mi += 1
                if mi < sizes[si]:
                    continue
                losses = self.step_fn.finish()
                si, mi = si + 1, 0
            else:
                lr, b1 = self.sched.at(self.global_step)
                self.opt.set_hyper(lr=lr, beta1=b1)
                losses = self.step_fn(None, draw_block_mask((g, g, g), self.model.masking_prob, rng=random))
            self.global_step += 1
            loss_acc += losses[0]
        self.prefetch_stats = getattr(pf, "stats", None)
        return float(loss_acc) / self.steps_per_epoch

    @torch.no_grad()
    def evaluate(self):
        self.model.eval()
        ps, ms = [], []
        for s in self.val_scenes:
            xb, ext = self.val_batcher([self._scene(s)], flags=[0])
            a0, a1, a2 = ext[0].tolist()
            out = self.model([xb[0, :, :a0, :a1, :a2]], is_eval=True)
            p, m = eval_metrics(out)
            ps.append(float(p)); ms.append(float(m))
        self.model.train()
        return sum(ps) / len(ps), sum(ms) / len(ms)

    def resume(self, path: str) -> dict:
        """continue a run from a file that fit() wrote: weights, optimizer state, schedule position; fit() then starts at the epoch after the file's, which is an
        optimizer-step boundary (no step spans two epochs).  A file written under another `accumulate` is refused (restore_resume)."""
        ck = load_checkpoint(path, self.model, self.opt)
        self.start_epoch = int(ck["epoch"]) + 1
        step = ck.get("resume", {}).get("step")
        self.global_step = int(step) if step is not None else (self.start_epoch - 1) * self.steps_per_epoch
        return ck

    def fit(self):
        import os
        if self.save_path and self.rank == 0:
            os.makedirs(self.save_path, exist_ok=True)
        for epoch in range(self.start_epoch, self.epochs + 1):
            loss = self.train_epoch(epoch)
            rec = {"epoch": epoch, "train_loss": loss}
            if self.rank == 0 and _eval_epoch(self.val_scenes, epoch, self.eval_interval, self.epochs):
                rec["psnr"], rec["mse"] = self.evaluate()
                if self.save_path:
                    if self.best_metric is None or rec["psnr"] > self.best_metric:
                        self.best_metric = rec["psnr"]
                        save_checkpoint(os.path.join(self.save_path, "model_best.pt"), self.model, epoch, self.args, self.opt, self.global_step)
                    save_checkpoint(os.path.join(self.save_path, f"epoch_{epoch}.pt"), self.model, epoch, self.args, self.opt, self.global_step)
            self.history.append(rec)
            if self.rank == 0:
                self.log(_format_record(rec))
        return self.history


# --------------------------------------------------------------------------------------------------
# Detection fine-tuning: the reference's checkpoint format and the epoch loop of run_fcos_pretrained.py
# --------------------------------------------------------------------------------------------------
def _plain(v):
    """train_args as the weights-only torch.load of _read_checkpoint reads them back: numbers, strings, None and containers of those; anything else by its str()"""
    if isinstance(v, (bool, int, float, str, type(None))):
        return v
    if isinstance(v, dict):
        return {str(k): _plain(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_plain(x) for x in v]
    return str(v)


def save_detection_checkpoint(path: str, model, epoch: int, train_args: dict, opt: "FusedAdamW" = None, step: int = None):
    """the reference's detection checkpoint (run_fcos_pretrained.py:477-497): {"epoch", "backbone_state_dict", "fcos_state_dict", "train_args"} of a
    FCOSOverNeRF, keys and shapes the reference's, so nerf_rpn loads it unchanged.  With `opt` (a FusedAdamW over a finetune.FlatParameters of this model) the
    file also carries the "resume" section of save_checkpoint: moments over the flat buffer, t, lr, betas, step and the name -> [offset, numel] layout."""
    model = _unwrapped(model)
    _write_checkpoint(path, {"backbone_state_dict": model.backbone.state_dict(), "fcos_state_dict": model.fcos_module.state_dict()}, epoch,
                      _plain(dict(train_args)), opt, step)


def load_detection_checkpoint(path: str, model, opt: "FusedAdamW" = None) -> dict:
    """loads a detection checkpoint (also one written by the reference) strictly into model.backbone and model.fcos_module; returns the checkpoint dict.  With
    `opt` and a "resume" section the optimizer continues where it stopped; moments written under another flat layout are remapped by parameter name."""
    model = _unwrapped(model)
    return _read_checkpoint(path, [("backbone_state_dict", model.backbone, True), ("fcos_state_dict", model.fcos_module, True)], opt, "load_detection_checkpoint")


def save_two_stage_checkpoint(path: str, model, epoch: int, train_args: dict, opt: "FusedAdamW" = None, step: int = None, fine_tune: bool = True):
    """the reference's second-stage checkpoint (run_rpn_detect.py:261-269): {"epoch", "backbone_state_dict" (None unless fine_tune), "RCNN_dict", "train_args"} of a
    detector.TwoStageDetector, keys and shapes the reference's, so its RCNN loads "RCNN_dict" unchanged.  The first stage's head, which the reference keeps in
    run_rpn.py's own file, goes under "rpn_state_dict".  With `opt` (a FusedAdamW over a finetune.FlatParameters of this model) the file also carries the
    "resume" section of save_checkpoint, in place of the reference's torch optimizer and scheduler state."""
    model = _unwrapped(model)
    _write_checkpoint(path, {"backbone_state_dict": model.rpn_network.backbone.state_dict() if fine_tune else None,
                             "RCNN_dict": model.roi_model.RCNN_model.state_dict(), "rpn_state_dict": model.rpn_network.rpn.state_dict()}, epoch,
                      _plain(dict(train_args)), opt, step)


def load_two_stage_checkpoint(path: str, model, opt: "FusedAdamW" = None) -> dict:
    """loads a second-stage checkpoint (also one written by the reference) strictly into the parts it carries: "RCNN_dict" always, the backbone and the first
    stage's head where present; returns the checkpoint dict.  With `opt` and a "resume" section the optimizer continues where it stopped."""
    model = _unwrapped(model)
    return _read_checkpoint(path, [("RCNN_dict", model.roi_model.RCNN_model, True), ("backbone_state_dict", model.rpn_network.backbone, False),
                                   ("rpn_state_dict", model.rpn_network.rpn, False)], opt, "load_two_stage_checkpoint")


def delete_suboptimal_checkpoints(checkpoint_dir: str, metric_name: str = "ap50", max_to_keep: int = 6, min_to_keep: int = 1):
    """run_fcos_pretrained.py:507-535: every *.pt of the directory is ranked by the number its name carries -- for "ap50" the second-to-last '_' field, which
    is AP50 under both best-checkpoint name patterns; for "ap25" the last field -- and all but the max(max_to_keep, min_to_keep) highest are removed; ties keep
    the directory order.  A *.pt whose name carries no such number ranks as 0.0 (the reference raises ValueError on it)."""
    import glob
    import os

    def metric(filename):
        parts = filename.split("_")
        try:
            if len(parts) >= 2:
                return float(parts[-1].replace(".pt", "")) if metric_name == "ap25" else float(parts[-2])
        except ValueError:
            pass
        return 0.0

    files = glob.glob(os.path.join(checkpoint_dir, "*.pt"))
    files.sort(key=metric)
    keep = files[-min(max(max_to_keep, min_to_keep), len(files)):] if files else []
    for f in files:
        if f not in keep:
            os.remove(f)


def dp_epoch_plan(n: int, batch: int, rank: int, world: int, epoch: int, seed: int = 0):
    """the batches of one epoch for one rank, as lists of scene indices: rank's shard of dist.shard_indices (the epoch-seeded permutation, padded to a multiple
    of `world`) cut into ceil(len / batch) slices, the last one ragged (no drop_last).  The shards have equal length, so every rank gets the same number of
    steps with the same batch sizes.  Raises on an empty shard (n == 0) and on batch < 1."""
    from .dist import shard_indices
    if batch < 1 or world < 1 or not 0 <= rank < world:
        raise ValueError(f"dp_epoch_plan: batch {batch}, rank {rank} of {world}")
    idx = shard_indices(n, rank, world, epoch, seed=seed)
    if not idx:
        raise ValueError("dp_epoch_plan: empty training shard")
    return [idx[b * batch:(b + 1) * batch] for b in range(-(-len(idx) // batch))]


class _FinetuneTrainer:
    """What DetectionTrainer and VoxelTrainer share: the epoch loop of the reference's fine-tuning scripts without wandb, one process per GPU.

    One optimizer group over ALL parameters (the reference passes model.parameters(): weight decay applies to everything), clip + AdamW by FusedAdamW over
    finetune.FlatParameters, the OneCycle schedule over schedule_epochs * steps_per_epoch steps, stepped every iteration.  No drop_last: the ragged last batch
    of an epoch runs as a smaller batch.  The epoch's logged losses accumulate on the device and are read back once per epoch.  Every `eval_interval` epochs and
    at the last one: evaluate(), in model.eval(); with `save_path` the subclass then keeps its best checkpoints (_keep_best), which carry the optimizer state.
    `resume(path)` continues a run from such a file.

    train_scenes / val_scenes: stored scenes ((W,L,H,4) arrays or paths); train_targets / val_targets: one target per scene, as the subclass's batcher takes it.

    Data-parallel (rank, world, reducer; the conventions of Trainer; the reference wraps the model in DDP, run_fcos_pretrained.py:359-361): `batch_size` is per
    rank and train_args["batch_size"] = batch_size * world (:614); every rank holds all scenes and trains on its shard (dp_epoch_plan).  INVARIANT: every rank
    runs the same number of steps per epoch with the same batch sizes, the ragged last one included, because dist.shard_indices pads the shards to equal length
    -- each step holds collectives (the loss normalisers, the gradient ranges), and a rank that ran one step fewer would hang the others.  The constructor
    broadcasts rank 0's parameters.  Under accumulation the same holds for the micro-steps of every optimizer step (accum_epoch_plan over equal-length plans), and only
    the last micro-step of a step exchanges gradients.  `reducer`: a dist.FlatGradReducer over a finetune.FlatParameters of this model, which the trainer then adopts (that is how
    bf16 buckets are chosen); None with world > 1 builds one with fp32 buckets.  The augmentation draws of rank r come from random.Random(seed + 1000003 * r),
    scene by scene, batch by batch, and nothing else uses that generator.  The accumulated epoch losses are averaged over the ranks in ONE all-reduce per epoch
    (the reference: a barrier and four all-reduces per step, :747-751).  Evaluation and files are rank 0's; the other ranks wait at one barrier per evaluated
    epoch and their `history` carries the training losses only.  With world = 1 nothing of this is active.

    exclude: sub-modules that are frozen as a whole.  They are handed to FlatParameters(exclude=), so the optimizer neither steps nor decays them and a reducer
    does not exchange them (the initial broadcast still sends them once), and they are put back into eval() after every model.train() of the loop.

    layer_decay, no_decay, freeze (the defaults are the one group above): layer-wise learning-rate decay over the encoder's blocks
    (finetune.layer_decay_rules), no weight decay on norms, biases, relative-position tables, mask_token and fcos.Scale (no_decay_rules), and selectors (name
    prefixes, sub-modules, callables) of parameters that stay INSIDE the flat buffers but are not stepped (freeze_rules): the optimizer writes neither them nor
    their moments and clips over the rest; their gradients are still computed and, data-parallel, exchanged.  `freeze` adds to `exclude`; a selector that matches
    only what `exclude` left out is refused.  The three are recorded in train_args, and a resume under other settings is refused (restore_resume).

    freeze_stages = k: the encoder's frozen prefix -- patch embed and stages[:k] -- is frozen as freeze=(patch_partition, *stages[:k]) freezes it
    AND its backward is not run: no gradient kernel, no activation kept, no range exchanged (finetune.frozen_stage_rules, model.frozen_stages).  The prefix stays
    in train() mode and keeps its stochastic-depth draws.  Recorded in train_args; the range table makes a resume under another k refused.  Refused: k outside
    0 .. len(stages), a model without exactly one encoder, and an encoder that `exclude` left out as a whole.

    accumulate = k: an optimizer step takes k consecutive batches of the epoch's plan as micro-batches (accum_epoch_plan; an epoch's last step takes what
    is left) through FinetuneStep.accumulate and steps on the mean of their gradients.  steps_per_epoch, global_step, the optimizer's step count and the schedule
    count optimizer steps; the logged losses are the mean over them of the per-step mean; train_args records accumulate and batch_size = batch * world * k; resume
    continues at an optimizer-step boundary, and a file written under another k is refused (restore_resume).

    A subclass supplies its checkpoint pair (_save_checkpoint, _load_checkpoint) and
      _logged(losses)         the step's detached losses -> the 1-D tensor that the epoch accumulates
      _record(vals)           the epoch's means of _logged, read back as a list -> the training part of the history record
      evaluate()              -> the evaluation part of the record
      _keep_best(epoch, rec)  rank 0 has evaluated `epoch` with record `rec` and there is a save_path: the best-checkpoint policy
    and may override _target(t), a stored target as the batcher takes it."""

    def __init__(self, model, train_scenes, train_targets, val_scenes, val_targets, batcher, val_batcher, loss_fn, weights, args: dict, batch_size: int,
                 num_epochs: int, schedule_epochs: int, lr: float, weight_decay: float, clip_grad_norm: float, eval_interval: int, save_path: str, log, seed: int,
                 rank: int, world: int, reducer, exclude=(), layer_decay: float = None, no_decay: bool = False, freeze=(), accumulate: int = 1,
                 freeze_stages: int = 0):
        import random
        from . import dist as _dist
        from .finetune import FinetuneStep, FlatParameters, _encoder_of, param_ranges, recipe_rules, selector_names
        self.model, self.train_scenes, self.train_targets, self.val_scenes, self.val_targets = model, train_scenes, train_targets, val_scenes, val_targets
        self.batch, self.epochs, self.eval_interval, self.save_path, self.log, self.seed = batch_size, num_epochs, eval_interval, save_path, log, seed
        self.rank, self.world = rank, world
        if int(accumulate) != accumulate or accumulate < 1:
            raise ValueError(f"{type(self).__name__}: accumulate >= 1, got {accumulate}")
        self.accumulate = int(accumulate)
        # (the subclasses pass batch_size = batch * world, the reference's --batch_size; an optimizer step under accumulation takes `accumulate` times as many)
        self.args = _plain(dict(args, batch_size=batch_size * world * self.accumulate, accumulate=self.accumulate, layer_decay=layer_decay, no_decay=bool(no_decay),
                                freeze=selector_names(model, freeze), freeze_stages=freeze_stages))
        self.batcher, self.val_batcher = batcher, val_batcher
        self.exclude = tuple(exclude)                            # the frozen part: outside the flat buffers, kept in eval()
        who = type(self).__name__
        if isinstance(freeze_stages, bool) or int(freeze_stages) != freeze_stages:
            raise ValueError(f"{who}: freeze_stages = {freeze_stages!r}; it is the number of leading encoder stages to freeze, 0 for none")
        if freeze_stages:
            left_out = {id(m) for e in self.exclude for m in e.modules()}
            if id(_encoder_of(model, who)) in left_out:
                raise ValueError(f"{who}: freeze_stages = {freeze_stages} with the backbone left out as a whole (freeze_backbone / a frozen first stage / exclude=): "
                                 "an excluded encoder is already frozen entirely and runs without a graph; drop one of the two")
        if reducer is not None:
            if getattr(reducer.model, "module", None) is not model:
                raise ValueError(f"{type(self).__name__}: the reducer must be a dist.FlatGradReducer over a finetune.FlatParameters of this model")
            if [id(m) for m in getattr(reducer.model, "exclude", ())] != [id(m) for m in self.exclude]:
                raise ValueError(f"{type(self).__name__}: the reducer's FlatParameters must leave out exactly what this trainer freezes (exclude=)")
            self.flat = reducer.model
        else:
            self.flat = FlatParameters(model, next(model.parameters()).device, exclude=self.exclude)
            if world > 1:
                reducer = _dist.FlatGradReducer(self.flat)
        self.reducer = reducer
        if world > 1:
            _dist.broadcast_flat_parameters(self.flat)   # DDP's initial broadcast: every rank starts from rank 0's weights
        # per-range settings: a selector that matches nothing in the flat buffer -- a typo, or a part that `exclude` left out -- is refused
        if self.flat.base is not None:
            self.flat.base.frozen_stages = freeze_stages         # (0 too: a prefix that an earlier trainer left on the encoder would run unstepped but decayed)
        rules = recipe_rules(model, layer_decay, no_decay, freeze, freeze_stages)
        self.opt = FusedAdamW(self.flat, lr=lr, weight_decay=weight_decay, max_grad_norm=clip_grad_norm, ranges=param_ranges(self.flat, rules) if rules else None,
                              accumulate=self.accumulate)
        self.micro_per_epoch = len(dp_epoch_plan(len(train_scenes), batch_size, rank, world, 0, seed))   # len(train_loader) without drop_last, the same on every rank
        self.steps_per_epoch = len(accum_epoch_plan(range(self.micro_per_epoch), self.accumulate))      # optimizer steps: what the schedule counts
        self.sched = OneCycle(lr, schedule_epochs * self.steps_per_epoch)
        self.step_fn = FinetuneStep(self.flat, self.opt, loss_fn, weights=weights, reducer=reducer)
        self._rng = random.Random(seed + 1000003 * rank)         # the augmentation draws: another sequence on every rank
        self.global_step, self.start_epoch, self.history = 0, 1, []

    @staticmethod
    def _load(s):
        from . import data
        return data.load_scene(s) if isinstance(s, str) else s

    @staticmethod
    def _meshes(xb, ext):
        """the batcher's padded batch as the list of grids in their own sizes that the reference forward takes (it pads them again and keeps the sizes)"""
        return [xb[i, :, :e[0], :e[1], :e[2]] for i, e in enumerate(ext)]

    def _target(self, t):
        return t

    def _batch(self, ids):
        """the scenes `ids` -> (meshes, targets) of one step, the augmentation drawn from this rank's generator"""
        xb, ext, targets = self.batcher.prepare([self._load(self.train_scenes[i]) for i in ids], [self._target(self.train_targets[i]) for i in ids], rng=self._rng)
        return self._meshes(xb, ext), targets

    def _train_mode(self):
        """model.train(), the frozen part back in eval(): its features are deterministic (the reference leaves a frozen backbone in train mode, with stochastic
        depth drawing; a stated deviation)"""
        self.model.train()
        for m in self.exclude:
            m.eval()

    def train_epoch(self, epoch: int):
        self._train_mode()
        acc = None
        batches = dp_epoch_plan(len(self.train_scenes), self.batch, self.rank, self.world, epoch, self.seed)     # the DataLoader's shuffle, this rank's shard
        for step in accum_epoch_plan(batches, self.accumulate):
            lr, b1 = self.sched.at(self.global_step)
            self.opt.set_hyper(lr=lr, beta1=b1)
            parts = None
            for ids in step[:-1]:               # all micro-batches but the last: forward and backward only, no collective
                p = self._logged(self.step_fn.accumulate(*self._batch(ids)))
                parts = p if parts is None else parts + p
            out = self.step_fn(*self._batch(step[-1]))
            if parts is None:                   # a step of one batch: the call's own losses, as without accumulation
                parts = self._logged(out)
            else:                               # (the call returns the step's mean; `last` keeps this batch's own losses, which _logged pairs with its side values)
                parts = (parts + self._logged(self.step_fn.last)) / len(step)
            self.global_step += 1
            acc = parts if acc is None else acc + parts
        if self.world > 1:
            import torch.distributed as tdist
            tdist.all_reduce(acc, op=tdist.ReduceOp.SUM)              # the epoch's one exchange of the logged losses: their mean over the ranks
            acc = acc / self.world
        return self._record((acc / self.steps_per_epoch).tolist())   # the epoch's one read-back

    def _save(self, name: str, epoch: int):
        import os
        self._save_checkpoint(os.path.join(self.save_path, name), self.model, epoch, self.args, self.opt, self.global_step)

    def resume(self, path: str) -> dict:
        """continue a run from a file of this trainer's checkpoint writer: weights, optimizer state, schedule position; fit() then starts at the epoch after the
        file's"""
        ck = self._load_checkpoint(path, self.model, self.opt)
        self.flat.check()
        self.start_epoch = int(ck["epoch"]) + 1
        step = ck.get("resume", {}).get("step")
        self.global_step = int(step) if step is not None else (self.start_epoch - 1) * self.steps_per_epoch
        return ck

    def fit(self):
        import os
        if self.save_path and self.rank == 0:
            os.makedirs(self.save_path, exist_ok=True)
        for epoch in range(self.start_epoch, self.epochs + 1):
            rec = {"epoch": epoch, **self.train_epoch(epoch)}
            evaluated = _eval_epoch(self.val_scenes, epoch, self.eval_interval, self.epochs)    # the same decision on every rank
            if evaluated and self.rank == 0:
                rec.update(self.evaluate())
                if self.save_path:
                    self._keep_best(epoch, rec)
            if evaluated and self.world > 1:
                import torch.distributed as tdist
                tdist.barrier()        # the other ranks wait here for rank 0's evaluation and files, once per evaluated epoch
            self.history.append(rec)
            if self.rank == 0:
                self.log(_format_record(rec))
        return self.history


class DetectionTrainer(_FinetuneTrainer):
    """Epoch loop of run_fcos_pretrained.py:537-815 for FCOSOverNeRF (the conventions of _FinetuneTrainer): input from data.DetectionBatcher,
    loss = loss_cls + reg_loss_weight * loss_reg + loss_centerness.

    `schedule_epochs`: the reference sizes its schedule by a literal 1000 epochs whatever --num_epochs says (`total_steps=1000 * len(train_loader)`, :643-647);
    that is the default here, so a run of num_epochs < 1000 stops part-way up or down the cycle exactly as the reference's does.  Pass num_epochs for a
    schedule that ends with the run.

    `train_loss` of the history is the weighted total, `loss_cls` / `loss_reg` / `loss_centerness` the unweighted parts (the reference logs loss_reg after its
    in-place weighting).  Evaluation: detections through the reference forward, scored by DetectionEvaluator with the limits [300, 1000, fpn_post_nms_top_n]
    that do not exceed fpn_post_nms_top_n (:875-877) -> recall at 0.25 / 0.5, AR, AP at 0.25 / 0.5 (train_args["ap_top_n"]: detections kept per scene for AP,
    default all).  Best checkpoints by AP50 and by AP25 under the reference's file names (save_detection_checkpoint), then the best 6 by AP50 are kept
    (delete_suboptimal_checkpoints).

    train_boxes / val_boxes: one [G, 6|7] array per scene.  Data-parallel: the model must have been built with world_size=world (its loss all-reduces the
    normalisers)."""

    _save_checkpoint, _load_checkpoint = staticmethod(save_detection_checkpoint), staticmethod(load_detection_checkpoint)

    def __init__(self, model, train_scenes, train_boxes, val_scenes=None, val_boxes=None, batch_size: int = 2, num_epochs: int = 1, lr: float = 3e-4,
                 weight_decay: float = 1e-3, clip_grad_norm: float = 0.1, reg_loss_weight: float = 1.0, eval_interval: int = 1, save_path: str = None,
                 normalize_density: bool = True, flip_prob: float = 0.0, rotate_prob: float = 0.0, rot_scale_prob: float = 0.0, schedule_epochs: int = 1000,
                 log=print, train_args: dict = None, seed: int = 0, rank: int = 0, world: int = 1, reducer=None, layer_decay: float = None,
                 no_decay: bool = False, freeze=(), accumulate: int = 1, freeze_stages: int = 0):
        from . import data
        from .finetune import fcos_loss_fn
        if len(train_scenes) != len(train_boxes) or (val_scenes is not None and len(val_scenes) != len(val_boxes or [])):
            raise ValueError("DetectionTrainer: one box array per scene")
        if len(train_scenes) < 1:
            raise ValueError("DetectionTrainer: no training scene")
        resolution = getattr(model, "resoluton", None)          # (the reference's spelling, fcos.FCOSOverNeRF)
        if resolution is None:
            raise ValueError("DetectionTrainer: the model needs a fixed resolution (FCOSOverNeRF(..., resolution=R)): the batcher pads every scene to it")
        if world > 1 and getattr(model, "world_size", 1) != world:
            raise ValueError(f"DetectionTrainer: world = {world}, but the model's loss was built with world_size = {getattr(model, 'world_size', 1)}: its two "
                             "normalisers would be per-rank sums and the result silently another; build FCOSOverNeRF(..., world_size=world)")
        self.train_boxes, self.val_boxes, self.reg_loss_weight = train_boxes, val_boxes, reg_loss_weight
        dev = next(model.parameters()).device
        super().__init__(model, train_scenes, train_boxes, val_scenes, val_boxes,
                         data.DetectionBatcher(resolution, dev, normalize_density, flip_prob, rotate_prob, rot_scale_prob),
                         data.DetectionBatcher(resolution, dev, normalize_density), fcos_loss_fn(model), {"loss_reg": reg_loss_weight},
                         dict(train_args or {}, lr=lr, weight_decay=weight_decay, clip_grad_norm=clip_grad_norm, reg_loss_weight=reg_loss_weight,
                              batch_size=batch_size * world, num_epochs=num_epochs, normalize_density=normalize_density, flip_prob=flip_prob,
                              rotate_prob=rotate_prob, rot_scale_prob=rot_scale_prob),
                         batch_size, num_epochs, schedule_epochs, lr, weight_decay, clip_grad_norm, eval_interval, save_path, log, seed, rank, world, reducer,
                         layer_decay=layer_decay, no_decay=no_decay, freeze=freeze, accumulate=accumulate, freeze_stages=freeze_stages)
        self.top_n = int(model.args.fpn_post_nms_top_n)
        self.limits = [l for l in (300, 1000, self.top_n) if l <= self.top_n]
        self.ap_top_n = (train_args or {}).get("ap_top_n")
        self.best_metric_ap50 = self.best_metric_ap25 = None

    def _logged(self, losses):
        return torch.stack([losses["loss_cls"], losses["loss_reg"], losses["loss_centerness"]])

    def _record(self, vals):
        cls, reg, ctr = vals
        return {"train_loss": cls + self.reg_loss_weight * reg + ctr, "loss_cls": cls, "loss_reg": reg, "loss_centerness": ctr}

    @torch.no_grad()
    def evaluate(self):
        from .det_eval import DetectionEvaluator
        self.model.eval()
        ev = DetectionEvaluator(limits=self.limits, ap_thresholds=(0.25, 0.5), top_k=self.ap_top_n)
        for b in range(0, len(self.val_scenes), self.batch):
            scenes = [self._load(s) for s in self.val_scenes[b:b + self.batch]]
            xb, ext, gt = self.val_batcher.prepare(scenes, list(self.val_boxes[b:b + self.batch]), params=[(0, 0.0, 1.0)] * len(scenes))
            boxes, _, scores = self.model(self._meshes(xb, ext))
            ev.update([p[:, 1:] for p in boxes], list(scores), list(gt))       # column 0 is the level index (the reference drops it too, :857-858)
        self.model.train()
        out = ev.compute()
        rec = {}
        for l in self.limits:
            for key in ("25", "50", "ar"):
                rec[f"recall_{key}_top_{l}"] = float(out[f"recall_{key}_top_{l}"]["ar"])
        rec["ap_25"], rec["ap_50"] = float(out["ap_25"]["ap"]), float(out["ap_50"]["ap"])
        return rec

    def _keep_best(self, epoch: int, rec: dict):
        ap50, ap25 = rec["ap_50"], rec["ap_25"]
        if self.best_metric_ap50 is None or ap50 > self.best_metric_ap50:
            self.best_metric_ap50 = ap50
            self._save(f"model_best_ap50_ap25_{ap50}_{ap25}.pt", epoch)
        if self.best_metric_ap25 is None or ap25 > self.best_metric_ap25:
            self.best_metric_ap25 = ap25
            self._save(f"model_best_ap25_ap50_{ap50}_{ap25}.pt", epoch)
        delete_suboptimal_checkpoints(self.save_path, "ap50", 6, 1)


# --------------------------------------------------------------------------------------------------
# The RPN and the two-stage detector: the epoch loops of run_rpn.py and run_rpn_detect.py
# --------------------------------------------------------------------------------------------------
def save_rpn_checkpoint(path: str, model, epoch: int, train_args: dict, opt: "FusedAdamW" = None, step: int = None):
    """the reference's RPN checkpoint (run_rpn.py:294-300): {"epoch", "backbone_state_dict", "rpn_head_state_dict" (= model.rpn.head.state_dict()), "train_args"}
    of a NeRFRegionProposalNetwork, keys and shapes the reference's.  The backbone is written whether it trained or not, as the reference does.  With `opt` (a
    FusedAdamW over a finetune.FlatParameters of this model) the file also carries the "resume" section of save_checkpoint."""
    model = _unwrapped(model)
    _write_checkpoint(path, {"backbone_state_dict": model.backbone.state_dict(), "rpn_head_state_dict": model.rpn.head.state_dict()}, epoch,
                      _plain(dict(train_args)), opt, step)


def load_rpn_checkpoint(path: str, model, opt: "FusedAdamW" = None, backbone_only: bool = False) -> dict:
    """loads an RPN checkpoint (also one written by the reference) strictly into model.backbone and model.rpn.head; returns the checkpoint dict.
    backbone_only: the backbone alone, the reference's --load_backbone_only (run_rpn.py:189-191); the optimizer is then left as it is.  Otherwise, with `opt`
    and a "resume" section, the optimizer continues where it stopped."""
    model = _unwrapped(model)
    parts = [("backbone_state_dict", model.backbone, True)] + ([] if backbone_only else [("rpn_head_state_dict", model.rpn.head, True)])
    return _read_checkpoint(path, parts, None if backbone_only else opt, "load_rpn_checkpoint")


def keep_latest_checkpoints(checkpoint_dir: str, keep_latest: int = 5):
    """delete_old_checkpoints of run_rpn.py:302-308 and run_rpn_detect.py:271-277: of the directory's epoch_*.pt the `keep_latest` newest by modification time
    stay (equal times: the higher epoch is the newer), the others are removed; the model_best* files are not touched.  keep_latest < 1 raises ValueError (the
    reference's slice keeps everything there)."""
    import glob
    import os
    import re
    if int(keep_latest) < 1:
        raise ValueError(f"keep_latest_checkpoints: keep_latest >= 1, got {keep_latest}")

    def age(f):
        m = re.search(r"epoch_(\d+)\.pt$", f)
        return os.path.getmtime(f), int(m.group(1)) if m else -1

    files = sorted(glob.glob(os.path.join(checkpoint_dir, "epoch_*.pt")), key=age)
    for f in files[:max(len(files) - int(keep_latest), 0)]:
        os.remove(f)


def proposal_limits(top_n: int):
    """the proposal limits of the reference's evaluations: those of [300, 1000, top_n] that do not exceed top_n (run_rpn.py:533-535)"""
    return [l for l in (300, 1000, int(top_n)) if l <= int(top_n)]


def _loss_record(keys, vals, weights: dict) -> dict:
    """the epoch means of the unweighted losses -> {"train_loss": sum(weights.get(k, 1) * v), then every loss under its key}: FinetuneStep's total"""
    rec = {"train_loss": sum(float(weights.get(k, 1.0)) * v for k, v in zip(keys, vals))}
    rec.update(zip(keys, vals))
    return rec


def _backbone_resolution(backbone):
    for owner in (backbone, getattr(backbone, "base", None)):
        r = getattr(owner, "resolution", None)
        if isinstance(r, int):
            return r
    return None


def _dense_targets(gt, device):
    """per-scene box tensors -> (gt_boxes [N, Gmax, 6|7] zero-padded, gt_counts [N] int32), what DetectionEvaluator.update takes in its dense form; no host wait"""
    import torch.nn.functional as F
    gmax = max(max(int(g.shape[0]) for g in gt), 1)
    dense = torch.stack([F.pad(g.to(device=device, dtype=torch.float32), (0, 0, 0, gmax - int(g.shape[0]))) for g in gt])
    return dense, torch.tensor([int(g.shape[0]) for g in gt], dtype=torch.int32).to(device, non_blocking=True)


class _BoxTrainer(_FinetuneTrainer):
    """What RPNTrainer and TwoStageTrainer share: the argument checks, the two DetectionBatchers, the loss bookkeeping by key, the validation loop in the
    evaluator's dense form and the reference's keep-the-newest policy."""

    def _setup(self, model, backbone, train_scenes, train_boxes, val_scenes, val_boxes, resolution, loss_fn, weights, keys, common: dict, exclude):
        from . import data
        who = type(self).__name__
        if len(train_scenes) != len(train_boxes) or (val_scenes is not None and len(val_scenes) != len(val_boxes or [])):
            raise ValueError(f"{who}: one box array per scene")
        if len(train_scenes) < 1:
            raise ValueError(f"{who}: no training scene")
        if resolution is None:
            resolution = _backbone_resolution(backbone)
        if resolution is None:
            raise ValueError(f"{who}: the backbone exposes no resolution; pass resolution=R (the batcher pads every scene to it)")
        if int(common["keep_checkpoints"]) < 1:
            raise ValueError(f"{who}: keep_checkpoints >= 1")
        self.train_boxes, self.val_boxes, self.weights, self.keys = train_boxes, val_boxes, dict(weights), tuple(keys)
        self.keep_checkpoints, self.top_k = int(common["keep_checkpoints"]), common["top_k"]
        c = common
        dev = next(model.parameters()).device
        _FinetuneTrainer.__init__(self, model, train_scenes, train_boxes, val_scenes, val_boxes,
                                  data.DetectionBatcher(resolution, dev, c["normalize_density"], c["flip_prob"], c["rotate_prob"], c["rot_scale_prob"]),
                                  data.DetectionBatcher(resolution, dev, c["normalize_density"]), loss_fn, weights, c["args"], c["batch_size"], c["num_epochs"],
                                  c["schedule_epochs"] or c["num_epochs"], c["lr"], c["weight_decay"], c["clip_grad_norm"], c["eval_interval"], c["save_path"],
                                  c["log"], c["seed"], c["rank"], c["world"], c["reducer"], exclude=exclude, layer_decay=c["layer_decay"], no_decay=c["no_decay"],
                                  freeze=c["freeze"], accumulate=c["accumulate"], freeze_stages=c["freeze_stages"])

    def _logged(self, losses):
        return torch.stack([losses[k] for k in self.keys])

    def _record(self, vals):
        return _loss_record(self.keys, vals, self.weights)

    def _val_batches(self):
        """the validation scenes in order, `batch` at a time, without augmentation -> (meshes, gt_boxes [N, Gmax, 6|7], gt_counts [N])"""
        for b in range(0, len(self.val_scenes), self.batch):
            scenes = [self._load(s) for s in self.val_scenes[b:b + self.batch]]
            xb, ext, gt = self.val_batcher.prepare(scenes, list(self.val_boxes[b:b + self.batch]), params=[(0, 0.0, 1.0)] * len(scenes))
            yield (self._meshes(xb, ext), *_dense_targets(gt, xb.device))

    def resume(self, path: str) -> dict:
        """_FinetuneTrainer.resume, and the samplers' counters: each draws once per step (rpn_sample, roi_targets: "the counter advances by one"), so the
        run continues with the draws an uninterrupted one would make when the counters are set to the file's step"""
        ck = super().resume(path)
        # under accumulation a draw per MICRO-step: whole epochs of micro_per_epoch, then `accumulate` per optimizer step (only an epoch's last step is short)
        epochs_done, rest = divmod(self.global_step, self.steps_per_epoch)
        draws = epochs_done * self.micro_per_epoch + min(rest * self.accumulate, self.micro_per_epoch)
        for s in self._samplers():
            s.rng_state = torch.tensor([s.seed, draws], dtype=torch.int64, device=self.flat._flat.device)
        return ck

    def _newest(self, epoch: int):
        self._save(f"epoch_{epoch}.pt", epoch)
        keep_latest_checkpoints(self.save_path, self.keep_checkpoints)


class RPNTrainer(_BoxTrainer):
    """Epoch loop of run_rpn.py:310-431, 455-591 for NeRFRegionProposalNetwork (the conventions of _FinetuneTrainer): input from data.DetectionBatcher
    (`resolution` from the backbone where it exposes one), loss = loss_objectness + reg_loss_weight * loss_rpn_box_reg + reg_loss_weight_2d *
    loss_rpn_box_reg_2d (:385-387), OneCycle over (schedule_epochs or num_epochs) * steps_per_epoch steps (the reference sizes it by num_epochs, :348-349).

    `train_loss` of the history is the weighted total, the three losses under their own keys are unweighted.  Evaluation: model.eval(), rpn.proposals_dense
    per validation batch into DetectionEvaluator's dense form (no host wait per batch), the limits of [300, 1000, rpn_post_nms_top_n_test] not above the last
    (:533-535), AP at 0.25 and 0.5 over each scene's `top_k` best; record keys as DetectionTrainer's.  `model_best.pt` when recall at 0.5 under the largest limit
    improves (:363-367), `epoch_{n}.pt` at every evaluated epoch, of which the `keep_checkpoints` newest stay.

    freeze_backbone (run_rpn.py:193-195): the backbone is left out of the flat buffers (FlatParameters(exclude=)) and runs without a graph
    (model.backbone_no_grad), in eval(): only model.rpn is stepped and weight-decayed.  The checkpoint carries the backbone regardless (:294-300).

    train_boxes / val_boxes: one [G, 6|7] array per scene."""

    _save_checkpoint, _load_checkpoint = staticmethod(save_rpn_checkpoint), staticmethod(load_rpn_checkpoint)
    KEYS = ("loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d")

    def __init__(self, model, train_scenes, train_boxes, val_scenes=None, val_boxes=None, resolution: int = None, batch_size: int = 1, num_epochs: int = 100,
                 lr: float = 1e-4, weight_decay: float = 0.01, clip_grad_norm: float = 0.1, reg_loss_weight: float = 5.0, reg_loss_weight_2d: float = 0.0,
                 eval_interval: int = 1, keep_checkpoints: int = 1, top_k: int = None, freeze_backbone: bool = False, normalize_density: bool = True,
                 flip_prob: float = 0.0, rotate_prob: float = 0.0, rot_scale_prob: float = 0.0, schedule_epochs: int = None, save_path: str = None, log=print,
                 train_args: dict = None, seed: int = 0, rank: int = 0, world: int = 1, reducer=None, layer_decay: float = None, no_decay: bool = False, freeze=(),
                 accumulate: int = 1, freeze_stages: int = 0):
        from .finetune import rpn_loss_fn
        self.freeze_backbone = bool(freeze_backbone)
        args = dict(train_args or {}, lr=lr, weight_decay=weight_decay, clip_grad_norm=clip_grad_norm, reg_loss_weight=reg_loss_weight,
                    reg_loss_weight_2d=reg_loss_weight_2d, batch_size=batch_size * world, num_epochs=num_epochs, keep_checkpoints=keep_checkpoints, top_k=top_k,
                    freeze_backbone=self.freeze_backbone, normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob,
                    rot_scale_prob=rot_scale_prob)
        self._setup(model, model.backbone, train_scenes, train_boxes, val_scenes, val_boxes, resolution, rpn_loss_fn(model),
                    {"loss_rpn_box_reg": reg_loss_weight, "loss_rpn_box_reg_2d": reg_loss_weight_2d}, self.KEYS,
                    dict(args=args, batch_size=batch_size, num_epochs=num_epochs, schedule_epochs=schedule_epochs, lr=lr, weight_decay=weight_decay,
                         clip_grad_norm=clip_grad_norm, eval_interval=eval_interval, keep_checkpoints=keep_checkpoints, top_k=top_k, save_path=save_path, log=log,
                         seed=seed, rank=rank, world=world, reducer=reducer, normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob,
                         rot_scale_prob=rot_scale_prob, layer_decay=layer_decay, no_decay=no_decay, freeze=freeze, accumulate=accumulate,
                         freeze_stages=freeze_stages),
                    (model.backbone,) if self.freeze_backbone else ())
        if self.freeze_backbone:
            model.backbone_no_grad = True
        self.limits = proposal_limits(model.rpn._post_nms_top_n["testing"])
        self.best_metric = None

    @torch.no_grad()
    def evaluate(self):
        from .det_eval import DetectionEvaluator
        self.model.eval()
        ev = DetectionEvaluator(limits=self.limits, ap_thresholds=(0.25, 0.5), top_k=self.top_k)
        try:
            for meshes, gt, gt_counts in self._val_batches():
                boxes, scores, _, _, counts = self.model.proposals_dense(meshes)
                ev.update(boxes, scores, counts, gt, gt_counts)
        finally:
            self._train_mode()
        out = ev.compute()                                            # the evaluation's one synchronisation
        rec = {}
        for l in self.limits:
            for key in ("25", "50", "ar"):
                rec[f"recall_{key}_top_{l}"] = float(out[f"recall_{key}_top_{l}"]["ar"])
        rec["ap_25"], rec["ap_50"] = float(out["ap_25"]["ap"]), float(out["ap_50"]["ap"])
        return rec

    def _samplers(self):
        return [self.model.rpn.loss]

    def _keep_best(self, epoch: int, rec: dict):
        metric = rec[f"recall_50_top_{self.limits[-1]}"]
        if self.best_metric is None or metric > self.best_metric:
            self.best_metric = metric
            self._save("model_best.pt", epoch)
        self._newest(epoch)


class TwoStageTrainer(_BoxTrainer):
    """Epoch loop of run_rpn_detect.py:279-390, 441-551 for detector.TwoStageDetector (the conventions of _FinetuneTrainer), the two stages joined: the
    proposals come from the detector's own first stage, not from stored files.  loss = loss_objectness + reg_loss_weight * loss_rpn_box_reg of the box head
    (obj_only: the regression term gets weight 0, :359-363), and with model.train_rpn the first stage's losses under their "rpn_" keys, weighted as run_rpn.py
    weights them (rpn_reg_loss_weight, rpn_reg_loss_weight_2d).  OneCycle over (schedule_epochs or num_epochs) * steps_per_epoch steps.

    The mode follows from model.train_rpn and freeze_first_stage (None: not model.train_rpn), see resolve_mode:
      head       train_rpn off, frozen: the reference's default without --fine_tune.  The first stage is left out of the flat buffers and runs without a graph
                 (model.first_stage_no_grad), in eval(); only roi_model is stepped; the checkpoint's "backbone_state_dict" is None.
      joint      train_rpn on: everything trains, the five losses are logged.
      fine_tune  train_rpn off, not frozen: the pooling's gradient trains the backbone under a first-stage head that stays as it is (the detector's behaviour
                 without a trainer; its proposals follow the moving features with nothing holding them, so choose it knowingly).
      heads      train_rpn on, frozen: the backbone alone is frozen; both heads train on its detached features.

    Evaluation: detections_dense per validation batch into DetectionEvaluator(ap_thresholds=(0.25, 0.5), top_k) -> ap_25, ap_50.  `model_best_ap25.pt` /
    `model_best_ap50.pt` whenever that AP improves, `epoch_{n}.pt` at every evaluated epoch, of which the `keep_checkpoints` newest stay (:327-340).  Stated
    deviations: the first evaluation writes both best files (the reference's only initialises its best values); epochs count from 1, as in the other trainers.
    init_from_rpn(path) loads an RPNTrainer's (or the reference's run_rpn.py) checkpoint into the first stage: the hand-over the reference does on disk."""

    _load_checkpoint = staticmethod(load_two_stage_checkpoint)

    @staticmethod
    def resolve_mode(train_rpn: bool, freeze_first_stage=None):
        """-> (mode, frozen): mode in "head" | "joint" | "fine_tune" | "heads"; frozen: "first_stage", "backbone" or None"""
        train_rpn = bool(train_rpn)
        freeze = (not train_rpn) if freeze_first_stage is None else bool(freeze_first_stage)
        if train_rpn:
            return ("heads", "backbone") if freeze else ("joint", None)
        return ("head", "first_stage") if freeze else ("fine_tune", None)

    def __init__(self, model, train_scenes, train_boxes, val_scenes=None, val_boxes=None, resolution: int = None, batch_size: int = 2, num_epochs: int = 100,
                 lr: float = 1e-4, weight_decay: float = 5e-4, clip_grad_norm: float = 0.1, reg_loss_weight: float = 5.0, rpn_reg_loss_weight: float = 5.0,
                 rpn_reg_loss_weight_2d: float = 0.0, obj_only: bool = False, freeze_first_stage: bool = None, eval_interval: int = 1, keep_checkpoints: int = 1,
                 top_k: int = None, normalize_density: bool = True, flip_prob: float = 0.0, rotate_prob: float = 0.0, rot_scale_prob: float = 0.0,
                 schedule_epochs: int = None, save_path: str = None, log=print, train_args: dict = None, seed: int = 0, rank: int = 0, world: int = 1, reducer=None,
                 layer_decay: float = None, no_decay: bool = False, freeze=(), accumulate: int = 1, freeze_stages: int = 0):
        from .finetune import roi_loss_fn
        if obj_only and model.is_reg:
            raise ValueError("TwoStageTrainer: obj_only trains no box regression, but the detector decodes with it (is_reg=True): build TwoStageDetector(..., "
                             "is_reg=False), whose detections are the proposals themselves")
        self.mode, frozen = self.resolve_mode(model.train_rpn, freeze_first_stage)
        self.frozen = frozen
        self.obj_only = bool(obj_only)
        exclude = {"first_stage": (model.rpn_network,), "backbone": (model.rpn_network.backbone,), None: ()}[frozen]
        weights = {"loss_rpn_box_reg": 0.0 if obj_only else reg_loss_weight}
        keys = ("loss_objectness", "loss_rpn_box_reg")
        if model.train_rpn:
            weights.update({"rpn_loss_rpn_box_reg": rpn_reg_loss_weight, "rpn_loss_rpn_box_reg_2d": rpn_reg_loss_weight_2d})
            keys += ("rpn_loss_objectness", "rpn_loss_rpn_box_reg", "rpn_loss_rpn_box_reg_2d")
        args = dict(train_args or {}, lr=lr, weight_decay=weight_decay, clip_grad_norm=clip_grad_norm, reg_loss_weight=reg_loss_weight,
                    rpn_reg_loss_weight=rpn_reg_loss_weight, rpn_reg_loss_weight_2d=rpn_reg_loss_weight_2d, obj_only=self.obj_only, mode=self.mode,
                    fine_tune=self.mode != "head", batch_size=batch_size * world, num_epochs=num_epochs, keep_checkpoints=keep_checkpoints, top_k=top_k,
                    normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob, rot_scale_prob=rot_scale_prob)
        self._setup(model, model.rpn_network.backbone, train_scenes, train_boxes, val_scenes, val_boxes, resolution, roi_loss_fn(model), weights, keys,
                    dict(args=args, batch_size=batch_size, num_epochs=num_epochs, schedule_epochs=schedule_epochs, lr=lr, weight_decay=weight_decay,
                         clip_grad_norm=clip_grad_norm, eval_interval=eval_interval, keep_checkpoints=keep_checkpoints, top_k=top_k, save_path=save_path, log=log,
                         seed=seed, rank=rank, world=world, reducer=reducer, normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob,
                         rot_scale_prob=rot_scale_prob, layer_decay=layer_decay, no_decay=no_decay, freeze=freeze, accumulate=accumulate,
                         freeze_stages=freeze_stages),
                    exclude)
        model.first_stage_no_grad = frozen is not None
        self.best_metric = {}

    def _save_checkpoint(self, path, model, epoch, train_args, opt=None, step=None):
        save_two_stage_checkpoint(path, model, epoch, train_args, opt, step, fine_tune=self.mode != "head")

    def init_from_rpn(self, path: str, backbone_only: bool = False) -> dict:
        """the first stage from a save_rpn_checkpoint file (or the reference's run_rpn.py checkpoint): backbone and RPN head, strictly; the parameters keep their
        storage, so the flat buffers stay valid"""
        ck = load_rpn_checkpoint(path, self.model.rpn_network, backbone_only=backbone_only)
        self.flat.check()
        return ck

    @torch.no_grad()
    def evaluate(self):
        from .det_eval import DetectionEvaluator
        self.model.eval()
        ev = DetectionEvaluator(limits=(None,), ap_thresholds=(0.25, 0.5), top_k=self.top_k)
        try:
            for meshes, gt, gt_counts in self._val_batches():
                boxes, scores, counts = self.model.detections_dense(meshes)
                ev.update(boxes, scores, counts, gt, gt_counts)
        finally:
            self._train_mode()
        out = ev.compute()                                            # the evaluation's one synchronisation
        return {"ap_25": float(out["ap_25"]["ap"]), "ap_50": float(out["ap_50"]["ap"])}

    def _samplers(self):
        return [self.model.roi_model.sample_model] + ([self.model.rpn_network.rpn.loss] if self.model.train_rpn else [])

    def _keep_best(self, epoch: int, rec: dict):
        for name in ("25", "50"):
            ap = rec[f"ap_{name}"]
            if name not in self.best_metric or ap > self.best_metric[name]:
                self.best_metric[name] = ap
                self._save(f"model_best_ap{name}.pt", epoch)
        self._newest(epoch)


# --------------------------------------------------------------------------------------------------
# Voxel heads: the reference's checkpoint format and the epoch loops of run_voxelSR.py / run_voxel_semantics.py
# --------------------------------------------------------------------------------------------------
def save_voxel_checkpoint(path: str, model, epoch: int, train_args: dict, opt: "FusedAdamW" = None, step: int = None):
    """the voxel runs' checkpoint (run_voxel_semantics.py:509-527, run_voxelSR.py:494-512): {"epoch", "state_dict", "train_args"} of a voxel head, keys and
    shapes the reference's.  With `opt` (a FusedAdamW over a finetune.FlatParameters of this model) the file also carries the "resume" section of
    save_checkpoint."""
    _write_checkpoint(path, {"state_dict": _unwrapped(model).state_dict()}, epoch, _plain(dict(train_args)), opt, step)


def load_voxel_checkpoint(path: str, model, opt: "FusedAdamW" = None) -> dict:
    """loads a voxel-head checkpoint (also one written by the reference) strictly; returns the checkpoint dict.  With `opt` and a "resume" section the optimizer
    continues where it stopped; a file without the section loads the weights only."""
    return _read_checkpoint(path, [("state_dict", _unwrapped(model), True)], opt, "load_voxel_checkpoint")


class VoxelTrainer(_FinetuneTrainer):
    """Epoch loops of run_voxel_semantics.py:537-958 and run_voxelSR.py:600-790 for the two heads of heads.py (the conventions of _FinetuneTrainer): input from
    data.VoxelBatcher (scene and target under one augmentation draw, the target never a host fp32 batch), OneCycle sized by `num_epochs` (`schedule_epochs`
    overrides; the reference: total_steps = num_epochs * len(train_loader)).  The head decides the rest:

      semantics   train_targets: one label volume per scene ((W,L,H) or (1,W,L,H), uint8 / int32 / int64 / float32).  History: train_loss, train_iou (the loss's
                  mean soft IoU, its second output, outside the backward), and from SemanticEvaluator mIoU, mAcc, allAcc; best by mIoU.
      SR          train_targets: one stored high-resolution scene (W',L',H',4) per scene, padded to int(R * final_upsample.scale_factor).  History: train_loss,
                  and from heads.SREvaluator psnr, mse (the means of the per-batch values); best by psnr.

    Evaluation with flags 0; `model_best.pt` = {"epoch", "state_dict", "train_args"} plus the resume section (save_voxel_checkpoint).

    Augmentation: flip_prob / rotate_prob > 0 apply ONE draw to scene and target, which the reference cannot do (see data.VoxelBatcher); rot_scale_prob is a
    trilinear blend without meaning for labels and must be 0."""

    _save_checkpoint, _load_checkpoint = staticmethod(save_voxel_checkpoint), staticmethod(load_voxel_checkpoint)

    def __init__(self, model, train_scenes, train_targets, val_scenes=None, val_targets=None, batch_size: int = 1, num_epochs: int = 1, lr: float = 5e-3,
                 weight_decay: float = 0.01, clip_grad_norm: float = 0.1, eval_interval: int = 1, save_path: str = None, normalize_density: bool = True,
                 flip_prob: float = 0.0, rotate_prob: float = 0.0, rot_scale_prob: float = 0.0, schedule_epochs: int = None, log=print,
                 train_args: dict = None, seed: int = 0, rank: int = 0, world: int = 1, reducer=None, layer_decay: float = None, no_decay: bool = False, freeze=(),
                 accumulate: int = 1, freeze_stages: int = 0):
        from . import data
        from .heads import SwinTransformer_VoxelSemantics_Pretrained_Skip, SwinTransformer_VoxelSR_Pretrained_Skip
        if isinstance(model, SwinTransformer_VoxelSemantics_Pretrained_Skip):
            self.kind, self.best_key = "semantics", "mIoU"
        elif isinstance(model, SwinTransformer_VoxelSR_Pretrained_Skip):
            self.kind, self.best_key = "sr", "psnr"
        else:
            raise TypeError(f"VoxelTrainer: {type(model).__name__} is neither voxel head (SwinTransformer_VoxelSR_Pretrained_Skip, "
                            "SwinTransformer_VoxelSemantics_Pretrained_Skip); the detectors train with DetectionTrainer")
        if rot_scale_prob != 0:
            raise ValueError("VoxelTrainer: rot_scale_prob must be 0: the small rotation + scaling is a trilinear blend, which has no meaning for a label volume")
        if len(train_scenes) != len(train_targets) or (val_scenes is not None and len(val_scenes) != len(val_targets or [])):
            raise ValueError("VoxelTrainer: one target per scene")
        if len(train_scenes) < 1:
            raise ValueError("VoxelTrainer: no training scene")
        dev = next(model.parameters()).device
        R = model.input_resolution
        kw = dict(target="labels") if self.kind == "semantics" else dict(target="grid", target_resolution=int(R * float(model.final_upsample.scale_factor)))
        self._aux = None                                     # the semantics loss's mean soft IoU of the step: logged, never part of the backward
        super().__init__(model, train_scenes, train_targets, val_scenes, val_targets,
                         data.VoxelBatcher(R, dev, normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob, **kw),
                         data.VoxelBatcher(R, dev, normalize_density=normalize_density, **kw), self._loss, None,
                         dict(train_args or {}, lr=lr, weight_decay=weight_decay, clip_grad_norm=clip_grad_norm, batch_size=batch_size * world,
                              num_epochs=num_epochs, normalize_density=normalize_density, flip_prob=flip_prob, rotate_prob=rotate_prob,
                              rot_scale_prob=rot_scale_prob),
                         batch_size, num_epochs, schedule_epochs or num_epochs, lr, weight_decay, clip_grad_norm, eval_interval, save_path, log, seed, rank, world,
                         reducer, layer_decay=layer_decay, no_decay=no_decay, freeze=freeze, accumulate=accumulate, freeze_stages=freeze_stages)
        self.best_metric = None

    def _loss(self, meshes, tb):
        out = self.model.loss_fn(tb, self.model(meshes))
        if self.kind == "semantics":
            self._aux = out[2].detach()
            return {"loss": out[0]}
        return {"loss": out}

    def _target(self, t):
        """a stored target by path: the scene file's `rgbsigma` for the SR head; label volumes are passed as arrays"""
        return self._load(t) if self.kind == "sr" else t

    def _logged(self, losses):
        return torch.stack([losses["loss"], self._aux]) if self.kind == "semantics" else losses["loss"].reshape(1)

    def _record(self, vals):
        return dict(zip(("train_loss", "train_iou"), vals))

    @torch.no_grad()
    def evaluate(self):
        from .heads import SREvaluator
        from .sem_eval import SemanticEvaluator
        self.model.eval()
        ev = SemanticEvaluator(self.model.out_channels, self.model.class_weights) if self.kind == "semantics" else SREvaluator(self.model)
        try:
            for b in range(0, len(self.val_scenes), self.batch):
                scenes = [self._load(s) for s in self.val_scenes[b:b + self.batch]]
                xb, ext, tb = self.val_batcher.prepare(scenes, [self._target(t) for t in self.val_targets[b:b + self.batch]], flags=[0] * len(scenes))
                ev.update(tb, self.model(self._meshes(xb, ext)))
        finally:
            self.model.train()
        out = ev.compute()                                            # the evaluation's one synchronisation
        if self.kind == "semantics":
            return {k: float(out[k]) for k in ("mIoU", "mAcc", "allAcc")}
        return {"psnr": float(out["psnr_mean"]), "mse": float(out["mse_mean"])}

    def _keep_best(self, epoch: int, rec: dict):
        if self.best_metric is None or rec[self.best_key] > self.best_metric:
            self.best_metric = rec[self.best_key]
            self._save("model_best.pt", epoch)
