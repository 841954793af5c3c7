"""Fine-tuning of the downstream models (the detectors, the voxel heads) with the fused optimizer of the MAE path.

  FlatParameters   one flat fp32 parameter buffer and one flat gradient buffer over ANY module of this package: the trainable parameters of its
                   SwinTransformer_MAE3D_New (`base` of the FPN backbone or of a voxel head) first, in base._trainable() order and filling the base's own flat
                   buffers in place, then every other trainable parameter in named_parameters() order, each on an 8-element granule.  It has the attributes
                   FusedAdamW, trainer.flat_layout and the checkpoint functions read (_flat, _flat_grad, _offsets, flatten_parameters, named_parameters,
                   state_dict), so those work on it unchanged.  exclude=(sub-modules) leaves a frozen part out of the buffers altogether.
  FinetuneStep     one eager step: check the views, forward, backward, clip + AdamW (three launches; the update clears the gradient buffer).
  fcos_loss_fn, rpn_loss_fn, voxel_loss_fn, loss_fn_for   the loss functions FinetuneStep takes, for the four downstream models.
  param_ranges     per-range optimizer settings over the flat layout, from ordered rules: the table FusedAdamW(ranges=) steps with.
  layer_decay_rules, no_decay_rules, freeze_rules, recipe_rules   the rules of the usual fine-tuning recipe.
  frozen_stage_rules   the frozen prefix of the encoder (patch embed + stages[:k]): its freeze rules, and the encoder told to end the backward there.

No kernel of its own: forward and backward are the models', the optimizer is nmh_grad_sqnorm / nmh_clip_coef / nmh_adamw_step (trainer.FusedAdamW), or their
*_ranges forms under a table.

Ordering of the gradient producers before the optimizer reads the buffer: every Function of this package that forks the side stream joins it
before its backward returns, and the base's deferred weight gradients are issued and joined by _EmbedFn.backward and by the end-of-backward callback of its
queue, so `loss.backward()` returns with every gradient launch ordered before whatever the calling stream is given next.  The step adds no join.

Eager.  Data-parallel with a dist.FlatGradReducer (FinetuneStep(..., reducer=)): the gradient ranges are exchanged from autograd triggers and by finish().
A graph capture of the detectors needs padded target lists first and is left out."""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import torch
from torch import nn

from .model import SwinTransformer_MAE3D_New

__all__ = ["FlatParameters", "FinetuneStep", "fcos_loss_fn", "rpn_loss_fn", "voxel_loss_fn", "loss_fn_for", "ParamRanges", "param_ranges", "layer_ids",
           "layer_decay_rules", "no_decay_rules", "freeze_rules", "frozen_stage_rules", "recipe_rules"]


def _round8(n: int) -> int:
    return (n + 7) // 8 * 8


def _same_device(a: torch.device, b: torch.device) -> bool:
    if a.type != b.type:
        return False
    if a.type != "cuda":
        return True
    cur = torch.cuda.current_device() if (a.index is None or b.index is None) else 0
    return (cur if a.index is None else a.index) == (cur if b.index is None else b.index)


class FlatParameters:
    """FlatParameters(module, device=None, exclude=()): re-homes every trainable parameter of `module` and its .grad as views of one flat fp32 buffer pair.

    Layout: [base._trainable() on 8-element granules = base._flat | the other trainable parameters in named_parameters() order, 8-element granules]; a parameter
    object registered under two names is placed once.  Frozen parameters (pos_embed) and buffers stay where they are.  The module must already be on the device
    it trains on: `device` only states what the caller expects and is refused when the parameters live elsewhere (moving the parameters alone would leave the
    frozen ones and the buffers behind).  Refused as well: more than one SwinTransformer_MAE3D_New, and one without a trainable parameter.

    exclude: sub-modules of `module` that are left out (a frozen first stage).  Their parameters stay where they are: no view, no gradient
    view, no offset, so neither the optimizer nor a reducer over this object touches them, and they are not searched for a SwinTransformer_MAE3D_New -- an
    excluded encoder runs from the flat buffer it makes for itself (model._ensure_ready), as it does without a FlatParameters.  Names stay those of
    module.named_parameters().  With exclude=() the layout is the one described above.  Refused: an entry that is not a sub-module of `module`, and an
    exclusion that leaves no trainable parameter.

    The modules outside model.py rebuild their packed weights when a parameter's storage moves (conv_layer.ensure_packed keys on data_ptr()), and the base's
    _ensure_ready finds its parameters where its own _offsets say, so nothing re-flattens afterwards.  `check()` verifies exactly that before every step."""

    def __init__(self, module: nn.Module, device=None, exclude=()):
        self.module = module
        self.exclude = tuple(exclude)
        self._flat = self._flat_grad = None
        self._offsets: Dict[int, int] = {}
        self._views = []
        self.base: Optional[SwinTransformer_MAE3D_New] = None
        self.flatten_parameters(device)

    # ---- layout -----------------------------------------------------------------------------------------------------------------------------
    def flatten_parameters(self, device=None):
        module = self.module
        inside = {id(m) for m in module.modules()}
        for e in self.exclude:
            if not isinstance(e, nn.Module) or id(e) not in inside:
                raise ValueError(f"FlatParameters: exclude takes sub-modules of the module; {type(e).__name__} is not one of {type(module).__name__}'s")
        out_mods = {id(m) for e in self.exclude for m in e.modules()}
        out_params = {id(p) for e in self.exclude for p in e.parameters()}
        bases = [m for m in module.modules() if isinstance(m, SwinTransformer_MAE3D_New) and id(m) not in out_mods]
        if len(bases) > 1:
            raise ValueError(f"FlatParameters: the module holds {len(bases)} SwinTransformer_MAE3D_New; one flat buffer can lead with the parameters of one only")
        base = bases[0] if bases else None
        lead = base._trainable() if base is not None else []
        if base is not None and not lead:
            raise ValueError("FlatParameters: the module's SwinTransformer_MAE3D_New has no trainable parameter (a frozen encoder is not supported: it keeps no "
                             "flat buffer of its own to run from)")
        if any(id(p) in out_params for p in lead):
            raise ValueError("FlatParameters: exclude the SwinTransformer_MAE3D_New as a whole (or a module around it), not a part of it: its flat buffer is "
                             "one piece")
        seen = {id(p) for p in lead} | out_params
        rest = []
        for name, p in module.named_parameters():
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                rest.append(p)
        if not lead and not rest:
            raise ValueError("FlatParameters: the exclusion leaves no trainable parameter" if self.exclude else "FlatParameters: the module has no trainable parameter")
        everything = list(module.parameters()) + list(module.buffers())
        where = (lead + rest)[0].device
        stray = [t for t in everything if not _same_device(t.device, where)]
        if stray:
            raise RuntimeError(f"FlatParameters: the module's parameters and buffers are spread over {where} and {stray[0].device}; move the module first")
        if device is not None and not _same_device(torch.device(device), where):
            raise RuntimeError(f"FlatParameters: the parameters are on {where}, not on {torch.device(device)}: move the module first (.cuda() / .to()); the flat "
                               "buffers are made where the parameters are")
        if any(p.dtype != torch.float32 for p in lead + rest):
            raise TypeError("FlatParameters: fp32 master parameters only")
        nb = base.flat_numel() if base is not None else 0
        n = nb + sum(_round8(p.numel()) for p in rest)
        flat, fg = torch.zeros(n, device=where), torch.zeros(n, device=where)
        offsets: Dict[int, int] = {}
        if base is not None:
            base.flatten_parameters(out=(flat[:nb], fg[:nb]))
            offsets.update(base._offsets)
        off = nb
        with torch.no_grad():
            for p in rest:
                k = p.numel()
                flat[off:off + k].copy_(p.data.reshape(-1))
                p.data = flat[off:off + k].view(p.shape)
                p.grad = fg[off:off + k].view(p.shape)
                offsets[id(p)] = off
                off += _round8(k)
        self.base, self._flat, self._flat_grad, self._offsets = base, flat, fg, offsets
        self._views = [(name, p, offsets[id(p)]) for name, p in module.named_parameters() if id(p) in offsets]
        return flat, fg

    # ---- what FusedAdamW, flat_layout and the checkpoint functions read ------------------------------------------------------------------------
    def named_parameters(self, *args, **kwargs):
        return self.module.named_parameters(*args, **kwargs)

    def state_dict(self, *args, **kwargs):
        return self.module.state_dict(*args, **kwargs)

    def zero_grad(self):
        self._flat_grad.zero_()

    def check(self):
        """every trainable parameter's .data and .grad must still be the view it was given (compared by pointer); raises RuntimeError naming the first that is
        not.  What breaks it: nn.Module.zero_grad() with torch's default set_to_none=True (use zero_grad() of this object), .cuda() / .to() / .float() after
        flattening, a base that re-flattened itself.  Without this the optimizer would update memory nothing reads."""
        p0, g0 = self._flat.data_ptr(), self._flat_grad.data_ptr()
        for name, p, off in self._views:
            if p.data_ptr() != p0 + 4 * off:
                raise RuntimeError(f"FlatParameters.check: parameter '{name}' no longer lives in the flat buffer (moved by .cuda() / .to(), its .data replaced, or "
                                   "its SwinTransformer_MAE3D_New flattened itself again); build a new FlatParameters and optimizer")
            g = p.grad
            if g is None or g.data_ptr() != g0 + 4 * off:
                raise RuntimeError(f"FlatParameters.check: the .grad of parameter '{name}' is no longer its view of the flat gradient buffer "
                                   f"({'None: zero_grad(set_to_none=True)?' if g is None else 'replaced'}); clear gradients with FlatParameters.zero_grad()")
        b = self.base
        if b is not None and (b._flat is None or b._flat.data_ptr() != p0 or b._flat_grad.data_ptr() != g0):
            raise RuntimeError("FlatParameters.check: the SwinTransformer_MAE3D_New flattened itself again; build a new FlatParameters and optimizer")


# ---- per-range optimizer settings over the flat layout -------------------------------------------------------------------------
class ParamRanges(NamedTuple):
    """what param_ranges returns and FusedAdamW(ranges=) takes: the device table of nmh_adamw_step_ranges and its host record"""
    bounds: torch.Tensor    # int64 [R+1] on the flat buffer's device
    scale: torch.Tensor     # float32 [R, 2] = (lr_scale, wd_scale)
    record: dict            # {"bounds": [int] * (R+1), "scale": [[lr_scale, wd_scale]] * R}: plain numbers, what a checkpoint's resume section stores


def _selector(sel) -> Callable:
    """a rule's selector -> predicate(name, param): a name prefix, a callable (name, param) -> bool, or a sub-module (its parameters)"""
    if isinstance(sel, str):
        return lambda name, p: name.startswith(sel)
    if isinstance(sel, nn.Module):
        ids = {id(p) for p in sel.parameters()}
        return lambda name, p: id(p) in ids
    if callable(sel):
        return sel
    raise TypeError(f"param_ranges: a selector is a name prefix, a callable (name, param) -> bool or a sub-module, not {type(sel).__name__}")


def _selector_text(sel) -> str:
    return repr(sel) if isinstance(sel, str) else f"{type(sel).__name__} (sub-module)" if isinstance(sel, nn.Module) else getattr(sel, "__name__", repr(sel))


def param_ranges(flat, rules) -> ParamRanges:
    """param_ranges(flat, rules): the per-range table of trainer.FusedAdamW(ranges=) over the flat layout of `flat`, an MAE model or a FlatParameters (anything
    trainer.flat_layout takes).

    rules: an ordered list of (selector, lr_scale, wd_scale).  For every parameter of the flat buffer, each of the two scales comes from the FIRST rule that
    matches the parameter and states that scale; None in a rule leaves the scale to a later rule, and a scale no rule states is 1.  lr_scale 0 freezes the
    parameter (no update, no moments, outside the clip norm: DESIGN.md 3.25).  A parameter's range runs up to the next parameter's offset, so the granule padding
    behind it joins it; adjacent parameters with equal scales share one range.
    Refused (ValueError): a negative or non-finite scale; a rule that matches no parameter of the flat buffer (a typo must not silently train everything; a
    parameter that FlatParameters(exclude=) left out is not there to be selected); more ranges than ops.ADAMW_MAX_RANGES."""
    import math
    from . import ops
    if flat._flat is None:
        flat.flatten_parameters()
    n = int(flat._flat.numel())
    params = sorted(((int(flat._offsets[id(p)]), name, p) for name, p in flat.named_parameters() if id(p) in flat._offsets), key=lambda t: t[0])
    if not params or params[0][0] != 0:
        raise ValueError("param_ranges: the flat layout does not start at offset 0")
    compiled = []
    for k, rule in enumerate(rules):
        if not isinstance(rule, (tuple, list)) or len(rule) != 3:
            raise TypeError(f"param_ranges: rule {k} is not (selector, lr_scale, wd_scale)")
        sel, ls, ws = rule
        for what, s in (("lr_scale", ls), ("wd_scale", ws)):
            if s is not None and not (math.isfinite(float(s)) and float(s) >= 0.0):
                raise ValueError(f"param_ranges: rule {k} ({_selector_text(sel)}): {what} = {s}; a scale is finite and >= 0")
        compiled.append((_selector(sel), None if ls is None else float(ls), None if ws is None else float(ws)))
    matched = [False] * len(compiled)
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731  (the value the device table holds: the record compares equal after a round trip)
    bounds, scale = [], []
    for off, name, p in params:
        ls = ws = None
        for k, (pred, rl, rw) in enumerate(compiled):
            if (ls is not None and ws is not None) or not pred(name, p):
                continue
            matched[k] = True
            ls, ws = rl if ls is None else ls, rw if ws is None else ws
        s = [f32(1.0 if ls is None else ls), f32(1.0 if ws is None else ws)]
        if not scale or scale[-1] != s:
            bounds.append(off)
            scale.append(s)
    for k, hit in enumerate(matched):
        if not hit:
            raise ValueError(f"param_ranges: rule {k} ({_selector_text(rules[k][0])}) matches no parameter of the flat buffer")
    bounds.append(n)
    if len(scale) > ops.ADAMW_MAX_RANGES:
        raise ValueError(f"param_ranges: {len(scale)} ranges, the kernels take {ops.ADAMW_MAX_RANGES}")
    dev = flat._flat.device
    return ParamRanges(torch.tensor(bounds, dtype=torch.int64).to(dev), torch.tensor(scale, dtype=torch.float32).reshape(-1, 2).to(dev),
                       {"bounds": bounds, "scale": scale})


def _encoder_of(module, who: str) -> SwinTransformer_MAE3D_New:
    """the one SwinTransformer_MAE3D_New inside `module` (a module or a FlatParameters), found by identity as FlatParameters finds it"""
    module = module.module if isinstance(module, FlatParameters) else module
    bases = [m for m in module.modules() if isinstance(m, SwinTransformer_MAE3D_New)]
    if len(bases) != 1:
        raise ValueError(f"{who}: the module holds {len(bases)} SwinTransformer_MAE3D_New, it takes exactly one")
    return bases[0]


def layer_ids(module) -> Dict[int, int]:
    """{id(parameter): layer id} of the encoder's parameters for layer-wise learning-rate decay, L = the number of Swin blocks: patch_partition and mask_token 0;
    the k-th block over all stages (0-based) k + 1; a stage's PatchMerging3D the id of that stage's first block.  Every parameter that is not listed (decoders,
    out, neck, heads) has id L + 1."""
    from .model import PatchMerging3D, SwinBlock3D
    base = _encoder_of(module, "layer_ids")
    ids = {id(p): 0 for p in base.patch_partition.parameters()}
    if "mask_token" in base._parameters:       # (the downstream backbones drop it)
        ids[id(base.mask_token)] = 0
    k = 0
    for stage in base.stages:
        merges = [m for m in stage if isinstance(m, PatchMerging3D)]
        first = k + 1
        for m in stage:
            if isinstance(m, SwinBlock3D):
                k += 1
                ids.update({id(p): k for p in m.parameters()})
        for m in merges:
            ids.update({id(p): first for p in m.parameters()})
    return ids


def layer_decay_rules(module, decay: float):
    """rules of layer-wise learning-rate decay over the encoder of `module`: lr_scale = decay ** (L + 1 - id) with the ids of layer_ids, one rule per id; what
    lies after the encoder (id L + 1) keeps scale 1 and needs no rule.  Refused: a module without exactly one SwinTransformer_MAE3D_New."""
    from .model import SwinBlock3D
    base = _encoder_of(module, "layer_decay_rules")
    if not float(decay) > 0.0:
        raise ValueError(f"layer_decay_rules: decay = {decay}; it is positive (freeze_rules freezes)")
    ids = layer_ids(base)
    L = sum(isinstance(m, SwinBlock3D) for st in base.stages for m in st)
    rules = []
    for layer in sorted(set(ids.values())):
        members = {i for i, l in ids.items() if l == layer}

        def pred(name, p, members=members):
            return id(p) in members
        pred.__name__ = f"layer {layer}"
        rules.append((pred, float(decay) ** (L + 1 - layer), None))
    return rules


def no_decay_rules(module):
    """one rule, wd_scale 0, for every parameter with dim() <= 1 (norms, biases), the relative-position bias tables, mask_token and the parameters of fcos.Scale"""
    from .fcos import Scale
    module = module.module if isinstance(module, FlatParameters) else module
    special = {id(p) for m in module.modules() if isinstance(m, Scale) for p in m.parameters()}
    special |= {id(p) for name, p in module.named_parameters() if name.endswith("relative_position_bias_table") or name.split(".")[-1] == "mask_token"}

    def no_decay(name, p):
        return p.dim() <= 1 or id(p) in special
    return [(no_decay, None, 0.0)]


def freeze_rules(*selectors):
    """lr_scale 0 for what each selector matches: those parameters, and their moments, are not written by the step"""
    return [(s, 0.0, None) for s in selectors]


def frozen_stage_rules(module, k: int):
    """the frozen prefix of the one encoder inside `module` (a module or a FlatParameters): sets encoder.frozen_stages = k -- the patch embed and stages[:k] then
    run without a graph, no backward kernel runs for them, none of their activations is kept and no reducer exchanges their ranges -- and returns
    the freeze rules of exactly those parameters: patch_partition, mask_token where the encoder has one, stages[0] .. stages[k-1].  The two belong together: a
    prefix that is not stepped-as-frozen would still decay under its zero gradient.  The table equals the one of freeze=(patch_partition, *stages[:k]) (plus
    mask_token).  k = 0: no prefix, no rule.  Refused (ValueError): k outside 0 .. len(stages), a module without exactly one SwinTransformer_MAE3D_New."""
    base = _encoder_of(module, "frozen_stage_rules")
    base.frozen_stages = k          # (the setter checks the range)
    if not base.frozen_stages:
        return []
    sels = [base.patch_partition]
    if "mask_token" in base._parameters:       # (the downstream backbones drop it)
        token = base.mask_token

        def mask_token(name, p):
            return p is token
        sels.append(mask_token)
    return freeze_rules(*sels, *base.stages[:base.frozen_stages])


def _selectors(freeze) -> tuple:
    return (freeze,) if isinstance(freeze, (str, nn.Module)) or callable(freeze) else tuple(freeze)


def selector_names(module, freeze) -> list:
    """the trainers' `freeze` as a checkpoint's train_args record it: a prefix as it is, a sub-module by its name inside `module`, a callable by its __name__"""
    names = {id(m): n for n, m in module.named_modules()}
    return [s if isinstance(s, str) else names.get(id(s), type(s).__name__) if isinstance(s, nn.Module) else getattr(s, "__name__", repr(s)) for s in _selectors(freeze)]


def recipe_rules(module, layer_decay: float = None, no_decay: bool = False, freeze=(), freeze_stages: int = 0):
    """the trainers' switches as one rule list: freeze and the frozen prefix first (they win the lr_scale), then layer decay, then the no-decay set.  freeze_stages
    != 0 also sets the encoder's frozen_stages (frozen_stage_rules); 0 leaves the encoder as it is"""
    freeze = _selectors(freeze)
    return (freeze_rules(*freeze) + (frozen_stage_rules(module, freeze_stages) if freeze_stages else [])
            + (layer_decay_rules(module, layer_decay) if layer_decay is not None else []) + (no_decay_rules(module) if no_decay else []))


# ---- loss functions of the five downstream models ----------------------------------------------------------------------------------------------
def fcos_loss_fn(model) -> Callable:
    """FCOSOverNeRF: (meshes, targets) -> {"loss_cls", "loss_reg", "loss_centerness"}"""
    return lambda meshes, targets: model(list(meshes), targets)[1]


def rpn_loss_fn(model) -> Callable:
    """NeRFRegionProposalNetwork: (meshes, targets) -> {"loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d"}"""
    return lambda meshes, targets: model(list(meshes), targets)[1]


def roi_loss_fn(model) -> Callable:
    """detector.TwoStageDetector: (meshes, targets) -> {"loss_objectness", "loss_rpn_box_reg"} of the second stage (and the first stage's under "rpn_" keys with
    train_rpn); weights={"loss_rpn_box_reg": reg_loss_weight} reproduces run_rpn_detect.py:359-363"""
    return lambda meshes, targets, *sampler: model(list(meshes), targets, *sampler)


def voxel_loss_fn(model) -> Callable:
    """the voxel heads: (grids, target grids) -> {"loss": model.loss_fn(targets, model(grids))} (the first entry where loss_fn returns a tuple)"""

    def fn(x, t):
        out = model.loss_fn(t, model(x))
        return {"loss": out[0] if isinstance(out, (tuple, list)) else out}

    return fn


def loss_fn_for(model) -> Callable:
    from .detector import TwoStageDetector
    from .fcos import FCOSOverNeRF
    from .heads import _VoxelHeadBase
    from .rpn import NeRFRegionProposalNetwork
    if isinstance(model, FCOSOverNeRF):
        return fcos_loss_fn(model)
    if isinstance(model, NeRFRegionProposalNetwork):
        return rpn_loss_fn(model)
    if isinstance(model, TwoStageDetector):
        return roi_loss_fn(model)
    if isinstance(model, _VoxelHeadBase):
        return voxel_loss_fn(model)
    raise TypeError(f"loss_fn_for: no ready-made loss function for {type(model).__name__}; pass your own to FinetuneStep")


class FinetuneStep:
    """FinetuneStep(flat_params, opt, loss_fn, weights=None, reducer=None): one eager fine-tuning step.

    loss_fn(*batch) -> a tensor or a dict of tensors; the total of a dict is sum(weights.get(k, 1.0) * losses[k]) (the reference's `losses["loss_reg"] *=
    reg_loss_weight; loss = cls + reg + centerness`, run_fcos_pretrained.py:729-731, is weights={"loss_reg": w}).  __call__(*batch): check(), forward, backward,
    the optimizer's three launches.  The AdamW kernel clears the gradient buffer (opt.zero_grads_after_step), so no step starts with a zero fill; the buffer is
    cleared once here.  Returns the UNWEIGHTED losses as detached device tensors (a bare tensor under the key "loss"); nothing waits for the host.
    Set the step's learning rate and beta1 with opt.set_hyper() before the call.
    Gradient accumulation: accumulate(*batch) for all micro-batches of a step but the last, then __call__ with the last.

    reducer: a dist.FlatGradReducer over the same FlatParameters.  When it is active (more than one rank, or NMH_DP_FORCE=1) the base gets it as its _reducer,
    so the forward places the segment triggers, and reducer.finish() runs between backward and the update: every rank then steps on the mean gradient.  With
    None or an inactive reducer the step issues exactly the launches it issues without one."""

    def __init__(self, flat_params: FlatParameters, opt, loss_fn: Callable, weights: Optional[Dict[str, float]] = None, reducer=None):
        if not flat_params._flat.is_cuda:
            raise RuntimeError("FinetuneStep needs the parameters on a HIP device: call .cuda() on the module before FlatParameters (no CPU fallback)")
        if opt.model is not flat_params:
            raise ValueError("FinetuneStep: the optimizer must have been built over the same FlatParameters (FusedAdamW(flat_params, ...))")
        if reducer is not None and reducer.model is not flat_params:
            raise ValueError("FinetuneStep: the reducer must have been built over the same FlatParameters (dist.FlatGradReducer(flat_params, ...))")
        self.flat, self.opt, self.loss_fn, self.weights = flat_params, opt, loss_fn, dict(weights or {})
        self.reducer = reducer if (reducer is not None and reducer.active) else None
        if self.reducer is not None and flat_params.base is not None:
            flat_params.base._reducer = self.reducer
        opt.zero_grads_after_step = True
        flat_params.zero_grad()
        self._held, self.last = [], None     # the losses of the accumulate() calls since the last step; the last step's own batch's losses

    def forward(self, *batch):
        """check() + forward -> (the loss dict as loss_fn returned it, the weighted total); __call__ without the backward and the update (tools/bench_finetune_step.py
        times the three parts)"""
        self.flat.check()
        out = self.loss_fn(*batch)
        losses = out if isinstance(out, dict) else {"loss": out}
        total = None
        for k, v in losses.items():
            w = self.weights.get(k, 1.0)
            t = v if w == 1.0 else v * w
            total = t if total is None else total + t
        return losses, total

    def accumulate(self, *batch):
        """a micro-batch of the coming optimizer step: check(), forward and backward only -- the gradients add to the buffer's (every weight-gradient kernel adds,
        and the AdamW kernel of the step before cleared it).  With a reducer the base's _reducer is taken away for the call, so no trigger issues a collective: the
        step's one exchange is __call__'s.  Returns the unweighted detached losses.  From the first call on the optimizer clips the mean of the accumulated sum
        (FusedAdamW.mean_clip), which for a step of one batch is the clip of before, bit for bit."""
        self.opt.mean_clip = True
        base = self.flat.base if self.reducer is not None else None
        if base is not None:
            base._reducer = None
        try:
            losses, total = self.forward(*batch)
            total.backward()
        finally:
            if base is not None:
                base._reducer = self.reducer
        self._held.append({k: v.detach() for k, v in losses.items()})
        return self._held[-1]

    def __call__(self, *batch):
        """the optimizer step.  After j calls of accumulate() since the last step: the mean of the j + 1 gradients is clipped and stepped, each weighing 1 / (j + 1)
        whatever its batch size (as DDP weighs ranks), exchanged once, and the mean of the j + 1 loss dicts is returned; `last` keeps this batch's own losses."""
        losses, total = self.forward(*batch)
        total.backward()
        # every gradient launch is ordered before this point on the current stream (module docstring): no join here
        if self.reducer is not None:
            self.reducer.finish()   # the ranges no trigger launched, then the join of the comm stream
        if self.opt.mean_clip:
            self.opt.set_grad_scale(1.0 / (len(self._held) + 1))
        self.opt.step()
        self.last = {k: v.detach() for k, v in losses.items()}
        if not self._held:
            return self.last
        held, self._held = self._held + [self.last], []
        return {k: sum(h[k] for h in held) / len(held) for k in self.last}
