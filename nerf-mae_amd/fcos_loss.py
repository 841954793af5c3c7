"""FCOS training losses and target assignment of the reference's 3-D detector head on the HIP kernels of csrc/fcos.hip, with the reference's
names, argument order and return tuple (the import swap is one line):

  FCOSLossComputation                  nerf_rpn/model/fcos/loss.py:174-591
  FCOSProj2dLossComputation            the same for oriented boxes with the 2-D projection term, proj2d_loss_weight > 0 (loss.py:447-475, 579-585)
  encode_fcos_obb, decode_fcos_obb     nerf_rpn/model/fcos/utils.py:12-105
  fcos_targets                         the assignment on its own (prepare_targets), for inspection

Head outputs are the per-level NCDHW tensors as the head writes them, (N, 1, w, l, h) logits and (N, 6|8, w, l, h) regression, fp32; they are
read and differentiated in place (no permute, no cat).  Ground-truth boxes are one fp32 tensor per scene, [G, 6] (x0,y0,z0,x1,y1,z1) or [G, 7]
(x,y,z,w,l,h,theta in radians).  Targets come back in the dense layout: level by level, within a level scene by scene, within a scene the
locations of the flattened (w, l, h) grid, i.e. the reference's per-level label tensors concatenated.  Semantics: the header of csrc/fcos.hip
and DESIGN.md 3.9.

The loss is one autograd.Function: the assignment, the two device scalars (number of positives, sum of centerness targets), the focal loss and
the regression / centerness losses in the forward, two kernels in the backward; gradients go to box_cls, box_regression and centerness only.
With world_size == 1 the host never waits and nothing is allocated beyond the outputs, the dense target buffers and one partial-sum
workspace (8 bytes per 256 locations), so forward + backward can be captured with torch.cuda.graph (create the leaves on the capture stream:
DESIGN.md 3.8, Capture).  With world_size > 1 the two scalars are all-reduced as one 2-float tensor.

Stated deviations from the reference:
  - iou_loss_type="smooth_l1" raises NotImplementedError;
  - the 2-D projection term is opt-in through a class of its own, FCOSProj2dLossComputation (oriented boxes only, as in the reference), which FCOSModule builds
    for rotated_bbox=True and proj2d_loss_weight > 0: every positive's regression term gains proj2d_loss_weight T / 160 / 16 before the centerness weight, in the
    same fused forward and backward (csrc/fcos.hip, fcos_pos2d).  FCOSLossComputation itself keeps raising NotImplementedError for proj2d_loss_weight > 0, so that
    the default path runs the kernels without the term, unchanged; with axis-aligned boxes the reference ignores the weight, and a positive weight raises here;
  - the "unweighted sum if the weights sum to 0" branch of the IoU losses is not reproduced: positives always have positive centerness
    targets, because the in-box tests are strict;
  - with no positives reg_loss and centerness_loss are exact zeros with zero gradients (as in the reference);
  - a ground-truth box of volume 1e8 or more is unspecified; at most 64 scenes and 4 levels per call;
  - other dtypes than fp32 raise TypeError, CPU tensors RuntimeError, more than 4 levels ValueError (as rotated_iou._check);
  - `locations` is accepted and ignored (locations follow from the feature sizes and strides); `padding_masks`, when given, is the validity
    mask; the keyword grid_sizes= (int32 device tensor [N, 3], the scenes' original sizes) computes validity in the kernel instead."""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops

MAX_LEVELS, MAX_SCENES = ops.FCOS_MAX_LEVELS, ops.FCOS_MAX_SCENES


def _check(name, *tensors):
    for t in tensors:
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError(f"{name} takes fp32 tensors, got {getattr(t, 'dtype', type(t))}")
        if not t.is_cuda:
            raise RuntimeError(f"{name} needs HIP device tensors (there is no CPU path)")


def _boxes(name, targets, ncols):
    """list of per-scene [G, ncols] tensors -> (one [sum G, ncols] tensor, host offsets)"""
    _check(name, *targets)
    rows = [t.detach().reshape(-1, ncols) if t.numel() == 0 else t.detach() for t in targets]
    for t in rows:
        if t.dim() != 2 or t.shape[1] != ncols:
            raise ValueError(f"{name}: ground-truth boxes must be [G, {ncols}] per scene, got {tuple(t.shape)}")
    offsets = [0]
    for t in rows:
        offsets.append(offsets[-1] + t.shape[0])
    return (rows[0] if len(rows) == 1 else torch.cat(rows, 0)).contiguous(), offsets


def _validity(name, plan, grid_sizes, padding_masks, device):
    masks = None
    if padding_masks is not None:
        masks = [m.contiguous() for m in padding_masks]
        if len(masks) != plan.L or any(m.numel() != plan.N * n or m.element_size() != 1 or not m.is_cuda for m, n in zip(masks, plan.n)):
            raise ValueError(f"{name}: padding_masks must be one bool device tensor (N, w, l, h) per level")
        grid_sizes = None
    if grid_sizes is not None:
        if not isinstance(grid_sizes, torch.Tensor):
            grid_sizes = torch.tensor(grid_sizes, dtype=torch.int32, device=device)       # a host list costs a copy; pass a device tensor
        if grid_sizes.dtype != torch.int32 or tuple(grid_sizes.shape) != (plan.N, 3) or not grid_sizes.is_cuda:
            raise ValueError(f"{name}: grid_sizes must be an int32 device tensor [N, 3]")
        grid_sizes = grid_sizes.contiguous()
    return grid_sizes, masks


def fcos_targets(feature_sizes, fpn_strides, targets, center_sampling_radius=0.0, norm_reg_targets=False, grid_sizes=None, padding_masks=None,
                 return_scalars=False):
    """feature_sizes [(w,l,h)] per level, fpn_strides, targets: list of per-scene fp32 device boxes [G,6] or [G,7] ->
    (labels [P] fp32 0/1, reg_targets [P,6|8], gt_index [P] int32 (-1: none), centerness_targets [P], valid [P] bool) in the dense layout;
    return_scalars adds the fp32 device pair (valid positives, sum of their centerness targets)."""
    if len(feature_sizes) > MAX_LEVELS:
        raise ValueError(f"fcos_targets supports at most {MAX_LEVELS} levels, got {len(feature_sizes)}")
    ncols = targets[0].shape[-1] if isinstance(targets[0], torch.Tensor) and targets[0].dim() >= 1 else 0
    if ncols not in (6, 7):
        raise ValueError("fcos_targets: ground-truth boxes must have 6 or 7 columns")
    boxes, offsets = _boxes("fcos_targets", targets, ncols)
    plan = ops.FcosPlan(feature_sizes, fpn_strides, len(targets))
    grid_sizes, masks = _validity("fcos_targets", plan, grid_sizes, padding_masks, boxes.device)
    out = ops.fcos_assign(plan, boxes, offsets, ncols, grid_sizes, masks, float(center_sampling_radius), norm_reg_targets)
    return out[:6] if return_scalars else out[:5]


class _FcosLoss(Function):
    """(cfg, boxes, offsets, grid_sizes, masks, *cls levels, *regression levels, *centerness levels) -> (cls_loss, reg_loss, centerness_loss)"""

    @staticmethod
    def forward(ctx, cfg, boxes, offsets, grid_sizes, masks, *heads):
        plan, ncols, loss_type, add_l1, radius, norm, world, w2d = cfg        # w2d: the 2-D projection weight, None without the term
        L = plan.L
        heads = [h.contiguous() for h in heads]
        cls, reg, ctr = heads[:L], heads[L:2 * L], heads[2 * L:]
        labels, targets, _, ctr_t, valid, scalars, partials = ops.fcos_assign(plan, boxes, offsets, ncols, grid_sizes, masks, radius, norm)
        if world > 1:
            import torch.distributed as dist
            dist.all_reduce(scalars, op=dist.ReduceOp.SUM)
        cls_loss = ops.fcos_focal_fwd(plan, cls, labels, valid, scalars, float(world), partials)
        if w2d is None:
            reg_loss, ctr_loss = ops.fcos_pos_fwd(plan, 6 if ncols == 6 else 8, loss_type, add_l1, reg, ctr, labels, targets, ctr_t, valid, scalars, float(world), partials)
        else:
            reg_loss, ctr_loss = ops.fcos_pos2d_fwd(plan, loss_type, add_l1, w2d, reg, ctr, labels, targets, ctr_t, valid, scalars, float(world), partials)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(labels, targets, ctr_t, valid, scalars, *heads)
        ctx.cfg = cfg
        return cls_loss, reg_loss, ctr_loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_reg, g_ctr):
        plan, ncols, loss_type, add_l1, _, _, world, w2d = ctx.cfg
        L = plan.L
        labels, targets, ctr_t, valid, scalars, *heads = ctx.saved_tensors
        cls, reg, ctr = heads[:L], heads[L:2 * L], heads[2 * L:]
        gs = [g if g is None else g.contiguous() for g in (g_cls, g_reg, g_ctr)]
        none = [None] * L
        dcls = ops.fcos_focal_bwd(plan, cls, labels, valid, scalars, float(world), gs[0]) if gs[0] is not None and any(ctx.needs_input_grad[5:5 + L]) else none
        if (gs[1] is not None or gs[2] is not None) and any(ctx.needs_input_grad[5 + L:]):
            if w2d is None:
                dreg, dctr = ops.fcos_pos_bwd(plan, 6 if ncols == 6 else 8, loss_type, add_l1, reg, ctr, labels, targets, ctr_t, valid, scalars, float(world), gs[1], gs[2])
            else:
                dreg, dctr = ops.fcos_pos2d_bwd(plan, loss_type, add_l1, w2d, reg, ctr, labels, targets, ctr_t, valid, scalars, float(world), gs[1], gs[2])
        else:
            dreg, dctr = none, none
        return (None, None, None, None, None, *dcls, *dreg, *dctr)


class FCOSLossComputation(object):
    """The reference's FCOSLossComputation on the fused kernels: same constructor, same call, same three losses."""

    def __init__(self, fpn_strides, center_sampling_radius, iou_loss_type, norm_reg_targets, world_size, use_obb, use_additional_l1_loss, proj2d_loss_weight=0.0):
        if len(fpn_strides) > MAX_LEVELS:
            raise ValueError(f"FCOSLossComputation supports at most {MAX_LEVELS} levels (the reference's range table has four rows), got {len(fpn_strides)}")
        if iou_loss_type == "smooth_l1":
            raise NotImplementedError('iou_loss_type "smooth_l1" is not built; use "iou", "linear_iou", "giou"' + (' or "diou"' if use_obb else ""))
        if proj2d_loss_weight > 0:
            raise NotImplementedError("FCOSLossComputation runs without the 2-D projection loss; proj2d_loss_weight > 0 is FCOSProj2dLossComputation (oriented boxes only)")
        if iou_loss_type not in ops.FCOS_LOSS_TYPES or (iou_loss_type == "diou" and not use_obb):
            raise NotImplementedError(f"iou_loss_type {iou_loss_type!r} is not defined for use_obb={bool(use_obb)}")
        self.fpn_strides = [int(s) for s in fpn_strides]
        self.center_sampling_radius = float(center_sampling_radius)
        self.iou_loss_type = iou_loss_type
        self.norm_reg_targets = bool(norm_reg_targets)
        self.world_size = max(int(world_size), 1)
        self.use_obb = bool(use_obb)
        self.use_additional_l1_loss = bool(use_additional_l1_loss)
        self.proj2d_loss_weight = proj2d_loss_weight
        self._w2d = None                # set by FCOSProj2dLossComputation

    def __call__(self, locations, box_cls, box_regression, centerness, targets, padding_masks=None, grid_sizes=None):
        """box_cls, box_regression, centerness: lists of per-level tensors (N,1,w,l,h), (N,6|8,w,l,h), (N,1,w,l,h); targets: list of N box tensors
        -> (cls_loss, reg_loss, centerness_loss), 0-dim fp32 device tensors"""
        name = type(self).__name__
        L = len(box_cls)
        if L > MAX_LEVELS:
            raise ValueError(f"{name} supports at most {MAX_LEVELS} levels, got {L}")
        if L != len(self.fpn_strides) or len(box_regression) != L or len(centerness) != L:
            raise ValueError(f"{name}: one tensor per level and stride for box_cls, box_regression and centerness")
        _check(name, *box_cls, *box_regression, *centerness)
        C, ncols = (8, 7) if self.use_obb else (6, 6)
        N = box_cls[0].shape[0]
        sizes = [tuple(t.shape[2:]) for t in box_cls]
        for c, r, t, s in zip(box_cls, box_regression, centerness, sizes):
            if c.dim() != 5 or tuple(c.shape) != (N, 1, *s) or tuple(r.shape) != (N, C, *s) or t.numel() != c.numel():
                raise ValueError(f"{name}: per level box_cls (N,1,w,l,h), box_regression (N,{C},w,l,h), centerness (N,1,w,l,h); got {tuple(c.shape)}, {tuple(r.shape)}, {tuple(t.shape)}")
        if len(targets) != N:
            raise ValueError(f"{name}: {N} scenes but {len(targets)} box tensors")
        boxes, offsets = _boxes(name, targets, ncols)
        plan = ops.FcosPlan(sizes, self.fpn_strides, N)
        grid_sizes, masks = _validity(name, plan, grid_sizes, padding_masks, boxes.device)
        cfg = (plan, ncols, ops.FCOS_LOSS_TYPES[self.iou_loss_type], self.use_obb and self.use_additional_l1_loss, self.center_sampling_radius, self.norm_reg_targets,
               self.world_size, self._w2d)
        return _FcosLoss.apply(cfg, boxes, offsets, grid_sizes, masks, *box_cls, *box_regression, *centerness)


class FCOSProj2dLossComputation(FCOSLossComputation):
    """FCOSLossComputation for oriented boxes with the reference's 2-D projection term (--proj2d_loss_weight of the FCOS launchers): same call, same three losses;
    cls_loss and centerness_loss have the bits of FCOSLossComputation's, reg_loss gains proj2d_loss_weight sum_p ct_p T_p / 160 / 16 / (sum ct / world_size) with T
    (proj2d.py) between decode_fcos_obb(0, box_regression) and decode_fcos_obb(0, reg_targets) under the cameras of get_w2cs(160), for every iou_loss_type and next
    to the additional L1 term."""

    def __init__(self, fpn_strides, center_sampling_radius, iou_loss_type, norm_reg_targets, world_size, use_additional_l1_loss, proj2d_loss_weight):
        if not proj2d_loss_weight > 0:
            raise ValueError(f"FCOSProj2dLossComputation: proj2d_loss_weight > 0, got {proj2d_loss_weight!r}; without the term use FCOSLossComputation")
        super().__init__(fpn_strides, center_sampling_radius, iou_loss_type, norm_reg_targets, world_size, True, use_additional_l1_loss)
        self.proj2d_loss_weight = self._w2d = float(proj2d_loss_weight)


def encode_fcos_obb(locations, boxes):
    """locations [n,3], boxes [n,7] fp32 -> midpoint-offset targets [n,8] (no gradient)"""
    _check("encode_fcos_obb", locations, boxes)
    if boxes.dim() != 2 or boxes.shape[1] != 7 or tuple(locations.shape) != (boxes.shape[0], 3):
        raise ValueError("encode_fcos_obb: locations [n,3], boxes [n,7]")
    return ops.fcos_obb_encode(locations.detach().contiguous(), boxes.detach().contiguous())


class _Decode(Function):
    @staticmethod
    def forward(ctx, locations, box_regression):
        locations, box_regression = locations.contiguous(), box_regression.contiguous()
        ctx.save_for_backward(box_regression)
        return ops.fcos_obb_decode_fwd(locations, box_regression)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        reg, = ctx.saved_tensors
        g = g.contiguous()
        return (g[:, :3].contiguous() if ctx.needs_input_grad[0] else None), (ops.fcos_obb_decode_bwd(reg, g) if ctx.needs_input_grad[1] else None)


def decode_fcos_obb(locations, box_regression):
    """locations [n,3], box_regression [n,8] fp32 -> boxes [n,7] (x,y,z,w,l,h,theta); differentiable through the device code of the loss"""
    _check("decode_fcos_obb", locations, box_regression)
    if box_regression.dim() != 2 or box_regression.shape[1] != 8 or tuple(locations.shape) != (box_regression.shape[0], 3):
        raise ValueError("decode_fcos_obb: locations [n,3], box_regression [n,8]")
    return _Decode.apply(locations, box_regression)
