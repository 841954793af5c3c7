"""The RoI (second) stage of the reference's two-stage detector on the HIP kernels of csrc/roi_head.hip, with the reference's names (the import swap
is one line):

  roi_targets_dense / ProposalTargetLayer   nerf_rpn/model/detector.py:12-167 over batched_box_iou (model/utils.py:371-458)
  LevelMapper                               model/level_mapper.py:21-77 (with _setup_scales)
  ROIPool                                   detector.py:170-438: normal_forward and rotated_forward with feature_extracting_type "pooling" or (oriented
                                            boxes) "interpolation", remap
  RCNN                                      detector.py:441-496, a torch module with the reference's state_dict keys (two small convs and two Linear layers), on
                                            stock nn.Conv3d / nn.Linear: the default
  FusedRCNN                                 the same head, parameters and state_dict on the channels-last 3x3x3 conv layer and the output kernels of
                                            csrc/box_head.hip (compute_dtype is an addition); chosen by constructing it
  roi_head_loss / roi_decode / RotatedCoder  detector.py:536-559 with coder/rotated_coder.py and coder/AABB_coder.py
  Classification_Model                      detector.py:499-627

All tensors are fp32 on the device.  Boxes are [.., 6] (x0,y0,z0,x1,y1,z1) or [.., 7] (x,y,z,w,h,d,theta); RoIs carry their pyramid level in front, [.., 1+6|7].
roi_targets_dense takes what rpn.rpn_proposals_dense returns (boxes [N,cap,6|7], levels, counts), so the first stage feeds the second without a host wait.
Feature maps are one (N, C, W, H, D) tensor per level, as fpn.py returns them; the reference's list of per-scene lists is accepted and stacked.

In sampling mode nothing waits for the host and every sum of ours has a fixed order (the scatter of the pooling backward uses fp32 atomics, as rotated.py's
does), so targets + pooling + head + losses, forward and backward, can be captured with torch.cuda.graph; the sampler's counter lives on the device and
advances inside the graph, so every replay draws afresh.  Evaluation with dense input waits once, for the N counts that size its lists.

Stated deviations from the reference:
  - the order of the foreground slots is ours (ascending proposal index); the losses do not depend on it;
  - np.random's stream is not reproduced: a foreground candidate's key is a hash of (seed, counter, scene, index) and the smallest keys are taken (uniform
    without replacement, ties at the cut to the lower index); background draw j is candidate floor(u_j n_bg) in index order with u_j a hash of (seed, counter,
    scene, j): uniform with replacement, as the reference's floor(rand * n);
  - equal IoU of one RoI with several boxes goes to the lowest box index (torch.max leaves it open); if bg_threshold > fg_threshold a RoI above both
    is foreground;
  - a scene with neither foreground nor background candidates: the reference raises; here its rows have label -1 and zero boxes, and the losses ignore them;
  - in evaluation mode (dense entry) rows past counts[i] are zero with label -1; a scene without ground-truth boxes has IoU 0 everywhere;
  - the axis-aligned crop: the reference's negative lower index wraps Python-style; here the crop is clamped to the map and an empty crop gives zeros;
  - oriented RoIs: the reference's enlarge_roi writes the enlarged sizes into the caller's RoI tensor (detector.py:199-201), so with remap off
    Classification_Model encodes, decodes and returns the ENLARGED RoIs (tests/golden/g22_roi_head.npz confirms this reading), and with remap on (where the
    reference enlarges a copy) the original ones.  This module computes the same values but never writes into a caller's tensor;
  - an oriented RoI's sampling grid is cut at ROI_MAX_GRID points per axis (the reference would run out of memory long before);
  - where the zero padding or a masked point ties with a value, the value wins; among equal values the first in (x, y, z) order wins, as in nn.MaxPool3d;
  - roi_decode has no gradient (the reference's decode only feeds outputs); RoIs get no gradient from the pooling;
  - both losses are 0 with zero gradient when no row counts (the reference: NaN objectness without valid rows); labels outside [0, n_classes) are ignored rows
    (F.cross_entropy raises);
  - feature_extracting_type="interpolation" with axis-aligned boxes raises NotImplementedError: there the reference silently max-pools and ignores the
    switch (only rotated_forward reads it); any other string raises ValueError at construction (the reference: NameError on the first oriented forward);
  - in an oriented RoI's interpolation an output size of 1 on an axis takes grid point 0 of that axis (the grid's corner, not its centre), as F.interpolate
    with align_corners=True does: the reference's behaviour, kept;
  - use_cuda=True raises NotImplementedError: that path returns features in level order rather than RoI order.  (The launcher, run_rpn_detect.py, hands
    --feature_extracting_type to ROIPool (:103, :166-169); it parses --use_cuda and --remap (:97-100) but hands neither over);
  - other dtypes than fp32 raise TypeError, CPU tensors RuntimeError; more than MAX_LEVELS levels, MAX_SCENES scenes, MAX_ROWS rows per scene, MAX_CELLS
    output cells or MAX_CLASSES classes raise ValueError."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import conv_layer, ops
from .fcos_loss import _boxes, _check
from .model import _gradbuf
from .rpn import MAX_LEVELS, MAX_SCENES

MAX_ROWS, MAX_CELLS, MAX_CLASSES, MAX_GRID = ops.ROI_MAX_ROWS, ops.ROI_MAX_CELLS, ops.ROI_MAX_CLASSES, ops.ROI_MAX_GRID


def _int32(name, what, t, shape):
    if not isinstance(t, torch.Tensor) or t.dtype != torch.int32 or tuple(t.shape) != tuple(shape) or not t.is_cuda:
        raise ValueError(f"{name}: {what} must be an int32 device tensor {list(shape)}")
    return t.contiguous()


def _rng(name, rng_state):
    if not isinstance(rng_state, torch.Tensor) or rng_state.dtype != torch.int64 or tuple(rng_state.shape) != (2,) or not rng_state.is_cuda:
        raise ValueError(f"{name}: rng_state must be an int64 device tensor [2] = (seed, counter)")
    return rng_state


# ---- proposal targets ------------------------------------------------------------------------------------------------------------------------
def roi_targets_dense(boxes, levels, counts, gt_boxes, gt_labels, rois_per_image, fg_rois_per_image, fg_threshold, bg_threshold, rng_state, is_sample,
                      keep=None, keep_counts=None):
    """boxes [N,cap,6|7], levels [N,cap] int32, counts [N] int32: rpn_proposals_dense's results; gt_boxes, gt_labels: per scene [k,6|7] and [k] fp32.
    Sampling: R = rois_per_image rows per scene, drawn by rng_state (int64 device [2] = (seed, counter), the counter advances by one) or given by keep [N,R]
    int32 (proposal index, -1: none) with keep_counts [N,2] int32 (foreground slots first, then background).  Evaluation: R = cap, every proposal.
    -> (labels [N,R], rois [N,R,1+6|7], gt_rois [N,R,6|7], keep [N,R] int32, counts [N,2] int32 = (foreground, background) slots; None in evaluation)"""
    name = "roi_targets_dense"
    _check(name, boxes)
    if boxes.dim() != 3 or boxes.shape[2] not in (6, 7):
        raise ValueError(f"{name}: boxes must be [N, cap, 6|7], got {tuple(boxes.shape)}")
    N, cap, B = boxes.shape
    if not 1 <= N <= MAX_SCENES:
        raise ValueError(f"{name} supports 1 to {MAX_SCENES} scenes, got {N}")
    if not 1 <= cap <= MAX_ROWS:
        raise ValueError(f"{name} supports 1 to {MAX_ROWS} proposals per scene, got {cap}")
    if len(gt_boxes) != N or len(gt_labels) != N:
        raise ValueError(f"{name}: {N} scenes but {len(gt_boxes)} box and {len(gt_labels)} label tensors")
    levels, counts = _int32(name, "levels", levels, (N, cap)), _int32(name, "counts", counts, (N,))
    gt, offsets = _boxes(name, gt_boxes, B)
    _check(name, *gt_labels)
    if any(l.numel() != b.shape[0] for l, b in zip(gt_labels, gt_boxes)):
        raise ValueError(f"{name}: one label per ground-truth box")
    lab = torch.cat([l.detach().reshape(-1) for l in gt_labels]).contiguous()
    R, want_fg = cap, 0
    if is_sample:
        R, want_fg = int(rois_per_image), int(fg_rois_per_image)
        if not 1 <= R <= MAX_ROWS or want_fg < 0:
            raise ValueError(f"{name}: 1 to {MAX_ROWS} rois_per_image and fg_rois_per_image >= 0, got {R}, {want_fg}")
        if keep is None:
            rng_state = _rng(name, rng_state)
        else:
            keep, keep_counts, rng_state = _int32(name, "keep", keep, (N, R)), _int32(name, "keep_counts", keep_counts, (N, 2)), None
    with torch.no_grad():
        labels, rois, gt_rois, keep, counts2, _, _ = ops.roi_targets(boxes.detach().contiguous(), levels, counts, gt, lab, offsets, R, want_fg, float(fg_threshold), float(bg_threshold),
                                                                     bool(is_sample), rng_state, keep, keep_counts)
    return labels, rois, gt_rois, keep, counts2


def _pack(name, all_rois, B):
    """list of per-scene [K, 1+B] RoIs -> (boxes [N,cap,B], levels [N,cap] int32, counts [N] int32, host counts)"""
    _check(name, *all_rois)
    if any(r.dim() != 2 or r.shape[1] != 1 + B for r in all_rois):
        raise ValueError(f"{name}: RoIs must be [K, {1 + B}] per scene (level, box)")
    ks = [r.shape[0] for r in all_rois]
    cap = max(max(ks), 1)
    dense = torch.stack([F.pad(r.detach(), (0, 0, 0, cap - k)) for r, k in zip(all_rois, ks)])
    counts = torch.tensor(ks, dtype=torch.int32).to(dense.device, non_blocking=True)
    return dense[..., 1:].contiguous(), dense[..., 0].to(torch.int32).contiguous(), counts, ks


class ProposalTargetLayer(nn.Module):
    """The reference's constructor and forward(all_rois, gt_boxes, gt_labels, is_sample); all_rois: per scene [K, 1+6|7] with the level in column 0.
    Sampling -> (labels [N,R], rois [N,R,1+6|7], gt_rois [N,R,6|7]); evaluation -> per-scene lists.  rng_state (int64 device [2]) is created on the first
    sampling call from `seed`; copy into it to replay a draw.  forward_dense takes rpn_proposals_dense's results."""

    def __init__(self, nclasses, batch_size=1000, fg_fraction=0.5, fg_threshold=0.5, bg_threshold=0.2, is_rotated_bbox=False, seed=0):
        super().__init__()
        self._num_classes = nclasses
        self.batch_size, self.fg_fraction = batch_size, fg_fraction
        self.fg_threshold, self.bg_threshold = fg_threshold, bg_threshold
        self.is_rotated_bbox = is_rotated_bbox
        self.bbox_size = 7 if is_rotated_bbox else 6
        self.seed = int(seed)
        self.rng_state = None

    def _sizes(self, num_mesh):
        rois_per_image = int(self.batch_size / num_mesh)
        fg = int(np.round(self.fg_fraction * rois_per_image))
        return rois_per_image, (1 if fg == 0 else fg)

    def forward_dense(self, boxes, levels, counts, gt_boxes, gt_labels, is_sample, keep=None, keep_counts=None):
        """-> roi_targets_dense's five results"""
        R, fg = self._sizes(boxes.shape[0])
        if is_sample and keep is None and self.rng_state is None:
            self.rng_state = torch.tensor([self.seed, 0], dtype=torch.int64, device=boxes.device)
        return roi_targets_dense(boxes, levels, counts, gt_boxes, gt_labels, R, fg, self.fg_threshold, self.bg_threshold, self.rng_state, is_sample, keep, keep_counts)

    def forward(self, all_rois, gt_boxes, gt_labels, is_sample, keep=None, keep_counts=None):
        if not (len(all_rois) == len(gt_boxes) == len(gt_labels)):
            raise ValueError("ProposalTargetLayer: one RoI, box and label tensor per scene")
        boxes, levels, counts, ks = _pack("ProposalTargetLayer", all_rois, self.bbox_size)
        labels, rois, gt_rois, _, _ = self.forward_dense(boxes, levels, counts, gt_boxes, gt_labels, is_sample, keep, keep_counts)
        if is_sample:
            return labels, rois, gt_rois
        return [labels[i, :k] for i, k in enumerate(ks)], [rois[i, :k] for i, k in enumerate(ks)], [gt_rois[i, :k] for i, k in enumerate(ks)]


# ---- level mapper ----------------------------------------------------------------------------------------------------------------------------
class LevelMapper:
    """boxes [..., 6|7] fp32 device -> int64 levels clamp(floor(lvl0 + log2(cbrt(b3 b4 b5) / s0) + eps), k_min, k_max) - k_min.  As in the reference the
    "volume" is the product of columns 3, 4, 5 whatever the box form."""

    def __init__(self, k_min, k_max, canonical_scale=160, canonical_level=4, eps=1e-6):
        self.k_min, self.k_max, self.s0, self.lvl0, self.eps = k_min, k_max, canonical_scale, canonical_level, eps

    def levels32(self, boxes):
        _check("LevelMapper", boxes)
        if boxes.shape[-1] not in (6, 7):
            raise ValueError(f"LevelMapper: boxes must be [..., 6|7], got {tuple(boxes.shape)}")
        flat = boxes.detach().reshape(-1, boxes.shape[-1]).contiguous()
        return ops.roi_level_map(flat, boxes.shape[-1], int(self.k_min), int(self.k_max), float(self.s0), float(self.lvl0), float(self.eps)).reshape(boxes.shape[:-1])

    def __call__(self, boxlists):
        return self.levels32(boxlists).to(torch.int64)


def initLevelMapper(k_min, k_max, canonical_scale=160, canonical_level=4, eps=1e-6):
    return LevelMapper(k_min, k_max, canonical_scale, canonical_level, eps)


def _setup_scales(scales, canonical_scale, canonical_level):
    lvl_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
    lvl_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
    return initLevelMapper(int(lvl_min), int(lvl_max), canonical_scale=canonical_scale, canonical_level=canonical_level)


# ---- pyramid RoI pooling -----------------------------------------------------------------------------------------------------------------------
class _RoiPool(Function):
    """(plan, rois [N,R,1+B], level override or None, *maps) -> [N*R, C, ow, oh, od]"""

    @staticmethod
    def forward(ctx, plan, rois, override, *maps):
        out, arg = ops.roi_pool_fwd(plan, maps, rois, override)
        ctx.save_for_backward(arg, rois, *([] if override is None else [override]))
        ctx.plan = plan
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        arg, rois, *rest = ctx.saved_tensors
        dmaps = ops.roi_pool_bwd(ctx.plan, dout.contiguous(), arg, rois, rest[0] if rest else None, ctx.needs_input_grad[3:])
        return (None, None, None, *dmaps)


class _RoiInterp(Function):
    """(plan, oriented rois [N,R,8], level override or None, *maps) -> [N*R, C, ow, oh, od]; the backward forms the geometry again from the RoIs"""

    @staticmethod
    def forward(ctx, plan, rois, override, *maps):
        out = ops.roi_interp_fwd(plan, maps, rois, override)
        ctx.save_for_backward(rois, *([] if override is None else [override]))
        ctx.plan = plan
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        rois, *rest = ctx.saved_tensors
        dmaps = ops.roi_interp_bwd(ctx.plan, dout.contiguous(), rois, rest[0] if rest else None, ctx.needs_input_grad[3:])
        return (None, None, None, *dmaps)


class ROIPool(nn.Module):
    """The reference's constructor.  forward(feature, rois, original_size=None): feature = one (N, C, W, H, D) fp32 map per level (or the reference's list
    of per-scene lists of (C, W, H, D) maps); rois = [N, R, 1+6|7], or a list of per-scene [K, 1+6|7] ->  [N*R, C, ow, oh, od] in RoI order for a tensor,
    the reference's per-scene list for a list.  Differentiable with respect to the maps."""

    def __init__(self, output_size=[1, 1, 1], spatial_scale=[1, 1, 1, 1], enlarge_scale=0.2, is_rotated_bbox=False, feature_extracting_type="pooling", max_res=200,
                 remap=False, use_cuda=False):
        super().__init__()
        if use_cuda:
            raise NotImplementedError("ROIPool(use_cuda=True) is not built: that path returns features in level order, not RoI order; "
                                      "rotated.ROIAlignRotated3D is available on its own")
        if feature_extracting_type not in ("pooling", "interpolation"):
            raise ValueError(f'ROIPool: feature_extracting_type must be "pooling" or "interpolation", got {feature_extracting_type!r}')
        if feature_extracting_type == "interpolation" and not is_rotated_bbox:
            raise NotImplementedError('ROIPool(feature_extracting_type="interpolation") exists for oriented boxes (is_rotated_bbox=True) only: with axis-aligned '
                                      "boxes the reference max-pools whatever the type, and this module does not label that as interpolation")
        if not 1 <= len(spatial_scale) <= MAX_LEVELS:
            raise ValueError(f"ROIPool supports 1 to {MAX_LEVELS} levels, got {len(spatial_scale)}")
        self.output_size = tuple(int(v) for v in output_size)
        if len(self.output_size) != 3 or min(self.output_size) < 1 or self.output_size[0] * self.output_size[1] * self.output_size[2] > MAX_CELLS:
            raise ValueError(f"ROIPool: output_size must be three sizes >= 1 with at most {MAX_CELLS} cells, got {output_size}")
        self.spatial_scale = [float(s) for s in spatial_scale]
        if min(self.spatial_scale) <= 0:
            raise ValueError("ROIPool: spatial_scale must be positive")
        self.enlarge_scale = enlarge_scale
        self.is_rotated_bbox = bool(is_rotated_bbox)
        self.feature_extracting_type = feature_extracting_type
        self.canonical_scale, self.canonical_level = max_res, len(spatial_scale)
        self.remap, self.use_cuda = bool(remap), False
        self.bbox_size = 7 if is_rotated_bbox else 6
        self.map_levels = _setup_scales([1 / s for s in self.spatial_scale], self.canonical_scale, self.canonical_level)

    def enlarge_roi(self, roi):
        """the reference's arithmetic, out of place: oriented sizes times 1 + enlarge_scale; axis-aligned mid -+ (hi - lo) / 4 (1 + enlarge_scale)"""
        if self.is_rotated_bbox:
            return torch.cat([roi[..., :3], roi[..., 3:6] * (1 + self.enlarge_scale), roi[..., 6:]], -1)
        extent, offset = (roi[..., 3:] - roi[..., :3]) / 2 * (1 + self.enlarge_scale), (roi[..., 3:] + roi[..., :3]) / 2
        return torch.cat([-0.5 * extent + offset, 0.5 * extent + offset], -1)

    def _maps(self, feature):
        if len(feature) and isinstance(feature[0], (list, tuple)):
            feature = [torch.stack([scene[k] for scene in feature]) for k in range(len(feature[0]))]
        feature = list(feature)
        if len(feature) != len(self.spatial_scale):
            raise ValueError(f"ROIPool: {len(self.spatial_scale)} levels but {len(feature)} feature maps")
        _check("ROIPool", *feature)
        N, C = feature[0].shape[:2]
        if any(f.dim() != 5 or tuple(f.shape[:2]) != (N, C) for f in feature):
            raise ValueError("ROIPool: feature maps must be (N, C, W, H, D) per level with the same N and C")
        if not 1 <= N <= MAX_SCENES:
            raise ValueError(f"ROIPool supports 1 to {MAX_SCENES} scenes, got {N}")
        return [f.contiguous() for f in feature]

    def forward(self, feature, rois, original_size=None):
        maps = self._maps(feature)
        N, B = maps[0].shape[0], self.bbox_size
        ks = None
        if not isinstance(rois, torch.Tensor):
            _check("ROIPool", *rois)
            ks = [r.shape[0] for r in rois]
            R = max(max(ks), 1)
            rois = torch.stack([F.pad(r.detach().reshape(-1, 1 + B), (0, 0, 0, R - k)) for r, k in zip(rois, ks)])
        _check("ROIPool", rois)
        if rois.dim() != 3 or rois.shape[0] != N or rois.shape[2] != 1 + B:
            raise ValueError(f"ROIPool: rois must be [N = {N}, R, {1 + B}], got {tuple(rois.shape)}")
        if not 1 <= rois.shape[1] <= MAX_ROWS:
            raise ValueError(f"ROIPool supports 1 to {MAX_ROWS} RoIs per scene, got {rois.shape[1]}")
        rois = rois.detach().contiguous()
        override = self.map_levels.levels32(rois[..., 1:]).reshape(-1).contiguous() if self.remap else None
        plan = ops.RoiPoolPlan(maps, self.spatial_scale, self.output_size, 1 + self.enlarge_scale, B)
        out = (_RoiInterp if self.feature_extracting_type == "interpolation" else _RoiPool).apply(plan, rois, override, *maps)
        if ks is None:
            return out
        R = rois.shape[1]
        return [out[i * R:i * R + k] for i, k in enumerate(ks)]


# ---- box head --------------------------------------------------------------------------------------------------------------------------------
class RCNN(nn.Module):
    """Two optional 3x3x3 conv + ReLU layers, then two Linear layers on the flattened (or mean-pooled) volume -> (pred_bbox_delta, pred_scores).
    state_dict keys: layer.0, layer.2, RCNN_bbox_pred, RCNN_cls_score.  `block` is accepted and unused, as in the reference."""

    def __init__(self, input_dim, block, n_classes, input_size, is_add_layer=False, is_rotated_bbox=False, is_flatten=True):
        super().__init__()
        self.in_planes, self.n_classes = input_dim, n_classes
        self.is_rotated_bbox, self.is_flatten = is_rotated_bbox, is_flatten
        self.reg_dim = 7 if is_rotated_bbox else 6
        self.layer = None
        if is_add_layer:
            self.layer = nn.Sequential(nn.Conv3d(input_dim, input_dim, kernel_size=3, padding=1), nn.ReLU(inplace=True),
                                       nn.Conv3d(input_dim, input_dim, kernel_size=3, padding=1), nn.ReLU(inplace=True))
        width = input_dim
        if is_flatten:
            self.flatten_size = input_size[0] * input_size[1] * input_size[2]
            width = input_dim * self.flatten_size
        self.RCNN_bbox_pred = nn.Linear(width, self.reg_dim)
        self.RCNN_cls_score = nn.Linear(width, n_classes)

    def forward(self, pooling_feature):
        x = pooling_feature if self.layer is None else self.layer(pooling_feature)
        x = x.reshape(x.size(0), -1) if self.is_flatten else x.mean((-1, -2, -3))
        return self.RCNN_bbox_pred(x), self.RCNN_cls_score(x)


class _FusedRCNNFn(Function):
    """(anchor, head, pooled fp32 (M, C, ow, oh, od)) -> (pred_bbox_delta [M, 6|7], pred_scores [M, n_classes]) fp32: the layout pass to channels-last per RoI,
    the two 3x3x3 convs with the RoI as the batch index (is_add_layer), then the output kernel.  The parameters are not autograd inputs: the kernels add their
    gradients into .grad (as in rpn._RPNHeadFn), every one of them in a fixed order.  anchor is the head's one-element leaf that requires a gradient (as
    model._EmbedFn's): with it the outputs carry a graph, and the backward runs, also when the pooled tensor needs no gradient (a head trained on stored
    features); it receives none.  Saved: the input of every conv (rectified in place) and the last conv's output before its ReLU, which the output kernel applies
    as it reads."""

    @staticmethod
    def forward(ctx, anchor, head, pooled):
        M, C = pooled.shape[:2]
        xs = [ops.ncdhw_to_ndhwc(pooled, head.compute_dtype)]
        if head.layer is not None:
            for k in range(2):
                y = conv_layer.forward(head._pk, f"c{k}", head.layer[2 * k], xs[-1])
                if k == 0:                      # the last conv's ReLU is fused into the output kernel's load
                    ops.relu_(y)
                xs.append(y)
        box, cls, xmean = ops.box_head_out_fwd(xs[-1].view(M, -1, C), head._wcat, head.RCNN_bbox_pred.bias, head.RCNN_cls_score.bias, head.is_flatten, head.layer is not None)
        ctx.set_materialize_grads(False)
        ctx.head, ctx.saved = head, (xs, xmean)
        return box, cls

    @staticmethod
    @once_differentiable
    def backward(ctx, g_box, g_cls):
        head, (xs, xmean) = ctx.head, ctx.saved
        if g_box is None and g_cls is None:
            return None, None, None
        need_dx = ctx.needs_input_grad[2]
        M, C = xs[-1].shape[0], xs[-1].shape[-1]
        box, cls = head.RCNN_bbox_pred, head.RCNN_cls_score
        grads = [None if g is None else g.contiguous() for g in (g_box, g_cls)]
        bufs = [(None, None) if g is None else (_gradbuf(lin.weight), _gradbuf(lin.bias)) for g, lin in zip(grads, (box, cls))]
        dy = ops.box_head_out_bwd(xs[-1].view(M, -1, C), head._wcat, xmean, grads[0], grads[1], head.reg_dim, head.n_classes, head.is_flatten, head.layer is not None,
                                  bufs[0][0], bufs[1][0], bufs[0][1], bufs[1][1]).view(xs[-1].shape)
        keep = []   # tensors the forked side stream still reads -- referenced until the join
        if head.layer is not None:
            for k in (1, 0):
                conv = head.layer[2 * k]
                if k == 0:
                    ops.relu_bwd_(dy, xs[1])
                keep.append(dy)
                with ops.side_stream():         # conv_layer.backward's two sums add atomically; these add in a fixed order
                    ops.conv3d_k3_wgrad_fixed(dy, xs[k], _gradbuf(conv.weight))
                    ops.colsum_fixed(dy, _gradbuf(conv.bias))
                if k > 0 or need_dx:
                    dy = ops.conv3d_k3(dy, head._pk[f"c{k}.wd"], C)
            ops.join_side()
        del keep
        return None, None, (ops.ndhwc_to_ncdhw(dy) if need_dx else None)


class FusedRCNN(RCNN):
    """RCNN on the project's kernels: the reference's constructor plus compute_dtype (bfloat16 or float32); the same parameter holders, names, shapes and default
    initialisation, so a state dict moves between the two classes under strict=True; the holders' own forward is never used.
    forward(pooling_feature): the fp32 (M, C, ow, oh, od) tensor of ROIPool -> (pred_bbox_delta [M, 6|7], pred_scores [M, n_classes]) fp32, differentiable with
    respect to pooling_feature; the parameters' gradients are added into .grad by the kernels, every sum in a fixed order (two runs give the same bits).
    A row's outputs do not depend on how many rows share the call or where the row stands: the output kernel's contraction order is fixed by S and C alone, and the
    shared conv layer sums an output element's taps and channels in one order whatever the batch (tests/test_box_head_gpu.py holds both to torch.equal).
    The fp32 masters are repacked into the compute dtype on every call: the convs through conv_layer.ensure_packed, the two Linear weights by csrc/box_head.hip's
    own pack, which also permutes nn.Linear's NCDHW flatten order (c S + s) to the activations' (s C + c).  The mean-pooled form (is_flatten=False) averages the
    cells in fp32 and multiplies in fp32 for either compute dtype.
    Limits: input_dim a multiple of 8 (NotImplementedError) and at most MAX_CHANNELS; reg_dim + n_classes <= MAX_COLS (n_classes up to 25); at most MAX_HEAD_CELLS
    cells per RoI (7^3 fits); M >= 1 (more than MAX_HEAD_ROWS rows go through the kernels in slices of that many); fp32 device input of the constructor's
    channel count and, when flattening, its input_size (ValueError / TypeError); parameters on the host raise RuntimeError."""

    MAX_COLS, MAX_HEAD_CELLS, MAX_CHANNELS, MAX_HEAD_ROWS = ops.BOX_HEAD_MAX_COLS, ops.BOX_HEAD_MAX_CELLS, ops.BOX_HEAD_MAX_CHANNELS, ops.BOX_HEAD_MAX_ROWS

    def __init__(self, input_dim, block, n_classes, input_size, is_add_layer=False, is_rotated_bbox=False, is_flatten=True, compute_dtype: torch.dtype = torch.bfloat16):
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"compute_dtype must be bfloat16 or float32, got {compute_dtype}")
        size = tuple(int(v) for v in input_size)
        if len(size) != 3 or min(size) < 1:
            raise ValueError(f"FusedRCNN: input_size must be three sizes >= 1, got {input_size}")
        ops.box_head_limits("FusedRCNN", None, size[0] * size[1] * size[2], int(input_dim), 7 if is_rotated_bbox else 6, int(n_classes))
        super().__init__(input_dim, block, n_classes, input_size, is_add_layer, is_rotated_bbox, is_flatten)
        self.compute_dtype, self.input_size = compute_dtype, size
        self._pk = self._pk_key = self._wcat = self._anchor = None

    def _pack(self):
        if self.layer is not None:
            conv_layer.ensure_packed(self, list(self.parameters()), "FusedRCNN (HIP) needs its parameters on a HIP device: call .cuda() first (no CPU fallback)",
                                     lambda P: [conv_layer.register(P, f"c{k}", self.layer[2 * k], self.compute_dtype) for k in range(2)])
        S = self.flatten_size if self.is_flatten else 1
        dtype = self.compute_dtype if self.is_flatten else torch.float32
        w = self.RCNN_bbox_pred.weight
        if self._wcat is None or self._wcat.device != w.device:
            self._wcat = torch.empty((self.reg_dim + self.n_classes, S * self.in_planes), dtype=dtype, device=w.device)
            self._anchor = torch.zeros(1, device=w.device, requires_grad=True)
        ops.box_head_pack(w.detach(), self.RCNN_cls_score.weight.detach(), self.in_planes, S, dtype, out=self._wcat)

    def forward(self, pooling_feature):
        x = pooling_feature
        if not self.RCNN_bbox_pred.weight.is_cuda:
            raise RuntimeError("FusedRCNN (HIP) needs its parameters on a HIP device: call .cuda() first (no CPU fallback)")
        _check("FusedRCNN", x)
        if x.dim() != 5 or x.shape[0] < 1 or x.shape[1] != self.in_planes or (self.is_flatten and tuple(x.shape[2:]) != self.input_size):
            raise ValueError(f"FusedRCNN: pooling_feature must be (M >= 1, {self.in_planes}, {'ow, oh, od' if not self.is_flatten else ', '.join(map(str, self.input_size))}), "
                             f"got {tuple(x.shape)}")
        if x.shape[2] * x.shape[3] * x.shape[4] > self.MAX_HEAD_CELLS:
            raise ValueError(f"FusedRCNN supports at most {self.MAX_HEAD_CELLS} cells per RoI, got {tuple(x.shape[2:])}")
        self._pack()
        x = x.contiguous()
        M, step = x.shape[0], self.MAX_HEAD_ROWS
        if M <= step:
            return _FusedRCNNFn.apply(self._anchor, self, x)
        parts = [_FusedRCNNFn.apply(self._anchor, self, x[m0:m0 + step]) for m0 in range(0, M, step)]
        return torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])


# ---- losses and decode -----------------------------------------------------------------------------------------------------------------------
class _RoiHeadLoss(Function):
    @staticmethod
    def forward(ctx, ncols, scores, deltas, labels, rois, gt_rois):
        scores, deltas = scores.contiguous(), deltas.contiguous()
        scalars, targets = ops.roi_loss_fwd(ncols, scores, deltas, labels, rois, gt_rois)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(scores, deltas, labels, targets, scalars)
        ctx.ncols = ncols
        ctx.mark_non_differentiable(targets)
        return scalars[0], scalars[1], targets

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obj, g_reg, _):
        scores, deltas, labels, targets, scalars = ctx.saved_tensors
        if (g_obj is None and g_reg is None) or not any(ctx.needs_input_grad[1:3]):
            return (None,) * 6
        gs = [g if g is None else g.contiguous() for g in (g_obj, g_reg)]
        dscores, ddeltas = ops.roi_loss_bwd(ctx.ncols, scores, deltas, labels, targets, scalars, gs[0], gs[1])
        return (None, dscores, ddeltas, None, None, None)


def _rows(name, what, t, M, cols):
    _check(name, t)
    t = t.detach().reshape(-1, t.shape[-1]) if t.dim() > 1 else t.detach().reshape(-1)
    if t.shape[0] != M or (t.dim() == 2 and t.shape[1] not in cols):
        raise ValueError(f"{name}: {what} must have {M} rows and {' or '.join(str(c) for c in cols)} columns, got {tuple(t.shape)}")
    return t.contiguous()


def roi_head_loss(pred_scores, pred_bbox_deltas, labels, rois, gt_rois, return_targets=False):
    """pred_scores [M,n_classes], pred_bbox_deltas [M,6|7], labels [M] (or [N,R]) fp32, rois [M,6|7] or [M,1+6|7], gt_rois [M,6|7] ->
    {"loss_objectness": mean cross-entropy over rows with label >= 0, "loss_rpn_box_reg": smooth-L1 (beta 1/9) summed over rows with label > 0 / their count}
    (and the regression targets [M,6|7] with return_targets).  Gradients go to the two head outputs."""
    name = "roi_head_loss"
    _check(name, pred_scores, pred_bbox_deltas)
    if pred_scores.dim() != 2 or pred_bbox_deltas.dim() != 2 or pred_bbox_deltas.shape[1] not in (6, 7) or pred_scores.shape[0] != pred_bbox_deltas.shape[0]:
        raise ValueError(f"{name}: pred_scores [M, n_classes] and pred_bbox_deltas [M, 6|7], got {tuple(pred_scores.shape)}, {tuple(pred_bbox_deltas.shape)}")
    M, B = pred_bbox_deltas.shape
    if M < 1 or not 1 <= pred_scores.shape[1] <= MAX_CLASSES:
        raise ValueError(f"{name}: at least one row and 1 to {MAX_CLASSES} classes, got {M} rows, {pred_scores.shape[1]} classes")
    _check(name, labels)
    labels, rois, gt_rois = _rows(name, "labels", labels.reshape(-1), M, ()), _rows(name, "rois", rois, M, (B, B + 1)), _rows(name, "gt_rois", gt_rois, M, (B,))
    if labels.dim() != 1 or rois.dim() != 2 or gt_rois.dim() != 2:
        raise ValueError(f"{name}: labels [M], rois [M, {B}|{B + 1}], gt_rois [M, {B}]")
    obj, reg, targets = _RoiHeadLoss.apply(B, pred_scores, pred_bbox_deltas, labels, rois, gt_rois)
    loss = {"loss_objectness": obj, "loss_rpn_box_reg": reg}
    return (loss, targets) if return_targets else loss


def roi_decode(pred_bbox_deltas, rois):
    """pred_bbox_deltas [M,6|7], rois [M,6|7] or [M,1+6|7] -> boxes [M,6|7]: dw, dh, dd clipped at log 2000, the angle wrapped into (-pi/2, pi/2]; no gradient"""
    name = "roi_decode"
    _check(name, pred_bbox_deltas)
    if pred_bbox_deltas.dim() != 2 or pred_bbox_deltas.shape[1] not in (6, 7):
        raise ValueError(f"{name}: pred_bbox_deltas must be [M, 6|7], got {tuple(pred_bbox_deltas.shape)}")
    M, B = pred_bbox_deltas.shape
    rois = _rows(name, "rois", rois, M, (B, B + 1))
    with torch.no_grad():
        return ops.roi_decode(B, pred_bbox_deltas.detach().contiguous(), rois)


class RotatedCoder:
    """RotatedCoder of the reference: encode_single(gt_rois, ex_drois) and decode_single(deltas, ex_drois) on [M, 7] boxes; no gradient"""
    ncols = 7

    def __init__(self, bbox_xform_clip=math.log(2000.0)):
        if abs(bbox_xform_clip - math.log(2000.0)) > 1e-6:
            raise NotImplementedError("the decode kernel clips at log(2000), the only value the reference uses")
        self.bbox_xform_clip = bbox_xform_clip

    def encode_single(self, gt_rois, ex_rois):
        _check(type(self).__name__, gt_rois, ex_rois)
        M = gt_rois.shape[0]
        gt, ex = _rows("encode_single", "gt_rois", gt_rois, M, (self.ncols,)), _rows("encode_single", "ex_rois", ex_rois, M, (self.ncols,))
        # The encode is part of the loss forward, which writes the targets of every valid row (0 <= label < n_classes, roi_head.hip's header) and zeros
        # elsewhere: one score column and label 0 make every row valid.  If that rule changes, this must change with it; test_decode_clip_and_angle_wrap
        # compares the result with the restatement's encode.
        zeros = torch.zeros((M, self.ncols), dtype=torch.float32, device=gt.device)
        with torch.no_grad():
            return ops.roi_loss_fwd(self.ncols, zeros[:, :1].contiguous(), zeros, zeros[:, 0].contiguous(), ex, gt)[1]

    def decode_single(self, deltas, ex_rois):
        return roi_decode(deltas, ex_rois)


class AABBCoder(RotatedCoder):
    """AABBCoder of the reference on [M, 6] boxes"""
    ncols = 6


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
class Classification_Model(nn.Module):
    """The reference's constructor and forward(rois, gt_bboxes, gt_bbox_labels, features, is_sample, is_reg) ->
    ([per-scene RoIs (or, is_reg, decoded proposals), gt_labels], per-scene class probabilities, {"loss_objectness", "loss_rpn_box_reg"} (0 in evaluation)).
    rois: per scene [K, 1+6|7], or the dense triple (boxes, levels, counts) of rpn_proposals_dense.  features: one (N, C, W, H, D) map per level (or per-scene
    lists); with a feature_extractor, the per-scene raw grids [[grid], ...], which are zero-padded to a common size, stacked and run through it."""

    def __init__(self, feature_extractor, sample_model, pooling_model, RCNN_model, n_classes=2, is_training=True, batch_size=20, is_rotated_bbox=False):
        super().__init__()
        self.batch_size = batch_size
        self.feature_extractor, self.sample_model, self.pooling_model, self.RCNN_model = feature_extractor, sample_model, pooling_model, RCNN_model
        self.num_class = n_classes
        self.score_thresh = 0.7
        self.is_training, self.is_rotated_bbox = is_training, is_rotated_bbox
        self.reg_dim = 7 if is_rotated_bbox else 6
        self.box_coder = RotatedCoder() if is_rotated_bbox else AABBCoder()

    def transform(self, meshes):
        if len(meshes) > 1:
            target = np.max([m.shape for m in meshes], axis=0)
            meshes = [F.pad(m, (0, int(target[-1] - m.shape[-1]), 0, int(target[-2] - m.shape[-2]), 0, int(target[-3] - m.shape[-3]))) for m in meshes]
        return meshes

    def compute_loss(self, pred_scores, pred_bbox_deltas, gt_labels, rois, gt_rois):
        """as the reference's, but from the RoIs and their matched boxes: the encode is part of the fused loss"""
        return roi_head_loss(pred_scores, pred_bbox_deltas, gt_labels, rois, gt_rois)

    def forward(self, rois, gt_bboxes, gt_bbox_labels, features, is_sample=True, is_reg=False, keep=None, keep_counts=None):
        original_size = []
        if self.feature_extractor is not None:
            flat = self.transform([f[0] for f in features])
            original_size = [f.shape[1:] for f in flat]
            features = [f.to(torch.float32) for f in self.feature_extractor(torch.stack(flat, dim=0))]
        dense = isinstance(rois, tuple)
        if dense:
            boxes, levels, counts = rois
            ks = None
        else:
            boxes, levels, counts, ks = _pack("Classification_Model", rois, self.reg_dim)
        labels, sample_rois, gt_rois, _, _ = self.sample_model.forward_dense(boxes, levels, counts, gt_bboxes, gt_bbox_labels, is_sample, keep, keep_counts)
        N, R = labels.shape
        pooled = self.pooling_model(features, sample_rois, original_size)
        if self.pooling_model.is_rotated_bbox and not self.pooling_model.remap:           # the reference's enlarge_roi wrote into these (module header)
            sample_rois = torch.cat([sample_rois[..., :1], self.pooling_model.enlarge_roi(sample_rois[..., 1:])], -1)
        pred_bbox_deltas, pred_scores = self.RCNN_model(pooled)
        cls_prob = F.softmax(pred_scores, 1)
        flat_rois = sample_rois.reshape(N * R, -1)
        loss = 0.
        if is_sample:
            ks = [R] * N
            loss = roi_head_loss(pred_scores, pred_bbox_deltas, labels.reshape(-1), flat_rois, gt_rois.reshape(N * R, -1))
            gt_labels = labels
        else:
            if ks is None:
                ks = counts.tolist()                  # the one synchronisation
            gt_labels = [labels[i, :k] for i, k in enumerate(ks)]
        out_boxes = roi_decode(pred_bbox_deltas, flat_rois).reshape(N, R, -1) if is_reg else sample_rois[..., 1:]
        return [[out_boxes[i, :k] for i, k in enumerate(ks)], gt_labels], [cls_prob[i * R:i * R + k] for i, k in enumerate(ks)], loss

    HEAD_BLOCK = 256

    def _head_blocks(self, pooled):
        """RCNN_model over blocks of exactly HEAD_BLOCK rows, the last one zero-padded.  The box head is torch (nn.Linear, nn.Conv3d), whose libraries choose their
        kernel, and with it the order of a row's sums, by the shape of the whole call; with one fixed shape a row's logits and deltas do not depend on how many
        rows share its call, so predict_dense gives the same bits for every chunk_rows.  -> (pred_bbox_deltas, pred_scores)
        This rests on a property of the libraries' kernels that nothing guarantees: within a call of one shape, a row's result depends neither on its position
        nor on the other rows.  It held for the two Linear layers (is_add_layer off, is_flatten on) on the rocBLAS this was written against; the conv layers of
        is_add_layer and the mean-pooled head were not measured.  tests/test_two_stage_gpu.py::test_chunked_prediction_is_bit_identical is
        the check, and the place to look after a library update.  The price is one head call per 256 rows, about 0.8 ms at 2 x 2000 rows.
        A FusedRCNN needs none of this: a row's bits do not depend on the other rows of its call by construction, so it takes all rows at once."""
        if isinstance(self.RCNN_model, FusedRCNN):
            return self.RCNN_model(pooled)
        M, B = pooled.shape[0], self.HEAD_BLOCK
        deltas, scores = [], []
        for m0 in range(0, M, B):
            blk = pooled[m0:m0 + B]
            n = blk.shape[0]
            if n < B:
                blk = F.pad(blk, (0, 0) * (blk.dim() - 1) + (0, B - n))
            d, s = self.RCNN_model(blk)
            deltas.append(d[:n])
            scores.append(s[:n])
        return torch.cat(deltas), torch.cat(scores)

    def predict_dense(self, boxes, levels, counts, features, chunk_rows=None):
        """The evaluation forward without ground truth: pooling, then RCNN_model, for all N x R rows of the dense triple (boxes [N,R,6|7], levels [N,R] int32,
        counts [N] int32) of rpn_proposals_dense -> (pred_scores [N*R, n_classes] logits, pred_bbox_deltas [N*R, 6|7], rois_used [N*R, 1+6|7]: the RoIs the
        head's deltas refer to, enlarged for oriented boxes with remap off, as in forward).  Rows past counts are computed like any other (zero boxes pool to
        zeros); roi_postprocess_dense ignores them.  chunk_rows: the rows of every scene go through pooling and head chunk_rows at a time, which bounds the
        pooled tensor (the reference chunks by cls_batch_size); the loop is over fixed sizes and needs no host wait.  The head always runs in blocks of
        HEAD_BLOCK rows (_head_blocks), so the results are the same bits for every chunk_rows.  No gradient."""
        name = "Classification_Model.predict_dense"
        _check(name, boxes)
        if boxes.dim() != 3 or boxes.shape[2] != self.reg_dim:
            raise ValueError(f"{name}: boxes must be [N, R, {self.reg_dim}], got {tuple(boxes.shape)}")
        N, R, B = boxes.shape
        levels = _int32(name, "levels", levels, (N, R))
        _int32(name, "counts", counts, (N,))
        step = R if chunk_rows is None else int(chunk_rows)
        if step < 1:
            raise ValueError(f"{name}: chunk_rows must be at least 1, got {chunk_rows}")
        with torch.no_grad():
            original_size = []
            if self.feature_extractor is not None:
                flat = self.transform([f[0] for f in features])
                original_size = [f.shape[1:] for f in flat]
                features = [f.to(torch.float32) for f in self.feature_extractor(torch.stack(flat, dim=0))]
            rois = torch.cat([levels.to(torch.float32)[..., None], boxes.detach()], -1)
            scores, deltas = [], []
            for r0 in range(0, R, step):
                part = rois[:, r0:r0 + step].contiguous()
                d, s = self._head_blocks(self.pooling_model(features, part, original_size))
                scores.append(s.reshape(N, part.shape[1], -1))
                deltas.append(d.reshape(N, part.shape[1], -1))
            if self.pooling_model.is_rotated_bbox and not self.pooling_model.remap:
                rois = torch.cat([rois[..., :1], self.pooling_model.enlarge_roi(rois[..., 1:])], -1)
            return torch.cat(scores, 1).reshape(N * R, -1), torch.cat(deltas, 1).reshape(N * R, B), rois.reshape(N * R, 1 + B).contiguous()


# ---- post-processing of the second stage -------------------------------------------------------------------------------------------------------
POST_MAX_ROWS, POST_MASK_BYTES_MAX = ops.ROI_POST_MAX_ROWS, ops.ROI_POST_MASK_BYTES_MAX


def _mesh_sizes(name, mesh_sizes, N, dev):
    """a triple, a list of N triples, or an int32 device tensor [N, 3] -> int32 device tensor [N, 3] (a host list costs one small copy)"""
    if isinstance(mesh_sizes, torch.Tensor):
        if mesh_sizes.dtype != torch.int32 or tuple(mesh_sizes.shape) != (N, 3) or not mesh_sizes.is_cuda:
            raise ValueError(f"{name}: mesh_sizes must be a triple, a list of {N} triples or an int32 device tensor [{N}, 3]")
        return mesh_sizes.contiguous()
    rows = list(mesh_sizes)
    if len(rows) == 3 and not isinstance(rows[0], (list, tuple, torch.Size, np.ndarray)):
        rows = [rows] * N
    if len(rows) != N or any(len(r) != 3 for r in rows):
        raise ValueError(f"{name}: mesh_sizes must be a triple, a list of {N} triples or an int32 device tensor [{N}, 3]")
    if any(float(v) != int(v) for r in rows for v in r):    # the reference passes shape * spatial_scale, floats: int() would cut a size down silently
        raise ValueError(f"{name}: mesh_sizes must be whole numbers, got {rows}")
    return torch.tensor([[int(v) for v in r] for r in rows], dtype=torch.int32).to(dev, non_blocking=True)


def roi_postprocess_dense(pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes, score_thresh=0.5, nms_thresh=0.1, min_size=1e-3, is_reg=True, threshold_mode="any"):
    """Trainer.filter_proposals (run_rpn_detect.py:403-439) for all scenes at once, with the softmax and the decode of the evaluation forward in front of it.
    pred_scores [N*R, K] logits, pred_bbox_deltas [N*R, 6|7] (None without is_reg), rois [N*R, 1+6|7] (or the three with [N, R, ..]), counts [N] int32 device
    (clamped to 0 .. R), mesh_sizes: a triple, N triples or an int32 device tensor [N, 3] (use the tensor when capturing).
    -> (boxes [N, R, 6|7], scores [N, R], index [N, R] int32, counts [N] int32): scene i's results are rows 0 .. counts[i]-1 in descending score (equal scores:
    the lower row first), index the source row of each (gather gt_labels or anything else by it); rows past them are zero with index -1.
    threshold_mode "any" (the reference's reading): a row passes iff any class probability >= score_thresh; "object": iff p[1] does.  Semantics: the header of
    csrc/roi_post.hip.  Never waits for the host; capturable with torch.cuda.graph on one stream."""
    name = "roi_postprocess_dense"
    _check(name, pred_scores, rois)
    if threshold_mode not in ops.ROI_POST_MODES:
        raise ValueError(f"{name}: threshold_mode must be one of {sorted(ops.ROI_POST_MODES)}, got {threshold_mode!r}")
    if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or counts.dim() != 1 or not counts.is_cuda:
        raise ValueError(f"{name}: counts must be an int32 device tensor [N]")
    N = counts.shape[0]
    if not 1 <= N <= MAX_SCENES:
        raise ValueError(f"{name} supports 1 to {MAX_SCENES} scenes, got {N}")
    if rois.shape[-1] not in (7, 8):
        raise ValueError(f"{name}: rois must be [N*R, 1+6|7] (level, box), got {tuple(rois.shape)}")
    B, K = rois.shape[-1] - 1, pred_scores.shape[-1]
    M = rois.numel() // (1 + B)
    if M < N or M % N:
        raise ValueError(f"{name}: {M} rows do not divide into {N} scenes of at least one row")
    R = M // N
    if R > POST_MAX_ROWS:
        raise ValueError(f"{name} supports at most {POST_MAX_ROWS} rows per scene, got {R}")
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"{name} supports 2 to {MAX_CLASSES} classes, got {K}")
    if N * R * ((R + 63) // 64) * 8 > POST_MASK_BYTES_MAX:
        raise ValueError(f"{name}: the suppression workspace of {N} scenes x {R} rows exceeds {POST_MASK_BYTES_MAX} bytes; pass fewer scenes per call")
    if pred_scores.numel() != M * K:
        raise ValueError(f"{name}: pred_scores must have {M} rows, got {tuple(pred_scores.shape)}")
    deltas = None
    if is_reg:
        _check(name, pred_bbox_deltas)
        if pred_bbox_deltas.shape[-1] != B or pred_bbox_deltas.numel() != M * B:
            raise ValueError(f"{name}: pred_bbox_deltas must be [{M}, {B}], got {tuple(pred_bbox_deltas.shape)}")
        deltas = pred_bbox_deltas.detach().reshape(M, B).contiguous()
    with torch.no_grad():
        mesh = _mesh_sizes(name, mesh_sizes, N, rois.device)
        cand_boxes, cand_scores, keys = ops.roi_post_select(N, R, B, pred_scores.detach().reshape(M, K).contiguous(), deltas, rois.detach().reshape(M, 1 + B).contiguous(),
                                                            counts.contiguous(), mesh, float(score_thresh), float(min_size), bool(is_reg), ops.ROI_POST_MODES[threshold_mode])
        sorted_keys, order = torch.sort(keys, dim=1, descending=True, stable=True)        # dropped rows (key 0) sort last
        return ops.roi_post_nms(B, cand_boxes, cand_scores, sorted_keys, order, float(nms_thresh))


def filter_proposals(proposals, objectness, gt_labels, mesh_sizes, score_threhold=0.8, nms_thresh=0.1, min_size=1e-3, threshold_mode="any"):
    """Trainer.filter_proposals with the reference's name, argument order and spelling: per scene proposals [K, 6|7] (already decoded), objectness [K, n_classes]
    class PROBABILITIES, gt_labels [K] (anything per row, passed through), mesh_sizes per scene -> (final_boxes, final_scores [k, n_classes], final_gt_labels)
    per scene, in descending objectness[:, 1].  The kernel takes logits: log(objectness) is handed over with is_reg=False, and softmax(log p) = p for rows that
    sum to 1, as a softmax's do (a probability of 0 becomes -inf and comes back as 0).  One host wait, for the N counts."""
    name = "filter_proposals"
    N = len(proposals)
    if not (N == len(objectness) == len(gt_labels)) or N < 1:
        raise ValueError(f"{name}: one proposal, objectness and label tensor per scene")
    _check(name, *proposals, *objectness)
    B = proposals[0].shape[-1]
    boxes, levels, counts, ks = _pack(name, [F.pad(p.detach().reshape(-1, B), (1, 0)) for p in proposals], B)
    R = boxes.shape[1]
    logits = torch.stack([F.pad(torch.log(o.detach()), (0, 0, 0, R - k)) for o, k in zip(objectness, ks)])
    rois = torch.cat([levels.to(torch.float32)[..., None], boxes], -1)
    out_boxes, _, index, kept = roi_postprocess_dense(logits, None, rois, counts, mesh_sizes, score_threhold, nms_thresh, min_size, False, threshold_mode)
    kept = kept.tolist()                  # the one synchronisation
    rows = [index[i, :k].long() for i, k in enumerate(kept)]
    return [out_boxes[i, :k] for i, k in enumerate(kept)], [o[r] for o, r in zip(objectness, rows)], [g[r.to(g.device)] for g, r in zip(gt_labels, rows)]


# ---- the two stages joined ---------------------------------------------------------------------------------------------------------------------
class TwoStageDetector(nn.Module):
    """A NeRFRegionProposalNetwork and a Classification_Model(feature_extractor=None) on the same FPN features: the backbone runs once, rpn.proposals_dense
    hands its dense triple to the second stage, and in evaluation roi_postprocess_dense turns the head's outputs into detections (the reference runs the two
    stages as two programs, run_rpn.py and run_rpn_detect.py, with the proposals on disk between them).

    Training, forward(meshes, targets): {"loss_objectness", "loss_rpn_box_reg"} of the sampled second stage (all ground-truth labels 1, as
    run_rpn_detect.py:351); the first stage runs under no_grad unless train_rpn, in which case its three losses are added under "rpn_"-prefixed keys (its head
    then runs twice, once for the losses and once for the proposals).  The features carry gradient to the backbone through the pooling either way.
    keep / keep_counts replace the second stage's sampler (roi_targets_dense).
    Evaluation: detections_dense(meshes) -> (boxes [N,R,6|7], scores [N,R], counts [N] int32), what DetectionEvaluator.update takes, without a host wait;
    forward(meshes) -> (boxes, scores) as per-scene lists, with one host wait.  Boxes are clipped to, and oriented centres tested against, each scene's own
    size before padding.  state_dict: the parts' keys under rpn_network. and roi_model.RCNN_model.
    first_stage_no_grad = True (an attribute): the backbone runs under torch.no_grad() and its features are handed on detached, so the pooling sends nothing
    into it and the box head trains on fixed features (the reference's second stage without --fine_tune); without train_rpn the whole first stage then runs
    without a graph, with train_rpn the first stage's head still trains, on the detached features (trainer.TwoStageTrainer chooses)."""

    first_stage_no_grad = False

    def __init__(self, rpn_network, roi_model, score_thresh, nms_thresh, min_size=1e-3, is_reg=True, threshold_mode="any", train_rpn=False):
        super().__init__()
        if roi_model.feature_extractor is not None:
            raise ValueError("TwoStageDetector: the second stage must be a Classification_Model(feature_extractor=None); it reads the first stage's features")
        if threshold_mode not in ops.ROI_POST_MODES:
            raise ValueError(f"TwoStageDetector: threshold_mode must be one of {sorted(ops.ROI_POST_MODES)}, got {threshold_mode!r}")
        if bool(rpn_network.rpn.rotate) != bool(roi_model.is_rotated_bbox):
            raise ValueError("TwoStageDetector: both stages must use the same box form")
        self.rpn_network, self.roi_model = rpn_network, roi_model
        self.score_thresh, self.nms_thresh, self.min_size = score_thresh, nms_thresh, min_size
        self.is_reg, self.threshold_mode, self.train_rpn = is_reg, threshold_mode, train_rpn
        self.chunk_rows = None
        self._size_cache = {}
        if not train_rpn:                                  # the first stage's head gets no gradient: it is frozen, so that an optimizer's weight decay leaves it alone
            for p in rpn_network.rpn.parameters():
                p.requires_grad_(False)

    def _first_stage(self, meshes, targets=None):
        """-> (features, (boxes, levels, counts), sizes int32 device [N,3], the first stage's losses or {})"""
        net = self.rpn_network
        sizes = tuple(tuple(int(v) for v in m.shape[-3:]) for m in meshes)
        meshes, _ = net.transform(list(meshes))
        x = torch.stack(meshes, dim=0)
        key = (sizes, x.device)
        if key not in self._size_cache:                    # one host-to-device copy per distinct set of sizes
            self._size_cache[key] = torch.tensor(sizes, dtype=torch.int32, device=x.device)
        ori = self._size_cache[key]
        if self.first_stage_no_grad:
            with torch.no_grad():
                features = [f.detach() for f in net.backbone(x)]
        else:
            features = list(net.backbone(x))
        losses = {}
        if self.training and self.train_rpn:
            losses = net.rpn(x, features, ori, targets)[2]
        with torch.no_grad():
            boxes, _, levels, _, counts = net.rpn.proposals_dense(x, features, ori)
        return features, (boxes, levels, counts), ori, losses

    def detections_dense(self, meshes):
        with torch.no_grad():
            features, (boxes, levels, counts), sizes, _ = self._first_stage(meshes)
            pred_scores, pred_bbox_deltas, rois = self.roi_model.predict_dense(boxes, levels, counts, features, self.chunk_rows)
            out_boxes, scores, _, kept = roi_postprocess_dense(pred_scores, pred_bbox_deltas, rois, counts, sizes, self.score_thresh, self.nms_thresh, self.min_size, self.is_reg,
                                                               self.threshold_mode)
        return out_boxes, scores, kept

    def forward(self, meshes, targets=None, keep=None, keep_counts=None):
        if not self.training:
            boxes, scores, counts = self.detections_dense(meshes)
            counts = counts.tolist()              # the one synchronisation
            return [boxes[i, :k] for i, k in enumerate(counts)], [scores[i, :k] for i, k in enumerate(counts)]
        if targets is None:
            raise ValueError("TwoStageDetector: targets should not be None in training mode")
        features, dense, _, rpn_losses = self._first_stage(meshes, targets)
        gt_labels = [t.new_ones(t.shape[0]) for t in targets]
        losses = dict(self.roi_model(dense, targets, gt_labels, features, is_sample=True, keep=keep, keep_counts=keep_counts)[2])
        losses.update({"rpn_" + k: v for k, v in rpn_losses.items()})
        return losses
