"""The reference's anchor-based 3-D region proposal network on the HIP kernels of csrc/rpn.hip (training path) and csrc/rpn_post.hip (inference path), with
the reference's names (the import swap is one line):

  AnchorGenerator3D            nerf_rpn/model/anchor.py:14-174 (same constructor, num_anchors_per_location, forward, get_padding_masks)
  rpn_assign_targets           RegionProposalNetwork.assign_targets_to_anchors + box_coder.encode (model/rpn.py:240-290, 524) over Matcher
                               (model/utils.py:98-211) and AABBCoder / MidpointOffsetCoder.encode_single (model/coder/)
  rpn_sample                   BalancedPositiveNegativeSampler (model/utils.py:35-95)
  RPNLossComputation           RegionProposalNetwork.compute_loss and the training half of forward (model/rpn.py:372-419, 514-534), reg_loss_type "smooth_l1"
  RPNIoULossComputation        the same with reg_loss_type "iou" | "linear_iou" | "giou" | "diou": RotatedIOULoss over the decoded proposals of the sampled
                               positives (model/rpn.py:133-164, 214-217, 400-417, 518-520), oriented boxes only
  rpn_decode_proposals         box_coder.decode_list (model/coder/base_bbox_coder.py:55-86) over AABBCoder / MidpointOffsetCoder.decode_single
  rpn_proposals_dense          _get_top_n_idx + filter_proposals (model/rpn.py:292-370) with fixed-size results and no host synchronisation, for HIP graphs
  RPNProposalFilter            the inference half of forward (model/rpn.py:507-512): per-scene lists (boxes, level_indexes, scores)
  RPNHead                      model/anchor.py:177-213 on the channels-last convolutions and the output kernels of csrc/rpn_head.hip (same constructor, state_dict
                               keys, shapes and initialisation; compute_dtype is an addition)
  RegionProposalNetwork        model/rpn.py:167-549: head + RPNLossComputation (training) or RPNProposalFilter (evaluation); same constructor, state_dict keys
                               head.* only; proposals_dense() is the capturable hand-over to the RoI stage
  NeRFRegionProposalNetwork    model/nerf_rpn.py: backbone + RegionProposalNetwork, zero padding to the batch maximum, the degenerate-box check

Head outputs are the per-level tensors as the head writes them, (N, A, W, H, D) objectness logits and (N, A*6|8, W, H, D) regression (channel
a*C + c), fp32; they are read and differentiated in place (no permute, no cat).  Ground-truth boxes are one fp32 device tensor per scene, [k, 6]
(x0,y0,z0,x1,y1,z1) or [k, 7] (x,y,z,w,l,h,theta in radians).  Per-anchor results are [N, n] over every scene's concatenated levels, anchor
((w*H + h)*D + d)*A + a within a level: the order of the reference's concatenated anchors.  The kernels never read an anchor tensor: they derive
every anchor from its index, the per-axis strides mesh_size // grid_size and the base table, which is built here on the host with the
reference's arithmetic.  Semantics: the headers of csrc/rpn.hip and csrc/rpn_post.hip, DESIGN.md 3.11 and 3.12.

Nothing waits for the host and every sum has a fixed order, so assignment + sampling + loss forward + backward can be captured with
torch.cuda.graph (create the leaves on the capture stream: DESIGN.md 3.8, Capture); the sampler's counter lives on the device and advances
inside the graph, so every replay draws a fresh sample.  rpn_proposals_dense is capturable in the same way; RPNProposalFilter waits exactly once, to
read the N counts that size its lists.

Stated deviations from the reference, training path:
  - the sampler does not reproduce torch.randperm's stream: a candidate's key is a hash of (seed, counter, scene, anchor index) and the num_pos /
    num_neg smallest keys are taken (uniform without replacement; equal keys at the cut go to the lower anchor index);
  - equal IoU of one anchor with several boxes goes to the lowest box index (torch.max leaves it open);
  - loss_rpn_box_reg_2d, the 2-D projection loss (model/rpn.py:421-453), is opt-in: with the trailing keyword reg_loss_2d=True of the two loss classes and
    the two networks it is the reference's value, with its gradient, from the same fused forward and the same single backward launch (csrc/rpn.hip, 2-D
    projection term; csrc/proj2d.hpp).  By default it stays a constant zero without gradient and the kernels without the term run: the reference weights
    it by --reg_loss_weight_2d, whose default is 0.0 and which no launcher sets, so the default costs nothing and gives the reference's total loss and
    gradients.  The weighting stays in the step, as in run_rpn.py:386-387: FinetuneStep(weights={"loss_rpn_box_reg_2d": w2d}).  Without a sampled positive
    it is 0 (the reference gives NaN); a sampled positive without a box row or in the padding (only `sampled=` can produce one) contributes nothing;
  - the IoU-type losses are a class of their own, RPNIoULossComputation, which RegionProposalNetwork builds for rotated_bbox=True and a reg_loss_type other
    than "smooth_l1"; RPNLossComputation itself raises NotImplementedError for them, and so does either network with rotated_bbox=False (the reference
    fails there too: its rotated_iou_loss is None).  An unknown reg_loss_type raises ValueError with rotated_bbox=True;
  - only the sampled positives are decoded for the IoU-type losses (the reference decodes every anchor and reads those); the backward of the decode is
    written by hand, with the conventions stated at rpn_decode_obb_bwd (csrc/rpn_decode.hpp); a sampled positive in a scene without boxes or in the padding,
    which only `sampled=` can produce, contributes nothing;
  - a scene without boxes has labels 0 (-1 in the padding) and all-zero targets (the reference takes log(0) there; nothing reads them);
  - without any sampled anchor both losses are 0 with zero gradients (the reference gives NaN);
  - other dtypes than fp32 raise TypeError, CPU tensors RuntimeError, more than 4 levels, 64 scenes or 32 anchors per location ValueError.
Stated deviations, inference path:
  - where topk and argsort leave tie winners and order open, they are defined on the fp32 bits of the logits (-0 below +0): a tie at a level's top-k
    cut goes to the anchor that lies first in the objectness tensor's memory, (a, w, h, d) order; the pre-NMS slots are level-major, then that memory
    order; the NMS order and the order of the results is descending logit, ties to the lower slot; a NaN logit is read as -inf;
  - a masked anchor (padding) orders below every logit, is still selected when a level has fewer unmasked anchors than the cut, and then has score
    exactly 0, as in the reference (sigmoid(-inf) = 0 and 0 >= score_thresh at the default 0.0);
  - the oriented centre filter drops the box together with its score and level.  The reference's clip_boxes_to_mesh shortens only `boxes`, so its
    later indexing pairs boxes with the wrong scores whenever a centre is outside; this module takes the aligned reading;
  - the two identical-box and epsilon deviations of the IoU geometry apply to the NMS;
  - cap = sum over the levels of min(pre_nms_top_n, anchors of the level) above rotated_iou.NMS_MAX_BOXES raises ValueError, and so does a
    suppression workspace above MASK_BYTES_MAX = 1 GiB: lower pre_nms_top_n or pass fewer scenes per call; post_nms_top_n < 1 raises ValueError."""
from __future__ import annotations

import itertools

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import conv_layer, ops, proj2d
from .fcos_loss import _boxes, _check
from .fpn import _NCDHWToCL, check_channels_last
from .model import _gradbuf

MAX_LEVELS, MAX_SCENES, MAX_ANCHORS = ops.FCOS_MAX_LEVELS, ops.FCOS_MAX_SCENES, ops.RPN_MAX_ANCHORS
NMS_MAX_BOXES = ops.OBB_NMS_MAX
MASK_BYTES_MAX = ops.FCOS_POST_MASK_BYTES_MAX


class AnchorGenerator3D(nn.Module):
    """sizes: one tuple of anchor sizes per level; aspect_ratios: one tuple of (x, y, z) ratio triples per level.  Every distinct permutation of
    a triple times every size is one base anchor.  The anchor index follows the iteration order of set(itertools.permutations(ratio)), which
    the same Python expression reproduces here (tuples of numbers hash the same in every process)."""

    def __init__(self, sizes, aspect_ratios, is_normalized=False):
        super().__init__()
        self.sizes = sizes
        self.aspect_ratios = aspect_ratios
        self.is_normalized = is_normalized
        self.aspect_ratios_unique = []
        for level in self.aspect_ratios:
            seen = set()
            for ratio in level:
                seen.update(set(itertools.permutations(ratio)))
            self.aspect_ratios_unique.append(list(seen))
        self.cell_anchors = None

    def num_anchors_per_location(self):
        return [len(s) * len(a) for s, a in zip(self.sizes, self.aspect_ratios_unique)]

    def generate_anchors(self, scales, xyz_ratios, dtype=torch.float32, device="cpu"):
        """-> [A, 6] base anchors (-w, -h, -d, w, h, d) / 2, rounded half to even, permutation-major and size-minor"""
        scales = torch.as_tensor(scales, dtype=dtype, device=device)
        cols = ([], [], [])
        for ratio in xyz_ratios:
            P = torch.tensor(list(set(itertools.permutations(ratio))))
            if self.is_normalized:
                weight = torch.tensor(1.)
                for i in range(3):
                    weight *= ratio[i]
                P = P / torch.pow(weight, 1. / 3.)
            for c in range(3):
                cols[c].append(P[:, c])
        ws, hs, ds = [(torch.cat(c, dim=0).to(device)[:, None] * scales[None, :]).view(-1) for c in cols]
        return (torch.stack([-ws, -hs, -ds, ws, hs, ds], dim=1) / 2).round()

    def set_cell_anchors(self, dtype, device):
        self.cell_anchors = [self.generate_anchors(s, a, dtype, device) for s, a in zip(self.sizes, self.aspect_ratios)]

    def half_extents(self):
        """per level, the host list [A][3] the kernels take: the base table is symmetric, (-e, e)"""
        out = []
        for s, a in zip(self.sizes, self.aspect_ratios):
            t = self.generate_anchors(s, a, torch.float32, "cpu")
            if not torch.equal(t[:, :3], -t[:, 3:]) or not bool((t[:, 3:] > 0).all()):
                raise ValueError("AnchorGenerator3D: a base anchor has a side that rounds to zero")
            out.append(t[:, 3:].tolist())
        return out

    @staticmethod
    def strides(mesh_size, grid_sizes):
        return [tuple(int(m) // int(g) for m, g in zip(mesh_size, grid)) for grid in grid_sizes]

    def grid_anchors(self, grid_sizes, strides):
        anchors = []
        for size, stride, base in zip(grid_sizes, strides, self.cell_anchors):
            dev = base.device
            sh = [torch.arange(0, int(g), dtype=torch.float32, device=dev) * int(s) for g, s in zip(size, stride)]
            x, y, z = [t.reshape(-1) for t in torch.meshgrid(sh[0], sh[1], sh[2], indexing="ij")]
            shifts = torch.stack((x, y, z, x, y, z), dim=1)
            anchors.append((shifts.view(-1, 1, 6) + base.view(1, -1, 6)).reshape(-1, 6))
        return anchors

    def get_padding_masks(self, meshes, feature_maps, ori_sizes):
        """-> per level a bool (N, A, W, H, D): True where the anchor's grid index is below ceil(ori_size / stride) on every axis"""
        grid_sizes = [tuple(f.shape[-3:]) for f in feature_maps]
        device = feature_maps[0].device
        masks = []
        for size, stride, A in zip(grid_sizes, self.strides(meshes.shape[-3:], grid_sizes), self.num_anchors_per_location()):
            level = []
            for ori in ori_sizes:
                lim = [-(-int(o) // s) for o, s in zip(ori, stride)]
                m = torch.zeros((A, *size), dtype=torch.bool, device=device)
                m[:, :lim[0], :lim[1], :lim[2]] = True
                level.append(m)
            masks.append(torch.stack(level, dim=0))
        return masks

    def forward(self, meshes, feature_maps):
        """-> (anchors: per scene the [n, 6] anchors of all levels, non_cat_anchors: per scene the per-level list); for users and tests, the kernels do
        not read them"""
        grid_sizes = [tuple(f.shape[-3:]) for f in feature_maps]
        self.set_cell_anchors(feature_maps[0].dtype, feature_maps[0].device)
        per_level = self.grid_anchors(grid_sizes, self.strides(meshes.shape[-3:], grid_sizes))
        non_cat = [list(per_level) for _ in range(meshes.shape[0])]
        return [torch.cat(a) for a in non_cat], non_cat


def _plan(anchor_generator, mesh_size, grid_sizes, N, name):
    grid_sizes = [tuple(int(v) for v in g) for g in grid_sizes]
    if len(grid_sizes) > MAX_LEVELS:
        raise ValueError(f"{name} supports at most {MAX_LEVELS} levels, got {len(grid_sizes)}")
    if N > MAX_SCENES:
        raise ValueError(f"{name} supports at most {MAX_SCENES} scenes, got {N}")
    if len(grid_sizes) != len(anchor_generator.sizes):
        raise ValueError(f"{name}: {len(grid_sizes)} levels but anchor sizes for {len(anchor_generator.sizes)}")
    key = (tuple(int(m) for m in mesh_size[-3:]), tuple(grid_sizes), N)
    cache = anchor_generator.__dict__.setdefault("_plans", {})
    if key not in cache:
        cache[key] = ops.RpnPlan(grid_sizes, anchor_generator.strides(key[0], grid_sizes), anchor_generator.half_extents(), N)
    return cache[key]


def _ori(name, ori_sizes, N, device):
    if ori_sizes is None:
        return None
    if not isinstance(ori_sizes, torch.Tensor):
        ori_sizes = torch.tensor([[int(v) for v in o] for o in ori_sizes], dtype=torch.int32, device=device)      # a host list costs a copy; pass a device tensor
    if ori_sizes.dtype != torch.int32 or tuple(ori_sizes.shape) != (N, 3) or not ori_sizes.is_cuda:
        raise ValueError(f"{name}: ori_sizes must be an int32 device tensor [N, 3] or a list of N triples")
    return ori_sizes.contiguous()


def rpn_assign_targets(anchor_generator, mesh_size, grid_sizes, targets, ori_sizes=None, fg_iou_thresh=0.35, bg_iou_thresh=0.2, rotated=False):
    """mesh_size (X, Y, Z), grid_sizes [(W, H, D)] per level, targets: list of per-scene fp32 device boxes [k, 6] or (rotated) [k, 7]; ori_sizes: the
    scenes' sizes before padding (list of triples or int32 device tensor [N, 3]), None: no padding mask ->
    (labels [N, n] fp32 in {1, 0, -1}, matched_idxs [N, n] int32 (box index, -1 below bg_iou_thresh, -2 between the thresholds),
    regression_targets [N, n, 6|8] fp32: the encode of box max(matched_idxs, 0))"""
    name = "rpn_assign_targets"
    ncols = 7 if rotated else 6
    boxes, offsets = _boxes(name, targets, ncols)
    plan = _plan(anchor_generator, mesh_size, grid_sizes, len(targets), name)
    return ops.rpn_assign(plan, boxes, offsets, ncols, _ori(name, ori_sizes, plan.N, boxes.device), float(fg_iou_thresh), float(bg_iou_thresh))


def rpn_sample(labels, batch_size_per_mesh, positive_fraction, rng_state):
    """labels [N, n] fp32 (>= 1 positive, 0 negative, else ignored); rng_state: int64 device tensor [2] = (seed, counter), the counter advances by
    one -> (flags [N, n] uint8: 0 unsampled, 1 positive, 2 negative; counts [N, 2] int32 = (num_pos, num_neg))"""
    _check("rpn_sample", labels)
    if labels.dim() != 2 or labels.shape[0] > MAX_SCENES:
        raise ValueError(f"rpn_sample: labels [N, n] with at most {MAX_SCENES} scenes, got {tuple(labels.shape)}")
    if not isinstance(rng_state, torch.Tensor) or rng_state.dtype != torch.int64 or tuple(rng_state.shape) != (2,) or not rng_state.is_cuda:
        raise ValueError("rpn_sample: rng_state must be an int64 device tensor [2] = (seed, counter)")
    batch = int(batch_size_per_mesh)
    return ops.rpn_sample(labels.contiguous(), batch, int(batch * positive_fraction), rng_state)


class _RpnLoss(Function):
    """(plan, C, loss_type or None (smooth-L1), cams or None (without the 2-D projection term), res, flags, targets, boxes, offsets, ori, matched_idxs, *objectness levels,
    *regression levels) -> (loss_objectness, loss_rpn_box_reg) and, with cams, loss_rpn_box_reg_2d: one forward and one backward launch for either box loss"""

    @staticmethod
    def forward(ctx, plan, C, loss_type, cams, res, flags, targets, boxes, offsets, ori, midx, *heads):
        heads = [h.contiguous() for h in heads]
        scalars = ops.rpn_loss_fwd(plan, C, loss_type, heads[:plan.L], heads[plan.L:], flags, targets, boxes, offsets, ori, midx, cams, res)
        ctx.set_materialize_grads(False)
        if cams is None:                         # kept alive until the backward: only what this variant's kernel reads
            targets, boxes, midx = (targets, None, None) if loss_type is None else (None, boxes, midx)
        ctx.save_for_backward(flags, targets, boxes, midx, scalars, *heads)
        ctx.cfg = (plan, C, loss_type, cams, res, offsets, ori)
        return (scalars[0], scalars[1]) if cams is None else (scalars[0], scalars[1], scalars[3])

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        plan, C, loss_type, cams, res, offsets, ori = ctx.cfg
        flags, targets, boxes, midx, scalars, *heads = ctx.saved_tensors
        if all(g is None for g in gs) or not any(ctx.needs_input_grad[11:]):
            return (None,) * (11 + 2 * plan.L)
        gs = [g if g is None else g.contiguous() for g in gs]
        dobj, dreg = ops.rpn_loss_bwd(plan, C, loss_type, heads[:plan.L], heads[plan.L:], flags, targets, boxes, offsets, ori, midx, cams, res, scalars, *gs)
        return (None,) * 11 + (*dobj, *dreg)


class _RPNLossBase(object):
    """What the two loss classes share: the checks, assignment and sampling (one seed draws the same sample in either), and the result's three keys.
    rng_state (int64 device tensor [2] = (seed, counter)) is created on the first call; copy into it to replay a draw."""

    def __init__(self, anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, rotated_bbox, reg_loss_type, seed, reg_loss_2d=False):
        self.name = type(self).__name__
        self.reg_loss_2d = bool(reg_loss_2d)
        if len(anchor_generator.sizes) > MAX_LEVELS:
            raise ValueError(f"{self.name} supports at most {MAX_LEVELS} levels, got {len(anchor_generator.sizes)}")
        if bg_iou_thresh > fg_iou_thresh:
            raise ValueError(f"{self.name}: bg_iou_thresh must not exceed fg_iou_thresh")
        self.anchor_generator = anchor_generator
        self.fg_iou_thresh, self.bg_iou_thresh = float(fg_iou_thresh), float(bg_iou_thresh)
        self.batch_size_per_mesh, self.positive_fraction = int(batch_size_per_mesh), float(positive_fraction)
        self.rotate = bool(rotated_bbox)
        self.reg_loss_type = reg_loss_type
        self.seed = int(seed)
        self.rng_state = None

    def __call__(self, mesh_size, objectness, pred_bbox_deltas, targets, original_mesh_sizes=None, sampled=None):
        """mesh_size (X, Y, Z) of the padded batch; objectness, pred_bbox_deltas: the head's per-level lists; targets: list of N box tensors;
        original_mesh_sizes: the scenes' sizes before padding, used as the reference does, only when N > 1; sampled: flags [N, n] uint8 in place of the
        sampler -> {"loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d"}, 0-dim fp32 device tensors (the last a constant zero unless reg_loss_2d)"""
        name = self.name
        L = len(objectness)
        if L > MAX_LEVELS:
            raise ValueError(f"{name} supports at most {MAX_LEVELS} levels, got {L}")
        if len(pred_bbox_deltas) != L:
            raise ValueError(f"{name}: one objectness and one regression tensor per level")
        _check(name, *objectness, *pred_bbox_deltas)
        C, ncols = (8, 7) if self.rotate else (6, 6)
        N = objectness[0].shape[0]
        if N > MAX_SCENES:
            raise ValueError(f"{name} supports at most {MAX_SCENES} scenes, got {N}")
        if len(targets) != N:
            raise ValueError(f"{name}: {N} scenes but {len(targets)} box tensors")
        grid_sizes = [tuple(o.shape[2:]) for o in objectness]
        plan = _plan(self.anchor_generator, mesh_size, grid_sizes, N, name)
        for o, r, g, A in zip(objectness, pred_bbox_deltas, grid_sizes, plan.A):
            if o.dim() != 5 or tuple(o.shape) != (N, A, *g) or tuple(r.shape) != (N, A * C, *g):
                raise ValueError(f"{name}: per level objectness (N,{A},W,H,D) and pred_bbox_deltas (N,{A * C},W,H,D); got {tuple(o.shape)}, {tuple(r.shape)}")
        boxes, offsets = _boxes(name, targets, ncols)
        ori = _ori(name, original_mesh_sizes if N > 1 else None, N, boxes.device)
        labels, matched_idxs, reg_targets = ops.rpn_assign(plan, boxes, offsets, ncols, ori, self.fg_iou_thresh, self.bg_iou_thresh)
        if sampled is None:
            if self.rng_state is None:
                self.rng_state = torch.tensor([self.seed, 0], dtype=torch.int64, device=boxes.device)
            flags, _ = ops.rpn_sample(labels, self.batch_size_per_mesh, int(self.batch_size_per_mesh * self.positive_fraction), self.rng_state)
        else:
            if not isinstance(sampled, torch.Tensor) or sampled.dtype != torch.uint8 or tuple(sampled.shape) != (N, plan.n) or not sampled.is_cuda:
                raise ValueError(f"{name}: sampled must be a uint8 device tensor [N, n] = {(N, plan.n)}")
            flags = sampled.contiguous()
        heads = (*objectness, *pred_bbox_deltas)
        loss_type = None if self.reg_loss_type == "smooth_l1" else self.reg_loss_type
        if self.reg_loss_2d:                     # the cameras stand around a scene of max(mesh_size), which is also the divisor
            res = float(max(int(m) for m in mesh_size[-3:]))
            loss_obj, loss_reg, loss_2d = _RpnLoss.apply(plan, C, loss_type, proj2d._cams(res), res, flags, reg_targets, boxes, offsets, ori, matched_idxs, *heads)
        else:
            loss_obj, loss_reg = _RpnLoss.apply(plan, C, loss_type, None, None, flags, reg_targets, boxes, offsets, ori, matched_idxs, *heads)
            loss_2d = torch.zeros((), dtype=torch.float32, device=boxes.device)
        return {"loss_objectness": loss_obj, "loss_rpn_box_reg": loss_reg, "loss_rpn_box_reg_2d": loss_2d}


class RPNLossComputation(_RPNLossBase):
    """The training half of the reference's RegionProposalNetwork.forward on the fused kernels: assignment, sampling, the objectness loss and the
    smooth-L1 box loss on the encoded targets."""

    def __init__(self, anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, rotated_bbox=False, reg_loss_type="smooth_l1", seed=0,
                 reg_loss_2d=False):
        if reg_loss_type != "smooth_l1":
            raise NotImplementedError(f'RPNLossComputation computes reg_loss_type "smooth_l1" only, got {reg_loss_type!r}; the IoU-type losses of oriented boxes '
                                      "are RPNIoULossComputation")
        super().__init__(anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, rotated_bbox, reg_loss_type, seed, reg_loss_2d)


class RPNIoULossComputation(_RPNLossBase):
    """The same training half with the reference's IoU-type box losses (run_rpn.py --rotated_bbox --reg_loss_type iou | linear_iou | giou | diou): the box
    term is RotatedIOULoss between the decoded proposal of every sampled positive and its matched box, differentiated through the decode (csrc/rpn.hip, IoU-type
    box losses).  Always oriented: 8 regression columns, [k, 7] boxes.  Same call, same keys, same sampler as RPNLossComputation."""

    def __init__(self, anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, reg_loss_type="iou", seed=0, reg_loss_2d=False):
        if reg_loss_type not in ops.FCOS_LOSS_TYPES:
            raise ValueError(f"RPNIoULossComputation: reg_loss_type must be one of {sorted(ops.FCOS_LOSS_TYPES)}, got {reg_loss_type!r}")
        super().__init__(anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, True, reg_loss_type, seed, reg_loss_2d)


# ---- inference path --------------------------------------------------------------------------------------------------------------------------
def _heads(name, anchor_generator, mesh_size, objectness, pred_bbox_deltas, C):
    """the checks shared by the inference entries -> (plan, detached contiguous objectness or None, regression)"""
    L = len(pred_bbox_deltas)
    if L > MAX_LEVELS:
        raise ValueError(f"{name} supports at most {MAX_LEVELS} levels, got {L}")
    if L < 1 or (objectness is not None and len(objectness) != L):
        raise ValueError(f"{name}: one objectness and one regression tensor per level")
    _check(name, *(objectness or ()), *pred_bbox_deltas)
    N = pred_bbox_deltas[0].shape[0]
    if N > MAX_SCENES:
        raise ValueError(f"{name} supports at most {MAX_SCENES} scenes, got {N}")
    if any(r.dim() != 5 for r in pred_bbox_deltas):
        raise ValueError(f"{name}: pred_bbox_deltas must be (N, A*{C}, W, H, D) per level")
    grid_sizes = [tuple(r.shape[2:]) for r in pred_bbox_deltas]
    plan = _plan(anchor_generator, mesh_size, grid_sizes, N, name)
    for k, (r, g, A) in enumerate(zip(pred_bbox_deltas, grid_sizes, plan.A)):
        if tuple(r.shape) != (N, A * C, *g) or (objectness is not None and tuple(objectness[k].shape) != (N, A, *g)):
            raise ValueError(f"{name}: per level objectness (N,{A},W,H,D) and pred_bbox_deltas (N,{A * C},W,H,D); got "
                             f"{tuple(objectness[k].shape) if objectness is not None else None}, {tuple(r.shape)}")
    obj = None if objectness is None else [t.detach().contiguous() for t in objectness]
    return plan, obj, [t.detach().contiguous() for t in pred_bbox_deltas]


def rpn_decode_proposals(anchor_generator, mesh_size, pred_bbox_deltas, rotated=False):
    """the unclipped decode of every anchor -> [N, n, 6] (x0,y0,z0,x1,y1,z1) or (rotated) [N, n, 7] (x,y,z,w,h,d,theta), anchor order; no gradient"""
    C = 8 if rotated else 6
    with torch.no_grad():
        plan, _, reg = _heads("rpn_decode_proposals", anchor_generator, mesh_size, None, pred_bbox_deltas, C)
        return ops.rpn_decode(plan, C, reg)


def _select(name, anchor_generator, mesh_size, objectness, pred_bbox_deltas, original_mesh_sizes, pre_nms_top_n, score_thresh, min_size, rotated):
    C = 8 if rotated else 6
    plan, obj, reg = _heads(name, anchor_generator, mesh_size, objectness, pred_bbox_deltas, C)
    post = plan.__dict__.setdefault("_post", {}).get(int(pre_nms_top_n))
    if post is None:
        post = plan._post[int(pre_nms_top_n)] = ops.RpnPostPlan(plan, pre_nms_top_n)
    ori = _ori(name, original_mesh_sizes, plan.N, obj[0].device)
    return post, C, ops.rpn_post_select(post, C, obj, reg, ori, [int(m) for m in mesh_size[-3:]], float(score_thresh), float(min_size))


def rpn_proposals_dense(anchor_generator, mesh_size, objectness, pred_bbox_deltas, original_mesh_sizes, pre_nms_top_n, post_nms_top_n, nms_thresh, score_thresh=0.0,
                        min_size=1e-3, rotated=False):
    """original_mesh_sizes: list of N triples, an int32 device tensor [N, 3] (a host list costs one small copy) or None (no padding mask) ->
    (boxes [N, cap, 6|7], scores [N, cap], levels [N, cap] int32, anchor_index [N, cap] int32, counts [N] int32), cap = sum over the levels of
    min(pre_nms_top_n, anchors of the level); scene i's proposals are rows 0 .. counts[i]-1 in descending score, rows past them are zero.  Never waits for
    the host; capturable with torch.cuda.graph."""
    name = "rpn_proposals_dense"
    if int(post_nms_top_n) < 1:
        raise ValueError(f"{name}: post_nms_top_n >= 1, got {post_nms_top_n}")
    with torch.no_grad():
        post, C, (keys, pre_boxes, pre_scores, pre_index, pre_counts) = _select(name, anchor_generator, mesh_size, objectness, pred_bbox_deltas, original_mesh_sizes, pre_nms_top_n,
                                                                                score_thresh, min_size, rotated)
        sorted_keys, order = torch.sort(keys, dim=1, descending=True, stable=True)      # level-major, descending logit, ties to the lower slot, empty slots of a level last
        return ops.rpn_post_nms(post, C, pre_boxes, pre_scores, pre_index, sorted_keys, order, pre_counts, float(nms_thresh), int(post_nms_top_n))


class RPNProposalFilter(object):
    """The inference half of the reference's RegionProposalNetwork.forward on the fused kernels: decode of the selected anchors, top-k per level,
    clip / centre / size / score filters, NMS within each level and the post-NMS cut."""

    def __init__(self, anchor_generator, pre_nms_top_n, post_nms_top_n, nms_thresh, score_thresh=0.0, rotated_bbox=False):
        if len(anchor_generator.sizes) > MAX_LEVELS:
            raise ValueError(f"RPNProposalFilter supports at most {MAX_LEVELS} levels, got {len(anchor_generator.sizes)}")
        if int(pre_nms_top_n) < 1 or int(post_nms_top_n) < 1:
            raise ValueError("RPNProposalFilter: pre_nms_top_n and post_nms_top_n >= 1")
        self.anchor_generator = anchor_generator
        self.pre_nms_top_n, self.post_nms_top_n = int(pre_nms_top_n), int(post_nms_top_n)
        self.nms_thresh, self.score_thresh = float(nms_thresh), float(score_thresh)
        self.rotate = bool(rotated_bbox)
        self.min_size = 1e-3            # fixed by the reference (rpn.py:219)

    def __call__(self, mesh_size, objectness, pred_bbox_deltas, original_mesh_sizes=None):
        """mesh_size (X, Y, Z) of the padded batch; objectness, pred_bbox_deltas: the head's per-level lists; original_mesh_sizes: the scenes' sizes before
        padding, used as the reference does, only when N > 1 -> (boxes, level_indexes, scores): per scene [K, 6|7] fp32, [K] int64 and [K] fp32 in decreasing
        score.  One host synchronisation: the N counts."""
        N = objectness[0].shape[0] if len(objectness) else 0
        boxes, scores, levels, _, counts = rpn_proposals_dense(self.anchor_generator, mesh_size, objectness, pred_bbox_deltas, original_mesh_sizes if N > 1 else None,
                                                               self.pre_nms_top_n, self.post_nms_top_n, self.nms_thresh, self.score_thresh, self.min_size, self.rotate)
        counts = counts.tolist()                # the one synchronisation
        return ([boxes[i, :k] for i, k in enumerate(counts)], [levels[i, :k].long() for i, k in enumerate(counts)], [scores[i, :k] for i, k in enumerate(counts)])


# ---- head and network ------------------------------------------------------------------------------------------------------------------------
class _RPNHeadFn(Function):
    """(anchor, head, *channels-last features) -> (*objectness levels, *regression levels): the 3x3x3 convs with ReLU on channels-last tensors, then the output
    kernel that writes the fp32 NCDHW planes.  The parameters are not autograd inputs: their gradients are accumulated into .grad by the kernels (as in
    fpn._FPNFn).  anchor is the head's one-element leaf that requires a gradient (as detector._FusedRCNNFn's): with it the outputs carry a graph, and the
    backward runs, also when no feature needs a gradient (a head trained on a frozen backbone's detached features); it receives none, and the first conv's
    input gradient is then not formed.  Saved per level: the input of every conv (rectified in place) and the last conv's output before its ReLU."""

    @staticmethod
    def forward(ctx, anchor, head, *feats):
        pk, depth, C = head._pk, head.conv_depth, head.num_delta_digits
        acts = []
        for f in feats:
            xs = [f.contiguous()]
            for k in range(depth):
                y = conv_layer.forward(pk, f"c{k}", head.conv[2 * k], xs[-1])
                if k < depth - 1:               # the last conv's ReLU is fused into the output kernel's load
                    ops.relu_(y)
                xs.append(y)
            acts.append(xs)
        obj, reg = ops.rpn_head_out_fwd([xs[-1] for xs in acts], pk["cls.w"], pk["box.w"], head.cls_logits.bias, head.bbox_pred.bias, C, depth > 0)
        ctx.head, ctx.saved = head, acts
        return (*obj, *reg)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        head, acts = ctx.head, ctx.saved
        pk, depth, C, L = head._pk, head.conv_depth, head.num_delta_digits, len(ctx.saved)
        g_obj, g_reg = [g.contiguous() for g in gs[:L]], [g.contiguous() for g in gs[L:]]
        cls, box = head.cls_logits, head.bbox_pred
        dts = ops.rpn_head_out_bwd([xs[-1] for xs in acts], pk["cls.w"], pk["box.w"], g_obj, g_reg, C, depth > 0, _gradbuf(cls.weight), _gradbuf(box.weight),
                                   _gradbuf(cls.bias), _gradbuf(box.bias))
        dfeats, keep = [], []   # keep: tensors the forked side stream still reads -- referenced until the join
        for i, (xs, dy) in enumerate(zip(acts, dts)):
            for k in range(depth - 1, -1, -1):
                if k < depth - 1:
                    ops.relu_bwd_(dy, xs[k + 1])
                keep.append(dy)
                dy = conv_layer.backward(pk, f"c{k}", head.conv[2 * k], dy, xs[k], need_dx=k > 0 or ctx.needs_input_grad[2 + i])
            dfeats.append(dy)
        ops.join_side()
        del keep
        return (None, None, *dfeats)


class RPNHead(nn.Module):
    """model/anchor.py:177-213.  Parameters live in `nn.Conv3d` holders (`conv` = Sequential of Conv3d, ReLU pairs; `cls_logits`; `bbox_pred`) so that names,
    shapes and the initialisation (normal 0.01, zero bias) equal the reference's; their forward is never used.  conv_depth 0 is legal (the features are then
    not rectified).  Outputs per level: objectness (N, A, W, H, D) and pred_bbox_deltas (N, A*6|8, W, H, D), fp32."""

    def __init__(self, in_channels, num_anchors, conv_depth=1, rotate=False, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if in_channels % 8:
            raise NotImplementedError("channel counts must be multiples of 8")
        if not 1 <= int(num_anchors) <= MAX_ANCHORS:
            raise ValueError(f"RPNHead supports 1 to {MAX_ANCHORS} anchors per location, got {num_anchors}")
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"compute_dtype must be bfloat16 or float32, got {compute_dtype}")
        self.in_channels, self.num_anchors, self.conv_depth = int(in_channels), int(num_anchors), int(conv_depth)
        self.num_delta_digits = 8 if rotate else 6
        self.compute_dtype = compute_dtype
        convs = []
        for _ in range(self.conv_depth):
            convs.append(nn.Conv3d(in_channels, in_channels, kernel_size=3, padding=1))
            convs.append(nn.ReLU(inplace=True))
        self.conv = nn.Sequential(*convs)
        self.cls_logits = nn.Conv3d(in_channels, num_anchors, kernel_size=1, stride=1)
        self.bbox_pred = nn.Conv3d(in_channels, num_anchors * self.num_delta_digits, kernel_size=1, stride=1)
        for layer in self.modules():
            if isinstance(layer, nn.Conv3d):
                torch.nn.init.normal_(layer.weight, std=0.01)
                torch.nn.init.constant_(layer.bias, 0)
        self._pk = None
        self._pk_key = None
        self._anchor = None

    def _pack(self):
        def fill(P):
            for k in range(self.conv_depth):
                conv_layer.register(P, f"c{k}", self.conv[2 * k], self.compute_dtype)
            P.add("cls.w", self.cls_logits.weight, P.CAST)
            P.add("box.w", self.bbox_pred.weight, P.CAST)

        conv_layer.ensure_packed(self, list(self.parameters()), "RPNHead (HIP) needs its parameters on a HIP device: call .cuda() first (no CPU fallback)", fill)
        dev = self.cls_logits.weight.device
        if self._anchor is None or self._anchor.device != dev:
            self._anchor = torch.zeros(1, device=dev, requires_grad=True)

    def forward_channels_last(self, feats):
        """feats: per level a channels-last (N, W, H, D, C) tensor in the compute dtype -> (logits, bbox_reg), lists of fp32 NCDHW tensors"""
        feats = list(feats)
        if not 1 <= len(feats) <= MAX_LEVELS:
            raise ValueError(f"RPNHead supports 1 to {MAX_LEVELS} levels, got {len(feats)}")
        check_channels_last("RPNHead", "W, H, D", feats, self.in_channels, self.compute_dtype)
        self._pack()
        out = _RPNHeadFn.apply(self._anchor, self, *feats)
        return list(out[:len(feats)]), list(out[len(feats):])

    def forward(self, x):
        """reference signature: list of NCDHW tensors -> (logits, bbox_reg)"""
        return self.forward_channels_last([_NCDHWToCL.apply(f, self.compute_dtype) for f in x])


class RegionProposalNetwork(nn.Module):
    """model/rpn.py:167-549 with the reference's constructor.  Training: the losses of RPNLossComputation, no proposals; evaluation: the lists of
    RPNProposalFilter and {}.  The only registered submodules are anchor_generator (no parameters) and head, so the state_dict keys are head.*."""

    def __init__(self, anchor_generator, head, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, pre_nms_top_n, post_nms_top_n, nms_thresh,
                 score_thresh=0.0, iou_batch_size=16, rotated_bbox=False, reg_loss_type="smooth_l1", reg_loss_2d=False):
        super().__init__()
        self.anchor_generator = anchor_generator
        self.head = head
        self.rotate = bool(rotated_bbox)
        self.num_bbox_digits = 7 if rotated_bbox else 6
        self.num_delta_digits = 8 if rotated_bbox else 6
        self.iou_batch_size = iou_batch_size        # kept for the signature: the assignment kernel needs no batching
        self._pre_nms_top_n = pre_nms_top_n
        self._post_nms_top_n = post_nms_top_n
        self.nms_thresh = nms_thresh
        self.score_thresh = score_thresh
        self.reg_loss_type = reg_loss_type
        self.min_size = 1e-3
        if rotated_bbox and reg_loss_type != "smooth_l1":
            self.loss = RPNIoULossComputation(anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, reg_loss_type, reg_loss_2d=reg_loss_2d)
        else:           # an IoU type without rotated_bbox raises NotImplementedError here: the reference has no such loss either (its rotated_iou_loss is None)
            self.loss = RPNLossComputation(anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, rotated_bbox, reg_loss_type,
                                           reg_loss_2d=reg_loss_2d)
        self.filters = {mode: RPNProposalFilter(anchor_generator, pre_nms_top_n[mode], post_nms_top_n[mode], nms_thresh, score_thresh, rotated_bbox)
                        for mode in ("training", "testing")}

    def pre_nms_top_n(self):
        return self._pre_nms_top_n["training" if self.training else "testing"]

    def post_nms_top_n(self):
        return self._post_nms_top_n["training" if self.training else "testing"]

    def _filter(self):
        return self.filters["training" if self.training else "testing"]

    def forward(self, meshes, features, original_mesh_sizes, targets=None, objectness_output_paths=None, sampled=None):
        """meshes (N, C, X, Y, Z): only its size is read; features: per level NCDHW; original_mesh_sizes: the scenes' sizes before padding, used only when N > 1;
        sampled: uint8 flags [N, n] in place of the sampler (RPNLossComputation) -> (boxes, level_indexes, losses, scores)"""
        objectness, pred_bbox_deltas = self.head(features)
        if objectness_output_paths is not None:
            self.output_objectness(objectness, original_mesh_sizes, objectness_output_paths)
        mesh_size = tuple(int(v) for v in meshes.shape[-3:])
        if self.training:
            if targets is None:
                raise ValueError("targets should not be None")
            return None, None, self.loss(mesh_size, objectness, pred_bbox_deltas, targets, original_mesh_sizes, sampled=sampled), None
        boxes, level_indexes, scores = self._filter()(mesh_size, objectness, pred_bbox_deltas, original_mesh_sizes)
        return boxes, level_indexes, {}, scores

    def proposals_dense(self, meshes, features, original_mesh_sizes=None):
        """the proposals of the current mode's top-n as rpn_proposals_dense's fixed-size quintuple (boxes, scores, levels, anchor_index, counts): never waits
        for the host, capturable (pass original_mesh_sizes as an int32 device tensor [N, 3] then)"""
        objectness, pred_bbox_deltas = self.head(features)
        f = self._filter()
        N = objectness[0].shape[0]
        return rpn_proposals_dense(self.anchor_generator, tuple(int(v) for v in meshes.shape[-3:]), objectness, pred_bbox_deltas, original_mesh_sizes if N > 1 else None,
                                   f.pre_nms_top_n, f.post_nms_top_n, f.nms_thresh, f.score_thresh, f.min_size, f.rotate)

    def output_objectness(self, objectness, ori_sizes, output_paths):
        """model/rpn.py:538-549, in plain torch as the reference has it"""
        for i in range(len(ori_sizes)):
            all_levels = {}
            for level in range(len(objectness)):
                score = objectness[level][i].max(dim=0)[0]
                w, l, h = np.ceil(np.array([int(v) for v in ori_sizes[i]]) / 2 ** (level + 2)).astype(int)
                all_levels[str(level)] = score[:w, :l, :h].detach().cpu().numpy()
            np.savez_compressed(output_paths[i], **all_levels)


def _default_anchorgen():
    anchor_sizes = ((8,), (16,), (32,), (64,),)
    aspect_ratios = (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * len(anchor_sizes)
    return AnchorGenerator3D(anchor_sizes, aspect_ratios)


class NeRFRegionProposalNetwork(nn.Module):
    """model/nerf_rpn.py: backbone + RegionProposalNetwork over a list of (C, W, H, D) grids -> [features, proposals, level_index], losses, scores.
    With rpn_head=None the head is RPNHead(out_channels, A, rotated_bbox) as in the reference, so the flag lands in conv_depth (depth 0 or 1, always 6 regression
    columns).  check_targets = False skips the degenerate-box check, the one place that waits for the host in training (for graph capture).
    backbone_no_grad = True (an attribute, the constructor is the reference's): the backbone runs under torch.no_grad() and its features are handed on
    detached, so nothing of it is kept for a backward and the head skips the gradient of its input: a frozen backbone (run_rpn.py --freeze_backbone,
    trainer.RPNTrainer(freeze_backbone=True))."""

    backbone_no_grad = False

    def __init__(self, backbone, rpn_anchor_generator=None, rpn_head=None, rpn_pre_nms_top_n_train=2000, rpn_pre_nms_top_n_test=1000, rpn_post_nms_top_n_train=2000,
                 rpn_post_nms_top_n_test=1000, rpn_nms_thresh=0.7, rpn_fg_iou_thresh=0.7, rpn_bg_iou_thresh=0.3, rpn_batch_size_per_image=256, rpn_positive_fraction=0.5,
                 rpn_score_thresh=0.0, iou_batch_size=16, rotated_bbox=False, reg_loss_type="smooth_l1", reg_loss_2d=False, **kwargs):
        if not hasattr(backbone, "out_channels"):
            raise ValueError("backbone should contain an attribute out_channels specifying the number of output channels (assumed to be the same for all the levels)")
        if not isinstance(rpn_anchor_generator, (AnchorGenerator3D, type(None))):
            raise TypeError(f"rpn_anchor_generator should be of type AnchorGenerator or None instead of {type(rpn_anchor_generator)}")
        out_channels = backbone.out_channels
        if rpn_anchor_generator is None:
            rpn_anchor_generator = _default_anchorgen()
        if rpn_head is None:
            rpn_head = RPNHead(out_channels, rpn_anchor_generator.num_anchors_per_location()[0], rotated_bbox)      # the reference's quirk: the flag is conv_depth
        rpn = RegionProposalNetwork(rpn_anchor_generator, rpn_head, rpn_fg_iou_thresh, rpn_bg_iou_thresh, rpn_batch_size_per_image, rpn_positive_fraction,
                                    dict(training=rpn_pre_nms_top_n_train, testing=rpn_pre_nms_top_n_test),
                                    dict(training=rpn_post_nms_top_n_train, testing=rpn_post_nms_top_n_test), rpn_nms_thresh, score_thresh=rpn_score_thresh,
                                    iou_batch_size=iou_batch_size, rotated_bbox=rotated_bbox, reg_loss_type=reg_loss_type, reg_loss_2d=reg_loss_2d)
        super().__init__()
        self.backbone = backbone
        self.rpn = rpn
        self.check_targets = True
        self._ori_cache = {}

    def transform(self, meshes, targets=None):
        """zero padding to the batch maximum (in place in the list, as the reference does)"""
        if len(meshes) > 1:
            target_shape = np.max([m.shape for m in meshes], axis=0)
            for i, mesh in enumerate(meshes):
                meshes[i] = F.pad(mesh, (0, int(target_shape[-1] - mesh.shape[-1]), 0, int(target_shape[-2] - mesh.shape[-2]), 0, int(target_shape[-3] - mesh.shape[-3])),
                                  mode="constant", value=0)
        return meshes, targets

    def check_bbox_degeneration(self, targets):
        if targets is not None:
            for target_idx, boxes in enumerate(targets):
                degenerate_boxes = boxes[:, 3:] <= boxes[:, :3] if boxes.shape[1] == 6 else boxes[:, 3:6] <= 0
                if degenerate_boxes.any():
                    bb_idx = torch.where(degenerate_boxes.any(dim=1))[0][0]
                    torch._assert(False, "All bounding boxes should have positive height, width and depth."
                                         f" Found invalid box {boxes[bb_idx].tolist()} for target at index {target_idx}.")

    def forward(self, meshes, targets=None, objectness_output_paths=None):
        if self.training:
            if targets is None:
                torch._assert(False, "targets should not be none when in training mode")
            for boxes in targets:
                if isinstance(boxes, torch.Tensor):
                    torch._assert(len(boxes.shape) == 2 and boxes.shape[-1] in (6, 7), f"Expected target boxes to be a tensor of shape [N, 6], got {boxes.shape}.")
                else:
                    torch._assert(False, f"Expected target boxes to be of type Tensor, got {type(boxes)}.")
        original_mesh_sizes = []
        for mesh in meshes:
            val = mesh.shape[-3:]
            torch._assert(len(val) == 3, f"expecting the last three dimensions of the Tensor to be W, H and D instead got {mesh.shape[-3:]}")
            original_mesh_sizes.append((val[0], val[1], val[2]))
        meshes, targets = self.transform(meshes, targets)
        if self.check_targets:
            self.check_bbox_degeneration(targets)
        mesh_tensors = torch.stack(meshes, dim=0)
        features = self._features(mesh_tensors)
        ori = original_mesh_sizes
        if len(meshes) > 1 and objectness_output_paths is None:      # one host-to-device copy per distinct set of sizes, none afterwards (nothing waits for the host)
            ori = self._ori_tensor(ori, mesh_tensors.device)
        proposals, level_index, proposal_losses, scores = self.rpn(mesh_tensors, features, ori, targets, objectness_output_paths)
        return [features, proposals, level_index], proposal_losses, scores

    def _features(self, mesh_tensors):
        if not self.backbone_no_grad:
            return list(self.backbone(mesh_tensors))
        with torch.no_grad():
            return [f.detach() for f in self.backbone(mesh_tensors)]

    def _ori_tensor(self, ori, device):
        key = (tuple(tuple(int(v) for v in o) for o in ori), device)
        if key not in self._ori_cache:
            self._ori_cache[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
        return self._ori_cache[key]

    def proposals_dense(self, meshes):
        """the list of (C, W, H, D) grids -> rpn.proposals_dense's fixed-size quintuple (boxes, scores, levels, anchor_index, counts) of the current mode's
        top-n: padding, backbone and head as in forward, no gradient, no host wait once the sizes' tensor exists (what DetectionEvaluator.update takes in its
        dense form)"""
        with torch.no_grad():
            meshes = list(meshes)
            ori = [tuple(int(v) for v in m.shape[-3:]) for m in meshes]
            meshes, _ = self.transform(meshes)
            x = torch.stack(meshes, dim=0)
            return self.rpn.proposals_dense(x, list(self.backbone(x)), self._ori_tensor(ori, x.device) if len(meshes) > 1 else None)
