"""The reference's anchor-based 3-D region proposal network on the HIP kernels of csrc/rpn.hip (training path) and csrc/rpn_post.hip (inference path), with
the reference's names (the import swap is one line):

  AnchorGenerator3D            nerf_rpn/model/anchor.py:14-174 (same constructor, num_anchors_per_location, forward, get_padding_masks)
  rpn_assign_targets           RegionProposalNetwork.assign_targets_to_anchors + box_coder.encode (model/rpn.py:240-290, 524) over Matcher
                               (model/utils.py:98-211) and AABBCoder / MidpointOffsetCoder.encode_single (model/coder/)
  rpn_sample                   BalancedPositiveNegativeSampler (model/utils.py:35-95)
  RPNLossComputation           RegionProposalNetwork.compute_loss and the training half of forward (model/rpn.py:372-419, 514-534)
  rpn_decode_proposals         box_coder.decode_list (model/coder/base_bbox_coder.py:55-86) over AABBCoder / MidpointOffsetCoder.decode_single
  rpn_proposals_dense          _get_top_n_idx + filter_proposals (model/rpn.py:292-370) with fixed-size results and no host synchronisation, for HIP graphs
  RPNProposalFilter            the inference half of forward (model/rpn.py:507-512): per-scene lists (boxes, level_indexes, scores)

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
  - loss_rpn_box_reg_2d is returned as a constant zero without gradient: the reference weights it by --reg_loss_weight_2d, whose default is
    0.0 and which no launcher sets, so the total loss and every gradient are the reference's under its defaults;
  - reg_loss_type other than "smooth_l1" raises NotImplementedError (the IoU-type losses need the differentiable decode of the proposals);
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

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from .fcos_loss import _boxes, _check

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
    """(plan, C, flags, targets, *objectness levels, *regression levels) -> (loss_objectness, loss_rpn_box_reg)"""

    @staticmethod
    def forward(ctx, plan, C, flags, targets, *heads):
        heads = [h.contiguous() for h in heads]
        obj, reg = heads[:plan.L], heads[plan.L:]
        scalars = ops.rpn_loss_fwd(plan, C, obj, reg, flags, targets)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(flags, targets, scalars, *heads)
        ctx.cfg = (plan, C)
        return scalars[0], scalars[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_obj, g_reg):
        plan, C = ctx.cfg
        flags, targets, scalars, *heads = ctx.saved_tensors
        if (g_obj is None and g_reg is None) or not any(ctx.needs_input_grad[4:]):
            return (None,) * (4 + 2 * plan.L)
        gs = [g if g is None else g.contiguous() for g in (g_obj, g_reg)]
        dobj, dreg = ops.rpn_loss_bwd(plan, C, heads[:plan.L], heads[plan.L:], flags, targets, scalars, gs[0], gs[1])
        return (None, None, None, None, *dobj, *dreg)


class RPNLossComputation(object):
    """The training half of the reference's RegionProposalNetwork.forward on the fused kernels: assignment, sampling and the two losses.
    rng_state (int64 device tensor [2] = (seed, counter)) is created on the first call; copy into it to replay a draw."""

    def __init__(self, anchor_generator, fg_iou_thresh, bg_iou_thresh, batch_size_per_mesh, positive_fraction, rotated_bbox=False, reg_loss_type="smooth_l1", seed=0):
        if reg_loss_type != "smooth_l1":
            raise NotImplementedError(f'reg_loss_type {reg_loss_type!r} is not built; use "smooth_l1" (the IoU-type losses need the differentiable decode of the proposals)')
        if len(anchor_generator.sizes) > MAX_LEVELS:
            raise ValueError(f"RPNLossComputation supports at most {MAX_LEVELS} levels, got {len(anchor_generator.sizes)}")
        if bg_iou_thresh > fg_iou_thresh:
            raise ValueError("RPNLossComputation: bg_iou_thresh must not exceed fg_iou_thresh")
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
        sampler -> {"loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d"}, 0-dim fp32 device tensors"""
        name = "RPNLossComputation"
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
        labels, _, reg_targets = ops.rpn_assign(plan, boxes, offsets, ncols, ori, self.fg_iou_thresh, self.bg_iou_thresh)
        if sampled is None:
            if self.rng_state is None:
                self.rng_state = torch.tensor([self.seed, 0], dtype=torch.int64, device=boxes.device)
            flags, _ = ops.rpn_sample(labels, self.batch_size_per_mesh, int(self.batch_size_per_mesh * self.positive_fraction), self.rng_state)
        else:
            if not isinstance(sampled, torch.Tensor) or sampled.dtype != torch.uint8 or tuple(sampled.shape) != (N, plan.n) or not sampled.is_cuda:
                raise ValueError(f"{name}: sampled must be a uint8 device tensor [N, n] = {(N, plan.n)}")
            flags = sampled.contiguous()
        loss_obj, loss_reg = _RpnLoss.apply(plan, C, flags, reg_targets, *objectness, *pred_bbox_deltas)
        return {"loss_objectness": loss_obj, "loss_rpn_box_reg": loss_reg, "loss_rpn_box_reg_2d": torch.zeros((), dtype=torch.float32, device=boxes.device)}


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
