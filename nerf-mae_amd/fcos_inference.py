"""FCOS inference post-processing of the reference's 3-D detector head on the HIP kernels of csrc/fcos_post.hip, with the reference's name,
constructor, call and return form (the import swap is one line):

  FCOSPostProcessor          nerf_rpn/model/fcos/inference.py:11-195 (called from FCOSModule._forward_test, fcos/fcos.py:258-270)
  fcos_postprocess_dense     the same computation with fixed-size results and no host synchronisation, for HIP graphs

Head outputs are the per-level NCDHW tensors as the head writes them, (N, 1, w, l, h) logits, (N, 6|8, w, l, h) regression and (N, 1, w, l, h)
centerness, fp32, read in place (no permute, no cat).  `locations` (per level [n, 3] fp32) is honoured and read by the kernels: this
constructor has no strides, so locations are not re-derived.  `grid_sizes` is a list of (w, l, h) per scene or an int32 device tensor [N, 3]
(a host list costs one small copy); `padding_masks` is None or one bool tensor [N, n] per level.  Semantics: the header of csrc/fcos_post.hip
and DESIGN.md 3.10.  The outputs carry no gradient.

Three kernels and one torch.sort: selection (threshold, exact top-k, decode, clip, size filter, sqrt) for every (level, scene) in one launch,
the stable descending sort of the padded [N, cap] scores, one suppression-matrix launch and one scan launch for all scenes, the post-NMS cut in
the scan's epilogue.  fcos_postprocess_dense never waits for the host; FCOSPostProcessor.forward is that plus the slicing, and waits exactly
once, to read the N kept counts that size the results.

Stated deviations from the reference:
  - where topk(sorted=False) and argsort leave order and tie winners open, they are defined: the pre-NMS order is level-major, then ascending
    location index; a tie at a top-k cut goes to the lower location index; the NMS order is the stable descending sort of the scores (as
    rotated_iou.nms); the post-NMS cut keeps every box whose score is >= the fpn_post_nms_top_n-th largest kept score (the reference's
    kthvalue rule, ties included);
  - more than one class channel raises ValueError (the reference's own comment: "always one in RPN");
  - other dtypes than fp32 raise TypeError, CPU tensors RuntimeError, more than 4 levels or 64 scenes ValueError (as fcos_loss);
  - cap = sum over the levels of min(pre_nms_top_n, n_level) above rotated_iou.NMS_MAX_BOXES raises ValueError, and so does a suppression
    workspace (N cap^2 / 8 bytes) above MASK_BYTES_MAX = 1 GiB: lower pre_nms_top_n or pass fewer scenes per call;
  - the two identical-box and epsilon deviations of the IoU geometry apply to the NMS."""
from __future__ import annotations

import torch

from . import ops
from .fcos_loss import _check

MAX_LEVELS, MAX_SCENES = ops.FCOS_MAX_LEVELS, ops.FCOS_MAX_SCENES
NMS_MAX_BOXES = ops.OBB_NMS_MAX
MASK_BYTES_MAX = ops.FCOS_POST_MASK_BYTES_MAX


def _prepare(name, locations, box_cls, box_regression, centerness, grid_sizes, padding_masks, pre_nms_top_n, use_obb):
    L = len(box_cls)
    if L > MAX_LEVELS:
        raise ValueError(f"{name} supports at most {MAX_LEVELS} levels, got {L}")
    if L < 1 or len(box_regression) != L or len(centerness) != L or locations is None or len(locations) != L:
        raise ValueError(f"{name}: one tensor per level for locations, box_cls, box_regression and centerness")
    _check(name, *locations, *box_cls, *box_regression, *centerness)
    C = 8 if use_obb else 6
    N = box_cls[0].shape[0]
    if N > MAX_SCENES:
        raise ValueError(f"{name} supports at most {MAX_SCENES} scenes per call, got {N}")
    level_n = []
    for loc, c, r, t in zip(locations, box_cls, box_regression, centerness):
        if c.dim() != 5 or c.shape[0] != N:
            raise ValueError(f"{name}: box_cls must be (N, 1, w, l, h) per level, got {tuple(c.shape)}")
        if c.shape[1] != 1:
            raise ValueError(f"{name}: one class channel only (the reference's own comment: always one in RPN), got {c.shape[1]}")
        s, n = tuple(c.shape[2:]), c[0].numel()
        if tuple(r.shape) != (N, C, *s) or t.numel() != c.numel() or tuple(loc.shape) != (n, 3):
            raise ValueError(f"{name}: per level locations [n,3], box_regression (N,{C},w,l,h), centerness (N,1,w,l,h); got {tuple(loc.shape)}, {tuple(r.shape)}, {tuple(t.shape)}")
        level_n.append(n)
    plan = ops.FcosPostPlan(level_n, N, pre_nms_top_n)
    dev = box_cls[0].device
    masks = None
    if padding_masks is not None:
        masks = [m.contiguous() for m in padding_masks]
        if len(masks) != L or any(m.numel() != N * n or m.element_size() != 1 or not m.is_cuda for m, n in zip(masks, level_n)):
            raise ValueError(f"{name}: padding_masks must be one bool device tensor [N, n] per level")
    if grid_sizes is not None:
        if not isinstance(grid_sizes, torch.Tensor):
            grid_sizes = torch.tensor([[int(v) for v in g] for g in grid_sizes], dtype=torch.int32).to(dev, non_blocking=True)   # a host list costs a copy
        if grid_sizes.dtype != torch.int32 or tuple(grid_sizes.shape) != (N, 3) or not grid_sizes.is_cuda:
            raise ValueError(f"{name}: grid_sizes must be a list of N (w, l, h) or an int32 device tensor [N, 3]")
        grid_sizes = grid_sizes.contiguous()
    elif not use_obb:
        raise ValueError(f"{name}: grid_sizes is required for axis-aligned boxes (they are clipped to it)")
    heads = [[t.detach().contiguous() for t in ts] for ts in (box_cls, box_regression, centerness)]
    return plan, heads, [t.detach().contiguous() for t in locations], masks, grid_sizes


def fcos_postprocess_dense(locations, box_cls, box_regression, centerness, grid_sizes, padding_masks, pre_nms_thresh, pre_nms_top_n, nms_thresh, fpn_post_nms_top_n, min_size,
                           bbox_aug_enabled=False, use_obb=False):
    """-> (boxes [N, cap, 1+6|7], scores [N, cap], counts [N] int32), cap = sum over the levels of min(pre_nms_top_n, n_level); scene i's results
    are rows 0 .. counts[i]-1 (column 0 the level index, decreasing score), rows past them are zero.  Never waits for the host; capturable with
    torch.cuda.graph.  bbox_aug_enabled: the per-scene concatenation before NMS, level-major and in ascending location index."""
    name = "fcos_postprocess_dense"
    with torch.no_grad():
        plan, (cls, reg, ctr), locs, masks, sizes = _prepare(name, locations, box_cls, box_regression, centerness, grid_sizes, padding_masks, pre_nms_top_n, use_obb)
        ncols = 8 if use_obb else 6
        pre_boxes, pre_scores, pre_counts = ops.fcos_post_select(plan, ncols, cls, reg, ctr, locs, masks, sizes, float(pre_nms_thresh), float(min_size))
        if bbox_aug_enabled:
            empty = pre_scores < 0
            order = torch.sort(empty.to(torch.uint8), dim=1, stable=True).indices          # the filled slots first, in their order
            empty = torch.gather(empty, 1, order)
            boxes = torch.gather(pre_boxes, 1, order[:, :, None].expand(-1, -1, pre_boxes.shape[2])).masked_fill_(empty[:, :, None], 0.0)
            scores = torch.gather(pre_scores, 1, order).masked_fill_(empty, 0.0)
            return boxes, scores, pre_counts.sum(0, dtype=torch.int32)
        sorted_scores, order = torch.sort(pre_scores, dim=1, descending=True, stable=True)   # empty slots (-1) sort last
        return ops.fcos_post_nms(plan, ncols, pre_boxes, sorted_scores, order, pre_counts, float(nms_thresh), int(fpn_post_nms_top_n))


class FCOSPostProcessor(torch.nn.Module):
    """The reference's FCOSPostProcessor on the fused kernels: same constructor, same call, same (boxes, scores) lists."""

    def __init__(self, pre_nms_thresh, pre_nms_top_n, nms_thresh, fpn_post_nms_top_n, min_size, num_classes, bbox_aug_enabled=False, use_obb=False):
        super().__init__()
        self.pre_nms_thresh = pre_nms_thresh
        self.pre_nms_top_n = pre_nms_top_n
        self.nms_thresh = nms_thresh
        self.fpn_post_nms_top_n = fpn_post_nms_top_n
        self.min_size = min_size
        self.num_classes = num_classes        # unused, as in the reference
        self.bbox_aug_enabled = bbox_aug_enabled
        self.use_obb = use_obb

    def forward(self, locations, box_cls, box_regression, centerness, grid_sizes, padding_masks):
        """-> (boxes, scores): per scene boxes [K, 1+6|7] fp32 (column 0 the level index) and scores [K] in decreasing score (with
        bbox_aug_enabled: every level's boxes before NMS, level-major).  One host synchronisation: the N kept counts."""
        boxes, scores, counts = fcos_postprocess_dense(locations, box_cls, box_regression, centerness, grid_sizes, padding_masks, self.pre_nms_thresh, self.pre_nms_top_n,
                                                       self.nms_thresh, self.fpn_post_nms_top_n, self.min_size, self.bbox_aug_enabled, self.use_obb)
        counts = counts.tolist()                # the one synchronisation
        return [boxes[i, :k] for i, k in enumerate(counts)], [scores[i, :k] for i, k in enumerate(counts)]
