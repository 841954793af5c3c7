"""Oriented 3-D box IoU / GIoU / DIoU losses, all-pairs IoU and rotated NMS on the HIP kernels of csrc/rotated_iou.hip, with the
reference's names, argument order and return tuples (the import swap is one line):

  cal_iou_3d, cal_giou_3d, cal_diou_3d   nerf_rpn/model/rotated_iou/oriented_iou_loss.py:82-148 (fcos/loss.py:135-171, rpn.py:143-156)
  box_iou_3d, nms, batched_nms           nerf_rpn/model/fcos/utils.py:109-158, 229-255 (and model/utils.py)

Boxes are fp32 (x, y, z, w, l, h, theta) with theta in RADIANS about the third axis (roi_align_rotated_3d of rotated.py takes degrees);
box_iou_3d / nms / batched_nms also take the 6-column axis-aligned form (x1, y1, z1, x2, y2, z2).  Semantics, the algorithm and the two
stated deviations from the reference (identical boxes give IoU >= 1 - 1e-4; no epsilon stabilisers) are in DESIGN.md 3.8.

The loss functions are one autograd.Function over one forward and one backward kernel: the backward recomputes the geometry from the boxes,
gradients go to whichever box tensor requires them, nothing is allocated beyond the outputs and the host never waits, so forward + backward can be captured
in a HIP graph (create the box leaves on the capture stream: DESIGN.md 3.8, Capture).  Other dtypes than fp32 raise TypeError.  There is no CPU path: CPU tensors raise RuntimeError."""
from __future__ import annotations

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops

NMS_MAX_BOXES = ops.OBB_NMS_MAX
_MODES = {("giou", "smallest"): ops.OBB_GIOU_SMALLEST, ("giou", "aligned"): ops.OBB_GIOU_ALIGNED,
          ("diou", "smallest"): ops.OBB_DIOU_SMALLEST, ("diou", "aligned"): ops.OBB_DIOU_ALIGNED}


def _check(name, *boxes, cols=(7,)):
    for b in boxes:
        if not isinstance(b, torch.Tensor) or b.dtype != torch.float32:
            raise TypeError(f"{name} takes fp32 box tensors, got {getattr(b, 'dtype', type(b))}")
        if not b.is_cuda:
            raise RuntimeError(f"{name} needs HIP device tensors (there is no CPU path)")
        if b.dim() < 2 or b.shape[-1] not in cols:
            raise ValueError(f"{name}: boxes must end in {' or '.join(map(str, cols))} columns, got shape {tuple(b.shape)}")


def _mode(kind, enclosing_type):
    if enclosing_type == "pca":
        raise NotImplementedError('enclosing_type "pca" is not built; use "smallest" or "aligned"')
    if (kind, enclosing_type) not in _MODES:
        raise ValueError(f'unknown enclosing_type {enclosing_type!r}; supported: "smallest", "aligned"')
    return _MODES[(kind, enclosing_type)]


class _ObbIoU(Function):
    """(box1, box2, mode, verbose) -> (iou, u3d, z_range, loss, corners1, corners2); iou, u3d and loss carry gradient"""

    @staticmethod
    def forward(ctx, box1, box2, mode, verbose):
        box1, box2 = box1.contiguous(), box2.contiguous()
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(box1, box2)
        ctx.mode = mode
        iou, u3d, zr, loss, c1, c2 = ops.obb_iou_fwd(mode, box1, box2, want_u3d=True, want_z_range=verbose, want_corners=verbose)
        ctx.mark_non_differentiable(*(t for t in (zr, c1, c2) if t is not None))
        return iou, u3d, zr, loss, c1, c2

    @staticmethod
    @once_differentiable
    def backward(ctx, g_iou, g_u3d, g_zr, g_loss, g_c1, g_c2):
        box1, box2 = ctx.saved_tensors
        need1, need2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # an expanded single value (the gradient of a sum()) is passed on as it is: ops.obb_iou_bwd reads it as one value, no copy
        gs = [g if g is None or all(s == 0 for s in g.stride()) else g.contiguous() for g in (g_iou, g_u3d, g_loss)]
        if all(g is None for g in gs):
            return None, None, None, None
        d1, d2 = ops.obb_iou_bwd(ctx.mode, box1, box2, gs[0], gs[1], gs[2], need1, need2)
        return d1, d2, None, None


def _paired(name, box3d1, box3d2, mode, verbose):
    _check(name, box3d1, box3d2)
    if box3d1.shape != box3d2.shape:
        raise ValueError(f"{name}: box tensors must have the same shape, got {tuple(box3d1.shape)} and {tuple(box3d2.shape)}")
    return _ObbIoU.apply(box3d1, box3d2, mode, verbose)


def cal_iou_3d(box3d1, box3d2, verbose=False):
    """(B,N,7) x2 -> iou (B,N); verbose: (iou, corners1 (B,N,4,2), corners2, z_range, u3d).  iou and u3d carry gradient; corners1, corners2
    and z_range come back WITHOUT gradient (every caller in the reference discards them)."""
    iou, u3d, zr, _, c1, c2 = _paired("cal_iou_3d", box3d1, box3d2, ops.OBB_IOU, bool(verbose))
    return (iou, c1, c2, zr, u3d) if verbose else iou


def cal_giou_3d(box3d1, box3d2, enclosing_type="smallest"):
    """-> (giou_loss, giou, iou3d), each (B,N); enclosing_type "smallest" or "aligned" ("pca" raises NotImplementedError)"""
    iou, _, _, loss, _, _ = _paired("cal_giou_3d", box3d1, box3d2, _mode("giou", enclosing_type), False)
    return loss, 1 - loss, iou


def cal_diou_3d(box3d1, box3d2, enclosing_type="smallest"):
    """-> (diou_loss, iou3d), each (B,N)"""
    iou, _, _, loss, _, _ = _paired("cal_diou_3d", box3d1, box3d2, _mode("diou", enclosing_type), False)
    return loss, iou


def box_iou_3d(boxes1, boxes2):
    """[N,7] x [M,7] oriented, or [N,6] x [M,6] axis-aligned (x1,y1,z1,x2,y2,z2) -> IoU [N,M] fp32 on the boxes' device.  The N x M x 7
    repeat of the reference is never formed, so no batching is needed.  No gradient."""
    _check("box_iou_3d", boxes1, boxes2, cols=(6, 7))
    if boxes1.dim() != 2 or boxes2.dim() != 2 or boxes1.shape[1] != boxes2.shape[1]:
        raise ValueError("box_iou_3d: boxes1 [N,C] and boxes2 [M,C] with the same C in (6, 7)")
    return ops.obb_iou_pairwise(boxes1.detach().contiguous(), boxes2.detach().contiguous())


def _nms(name, boxes, scores, idxs, iou_threshold):
    _check(name, boxes, cols=(6, 7))
    if boxes.dim() != 2 or scores.shape != boxes.shape[:1] or (idxs is not None and idxs.shape != scores.shape):
        raise ValueError(f"{name}: boxes [N,6|7], scores [N]" + (", idxs [N]" if idxs is not None else ""))
    n = boxes.shape[0]
    if n > NMS_MAX_BOXES:
        raise ValueError(f"{name} supports at most {NMS_MAX_BOXES} boxes (the suppression matrix takes N^2/8 bytes), got {n}")
    if n == 0:
        return torch.empty((0,), dtype=torch.int64, device=boxes.device)
    order = torch.sort(scores.to(boxes.device), descending=True, stable=True).indices
    cats = None if idxs is None else idxs.to(boxes.device)[order].to(torch.int32).contiguous()
    keep, count = ops.obb_nms(boxes.detach()[order].contiguous(), cats, float(iou_threshold))
    return order[keep[:int(count.item())].long()]          # the one synchronisation: the kept count sizes the result


def nms(boxes, scores, iou_threshold):
    """boxes [N,7] (or [N,6] axis-aligned) fp32, scores [N] -> int64 indices of the kept boxes in decreasing score, on the boxes' device.
    Order: stable descending sort of the scores (a tie goes to the lower index); a box is suppressed iff its IoU with a kept box is
    > iou_threshold.  At most NMS_MAX_BOXES = 16384 boxes (the bit matrix takes N^2/8 bytes: 32 MB there); more raise ValueError.
    The only host synchronisation is reading the kept count."""
    return _nms("nms", boxes, scores, None, iou_threshold)


def batched_nms(boxes, scores, idxs, iou_threshold):
    """nms within each category idxs [N] (integers); the kept indices of all categories merged, in decreasing score.  Same limits as nms."""
    return _nms("batched_nms", boxes, scores, idxs, iou_threshold)
