"""The 2-D projection regression term of the reference's two detectors on the HIP kernels of csrc/proj2d.hip (device code: csrc/proj2d.hpp):

  proj2d_cameras(res)      get_w2cs(res) (nerf_rpn/model/rpn.py:58-85, identical in fcos/utils.py:300-353) times the intrinsics of rpn.py:422-423
  proj2d_points(boxes)     the two opposite corners that are projected: a box's own (6 columns) or obb2points_3d (fcos/utils.py:373-379, 7 columns)
  proj2d_terms(pred, target, res)
                           per row, the sum over four cameras, two points and two pixel coordinates of smooth_l1(uv_pred - uv_target; beta 1/9):
                           compute_2d_projection_loss (rpn.py:421-453, fcos/loss.py:447-475) before any weighting and normalisation

The fused losses apply the same device code to their decoded positives: RPNLossComputation / RPNIoULossComputation(reg_loss_2d=True) (rpn.py) and
FCOSProj2dLossComputation (fcos_loss.py); this module is the per-operator face, and what the operator tests measure against float64.  Boxes are fp32
device tensors [n, 6] (x0,y0,z0,x1,y1,z1) or [n, 7] (x,y,z,w,l,h,theta in radians).  proj2d_terms is differentiable in `pred`; `target` gets no gradient.
A camera is handed to the kernels as ONE 3x4 matrix K [R|t], formed in float64 on the host and rounded to fp32 once (the reference rounds w2c to fp32
and multiplies by K in fp32).  As in the reference there is no clamp and no sign test on the depth.  Other dtypes than fp32 raise TypeError, CPU tensors
RuntimeError (as fcos_loss._check)."""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops
from .fcos_loss import _check

INTRINSICS = ((600.0, 0.0, 320.0), (0.0, 600.0, 240.0), (0.0, 0.0, 1.0))
_CAMS = {}


def proj2d_cameras(res):
    """-> fp32 host tensor [4, 3, 4]: K w2c[:3] of the four cameras at c + (+-res, +-res, res), c = (res/2,)*3, looking at c with up = (0, 0, 1);
    built in float64, cached per res"""
    res = float(res)
    if not res > 0:
        raise ValueError(f"proj2d_cameras: res > 0, got {res}")
    if res not in _CAMS:
        c, up, K = np.full(3, res / 2), np.array([0.0, 0.0, 1.0]), np.array(INTRINSICS)
        out = []
        for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
            pos = c + np.array([sx * res, sy * res, res])
            z = (pos - c) / np.linalg.norm(pos - c)
            x = np.cross(up, z)
            x /= np.linalg.norm(x)
            y = np.cross(z, x)
            y /= np.linalg.norm(y)
            c2w = np.eye(4)
            c2w[:3, :3], c2w[:3, 3] = np.stack([x, y, z], 1), pos
            out.append(K @ np.linalg.inv(c2w)[:3])
        _CAMS[res] = (torch.from_numpy(np.stack(out)).float(), ops._cams48(torch.from_numpy(np.stack(out)).float()))
    return _CAMS[res][0].clone()


def _cams(res):
    proj2d_cameras(res)
    return _CAMS[float(res)][1]


def _rows(name, *boxes):
    _check(name, *boxes)
    shape = tuple(boxes[0].shape)
    if len(shape) != 2 or shape[1] not in (6, 7) or any(tuple(b.shape) != shape for b in boxes):
        raise ValueError(f"{name}: boxes must be [n, 6] or [n, 7], the same for prediction and target; got {[tuple(b.shape) for b in boxes]}")


def proj2d_points(boxes):
    """boxes [n, 6|7] -> [2, n, 3]: (x0,y0,z0), (x1,y1,z1), or centre -+ (w/2 cos - l/2 sin, w/2 sin + l/2 cos, h/2); plain tensor arithmetic (not a hot path)"""
    _rows("proj2d_points", boxes)
    if boxes.shape[1] == 6:
        return torch.stack([boxes[:, :3], boxes[:, 3:]])
    w, l, h, cs, sn = boxes[:, 3] / 2, boxes[:, 4] / 2, boxes[:, 5] / 2, torch.cos(boxes[:, 6]), torch.sin(boxes[:, 6])
    v = torch.stack([w * cs - l * sn, w * sn + l * cs, h], 1)
    return torch.stack([boxes[:, :3] - v, boxes[:, :3] + v])


class _Proj2dTerms(Function):
    @staticmethod
    def forward(ctx, pred, target, cams):
        pred, target = pred.contiguous(), target.contiguous()
        ctx.save_for_backward(pred, target)
        ctx.cams = cams
        return ops.proj2d_fwd(pred, target, cams)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        pred, target = ctx.saved_tensors
        return (ops.proj2d_bwd(pred, target, g.contiguous(), ctx.cams) if ctx.needs_input_grad[0] else None), None, None


def proj2d_terms(pred, target, res):
    """pred, target [n, 6|7] fp32 device rows, res: the cameras' scene size (max(mesh_size) in the RPN, 160 in FCOS) -> terms [n]"""
    _rows("proj2d_terms", pred, target)
    return _Proj2dTerms.apply(pred, target.detach(), _cams(res))
