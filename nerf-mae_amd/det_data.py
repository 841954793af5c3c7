"""The reference's two augmentation functions of the detection path under their own signatures, on device tensors (nerf_rpn/datasets.py:173-244 and
478-524): compatibility wrappers over `ops.grid_prepare` / `ops.grid_prepare_rs` / `ops.boxes_augment`.  They take the channel-first (4,W,L,H) grid the
reference passes around, so they pay a permute copy on the way in and a crop on the way out; the product path is `data.DetectionBatcher`, which reads the
scene as stored and writes the padded batch directly."""
import random

import torch

from . import ops
from .data import draw_detection_augmentation


def _scene(rgbsigma, boxes, flags, has_rs, angle, scale):
    if rgbsigma.dim() != 4 or rgbsigma.shape[0] != 4 or not rgbsigma.is_cuda:
        raise ValueError("expected a (4,W,L,H) device tensor")
    src = rgbsigma.to(torch.float32).permute(1, 2, 3, 0).contiguous()
    R = max(src.shape[:3])
    dst = torch.empty((4, R, R, R), dtype=torch.float32, device=src.device)
    e = ops.grid_prepare_rs(src, dst, R, flags, angle, scale) if has_rs else ops.grid_prepare(src, dst, R, flags)
    out = dst[:, :e[0], :e[1], :e[2]].contiguous()
    if boxes is not None:
        b = boxes.to(torch.float32).contiguous()
        boxes = ops.boxes_augment(b, [(0, b.shape[0], flags, has_rs, e, angle, scale)])
    return out, boxes


def rotate_and_scale_scene(rgbasigma, boxes, angle, scale):
    """datasets.py:478-524: rotate the scene about its centre's z axis by `angle` and scale it, boxes [G,7] (or None) along with it"""
    assert boxes is None or boxes.shape[1] == 7
    return _scene(rgbasigma, boxes, 0, True, float(angle), float(scale))


def augment_rpn_inputs(rgbsigma, boxes, flip_prob, rotate_prob, rot_scale_prob, z_up=True):
    """datasets.py:173-244 with the draws from the global `random` module, in the reference's order"""
    if boxes is not None:
        assert (z_up and boxes.shape[1] == 7) or boxes.shape[1] == 6, "z_up must be True when boxes are in (x, y, z, w, l, h, t) format"
    oriented = boxes is not None and boxes.shape[1] == 7
    if not z_up:
        draw_detection_augmentation(flip_prob, rotate_prob, rot_scale_prob, oriented, random.Random(0))     # the ValueErrors come first, as in the reference
        raise NotImplementedError("augment_rpn_inputs: z_up=False (Hypersim) is not built")
    flags, angle, scale = draw_detection_augmentation(flip_prob, rotate_prob, rot_scale_prob, oriented, random)
    return _scene(rgbsigma, boxes, flags, (angle, scale) != (0.0, 1.0), angle, scale)
