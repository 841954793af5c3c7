"""The reference's two native downstream ops on the HIP kernels of csrc/rotated.hip, with the reference's Python signatures.

  roi_align_rotated_3d / ROIAlignRotated3D   nerf_rpn/model/rotated_align/roi_align_rotate_3d.py (used by detector.py:192-193), NCWLH fp32
  roi_align_rotated_3d_channels_last         the same op on a channels-last (B,W,L,H,C) fp32|bf16 map, returning [N,PW,PL,PH,C]
  sort_v                                     nerf_rpn/model/rotated_iou/cuda_op/cuda_ext.py (called from box_intersection_2d.py:141)

rois are fp32 [N, 8]: batch index, centre (w,l,h), size (w,l,h), angle in degrees.  The gradient with respect to the map is fp32 for
either dtype (a running bf16 sum would lose bits at every add) and is cast to the map's dtype once; rois get no gradient, as in the
reference.  Voxel strides are the correct ones on non-cubic maps, where the reference's are not ("Rotated RoIAlign").
There is no CPU path: CPU tensors raise."""
from __future__ import annotations

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import ops


class _ROIAlignRotated3D(Function):
    @staticmethod
    def forward(ctx, input, rois, output_size, spatial_scale, sampling_ratio, layout):
        input, rois = input.contiguous(), rois.contiguous()
        ctx.save_for_backward(rois)
        ctx.args = (tuple(input.shape), input.dtype, tuple(int(v) for v in output_size), float(spatial_scale), int(sampling_ratio), layout)
        return ops.roi_align_rotated_3d_fwd(input, rois, ctx.args[2], ctx.args[3], ctx.args[4], layout)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        rois, = ctx.saved_tensors
        shape, dtype, output_size, spatial_scale, sampling_ratio, layout = ctx.args
        dx = ops.roi_align_rotated_3d_bwd(grad_output.contiguous(), rois, shape, output_size, spatial_scale, sampling_ratio, layout)
        if dtype == torch.bfloat16:     # one rounding of the finished fp32 sum (numel is a multiple of 8: C is)
            dx = ops.grad_to_bf16(dx.view(-1), torch.empty(dx.numel(), dtype=dtype, device=dx.device)).view(shape)
        return dx, None, None, None, None, None


def roi_align_rotated_3d(input, rois, output_size, spatial_scale, sampling_ratio):
    """input (B,C,W,L,H) fp32 -> [N,C,PW,PL,PH] fp32: the reference's layout and call"""
    if input.dtype != torch.float32:
        raise TypeError("roi_align_rotated_3d takes an fp32 NCWLH map; bf16 maps go through roi_align_rotated_3d_channels_last")
    return _ROIAlignRotated3D.apply(input, rois, output_size, spatial_scale, sampling_ratio, ops.ROI_NCWLH)


def roi_align_rotated_3d_channels_last(input, rois, output_size, spatial_scale, sampling_ratio):
    """input (B,W,L,H,C) fp32 or bf16, C a multiple of 8 -> [N,PW,PL,PH,C] in the same dtype"""
    return _ROIAlignRotated3D.apply(input, rois, output_size, spatial_scale, sampling_ratio, ops.ROI_CHANNELS_LAST)


class ROIAlignRotated3D(nn.Module):
    def __init__(self, output_size, sampling_ratio):
        super().__init__()
        self.output_size = output_size
        self.sampling_ratio = sampling_ratio

    def forward(self, input, rois, spatial_scale):
        return roi_align_rotated_3d(input, rois, self.output_size, spatial_scale, self.sampling_ratio)

    def extra_repr(self):
        return f"output_size={self.output_size}, sampling_ratio={self.sampling_ratio}"


class _SortVertices(Function):
    @staticmethod
    def forward(ctx, vertices, mask, num_valid):
        idx = ops.sort_vertices(vertices.contiguous(), mask.contiguous(), num_valid.contiguous())
        ctx.mark_non_differentiable(idx)
        return idx

    @staticmethod
    def backward(ctx, gradout):
        return None, None, None


sort_v = _SortVertices.apply
