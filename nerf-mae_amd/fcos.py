"""The reference's anchor-free FCOS detector (nerf_rpn/model/fcos/fcos.py) on the HIP kernels of csrc/fcos_head.hip (head), csrc/fcos.hip (losses) and
csrc/fcos_post.hip (post-processing), with the reference's names (the import swap is one line):

  Scale          fcos.py:17-23
  FCOSHead       fcos.py:26-139: two towers of num_convs x (Conv3d 3^3 -> GroupNorm(32) -> ReLU) on the channels-last convolutions and the GroupNorm kernels,
                 then cls_logits, bbox_pred and centerness by the output kernel, which writes the fp32 NCDHW planes the loss and the post-processing read in
                 place.  Same constructor, state_dict keys, shapes and initialisation; compute_dtype is an addition.
  FCOSModule     fcos.py:142-336: head + FCOSLossComputation (training) or FCOSPostProcessor (evaluation); detections_dense() is the capturable form
  FCOSOverNeRF   fcos.py:339-474: backbone + FCOSModule over a list of (C, W, L, H) grids, zero padding to `resolution` or to the batch maximum

The head's parameters are not autograd inputs of its Function: their gradients are accumulated into .grad by the kernels (as in rpn._RPNHeadFn).  Nothing in the
training forward and backward waits for the host; FCOSPostProcessor waits once, for the counts that size its lists.

Saved for the backward, per tower, level and layer: the convolution's output x and the normalised, rectified y (the next convolution's input, which its weight
gradient reads), both in the compute dtype, and 8 bytes of statistics per (scene, group): 2 N V C sizeof(dt) bytes per layer and tower.

Stated deviations from the reference:
  - in_channels must be a multiple of 32 (nn.GroupNorm(32, C) needs that too) up to 2048; at most 5 levels (the reference has 5 Scale parameters), and at most 4
    in FCOSModule (the range table of the loss has four rows);
  - the stored activations are in compute_dtype (bfloat16 by default; float32 reproduces the reference to fp32 rounding);
  - the deviations of fcos_loss.py and fcos_inference.py apply to FCOSModule;
  - FCOSModule.output_objectness uses int where the reference uses the removed alias np.int."""
from __future__ import annotations

import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import conv_layer, ops
from .fcos_inference import FCOSPostProcessor, fcos_postprocess_dense
from .fcos_loss import FCOSLossComputation, FCOSProj2dLossComputation
from .fpn import _NCDHWToCL, check_channels_last
from .model import _gradbuf

MAX_LEVELS = ops.FCOS_HEAD_MAX_LEVELS


class Scale(nn.Module):
    def __init__(self, init_value=1.0):
        super().__init__()
        self.scale = nn.Parameter(torch.FloatTensor([init_value]))

    def forward(self, input):
        return input * self.scale


class _FCOSHeadFn(Function):
    """(head, mode, *channels-last features) -> (*cls levels, *regression levels, *centerness levels).  Jobs are numbered 2 l + t (level l, tower t: 0 cls,
    1 bbox); every GroupNorm launch covers all of them."""

    @staticmethod
    def forward(ctx, head, mode, *feats):
        pk, depth, L = head._pk, head.num_convs, len(feats)
        towers = [0, 1] * L
        cur = [f.contiguous() for f in feats for _ in (0, 1)]
        saved = []
        for k in range(depth):
            xs = []
            for j, a in enumerate(cur):
                t = j & 1
                xs.append(conv_layer.forward(pk, f"t{t}c{k}", head._tower(t)[3 * k], a))
            gn = [head._tower(t)[3 * k + 1] for t in (0, 1)]
            stats = ops.fcos_gn_stats(xs, gn[0].num_groups, gn[0].eps)
            ys = ops.fcos_gn_apply(xs, towers, stats, [g.weight for g in gn], [g.bias for g in gn], gn[0].num_groups)
            saved.append((cur, xs, ys, stats))
            cur = ys
        acts = [(cur[2 * l], cur[2 * l + 1]) for l in range(L)]
        cls, reg, ctr, u = ops.fcos_head_out_fwd(acts, [pk["o0.w"], pk["o1.w"]], head.cls_logits.bias, head.bbox_pred.bias, head.centerness.bias,
                                                 [head.scales[l].scale for l in range(L)], head.fpn_strides[:L], head.num_reg, head.centerness_on_reg, mode)
        ctx.head, ctx.mode, ctx.saved, ctx.acts, ctx.u = head, mode, saved, acts, u
        return (*cls, *reg, *ctr)

    @staticmethod
    @once_differentiable
    def backward(ctx, *gs):
        head, mode, saved, acts, u = ctx.head, ctx.mode, ctx.saved, ctx.acts, ctx.u
        pk, C, depth, L = head._pk, head.in_channels, head.num_convs, len(acts)
        towers = [0, 1] * L
        g_cls, g_reg, g_ctr = [[g.contiguous() for g in gs[i * L:(i + 1) * L]] for i in range(3)]
        scales = [head.scales[l].scale for l in range(L)]
        g16, gt = ops.fcos_head_out_bwd(acts, g_cls, g_reg, g_ctr, u, scales, head.fpn_strides[:L], head.num_reg, head.centerness_on_reg, mode,
                                        _gradbuf(head.cls_logits.bias), _gradbuf(head.bbox_pred.bias), _gradbuf(head.centerness.bias), [_gradbuf(s) for s in scales])
        keep = [gt]             # keep: tensors the forked side stream still reads -- referenced until the join
        with ops.side_stream():
            keep.append(ops.fcos_head_out_wgrad(acts, gt, head.num_reg, head.centerness_on_reg, _gradbuf(head.cls_logits.weight), _gradbuf(head.bbox_pred.weight),
                                                _gradbuf(head.centerness.weight)))
        dcur = [ops.conv3d_k3(g16[l][t], pk[f"o{t}.wd"], C) for l in range(L) for t in (0, 1)]
        for k in range(depth - 1, -1, -1):
            inp, xs, ys, stats = saved[k]
            gn = [head._tower(t)[3 * k + 1] for t in (0, 1)]
            dxs = ops.fcos_gn_bwd(dcur, xs, ys, towers, stats, [g.weight for g in gn], [_gradbuf(g.weight) for g in gn], [_gradbuf(g.bias) for g in gn], gn[0].num_groups)
            keep.append(dxs)
            dcur = []
            for j, dx in enumerate(dxs):
                t = j & 1
                dcur.append(conv_layer.backward(pk, f"t{t}c{k}", head._tower(t)[3 * k], dx, inp[j], need_dx=k > 0 or ctx.needs_input_grad[2 + j // 2]))
        dfeats = [None if dcur[2 * l] is None or not ctx.needs_input_grad[2 + l] else ops.add_inplace(dcur[2 * l], dcur[2 * l + 1]) for l in range(L)]
        ops.join_side()
        del keep
        return (None, None, *dfeats)


class FCOSHead(nn.Module):
    """fcos.py:26-139.  Parameters live in `nn.Conv3d`, `nn.GroupNorm` and `nn.ReLU` holders inside `nn.Sequential` (cls_tower, bbox_tower) and in cls_logits,
    bbox_pred, centerness and scales, so that names, shapes and the initialisation (normal 0.01, zero bias, cls_logits.bias = -log(99)) equal the reference's; their
    forward is never used.  Outputs per level: logits (N, 1, W, L, H), bbox_reg (N, 6|8, W, L, H), centerness (N, 1, W, L, H), fp32.  self.training selects the
    stride multiply of the evaluation mode."""

    def __init__(self, in_channels, num_convs, fpn_strides, norm_reg_targets=True, centerness_on_reg=True, use_obb=False, compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if in_channels % 32 or not 32 <= in_channels <= 2048:
            raise NotImplementedError(f"FCOSHead: in_channels must be a multiple of 32 up to 2048 (GroupNorm(32, C) and the kernels' channel tiles), got {in_channels}")
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise TypeError(f"compute_dtype must be bfloat16 or float32, got {compute_dtype}")
        if int(num_convs) < 0:
            raise ValueError(f"FCOSHead: num_convs >= 0, got {num_convs}")
        self.in_channels, self.num_convs = int(in_channels), int(num_convs)
        self.fpn_strides = list(fpn_strides)
        self.norm_reg_targets = norm_reg_targets
        self.centerness_on_reg = centerness_on_reg
        self.use_obb = use_obb
        self.num_reg = 8 if use_obb else 6
        self.compute_dtype = compute_dtype
        cls_tower, bbox_tower = [], []
        for _ in range(self.num_convs):
            for tower in (cls_tower, bbox_tower):
                tower.append(nn.Conv3d(in_channels, in_channels, kernel_size=3, stride=1, padding=1, bias=True))
                tower.append(nn.GroupNorm(32, in_channels))
                tower.append(nn.ReLU())
        self.add_module("cls_tower", nn.Sequential(*cls_tower))
        self.add_module("bbox_tower", nn.Sequential(*bbox_tower))
        self.cls_logits = nn.Conv3d(in_channels, 1, kernel_size=3, stride=1, padding=1)
        self.bbox_pred = nn.Conv3d(in_channels, self.num_reg, kernel_size=3, stride=1, padding=1)
        self.centerness = nn.Conv3d(in_channels, 1, kernel_size=3, stride=1, padding=1)
        for modules in (self.cls_tower, self.bbox_tower, self.cls_logits, self.bbox_pred, self.centerness):
            for layer in modules.modules():
                if isinstance(layer, nn.Conv3d):
                    torch.nn.init.normal_(layer.weight, std=0.01)
                    torch.nn.init.constant_(layer.bias, 0)
        prior_prob = 0.01
        torch.nn.init.constant_(self.cls_logits.bias, -math.log((1 - prior_prob) / prior_prob))
        self.scales = nn.ModuleList([Scale(init_value=1.0) for _ in range(5)])
        self._pk = None
        self._pk_key = None
        self._w16 = None

    def _tower(self, t):
        return self.bbox_tower if t else self.cls_tower

    def _pack(self):
        ps = list(self.parameters())

        def fill(P):
            # the output convs of one tower as one 16-row weight (csrc/fcos_head.hip: tower columns); the rows past the tower's columns stay zero
            self._w16 = [torch.zeros((16, self.in_channels, 3, 3, 3), dtype=torch.float32, device=ps[0].device) for _ in (0, 1)]
            for t in (0, 1):
                for k in range(self.num_convs):
                    conv_layer.register(P, f"t{t}c{k}", self._tower(t)[3 * k], self.compute_dtype)
                P.add(f"o{t}.w", self._w16[t], P.CONV_F)
                P.add(f"o{t}.wd", self._w16[t], P.CONV_D)

        @torch.no_grad()
        def refresh():
            self._w16[0][0].copy_(self.cls_logits.weight[0])
            self._w16[1][:self.num_reg].copy_(self.bbox_pred.weight)
            if self.centerness_on_reg:
                self._w16[1][self.num_reg].copy_(self.centerness.weight[0])
            else:
                self._w16[0][1].copy_(self.centerness.weight[0])

        conv_layer.ensure_packed(self, ps, "FCOSHead (HIP) needs its parameters on a HIP device: call .cuda() first (no CPU fallback)", fill, refresh)

    def forward_channels_last(self, feats):
        """feats: per level a channels-last (N, W, L, H, C) tensor in the compute dtype -> (logits, bbox_reg, centerness), lists of fp32 NCDHW tensors"""
        feats = list(feats)
        if not 1 <= len(feats) <= MAX_LEVELS:
            raise ValueError(f"FCOSHead supports 1 to {MAX_LEVELS} levels (the reference has {MAX_LEVELS} scales), got {len(feats)}")
        if len(feats) > len(self.fpn_strides):
            raise ValueError(f"FCOSHead: {len(feats)} levels but {len(self.fpn_strides)} fpn_strides")
        check_channels_last("FCOSHead", "W, L, H", feats, self.in_channels, self.compute_dtype)
        self._pack()
        mode = ("train" if self.training else "eval") if self.norm_reg_targets else "exp"
        out = _FCOSHeadFn.apply(self, mode, *feats)
        L = len(feats)
        return list(out[:L]), list(out[L:2 * L]), list(out[2 * L:])

    def forward(self, x):
        """reference signature: list of NCDHW tensors -> (logits, bbox_reg, centerness)"""
        x = list(x)
        for f in x:
            if not f.is_cuda:
                raise RuntimeError("FCOSHead (HIP) needs HIP device tensors (no CPU fallback)")
        return self.forward_channels_last([_NCDHWToCL.apply(f, self.compute_dtype) for f in x])


class FCOSModule(nn.Module):
    """fcos.py:142-336 with the reference's constructor (args: num_convs, norm_reg_targets, centerness_on_reg, rotated_bbox, pre_nms_thresh, pre_nms_top_n,
    nms_thresh, fpn_post_nms_top_n, min_size, center_sampling_radius, iou_loss_type, use_additional_l1_loss, proj2d_loss_weight; compute_dtype optional).
    Training: (None, None, losses); evaluation: (boxes, scores, {}).  The only submodule with parameters is head, so the state_dict keys are head.*."""

    def __init__(self, args, in_channels, fpn_strides, resolution=None, world_size=1):
        super().__init__()
        self.head = FCOSHead(in_channels, args.num_convs, fpn_strides, norm_reg_targets=args.norm_reg_targets, centerness_on_reg=args.centerness_on_reg,
                             use_obb=args.rotated_bbox, compute_dtype=getattr(args, "compute_dtype", torch.bfloat16))
        self.box_selector_test = FCOSPostProcessor(args.pre_nms_thresh, args.pre_nms_top_n, args.nms_thresh, args.fpn_post_nms_top_n, args.min_size, 1,
                                                   use_obb=args.rotated_bbox)
        proj2d_loss_weight = getattr(args, "proj2d_loss_weight", 0.0)
        if args.rotated_bbox and proj2d_loss_weight > 0:
            self.loss_evaluator = FCOSProj2dLossComputation(fpn_strides, args.center_sampling_radius, args.iou_loss_type, args.norm_reg_targets, world_size,
                                                            args.use_additional_l1_loss, proj2d_loss_weight)
        else:       # a positive weight with axis-aligned boxes raises NotImplementedError here
            self.loss_evaluator = FCOSLossComputation(fpn_strides, args.center_sampling_radius, args.iou_loss_type, args.norm_reg_targets, world_size=world_size,
                                                      use_obb=args.rotated_bbox, use_additional_l1_loss=args.use_additional_l1_loss,
                                                      proj2d_loss_weight=proj2d_loss_weight)
        self.resolution = resolution
        self.fpn_strides = fpn_strides
        self.world_size = world_size
        self._loc_cache = {}
        self._mask_cache = {}

    def _masks_wanted(self, features):
        return self.resolution is not None or features[0].shape[0] > 1          # fcos.py:207-214

    def forward(self, grid_sizes, features, targets=None, objectness_output_paths=None):
        """grid_sizes: the scenes' sizes before padding, a list of (w, l, h); features: per level NCDHW; targets: per scene the boxes [k, 6|7] ->
        (boxes, scores, losses)"""
        box_cls, box_regression, centerness = self.head(features)
        locations = self.compute_locations(features)
        padding_masks = self.compute_padding_masks(locations, grid_sizes) if self._masks_wanted(features) else None
        if objectness_output_paths is not None:
            self.output_objectness(box_cls, centerness, grid_sizes, objectness_output_paths)
        if self.training:
            loss_box_cls, loss_box_reg, loss_centerness = self.loss_evaluator(locations, box_cls, box_regression, centerness, targets, padding_masks=padding_masks)
            return None, None, {"loss_cls": loss_box_cls, "loss_reg": loss_box_reg, "loss_centerness": loss_centerness}
        boxes, scores = self.box_selector_test(locations, box_cls, box_regression, centerness, grid_sizes, padding_masks=padding_masks)
        return boxes, scores, {}

    def detections_dense(self, grid_sizes, features):
        """the detections as fcos_postprocess_dense's fixed-size triple (boxes [N, cap, 1+6|7], scores [N, cap], counts [N] int32): never waits for the host and is
        capturable once the locations and masks of these sizes are cached (one eager call); pass grid_sizes as an int32 device tensor [N, 3] when capturing"""
        box_cls, box_regression, centerness = self.head(features)
        locations = self.compute_locations(features)
        masks = None
        if self._masks_wanted(features):
            if isinstance(grid_sizes, torch.Tensor):
                masks = [((loc[None, :, 0] < grid_sizes[:, None, 0]) & (loc[None, :, 1] < grid_sizes[:, None, 1]) & (loc[None, :, 2] < grid_sizes[:, None, 2])) for loc in locations]
            else:
                masks = self.compute_padding_masks(locations, grid_sizes)
        p = self.box_selector_test
        return fcos_postprocess_dense(locations, box_cls, box_regression, centerness, grid_sizes, masks, p.pre_nms_thresh, p.pre_nms_top_n, p.nms_thresh, p.fpn_post_nms_top_n,
                                      p.min_size, p.bbox_aug_enabled, p.use_obb)

    def compute_locations(self, features):
        """fcos.py:272-299, cached per (level, feature size, device)"""
        locations = []
        for level, feature in enumerate(features):
            w, l, h = feature.size()[-3:]
            key = (level, int(w), int(l), int(h), feature.device)
            if key not in self._loc_cache:
                self._loc_cache[key] = self.compute_locations_per_level(w, l, h, self.fpn_strides[level], feature.device)
            locations.append(self._loc_cache[key])
        return locations

    def compute_locations_per_level(self, w, l, h, stride, device):
        shifts = [torch.arange(0, n * stride, step=stride, dtype=torch.float32, device=device) for n in (w, l, h)]
        shift_x, shift_y, shift_z = torch.meshgrid(*shifts, indexing="ij")
        return torch.stack((shift_x.reshape(-1), shift_y.reshape(-1), shift_z.reshape(-1)), dim=1) + stride // 2

    def compute_padding_masks(self, locations, ori_sizes):
        """fcos.py:301-320: per level a bool [N, n], True where the location lies inside the scene's original size; cached per (locations, sizes)"""
        sizes = tuple(tuple(int(v) for v in o) for o in ori_sizes)
        masks = []
        for loc in locations:
            key = (loc.data_ptr(), tuple(loc.shape), sizes)
            if key not in self._mask_cache:
                self._mask_cache[key] = self.compute_padding_masks_per_level(loc, sizes)
            masks.append(self._mask_cache[key])
        return masks

    def compute_padding_masks_per_level(self, locations, ori_sizes):
        return torch.stack([(locations[:, 0] < w) & (locations[:, 1] < l) & (locations[:, 2] < h) for w, l, h in ori_sizes], dim=0)

    def output_objectness(self, box_cls, centerness, ori_sizes, output_paths):
        """fcos.py:322-336, in plain torch as the reference has it"""
        for i in range(len(ori_sizes)):
            all_levels = {}
            for level in range(len(box_cls)):
                score = box_cls[level][i].sigmoid() * centerness[level][i].sigmoid()
                w, l, h = np.ceil(np.array([int(v) for v in ori_sizes[i]]) / self.fpn_strides[level]).astype(int)
                all_levels[str(level)] = torch.sqrt(score[0, :w, :l, :h]).detach().cpu().numpy()
            np.savez_compressed(output_paths[i], **all_levels)


class FCOSOverNeRF(nn.Module):
    """fcos.py:339-474: backbone + FCOSModule over a list of (C, W, L, H) grids -> (boxes, losses, scores)"""

    def __init__(self, args, backbone, fpn_strides, resolution=None, world_size=1):
        if not hasattr(backbone, "out_channels"):
            raise ValueError("backbone should contain an attribute out_channels specifying the number of output channels (assumed to be the same for all the levels)")
        super().__init__()
        self.args = args
        self.world_size = world_size
        self.backbone = backbone
        self.fcos_module = FCOSModule(args, backbone.out_channels, fpn_strides, resolution=resolution, world_size=world_size)
        self.resoluton = resolution          # the reference's spelling

    def transform(self, meshes, target_shape=None):
        """zero padding to target_shape or to the batch maximum (in place in the list, as the reference does)"""
        target_shape = np.max([mesh.shape for mesh in meshes], axis=0) if target_shape is None else np.array(target_shape)
        for i, mesh in enumerate(meshes):
            meshes[i] = F.pad(mesh, (0, int(target_shape[-1] - mesh.shape[-1]), 0, int(target_shape[-2] - mesh.shape[-2]), 0, int(target_shape[-3] - mesh.shape[-3])),
                              mode="constant", value=0)
        return meshes

    def forward(self, meshes, targets=None, objectness_output_paths=None):
        if self.training:
            if targets is None:
                torch._assert(False, "targets should not be none when in training mode")
            ncols = 7 if self.args.rotated_bbox else 6
            for boxes in targets:
                if isinstance(boxes, torch.Tensor):
                    torch._assert(len(boxes.shape) == 2 and boxes.shape[-1] == ncols, f"Expected target boxes to be a tensor of shape [N, {ncols}], got {boxes.shape}.")
                else:
                    torch._assert(False, f"Expected target boxes to be of type Tensor, got {type(boxes)}.")
        original_mesh_sizes = []
        for mesh in meshes:
            val = mesh.shape[-3:]
            torch._assert(len(val) == 3, f"expecting the last three dimensions of the Tensor to be W, L and H instead got {mesh.shape[-3:]}")
            original_mesh_sizes.append((val[0], val[1], val[2]))
        if self.resoluton is not None:
            meshes = self.transform(meshes, [self.resoluton, self.resoluton, self.resoluton])
        elif len(meshes) > 1:
            meshes = self.transform(meshes)
        mesh_tensors = torch.stack(meshes, dim=0)
        features = list(self.backbone(mesh_tensors))
        boxes, scores, losses = self.fcos_module(original_mesh_sizes, features, targets, objectness_output_paths)
        return boxes, losses, scores
