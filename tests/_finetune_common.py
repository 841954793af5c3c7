"""What tests/test_finetune_cpu.py and tests/test_finetune_gpu.py share: the common small models (resolution 32, swin_t, 64 FPN channels, fp32 compute), the
scenes and their boxes.  FCOS arguments: those of tests/test_fcos_network_gpu.py with num_convs=2, rotated_bbox=True, strides [4, 8, 16, 32], resolution 32."""
import types

import numpy as np
import torch

R = 32
STRIDES = [4, 8, 16, 32]
POST = dict(pre_nms_thresh=0.05, pre_nms_top_n=40, nms_thresh=0.3, fpn_post_nms_top_n=15, min_size=0.0)
BASE_FLAT_NUMEL = 29115504           # the base's flat buffer of the common model: 169 tensors, 29 115 462 elements on 8-element granules


def fcos_args(dtype=torch.float32):
    return types.SimpleNamespace(num_convs=2, norm_reg_targets=True, centerness_on_reg=True, rotated_bbox=True, center_sampling_radius=1.5, iou_loss_type="iou",
                                 use_additional_l1_loss=True, proj2d_loss_weight=0.0, compute_dtype=dtype, **POST)


def backbone(dtype=torch.float32):
    from nerf_mae_amd.fpn import SwinTransformer_FPN_Pretrained_Skip
    return SwinTransformer_FPN_Pretrained_Skip(resolution=R, is_eval=True, backbone_type="swin_t", out_channels=64, compute_dtype=dtype)


def fcos_model(seed=0):
    from nerf_mae_amd.fcos import FCOSOverNeRF
    torch.manual_seed(seed)
    return FCOSOverNeRF(fcos_args(), backbone(), list(STRIDES), resolution=R)


def rpn_model(seed=0):
    from nerf_mae_amd.rpn import NeRFRegionProposalNetwork, RPNHead, _default_anchorgen
    torch.manual_seed(seed)
    bb = backbone()
    gen = _default_anchorgen()
    head = RPNHead(bb.out_channels, gen.num_anchors_per_location()[0], 1, rotate=False, compute_dtype=torch.float32)
    net = NeRFRegionProposalNetwork(bb, rpn_anchor_generator=gen, rpn_head=head, rpn_fg_iou_thresh=0.35, rpn_bg_iou_thresh=0.2)
    net.check_targets = False
    return net


def semantics_model(seed=0):
    from nerf_mae_amd.heads import SwinTransformer_VoxelSemantics_Pretrained_Skip
    torch.manual_seed(seed)
    return SwinTransformer_VoxelSemantics_Pretrained_Skip(resolution=R, is_eval=True, compute_dtype=torch.float32)


def scene(seed):
    from nerf_mae_amd import data
    return data.synthetic_scene((R, R, R), seed)


def obb_boxes(seed):
    """two oriented boxes (x, y, z, w, l, h, theta) well inside the 32^3 grid, extents 8 .. 12: their largest regression distance stays under 16, the range of
    the stride-4 level, whose 8^3 locations then hold the positives"""
    rng = np.random.default_rng(1000 + seed)
    c = np.array([[11.0, 12.0, 10.0], [21.0, 20.0, 21.0]]) + rng.uniform(-1.0, 1.0, (2, 3))
    s = rng.uniform(8.0, 12.0, (2, 3))
    th = rng.uniform(-0.5, 0.5, (2, 1))
    return np.concatenate([c, s, th], 1).astype(np.float32)


def aabb_boxes(seed):
    """the same boxes axis-aligned (x0, y0, z0, x1, y1, z1)"""
    b = obb_boxes(seed)
    return np.concatenate([b[:, :3] - b[:, 3:6] / 2, b[:, :3] + b[:, 3:6] / 2], 1).astype(np.float32)


def label_grid(seed, classes=19):
    """(1, R, R, R) float label grid, classes 0 .. classes-1"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, classes, (1, R, R, R), generator=g).float()


def trainable(module):
    return [(n, p) for n, p in module.named_parameters() if p.requires_grad]


def round8(n):
    return (n + 7) // 8 * 8


def record_batches(tr, scenes):
    """wraps tr.batcher.prepare -> the list that fills with the batches it receives, each as the indices into `scenes` of the arrays handed over"""
    seen, prepare = [], tr.batcher.prepare

    def recording(batch, *a, **k):
        seen.append([next(i for i, s in enumerate(scenes) if s is b) for b in batch])
        return prepare(batch, *a, **k)
    tr.batcher.prepare = recording
    return seen
