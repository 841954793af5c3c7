"""What tests/test_det_trainers_cpu.py, test_det_trainers_gpu.py and test_det_trainers_dist_gpu.py share: builders on the common small model of
tests/_finetune_common.py (swin_t, resolution 32, 64 FPN channels, fp32 compute, axis-aligned boxes), left on the host so that the CPU tests can use them.

  rpn_model      C.rpn_model, optionally without stochastic depth
  two_stage      the detector of tests/test_two_stage_gpu.py::detector (tests/_two_stage_ref.two_stage: 2^3 RoI output, 24 sampled rows, stock RCNN or
                 FusedRCNN) with its score threshold of 0.05 under threshold_mode "any": an untrained box head's two class probabilities lie near 0.5, so
                 every row passes and the NMS decides what is kept
  scenes, boxes  synthetic 32^3 scenes and their two axis-aligned boxes"""
import torch

from tests import _finetune_common as C
from tests._two_stage_ref import MODEL_POST, OUT, ROWS

TRAIN, VAL = (11, 12, 13), (14, 15)          # three training scenes: with batch 2 the last batch of an epoch is ragged


def no_stochastic_depth(model):
    for mod in model.modules():
        if hasattr(mod, "sd_prob"):
            mod.sd_prob = 0.0
    return model


def rpn_model(seed=0, stochastic_depth=True):
    m = C.rpn_model(seed)
    return m if stochastic_depth else no_stochastic_depth(m)


def two_stage(seed=0, fused=False, stochastic_depth=True, **kw):
    from nerf_mae_amd import detector as D
    rpn = rpn_model(seed, stochastic_depth)
    torch.manual_seed(100 + seed)
    layer = D.ProposalTargetLayer(2, batch_size=ROWS, fg_fraction=0.5, fg_threshold=0.35, bg_threshold=0.2, is_rotated_bbox=False, seed=seed)
    pool = D.ROIPool(OUT, [float(s) for s in C.STRIDES], 0.2, False, "pooling", C.R, False)
    head = (D.FusedRCNN if fused else D.RCNN)(rpn.backbone.out_channels, None, 2, OUT, is_add_layer=False, is_rotated_bbox=False, is_flatten=True)
    roi = D.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=False)
    return D.TwoStageDetector(rpn, roi, MODEL_POST["score_thresh"], MODEL_POST["nms_thresh"], **kw)


def scenes(seeds):
    return [C.scene(s) for s in seeds]


def boxes(seeds):
    return [C.aabb_boxes(s) for s in seeds]


def snapshot(module):
    """every parameter and buffer of the module, cloned"""
    out = {"p." + n: p.detach().clone() for n, p in module.named_parameters()}
    out.update({"b." + n: b.detach().clone() for n, b in module.named_buffers()})
    return out


def same(module, snap):
    now = snapshot(module)
    return list(now) == list(snap) and all(torch.equal(now[k], snap[k]) for k in snap)
