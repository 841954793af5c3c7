"""The two detectors' dense results fed straight into DetectionEvaluator (nerf_mae_amd.det_eval): FCOSOverNeRF and NeRFRegionProposalNetwork with stub backbones
on the small grids of tests/test_fcos_network_gpu.py and tests/test_rpn_network_gpu.py, their detections_dense() / proposals_dense() tensors passed to update()
as they are (FCOS's rows with the level in column 0 read in place), and compute() compared with the float64 restatement (tests/_det_eval_ref.py) run on the same
tensors copied to the host, as tests/test_det_eval_gpu.py compares.  Ground truth: the scenes those tests train on.  The restatement's decision margins on these
detections are asserted first (at least 1e-5, against an fp32 IoU error of about 1e-7)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _det_eval_ref as E  # noqa: E402
from tests import test_fcos_network_gpu as TF  # noqa: E402
from tests import test_rpn_network_gpu as TR  # noqa: E402
from tests.test_det_eval_gpu import check_compute  # noqa: E402

pytestmark = pytest.mark.gpu
AP_THRESHOLDS = (0.1, 0.25, 0.5)


def _evaluate(boxes, scores, counts, gt_list, limits, top_k, level_column, tag):
    from nerf_mae_amd import DetectionEvaluator
    N, ncols = len(gt_list), gt_list[0].shape[1]
    gmax = max(len(g) for g in gt_list)
    gt = torch.zeros((N, gmax, ncols), device="cuda")
    for n, g in enumerate(gt_list):
        gt[n, :len(g)] = g.float().cuda()
    gt_counts = torch.tensor([len(g) for g in gt_list], dtype=torch.int32).cuda()
    ev = DetectionEvaluator(limits, AP_THRESHOLDS, top_k=top_k)
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev.update(boxes, scores, counts, gt, gt_counts, level_column=level_column)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    out = ev.compute()
    off = int(level_column)
    scenes = [(boxes[n, :int(counts[n]), off:].cpu().numpy(), scores[n, :int(counts[n])].cpu().numpy(), gt_list[n].float().numpy()) for n in range(N)]
    assert all((s[1][:-1] >= s[1][1:]).all() for s in scenes), "the dense rows are in descending score"
    m = E.decision_margins(scenes, limits, (top_k,), AP_THRESHOLDS, argmax_of_claimants_only=True)      # compute() is compared, not the arg-max indices
    print(tag, [len(s[0]) for s in scenes], m)
    assert min(m["recall_thr"], m["ap_thr"], m["greedy_gap"], m["argmax_gap"]) >= E.MARGIN, m
    ious = E.iou_matrices(scenes)
    assert sum(len(s[0]) for s in scenes) > 0 and max(i.max() for i in ious if i.size) > 0, "detections that overlap the ground truth"
    check_compute(out, scenes, ious, limits, AP_THRESHOLDS, top_k, tag)


@pytest.mark.parametrize("obb", (False, True), ids=("aabb", "obb"))
def test_fcos_over_nerf_detections_into_the_evaluator(obb):
    c = TF.train_ref(obb)
    maps = [f.float().cuda() for f in c["feats"]]
    net = TF._over(obb, c["P"], maps).eval()
    grid = torch.zeros((TF.N, 4, *TF.MESH), device="cuda")
    with torch.no_grad():
        boxes, scores, counts = net.fcos_module.detections_dense(list(TF.ORI), list(net.backbone(grid)))
    assert boxes.shape[2] == (8 if obb else 7)
    _evaluate(boxes, scores, counts, c["boxes"], (5, 10, 300), 8, True, f"fcos obb={obb}")


@pytest.mark.parametrize("rotated", (False, True), ids=("aabb", "obb"))
def test_nerf_rpn_proposals_into_the_evaluator(rotated):
    c = TR.train_ref(rotated)
    maps = [f.float().cuda() for f in c["feats"]]
    net = TR._nerf(rotated, c["P"], maps).eval()
    with torch.no_grad():
        boxes, scores, _, _, counts = net.rpn.proposals_dense(TR.meshes(), list(net.backbone(TR.meshes())), TR.R.ORI)
    assert boxes.shape[2] == (7 if rotated else 6)
    _evaluate(boxes, scores, counts, c["boxes"], (10, 50, 300), None, False, f"rpn rotated={rotated}")
