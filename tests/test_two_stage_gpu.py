"""GPU: nerf_mae_amd.detector.TwoStageDetector, Classification_Model.predict_dense, finetune.roi_loss_fn and the two-stage checkpoint functions.

detections_dense is compared with tests/_two_stage_ref.chain, the float64 restatements of the first stage's post-processing, of the pooling, of the box head
and of the RoI post-processing one after the other.  The restatements begin at the RPN head's outputs and the FPN maps, so the detector of that test has
recorded maps and head outputs where its backbone and RPN head stand (tests/_two_stage_ref.chained_detector); proposals, pooling, box head and
post-processing are the package's.  Every margin of the chain is asserted from the restatements before anything runs: the first stage's at its own suite's
1e-5, the pooling's floors and every decision of the post-processing at 1e-3.  Counts and source rows are compared exactly, boxes and scores by
assert_close(rtol=1e-3), and the evaluator's AP with that of the restated detections as lists.  Axis-aligned only: tests/_two_stage_ref.py says why.

The other tests run the common small model of tests/_finetune_common.py (swin_t backbone, 64 FPN channels, mesh 32^3, strides 4 / 8 / 16 / 32, axis-aligned
boxes) with a 2^3 RoI output: detections_dense never waits for the host and is, bit for bit, its three parts called one after the other."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402
from tests import _roi_head_ref as H  # noqa: E402
from tests import _roi_post_ref as P  # noqa: E402
from tests import _rpn_post_ref as RP  # noqa: E402
from tests import _two_stage_ref as T  # noqa: E402
from tests._metrics import assert_close, relerr  # noqa: E402
from tests._two_stage_ref import OUT, ROWS, scenes, two_stage  # noqa: E402

pytestmark = pytest.mark.gpu
POST = T.MODEL_POST
LR, WD, EPS, CLIP = 1e-4, 1e-2, 1e-8, 1.0
AP_THRESHOLDS = T.AP_THRESHOLDS


@pytest.fixture(scope="module")
def detector():
    return two_stage().eval()


@pytest.fixture(scope="module")
def chained():
    """the chain's margins, asserted once, then the detector over the recorded first stage and its detections"""
    c, out, res, marg = T.chain()
    assert not {k: v for k, v in c["marg"].items() if v < RP.MARGIN}, c["marg"]
    assert c["pm"]["floor"] >= H.MARGIN, c["pm"]
    assert all(v >= P.MARGIN for v in marg.values()), marg
    kept, passed = [len(r["scores"]) for r in res], [int(r["cand_ok"].sum()) for r in res]
    assert all(0 < k < p < T.POST_N for k, p in zip(kept, passed)), "the score threshold and the NMS both remove rows, and some stay"
    det, meshes = T.chained_detector()
    det.detections_dense(meshes)                             # plans and the size tensor are made on the first call
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = det.detections_dense(meshes)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    return det, meshes, got, (c, out, res)


def test_detections_equal_the_chain_of_the_restatements(chained):
    from nerf_mae_amd import detector as D
    det, meshes, (boxes, scores, counts), (c, out, res) = chained
    N, n = len(res), T.POST_N
    want = [len(r["scores"]) for r in res]
    assert counts.dtype == torch.int32 and counts.tolist() == want
    for i, (r, k) in enumerate(zip(res, want)):
        assert_close(boxes[i, :k], r["boxes"], 1e-3, f"boxes, scene {i}")
        assert_close(scores[i, :k], r["scores"], 1e-3, f"scores, scene {i}")
        assert not boxes[i, k:].any() and not scores[i, k:].any(), f"rows past the count, scene {i}"
    # the stages in between, and the source rows, which detections_dense does not return
    with torch.no_grad():
        features, (pb, pl, pc), sizes, _ = det._first_stage(meshes)
        ps, pd, rois = det.roi_model.predict_dense(pb, pl, pc, features)
        parts = D.roi_postprocess_dense(ps, pd, rois, pc, sizes, T.POST["score_thresh"], T.POST["nms_thresh"], T.POST["min_size"], True, T.POST["threshold_mode"])
    assert sizes.tolist() == [list(o) for o in c["ori"]] and pc.tolist() == [n] * N and pl[:, :n].tolist() == c["rois"][..., 0].long().tolist()
    cap = pb.shape[1]
    assert_close(pb[:, :n], c["rois"][..., 1:], 1e-3, "proposals")
    assert_close(rois.reshape(N, cap, -1)[:, :n, 1:], c["rois"][..., 1:], 1e-3, "the RoIs the deltas refer to")
    assert_close(ps.reshape(N, cap, -1)[:, :n], out["scores"], 1e-3, "logits")
    assert_close(pd.reshape(N, cap, -1)[:, :n], out["deltas"], 1e-3, "deltas")
    assert torch.equal(parts[0], boxes) and torch.equal(parts[1], scores) and torch.equal(parts[3], counts)
    for i, (r, k) in enumerate(zip(res, want)):
        assert parts[2][i, :k].tolist() == r["index"].tolist(), f"kept rows and their order, scene {i}"
        assert (parts[2][i, k:] == -1).all()


def test_the_triple_goes_into_the_evaluator_unchanged(chained):
    """DetectionEvaluator on detections_dense's triple against the same evaluator on the restated detections as per-scene lists: every IoU between a restated
    detection and a ground-truth box keeps 1e-3 from both AP thresholds and neighbouring scores of the global order differ by 1e-3, so the true-positive flags, the curves and the AP are the same numbers"""
    from nerf_mae_amd.det_eval import DetectionEvaluator
    det, meshes, (boxes, scores, counts), (c, _, res) = chained
    assert min(T.ap_margin(AP_THRESHOLDS)) >= P.MARGIN
    targets = [g.cuda() for g in c["gts"]]
    gt_counts = torch.tensor([t.shape[0] for t in targets], dtype=torch.int32, device="cuda")
    dense = DetectionEvaluator(limits=(100,), ap_thresholds=AP_THRESHOLDS)
    dense.update(boxes, scores, counts, torch.stack(targets), gt_counts)
    lists = DetectionEvaluator(limits=(100,), ap_thresholds=AP_THRESHOLDS)
    lists.update([r["boxes"].float().cuda() for r in res], [r["scores"].float().cuda() for r in res], targets)
    a, b = dense.compute(), lists.compute()
    for t in AP_THRESHOLDS:
        key = f"ap_{int(round(100 * t))}"
        assert int(a[key]["tp_cum"][-1]) > 0, "some detections are true positives"
        flat = lambda r: torch.cat([torch.as_tensor(v, dtype=torch.float64).reshape(-1).cpu() for v in _leaves(r)])
        assert torch.equal(flat(a[key]), flat(b[key])), key
    assert_close(a["recall_ar_top_100"]["gt_overlaps"], b["recall_ar_top_100"]["gt_overlaps"], 1e-3, "gt overlaps")
    lb, ls = det(meshes)                                     # eval forward: the same as per-scene lists, one host wait
    assert [x.shape[0] for x in lb] == counts.tolist() and all(torch.equal(x, boxes[i, :x.shape[0]]) and torch.equal(s, scores[i, :s.shape[0]]) for i, (x, s) in enumerate(zip(lb, ls)))


def test_detections_are_the_three_parts_and_never_wait(detector):
    """the whole model, backbone included: no host wait, and bit for bit the three parts called one after the other"""
    from nerf_mae_amd import detector as D
    meshes, _ = scenes()
    detector.detections_dense(meshes)                        # plans and the size tensor are made on the first call
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        boxes, scores, counts = detector.detections_dense(meshes)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    with torch.no_grad():
        features, (pb, pl, pc), sizes, _ = detector._first_stage(meshes)
        ps, pd, rois = detector.roi_model.predict_dense(pb, pl, pc, features)
        want = D.roi_postprocess_dense(ps, pd, rois, pc, sizes, POST["score_thresh"], POST["nms_thresh"])
    assert torch.equal(boxes, want[0]) and torch.equal(scores, want[1]) and torch.equal(counts, want[3])
    assert sizes.tolist() == [[C.R] * 3] * 2 and int(counts.min()) > 0 and int(pc.min()) > 0


def _leaves(r):
    if isinstance(r, dict):
        for k in sorted(r):
            yield from _leaves(r[k])
    elif isinstance(r, (list, tuple)):
        for v in r:
            yield from _leaves(v)
    elif isinstance(r, (torch.Tensor, float, int)):
        yield r


def test_chunked_prediction_is_bit_identical(detector):
    """predict_dense with chunk_rows = 48 against the unchunked call, bit for bit: the pooling is a per-row computation, and the box head runs in blocks of one
    fixed shape (Classification_Model._head_blocks), so no row's sums depend on how many rows share its call (called plainly, the head's nn.Linear layers gave
    logits 9.5e-7 apart for 96 and for all 3898 rows on an MI355X)"""
    meshes, _ = scenes()
    with torch.no_grad():
        features, (pb, pl, pc), _, _ = detector._first_stage(meshes)
        whole = detector.roi_model.predict_dense(pb, pl, pc, features)
        parts = detector.roi_model.predict_dense(pb, pl, pc, features, chunk_rows=48)
    assert pb.shape[1] > 48 and pb.shape[1] % 48
    for a, b in zip(whole, parts):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="chunk_rows"):
        detector.roi_model.predict_dense(pb, pl, pc, features, chunk_rows=0)


def test_state_dict_keys_and_checkpoint_round_trip(detector, tmp_path):
    from nerf_mae_amd import detector as D
    from nerf_mae_amd.trainer import load_two_stage_checkpoint, save_two_stage_checkpoint
    keys = list(detector.state_dict())
    assert keys and all(k.startswith(("rpn_network.", "roi_model.RCNN_model.")) for k in keys) and any(k.startswith("roi_model.RCNN_model.") for k in keys)
    path = str(tmp_path / "epoch_3.pt")
    save_two_stage_checkpoint(path, detector, 3, {"lr": 1e-4, "rotated_bbox": False})
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert {"epoch", "backbone_state_dict", "RCNN_dict", "train_args"} <= set(ck) and ck["epoch"] == 3
    plain = D.RCNN(detector.rpn_network.backbone.out_channels, None, 2, OUT)
    plain.load_state_dict(ck["RCNN_dict"], strict=True)                         # the reference's RCNN takes the dict as it is
    other = two_stage(seed=5).eval()
    assert not torch.equal(other.roi_model.RCNN_model.RCNN_cls_score.weight, detector.roi_model.RCNN_model.RCNN_cls_score.weight)
    load_two_stage_checkpoint(path, other)
    for (k, a), (_, b) in zip(detector.state_dict().items(), other.state_dict().items()):
        assert torch.equal(a, b), k


def _keep():
    rows = ROWS // 2
    keep = torch.arange(rows, dtype=torch.int32).repeat(2, 1).cuda()
    return keep, torch.tensor([[rows // 2, rows - rows // 2]] * 2, dtype=torch.int32).cuda()


def _stock(seed, steps=3):
    m = two_stage(seed).train()
    meshes, targets = scenes()
    keep, kc = _keep()
    opt = torch.optim.AdamW([p for p in m.parameters() if p.requires_grad], lr=LR, weight_decay=WD, eps=EPS)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        out = m(list(meshes), targets, keep, kc)
        (out["loss_objectness"] + 2.0 * out["loss_rpn_box_reg"]).backward()
        torch.nn.utils.clip_grad_norm_([p for p in m.parameters() if p.requires_grad], CLIP)
        opt.step()
        losses.append(torch.stack([out["loss_objectness"].detach(), out["loss_rpn_box_reg"].detach()]))
    return m, torch.stack(losses)


def test_three_finetune_steps_match_adamw_and_clip():
    """FinetuneStep over FlatParameters(two_stage) against torch.optim.AdamW + clip_grad_norm_ on a copy, the sampler given the same keep rows on both sides;
    the bound of tests/test_finetune_gpu.py: relerr(A, B) <= 3 * 1e-5 + 4 * relerr(B, B'), B' the stock path's own second run"""
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for, roi_loss_fn
    from nerf_mae_amd.trainer import FusedAdamW
    b, lb = _stock(0)
    b2, lb2 = _stock(0)
    a = two_stage(0).train()
    assert not any(p.requires_grad for p in a.rpn_network.rpn.parameters())
    flat = FlatParameters(a, torch.device("cuda"))
    opt = FusedAdamW(flat, lr=LR, weight_decay=WD, eps=EPS, max_grad_norm=CLIP)
    assert loss_fn_for(a).__code__ is roi_loss_fn(a).__code__
    step = FinetuneStep(flat, opt, loss_fn_for(a), weights={"loss_rpn_box_reg": 2.0})
    meshes, targets = scenes()
    keep, kc = _keep()
    la = []
    for _ in range(3):
        out = step(meshes, targets, keep, kc)
        la.append(torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"]]))
    la = torch.stack(la)
    assert torch.isfinite(la).all() and float(la[:, 0].min()) > 0
    spread = max(relerr(lb2, lb), max(relerr(q, p) for (_, p), (_, q) in zip(C.trainable(b), C.trainable(b2))))
    bound = 3e-5 + 4 * spread
    assert relerr(la, lb) <= bound, (relerr(la, lb), bound)
    for (n, p), (_, q) in zip(C.trainable(b), C.trainable(a)):
        assert relerr(q, p) <= bound, (n, relerr(q, p), bound)
