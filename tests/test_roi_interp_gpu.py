"""The "interpolation" RoI feature type on the GPU (nerf_mae_amd.detector.ROIPool(is_rotated_bbox=True, feature_extracting_type="interpolation") over
csrc/roi_head.hip's roi_interp kernels) against the float64 restatement of tests/_roi_interp_ref.py (itself checked against the recorded reference,
tests/golden/g31_roi_interp.npz, and against F.interpolate in tests/test_roi_interp_ref_cpu.py).

Tolerance: the project's contract for fp32, assert_close(rtol=1e-3), on the features and on every level's map gradient, no element left out.  The only discrete
decisions are those of the sampling grid (ceil, floor, the in-map test); every input keeps 1e-3 on them (asserted before each comparison; fp32 errs by about 1e-6
on a grid position).  Exact zeros are asserted only where they are exact by construction: rows of an invalid level, rows whose every grid point lies outside
the map, the gradient slice of a scene that has only such rows, the gradient of a level no RoI uses.  Elsewhere an fp32 resampling weight may be 1e-7 where
float64 has 0.  Inputs: the oriented sets of tests/_roi_head_ref.py on the 32^3 and 32 x 24 x 16 meshes (C = 5 with output (3,2,1): channel tail, an output axis
of 1; C = 8 with (2,2,2) on non-cubic maps; C = 20 with (5,4,3): three channel groups, the last ragged; C = 12 with (7,7,7): three workgroups per RoI), the
four-level set and the remap set.  Measured on an MI355X (NMH_PRINT_ERR=1): DESIGN.md 3.13."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _roi_head_ref as H  # noqa: E402
from tests import _roi_interp_ref as I  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g31_roi_interp.npz"))


def _m():
    from nerf_mae_amd import detector
    return detector


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).cuda()


def _pool(M, c):
    remap = c["levels"] is not None
    return M.ROIPool(c["out"], c["scales"], H.ENLARGE, True, "interpolation", H.GOLD["max_res"] if remap else 200, remap)


# ---- 1. forward and backward ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I.CASES)
def test_interpolation_forward_and_backward(name):
    M = _m()
    c = I.case(name)
    m = c["facts"]
    assert m["floor"] >= I.MARGIN and m["masked_points"] > 0 and (m["all_masked"] >= 1 or not c["noncubic"]), m
    pool = _pool(M, c)
    if c["levels"] is not None:
        assert torch.equal(pool.map_levels(c["rois"][..., 1:].cuda()).cpu(), c["levels"]), "the level mapper gives the restatement's levels"
    leaves = [t.cuda().requires_grad_(True) for t in c["maps"]]
    got = pool(leaves, c["rois"].cuda())
    assert got.shape == c["res"].shape and got.dtype == torch.float32
    assert_close(got, c["res"], 1e-3, f"interpolated, {name}")
    for r in m["all_masked_rows"]:
        assert not got[r].any(), "a RoI wholly outside its map gives exact zeros"
    got.backward(c["dout"].cuda())
    for k, (leaf, want) in enumerate(zip(leaves, c["dmaps"])):
        assert_close(leaf.grad, want, 1e-3, f"d map {k}, {name}")
    # the reference's per-scene lists give the same features
    lists = pool([[t[i].cuda() for t in c["maps"]] for i in range(c["rois"].shape[0])], [r.cuda() for r in c["rois"]])
    assert torch.equal(torch.cat(lists), got.detach())
    lists = pool([t.cuda() for t in c["maps"]], [c["rois"][0, :5].cuda(), c["rois"][1].cuda()])
    R = c["rois"].shape[1]
    assert [t.shape[0] for t in lists] == [5, R] and torch.equal(lists[0], got.detach()[:5]) and torch.equal(lists[1], got.detach()[R:])


def test_the_cases_cover_every_relation_of_grid_and_output_size():
    facts = [I.case(n)["facts"] for n in I.CASES]
    assert all(sum(f[k] for f in facts) > 0 for k in ("axes_lt", "axes_eq", "axes_gt", "axes_one"))


# ---- 2. exact zeros ------------------------------------------------------------------------------------------------------------------------
def test_exact_zeros_where_they_hold_by_construction():
    """rows of an invalid level (-1 and 7); a scene whose RoIs are all invalid or wholly outside the map; a level no RoI uses"""
    M = _m()
    c = I.zeros_case()
    rois, res, m, dmaps = c["rois"], c["res"], c["facts"], c["dmaps"]
    R = rois.shape[1]
    assert m["floor"] >= I.MARGIN and m["levels_used"] == {0, 1} and c["distinct_outside"] >= 2, m
    assert {2, 5, R, R + 1} <= set(c["invalid"]) and set(range(R, 2 * R)) <= set(m["all_masked_rows"]) | {R, R + 1}, "every valid row of scene 1 is wholly outside"
    leaves = [t.cuda().requires_grad_(True) for t in c["maps"]]
    got = _pool(M, c)(leaves, rois.cuda())
    assert_close(got, res, 1e-3, "interpolated, with invalid levels")
    for r in c["invalid"]:
        assert not got[r].any(), "a level outside 0 .. L-1 gives zeros"
    assert not got[R:].any(), "the scene of RoIs wholly outside"
    assert got[:R].abs().sum() > 0
    got.backward(c["dout"].cuda())
    for k, (leaf, want) in enumerate(zip(leaves, dmaps)):
        assert_close(leaf.grad, want, 1e-3, f"d map {k}, with invalid levels")
        assert not leaf.grad[1].any(), "the scene of RoIs wholly outside takes no gradient"
    assert not leaves[2].grad.any(), "a level no RoI uses takes no gradient"
    assert leaves[0].grad[0].abs().sum() > 0 and leaves[1].grad[0].abs().sum() > 0


def test_a_map_that_needs_no_gradient_gets_none():
    M = _m()
    c = I.case("cubic-C5-3x2x1")
    leaves = [t.cuda().requires_grad_(k != 1) for k, t in enumerate(c["maps"])]
    _pool(M, c)(leaves, c["rois"].cuda()).backward(c["dout"].cuda())
    assert leaves[1].grad is None
    for k in (0, 2):
        assert_close(leaves[k].grad, c["dmaps"][k], 1e-3, f"d map {k}, level 1 frozen")


# ---- 3. the model ----------------------------------------------------------------------------------------------------------------------------
def _model(M, seed=3):
    layer = M.ProposalTargetLayer(2, batch_size=H.GOLD["N"] * H.GOLD["R"], fg_fraction=0.5, fg_threshold=H.FG, bg_threshold=H.BG, is_rotated_bbox=True, seed=seed)
    pool = M.ROIPool(H.GOLD["out"], H.SCALES, H.ENLARGE, True, "interpolation", H.GOLD["max_res"], False)
    head = M.RCNN(H.GOLD["C"], None, 2, H.GOLD["out"], is_add_layer=False, is_rotated_bbox=True, is_flatten=True).cuda()
    hp = H.gold_head(True)
    with torch.no_grad():
        head.RCNN_bbox_pred.weight.copy_(hp["RCNN_bbox_pred_w"]); head.RCNN_bbox_pred.bias.copy_(hp["RCNN_bbox_pred_b"])
        head.RCNN_cls_score.weight.copy_(hp["RCNN_cls_score_w"]); head.RCNN_cls_score.bias.copy_(hp["RCNN_cls_score_b"])
    return M.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=True)


def _keep():
    keep, n_fg = GOLD["keep"], GOLD["n_fg"]
    return _i32(keep), _i32(np.stack([n_fg, keep.shape[1] - n_fg], 1))


def test_classification_model_against_the_recorded_run():
    M = _m()
    rois, gts, labs, maps = H.gold_inputs(True)
    kept = torch.stack([r[torch.as_tensor(k)] for r, k in zip(rois, GOLD["keep"])])
    assert I.interp(maps, kept, out=H.GOLD["out"])[1]["floor"] >= I.MARGIN
    model = _model(M)
    keep, kc = _keep()
    before = [r.clone() for r in rois]
    args = ([r.cuda() for r in rois], [g.cuda() for g in gts], [l.cuda() for l in labs], [t.cuda() for t in maps])
    assert_close(model.pooling_model(args[3], kept.cuda()), torch.as_tensor(GOLD["pooled"]), 1e-3, "recorded features")
    (proposals, labels), probs, loss = model(*args, is_sample=True, is_reg=True, keep=keep, keep_counts=kc)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(args[0], before)), "the caller's RoIs are not written to"
    assert torch.equal(labels.cpu().long(), torch.as_tensor(GOLD["sample_labels"]))
    assert_close(torch.stack([loss["loss_objectness"], loss["loss_rpn_box_reg"]]), torch.as_tensor(GOLD["losses"]), 1e-3, "losses")
    assert_close(torch.cat(proposals), torch.as_tensor(GOLD["proposals"]), 1e-3, "decoded proposals")
    assert_close(torch.cat(probs), torch.as_tensor(GOLD["cls_prob"]), 1e-3, "cls_prob")
    (sample_rois, _), _, _ = model(*args, is_sample=True, is_reg=False, keep=keep, keep_counts=kc)
    assert_close(torch.cat(sample_rois), torch.as_tensor(GOLD["encoded_rois"]), 1e-6, "the returned RoIs are the ones the reference encoded against")


class _Maps(torch.nn.Module):
    """stands where the backbone and the FPN stand: trainable maps, so that the step's gradient has to come through the interpolation's backward"""

    def __init__(self, maps):
        super().__init__()
        self.maps, self.out_channels = torch.nn.ParameterList([torch.nn.Parameter(m.clone()) for m in maps]), maps[0].shape[1]

    def forward(self, x):
        return list(self.maps)


class _Proposals(torch.nn.Module):
    """stands where the RPN stands: hands out the recorded scenes' RoIs as the dense triple"""
    rotate = True

    def __init__(self, rois):
        super().__init__()
        d = torch.stack(rois)
        self.dense = (d[..., 1:].contiguous().cuda(), d[..., 0].to(torch.int32).cuda(), _i32([r.shape[0] for r in rois]))

    def proposals_dense(self, x, features, ori):
        return self.dense[0], None, self.dense[1], None, self.dense[2]


class _FirstStage(torch.nn.Module):
    def __init__(self, rois, maps):
        super().__init__()
        self.backbone, self.rpn = _Maps(maps), _Proposals(rois)

    def transform(self, meshes):
        return meshes, None


def test_one_finetune_step_through_roi_loss_fn():
    """TwoStageDetector over the recorded scenes with the interpolation ROIPool: FinetuneStep(roi_loss_fn) returns the recorded losses and moves the head and,
    through the interpolation's backward, the maps"""
    M = _m()
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for, roi_loss_fn
    from nerf_mae_amd.trainer import FusedAdamW
    rois, gts, _, maps = H.gold_inputs(True)
    det = M.TwoStageDetector(_FirstStage(rois, maps), _model(M), 0.05, 0.3).cuda().train()
    assert det.roi_model.pooling_model.feature_extracting_type == "interpolation"
    flat = FlatParameters(det, torch.device("cuda"))
    opt = FusedAdamW(flat, lr=1e-2, weight_decay=0.0, eps=1e-8, max_grad_norm=1.0)
    assert loss_fn_for(det).__code__ is roi_loss_fn(det).__code__
    step = FinetuneStep(flat, opt, roi_loss_fn(det))
    start = {n: p.detach().clone() for n, p in det.named_parameters() if p.requires_grad}
    assert any(n.startswith("rpn_network.backbone.maps") for n in start)
    keep, kc = _keep()
    out = step([torch.zeros((1, *H.MESH), device="cuda")] * 2, [g.cuda() for g in gts], keep, kc)
    assert_close(torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"]]), torch.as_tensor(GOLD["losses"]), 1e-3, "losses of the step")
    for n, p in det.named_parameters():
        if n in start:
            assert torch.isfinite(p).all() and not torch.equal(p.detach(), start[n]), f"{n} is finite and has moved"


# ---- 4. capture ------------------------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_in_a_captured_graph():
    M = _m()
    c = I.case("cubic-C20-5x4x3")
    pool, rois, dout = _pool(M, c), c["rois"].cuda(), c["dout"].cuda()
    base = [t.cuda() for t in c["maps"]]

    def run(leaves):
        out = pool(leaves, rois)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, dout))

    eager = run([t.clone().requires_grad_(True) for t in base])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        leaves = [t.clone().requires_grad_(True) for t in base]
        run(leaves)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(leaves)
    for replay in range(2):
        for t in out:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]), f"replay {replay}: the forward is bit-equal to the eager one"
        for k, (g, want) in enumerate(zip(out[1:], c["dmaps"])):
            assert_close(g, want, 1e-3, f"replay {replay}: d map {k}")


# ---- 5. error paths --------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    M = _m()
    c = I.case("cubic-C5-3x2x1")
    pool = _pool(M, c)
    dev, r = [t.cuda() for t in c["maps"]], c["rois"].cuda()
    pool(dev, r)
    with pytest.raises(TypeError):
        pool([t.double() for t in dev], r)
    with pytest.raises(TypeError):
        pool(dev, r.double())
    with pytest.raises(RuntimeError):
        pool(c["maps"], r)
    with pytest.raises(RuntimeError):
        pool(dev, c["rois"])
    for bad_maps, bad_rois in ((dev[:2], r), (dev, r[:1]), (dev, r[..., :7]), ([dev[0], dev[1], dev[2][:, :2]], r), (dev, r[0])):
        with pytest.raises(ValueError):
            pool(bad_maps, bad_rois)
    with pytest.raises(NotImplementedError):
        M.ROIPool([2, 2, 2], [2, 4, 8], feature_extracting_type="interpolation")
    with pytest.raises(ValueError):
        M.ROIPool([2, 2, 2], [2, 4, 8], is_rotated_bbox=True, feature_extracting_type="nearest")
    from nerf_mae_amd import ops
    plan = ops.RoiPoolPlan(dev, H.SCALES, (2, 2, 2), 1.2, 6)
    with pytest.raises(RuntimeError):                                        # the C ABI refuses axis-aligned rows (ncols != 7): an argument error, no launch
        ops.roi_interp_fwd(plan, dev, r[..., :7].contiguous(), None)
    with pytest.raises(RuntimeError):
        ops.roi_interp_bwd(plan, c["dout"].cuda(), r[..., :7].contiguous(), None, [True] * 3)
