"""The two stages of the detector joined on the GPU: nerf_mae_amd.rpn.rpn_proposals_dense hands its (boxes, levels, counts) unchanged to
nerf_mae_amd.detector.Classification_Model, against the chain of the two float64 restatements (tests/_rpn_post_ref.proposals -> tests/_roi_head_ref.targets ->
pool -> the tiny head in float64 -> loss / decode; tests/_roi_head_ref.joined_case, joined_chain).

The first stage runs two configurations of tests/test_rpn_post_gpu.py (pre 200, post 100, NMS 0.3, two scenes, axis-aligned and oriented) on its recorded heads;
its four levels are the second stage's pyramid (strides 4 / 8 / 16 / 32, maps 8^3 .. 1^3, C = 4, output 2^3, 12 rows per batch).  "empty" adds a third scene
that hands over no proposal (objectness 20 below, score_thresh 0.5).  Ground truth: three of each scene's own proposals, enlarged and moved.

What is compared exactly is a copy or a decision with a margin: the dense rows as that suite compares them, rows past counts exactly zero; labels, kept
rows and gt_rois on rows that keep 1e-3 on every IoU decision (the kept rows are chosen among those, and among the rows whose pooling grid keeps 1e-3 on every
floor).  Pooled features, losses, decoded boxes and gradients: assert_close(rtol=1e-3), the project's fp32 contract.  With the device sampler the drawn rows
are compared with the sampler's restatement in integers (every row of these scenes keeps 1e-3 from both thresholds, so the candidate lists are exact)."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _roi_head_ref as H  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402
from tests.test_roi_head_gpu import _i32, _model, _state  # noqa: E402
from tests.test_rpn_post_gpu import check_dense, cuda, gen, margins_short  # noqa: E402

pytestmark = pytest.mark.gpu
J = H.JOIN


def _mods():
    from nerf_mae_amd import detector, rpn
    return rpn, detector


@functools.lru_cache(maxsize=None)
def ref(rotated, empty):
    c = H.joined_case(rotated, empty)
    return c, H.joined_chain(c, rotated)


def first_stage(rpn, c, rotated, obj, reg, ori):
    return rpn.rpn_proposals_dense(gen(), R.MESH, obj, reg, ori, J["pre"], J["post"], J["nms"], score_thresh=c["score"], rotated=rotated)


def second_stage(D, rotated, seed=3):
    model = _model(D, rotated, seed)
    model.pooling_model = D.ROIPool(H.GOLD["out"], J["scales"], H.ENLARGE, rotated)
    return model


def _params(model):
    head = model.RCNN_model
    return dict(RCNN_bbox_pred_w=head.RCNN_bbox_pred.weight, RCNN_bbox_pred_b=head.RCNN_bbox_pred.bias, RCNN_cls_score_w=head.RCNN_cls_score.weight,
                RCNN_cls_score_b=head.RCNN_cls_score.bias)


@pytest.mark.parametrize("empty", [False, True], ids=["two-scenes", "with-an-empty-scene"])
@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_proposals_feed_the_second_stage(rotated, empty):
    rpn, D = _mods()
    c, ch = ref(rotated, empty)
    assert not margins_short(c["marg"]), c["marg"]
    assert ch["pm"]["floor"] >= H.MARGIN and ch["pm"]["cell_gap"] >= H.MARGIN and ch["wrap"] >= H.MARGIN, (ch["pm"], ch["wrap"])
    N, Rr, K = len(c["rois"]), c["R"], [r.shape[0] for r in c["rois"]]
    assert all(bool(rm["decided"][k[k >= 0]].all()) for rm, k in zip(c["rows"], c["keep"])), "the kept rows are decided rows"
    assert K[:2] == [100, 100] and (not empty or K[2] == 0) and len(set(ch["Ro"][..., 0].reshape(-1).tolist())) >= 3, "levels are mixed among the kept rows"
    # the first stage, as its own suite compares it
    out = first_stage(rpn, c, rotated, cuda(c["obj"]), cuda(c["reg"]), c["ori"])
    check_dense(out, c["res"], rotated, f"joined {rotated} {empty}")
    boxes, _, levels, _, counts = out
    assert boxes.shape[:2] == (N, J["cap"]) and levels.dtype == torch.int32 and counts.tolist() == K
    dense = (boxes, levels, counts)
    gts, labs = [g.cuda() for g in c["gts"]], [l.cuda() for l in c["labs"]]
    keep, kc = c["keep"], _i32([[nf, Rr - nf] if nf else [0, 0] for nf in c["n_fg"]])
    # targets on the handed-over triple
    labels, rois, gt_rois, kept, _ = [t.cpu() for t in D.roi_targets_dense(boxes, levels, counts, gts, labs, Rr, Rr // 2, H.FG, H.BG, None, True, keep=_i32(keep), keep_counts=kc)]
    assert torch.equal(kept.long(), keep) and torch.equal(labels.double(), ch["L"]) and torch.equal(gt_rois.double(), ch["Gr"]), "labels and matched boxes of decided rows"
    src = torch.cat([levels.cpu().float()[..., None], boxes.cpu()], -1)
    want = torch.stack([src[i][keep[i].clamp_min(0)] * (keep[i] >= 0)[:, None] for i in range(N)])
    assert torch.equal(rois, want), "the sampled RoIs are copies of the dense rows, zero where none was kept"
    assert_close(rois, ch["Ro"], 1e-3, "sampled RoIs")
    # pooling of those RoIs, then the model on the triple: losses, decode, gradients
    model = second_stage(D, rotated)
    leaves = [t.cuda().requires_grad_(True) for t in c["maps"]]
    assert_close(model.pooling_model(leaves, rois.cuda()), ch["pooled"], 1e-3, "pooled")
    (proposals, lab2), probs, loss = model(dense, gts, labs, leaves, is_sample=True, is_reg=True, keep=_i32(keep), keep_counts=kc)
    assert torch.equal(lab2.cpu().double(), ch["L"])
    assert_close(torch.stack([loss["loss_objectness"], loss["loss_rpn_box_reg"]]), torch.stack([ch["loss"]["obj"], ch["loss"]["reg"]]), 1e-3, "losses")
    assert_close(torch.cat(proposals), ch["boxes"], 1e-3, "decoded proposals")
    assert_close(torch.cat(probs), torch.softmax(ch["scores"], 1), 1e-3, "cls_prob")
    (loss["loss_objectness"] + loss["loss_rpn_box_reg"]).backward()
    for k, (leaf, w) in enumerate(zip(leaves, ch["dmaps"])):
        assert_close(leaf.grad, w, 1e-3, f"d map {k}")
        assert (leaf.grad.cpu()[w == 0] == 0).all()
    for name, p in _params(model).items():
        assert_close(p.grad, ch["dparams"][name], 1e-3, f"d {name}")
    if empty:
        assert (labels[2] == -1).all() and not rois[2].any() and not gt_rois[2].any(), "a scene without proposals: label -1, zero rows"
        assert all(not leaf.grad[2].any() for leaf in leaves), "and no gradient to its maps"
        assert int((ch["L"] >= 0).sum()) == 2 * Rr, "both losses are means over the other scenes' rows alone"
    # evaluation: lists sized by the counts, labels of the decided rows
    (ev_rois, ev_labels), ev_probs, ev_loss = model(dense, gts, labs, [t.detach() for t in leaves], is_sample=False)
    assert ev_loss == 0. and [p.shape[0] for p in ev_probs] == K and [r.shape[0] for r in ev_rois] == K and [l.shape[0] for l in ev_labels] == K
    L_ev = H.targets(c["rois"], c["gts"], c["labs"], rows=c["rows"])[0]
    for got, w, rm in zip(ev_labels, L_ev, c["rows"]):
        assert torch.equal(got.cpu().double()[rm["decided"]], w[rm["decided"]])


@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_joined_stages_never_wait_and_replay_in_one_graph(rotated):
    """proposals -> targets with the device sampler -> pooling -> head -> losses -> backward: no host synchronisation, and the whole chain in one graph whose
    replays draw the rows that the sampler's restatement draws for their counters"""
    rpn, D = _mods()
    c, _ = ref(rotated, False)
    assert not margins_short(c["marg"])
    assert all(bool(((rm["d_fg"] >= H.MARGIN) & (rm["d_bg"] >= H.MARGIN)).all()) for rm in c["rows"]), "every row keeps 1e-3 from both thresholds: the candidate lists are exact"
    assert all(f.numel() and b.numel() for f, b in c["candidates"])
    seed = 9
    model = second_stage(D, rotated, seed=seed)
    gobj, greg, gori = cuda(c["obj"]), cuda(c["reg"]), torch.tensor(c["ori"], dtype=torch.int32).cuda()
    gts, labs = [g.cuda() for g in c["gts"]], [l.cuda() for l in c["labs"]]
    base = [t.cuda() for t in c["maps"]]
    params = list(model.RCNN_model.parameters())
    Rr, want_fg = model.sample_model._sizes(2)
    assert (Rr, want_fg) == (c["R"], c["R"] // 2)

    def run(obj, reg, leaves):
        boxes, _, levels, _, counts = first_stage(rpn, c, rotated, obj, reg, gori)
        (sample_rois, labels), _, loss = model((boxes, levels, counts), gts, labs, leaves, is_sample=True)
        grads = torch.autograd.grad(loss["loss_objectness"] + loss["loss_rpn_box_reg"], leaves + params)
        return [loss["loss_objectness"].detach(), loss["loss_rpn_box_reg"].detach(), torch.stack(sample_rois).detach(), labels, boxes, levels, counts] + list(grads)

    def expected(out, counter):
        """the rows that the restated sampler keeps, copied from the dense triple of this run"""
        boxes, levels, counts = [t.cpu() for t in out[4:7]]
        assert counts.tolist() == [r.shape[0] for r in c["rois"]]
        rows, labels = [], []
        for i, (f, b) in enumerate(c["candidates"]):
            keep, (nf, _), _ = H.sample(f, b, Rr, want_fg, seed, counter, i)
            assert len(set(map(tuple, boxes[i, :counts[i]].tolist()))) == counts[i], "distinct rows: equal RoIs mean equal kept indices"
            rows.append(torch.cat([levels[i].float()[:, None], boxes[i]], 1)[torch.tensor(keep)])
            labels.append(torch.tensor([1.0] * nf + [0.0] * (Rr - nf)))
        return torch.stack(rows), torch.stack(labels)

    def same_rows(sampled, rows):
        """the returned RoIs (without their level) are exact copies; with remap off an oriented RoI comes back with its sizes enlarged (detector.py's header)"""
        rows = rows[..., 1:]
        if not rotated:
            return torch.equal(sampled, rows)
        return torch.equal(sampled[..., [0, 1, 2, 6]], rows[..., [0, 1, 2, 6]]) and torch.allclose(sampled[..., 3:6], rows[..., 3:6] * (1 + H.ENLARGE), rtol=1e-6, atol=0)

    leaves = [t.clone().requires_grad_(True) for t in base]
    run(gobj, greg, leaves)                                  # plans and the sampler's state are made on the first call
    torch.cuda.synchronize()
    model.sample_model.rng_state.copy_(_state(seed, 40))
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = run(gobj, greg, leaves)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    rows, labels = expected(eager, 40)
    assert same_rows(eager[2].cpu(), rows) and torch.equal(eager[3].cpu(), labels), "the eager draw is the restated one"
    assert model.sample_model.rng_state.cpu().tolist() == [seed, 41]

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                               # leaves made, warmed up and captured on one side stream (Capture)
        obj2, reg2 = [torch.zeros_like(t) for t in gobj], [torch.zeros_like(t) for t in greg]
        leaves = [t.clone().requires_grad_(True) for t in base]
        run(obj2, reg2, leaves)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(obj2, reg2, leaves)
    for d, t in zip(obj2 + reg2, gobj + greg):               # the heads' values copied in
        d.copy_(t)
    model.sample_model.rng_state.copy_(_state(seed, 100))
    seen = []
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t.float()).all() for t in out), f"replay {k}"
        assert out[0].item() > 0 and any((g != 0).any() for g in out[7:7 + len(leaves)])
        rows, labels = expected(out, 100 + k)
        assert same_rows(out[2].cpu(), rows) and torch.equal(out[3].cpu(), labels), f"replay {k} draws the restated rows of counter {100 + k}"
        seen.append(out[2].clone())
    assert model.sample_model.rng_state.cpu().tolist() == [seed, 102], "the counter advances inside the graph"
    assert not torch.equal(seen[0], seen[1]), "the replays draw different samples"
