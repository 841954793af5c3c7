"""CPU (-m "not gpu"): tests/_roi_post_ref.py, the float64 restatement of the RoI post-processing, against results recorded from the reference's own
filter_proposals (tests/golden/g27_roi_post.npz, tools/gen_golden_roi_post.py) and against known answers; and the constructed cases of
tests/test_roi_post_gpu.py hold every decision with a margin."""
import os

import numpy as np
import pytest
import torch

from tests import _roi_post_ref as P

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g27_roi_post.npz")
TAGS = {0.5: "_t50", 0.8: "_t80", 0.3: "_t30"}


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def _run(rotated, thr, mode="any"):
    probs, rois, counts, mesh = P.gold_dense(rotated)
    return P.postprocess(probs, None, rois, counts, mesh, thr, P.GOLD["nms_thresh"], P.MIN_SIZE, False, mode, probabilities=True)


@pytest.mark.parametrize("rotated", [False, True])
def test_recorded_inputs_are_the_generators(gold, rotated):
    pre = "o_" if rotated else "a_"
    boxes, probs, _ = P.gold_inputs(rotated)
    assert int(gold[pre + "seed"]) == P.GOLD_SEED[rotated]
    np.testing.assert_allclose(P.input_sums(boxes, probs), gold[pre + "input_sums"], rtol=1e-12)
    assert float(gold["nms_thresh"]) == P.GOLD["nms_thresh"] and float(gold["min_size"]) == P.MIN_SIZE and tuple(gold["thresholds"]) == P.GOLD["thresholds"]


@pytest.mark.parametrize("thr", [0.5, 0.8, 0.3])
@pytest.mark.parametrize("rotated", [False, True])
def test_restatement_reproduces_the_reference(gold, rotated, thr):
    pre, tag = "o_" if rotated else "a_", TAGS[thr]
    res, m = _run(rotated, thr)
    assert all(v >= P.MARGIN for v in m.values()), m
    counts = [len(r["scores"]) for r in res]
    assert counts == gold[pre + "counts" + tag].tolist() and sum(counts) > 0
    assert torch.cat([r["index"] for r in res]).tolist() == gold[pre + "index" + tag].tolist()            # kept rows and their order
    np.testing.assert_allclose(torch.cat([r["boxes"] for r in res]).numpy(), gold[pre + "boxes" + tag], rtol=0, atol=1e-9)
    np.testing.assert_allclose(torch.cat([r["scores"] for r in res]).numpy(), gold[pre + "probs" + tag][:, 1], rtol=0, atol=1e-9)


@pytest.mark.parametrize("rotated", [False, True])
def test_duplicate_rows_share_their_fate(rotated):
    """at 0.3 the reference's 2-D torch.where hands rows with both probabilities >= 0.3 to the NMS twice; the results are those without the copies"""
    boxes, probs, mesh = P.gold_inputs(rotated)
    res, _ = _run(rotated, 0.3)
    doubled = 0
    for b, p, ms, r in zip(boxes, probs, mesh, res):
        idx, bx, sc = P.reference_literal(b, p, ms, 0.3, P.GOLD["nms_thresh"])
        doubled += int(((p.double() >= 0.3).sum(1) == 2).sum())
        assert idx.tolist() == r["index"].tolist()
        assert torch.equal(bx, r["boxes"]) and torch.equal(sc, r["scores"])
    assert doubled > 0


@pytest.mark.parametrize("rotated", [False, True])
def test_any_at_half_keeps_every_row_that_survives_clip_and_size(rotated):
    probs, rois, counts, mesh = P.gold_dense(rotated)
    marg = P.new_margins()
    any_, _ = _run(rotated, 0.5, "any")
    obj, _ = _run(rotated, 0.5, "object")
    for b in range(len(counts)):
        _, p, ok = P.candidates(probs[b], None, rois[b], mesh[b], 0.0, P.MIN_SIZE, False, "any", marg, probabilities=True)
        assert torch.equal(any_[b]["cand_ok"], ok)                                 # the threshold removed nothing
        assert torch.equal(obj[b]["cand_ok"], ok & (p[:, 1] >= 0.5)) and obj[b]["cand_ok"].sum() < ok.sum()
    if not rotated:
        assert not any_[0]["cand_ok"][3]                                           # the box thinner than min_size


def test_known_answers():
    """three boxes in a row, IoU(0,1) = IoU(1,2) = 1/3 and IoU(0,2) = 0: box 1 falls to box 0, box 2 stays; a box outside is clipped away; equal scores go to
    the lower row"""
    b = torch.tensor([[0, 0, 0, 4, 4, 4], [2, 0, 0, 6, 4, 4], [4, 0, 0, 8, 4, 4], [-5, 0, 0, -1, 4, 4], [20, 20, 20, 24, 24, 24], [20, 20, 20, 24, 24, 24]], dtype=torch.float32)
    rois = torch.cat([torch.zeros(6, 1), b], 1)[None]
    logits = torch.tensor([[0.0, 2.0], [0.0, 1.5], [0.0, 1.0], [0.0, 3.0], [0.0, 0.5], [0.0, 0.5]])[None]
    res, m = P.postprocess(logits, None, rois, [6], [(32, 32, 32)], 0.5, 0.3, P.MIN_SIZE, False, "any")
    assert res[0]["index"].tolist() == [0, 2, 4]
    assert abs(m["m_iou"] - (1 / 3 - 0.3)) < 1e-12
    np.testing.assert_allclose(res[0]["scores"].numpy(), torch.sigmoid(torch.tensor([2.0, 1.0, 0.5], dtype=torch.float64)).numpy(), rtol=1e-12)
    res, _ = P.postprocess(logits, None, rois, [6], [(32, 32, 32)], 0.8, 0.3, P.MIN_SIZE, False, "object")
    assert res[0]["index"].tolist() == [0]                                         # sigmoid(1.5) = 0.818 passes the threshold, then box 0 removes it
    res, _ = P.postprocess(logits, None, rois, [2], [(32, 32, 32)], 0.5, 0.5, P.MIN_SIZE, False, "any")
    assert res[0]["index"].tolist() == [0, 1]                                      # counts cut the rows; 1/3 <= 0.5 keeps both


@pytest.mark.parametrize("case", ["small", "large"])
@pytest.mark.parametrize("rotated", [False, True])
def test_constructed_cases_hold_every_decision(rotated, case):
    from tests.test_roi_post_gpu import LARGE, SMALL, constructed
    for cfg in (SMALL if case == "small" else LARGE):
        inp, kw = constructed(rotated, cfg)
        res, m = P.postprocess(**inp, **kw)
        assert all(v >= P.MARGIN for v in m.values()), (cfg, m)
        assert sum(len(r["scores"]) for r in res) > 0
