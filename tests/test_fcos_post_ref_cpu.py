"""The float64 restatement of the FCOS inference post-processing (tests/_fcos_post_ref.py) against results recorded from the reference's own
FCOSPostProcessor (tests/golden/g19_fcos_post.npz, tools/gen_golden_fcos_post.py) and against hand-made known answers.  No GPU."""
import math
import os

import numpy as np
import pytest
import torch

from tests import _fcos_post_ref as P
from tests import _fcos_ref as F

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g19_fcos_post.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope="module", params=[False, True], ids=["aabb", "obb"])
def recorded(request, golden):
    use_obb = request.param
    pre = "o_" if use_obb else "a_"
    seed = int(golden[pre + "head_seed"])
    assert seed == P.HEAD_SEED[use_obb]
    locs, cls, reg, ctr, sizes, masks = P.inputs(seed, use_obb)
    sums = np.array([sum(t.double().sum().item() for t in ts) for ts in (cls, reg, ctr)])
    np.testing.assert_allclose(sums, golden[pre + "head_sums"], rtol=1e-12)        # the generator has not drifted
    cfg = dict(pre_nms_thresh=float(golden["pre_nms_thresh"]), pre_nms_top_n=int(golden["pre_nms_top_n"]), nms_thresh=float(golden["nms_thresh"]),
               fpn_post_nms_top_n=int(golden["fpn_post_nms_top_n"]), min_size=float(golden["min_size"]))
    assert cfg == P.CFG
    res, marg = P.postprocess(locs, cls, reg, ctr, sizes, masks, **cfg)
    return pre, res, marg


def test_restatement_reproduces_the_reference(recorded, golden):
    pre, res, _ = recorded
    counts = golden[pre + "counts"]
    assert [len(r["scores"]) for r in res] == counts.tolist()
    assert torch.cat([r["level"] for r in res]).tolist() == golden[pre + "level"].tolist()
    assert torch.cat([r["index"] for r in res]).tolist() == golden[pre + "index"].tolist()
    boxes, scores = torch.cat([r["boxes"] for r in res]).numpy(), torch.cat([r["scores"] for r in res]).numpy()
    assert np.abs(boxes - golden[pre + "boxes"]).max() <= 1e-7 * max(1.0, np.abs(golden[pre + "boxes"]).max())
    assert np.abs(scores - golden[pre + "scores"]).max() <= 1e-7


def test_recorded_inputs_have_a_margin_on_every_decision(recorded):
    _, res, marg = recorded
    assert set(marg) == {"m_thresh", "m_topk", "m_size", "m_iou", "m_post", "m_order"}
    assert all(v >= P.MARGIN for v in marg.values()), marg
    # NMS does real work on these inputs, two levels are cut by the top-k and the post-NMS cut is active
    assert all(len(r["pre_scores"]) > 3 * len(r["scores"]) for r in res) and all(len(r["scores"]) == 100 for r in res)
    assert all(math.isfinite(marg[k]) for k in ("m_topk", "m_post", "m_iou"))


# ---- hand-made known answers -------------------------------------------------------------------------------------------------------------
def _one(cls, ctr, reg, loc, size=(64, 64, 64), mask=None, **cfg):
    """one level, one scene, flat lists -> the scene's result"""
    n = len(cls)
    c = dict(pre_nms_thresh=0.05, pre_nms_top_n=1000, nms_thresh=0.3, fpn_post_nms_top_n=0, min_size=0.0)
    c.update(cfg)
    t = lambda v, ch: torch.tensor(v, dtype=torch.float64).reshape(n, ch).t().reshape(1, ch, n, 1, 1)      # noqa: E731
    masks = None if mask is None else [torch.tensor(mask, dtype=torch.bool).reshape(1, n)]
    res, _ = P.postprocess([torch.tensor(loc, dtype=torch.float64).reshape(n, 3)], [t(cls, 1)], [t(reg, len(reg[0]))], [t(ctr, 1)], [size], masks, **c)
    return res[0]


def test_one_location():
    r = _one([0.0], [0.0], [[1, 2, 3, 4, 5, 6]], [[10, 10, 10]])
    assert r["level"].tolist() == [0] and r["index"].tolist() == [0]
    assert r["boxes"].tolist() == [[9.0, 8.0, 7.0, 14.0, 15.0, 16.0]]
    assert r["scores"].tolist() == [0.5]                    # sqrt(0.5 * 0.5)
    r = _one([0.0], [0.0], [[1, 2, 3, 4, 5, 6]], [[10, 10, 10]], size=(12, 64, 15))
    assert r["boxes"].tolist() == [[9.0, 8.0, 7.0, 12.0, 15.0, 15.0]]          # clipped to the scene
    r = _one([0.0], [0.0], [[1, 2, 3, 4, 5, 6]], [[10, 10, 10]], min_size=5.5)
    assert r["scores"].numel() == 0                          # the x side is 5
    r = _one([0.0], [0.0], [[2, 1, 3, 2, 1, 3, 0, 0]], [[10, 10, 10]])
    assert torch.allclose(r["boxes"], torch.tensor([[10.0, 10.0, 10.0, 2 * math.sqrt(2), 2 * math.sqrt(2), 6.0, math.pi / 4]], dtype=torch.float64), atol=1e-6)


def test_empty_results():
    reg, loc = [[1, 1, 1, 1, 1, 1]] * 4, [[4, 4, 4], [12, 4, 4], [20, 4, 4], [28, 4, 4]]
    r = _one([3.0] * 4, [0.0] * 4, reg, loc, mask=[False] * 4)
    assert r["scores"].numel() == 0 and r["boxes"].shape == (0, 6) and r["pre_scores"].numel() == 0       # an all-padding scene
    r = _one([30.0] * 4, [0.0] * 4, reg, loc, pre_nms_thresh=1.0)
    assert r["scores"].numel() == 0                          # p > 1 never holds
    r = _one([3.0] * 4, [0.0] * 4, reg, loc, mask=[False, True, False, True])
    assert sorted(r["index"].tolist()) == [1, 3]


def test_equal_logits_go_to_the_first_locations():
    n = 10
    reg, loc = [[1, 1, 1, 1, 1, 1]] * n, [[4 + 8 * i, 4, 4] for i in range(n)]         # disjoint boxes: NMS keeps all
    r = _one([1.0] * n, [0.5] * n, reg, loc, pre_nms_top_n=4)
    assert r["pre_index"].tolist() == [0, 1, 2, 3] and r["index"].tolist() == [0, 1, 2, 3]
    r = _one([1.0] * n, [0.5] * 5 + [0.7] + [0.5] * 4, reg, loc, pre_nms_top_n=4)
    assert r["pre_index"].tolist() == [0, 1, 2, 5] and r["index"].tolist() == [5, 0, 1, 2]
    # the post-NMS cut keeps every box that ties with the cut score (the reference's kthvalue rule)
    r = _one([1.0] * n, [0.9] + [0.5] * 9, reg, loc, fpn_post_nms_top_n=3)
    assert r["index"].tolist() == list(range(n))
    r = _one([1.0] * n, [0.9, 0.8, 0.7] + [0.5] * 7, reg, loc, fpn_post_nms_top_n=3)
    assert r["index"].tolist() == [0, 1, 2]


def test_suppression_and_levels():
    # two nested boxes (IoU 0.512 > 0.3) and one apart; the higher score wins
    reg, loc = [[5, 5, 5, 5, 5, 5], [4, 4, 4, 4, 4, 4], [2, 2, 2, 2, 2, 2]], [[10, 10, 10], [10, 10, 10], [40, 40, 40]]
    r = _one([0.0, 1.0, -1.0], [0.0] * 3, reg, loc)
    assert r["index"].tolist() == [1, 2]
    r = _one([0.0, 1.0, -1.0], [0.0] * 3, reg, loc, nms_thresh=0.6)
    assert r["index"].tolist() == [1, 0, 2]
    r = _one([0.0, 1.0, -1.0], [0.0] * 3, reg, loc, bbox_aug_enabled=True)
    assert r["index"].tolist() == [0, 1, 2]
