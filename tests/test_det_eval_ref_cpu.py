"""The float64 restatement of the detection metrics (tests/_det_eval_ref.py) against results recorded from the reference's own eval.py
(tests/golden/g26_det_eval.npz, tools/gen_golden_det_eval.py: an fp32 run, the only precision the reference runs in) and against hand cases.

Tolerances.  Integer results (num_pos, num_det, the cumulative true positives recovered as rint(recalls num_gt), hence every per-detection flag) are exact.
gt_overlaps and recalls: the project's contract for fp32, assert_close(rtol=1e-3).  Measured on this generator, the fp32 recording against the float64
restatement: gt_overlaps differ by at most 1.9e-7 absolute with 6 columns and 1.3e-5 with 7 (the reference's fp32 vertex-list intersection; relative to the
values, 3e-5), recalls and precisions by at most 3e-8.  The seed keeps every decision at least 1e-5 away (conditions 1 and 2, asserted here from the
restatement; on the oriented scenes the recall margin is 7.6e-4), and the recorded decisions are checked to be the restatement's.
ap: n_terms 2^-23 absolute, n_terms the number of recall steps: the reference sums n_terms fp32 products of factors in [0, 1] (tests/_det_eval_ref.ap_bound)."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _det_eval_ref as E  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

CASES = (("a_", 6), ("o_", 7))


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


@pytest.mark.parametrize("pre,ncols", CASES, ids=("aabb", "obb"))
def test_generated_scenes_meet_the_five_conditions(pre, ncols, golden):
    g = golden("g26_det_eval.npz")
    scenes = E.make_scenes(E.SEED[ncols], ncols)
    assert int(g[pre + "seed"]) == E.SEED[ncols]
    assert [(len(s[0]), len(s[2])) for s in scenes] == list(E.SCENES) and g["shapes"].tolist() == [list(s) for s in E.SCENES[:E.RECORDED]]
    np.testing.assert_allclose(E.input_sums(scenes), g[pre + "input_sums"], rtol=1e-12)
    m = E.decision_margins(scenes)
    print(m)
    assert m["recall_thr"] >= E.MARGIN and m["ap_thr"] >= E.MARGIN, m          # condition 1
    assert m["greedy_gap"] >= E.MARGIN and m["argmax_gap"] >= E.MARGIN, m       # condition 2
    assert m["score_gap"] > 0, m                                                # condition 3
    assert m["column_max_differs"], m                                           # condition 4
    assert m["claimed_fp"] >= 1, m                                              # condition 5
    assert E.conditions_hold(m)


@pytest.mark.parametrize("pre,ncols", CASES, ids=("aabb", "obb"))
def test_recall_against_the_recording(pre, ncols, golden):
    g = golden("g26_det_eval.npz")
    scenes = E.make_scenes(E.SEED[ncols], ncols)[:E.RECORDED]
    ious = E.iou_matrices(scenes)
    for limit in E.LIMITS:
        for lo in (0.5, 0.25):
            key = f"{pre}r{limit}_t{int(lo * 100)}_"
            r = E.recall(scenes, E.recall_thresholds(lo), limit, ious)
            assert r["num_pos"] == int(g[key + "num_pos"]) == sum(G for P, G in E.SCENES[:E.RECORDED] if P and G)
            print(key, "max |gt_overlaps - recorded|", np.abs(r["gt_overlaps"] - g[key + "gt_overlaps"]).max(), "recalls", np.abs(r["recalls"] - g[key + "recalls"]).max())
            assert_close(_t(r["gt_overlaps"]), _t(g[key + "gt_overlaps"]), 1e-3, key + "gt_overlaps")
            assert_close(_t(r["recalls"]), _t(g[key + "recalls"]), 1e-3, key + "recalls")
            assert_close(_t([r["ar"]]), _t([g[key + "ar"]]), 1e-3, key + "ar")
            # the same decisions: the number of overlaps at or above each threshold
            assert [(r["gt_overlaps"] >= np.float64(t)).sum() for t in r["thresholds"]] == [(g[key + "gt_overlaps"] >= t).sum() for t in r["thresholds"]]


@pytest.mark.parametrize("pre,ncols", CASES, ids=("aabb", "obb"))
def test_ap_against_the_recording(pre, ncols, golden):
    g = golden("g26_det_eval.npz")
    scenes = E.make_scenes(E.SEED[ncols], ncols)[:E.RECORDED]
    ious = E.iou_matrices(scenes)
    num_gt = sum(G for _, G in E.SCENES[:E.RECORDED])
    for t in E.AP_THRESHOLDS:
        for k in E.TOP_KS:
            key = f"{pre}p{int(t * 100)}_k{k or 0}_"
            r = E.ap(scenes, t, k, ious)
            assert r["num_gt"] == num_gt
            assert np.array_equal(r["num_det"], g[key + "num_det"]) and len(r["tp"]) == sum(min(P, k or P) for P, _ in E.SCENES[:E.RECORDED])
            tp_cum = np.rint(g[key + "recalls"].astype(np.float64) * num_gt).astype(np.int64)
            assert np.abs(tp_cum / num_gt - g[key + "recalls"]).max() < 1e-6
            assert np.array_equal(r["tp_cum"], tp_cum), key                     # every per-detection flag
            assert r["tp"].sum() > 0 and r["claimed_fp"] >= 1
            print(key, "precisions", np.abs(r["precisions"] - g[key + "precisions"]).max(), "ap", r["ap"], float(g[key + "ap"]), "bound", E.ap_bound(r["n_terms"]))
            assert_close(_t(r["recalls"]), _t(g[key + "recalls"]), 1e-3, key + "recalls")
            assert_close(_t(r["precisions"]), _t(g[key + "precisions"]), 1e-3, key + "precisions")
            assert r["n_terms"] == int(r["tp"].sum()) + 1                       # one step per true positive and the closing step to recall 1
            assert abs(r["ap"] - float(g[key + "ap"])) <= E.ap_bound(r["n_terms"]), key


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=0, atol=1e-15)


@pytest.mark.parametrize("name", sorted(E.hand_cases()))
def test_hand_cases(name):
    scenes, want = E.hand_cases()[name]
    r = E.recall(scenes, np.array([0.25, 0.5], dtype=np.float32), None)
    assert r["num_pos"] == want["num_pos"]
    assert _same(r["gt_overlaps"], want["gt_overlaps"]) and _same(r["recalls"], want["recalls"]), (r["gt_overlaps"], r["recalls"])
    for t in (0.25, 0.5):
        a = E.ap(scenes, t, None)
        assert a["tp"].tolist() == want["tp"][t], (t, a["tp"])
        assert _same([a["ap"]], [want["ap"][t]]), (t, a["ap"])


def test_greedy_is_not_the_column_maximum_and_ties_follow_first_occurrence():
    # proposal 0 is the best of both boxes; the greedy matching gives it to box 0 (the larger IoU) and box 1 falls back to proposal 1
    o, _ = E.greedy_match(np.array([[0.9, 0.8], [0.1, 0.3]]))
    assert o.tolist() == [0.9, 0.3]
    # equal maxima: the lowest gt first, then the lowest proposal -> (row 0, gt 0), then only (row 1, gt 1) remains
    o, _ = E.greedy_match(np.array([[0.5, 0.5], [0.5, 0.2]]))
    assert o.tolist() == [0.5, 0.2]
    # P < G leaves zeros
    o, _ = E.greedy_match(np.array([[0.2, 0.7, 0.1]]))
    assert o.tolist() == [0.7, 0.0, 0.0]
    assert math.isnan(E.recall([], None, None)["ar"]) and E.ap([], 0.5, None)["ap"] == 0.0
