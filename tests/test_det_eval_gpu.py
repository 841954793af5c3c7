"""Detection evaluation on the GPU (nerf_mae_amd.det_eval over csrc/det_eval.hip) against the float64 restatement (tests/_det_eval_ref.py), the reference's
recording (tests/golden/g26_det_eval.npz) and hand cases.

Scenes: tests/_det_eval_ref.make_scenes, (P, G) = (65, 3), (300, 70), (2, 5), (0, 2), (4, 0), 6 and 7 columns, with limits (100, 300) and top_k 100 / None: a
64-row tile is crossed, more than 64 ground-truth boxes, a limit that cuts, P < G, a skipped scene, detections without ground truth.  The dense padding is
not neutral (tests/_det_eval_ref.pack_dense).  Two shapes the scenes do not reach are tested on their own: more than 256 ground-truth columns with more than 256
rows (the matcher's column loop, several IoU workgroups), and more than 1024 detections in the precision / recall scan (its chunk carry, both directions).

Tolerances.  gt_overlaps, best IoUs, recalls, precisions: the project's contract for fp32, assert_close(rtol=1e-3) over every entry, the -1 and 0 slots
included; nothing is masked.  Arg-max indices, counted, kept, the true-positive masks, the cumulative counts: exact; the restatement's decision margins of at
least 1e-5 (against an fp32 IoU error of about 1e-7) are asserted first.  ap: n_terms 2^-23 absolute against the float64 restatement and against the recording
(tests/_det_eval_ref.ap_bound)."""
import functools
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

pytestmark = pytest.mark.gpu
AR_SET = E.recall_thresholds(0.25)


def _m():
    from nerf_mae_amd import det_eval
    return det_eval


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64)))


@functools.lru_cache(maxsize=None)
def reference(ncols, recorded_only=False):
    """the restatement on the generated scenes, computed once and shared (never modified)"""
    scenes = E.make_scenes(E.SEED[ncols], ncols)
    m = E.decision_margins(scenes)
    assert E.conditions_hold(m), m
    scenes = scenes[:E.RECORDED] if recorded_only else scenes
    ious = E.iou_matrices(scenes)
    rec = {(limit, lo): E.recall(scenes, E.recall_thresholds(lo), limit, ious) for limit in E.LIMITS for lo in (0.5, 0.25)}
    ap = {(t, k): E.ap(scenes, t, k, ious) for t in E.AP_THRESHOLDS for k in E.TOP_KS}
    return dict(scenes=scenes, ious=ious, recall=rec, ap=ap)


def expected_dense(scenes, ious, limits, thresholds, top_k, cap, gmax):
    """the restatement laid out as det_eval_dense's tensors"""
    N, L = len(scenes), len(limits)
    gt_overlaps, counted = np.full((N, L, gmax), -1.0), np.zeros((N, L), np.int64)
    best_iou, best_gt = np.zeros((N, cap)), np.full((N, cap), -1, np.int64)
    tp_mask, kept = np.zeros((N, cap), np.int64), np.zeros((N, cap), bool)
    for l, limit in enumerate(limits):
        r = E.recall(scenes, None, limit, ious)
        for n, o in enumerate(r["per_scene"]):
            if o is not None:
                gt_overlaps[n, l, :len(o)] = o
                counted[n, l] = len(o)
    for n, iou in enumerate(ious):
        P, G = iou.shape
        kept[n, :P if top_k is None else min(P, top_k)] = True
        if P and G:
            best_iou[n, :P], best_gt[n, :P] = iou.max(axis=1), iou.argmax(axis=1)
    for q, t in enumerate(thresholds):
        a = E.ap(scenes, t, top_k, ious)
        tp_mask[a["scene"][a["tp"]], a["rank"][a["tp"]]] |= 1 << q
    return dict(gt_overlaps=gt_overlaps, counted=counted, best_iou=best_iou, best_gt=best_gt, tp_mask=tp_mask, kept=kept)


def check_dense(got, want, tag):
    assert torch.equal(got["counted"].cpu().long(), torch.from_numpy(want["counted"])), tag
    assert torch.equal(got["best_gt"].cpu().long(), torch.from_numpy(want["best_gt"])), tag
    assert torch.equal(got["kept"].cpu(), torch.from_numpy(want["kept"])), tag
    assert torch.equal(got["tp_mask"].cpu().long(), torch.from_numpy(want["tp_mask"])), tag
    if want["gt_overlaps"].size:
        assert_close(got["gt_overlaps"].cpu(), _t(want["gt_overlaps"]), 1e-3, tag + " gt_overlaps")
        assert torch.equal(got["gt_overlaps"].cpu() < 0, torch.from_numpy(want["gt_overlaps"] < 0)) and torch.equal(got["gt_overlaps"].cpu() == 0, torch.from_numpy(want["gt_overlaps"] == 0))
    if want["best_iou"].size:
        assert_close(got["best_iou"].cpu(), _t(want["best_iou"]), 1e-3, tag + " best_iou")


def check_compute(out, scenes, ious, limits, thresholds, top_k, tag, ar_set=AR_SET):
    """DetectionEvaluator.compute() against the restatement on the same scenes"""
    for limit in limits:
        for key, thr in (("50", np.array([0.5], np.float32)), ("25", np.array([0.25], np.float32)), ("ar", ar_set)):
            got, want = out[f"recall_{key}_top_{limit}"], E.recall(scenes, thr, limit, ious)
            assert got["num_pos"] == want["num_pos"], (tag, key, limit)
            assert tuple(got["gt_overlaps"].shape) == want["gt_overlaps"].shape and np.array_equal(got["thresholds"].cpu().numpy(), thr)
            if want["num_pos"]:
                assert_close(got["gt_overlaps"].cpu(), _t(want["gt_overlaps"]), 1e-3, f"{tag} gt_overlaps {key} {limit}")
                want_counts = [(want["gt_overlaps"] >= np.float64(t)).sum() for t in thr]
                assert [int(round(v * want["num_pos"])) for v in got["recalls"].cpu().tolist()] == want_counts, "the same overlaps pass each threshold"
                assert_close(got["recalls"].cpu(), _t(want["recalls"]), 1e-3, f"{tag} recalls {key} {limit}")
                assert_close(got["ar"].reshape(1).cpu(), _t([want["ar"]]), 1e-3, f"{tag} ar {key} {limit}")
            else:
                assert torch.isnan(got["recalls"]).all() and torch.isnan(got["ar"])
    for t in thresholds:
        got, want = out[f"ap_{int(round(100 * t))}"], E.ap(scenes, t, top_k, ious)
        assert got["num_gt"] == want["num_gt"] and got["thresholds"] == t
        assert torch.equal(got["tp_cum"].cpu().long(), torch.from_numpy(want["tp_cum"])) and torch.equal(got["fp_cum"].cpu().long(), torch.from_numpy(want["fp_cum"])), (tag, t)
        assert torch.equal(got["num_det"].cpu(), torch.from_numpy(want["num_det"]).long())
        print(f"{tag} ap@{t}: {got['ap'].item():.9f} restatement {want['ap']:.9f} bound {E.ap_bound(want['n_terms']):.2e}")
        if math.isnan(want["ap"]):
            assert torch.isnan(got["ap"]) and (len(want["tp"]) == 0 or torch.isnan(got["recalls"]).all())
            continue
        assert got["ap"].dtype == torch.float64 and abs(got["ap"].item() - want["ap"]) <= E.ap_bound(want["n_terms"]), (tag, t)
        if len(want["tp"]):
            assert_close(got["recalls"].cpu(), _t(want["recalls"]), 1e-3, f"{tag} recalls@{t}")
            assert_close(got["precisions"].cpu(), _t(want["precisions"]), 1e-3, f"{tag} precisions@{t}")


def cuda(ts):
    return [t.cuda() for t in ts]


@pytest.mark.parametrize("top_k", E.TOP_KS, ids=("top100", "all"))
@pytest.mark.parametrize("level_column", (False, True), ids=("plain", "level"))
@pytest.mark.parametrize("ncols", (6, 7), ids=("aabb", "obb"))
def test_dense_and_evaluator_against_the_restatement(ncols, level_column, top_k):
    M, c = _m(), reference(ncols)
    tag = f"{ncols} cols level={level_column} top_k={top_k}"
    dense = cuda(E.pack_dense(c["scenes"], level_column))
    got = M.det_eval_dense(*dense, E.LIMITS, E.AP_THRESHOLDS, top_k, level_column)
    check_dense(got, expected_dense(c["scenes"], c["ious"], E.LIMITS, E.AP_THRESHOLDS, top_k, dense[0].shape[1], dense[3].shape[1]), tag)
    ev = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=top_k)
    ev.update(*dense, level_column=level_column)
    check_compute(ev.compute(), c["scenes"], c["ious"], E.LIMITS, E.AP_THRESHOLDS, top_k, tag)


@pytest.mark.parametrize("pre,ncols", (("a_", 6), ("o_", 7)), ids=("aabb", "obb"))
def test_evaluator_against_the_reference_recording(pre, ncols, golden):
    M, g, c = _m(), golden("g26_det_eval.npz"), reference(ncols, True)
    np.testing.assert_allclose(E.input_sums(E.make_scenes(E.SEED[ncols], ncols)), g[pre + "input_sums"], rtol=1e-12)
    lists = [[torch.from_numpy(s[k]).cuda() for s in c["scenes"]] for k in range(3)]
    for k in E.TOP_KS:
        ev = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=k)
        ev.update(*lists)
        out = ev.compute()
        for limit in E.LIMITS:
            r, key = out[f"recall_ar_top_{limit}"], f"{pre}r{limit}_t25_"
            assert r["num_pos"] == int(g[key + "num_pos"])
            assert_close(r["gt_overlaps"].cpu(), _t(g[key + "gt_overlaps"]), 1e-3, key + "gt_overlaps")
            assert_close(r["recalls"].cpu(), _t(g[key + "recalls"]), 1e-3, key + "recalls")
            assert_close(r["ar"].reshape(1).cpu(), _t([g[key + "ar"]]), 1e-3, key + "ar")
            r = M.evaluate_box_proposals_recall(*lists, limit=limit)                 # the default thresholds 0.5 .. 0.95
            key = f"{pre}r{limit}_t50_"
            assert r["num_pos"] == int(g[key + "num_pos"])
            assert_close(r["recalls"].cpu(), _t(g[key + "recalls"]), 1e-3, key + "recalls")
        for t in E.AP_THRESHOLDS:
            r, key = out[f"ap_{int(t * 100)}"], f"{pre}p{int(t * 100)}_k{k or 0}_"
            n_terms = c["ap"][(t, k)]["n_terms"]
            assert torch.equal(r["num_det"].cpu(), torch.from_numpy(g[key + "num_det"]))
            assert torch.equal(r["tp_cum"].cpu().long(), torch.from_numpy(np.rint(g[key + "recalls"].astype(np.float64) * r["num_gt"]).astype(np.int64)))
            assert_close(r["precisions"].cpu(), _t(g[key + "precisions"]), 1e-3, key + "precisions")
            print(f"{key}ap {r['ap'].item():.9f} recorded {float(g[key + 'ap']):.9f} bound {E.ap_bound(n_terms):.2e}")
            assert abs(r["ap"].item() - float(g[key + "ap"])) <= E.ap_bound(n_terms), key


def _same(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)) and np.allclose(got[~np.isnan(got)], want[~np.isnan(want)], rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", sorted(E.hand_cases()))
def test_hand_cases_through_the_reference_signatures(name):
    M = _m()
    scenes, want = E.hand_cases()[name]
    lists = [[torch.from_numpy(s[k]).cuda() for s in scenes] for k in range(3)]
    r = M.evaluate_box_proposals_recall(*lists, thresholds=torch.tensor([0.25, 0.5]), limit=None)
    assert sorted(r) == ["ar", "gt_overlaps", "num_pos", "recalls", "thresholds"] and all(v.is_cuda for v in r.values() if isinstance(v, torch.Tensor) and v is not r["thresholds"])
    assert r["num_pos"] == want["num_pos"]
    assert _same(r["gt_overlaps"].cpu().numpy(), want["gt_overlaps"]) and _same(r["recalls"].cpu().numpy(), want["recalls"]), (r["gt_overlaps"], r["recalls"])
    for t in (0.25, 0.5):
        a = M.evaluate_box_proposals_ap(*lists, iou_thresh=t, top_k=None)
        assert sorted(a) == ["ap", "num_det", "precisions", "recalls", "thresholds"] and a["thresholds"] == t
        n = len(want["tp"][t])
        tp_cum = np.cumsum(np.asarray(want["tp"][t], dtype=np.int64))
        assert a["num_det"].cpu().tolist() == list(range(1, n + 1))
        assert _same(a["precisions"].cpu().numpy(), tp_cum / np.arange(1, n + 1)), (t, a["precisions"])
        assert _same([a["ap"].item()], [want["ap"][t]]), (t, a["ap"])
        num_gt = sum(len(s[2]) for s in scenes)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert _same(a["recalls"].cpu().numpy(), tp_cum / np.float64(num_gt)), (t, a["recalls"])
    # the lists on the CPU give tensors on the CPU
    r = M.evaluate_box_proposals_recall(*[[t.cpu() for t in ts] for ts in lists], limit=None)
    assert not r["recalls"].is_cuda and not r["gt_overlaps"].is_cuda and r["num_pos"] == want["num_pos"]


def _flat(out):
    return [(k, kk, v) for k, d in sorted(out.items()) for kk, v in sorted(d.items())]


def _equal_outputs(a, b):
    for (k, kk, v), (k2, kk2, w) in zip(_flat(a), _flat(b)):
        assert (k, kk) == (k2, kk2)
        if isinstance(v, torch.Tensor):
            assert v.dtype == w.dtype and v.shape == w.shape and torch.equal(v, w), (k, kk)
        else:
            assert v == w, (k, kk)
    assert len(_flat(a)) == len(_flat(b))


@pytest.mark.parametrize("ncols", (6, 7), ids=("aabb", "obb"))
def test_two_batches_equal_one_call_and_lists_equal_dense(ncols):
    M, c = _m(), reference(ncols)
    scenes = c["scenes"]
    one = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=100)
    one.update(*cuda(E.pack_dense(scenes)))
    whole = one.compute()
    two = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=100)
    two.update(*cuda(E.pack_dense(scenes[:2])))
    two.update(*cuda(E.pack_dense(scenes[2:])))
    _equal_outputs(two.compute(), whole)
    lists = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=100)
    lists.update(*[[torch.from_numpy(s[k]).cuda() for s in scenes] for k in range(3)])
    _equal_outputs(lists.compute(), whole)
    # the level column is skipped, not read
    lvl = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=100)
    lvl.update(*cuda(E.pack_dense(scenes, True)), level_column=True)
    _equal_outputs(lvl.compute(), whole)
    two.reset()
    assert two.compute()["ap_50"]["ap"].item() == 0.0 and math.isnan(two.compute()["recall_50_top_100"]["ar"].item())
    assert whole["ap_75"]["thresholds"] == 0.75 and not torch.equal(whole["ap_75"]["tp_cum"], whole["ap_25"]["tp_cum"]), "ap_75 is AP at 0.75"


def test_update_never_waits_and_dense_is_capturable_and_bit_identical():
    M, c = _m(), reference(7)
    dense = cuda(E.pack_dense(c["scenes"], True))
    lists = [[torch.from_numpy(s[k]).cuda() for s in c["scenes"]] for k in range(3)]
    args = (E.LIMITS, E.AP_THRESHOLDS, 100, True)
    eager = M.det_eval_dense(*dense, *args)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ev = M.DetectionEvaluator(E.LIMITS, E.AP_THRESHOLDS, top_k=100)
        ev.update(*dense, level_column=True)
        ev.update(*lists)
        again = M.det_eval_dense(*dense, *args)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert all(torch.equal(eager[k], again[k]) for k in eager), "two runs are bit-identical"
    static = [t.clone() for t in dense]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        M.det_eval_dense(*static, *args)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.det_eval_dense(*static, *args)
    replays = []
    for _ in range(2):
        for d in static:
            d.zero_()
        graph.replay()                                # stale inputs: every output is rewritten by the next replay
        for d, f in zip(static, dense):
            d.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
        replays.append({k: v.clone() for k, v in out.items()})
    assert all(torch.equal(replays[0][k], replays[1][k]) and torch.equal(replays[0][k], eager[k]) for k in eager)


def test_more_than_256_ground_truth_columns_and_rows():
    """the matcher's column loop (G > 256 lanes), several IoU workgroups per scene (cap > 256) and ground-truth tiles (G > 64), with a limit that cuts; random
    axis-aligned boxes in a 12^3 room: about 1600 positive IoUs, several per column"""
    M = _m()
    rng = np.random.default_rng(0)                     # the first seed whose decisions all keep the margin (asserted below)

    def boxes(n):
        c, s = rng.uniform(0, 12, (n, 3)), rng.uniform(1.0, 2.5, (n, 3))
        return np.concatenate([c - 0.5 * s, c + 0.5 * s], 1).astype(np.float32)

    scenes = [(boxes(300), rng.permutation(300).astype(np.float32), boxes(270))]
    ious = E.iou_matrices(scenes)
    limits = (None, 260)
    gaps = [E.recall(scenes, None, limit, ious)["greedy_gap"] for limit in limits]
    top2 = np.sort(ious[0], axis=1)[:, -2:]
    assert min(gaps) >= E.MARGIN and (top2[:, 1] - top2[:, 0])[top2[:, 0] > 0].min() >= E.MARGIN, (gaps, "choose another seed: a decision is closer than the margin")
    assert np.abs(top2[:, 1] - 0.3).min() >= E.MARGIN
    dense = cuda(E.pack_dense(scenes))
    got = M.det_eval_dense(*dense, limits, (0.3,), None)
    want = expected_dense(scenes, ious, limits, (0.3,), None, 300, 270)
    assert (want["gt_overlaps"][0, 1] == 0).sum() >= 20, "the limit leaves boxes unmatched"
    check_dense(got, want, "300 x 270")


def test_precision_recall_scan_over_more_than_one_chunk():
    """det_eval_pr on 2500 bytes of which the first 2300 count: three chunks of 1024 in both directions, two thresholds in one launch"""
    from nerf_mae_amd import ops
    rng = np.random.default_rng(9)
    M, n, num_gt = 2500, 2300, 900
    bits = (rng.uniform(size=M) < np.linspace(0.9, 0.05, M)).astype(np.uint8) | ((rng.uniform(size=M) < 0.2).astype(np.uint8) << 1)
    dev = lambda a, dt: torch.tensor(a, dtype=dt).cuda()   # noqa: E731
    tp_cum, fp_cum, rec, pre, ap = ops.det_eval_pr(dev(bits, torch.uint8), dev([n], torch.int32), dev([num_gt], torch.int32), 2)
    for q in range(2):
        tp = ((bits[:n] >> q) & 1).astype(bool)
        tpc, fpc = np.cumsum(tp), np.cumsum(~tp)
        assert np.array_equal(tp_cum[q, :n].cpu().numpy(), tpc) and np.array_equal(fp_cum[q, :n].cpu().numpy(), fpc)
        assert not tp_cum[q, n:].any() and not fp_cum[q, n:].any() and not rec[q, n:].any() and not pre[q, n:].any()
        area, n_terms = E.voc_area(tpc / num_gt, tpc / (tpc + fpc))
        assert_close(rec[q, :n].cpu(), _t(tpc / num_gt), 1e-3, "recalls")
        assert_close(pre[q, :n].cpu(), _t(tpc / (tpc + fpc)), 1e-3, "precisions")
        print(f"ap {ap[q].item():.12f} float64 {area:.12f}")
        assert abs(ap[q].item() - area) <= E.ap_bound(n_terms)


def test_limits_and_arguments():
    M = _m()
    from nerf_mae_amd import ops
    from nerf_mae_amd._lib import NmhError
    z = lambda *s: torch.zeros(s, device="cuda")                       # noqa: E731
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")    # noqa: E731
    assert M.NMS_MAX_BOXES == 16384 and M.MAX_GT_BOXES >= 1024
    with pytest.raises(ValueError, match="detections per scene"):
        M.det_eval_dense(z(1, M.NMS_MAX_BOXES + 1, 6), z(1, M.NMS_MAX_BOXES + 1), i(1), z(1, 2, 6), i(1), (100,))
    with pytest.raises(ValueError, match="ground-truth boxes"):
        M.det_eval_dense(z(1, 4, 6), z(1, 4), i(1), z(1, M.MAX_GT_BOXES + 1, 6), i(1), (100,))
    with pytest.raises(ValueError, match="limits"):
        M.det_eval_dense(z(1, 4, 6), z(1, 4), i(1), z(1, 2, 6), i(1), tuple(range(1, M.MAX_LIMITS + 2)))
    with pytest.raises(ValueError, match="AP thresholds"):
        M.DetectionEvaluator(ap_thresholds=[0.1 * k for k in range(M.MAX_THRESHOLDS + 1)])
    with pytest.raises(ValueError, match="level_column"):
        M.det_eval_dense(z(1, 4, 7), z(1, 4), i(1), z(1, 2, 6), i(1), (100,))                  # a 7-column row against 6-column ground truth: say which it is
    ok = M.det_eval_dense(z(1, 4, 7), z(1, 4), i(1), z(1, 2, 6), i(1), (100,), level_column=True)
    assert tuple(ok["gt_overlaps"].shape) == (1, 1, 2) and (ok["gt_overlaps"] == -1).all() and not ok["kept"].any()
    # the C ABI's own checks: a NULL pointer and sizes beyond the constants are argument errors, not faults
    with pytest.raises(NmhError, match="invalid argument"):
        ops.lib().call("nmh_det_eval_iou", 6, 1, 4, 6, 0, None, i(1), 2, z(1, 2, 6), i(1), z(1, 2, 4), z(1, 4), i(1, 4), 0)
    with pytest.raises(NmhError, match="invalid argument"):
        ops.lib().call("nmh_det_eval_iou", 6, 1, 4, 6, 1, z(1, 4, 6), i(1), 2, z(1, 2, 6), i(1), z(1, 2, 4), z(1, 4), i(1, 4), 0)     # the box would run past the row
    with pytest.raises(NmhError, match="invalid argument"):
        ops.lib().call("nmh_det_eval_pr", 8, torch.zeros(8, dtype=torch.uint8, device="cuda"), i(1), i(1), 9, i(9, 8), i(9, 8), z(9, 8), z(9, 8), torch.zeros(9, dtype=torch.float64, device="cuda"), 0)
