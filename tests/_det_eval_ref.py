"""Float64 restatement of the reference's detection metrics, evaluate_box_proposals_recall (nerf_rpn/eval.py:14-81) and evaluate_box_proposals_ap
(eval.py:319-395), written from the semantics stated in nerf-mae_amd/csrc/det_eval.hip (numpy on the CPU, the IoU from tests/_obb_iou_ref.pairwise): the
yardstick of tests/test_det_eval_gpu.py.  tests/test_det_eval_ref_cpu.py checks it against known answers and against results recorded from the reference
(tests/golden/g26_det_eval.npz).  Also here: the seeded scene generator of the recorded fixture, the dense packing, and the decision margins.

Tie rules (torch's first occurrence on the CPU): the greedy recall matching takes the largest remaining IoU, then the lowest ground-truth index, then the lowest
proposal index; a detection's arg-max ground-truth box is the lowest index; every sort is stable, so equal scores go to the lower (scene, rank).  A scene with
detections and no ground truth makes the reference raise; here its detections are false positives.  AP is restated as the reference's sequential walk over
gt_used, NOT by the closed form the kernels use."""
import math

import numpy as np
import torch

from tests._obb_iou_ref import pairwise
from tests._rpn_post_ref import MARGIN  # noqa: F401  (the project's decision margin, re-exported)

SCENES = ((65, 3), (300, 70), (2, 5), (0, 2), (4, 0))      # (proposals, ground-truth boxes); the last one is left out of the recording (the reference raises)
RECORDED = 4
LIMITS = (100, 300)
TOP_KS = (100, None)
AP_THRESHOLDS = (0.25, 0.5, 0.75)
SEED = {6: 0, 7: 0}                                         # tools/gen_golden_det_eval.py --search


def recall_thresholds(lo):
    """the two threshold sets of the run scripts: lo = 0.5 is eval.py:68's default, lo = 0.25 is arange(0.25, 1.0, 0.05); fp32 as the reference compares"""
    return (torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32) if lo == 0.5 else torch.arange(0.25, 1.0, 0.05, dtype=torch.float32)).numpy()


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------------------------
def _to_cols(c, s, th, ncols):
    return np.concatenate([c - 0.5 * s, c + 0.5 * s], 1) if ncols == 6 else np.concatenate([c, s, th], 1)


def make_scenes(seed, ncols, shapes=SCENES):
    """-> [(boxes fp32 [P, ncols], scores fp32 [P], gt fp32 [G, ncols])] in a 20^3 room.  About a third of the ground truth sits half a box away from an earlier
    box (so one proposal can be the best of two), 70 % of the proposals are copies of the ground truth, box i % G at a noise that grows with i, the rest are
    random; the scores are a global ranking of (noise + a random term), all distinct"""
    rng = np.random.default_rng(1000 * ncols + seed)
    out, quality = [], []
    for P, G in shapes:
        c = rng.uniform(3, 17, (G, 3))
        s = rng.uniform(1.0, 3.0, (G, 3))
        th = rng.uniform(-0.5 * math.pi, 0.5 * math.pi, (G, 1))
        for g in range(1, G):
            if rng.uniform() < 0.35:
                k = rng.integers(0, g)
                c[g] = c[k] + rng.choice([-0.5, 0.5], 3) * s[k] * rng.uniform(0.5, 1.0, 3)
        pc, ps, pt = rng.uniform(3, 17, (P, 3)), rng.uniform(1.0, 3.0, (P, 3)), rng.uniform(-0.5 * math.pi, 0.5 * math.pi, (P, 1))
        noise = np.ones(P)
        for i in range(int(0.7 * P) if G else 0):
            g, sg = i % G, 0.01 + 0.5 * i / P
            noise[i] = sg
            pc[i] = c[g] + sg * s[g] * rng.normal(0, 1, 3)
            ps[i] = s[g] * np.exp(0.4 * sg * rng.normal(0, 1, 3))
            pt[i] = th[g] + 0.5 * sg * rng.normal(0, 1, 1)
        quality.append(-noise + 0.25 * rng.normal(0, 1, P))
        out.append([_to_cols(pc, ps, pt, ncols).astype(np.float32), None, _to_cols(c, s, th, ncols).astype(np.float32)])
    rank = np.argsort(np.argsort(np.concatenate(quality)))
    total, at = len(rank), 0
    for sc in out:
        P = len(sc[0])
        sc[1] = ((rank[at:at + P] + 1) / (total + 1)).astype(np.float32)
        at += P
    return [tuple(sc) for sc in out]


def input_sums(scenes):
    """float64 sums of the generated inputs (boxes, scores, gt), stored with the recording"""
    return np.array([sum(float(np.asarray(sc[k], dtype=np.float64).sum()) for sc in scenes) for k in range(3)], dtype=np.float64)


def sort_scene(boxes, scores):
    """stable descending sort of one scene"""
    order = np.argsort(-np.asarray(scores, dtype=np.float64), kind="stable")
    return boxes[order], scores[order]


def pack_dense(scenes, level_column=False, cap=None, gmax=None):
    """-> torch CPU tensors (boxes [N, cap, C (+1)], scores [N, cap], counts [N] int32, gt [N, Gmax, C], gt_counts [N] int32) of the dense form: rows in stable
    descending score.  The padding is NOT neutral: padded detection rows and padded ground-truth rows repeat the scene's first real box of either kind, so
    code that ignores the counts sees boxes that match"""
    N, C = len(scenes), scenes[0][0].shape[1]
    cap = max(len(s[0]) for s in scenes) if cap is None else cap
    gmax = max(len(s[2]) for s in scenes) if gmax is None else gmax
    boxes, scores = np.zeros((N, cap, C + int(level_column)), np.float32), np.full((N, cap), -1.0, np.float32)
    gt = np.zeros((N, gmax, C), np.float32)
    for n, (b, s, g) in enumerate(scenes):
        b, s = sort_scene(b, s)
        fill = g[0] if len(g) else (b[0] if len(b) else np.ones(C, np.float32))
        boxes[n, :, int(level_column):] = fill
        gt[n] = fill
        boxes[n, :len(b), int(level_column):] = b
        scores[n, :len(b)] = s
        gt[n, :len(g)] = g
        if level_column:
            boxes[n, :, 0] = np.arange(cap) % 3
    counts = np.array([len(s[0]) for s in scenes], np.int32)
    gt_counts = np.array([len(s[2]) for s in scenes], np.int32)
    return tuple(torch.from_numpy(a) for a in (boxes, scores, counts, gt, gt_counts))


def iou_matrices(scenes):
    """float64 IoU [P, G] per scene, rows in the scene's stable descending score order"""
    out = []
    for b, s, g in scenes:
        b, _ = sort_scene(b, s)
        if len(b) == 0 or len(g) == 0:
            out.append(np.zeros((len(b), len(g))))
        else:
            out.append(pairwise(torch.from_numpy(b).double(), torch.from_numpy(g).double()).numpy())
    return out


# ---- recall ----------------------------------------------------------------------------------------------------------------------------------------------
def greedy_match(iou):
    """eval.py:37-56 on one [P, G] matrix -> (overlaps [G] in the order taken, smallest gap between the value taken and the next remaining positive value)"""
    iou = np.array(iou, dtype=np.float64)
    P, G = iou.shape
    out, gap = np.zeros(G), math.inf
    for j in range(min(P, G)):
        colarg = iou.argmax(axis=0)                      # first occurrence: the lowest row
        colmax = iou[colarg, np.arange(G)]
        g = int(colmax.argmax())                         # the lowest gt
        r = int(colarg[g])
        out[j] = iou[r, g]
        if iou.size > 1:
            top2 = np.partition(iou.ravel(), -2)[-2:]        # retired entries are -1, live ones >= 0
            if top2[0] > 0:
                gap = min(gap, float(top2[1] - top2[0]))
        iou[r, :] = -1
        iou[:, g] = -1
    return out, gap


def recall(scenes, thresholds=None, limit=None, ious=None):
    """evaluate_box_proposals_recall -> its dict (float64 arrays) plus per_scene (each counted scene's overlaps in the order taken, None for a skipped scene),
    greedy_gap and column_max_differs (a scene where the sorted greedy overlaps are not the per-column maxima)"""
    ious = iou_matrices(scenes) if ious is None else ious
    thresholds = recall_thresholds(0.5) if thresholds is None else np.asarray(thresholds)
    per_scene, num_pos, gap, differs = [], 0, math.inf, False
    for (b, s, g), iou in zip(scenes, ious):
        if len(b) == 0 or len(g) == 0:
            per_scene.append(None)
            continue
        num_pos += len(g)
        iou = iou[:limit] if limit is not None else iou
        o, gp = greedy_match(iou)
        gap = min(gap, gp)
        differs = differs or not np.array_equal(np.sort(o), np.sort(iou.max(axis=0)))
        per_scene.append(o)
    kept = [o for o in per_scene if o is not None]
    gt_overlaps = np.sort(np.concatenate(kept)) if kept else np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        recalls = np.array([np.float64((gt_overlaps >= np.float64(t)).sum()) / np.float64(num_pos) for t in thresholds])
    return dict(ar=recalls.mean() if len(recalls) else np.float64("nan"), recalls=recalls, thresholds=thresholds, gt_overlaps=gt_overlaps, num_pos=num_pos, per_scene=per_scene,
                greedy_gap=gap, column_max_differs=differs)


# ---- AP --------------------------------------------------------------------------------------------------------------------------------------------------
def voc_area(recalls, precisions):
    """eval.py:373-387 -> (ap, number of recall steps)"""
    mrec = np.concatenate([[0.0], recalls, [1.0]])
    mpre = np.concatenate([[0.0], precisions, [0.0]])
    for i in range(len(mpre) - 1, 0, -1):
        mpre[i - 1] = max(mpre[i - 1], mpre[i]) if not (math.isnan(mpre[i - 1]) or math.isnan(mpre[i])) else math.nan
    i = np.where(mrec[1:] != mrec[:-1])[0]
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1])), len(i)


def ap(scenes, iou_thresh=0.25, top_k=None, ious=None):
    """evaluate_box_proposals_ap by its sequential walk -> its dict (float64) plus, in the global order: scene, rank (row of the scene's sorted detections), tp
    (bool), best_iou, best_gt; n_terms (recall steps of the area) and claimed_fp (detections above the threshold whose box was already taken)"""
    ious = iou_matrices(scenes) if ious is None else ious
    scene, rank, score = [], [], []
    num_gt = 0
    for n, (b, s, g) in enumerate(scenes):
        _, ss = sort_scene(b, s)
        k = len(ss) if top_k is None else min(len(ss), top_k)
        scene += [n] * k
        rank += list(range(k))
        score += list(ss[:k])
        num_gt += len(g)
    order = np.argsort(-np.asarray(score, dtype=np.float64), kind="stable")
    scene, rank = np.asarray(scene, dtype=np.int64)[order], np.asarray(rank, dtype=np.int64)[order]
    used = [np.zeros(len(sc[2]), bool) for sc in scenes]
    M = len(order)
    tp, best_iou, best_gt, claimed_fp = np.zeros(M, bool), np.zeros(M), np.full(M, -1, np.int64), 0
    for i in range(M):
        row = ious[scene[i]][rank[i]]
        if len(row) == 0:
            continue
        a = int(row.argmax())
        best_iou[i], best_gt[i] = row[a], a
        if row[a] > iou_thresh:
            if not used[scene[i]][a]:
                tp[i] = True
                used[scene[i]][a] = True
            else:
                claimed_fp += 1
    tpc = np.cumsum(tp).astype(np.float64)
    fpc = np.cumsum(~tp).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        recalls = tpc / np.float64(num_gt)
        precisions = tpc / (tpc + fpc)
    area, n_terms = voc_area(recalls, precisions) if M else (0.0, 0)
    return dict(ap=area, precisions=precisions, recalls=recalls, thresholds=iou_thresh, num_det=tpc + fpc, scene=scene, rank=rank, tp=tp, tp_cum=np.cumsum(tp), fp_cum=np.cumsum(~tp),
                best_iou=best_iou, best_gt=best_gt, n_terms=n_terms, claimed_fp=claimed_fp, num_gt=num_gt)


def ap_bound(n_terms):
    """the reference sums n_terms fp32 products of factors in [0, 1]: each term and each partial sum is within 2^-24 of exact, so the sum is within n_terms 2^-23"""
    return max(n_terms, 1) * 2.0 ** -23


# ---- conditions ------------------------------------------------------------------------------------------------------------------------------------------
def _gap_to(values, thresholds):
    values, thresholds = np.asarray(values, dtype=np.float64).ravel(), np.asarray(thresholds, dtype=np.float64).ravel()
    return float(np.abs(values[:, None] - thresholds[None, :]).min()) if len(values) and len(thresholds) else math.inf


def decision_margins(scenes, limits=LIMITS, top_ks=TOP_KS, ap_thresholds=AP_THRESHOLDS, argmax_of_claimants_only=False):
    """-> dict: recall_thr (every recorded overlap against every recall threshold of both sets), ap_thr (every detection's best IoU against every AP
    threshold), greedy_gap (condition 2), argmax_gap (a detection's best IoU against its second best, where that is positive), score_gap (distinct scores),
    and the facts column_max_differs (condition 4) and claimed_fp (condition 5: the fewest over thresholds and top_k).  argmax_of_claimants_only: argmax_gap
    over the detections whose best IoU exceeds the lowest AP threshold only; the others are false positives whichever box is their arg-max, so for the metrics
    (not for a comparison of the arg-max indices themselves) their choice takes part in no decision"""
    ious = iou_matrices(scenes)
    thr = np.concatenate([recall_thresholds(0.5), recall_thresholds(0.25)]).astype(np.float64)
    m = dict(recall_thr=math.inf, ap_thr=math.inf, greedy_gap=math.inf, argmax_gap=math.inf, column_max_differs=False, claimed_fp=1 << 30)
    for limit in limits:
        r = recall(scenes, None, limit, ious)
        m["recall_thr"] = min(m["recall_thr"], _gap_to(r["gt_overlaps"], thr))
        m["greedy_gap"] = min(m["greedy_gap"], r["greedy_gap"])
        m["column_max_differs"] = m["column_max_differs"] or r["column_max_differs"]
    for iou in ious:
        if iou.shape[0] and iou.shape[1]:
            m["ap_thr"] = min(m["ap_thr"], _gap_to(iou.max(axis=1), ap_thresholds))
            if iou.shape[1] > 1:
                top2 = np.sort(iou, axis=1)[:, -2:]
                pos = (top2[:, 0] > 0) & ((top2[:, 1] > min(ap_thresholds)) | (not argmax_of_claimants_only))
                if pos.any():
                    m["argmax_gap"] = min(m["argmax_gap"], float((top2[pos, 1] - top2[pos, 0]).min()))
    for t in ap_thresholds:
        for k in top_ks:
            m["claimed_fp"] = min(m["claimed_fp"], ap(scenes, t, k, ious)["claimed_fp"])
    scores = np.sort(np.concatenate([np.asarray(s[1], dtype=np.float64) for s in scenes]))
    m["score_gap"] = float(np.diff(scores).min()) if len(scores) > 1 else math.inf
    return m


def conditions_hold(m):
    return (m["recall_thr"] >= MARGIN and m["ap_thr"] >= MARGIN and m["greedy_gap"] >= MARGIN and m["argmax_gap"] >= MARGIN and m["score_gap"] > 0 and m["column_max_differs"]
            and m["claimed_fp"] >= 1)


# ---- hand cases with known answers (axis-aligned; the ground-truth box [0,0,0,2,2,2] and its lower half have IoU exactly 0.5) ---------------------------------
def _f(rows, cols=6):
    return np.asarray(rows, dtype=np.float32).reshape(-1, cols)


def hand_cases():
    """-> {name: (scenes, expect)}; expect: num_pos, gt_overlaps and recalls at the thresholds [0.25, 0.5] without a limit, and per AP threshold 0.25 / 0.5 the
    true-positive flags in the global order and ap (NaN where the reference divides 0 by 0)"""
    nan = math.nan
    whole, half = [0, 0, 0, 2, 2, 2], [0, 0, 0, 2, 2, 1]
    row = [[3 * g, 0, 0, 3 * g + 2, 2, 2] for g in range(70)]
    return {
        # IoU exactly 0.5: recalled at 0.5 (>=), a false positive at AP 0.5 (strictly greater)
        "one_one": ([(_f([half]), _f([0.9], 1)[:, 0], _f([whole]))], dict(num_pos=1, gt_overlaps=[0.5], recalls=[1.0, 1.0], tp={0.25: [True], 0.5: [False]}, ap={0.25: 1.0, 0.5: 0.0})),
        # equal boxes and equal scores: the lower rank claims the box, the other is a false positive
        "two_identical": ([(_f([half, half]), _f([0.9, 0.9], 1)[:, 0], _f([whole]))],
                          dict(num_pos=1, gt_overlaps=[0.5], recalls=[1.0, 1.0], tp={0.25: [True, False], 0.5: [False, False]}, ap={0.25: 1.0, 0.5: 0.0})),
        "p1_g70": ([(_f([row[37]]), _f([0.5], 1)[:, 0], _f(row))], dict(num_pos=70, gt_overlaps=[0.0] * 69 + [1.0], recalls=[1 / 70, 1 / 70], tp={0.25: [True], 0.5: [True]},
                                                                    ap={0.25: 1 / 70, 0.5: 1 / 70})),
        "p0_everywhere": ([(_f([]), _f([], 1)[:, 0], _f([whole, half])), (_f([]), _f([], 1)[:, 0], _f([whole]))],
                          dict(num_pos=0, gt_overlaps=[], recalls=[nan, nan], tp={0.25: [], 0.5: []}, ap={0.25: 0.0, 0.5: 0.0})),
        # global order: B0 (no gt: fp), A0 (tp), B1, B2 (fp)
        "dets_no_gt": ([(_f([whole]), _f([0.8], 1)[:, 0], _f([whole])), (_f([whole, half, row[5]]), _f([0.95, 0.7, 0.6], 1)[:, 0], _f([]))],
                       dict(num_pos=1, gt_overlaps=[1.0], recalls=[1.0, 1.0], tp={0.25: [False, True, False, False], 0.5: [False, True, False, False]}, ap={0.25: 0.5, 0.5: 0.5})),
        "num_gt0": ([(_f([whole, half]), _f([0.9, 0.8], 1)[:, 0], _f([]))], dict(num_pos=0, gt_overlaps=[], recalls=[nan, nan], tp={0.25: [False, False], 0.5: [False, False]},
                                                                                ap={0.25: nan, 0.5: nan})),
    }
