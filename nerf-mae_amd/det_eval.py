"""The reference's detection metrics (nerf_rpn/eval.py: evaluate_box_proposals_recall, lines 14-81, and evaluate_box_proposals_ap, lines 319-395) on the HIP kernels
of csrc/det_eval.hip: recall at IoU thresholds under proposal limits, average recall, and VOC-style AP, as every run script of the reference reports them
(run_fcos*.py:848-932, run_rpn.py:538-565, run_rpn_detect.py:522).

  det_eval_dense      the per-batch half on the dense results of FCOSOverNeRF.detections_dense() / NeRFRegionProposalNetwork.proposals_dense(): the IoU matrix of
                      each scene is formed once and serves every limit and every AP threshold; fixed-size device tensors, no host wait, capturable;
  DetectionEvaluator  accumulates batches (dense or the reference's lists) and computes the run scripts' metric dicts with one synchronisation;
  evaluate_box_proposals_recall / evaluate_box_proposals_ap   the reference's signatures and dict keys over the same kernels.

Semantics (the header of csrc/det_eval.hip has the full statement).  fp32 boxes, 6 columns (x0,y0,z0,x1,y1,z1) or 7 (x,y,z,w,l,h,theta).  Recall: per scene the
proposals in descending score, cut to `limit`; a scene without proposals or without ground truth is skipped and its ground truth is NOT counted in num_pos
(eval.py:28); min(P, G) greedy steps on the largest remaining IoU, ties to the lowest ground-truth index, then the lowest proposal (torch's first occurrence on
the CPU); recalls[i] = #(gt_overlaps >= thresholds[i]) / num_pos with fp32 thresholds, NaN when num_pos == 0.  AP: each scene keeps its top_k scores; in the
global descending order a detection is a true positive iff its largest IoU with its scene's ground truth (arg-max: the lowest index, taken regardless of the
threshold) is strictly greater than iou_thresh and no earlier detection that passed the threshold has the same arg-max; recalls = cumsum(tp) / num_gt over every
scene's boxes, precisions = tp / (tp + fp), ap = the VOC area under the precision envelope, summed in fp64; no detections: ap = 0; num_gt == 0: NaN.

Two deviations from the reference, both on input where it is undefined or fails:
  - its argsort is unstable; every sort here is stable, so equal scores go to the lower (scene, rank);
  - it raises IndexError for a scene with detections and no ground truth (max() over an empty dimension, eval.py:358); here those detections are false positives.
Limits: at most NMS_MAX_BOXES detections and MAX_GT_BOXES ground-truth boxes per scene, MAX_LIMITS limits and MAX_THRESHOLDS AP thresholds per call; more raise
ValueError."""
from __future__ import annotations

import torch

from . import ops

NMS_MAX_BOXES = ops.OBB_NMS_MAX
MAX_GT_BOXES = ops.DET_EVAL_MAX_GT
MAX_LIMITS = ops.DET_EVAL_MAX_LIMITS
MAX_THRESHOLDS = ops.DET_EVAL_MAX_THRESH

__all__ = ["det_eval_dense", "DetectionEvaluator", "evaluate_box_proposals_recall", "evaluate_box_proposals_ap", "NMS_MAX_BOXES", "MAX_GT_BOXES", "MAX_LIMITS", "MAX_THRESHOLDS"]


def _check_sizes(cap, gmax, limits, ap_thresholds):
    if cap > NMS_MAX_BOXES:
        raise ValueError(f"detection evaluation supports at most {NMS_MAX_BOXES} detections per scene, got cap = {cap}")
    if gmax > MAX_GT_BOXES:
        raise ValueError(f"detection evaluation supports at most {MAX_GT_BOXES} ground-truth boxes per scene, got {gmax}")
    if not 1 <= len(limits) <= MAX_LIMITS:
        raise ValueError(f"detection evaluation takes 1 to {MAX_LIMITS} limits per call, got {len(limits)}")
    if not 1 <= len(ap_thresholds) <= MAX_THRESHOLDS:
        raise ValueError(f"detection evaluation takes 1 to {MAX_THRESHOLDS} AP thresholds per call, got {len(ap_thresholds)}")


def det_eval_dense(boxes, scores, counts, gt_boxes, gt_counts, limits, ap_thresholds=(0.25, 0.5, 0.75), top_k=None, level_column=False):
    """boxes [N, cap, 6|7] (level_column: [N, cap, 1 + 6|7] with the level in column 0, FCOS's rows, read in place) with each scene's first counts[n] rows in
    descending score, scores [N, cap], counts [N]; gt_boxes [N, Gmax, 6|7] padded, gt_counts [N]; limits: proposal limits (None: no cut); top_k: detections kept
    per scene for AP (None: all) -> dict of fixed-size device tensors:
      gt_overlaps [N, L, Gmax]  the greedy matching's recorded IoUs in the order taken; 0 up to gt_counts[n], -1 behind it and in every slot of a skipped scene
      counted [N, L] int32      the scene's contribution to num_pos: gt_counts[n], or 0 for a skipped scene
      best_iou, best_gt [N, cap]   each detection's largest IoU and its ground-truth box (int32; -1 and IoU 0 without ground truth or past counts[n])
      tp_mask [N, cap] uint8    bit q: true positive at ap_thresholds[q];   kept [N, cap] bool: row < min(counts[n], top_k)
    Never waits for the host; capturable with torch.cuda.graph on one stream.  `scores` only fixes the contract (rows are already ordered by it) and is not read."""
    if gt_boxes.dim() != 3 or gt_boxes.shape[2] not in (6, 7):
        raise ValueError(f"det_eval_dense: gt_boxes [N, Gmax, 6|7], got {tuple(gt_boxes.shape)}")
    ncols, off = gt_boxes.shape[2], int(bool(level_column))
    if boxes.dim() != 3 or boxes.shape[2] != ncols + off or boxes.shape[0] != gt_boxes.shape[0] or tuple(scores.shape) != tuple(boxes.shape[:2]):
        raise ValueError(f"det_eval_dense: boxes [N, cap, {ncols + off}] (level_column={bool(level_column)}) and scores [N, cap] for {ncols}-column ground truth, got "
                         f"{tuple(boxes.shape)} and {tuple(scores.shape)}")
    limits, ap_thresholds = list(limits), [float(t) for t in ap_thresholds]
    _check_sizes(boxes.shape[1], gt_boxes.shape[1], limits, ap_thresholds)
    dev = boxes.device
    out = ops.det_eval_match(boxes.detach().float().contiguous(), counts.to(device=dev, dtype=torch.int32).contiguous(), gt_boxes.detach().to(dev).float().contiguous(),
                             gt_counts.to(device=dev, dtype=torch.int32).contiguous(), [-1 if v is None else int(v) for v in limits], ap_thresholds, 0 if top_k is None else int(top_k),
                             col_offset=off)
    gt_overlaps, counted, best_iou, best_gt, tp_mask, kept = out
    return dict(gt_overlaps=gt_overlaps, counted=counted, best_iou=best_iou, best_gt=best_gt, tp_mask=tp_mask, kept=kept.view(torch.bool))


def _pack_lists(proposals_list, scores_list, gt_boxes_list, device):
    """the reference's lists (any device) -> the dense form on `device`, each scene by a stable descending sort of its scores; no device-to-host read"""
    N = len(proposals_list)
    if len(scores_list) != N or len(gt_boxes_list) != N:
        raise ValueError("detection evaluation: one proposal tensor, one score tensor and one ground-truth tensor per scene")
    cols = {int(t.shape[1]) for t in list(proposals_list) + list(gt_boxes_list) if t.dim() == 2}
    if any(t.dim() != 2 for t in list(proposals_list) + list(gt_boxes_list)) or len(cols) > 1 or (cols and next(iter(cols)) not in (6, 7)):
        raise ValueError("detection evaluation: proposals [P, 6|7] and ground truth [G, 6|7] with the same column count")
    C = next(iter(cols)) if cols else 6
    cap = max([int(p.shape[0]) for p in proposals_list], default=0)
    gmax = max([int(g.shape[0]) for g in gt_boxes_list], default=0)
    boxes = torch.zeros((N, cap, C), dtype=torch.float32, device=device)
    scores = torch.full((N, cap), float("-inf"), dtype=torch.float32, device=device)
    gt = torch.zeros((N, gmax, C), dtype=torch.float32, device=device)
    counts, gt_counts = torch.zeros((N,), dtype=torch.int32, device=device), torch.zeros((N,), dtype=torch.int32, device=device)     # filled by scalar: no copy from the host
    for n, (p, s, g) in enumerate(zip(proposals_list, scores_list, gt_boxes_list)):
        P, G = int(p.shape[0]), int(g.shape[0])
        if int(s.numel()) != P:
            raise ValueError(f"detection evaluation: scene {n} has {P} proposals and {int(s.numel())} scores")
        if P:
            srt = torch.sort(s.detach().reshape(-1).to(device=device, dtype=torch.float32), descending=True, stable=True)
            boxes[n, :P] = p.detach().to(device=device, dtype=torch.float32)[srt.indices]
            scores[n, :P] = srt.values
        if G:
            gt[n, :G] = g.detach().to(device=device, dtype=torch.float32)
        counts[n].fill_(P)
        gt_counts[n].fill_(G)
    return boxes, scores, counts, gt, gt_counts


def _default_device(*lists):
    for ts in lists:
        for t in ts:
            if t.is_cuda:
                return t.device
    return torch.device("cuda", torch.cuda.current_device())


class DetectionEvaluator:
    """Accumulates det_eval_dense results over batches and computes the metric dicts of the reference's run scripts.

    update(boxes, scores, counts, gt_boxes, gt_counts, level_column=False)   the dense form of det_eval_dense, or
    update(proposals_list, scores_list, gt_boxes_list)                       the reference's lists, on any device
        stores the batch's device results; no host synchronisation.
    compute() -> {"recall_50_top_{limit}", "recall_25_top_{limit}", "recall_ar_top_{limit}" for every limit, "ap_{100 t}" for every AP threshold}: the dicts of
        evaluate_box_proposals_recall (thresholds [0.5], [0.25] and recall_thresholds, default arange(0.25, 1.0, 0.05)) and evaluate_box_proposals_ap, device tensors
        and Python ints.  One synchronisation (the counts that size the results).  "ap_75" holds AP at 0.75: the reference's run_fcos.py:932 stores its ap25 under
        that key, a slip that is not copied.
    reset() clears the state."""

    def __init__(self, limits=(300, 1000, 2500), ap_thresholds=(0.25, 0.5, 0.75), recall_thresholds=None, top_k=None):
        self.limits, self.ap_thresholds, self.top_k = list(limits), [float(t) for t in ap_thresholds], top_k
        _check_sizes(0, 0, self.limits, self.ap_thresholds)
        self.recall_thresholds = torch.arange(0.25, 1.0, 0.05, dtype=torch.float32) if recall_thresholds is None else torch.as_tensor(recall_thresholds, dtype=torch.float32).reshape(-1).cpu()
        self.reset()

    def reset(self):
        self._batches = []

    def update(self, *args, level_column=False):
        if len(args) == 3 and isinstance(args[0], (list, tuple)):
            boxes, scores, counts, gt, gt_counts = _pack_lists(*args, _default_device(*args))
            level_column = False
        elif len(args) == 5:
            boxes, scores, counts, gt, gt_counts = args
        else:
            raise TypeError("DetectionEvaluator.update(boxes, scores, counts, gt_boxes, gt_counts, level_column=False) or update(proposals_list, scores_list, gt_boxes_list)")
        r = det_eval_dense(boxes, scores, counts, gt, gt_counts, self.limits, self.ap_thresholds, self.top_k, level_column)
        gmax = gt.shape[1]
        self._batches.append(dict(gt_overlaps=r["gt_overlaps"], counted=r["counted"], tp_mask=r["tp_mask"], kept=r["kept"], scores=scores.detach().to(boxes.device).float(),
                                  num_gt=gt_counts.to(boxes.device).clamp(0, gmax).sum()))

    def compute(self):
        L, T = len(self.limits), len(self.ap_thresholds)
        dev = self._batches[0]["scores"].device if self._batches else torch.device("cuda", torch.cuda.current_device())
        def cat(key, shape, dtype):
            return torch.cat([b[key].reshape(shape) for b in self._batches]) if self._batches else torch.zeros([max(v, 0) for v in shape], dtype=dtype, device=dev)

        # recall: the recorded overlaps of every counted scene, ascending; the -1 slots sort to the front and never pass a threshold
        thr = torch.cat([torch.tensor([0.5, 0.25], dtype=torch.float32), self.recall_thresholds]).to(dev)
        overlaps = torch.stack([torch.sort(torch.cat([b["gt_overlaps"][:, l].reshape(-1) for b in self._batches])).values for l in range(L)]) if self._batches else \
            torch.zeros((L, 0), dtype=torch.float32, device=dev)
        num_pos = cat("counted", (-1, L), torch.int32).sum(0)                                                     # [L]
        recalls = (overlaps[:, None, :] >= thr[None, :, None]).sum(2).float() / num_pos[:, None].float()          # [L, thresholds]
        ar = recalls[:, 2:].mean(1)
        # AP: the global stable descending order with the kept detections first
        scores, kept, bits = cat("scores", (-1,), torch.float32), cat("kept", (-1,), torch.bool), cat("tp_mask", (-1,), torch.uint8)
        by_score = torch.sort(scores, descending=True, stable=True).indices
        order = by_score[torch.sort(kept[by_score].to(torch.uint8), descending=True, stable=True).indices]
        n_det = kept.sum().to(torch.int32).reshape(1)
        num_gt = (torch.stack([b["num_gt"] for b in self._batches]).sum() if self._batches else torch.zeros((), dtype=torch.int64, device=dev)).to(torch.int32).reshape(1)
        tp_cum, fp_cum, rec, pre, ap = ops.det_eval_pr(bits[order].contiguous(), n_det, num_gt, T)
        host = torch.cat([num_pos.to(torch.int64), n_det.to(torch.int64), num_gt.to(torch.int64)]).cpu().tolist()  # the one synchronisation
        npos, nd, ng = host[:L], host[L], host[L + 1]
        out = {}
        for l, limit in enumerate(self.limits):
            ov = overlaps[l, overlaps.shape[1] - npos[l]:]
            for key, sl, t in (("50", slice(0, 1), thr[0:1]), ("25", slice(1, 2), thr[1:2]), ("ar", slice(2, None), thr[2:])):
                r = recalls[l, sl]
                out[f"recall_{key}_top_{limit}"] = dict(ar=ar[l] if key == "ar" else r.mean(), recalls=r, thresholds=t, gt_overlaps=ov, num_pos=npos[l])
        for q, t in enumerate(self.ap_thresholds):
            out[f"ap_{int(round(100 * t))}"] = dict(ap=ap[q], precisions=pre[q, :nd], recalls=rec[q, :nd], thresholds=t, num_det=(tp_cum[q, :nd] + fp_cum[q, :nd]).long(),
                                                     tp_cum=tp_cum[q, :nd], fp_cum=fp_cum[q, :nd], num_gt=ng)
        return out


def _to(d, device):
    return {k: (v.to(device) if isinstance(v, torch.Tensor) else v) for k, v in d.items()}


def _input_device(*lists):
    for ts in lists:
        for t in ts:
            return t.device
    return torch.device("cpu")


def evaluate_box_proposals_recall(proposals_list, proposal_scores_list, gt_boxes_list, thresholds=None, limit=None):
    """eval.py:14-81 with its signature -> {"ar", "recalls", "thresholds", "gt_overlaps", "num_pos"}; tensors on the inputs' device.  thresholds None:
    arange(0.5, 0.95 + 1e-5, 0.05) fp32, as the reference.  Semantics, tie rules and the two deviations: the module docstring."""
    thr = torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32) if thresholds is None else thresholds
    ev = DetectionEvaluator(limits=(limit,), ap_thresholds=(0.5,), recall_thresholds=thr)
    ev.update(list(proposals_list), list(proposal_scores_list), list(gt_boxes_list))
    r = ev.compute()[f"recall_ar_top_{limit}"]
    r["thresholds"] = thr
    return _to(r, _input_device(proposals_list, gt_boxes_list))


def evaluate_box_proposals_ap(proposals_list, proposal_scores_list, gt_boxes_list, iou_thresh=0.25, top_k=None):
    """eval.py:319-395 with its signature -> {"ap" (fp64), "precisions", "recalls", "thresholds", "num_det"}; tensors on the inputs' device.  Semantics, tie rules
    and the two deviations: the module docstring."""
    ev = DetectionEvaluator(limits=(None,), ap_thresholds=(iou_thresh,), top_k=top_k)
    ev.update(list(proposals_list), list(proposal_scores_list), list(gt_boxes_list))
    r = ev.compute()[f"ap_{int(round(100 * float(iou_thresh)))}"]
    return _to({k: r[k] for k in ("ap", "precisions", "recalls", "thresholds", "num_det")}, _input_device(proposals_list, gt_boxes_list))
