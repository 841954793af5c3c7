"""The reference's voxel-semantics scoring on the HIP kernels of csrc/heads.hip (sem_eval_kernel): what `output_metrics` of
`SwinTransformer_VoxelSemantics_Pretrained_Skip` returns per batch (nerf_rpn/model/feature_extractor.py:2748-2806, through intersectionAndUnionGPU,
nerf_rpn/model/metrics.py:491-518) and what the evaluation loop makes of it (nerf_rpn/run_voxel_semantics.py:805-958: three AverageMeters, then mean IoU, mean
class accuracy and overall accuracy over the labelled voxels).

  sem_eval_dense          one pass over the logits of a batch: the loss scalars of the training loss, the per-class counts and the two label volumes;
  intersection_and_union  the reference's intersectionAndUnionGPU signature on two device label tensors, the same counting code without the logits;
  SemanticEvaluator       running int64 totals on the device, one synchronisation in compute().

Semantics.  logits (B,K,*) fp32, labels (B,*) class ids as fp32, 0 = unlabelled, 2 <= K <= 32.  The predicted label p(v) is the arg-max over all K classes, class 0
included.  Over the voxels with label > 0, summed over the batch, for every class c = 1..K-1:  intersection[c] = #(p == c and label == c),  area_pred[c] = #(p == c),
target[c] = #(label == c),  union = area_pred + target - intersection.  A labelled voxel predicted as class 0 enters no area_pred bin (the reference's
histc(min=1)).  All counts are int64 from the first addition to the last; `sem_ce_loss_val` and `iou_val` are the two numbers of `forward_loss`.  Every sum has a
fixed order: two runs give the same bits.

Stated deviations from the reference:
  - p(v) is the arg-max of the RAW logits, the lowest index on an exact tie; the reference takes the arg-max of the fp32 softmax, which can differ only where two
    distinct logits round to the same probability;
  - for K = 2 the reference's histc(bins=1, min=1, max=1) has an empty range, which ATen widens to [0, 2]: its single area_pred bin then also takes the labelled
    voxels predicted as class 0; here area_pred[1] = #(p == 1) for every K;
  - the reference's histc returns fp32 counts (exact up to 2^24 per bin); these are int64;
  - a label outside [0, K) is a caller error there (its cross entropy raises); here it is a labelled voxel of no class: it counts in area_pred (and so in the
    union) if predicted, in no target or intersection bin, and weighs 0 in the loss;
  - intersection_and_union treats `target > 0` as labelled where the reference tests `target != 0`: the two differ only for negative labels, which neither defines."""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import ops

__all__ = ["sem_eval_dense", "intersection_and_union", "pad_label_grids", "SemanticEvaluator", "label_class_counts", "class_weights_from_counts",
           "calculate_class_weights"]


def pad_label_grids(x, spatial, device):
    """list of (1,W,L,H) label grids -> (B,*spatial) fp32 on `device`, zero (unlabelled) padded: the pad_tensor rule of the heads' `transform`"""
    out = torch.zeros((len(x),) + tuple(spatial), dtype=torch.float32, device=device)
    for i, t in enumerate(x):
        a0, a1, a2 = t.shape[-3:]
        out[i, :a0, :a1, :a2] = t.reshape(a0, a1, a2).to(device=device, dtype=torch.float32, non_blocking=True)
    return out


def sem_eval_dense(logits, labels, class_weights=None, totals=None):
    """logits (B,K,*spatial) fp32 on the device, labels (B,*spatial) -> (sem_ce_loss_val, metrics, pred_labels_vis, target_vis) as `output_metrics` returns them:
    metrics = {intersection, union, target, area_pred: int64 [K-1]; iou_val}, the two volumes int64 (B,*spatial).  totals: int64 [3][K-1] running totals
    {intersection, union, target}, added to on the device.  Never waits for the host; capturable on one stream."""
    if not logits.is_cuda:
        raise RuntimeError("voxel-semantics evaluation (HIP) needs the logits on a HIP device (no CPU fallback)")
    B = logits.shape[0]
    spatial = tuple(logits.shape[2:])
    cw = None if class_weights is None else class_weights.to(device=logits.device, dtype=torch.float32, non_blocking=True).contiguous()   # (host weights: no wait)
    lab = labels.to(device=logits.device, dtype=torch.float32, non_blocking=True).reshape(B, -1).contiguous()
    out, counts, pv, tv = ops.sem_eval(logits.detach().contiguous(), lab, cw, totals)
    metrics = dict(intersection=counts[0], union=counts[1], target=counts[2], area_pred=counts[3], iou_val=out[1])
    return out[0], metrics, pv.view((B,) + spatial), tv.view((B,) + spatial)


def intersection_and_union(output, target, K):
    """intersectionAndUnionGPU(output, target, K) (metrics.py:491-518) -> (area_intersection, area_union, area_target), int64 [K-1] on the device; output and target
    are device label tensors of one shape, integer or fp32."""
    if not (output.is_cuda and target.is_cuda):
        raise RuntimeError("intersection_and_union (HIP) needs device tensors (no CPU fallback)")
    if output.shape != target.shape:
        raise ValueError(f"intersection_and_union: output {tuple(output.shape)} and target {tuple(target.shape)} differ in shape")
    dt = torch.float32 if (output.is_floating_point() or target.is_floating_point()) else (torch.int32 if output.dtype == target.dtype == torch.int32 else torch.int64)
    c = ops.sem_label_counts(output.to(dt).contiguous(), target.to(dt).contiguous(), K)
    return c[0], c[1], c[2]


class SemanticEvaluator:
    """The evaluation loop's bookkeeping (run_voxel_semantics.py:805-958) with the totals kept on the device.
        ev = SemanticEvaluator(num_classes)
        for label_grids, pred in batches: ev.update(label_grids, pred)        # or ev.update_counts(head.output_metrics(label_grids, pred)[1])
        ev.compute() -> {iou_class, accuracy_class [K-1], mIoU, mAcc, allAcc}   (float64; the one synchronisation)"""

    def __init__(self, num_classes: int, class_weights: Optional[torch.Tensor] = None):
        if not 2 <= int(num_classes) <= 32:
            raise ValueError("SemanticEvaluator: 2 <= num_classes <= 32")
        self.num_classes, self.class_weights = int(num_classes), class_weights
        self.totals = None     # int64 [3][K-1] = {intersection, union, target}, made on the device of the first update

    def _totals(self, device):
        if self.totals is None:
            self.totals = torch.zeros((3, self.num_classes - 1), dtype=torch.int64, device=device)
        return self.totals

    def update(self, label_grids, pred):
        """label_grids: list of (1,W,L,H) grids (zero padded to pred's extent) or a dense (B,*spatial) tensor; pred (B,K,*spatial) logits on the device.
        Adds the batch to the running totals inside the kernel and returns what sem_eval_dense returns.  No synchronisation."""
        if pred.shape[1] != self.num_classes:
            raise ValueError(f"SemanticEvaluator({self.num_classes}): pred has {pred.shape[1]} classes")
        if not pred.is_cuda:
            raise RuntimeError("voxel-semantics evaluation (HIP) needs the logits on a HIP device (no CPU fallback)")
        labels = pad_label_grids(label_grids, pred.shape[2:], pred.device) if isinstance(label_grids, (list, tuple)) else label_grids
        return sem_eval_dense(pred, labels, self.class_weights, self._totals(pred.device))

    def update_counts(self, metrics):
        """adds a batch's {intersection, union, target} (an `output_metrics` dict) on the device"""
        t = self._totals(metrics["intersection"].device)
        for row, key in enumerate(("intersection", "union", "target")):
            t[row] += metrics[key].to(torch.int64)

    @staticmethod
    def accuracy(metrics):
        """the loop's per-batch accuracy, sum(intersection) / (sum(target) + 1e-10), as a float64 device scalar (no synchronisation)"""
        return metrics["intersection"].sum().double() / (metrics["target"].sum().double() + 1e-10)

    def compute(self):
        if self.totals is None:
            raise RuntimeError("SemanticEvaluator.compute() before any update")
        I, U, T = self.totals.cpu().numpy().astype(np.float64)
        iou_class, accuracy_class = I / (U + 1e-10), I / (T + 1e-10)
        return dict(iou_class=iou_class, accuracy_class=accuracy_class, mIoU=float(np.mean(iou_class)), mAcc=float(np.mean(accuracy_class)),
                    allAcc=float(I.sum() / (T.sum() + 1e-10)))

    def reset(self):
        if self.totals is not None:
            self.totals.zero_()


# ---- class weights of the training loss (nerf_rpn/model/metrics.py:383-426 calculate_class_weights) --------------------------------------------------------
def label_class_counts(labels, num_classes: int):
    """labels: a device tensor of class ids (any shape; fp32, int32, int64 or uint8) -> int64 [num_classes] on the device: entry c = #(label == c) for
    c = 1..num_classes-1, entry 0 = 0 (unlabelled voxels are not counted, metrics.py:400, 414); a label >= num_classes enters no bin.  The target histogram of
    nmh_sem_label_counts with output = target = labels: no atomics, fixed summation order, no host wait."""
    if not labels.is_cuda:
        raise RuntimeError("label_class_counts (HIP) needs a device tensor (no CPU fallback)")
    if labels.dtype not in (torch.float32, torch.int32, torch.int64):
        if labels.dtype != torch.uint8:
            raise ValueError(f"label_class_counts: labels must be uint8, int32, int64 or float32, got {labels.dtype}")
        labels = labels.to(torch.int32)
    lab = labels.contiguous()
    counts = torch.zeros(int(num_classes), dtype=torch.int64, device=labels.device)
    counts[1:] = ops.sem_label_counts(lab, lab, num_classes)[2]
    return counts


def class_weights_from_counts(counts, c: float = 1.02) -> np.ndarray:
    """w = 1 / log(c + counts / counts.sum()) with counts[0] taken as 0 and w[0] = 0 (metrics.py:414-426), float64 numpy; importable and usable without a GPU.
    An all-zero histogram raises ValueError (the reference divides by zero)."""
    n = np.array(counts, dtype=np.float64)
    if n.ndim != 1 or n.size < 2:
        raise ValueError("class_weights_from_counts: a histogram over at least two classes")
    n[0] = 0
    total = n.sum()
    if not total > 0:
        raise ValueError("class_weights_from_counts: no labelled voxel in the histogram")
    w = 1 / np.log(c + n / total)
    w[0] = 0
    return w


def calculate_class_weights(label_volumes, num_classes: int = 19, c: float = 1.02, device=None) -> np.ndarray:
    """metrics.py:383-426 over an iterable of stored label volumes (numpy arrays or tensors, any shape): the histograms are taken on the device and summed
    there, read back once -> float64 [num_classes] for `class_weights=` of the semantics head.  device: where host volumes are counted (default: the current one)"""
    total = None
    for v in label_volumes:
        t = torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v
        if not t.is_cuda:
            t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()), non_blocking=True)
        n = label_class_counts(t, num_classes)
        total = n if total is None else total + n
    if total is None:
        raise ValueError("calculate_class_weights: no label volume")
    return class_weights_from_counts(total.cpu().numpy(), c)
