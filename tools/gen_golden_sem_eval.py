"""Records tests/golden/g26_sem_eval.npz from the reference's own SwinTransformer_VoxelSemantics_Pretrained_Skip.output_metrics
(nerf_rpn/model/feature_extractor.py:2748-2806), run on the CPU in fp32.
    python tools/gen_golden_sem_eval.py --reference PATH_TO_REFERENCE_CHECKOUT

The class is imported with the stand-ins of oracle/gen_golden_heads.py (torchvision's StochasticDepth / MLP / Permute, np.float, an empty torchmetrics) and built
once at resolution 32; for every case its `out_channels`, `input_resolution`, `criterion` and `iou_loss` are set to the case's (these four and `transform` are all
that output_metrics reads).  Its network is never run: `pred` is the case's seeded logits.

torch.histc is wrapped for the duration of the run to cast an integer argument to float.  output_metrics reaches it through intersectionAndUnionGPU
(metrics.py:505-513) with int64 labels; the reference makes that call only on CUDA tensors, where ATen accepts integers, and the CPU kernel rejects them.  The
wrapper changes no value: the labels are below 2^24.

The evaluation loop (nerf_rpn/run_voxel_semantics.py:805-958) cannot be imported here (it parses arguments and opens datasets at import).  Its three meters and
five formulas are restated below on the recorded per-batch counts of tests/_sem_eval_ref.EVAL_SEQUENCE: sums of the per-batch numpy arrays, then
I / (U + 1e-10), I / (T + 1e-10), their means, and sum I / (sum T + 1e-10); `accuracy` is the loop's per-batch figure.  The loop holds the histograms as the fp32
arrays that histc returned; the restatement evaluates the same formulas in float64 (the counts are exact integers in both).

Stored per case (key prefix = the case's name): intersection, union, target (the reference's fp32 histograms, exact integers, as int64), ce and iou_val (fp32),
and tests/_sem_eval_ref.checksum of pred_labels_vis and target_vis.  The inputs are NOT stored: they are tests/_sem_eval_ref.inputs(case); the file carries
their float64 sums.  The arg-max margin of every case is asserted here from the restatement, never from code under test."""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _sem_eval_ref as S  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g26_sem_eval.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from oracle.gen_golden import _install_shims
    _install_shims()
    tm = types.ModuleType("torchmetrics")
    tm.JaccardIndex = object
    sys.modules["torchmetrics"] = tm
    sys.path.insert(0, args.reference)
    sys.path.insert(0, os.path.join(args.reference, "nerf_rpn"))
    from nerf_rpn.model import feature_extractor as FE
    from nerf_rpn.model.metrics import mIoULoss_new
    with contextlib.redirect_stdout(io.StringIO()):
        head = FE.SwinTransformer_VoxelSemantics_Pretrained_Skip(resolution=32, out_channels=19, is_eval=True)
    histc = torch.histc
    torch.histc = lambda x, *a, **k: histc(x if x.is_floating_point() else x.float(), *a, **k)
    rec, seq = {}, []
    try:
        for case in S.GOLDEN_CASES:
            name, K, _, shape, B, _, _ = case
            assert shape[0] == shape[1] == shape[2]
            logits, labels, cw, ties = S.inputs(case)
            assert not ties.any() and S.argmax_margin(logits) >= S.MARGIN, name
            head.out_channels, head.input_resolution = K, shape[0]
            head.criterion, head.iou_loss = torch.nn.CrossEntropyLoss(weight=cw), mIoULoss_new(n_classes=K)
            with torch.no_grad(), contextlib.redirect_stdout(io.StringIO()):
                ce, m, pv, tv = head.output_metrics([labels[b][None] for b in range(B)], logits)
            for key in ("intersection", "union", "target"):
                h = m[key].double().numpy()
                assert m[key].dtype == torch.float32 and (h == np.round(h)).all() and h.max() < 2 ** 24
                rec[f"{name}.{key}"] = h.astype(np.int64)
            rec[f"{name}.ce"], rec[f"{name}.iou_val"] = np.float32(ce.item()), np.float32(m["iou_val"].item())
            assert pv.dtype == torch.int64 and tv.dtype == torch.int64 and tuple(pv.shape) == (B,) + tuple(shape)
            rec[f"{name}.pred_vis_sums"], rec[f"{name}.target_vis_sums"] = S.checksum(pv), S.checksum(tv)
            rec[f"{name}.input_sums"] = np.array([logits.double().sum().item(), labels.double().sum().item(), 0.0 if cw is None else cw.double().sum().item()])
            if name in S.EVAL_SEQUENCE:
                seq.append([m[k].cpu().numpy() for k in ("intersection", "union", "target")])
            print(name, "ce %.6f iou %.6f" % (ce.item(), m["iou_val"].item()), "intersection", rec[f"{name}.intersection"].sum(), "target", rec[f"{name}.target"].sum())
    finally:
        torch.histc = histc
    assert [c[0] for c in S.GOLDEN_CASES[:len(seq)]] == S.EVAL_SEQUENCE
    # the loop's bookkeeping: AverageMeter.sum += val for the three arrays of every batch, `accuracy` from the batch's own arrays
    sums = [sum(b[j].astype(np.float64) for b in seq) for j in range(3)]
    rec["loop.accuracy"] = np.array([b[0].astype(np.float64).sum() / (b[2].astype(np.float64).sum() + 1e-10) for b in seq])
    iou_class = sums[0] / (sums[1] + 1e-10)
    accuracy_class = sums[0] / (sums[2] + 1e-10)
    rec["loop.iou_class"], rec["loop.accuracy_class"] = iou_class, accuracy_class
    rec["loop.mIoU"], rec["loop.mAcc"] = np.float64(np.mean(iou_class)), np.float64(np.mean(accuracy_class))
    rec["loop.allAcc"] = np.float64(sums[0].sum() / (sums[2].sum() + 1e-10))
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays; mIoU {rec['loop.mIoU']:.6f} mAcc {rec['loop.mAcc']:.6f} allAcc {rec['loop.allAcc']:.6f}")


if __name__ == "__main__":
    main()
