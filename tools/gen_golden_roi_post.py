"""Records tests/golden/g27_roi_post.npz from the reference's own Trainer.filter_proposals, run on the CPU in float64.
    python tools/gen_golden_roi_post.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_roi_post.py --search      (no reference needed: prints scene seeds whose decision margins are all >= 1e-3)

nerf_rpn/run_rpn_detect.py is loaded as a module with stand-ins for what it imports and this recording does not need: `wandb` and `tqdm` (absent or beside the
point), `datasets`, `eval`, `model.feature_extractor` and `model.detector` (empty modules with the imported names), and the stand-ins of
tools/gen_golden_fcos.py for the compiled vertex sort behind model.utils.  model.utils itself (clip_boxes_to_mesh, remove_small_boxes, nms, box_iou_3d) is
the reference's own file.  Trainer.filter_proposals is called as the unbound method with a namespace for `self` (args.rotated_bbox, args.nms_thresh,
min_size).  box_iou_3d calls Tensor.cuda() for oriented boxes, so Tensor.cuda is patched to the identity for the duration of the run.

Recorded, for tests/_roi_post_ref.gold_inputs (two scenes of 24 rows; axis-aligned, prefix a_, and oriented, prefix o_; all oriented centres inside the mesh,
because the reference's clip misaligns boxes and scores otherwise) and the score thresholds 0.5, 0.8 and 0.3 (suffix _t50, _t80, _t30), nms_thresh 0.3,
min_size 1e-3: per scene the kept count, and for all scenes concatenated the source row of every output (the row indices are handed over as gt_labels and come
back in final_gt_labels), the boxes and the [k, 2] probabilities.  With two classes every row passes at 0.5; at 0.3 rows with both probabilities >= 0.3 enter
the NMS twice (the second copy has IoU 1 with the first), which this file pins.  The inputs are NOT stored: they are regenerated from the seeds, and the file
carries their float64 sums so that a drift of the generator is noticed.

Precision: fp32 inputs, the reference evaluated on them in float64, results stored as float64 (they are small)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _roi_post_ref as P  # noqa: E402
from tools.gen_golden_fcos import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g27_roi_post.npz")
CASES = (("a_", False), ("o_", True))


def load_trainer(ref):
    load_reference(ref)                                    # `model` as a bare namespace over the reference's directory, the vertex sort stand-ins

    def stub(name, *names):
        m = types.ModuleType(name)
        for n in names:
            setattr(m, n, None)
        sys.modules[name] = m

    stub("wandb")
    stub("tqdm", "tqdm")
    stub("datasets", "RPNClassificationDataset")
    stub("eval", "evaluate_box_proposals_ap")
    stub("model.feature_extractor", "Bottleneck", "ResNet_FPN_256", "ResNet_FPN_64", "VGG_FPN", "SwinTransformer_FPN")
    stub("model.detector", "ProposalTargetLayer", "ROIPool", "RCNN", "Classification_Model")
    sys.path.insert(0, os.path.join(ref, "nerf_rpn"))
    try:
        return importlib.import_module("run_rpn_detect").Trainer
    finally:
        sys.path.pop(0)


def margins(seed, rotated):
    probs, rois, counts, mesh = P.gold_dense(rotated, seed)
    worst, kept = {}, []
    for thr in P.GOLD["thresholds"]:
        res, m = P.postprocess(probs, None, rois, counts, mesh, thr, P.GOLD["nms_thresh"], P.MIN_SIZE, False, "any", probabilities=True)
        kept.append([len(r["scores"]) for r in res])
        for k, v in m.items():
            worst[k] = min(worst.get(k, float("inf")), v)
    return worst, kept


def search(limit):
    for rotated in (False, True):
        for seed in range(limit):
            m, kept = margins(seed, rotated)
            if all(v >= P.MARGIN for v in m.values()):
                print(f"rotated={rotated}: seed {seed}  " + "  ".join(f"{k} {v:.3g}" for k, v in m.items()) + f"  results {kept}")
                break
        else:
            print(f"rotated={rotated}: no seed below {limit}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=400, help="print the first scene seeds with every decision margin >= 1e-3")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    Trainer = load_trainer(args.reference)
    rec = dict(nms_thresh=np.float64(P.GOLD["nms_thresh"]), min_size=np.float64(P.MIN_SIZE), thresholds=np.array(P.GOLD["thresholds"], dtype=np.float64))
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for pre, rotated in CASES:
            m, _ = margins(P.GOLD_SEED[rotated], rotated)
            assert all(v >= P.MARGIN for v in m.values()), m
            boxes, probs, mesh = P.gold_inputs(rotated)
            rec[pre + "seed"] = np.int32(P.GOLD_SEED[rotated])
            rec[pre + "input_sums"] = P.input_sums(boxes, probs)
            me = types.SimpleNamespace(args=types.SimpleNamespace(rotated_bbox=rotated, nms_thresh=P.GOLD["nms_thresh"]), min_size=P.MIN_SIZE)
            for thr in P.GOLD["thresholds"]:
                rows = [torch.arange(b.shape[0]) for b in boxes]
                fb, fs, fl = Trainer.filter_proposals(me, [b.double() for b in boxes], [p.double() for p in probs], rows, mesh, score_threhold=thr)
                tag = f"_t{int(round(thr * 100))}"
                rec[pre + "counts" + tag] = np.array([len(s) for s in fs], dtype=np.int32)
                rec[pre + "index" + tag] = torch.cat(fl).numpy().astype(np.int64)
                rec[pre + "boxes" + tag] = torch.cat(fb).double().numpy()
                rec[pre + "probs" + tag] = torch.cat(fs).double().numpy()
    finally:
        torch.Tensor.cuda = cuda
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
