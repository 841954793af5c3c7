"""Records tests/golden/g26_det_eval.npz from the reference's own nerf_rpn/eval.py, run on the CPU in fp32.
    python tools/gen_golden_det_eval.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_det_eval.py --search       (no reference needed: prints the first seed that meets the conditions below, per box form)

eval.py is loaded from its file (its name shadows a builtin).  Its only import from the project is model.utils.box_iou_3d, which for oriented boxes goes through
model.rotated_iou.oriented_iou_loss and its compiled vertex sort: the imports get the stand-ins of tools/gen_golden_fcos.py (load_reference), and
model/utils.py:412 calls Tensor.cuda() unconditionally, so Tensor.cuda is patched to the identity for the duration of the run, as in tools/gen_golden_rpn_post.py.

Recorded, axis-aligned (prefix a_) and oriented (prefix o_), for the first four scenes of tests/_det_eval_ref.SCENES (the fifth has detections and no ground truth,
where the reference raises IndexError):
  evaluate_box_proposals_recall for every limit of LIMITS and both threshold sets (key r{limit}_t{50|25}_): gt_overlaps, recalls, ar, num_pos;
  evaluate_box_proposals_ap for every threshold of AP_THRESHOLDS and top_k of TOP_KS (key p{threshold in percent}_k{top_k or 0}_): ap, precisions, recalls,
  num_det (the reference's tp + fp).
The inputs are NOT stored: they are tests/_det_eval_ref.make_scenes(SEED[ncols], ncols), and the file carries their float64 sums (boxes, scores, gt).

Conditions on the seed, asserted here from the restatement (tests/_det_eval_ref.py), never from code under test: every IoU that takes part in a decision is at
least MARGIN away from every threshold used; no greedy step and no arg-max chooses between two positive IoUs closer than MARGIN; all scores are distinct; in at
least one scene the greedy matching differs from the per-column maxima; at every AP threshold and top_k at least one detection is a false positive only because
its box was already claimed.

Precision: the reference only runs in fp32 (with float64 inputs its own assert at eval.py:53 fails), so this is an fp32 recording, stored as fp32 / fp64 scalars."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _det_eval_ref as E  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g26_det_eval.npz")
CASES = (("a_", 6), ("o_", 7))


def search(limit):
    for _, ncols in CASES:
        for seed in range(limit):
            m = E.decision_margins(E.make_scenes(seed, ncols))
            if E.conditions_hold(m):
                print(f"ncols={ncols}: seed {seed}  " + "  ".join(f"{k} {v:.3g}" if isinstance(v, float) else f"{k} {v}" for k, v in m.items()))
                break
        else:
            print(f"ncols={ncols}: no seed below {limit}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=64, help="print the first seed that meets the conditions, per box form")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    from tools.gen_golden_fcos import load_reference
    load_reference(args.reference)
    spec = importlib.util.spec_from_file_location("nerf_rpn_eval", os.path.join(args.reference, "nerf_rpn", "eval.py"))
    ref = importlib.util.module_from_spec(spec)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    rec = dict(limits=np.array(E.LIMITS, dtype=np.int32), top_ks=np.array([k or 0 for k in E.TOP_KS], dtype=np.int32), ap_thresholds=np.array(E.AP_THRESHOLDS, dtype=np.float64),
               shapes=np.array(E.SCENES[:E.RECORDED], dtype=np.int32))
    try:
        spec.loader.exec_module(ref)
        for pre, ncols in CASES:
            seed = E.SEED[ncols]
            scenes = E.make_scenes(seed, ncols)
            m = E.decision_margins(scenes)
            assert E.conditions_hold(m), (pre, m)
            part = scenes[:E.RECORDED]
            lists = [[torch.from_numpy(sc[k]) for sc in part] for k in range(3)]
            assert all(t.dtype == torch.float32 for ts in lists for t in ts)
            rec[pre + "seed"] = np.int32(seed)
            rec[pre + "input_sums"] = E.input_sums(scenes)
            for limit in E.LIMITS:
                for lo in (0.5, 0.25):
                    thr = None if lo == 0.5 else torch.from_numpy(E.recall_thresholds(lo))
                    r = ref.evaluate_box_proposals_recall(*lists, thresholds=thr, limit=limit)
                    key = f"{pre}r{limit}_t{int(lo * 100)}_"
                    rec[key + "gt_overlaps"] = r["gt_overlaps"].numpy().astype(np.float32)
                    rec[key + "recalls"] = r["recalls"].numpy().astype(np.float32)
                    rec[key + "ar"] = np.float32(r["ar"].item())
                    rec[key + "num_pos"] = np.int64(r["num_pos"])
            for t in E.AP_THRESHOLDS:
                for k in E.TOP_KS:
                    r = ref.evaluate_box_proposals_ap(*lists, iou_thresh=t, top_k=k)
                    key = f"{pre}p{int(t * 100)}_k{k or 0}_"
                    rec[key + "ap"] = np.float64(r["ap"].item())
                    rec[key + "precisions"] = r["precisions"].numpy().astype(np.float32)
                    rec[key + "recalls"] = r["recalls"].numpy().astype(np.float32)
                    rec[key + "num_det"] = r["num_det"].numpy().astype(np.int64)
            print(pre, {k: (f"{v:.3g}" if isinstance(v, float) else v) for k, v in m.items()})
    finally:
        torch.Tensor.cuda = cuda
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
