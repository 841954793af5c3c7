"""Records tests/golden/g19_fcos_post.npz from the reference's own FCOSPostProcessor, run on the CPU.
    python tools/gen_golden_fcos_post.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_fcos_post.py --search     (no reference needed: prints head seeds whose decision margins are all >= 1e-5)

The reference's nerf_rpn/model/fcos/inference.py is plain torch over fcos/utils.py, whose imports get the stand-ins of tools/gen_golden_fcos.py
(the compiled `sort_vertices` module and `cuda_op.cuda_ext.sort_v` from tests/_rotated_ref.sort_vertices_ref, bare namespace stubs for the
packages `model`, `model.fcos` and `model.rotated_iou`).  inference.py:150 and fcos/utils.py:253 call Tensor.cuda() unconditionally, so
Tensor.cuda is patched to the identity for the duration of the run.

Recorded, for the geometry of tests/_fcos_ref.py (strides 4/8/16/32, feature sizes (20,18,17) .. (3,3,3), three scenes with original sizes
(80,72,68), (61,72,50), (80,40,68) and their padding masks) and the configuration tests/_fcos_post_ref.CFG (pre_nms_thresh 0.05, pre_nms_top_n
300, nms_thresh 0.3, fpn_post_nms_top_n 100, min_size 2.0), for use_obb False (prefix a_) and True (prefix o_): per scene the kept count, and
for all scenes concatenated the level indices, boxes and scores of the outputs, plus the location index of every output row within its level
(found by matching the reference's box to the decoded boxes of that level; the reference does not return it).  The head outputs themselves
are NOT stored: they are tests/_fcos_ref.make_heads(HEAD_SEED, use_obb, False), and the file carries their float64 sums so that a drift of
the generator is noticed.

Precision: fp32 inputs, the reference evaluated on them in float64, results stored as float64 (they are small)."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _fcos_post_ref as P  # noqa: E402
from tools.gen_golden_fcos import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g19_fcos_post.npz")
CASES = (("a_", False), ("o_", True))


def margins(seed, use_obb):
    locs, cls, reg, ctr, sizes, masks = P.inputs(seed, use_obb)
    res, m = P.postprocess(locs, cls, reg, ctr, sizes, masks, **P.CFG)
    return m, [len(r["pre_scores"]) for r in res], [len(r["scores"]) for r in res]


def search(limit):
    for use_obb in (False, True):
        for seed in range(1800, 1800 + limit):
            m, pre, kept = margins(seed, use_obb)
            if all(v >= P.MARGIN for v in m.values()):
                print(f"use_obb={use_obb}: seed {seed}  " + "  ".join(f"{k} {v:.3g}" for k, v in m.items()) + f"  before NMS {pre}  results {kept}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=12, help="print the head seeds from 1800 on with every decision margin >= 1e-5")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    load_reference(args.reference)
    inference = importlib.import_module("model.fcos.inference")
    rec = dict(pre_nms_thresh=np.float64(P.CFG["pre_nms_thresh"]), pre_nms_top_n=np.int32(P.CFG["pre_nms_top_n"]), nms_thresh=np.float64(P.CFG["nms_thresh"]),
               fpn_post_nms_top_n=np.int32(P.CFG["fpn_post_nms_top_n"]), min_size=np.float64(P.CFG["min_size"]))
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for pre, use_obb in CASES:
            seed = P.HEAD_SEED[use_obb]
            locs, cls, reg, ctr, sizes, masks = P.inputs(seed, use_obb)
            fn = inference.FCOSPostProcessor(P.CFG["pre_nms_thresh"], P.CFG["pre_nms_top_n"], P.CFG["nms_thresh"], P.CFG["fpn_post_nms_top_n"], P.CFG["min_size"], 1, False, use_obb)
            boxes, scores = fn([l.double() for l in locs], [t.double() for t in cls], [t.double() for t in reg], [t.double() for t in ctr], sizes, masks)
            ours, _ = P.postprocess(locs, cls, reg, ctr, sizes, masks, **P.CFG)
            index = []
            for b, o in zip(boxes, ours):
                for row in b:
                    sel = torch.nonzero(o["pre_level"] == int(row[0])).reshape(-1)
                    d = (o["pre_boxes"][sel] - row[1:].double()).abs().amax(1)
                    assert d.min().item() < 1e-6, d.min().item()
                    index.append(int(o["pre_index"][sel[d.argmin()]]))
            rec[pre + "head_seed"] = np.int32(seed)
            rec[pre + "head_sums"] = np.array([sum(t.double().sum().item() for t in ts) for ts in (cls, reg, ctr)], dtype=np.float64)
            rec[pre + "counts"] = np.array([len(s) for s in scores], dtype=np.int32)
            rec[pre + "level"] = torch.cat([b[:, 0] for b in boxes]).numpy().astype(np.int64)
            rec[pre + "index"] = np.array(index, dtype=np.int64)
            rec[pre + "boxes"] = torch.cat([b[:, 1:] for b in boxes]).double().numpy()
            rec[pre + "scores"] = torch.cat(scores).double().numpy()
    finally:
        torch.Tensor.cuda = cuda
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
