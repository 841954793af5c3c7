"""Records tests/golden/g21_rpn_proposals.npz from the reference's own RPN Python (model.rpn), run on the CPU.
    python tools/gen_golden_rpn_post.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_rpn_post.py --search       (no reference needed: prints the head seeds that meet the conditions below)

The reference's inference half is plain torch except for batched_nms of oriented boxes, which goes through model.rotated_iou.oriented_iou_loss and its compiled
vertex sort: the imports get the stand-ins of tools/gen_golden_fcos.py (load_reference), and model/utils.py:412 calls Tensor.cuda() unconditionally, so
Tensor.cuda is patched to the identity for the duration of the run, as in tools/gen_golden_fcos_post.py.

Recorded, for the geometry of tests/_rpn_ref.py (mesh 32^3, grids 8^3 .. 1^3, 13 anchors per location, 7 605 per scene, two scenes of original sizes
(32,32,32) and (24,28,20)) and the configuration tests/_rpn_post_ref.CFG, axis-aligned (prefix a_) and oriented (prefix o_): box_coder.decode_list at every
32nd anchor (d_index, d_boxes), and of filter_proposals per scene the count and, for all scenes concatenated, levels, boxes, scores and the anchor index of each
row (found by matching the row to the decode of all anchors; the reference does not return it).  Head tensors are NOT stored: they are
tests/_rpn_post_ref.inputs(HEAD_SEED, rotated) over tests/_rpn_ref.make_heads, and the file carries their float64 sums.

Conditions on the head seed, asserted here from the restatement (tests/_rpn_post_ref.py), never from code under test:
  every decision margin is at least MARGIN; pre_nms_top_n is no larger than the unmasked anchor count of every level that has masked anchors (so the
  reference's open tie order among score-0 fills never matters); no oriented centre lies outside the mesh (where the reference pairs boxes with the wrong
  scores); no two selected logits are equal.

Precision: fp32 inputs, the reference evaluated on them in float64, results stored as float64 (they are small), the decoded subsample as fp32."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _rpn_post_ref as P  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g21_rpn_proposals.npz")
CASES = (("a_", False), ("o_", True))


def conditions(seed, rotated):
    """-> (ok, margins, facts) for make_heads(seed) under the recorded configuration"""
    obj, reg = P.inputs(seed, rotated)
    res, m = P.proposals(obj, reg, ori=R.ORI, rotated=rotated, **P.CFG)
    n_level = [o[0].numel() for o in obj]
    ok = all(v >= P.MARGIN for v in m.values())
    for b, r in enumerate(res):
        for k, (u, n) in enumerate(zip(r["unmasked"], n_level)):
            ok = ok and (u == n or min(P.CFG["pre_nms_top_n"], n) <= u)
        sel = len(r["pre_keys"])
        if rotated:                      # nothing dropped: in particular no centre outside the mesh
            ok = ok and sel == sum(min(P.CFG["pre_nms_top_n"], n) for n in n_level)
        ok = ok and all(torch.unique(r["pre_keys"][r["pre_level"] == k]).numel() == int((r["pre_level"] == k).sum()) for k in range(len(obj)))
        ok = ok and 0 < len(r["scores"]) < sel
    return ok, m, dict(before_nms=[len(r["pre_keys"]) for r in res], results=[len(r["scores"]) for r in res])


def search(limit):
    for rotated in (False, True):
        for seed in range(limit):
            ok, m, facts = conditions(seed, rotated)
            if ok:
                print(f"rotated={rotated}: seed {seed}  " + "  ".join(f"{k} {v:.3g}" for k, v in m.items()) + f"  {facts}")
                break
        else:
            print(f"rotated={rotated}: no seed below {limit}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=64, help="print the first head seed that meets the conditions, per box form")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    from tools.gen_golden_fcos import load_reference
    load_reference(args.reference)
    M = importlib.import_module("model.rpn")
    N = len(R.ORI)
    gen = M.AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS, is_normalized=False)
    meshes = torch.zeros((N, 4, *R.MESH))
    features = [torch.zeros((N, 1, *g)) for g in R.GRIDS]
    _, non_cat = gen(meshes, features)
    non_cat = [[a.double() for a in scene] for scene in non_cat]
    rec = dict(mesh=np.array(R.MESH, dtype=np.int32), grids=np.array(R.GRIDS, dtype=np.int32), ori=np.array(R.ORI, dtype=np.int32),
               pre_nms_top_n=np.int32(P.CFG["pre_nms_top_n"]), post_nms_top_n=np.int32(P.CFG["post_nms_top_n"]), nms_thresh=np.float64(P.CFG["nms_thresh"]),
               score_thresh=np.float64(P.CFG["score_thresh"]))
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        for pre, rotated in CASES:
            seed = P.HEAD_SEED[rotated]
            ok, margins, facts = conditions(seed, rotated)
            assert ok, (pre, margins, facts)
            C, nb = (8, 7) if rotated else (6, 6)
            obj, reg = P.inputs(seed, rotated)
            rpn = M.RegionProposalNetwork(gen, None, R.FG, R.BG, R.BATCH, R.FRACTION, dict(training=1, testing=P.CFG["pre_nms_top_n"]),
                                          dict(training=1, testing=P.CFG["post_nms_top_n"]), P.CFG["nms_thresh"], score_thresh=P.CFG["score_thresh"], rotated_bbox=rotated)
            rpn.eval()
            o, _, unflat = M.concat_box_prediction_layers([t.double() for t in obj], [t.double() for t in reg], C)
            n_level = [t[0].numel() for t in obj]
            masks = rpn.get_padding_masks(meshes, features, [tuple(v) for v in R.ORI])
            decoded = rpn.box_coder.decode_list(unflat, non_cat)
            lvl_col, props = decoded[..., -1], decoded[..., :nb]
            boxes, scores, levels = rpn.filter_proposals(props, o, lvl_col, [tuple(R.MESH)] * N, n_level, masks)
            index = []
            for b in range(N):
                for row in boxes[b]:
                    clipped = torch.minimum(props[b].clamp_min(0.0), torch.tensor(R.MESH, dtype=torch.float64).repeat(2)) if not rotated else props[b]
                    d = (clipped - row[None, :]).abs().amax(1)
                    assert d.min().item() < 1e-9 and int((d < 1e-9).sum()) == 1, d.min().item()
                    index.append(int(d.argmin()))
            d_index = torch.arange(0, props.shape[1], 32)
            rec[pre + "head_seed"] = np.int32(seed)
            rec[pre + "head_sums"] = np.array([sum(t.double().sum().item() for t in ts) for ts in (obj, reg)], dtype=np.float64)
            rec[pre + "d_index"] = d_index.numpy().astype(np.int32)
            rec[pre + "d_boxes"] = props[:, d_index].numpy().astype(np.float32)
            rec[pre + "counts"] = np.array([len(s) for s in scores], dtype=np.int32)
            rec[pre + "level"] = torch.cat(levels).numpy().astype(np.int64)
            rec[pre + "index"] = np.array(index, dtype=np.int64)
            rec[pre + "boxes"] = torch.cat(boxes).double().numpy()
            rec[pre + "scores"] = torch.cat(scores).double().numpy()
            print(pre, margins, facts, "recorded counts", rec[pre + "counts"].tolist())
    finally:
        torch.Tensor.cuda = cuda
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
