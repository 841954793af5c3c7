"""Records tests/golden/g20_rpn_targets.npz from the reference's own RPN Python, run on the CPU.
    python tools/gen_golden_rpn.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_rpn.py --search          (no reference needed: prints scene seeds whose decision margins are all >= 1e-3)

The reference's nerf_rpn/model/rpn.py (RegionProposalNetwork), anchor.py, utils.py and coder/ are plain torch except for one import, the compiled
oriented IoU of `model.rotated_iou.oriented_iou_loss`, which no code path used here calls: it gets a stand-in in sys.modules.  The packages
`model` and `model.rotated_iou` are entered as bare namespace stubs so that their __init__ files (which pull in the whole detector) do not run.

Recorded, for the geometry of tests/_rpn_ref.py (mesh 32^3, grids 8^3 .. 1^3, run_rpn.py's anchor set: 13 anchors per location, 7 605 per scene;
scenes of 5 and 3 boxes, original sizes (32,32,32) and (24,28,20); fg 0.35, bg 0.2), axis-aligned (prefix a_) and oriented (prefix o_):
  the base anchor table; the boxes and their per-scene offsets; `labels` of assign_targets_to_anchors; the row of the matched box it returns
  (box max(matched_idxs, 0)); the coder's encoded targets at the anchors listed in t_index (every positive and every 8th anchor: all of them would
  exceed the size that a fixture should have); the sampled set (tests/_rpn_ref.make_flags(FLAG_SEED, labels), the sampler's counts drawn by a numpy
  stream) and compute_loss's objectness and box losses for it.
The head outputs are NOT stored: they are tests/_rpn_ref.make_heads(HEAD_SEED, ...), and the file carries their float64 sums.

Precision: fp32 inputs; the reference evaluated on them in float64 wherever its code lets the dtype through (bbox2delta_sp casts to fp32 itself), results
stored as fp32."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _rpn_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz")
FLAG_SEED = 11
CASES = (("a_", False), ("o_", True))


def load_reference(ref):
    def stub(name, path=None, **attrs):
        m = types.ModuleType(name)
        if path is not None:
            m.__path__ = [path]
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    model = os.path.join(ref, "nerf_rpn", "model")
    stub("model", path=model)
    stub("model.rotated_iou", path=os.path.join(model, "rotated_iou"))
    stub("model.rotated_iou.oriented_iou_loss", cal_iou_3d=None, cal_giou_3d=None, cal_diou_3d=None)
    return importlib.import_module("model.rpn")


def kinds(a):
    """how many anchors of each kind the fixture must contain"""
    lab, m, valid = a["labels"], a["matched"], a["valid"]
    return dict(positive=int(((lab == 1) & ~a["restored"]).sum()), between=int(((m == -2) & valid).sum()), restored=int(a["restored"].sum()), padded=int((~valid).sum()))


def check(seed, rotated):
    a = R.assign(R.make_scene(seed, rotated=rotated, ori=R.ORI), ori=R.ORI, rotated=rotated)
    m, k = R.decision_margins(a), kinds(a)
    ok = all(v >= 1e-3 for v in m.values()) and all(v > 0 for v in k.values()) and all((g > 0).all() for g in a["gtmax"]) and bool(torch.isfinite(a["targets"]).all())
    return ok, m, k


def search(limit):
    for rotated in (False, True):
        for seed in range(limit):
            ok, m, k = check(seed, rotated)
            if ok:
                print(f"rotated={rotated}: seed {seed}  " + "  ".join(f"{n} {v:.3g}" for n, v in m.items()) + "  " + "  ".join(f"{n} {v}" for n, v in k.items()))
                break
        else:
            print(f"rotated={rotated}: no seed below {limit}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=200, help="print the first scene seeds with every decision margin >= 1e-3 and every kind of anchor")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    M = load_reference(args.reference)
    N = len(R.NBOX)
    gen = M.AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS, is_normalized=False)
    meshes = torch.zeros((N, 4, *R.MESH))
    features = [torch.zeros((N, 1, *g)) for g in R.GRIDS]
    anchors, _ = gen(meshes, features)
    rec = dict(base=torch.cat(gen.cell_anchors).numpy().astype(np.float32), base_counts=np.array([len(c) for c in gen.cell_anchors], dtype=np.int32),
               num_anchors=np.array(gen.num_anchors_per_location(), dtype=np.int32), mesh=np.array(R.MESH, dtype=np.int32), grids=np.array(R.GRIDS, dtype=np.int32),
               ori=np.array(R.ORI, dtype=np.int32), fg=np.float32(R.FG), bg=np.float32(R.BG), batch=np.int32(R.BATCH), fraction=np.float32(R.FRACTION),
               head_seed=np.int32(R.HEAD_SEED), flag_seed=np.int32(FLAG_SEED))
    for pre, rotated in CASES:
        ok, margins, have = check(R.SEED[rotated], rotated)
        assert ok, (pre, margins, have)
        boxes = R.make_scene(R.SEED[rotated], rotated=rotated, ori=R.ORI)
        rpn = M.RegionProposalNetwork(gen, None, R.FG, R.BG, R.BATCH, R.FRACTION, dict(training=1, testing=1), dict(training=1, testing=1), 0.3, rotated_bbox=rotated)
        masks = rpn.get_padding_masks(meshes, features, [tuple(o) for o in R.ORI])
        anc64, gts = [a.double() for a in anchors], [b.double() for b in boxes]
        labels, matched_boxes = rpn.assign_targets_to_anchors(anc64, gts, masks)
        targets = rpn.box_coder.encode(matched_boxes, anc64)
        labels, targets = torch.stack(labels), torch.stack([t.double() for t in targets])
        rows = torch.stack([(mb[:, None, :] == g[None, :, :]).all(-1).double().argmax(1) for mb, g in zip(matched_boxes, gts)])
        assert all(torch.equal(g[r], mb) for g, r, mb in zip(gts, rows, matched_boxes))
        C = 8 if rotated else 6
        flags = R.make_flags(FLAG_SEED, labels)
        obj, reg = R.make_heads(R.HEAD_SEED, N, C)
        rpn.fg_bg_sampler = lambda _labels: ([f == 1 for f in flags], [f == 2 for f in flags])
        o, r, _ = M.concat_box_prediction_layers([t.double() for t in obj], [t.double() for t in reg], C)
        proposals = rpn.box_coder.decode(r, anc64).view(-1, 7 if rotated else 6)
        out = rpn.compute_loss(o, r, list(labels), list(targets), proposals, matched_boxes, max(R.MESH))
        t_index = torch.nonzero(((labels == 1) | (torch.arange(labels.shape[1])[None, :] % 8 == 0)).reshape(-1))[:, 0]
        rec[pre + "boxes"] = torch.cat(boxes, 0).numpy()
        rec[pre + "offsets"] = np.cumsum([0] + [b.shape[0] for b in boxes]).astype(np.int32)
        rec[pre + "labels"] = labels.numpy().astype(np.int8)
        rec[pre + "matched_row"] = rows.numpy().astype(np.int16)
        rec[pre + "t_index"] = t_index.numpy().astype(np.int32)
        rec[pre + "targets"] = targets.reshape(-1, C)[t_index].numpy().astype(np.float32)
        rec[pre + "flags"] = flags.numpy()
        rec[pre + "losses"] = np.array([float(out[0]), float(out[1])], dtype=np.float32)
        rec[pre + "head_sums"] = np.array([sum(t.double().sum().item() for t in ts) for ts in (obj, reg)], dtype=np.float64)
        print(pre, margins, have, "positives per scene", (labels == 1).sum(1).tolist(), "ignored", (labels == -1).sum(1).tolist(), "losses", rec[pre + "losses"])
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
