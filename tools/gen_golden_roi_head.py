"""Records tests/golden/g22_roi_head.npz from the reference's own RoI stage (model.detector), run on the CPU.
    python tools/gen_golden_roi_head.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_roi_head.py --search       (no reference needed: prints the seeds that meet the conditions below)

The reference's imports get the stand-ins of tools/gen_golden_fcos.py (load_reference), and model.feature_extractor (the backbones, which the RoI stage does not
use) an empty one.  detector.py calls Tensor.cuda() and passes Tensor.get_device() to
.to(), so for the duration of the run Tensor.cuda is the identity and Tensor.get_device returns the tensor's device.  To evaluate in float64 where the reference
allows, the inputs (fp32 values) are converted to float64, the default dtype is float64 and the name torch.float, with which detector.py casts its grids and its
rotation, is bound to float64 for the run.

Recorded for two runs, axis-aligned (prefix a_) and oriented (prefix o_), over tests/_roi_head_ref.gold_inputs (mesh 32^3, maps 16^3 / 8^3 / 4^3 of 4 channels,
two scenes of 8 RoIs and 3 boxes): ProposalTargetLayer in evaluation mode (labels, matched boxes) and in sampling mode under np.random.seed (labels, the kept
indices recovered by matching rows, the number of foreground slots); ROIPool('pooling') on the sampled RoIs with remap off, and for the axis-aligned run with
remap on (with its levels); Classification_Model(is_sample=True, is_reg=True) on a flattening RCNN with the parameters of _roi_head_ref.gold_head: the regression
targets (captured at box_coder.encode_single), the RoIs it encoded against, the two losses and the decoded proposals.  Inputs are NOT stored: the file carries
their float64 sums.

Conditions on the seeds, asserted here from the restatement (tests/_roi_head_ref.py), never from code under test: every margin is at least MARGIN = 1e-3; every
enlarged RoI lies inside its map; every scene has both foreground and background candidates."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _roi_head_ref as H  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g22_roi_head.npz")
CASES = (("a_", False), ("o_", True))
NP_SEED = 5
G = H.GOLD


def scene_conditions(seed, rotated):
    """the conditions that do not need the maps -> (ok, facts)"""
    rois, gts, labs = H.make_scene(seed, rotated, N=G["N"], K=G["K"], G=G["G"])
    _, _, _, m = H.targets(rois, gts, labs)
    ok = all(m[k] >= H.MARGIN for k in ("iou_fg", "iou_bg", "iou_top2")) and all(len(f) > 0 and len(b) > 0 for f, b in m["candidates"])
    dense = torch.stack(rois)
    _, pm, _ = H.pool(H.make_maps(0, 1, G["N"]), dense, out=G["out"], rotated=rotated, want_values=False)
    ok = ok and pm["floor"] >= H.MARGIN and pm["inside"]
    facts = {k: m[k] for k in ("iou_fg", "iou_bg", "iou_top2")}
    facts.update(floor=pm["floor"], inside=pm["inside"], ragged=pm["ragged"], cands=[(len(f), len(b)) for f, b in m["candidates"]])
    if not rotated:
        kmin, kmax = H.mapper_range(H.SCALES)
        _, lm = H.level_map(dense[..., 1:], kmin, kmax, G["max_res"], len(H.SCALES))
        ok, facts["level"] = ok and lm >= H.MARGIN, lm
    return ok, facts


def map_conditions(seed, map_seed, rotated):
    rois, _, _ = H.make_scene(seed, rotated, N=G["N"], K=G["K"], G=G["G"])
    _, pm, _ = H.pool(H.make_maps(map_seed, G["C"], G["N"]), torch.stack(rois), out=G["out"], rotated=rotated)
    return pm["cell_gap"] >= H.MARGIN and pm["padded_cells"] > 0, dict(cell_gap=pm["cell_gap"], padded_cells=pm["padded_cells"])


def search(limit):
    for rotated in (False, True):
        for seed in range(limit):
            ok, facts = scene_conditions(seed, rotated)
            if not ok:
                continue
            for map_seed in range(limit):
                ok2, f2 = map_conditions(seed, map_seed, rotated)
                if ok2:
                    print(f"rotated={rotated}: (scene seed, map seed) = ({seed}, {map_seed})  {facts}  {f2}")
                    break
            else:
                continue
            break
        else:
            print(f"rotated={rotated}: no seed below {limit}")


def rows_in(rows, table):
    idx = []
    for row in rows:
        hit = torch.nonzero((table == row[None, :]).all(1)).view(-1)
        assert hit.numel() == 1, hit
        idx.append(int(hit))
    return idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=400, help="print the first seeds that meet the conditions, per box form")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    from tools.gen_golden_fcos import load_reference
    load_reference(args.reference)
    import types
    sys.modules["model.feature_extractor"] = types.ModuleType("model.feature_extractor")     # the backbones: detector.py imports them but the RoI stage uses none
    saved = (torch.Tensor.cuda, torch.Tensor.get_device, torch.float, torch.get_default_dtype())
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.Tensor.get_device = lambda self: self.device
    torch.float = torch.float64
    torch.set_default_dtype(torch.float64)
    rec = dict(np_seed=np.int32(NP_SEED), max_res=np.int32(G["max_res"]), out=np.array(G["out"], dtype=np.int32))
    try:
        M = importlib.import_module("model.detector")
        for pre, rotated in CASES:
            seed, map_seed = H.GOLD_SEED[rotated]
            ok, facts = scene_conditions(seed, rotated)
            ok2, f2 = map_conditions(seed, map_seed, rotated)
            assert ok and ok2, (pre, facts, f2)
            rois32, gts32, labs32, maps32 = H.gold_inputs(rotated)
            rois, gts, labs = [r.double() for r in rois32], [g.double() for g in gts32], [l.double() for l in labs32]
            feats = [[m[i].double() for m in maps32] for i in range(G["N"])]
            fresh = lambda: [r.clone() for r in rois]
            layer = M.ProposalTargetLayer(2, batch_size=G["N"] * G["R"], fg_fraction=0.5, fg_threshold=H.FG, bg_threshold=H.BG, is_rotated_bbox=rotated)
            e_lab, e_rois, e_gt = layer(fresh(), gts, labs, is_sample=False)
            np.random.seed(NP_SEED)
            s_lab, s_rois, s_gt = layer(fresh(), gts, labs, is_sample=True)
            keep = [rows_in(s_rois[i], rois[i]) for i in range(G["N"])]
            n_fg = [int((s_lab[i] > 0).sum()) for i in range(G["N"])]
            pool = M.ROIPool(list(G["out"]), list(H.SCALES), H.ENLARGE, rotated, "pooling", G["max_res"], False)
            pooled = torch.cat(pool(feats, s_rois.clone()))
            rec[pre + "seeds"] = np.array([seed, map_seed], dtype=np.int32)
            rec[pre + "input_sums"] = H.input_sums(rois32, gts32, maps32)
            rec[pre + "eval_labels"] = torch.cat(e_lab).numpy().astype(np.int64)
            rec[pre + "eval_gt_rois"] = torch.cat(e_gt).numpy()
            rec[pre + "keep"] = np.array(keep, dtype=np.int64)
            rec[pre + "n_fg"] = np.array(n_fg, dtype=np.int64)
            rec[pre + "sample_labels"] = s_lab.numpy().astype(np.int64)
            rec[pre + "sample_gt_rois"] = s_gt.numpy()
            rec[pre + "pooled"] = pooled.numpy()
            if not rotated:
                remap = M.ROIPool(list(G["out"]), list(H.SCALES), H.ENLARGE, rotated, "pooling", G["max_res"], True)
                rec[pre + "pooled_remap"] = torch.cat(remap(feats, s_rois.clone(), [])).numpy()
                scales = [1 / s for s in H.SCALES]
                rec[pre + "remap_levels"] = M._setup_scales(scales, G["max_res"], len(scales))(s_rois.reshape(-1, s_rois.shape[-1])[:, 1:]).numpy().astype(np.int64)
            head = M.RCNN(G["C"], None, 2, list(G["out"]), is_add_layer=False, is_rotated_bbox=rotated, is_flatten=True).double()
            hp = H.gold_head(rotated)
            with torch.no_grad():
                head.RCNN_bbox_pred.weight.copy_(hp["RCNN_bbox_pred_w"]); head.RCNN_bbox_pred.bias.copy_(hp["RCNN_bbox_pred_b"])
                head.RCNN_cls_score.weight.copy_(hp["RCNN_cls_score_w"]); head.RCNN_cls_score.bias.copy_(hp["RCNN_cls_score_b"])
            model = M.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=rotated)
            seen = {}
            enc = model.box_coder.encode_single

            def spy(gt_rois, ex_rois, enc=enc, seen=seen):
                seen["ex"], seen["targets"] = ex_rois.clone(), enc(gt_rois, ex_rois)
                return seen["targets"]
            model.box_coder.encode_single = spy
            np.random.seed(NP_SEED)
            (proposals, m_lab), probs, loss = model(fresh(), gts, labs, feats, is_sample=True, is_reg=True)
            assert torch.equal(m_lab, s_lab)
            rec[pre + "encoded_rois"] = seen["ex"].detach().numpy()
            rec[pre + "targets"] = seen["targets"].detach().numpy()
            rec[pre + "losses"] = np.array([loss["loss_objectness"].item(), loss["loss_rpn_box_reg"].item()], dtype=np.float64)
            rec[pre + "proposals"] = torch.cat(proposals).detach().numpy()
            rec[pre + "cls_prob"] = torch.cat(probs).detach().numpy()
            print(pre, facts, f2, "keep", keep, "n_fg", n_fg, "losses", rec[pre + "losses"])
    finally:
        torch.Tensor.cuda, torch.Tensor.get_device, torch.float = saved[:3]
        torch.set_default_dtype(saved[3])
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
