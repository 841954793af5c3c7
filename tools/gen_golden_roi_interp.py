"""Records tests/golden/g31_roi_interp.npz from the reference's own RoI stage (model.detector) with feature_extracting_type="interpolation", run on the CPU.
    python tools/gen_golden_roi_interp.py --reference PATH_TO_REFERENCE_CHECKOUT

The pattern of tools/gen_golden_roi_head.py: the reference's imports get the stand-ins of tools/gen_golden_fcos.py (load_reference) and an empty
model.feature_extractor; for the duration of the run Tensor.cuda is the identity, Tensor.get_device returns the tensor's device, the default dtype is float64 and
the name torch.float, with which detector.py casts its grids and its rotation, is bound to float64, so that the reference evaluates in float64 on inputs that hold
fp32 values.

One oriented run over tests/_roi_head_ref.gold_inputs(True) (mesh 32^3, maps 16^3 / 8^3 / 4^3 of 4 channels, two scenes of 8 RoIs and 3 boxes), with the sampler
under the np.random seed that tests/golden/g22_roi_head.npz records, so that the kept rows are the recorded ones (asserted):
ROIPool(feature_extracting_type="interpolation") on the sampled RoIs, and Classification_Model(is_sample=True, is_reg=True) on a flattening RCNN with the parameters
of _roi_head_ref.gold_head(True): the pooled features, the two losses, the decoded proposals, the class probabilities, the regression targets and the RoIs it
encoded against (captured at box_coder.encode_single).  The reference's enlarge_roi writes into its argument, so every call gets clones.  Inputs are NOT stored:
the file carries their float64 sums.

Condition on the inputs, asserted here from the restatement (tests/_roi_interp_ref.py), never from code under test: the "floor" margin of the sampled RoIs' grids is
at least MARGIN = 1e-3."""
import argparse
import contextlib
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _roi_head_ref as H  # noqa: E402
from tests import _roi_interp_ref as I  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g31_roi_interp.npz")
G22 = os.path.join(ROOT, "tests", "golden", "g22_roi_head.npz")
G = H.GOLD


@contextlib.contextmanager
def float64_reference():
    saved = (torch.Tensor.cuda, torch.Tensor.get_device, torch.float, torch.get_default_dtype())
    torch.Tensor.cuda = lambda self, *a, **k: self
    torch.Tensor.get_device = lambda self: self.device
    torch.float = torch.float64
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.Tensor.cuda, torch.Tensor.get_device, torch.float = saved[:3]
        torch.set_default_dtype(saved[3])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from tools.gen_golden_fcos import load_reference
    from tools.gen_golden_roi_head import rows_in
    load_reference(args.reference)
    sys.modules["model.feature_extractor"] = types.ModuleType("model.feature_extractor")     # the backbones: detector.py imports them but the RoI stage uses none
    g22 = np.load(G22)
    np_seed, keep22, n_fg22 = int(g22["np_seed"]), g22["o_keep"], g22["o_n_fg"]
    rois32, gts32, labs32, maps32 = H.gold_inputs(True)
    kept = torch.stack([r[torch.as_tensor(k)] for r, k in zip(rois32, keep22)])
    _, facts, _ = I.interp(maps32, kept, out=G["out"])
    assert facts["floor"] >= H.MARGIN, facts
    rec = dict(np_seed=np.int32(np_seed), out=np.array(G["out"], dtype=np.int32), seeds=np.array(H.GOLD_SEED[True], dtype=np.int32),
               input_sums=H.input_sums(rois32, gts32, maps32), keep=keep22.astype(np.int64), n_fg=n_fg22.astype(np.int64), floor_margin=np.float64(facts["floor"]))
    with float64_reference():
        M = importlib.import_module("model.detector")
        rois, gts, labs = [r.double() for r in rois32], [g.double() for g in gts32], [l.double() for l in labs32]
        feats = [[m[i].double() for m in maps32] for i in range(G["N"])]
        fresh = lambda: [r.clone() for r in rois]          # noqa: E731
        layer = M.ProposalTargetLayer(2, batch_size=G["N"] * G["R"], fg_fraction=0.5, fg_threshold=H.FG, bg_threshold=H.BG, is_rotated_bbox=True)
        np.random.seed(np_seed)
        s_lab, s_rois, _ = layer(fresh(), gts, labs, is_sample=True)
        assert np.array_equal(np.array([rows_in(s_rois[i], rois[i]) for i in range(G["N"])]), keep22), "the sampler repeats the recorded kept rows"
        pool = M.ROIPool(list(G["out"]), list(H.SCALES), H.ENLARGE, True, "interpolation", G["max_res"], False)
        rec["pooled"] = torch.cat(pool(feats, s_rois.clone())).numpy()
        head = M.RCNN(G["C"], None, 2, list(G["out"]), is_add_layer=False, is_rotated_bbox=True, is_flatten=True).double()
        hp = H.gold_head(True)
        with torch.no_grad():
            head.RCNN_bbox_pred.weight.copy_(hp["RCNN_bbox_pred_w"]); head.RCNN_bbox_pred.bias.copy_(hp["RCNN_bbox_pred_b"])
            head.RCNN_cls_score.weight.copy_(hp["RCNN_cls_score_w"]); head.RCNN_cls_score.bias.copy_(hp["RCNN_cls_score_b"])
        model = M.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=True)
        seen = {}
        enc = model.box_coder.encode_single

        def spy(gt_rois, ex_rois):
            seen["ex"], seen["targets"] = ex_rois.clone(), enc(gt_rois, ex_rois)
            return seen["targets"]
        model.box_coder.encode_single = spy
        np.random.seed(np_seed)
        (proposals, m_lab), probs, loss = model(fresh(), gts, labs, feats, is_sample=True, is_reg=True)
        assert torch.equal(m_lab, s_lab)
        rec["sample_labels"] = s_lab.numpy().astype(np.int64)
        rec["encoded_rois"] = seen["ex"].detach().numpy()
        rec["targets"] = seen["targets"].detach().numpy()
        rec["losses"] = np.array([loss["loss_objectness"].item(), loss["loss_rpn_box_reg"].item()], dtype=np.float64)
        rec["proposals"] = torch.cat(proposals).detach().numpy()
        rec["cls_prob"] = torch.cat(probs).detach().numpy()
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()), "losses", rec["losses"], "floor", facts["floor"])


if __name__ == "__main__":
    main()
