"""Records tests/golden/g32_box_head.npz from the reference's own box head (model.detector.RCNN, detector.py:441-496), run on the CPU in float64.
    python tools/gen_golden_box_head.py --reference PATH_TO_REFERENCE_CHECKOUT

The reference's imports get the stand-ins of tools/gen_golden_fcos.py (load_reference), and model.feature_extractor (the backbones, which the head does not use)
an empty one; the default dtype is float64 for the run and the module is converted with .double().

Recorded for all eight combinations of is_add_layer x is_flatten x is_rotated_bbox at input_size (3, 3, 3) and (2, 3, 1), C = 16, M = 5 RoIs, n_classes = 2
(tests/_box_head_ref.golden_case: input, parameters and the cotangent pair are filled by formula): both outputs and, for sum(output * cotangent), the gradient
of the input and of every parameter (of a 3x3x3 weight every 16th element, of a flattening Linear weight every 4th: _box_head_ref.recorded_view).  Inputs are
NOT stored: the file carries their float64 sums."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _box_head_ref as B  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g32_box_head.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    from tools.gen_golden_fcos import load_reference
    load_reference(args.reference)
    sys.modules["model.feature_extractor"] = types.ModuleType("model.feature_extractor")     # the backbones: detector.py imports them but the head uses none
    saved = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    rec = dict(geometry=np.array([B.G_C, B.G_M, B.G_NCLS], dtype=np.int32))
    try:
        M = importlib.import_module("model.detector")
        for size in B.G_SIZES:
            for add_layer, flatten, rotated in B.G_CONFIGS:
                pre = B.golden_prefix(size, add_layer, flatten, rotated)
                x, P, cot_box, cot_cls = B.golden_case(size, add_layer, flatten, rotated)
                head = M.RCNN(B.G_C, None, B.G_NCLS, list(size), is_add_layer=add_layer, is_rotated_bbox=rotated, is_flatten=flatten).double()
                assert list(head.state_dict()) == B.keys(add_layer), list(head.state_dict())
                head.load_state_dict(P, strict=True)
                xin = x.clone().requires_grad_(True)
                box, cls = head(xin)
                ((box * cot_box).sum() + (cls * cot_cls).sum()).backward()
                rec[pre + "input_sums"] = B.input_sums(x, P, cot_box, cot_cls)
                rec[pre + "box"], rec[pre + "cls"], rec[pre + "dx"] = B.as_np(box), B.as_np(cls), B.as_np(xin.grad)
                for k, p in head.named_parameters():
                    rec[pre + "d_" + k] = B.as_np(B.recorded_view(k, p.grad, flatten))
                print(pre, tuple(box.shape), tuple(cls.shape), f"|box| {box.abs().max().item():.3f} |cls| {cls.abs().max().item():.3f} |dx| {xin.grad.abs().max().item():.3f}")
    finally:
        torch.set_default_dtype(saved)
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
