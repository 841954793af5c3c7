"""Records tests/golden/g17_obb_iou.npz from the reference's own oriented-box IoU Python, run on the CPU.
    python tools/gen_golden_obb_iou.py --reference PATH_TO_REFERENCE_CHECKOUT

The reference's functions (nerf_rpn/model/rotated_iou/oriented_iou_loss.py cal_iou_3d / cal_giou_3d / cal_diou_3d) are plain torch except
for sort_v, a compiled CUDA extension.  They are imported from the reference tree with stand-ins placed in sys.modules for the compiled
`sort_vertices` module and for `cuda_op.cuda_ext`, whose sort_v becomes tests/_rotated_ref.sort_vertices_ref (an index sort: it carries no
gradient in the reference either).

Recorded: 512 pairs from np.random.default_rng(17) (tests/_obb_iou_ref.make_boxes), the two box arrays, iou, giou_loss and diou_loss
("smallest"), and the gradients of each of the three sums with respect to both box arrays.  fp32 data only.

Precision.  The boxes are fp32; the reference's functions are evaluated on them in float64 and the results are stored as fp32, so that the
fixture carries the reference's function and not the rounding noise of its fp32 run.  (Run in fp32, the reference differs from its own
float64 run by up to 3e-5 of the gradient's maximum: on these 512 pairs ONE of the 3584 entries of the GIoU gradient with respect to box 2,
pair 362's theta, -0.0625855 in fp32 against -0.0625562 in float64, then exceeds the elementwise part of assert_close(rtol=1e-4) by 1.13x,
whatever it is compared with.  smallest_bounding_box casts its result to fp32 in either run.)"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests._obb_iou_ref import make_boxes  # noqa: E402
from tests._rotated_ref import sort_vertices_ref  # noqa: E402

NPAIRS, SEED = 512, 17
OUT = os.path.join(ROOT, "tests", "golden", "g17_obb_iou.npz")


def load_reference(ref):
    def sort_v(vertices, mask, num_valid):
        idx = sort_vertices_ref(vertices.detach().double().numpy(), mask.numpy(), num_valid.numpy())
        return torch.from_numpy(idx)

    sys.modules["sort_vertices"] = types.ModuleType("sort_vertices")
    pkg = types.ModuleType("rotated_iou.cuda_op")
    pkg.__path__ = []
    ext = types.ModuleType("rotated_iou.cuda_op.cuda_ext")
    ext.sort_v = sort_v
    sys.modules["rotated_iou.cuda_op"] = pkg
    sys.modules["rotated_iou.cuda_op.cuda_ext"] = ext
    sys.path.insert(0, os.path.join(ref, "nerf_rpn", "model"))
    from rotated_iou import oriented_iou_loss
    return oriented_iou_loss


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    L = load_reference(args.reference)
    rng = np.random.default_rng(SEED)
    b1, b2 = make_boxes(rng, NPAIRS), make_boxes(rng, NPAIRS)
    rec = dict(box1=b1, box2=b2)
    for name, fn in (("iou", lambda p, q: L.cal_iou_3d(p, q)), ("giou_loss", lambda p, q: L.cal_giou_3d(p, q)[0]), ("diou_loss", lambda p, q: L.cal_diou_3d(p, q)[0])):
        p = torch.from_numpy(b1)[None].double().requires_grad_(True)
        q = torch.from_numpy(b2)[None].double().requires_grad_(True)
        v = fn(p, q)
        v.sum().backward()
        rec[name] = v.detach()[0].numpy().astype(np.float32)
        rec[f"grad_{name}_box1"] = p.grad[0].numpy().astype(np.float32)
        rec[f"grad_{name}_box2"] = q.grad[0].numpy().astype(np.float32)
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{v.shape}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
