"""Records tests/golden/g29_rpn_iou_loss.npz from the reference's own delta_sp2bbox (nerf_rpn/model/coder/midpoint_offset_coder.py) and RotatedIOULoss
(nerf_rpn/model/rpn.py) over its oriented IoU Python (model/rotated_iou/), run on the CPU.
    python tools/gen_golden_rpn_iou.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_rpn_iou.py --search          (no reference needed: prints the first scene seeds that meet tests/_rpn_iou_ref.check_case)

The reference is loaded as tools/gen_golden_rpn.py and tools/gen_golden_fcos.py do: `model` and `model.rotated_iou` are entered as bare namespace stubs so
that their __init__ files (which pull in the whole detector) do not run, and the compiled `sort_vertices` module with `cuda_op.cuda_ext.sort_v` gets the
stand-in tests/_rotated_ref.sort_vertices_ref.

Rows: the flagged positives of tests/_rpn_iou_ref.make_case() (the g20 geometry with more boxes, both scenes, the planted rows included).  Recorded as
fp32: the dense anchor index of every row, its deltas [P, 8], anchor [P, 6] and matched box [P, 7], the reference's decoded proposals [P, 7], and for each
of the four loss types the summed loss and its gradient over the deltas [P, 8] from the reference's autograd.  Evaluated in float64 on the fp32 inputs.
The script also prints how far the reference's fp32 evaluation lies from its float64 one (the condition of the GPU tests' tolerance)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _rpn_iou_ref as Q  # noqa: E402
from tests._rotated_ref import sort_vertices_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g29_rpn_iou_loss.npz")


def load_reference(ref):
    def sort_v(vertices, mask, num_valid):
        return torch.from_numpy(sort_vertices_ref(vertices.detach().double().numpy(), mask.numpy(), num_valid.numpy()))

    def stub(name, path=None, **attrs):
        m = types.ModuleType(name)
        if path is not None:
            m.__path__ = [path]
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    model = os.path.join(ref, "nerf_rpn", "model")
    stub("sort_vertices")
    stub("model", path=model)
    stub("model.rotated_iou", path=os.path.join(model, "rotated_iou"))
    stub("model.rotated_iou.cuda_op", path="")
    stub("model.rotated_iou.cuda_op.cuda_ext", sort_v=sort_v)
    return importlib.import_module("model.rpn"), importlib.import_module("model.coder.midpoint_offset_coder")


def search(limit):
    for seed in range(limit):
        try:
            case = Q.make_case(seed)
            Q.check_case(case)
        except AssertionError as e:
            print(f"seed {seed}: {e}")
            continue
        print(f"seed {seed} ok: flagged positives per scene {(case['flags'] == 1).sum(1).tolist()}")
        break


def evaluate(M, C, deltas, anchors, boxes, loss_type, dtype):
    d = deltas.detach().clone().to(dtype).requires_grad_(True)
    proposals = C.delta_sp2bbox(anchors.to(dtype), d)
    loss = M.RotatedIOULoss(loss_type)(proposals, boxes.to(dtype))
    loss.backward()
    return proposals.detach(), loss.detach(), d.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=200, help="print the first scene seed that meets every condition of the case generator")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    M, C = load_reference(args.reference)
    case = Q.make_case()
    br = Q.check_case(case)
    deltas, anchors, boxes = Q.rows_of(case)
    rec = dict(seed=np.int32(Q.SEED), nbox=np.array(Q.NBOX, dtype=np.int32), flag_seed=np.int32(Q.FLAG_SEED), index=case["index"].numpy().astype(np.int32),
               deltas=deltas.numpy(), anchors=anchors.numpy(), boxes=boxes.numpy(), planted=np.array([case["planted"][k] for k in Q.PLANTED], dtype=np.int32))
    for t in Q.TYPES:
        prop, loss, grad = evaluate(M, C, deltas, anchors, boxes, t, torch.float64)
        p32, l32, g32 = evaluate(M, C, deltas, anchors, boxes, t, torch.float32)
        rec["proposals"] = prop.numpy().astype(np.float32)
        rec[t + "_loss"] = np.float32(loss)
        rec[t + "_grad"] = grad.numpy().astype(np.float32)
        print(f"{t}: loss {float(loss):.9g}; fp32 against float64: loss {abs(float(l32) - float(loss)) / abs(float(loss)):.2e} relative, gradient "
              f"{float((g32.double() - grad).abs().max() / grad.abs().max()):.2e} of the max norm ({float(grad.abs().max()):.3g})")
        worst = int((g32.double() - grad).abs().amax(1).argmax())
        print(f"    the row furthest off: {worst} (dense index {int(case['index'][worst])}), |gradient| {float(grad[worst].abs().max()):.3g}, deltas {deltas[worst].tolist()}")
    assert all(np.isfinite(v).all() for v in rec.values())
    print("rows", deltas.shape[0], "branches", {k: int(br[k].sum()) for k in Q.REQUIRED})
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
