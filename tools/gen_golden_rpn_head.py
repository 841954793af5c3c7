"""Records tests/golden/g23_rpn_head.npz from the reference's own RPNHead (nerf_rpn/model/anchor.py:177-213), run on the CPU in float64.
    python tools/gen_golden_rpn_head.py --reference PATH_TO_REFERENCE_CHECKOUT

The reference is imported the way tools/gen_golden_rpn.py does it: `model` and `model.rotated_iou` as bare namespace stubs, the compiled oriented IoU as a
stand-in that no code path used here calls.

Recorded, for the geometry of tests/_rpn_head_ref.py (Cin 16, A 2, N 2, levels (3,2,2) and (2,1,2)): conv_depth 0, 1 and 2 with rotate False (prefix dKa_)
and True (dKr_).  Inputs x0, x1 (fp32, with exact zeros and negatives); the 3x3x3 weights conv.0 / conv.2 (fp16-exact, shared by all cases) and biases; the
1x1x1 parameters per box type (a_ / r_); per case a fixed random cotangent (fp16-exact), the head's outputs, and the gradients of sum(output * cotangent)
with respect to the inputs and every parameter, float64 (of a 3x3x3 weight's gradient every 32nd element: all of them would exceed the size that a
fixture should have).  Also the ordered state_dict keys and shapes of NeRFRegionProposalNetwork(...).rpn: with an explicit RPNHead(16, 13, 2, rotate=True)
(rpn_keys / rpn_shapes) and with the default constructor, rotated_bbox False and True (rpn0_ / rpn1_: the flag lands in conv_depth)."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _rpn_head_ref as H  # noqa: E402
from tools.gen_golden_rpn import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g23_rpn_head.npz")


def state_table(module):
    sd = module.state_dict()
    shapes = np.zeros((len(sd), 5), dtype=np.int32)
    for i, v in enumerate(sd.values()):
        shapes[i, :v.dim()] = list(v.shape)
    return np.array(list(sd.keys())), shapes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    load_reference(args.reference)
    import importlib
    A_ = importlib.import_module("model.anchor")
    NR = importlib.import_module("model.nerf_rpn")
    Cin, A, N, L = H.G_CIN, H.G_A, H.G_N, len(H.G_GRIDS)
    feats = [f.float().double() for f in H.make_features(H.G_SEED, N, Cin, H.G_GRIDS)]
    rec = {f"x{i}": H.as_np(f).astype(np.float32) for i, f in enumerate(feats)}
    shared = H.make_params(H.G_SEED + 1, 2, Cin, A, 6)
    for k in ("conv.0.weight", "conv.2.weight"):
        rec[k] = H.as_np(shared[k]).astype(np.float16)
    for k in ("conv.0.bias", "conv.2.bias"):
        rec[k] = H.as_np(shared[k]).astype(np.float32)
    for rotate in (False, True):
        small = H.make_params(H.G_SEED + 2 + rotate, 0, Cin, A, 8 if rotate else 6)
        for k, v in small.items():
            rec[f"{'r' if rotate else 'a'}_{k}"] = H.as_np(v).astype(np.float32)
    g = torch.Generator().manual_seed(H.G_SEED + 9)
    for depth, rotate in H.G_CASES:
        pre = f"d{depth}{'r' if rotate else 'a'}_"
        C = 8 if rotate else 6
        P = H.golden_params(rec, depth, rotate)
        ref = A_.RPNHead(Cin, A, depth, rotate).double()
        ref.load_state_dict(P, strict=True)
        xs = [f.clone().requires_grad_(True) for f in feats]
        obj, reg = ref(xs)
        cot_obj = [torch.randn(o.shape, generator=g).half().double() for o in obj]
        cot_reg = [torch.randn(r.shape, generator=g).half().double() for r in reg]
        (sum((o * c).sum() for o, c in zip(obj, cot_obj)) + sum((r * c).sum() for r, c in zip(reg, cot_reg))).backward()
        assert [tuple(o.shape) for o in obj] == [(N, A, *gr) for gr in H.G_GRIDS] and [tuple(r.shape) for r in reg] == [(N, A * C, *gr) for gr in H.G_GRIDS]
        for i in range(L):
            rec[f"{pre}cot_obj{i}"], rec[f"{pre}cot_reg{i}"] = H.as_np(cot_obj[i]).astype(np.float16), H.as_np(cot_reg[i]).astype(np.float16)
            rec[f"{pre}obj{i}"], rec[f"{pre}reg{i}"], rec[f"{pre}dx{i}"] = H.as_np(obj[i]), H.as_np(reg[i]), H.as_np(xs[i].grad)
        grads = dict(ref.named_parameters())
        for k in H.keys(depth):
            rec[f"{pre}d_{k}"] = H.as_np(H.recorded_view(k, grads[k].grad))
        print(pre, "outputs", [tuple(o.shape) for o in obj + reg], "max |dx|", max(float(x.grad.abs().max()) for x in xs))

    class Backbone(torch.nn.Module):
        out_channels = Cin

    gen = NR.AnchorGenerator3D(((8,), (16,), (32,), (64,)), (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * 4)
    rec["rpn_keys"], rec["rpn_shapes"] = state_table(NR.NeRFRegionProposalNetwork(Backbone(), gen, A_.RPNHead(Cin, 13, 2, rotate=True), rotated_bbox=True).rpn)
    for flag in (False, True):
        rec[f"rpn{int(flag)}_keys"], rec[f"rpn{int(flag)}_shapes"] = state_table(NR.NeRFRegionProposalNetwork(Backbone(), rotated_bbox=flag).rpn)
    assert all(np.isfinite(v).all() for v in rec.values() if v.dtype.kind == "f")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
