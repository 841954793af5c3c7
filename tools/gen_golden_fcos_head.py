"""Records tests/golden/g24_fcos_head.npz from the reference's own FCOSHead (nerf_rpn/model/fcos/fcos.py:26-139), run on the CPU in float64.
    python tools/gen_golden_fcos_head.py --reference PATH_TO_REFERENCE_CHECKOUT

The reference is imported with the stand-ins of tools/gen_golden_fcos.py (fcos.py imports the loss and the post-processing, which import the compiled helpers; no
code path used here calls them).

Recorded, for the geometry of tests/_fcos_head_ref.py (C 64: 2 channels per group, num_convs 1, N 2, levels (3,2,2) and (2,1,2), strides 4 and 8): the cases
G_CASES = (use_obb, centerness_on_reg, training), prefix {a|o}{r|c}{t|e}_.  Inputs x0, x1 (fp32, with exact zeros and negatives); the parameters, shared by all
cases except bbox_pred (a_ / o_: 6 or 8 rows): convolution weights as bf16 bits (uint16; they are drawn bf16-exact), biases, non-trivial GroupNorm affine
parameters and non-unit Scales (one negative) as fp32; per case a fixed random cotangent of each output (fp16-exact), the head's outputs, and the gradients of
sum(output * cotangent) with respect to the inputs and every parameter, float64 (of a tower weight's gradient every 64th element, of an output weight's every 8th:
all of them would exceed the size that a fixture should have)."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _fcos_head_ref as H  # noqa: E402
from tools.gen_golden_fcos import load_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g24_fcos_head.npz")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    load_reference(args.reference)
    M = importlib.import_module("model.fcos.fcos")
    C, N, L = H.G_C, H.G_N, len(H.G_GRIDS)
    feats = [f.float().double() for f in H.make_features(H.G_SEED, N, C, H.G_GRIDS)]
    rec = {f"x{i}": H.as_np(f).astype(np.float32) for i, f in enumerate(feats)}
    for use_obb in (False, True):
        P = H.make_params(H.G_SEED + 1 + use_obb, H.G_CONVS, C, 8 if use_obb else 6, scales=(*H.G_SCALES, 0.5, 1.5, 1.0))
        for k, v in P.items():
            if k.startswith("bbox_pred"):
                name = f"{'o' if use_obb else 'a'}_{k}"
            elif use_obb:
                continue            # shared parameters: recorded once, from the first draw
            else:
                name = k
            rec[name] = H.bf16_bits(v.float().bfloat16().float()) if v.dim() == 5 else H.as_np(v).astype(np.float32)
    g = torch.Generator().manual_seed(H.G_SEED + 9)
    for use_obb, ctr_on_reg, training in H.G_CASES:
        pre = H.case_prefix(use_obb, ctr_on_reg, training)
        P = H.golden_params(rec, use_obb)
        ref = M.FCOSHead(C, H.G_CONVS, list(H.G_STRIDES), norm_reg_targets=True, centerness_on_reg=ctr_on_reg, use_obb=use_obb).double()
        ref.load_state_dict(P, strict=True)
        ref.train(training)
        xs = [f.clone().requires_grad_(True) for f in feats]
        outs = ref(xs)
        cots = [[torch.randn(o.shape, generator=g).half().double() for o in os_] for os_ in outs]
        sum((o * c).sum() for os_, cs in zip(outs, cots) for o, c in zip(os_, cs)).backward()
        nreg = 8 if use_obb else 6
        assert [tuple(o.shape) for o in outs[1]] == [(N, nreg, *gr) for gr in H.G_GRIDS]
        for n, os_, cs in zip(("cls", "reg", "ctr"), outs, cots):
            for i in range(L):
                rec[f"{pre}cot_{n}{i}"], rec[f"{pre}{n}{i}"] = H.as_np(cs[i]).astype(np.float16), H.as_np(os_[i])
        for i in range(L):
            rec[f"{pre}dx{i}"] = H.as_np(xs[i].grad)
        grads = dict(ref.named_parameters())
        for k in H.keys(H.G_CONVS):
            if k.startswith("scales.") and int(k.split(".")[1]) >= L:
                assert grads[k].grad is None
                continue
            rec[f"{pre}d_{k}"] = H.as_np(H.recorded_view(k, grads[k].grad))
        assert any(float((o == 0).double().mean()) > 0.05 for o in outs[1]), "the column-wise ReLU must be active"
        print(pre, "outputs", [tuple(o.shape) for os_ in outs for o in os_], "max |dx|", max(float(x.grad.abs().max()) for x in xs))
    assert all(np.isfinite(v).all() for v in rec.values() if v.dtype.kind == "f")
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
