"""Records tests/golden/g18_fcos_loss.npz from the reference's own FCOS loss Python, run on the CPU.
    python tools/gen_golden_fcos.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_fcos.py --search          (no reference needed: prints scene seeds whose decision margins are all >= 1e-3)

The reference's nerf_rpn/model/fcos/loss.py (FCOSLossComputation) is plain torch except for three imports, which get stand-ins in sys.modules:
the compiled `sort_vertices` module and `cuda_op.cuda_ext.sort_v` (tests/_rotated_ref.sort_vertices_ref, as tools/gen_golden_obb_iou.py), and
`torchvision.ops.sigmoid_focal_loss`, written here from the public formula (p = sigmoid(x); ce = BCE-with-logits; p_t = p t + (1-p)(1-t);
loss = alpha_t ce (1 - p_t)^gamma, alpha 0.25, gamma 2).  The packages `model`, `model.fcos` and `model.rotated_iou` are entered as bare
namespace stubs so that their __init__ files (which pull in the whole detector) do not run.

Recorded, for the geometry of tests/_fcos_ref.py (strides 4/8/16/32, feature sizes (20,18,17) .. (3,3,3), scenes of 70 / 1 / 0 boxes, original
sizes (80,72,68), (61,72,50), (80,40,68)), center sampling 1.5, normalised targets, for use_obb False with "giou" (prefix a_) and True with
"iou" plus the additional L1 (prefix o_): the boxes and their per-scene offsets, `labels` and `reg_targets` of prepare_targets in the dense
layout, the three losses, and the gradients of their sum with respect to the three head outputs (dense layout, every level).  The head
outputs themselves are NOT stored (they alone would exceed the size limit for a committed file): they are tests/_fcos_ref.make_heads(HEAD_SEED,
...), a numpy PCG64 stream, and the file carries their float64 sums so that a drift of the generator is noticed.

Precision: fp32 inputs, the reference evaluated on them in float64, results stored as fp32 (DESIGN.md 3.8 gives the reason)."""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _fcos_ref as F  # noqa: E402
from tests._rotated_ref import sort_vertices_ref  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g18_fcos_loss.npz")
RADIUS, NORM = 1.5, True
CASES = (("a_", False, "giou", False), ("o_", True, "iou", True))


def sigmoid_focal_loss(inputs, targets, alpha=0.25, gamma=2, reduction="none"):
    p = torch.sigmoid(inputs)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * (1 - p_t) ** gamma
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean() if reduction == "mean" else (loss.sum() if reduction == "sum" else loss)


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
    stub("torchvision", path="")
    stub("torchvision.ops", sigmoid_focal_loss=sigmoid_focal_loss)
    stub("model", path=model)
    stub("model.fcos", path=os.path.join(model, "fcos"))
    stub("model.rotated_iou", path=os.path.join(model, "rotated_iou"))
    stub("model.rotated_iou.cuda_op", path="")
    stub("model.rotated_iou.cuda_op.cuda_ext", sort_v=sort_v)
    return importlib.import_module("model.fcos.loss")


def margins(seed, use_obb):
    boxes = F.make_scene(seed, use_obb)
    worst = {}
    for radius in (0.0, RADIUS):
        a = F.assign(boxes, radius, NORM, orig=F.ORIG)
        for k, v in F.decision_margins(a).items():
            worst[k] = min(worst.get(k, float("inf")), v)
        worst["npos"] = min(worst.get("npos", 1 << 30), a["npos"])
    return worst


def search(limit):
    for use_obb in (False, True):
        for seed in range(limit):
            m = margins(seed, use_obb)
            if all(v >= 1e-3 for k, v in m.items() if k != "npos"):
                print(f"use_obb={use_obb}: seed {seed}  " + "  ".join(f"{k} {v:.3g}" for k, v in m.items()))
                break
        else:
            print(f"use_obb={use_obb}: no seed below {limit}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=200, help="print the first scene seeds with every decision margin >= 1e-3")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    L = load_reference(args.reference)
    locs = F.locations()
    masks = F.valid_masks(F.ORIG)
    rec = dict(radius=np.float32(RADIUS), norm=np.int32(NORM), head_seed=np.int32(F.HEAD_SEED))
    for pre, use_obb, loss_type, add_l1 in CASES:
        boxes = F.make_scene(F.SEED[use_obb], use_obb)
        cls, reg, ctr = F.make_heads(F.HEAD_SEED, use_obb, NORM)
        heads = [[t.double().requires_grad_(True) for t in ts] for ts in (cls, reg, ctr)]
        fn = L.FCOSLossComputation(list(F.STRIDES), RADIUS, loss_type, NORM, 1, use_obb, add_l1)
        targets = [b.double() for b in boxes]
        labels, reg_targets = fn.prepare_targets(locs, targets)
        out = fn(locs, heads[0], heads[1], heads[2], targets, masks)
        sum(out).backward()
        C = 8 if use_obb else 6
        rec[pre + "boxes"] = torch.cat(boxes, 0).numpy()
        rec[pre + "offsets"] = np.cumsum([0] + [b.shape[0] for b in boxes]).astype(np.int32)
        rec[pre + "labels"] = torch.cat([t.reshape(-1) for t in labels]).numpy().astype(np.float32)
        rec[pre + "reg_targets"] = torch.cat([t.reshape(-1, C) for t in reg_targets]).numpy().astype(np.float32)
        rec[pre + "losses"] = np.array([float(v.detach()) for v in out], dtype=np.float32)
        rec[pre + "head_sums"] = np.array([sum(t.double().sum().item() for t in ts) for ts in (cls, reg, ctr)], dtype=np.float64)
        g = F.flatten_heads(*[[t.grad for t in ts] for ts in heads])
        for name, v in zip(("grad_cls", "grad_reg", "grad_ctr"), g):
            rec[pre + name] = v.numpy().astype(np.float32)
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items()))


if __name__ == "__main__":
    main()
