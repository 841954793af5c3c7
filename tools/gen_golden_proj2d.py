"""Records tests/golden/g30_proj2d.npz from the reference's own 2-D projection loss, run on the CPU: get_w2cs, project and obb2points_3d
(nerf_rpn/model/rpn.py:58-102, model/coder/misc.py, identical in model/fcos/utils.py), FCOSLossComputation.compute_2d_projection_loss (model/fcos/loss.py:447-475)
and the third return of RegionProposalNetwork.compute_loss (model/rpn.py:421-456).
    python tools/gen_golden_proj2d.py --reference PATH_TO_REFERENCE_CHECKOUT

The reference is loaded as tools/gen_golden_rpn_iou.py and tools/gen_golden_fcos.py do: `model`, `model.fcos` and `model.rotated_iou` are entered as bare namespace
stubs so that their __init__ files (which pull in the whole detector) do not run, and the compiled `sort_vertices` module, `cuda_op.cuda_ext.sort_v` and
torchvision.ops get stand-ins (none of them is called here).

Recorded (fp32 unless stated; the inputs are regenerated from seeds by tests/_proj2d_ref.py, tests/_rpn_ref.py, tests/_rpn_iou_ref.py and tests/_fcos_ref.py):
  w2c_32, w2c_160                      get_w2cs(res), [4, 4, 4];
  per (ncols, res, n) of the planted rows   pts: obb2points_3d of the 7-column predictions (float64), uv: project of the prediction's points under every camera
                                       (float64 inputs), t32 / g32: the row terms and their gradients as the reference runs them (fp32), t64 / g64: the same with
                                       float64 inputs (Tensor.float patched to Tensor.double for that run, the cameras being the reference's fp32 ones);
  fcos_2d_f32, fcos_2d_f64             compute_2d_projection_loss(box_regression, reg_targets, centerness_targets) on the positives of the oriented g18 geometry as the
                                       reference runs it, and the same sum from its decode_fcos_obb, obb2points_3d and project with float64 inputs;
  rpn_{aabb,obb,iou}_2d                compute_loss(...)[2] for the g20 geometry (both box kinds) and the g29 geometry with their recorded flags, fp32.
The script prints how far the reference's fp32 evaluation of the near rows lies from its float64 one: the GPU test's bound is four times that."""
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
from tests import _proj2d_ref as J  # noqa: E402
from tests import _rpn_iou_ref as Q  # noqa: E402
from tests import _rpn_post_ref as P  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g30_proj2d.npz")
ROW_CASES = [(ncols, res, n) for ncols in (6, 7) for res in (32, 160) for n in (J.N_ROWS, 1)]
RADIUS, NORM = 1.5, True              # the g18 configuration (tools/gen_golden_fcos.py)


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
    stub("sort_vertices")
    if "torchvision" not in sys.modules:
        stub("torchvision", path="")
        stub("torchvision.ops", sigmoid_focal_loss=None)
    stub("model", path=model)
    stub("model.fcos", path=os.path.join(model, "fcos"))
    stub("model.rotated_iou", path=os.path.join(model, "rotated_iou"))
    stub("model.rotated_iou.cuda_op", path="")
    stub("model.rotated_iou.cuda_op.cuda_ext", sort_v=None)
    return importlib.import_module("model.rpn"), importlib.import_module("model.fcos.loss"), importlib.import_module("model.fcos.utils")


class as_float64:
    """inside: Tensor.float() keeps float64 (project casts its points with .float())"""

    def __enter__(self):
        self.saved = torch.Tensor.float
        torch.Tensor.float = lambda t, *a, **k: t.double()

    def __exit__(self, *exc):
        torch.Tensor.float = self.saved


def row_terms(M, U, pred, target, res, dtype):
    """the reference's own steps on rows: points, project under every camera, smooth-L1 without reduction -> (T [n], dT/dpred [n, ncols], points, uv)"""
    Kmat = torch.tensor(J.K, dtype=dtype)
    poses = [w.to(dtype) for w in M.get_w2cs(res=res)]
    p = pred.to(dtype).clone().requires_grad_(True)
    t = target.to(dtype)

    def pts(b):
        q = torch.cat([b[:, :3], b[:, 3:]], 0) if b.shape[1] == 6 else U.obb2points_3d(b)
        return torch.cat([q, torch.ones(q.shape[0], 1, dtype=dtype)], 1)

    pp, tt = pts(p), pts(t)
    up = torch.cat([M.project(Kmat, w, pp) for w in poses], 0)
    ut = torch.cat([M.project(Kmat, w, tt) for w in poses], 0)
    loss = torch.nn.functional.smooth_l1_loss(up, ut, beta=1 / 9, reduction="none")          # [4 * 2 * n, 2]
    T = loss.reshape(4, 2, pred.shape[0], 2).sum((0, 1, 3))
    T.sum().backward()
    return T.detach(), p.grad, pp.detach()[:, :3], up.detach()


def rpn_third_return(M, rotated, boxes, a, flags, obj, reg):
    """compute_loss(...)[2] of the reference in fp32, the sampler replaced by the recorded flags, the decoded proposals from the reference's own coders"""
    C = 8 if rotated else 6
    N, n = flags.shape
    o, r = R.flatten_heads(obj, reg, C)
    anc = P.anchors_t(dtype=torch.float32).repeat(N, 1)
    flat = r.reshape(N * n, C).float()
    if rotated:
        coder = importlib.import_module("model.coder.midpoint_offset_coder")
        pred_bbox = coder.delta_sp2bbox(anc, flat)
    else:
        pred_bbox = importlib.import_module("model.coder.AABB_coder").AABBCoder().decode_single(flat, anc)
    matched = [boxes[b][a["matched"][b].clamp(min=0)] for b in range(N)]
    this = types.SimpleNamespace(fg_bg_sampler=lambda labels: ([flags[b] == 1 for b in range(N)], [flags[b] == 2 for b in range(N)]), reg_loss_type="smooth_l1")
    out = M.RegionProposalNetwork.compute_loss(this, o.reshape(-1, 1).float(), flat, [a["labels"][b].float() for b in range(N)],
                                               [a["targets"][b].float() for b in range(N)], pred_bbox.reshape(N * n, -1), matched, max(R.MESH))
    return np.float32(out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    args = ap.parse_args()
    M, L, U = load_reference(args.reference)
    rec = dict(row_seed=np.int32(J.ROW_SEED), n_rows=np.int32(J.N_ROWS))
    for res in (32, 160):
        rec[f"w2c_{res}"] = torch.stack(M.get_w2cs(res=res)).numpy()
        assert np.array_equal(rec[f"w2c_{res}"], torch.stack(U.get_w2cs(res=res)).numpy())
    for ncols, res, n in ROW_CASES:
        pred, target, where = J.make_rows(ncols, res, n)
        tag = f"r{ncols}_{res}_{n}"
        t32, g32, _, _ = row_terms(M, U, pred, target, res, torch.float32)
        with as_float64():
            t64, g64, pts, uv = row_terms(M, U, pred, target, res, torch.float64)
        rec.update({f"{tag}_t32": t32.numpy(), f"{tag}_g32": g32.numpy(), f"{tag}_t64": t64.numpy(), f"{tag}_g64": g64.numpy(), f"{tag}_uv": uv.numpy()})
        if ncols == 7:
            rec[f"{tag}_pts"] = pts.numpy()
        if where["near"]:
            k = where["near"]
            print(f"{tag} near rows: max |fp32 - float64| terms {float((t32[k].double() - t64[k]).abs().max()):.3e} (terms up to {float(t64[k].max()):.3e}), "
                  f"gradients {float((g32[k].double() - g64[k]).abs().max()):.3e} (up to {float(g64[k].abs().max()):.3e})")
    # FCOS: the positives of the g18 geometry, oriented
    boxes = F.make_scene(F.SEED[True], True)
    asg = F.assign(boxes, RADIUS, NORM, orig=F.ORIG)
    reg = F.make_heads(F.HEAD_SEED, True, NORM)[1]
    r = F.flatten_heads(reg, reg, reg)[1]
    pos = asg["valid"] & (asg["labels"] > 0)
    rec["fcos_2d_f32"] = np.float32(L.FCOSLossComputation.compute_2d_projection_loss(types.SimpleNamespace(), r[pos].float(), asg["targets"][pos].float(), asg["ctr"][pos].float()))
    zero = torch.zeros((int(pos.sum()), 3), dtype=torch.float64)
    with as_float64():
        T = row_terms(M, U, U.decode_fcos_obb(zero, r[pos].double()), U.decode_fcos_obb(zero, asg["targets"][pos]), J.FCOS_RES, torch.float64)[0]
    rec["fcos_2d_f64"] = np.float64((T * asg["ctr"][pos]).sum() / J.FCOS_RES / 16)
    rec["fcos_csum"], rec["fcos_npos"] = np.float64(asg["csum"]), np.int32(asg["npos"])
    # RPN: the g20 geometry with its recorded flags, both box kinds, and the g29 geometry
    g20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz"))
    for rotated, name in ((False, "aabb"), (True, "obb")):
        boxes = R.make_scene(R.SEED[rotated], rotated=rotated, ori=R.ORI)
        a = R.assign(boxes, ori=R.ORI, rotated=rotated)
        obj, regs = R.make_heads(R.HEAD_SEED, len(R.NBOX), 8 if rotated else 6)
        rec[f"rpn_{name}_2d"] = rpn_third_return(M, rotated, boxes, a, torch.from_numpy(g20[("o_" if rotated else "a_") + "flags"]), obj, regs)
    case = Q.make_case()
    rec["rpn_iou_2d"] = rpn_third_return(M, True, case["boxes"], case["assign"], case["flags"], case["obj"], case["reg"])
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, " + ", ".join(f"{k}{np.shape(v)}" for k, v in rec.items() if np.ndim(v) == 0 or k.startswith("w2c")))
    print({k: float(v) for k, v in rec.items() if np.ndim(v) == 0})


if __name__ == "__main__":
    main()
