"""What the 2-D projection loss costs at the downstream shape of tools/bench_rpn.py: 2 scenes x 950 625 anchors (levels 40^3 .. 5^3 on a 160^3 mesh, 13 anchors
per location), 32 boxes and 256 sampled anchors per scene.
    python tools/bench_proj2d.py [reps]

Timed with HIP events, median and minimum of `reps` >= 20 calls after 5 warm-up calls:
  off / on      RPNLossComputation / RPNIoULossComputation(reg_loss_2d=False | True): assignment + sampling + loss forward + backward, eager, for
                (AABB, smooth_l1), (OBB, smooth_l1) and (OBB, giou); and the loss forward + backward alone on a fixed sampled set (the ops entries)
  composition   the 2-D loss of the AABB case from framework ops around nerf_mae_amd.proj2d.proj2d_terms: nonzero of the flags, gather of deltas, anchors and
                matched boxes, the decode in autograd, proj2d_terms, sum / P / res, backward; its value must agree with the fused one to 1e-4
The measured figures are in DESIGN.md 3.22."""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import bench_rpn as B
from nerf_mae_amd import ops, proj2d, rpn


def loss_fn(gen, rotated, loss_type, on):
    if loss_type == "smooth_l1":
        return rpn.RPNLossComputation(gen, B.FG, B.BG, B.BATCH, B.FRACTION, rotated_bbox=rotated, reg_loss_2d=on)
    return rpn.RPNIoULossComputation(gen, B.FG, B.BG, B.BATCH, B.FRACTION, reg_loss_type=loss_type, reg_loss_2d=on)


def main(reps=30):
    assert torch.cuda.is_available(), "bench_proj2d.py needs an MI355X"
    gen = rpn.AnchorGenerator3D(B.SIZES, B.RATIOS)
    res = float(max(B.MESH))
    for rotated, loss_type in ((False, "smooth_l1"), (True, "smooth_l1"), (True, "giou")):
        boxes, obj, reg = B.make_inputs(rotated)
        heads = [[t.clone().requires_grad_(True) for t in ts] for ts in (obj, reg)]
        flat = [t for ts in heads for t in ts]
        name = f"{'obb' if rotated else 'aabb'} {loss_type}"
        times = {}
        for on in (False, True):
            fn = loss_fn(gen, rotated, loss_type, on)

            def step():
                out = fn(B.MESH, heads[0], heads[1], boxes)
                torch.autograd.grad(out["loss_objectness"] + out["loss_rpn_box_reg"] + out["loss_rpn_box_reg_2d"] if on else out["loss_objectness"] + out["loss_rpn_box_reg"], flat)

            times[on] = B.timed(step, reps)
        print(f"{name:16s} whole call      off {times[False][0]:8.1f} us (min {times[False][1]:8.1f})   on {times[True][0]:8.1f} us (min {times[True][1]:8.1f})")
        # the loss kernels alone, on a fixed sampled set
        ncols, C = (7, 8) if rotated else (6, 6)
        plan = rpn._plan(gen, B.MESH, B.GRIDS, B.SCENES, "bench")
        bx, offs = rpn._boxes("bench", boxes, ncols)
        labels, midx, targets = ops.rpn_assign(plan, bx, offs, ncols, None, B.FG, B.BG)
        flags, _ = ops.rpn_sample(labels, B.BATCH, int(B.BATCH * B.FRACTION), torch.tensor([0, 0], dtype=torch.int64, device="cuda"))
        one = torch.ones(1, device="cuda")
        lt = None if loss_type == "smooth_l1" else loss_type
        cams = proj2d._cams(res)

        def off():
            s = ops.rpn_loss_fwd(plan, C, lt, obj, reg, flags, targets, bx, offs, None, midx)
            ops.rpn_loss_bwd(plan, C, lt, obj, reg, flags, targets, bx, offs, None, midx, None, None, s, one, one)

        def on_():
            s = ops.rpn_loss_fwd(plan, C, lt, obj, reg, flags, targets, bx, offs, None, midx, cams, res)
            ops.rpn_loss_bwd(plan, C, lt, obj, reg, flags, targets, bx, offs, None, midx, cams, res, s, one, one, one)

        t0, t1 = B.timed(off, reps), B.timed(on_, reps)
        print(f"{name:16s} loss fwd + bwd  off {t0[0]:8.1f} us (min {t0[1]:8.1f})   on {t1[0]:8.1f} us (min {t1[1]:8.1f})   positives {int((flags == 1).sum())}")
        if not rotated:
            fused = ops.rpn_loss_fwd(plan, C, lt, obj, reg, flags, targets, bx, offs, None, midx, cams, res)[3].item()
            anchors = torch.cat(gen(torch.zeros((1, 1, *B.MESH)), obj)[0][:1]).cuda()
            n = anchors.shape[0]

            def composition():
                r = torch.cat([t.view(B.SCENES, -1, 6, *t.shape[2:]).permute(0, 3, 4, 5, 1, 2).reshape(B.SCENES, -1, 6) for t in heads[1]], 1).reshape(-1, 6)
                idx = torch.nonzero(flags.reshape(-1) == 1)[:, 0]
                a, d = anchors[idx % n], r[idx]
                rows = torch.cat([boxes[b][midx[b].clamp(min=0)] for b in range(B.SCENES)])[idx]
                e = a[:, 3:] - a[:, :3]
                c = d[:, :3] * e + (a[:, :3] + 0.5 * e)
                h = 0.5 * torch.exp(d[:, 3:].clamp(max=math.log(2000.0))) * e
                loss = proj2d.proj2d_terms(torch.cat([c - h, c + h], 1), rows, res).sum() / idx.numel() / res
                torch.autograd.grad(loss, heads[1])
                return loss

            comp = composition().item()
            assert abs(comp - fused) <= 1e-4 * abs(fused), (comp, fused)
            tc = B.timed(composition, reps)
            print(f"{name:16s} composition of the 2-D loss alone {tc[0]:8.1f} us (min {tc[1]:8.1f}); value {comp:.6g} against the fused {fused:.6g}")


if __name__ == "__main__":
    main(max(int(sys.argv[1]), 20) if len(sys.argv) > 1 else 30)
