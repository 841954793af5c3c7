"""RPN training path at the downstream shape: 2 scenes x 950 625 anchors (levels 40^3, 20^3, 10^3, 5^3 on a 160^3 mesh, run_rpn.py's 13 anchors
per location) x 32 boxes per scene, fg 0.35, bg 0.2, 256 samples per scene, axis-aligned and oriented.
    python tools/bench_rpn.py [reps]

Timed with HIP events, median and minimum of `reps` >= 20 calls after 5 warm-up calls, each line in two runs of the loop:
  fused        nerf_mae_amd.rpn.RPNLossComputation: assignment + sampling + loss forward + backward, eager (no host synchronisation)
  graph        the same replayed from a captured graph
  composition  the steps of the semantics (csrc/rpn.hip) from framework ops, as the reference composes them: head tensors permuted and concatenated,
               the box x anchor IoU matrix in slices of 16 boxes, two maxima, the equality scan for the restore, boolean-mask writes, the encode, randperm
               sampling, gathered losses, autograd backward.  Written here from the semantics; it lives in this tool, not in the product.
The composition and the fused op are also compared: the same labels, and, for the fused op's sampled set, losses that agree to 1e-4.

    python tools/bench_rpn.py iou [reps]      (these rows alone; without "iou" they follow the lines above)
The IoU-type box losses of the oriented RPN, loss forward + backward alone on a given sampled set: each of iou, linear_iou, giou, diou through the fused
kernels, the smooth-L1 path on the same inputs, and a composition of each IoU type from framework ops (nonzero of the flags, gather, the decode in
autograd, nerf_mae_amd.rotated_iou.cal_*_3d, backward), whose losses must agree with the fused ones to 1e-4."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from nerf_mae_amd import rpn

MESH, GRIDS, SCENES, NBOX = (160,) * 3, ((40,) * 3, (20,) * 3, (10,) * 3, (5,) * 3), 2, 32
SIZES = ((8,), (16,), (32,), (64,))
RATIOS = (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * 4
FG, BG, BATCH, FRACTION = 0.35, 0.2, 256, 0.5


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(us), min(us)


def make_inputs(rotated, seed=5):
    rng = np.random.default_rng(seed)
    C, boxes = (8 if rotated else 6), []
    for _ in range(SCENES):
        size = rng.uniform(8, 48, (NBOX, 3))
        ctr = size / 2 + rng.uniform(0, 1, (NBOX, 3)) * (MESH[0] - size)
        b = np.concatenate([ctr, size, rng.uniform(-1.5, 1.5, (NBOX, 1))], 1) if rotated else np.concatenate([ctr - size / 2, ctr + size / 2], 1)
        boxes.append(torch.from_numpy(b.astype(np.float32)).cuda())
    obj = [torch.from_numpy(rng.standard_normal((SCENES, 13, *g)).astype(np.float32)).cuda() for g in GRIDS]
    reg = [torch.from_numpy((0.5 * rng.standard_normal((SCENES, 13 * C, *g))).astype(np.float32)).cuda() for g in GRIDS]
    return boxes, obj, reg


def to_aabb(b):
    cs, sn = torch.cos(b[:, 6]), torch.sin(b[:, 6])
    bx, by = (b[:, 3] / 2 * cs).abs() + (b[:, 4] / 2 * sn).abs(), (b[:, 3] / 2 * sn).abs() + (b[:, 4] / 2 * cs).abs()
    return torch.stack([b[:, 0] - bx, b[:, 1] - by, b[:, 2] - b[:, 5] / 2, b[:, 0] + bx, b[:, 1] + by, b[:, 2] + b[:, 5] / 2], 1)


def encode(g, a, rotated):
    e = a[:, 3:] - a[:, :3]
    if not rotated:
        s = g[:, 3:] - g[:, :3]
        return torch.cat([((g[:, :3] + 0.5 * s) - (a[:, :3] + 0.5 * e)) / e, torch.log(s / e)], 1)
    p, h = (a[:, :3] + a[:, 3:]) * 0.5, to_aabb(g)
    gx, gy, gw, gh = (h[:, 0] + h[:, 3]) * 0.5, (h[:, 1] + h[:, 4]) * 0.5, h[:, 3] - h[:, 0], h[:, 4] - h[:, 1]
    cs, sn, w, l = torch.cos(g[:, 6]), torch.sin(g[:, 6]), g[:, 3], g[:, 4]
    v1x, v1y, v2x, v2y = w / 2 * cs, -w / 2 * sn, -l / 2 * sn, -l / 2 * cs
    X = torch.stack([g[:, 0] + v1x + v2x, g[:, 0] + v1x - v2x, g[:, 0] - v1x - v2x, g[:, 0] - v1x + v2x], 1)
    Y = torch.stack([g[:, 1] + v1y + v2y, g[:, 1] + v1y - v2y, g[:, 1] - v1y - v2y, g[:, 1] - v1y + v2y], 1)
    ga = torch.where((Y - Y.min(1, keepdim=True).values).abs() > 0.1, torch.full_like(X, -1000.0), X).max(1).values
    gb = torch.where((X - X.max(1, keepdim=True).values).abs() > 0.1, torch.full_like(Y, -1000.0), Y).max(1).values
    return torch.stack([(gx - p[:, 0]) / e[:, 0], (gy - p[:, 1]) / e[:, 1], (g[:, 2] - p[:, 2]) / e[:, 2], torch.log(gw / e[:, 0]), torch.log(gh / e[:, 1]),
                        torch.log(g[:, 5] / e[:, 2]), (ga - gx) / gw, (gb - gy) / gh], 1)


def composition(anchors, boxes, obj, reg, rotated, flags=None):
    """the semantics of csrc/rpn.hip, step by step, from framework ops -> (labels [N, n], loss_objectness, loss_rpn_box_reg); backward included"""
    N, C = len(boxes), 8 if rotated else 6
    o = torch.cat([t.permute(0, 2, 3, 4, 1).reshape(N, -1) for t in obj], 1).reshape(-1)
    r = torch.cat([t.view(N, -1, C, *t.shape[2:]).permute(0, 3, 4, 5, 1, 2).reshape(N, -1, C) for t in reg], 1).reshape(-1, C)
    va = (anchors[:, 3:] - anchors[:, :3]).prod(1)
    labels, targets = [], []
    for g in boxes:
        hb = to_aabb(g) if rotated else g
        rows = []
        for i in range(0, hb.shape[0], 16):
            s = hb[i:i + 16]
            whd = (torch.min(s[:, None, 3:], anchors[:, 3:]) - torch.max(s[:, None, :3], anchors[:, :3])).clamp(min=0)
            inter = whd[..., 0] * whd[..., 1] * whd[..., 2]
            rows.append(inter / ((s[:, 3:] - s[:, :3]).prod(1)[:, None] + va - inter))
        q = torch.cat(rows, 0)
        vals, m = q.max(0)
        every = m.clone()
        m[vals < BG] = -1
        m[(vals >= BG) & (vals < FG)] = -2
        upd = torch.where(q == q.max(1).values[:, None])[1]
        m[upd] = every[upd]
        lab = (m >= 0).float()
        lab[m == -2] = -1.0
        labels.append(lab)
        targets.append(encode(g[m.clamp(min=0)], anchors, rotated))
    if flags is None:
        pos_idx, neg_idx = [], []
        for i, lab in enumerate(labels):
            pos, neg = torch.where(lab >= 1)[0], torch.where(lab == 0)[0]
            k = min(pos.numel(), int(BATCH * FRACTION))
            pos_idx.append(pos[torch.randperm(pos.numel(), device=pos.device)[:k]] + i * lab.numel())
            neg_idx.append(neg[torch.randperm(neg.numel(), device=neg.device)[:min(neg.numel(), BATCH - k)]] + i * lab.numel())
        pos_idx, neg_idx = torch.cat(pos_idx), torch.cat(neg_idx)
    else:
        pos_idx, neg_idx = torch.where(flags.reshape(-1) == 1)[0], torch.where(flags.reshape(-1) == 2)[0]
    sampled = torch.cat([pos_idx, neg_idx])
    lab_all, tg_all = torch.cat(labels), torch.cat(targets)
    loss_reg = F.smooth_l1_loss(r[pos_idx], tg_all[pos_idx], beta=1 / 9, reduction="sum") / sampled.numel()
    loss_obj = F.binary_cross_entropy_with_logits(o[sampled], lab_all[sampled])
    if o.requires_grad:
        torch.autograd.grad(loss_obj + loss_reg, list(obj) + list(reg))
    return torch.stack(labels), loss_obj.detach(), loss_reg.detach()


def main(reps=20):
    assert torch.cuda.is_available(), "bench_rpn.py needs an MI355X"
    reps = max(20, reps)
    gen = rpn.AnchorGenerator3D(SIZES, RATIOS)
    anchors = gen(torch.zeros((1, 1, *MESH)), [torch.zeros((1, 1, *g)) for g in GRIDS])[0][0].cuda()
    print(f"RPN training path: {SCENES} scenes x {anchors.shape[0]} anchors x {NBOX} boxes; {reps} reps, two runs per line")
    for rotated in (False, True):
        boxes, obj, reg = make_inputs(rotated)
        fn = rpn.RPNLossComputation(gen, FG, BG, BATCH, FRACTION, rotated_bbox=rotated)

        def fused(heads=None, sampled=None):
            o, r = heads or ([t.requires_grad_(True) for t in obj], [t.requires_grad_(True) for t in reg])
            out = fn(MESH, o, r, boxes, sampled=sampled)
            grads = torch.autograd.grad(out["loss_objectness"] + out["loss_rpn_box_reg"], list(o) + list(r))
            return out, grads

        labels, _, _ = rpn.rpn_assign_targets(gen, MESH, GRIDS, boxes, None, FG, BG, rotated=rotated)
        flags, counts = rpn.rpn_sample(labels, BATCH, FRACTION, torch.tensor([1, 0], dtype=torch.int64).cuda())
        out, _ = fused(sampled=flags)
        clab, cobj, creg = composition(anchors, boxes, [t.detach() for t in obj], [t.detach() for t in reg], rotated, flags)
        agree = (torch.equal(clab, labels), abs(cobj.item() - out["loss_objectness"].item()) <= 1e-4 * abs(cobj.item()),
                 abs(creg.item() - out["loss_rpn_box_reg"].item()) <= 1e-4 * abs(creg.item()))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            heads = ([t.detach().clone().requires_grad_(True) for t in obj], [t.detach().clone().requires_grad_(True) for t in reg])
            fused(heads)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            fused(heads)
        name = "oriented" if rotated else "axis-aligned"
        print(f"  {name}: positives {(labels == 1).sum(1).tolist()}, sampled {counts.tolist()}; composition: same labels {agree[0]}, losses agree to 1e-4: {agree[1:]}")
        for run in (1, 2):
            t = dict(fused=timed(fused, reps), graph=timed(graph.replay, reps),
                     composition=timed(lambda: composition(anchors, boxes, obj, reg, rotated), max(5, reps // 4), warm=1))
            print(f"  {name} run {run}: " + " | ".join(f"{k} median {m:9.1f} us  min {b:9.1f} us" for k, (m, b) in t.items()))


def decode_obb(d, anc):
    """MidpointOffsetCoder.decode_single from framework ops (the semantics of csrc/rpn_decode.hpp), differentiable: d [P, 8], anc [P, 6] -> [P, 7]"""
    clip, pi = abs(float(np.log(16 / 1000))), 3.141592
    p, e = (anc[:, :3] + anc[:, 3:]) * 0.5, anc[:, 3:] - anc[:, :3]
    g, c = e * torch.exp(d[:, 3:6].clamp(-clip, clip)), p + e * d[:, :3]
    gx, gy, gw, gh = c[:, 0], c[:, 1], g[:, 0], g[:, 1]
    da, db = d[:, 6].clamp(-0.5, 0.5), d[:, 7].clamp(-0.5, 0.5)
    X = torch.stack([da * gw, gw * 0.5, -da * gw, -gw * 0.5], 1)
    Y = torch.stack([-gh * 0.5, db * gh, gh * 0.5, -db * gh], 1)
    ln = torch.sqrt(X * X + Y * Y)
    s = ln.max(1, keepdim=True).values / ln
    X, Y = X * s + gx[:, None], Y * s + gy[:, None]
    th = torch.atan2(-(Y[:, 1] - Y[:, 0]), X[:, 1] - X[:, 0] + 1e-7)
    cs, sn = torch.cos(th), torch.sin(th)
    x, y = X.sum(1) / 4, Y.sum(1) / 4
    ux, uy = X - x[:, None], Y - y[:, None]
    rx, ry = ux * cs[:, None] - uy * sn[:, None], ux * sn[:, None] + uy * cs[:, None]
    w, h = rx.max(1).values - rx.min(1).values, ry.max(1).values - ry.min(1).values
    keep = w > h
    t = torch.where(keep, th, th + pi / 2) + pi / 2
    return torch.stack([x, y, c[:, 2], torch.where(keep, w, h), torch.where(keep, h, w), g[:, 2], torch.remainder(t, pi) - pi / 2], 1)


def iou_composition(anchors, boxes, offsets, midx, obj, reg, flags, loss_type):
    """the IoU-type box loss from framework ops and the project's paired-box op: nonzero of the flags (one wait for the host), gather, the decode in
    autograd, rotated_iou.cal_*_3d, the objectness loss, backward -> (loss_objectness, loss_rpn_box_reg)"""
    from nerf_mae_amd import rotated_iou
    N, n = flags.shape
    o = torch.cat([t.permute(0, 2, 3, 4, 1).reshape(N, -1) for t in obj], 1).reshape(-1)
    r = torch.cat([t.view(N, -1, 8, *t.shape[2:]).permute(0, 3, 4, 5, 1, 2).reshape(N, -1, 8) for t in reg], 1).reshape(-1, 8)
    f = flags.reshape(-1)
    pos, sampled = torch.nonzero(f == 1)[:, 0], torch.nonzero(f != 0)[:, 0]
    rows = offsets[pos // n] + midx.reshape(-1)[pos].clamp(min=0).long()
    A, B = decode_obb(r[pos], anchors[pos % n])[None], boxes[rows][None]
    if loss_type in ("iou", "linear_iou"):
        iou, _, _, _, u = rotated_iou.cal_iou_3d(A, B, verbose=True)
        q = (iou * u + 1.0) / (u + 1.0)
        terms = -torch.log(q) if loss_type == "iou" else 1.0 - q
    elif loss_type == "giou":
        terms = rotated_iou.cal_giou_3d(A, B)[0]
    else:
        terms = rotated_iou.cal_diou_3d(A, B)[0]
    loss_reg = terms.sum() / sampled.numel()
    loss_obj = F.binary_cross_entropy_with_logits(o[sampled], (f[sampled] == 1).float())
    torch.autograd.grad(loss_obj + loss_reg, list(obj) + list(reg))
    return loss_obj.detach(), loss_reg.detach()


def iou_rows(reps):
    """the loss forward + backward alone (assignment and sampling are done once, outside the timed region) on the oriented inputs: the four IoU types, the
    smooth-L1 path on the same inputs, and the framework composition of each IoU type"""
    from nerf_mae_amd import ops
    gen = rpn.AnchorGenerator3D(SIZES, RATIOS)
    anchors = gen(torch.zeros((1, 1, *MESH)), [torch.zeros((1, 1, *g)) for g in GRIDS])[0][0].cuda()
    boxes, obj, reg = make_inputs(True)
    plan = rpn._plan(gen, MESH, GRIDS, SCENES, "bench_rpn")
    bx, offsets = rpn._boxes("bench_rpn", boxes, 7)
    labels, midx, targets = ops.rpn_assign(plan, bx, offsets, 7, None, FG, BG)
    flags, counts = rpn.rpn_sample(labels, BATCH, FRACTION, torch.tensor([1, 0], dtype=torch.int64).cuda())
    heads = [t.requires_grad_(True) for t in obj] + [t.requires_grad_(True) for t in reg]
    offs_dev = torch.tensor(offsets[:-1], dtype=torch.int64).cuda()

    def fused(loss_type):
        out = rpn._RpnLoss.apply(plan, 8, None if loss_type == "smooth_l1" else loss_type, None, None, flags, targets, bx, offsets, None, midx, *heads)
        torch.autograd.grad(out[0] + out[1], heads)
        return out

    print(f"IoU-type box losses, forward + backward on given flags: {SCENES} scenes x {anchors.shape[0]} anchors, sampled {counts.tolist()}; {reps} reps, two runs per line")
    for t in ("smooth_l1",) + tuple(ops.FCOS_LOSS_TYPES):
        line = {}
        if t != "smooth_l1":
            got, want = fused(t), iou_composition(anchors, bx, offs_dev, midx, obj, reg, flags, t)
            line["agree to 1e-4"] = all(abs(a.item() - b.item()) <= 1e-4 * abs(b.item()) for a, b in zip(got, want))
        for run in (1, 2):
            res = {"fused": timed(lambda: fused(t), reps)}
            if t != "smooth_l1":
                res["composition"] = timed(lambda: iou_composition(anchors, bx, offs_dev, midx, obj, reg, flags, t), max(5, reps // 4), warm=1)
            print(f"  {t:10s} run {run}: " + " | ".join(f"{k} median {m:9.1f} us  min {b:9.1f} us" for k, (m, b) in res.items()) + (f" | {line}" if line and run == 1 else ""))


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "iou":
        iou_rows(max(20, int(sys.argv[2]) if len(sys.argv) > 2 else 20))
    else:
        main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
        iou_rows(max(20, int(sys.argv[1]) if len(sys.argv) > 1 else 20))
