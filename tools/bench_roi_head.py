"""RoI stage at the launcher's shape: 2 scenes, 256 channels, the FPN's levels of a 160^3 grid (40^3, 20^3, 10^3, 5^3; 4, 8, 16, 32 mesh units per voxel),
output 5^3, 2000 proposals and 32 boxes per scene, 256 sampled RoIs per scene, axis-aligned and oriented.
    python tools/bench_roi_head.py [reps]

Timed with HIP events, median and minimum (the interpolation rows: and maximum) of `reps` >= 10 calls after 3 warm-up calls:
  targets      detector.roi_targets_dense: matching + sampling + gather (no host synchronisation)
  pool fwd     detector.ROIPool forward;  pool bwd: its backward to the four maps (the zeroing of the gradients included)
  loss fwd+bwd detector.roi_head_loss and the gradients to both head outputs
Next to each, a plain-torch composition of the same semantics (detector.py's header), written here from the semantics: the IoU matrix with torch.nonzero
sampling per scene; a Python loop over the RoIs with a crop (or an 8-corner gather), F.pad and max_pool3d each, reading the sizes back from the device;
cross_entropy and smooth_l1_loss over gathered rows, with autograd for the backward.  The composition's pooled features are compared with the kernel's.
The oriented run adds the "interpolation" feature type on the same maps and RoIs: interp fwd, interp bwd and interp fwd+bwd next to the pooling rows of the
same run and to a composition that loops over the RoIs with F.interpolate(trilinear, align_corners=True), as the reference does; median [min .. max]."""
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from nerf_mae_amd import detector

MESH, DIMS, SCALES, C, OUT = 160, (40, 20, 10, 5), (4, 8, 16, 32), 256, (5, 5, 5)
SCENES, CAP, NBOX, R, WANT_FG, FG, BG, ENLARGE = 2, 2000, 32, 256, 128, 0.5, 0.2, 0.2


def timed(fn, reps, warm=3):
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
    return statistics.median(us), min(us), max(us)


def make_inputs(rotated, seed=5):
    rng = np.random.default_rng(seed)

    def boxes(n, near=None):
        size = rng.uniform(10, 48, (n, 3))
        ctr = 30 + rng.uniform(0, 1, (n, 3)) * (MESH - 60)
        if near is not None:
            pick = rng.integers(0, near.shape[0], n // 2)
            ctr[:n // 2], size[:n // 2] = near[pick, :3] + rng.uniform(-3, 3, (n // 2, 3)), near[pick, 3:6] * rng.uniform(0.8, 1.2, (n // 2, 3))
        return np.concatenate([ctr, size, rng.uniform(-1.5, 1.5, (n, 1))], 1)
    gts, props = [], []
    for _ in range(SCENES):
        g = boxes(NBOX)
        gts.append(g)
        props.append(boxes(CAP, g))
    conv = (lambda b: b) if rotated else (lambda b: np.concatenate([b[:, :3] - b[:, 3:6] / 2, b[:, :3] + b[:, 3:6] / 2], 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.float32)).cuda()
    gt = [t(conv(g)) for g in gts]
    dense = t(np.stack([conv(p) for p in props]))
    levels = torch.from_numpy(rng.integers(0, 4, (SCENES, CAP)).astype(np.int32)).cuda()
    maps = [t(rng.standard_normal((SCENES, C, d, d, d))) for d in DIMS]
    return dense, levels, torch.full((SCENES,), CAP, dtype=torch.int32).cuda(), gt, [torch.ones(NBOX).cuda() for _ in gt], maps


def iou_matrix(a, b):
    whd = (torch.min(a[:, None, 3:], b[:, 3:]) - torch.max(a[:, None, :3], b[:, :3])).clamp(min=0)
    inter = whd.prod(2)
    return inter / ((a[:, 3:] - a[:, :3]).prod(1)[:, None] + (b[:, 3:] - b[:, :3]).prod(1) - inter)


def comp_targets(dense, levels, gt):
    """axis-aligned only: the oriented IoU has no plain-torch form short of the polygon clipping the reference compiles"""
    out = []
    for i in range(SCENES):
        best, arg = iou_matrix(dense[i], gt[i]).max(1)
        fg, bg = torch.nonzero(best >= FG).view(-1), torch.nonzero(best < BG).view(-1)
        nf = min(WANT_FG, fg.numel())
        keep = torch.cat([fg[torch.randperm(fg.numel(), device=fg.device)[:nf]], bg[(torch.rand(R - nf, device=bg.device) * bg.numel()).long()]])
        out.append((torch.cat([levels[i, keep, None].float(), dense[i, keep]], 1), gt[i][arg[keep]]))
    return out


def comp_pool(maps, rois, rotated, interp=False):
    """per-RoI loop, sizes read back from the device; interp (oriented): F.interpolate on the RoI's grid in place of the padded max-pool, as the reference does"""
    feats = []
    N, Rr = rois.shape[:2]
    host = rois.cpu()
    for b in range(N):
        for r in range(Rr):
            lvl, box = int(host[b, r, 0]), host[b, r, 1:].double()
            f, sc = maps[lvl][b], SCALES[lvl]
            W = f.shape[1]
            if not rotated:
                half, mid = (box[3:] - box[:3]) / 2 * (1 + ENLARGE), (box[3:] + box[:3]) / 2
                p0 = torch.floor((-0.5 * half + mid).float() / sc).long().clamp(min=0)
                p1 = (torch.floor((0.5 * half + mid).float() / sc).long() + 1).clamp(max=W)
                crop = f[:, p0[0]:p1[0], p0[1]:p1[1], p0[2]:p1[2]]
            else:
                g = torch.ceil(box[3:6].float() * (1 + ENLARGE) / sc).long().clamp(min=1)
                ix, iy, iz = torch.meshgrid(*[torch.arange(int(v), device=f.device, dtype=torch.float32) for v in g], indexing="ij")
                px, py, pz = ix - (g[0] - 1) / 2, iy - (g[1] - 1) / 2, iz - (g[2] - 1) / 2
                cs, sn = math.cos(float(box[6])), math.sin(float(box[6]))
                X, Y, Z = cs * px - sn * py + float(box[0]) / sc, sn * px + cs * py + float(box[1]) / sc, pz + float(box[2]) / sc
                mask = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= W - 1) & (Z >= 0) & (Z <= W - 1)
                crop = 0.
                for fa in (torch.floor, torch.ceil):
                    for fb in (torch.floor, torch.ceil):
                        for fc in (torch.floor, torch.ceil):
                            a, bb, c = fa(X), fb(Y), fc(Z)
                            v = f[:, a.clamp(0, W - 1).long(), bb.clamp(0, W - 1).long(), c.clamp(0, W - 1).long()]
                            crop = crop + v * (1 - (X - a).abs() * (Y - bb).abs() * (Z - c).abs())
                crop = crop * mask / 8
            if interp:
                feats.append(F.interpolate(crop[None], size=OUT, mode="trilinear", align_corners=True)[0])
                continue
            s = crop.shape[1:]
            if min(s) == 0:
                feats.append(torch.zeros((C, *OUT), device=f.device))
                continue
            k = [-(-v // o) for v, o in zip(s, OUT)]
            crop = F.pad(crop, (0, k[2] * OUT[2] - s[2], 0, k[1] * OUT[1] - s[1], 0, k[0] * OUT[0] - s[0]))
            feats.append(F.max_pool3d(crop[None], k, k)[0])
    return torch.stack(feats)


def comp_loss(scores, deltas, labels, targets):
    obj = F.cross_entropy(scores, labels.long())
    pos = torch.nonzero(labels > 0).view(-1)
    reg = F.smooth_l1_loss(deltas[pos], targets[pos], beta=1 / 9, reduction="sum") / max(pos.numel(), 1)
    torch.autograd.grad(obj + reg, (scores, deltas))


def interp_rows(maps, leaves, rois, dout, pool_t, pool_c, reps):
    """feature_extracting_type="interpolation" on the same maps and RoIs, next to the pooling rows of this run and to the per-RoI F.interpolate composition"""
    interp = detector.ROIPool(OUT, SCALES, ENLARGE, True, "interpolation")
    feat = interp(leaves, rois)
    with torch.no_grad():
        ref = comp_pool([m.detach() for m in maps], rois, True, interp=True)
    err = ((ref - feat.detach()).abs().max() / ref.abs().max()).item()
    t = {"interp fwd": timed(lambda: interp(maps, rois), reps), "interp bwd": timed(lambda: torch.autograd.grad(feat, leaves, dout, retain_graph=True), reps),
         "interp fwd+bwd": timed(lambda: torch.autograd.grad(interp(leaves, rois), leaves, dout), reps)}
    c = {"interp fwd": timed(lambda: comp_pool([m.detach() for m in maps], rois, True, interp=True), 3, warm=1),
         "interp fwd+bwd": timed(lambda: torch.autograd.grad(comp_pool(leaves, rois, True, interp=True), leaves, dout), 3, warm=1)}
    row = lambda d: " | ".join(f"{k} median {v[0]:10.1f} us [{v[1]:.1f} .. {v[2]:.1f}]" for k, v in d.items())          # noqa: E731
    print(f"  oriented interpolation: composition's features differ by {err:.2e} of the largest")
    print("  oriented interpolation kernels:     " + row(t))
    print("  oriented interpolation composition: " + row(c))
    print("  oriented pooling, same run:         " + row({k: pool_t[k] for k in ("pool fwd", "pool bwd")}) + " | composition " + row({k: pool_c[k] for k in ("pool fwd", "pool fwd+bwd")}))


def main(reps=10):
    assert torch.cuda.is_available(), "bench_roi_head.py needs an MI355X"
    reps = max(10, reps)
    print(f"RoI stage: {SCENES} scenes x {CAP} proposals x {NBOX} boxes, {R} RoIs per scene, C = {C}, maps {DIMS}, output {OUT}; {reps} reps")
    for rotated in (False, True):
        name = "oriented" if rotated else "axis-aligned"
        dense, levels, counts, gt, gl, maps = make_inputs(rotated)
        state = torch.tensor([1, 0], dtype=torch.int64).cuda()
        tg = lambda: detector.roi_targets_dense(dense, levels, counts, gt, gl, R, WANT_FG, FG, BG, state, True)
        labels, rois, gt_rois, _, c2 = tg()
        pool = detector.ROIPool(OUT, SCALES, ENLARGE, rotated)
        leaves = [m.requires_grad_(True) for m in maps]
        pooled = pool(leaves, rois)
        dout = torch.randn_like(pooled)
        B = 7 if rotated else 6
        scores, deltas = torch.randn((SCENES * R, 2), device="cuda", requires_grad=True), (0.3 * torch.randn((SCENES * R, B), device="cuda")).requires_grad_(True)

        def loss():
            out = detector.roi_head_loss(scores, deltas, labels.reshape(-1), rois.reshape(SCENES * R, -1), gt_rois.reshape(SCENES * R, -1))
            torch.autograd.grad(out["loss_objectness"] + out["loss_rpn_box_reg"], (scores, deltas))
        t = {"targets": timed(tg, reps), "pool fwd": timed(lambda: pool(maps, rois), reps),
             "pool bwd": timed(lambda: torch.autograd.grad(pooled, leaves, dout, retain_graph=True), reps), "loss fwd+bwd": timed(loss, reps)}
        with torch.no_grad():
            ref = comp_pool([m.detach() for m in maps], rois, rotated)
        err = ((ref - pooled.detach()).abs().max() / ref.abs().max()).item()
        _, targets = detector.roi_head_loss(scores, deltas, labels.reshape(-1), rois.reshape(SCENES * R, -1), gt_rois.reshape(SCENES * R, -1), return_targets=True)
        lab = labels.reshape(-1).clamp(min=0)
        c = {"pool fwd": timed(lambda: comp_pool([m.detach() for m in maps], rois, rotated), 3, warm=1),
             "pool fwd+bwd": timed(lambda: torch.autograd.grad(comp_pool(leaves, rois, rotated), leaves, dout), 3, warm=1),
             "loss fwd+bwd": timed(lambda: comp_loss(scores, deltas, lab, targets), reps)}
        if not rotated:
            c["targets"] = timed(lambda: comp_targets(dense, levels, gt), reps)
        print(f"  {name}: sampled (fg, bg) {c2.tolist()}; composition's pooled features differ by {err:.2e} of the largest")
        print(f"  {name} kernels:     " + " | ".join(f"{k} median {m:10.1f} us  min {b:10.1f} us" for k, (m, b, _) in t.items()))
        print(f"  {name} composition: " + " | ".join(f"{k} median {m:10.1f} us  min {b:10.1f} us" for k, (m, b, _) in c.items()))
        if rotated:
            interp_rows(maps, leaves, rois, dout, t, c, reps)


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 10)
