"""Times the voxel-semantics evaluation (nerf_mae_amd.sem_eval over csrc/heads.hip) on the GPU, all in one process, and prints one JSON document.
    python tools/bench_sem_eval.py [--reps 20] [--warmup 5] [--res 160] [--classes 19] [--batches 1 2 4] [--out FILE]

Workload: logits (B,K,res^3) fp32 and fp32 label grids with about 40 % unlabelled voxels (seeded), class weights given.  Timed with device events on one stream,
median over the repetitions after the warm-up calls, microseconds per call:
    fused         ops.sem_eval: the evaluation pass and its one-workgroup finalize (loss scalars, counts, both int64 label volumes), outputs allocated inside
    masked_ce     ops.masked_ce_fwd alone, the training loss's forward: the same loss scalars and nothing else
    stock         the reference's output_metrics expression composed from stock torch ops on the device (softmax, argmax, masked cross entropy with weights,
                  one-hot soft IoU, boolean selection, three histc calls on the labels cast to float)
Achieved GB/s is the byte model over the time: fused reads 4K + 4 and writes 16 bytes per voxel, masked_ce reads 4K + 4.  The stock expression has no byte model
(it makes about ten passes with temporaries); its time is given as it is.  The three agree on their results before anything is timed.  Nothing is gated; the
numbers are figures of whatever machine this runs on."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_mae_amd import ops  # noqa: E402


def timed(fn, reps, warmup):
    out = []
    for k in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if k >= warmup:
            out.append(e0.elapsed_time(e1) * 1e3)
    return dict(median_us=statistics.median(out), min_us=min(out), max_us=max(out), reps=reps)


def stock(logits, labels, cw):
    """output_metrics' arithmetic in stock torch ops: -> (ce, iou_val, intersection, union, target, pred_vis, target_vis)"""
    B, K = logits.shape[:2]
    pred = logits.reshape(B, K, -1).permute(0, 2, 1)                         # (B,V,K)
    target = labels.reshape(B, -1).long()
    mask = (target > 0).long()
    prob = F.softmax(pred, dim=-1)
    arg = torch.argmax(prob, dim=-1)
    pred_vis, target_vis = arg * mask, target * mask
    ce = F.cross_entropy((pred * mask[..., None]).reshape(-1, K), target_vis.reshape(-1), weight=cw)
    pm = prob * mask[..., None].float()
    onehot = torch.zeros_like(pm).scatter_(-1, target_vis[..., None], 1.0)
    inter = (pm[..., 1:] * onehot[..., 1:]).sum(1)
    union = (pm[..., 1:] + onehot[..., 1:] - pm[..., 1:] * onehot[..., 1:]).sum(1)
    iou_val = (inter / (union + 1e-8)).mean()
    keep = mask.reshape(-1) == 1
    p, t = arg.reshape(-1)[keep].float(), target.reshape(-1)[keep].float()
    hi, hp, ht = (torch.histc(x, bins=K - 1, min=1, max=K - 1) for x in (p[p == t], p, t))
    return ce, iou_val, hi, hp + ht - hi, ht, pred_vis, target_vis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--res", type=int, default=160)
    ap.add_argument("--classes", type=int, default=19)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--out")
    args = ap.parse_args()
    K, R = args.classes, args.res
    V = R ** 3
    res = dict(device=torch.cuda.get_device_name(0), resolution=R, classes=K, reps=args.reps, warmup=args.warmup, rows=[])
    for B in args.batches:
        g = torch.Generator(device="cuda").manual_seed(B)
        logits = torch.randn((B, K, R, R, R), generator=g, device="cuda") * 2.0
        labels = torch.randint(1, K, (B, R, R, R), generator=g, device="cuda").float()
        labels[torch.rand(labels.shape, generator=g, device="cuda") < 0.4] = 0.0
        cw = torch.cat([torch.tensor([0.05]), 0.5 + torch.rand(K - 1)]).cuda()
        lab2 = labels.view(B, V)
        sums = torch.empty(2, dtype=torch.float64, device="cuda")
        iou = torch.empty((B, K - 1, 3), dtype=torch.float64, device="cuda")
        out2 = torch.empty(2, device="cuda")
        # agreement first: counts and volumes exactly (random fp32 logits: no two equal, no two probabilities rounded together is checked by the comparison itself)
        out, counts, pv, tv = ops.sem_eval(logits, lab2, cw)
        ops.masked_ce_fwd(logits, labels, cw, sums, iou, out2)
        s = stock(logits, labels, cw)
        torch.cuda.synchronize()
        agree = dict(counts=bool(torch.equal(counts[0], s[2].long()) and torch.equal(counts[1], s[3].long()) and torch.equal(counts[2], s[4].long())),
                     volumes=bool(torch.equal(pv, s[5]) and torch.equal(tv, s[6])),
                     ce_vs_masked_ce=abs(out[0].item() - out2[0].item()) / abs(out2[0].item()), iou_vs_masked_ce=abs(out[1].item() - out2[1].item()) / abs(out2[1].item()),
                     ce_vs_stock=abs(out[0].item() - s[0].item()) / abs(s[0].item()), iou_vs_stock=abs(out[1].item() - s[1].item()) / abs(s[1].item()))
        del s
        t_f = timed(lambda: ops.sem_eval(logits, lab2, cw), args.reps, args.warmup)
        t_m = timed(lambda: ops.masked_ce_fwd(logits, labels, cw, sums, iou, out2), args.reps, args.warmup)
        t_s = timed(lambda: stock(logits, labels, cw), max(args.reps // 4, 3), 2)
        bytes_f, bytes_m = B * V * (4 * K + 4 + 16), B * V * (4 * K + 4)
        t_f["gb_per_s"], t_m["gb_per_s"] = bytes_f / t_f["median_us"] * 1e-3, bytes_m / t_m["median_us"] * 1e-3
        res["rows"].append(dict(B=B, voxels=B * V, bytes_fused=bytes_f, bytes_masked_ce=bytes_m, fused=t_f, masked_ce=t_m, stock=t_s, agree=agree))
        del logits, labels, lab2, pv, tv
        torch.cuda.empty_cache()
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
