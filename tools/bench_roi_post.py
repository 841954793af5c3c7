"""Times the RoI post-processing and the two-stage detector's inference on one GPU.
    python tools/bench_roi_post.py [--rows 2000] [--scenes 2] [--calls 20] [--warmup 3]

Workload: N = 2 scenes of R = 2000 rows, both box forms; inputs are tests/_roi_post_ref.lattice_case (clusters of overlapping boxes, graded scores).
Timed, median and minimum of --calls calls after --warmup warm-ups, device time by events around each call:
  roi_postprocess_dense   select + sort + NMS (three launches and one torch.sort)
  detections_dense        TwoStageDetector.detections_dense from the FPN features on (the backbone's output is computed once and handed out): RPN head, proposals, pooling, box head, post-processing (axis-aligned common small model)
  torch composition       the same result as the reference structures it, in plain torch on the device: softmax, decode, clamp, nonzero, and a host loop over
                          box_iou_3d (nerf_mae_amd.rotated_iou) that waits for the host once per kept box; 3 calls after 1 when a call takes more than 2 s
Prints one JSON line."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _roi_post_ref as P  # noqa: E402

CLIP = math.log(2000.0)


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), calls=calls)


def decode(d, ex, rotated):
    dw = d[:, 3:6].clamp(max=CLIP)
    if rotated:
        cs, sn = torch.cos(ex[:, 6]), torch.sin(ex[:, 6])
        xyz = torch.stack([d[:, 0] * ex[:, 3] * cs - d[:, 1] * ex[:, 4] * sn + ex[:, 0], d[:, 0] * ex[:, 3] * sn + d[:, 1] * ex[:, 4] * cs + ex[:, 1], d[:, 2] * ex[:, 5] + ex[:, 2]], 1)
        a = torch.remainder(2 * math.pi * d[:, 6] + ex[:, 6], math.pi)
        return torch.cat([xyz, torch.exp(dw) * ex[:, 3:6], torch.where(a > math.pi / 2, a - math.pi, a)[:, None]], 1)
    s = ex[:, 3:] - ex[:, :3]
    c, h = d[:, :3] * s + (ex[:, :3] + 0.5 * s), 0.5 * torch.exp(dw) * s
    return torch.cat([c - h, c + h], 1)


def composition(logits, deltas, rois, counts, mesh, thr, nms, min_size, rotated, iou):
    """per scene: softmax, decode, clip, size and score filters, then the reference's NMS loop (one IoU row and one host wait per kept box)"""
    out = []
    for b, n in enumerate(counts):
        p = torch.softmax(logits[b, :n], 1)
        boxes = decode(deltas[b, :n], rois[b, :n, 1:], rotated)
        size = torch.tensor(mesh[b], dtype=torch.float32, device=boxes.device)
        if rotated:
            ok = ((boxes[:, :3] >= 0) & (boxes[:, :3] <= size)).all(1) & (boxes[:, 3:6] >= min_size).all(1)
        else:
            boxes = torch.minimum(boxes.clamp(min=0), size.repeat(2))
            ok = ((boxes[:, 3:] - boxes[:, :3]) >= min_size).all(1)
        keep = torch.nonzero(ok & (p.max(1).values >= thr)).reshape(-1)
        boxes, s = boxes[keep], p[keep, 1]
        idxs = s.argsort(descending=True)
        kept = []
        while idxs.numel() > 0:
            i = idxs[0]
            kept.append(i)
            if idxs.numel() == 1:
                break
            row = iou(boxes[i][None], boxes[idxs[1:]]).reshape(-1)
            idxs = idxs[1:][row <= nms]
        kept = torch.stack(kept) if kept else idxs
        out.append((boxes[kept], s[kept]))
    return out


class Recorded(torch.nn.Module):
    """a backbone that hands out features computed before"""

    def __init__(self, features):
        super().__init__()
        self.features = features

    def forward(self, x):
        return self.features


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--scenes", type=int, default=2)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    from nerf_mae_amd import detector as D
    from nerf_mae_amd.rotated_iou import box_iou_3d
    res = dict(bench="roi_post", scenes=args.scenes, rows=args.rows, device=torch.cuda.get_device_name(0))
    for rotated in (False, True):
        inp = P.lattice_case(0, rotated, args.rows, [args.rows] * args.scenes, 2, True, (88, 88, 88), special=False)
        cu = {k: v.cuda() for k, v in inp.items() if isinstance(v, torch.Tensor)}
        counts = torch.tensor(inp["counts"], dtype=torch.int32).cuda()
        mesh = torch.tensor(inp["mesh_sizes"], dtype=torch.int32).cuda()
        flat = lambda t: t.reshape(-1, t.shape[-1])
        fn = lambda: D.roi_postprocess_dense(flat(cu["pred_scores"]), flat(cu["pred_bbox_deltas"]), flat(cu["rois"]), counts, mesh, 0.5, 0.3, 1e-3, True, "any")
        key = "obb" if rotated else "aabb"
        res[key + "_dense"] = timed(fn, args.calls, args.warmup)
        kept = fn()[3].tolist()
        comp = lambda: composition(cu["pred_scores"], cu["pred_bbox_deltas"], cu["rois"], inp["counts"], inp["mesh_sizes"], 0.5, 0.3, 1e-3, rotated, box_iou_3d)
        t0 = time.perf_counter()
        got = comp()
        torch.cuda.synchronize()
        slow = time.perf_counter() - t0 > 2.0
        assert [len(s) for _, s in got] == kept, ([len(s) for _, s in got], kept)
        res[key + "_torch_composition"] = timed(comp, 3 if slow else args.calls, 1 if slow else args.warmup)
        res[key + "_kept"] = kept
    from tests._two_stage_ref import scenes, two_stage
    det = two_stage().eval()
    meshes, _ = scenes()
    with torch.no_grad():
        features = list(det.rpn_network.backbone(torch.stack(meshes)))
    det.rpn_network.backbone = Recorded(features)            # the timed call is TwoStageDetector.detections_dense itself, its backbone replaced by its output
    res["detections_dense_from_features"] = dict(timed(lambda: det.detections_dense(meshes), args.calls, args.warmup), rows=int(det.detections_dense(meshes)[1].shape[1]))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
