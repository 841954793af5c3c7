"""Times the detection evaluation (nerf_mae_amd.det_eval over csrc/det_eval.hip) on the GPU, all in one process, and prints one JSON document.
    python tools/bench_det_eval.py [--reps 20] [--warmup 3] [--scenes 100] [--out FILE]

Workload: batches of 8 scenes, 2500 proposals and 40 ground-truth boxes each (tests/_det_eval_ref.make_scenes), oriented and axis-aligned, limits (300, 1000,
2500), AP thresholds (0.25, 0.5, 0.75).  Timed with device events on one stream:
    iou / match / claims   each of the three per-batch launches (the library's per-call event brackets), median over the repetitions, microseconds per batch
    update                 DetectionEvaluator.update of one dense batch, launch to completion
    compute                DetectionEvaluator.compute() over --scenes accumulated scenes (concatenate, sort, the precision / recall scan, the one read-back)
    restatement            the float64 restatement of the same twelve metrics on the CPU (tests/_det_eval_ref.py), wall clock, once
Nothing is gated; the numbers are single-run figures of whatever machine this runs on."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_mae_amd import det_eval  # noqa: E402
from nerf_mae_amd._lib import lib  # noqa: E402
from tests import _det_eval_ref as E  # noqa: E402

BATCH, P, G = 8, 2500, 40
LIMITS, THRESHOLDS = (300, 1000, 2500), (0.25, 0.5, 0.75)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scenes", type=int, default=100, help="scenes accumulated for compute() and for the CPU restatement")
    ap.add_argument("--out")
    args = ap.parse_args()
    res = dict(device=torch.cuda.get_device_name(0), batch=BATCH, proposals=P, gt=G, limits=LIMITS, ap_thresholds=THRESHOLDS, scenes=args.scenes)
    nb = (args.scenes + BATCH - 1) // BATCH
    for ncols in (7, 6):
        scenes = E.make_scenes(1, ncols, ((P, G),) * (nb * BATCH))[:args.scenes]
        batches = [[t.cuda() for t in E.pack_dense(scenes[k:k + BATCH])] for k in range(0, args.scenes, BATCH)]
        first = batches[0]
        r = {}
        L = lib()
        for _ in range(args.warmup):
            det_eval.det_eval_dense(*first, LIMITS, THRESHOLDS)
        L.profile = {}
        for _ in range(args.reps):
            det_eval.det_eval_dense(*first, LIMITS, THRESHOLDS)
        torch.cuda.synchronize()
        for key, evs in L.profile.items():
            us = [a.elapsed_time(b) * 1e3 for a, b in evs]
            r[key[0].replace("nmh_det_eval_", "")] = dict(median_us=statistics.median(us), min_us=min(us), max_us=max(us), reps=len(us))
        L.profile = None
        ev = det_eval.DetectionEvaluator(LIMITS, THRESHOLDS)

        def one_update():
            ev.reset()
            ev.update(*first)
        r["update"] = timed(one_update, args.reps, args.warmup)
        ev.reset()
        for b in batches:
            ev.update(*b)
        holder = {}
        r["compute"] = timed(lambda: holder.update(out=ev.compute()), max(args.reps // 4, 3), 1)
        out = holder["out"]
        t0 = time.perf_counter()
        ious = E.iou_matrices(scenes)
        t1 = time.perf_counter()
        want = {f"recall_ar_top_{limit}": E.recall(scenes, E.recall_thresholds(0.25), limit, ious)["ar"] for limit in LIMITS}
        for limit in LIMITS:
            E.recall(scenes, [0.5], limit, ious), E.recall(scenes, [0.25], limit, ious)
        want.update({f"ap_{int(t * 100)}": E.ap(scenes, t, None, ious)["ap"] for t in THRESHOLDS})
        t2 = time.perf_counter()
        r["restatement"] = dict(iou_s=t1 - t0, metrics_s=t2 - t1)
        r["values"] = {k: dict(gpu=float(out[k]["ar" if k.startswith("recall") else "ap"]), float64=float(v)) for k, v in want.items()}
        res["obb" if ncols == 7 else "aabb"] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
