"""Times the voxel heads' target pipeline on the GPU at the sizes users run and writes profiles/voxel_input_bench.json.
    python tools/bench_voxel_input.py [--reps 10] [--warmup 3] [--out profiles/voxel_input_bench.json]

Per configuration (batch 2, R = 160, host-resident synthetic scenes) two paths that end in the same device tensors are timed, alternated within every
repetition so that clock and cache state drift hits both alike:
    batcher   data.VoxelBatcher.prepare: scene and STORED target through pinned rings, nmh_grid_prepare + nmh_labels_prepare (or nmh_grid_prepare at Ro)
    list      the path without it: data.GridBatcher.prepare for the scenes, and for the targets what a caller of loss_fn does today -- a list of host fp32
              grids at full size, `[t.cuda() for t in targets]`, then the head's `transform` (zero fill + one copy per grid)
Configurations: labels (stored uint8 (160,160,160); list form (1,160,160,160) fp32), and the SR target at Ro = 256 stored as uint8 and as fp32
((256,256,256,4); list form (4,256,256,256) fp32, alpha already normalised).  Every batch is timed twice: by the wall clock from the call to the
completion of its last kernel (the stream is idle at the start), and with device events around it.  The wall clock is the figure to read: the first event is
submitted together with the first device work, so host-side staging in front of it (the copy into the pinned ring) is not inside the event interval.
Reported: median, 10th and 90th percentile of the event times and the wall-clock median in milliseconds per batch, the target bytes that cross to the device per
batch on either path, and the ratio of the wall-clock medians.  Nothing is asserted."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_mae_amd import data  # noqa: E402
from nerf_mae_amd.heads import _VoxelHeadBase  # noqa: E402

R, RO, BATCH = 160, 256, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_input_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    head = types.SimpleNamespace(base=types.SimpleNamespace(pos_embed=torch.empty(0, device=dev)))          # all that `transform` reads of a head
    scenes = [data.synthetic_scene((R, R, R), seed=i, dtype=np.uint8) for i in range(BATCH)]
    rng = np.random.default_rng(0)
    results = []
    for name, stored_dtype in (("labels", np.uint8), ("sr", np.uint8), ("sr", np.float32)):
        if name == "labels":
            stored = [rng.integers(0, 19, (R, R, R)).astype(stored_dtype) for _ in range(BATCH)]
            as_list = [torch.from_numpy(s.astype(np.float32))[None] for s in stored]
            batcher = data.VoxelBatcher(R, dev, target="labels")
            res = R
        else:
            stored = [data.synthetic_scene((RO, RO, RO), seed=10 + i, dtype=stored_dtype) for i in range(BATCH)]
            as_list = [torch.from_numpy(np.ascontiguousarray(np.moveaxis(data.synthetic_scene((RO, RO, RO), seed=10 + i, dtype=np.uint8).astype(np.float32) / 255.0, 3, 0)))
                       for i in range(BATCH)]
            batcher = data.VoxelBatcher(R, dev, target="grid", target_resolution=RO)
            res = RO
        plain = data.GridBatcher(R, dev)
        flags = [0] * BATCH

        def v_batcher():
            return batcher.prepare(scenes, stored, flags=flags)

        def v_list():
            xb, ext = plain.prepare(scenes, flags=flags)
            tb = _VoxelHeadBase.transform(head, [t.cuda() for t in as_list], resolution=res)
            return xb, ext, tb
        variants = [("batcher", v_batcher), ("list", v_list)]
        times, walls = {n: [] for n, _ in variants}, {n: [] for n, _ in variants}
        for rep in range(args.warmup + args.reps):
            for n, fn in variants:
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                out = fn()
                e1.record()
                e1.synchronize()
                t1 = time.perf_counter()
                del out
                if rep >= args.warmup:
                    times[n].append(e0.elapsed_time(e1))
                    walls[n].append((t1 - t0) * 1e3)
        row = dict(target=name, stored_dtype=np.dtype(stored_dtype).name, batch=BATCH, R=R, target_resolution=res, reps=args.reps, warmup=args.warmup,
                   target_bytes_to_device=dict(batcher=sum(s.nbytes for s in stored), list=sum(t.numel() * 4 for t in as_list)))
        for n, _ in variants:
            t, w = np.array(times[n]), np.array(walls[n])
            row[n] = dict(median_ms=float(np.median(t)), p10_ms=float(np.percentile(t, 10)), p90_ms=float(np.percentile(t, 90)), wall_median_ms=float(np.median(w)))
        row["list_over_batcher_wall"] = row["list"]["wall_median_ms"] / row["batcher"]["wall_median_ms"]
        results.append(row)
        print(json.dumps(row))
        del stored, as_list, batcher, plain
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), results=results), fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
