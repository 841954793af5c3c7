"""Times the detection input pipeline's kernels on the GPU at the sizes users run and writes profiles/det_input_bench.json.
    python tools/bench_det_input.py [--reps 50] [--warmup 10] [--out profiles/det_input_bench.json]

Per configuration (scene shape x stored dtype, batch 4, R = 160) four variants are timed with device events around one batch each, alternated within
every repetition so that clock and cache state drift hits all of them alike:
    grid_prepare     the existing kernel (rot + flip), the floor: it moves the same bytes without the resample
    grid_prepare_rs  rot + flip + rot-scale in one pass
    boxes            one nmh_boxes_augment launch for the batch (4 x 32 oriented boxes)
    torch            the same result from stock torch ops on the same GPU: convert, permute, transpose/flip, sampling grid, F.grid_sample, pad
Reported: median, 10th and 90th percentile in microseconds per batch, algorithmic GB/s (stored scenes read once + 4 R^3 floats written per scene), the
ratio of grid_prepare_rs to grid_prepare and of torch to grid_prepare_rs, and whether the gap to torch exceeds the observed spread."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nerf_mae_amd import data, ops  # noqa: E402

R, BATCH, FLAGS, ANGLE, SCALE = 160, 4, ops.GRID_ROT | ops.GRID_FLIP0, 0.12, 0.94


def torch_composition(src, dst, flags, angle, scale, density):
    """stock-torch equivalent of grid_prepare_rs on the device"""
    g = src.float()
    if src.dtype == torch.uint8:
        g = g / 255.0
    elif density:
        g = torch.cat([g[..., :3], torch.clamp(1.0 - torch.exp(-torch.exp(g[..., 3:]) / 100.0), 0.0, 1.0)], -1)
    g = g.permute(3, 0, 1, 2)
    if flags & ops.GRID_ROT:
        g = g.transpose(1, 2).flip(1)
    if flags & ops.GRID_FLIP0:
        g = g.flip(1)
    if flags & ops.GRID_FLIP1:
        g = g.flip(2)
    r0, r1, r2 = g.shape[1:]
    dev = g.device
    axes = [torch.linspace(-1, 1, r, device=dev) * r / 2 for r in (r0, r1, r2)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3)
    c, s = math.cos(angle), math.sin(angle)
    m = torch.tensor([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]], device=dev) * scale
    pts = pts @ m.T
    norm = torch.stack([pts[:, 2] / (r2 / 2), pts[:, 1] / (r1 / 2), pts[:, 0] / (r0 / 2)], -1).reshape(1, r0, r1, r2, 3)
    out = F.grid_sample(g.unsqueeze(0), norm, align_corners=True)[0]
    dst.zero_()
    dst[:, :r0, :r1, :r2] = out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "det_input_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    xb = torch.empty((BATCH, 4, R, R, R), dtype=torch.float32, device=dev)
    rng = np.random.default_rng(0)
    boxes = torch.from_numpy(rng.uniform(1.0, 150.0, size=(BATCH * 32, 7)).astype(np.float32)).to(dev)
    results = []
    for shape in ((160, 160, 160), (160, 132, 96)):
        for dtype in (np.float32, np.uint8):
            scenes = [torch.from_numpy(data.synthetic_scene(shape, seed=i, dtype=dtype)).to(dev) for i in range(BATCH)]
            f = FLAGS | (ops.GRID_DENSITY if dtype == np.float32 else 0)
            ext = (shape[1], shape[0], shape[2])
            table = [(32 * i, 32, FLAGS, True, ext, ANGLE, SCALE) for i in range(BATCH)]
            out_boxes = torch.empty_like(boxes)

            def v_prepare():
                for i, s in enumerate(scenes):
                    ops.grid_prepare(s, xb[i], R, f)

            def v_rs():
                for i, s in enumerate(scenes):
                    ops.grid_prepare_rs(s, xb[i], R, f, ANGLE, SCALE)

            def v_boxes():
                ops.boxes_augment(boxes, table, out_boxes)

            def v_torch():
                for i, s in enumerate(scenes):
                    torch_composition(s, xb[i], FLAGS, ANGLE, SCALE, dtype == np.float32)
            variants = [("grid_prepare", v_prepare), ("grid_prepare_rs", v_rs), ("boxes", v_boxes), ("torch", v_torch)]
            v_rs()
            a = xb.clone()
            v_torch()
            agree = float((a - xb).abs().max())          # the two compute the same thing (fp32 coordinate rounding apart)
            times = {n: [] for n, _ in variants}
            for rep in range(args.warmup + args.reps):
                for n, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    if rep >= args.warmup:
                        times[n].append(e0.elapsed_time(e1) * 1e3)
            nbytes = BATCH * (scenes[0].numel() * scenes[0].element_size() + 4 * R ** 3 * 4)
            row = dict(shape=list(shape), dtype=np.dtype(dtype).name, batch=BATCH, R=R, reps=args.reps, warmup=args.warmup, algorithmic_bytes=nbytes,
                       max_abs_diff_rs_vs_torch=agree)
            for n, _ in variants:
                t = np.array(times[n])
                row[n] = dict(median_us=float(np.median(t)), p10_us=float(np.percentile(t, 10)), p90_us=float(np.percentile(t, 90)),
                              min_us=float(t.min()), max_us=float(t.max()))
                if n != "boxes":
                    row[n]["GBps"] = nbytes / (float(np.median(t)) * 1e-6) / 1e9
            row["rs_over_prepare"] = row["grid_prepare_rs"]["median_us"] / row["grid_prepare"]["median_us"]
            row["torch_over_rs"] = row["torch"]["median_us"] / row["grid_prepare_rs"]["median_us"]
            row["rs_faster_than_torch_beyond_spread"] = bool(row["grid_prepare_rs"]["p90_us"] < row["torch"]["p10_us"])
            results.append(row)
            print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(dict(device=torch.cuda.get_device_name(0), flags=FLAGS, angle=ANGLE, scale=SCALE, results=results), fh, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
