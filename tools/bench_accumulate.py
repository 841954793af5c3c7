"""Gradient accumulation: ms per optimizer step and per micro-step of GraphedTrainStep(accumulate=k) at k = 1, 2, 4, micro-batches of 8 grids
of 160^3 (swin_s, bf16), on one GPU.  k = 1 is the step without the keyword -- the same graph, the same launches -- so its line is the step of the commit before;
it is measured first and once more at the end, which shows the drift of the run.  For k > 1 device events split each optimizer step into the k replays of the
forward + backward graph and the one replay of the clip + AdamW graph: what the separate optimizer graph costs is that last figure plus whatever a micro-step
takes beyond (step of k = 1 minus the optimizer's three kernels).

    python tools/bench_accumulate.py [--grids 8] [--resolution 160] [--backbone swin_s] [--steps 6] [--warmup 2] [--ks 1,2,4]

Prints one line per configuration and, last, one JSON line."""
import argparse
import json
import random
import statistics
import sys

import torch

sys.path.insert(0, ".")
from nerf_mae_amd import data, ops  # noqa: E402
from nerf_mae_amd.model import build_model, draw_block_mask  # noqa: E402
from nerf_mae_amd.trainer import FusedAdamW, GraphedTrainStep  # noqa: E402


def measure(model, xb, ext, k, steps, warmup, rng):
    """-> medians over `steps` optimizer steps: (ms per step, ms per micro-step, ms of the optimizer graph or None)"""
    B, g = xb.shape[0], model.resolution // 4
    opt = FusedAdamW(model, lr=1e-6, weight_decay=1e-3, max_grad_norm=0.1)
    step = GraphedTrainStep(model, opt, B, accumulate=k)
    step.x.copy_(xb)
    mask = lambda: draw_block_mask((g, g, g), model.masking_prob, rng=rng)  # noqa: E731
    rows = []
    for it in range(warmup + steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        if k == 1:
            step.set_extents(ext)
            step(None, mask())
            ev[1].record()
        else:
            step.begin([mask() for _ in range(k)])
            for j in range(k):
                step.set_extents(ext)
                step.micro(j)
            ev[1].record()
            step.finish()
        ev[2].record()
        torch.cuda.synchronize()
        if it >= warmup:
            rows.append((ev[0].elapsed_time(ev[2]), ev[0].elapsed_time(ev[1]) / k, ev[1].elapsed_time(ev[2])))
    del step, opt
    torch.cuda.empty_cache()
    med = [statistics.median(c) for c in zip(*rows)]
    return med[0], (med[0] if k == 1 else med[1]), (None if k == 1 else med[2]), min(r[0] for r in rows), max(r[0] for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--grids", type=int, default=8)
    ap.add_argument("--resolution", type=int, default=160)
    ap.add_argument("--backbone", default="swin_s")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--ks", default="1,2,4")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_accumulate: needs the GPU (no CPU timing)")
    R = a.resolution
    ops.side_stream.auto(a.grids)
    torch.manual_seed(0)
    model = build_model(a.backbone, R, 0.75, 0.1).cuda().train()
    model.flatten_parameters()
    batcher = data.GridBatcher(R, torch.device("cuda"), True)
    xb, ext = batcher([data.synthetic_scene((R, R, R), seed=50 + i) for i in range(a.grids)], flags=[0] * a.grids)
    ext = ext.tolist() if hasattr(ext, "tolist") else ext
    ks = [int(v) for v in a.ks.split(",")]
    out = []
    for k in ks + [1]:           # k = 1 again at the end: the drift of the run
        rng = random.Random(7)
        ms, micro, optg, lo, hi = measure(model, xb, ext, k, a.steps, a.warmup, rng)
        out.append({"accumulate": k, "ms_per_optimizer_step": round(ms, 3), "ms_per_micro_step": round(micro, 3),
                    "ms_optimizer_graph": None if optg is None else round(optg, 3), "min": round(lo, 3), "max": round(hi, 3)})
        print(f"accumulate {k}: {ms:8.2f} ms / optimizer step (min {lo:.2f}, max {hi:.2f}), {micro:8.2f} ms / micro-step"
              + ("" if optg is None else f", optimizer graph {optg:.2f} ms"), flush=True)
    print(json.dumps({"bench": "accumulate", "backbone": a.backbone, "resolution": R, "grids_per_micro_batch": a.grids, "dtype": "bf16", "steps": a.steps,
                      "warmup": a.warmup, "rows": out}))


if __name__ == "__main__":
    main()
