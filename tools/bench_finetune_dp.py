"""What data-parallel fine-tuning adds to a FCOS step: the model and batch of tools/bench_finetune_step.py (swin_s + FPN(256) + FCOS head with 4 tower layers,
oriented boxes, 160^3, batch 2, bf16 compute) with dist.FlatGradReducer.

One GPU (python tools/bench_finetune_dp.py): prints the segment table (elements and bytes on the wire per range, fp32 and bf16 buckets), then times
finetune.FinetuneStep without a reducer, with a forced one-rank reducer (NMH_DP_FORCE=1 over a one-rank RCCL group: triggers, bucket casts, comm stream and
joins are real, the collective moves nothing) with fp32 buckets, and the same with bf16 buckets: three models with the same weights and the same fixed batch,
alternated step by step in one process, HIP events around the whole step, 10 warm-ups, median [min .. max] of --steps (default 50).  The value to compare
against is the step without the reducer IN THE SAME RUN.

N > 1 GPUs (python -m torch.distributed.run --nproc_per_node N tools/bench_finetune_dp.py [--comm fp32]): every rank runs the step with the reducer over
RCCL on the same batch; rank 0 prints the step time and timing_report(): per-range ms and the exposed comm time.

--freeze-stages K: every model of the run trains under freeze_stages=K, and the bytes exchanged per step -- the ranges from the first live
segment on -- are reported beside the whole buffer's.

Prints one JSON line at the end.  Nothing is asserted on the times."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def segment_table(red):
    """[{"segment", "lo", "hi", "elements", "bytes_fp32", "bytes_bf16"}] in forward order"""
    names = {0: "embed", red.seg_tail(): "tail"}
    for si in range(4):
        if si == red.chunk_stage:
            for k in range(red.nchunks):
                names[red.seg_stage(si, k)] = f"stage {si}, block group {k}"
        else:
            names[red.seg_stage(si)] = f"stage {si}"
    return [{"segment": names[s], "lo": red.bounds[s], "hi": red.bounds[s + 1], "elements": red.bounds[s + 1] - red.bounds[s],
             "bytes_fp32": 4 * (red.bounds[s + 1] - red.bounds[s]), "bytes_bf16": 2 * (red.bounds[s + 1] - red.bounds[s])} for s in range(red.nseg)]


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def show(name, s):
    print(f"{name:28s} step {s['median']:.3f} ms [{s['min']:.3f} .. {s['max']:.3f}]")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=160)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--backbone", default="swin_s")
    ap.add_argument("--comm", default="bf16", choices=["bf16", "fp32"], help="bucket dtype of the N > 1 run")
    ap.add_argument("--freeze-stages", type=int, default=0, help="K: every model of the run trains under freeze_stages=K (DESIGN.md 3.27)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune_dp needs an MI355X (no CPU fallback)")
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(dev)
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29537")
    if world == 1:
        os.environ["NMH_DP_FORCE"] = "1"
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
    import bench_finetune_step as one
    from nerf_mae_amd.dist import FlatGradReducer, broadcast_flat_parameters
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, fcos_loss_fn, param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW
    meshes, targets = one.batch(args)
    result = {"metric": "fcos_finetune_dp_step_ms", "backbone": args.backbone, "resolution": args.resolution, "batch": args.batch, "dtype": "bf16",
              "steps": args.steps, "warmup": args.warmup, "n_gpus": world}

    def make(comm, weights=None):
        """comm: None (no reducer), "fp32" or "bf16" buckets -> (the step, its reducer, the model)"""
        m = one.build(args)
        m.world_size = m.fcos_module.world_size = m.fcos_module.loss_evaluator.world_size = world
        if weights is not None:
            m.load_state_dict(weights, strict=True)
        m = m.to(dev).train()
        flat = FlatParameters(m)
        red = None if comm is None else FlatGradReducer(flat, comm_dtype=torch.bfloat16 if comm == "bf16" else None)
        broadcast_flat_parameters(flat)
        rules = recipe_rules(m, freeze_stages=args.freeze_stages)
        opt = FusedAdamW(flat, lr=1e-4, weight_decay=1e-2, max_grad_norm=0.1, ranges=param_ranges(flat, rules) if rules else None)
        if red is not None:
            n, lo = int(red.bounds[-1]), int(red.bounds[red.first_live_segment()])
            result["exchanged_per_step"] = {"freeze_stages": args.freeze_stages, "elements": n - lo, "of": n, "bytes_fp32": 4 * (n - lo), "bytes_bf16": 2 * (n - lo)}
        return FinetuneStep(flat, opt, fcos_loss_fn(m), reducer=red), red, m

    def timed(step):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(meshes, targets)
        e1.record()
        return e0, e1

    try:
        if world == 1:
            plain, _, m0 = make(None)
            w = {k: v.detach().cpu().clone() for k, v in m0.state_dict().items()}
            paths = {"no reducer": plain, "one-rank reducer, fp32 buckets": make("fp32", w)[0], "one-rank reducer, bf16 buckets": make("bf16", w)[0]}
            red = paths["one-rank reducer, fp32 buckets"].reducer
            result["elements"] = int(red.bounds[-1])
            result["segments"] = segment_table(red)
            print(f"{'segment':24s} {'lo':>10s} {'hi':>10s} {'elements':>10s} {'fp32 bytes':>12s} {'bf16 bytes':>12s}")
            for r in result["segments"]:
                print(f"{r['segment']:24s} {r['lo']:10d} {r['hi']:10d} {r['elements']:10d} {r['bytes_fp32']:12d} {r['bytes_bf16']:12d}")
            x = result["exchanged_per_step"]
            print(f"exchanged per step under freeze_stages = {x['freeze_stages']}: {x['elements']} of {x['of']} elements, {x['bytes_fp32']} bytes in fp32 buckets, "
                  f"{x['bytes_bf16']} in bf16")
            for _ in range(args.warmup):
                for s in paths.values():
                    s(meshes, targets)
            torch.cuda.synchronize()
            rec = {k: [] for k in paths}
            for _ in range(max(args.steps, 1)):
                for k, s in paths.items():
                    rec[k].append(timed(s))
            torch.cuda.synchronize()
            result["paths"] = {k: stats([a.elapsed_time(b) for a, b in v]) for k, v in rec.items()}
            for k, s in result["paths"].items():
                show(k, s)
        else:
            step, red, _ = make(args.comm)
            result["grad_comm_dtype"] = args.comm
            for _ in range(args.warmup):
                step(meshes, targets)
            torch.cuda.synchronize()
            dist.barrier()
            red.timing_begin()
            runs = [timed(step) for _ in range(max(args.steps, 1))]
            torch.cuda.synchronize()
            result["paths"] = {f"{world} ranks, {args.comm} buckets": stats([a.elapsed_time(b) for a, b in runs])}
            result["comm_events"] = red.timing_report(max(args.steps, 1))
            if rank == 0:
                for k, s in result["paths"].items():
                    show(k, s)
                print(result["comm_events"])
        if rank == 0:
            print(json.dumps(result))
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
