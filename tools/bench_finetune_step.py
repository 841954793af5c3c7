"""Times one FCOS fine-tuning step on the GPU: swin_s backbone + FPN(256) + FCOS head (4 tower layers, oriented boxes), 160^3, batch 2, bf16 compute.

Two paths over models with the same weights and the same fixed batch, alternated step by step in one process:
  fused   finetune.FinetuneStep: forward, backward, FusedAdamW over finetune.FlatParameters (three launches, the update clears the gradients)
  stock   the same forward and backward, then torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW over the separate tensors and a zero_grad fill
          (the only way to train the detector before finetune.py existed)
HIP events around forward, backward and optimizer (the stock path's zero fill counts as optimizer time); 10 warm-up steps, --steps (default 50, at least 50)
timed steps per path.  Prints the median and mean of each part in ms and one JSON line.  Nothing is asserted on the times.

Then the optimizer alone over the fused path's flat buffers, two rows from the same run, alternated launch by launch:
  uniform  FusedAdamW.launch(): nmh_grad_sqnorm, nmh_clip_coef, nmh_adamw_step
  ranged   the same under the layer-decay (0.75) + no-decay table of this model: nmh_grad_sqnorm_ranges, nmh_clip_coef, nmh_adamw_step_ranges
HIP events around the norm launch, around the update launch and around all three; --opt-repeats (default 100) timed launches per row after 10 warm-up ones,
each figure as median [min .. max].  --optimizer-only skips the step timing.

--freeze-stages K runs, instead of the above, two rows over two models with the same weights, the same batch and the same range table, alternated
step by step in one process with the same events and warm-ups:
  freeze=        FinetuneStep under freeze=(patch_partition, *stages[:K]): the prefix is not stepped, its backward runs (the path before freeze_stages existed)
  freeze_stages  FinetuneStep under freeze_stages=K: the prefix runs without a graph and the backward ends at stage K
forward, backward, optimizer and step as median [min .. max], and torch.cuda.max_memory_allocated() over one step of each row, measured after the timed steps."""
import argparse
import json
import os
import statistics
import sys
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402


def build(args):
    from nerf_mae_amd.fcos import FCOSOverNeRF
    from nerf_mae_amd.fpn import SwinTransformer_FPN_Pretrained_Skip
    a = types.SimpleNamespace(num_convs=4, norm_reg_targets=True, centerness_on_reg=True, rotated_bbox=True, center_sampling_radius=1.5, iou_loss_type="iou",
                              use_additional_l1_loss=True, proj2d_loss_weight=0.0, pre_nms_thresh=0.0, pre_nms_top_n=2500, nms_thresh=0.3, fpn_post_nms_top_n=2500,
                              min_size=0.0, compute_dtype=torch.bfloat16)
    torch.manual_seed(0)
    bb = SwinTransformer_FPN_Pretrained_Skip(resolution=args.resolution, is_eval=True, backbone_type=args.backbone, out_channels=256, compute_dtype=torch.bfloat16)
    return FCOSOverNeRF(a, bb, [4, 8, 16, 32], resolution=args.resolution)


def batch(args):
    from nerf_mae_amd import data
    R = args.resolution
    batcher = data.DetectionBatcher(R, torch.device("cuda"), normalize_density=True)
    rng = np.random.default_rng(0)
    boxes = []
    for _ in range(args.batch):
        c = rng.uniform(0.25 * R, 0.75 * R, (8, 3))
        s = np.exp(rng.uniform(np.log(8.0), np.log(0.4 * R), (8, 3)))
        boxes.append(np.concatenate([c, s, rng.uniform(-0.5, 0.5, (8, 1))], 1).astype(np.float32))
    xb, ext, targets = batcher.prepare([data.synthetic_scene((R, R, R), i + 1) for i in range(args.batch)], boxes, params=[(0, 0.0, 1.0)] * args.batch)
    return [xb[i] for i in range(args.batch)], targets


def freeze_rows(args):
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, fcos_loss_fn, param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW
    K = args.freeze_stages
    P = build(args)
    Q = build(args)
    Q.load_state_dict(P.state_dict(), strict=True)
    meshes, targets = batch(args)
    rows = {}
    for name, m in (("freeze=", P), ("freeze_stages", Q)):
        m = m.cuda().train()
        flat = FlatParameters(m)
        base = flat.base
        rules = recipe_rules(m, freeze=(base.patch_partition, *base.stages[:K])) if name == "freeze=" else recipe_rules(m, freeze_stages=K)
        opt = FusedAdamW(flat, lr=1e-4, weight_decay=1e-2, max_grad_norm=0.1, ranges=param_ranges(flat, rules))
        rows[name] = (flat, opt, FinetuneStep(flat, opt, fcos_loss_fn(m)))
    assert rows["freeze="][1].range_record == rows["freeze_stages"][1].range_record

    def one(name):
        flat, opt, step = rows[name]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        losses, total = step.forward(meshes, targets)
        e[1].record()
        total.backward()
        e[2].record()
        opt.step()
        e[3].record()
        return e

    for _ in range(args.warmup):
        for name in rows:
            one(name)
    torch.cuda.synchronize()
    rec = {name: [] for name in rows}
    for _ in range(max(args.steps, 1)):
        for name in rows:
            rec[name].append(one(name))
    torch.cuda.synchronize()
    result = {"metric": "fcos_finetune_freeze_stages_ms", "backbone": args.backbone, "resolution": args.resolution, "batch": args.batch, "dtype": "bf16",
              "steps": args.steps, "warmup": args.warmup, "freeze_stages": K, "elements": int(rows["freeze="][0]._flat.numel()),
              "frozen_elements": int(rows["freeze="][1].range_record["bounds"][1])}
    print(f"freeze_stages = {K}, {args.backbone} {args.resolution}^3 batch {args.batch}, {args.steps} steps each, ms as median [min .. max]:")
    for name, runs in rec.items():
        parts = {"forward": [e[0].elapsed_time(e[1]) for e in runs], "backward": [e[1].elapsed_time(e[2]) for e in runs],
                 "optimizer": [e[2].elapsed_time(e[3]) for e in runs], "step": [e[0].elapsed_time(e[3]) for e in runs]}
        result[name] = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in parts.items()}
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        one(name)
        torch.cuda.synchronize()
        result[name]["max_memory_allocated_mib"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
        result[name]["allocated_before_the_step_mib"] = round(held / 2 ** 20, 1)
        print(f"{name:13s} " + "  ".join(f"{k} {statistics.median(v):.3f} [{min(v):.3f} .. {max(v):.3f}]" for k, v in parts.items())
              + f"  peak {result[name]['max_memory_allocated_mib']:.1f} MiB (held before the step {result[name]['allocated_before_the_step_mib']:.1f})")
    print(json.dumps(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=160)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--backbone", default="swin_s")
    ap.add_argument("--opt-repeats", type=int, default=100)
    ap.add_argument("--optimizer-only", action="store_true")
    ap.add_argument("--freeze-stages", type=int, default=0, help="K > 0: time freeze= over the prefix against freeze_stages=K instead (DESIGN.md 3.27)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_finetune_step needs an MI355X (no CPU fallback)")
    if args.freeze_stages:
        return freeze_rows(args)
    from nerf_mae_amd import ops
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, fcos_loss_fn, param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW
    A = build(args)
    B = build(args)
    B.load_state_dict(A.state_dict(), strict=True)
    A, B = A.cuda().train(), B.cuda().train()
    meshes, targets = batch(args)
    flat = FlatParameters(A)
    fopt = FusedAdamW(flat, lr=1e-4, weight_decay=1e-2, max_grad_norm=0.1)
    step = FinetuneStep(flat, fopt, fcos_loss_fn(A))
    sopt = torch.optim.AdamW(B.parameters(), lr=1e-4, weight_decay=1e-2)

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def fused():
        e = [ev() for _ in range(4)]
        e[0].record()
        losses, total = step.forward(meshes, targets)
        e[1].record()
        total.backward()
        e[2].record()
        fopt.step()
        e[3].record()
        return e

    def stock():
        e = [ev() for _ in range(4)]
        e[0].record()
        out = B(list(meshes), targets)[1]
        total = out["loss_cls"] + out["loss_reg"] + out["loss_centerness"]
        e[1].record()
        total.backward()
        e[2].record()
        torch.nn.utils.clip_grad_norm_(B.parameters(), 0.1)
        sopt.step()
        sopt.zero_grad(set_to_none=False)
        e[3].record()
        return e

    rec = {"fused": [], "stock": []}
    if not args.optimizer_only:
        for _ in range(args.warmup):
            fused()
            stock()
        torch.cuda.synchronize()
        for _ in range(max(args.steps, 1)):
            rec["fused"].append(fused())
            rec["stock"].append(stock())
        torch.cuda.synchronize()
    result = {"metric": "fcos_finetune_step_ms", "backbone": args.backbone, "resolution": args.resolution, "batch": args.batch, "dtype": "bf16", "steps": args.steps,
              "warmup": args.warmup, "tensors": len([p for p in A.parameters() if p.requires_grad]), "elements": int(flat._flat.numel())}
    for name, runs in rec.items():
        if not runs:
            continue
        parts = {"forward": [e[0].elapsed_time(e[1]) for e in runs], "backward": [e[1].elapsed_time(e[2]) for e in runs],
                 "optimizer": [e[2].elapsed_time(e[3]) for e in runs], "step": [e[0].elapsed_time(e[3]) for e in runs]}
        result[name] = {k: {"median": round(statistics.median(v), 3), "mean": round(statistics.fmean(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}
                        for k, v in parts.items()}
        print(f"{name:5s} " + "  ".join(f"{k} {result[name][k]['median']:.3f} ms (mean {result[name][k]['mean']:.3f})" for k in parts))
    # ---- the optimizer alone: one setting against the per-range table, over the same buffers --------------------------------------------------
    table = param_ranges(flat, recipe_rules(A, layer_decay=0.75, no_decay=True))
    ropt = FusedAdamW(flat, lr=1e-4, weight_decay=1e-2, max_grad_norm=0.1, ranges=table)
    flat._flat_grad.normal_(0.0, 1e-3)                                # a gradient that stays: neither optimizer clears it here
    for o in (fopt, ropt):
        o.zero_grads_after_step = False
        o.set_hyper(lr=1e-6)
        o.update_hyper()
    g, (bounds, scale) = flat._flat_grad, ropt.ranges

    def opt_uniform():
        e = [ev() for _ in range(4)]
        e[0].record()
        ops.grad_sqnorm(g, fopt.acc)
        e[1].record()
        ops.clip_coef(fopt.acc, 0.1, fopt.coef, fopt.norm)
        e[2].record()
        ops.adamw_step(flat._flat, g, fopt.m, fopt.v, fopt.hyper, fopt.coef)
        e[3].record()
        return e

    def opt_ranged():
        e = [ev() for _ in range(4)]
        e[0].record()
        ops.grad_sqnorm_ranges(g, bounds, scale, ropt.acc)
        e[1].record()
        ops.clip_coef(ropt.acc, 0.1, ropt.coef, ropt.norm)
        e[2].record()
        ops.adamw_step_ranges(flat._flat, g, ropt.m, ropt.v, ropt.hyper, bounds, scale, ropt.coef)
        e[3].record()
        return e

    for _ in range(10):
        opt_uniform()
        opt_ranged()
    torch.cuda.synchronize()
    orec = {"uniform": [], "ranged": []}
    for _ in range(max(args.opt_repeats, 1)):
        orec["uniform"].append(opt_uniform())
        orec["ranged"].append(opt_ranged())
    torch.cuda.synchronize()
    result["optimizer_rows"] = {"ranges": len(table.record["scale"]), "repeats": args.opt_repeats, "bytes_per_launch_set": 8 * 4 * int(flat._flat.numel())}
    print(f"optimizer alone over {flat._flat.numel()} elements, {len(table.record['scale'])} ranges, {args.opt_repeats} launches each, ms as median [min .. max]:")
    for name, runs in orec.items():
        parts = {"norm": [e[0].elapsed_time(e[1]) for e in runs], "update": [e[2].elapsed_time(e[3]) for e in runs], "three": [e[0].elapsed_time(e[3]) for e in runs]}
        result["optimizer_rows"][name] = {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in parts.items()}
        print(f"{name:8s} " + "  ".join(f"{k} {statistics.median(v):.4f} [{min(v):.4f} .. {max(v):.4f}]" for k, v in parts.items()))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
