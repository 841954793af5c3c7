"""Times one training step of the RPN and of the two-stage detector in the modes of trainer.RPNTrainer / trainer.TwoStageTrainer on the GPU, at
the launcher's shape: swin_s backbone, 160^3, 256 FPN channels, batch 2, bf16 compute, axis-aligned boxes, the reference's default RPN head; the second stage
with a 3^3 RoI output, 512 sampled rows and FusedRCNN(is_add_layer, is_flatten).

  rpn/unfrozen, rpn/frozen                       NeRFRegionProposalNetwork, everything trains / freeze_backbone
  two_stage/head, /fine_tune, /joint, /heads     TwoStageDetector in the four combinations of train_rpn and freeze_first_stage

Every path is the trainer's own FinetuneStep over its own model (same seed, same fixed batch), so what is timed is what train_epoch runs per batch without the
input pipeline.  The paths of a group are alternated step by step in one process; HIP events around the whole step (forward, backward, clip + AdamW); --warmup
(10) steps of every path first, then --steps (default 50) timed steps per path.  Prints median [min .. max] in ms per path and one JSON line.  Nothing is
asserted on the times."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT, ROWS = (3, 3, 3), 512


def rpn_model(args):
    from nerf_mae_amd.fpn import SwinTransformer_FPN_Pretrained_Skip
    from nerf_mae_amd.rpn import NeRFRegionProposalNetwork
    torch.manual_seed(0)
    bb = SwinTransformer_FPN_Pretrained_Skip(resolution=args.resolution, is_eval=True, backbone_type=args.backbone, out_channels=256, compute_dtype=torch.bfloat16)
    net = NeRFRegionProposalNetwork(bb, rpn_fg_iou_thresh=0.35, rpn_bg_iou_thresh=0.2)
    net.check_targets = False
    return net


def two_stage(args, train_rpn):
    from nerf_mae_amd import detector as D
    rpn = rpn_model(args)
    torch.manual_seed(100)
    layer = D.ProposalTargetLayer(2, batch_size=ROWS, fg_fraction=0.5, fg_threshold=0.35, bg_threshold=0.15, is_rotated_bbox=False)
    pool = D.ROIPool(OUT, [4.0, 8.0, 16.0, 32.0], 0.2, False, "pooling", args.resolution, False)
    head = D.FusedRCNN(256, None, 2, OUT, is_add_layer=True, is_rotated_bbox=False, is_flatten=True)
    return D.TwoStageDetector(rpn, D.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=False), 0.5, 0.1, train_rpn=train_rpn)


def scenes_and_boxes(args):
    from nerf_mae_amd import data
    R = args.resolution
    rng = np.random.default_rng(0)
    boxes = []
    for _ in range(args.batch):
        c = rng.uniform(0.25 * R, 0.75 * R, (8, 3))
        s = np.exp(rng.uniform(np.log(8.0), np.log(0.4 * R), (8, 3)))
        boxes.append(np.concatenate([np.clip(c - s / 2, 0, R - 1), np.clip(c + s / 2, 1, R)], 1).astype(np.float32))
    return [data.synthetic_scene((R, R, R), i + 1) for i in range(args.batch)], boxes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--resolution", type=int, default=160)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--backbone", default="swin_s")
    ap.add_argument("--only", choices=["rpn", "two_stage"], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_det_trainers needs an MI355X (no CPU fallback)")
    from nerf_mae_amd.trainer import RPNTrainer, TwoStageTrainer
    scenes, boxes = scenes_and_boxes(args)
    common = dict(batch_size=args.batch, num_epochs=1, log=lambda s: None)
    groups = {}
    if args.only in (None, "rpn"):
        groups["rpn"] = {name: RPNTrainer(rpn_model(args).cuda().train(), scenes, boxes, freeze_backbone=frozen, **common)
                         for name, frozen in (("unfrozen", False), ("frozen", True))}
    if args.only in (None, "two_stage"):
        groups["two_stage"] = {name: TwoStageTrainer(two_stage(args, train_rpn).cuda().train(), scenes, boxes, freeze_first_stage=freeze, **common)
                               for name, train_rpn, freeze in (("head", False, True), ("fine_tune", False, False), ("joint", True, False), ("heads", True, True))}
    result = {"metric": "det_trainer_step_ms", "backbone": args.backbone, "resolution": args.resolution, "batch": args.batch, "dtype": "bf16", "steps": args.steps,
              "warmup": args.warmup}
    for group in list(groups):
        trainers, batches = groups.pop(group), {}          # popped: a group's models are freed before the next group's steps
        for name, tr in trainers.items():
            tr._train_mode()
            batches[name] = tr._batch(list(range(args.batch)))          # one fixed batch per path, prepared once, without augmentation
            lr, b1 = tr.sched.at(0)
            tr.opt.set_hyper(lr=lr, beta1=b1)

        def one(name):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            e[0].record()
            trainers[name].step_fn(*batches[name])
            e[1].record()
            return e

        for _ in range(args.warmup):
            for name in trainers:
                one(name)
        torch.cuda.synchronize()
        runs = {name: [] for name in trainers}
        for _ in range(max(args.steps, 1)):
            for name in trainers:
                runs[name].append(one(name))
        torch.cuda.synchronize()
        for name, tr in trainers.items():
            ms = [a.elapsed_time(b) for a, b in runs[name]]
            result[f"{group}/{name}"] = {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3),
                                         "stepped_elements": int(tr.flat._flat.numel())}
            print(f"{group + '/' + name:22s} {statistics.median(ms):9.3f} ms [{min(ms):.3f} .. {max(ms):.3f}]  stepped elements {tr.flat._flat.numel()}")
        del trainers, batches, one
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
