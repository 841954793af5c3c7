"""Times the two-stage detector's box head on the GPU at the shape of the reference's launcher (nerf_rpn/train_rcnn.sh: 256 channels, RoI output 3^3, is_add_layer,
is_flatten, oriented boxes, 2 classes):
  (a) training: forward + backward of the head alone at M = 512 rows (the pooled tensor requires a gradient, both outputs have a cotangent);
  (b) prediction: forward under no_grad at M = 4000 rows.
Paths, alternated call by call in one process:
  stock          detector.RCNN, fp32, nn.Conv3d / nn.Linear, called once on all rows
  stock-blocks   (b) only: the same head through Classification_Model._head_blocks, 256 rows per call (what predict_dense does with a stock head)
  fused-bf16     detector.FusedRCNN, compute_dtype bfloat16
  fused-fp32     detector.FusedRCNN, compute_dtype float32
  fused-bf16-out (a) and (b): FusedRCNN(is_add_layer=False), the layout passes and the output kernels alone; fused-bf16 minus this is the conv part on the shared layer
HIP events on one stream around forward and backward; --warmup (10) calls of every path first, then --steps (default 50, at least 50) timed calls per path.
Prints median [min .. max] in ms per path and part, and one JSON line.  Nothing is asserted on the times."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

C, SIZE, NCLS = 256, (3, 3, 3), 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--train-rows", type=int, default=512)
    ap.add_argument("--predict-rows", type=int, default=4000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_box_head needs an MI355X (no CPU fallback)")
    from nerf_mae_amd import detector as D
    torch.manual_seed(0)
    stock = D.RCNN(C, None, NCLS, SIZE, is_add_layer=True, is_rotated_bbox=True, is_flatten=True).cuda()
    heads = {"stock": stock}
    for name, dtype, add in (("fused-bf16", torch.bfloat16, True), ("fused-fp32", torch.float32, True), ("fused-bf16-out", torch.bfloat16, False)):
        h = D.FusedRCNN(C, None, NCLS, SIZE, is_add_layer=add, is_rotated_bbox=True, is_flatten=True, compute_dtype=dtype)
        h.load_state_dict({k: v for k, v in stock.state_dict().items() if add or not k.startswith("layer.")}, strict=True)
        heads[name] = h.cuda()
    blocks = D.Classification_Model(None, None, None, stock, n_classes=NCLS, is_rotated_bbox=True)
    g = torch.Generator().manual_seed(1)
    xt = torch.randn((args.train_rows, C, *SIZE), generator=g).cuda().requires_grad_(True)
    xp = torch.randn((args.predict_rows, C, *SIZE), generator=g).cuda()
    cb, cc = torch.randn((args.train_rows, 7), generator=g).cuda(), torch.randn((args.train_rows, NCLS), generator=g).cuda()

    def ev():
        return torch.cuda.Event(enable_timing=True)

    def train(head):
        e = [ev() for _ in range(3)]
        xt.grad = None
        e[0].record()
        box, cls = head(xt)
        total = (box * cb).sum() + (cls * cc).sum()
        e[1].record()
        total.backward()
        e[2].record()
        return e

    def predict(fn):
        e = [ev() for _ in range(2)]
        with torch.no_grad():
            e[0].record()
            fn(xp)
            e[1].record()
        return e

    jobs = {f"train/{n}": (lambda h=h: train(h)) for n, h in heads.items()}
    jobs.update({f"predict/{n}": (lambda h=h: predict(h)) for n, h in heads.items()})
    jobs["predict/stock-blocks"] = lambda: predict(blocks._head_blocks)
    for _ in range(args.warmup):
        for fn in jobs.values():
            fn()
    torch.cuda.synchronize()
    with torch.no_grad():           # faster and different is not faster: the outputs at the timed size against the stock head's, max-norm relative
        want = stock(xt)
        diff = {n: max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(h(xt), want)) for n, h in heads.items() if n in ("fused-bf16", "fused-fp32")}
    rec = {n: [] for n in jobs}
    for _ in range(max(args.steps, 50)):
        for n, fn in jobs.items():
            rec[n].append(fn())
    torch.cuda.synchronize()
    result = {"metric": "box_head_ms", "channels": C, "output_size": list(SIZE), "train_rows": args.train_rows, "predict_rows": args.predict_rows, "steps": max(args.steps, 50),
              "warmup": args.warmup, "device": torch.cuda.get_device_name(0), "max_rel_diff_vs_stock": {n: float(f"{v:.3e}") for n, v in diff.items()}}
    print("outputs against the stock head, max-norm relative: " + "  ".join(f"{n} {v:.2e}" for n, v in diff.items()))
    for n, runs in rec.items():
        parts = {"forward": [e[0].elapsed_time(e[1]) for e in runs]}
        if n.startswith("train/"):
            parts["backward"] = [e[1].elapsed_time(e[2]) for e in runs]
            parts["both"] = [e[0].elapsed_time(e[2]) for e in runs]
        result[n] = {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)} for k, v in parts.items()}
        print(f"{n:24s} " + "  ".join(f"{k} {r['median']:.3f} [{r['min']:.3f} .. {r['max']:.3f}] ms" for k, r in result[n].items()))
    print(json.dumps(result))


if __name__ == "__main__":
    main()
