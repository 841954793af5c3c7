"""FCOS inference post-processing at the downstream shape: 2 scenes x 73 125 locations (levels 40^3, 20^3, 10^3, 5^3, strides 4 .. 32 on a
160^3 scene), pre_nms_top_n = fpn_post_nms_top_n = 2500, pre_nms_thresh 0.0, nms_thresh 0.3, axis-aligned and oriented.
    python tools/bench_fcos_post.py [reps]          (also run as the last case of tools/bench_rotated.py)

Timed with HIP events, median and minimum of `reps` >= 20 calls after 5 warm-up calls, each line in two runs of the loop:
  fused        nerf_mae_amd.fcos_inference.FCOSPostProcessor (list form: one host synchronisation)
  dense        fcos_postprocess_dense, eager (no host synchronisation)
  graph        the dense form replayed from a captured graph
  composition  the steps of the semantics (csrc/fcos_post.hip) from framework ops around this project's decode_fcos_obb and rotated_iou.nms:
               per level and scene sigmoid, threshold, nonzero, topk, decode, clip, size filter, sqrt; per scene cat, nms, kthvalue cut.
               Written here from the semantics; it lives in this tool, not in the product.
The composition and the fused op are also compared: the same counts and, in order, scores that agree to 1e-5 (torch.sigmoid and the kernel's
sigmoid round differently, so bit equality is not expected)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_mae_amd import fcos_inference, fcos_loss, rotated_iou

SIZES, STRIDES, SCENES, EXTENT = ((40,) * 3, (20,) * 3, (10,) * 3, (5,) * 3), (4, 8, 16, 32), 2, 160
CFG = dict(pre_nms_thresh=0.0, pre_nms_top_n=2500, nms_thresh=0.3, fpn_post_nms_top_n=2500, min_size=0.0)


def timed(fn, reps, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(us), min(us)


def make_inputs(use_obb, seed=5):
    rng = np.random.default_rng(seed)
    locs, cls, reg, ctr = [], [], [], []
    for (w, l, h), s in zip(SIZES, STRIDES):
        g = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(l), torch.arange(h), indexing="ij"), -1).reshape(-1, 3)
        locs.append((g * s + s // 2).float().cuda())
        cls.append(torch.from_numpy((rng.standard_normal((SCENES, 1, w, l, h)) - 2.0).astype(np.float32)).cuda())
        ctr.append(torch.from_numpy(rng.standard_normal((SCENES, 1, w, l, h)).astype(np.float32)).cuda())
        d = 0.05 + rng.uniform(0, 4, (SCENES, 6, w, l, h)) * s
        if use_obb:
            d = np.concatenate([d, rng.uniform(-0.45, 0.45, (SCENES, 2, w, l, h))], 1)
        reg.append(torch.from_numpy(d.astype(np.float32)).cuda())
    return locs, cls, reg, ctr, torch.tensor([[EXTENT] * 3] * SCENES, dtype=torch.int32).cuda()


def composition(locs, cls, reg, ctr, sizes_host, use_obb, cfg):
    """the semantics of csrc/fcos_post.hip, step by step, from framework ops"""
    N = cls[0].shape[0]
    per_scene = [[] for _ in range(N)]
    for k, (loc, c, r, t) in enumerate(zip(locs, cls, reg, ctr)):
        n = loc.shape[0]
        p, q = torch.sigmoid(c.reshape(N, n)), torch.sigmoid(t.reshape(N, n))
        s, r = p * q, r.reshape(N, -1, n)
        for b in range(N):
            idx = torch.nonzero(p[b] > cfg["pre_nms_thresh"]).reshape(-1)
            if idx.numel() > cfg["pre_nms_top_n"]:
                idx = idx[torch.topk(s[b][idx], cfg["pre_nms_top_n"], sorted=False).indices].sort().values
            rr, ll = r[b][:, idx].t(), loc[idx]
            if use_obb:
                boxes = fcos_loss.decode_fcos_obb(ll.contiguous(), rr.contiguous())
                sides = boxes[:, 3:6]
            else:
                hi = torch.tensor(list(sizes_host[b]) * 2, dtype=torch.float32, device=ll.device)
                boxes = torch.minimum(torch.cat([ll - rr[:, :3], ll + rr[:, 3:]], 1).clamp_min(0.0), hi)
                sides = boxes[:, 3:] - boxes[:, :3]
            ok = (sides >= cfg["min_size"]).all(1)
            per_scene[b].append((torch.cat([torch.full((int(ok.sum()), 1), float(k), device=ll.device), boxes[ok]], 1), torch.sqrt(s[b][idx][ok])))
    out_b, out_s = [], []
    for b in range(N):
        boxes, scores = torch.cat([x for x, _ in per_scene[b]]), torch.cat([y for _, y in per_scene[b]])
        keep = rotated_iou.nms(boxes[:, 1:].contiguous(), scores, cfg["nms_thresh"])
        boxes, scores = boxes[keep], scores[keep]
        top = cfg["fpn_post_nms_top_n"]
        if scores.numel() > top > 0:
            cut = torch.kthvalue(scores, scores.numel() - top + 1).values
            sel = scores >= cut
            boxes, scores = boxes[sel], scores[sel]
        out_b.append(boxes); out_s.append(scores)
    return out_b, out_s


def main(reps=20):
    assert torch.cuda.is_available(), "bench_fcos_post.py needs an MI355X"
    reps = max(20, reps)
    n_loc = sum(w * l * h for w, l, h in SIZES)
    print(f"FCOS post-processing: {SCENES} scenes x {n_loc} locations (levels {[s[0] for s in SIZES]}^3), cfg {CFG}; {reps} reps, two runs per line")
    for use_obb in (False, True):
        locs, cls, reg, ctr, sizes = make_inputs(use_obb)
        sizes_host = [(EXTENT,) * 3] * SCENES
        fn = fcos_inference.FCOSPostProcessor(CFG["pre_nms_thresh"], CFG["pre_nms_top_n"], CFG["nms_thresh"], CFG["fpn_post_nms_top_n"], CFG["min_size"], 1, False, use_obb)
        dense = lambda: fcos_inference.fcos_postprocess_dense(locs, cls, reg, ctr, sizes, None, CFG["pre_nms_thresh"], CFG["pre_nms_top_n"], CFG["nms_thresh"],   # noqa: E731
                                                              CFG["fpn_post_nms_top_n"], CFG["min_size"], False, use_obb)
        with torch.no_grad():
            fb, fs = fn(locs, cls, reg, ctr, sizes, None)
            cb, cs = composition(locs, cls, reg, ctr, sizes_host, use_obb, CFG)
        same = [len(a) == len(b) and torch.allclose(a, b, rtol=1e-5, atol=0) for a, b in zip(fs, cs)]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            dense()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            dense()
        name = "oriented" if use_obb else "axis-aligned"
        print(f"  {name}: results per scene {[len(x) for x in fs]}, composition {[len(x) for x in cs]}, scores agree to 1e-5 in order: {same}")
        for run in (1, 2):
            with torch.no_grad():
                t = dict(fused=timed(lambda: fn(locs, cls, reg, ctr, sizes, None), reps), dense=timed(dense, reps), graph=timed(graph.replay, reps),
                         composition=timed(lambda: composition(locs, cls, reg, ctr, sizes_host, use_obb, CFG), max(5, reps // 4), warm=1))
            print(f"  {name} run {run}: " + " | ".join(f"{k} median {m:9.1f} us  min {b:9.1f} us" for k, (m, b) in t.items()))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
