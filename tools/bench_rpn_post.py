"""RPN proposals at the reference's own workload: mesh 160^3, grids 40^3 / 20^3 / 10^3 / 5^3, 13 anchors per location (950 625 anchors per scene),
pre_nms_top_n = post_nms_top_n = 2500 (cap 9 125), nms_thresh 0.3, axis-aligned and oriented, 1 scene and 4 scenes.
    python tools/bench_rpn_post.py [reps]

Timed with HIP events, median and minimum of `reps` >= 20 calls after 5 warm-up calls, each line in two runs of the loop:
  select / sort / nms   the three stages of rpn_proposals_dense on their own (ops.rpn_post_select, torch.sort of the keys, ops.rpn_post_nms)
  decode                rpn_decode_proposals over all anchors (not part of the fused path: it decodes the selected anchors only)
  dense                 rpn_proposals_dense, eager (no host synchronisation)
  graph                 the dense form replayed from a captured graph
  list                  RPNProposalFilter (one host synchronisation)
  composition           the steps of the semantics (csrc/rpn_post.hip) from framework ops around this project's own pieces: rpn_decode_proposals over all
                        anchors, per level topk and gather, clip / size filter, sigmoid, rotated_iou.nms per level, sort and cut.  Written here from the
                        semantics; it lives in this tool, not in the product.
The composition and the fused op are also compared: the same counts and, in order, the same anchor indices."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_mae_amd import ops, rotated_iou, rpn

MESH, GRIDS = (160,) * 3, ((40,) * 3, (20,) * 3, (10,) * 3, (5,) * 3)
SIZES = ((8,), (16,), (32,), (64,))
RATIOS = (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * 4
PRE, POST, NMS = 2500, 2500, 0.3


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


def make_inputs(N, C, seed=5):
    rng = np.random.default_rng(seed)
    obj = [torch.from_numpy(rng.normal(0, 2.0, (N, 13, *g)).astype(np.float32)).cuda() for g in GRIDS]
    reg = []
    for g in GRIDS:
        d = rng.normal(0, 0.3, (N, 13, C, *g)).astype(np.float32)
        if C == 8:
            d[:, :, :3] = 0.05 * np.abs(d[:, :, :3])          # centres stay inside the mesh
            d[:, :, 6:] *= 0.3
        reg.append(torch.from_numpy(d.reshape(N, 13 * C, *g)).cuda())
    return obj, reg


def composition(gen, obj, reg, rotated):
    N = obj[0].shape[0]
    dec = rpn.rpn_decode_proposals(gen, MESH, reg, rotated=rotated)
    hi = torch.tensor(MESH * 2, dtype=torch.float32, device=dec.device)
    out, off = [], 0
    per = [[] for _ in range(N)]
    for k, o in enumerate(obj):
        A, nloc = o.shape[1], o[0, 0].numel()
        flat = o.reshape(N, A * nloc)
        top = torch.topk(flat, min(PRE, flat.shape[1]), dim=1).indices
        anchor = off + (top % nloc) * A + top // nloc
        for b in range(N):
            boxes, logit = dec[b][anchor[b]], flat[b][top[b]]
            if rotated:
                ok = ((boxes[:, :3] >= 0) & (boxes[:, :3] <= hi[:3])).all(1) & (boxes[:, 3:6] >= 1e-3).all(1)
            else:
                boxes = torch.minimum(boxes.clamp_min(0.0), hi)
                ok = (boxes[:, 3:] - boxes[:, :3] >= 1e-3).all(1)
            boxes, logit, idx = boxes[ok], logit[ok], anchor[b][ok]
            keep = rotated_iou.nms(boxes.contiguous(), logit, NMS)
            per[b].append((boxes[keep], logit[keep], idx[keep]))
        off += A * nloc
    for b in range(N):
        boxes, logit, idx = (torch.cat([p[i] for p in per[b]]) for i in range(3))
        order = torch.sort(logit, descending=True, stable=True).indices[:POST]
        out.append((boxes[order], torch.sigmoid(logit[order]), idx[order]))
    return out


def main(reps=20):
    assert torch.cuda.is_available(), "bench_rpn_post.py needs an MI355X"
    reps = max(20, reps)
    gen = rpn.AnchorGenerator3D(SIZES, RATIOS)
    print(f"RPN proposals: mesh {MESH[0]}^3, grids {[g[0] for g in GRIDS]}^3 x 13 anchors, pre/post {PRE}/{POST}, nms {NMS}; {reps} reps, two runs per line")
    for rotated in (False, True):
        for N in (1, 4):
            C = 8 if rotated else 6
            obj, reg = make_inputs(N, C)
            dense = lambda: rpn.rpn_proposals_dense(gen, MESH, obj, reg, None, PRE, POST, NMS, rotated=rotated)      # noqa: E731
            fn = rpn.RPNProposalFilter(gen, PRE, POST, NMS, rotated_bbox=rotated)
            post, _, sel = rpn._select("bench", gen, MESH, obj, reg, None, PRE, 0.0, 1e-3, rotated)
            keys, pre_boxes, pre_scores, pre_index, pre_counts = sel
            skeys, order = torch.sort(keys, dim=1, descending=True, stable=True)
            out = dense()
            comp = composition(gen, obj, reg, rotated)
            same = [int(out[4][b]) == len(comp[b][2]) and torch.equal(out[3][b, :len(comp[b][2])].long(), comp[b][2].long()) for b in range(N)]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                dense()
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
                dense()
            name = f"{'oriented' if rotated else 'axis-aligned'} N={N}"
            print(f"  {name}: cap {post.cap}, results per scene {out[4].tolist()}, composition agrees in counts and anchor order: {same}")
            for run in (1, 2):
                t = dict(select=timed(lambda: rpn._select("bench", gen, MESH, obj, reg, None, PRE, 0.0, 1e-3, rotated), reps),
                         sort=timed(lambda: torch.sort(keys, dim=1, descending=True, stable=True), reps),
                         nms=timed(lambda: ops.rpn_post_nms(post, C, pre_boxes, pre_scores, pre_index, skeys, order, pre_counts, NMS, POST), reps),
                         decode=timed(lambda: rpn.rpn_decode_proposals(gen, MESH, reg, rotated=rotated), reps),
                         dense=timed(dense, reps), graph=timed(graph.replay, reps), list=timed(lambda: fn(MESH, obj, reg), reps),
                         composition=timed(lambda: composition(gen, obj, reg, rotated), max(5, reps // 4), warm=1))
                print(f"  {name} run {run}: " + " | ".join(f"{k} {m:8.1f}/{b:8.1f}" for k, (m, b) in t.items()) + "   (median/min us)")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
