"""GPU: nerf_mae_amd.detector.roi_postprocess_dense and filter_proposals (csrc/roi_post.hip) against tests/_roi_post_ref.py, the float64 restatement of the
kernels' stated semantics, and against results recorded from the reference's own filter_proposals (tests/golden/g27_roi_post.npz).

Kept rows, their order, `index` and the counts are compared exactly.  That is defined because every test first asserts, from the restatement and never from
the code under test, that its inputs have a margin of at least 1e-3 on every decision (score threshold, size filter, mesh bounds, suppression, order), four
orders of magnitude above the ~1e-7 fp32 error of a softmax or a decode.  Boxes and scores: the project's contract for fp32, assert_close(rtol=1e-3).
Measured on an MI355X (NMH_PRINT_ERR=1): DESIGN.md 3.20.

The constructed cases (tests/_roi_post_ref.lattice_case) hold their NMS decisions by construction: jittered copies around lattice points, IoU inside a
cluster well above nms_thresh and zero between clusters, plus chains A, B, C across a 64-column block boundary.  tests/test_roi_post_ref_cpu.py asserts the
same margins on the CPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _roi_post_ref as P  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g27_roi_post.npz")
NMS = 0.3
R_SMALL = 130                             # three 64-column blocks, the last partial
COUNTS = (130, 65, 64, 1, 0)
# (seed, K, is_reg, score threshold, mode, counts): the three thresholds in both modes, K = 2 and 3, is_reg on and off, a count of -3 and one of R + 7
SMALL = ((0, 2, True, 0.5, "any", COUNTS), (1, 3, True, 0.3, "any", COUNTS), (32, 3, False, 0.8, "any", COUNTS), (3, 2, False, 0.3, "object", COUNTS),
         (4, 3, True, 0.5, "object", COUNTS), (5, 2, True, 0.8, "object", (R_SMALL + 7, -3, 64, 1, 0)))
LARGE = ((6, 2, True, 0.5, "object", (1500, 1203)),)


def _det():
    from nerf_mae_amd import detector
    return detector


def constructed(rotated, cfg):
    seed, K, is_reg, thr, mode, counts = cfg
    R_ = R_SMALL if len(counts) == len(COUNTS) else 1500
    mesh = (28, 28, 28) if R_ == R_SMALL else (88, 88, 88)          # 27 and 729 lattice points
    inp = P.lattice_case(seed + (100 if rotated else 0), rotated, R_, counts, K, is_reg, mesh, pin=thr)
    return inp, dict(score_thresh=thr, nms_thresh=NMS, min_size=P.MIN_SIZE, is_reg=is_reg, threshold_mode=mode)


@functools.lru_cache(maxsize=None)
def reference(rotated, cfg):
    inp, kw = constructed(rotated, cfg)
    return inp, kw, P.postprocess(**inp, **kw)


def run_gpu(inp, kw, mesh_tensor=True):
    D = _det()
    cu = lambda t: None if t is None else t.cuda()
    N = len(inp["counts"])
    mesh = torch.tensor(inp["mesh_sizes"], dtype=torch.int32).cuda() if mesh_tensor else inp["mesh_sizes"]
    flat = lambda t: None if t is None else t.reshape(-1, t.shape[-1])
    return D.roi_postprocess_dense(cu(flat(inp["pred_scores"])), cu(flat(inp["pred_bbox_deltas"])), cu(flat(inp["rois"])), torch.tensor(inp["counts"], dtype=torch.int32).cuda(),
                                   mesh, **kw), N


def check(out, res, name):
    boxes, scores, index, counts = [t.cpu() for t in out]
    N, R_ = scores.shape
    assert index.dtype == torch.int32 and counts.dtype == torch.int32 and boxes.shape[:2] == (N, R_)
    want = [len(r["scores"]) for r in res]
    assert counts.tolist() == want, f"{name}: counts"
    for i, (r, k) in enumerate(zip(res, want)):
        assert index[i, :k].tolist() == r["index"].tolist(), f"{name}: kept rows and their order, scene {i}"
        assert (index[i, k:] == -1).all() and not boxes[i, k:].any() and not scores[i, k:].any(), f"{name}: rows past the count, scene {i}"
    got_b, got_s = torch.cat([boxes[i, :k] for i, k in enumerate(want)]), torch.cat([scores[i, :k] for i, k in enumerate(want)])
    if got_s.numel():
        assert_close(got_b, torch.cat([r["boxes"] for r in res]), 1e-3, name + " boxes")
        assert_close(got_s, torch.cat([r["scores"] for r in res]), 1e-3, name + " scores")


def margins_ok(m):
    return all(v >= P.MARGIN for v in m.values())


@pytest.mark.parametrize("cfg", SMALL + LARGE, ids=lambda c: f"seed{c[0]}-K{c[1]}-{'reg' if c[2] else 'noreg'}-{c[3]}-{c[4]}-{len(c[5])}x")
@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_against_the_restatement(rotated, cfg):
    inp, kw, (res, m) = reference(rotated, cfg)
    assert margins_ok(m), m
    out, _ = run_gpu(inp, kw)
    check(out, res, f"{rotated} {cfg[:5]}")


@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_the_constructed_edges_are_there(rotated):
    """what the small case is for: chains across a block boundary, the clipped or outside boxes, equal scores, garbage behind the counts"""
    inp, kw, (res, m) = reference(rotated, SMALL[0])
    r0 = res[0]
    ok, boxes, p = r0["cand_ok"], r0["cand_boxes"], r0["cand_p"][:, 1]
    assert int((~ok).sum()) >= (6 if rotated else 2), "rows dropped by the centre test or clipped below min_size"
    order = torch.nonzero(ok).reshape(-1)[torch.sort(p[ok], descending=True, stable=True).indices]
    pos = {int(r): i for i, r in enumerate(order)}
    kept = set(r0["index"].tolist())
    from tests._obb_iou_ref import pairwise
    iou = pairwise(boxes, boxes).tolist()
    chains = 0
    for a in order[:64].tolist():
        for b in order[:64].tolist():
            if pos[b] > pos[a] and iou[a][b] > NMS and a in kept:
                for c in order[64:].tolist():
                    if iou[b][c] > NMS and iou[a][c] < NMS and c in kept:
                        chains += 1
    assert chains >= 3, "A removes B, B would have removed C, which stays, across the first block boundary"
    sc = r0["cand_p"][ok][:, 1]
    assert sc.numel() - sc.unique().numel() >= 2, "exactly equal scores"
    assert inp["pred_scores"][0].shape[0] == R_SMALL and float(inp["pred_scores"][1, 65:, 1].min()) == 9.0, "garbage past the counts would win every sort"


@pytest.mark.parametrize("thr", [0.5, 0.8, 0.3])
@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_recorded_reference_results(rotated, thr):
    """g27 through filter_proposals, the reference's call: probabilities and decoded boxes in, lists out"""
    D = _det()
    g = np.load(GOLDEN)
    pre, tag = "o_" if rotated else "a_", f"_t{int(round(thr * 100))}"
    boxes, probs, mesh = P.gold_inputs(rotated)
    np.testing.assert_allclose(P.input_sums(boxes, probs), g[pre + "input_sums"], rtol=1e-12)
    labels = [torch.arange(b.shape[0]) for b in boxes]
    fb, fs, fl = D.filter_proposals([b.cuda() for b in boxes], [p.cuda() for p in probs], labels, mesh, score_threhold=thr, nms_thresh=float(g["nms_thresh"]), min_size=float(g["min_size"]))
    assert [len(s) for s in fs] == g[pre + "counts" + tag].tolist()
    assert torch.cat(fl).tolist() == g[pre + "index" + tag].tolist()
    assert_close(torch.cat(fb).cpu(), torch.from_numpy(g[pre + "boxes" + tag]), 1e-3, "g27 boxes")
    assert_close(torch.cat(fs).cpu(), torch.from_numpy(g[pre + "probs" + tag]), 1e-3, "g27 probabilities")


@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_two_runs_are_bit_identical_and_a_host_list_of_sizes_is_the_tensor(rotated):
    inp, kw, _ = reference(rotated, SMALL[1])
    a, _ = run_gpu(inp, kw)
    b, _ = run_gpu(inp, kw)
    c, _ = run_gpu(inp, kw, mesh_tensor=False)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    one = dict(inp, mesh_sizes=inp["mesh_sizes"][0])                                  # a single triple for all scenes
    for x, y in zip(a, run_gpu(one, kw, mesh_tensor=False)[0]):
        assert torch.equal(x, y)


@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_capture_and_replay_with_changed_counts(rotated):
    """one capture of roi_postprocess_dense on one stream; between replays the counts change, and no call waits for the host"""
    D = _det()
    inp, kw, (res, m) = reference(rotated, SMALL[0])
    assert margins_ok(m)
    flat = lambda t: t.reshape(-1, t.shape[-1]).cuda()
    args = [flat(inp["pred_scores"]), flat(inp["pred_bbox_deltas"]), flat(inp["rois"])]
    counts = torch.tensor(inp["counts"], dtype=torch.int32).cuda()
    mesh = torch.tensor(inp["mesh_sizes"], dtype=torch.int32).cuda()
    D.roi_postprocess_dense(*args, counts, mesh, **kw)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = D.roi_postprocess_dense(*args, counts, mesh, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    check(eager, res, "eager, no host wait")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        D.roi_postprocess_dense(*args, counts, mesh, **kw)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = D.roi_postprocess_dense(*args, counts, mesh, **kw)
    graph.replay()
    torch.cuda.synchronize()
    check(out, res, "replay 1")
    other = [64, 130, 0, 1, 65]
    res2, m2 = P.postprocess(**dict(inp, counts=other), **kw)
    assert margins_ok(m2), m2
    counts.copy_(torch.tensor(other, dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    check(out, res2, "replay 2, other counts")


def not_finite_case(rotated, cfg):
    """a constructed case with a NaN or an infinity in five rows' deltas (is_reg), RoI or logits -> (inputs, arguments, and the restatement of the same inputs
    with these rows' logits at (30, -30) instead, which the OBJECT threshold drops, and its margins)"""
    inp, kw, _ = reference(rotated, cfg)
    kw = dict(kw, threshold_mode="object")
    inp = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    ref_in = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in inp.items()}
    rows = [(0, 3), (0, 70), (1, 5), (1, 64), (2, 0)]
    bad = [float("nan"), float("inf"), float("-inf"), float("nan"), float("nan")]
    for q, ((b, r), v) in enumerate(zip(rows, bad)):
        if q == 4:
            inp["pred_scores"][b, r, 1] = v                                           # a NaN score
        elif kw["is_reg"] and q % 2 == 0:
            inp["pred_bbox_deltas"][b, r, q % 6] = v
        else:
            inp["rois"][b, r, 1 + (q + 2) % 6] = v
        ref_in["pred_scores"][b, r] = torch.tensor([30.0, -30.0])
    return inp, kw, rows, P.postprocess(**ref_in, **kw)


@pytest.mark.parametrize("cfg", [SMALL[0], SMALL[3]], ids=["reg", "noreg"])
@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_rows_with_a_box_that_is_not_finite_are_dropped(rotated, cfg):
    """the row is dropped, in both box forms, and the other rows' results are those of the restatement without it"""
    inp, kw, rows, (res, m) = not_finite_case(rotated, cfg)
    assert margins_ok(m), m
    assert all(r not in res[b]["index"].tolist() for b, r in rows)
    out, _ = run_gpu(inp, kw)
    assert all(torch.isfinite(t.float()).all() for t in out[:2])
    check(out, res, f"not finite {rotated} {cfg[:5]}")


def test_limits_raise():
    D = _det()
    z = lambda *s: torch.zeros(s, device="cuda")
    c = lambda n: torch.ones(n, dtype=torch.int32, device="cuda")
    ok = lambda: D.roi_postprocess_dense(z(4, 2), z(4, 6), z(4, 7), c(2), (8, 8, 8))
    assert ok()[3].tolist() == [0, 0]                                                # zero boxes have no side >= min_size
    R_ = D.POST_MAX_ROWS + 1
    with pytest.raises(ValueError, match="rows per scene"):
        D.roi_postprocess_dense(z(R_, 2), z(R_, 6), z(R_, 7), c(1), (8, 8, 8))
    with pytest.raises(ValueError, match="classes"):
        D.roi_postprocess_dense(z(4, D.MAX_CLASSES + 1), z(4, 6), z(4, 7), c(2), (8, 8, 8))
    with pytest.raises(ValueError, match="classes"):
        D.roi_postprocess_dense(z(4, 1), z(4, 6), z(4, 7), c(2), (8, 8, 8))
    n = D.MAX_SCENES + 1
    with pytest.raises(ValueError, match="scenes"):
        D.roi_postprocess_dense(z(n, 2), z(n, 6), z(n, 7), c(n), (8, 8, 8))
    with pytest.raises(ValueError, match="workspace"):
        D.roi_postprocess_dense(z(64 * 16384, 2), None, z(64 * 16384, 7), c(64), (8, 8, 8), is_reg=False)
    with pytest.raises(ValueError, match="threshold_mode"):
        D.roi_postprocess_dense(z(4, 2), z(4, 6), z(4, 7), c(2), (8, 8, 8), threshold_mode="both")
    with pytest.raises(ValueError, match="divide"):
        D.roi_postprocess_dense(z(5, 2), z(5, 6), z(5, 7), c(2), (8, 8, 8))
    with pytest.raises(ValueError, match="mesh_sizes"):
        D.roi_postprocess_dense(z(4, 2), z(4, 6), z(4, 7), c(2), [(8, 8, 8)] * 3)
    with pytest.raises(ValueError, match="counts"):
        D.roi_postprocess_dense(z(4, 2), z(4, 6), z(4, 7), [1, 1], (8, 8, 8))
    with pytest.raises(ValueError, match="whole numbers"):
        D.roi_postprocess_dense(z(4, 2), z(4, 6), z(4, 7), c(2), (8, 8.5, 8))
    assert ok()[3].tolist() == D.roi_postprocess_dense(z(4, 2), z(4, 6), z(4, 7), c(2), (8.0, 8.0, 8.0))[3].tolist()
