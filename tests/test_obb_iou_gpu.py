"""Oriented 3-D box IoU / GIoU / DIoU losses (values and gradients), all-pairs IoU and rotated NMS on the GPU, against the values and gradients
recorded from the reference's own Python (tests/golden/g17_obb_iou.npz) and against the float64 restatement of tests/_obb_iou_ref.py
(itself checked in tests/test_obb_iou_cpu.py).

Tolerance: the project's contract for fp32, assert_close(rtol=1e-3).  On this generator the reference run in fp32 and in float64 agree to
3e-7 (IoU), 1.1e-6 (IoU gradient), 2.1e-5 (GIoU gradient) and 7.4e-6 (DIoU gradient) in the max norm, so the bound has two orders of
magnitude of margin and NO pair is left out of any comparison.  NMS results are compared exactly; that is defined only when no IoU sits on
the threshold, which the test asserts on the float64 matrix (margin 1e-5, against an fp32 IoU error of about 1e-7).
Measured on an MI355X (NMH_PRINT_ERR=1): see DESIGN.md 3.8."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _obb_iou_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (1, 1000), (3, 333))
NMS_SEED = 47          # base seed of R.make_clusters: no float64 IoU within 1e-5 of 0.1 or 0.5 at any N below (checked on the host)
NMS_SIZES = (1, 63, 64, 65, 200, 1000)


def _m():
    from nerf_mae_amd import rotated_iou
    return rotated_iou


def _call(M, mode, p, q):
    """-> (iou, loss or None, giou or None)"""
    if mode == "iou":
        return M.cal_iou_3d(p, q), None, None
    kind, enc = mode.split("_")
    if kind == "giou":
        loss, giou, iou = M.cal_giou_3d(p, q, enclosing_type=enc)
        return iou, loss, giou
    loss, iou = M.cal_diou_3d(p, q, enclosing_type=enc)
    return iou, loss, None


@functools.lru_cache(maxsize=None)
def pairs(shape):
    rng = np.random.default_rng(100 + shape[0] * 7 + shape[1])
    n = shape[0] * shape[1]
    return (torch.from_numpy(R.make_boxes(rng, n)).reshape(*shape, 7), torch.from_numpy(R.make_boxes(rng, n)).reshape(*shape, 7))


@functools.lru_cache(maxsize=None)
def ref_case(shape, mode):
    """float64 values, and gradients of (iou a + u3d b).sum() [+ (loss c).sum()] with respect to both boxes, for fixed random a, b, c"""
    b1, b2 = pairs(shape)
    g = torch.Generator().manual_seed(shape[1])
    a, b, c = (torch.randn(shape, generator=g) for _ in range(3))
    p, q = b1.double().requires_grad_(True), b2.double().requires_grad_(True)
    r = R.paired(p, q, mode)
    obj = (r["iou"] * a.double() + r["u3d"] * b.double()).sum()
    if mode != "iou":
        obj = obj + (r["loss"] * c.double()).sum()
    obj.backward()
    return {k: v.detach() for k, v in r.items()}, (a, b, c), p.grad, q.grad


# ---- 1. against the recorded reference -------------------------------------------------------------------------------------------------
def test_values_and_gradients_against_the_recorded_reference():
    M = _m()
    g = np.load(os.path.join(ROOT, "tests", "golden", "g17_obb_iou.npz"))
    for name, mode in (("iou", "iou"), ("giou_loss", "giou_smallest"), ("diou_loss", "diou_smallest")):
        p = torch.from_numpy(g["box1"])[None].cuda().requires_grad_(True)
        q = torch.from_numpy(g["box2"])[None].cuda().requires_grad_(True)
        iou, loss, _ = _call(M, mode, p, q)
        v = iou if mode == "iou" else loss
        v.sum().backward()
        assert_close(iou[0].cpu(), torch.from_numpy(g["iou"]), 1e-3, f"g17 iou ({mode})")
        assert_close(v[0].cpu(), torch.from_numpy(g[name]), 1e-3, f"g17 {name}")
        assert_close(p.grad[0].cpu(), torch.from_numpy(g[f"grad_{name}_box1"]), 1e-3, f"g17 grad_{name}_box1")
        assert_close(q.grad[0].cpu(), torch.from_numpy(g[f"grad_{name}_box2"]), 1e-3, f"g17 grad_{name}_box2")


# ---- 2. values and gradients against float64, all five modes ----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("mode", R.MODES)
def test_values_and_gradients_against_float64(shape, mode):
    M = _m()
    b1, b2 = pairs(shape)
    r, (a, b, c), g1, g2 = ref_case(shape, mode)
    p, q = b1.cuda().requires_grad_(True), b2.cuda().requires_grad_(True)
    if mode == "iou":
        iou, c1, c2, zr, u3d = M.cal_iou_3d(p, q, verbose=True)
        assert not zr.requires_grad and not c1.requires_grad and not c2.requires_grad
        assert_close(zr.cpu(), r["z_range"], 1e-3, "z_range")
        assert_close(c1.cpu(), r["corners1"], 1e-3, "corners1")
        assert_close(c2.cpu(), r["corners2"], 1e-3, "corners2")
        k = shape[1] // 2
        want = R.rect_corners(*(float(b1[0, k, j]) for j in (0, 1, 3, 4, 6)))
        assert np.abs(c1[0, k].cpu().numpy() - want).max() < 1e-5
        assert torch.equal(M.cal_iou_3d(p, q), iou)
        loss = None
    else:
        iou, loss, giou = _call(M, mode, p, q)
        u3d = M.cal_iou_3d(p, q, verbose=True)[4]
        assert_close(loss.detach().cpu(), r["loss"], 1e-3, f"{mode} loss")
        if giou is not None:
            assert_close(giou.detach().cpu(), 1.0 - r["loss"], 1e-3, "giou")
    assert iou.shape == shape and u3d.shape == shape
    assert_close(iou.detach().cpu(), r["iou"], 1e-3, "iou")
    assert_close(u3d.detach().cpu(), r["u3d"], 1e-3, "u3d")
    obj = (iou * a.cuda() + u3d * b.cuda()).sum()
    if loss is not None:
        obj = obj + (loss * c.cuda()).sum()
    obj.backward()
    assert_close(p.grad.cpu(), g1, 1e-3, f"{mode} dbox1")
    assert_close(q.grad.cpu(), g2, 1e-3, f"{mode} dbox2")


def test_gradient_goes_only_where_it_is_required():
    M = _m()
    b1, b2 = pairs((3, 333))
    _, (a, b, c), g1, g2 = ref_case((3, 333), "diou_smallest")
    for side in (0, 1):
        p, q = b1.cuda().requires_grad_(side == 0), b2.cuda().requires_grad_(side == 1)
        loss, iou = M.cal_diou_3d(p, q)
        u3d = M.cal_iou_3d(p, q, verbose=True)[4]
        ((iou * a.cuda() + u3d * b.cuda()).sum() + (loss * c.cuda()).sum()).backward()
        assert (q if side == 0 else p).grad is None
        assert_close((p if side == 0 else q).grad.cpu(), g1 if side == 0 else g2, 1e-3, f"one-sided dbox{side + 1}")


def test_no_bev_overlap_gives_an_exactly_zero_iou_gradient():
    M = _m()
    b1, b2 = pairs((1, 1000))
    r = ref_case((1, 1000), "iou")[0]
    apart = r["inter2d"] == 0
    frac = apart.double().mean().item()
    assert 0.05 <= frac <= 0.40, frac
    p, q = b1.cuda().requires_grad_(True), b2.cuda().requires_grad_(True)
    iou = M.cal_iou_3d(p, q)
    assert (iou.detach().cpu()[apart] == 0).all()
    (iou * torch.randn_like(iou)).sum().backward()
    assert (p.grad.cpu()[apart] == 0).all() and (q.grad.cpu()[apart] == 0).all()
    assert (p.grad.cpu()[r["iou"] > 0].abs().sum(-1) > 0).all()


def test_through_the_reference_loss_form():
    """RotatedIOULoss of the reference: -log((ious * unions + 1) / (unions + 1))"""
    M = _m()
    b1, b2 = pairs((1, 1000))
    p, t = b1[0].cuda().requires_grad_(True), b2[0].cuda()
    ious, _, _, _, unions = M.cal_iou_3d(p[None], t[None], verbose=True)
    ((ious * unions + 1) / (unions + 1)).log().neg().sum().backward()
    pr = b1[0].double().requires_grad_(True)
    r = R.paired(pr[None], b2[0].double()[None])
    want = ((r["iou"] * r["u3d"] + 1) / (r["u3d"] + 1)).log().neg()
    want.sum().backward()
    assert_close(((ious * unions + 1) / (unions + 1)).log().neg().detach().cpu(), want.detach(), 1e-3, "rotated iou loss")
    assert_close(p.grad.cpu(), pr.grad, 1e-3, "rotated iou loss dbox")


# ---- 3. edges ---------------------------------------------------------------------------------------------------------------------------
def test_empty_input():
    M = _m()
    p = torch.zeros((2, 0, 7), device="cuda", requires_grad=True)
    q = torch.zeros((2, 0, 7), device="cuda", requires_grad=True)
    for mode in R.MODES:
        iou, loss, _ = _call(M, mode, p, q)
        assert iou.shape == (2, 0) and (loss is None or loss.shape == (2, 0))
        (iou.sum() if loss is None else (iou.sum() + loss.sum())).backward()
    assert p.grad.shape == (2, 0, 7) and q.grad.shape == (2, 0, 7)
    assert p.grad.abs().sum().item() == 0 and q.grad.abs().sum().item() == 0
    iou, c1, c2, zr, u3d = M.cal_iou_3d(p, q, verbose=True)
    assert c1.shape == (2, 0, 4, 2) and zr.shape == (2, 0) and u3d.shape == (2, 0)
    assert M.box_iou_3d(p[0], torch.zeros((5, 7), device="cuda")).shape == (0, 5)
    assert M.box_iou_3d(torch.zeros((5, 7), device="cuda"), p[0]).shape == (5, 0)


def test_identical_boxes():
    """the stated deviation: IoU of a box with itself is >= 1 - 1e-4"""
    M = _m()
    b = torch.from_numpy(R.make_boxes(np.random.default_rng(5), 256))[None].cuda()
    iou = M.cal_iou_3d(b, b.clone())
    assert iou.min().item() >= 1 - 1e-4 and iou.max().item() <= 1 + 1e-6, (iou.min().item(), iou.max().item())
    d = M.box_iou_3d(b[0], b[0]).diagonal()
    assert d.min().item() >= 1 - 1e-4


def test_axis_aligned_pairs_match_the_closed_form():
    M = _m()
    rng = np.random.default_rng(6)
    n = 300
    b1, b2 = R.make_boxes(rng, n), R.make_boxes(rng, n)
    quarter = rng.integers(0, 2, (2, n)).astype(bool)
    b1[:, 6] = np.where(quarter[0], np.float32(math.pi / 2), np.float32(0))
    b2[:, 6] = np.where(quarter[1], np.float32(math.pi / 2), np.float32(0))

    def aabb(b, turned):
        w, l = np.where(turned, b[:, 4], b[:, 3]).astype(np.float64), np.where(turned, b[:, 3], b[:, 4]).astype(np.float64)
        c, h = b[:, :3].astype(np.float64), b[:, 5].astype(np.float64)
        half = np.stack([w, l, h], 1) / 2
        return torch.from_numpy(np.concatenate([c - half, c + half], 1))
    a1, a2 = aabb(b1, quarter[0]), aabb(b2, quarter[1])
    inter = (torch.minimum(a1[:, 3:], a2[:, 3:]) - torch.maximum(a1[:, :3], a2[:, :3])).clamp_min(0).prod(-1)
    want = inter / ((a1[:, 3:] - a1[:, :3]).prod(-1) + (a2[:, 3:] - a2[:, :3]).prod(-1) - inter)
    got = M.cal_iou_3d(torch.from_numpy(b1)[None].cuda(), torch.from_numpy(b2)[None].cuda())[0].cpu().double()
    assert (want > 0).double().mean() > 0.5
    assert (got - want).abs().max().item() < 1e-5, (got - want).abs().max().item()


def test_box_inside_box_and_touching_in_z():
    M = _m()
    rng = np.random.default_rng(8)
    big = R.make_boxes(rng, 100)
    small = big.copy()
    small[:50, 3:6] *= rng.uniform(0.2, 0.6, (50, 3)).astype(np.float32)       # same centre and angle, every size smaller
    side = 0.4 * np.minimum(big[50:, 3], big[50:, 4])                           # a square whose diagonal (0.57 min) fits at any angle
    small[50:, 3], small[50:, 4], small[50:, 5] = side, side, 0.5 * big[50:, 5]
    small[50:, 6] = rng.uniform(-math.pi, math.pi, 50).astype(np.float32)
    got = M.cal_iou_3d(torch.from_numpy(small)[None].cuda(), torch.from_numpy(big)[None].cuda())[0].cpu().double()
    want = torch.from_numpy(small[:, 3:6].astype(np.float64).prod(1) / big[:, 3:6].astype(np.float64).prod(1))
    assert ((got - want).abs() <= 1e-5 * want + 1e-6).all(), (got - want).abs().max().item()
    # touching only in z: same BEV rectangle, z ranges [-(h/2), h/2] and [h/2, 3h/2] with h a power of two (exact)
    a = torch.tensor([[[0.0, 0, 0, 2, 1, 2, 0.3], [1.0, 1, 1, 1, 3, 0.5, -1.0]]], device="cuda")
    b = a.clone()
    b[..., 2] += a[..., 5]
    assert (M.cal_iou_3d(a, b) == 0).all()
    assert (M.box_iou_3d(a[0], b[0]).diagonal() == 0).all()


# ---- 4. all pairs ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nm", ((1, 1), (37, 129), (200, 300)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_pairwise(nm):
    M = _m()
    rng = np.random.default_rng(nm[0] + nm[1])
    b1, b2 = torch.from_numpy(R.make_boxes(rng, nm[0])), torch.from_numpy(R.make_boxes(rng, nm[1]))
    b1[:, :3] *= 2.5                                   # spread the centres so that a good part of the pairs does not overlap
    b2[:, :3] *= 2.5
    want = R.pairwise(b1.double(), b2.double())
    got = M.box_iou_3d(b1.cuda(), b2.cuda())
    assert got.shape == nm and got.dtype == torch.float32 and got.is_cuda
    got = got.cpu()
    assert_close(got, want, 1e-3, f"pairwise {nm}")
    assert (got[want == 0] == 0).all()
    if nm[0] > 1:
        assert 0.1 < (want == 0).double().mean().item() < 0.9
        sym = M.box_iou_3d(b2.cuda(), b2.cuda()).cpu()
        assert (sym - sym.T).abs().max().item() <= 1e-6


def test_pairwise_axis_aligned_form():
    M = _m()
    rng = np.random.default_rng(9)
    lo1, lo2 = rng.uniform(0, 4, (70, 3)), rng.uniform(0, 4, (131, 3))
    b1 = torch.from_numpy(np.concatenate([lo1, lo1 + rng.uniform(0.3, 2.5, (70, 3))], 1).astype(np.float32))
    b2 = torch.from_numpy(np.concatenate([lo2, lo2 + rng.uniform(0.3, 2.5, (131, 3))], 1).astype(np.float32))
    want = R.pairwise(b1.double(), b2.double())
    got = M.box_iou_3d(b1.cuda(), b2.cuda()).cpu()
    assert_close(got, want, 1e-3, "pairwise 6-column")
    assert (got[want == 0] == 0).all() and 0.1 < (want == 0).double().mean().item() < 0.9


# ---- 5. NMS ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def nms_case(n):
    boxes, scores = R.make_clusters(NMS_SEED + n, n)
    return boxes, scores, R.pairwise(boxes.double(), boxes.double())


@pytest.mark.parametrize("n", NMS_SIZES)
def test_nms_equals_the_greedy_reference(n):
    M = _m()
    boxes, scores, iou = nms_case(n)
    upper = iou[torch.triu(torch.ones(n, n, dtype=torch.bool), 1)]
    for thr in (0.1, 0.5):
        assert n == 1 or (upper - thr).abs().min().item() > 1e-5     # no pair on the threshold: the outcome is defined
        got = M.nms(boxes.cuda(), scores.cuda(), thr)
        assert got.dtype == torch.int64 and got.is_cuda
        want = R.nms(iou, scores, thr)
        assert got.cpu().tolist() == want, (n, thr)
        if n >= 200:
            assert 3 < len(want) < n - 3
    if n == 1000:       # suppression must have crossed 64-bit word boundaries of the score order
        order = torch.sort(scores, descending=True, stable=True).indices
        s = iou[order][:, order] > 0.5
        i, j = torch.nonzero(torch.triu(s, 1), as_tuple=True)
        assert ((j // 64) - (i // 64)).max().item() >= 8


def test_nms_ties_go_to_the_lower_index():
    M = _m()
    boxes, _, iou = nms_case(200)
    scores = torch.full((200,), 0.5)
    scores[100:] = 0.75
    for thr in (0.1, 0.5):
        assert M.nms(boxes.cuda(), scores.cuda(), thr).cpu().tolist() == R.nms(iou, scores, thr)


def test_batched_nms_and_empty():
    M = _m()
    boxes, scores, iou = nms_case(200)
    cats = torch.arange(200) % 3
    for thr in (0.1, 0.5):
        got = M.batched_nms(boxes.cuda(), scores.cuda(), cats.cuda(), thr)
        assert got.dtype == torch.int64 and got.is_cuda
        per = []
        for c in range(3):
            idx = torch.nonzero(cats == c)[:, 0]
            per += idx[M.nms(boxes[idx].cuda(), scores[idx].cuda(), thr).cpu()].tolist()
        per.sort(key=lambda i: -scores[i].item())
        assert got.cpu().tolist() == per == R.nms(iou, scores, thr, cats=cats.tolist())
        assert len(per) > len(R.nms(iou, scores, thr))
    e = M.nms(torch.zeros((0, 7), device="cuda"), torch.zeros((0,), device="cuda"), 0.5)
    assert e.shape == (0,) and e.dtype == torch.int64 and e.is_cuda
    assert M.batched_nms(torch.zeros((0, 7), device="cuda"), torch.zeros((0,), device="cuda"), torch.zeros((0,), dtype=torch.long, device="cuda"), 0.5).shape == (0,)
    ab = torch.tensor([[0.0, 0, 0, 2, 2, 2], [0.2, 0, 0, 2.2, 2, 2], [5.0, 5, 5, 6, 6, 6]], device="cuda")
    assert M.nms(ab, torch.tensor([0.5, 0.9, 0.1], device="cuda"), 0.5).cpu().tolist() == [1, 2]
    with pytest.raises(ValueError):
        M.nms(torch.zeros((M.NMS_MAX_BOXES + 1, 7), device="cuda"), torch.zeros((M.NMS_MAX_BOXES + 1,), device="cuda"), 0.5)


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------
def _capture_and_replay(run, make_leaves):
    """run(p, q) -> tuple of tensors.  Eager on leaves of its own; then leaves made, warmed up and captured on ONE side stream in
    thread-local mode (trainer.GraphedTrainStep's recipe); outputs zeroed, one replay -> (eager, replayed).
    The leaves must be created on the capture stream and no earlier autograd graph over them may be alive: autograd remembers the stream
    on which a leaf's gradient-accumulation node was made and joins that stream to the backward's stream; if it is another stream (the
    default one, from an eager run kept alive by its results), that join is pulled into the capture as a branch which never rejoins."""
    eager = run(*make_leaves())
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        p, q = make_leaves()
        run(p, q)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(p, q)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    return eager, out


def test_diou_forward_backward_in_a_captured_graph():
    M = _m()
    b1, b2 = pairs((1, 1000))
    b1, b2 = b1[:, :256].cuda(), b2[:, :256].cuda()

    def run(p, q):
        loss, iou = M.cal_diou_3d(p, q)
        return (loss.detach(), iou.detach()) + torch.autograd.grad(loss.sum(), (p, q))
    eager, out = _capture_and_replay(run, lambda: (b1.clone().requires_grad_(True), b2.clone().requires_grad_(True)))
    assert len(out) == 4 and all(torch.equal(a, b) for a, b in zip(out, eager))
    assert eager[2].abs().sum().item() > 0 and eager[3].abs().sum().item() > 0


def test_diou_backward_into_grad_in_a_captured_graph():
    """.backward() accumulating into .grad inside the capture, the form a training step uses: the warm-up creates .grad, the capture adds to
    it in place, so .grad is cleared before the replay"""
    M = _m()
    b1, b2 = pairs((1, 1000))
    b1, b2 = b1[:, :256].cuda(), b2[:, :256].cuda()
    leaves = []

    def make():
        leaves.append((b1.clone().requires_grad_(True), b2.clone().requires_grad_(True)))
        return leaves[-1]

    def run(p, q):
        loss, iou = M.cal_diou_3d(p, q)
        loss.sum().backward()
        return loss.detach(), iou.detach(), p.grad, q.grad
    eager, out = _capture_and_replay(run, make)          # _capture_and_replay zeroes `out`, .grad included, before the replay
    assert out[2] is leaves[1][0].grad and all(torch.equal(a, b) for a, b in zip(out, eager))
    assert eager[2].abs().sum().item() > 0


def test_the_two_launches_in_a_captured_graph():
    """the forward and backward C-ABI launches alone, without autograd"""
    ops = M_ops()
    b1, b2 = pairs((1, 1000))
    b1, b2 = b1[:, :256].cuda(), b2[:, :256].cuda()
    g = torch.randn((1, 256), device="cuda")

    def run(p, q):
        iou, u3d, _, loss, _, _ = ops.obb_iou_fwd(ops.OBB_DIOU_SMALLEST, p, q)
        return (iou, u3d, loss) + ops.obb_iou_bwd(ops.OBB_DIOU_SMALLEST, p, q, g, None, g, True, True)
    eager, out = _capture_and_replay(run, lambda: (b1, b2))
    assert len(out) == 5 and all(torch.equal(a, b) for a, b in zip(out, eager))


def M_ops():
    from nerf_mae_amd import ops
    return ops
