"""FCOS inference post-processing on the GPU (nerf_mae_amd.fcos_inference over csrc/fcos_post.hip) against the float64 restatement of
tests/_fcos_post_ref.py (itself checked against the recorded reference in tests/test_fcos_post_ref_cpu.py) and against the recorded
reference (tests/golden/g19_fcos_post.npz) directly.

Kept sets, levels and order are compared exactly.  That is defined because every test first asserts, from the restatement and never from
the code under test, that its inputs have a margin of at least 1e-5 on every decision (threshold, top-k cut, size filter, suppression,
post-NMS cut, order), about 100x the ~1e-7 fp32 error of a sigmoid product.  Boxes and scores: the project's contract for fp32,
assert_close(rtol=1e-3).  Measured on an MI355X (NMH_PRINT_ERR=1): DESIGN.md 3.10.

Head seeds per configuration come from tools/gen_golden_fcos_post.py --search and its like: a seed is accepted on the restatement's margins."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_post_ref as P  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "g19_fcos_post.npz")

# (use_obb, pre_nms_thresh, min_size, masks, fpn_post_nms_top_n, bbox_aug_enabled) -> (head seed, graded scores) with every margin >= 1e-5.
# Without the post-NMS cut a scene has 400 to 650 results; random scores leave no margin on the order of that many (the smallest relative gap
# of 600 random scores is about 1e-6), so those two cases take the graded scores of _fcos_post_ref.inputs.
CASES = {
    (False, 0.05, 2.0, True, 100, False): (1804, False),       # the recorded configuration
    (True, 0.05, 2.0, True, 100, False): (1825, False),
    (False, 0.0, 0.0, False, 0, False): (1800, True),
    (True, 0.0, 0.0, False, 0, False): (1801, True),
    (False, 0.05, 2.0, True, 100, True): (1804, False),
    (True, 0.0, 0.0, False, 100, True): (1801, True),
}


def _m():
    from nerf_mae_amd import fcos_inference
    return fcos_inference


def _cfg(thr, min_size, post, top_n=300, nms=0.3):
    return dict(pre_nms_thresh=thr, pre_nms_top_n=top_n, nms_thresh=nms, fpn_post_nms_top_n=post, min_size=min_size)


@functools.lru_cache(maxsize=None)
def ref_case(use_obb, thr, min_size, masks, post, aug):
    seed, graded = CASES[(use_obb, thr, min_size, masks, post, aug)]
    inp = P.inputs(seed, use_obb, masks=masks, graded=graded)
    res, marg = P.postprocess(*inp, **_cfg(thr, min_size, post), bbox_aug_enabled=aug)
    return inp, res, marg


def to_gpu(inp, sizes_as_list=False):
    locs, cls, reg, ctr, sizes, masks = inp
    g = lambda ts: [t.float().cuda() for t in ts]       # noqa: E731
    sizes = sizes if sizes_as_list or sizes is None else torch.tensor(sizes, dtype=torch.int32).cuda()
    return g(locs), g(cls), g(reg), g(ctr), sizes, (None if masks is None else [m.cuda() for m in masks])


def run_gpu(inp, cfg, use_obb, aug=False):
    fn = _m().FCOSPostProcessor(cfg["pre_nms_thresh"], cfg["pre_nms_top_n"], cfg["nms_thresh"], cfg["fpn_post_nms_top_n"], cfg["min_size"], 1, aug, use_obb)
    boxes, scores = fn(*to_gpu(inp))
    torch.cuda.synchronize()
    return boxes, scores


def check(res, boxes, scores, name):
    """kept sets, levels and order equal; boxes and scores within the fp32 contract"""
    assert len(boxes) == len(scores) == len(res)
    assert [len(s) for s in scores] == [len(r["scores"]) for r in res], name
    for b, s, r in zip(boxes, scores, res):
        assert b.dtype == torch.float32 and s.dtype == torch.float32 and b.shape == (len(r["scores"]), 1 + r["pre_boxes"].shape[1]) and not b.requires_grad
        assert b[:, 0].cpu().tolist() == r["level"].double().tolist(), name
    got_b, got_s = torch.cat([b[:, 1:] for b in boxes]).cpu(), torch.cat(scores).cpu()
    ref_b, ref_s = torch.cat([r["boxes"] for r in res]), torch.cat([r["scores"] for r in res])
    if ref_s.numel():
        # a wrong box in a right slot is an error of the size of a box, far above 1e-3 of the largest coordinate: order and identity are checked by this too
        assert_close(got_b, ref_b, 1e-3, name + " boxes")
        assert_close(got_s, ref_s, 1e-3, name + " scores")


def margins_ok(marg, skip=()):
    bad = {k: v for k, v in marg.items() if k not in skip and v < P.MARGIN}
    assert not bad, bad


# ---- 1. the configurations on the recorded geometry -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES), ids=lambda c: "-".join(str(v) for v in c))
def test_configurations_against_the_restatement(case):
    use_obb, thr, min_size, masks, post, aug = case
    inp, res, marg = ref_case(*case)
    margins_ok(marg)
    check(res, *run_gpu(inp, _cfg(thr, min_size, post), use_obb, aug), name=str(case))
    if not aug:
        assert all(len(r["pre_scores"]) > len(r["scores"]) > 0 for r in res)          # NMS does real work


@pytest.mark.parametrize("use_obb", [False, True], ids=["aabb", "obb"])
def test_against_the_recorded_reference(use_obb):
    g, pre = np.load(GOLDEN), "o_" if use_obb else "a_"
    case = (use_obb, 0.05, 2.0, True, 100, False)
    inp, _, marg = ref_case(*case)
    margins_ok(marg)
    boxes, scores = run_gpu(inp, P.CFG, use_obb)
    assert [len(s) for s in scores] == g[pre + "counts"].tolist()
    assert torch.cat([b[:, 0] for b in boxes]).cpu().tolist() == g[pre + "level"].astype(np.float64).tolist()
    assert_close(torch.cat([b[:, 1:] for b in boxes]).cpu(), torch.from_numpy(g[pre + "boxes"]), 1e-3, "g19 boxes")
    assert_close(torch.cat(scores).cpu(), torch.from_numpy(g[pre + "scores"]), 1e-3, "g19 scores")


# ---- 2. edges of the selection, on crafted inputs ---------------------------------------------------------------------------------------------
def crafted(sizes, counts, seed, use_obb=False, stride0=8, equal=False):
    """levels of the given feature sizes; counts[level][scene] candidates per (level, scene) at random locations, their logits a shuffled grid
    over about [0, 3] (another grid per level; relative score gaps far above the margin; `equal`: all 1.0), every other location at logit -10 (p = 4.5e-5, no candidate at
    pre_nms_thresh 0.05); centerness logit 0; boxes of side 1 to 3 around locations `stride` apart, so that none overlap."""
    rng = np.random.default_rng(seed)
    N = len(counts[0])
    locs, cls, reg, ctr = [], [], [], []
    for k, ((w, l, h), cnt) in enumerate(zip(sizes, counts)):
        n, stride = w * l * h, stride0 << k                # level k's locations sit between those of level k - 1
        g = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(l), torch.arange(h), indexing="ij"), -1).reshape(-1, 3)
        locs.append((g * stride + stride // 2).float())
        x = np.full((N, n), -10.0)
        for b, m in enumerate(cnt):
            x[b, rng.permutation(n)[:m]] = 1.0 if equal else rng.permutation(np.linspace(0.1 * k, 3.0 - 0.13 * k, max(m, 1)))[:m]
        cls.append(torch.from_numpy(x.astype(np.float32)).reshape(N, 1, w, l, h))
        ctr.append(torch.zeros((N, 1, w, l, h)))
        d = rng.uniform(0.5, 1.5, (N, 6, w, l, h))
        if use_obb:
            d = np.concatenate([d, rng.uniform(-0.4, 0.4, (N, 2, w, l, h))], 1)
        reg.append(torch.from_numpy(d.astype(np.float32)))
    size = tuple(int(max(s[a] << k for k, s in enumerate(sizes)) * stride0) for a in range(3))
    return locs, cls, reg, ctr, [size] * N, None


EDGES = {
    # name: (sizes, counts[level][scene], cfg overrides, margins that the case is about and that are therefore not asserted)
    "one-location-level": (((3, 3, 3), (1, 1, 1)), ((20, 27, 0), (1, 0, 1)), dict(top_n=16), ()),
    "around-64": (((10, 6, 5),), ((63, 64, 65),), dict(top_n=64), ()),
    "around-256": (((10, 6, 5),), ((255, 256, 257),), dict(top_n=256), ()),
    "empty-level-scene": (((10, 6, 5), (4, 4, 4)), ((0, 0, 40), (30, 0, 64)), dict(top_n=32), ()),
    "empty-everywhere": (((10, 6, 5), (4, 4, 4)), ((0, 0), (0, 0)), dict(top_n=32), ()),
    "all-too-small": (((10, 6, 5),), ((40, 100),), dict(top_n=64, min_size=5.0), ()),
    "all-equal": (((10, 6, 5), (4, 4, 4)), ((300, 100, 64), (64, 3, 0)), dict(top_n=64, equal=True), ("m_topk", "m_order", "m_post")),
    "all-equal-cut": (((10, 6, 5),), ((300, 10),), dict(top_n=64, equal=True, post=7), ("m_topk", "m_order", "m_post")),
}


@pytest.mark.parametrize("use_obb", [False, True], ids=["aabb", "obb"])
@pytest.mark.parametrize("name", sorted(EDGES))
def test_selection_edges(name, use_obb):
    sizes, counts, over, skip = EDGES[name]
    over = dict(over)
    equal = over.pop("equal", False)
    inp = crafted(sizes, counts, 7, use_obb, equal=equal)
    cfg = _cfg(0.05, over.pop("min_size", 0.0), over.pop("post", 0), **over)
    res, marg = P.postprocess(*inp, **cfg)
    margins_ok(marg, skip)
    # the condition on the input, checked here on the CPU: the candidate counts are what the case is about
    for k, cnt in enumerate(counts):
        assert ((torch.sigmoid(inp[1][k].double()) > 0.05).reshape(len(cnt), -1).sum(1)).tolist() == list(cnt)
    if name == "all-too-small":
        assert all(len(r["scores"]) == 0 for r in res)
    if equal:                     # the tie rule: the first locations win, in ascending order
        n0 = min(cfg["pre_nms_top_n"], counts[0][0])
        assert res[0]["pre_index"][:n0].tolist() == torch.nonzero(inp[1][0][0].reshape(-1) > 0).reshape(-1)[:n0].tolist()
    check(res, *run_gpu(inp, cfg, use_obb), name=name)


@functools.lru_cache(maxsize=None)
def big_case():
    """one scene, one 40^3 level (64 000 locations), every location a candidate (pre_nms_thresh 0), pre_nms_top_n 2500: 3000 strong locations
    with logits on a shuffled grid over [0, 3], the others N(-3, 0.3) (all below the strong ones, so the cut has a margin by construction)"""
    rng = np.random.default_rng(11)
    w = 40
    g = torch.stack(torch.meshgrid(torch.arange(w), torch.arange(w), torch.arange(w), indexing="ij"), -1).reshape(-1, 3)
    x = np.minimum(rng.normal(-3.0, 0.3, w ** 3), -1.0)
    x[rng.permutation(w ** 3)[:3000]] = rng.permutation(np.linspace(0.0, 3.0, 3000))
    d = rng.uniform(0.3, 2.2, (1, 6, w, w, w))
    inp = ([(g * 2 + 1).float()], [torch.from_numpy(x.astype(np.float32)).reshape(1, 1, w, w, w)], [torch.from_numpy(d.astype(np.float32))], [torch.zeros((1, 1, w, w, w))],
           [(80, 80, 80)], None)
    cfg = _cfg(0.0, 1.0, 1000, top_n=2500)
    return inp, cfg, P.postprocess(*inp, **cfg)


def test_a_level_of_64000_locations():
    inp, cfg, (res, marg) = big_case()
    margins_ok(marg)
    assert len(res[0]["pre_scores"]) > 2000 and 1000 <= len(res[0]["scores"]) < len(res[0]["pre_scores"])
    check(res, *run_gpu(inp, cfg, False), name="40^3")


# ---- 3. determinism, synchronisation, capture ------------------------------------------------------------------------------------------------
def _dense(M, gin, cfg, use_obb):
    return M.fcos_postprocess_dense(*gin, cfg["pre_nms_thresh"], cfg["pre_nms_top_n"], cfg["nms_thresh"], cfg["fpn_post_nms_top_n"], cfg["min_size"], False, use_obb)


def test_dense_form_is_deterministic_capturable_and_never_waits():
    M = _m()
    case = (True, 0.05, 2.0, True, 100, False)
    inp, res, marg = ref_case(*case)
    margins_ok(marg)
    gin = to_gpu(inp)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = _dense(M, gin, P.CFG, True)
        again = _dense(M, gin, P.CFG, True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, again))                      # two runs are bit-identical
    boxes, scores, counts = eager
    cap = sum(min(300, l.shape[0]) for l in gin[0])
    assert boxes.shape == (3, cap, 8) and scores.shape == (3, cap) and counts.dtype == torch.int32
    assert counts.tolist() == [len(r["scores"]) for r in res]
    for i, k in enumerate(counts.tolist()):
        assert not boxes[i, k:].any() and not scores[i, k:].any()                  # rows past the count are zero
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        gin2 = tuple([t.clone() for t in v] if isinstance(v, list) else v.clone() for v in gin)
        _dense(M, gin2, P.CFG, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = _dense(M, gin2, P.CFG, True)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(out, eager))


def test_list_form_synchronises_exactly_once():
    import warnings
    M = _m()
    case = (False, 0.05, 2.0, True, 100, False)
    inp, res, _ = ref_case(*case)
    gin = to_gpu(inp, sizes_as_list=True)       # grid_sizes as the reference passes it: a host list
    fn = M.FCOSPostProcessor(0.05, 300, 0.3, 100, 2.0, 1, False, False)
    fn(*gin)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            boxes, scores = fn(*gin)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    syncs = [x for x in w if "synchroniz" in str(x.message).lower()]
    assert len(syncs) == 1, [str(x.message) for x in w]
    check(res, boxes, scores, name="list form")


# ---- 4. consistency with the shipped NMS ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_obb", [False, True], ids=["aabb", "obb"])
def test_one_scene_equals_selection_then_rotated_iou_nms(use_obb):
    from nerf_mae_amd import rotated_iou
    M = _m()
    case = (use_obb, 0.05, 2.0, True, 100, False)
    inp, _, marg = ref_case(*case)
    margins_ok(marg)
    one = tuple([t[:1] for t in v] if i in (1, 2, 3, 5) else v for i, v in enumerate(inp))
    one = one[:4] + (one[4][:1],) + one[5:]
    pre = M.FCOSPostProcessor(0.05, 300, 0.3, 0, 2.0, 1, True, use_obb)(*to_gpu(one))       # the same selection, before NMS
    fin = M.FCOSPostProcessor(0.05, 300, 0.3, 0, 2.0, 1, False, use_obb)(*to_gpu(one))
    keep = rotated_iou.nms(pre[0][0][:, 1:].contiguous(), pre[1][0], 0.3)
    assert torch.equal(fin[0][0], pre[0][0][keep]) and torch.equal(fin[1][0], pre[1][0][keep])
    assert 0 < keep.numel() < pre[1][0].numel()


# ---- 5. error paths ------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    M = _m()
    inp = crafted(((4, 4, 4), (2, 2, 2)), ((10, 5), (3, 2)), 3)
    locs, cls, reg, ctr, sizes, _ = to_gpu(inp)
    args = (0.05, 16, 0.3, 0, 0.0)
    with pytest.raises(ValueError, match="one class channel"):
        M.fcos_postprocess_dense(locs, [torch.cat([c, c], 1) for c in cls], reg, ctr, sizes, None, *args)
    with pytest.raises(TypeError):
        M.fcos_postprocess_dense(locs, [c.double() for c in cls], reg, ctr, sizes, None, *args)
    with pytest.raises(TypeError):
        M.fcos_postprocess_dense(locs, cls, [r.half() for r in reg], ctr, sizes, None, *args)
    with pytest.raises(RuntimeError):
        M.fcos_postprocess_dense(locs, [c.cpu() for c in cls], reg, ctr, sizes, None, *args)
    with pytest.raises(ValueError, match="at most 4 levels"):
        M.fcos_postprocess_dense(locs[:1] * 5, cls[:1] * 5, reg[:1] * 5, ctr[:1] * 5, sizes, None, *args)
    big = lambda t: t[:1].expand(65, *t.shape[1:])       # noqa: E731
    with pytest.raises(ValueError, match="at most 64 scenes"):
        M.fcos_postprocess_dense(locs, [big(c) for c in cls], [big(r) for r in reg], [big(c) for c in ctr], sizes, None, *args)
    with pytest.raises(ValueError, match="grid_sizes"):
        M.fcos_postprocess_dense(locs, cls, reg, ctr, None, None, *args)
    with pytest.raises(ValueError, match="box_regression"):
        M.fcos_postprocess_dense(locs, cls, reg, ctr, sizes, None, *args, use_obb=True)
    # cap above the NMS limit, and the workspace bound that names its two knobs
    w = 27
    g = torch.zeros((w ** 3, 3), device="cuda")
    h = lambda c, n: [torch.zeros((n, c, w, w, w), device="cuda")]       # noqa: E731
    with pytest.raises(ValueError, match="pre_nms_top_n"):
        M.fcos_postprocess_dense([g], h(1, 1), h(6, 1), h(1, 1), [(8, 8, 8)], None, 0.05, M.NMS_MAX_BOXES + 1, 0.3, 0, 0.0)
    with pytest.raises(ValueError, match="pre_nms_top_n or pass fewer scenes"):
        M.fcos_postprocess_dense([g], h(1, 64), h(6, 64), h(1, 64), [(8, 8, 8)] * 64, None, 0.05, M.NMS_MAX_BOXES, 0.3, 0, 0.0)
    # the library's own argument checks: a NULL required pointer is the argument error, not a fault
    from nerf_mae_amd import ops
    from nerf_mae_amd._lib import NmhError, lib
    plan = ops.FcosPostPlan([64, 8], 2, 16)
    with pytest.raises(NmhError):
        lib().call("nmh_fcos_post_select", plan.L, plan.dims, plan.N, 6, 16, None, None, None, None, None, None, 0.05, 0.0, None, None, None, None, 0)
    with pytest.raises(NmhError):
        lib().call("nmh_fcos_post_nms", plan.L, plan.dims, plan.N, 6, 16, None, None, None, None, 0.3, 0, None, None, None, None, None, 0)
