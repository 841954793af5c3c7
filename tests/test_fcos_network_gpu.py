"""FCOSModule and FCOSOverNeRF on the GPU (nerf_mae_amd.fcos): the head of tests/test_fcos_head_gpu.py joined to the loss and the post-processing kernels, on a
mesh of 40 x 36 x 32 with strides 4 .. 32 (levels (10,9,8) .. (2,2,1)), 64 channels, one tower layer, two scenes of different original size.

Training (fp32 compute): the three losses against tests/_fcos_ref.losses applied to the restated head (tests/_fcos_head_ref.head), gradients of
1.0 cls + 0.7 reg + 1.3 centerness to the head's parameters and to the features against float64 autograd of that chain, assert_close(rtol=1e-3), AABB and OBB.
Evaluation: the head's outputs are held to 1e-3; every discrete decision is then judged on identical inputs: the restated post-processing
(tests/_fcos_post_ref.postprocess) is fed the head tensors the module computed, its margins are asserted, and the module's lists are compared as
tests/test_fcos_post_gpu.py compares.  Then FCOSOverNeRF with a stub backbone (padding, return structure, target asserts), the training forward + backward and
detections_dense each without a host wait and captured once in a graph, and one whole-model step with the Swin FPN backbone."""
import functools
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_head_ref as H  # noqa: E402
from tests import _fcos_post_ref as P  # noqa: E402
from tests import _fcos_ref as F  # noqa: E402
from tests._metrics import assert_close  # noqa: E402
from tests.test_fcos_post_gpu import check, margins_ok  # noqa: E402

pytestmark = pytest.mark.gpu
C, N, CONVS = 64, 2, 1
MESH = (40, 36, 32)
STRIDES = (4, 8, 16, 32)
SIZES = ((10, 9, 8), (5, 5, 4), (3, 3, 2), (2, 2, 1))
ORI = ((40, 36, 32), (30, 36, 25))
NBOX = (9, 3)
NET_SEED = {False: 2, True: 0}          # head parameters and features: seeds whose detections keep every margin of tests/_fcos_post_ref.py above 1e-4 on the CPU
POST = dict(pre_nms_thresh=0.05, pre_nms_top_n=40, nms_thresh=0.3, fpn_post_nms_top_n=15, min_size=0.0)
WEIGHTS = (1.0, 0.7, 1.3)


def _m():
    from nerf_mae_amd import fcos
    return fcos


def make_args(obb, dtype=torch.float32, num_convs=CONVS):
    return types.SimpleNamespace(num_convs=num_convs, norm_reg_targets=True, centerness_on_reg=True, rotated_bbox=obb, center_sampling_radius=1.5,
                                 iou_loss_type="iou" if obb else "giou", use_additional_l1_loss=obb, proj2d_loss_weight=0.0, compute_dtype=dtype, **POST)


def params_and_features(obb, seed=None):
    seed = NET_SEED[obb] if seed is None else seed
    nreg = 8 if obb else 6
    Pm = H.make_params(700 + 10 * seed + obb, CONVS, C, nreg, scales=(1.1, 0.9, 1.2, 0.8, 1.0))
    w, b = Pm["bbox_pred.weight"], Pm["bbox_pred.bias"]
    w[:6] *= 0.3                         # distances around 1.5 (times the stride in evaluation): the ReLU masks are the subject of tests/test_fcos_head_gpu.py
    b[:6] = 1.5 + b[:6].abs()
    w[6:] *= 0.05                        # alpha, beta well inside the decode's clamp
    b[6:] *= 0.3
    Pm["cls_logits.bias"][:] = -1.0
    feats = [f.float().double() for f in H.make_features(800 + 10 * seed + obb, N, C, SIZES)]
    return {k: v.float().double() for k, v in Pm.items()}, feats


@functools.lru_cache(maxsize=None)
def train_ref(obb):
    """float64: the restated head in training mode, then the restated losses; gradients of the weighted sum"""
    Pm, feats = params_and_features(obb)
    boxes = F.make_scene(F.SEED[obb], obb, nbox=NBOX, extent=MESH)
    asg = F.assign(boxes, 1.5, True, SIZES, STRIDES, orig=ORI)
    Pg = {k: v.clone().requires_grad_(True) for k, v in Pm.items()}
    fg = [f.clone().requires_grad_(True) for f in feats]
    cls, reg, ctr = H.head(fg, Pg, CONVS, True, "train", STRIDES)
    losses = F.losses(cls, reg, ctr, asg, "iou" if obb else "giou", add_l1=obb)
    sum(w * l for w, l in zip(WEIGHTS, losses)).backward()
    dparam = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in Pg.items() if k != "scales.4.scale"}
    return dict(P=Pm, feats=feats, boxes=boxes, npos=asg["npos"], losses=[l.detach() for l in losses], dparam=dparam, dfeat=[f.grad for f in fg])


@functools.lru_cache(maxsize=None)
def eval_ref(obb):
    Pm, feats = params_and_features(obb)
    with torch.no_grad():
        return H.head(feats, Pm, CONVS, True, "eval", STRIDES)


def build(obb, Pm, dtype=torch.float32, resolution=None):
    net = _m().FCOSModule(make_args(obb, dtype), C, list(STRIDES), resolution=resolution)
    net.load_state_dict({"head." + k: v.float() for k, v in Pm.items()}, strict=True)
    return net.cuda()


@pytest.mark.parametrize("obb", (False, True), ids=("aabb", "obb"))
def test_training_losses_and_gradients_against_float64(obb):
    c = train_ref(obb)
    assert c["npos"] > 20 and all(l > 0 for l in c["losses"])
    net = build(obb, c["P"]).train()
    feats = [f.float().cuda().requires_grad_(True) for f in c["feats"]]
    boxes, scores, losses = net(list(ORI), feats, [b.cuda() for b in c["boxes"]])
    assert boxes is None and scores is None and sorted(losses) == ["loss_centerness", "loss_cls", "loss_reg"]
    got = [losses["loss_cls"], losses["loss_reg"], losses["loss_centerness"]]
    sum(w * l for w, l in zip(WEIGHTS, got)).backward()
    tag = "obb" if obb else "aabb"
    assert_close(torch.stack(got).detach().cpu(), torch.stack(c["losses"]), 1e-3, f"{tag} losses")
    grads = dict(net.head.named_parameters())
    assert grads["scales.4.scale"].grad is None
    for name, want in c["dparam"].items():
        assert_close(grads[name].grad.cpu(), want, 1e-3, f"{tag} d {name}")
    for k, f in enumerate(feats):
        assert_close(f.grad.cpu(), c["dfeat"][k], 1e-3, f"{tag} d features {k}")


@pytest.mark.parametrize("obb", (False, True), ids=("aabb", "obb"))
def test_evaluation_detections_on_the_modules_own_head_tensors(obb):
    M = _m()
    Pm, fe = params_and_features(obb)
    net = build(obb, Pm).eval()
    feats = [f.float().cuda() for f in fe]
    with torch.no_grad():
        cls, reg, ctr = net.head(feats)
        boxes, scores, losses = net(list(ORI), feats)
        dense = net.detections_dense(list(ORI), feats)
    tag = "obb" if obb else "aabb"
    for name, got, want in zip(("logits", "bbox_reg", "centerness"), (cls, reg, ctr), eval_ref(obb)):
        for k in range(len(feats)):
            assert_close(got[k].cpu(), want[k], 1e-3, f"{tag} {name} {k}")
    assert losses == {} and len(boxes) == len(scores) == N
    locs = [l.float() for l in F.locations(SIZES, STRIDES)]
    assert all(torch.equal(a.cpu(), b) for a, b in zip(net.compute_locations(feats), locs)), "compute_locations: the reference's semantics"
    masks = F.valid_masks(ORI, SIZES, STRIDES)
    assert all(torch.equal(a.cpu(), b) for a, b in zip(net.compute_padding_masks(net.compute_locations(feats), ORI), masks))
    res, marg = P.postprocess(locs, [t.cpu() for t in cls], [t.cpu() for t in reg], [t.cpu() for t in ctr], [tuple(o) for o in ORI], masks, **POST)
    margins_ok(marg)
    check(res, boxes, scores, f"network {tag}")
    assert all(len(r["pre_scores"]) > len(r["scores"]) > 0 for r in res), "NMS does real work"
    for i in range(N):
        k = int(dense[2][i])
        assert torch.equal(dense[0][i, :k], boxes[i]) and torch.equal(dense[1][i, :k], scores[i])
    # one scene without a resolution: no padding mask (fcos.py:207-214)
    one = [f[:1].contiguous() for f in feats]
    with torch.no_grad():
        b1, s1, _ = net([ORI[1]], one)
        c1, r1, t1 = net.head(one)
    res1, _ = P.postprocess(locs, [t.cpu() for t in c1], [t.cpu() for t in r1], [t.cpu() for t in t1], [tuple(ORI[1])], None, **POST)
    assert [len(s) for s in s1] == [len(r["scores"]) for r in res1]
    assert isinstance(M.FCOSModule(make_args(obb), C, list(STRIDES), resolution=40).head, M.FCOSHead)


class _Backbone(torch.nn.Module):
    """returns four fixed maps, whatever the grids hold"""
    out_channels = C

    def __init__(self, maps):
        super().__init__()
        self.maps = maps
        self.seen = None

    def forward(self, x):
        self.seen = x
        return tuple(self.maps)


def _over(obb, Pm, maps, resolution=None):
    net = _m().FCOSOverNeRF(make_args(obb), _Backbone(maps), list(STRIDES), resolution=resolution)
    net.fcos_module.load_state_dict({"head." + k: v.float() for k, v in Pm.items()}, strict=True)
    return net.cuda()


def test_fcos_over_nerf_pads_returns_the_reference_structure_and_checks_targets():
    c = train_ref(False)
    maps = [f.float().cuda() for f in c["feats"]]
    net = _over(False, c["P"], maps)
    grids = [torch.randn(4, *o).cuda() + 3.0 for o in ORI]
    targets = [b.cuda() for b in c["boxes"]]
    net.train()
    boxes, losses, scores = net(list(grids), targets)
    seen = net.backbone.seen
    assert tuple(seen.shape) == (N, 4, *MESH) and torch.equal(seen[0], grids[0]) and torch.equal(seen[1, :, :30, :36, :25], grids[1])
    assert not seen[1, :, 30:].any() and not seen[1, :, :, :, 25:].any(), "zero padding to the batch maximum"
    assert boxes is None and scores is None and sorted(losses) == ["loss_centerness", "loss_cls", "loss_reg"]
    direct = net.fcos_module(list(ORI), maps, targets)[2]
    assert all(torch.equal(direct[k], losses[k]) for k in losses), "the original sizes reach the padding masks"
    assert_close(torch.stack([losses["loss_cls"], losses["loss_reg"], losses["loss_centerness"]]).detach().cpu(), torch.stack(c["losses"]), 1e-3, "losses through FCOSOverNeRF")
    net.eval()
    with torch.no_grad():
        boxes, losses, scores = net(list(grids))
        want = net.fcos_module(list(ORI), maps)
    assert losses == {} and len(boxes) == N and all(torch.equal(a, b) for got, w in zip((boxes, scores), want[:2]) for a, b in zip(got, w))
    assert all(b.shape == (s.shape[0], 7) for b, s in zip(boxes, scores))
    # resolution: every grid is padded to it, also a single one
    big = _over(False, c["P"], [m[:1].contiguous() for m in maps], resolution=40).eval()
    with torch.no_grad():
        big([grids[1]])
    assert tuple(big.backbone.seen.shape) == (1, 4, 40, 40, 40) and not big.backbone.seen[0, :, 30:].any()
    # target asserts
    net.train()
    with pytest.raises(AssertionError, match="targets should not be none"):
        net(list(grids))
    with pytest.raises(AssertionError, match=r"shape \[N, 6\]"):
        net(list(grids), [torch.zeros(2, 7).cuda(), targets[1]])
    with pytest.raises(AssertionError, match="of type Tensor"):
        net(list(grids), [None, targets[1]])
    with pytest.raises(ValueError):
        _m().FCOSOverNeRF(make_args(False), torch.nn.Identity(), list(STRIDES))


def test_training_forward_and_backward_never_wait_and_replay_from_one_graph():
    """FCOSOverNeRF: stub backbone -> head -> assignment -> losses -> backward, N = 2 with padding masks"""
    c = train_ref(True)
    base = [f.float().cuda() for f in c["feats"]]
    targets = [b.cuda() for b in c["boxes"]]
    grids = [torch.randn(4, *o).cuda() for o in ORI]
    net = _over(True, c["P"], [b.clone().requires_grad_(True) for b in base]).train()
    params = [p for n, p in net.fcos_module.head.named_parameters() if n != "scales.4.scale"]
    names = [n for n, _ in net.fcos_module.head.named_parameters() if n != "scales.4.scale"]

    def run():
        for p in params:
            if p.grad is not None:
                p.grad.zero_()
        _, losses, _ = net(list(grids), targets)
        g = torch.autograd.grad(losses["loss_cls"] + losses["loss_reg"] + losses["loss_centerness"], net.backbone.maps)
        return [losses["loss_cls"].detach(), losses["loss_reg"].detach(), losses["loss_centerness"].detach(), *g, *[p.grad for p in params]]

    run()                                        # the packed weights, the gradient buffers, the locations and the padding masks are made on the first call
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = run()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    eager = [t.clone() for t in eager]
    assert all(torch.isfinite(t).all() for t in eager) and all(p.grad.abs().sum() > 0 for n, p in zip(names, params) if not n.startswith("scales."))      # (a level without positives leaves its Scale without gradient)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        net.backbone.maps = [b.clone().requires_grad_(True) for b in base]
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        exact = [0, 1, 2] + [3 + len(base) + i for i, n in enumerate(names) if "tower" not in n or n.split(".")[1] == "1"]
        for i, (a, b) in enumerate(zip(out, eager)):     # bit for bit where the sums have a fixed order (the losses, the output stage's and the GroupNorm's parameter
            if i in exact:                                # gradients); the tower convs' weight and bias gradients add atomically
                assert torch.equal(a, b), f"replay output {i}"
            else:
                assert_close(a, b, 1e-4, f"replay output {i}")


def test_detections_dense_never_waits_and_is_capturable():
    Pm, fe = params_and_features(False)
    net = build(False, Pm).eval()
    feats = [f.float().cuda() for f in fe]
    ori = torch.tensor(ORI, dtype=torch.int32).cuda()
    with torch.no_grad():
        net.detections_dense(ori, feats)
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eager = net.detections_dense(ori, feats)
        finally:
            torch.cuda.set_sync_debug_mode(mode)
        torch.cuda.synchronize()
        lists = net(list(ORI), feats)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            static = [torch.zeros_like(f) for f in feats]
            net.detections_dense(ori, static)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
            out = net.detections_dense(ori, static)
        for d, f in zip(static, feats):
            d.copy_(f)
        graph.replay()
        torch.cuda.synchronize()
    assert int(eager[2].min()) > 0 and all(torch.equal(a, b) for a, b in zip(out, eager))
    for i in range(N):
        assert torch.equal(eager[0][i, :int(eager[2][i])], lists[0][i]), "the dense form with device sizes is the list form"


def test_whole_model_training_step_with_the_swin_fpn_backbone():
    """the real backbone (resolution 32, the smallest its four stages accept) -> FCOSOverNeRF in bf16: finite losses and a gradient on every parameter"""
    from nerf_mae_amd.fpn import SwinTransformer_FPN_Pretrained_Skip
    torch.manual_seed(0)
    backbone = SwinTransformer_FPN_Pretrained_Skip(is_eval=True, resolution=32, out_channels=64)
    net = _m().FCOSOverNeRF(make_args(False, torch.bfloat16, num_convs=2), backbone, list(STRIDES), resolution=32).cuda().train()
    boxes = [b.cuda() for b in F.make_scene(F.SEED[False], False, nbox=(5,), extent=(32, 32, 32))]
    grid = torch.rand(4, 30, 32, 27).cuda()
    out, losses, scores = net([grid], boxes)
    assert out is None and scores is None
    (losses["loss_cls"] + losses["loss_reg"] + losses["loss_centerness"]).backward()
    torch.cuda.synchronize()
    assert all(torch.isfinite(v) for v in losses.values()) and losses["loss_cls"].item() > 0
    missing = [n for n, p in net.named_parameters() if p.requires_grad and not n.endswith("scales.4.scale") and (p.grad is None or not torch.isfinite(p.grad).all())]
    assert not missing, missing          # (pos_embed is frozen; the fifth Scale has no level)
    head = net.fcos_module.head
    assert all(p.grad.abs().sum() > 0 for n, p in head.named_parameters() if n != "scales.4.scale" and not n.startswith(("bbox_pred", "scales")))
