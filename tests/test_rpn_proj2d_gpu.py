"""The 2-D projection loss of the RPN on the GPU (reg_loss_2d=True of nerf_mae_amd.rpn over csrc/rpn.hip) against the float64 restatements tests/_rpn_ref.py,
tests/_rpn_iou_ref.py and tests/_proj2d_ref.py, and against the reference's own third return of compute_loss recorded in tests/golden/g30_proj2d.npz.

Cases: the g20 geometry (mesh 32^3, 2 scenes, the second padded) with its recorded flags for (AABB, smooth_l1) and (OBB, smooth_l1), the g29 geometry with its planted
rows for (OBB, giou), and the wide AABB case of tests/test_rpn_gpu.py (582 workgroups: the final pass's strided loop).  Tolerance: the project's contract for fp32,
assert_close(rtol=1e-3); the rows here are far rows in the sense of tests/test_proj2d_gpu.py (decoded proposals lie voxels away from their boxes)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _proj2d_ref as J  # noqa: E402
from tests import _rpn_iou_ref as Q  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = ("aabb", "obb", "giou")
W_REG, W_2D = 0.7, 0.3


def _m():
    from nerf_mae_amd import rpn
    return rpn


def _gen():
    return _m().AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)


@functools.lru_cache(maxsize=None)
def g30():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g30_proj2d.npz")))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(rotated, loss_type, boxes, assign, flags, obj, reg)"""
    if name == "giou":
        c = Q.make_case()
        return dict(rotated=True, loss_type="giou", boxes=c["boxes"], assign=c["assign"], flags=c["flags"], obj=c["obj"], reg=c["reg"])
    rotated = name == "obb"
    boxes = R.make_scene(R.SEED[rotated], rotated=rotated, ori=R.ORI)
    g20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz"))
    obj, reg = R.make_heads(R.HEAD_SEED, len(R.NBOX), 8 if rotated else 6)
    return dict(rotated=rotated, loss_type="smooth_l1", boxes=boxes, assign=R.assign(boxes, ori=R.ORI, rotated=rotated),
                flags=torch.from_numpy(g20[("o_" if rotated else "a_") + "flags"]), obj=obj, reg=reg)


def _ref_losses(c, heads, mesh=R.MESH, **geom):
    a = c["assign"]
    if c["loss_type"] == "smooth_l1":
        lo, lr = R.losses(*heads, c["flags"], a["targets"])
    else:
        lo, lr = Q.losses(*heads, c["flags"], a["matched"], c["boxes"], c["loss_type"])
    return lo, lr, J.rpn_loss_2d(*heads, c["flags"], a["matched"], c["boxes"], mesh, a["valid"], **geom)


@functools.lru_cache(maxsize=None)
def ref(name):
    """float64 losses and the gradients of objectness + 0.7 box + 0.3 2-D"""
    c = case(name)
    heads = [[t.double().requires_grad_(True) for t in ts] for ts in (c["obj"], c["reg"])]
    out = _ref_losses(c, heads)
    (out[0] + W_REG * out[1] + W_2D * out[2]).backward()
    return [o.detach() for o in out], [[t.grad for t in ts] for ts in heads]


def _fn(c, gen=None, **kw):
    M, gen = _m(), _gen() if gen is None else gen
    if c["loss_type"] == "smooth_l1":
        return M.RPNLossComputation(gen, R.FG, R.BG, R.BATCH, R.FRACTION, rotated_bbox=c["rotated"], **kw)
    return M.RPNIoULossComputation(gen, R.FG, R.BG, R.BATCH, R.FRACTION, reg_loss_type=c["loss_type"], **kw)


def _ori(ori=R.ORI):
    return torch.tensor(ori, dtype=torch.int32).cuda()


def _gpu_heads(c, grad=True):
    return [[t.cuda().requires_grad_(grad) for t in ts] for ts in (c["obj"], c["reg"])]


def _keys(out):
    return torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"], out["loss_rpn_box_reg_2d"]]).detach()


def _compare_grads(heads, wgrads, tag):
    for name, ts, ws in zip(("d objectness", "d pred_bbox_deltas"), heads, wgrads):
        for k, (t, w) in enumerate(zip(ts, ws)):
            if w.abs().sum() > 0:
                assert_close(t.grad.cpu(), w, 1e-3, f"{tag} {name} level {k}")
            else:
                assert (t.grad == 0).all()


# ---- 1. against float64 and the recorded reference; the switch changes nothing else ---------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_three_losses_and_gradients_against_float64_and_the_first_two_bit_equal_to_the_run_without_the_term(name):
    c = case(name)
    want, wgrads = ref(name)
    boxes = [b.cuda() for b in c["boxes"]]
    heads = _gpu_heads(c)
    out = _fn(c, reg_loss_2d=True)(R.MESH, heads[0], heads[1], boxes, _ori(), sampled=c["flags"].cuda())
    assert out["loss_rpn_box_reg_2d"].requires_grad and out["loss_rpn_box_reg_2d"].item() > 0
    (out["loss_objectness"] + W_REG * out["loss_rpn_box_reg"] + W_2D * out["loss_rpn_box_reg_2d"]).backward()
    assert_close(_keys(out).cpu(), torch.stack(want), 1e-3, f"{name} losses")
    rec = float(g30()["rpn_iou_2d" if name == "giou" else f"rpn_{name}_2d"])
    assert abs(out["loss_rpn_box_reg_2d"].item() - rec) <= 1e-3 * rec, (name, out["loss_rpn_box_reg_2d"].item(), rec)
    _compare_grads(heads, wgrads, name)
    C = 8 if c["rotated"] else 6
    go, gr = R.flatten_heads([t.grad.cpu() for t in heads[0]], [t.grad.cpu() for t in heads[1]], C)
    assert (go[c["flags"] == 0] == 0).all() and (gr[c["flags"] != 1] == 0).all() and torch.isfinite(gr).all()
    # the default: the kernels without the term, the same bits for the first two losses, a constant zero for the third
    plain = _gpu_heads(c)
    off = _fn(c)(R.MESH, plain[0], plain[1], boxes, _ori(), sampled=c["flags"].cuda())
    assert torch.equal(off["loss_objectness"], out["loss_objectness"]) and torch.equal(off["loss_rpn_box_reg"], out["loss_rpn_box_reg"])
    assert off["loss_rpn_box_reg_2d"].item() == 0 and not off["loss_rpn_box_reg_2d"].requires_grad
    again = _fn(c, reg_loss_2d=True)(R.MESH, plain[0], plain[1], boxes, _ori(), sampled=c["flags"].cuda())
    assert torch.equal(_keys(again), _keys(out)), "two runs are bit-identical"


def test_above_256_partial_blocks():
    from tests import test_rpn_gpu as T
    W = T.WIDE
    boxes, a = T.wide_case()
    flags = R.make_flags(3, a["labels"], batch=W["batch"])
    obj, reg = R.make_heads(R.HEAD_SEED, len(W["nbox"]), 6, grids=W["grids"], A=[1, 1])
    c = dict(rotated=False, loss_type="smooth_l1", boxes=boxes, assign=a, flags=flags, obj=obj, reg=reg)
    h64 = [[t.double().requires_grad_(True) for t in ts] for ts in (obj, reg)]
    want = _ref_losses(c, h64, W["mesh"], grids=W["grids"], base=R.base_anchors(W["sizes"], W["ratios"]))
    (want[0] + W_REG * want[1] + W_2D * want[2]).backward()
    heads = _gpu_heads(c)
    gen = _m().AnchorGenerator3D(W["sizes"], W["ratios"])
    out = _fn(c, gen, reg_loss_2d=True)(W["mesh"], heads[0], heads[1], [b.cuda() for b in boxes], _ori(W["ori"]), sampled=flags.cuda())
    (out["loss_objectness"] + W_REG * out["loss_rpn_box_reg"] + W_2D * out["loss_rpn_box_reg_2d"]).backward()
    assert _m()._plan(gen, W["mesh"], W["grids"], 2, "test").nblocks > 256 and int((flags == 1).sum()) > 100
    assert_close(_keys(out).cpu(), torch.stack([w.detach() for w in want]), 1e-3, "wide losses")
    _compare_grads(heads, [[t.grad for t in ts] for ts in h64], "wide")


# ---- 2. every element written, degenerate calls -----------------------------------------------------------------------------------------------------
def _ops_call(c, obj, reg, flags, boxes, g=(1.0, 1.0, 1.0)):
    """the two ops entries on NaN-filled gradient workspaces -> (scalars, dobj, dreg)"""
    from nerf_mae_amd import ops, proj2d
    M = _m()
    ncols, C = (7, 8) if c["rotated"] else (6, 6)
    plan = M._plan(_gen(), R.MESH, R.GRIDS, flags.shape[0], "test")
    bx, offs = M._boxes("test", boxes, ncols)
    _, midx, targets = ops.rpn_assign(plan, bx, offs, ncols, _ori(), R.FG, R.BG)
    lt = None if c["loss_type"] == "smooth_l1" else c["loss_type"]
    args = (plan, C, lt, obj, reg, flags, targets, bx, offs, _ori(), midx, proj2d._cams(32.0), 32.0)
    scalars = ops.rpn_loss_fwd(*args)
    outs = ([torch.full_like(t, float("nan")) for t in obj], [torch.full_like(t, float("nan")) for t in reg])
    gs = [None if v is None else torch.tensor([v], dtype=torch.float32).cuda() for v in g]
    ops.rpn_loss_bwd(*args, scalars, *gs, out=outs)
    return scalars.cpu(), outs[0], outs[1]


@pytest.mark.parametrize("name", ("aabb", "giou"))
def test_every_element_is_written_and_the_degenerate_calls_give_zero(name):
    c = case(name)
    obj, reg = _gpu_heads(c, grad=False)
    boxes = [b.cuda() for b in c["boxes"]]
    flags = c["flags"].cuda()
    ncols, C = (7, 8) if c["rotated"] else (6, 6)
    scalars, dobj, dreg = _ops_call(c, obj, reg, flags, boxes)
    assert all(torch.isfinite(t).all() for t in dobj + dreg) and torch.isfinite(scalars).all(), "every element of both gradients is written"
    assert scalars[2].item() == int((c["flags"] != 0).sum()) and scalars[4].item() == int((c["flags"] == 1).sum()) and scalars[3].item() > 0
    go, gr = R.flatten_heads([t.cpu() for t in dobj], [t.cpu() for t in dreg], C)
    assert (go[c["flags"] == 0] == 0).all() and (gr[c["flags"] != 1] == 0).all()
    # no flagged anchor: losses 0 (the reference gives NaN), gradients 0
    scalars, dobj, dreg = _ops_call(c, obj, reg, torch.zeros_like(flags), boxes)
    assert scalars.tolist() == [0.0] * 5 and all((t == 0).all() for t in dobj + dreg)
    # only negatives: P = 0, the 2-D loss is 0
    neg = torch.where(flags == 1, torch.zeros_like(flags), flags)
    scalars, dobj, dreg = _ops_call(c, obj, reg, neg, boxes)
    assert scalars[3].item() == 0 and scalars[4].item() == 0 and scalars[0].item() > 0 and all((t == 0).all() for t in dreg)
    # a scene without boxes: its flagged positives count in P and contribute nothing
    s_full, _, _ = _ops_call(c, obj, reg, flags, boxes)
    only0 = c["flags"].clone()
    only0[1][only0[1] == 1] = 2
    s_empty, dobj_e, dreg_e = _ops_call(c, obj, reg, flags, [boxes[0], torch.zeros((0, ncols)).cuda()])
    s_only0, _, dreg_0 = _ops_call(c, obj, reg, only0.cuda(), boxes)
    p_all, p_0 = int((c["flags"] == 1).sum()), int((only0 == 1).sum())
    assert 0 < p_0 < p_all and s_empty[4].item() == p_all and s_only0[4].item() == p_0
    assert abs(s_empty[3].item() * p_all - s_only0[3].item() * p_0) <= 1e-5 * s_only0[3].item() * p_0, "the same sum of terms, divided by the two counts"
    assert all(torch.isfinite(t).all() for t in dobj_e + dreg_e)
    # only the 2-D loss has an upstream gradient: the objectness gradient is exactly zero, the box gradient is the 2-D term's alone
    _, dobj_2, dreg_2 = _ops_call(c, obj, reg, flags, boxes, g=(None, None, 1.0))
    assert all((t == 0).all() for t in dobj_2) and all(torch.isfinite(t).all() for t in dreg_2) and any((t != 0).any() for t in dreg_2)
    _, dobj_n, dreg_n = _ops_call(c, obj, reg, flags, boxes, g=(1.0, 1.0, None))
    _, _, dreg_a = _ops_call(c, obj, reg, flags, boxes)
    for a, b, both in zip(dreg_n, dreg_2, dreg_a):
        assert_close(both.cpu(), (a + b).cpu().double(), 1e-5, "the gradients of the three losses add")


def test_one_upstream_gradient_through_autograd():
    c = case("obb")
    boxes = [b.cuda() for b in c["boxes"]]
    heads = _gpu_heads(c)
    out = _fn(c, reg_loss_2d=True)(R.MESH, heads[0], heads[1], boxes, _ori(), sampled=c["flags"].cuda())
    out["loss_rpn_box_reg_2d"].backward()
    assert all((t.grad == 0).all() for t in heads[0]) and any((t.grad != 0).any() for t in heads[1])
    h64 = [[t.double().requires_grad_(True) for t in ts] for ts in (c["obj"], c["reg"])]
    _ref_losses(c, h64)[2].backward()
    _compare_grads([heads[1]], [[t.grad for t in h64[1]]], "only the 2-D loss")


# ---- 3. capture ---------------------------------------------------------------------------------------------------------------------------------------
def test_assignment_sampling_forward_backward_in_a_captured_graph_without_host_synchronisation():
    from tests.test_rpn_gpu import _state
    c = case("giou")
    boxes, ori = [b.cuda() for b in c["boxes"]], _ori()
    fn = _fn(c, seed=9, reg_loss_2d=True)
    base = [[t.cuda() for t in ts] for ts in (c["obj"], c["reg"])]

    def leaves():
        return [[t.clone().requires_grad_(True) for t in ts] for ts in base]

    def run(heads):
        out = fn(R.MESH, heads[0], heads[1], boxes, ori)
        flat = [t for ts in heads for t in ts]
        total = out["loss_objectness"] + out["loss_rpn_box_reg"] + out["loss_rpn_box_reg_2d"]
        return list(_keys(out).unbind()) + list(torch.autograd.grad(total, flat))

    run(leaves())                                # creates rng_state, the level table and the cameras
    eager = []
    for k in range(2):
        fn.rng_state.copy_(_state(9, 100 + k))
        heads = leaves()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eager.append([t.clone() for t in run(heads)])
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert fn.rng_state.cpu().tolist() == [9, 102] and not torch.equal(eager[0][3], eager[1][3])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        heads = leaves()
        run(heads)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(heads)
    fn.rng_state.copy_(_state(9, 100))
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert len(out) == 11 and all(torch.equal(a, b) for a, b in zip(out, eager[k])), f"replay {k}"
    assert fn.rng_state.cpu().tolist() == [9, 102] and eager[0][2].item() > 0


# ---- 4. through the networks ----------------------------------------------------------------------------------------------------------------------------
def test_nerf_rpn_with_the_switch_trains_on_the_2d_loss_alone():
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for
    from nerf_mae_amd.trainer import FusedAdamW
    from tests import test_rpn_network_gpu as NT
    M = _m()
    ref_case = NT.train_ref(False)
    maps = [f.float().cuda().requires_grad_(True) for f in ref_case["feats"]]          # a backbone's outputs: the head differentiates only behind inputs that ask

    def build(**kw):
        net = M.NeRFRegionProposalNetwork(NT._Backbone(maps), _gen(), M.RPNHead(NT.CIN, NT.A, NT.DEPTH, compute_dtype=torch.float32), rpn_fg_iou_thresh=R.FG,
                                          rpn_bg_iou_thresh=R.BG, rpn_batch_size_per_image=R.BATCH, rpn_positive_fraction=R.FRACTION, **kw)
        net.rpn.load_state_dict({"head." + k: v.float() for k, v in ref_case["P"].items()}, strict=True)
        return net.cuda().train()

    grids = [torch.randn(4, *o).cuda() for o in R.ORI]
    targets = [b.cuda() for b in ref_case["boxes"]]
    off, on = build(), build(reg_loss_2d=True)
    assert on.rpn.loss.reg_loss_2d and not off.rpn.loss.reg_loss_2d
    l_off, l_on = off(list(grids), targets)[1], on(list(grids), targets)[1]
    assert torch.equal(l_off["loss_objectness"], l_on["loss_objectness"]) and torch.equal(l_off["loss_rpn_box_reg"], l_on["loss_rpn_box_reg"])
    assert l_off["loss_rpn_box_reg_2d"].item() == 0 and l_on["loss_rpn_box_reg_2d"].item() > 0 and l_on["loss_rpn_box_reg_2d"].requires_grad
    flat = FlatParameters(on, torch.device("cuda"))
    opt = FusedAdamW(flat, lr=1e-3, weight_decay=0.0)
    step = FinetuneStep(flat, opt, loss_fn_for(on), weights={"loss_objectness": 0.0, "loss_rpn_box_reg": 0.0, "loss_rpn_box_reg_2d": 0.5})
    before = {k: v.detach().clone() for k, v in on.rpn.head.named_parameters()}
    out = step(list(grids), targets)
    assert torch.isfinite(out["loss_rpn_box_reg_2d"]) and out["loss_rpn_box_reg_2d"].item() > 0
    after = dict(on.rpn.head.named_parameters())
    assert not torch.equal(after["bbox_pred.weight"], before["bbox_pred.weight"]), "the 2-D weight alone moves the regression head"
    assert torch.equal(after["cls_logits.weight"], before["cls_logits.weight"]), "and nothing else reaches the objectness head"
