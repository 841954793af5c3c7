"""The oriented RPN's IoU-type box regression losses on the GPU (nerf_mae_amd.rpn.RPNIoULossComputation over csrc/rpn.hip and csrc/rpn_decode.hpp) against
the float64 restatement tests/_rpn_iou_ref.py (itself checked against the recorded reference, tests/golden/g29_rpn_iou_loss.npz, in
tests/test_rpn_iou_ref_cpu.py) and against that recording directly.

Geometry: the g20 case (mesh 32^3, grids 8^3 .. 1^3, 13 anchors per location, 7 605 anchors per scene, N = 2, original sizes (32,32,32) and (24,28,20)) with
the scenes of tests/_rpn_iou_ref.make_case: 85 flagged positives on the two levels that have any, nine of them planted, one per branch of the decode and the pair geometry.

Tolerance: the project's contract for fp32, assert_close(rtol=1e-3), on the two scalars and on every level's dobj and dreg; no row is left out.  Condition,
measured on the CPU when the fixture was recorded (tools/gen_golden_rpn_iou.py prints it): on these rows the reference evaluated in fp32 stays within
8.9e-8 (loss, relative) and 6.6e-6 (gradient, of the max norm) of its float64 evaluation, for all four types; the bound of the condition is 1e-4.
Measured on an MI355X (NMH_PRINT_ERR=1): losses 1.2e-7, dreg 3.0e-6 in the max norm and 0.03 of the elementwise tolerance at worst."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_iou_ref as Q  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
G_OBJ, G_REG = 1.3, 0.7


def _m():
    from nerf_mae_amd import rpn
    return rpn


def _gen():
    return _m().AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)


@functools.lru_cache(maxsize=None)
def case():
    c = Q.make_case()
    Q.check_case(c)
    return c


@functools.lru_cache(maxsize=None)
def g29():
    return {k: v for k, v in np.load(os.path.join(ROOT, "tests", "golden", "g29_rpn_iou_loss.npz")).items()}


@functools.lru_cache(maxsize=None)
def ref(loss_type):
    """float64 losses and the gradients of G_OBJ objectness + G_REG box for the case's recorded sampled set"""
    c = case()
    heads = [[t.double().requires_grad_(True) for t in ts] for ts in (c["obj"], c["reg"])]
    out = Q.losses(*heads, c["flags"], c["assign"]["matched"], c["boxes"], loss_type)
    (G_OBJ * out[0] + G_REG * out[1]).backward()
    return [o.detach() for o in out], [[t.grad for t in ts] for ts in heads]


def _fn(loss_type, **kw):
    return _m().RPNIoULossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION, reg_loss_type=loss_type, **kw)


def _gpu_heads(c=None):
    c = case() if c is None else c
    return [[t.cuda().requires_grad_(True) for t in ts] for ts in (c["obj"], c["reg"])]


def _ori():
    return torch.tensor(R.ORI, dtype=torch.int32).cuda()


def _run(loss_type, heads, flags, boxes=None, backward=True):
    boxes = case()["boxes"] if boxes is None else boxes
    out = _fn(loss_type)(R.MESH, heads[0], heads[1], [b.cuda() for b in boxes], _ori(), sampled=flags.cuda())
    if backward:
        (G_OBJ * out["loss_objectness"] + G_REG * out["loss_rpn_box_reg"]).backward()
    return out


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", Q.TYPES)
def test_losses_and_gradients_against_float64(loss_type):
    c = case()
    want, wgrads = ref(loss_type)
    heads = _gpu_heads()
    out = _run(loss_type, heads, c["flags"])
    assert_close(torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"]]).detach().cpu(), torch.stack(want), 1e-3, f"{loss_type} losses")
    assert out["loss_rpn_box_reg_2d"].item() == 0 and not out["loss_rpn_box_reg_2d"].requires_grad
    for name, ts, ws in zip(("d objectness", "d pred_bbox_deltas"), heads, wgrads):
        for k, (t, w) in enumerate(zip(ts, ws)):
            if w.abs().sum() > 0:
                assert_close(t.grad.cpu(), w, 1e-3, f"{loss_type} {name} level {k}")
            else:
                assert (t.grad == 0).all()
    go, gr = R.flatten_heads([t.grad.cpu() for t in heads[0]], [t.grad.cpu() for t in heads[1]], 8)
    flags = c["flags"]
    assert (go[flags == 0] == 0).all() and (gr[flags != 1] == 0).all(), "gradients are exactly zero at unsampled anchors, the box gradient at every anchor but the flagged positives"
    assert torch.isfinite(gr).all() and (go[flags != 0] != 0).all() and (gr[flags == 1].abs().sum(-1) > 0).all()
    # the rows without overlap: no centre gradient under the IoU types (exactly), one under GIoU and DIoU
    n = flags.shape[1]
    rows = gr.reshape(-1, 8)[[c["planted"]["no_bev"], c["planted"]["no_z"]]]
    assert c["planted"]["no_z"] < n
    if loss_type in ("iou", "linear_iou"):
        assert (rows[:, :3] == 0).all() and (rows[:, 3:6] != 0).all()
    else:
        assert (rows[:, :3].abs().sum(1) > 0).all()


# ---- 2. against the recorded reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss_type", Q.TYPES)
def test_recorded_rows_at_their_anchors_in_an_otherwise_unsampled_scene(loss_type):
    c, g = case(), g29()
    N, n = c["flags"].shape
    P = g["index"].shape[0]
    flags = torch.zeros((N, n), dtype=torch.uint8)
    flags.view(-1)[torch.from_numpy(g["index"]).long()] = 1
    heads = [[torch.zeros_like(t) for t in ts] for ts in (c["obj"], c["reg"])]
    flat = [t.reshape(N, -1, 8, *t.shape[2:]) for t in heads[1]]
    for i, row in zip(g["index"].tolist(), torch.from_numpy(g["deltas"])):
        lvl, (a, w, h, d) = Q.locate(i % n)
        flat[lvl][i // n, a, :, w, h, d] = row
    heads = [[t.cuda().requires_grad_(True) for t in ts] for ts in heads]
    out = _fn(loss_type)(R.MESH, heads[0], heads[1], [b.cuda() for b in c["boxes"]], _ori(), sampled=flags.cuda())
    out["loss_rpn_box_reg"].backward()
    want = torch.tensor([float(g[loss_type + "_loss"]) / P], dtype=torch.float64)          # the recorded sum over the P sampled anchors
    assert_close(out["loss_rpn_box_reg"].detach().cpu().reshape(1), want, 1e-3, f"g29 {loss_type} loss")
    gr = R.flatten_heads([t.grad.cpu() for t in heads[0]], [t.grad.cpu() for t in heads[1]], 8)[1].reshape(-1, 8)
    assert_close(gr[torch.from_numpy(g["index"]).long()], torch.from_numpy(g[loss_type + "_grad"]).double() / P, 1e-3, f"g29 {loss_type} gradient")
    assert all((t.grad == 0).all() for t in heads[0]), "no upstream gradient for the objectness loss"


# ---- 3. every element written ----------------------------------------------------------------------------------------------------------------
def _ops_call(loss_type, obj, reg, flags, boxes, ori=None, g=(1.0, 1.0)):
    """the two ops entries on NaN-filled gradient workspaces -> (scalars, dobj, dreg)"""
    from nerf_mae_amd import ops
    M = _m()
    plan = M._plan(_gen(), R.MESH, R.GRIDS, flags.shape[0], "test")
    bx, offs = M._boxes("test", boxes, 7)
    _, midx, _ = ops.rpn_assign(plan, bx, offs, 7, ori, R.FG, R.BG)
    scalars = ops.rpn_loss_fwd(plan, 8, loss_type, obj, reg, flags, None, bx, offs, ori, midx)
    outs = ([torch.full_like(t, float("nan")) for t in obj], [torch.full_like(t, float("nan")) for t in reg])
    go, gr = [torch.tensor([v], dtype=torch.float32).cuda() for v in g]
    ops.rpn_loss_bwd(plan, 8, loss_type, obj, reg, flags, None, bx, offs, ori, midx, None, None, scalars, go, gr, out=outs)
    return scalars, outs[0], outs[1]


@pytest.mark.parametrize("loss_type", ("linear_iou", "diou"))
def test_every_element_is_written_and_the_degenerate_calls_give_zero(loss_type):
    c = case()
    obj, reg = [[t.cuda() for t in ts] for ts in (c["obj"], c["reg"])]
    boxes = [b.cuda() for b in c["boxes"]]
    flags = c["flags"].cuda()
    scalars, dobj, dreg = _ops_call(loss_type, obj, reg, flags, boxes, _ori())
    assert all(torch.isfinite(t).all() for t in dobj + dreg) and torch.isfinite(scalars).all(), "every element of both gradients is written; all values are finite on the planted rows"
    go, gr = R.flatten_heads([t.cpu() for t in dobj], [t.cpu() for t in dreg], 8)
    assert (go[c["flags"] == 0] == 0).all() and (gr[c["flags"] != 1] == 0).all() and scalars[2].item() == int((c["flags"] != 0).sum())
    # no sampled anchor: loss 0, gradients 0
    scalars, dobj, dreg = _ops_call(loss_type, obj, reg, torch.zeros_like(flags), boxes, _ori())
    assert scalars.cpu().tolist() == [0.0, 0.0, 0.0] and all((t == 0).all() for t in dobj + dreg)
    # a scene without boxes: its flagged positives count as sampled anchors, take part in the objectness loss and contribute no box term
    only0 = c["flags"].clone()
    only0[1][only0[1] == 1] = 2
    s_empty, dobj_e, dreg_e = _ops_call(loss_type, obj, reg, flags, [boxes[0], torch.zeros((0, 7)).cuda()], _ori())
    s_only0, _, dreg_0 = _ops_call(loss_type, obj, reg, only0.cuda(), boxes, _ori())
    assert s_empty[1].item() == s_only0[1].item() > 0 and s_empty[2].item() == s_only0[2].item()
    assert all(torch.equal(a, b) for a, b in zip(dreg_e, dreg_0)) and all(torch.isfinite(t).all() for t in dobj_e)
    assert all((t[1] == 0).all() for t in dreg_e) and any((t[1] != 0).any() for t in dobj_e)
    # a flagged positive in the padding of the second scene (only `sampled=` can produce one) contributes nothing either
    valid = torch.from_numpy(R.valid_mask(R.ORI[1]))
    pad = int(torch.nonzero(~valid)[0, 0])
    extra = c["flags"].clone()
    extra[1, pad] = 1
    as_neg = c["flags"].clone()
    as_neg[1, pad] = 2
    s_pad, _, dreg_p = _ops_call(loss_type, obj, reg, extra.cuda(), boxes, _ori())
    s_neg, _, dreg_n = _ops_call(loss_type, obj, reg, as_neg.cuda(), boxes, _ori())
    assert s_pad[1].item() == s_neg[1].item() and all(torch.equal(a, b) for a, b in zip(dreg_p, dreg_n))


# ---- 4. autograd conventions -----------------------------------------------------------------------------------------------------------------
def test_one_upstream_gradient_and_heads_that_need_none():
    c = case()
    want, wgrads = ref("giou")
    for which, scale in ((0, G_OBJ), (1, G_REG)):
        heads = _gpu_heads()
        out = _run("giou", heads, c["flags"], backward=False)
        (out["loss_objectness"] if which == 0 else out["loss_rpn_box_reg"]).backward()
        other = heads[1 - which]
        assert all((t.grad == 0).all() for t in other), "the loss that got no upstream gradient leaves exact zeros"
        for k, (t, w) in enumerate(zip(heads[which], wgrads[which])):
            if w.abs().sum() > 0:
                assert_close(t.grad.cpu(), w / scale, 1e-3, f"only g[{which}] level {k}")
    heads = [[t.cuda() for t in ts] for ts in (c["obj"], c["reg"])]
    out = _run("giou", heads, c["flags"], backward=False)
    assert not out["loss_objectness"].requires_grad and not out["loss_rpn_box_reg"].requires_grad
    assert_close(torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"]]).cpu(), torch.stack(want), 1e-3, "losses without gradient")
    mixed = [[t.cuda() for t in c["obj"]], [t.cuda().requires_grad_(True) for t in c["reg"]]]       # only the regression head asks
    out = _run("giou", mixed, c["flags"])
    for k, (t, w) in enumerate(zip(mixed[1], wgrads[1])):
        if w.abs().sum() > 0:
            assert_close(t.grad.cpu(), w, 1e-3, f"regression only, level {k}")


# ---- 5. determinism and the shared sampler ---------------------------------------------------------------------------------------------------
def test_two_runs_are_bit_identical_and_the_sampler_is_shared_with_the_smooth_l1_class():
    c = case()
    res = []
    for _ in range(2):
        heads = _gpu_heads()
        out = _run("diou", heads, c["flags"])
        res.append([out["loss_objectness"].detach(), out["loss_rpn_box_reg"].detach()] + [t.grad for ts in heads for t in ts])
    assert all(torch.equal(a, b) for a, b in zip(*res))
    boxes, ori = [b.cuda() for b in c["boxes"]], _ori()
    heads = [[t.cuda() for t in ts] for ts in (c["obj"], c["reg"])]
    a = _fn("iou", seed=21)(R.MESH, heads[0], heads[1], boxes, ori)
    b = _m().RPNLossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION, rotated_bbox=True, seed=21)(R.MESH, heads[0], heads[1], boxes, ori)
    assert torch.equal(a["loss_objectness"], b["loss_objectness"]) and a["loss_objectness"].item() > 0, "one seed, one sample, one BCE: the same bits"
    assert a["loss_rpn_box_reg"].item() != b["loss_rpn_box_reg"].item()
    other = _fn("iou", seed=22)(R.MESH, heads[0], heads[1], boxes, ori)
    assert not torch.equal(other["loss_objectness"], a["loss_objectness"])


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------------
def test_assignment_sampling_forward_backward_in_a_captured_graph_without_host_synchronisation():
    from tests.test_rpn_gpu import _state
    c = case()
    boxes, ori = [b.cuda() for b in c["boxes"]], _ori()
    fn = _fn("giou", seed=9)
    base = [[t.cuda() for t in ts] for ts in (c["obj"], c["reg"])]

    def leaves():
        return [[t.clone().requires_grad_(True) for t in ts] for ts in base]

    def run(heads):
        out = fn(R.MESH, heads[0], heads[1], boxes, ori)
        flat = [t for ts in heads for t in ts]
        return [out["loss_objectness"].detach(), out["loss_rpn_box_reg"].detach()] + list(torch.autograd.grad(out["loss_objectness"] + out["loss_rpn_box_reg"], flat))

    run(leaves())                                # creates rng_state and the level table
    eager = []
    for k in range(2):
        fn.rng_state.copy_(_state(9, 100 + k))
        heads = leaves()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eager.append(run(heads))
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert fn.rng_state.cpu().tolist() == [9, 102] and not torch.equal(eager[0][2], eager[1][2])
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
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert len(out) == 10 and all(torch.equal(a, b) for a, b in zip(out, eager[k])), f"replay {k}"
    assert fn.rng_state.cpu().tolist() == [9, 102] and eager[0][1].item() > 0


# ---- 7. error paths ----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_c_entries_and_of_the_class():
    from nerf_mae_amd import ops
    from nerf_mae_amd._lib import lib
    M = _m()
    c = case()
    obj, reg = [[t.cuda() for t in ts] for ts in (c["obj"], c["reg"])]
    boxes = [b.cuda() for b in c["boxes"]]
    flags = c["flags"].cuda()
    plan = M._plan(_gen(), R.MESH, R.GRIDS, 2, "test")
    bx, offsets = M._boxes("test", boxes, 7)
    _, midx, _ = ops.rpn_assign(plan, bx, offsets, 7, None, R.FG, R.BG)
    offs = (ctypes.c_int * 3)(*offsets)
    partials = torch.empty((3 * plan.nblocks,), dtype=torch.float32).cuda()
    scalars = torch.zeros((3,), dtype=torch.float32).cuda()
    dobj, dreg = [torch.empty_like(t) for t in obj], [torch.empty_like(t) for t in reg]
    tab = lambda ts: ops._ptr_table(ts, plan.L)          # noqa: E731
    L = lib()

    def fwd(ncols=8, lt=0, o=None, r=None, base=plan.base, dims=plan.dims):
        return L.cdll.nmh_rpn_iou_loss_fwd(plan.L, dims, base, plan.N, ncols, lt, tab(obj) if o is None else o, tab(reg) if r is None else r, flags.data_ptr(), bx.data_ptr(), offs, None,
                                           midx.data_ptr(), partials.data_ptr(), scalars.data_ptr(), None)

    def bwd(ncols=8, lt=0, do=None, dr=None, base=plan.base):
        return L.cdll.nmh_rpn_iou_loss_bwd(plan.L, plan.dims, base, plan.N, ncols, lt, tab(obj), tab(reg), flags.data_ptr(), bx.data_ptr(), offs, None, midx.data_ptr(), scalars.data_ptr(), None,
                                           None, tab(dobj) if do is None else do, tab(dreg) if dr is None else dr, None)

    assert fwd() == 0 and bwd() == 0
    null_level = ops._ptr_table([None] + obj[1:], plan.L)
    for rc in (fwd(ncols=6), fwd(ncols=7), fwd(lt=-1), fwd(lt=4), fwd(base=None),fwd(dims=None), fwd(o=null_level), fwd(r=ops._ptr_table([None] + reg[1:], plan.L)),
               bwd(ncols=6), bwd(lt=4), bwd(base=None), bwd(do=null_level), bwd(dr=ops._ptr_table(dreg[:-1] + [None], plan.L))):
        assert rc == -4
    torch.cuda.synchronize()
    fn = _fn("iou")
    with pytest.raises(TypeError):
        fn(R.MESH, [t.double() for t in obj], reg, boxes)
    with pytest.raises(RuntimeError):
        fn(R.MESH, [t.cpu() for t in obj], reg, boxes)
    with pytest.raises(ValueError):
        fn(R.MESH, obj, [t[:, :13 * 6].contiguous() for t in reg], boxes)          # six columns: the class is always oriented
    with pytest.raises(ValueError):
        fn(R.MESH, obj, reg, boxes, sampled=flags.cpu())
    with pytest.raises(ValueError):
        fn(R.MESH, obj, reg, boxes[:1])
    five = M.AnchorGenerator3D(R.ANCHOR_SIZES + ((128,),), R.ASPECT_RATIOS[:1] * 5)
    with pytest.raises(ValueError):
        M.RPNIoULossComputation(five, R.FG, R.BG, R.BATCH, R.FRACTION)
    one = M.AnchorGenerator3D(((8,),), (((1., 1., 1.),),))
    many = M.RPNIoULossComputation(one, R.FG, R.BG, R.BATCH, R.FRACTION)
    with pytest.raises(ValueError):
        many((8, 8, 8), [torch.zeros((65, 1, 2, 2, 2)).cuda()], [torch.zeros((65, 8, 2, 2, 2)).cuda()], [torch.zeros((0, 7)).cuda()] * 65)
    with pytest.raises(ValueError):
        M.RPNIoULossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION, reg_loss_type="smooth_l1")
