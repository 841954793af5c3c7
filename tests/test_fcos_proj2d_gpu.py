"""The 2-D projection term of the FCOS regression loss on the GPU (nerf_mae_amd.fcos_loss.FCOSProj2dLossComputation over csrc/fcos.hip) against the float64
restatements tests/_fcos_ref.py and tests/_proj2d_ref.py (themselves checked against the recorded reference, tests/golden/g18_fcos_loss.npz and g30_proj2d.npz).
The geometry is that of tests/test_fcos_loss_gpu.py: three scenes (70, 1 and 0 boxes), four levels, center sampling 1.5, normalised targets, oriented boxes.
Tolerance: the project's contract for fp32, assert_close(rtol=1e-3); the decoded predictions lie voxels away from the decoded targets (far rows in the sense
of tests/test_proj2d_gpu.py)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_ref as F  # noqa: E402
from tests import _proj2d_ref as J  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [("iou", False, 0.5), ("iou", True, 2.0), ("giou", False, 2.0), ("giou", True, 0.5)]
WEIGHTS = (1.0, 0.7, 1.3)


def _m():
    from nerf_mae_amd import fcos_loss
    return fcos_loss


@functools.lru_cache(maxsize=None)
def scene():
    return tuple(F.make_scene(F.SEED[True], True))


@functools.lru_cache(maxsize=None)
def assignment():
    return F.assign(list(scene()), 1.5, True, orig=F.ORIG)


@functools.lru_cache(maxsize=None)
def ref(loss_type, add_l1, weight):
    """float64: the three losses with the 2-D part in reg_loss, the 2-D part on its own, and the gradients of 1.0 cls + 0.7 reg + 1.3 ctr in the dense layout"""
    a = assignment()
    heads = [[t.double().requires_grad_(True) for t in ts] for ts in F.make_heads(F.HEAD_SEED, True, True)]
    out = list(F.losses(*heads, a, loss_type, add_l1))
    part = J.fcos_reg_2d(heads[1], a, weight)
    out[1] = out[1] + part
    sum(w * o for w, o in zip(WEIGHTS, out)).backward()
    return [o.detach() for o in out], part.detach(), F.flatten_heads(*[[t.grad for t in ts] for ts in heads])


def _gpu_heads():
    return [[t.cuda().requires_grad_(True) for t in ts] for ts in F.make_heads(F.HEAD_SEED, True, True)]


def _sizes():
    return torch.tensor(F.ORIG, dtype=torch.int32).cuda()


def _run(fn, heads, boxes, backward=True):
    out = fn(None, heads[0], heads[1], heads[2], boxes, None, grid_sizes=_sizes())
    if backward:
        sum(w * o for w, o in zip(WEIGHTS, out)).backward()
    return out


@pytest.mark.parametrize("loss_type,add_l1,weight", CASES, ids=[f"{t}-l1{int(l)}-w{w}" for t, l, w in CASES])
def test_losses_and_gradients_against_float64_and_against_the_class_without_the_term(loss_type, add_l1, weight):
    M = _m()
    want, part, wgrads = ref(loss_type, add_l1, weight)
    boxes = [b.cuda() for b in scene()]
    heads = _gpu_heads()
    fn = M.FCOSProj2dLossComputation(list(F.STRIDES), 1.5, loss_type, True, 1, add_l1, weight)
    out = _run(fn, heads, boxes)
    tag = f"{loss_type}{' +l1' if add_l1 else ''} w {weight}"
    assert_close(torch.stack([o.detach() for o in out]).cpu(), torch.stack(want), 1e-3, f"{tag} losses")
    grads = F.flatten_heads(*[[t.grad.cpu() for t in ts] for ts in heads])
    for name, g, w in zip(("d box_cls", "d box_regression", "d centerness"), grads, wgrads):
        assert_close(g, w, 1e-3, f"{tag} {name}")
    a = assignment()
    off = ~(a["valid"] & (a["labels"] > 0))
    assert (grads[1][off] == 0).all() and (grads[1][~off].abs().sum(-1) > 0).all()
    # the class without the term: the same bits for cls and centerness, and the difference of the two reg losses is the float64 2-D part
    plain_heads = _gpu_heads()
    plain = _run(M.FCOSLossComputation(list(F.STRIDES), 1.5, loss_type, True, 1, True, add_l1), plain_heads, boxes)
    assert torch.equal(plain[0], out[0]) and torch.equal(plain[2], out[2])
    diff = out[1].item() - plain[1].item()
    assert float(part) > 100 * 2e-6 * abs(out[1].item()), "the 2-D part stands clear of the rounding of the sum"
    assert abs(diff - float(part)) <= 1e-3 * float(part) + 2e-6 * abs(out[1].item()), (diff, float(part))
    assert all(torch.equal(x.grad, y.grad) for x, y in zip(plain_heads[0] + plain_heads[2], heads[0] + heads[2]))
    again_heads = _gpu_heads()
    again = _run(fn, again_heads, boxes)
    assert all(torch.equal(x, y) for x, y in zip(again, out)) and all(torch.equal(x.grad, y.grad) for x, y in zip(again_heads[1], heads[1])), "two runs are bit-identical"


def test_the_weight_scales_the_2d_part_and_the_recorded_reference_agrees():
    M = _m()
    boxes = [b.cuda() for b in scene()]
    regs = []
    for w in (0.5, 2.0):
        heads = _gpu_heads()
        regs.append(_run(M.FCOSProj2dLossComputation(list(F.STRIDES), 1.5, "iou", True, 1, False, w), heads, boxes, backward=False)[1].item())
    heads = _gpu_heads()
    base = _run(M.FCOSLossComputation(list(F.STRIDES), 1.5, "iou", True, 1, True, False), heads, boxes, backward=False)[1].item()
    g = np.load(os.path.join(ROOT, "tests", "golden", "g30_proj2d.npz"))
    unit = float(g["fcos_2d_f64"]) / float(g["fcos_csum"])                 # the reference's compute_2d_projection_loss / sum of the centerness targets
    for w, r in zip((0.5, 2.0), regs):
        assert abs((r - base) - w * unit) <= 1e-3 * w * unit + 2e-6 * r, (w, r - base, w * unit)


def test_no_positives_gives_exact_zeros():
    M = _m()
    heads = _gpu_heads()
    empty = [torch.zeros((0, 7), device="cuda") for _ in range(3)]
    out = _run(M.FCOSProj2dLossComputation(list(F.STRIDES), 1.5, "giou", True, 1, True, 0.5), heads, empty)
    assert out[1].item() == 0 and out[2].item() == 0 and np.isfinite(out[0].item())
    assert all((t.grad == 0).all() for t in heads[1]) and all((t.grad == 0).all() for t in heads[2])


def test_world_size_divisors_on_one_process():
    """world_size enters only as the two divisors (the all-reduce of the two scalars needs a process group, which tests/test_dist_gpu.py covers for the plain class):
    the kernels are driven through the ops entries with world = 2, where reg_loss doubles and the cls / centerness normaliser halves"""
    from nerf_mae_amd import ops
    M = _m()
    boxes, offs = M._boxes("test", [b.cuda() for b in scene()], 7)
    plan = ops.FcosPlan(F.SIZES, F.STRIDES, 3)
    labels, targets, _, ctr_t, valid, scalars, partials = ops.fcos_assign(plan, boxes, offs, 7, _sizes(), None, 1.5, True)
    heads = [[t.cuda() for t in ts] for ts in F.make_heads(F.HEAD_SEED, True, True)]
    r1, c1 = ops.fcos_pos2d_fwd(plan, 0, True, 0.5, heads[1], heads[2], labels, targets, ctr_t, valid, scalars, 1.0, partials)
    r2, c2 = ops.fcos_pos2d_fwd(plan, 0, True, 0.5, heads[1], heads[2], labels, targets, ctr_t, valid, scalars, 2.0, partials)
    assert r2.item() == 2 * r1.item() and c2.item() == 2 * c1.item() and r1.item() > 0
    one = torch.ones(1, device="cuda")
    d1 = ops.fcos_pos2d_bwd(plan, 0, True, 0.5, heads[1], heads[2], labels, targets, ctr_t, valid, scalars, 1.0, one, one)
    d2 = ops.fcos_pos2d_bwd(plan, 0, True, 0.5, heads[1], heads[2], labels, targets, ctr_t, valid, scalars, 2.0, one, one)
    assert all(torch.equal(2 * a, b) for a, b in zip(d1[0] + d1[1], d2[0] + d2[1]))
    from nerf_mae_amd._lib import NmhError
    with pytest.raises(NmhError):               # six columns, and a negative weight
        ops.lib().call("nmh_fcos_pos2d_fwd", plan.L, plan.dims, plan.N, 6, 0, 0, 0.5, ops._ptr_table(heads[1], 4), ops._ptr_table(heads[2], 4), labels, targets, ctr_t, valid, scalars,
                       1.0, partials, r1, c1, None)
    with pytest.raises(NmhError):
        ops.fcos_pos2d_fwd(plan, 0, True, -1.0, heads[1], heads[2], labels, targets, ctr_t, valid, scalars, 1.0, partials)


def test_constructors():
    M = _m()
    with pytest.raises(ValueError):
        M.FCOSProj2dLossComputation(list(F.STRIDES), 1.5, "iou", True, 1, False, 0.0)
    with pytest.raises(NotImplementedError):
        M.FCOSProj2dLossComputation(list(F.STRIDES), 1.5, "smooth_l1", True, 1, False, 0.5)
    fn = M.FCOSProj2dLossComputation(list(F.STRIDES), 1.5, "diou", True, 2, True, 0.5)
    assert fn.use_obb and fn.world_size == 2 and fn.proj2d_loss_weight == 0.5 and fn.use_additional_l1_loss


def test_fcos_module_builds_the_class_trains_with_it_and_still_raises_for_axis_aligned_boxes():
    from nerf_mae_amd import fcos
    from tests import test_fcos_network_gpu as NT
    c = NT.train_ref(True)

    def args(obb, w):
        a = NT.make_args(obb)
        a.proj2d_loss_weight = w
        return a

    net = fcos.FCOSModule(args(True, 0.5), NT.C, list(NT.STRIDES))
    assert isinstance(net.loss_evaluator, _m().FCOSProj2dLossComputation) and net.loss_evaluator.proj2d_loss_weight == 0.5
    net.load_state_dict({"head." + k: v.float() for k, v in c["P"].items()}, strict=True)
    net = net.cuda().train()
    plain = NT.build(True, c["P"]).train()
    assert type(plain.loss_evaluator) is _m().FCOSLossComputation
    feats = [f.float().cuda().requires_grad_(True) for f in c["feats"]]
    boxes = [b.cuda() for b in c["boxes"]]
    losses = net(list(NT.ORI), feats, boxes)[2]
    base = plain(list(NT.ORI), [f.detach() for f in feats], boxes)[2]
    assert torch.equal(losses["loss_cls"], base["loss_cls"]) and torch.equal(losses["loss_centerness"], base["loss_centerness"])
    assert losses["loss_reg"].item() > base["loss_reg"].item() > 0
    losses["loss_reg"].backward()
    params = dict(net.head.named_parameters())
    assert torch.isfinite(params["bbox_pred.weight"].grad).all() and params["bbox_pred.weight"].grad.abs().sum().item() > 0
    assert all(torch.isfinite(f.grad).all() for f in feats)
    with pytest.raises(NotImplementedError):
        fcos.FCOSModule(args(False, 0.5), NT.C, list(NT.STRIDES))
    assert type(fcos.FCOSModule(args(True, 0.0), NT.C, list(NT.STRIDES)).loss_evaluator) is _m().FCOSLossComputation
