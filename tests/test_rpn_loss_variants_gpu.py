"""Every box loss of the RPN with and without the 2-D projection term (reg_loss_2d of nerf_mae_amd.rpn.RPNLossComputation / RPNIoULossComputation over csrc/rpn.hip):
the switch must leave the first two losses and, without an upstream gradient for the third, every head gradient bit for bit as they are.

Settings: smooth-L1 with 6 and with 8 columns (the scenes of tests/_rpn_ref.make_scene with the recorded g20 flags) and iou, linear_iou, giou, diou (the scenes, heads and
flags of tests/_rpn_iou_ref.make_case).  Geometry: the g20 case, mesh 32^3, grids 8^3 .. 1^3, 5 anchors per location (2 x 2 925 anchors), 2 scenes, the second padded by ORI; the
8^3 level alone has 10 workgroups per scene, so the case has four levels, a padded scene and several partial rows per level.  The 2-D loss of iou, linear_iou and diou, which no other
test runs, is compared with the float64 restatement tests/_proj2d_ref.rpn_loss_2d under the project's contract for fp32, assert_close(rtol=1e-3), as
tests/test_rpn_proj2d_gpu.py does for the other three settings.  The losses and the objectness gradients are compared exactly, and so are the box gradients of the two
smooth-L1 settings: with no upstream gradient the backward's 2-D branch adds g * 0 to a finite box gradient, so the two runs agree in every bit as long as the gradients
are finite, which is asserted.  The box gradients of the four IoU types are NOT equal in every bit between the two runs: the backward of the decode and of the pair
geometry is free to contract (csrc/rpn_decode.hpp), and the compiler contracts it differently beside the 2-D term's own decode.  Both are fp32 evaluations of one
function, the run without the term is held to float64 by tests/test_rpn_iou_gpu.py, and the run with it is held to the run without it under the same contract,
assert_close(rtol=1e-3)."""
import functools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_iou_ref as Q  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests import test_rpn_proj2d_gpu as P  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

SETTINGS = ("aabb", "obb") + tuple(Q.TYPES)
W_REG = 0.7


@functools.lru_cache(maxsize=None)
def case(setting):
    """-> dict(rotated, loss_type, boxes, assign, flags, obj, reg), as tests/test_rpn_proj2d_gpu.case"""
    if setting in ("aabb", "obb"):
        return P.case(setting)
    c = Q.make_case()
    return dict(rotated=True, loss_type=setting, boxes=c["boxes"], assign=c["assign"], flags=c["flags"], obj=c["obj"], reg=c["reg"])


@functools.lru_cache(maxsize=None)
def run(setting, on):
    """the public class on the setting's fixed flags; backward of objectness + 0.7 box only -> (the three losses [3], the head gradients), on the host"""
    c = case(setting)
    heads = P._gpu_heads(c)
    out = P._fn(c, reg_loss_2d=on)(R.MESH, heads[0], heads[1], [b.cuda() for b in c["boxes"]], P._ori(), sampled=c["flags"].cuda())
    (out["loss_objectness"] + W_REG * out["loss_rpn_box_reg"]).backward()
    return P._keys(out).cpu(), [t.grad.cpu() for ts in heads for t in ts]


@pytest.mark.parametrize("setting", SETTINGS)
def test_the_2d_term_leaves_the_first_two_losses_and_their_gradients_bit_for_bit(setting):
    (l_off, g_off), (l_on, g_on) = run(setting, False), run(setting, True)
    assert torch.equal(l_off[0], l_on[0]) and torch.equal(l_off[1], l_on[1]), (setting, l_off.tolist(), l_on.tolist())
    assert l_off[0].item() > 0 and l_off[1].item() > 0 and l_off[2].item() == 0 and l_on[2].item() > 0
    if setting in ("iou", "linear_iou", "diou"):
        c = case(setting)
        want = P._ref_losses(c, [[t.double() for t in ts] for ts in (c["obj"], c["reg"])])[2]
        assert_close(l_on[2].reshape(1), want.reshape(1), 1e-3, f"{setting} 2-D loss")
    L = len(R.GRIDS)
    assert len(g_off) == len(g_on) == 2 * L
    for k, (a, b) in enumerate(zip(g_off, g_on)):
        assert torch.isfinite(a).all() and torch.isfinite(b).all(), (setting, k)
        if k < L or setting in ("aabb", "obb"):
            assert torch.equal(a, b), f"{setting}: head gradient {k} differs between the runs with and without the term"
        elif a.abs().sum() > 0:
            assert_close(b, a.double(), 1e-3, f"{setting} d pred_bbox_deltas level {k - L}, with the term against without")
        else:
            assert (b == 0).all()
    assert any((g != 0).any() for g in g_off[L:]), "the box loss reaches the regression head"


def test_linear_iou_against_iou_the_box_loss_differs_and_the_objectness_bits_do_not():
    for on in (False, True):
        (l_iou, _), (l_lin, _) = run("iou", on), run("linear_iou", on)
        assert torch.equal(l_iou[0], l_lin[0]) and l_iou[1].item() != l_lin[1].item(), (on, l_iou.tolist(), l_lin.tolist())
        assert torch.equal(l_iou[2], l_lin[2]), "the 2-D term does not depend on the box loss"
