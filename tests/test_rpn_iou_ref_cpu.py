"""The float64 restatement of the oriented RPN's IoU-type box losses (tests/_rpn_iou_ref.py) against tests/golden/g29_rpn_iou_loss.npz, recorded from
the reference's own delta_sp2bbox and RotatedIOULoss by tools/gen_golden_rpn_iou.py, and the conditions of the case generator that the GPU tests use.

The fixture holds float64 results rounded to fp32 (2^-24 = 6e-8 relative), evaluated on fp32 inputs that the restatement reads back exactly; when it was
recorded the restatement matched it to 4.4e-8 in the losses and 6.9e-8 of the gradients' max norm.  Bounds: 1e-6 relative on the summed losses,
assert_close(1e-5) on the gradients, 1e-5 on the decoded boxes relative to their largest coordinate."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_iou_ref as Q  # noqa: E402
from tests import _rpn_post_ref as P  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "g29_rpn_iou_loss.npz")


@pytest.fixture(scope="module")
def g29():
    return {k: v for k, v in np.load(GOLDEN).items()}


@pytest.fixture(scope="module")
def case():
    return Q.make_case()


def test_the_fixture_holds_the_rows_of_the_case_generator(g29, case):
    assert int(g29["seed"]) == Q.SEED and tuple(g29["nbox"]) == Q.NBOX and int(g29["flag_seed"]) == Q.FLAG_SEED
    deltas, anchors, boxes = Q.rows_of(case)
    assert torch.equal(torch.from_numpy(g29["index"]).long(), case["index"])
    assert torch.equal(torch.from_numpy(g29["deltas"]), deltas) and torch.equal(torch.from_numpy(g29["anchors"]), anchors) and torch.equal(torch.from_numpy(g29["boxes"]), boxes)
    assert g29["planted"].tolist() == [case["planted"][k] for k in Q.PLANTED]
    assert 64 <= deltas.shape[0] <= 128


def test_the_case_meets_the_generators_conditions_and_the_planted_branches_are_present(case):
    br = Q.check_case(case)         # margins >= 1e-3, >= 64 flagged positives, every level that has a positive, every required branch
    deltas, anchors, boxes = Q.rows_of(case)
    where = {int(i): r for r, i in enumerate(case["index"].tolist())}
    for name in Q.PLANTED:           # each planted row takes the branch it was planted for
        r = where[case["planted"][name]]
        want = {"size_hi": ("dw_hi", "dh_hi", "dd_hi"), "size_lo": ("dw_lo", "dh_lo", "dd_lo")}.get(name, (name,))
        assert all(bool(br[k][r]) for k in want), name
    # no row is the ill-conditioned one: (da, db) after the clamp stay 0.25 away from (0.5, -0.5) and (-0.5, 0.5)
    da, db = deltas[:, 6].clamp(-0.5, 0.5).double(), deltas[:, 7].clamp(-0.5, 0.5).double()
    assert float(torch.minimum(torch.hypot(da - 0.5, db + 0.5), torch.hypot(da + 0.5, db - 0.5)).min()) >= 0.25


@pytest.mark.parametrize("loss_type", Q.TYPES)
def test_restatement_against_the_recorded_reference(g29, loss_type):
    d = torch.from_numpy(g29["deltas"]).double().requires_grad_(True)
    anc, b = torch.from_numpy(g29["anchors"]).double(), torch.from_numpy(g29["boxes"]).double()
    if loss_type == Q.TYPES[0]:
        got, want = P.decode_obb(d.detach(), anc), torch.from_numpy(g29["proposals"]).double()
        assert float((got - want).abs().max() / want.abs().max()) <= 1e-5
    terms = Q.box_terms(d, anc, b, loss_type)
    terms.sum().backward()
    want = float(g29[loss_type + "_loss"])
    got = float(terms.sum().detach())
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert torch.isfinite(d.grad).all()
    assert_close(d.grad, torch.from_numpy(g29[loss_type + "_grad"]).double(), 1e-5, f"{loss_type} gradient")


def test_rows_without_overlap_have_no_centre_gradient_under_the_iou_types_but_one_under_giou_and_diou(g29, case):
    """Without BEV overlap, or disjoint in z, inter3d is 0 and the IoU types reduce to a function of the union, log(u3d + 1) or u3d / (u3d + 1): the gradient
    over the centre deltas is 0 and the one over the size deltas is not (the +1 smoothing keeps it); GIoU and DIoU pull the centre.  The reference's autograd
    leaves 1e-16 there, the rounding of the four midpoints' mean, which is the centre identically; the kernels give exactly 0 (tests/test_rpn_iou_gpu.py)."""
    where = {int(i): r for r, i in enumerate(case["index"].tolist())}
    rows = [where[case["planted"]["no_bev"]], where[case["planted"]["no_z"]]]
    for t in Q.TYPES:
        g = torch.from_numpy(g29[t + "_grad"])[rows]
        if t in ("iou", "linear_iou"):
            assert (g[:, :3].abs() <= 1e-12).all() and (g[:, 3:6].abs() > 1e-6).all(), t
        else:
            assert (g[:, :3].abs().sum(1) > 1e-4).all(), t


def test_losses_of_the_whole_case_and_its_degenerate_forms(case):
    obj = [t.double().requires_grad_(True) for t in case["obj"]]
    reg = [t.double().requires_grad_(True) for t in case["reg"]]
    a = case["assign"]
    lo, lr = Q.losses(obj, reg, case["flags"], a["matched"], case["boxes"], "giou")
    want_obj = R.losses(obj, reg, case["flags"], a["targets"])[0]
    assert lo.item() == want_obj.item() and lr.item() > 0
    (lo + lr).backward()
    go, gr = R.flatten_heads([t.grad for t in obj], [t.grad for t in reg], 8)
    assert (gr[case["flags"] != 1] == 0).all() and (gr[case["flags"] == 1].abs().sum(-1) > 0).all() and (go[case["flags"] == 0] == 0).all()
    none = torch.zeros_like(case["flags"])
    assert all(v.item() == 0 for v in Q.losses(obj, reg, none, a["matched"], case["boxes"], "iou"))
    empty = [case["boxes"][0], torch.zeros((0, 7))]
    l2 = Q.losses(obj, reg, case["flags"], a["matched"], empty, "iou")[1]
    only0 = case["flags"].clone()
    only0[1][only0[1] == 1] = 2       # the second scene's positives count as sampled, and contribute nothing
    assert l2.item() == Q.losses(obj, reg, only0, a["matched"], case["boxes"], "iou")[1].item()


def test_constructors():
    from nerf_mae_amd.rpn import AnchorGenerator3D, RegionProposalNetwork, RPNHead, RPNIoULossComputation, RPNLossComputation, NeRFRegionProposalNetwork
    gen = AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)
    head = RPNHead(16, 13, 1, rotate=True)
    args = (gen, head, R.FG, R.BG, 256, 0.5, dict(training=10, testing=10), dict(training=10, testing=10), 0.3)
    for t in Q.TYPES:
        net = RegionProposalNetwork(*args, rotated_bbox=True, reg_loss_type=t)
        assert type(net.loss) is RPNIoULossComputation and net.loss.reg_loss_type == t and net.loss.rotate
        assert list(net.state_dict()) == ["head." + k for k in head.state_dict()]
    assert type(RegionProposalNetwork(*args, rotated_bbox=True).loss) is RPNLossComputation
    with pytest.raises(ValueError):
        RegionProposalNetwork(*args, rotated_bbox=True, reg_loss_type="ciou")
    with pytest.raises(ValueError):
        RPNIoULossComputation(gen, R.FG, R.BG, 256, 0.5, reg_loss_type="smooth_l1")
    with pytest.raises(ValueError):
        RPNIoULossComputation(gen, 0.2, 0.35, 256, 0.5)               # bg above fg
    for t in ("iou", "giou"):
        with pytest.raises(NotImplementedError, match="RPNIoULossComputation"):
            RegionProposalNetwork(*args, rotated_bbox=False, reg_loss_type=t)
        with pytest.raises(NotImplementedError, match="RPNIoULossComputation"):
            RPNLossComputation(gen, R.FG, R.BG, 256, 0.5, rotated_bbox=True, reg_loss_type=t)

    class _Backbone(torch.nn.Module):
        out_channels = 16

    nerf = NeRFRegionProposalNetwork(_Backbone(), gen, RPNHead(16, 13, 1, rotate=True), rotated_bbox=True, reg_loss_type="diou")
    assert type(nerf.rpn.loss) is RPNIoULossComputation and nerf.rpn.loss.reg_loss_type == "diou"
    with pytest.raises(NotImplementedError):
        NeRFRegionProposalNetwork(_Backbone(), gen, RPNHead(16, 13, 1), reg_loss_type="diou")
