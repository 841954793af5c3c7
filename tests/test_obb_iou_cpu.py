"""Host-side checks of the oriented-box IoU / NMS ops: the C ABI declares the five entries, the Python module imports without a GPU and
refuses CPU tensors and non-fp32 boxes, and the float64 restatement that the GPU tests are measured against (tests/_obb_iou_ref.py)
reproduces known answers, the Sutherland-Hodgman clip of tests/_rotated_ref.py, and the values and gradients recorded from the reference's
own Python (tests/golden/g17_obb_iou.npz, tools/gen_golden_obb_iou.py)."""
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

NAMES = ("nmh_obb_iou_fwd", "nmh_obb_iou_bwd", "nmh_obb_iou_pairwise", "nmh_obb_nms_mask", "nmh_obb_nms_scan")
G17 = os.path.join(ROOT, "tests", "golden", "g17_obb_iou.npz")


def box(*v):
    return torch.tensor([v], dtype=torch.float64)


def test_header_declares_the_obb_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    for n in NAMES:
        assert n in sigs, n
        ret, args = sigs[n]
        assert ret == "int" and args[-1] == ("void*", "stream"), (n, ret, args[-1])
    assert [a for _, a in sigs["nmh_obb_iou_fwd"][1][:4]] == ["mode", "box1", "box2", "npairs"]
    assert [a for _, a in sigs["nmh_obb_iou_bwd"][1][-3:-1]] == ["dbox1", "dbox2"]


def test_module_imports_and_refuses_cpu_and_non_fp32():
    from nerf_mae_amd import rotated_iou as M
    b = torch.tensor([[[0.0, 0, 0, 1, 1, 1, 0]]])
    flat, s = b[0], torch.tensor([1.0])
    calls = (lambda x: M.cal_iou_3d(x, x), lambda x: M.cal_iou_3d(x, x, verbose=True), lambda x: M.cal_giou_3d(x, x), lambda x: M.cal_diou_3d(x, x, "aligned"))
    for f in calls:
        with pytest.raises(RuntimeError):
            f(b)
        with pytest.raises(TypeError):
            f(b.double())
        with pytest.raises(TypeError):
            f(b.half())
    for f in (lambda x: M.box_iou_3d(x, x), lambda x: M.nms(x, s, 0.5), lambda x: M.batched_nms(x, s, torch.tensor([0]), 0.5)):
        with pytest.raises(RuntimeError):
            f(flat)
        with pytest.raises(RuntimeError):
            f(flat[:, :6].contiguous())
        with pytest.raises(TypeError):
            f(flat.double())
    with pytest.raises(NotImplementedError):
        M.cal_giou_3d(b, b, enclosing_type="pca")
    with pytest.raises(NotImplementedError):
        M.cal_diou_3d(b, b, enclosing_type="pca")


def test_restatement_shifted_unit_squares():
    r = R.paired(box(0, 0, 0, 1, 1, 1, 0), box(0.5, 0.5, 0, 1, 1, 1, 0))
    assert abs(r["inter2d"].item() - 0.25) < 1e-15
    assert abs(r["iou"].item() - 1.0 / 7.0) < 1e-15
    assert abs(r["u3d"].item() - 1.75) < 1e-15 and abs(r["z_range"].item() - 1.0) < 1e-15


def test_restatement_identical_boxes():
    b = torch.from_numpy(R.make_boxes(np.random.default_rng(3), 200)).double()
    assert (R.paired(b, b.clone())["iou"] - 1.0).abs().max().item() < 1e-12


def test_restatement_crossed_rectangles():
    r = R.paired(box(0.3, -0.2, 0, 2, 1, 1, 0), box(0.3, -0.2, 0, 2, 1, 1, math.pi / 2))
    assert abs(r["inter2d"].item() - 1.0) < 1e-12
    assert abs(r["iou"].item() - 1.0 / 3.0) < 1e-12


def test_restatement_disjoint_boxes_and_giou_by_hand():
    # 2 x 2 x 1 at the origin and 1 x 2 x 1 centred at x = 3: BEV gap 1.5, z ranges [-0.5, 0.5] and [0, 1]
    b1, b2 = box(0, 0, 0, 2, 2, 1, 0), box(3, 0, 0.5, 1, 2, 1, 0)
    for mode in ("giou_smallest", "giou_aligned"):
        r = R.paired(b1, b2, mode)
        assert r["iou"].item() == 0.0 and r["inter2d"].item() == 0.0
        assert abs(r["u3d"].item() - 6.0) < 1e-15
        # enclosing rectangle 4.5 x 2, z range 1.5: v_c = 13.5, loss = 1 - 0 + (13.5 - 6) / 13.5
        assert abs(r["w_c"].item() * r["h_c"].item() - 9.0) < 1e-12
        assert abs(r["loss"].item() - (1.0 + 7.5 / 13.5)) < 1e-12
    r = R.paired(b1, b2, "diou_aligned")
    assert abs(r["loss"].item() - (1.0 + 9.25 / (4.5 ** 2 + 2.0 ** 2 + 1.5 ** 2))) < 1e-12


def test_restatement_smallest_enclosing_of_a_rotated_pair():
    """two copies of a rotated rectangle, one shifted along its own long axis: the smallest enclosing rectangle is the rotated one"""
    th = 0.7
    b1 = box(0, 0, 0, 2, 1, 1, th)
    b2 = box(1.5 * math.cos(th), 1.5 * math.sin(th), 0, 2, 1, 1, th)
    r = R.paired(b1, b2, "giou_smallest")
    wh = sorted((r["w_c"].item(), r["h_c"].item()))
    assert abs(wh[0] - 1.0) < 1e-12 and abs(wh[1] - 3.5) < 1e-12
    assert abs(r["inter2d"].item() - 0.5) < 1e-12
    a = R.paired(b1, b2, "giou_aligned")
    assert a["w_c"].item() * a["h_c"].item() > 3.5 + 1e-3


def test_restatement_bev_area_against_clip():
    rng = np.random.default_rng(11)
    b1, b2 = R.make_boxes(rng, 2000).astype(np.float64), R.make_boxes(rng, 2000).astype(np.float64)
    got = R.inter2d(torch.from_numpy(b1), torch.from_numpy(b2)).numpy()
    want = np.array([R.clip_area(R.rect_corners(p[0], p[1], p[3], p[4], p[6]), R.rect_corners(q[0], q[1], q[3], q[4], q[6])) for p, q in zip(b1, b2)])
    assert np.abs(got - want).max() < 1e-12
    assert ((want == 0) == (got == 0)).all() and 0.02 < (want == 0).mean() < 0.5
    c = R.corners(torch.from_numpy(b1[:5])).numpy()
    for k in range(5):
        assert np.abs(c[k] - R.rect_corners(b1[k, 0], b1[k, 1], b1[k, 3], b1[k, 4], b1[k, 6])).max() < 1e-14


def test_restatement_reproduces_the_recorded_reference():
    g = np.load(G17)
    assert all(v.dtype == np.float32 for v in g.values()) and g["box1"].shape == (512, 7)
    rng = np.random.default_rng(17)
    assert np.array_equal(g["box1"], R.make_boxes(rng, 512)) and np.array_equal(g["box2"], R.make_boxes(rng, 512))
    for name, mode, key in (("iou", "iou", "iou"), ("giou_loss", "giou_smallest", "loss"), ("diou_loss", "diou_smallest", "loss")):
        p = torch.from_numpy(g["box1"]).double().requires_grad_(True)
        q = torch.from_numpy(g["box2"]).double().requires_grad_(True)
        v = R.paired(p, q, mode)[key]
        v.sum().backward()
        assert_close(v.detach(), torch.from_numpy(g[name]).double(), 1e-4, name)
        assert_close(p.grad, torch.from_numpy(g[f"grad_{name}_box1"]).double(), 1e-4, f"grad_{name}_box1")
        assert_close(q.grad, torch.from_numpy(g[f"grad_{name}_box2"]).double(), 1e-4, f"grad_{name}_box2")


def test_restatement_nms_chain():
    """A suppresses B, B would suppress C, A does not suppress C: A and C are kept"""
    boxes = torch.tensor([[0.0, 0, 0, 2, 1, 1, 0], [0.8, 0, 0, 2, 1, 1, 0], [1.6, 0, 0, 2, 1, 1, 0]], dtype=torch.float64)
    iou = R.pairwise(boxes, boxes)
    assert abs(iou[0, 1].item() - 1.2 / 2.8) < 1e-12 and abs(iou[0, 2].item() - 0.4 / 3.6) < 1e-12
    assert R.nms(iou, torch.tensor([0.9, 0.8, 0.7]), 0.3) == [0, 2]
    assert R.nms(iou, torch.tensor([0.7, 0.9, 0.8]), 0.3) == [1]
    assert R.nms(iou, torch.tensor([0.5, 0.5, 0.5]), 0.3) == [0, 2]                       # ties go to the lower index
    assert R.nms(iou, torch.tensor([0.9, 0.8, 0.7]), 0.3, cats=[0, 1, 0]) == [0, 1, 2]    # other categories do not suppress
    ab = torch.tensor([[0.0, 0, 0, 2, 2, 2], [1.0, 1, 1, 3, 3, 3]], dtype=torch.float64)
    assert abs(R.pairwise(ab, ab)[0, 1].item() - 1.0 / 15.0) < 1e-15
