"""The float64 restatement of the 2-D projection loss (tests/_proj2d_ref.py) and the host side of nerf_mae_amd.proj2d against the reference's own results
recorded in tests/golden/g30_proj2d.npz (tools/gen_golden_proj2d.py), and the conditions that the planted rows of the GPU tests must meet.  No GPU."""
import ctypes
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
from tests import _rpn_iou_ref as Q  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402

ROW_CASES = [(ncols, res, n) for ncols in (6, 7) for res in (32, 160) for n in (J.N_ROWS, 1)]


@pytest.fixture(scope="module")
def g30():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g30_proj2d.npz")))


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize("res", (32, 160))
def test_cameras_against_the_reference(g30, res):
    want = torch.from_numpy(g30[f"w2c_{res}"]).double()
    assert float((J.w2cs(res) - want).abs().max()) <= 1e-6 * max(1.0, float(want.abs().max()))
    # the four positions, in the reference's order: c2w = inv(w2c)
    pos = torch.linalg.inv(J.w2cs(res))[:, :3, 3]
    assert torch.allclose(pos, torch.tensor([[1.5, 1.5, 1.5], [1.5, -0.5, 1.5], [-0.5, 1.5, 1.5], [-0.5, -0.5, 1.5]], dtype=J.F64) * res)


@pytest.mark.parametrize("res", (32, 160))
def test_fused_cameras_of_the_package_and_of_the_library(g30, res):
    from nerf_mae_amd import proj2d
    from nerf_mae_amd._lib import lib
    want = torch.tensor(J.K, dtype=J.F64) @ torch.from_numpy(g30[f"w2c_{res}"]).double()[:, :3]
    got = proj2d.proj2d_cameras(res)
    assert got.dtype == torch.float32 and tuple(got.shape) == (4, 3, 4) and not got.is_cuda
    assert float((got.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())
    assert torch.equal(got, J.cameras(res).float()), "one rounding of the float64 product"
    buf = (ctypes.c_float * 48)()
    lib().call("nmh_proj2d_cameras", float(res), buf)                     # host only: what the FCOS entries build for res 160
    host = torch.tensor(list(buf)).reshape(4, 3, 4)
    assert float((host.double() - J.cameras(res)).abs().max()) <= 2e-7 * float(want.abs().max())
    with pytest.raises(Exception):
        lib().call("nmh_proj2d_cameras", 0.0, buf)


@pytest.mark.parametrize("ncols,res,n", ROW_CASES)
def test_rows_meet_the_generator_conditions(ncols, res, n):
    pred, target, where = J.make_rows(ncols, res, n)
    assert pred.dtype == torch.float32 and tuple(pred.shape) == (n, ncols) and sum(len(v) for v in where.values()) == n
    d = J.differences(pred.double(), target.double(), res)
    for group, rows in where.items():
        for k in rows:
            assert J.branch_ok(group, d[k]), (group, k)
    if n > 1:
        assert len(where["far"]) >= 20 and len(where["near"]) >= 20 and len(where["mixed"]) >= 20 and len(where["exact"]) == 1
        assert torch.equal(pred[where["exact"]], target[where["exact"]])
        corner = (J.points(pred.double()) - J.points(target.double())).norm(dim=-1)          # [2, n]
        far = corner[:, where["far"]]
        assert 0.4 <= float(far.min()) and float(far.max()) <= 4.1


@pytest.mark.parametrize("ncols,res,n", ROW_CASES)
def test_points_projections_terms_and_gradients_against_the_reference(g30, ncols, res, n):
    pred, target, _ = J.make_rows(ncols, res, n)
    tag = f"r{ncols}_{res}_{n}"
    cams = torch.tensor(J.K, dtype=J.F64) @ torch.from_numpy(g30[f"w2c_{res}"]).double()[:, :3]          # the reference's own fp32 cameras
    pts = J.points(pred.double())
    if ncols == 7:
        assert _rel(pts.reshape(-1, 3), torch.from_numpy(g30[tag + "_pts"])) <= 1e-12
    uv = J.project(cams, pts).reshape(-1, 2)                                    # camera-major, then point, then row: the reference's cat order
    assert _rel(uv, torch.from_numpy(g30[tag + "_uv"])) <= 1e-9
    p = pred.double().requires_grad_(True)
    T = J.terms(p, target.double(), res, cams)
    T.sum().backward()
    t64, g64 = torch.from_numpy(g30[tag + "_t64"]), torch.from_numpy(g30[tag + "_g64"])
    assert float((T.detach() - t64).abs().max()) <= 1e-9 * float(t64.abs().max())
    assert float((p.grad - g64).abs().max()) <= 1e-9 * float(g64.abs().max())
    # the unrounded cameras of the restatement change nothing that a test could see
    assert float((J.terms(pred.double(), target.double(), res) - t64).abs().max()) <= 1e-5 * float(t64.abs().max())


def test_package_points_on_the_host_formula(g30):
    pred, _, _ = J.make_rows(7, 32, J.N_ROWS)
    from nerf_mae_amd import proj2d
    with pytest.raises(RuntimeError):
        proj2d.proj2d_points(pred)                      # no CPU path
    with pytest.raises(TypeError):
        proj2d.proj2d_terms(pred.double(), pred.double(), 32)


def test_fcos_form_against_the_reference(g30):
    asg = F.assign(F.make_scene(F.SEED[True], True), 1.5, True, orig=F.ORIG)
    assert asg["npos"] == int(g30["fcos_npos"]) and abs(asg["csum"] - float(g30["fcos_csum"])) <= 1e-12 * asg["csum"]
    reg = [t.double() for t in F.make_heads(F.HEAD_SEED, True, True)[1]]
    got = float(J.fcos_reg_2d(reg, asg, 1.0)) * asg["csum"]                   # the reference's function stops before the division by sum ct
    assert abs(got - float(g30["fcos_2d_f64"])) <= 1e-6 * got
    assert abs(got - float(g30["fcos_2d_f32"])) <= 1e-3 * got


@pytest.mark.parametrize("name", ("aabb", "obb", "iou"))
def test_rpn_form_against_the_reference(g30, name):
    if name == "iou":
        case = Q.make_case()
        boxes, a, flags, obj, reg = case["boxes"], case["assign"], case["flags"], case["obj"], case["reg"]
    else:
        rotated = name == "obb"
        boxes = R.make_scene(R.SEED[rotated], rotated=rotated, ori=R.ORI)
        a = R.assign(boxes, ori=R.ORI, rotated=rotated)
        g20 = np.load(os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz"))
        flags = torch.from_numpy(g20[("o_" if rotated else "a_") + "flags"])
        obj, reg = R.make_heads(R.HEAD_SEED, len(R.NBOX), 8 if rotated else 6)
    got = float(J.rpn_loss_2d([t.double() for t in obj], [t.double() for t in reg], flags, a["matched"], boxes, R.MESH, a["valid"]))
    want = float(g30[f"rpn_{name}_2d"])
    assert abs(got - want) <= 1e-3 * want, (got, want)
