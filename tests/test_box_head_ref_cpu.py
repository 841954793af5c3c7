"""The float64 restatement of the box head (tests/_box_head_ref.py) against what the reference's own RCNN recorded (tests/golden/g32_box_head.npz,
tools/gen_golden_box_head.py), and everything of nerf_mae_amd.detector.FusedRCNN that needs no GPU: its parameter holders, its refusals and the C ABI."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _box_head_ref as B  # noqa: E402

CASES = [(size, *cfg) for size in B.G_SIZES for cfg in B.G_CONFIGS]
IDS = [B.golden_prefix(*c)[:-1] for c in CASES]


@pytest.fixture(scope="module")
def g32():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g32_box_head.npz")))


def _rel(a, b):
    return B.max_err(torch.as_tensor(a), torch.as_tensor(b))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restatement_reproduces_the_recorded_reference(g32, case):
    size, add_layer, flatten, rotated = case
    pre = B.golden_prefix(*case)
    x, P, cot_box, cot_cls = B.golden_case(*case)
    assert tuple(g32["geometry"]) == (B.G_C, B.G_M, B.G_NCLS)
    np.testing.assert_allclose(B.input_sums(x, P, cot_box, cot_cls), g32[pre + "input_sums"], rtol=0, atol=1e-12)      # the formula still fills what was recorded
    assert (x == 0).any() and (x < 0).any()
    res = B.run(x, P, add_layer, flatten, cot_box, cot_cls)
    assert list(res["dparam"]) == B.keys(add_layer)
    assert tuple(res["box"].shape) == (B.G_M, 7 if rotated else 6) and tuple(res["cls"].shape) == (B.G_M, B.G_NCLS)
    for name, got in (("box", res["box"]), ("cls", res["cls"]), ("dx", res["dx"])):
        assert _rel(got, g32[pre + name]) <= 1e-9, name
    for k, grad in res["dparam"].items():
        assert _rel(B.recorded_view(k, grad, flatten), g32[pre + "d_" + k]) <= 1e-9, k


@pytest.mark.parametrize("case", CASES[:8], ids=IDS[:8])
def test_rounding_hook_disabled_equals_the_plain_head_and_enabled_does_not(case):
    size, add_layer, flatten, rotated = case
    x, P, cot_box, cot_cls = B.golden_case(*case)
    plain = B.quantities(B.run(x, P, add_layer, flatten, cot_box, cot_cls))
    same = B.quantities(B.run(x, P, add_layer, flatten, cot_box, cot_cls, rnd=lambda t: t))
    assert list(plain) == list(same) and all(torch.equal(plain[k], same[k]) for k in plain)
    rounded = B.quantities(B.run(x, P, add_layer, flatten, cot_box, cot_cls, rnd=B.round_bf16))
    errs = {k: B.max_err(rounded[k], plain[k]) for k in plain}
    assert max(errs.values()) > 0, errs
    assert errs["d RCNN_bbox_pred.bias"] == 0 and errs["d RCNN_cls_score.bias"] == 0          # plain sums of the cotangents: no rounding reaches them
    none = B.run(x, P, add_layer, flatten, None, cot_cls)
    assert none["dparam"]["RCNN_bbox_pred.weight"] is None and none["dparam"]["RCNN_cls_score.weight"].abs().sum() > 0   # a None cotangent: that output is left out


@pytest.mark.parametrize("add_layer,flatten", [(a, f) for a in (False, True) for f in (False, True)])
def test_fused_head_has_the_stock_heads_parameters(add_layer, flatten):
    from nerf_mae_amd import detector as D
    for rotated in (False, True):
        torch.manual_seed(1)
        stock = D.RCNN(16, None, 3, (2, 3, 1), add_layer, rotated, flatten)
        torch.manual_seed(1)
        fused = D.FusedRCNN(16, None, 3, (2, 3, 1), add_layer, rotated, flatten)
        a, b = stock.state_dict(), fused.state_dict()
        assert list(a) == list(b) == B.keys(add_layer)
        assert {k: tuple(v.shape) for k, v in a.items()} == {k: tuple(v.shape) for k, v in b.items()} == B.shapes(16, (2, 3, 1), 3, add_layer, flatten, rotated)
        assert all(torch.equal(a[k], b[k]) for k in a), "the same default initialisation"
        other = D.RCNN(16, None, 3, (2, 3, 1), add_layer, rotated, flatten)
        fused.load_state_dict(other.state_dict(), strict=True)
        stock.load_state_dict(fused.state_dict(), strict=True)
        assert all(torch.equal(stock.state_dict()[k], other.state_dict()[k]) for k in a)
        assert fused.compute_dtype == torch.bfloat16 and D.FusedRCNN(16, None, 3, (2, 3, 1), compute_dtype=torch.float32).compute_dtype == torch.float32


def test_constructor_and_forward_refusals():
    from nerf_mae_amd import detector as D
    from nerf_mae_amd import ops
    with pytest.raises(NotImplementedError):
        D.FusedRCNN(12, None, 2, (3, 3, 3))                                     # C % 8
    for dtype in (torch.float16, torch.float64, None):
        with pytest.raises(TypeError):
            D.FusedRCNN(16, None, 2, (3, 3, 3), compute_dtype=dtype)
    assert ops.BOX_HEAD_MAX_COLS >= 7 + 9 and ops.BOX_HEAD_MAX_CELLS >= 7 ** 3
    D.FusedRCNN(16, None, ops.BOX_HEAD_MAX_COLS - 7, (7, 7, 7), is_rotated_bbox=True)
    D.FusedRCNN(16, None, 9, (8, 8, 8))
    with pytest.raises(ValueError):
        D.FusedRCNN(16, None, ops.BOX_HEAD_MAX_COLS - 6, (3, 3, 3), is_rotated_bbox=True)    # one class too many for 7 regression columns
    with pytest.raises(ValueError):
        D.FusedRCNN(16, None, 0, (3, 3, 3))
    with pytest.raises(ValueError):
        D.FusedRCNN(16, None, 2, (9, 8, 8))                                     # 576 cells
    with pytest.raises(ValueError):
        D.FusedRCNN(16, None, 2, (3, 3))
    with pytest.raises(ValueError):
        D.FusedRCNN(ops.BOX_HEAD_MAX_CHANNELS + 8, None, 2, (1, 1, 1))
    head = D.FusedRCNN(16, None, 2, (3, 3, 3), is_add_layer=True)
    with pytest.raises(RuntimeError, match="parameters on a HIP device"):
        head(torch.zeros(4, 16, 3, 3, 3))                                       # parameters on the host: no CPU fallback


def test_header_declares_the_box_head_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    for name in ("nmh_box_head_pack", "nmh_box_head_out_fwd", "nmh_box_head_bwd_ws_floats", "nmh_box_head_out_bwd", "nmh_box_head_colsum_ws_floats", "nmh_box_head_colsum",
                 "nmh_conv3d_k3_wgrad_fixed_ws_floats", "nmh_conv3d_k3_wgrad_fixed"):
        assert name in sigs, name
    assert [n for _, n in sigs["nmh_box_head_out_fwd"][1]][:8] == ["dt", "M", "S", "C", "reg_dim", "n_classes", "flatten", "relu"]
    assert sigs["nmh_box_head_bwd_ws_floats"][0] == "int64_t" and sigs["nmh_box_head_out_bwd"][0] == "int"
