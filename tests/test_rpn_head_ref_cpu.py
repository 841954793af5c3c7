"""The float64 restatement of the RPN head (tests/_rpn_head_ref.py) against outputs and gradients recorded from the reference's own RPNHead
(tests/golden/g23_rpn_head.npz, tools/gen_golden_rpn_head.py), the state_dict layout of NeRFRegionProposalNetwork(...).rpn against the recorded one,
the default constructor's conv_depth quirk, the rounding hook's placement, and the C ABI.  No GPU."""
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_head_ref as H  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402

NAMES = ("nmh_rpn_head_out_fwd", "nmh_rpn_head_bwd_ws_floats", "nmh_rpn_head_out_bwd", "nmh_relu_", "nmh_relu_bwd_")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g23_rpn_head.npz")))


class _Backbone(torch.nn.Module):
    out_channels = H.G_CIN


def _table(module):
    sd = module.state_dict()
    return list(sd.keys()), [list(v.shape) for v in sd.values()]


def test_header_declares_and_capi_defines_the_head_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    capi = open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "capi.hip")).read()
    for n in NAMES:
        assert n in sigs, n
        ret, args = sigs[n]
        assert re.search(r"^(int|int64_t)\s+" + n + r"\s*\(", capi, re.M), f"capi.hip does not define {n}"
        if n != "nmh_rpn_head_bwd_ws_floats":
            assert ret == "int" and args[-1] == ("void*", "stream"), (n, ret, args[-1])
    assert [a for _, a in sigs["nmh_rpn_head_out_fwd"][1][:8]] == ["dt", "nlevels", "level_vox", "N", "Cin", "A", "C", "relu"]
    assert [a for _, a in sigs["nmh_rpn_head_out_fwd"][1][-3:-1]] == ["objectness", "regression"]
    assert [a for _, a in sigs["nmh_rpn_head_out_bwd"][1][-7:-1]] == ["dt_out", "partials", "dw_cls", "dw_box", "db_cls", "db_box"]
    assert "rpn_head.hip" in open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("depth,rotate", H.G_CASES)
def test_restatement_against_the_recorded_reference(depth, rotate):
    feats, P, cot_obj, cot_reg, rec = H.golden_case(golden(), depth, rotate)
    out = H.run(feats, P, depth, cot_obj, cot_reg)
    C = 8 if rotate else 6
    assert [tuple(o.shape) for o in out["obj"]] == [(H.G_N, H.G_A, *g) for g in H.G_GRIDS]
    assert [tuple(r.shape) for r in out["reg"]] == [(H.G_N, H.G_A * C, *g) for g in H.G_GRIDS]
    for name in ("obj", "reg", "dfeat"):
        for i, (a, b) in enumerate(zip(out[name], rec[name])):
            assert a.shape == b.shape and H.max_err(a, b) < 1e-9, (name, i, H.max_err(a, b))
    assert list(rec["dparam"]) == H.keys(depth)
    for k, b in rec["dparam"].items():
        a = H.recorded_view(k, out["dparam"][k])
        assert a.shape == b.shape and H.max_err(a, b) < 1e-9, (k, H.max_err(a, b))
    assert any((f == 0).any() and (f < 0).any() for f in feats), "the recorded input must hold exact zeros and negatives"


def test_rounding_hook_rounds_what_the_kernels_store_and_nothing_else():
    feats, P, cot_obj, cot_reg, _ = H.golden_case(golden(), 2, True)
    exact, rounded = H.run(feats, P, 2, cot_obj, cot_reg), H.run(feats, P, 2, cot_obj, cot_reg, H.round_bf16)
    # the stored gradient of the input is a bf16 value; weight and bias gradients are not rounded; the error is of the size of a bf16 rounding
    for d in rounded["dfeat"]:
        assert torch.equal(d, H.round_bf16(d))
    assert not torch.equal(rounded["dparam"]["conv.0.weight"], H.round_bf16(rounded["dparam"]["conv.0.weight"]))
    e = max(H.max_err(rounded[n], exact[n]) for n in ("obj", "reg"))          # (a gradient can move by much more: one flipped ReLU mask moves a whole voxel's share)
    assert 1e-4 < e < 5e-2, e
    # an identity hook is the plain head, bit for bit
    same = H.run(feats, P, 2, cot_obj, cot_reg, lambda v: v)
    assert all(torch.equal(a, b) for n in ("obj", "reg", "dfeat") for a, b in zip(same[n], exact[n]))
    # conv_depth 0: the features reach the 1x1x1 convs without a ReLU (the reference's empty nn.Sequential)
    o0, _ = H.head(feats, H.golden_params(golden(), 0, False), 0)
    w, b = golden()["a_cls_logits.weight"].astype(np.float64), golden()["a_cls_logits.bias"].astype(np.float64)
    want = np.einsum("ncxyz,ac->naxyz", feats[0].numpy(), w.reshape(w.shape[0], -1)) + b[None, :, None, None, None]
    assert np.allclose(o0[0].numpy(), want, rtol=1e-12, atol=1e-12)


def test_state_dict_layout_equals_the_recorded_reference():
    from nerf_mae_amd.rpn import AnchorGenerator3D, NeRFRegionProposalNetwork, RegionProposalNetwork, RPNHead
    g = golden()
    gen = AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)
    net = NeRFRegionProposalNetwork(_Backbone(), gen, RPNHead(H.G_CIN, 13, 2, rotate=True), rotated_bbox=True)
    assert isinstance(net.rpn, RegionProposalNetwork)
    keys, shapes = _table(net.rpn)
    assert keys == g["rpn_keys"].tolist() and all(k.startswith("head.") for k in keys)
    assert shapes == [[v for v in row if v] for row in g["rpn_shapes"].tolist()]
    # the reference's initialisation: normal(0, 0.01) weights, zero biases
    for k, v in net.rpn.state_dict().items():
        if k.endswith("bias"):
            assert not v.any()
        elif v.numel() > 1000:
            assert 0.008 < float(v.std()) < 0.012 and abs(float(v.mean())) < 2e-3
    assert (net.rpn.pre_nms_top_n(), net.rpn.post_nms_top_n()) == (2000, 2000)
    net.eval()
    assert (net.rpn.pre_nms_top_n(), net.rpn.post_nms_top_n()) == (1000, 1000)


def test_default_constructor_puts_the_flag_into_conv_depth():
    from nerf_mae_amd.rpn import NeRFRegionProposalNetwork
    g = golden()
    for flag in (False, True):
        net = NeRFRegionProposalNetwork(_Backbone(), rotated_bbox=flag)
        keys, shapes = _table(net.rpn)
        assert keys == g[f"rpn{int(flag)}_keys"].tolist()
        assert shapes == [[v for v in row if v] for row in g[f"rpn{int(flag)}_shapes"].tolist()]
        assert net.rpn.head.conv_depth == int(flag) and net.rpn.head.bbox_pred.out_channels == 13 * 6 and net.check_targets is True
    with pytest.raises(ValueError):
        NeRFRegionProposalNetwork(torch.nn.Identity())
    with pytest.raises(TypeError):
        NeRFRegionProposalNetwork(_Backbone(), rpn_anchor_generator=object())


def test_constructor_errors():
    from nerf_mae_amd.rpn import AnchorGenerator3D, RegionProposalNetwork, RPNHead
    with pytest.raises(NotImplementedError):
        RPNHead(12, 3)
    with pytest.raises(ValueError):
        RPNHead(16, 33)
    head = RPNHead(16, 13, 0)
    assert len(head.conv) == 0 and list(head.state_dict()) == H.keys(0)
    gen = AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)
    with pytest.raises(NotImplementedError):
        RegionProposalNetwork(gen, head, 0.35, 0.2, 256, 0.5, dict(training=10, testing=10), dict(training=10, testing=10), 0.3, reg_loss_type="iou")
    with pytest.raises(RuntimeError):      # no CPU fallback
        head([torch.zeros(1, 16, 2, 2, 2)])
