"""The float64 restatement of the FCOS head (tests/_fcos_head_ref.py) against outputs and gradients recorded from the reference's own FCOSHead
(tests/golden/g24_fcos_head.npz, tools/gen_golden_fcos_head.py), its GroupNorm against torch.nn.functional.group_norm, the rounding hook's placement, the
module's state_dict layout, initialisation and constructor errors, and the C ABI.  No GPU."""
import functools
import math
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_head_ref as H  # noqa: E402

NAMES = ("nmh_fcos_gn_ws_doubles", "nmh_fcos_gn_stats", "nmh_fcos_gn_apply", "nmh_fcos_gn_bwd", "nmh_fcos_head_out_fwd", "nmh_fcos_head_pack_ws_floats",
         "nmh_fcos_head_out_bwd_pack", "nmh_fcos_head_wgrad_ws_floats", "nmh_fcos_head_out_wgrad")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g24_fcos_head.npz")))


def test_header_declares_and_capi_defines_the_head_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    capi = open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "capi.hip")).read()
    header = open(os.path.join(ROOT, "include", "nerfmae_hip.h")).read()
    for n in NAMES:
        assert n in sigs, n
        ret, args = sigs[n]
        assert re.search(r"^(int|int64_t)\s+" + n + r"\s*\(", capi, re.M), f"capi.hip does not define {n}"
        if not n.endswith(("_ws_doubles", "_ws_floats")):
            assert ret == "int" and args[-1] == ("void*", "stream"), (n, ret, args[-1])
    assert "fcos/fcos.py:26-139" in header and "fcos.py:123-137" in header or "fcos.py:126-130" in header, "the entries cite the reference op"
    assert "fcos_head.hip" in open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("use_obb,ctr_on_reg,training", H.G_CASES)
def test_restatement_against_the_recorded_reference(use_obb, ctr_on_reg, training):
    feats, P, cots, mode, rec = H.golden_case(golden(), use_obb, ctr_on_reg, training)
    out = H.run(feats, P, H.G_CONVS, ctr_on_reg, mode, H.G_STRIDES, cots)
    nreg = 8 if use_obb else 6
    assert [tuple(r.shape) for r in out["reg"]] == [(H.G_N, nreg, *g) for g in H.G_GRIDS]
    for name in ("cls", "reg", "ctr", "dfeat"):
        for i, (a, b) in enumerate(zip(out[name], rec[name])):
            assert a.shape == b.shape and H.max_err(a, b) < 1e-9, (name, i, H.max_err(a, b))
    assert list(rec["dparam"]) == [k for k in H.keys(H.G_CONVS) if not k.startswith("scales.") or int(k.split(".")[1]) < len(H.G_GRIDS)]
    for k, b in rec["dparam"].items():
        a = H.recorded_view(k, out["dparam"][k])
        assert a.shape == b.shape and H.max_err(a, b) < 1e-9, (k, H.max_err(a, b))
    assert any((f == 0).any() and (f < 0).any() for f in feats), "the recorded input must hold exact zeros and negatives"
    assert min(float(P[f"scales.{i}.scale"]) for i in range(len(H.G_GRIDS))) < 0 and all(float(P[f"scales.{i}.scale"]) != 1 for i in range(len(H.G_GRIDS)))
    assert float((P["cls_tower.1.weight"] - 1).abs().max()) > 0.1 and float(P["cls_tower.1.bias"].abs().max()) > 0.1, "non-trivial GroupNorm affine parameters"
    w = P["cls_tower.0.weight"]
    assert torch.equal(w, H.round_bf16(w)), "the recorded weights are bf16-exact"


def test_group_norm_against_torch_at_8_channels_per_group():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((3, 256, 4, 3, 2), generator=g, dtype=torch.float64) * 3 + 1.5
    gamma, beta = torch.randn(256, generator=g, dtype=torch.float64), torch.randn(256, generator=g, dtype=torch.float64)
    x.requires_grad_(True)
    a = H.group_norm(x, gamma, beta)
    b = torch.nn.functional.group_norm(x, 32, gamma, beta, 1e-5)
    assert H.max_err(a, b) < 1e-12
    cot = torch.randn(a.shape, generator=g, dtype=torch.float64)
    ga, = torch.autograd.grad((a * cot).sum(), x)
    gb, = torch.autograd.grad((b * cot).sum(), x)
    assert H.max_err(ga, gb) < 1e-10


def test_rounding_hook_rounds_what_the_kernels_store_and_nothing_else():
    feats, P, cots, mode, _ = H.golden_case(golden(), True, False, True)
    args = (feats, P, H.G_CONVS, False, mode, H.G_STRIDES, cots)
    exact, rounded = H.run(*args), H.run(*args, H.round_bf16)
    for d in rounded["dfeat"]:
        assert torch.equal(d, H.round_bf16(d))
    assert not torch.equal(rounded["dparam"]["cls_logits.weight"], H.round_bf16(rounded["dparam"]["cls_logits.weight"]))
    e = max(H.max_err(rounded[n], exact[n]) for n in ("cls", "reg", "ctr"))
    assert 1e-4 < e < 5e-2, e
    same = H.run(*args, lambda v: v)          # an identity hook is the plain head, bit for bit
    assert all(torch.equal(a, b) for n in ("cls", "reg", "ctr", "dfeat") for a, b in zip(same[n], exact[n]))
    assert all(torch.equal(same["dparam"][k], exact["dparam"][k]) for k in exact["dparam"])
    # the branches of the epilogue
    u = torch.tensor([[-2.0, 1.0, 3.0, -1.0, 2.0, 0.5, -4.0, 5.0]], dtype=torch.float64).view(1, 8, 1, 1, 1)
    assert H.epilogue(u, torch.tensor([-1.0]).double(), "train", 4).flatten().tolist() == [2.0, 0.0, 0.0, 1.0, 0.0, 0.0, 4.0, -5.0]
    assert H.epilogue(u, torch.tensor([2.0]).double(), "eval", 4).flatten().tolist() == [0.0, 8.0, 24.0, 0.0, 16.0, 4.0, -8.0, 10.0]
    assert torch.equal(H.epilogue(u, torch.tensor([0.5]).double(), "exp", 4), torch.exp(u * 0.5))


def _args(**kw):
    d = dict(num_convs=1, norm_reg_targets=True, centerness_on_reg=True, rotated_bbox=False, pre_nms_thresh=0.0, pre_nms_top_n=100, nms_thresh=0.3, fpn_post_nms_top_n=50,
             min_size=0.0, center_sampling_radius=1.5, iou_loss_type="iou", use_additional_l1_loss=False, proj2d_loss_weight=0.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def test_state_dict_layout_initialisation_and_errors():
    from nerf_mae_amd.fcos import FCOSHead, FCOSModule, FCOSOverNeRF, Scale
    for convs, obb in ((0, False), (1, True), (4, False)):
        head = FCOSHead(64, convs, [4, 8, 16, 32], use_obb=obb)
        sd = head.state_dict()
        assert list(sd) == H.keys(convs)
        assert {k: tuple(v.shape) for k, v in sd.items()} == H.shapes(convs, 64, 8 if obb else 6)
        for k, v in sd.items():
            if k == "cls_logits.bias":
                assert abs(float(v) + math.log(99)) < 1e-6
            elif k.startswith("scales.") or (("tower" in k) and int(k.split(".")[1]) % 3 == 1 and k.endswith("weight")):
                assert (v == 1).all()
            elif k.endswith("bias"):
                assert not v.any()
            elif v.numel() > 1000:
                assert 0.008 < float(v.std()) < 0.012 and abs(float(v.mean())) < 2e-3
    head = FCOSHead(H.G_C, H.G_CONVS, list(H.G_STRIDES), use_obb=True)
    head.load_state_dict({k: v.float() for k, v in H.golden_params(golden(), True).items()}, strict=True)       # a reference checkpoint loads strictly
    assert isinstance(head.scales[0], Scale) and head.scales[1].scale.item() == H.G_SCALES[1]
    with pytest.raises(NotImplementedError):
        FCOSHead(48, 1, [4, 8])
    with pytest.raises(TypeError):
        FCOSHead(64, 1, [4, 8], compute_dtype=torch.float16)
    with pytest.raises(RuntimeError):          # no CPU fallback
        head([torch.zeros(1, 64, 2, 2, 2)])
    mod = FCOSModule(_args(), 64, [4, 8, 16, 32])
    assert all(k.startswith("head.") for k in mod.state_dict()) and [k[5:] for k in mod.state_dict()] == H.keys(1)
    with pytest.raises(ValueError):
        FCOSOverNeRF(_args(), torch.nn.Identity(), [4, 8, 16, 32])
    # compute_locations and compute_padding_masks: the reference's semantics (fcos.py:272-320)
    loc = mod.compute_locations_per_level(2, 1, 3, 8, "cpu")
    assert loc.tolist() == [[4.0, 4.0, 4.0], [4.0, 4.0, 12.0], [4.0, 4.0, 20.0], [12.0, 4.0, 4.0], [12.0, 4.0, 12.0], [12.0, 4.0, 20.0]]
    m = mod.compute_padding_masks([loc], [(16, 8, 24), (12, 8, 12)])
    assert m[0].tolist() == [[True] * 6, [True, False, False, False, False, False]]
    assert mod.compute_padding_masks([loc], [(16, 8, 24), (12, 8, 12)])[0] is m[0], "cached per feature size and scene sizes"
