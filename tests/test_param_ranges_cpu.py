"""finetune.param_ranges and its rule builders on the host (CPU tensors for the table), and the range table in the resume section.

  small      an nn.Sequential whose flat layout is written out below: first-match order, None falling through to a later rule, merging, padding
  encoder    build_model("swin_t", resolution=32): the layer ids and scales of layer_decay_rules, the set of no_decay_rules
  refusals   an unmatched rule, a negative scale, no encoder
  resume     trainer.resume_section / restore_resume: the table is written, read back through torch.save / load, and a mismatch raises"""
import functools
import os
import re
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

CPU = torch.device("cpu")


def small():
    """parameters, [offset, numel] on 8-element granules: 0.weight [0, 15], 0.bias [16, 3], 1.weight [24, 3], 1.bias [32, 3], 2.weight [40, 6], 2.bias [48, 2];
    56 elements"""
    from nerf_mae_amd.finetune import FlatParameters
    torch.manual_seed(0)
    m = nn.Sequential(nn.Linear(5, 3), nn.LayerNorm(3), nn.Linear(3, 2))
    return m, FlatParameters(m, CPU)


@functools.lru_cache(maxsize=None)
def encoder():
    from nerf_mae_amd.model import build_model
    torch.manual_seed(0)
    m = build_model("swin_t", resolution=32, compute_dtype=torch.float32)
    m.flatten_parameters(CPU)
    return m


def scales_by_name(flat, table):
    """{name: (lr_scale, wd_scale)}; asserts that every parameter, its granule padding included, lies in ONE range"""
    from nerf_mae_amd.trainer import flat_layout
    b, out = table.record["bounds"], {}
    for name, (off, numel) in flat_layout(flat).items():
        r = max(i for i in range(len(b) - 1) if b[i] <= off)
        assert off + (numel + 7) // 8 * 8 <= b[r + 1], name
        out[name] = tuple(table.record["scale"][r])
    return out


def test_first_match_none_fall_through_merging_and_padding():
    from nerf_mae_amd.finetune import param_ranges
    m, flat = small()
    rules = [("0.", 0.5, None),                         # lr of all of layer 0; leaves wd to a later rule
             ("0.bias", 0.25, 0.0),                     # its lr comes too late for 0.bias (the first match holds), its wd is the first stated
             (lambda n, p: p.dim() <= 1, None, 0.0),    # wd 0 for the remaining 1-D parameters
             (m[2], 1.0, None)]                         # a sub-module; states the default
    t = param_ranges(flat, rules)
    assert t.record == {"bounds": [0, 16, 24, 40, 48, 56], "scale": [[0.5, 1.0], [0.5, 0.0], [1.0, 0.0], [1.0, 1.0], [1.0, 0.0]]}
    # 0.weight has 15 elements: its range runs to 16, the padding joined; 1.weight and 1.bias (24 .. 40) are one range
    assert t.bounds.dtype == torch.int64 and t.bounds.tolist() == t.record["bounds"] and t.bounds.device == flat._flat.device
    assert t.scale.dtype == torch.float32 and t.scale.tolist() == t.record["scale"]
    assert scales_by_name(flat, t) == {"0.weight": (0.5, 1.0), "0.bias": (0.5, 0.0), "1.weight": (1.0, 0.0), "1.bias": (1.0, 0.0), "2.weight": (1.0, 1.0),
                                       "2.bias": (1.0, 0.0)}
    # equal neighbours merge down to one range
    one = param_ranges(flat, [("", 1.0, 1.0)])
    assert one.record == {"bounds": [0, 56], "scale": [[1.0, 1.0]]}
    # the order decides
    swapped = param_ranges(flat, [("0.bias", 0.25, 0.0), ("0.", 0.5, None)])
    assert scales_by_name(flat, swapped)["0.bias"] == (0.25, 0.0) and scales_by_name(flat, swapped)["0.weight"] == (0.5, 1.0)


def test_rules_on_the_encoder_first_match_and_merging():
    from nerf_mae_amd.finetune import freeze_rules, param_ranges
    m = encoder()
    t = param_ranges(m, freeze_rules(m.patch_partition, "mask_token") + [("stages.0.", 0.5, None), ("stages.", 0.25, 0.5)])
    s = scales_by_name(m, t)
    assert s["mask_token"] == (0.0, 1.0) and s["patch_partition.0.weight"] == (0.0, 1.0)
    assert s["stages.0.0.norm1.weight"] == (0.5, 0.5) and s["stages.1.0.norm.weight"] == (0.25, 0.5) and s["decoder1.transp_conv.weight"] == (1.0, 1.0)
    # mask_token and the patch embed lead the buffer with one setting, stage 0, the other stages and the tail follow: four ranges for 202 tensors
    assert t.record["bounds"][0] == 0 and t.record["bounds"][-1] == m._flat.numel() and len(t.record["scale"]) == 4
    assert all(b % 8 == 0 for b in t.record["bounds"])


def test_layer_decay_ids_and_scales():
    from nerf_mae_amd.finetune import layer_decay_rules, layer_ids, param_ranges
    from nerf_mae_amd.model import PatchMerging3D, SwinBlock3D
    m = encoder()
    L = sum(isinstance(x, SwinBlock3D) for st in m.stages for x in st)
    assert L == 12
    ids = layer_ids(m)
    assert ids[id(m.mask_token)] == 0 and all(ids[id(p)] == 0 for p in m.patch_partition.parameters())
    k = 0
    for st in m.stages:
        first = k + 1
        for mod in st:
            if isinstance(mod, SwinBlock3D):
                k += 1
                assert all(ids[id(p)] == k for p in mod.parameters())
            else:
                assert isinstance(mod, PatchMerging3D) and all(ids[id(p)] == first for p in mod.parameters())
    assert k == L
    tail = [p for n, p in m.named_parameters() if n.startswith(("decoder", "out."))]
    assert tail and all(id(p) not in ids for p in tail)                           # id L + 1: no entry, scale 1
    s = scales_by_name(m, param_ranges(m, layer_decay_rules(m, 0.75)))
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    for name, p in m.named_parameters():
        if name in s:
            assert s[name] == (f32(0.75 ** (L + 1 - ids.get(id(p), L + 1))), 1.0), name
    assert s["mask_token"][0] == f32(0.75 ** 13) and s["stages.3.2.norm2.weight"][0] == f32(0.75) and s["out.conv.weight"][0] == 1.0
    assert s["stages.1.0.norm.weight"][0] == s["stages.1.1.norm1.weight"][0] == f32(0.75 ** (13 - 3))      # the merging layer with its stage's first block


def test_layer_decay_finds_the_encoder_inside_a_wrapper():
    from nerf_mae_amd.finetune import layer_decay_rules
    m = encoder()
    wrap = nn.Sequential()
    wrap.add_module("base", m)
    assert len(layer_decay_rules(wrap, 0.9)) == len(layer_decay_rules(m, 0.9)) == 13      # ids 0 .. 12; id 13 needs no rule


def test_recipe_on_a_downstream_model_whose_encoder_has_no_mask_token():
    """the detectors' backbone drops mask_token; everything behind the encoder (the FPN neck, the FCOS head) has layer id L + 1, and fcos.Scale is not decayed"""
    from nerf_mae_amd.finetune import FlatParameters, param_ranges, recipe_rules
    from tests import _finetune_common as C
    m = C.fcos_model()
    flat = FlatParameters(m, CPU)
    assert not any(n.endswith("mask_token") for n, _ in m.named_parameters())
    s = scales_by_name(flat, param_ranges(flat, recipe_rules(m, layer_decay=0.75, no_decay=True, freeze=(m.backbone.base.patch_partition,))))
    f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
    assert s["backbone.base.patch_partition.0.weight"] == (0.0, 1.0) and s["backbone.base.patch_partition.0.bias"] == (0.0, 0.0)
    assert s["backbone.base.stages.0.0.norm1.weight"] == (f32(0.75 ** 12), 0.0) and s["backbone.base.stages.3.2.mlp.0.weight"] == (f32(0.75), 1.0)
    outside = {n: v for n, v in s.items() if not n.startswith("backbone.base.")}
    assert outside and all(v[0] == 1.0 for v in outside.values())
    scales = [n for n in outside if n.startswith("fcos_module.head.scales.")]
    assert scales and all(outside[n] == (1.0, 0.0) for n in scales)


def test_no_decay_selects_exactly_its_set():
    from nerf_mae_amd.finetune import no_decay_rules, param_ranges
    m = encoder()
    s = scales_by_name(m, param_ranges(m, no_decay_rules(m)))
    want = {n: (1.0, 0.0 if (p.dim() <= 1 or n.endswith("relative_position_bias_table") or n == "mask_token") else 1.0)
            for n, p in m.named_parameters() if n in s}
    assert s == want
    assert sum(n.endswith("relative_position_bias_table") for n in s) == 12 and any(v == (1.0, 1.0) for v in s.values())
    small_m, flat = small()
    assert scales_by_name(flat, param_ranges(flat, no_decay_rules(small_m))) == {"0.weight": (1.0, 1.0), "0.bias": (1.0, 0.0), "1.weight": (1.0, 0.0),
                                                                                "1.bias": (1.0, 0.0), "2.weight": (1.0, 1.0), "2.bias": (1.0, 0.0)}


def test_refusals():
    from nerf_mae_amd.finetune import FlatParameters, freeze_rules, layer_decay_rules, param_ranges
    m, flat = small()
    with pytest.raises(ValueError, match="matches no parameter"):
        param_ranges(flat, [("0.", 0.5, None), ("3.", 0.5, None)])                # a typo must not silently train everything
    with pytest.raises(ValueError, match="matches no parameter"):
        param_ranges(flat, [(lambda n, p: False, 0.5, None)])
    with pytest.raises(ValueError, match="finite and >= 0"):
        param_ranges(flat, [("0.", -0.5, None)])
    with pytest.raises(ValueError, match="finite and >= 0"):
        param_ranges(flat, [("0.", None, float("nan"))])
    with pytest.raises(ValueError, match="SwinTransformer_MAE3D_New"):
        layer_decay_rules(m, 0.75)
    # what exclude= left out of the buffers is not there to be frozen a second time
    torch.manual_seed(0)
    m2 = nn.Sequential(nn.Linear(5, 3), nn.LayerNorm(3), nn.Linear(3, 2))
    part = FlatParameters(m2, CPU, exclude=(m2[0],))
    with pytest.raises(ValueError, match="matches no parameter"):
        param_ranges(part, freeze_rules(m2[0]))
    assert param_ranges(part, freeze_rules(m2[1])).record["scale"] == [[0.0, 1.0], [1.0, 1.0]]


def test_max_ranges_is_the_header_value():
    from nerf_mae_amd import ops
    from nerf_mae_amd._lib import HEADER
    assert ops.ADAMW_MAX_RANGES == int(re.search(r"#define\s+NMH_ADAMW_MAX_RANGES\s+(\d+)", open(HEADER).read()).group(1))


def test_resume_section_carries_the_table_and_a_mismatch_raises(tmp_path):
    from nerf_mae_amd.finetune import freeze_rules, no_decay_rules, param_ranges
    from nerf_mae_amd.trainer import FusedAdamW, resume_section, restore_resume
    m, flat = small()
    table = param_ranges(flat, no_decay_rules(m) + freeze_rules("0."))
    other = param_ranges(flat, no_decay_rules(m))
    opt = FusedAdamW(flat, ranges=table)
    opt.m.uniform_(), opt.v.uniform_()
    opt.t = 3
    path = str(tmp_path / "r.pt")
    torch.save({"resume": resume_section(flat, opt, step=3)}, path)
    r = torch.load(path, map_location="cpu", weights_only=True)["resume"]
    assert r["ranges"] == table.record                                              # written, and read back as plain lists
    again = FusedAdamW(flat, ranges=param_ranges(flat, no_decay_rules(m) + freeze_rules("0.")))
    restore_resume(r, flat, again, "test")
    assert again.t == 3 and torch.equal(again.m, opt.m) and torch.equal(again.v, opt.v)
    for bad in (FusedAdamW(flat, ranges=other), FusedAdamW(flat)):
        with pytest.raises(RuntimeError, match="range table"):
            restore_resume(r, flat, bad, "test")
        assert bad.t == 0 and not bad.m.any()                                       # refused before anything is copied
    # a file without a table: into an optimizer without one as before, refused by one with a table
    plain = FusedAdamW(flat)
    plain.t = 2
    r0 = resume_section(flat, plain, step=2)
    assert "ranges" not in r0
    restore_resume(r0, flat, FusedAdamW(flat), "test")
    with pytest.raises(RuntimeError, match="range table"):
        restore_resume(r0, flat, FusedAdamW(flat, ranges=table), "test")
    with pytest.raises(ValueError, match="range table"):
        FusedAdamW(encoder(), ranges=table)                                         # a table over another layout
