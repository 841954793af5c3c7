"""finetune.FlatParameters and the detection checkpoint on the host (flatten_parameters(device=cpu) is supported, so the layout logic needs no GPU): the common
small models of tests/_finetune_common.py; the four checkpoint formats (key order, train_args, resume section, weights-only files, missing sections) on stand-in
modules.  The step itself, the optimizer arithmetic and DetectionTrainer are tests/test_finetune_gpu.py."""
import copy
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402

CPU = torch.device("cpu")


def _check_layout(module, n_trainable=None, base_numel=None):
    """flattens `module` and checks test 1's properties; returns the FlatParameters"""
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.trainer import flat_layout
    before = {k: v.clone() for k, v in module.state_dict().items()}
    frozen = {n: p.data_ptr() for n, p in module.named_parameters() if not p.requires_grad}
    buffers = {n: b.data_ptr() for n, b in module.named_buffers()}
    names = [n for n, _ in C.trainable(module)]
    flat = FlatParameters(module, CPU)
    after = module.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before), "every state_dict entry bit-identical"
    assert {n: p.data_ptr() for n, p in module.named_parameters() if not p.requires_grad} == frozen, "frozen parameters stay where they are"
    assert {n: b.data_ptr() for n, b in module.named_buffers()} == buffers, "buffers stay where they are"
    lay = flat_layout(flat)
    assert sorted(lay) == sorted(names), "flat_layout names exactly the trainable names"
    if n_trainable is not None:
        assert len(names) == n_trainable
    p0, g0 = flat._flat.data_ptr(), flat._flat_grad.data_ptr()
    for n, p in C.trainable(module):
        off, numel = lay[n]
        assert off % 8 == 0 and numel == p.numel(), n
        assert p.data_ptr() == p0 + 4 * off and p.grad is not None and p.grad.data_ptr() == g0 + 4 * off, n
        assert p.is_contiguous() and p.grad.shape == p.shape
    spans = sorted((off, off + C.round8(k)) for off, k in lay.values())
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == flat._flat.numel(), "granules tile the buffer"
    base = flat.base
    assert base is not None and base._flat.data_ptr() == p0 and base._flat_grad.data_ptr() == g0
    inside = {id(p) for p in base._trainable()}
    assert base._flat.numel() == base.flat_numel() == sum(C.round8(p.numel()) for p in base._trainable())
    if base_numel is not None:
        assert base._flat.numel() == base_numel
    rest = [p for _, p in C.trainable(module) if id(p) not in inside]
    assert flat._flat.numel() == base._flat.numel() + sum(C.round8(p.numel()) for p in rest)
    assert all(flat._offsets[id(p)] == base._offsets[id(p)] for p in base._trainable()), "base._offsets holds"
    assert max(base._offsets.values()) < base._flat.numel() <= min(flat._offsets[id(p)] for p in rest)
    # the base's own staleness test (model._ensure_ready) finds nothing to re-flatten
    assert all(p.data_ptr() == base._flat.data_ptr() + 4 * base._offsets[id(p)] for p in base._trainable())
    assert not flat._flat_grad.any()
    flat.check()
    return flat, rest


def test_fcos_layout_counts_offsets_and_views():
    m = C.fcos_model()
    assert [n for n, p in m.named_parameters() if not p.requires_grad] == ["backbone.base.pos_embed"]
    flat, rest = _check_layout(m, n_trainable=212, base_numel=C.BASE_FLAT_NUMEL)
    assert sum(p.numel() for _, p in C.trainable(m)) == 30110933
    assert len(flat.base._trainable()) == 169 and sum(p.numel() for p in flat.base._trainable()) == 29115462
    assert len(rest) == 43 and sum(p.numel() for p in rest) == 995471
    assert flat._flat.numel() == C.BASE_FLAT_NUMEL + sum(C.round8(p.numel()) for p in rest)
    # named_parameters() order behind the base
    offs = [flat._offsets[id(p)] for n, p in m.named_parameters() if p.requires_grad and not n.startswith("backbone.base.")]
    assert offs == sorted(offs)


@pytest.mark.parametrize("which", ("rpn", "semantics"))
def test_other_models_layout(which):
    m = C.rpn_model() if which == "rpn" else C.semantics_model()
    n = len(C.trainable(m))
    flat, rest = _check_layout(m, n_trainable=n)
    assert len(rest) == n - len(flat.base._trainable()) > 0
    assert sum(p.numel() for _, p in C.trainable(m)) == sum(p.numel() for p in flat.base._trainable()) + sum(p.numel() for p in rest)


def test_shared_parameter_is_placed_once():
    from nerf_mae_amd.finetune import FlatParameters
    a = torch.nn.Linear(8, 3)
    b = torch.nn.Linear(8, 3)
    b.weight = a.weight
    m = torch.nn.ModuleDict({"a": a, "b": b})
    flat = FlatParameters(m)
    assert flat.base is None and flat._flat.numel() == 24 + 8 + 8
    assert b.weight.data_ptr() == a.weight.data_ptr() == flat._flat.data_ptr()
    flat.check()


def test_check_and_refusals():
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters
    from nerf_mae_amd.model import SWIN_CONFIGS, SwinTransformer_MAE3D_New
    m = C.fcos_model()
    flat = FlatParameters(m)
    flat.check()
    fresh = C.fcos_model(seed=1)
    m.load_state_dict(fresh.state_dict(), strict=True)
    flat.check()                                                    # load_state_dict copies in place
    assert torch.equal(m.backbone.fpn_neck.fpn_convs[0].weight, fresh.backbone.fpn_neck.fpn_convs[0].weight)
    with pytest.raises(RuntimeError, match="HIP device"):
        FinetuneStep(flat, types.SimpleNamespace(model=flat), lambda: None)
    with pytest.raises(RuntimeError, match="move the module first"):
        FlatParameters(m, torch.device("cuda", 0))                   # parameters on the host where a device is asked for

    torch.nn.Module.zero_grad(m)                                    # torch's default set_to_none=True
    with pytest.raises(RuntimeError, match=r"\.grad of parameter '"):
        flat.check()
    flat.flatten_parameters()
    flat.check()

    p = m.fcos_module.head.cls_logits.weight
    p.data = p.data.clone()
    with pytest.raises(RuntimeError, match="fcos_module.head.cls_logits.weight"):
        flat.check()
    flat.flatten_parameters()
    flat.check()

    m.backbone.base.flatten_parameters(CPU)                         # the base re-flattens itself
    with pytest.raises(RuntimeError, match="backbone.base"):
        flat.check()

    two = torch.nn.ModuleList([C.backbone(), C.backbone()])
    with pytest.raises(ValueError, match="2 SwinTransformer_MAE3D_New"):
        FlatParameters(two)
    frozen = C.backbone()
    for q in frozen.base.parameters():
        q.requires_grad_(False)
    with pytest.raises(ValueError, match="no trainable parameter"):
        FlatParameters(frozen)

    # a bare MAE model without `out` flattens as before: the offsets of a second instance flattened the old way (allocate, walk _trainable())
    cfg = SWIN_CONFIGS["swin_t"]
    kw = dict(patch_size=[4] * 3, embed_dim=cfg["embed_dim"], depths=cfg["depths"], num_heads=cfg["num_heads"], window_size=[4] * 3, resolution=32,
              compute_dtype=torch.float32)
    a, b = SwinTransformer_MAE3D_New(**kw), SwinTransformer_MAE3D_New(**kw)
    fa, ga = a.flatten_parameters(CPU)
    off, old, names_b = 0, {}, {id(q): n for n, q in b.named_parameters()}
    for q in b._trainable():
        old[names_b[id(q)]] = off
        off += (q.numel() + 7) // 8 * 8
    names = {id(q): n for n, q in a.named_parameters()}
    assert {names[i]: o for i, o in a._offsets.items()} == old and fa.numel() == ga.numel() == off == a.flat_numel()
    assert a.mask_token.data_ptr() == fa.data_ptr()


class _Opt:
    """CPU stand-in for FusedAdamW: what the resume section reads and writes"""

    def __init__(self, flat, fill):
        n = flat._flat.numel()
        self.model = flat
        self.m = torch.arange(n, dtype=torch.float32) * fill
        self.v = torch.arange(n, dtype=torch.float32) * fill + 0.5
        self.t, self.lr, self.betas = 7, 3e-4, (0.87, 0.999)


def test_detection_checkpoint_format_and_resume_roundtrip(tmp_path):
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.trainer import flat_layout, load_detection_checkpoint, save_detection_checkpoint
    m = C.fcos_model()
    path = str(tmp_path / "a.pt")
    save_detection_checkpoint(path, m, 3, {"lr": 1e-3, "dataset": "front3d"})
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(ck) == ["backbone_state_dict", "epoch", "fcos_state_dict", "train_args"] and ck["epoch"] == 3 and ck["train_args"]["dataset"] == "front3d"
    assert list(ck["backbone_state_dict"]) == list(m.backbone.state_dict()) and list(ck["fcos_state_dict"]) == list(m.fcos_module.state_dict())
    fresh = C.fcos_model(seed=5)
    assert not torch.equal(fresh.fcos_module.head.cls_logits.weight, m.fcos_module.head.cls_logits.weight)
    load_detection_checkpoint(path, fresh)                          # strict in both halves
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), m.state_dict().values()))

    flat = FlatParameters(m)
    opt = _Opt(flat, 1.0)
    save_detection_checkpoint(path, m, 4, {}, opt, step=11)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(ck) == ["backbone_state_dict", "epoch", "fcos_state_dict", "resume", "train_args"]
    assert sorted(ck["resume"]) == ["betas", "layout", "lr", "m", "step", "t", "v"]
    assert ck["resume"]["layout"] == flat_layout(flat) and ck["resume"]["step"] == 11
    flat2 = FlatParameters(fresh)
    opt2 = _Opt(flat2, 0.0)
    opt2.t, opt2.lr, opt2.betas = 0, 0.0, (0.0, 0.0)
    load_detection_checkpoint(path, fresh, opt2)
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and (opt2.t, opt2.lr, opt2.betas) == (7, 3e-4, (0.87, 0.999))

    # a file written under a permuted layout is remapped by name
    lay = ck["resume"]["layout"]
    names = list(lay)[::-1]
    perm, off = {}, 0
    for n in names:
        perm[n] = [off, lay[n][1]]
        off += lay[n][1] + 3                                        # another granule as well
    pm, pv = torch.zeros(off), torch.zeros(off)
    for n in names:
        (o1, k), o2 = lay[n], perm[n][0]
        pm[o2:o2 + k] = ck["resume"]["m"][o1:o1 + k]
        pv[o2:o2 + k] = ck["resume"]["v"][o1:o1 + k]
    ck2 = copy.copy(ck)
    ck2["resume"] = dict(ck["resume"], m=pm, v=pv, layout=perm)
    path2 = str(tmp_path / "b.pt")
    torch.save(ck2, path2)
    opt3 = _Opt(flat2, 0.0)
    load_detection_checkpoint(path2, fresh, opt3)
    for n, (o, k) in lay.items():
        assert torch.equal(opt3.m[o:o + k], opt.m[o:o + k]) and torch.equal(opt3.v[o:o + k], opt.v[o:o + k]), n
    ck2["resume"]["layout"] = {("x" + n): v for n, v in perm.items()}
    torch.save(ck2, path2)
    with pytest.raises(RuntimeError, match="different parameter set"):
        load_detection_checkpoint(path2, fresh, opt3)


def test_delete_suboptimal_checkpoints_keeps_the_best_six_by_ap50(tmp_path):
    from nerf_mae_amd.trainer import delete_suboptimal_checkpoints
    ap50 = [0.1, 0.5, 0.3, 0.7, 0.2, 0.6, 0.4, 0.05]
    for i, a in enumerate(ap50):
        kind = "ap50_ap25" if i % 2 else "ap25_ap50"
        (tmp_path / f"model_best_{kind}_{a}_{0.9 - a}.pt").write_bytes(b"")
    delete_suboptimal_checkpoints(str(tmp_path), "ap50", 6, 1)
    left = sorted(float(f.split("_")[-2]) for f in os.listdir(tmp_path))
    assert left == sorted(ap50)[-6:]


# ---- the four checkpoint formats: key order, train_args, resume section, weights-only files, missing sections ---------------------------------------------
class _Flat(torch.nn.Module):
    """stand-in for a flattened model (and for finetune.FlatParameters): what flat_layout reads"""

    def __init__(self, module):
        super().__init__()
        self.module = module
        self._offsets, off = {}, 0
        for p in module.parameters():
            self._offsets[id(p)] = off
            off += C.round8(p.numel())
        self._flat = torch.zeros(off)

    def named_parameters(self, *a, **k):
        return self.module.named_parameters(*a, **k)


def _lin(seed):
    torch.manual_seed(seed)
    return torch.nn.Linear(3, 2)


def _stand_in(which, seed):
    """a module with the attribute names the writer of `which` reads, and the {section: module} it stores"""
    if which in ("mae", "voxel"):
        m = _lin(seed)
        return m, {"state_dict": m}
    m = torch.nn.Module()
    if which == "detection":
        m.backbone, m.fcos_module = _lin(seed), _lin(seed + 1)
        return m, {"backbone_state_dict": m.backbone, "fcos_state_dict": m.fcos_module}
    m.rpn_network, m.roi_model = torch.nn.Module(), torch.nn.Module()
    m.rpn_network.backbone, m.rpn_network.rpn, m.roi_model.RCNN_model = _lin(seed), _lin(seed + 1), _lin(seed + 2)
    return m, {"backbone_state_dict": m.rpn_network.backbone, "RCNN_dict": m.roi_model.RCNN_model, "rpn_state_dict": m.rpn_network.rpn}


CHECKPOINT_KEYS = {"mae": ["epoch", "state_dict", "train_args"],
                   "detection": ["epoch", "backbone_state_dict", "fcos_state_dict", "train_args"],
                   "two_stage": ["epoch", "backbone_state_dict", "RCNN_dict", "rpn_state_dict", "train_args"],
                   "voxel": ["epoch", "state_dict", "train_args"]}
REQUIRED = {"mae": "state_dict", "detection": "fcos_state_dict", "two_stage": "RCNN_dict", "voxel": "state_dict"}


@pytest.mark.parametrize("which", list(CHECKPOINT_KEYS))
def test_checkpoint_writers_key_order_resume_and_required_sections(tmp_path, which):
    from nerf_mae_amd import trainer as T
    save, load = {"mae": (T.save_checkpoint, T.load_checkpoint), "detection": (T.save_detection_checkpoint, T.load_detection_checkpoint),
                  "two_stage": (T.save_two_stage_checkpoint, T.load_two_stage_checkpoint), "voxel": (T.save_voxel_checkpoint, T.load_voxel_checkpoint)}[which]
    m, parts = _stand_in(which, 0)
    # save_checkpoint stores train_args as passed, the fine-tuning formats through _plain
    args = {"lr": 1e-3, "sizes": [1, 2]} if which == "mae" else {"lr": 1e-3, "sizes": (1, 2), "device": CPU, 5: None}
    plain = {"lr": 1e-3, "sizes": [1, 2]} if which == "mae" else {"lr": 1e-3, "sizes": [1, 2], "device": "cpu", "5": None}
    path = str(tmp_path / "a.pt")

    def equal(a, b):
        a, b = a.state_dict(), b.state_dict()
        return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)

    # without an optimizer: the format's keys in their order, no resume section; the file loads the weights only, also with an optimizer at hand
    save(path, m if which == "mae" else types.SimpleNamespace(module=m), 3, args)          # (the fine-tuning formats store a wrapper's .module)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ck) == CHECKPOINT_KEYS[which] and ck["epoch"] == 3
    assert ck["train_args"] == plain and (which == "mae" or T._plain(args) == plain)
    for section, mod in parts.items():
        assert list(ck[section]) == list(mod.state_dict()) and all(torch.equal(ck[section][k], v) for k, v in mod.state_dict().items())
    fresh, fresh_parts = _stand_in(which, 10)
    flat2 = fresh if which == "mae" else _Flat(fresh)
    if which == "mae":
        fresh._offsets, fresh._flat = _Flat(fresh)._offsets, None
    opt2 = _Opt(_Flat(fresh), 0.0)
    opt2.model = flat2
    m0, v0 = opt2.m.clone(), opt2.v.clone()
    assert "resume" not in load(path, fresh, opt2)
    assert all(equal(parts[s], fresh_parts[s]) for s in parts) and torch.equal(opt2.m, m0) and torch.equal(opt2.v, v0) and opt2.t == 7

    # with an optimizer: "resume" is the last key, its layout is flat_layout's
    flat = m if which == "mae" else _Flat(m)
    if which == "mae":
        m._offsets = _Flat(m)._offsets
    opt = _Opt(_Flat(m), 1.0)
    opt.model = flat
    save(path, m, 4, args, opt, step=11)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ck) == CHECKPOINT_KEYS[which] + ["resume"] and list(ck["resume"]) == ["m", "v", "t", "lr", "betas", "step", "layout"]
    assert ck["resume"]["layout"] == T.flat_layout(flat) and ck["resume"]["step"] == 11 and torch.equal(ck["resume"]["m"], opt.m)
    if which == "mae":          # the moments lie over the model itself, which must be on the device by then
        with pytest.raises(RuntimeError, match="move the model to the HIP device"):
            load(path, fresh, opt2)
    else:
        opt2.t = 0
        load(path, fresh, opt2)
        assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and (opt2.t, opt2.lr, opt2.betas) == (7, 3e-4, (0.87, 0.999))

    # a missing required section raises; the two-stage format's optional ones may be None or absent
    del ck[REQUIRED[which]]
    torch.save(ck, path)
    with pytest.raises(KeyError, match=REQUIRED[which]):
        load(path, fresh)
    if which == "two_stage":
        save(path, m, 5, args, fine_tune=False)
        ck = torch.load(path, map_location="cpu", weights_only=True)
        assert list(ck) == CHECKPOINT_KEYS[which] and ck["backbone_state_dict"] is None
        other, other_parts = _stand_in(which, 20)
        before = {k: v.clone() for k, v in other.rpn_network.backbone.state_dict().items()}
        load(path, other)
        assert equal(other_parts["RCNN_dict"], parts["RCNN_dict"]) and equal(other_parts["rpn_state_dict"], parts["rpn_state_dict"])
        assert all(torch.equal(v, before[k]) for k, v in other.rpn_network.backbone.state_dict().items())
        del ck["rpn_state_dict"], ck["backbone_state_dict"]
        torch.save(ck, path)
        load(path, _stand_in(which, 21)[0])
