"""The host side of trainer.RPNTrainer / TwoStageTrainer, on the builders of tests/_det_trainers_common.py:

  FlatParameters(exclude=)   offsets, views and numel over the remaining parameters on 8-element granules; the excluded parameters stay where they are;
                             exclude=() is the layout of a second object built without the argument; the refusals
  save / load_rpn_checkpoint the exact key set, the reference's head keys, a strict round trip into a differently seeded model, a hand-written file in the
                             reference's form, backbone_only, the resume section of a frozen-backbone layout
  keep_latest_checkpoints    on files with set modification times
  proposal_limits, _loss_record, TwoStageTrainer.resolve_mode and the obj_only / is_reg refusal"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _det_trainers_common as D  # noqa: E402
from tests import _finetune_common as C  # noqa: E402

CPU = torch.device("cpu")


def _layout_over(flat, module, kept):
    """the flat buffers hold exactly `kept` ([(name, parameter)] in named_parameters() order), each on an 8-element granule, tiling the buffer"""
    from nerf_mae_amd.trainer import flat_layout
    lay = flat_layout(flat)
    assert list(lay) == [n for n, _ in kept]
    p0, g0 = flat._flat.data_ptr(), flat._flat_grad.data_ptr()
    off = 0
    for n, p in kept:
        assert lay[n] == [off, p.numel()] and flat._offsets[id(p)] == off, n
        assert p.data_ptr() == p0 + 4 * off and p.grad is not None and p.grad.data_ptr() == g0 + 4 * off, n
        off += C.round8(p.numel())
    assert flat._flat.numel() == flat._flat_grad.numel() == off == sum(C.round8(p.numel()) for _, p in kept)
    flat.check()


def test_excluding_the_backbone_leaves_the_head_alone_in_the_flat_buffer():
    from nerf_mae_amd.finetune import FlatParameters
    m = D.rpn_model()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    where = {n: p.data_ptr() for n, p in m.backbone.named_parameters()}
    flat = FlatParameters(m, CPU, exclude=(m.backbone,))
    assert flat.base is None and m.backbone.base._flat is None, "an excluded encoder is not searched for and not flattened"
    assert {n: p.data_ptr() for n, p in m.backbone.named_parameters()} == where and all(p.grad is None for p in m.backbone.parameters())
    assert not any(id(p) in flat._offsets for p in m.backbone.parameters())
    kept = [(n, p) for n, p in m.named_parameters() if n.startswith("rpn.")]
    assert len(kept) == 6 and all(p.requires_grad for _, p in kept)
    _layout_over(flat, m, kept)
    after = m.state_dict()
    assert list(after) == list(before) and all(torch.equal(after[k], before[k]) for k in before)


def test_excluding_the_first_stage_of_the_detector():
    from nerf_mae_amd.finetune import FlatParameters
    det = D.two_stage()
    assert not any(p.requires_grad for p in det.rpn_network.rpn.parameters()), "without train_rpn the detector freezes the first stage's head"
    where = {n: p.data_ptr() for n, p in det.rpn_network.named_parameters()}
    flat = FlatParameters(det, CPU, exclude=(det.rpn_network,))
    assert {n: p.data_ptr() for n, p in det.rpn_network.named_parameters()} == where
    kept = [(n, p) for n, p in det.named_parameters() if n.startswith("roi_model.")]
    assert [n for n, _ in kept] == ["roi_model.RCNN_model.RCNN_bbox_pred.weight", "roi_model.RCNN_model.RCNN_bbox_pred.bias",
                                    "roi_model.RCNN_model.RCNN_cls_score.weight", "roi_model.RCNN_model.RCNN_cls_score.bias"]
    _layout_over(flat, det, kept)
    # the backbone alone: the first stage's head joins the buffer when it trains
    det2 = D.two_stage(train_rpn=True)
    flat2 = FlatParameters(det2, CPU, exclude=(det2.rpn_network.backbone,))
    _layout_over(flat2, det2, [(n, p) for n, p in det2.named_parameters() if not n.startswith("rpn_network.backbone.")])


def test_no_exclusion_is_the_layout_without_the_argument():
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.trainer import flat_layout
    a, b = D.rpn_model(), D.rpn_model()
    fa, fb = FlatParameters(a, CPU, exclude=()), FlatParameters(b, CPU)
    assert flat_layout(fa) == flat_layout(fb) and fa._flat.numel() == fb._flat.numel() and torch.equal(fa._flat, fb._flat)
    assert fa.base is a.backbone.base and fa.base._flat.data_ptr() == fa._flat.data_ptr() and fa.base._flat.numel() == C.BASE_FLAT_NUMEL
    assert fa.exclude == () and fb.exclude == ()


def test_exclusion_refusals():
    from nerf_mae_amd.finetune import FlatParameters
    m = D.rpn_model()
    with pytest.raises(ValueError, match="not one of"):
        FlatParameters(m, CPU, exclude=(torch.nn.Linear(2, 2),))
    with pytest.raises(ValueError, match="not one of"):
        FlatParameters(m, CPU, exclude=(D.rpn_model().backbone,))            # a module of the same kind, of another model
    with pytest.raises(ValueError, match="leaves no trainable parameter"):
        FlatParameters(m, CPU, exclude=(m.backbone, m.rpn))
    det = D.two_stage()
    with pytest.raises(ValueError, match="leaves no trainable parameter"):
        FlatParameters(det, CPU, exclude=(det.rpn_network.backbone, det.roi_model))
    with pytest.raises(ValueError, match="as a whole"):
        FlatParameters(m, CPU, exclude=(m.backbone.base.stages[0],))
    assert m.backbone.base._flat is None and all(p.grad is None for p in m.parameters()), "a refused call re-homes nothing"


# ---- the RPN checkpoint ------------------------------------------------------------------------------------------------------------------------------
def _equal(a, b):
    a, b = a.state_dict(), b.state_dict()
    return list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in a)


def test_rpn_checkpoint_keys_round_trip_reference_form_and_backbone_only(tmp_path):
    from nerf_mae_amd.rpn import RPNHead
    from nerf_mae_amd.trainer import load_rpn_checkpoint, save_rpn_checkpoint
    m = D.rpn_model()
    path = str(tmp_path / "rpn.pt")
    save_rpn_checkpoint(path, m, 3, {"lr": 1e-4, "dataset_name": "front3d", "device": CPU})
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert list(ck) == ["epoch", "backbone_state_dict", "rpn_head_state_dict", "train_args"] and ck["epoch"] == 3
    assert ck["train_args"] == {"lr": 1e-4, "dataset_name": "front3d", "device": "cpu"}
    head = RPNHead(64, m.rpn.anchor_generator.num_anchors_per_location()[0], 1)
    assert list(ck["rpn_head_state_dict"]) == list(head.state_dict()) == ["conv.0.weight", "conv.0.bias", "cls_logits.weight", "cls_logits.bias", "bbox_pred.weight",
                                                                            "bbox_pred.bias"]
    assert list(ck["backbone_state_dict"]) == list(m.backbone.state_dict())
    fresh = D.rpn_model(seed=5)
    assert not _equal(fresh.rpn.head, m.rpn.head) and not _equal(fresh.backbone, m.backbone)
    load_rpn_checkpoint(path, fresh)
    assert _equal(fresh, m)

    # a file as run_rpn.py writes it: the four keys, tensors as they come from state_dict(), argparse's __dict__, no resume section
    ref = str(tmp_path / "reference.pt")
    torch.save({"epoch": 7, "backbone_state_dict": m.backbone.state_dict(), "rpn_head_state_dict": m.rpn.head.state_dict(),
                "train_args": {"mode": "train", "lr": 3e-4, "freeze_backbone": False, "tags": None}}, ref)
    other = D.rpn_model(seed=6)
    got = load_rpn_checkpoint(ref, other, opt=object())                       # no resume section: the optimizer is not looked at
    assert got["epoch"] == 7 and "resume" not in got and _equal(other, m)

    only = D.rpn_model(seed=7)
    head_before = {k: v.clone() for k, v in only.rpn.head.state_dict().items()}
    load_rpn_checkpoint(path, only, backbone_only=True)
    assert _equal(only.backbone, m.backbone) and all(torch.equal(v, head_before[k]) for k, v in only.rpn.head.state_dict().items())

    del ck["rpn_head_state_dict"]
    torch.save(ck, path)
    with pytest.raises(KeyError, match="rpn_head_state_dict"):
        load_rpn_checkpoint(path, fresh)
    load_rpn_checkpoint(path, fresh, backbone_only=True)


class _Opt:
    """CPU stand-in for FusedAdamW: what the resume section reads and writes"""

    def __init__(self, flat, fill):
        n = flat._flat.numel()
        self.model = flat
        self.m, self.v = torch.arange(n, dtype=torch.float32) * fill, torch.arange(n, dtype=torch.float32) * fill + 0.5
        self.t, self.lr, self.betas = 7, 3e-4, (0.87, 0.999)


def test_rpn_checkpoint_resume_section_of_a_frozen_backbone_layout(tmp_path):
    """the moments lie over the head alone, under the names of module.named_parameters(); the file still carries the backbone"""
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.trainer import flat_layout, load_rpn_checkpoint, save_rpn_checkpoint
    m, fresh = D.rpn_model(), D.rpn_model(seed=5)
    flat, flat2 = FlatParameters(m, CPU, exclude=(m.backbone,)), FlatParameters(fresh, CPU, exclude=(fresh.backbone,))
    opt, opt2 = _Opt(flat, 1.0), _Opt(flat2, 0.0)
    opt2.t = 0
    path = str(tmp_path / "rpn.pt")
    save_rpn_checkpoint(path, m, 2, {}, opt, step=6)
    ck = load_rpn_checkpoint(path, fresh, opt2)
    assert list(ck) == ["epoch", "backbone_state_dict", "rpn_head_state_dict", "train_args", "resume"]
    assert ck["resume"]["layout"] == flat_layout(flat) and all(n.startswith("rpn.head.") for n in ck["resume"]["layout"]) and ck["resume"]["step"] == 6
    assert ck["resume"]["m"].numel() == flat._flat.numel() < 200000
    assert torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v) and opt2.t == 7 and _equal(fresh, m)
    flat2.check()
    whole = _Opt(FlatParameters(D.rpn_model(seed=8), CPU), 0.0)               # the same file into an unfrozen layout: another parameter set
    with pytest.raises(RuntimeError, match="different parameter set"):
        load_rpn_checkpoint(path, whole.model.module, whole)


def test_keep_latest_checkpoints_by_modification_time(tmp_path):
    from nerf_mae_amd.trainer import keep_latest_checkpoints
    times = {"epoch_1.pt": 1000, "epoch_2.pt": 4000, "epoch_3.pt": 2000, "epoch_10.pt": 3000, "epoch_11.pt": 3000}
    for name, t in times.items():
        (tmp_path / name).write_bytes(b"")
        os.utime(tmp_path / name, (t, t))
    for name in ("model_best.pt", "model_best_ap25.pt", "epoch_9.txt"):
        (tmp_path / name).write_bytes(b"")
        os.utime(tmp_path / name, (1, 1))
    others = {"model_best.pt", "model_best_ap25.pt", "epoch_9.txt"}
    keep_latest_checkpoints(str(tmp_path), 5)
    assert set(os.listdir(tmp_path)) == set(times) | others
    keep_latest_checkpoints(str(tmp_path), 3)
    assert set(os.listdir(tmp_path)) == {"epoch_2.pt", "epoch_10.pt", "epoch_11.pt"} | others
    keep_latest_checkpoints(str(tmp_path), 2)                                 # equal times: the higher epoch is the newer
    assert set(os.listdir(tmp_path)) == {"epoch_2.pt", "epoch_11.pt"} | others
    keep_latest_checkpoints(str(tmp_path), 1)
    assert set(os.listdir(tmp_path)) == {"epoch_2.pt"} | others
    with pytest.raises(ValueError, match="keep_latest >= 1"):
        keep_latest_checkpoints(str(tmp_path), 0)
    keep_latest_checkpoints(str(tmp_path / "nothing_here"), 1)


def test_limits_rule_and_record_arithmetic():
    from nerf_mae_amd.trainer import RPNTrainer, _loss_record, proposal_limits
    assert proposal_limits(2500) == [300, 1000, 2500] and proposal_limits(1000) == [300, 1000, 1000] and proposal_limits(999) == [300, 999]
    assert proposal_limits(300) == [300, 300] and proposal_limits(40) == [40]
    rec = _loss_record(RPNTrainer.KEYS, [0.5, 0.25, 2.0], {"loss_rpn_box_reg": 5.0, "loss_rpn_box_reg_2d": 0.125})
    assert list(rec) == ["train_loss", "loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d"]
    assert rec == {"train_loss": 0.5 + 5.0 * 0.25 + 0.125 * 2.0, "loss_objectness": 0.5, "loss_rpn_box_reg": 0.25, "loss_rpn_box_reg_2d": 2.0}
    keys = ("loss_objectness", "loss_rpn_box_reg", "rpn_loss_objectness", "rpn_loss_rpn_box_reg", "rpn_loss_rpn_box_reg_2d")
    rec = _loss_record(keys, [1.0, 2.0, 4.0, 8.0, 16.0], {"loss_rpn_box_reg": 0.0, "rpn_loss_rpn_box_reg": 5.0, "rpn_loss_rpn_box_reg_2d": 0.0})
    assert rec["train_loss"] == 1.0 + 4.0 + 40.0 and [rec[k] for k in keys] == [1.0, 2.0, 4.0, 8.0, 16.0]


def test_two_stage_mode_resolution_and_the_obj_only_refusal():
    from nerf_mae_amd.trainer import TwoStageTrainer
    mode = TwoStageTrainer.resolve_mode
    assert mode(False) == mode(False, None) == mode(False, True) == ("head", "first_stage")
    assert mode(True) == mode(True, None) == mode(True, False) == ("joint", None)
    assert mode(False, False) == ("fine_tune", None)
    assert mode(True, True) == ("heads", "backbone")
    det = D.two_stage()
    assert det.is_reg and det.first_stage_no_grad is False and det.rpn_network.backbone_no_grad is False
    with pytest.raises(ValueError, match="obj_only"):
        TwoStageTrainer(det, D.scenes((11,)), D.boxes((11,)), obj_only=True)
    assert det.first_stage_no_grad is False, "a refused construction leaves the detector as it was"
    with pytest.raises(ValueError, match="one box array per scene"):
        TwoStageTrainer(det, D.scenes((11, 12)), D.boxes((11,)))
