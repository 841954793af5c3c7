"""trainer.RPNTrainer and trainer.TwoStageTrainer on the GPU, on the builders of tests/_det_trainers_common.py: swin_t, 32^3, 64 FPN channels,
fp32 compute, axis-aligned boxes; at most three training and two validation scenes, two epochs, batch 2 (three scenes: one ragged batch per epoch).

  RPNTrainer
    fit                  history, schedule, files, a strict load, and the last record against the same weights evaluated by hand (twice: first the two by-hand
                         results against each other, then the trainer's against them, ==)
    one epoch            against the same batches stepped by hand (dp_epoch_plan, DetectionBatcher.prepare with the draws of random.Random(seed), OneCycle.at,
                         FinetuneStep): relerr(A, B) <= steps * STEP_BOUND + 4 * relerr(B, B'), B' a second by-hand run, AdamW's eps = 1, stochastic depth off
                         (relerr, STEP_BOUND and the form of the bound as tests/test_finetune_gpu.py has them)
    freeze_backbone      three steps: the backbone bit for bit where it started and without a gradient, every parameter of model.rpn moved, the flat buffer is
                         the head's; the first step's losses against model.rpn on features computed by hand under no_grad with the backbone in eval()
    resume               the twin of tests/test_finetune_gpu.py::test_detection_trainer_resume_continues_where_it_stopped, with its bound
  TwoStageTrainer
    head mode            with the stock RCNN and with FusedRCNN (bf16): fit, files, "backbone_state_dict" None, first stage bit for bit where it started, box head
                         moved, the record against a by-hand detections_dense evaluation
    joint mode           five finite losses, their weighted sum, RPN head and backbone moved
    fine_tune, heads     what moves and what does not
    init_from_rpn        from a file an RPNTrainer wrote in the same test

NMH_PRINT_ERR=1 prints every measured value."""
import functools
import os
import random
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _det_trainers_common as D  # noqa: E402
from tests import _finetune_common as C  # noqa: E402
from tests._metrics import relerr  # noqa: E402

pytestmark = pytest.mark.gpu
LR, WD, CLIP, EPS = 1e-3, 1e-3, 0.1, 1.0
STEP_BOUND = 1e-5                        # the project's per-step optimizer bound (tests/test_finetune_gpu.py)
CUDA = torch.device("cuda")
RPN_KEYS = ("loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d")
JOINT_KEYS = ("loss_objectness", "loss_rpn_box_reg", "rpn_loss_objectness", "rpn_loss_rpn_box_reg", "rpn_loss_rpn_box_reg_2d")


def _print(*a):
    if os.environ.get("NMH_PRINT_ERR"):
        print(*a)


def _finite(h, keys):
    for k in keys:
        assert k in h and h[k] == h[k] and abs(h[k]) != float("inf"), (k, h)


def _state_equal(a, b):
    return list(a) == list(b) and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a)


def _moved(module, snap):
    """names of the module's parameters that still hold their snapshot's bits"""
    return [n for n, p in module.named_parameters() if torch.equal(p.detach(), snap["p." + n])]


def _val_batches(batch=2):
    """the validation scenes as RPNTrainer / TwoStageTrainer see them: in order, `batch` at a time, no augmentation -> (xb, ext, per-scene gt)"""
    from nerf_mae_amd import data
    batcher = data.DetectionBatcher(C.R, CUDA, normalize_density=True)
    for b in range(0, len(D.VAL), batch):
        seeds = D.VAL[b:b + batch]
        xb, ext, gt = batcher.prepare(D.scenes(seeds), D.boxes(seeds), params=[(0, 0.0, 1.0)] * len(seeds))
        assert ext == [[C.R] * 3] * len(seeds)
        yield xb, ext, gt


def _dense_gt(gt):
    g = max(t.shape[0] for t in gt)
    return (torch.stack([torch.nn.functional.pad(t, (0, 0, 0, g - t.shape[0])) for t in gt]),
            torch.tensor([t.shape[0] for t in gt], dtype=torch.int32, device=gt[0].device))


# ---- RPNTrainer -----------------------------------------------------------------------------------------------------------------------------------------
def _rpn_eval_by_hand(model, limits):
    """eval(), backbone, rpn.proposals_dense, DetectionEvaluator in its dense form -> (the record's evaluation part, the proposal count of every scene)"""
    from nerf_mae_amd.det_eval import DetectionEvaluator
    model.eval()
    ev = DetectionEvaluator(limits=limits, ap_thresholds=(0.25, 0.5))
    kept = []
    with torch.no_grad():
        for xb, ext, gt in _val_batches():
            ori = torch.tensor(ext, dtype=torch.int32, device=CUDA)
            boxes, scores, _, _, counts = model.rpn.proposals_dense(xb, list(model.backbone(xb)), ori if len(ext) > 1 else None)
            ev.update(boxes, scores, counts, *_dense_gt(gt))
            kept += counts.tolist()
    out = ev.compute()
    rec = {f"recall_{key}_top_{l}": float(out[f"recall_{key}_top_{l}"]["ar"]) for l in limits for key in ("25", "50", "ar")}
    rec["ap_25"], rec["ap_50"] = float(out["ap_25"]["ap"]), float(out["ap_50"]["ap"])
    return rec, kept


def test_rpn_trainer_fit_files_and_the_record_against_a_by_hand_evaluation(tmp_path):
    from nerf_mae_amd.trainer import RPNTrainer, load_rpn_checkpoint
    m = D.rpn_model().cuda().train()
    lines = []
    tr = RPNTrainer(m, D.scenes(D.TRAIN), D.boxes(D.TRAIN), D.scenes(D.VAL), D.boxes(D.VAL), batch_size=2, num_epochs=2, lr=1e-4, weight_decay=1e-3,
                    save_path=str(tmp_path), flip_prob=0.5, rotate_prob=0.5, log=lines.append)
    assert tr.steps_per_epoch == 2 and tr.sched.total == 2 * 2 and tr.limits == [300, 1000, 1000] and tr.batcher.R == C.R
    assert tr.flat.base is m.backbone.base and m.backbone_no_grad is False and tr.exclude == ()
    hist = tr.fit()
    torch.cuda.synchronize()
    assert tr.global_step == 4 and len(hist) == len(lines) == 2 and [h["epoch"] for h in hist] == [1, 2]
    eval_keys = [f"recall_{key}_top_{l}" for l in (300, 1000) for key in ("25", "50", "ar")] + ["ap_25", "ap_50"]
    for h in hist:
        _finite(h, ("train_loss",) + RPN_KEYS + tuple(eval_keys))
        total = h["loss_objectness"] + 5.0 * h["loss_rpn_box_reg"] + 0.0 * h["loss_rpn_box_reg_2d"]
        assert abs(h["train_loss"] - total) <= 1e-5 * abs(total) and h["loss_rpn_box_reg"] > 0 and h["loss_rpn_box_reg_2d"] == 0.0
    assert sorted(os.listdir(tmp_path)) == ["epoch_2.pt", "model_best.pt"]          # keep_checkpoints = 1: epoch_1.pt went when epoch_2.pt came
    fresh = D.rpn_model(seed=3)
    ck = load_rpn_checkpoint(str(tmp_path / "epoch_2.pt"), fresh)
    assert list(ck) == ["epoch", "backbone_state_dict", "rpn_head_state_dict", "train_args", "resume"] and ck["epoch"] == 2 and ck["resume"]["step"] == 4
    assert ck["train_args"]["batch_size"] == 2 and ck["train_args"]["freeze_backbone"] is False and ck["train_args"]["reg_loss_weight"] == 5.0
    assert _state_equal(fresh.state_dict(), m.state_dict())
    tr.flat.check()
    # the last record against the same weights evaluated by hand
    first, kept = _rpn_eval_by_hand(m, tr.limits)
    second, _ = _rpn_eval_by_hand(m, tr.limits)
    assert first == second, "the by-hand evaluation repeats itself"
    assert max(kept) > 0 and len(kept) == len(D.VAL), kept
    _print(f"  [rpn fit] proposals per validation scene {kept}  record {first}")
    assert {k: hist[-1][k] for k in first} == first


def _by_hand_rpn_epoch(seed):
    """one epoch as RPNTrainer runs it, from the parts -> (the flat parameter buffer, the epoch's mean losses [3])"""
    from nerf_mae_amd import data
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, rpn_loss_fn
    from nerf_mae_amd.trainer import FusedAdamW, OneCycle, dp_epoch_plan
    m = D.rpn_model(stochastic_depth=False).cuda().train()
    flat = FlatParameters(m, CUDA)
    opt = FusedAdamW(flat, lr=LR, weight_decay=WD, max_grad_norm=CLIP, eps=EPS)
    step = FinetuneStep(flat, opt, rpn_loss_fn(m), weights={"loss_rpn_box_reg": 5.0, "loss_rpn_box_reg_2d": 0.0})
    batcher = data.DetectionBatcher(C.R, CUDA, True, 0.5, 0.5, 0.0)
    scenes, boxes = D.scenes(D.TRAIN), D.boxes(D.TRAIN)
    plan = dp_epoch_plan(len(scenes), 2, 0, 1, 1, seed)
    sched, rng, acc = OneCycle(LR, 1 * len(plan)), random.Random(seed), 0
    for k, ids in enumerate(plan):
        params = [data.draw_detection_augmentation(0.5, 0.5, 0.0, False, rng) for _ in ids]
        xb, ext, targets = batcher.prepare([scenes[i] for i in ids], [boxes[i] for i in ids], params=params)
        lr, b1 = sched.at(k)
        opt.set_hyper(lr=lr, beta1=b1)
        out = step([xb[i, :, :e[0], :e[1], :e[2]] for i, e in enumerate(ext)], targets)
        acc = acc + torch.stack([out[key] for key in RPN_KEYS])
    torch.cuda.synchronize()
    return flat._flat.detach().cpu().clone(), (acc / len(plan)).cpu(), len(plan)


def test_rpn_trainer_epoch_equals_the_same_batches_stepped_by_hand():
    """relerr(A, B) <= steps * STEP_BOUND + 4 * relerr(B, B') over the flat parameter buffer and over the epoch's three mean losses; not vacuous: the
    parameters moved by at least 100 x the bound and the box loss is positive"""
    from nerf_mae_amd.trainer import RPNTrainer
    seed = 4
    m = D.rpn_model(stochastic_depth=False).cuda().train()
    tr = RPNTrainer(m, D.scenes(D.TRAIN), D.boxes(D.TRAIN), batch_size=2, num_epochs=1, lr=LR, weight_decay=WD, clip_grad_norm=CLIP, flip_prob=0.5, rotate_prob=0.5,
                    log=lambda s: None, seed=seed)
    tr.opt.eps = EPS
    rec = tr.train_epoch(1)
    torch.cuda.synchronize()
    a, la = tr.flat._flat.detach().cpu().clone(), torch.tensor([rec[k] for k in RPN_KEYS])
    (b, lb, steps), (b2, lb2, _) = _by_hand_rpn_epoch(seed), _by_hand_rpn_epoch(seed)
    assert steps == tr.global_step == 2 and a.numel() == b.numel()
    err_p, spread_p, err_l, spread_l = relerr(a, b), relerr(b2, b), relerr(la, lb), relerr(lb2, lb)
    bound_p, bound_l = steps * STEP_BOUND + 4 * spread_p, steps * STEP_BOUND + 4 * spread_l
    lay = {n: (tr.flat._offsets[id(p)], p.numel()) for n, p in m.named_parameters() if id(p) in tr.flat._offsets}
    per_tensor = max(relerr(a[o:o + k], b[o:o + k]) for o, k in lay.values())
    _print(f"  [rpn epoch] parameters relerr(A,B) {err_p:.2e}  relerr(B,B') {spread_p:.2e}  bound {bound_p:.2e}  (largest per tensor {per_tensor:.2e})")
    _print(f"  [rpn epoch] losses     relerr(A,B) {err_l:.2e}  relerr(B,B') {spread_l:.2e}  bound {bound_l:.2e}  A {la.tolist()}")
    assert err_p <= bound_p, (err_p, bound_p)
    assert err_l <= bound_l, (err_l, bound_l)
    assert lb[1].item() > 0, "the batches have positive anchors"
    fresh = D.rpn_model(stochastic_depth=False)
    before = torch.zeros_like(a)
    for n, p in fresh.named_parameters():
        if n in lay:
            before[lay[n][0]:lay[n][0] + lay[n][1]] = p.detach().reshape(-1)
    moved = max(relerr(before[o:o + k], a[o:o + k]) for o, k in lay.values())          # the largest per-tensor move, as tests/test_finetune_gpu.py measures it
    _print(f"  [rpn epoch] moved {moved:.2e}")
    assert moved >= 100 * bound_p, "the epoch moved the parameters by far more than the bound"


def test_rpn_trainer_with_a_frozen_backbone():
    from nerf_mae_amd import data
    from nerf_mae_amd.trainer import RPNTrainer
    m = D.rpn_model().cuda().train()                         # stochastic depth left on: the frozen backbone must not draw it
    backbone0, rpn0 = D.snapshot(m.backbone), D.snapshot(m.rpn)
    scenes, boxes = D.scenes(D.TRAIN), D.boxes(D.TRAIN)
    tr = RPNTrainer(m, scenes, boxes, batch_size=1, num_epochs=1, lr=LR, weight_decay=WD, freeze_backbone=True, log=lambda s: None)
    assert m.backbone_no_grad is True and tr.exclude == (m.backbone,) and tr.flat.base is None and tr.steps_per_epoch == 3
    head = [p for p in m.rpn.parameters()]
    assert tr.flat._flat.numel() == sum(C.round8(p.numel()) for p in head) and len(tr.flat._offsets) == len(head) == 6
    seen, outs, step = C.record_batches(tr, scenes), [], tr.step_fn

    def recording(*batch):
        outs.append(step(*batch))
        return outs[-1]
    tr.step_fn = recording
    tr.train_epoch(1)
    torch.cuda.synchronize()
    assert tr.global_step == 3 and len(outs) == 3 and m.backbone.training is False and m.rpn.training is True and m.training is True
    assert D.same(m.backbone, backbone0), "every backbone parameter and buffer is where it started, bit for bit"
    assert all(p.grad is None or not p.grad.any() for p in m.backbone.parameters()), "no backbone parameter has received a gradient"
    assert _moved(m.rpn, rpn0) == [], "every parameter of model.rpn moved"
    tr.flat.check()
    # the first step's losses: model.rpn on features computed by hand, no_grad, backbone in eval()
    ref = D.rpn_model().cuda()
    ref.backbone.eval()
    ref.rpn.train()
    batcher = data.DetectionBatcher(C.R, CUDA, normalize_density=True)
    i = seen[0][0]
    xb, ext, targets = batcher.prepare([scenes[i]], [boxes[i]], params=[(0, 0.0, 1.0)])
    with torch.no_grad():
        feats = [f.detach() for f in ref.backbone(xb)]
        want = ref.rpn(xb, feats, [tuple(ext[0])], targets)[2]
    for k in RPN_KEYS:
        got, w = outs[0][k].item(), want[k].item()
        _print(f"  [frozen backbone] first step {k}: trainer {got:.8g}  by hand {w:.8g}")
        assert abs(got - w) <= 1e-6 * abs(w), (k, got, w)
    assert want["loss_rpn_box_reg"].item() > 0


def _resume_trainer(seed=0):
    from nerf_mae_amd.trainer import RPNTrainer
    m = D.rpn_model(seed, stochastic_depth=False).cuda().train()
    tr = RPNTrainer(m, D.scenes((11, 12)), D.boxes((11, 12)), batch_size=1, num_epochs=2, lr=LR, weight_decay=WD, log=lambda s: None)
    tr.opt.eps = EPS          # 1, as in the step tests: the order noise of fp32 atomics is not blown up to +-lr
    return tr


@functools.lru_cache(maxsize=None)
def _uninterrupted():
    """U, U': two epochs without a stop, twice.  Computed once, left unchanged."""
    runs = []
    for _ in range(2):
        tr = _resume_trainer()
        tr.fit()
        torch.cuda.synchronize()
        runs.append(tr.flat._flat.detach().cpu().clone())
    return runs


def test_rpn_trainer_resume_continues_where_it_stopped(tmp_path):
    """one epoch + checkpoint + fresh trainer + resume() + one epoch against two uninterrupted epochs: relerr <= 3 * 1e-5 + 4 relerr(U, U').  The anchor
    sampler's counter continues as well: without it the second epoch would draw the first epoch's samples"""
    from nerf_mae_amd.trainer import save_rpn_checkpoint
    u, u2 = _uninterrupted()
    a = _resume_trainer()
    a.train_epoch(1)
    path = str(tmp_path / "epoch_1.pt")
    save_rpn_checkpoint(path, a.model, 1, a.args, a.opt, a.global_step)
    b = _resume_trainer(seed=9)          # other weights: everything must come from the file
    ck = b.resume(path)
    assert ck["resume"]["step"] == 2 and b.global_step == 2 and b.start_epoch == 2 and b.opt.t == 2
    assert torch.equal(b.opt.m, a.opt.m) and torch.equal(b.opt.v, a.opt.v) and torch.equal(b.flat._flat, a.flat._flat)
    assert torch.equal(b.model.rpn.loss.rng_state, a.model.rpn.loss.rng_state) and a.model.rpn.loss.rng_state.tolist() == [0, 2]
    hist = b.fit()
    torch.cuda.synchronize()
    assert [h["epoch"] for h in hist] == [2] and b.global_step == 4
    err, spread = relerr(b.flat._flat.cpu(), u), relerr(u2, u)
    _print(f"  [rpn resume] relerr(resumed, uninterrupted) {err:.2e}  relerr(U, U') {spread:.2e}  bound {3 * STEP_BOUND + 4 * spread:.2e}")
    assert err <= 3 * STEP_BOUND + 4 * spread, (err, spread)


# ---- TwoStageTrainer ------------------------------------------------------------------------------------------------------------------------------------
def _detector_eval_by_hand(det):
    from nerf_mae_amd.det_eval import DetectionEvaluator
    det.eval()
    ev = DetectionEvaluator(limits=(None,), ap_thresholds=(0.25, 0.5))
    kept = []
    with torch.no_grad():
        for xb, ext, gt in _val_batches():
            boxes, scores, counts = det.detections_dense([xb[i] for i in range(xb.shape[0])])
            ev.update(boxes, scores, counts, *_dense_gt(gt))
            kept += counts.tolist()
    out = ev.compute()
    return {"ap_25": float(out["ap_25"]["ap"]), "ap_50": float(out["ap_50"]["ap"])}, kept


@pytest.mark.parametrize("fused", [False, True], ids=["RCNN", "FusedRCNN"])
def test_two_stage_trainer_head_mode(fused, tmp_path):
    from nerf_mae_amd.trainer import TwoStageTrainer, load_two_stage_checkpoint
    det = D.two_stage(fused=fused).cuda().train()
    first0, head0 = D.snapshot(det.rpn_network), D.snapshot(det.roi_model.RCNN_model)
    lines = []
    tr = TwoStageTrainer(det, D.scenes(D.TRAIN), D.boxes(D.TRAIN), D.scenes(D.VAL), D.boxes(D.VAL), batch_size=2, num_epochs=2, lr=LR, weight_decay=WD,
                         save_path=str(tmp_path), flip_prob=0.5, rotate_prob=0.5, log=lines.append)
    assert tr.mode == "head" and tr.frozen == "first_stage" and det.first_stage_no_grad is True and tr.exclude == (det.rpn_network,) and tr.flat.base is None
    assert tr.flat._flat.numel() == sum(C.round8(p.numel()) for p in det.roi_model.RCNN_model.parameters()) and len(tr.flat._offsets) == 4
    assert tr.steps_per_epoch == 2 and tr.sched.total == 2 * 2
    hist = tr.fit()
    torch.cuda.synchronize()
    assert tr.global_step == 4 and len(hist) == len(lines) == 2 and det.rpn_network.training is False and det.roi_model.training is True
    for h in hist:
        _finite(h, ("train_loss", "loss_objectness", "loss_rpn_box_reg", "ap_25", "ap_50"))
        total = h["loss_objectness"] + 5.0 * h["loss_rpn_box_reg"]
        assert list(h) == ["epoch", "train_loss", "loss_objectness", "loss_rpn_box_reg", "ap_25", "ap_50"] and abs(h["train_loss"] - total) <= 1e-5 * abs(total)
    assert sorted(os.listdir(tmp_path)) == ["epoch_2.pt", "model_best_ap25.pt", "model_best_ap50.pt"]
    fresh = D.two_stage(seed=3, fused=fused)
    backbone_before = {k: v.clone() for k, v in fresh.rpn_network.backbone.state_dict().items()}
    ck = load_two_stage_checkpoint(str(tmp_path / "epoch_2.pt"), fresh)
    assert list(ck) == ["epoch", "backbone_state_dict", "RCNN_dict", "rpn_state_dict", "train_args", "resume"] and ck["backbone_state_dict"] is None
    assert ck["train_args"]["mode"] == "head" and ck["train_args"]["fine_tune"] is False and ck["epoch"] == 2
    assert _state_equal(fresh.roi_model.RCNN_model.state_dict(), det.roi_model.RCNN_model.state_dict())
    assert _state_equal(fresh.rpn_network.rpn.state_dict(), det.rpn_network.rpn.state_dict())
    assert _state_equal(fresh.rpn_network.backbone.state_dict(), backbone_before), "the file carries no backbone"
    assert D.same(det.rpn_network, first0), "backbone and RPN head are where they started, bit for bit"
    assert all(p.grad is None or not p.grad.any() for p in det.rpn_network.parameters())
    assert _moved(det.roi_model.RCNN_model, head0) == [], "every parameter of the box head moved"
    tr.flat.check()
    first, kept = _detector_eval_by_hand(det)
    second, _ = _detector_eval_by_hand(det)
    assert first == second, "the by-hand evaluation repeats itself"
    assert max(kept) > 0 and len(kept) == len(D.VAL), kept
    _print(f"  [two-stage head, fused={fused}] detections per validation scene {kept}  record {first}")
    assert {k: hist[-1][k] for k in first} == first


def test_two_stage_trainer_joint_mode():
    from nerf_mae_amd.trainer import TwoStageTrainer
    det = D.two_stage(train_rpn=True).cuda().train()
    start = D.snapshot(det)
    tr = TwoStageTrainer(det, D.scenes(D.TRAIN), D.boxes(D.TRAIN), batch_size=2, num_epochs=1, lr=LR, weight_decay=WD, log=lambda s: None)
    assert tr.mode == "joint" and tr.frozen is None and det.first_stage_no_grad is False and tr.exclude == () and tr.flat.base is det.rpn_network.backbone.base
    hist = tr.fit()
    torch.cuda.synchronize()
    assert tr.global_step == 2 and len(hist) == 1 and list(hist[0]) == ["epoch", "train_loss", *JOINT_KEYS]
    h = hist[0]
    _finite(h, ("train_loss",) + JOINT_KEYS)
    total = h["loss_objectness"] + 5.0 * h["loss_rpn_box_reg"] + h["rpn_loss_objectness"] + 5.0 * h["rpn_loss_rpn_box_reg"] + 0.0 * h["rpn_loss_rpn_box_reg_2d"]
    assert abs(h["train_loss"] - total) <= 1e-5 * abs(total) and h["rpn_loss_rpn_box_reg"] > 0 and h["rpn_loss_objectness"] > 0
    still = [n for n, p in det.named_parameters() if p.requires_grad and torch.equal(p.detach(), start["p." + n])]
    assert still == [], "RPN head, backbone and box head all moved"
    tr.flat.check()


@pytest.mark.parametrize("mode", ["fine_tune", "heads"])
def test_two_stage_trainer_other_modes_move_what_they_should(mode):
    from nerf_mae_amd.trainer import TwoStageTrainer
    det = D.two_stage(train_rpn=mode == "heads").cuda().train()
    net = det.rpn_network
    backbone0, rpn0, head0 = D.snapshot(net.backbone), D.snapshot(net.rpn), D.snapshot(det.roi_model.RCNN_model)
    tr = TwoStageTrainer(det, D.scenes(D.TRAIN[:2]), D.boxes(D.TRAIN[:2]), batch_size=2, num_epochs=1, lr=LR, weight_decay=WD, freeze_first_stage=mode == "heads",
                         schedule_epochs=10, log=lambda s: None)
    # one step; the schedule is sized for ten, so that the step runs at the cycle's initial rate lr / 25 (a one-step cycle is its own last step, at lr / 2.5e5,
    # where AdamW's update of a LayerNorm weight of 1.0 is below fp32's resolution)
    assert tr.mode == mode and tr.steps_per_epoch == 1 and tr.sched.total == 10 and abs(tr.sched.at(0)[0] - LR / 25) < 1e-12
    hist = tr.fit()
    torch.cuda.synchronize()
    _finite(hist[0], ("train_loss", "loss_objectness", "loss_rpn_box_reg"))
    assert _moved(det.roi_model.RCNN_model, head0) == []
    if mode == "fine_tune":          # the detector's behaviour without a trainer: the pooling's gradient trains the backbone, the first stage's head stays
        assert det.first_stage_no_grad is False and tr.exclude == () and tr.flat.base is net.backbone.base
        assert D.same(net.rpn, rpn0) and [n for n in _moved(net.backbone, backbone0) if n != "base.pos_embed"] == []
    else:                            # the backbone alone is frozen; both heads train on its detached features
        assert det.first_stage_no_grad is True and tr.exclude == (net.backbone,) and tr.flat.base is None and net.backbone.training is False
        assert D.same(net.backbone, backbone0) and _moved(net.rpn, rpn0) == [] and hist[0]["rpn_loss_rpn_box_reg"] > 0
    tr.flat.check()


def test_two_stage_trainer_takes_its_first_stage_from_an_rpn_trainers_file(tmp_path):
    from nerf_mae_amd.trainer import RPNTrainer, TwoStageTrainer
    m = D.rpn_model(seed=5).cuda().train()
    RPNTrainer(m, D.scenes((11,)), D.boxes((11,)), D.scenes((14,)), D.boxes((14,)), batch_size=1, num_epochs=1, lr=LR, freeze_backbone=True, save_path=str(tmp_path),
               log=lambda s: None).fit()
    torch.cuda.synchronize()
    path = str(tmp_path / "epoch_1.pt")
    det = D.two_stage(seed=7).cuda().train()
    assert not _state_equal(det.rpn_network.rpn.head.state_dict(), m.rpn.head.state_dict())
    tr = TwoStageTrainer(det, D.scenes((11,)), D.boxes((11,)), batch_size=1, num_epochs=1, log=lambda s: None)
    ck = tr.init_from_rpn(path)
    assert _state_equal(det.rpn_network.backbone.state_dict(), ck["backbone_state_dict"]) and _state_equal(det.rpn_network.rpn.head.state_dict(), ck["rpn_head_state_dict"])
    assert _state_equal(det.rpn_network.state_dict(), m.state_dict())
    tr.flat.check()
    tr.fit()                                                  # and trains from there
    torch.cuda.synchronize()
    assert _state_equal(det.rpn_network.state_dict(), m.state_dict()), "head mode leaves the loaded first stage alone"
