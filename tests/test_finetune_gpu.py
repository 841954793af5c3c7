"""finetune.FlatParameters / FinetuneStep and trainer.DetectionTrainer on the GPU, on the common small models of tests/_finetune_common.py (resolution 32,
swin_t, 64 FPN channels, fp32 compute; FCOS with num_convs=2 and oriented boxes), two synthetic scenes with two oriented boxes each per batch.

  optimizer arithmetic   FusedAdamW over the composite buffer against torch.optim.AdamW + clip_grad_norm_ on CPU copies fed the same gradients, the bounds of
                         tests/test_kernels_gpu.py::test_adamw_and_clip_match_torch (norm 1e-5 relative, parameters relerr < 1e-5)
  the step               three FinetuneSteps (A) against the same three steps with torch.optim.AdamW(model.parameters()) + clip_grad_norm_ (B, and B' for the
                         stock path's own run-to-run spread): relerr(A, B) <= 3 * 1e-5 + 4 * relerr(B, B')
  generality             eight steps lower the loss of FCOSOverNeRF, NeRFRegionProposalNetwork and the voxel-semantics head
  resume                 two steps, checkpoint, fresh model and optimizer, third step == three uninterrupted steps within the bound above
  DetectionTrainer.fit   two epochs over three scenes with evaluation and the reference's checkpoint names
  the epoch loop         the batcher receives dp_epoch_plan's batches, and the trainer's generator is drawn from once per scene in that order and by nothing else
  DetectionTrainer.resume  one epoch + checkpoint + fresh trainer + one epoch against two uninterrupted epochs: relerr <= 3 * 1e-5 + 4 relerr(U, U'), the
                         construction of tests/test_voxel_trainer_gpu.py::test_true_resume_continues_where_it_stopped (stochastic depth off, AdamW's eps 1)

relerr over a set of tensors is the LARGEST of the per-tensor tests/_metrics.relerr (max |a - b| / max |b|), so a small tensor is not hidden behind a large one."""
import functools
import glob
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402
from tests._metrics import relerr  # noqa: E402

pytestmark = pytest.mark.gpu
LR, WD, CLIP, EPS = 1e-3, 1e-3, 0.1, 1.0
STEP_BOUND = 1e-5                        # the project's per-step optimizer bound (test_adamw_and_clip_match_torch)
KEYS = ("loss_cls", "loss_reg", "loss_centerness")


def _print(*a):
    if os.environ.get("NMH_PRINT_ERR"):
        print(*a)


def worst(a, b):
    """largest per-tensor relerr of two {name: tensor} dicts with the same keys"""
    assert list(a) == list(b)
    return max(relerr(a[k], b[k]) for k in a)


def params_of(module):
    return {n: p.detach().clone() for n, p in module.named_parameters()}


@functools.lru_cache(maxsize=None)
def batches():
    """three batches of two scenes through DetectionBatcher (no augmentation): [(meshes, targets)], device tensors"""
    from nerf_mae_amd import data
    batcher = data.DetectionBatcher(C.R, torch.device("cuda"), normalize_density=True)
    out = []
    for k in range(3):
        seeds = (2 * k + 1, 2 * k + 2)
        xb, ext, targets = batcher.prepare([C.scene(s) for s in seeds], [C.obb_boxes(s) for s in seeds], params=[(0, 0.0, 1.0)] * 2)
        assert ext == [[C.R] * 3] * 2
        out.append(([xb[i].clone() for i in range(2)], [t.clone() for t in targets]))
    torch.cuda.synchronize()
    return out


@functools.lru_cache(maxsize=None)
def weights():
    return {k: v.clone() for k, v in C.fcos_model().state_dict().items()}


def fcos_on_gpu():
    m = C.fcos_model()
    m.load_state_dict(weights(), strict=True)
    return m.cuda().train()


def fused(model, eps=EPS, lr=LR):
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for
    from nerf_mae_amd.trainer import FusedAdamW
    flat = FlatParameters(model, torch.device("cuda"))
    opt = FusedAdamW(flat, lr=lr, weight_decay=WD, eps=eps, max_grad_norm=CLIP)
    return flat, opt, FinetuneStep(flat, opt, loss_fn_for(model))


def fused_steps(step, opt, ks):
    losses, norms = [], []
    for k in ks:
        meshes, targets = batches()[k]
        torch.manual_seed(100 + k)
        out = step(meshes, targets)
        losses.append(torch.stack([out[key] for key in KEYS]))
        norms.append(opt.norm.clone())
    return losses, norms


def stock_steps(model, ks=(0, 1, 2)):
    """the only training path of the parent commit: torch.optim.AdamW over the separate tensors + clip_grad_norm_"""
    opt = torch.optim.AdamW(model.parameters(), lr=LR, weight_decay=WD, eps=EPS)
    losses = []
    for k in ks:
        meshes, targets = batches()[k]
        opt.zero_grad(set_to_none=False)
        torch.manual_seed(100 + k)
        out = model(list(meshes), targets)[1]
        (out["loss_cls"] + out["loss_reg"] + out["loss_centerness"]).backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), CLIP)
        opt.step()
        losses.append(torch.stack([out[key].detach() for key in KEYS]))
    return losses


@functools.lru_cache(maxsize=None)
def three_step_runs():
    """A: three FinetuneSteps; B, B': the stock path twice.  Computed once, shared by the step test and the resume test, left unchanged."""
    A, B, B2 = fcos_on_gpu(), fcos_on_gpu(), fcos_on_gpu()
    before = params_of(A)
    flat, opt, step = fused(A)
    la, norms = fused_steps(step, opt, (0, 1, 2))
    lb, lb2 = stock_steps(B), stock_steps(B2)
    torch.cuda.synchronize()
    pa, pb, pb2 = params_of(A), params_of(B), params_of(B2)
    spread_p, spread_l = worst(pb2, pb), max(relerr(x, y) for x, y in zip(lb2, lb))
    return dict(before=before, pa=pa, pb=pb, la=la, lb=lb, norms=[float(n) for n in norms], spread_p=spread_p, spread_l=spread_l,
                bound_p=3 * STEP_BOUND + 4 * spread_p, bound_l=3 * STEP_BOUND + 4 * spread_l)


def test_fused_adamw_over_the_composite_buffer_matches_torch():
    """gradients written through the parameters' .grad VIEWS; step 1 and 2 clip (norm about 3.9 and 0.39), step 3 does not (0.039); lr and beta1 change
    between the steps.  The CPU copies are float64: with float32 copies the stock path's own norm is off by 1.6e-5 from the exact value on these 30 M elements
    (torch's fp32 CPU reduction: 3.880089 against 3.880150 in float64, up to 3e-5 on a single 2.4 M-element tensor; FusedAdamW gave 3.88015), more than the
    1e-5 this test allows for the kernel.  Same functions, same gradients, same bounds."""
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.trainer import FusedAdamW
    m = fcos_on_gpu()
    flat = FlatParameters(m, torch.device("cuda"))
    opt = FusedAdamW(flat, lr=1e-3, weight_decay=1e-2, max_grad_norm=CLIP)
    opt.zero_grads_after_step = True                               # as FinetuneStep runs it
    named = [(n, p) for n, p in m.named_parameters() if p.requires_grad]
    assert len(named) == 212
    ref = [p.detach().cpu().double().requires_grad_(True) for _, p in named]
    topt = torch.optim.AdamW(ref, lr=1e-3, weight_decay=1e-2, betas=(0.9, 0.999))
    sched = ((1e-3, 1e-3, 0.9), (1e-4, 5e-4, 0.85), (1e-5, 2e-3, 0.95))      # (gradient scale, lr, beta1)
    norms = []
    for scale, lr, b1 in sched:
        for i, ((n, p), r) in enumerate(zip(named, ref)):
            g = scale * torch.sin(0.37 * i + 1e-3 * torch.arange(p.numel(), device="cuda", dtype=torch.float32)).view(p.shape)
            p.grad.copy_(g)
            r.grad = g.cpu().double()
        flat.check()
        opt.set_hyper(lr=lr, beta1=b1)
        opt.step()
        topt.param_groups[0]["lr"], topt.param_groups[0]["betas"] = lr, (b1, 0.999)
        tn = torch.nn.utils.clip_grad_norm_(ref, CLIP)
        topt.step()
        norms.append(tn.item())
        e = abs(opt.norm.item() - tn.item()) / tn.item()
        _print(f"  [composite adamw] norm {opt.norm.item():.6g} vs {tn.item():.6g} rel {e:.2e}")
        assert e < 1e-5
    assert norms[0] > CLIP and norms[1] > CLIP and norms[2] < CLIP
    got = dict(m.named_parameters())
    errs = {n: relerr(got[n], r) for (n, _), r in zip(named, ref)}
    name = max(errs, key=errs.get)
    _print(f"  [composite adamw] worst parameter relerr {errs[name]:.2e} ({name})")
    assert errs[name] < 1e-5, (name, errs[name])
    assert not flat._flat_grad.any(), "the update clears the flat gradient buffer"


def test_finetune_step_matches_the_stock_optimizer_path():
    """relerr(A, B) <= 3 * 1e-5 + 4 * relerr(B, B') over all parameters and over the three loss values of each step.  eps = 1.0 (the device of
    tests/test_dist_gpu.py): the update stays linear in tiny gradients, so the order noise of fp32 atomics is not blown up to +-lr.  Not vacuous: the
    parameters moved by at least 100 x the bound (largest per-tensor max |after - before| / max |after|), the gradient norm exceeded the clip in some step, and
    loss_reg > 0 at the first step (the batch has positives)."""
    r = three_step_runs()
    assert r["la"][0][1].item() > 0, "loss_reg > 0 at the first step: the batch has positive locations"
    assert all(torch.isfinite(l).all() for l in r["la"])
    err_p = worst(r["pa"], r["pb"])
    err_l = max(relerr(x, y) for x, y in zip(r["la"], r["lb"]))
    moved = worst(r["before"], r["pa"])
    _print(f"  [finetune step] parameters relerr(A,B) {err_p:.2e}  relerr(B,B') {r['spread_p']:.2e}  bound {r['bound_p']:.2e}  moved {moved:.2e}")
    _print(f"  [finetune step] losses     relerr(A,B) {err_l:.2e}  relerr(B,B') {r['spread_l']:.2e}  bound {r['bound_l']:.2e}  grad norms {r['norms']}")
    assert err_p <= r["bound_p"], (err_p, r["bound_p"])
    assert err_l <= r["bound_l"], (err_l, r["bound_l"])
    assert moved >= 100 * r["bound_p"], (moved, r["bound_p"])
    assert max(r["norms"]) > CLIP


def _descends(model, batch, before_forward=None, steps=8):
    flat, opt, step = fused(model, eps=1e-8, lr=2e-4)
    totals = []
    for _ in range(steps):
        torch.manual_seed(7)                                       # the same stochastic-depth draw in every step
        if before_forward is not None:
            before_forward()
        out = step(*batch)
        totals.append(torch.stack(list(out.values())).sum())
    totals = torch.stack(totals).tolist()
    _print(f"  [{type(model).__name__}] totals {['%.5g' % t for t in totals]}")
    assert all(t == t for t in totals) and totals[-1] < totals[0], totals
    flat.check()


def test_eight_steps_lower_the_fcos_loss():
    _descends(fcos_on_gpu(), batches()[0])


def test_eight_steps_lower_the_rpn_loss():
    m = C.rpn_model().cuda().train()
    assert m.check_targets is False
    meshes, _ = batches()[0]
    targets = [torch.from_numpy(C.aabb_boxes(s)).cuda() for s in (1, 2)]
    state0 = torch.tensor([m.rpn.loss.seed, 0], dtype=torch.int64, device="cuda")

    def same_sample():                                             # the anchor sampler's draw is replayed as well: one fixed objective
        if m.rpn.loss.rng_state is not None:
            m.rpn.loss.rng_state.copy_(state0)

    _descends(m, (meshes, targets), same_sample)


def test_eight_steps_lower_the_voxel_semantics_loss():
    m = C.semantics_model().cuda().train()
    meshes, _ = batches()[0]
    labels = [C.label_grid(s).cuda() for s in (1, 2)]
    _descends(m, (meshes, labels))


def test_true_resume_continues_where_it_stopped(tmp_path):
    from nerf_mae_amd.trainer import load_detection_checkpoint, save_detection_checkpoint
    r = three_step_runs()
    m = fcos_on_gpu()
    flat, opt, step = fused(m)
    fused_steps(step, opt, (0, 1))
    path = str(tmp_path / "resume.pt")
    save_detection_checkpoint(path, m, 1, {"lr": LR}, opt, step=2)
    m2 = C.fcos_model(seed=9).cuda().train()
    flat2, opt2, step2 = fused(m2)
    ck = load_detection_checkpoint(path, m2, opt2)
    flat2.check()
    assert ck["resume"]["step"] == 2 and opt2.t == 2 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
    fused_steps(step2, opt2, (2,))
    torch.cuda.synchronize()
    err = worst(params_of(m2), r["pa"])
    _print(f"  [resume] relerr(resumed, uninterrupted) {err:.2e}  bound {r['bound_p']:.2e}")
    assert err <= r["bound_p"], (err, r["bound_p"])


def test_detection_trainer_fit(tmp_path):
    """three training scenes (a ragged last batch of one), two validation scenes, two epochs.  cls_logits.bias is raised to -1 as tests/test_fcos_network_gpu.py
    does, so that the untrained head's scores pass pre_nms_thresh and the metrics have detections to score."""
    from nerf_mae_amd.trainer import DetectionTrainer, load_detection_checkpoint
    m = fcos_on_gpu()
    with torch.no_grad():
        m.fcos_module.head.cls_logits.bias.fill_(-1.0)
    lines = []
    tr = DetectionTrainer(m, [C.scene(s) for s in (11, 12, 13)], [C.obb_boxes(s) for s in (11, 12, 13)], [C.scene(s) for s in (14, 15)],
                          [C.obb_boxes(s) for s in (14, 15)], batch_size=2, num_epochs=2, lr=1e-4, weight_decay=1e-3, eval_interval=1, save_path=str(tmp_path),
                          normalize_density=True, flip_prob=0.5, rotate_prob=0.5, rot_scale_prob=0.5, log=lines.append)
    assert tr.steps_per_epoch == 2 and tr.sched.total == 1000 * 2 and tr.limits == [15]
    hist = tr.fit()
    assert tr.global_step == 4 and len(hist) == len(lines) == 2 and [h["epoch"] for h in hist] == [1, 2]
    for h in hist:
        for k in ("train_loss", "loss_cls", "loss_reg", "loss_centerness", "ap_25", "ap_50", "recall_25_top_15", "recall_50_top_15", "recall_ar_top_15"):
            assert k in h and h[k] == h[k] and abs(h[k]) != float("inf"), (k, h)
        assert abs(h["train_loss"] - (h["loss_cls"] + h["loss_reg"] + h["loss_centerness"])) <= 1e-5 * abs(h["train_loss"]) and h["loss_reg"] > 0
    by50, by25 = glob.glob(str(tmp_path / "model_best_ap50_ap25_*_*.pt")), glob.glob(str(tmp_path / "model_best_ap25_ap50_*_*.pt"))
    assert by50 and by25 and len(os.listdir(tmp_path)) <= 6
    fresh = C.fcos_model(seed=3)
    for path in (by50[0], by25[0]):
        ck = load_detection_checkpoint(path, fresh)
        assert sorted(ck) == ["backbone_state_dict", "epoch", "fcos_state_dict", "resume", "train_args"] and ck["train_args"]["batch_size"] == 2
        float(os.path.basename(path)[:-3].split("_")[-1]), float(os.path.basename(path).split("_")[-2])
    tr.flat.check()


def test_train_epoch_follows_the_plan_and_draws_scene_by_scene():
    """the shared epoch loop hands the batcher exactly the batches of dp_epoch_plan, and the trainer's generator ends where a fresh one ends after one
    draw_detection_augmentation per scene in that order: drawn scene by scene, batch by batch, and nothing else uses the generator"""
    import random
    from nerf_mae_amd.data import draw_detection_augmentation
    from nerf_mae_amd.trainer import DetectionTrainer, dp_epoch_plan
    seed, scenes = 4, [C.scene(s) for s in (11, 12, 13)]
    tr = DetectionTrainer(fcos_on_gpu(), scenes, [C.obb_boxes(s) for s in (11, 12, 13)], batch_size=2, num_epochs=1, lr=1e-4, flip_prob=0.5, rotate_prob=0.5,
                          rot_scale_prob=0.5, log=lambda s: None, seed=seed)
    seen = C.record_batches(tr, scenes)
    tr.train_epoch(1)
    plan = dp_epoch_plan(3, 2, 0, 1, 1, seed)
    assert seen == plan and [len(ids) for ids in plan] == [2, 1]
    rng = random.Random(seed + 1000003 * 0)
    for ids in plan:
        for _ in ids:
            draw_detection_augmentation(0.5, 0.5, 0.5, True, rng)
    assert rng.getstate() == tr._rng.getstate()


# ---- DetectionTrainer.resume: the twin of tests/test_voxel_trainer_gpu.py::test_true_resume_continues_where_it_stopped ------------------------------------
def _resume_trainer(seed=0):
    from nerf_mae_amd.trainer import DetectionTrainer
    from tests._voxel_common import no_stochastic_depth
    m = no_stochastic_depth(C.fcos_model(seed)).cuda().train()
    tr = DetectionTrainer(m, [C.scene(s) for s in (11, 12)], [C.obb_boxes(s) for s in (11, 12)], batch_size=1, num_epochs=2, lr=LR, weight_decay=WD,
                          log=lambda s: None)
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


def test_detection_trainer_resume_continues_where_it_stopped(tmp_path):
    """one epoch + checkpoint + fresh trainer + resume() + one epoch against two uninterrupted epochs: relerr <= 3 * 1e-5 + 4 relerr(U, U')"""
    from nerf_mae_amd.trainer import save_detection_checkpoint
    u, u2 = _uninterrupted()
    a = _resume_trainer()
    a.train_epoch(1)
    path = str(tmp_path / "epoch_1.pt")
    save_detection_checkpoint(path, a.model, 1, a.args, a.opt, a.global_step)
    b = _resume_trainer(seed=9)          # other weights: everything must come from the file
    ck = b.resume(path)
    assert ck["resume"]["step"] == 2 and b.global_step == 2 and b.start_epoch == 2 and b.opt.t == 2
    assert torch.equal(b.opt.m, a.opt.m) and torch.equal(b.opt.v, a.opt.v) and torch.equal(b.flat._flat, a.flat._flat)
    hist = b.fit()
    torch.cuda.synchronize()
    assert [h["epoch"] for h in hist] == [2] and b.global_step == 4
    err, spread = relerr(b.flat._flat, u), relerr(u2, u)
    _print(f"  [detection resume] relerr(resumed, uninterrupted) {err:.2e}  relerr(U, U') {spread:.2e}  bound {3 * STEP_BOUND + 4 * spread:.2e}")
    assert err <= 3 * STEP_BOUND + 4 * spread, (err, spread)
