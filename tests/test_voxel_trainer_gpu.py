"""trainer.VoxelTrainer and the heads' dense targets on the GPU, on the common small models of tests/_finetune_common.py (resolution 32, fp32 compute, the heads'
swin_s base) with stochastic depth off; the SR head has out_resolution=256, so its output resolution is int(32 * 1.6) = 51.

  dense vs list     loss_fn on the batcher's dense target against the list of per-scene grids, on a fixed seeded `pred` without a network.  Both loss kernels
                    reduce with atomics, so two runs of the SAME path differ in the last bits: relerr(dense, list) <= 2.4e-7 (two fp32 ulps) + 4 relerr(list, list'),
                    list' being a second run of the list path.  output_metrics of the semantics head sums in a fixed order: torch.equal.
  fit               three scenes with batch 2 (a ragged last batch), two validation scenes, two epochs: history, schedule, model_best.pt, for both heads
  best selection    a scripted evaluate: one file, from the best epoch
  true resume       one epoch + checkpoint + fresh trainer + one epoch against two uninterrupted epochs: relerr <= 3 * 1e-5 + 4 relerr(U, U'), the construction and
                    constants of tests/test_finetune_gpu.py::test_true_resume_continues_where_it_stopped with the uninterrupted run's own spread in the place of
                    the stock path's (there is no stock voxel trainer); AdamW's eps is 1 as there, so the order noise of fp32 atomics is not blown up to +-lr
  the epoch loop    the batcher receives dp_epoch_plan's batches; the trainer's generator is drawn from once per scene in that order and by nothing else
  augmentation on   runs and gives a finite loss (the reference cannot run this configuration: nothing to compare with)
  two ranks         on one GPU over gloo: bit-equal parameters, files and evaluation on rank 0 only

NMH_PRINT_ERR=1 prints every measured value."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402
from tests import _voxel_common as V  # noqa: E402
from tests import _voxel_input_ref as P  # noqa: E402
from tests._metrics import relerr  # noqa: E402

pytestmark = pytest.mark.gpu
ULPS2 = 2.4e-7          # two fp32 ulps
SEM_KEYS = ["epoch", "train_loss", "train_iou", "mIoU", "mAcc", "allAcc"]
SR_KEYS = ["epoch", "train_loss", "psnr", "mse"]


def _finite(h, keys):
    for k in keys:
        assert k in h and h[k] == h[k] and abs(h[k]) != float("inf"), (k, h)


# ---- dense against list targets -------------------------------------------------------------------------------------------------------------------------
def _loss_and_grad(fn, pred):
    p = pred.clone().requires_grad_(True)
    out = fn(p)
    loss = out[0] if isinstance(out, tuple) else out
    loss.backward()
    return torch.stack([o.detach() for o in out]) if isinstance(out, tuple) else loss.detach().reshape(1), p.grad


def _check_dense_against_list(name, head, pred, dense, as_list):
    ld, gd = _loss_and_grad(lambda p: head.loss_fn(dense, p), pred)
    l1, g1 = _loss_and_grad(lambda p: head.loss_fn(as_list, p), pred)
    l2, g2 = _loss_and_grad(lambda p: head.loss_fn(as_list, p), pred)
    torch.cuda.synchronize()
    assert g1.abs().max() > 0
    for what, d, a, b in (("loss", ld, l1, l2), ("gradient", gd, g1, g2)):
        err, spread = relerr(d, a), relerr(b, a)
        V.print_err(f"  [{name} dense vs list, {what}] relerr(dense, list) {err:.2e}  relerr(list, list') {spread:.2e}  bound {ULPS2 + 4 * spread:.2e}")
        assert err <= ULPS2 + 4 * spread, (name, what, err, spread)


def test_semantics_dense_labels_equal_the_list_form():
    from nerf_mae_amd import data
    head = V.semantics_model()
    seeds = (1, 2)
    vols = [V.label_volume(s)[0, :30 - 3 * i, :, :27] for i, s in enumerate(seeds)]          # (W,L,H) of different extents: the dense form carries the padding
    scenes = [data.synthetic_scene(v.shape, s, dtype=np.uint8) for v, s in zip(vols, seeds)]
    _, _, dense = data.VoxelBatcher(C.R, "cuda", target="labels").prepare(scenes, vols, flags=[0, 0])
    as_list = [torch.from_numpy(np.ascontiguousarray(v))[None].cuda() for v in vols]
    pred = torch.randn((2, head.out_channels, C.R, C.R, C.R), generator=torch.Generator().manual_seed(3)).cuda()
    _check_dense_against_list("semantics", head, pred, dense, as_list)
    ce_d, m_d, pv_d, tv_d = head.output_metrics(dense, pred)
    ce_l, m_l, pv_l, tv_l = head.output_metrics(as_list, pred)
    assert torch.equal(pv_d, pv_l) and torch.equal(tv_d, tv_l) and torch.equal(ce_d, ce_l)
    for k in ("intersection", "union", "target", "area_pred", "iou_val"):
        assert torch.equal(m_d[k], m_l[k]), k
    for bad in (dense[:, :31], dense.double(), dense.cpu(), dense.transpose(1, 2), dense[:, None]):
        with pytest.raises(ValueError, match="float32"):
            head.loss_fn(bad, pred)


def test_sr_dense_target_equals_the_list_form():
    from nerf_mae_amd import data
    from nerf_mae_amd.heads import SREvaluator
    head = V.sr_model()
    shapes = [(40, V.RO, 37), (V.RO, 45, V.RO)]
    his = [data.synthetic_scene(sh, 60 + i, dtype=np.uint8) for i, sh in enumerate(shapes)]
    los = [data.synthetic_scene((25, C.R, 23), 70, dtype=np.uint8), data.synthetic_scene((C.R, 28, C.R), 71, dtype=np.uint8)]
    _, _, dense = data.VoxelBatcher(C.R, "cuda", target="grid", target_resolution=V.RO).prepare(los, his, flags=[0, 0])
    as_list = [torch.from_numpy(P.grid_ref(h, V.RO, 0))[:, :sh[0], :sh[1], :sh[2]].cuda() for h, sh in zip(his, shapes)]
    pred = torch.rand((2, 4, V.RO, V.RO, V.RO), generator=torch.Generator().manual_seed(4)).cuda()
    _check_dense_against_list("SR", head, pred, dense, as_list)
    want = head.output_metrics(as_list, pred)
    got = head.output_metrics(dense, pred)
    ev = SREvaluator(head)
    ev.update(dense, pred)
    ev.update(as_list, pred * 0.5)
    out = ev.compute()
    half = head.output_metrics(as_list, pred * 0.5)
    for k in ("MSE", "PSNR"):
        assert abs(got[k] - want[k]) <= 1e-6 * abs(want[k])
    assert abs(out["psnr_mean"] - (want["PSNR"] + half["PSNR"]) / 2) <= 1e-5 * abs(want["PSNR"])          # the mean of the per-batch values
    assert abs(out["mse_mean"] - (want["MSE"] + half["MSE"]) / 2) <= 1e-5 * want["MSE"]
    for bad in (dense[:, :3], dense.double(), dense.cpu(), dense.transpose(2, 3)):
        with pytest.raises(ValueError, match="float32"):
            head.loss_fn(bad, pred)


# ---- fit ------------------------------------------------------------------------------------------------------------------------------------------------
def _check_best(tmp_path, hist, key, fresh):
    from nerf_mae_amd.trainer import load_voxel_checkpoint
    assert os.listdir(tmp_path) == ["model_best.pt"]
    ck = load_voxel_checkpoint(str(tmp_path / "model_best.pt"), fresh)          # strict
    assert sorted(ck) == ["epoch", "resume", "state_dict", "train_args"] and ck["train_args"]["batch_size"] == 2 and ck["train_args"]["num_epochs"] == 2
    vals = [h[key] for h in hist]
    assert ck["epoch"] == (2 if vals[1] > vals[0] else 1), (ck["epoch"], vals)
    plain = {k: v for k, v in ck.items() if k != "resume"}          # a reference-written file has no resume section: the weights load all the same
    torch.save(plain, str(tmp_path / "plain.pt"))
    assert "resume" not in load_voxel_checkpoint(str(tmp_path / "plain.pt"), fresh)


def test_voxel_trainer_fit_semantics(tmp_path):
    from nerf_mae_amd.trainer import VoxelTrainer
    m = V.semantics_model()
    lines = []
    tr = VoxelTrainer(m, [C.scene(s) for s in (11, 12, 13)], [V.label_volume(s) for s in (11, 12, 13)], [C.scene(s) for s in (14, 15)],
                      [V.label_volume(s) for s in (14, 15)], batch_size=2, num_epochs=2, lr=1e-3, eval_interval=1, save_path=str(tmp_path), log=lines.append)
    assert tr.steps_per_epoch == 2 and tr.sched.total == 2 * 2 and tr.batcher.target == "labels"
    hist = tr.fit()
    assert tr.global_step == 4 and len(hist) == len(lines) == 2 and [list(h) for h in hist] == [SEM_KEYS] * 2
    for h in hist:
        _finite(h, SEM_KEYS)
        assert h["train_loss"] > 0 and 0 <= h["mIoU"] <= 1 and 0 <= h["allAcc"] <= 1
    _check_best(tmp_path, hist, "mIoU", C.semantics_model(seed=3))
    tr.flat.check()


def test_voxel_trainer_fit_sr(tmp_path):
    from nerf_mae_amd.trainer import VoxelTrainer
    m = V.sr_model()
    lines = []
    tr = VoxelTrainer(m, [C.scene(s) for s in (11, 12, 13)], [V.sr_target(s) for s in (11, 12, 13)], [C.scene(s) for s in (14, 15)],
                      [V.sr_target(s) for s in (14, 15)], batch_size=2, num_epochs=2, lr=1e-3, eval_interval=1, save_path=str(tmp_path), log=lines.append)
    assert tr.steps_per_epoch == 2 and tr.sched.total == 2 * 2 and tr.batcher.target == "grid" and tr.batcher.Ro == V.RO
    hist = tr.fit()
    assert tr.global_step == 4 and len(hist) == len(lines) == 2 and [list(h) for h in hist] == [SR_KEYS] * 2
    for h in hist:
        _finite(h, SR_KEYS)
        assert h["train_loss"] > 0 and h["mse"] > 0 and abs(h["psnr"] + 10 * np.log10(h["mse"])) < 1.0          # (means of per-batch values: close, not equal)
    _check_best(tmp_path, hist, "psnr", V.sr_model(seed=3))
    tr.flat.check()


def test_best_checkpoint_follows_the_metric(tmp_path):
    """evaluate replaced by the scripted sequence 0.2, 0.5, 0.3: the file is written at epoch 1, replaced at epoch 2 and left alone at epoch 3"""
    from nerf_mae_amd.trainer import VoxelTrainer
    m = V.semantics_model()
    tr = VoxelTrainer(m, [C.scene(11)], [V.label_volume(11)], [C.scene(14)], [V.label_volume(14)], batch_size=1, num_epochs=3, lr=1e-3,
                      save_path=str(tmp_path), log=lambda s: None)
    script = iter((0.2, 0.5, 0.3))
    tr.evaluate = lambda: {"mIoU": next(script), "mAcc": 0.0, "allAcc": 0.0}
    hist = tr.fit()
    assert [h["mIoU"] for h in hist] == [0.2, 0.5, 0.3] and tr.best_metric == 0.5
    assert os.listdir(tmp_path) == ["model_best.pt"]
    ck = torch.load(str(tmp_path / "model_best.pt"), weights_only=True)
    assert ck["epoch"] == 2 and ck["resume"]["step"] == 2


# ---- true resume ----------------------------------------------------------------------------------------------------------------------------------------
def _resume_trainer(seed=0):
    from nerf_mae_amd.trainer import VoxelTrainer
    tr = VoxelTrainer(V.semantics_model(seed), [C.scene(s) for s in (11, 12)], [V.label_volume(s) for s in (11, 12)], batch_size=1, num_epochs=2, lr=1e-3,
                      weight_decay=1e-3, log=lambda s: None)
    tr.opt.eps = 1.0
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


def test_true_resume_continues_where_it_stopped(tmp_path):
    from nerf_mae_amd.trainer import save_voxel_checkpoint
    u, u2 = _uninterrupted()
    a = _resume_trainer()
    a.train_epoch(1)
    path = str(tmp_path / "epoch_1.pt")
    save_voxel_checkpoint(path, a.model, 1, a.args, a.opt, a.global_step)
    b = _resume_trainer(seed=9)          # other weights: everything must come from the file
    ck = b.resume(path)
    assert ck["resume"]["step"] == 2 and b.global_step == 2 and b.start_epoch == 2 and b.opt.t == 2
    assert torch.equal(b.opt.m, a.opt.m) and torch.equal(b.opt.v, a.opt.v) and torch.equal(b.flat._flat, a.flat._flat)
    hist = b.fit()
    torch.cuda.synchronize()
    assert [h["epoch"] for h in hist] == [2] and b.global_step == 4
    err, spread = relerr(b.flat._flat, u), relerr(u2, u)
    V.print_err(f"  [voxel resume] relerr(resumed, uninterrupted) {err:.2e}  relerr(U, U') {spread:.2e}  bound {3e-5 + 4 * spread:.2e}")
    assert err <= 3 * 1e-5 + 4 * spread, (err, spread)


# ---- augmentation, refusals -------------------------------------------------------------------------------------------------------------------------------
def test_paired_augmentation_runs():
    from nerf_mae_amd.trainer import VoxelTrainer
    tr = VoxelTrainer(V.semantics_model(), [C.scene(s) for s in (11, 12)], [V.label_volume(s) for s in (11, 12)], batch_size=2, num_epochs=1, lr=1e-3,
                      flip_prob=0.5, rotate_prob=0.5, log=lambda s: None)
    drawn = []
    draw = tr.batcher.draw_flags
    tr.batcher.draw_flags = lambda n, rng: (drawn.append(draw(n, rng)), drawn[-1])[1]
    hist = tr.fit()
    assert len(drawn) == 1 and len(drawn[0]) == 2
    _finite(hist[0], ["train_loss", "train_iou"])
    assert hist[0]["train_loss"] > 0


def test_refusals():
    from nerf_mae_amd.trainer import VoxelTrainer
    m = V.semantics_model()
    with pytest.raises(ValueError, match="rot_scale_prob"):
        VoxelTrainer(m, [C.scene(11)], [V.label_volume(11)], rot_scale_prob=0.1)
    with pytest.raises(TypeError, match="neither voxel head"):
        VoxelTrainer(C.fcos_model().cuda(), [C.scene(11)], [C.obb_boxes(11)])
    with pytest.raises(ValueError, match="one target per scene"):
        VoxelTrainer(m, [C.scene(11), C.scene(12)], [V.label_volume(11)])


# ---- two ranks on one GPU over gloo -------------------------------------------------------------------------------------------------------------------------
def _trainer_worker(rank, world, port, out_dir, q):
    import torch.distributed as dist
    V.init_gloo(rank, world, port)
    try:
        from nerf_mae_amd.trainer import VoxelTrainer
        m = V.semantics_model(seed=rank)          # another initialisation on rank 1: the broadcast must equalise it
        save = os.path.join(out_dir, f"rank{rank}")
        lines = []
        tr = VoxelTrainer(m, [C.scene(s) for s in (11, 12, 13, 14)], [V.label_volume(s) for s in (11, 12, 13, 14)], [C.scene(s) for s in (15, 16)],
                          [V.label_volume(s) for s in (15, 16)], batch_size=1, num_epochs=2, lr=1e-3, eval_interval=1, save_path=save, log=lines.append,
                          rank=rank, world=world)
        assert tr.steps_per_epoch == 2 and tr.args["batch_size"] == 2 and tr.reducer is not None and tr.reducer.active
        hist = tr.fit()
        torch.cuda.synchronize()
        assert tr.global_step == 4 and len(lines) == (2 if rank == 0 else 0)
        final = tr.flat._flat.detach().cpu()
        both = [torch.empty_like(final) for _ in range(world)]
        dist.all_gather(both, final)
        assert torch.equal(both[0], both[1]), (both[0] - both[1]).abs().max()
        tr.flat.check()
        q.put((rank, "ok", hist))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_voxel_trainer_fit_on_two_ranks(tmp_path):
    """four scenes, per-rank batch 1, two epochs, semantics: bit-equal parameters on both ranks (asserted in the children), only rank 0 evaluates and writes,
    both report the same training losses"""
    port = 25300 + (os.getpid() % 2000)
    hist = V.spawn(_trainer_worker, lambda r: (r, 2, port, str(tmp_path)))
    assert [list(h) for h in hist[1]] == [SEM_KEYS[:3]] * 2 and [list(h) for h in hist[0]] == [SEM_KEYS] * 2
    for h0, h1 in zip(hist[0], hist[1]):
        _finite(h0, SEM_KEYS)
        assert all(h0[k] == h1[k] for k in SEM_KEYS[:3]), (h0, h1)
    assert os.listdir(tmp_path / "rank0") == ["model_best.pt"]
    assert not os.path.exists(tmp_path / "rank1") or not os.listdir(tmp_path / "rank1")


def test_train_epoch_follows_the_plan_and_draws_scene_by_scene():
    """the voxel twin of tests/test_finetune_gpu.py's test of the same name: the batches are dp_epoch_plan's, one draw_augmentation per scene in that order"""
    import random
    from nerf_mae_amd.data import draw_augmentation
    from nerf_mae_amd.trainer import VoxelTrainer, dp_epoch_plan
    seed, scenes = 4, [C.scene(s) for s in (11, 12, 13)]
    tr = VoxelTrainer(V.semantics_model(), scenes, [V.label_volume(s) for s in (11, 12, 13)], batch_size=2, num_epochs=1, lr=1e-3, flip_prob=0.5,
                      rotate_prob=0.5, log=lambda s: None, seed=seed)
    seen = C.record_batches(tr, scenes)
    tr.train_epoch(1)
    plan = dp_epoch_plan(3, 2, 0, 1, 1, seed)
    assert seen == plan and [len(ids) for ids in plan] == [2, 1]
    rng = random.Random(seed + 1000003 * 0)
    for ids in plan:
        for _ in ids:
            draw_augmentation(0.5, 0.5, rng)
    assert rng.getstate() == tr._rng.getstate()
