"""Gradient accumulation in the fine-tuning epoch loop (_FinetuneTrainer, here as RPNTrainer with a frozen backbone, the cheapest of the
four): three scenes, batch 1, accumulate = 2 -> two optimizer steps per epoch, the second of one micro-batch.  The step's arithmetic is
tests/test_accumulate_gpu.py::test_finetune_step_accumulates_and_steps_on_the_mean; this is the bookkeeping around it."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _det_trainers_common as D  # noqa: E402

pytestmark = pytest.mark.gpu


def _trainer(accumulate, **kw):
    from nerf_mae_amd.trainer import RPNTrainer
    m = D.rpn_model(stochastic_depth=False).cuda().train()
    return RPNTrainer(m, D.scenes(D.TRAIN), D.boxes(D.TRAIN), batch_size=1, num_epochs=2, lr=1e-3, weight_decay=1e-3, freeze_backbone=True, log=lambda s: None,
                      accumulate=accumulate, **kw)


def test_finetune_trainer_counts_optimizer_steps_and_logs_the_mean_of_step_means(tmp_path):
    from nerf_mae_amd.trainer import RPNTrainer
    assert len(D.TRAIN) == 3
    tr = _trainer(2, save_path=str(tmp_path))
    assert tr.micro_per_epoch == 3 and tr.steps_per_epoch == 2 and tr.sched.total == 4
    assert tr.args["accumulate"] == 2 and tr.args["batch_size"] == 2
    logged, inner, t_at_call = [], tr._logged, []
    tr._logged = lambda losses: (logged.append(inner(losses).clone()), t_at_call.append(tr.opt.t), logged[-1])[2]
    before = tr.flat._flat.detach().clone()
    rec = tr.train_epoch(1)
    torch.cuda.synchronize()
    assert tr.global_step == 2 and tr.opt.t == 2 and len(logged) == 3
    assert t_at_call == [0, 1, 2], "the first micro-batch is logged before any update, the other two after the step they close"
    assert tr.opt.grad_scale == 1.0, "the epoch's last step had one micro-batch"
    assert not torch.equal(before, tr.flat._flat) and not tr.flat._flat_grad.any()
    want = (((logged[0] + logged[1]) / 2 + logged[2]) / 2).tolist()
    for k, w in zip(RPNTrainer.KEYS, want):
        assert rec[k] == pytest.approx(w, rel=1e-6), (k, rec[k], w)
    # a file of this run: refused under another k, continued under the same at an optimizer-step boundary, the sampler's counter in micro-steps
    tr._save("epoch_1.pt", 1)
    path = str(tmp_path / "epoch_1.pt")
    with pytest.raises(RuntimeError, match="accumulate"):
        _trainer(1).resume(path)
    tr2 = _trainer(2)
    ck = tr2.resume(path)
    assert ck["resume"]["accumulate"] == 2 and tr2.start_epoch == 2 and tr2.global_step == 2 and tr2.opt.t == 2
    assert tr2.model.rpn.loss.rng_state.tolist() == [tr2.model.rpn.loss.seed, 3]
    assert torch.equal(tr2.flat._flat, tr.flat._flat)


def test_finetune_trainer_without_accumulation_is_unchanged():
    tr = _trainer(1)
    assert tr.micro_per_epoch == tr.steps_per_epoch == 3 and tr.sched.total == 6 and tr.args["accumulate"] == 1 and tr.args["batch_size"] == 1
    tr.train_epoch(1)
    torch.cuda.synchronize()
    assert tr.global_step == 3 and tr.opt.t == 3 and tr.opt.mean_clip is False
