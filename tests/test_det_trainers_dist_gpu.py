"""RPNTrainer(freeze_backbone=True) on two ranks: the reducer covers one range, the head's, and the initial broadcast still sends the frozen
backbone.  RCCL refuses two ranks on one device, so two ranks share the GPU over gloo, with the child-process pattern of tests/test_finetune_dist_gpu.py
(tests/_voxel_common.spawn: fresh spawned children, one answer per child, a timeout or a dead child terminates both and fails, no retry)."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _det_trainers_common as D  # noqa: E402
from tests._voxel_common import init_gloo, spawn  # noqa: E402

pytestmark = pytest.mark.gpu
TRAIN_KEYS = ["epoch", "train_loss", "loss_objectness", "loss_rpn_box_reg", "loss_rpn_box_reg_2d"]


def _worker(rank, world, port, out_dir, q):
    import torch.distributed as dist
    init_gloo(rank, world, port)
    try:
        from nerf_mae_amd.trainer import RPNTrainer
        m = D.rpn_model(seed=rank).cuda().train()          # another initialisation on rank 1, backbone included: the broadcast must equalise it
        lines = []
        tr = RPNTrainer(m, D.scenes((11, 12, 13, 14)), D.boxes((11, 12, 13, 14)), D.scenes(D.VAL), D.boxes(D.VAL), batch_size=1, num_epochs=1, lr=1e-3,
                        weight_decay=1e-3, freeze_backbone=True, save_path=os.path.join(out_dir, f"rank{rank}"), flip_prob=0.5, rotate_prob=0.5, log=lines.append,
                        rank=rank, world=world)
        assert tr.steps_per_epoch == 2 and tr.args["batch_size"] == 2 and tr.reducer is not None and tr.reducer.active
        assert tr.flat.base is None and tr.reducer.nseg == 1 and tr.reducer.bounds == [0, tr.flat._flat.numel()], "one range: the head's"
        hist = tr.fit()
        torch.cuda.synchronize()
        assert tr.global_step == 2 and len(lines) == (1 if rank == 0 else 0)
        final = tr.flat._flat.detach().cpu()
        frozen = torch.cat([t.detach().reshape(-1).float().cpu() for t in list(m.backbone.parameters()) + list(m.backbone.buffers())])
        for name, mine in (("flat buffer", final), ("frozen backbone", frozen)):
            both = [torch.empty_like(mine) for _ in range(world)]
            dist.all_gather(both, mine)
            assert torch.equal(both[0], both[1]), (name, (both[0] - both[1]).abs().max())
        tr.flat.check()
        q.put((rank, "ok", hist))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_rpn_trainer_with_a_frozen_backbone_on_two_ranks(tmp_path):
    """four scenes, per-rank batch 1, one epoch with evaluation: both ranks end with bit-equal flat buffers and bit-equal frozen backbones (asserted in the
    children, rank 1 having been seeded differently), only rank 0 evaluates and writes, both report the same training losses, and nobody hangs"""
    port = 25300 + (os.getpid() % 2000)
    hist = spawn(_worker, lambda r: (r, 2, port, str(tmp_path)))
    assert [list(h) for h in hist[1]] == [TRAIN_KEYS]
    h0, h1 = hist[0][0], hist[1][0]
    for k in ("ap_25", "ap_50", "recall_25_top_1000", "recall_50_top_1000", "recall_ar_top_1000"):
        assert k in h0 and h0[k] == h0[k], (k, h0)
    assert all(h0[k] == h1[k] for k in TRAIN_KEYS), (h0, h1)
    assert h0["loss_rpn_box_reg"] > 0 and h0["train_loss"] == h0["train_loss"]
    assert sorted(os.listdir(tmp_path / "rank0")) == ["epoch_1.pt", "model_best.pt"]
    assert not os.path.exists(tmp_path / "rank1") or not os.listdir(tmp_path / "rank1")
