"""Data-parallel fine-tuning on the host: the segment table of dist.FlatGradReducer over the three model kinds of tests/_finetune_common.py, its exchange over
gloo with two ranks (a base-less module: one segment), and trainer.dp_epoch_plan, the batching arithmetic of DetectionTrainer.  The triggers, the step and the
trainer on two ranks are tests/test_finetune_dist_gpu.py."""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402

CPU = torch.device("cpu")


@pytest.mark.parametrize("which", ("fcos", "rpn", "semantics"))
def test_segment_table(which):
    from nerf_mae_amd.dist import FlatGradReducer
    from nerf_mae_amd.finetune import FlatParameters
    m = {"fcos": C.fcos_model, "rpn": C.rpn_model, "semantics": C.semantics_model}[which]()
    flat = FlatParameters(m, CPU)
    red = FlatGradReducer(flat)
    base, b, off = flat.base, red.bounds, flat._offsets
    nblocks = sum(1 for mod in base.stages[2] if hasattr(mod, "attn"))
    assert red.chunk_stage == 2 and red.nchunks == len(red.chunk_groups) == min(3, nblocks)
    assert red.nseg == len(b) - 1 == 5 + red.nchunks                      # embed, stage 0, stage 1, the groups of stage 2, stage 3, tail
    assert b[0] == 0 and b[-1] == flat._flat_grad.numel()
    assert all(x < y for x, y in zip(b, b[1:])), b
    assert all(x % 8 == 0 for x in b), b

    def seg_of(p):
        lo, hi = off[id(p)], off[id(p)] + p.numel()
        hits = [s for s in range(red.nseg) if b[s] <= lo and hi <= b[s + 1]]
        assert len(hits) == 1, (lo, hi, b)
        return hits[0]

    placed = {id(p): seg_of(p) for _, p in C.trainable(m)}
    assert len(placed) == len(off)
    # the embed range, the stages (stage 2 by block group), the tail
    assert {placed[id(p)] for p in base.patch_partition.parameters()} == {0}
    in_encoder = {id(p) for p in base.patch_partition.parameters()}
    for s in range(4):
        groups = red.chunk_groups if s == red.chunk_stage else [list(base.stages[s])]
        assert sum(len(g) for g in groups) == len(base.stages[s])
        for k, grp in enumerate(groups):
            ps = [p for mod in grp for p in mod.parameters()]
            assert ps and {placed[id(p)] for p in ps} == {red.seg_stage(s, k)}, (s, k)
            in_encoder.update(id(p) for p in ps)
    assert [red.seg_stage(0), red.seg_stage(1), red.seg_stage(2, 0), red.seg_stage(3), red.seg_tail()] == [1, 2, 3, 3 + red.nchunks, red.nseg - 1]
    outside = [p for _, p in C.trainable(m) if id(p) not in in_encoder]
    assert outside and {placed[id(p)] for p in outside} == {red.seg_tail()}
    assert sum(1 for v in placed.values() if v == red.seg_tail()) == len(outside), "the tail holds nothing of the encoder"
    if which == "semantics":     # the base keeps decoder4..2 behind stage 3: they open the tail
        assert b[red.seg_tail()] == off[id(next(base.decoder4.parameters()))] < base._flat.numel()
    else:                        # the FPN backbone's base ends with stage 3
        assert b[red.seg_tail()] == base._flat.numel()
    from nerf_mae_amd.dist import GradReducer
    assert not hasattr(GradReducer, "seg_tail"), "the FPN backbone tells the two reducers apart by seg_tail"


def _small_fpn():
    from nerf_mae_amd.fpn import FPN
    torch.manual_seed(3)
    return FPN([32, 32], 32, 2, compute_dtype=torch.float32)


def _formula(n, rank):
    i = torch.arange(n, dtype=torch.float32)
    return torch.sin(0.01 * i + rank) * (rank + 1) + 1e-3 * i * (1 - 2 * rank)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nerf_mae_amd.dist import FlatGradReducer, broadcast_flat_parameters
        from nerf_mae_amd.finetune import FlatParameters
        m = _small_fpn()
        with torch.no_grad():
            for p in m.parameters():
                p.add_(rank)                      # different parameters per rank: the broadcast must equalise them
        flat = FlatParameters(m, CPU)
        broadcast_flat_parameters(flat)
        ref = flat._flat.clone()
        dist.broadcast(ref, src=0)
        assert torch.equal(ref, flat._flat)
        red = FlatGradReducer(flat)
        n = flat._flat_grad.numel()
        assert flat.base is None and red.active and red.nseg == 1 and red.bounds == [0, n] and red.seg_tail() == 0 and red.chunk_stage == -1
        flat._flat_grad.copy_(_formula(n, rank))
        red.finish()
        assert torch.equal(flat._flat_grad, (_formula(n, 0) + _formula(n, 1)) / 2)
        assert red.pending == []
        flat.check()
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_flat_grad_reducer_gloo_world2():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 22500 + (os.getpid() % 2000)          # apart from tests/test_dist_cpu.py (29500 ..) and the GPU files
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=300) for _ in procs]
    except Exception:
        for p in procs:
            p.terminate()
        raise
    for p in procs:
        p.join(60)
    for rank, msg in res:
        assert msg == "ok", f"rank {rank}: {msg}"


@pytest.mark.parametrize("n,batch,world", [(4, 1, 2), (5, 2, 2), (7, 2, 3), (3, 2, 1), (9, 4, 8), (1, 1, 2)])
def test_dp_epoch_plan_gives_every_rank_the_same_steps(n, batch, world):
    from nerf_mae_amd.trainer import dp_epoch_plan
    for epoch in (1, 2):
        plans = [dp_epoch_plan(n, batch, r, world, epoch, seed=5) for r in range(world)]
        sizes = [[len(ids) for ids in pl] for pl in plans]
        assert all(s == sizes[0] for s in sizes), sizes
        per_rank = -(-n // world)
        assert len(sizes[0]) == -(-per_rank // batch) and sum(sizes[0]) == per_rank and all(0 < k <= batch for k in sizes[0])
        assert {i for pl in plans for ids in pl for i in ids} == set(range(n)), "the union over the ranks covers every scene"
    assert dp_epoch_plan(n, batch, 0, world, 1, seed=5) != dp_epoch_plan(n, batch, 0, world, 2, seed=5) or n == 1


def test_dp_epoch_plan_world_one_is_the_single_process_slicing():
    """what DetectionTrainer.train_epoch did before it knew ranks: shard_indices(n, 0, 1, epoch, seed) cut into ceil(n / batch) slices"""
    from nerf_mae_amd.dist import shard_indices
    from nerf_mae_amd.trainer import dp_epoch_plan
    for n, batch, epoch, seed in ((3, 2, 1, 0), (8, 3, 4, 7), (5, 5, 2, 1), (2, 4, 1, 0)):
        idx = shard_indices(n, 0, 1, epoch, seed=seed)
        steps = -(-n // batch)
        assert dp_epoch_plan(n, batch, 0, 1, epoch, seed) == [idx[b * batch:(b + 1) * batch] for b in range(steps)]


def test_dp_epoch_plan_refuses_an_empty_shard():
    from nerf_mae_amd.trainer import dp_epoch_plan
    with pytest.raises(ValueError, match="empty"):
        dp_epoch_plan(0, 2, 0, 2, 1, 0)
    with pytest.raises(ValueError):
        dp_epoch_plan(4, 0, 0, 2, 1, 0)
