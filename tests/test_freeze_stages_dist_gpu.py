"""Data-parallel fine-tuning under a frozen prefix of the encoder on ONE GPU, in the patterns of tests/test_finetune_dist_gpu.py: the triggers
and the comm stream over a one-rank RCCL group (NMH_DP_FORCE=1), and two ranks on one device over gloo, whose exchange is the single message of finish().

  forced one rank   the triggers of the live segments fire once each and in backward order, none fires for the prefix, finish() issues nothing below the bound
                    (recorded through allreduce_range); the parameters after two steps stay within 4 relerr(B, B') of the step without a reducer
  two gloo ranks    both ranks end with bit-equal parameters; the one message starts at the bound; the parameters match the one-process run on both scenes
                    by that file's yardstick, relerr over the whole buffer <= 1e-5 + 4 relerr(S, S')"""
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests._metrics import relerr  # noqa: E402
from tests.test_finetune_dist_gpu import CLIP, EPS, LR, WD, _answers, _init, _print, _spawn, fcos_model, per_tensor, scenes_on_gpu  # noqa: E402

pytestmark = pytest.mark.gpu
K = 2


def _build(world_size, seed, reducer, comm=None):
    """the FCOS model with freeze_stages=K -> (model, flat, reducer or None, optimizer, step); the reducer is built BEFORE the prefix is set"""
    from nerf_mae_amd.dist import FlatGradReducer
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for, param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW
    m = fcos_model(world_size=world_size, seed=seed)
    flat = FlatParameters(m, torch.device("cuda"))
    red = FlatGradReducer(flat) if reducer else None
    opt = FusedAdamW(flat, lr=LR, weight_decay=WD, max_grad_norm=CLIP, eps=EPS, ranges=param_ranges(flat, recipe_rules(m, freeze_stages=K)))
    assert flat.base.frozen_stages == K
    return m, flat, red, opt, FinetuneStep(flat, opt, loss_fn_for(m), reducer=red)


def _forced_worker(port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NMH_DP_FORCE="1")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from nerf_mae_amd.trainer import flat_layout
        meshes, targets = scenes_on_gpu()
        finals, launched, ranges = [], None, None
        for forced in (False, False, True):          # B, B', then the step with the reducer
            m, flat, red, opt, step = _build(1, 0, forced)
            if forced:
                assert red.active and red.world == 1 and red.comm_stream is not None and flat.base._reducer is red
                launched, launch, ranges, rng = [], red.launch, [], red.allreduce_range
                red.launch = lambda seg: (launched.append(seg), launch(seg))[1]
                red.allreduce_range = lambda lo, hi, overlap=True: (ranges.append((lo, hi)), rng(lo, hi, overlap))[1]
            for _ in range(2):
                step(meshes, targets)
            torch.cuda.synchronize()
            finals.append(flat._flat.detach().cpu().clone())
            layout = flat_layout(flat)
        live, nseg = red.first_live_segment(), red.nseg
        assert live == red.seg_stage(K) == 3 and nseg == 8
        bound = red.bounds[live]
        assert bound == min(flat._offsets[id(p)] for p in flat.base.stages[K].parameters())
        # the triggers of the live segments in backward order, once each, every step; nothing for embed, stage 0, stage 1, and finish() has nothing left to launch
        assert launched == list(range(nseg - 1, live - 1, -1)) * 2, launched
        per_step = [(red.bounds[s], red.bounds[s + 1]) for s in range(nseg - 1, live - 1, -1)]
        assert ranges == per_step * 2 and min(lo for lo, _ in ranges) == bound, ranges
        assert not flat._flat_grad[:bound].any(), "the prefix's gradient ranges are never written"
        q.put((0, "ok", {"err": per_tensor(layout, finals[2], finals[0]), "spread": per_tensor(layout, finals[1], finals[0])}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((0, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_forced_one_rank_reducer_skips_the_prefix_and_leaves_the_step_as_it_is():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_forced_worker, args=(21100 + (os.getpid() % 2000), q))
    p.start()
    _, msg, ans = _answers(q, [p], 600)[0]
    p.join(60)
    assert msg == "ok", msg
    _print(f"  [forced one-rank reducer, freeze_stages={K}] parameters relerr(forced, B) {ans['err']:.2e}  relerr(B, B') {ans['spread']:.2e}  bound {4 * ans['spread']:.2e}")
    assert ans["err"] <= 4 * ans["spread"], (ans["err"], ans["spread"])


def _step_worker(rank, world, port, out_dir, q):
    _init(rank, world, port)
    try:
        from nerf_mae_amd.dist import broadcast_flat_parameters
        m, flat, red, opt, step = _build(world, rank, True)          # another initialisation on rank 1: the broadcast equalises it
        broadcast_flat_parameters(flat)
        assert red.active and red.world == 2 and flat.base._reducer is red
        bound = red.bounds[red.first_live_segment()]
        messages, exchange = [], red._exchange
        red._exchange = lambda lo, hi: (messages.append((lo, hi)), exchange(lo, hi))[1]
        meshes, targets = scenes_on_gpu()
        for _ in range(2):
            step([meshes[rank]], [targets[rank]])
        torch.cuda.synchronize()
        n = flat._flat_grad.numel()
        assert messages == [(bound, n)] * 2 and 0 < bound < n, (messages, bound, n)          # device tensors over gloo: one message per step, from the bound on
        final = flat._flat.detach().cpu()
        both = [torch.empty_like(final) for _ in range(world)]
        dist.all_gather(both, final)
        assert torch.equal(both[0], both[1]), (both[0] - both[1]).abs().max()
        if rank == 0:
            torch.save({"final": final}, os.path.join(out_dir, "rank0.pt"))
        q.put((rank, "ok", bound))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_two_ranks_one_gpu_match_one_process_under_a_frozen_prefix(tmp_path):
    """S, S': one process, both scenes as one batch, two steps without a reducer, twice.  Two ranks, one scene each: relerr over the whole flat buffer
    <= 1e-5 + 4 relerr(S, S') (fp32 buckets), the yardstick of tests/test_finetune_dist_gpu.py::test_two_ranks_one_gpu_match_one_process_on_both_scenes."""
    meshes, targets = scenes_on_gpu()
    runs = []
    for _ in range(2):
        m, flat, _, opt, step = _build(1, 0, False)
        for _ in range(2):
            step(meshes, targets)
        torch.cuda.synchronize()
        runs.append(flat._flat.detach().cpu().clone())
        del m, flat, opt, step
    port = 23100 + (os.getpid() % 2000)
    _spawn(_step_worker, lambda r: (r, 2, port, str(tmp_path)))
    final = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)["final"]
    err, spread = relerr(final, runs[0]), relerr(runs[1], runs[0])
    _print(f"  [two ranks, freeze_stages={K}] parameters after two steps relerr {err:.2e}  relerr(S, S') {spread:.2e}  bound {1e-5 + 4 * spread:.2e}")
    assert err <= 1e-5 + 4 * spread, (err, spread)
