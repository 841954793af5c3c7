"""The frozen prefix of the encoder on the host: finetune.frozen_stage_rules and recipe_rules(freeze_stages=) over CPU flat buffers, the
encoder's frozen_stages attribute and its refusals, the range table in the resume section, and dist.FlatGradReducer's first live segment -- its arithmetic
without a process group, and what two gloo ranks really exchange.  The kernels, the steps and the trainers are tests/test_freeze_stages_gpu.py."""
import functools
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


def encoder():
    from nerf_mae_amd.model import build_model
    torch.manual_seed(0)
    m = build_model("swin_t", resolution=32, compute_dtype=torch.float32)
    m.flatten_parameters(CPU)
    return m


@functools.lru_cache(maxsize=None)
def fcos():
    from nerf_mae_amd.finetune import FlatParameters
    m = C.fcos_model()
    return m, FlatParameters(m, CPU)


def frozen_names(flat, table):
    """the names of the parameters whose range has lr_scale 0, in layout order; every parameter lies in one range"""
    from nerf_mae_amd.trainer import flat_layout
    b, out = table.record["bounds"], []
    for name, (off, numel) in sorted(flat_layout(flat).items(), key=lambda kv: kv[1][0]):
        r = max(i for i in range(len(b) - 1) if b[i] <= off)
        assert off + (numel + 7) // 8 * 8 <= b[r + 1], name
        if table.record["scale"][r][0] == 0.0:
            out.append(name)
    return out


PE = ["patch_partition.0.weight", "patch_partition.0.bias", "patch_partition.2.weight", "patch_partition.2.bias"]
BLOCK = ["norm1.weight", "norm1.bias", "attn.relative_position_bias_table", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
         "norm2.weight", "norm2.bias", "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias"]
MERGE = ["reduction.weight", "norm.weight", "norm.bias"]
DEPTHS = [2, 2, 6, 2]          # swin_t


def stage_names(s):
    """the parameter names of stage s of swin_t, written out by hand: a PatchMerging3D leads every stage but the first, then the blocks"""
    mods = ([MERGE] if s > 0 else []) + [BLOCK] * DEPTHS[s]
    return [f"stages.{s}.{i}.{n}" for i, names in enumerate(mods) for n in names]


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_rules_on_the_mae_encoder_freeze_the_embed_the_mask_token_and_k_stages(k):
    from nerf_mae_amd.finetune import freeze_rules, frozen_stage_rules, param_ranges
    m = encoder()
    t = param_ranges(m, frozen_stage_rules(m, k))
    assert m.frozen_stages == k
    want = ["mask_token"] + PE + [n for s in range(k) for n in stage_names(s)]
    assert frozen_names(m, t) == want
    # the prefix leads the buffer: one frozen range, one live range
    live = m.stages[k] if k < 4 else m.decoder4
    assert t.record["scale"] == [[0.0, 1.0], [1.0, 1.0]] and t.record["bounds"][1] == min(m._offsets[id(p)] for p in live.parameters())
    same = param_ranges(m, freeze_rules(m.patch_partition, "mask_token", *m.stages[:k]))
    assert same.record == t.record


@pytest.mark.parametrize("k", [1, 2, 4])
def test_rules_on_the_fcos_model_have_no_mask_token_and_equal_freeze_over_the_modules(k):
    from nerf_mae_amd.finetune import frozen_stage_rules, param_ranges, recipe_rules
    m, flat = fcos()
    base = m.backbone.base
    try:
        t = param_ranges(flat, frozen_stage_rules(m, k))
        assert base.frozen_stages == k
        want = ["backbone.base." + n for n in PE + [n for s in range(k) for n in stage_names(s)]]
        assert frozen_names(flat, t) == want and not any("mask_token" in n for n in want)
        same = param_ranges(flat, recipe_rules(m, freeze=(base.patch_partition, *base.stages[:k])))
        assert same.record == t.record, "the same table as freeze= over the same modules"
        assert param_ranges(flat, recipe_rules(m, freeze_stages=k)).record == t.record
        assert param_ranges(flat, frozen_stage_rules(flat, k)).record == t.record, "a FlatParameters is taken as well"
    finally:
        base.frozen_stages = 0


def test_composes_with_layer_decay_and_no_decay_and_freeze_wins():
    from nerf_mae_amd.finetune import param_ranges, recipe_rules
    from nerf_mae_amd.trainer import flat_layout
    m, flat = fcos()
    base = m.backbone.base
    try:
        t = param_ranges(flat, recipe_rules(m, layer_decay=0.75, no_decay=True, freeze=("fcos_module.head.cls_logits",), freeze_stages=2))
        b, sc = t.record["bounds"], t.record["scale"]
        s = {}
        for name, (off, _) in flat_layout(flat).items():
            s[name] = tuple(sc[max(i for i in range(len(b) - 1) if b[i] <= off)])
        f32 = lambda x: float(torch.tensor(x, dtype=torch.float32))  # noqa: E731
        # the prefix: lr 0 although layer decay states a scale for it (freeze comes first); the no-decay set still decides the weight decay scale
        assert s["backbone.base.patch_partition.0.weight"] == (0.0, 1.0) and s["backbone.base.patch_partition.0.bias"] == (0.0, 0.0)
        assert s["backbone.base.stages.1.1.mlp.0.weight"] == (0.0, 1.0) and s["backbone.base.stages.1.0.norm.weight"] == (0.0, 0.0)
        # behind it: layer decay (12 blocks: block 5 is stage 2's first) and the no-decay set as without a prefix
        assert s["backbone.base.stages.2.1.norm1.weight"] == (f32(0.75 ** (13 - 5)), 0.0) and s["backbone.base.stages.3.2.mlp.0.weight"] == (f32(0.75), 1.0)
        assert s["fcos_module.head.cls_logits.weight"] == (0.0, 1.0) and s["backbone.fpn_neck.lateral_convs.0.weight"] == (1.0, 1.0)
        again = param_ranges(flat, recipe_rules(m, layer_decay=0.75, no_decay=True,
                                                freeze=("fcos_module.head.cls_logits", base.patch_partition, *base.stages[:2])))
        assert again.record == t.record
    finally:
        base.frozen_stages = 0


def test_the_attribute_and_its_refusals():
    from torch import nn
    from nerf_mae_amd.finetune import frozen_stage_rules, recipe_rules
    m = encoder()
    assert m.frozen_stages == 0
    assert frozen_stage_rules(m, 0) == [] and m.frozen_stages == 0 and recipe_rules(m) == []
    for bad in (-1, 5, 1.5, True, "2"):
        with pytest.raises(ValueError, match="from 0 .* to 4"):
            m.frozen_stages = bad
        assert m.frozen_stages == 0
    for bad in (-1, 5):
        with pytest.raises(ValueError, match="frozen_stages"):
            frozen_stage_rules(m, bad)
        with pytest.raises(ValueError, match="frozen_stages"):
            recipe_rules(m, freeze_stages=bad)
    m.frozen_stages = 4
    assert m.frozen_stages == 4
    with pytest.raises(ValueError, match="exactly one"):
        frozen_stage_rules(nn.Linear(3, 3), 1)
    # the MAE pre-training path refuses a prefix instead of training something untested
    from nerf_mae_amd.dist import GradReducer
    from nerf_mae_amd.trainer import FusedAdamW, GraphedTrainStep, Trainer
    m.frozen_stages = 1
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        GradReducer(m)
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        GraphedTrainStep(m, FusedAdamW(m), 1)
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        Trainer(m, [None])
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        m([torch.zeros(4, 32, 32, 32)])
    m.frozen_stages = 0
    GradReducer(m)


def test_a_resume_under_another_k_is_refused_by_the_range_table(tmp_path):
    from nerf_mae_amd.finetune import param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW, restore_resume, resume_section
    m, flat = fcos()
    try:
        opt = FusedAdamW(flat, ranges=param_ranges(flat, recipe_rules(m, freeze_stages=1)))
        opt.t = 3
        path = str(tmp_path / "r.pt")
        torch.save({"resume": resume_section(flat, opt, step=3)}, path)
        r = torch.load(path, weights_only=True)["resume"]
        restore_resume(r, flat, FusedAdamW(flat, ranges=param_ranges(flat, recipe_rules(m, freeze_stages=1))), "test")
        for other in (FusedAdamW(flat, ranges=param_ranges(flat, recipe_rules(m, freeze_stages=2))), FusedAdamW(flat)):
            with pytest.raises(RuntimeError, match="range"):
                restore_resume(r, flat, other, "test")
    finally:
        m.backbone.base.frozen_stages = 0


# ---- the reducer ---------------------------------------------------------------------------------------------------------------------------------
def test_first_live_segment_follows_the_attribute_when_it_is_read():
    from nerf_mae_amd.dist import FlatGradReducer
    m, flat = fcos()
    base = m.backbone.base
    red = FlatGradReducer(flat)                    # built before any k is set
    assert red.nchunks == 3 and red.nseg == 8
    try:
        for k in range(5):
            base.frozen_stages = k
            live = red.first_live_segment()
            assert live == (0 if k == 0 else red.seg_stage(k) if k < 4 else red.seg_tail()), k
            assert live == [0, 2, 3, 6, 7][k]
            if 0 < k < 4:                          # the bound is where stage k's parameters begin: everything below belongs to the prefix
                assert red.bounds[live] == min(flat._offsets[id(p)] for p in base.stages[k].parameters())
            if k == 4:
                assert red.bounds[live] == base._flat.numel()
    finally:
        base.frozen_stages = 0
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.fpn import FPN
    assert FlatGradReducer(FlatParameters(FPN([32, 32], 32, 2, compute_dtype=torch.float32), CPU)).first_live_segment() == 0


def _formula(n, rank):
    i = torch.arange(n, dtype=torch.float32)
    return torch.sin(0.01 * i + rank) * (rank + 1) + 1e-3 * (i % 977) * (1 - 2 * rank)


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from nerf_mae_amd.dist import FlatGradReducer
        from nerf_mae_amd.finetune import FlatParameters
        m = C.fcos_model()
        flat = FlatParameters(m, CPU)
        red = FlatGradReducer(flat)
        base, n = flat.base, flat._flat_grad.numel()
        base.frozen_stages = 2                     # after the reducer was built
        bound = red.bounds[red.first_live_segment()]
        assert red.active and 0 < bound < n and bound == min(flat._offsets[id(p)] for p in base.stages[2].parameters())
        calls, exchange = [], red._exchange

        def recording(lo, hi):
            calls.append((lo, hi))
            exchange(lo, hi)
        red._exchange = recording
        mine = _formula(n, rank)
        flat._flat_grad.copy_(mine)
        red.launch(red.seg_stage(3))               # as a trigger would: the synchronous CPU path exchanges at once
        red.finish()
        assert calls and min(lo for lo, _ in calls) == bound, "nothing below the bound is exchanged"
        spans = sorted(calls)
        assert spans[0][0] == bound and spans[-1][1] == n and all(a[1] == b[0] for a, b in zip(spans, spans[1:])), spans   # the union is [bound, n), once each
        assert torch.equal(flat._flat_grad[:bound], mine[:bound]), "the prefix's ranges are left alone"
        assert torch.equal(flat._flat_grad[bound:], ((_formula(n, 0) + _formula(n, 1)) / 2)[bound:])
        assert red.pending == []
        q.put((rank, "ok"))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc()))
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_exchange_nothing_below_the_first_live_segment():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 20300 + (os.getpid() % 2000)          # apart from the other host files (22500 .., 29500 ..) and the GPU files
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
