"""The frozen prefix of the encoder on the GPU: freeze_stages=k against the parent's path, freeze= over the same modules, on the common small
models of tests/_finetune_common.py (resolution 32, swin_t, 64 FPN channels, token grids 8^3 / 4^3 / 2^3 / 1^3: stage 1 is exactly one window, stage 2 is padded).

  A   freeze_stages=k: the prefix runs without a graph, the backward ends at stage k
  B   freeze=(patch_partition, *stages[:k]): the same range table, the whole backward; B' is B again (the parent path's own run-to-run spread)

  equivalence   three FinetuneSteps, fp32 and bf16 compute, k = 1 and 2: relerr(A, B) <= 3e-5 + 4 relerr(B, B') over all parameters and over each step's three
                losses; the boundary is a leaf that requires a gradient, so the first live block's BlockPlan is B's and the buffers are compared bit for bit
                as well wherever B' reproduces B bit for bit; the frozen ranges of the parameters and of both moments stay bit-unchanged
  no backward   the prefix's gradient ranges are exactly zero under A (and not under B), and the LayerNorm backward -- which _BlockFn.backward, _MergeFn.backward
                and _EmbedFn.backward each call on their own norm -- ran once per live block / merge and never for the prefix; k = 4: no encoder backward
  the queue     bf16 + the grouped weight-gradient queue: every live parameter gets its gradient, once
  memory        the peak over one forward + backward is strictly lower
  the others    the RPN and the voxel-semantics model (frozen skips into the decoders) descend; DetectionTrainer(freeze_stages=1) with a true resume;
                accumulate=2
  refusals      and k = 0 launch for launch the path of before

relerr over a set of tensors is the largest per-tensor value, as tests/test_finetune_gpu.py defines it; the stochastic-depth draws are ON (the prefix keeps its
mode) and seeded per step."""
import functools
import inspect
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402
from tests._metrics import relerr  # noqa: E402
from tests.test_finetune_gpu import CLIP, EPS, KEYS, LR, STEP_BOUND, WD, batches, fused_steps, params_of, worst  # noqa: E402

pytestmark = pytest.mark.gpu
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


def _print(*a):
    if os.environ.get("NMH_PRINT_ERR"):
        print(*a)


@functools.lru_cache(maxsize=None)
def weights(dt):
    return {k: v.clone() for k, v in _fcos(dt).state_dict().items()}


def _fcos(dt):
    from nerf_mae_amd.fcos import FCOSOverNeRF
    torch.manual_seed(0)
    return FCOSOverNeRF(C.fcos_args(DTYPES[dt]), C.backbone(DTYPES[dt]), list(C.STRIDES), resolution=C.R)


def fcos_on_gpu(dt="fp32"):
    """stochastic depth stays on: the prefix keeps its mode, and A and B take their factors from the same seeded draw"""
    m = _fcos(dt)
    m.load_state_dict(weights(dt), strict=True)
    return m.cuda().train()


def encoder_of(model):
    from nerf_mae_amd.finetune import _encoder_of
    return _encoder_of(model, "test")


def prefix_modules(model, k):
    base = encoder_of(model)
    return (base.patch_partition, *base.stages[:k])


def setup(model, k, how, accumulate=1, eps=EPS, lr=LR):
    """how = "A": freeze_stages=k; "B": freeze= over the same modules (the parent's path) -> (flat, opt, step)"""
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for, param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW
    flat = FlatParameters(model, torch.device("cuda"))
    rules = recipe_rules(model, freeze_stages=k) if how == "A" else recipe_rules(model, freeze=prefix_modules(model, k))
    assert encoder_of(model).frozen_stages == (k if how == "A" else 0)
    opt = FusedAdamW(flat, lr=lr, weight_decay=WD, eps=eps, max_grad_norm=CLIP, ranges=param_ranges(flat, rules) if rules else None, accumulate=accumulate)
    return flat, opt, FinetuneStep(flat, opt, loss_fn_for(model))


def prefix_end(flat, k):
    """the first element of the flat buffers behind the prefix: where stage k's parameters begin, or the end of the encoder's stages"""
    base = flat.base
    if k < len(base.stages):
        return min(flat._offsets[id(p)] for p in base.stages[k].parameters())
    return max((flat._offsets[id(p)] + p.numel() + 7) // 8 * 8 for p in base.stages[-1].parameters())


def start_moments(opt):
    """non-zero moments everywhere, the same in every run: a frozen range that was stepped would show"""
    i = torch.arange(opt.m.numel(), device=opt.m.device, dtype=torch.float32)
    opt.m.copy_(1e-3 * torch.sin(0.37 * i))
    opt.v.copy_(1e-6 * (1.0 + torch.cos(0.11 * i)))
    return opt.m.clone(), opt.v.clone()


@functools.lru_cache(maxsize=None)
def three_runs(k, dt):
    """A, B, B': three steps each.  Computed once per (k, compute dtype), left unchanged."""
    out = {}
    for name, how in (("A", "A"), ("B", "B"), ("B2", "B")):
        m = fcos_on_gpu(dt)
        before = params_of(m)
        flat, opt, step = setup(m, k, how)
        m0, v0 = start_moments(opt)
        start = flat._flat.clone()
        losses, norms = fused_steps(step, opt, (0, 1, 2))
        torch.cuda.synchronize()
        out[name] = dict(params=params_of(m), losses=losses, norms=[float(n) for n in norms], flat=flat._flat.clone(), m=opt.m.clone(), v=opt.v.clone(),
                         start=start, m0=m0, v0=v0, end=prefix_end(flat, k), before=before, table=opt.range_record)
        del m, flat, opt, step
    return out


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("k", [1, 2])
def test_three_steps_match_freeze_over_the_same_modules(k, dt):
    """relerr(A, B) <= 3e-5 + 4 relerr(B, B') over all parameters and over each step's three losses (the bound of test_finetune_step_matches_the_stock_optimizer_path,
    B being unchanged code).  The boundary is a leaf that requires a gradient, so the first live block plans as under B and runs B's kernels on B's operands: where
    B' reproduces B bit for bit -- otherwise bit equality is not defined for the parent's path itself -- A's buffers equal B's bit for bit too, and the first
    step's losses (before any update) are compared bit for bit under the same condition.  Measured on an MI355X, parameters relerr(A, B) / relerr(B, B'): k=1 fp32
    1.13e-7 / 1.13e-7, k=1 bf16 5.73e-8 / 1.15e-7, k=2 fp32 5.74e-8 / 5.71e-8, k=2 bf16 1.15e-7 / 5.73e-8; losses and clip norms equal to the last digit.  B' did
    not reproduce B's buffers bit for bit in any of the four cases (the order of fp32 atomic sums), so the buffers' bit equality was never in force there."""
    r = three_runs(k, dt)
    A, B, B2 = r["A"], r["B"], r["B2"]
    assert A["table"] == B["table"], "the same range table"
    spread_p, spread_l = worst(B2["params"], B["params"]), max(relerr(x, y) for x, y in zip(B2["losses"], B["losses"]))
    err_p, err_l = worst(A["params"], B["params"]), max(relerr(x, y) for x, y in zip(A["losses"], B["losses"]))
    bound_p, bound_l = 3 * STEP_BOUND + 4 * spread_p, 3 * STEP_BOUND + 4 * spread_l
    moved = worst({n: t for n, t in A["before"].items()}, A["params"])
    reproducible = torch.equal(B2["flat"], B["flat"]) and torch.equal(B2["m"], B["m"]) and torch.equal(B2["v"], B["v"])
    bitwise = torch.equal(A["flat"], B["flat"]) and torch.equal(A["m"], B["m"]) and torch.equal(A["v"], B["v"])
    _print(f"  [freeze_stages={k} {dt}] parameters relerr(A,B) {err_p:.2e}  relerr(B,B') {spread_p:.2e}  bound {bound_p:.2e}  moved {moved:.2e}")
    _print(f"  [freeze_stages={k} {dt}] losses     relerr(A,B) {err_l:.2e}  relerr(B,B') {spread_l:.2e}  bound {bound_l:.2e}  grad norms {A['norms']} / {B['norms']}")
    _print(f"  [freeze_stages={k} {dt}] B' == B bit for bit: {reproducible}; A == B bit for bit: {bitwise}")
    assert all(torch.isfinite(l).all() for l in A["losses"]) and A["losses"][0][1].item() > 0
    assert err_p <= bound_p, (err_p, bound_p)
    assert err_l <= bound_l, (err_l, bound_l)
    assert max(A["norms"]) > CLIP and moved >= 100 * bound_p, (A["norms"], moved)
    if reproducible:
        assert bitwise, "the leaf route runs B's kernels on B's operands: the buffers must be B's bit for bit"
    if torch.equal(B2["losses"][0], B["losses"][0]):          # the first forward pass, before any update: the prefix without a graph computes the same bits
        assert torch.equal(A["losses"][0], B["losses"][0]), (A["losses"][0], B["losses"][0])
    # the frozen ranges: parameters and both moments bit-unchanged, under A and under B
    for run in (A, B):
        e = run["end"]
        assert e > 0 and torch.equal(run["flat"][:e], run["start"][:e]) and torch.equal(run["m"][:e], run["m0"][:e]) and torch.equal(run["v"][:e], run["v0"][:e])
        assert not torch.equal(run["flat"][e:], run["start"][e:]) and not torch.equal(run["m"][e:], run["m0"][e:])


# ---- no backward work for the prefix -------------------------------------------------------------------------------------------------------------
def record_norm_backwards(monkeypatch, model):
    """wraps ops.layernorm_bwd -- _BlockFn.backward calls it on the block's norm1 (every plan), _MergeFn.backward on the merging's norm, _EmbedFn.backward on the
    patch embed's LayerNorm -- and the two attention backward kernels -> the list that fills with the names of the modules whose backward ran"""
    from nerf_mae_amd import ops
    base = encoder_of(model)
    owner = {}
    for name, mod in base.named_modules():
        for attr in ("norm1", "norm"):
            if hasattr(mod, attr) and isinstance(getattr(mod, attr), torch.nn.LayerNorm):
                owner[getattr(mod, attr).weight.data_ptr()] = name
    owner[base.patch_partition[2].weight.data_ptr()] = "patch_partition"
    calls = []
    ln, wa, wat = ops.layernorm_bwd, ops.window_attn_bwd, ops.window_attn_bwd_tokens

    def layernorm_bwd(dy, x, w, *a, **kw):
        if w.data_ptr() in owner:
            calls.append(owner[w.data_ptr()])
        return ln(dy, x, w, *a, **kw)

    def attn(fn):
        def wrapped(*a, **kw):
            calls.append("attention")
            return fn(*a, **kw)
        return wrapped
    monkeypatch.setattr(ops, "layernorm_bwd", layernorm_bwd)
    monkeypatch.setattr(ops, "window_attn_bwd", attn(wa))
    monkeypatch.setattr(ops, "window_attn_bwd_tokens", attn(wat))
    return calls


def module_names(base, stages):
    """the names (inside the encoder) of the blocks and mergings of the given stages"""
    return sorted(f"stages.{s}.{i}" for s in stages for i in range(len(base.stages[s])))


@pytest.mark.parametrize("k", [1, 2, 4])
def test_no_backward_kernel_runs_for_the_prefix(k, monkeypatch):
    nonzero = {}          # by parameter name: B's gradient is not all zero (stage 3 runs on one token per sample: some of its gradients vanish under B as well)
    for how in ("B", "A"):
        m = fcos_on_gpu()
        flat, opt, step = setup(m, k, how)       # (the owner table is read after flattening: the parameters live in the flat buffer)
        calls = record_norm_backwards(monkeypatch, m)
        base, e = flat.base, prefix_end(flat, k)
        torch.manual_seed(100)
        losses, total = step.forward(*batches()[0])
        total.backward()
        torch.cuda.synchronize()
        g = flat._flat_grad
        nblocks = lambda stages: sum(hasattr(mod, "attn") for s in stages for mod in base.stages[s])  # noqa: E731
        if how == "A":
            assert not g[:e].any(), "the prefix's gradient ranges are never written"
            assert sorted(c for c in calls if c != "attention") == module_names(base, range(k, 4)), calls
            assert calls.count("attention") == nblocks(range(k, 4))
        else:
            assert g[:e].any(), "the parent's path computes the gradients it then does not step: the two can be told apart"
            assert sorted(c for c in calls if c != "attention") == sorted(module_names(base, range(4)) + ["patch_partition"]), calls
            assert calls.count("attention") == nblocks(range(4))
        if how == "B":
            nonzero = {n: bool(p.grad.any()) for n, p in m.named_parameters() if p.requires_grad}
            assert all(v for n, v in nonzero.items() if n.startswith(("backbone.base.patch_partition", "backbone.base.stages.0.", "backbone.base.stages.1.")))
        for name, p in m.named_parameters():
            if p.requires_grad:
                in_prefix = name.startswith("backbone.base.patch_partition") or (name.startswith("backbone.base.stages.") and int(name.split(".")[3]) < k)
                assert bool(p.grad.any()) == (nonzero[name] and not (how == "A" and in_prefix)), (how, name)
        assert g[e:].any()
        neck = [p for n, p in m.named_parameters() if n.startswith("backbone.fpn_neck.")]
        assert neck and all(p.grad.any() for p in neck) and m.fcos_module.head.cls_logits.weight.grad.any(), "the neck and the head still get their gradients"
        before = flat._flat.clone()
        opt.step()
        torch.cuda.synchronize()
        assert torch.equal(flat._flat[:e], before[:e]) and not torch.equal(flat._flat[e:], before[e:]), "the head still trains, the prefix does not move"
        monkeypatch.undo()
    assert base._wq.pending == [] and base._wq.deferred == []


# ---- the weight-gradient queue ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
def test_the_first_live_stage_flushes_the_weight_gradient_queue(k, monkeypatch):
    """bf16 compute, ops.GROUPED_WGRAD on: the first live stage's input is a leaf, so its _StageFlushFn exists and is the one marked last.  Every live encoder
    parameter has a gradient; a second forward + backward straight after gives the same gradients (nothing stayed queued to be added twice); and against B
    tensor by tensor relerr(g_A, g_B) <= 3e-5 + 4 relerr(g_B, g_B'), the file's one yardstick (B and B': the parent's path twice)."""
    from nerf_mae_amd import model as M, ops
    monkeypatch.setattr(ops, "GROUPED_WGRAD", True)
    lasts, fwd = [], M._StageFlushFn.forward

    def forward(ctx, x, wq, last=False):
        lasts.append(bool(last))
        return fwd(ctx, x, wq, last)
    monkeypatch.setattr(M._StageFlushFn, "forward", staticmethod(forward))

    def grads(how, repeat):
        m = fcos_on_gpu("bf16")
        flat, opt, step = setup(m, k, how)
        out = []
        for _ in range(repeat):
            flat.zero_grad()
            del lasts[:]
            torch.manual_seed(100)
            _, total = step.forward(*batches()[0])
            total.backward()
            torch.cuda.synchronize()
            q = flat.base._wq
            assert q.pending == [] and q.deferred == [] and q.inflight == [] and not q._due, "the queue is empty when the backward pass has returned"
            out.append({n: p.grad.detach().clone() for n, p in m.named_parameters() if p.requires_grad})
        return out, list(lasts), flat

    (a1, a2), lasts_a, flat = grads("A", 2)
    (b1,), lasts_b, _ = grads("B", 1)
    (b2,), _, _ = grads("B", 1)
    # stage k .. 3 have a flush each under A, the first of them is the last of the backward pass; under B all four stages, stage 0's is the last
    assert lasts_a == [True] + [False] * (3 - k) and lasts_b == [True, False, False, False], (lasts_a, lasts_b)
    live = [n for n in a1 if n.startswith("backbone.base.stages.") and int(n.split(".")[3]) >= k]
    dead = [n for n in a1 if n.startswith("backbone.base.") and n not in live]
    vanishing = [n for n in live if not b1[n].any()]          # zero under the parent's path too (stage 3 attends over one token per sample)
    _print(f"  [queue k={k}] live encoder parameters {len(live)}, of them with a zero gradient under B as well: {vanishing}")
    assert live and dead and len(vanishing) < len(live) // 4 and not any(a1[n].any() for n in dead)
    assert all(bool(a1[n].any()) == bool(b1[n].any()) for n in live), "every live parameter has the gradient it has under B"
    rest = [n for n in a1 if n not in dead]
    spread = max(relerr(b2[n], b1[n]) for n in rest)
    again, err = max(relerr(a2[n], a1[n]) for n in rest), max(relerr(a1[n], b1[n]) for n in rest)
    bound = 3 * STEP_BOUND + 4 * spread
    _print(f"  [queue k={k}] gradients relerr(A,B) {err:.2e}  relerr(A,A again) {again:.2e}  relerr(B,B') {spread:.2e}  bound {bound:.2e}")
    assert again <= bound, (again, bound)
    assert err <= bound, (err, bound)


# ---- memory ----------------------------------------------------------------------------------------------------------------------------------------
def test_the_peak_of_forward_and_backward_is_lower():
    """torch.cuda.max_memory_allocated() over one forward + backward at batch 2, k = 2, above what is allocated when the pass begins: A strictly below B (a
    condition, not a measurement: stages 0 and 1 keep no activation for a backward)"""
    peak = {}
    for how in ("A", "B"):
        m = fcos_on_gpu()
        flat, opt, step = setup(m, 2, how)
        for measured in (False, True):          # a first pass fills the packed weights and the allocator's pools
            flat.zero_grad()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base0 = torch.cuda.memory_allocated()
            torch.manual_seed(100)
            _, total = step.forward(*batches()[0])
            total.backward()
            torch.cuda.synchronize()
            peak[how] = torch.cuda.max_memory_allocated() - base0
            del total
        del m, flat, opt, step
    _print(f"  [memory k=2, batch 2] peak over forward + backward: freeze_stages {peak['A'] / 2 ** 20:.1f} MiB, freeze= {peak['B'] / 2 ** 20:.1f} MiB")
    assert peak["A"] < peak["B"], peak


# ---- the other models ------------------------------------------------------------------------------------------------------------------------------
def _descends(model, batch, k, before_forward=None, steps=8):
    """tests/test_finetune_gpu.py::_descends under freeze_stages=k"""
    flat, opt, step = setup(model, k, "A", eps=1e-8, lr=2e-4)
    e, start = prefix_end(flat, k), flat._flat.clone()
    totals = []
    for _ in range(steps):
        torch.manual_seed(7)
        if before_forward is not None:
            before_forward()
        out = step(*batch)
        totals.append(torch.stack(list(out.values())).sum())
    totals = torch.stack(totals).tolist()
    _print(f"  [{type(model).__name__} freeze_stages={k}] totals {['%.5g' % t for t in totals]}")
    assert all(t == t for t in totals) and totals[-1] < totals[0], totals
    assert torch.equal(flat._flat[:e], start[:e]) and not torch.equal(flat._flat[e:], start[e:])
    flat.check()


def test_eight_steps_lower_the_rpn_loss_with_two_frozen_stages():
    m = C.rpn_model().cuda().train()
    meshes, _ = batches()[0]
    targets = [torch.from_numpy(C.aabb_boxes(s)).cuda() for s in (1, 2)]
    state0 = torch.tensor([m.rpn.loss.seed, 0], dtype=torch.int64, device="cuda")

    def same_sample():
        if m.rpn.loss.rng_state is not None:
            m.rpn.loss.rng_state.copy_(state0)

    _descends(m, (meshes, targets), 2, same_sample)


@pytest.mark.parametrize("k", [2, 4])
def test_eight_steps_lower_the_voxel_semantics_loss_with_frozen_skips(k):
    """decoder3 and decoder2 (k = 2), and all of decoder4 .. decoder2 (k = 4), consume skips that require no gradient"""
    m = C.semantics_model().cuda().train()
    meshes, _ = batches()[0]
    _descends(m, (meshes, [C.label_grid(s).cuda() for s in (1, 2)]), k)
    base = m.base
    assert all(p.grad is not None for p in base.decoder4.parameters())


def test_accumulate_two_matches_freeze_over_the_same_modules():
    """accumulate(batch 0) + step(batch 1), k = 1, under the bound of the three-step test"""
    runs = {}
    for name, how in (("A", "A"), ("B", "B"), ("B2", "B")):
        m = fcos_on_gpu()
        flat, opt, step = setup(m, 1, how, accumulate=2)
        torch.manual_seed(100)
        step.accumulate(*batches()[0])
        torch.manual_seed(101)
        out = step(*batches()[1])
        torch.cuda.synchronize()
        runs[name] = (params_of(m), torch.stack([out[key] for key in KEYS]), float(opt.norm))
    spread_p, spread_l = worst(runs["B2"][0], runs["B"][0]), relerr(runs["B2"][1], runs["B"][1])
    err_p, err_l = worst(runs["A"][0], runs["B"][0]), relerr(runs["A"][1], runs["B"][1])
    _print(f"  [accumulate=2 k=1] parameters relerr(A,B) {err_p:.2e}  relerr(B,B') {spread_p:.2e}; losses {err_l:.2e} / {spread_l:.2e}; norms {runs['A'][2]:.6g} {runs['B'][2]:.6g}")
    assert err_p <= 3 * STEP_BOUND + 4 * spread_p, (err_p, spread_p)
    assert err_l <= 3 * STEP_BOUND + 4 * spread_l, (err_l, spread_l)


def _trainer(k=1, seed=0):
    from nerf_mae_amd.trainer import DetectionTrainer
    m = C.fcos_model(seed).cuda().train()
    tr = DetectionTrainer(m, [C.scene(s) for s in (11, 12)], [C.obb_boxes(s) for s in (11, 12)], batch_size=1, num_epochs=2, lr=LR, weight_decay=WD,
                          log=lambda s: None, freeze_stages=k)
    tr.opt.eps = EPS
    return tr


def test_detection_trainer_with_a_frozen_stage_resumes_where_it_stopped(tmp_path):
    """the construction of tests/test_finetune_gpu.py::test_detection_trainer_resume_continues_where_it_stopped under freeze_stages=1, with the stochastic-depth
    draws on and seeded by the epoch: one epoch + checkpoint + fresh trainer + resume() + one epoch against two uninterrupted epochs, relerr <= 3e-5 + 4
    relerr(U, U').  The file records freeze_stages, and a trainer under another k refuses it through the range table."""
    from nerf_mae_amd.trainer import save_detection_checkpoint

    def epochs(tr, which):
        for ep in which:
            torch.manual_seed(500 + ep)
            tr.train_epoch(ep)
        torch.cuda.synchronize()
        return tr

    u, u2 = (epochs(_trainer(), (1, 2)).flat._flat.detach().cpu().clone() for _ in range(2))
    a = epochs(_trainer(), (1,))
    assert a.args["freeze_stages"] == 1 and a.model.backbone.base.frozen_stages == 1 and a.opt.ranges is not None
    e = prefix_end(a.flat, 1)
    fresh = C.fcos_model(0).cuda()
    assert torch.equal(a.flat._flat[:e].cpu(), u[:e]) and torch.equal(a.model.backbone.base.patch_partition[0].weight, fresh.backbone.base.patch_partition[0].weight)
    path = str(tmp_path / "epoch_1.pt")
    save_detection_checkpoint(path, a.model, 1, a.args, a.opt, a.global_step)
    assert torch.load(path, weights_only=True)["train_args"]["freeze_stages"] == 1
    with pytest.raises(RuntimeError, match="range"):
        _trainer(k=2, seed=9).resume(path)
    b = _trainer(seed=9)
    ck = b.resume(path)
    assert ck["resume"]["step"] == 2 and b.global_step == 2 and b.start_epoch == 2 and torch.equal(b.flat._flat, a.flat._flat)
    epochs(b, (2,))
    err, spread = relerr(b.flat._flat.detach().cpu(), u), relerr(u2, u)
    _print(f"  [trainer freeze_stages=1 resume] relerr(resumed, uninterrupted) {err:.2e}  relerr(U, U') {spread:.2e}  bound {3 * STEP_BOUND + 4 * spread:.2e}")
    assert err <= 3 * STEP_BOUND + 4 * spread, (err, spread)
    hist = _trainer().fit()
    assert [h["epoch"] for h in hist] == [1, 2] and all(h["train_loss"] == h["train_loss"] for h in hist)


# ---- refusals, and k = 0 ---------------------------------------------------------------------------------------------------------------------------
def test_the_trainers_refuse_what_they_cannot_do():
    from nerf_mae_amd.trainer import DetectionTrainer, RPNTrainer, VoxelTrainer
    scenes, boxes = [C.scene(11)], [C.obb_boxes(11)]
    for bad in (5, -1, 1.5):
        with pytest.raises(ValueError, match="freeze_stages|frozen_stages"):
            DetectionTrainer(fcos_on_gpu(), scenes, boxes, batch_size=1, log=lambda s: None, freeze_stages=bad)
    rpn = C.rpn_model().cuda().train()
    with pytest.raises(ValueError, match="left out as a whole"):
        RPNTrainer(rpn, scenes, [C.aabb_boxes(11)], log=lambda s: None, freeze_backbone=True, freeze_stages=1)
    assert rpn.backbone.base.frozen_stages == 0
    tr = RPNTrainer(rpn, scenes, [C.aabb_boxes(11)], log=lambda s: None, freeze_stages=4)
    assert tr.args["freeze_stages"] == 4 and rpn.backbone.base.frozen_stages == 4
    again = RPNTrainer(rpn, scenes, [C.aabb_boxes(11)], log=lambda s: None)
    assert again.args["freeze_stages"] == 0 and rpn.backbone.base.frozen_stages == 0, "a trainer without a prefix takes an earlier one off the encoder"
    vox = VoxelTrainer(C.semantics_model().cuda().train(), scenes, [C.label_grid(11)], log=lambda s: None, freeze_stages=2)
    assert vox.args["freeze_stages"] == 2 and vox.model.base.frozen_stages == 2
    # the pre-training path
    from nerf_mae_amd.model import build_model
    from nerf_mae_amd.trainer import FusedAdamW, GraphedTrainStep, Trainer
    mae = build_model("swin_t", resolution=32, compute_dtype=torch.float32).cuda()
    mae.frozen_stages = 1
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        Trainer(mae, [C.scene(11)])
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        GraphedTrainStep(mae, FusedAdamW(mae), 1)
    with pytest.raises(ValueError, match="frozen_stages = 1"):
        mae([torch.zeros(4, 32, 32, 32, device="cuda")])


def test_k_zero_is_launch_for_launch_the_path_of_before(monkeypatch):
    """every function of nerf_mae_amd.ops is wrapped to record its name: one step with freeze_stages=0 stated everywhere issues the call list of a step on a model
    whose attribute nobody touched"""
    from nerf_mae_amd import ops
    calls = []

    def recorder(name, fn):
        def wrapped(*a, **kw):
            calls.append(name)
            return fn(*a, **kw)
        return wrapped
    for name, fn in list(vars(ops).items()):
        if inspect.isfunction(fn) and fn.__module__ == ops.__name__ and not name.startswith("_") and not inspect.isgeneratorfunction(inspect.unwrap(fn)):
            monkeypatch.setattr(ops, name, recorder(name, fn))
    lists = {}
    for how in ("untouched", "zero"):
        m = fcos_on_gpu()
        if how == "zero":
            flat, opt, step = setup(m, 0, "A")
            assert opt.ranges is None and "_frozen_stages" in vars(encoder_of(m))
            encoder_of(m).frozen_stages = 0
        else:
            from tests.test_finetune_gpu import fused
            flat, opt, step = fused(m)
        torch.manual_seed(100)
        step(*batches()[0])          # the first step packs the weights
        del calls[:]
        torch.manual_seed(101)
        step(*batches()[1])
        torch.cuda.synchronize()
        lists[how] = list(calls)
    assert len(lists["zero"]) > 100 and lists["zero"] == lists["untouched"]
