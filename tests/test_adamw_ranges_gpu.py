"""nmh_grad_sqnorm_ranges / nmh_adamw_step_ranges, trainer.FusedAdamW(ranges=) and the trainers' layer_decay / no_decay / freeze against the float64 reference
of tests/_adamw_ranges_ref.py (torch.optim.AdamW with one param group per range, clip_grad_norm_ over the groups that train).

Bounds: the project's optimizer bound of tests/test_kernels_gpu.py::test_adamw_and_clip_match_torch -- the clip's norm within 1e-5 relative in every step, the
final parameters relerr < 1e-5 -- here also range by range, so that a few elements under a wrong setting cannot hide among ten thousand right ones.  Frozen
ranges and the one-range case are compared bit for bit.  The trainer-level test uses the construction of tests/test_finetune_gpu.py's resume tests:
relerr(resumed, uninterrupted) <= 3 * 1e-5 + 4 * relerr(U, U') with U' a second uninterrupted run."""
import functools
import os
import sys

import pytest
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402
from tests._adamw_ranges_ref import RangedAdamWRef  # noqa: E402
from tests._metrics import relerr  # noqa: E402

pytestmark = pytest.mark.gpu
BOUND = 1e-5
N = 10007                                # the size of test_adamw_and_clip_match_torch: 2501 16-byte groups in 5 blocks, and a scalar tail of 3
BOUNDS = [0, 4, 8, 1032, 1036, 4096, N]  # a one-group range at the very start, one in the middle, a last range that ends off a multiple of 4
SCALES = [(1.0, 1.0), (0.0, 1.0), (0.5, 0.0), (0.0, 0.0), (0.75 ** 24, 1.0), (1.0, 0.0)]
LR, WD, B1, B2, EPS, CLIP = 1e-3, 1e-2, 0.9, 0.999, 1e-8, 0.1


def _print(*a):
    if os.environ.get("NMH_PRINT_ERR"):
        print(*a)


def _ops():
    from nerf_mae_amd import ops
    return ops


def rnd(n, seed=0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed))


def table(bounds, scales):
    return torch.tensor(bounds, dtype=torch.int64).cuda(), torch.tensor(scales, dtype=torch.float32).reshape(-1, 2).cuda()


def hyper(step, lr=LR, wd=WD, zero_g=0.0):
    return torch.tensor([lr, B1, B2, EPS, wd, 1 - B1 ** step, 1 - B2 ** step, zero_g]).cuda()


def live_ranges(bounds, scales):
    return [(lo, hi) for (lo, hi), (ls, _) in zip(zip(bounds[:-1], bounds[1:]), scales) if ls != 0.0]


def run_kernels(n, bounds, scales, steps=3):
    """`steps` steps with gradients g0 * step from zero moments -> (p, m, v, norms, p0); the float64 reference's (flat, norms, frozen mask)"""
    ops = _ops()
    p0, g0 = rnd(n), rnd(n, seed=1) * 3
    ref = RangedAdamWRef(p0, bounds, scales, WD, (B1, B2), EPS, CLIP)
    b, s = table(bounds, scales)
    p, m, v = p0.cuda(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    coef, nrm = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    norms, ref_norms = [], []
    for step in range(1, steps + 1):
        g = g0 * step
        ref_norms.append(ref.step(g, LR))
        gd = g.cuda()
        ops.grad_sqnorm_ranges(gd, b, s, acc)
        ops.clip_coef(acc, CLIP, coef, nrm)
        ops.adamw_step_ranges(p, gd, m, v, hyper(step), b, s, coef)
        norms.append(nrm.item())
        assert torch.equal(gd.cpu(), g), "without the flag the gradient is left as it is"
    return (p.cpu(), m.cpu(), v.cpu(), norms, p0), (ref.flat(), ref_norms, ref.frozen)


def check_against_reference(n, bounds, scales):
    (p, m, v, norms, p0), (rp, rnorms, frozen) = run_kernels(n, bounds, scales)
    for k, (a, b) in enumerate(zip(norms, rnorms)):
        _print(f"  [ranges n={n}] step {k + 1} norm {a:.7g} vs {b:.7g} rel {abs(a - b) / b:.2e}")
        assert abs(a - b) / b < BOUND
    assert max(rnorms) > CLIP, "the clip is active"
    err = relerr(p, rp)
    _print(f"  [ranges n={n}] parameters relerr {err:.2e}")
    assert err < BOUND
    # Range by range, and on the UPDATE p - p0 as well: the range under 0.75 ** 24 moves by about 3e-6 in three steps, which the bound on p (1e-5 of max |p|)
    # cannot tell from no step at all.  What fp32 allows: each step rounds p once, by at most eps / 2 * |p|; the update's own arithmetic is below that.  So
    # |(p - p0) - (ref - p0)| <= steps * eps * max |p| (a factor 2 of slack) + 1e-5 * max |ref - p0|, and the update must exceed that for the check to see it.
    eps32, steps = torch.finfo(torch.float32).eps, len(norms)
    for lo, hi in live_ranges(bounds, scales):
        e = relerr(p[lo:hi], rp[lo:hi])
        moved = (rp[lo:hi] - p0[lo:hi].double()).abs().max().item()
        tol = steps * eps32 * p0[lo:hi].abs().max().item() + BOUND * moved
        upd = ((p[lo:hi].double() - p0[lo:hi].double()) - (rp[lo:hi] - p0[lo:hi].double())).abs().max().item()
        _print(f"  [ranges n={n}] range [{lo}, {hi}) relerr {e:.2e}  update error {upd:.2e} (allowed {tol:.2e}) of an update of {moved:.2e}")
        assert e < BOUND, (lo, hi, e)
        assert upd <= tol < moved, (lo, hi, upd, tol, moved)
    assert torch.equal(p[frozen], p0[frozen]) and not m[frozen].any() and not v[frozen].any()
    assert m[~frozen].abs().min() > 0 and v[~frozen].min() > 0, "every element that trains has moments"


def test_six_ranges_match_the_float64_reference():
    check_against_reference(N, BOUNDS, SCALES)


def test_one_block_two_ranges():
    check_against_reference(8, [0, 4, 8], [(1.0, 1.0), (0.5, 0.0)])


def test_frozen_ranges_are_not_written_and_their_gradient_is_cleared():
    """from non-zero moments, so that an update with lr = 0 (torch's meaning of it, which moves the moments) would show"""
    ops = _ops()
    b, s = table(BOUNDS, SCALES)
    p0, m0, v0, g = rnd(N, 2).cuda(), rnd(N, 3).cuda() * 1e-2, rnd(N, 4).cuda().square() * 1e-4, rnd(N, 5).cuda()
    frozen = RangedAdamWRef(p0, BOUNDS, SCALES, WD).frozen.cuda()
    assert frozen.sum().item() == 4 + 4
    coef = torch.full((1,), 0.5, device="cuda")
    for zero_g in (0.0, 1.0):
        p, m, v, gd = p0.clone(), m0.clone(), v0.clone(), g.clone()
        ops.adamw_step_ranges(p, gd, m, v, hyper(1, zero_g=zero_g), b, s, coef)
        for now, was in ((p, p0), (m, m0), (v, v0)):
            assert torch.equal(now[frozen], was[frozen])
        assert (m[~frozen] != m0[~frozen]).all() and (v[~frozen] != v0[~frozen]).all()
        assert all((p[lo:hi] != p0[lo:hi]).any() for lo, hi in live_ranges(BOUNDS, SCALES))
        assert (not gd.any()) if zero_g else torch.equal(gd, g), "the flag clears every gradient, frozen ranges included; without it none"


def test_one_range_gives_the_bits_of_adamw_step():
    ops = _ops()
    b, s = table([0, N], [(1.0, 1.0)])
    p0, g0 = rnd(N), rnd(N, seed=1) * 3
    acc = torch.zeros(1, dtype=torch.float64, device="cuda")
    coef, nrm, nrm_r = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    pa, ma, va = p0.cuda(), torch.zeros(N, device="cuda"), torch.zeros(N, device="cuda")
    pb, mb, vb = pa.clone(), ma.clone(), va.clone()
    for step in range(1, 4):
        ga = (g0 * step).cuda()
        gb = ga.clone()
        ops.grad_sqnorm_ranges(ga, b, s, acc)
        ops.clip_coef(acc, CLIP, coef, nrm_r)
        ops.grad_sqnorm(ga, acc)
        ops.clip_coef(acc, CLIP, coef, nrm)
        assert abs(nrm_r.item() - nrm.item()) <= 1e-6 * nrm.item()          # the same sums; the order of the blocks' atomics is free
        h = hyper(step, zero_g=float(step == 3))
        ops.adamw_step(pa, ga, ma, va, h, coef)                          # both from the same inputs and the same coef
        ops.adamw_step_ranges(pb, gb, mb, vb, h, b, s, coef)
        assert torch.equal(pa, pb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ga, gb)
    assert not ga.any() and (pa.cpu() != p0).all()


def test_the_entries_refuse_a_bad_table_and_write_nothing():
    from nerf_mae_amd._lib import NmhError
    ops = _ops()
    n = 64
    cases = {"an interior boundary at 6": ([0, 6, n], [(1.0, 1.0)] * 2, n),
             "a descending table": ([0, 32, 16, n], [(1.0, 1.0)] * 3, n),
             "bounds[R] != n": ([0, 16, n - 4], [(1.0, 1.0)] * 2, n),
             "bounds[0] != 0": ([4, 16, n], [(1.0, 1.0)] * 2, n),
             "a negative scale": ([0, 16, n], [(1.0, 1.0), (-0.5, 1.0)], n),
             "R above the maximum": (list(range(0, 4 * (ops.ADAMW_MAX_RANGES + 2), 4)), [(1.0, 1.0)] * (ops.ADAMW_MAX_RANGES + 1), 4 * (ops.ADAMW_MAX_RANGES + 1))}
    for what, (bounds, scales, n) in cases.items():
        b, s = table(bounds, scales)
        p0, m0, v0, g0 = rnd(n, 2).cuda(), rnd(n, 3).cuda(), rnd(n, 4).cuda().square(), rnd(n, 5).cuda()
        p, m, v, g = p0.clone(), m0.clone(), v0.clone(), g0.clone()
        acc = torch.full((1,), 123.0, dtype=torch.float64, device="cuda")
        with pytest.raises(NmhError, match="bad range table"):
            ops.grad_sqnorm_ranges(g, b, s, acc)
        with pytest.raises(NmhError, match="bad range table"):
            ops.adamw_step_ranges(p, g, m, v, hyper(1, zero_g=1.0), b, s, None)
        torch.cuda.synchronize()
        assert acc.item() == 123.0 and torch.equal(p, p0) and torch.equal(m, m0) and torch.equal(v, v0) and torch.equal(g, g0), what
    b, s = table([0, 16, 64], [(1.0, 1.0), (0.0, 1.0)])                       # the largest table that is taken, and the cases' neighbour that is
    ops.grad_sqnorm_ranges(g0[:64].contiguous(), b, s, acc)
    full = list(range(0, 4 * (ops.ADAMW_MAX_RANGES + 1), 4))
    b, s = table(full, [(1.0, 1.0), (0.0, 1.0)] * (ops.ADAMW_MAX_RANGES // 2))
    g = torch.ones(full[-1], device="cuda")
    ops.grad_sqnorm_ranges(g, b, s, acc)
    assert acc.item() == full[-1] / 2                                       # every second group of four ones


# ---- FusedAdamW(ranges=) over a FlatParameters ------------------------------------------------------------------------------------------------
def two_layers(seed=0):
    torch.manual_seed(seed)
    return nn.Sequential(nn.Linear(37, 19), nn.Linear(19, 5)).cuda()


def host_optimizer(m, wd=0.1):
    """no weight decay on the biases, layer 0 frozen: ranges [0.weight, 0.bias | 1.weight | 1.bias]"""
    from nerf_mae_amd.finetune import FlatParameters, freeze_rules, no_decay_rules, param_ranges
    from nerf_mae_amd.trainer import FusedAdamW
    flat = FlatParameters(m, torch.device("cuda"))
    ranges = param_ranges(flat, freeze_rules(m[0]) + no_decay_rules(m))
    assert ranges.record["scale"] == [[0.0, 1.0], [0.0, 0.0], [1.0, 1.0], [1.0, 0.0]] and ranges.record["bounds"] == [0, 704, 728, 824, 832]
    return flat, ranges, FusedAdamW(flat, lr=LR, weight_decay=wd, max_grad_norm=CLIP, ranges=ranges)


def set_grads(flat, scale):
    """the gradients, written through the parameters' .grad views -> the flat gradient as the reference takes it"""
    for i, (name, p) in enumerate(flat.named_parameters()):
        p.grad.copy_(scale * torch.sin(0.37 * i + 0.11 * torch.arange(p.numel(), device="cuda", dtype=torch.float32)).view(p.shape))
    return flat._flat_grad.clone()


SCHED = ((1.0, 1e-3, 0.9), (0.1, 5e-4, 0.85), (0.004, 2e-3, 0.95))          # (gradient scale, lr, beta1): two steps clip, the third does not


def test_fused_adamw_with_ranges_matches_the_reference():
    m = two_layers()
    flat, ranges, opt = host_optimizer(m)
    p0 = flat._flat.clone()
    ref = RangedAdamWRef(p0, ranges.record["bounds"], ranges.record["scale"], 0.1, (0.9, 0.999), 1e-8, CLIP)
    decayed = RangedAdamWRef(p0, ranges.record["bounds"], [[ls, 1.0] for ls, _ in ranges.record["scale"]], 0.1, (0.9, 0.999), 1e-8, CLIP)
    norms = []
    for scale, lr, b1 in SCHED:
        g = set_grads(flat, scale)
        opt.set_hyper(lr=lr, beta1=b1)
        opt.step()
        tn = ref.step(g, lr, b1)
        decayed.step(g, lr, b1)
        norms.append(tn)
        live = g[728:832].double().norm().item()                            # layer 1 alone: what clip_grad_norm_ sees when layer 0 has no gradient
        assert abs(tn - live) <= 1e-12 * live
        e = abs(opt.norm.item() - tn) / tn
        _print(f"  [host ranges] norm {opt.norm.item():.7g} vs {tn:.7g} rel {e:.2e}")
        assert e < BOUND
    assert norms[0] > CLIP and norms[1] > CLIP and norms[2] < CLIP
    got, want = flat._flat.cpu(), ref.flat()
    for name, (off, numel) in {"1.weight": (728, 95), "1.bias": (824, 5)}.items():
        e = relerr(got[off:off + numel], want[off:off + numel])
        _print(f"  [host ranges] {name} relerr {e:.2e}")
        assert e < BOUND, (name, e)
    assert relerr(got[824:829], decayed.flat()[824:829]) > 10 * BOUND, "a decayed bias would show"
    assert torch.equal(flat._flat[:728], p0[:728]) and not opt.m[:728].any() and not opt.v[:728].any()
    assert torch.equal(m[0].weight.detach(), p0[:703].view(19, 37))


def test_launch_is_graph_capturable():
    """opt.launch() captured once on one stream and replayed twice, update_hyper() between the replays, against the same two steps issued eagerly (which also
    load the kernels before the capture)"""
    eager_m, graph_m = two_layers(), two_layers()
    fe, _, oe = host_optimizer(eager_m)
    fg, ranges, og = host_optimizer(graph_m)
    for flat in (fe, fg):
        set_grads(flat, 1.0)
    for _ in range(2):
        oe.update_hyper()
        oe.launch()
    torch.cuda.synchronize()
    before = fg._flat.clone()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        og.launch()
    torch.cuda.synchronize()
    assert torch.equal(fg._flat, before) and not og.m.any() and og.t == 0      # a capture runs nothing
    for _ in range(2):
        og.update_hyper()
        graph.replay()
    torch.cuda.synchronize()
    assert og.t == oe.t == 2
    assert abs(og.norm.item() - oe.norm.item()) <= BOUND * oe.norm.item()
    for lo, hi in live_ranges(ranges.record["bounds"], ranges.record["scale"]):
        assert relerr(fg._flat[lo:hi], fe._flat[lo:hi]) < BOUND
        assert relerr(og.m[lo:hi], oe.m[lo:hi]) < BOUND and relerr(og.v[lo:hi], oe.v[lo:hi]) < BOUND
    assert torch.equal(fg._flat[:728], before[:728]) and not og.m[:728].any()
    assert relerr(fg._flat[728:], before[728:]) > 10 * BOUND, "the replays stepped"


# ---- the trainers' switches through FinetuneStep ---------------------------------------------------------------------------------------------
T_LR, T_WD, T_EPS, DECAY = 1e-3, 0.5, 1.0, 0.75       # weight decay large enough that its absence on a norm weight shows; eps 1 as tests/test_finetune_gpu.py


@functools.lru_cache(maxsize=None)
def fcos_weights():
    return {k: v.clone() for k, v in C.fcos_model().state_dict().items()}


@functools.lru_cache(maxsize=None)
def two_batches():
    from nerf_mae_amd import data
    batcher = data.DetectionBatcher(C.R, torch.device("cuda"), normalize_density=True)
    out = []
    for seeds in ((1, 2), (3, 4)):
        xb, ext, targets = batcher.prepare([C.scene(s) for s in seeds], [C.obb_boxes(s) for s in seeds], params=[(0, 0.0, 1.0)] * 2)
        out.append(([xb[i].clone() for i in range(2)], [t.clone() for t in targets]))
    torch.cuda.synchronize()
    return out


def recipe_step(seed=0):
    """the common FCOS model under layer_decay = 0.75, no_decay, freeze = its patch embed -> (model, flat, ranges, opt, step)"""
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for, param_ranges, recipe_rules
    from nerf_mae_amd.trainer import FusedAdamW
    m = C.fcos_model(seed=seed)
    if seed == 0:
        m.load_state_dict(fcos_weights(), strict=True)
    m = m.cuda().train()
    flat = FlatParameters(m, torch.device("cuda"))
    ranges = param_ranges(flat, recipe_rules(m, layer_decay=DECAY, no_decay=True, freeze=(m.backbone.base.patch_partition,)))
    opt = FusedAdamW(flat, lr=T_LR, weight_decay=T_WD, eps=T_EPS, max_grad_norm=CLIP, ranges=ranges)
    return m, flat, ranges, opt, FinetuneStep(flat, opt, loss_fn_for(m))


def params_of(m):
    return {n: p.detach().clone() for n, p in m.named_parameters()}


def two_steps(step, ks=(0, 1), keep=None):
    for k in ks:
        torch.manual_seed(100 + k)
        if keep is None:
            step(*two_batches()[k])
            continue
        losses, total = step.forward(*two_batches()[k])       # FinetuneStep.__call__ in its parts, to keep the gradient the update then clears
        total.backward()
        keep.append(step.flat._flat_grad.clone())
        step.opt.step()


@functools.lru_cache(maxsize=None)
def recipe_runs():
    """U: two steps, the gradients kept; U': the same again.  Computed once, shared, left unchanged."""
    m, flat, ranges, opt, step = recipe_step()
    p0, grads = flat._flat.clone(), []
    two_steps(step, keep=grads)
    m2, _, _, _, step2 = recipe_step()
    two_steps(step2)
    torch.cuda.synchronize()
    pu, pu2 = params_of(m), params_of(m2)
    spread = max(relerr(pu2[k], pu[k]) for k in pu)
    return dict(p0=p0, grads=grads, record=ranges.record, layout={n: flat._offsets[id(p)] for n, p in m.named_parameters() if id(p) in flat._offsets},
                flat=flat._flat.clone(), m=opt.m.clone(), pu=pu, spread=spread, bound=3 * BOUND + 4 * spread)


def test_recipe_freezes_the_patch_embed_and_leaves_norm_weights_undecayed():
    r = recipe_runs()
    emb = [n for n in r["pu"] if n.startswith("backbone.base.patch_partition.")]
    assert len(emb) == 4
    for n in emb:
        assert torch.equal(r["pu"][n].cpu(), fcos_weights()[n]), n                       # bit-unchanged, and so are its moments
        off = r["layout"][n]
        assert not r["m"][off:off + r["pu"][n].numel()].any()
    # the last Swin block's second norm: layer id 12 of 12, so lr_scale 0.75, and wd_scale 0
    name = "backbone.base.stages.3.2.norm2.weight"
    off, numel = r["layout"][name], r["pu"][name].numel()
    b = r["record"]["bounds"]
    k = max(i for i in range(len(b) - 1) if b[i] <= off)
    assert r["record"]["scale"][k] == [0.75, 0.0]
    ref = RangedAdamWRef(r["p0"], b, r["record"]["scale"], T_WD, (0.9, 0.999), T_EPS, CLIP)
    decayed = RangedAdamWRef(r["p0"], b, [[ls, 1.0] for ls, _ in r["record"]["scale"]], T_WD, (0.9, 0.999), T_EPS, CLIP)
    for g in r["grads"]:
        ref.step(g, T_LR)
        decayed.step(g, T_LR)
    got, want, other = r["pu"][name].reshape(-1), ref.flat()[off:off + numel], decayed.flat()[off:off + numel]
    e = relerr(got, want)
    _print(f"  [recipe] {name} relerr {e:.2e} against the no-decay update, {relerr(got, other):.2e} against the decayed one")
    assert e < BOUND and relerr(got, other) > 10 * BOUND
    assert relerr(r["flat"], ref.flat()) < BOUND                                          # and the whole buffer, frozen ranges included


def test_recipe_resume_continues_where_it_stopped(tmp_path):
    from nerf_mae_amd.trainer import load_detection_checkpoint, save_detection_checkpoint
    r = recipe_runs()
    m, flat, ranges, opt, step = recipe_step()
    two_steps(step, ks=(0,))
    path = str(tmp_path / "recipe.pt")
    save_detection_checkpoint(path, m, 1, {"lr": T_LR, "layer_decay": DECAY, "no_decay": True}, opt, step=1)
    m2, flat2, ranges2, opt2, step2 = recipe_step(seed=9)          # other weights: everything must come from the file
    ck = load_detection_checkpoint(path, m2, opt2)
    flat2.check()
    assert ck["resume"]["ranges"] == ranges2.record == r["record"] and opt2.t == 1 and torch.equal(opt2.m, opt.m) and torch.equal(opt2.v, opt.v)
    two_steps(step2, ks=(1,))
    torch.cuda.synchronize()
    p2 = params_of(m2)
    err = max(relerr(p2[k], r["pu"][k]) for k in p2)
    _print(f"  [recipe resume] relerr(resumed, uninterrupted) {err:.2e}  relerr(U, U') {r['spread']:.2e}  bound {r['bound']:.2e}")
    assert err <= r["bound"], (err, r["bound"])
    # an optimizer without the table must not take the file
    from nerf_mae_amd.finetune import FlatParameters
    from nerf_mae_amd.trainer import FusedAdamW
    m3 = C.fcos_model(seed=9).cuda().train()
    with pytest.raises(RuntimeError, match="range table"):
        load_detection_checkpoint(path, m3, FusedAdamW(FlatParameters(m3, torch.device("cuda")), lr=T_LR))


# ---- the keywords on the trainer classes ---------------------------------------------------------------------------------------------------
def test_trainer_keywords_build_the_table_and_are_recorded(tmp_path):
    """DetectionTrainer: the three keywords give the optimizer the table recipe_rules gives, land in train_args in plain form and in the checkpoint; the defaults
    give an optimizer without a table.  One epoch of one step runs under it."""
    from nerf_mae_amd.finetune import param_ranges, recipe_rules
    from nerf_mae_amd.trainer import DetectionTrainer, load_detection_checkpoint
    m = C.fcos_model()
    m.load_state_dict(fcos_weights(), strict=True)
    m = m.cuda().train()
    scenes, boxes = [C.scene(11)], [C.obb_boxes(11)]
    tr = DetectionTrainer(m, scenes, boxes, batch_size=1, num_epochs=1, lr=1e-4, log=lambda s: None, layer_decay=DECAY, no_decay=True,
                          freeze=(m.backbone.base.patch_partition, "backbone.base.stages.0.0.norm1"))
    want = param_ranges(tr.flat, recipe_rules(m, DECAY, True, (m.backbone.base.patch_partition, "backbone.base.stages.0.0.norm1")))
    assert tr.opt.range_record == want.record and len(want.record["scale"]) > 13
    assert tr.args["layer_decay"] == DECAY and tr.args["no_decay"] is True and tr.args["freeze"] == ["backbone.base.patch_partition", "backbone.base.stages.0.0.norm1"]
    emb = {n: p.detach().clone() for n, p in m.backbone.base.patch_partition.named_parameters()}
    tr.train_epoch(1)
    assert all(torch.equal(p, emb[n]) for n, p in m.backbone.base.patch_partition.named_parameters())
    tr.save_path = str(tmp_path)
    tr._save("ck.pt", 1)
    ck = load_detection_checkpoint(str(tmp_path / "ck.pt"), m)
    assert ck["train_args"]["freeze"] == tr.args["freeze"] and ck["train_args"]["layer_decay"] == DECAY and ck["resume"]["ranges"] == want.record
    plain = DetectionTrainer(m, scenes, boxes, batch_size=1, num_epochs=1, lr=1e-4, log=lambda s: None)
    assert plain.opt.ranges is None and plain.args["layer_decay"] is None and plain.args["no_decay"] is False and plain.args["freeze"] == []


def test_freezing_what_is_excluded_is_refused():
    from nerf_mae_amd.trainer import RPNTrainer
    m = C.rpn_model().cuda().train()
    scenes, boxes = [C.scene(11)], [C.aabb_boxes(11)]
    with pytest.raises(ValueError, match="matches no parameter"):
        RPNTrainer(m, scenes, boxes, resolution=C.R, freeze_backbone=True, freeze=(m.backbone,), log=lambda s: None)
    with pytest.raises(ValueError, match="layer 0.*matches no parameter"):     # layer decay over an encoder that is not in the buffers
        RPNTrainer(m, scenes, boxes, resolution=C.R, freeze_backbone=True, layer_decay=DECAY, log=lambda s: None)
    tr = RPNTrainer(m, scenes, boxes, resolution=C.R, freeze_backbone=True, no_decay=True, freeze=("rpn.head.conv",), log=lambda s: None)   # the two compose
    assert tr.exclude == (m.backbone,) and tr.opt.ranges is not None and tr.args["freeze"] == ["rpn.head.conv"] and tr.args["freeze_backbone"] is True


def test_pretraining_trainer_takes_no_decay_and_freeze(tmp_path):
    """Trainer, the pre-training loop: its step is a HIP graph, so the ranged launches are captured with the forward and backward.  One epoch of two steps on a
    tiny encoder: the frozen patch embed and mask_token are bit-unchanged with zero moments, everything else trained, and the file carries table and keywords."""
    from nerf_mae_amd import data
    from nerf_mae_amd.model import SwinTransformer_MAE3D
    from nerf_mae_amd.trainer import FusedAdamW, Trainer, load_checkpoint, save_checkpoint
    tiny = dict(patch_size=[4] * 3, window_size=[4] * 3, embed_dim=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8], resolution=32, masking_prob=0.75,
                stochastic_depth_prob=0.1)
    torch.manual_seed(0)
    model = SwinTransformer_MAE3D(compute_dtype=torch.float32, **tiny).cuda()
    scenes = [data.synthetic_scene((32, 32, 32), i) for i in range(4)]
    tr = Trainer(model, scenes, batch_size=2, num_epochs=1, lr=2e-3, log=lambda s: None, no_decay=True, freeze=(model.patch_partition, "mask_token"))
    assert tr.args["no_decay"] is True and tr.args["freeze"] == ["patch_partition", "mask_token"]
    rec = tr.opt.range_record
    assert rec["scale"][0] == [0.0, 0.0] and rec["scale"][1] == [0.0, 1.0] and [1.0, 0.0] in rec["scale"] and [1.0, 1.0] in rec["scale"]   # mask_token leads
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    tr.train_epoch(1)
    torch.cuda.synchronize()
    lo = rec["bounds"][next(i for i, s in enumerate(rec["scale"]) if s[0] != 0.0)]         # where the frozen head of the buffer ends
    for n, p in model.named_parameters():
        if n == "mask_token" or n.startswith("patch_partition."):
            assert torch.equal(p, before[n]), n
        elif p.requires_grad and p.dim() > 1:           # (a conv bias in front of an InstanceNorm has no gradient, and under no_decay nothing else moves it)
            assert not torch.equal(p, before[n]), n
    assert lo > 0 and not tr.opt.m[:lo].any() and not tr.opt.v[:lo].any() and tr.opt.m[lo:].any()
    path = str(tmp_path / "pre.pt")
    save_checkpoint(path, model, 1, tr.args, tr.opt, tr.global_step)
    with pytest.raises(RuntimeError, match="range table"):
        load_checkpoint(path, model, FusedAdamW(model))
    ck = load_checkpoint(path, model, tr.opt)
    assert ck["resume"]["ranges"] == rec and ck["train_args"]["freeze"] == ["patch_partition", "mask_token"]
