"""FCOS target assignment and training losses on the GPU (nerf_mae_amd.fcos_loss over csrc/fcos.hip) against the float64 restatement of
tests/_fcos_ref.py (itself checked against the recorded reference in tests/test_fcos_ref_cpu.py) and against the recorded reference
(tests/golden/g18_fcos_loss.npz) directly.

Tolerance: the project's contract for fp32, assert_close(rtol=1e-3).  Labels, box indices and validity are compared exactly; that is defined
because the generator's scenes have a margin of at least 1e-3 voxels on every decision (asserted in the CPU test), against an fp32 error of
about 1e-5 voxels on coordinates below 100.  Measured on an MI355X (NMH_PRINT_ERR=1): DESIGN.md 3.9."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_ref as F  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

ONE = dict(sizes=((1, 1, 1),), strides=(4,))
# Two scenes of 42^3 + 3^3 locations are 2 x (290 + 1) = 582 workgroups of every loss kernel, more than the 256 partial sums that the final pass takes in its
# first round, so its strided loop runs.  The scene seed is the first whose decisions all have their margin (asserted in ref_assign) and which has
# positives in both scenes and on both levels.
WIDE = dict(sizes=((42, 42, 42), (3, 3, 3)), strides=(4, 56), orig=((168, 168, 168), (150, 168, 121)), nbox=(12, 5), seed=1)
LOSS_CASES = [(False, t, False, False) for t in ("iou", "linear_iou", "giou")] + [(True, t, l1, False) for t in ("iou", "linear_iou", "giou", "diou") for l1 in (False, True)]
LOSS_CASES.append((True, "giou", True, True))
LOSS_IDS = [f"{o}-{t}-{l1}" + ("-above-256-partials" if wide else "") for o, t, l1, wide in LOSS_CASES]


def _m():
    from nerf_mae_amd import fcos_loss
    return fcos_loss


def _one_box(use_obb):
    return [torch.tensor([[2.2, 1.9, 2.4, 3.1, 2.7, 3.9, 0.4]] if use_obb else [[0.4, 0.7, 0.2, 3.9, 3.3, 4.1]])]


@functools.lru_cache(maxsize=None)
def scene(use_obb, small):
    return tuple(_one_box(use_obb) if small else F.make_scene(F.SEED[use_obb], use_obb))


@functools.lru_cache(maxsize=None)
def wide_scene(use_obb):
    return tuple(F.make_scene(WIDE["seed"], use_obb, nbox=WIDE["nbox"], extent=WIDE["orig"][0]))


@functools.lru_cache(maxsize=None)
def wide_assign(use_obb):
    """center sampling 1.5, normalised targets"""
    a = F.assign(list(wide_scene(use_obb)), 1.5, True, WIDE["sizes"], WIDE["strides"], WIDE["orig"])
    n0, pos = 42 ** 3, a["valid"] & (a["labels"] > 0)
    assert min(F.decision_margins(a).values()) >= 1e-3 and pos[:n0].any() and pos[n0:2 * n0].any() and pos[2 * n0:].any()
    return a


@functools.lru_cache(maxsize=None)
def ref_assign(use_obb, radius, norm, small):
    if small:
        return F.assign(list(scene(use_obb, True)), radius, norm, **ONE)
    return F.assign(list(scene(use_obb, False)), radius, norm, orig=F.ORIG)


def _heads(use_obb, norm, wide):
    return F.make_heads(F.HEAD_SEED, use_obb, norm, len(WIDE["nbox"]), WIDE["sizes"], WIDE["strides"]) if wide else F.make_heads(F.HEAD_SEED, use_obb, norm)


@functools.lru_cache(maxsize=None)
def ref_losses(use_obb, loss_type, add_l1, wide=False):
    """float64 losses and the gradients of (1.0 cls + 0.7 reg + 1.3 ctr) in the dense layout; center sampling 1.5, normalised targets"""
    a = wide_assign(use_obb) if wide else ref_assign(use_obb, 1.5, True, False)
    heads = [[t.double().requires_grad_(True) for t in ts] for ts in _heads(use_obb, True, wide)]
    out = F.losses(*heads, a, loss_type, add_l1)
    (out[0] + 0.7 * out[1] + 1.3 * out[2]).backward()
    return [o.detach() for o in out], F.flatten_heads(*[[t.grad for t in ts] for ts in heads])


def _sizes_dev(wide=False):
    return torch.tensor(WIDE["orig"] if wide else F.ORIG, dtype=torch.int32).cuda()


def _gpu_heads(use_obb, norm=True, wide=False):
    return [[t.cuda().requires_grad_(True) for t in ts] for ts in _heads(use_obb, norm, wide)]


def _run(M, use_obb, loss_type, add_l1, heads, boxes, weights=(1.0, 0.7, 1.3), strides=F.STRIDES, **kw):
    fn = M.FCOSLossComputation(list(strides), 1.5, loss_type, True, 1, use_obb, add_l1)
    out = fn(None, heads[0], heads[1], heads[2], boxes, None, **kw)
    sum(w * o for w, o in zip(weights, out)).backward()
    return out


# ---- 1. assignment -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("small", (False, True), ids=("pyramid", "one-location"))
@pytest.mark.parametrize("norm", (False, True), ids=("raw", "normalised"))
@pytest.mark.parametrize("radius", (0.0, 1.5))
@pytest.mark.parametrize("use_obb", (False, True), ids=("aabb", "obb"))
def test_targets_against_float64(use_obb, radius, norm, small):
    M = _m()
    a = ref_assign(use_obb, radius, norm, small)
    boxes = [b.cuda() for b in scene(use_obb, small)]
    if small:
        out = M.fcos_targets(ONE["sizes"], ONE["strides"], boxes, radius, norm, return_scalars=True)
        assert a["npos"] == 1
    else:
        out = M.fcos_targets(F.SIZES, F.STRIDES, boxes, radius, norm, grid_sizes=_sizes_dev(), return_scalars=True)
    labels, tg, gi, ct, valid, scalars = [t.cpu() for t in out]
    assert labels.dtype == torch.float32 and gi.dtype == torch.int32 and valid.dtype == torch.bool
    assert torch.equal(labels.double(), a["labels"]) and torch.equal(gi.long(), a["gt_index"]) and torch.equal(valid, a["valid"])
    assert_close(tg, a["targets"], 1e-3, "reg_targets")
    assert_close(ct, a["ctr"], 1e-3, "centerness_targets")
    assert (tg[labels == 0] == 0).all() and (ct[labels == 0] == 0).all()
    assert scalars[0].item() == a["npos"]
    assert abs(scalars[1].item() - a["csum"]) <= 1e-5 * a["csum"], (scalars[1].item(), a["csum"])
    if not small and radius == 1.5 and norm:     # the padding masks give the same validity as the sizes
        masks = [m.cuda() for m in F.valid_masks(F.ORIG)]
        again = M.fcos_targets(F.SIZES, F.STRIDES, boxes, radius, norm, padding_masks=masks, return_scalars=True)
        assert all(torch.equal(x.cpu(), y) for x, y in zip(again, (labels, tg, gi, ct, valid, scalars)))
        g = np.load(os.path.join(ROOT, "tests", "golden", "g18_fcos_loss.npz"))
        pre = "o_" if use_obb else "a_"
        assert torch.equal(labels, torch.from_numpy(g[pre + "labels"]))
        pos = labels > 0
        assert_close(tg[pos], torch.from_numpy(g[pre + "reg_targets"])[pos], 1e-3, "g18 reg_targets")


def test_encode_decode():
    M = _m()
    boxes = scene(True, False)[0]
    locs = torch.from_numpy(np.random.default_rng(4).uniform(0, 80, (boxes.shape[0], 3)).astype(np.float32))
    enc = M.encode_fcos_obb(locs.cuda(), boxes.cuda())
    assert_close(enc.cpu(), F.encode(locs.double(), boxes.double()), 1e-3, "encode")
    reg = F.flatten_heads(*[F.make_heads(F.HEAD_SEED, True, True)[1]] * 3)[1][:4000]
    loc2 = torch.from_numpy(np.random.default_rng(5).uniform(0, 80, (4000, 3)).astype(np.float32))
    w = torch.randn(4000, 7, generator=torch.Generator().manual_seed(1))
    r64 = reg.double().requires_grad_(True)
    want = F.decode(loc2.double(), r64)
    (want * w.double()).sum().backward()
    rg = reg.cuda().requires_grad_(True)
    got = M.decode_fcos_obb(loc2.cuda(), rg)
    (got * w.cuda()).sum().backward()
    assert_close(got.detach().cpu(), want.detach(), 1e-3, "decode")
    assert_close(rg.grad.cpu(), r64.grad, 1e-3, "decode gradient")


# ---- 2. losses and gradients -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_obb,loss_type,add_l1,wide", LOSS_CASES, ids=LOSS_IDS)
def test_losses_and_gradients_against_float64(use_obb, loss_type, add_l1, wide):
    M = _m()
    want, wgrads = ref_losses(use_obb, loss_type, add_l1, wide)
    a = wide_assign(use_obb) if wide else ref_assign(use_obb, 1.5, True, False)
    boxes = wide_scene(use_obb) if wide else scene(use_obb, False)
    heads = _gpu_heads(use_obb, wide=wide)
    out = _run(M, use_obb, loss_type, add_l1, heads, [b.cuda() for b in boxes], strides=WIDE["strides"] if wide else F.STRIDES, grid_sizes=_sizes_dev(wide))
    tag = f"{'obb' if use_obb else 'aabb'} {loss_type}{' +l1' if add_l1 else ''}{' wide' if wide else ''}"
    assert_close(torch.stack([o.detach() for o in out]).cpu(), torch.stack(want), 1e-3, f"{tag} losses")
    grads = F.flatten_heads(*[[t.grad.cpu() for t in ts] for ts in heads])
    for name, g, wgt in zip(("d box_cls", "d box_regression", "d centerness"), grads, wgrads):
        assert_close(g, wgt, 1e-3, f"{tag} {name}")
    off = ~(a["valid"] & (a["labels"] > 0))
    assert (grads[1][off] == 0).all() and (grads[2][off] == 0).all() and (grads[0][~a["valid"]] == 0).all()
    assert (grads[1][~off].abs().sum(-1) > 0).all()


@pytest.mark.parametrize("pre,use_obb,loss_type,add_l1", (("a_", False, "giou", False), ("o_", True, "iou", True)), ids=("aabb-giou", "obb-iou-l1"))
def test_losses_and_gradients_against_the_recorded_reference(pre, use_obb, loss_type, add_l1):
    M = _m()
    g = np.load(os.path.join(ROOT, "tests", "golden", "g18_fcos_loss.npz"))
    heads = _gpu_heads(use_obb, bool(g["norm"]))
    boxes = [torch.from_numpy(g[pre + "boxes"][a:b]).cuda() for a, b in zip(g[pre + "offsets"][:-1], g[pre + "offsets"][1:])]
    masks = [m.cuda() for m in F.valid_masks(F.ORIG)]
    fn = M.FCOSLossComputation(list(F.STRIDES), float(g["radius"]), loss_type, bool(g["norm"]), 1, use_obb, add_l1)
    out = fn(None, heads[0], heads[1], heads[2], boxes, masks)
    sum(out).backward()
    assert_close(torch.stack([o.detach() for o in out]).cpu(), torch.from_numpy(g[pre + "losses"]), 1e-3, f"g18 {pre}losses")
    grads = F.flatten_heads(*[[t.grad.cpu() for t in ts] for ts in heads])
    for name, v in zip(("grad_cls", "grad_reg", "grad_ctr"), grads):
        assert_close(v, torch.from_numpy(g[pre + name]), 1e-3, f"g18 {pre}{name}")


def test_no_positives():
    M = _m()
    for use_obb in (False, True):
        heads = _gpu_heads(use_obb)
        empty = [torch.zeros((0, 7 if use_obb else 6), device="cuda") for _ in range(3)]
        out = _run(M, use_obb, "iou", use_obb, heads, empty, grid_sizes=_sizes_dev())
        assert out[1].item() == 0 and out[2].item() == 0
        x = F.flatten_heads(*[[t.detach().cpu().double() for t in ts] for ts in heads])[0]
        valid = ref_assign(use_obb, 1.5, True, False)["valid"]
        want = F.focal(x[valid], torch.zeros(int(valid.sum()), dtype=F.F64)).sum()          # normalised by max(0, 1) = 1
        assert np.isfinite(out[0].item()) and abs(out[0].item() - want.item()) <= 1e-3 * want.item()
        assert all((t.grad == 0).all() for t in heads[1]) and all((t.grad == 0).all() for t in heads[2])
        assert sum(t.grad.abs().sum().item() for t in heads[0]) > 0


def test_two_runs_are_bit_identical():
    M = _m()
    res = []
    for _ in range(2):
        heads = _gpu_heads(True)
        out = _run(M, True, "giou", True, heads, [b.cuda() for b in scene(True, False)], grid_sizes=_sizes_dev())
        res.append([o.detach().clone() for o in out] + [t.grad for ts in heads for t in ts])
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ---- 3. capture and synchronisation ------------------------------------------------------------------------------------------------------
def test_forward_backward_in_a_captured_graph_and_without_host_synchronisation():
    M = _m()
    boxes, sizes = [b.cuda() for b in scene(True, False)], _sizes_dev()
    fn = M.FCOSLossComputation(list(F.STRIDES), 1.5, "iou", True, 1, True, True)
    base = [[t.cuda() for t in ts] for ts in F.make_heads(F.HEAD_SEED, True, True)]

    def leaves():
        return [[t.clone().requires_grad_(True) for t in ts] for ts in base]

    def run(heads):
        out = fn(None, heads[0], heads[1], heads[2], boxes, None, grid_sizes=sizes)
        flat = [t for ts in heads for t in ts]
        return [o.detach() for o in out] + list(torch.autograd.grad(out[0] + out[1] + out[2], flat))

    heads = leaves()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        eager = run(heads)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        heads = leaves()
        run(heads)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(heads)
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert len(out) == 15 and all(torch.equal(a, b) for a, b in zip(out, eager))
    assert eager[1].item() > 0 and eager[-1].abs().sum().item() > 0


# ---- 4. error paths ----------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    M = _m()
    heads = _gpu_heads(False)
    boxes = [b.cuda() for b in scene(False, False)]
    fn = M.FCOSLossComputation(list(F.STRIDES), 1.5, "giou", True, 1, False, False)
    with pytest.raises(TypeError):
        fn(None, [t.double() for t in heads[0]], heads[1], heads[2], boxes, None)
    with pytest.raises(RuntimeError):
        fn(None, [t.cpu() for t in heads[0]], heads[1], heads[2], boxes, None)
    with pytest.raises(ValueError):
        M.FCOSLossComputation([4, 8, 16, 32, 64], 1.5, "giou", True, 1, False, False)
    with pytest.raises(ValueError):
        M.fcos_targets(F.SIZES + ((2, 2, 2),), F.STRIDES + (64,), boxes)
    with pytest.raises(NotImplementedError):
        M.FCOSLossComputation(list(F.STRIDES), 1.5, "smooth_l1", True, 1, False, False)
    with pytest.raises(NotImplementedError):
        M.FCOSLossComputation(list(F.STRIDES), 1.5, "iou", True, 1, True, False, proj2d_loss_weight=0.5)
