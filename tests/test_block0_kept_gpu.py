"""GPU: stage 0's first Swin block on the kept windows plus one representative all-mask window per sample (ops.BLOCK0_KEPT, csrc/block0.hip) against the dense
block (the switch off): the kernels alone against torch indexing / float64 sums, the block's dense output bit for bit, loss and gradients of the whole model,
a capacity above the kept count, the captured step and its fall-back for a mask that cuts through windows.

Bounds.  fp32 gradients differ by the order of fp32 sums only: max(4 x run-to-run noise, 2e-6), the bound of test_patch_embed_of_the_kept_tokens_only_changes_nothing.
bf16: the summed gradient of the representative rows is rounded once where the dense path rounds per row, so the change may move the gradients by at most HALF of
what the bf16 arithmetic itself moves them: half the distance of the dense bf16 path to the fp32 mode on the same input and mask (both figures are printed)."""
import random

import numpy as np
import pytest
import torch

from tests._metrics import relerr
from tests.test_model_gpu import SWIN_T, _pair

pytestmark = pytest.mark.gpu

U32, UBF = 2.0 ** -24, 2.0 ** -8   # unit roundoffs: fp32 (24-bit significand), bf16 (8-bit significand), round to nearest


def _masks():
    from oracle import mae3d_oracle as O
    one = torch.zeros(8, 8, 8, dtype=torch.uint8)
    one[4:, :4, 4:] = 1
    return {"bernoulli": O.draw_block_mask((8, 8, 8), 0.75, rng=random.Random(8)), "one_removed": one, "all_removed": torch.ones(8, 8, 8, dtype=torch.uint8)}


def _unaligned():
    m = torch.ones(8, 8, 8, dtype=torch.uint8)
    m[2:6, :4, :4] = 0     # a kept 4^3 block that straddles two windows
    m[4:, 4:, 4:] = 0
    return m


def _inputs():
    from oracle import mae3d_oracle as O
    return [O.synthetic_grid((32, 32, 32), 41).cuda(), O.synthetic_grid((32, 30, 27), 42).cuda()]


def _win_tokens(g):
    """[nW, 64] token index of in-window position i of window w (raster order of windows, (dz, dy, dx) inside)"""
    nw = g // 4
    t = np.arange(g ** 3).reshape(nw, 4, nw, 4, nw, 4).transpose(0, 2, 4, 1, 3, 5).reshape(nw ** 3, 64)
    return torch.from_numpy(t)


def test_mask_window_aligned_is_decided_on_the_host():
    from nerf_mae_amd.model import mask_window_aligned
    for m in _masks().values():
        assert mask_window_aligned(m.numpy())
    assert not mask_window_aligned(_unaligned().numpy())
    assert not mask_window_aligned(np.zeros((6, 6, 6), dtype=np.uint8))      # 6 % 4 != 0
    assert not mask_window_aligned(np.zeros((8, 8, 4), dtype=np.uint8))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("g,extra", [(8, 0), (8, 2), (16, 3)])
def test_row_map_expand_and_reduce_alone(dtype, g, extra):
    """g = 16: 64 windows, the representative sum runs over 16 segments of 4 windows; g = 8: one window per segment.  extra: slots behind the kept count"""
    from nerf_mae_amd import ops
    B, C, nW, n = 2, 96, (g // 4) ** 3, g ** 3
    rng = np.random.RandomState(g + extra)
    bits = (rng.rand(nW) < 0.6).astype(np.uint8)
    bits[1], bits[2] = 0, 1
    kept = np.flatnonzero(bits == 0)
    removed = torch.from_numpy(np.flatnonzero(bits == 1))
    capW = len(kept) + extra
    wt = _win_tokens(g)
    mask = torch.zeros(n, dtype=torch.uint8)
    mask[wt[removed].flatten()] = 1
    rowmap, wmap = ops.block0_window_rows(mask.cuda(), g, capW)
    rowmap, wmap = rowmap.cpu(), wmap.cpu()
    want_w = -np.ones(nW + capW, dtype=np.int64)
    want_w[kept] = np.arange(len(kept))
    want_w[nW:nW + len(kept)] = kept
    assert np.array_equal(wmap.numpy(), want_w)
    want_r = -torch.ones(n + 2, dtype=torch.int64)
    want_r[wt[kept].flatten()] = torch.arange(64 * len(kept))
    want_r[n], want_r[n + 1] = 64 * len(kept), 0
    assert torch.equal(rowmap.long(), want_r)
    # a capacity below the kept count: flagged, nothing out of range
    assert len(kept) > 1
    rm2, wm2 = ops.block0_window_rows(mask.cuda(), g, len(kept) - 1)
    assert rm2[n].item() == 64 * (len(kept) - 1) and rm2[n + 1].item() == 1 and wm2.max().item() < max(nW, len(kept) - 1) and rm2[:n].max().item() < 64 * (len(kept) - 1)

    torch.manual_seed(g)
    yc = torch.randn(B, capW + 1, 64, C).to(dtype)
    y = ops.block0_expand(yc.cuda().view(-1, C), wmap.cuda(), B, g, capW, C).cpu().view(B, n, C)
    want = torch.empty(B, n, C, dtype=dtype)
    want[:, wt[kept].flatten()] = yc[:, :len(kept)].reshape(B, -1, C)
    want[:, wt[removed].flatten()] = yc[:, capW:].expand(B, len(removed), 64, C).reshape(B, -1, C)
    assert torch.equal(y, want)                                                   # expand is a copy: exact

    dy = torch.randn(B, n, C).to(dtype)
    dyc = ops.block0_reduce(dy.cuda().view(-1, C), wmap.cuda(), B, g, capW, C).cpu().view(B, capW + 1, 64, C)
    assert torch.equal(dyc[:, :len(kept)].reshape(B, -1, C), dy[:, wt[kept].flatten()])   # kept windows: copied
    assert (dyc[:, len(kept):capW] == 0).all()                                             # behind the count: zero
    terms = dy[:, wt[removed]].double()                                                   # [B, removed, 64, C]
    exact, mag = terms.sum(1), terms.abs().sum(1)
    # fixed order: at most ceil(nW / 16) terms per segment in sequence, then 16 partial sums in sequence -> (L - 1 + 15) roundings of partial sums <= sum |x|;
    # then one rounding to the compute dtype
    L = -(-nW // 16)
    bound = (L + 14) * U32 * mag + (UBF * exact.abs() if dtype == torch.bfloat16 else 0.0) + 1e-30
    err = (dyc[:, capW].double() - exact).abs()
    print(f"reduce [{dtype}, g {g}]: {len(removed)} removed windows, worst error / bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all()


def _run(hip, xs, bm, dense_out=None):
    hip.zero_grad()
    hook = None
    if dense_out is not None:   # switch off: the block's own output IS the dense tensor
        hook = hip.stages[0][0].register_forward_hook(lambda mod, i, o: dense_out.append(o.detach().reshape(-1, o.shape[-1]).clone()))
    try:
        out = hip(xs, block_mask=bm)
    finally:
        if hook is not None:
            hook.remove()
    out[0].backward()
    torch.cuda.synchronize()
    return out[0].item(), hip._flat_grad.clone()


def _slice(hip, flat, p):
    off = hip._offsets[id(p)]
    return flat[off:off + p.numel()]


@pytest.mark.parametrize("mode", ["fp32", "bf16", "bf16_fused"])
def test_block0_on_the_kept_windows_changes_nothing(monkeypatch, mode):
    """bf16_fused: the row / window thresholds at 1, so that block 0 runs the fused attention and the LDS MLP (the kernels of the benchmark's shapes) on both sides"""
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import SwinBlock3D
    dtype = torch.float32 if mode == "fp32" else torch.bfloat16
    if mode == "bf16_fused":
        for name in ("SWIN_ATTN_MIN_WINDOWS", "SWIN_MLP_MIN_ROWS", "MLP_FUSED_MIN_ROWS"):
            monkeypatch.setattr(ops, name, 1)
    _, hip = _pair(SWIN_T, dtype, res=32, init="default")
    ref32 = None
    if dtype == torch.bfloat16:
        _, ref32 = _pair(SWIN_T, torch.float32, res=32, init="default")   # the same weights (same seed): the fp32 mode
    xs = _inputs()
    plans = []
    real_plan = SwinBlock3D._plan
    monkeypatch.setattr(SwinBlock3D, "_plan", lambda self, *a: (plans.append((self is hip.stages[0][0], real_plan(self, *a))), plans[-1][1])[1])
    expands = []
    real_expand = ops.block0_expand
    monkeypatch.setattr(ops, "block0_expand", lambda *a, **k: (expands.append(real_expand(*a, **k)), expands[-1])[1])
    table, token = hip.stages[0][0].attn.relative_position_bias_table, hip.mask_token
    for name, bm in _masks().items():
        res, dense, b0_plans = [], [], []
        for flag in (False, True, False):
            monkeypatch.setattr(ops, "BLOCK0_KEPT", flag)
            del plans[:], expands[:]
            res.append(_run(hip, xs, bm, dense_out=None if flag else dense))
            assert len(expands) == (1 if flag else 0)             # the path under test is the one that ran
            if flag:
                dense.append(expands[0].detach().clone())
            b0_plans.append([p for first, p in plans if first])
        assert b0_plans[0] == b0_plans[1] and len(b0_plans[1]) == 1, b0_plans    # the same BlockPlan on both sides
        if mode == "bf16_fused":
            assert b0_plans[1][0].attn == "fused" and b0_plans[1][0].mlp == "lds"
        assert torch.equal(dense[0], dense[1]) and torch.equal(dense[0], dense[2]), name   # block 0's dense output: bit-identical
        assert abs(res[0][0] - res[1][0]) <= 5e-6 * abs(res[0][0]), (name, res[0][0], res[1][0])
        assert torch.isfinite(res[1][1]).all()
        if dtype == torch.bfloat16:
            monkeypatch.setattr(ops, "BLOCK0_KEPT", False)
            g32 = _run(ref32, xs, bm)[1]
        for what, pick in (("all", lambda m, f: f), ("bias table of block 0", lambda m, f: _slice(m, f, m.stages[0][0].attn.relative_position_bias_table)),
                           ("mask_token", lambda m, f: _slice(m, f, m.mask_token))):
            off0, on, off1 = (pick(hip, r[1]).double() for r in res)
            ref = off0 if dtype == torch.float32 else pick(ref32, g32).double()
            scale = ref.abs().max().item()     # every distance of a tensor is taken relative to ONE scale, the largest entry of its fp32 gradient
            diff, noise = (on - off0).abs().max().item() / scale, (off1 - off0).abs().max().item() / scale
            if name == "all_removed" and what == "bias table of block 0":
                # the exact gradient is ZERO here (dS = 0 in a window of identical rows, and no window holds anything else): both paths hold the cancellation noise
                # of the softmax backward alone -- fp32: 3.4e-10 in the dense path against 9.5e-6 for the same table under the Bernoulli mask; bf16: two runs of the
                # dense path differ by as much as the two paths do -- and no bound relative to that noise can hold between two summation orders.  The reference's own
                # error is the yardstick: the kept-window path may differ from the dense path by no more than the dense path differs from the exact value, zero
                # (or from itself, run to run)
                exact0, d, nz = off0.abs().max().item(), (on - off0).abs().max().item(), (off1 - off0).abs().max().item()
                print(f"[{mode}, {name}, {what}] exact gradient 0: on vs off {d:.3e} absolute, dense path vs exact {exact0:.3e}, run-to-run {nz:.3e}")
                assert d <= max(4 * nz, exact0), (name, what, d, nz, exact0)
                continue
            if dtype == torch.float32:
                print(f"[{mode}, {name}, {what}] on vs off {diff:.3e}, run-to-run {noise:.3e} (scale {scale:.3e})")
                assert diff <= max(4 * noise, 2e-6), (name, what, diff, noise)
            else:
                dist = (off0 - ref).abs().max().item() / scale
                print(f"[{mode}, {name}, {what}] on vs off {diff:.3e}, dense bf16 vs fp32 mode {dist:.3e}, run-to-run {noise:.3e} (scale {scale:.3e})")
                assert diff <= 0.5 * dist, f"{name}, {what}: kept-window path differs from the dense bf16 path by {diff:.3e}, the dense bf16 path from the fp32 mode by {dist:.3e}"
    assert table.grad is not None and token.grad is not None


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_mask_that_cuts_through_windows_takes_the_dense_block(monkeypatch, dtype):
    from nerf_mae_amd import ops
    _, hip = _pair(SWIN_T, dtype, res=32, init="default")
    xs, bm = _inputs(), _unaligned()
    calls = []
    real_expand = ops.block0_expand
    monkeypatch.setattr(ops, "block0_expand", lambda *a, **k: (calls.append(1), real_expand(*a, **k))[1])
    res = []
    for flag in (False, True, False):
        monkeypatch.setattr(ops, "BLOCK0_KEPT", flag)
        res.append(_run(hip, xs, bm))
    assert not calls                                                     # the dense block ran, switch on or off
    noise = relerr(res[0][1], res[2][1])
    assert abs(res[0][0] - res[1][0]) <= 5e-6 * abs(res[0][0])
    assert relerr(res[1][1], res[0][1]) <= max(4 * noise, 2e-6), (relerr(res[1][1], res[0][1]), noise)   # the same launches: run-to-run noise only


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_capacity_above_the_kept_window_count(monkeypatch, dtype):
    """what a captured step runs with: forward_static with the bound's rows above the kept count -- zero windows behind the count.  Bounds: those of the capacity
    part of test_patch_embed_of_the_kept_tokens_only_changes_nothing"""
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import EmbedBound, embed_capacity_rows
    _, hip = _pair(SWIN_T, dtype, res=32, init="default")
    xs, bm = _inputs(), _masks()["bernoulli"]
    calls = []
    real_expand = ops.block0_expand
    monkeypatch.setattr(ops, "block0_expand", lambda *a, **k: (calls.append(a[4]), real_expand(*a, **k))[1])
    hip._ensure_ready(torch.device("cuda"))
    xb, ext = hip.transform(xs, torch.device("cuda"))
    md = bm.to(torch.uint8).contiguous().view(-1).cuda()
    exact = embed_capacity_rows(8, kept=int(512 - int(bm.sum())))
    assert exact < 512
    outs = []
    for cap in (exact, 512):
        hip.zero_grad()
        torch.manual_seed(3)
        l = hip.forward_static(xb, ext, md, EmbedBound(cap, aligned=True))
        l[0].backward()
        torch.cuda.synchronize()
        outs.append((l[0].item(), hip._flat_grad.clone()))
    assert calls == [exact // 64, 8]                                     # both ran the kept-window path, with these slot counts
    assert abs(outs[1][0] - outs[0][0]) <= 5e-6 * abs(outs[0][0])
    assert relerr(outs[1][1], outs[0][1]) <= (2e-5 if dtype == torch.float32 else 5e-3)
    assert torch.isfinite(outs[1][1]).all()


def test_captured_step_replays_the_kept_window_block_and_falls_back(monkeypatch):
    """GraphedTrainStep with two different window-aligned masks against eager steps of a second model on the same masks, then a mask that cuts through windows:
    the step is captured again with the dense block (as on a capacity overflow) and still agrees.  Bounds: the loss as in
    test_graphed_step_recaptures_when_a_mask_keeps_more_tokens_than_the_embed_capacity (2e-5), the global gradient norm at the bf16 gradient bound of the capacity test (5e-3)"""
    from nerf_mae_amd import ops
    from nerf_mae_amd.trainer import FusedAdamW, GraphedTrainStep
    _, hip = _pair(SWIN_T, torch.bfloat16, res=32, init="default")
    _, ref = _pair(SWIN_T, torch.bfloat16, res=32, init="default")
    ref.load_state_dict(hip.state_dict(), strict=True)
    xs = _inputs()
    opt = FusedAdamW(hip, lr=0.0, weight_decay=0.0, max_grad_norm=0.1)     # lr 0: the weights stay put
    step = GraphedTrainStep(hip, opt, 2)
    step.bound = step.bound._replace(rows=256)                                           # four window slots: above the first mask's count, equal to the second's
    calls = []
    real_expand = ops.block0_expand
    monkeypatch.setattr(ops, "block0_expand", lambda *a, **k: (calls.append(1), real_expand(*a, **k))[1])
    m1 = torch.ones(8, 8, 8, dtype=torch.uint8)
    m1[:4, :4, :4] = 0
    m1[4:, 4:, :4] = 0                                                    # two windows kept
    m2 = torch.ones(8, 8, 8, dtype=torch.uint8)
    m2[:4, 4:, :] = 0
    m2[4:, :4, :] = 0                                                     # four windows kept
    assert step.bound.aligned
    for i, bm in enumerate((m1, m2, m1, _unaligned())):
        n0 = len(calls)
        losses = step(xs if i == 0 else None, bm)
        torch.cuda.synchronize()
        with_block0 = len(calls) > n0
        gn = opt.norm.item()
        ref.zero_grad()
        want = ref(xs, block_mask=bm)
        want[0].backward()
        torch.cuda.synchronize()
        wn = ref._flat_grad.double().norm().item()
        assert abs(losses[0].item() - want[0].item()) <= 2e-5 * abs(want[0].item()), (i, losses[0].item(), want[0].item())
        assert abs(gn - wn) <= 5e-3 * wn, (i, gn, wn)
        assert step.bound.aligned == (i < 3)
        assert with_block0 == (i == 0)                                  # captured with the kept-window block once; the fall-back capture holds none
