"""The decoder tail over each sample's valid box alone (csrc/tail_box.hpp; csrc/norm.hip: tail_fwd_coarse_kernel<true>, tail_bwd_kernel with extents) against the
full walk of the same kernels: on a target that is zero outside the extents, d(pred) is exactly zero in the padding, so the box walk must give the same bytes
inside the box, leave everything outside it unwritten, and agree in every sum up to the order of the fp32 partials.

The bound on a sum is four times what two runs of the full walk differ by on the same inputs, relative to the tensor's largest entry, with a floor of 1e-6;
both are measured in the test and printed (pytest -s).  Measured on an MI355X over the six cases (also DESIGN.md 6.1), full against full | box against full:
loss sums <= 2.4e-8 | <= 4.1e-8, losses <= 6.8e-8 | <= 6.8e-8, bwd_sums <= 1.3e-9 | <= 2.6e-8 -- the fp32 partials meet in fp64 atomics, so every bound is the
floor.  Model level (swin_t, 32^3, two samples, bf16): the losses agree exactly, the gradients differ by 1.47e-3 with the switch on against off and by 1.43e-3
between two runs with it off (bf16 roundings that flip along the chain)."""
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests._metrics import relerr
from tests.test_kernels_gpu import TOL, check, dev, q, rnd

pytestmark = pytest.mark.gpu

Cd = 48
FLOOR = 1e-6


def _ops():
    from nerf_mae_amd import ops
    return ops


def _rel(a, b):
    """max |a - b| relative to the largest entry of b"""
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300)).item()


def _box_mask(ext, R):
    """[B, R, R, R] bool: the voxels of every coarse cell that meets the extents (ceil(e / 4) cells per axis)"""
    ax = torch.arange(R)
    m = [(ax[None, :, None, None] < 4 * ((e[0] + 3) // 4)) & (ax[None, None, :, None] < 4 * ((e[1] + 3) // 4)) & (ax[None, None, None, :] < 4 * ((e[2] + 3) // 4)) for e in ext]
    return torch.cat(m).cuda()


def _inputs(R, ext, seed=0):
    """a batch of the tail's inputs on the device; the target is zero outside each sample's extents (the box walk's precondition)"""
    from oracle import mae3d_oracle as O
    ops = _ops()
    dt, B, gd, V = torch.bfloat16, len(ext), R // 4, R ** 3
    x = torch.stack([O.synthetic_grid((R, R, R), 3 + seed + i) for i in range(B)])
    valid = torch.zeros_like(x)
    for i, e in enumerate(ext):
        valid[i, :, :e[0], :e[1], :e[2]] = 1
    x = x * valid
    y = q(rnd(B, V, Cd, seed=seed) * 1.3 + 0.2, dt)
    xc = q(rnd(B, gd, gd, gd, 96, seed=11 + seed), dt)
    Wt, bt = rnd(96, 48, 4, 4, 4, seed=12, scale=96 ** -0.5), rnd(48, seed=13, scale=0.5)
    Wo, bo = rnd(4, Cd, seed=1, scale=0.2), rnd(4, seed=2, scale=0.1)
    tm = O.draw_block_mask((gd,) * 3, 0.6, rng=random.Random(5))
    ws = torch.empty(ops.cconv_pack_ws_floats(), dtype=torch.float32, device="cuda")
    ops.cconv_pack(dev(Wt), dev(rnd(48, 48, 3, 3, 3, seed=3)), dev(bt), torch.empty(ops.cconv_pack_numel(), dtype=dt, device="cuda"), torch.empty(27, 48, device="cuda"), ws)
    Wres = torch.empty(ops.tail_residual_pack_numel(), dtype=dt, device="cuda")
    ops.tail_residual_pack(ws, Wres)
    yd = dev(y, dt).view(-1, Cd)
    stats = torch.empty(B, Cd, 2, device="cuda")
    ops.instnorm_stats(yd, stats, torch.empty(B, Cd, 2, dtype=torch.float64, device="cuda"), B, V, Cd)
    host = dict(x=x, valid=valid, y=y, xc=xc, Wt=Wt, bt=bt, Wo=Wo, bo=bo, tm=tm)
    return host, dict(y=yd, stats=stats, xc=dev(xc, dt), Wres=Wres, bt=dev(bt), Wo=dev(Wo), bo=dev(bo), x=dev(x), ext=dev(torch.tensor(ext, dtype=torch.int32)),
                      tm=dev(tm.to(torch.uint8)), B=B, R=R, V=V)


def _forward(d, box, pred=None):
    """one tail forward into sentinel-filled outputs: (loss sums, losses, d(pred), backward sums, sign mask)"""
    ops = _ops()
    B, R, V = d["B"], d["R"], d["V"]
    lsums, losses = torch.empty(8, dtype=torch.float64, device="cuda"), torch.empty(3, device="cuda")
    dpred = torch.full((B * V, 4), 7.0, device="cuda")
    bsum = torch.empty(B * Cd * 4 + 4 * Cd, dtype=torch.float64, device="cuda")
    smask = torch.full((B * V, 8), 0xAA, dtype=torch.uint8, device="cuda")
    ops.mae_tail_fwd_from_coarse(d["y"], d["stats"], d["xc"], d["Wres"], d["bt"], d["Wo"], d["bo"], d["x"], d["ext"], d["tm"], B, R, Cd, lsums, losses, dpred, bsum, smask,
                                 pred=pred, box=box)
    torch.cuda.synchronize()
    return lsums, losses, dpred, bsum, smask


def _backward(d, lsums, dpred, bsum, smask, box):
    ops = _ops()
    B, R, V = d["B"], d["R"], d["V"]
    dy, dr = torch.empty(B * V, Cd, dtype=torch.bfloat16, device="cuda"), torch.empty(B * V, Cd, dtype=torch.bfloat16, device="cuda")
    dW, db, in_sums = torch.zeros(4, Cd, device="cuda"), torch.zeros(4, device="cuda"), torch.empty(B, Cd, 2, dtype=torch.float64, device="cuda")
    kw = dict(extents=d["ext"], R=R) if box else {}
    ops.mae_tail_bwd(None, d["y"], d["stats"], dpred, lsums, d["Wo"], in_sums, dy, dr, dW, db, B, V, Cd, bwd_sums=bsum, sign_mask=smask, **kw)
    torch.cuda.synchronize()
    return dy, dr, dW, db, in_sums


def _extents_cases(R):
    return {"full+slab": [[R, R, R], [R - 4, R, R - 6]],                  # a full cube beside whole cells cut off two axes
            "ragged+7x8x5": [[R - 7, R - 13, R - 1], [26, 30, 18]],       # no axis a multiple of 4; 7 x 8 x 5 = 280 cells: a partial last step
            "one_cell+full": [[3, 2, 1], [R, R, R]]}                      # a box smaller than one step


@pytest.mark.parametrize("case", ["full+slab", "ragged+7x8x5", "one_cell+full"])
@pytest.mark.parametrize("R", [32, 48])
def test_box_walk_against_the_full_walk(R, case, monkeypatch):
    """R = 32: 8^3 cells; R = 48: 12^3 cells, rows of 12 against steps of 16.  Forward: the bytes of the box are the full walk's, nothing else is touched, the sums
    agree to four times the full walk's own run-to-run difference (floor 1e-6).  Backward: dy and dr equal everywhere, looping and streaming apply pass."""
    ext = _extents_cases(R)[case]
    _, d = _inputs(R, ext)
    B, V = d["B"], d["V"]
    ref, ref2, box = _forward(d, False), _forward(d, False), _forward(d, True)
    inside = _box_mask(ext, R).view(B * V)
    # the precondition, on the reference alone: d(pred) is exactly zero outside the box
    assert (ref[2][~inside] == 0).all()
    # inside: bit-identical d(pred) and sign bytes (6 of the 8-byte row are defined)
    assert torch.equal(box[2][inside].view(torch.int32), ref[2][inside].view(torch.int32))
    assert torch.equal(box[4][inside][:, :6], ref[4][inside][:, :6])
    # outside: the sentinels
    assert (box[2][~inside] == 7.0).all() and (box[4][~inside] == 0xAA).all()
    # losses, the eight loss sums, the backward sums: the order of fp32 partial sums alone
    for name, i in (("loss sums", 0), ("losses", 1), ("bwd_sums", 3)):
        noise, err = _rel(ref2[i], ref[i]), _rel(box[i], ref[i])
        print(f"R {R} {case}: {name}: full vs full {noise:.2e}, box vs full {err:.2e}")
        assert err <= max(4 * noise, FLOOR), (name, err, noise)
    # backward: the box pass on the box walk's d(pred) and sign mask, the full pass on the full walk's -- both behind the SAME in_sums, which the entry forms
    # from (loss sums, bwd_sums): the reference's are given to both
    for stream in (False, True):
        if stream:
            monkeypatch.setenv("NMH_IN_STREAM_MIN_MB", "0")
            monkeypatch.delenv("NMH_IN_STREAM", raising=False)
        gb = _backward(d, ref[0], box[2], ref[3], box[4], True)
        gr = _backward(d, ref[0], ref[2], ref[3], ref[4], False)
        assert torch.equal(gb[4], gr[4])
        assert torch.equal(gb[0], gr[0]) and torch.equal(gb[1], gr[1]), (stream, (gb[0] != gr[0]).sum().item(), (gb[1] != gr[1]).sum().item())
        assert (gb[1].view(B * V, Cd)[~inside] == 0).all()
        assert torch.equal(gb[2], gr[2]) and torch.equal(gb[3], gr[3])


def test_box_walk_against_fp32_autograd():
    """the chain of test_tail_forward_with_the_residual_formed_from_the_coarse_tensor at R = 32 with ragged extents, box walk forward and backward, its tolerances"""
    from oracle import mae3d_oracle as O
    R, ext, dt = 32, [[32, 32, 32], [25, 19, 31]], torch.bfloat16
    h, d = _inputs(R, ext, seed=4)
    B, V = d["B"], d["V"]
    yr, Wr, br_ = (t.clone().requires_grad_(True) for t in (h["y"], h["Wo"], h["bo"]))
    r_ref = F.conv_transpose3d(h["xc"].permute(0, 4, 1, 2, 3), q(h["Wt"], dt), h["bt"], stride=4).permute(0, 2, 3, 4, 1).reshape(B, V, Cd).clone().requires_grad_(True)
    inorm = lambda t: F.instance_norm(t.permute(0, 2, 1), eps=1e-5).permute(0, 2, 1)  # noqa: E731
    d0_ref = F.leaky_relu(inorm(yr) + r_ref, 0.01)
    d0s = d0_ref + (q(d0_ref.detach(), dt) - d0_ref).detach()
    pred = (d0s.reshape(B, R, R, R, Cd) @ Wr.T + br_).permute(0, 4, 1, 2, 3)
    l, lr, la, *_ = O.mae_loss(h["x"], pred, h["valid"], h["tm"][None, ..., None].expand(B, -1, -1, -1, 1))
    l.backward()
    lsums, losses, dpred, bsum, smask = _forward(d, True)
    np.testing.assert_allclose(losses.cpu().numpy(), [l.item(), lr.item(), la.item()], rtol=TOL[dt])
    dy, dr, dW, db, _ = _backward(d, lsums, dpred, bsum, smask, True)
    check(dr, r_ref.grad.reshape(-1, Cd), dt, "dr", 3)
    check(dy, yr.grad.reshape(-1, Cd), dt, "dy", 3)
    check(dW, Wr.grad, dt, "dWout", 2)
    check(db, br_.grad, dt, "dbout", 2)


def test_box_walk_refuses_pred():
    from nerf_mae_amd._lib import NmhError, lib
    _, d = _inputs(32, [[32, 32, 32], [30, 32, 27]])
    pred = torch.empty(2, 4, 32, 32, 32, device="cuda")
    with pytest.raises(ValueError):
        _forward(d, True, pred=pred)
    ops = _ops()
    lsums, losses, dpred = torch.empty(8, dtype=torch.float64, device="cuda"), torch.empty(3, device="cuda"), torch.empty(2 * 32 ** 3, 4, device="cuda")
    bsum, smask = torch.empty(2 * Cd * 4 + 4 * Cd, dtype=torch.float64, device="cuda"), torch.empty(2 * 32 ** 3, 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(NmhError):   # the entry itself: -4
        lib().call("nmh_mae_tail_fwd_from_coarse_box", ops.dt_of(d["y"]), d["y"], d["stats"], d["xc"], d["Wres"], d["bt"], d["Wo"], d["bo"], d["x"], d["ext"], d["tm"], 2, 32, Cd,
                   lsums, losses, pred, dpred, 0.01, bsum, smask, ops._st())


def test_model_with_and_without_the_box_walk(monkeypatch):
    """swin_t at 32^3, two samples, ragged extents: loss and gradients with ops.TAIL_BOX on against off, within four times what two runs with it off differ by"""
    from nerf_mae_amd import ops
    from oracle import mae3d_oracle as O
    from tests.test_model_gpu import SWIN_T, _pair
    _, hip = _pair(SWIN_T, torch.bfloat16, res=32, init="default")
    xs = [O.synthetic_grid((32, 32, 32), 61).cuda(), O.synthetic_grid((25, 19, 31), 62).cuda()]
    bm = O.draw_block_mask((8, 8, 8), 0.75, rng=random.Random(6))
    res = []
    for flag in (False, True, False):
        monkeypatch.setattr(ops, "TAIL_BOX", flag)
        hip.zero_grad()
        out = hip(xs, block_mask=bm)
        assert hip.decoder1._plan(2, 8, torch.bfloat16, True, (hip, None, None, None, None, True)).tail_box == flag   # (the path the forward just took)
        out[0].backward()
        torch.cuda.synchronize()
        res.append((torch.stack(out[:3]).detach().clone(), hip._flat_grad.clone()))
    for i, name in enumerate(("losses", "gradients")):
        noise, err = relerr(res[2][i], res[0][i]), relerr(res[1][i], res[0][i])
        print(f"model: {name}: off vs off {noise:.2e}, on vs off {err:.2e}")
        assert err <= max(4 * noise, FLOOR), (name, err, noise)
    assert torch.isfinite(res[1][1]).all()
    # asked for pred, or on a batch nobody vouches for, the plan keeps the full walk
    monkeypatch.setattr(ops, "TAIL_BOX", True)
    assert not hip.decoder1._plan(2, 8, torch.bfloat16, True, (hip, None, None, None, torch.empty(1), True)).tail_box
    assert not hip.decoder1._plan(2, 8, torch.bfloat16, True, (hip, None, None, None, None)).tail_box
