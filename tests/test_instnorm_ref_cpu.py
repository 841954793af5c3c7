"""Checks of tests/_instnorm_ref.py itself (no GPU): the float64 reference against float64 autograd, the derived bounds against an fp32 emulation of each
reduction's summation order on every hard input the GPU tests use, and the launch-geometry mirrors against values worked out by hand from csrc/norm.hip.

The emulation (per-thread strided voxels in fp32, the NV partials of a block in fp32, blocks in fp64) must stay under 1/4 of the bound: a correct kernel
then passes tests/test_instnorm_gpu.py before a GPU is involved.  The statistics are compared before their final store to fp32 (see emulate_stats).  An
input that fails here is the wrong input, not a reason to move the bound.  Worst emulated error over all cases: 0.03 of the bound on the mean, 0.06 on
rstd, 0.03 on the backward sums.

Measured with the emulation at C = 48, V = 4099 (fp32 inputs, stored to fp32, worst channel of its class):
  mean offset 20, sigma 0.5      relative rstd error 6e-8, mean error / sigma 1.9e-6 (the store of a mean of 20)
  first voxel at +30 sigma       relative rstd error 1.3e-5
  first voxel at +300 sigma      1.7e-4 -- too hard for a shifted fp32 sum of squares; not used."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _instnorm_ref as R


@pytest.mark.parametrize("rmode", [0, 1, 2])
def test_reference_chain_equals_float64_autograd(rmode):
    B, V, C = 2, 157, 24
    x, r, dout = R.chain_autograd_inputs(B, V, C, rmode)
    xr = x.clone().requires_grad_(True)
    rr = r.clone().requires_grad_(True) if rmode else None
    inorm = lambda t: F.instance_norm(t.permute(0, 2, 1), eps=R.EPS).permute(0, 2, 1)
    want = F.leaky_relu(inorm(xr) + (rr if rmode == 1 else inorm(rr) if rmode == 2 else 0), R.SLOPE)
    want.backward(dout)
    st = torch.stack(R.stats(x), -1)            # float64 statistics: the chain in exact arithmetic
    st_r = torch.stack(R.stats(r), -1) if rmode == 2 else None
    out, _ = R.apply(x, st, r, st_r, rmode)
    assert (out - want.detach()).abs().max() < 1e-12
    for src in ((out, None) if rmode == 0 else (out,)):      # rmode 0: the sign of x - mu stands in for a missing `out`
        s = R.bwd_sums(dout, src, x, st, r, st_r, rmode)
        o = R.bwd_apply(dout, src, x, st, s["S"], r, st_r, s["Sr"], rmode)
        assert (o["dx"] - xr.grad).abs().max() < 1e-12
        if rmode:
            assert (o["dr"] - rr.grad).abs().max() < 1e-12
    if rmode == 1:   # dr accumulates onto an initial dr
        dr0 = R.benign(B, V, C, torch.float64, 5)
        o = R.bwd_apply(dout, out, x, st, s["S"], r, st_r, None, 1, dr0=dr0)
        assert (o["dr"] - (rr.grad + dr0)).abs().max() < 1e-12


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("C", R.CS)
def test_shifted_reduction_emulated_in_fp32_stays_under_a_quarter_of_the_bound(C, dt):
    worst = [0.0, 0.0]
    for B, V in R.stats_cases(C):
        x = R.hard_input(B, V, C, dt)
        mu, rstd = R.stats(x)
        bm, br = R.stats_bounds(x, x[:, 0], R.reduce_chain(V, C))
        em, er = R.emulate_stats(x, C)
        worst[0] = max(worst[0], R.ratio_check(em, mu, bm, f"mean B{B} V{V} C{C}", frac=0.25))
        worst[1] = max(worst[1], R.ratio_check(er / rstd, torch.ones_like(rstd), br, f"rstd B{B} V{V} C{C}", frac=0.25))
        const = (torch.arange(C) % 5 == 3)
        em, er = R.emulate_stats(x, C, store32=True)    # a constant channel as stored: the mean exact, rstd = fp32(eps^-1/2)
        assert torch.equal(em[:, const], mu[:, const]) and bool((er[:, const] == float(np.float32(R.EPS ** -0.5))).all())
    print(f"C {C}: worst mean {worst[0]:.3g}, rstd {worst[1]:.3g} of the bound")


def test_documented_figures_of_the_shifted_reduction():
    """the three figures of the module docstring, and that the +300 sigma outlier is indeed an order harder than the +30 sigma one"""
    C, V = 48, 4099
    x = R.hard_input(1, V, C, torch.float32)
    cls = torch.arange(C) % 5
    mu, rstd = R.stats(x)
    em, er = R.emulate_stats(x, C, store32=True)
    rel = (er / rstd - 1).abs()[0]
    off_rstd, off_mean = float(rel[cls == 1].max()), float(((em - mu).abs() * rstd)[0][cls == 1].max())
    out30 = float(rel[cls == 2].max())
    x300 = x.clone()
    x300[:, 0, cls == 2] = (x300[:, 0, cls == 2] + 270.0).float().double()
    mu3, rstd3 = R.stats(x300)
    out300 = float((R.emulate_stats(x300, C, store32=True)[1] / rstd3 - 1).abs()[0][cls == 2].max())
    print(f"offset: rstd rel {off_rstd:.2e}, mean err / sigma {off_mean:.2e}; outlier 30 sigma {out30:.2e}; 300 sigma {out300:.2e}")
    assert off_rstd < 1e-6 and off_mean < 1e-5 and out30 < 2e-4 and out300 > 2 * out30


@pytest.mark.parametrize("rho", [0.0, 2.0, 8.0])
def test_unshifted_sums_emulated_in_fp32_stay_under_a_quarter_of_the_bound(rho):
    """the path of the conv epilogues (c = 0): one 256-voxel tile per fp32 chain (16 lanes x 16 steps stand in for the tile's order), tiles in fp64"""
    B, V, C = 2, 1024, 64
    x = R.benign(B, V, C, torch.bfloat16, 3, 1.0, rho)
    mu, rstd = R.stats(x)
    bm, br = R.stats_bounds(x, torch.zeros(B, C, dtype=torch.float64), 256)
    em, er = R.emulate_stats(x, C, shift_first=False, vpb=256, NV=16)
    R.ratio_check(em, mu, bm, f"mean rho {rho}", frac=0.25)
    R.ratio_check(er / rstd, torch.ones_like(rstd), br, f"rstd rho {rho}", frac=0.25)


@pytest.mark.parametrize("mode", R.BWD_REDUCE_MODES)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_sums_emulated_in_fp32_stay_under_a_quarter_of_the_bound(dt, mode):
    for C, V in R.BWD_REDUCE_SHAPES:
        for B in ((2, 5) if V > 1000 else R.BWD_REDUCE_BS):
            d = R.bwd_reduce_inputs(B, V, C, dt, mode)
            ref = R.bwd_sums(d["dout"], d["out"], d["x"], d["stats32"], d["r"], d["stats_r32"], d["rmode"])
            S, Sr = R.emulate_bwd_sums(d["dout"], d["out"], d["x"], d["stats32"], d["r"], d["stats_r32"], d["rmode"], B)
            L = R.reduce_chain(V, C, B)
            R.ratio_check(S, ref["S"], R.bwd_sums_bound(ref["A"], L), f"sums {mode} B{B} V{V} C{C}", frac=0.25)
            if d["rmode"] == 2:
                R.ratio_check(Sr, ref["Sr"], R.bwd_sums_bound(ref["Ar"], L), f"sums_r {mode} B{B} V{V} C{C}", frac=0.25)


def test_geometry_mirrors_against_hand_values():
    """values worked out by hand from csrc/norm.hip (in_vox_per_block, in_apply_vpb, NV = 256 / (C / 8), in_apply_streaming)"""
    assert [R.nv(C) for C in (8, 24, 40, 48, 96, 192, 384, 2048)] == [256, 85, 51, 42, 21, 10, 5, 1]
    for V, B, want in [(1, 4, 128), (129, 4, 128), (32768, 4, 128), (32769, 4, 192), (4096000, 4, 16000), (4096000, 8, 16000), (4096000, 1, 4032),
                       (4096000, 2, 8000), (4096000, 3, 12032), (33000, 2, 128), (33000, 5, 192), (64000, 1, 128)]:
        assert R.in_vox_per_block(V, B) == want, (V, B)
    for V, B, C, want in [(41, 1, 48, 168), (1000, 2, 48, 168), (4096000, 1, 48, 2048), (262144, 2, 48, 512), (64000, 2, 96, 125), (8000, 2, 192, 40),
                          (300, 1, 2048, 4), (5000, 3, 8, 1024), (1000, 1, 384, 20)]:
        assert R.in_apply_vpb(V, B, C) == want, (V, B, C)
    assert R.in_apply_vpb(10 ** 6, 1, 48, streaming=True, mult=4) == 168 and R.in_apply_vpb(10 ** 6, 1, 96, streaming=True) == 168
    assert R.in_apply_vpb(10 ** 6, 1, 8, streaming=True, mult=16) == 4096 and R.in_apply_vpb(10 ** 6, 1, 48, streaming=True, env_vpb=77) == 77
    assert R.apply_streaming(160 ** 3, 1, 48, True) and not R.apply_streaming(146 ** 3, 1, 48, True)        # 393 MB / 299 MB
    assert not R.apply_streaming(160 ** 3, 1, 48, False) and not R.apply_streaming(160 ** 3, 1, 192, True)   # fp32; wider than the LDS table
    assert R.apply_streaming(10, 1, 96, True, min_mb=0.0) and not R.apply_streaming(160 ** 3, 1, 48, True, on=0)
    assert R.reduce_chain(4099, 48) == 4 + 42 and R.reduce_chain(1, 8) == 1 + 256 and R.reduce_chain(300, 2048) == 128 + 1
    assert R.c_supported(2048) and not R.c_supported(12) and not R.c_supported(2056)
