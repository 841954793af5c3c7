"""GPU, decoder1 in the centered form (include/nerfmae_hip.h above nmh_cconv_pack_centered): conv1 stores z = lrelu(y1 - mean), the per-sample
rstd is folded into conv2's weights, the backward reads z.  Each of the five launches that only exist for this form against a float64 reference written from
the definition of the operation, on inputs built so that a mixed-up sample or a wrong constant is an O(1) error:
  * rstd spans four decades across samples (RSTD_B) and a factor 4 across channels; z = bf16(lrelu(t)) with t ~ N(0, 1 / rstd^2), so rstd * z is O(1) in
    every sample, holds both signs and exact zeros; the reference recovers t = z > 0 ? z : z / slope, as the kernels define it;
  * the residual mean e = stats1[..., 0] is +-0.3 sigma with a sign per channel (in a real model it is ~2e-5 sigma: a wrong e term would be invisible);
  * outputs and fp64 accumulators start as garbage (the entries zero them), dW starts nonzero (the reduce accumulates);
  * ragged 4x8x16 forward tiles and 4x4x16 weight-gradient tiles, B in {1, 3, 8} / {1, 2, 4, 8}, both launch regimes of the persistent kernels.
Then the domain of the scaled weight gradient (and that the model's gate never sends it a shape it refuses), the whole chain at small sizes against float64
autograd of the true block (unetr_block.py:57-62), and the launches at the benched shape (B = 8, 160^3: sample 7 lies past 2^31 bytes).
Tolerance comments cite the errors measured on the MI355X (NMH_PRINT_ERR=1)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests.test_kernels_gpu import TOL, _pack_via_kernel, check, dev, q, rnd

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SLOPE = 0.01
RSTD_B = [0.01, 0.1, 1.0, 10.0, 100.0, 0.3, 3.0, 30.0]   # per-sample rstd: a sample that reads another's scale is off by >= 3x


def _ops():
    from nerf_mae_amd import ops
    return ops


def _nmh_error():
    from nerf_mae_amd._lib import NmhError
    return NmhError


def _stats1(B, seed=0, e_sigma=0.3):
    """(e, rstd) pairs [B,48,2] fp32 as conv1's instnorm_finalize leaves them: rstd = RSTD_B[b] x 2^U(-1,1) per channel, e = +-e_sigma / rstd (sign per channel)"""
    g = torch.Generator().manual_seed(4242 + seed)
    rs = torch.tensor([RSTD_B[b % 8] for b in range(B)])[:, None] * torch.exp2(torch.rand(B, 48, generator=g) * 2 - 1)
    sign = torch.where(torch.rand(48, generator=g) < 0.5, -1.0, 1.0)
    e = e_sigma * sign * (0.5 + torch.rand(B, 48, generator=g)) / rs
    return torch.stack([e, rs], -1).float().contiguous()


def _z(B, D, H, W, rs, seed=0):
    """z = bf16(lrelu(t)), t ~ N(0, 1 / rstd[b, c]^2), ~3 % exact zeros (host fp32 holding bf16 values)"""
    t = rnd(B, D, H, W, 48, seed=seed) / rs[:, None, None, None, :]
    z = q(F.leaky_relu(t, SLOPE), BF)
    zero = torch.rand(B, D, H, W, 48, generator=torch.Generator().manual_seed(seed + 7)) < 0.03
    return z.masked_fill(zero, 0.0)


def _t(z):
    """t = y1 - mean recovered from z the way the kernels define it (float64)"""
    z = z.double()
    return torch.where(z > 0, z, z / SLOPE)


def _conv_ref(z, W, rs):
    """float64 conv2 of each sample with its own weights W[co][ci] * rs[b, ci]: z [B,D,H,W,48] -> [B,D,H,W,48]"""
    out = []
    for b in range(z.shape[0]):
        wb = W.double() * rs[b].double().view(1, 48, 1, 1, 1)
        out.append(F.conv3d(z[b:b + 1].double().permute(0, 4, 1, 2, 3), wb, padding=1).permute(0, 2, 3, 4, 1))
    return torch.cat(out)


def _wgrad_ref(dy, z, rs):
    """float64 sum_b rs[b, ci] sum_v dy_b[v, co] z_b[v + tap, ci] and the same sum over |terms| ([48,48,3,3,3] each)"""
    zs = (z.double() * rs.double()[:, None, None, None, :]).permute(0, 4, 1, 2, 3)
    d = dy.double().permute(0, 4, 1, 2, 3)
    ref = torch.nn.grad.conv3d_weight(zs, (48, 48, 3, 3, 3), d, padding=1)
    mag = torch.nn.grad.conv3d_weight(zs.abs(), (48, 48, 3, 3, 3), d.abs(), padding=1)
    return ref, mag


def _c48_workgroup_samples(B, D, H, W):
    """the largest number of samples one workgroup of conv48_kernel walks (csrc/conv48.hip: 4x8x16 tiles in sample-major order, nb = 256 or the tile count
    rounded up to 8, XCD x owns the contiguous range [x per, (x + 1) per), per = ceil(tiles / 8); workgroup 8 j + x walks it from j with stride nb / 8).
    A workgroup that moves to another sample flushes its statistics accumulators and loads the next sample's weight image for the next tile"""
    tps = math.ceil(D / 4) * math.ceil(H / 8) * math.ceil(W / 16)
    total = B * tps
    nb = (total + 7) // 8 * 8 if total < 256 else 256
    per, js = (total + 7) // 8, nb // 8
    return max(len({t // tps for t in range(x * per + j, min(x * per + per, total), js)}) for x in range(8) for j in range(js))


def _print_err(name, err):
    import os
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  [{name}] {err:.2e}")


# ------------------------------------------------------------------------------------------------
# 1. one test per entry, small shapes
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 8])
def test_conv48_pack_scaled_is_the_mode6_pack_of_the_scaled_weights(B):
    """nmh_conv48_pack_scaled: image b == the forward fragment pack (mode 6) of W[co][ci][tap] * rstd[b][ci], bit for bit (the same fp32 product, the same
    round-to-nearest-even bf16 conversion), zero pads included; nothing past B images is written"""
    ops = _ops()
    W = rnd(48, 48, 3, 3, 3, seed=11, scale=(27 * 48) ** -0.5)
    st = _stats1(B, seed=B)
    pad = 4096
    out = torch.full((B * ops.C48_IMG + pad,), float("nan"), dtype=BF, device="cuda")
    out[B * ops.C48_IMG:] = 5.0
    ops.conv48_pack_scaled(dev(W), dev(st), out, B)
    torch.cuda.synchronize()
    for b in range(B):
        ref = _pack_via_kernel(W * st[b, :, 1].view(1, 48, 1, 1, 1), 6, BF, ops.C48_IMG)
        img = out[b * ops.C48_IMG:(b + 1) * ops.C48_IMG]
        assert torch.equal(img.view(torch.int16), ref.view(torch.int16)), f"image {b}"
    assert torch.equal(out[B * ops.C48_IMG:].float().cpu(), torch.full((pad,), 5.0)), "wrote past B images"


@pytest.mark.parametrize("B,D,H,W,nsamp", [(1, 7, 9, 19, 1), (3, 6, 10, 20, 1), (8, 11, 23, 61, 1), (3, 23, 31, 61, 2)],
                         ids=["b1_ragged", "b3_one_tile_per_workgroup", "b8_288_tiles_one_sample_per_xcd", "b3_288_tiles_workgroups_cross_samples"])
def test_conv48_per_sample_forward_against_fp64(B, D, H, W, nsamp):
    """nmh_conv3d_k3_c48_per_sample (conv2 forward): every tile reads the weight image of its own sample.  (8, 11, 23, 61): 288 ragged tiles on 256
    workgroups, but each XCD range is exactly one sample; (3, 23, 31, 61): 96 ragged tiles per sample, 288 in all, so XCD 2's range [72, 108) holds the
    boundary at tile 96 and workgroups walk tiles of two samples: the switch of the weight image for the next tile and the statistics flush on the
    sample change run (nsamp: the most samples one workgroup walks, from the tile schedule)"""
    assert _c48_workgroup_samples(B, D, H, W) == nsamp
    ops = _ops()
    Wm = rnd(48, 48, 3, 3, 3, seed=21, scale=(27 * 48) ** -0.5)
    st = _stats1(B, seed=10 + B)
    rs = st[..., 1]
    z = _z(B, D, H, W, rs, seed=B)
    wk = torch.empty(B * ops.C48_IMG, dtype=BF, device="cuda")
    ops.conv48_pack_scaled(dev(Wm), dev(st), wk, B)
    zd = dev(z, BF)
    out = torch.full((B, D, H, W, 48), float("nan"), dtype=BF, device="cuda")
    acc = torch.full((B, 48, 2), 5.0, dtype=torch.float64, device="cuda")   # zeroed by the entry
    y = ops.conv3d_k3_c48_per_sample(zd, wk, out=out, stats_acc=acc)
    torch.cuda.synchronize()
    ref = _conv_ref(z, Wm, rs)
    # bf16 weights W * rstd and bf16 outputs against fp64 weights: measured max-norm <= 3.8e-3 per sample
    for b in range(B):
        check(y[b], ref[b], BF, f"per-sample conv b={b}")
    # fused statistics == fp64 statistics of the stored output; fp32 per-workgroup partials: relative to sum |y| / sum y^2, measured <= 1.0e-7
    yd = y.double().cpu().reshape(B, -1, 48)
    for k, (val, mag) in enumerate(((yd.sum(1), yd.abs().sum(1)), ((yd * yd).sum(1), (yd * yd).sum(1)))):
        err = ((acc[..., k].cpu() - val).abs() / mag).max().item()
        _print_err(f"per-sample fused stats k={k}", err)
        assert err < 1e-6, (k, err)
    # without statistics: the same output, bit for bit
    y2 = ops.conv3d_k3_c48_per_sample(zd, wk)
    assert torch.equal(y2, y)
    # one rstd for every sample: bit-identical to the single-image kernel
    st1 = st.clone()
    st1[..., 1] = st[0, :, 1]
    wk1 = torch.empty(B * ops.C48_IMG, dtype=BF, device="cuda")
    ops.conv48_pack_scaled(dev(Wm), dev(st1), wk1, B)
    y3 = ops.conv3d_k3_c48_per_sample(zd, wk1)
    y4 = ops.conv3d_k3_c48(zd, wk1[:ops.C48_IMG])
    torch.cuda.synchronize()
    assert torch.equal(y3, y4)


@pytest.mark.parametrize("B,D,H,W,dc,nsamp", [(1, 7, 9, 19, 0.0, 1), (2, 20, 24, 40, 0.0, 1), (8, 11, 23, 61, 0.0, 1), (3, 9, 17, 33, 2.0, 1),
                                               (3, 24, 32, 64, 0.0, 2), (3, 23, 31, 61, 2.0, 2)],
                         ids=["b1_ragged", "b2_sample_spans_workgroups", "b8_288_tiles_one_sample_per_xcd", "b3_e_sum_g_dominates",
                              "b3_288_tiles_workgroups_cross_samples", "b3_ragged_cross_samples_e_sum_g_dominates"])
def test_conv48_bwd_reduce_centered_against_fp64(B, D, H, W, dc, nsamp):
    """nmh_conv3d_k3_c48_bwd_reduce_centered (conv2's input gradient reading z): dX == the plain dgrad bit for bit, and the InstanceNorm-backward sums
    sum g and sum g (t - e) rstd, g = dX lrelu'(t), against float64.  Cases with dc have a per-channel DC in dY and e = +-5 sigma, so that e sum g is
    several times sum dX z (in most channels): the flush's `- e sum g` term carries the result.  The last two have 96 tiles per sample and 288 in all:
    workgroups of XCD 2 walk tiles of two samples, so the flush with the e correction runs on a sample change, not only at the end (nsamp: the most
    samples one workgroup walks, from the tile schedule)"""
    assert _c48_workgroup_samples(B, D, H, W) == nsamp
    ops = _ops()
    Wm = rnd(48, 48, 3, 3, 3, seed=31, scale=(27 * 48) ** -0.5)
    wkd = _pack_via_kernel(Wm, 7, BF, ops.C48_IMG)
    st = _stats1(B, seed=20 + B, e_sigma=5.0 if dc else 0.3)
    rs, e = st[..., 1].double(), st[..., 0].double()
    z = _z(B, D, H, W, st[..., 1], seed=B + 3)
    dy = q(rnd(B, D, H, W, 48, seed=32) + dc * rnd(1, 1, 1, 1, 48, seed=33).sign(), BF)
    dyd, zd = dev(dy, BF), dev(z, BF)
    sums = torch.full((B, 48, 2), 5.0, dtype=torch.float64, device="cuda")     # zeroed by the entry
    dx = ops.conv3d_k3_c48_bwd_reduce_centered(dyd, wkd, zd, dev(st), sums, out=torch.full_like(dyd, float("nan")), slope=SLOPE)
    ref_dx = ops.conv3d_k3_c48(dyd, wkd)
    torch.cuda.synchronize()
    assert torch.equal(dx, ref_dx)
    d, t = dx.double().cpu(), _t(z)
    g = d * torch.where(t > 0, 1.0, SLOPE)
    ref = torch.stack([g.sum(dim=(1, 2, 3)), (g * (t - e[:, None, None, None, :]) * rs[:, None, None, None, :]).sum(dim=(1, 2, 3))], -1)
    if dc:
        dz = (d * z.double()).sum(dim=(1, 2, 3)) * rs
        esg = e * ref[..., 0] * rs
        assert (esg.abs() > 2 * dz.abs()).float().mean() > 0.5, "the case does not exercise the e term"
    # the scale normalisation of test_conv48_input_gradient_with_fused_instnorm_backward_sums: relative to sum |dX| per (sample, channel)
    # (rstd (t - e) is O(1)); measured <= 2.2e-8 (k = 0), 1.2e-7 (k = 1, in the e-dominated case)
    scale = d.abs().sum(dim=(1, 2, 3))
    for k in range(2):
        err = ((sums[..., k].cpu() - ref[..., k]).abs() / scale).max().item()
        _print_err(f"bwd_reduce_centered sums k={k}", err)
        assert err < 1e-6, (k, err)


@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("V", [41, 1500])
def test_instnorm_bwd_apply_bg_centered_against_fp64(B, V):
    """nmh_instnorm_bwd_apply_bg_centered: dx = rstd (g - m1 - (t - e) rstd m2), g = d lrelu'(t), m = sums / V, per element.  wps = 256 / B workgroups per
    sample split V unevenly (41 voxels: most workgroups of a sample have none)"""
    ops = _ops()
    st = _stats1(B, seed=30 + B)
    rs, e = st[..., 1].double(), st[..., 0].double()
    z = _z(B, 1, 1, V, st[..., 1], seed=V + B).reshape(B * V, 48)
    d = q(rnd(B * V, 48, seed=41), BF)
    g = torch.Generator().manual_seed(43)
    sums = torch.stack([0.5 * torch.randn(B, 48, generator=g), 0.5 * torch.randn(B, 48, generator=g)], -1).double() * V
    dx = torch.full((B * V, 48), float("nan"), dtype=BF, device="cuda")
    ops.instnorm_bwd_apply_bg_centered(dev(d, BF), dev(z, BF), dev(st), dev(sums), dx, B, V, 48, slope=SLOPE)
    torch.cuda.synchronize()
    m1, m2 = (sums / V).unbind(-1)
    t = _t(z).view(B, V, 48)
    gg = d.double().view(B, V, 48) * torch.where(t > 0, 1.0, SLOPE)
    r, e_, m1, m2 = rs[:, None, :], e[:, None, :], m1[:, None, :], m2[:, None, :]
    ref = r * (gg - m1 - (t - e_) * r * m2)
    # bound: one bf16 rounding of the result (half an ulp <= 2^-8 |dx|) + the fp32 rounding of the per-channel constants and the two FMAs, a few 2^-24 of
    # the magnitudes that enter them; measured worst |dx - ref| / bound 0.995 (the rounding alone reaches 2^-8 |dx| just above a power of two)
    mag = (r * gg).abs() + (r * m1).abs() + (r * r * m2 * t).abs() + (r * r * m2 * e_).abs()
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -19 * mag
    worst = ((dx.double().cpu().view(B, V, 48) - ref).abs() / bound).max().item()
    _print_err(f"apply_bg_centered B={B} V={V} / bound", worst)
    assert worst <= 1.0, worst


@pytest.mark.parametrize("B,D,H,W", [(8, 3, 4, 13), (1, 7, 6, 30), (2, 4, 7, 20), (4, 5, 6, 16), (2, 32, 32, 64), (4, 20, 18, 50), (1, 28, 30, 70),
                                     (8, 16, 16, 48)],
                         ids=["b8_one_tile_per_sample", "b1_eight_tiles", "b2_ragged", "b4_ragged", "b2_512_tiles", "b4_400_tiles_ragged", "b1_280_tiles_ragged",
                              "b8_384_tiles"])
def test_conv48_wgrad_scaled_against_fp64(B, D, H, W):
    """nmh_conv3d_k3_c48_wgrad_scaled (conv2's weight gradient on (dY, z)): += sum_b rstd[b, ci] sum_v dY_b[v, co] z_b[v + tap, ci].  The first four cases
    have fewer than 256 tiles (one tile per workgroup; B = 8 with one tile per sample and B = 1 with 8 tiles are the smallest valid counts), the others more
    (256 workgroups each walk several tiles, unroll slot u of the reduce = sample (u B) >> 3)"""
    ops = _ops()
    st = _stats1(B, seed=50 + B)
    rs = st[..., 1]
    z = _z(B, D, H, W, rs, seed=D + B)
    dy = q(rnd(B, D, H, W, 48, seed=51), BF)
    dW0 = rnd(48, 48, 3, 3, 3, seed=52, scale=10.0)
    dW = dev(dW0)
    ops.conv3d_k3_c48_wgrad_scaled(dev(dy, BF), dev(z, BF), dev(st), dW)
    torch.cuda.synchronize()
    ref, mag = _wgrad_ref(dy, z, rs)
    # bf16 products are exact in fp32: fp32 summation order only, relative to sum |terms| (+ the fp32 rounding of dW0 + ...): measured <= 5.6e-8
    err = ((dW.double().cpu() - dW0.double() - ref).abs() / (mag + dW0.double().abs() + 1e-30)).max().item()
    _print_err(f"wgrad_scaled B={B} {D}x{H}x{W}", err)
    assert err < 1e-6, err
    check(dW - dev(dW0), ref, torch.float32, "wgrad_scaled")


# ------------------------------------------------------------------------------------------------
# 2. domain and refusal
# ------------------------------------------------------------------------------------------------
def _tps(D, H, W):
    return math.ceil(D / 4) * math.ceil(H / 4) * math.ceil(W / 16)


@pytest.mark.parametrize("B,D,H,W", [(3, 4, 4, 16), (5, 4, 4, 16), (6, 4, 8, 16), (7, 4, 4, 16), (16, 4, 4, 16), (2, 4, 4, 48), (4, 4, 4, 16), (4, 12, 4, 16),
                                     (2, 4, 12, 16)])
def test_conv48_wgrad_scaled_refuses_split_samples(B, D, H, W):
    """B outside {1, 2, 4, 8}, or tiles per sample not a multiple of 8 / B: some XCD tile range would straddle two samples -> NmhError, dW untouched"""
    ops = _ops()
    assert 8 % B or _tps(D, H, W) % (8 // B)
    dy = dev(q(rnd(B, D, H, W, 48, seed=61), BF), BF)
    z = dev(q(rnd(B, D, H, W, 48, seed=62), BF), BF)
    st = dev(_stats1(B))
    dW = dev(rnd(48, 48, 3, 3, 3, seed=63))
    dW0 = dW.clone()
    with pytest.raises(_nmh_error()):
        ops.conv3d_k3_c48_wgrad_scaled(dy, z, st, dW)
    torch.cuda.synchronize()
    assert torch.equal(dW, dW0)


def test_centered_entries_refuse_slopes_outside_their_domain():
    """conv3d_k3_c48_bwd_reduce_centered needs 0 < slope < 1 (t = z / slope for z <= 0), instnorm_bwd_apply_bg_centered slope > 0"""
    ops = _ops()
    B, D, H, W = 1, 4, 8, 16
    wkd = _pack_via_kernel(rnd(48, 48, 3, 3, 3, seed=71), 7, BF, ops.C48_IMG)
    dy = dev(q(rnd(B, D, H, W, 48, seed=72), BF), BF)
    z = dev(q(rnd(B, D, H, W, 48, seed=73), BF), BF)
    st = dev(_stats1(B))
    sums = torch.zeros(B, 48, 2, dtype=torch.float64, device="cuda")
    for s in (0.0, -0.01, 1.0, 1.5, float("nan")):
        with pytest.raises(_nmh_error()):
            ops.conv3d_k3_c48_bwd_reduce_centered(dy, wkd, z, st, sums, slope=s)
    ops.conv3d_k3_c48_bwd_reduce_centered(dy, wkd, z, st, sums, slope=0.2)
    V = D * H * W
    dx = torch.empty(B * V, 48, dtype=BF, device="cuda")
    for s in (0.0, -0.01, float("nan")):
        with pytest.raises(_nmh_error()):
            ops.instnorm_bwd_apply_bg_centered(dy.view(-1, 48), z.view(-1, 48), st, sums, dx, B, V, 48, slope=s)
    ops.instnorm_bwd_apply_bg_centered(dy.view(-1, 48), z.view(-1, 48), st, sums, dx, B, V, 48, slope=2.0)
    torch.cuda.synchronize()


def test_model_gate_never_sends_wgrad_scaled_a_shape_it_refuses():
    """For cubes S in {32, ..., 160} and B in 1..9 the entry accepts exactly the (B, S) that pass the weight-gradient part of the cz gate in model.py, so the
    centered form can never fail in the middle of a backward pass (inputs are zeros: the accepted launches add 0 to dW)"""
    from nerf_mae_amd.model import centered_wgrad_ok
    ops = _ops()
    assert centered_wgrad_ok(8, 160) and centered_wgrad_ok(2, 64)   # the benched shape and the agreement test's take the centered form
    Smax, Bmax = 160, 9
    buf_dy = torch.zeros(Bmax * Smax ** 3 * 48, dtype=BF, device="cuda")
    buf_z = torch.zeros_like(buf_dy)
    st = dev(_stats1(Bmax))
    dW = torch.zeros(48, 48, 3, 3, 3, device="cuda")
    bad = []
    for S in (32, 48, 64, 96, 128, 160):
        n = S ** 3 * 48
        for B in range(1, Bmax + 1):
            gate = centered_wgrad_ok(B, S)   # the weight-gradient part of the cz gate, as the model evaluates it
            try:
                ops.conv3d_k3_c48_wgrad_scaled(buf_dy[:B * n].view(B, S, S, S, 48), buf_z[:B * n].view(B, S, S, S, 48), st[:B].contiguous(), dW)
                accepted = True
            except _nmh_error():
                accepted = False
            if accepted != gate:
                bad.append((B, S, gate, accepted))
    torch.cuda.synchronize()
    assert not bad, bad
    assert not dW.any()


# ------------------------------------------------------------------------------------------------
# 3. the chain at small sizes against float64 autograd of the true block
# ------------------------------------------------------------------------------------------------
CHAIN = {   # name -> (B, v, per-sample input scale, per-channel DC of the coarse input in sigma)
    "b1": (1, 8, None, 0.0),
    "b2": (2, 8, None, 0.0),
    "b4": (4, 8, None, 0.0),
    "b8": (8, 8, None, 0.0),
    "b2_v16": (2, 16, None, 0.0),
    "b4_scaled_1e2": (4, 8, [1.0, 100.0, 0.01, 10.0], 0.0),
    "b2_dc_30_sigma": (2, 8, None, 30.0),
}


@pytest.mark.parametrize("case", list(CHAIN))
def test_centered_chain_against_fp64_autograd_of_the_block(case):
    """decoder1's conv block exactly as model.py runs it when cz holds (pack + mean table, mean from the coarse tensor, centered conv1, finalize, scaled pack,
    per-sample conv2 + statistics, then for a random dy2: fused input gradient + sums, background InstanceNorm backward, scaled weight gradient) against CPU
    float64 autograd of conv_transpose3d -> conv3d -> instance_norm -> leaky_relu -> conv3d on the same bf16 x / dy2 and the fp32 master weights"""
    ops = _ops()
    B, v, scales, dc = CHAIN[case]
    S = 4 * v
    V = S ** 3
    x = rnd(B, v, v, v, 96, seed=81)
    if scales is not None:
        x = x * torch.tensor(scales).view(B, 1, 1, 1, 1)
    if dc:
        x = x + dc * rnd(1, 1, 1, 1, 96, seed=82).sign()
    x = q(x, BF)
    Wt = rnd(96, 48, 4, 4, 4, seed=83, scale=96 ** -0.5)
    W1 = rnd(48, 48, 3, 3, 3, seed=84, scale=(27 * 48) ** -0.5)
    bt = rnd(48, seed=85, scale=0.5)
    W2 = rnd(48, 48, 3, 3, 3, seed=86, scale=(27 * 48) ** -0.5)
    dy2 = q(rnd(B, S, S, S, 48, seed=87), BF)

    # --- the HIP chain (model.py, _Decoder1Fn with cz)
    Wcp = torch.empty(ops.cconv_pack_numel(), dtype=BF, device="cuda")
    delta = torch.empty(27, 48, device="cuda")
    ws = torch.empty(ops.cconv_pack_ws_floats(), device="cuda")
    mtab = torch.empty(27, 96, 48, device="cuda")
    ops.cconv_pack_centered(dev(Wt), dev(W1), dev(bt), Wcp, delta, ws, mtab)
    xd = dev(x, BF)
    mhat = ops.cconv_output_mean(xd, mtab, delta, B, v)
    acc1 = torch.full((B, 48, 2), 5.0, dtype=torch.float64, device="cuda")
    z = ops.cconv_fwd_centered(xd, Wcp, delta, mhat, B, v, stats_acc=acc1)
    st1 = torch.empty(B, 48, 2, device="cuda")
    ops.instnorm_finalize(acc1, st1, B, V, 48)
    wk2 = torch.empty(B * ops.C48_IMG, dtype=BF, device="cuda")
    ops.conv48_pack_scaled(dev(W2), st1, wk2, B)
    acc2 = torch.full((B, 48, 2), 5.0, dtype=torch.float64, device="cuda")
    y2 = ops.conv3d_k3_c48_per_sample(z, wk2, stats_acc=acc2)
    st2 = torch.empty(B, 48, 2, device="cuda")
    ops.instnorm_finalize(acc2, st2, B, V, 48)
    wkd = _pack_via_kernel(W2, 7, BF, ops.C48_IMG)
    dy2d = dev(dy2, BF)
    sums1 = torch.full((B, 48, 2), 5.0, dtype=torch.float64, device="cuda")
    da1 = ops.conv3d_k3_c48_bwd_reduce_centered(dy2d, wkd, z, st1, sums1)
    dy1 = torch.full((B * V, 48), float("nan"), dtype=BF, device="cuda")
    ops.instnorm_bwd_apply_bg_centered(da1.view(B * V, 48), z.view(B * V, 48), st1, sums1, dy1, B, V, 48)
    dW2 = torch.zeros(48, 48, 3, 3, 3, device="cuda")
    ops.conv3d_k3_c48_wgrad_scaled(dy2d, z, st1, dW2)
    torch.cuda.synchronize()

    # --- float64 autograd of the reference block (unetr_block.py:57-62)
    u = F.conv_transpose3d(x.double().permute(0, 4, 1, 2, 3), Wt.double(), bt.double(), stride=4)
    y1r = F.conv3d(u, W1.double(), padding=1).detach().requires_grad_(True)
    W2r = W2.double().requires_grad_(True)
    a1 = F.leaky_relu(F.instance_norm(y1r, eps=1e-5), SLOPE)
    y2r = F.conv3d(a1, W2r, padding=1)
    y2r.backward(dy2.double().permute(0, 4, 1, 2, 3))
    y2ref = y2r.detach().permute(0, 2, 3, 4, 1)
    dy1ref = y1r.grad.permute(0, 2, 3, 4, 1).reshape(B, V, 48)

    # y2 per sample (the InstanceNorm makes the samples comparable whatever their input scale); measured max-norm <= 4.8e-3
    for b in range(B):
        check(y2[b], y2ref[b], BF, f"{case} y2 b={b}")
    # statistics of y2: rstd relative, mean in units of sigma; measured <= 9.2e-4 / 3.9e-3
    yr = y2ref.reshape(B, V, 48)
    mean_r, rstd_r = yr.mean(1), (yr.var(1, unbiased=False) + 1e-5).rsqrt()
    st2c = st2.double().cpu()
    err_mean = ((st2c[..., 0] - mean_r).abs() * rstd_r).max().item()
    _print_err(f"{case} y2 mean / sigma", err_mean)
    assert err_mean < TOL[BF], err_mean
    check(st2c[..., 1], rstd_r, BF, f"{case} y2 rstd")
    # dL/dy1 per sample (it scales with 1 / the input scale).  At the LeakyReLU kink the kernels take lrelu'(t) from the sign of z, the sign of conv1's output
    # computed with bf16 composed weights; where that differs from the sign of the fp64 reference, the two gradients differ by rstd dL/da1 (1 - slope), an O(1)
    # error that no tolerance on the whole tensor can absorb (measured on the unmasked tensor: max-norm 0.77, rel-L2 3.3e-2).  Those elements are compared
    # separately: they must be few and all next to the kink (|xhat| < 2e-2: measured <= 6.0e-3; fraction < 2e-3: measured <= 5.3e-4), and the rest is held to TOL[bf16]
    xh = F.instance_norm(y1r.detach(), eps=1e-5).permute(0, 2, 3, 4, 1).reshape(B, V, 48)
    flip = (z.view(B, V, 48) > 0).cpu() != (xh > 0)
    frac, near = flip.double().mean().item(), (xh[flip].abs().max().item() if flip.any() else 0.0)
    _print_err(f"{case} kink sign flips: fraction", frac)
    _print_err(f"{case} kink sign flips: max |xhat|", near)
    assert frac < 2e-3 and near < 2e-2, (frac, near)
    dy1c = dy1.view(B, V, 48).float().cpu()
    for b in range(B):
        keep = ~flip[b]
        check(dy1c[b][keep], dy1ref[b][keep], BF, f"{case} dL/dy1 b={b} (off the kink)")   # measured max-norm <= 6.0e-3
    check(dW2, W2r.grad, BF, f"{case} dW2")   # measured max-norm <= 2.6e-3


# ------------------------------------------------------------------------------------------------
# 4. the benched shape: B = 8, 160^3 (v = 40); data made on the GPU, float64 references per sample
# ------------------------------------------------------------------------------------------------
SB, SS = 8, 160


def _gen():
    return torch.Generator(device="cuda").manual_seed(160)


def _z_gpu(rs, gen, seed_shift=0):
    """[8,160,160,160,48] bf16 z = lrelu(t), t ~ N(0, 1 / rstd^2), ~3 % exact zeros, one sample at a time"""
    z = torch.empty(SB, SS, SS, SS, 48, dtype=BF, device="cuda")
    for b in range(SB):
        t = torch.randn(SS, SS, SS, 48, generator=gen, device="cuda").div_(rs[b])
        zero = torch.rand(SS, SS, SS, 48, generator=gen, device="cuda") < 0.03
        z[b] = F.leaky_relu(t, SLOPE).masked_fill_(zero, 0.0).to(BF)
        del t, zero
    return z


def _randn_bf16_gpu(gen, scale=1.0):
    out = torch.empty(SB, SS, SS, SS, 48, dtype=BF, device="cuda")
    for b in range(SB):
        out[b] = (torch.randn(SS, SS, SS, 48, generator=gen, device="cuda") * scale).to(BF)
    return out


def _voxels(gen):
    """4096 voxels of one 160^3 sample: every corner and the tile seams (a product grid of z = 0, 3 mod 4, y = 0, 7 mod 8, x = 0, 15 mod 16 near both faces and
    the middle: 512), random voxels on the six faces (1024), random seam voxels (1536), random interior voxels (1024)"""
    zs = torch.tensor([0, 3, 4, 7, 80, 83, 156, 159])
    ys = torch.tensor([0, 7, 8, 15, 80, 87, 152, 159])
    xs = torch.tensor([0, 15, 16, 31, 80, 95, 144, 159])
    grid = torch.cartesian_prod(zs, ys, xs).cuda()
    r = lambda n, hi: torch.randint(0, hi, (n,), generator=gen, device="cuda")   # noqa: E731
    face = r(3 * 1024, SS).view(1024, 3)
    ax = r(1024, 3)
    face[torch.arange(1024, device="cuda"), ax] = r(1024, 2) * (SS - 1)
    seam = torch.stack([r(1536, SS // 4) * 4 + r(1536, 2) * 3, r(1536, SS // 8) * 8 + r(1536, 2) * 7, r(1536, SS // 16) * 16 + r(1536, 2) * 15], 1)
    inner = r(3 * 1024, SS - 2).view(1024, 3) + 1
    return torch.cat([grid, face, seam, inner])


def _conv_at(zb, W64, pts):
    """float64 conv of one sample at the voxels pts [N,3] from the gathered 3x3x3 neighbourhood (zero padding): zb [S,S,S,48], W64 [48,48,27] -> [N,48]"""
    N = pts.shape[0]
    nb = torch.zeros(N, 27, 48, dtype=torch.float64, device=zb.device)
    for tap in range(27):
        o = torch.tensor([tap // 9 - 1, (tap // 3) % 3 - 1, tap % 3 - 1], device=zb.device)
        p = pts + o
        ok = ((p >= 0) & (p < SS)).all(1)
        pc = p.clamp(0, SS - 1)
        nb[:, tap] = zb[pc[:, 0], pc[:, 1], pc[:, 2]].double() * ok[:, None]
    return torch.einsum("ntc,oct->no", nb, W64)


def test_benched_shape_per_sample_forward():
    """conv3d_k3_c48_per_sample at B = 8, 160^3 against float64 at 4096 voxels per sample (corners, faces, tile seams, the last voxel of sample 7 whose byte
    offset is past 2^31), fused statistics against float64 statistics of the whole stored output"""
    ops = _ops()
    gen = _gen()
    st = _stats1(SB, seed=160)
    rs = st[..., 1].cuda()
    z = _z_gpu(rs, gen)
    Wm = rnd(48, 48, 3, 3, 3, seed=91, scale=(27 * 48) ** -0.5)
    wk = torch.empty(SB * ops.C48_IMG, dtype=BF, device="cuda")
    ops.conv48_pack_scaled(dev(Wm), dev(st), wk, SB)
    acc = torch.full((SB, 48, 2), 5.0, dtype=torch.float64, device="cuda")
    y = ops.conv3d_k3_c48_per_sample(z, wk, stats_acc=acc)
    torch.cuda.synchronize()
    pts = _voxels(gen)
    assert (pts == SS - 1).all(1).any()
    W64 = Wm.double().cuda().reshape(48, 48, 27)
    for b in range(SB):
        ref = _conv_at(z[b], W64 * rs[b].double().view(1, 48, 1), pts)
        got = y[b][pts[:, 0], pts[:, 1], pts[:, 2]]
        check(got, ref, BF, f"160^3 per-sample conv b={b}")   # measured max-norm <= 3.5e-3
    # fused statistics; measured <= 3.7e-7 relative to sum |y| / sum y^2
    for b in range(SB):
        yb = y[b].view(-1, 48).double()
        s1, a1, s2 = yb.sum(0), yb.abs().sum(0), (yb * yb).sum(0)
        e0 = ((acc[b, :, 0] - s1).abs() / a1).max().item()
        e1 = ((acc[b, :, 1] - s2).abs() / s2).max().item()
        _print_err(f"160^3 fused stats b={b}", max(e0, e1))
        assert e0 < 3e-6 and e1 < 3e-6, (b, e0, e1)
        del yb


def test_benched_shape_bwd_reduce_centered():
    """conv3d_k3_c48_bwd_reduce_centered at B = 8, 160^3: dX == the plain dgrad bit for bit, the sums against float64 reductions of (dX, z)"""
    ops = _ops()
    gen = _gen()
    st = _stats1(SB, seed=161)
    rs, e = st[..., 1].double().cuda(), st[..., 0].double().cuda()
    z = _z_gpu(st[..., 1].cuda(), gen)
    dy = _randn_bf16_gpu(gen)
    wkd = _pack_via_kernel(rnd(48, 48, 3, 3, 3, seed=92, scale=(27 * 48) ** -0.5), 7, BF, ops.C48_IMG)
    sums = torch.full((SB, 48, 2), 5.0, dtype=torch.float64, device="cuda")
    dx = ops.conv3d_k3_c48_bwd_reduce_centered(dy, wkd, z, dev(st), sums)
    ref_dx = ops.conv3d_k3_c48(dy, wkd)
    torch.cuda.synchronize()
    assert torch.equal(dx, ref_dx)
    del ref_dx, dy
    for b in range(SB):
        ref, scale = torch.zeros(2, 48, dtype=torch.float64, device="cuda"), torch.zeros(48, dtype=torch.float64, device="cuda")
        for h in range(2):   # half a sample at a time (float64 temporaries)
            d = dx[b, h * 80:(h + 1) * 80].reshape(-1, 48).double()
            t = _t(z[b, h * 80:(h + 1) * 80].reshape(-1, 48))
            g = d * torch.where(t > 0, 1.0, SLOPE)
            ref[0] += g.sum(0)
            ref[1] += (g * (t - e[b]) * rs[b]).sum(0)
            scale += d.abs().sum(0)
            del d, t, g
        for k in range(2):
            err = ((sums[b, :, k] - ref[k]).abs() / scale).max().item()
            _print_err(f"160^3 bwd_reduce_centered sums b={b} k={k}", err)
            assert err < 2e-8, (b, k, err)   # relative to sum |dX|, as in the small test: measured <= 1.2e-9


def test_benched_shape_instnorm_bwd_apply_bg_centered():
    """instnorm_bwd_apply_bg_centered at B = 8, 160^3 against the float64 formula, every element (bound as in the small test)"""
    ops = _ops()
    gen = _gen()
    st = _stats1(SB, seed=162)
    rs, e = st[..., 1].double().cuda(), st[..., 0].double().cuda()
    z = _z_gpu(st[..., 1].cuda(), gen)
    d = _randn_bf16_gpu(gen)
    V = SS ** 3
    sums = (0.5 * torch.randn(SB, 48, 2, generator=gen, device="cuda")).double() * V
    dx = torch.empty(SB * V, 48, dtype=BF, device="cuda")
    ops.instnorm_bwd_apply_bg_centered(d.view(-1, 48), z.view(-1, 48), dev(st), sums, dx, SB, V, 48, slope=SLOPE)
    torch.cuda.synchronize()
    dx = dx.view(SB, V, 48)
    worst = 0.0
    for b in range(SB):
        m1, m2 = sums[b, :, 0] / V, sums[b, :, 1] / V
        r = rs[b]
        for h in range(4):
            sl = slice(h * V // 4, (h + 1) * V // 4)
            t = _t(z[b].view(V, 48)[sl])
            gg = d[b].view(V, 48)[sl].double() * torch.where(t > 0, 1.0, SLOPE)
            ref = r * (gg - m1 - (t - e[b]) * r * m2)
            mag = (r * gg).abs() + (r * m1).abs() + (r * r * m2 * t).abs() + (r * r * m2 * e[b]).abs()
            bound = 2.0 ** -8 * ref.abs() + 2.0 ** -19 * mag
            worst = max(worst, ((dx[b, sl].double() - ref).abs() / bound).max().item())
            del t, gg, ref, mag, bound
    _print_err("160^3 apply_bg_centered / bound", worst)
    assert worst <= 1.0, worst


def test_benched_shape_wgrad_scaled():
    """conv3d_k3_c48_wgrad_scaled at B = 8, 160^3 against the float64 combination sum_b rstd_b[ci] conv3d_k3_c48_wgrad(dY_b, z_b) of eight B = 1 launches
    (the plain kernel is checked against F.conv3d and by the 160^3 adjoint identity); sum |terms| from the same launches on (|dY_b|, |z_b|)"""
    ops = _ops()
    gen = _gen()
    st = _stats1(SB, seed=163)
    rs = st[..., 1].double().cuda()
    z = _z_gpu(st[..., 1].cuda(), gen)
    dy = _randn_bf16_gpu(gen)
    dW0 = rnd(48, 48, 3, 3, 3, seed=93, scale=10.0).cuda()
    dW = dW0.clone()
    ops.conv3d_k3_c48_wgrad_scaled(dy, z, dev(st), dW)
    ref = dW0.double().clone()
    mag = dW0.double().abs()
    for b in range(SB):
        part = torch.zeros(48, 48, 3, 3, 3, device="cuda")
        ops.conv3d_k3_c48_wgrad(dy[b:b + 1], z[b:b + 1], part)
        ref += part.double() * rs[b].view(1, 48, 1, 1, 1)
        part.zero_()
        ops.conv3d_k3_c48_wgrad(dy[b:b + 1].abs(), z[b:b + 1].abs(), part)
        mag += part.double() * rs[b].view(1, 48, 1, 1, 1)
    torch.cuda.synchronize()
    # fp32 summation order of two fp32 computations, relative to sum |terms|; a wrong slot-to-sample scale is off by O(1); measured <= 6.3e-9
    err = ((dW.double() - ref).abs() / mag).max().item()
    _print_err("160^3 wgrad_scaled", err)
    assert err < 1e-7, err
