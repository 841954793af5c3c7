"""GPU: the eight entries of csrc/heads.hip one by one through nerf_mae_amd.ops, and the host glue around them (_HeadFn, _ResBlock8Fn), against the float64
references of tests/_heads_ref.py (checked themselves by tests/test_heads_ref_cpu.py).  Reference inputs are the fp32 / bf16-rounded values a kernel sees.

Bounds.  The data-movement kernels copy or add at most 27 terms: bit equality, or a bound derived from the term count.  The SR loss accumulates in fp32:
the bounds are derived at each test.  The masked CE uses __expf / __logf, whose error depends on the argument range: CE_FWD_TOL / CE_BWD_TOL are 4x the worst
error measured on the MI355X over every case below, rounded up to one digit, and stay under _heads_ref.CE_TOL_CEILING = 2e-5.  Every figure is printed
before it is asserted (pytest -s shows them)."""
import pytest
import torch

from tests import _heads_ref as HR
from tests._metrics import assert_close, rel_l2

pytestmark = pytest.mark.gpu

F64, BF = torch.float64, torch.bfloat16
DTS = [torch.float32, BF]
DT_ID = {torch.float32: "fp32", BF: "bf16"}
CE_FWD_TOL = 3e-6   # worst measured over all cases 5.2e-7 (an intersection sum of the soft IoU); the scalars and sums[] <= 1.2e-7   
CE_BWD_TOL = 3e-6   # worst measured 6.0e-7 of max|ref| (rel-L2 1.4e-7)
assert CE_FWD_TOL <= HR.CE_TOL_CEILING and CE_BWD_TOL <= HR.CE_TOL_CEILING
GLUE_TOL = {torch.float32: 2e-4, BF: 3e-2}


def _ops():
    from nerf_mae_amd import ops
    return ops


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ---- grid_to_cl8 ---------------------------------------------------------------------------------------------------------------------------
def _check_grid_to_cl8(S, B, dt):
    xb = (torch.randn((B, 4, S, S, S), generator=_gen(S + B)) * 3.0)
    xb[:, :, 0, 0, :2] = torch.tensor([0.0, -0.0])
    got = _ops().grid_to_cl8(xb.cuda(), dt)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, S, S, S, 8) and got.dtype == dt
    want = xb.cuda().to(dt).permute(0, 2, 3, 4, 1)
    assert torch.equal(_bits(got[..., :4].contiguous()), _bits(want.contiguous())), "channels 0..3 are not the input rounded to the dtype, bit for bit"
    assert (_bits(got[..., 4:].contiguous()) == 0).all(), "channels 4..7 are not +0"


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("S,B", [(7, 1), (7, 3), (33, 1), (33, 3)])
def test_grid_to_cl8(S, B, dt):
    _check_grid_to_cl8(S, B, dt)


def test_grid_to_cl8_full_size():
    for dt in DTS:
        for B in (1, 3):
            _check_grid_to_cl8(160, B, dt)


# ---- head_upsample_fwd / head_upsample_bwd -------------------------------------------------------------------------------------------------
UP_SMALL = [(R, s, Co, Cp, B) for (R, s) in [(32, 1.6), (32, 2.4), (20, 2.4), (40, 1.6)] for (Co, Cp) in [(4, 8), (19, 24), (1, 8), (32, 32)] for B in (1, 2)]


def _check_upsample_fwd(R, scale, Co, Cp, B, dt, on_device):
    Ro, src = HR.nn_src_index(R, scale)
    y = (torch.randn((B * R ** 3, Cp), generator=_gen(R + Co + B)) * 2.0).to(dt)      # the columns >= Co hold values too: they must not be read
    yd = y.cuda()
    got = _ops().head_upsample_fwd(yd, Co, B, R, Ro, HR.inv_scale_f32(scale))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, Co, Ro, Ro, Ro) and got.dtype == torch.float32
    want = HR.upsample_fwd(yd if on_device else y, Co, B, R, src).float()
    assert torch.equal(_bits(got), _bits(want.cuda())), "head_upsample_fwd is not a bit-exact copy of the source voxels"


def _check_upsample_bwd(R, scale, Co, Cp, B, dt, on_device):
    Ro, src = HR.nn_src_index(R, scale)
    inv = HR.inv_scale_f32(scale)
    g = _gen(3 * R + Co + B)
    # integers in [-4, 4]: every sum is <= 27 * 4 in magnitude, exact in fp32 and in bf16 -> equality; catches a wrong [lo, hi) at any source index
    dint = torch.randint(-4, 5, (B, Co, Ro, Ro, Ro), generator=g).float()
    dd = dint.cuda()
    got = _ops().head_upsample_bwd(dd, Cp, R, dt, inv)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B * R ** 3, Cp) and got.dtype == dt
    ref = HR.upsample_adjoint(dd if on_device else dint, Cp, R, src).cuda()
    assert ref.abs().max().item() <= 108
    assert torch.equal(got.double(), ref), f"integer adjoint differs at {int((got.double() != ref).sum())} entries"
    assert (got[:, Co:] == 0).all()
    del got, ref, dd, dint
    # Gaussian: <= 27 fp32 additions -> |err| <= 32 * 2^-24 * adj(|dpred|); the bf16 store adds 2^-8 |ref|
    dgs = torch.randn((B, Co, Ro, Ro, Ro), generator=g)
    dd = dgs.cuda()
    got = _ops().head_upsample_bwd(dd, Cp, R, dt, inv).double()
    torch.cuda.synchronize()
    ref = HR.upsample_adjoint(dd if on_device else dgs, Cp, R, src).cuda()
    mag = HR.upsample_adjoint((dd if on_device else dgs).abs(), Cp, R, src).cuda()
    bound = 32 * 2.0 ** -24 * mag + (2.0 ** -8 * ref.abs() if dt == BF else 0.0)
    err = (got - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"  [head_upsample_bwd {DT_ID[dt]} R{R} x{scale} Co{Co} B{B}] worst |err| / bound {worst:.3f}, max |err| / max |ref| {err.max().item() / ref.abs().max().item():.2e}")
    assert (err <= bound).all(), f"gaussian adjoint exceeds its bound by {worst:.2f}x"
    assert (got[:, Co:] == 0).all()


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("R,scale,Co,Cp,B", UP_SMALL)
def test_head_upsample_fwd(R, scale, Co, Cp, B, dt):
    _check_upsample_fwd(R, scale, Co, Cp, B, dt, on_device=False)


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("R,scale,Co,Cp,B", UP_SMALL)
def test_head_upsample_bwd(R, scale, Co, Cp, B, dt):
    _check_upsample_bwd(R, scale, Co, Cp, B, dt, on_device=False)


def _upsample_full(R, scale, Co, Cp, B):
    """the reference is built on the device from the CPU-derived index map, by torch indexing / index_add_ (not F.interpolate, not the kernels)"""
    for dt in DTS:
        _check_upsample_fwd(R, scale, Co, Cp, B, dt, on_device=True)
        _check_upsample_bwd(R, scale, Co, Cp, B, dt, on_device=True)
        torch.cuda.empty_cache()


def test_head_upsample_full_size_160_to_256():
    _upsample_full(160, 1.6, 4, 8, 1)


def test_head_upsample_full_size_160_to_384():
    _upsample_full(160, 2.4, 1, 8, 1)


def test_head_upsample_full_size_160_to_384_grid_stride():
    """B = 5: 5 * 384^3 / 256 = 1 105 920 blocks > the cap of 65535 * 16 = 1 048 560, so the forward's grid-stride loop takes a second trip"""
    assert (5 * 384 ** 3 + 255) // 256 > 65535 * 16
    _upsample_full(160, 2.4, 1, 8, 5)


# ---- add_cols_f32 --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,C,lds,ldd", [(48, 108, 216, 108), (48, 4, 8, 4), (19, 5, 7, 11)])
def test_add_cols_f32(M, C, lds, ldd):
    src = torch.randn((M, lds), generator=_gen(M + C))
    dst = torch.randn((M, ldd), generator=_gen(M + C + 1))
    want = dst.clone()
    want[:, :C] = dst[:, :C] + src[:, :C]
    sd, dd = src.cuda(), dst.cuda()
    _ops().add_cols_f32(sd, dd, C)
    torch.cuda.synchronize()
    assert torch.equal(_bits(dd), _bits(want.cuda())), "dst[:, :C] += src[:, :C] is not bit-exact, or columns >= C were touched"
    assert torch.equal(sd.cpu(), src)


# ---- VoxelSR loss --------------------------------------------------------------------------------------------------------------------------
def _sr_inputs(S, B):
    g = _gen(11 * S + B)
    pred = torch.randn((B, 4, S, S, S), generator=g)
    tgt = torch.rand((B, 4, S, S, S), generator=g)
    alpha = torch.rand((B, S, S, S), generator=g) * 0.02            # both sides of 0.01
    r = torch.rand((B, S, S, S), generator=g)
    alpha[r < 0.05] = 0.0
    alpha[(r >= 0.05) & (r < 0.10)] = 0.01                          # float32(0.01) exactly: not counted, the comparison is strict
    alpha[(r >= 0.10) & (r < 0.15)] = 0.8
    alpha.view(B, -1)[:, :3] = torch.tensor([0.01, 0.0, 0.5])
    tgt[:, 3] = alpha
    return pred, tgt


def _check_sr_loss(S, B, on_device):
    ops = _ops()
    pred, tgt = _sr_inputs(S, B)
    assert int((tgt[:, 3] == _f32(0.01)).sum()) > 0 and int((tgt[:, 3] > 0.01).sum()) > 0 and int((tgt[:, 3] < 0.01).sum()) > 0
    pd, td = pred.cuda(), tgt.cuda()
    sums = torch.full((2,), 7.0, dtype=F64, device="cuda")
    loss = torch.full((1,), 7.0, device="cuda")
    ops.voxel_sr_loss_fwd(pd, td, sums, loss)
    torch.cuda.synchronize()
    rp, rt = (pd, td) if on_device else (pred, tgt)
    s0, s1, l = (x.item() for x in HR.sr_loss(rp, rt))
    e0, el = abs(sums[0].item() - s0) / s0, abs(loss.item() - l) / l
    print(f"  [sr_loss_fwd S{S} B{B}] sums[0] rel {e0:.2e}, loss rel {el:.2e}, count {int(s1)}")
    assert sums[1].item() == s1, "sums[1] is an integer count: exact"
    # non-negative terms summed in fp32: relative error ~ 2^-24 * (terms per thread + ~20) <= 2^-24 * 84 = 5e-6 at 2 * 256^3 under the 2048-block cap
    assert e0 <= 1e-5 and el <= 1e-5
    for gs in (1.0, 0.37):
        dp = torch.full_like(pd, 7.0)
        ops.voxel_sr_loss_bwd(pd, td, sums, gs, dp)
        torch.cuda.synchronize()
        ref = HR.sr_loss_grad(rp, rt, _f32(gs)).cuda()
        err = (dp.double() - ref).abs()
        worst = (err / ref.abs().clamp_min(1e-300))[ref != 0].max().item()
        print(f"  [sr_loss_bwd S{S} B{B} gscale {gs}] worst |err| / |ref| {worst:.2e}")
        assert (err <= 1e-6 * ref.abs()).all(), f"worst relative error {worst:.2e} > 1e-6 (about four fp32 roundings)"
        assert (dp[:, 3] == 0).all(), "the alpha plane has no gradient"
        dead = (td[:, 3:] <= _f32(0.01)).expand(-1, 3, -1, -1, -1)
        assert (dp[:, :3][dead] == 0).all(), "a voxel with m = 0 has no gradient"
        del dp, ref, err


@pytest.mark.parametrize("S,B", [(7, 1), (7, 2), (7, 3), (51, 1), (51, 2), (51, 3)])
def test_voxel_sr_loss(S, B):
    _check_sr_loss(S, B, on_device=False)


def test_voxel_sr_loss_full_size_256():
    _check_sr_loss(256, 1, on_device=True)


# ---- masked cross entropy + soft-IoU sums --------------------------------------------------------------------------------------------------
def _rel(got, ref):
    return (got - ref).abs().max().item() / ref.abs().max().item()


def _check_masked_ce(case, on_device):
    ops = _ops()
    name, K, has_cw, shape, B, sig, kind = case
    logits, labels, cw = HR.ce_inputs(case)
    ld, bd, cd = logits.cuda(), labels.cuda(), None if cw is None else cw.cuda()
    sums = torch.full((2,), 7.0, dtype=F64, device="cuda")
    iou = torch.full((B, K - 1, 3), 7.0, dtype=F64, device="cuda")
    out = torch.full((2,), 7.0, device="cuda")
    ops.masked_ce_fwd(ld, bd, cd, sums, iou, out)
    torch.cuda.synchronize()
    rl, rb, rc = (ld, bd, cd) if on_device else (logits, labels, cw)
    ref = HR.masked_ce(rl, rb, rc)
    r_sums, r_iou = ref["sums"].cuda(), ref["iou"].cuda()
    figs = {"out[0]": abs(out[0].item() - ref["ce"].item()) / ref["ce"].item(), "out[1]": abs(out[1].item() - ref["miou"].item()) / ref["miou"].item(),
            "sums[0]": abs(sums[0].item() - r_sums[0].item()) / r_sums[0].item(), "sums[1]": abs(sums[1].item() - r_sums[1].item()) / r_sums[1].item()}
    for j, nm in ((0, "iou sum m p"), (2, "iou inter")):
        e = (iou[..., j] - r_iou[..., j]).abs()
        assert (iou[..., j][r_iou[..., j] == 0] == 0).all(), f"{nm}: an absent class / a blank sample must sum to exactly 0"
        nz = r_iou[..., j] != 0
        figs[nm] = (e[nz] / r_iou[..., j][nz]).max().item()
    print(f"  [masked_ce_fwd {name}] " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert torch.equal(iou[..., 1], r_iou[..., 1]), "the per-class voxel counts are integers: exact"
    for k, v in figs.items():
        assert v <= CE_FWD_TOL, f"{name} {k}: relative error {v:.2e} > {CE_FWD_TOL:g}"
    unl = (bd == 0)[:, None].expand(-1, K, *[-1] * len(shape))
    for gs in (1.0, 0.37):
        dl = torch.full_like(ld, 7.0)
        ops.masked_ce_bwd(ld, bd, cd, sums, gs, dl)
        torch.cuda.synchronize()
        gref = HR.masked_ce_grad(rl, rb, rc, _f32(gs)).cuda()
        e_max, e_l2 = _rel(dl.double(), gref), rel_l2(dl, gref) if not on_device else ((dl.double() - gref).norm() / gref.norm()).item()
        print(f"  [masked_ce_bwd {name} gscale {gs}] max |err| / max |ref| {e_max:.2e}, rel-L2 {e_l2:.2e}")
        assert e_max <= CE_BWD_TOL and e_l2 <= CE_BWD_TOL, f"{name}: gradient error max {e_max:.2e} / L2 {e_l2:.2e} > {CE_BWD_TOL:g}"
        assert (dl[unl] == 0).all(), "an unlabelled voxel has no gradient"
        del dl, gref


@pytest.mark.parametrize("case", HR.ce_cases(), ids=lambda c: c[0])
def test_masked_ce(case):
    _check_masked_ce(case, on_device=False)


def test_masked_ce_full_size_160():
    _check_masked_ce(HR.CE_FULL_SIZE, on_device=True)


def test_masked_ce_rejects_k_outside_2_to_32():
    from nerf_mae_amd._lib import NmhError
    for K in (1, 33):
        lg, lb = torch.zeros((1, K, 8), device="cuda"), torch.zeros((1, 8), device="cuda")
        sums, iou, out = torch.zeros(2, dtype=F64, device="cuda"), torch.zeros((1, max(K - 1, 1), 3), dtype=F64, device="cuda"), torch.zeros(2, device="cuda")
        with pytest.raises(NmhError):
            _ops().masked_ce_fwd(lg, lb, None, sums, iou, out)
        with pytest.raises(NmhError):
            _ops().masked_ce_bwd(lg, lb, None, sums, 1.0, torch.zeros_like(lg))


# ---- host glue at resolution 32 ------------------------------------------------------------------------------------------------------------
_HEADS = {}


def _heads(dt):
    """the two heads of tests/test_heads.py::_hip_heads (oracle-initialised), packed, built once per dtype"""
    if dt not in _HEADS:
        from tests.test_heads import _hip_heads
        sr, se, _, _ = _hip_heads(dt)
        for m in (sr, se):
            m._pack()
        torch.cuda.synchronize()
        _HEADS[dt] = (sr, se)
    return _HEADS[dt]


def _q(t, dt):
    return t.detach().to(dt).double().cpu()


def _run_head_fn(head, conv, d0, dpred, B, R, Ro, inv):
    from nerf_mae_amd.heads import _HeadFn
    conv.weight.grad = conv.bias.grad = None
    x = d0.clone().requires_grad_(True)
    pred = _HeadFn.apply(x, head, conv, B, R, Ro, inv)
    pred.backward(dpred)
    torch.cuda.synchronize()
    return pred.detach().clone(), x.grad.clone(), conv.weight.grad.clone(), conv.bias.grad.clone()


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("which", ["sr_Co4_x1.6", "sem_Co19_x1"])
def test_head_fn_matches_float64_conv_and_upsample(which, dt):
    """_HeadFn pads Co to a multiple of 8 rows for the GEMM: pred, dd0, the ragged-N weight gradient and the fused bias gradient against a float64 1x1x1 conv
    + nearest upsampling; the padding contributes nothing (the pack zeroes the padded weight rows whatever they held, and a poisoned bias padding only
    reaches output columns nobody reads: same bits with and without)"""
    sr, se = _heads(dt)
    head, conv, scale = (sr, sr.voxel_out.conv, 1.6) if which.startswith("sr") else (se, se.sem_out.conv, 1.0)
    B, R = 2, 32
    Co, C = conv.weight.shape[0], conv.weight.shape[1]
    Cop = (Co + 7) // 8 * 8
    assert Cop > Co
    if scale == 1.0:
        Ro, src, inv = R, torch.arange(R), 1.0
    else:
        (Ro, src), inv = HR.nn_src_index(R, scale), HR.inv_scale_f32(scale)
    g = _gen(Co)
    d0 = torch.randn((B * R ** 3, C), generator=g).to(dt).cuda()
    dpred = torch.randn((B, Co, Ro, Ro, Ro), generator=g).cuda()
    # the pack writes every padded entry: poison the packed operands, re-run the pack, the padding must be +0 again
    head._pk["out.w"].fill_(float("nan"))
    head._pk["out.wT"].fill_(float("nan"))
    head._pack()
    torch.cuda.synchronize()
    assert (head._pk["out.w"].view(Cop, C)[Co:] == 0).all() and (head._pk["out.wT"].view(C, Cop)[:, Co:] == 0).all()
    assert torch.equal(head._pk["out.w"].view(Cop, C)[:Co].float(), conv.weight.detach().view(Co, C).to(dt).float())
    head._bias_pad.zero_()
    clean = _run_head_fn(head, conv, d0, dpred, B, R, Ro, inv)
    head._bias_pad[Co:] = float("nan")
    try:
        poisoned = _run_head_fn(head, conv, d0, dpred, B, R, Ro, inv)
    finally:
        head._bias_pad.zero_()
    for a, b, nm in zip(clean[:2], poisoned[:2], ("pred", "dd0")):
        assert torch.equal(_bits(a), _bits(b)), f"{nm} depends on the bias padding"
    # (dW and dbias are reduced with atomics: no two runs agree bit for bit, so both runs are held to the reference instead)
    w = _q(conv.weight.view(Co, C), dt)
    x = d0.double().cpu()
    want = HR.out_conv_upsample(x, w, conv.bias.detach().double().cpu(), B, R, src)
    gref = HR.upsample_adjoint(dpred.cpu(), Co, R, src)                    # [B*R^3][Co]
    tol = GLUE_TOL[dt]
    for run, (pred, dd0, dW, db) in (("clean", clean), ("poisoned bias padding", poisoned)):
        assert_close(pred, want, tol, f"_HeadFn {which} pred {DT_ID[dt]} ({run})")
        assert_close(dd0, gref @ w, tol, f"_HeadFn {which} dd0 {DT_ID[dt]} ({run})")
        assert_close(dW.view(Co, C), gref.t() @ x, tol, f"_HeadFn {which} dW {DT_ID[dt]} ({run})")
        assert_close(db, gref.sum(0), tol, f"_HeadFn {which} dbias {DT_ID[dt]} ({run})")


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
def test_res_block8_fn_matches_float64_block(dt):
    """encoder1 = UnetResBlock(4 -> 48) on the 8-channel zero-padded input: output and the un-padded weight gradients (conv1 (C,4,27) and conv3 (C,4) through
    add_cols_f32, conv2) against float64 autograd of the block on the same rounded inputs and weights; the bias gradients are exact zeros (a constant per
    channel in front of an affine-free InstanceNorm cancels).  bf16 takes the conv48 path (e1.c2.wk).
    The derivative of the two LeakyReLUs is taken, as the kernels take it, from the sign of the activation the forward stored (a1 and out): with bf16
    storage 1e-3 of the voxels next to the kink land on the other side than in float64, each an O(1) change of that voxel's gradient, which an independent
    random dout does not average out (measured: 4 % relative L2 on all three weight gradients, 3.9e-2 .. 4.4e-2 max-norm, against signs from float64).  The
    flips must be few (< 2e-3 of the voxels, the figure tests/test_centered_decoder1_gpu.py uses) and sit at the kink (|float64 pre-activation| < 2e-2)."""
    from nerf_mae_amd.heads import _ResBlock8Fn
    ops = _ops()
    sr, _ = _heads(dt)
    blk = sr.encoder1.layer
    B, S, C = 2, 32, blk.conv2.weight.shape[0]
    assert ("e1.c2.wk" in sr._pk.views) == (dt == BF), "bf16 has to take the conv48 path, fp32 the generic one"
    g = _gen(8)
    xb = torch.randn((B, 4, S, S, S), generator=g)
    dout = torch.randn((B * S ** 3, C), generator=g).to(dt)
    for p in blk.parameters():
        p.grad = None
    x8 = ops.grid_to_cl8(xb.cuda(), dt)
    anchor = torch.zeros(1, device="cuda", requires_grad=True)
    out = _ResBlock8Fn.apply(anchor, sr, x8, B, S)
    out.backward(dout.cuda())
    torch.cuda.synchronize()
    ws = [_q(p, dt).requires_grad_(True) for p in (blk.conv1.weight, blk.conv2.weight, blk.conv3.weight)]
    bs = [p.detach().double().cpu() for p in (blk.conv1.bias, blk.conv2.bias, blk.conv3.bias)]
    signs = [(t.detach().float().cpu().view(B, S, S, S, C).permute(0, 4, 1, 2, 3) > 0) for t in (out.grad_fn.saved[3], out)]
    want, pre = HR.res_block(_q(xb, dt), ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], signs=signs)
    for sg, pr, nm in zip(signs, pre, ("a1", "out")):
        flip = sg != (pr > 0)
        frac, near = flip.double().mean().item(), (pr[flip].abs().max().item() if flip.any() else 0.0)
        print(f"  [_ResBlock8Fn {DT_ID[dt]} {nm}] kink sign flips: fraction {frac:.2e}, max |pre-activation| {near:.2e}")
        assert frac < 2e-3 and near < 2e-2, (nm, frac, near)
    want.backward(dout.double().view(B, S, S, S, C).permute(0, 4, 1, 2, 3))
    tol = GLUE_TOL[dt]
    failed = []
    pairs = [("out", out.view(B, S, S, S, C).permute(0, 4, 1, 2, 3), want.detach())]
    for conv, w, nm in zip((blk.conv1, blk.conv2, blk.conv3), ws, ("conv1", "conv2", "conv3")):
        assert conv.weight.grad.shape == conv.weight.shape
        assert conv.bias.grad is not None and (conv.bias.grad == 0).all(), f"{nm}.bias.grad must be exact zeros"
        pairs.append((nm + ".weight.grad", conv.weight.grad, w.grad))
    for nm, a, b in pairs:       # every figure is looked at before the first failure is raised
        try:
            assert_close(a, b, tol, f"_ResBlock8Fn {nm} {DT_ID[dt]}")
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed
