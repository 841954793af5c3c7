"""GPU: the four entry points of the kept-token patch embed one by one through nerf_mae_amd.ops -- embed_kept_rows (mask_rowmap_kernel),
patch_embed_gather_kept (embed_gather_kept_kernel), embed_norm_fwd_kept / embed_norm_bwd_kept (the rowmap branches of the LayerNorm kernels) -- and their chain
with the GEMM and the weight gradient, against the references of tests/_embed_kept_ref.py.  Reference inputs are the fp32 / bf16-rounded values a kernel sees.

Every buffer a kernel has to fill or zero holds NaN (the row map: a poison integer) before the call, and every compact operand lies between two guard regions
that must come back untouched.  The row map and the gather are equalities.  The LayerNorm and chain bounds are 4x the worst figure (max-norm, relative L2,
elementwise; tests/_metrics.py) measured on the MI355X over every case below against float64, rounded up to one digit and capped by the bounds
tests/test_kernels_gpu.py uses for the same arithmetic (2e-4 / 3e-2, twice that for a LayerNorm backward).  Every figure is printed before it is asserted
(NMH_PRINT_ERR=1, pytest -s).

When more tokens are kept than the capacity holds, the forward normalises a kept token without a row from zeros and the backward adds its dtok to dmask_token:
both are documented as memory-safe only (the host re-captures before such a step runs), so the overflow cases here assert the row-map contract, the rows that
are present and the guards, and pin none of those values."""
import os
import random

import pytest
import torch

from tests import _embed_kept_ref as ER
from tests._metrics import assert_close, rel_l2, relerr, worst_elementwise

pytestmark = pytest.mark.gpu

F64, BF = torch.float64, torch.bfloat16
DTS = [torch.float32, BF]
DT_ID = {torch.float32: "fp32", BF: "bf16"}
CEIL = {torch.float32: 2e-4, BF: 3e-2}          # tests/test_kernels_gpu.py: TOL; its LayerNorm-backward checks take twice that
# bound = min(ceiling, 4 x the worst figure measured on the MI355X over all cases of this file, rounded up to one digit); a figure is the largest of the
# max-norm, the relative L2 and the elementwise error
FWD_TOK_TOL = {torch.float32: 2e-5, BF: 2e-2}     # measured 3.0e-6 / 3.6e-3 (elementwise; max-norm 1.6e-7 / 3.4e-3)
FWD_STAT_TOL = 9e-7                               # mean / rstd are fp32 in both modes: measured 2.1e-7
BWD_DY0_TOL = {torch.float32: 9e-7, BF: 2e-2}     # measured 2.2e-7 / 3.8e-3
BWD_PARAM_TOL = {torch.float32: 5e-6, BF: 5e-6}   # dgamma, dbeta, dmask_token: fp32 sums of fp32 products in both modes: measured 1.1e-6 / 9.3e-7
CHAIN_TOK_TOL = {torch.float32: 2e-5, BF: 3e-2}   # measured 3.1e-6 / 1.4e-2 (elementwise, K = 64 rows at R = 32; max-norm 4.2e-3): 4 x is above the ceiling
CHAIN_GRAD_TOL = {torch.float32: 2e-5, BF: 3e-2}  # dW, db, dgamma, dbeta, dmask_token: measured 2.6e-6 / 6.8e-3 (dW elementwise; max-norm 1.4e-6 / 2.8e-3)
RUN_TO_RUN_TOL = 5e-6                             # dgamma / dbeta / dmask_token are fp32 atomic sums: two runs differ by the order of additions; measured 1.1e-6
for _t, _m in ((FWD_TOK_TOL, 1), (BWD_DY0_TOL, 2), (BWD_PARAM_TOL, 2), (CHAIN_TOK_TOL, 1), (CHAIN_GRAD_TOL, 2)):
    assert all(_t[d] <= _m * CEIL[d] for d in DTS)
assert FWD_STAT_TOL <= CEIL[torch.float32] and RUN_TO_RUN_TOL <= CEIL[torch.float32]

POISON = -123456789
SENTINEL = -7.25        # exact in bf16
GUARD_ROWS = 4


def _ops():
    from nerf_mae_amd import ops
    return ops


def _close(a, b, tol, name):
    """assert_close, after printing the smallest tolerance each of its three checks would still pass with"""
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  [{name}] needs max-norm {relerr(a, b):.2e}  rel-L2 {rel_l2(a, b):.2e}  elementwise {worst_elementwise(a, b, 1.0):.2e}  (bound {tol:g})")
    assert_close(a, b, tol, name)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _nan(shape, dt):
    t = torch.full(shape, float("nan"), dtype=dt, device="cuda")
    assert (_bits(t) == (0x7FC00000 if dt == torch.float32 else 0x7FC0)).all()
    return t


def _guarded(rows, cols, dt):
    """a NaN-filled [rows, cols] operand between two sentinel-filled guard regions of GUARD_ROWS rows each -> (whole buffer, the operand)"""
    G = GUARD_ROWS * cols
    buf = torch.full((2 * G + rows * cols,), SENTINEL, dtype=dt, device="cuda")
    A = buf[G:G + rows * cols].view(rows, cols)
    A.fill_(float("nan"))
    assert A.is_contiguous() and A.data_ptr() % 16 == 0
    return buf, A


def _guards_untouched(buf, cols):
    G = GUARD_ROWS * cols
    return bool((buf[:G] == SENTINEL).all() and (buf[-G:] == SENTINEL).all())


def _padded_input(x):
    """x on the device as a view into a larger allocation (nothing behind the last voxel is part of the input)"""
    buf = torch.zeros(x.numel() + 256, dtype=x.dtype, device="cuda")
    v = buf[:x.numel()].view(x.shape)
    v.copy_(x)
    return v


# ---- 1. embed_kept_rows ---------------------------------------------------------------------------------------------------------------------
ROWMAP_N = [1, 15, 16, 17, 343, 512, 1000,             # one wave; n % 16 != 0: the scalar tail of load16
            1023, 1024, 1025, 1728, 4096,              # later waves: the prefix over wsum[]
            16384, 16385, 17576,                       # seg 1024 -> 2048: two steps per wave
            64000,                                     # 40^3, the benchmarked size: 16 waves x 4 steps
            131072, 131073, 262149]                    # 8, 9 and 17 steps


def _rowmap_call(mask_dev, cap):
    out = torch.full((mask_dev.numel() + 2,), POISON, dtype=torch.int32, device="cuda")
    got = _ops().embed_kept_rows(mask_dev, cap, out=out)
    assert got.data_ptr() == out.data_ptr()
    return got.cpu()


@pytest.mark.parametrize("n", ROWMAP_N)
def test_embed_kept_rows_equals_the_integer_reference(n):
    ncase = 0
    for name, mask in ER.masks_for(n, seed=n):
        K = int((mask == 0).sum())
        md = mask.cuda()
        fit, over = ER.caps_for(n, K)
        for cap in fit + over:
            want = ER.rowmap_ref(mask, cap)
            got = _rowmap_call(md, cap)
            assert torch.equal(got, want), (f"n {n} mask {name} cap {cap} (kept {K}): {int((got != want).sum())} of {n + 2} entries differ, "
                                            f"first at {int((got != want).nonzero()[0])}")
            if cap < K:    # overflow: the kept tokens behind the capacity read -1, the count is clamped, the flag is up
                assert int(got[n]) == cap and int(got[n + 1]) == 1 and int((got[:n] >= 0).sum()) == cap and int(got[:n].max()) == cap - 1
            else:
                assert int(got[n]) == K and int(got[n + 1]) == 0
            ncase += 1
    assert ncase >= 6


@pytest.mark.parametrize("n", [17, 1000, 4096, 17576, 64000])
def test_embed_kept_rows_with_a_misaligned_mask_pointer(n):
    """a mask that starts one byte behind a 16-byte boundary takes the scalar load16 everywhere: the same row map"""
    mask = ER.masks_for(n, seed=n + 1)[0][1]
    buf = torch.ones(n + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[1:1 + n]
    view.copy_(mask)
    assert view.is_contiguous() and view.data_ptr() % 16 == 1
    K = int((mask == 0).sum())
    for cap in (K, n, max(1, K - 1)):
        aligned = _rowmap_call(mask.cuda(), cap)
        assert torch.equal(_rowmap_call(view, cap), aligned) and torch.equal(aligned, ER.rowmap_ref(mask, cap))


def test_embed_kept_rows_refuses_an_empty_mask_and_a_zero_capacity():
    from nerf_mae_amd._lib import NmhError
    ops = _ops()
    mask = torch.zeros(64, dtype=torch.uint8, device="cuda")
    out = torch.full((66,), POISON, dtype=torch.int32, device="cuda")
    for cap in (0, -1):
        with pytest.raises(NmhError):
            ops.embed_kept_rows(mask, cap, out=out)
    with pytest.raises(NmhError):
        ops.embed_kept_rows(torch.zeros(0, dtype=torch.uint8, device="cuda"), 1)
    with pytest.raises(RuntimeError):
        ops.embed_kept_rows(mask, 64, out=torch.empty(64, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    assert (out == POISON).all(), "a refused call wrote to the row map"


# ---- 2. patch_embed_gather_kept -------------------------------------------------------------------------------------------------------------
def _gather_input(R, B):
    x = torch.randn((B, 4, R, R, R), generator=_gen(R + B)) * 3.0
    x[:, :, 0, 0, :2] = torch.tensor([0.0, -0.0])
    x[:, :, -1, -1, -2:] = torch.tensor([-0.0, 1e-30])
    return _padded_input(x)


def _check_gather(xd, ref_full, A_full, B, R, dt, mask, cap, name):
    """(a) the row of every kept token that has one, bit for bit; (b) the rows behind the kept count +0; (c) the guards around A untouched"""
    g = R // 4
    n = g ** 3
    rm = ER.rowmap_ref(mask, cap)
    rmd = rm.cuda()
    buf, A = _guarded(B * cap, 256, dt)
    _ops().patch_embed_gather_kept(xd, A, B, R, rmd, cap)
    torch.cuda.synchronize()
    Kc = int(rm[n])
    has = (rm[:n] >= 0).cuda()
    rows = rmd[:n][has].long()
    got = A.view(B, cap, 256)
    tag = f"R {R} B {B} {DT_ID[dt]} mask {name} cap {cap} (rows {Kc})"
    assert _guards_untouched(buf, 256), f"{tag}: wrote outside A"
    assert int(has.sum()) == Kc
    assert torch.equal(_bits(got[:, rows]), _bits(ref_full[:, has])), f"{tag}: a kept row is not the index gather of x rounded to the dtype"
    assert torch.equal(_bits(got[:, rows]), _bits(A_full.view(B, n, 256)[:, has])), f"{tag}: a kept row differs from patch_embed_gather's"
    assert (_bits(got[:, Kc:]) == 0).all(), f"{tag}: the rows behind the kept count are not +0"


def _gather_cases(R, B, dt, all_masks=True):
    ops = _ops()
    g = R // 4
    n = g ** 3
    xd = _gather_input(R, B)
    ref_full = ER.im2row_ref(xd, dt)
    A_full = _nan((B * n, 256), dt)
    ops.patch_embed_gather(xd, A_full, B, R)
    torch.cuda.synchronize()
    assert torch.equal(_bits(A_full.view(B, n, 256)), _bits(ref_full)), "patch_embed_gather is not the index gather of x rounded to the dtype"
    masks = ER.masks_for(n, seed=R)
    for name, mask in (masks if all_masks else masks[:2]):
        K = int((mask == 0).sum())
        fit, over = ER.caps_for(n, K)
        for cap in fit:
            _check_gather(xd, ref_full, A_full, B, R, dt, mask, cap, name)
    # more kept tokens than rows (memory safety only: which tokens go without a row is the row map's contract, tested above)
    name, mask = masks[0]
    K = int((mask == 0).sum())
    _check_gather(xd, ref_full, A_full, B, R, dt, mask, K - 1, name + " overflow")
    _check_gather(xd, ref_full, A_full, B, R, dt, mask, 1, name + " overflow")


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("R", [16, 28, 32, 40, 48, 104])
def test_patch_embed_gather_kept_is_bit_exact(R, B, dt):
    """R = 28 / 40: g = 7 / 10, a ragged last run of four tokens; R = 104: g = 26, a two-step row map"""
    _gather_cases(R, B, dt)


def test_patch_embed_gather_kept_full_size():
    _gather_cases(160, 2, BF, all_masks=False)


# ---- 3. / 4. embed_norm_fwd_kept, embed_norm_bwd_kept ---------------------------------------------------------------------------------------
def _ln_masks(g):
    n = g ** 3
    by = dict(ER.masks_for(n, seed=g))
    names = (["block"] if "block" in by else []) + ["bernoulli", "all_removed", "none_removed", "only_last"]
    out = []
    for name in names:
        K = int((by[name] == 0).sum())
        for cap in sorted({max(K, 1), min(n, max(64, -(-K // 64) * 64))}):
            out.append((name, by[name], cap))
    return out


def _ln_setup(C, dt, g, B, mask, cap, seed):
    """compact y0 [B][cap][C]: the kept tokens' rows hold values of the dtype, every other row NaN.  References on the device in float64"""
    n = g ** 3
    gen = _gen(seed)
    rm = ER.rowmap_ref(mask, cap)
    K = int(rm[n])
    assert int(rm[n + 1]) == 0
    buf, y0 = _guarded(B * cap, C, dt)
    y0.view(B, cap, C)[:, :K] = (torch.randn((B, K, C), generator=gen) * 1.5 + 0.3).to(dt).cuda()
    gam = (1 + 0.2 * torch.randn(C, generator=gen)).cuda()
    bet = (0.1 * torch.randn(C, generator=gen)).cuda()
    pos = torch.randn((n, C), generator=gen).cuda()
    mt = (0.1 * torch.randn(C, generator=gen)).cuda()
    return dict(n=n, K=K, rm=rm.cuda(), kept=(rm[:n] >= 0).cuda(), mask=mask.cuda(), buf=buf, y0=y0, gam=gam, bet=bet, pos=pos, mt=mt, gen=gen)


def _check_ln_fwd(C, dt, g, B, name, mask, cap):
    ops = _ops()
    s = _ln_setup(C, dt, g, B, mask, cap, seed=C + g + B)
    n, K, T, kept = s["n"], s["K"], B * s["n"], s["kept"]
    tag = f"fwd {DT_ID[dt]} C{C} g{g} B{B} {name} cap{cap}"
    tok, mean, rstd = _nan((T, C), dt), _nan((T,), torch.float32), _nan((T,), torch.float32)
    ops.embed_norm_fwd_kept(s["y0"], s["gam"], s["bet"], tok, mean, rstd, T, C, s["pos"], s["mask"], s["mt"], n, s["rm"], cap)
    torch.cuda.synchronize()
    assert _guards_untouched(s["buf"], C)
    assert not torch.isnan(tok).any(), f"{tag}: NaN in tok -- a row of y0 that holds no kept token was read, or a row of tok was not written"
    y_tok = ER.scatter_rows(s["y0"].view(B, cap, C).to(F64), s["rm"], n)
    ref, mean_ref, rstd_ref = ER.embed_post_ref(y_tok, s["gam"].to(F64), s["bet"].to(F64), s["pos"].to(F64), s["mask"], s["mt"].to(F64))
    _close(tok, ref.view(T, C), FWD_TOK_TOL[dt], f"{tag} tok")
    removed = ~kept
    assert (_bits(tok.view(B, n, C)[:, removed]) == _bits(s["mt"].to(dt))).all(), f"{tag}: a removed token's row is not mask_token rounded to the dtype"
    # the same instantiation on the same values laid out one row per token: bit-identical
    x_full = ER.scatter_rows(s["y0"].view(B, cap, C), s["rm"], n).view(T, C).contiguous()
    tok2, mean2, rstd2 = _nan((T, C), dt), _nan((T,), torch.float32), _nan((T,), torch.float32)
    ops.layernorm_fwd(x_full, s["gam"], s["bet"], tok2, mean2, rstd2, T, C, pos=s["pos"], mask=s["mask"], mask_token=s["mt"], tokens_per_sample=n)
    torch.cuda.synchronize()
    assert torch.equal(_bits(tok), _bits(tok2)), f"{tag}: tok differs from layernorm_fwd on the same values, one row per token"
    if K:
        _close(mean.view(B, n)[:, kept], mean_ref[:, kept], FWD_STAT_TOL, f"{tag} mean")
        _close(rstd.view(B, n)[:, kept], rstd_ref[:, kept], FWD_STAT_TOL, f"{tag} rstd")
        assert torch.equal(_bits(mean.view(B, n)[:, kept]), _bits(mean2.view(B, n)[:, kept])) and torch.equal(_bits(rstd.view(B, n)[:, kept]), _bits(rstd2.view(B, n)[:, kept]))


def _check_ln_bwd(C, dt, g, B, name, mask, cap):
    ops = _ops()
    s = _ln_setup(C, dt, g, B, mask, cap, seed=2 * C + g + B)
    n, K, T, kept, rm = s["n"], s["K"], B * s["n"], s["kept"], s["rm"]
    tag = f"bwd {DT_ID[dt]} C{C} g{g} B{B} {name} cap{cap}"
    dtok = torch.randn((T, C), generator=s["gen"]).to(dt).cuda()
    # float64 autograd of the forward, on one row per token
    y_tok = ER.scatter_rows(s["y0"].view(B, cap, C).to(F64), rm, n).requires_grad_(True)
    ps = [s[k].to(F64).requires_grad_(True) for k in ("gam", "bet", "mt")]
    ref, mean_ref, rstd_ref = ER.embed_post_ref(y_tok, ps[0], ps[1], s["pos"].to(F64), s["mask"], ps[2])
    dy_ref, dg_ref, db_ref, dm_ref = torch.autograd.grad((ref * dtok.view(B, n, C).to(F64)).sum(), [y_tok] + ps)
    # mean / rstd as the forward leaves them for the kept tokens (the float64 values rounded to fp32); NaN for the removed ones: they must not reach any output
    nanrow = torch.full_like(mean_ref, float("nan"))
    mean = torch.where(kept[None], mean_ref.detach(), nanrow).float().view(T).contiguous()
    rstd = torch.where(kept[None], rstd_ref.detach(), nanrow).float().view(T).contiguous()
    rows = rm[:n][kept].long()
    runs = []
    for pre in (None, s["gen"]):
        P = [torch.zeros(C) if pre is None else torch.randn(C, generator=pre) * 3.0 for _ in range(3)]
        dgam, dbet, dmt = [p.clone().cuda() for p in P]
        buf, dy0 = _guarded(B * cap, C, dt)
        ops.embed_norm_bwd_kept(dtok, s["y0"], s["gam"], mean, rstd, dy0, dgam, dbet, T, C, s["mask"], dmt, n, rm, cap)
        torch.cuda.synchronize()
        assert _guards_untouched(buf, C), f"{tag}: wrote outside dy0"
        d3 = dy0.view(B, cap, C)
        assert (_bits(d3[:, K:]) == 0).all(), f"{tag}: the rows behind the kept count of dy0 are not +0 (they are operands of the weight gradient)"
        assert torch.isfinite(d3[:, :K]).all(), f"{tag}: a kept row of dy0 was not written"
        if K:
            _close(d3[:, rows], dy_ref[:, kept], BWD_DY0_TOL[dt], f"{tag} dy0")
        # the accumulators are added to, not overwritten: the pre-loaded value comes off again in float64
        sums = [(a.double().cpu() - p.double()) for a, p in zip((dgam, dbet, dmt), P)]
        for a, r, nm in zip(sums, (dg_ref, db_ref, dm_ref), ("dgamma", "dbeta", "dmask_token")):
            _close(a, r.cpu(), BWD_PARAM_TOL[dt], f"{tag} {nm}{'' if pre is None else ' (+=)'}")
        runs.append((d3.clone(), sums))
    assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])), f"{tag}: dy0 differs between two runs"
    for a, b, nm in zip(runs[0][1], runs[1][1], ("dgamma", "dbeta", "dmask_token")):
        if b.abs().max() > 0:
            d = relerr(a, b)
            print(f"  [{tag} {nm}] run to run {d:.2e}")
            assert d <= RUN_TO_RUN_TOL, f"{tag} {nm}: two runs differ by {d:.2e} of the largest entry"
        else:
            assert a.abs().max() == 0


LN_CASES = [(C, g, B) for C in (96, 128, 192) for g in (7, 8, 10, 16) for B in (1, 3)]


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("C,g,B", LN_CASES)
def test_embed_norm_fwd_kept(C, g, B, dt):
    for name, mask, cap in _ln_masks(g):
        _check_ln_fwd(C, dt, g, B, name, mask, cap)


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("C,g,B", LN_CASES)
def test_embed_norm_bwd_kept(C, g, B, dt):
    for name, mask, cap in _ln_masks(g):
        _check_ln_bwd(C, dt, g, B, name, mask, cap)


# ---- 5. the chain ---------------------------------------------------------------------------------------------------------------------------
class _InBackward(torch.autograd.Function):
    """runs fn inside a backward pass, where ops.WgradQueue.add may install its end-of-backward callback (as it does under _EmbedFn.backward)"""

    @staticmethod
    def forward(ctx, a, fn):
        ctx.fn = fn
        return a.clone()

    @staticmethod
    def backward(ctx, g):
        ctx.fn()
        return g, None


def _check_chain(R, B, C, dt, cap_mode, seed):
    from oracle import mae3d_oracle as O
    from nerf_mae_amd.model import embed_capacity_rows
    ops = _ops()
    g = R // 4
    n, T = g ** 3, B * g ** 3
    gen = _gen(seed)
    mask = O.draw_block_mask((g, g, g), 0.75, rng=random.Random(seed)).to(torch.uint8).reshape(-1)
    K = int((mask == 0).sum())
    cap = K if cap_mode == "kept" else min(n, embed_capacity_rows(g, p_remove=0.75))
    assert 0 < K <= cap
    tag = f"chain {DT_ID[dt]} R{R} B{B} C{C} cap {cap} (kept {K} of {n})"
    x = _padded_input(torch.randn((B, 4, R, R, R), generator=gen))
    w = (torch.randn((C, 4, 4, 4, 4), generator=gen) / 16.0).to(dt)
    bias, gam, bet = 0.5 + 0.1 * torch.randn(C, generator=gen), 1 + 0.2 * torch.randn(C, generator=gen), 0.1 * torch.randn(C, generator=gen)
    pos, mt = torch.randn((n, C), generator=gen), 0.1 * torch.randn(C, generator=gen)
    dtok = torch.randn((T, C), generator=gen).to(dt)
    md, wd, biasd, gamd, betd, posd, mtd, dtokd = [t.cuda() for t in (mask, w, bias, gam, bet, pos, mt, dtok)]
    # forward
    rowmap = torch.full((n + 2,), POISON, dtype=torch.int32, device="cuda")
    ops.embed_kept_rows(md, cap, out=rowmap)
    bufA, A = _guarded(B * cap, 256, dt)
    ops.patch_embed_gather_kept(x, A, B, R, rowmap, cap)
    y0 = ops.gemm_nt(A, wd.view(C, 256), bias=biasd)
    tok, mean, rstd = _nan((T, C), dt), _nan((T,), torch.float32), _nan((T,), torch.float32)
    ops.embed_norm_fwd_kept(y0, gamd, betd, tok, mean, rstd, T, C, posd, md, mtd, n, rowmap, cap)
    # backward and weight gradient
    bufD, dy0 = _guarded(B * cap, C, dt)
    dgam, dbet, dmt, dbias = [torch.zeros(C, device="cuda") for _ in range(4)]
    dW = torch.zeros((C, 256), device="cuda")
    ops.embed_norm_bwd_kept(dtokd, y0, gamd, mean, rstd, dy0, dgam, dbet, T, C, md, dmt, n, rowmap, cap)
    if dt == BF:   # the grouped queue, as _EmbedFn.backward issues it
        q = ops.WgradQueue()

        def wgrad():
            q.add(dy0, A, dW, dbias=dbias, rows_per_sample=cap)
            q.flush(foreground=True)
            q.join()
        _InBackward.apply(torch.zeros(1, requires_grad=True), wgrad).sum().backward()
    else:
        ops.gemm_tn(dy0, A, dW, dbias=dbias)
    torch.cuda.synchronize()
    assert torch.equal(rowmap.cpu(), ER.rowmap_ref(mask, cap)), f"{tag}: row map"
    assert _guards_untouched(bufA, 256) and _guards_untouched(bufD, C), f"{tag}: wrote outside A or dy0"
    assert (_bits(A.view(B, cap, 256)[:, K:]) == 0).all() and (_bits(dy0.view(B, cap, C)[:, K:]) == 0).all(), f"{tag}: tail rows of A or dy0 are not +0"
    assert not torch.isnan(tok).any(), f"{tag}: NaN in tok"
    # float64 from the definition, on the values the kernels see: x and w rounded to the dtype, fp32 parameters
    ref, (dW_ref, db_ref, dg_ref, dbeta_ref, dm_ref) = ER.chain_ref(x.cpu().to(dt).to(F64), w.to(F64), bias.to(F64), gam.to(F64), bet.to(F64), pos.to(F64), mask,
                                                                    mt.to(F64), dtok.to(F64))
    _close(tok, ref.view(T, C), CHAIN_TOK_TOL[dt], f"{tag} tok")
    for got, want, nm in ((dW, dW_ref.view(C, 256), "dW"), (dbias, db_ref, "db"), (dgam, dg_ref, "dgamma"), (dbet, dbeta_ref, "dbeta"), (dmt, dm_ref, "dmask_token")):
        _close(got, want, CHAIN_GRAD_TOL[dt], f"{tag} {nm}")


@pytest.mark.parametrize("dt", DTS, ids=DT_ID.get)
@pytest.mark.parametrize("cap_mode", ["kept", "captured"])
@pytest.mark.parametrize("R", [32, 40, 48])
def test_embed_kept_chain(R, cap_mode, dt):
    """cap = the kept count, and cap = embed_capacity_rows(g, p_remove=0.75): what a captured step runs with (tail rows: +0 in A, the bias in y0, +0 in dy0)"""
    for C in (96, 128):
        _check_chain(R, 2, C, dt, cap_mode, seed=R + C)


def test_embed_kept_chain_full_size():
    """160^3, two samples, bf16, a captured step's capacity: thousands of tail rows per sample hold the GEMM's bias in y0, not zero, so a backward that left
    dy0's tail alone would show in db first"""
    _check_chain(160, 2, 96, BF, "captured", seed=160)
