"""The FCOS head on the GPU (nerf_mae_amd.fcos.FCOSHead over csrc/fcos_head.hip and the channels-last convolutions) against the float64 restatement of
tests/_fcos_head_ref.py (itself checked against the recorded reference in tests/test_fcos_head_ref_cpu.py).

(a) The GroupNorm kernels alone (ops.fcos_gn_stats / _apply / _bwd), every level and both towers in one call, on inputs the compute dtype holds exactly.  fp32:
    assert_close(1e-3), the project's fp32 contract.  bf16: the statistics and the parameter gradients are fp64 / fp32 sums of exact inputs, 1e-3 as well; y and dx
    are STORED in bf16, one rounding of at most 2^-9 relative, and are held to 2^-8 (the factor 2 covers roundings that flip at a bf16 boundary).  The backward is
    given the float64 y (rounded to the compute dtype) and the float64 statistics, so that its ReLU mask is the reference's.
(b) fp32 groups with mean 30 and standard deviation 0.05, and a constant group (variance 0: relu(beta)), at 1e-3: a single-pass fp32 sum of squares loses the variance.
(c) The output stage alone (ops.fcos_head_out_fwd / _bwd / _wgrad), forward and backward, against float64 convolutions: outputs, weight, bias and Scale gradients at
    1e-3 (in bf16 the gradient enters the weight-gradient product as hi + lo, 16 mantissa bits); the 16-column gradient is stored in the compute dtype (2^-8 in bf16)
    and its input-gradient convolution is compared with the float64 convolution of that ROUNDED gradient, which leaves the fp32 accumulation and one store (2^-8).
(d) The module.  fp32: 1e-3 on all outputs and gradients.  bf16: per quantity e_round = the max-norm error, relative to the tensor's largest entry, of the
    rounding-aware restatement against the unrounded one, computed on the CPU; the kernels are held to 2 e_round against the UNROUNDED float64 result (1e-3 where
    e_round is 0).  Measured values: DESIGN.md 3.15.
(e) Strict load_state_dict of the recorded reference parameters, reproducing the recorded outputs and gradients.
Every kernel result is bit-identical between two runs, and gradient buffers start at one to prove the +=."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_head_ref as H  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
FOUR = ((12, 11, 10), (7, 6, 5), (5, 4, 3), (2, 1, 1))
STORE_TOL = 2.0 ** -8
F64 = torch.float64


def _m():
    from nerf_mae_amd import fcos, ops
    return ops, fcos


def _tol(dtype):
    return 1e-3 if dtype == torch.float32 else STORE_TOL


def _cl(x):
    """NCDHW -> channels-last"""
    return x.permute(0, 2, 3, 4, 1).contiguous()


def _nc(x):
    """channels-last -> NCDHW"""
    return x.permute(0, 4, 1, 2, 3).contiguous()


# ---- (a) the GroupNorm kernels -------------------------------------------------------------------------------------------------------------------
GN_CASES = [(dtype, C, N) for dtype in (torch.float32, torch.bfloat16) for C in (32, 64, 256) for N in (1, 3)]


def _gn_ref(x, gamma, beta, dy, y_in, groups=H.GROUPS, eps=H.EPS):
    """x, dy, y_in: channels-last float64 -> statistics, y, and the backward written out with the mask of y_in"""
    N, C = x.shape[0], x.shape[-1]
    xg = _nc(x).reshape(N, groups, -1)
    mean = xg.mean(2)
    rstd = 1.0 / torch.sqrt(((xg - mean[:, :, None]) ** 2).mean(2) + eps)
    y = _cl(F.relu(H.group_norm(_nc(x), gamma, beta, groups, eps)))
    if dy is None:
        return torch.stack([mean, rstd], dim=2), y, None, None, None
    xh = _cl(((xg - mean[:, :, None]) * rstd[:, :, None]).reshape(_nc(x).shape))
    dm = dy * (y_in > 0)
    dgamma, dbeta = (dm * xh).sum((0, 1, 2, 3)), dm.sum((0, 1, 2, 3))
    dh = dm * gamma
    grp = lambda t: _nc(t).reshape(N, groups, -1)
    m1, m2 = grp(dh).mean(2, keepdim=True), (grp(dh) * grp(xh)).mean(2, keepdim=True)
    dx = _cl(((grp(dh) - m1 - grp(xh) * m2) * rstd[:, :, None]).reshape(_nc(x).shape))
    return torch.stack([mean, rstd], dim=2), y, dx, dgamma, dbeta


@functools.lru_cache(maxsize=None)
def gn_case(dtype, C, N):
    g = torch.Generator().manual_seed(C * 10 + N)
    cast = lambda v: v.to(dtype).double()
    gam = [(1.0 + 0.3 * torch.randn(C, generator=g)).float().double() for _ in (0, 1)]
    bet = [(0.4 * torch.randn(C, generator=g)).float().double() for _ in (0, 1)]
    jobs = []
    dgam, dbet = [torch.zeros(C, dtype=F64) for _ in (0, 1)], [torch.zeros(C, dtype=F64) for _ in (0, 1)]
    for grid in FOUR:
        for t in (0, 1):
            x = cast(torch.randn((N, *grid, C), generator=g) * 1.5 + 0.3)
            dy = cast(torch.randn((N, *grid, C), generator=g))
            _, y, _, _, _ = _gn_ref(x, gam[t], bet[t], None, None)
            y_in = cast(y)
            stats, y, dx, dg, db = _gn_ref(x, gam[t], bet[t], dy, y_in)
            dgam[t] += dg
            dbet[t] += db
            jobs.append(dict(t=t, x=x, dy=dy, y=y, y_in=y_in, stats=stats, dx=dx))
    return dict(jobs=jobs, gam=gam, bet=bet, dgam=dgam, dbet=dbet)


def _gn_run(ops, c, dtype):
    jobs = c["jobs"]
    xs = [j["x"].to(dtype).cuda() for j in jobs]
    towers = [j["t"] for j in jobs]
    gam, bet = [v.float().cuda() for v in c["gam"]], [v.float().cuda() for v in c["bet"]]
    stats = ops.fcos_gn_stats(xs, H.GROUPS)
    ys = ops.fcos_gn_apply(xs, towers, stats, gam, bet, H.GROUPS)
    ref_stats = torch.stack([j["stats"] for j in jobs]).float().cuda()
    dgam, dbet = [torch.ones_like(v) for v in gam], [torch.ones_like(v) for v in bet]        # += : the buffers start at one
    dxs = ops.fcos_gn_bwd([j["dy"].to(dtype).cuda() for j in jobs], xs, [j["y_in"].to(dtype).cuda() for j in jobs], towers, ref_stats, gam, dgam, dbet, H.GROUPS)
    return stats, ys, dxs, dgam, dbet


@pytest.mark.parametrize("dtype,C,N", GN_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_groupnorm_kernels_against_float64(dtype, C, N):
    ops, _ = _m()
    c = gn_case(dtype, C, N)
    stats, ys, dxs, dgam, dbet = _gn_run(ops, c, dtype)
    assert tuple(stats.shape) == (len(c["jobs"]), N, H.GROUPS, 2) and stats.dtype == torch.float32
    tag = f"{dtype} C {C} N {N}"
    for k, j in enumerate(c["jobs"]):
        assert_close(stats[k].cpu(), j["stats"], 1e-3, f"{tag} stats {k}")
        assert ys[k].dtype == dtype and dxs[k].dtype == dtype
        assert_close(ys[k].double().cpu(), j["y"], _tol(dtype), f"{tag} y {k}")
        assert (ys[k] >= 0).all()
        assert_close(dxs[k].double().cpu(), j["dx"], _tol(dtype), f"{tag} dx {k}")
    for t in (0, 1):
        assert_close(dgam[t].double().cpu() - 1.0, c["dgam"][t], 1e-3, f"{tag} dgamma {t}")
        assert_close(dbet[t].double().cpu() - 1.0, c["dbet"][t], 1e-3, f"{tag} dbeta {t}")
    again = _gn_run(ops, c, dtype)
    for a, b in zip([stats, *ys, *dxs, *dgam, *dbet], [again[0], *again[1], *again[2], *again[3], *again[4]]):
        assert torch.equal(a, b), "two runs are bit-identical"


# ---- (b) |mean| >> std and a constant group ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [64, 256])
def test_groupnorm_with_a_large_mean_and_a_constant_group(C):
    ops, _ = _m()
    g = torch.Generator().manual_seed(C)
    N, grid, cpg = 2, (5, 4, 3), C // H.GROUPS
    x = (30.0 + 0.05 * torch.randn((N, *grid, C), generator=g)).float()
    x[..., 3 * cpg:4 * cpg] = 7.25           # group 3 is constant: variance 0
    gamma, beta = (1.0 + 0.3 * torch.randn(C, generator=g)).float(), (0.4 * torch.randn(C, generator=g)).float()
    want_stats, want_y, _, _, _ = _gn_ref(x.double(), gamma.double(), beta.double(), None, None)
    xs = [x.cuda()]
    stats = ops.fcos_gn_stats(xs, H.GROUPS)
    y = ops.fcos_gn_apply(xs, [1], stats, [None, gamma.cuda()], [None, beta.cuda()], H.GROUPS)[0]
    assert_close(stats[0].cpu(), want_stats, 1e-3, f"C {C} stats")
    assert abs(float(want_stats[0, 0, 1]) - 20.0) < 5.0 and abs(float(want_stats[0, 3, 1]) - 1e-5 ** -0.5) < 1e-6
    assert_close(y.double().cpu(), want_y, 1e-3, f"C {C} y")
    assert torch.equal(y[..., 3 * cpg:4 * cpg].cpu(), F.relu(beta[3 * cpg:4 * cpg]).expand(N, *grid, cpg)), "a constant group gives relu(beta) exactly"


# ---- (c) the output stage ------------------------------------------------------------------------------------------------------------------------
TWO = ((7, 6, 5), (2, 1, 1))
#            dtype           C    obb    on_reg  mode     grids              N  sparse
OUT_CASES = [
    (torch.float32,   32, False, True,  "train", FOUR,              3, False),
    (torch.float32,   32, True,  False, "eval",  FOUR,              1, True),
    (torch.float32,  256, True,  True,  "exp",   TWO,               1, False),
    (torch.float32,  256, False, False, "train", ((5, 4, 3),),      3, True),
    (torch.bfloat16,  32, True,  True,  "train", FOUR,              3, True),
    (torch.bfloat16,  32, False, False, "exp",   FOUR,              1, False),
    (torch.bfloat16, 256, False, True,  "eval",  TWO,               3, False),
    (torch.bfloat16, 256, True,  False, "train", ((12, 11, 10),),   1, True),
]
SCALES = (1.3, -0.7, 0.5, 2.0)
STRIDES = (4, 8, 16, 32)


def _w16(P, nreg, on_reg):
    """the two towers' 16-row weights (csrc/fcos_head.hip: tower columns), float64 [16, C, 3, 3, 3]"""
    C = P["cls_logits.weight"].shape[1]
    w = [torch.zeros((16, C, 3, 3, 3), dtype=F64) for _ in (0, 1)]
    w[0][0] = P["cls_logits.weight"][0]
    w[1][:nreg] = P["bbox_pred.weight"]
    w[1 if on_reg else 0][nreg if on_reg else 1] = P["centerness.weight"][0]
    return w


@functools.lru_cache(maxsize=None)
def out_case(dtype, C, obb, on_reg, mode, grids, N, sparse):
    g = torch.Generator().manual_seed(C + 7 * obb + 3 * on_reg + len(grids))
    cast = lambda v: v.to(dtype).double()
    nreg, L = 8 if obb else 6, len(grids)
    P = {}
    for name, n in (("cls_logits", 1), ("bbox_pred", nreg), ("centerness", 1)):
        P[f"{name}.weight"] = cast(torch.randn((n, C, 3, 3, 3), generator=g) * (1.0 / (C * 27)) ** 0.5)
        P[f"{name}.bias"] = (0.5 * torch.randn(n, generator=g)).float().double()
    for l in range(L):
        P[f"scales.{l}.scale"] = torch.tensor([SCALES[l]], dtype=F64)
    P = {k: v.requires_grad_(True) for k, v in P.items()}
    acts, us, outs, cots = [], [], [], []
    total = 0.0
    for l, grid in enumerate(grids):
        pair = []
        for _ in (0, 1):
            a = torch.randn((N, *grid, C), generator=g)
            a[torch.rand(a.shape, generator=g) < 0.1] = 0.0
            pair.append(cast(a).requires_grad_(True))
        a_cls, a_box = _nc(pair[0]), _nc(pair[1])
        cls = F.conv3d(a_cls, P["cls_logits.weight"], P["cls_logits.bias"], padding=1)
        ctr = F.conv3d(a_box if on_reg else a_cls, P["centerness.weight"], P["centerness.bias"], padding=1)
        u = F.conv3d(a_box, P["bbox_pred.weight"], P["bbox_pred.bias"], padding=1)
        u.retain_grad()
        reg = H.epilogue(u, P[f"scales.{l}.scale"], mode, STRIDES[l])
        cot = [torch.randn(o.shape, generator=g).double() for o in (cls, reg, ctr)]
        if sparse:
            keep = torch.zeros((N, 1, *grid), dtype=F64)
            for i in range(N):
                for _ in range(7):
                    w, ll, h = [int(torch.randint(s, (1,), generator=g)) for s in grid]
                    keep[i, 0, w, ll, h] = 1
            cot = [c * keep for c in cot]
        total = total + sum((o * c).sum() for o, c in zip((cls, reg, ctr), cot))
        acts.append(pair); us.append(u); outs.append((cls, reg, ctr)); cots.append(cot)
    total.backward()
    # the 16-column gradient per (level, tower), channels-last, and the input gradients from its rounded value
    w16 = _w16({k: v.detach() for k, v in P.items()}, nreg, on_reg)
    g16, dact = [], []
    for l, grid in enumerate(grids):
        G = [torch.zeros((N, 16, *grid), dtype=F64) for _ in (0, 1)]
        G[0][:, 0:1] = cots[l][0]
        G[1][:, :nreg] = us[l].grad
        G[1 if on_reg else 0][:, nreg if on_reg else 1] = cots[l][2][:, 0]
        g16.append([_cl(v) for v in G])
        dact.append([_cl(torch.nn.grad.conv3d_input((N, C, *grid), w16[t], cast(G[t]), padding=1)) for t in (0, 1)])
    return dict(P={k: v.detach() for k, v in P.items()}, dP={k: v.grad for k, v in P.items()}, acts=[[a.detach() for a in p] for p in acts], us=[u.detach() for u in us],
                outs=[[o.detach() for o in os_] for os_ in outs], cots=cots, g16=g16, dact=dact, w16=w16, nreg=nreg)


def _out_run(ops, c, dtype, on_reg, mode):
    L, nreg, C = len(c["acts"]), c["nreg"], c["w16"][0].shape[1]
    P = c["P"]
    acts = [tuple(a.to(dtype).cuda() for a in pair) for pair in c["acts"]]
    wf = [w.reshape(16, C, 27).permute(0, 2, 1).contiguous().to(dtype).cuda() for w in c["w16"]]              # [16][27][C]
    wd = [w.reshape(16, C, 27).flip(2).permute(1, 2, 0).contiguous().to(dtype).cuda() for w in c["w16"]]      # [C][27 flipped][16]
    scales = [P[f"scales.{l}.scale"].float().cuda() for l in range(L)]
    bias = [P[f"{n}.bias"].float().cuda() for n in ("cls_logits", "bbox_pred", "centerness")]
    cls, reg, ctr, u = ops.fcos_head_out_fwd(acts, wf, *bias, scales, STRIDES[:L], nreg, on_reg, mode)
    grads = {k: torch.ones(v.shape, dtype=torch.float32).cuda() for k, v in P.items()}                          # += : the buffers start at one
    cot = [[t.float().cuda() for t in level] for level in c["cots"]]
    g16, gt = ops.fcos_head_out_bwd(acts, [t[0] for t in cot], [t[1] for t in cot], [t[2] for t in cot], u, scales, STRIDES[:L], nreg, on_reg, mode,
                                    grads["cls_logits.bias"], grads["bbox_pred.bias"], grads["centerness.bias"], [grads[f"scales.{l}.scale"] for l in range(L)])
    ops.fcos_head_out_wgrad(acts, gt, nreg, on_reg, grads["cls_logits.weight"], grads["bbox_pred.weight"], grads["centerness.weight"])
    dact = [[ops.conv3d_k3(g16[l][t], wd[t], C) for t in (0, 1)] for l in range(L)]
    return cls, reg, ctr, u, g16, dact, grads


@pytest.mark.parametrize("case", OUT_CASES, ids=lambda c: f"{str(c[0])[6:]}-c{c[1]}-{'obb' if c[2] else 'aabb'}-{'reg' if c[3] else 'cls'}-{c[4]}-{len(c[5])}lv-n{c[6]}-{'sparse' if c[7] else 'dense'}")
def test_output_stage_against_float64(case):
    ops, _ = _m()
    dtype, C, obb, on_reg, mode, grids, N, sparse = case
    c = out_case(*case)
    assert all((a == 0).any() and (a < 0).any() for p in c["acts"] for a in p if a.numel() >= 64), "the activations hold exact zeros and negatives"
    assert len(grids) == 1 or min(SCALES[:len(grids)]) < 0, "one level has a negative scale"
    cls, reg, ctr, u, g16, dact, grads = _out_run(ops, c, dtype, on_reg, mode)
    tag = f"{dtype} C {C} obb {obb} on_reg {on_reg} {mode}"
    for l, grid in enumerate(grids):
        for name, got, want in zip(("logits", "bbox_reg", "centerness"), (cls[l], reg[l], ctr[l]), c["outs"][l]):
            assert got.dtype == torch.float32 and got.is_contiguous() and got.shape == want.shape
            assert_close(got.cpu(), want, 1e-3, f"{tag} {name} {l}")
        assert_close(u[l].cpu(), c["us"][l], 1e-3, f"{tag} u {l}")
        if mode != "exp":
            assert ((reg[l][:, :6] == 0) == (c["outs"][l][1][:, :6] == 0).cuda()).float().mean() > 0.999, "the ReLU reaches columns 0-5 only"
        for t in (0, 1):
            got, want = g16[l][t].double().cpu(), c["g16"][l][t]
            assert g16[l][t].dtype == dtype
            if want.abs().sum() > 0:
                assert_close(got, want, _tol(dtype), f"{tag} g16 {l} tower {t}")
            assert (got[want == 0] == 0).all(), "the packed gradient is exactly zero where the mask or the gradient is"
            if c["dact"][l][t].abs().sum() > 0:
                assert_close(dact[l][t].double().cpu(), c["dact"][l][t], _tol(dtype), f"{tag} input gradient {l} tower {t}")
    for k, want in c["dP"].items():
        assert_close(grads[k].double().cpu() - 1.0, want, 1e-3, f"{tag} d {k}")
    again = _out_run(ops, c, dtype, on_reg, mode)
    flat = lambda r: [*r[0], *r[1], *r[2], *r[3], *[t for p in r[4] for t in p], *r[6].values()]
    for a, b in zip(flat((cls, reg, ctr, u, g16, dact, grads)), flat(again)):
        assert torch.equal(a, b), "two runs are bit-identical"


def test_error_paths():
    ops, fcos = _m()
    x = torch.zeros(1, 2, 2, 2, 32).cuda()
    with pytest.raises(RuntimeError):
        ops.fcos_gn_stats([x.cpu()], 32)
    with pytest.raises(NotImplementedError):
        ops.fcos_gn_stats([torch.zeros(1, 2, 2, 2, 48).cuda()], 16)
    with pytest.raises(NotImplementedError):
        ops.fcos_gn_stats([torch.zeros(1, 2, 2, 2, 96).cuda()], 32)          # 3 channels per group
    with pytest.raises(ValueError):
        ops.fcos_gn_stats([x] * 11, 32)
    head = fcos.FCOSHead(32, 1, [4, 8, 16, 32, 64, 128]).cuda()
    with pytest.raises(ValueError):
        head([torch.zeros(1, 32, 2, 2, 2).cuda()] * 6)                          # the reference has 5 scales
    with pytest.raises(ValueError):
        head.forward_channels_last([x])                                          # fp32 features into a bf16 head
    with pytest.raises(RuntimeError):
        head([torch.zeros(1, 32, 2, 2, 2)])
    with pytest.raises(RuntimeError):
        fcos.FCOSHead(32, 1, [4])([torch.zeros(1, 32, 2, 2, 2).cuda()])       # parameters on the host


# ---- (d) the module ------------------------------------------------------------------------------------------------------------------------------
MOD_GRIDS = ((5, 4, 3), (3, 2, 2), (2, 1, 2))
MOD_STRIDES = (4, 8, 16)
MOD_CASES = [(depth, obb) for depth in (0, 1, 4) for obb in (False, True)]


@functools.lru_cache(maxsize=None)
def mod_case(depth, obb, mode="train", C=64, N=2, grids=MOD_GRIDS, want_rounded=True):
    nreg, on_reg = 8 if obb else 6, not obb
    P = H.make_params(100 + depth * 2 + obb, depth, C, nreg)
    feats = [f.float().double() for f in H.make_features(200 + depth, N, C, grids)]
    g = torch.Generator().manual_seed(300 + depth)
    cots = tuple([torch.randn((N, n, *gr), generator=g).double() for gr in grids] for n in (1, nreg, 1))
    args = (feats, P, depth, on_reg, mode, MOD_STRIDES, cots)
    return dict(P=P, feats=feats, cots=cots, exact=H.run(*args), rounded=H.run(*args, H.round_bf16) if want_rounded else None, C=C, on_reg=on_reg, mode=mode)


def _quantities(res):
    out = {"logits": res["cls"], "bbox_reg": res["reg"], "centerness": res["ctr"], "d features": res["dfeat"]}
    out.update({f"d {k}": [v] for k, v in res["dparam"].items()})
    return out


def _mod_run(fcos, c, depth, obb, dtype, channels_last=False):
    head = fcos.FCOSHead(c["C"], depth, list(MOD_STRIDES), norm_reg_targets=c["mode"] != "exp", centerness_on_reg=c["on_reg"], use_obb=obb, compute_dtype=dtype)
    head.load_state_dict({k: v.float() for k, v in c["P"].items()}, strict=True)
    head = head.cuda().train(c["mode"] != "eval")
    feats = [f.float().cuda().requires_grad_(True) for f in c["feats"]]
    if channels_last:
        ops, _ = _m()
        outs = head.forward_channels_last([ops.ncdhw_to_ndhwc(f.detach(), dtype) for f in feats])
    else:
        outs = head(feats)
        sum((o * t.float().cuda()).sum() for os_, ts in zip(outs, c["cots"]) for o, t in zip(os_, ts)).backward()
    L = len(feats)
    dparam = {k: p.grad for k, p in head.named_parameters() if not k.startswith("scales.") or int(k.split(".")[1]) < L}
    return dict(cls=[o.detach() for o in outs[0]], reg=[o.detach() for o in outs[1]], ctr=[o.detach() for o in outs[2]], dfeat=[f.grad for f in feats], dparam=dparam)


def _fp32_check(fcos, c, depth, obb, tag):
    got = _mod_run(fcos, c, depth, obb, torch.float32)
    assert list(got["dparam"]) == list(c["exact"]["dparam"])
    want = _quantities(c["exact"])
    for name, ts in _quantities(got).items():
        for k, (a, b) in enumerate(zip(ts, want[name])):
            assert a is not None, f"{name} {k}: no gradient"
            assert_close(a.cpu(), b, 1e-3, f"{tag} {name} {k}")


@pytest.mark.parametrize("depth,obb", MOD_CASES)
def test_module_fp32_against_float64(depth, obb):
    _, fcos = _m()
    _fp32_check(fcos, mod_case(depth, obb), depth, obb, f"fp32 depth {depth} obb {obb}")


@pytest.mark.parametrize("mode", ["eval", "exp"])
def test_module_fp32_in_the_evaluation_and_exp_modes(mode):
    _, fcos = _m()
    _fp32_check(fcos, mod_case(1, True, mode, want_rounded=False), 1, True, f"fp32 {mode}")


def _bf16_check(fcos, c, depth, obb, tag):
    want, rnd = _quantities(c["exact"]), _quantities(c["rounded"])
    e_round = {name: H.max_err(rnd[name], want[name]) for name in want}
    got = _quantities(_mod_run(fcos, c, depth, obb, torch.bfloat16))
    e_kernel = {name: H.max_err([t.cpu() for t in got[name]], want[name]) for name in want}
    print(f"{tag}: e_round {max(e_round.values()):.3e}  kernel {max(e_kernel.values()):.3e}")
    assert max(e_round.values()) > 0
    for name in want:
        # a quantity that no stored tensor reaches (the gradients of the cls_logits and centerness biases are plain sums of the cotangent) has e_round 0: the fp32 contract
        bound = 2 * e_round[name] if e_round[name] > 0 else 1e-3
        print(f"    {name:28s} e_round {e_round[name]:.3e}  kernel {e_kernel[name]:.3e}  bound {bound:.3e}")
        assert e_kernel[name] <= bound, f"{tag} {name}: kernel error {e_kernel[name]:.3e} > {bound:.3e} (e_round {e_round[name]:.3e})"


@pytest.mark.parametrize("depth,obb", MOD_CASES)
def test_module_bf16_within_twice_the_rounding_error(depth, obb):
    _, fcos = _m()
    _bf16_check(fcos, mod_case(depth, obb), depth, obb, f"bf16 depth {depth} obb {obb}")


def test_module_bf16_on_the_64_channel_block_convolution():
    """64 channels and a 32^3 level: ops.use_conv64 holds, so both towers' LDS-halo conv with the bias epilogue and its dgrad run; the second level takes the
    generic conv"""
    ops, fcos = _m()
    c = mod_case(1, False, C=64, N=1, grids=((32, 32, 32), (3, 2, 2)))
    assert ops.use_conv64(torch.empty(1, 32, 32, 32, 64, dtype=torch.bfloat16), 64)
    assert not ops.use_conv64(torch.empty(1, 3, 2, 2, 64, dtype=torch.bfloat16), 64)
    _bf16_check(fcos, c, 1, False, "bf16 conv64 depth 1")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ncdhw_entry_equals_the_channels_last_entry_bit_for_bit(dtype):
    _, fcos = _m()
    c = mod_case(4, True)
    a, b = _mod_run(fcos, c, 4, True, dtype), _mod_run(fcos, c, 4, True, dtype, channels_last=True)
    assert all(torch.equal(x, y) for n in ("cls", "reg", "ctr") for x, y in zip(a[n], b[n]))
    again = _mod_run(fcos, c, 4, True, dtype)
    for n, ts in _quantities(a).items():        # fixed-order sums: the outputs and the output stage's gradients (the tower convs' weight and bias gradients add atomically)
        if "tower" not in n and n != "d features":
            assert all(torch.equal(x, y) for x, y in zip(ts, _quantities(again)[n])), f"{n}: two runs are bit-identical"


# ---- (e) the recorded reference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_obb,ctr_on_reg,training", H.G_CASES)
def test_reference_checkpoint_loads_strictly_and_reproduces_the_recorded_outputs(use_obb, ctr_on_reg, training):
    _, fcos = _m()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g24_fcos_head.npz")))
    feats, P, cots, mode, rec = H.golden_case(g, use_obb, ctr_on_reg, training)
    head = fcos.FCOSHead(H.G_C, H.G_CONVS, list(H.G_STRIDES), centerness_on_reg=ctr_on_reg, use_obb=use_obb, compute_dtype=torch.float32)
    head.load_state_dict({k: v.float() for k, v in P.items()}, strict=True)
    head = head.cuda().train(training)
    xs = [f.float().cuda().requires_grad_(True) for f in feats]
    outs = head(xs)
    sum((o * t.float().cuda()).sum() for os_, ts in zip(outs, cots) for o, t in zip(os_, ts)).backward()
    for n, os_ in zip(("cls", "reg", "ctr"), outs):
        for k, o in enumerate(os_):
            assert_close(o.cpu(), rec[n][k], 1e-3, f"g24 {n} {k}")
    for k in range(len(feats)):
        assert_close(xs[k].grad.cpu(), rec["dfeat"][k], 1e-3, f"g24 d features {k}")
    grads = dict(head.named_parameters())
    for name, want in rec["dparam"].items():
        assert_close(H.recorded_view(name, grads[name].grad.cpu()), want, 1e-3, f"g24 d {name}")
