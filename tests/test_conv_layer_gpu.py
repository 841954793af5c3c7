"""The detector's shared pieces one by one against float64 on the host: the biased 3x3x3 layer (nerf_mae_amd.conv_layer over the implicit-GEMM conv, the
64-channel-block LDS-halo conv and the three weight-gradient kernels), the FPN's 1x1 lateral GEMMs at N = 256, and the FPN glue (nearest_upsample_add and its
adjoint, the NCDHW <-> channels-last transposes, add_inplace).

Conventions: inputs are rounded to the storage dtype first (`q`), the reference is float64 (tests/_conv_layer_ref.py), the check is tests/_metrics.assert_close
(max-norm, relative L2 and elementwise) at the project's tolerances TOL -- except the pure moves and single additions of sections 6 and 7, which have one
correctly rounded result and are held to torch.equal, and sections 2b and 2c, which hold single kernels on bf16-rounded operands to a measured rounding bound
far below TOL (one lost voxel or tap must fail).  Every conv, weight-gradient and GEMM case names the dispatch line it reaches (`dispatch_nt` of
csrc/gemm.hip, the branch of ops.conv3d_k3_wgrad, ops.use_conv64); where the rule is visible from Python the test asserts it, and the C entry point that
ran is read off a spy on the library's call()."""
import pytest
import torch
from torch import nn

from tests import _conv_layer_ref as R
from tests._conv_layer_ref import cl, ncdhw, q, rnd
from tests._metrics import assert_close

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
DTS = [F32, BF16]
TOL = {F32: 2e-4, BF16: 3e-2}
NAME = {F32: "fp32", BF16: "bf16"}


def _ops():
    from nerf_mae_amd import ops
    return ops


def dev(t, dt=None):
    return (t if dt is None else t.to(dt)).cuda().contiguous()


def check(a, b, dt, name=""):
    assert_close(a, b, TOL[dt], f"{name} {NAME[dt]}")


@pytest.fixture
def entries(monkeypatch):
    """names of the C entry points called through ops.lib().call, in order"""
    L = _ops().lib()
    names, call = [], L.call

    def spy(name, *args):
        names.append(name)
        return call(name, *args)

    monkeypatch.setattr(L, "call", spy)
    return names


# ---- 1. the implicit-GEMM conv at detector widths ----------------------------------------------------------------------------------------------------
# k_conv3_nt: M = D*H*W rows per sample, batch = B, K = 27 * Cin, t16 = Cout / 16.  Loader: bf16 with Cin % 64 == 0 -> AConv3F, other bf16 -> AConv3<bf16>,
# fp32 -> AConv3<float>.  dispatch_nt with a conv loader (the narrow-tile selection for K >= 384 is compiled for the plain-matrix loader only: section 5):
#   B*M <= 8192 or K <= 1024, t16 >= 4:  t16 % 6 == 0 -> <1,6>, else t16 % 4 == 0 -> <1,4>       (64-row tiles)
#   otherwise:  t16 == 4 -> <4,4>,  t16 % 6 == 0 -> <2,6>,  else <2,8>                            (256- / 128-row tiles)
# The bias-free call of a bf16 case with B*M <= 65536 may also split the contraction (k_conv3_nt: s = min(8, ceil(1024 / tiles), (K / 64) / 16) > 1).
CONV_CASES = [
    # dt    B   D   H   W  Cin Cout
    (BF16, 1,  5,  5,  5,  64,  64),    # 125 rows: AConv3F, t16 4 -> <1,4>; 27 k-tiles: no split
    (BF16, 2,  5,  6,  7, 256, 128),    # 420 rows: AConv3F, t16 8 -> <1,4>; bias-free call splits 6 ways (14 tiles, 108 k-tiles)
    (BF16, 1,  5,  5,  5, 256, 256),    # 125 rows: AConv3F, t16 16 -> <1,4>; bias-free call splits 6 ways (8 tiles)
    (BF16, 2,  5,  6,  7,  72, 256),    # 420 rows: AConv3<bf16> (Cin % 64 != 0), t16 16 -> <1,4>; K = 1944 is no multiple of the 64-deep k-tile
    (BF16, 1,  5,  5,  5,  72,  96),    # 125 rows: AConv3<bf16>, t16 6 -> <1,6>
    (F32,  1,  5,  5,  5,  64,  64),    # 125 rows: AConv3<float>, t16 4 -> <1,4>
    (F32,  2,  5,  6,  7, 256, 256),    # 420 rows: AConv3<float>, t16 16 -> <1,4>
    (F32,  1,  5,  5,  5,  72, 128),    # 125 rows: AConv3<float>, t16 8 -> <1,4>
    (BF16, 2, 17, 16, 17,  64,  64),    # 9248 rows, K 1728: AConv3F, t16 4 -> <4,4>; 4624 rows per sample = 18 tiles of 256 + 16 rows
    (BF16, 2, 17, 16, 17,  64, 128),    # 9248 rows: AConv3F, t16 8 -> <2,8>; 36 tiles of 128 + 16 rows
    (BF16, 2, 17, 16, 17, 256, 256),    # 9248 rows, K 6912: AConv3F, t16 16 -> <2,8> (the FPN output conv's shape class); bias-free call splits 6 ways (148 tiles)
    (BF16, 2, 17, 16, 17,  72,  96),    # 9248 rows, K 1944: AConv3<bf16>, t16 6 -> <2,6>
    (F32,  2, 17, 16, 17,  64, 256),    # 9248 rows: AConv3<float>, t16 16 -> <2,8>
    (F32,  2, 17, 16, 17,  72,  64),    # 9248 rows: AConv3<float>, t16 4 -> <4,4>
]


def _conv_id(c):
    return f"{NAME[c[0]]}-b{c[1]}-{c[2]}x{c[3]}x{c[4]}-{c[5]}to{c[6]}"


@pytest.mark.parametrize("case", CONV_CASES, ids=_conv_id)
def test_generic_conv_with_and_without_the_bias_epilogue(case, entries):
    ops = _ops()
    dt, B, D, H, W, Cin, Cout = case
    c = R.conv_case(*case, grads=False)
    assert (c["b"].abs() >= 0.25).all(), "a zero bias would hide a dropped epilogue"
    x, wp, bias = dev(cl(c["x"]), dt), dev(R.pack_fwd(c["w"]), dt), dev(c["b"])
    assert not ops.use_conv64(x, Cout), "these volumes stay on the generic kernel"
    y = ops.conv3d_k3_bias(x, wp, bias, Cout)
    assert y.dtype == dt and tuple(y.shape) == (B, D, H, W, Cout)
    check(ncdhw(y), c["y"], dt, "conv3d_k3_bias")
    y0 = ops.conv3d_k3(x, wp, Cout)
    check(ncdhw(y0), c["y"] - c["b"].double()[None, :, None, None, None], dt, "conv3d_k3")
    assert entries == ["nmh_conv3d_k3_bias", "nmh_conv3d_k3"]


@pytest.mark.parametrize("accumulate", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("D", [5, 10])
def test_input_gradient_with_the_split_contraction(D, accumulate):
    """bf16 256 -> 256 input gradient on the flipped [Ci][27][Co] pack.  ops.conv3d_k3 hands the workspace over for B*V <= 65536; k_conv3_nt then cuts the 108
    k-tiles 6 ways (5^3: 2 x 4 tiles of 64 x 64, 10^3: 16 x 4) and nt_ksplit_reduce_kernel sums the partial tiles and applies `accumulate`."""
    ops = _ops()
    dt, B, C = BF16, 1, 256
    c = R.conv_case(dt, B, D, D, D, C, C)
    assert B * D ** 3 <= 65536
    dy, wd = dev(cl(c["dy"]), dt), dev(R.pack_dgrad(c["w"]), dt)
    if not accumulate:
        dx = ops.conv3d_k3(dy, wd, C)
        check(ncdhw(dx), c["dx"], dt, f"dgrad {D}^3")
    else:
        base = q(rnd(B, D, D, D, C, seed=5), dt)
        assert base.abs().min() > 0
        out = dev(base, dt)
        got = ops.conv3d_k3(dy, wd, C, out=out, accumulate=True)
        assert got is out
        check(ncdhw(out), c["dx"] + ncdhw(base).double(), dt, f"dgrad + accumulate {D}^3")


# ---- 2. the weight gradient's three branches (ops.conv3d_k3_wgrad) and the bias gradient -----------------------------------------------------------
HALO48, HALO64, IGEMM = "nmh_conv3d_k3_wgrad_halo", "nmh_conv3d_k3_c64_wgrad", "nmh_conv3d_k3_wgrad"
WGRAD_CASES = [
    # dt    B   D   H   W  Cin Cout  entry
    (BF16, 1, 16, 16, 16, 256, 256, HALO64),   # 64-block kernel, 16 block pairs in the fixed workspace (8 workgroups per pair and tap group)
    (BF16, 2, 16, 16, 16, 256, 256, HALO64),   # the same on two samples
    (BF16, 1, 16, 16, 16,  64, 128, HALO64),   # 64-block kernel, dW 128 x 64: 2 block pairs
    (BF16, 2, 16, 16, 16,  64, 128, HALO64),
    (BF16, 1,  5,  6,  7, 256, 256, IGEMM),    # below 4096 voxels: implicit GEMM k_conv3_tn
    (F32,  1,  5,  6,  7, 256, 256, IGEMM),    # fp32: implicit GEMM
    (BF16, 1, 16, 16, 16,  72,  40, IGEMM),    # 4096 voxels, channel counts divisible by neither 48 nor 64: the fall-through
    (F32,  1, 16, 16, 16,  72,  40, IGEMM),
    (BF16, 1, 16, 16, 16,  96, 192, HALO48),   # 48-block kernel (2 x 4 block pairs)
    (BF16, 2, 18, 18, 18, 192,  96, HALO48),   # 48-block kernel, 8 sub-problems of 16 workgroups on 2 x 50 tiles, ragged on every axis (section 2b holds it to HALO_EPS)
]


def _wgrad_rule(ops, dt, V, Cin, Cout):
    """the branch conditions of ops.conv3d_k3_wgrad, restated"""
    if ops.HALO_WGRAD and dt == BF16 and V >= 4096:
        if Cin % 48 == 0 and Cout % 48 == 0 and (Cin // 48) * (Cout // 48) <= 256:
            return HALO48
        if Cin % 64 == 0 and Cout % 64 == 0 and (Cin // 64) * (Cout // 64) <= 128:
            return HALO64
    return IGEMM


@pytest.mark.parametrize("case", WGRAD_CASES, ids=lambda c: _conv_id(c[:7]) + "-" + c[7].replace("nmh_conv3d_k3_", ""))
def test_weight_gradient_added_onto_a_nonzero_buffer(case, entries):
    ops = _ops()
    dt, B, D, H, W, Cin, Cout, entry = case
    assert _wgrad_rule(ops, dt, D * H * W, Cin, Cout) == entry
    c = R.conv_case(dt, B, D, H, W, Cin, Cout)
    dW = torch.full((Cout, Cin, 3, 3, 3), 0.5, device="cuda")
    ops.conv3d_k3_wgrad(dev(cl(c["dy"]), dt), dev(cl(c["x"]), dt), dW)
    assert entries[-1] == entry, entries
    check(dW, c["dw"] + 0.5, dt, f"wgrad {entry}")


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("N", [64, 256])
@pytest.mark.parametrize("M", [125, 4096 * 2])
def test_bias_gradient_added_onto_a_nonzero_buffer(M, N, dt):
    ops = _ops()
    dy = q(rnd(M, N, seed=M + N), dt)
    db = torch.full((N,), -0.75, device="cuda")
    ops.bias_grad(dev(dy, dt), db, M, N)
    check(db, dy.double().sum(0) - 0.75, dt, f"bias_grad {M}x{N}")


# ---- 2b. the 48-block halo weight gradient in channel sub-problem mode, held to a rounding bound ----------------------------------------------------
# launch_wgrad_halo (csrc/conv48.hip) with nsub = (Cin / 48) (Cout / 48) > 1: gridDim.y = nsub, nb = 128 / nsub workgroups per sub-problem (floored at 1,
# clamped to the number of 4x4x16 tiles), workgroup j of a sub-problem walks tiles j, j + nb, ... of the B * tz * ty * tx tile sequence (samples back to back),
# its partial goes to workspace slot sub * nb + j and the reduce kernel sums the nb slots of a sub-problem onto dW.
#
# The bound.  dW is fp32 and the operands hold bf16 values, so every product is exact in fp32 and the result differs from float64 by the accumulation order
# only: |a - b| <= HALO_EPS * rms(b) for EVERY entry.  One voxel dropped from (or counted twice in) the contraction moves entries by about |x dy| / sqrt(L) of
# rms (L = B D H W terms of unit variance), so HALO_EPS must stay below 0.1 / sqrt(L) of the case at hand -- asserted -- for a single lost voxel to fail; TOL[bf16]
# = 3e-2 would let it through at every L >= 10 or so.  HALO_EPS is 4 x the worst value measured over the cases below on an MI355X (the measured figures are at
# HALO_MEASURED; float32 F.conv3d on the host sits at 6e-6 ... 1.6e-5).
HALO_SUB_CASES = [
    # B   D   H   W  Cin Cout   nsub  nb  tiles
    (1,  5,  6, 20,  96,  96),  #  4  32 -> 8   8: ragged on every axis; nb clamped to the tile count
    (2,  6, 10, 20, 192,  96),  #  8  16       24: uneven shares (workgroups 0..7 two tiles, 8..15 one), and the stride of 16 takes workgroup j from sample 0 (tile j) into sample 1 (tile j + 16)
    (3,  3,  5, 40,  96, 192),  #  8  16       18: D below one tile, x = 2.5 tiles (the 40^3 level's), three samples
    (1,  9,  9, 17, 384, 192),  # 32   4       18: four or five tiles per workgroup through the prefetch loop
    (1,  4,  4, 16, 576, 576),  # 144  1        1: the nb = 1 floor, 144 of the 256 workspace slots
    (1,  2,  3,  5,  48,  96),  #  2  64 -> 1   1: the volume inside one tile on every axis
]
# max|a - b| / rms(b) on an MI355X, in the order of HALO_SUB_CASES: 8.6e-7, 7.1e-7, 6.2e-7, 1.66e-6, 1.23e-6, 3.8e-7; the dispatcher's 18^3 case 1.44e-6;
# against caps of 4.1e-3, 2.0e-3, 2.4e-3, 2.7e-3, 6.3e-3, 1.8e-2 and 9.3e-4
HALO_MEASURED = 1.66e-6        # the worst of them
HALO_EPS = 4 * HALO_MEASURED


def _halo_cap(B, D, H, W):
    return 0.1 / (B * D * H * W) ** 0.5


def _assert_rounding_bound(a, b, eps, cap, name, ulp=0.0):
    """|a - b| <= ulp * |b| + eps * rms(b) for every entry, with eps <= cap (the caller's derivation of what one lost term would move)"""
    assert eps <= cap, f"{name}: eps {eps:.2e} is no sharper than the cap {cap:.2e}"
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape
    rms = b.pow(2).mean().sqrt().item()
    diff = (a - b).abs()
    need = ((diff - ulp * b.abs()).clamp_min(0).max() / rms).item()
    print(f"  [{name}] max|a-b| / rms {diff.max().item() / rms:.2e}  eps needed {need:.2e}  (eps {eps:.2e}, cap {cap:.2e})")
    assert need <= eps, f"{name}: |a-b| exceeds {ulp:g} |b| + eps rms(b): needs eps {need:.3e} > {eps:.3e}"


def _wgrad_halo_direct(ops, c, ws):
    """nmh_conv3d_k3_wgrad_halo on the case's bf16 operands, added onto a dW filled with 0.5"""
    B, Cin, D, H, W = c["x"].shape
    Cout = c["dy"].shape[1]
    dW = torch.full((Cout, Cin, 3, 3, 3), 0.5, device="cuda")
    ops.lib().call("nmh_conv3d_k3_wgrad_halo", dev(cl(c["dy"]), BF16), dev(cl(c["x"]), BF16), dW, ws, B, D, H, W, Cin, Cout, torch.cuda.current_stream().cuda_stream)
    return dW


def _halo_ws(ops):
    """a workspace of the documented size, NaN in every slot: a slot the reduce reads and the launch did not write shows"""
    return torch.full((ops.lib().call("nmh_conv3d_k3_c48_wgrad_ws_floats"),), float("nan"), device="cuda")


@pytest.mark.parametrize("case", HALO_SUB_CASES, ids=lambda c: _conv_id((BF16,) + c))
def test_halo_weight_gradient_sub_problem_mode(case):
    ops = _ops()
    B, D, H, W, Cin, Cout = case
    assert (Cin // 48) * (Cout // 48) > 1 and Cin % 48 == 0 and Cout % 48 == 0 and (Cin // 48) * (Cout // 48) <= 256
    c = R.conv_case(BF16, *case)
    dW = _wgrad_halo_direct(ops, c, _halo_ws(ops))
    _assert_rounding_bound(dW, c["dw"] + 0.5, HALO_EPS, _halo_cap(B, D, H, W), f"wgrad_halo {_conv_id((BF16,) + case)}")


def test_halo_weight_gradient_ignores_stale_partials():
    """the fourth case (32 sub-problems x 4 workgroups: 128 slots) and then the first (4 x 8: 32 slots) on the SAME workspace, nothing cleared in between:
    the second launch's reduce must sum its own 8 slots per sub-problem and none of the larger launch's"""
    ops = _ops()
    ws = _halo_ws(ops)
    big, small = HALO_SUB_CASES[3], HALO_SUB_CASES[0]
    cb, cs = R.conv_case(BF16, *big), R.conv_case(BF16, *small)
    dWb = _wgrad_halo_direct(ops, cb, ws)
    dWs = _wgrad_halo_direct(ops, cs, ws)
    _assert_rounding_bound(dWb, cb["dw"] + 0.5, HALO_EPS, _halo_cap(*big[:4]), "wgrad_halo, first on the workspace")
    _assert_rounding_bound(dWs, cs["dw"] + 0.5, HALO_EPS, _halo_cap(*small[:4]), "wgrad_halo, second on the same workspace")


def test_halo_weight_gradient_through_the_dispatcher_at_the_rounding_bound(entries):
    """WGRAD_CASES' 18^3 case once more, through ops.conv3d_k3_wgrad and its own workspace, held to HALO_EPS instead of TOL"""
    ops = _ops()
    case = (2, 18, 18, 18, 192, 96)
    c = R.conv_case(BF16, *case)
    dW = torch.full((96, 192, 3, 3, 3), 0.5, device="cuda")
    ops.conv3d_k3_wgrad(dev(cl(c["dy"]), BF16), dev(cl(c["x"]), BF16), dW)
    assert entries[-1] == HALO48
    _assert_rounding_bound(dW, c["dw"] + 0.5, HALO_EPS, _halo_cap(*case[:4]), "wgrad_halo 18^3 through the dispatcher")


# ---- 2c. the 48-block conv (ops.conv3d_k3_c48mb), forward and input gradient, held to a rounding bound ------------------------------------------------
# bf16 outputs of an fp32 accumulation over 27 * C exact products: |a - b| <= 2^-8 |b| + C48MB_EPS * rms(b), half a bf16 ulp (the ulp of a value in
# [2^e, 2^(e+1)) is 2^(e-7) <= 2^-7 |b|) plus accumulation noise.  One dropped tap moves an output by about 1 / sqrt(27 C) of rms; C48MB_EPS must stay below a
# tenth of that -- asserted with the larger of the two channel counts, C = 192, for both directions.  C48MB_EPS is 4 x the worst value measured on an MI355X.
C48MB_SHARP_CASES = [(2, 6, 10, 20, 192, 96), (1, 12, 9, 40, 96, 192)]
# eps needed on an MI355X (max of (|a - b| - 2^-8 |b|) / rms(b)): forward 4.9e-7 and 6.6e-7, input gradient 2.5e-7 and 6.2e-7; the cap is 1.39e-3
C48MB_MEASURED = 6.6e-7        # the worst of them
C48MB_EPS = 4 * C48MB_MEASURED


@pytest.mark.parametrize("case", C48MB_SHARP_CASES, ids=lambda c: _conv_id((BF16,) + c))
def test_conv48_multiblock_at_the_rounding_bound(case, entries):
    ops = _ops()
    B, D, H, W, Cin, Cout = case
    c = R.conv_case(BF16, *case)
    w = nn.Parameter(c["w"].cuda())
    P = _pack([("wkm", w, "C48_F"), ("wkmd", w, "C48_D")], BF16)
    cap = 0.1 / (27 * max(Cin, Cout)) ** 0.5
    y = ops.conv3d_k3_c48mb(dev(cl(c["x"]), BF16), P["wkm"], Cout)
    yref = c["y"] - c["b"].double()[None, :, None, None, None]
    check(ncdhw(y), yref, BF16, "conv48mb forward")
    _assert_rounding_bound(ncdhw(y), yref, C48MB_EPS, cap, f"conv48mb forward {_conv_id((BF16,) + case)}", ulp=2.0 ** -8)
    dx = ops.conv3d_k3_c48mb(dev(cl(c["dy"]), BF16), P["wkmd"], Cin)
    check(ncdhw(dx), c["dx"], BF16, "conv48mb input gradient")
    _assert_rounding_bound(ncdhw(dx), c["dx"], C48MB_EPS, cap, f"conv48mb input gradient {_conv_id((BF16,) + case)}", ulp=2.0 ** -8)
    assert [e for e in entries if "conv3d" in e] == ["nmh_conv3d_k3_c48mb"] * 2


# ---- 3. the 64-channel-block conv with the bias epilogue --------------------------------------------------------------------------------------------
def _pack(params_and_modes, dt):
    """views of a _Packer holding the given (key, parameter, mode name) layouts, produced by the pack kernel as the modules do"""
    from nerf_mae_amd.model import _Packer
    P = _Packer()
    for key, p, mode in params_and_modes:
        P.add(key, p, getattr(P, mode))
    P.build(dt, params_and_modes[0][1].device)
    P.split = None
    P.run()
    return P


C64_CASES = [
    # B   D   H   W  Cin Cout stats
    (1,  6, 10, 20,  64,  64, True),     # ragged on every axis of the 4x4x16 tile; the fused statistics
    (2,  8,  8, 16,  64,  64, False),    # full tiles
    (1,  6, 10, 20, 128,  64, False),    # two input-channel blocks
    (2,  8,  8, 16, 128,  64, True),
    (1,  6, 10, 20, 256, 256, False),    # the FPN output conv: 4 x 4 blocks
    (1,  8,  8, 16, 256, 256, False),
]


@pytest.mark.parametrize("case", C64_CASES, ids=lambda c: f"b{c[0]}-{c[1]}x{c[2]}x{c[3]}-{c[4]}to{c[5]}{'-stats' if c[6] else ''}")
def test_conv64_with_the_bias_epilogue(case, entries):
    """ops.conv3d_k3_c64(..., bias=): the bias is added in fp32 before the one rounding of the store.  csrc/conv64.hip documents the fused statistics as
    those "of exactly what the normalisation pass will read back", i.e. sum and sum of squares of the STORED bf16 outputs, bias included; with |bias| >= 0.25
    the sums without it would be off by V * bias."""
    ops = _ops()
    dt = BF16
    B, D, H, W, Cin, Cout, stats = case
    c = R.conv_case(dt, B, D, H, W, Cin, Cout, grads=False)
    wk = _pack([("w64", nn.Parameter(c["w"].cuda()), "C64_F")], dt)["w64"]
    assert wk.numel() == ops.conv64_pack_numel(Cin, Cout)
    acc = torch.full((B, Cout, 2), float("nan"), dtype=torch.float64, device="cuda") if stats else None
    y = ops.conv3d_k3_c64(dev(cl(c["x"]), dt), wk, Cout, stats_acc=acc, bias=dev(c["b"]))
    assert entries[-1] == "nmh_conv3d_k3_c64"
    check(ncdhw(y), c["y"], dt, "conv64 + bias")
    if stats:
        stored = y.double().cpu().reshape(B, -1, Cout)
        # fp32 partial sums per tile, fp64 across tiles: the fp32 tolerance
        check(acc[..., 0].cpu(), stored.sum(1), F32, "fused sum of the stored outputs")
        check(acc[..., 1].cpu(), stored.pow(2).sum(1), F32, "fused sum of squares of the stored outputs")
        check(acc[..., 0].cpu(), c["y"].sum((2, 3, 4)), dt, "fused sum against the float64 conv + bias")


# ---- 4. conv_layer.forward / backward as a unit --------------------------------------------------------------------------------------------------
LAYER_CASES = [
    # dt    B   D   H   W   C  C64_MIN_VOXELS  use_conv64
    (BF16, 1, 16, 16, 16,  64, 32768, False),   # the default threshold: generic conv3d_k3_bias / conv3d_k3; weight gradient on 64-channel blocks
    (BF16, 1, 16, 16, 16,  64,  4096, True),    # 16^3 qualifies: conv3d_k3_c64 with the bias, and with the input-gradient pack
    (BF16, 1, 16, 16, 16, 256,  4096, True),    # the FPN's width on the 64-block side
    (F32,  2,  5,  6,  7,  72, 32768, False),   # fp32 never takes the 64-block kernels
]


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: f"{NAME[c[0]]}-b{c[1]}-{c[2]}x{c[3]}x{c[4]}-c{c[5]}-{'conv64' if c[7] else 'generic'}")
def test_conv_layer_forward_and_backward(case, monkeypatch, entries):
    from nerf_mae_amd import conv_layer
    from nerf_mae_amd.model import _Packer
    ops = _ops()
    dt, B, D, H, W, C, min_voxels, c64 = case
    monkeypatch.setattr(ops, "C64_MIN_VOXELS", min_voxels)
    c = R.conv_case(dt, B, D, H, W, C, C)
    conv = nn.Conv3d(C, C, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(c["w"])
        conv.bias.copy_(c["b"])
    conv = conv.cuda()
    P = _Packer()
    conv_layer.register(P, "c", conv, dt)
    P.build(dt, conv.weight.device)
    P.split = None
    P.run()
    assert ("c.w64" in P.views) == (dt == BF16 and C % 64 == 0)
    x, dy = dev(cl(c["x"]), dt), dev(cl(c["dy"]), dt)
    assert ops.use_conv64(x, C) == c64 and ops.use_conv64(dy, C) == c64
    tag = f"conv_layer {'conv64' if c64 else 'generic'}"

    y = conv_layer.forward(P, "c", conv, x)
    assert entries[-1] == ("nmh_conv3d_k3_c64" if c64 else "nmh_conv3d_k3_bias")
    check(ncdhw(y), c["y"], dt, f"{tag} forward")

    dx = conv_layer.backward(P, "c", conv, dy, x)
    ops.join_side()                                  # the parameter gradients ran on the side stream
    assert entries[-1] == ("nmh_conv3d_k3_c64" if c64 else "nmh_conv3d_k3") and "nmh_bias_grad" in entries
    check(ncdhw(dx), c["dx"], dt, f"{tag} dx")
    check(conv.weight.grad, c["dw"], dt, f"{tag} weight.grad")
    check(conv.bias.grad, c["db"], dt, f"{tag} bias.grad")

    # a second backward with another cotangent and no input gradient: None, and both .grad hold the sum of the two references
    dy2 = q(rnd(*c["dy"].shape, seed=77), dt)
    dw2 = torch.nn.grad.conv3d_weight(c["x"].double(), c["w"].shape, dy2.double(), padding=1)
    dy2d = dev(cl(dy2), dt)
    assert conv_layer.backward(P, "c", conv, dy2d, x, need_dx=False) is None
    ops.join_side()
    check(conv.weight.grad, c["dw"] + dw2, dt, f"{tag} weight.grad after two backwards")
    check(conv.bias.grad, c["db"] + dy2.double().sum((0, 2, 3, 4)), dt, f"{tag} bias.grad after two backwards")


# ---- 5. the FPN's lateral 1x1 GEMMs at N = 256 -----------------------------------------------------------------------------------------------------
# forward gemm_nt(f [M,C], W [256,C], bias): N = 256 (t16 16), K = C.  dispatch_nt with the plain-matrix loader:
#   bf16, 8000 rows, C >= 384:        w22_config 242 (2048 <= M <= 16384, K >= 384, N % 128 == 0): the 2x2-wave kernel's 64 x 128 tile
#   bf16, 125 / 1000 rows, C >= 384:  the narrow-tile selection (2 / 16 row tiles x 8 tiles of 32 columns <= 384) -> <1,2>
#   everything else (C <= 192, fp32): K <= 1024, t16 % 4 == 0 -> <1,4>
# input gradient gemm_nt(dl [M,256], W^T [C,256]): N = C in {96, 192, 384, 768} (t16 % 6 == 0), K = 256 -> <1,6> in both dtypes
# weight and bias gradient gemm_tn(dl, f, dW [256,C], dbias=): one pass
@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("M", [125, 1000, 8000])
@pytest.mark.parametrize("C", [96, 192, 384, 768])
def test_fpn_lateral_gemms(C, M, dt):
    ops = _ops()
    N = 256
    f = q(rnd(M, C, seed=C + M), dt)
    w = q(rnd(N, C, seed=C + M + 1, scale=C ** -0.5), dt)
    b = rnd(N, seed=C + M + 2)
    dl = q(rnd(M, N, seed=C + M + 3), dt)
    fd, wd, dld = f.double(), w.double(), dl.double()
    fg, dlg = dev(f, dt), dev(dl, dt)
    lat = ops.gemm_nt(fg, dev(w, dt), bias=dev(b))
    check(lat, fd @ wd.T + b.double(), dt, f"lateral forward {M}x{N}x{C}")
    df = ops.gemm_nt(dlg, dev(w.T, dt))
    check(df, dld @ wd, dt, f"lateral input gradient {M}x{C}x{N}")
    dW, db = torch.full((N, C), 0.25, device="cuda"), torch.full((N,), -0.5, device="cuda")
    ops.gemm_tn(dlg, fg, dW, dbias=db)
    check(dW, dld.T @ fd + 0.25, dt, f"lateral weight gradient {N}x{C} over {M} rows")
    check(db, dld.sum(0) - 0.5, dt, f"lateral bias gradient over {M} rows")


# ---- 6. nearest_upsample_add and its adjoint ------------------------------------------------------------------------------------------------------
UP_SIZES = [
    ((5, 5, 5), (10, 10, 10)),    # halves
    ((3, 3, 3), (5, 5, 5)),       # ceil-halves
    ((3, 3, 4), (6, 5, 7)),       # ragged
    ((1, 1, 1), (4, 4, 4)),
    ((4, 5, 6), (4, 5, 6)),       # equal sizes
    ((3, 3, 3), (7, 7, 7)),       # ratios outside the FPN's own: ATen's floorf(i * in / out)
    ((2, 2, 2), (5, 5, 5)),
]
UP_IDS = ["halves", "ceil_halves", "ragged", "one_to_four", "equal", "three_to_seven", "two_to_five"]


def _exact_sum(a, b):
    """the one correctly rounded a + b in a's dtype: fp32 addition, or fp32 addition of the bf16 values followed by one rounding"""
    return a + b if a.dtype == F32 else (a.float() + b.float()).to(BF16)


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("sizes", UP_SIZES, ids=UP_IDS)
def test_nearest_upsample_add_is_bit_exact(sizes, dt):
    ops = _ops()
    (Dc, Hc, Wc), (Df, Hf, Wf) = sizes
    for C in (8, 256):
        for B in (1, 2):
            coarse = rnd(B, Dc, Hc, Wc, C, seed=C + B).to(dt)
            fine = rnd(B, Df, Hf, Wf, C, seed=C + B + 1).to(dt)
            want = _exact_sum(fine, R.upsample_add(coarse, fine))
            got = fine.cuda()
            assert ops.nearest_upsample_add(coarse.cuda(), got) is got
            assert torch.equal(got.cpu(), want), f"C {C} B {B}: {(got.cpu().float() - want.float()).abs().max().item():.3e}"


def test_nearest_upsample_add_beyond_the_launch_cap():
    """B 3, 20^3 -> 40^3, C 256: 6.1 M threads of 8 channels against the cap of 16384 blocks x 256 threads, so the grid-stride loop runs twice"""
    ops = _ops()
    B, C = 3, 256
    assert B * 40 ** 3 * (C // 8) > 16384 * 256
    coarse32, fine32 = rnd(B, 20, 20, 20, C, seed=1), rnd(B, 40, 40, 40, C, seed=2)
    for dt in DTS:
        coarse, fine = coarse32.to(dt), fine32.to(dt)
        want = _exact_sum(fine, R.upsample_add(coarse, fine))
        got = fine.cuda()
        ops.nearest_upsample_add(coarse.cuda(), got)
        assert torch.equal(got.cpu(), want), NAME[dt]
        del got, want


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("sizes", UP_SIZES, ids=UP_IDS)
def test_nearest_upsample_add_adjoint(sizes, dt):
    """dcoarse += the sum of dfine over the fine voxels that read it (8 terms at the FPN's ratios, 64 at 1 -> 4), accumulated in fp32 and rounded once"""
    ops = _ops()
    (Dc, Hc, Wc), (Df, Hf, Wf) = sizes
    for C in (8, 256):
        for B in (1, 2):
            dfine = q(rnd(B, Df, Hf, Wf, C, seed=C + B + 2), dt)
            pre = q(rnd(B, Dc, Hc, Wc, C, seed=C + B + 3), dt)
            assert pre.abs().min() > 0
            got = dev(pre, dt)
            assert ops.nearest_upsample_add_bwd(dev(dfine, dt), got) is got
            check(got, R.upsample_adjoint(dfine, pre.shape) + pre.double(), dt, f"adjoint C {C} B {B}")


# ---- 7. layout transposes and add_inplace: pure moves ----------------------------------------------------------------------------------------------
VOLS = {1: (1, 1, 1), 33: (1, 3, 11), 125: (5, 5, 5), 1000: (10, 10, 10)}     # no multiples of the 32-wide tile


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
@pytest.mark.parametrize("V", list(VOLS))
def test_layout_transposes_are_exact(V, dt):
    ops = _ops()
    D, H, W = VOLS[V]
    for C in (8, 24, 72, 256):
        for B in (1, 3):
            x = rnd(B, D, H, W, C, seed=V + C + B).to(dt)
            n = ops.ndhwc_to_ncdhw(x.cuda())
            assert n.dtype == F32 and n.is_contiguous() and torch.equal(n.cpu(), x.permute(0, 4, 1, 2, 3).float()), f"ndhwc_to_ncdhw C {C} B {B}"
            g = rnd(B, C, D, H, W, seed=V + C + B + 1)                    # fp32 values that bf16 does not hold: the bf16 direction rounds once
            c = ops.ncdhw_to_ndhwc(g.cuda(), dt)
            assert c.dtype == dt and c.is_contiguous() and torch.equal(c.cpu(), g.permute(0, 2, 3, 4, 1).to(dt)), f"ncdhw_to_ndhwc C {C} B {B}"
            assert torch.equal(ops.ncdhw_to_ndhwc(n, dt).cpu(), x), f"round trip C {C} B {B}"


@pytest.mark.parametrize("dt", DTS, ids=NAME.get)
def test_add_inplace_is_exact(dt):
    ops = _ops()
    a, b = rnd(3, 5, 7, 24, seed=1).to(dt), rnd(3, 5, 7, 24, seed=2).to(dt)
    got = a.cuda()
    assert ops.add_inplace(got, b.cuda()) is got
    assert torch.equal(got.cpu(), _exact_sum(a, b))
