"""The RPN head on the GPU (nerf_mae_amd.rpn.RPNHead over csrc/rpn_head.hip and the channels-last convolutions) against the float64 restatement of
tests/_rpn_head_ref.py (itself checked against the recorded reference in tests/test_rpn_head_ref_cpu.py).

1. The output kernels alone (ops.rpn_head_out_fwd / _bwd) against float64 matrix products.  fp32 compute: assert_close(rtol=1e-3), the project's fp32
   contract.  bf16 compute: t and the weights are bf16 values, so outputs, weight and bias gradients differ from float64 only by the fp32 accumulation and
   the hi + lo split of G (16 mantissa bits): 1e-3 as well; dt is STORED in bf16, one rounding of at most 2^-9 relative, and is held to 2^-8 (the factor 2
   covers roundings that flip at a bf16 boundary because of the accumulation order).  Every result is bit-identical between two runs.
2. The module.  fp32 compute: 1e-3 on outputs, the gradient of every parameter and of the features.  bf16 compute: the tolerance is not fixed in advance;
   per case and per quantity (objectness, pred_bbox_deltas, the gradient of the features and of each parameter) e_round = the max-norm error, relative to
   the tensor's largest entry, of the rounding-aware restatement against the unrounded one, computed on the CPU; the kernels are held to 2 e_round against
   the UNROUNDED float64 result (1e-3 where e_round is 0: the output biases' gradients, which no rounding reaches).  On these small grids e_round of the
   gradients is dominated by the few ReLU masks that the rounding of the layer before flips (each moves one voxel's gradient by its full size).
   Measured values: DESIGN.md 3.14."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_head_ref as H  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
FOUR = ((12, 11, 10), (7, 6, 5), (5, 4, 3), (1, 1, 1))
DT_STORE_TOL = 2.0 ** -8


def _m():
    from nerf_mae_amd import ops, rpn
    return ops, rpn


# ---- 1. the output kernels ---------------------------------------------------------------------------------------------------------------------
#            dtype           Cin  A   C  grids              N  relu   sparse G
OP_CASES = [
    (torch.float32,    8,  1, 6, ((1, 1, 1),),      1, True,  False),
    (torch.float32,   40,  5, 6, ((5, 4, 3),),      3, False, False),
    (torch.float32,   64,  5, 8, FOUR,              3, True,  True),
    (torch.float32,  256, 32, 8, ((7, 6, 5),),      1, True,  False),
    (torch.float32,  256,  5, 8, ((12, 11, 10),),   1, True,  False),
    (torch.bfloat16,   8,  1, 6, ((1, 1, 1),),      1, True,  False),
    (torch.bfloat16,  64,  5, 8, FOUR,              3, True,  False),
    (torch.bfloat16, 256,  5, 6, ((12, 11, 10),),   3, True,  True),
    (torch.bfloat16,  40, 32, 8, FOUR,              1, False, False),
    (torch.bfloat16, 256,  5, 8, ((7, 6, 5),),      1, False, True),
]


@functools.lru_cache(maxsize=None)
def op_case(dtype, Cin, A, C, grids, N, relu, sparse):
    """inputs that the compute dtype holds exactly and the float64 results.  t has exact zeros and negatives; a sparse G has 7 nonzero anchors per scene."""
    g = torch.Generator().manual_seed(Cin * 1000 + A * 10 + C + len(grids))
    cast = (lambda v: v.to(dtype).double())
    ts = []
    for grid in grids:
        t = torch.randn((N, *grid, Cin), generator=g)
        t[torch.rand(t.shape, generator=g) < 0.1] = 0.0
        ts.append(cast(t))
    wc, wb = cast(torch.randn((A, Cin), generator=g) * 0.2), cast(torch.randn((A * C, Cin), generator=g) * 0.2)
    bc, bb = torch.randn((A,), generator=g).double(), torch.randn((A * C,), generator=g).double()
    go = [torch.randn((N, A, *grid), generator=g).double() for grid in grids]
    gr = [torch.randn((N, A * C, *grid), generator=g).double() for grid in grids]
    if sparse:
        for k in range(len(grids)):
            for i in range(N):
                keep_o, keep_r = torch.zeros_like(go[k][i]), torch.zeros_like(gr[k][i])
                for _ in range(7):
                    a = int(torch.randint(A, (1,), generator=g))
                    w, h, d = [int(torch.randint(s, (1,), generator=g)) for s in grids[k]]
                    keep_o[a, w, h, d] = 1
                    keep_r[a * C:(a + 1) * C, w, h, d] = 1
                go[k][i] *= keep_o
                gr[k][i] *= keep_r
    obj, reg, dts = [], [], []
    dwc, dwb, dbc, dbb = torch.zeros_like(wc), torch.zeros_like(wb), torch.zeros_like(bc), torch.zeros_like(bb)
    for t, o_g, r_g in zip(ts, go, gr):
        a = t.clamp(min=0) if relu else t
        obj.append((torch.einsum("nxyzc,ac->naxyz", a, wc) + bc[None, :, None, None, None]))
        reg.append((torch.einsum("nxyzc,ac->naxyz", a, wb) + bb[None, :, None, None, None]))
        d = torch.einsum("naxyz,ac->nxyzc", o_g, wc) + torch.einsum("naxyz,ac->nxyzc", r_g, wb)
        dts.append(d * (t > 0) if relu else d)
        dwc += torch.einsum("naxyz,nxyzc->ac", o_g, a)
        dwb += torch.einsum("naxyz,nxyzc->ac", r_g, a)
        dbc += o_g.sum((0, 2, 3, 4))
        dbb += r_g.sum((0, 2, 3, 4))
    return dict(ts=ts, wc=wc, wb=wb, bc=bc, bb=bb, go=go, gr=gr, obj=obj, reg=reg, dts=dts, dwc=dwc, dwb=dwb, dbc=dbc, dbb=dbb)


def _op_run(ops, c, dtype, C, relu):
    ts = [t.to(dtype).cuda() for t in c["ts"]]
    wc, wb = c["wc"].to(dtype).cuda(), c["wb"].to(dtype).cuda()
    obj, reg = ops.rpn_head_out_fwd(ts, wc, wb, c["bc"].float().cuda(), c["bb"].float().cuda(), C, relu)
    grads = [torch.ones(v.shape, dtype=torch.float32).cuda() for v in (c["dwc"], c["dwb"], c["dbc"], c["dbb"])]      # += : the buffers start at one
    dts = ops.rpn_head_out_bwd(ts, wc, wb, [g.float().cuda() for g in c["go"]], [g.float().cuda() for g in c["gr"]], C, relu, *grads)
    return obj, reg, dts, grads


@pytest.mark.parametrize("case", OP_CASES, ids=lambda c: f"{str(c[0])[6:]}-c{c[1]}-a{c[2]}x{c[3]}-{len(c[4])}lv{c[4][0][0]}-n{c[5]}-{'relu' if c[6] else 'id'}-{'sparse' if c[7] else 'dense'}")
def test_output_kernels_against_float64(case):
    ops, _ = _m()
    dtype, Cin, A, C, grids, N, relu, sparse = case
    c = op_case(*case)
    assert all((t == 0).any() and (t < 0).any() for t in c["ts"] if t.numel() >= 64), "t holds exact zeros and negatives"
    obj, reg, dts, grads = _op_run(ops, c, dtype, C, relu)
    tag = f"{dtype} Cin {Cin} A {A} C {C}"
    for k in range(len(grids)):
        assert obj[k].dtype == torch.float32 and tuple(obj[k].shape) == (N, A, *grids[k]) and tuple(reg[k].shape) == (N, A * C, *grids[k]) and obj[k].is_contiguous()
        assert_close(obj[k].cpu(), c["obj"][k], 1e-3, f"{tag} objectness {k}")
        assert_close(reg[k].cpu(), c["reg"][k], 1e-3, f"{tag} pred_bbox_deltas {k}")
        assert dts[k].dtype == dtype and dts[k].shape == c["dts"][k].shape
        got, want = dts[k].double().cpu(), c["dts"][k]
        if want.abs().sum() > 0:
            assert_close(got, want, 1e-3 if dtype == torch.float32 else DT_STORE_TOL, f"{tag} dt {k}")
        assert (got[want == 0] == 0).all(), "dt is exactly zero where the mask or the gradient is"
    for name, g, want in zip(("dw_cls", "dw_box", "db_cls", "db_box"), grads, (c["dwc"], c["dwb"], c["dbc"], c["dbb"])):
        assert_close(g.double().cpu() - 1.0, want, 1e-3, f"{tag} {name}")
    again = _op_run(ops, c, dtype, C, relu)
    for a, b in zip([*obj, *reg, *dts, *grads], [*again[0], *again[1], *again[2], *again[3]]):
        assert torch.equal(a, b), "two runs are bit-identical"


def test_relu_passes_and_error_paths():
    ops, rpn = _m()
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(3, 5, 4, 3, 24).to(dtype)
        x[0, 0, 0, 0, :4] = 0.0
        x[0, 0, 0, 0, 4] = -0.0
        y = ops.relu_(x.clone().cuda())
        assert torch.equal(y.cpu(), x.clamp(min=0)) and not torch.signbit(y.cpu().float()[x.float() <= 0]).any()
        dy = torch.randn(x.shape).to(dtype)
        got = ops.relu_bwd_(dy.clone().cuda(), y)
        assert torch.equal(got.cpu(), torch.where(x > 0, dy, torch.zeros_like(dy))), "relu'(0) = 0"
    t = torch.zeros(1, 2, 2, 2, 16).cuda()
    w1, w6 = torch.zeros(3, 16).cuda(), torch.zeros(18, 16).cuda()
    b1, b6 = torch.zeros(3).cuda(), torch.zeros(18).cuda()
    with pytest.raises(RuntimeError):
        ops.rpn_head_out_fwd([t.cpu()], w1, w6, b1, b6, 6, True)
    with pytest.raises(NotImplementedError):
        ops.rpn_head_out_fwd([torch.zeros(1, 2, 2, 2, 12).cuda()], torch.zeros(3, 12).cuda(), torch.zeros(18, 12).cuda(), b1, b6, 6, True)
    with pytest.raises(ValueError):
        ops.rpn_head_out_fwd([t] * 5, w1, w6, b1, b6, 6, True)
    with pytest.raises(ValueError):
        ops.rpn_head_out_fwd([t], w1, w6, b1, b6, 7, True)
    with pytest.raises(ValueError):
        ops.rpn_head_out_fwd([t], torch.zeros(33, 16).cuda(), torch.zeros(33 * 6, 16).cuda(), torch.zeros(33).cuda(), torch.zeros(198).cuda(), 6, True)
    head = rpn.RPNHead(16, 3, 1).cuda()
    with pytest.raises(RuntimeError):
        head([torch.zeros(1, 16, 2, 2, 2)])
    with pytest.raises(ValueError):
        head.forward_channels_last([torch.zeros(1, 2, 2, 2, 16).cuda()])          # fp32 features into a bf16 head
    with pytest.raises(RuntimeError):
        rpn.RPNHead(16, 3, 1)([torch.zeros(1, 16, 2, 2, 2).cuda()])                 # parameters on the host


# ---- 2. the module -----------------------------------------------------------------------------------------------------------------------------
MOD_GRIDS = ((5, 4, 3), (3, 2, 2), (2, 1, 2))
MOD_CASES = [(depth, rotate) for depth in (0, 1, 4) for rotate in (False, True)]


@functools.lru_cache(maxsize=None)
def mod_case(depth, rotate, Cin=16, A=3, N=2, grids=MOD_GRIDS, want_rounded=True):
    C = 8 if rotate else 6
    P = {k: v.float().double() for k, v in H.make_params(100 + depth * 2 + rotate, depth, Cin, A, C, std=2.0 / Cin ** 0.5).items()}
    feats = [f.float().double() for f in H.make_features(200 + depth, N, Cin, grids)]
    g = torch.Generator().manual_seed(300 + depth)
    cot_obj = [torch.randn((N, A, *gr), generator=g).double() for gr in grids]
    cot_reg = [torch.randn((N, A * C, *gr), generator=g).double() for gr in grids]
    exact = H.run(feats, P, depth, cot_obj, cot_reg)
    rounded = H.run(feats, P, depth, cot_obj, cot_reg, H.round_bf16) if want_rounded else None
    return dict(P=P, feats=feats, cot_obj=cot_obj, cot_reg=cot_reg, exact=exact, rounded=rounded, Cin=Cin, A=A, C=C)


def _quantities(res):
    out = {"objectness": res["obj"], "pred_bbox_deltas": res["reg"], "d features": res["dfeat"]}
    out.update({f"d {k}": [v] for k, v in res["dparam"].items()})
    return out


def _mod_run(rpn, c, depth, rotate, dtype, channels_last=False):
    head = rpn.RPNHead(c["Cin"], c["A"], depth, rotate, compute_dtype=dtype)
    head.load_state_dict({k: v.float() for k, v in c["P"].items()}, strict=True)
    head = head.cuda()
    feats = [f.float().cuda().requires_grad_(True) for f in c["feats"]]
    if channels_last:
        ops, _ = _m()
        obj, reg = head.forward_channels_last([ops.ncdhw_to_ndhwc(f.detach(), dtype) for f in feats])
    else:
        obj, reg = head(feats)
    total = sum((o * t.float().cuda()).sum() for o, t in zip(obj, c["cot_obj"])) + sum((r * t.float().cuda()).sum() for r, t in zip(reg, c["cot_reg"]))
    if not channels_last:
        total.backward()
    return dict(obj=[o.detach() for o in obj], reg=[r.detach() for r in reg], dfeat=[f.grad for f in feats], dparam={k: p.grad for k, p in head.named_parameters()})


@pytest.mark.parametrize("depth,rotate", MOD_CASES)
def test_module_fp32_against_float64(depth, rotate):
    _, rpn = _m()
    c = mod_case(depth, rotate)
    got = _mod_run(rpn, c, depth, rotate, torch.float32)
    assert list(got["dparam"]) == H.keys(depth)
    want = _quantities(c["exact"])
    for name, ts in _quantities(got).items():
        for k, (a, b) in enumerate(zip(ts, want[name])):
            assert a is not None, f"{name} {k}: no gradient"
            assert_close(a.cpu(), b, 1e-3, f"fp32 depth {depth} rotate {rotate} {name} {k}")


def _bf16_check(rpn, c, depth, rotate, tag):
    want, rnd = _quantities(c["exact"]), _quantities(c["rounded"])
    e_round = {name: H.max_err(rnd[name], want[name]) for name in want}
    got = _quantities(_mod_run(rpn, c, depth, rotate, torch.bfloat16))
    e_kernel = {name: H.max_err([t.cpu() for t in got[name]], want[name]) for name in want}
    print(f"{tag}: e_round {max(e_round.values()):.3e}  kernel {max(e_kernel.values()):.3e}")
    assert max(e_round.values()) > 0
    for name in want:
        # a quantity that no stored tensor reaches (the gradients of the two output biases are plain sums of the cotangent) has e_round 0: the fp32 contract
        bound = 2 * e_round[name] if e_round[name] > 0 else 1e-3
        print(f"    {name:28s} e_round {e_round[name]:.3e}  kernel {e_kernel[name]:.3e}  bound {bound:.3e}")
        assert e_kernel[name] <= bound, f"{tag} {name}: kernel error {e_kernel[name]:.3e} > {bound:.3e} (e_round {e_round[name]:.3e})"


@pytest.mark.parametrize("depth,rotate", MOD_CASES)
def test_module_bf16_within_twice_the_rounding_error(depth, rotate):
    _, rpn = _m()
    _bf16_check(rpn, mod_case(depth, rotate), depth, rotate, f"bf16 depth {depth} rotate {rotate}")


def test_module_bf16_on_the_64_channel_block_convolution():
    """Cin 64 and a 32^3 level: ops.use_conv64 holds, so the LDS-halo conv with the bias epilogue and its dgrad run; the second level takes the generic conv"""
    ops, rpn = _m()
    c = mod_case(1, False, Cin=64, A=2, N=1, grids=((32, 32, 32), (3, 2, 2)))
    assert ops.use_conv64(torch.empty(1, 32, 32, 32, 64, dtype=torch.bfloat16), 64) and not ops.use_conv64(torch.empty(1, 3, 2, 2, 64, dtype=torch.bfloat16), 64)
    _bf16_check(rpn, c, 1, False, "bf16 conv64 depth 1")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_ncdhw_entry_equals_the_channels_last_entry_bit_for_bit(dtype):
    _, rpn = _m()
    c = mod_case(4, True)
    a, b = _mod_run(rpn, c, 4, True, dtype), _mod_run(rpn, c, 4, True, dtype, channels_last=True)
    assert all(torch.equal(x, y) for n in ("obj", "reg") for x, y in zip(a[n], b[n]))
    again = _mod_run(rpn, c, 4, True, dtype)
    for n, ts in _quantities(a).items():        # fixed-order sums: the outputs and the output stage's gradients (the 3x3x3 convs' weight and bias gradients add atomically)
        if "conv." not in n and n != "d features":
            assert all(torch.equal(x, y) for x, y in zip(ts, _quantities(again)[n])), f"{n}: two runs are bit-identical"


def test_reference_checkpoint_loads_strictly_and_reproduces_the_recorded_outputs():
    _, rpn = _m()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g23_rpn_head.npz")))
    feats, P, cot_obj, cot_reg, rec = H.golden_case(g, 2, True)
    gen = rpn.AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)
    net = rpn.RegionProposalNetwork(gen, rpn.RPNHead(H.G_CIN, H.G_A, 2, rotate=True, compute_dtype=torch.float32), 0.35, 0.2, 256, 0.5, dict(training=10, testing=10),
                                    dict(training=10, testing=10), 0.3, rotated_bbox=True)
    ckpt = {"rpn.head." + k: v.float() for k, v in P.items()}
    ckpt["backbone.something"] = torch.zeros(1)
    net.load_state_dict({k[len("rpn."):]: v for k, v in ckpt.items() if k.startswith("rpn.")}, strict=True)
    net = net.cuda()
    xs = [f.float().cuda().requires_grad_(True) for f in feats]
    obj, reg = net.head(xs)
    (sum((o * t.float().cuda()).sum() for o, t in zip(obj, cot_obj)) + sum((r * t.float().cuda()).sum() for r, t in zip(reg, cot_reg))).backward()
    for k in range(len(feats)):
        assert_close(obj[k].cpu(), rec["obj"][k], 1e-3, f"g23 objectness {k}")
        assert_close(reg[k].cpu(), rec["reg"][k], 1e-3, f"g23 pred_bbox_deltas {k}")
        assert_close(xs[k].grad.cpu(), rec["dfeat"][k], 1e-3, f"g23 d features {k}")
    for name, p in net.head.named_parameters():
        assert_close(H.recorded_view(name, p.grad.cpu()), rec["dparam"][name], 1e-3, f"g23 d {name}")
