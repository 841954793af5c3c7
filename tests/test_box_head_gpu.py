"""The fused box head on the GPU (nerf_mae_amd.detector.FusedRCNN over csrc/box_head.hip and the channels-last 3x3x3 conv layer) against the float64
restatement of tests/_box_head_ref.py (itself checked against the recorded reference in tests/test_box_head_ref_cpu.py).

1. The output kernels alone (ops.box_head_pack / box_head_out_fwd / box_head_out_bwd) against float64 matrix products.  fp32 compute: assert_close(rtol=1e-3), the
   project's fp32 contract.  bf16 compute: x and the packed weights are bf16 values (the mean form multiplies the fp32 mean with fp32 weights), so outputs,
   weight and bias gradients differ from float64 only by the fp32 accumulation and the hi + lo split of G (16 mantissa bits): 1e-3 as well; dx is STORED in
   bf16, one rounding of at most 2^-9 relative, and is held to 2^-8 (the rules of tests/test_rpn_head_gpu.py).  Every result is bit-identical between runs.
3. The module in fp32 compute at 1e-3 on outputs and the gradient of the pooled tensor and of every parameter; the recorded g32 after a strict load.
4. The module in bf16 compute: the tolerance is not fixed in advance; per case and per quantity e_round = the max-norm error, relative to the tensor's largest
   entry, of the rounding-aware restatement against the unrounded one, computed on the CPU; the kernels are held to 2 e_round against the UNROUNDED float64
   result (1e-3 where e_round is 0: the two output biases' gradients).  Measured values: DESIGN.md 3.23.
5. - 10. Row independence, run-to-run identity, None cotangents, the head inside Classification_Model, predict_dense, TwoStageDetector under FinetuneStep, checkpoints
   across the two head classes, graph capture.
(2., the small-volume conv kernels, does not exist: the head ships on the shared conv layer)"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _box_head_ref as B  # noqa: E402
from tests._metrics import assert_close, relerr  # noqa: E402

pytestmark = pytest.mark.gpu
DX_STORE_TOL = 2.0 ** -8
DTYPES = (torch.float32, torch.bfloat16)


def _m():
    from nerf_mae_amd import detector, ops
    return ops, detector


# ---- 1. the output kernels -----------------------------------------------------------------------------------------------------------------------
OP_MS = (1, 37, 130, 257)                                   # partial row tiles on both sides of 128 and 256
OP_CS = ((16, 27), (24, 6), (8, 1), (64, 8))                # contractions of 432, 144, 8 and 512 in the flatten form
# the other four factors go round with the two indices so that every value of each meets every dtype, every M and every (C, S)
OP_CASES = [(dtype, M, C, S, 7 if (mi + ci // 2 + di) % 2 else 6, 2 + (mi // 2 + ci + di) % 2, (mi + ci + di) % 2 == 0, (mi // 2 + ci // 2 + mi + di) % 2 == 0)
            for di, dtype in enumerate(DTYPES) for mi, M in enumerate(OP_MS) for ci, (C, S) in enumerate(OP_CS)]


def test_the_output_kernel_cases_cover_every_factor():
    for col, values in ((4, (6, 7)), (5, (2, 3)), (6, (False, True)), (7, (False, True))):
        for dtype in DTYPES:
            for pick, keys in ((1, OP_MS), (2, [c for c, _ in OP_CS])):
                for key in keys:
                    assert {c[col] for c in OP_CASES if c[0] == dtype and c[pick] == key} == set(values), (col, dtype, key)


@functools.lru_cache(maxsize=None)
def op_case(dtype, M, C, S, reg, ncls, flatten, relu):
    """inputs that the kernels' operand dtypes hold exactly and the float64 results.  x has exact zeros and negatives."""
    g = torch.Generator().manual_seed(M * 1000 + C * 10 + S + reg + ncls)
    cast = lambda v: v.to(dtype).double()
    x = torch.randn((M, S, C), generator=g)
    x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
    x = cast(x)
    K = C * S if flatten else C
    wcast = cast if flatten else (lambda v: v.float().double())
    wb, wc = wcast(torch.randn((reg, K), generator=g) * 0.2), wcast(torch.randn((ncls, K), generator=g) * 0.2)
    bb, bc = torch.randn((reg,), generator=g).double(), torch.randn((ncls,), generator=g).double()
    gb, gc = torch.randn((M, reg), generator=g).double(), torch.randn((M, ncls), generator=g).double()
    a = x.clamp(min=0) if relu else x
    v = a.permute(0, 2, 1).reshape(M, -1) if flatten else a.mean(1)            # nn.Linear's column c S + s
    dv = gb @ wb + gc @ wc
    da = dv.reshape(M, C, S).permute(0, 2, 1) if flatten else (dv / S)[:, None, :].expand(M, S, C)
    dx = da * (x > 0) if relu else da.clone()
    return dict(x=x, wb=wb, wc=wc, bb=bb, bc=bc, gb=gb, gc=gc, box=v @ wb.T + bb, cls=v @ wc.T + bc, dx=dx, dwb=gb.T @ v, dwc=gc.T @ v, dbb=gb.sum(0), dbc=gc.sum(0))


def _op_run(ops, c, dtype, C, S, flatten, relu):
    x = c["x"].to(dtype).cuda()
    wcat = ops.box_head_pack(c["wb"].float().cuda(), c["wc"].float().cuda(), C, S if flatten else 1, dtype if flatten else torch.float32)
    box, cls, xmean = ops.box_head_out_fwd(x, wcat, c["bb"].float().cuda(), c["bc"].float().cuda(), flatten, relu)
    grads = [torch.ones(v.shape, dtype=torch.float32).cuda() for v in (c["dwb"], c["dwc"], c["dbb"], c["dbc"])]      # += : the buffers start at one
    dx = ops.box_head_out_bwd(x, wcat, xmean, c["gb"].float().cuda(), c["gc"].float().cuda(), c["wb"].shape[0], c["wc"].shape[0], flatten, relu, *grads)
    return box, cls, dx, grads


def _op_id(c):
    return f"{str(c[0])[6:]}-m{c[1]}-c{c[2]}s{c[3]}-{c[4]}+{c[5]}-{'flat' if c[6] else 'mean'}-{'relu' if c[7] else 'id'}"


@pytest.mark.parametrize("case", OP_CASES, ids=_op_id)
def test_output_kernels_against_float64(case):
    ops, _ = _m()
    dtype, M, C, S, reg, ncls, flatten, relu = case
    c = op_case(*case)
    assert M * S * C < 64 or ((c["x"] == 0).any() and (c["x"] < 0).any()), "x holds exact zeros and negatives"
    box, cls, dx, grads = _op_run(ops, c, dtype, C, S, flatten, relu)
    tag = _op_id(case)
    assert box.dtype == torch.float32 and tuple(box.shape) == (M, reg) and tuple(cls.shape) == (M, ncls)
    assert_close(box.cpu(), c["box"], 1e-3, f"{tag} pred_bbox_delta")
    assert_close(cls.cpu(), c["cls"], 1e-3, f"{tag} pred_scores")
    assert dx.dtype == dtype and dx.shape == c["dx"].shape
    got, want = dx.double().cpu(), c["dx"]
    assert_close(got, want, 1e-3 if dtype == torch.float32 else DX_STORE_TOL, f"{tag} dx")
    assert (got[want == 0] == 0).all(), "dx is exactly zero where the mask is"
    for name, g, w in zip(("dw_box", "dw_cls", "db_box", "db_cls"), grads, (c["dwb"], c["dwc"], c["dbb"], c["dbc"])):
        assert_close(g.double().cpu() - 1.0, w, 1e-3, f"{tag} {name}")
    again = _op_run(ops, c, dtype, C, S, flatten, relu)
    for a, b in zip([box, cls, dx, *grads], [again[0], again[1], again[2], *again[3]]):
        assert torch.equal(a, b), "two runs are bit-identical"


def test_entries_refuse_what_is_outside_the_limits():
    ops, D = _m()
    from nerf_mae_amd._lib import lib
    z = lambda *s: torch.zeros(s).cuda()
    x, w6, w2, b6, b2 = z(4, 6, 16), z(6, 96), z(2, 96), z(6), z(2)
    wcat = ops.box_head_pack(w6, w2, 16, 6, torch.float32)
    assert tuple(wcat.shape) == (8, 96)
    with pytest.raises(RuntimeError):
        ops.box_head_out_fwd(x.cpu(), wcat, b6, b2, True, False)
    with pytest.raises(NotImplementedError):
        ops.box_head_out_fwd(z(4, 6, 12), wcat, b6, b2, True, False)
    with pytest.raises(ValueError):
        ops.box_head_out_fwd(x, wcat, z(5), b2, True, False)                       # reg_dim 5
    with pytest.raises(ValueError):
        ops.box_head_out_fwd(x, wcat.bfloat16(), b6, b2, True, False)              # the weights are not in the activations' dtype
    with pytest.raises(ValueError):
        ops.box_head_out_fwd(z(4, ops.BOX_HEAD_MAX_CELLS + 1, 8), wcat, b6, b2, False, False)
    raw = lib().cdll
    out6, out2 = z(4, 6), z(4, 2)
    st = torch.cuda.current_stream().cuda_stream
    ok = lambda M, S, C, reg, ncls: raw.nmh_box_head_out_fwd(0, M, S, C, reg, ncls, 1, 0, x.data_ptr(), wcat.data_ptr(), b6.data_ptr(), b2.data_ptr(), None, out6.data_ptr(), out2.data_ptr(), st)
    assert ok(4, 6, 16, 6, 2) == 0
    for bad in ((0, 6, 16, 6, 2), (4, 0, 16, 6, 2), (4, 6, 12, 6, 2), (4, 6, 16, 5, 2), (4, 6, 16, 7, 26), (4, 513, 16, 6, 2), (65536, 6, 16, 6, 2)):
        assert ok(*bad) == -4, bad
    assert raw.nmh_box_head_out_fwd(0, 4, 6, 16, 6, 2, 0, 0, x.data_ptr(), wcat.data_ptr(), b6.data_ptr(), b2.data_ptr(), None, out6.data_ptr(), out2.data_ptr(), st) == -4   # mean form without xmean
    assert raw.nmh_box_head_bwd_ws_floats(0, 6, 16, 6, 2, 1) == -1
    torch.cuda.synchronize()
    head = D.FusedRCNN(16, None, 2, (2, 3, 1), compute_dtype=torch.float32).cuda()
    for bad in (z(3, 16, 2, 3, 2), z(3, 8, 2, 3, 1), z(0, 16, 2, 3, 1), z(3, 16, 6)):
        with pytest.raises(ValueError):
            head(bad)
    with pytest.raises(TypeError):
        head(z(3, 16, 2, 3, 1).double())
    with pytest.raises(RuntimeError):
        head(torch.zeros(3, 16, 2, 3, 1))


# ---- 3. / 4. the module ----------------------------------------------------------------------------------------------------------------------------
MOD_C, MOD_M, MOD_NCLS, MOD_SIZE = 16, 37, 2, (3, 3, 3)
MOD_IDS = ["-".join(("conv" if a else "noconv", "flat" if f else "mean", "obb" if r else "aabb")) for a, f, r in B.G_CONFIGS]


@functools.lru_cache(maxsize=None)
def mod_case(add_layer, flatten, rotated, M=MOD_M, C=MOD_C, size=MOD_SIZE, ncls=MOD_NCLS, want_rounded=True):
    x, P, cot_box, cot_cls = B.random_case(400 + 4 * add_layer + 2 * flatten + rotated, M, C, size, ncls, add_layer, flatten, rotated)
    x, P = x.float().double(), {k: v.float().double() for k, v in P.items()}
    exact = B.run(x, P, add_layer, flatten, cot_box, cot_cls)
    rounded = B.run(x, P, add_layer, flatten, cot_box, cot_cls, B.round_bf16) if want_rounded else None
    return dict(x=x, P=P, cot_box=cot_box, cot_cls=cot_cls, exact=exact, rounded=rounded, C=C, size=size, ncls=ncls)


def _head(D, c, add_layer, flatten, rotated, dtype):
    head = D.FusedRCNN(c["C"], None, c["ncls"], c["size"], add_layer, rotated, flatten, compute_dtype=dtype)
    head.load_state_dict({k: v.float() for k, v in c["P"].items()}, strict=True)
    return head.cuda()


def _mod_run(D, c, add_layer, flatten, rotated, dtype, cot=(True, True), head=None):
    head = _head(D, c, add_layer, flatten, rotated, dtype) if head is None else head
    x = c["x"].float().cuda().requires_grad_(True)
    box, cls = head(x)
    total = sum((o * t.float().cuda()).sum() for o, t, on in ((box, c["cot_box"], cot[0]), (cls, c["cot_cls"], cot[1])) if on)
    total.backward()
    return dict(box=box.detach(), cls=cls.detach(), dx=x.grad, dparam={k: p.grad for k, p in head.named_parameters()}), head


@pytest.mark.parametrize("add_layer,flatten,rotated", B.G_CONFIGS, ids=MOD_IDS)
def test_module_fp32_against_float64(add_layer, flatten, rotated):
    _, D = _m()
    c = mod_case(add_layer, flatten, rotated)
    got, _ = _mod_run(D, c, add_layer, flatten, rotated, torch.float32)
    assert list(got["dparam"]) == B.keys(add_layer)
    assert got["box"].dtype == torch.float32 and tuple(got["box"].shape) == (MOD_M, 7 if rotated else 6) and tuple(got["dx"].shape) == tuple(c["x"].shape)
    want = B.quantities(c["exact"])
    for name, a in B.quantities(got).items():
        assert a is not None, f"{name}: no gradient"
        assert_close(a.cpu(), want[name], 1e-3, f"fp32 {add_layer} {flatten} {rotated} {name}")


@pytest.mark.parametrize("size", B.G_SIZES, ids=["3x3x3", "2x3x1"])
@pytest.mark.parametrize("add_layer,flatten,rotated", B.G_CONFIGS, ids=MOD_IDS)
def test_recorded_reference_after_a_strict_load(size, add_layer, flatten, rotated):
    _, D = _m()
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "g32_box_head.npz")))
    pre = B.golden_prefix(size, add_layer, flatten, rotated)
    x, P, cot_box, cot_cls = B.golden_case(size, add_layer, flatten, rotated)
    c = dict(x=x, P=P, cot_box=cot_box, cot_cls=cot_cls, C=B.G_C, size=size, ncls=B.G_NCLS)
    got, _ = _mod_run(D, c, add_layer, flatten, rotated, torch.float32)
    for name, a in (("box", got["box"]), ("cls", got["cls"]), ("dx", got["dx"])):
        assert_close(a.cpu(), torch.from_numpy(g[pre + name]), 1e-3, f"g32 {pre}{name}")
    for k, grad in got["dparam"].items():
        assert_close(B.recorded_view(k, grad.cpu(), flatten), torch.from_numpy(g[pre + "d_" + k]), 1e-3, f"g32 {pre}d {k}")


@pytest.mark.parametrize("add_layer,flatten,rotated", B.G_CONFIGS, ids=MOD_IDS)
def test_module_bf16_within_twice_the_rounding_error(add_layer, flatten, rotated):
    _, D = _m()
    c = mod_case(add_layer, flatten, rotated)
    tag = f"bf16 conv {add_layer} flatten {flatten} rotated {rotated}"
    want, rnd = B.quantities(c["exact"]), B.quantities(c["rounded"])
    e_round = {name: B.max_err(rnd[name], want[name]) for name in want}
    got = B.quantities(_mod_run(D, c, add_layer, flatten, rotated, torch.bfloat16)[0])
    e_kernel = {name: B.max_err(got[name].cpu(), want[name]) for name in want}
    print(f"{tag}: e_round {max(e_round.values()):.3e}  kernel {max(e_kernel.values()):.3e}")
    assert max(e_round.values()) > 0
    for name in want:
        bound = 2 * e_round[name] if e_round[name] > 0 else 1e-3      # no stored tensor reaches the two output biases' gradients: the fp32 contract
        print(f"    {name:28s} e_round {e_round[name]:.3e}  kernel {e_kernel[name]:.3e}  bound {bound:.3e}")
        assert e_kernel[name] <= bound, f"{tag} {name}: kernel error {e_kernel[name]:.3e} > {bound:.3e} (e_round {e_round[name]:.3e})"


# ---- 5. row independence ---------------------------------------------------------------------------------------------------------------------------
# C 64 at 3^3: the shared conv layer picks its tile by (rows x cells <= 8192 or a short contraction), so 300 and 310 rows stand on either side of that choice
# and a single row or 96 on the first; C 16 at (2, 3, 1): a contraction of 432 and partial 8-channel steps.
@pytest.mark.parametrize("M,C,size", [(300, 64, (3, 3, 3)), (310, 64, (3, 3, 3)), (300, 16, (2, 3, 1))], ids=["m300-c64-3x3x3", "m310-c64-3x3x3", "m300-c16-2x3x1"])
@pytest.mark.parametrize("flatten", [True, False], ids=["flat", "mean"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_a_rows_bits_do_not_depend_on_the_other_rows(dtype, flatten, M, C, size):
    _, D = _m()
    c = mod_case(True, flatten, True, M=M, C=C, size=size, want_rounded=False)
    head = _head(D, c, True, flatten, True, dtype)
    x = c["x"].float().cuda()
    with torch.no_grad():
        whole = head(x)
        for r in (0, 129, M - 1):
            one = head(x[r:r + 1])
            assert all(torch.equal(a[0], b[r]) for a, b in zip(one, whole)), f"row {r} alone"
        perm = torch.randperm(M, generator=torch.Generator().manual_seed(M)).cuda()
        shuffled = head(x[perm])
        assert all(torch.equal(a, b[perm]) for a, b in zip(shuffled, whole)), "a permutation of the rows"
        parts = [head(x[m0:m0 + 96]) for m0 in range(0, M, 96)]
        assert all(torch.equal(torch.cat([p[k] for p in parts]), whole[k]) for k in range(2)), "sub-batches of 96"


# ---- 6. run-to-run identity, accumulation, None cotangents -----------------------------------------------------------------------------------------
# M = 130 at 3^3 is 3510 voxels: the conv weight gradient's contraction has four splits there, M = 37 one; 64 channels in bf16 take its 96 x 96 tile kernel
@pytest.mark.parametrize("M,C", [(37, 16), (130, 16), (130, 64)], ids=["m37-c16", "m130-c16", "m130-c64"])
@pytest.mark.parametrize("add_layer,flatten", [(a, f) for a in (False, True) for f in (False, True)], ids=["noconv-mean", "noconv-flat", "conv-mean", "conv-flat"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_two_runs_are_bit_identical_and_a_second_backward_doubles(dtype, add_layer, flatten, M, C):
    _, D = _m()
    c = mod_case(add_layer, flatten, True, M=M, C=C, want_rounded=False)
    a, head = _mod_run(D, c, add_layer, flatten, True, dtype)
    b, _ = _mod_run(D, c, add_layer, flatten, True, dtype)
    qa, qb = B.quantities(a), B.quantities(b)
    for name in qa:
        assert torch.equal(qa[name], qb[name]), f"{name}: two runs are bit-identical"
    once = {k: v.clone() for k, v in a["dparam"].items()}
    _mod_run(D, c, add_layer, flatten, True, dtype, head=head)                     # the same .grad buffers
    for k, p in head.named_parameters():
        assert torch.equal(p.grad, 2 * once[k]), f"{k}: a second backward doubles the gradient exactly"
    for cot, untouched in (((True, False), "RCNN_cls_score"), ((False, True), "RCNN_bbox_pred")):
        head.zero_grad(set_to_none=False)
        for k, p in head.named_parameters():
            if k.startswith(untouched):
                p.grad.fill_(3.0)
        got, _ = _mod_run(D, c, add_layer, flatten, True, dtype, cot=cot, head=head)
        for k, p in head.named_parameters():
            if k.startswith(untouched):
                assert (p.grad == 3.0).all(), f"{k}: untouched without a cotangent"
            else:
                assert p.grad.abs().sum() > 0, k
        want = B.run(c["x"], c["P"], add_layer, flatten, c["cot_box"] if cot[0] else None, c["cot_cls"] if cot[1] else None)
        if dtype == torch.float32:
            assert_close(got["dx"].cpu(), want["dx"], 1e-3, f"d pooled with cotangents {cot}")


@pytest.mark.parametrize("add_layer", [False, True], ids=["noconv", "conv"])
def test_parameters_get_their_gradients_when_the_pooled_tensor_needs_none(add_layer):
    """a head trained on stored features: nothing upstream requires a gradient, the kernels still fill .grad, with the bits of the run whose input does"""
    _, D = _m()
    c = mod_case(add_layer, True, True, want_rounded=False)
    want, _ = _mod_run(D, c, add_layer, True, True, torch.bfloat16)
    head = _head(D, c, add_layer, True, True, torch.bfloat16)
    box, cls = head(c["x"].float().cuda())
    assert box.requires_grad and cls.requires_grad
    ((box * c["cot_box"].float().cuda()).sum() + (cls * c["cot_cls"].float().cuda()).sum()).backward()
    assert list(dict(head.named_parameters())) == B.keys(add_layer)
    for k, p in head.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, want["dparam"][k]), k
    with torch.no_grad():
        assert not head(c["x"].float().cuda())[0].requires_grad


# ---- 7. inside the stage ---------------------------------------------------------------------------------------------------------------------------
def _stage(D, H, head, rotated, seed=3):
    layer = D.ProposalTargetLayer(2, batch_size=H.GOLD["N"] * H.GOLD["R"], fg_fraction=0.5, fg_threshold=H.FG, bg_threshold=H.BG, is_rotated_bbox=rotated, seed=seed)
    pool = D.ROIPool(H.GOLD["out"], H.SCALES, H.ENLARGE, rotated, "pooling", H.GOLD["max_res"], False)
    return D.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=rotated)


@pytest.mark.parametrize("add_layer", [False, True], ids=["noconv", "conv"])
@pytest.mark.parametrize("pre,rotated", [("a_", False), ("o_", True)])
def test_inside_classification_model_against_the_stock_head(pre, rotated, add_layer):
    """tests/_roi_head_ref's recorded small case (its RoIs, boxes, labels and the recorded keep rows) with maps of 8 channels in place of its 4: the fused head
    takes multiples of 8"""
    _, D = _m()
    from tests import _roi_head_ref as H
    gold = np.load(os.path.join(ROOT, "tests", "golden", "g22_roi_head.npz"))
    C = 8
    rois, gts, labs, _ = H.gold_inputs(rotated)
    maps = H.make_maps(H.GOLD_SEED[rotated][1], C, H.GOLD["N"])
    torch.manual_seed(11)
    stock = D.RCNN(C, None, 2, H.GOLD["out"], add_layer, rotated, True)
    fused = D.FusedRCNN(C, None, 2, H.GOLD["out"], add_layer, rotated, True, compute_dtype=torch.float32)
    fused.load_state_dict(stock.state_dict(), strict=True)
    keep, n_fg = gold[pre + "keep"], gold[pre + "n_fg"]
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda()
    res = []
    for head in (stock.cuda(), fused.cuda()):
        model = _stage(D, H, head, rotated)
        leaves = [t.cuda().requires_grad_(True) for t in maps]
        _, _, loss = model([r.cuda() for r in rois], [g.cuda() for g in gts], [l.cuda() for l in labs], leaves, is_sample=True, is_reg=True,
                           keep=i32(keep), keep_counts=i32(np.stack([n_fg, keep.shape[1] - n_fg], 1)))
        (loss["loss_objectness"] + loss["loss_rpn_box_reg"]).backward()
        res.append((torch.stack([loss["loss_objectness"], loss["loss_rpn_box_reg"]]).detach(), [t.grad for t in leaves], {k: p.grad for k, p in head.named_parameters()}))
    (la, ga, pa), (lb, gb, pb) = res
    assert float(la.min()) > 0
    assert_close(lb.cpu(), la.cpu().double(), 1e-3, "losses")
    for k, (a, b) in enumerate(zip(ga, gb)):
        assert a.abs().sum() > 0 or k > 0
        if a.abs().sum() > 0:
            assert_close(b.cpu(), a.cpu().double(), 1e-3, f"map gradient, level {k}")
        else:
            assert not b.any(), f"map gradient, level {k}: zero"
    for k in pa:
        assert_close(pb[k].cpu(), pa[k].cpu().double(), 1e-3, f"d {k}")


# ---- 8. / 9. the detector ---------------------------------------------------------------------------------------------------------------------------
def _fused_two_stage(seed, dtype=torch.float32, **kw):
    """tests/_two_stage_ref.two_stage with the stock head's parameters in a FusedRCNN"""
    _, D = _m()
    from tests._two_stage_ref import OUT, two_stage
    det = two_stage(seed, **kw)
    stock = det.roi_model.RCNN_model
    fused = D.FusedRCNN(stock.in_planes, None, 2, OUT, is_add_layer=False, is_rotated_bbox=False, is_flatten=True, compute_dtype=dtype)
    fused.load_state_dict(stock.state_dict(), strict=True)
    det.roi_model.RCNN_model = fused.cuda()
    return det


@pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16"])
def test_predict_dense_gives_the_same_bits_for_every_chunking(dtype):
    from tests._two_stage_ref import scenes
    det = _fused_two_stage(0, dtype).eval()
    meshes, _ = scenes()
    with torch.no_grad():
        features, (pb, pl, pc), _, _ = det._first_stage(meshes)
        whole = det.roi_model.predict_dense(pb, pl, pc, features)
        assert pb.shape[1] > 96 and pb.shape[1] % 96
        for chunk in (96, 1):
            parts = det.roi_model.predict_dense(pb, pl, pc, features, chunk_rows=chunk)
            for a, b in zip(whole, parts):
                assert torch.equal(a, b), f"chunk_rows {chunk}"


def test_three_finetune_steps_match_the_stock_head():
    """FinetuneStep over the detector with the fused head (A) against the same steps over the detector with the stock head (B; B' its own second run), the
    sampler given the same keep rows: relerr(A, B) <= 3e-5 + 4 relerr(B, B'), on the losses of every step and on every trainable parameter"""
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for
    from nerf_mae_amd.trainer import FusedAdamW
    from tests import _finetune_common as C
    from tests._two_stage_ref import ROWS, scenes, two_stage
    LR, WD, EPS, CLIP = 1e-4, 1e-2, 1e-8, 1.0
    rows = ROWS // 2
    keep = torch.arange(rows, dtype=torch.int32).repeat(2, 1).cuda()
    kc = torch.tensor([[rows // 2, rows - rows // 2]] * 2, dtype=torch.int32).cuda()

    def steps(det):
        det = det.train()
        flat = FlatParameters(det, torch.device("cuda"))
        opt = FusedAdamW(flat, lr=LR, weight_decay=WD, eps=EPS, max_grad_norm=CLIP)
        step = FinetuneStep(flat, opt, loss_fn_for(det), weights={"loss_rpn_box_reg": 2.0})
        meshes, targets = scenes()
        out = []
        for _ in range(3):
            o = step(meshes, targets, keep, kc)
            out.append(torch.stack([o["loss_objectness"], o["loss_rpn_box_reg"]]))
        return det, torch.stack(out)

    b, lb = steps(two_stage(0))
    b2, lb2 = steps(two_stage(0))
    a, la = steps(_fused_two_stage(0))
    assert torch.isfinite(la).all() and float(la[:, 0].min()) > 0
    spread = max(relerr(lb2, lb), max(relerr(q, p) for (_, p), (_, q) in zip(C.trainable(b), C.trainable(b2))))
    bound = 3e-5 + 4 * spread
    assert relerr(la, lb) <= bound, (relerr(la, lb), bound)
    assert [n for n, _ in C.trainable(a)] == [n for n, _ in C.trainable(b)]
    for (n, p), (_, q) in zip(C.trainable(b), C.trainable(a)):
        assert relerr(q, p) <= bound, (n, relerr(q, p), bound)


def test_a_checkpoint_moves_between_the_two_head_classes(tmp_path):
    from nerf_mae_amd.trainer import load_two_stage_checkpoint, save_two_stage_checkpoint
    from tests._two_stage_ref import scenes, two_stage
    meshes, _ = scenes()
    for src, dst in ((two_stage(0), _fused_two_stage(5)), (_fused_two_stage(0), two_stage(5))):
        src, dst = src.eval(), dst.eval()
        path = str(tmp_path / f"{type(src.roi_model.RCNN_model).__name__}.pt")
        save_two_stage_checkpoint(path, src, 1, {"rotated_bbox": False})
        load_two_stage_checkpoint(path, dst)
        for (k, p), (_, q) in zip(src.state_dict().items(), dst.state_dict().items()):
            assert torch.equal(p, q), k
        want, got = src.detections_dense(meshes), dst.detections_dense(meshes)
        assert int(want[2].min()) > 0 and torch.equal(want[2], got[2]), "the same number of detections"
        assert_close(got[0].cpu(), want[0].cpu().double(), 1e-3, "boxes")
        assert_close(got[1].cpu(), want[1].cpu().double(), 1e-3, "scores")


# ---- 10. capture -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("add_layer,flatten", [(True, True), (False, False)], ids=["conv-flat", "noconv-mean"])
def test_forward_in_a_captured_graph(add_layer, flatten):
    _, D = _m()
    c = mod_case(add_layer, flatten, True, want_rounded=False)
    head = _head(D, c, add_layer, flatten, True, torch.bfloat16)
    first = c["x"].float().cuda()
    second = first.flip(0).contiguous() * 0.5
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():             # warmed up and captured on one side stream (Capture)
        x = first.clone()
        head(x)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"), torch.no_grad():
        out = head(x)
    for data in (second, first):
        x.copy_(data)
        graph.replay()
        torch.cuda.synchronize()
        with torch.no_grad():
            eager = head(data)
        assert all(torch.equal(a, b) for a, b in zip(out, eager)), "the replay gives the bits of the eager call"
