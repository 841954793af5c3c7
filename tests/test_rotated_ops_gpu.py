"""Rotated 3-D RoIAlign (forward + input gradient, channels-last and NCWLH) and the polygon vertex sort against the float64 restatements of
tests/_rotated_ref.py.  The reference's own ops are CUDA and cannot run here, so nothing of them is recorded; the restatement is checked
against analytic results in tests/test_rotated_ops_cpu.py.

Tolerances.  fp32: the project's contract, assert_close(rtol=1e-3).  bf16 forward: the restatement is evaluated on the bf16-rounded
map, a bin is a convex combination of map values accumulated in fp32 and rounded to bf16 once, so rtol = 2**-8 (one bf16 rounding is
2**-9).  The backward is fp32 for either dtype: rtol = 1e-3.
The op is discontinuous where a sample coordinate crosses -1 or the extent and, at sampling_ratio 0, where size / pooled crosses an
integer; bins with a sample within 1e-4 of such a place (about ten times the fp32 coordinate error at these magnitudes) are left out, and
the tests assert that this is at most 2 % of the bins.
Measured on an MI355X (NMH_PRINT_ERR=1): see DESIGN.md, "Rotated RoIAlign and vertex sort"."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rotated_ref as R  # noqa: E402
from tests._metrics import assert_close, relerr  # noqa: E402

pytestmark = pytest.mark.gpu

SCALE, POOLED, DELTA = 0.5, (3, 2, 4), 1e-4
MAPS = ((12, 12, 12), (10, 12, 14))
CL, NC = "channels_last", "ncwlh"


def _rot():
    from nerf_mae_amd import rotated
    return rotated


def _ops():
    from nerf_mae_amd import ops
    return ops


def to_nc(t):
    """(.., a, b, c, C) channels-last -> (.., C, a, b, c)"""
    return t.permute(0, 4, 1, 2, 3).contiguous()


def run_fwd(x_cl, rois, pooled, scale, sr, layout):
    """x_cl (B,W,L,H,C) on the host in its dtype -> output as channels-last [N,PW,PL,PH,C] on the host"""
    rot = _rot()
    if layout == CL:
        return rot.roi_align_rotated_3d_channels_last(x_cl.cuda(), rois.cuda(), pooled, scale, sr).cpu()
    out = rot.roi_align_rotated_3d(to_nc(x_cl).cuda(), rois.cuda(), pooled, scale, sr)
    return out.permute(0, 2, 3, 4, 1).contiguous().cpu()


def run_bwd(dout_cl, rois, shape_cl, pooled, scale, sr, layout):
    """dout_cl [N,PW,PL,PH,C] on the host -> fp32 gradient as channels-last (B,W,L,H,C) on the host; the wrapper zeroes the buffer"""
    ops = _ops()
    if layout == CL:
        return ops.roi_align_rotated_3d_bwd(dout_cl.cuda().contiguous(), rois.cuda(), shape_cl, pooled, scale, sr, ops.ROI_CHANNELS_LAST).cpu()
    B, W, L, H, C = shape_cl
    dx = ops.roi_align_rotated_3d_bwd(to_nc(dout_cl).cuda(), rois.cuda(), (B, C, W, L, H), pooled, scale, sr, ops.ROI_NCWLH)
    return dx.permute(0, 2, 3, 4, 1).contiguous().cpu()


@functools.lru_cache(maxsize=None)
def case(dims, C, sr, bf16=False, overlap=False):
    """inputs and float64 results of one configuration: map, rois, reference output + meta, dout and reference gradient"""
    g = torch.Generator().manual_seed(1000 * dims[2] + C + sr)
    x = torch.randn((2, *dims, C), generator=g)
    if bf16:
        x = x.bfloat16()
    rois = R.make_rois(0, 64, dims, SCALE)
    if overlap:   # 32 more boxes that all cover the middle of the map of batch item 0: many adds land on the same voxels
        r = np.random.default_rng(1)
        ctr = np.array(dims) / 2 + r.uniform(-0.75, 0.75, (32, 3))
        size = np.array(dims) * r.uniform(0.45, 0.6, (32, 3))
        extra = np.concatenate([np.zeros((32, 1)), ctr / SCALE, size / SCALE, r.uniform(-180, 180, (32, 1))], 1)
        rois = torch.cat([rois, torch.from_numpy(extra.astype(np.float32))])
    xr = x.double().requires_grad_(True)
    ref, meta = R.roi_align_ref(xr, rois, POOLED, SCALE, sr)
    keep = meta["margin"] >= DELTA
    dout = torch.randn(ref.shape, generator=g) * keep[..., None]
    if bf16:
        dout = dout.bfloat16()
    (dref,) = torch.autograd.grad(ref, xr, dout.double())
    return x, rois, ref.detach(), keep, meta["outside"], dout, dref


def _check_coverage(keep, outside):
    left_out = 1.0 - keep.double().mean().item()
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  bins left out {left_out:.4f}, samples contributing 0: {outside:.3f}")
    assert left_out <= 0.02, left_out
    assert 0.10 <= outside <= 0.60, outside


# ---- 1. forward, fp32, both layouts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (CL, NC))
@pytest.mark.parametrize("sr", (2, 0))
@pytest.mark.parametrize("C", (16, 256))
@pytest.mark.parametrize("dims", MAPS)
def test_forward_fp32(dims, C, sr, layout):
    x, rois, ref, keep, outside, _, _ = case(dims, C, sr)
    _check_coverage(keep, outside)
    out = run_fwd(x, rois, POOLED, SCALE, sr, layout)
    assert out.shape == ref.shape and out.dtype == torch.float32
    assert_close(out[keep], ref[keep], 1e-3, f"roi fwd {layout} {dims} C{C} sr{sr}")


# ---- 2. forward, bf16 channels-last -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", (2, 0))
@pytest.mark.parametrize("C", (16, 256))
@pytest.mark.parametrize("dims", MAPS)
def test_forward_bf16_channels_last(dims, C, sr):
    x, rois, ref, keep, outside, _, _ = case(dims, C, sr, bf16=True)
    _check_coverage(keep, outside)
    out = run_fwd(x, rois, POOLED, SCALE, sr, CL)
    assert out.dtype == torch.bfloat16
    assert_close(out[keep], ref[keep], 2.0 ** -8, f"roi fwd bf16 {dims} C{C} sr{sr}")


# ---- 3. backward, fp32 and bf16, both layouts, with heavily overlapping ROIs ---------------------------------------------------------------
@pytest.mark.parametrize("layout,bf16", ((CL, False), (CL, True), (NC, False)))
@pytest.mark.parametrize("sr", (2, 0))
@pytest.mark.parametrize("C", (16, 256))
@pytest.mark.parametrize("dims", MAPS)
def test_backward(dims, C, sr, layout, bf16):
    x, rois, ref, keep, _, dout, dref = case(dims, C, sr, bf16=bf16, overlap=True)
    assert 1.0 - keep.double().mean().item() <= 0.02
    dx = run_bwd(dout, rois, tuple(x.shape), POOLED, SCALE, sr, layout)
    assert dx.dtype == torch.float32 and dx.shape == dref.shape
    assert_close(dx, dref, 1e-3, f"roi bwd {layout} {'bf16' if bf16 else 'fp32'} {dims} C{C} sr{sr}")


@pytest.mark.parametrize("layout", (CL, NC))
def test_backward_leaves_unreached_voxels_exactly_zero(layout):
    dims, C = (10, 12, 14), 16
    r = np.random.default_rng(2)
    n = 12     # boxes of at most 3 voxels in the low corner of batch item 1: most of the map is reached by no sample
    rois = np.concatenate([np.ones((n, 1)), r.uniform(1.5, 3.0, (n, 3)) / SCALE, r.uniform(1.0, 3.0, (n, 3)) / SCALE, r.uniform(-180, 180, (n, 1))], 1)
    rois = torch.from_numpy(rois.astype(np.float32))
    xr = torch.zeros((2, *dims, C), dtype=torch.float64, requires_grad=True)
    ref, meta = R.roi_align_ref(xr, rois, POOLED, SCALE, 0)
    dout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(3)) * (meta["margin"] >= DELTA)[..., None]
    (dref,) = torch.autograd.grad(ref, xr, dout.double())
    dx = run_bwd(dout, rois, tuple(xr.shape), POOLED, SCALE, 0, layout)
    unreached = dref == 0
    assert unreached[0].all() and 0.5 < unreached.double().mean().item() < 1.0
    assert (dx[unreached] == 0).all()
    assert relerr(dx, dref) < 1e-3


# ---- 4. the two layouts are the same arithmetic ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", (2, 0))
def test_layouts_agree(sr):
    x, rois, _, _, _, dout, _ = case((10, 12, 14), 16, sr, overlap=True)
    a, b = run_fwd(x, rois, POOLED, SCALE, sr, CL), run_fwd(x, rois, POOLED, SCALE, sr, NC)
    assert relerr(a, b) <= 1e-6
    # the gradient is a sum of atomic adds whose order differs from run to run: rounding of an fp32 sum of ~100 terms, not 1e-6
    ga, gb = (run_bwd(dout, rois, tuple(x.shape), POOLED, SCALE, sr, lay) for lay in (CL, NC))
    assert relerr(ga, gb) <= 1e-5


# ---- 5. the stride deviation: voxel (x, y, z) of a (W, L, H) map is element (x L + y) H + z ------------------------------------------------
@pytest.mark.parametrize("layout", (CL, NC))
def test_non_cubic_strides(layout):
    dims, C, vox = (10, 12, 14), 8, (3, 7, 11)
    x = torch.zeros((1, *dims, C))
    x[0, vox[0], vox[1], vox[2]] = 1.0
    # axis-aligned box of bins of edge 1 placed so that the voxel is the centre of bin (1, 1, 1)
    rois = torch.tensor([[0.0, 3.0, 6.5, 11.5, 3.0, 2.0, 4.0, 0.0]])
    out = run_fwd(x, rois, POOLED, 1.0, 2, layout)
    assert out.shape == (1, 3, 2, 4, C)
    peak = np.unravel_index(out[0, ..., 0].argmax().item(), POOLED)
    assert peak == (1, 1, 1), peak
    assert abs(out[0, 1, 1, 1, 0].item() - 0.75 ** 3) < 1e-6      # samples at +-0.25 from the voxel on every axis
    dout = torch.zeros_like(out)
    dout[0, 1, 1, 1] = 1.0
    dx = run_bwd(dout, rois, tuple(x.shape), POOLED, 1.0, 2, layout)
    gpeak = np.unravel_index(dx[0, ..., 0].argmax().item(), dims)
    assert gpeak == vox, gpeak
    assert abs(dx[0, 3, 7, 11, 0].item() - 0.75 ** 3) < 1e-6 and abs(dx.sum().item() - C) < 1e-4


# ---- 6. edges --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (CL, NC))
def test_edges(layout):
    rot = _rot()
    dims, C = (10, 12, 14), 16
    g = torch.Generator().manual_seed(6)
    x = torch.randn((2, *dims, C), generator=g)

    def fwd_bwd(rois, sr=0):
        xin = (x if layout == CL else to_nc(x)).cuda().requires_grad_(True)
        fn = rot.roi_align_rotated_3d_channels_last if layout == CL else rot.roi_align_rotated_3d
        out = fn(xin, rois.cuda(), POOLED, SCALE, sr)
        out.sum().backward()
        torch.cuda.synchronize()
        o, gx = out.detach().cpu(), xin.grad.cpu()
        return (o, gx) if layout == CL else (o.permute(0, 2, 3, 4, 1), gx.permute(0, 2, 3, 4, 1))

    # N = 0
    o, gx = fwd_bwd(torch.zeros((0, 8)))
    assert o.shape[0] == 0 and o.numel() == 0 and (gx == 0).all()
    # a size below 1 after scaling is the size 1
    small = torch.tensor([[1.0, 9.0, 11.0, 13.0, 0.2, 1.0, 0.02, 25.0]])
    unit = torch.tensor([[1.0, 9.0, 11.0, 13.0, 2.0, 2.0, 2.0, 25.0]])
    (o1, g1), (o2, g2) = fwd_bwd(small), fwd_bwd(unit)
    assert torch.equal(o1, o2) and relerr(g1, g2) <= 1e-5 and o1.abs().max() > 0    # (atomic adds: the order of a voxel's sum varies)
    # a full turn: the angle is reduced exactly, so nothing but the sign of a zero can differ
    base = R.make_rois(5, 16, dims, SCALE)
    base[:, 7] = 0.0
    turned = base.clone()
    turned[:, 7] = 360.0
    (o1, g1), (o2, g2) = fwd_bwd(base), fwd_bwd(turned)
    assert relerr(o2, o1) <= 1e-6 and relerr(g2, g1) <= 1e-5
    # wholly outside the map
    o, gx = fwd_bwd(torch.tensor([[0.0, -20.0, 5.0, 5.0, 6.0, 6.0, 6.0, 30.0], [1.0, 10.0, 12.0, 60.0, 8.0, 8.0, 8.0, 0.0]]))
    assert (o == 0).all() and (gx == 0).all()
    # a batch index outside [0, B): that ROI gives zeros and no gradient, the others are what they are without it
    good = R.make_rois(7, 6, dims, SCALE)
    bad = good.clone()
    bad[:, 0] = torch.tensor([-1.0, 2.0, 7.0, -3.0, 1.0e9, 2.0])
    mixed = torch.cat([good[:3], bad, good[3:]])
    (o1, g1), (o2, g2) = fwd_bwd(good), fwd_bwd(mixed)
    assert (o2[3:9] == 0).all()
    assert torch.equal(torch.cat([o2[:3], o2[9:]]), o1)
    assert relerr(g2, g1) <= 1e-5 and g1.abs().max() > 0


def test_channels_last_needs_a_multiple_of_8_channels():
    from nerf_mae_amd._lib import NmhError
    x = torch.zeros((1, 4, 4, 4, 12), device="cuda")
    with pytest.raises(NmhError):
        _rot().roi_align_rotated_3d_channels_last(x, torch.tensor([[0.0, 2, 2, 2, 2, 2, 2, 0]], device="cuda"), (2, 2, 2), 1.0, 2)


# ---- 7. the downstream shape: launch + spot check -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", (CL, NC))
def test_full_downstream_shape(layout):
    rot = _rot()
    dims, C, pooled, n = (40, 40, 40), 256, (7, 7, 7), 512
    g = torch.Generator().manual_seed(7)
    x = torch.randn((2, *dims, C), generator=g)
    r = np.random.default_rng(7)
    rois = np.concatenate([(np.arange(n) % 2)[:, None], r.uniform(0, 40, (n, 3)), r.uniform(4, 30, (n, 3)), r.uniform(-180, 180, (n, 1))], 1)
    rois = torch.from_numpy(rois.astype(np.float32))
    xg = x.cuda()
    if layout == CL:
        out = rot.roi_align_rotated_3d_channels_last(xg, rois.cuda(), pooled, 1.0, 0)
        assert out.shape == (n, 7, 7, 7, C)
    else:
        out = rot.ROIAlignRotated3D(pooled, 0)(xg.permute(0, 4, 1, 2, 3).contiguous(), rois.cuda(), 1.0)
        assert out.shape == (n, C, 7, 7, 7)
    assert torch.isfinite(out).all().item()
    which = [(int(r.integers(n)), int(r.integers(7)), int(r.integers(7)), int(r.integers(7))) for _ in range(64)]
    ref, margin = R.roi_align_ref_bins(x.double(), rois, pooled, 1.0, 0, which)
    got = torch.stack([(out[a, b, c, d] if layout == CL else out[a, :, b, c, d]).cpu() for a, b, c, d in which])
    keep = margin >= DELTA
    assert keep.sum().item() >= 60
    assert_close(got[keep], ref[keep], 1e-3, f"roi fwd 40^3 C256 {layout}")


# ---- 8. vertex sort ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def polygons(count=4096, seed=8):
    """`count` intersections of pairs of rotated rectangles with >= 3 vertices whose polar angles about their mean are all >= 1e-3 rad
    apart (pairs that do not qualify are drawn again): float64 vertices (count,24,2), masks, num_valid, the two boxes"""
    r = np.random.default_rng(seed)
    V, M, B1, B2 = [], [], [], []
    while len(V) < count:
        c1 = R.rect_corners(r.uniform(-1, 1), r.uniform(-1, 1), r.uniform(0.5, 3), r.uniform(0.5, 3), r.uniform(-np.pi, np.pi))
        c2 = R.rect_corners(r.uniform(-1, 1), r.uniform(-1, 1), r.uniform(0.5, 3), r.uniform(0.5, 3), r.uniform(-np.pi, np.pi))
        v, m = R.box_pair_vertices(c1, c2)
        if m.sum() < 3 or m.sum() > 8 or _min_gap(v, m) < 2e-3:
            continue
        V.append(v), M.append(m), B1.append(c1), B2.append(c2)
    V, M = np.stack(V), np.stack(M)
    return V, M, M.sum(1).astype(np.int32), B1, B2


def _centred(v, m):
    return v - (v * m[:, None]).sum(0) / m.sum()


def _min_gap(v, m):
    c = _centred(v, m)[m]
    a = np.sort(R.polar_angle(c[:, 0], c[:, 1]))
    return float(np.min(np.diff(np.concatenate([a, a[:1] + 2 * np.pi]))))


def _sort_gpu(vc, m, nv):
    """vc (B,N,M,2) float64 centred, m (B,N,M) bool, nv (B,N) -> idx (B,N,9) NumPy"""
    idx = _rot().sort_v(torch.from_numpy(vc.astype(np.float32)).cuda(), torch.from_numpy(m).cuda(), torch.from_numpy(nv.astype(np.int32)).cuda())
    assert idx.dtype == torch.int32 and idx.shape == (*m.shape[:2], 9)
    return idx.cpu().numpy()


def test_sort_matches_restatement_and_areas():
    V, M, nv, B1, B2 = polygons()
    vc = np.stack([_centred(v, m) for v, m in zip(V, M)])
    vc32 = vc.astype(np.float32).astype(np.float64)
    assert min(_min_gap(v, m) for v, m in zip(V, M)) >= 1e-3
    assert set(np.unique(nv)) >= {3, 4, 5, 6, 7, 8}
    shape = (8, 512)
    idx = _sort_gpu(vc.reshape(*shape, 24, 2), M.reshape(*shape, 24), nv.reshape(shape)).reshape(-1, 9)
    ref = R.sort_vertices_ref(vc32.reshape(*shape, 24, 2), M.reshape(*shape, 24), nv.reshape(shape)).reshape(-1, 9)
    assert np.array_equal(idx, ref), np.nonzero((idx != ref).any(1))[0][:10]
    worst, checked = 0.0, 0
    for i in range(len(V)):
        want = R.clip_area(B1[i], B2[i])
        if want <= 1e-3:
            continue
        got = R.shoelace(V[i][idx[i, :nv[i]]])
        worst, checked = max(worst, abs(got - want) / want), checked + 1
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  shoelace vs clip: worst relative difference {worst:.2e} over {checked} polygons")
    assert checked > 3500 and worst <= 1e-5, (checked, worst)


def test_sort_fewer_than_three_valid_vertices():
    V, M, nv, _, _ = polygons()
    v, m = V[:6].copy(), np.zeros((6, 24), dtype=bool)
    m[1, 2] = True
    m[2, [0, 9]] = True
    m[3, 8] = True                     # pad is the first unmasked slot from 8 on: 9 here
    m[4, [8, 9, 10]] = True            # three valid ones: sorted, not padded
    v[4, [8, 9, 10]] = [[-1.0, 0.5], [0.0, -1.0], [1.0, 0.5]]
    m[5, [8, 11]] = True
    n = m.sum(1).astype(np.int32)
    idx = _sort_gpu(v[None], m[None], n[None])[0]
    for i, pad in ((0, 8), (1, 8), (2, 8), (3, 9), (5, 9)):
        assert (idx[i] == pad).all(), (i, idx[i])
    assert list(idx[4]) == [10, 8, 9, 10, 11, 11, 11, 11, 11], idx[4]


def test_sort_two_identical_boxes():
    c = R.rect_corners(0.3, -0.2, 2.0, 1.0, 0.3)
    v, m = np.zeros((24, 2)), np.zeros(24, dtype=bool)
    v[0:4] = v[4:8] = c
    m[:8] = True
    idx = _sort_gpu(_centred(v, m)[None, None], m[None, None], np.array([[8]]))[0, 0]
    assert sorted(idx[:4]) == [0, 1, 2, 3] and idx[4] == idx[0] and (idx[5:] == 8).all(), idx
    assert abs(R.shoelace(v[idx[:4]]) - 2.0) <= 2e-5
    a = R.polar_angle(*(_centred(v, m)[idx[:4]].T))
    assert (np.diff(a) > 0).all()


def test_sort_vertex_on_the_x_axis_follows_the_angle():
    v, m = np.zeros((24, 2)), np.zeros(24, dtype=bool)
    pts = {5: (0.0, -1.0), 1: (-1.0, 0.0), 10: (1.0, 0.0), 3: (0.0, 1.0), 17: (0.5, -0.5), 6: (-0.5, 0.5)}
    for k, p in pts.items():
        v[k], m[k] = p, True
    idx = _sort_gpu(v[None, None], m[None, None], np.array([[6]]))[0, 0]
    # (1,0) angle 0; (0,1); (-.5,.5); (-1,0) angle pi; (0,-1); (.5,-.5)
    assert list(idx) == [10, 3, 6, 1, 5, 17, 10, 8, 8], idx


def test_sort_grid_not_a_multiple_of_the_workgroup():
    V, M, nv, _, _ = polygons()
    k = 3 * 101
    vc = np.stack([_centred(v, m) for v, m in zip(V[:k], M[:k])]).reshape(3, 101, 24, 2)
    m, n = M[:k].reshape(3, 101, 24), nv[:k].reshape(3, 101)
    idx = _sort_gpu(vc, m, n)
    assert np.array_equal(idx, R.sort_vertices_ref(vc.astype(np.float32), m, n))


# ---- 9. through the public classes -----------------------------------------------------------------------------------------------------------
def test_public_classes():
    rot = _rot()
    dims, C = (10, 12, 14), 16
    x0, rois, ref, keep, _, _, _ = case(dims, C, 0)
    x = to_nc(x0).cuda().requires_grad_(True)
    align = rot.ROIAlignRotated3D(POOLED, sampling_ratio=0)
    out = align(x, rois.cuda(), SCALE)
    assert out.shape == (64, C, *POOLED) and out.requires_grad
    out.sum().backward()
    xr = x0.double().requires_grad_(True)
    R.roi_align_ref(xr, rois, POOLED, SCALE, 0)[0].sum().backward()
    assert x.grad.shape == x.shape and x.grad.dtype == torch.float32
    assert relerr(x.grad.permute(0, 2, 3, 4, 1), xr.grad) < 1e-3
    # bf16 channels-last: the gradient comes back in the map's dtype
    xb = x0.bfloat16().cuda().requires_grad_(True)
    rot.roi_align_rotated_3d_channels_last(xb, rois.cuda(), POOLED, SCALE, 0).float().sum().backward()
    assert xb.grad.dtype == torch.bfloat16 and relerr(xb.grad, xr.grad) < 2.0 ** -7
    V, M, nv, _, _ = polygons()
    v = torch.from_numpy(V[:64].astype(np.float32)).reshape(1, 64, 24, 2).cuda().requires_grad_(True)
    idx = rot.sort_v(v, torch.from_numpy(M[:64]).reshape(1, 64, 24).cuda(), torch.from_numpy(nv[:64]).reshape(1, 64).cuda())
    assert idx.requires_grad is False and idx.dtype == torch.int32
