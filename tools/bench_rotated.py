"""Rotated 3-D RoIAlign and vertex sort: HIP-event times at the downstream shape (C = 256, map 40^3, B = 2, pooled 7^3, sampling ratio 0,
512 ROIs of 4-30 voxels) in both layouts, the sort at [8, 1024, 24], and the oriented-box IoU / GIoU / DIoU losses, all-pairs IoU and NMS
(second half of this file) next to their composition from framework ops around sort_v, and last the FCOS inference post-processing
(tools/bench_fcos_post.py, which also runs on its own).   python tools/bench_rotated.py [reps]

Printed per kernel: microseconds (median and minimum of `reps` >= 50 timed launches after 5 warm-up launches) and, for the channels-last
kernels, effective bytes/s: forward = (8 corner rows x C x element size x contributing samples + output bytes) / time, most of it served
from cache (the two maps are 131 MB in fp32); backward = bytes added by fp32 atomics (4 x C per corner with a non-zero weight) / time, to be read
against the ~1.3 TB/s chip-wide rate of global float atomics.  The sample and corner counts are computed on the host in float64 from the
same ROIs (a sample within rounding of a boundary may be counted differently from the kernel: parts in 1e5 at most)."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from nerf_mae_amd import ops

REPS = max(50, int(sys.argv[1])) if len(sys.argv) > 1 else 50
DIMS, C, POOLED, N, B = (40, 40, 40), 256, (7, 7, 7), 512, 2
assert torch.cuda.is_available(), "bench_rotated.py needs an MI355X"


def timed(fn, reps=REPS, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(us), min(us)


def count_work(rois, dims, pooled):
    """-> (contributing samples, corners with a non-zero weight) summed over all bins; float64, sampling ratio 0, scale 1"""
    samples = corners = 0
    for q in rois.astype(np.float64):
        size = np.maximum(q[4:7], 1.0)
        ax = []
        for a in range(3):
            g = int(np.ceil(size[a] / pooled[a]))
            ax.append((-size[a] / 2 + (np.arange(pooled[a])[:, None] + (np.arange(g)[None, :] + 0.5) / g) * size[a] / pooled[a]).ravel())
        th = q[7] * np.pi / 180
        x = ax[0][:, None] * np.cos(th) + ax[1][None, :] * np.sin(th) + q[1]
        y = ax[1][None, :] * np.cos(th) - ax[0][:, None] * np.sin(th) + q[2]
        z = ax[2] + q[3]

        def axis(v, ext):
            ok = (v >= -1) & (v <= ext)
            vc = np.maximum(v, 0)
            lo = np.floor(vc)
            two = (lo < ext - 1) & (vc != lo)          # both corners carry weight
            return ok, 1 + two
        okx, kx = axis(x, dims[0])
        oky, ky = axis(y, dims[1])
        okz, kz = axis(z, dims[2])
        oxy = okx & oky
        samples += int(oxy.sum()) * int(okz.sum())
        corners += int((kx * ky * oxy).sum()) * int((kz * okz).sum())
    return samples, corners


r = np.random.default_rng(7)
rois_h = np.concatenate([(np.arange(N) % B)[:, None], r.uniform(0, 40, (N, 3)), r.uniform(4, 30, (N, 3)), r.uniform(-180, 180, (N, 1))], 1).astype(np.float32)
samples, corners = count_work(rois_h, DIMS, POOLED)
rois = torch.from_numpy(rois_h).cuda()
nbins = N * POOLED[0] * POOLED[1] * POOLED[2]
print(f"shape: map {DIMS} x C{C} x B{B}, pooled {POOLED}, {N} ROIs, {nbins} bins, {samples} contributing samples, {corners} weighted corners; {REPS} reps")
torch.manual_seed(0)
x32 = torch.randn((B, *DIMS, C), device="cuda")
for name, x in (("fp32", x32), ("bf16", x32.bfloat16())):
    es = x.element_size()
    out = ops.roi_align_rotated_3d_fwd(x, rois, POOLED, 1.0, 0, ops.ROI_CHANNELS_LAST)
    med, best = timed(lambda: ops.lib().call("nmh_roi_align_rotated_3d_fwd", 0, ops.dt_of(x), x, rois, out, N, B, *DIMS, C, *POOLED, 1.0, 0, ops._st()))
    nbytes = 8 * C * es * samples + out.numel() * es
    print(f"channels-last {name} forward : median {med:9.1f} us  min {best:9.1f} us  {nbytes / med / 1e6:7.2f} TB/s effective ({nbytes / 1e9:.2f} GB of corner rows + output)")
    dout = torch.randn_like(out)
    dx = torch.zeros(x.shape, dtype=torch.float32, device="cuda")
    med, best = timed(lambda: ops.lib().call("nmh_roi_align_rotated_3d_bwd", 0, ops.dt_of(dout), dout, rois, dx, N, B, *DIMS, C, *POOLED, 1.0, 0, ops._st()))
    nbytes = 4 * C * corners
    print(f"channels-last {name} backward: median {med:9.1f} us  min {best:9.1f} us  {nbytes / med / 1e6:7.2f} TB/s of atomic-added bytes ({nbytes / 1e9:.2f} GB)")
    del out, dout, dx
xn = x32.permute(0, 4, 1, 2, 3).contiguous()
del x32
out = ops.roi_align_rotated_3d_fwd(xn, rois, POOLED, 1.0, 0, ops.ROI_NCWLH)
med, best = timed(lambda: ops.lib().call("nmh_roi_align_rotated_3d_fwd", 1, 0, xn, rois, out, N, B, *DIMS, C, *POOLED, 1.0, 0, ops._st()))
print(f"NCWLH fp32 forward         : median {med:9.1f} us  min {best:9.1f} us")
dout = torch.randn_like(out)
dx = torch.zeros_like(xn)
med, best = timed(lambda: ops.lib().call("nmh_roi_align_rotated_3d_bwd", 1, 0, dout, rois, dx, N, B, *DIMS, C, *POOLED, 1.0, 0, ops._st()))
print(f"NCWLH fp32 backward        : median {med:9.1f} us  min {best:9.1f} us")
del xn, out, dout, dx

v = torch.rand((8, 1024, 24, 2), device="cuda")
m = torch.rand((8, 1024, 24), device="cuda") > 0.8
m[..., 8] = False
nv = m.sum(-1).clamp(max=8).int()
v = (v - (v * m[..., None]).sum(2, keepdim=True) / m.sum(-1).clamp(min=1)[..., None, None]).contiguous()
idx = ops.sort_vertices(v, m, nv)
med, best = timed(lambda: ops.lib().call("nmh_sort_vertices", v, m, nv, idx, 8, 1024, 24, ops._st()), reps=max(REPS, 200))
print(f"sort_vertices [8,1024,24]  : median {med:9.1f} us  min {best:9.1f} us")
del v, m, nv, idx


# ---- oriented-box IoU / GIoU / DIoU, all-pairs IoU, NMS: the fused ops next to the only other way to compute them with this project -------
# The composition: the same quantities from framework ops around our sort_v (24 candidate vertices per pair, masked, sorted by the HIP
# vertex sort, shoelace; the 24-candidate enclosing rectangle by gathers and reductions), differentiated by autograd.  It lives here, not in
# the product.  Same protocol as above: HIP events, median of `reps` after 5 warm-ups.
from nerf_mae_amd import rotated, rotated_iou  # noqa: E402
from tests._obb_iou_ref import LINES, make_boxes, make_clusters  # noqa: E402

_SX = torch.tensor([0.5, -0.5, -0.5, 0.5], device="cuda")
_SY = torch.tensor([0.5, 0.5, -0.5, -0.5], device="cuda")
_LI = torch.tensor([i for i, _ in LINES], device="cuda")
_LJ = torch.tensor([j for _, j in LINES], device="cuda")


def comp_corners(b):
    c, s = torch.cos(b[..., 6:7]), torch.sin(b[..., 6:7])
    lx, ly = _SX * b[..., 3:4], _SY * b[..., 4:5]
    return torch.stack([b[..., 0:1] + lx * c - ly * s, b[..., 1:2] + lx * s + ly * c], -1)          # (B,N,4,2)


def comp_inside(c1, c2):
    a, ab, ad = c2[..., 0:1, :], c2[..., 1:2, :] - c2[..., 0:1, :], c2[..., 3:4, :] - c2[..., 0:1, :]
    am = c1 - a
    u, v = (ab * am).sum(-1) / (ab * ab).sum(-1), (ad * am).sum(-1) / (ad * ad).sum(-1)
    return (u > -1e-6) & (u < 1 + 1e-6) & (v > -1e-6) & (v < 1 + 1e-6)


def comp_inter2d(c1, c2):
    p, r = c1[..., :, None, :], (torch.roll(c1, -1, -2) - c1)[..., :, None, :]                         # (B,N,4,1,2)
    q, s = c2[..., None, :, :], (torch.roll(c2, -1, -2) - c2)[..., None, :, :]
    den = r[..., 0] * s[..., 1] - r[..., 1] * s[..., 0]
    safe = torch.where(den == 0, torch.ones_like(den), den)
    t = ((q[..., 0] - p[..., 0]) * s[..., 1] - (q[..., 1] - p[..., 1]) * s[..., 0]) / safe
    u = ((q[..., 0] - p[..., 0]) * r[..., 1] - (q[..., 1] - p[..., 1]) * r[..., 0]) / safe
    hit = (den != 0) & (t > 0) & (t < 1) & (u > 0) & (u < 1)
    pts = (p + t[..., None] * r) * hit[..., None]
    B, N = c1.shape[:2]
    verts = torch.cat([c1, c2, pts.reshape(B, N, 16, 2)], 2)
    mask = torch.cat([comp_inside(c1, c2), comp_inside(c2, c1), hit.reshape(B, N, 16)], 2)
    nv = mask.sum(-1).int()
    mean = (verts * mask[..., None]).sum(2, keepdim=True) / nv.clamp(min=1)[..., None, None]
    idx = rotated.sort_v((verts - mean).detach().contiguous(), mask, nv).long()
    sel = torch.gather(verts, 2, idx[..., None].expand(-1, -1, -1, 2))
    return (sel[..., :-1, 0] * sel[..., 1:, 1] - sel[..., :-1, 1] * sel[..., 1:, 0]).sum(-1).abs() / 2


def comp_smallest(c8):
    d = c8[..., _LJ, :] - c8[..., _LI, :]
    e = d / d.norm(dim=-1, keepdim=True).clamp(min=1e-12)
    along = e[..., 0:1] * c8[..., None, :, 0] + e[..., 1:2] * c8[..., None, :, 1]
    across = e[..., 0:1] * c8[..., None, :, 1] - e[..., 1:2] * c8[..., None, :, 0]
    proj, dist = along.amax(-1) - along.amin(-1), across.amax(-1) - across.amin(-1)
    area = proj * dist
    k = torch.where(area == 0, torch.full_like(area, 1e30), area).argmin(-1, keepdim=True)
    return proj.gather(-1, k).squeeze(-1), dist.gather(-1, k).squeeze(-1)


def comp_iou3d(b1, b2, kind="iou"):
    c1, c2 = comp_corners(b1), comp_corners(b2)
    zx1, zn1, zx2, zn2 = b1[..., 2] + b1[..., 5] / 2, b1[..., 2] - b1[..., 5] / 2, b2[..., 2] + b2[..., 5] / 2, b2[..., 2] - b2[..., 5] / 2
    i3 = comp_inter2d(c1, c2) * (torch.minimum(zx1, zx2) - torch.maximum(zn1, zn2)).clamp(min=0)
    u3 = b1[..., 3] * b1[..., 4] * b1[..., 5] + b2[..., 3] * b2[..., 4] * b2[..., 5] - i3
    iou = i3 / u3
    if kind == "iou":
        return iou
    zr = torch.maximum(zx1, zx2) - torch.minimum(zn1, zn2)
    w, h = comp_smallest(torch.cat([c1, c2], -2))
    if kind == "giou":
        return 1 - iou + (zr * w * h - u3) / (zr * w * h)
    return 1 - iou + ((b1[..., :3] - b2[..., :3]) ** 2).sum(-1) / (w * w + h * h + zr * zr)


def comp_nms(boxes, scores, thr):
    keep, idxs = [], scores.argsort(descending=True)
    while idxs.numel() > 0:
        i = idxs[0]
        keep.append(i)
        if idxs.numel() == 1:
            break
        rest = boxes[idxs[1:]]
        iou = comp_iou3d(boxes[i].expand_as(rest)[None], rest[None])[0]
        idxs = idxs[1:][iou <= thr]
    return torch.stack(keep)


rng = np.random.default_rng(17)
P = 8192
b1 = torch.from_numpy(make_boxes(rng, P))[None].cuda().requires_grad_(True)
b2 = torch.from_numpy(make_boxes(rng, P))[None].cuda()
fused = dict(iou=lambda: rotated_iou.cal_iou_3d(b1, b2), giou=lambda: rotated_iou.cal_giou_3d(b1, b2)[0], diou=lambda: rotated_iou.cal_diou_3d(b1, b2)[0])
print(f"oriented-box losses, forward + backward (gradient to box 1), (1, {P}) pairs:")
for kind in ("iou", "giou", "diou"):
    def run(f):
        b1.grad = None
        f().sum().backward()
    mf, bf = timed(lambda: run(fused[kind]))
    mc, bc = timed(lambda: run(lambda: comp_iou3d(b1, b2, kind)))
    err = (fused[kind]() - comp_iou3d(b1, b2, kind)).abs().max().item()
    print(f"  {kind:5s}: fused median {mf:9.1f} us  min {bf:9.1f} us | composition around sort_v median {mc:9.1f} us  min {bc:9.1f} us | max |difference| {err:.1e}")

NB = 2500
bb, sc = make_clusters(47, NB)
bb, sc = bb.cuda(), sc.cuda()
mf, bf = timed(lambda: rotated_iou.box_iou_3d(bb, bb))
rows = 16      # the reference's own batching of the repeat ("to avoid OOM")
with torch.no_grad():
    comp_pw = lambda: torch.cat([comp_iou3d(bb[i:i + rows, None, :].expand(-1, NB, -1), bb[None].expand(min(rows, NB - i), -1, -1)) for i in range(0, NB, rows)])   # noqa: E731
    mc, bc = timed(comp_pw, reps=5, warm=1)
    diff = (rotated_iou.box_iou_3d(bb, bb) - comp_pw()).abs()
    err_diag = diff.diagonal().max().item()      # a box against itself: the vertex method's weak spot (deviations)
    err = diff.fill_diagonal_(0).max().item()
print(f"box_iou_3d {NB} x {NB}: fused median {mf:9.1f} us  min {bf:9.1f} us | composition, 16 rows at a time (5 reps) median {mc:9.1f} us  min {bc:9.1f} us | "
      f"max |difference| off the diagonal {err:.1e}, on it {err_diag:.1e}")
mf, bf = timed(lambda: rotated_iou.nms(bb, sc, 0.1))
with torch.no_grad():
    mc, bc = timed(lambda: comp_nms(bb, sc, 0.1), reps=5, warm=1)
    kf, kc = rotated_iou.nms(bb, sc, 0.1), comp_nms(bb, sc, 0.1)
print(f"nms N = {NB}, threshold 0.1 ({kf.numel()} kept): fused median {mf:9.1f} us  min {bf:9.1f} us | host loop over the composition (5 reps) median {mc:9.1f} us  min {bc:9.1f} us | same result: {torch.equal(kf, kc)}")

# ---- FCOS inference post-processing: the fused op, its dense form eager and replayed from a graph, and a composition of the reference's steps ----
import bench_fcos_post  # noqa: E402

bench_fcos_post.main(REPS)
