"""Rotated 3-D RoIAlign and vertex sort: HIP-event times at the downstream shape (C = 256, map 40^3, B = 2, pooled 7^3, sampling ratio 0,
512 ROIs of 4-30 voxels) in both layouts, and the sort at [8, 1024, 24].   python tools/bench_rotated.py [reps]

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
