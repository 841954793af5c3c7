"""Float64 restatements of the rotated 3-D RoIAlign and the polygon vertex sort, written from the semantics stated in
nerf-mae_amd/csrc/rotated.hip (plain NumPy / PyTorch, CPU): the yardstick of tests/test_rotated_ops_gpu.py.  The RoIAlign one is
differentiable with respect to the map, so its backward is autograd's.  tests/test_rotated_ops_cpu.py checks it against analytic results."""
import math

import numpy as np
import torch


# ---- rotated RoIAlign -----------------------------------------------------------------------------------------------------------------
def make_rois(seed, n, dims, scale, nbatch=2):
    """centre uniform in [-1, extent + 1] / scale per axis, size uniform in [0.6, 0.6 max extent] / scale, angle uniform in +-180 degrees,
    batch index alternating; fp32 [n, 8]"""
    r = np.random.default_rng(seed)
    c = np.stack([r.uniform(-1, d + 1, n) for d in dims], 1) / scale
    s = r.uniform(0.6, 0.6 * max(dims), (n, 3)) / scale
    th = r.uniform(-180, 180, (n, 1))
    b = (np.arange(n) % nbatch)[:, None].astype(np.float64)
    return torch.from_numpy(np.concatenate([b, c, s, th], 1).astype(np.float32))


def _geometry(roi, pooled, scale, sr):
    """roi: 8 float64 numbers -> centre[3], per-axis ROI-local sample coordinates [(P, g)], distance of size / pooled to an integer"""
    c = [roi[1 + a] * scale for a in range(3)]
    s = [max(roi[4 + a] * scale, 1.0) for a in range(3)]
    loc, gdist = [], math.inf
    for a in range(3):
        P = pooled[a]
        if sr > 0:
            g = sr
        else:
            v = s[a] / P
            g = int(math.ceil(v))
            gdist = min(gdist, abs(v - round(v)))
        i = torch.arange(g, dtype=torch.float64)[None, :]
        p = torch.arange(P, dtype=torch.float64)[:, None]
        loc.append(-s[a] / 2.0 + p * (s[a] / P) + (i + 0.5) * (s[a] / P) / g)
    return c, loc, gdist


def _axis(v, ext):
    valid = (v >= -1.0) & (v <= ext)
    vc = v.clamp(min=0.0)
    lo = vc.floor().long()
    top = lo >= ext - 1
    lo = torch.where(top, torch.full_like(lo, ext - 1), lo).clamp(0, ext - 1)
    hi = torch.where(top, lo, lo + 1).clamp(0, ext - 1)
    frac = torch.where(top, torch.zeros_like(vc), vc - lo.double())
    near = torch.minimum((v + 1.0).abs(), (v - ext).abs())
    return valid, lo, hi, frac, near


def _roi_bins(xb, roi, pooled, scale, sr, only=None):
    """xb (W,L,H,C) float64 -> (bins (Pw,Pl,Ph,C), per-bin distance of the nearest sample coordinate to -1 / extent, size/pooled distance to
    an integer, samples, samples contributing 0).  only = (pw, pl, ph): that one bin, as shape (1,1,1,C)."""
    W, L, H, C = xb.shape
    c, loc, gdist = _geometry(roi, pooled, scale, sr)
    if only is not None:
        loc = [loc[a][only[a]:only[a] + 1] for a in range(3)]
    P = [t.shape[0] for t in loc]
    g = [t.shape[1] for t in loc]
    th = roi[7] * math.pi / 180.0
    cs, sn = math.cos(th), math.sin(th)
    xx, yy, zz = (t.reshape(-1) for t in loc)
    X = xx[:, None] * cs + yy[None, :] * sn + c[0]
    Y = yy[None, :] * cs - xx[:, None] * sn + c[1]
    Z = zz + c[2]
    vx, x0, x1, fx, nx = _axis(X, W)
    vy, y0, y1, fy, ny = _axis(Y, L)
    vz, z0, z1, fz, nz = _axis(Z, H)
    valid = ((vx & vy)[:, :, None] & vz[None, None, :]).double()
    acc = 0.0
    for xi, wx in ((x0, 1.0 - fx), (x1, fx)):
        for yi, wy in ((y0, 1.0 - fy), (y1, fy)):
            for zi, wz in ((z0, 1.0 - fz), (z1, fz)):
                w = (wx * wy)[:, :, None] * wz[None, None, :] * valid
                acc = acc + w[..., None] * xb[xi[:, :, None], yi[:, :, None], zi[None, None, :]]
    bins = acc.reshape(P[0], g[0], P[1], g[1], P[2], g[2], C).mean(dim=(1, 3, 5))
    nxy = torch.minimum(nx, ny).reshape(P[0], g[0], P[1], g[1]).amin(dim=(1, 3))
    nz = nz.reshape(P[2], g[2]).amin(dim=1)
    near = torch.minimum(nxy[:, :, None], nz[None, None, :])
    return bins, near, gdist, valid.numel(), int(valid.numel() - valid.sum().item())


def roi_align_ref(x, rois, pooled, scale, sr):
    """x (B,W,L,H,C) float64 channels-last, rois [N,8] -> out (N,Pw,Pl,Ph,C) float64 and a dict: `margin` (N,Pw,Pl,Ph) distance of each
    bin to a discontinuity of the op (a sample coordinate at -1 or extent; with sr == 0 also size / pooled at an integer, which counts for
    every bin of the ROI), `outside` fraction of samples that contribute 0 (ROIs with a valid batch index only)."""
    B = x.shape[0]
    R = rois.double().tolist()
    outs, margins, tot, out0 = [], [], 0, 0
    for roi in R:
        if not (0 <= roi[0] < B):
            outs.append(torch.zeros((*pooled, x.shape[-1]), dtype=torch.float64))
            margins.append(torch.full(tuple(pooled), math.inf, dtype=torch.float64))
            continue
        bins, near, gdist, n, n0 = _roi_bins(x[int(roi[0])], roi, pooled, scale, sr)
        outs.append(bins)
        margins.append(near.clamp(max=gdist))
        tot += n
        out0 += n0
    if not outs:
        return torch.zeros((0, *pooled, x.shape[-1]), dtype=torch.float64), dict(margin=torch.zeros((0, *pooled)), outside=0.0)
    return torch.stack(outs), dict(margin=torch.stack(margins), outside=out0 / max(tot, 1))


def roi_align_ref_bins(x, rois, pooled, scale, sr, which):
    """the bins which = [(n, pw, pl, ph), ...] only -> (len(which), C) float64 and their margins"""
    R = rois.double().tolist()
    vals, margins = [], []
    for n, pw, pl, ph in which:
        bins, near, gdist, _, _ = _roi_bins(x[int(R[n][0])], R[n], pooled, scale, sr, only=(pw, pl, ph))
        vals.append(bins.reshape(-1))
        margins.append(min(near.item(), gdist))
    return torch.stack(vals), torch.tensor(margins, dtype=torch.float64)


# ---- polygon vertex sort --------------------------------------------------------------------------------------------------------------
def polar_angle(x, y):
    """angle over [0, 2 pi); y == 0: x > 0 is 0, x < 0 is pi"""
    a = np.arctan2(y, x)
    return np.where(a < 0, a + 2 * np.pi, a)


def sort_vertices_ref(vertices, mask, num_valid):
    """vertices [B,N,M,2], mask [B,N,M] bool, num_valid [B,N] (NumPy) -> idx [B,N,9] int32, for polygons whose valid vertices all have
    different angles (any correct angular sort then has one answer)"""
    B, N, M, _ = vertices.shape
    out = np.zeros((B, N, 9), dtype=np.int32)
    for b in range(B):
        for n in range(N):
            m = mask[b, n]
            pad = next(j for j in range(8, M) if not m[j])
            nv = int(num_valid[b, n])
            out[b, n, :] = pad
            if nv < 3:
                continue
            ks = np.nonzero(m)[0]
            v = vertices[b, n, ks].astype(np.float64)
            order = ks[np.argsort(polar_angle(v[:, 0], v[:, 1]), kind="stable")][:nv]
            out[b, n, :nv] = order
            out[b, n, nv] = order[0]
    return out


def rect_corners(cx, cy, w, h, ang):
    """corners of a rotated rectangle, counter-clockwise, float64 (4, 2)"""
    d = np.array([[0.5, 0.5], [-0.5, 0.5], [-0.5, -0.5], [0.5, -0.5]]) * np.array([w, h])
    c, s = math.cos(ang), math.sin(ang)
    return d @ np.array([[c, s], [-s, c]]) + np.array([cx, cy])


def _inside(q, box, eps=0.0):
    """q inside the convex counter-clockwise polygon `box` (on the boundary counts when eps >= 0)"""
    e = np.roll(box, -1, axis=0) - box
    r = q[None, :] - box
    return bool(np.all(e[:, 0] * r[:, 1] - e[:, 1] * r[:, 0] >= -eps))


def box_pair_vertices(c1, c2):
    """The 24 candidate vertices of the intersection of two rectangles in the layout of the oriented-box IoU: corners of box 1 (0-3) with
    mask "inside box 2", corners of box 2 (4-7) with mask "inside box 1", then the 16 edge x edge intersections (8 + 4 i + j: edge i of
    box 1 with edge j of box 2; unmasked ones are 0).  float64."""
    v = np.zeros((24, 2))
    m = np.zeros(24, dtype=bool)
    v[0:4], v[4:8] = c1, c2
    for i in range(4):
        m[i] = _inside(c1[i], c2)
        m[4 + i] = _inside(c2[i], c1)
    for i in range(4):
        p, r = c1[i], c1[(i + 1) % 4] - c1[i]
        for j in range(4):
            q, s = c2[j], c2[(j + 1) % 4] - c2[j]
            den = r[0] * s[1] - r[1] * s[0]
            if den == 0.0:
                continue
            t = ((q[0] - p[0]) * s[1] - (q[1] - p[1]) * s[0]) / den
            u = ((q[0] - p[0]) * r[1] - (q[1] - p[1]) * r[0]) / den
            if 0.0 < t < 1.0 and 0.0 < u < 1.0:
                v[8 + 4 * i + j] = p + t * r
                m[8 + 4 * i + j] = True
    return v, m


def clip_area(subject, clip):
    """area of (subject polygon) intersected with (convex counter-clockwise clip polygon): Sutherland-Hodgman, float64"""
    poly = [tuple(p) for p in subject]
    for i in range(len(clip)):
        a, b = clip[i], clip[(i + 1) % len(clip)]
        side = lambda p: (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])   # noqa: E731
        nxt = []
        for k in range(len(poly)):
            p, q = poly[k], poly[(k + 1) % len(poly)]
            sp, sq = side(p), side(q)
            if sp >= 0:
                nxt.append(p)
            if (sp >= 0) != (sq >= 0):
                t = sp / (sp - sq)
                nxt.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
        poly = nxt
        if not poly:
            return 0.0
    return shoelace(np.array(poly))


def shoelace(p):
    """area of the closed polygon through the points p (K, 2) in order"""
    x, y = p[:, 0], p[:, 1]
    return 0.5 * abs(float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)))
