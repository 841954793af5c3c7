"""Float64 restatement of the RPN training path (nerf_mae_amd.rpn over csrc/rpn.hip): the anchor table and grid, the padding masks, the IoU
matching with the low-quality restore, both encodes, the sampler's count rule and the two losses, written from the stated semantics (the
header of csrc/rpn.hip).  tests/test_rpn_ref_cpu.py checks it against tests/golden/g20_rpn_targets.npz, recorded from the reference's own
Python by tools/gen_golden_rpn.py; the GPU tests are measured against it.

It also reports the decision margins that make exact comparisons of labels and indices defined:
  m_thr   every valid anchor's best IoU against both thresholds;
  m_gt    best against second-best box, over the anchors whose match is used (matched_idxs >= 0);
  m_anc   per box, the maximum over the valid anchors against the largest IoU below it (the low-quality restore takes the anchors AT the maximum);
  m_tol   the 0.1 tolerance of the midpoint-offset encode: | |corner - extreme| - 0.1 | over the corners of every oriented box.
A scene generator and a head generator (numpy PCG64 streams) are part of the restatement so that fixtures store seeds, not tensors."""
import itertools
import math

import numpy as np
import torch

F64 = torch.float64
ANCHOR_SIZES = ((8,), (16,), (32,), (64,))
ASPECT_RATIOS = (((1., 1., 1.), (1., 1., 2.), (1., 2., 2.), (1., 1., 3.), (1., 3., 3.)),) * 4
FG, BG = 0.35, 0.2
BATCH, FRACTION = 256, 0.5
# the g20 case
MESH = (32, 32, 32)
GRIDS = ((8, 8, 8), (4, 4, 4), (2, 2, 2), (1, 1, 1))
ORI = ((32, 32, 32), (24, 28, 20))
NBOX = (5, 3)
SEED = {False: 594, True: 4458}          # tools/gen_golden_rpn.py --search
HEAD_SEED = 7


# ---- anchors -------------------------------------------------------------------------------------------------------------------------------
def base_anchors(sizes=ANCHOR_SIZES, ratios=ASPECT_RATIOS):
    """per level [A, 6]: every distinct permutation of every ratio triple (in the iteration order of the set) times every size, halved, rounded
    half to even"""
    out = []
    for scales, level in zip(sizes, ratios):
        rows = []
        for ratio in level:
            for p in list(set(itertools.permutations(ratio))):
                for s in scales:
                    rows.append([-p[0] * s, -p[1] * s, -p[2] * s, p[0] * s, p[1] * s, p[2] * s])
        out.append(np.round(np.asarray(rows, dtype=np.float64) / 2))
    return out


def strides(mesh, grids):
    return [tuple(m // g for m, g in zip(mesh, grid)) for grid in grids]


def grid_index(grid, A):
    """(w, h, d, a) of every anchor of a level, anchor ((w H + h) D + d) A + a"""
    w, h, d, a = np.meshgrid(*[np.arange(v) for v in (*grid, A)], indexing="ij")
    return w.reshape(-1), h.reshape(-1), d.reshape(-1), a.reshape(-1)


def anchors(mesh=MESH, grids=GRIDS, base=None):
    base = base_anchors() if base is None else base
    out = []
    for grid, s, b in zip(grids, strides(mesh, grids), base):
        w, h, d, a = grid_index(grid, len(b))
        c = np.stack([w * s[0], h * s[1], d * s[2]], 1).astype(np.float64)
        out.append(np.concatenate([c, c], 1) + b[a])
    return np.concatenate(out, 0)


def valid_mask(ori, mesh=MESH, grids=GRIDS, base=None):
    base = base_anchors() if base is None else base
    out = []
    for grid, s, b in zip(grids, strides(mesh, grids), base):
        w, h, d, _ = grid_index(grid, len(b))
        lim = [math.ceil(o / t) for o, t in zip(ori, s)]
        out.append((w < lim[0]) & (h < lim[1]) & (d < lim[2]))
    return np.concatenate(out, 0)


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------------
def obb_to_aabb(b):
    cs, sn = np.cos(b[:, 6]), np.sin(b[:, 6])
    bx = np.abs(b[:, 3] / 2 * cs) + np.abs(b[:, 4] / 2 * sn)
    by = np.abs(b[:, 3] / 2 * sn) + np.abs(b[:, 4] / 2 * cs)
    bz = b[:, 5] / 2
    return np.stack([b[:, 0] - bx, b[:, 1] - by, b[:, 2] - bz, b[:, 0] + bx, b[:, 1] + by, b[:, 2] + bz], 1)


def iou_matrix(gt, anc):
    vol = lambda b: (b[:, 3] - b[:, 0]) * (b[:, 4] - b[:, 1]) * (b[:, 5] - b[:, 2])
    lt = np.maximum(gt[:, None, :3], anc[None, :, :3])
    rb = np.minimum(gt[:, None, 3:], anc[None, :, 3:])
    whd = np.clip(rb - lt, 0, None)
    inter = whd[..., 0] * whd[..., 1] * whd[..., 2]
    return inter / (vol(gt)[:, None] + vol(anc)[None, :] - inter)


def encode_aabb(gt, anc):
    e, g = anc[:, 3:] - anc[:, :3], gt[:, 3:] - gt[:, :3]
    return np.concatenate([((gt[:, :3] + 0.5 * g) - (anc[:, :3] + 0.5 * e)) / e, np.log(g / e)], 1)


def obb_corners_2d(b):
    """the four BEV corners in the order of the midpoint-offset encode"""
    x, y, w, h, cs, sn = b[:, 0], b[:, 1], b[:, 3], b[:, 4], np.cos(b[:, 6]), np.sin(b[:, 6])
    v1x, v1y, v2x, v2y = w / 2 * cs, -w / 2 * sn, -h / 2 * sn, -h / 2 * cs
    X = np.stack([x + v1x + v2x, x + v1x - v2x, x - v1x - v2x, x - v1x + v2x], 1)
    Y = np.stack([y + v1y + v2y, y + v1y - v2y, y - v1y - v2y, y - v1y + v2y], 1)
    return X, Y


def encode_obb(gt, anc):
    p = (anc[:, :3] + anc[:, 3:]) * 0.5
    e = anc[:, 3:] - anc[:, :3]
    hbb = obb_to_aabb(gt)
    gx, gy, gw, gh = (hbb[:, 0] + hbb[:, 3]) * 0.5, (hbb[:, 1] + hbb[:, 4]) * 0.5, hbb[:, 3] - hbb[:, 0], hbb[:, 4] - hbb[:, 1]
    X, Y = obb_corners_2d(gt)
    ga = np.where(np.abs(Y - Y.min(1, keepdims=True)) > 0.1, -1000.0, X).max(1)
    gb = np.where(np.abs(X - X.max(1, keepdims=True)) > 0.1, -1000.0, Y).max(1)
    return np.stack([(gx - p[:, 0]) / e[:, 0], (gy - p[:, 1]) / e[:, 1], (gt[:, 2] - p[:, 2]) / e[:, 2], np.log(gw / e[:, 0]), np.log(gh / e[:, 1]),
                     np.log(gt[:, 5] / e[:, 2]), (ga - gx) / gw, (gb - gy) / gh], 1)


def tolerance_margin(gt):
    X, Y = obb_corners_2d(gt)
    return float(min(np.abs(np.abs(Y - Y.min(1, keepdims=True)) - 0.1).min(), np.abs(np.abs(X - X.max(1, keepdims=True)) - 0.1).min()))


def make_scene(seed, nbox=NBOX, mesh=MESH, rotated=False, ori=None):
    """per scene [k, 6] or [k, 7] fp32 boxes inside the scene's original size; the first oriented box of a scene has theta 0"""
    rng = np.random.default_rng([seed, int(rotated)])
    out = []
    for i, k in enumerate(nbox):
        lim = np.asarray(mesh if ori is None else ori[i], dtype=np.float64)
        size = rng.uniform(0.15, 0.5, (k, 3)) * lim.min()
        ctr = size / 2 + rng.uniform(0, 1, (k, 3)) * (lim - size)
        if rotated:
            th = rng.uniform(-math.pi / 2, math.pi / 2, (k, 1))
            th[:1] = 0.0
            b = np.concatenate([ctr, size, th], 1)
        else:
            b = np.concatenate([ctr - size / 2, ctr + size / 2], 1)
        out.append(torch.from_numpy(b.astype(np.float32).reshape(k, 7 if rotated else 6)))
    return out


# ---- assignment ----------------------------------------------------------------------------------------------------------------------------
def assign(boxes, mesh=MESH, grids=GRIDS, ori=None, fg=FG, bg=BG, rotated=False, base=None):
    """boxes: per scene [k, 6|7]; ori: per scene original sizes or None -> dict of labels [N, n] f64, matched [N, n] int64, targets [N, n, 6|8] f64,
    valid [N, n] bool, restored [N, n] bool (label 1 only through the restore), the margins m_* and gtmax per scene"""
    anc = anchors(mesh, grids, base)
    n, C = anc.shape[0], 8 if rotated else 6
    res = dict(labels=[], matched=[], targets=[], valid=[], restored=[], gtmax=[], m_thr=math.inf, m_gt=math.inf, m_anc=math.inf, m_tol=math.inf)
    for i, b in enumerate(boxes):
        b = np.asarray(b, dtype=np.float64).reshape(-1, 7 if rotated else 6)
        valid = np.ones(n, dtype=bool) if ori is None else valid_mask(ori[i], mesh, grids, base)
        labels, matched, targets, restored = np.where(valid, 0.0, -1.0), np.full(n, -1, dtype=np.int64), np.zeros((n, C)), np.zeros(n, dtype=bool)
        if b.shape[0]:
            q = iou_matrix(obb_to_aabb(b) if rotated else b, anc)
            q[:, ~valid] = -1.0
            best, arg = q.max(0), q.argmax(0)                      # argmax: the first of equal values
            m = np.where(best >= fg, arg, np.where(best < bg, -1, -2))
            gtmax = q.max(1)
            at_max = ((q == gtmax[:, None]) & valid[None, :]).any(0)
            restored = at_max & (m < 0)
            m = np.where(at_max, arg, m)
            m = np.where(valid, m, -1)
            labels = np.where(valid, np.where(m >= 0, 1.0, np.where(m == -1, 0.0, -1.0)), -1.0)
            matched = m
            g = b[np.clip(m, 0, None)]
            targets = encode_obb(g, anc) if rotated else encode_aabb(g, anc)
            res["gtmax"].append(gtmax)
            res["m_thr"] = min(res["m_thr"], float(np.minimum(np.abs(best[valid] - fg), np.abs(best[valid] - bg)).min()))
            if b.shape[0] > 1 and (m >= 0).any():
                qp = q[:, m >= 0]                                      # exactly equal boxes tie exactly: the lowest index, by definition
                res["m_gt"] = min(res["m_gt"], float((qp.max(0) - np.where(qp < qp.max(0)[None, :], qp, -1.0).max(0)).min()))
            below = np.where(q < gtmax[:, None], q, -1.0).max(1)       # anchors AT the maximum tie exactly (same shape, box inside both): all restored
            res["m_anc"] = min(res["m_anc"], float((gtmax - below).min()))
            if rotated:
                res["m_tol"] = min(res["m_tol"], tolerance_margin(b))
        else:
            res["gtmax"].append(np.zeros(0))
        for k, v in (("labels", labels), ("matched", matched), ("targets", targets), ("valid", valid), ("restored", restored)):
            res[k].append(torch.from_numpy(np.ascontiguousarray(v)))
    for k in ("labels", "matched", "targets", "valid", "restored"):
        res[k] = torch.stack(res[k])
    return res


def decision_margins(a):
    return {k: a[k] for k in ("m_thr", "m_gt", "m_anc", "m_tol") if a[k] < math.inf}


# ---- sampling ------------------------------------------------------------------------------------------------------------------------------
def sample_counts(labels, batch=BATCH, fraction=FRACTION):
    """labels [N, n] -> [(num_pos, num_neg)] per scene"""
    out = []
    for row in labels:
        npos, nneg = int((row >= 1).sum()), int((row == 0).sum())
        p = min(npos, int(batch * fraction))
        out.append((p, min(nneg, batch - p)))
    return out


def make_flags(seed, labels, batch=BATCH, fraction=FRACTION):
    """a recorded sampled set: per scene the count rule's numbers of positives and negatives, drawn by a numpy stream -> uint8 [N, n]"""
    rng = np.random.default_rng(seed)
    flags = torch.zeros(labels.shape, dtype=torch.uint8)
    for i, (row, (p, q)) in enumerate(zip(labels, sample_counts(labels, batch, fraction))):
        pos, neg = torch.nonzero(row >= 1)[:, 0].numpy(), torch.nonzero(row == 0)[:, 0].numpy()
        flags[i, torch.from_numpy(rng.permutation(pos)[:p])] = 1
        flags[i, torch.from_numpy(rng.permutation(neg)[:q])] = 2
    return flags


# ---- heads and losses ----------------------------------------------------------------------------------------------------------------------
def make_heads(seed, N, C, grids=GRIDS, A=None):
    """per level objectness (N, A, W, H, D) and regression (N, A C, W, H, D), fp32, from a numpy stream"""
    A = [len(b) for b in base_anchors()] if A is None else A
    rng = np.random.default_rng(seed)
    obj = [torch.from_numpy(rng.normal(0, 2.0, (N, a, *g)).astype(np.float32)) for g, a in zip(grids, A)]
    reg = [torch.from_numpy(rng.normal(0, 0.5, (N, a * C, *g)).astype(np.float32)) for g, a in zip(grids, A)]
    return obj, reg


def flatten_heads(obj, reg, C):
    """per-level head tensors -> ([N, n], [N, n, C]) in anchor order (levels concatenated, ((w H + h) D + d) A + a)"""
    N = obj[0].shape[0]
    o = torch.cat([t.permute(0, 2, 3, 4, 1).reshape(N, -1) for t in obj], 1)
    r = torch.cat([t.reshape(N, -1, C, *t.shape[2:]).permute(0, 3, 4, 5, 1, 2).reshape(N, -1, C) for t in reg], 1)
    return o, r


def smooth_l1(d, beta=1.0 / 9.0):
    a = d.abs()
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta)


def losses(obj, reg, flags, targets):
    """float64 per-level heads (requires_grad for gradients), flags [N, n] uint8, targets [N, n, C] -> (loss_objectness, loss_rpn_box_reg)"""
    C = targets.shape[-1]
    o, r = flatten_heads(obj, reg, C)
    sampled, pos = flags != 0, flags == 1
    x, y = o[sampled], pos[sampled].to(o.dtype)
    bce = (x.clamp(min=0) - x * y + torch.log1p(torch.exp(-x.abs()))).sum()
    count = int(sampled.sum())
    return bce / count, smooth_l1(r[pos] - targets[pos].to(r.dtype)).sum() / count
