"""Float64 restatement of the RoI stage (nerf_mae_amd/detector.py over csrc/roi_head.hip), written from the semantics in that file's header, and the seeded
inputs of its tests.  Checked against the recorded reference (tests/golden/g22_roi_head.npz, tools/gen_golden_roi_head.py) in tests/test_roi_head_ref_cpu.py.

The matching, pooling and loss functions take the kept indices; the sampler that draws them is restated on its own, exactly, in Python integers (sample).
Next to its results each function returns the smallest margin of its discrete decisions,
so that a test can assert that fp32 arithmetic cannot flip one: IoU against the two thresholds ("iou_fg", "iou_bg"), top-two IoU gap per RoI ("iou_top2"),
distance of every floored or ceiled quantity from an integer ("floor"; quantities that are integers exactly, such as the points of an integer-placed RoI with
theta = 0, are exact in fp32 as well and do not count), top-two gap inside each pooling cell ("cell_gap", the padding zero included), the level mapper's floor
("level").  "inside": every oriented sampling point lies in its map and every axis-aligned crop is unclamped.  At realistic sizes (thousands of proposals)
no scene keeps 1e-3 on every row, so targets also returns the three IoU margins per row (margins["rows"]): a row is decided if all three are at least MARGIN, and
targets(alt_arg / alt_label) gives the other outcome that a near-tie allows on the rows that are not."""
import math

import numpy as np
import torch

from tests._obb_iou_ref import pairwise

F64 = torch.float64
MARGIN = 1e-3
MESH = (32, 32, 32)
SCALES = (2, 4, 8)
ENLARGE = 0.2
FG, BG = 0.5, 0.2
BETA = 1.0 / 9.0
XFORM_CLIP = math.log(2000.0)
FEATURE_SCALE = 8.0
GOLD = dict(N=2, C=4, K=8, G=3, R=6, out=(2, 2, 2), max_res=32)          # the recorded runs: K RoIs and G boxes per scene, R sampled rows
GOLD_SEED = {False: (0, 0), True: (7, 0)}                                # (scene seed, map seed): tools/gen_golden_roi_head.py --search


def _frac_margin(v):
    """smallest distance from an integer over the entries of v that are not integers"""
    v = v.reshape(-1)
    d = (v - v.round()).abs()
    d = d[d > 0]
    return float(d.min()) if d.numel() else float("inf")


# ---- inputs --------------------------------------------------------------------------------------------------------------------------------
def make_maps(seed, C, N=2, dims=None):
    """one fp32 (N, C, W, H, D) map per level, values of both signs"""
    g = torch.Generator().manual_seed(1000 + seed)
    dims = dims or [tuple(m // s for m in MESH) for s in SCALES]
    return [torch.randn((N, C, *d), generator=g, dtype=torch.float32) * FEATURE_SCALE for d in dims]


def make_scene(seed, rotated, N=2, K=24, G=4):
    """-> (rois: per scene [K, 1+6|7] fp32 with the level in column 0, gt_boxes: per scene [G, 6|7], gt_labels: per scene [G]); the first RoIs are jittered
    copies of the boxes (foreground), the rest are spread over the mesh; levels cycle"""
    g = torch.Generator().manual_seed(seed)
    u = lambda *s: torch.rand(*s, generator=g, dtype=F64)
    rois, gts, labs = [], [], []
    for _ in range(N):
        c, s = 11 + 10 * u(G, 3), 5 + 6 * u(G, 3)
        th = (u(G, 1) - 0.5) * 2.6
        jc, js = c.repeat(K, 1)[:K] + (u(K, 3) - 0.5) * 2.0, s.repeat(K, 1)[:K] * (0.85 + 0.3 * u(K, 3))
        jt = th.repeat(K, 1)[:K] + (u(K, 1) - 0.5) * 0.3
        far = torch.arange(K) >= K // 2
        jc[far] = 9 + 14 * u(int(far.sum()), 3)
        js[far] = 3 + 7 * u(int(far.sum()), 3)
        lvl = (torch.arange(K) % len(SCALES)).to(F64)[:, None]
        if rotated:
            gt, r = torch.cat([c, s, th], 1), torch.cat([lvl, jc, js, jt], 1)
        else:
            gt, r = torch.cat([c - s / 2, c + s / 2], 1), torch.cat([lvl, jc - js / 2, jc + js / 2], 1)
        rois.append(r.float())
        gts.append(gt.float())
        labs.append(torch.ones(G, dtype=torch.float32))
    return rois, gts, labs


# ---- proposal targets ------------------------------------------------------------------------------------------------------------------------
def _ious(rois, gt):
    if rois.shape[0] == 0 or gt.shape[0] == 0:
        return torch.zeros((rois.shape[0], gt.shape[0]), dtype=F64)
    iou = pairwise(rois.to(F64), gt.to(F64))
    return torch.where(iou > 0, iou, torch.zeros_like(iou))


def _match(iou):
    if iou.shape[1] == 0:                                   # a scene without boxes: IoU 0 with "box 0"
        return torch.zeros(iou.shape[0], dtype=F64), torch.zeros(iou.shape[0], dtype=torch.int64), float("inf")
    best, arg = iou.max(1)
    arg = (iou == best[:, None]).to(torch.int64).argmax(1)
    gap = float("inf")
    if iou.shape[1] > 1 and iou.shape[0] > 0:
        top = iou.topk(2, dim=1).values
        gap = float((top[:, 0] - top[:, 1])[top[:, 0] > 0].min()) if bool((top[:, 0] > 0).any()) else float("inf")
    return best, arg, gap


def match(rois, gt):
    """rois [K, 6|7], gt [G, 6|7] -> (max IoU [K], arg [K] with ties to the lowest index, top-two gap)"""
    return _match(_ious(rois, gt))


def row_margins(iou, fg=FG, bg=BG):
    """iou [K, G] -> per row: best, arg, arg2 (the runner-up, ties to the lowest index; arg where there is none), d_fg, d_bg = |best - threshold|, gap = best -
    runner-up (inf where best is 0, an exact tie that goes to box 0 in fp32 as well, or where G < 2), decided = all three >= MARGIN"""
    K, G = iou.shape
    best, arg, _ = _match(iou)
    arg2, gap = arg.clone(), torch.full((K,), float("inf"), dtype=F64)
    if G > 1 and K > 0:
        rest = iou.clone()
        rest[torch.arange(K), arg] = -1.0
        second, _ = rest.max(1)
        arg2 = (rest == second[:, None]).to(torch.int64).argmax(1)
        gap = torch.where(best > 0, best - second, gap)
    d_fg, d_bg = (best - fg).abs(), (best - bg).abs()
    return dict(best=best, arg=arg, arg2=arg2, d_fg=d_fg, d_bg=d_bg, gap=gap, decided=(d_fg >= MARGIN) & (d_bg >= MARGIN) & (gap >= MARGIN))


def targets(all_rois, gt_boxes, gt_labels, fg=FG, bg=BG, keep=None, n_fg=None, rows=None, alt_arg=False, alt_label=False):
    """all_rois per scene [K, 1+6|7]; keep: per scene the kept indices (foreground slots first, n_fg[i] of them; -1: none) or None for evaluation ->
    (labels, rois, gt_rois: per scene, float64), margins.  A scene may have no RoIs or no boxes (IoU 0, zero gt_rois, label 0).  rows: margins["rows"] of an
    earlier call on the same inputs (the IoUs are not formed again).  alt_arg: rows whose top-two gap is below MARGIN take the runner-up box; alt_label
    (evaluation): rows within MARGIN of fg take the other label."""
    m = dict(iou_fg=float("inf"), iou_bg=float("inf"), iou_top2=float("inf"))
    L, Ro, Gr, cand, per_row = [], [], [], [], []
    for i, (r, g, gl) in enumerate(zip(all_rois, gt_boxes, gt_labels)):
        r, g = r.to(F64), g.to(F64)
        rm = row_margins(_ious(r[:, 1:], g), fg, bg) if rows is None else rows[i]
        per_row.append(rm)
        best, arg = rm["best"], rm["arg"]
        if r.shape[0]:
            m["iou_fg"] = min(m["iou_fg"], float(rm["d_fg"].min()))
            m["iou_bg"] = min(m["iou_bg"], float(rm["d_bg"].min()))
            m["iou_top2"] = min(m["iou_top2"], float(rm["gap"][best > 0].min()) if bool((best > 0).any()) else float("inf"))
        if alt_arg:
            arg = torch.where(rm["gap"] < MARGIN, rm["arg2"], arg)
        cand.append((torch.nonzero(best >= fg).view(-1), torch.nonzero((best < bg) & ~(best >= fg)).view(-1)))
        gbox = g[arg] if g.shape[0] else torch.zeros((r.shape[0], r.shape[1] - 1), dtype=F64)
        glab = gl.to(F64)[arg] if g.shape[0] else torch.zeros(r.shape[0], dtype=F64)
        if keep is None:
            lab = best >= fg
            L.append((lab ^ (rm["d_fg"] < MARGIN) if alt_label else lab).to(F64))
            Ro.append(r)
            Gr.append(gbox)
            continue
        k = torch.as_tensor(keep[i], dtype=torch.int64)
        ok = k >= 0
        kk = k.clamp_min(0)
        if r.shape[0] == 0:
            L.append(torch.full((k.numel(),), -1.0, dtype=F64))
            Ro.append(torch.zeros((k.numel(), r.shape[1]), dtype=F64))
            Gr.append(torch.zeros((k.numel(), r.shape[1] - 1), dtype=F64))
            continue
        lab = glab[kk]
        lab[n_fg[i]:] = 0
        L.append(torch.where(ok, lab, torch.full_like(lab, -1.0)))
        Ro.append(r[kk] * ok[:, None])
        Gr.append(gbox[kk] * ok[:, None])
    m["candidates"] = cand
    m["rows"] = per_row
    return L, Ro, Gr, m


# ---- the sampler, in Python integers (csrc/roi_head.hip's header, csrc/rpn_shared.hpp) ---------------------------------------------------------
_M64 = (1 << 64) - 1
_PHI, _STEP, _SECOND = 0x9E3779B97F4A7C15, 0xD1342543DE82EF95, 0x5851F42D4C957F2D


def mix64(x):
    """the splitmix64 finaliser on a 64-bit unsigned value"""
    x ^= x >> 30
    x = x * 0xBF58476D1CE4E5B9 & _M64
    x ^= x >> 27
    x = x * 0x94D049BB133111EB & _M64
    return x ^ (x >> 31)


def sample_stream(seed, counter, scene):
    return mix64(mix64((seed + _PHI * (counter + 1)) & _M64) ^ (((scene + 1) << 40) & _M64))


def sample_key(stream, idx):
    """the complemented hash of one proposal: the largest keys are the smallest hashes"""
    return ~(mix64((stream + idx * _STEP) & _M64) >> 32) & 0xFFFFFFFF


def sample_draw(stream2, j, cnt):
    """slot j's draw, uniform in 0 .. cnt-1: floor(h cnt / 2^32)"""
    return ((mix64((stream2 + j * _STEP) & _M64) >> 32) * cnt) >> 32


def sample(fg, bg, R, want_fg, seed, counter, scene):
    """fg, bg: the scene's candidate indices in index order -> (keep [R], (foreground slots, background slots), positions: the list position of every draw
    with replacement, per slot, None in the slots filled without replacement)"""
    fg, bg = [int(v) for v in fg], [int(v) for v in bg]
    stream = sample_stream(seed, counter, scene)
    stream2 = mix64(stream ^ _SECOND)
    if not fg and not bg:
        return [-1] * R, (0, 0), [None] * R
    if not fg or not bg:
        lst = fg or bg
        pos = [sample_draw(stream2, j, len(lst)) for j in range(R)]
        return [lst[p] for p in pos], ((R, 0) if fg else (0, R)), pos
    nf = min(max(want_fg, 0), len(fg), R)
    chosen = sorted(sorted(fg, key=lambda q: (-sample_key(stream, q), q))[:nf])          # the nf largest keys, ties to the lower index, written in index order
    pos = [sample_draw(stream2, j, len(bg)) for j in range(nf, R)]
    return chosen + [bg[p] for p in pos], (nf, R - nf), [None] * nf + pos


def level_map(boxes, k_min, k_max, s0, lvl0, eps=1e-6):
    """boxes [..., 6|7] -> (levels int64, margin of the floor)"""
    b = boxes.to(F64)
    v = lvl0 + torch.log2((b[..., 3] * b[..., 4] * b[..., 5]) ** (1.0 / 3.0) / s0) + eps
    return (v.floor().clamp(k_min, k_max) - k_min).to(torch.int64), _frac_margin(v)


def mapper_range(scales):
    return int(math.log2(scales[0])), int(math.log2(scales[-1]))


# ---- pooling -------------------------------------------------------------------------------------------------------------------------------
def _grid(roi, rotated, scale, dims, enlarge):
    """one RoI [6|7] float64 -> (size (gx, gy, gz), corner voxels [P, 8] (linear index in the map), weights [P, 8] (already / 8; axis-aligned: one corner of weight
    1), mask [P], floor margin, inside)"""
    W, H, D = dims
    if not rotated:
        half, mid = (roi[3:] - roi[:3]) / 2 * (1 + enlarge), (roi[3:] + roi[:3]) / 2
        q = torch.cat([-0.5 * half + mid, 0.5 * half + mid]) / scale
        p0, p1 = q[:3].floor().to(torch.int64), q[3:].floor().to(torch.int64)
        size = torch.tensor(dims)
        lo, hi = p0.clamp_min(0), torch.minimum(p1 + 1, size)
        s = (hi - lo).clamp_min(0)
        inside = bool((p0 >= 0).all() and (p1 + 1 <= size).all() and (s > 0).all())
        ix, iy, iz = torch.meshgrid(*[torch.arange(int(v)) for v in s], indexing="ij")
        vox = ((lo[0] + ix) * H + lo[1] + iy) * D + lo[2] + iz
        P = vox.numel()
        vox8 = vox.reshape(P, 1).repeat(1, 8)
        w8 = torch.zeros((P, 8), dtype=F64)
        w8[:, 0] = 1.0
        return tuple(int(v) for v in s), vox8, w8, torch.ones(P, dtype=torch.bool), _frac_margin(q), inside
    e = roi[3:6] * (1 + enlarge) / scale
    g = e.ceil().clamp_min(1).to(torch.int64)
    ix, iy, iz = [t.reshape(-1).to(F64) for t in torch.meshgrid(*[torch.arange(int(v)) for v in g], indexing="ij")]
    px, py, pz = ix - (g[0] - 1) / 2, iy - (g[1] - 1) / 2, iz - (g[2] - 1) / 2
    cs, sn = torch.cos(roi[6]), torch.sin(roi[6])
    X, Y, Z = cs * px - sn * py + roi[0] / scale, sn * px + cs * py + roi[1] / scale, pz + roi[2] / scale
    mask = (X >= 0) & (X <= W - 1) & (Y >= 0) & (Y <= H - 1) & (Z >= 0) & (Z <= D - 1)
    vox8, w8 = [], []
    for fa in (torch.floor, torch.ceil):
        for fb in (torch.floor, torch.ceil):
            for fc in (torch.floor, torch.ceil):
                a, b, c = fa(X), fb(Y), fc(Z)
                vox8.append((a.clamp(0, W - 1) * H + b.clamp(0, H - 1)) * D + c.clamp(0, D - 1))
                w8.append((1 - (X - a).abs() * (Y - b).abs() * (Z - c).abs()) / 8)
    margin = min(_frac_margin(e), _frac_margin(torch.stack([X, Y, Z])))
    return tuple(int(v) for v in g), torch.stack(vox8, 1).to(torch.int64), torch.stack(w8, 1), mask, margin, bool(mask.all())


def pool(maps, rois, scales=SCALES, out=(2, 2, 2), enlarge=ENLARGE, rotated=False, levels=None, dout=None, want_values=True):
    """maps: per level (N, C, W, H, D); rois [N, R, 1+6|7]; levels: [N, R] override (remap) -> (out [N*R, C, ow, oh, od] float64, margins, dmaps or None:
    the analytic gradient of sum(out * dout) with respect to the maps).  want_values=False: only the geometric margins."""
    N, R = rois.shape[:2]
    C = maps[0].shape[1]
    res = torch.zeros((N * R, C, *out), dtype=F64)
    dmaps = None if dout is None else [torch.zeros(m.shape, dtype=F64) for m in maps]
    m = dict(floor=float("inf"), cell_gap=float("inf"), inside=True, padded_cells=0, masked_points=0, ragged=0)
    for b in range(N):
        for r in range(R):
            roi = rois[b, r].to(F64)
            lvl = int(roi[0]) if levels is None else int(levels[b, r])
            if not 0 <= lvl < len(maps):
                continue
            dims = tuple(maps[lvl].shape[2:])
            s, vox8, w8, mask, fm, inside = _grid(roi[1:], rotated, float(scales[lvl]), dims, enlarge)
            m["floor"], m["inside"] = min(m["floor"], fm), m["inside"] and inside
            m["masked_points"] += int((~mask).sum())
            m["ragged"] += int(any(v % o for v, o in zip(s, out)))
            if not want_values or min(s) == 0:
                continue
            f = maps[lvl][b].to(F64).reshape(C, -1)
            val = (f[:, vox8] * w8[None]).sum(2)                     # [C, P]
            k = [-(-v // o) for v, o in zip(s, out)]
            idx = torch.arange(vox8.shape[0]).reshape(s)
            for ox in range(out[0]):
                for oy in range(out[1]):
                    for oz in range(out[2]):
                        pts = idx[ox * k[0]:(ox + 1) * k[0], oy * k[1]:(oy + 1) * k[1], oz * k[2]:(oz + 1) * k[2]].reshape(-1)
                        padded = (ox + 1) * k[0] > s[0] or (oy + 1) * k[1] > s[1] or (oz + 1) * k[2] > s[2]
                        m["padded_cells"] += int(padded)
                        real = pts[mask[pts]]
                        zero = padded or real.numel() < pts.numel()
                        cand = val[:, real]
                        if zero:
                            cand = torch.cat([cand, torch.zeros((C, 1), dtype=F64)], 1)
                        if cand.shape[1] == 0:
                            continue
                        top, arg = cand.max(1)
                        arg = (cand == top[:, None]).to(torch.int64).argmax(1)          # the first of equal values; a value before the zero
                        if cand.shape[1] > 1:
                            t2 = cand.topk(2, dim=1).values
                            m["cell_gap"] = min(m["cell_gap"], float((t2[:, 0] - t2[:, 1]).min()))
                        res[b * R + r, :, ox, oy, oz] = top
                        if dmaps is not None:
                            for c in range(C):
                                if arg[c] < real.numel():
                                    p = real[arg[c]]
                                    dmaps[lvl][b, c].view(-1).index_add_(0, vox8[p], w8[p] * dout[b * R + r, c, ox, oy, oz].to(F64))
    return res, m, dmaps


# ---- coders and losses -----------------------------------------------------------------------------------------------------------------------
def encode(gt, ex, rotated):
    gt, ex = gt.to(F64), ex.to(F64)
    if rotated:
        d = gt[:, :3] - ex[:, :3]
        cs, sn = torch.cos(ex[:, 6]), torch.sin(ex[:, 6])
        return torch.stack([(cs * d[:, 0] + sn * d[:, 1]) / ex[:, 3], (-sn * d[:, 0] + cs * d[:, 1]) / ex[:, 4], d[:, 2] / ex[:, 5], torch.log(gt[:, 3] / ex[:, 3]),
                            torch.log(gt[:, 4] / ex[:, 4]), torch.log(gt[:, 5] / ex[:, 5]), (gt[:, 6] - ex[:, 6]) / (2 * math.pi)], 1)
    es, gs = ex[:, 3:] - ex[:, :3], gt[:, 3:] - gt[:, :3]
    return torch.cat([((gt[:, :3] + 0.5 * gs) - (ex[:, :3] + 0.5 * es)) / es, torch.log(gs / es)], 1)


def decode(d, ex, rotated):
    """-> (boxes, margin of the angle wrap: distance of the unwrapped angle from a multiple of pi and from pi/2 mod pi)"""
    d, ex = d.to(F64), ex.to(F64)
    dw = d[:, 3:6].clamp_max(XFORM_CLIP)
    if rotated:
        cs, sn = torch.cos(ex[:, 6]), torch.sin(ex[:, 6])
        x = d[:, 0] * ex[:, 3] * cs - d[:, 1] * ex[:, 4] * sn + ex[:, 0]
        y = d[:, 0] * ex[:, 3] * sn + d[:, 1] * ex[:, 4] * cs + ex[:, 1]
        z = d[:, 2] * ex[:, 5] + ex[:, 2]
        raw = 2 * math.pi * d[:, 6] + ex[:, 6]
        a = raw - torch.floor(raw / math.pi) * math.pi
        margin = float(torch.minimum(torch.minimum(a, math.pi - a), (a - math.pi / 2).abs()).min())
        a = torch.where(a > math.pi / 2, a - math.pi, a)
        return torch.cat([torch.stack([x, y, z], 1), torch.exp(dw) * ex[:, 3:6], a[:, None]], 1), margin
    s = ex[:, 3:] - ex[:, :3]
    c = d[:, :3] * s + (ex[:, :3] + 0.5 * s)
    h = 0.5 * torch.exp(dw) * s
    return torch.cat([c - h, c + h], 1), float("inf")


def _sl1(d):
    return torch.where(d.abs() < BETA, 0.5 * d * d / BETA, d.abs() - 0.5 * BETA)


def loss(scores, deltas, labels, rois, gt_rois, rotated):
    """rows with label < 0 are ignored -> dict(obj, reg: the two losses; targets: the encoded regression targets, 0 in ignored rows; dscores = d obj / d scores;
    ddeltas = d reg / d deltas)"""
    s, d, lab = scores.to(F64), deltas.to(F64), labels.to(F64).reshape(-1)
    valid, pos = lab >= 0, lab > 0
    li = lab.clamp_min(0).to(torch.int64)
    t = encode(gt_rois, rois, rotated)
    t = torch.where(valid[:, None], t, torch.zeros_like(t))
    lse = torch.logsumexp(s, 1)
    nv, npos = int(valid.sum()), int(pos.sum())
    ce = (lse - s.gather(1, li[:, None])[:, 0]) * valid
    obj = ce.sum() / nv if nv else torch.zeros((), dtype=F64)
    diff = torch.where(pos[:, None], d - t, torch.zeros_like(d))
    reg = _sl1(diff).sum() / npos if npos else torch.zeros((), dtype=F64)
    onehot = torch.zeros_like(s).scatter_(1, li[:, None], 1.0)
    dscores = (torch.softmax(s, 1) - onehot) * valid[:, None] / max(nv, 1)
    ddeltas = torch.where(diff.abs() < BETA, diff / BETA, torch.sign(diff)) * pos[:, None] / max(npos, 1)
    return dict(obj=obj, reg=reg, targets=t, dscores=dscores, ddeltas=ddeltas)


# ---- the recorded runs -------------------------------------------------------------------------------------------------------------------------
def gold_inputs(rotated):
    seed, map_seed = GOLD_SEED[rotated]
    rois, gts, labs = make_scene(seed, rotated, N=GOLD["N"], K=GOLD["K"], G=GOLD["G"])
    return rois, gts, labs, make_maps(map_seed, GOLD["C"], GOLD["N"])


def gold_head(rotated):
    """the tiny RCNN's parameters and its deterministic initialisation: (weights for bbox_pred [B, C*8], cls_score [2, C*8], biases)"""
    B, width = (7 if rotated else 6), GOLD["C"] * 8
    g = torch.Generator().manual_seed(77)
    return dict(RCNN_bbox_pred_w=torch.randn((B, width), generator=g, dtype=torch.float32) * 0.01, RCNN_bbox_pred_b=torch.randn((B,), generator=g, dtype=torch.float32) * 0.05,
                RCNN_cls_score_w=torch.randn((2, width), generator=g, dtype=torch.float32) * 0.01, RCNN_cls_score_b=torch.randn((2,), generator=g, dtype=torch.float32) * 0.05)


def input_sums(rois, gts, maps):
    return np.array([sum(t.double().sum().item() for t in ts) for ts in (rois, gts, maps)], dtype=np.float64)


# ---- targets and sampling at real extents ------------------------------------------------------------------------------------------------------
# Six scenes in one dense triple of cap 2500.  counts: a full cap, one past a 1024-lane chunk of the sampler, exactly a chunk, a single row, an empty scene,
# one past two chunks.  G: across the 64-box stage of the matching twice (130), one past it, on it, none, one, just past it.  The scene without boxes has one
# proposal, so that its IoU 0, box 0 and zero gt_rois are compared; the scene without proposals has one box.
BIG = dict(cap=2500, counts=(2500, 1025, 1024, 1, 0, 2049), G=(130, 65, 64, 0, 1, 70), R=1500, max_undecided=0.03)
BIG_SEED = {False: 0, True: 0}                                              # every scene's undecided share <= 3 %: tests/test_roi_head_ref_cpu.py


def big_case(rotated, seed=None):
    """-> dict(rois, gts, labs: per scene, rois [counts[i], 1+6|7]; boxes [N, cap, 6|7], levels [N, cap] int32: the dense form, rows past counts[i] hold
    garbage (boxes 5 .. 6, level 7); counts).  Labels cycle through 1 .. 5 so that a wrong matched box shows in the label."""
    seed = BIG_SEED[rotated] if seed is None else seed
    B, cap = (7 if rotated else 6), BIG["cap"]
    g = torch.Generator().manual_seed(4242 + seed)
    rois, gts, labs = [], [], []
    boxes, levels = 5 + torch.rand((len(BIG["counts"]), cap, B), generator=g, dtype=torch.float32), torch.full((len(BIG["counts"]), cap), 7, dtype=torch.int32)
    for i, (k, ng) in enumerate(zip(BIG["counts"], BIG["G"])):
        r, gt, _ = make_scene(100 * seed + i, rotated, N=1, K=max(k, 1), G=max(ng, 1))
        rois.append(r[0][:k])
        gts.append(gt[0][:ng])
        labs.append((1 + torch.arange(ng) % 5).to(torch.float32))
        boxes[i, :k], levels[i, :k] = rois[i][:, 1:], rois[i][:, 0].to(torch.int32)
    return dict(rois=rois, gts=gts, labs=labs, boxes=boxes, levels=levels, counts=list(BIG["counts"]))


def big_keep(candidates, R=None, seed=0):
    """kept rows from the restatement's candidates: up to R / 2 foreground rows (a seeded subset in index order), background rows with replacement; one class
    only: every slot from it; neither: -1 -> (keep [N, R] int64, n_fg)"""
    R = BIG["R"] if R is None else R
    g = torch.Generator().manual_seed(99 + seed)
    keep, n_fg = [], []
    for f, b in candidates:
        draw = lambda lst, n: lst[torch.randint(lst.numel(), (n,), generator=g)]          # noqa: E731
        if f.numel() and b.numel():
            nf = min(R // 2, f.numel())
            keep.append(torch.cat([f[torch.randperm(f.numel(), generator=g)[:nf]].sort().values, draw(b, R - nf)]))
        elif f.numel() or b.numel():
            nf = R if f.numel() else 0
            keep.append(draw(f if f.numel() else b, R))
        else:
            nf = 0
            keep.append(torch.full((R,), -1, dtype=torch.int64))
        n_fg.append(nf)
    return torch.stack(keep), n_fg


# The sampling scenes: one box and proposals that are copies of it (IoU 1), disjoint (IoU 0) or half overlapping (IoU 1/3: neither class), so that every row
# is decided by construction.  (foreground, background, neither) per scene: all three chunks of the sampler with a cut (want_fg below the foreground count)
# and more than 1024 background candidates; foreground only; background only; neither; fewer foreground rows than wanted (no cut); no proposals at all.
SAMPLER = dict(cap=2500, scenes=((900, 1300, 300), (1500, 0, 600), (0, 800, 230), (0, 0, 300), (20, 2000, 280), (0, 0, 0)), runs=((64, 32), (1500, 750)), seed=11, counters=(0, 5))


def sampler_case():
    """-> dict(boxes [N, cap, 6], levels, counts, gts, labs, kind: per scene [count] 0 / 1 / 2); rows past the counts are copies of the box (they would be
    foreground if read) with level 7"""
    cap, N = SAMPLER["cap"], len(SAMPLER["scenes"])
    gt = torch.tensor([[0.0, 0, 0, 4, 4, 4]])
    proto = torch.tensor([[0.0, 0, 0, 4, 4, 4], [10.0, 10, 10, 14, 14, 14], [2.0, 0, 0, 6, 4, 4]])
    boxes, levels = proto[0].repeat(N, cap, 1), torch.full((N, cap), 7, dtype=torch.int32)
    kinds, counts = [], []
    for i, ns in enumerate(SAMPLER["scenes"]):
        kind = torch.repeat_interleave(torch.arange(3), torch.tensor(ns))
        kind = kind[torch.randperm(kind.numel(), generator=torch.Generator().manual_seed(50 + i))]
        boxes[i, :kind.numel()], levels[i, :kind.numel()] = proto[kind], (torch.arange(kind.numel()) % 3).to(torch.int32)
        kinds.append(kind)
        counts.append(kind.numel())
    return dict(boxes=boxes, levels=levels, counts=counts, gts=[gt] * N, labs=[torch.full((1,), 3.0)] * N, kind=kinds)


def sampler_rois(case):
    return [torch.cat([case["levels"][i, :k, None].float(), case["boxes"][i, :k]], 1) for i, k in enumerate(case["counts"])]


# ---- the two stages joined ---------------------------------------------------------------------------------------------------------------------
# The first stage's restatement (tests/_rpn_post_ref.py) on its recorded heads with two of the configurations of tests/test_rpn_post_gpu.py (pre 200, post 100,
# NMS 0.3, N = 2), its four levels as the pyramid of the second stage (strides 4 / 8 / 16 / 32 of the 32^3 mesh, maps 8^3 .. 1^3), the tiny head of the
# recorded runs (C = 4, output 2^3, 12 rows per batch).  empty: a third scene whose objectness lies 20 below, with score_thresh 0.5 so that it hands over no
# proposal (the input of that suite's test_a_scene_where_every_box_is_dropped); the other two scenes lose their proposals below 0.5 as well.
JOIN = dict(pre=200, post=100, nms=0.3, scales=(4, 8, 16, 32), batch=12, cap=517, shift={False: 0.05, True: 0.1}, map_seed={(False, False): 0, (False, True): 0, (True, False): 2, (True, True): 2})


def joined_case(rotated, empty=False, map_seed=None, shift=None):
    """-> dict(obj, reg, ori, score: the first stage's inputs; res, marg: its restatement; rois (float64, level in front), gts, labs: per scene; rows,
    candidates: the float64 matching; keep [N, R], n_fg: kept rows chosen among the candidates that are decided rows and keep MARGIN on every floor of their
    pooling grid, foreground first; maps; R)"""
    from tests import _rpn_post_ref as P
    from tests import _rpn_ref as RR
    obj, reg = P.inputs(P.HEAD_SEED[rotated], rotated)
    ori, score = list(RR.ORI), 0.0
    if empty:
        o3, r3 = P.inputs(5, rotated, N=1)
        obj, reg = [torch.cat([a, b - 20.0]) for a, b in zip(obj, o3)], [torch.cat([a, b]) for a, b in zip(reg, r3)]
        ori, score = ori + [RR.MESH], 0.5
    N = len(ori)
    res, marg = P.proposals(obj, reg, ori=ori, pre_nms_top_n=JOIN["pre"], post_nms_top_n=JOIN["post"], nms_thresh=JOIN["nms"], score_thresh=score, rotated=rotated)
    rois = [torch.cat([r["level"].to(F64)[:, None], r["boxes"]], 1) for r in res]
    gts, shift = [], (JOIN["shift"][rotated] if shift is None else shift)
    for r in rois:                         # three of the scene's own proposals, 10 % larger (IoU 0.75 with their proposal) and moved a little
        K = r.shape[0]
        g = r[[1, K // 3, 2 * K // 3], 1:].clone() if K >= 3 else torch.tensor([[12.0, 12, 12, 8, 8, 8, 0.3]] if rotated else [[8.0, 8, 8, 16, 16, 16]], dtype=F64)
        if K >= 3 and rotated:
            g[:, 3:6] *= 1.1
            g[:, :3] += shift
        elif K >= 3:
            c, h = (g[:, :3] + g[:, 3:]) / 2 + shift, (g[:, 3:] - g[:, :3]) / 2 * 1.1
            g = torch.cat([c - h, c + h], 1)
        gts.append(g.float())
    labs = [torch.ones(g.shape[0], dtype=torch.float32) for g in gts]
    m = targets(rois, gts, labs)[3]
    dims = [tuple(int(v) for v in g) for g in RR.GRIDS]
    R = JOIN["batch"] // N
    keep, n_fg = [], []
    for r, rm, (f, b) in zip(rois, m["rows"], m["candidates"]):
        good = [bool(rm["decided"][q]) and _grid(r[q, 1:], rotated, float(JOIN["scales"][int(r[q, 0])]), dims[int(r[q, 0])], ENLARGE)[4] >= MARGIN for q in range(r.shape[0])]
        f, b = [int(q) for q in f if good[q]], [int(q) for q in b if good[q]]
        if not f or not b:
            keep.append([-1] * R)
            n_fg.append(0)
            continue
        nf = min(R // 2, len(f))
        b = sorted(b, key=lambda q: (-int(r[q, 0]), q))                                  # the coarse levels first, so that the kept rows mix the levels
        keep.append(f[:nf] + [b[j % len(b)] for j in range(R - nf)])
        n_fg.append(nf)
    seed = JOIN["map_seed"][(rotated, empty)] if map_seed is None else map_seed
    return dict(obj=obj, reg=reg, ori=ori, score=score, res=res, marg=marg, rois=rois, gts=gts, labs=labs, rows=m["rows"], candidates=m["candidates"], keep=torch.tensor(keep), n_fg=n_fg,
                maps=make_maps(seed, GOLD["C"], N, dims), R=R)


def joined_chain(case, rotated):
    """the second stage in float64 on the case's kept rows -> dict(L, Ro, Gr: [N, R, ..]; pooled; margins of the pooling; deltas, scores; loss (H.loss);
    boxes, wrap: the decode and its margin; dmaps, dparams: the gradient of the sum of both losses)"""
    N, R, B = len(case["rois"]), case["R"], 7 if rotated else 6
    L, Ro, Gr, _ = targets(case["rois"], case["gts"], case["labs"], keep=case["keep"], n_fg=case["n_fg"], rows=case["rows"])
    L, Ro, Gr = torch.stack(L), torch.stack(Ro), torch.stack(Gr)
    pooled, pm, _ = pool(case["maps"], Ro, scales=JOIN["scales"], out=GOLD["out"], rotated=rotated)
    hp = {k: v.double() for k, v in gold_head(rotated).items()}
    x = pooled.reshape(N * R, -1)
    deltas, scores = x @ hp["RCNN_bbox_pred_w"].T + hp["RCNN_bbox_pred_b"], x @ hp["RCNN_cls_score_w"].T + hp["RCNN_cls_score_b"]
    ex = Ro.reshape(N * R, -1)[:, 1:].clone()
    if rotated:                            # with remap off the model encodes and decodes against the enlarged RoIs
        ex[:, 3:6] *= 1 + ENLARGE
    lo = loss(scores, deltas, L.reshape(-1), ex, Gr.reshape(N * R, B), rotated)
    boxes, wrap = decode(deltas, ex, rotated)
    dx = lo["dscores"] @ hp["RCNN_cls_score_w"] + lo["ddeltas"] @ hp["RCNN_bbox_pred_w"]
    _, _, dmaps = pool(case["maps"], Ro, scales=JOIN["scales"], out=GOLD["out"], rotated=rotated, dout=dx.reshape(pooled.shape))
    dparams = dict(RCNN_bbox_pred_w=lo["ddeltas"].T @ x, RCNN_bbox_pred_b=lo["ddeltas"].sum(0), RCNN_cls_score_w=lo["dscores"].T @ x, RCNN_cls_score_b=lo["dscores"].sum(0))
    return dict(L=L, Ro=Ro, Gr=Gr, ex=ex, pooled=pooled, pm=pm, deltas=deltas, scores=scores, loss=lo, boxes=boxes, wrap=wrap, dmaps=dmaps, dparams=dparams)


# ---- the pooling cases of the GPU tests --------------------------------------------------------------------------------------------------------
NONCUBIC = [(16, 12, 8), (8, 6, 4), (4, 3, 2)]                     # a 32 x 24 x 16 mesh
# (rotated, non-cubic maps, C, output size) -> (scene seed, map seed), found with pool_case_search below: every margin >= MARGIN
POOL_CASES = {(False, False, 8, (2, 2, 2)): (0, 0), (False, True, 5, (3, 2, 1)): (0, 0), (True, False, 5, (3, 2, 1)): (0, 1), (True, True, 8, (2, 2, 2)): (0, 0)}
# Past one channel group and one workgroup per RoI, on the RoI sets above (the oriented geometry margins admit no larger set), map seeds found with
# pool_map_search below.  C = 20, output (5, 4, 3): three channel groups of 8, the last with 4 channels, several points per cell (maxima).  C = 12, output
# (7, 7, 7): 343 cells x 2 groups = 686 lanes = 3 workgroups per RoI, at most one point per cell (addressing).
POOL_WIDE = {(False, False, 20, (5, 4, 3)): (0, 0), (False, True, 20, (5, 4, 3)): (0, 0), (True, False, 20, (5, 4, 3)): (0, 4), (True, True, 20, (5, 4, 3)): (0, 4),
             (False, False, 12, (7, 7, 7)): (0, 0), (False, True, 12, (7, 7, 7)): (0, 0), (True, False, 12, (7, 7, 7)): (0, 0), (True, True, 12, (7, 7, 7)): (0, 0)}
POOL_CASES.update(POOL_WIDE)
# four levels (a 2^3 map at scale 16 behind the cubic three): rotated -> (scene seed, map seed), found with pool4_search below
SCALES4 = SCALES + (16,)
POOL4 = dict(C=12, out=(2, 2, 2), seeds={False: (0, 0), True: (5, 2)})


def pool_rois(seed, rotated, N=2, K=None):
    """[N, K + 3, 1+6|7]: K seeded RoIs spread over the levels (20 axis-aligned; 12 oriented, where every sampling point of every RoI has three coordinates that
    must keep MARGIN from an integer, and a larger set has no seed that does), then one whose grid is smaller than any output (padding-only cells), one partly outside its map
    (masked points, or a clamped crop) and one with theta = 0 at integer positions (an odd grid centred on a voxel)"""
    rois, _, _ = make_scene(seed, rotated, N=N, K=K or (12 if rotated else 20))
    if rotated:
        extra = [[2, 12.3, 13.1, 6.7, 3.0, 3.0, 3.0, 0.7], [1, 29.3, 5.23, 9.17, 14.0, 9.0, 8.0, 0.41], [0, 12.0, 14.0, 10.0, 4.5, 4.5, 4.5, 0.0]]
    else:
        extra = [[2, 10.8, 11.6, 5.2, 13.8, 14.6, 8.2], [1, 26.3, -3.1, 4.2, 37.4, 9.3, 13.9], [0, 9.1, 11.2, 7.3, 15.2, 17.1, 12.9]]
    return torch.stack([torch.cat([r, torch.tensor(extra, dtype=torch.float32)]) for r in rois])


def pool_case(key):
    rotated, noncubic, C, out = key
    seed, map_seed = POOL_CASES[key]
    rois = pool_rois(seed, rotated)
    return rois, make_maps(map_seed, C, rois.shape[0], NONCUBIC if noncubic else None)


def pool4_case(rotated, seed=None, map_seed=None):
    """pool_rois with every third RoI moved to level 3 and maps of four levels -> (rois, maps)"""
    seed, map_seed = (POOL4["seeds"][rotated][0] if seed is None else seed), (POOL4["seeds"][rotated][1] if map_seed is None else map_seed)
    rois = pool_rois(seed, rotated)
    rois[:, ::3, 0] = 3.0
    return rois, make_maps(map_seed, POOL4["C"], rois.shape[0], [tuple(m // s for m in MESH) for s in SCALES4])


def pool4_search(limit=200):
    for rotated in (False, True):
        for seed in range(limit):
            rois, maps = pool4_case(rotated, seed, 0)
            _, m, _ = pool(maps, rois, scales=SCALES4, out=POOL4["out"], rotated=rotated, want_values=False)
            if m["floor"] < MARGIN:
                continue
            for map_seed in range(20):
                rois, maps = pool4_case(rotated, seed, map_seed)
                _, m, _ = pool(maps, rois, scales=SCALES4, out=POOL4["out"], rotated=rotated)
                if m["cell_gap"] >= MARGIN:
                    print("POOL4", rotated, (seed, map_seed), {k: m[k] for k in ("floor", "cell_gap", "padded_cells", "masked_points", "ragged")}, flush=True)
                    break
            else:
                continue
            break


def pool_map_search(limit=16):
    """the first map seed of every POOL_WIDE case that keeps every margin, on the recorded scene seed"""
    for key, (seed, _) in POOL_WIDE.items():
        rotated, noncubic, C, out = key
        rois = pool_rois(seed, rotated)
        for map_seed in range(limit):
            _, m, _ = pool(make_maps(map_seed, C, rois.shape[0], NONCUBIC if noncubic else None), rois, out=out, rotated=rotated)
            if min(m["floor"], m["cell_gap"]) >= MARGIN:
                print(key, (seed, map_seed), {k: m[k] for k in ("floor", "cell_gap", "padded_cells", "masked_points", "ragged")}, flush=True)
                break
        else:
            print(key, "no map seed below", limit, flush=True)


# the oriented remap case of the GPU tests: (scene seed, map seed), found with remap_case_search below
REMAP_CASE = (11, 0)


def remap_case(seed=None, map_seed=None):
    """Oriented RoIs for ROIPool(remap=True) and the model around it: the recorded runs' sizes (GOLD), with the last two RoIs of each scene resized to a cube
    root of 18 and 34 mesh units so that the level mapper (k 1..3, canonical 32 at level 3) uses all three levels; kept rows chosen from the restatement's
    candidates: up to R / 2 foreground rows in index order, then background rows cyclically.
    -> dict(rois, gts, labs: per scene; maps; levels [N, K]; keep [N, R], n_fg; margins: every discrete decision, None if a scene lacks a class)"""
    seed, map_seed = (REMAP_CASE[0] if seed is None else seed), (REMAP_CASE[1] if map_seed is None else map_seed)
    rois, gts, labs = make_scene(seed, True, N=GOLD["N"], K=GOLD["K"], G=GOLD["G"])
    for r in rois:
        for row, side in ((-2, 18.0), (-1, 34.0)):
            r[row, 4:7] *= side / float(r[row, 4:7].double().prod() ** (1.0 / 3.0))
    maps = make_maps(map_seed, GOLD["C"], GOLD["N"])
    kmin, kmax = mapper_range(SCALES)
    dense = torch.stack(rois)
    levels, lm = level_map(dense[..., 1:], kmin, kmax, GOLD["max_res"], len(SCALES))
    m = targets(rois, gts, labs)[3]
    case = dict(rois=rois, gts=gts, labs=labs, maps=maps, levels=levels, keep=None, n_fg=None, margins=None)
    if any(fg.numel() == 0 or bg.numel() == 0 for fg, bg in m["candidates"]):
        return case
    R, keep, n_fg = GOLD["R"], [], []
    for fg, bg in m["candidates"]:
        nf = min(R // 2, fg.numel())
        keep.append(torch.cat([fg[:nf], bg[torch.arange(R - nf) % bg.numel()]]))
        n_fg.append(nf)
    _, pm, _ = pool(maps, dense, out=GOLD["out"], rotated=True, levels=levels, want_values=map_seed is not None)
    case.update(keep=torch.stack(keep), n_fg=n_fg, margins=dict(level=lm, iou=min(m["iou_fg"], m["iou_bg"], m["iou_top2"]), floor=pm["floor"], cell_gap=pm["cell_gap"],
                                                                 levels_used=len(set(levels.reshape(-1).tolist())), masked_points=pm["masked_points"]))
    return case


def remap_case_search(limit=3000):
    for seed in range(limit):
        for map_seed in range(20):
            m = remap_case(seed, map_seed)["margins"]
            if m is None or min(m["level"], m["iou"], m["floor"]) < MARGIN:
                break
            if m["cell_gap"] >= MARGIN:
                print("REMAP_CASE", (seed, map_seed), m, flush=True)
                return


def pool_case_search(limit=3000, only=None):
    for key in POOL_CASES:
        if only is not None and key[0] != only:
            continue
        rotated, noncubic, C, out = key
        dims = NONCUBIC if noncubic else None
        for seed in range(limit):
            rois = pool_rois(seed, rotated)
            _, m, _ = pool(make_maps(0, 1, rois.shape[0], dims), rois, out=out, rotated=rotated, want_values=False)
            if m["floor"] < MARGIN:
                continue
            for map_seed in range(60):
                _, m, _ = pool(make_maps(map_seed, C, rois.shape[0], dims), rois, out=out, rotated=rotated)
                if m["cell_gap"] >= MARGIN:
                    print(key, (seed, map_seed), {k: m[k] for k in ("floor", "cell_gap", "padded_cells", "masked_points", "ragged")}, flush=True)
                    break
            else:
                continue
            break
        else:
            print(key, "no seed below", limit, flush=True)
