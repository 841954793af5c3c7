"""Float64 restatement of the RPN inference path (nerf_mae_amd.rpn over csrc/rpn_post.hip): both decoders, the masked top-k per level on the fp32 bits of
the logits, the clip / centre / size / score filters, NMS within each level and the post-NMS cut, written from the semantics stated in the header of
csrc/rpn_post.hip (plain PyTorch / numpy on the CPU).  It builds on tests/_rpn_ref.py (geometry, anchors, padding masks, make_heads) and
tests/_obb_iou_ref.py (pairwise).  tests/test_rpn_post_ref_cpu.py checks it against tests/golden/g21_rpn_proposals.npz, recorded from the reference's
own Python by tools/gen_golden_rpn_post.py; the GPU tests are measured against it.

Selection and order work on the bits of the fp32 logits and need no margin.  Every other discrete choice depends on arithmetic, so `proposals` also
returns the smallest distance of each to its boundary:
  m_score  sigmoid(logit) against score_thresh (absolute; only when score_thresh > 0);
  m_size   a side against min_size (absolute);
  m_centre an oriented centre against 0 and the mesh (absolute);
  m_swap   |w - h| of regular_obb (absolute);
  m_wrap   the angle before the floor modulo against the multiples of the reference's pi (absolute, radians);
  m_iou    |IoU - nms_thresh| over the pairs the greedy walk consults.
The decoders take any float dtype, so that their fp32 evaluation can be measured against their float64 one (the tolerances of the GPU tests)."""
import math

import numpy as np
import torch

from tests import _obb_iou_ref as I
from tests import _rpn_ref as R
from tests._fcos_post_ref import nms_margin

F64 = torch.float64
MARGIN = 1e-5
XFORM_CLIP = math.log(2000.0)
RATIO_CLIP = abs(math.log(16 / 1000))
REF_PI = 3.141592                          # the reference's own constant (coder/misc.py)
MIN_SIZE = 1e-3
CFG = dict(pre_nms_top_n=200, post_nms_top_n=100, nms_thresh=0.3, score_thresh=0.0)      # the recorded configuration
HEAD_SEED = {False: 0, True: 1}            # tools/gen_golden_rpn_post.py --search


# ---- decoders ------------------------------------------------------------------------------------------------------------------------------
def decode_aabb(d, anc):
    """d [n, 6] deltas, anc [n, 6] anchors (same dtype) -> [n, 6] boxes, not clipped"""
    e = anc[:, 3:] - anc[:, :3]
    c = anc[:, :3] + 0.5 * e
    p = d[:, :3] * e + c
    h = 0.5 * (torch.exp(d[:, 3:6].clamp(max=XFORM_CLIP)) * e)
    return torch.cat([p - h, p + h], 1)


def decode_obb(d, anc, want_margins=False):
    """d [n, 8] deltas, anc [n, 6] anchors -> [n, 7] (x, y, z, w, h, d, theta) (and the per-row margins of the w/h swap and of the theta wrap)"""
    p = (anc[:, :3] + anc[:, 3:]) * 0.5
    e = anc[:, 3:] - anc[:, :3]
    g = e * torch.exp(d[:, 3:6].clamp(-RATIO_CLIP, RATIO_CLIP))
    c = p + e * d[:, :3]
    gx, gy, gw, gh = c[:, 0], c[:, 1], g[:, 0], g[:, 1]
    x1, y1, x2, y2 = gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5
    da, db = d[:, 6].clamp(-0.5, 0.5), d[:, 7].clamp(-0.5, 0.5)
    X = torch.stack([(gx + da * gw) - gx, x2 - gx, (gx - da * gw) - gx, x1 - gx], 1)
    Y = torch.stack([y1 - gy, (gy + db * gh) - gy, y2 - gy, (gy - db * gh) - gy], 1)
    ln = torch.sqrt(X * X + Y * Y)
    s = ln.max(1, keepdim=True).values / ln
    X, Y = X * s + gx[:, None], Y * s + gy[:, None]
    th = torch.atan2(-(Y[:, 1] - Y[:, 0]), X[:, 1] - X[:, 0] + 1e-7)
    cs, sn = torch.cos(th), torch.sin(th)
    x, y = X.sum(1) / 4, Y.sum(1) / 4
    ux, uy = X - x[:, None], Y - y[:, None]
    rx, ry = ux * cs[:, None] - uy * sn[:, None], ux * sn[:, None] + uy * cs[:, None]
    w, h = rx.max(1).values - rx.min(1).values, ry.max(1).values - ry.min(1).values
    keep = w > h
    t = torch.where(keep, th, th + REF_PI / 2) + REF_PI / 2
    out = torch.stack([x, y, c[:, 2], torch.where(keep, w, h), torch.where(keep, h, w), g[:, 2], torch.remainder(t, REF_PI) - REF_PI / 2], 1)
    if not want_margins:
        return out
    k = torch.round(t / REF_PI)
    near = torch.minimum((t - k * REF_PI).abs(), torch.minimum((t - (k + 1) * REF_PI).abs(), (t - (k - 1) * REF_PI).abs()))
    return out, (w - h).abs(), near


def anchors_t(mesh=R.MESH, grids=R.GRIDS, base=None, dtype=F64):
    return torch.from_numpy(R.anchors(mesh, grids, base)).to(dtype)


def decode_all(reg, rotated, mesh=R.MESH, grids=R.GRIDS, base=None, dtype=F64, want_margins=False):
    """per-level regression tensors -> [N, n, 6|7] in anchor order, evaluated in `dtype`"""
    C = 8 if rotated else 6
    N = reg[0].shape[0]
    r = torch.cat([t.reshape(N, -1, C, *t.shape[2:]).permute(0, 3, 4, 5, 1, 2).reshape(N, -1, C) for t in reg], 1).to(dtype)
    anc = anchors_t(mesh, grids, base, dtype)
    n = anc.shape[0]
    flat, ancs = r.reshape(N * n, C), anc.repeat(N, 1)
    if not rotated:
        return decode_aabb(flat, ancs).reshape(N, n, 6)
    out = decode_obb(flat, ancs, want_margins)
    if want_margins:
        return out[0].reshape(N, n, 7), out[1].reshape(N, n), out[2].reshape(N, n)
    return out.reshape(N, n, 7)


# ---- selection -------------------------------------------------------------------------------------------------------------------------------
def order_keys(x):
    """fp32 logits (numpy) -> int64 keys whose order is the float order of the bits (-0 below +0, NaN read as -inf); all >= 0x007fffff"""
    x = np.where(np.isnan(x), np.float32(-np.inf), x).astype(np.float32)
    u = x.view(np.uint32).astype(np.int64)
    return np.where(u >> 31 == 1, (~u) & 0xFFFFFFFF, u | 0x80000000)


def memory_valid(ori, grid, stride, A):
    """[A W H D] bool in the objectness tensor's memory order"""
    lim = [math.ceil(o / s) for o, s in zip(ori, stride)]
    m = np.zeros((A, *grid), dtype=bool)
    m[:, :lim[0], :lim[1], :lim[2]] = True
    return m.reshape(-1)


def proposals(obj, reg, ori=None, pre_nms_top_n=200, post_nms_top_n=100, nms_thresh=0.3, score_thresh=0.0, min_size=MIN_SIZE, rotated=False, mesh=R.MESH, grids=R.GRIDS,
              base=None):
    """obj, reg: per-level fp32 head tensors on the CPU; ori: per-scene original sizes or None -> (results, margins): one dict per scene with level, index
    (anchor index within the scene), boxes [K, 6|7] and scores [K] float64 in the order of the outputs, pre_* for the filled slots in slot order and
    unmasked[k] = the level's number of unmasked anchors"""
    base = R.base_anchors() if base is None else base
    N, L = obj[0].shape[0], len(obj)
    A = [len(b) for b in base]
    strides = R.strides(mesh, grids)
    nloc = [g[0] * g[1] * g[2] for g in grids]
    offs = np.concatenate([[0], np.cumsum([n * a for n, a in zip(nloc, A)])])
    if rotated:
        dec, m_swap, m_wrap = decode_all(reg, True, mesh, grids, base, want_margins=True)
    else:
        dec = decode_all(reg, False, mesh, grids, base)
    marg = dict(m_score=math.inf, m_size=math.inf, m_centre=math.inf, m_swap=math.inf, m_wrap=math.inf, m_iou=math.inf)
    hi = torch.tensor([float(v) for v in mesh], dtype=F64)
    out = []
    for b in range(N):
        pl, pi, pk, ps, unmasked = [], [], [], [], []
        for k in range(L):
            x = obj[k][b].reshape(-1).numpy()
            key = order_keys(x)
            valid = np.ones(x.shape, dtype=bool) if ori is None else memory_valid(ori[b], grids[k], strides[k], A[k])
            key = np.where(valid, key, 0)
            unmasked.append(int(valid.sum()))
            t = min(pre_nms_top_n, key.size)
            sel = np.sort(np.argsort(-key, kind="stable")[:t])          # the t largest, ties to the lower offset; slots in ascending offset
            a, loc = sel // nloc[k], sel % nloc[k]
            pi.append(offs[k] + loc * A[k] + a)
            pl.append(np.full(t, k))
            pk.append(np.where(valid[sel], key[sel], 1))
            xs = torch.from_numpy(np.where(np.isnan(x[sel]), np.float32(-np.inf), x[sel])).to(F64)
            ps.append(torch.where(torch.from_numpy(valid[sel]), torch.sigmoid(xs), torch.zeros_like(xs)))
        lv, ix, ky, sc = torch.from_numpy(np.concatenate(pl)), torch.from_numpy(np.concatenate(pi)), torch.from_numpy(np.concatenate(pk)), torch.cat(ps)
        bx = dec[b][ix]
        if rotated:
            marg["m_swap"] = min(marg["m_swap"], m_swap[b][ix].min().item())
            marg["m_wrap"] = min(marg["m_wrap"], m_wrap[b][ix].min().item())
            ctr = bx[:, :3]
            marg["m_centre"] = min(marg["m_centre"], torch.minimum(ctr.abs(), (ctr - hi).abs()).min().item())
            ok = ((ctr >= 0) & (ctr <= hi)).all(1)
            sides = bx[:, 3:6]
        else:
            bx = torch.minimum(bx.clamp_min(0.0), hi.repeat(2))
            ok = torch.ones(bx.shape[0], dtype=torch.bool)
            sides = bx[:, 3:] - bx[:, :3]
        marg["m_size"] = min(marg["m_size"], (sides - min_size).abs().min().item())
        ok &= (sides >= min_size).all(1)
        if score_thresh > 0:
            marg["m_score"] = min(marg["m_score"], (sc - score_thresh).abs().min().item())
        ok &= sc >= score_thresh
        lv, ix, ky, sc, bx = lv[ok], ix[ok], ky[ok], sc[ok], bx[ok]
        res = dict(pre_level=lv, pre_index=ix, pre_boxes=bx, pre_scores=sc, pre_keys=ky, unmasked=unmasked)
        keep = []
        for k in range(L):
            at = torch.nonzero(lv == k).reshape(-1)
            if at.numel() == 0:
                continue
            kk, m = nms_margin(I.pairwise(bx[at], bx[at]), ky[at].to(F64), nms_thresh)      # keys are below 2^32: exact in float64
            marg["m_iou"] = min(marg["m_iou"], m)
            keep += at[kk].tolist()
        keep = torch.tensor(keep, dtype=torch.int64)
        keep = keep[torch.sort(-ky[keep] * (1 << 20) + keep, stable=True).indices][:post_nms_top_n]      # descending key, ties to the lower slot
        res.update(level=lv[keep], index=ix[keep], boxes=bx[keep], scores=sc[keep])
        out.append(res)
    return out, marg


def decision_margins(*args, **kwargs):
    return proposals(*args, **kwargs)[1]


def inputs(seed, rotated, N=2):
    """the recorded inputs: tests/_rpn_ref.make_heads(seed, N, C) on the _rpn_ref geometry.  For the oriented form two things are changed, both because the
    reference could not be recorded otherwise.  The three centre deltas of every anchor become 0.02 |delta|: anchors of grid index 0 are centred ON the mesh
    boundary, so any negative centre delta puts the decoded centre outside the mesh, where the reference pairs boxes with the wrong scores.  da and db are
    scaled by 0.2: when both are clamped at 0.5 the rectangle is axis-aligned with theta = -pi/2 from atan2, which the reference's pi = 3.141592 places 3e-7
    below its own wrap boundary, far inside MARGIN.  The crafted inputs of the GPU tests cover centres outside and the clamps."""
    obj, reg = R.make_heads(seed, N, 8 if rotated else 6)
    if rotated:
        for t in reg:
            v = t.view(N, -1, 8, *t.shape[2:])
            v[:, :, :3] = 0.02 * v[:, :, :3].abs()
            v[:, :, 6:] *= 0.2
    return obj, reg
