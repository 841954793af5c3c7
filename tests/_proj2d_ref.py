"""Float64 restatement of the 2-D projection regression loss (nerf_mae_amd.proj2d over csrc/proj2d.hip, and its place in the fused RPN and FCOS losses),
written from the semantics stated in the header of csrc/proj2d.hpp: the four cameras, the two points of a box, the projection, the row term T and the two
forms that the detectors take of it.  Plain torch on the CPU, differentiable by autograd; the decodes are tests/_rpn_post_ref's and tests/_fcos_ref's.
tests/test_proj2d_ref_cpu.py checks it against tests/golden/g30_proj2d.npz, recorded from the reference's own functions by tools/gen_golden_proj2d.py; the
GPU tests are measured against it.

The row generator (`make_rows`) is part of the restatement, so that the fixture stores seeds and results, not inputs.  It plants three groups and one row:
  far     the corners of prediction and target 0.5 .. 4 voxels apart: all 16 summands of T on the linear branch of the smooth-L1;
  near    prediction = target + 1e-3 res/32 voxels: all 16 on the quadratic branch;
  mixed   both branches in the same row;
  exact   prediction == target: T = 0 and a gradient of exactly 0.
Every row is drawn again until, evaluated in float64 on its fp32 values, it has its branches and no summand lies within 1e-4 beta of the kink."""
import math

import numpy as np
import torch

from tests import _fcos_ref as F
from tests import _rpn_post_ref as P
from tests import _rpn_ref as R

F64 = torch.float64
BETA = 1.0 / 9.0
K = ((600.0, 0.0, 320.0), (0.0, 600.0, 240.0), (0.0, 0.0, 1.0))
FCOS_RES = 160                       # the reference's literal (fcos/loss.py:451, 470)
GROUPS = ("far", "near", "mixed", "exact")
ROW_SEED = 30
N_ROWS = 67                          # 22 far + 22 near + 22 mixed + 1 exact


# ---- cameras, points, projection, term -------------------------------------------------------------------------------------------------------
def w2cs(res):
    """-> float64 [4, 4, 4]: the inverse of [R | pos] for the positions c + (+-res, +-res, res), c = (res/2,)*3, R's columns x, y, z with
    z = normalize(pos - c), x = normalize(cross((0, 0, 1), z)), y = normalize(cross(z, x))"""
    c, up = np.full(3, res / 2.0), np.array([0.0, 0.0, 1.0])
    out = []
    for sx, sy in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        pos = c + np.array([sx * res, sy * res, res], dtype=np.float64)
        z = (pos - c) / np.linalg.norm(pos - c)
        x = np.cross(up, z)
        x = x / np.linalg.norm(x)
        y = np.cross(z, x)
        y = y / np.linalg.norm(y)
        c2w = np.eye(4)
        c2w[:3, :3], c2w[:3, 3] = np.stack([x, y, z], 1), pos
        out.append(np.linalg.inv(c2w))
    return torch.from_numpy(np.stack(out))


def cameras(res):
    """-> float64 [4, 3, 4]: K w2c[:3]"""
    return torch.tensor(K, dtype=F64) @ w2cs(res)[:, :3]


def points(boxes):
    """[n, 6|7] -> [2, n, 3]"""
    if boxes.shape[1] == 6:
        return torch.stack([boxes[:, :3], boxes[:, 3:]])
    w, l, h, cs, sn = boxes[:, 3] / 2, boxes[:, 4] / 2, boxes[:, 5] / 2, torch.cos(boxes[:, 6]), torch.sin(boxes[:, 6])
    v = torch.stack([w * cs - l * sn, w * sn + l * cs, h], 1)
    return torch.stack([boxes[:, :3] - v, boxes[:, :3] + v])


def project(cams, pts):
    """cams [4, 3, 4], pts [..., 3] -> pixel coordinates [4, ..., 2]; no clamp and no sign test on the depth"""
    h = torch.cat([pts, torch.ones_like(pts[..., :1])], -1)
    pic = torch.einsum("cij,...j->c...i", cams.to(pts.dtype), h)
    return pic[..., :2] / pic[..., 2:]


def smooth_l1(d, beta=BETA):
    a = d.abs()
    return torch.where(a < beta, 0.5 * d * d / beta, a - 0.5 * beta)


def differences(pred, target, res, cams=None):
    """-> [n, 16]: uv_pred - uv_target over (camera, point, coordinate); cams: float64 [4, 3, 4] in place of cameras(res)"""
    cams = cameras(res) if cams is None else cams
    d = project(cams, points(pred)) - project(cams, points(target))              # [4, 2, n, 2]
    return d.permute(2, 0, 1, 3).reshape(pred.shape[0], 16)


def terms(pred, target, res, cams=None):
    """pred, target [n, 6|7] float64 -> T [n]"""
    return smooth_l1(differences(pred, target, res, cams)).sum(1)


# ---- the two detectors' forms ----------------------------------------------------------------------------------------------------------------
def rpn_loss_2d(obj, reg, flags, matched, boxes, mesh, valid=None, grids=R.GRIDS, base=None):
    """float64 per-level heads, flags [N, n] uint8, matched [N, n], boxes: per scene [k, 6|7] -> sum over the flagged positives of T / P / max(mesh), T between the
    unclipped decode of the positive's deltas and its matched box; P counts every flag == 1, a positive without a box row or in the padding contributes 0;
    0 without a flagged positive"""
    N, n = flags.shape
    rotated = boxes[0].shape[1] == 7
    C = 8 if rotated else 6
    r = R.flatten_heads(obj, reg, C)[1].reshape(N * n, C)
    P_all = int((flags == 1).sum())
    idx, rows = [], []
    for b, k in torch.nonzero(flags == 1).tolist():
        if boxes[b].shape[0] == 0 or (valid is not None and not bool(valid[b, k])):
            continue
        idx.append(b * n + k)
        rows.append(boxes[b][max(int(matched[b, k]), 0)].to(F64))
    if not idx:
        return r.sum() * 0.0
    idx = torch.tensor(idx)
    anc = P.anchors_t(mesh, grids, base).repeat(N, 1)[idx]
    dec = P.decode_obb(r[idx], anc) if rotated else P.decode_aabb(r[idx], anc)
    return terms(dec, torch.stack(rows), max(mesh)).sum() / P_all / max(mesh)


def fcos_reg_2d(reg, asg, weight, world=1):
    """float64 regression heads (list of NCDHW), asg = tests/_fcos_ref.assign(...) -> what the 2-D term adds to reg_loss:
    weight sum_p ct_p T_p / 160 / 16 / (sum ct / world), T between the decodes of prediction and target at location zero under the cameras of res 160"""
    r = F.flatten_heads(reg, reg, reg)[1]
    pos = asg["valid"] & (asg["labels"] > 0)
    if not pos.any():
        return r.sum() * 0.0
    z = torch.zeros((int(pos.sum()), 3), dtype=F64)
    T = terms(F.decode(z, r[pos]), F.decode(z, asg["targets"][pos]), FCOS_RES)
    return weight * (T * asg["ctr"][pos]).sum() / FCOS_RES / 16.0 / (asg["csum"] / world)


# ---- the planted rows ------------------------------------------------------------------------------------------------------------------------
def _target(rng, ncols, res):
    size = rng.uniform(0.1, 0.4, 3) * res
    ctr = size / 2 + rng.uniform(0, 1, 3) * (res - size)
    if ncols == 6:
        return np.concatenate([ctr - size / 2, ctr + size / 2])
    return np.concatenate([ctr, size, [rng.uniform(-math.pi / 2, math.pi / 2)]])


def _offset(rng, t, res, step):
    """a perturbation of the box columns t that moves each of the two corners by `step` voxels (7 columns: up to 4 % more, by a little change of theta)"""
    u = rng.standard_normal((2, 3))
    u = u / np.linalg.norm(u, axis=1, keepdims=True) * step
    if len(t) == 6:
        return u.reshape(6)
    cs, sn, e = math.cos(t[6]), math.sin(t[6]), u[1] - u[0]                   # the corners are centre -+ R(theta) (w, l) / 2
    return np.concatenate([(u[0] + u[1]) / 2, [cs * e[0] + sn * e[1], cs * e[1] - sn * e[0], e[2]], [rng.uniform(-1, 1) * step / (10.0 * res)]])


def branch_ok(group, d):
    """d [16] float64 differences -> the row has the branches of its group and keeps 1e-4 beta from the kink"""
    a = d.abs()
    if group == "exact":
        return bool((a == 0).all())
    if bool(((a - BETA).abs() < 1e-4 * BETA).any()):
        return False
    lin = a >= BETA
    return bool(lin.all()) if group == "far" else (bool((~lin).all()) if group == "near" else bool(lin.any() and (~lin).any()))


def group_sizes(n):
    if n == 1:
        return dict(far=1, near=0, mixed=0, exact=0)
    k = (n - 1) // 3
    return dict(far=n - 1 - 2 * k, near=k, mixed=k, exact=1)


def make_rows(ncols, res, n=N_ROWS, seed=ROW_SEED):
    """-> (pred [n, ncols] fp32, target [n, ncols] fp32, group -> row indices); the rows of a group are contiguous, in the order of GROUPS"""
    rng = np.random.default_rng([seed, ncols, res, n])
    step = {"far": None, "near": 1e-3 * res / 32, "mixed": None, "exact": 0.0}
    px = 600.0 / (math.sqrt(3.0) * res)                       # pixels per voxel near the scene's centre
    pred, target, where, at = [], [], {}, 0
    for group, count in group_sizes(n).items():
        where[group] = list(range(at, at + count))
        at += count
        for _ in range(count):
            for _try in range(10000):
                t = _target(rng, ncols, res).astype(np.float32)
                s = step[group]
                if group == "far":
                    s = rng.uniform(0.5, 4.0) if res < 100 else rng.uniform(1.5, 4.0)
                elif group == "mixed":
                    s = rng.uniform(0.5, 2.5) * BETA / px
                p = (t.astype(np.float64) + _offset(rng, t.astype(np.float64), res, s)).astype(np.float32) if group != "exact" else t.copy()
                d = differences(torch.from_numpy(p[None]).double(), torch.from_numpy(t[None]).double(), res)[0]
                if branch_ok(group, d):
                    break
            else:
                raise AssertionError(f"no {group} row for ncols {ncols}, res {res}")
            pred.append(p)
            target.append(t)
    return torch.from_numpy(np.stack(pred)), torch.from_numpy(np.stack(target)), where


def reference_grad(pred, target, res, upstream=None):
    """float64 terms and d (sum upstream T) / d pred by autograd"""
    p = pred.double().clone().requires_grad_(True)
    T = terms(p, target.double(), res)
    (T if upstream is None else T * upstream.double()).sum().backward()
    return T.detach(), p.grad
