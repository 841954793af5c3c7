"""Float64 torch restatement of the reference's box head RCNN (nerf_rpn/model/detector.py:441-496), written from its semantics: two optional
conv3d(padding 1) + ReLU layers, then the volume flattened in NCDHW order (column c S + s) or averaged over its three axes, then two affine maps ->
(pred_bbox_delta, pred_scores); differentiated by autograd.  Parameters are a dict with the head's state_dict keys.

An optional rounding hook `rnd` (tensor -> tensor, e.g. round_bf16) is applied exactly where nerf_mae_amd.detector.FusedRCNN stores the compute dtype:
  the conv weights, and in the flatten form the two Linear weights (the fp32 biases are not rounded; the mean form multiplies the fp32 mean with the fp32
  master weights), each with the gradient passed straight through to the master;
  the pooled input; each conv's stored output (with bias, before the ReLU: rounding commutes with the ReLU);
  and, in the backward pass, the gradient that arrives at each of those stored tensors (a 0/1 ReLU mask commutes with the rounding).
Everything else (products, sums, the mean over the cells, the loss gradient itself, weight and bias gradients) stays in float64.  rnd=None is the plain head.

Inputs, parameters and cotangents are filled by formula (fill), so that the recorded fixture tests/golden/g32_box_head.npz (tools/gen_golden_box_head.py) need
not store them: it carries their float64 sums."""
import itertools

import numpy as np
import torch
import torch.nn.functional as F

from tests._rpn_head_ref import _Stored, _Weight, max_err, round_bf16  # noqa: F401  (one definition of "stored in the compute dtype" for both heads)

F64 = torch.float64
# the recorded geometry of tests/golden/g32_box_head.npz
G_C, G_M, G_NCLS = 16, 5, 2
G_SIZES = ((3, 3, 3), (2, 3, 1))
G_CONFIGS = tuple(itertools.product((False, True), repeat=3))           # (is_add_layer, is_flatten, is_rotated_bbox)
CONV_GRAD_STRIDE = 16     # the fixture keeps every 16th element of a 3x3x3 weight's gradient
LIN_GRAD_STRIDE = 4       # and every 4th of a flattening Linear weight's


def keys(add_layer):
    out = []
    if add_layer:
        for k in (0, 2):
            out += [f"layer.{k}.weight", f"layer.{k}.bias"]
    return out + ["RCNN_bbox_pred.weight", "RCNN_bbox_pred.bias", "RCNN_cls_score.weight", "RCNN_cls_score.bias"]


def shapes(C, size, ncls, add_layer, flatten, rotated):
    S = size[0] * size[1] * size[2]
    width, reg = (C * S if flatten else C), (7 if rotated else 6)
    s = {}
    if add_layer:
        for k in (0, 2):
            s[f"layer.{k}.weight"], s[f"layer.{k}.bias"] = (C, C, 3, 3, 3), (C,)
    s["RCNN_bbox_pred.weight"], s["RCNN_bbox_pred.bias"] = (reg, width), (reg,)
    s["RCNN_cls_score.weight"], s["RCNN_cls_score.bias"] = (ncls, width), (ncls,)
    return s


def fill(shape, tag, scale=1.0, zeros=False):
    """float64 tensor of fp32-representable values scale * sin(0.7311 i + 1.37 tag + 0.21), i the flat index: signs alternate irregularly; with zeros every
    element whose index is a multiple of 11 (shifted by tag) is exactly 0"""
    n = int(np.prod(shape))
    i = torch.arange(n, dtype=F64)
    v = torch.sin(i * 0.7311 + 1.37 * tag + 0.21) * scale
    if zeros:
        v[(torch.arange(n) + tag) % 11 == 0] = 0.0
    return v.reshape(shape).float().double()


def make_params(tag, C, size, ncls, add_layer, flatten, rotated):
    """conv weights at sqrt(2 / fan-in)-like scale so that activations stay of order one through the ReLUs; Linear weights at 1 / sqrt(width); biases non-zero"""
    P = {}
    for j, (k, s) in enumerate(shapes(C, size, ncls, add_layer, flatten, rotated).items()):
        if k.endswith("bias"):
            scale = 0.1 if k.startswith("layer.") else 0.5
        elif k.startswith("layer."):
            scale = 2.0 * (2.0 / (C * 27)) ** 0.5
        else:
            scale = 2.0 / s[1] ** 0.5
        P[k] = fill(s, 10 * tag + j, scale)
    return P


def make_case(tag, M, C, size, ncls, add_layer, flatten, rotated):
    """-> (x [M, C, *size] with exact zeros and negatives, P, cot_box [M, 6|7], cot_cls [M, ncls]), all float64 holding fp32 values"""
    x = fill((M, C, *size), 1000 + tag, 1.0, zeros=True)
    P = make_params(tag, C, size, ncls, add_layer, flatten, rotated)
    return x, P, fill((M, 7 if rotated else 6), 2000 + tag), fill((M, ncls), 3000 + tag)


def random_case(seed, M, C, size, ncls, add_layer, flatten, rotated):
    """make_case with normal draws in place of the formula (the GPU tests' cases: independent values keep few pre-activations near a ReLU's kink)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((M, C, *size), generator=g)
    x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
    P = {}
    for k, s in shapes(C, size, ncls, add_layer, flatten, rotated).items():
        scale = (0.1 if k.startswith("layer.") else 0.5) if k.endswith("bias") else (2.0 / (C * 27)) ** 0.5 if k.startswith("layer.") else 1.0 / s[1] ** 0.5
        P[k] = (torch.randn(s, generator=g) * scale).double()
    return x.double(), P, torch.randn((M, 7 if rotated else 6), generator=g).double(), torch.randn((M, ncls), generator=g).double()


def head(x, P, add_layer, flatten, rnd=None):
    """x: float64 (M, C, ow, oh, od) -> (pred_bbox_delta, pred_scores)"""
    st = (lambda v: v) if rnd is None else (lambda v: _Stored.apply(v, rnd))
    w = (lambda v: v) if rnd is None else (lambda v: _Weight.apply(v, rnd))
    h = st(x)
    if add_layer:
        for k in (0, 2):
            h = F.relu(st(F.conv3d(h, w(P[f"layer.{k}.weight"]), P[f"layer.{k}.bias"], padding=1)))
    if flatten:
        v, wl = h.reshape(h.shape[0], -1), w
    else:
        v, wl = h.mean((-1, -2, -3)), (lambda t: t)
    return v @ wl(P["RCNN_bbox_pred.weight"]).T + P["RCNN_bbox_pred.bias"], v @ wl(P["RCNN_cls_score.weight"]).T + P["RCNN_cls_score.bias"]


def run(x, P, add_layer, flatten, cot_box, cot_cls, rnd=None):
    """forward and the gradients of sum(output * cotangent) -> dict(box, cls, dx, dparam); a None cotangent leaves its output out of the sum"""
    x = x.detach().clone().requires_grad_(True)
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    box, cls = head(x, P, add_layer, flatten, rnd)
    total = sum((o * c).sum() for o, c in ((box, cot_box), (cls, cot_cls)) if c is not None)
    total.backward()
    return dict(box=box.detach(), cls=cls.detach(), dx=x.grad, dparam={k: v.grad for k, v in P.items()})


def quantities(res):
    out = {"pred_bbox_delta": res["box"], "pred_scores": res["cls"], "d pooled": res["dx"]}
    out.update({f"d {k}": v for k, v in res["dparam"].items()})
    return out


def recorded_view(k, grad, flatten):
    """the part of parameter k's gradient that the fixture holds"""
    if k.startswith("layer.") and k.endswith("weight"):
        return grad.reshape(-1)[::CONV_GRAD_STRIDE]
    if flatten and k.endswith("weight"):
        return grad.reshape(-1)[::LIN_GRAD_STRIDE]
    return grad


def golden_prefix(size, add_layer, flatten, rotated):
    return f"s{''.join(map(str, size))}_{'c' if add_layer else 'n'}{'f' if flatten else 'm'}{'r' if rotated else 'a'}_"


def golden_tag(size, add_layer, flatten, rotated):
    return 32 + 8 * G_SIZES.index(tuple(size)) + 4 * add_layer + 2 * flatten + rotated


def golden_case(size, add_layer, flatten, rotated):
    return make_case(golden_tag(size, add_layer, flatten, rotated), G_M, G_C, size, G_NCLS, add_layer, flatten, rotated)


def input_sums(x, P, cot_box, cot_cls):
    return np.array([x.sum().item(), cot_box.sum().item(), cot_cls.sum().item(), *[v.sum().item() for v in P.values()]], dtype=np.float64)


def as_np(x):
    return np.ascontiguousarray(x.detach().cpu().numpy())
