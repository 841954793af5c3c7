"""Float64 torch restatement of the reference's FCOSHead (nerf_rpn/model/fcos/fcos.py:26-139): per tower num_convs x (F.conv3d 3^3 -> explicit GroupNorm(32) ->
ReLU), then cls_logits, bbox_pred and centerness (F.conv3d 3^3), the Scale, the column-wise ReLU, the stride of the evaluation mode or the exp, differentiated by
autograd.  Parameters are a dict with the head's state_dict keys.

An optional rounding hook `rnd` (tensor -> tensor, e.g. round_bf16) is applied exactly where the HIP path stores the compute dtype:
  the convolution weights (towers and output convs; biases, GroupNorm affine parameters and Scales stay fp32), gradient straight through to the master weight;
  the input features; each layer's convolution output x (the statistics are taken from the stored x) and its normalised, rectified y;
  and, in the backward pass, the gradient that arrives at each of those stored tensors: the gradient of y (the next convolution's input gradient), of x (the
  GroupNorm backward's result), of each tower's input (stored per tower, then the two are added and stored as the features' gradient), and the 16-column
  gradient of the output convs as their INPUT-gradient convolution reads it (their weight gradients read it unrounded: hi + lo in the kernels).
Everything else (products, sums, statistics, parameter gradients) stays in float64.  rnd=None is the plain float64 head."""
import numpy as np
import torch
import torch.nn.functional as F

from tests._rpn_head_ref import _Stored, _Weight, as_np, max_err, round_bf16  # noqa: F401

F64 = torch.float64
GROUPS, EPS = 32, 1e-5
# the recorded geometry of tests/golden/g24_fcos_head.npz (tools/gen_golden_fcos_head.py)
G_C, G_CONVS, G_N = 64, 1, 2
G_GRIDS = ((3, 2, 2), (2, 1, 2))
G_STRIDES = (4, 8)
G_SCALES = (1.25, -0.75)
#          use_obb, centerness_on_reg, training
G_CASES = ((False, True, True), (True, False, True), (True, True, False), (False, False, False))
G_SEED = 24
TOWER_GRAD_STRIDE, OUT_GRAD_STRIDE = 64, 8     # the fixture keeps every 64th element of a tower weight's gradient and every 8th of an output weight's


class _OutConv(torch.autograd.Function):
    """an output convolution whose input gradient reads the stored (rounded) output gradient and whose weight gradient reads the unrounded one"""

    @staticmethod
    def forward(ctx, a, w, b, rnd):
        ctx.save_for_backward(a, w)
        ctx.rnd = rnd
        return F.conv3d(a, w, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        a, w = ctx.saved_tensors
        return (torch.nn.grad.conv3d_input(a.shape, w, ctx.rnd(g), padding=1), torch.nn.grad.conv3d_weight(a, w.shape, g, padding=1), g.sum((0, 2, 3, 4)), None)


def keys(num_convs):
    out = []
    for t in ("cls_tower", "bbox_tower"):
        for k in range(num_convs):
            out += [f"{t}.{3 * k}.weight", f"{t}.{3 * k}.bias", f"{t}.{3 * k + 1}.weight", f"{t}.{3 * k + 1}.bias"]
    out += ["cls_logits.weight", "cls_logits.bias", "bbox_pred.weight", "bbox_pred.bias", "centerness.weight", "centerness.bias"]
    return out + [f"scales.{i}.scale" for i in range(5)]


def shapes(num_convs, C, nreg):
    s = {}
    for t in ("cls_tower", "bbox_tower"):
        for k in range(num_convs):
            s[f"{t}.{3 * k}.weight"], s[f"{t}.{3 * k}.bias"] = (C, C, 3, 3, 3), (C,)
            s[f"{t}.{3 * k + 1}.weight"], s[f"{t}.{3 * k + 1}.bias"] = (C,), (C,)
    for name, n in (("cls_logits", 1), ("bbox_pred", nreg), ("centerness", 1)):
        s[f"{name}.weight"], s[f"{name}.bias"] = (n, C, 3, 3, 3), (n,)
    for i in range(5):
        s[f"scales.{i}.scale"] = (1,)
    return s


def make_params(seed, num_convs, C, nreg, scales=(1.25, -0.75, 0.5, 1.5, 1.0)):
    """float64 parameters (fp32-representable): 3^3 weights at sqrt(2 / fan-in) so that activations stay of order one, GroupNorm gamma around 1 with both signs of
    beta, non-zero biases, non-unit Scales with one negative"""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for k, s in shapes(num_convs, C, nreg).items():
        if k.startswith("scales."):
            P[k] = torch.tensor([scales[int(k.split(".")[1])]]).double()
        elif "tower" in k and int(k.split(".")[1]) % 3 == 1:
            P[k] = ((1.0 + 0.3 * torch.randn(s, generator=g)) if k.endswith("weight") else 0.4 * torch.randn(s, generator=g)).float().double()
        elif k.endswith("weight"):
            P[k] = (torch.randn(s, generator=g) * (2.0 / (C * 27)) ** 0.5).float().double()
        else:
            P[k] = (torch.randn(s, generator=g) * (0.1 if "tower" in k else 0.5)).float().double()
    return P


def make_features(seed, N, C, grids):
    """float64 NCDHW features with exact zeros and negatives"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for grid in grids:
        x = torch.randn((N, C, *grid), generator=g)
        x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
        out.append(x.double())
    return out


def group_norm(x, gamma, beta, groups=GROUPS, eps=EPS):
    """nn.GroupNorm on NCDHW, written out: biased variance over (channels of the group, voxels), eps inside the root, per-channel affine"""
    N, C = x.shape[:2]
    xg = x.reshape(N, groups, -1)
    mean = xg.mean(dim=2, keepdim=True)
    var = ((xg - mean) ** 2).mean(dim=2, keepdim=True)
    xh = ((xg - mean) / torch.sqrt(var + eps)).reshape(x.shape)
    return xh * gamma.view(1, C, 1, 1, 1) + beta.view(1, C, 1, 1, 1)


def epilogue(u, scale, mode, stride):
    """fcos.py:123-137 on u = bbox_pred(tower) with its bias"""
    z = u * scale
    if mode == "exp":
        return torch.exp(z)
    lo = F.relu(z[:, :6])
    if mode == "eval":
        lo = lo * stride
    return torch.cat([lo, z[:, 6:]], dim=1)


def output_stage(a_cls, a_box, P, level, ctr_on_reg, mode, stride, rnd=None):
    """a_cls, a_box: NCDHW float64 inputs of the output convs (each tower's last activation) -> (logits, bbox_reg, centerness) of one level"""
    w = (lambda v: v) if rnd is None else (lambda v: _Weight.apply(v, rnd))
    r = (lambda v: v) if rnd is None else rnd
    conv = lambda a, name: _OutConv.apply(a, w(P[f"{name}.weight"]), P[f"{name}.bias"], r)
    cls = conv(a_cls, "cls_logits")
    ctr = conv(a_box if ctr_on_reg else a_cls, "centerness")
    reg = epilogue(conv(a_box, "bbox_pred"), P[f"scales.{level}.scale"], mode, stride)
    return cls, reg, ctr


def head(feats, P, num_convs, ctr_on_reg, mode, strides, rnd=None, groups=GROUPS):
    """feats: list of float64 NCDHW tensors -> (logits, bbox_reg, centerness), lists per level"""
    st = (lambda v: v) if rnd is None else (lambda v: _Stored.apply(v, rnd))
    w = (lambda v: v) if rnd is None else (lambda v: _Weight.apply(v, rnd))
    out = ([], [], [])
    for level, f in enumerate(feats):
        xin = st(f)
        last = []
        for t in ("cls_tower", "bbox_tower"):
            a = st(xin)             # each tower's input gradient is stored on its own before the two are added
            for k in range(num_convs):
                x = st(F.conv3d(a, w(P[f"{t}.{3 * k}.weight"]), P[f"{t}.{3 * k}.bias"], padding=1))
                a = st(F.relu(group_norm(x, P[f"{t}.{3 * k + 1}.weight"], P[f"{t}.{3 * k + 1}.bias"], groups)))
            last.append(a)
        for o, v in zip(out, output_stage(last[0], last[1], P, level, ctr_on_reg, mode, strides[level], rnd)):
            o.append(v)
    return out


def run(feats, P, num_convs, ctr_on_reg, mode, strides, cots, rnd=None, groups=GROUPS):
    """forward and the gradients of sum(output * cotangent); cots = (cot_cls, cot_reg, cot_ctr) -> dict(cls, reg, ctr, dfeat: lists; dparam: dict)"""
    feats = [f.detach().clone().requires_grad_(True) for f in feats]
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    outs = head(feats, P, num_convs, ctr_on_reg, mode, strides, rnd, groups)
    sum((o * c).sum() for os_, cs in zip(outs, cots) for o, c in zip(os_, cs)).backward()
    L = len(feats)
    dparam = {k: (v.grad if v.grad is not None else torch.zeros_like(v)) for k, v in P.items() if not k.startswith("scales.") or int(k.split(".")[1]) < L}
    return dict(cls=[o.detach() for o in outs[0]], reg=[o.detach() for o in outs[1]], ctr=[o.detach() for o in outs[2]], dfeat=[f.grad for f in feats], dparam=dparam)


# ---- the fixture ---------------------------------------------------------------------------------------------------------------------------------
def bf16_bits(x):
    """bf16-exact float tensor -> its 16 bits as a numpy uint16 array"""
    return (x.detach().float().contiguous().view(torch.int32) >> 16).to(torch.int16).numpy().view(np.uint16)


def from_bf16_bits(a):
    return torch.from_numpy((a.astype(np.uint32) << 16).view(np.float32).astype(np.float64))


def case_prefix(use_obb, ctr_on_reg, training):
    return f"{'o' if use_obb else 'a'}{'r' if ctr_on_reg else 'c'}{'t' if training else 'e'}_"


def golden_params(g, use_obb):
    box = "o" if use_obb else "a"
    P = {}
    for k in keys(G_CONVS):
        name = f"{box}_{k}" if k.startswith("bbox_pred") else k
        P[k] = from_bf16_bits(g[name]) if g[name].dtype == np.uint16 else torch.from_numpy(g[name].astype(np.float64))
    return P


def recorded_view(k, grad):
    """the part of parameter k's gradient that the fixture holds"""
    if k.endswith("weight") and grad.dim() == 5:
        return grad.reshape(-1)[::TOWER_GRAD_STRIDE if "tower" in k else OUT_GRAD_STRIDE]
    return grad


def golden_case(g, use_obb, ctr_on_reg, training):
    """-> (feats, P, cots, mode, recorded results dict) of one recorded case"""
    pre, L = case_prefix(use_obb, ctr_on_reg, training), len(G_GRIDS)
    feats = [torch.from_numpy(g[f"x{i}"].astype(np.float64)) for i in range(L)]
    P = golden_params(g, use_obb)
    cots = tuple([torch.from_numpy(g[f"{pre}cot_{n}{i}"].astype(np.float64)) for i in range(L)] for n in ("cls", "reg", "ctr"))
    rec = {n: [torch.from_numpy(g[f"{pre}{n}{i}"]) for i in range(L)] for n in ("cls", "reg", "ctr")}
    rec["dfeat"] = [torch.from_numpy(g[f"{pre}dx{i}"]) for i in range(L)]
    rec["dparam"] = {k: torch.from_numpy(g[f"{pre}d_{k}"]) for k in keys(G_CONVS) if not k.startswith("scales.") or int(k.split(".")[1]) < L}
    return feats, P, cots, "train" if training else "eval", rec
