"""Float64 torch restatement of the reference's RPNHead (nerf_rpn/model/anchor.py:177-213): F.conv3d + ReLU per layer, then the two 1x1x1 convs,
differentiated by autograd.  Parameters are a dict with the head's state_dict keys.

An optional rounding hook `rnd` (tensor -> tensor, e.g. round_bf16) is applied exactly where the HIP path stores the compute dtype:
  the weights (conv, cls_logits, bbox_pred; the fp32 biases are not rounded), with the gradient passed straight through to the master weight;
  the input features; each layer's stored activation (the conv's output with bias, before the ReLU: rounding commutes with the ReLU);
  and, in the backward pass, the gradient that arrives at each of those stored tensors: dt of the output kernel, each layer's stored gradient, and the
  gradient of the input (a 0/1 ReLU mask commutes with the rounding, so rounding after the mask restates "store, then mask in place").
Everything else (products, sums, the loss gradient itself, weight and bias gradients) stays in float64.  rnd=None is the plain float64 head."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
# the recorded geometry of tests/golden/g23_rpn_head.npz (tools/gen_golden_rpn_head.py)
G_CIN, G_A, G_N = 16, 2, 2
G_GRIDS = ((3, 2, 2), (2, 1, 2))
G_CASES = tuple((depth, rotate) for depth in (0, 1, 2) for rotate in (False, True))
G_SEED = 23


def round_bf16(x):
    """round to nearest even to bfloat16, returned in x's dtype"""
    return x.float().bfloat16().to(x.dtype)       # float64 -> fp32 -> bf16: a double rounding only within 2^-29 of a tie, which the tolerances of the tests cover


class _Stored(torch.autograd.Function):
    """a tensor the kernels store in the compute dtype: rounded on the way forward, its gradient rounded on the way back"""

    @staticmethod
    def forward(ctx, x, rnd):
        ctx.rnd = rnd
        return rnd(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.rnd(g), None


class _Weight(torch.autograd.Function):
    """a packed weight: rounded forward, gradient straight through to the fp32 master"""

    @staticmethod
    def forward(ctx, w, rnd):
        return rnd(w)

    @staticmethod
    def backward(ctx, g):
        return g, None


def keys(depth):
    out = []
    for k in range(depth):
        out += [f"conv.{2 * k}.weight", f"conv.{2 * k}.bias"]
    return out + ["cls_logits.weight", "cls_logits.bias", "bbox_pred.weight", "bbox_pred.bias"]


def shapes(depth, Cin, A, C):
    s = {}
    for k in range(depth):
        s[f"conv.{2 * k}.weight"], s[f"conv.{2 * k}.bias"] = (Cin, Cin, 3, 3, 3), (Cin,)
    s["cls_logits.weight"], s["cls_logits.bias"] = (A, Cin, 1, 1, 1), (A,)
    s["bbox_pred.weight"], s["bbox_pred.bias"] = (A * C, Cin, 1, 1, 1), (A * C,)
    return s


def make_params(seed, depth, Cin, A, C, std=0.2):
    """float64 parameters (fp32-representable): 3x3x3 weights at the scale that keeps activations of order one through the ReLUs (sqrt(2 / fan-in)), 1x1x1 weights
    at `std`, biases non-zero so that they are tested"""
    g = torch.Generator().manual_seed(seed)
    scale = lambda k: (2.0 / (Cin * 27)) ** 0.5 if k.startswith("conv.") and k.endswith("weight") else std if k.endswith("weight") else 0.5 if not k.startswith("conv.") else 0.1
    return {k: (torch.randn(s, generator=g) * scale(k)).double() for k, s in shapes(depth, Cin, A, C).items()}


def make_features(seed, N, Cin, grids):
    """float64 NCDHW features with exact zeros and negatives"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for grid in grids:
        x = torch.randn((N, Cin, *grid), generator=g)
        x[torch.rand(x.shape, generator=g) < 0.1] = 0.0
        out.append(x.double())
    return out


def output_stage(t, P, relu, rnd=None):
    """t: NCDHW float64 (the last conv's output before its ReLU) -> (objectness, pred_bbox_deltas)"""
    w = (lambda v: v) if rnd is None else (lambda v: _Weight.apply(v, rnd))
    a = F.relu(t) if relu else t
    return F.conv3d(a, w(P["cls_logits.weight"]), P["cls_logits.bias"]), F.conv3d(a, w(P["bbox_pred.weight"]), P["bbox_pred.bias"])


def head(feats, P, depth, rnd=None):
    """feats: list of float64 NCDHW tensors -> (logits, bbox_reg), lists per level"""
    st = (lambda v: v) if rnd is None else (lambda v: _Stored.apply(v, rnd))
    w = (lambda v: v) if rnd is None else (lambda v: _Weight.apply(v, rnd))
    logits, bbox_reg = [], []
    for f in feats:
        x = st(f)
        for k in range(depth):
            x = st(F.conv3d(x, w(P[f"conv.{2 * k}.weight"]), P[f"conv.{2 * k}.bias"], padding=1))
            if k < depth - 1:
                x = F.relu(x)
        o, r = output_stage(x, P, depth > 0, rnd)
        logits.append(o)
        bbox_reg.append(r)
    return logits, bbox_reg


def run(feats, P, depth, cot_obj, cot_reg, rnd=None):
    """forward and the gradients of sum(output * cotangent) -> dict(obj, reg, dfeat: lists; dparam: dict)"""
    feats = [f.detach().clone().requires_grad_(True) for f in feats]
    P = {k: v.detach().clone().requires_grad_(True) for k, v in P.items()}
    obj, reg = head(feats, P, depth, rnd)
    total = sum((o * c).sum() for o, c in zip(obj, cot_obj)) + sum((r * c).sum() for r, c in zip(reg, cot_reg))
    total.backward()
    return dict(obj=[o.detach() for o in obj], reg=[r.detach() for r in reg], dfeat=[f.grad for f in feats], dparam={k: v.grad for k, v in P.items()})


def max_err(a, b):
    """max-norm error of a against b relative to max |b| (lists are compared tensor by tensor, the largest is returned)"""
    if isinstance(a, (list, tuple)):
        return max(max_err(x, y) for x, y in zip(a, b))
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-300)).item()


CONV_GRAD_STRIDE = 32     # the fixture keeps every 32nd element of a 3x3x3 weight's gradient


def golden_params(g, depth, rotate):
    r = "r" if rotate else "a"
    return {k: torch.from_numpy(g[k if k.startswith("conv.") else f"{r}_{k}"].astype(np.float64)) for k in keys(depth)}


def golden_case(g, depth, rotate):
    """the recorded case (depth, rotate) of g23_rpn_head.npz -> (feats, P, cot_obj, cot_reg, recorded results dict).  The 3x3x3 weights (fp16-exact) and
    biases are shared by all cases, the 1x1x1 parameters by the cases of one box type; recorded conv-weight gradients are the elements [::CONV_GRAD_STRIDE]."""
    pre = f"d{depth}{'r' if rotate else 'a'}_"
    L = len(G_GRIDS)
    feats = [torch.from_numpy(g[f"x{i}"].astype(np.float64)) for i in range(L)]
    P = golden_params(g, depth, rotate)
    cot_obj = [torch.from_numpy(g[f"{pre}cot_obj{i}"].astype(np.float64)) for i in range(L)]
    cot_reg = [torch.from_numpy(g[f"{pre}cot_reg{i}"].astype(np.float64)) for i in range(L)]
    rec = dict(obj=[torch.from_numpy(g[f"{pre}obj{i}"]) for i in range(L)], reg=[torch.from_numpy(g[f"{pre}reg{i}"]) for i in range(L)],
               dfeat=[torch.from_numpy(g[f"{pre}dx{i}"]) for i in range(L)], dparam={k: torch.from_numpy(g[f"{pre}d_{k}"]) for k in keys(depth)})
    return feats, P, cot_obj, cot_reg, rec


def recorded_view(k, grad):
    """the part of parameter k's gradient that the fixture holds"""
    return grad.reshape(-1)[::CONV_GRAD_STRIDE] if k.startswith("conv.") and k.endswith("weight") else grad


def as_np(x):
    return np.ascontiguousarray(x.detach().cpu().numpy())
