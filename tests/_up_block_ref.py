"""float64 host reference of one decoder up-block (model._UpBlockFn with the skip connection), in plain torch and channels-first layout:

    cat = cat(conv_transpose3d(x, k = s), skip)
    a1  = leaky_relu(instance_norm(conv1(cat)))
    out = leaky_relu(instance_norm(conv2(a1)) + instance_norm(conv3(cat)))          (instance_norm: eps 1e-5, leaky_relu: slope 0.01)

on the fp32 master weights (a dict with the parameter names of model.UpBlock3D / oracle.mae3d_oracle.UpBlock3D).

Derivative masks.  The HIP backward takes lrelu' from the sign of tensors it stored in bf16.  Where a pre-activation lies within rounding of zero that sign may
differ from float64's; either subgradient is right there, but the O(1) difference in one element spreads through the convolutions behind it and cannot be masked
out of a comparison afterwards.  So each LeakyReLU takes an optional boolean mask: the forward is the true leaky_relu, the backward multiplies by 1 where the mask
is set and by 0.01 elsewhere.  The reference then differentiates with the kernel's own sign pattern and every element stays in the comparison.  With no mask it
is plain autograd.

Rounding floor.  `store` (a dtype) rounds, at the point where the HIP chain stores it in that dtype, every tensor of the chain: the packed weights, cat, the conv
outputs y1 / y2 / y3, a1, out, and in the backward the gradients arriving at the same tensors (dy3, dy2, da1, dy1, dcat) and dx.  The difference between the
reference with and without `store`, under the same masks, is the error a correct kernel chain may show: the floor a chain tolerance is derived from."""
import torch
import torch.nn.functional as F

SLOPE, EPS = 0.01, 1e-5
PARAMS = ("transp_conv.weight", "transp_conv.bias", "conv_block.conv1.weight", "conv_block.conv1.bias", "conv_block.conv2.weight", "conv_block.conv2.bias",
          "conv_block.conv3.weight", "conv_block.conv3.bias")


class _MaskedLeakyReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mask):
        ctx.save_for_backward(mask)
        return F.leaky_relu(x, SLOPE)

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        return torch.where(mask, g, g * SLOPE), None


def leaky_relu(x, mask=None):
    return F.leaky_relu(x, SLOPE) if mask is None else _MaskedLeakyReLU.apply(x, mask)


class _Store(torch.autograd.Function):
    """a tensor the chain keeps in `dt`: the value is rounded on the way forward, the gradient that arrives at it on the way back"""

    @staticmethod
    def forward(ctx, x, dt):
        ctx.dt = dt
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g.to(ctx.dt).to(g.dtype), None


class _RoundValue(torch.autograd.Function):
    """a packed weight: rounded on the way forward, its (fp32) gradient is not"""

    @staticmethod
    def forward(ctx, x, dt):
        return x.to(dt).to(x.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def up_block(x, skip, w, k, masks=(None, None), store=None):
    """x (B, Cin, v, v, v), skip (B, Cout, kv, kv, kv), w: float64 tensors by the names in PARAMS -> (out, pre1, pre2), pre1 / pre2 the inputs of the two LeakyReLUs"""
    st = (lambda t: t) if store is None else (lambda t: _Store.apply(t, store))
    rw = (lambda t: t) if store is None else (lambda t: _RoundValue.apply(t, store))
    inorm = lambda t: F.instance_norm(t, eps=EPS)   # noqa: E731
    cat = st(torch.cat((F.conv_transpose3d(x, rw(w["transp_conv.weight"]), w["transp_conv.bias"], stride=k), skip), 1))
    y1 = st(F.conv3d(cat, rw(w["conv_block.conv1.weight"]), w["conv_block.conv1.bias"], padding=1))
    pre1 = inorm(y1)
    a1 = st(leaky_relu(pre1, masks[0]))
    y2 = st(F.conv3d(a1, rw(w["conv_block.conv2.weight"]), w["conv_block.conv2.bias"], padding=1))
    y3 = st(F.conv3d(cat, rw(w["conv_block.conv3.weight"]), w["conv_block.conv3.bias"]))
    pre2 = inorm(y2) + inorm(y3)
    return st(leaky_relu(pre2, masks[1])), pre1, pre2


def up_block_grads(x, skip, w, k, dy, masks=(None, None), store=None):
    """forward and backward of `up_block` in float64 on (copies of) the given tensors.  masks: None, "own" (the reference's own signs, `> 0` as torch differentiates
    leaky_relu) or a pair of boolean tensors.  Returns out, dx, dskip, grads (by parameter name), pre1, pre2 and the masks used."""
    x, skip = x.detach().double().requires_grad_(True), skip.detach().double().requires_grad_(True)
    w = {n: w[n].detach().double().requires_grad_(True) for n in PARAMS}
    if isinstance(masks, str):
        assert masks == "own"
        with torch.no_grad():
            _, p1, p2 = up_block(x, skip, w, k, store=store)
        masks = (p1 > 0, p2 > 0)
    elif masks is None:
        masks = (None, None)
    out, pre1, pre2 = up_block(x, skip, w, k, masks, store)
    out.backward(dy.double())
    dx = x.grad if store is None else x.grad.to(store).double()
    return dict(out=out.detach(), dx=dx, dskip=skip.grad, grads={n: w[n].grad for n in PARAMS}, pre1=pre1.detach(), pre2=pre2.detach(), masks=masks)
