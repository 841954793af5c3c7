"""float64 host references for tests/test_conv_layer_gpu.py: the biased 3x3x3 layer and the FPN glue, in plain torch.

Every function takes tensors that already hold storage-dtype values (rounded by `q`) and computes in float64.  The convolution layouts
are NCDHW here; `cl` / `ncdhw` move to and from the channels-last layout of the kernels.  The packed weight orders are restated from
include/nerfmae_hip.h: forward [Cout][27][Cin], input gradient [Cin][27 flipped][Cout]."""
import functools

import torch
import torch.nn.functional as F


def q(t, dt):
    """round to the storage dtype (so the reference sees the same inputs), back to fp32 on the host"""
    return t.to(dt).float()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def cl(t):
    """NCDHW -> channels-last (B, D, H, W, C), contiguous"""
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def pack_fwd(w):
    """[Cout][Cin][3][3][3] -> [Cout][27][Cin]"""
    Co, Ci = w.shape[:2]
    return w.reshape(Co, Ci, 27).permute(0, 2, 1).contiguous()


def pack_dgrad(w):
    """[Cout][Cin][3][3][3] -> [Cin][27 flipped][Cout]"""
    Co, Ci = w.shape[:2]
    return w.reshape(Co, Ci, 27).flip(2).permute(1, 2, 0).contiguous()


@functools.lru_cache(maxsize=16)
def conv_case(dt, B, D, H, W, Cin, Cout, grads=True):
    """storage-dtype inputs of one layer call (x, w, dy NCDHW fp32 holding dt values; bias fp32, non-zero in every channel) and the float64
    results: y = conv(x) + bias and, with grads, dx, dw, db (the autograd of F.conv3d)."""
    seed = B * 7 + D * 11 + H * 13 + W * 17 + Cin * 19 + Cout * 23
    x = q(rnd(B, Cin, D, H, W, seed=seed), dt)
    w = q(rnd(Cout, Cin, 3, 3, 3, seed=seed + 1, scale=(27 * Cin) ** -0.5), dt)
    b = rnd(Cout, seed=seed + 2)
    b = torch.where(b.abs() < 0.25, b.sign() * 0.25 + b, b)     # no channel whose bias is near zero
    dy = q(rnd(B, Cout, D, H, W, seed=seed + 3), dt)
    if not grads:
        return dict(x=x, w=w, b=b, dy=dy, y=F.conv3d(x.double(), w.double(), b.double(), padding=1))
    xr, wr, br = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv3d(xr, wr, br, padding=1)
    y.backward(dy.double())
    return dict(x=x, w=w, b=b, dy=dy, y=y.detach(), dx=xr.grad, dw=wr.grad, db=br.grad)


def upsample_add(coarse, fine):
    """the addend of nearest_upsample_add: coarse upsampled to fine's size by F.interpolate(mode='nearest'), channels-last, in coarse's dtype (a pure copy: the
    detour through fp32 is exact); the caller takes the sum"""
    up = F.interpolate(ncdhw(coarse.float()), size=tuple(fine.shape[1:4]), mode="nearest")
    return cl(up).to(coarse.dtype)


def upsample_adjoint(dfine, coarse_shape):
    """float64 autograd of F.interpolate(mode='nearest', size=fine): the sum of dfine over the fine voxels that read each coarse voxel"""
    c = torch.zeros(coarse_shape, dtype=torch.float64).requires_grad_(True)
    up = F.interpolate(ncdhw(c), size=tuple(dfine.shape[1:4]), mode="nearest")
    up.backward(ncdhw(dfine.double()))
    return c.grad
