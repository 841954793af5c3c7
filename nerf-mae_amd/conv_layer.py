"""The biased 3x3x3 layer of the detector necks and heads (FPN output convs, RPNHead.conv, the FCOS towers): an `nn.Conv3d(Cin, Cout, 3, padding=1)` holder
run on the channels-last kernels.  Which kernels run it and which packed weight layouts they need is decided here alone ("The biased 3x3x3
layer"); the layer's packs are `<key>.w` / `<key>.wd` and, where the 64-channel-block kernel can apply, `<key>.w64` / `<key>.w64d`.  Also `ensure_packed`, the
cache-or-rebuild step in front of every `_Packer` outside model.py."""
from __future__ import annotations

import torch

from . import ops
from .model import _gradbuf, _Packer


def register(P: _Packer, key: str, conv, dtype: torch.dtype):
    """adds the layer's weight layouts to P: forward and input-gradient order of the generic kernel, and those of the LDS-halo kernel on 64-channel blocks
    when it can ever be chosen (ops.use_conv64: bf16, both channel counts multiples of 64)"""
    w = conv.weight
    P.add(f"{key}.w", w, P.CONV_F)
    P.add(f"{key}.wd", w, P.CONV_D)
    if dtype == torch.bfloat16 and w.shape[0] % 64 == 0 and w.shape[1] % 64 == 0:
        P.add(f"{key}.w64", w, P.C64_F)
        P.add(f"{key}.w64d", w, P.C64_D)


def forward(pk: _Packer, key: str, conv, x):
    """x channels-last (B, D, H, W, Cin) -> conv(x) + bias (B, D, H, W, Cout); the bias goes through the kernel's epilogue in both branches"""
    Cout = conv.weight.shape[0]
    if ops.use_conv64(x, Cout) and f"{key}.w64" in pk.views:   # LDS-halo kernel on 64-channel blocks
        return ops.conv3d_k3_c64(x, pk[f"{key}.w64"], Cout, bias=conv.bias)
    return ops.conv3d_k3_bias(x, pk[f"{key}.w"], conv.bias, Cout)


def backward(pk: _Packer, key: str, conv, dy, x, need_dx: bool = True):
    """weight and bias gradients added into the parameters' .grad on the forked side stream, then the input gradient on the current stream (None when the
    layer's input needs none).  Does not join: the caller keeps dy and x referenced until its ops.join_side() (the caching allocator knows nothing of the
    side stream)."""
    Cout, Cin = conv.weight.shape[:2]
    with ops.side_stream():
        ops.conv3d_k3_wgrad(dy, x, _gradbuf(conv.weight))
        ops.bias_grad(dy.view(-1, Cout), _gradbuf(conv.bias), dy.numel() // Cout, Cout)
    if not need_dx:
        return None
    if ops.use_conv64(dy, Cin) and f"{key}.w64d" in pk.views:
        return ops.conv3d_k3_c64(dy, pk[f"{key}.w64d"], Cin)
    return ops.conv3d_k3(dy, pk[f"{key}.wd"], Cin)


def ensure_packed(owner, params, message: str, fill, refresh=None):
    """owner._pk holds the compute-dtype layouts of `params` (owner.compute_dtype): rebuilt by fill(P) on a fresh _Packer when a parameter's storage changed
    (.cuda(), load of a flat buffer), produced from the fp32 masters by one pack launch on every call.  refresh() runs before that launch (masters the owner
    derives itself).  Raises RuntimeError(message) while the parameters are on the host."""
    if not params[0].is_cuda:
        raise RuntimeError(message)
    key = tuple(p.data_ptr() for p in params)
    if owner._pk is None or owner._pk_key != key:
        P = _Packer()
        fill(P)
        P.build(owner.compute_dtype, params[0].device)
        P.split = None
        owner._pk, owner._pk_key = P, key
    if refresh is not None:
        refresh()
    owner._pk.run()
