"""tests/_up_block_ref.py (the float64 up-block that tests/test_up_block_gpu.py holds model._UpBlockFn to) against float64 autograd of
oracle.mae3d_oracle.UpBlock3D, which is itself pinned to the reference's golden file.  No GPU."""
import pytest
import torch

from oracle import mae3d_oracle as O
from tests import _up_block_ref as U

CASES = [(16, 8, 2, 2, 3), (24, 12, 2, 1, 2)]   # cin, cout, k, B, v


def _case(cin, cout, k, B, v):
    g = torch.Generator().manual_seed(cin + cout + B + v)
    torch.manual_seed(cin * 3 + v)
    blk = O.UpBlock3D(cin, cout, k).double()
    S = k * v
    x = torch.randn(B, cin, v, v, v, generator=g, dtype=torch.float64)
    skip = torch.randn(B, cout, S, S, S, generator=g, dtype=torch.float64)
    dy = torch.randn(B, cout, S, S, S, generator=g, dtype=torch.float64)
    return blk, x, skip, dy


def _oracle(blk, x, skip, dy):
    blk.zero_grad()
    xr, sr = x.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    out = blk(xr, sr)
    out.backward(dy)
    return out.detach(), xr.grad, sr.grad, {n: p.grad.clone() for n, p in blk.named_parameters()}


def _same(a, b, what):
    err = (a - b).abs().max().item()
    assert a.shape == b.shape and err <= 1e-10, f"{what}: {err:.3e}"


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(map(str, c)))
@pytest.mark.parametrize("masks", [None, "own"], ids=["autograd", "own_signs"])
def test_reference_equals_the_oracle_block(case, masks):
    """plain autograd without masks; and with the masks of its own signs (`> 0`, torch's convention for leaky_relu) the masked derivative is the same function"""
    blk, x, skip, dy = _case(*case)
    assert sorted(n for n, _ in blk.named_parameters()) == sorted(U.PARAMS)
    out, dx, dskip, grads = _oracle(blk, x, skip, dy)
    r = U.up_block_grads(x, skip, dict(blk.named_parameters()), case[2], dy, masks=masks)
    _same(r["out"], out, "out")
    _same(r["dx"], dx, "dx")
    _same(r["dskip"], dskip, "dskip")
    for n in U.PARAMS:
        _same(r["grads"][n], grads[n], n)
    if masks == "own":
        assert all(m.dtype == torch.bool and 0 < m.sum() < m.numel() for m in r["masks"])
    for n in ("conv_block.conv1.bias", "conv_block.conv2.bias", "conv_block.conv3.bias"):     # a bias in front of an InstanceNorm
        assert r["grads"][n].abs().max() < 1e-10


@pytest.mark.parametrize("which", [0, 1])
def test_one_flipped_mask_bit_changes_dx(which):
    blk, x, skip, dy = _case(*CASES[0])
    w = dict(blk.named_parameters())
    own = U.up_block_grads(x, skip, w, 2, dy, masks="own")
    masks = [m.clone() for m in own["masks"]]
    masks[which].view(-1)[7] ^= True
    r = U.up_block_grads(x, skip, w, 2, dy, masks=tuple(masks))
    assert torch.equal(r["out"], own["out"]), "the forward does not read the masks"
    assert (r["dx"] - own["dx"]).abs().max() > 1e-6 * own["dx"].abs().max()


def test_the_rounded_chain_is_the_same_function_up_to_rounding():
    """store=float64 rounds nothing: identical results; store=bfloat16 stays within a few bf16 ulps of the exact chain under the same masks"""
    blk, x, skip, dy = _case(*CASES[0])
    bf = lambda t: t.to(torch.bfloat16).double()   # noqa: E731
    x, skip, dy = bf(x), bf(skip), bf(dy)
    w = dict(blk.named_parameters())
    own = U.up_block_grads(x, skip, w, 2, dy, masks="own")
    same = U.up_block_grads(x, skip, w, 2, dy, masks=own["masks"], store=torch.float64)
    assert torch.equal(same["dx"], own["dx"]) and torch.equal(same["out"], own["out"])
    r = U.up_block_grads(x, skip, w, 2, dy, masks=own["masks"], store=torch.bfloat16)
    for n in ("out", "dx", "dskip"):
        e = ((r[n] - own[n]).norm() / own[n].norm()).item()
        assert 1e-4 < e < 3e-2, (n, e)
        assert torch.equal(bf(r[n]), r[n]), f"{n} is stored in bf16"
