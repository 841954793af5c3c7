"""The decoder's mid-level up-blocks (decoder4 / decoder3 / decoder2: model._UpBlockFn with the skip connection and the 1x1 projection branch) against the
float64 up-block of tests/_up_block_ref.py, once per conv family (`c48mb`, `c64`, `generic`) and per weight-gradient route (the weight-gradient queue, the
forked side stream, the main stream of the 64-block kernels).

Each case builds the smallest model that packs the family's layouts (depths [1, 1, 1, 1]; ops.C48MB_MIN_VOXELS / ops.C64_MIN_VOXELS patched before
construction: 1 packs and plans the family, 0 disables it), calls the block module on storage-dtype inputs and back-propagates a random cotangent.  Which
kernels ran is asserted, not assumed: the plan (family, defer_conv_wgrad, defer_upconv_wgrad) before the call, the C entry points through a spy on the
library's call() and the closures handed to WgradQueue.defer after it.

The reference differentiates its two LeakyReLUs with the kernel's own sign pattern (`a1 > 0`, `out > 0` on the function's saved tensors): see
tests/_up_block_ref.py.  That a sign differs from float64's only where it may is asserted separately (`_assert_flips_are_near_zero`).

Tolerances.  Everything is held by tests/_metrics.assert_close to the project's TOL (3e-2 bf16, 2e-4 fp32), or, where the rounding of the bf16 chain itself
leaves no room for that, to 2 x the measured floor: the error of the SAME float64 reference, under the same masks, with every tensor the HIP chain stores in
bf16 rounded at that point (`store=torch.bfloat16`), expressed as the smallest rtol at which assert_close passes (`needed_rtol`).  Floors and the errors of
the HIP chain are tabulated at FLOOR."""
import collections
import os

import pytest
import torch

from tests import _up_block_ref as U
from tests._metrics import assert_close, rel_l2, relerr

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
TOL = {F32: 2e-4, BF16: 3e-2}
HALO48, HALO64, IGEMM = "nmh_conv3d_k3_wgrad_halo", "nmh_conv3d_k3_c64_wgrad", "nmh_conv3d_k3_wgrad"
CONV = {"c48mb": "nmh_conv3d_k3_c48mb", "c64": "nmh_conv3d_k3_c64", "generic": "nmh_conv3d_k3"}
HEADS = {96: [3, 6, 12, 24], 128: [4, 8, 16, 32]}

Case = collections.namedtuple("Case", "name embed block dt B v family queue wgrad")
CASES = [
    # 18^3 = 5832 voxels: ragged on every axis of the 4x4x16 tile and >= 4096, so the halo weight gradients run in channel sub-problem mode (8 and 4 sub-problems)
    Case("dec2-c48mb-queue", 96, "decoder2", BF16, 2, 9, "c48mb", True, HALO48),
    Case("dec2-c48mb-side", 96, "decoder2", BF16, 2, 9, "c48mb", False, HALO48),
    Case("dec2-generic-queue", 96, "decoder2", BF16, 2, 9, "generic", True, HALO48),
    Case("dec3-c48mb-queue", 96, "decoder3", BF16, 1, 3, "c48mb", True, IGEMM),       # 6^3
    Case("dec4-c48mb-queue", 96, "decoder4", BF16, 1, 2, "c48mb", True, IGEMM),       # 4^3
    Case("dec2-c64-queue", 128, "decoder2", BF16, 2, 9, "c64", True, HALO64),         # conv weight gradients stay on the main stream by plan
    Case("dec3-c64-side", 128, "decoder3", BF16, 1, 3, "c64", False, IGEMM),
    Case("dec2-fp32-side", 96, "decoder2", F32, 2, 5, "generic", False, IGEMM),       # 10^3, no queue
    Case("dec2-fp32-queue", 96, "decoder2", F32, 2, 5, "generic", True, IGEMM),       # as the model runs it: the closures go through the queue in fp32 too
]

# FLOOR[(embed_dim, block)]: needed_rtol of the bf16-rounded float64 chain (store=torch.bfloat16) against the exact one -- same masks (the exact chain's own
# signs), same inputs and weights as the cases below, worst sample; measured on the host, no kernel involved.  A bf16 chain quantity is held to
# max(TOL, 2 x floor): TOL where the chain's own rounding leaves room for it, twice the floor where it does not (the elementwise measure is a maximum over up to
# 10^6 entries of an error whose rms is about 1e-2 of the tensor's: the floor of `out` at 18^3 is 2.2e-2 by itself).  HIP: needed_rtol of the HIP chain on an
# MI355X, for comparison -- it sits at the floor everywhere (0.8 x ... 1.7 x), i.e. the chain adds no error of its own beyond its bf16 stores.
QUANTITIES = ("out", "dx", "dskip", "transp_conv.weight", "transp_conv.bias", "conv_block.conv1.weight", "conv_block.conv2.weight", "conv_block.conv3.weight")
FLOOR = {
    #                 out      dx       dskip    t.weight t.bias   c1.weight c2.weight c3.weight
    (96, "decoder2"):  (2.20e-2, 1.52e-2, 1.53e-2, 1.31e-2, 2.51e-2, 1.80e-2, 1.49e-2, 6.93e-3),
    (96, "decoder3"):  (1.61e-2, 1.42e-2, 1.19e-2, 1.96e-2, 1.53e-2, 2.19e-2, 2.02e-2, 8.95e-3),
    (96, "decoder4"):  (1.89e-2, 1.44e-2, 1.35e-2, 2.29e-2, 1.91e-2, 2.70e-2, 3.17e-2, 1.29e-2),
    (128, "decoder2"): (2.47e-2, 1.52e-2, 1.46e-2, 1.54e-2, 4.19e-2, 1.85e-2, 1.75e-2, 7.15e-3),
    (128, "decoder3"): (1.49e-2, 1.41e-2, 1.46e-2, 1.74e-2, 1.76e-2, 2.03e-2, 2.36e-2, 7.77e-3),
}


HIP = {
    #                      out      dx       dskip    t.weight t.bias   c1.weight c2.weight c3.weight
    "dec2-c48mb-queue":   (2.17e-2, 1.91e-2, 1.73e-2, 1.53e-2, 2.90e-2, 1.82e-2, 1.55e-2, 7.61e-3),     # the side-stream route and the second pass: the same figures
    "dec2-generic-queue": (2.17e-2, 1.76e-2, 1.64e-2, 1.41e-2, 4.34e-2, 1.63e-2, 1.59e-2, 7.61e-3),
    "dec3-c48mb-queue":   (1.57e-2, 1.36e-2, 1.41e-2, 2.09e-2, 1.84e-2, 2.11e-2, 1.99e-2, 8.19e-3),
    "dec4-c48mb-queue":   (1.79e-2, 1.19e-2, 1.39e-2, 2.51e-2, 1.61e-2, 3.67e-2, 2.99e-2, 1.03e-2),
    "dec2-c64-queue":     (2.24e-2, 1.62e-2, 1.43e-2, 1.43e-2, 2.16e-2, 1.90e-2, 1.71e-2, 7.28e-3),
    "dec3-c64-side":      (1.57e-2, 1.51e-2, 1.40e-2, 2.07e-2, 1.97e-2, 2.30e-2, 2.35e-2, 9.49e-3),
    "dec2-fp32-*":        (7.6e-6, 4.1e-6, 5.7e-6, 3.7e-6, 8.1e-6, 6.3e-6, 6.1e-6, 2.8e-6),                # against TOL[fp32] = 2e-4
}
# Signs that differ from float64's, measured: 595 of 1.1 M at conv1's LeakyReLU of the 18^3 cases, the farthest at 5.1e-3 rms of the pre-activation; 1181 at the
# output LeakyReLU, the farthest at 1.0e-2 rms (c64: 819 / 5.2e-3 and 1509 / 1.2e-2); fp32: one sign at 2.7e-7 rms.  The bound is TOL.


def chain_tol(case, quantity):
    if case.dt == F32:
        return TOL[F32]       # fp32 stores and fp32 accumulation: no rounding floor near 2e-4
    return max(TOL[BF16], 2 * FLOOR[case.embed, case.block][QUANTITIES.index(quantity)])


def _ops():
    from nerf_mae_amd import ops
    return ops


def needed_rtol(a, b):
    """the smallest rtol at which tests/_metrics.assert_close(a, b, rtol) passes: max of its three measures"""
    a64, b64 = a.detach().double().cpu().flatten(), b.detach().double().cpu().flatten()
    rms = b64.pow(2).mean().sqrt()
    return max(relerr(a, b), rel_l2(a, b), ((a64 - b64).abs() / (b64.abs() + rms)).max().item())


def thresholds(case):
    """(C48MB_MIN_VOXELS, C64_MIN_VOXELS) that make the model pack and plan `case.family`"""
    return {"c48mb": (1, 0), "c64": (0, 1), "generic": (0, 0)}[case.family]


def host_model(case):
    """the model on the host, deterministic: tools that measure the floors build the same weights"""
    from nerf_mae_amd.model import SwinTransformer_MAE3D
    torch.manual_seed(case.embed)
    return SwinTransformer_MAE3D(patch_size=[4] * 3, window_size=[4] * 3, embed_dim=case.embed, depths=[1, 1, 1, 1], num_heads=HEADS[case.embed], resolution=32,
                                 stochastic_depth_prob=0.0, compute_dtype=case.dt)


def problem(case, blk, seed=0):
    """channels-last storage-dtype x (B, v, v, v, Cin), skip and dy (B, S, S, S, Cout) on the host, as fp32 holding `case.dt` values"""
    g = torch.Generator().manual_seed(1000 * seed + case.B * 7 + case.v * 11 + blk.cin)
    S = case.v * blk.k
    r = lambda *s: torch.randn(*s, generator=g).to(case.dt).float()   # noqa: E731
    return r(case.B, case.v, case.v, case.v, blk.cin), r(case.B, S, S, S, blk.cout), r(case.B, S, S, S, blk.cout)


def cf(t):
    """channels-last -> channels-first"""
    return t.permute(0, 4, 1, 2, 3)


def master_weights(blk):
    return {n: p.detach().cpu() for n, p in blk.named_parameters()}


_MODELS = {}     # (embed_dim, dtype, thresholds at construction) -> the model on the device: four models serve the nine cases


@pytest.fixture(scope="module", autouse=True)
def _release_models():
    yield
    _MODELS.clear()
    torch.cuda.empty_cache()


def _device_model(case, monkeypatch):
    ops = _ops()
    c48mb, c64 = thresholds(case)
    monkeypatch.setattr(ops, "C48MB_MIN_VOXELS", c48mb)     # before construction: _build_packer reads them, and the plan reads them again
    monkeypatch.setattr(ops, "C64_MIN_VOXELS", c64)
    key = (case.embed, case.dt, c48mb, c64)
    if key not in _MODELS:
        m = host_model(case).cuda()
        m.train()
        _MODELS[key] = m
    m = _MODELS[key]
    m._ensure_ready(torch.device("cuda"))
    m._packer.join()
    m.zero_grad()
    return m


def _saved(out):
    fn = out.grad_fn
    while not hasattr(fn, "saved"):
        fn = fn.next_functions[0][0]
    return fn.saved


def _run(case, blk, x, skip, dy):
    """one forward + backward of the block module -> out, dx, dskip (channels-last, on the host) and the two derivative masks (channels-first)"""
    ops = _ops()
    arena = ops.AccArena.get(torch.device("cuda", torch.cuda.current_device()))
    if arena is not None:
        arena.begin()                                        # as forward_decoder does in front of the decoder levels
    xg, sg = x.to(case.dt).cuda().requires_grad_(True), skip.to(case.dt).cuda().requires_grad_(True)
    out = blk(xg, sg)
    S, C = case.v * blk.k, blk.cout
    a1, o = _saved(out)[4], _saved(out)[9]
    assert a1.shape == o.shape == (case.B * S ** 3, C)
    masks = tuple(cf((t > 0).view(case.B, S, S, S, C)).cpu().contiguous() for t in (a1, o))
    out.backward(dy.to(case.dt).cuda())
    torch.cuda.synchronize()
    return out.detach().cpu(), xg.grad.cpu(), sg.grad.cpu(), masks


def _assert_flips_are_near_zero(mask, pre, tol, name):
    """a derivative mask may differ from the reference's own sign only where the reference pre-activation is within the forward tolerance of zero: a
    pre-activation computed to within tol * rms cannot change sign further out"""
    flipped = mask != (pre > 0)
    rms = pre.pow(2).mean().sqrt().item()
    worst = pre.abs()[flipped].max().item() if flipped.any() else 0.0
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  [{name}] {int(flipped.sum())} of {flipped.numel()} signs differ, the farthest at {worst / rms:.2e} rms (bound {tol:g})")
    assert worst <= tol * rms, f"{name}: a sign differs where the reference pre-activation is {worst / rms:.3e} rms (> {tol:g}); {int(flipped.sum())} of {flipped.numel()} differ"


def _compare(case, got, ref, grads, scale=1.0):
    """out / dx / dskip per sample, the five weight gradients; the three conv biases exactly zero.  scale: how many backward passes the gradients hold"""
    out, dx, dskip = got
    pairs = []     # (quantity, name, computed, reference)
    for b in range(case.B):
        pairs += [("out", f"out[{b}]", cf(out)[b], ref["out"][b]), ("dx", f"dx[{b}]", cf(dx)[b], ref["dx"][b]), ("dskip", f"dskip[{b}]", cf(dskip)[b], ref["dskip"][b])]
    pairs += [(n, n + ".grad", grads[n], ref["grads"][n] * scale) for n in QUANTITIES[3:]]
    if os.environ.get("NMH_PRINT_ERR"):     # every figure before the first assertion
        worst = {}
        for q, _, a, b in pairs:
            worst[q] = max(worst.get(q, 0.0), needed_rtol(a, b))
        print(f"  [{case.name} x{scale:g}] needed_rtol " + "  ".join(f"{q} {e:.2e} (tol {chain_tol(case, q):.2e})" for q, e in worst.items()))
    for q, name, a, b in pairs:
        assert_close(a, b, chain_tol(case, q), f"{case.name} {name}")
    for n in ("conv_block.conv1.bias", "conv_block.conv2.bias", "conv_block.conv3.bias"):
        # a bias in front of an InstanceNorm: the add is skipped, the gradient is exactly zero (tests/test_model_gpu.py states the contract)
        assert grads[n].abs().max().item() == 0.0 and ref["grads"][n].abs().max().item() < 1e-9, n


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_up_block_against_float64(case, monkeypatch):
    ops = _ops()
    model = _device_model(case, monkeypatch)
    blk = getattr(model, case.block)
    assert blk.has_proj and blk._wq is model._wq and ops.DEFER_DECODER_WGRAD and ops.side_stream.enabled and ops.HALO_WGRAD
    if not case.queue:
        monkeypatch.setattr(blk, "_wq", None)             # no queue: every weight gradient forks onto the side stream
    main = case.family == "c64"                           # the 64-block kernels' weight gradients stay on the main stream by plan
    plan = blk._plan(case.B, case.v, case.dt, True, None)
    assert plan.family == case.family and plan.proj and plan.epilogue_stats == main and plan.wgrad_main_stream == main
    assert plan.defer_conv_wgrad == (case.queue and not main) and plan.defer_upconv_wgrad == case.queue
    assert not (plan.composed_fwd or plan.fused_tail or plan.fused_reduce or plan.bg_norm_bwd)
    V = (case.v * blk.k) ** 3
    assert (V >= 4096) == (case.wgrad != IGEMM)

    names, call = [], ops.lib().call
    monkeypatch.setattr(ops.lib(), "call", lambda name, *a: (names.append(name), call(name, *a))[1])
    deferred = []
    if case.queue:
        defer = model._wq.defer
        monkeypatch.setattr(model._wq, "defer", lambda fn: (deferred.append(fn), defer(fn))[1])

    x, skip, dy = problem(case, blk)
    out, dx, dskip, masks = _run(case, blk, x, skip, dy)
    grads = {n: p.grad.detach().cpu().clone() for n, p in blk.named_parameters()}

    # ---- the path that ran
    n = collections.Counter(names)
    others = [e for e in list(CONV.values()) + [HALO48, HALO64, IGEMM] if e not in (CONV[case.family], case.wgrad)]
    assert n[CONV[case.family]] == 4 and n[case.wgrad] == 2 and not any(n[e] for e in others), n      # conv1, conv2 and their input gradients; two weight gradients
    assert (n["nmh_instnorm_finalize"], n["nmh_instnorm_stats"]) == ((2, 1) if main else (0, 3)), n   # the statistics epilogue of the 64-block kernel
    # the transpose conv's weight gradient: the grouped kernel in bf16 (ops.upconv_wgrad), the shuffled-view kernel in fp32; conv3: two GEMMs and a weight gradient
    assert (n["nmh_gemm_tn_grouped"], n["nmh_upconv_wgrad"]) == ((1, 0) if case.dt == BF16 else (0, 1)), n
    assert n["nmh_upconv_fwd"] == n["nmh_upconv_dgrad"] == n["nmh_gemm_tn"] == 1 and n["nmh_copy_cols"] == 2 and n["nmh_gemm_nt"] == 2, n
    assert len(deferred) == (3 if plan.defer_conv_wgrad else 0) + (1 if plan.defer_upconv_wgrad else 0)
    if case.queue:
        assert not (model._wq.deferred or model._wq.pending or model._wq.inflight), "the end-of-backward callback flushed and joined the queue"

    # ---- against float64, differentiated with the kernel's signs
    w = master_weights(blk)
    ref = U.up_block_grads(cf(x), cf(skip), w, blk.k, cf(dy), masks=masks)
    tol = TOL[case.dt]
    _assert_flips_are_near_zero(masks[0], ref["pre1"], tol, "conv1's LeakyReLU")
    _assert_flips_are_near_zero(masks[1], ref["pre2"], tol, "the output LeakyReLU")
    _compare(case, (out, dx, dskip), ref, grads)

    # ---- a second pass on the same model without zeroing: every parameter gradient accumulates
    if case.name in ("dec2-c48mb-queue", "dec3-c48mb-queue"):
        out2, dx2, dskip2, masks2 = _run(case, blk, x, skip, dy)
        if not all(torch.equal(a, b) for a, b in zip(masks, masks2)):     # (the forward's reductions are not ordered: a sign next to zero may come out differently)
            ref2 = U.up_block_grads(cf(x), cf(skip), w, blk.k, cf(dy), masks=masks2)
            ref2["grads"] = {k: (ref2["grads"][k] + ref["grads"][k]) / 2 for k in ref["grads"]}
            ref = ref2
        _compare(case, (out2, dx2, dskip2), ref, {n: p.grad.detach().cpu().clone() for n, p in blk.named_parameters()}, scale=2.0)
