"""CPU (-m "not gpu"): the C-ABI library loads and exports every symbol include/*.h declares (no compute calls), and the
host-side logic (tables, masking RNG, scheduler, sharding, state-dict contract, loud failure without a GPU)."""
import os
import random

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_capi_library_loads_and_exports_every_declared_symbol():
    from nerf_mae_amd._lib import HEADER, LIB_PATH, lib, parse_header
    assert os.path.exists(LIB_PATH), "run `python __graft_entry__.py` (build()) first"
    sigs = parse_header(HEADER)
    assert len(sigs) >= 28 and "nmh_window_attn_bwd" in sigs and "nmh_conv3d_k3_wgrad" in sigs
    L = lib()
    for name, (ret, args) in sigs.items():
        assert hasattr(L.cdll, name), f"{name} declared in nerfmae_hip.h but not exported"
    assert L.call("nmh_version") >= 100
    assert L.cdll.nmh_error_string(-2).decode().startswith("nmh:")
    # every NMH_API line parsed (the regex must not silently drop declarations)
    n_decl = sum(1 for line in open(HEADER) if line.startswith("NMH_API"))
    assert n_decl == len(sigs)


def test_no_cpu_fallback_product_fails_loudly_without_device():
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import build_model
    with pytest.raises(RuntimeError):
        ops.gemm_nt(torch.zeros(8, 8), torch.zeros(8, 8))
    m = build_model("swin_t", resolution=32)
    with pytest.raises(RuntimeError):
        m([torch.rand(4, 32, 32, 32)])
    # the product package never imports the oracle
    import sys
    for f in os.listdir(os.path.join(ROOT, "nerf-mae_amd")):
        if f.endswith(".py"):
            src = open(os.path.join(ROOT, "nerf-mae_amd", f)).read()
            assert "import oracle" not in src and "from oracle" not in src, f


def test_tables_and_mask_rng_match_reference_golden(golden):
    from nerf_mae_amd.model import draw_block_mask, relative_position_index, sincos_pos_embed_3d
    g2, g5 = golden("g2_tables.npz"), golden("g5_masks.npz")
    assert np.array_equal(relative_position_index(4).numpy().astype(np.int16), g2["rel_index"])
    np.testing.assert_allclose(sincos_pos_embed_3d(24, 8).astype(np.float32), g2["pos_embed_24_8"], atol=1e-6)
    big = sincos_pos_embed_3d(96, 40).astype(np.float32)
    np.testing.assert_allclose(big[0, ::13, ::11, ::7, :], g2["pos_embed_96_40_samples"], atol=1e-6)
    for key, gsz, seed, p in [("blocks_40_seed1234", 40, 1234, 0.75), ("blocks_8_seed1234", 8, 1234, 0.75), ("blocks_40_seed7_p50", 40, 7, 0.5)]:
        random.seed(seed)
        assert np.array_equal(draw_block_mask((gsz,) * 3, p)[::4, ::4, ::4].numpy(), g5[key]), key
    # swin_b deviation: 3 x 42 channels + 2 zero pads
    pe = sincos_pos_embed_3d(128, 4)
    assert pe.shape == (1, 4, 4, 4, 128) and np.all(pe[..., 126:] == 0)


def test_state_dict_contract_and_strict_interchange_with_oracle():
    from nerf_mae_amd.model import SwinTransformer_MAE3D, SwinTransformer_MAE3D_New, build_model
    from oracle import mae3d_oracle as O
    assert SwinTransformer_MAE3D is SwinTransformer_MAE3D_New
    for name, nkeys in [("swin_t", 215), ("swin_s", 383)]:
        m, o = build_model(name, resolution=32), O.build_oracle(name, resolution=32)
        sd, so = m.state_dict(), o.state_dict()
        assert len(sd) == nkeys and set(sd) == set(so)
        assert all(sd[k].shape == so[k].shape and sd[k].dtype == so[k].dtype for k in sd)
        assert not m.load_state_dict(so, strict=True).missing_keys
        assert not o.load_state_dict(sd, strict=True).missing_keys
    m = build_model("swin_s", resolution=160)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 70040938
    assert m.pos_embed.requires_grad is False and m.pos_embed.shape == (1, 40, 40, 40, 96)
    # nerf_rpn deletes the decoder half after a strict load (feature_extractor.py:1158-1163)
    del m.decoder4, m.decoder3, m.decoder2, m.decoder1, m.out, m.mask_token
    assert all(k.startswith(("patch_partition", "stages", "pos_embed")) for k in m.state_dict())
    with pytest.raises(ValueError):
        SwinTransformer_MAE3D(patch_size=[4] * 3, embed_dim=128, depths=[2, 2, 18, 2], num_heads=[3, 6, 12, 24], window_size=[4] * 3)


def test_flat_buffers_and_packer_layout_on_cpu():
    """flatten_parameters keeps values, makes params/grads views of two flat buffers (mask_token first: its gradient completes last)"""
    from nerf_mae_amd.model import build_model
    m = build_model("swin_t", resolution=32, compute_dtype=torch.float32)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    flat, fg = m.flatten_parameters(torch.device("cpu"))
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert m.mask_token.data_ptr() == flat.data_ptr()
    for p in m.parameters():
        if p.requires_grad:
            off = m._offsets[id(p)]
            assert p.data_ptr() == flat.data_ptr() + 4 * off and p.grad.data_ptr() == fg.data_ptr() + 4 * off and off % 4 == 0
    P = m._packer
    assert P["decoder1.c1.w"].numel() == 48 * 27 * 48 and P["s2.1.qkv.wT"].numel() == 3 * 384 * 384
    assert P.descs.numel() == 40 * len(P.items)


def test_onecycle_matches_torch_onecyclelr():
    from nerf_mae_amd.trainer import OneCycle
    p = torch.nn.Parameter(torch.zeros(1))
    for total in (10, 57, 2000):
        opt = torch.optim.AdamW([p], lr=1e-4)
        sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-4, total_steps=total)
        mine = OneCycle(1e-4, total)
        for step in range(total):
            lr, b1 = mine.at(step)
            assert abs(lr - opt.param_groups[0]["lr"]) < 1e-12 and abs(b1 - opt.param_groups[0]["betas"][0]) < 1e-9, (total, step)
            opt.step()
            sch.step()


def test_shard_indices_match_distributed_sampler():
    from torch.utils.data import DistributedSampler
    from nerf_mae_amd.dist import shard_indices
    ds = list(range(37))
    for world in (1, 2, 8):
        for rank in range(world):
            s = DistributedSampler(ds, num_replicas=world, rank=rank, shuffle=True, seed=0)
            for epoch in (0, 3):
                s.set_epoch(epoch)
                assert list(iter(s)) == shard_indices(len(ds), rank, world, epoch)


def test_window_geometry():
    from nerf_mae_amd.ops import WinGeom
    g = WinGeom(2, 5, 10, 2, [2, 2, 2])
    assert g.P == [8, 12, 4] and g.shift == [2, 2, 0] and g.rows == 2 * 8 * 12 * 4 and g.tokens == 200
    assert list(g.carr) == [2, 5, 10, 2, 8, 12, 4, 2, 2, 0]


def test_block_bits_roundtrip_and_rng_stream():
    """draw_block_bits consumes the python RNG exactly like draw_block_mask (the reference's window_masking_3d raster, swin_mae3d.py:
    1366-1373) and block_bits_of_mask inverts the block fill; non-block-structured masks are rejected (-> the upload fallback)"""
    import random
    import numpy as np
    from nerf_mae_amd.model import block_bits_of_mask, draw_block_bits, draw_block_mask
    for g in (8, 10, 40):
        m = draw_block_mask((g, g, g), 0.75, rng=random.Random(7)).numpy()
        bits = draw_block_bits((g, g, g), 0.75, rng=random.Random(7))
        back = block_bits_of_mask(m)
        assert back is not None and np.array_equal(back, bits)
    bad = draw_block_mask((8, 8, 8), 0.5, rng=random.Random(1)).numpy().copy()
    bad[1, 2, 3] ^= 1
    assert block_bits_of_mask(bad) is None


def test_capi_rejects_null_required_pointers_without_touching_the_device():
    """boundary contract (include/nerfmae_hip.h): a NULL in a required pointer argument returns the argument-error code -4 -- no launch,
    no device fault -- so the check runs on a box without a GPU"""
    import ctypes
    from nerf_mae_amd._lib import lib
    L = lib().cdll
    null = ctypes.c_void_p(None)
    assert L.nmh_gemm_nt(1, null, 96, null, 96, 64, 96, 96, null, 96, null, 0, null, null, null, 1, 0, null) == -4
    assert L.nmh_conv3d_k3(1, null, null, null, 1, 8, 8, 8, 48, 48, 0, null, 0, null) == -4
    assert L.nmh_conv3d_k3_c48mb(null, null, null, 1, 8, 8, 8, 96, 96, 0, null) == -4
    assert L.nmh_gemm_tn_grouped(1, null, 3, null, 0, null) == -4
    assert L.nmh_conv3d_k3_c64(null, null, null, 1, 8, 8, 8, 64, 64, 0, null, null, null) == -4
    assert L.nmh_set_prezeroed_arena(null, 4096) == -4 and L.nmh_set_prezeroed_arena(null, -1) == -4
    assert L.nmh_set_prezeroed_arena(null, 0) == 0      # bytes = 0 removes the arena
    from nerf_mae_amd import ops
    ar = ops.AccArena._inst
    if ar is not None:   # the arena is process-wide state: give back the one an earlier GPU test of this session registered
        assert L.nmh_set_prezeroed_arena(ctypes.c_void_p(ar.buf.data_ptr()), ar.BYTES) == 0
    assert L.nmh_error_string(-4).decode().startswith("nmh:")


# ---- the decoder up-block's plan (model.plan_up_block): which kernels a decoder level runs, asked with plain values
def _layouts(*families):
    from nerf_mae_amd.model import _CONV_LAYOUTS
    return {n for f in families + ("generic",) for n in _CONV_LAYOUTS[f]}


def _switches(**kw):
    from nerf_mae_amd.model import UpSwitches
    on = dict(tail_from_coarse=True, tail_sign_mask=True, cconv_wgrad=True, cconv_centered=True, c48_bwd_reduce=True, inbwd_bg=True, defer_decoder_wgrad=True,
              side_stream=True, c48mb_min_voxels=32768, c64_min_voxels=32768)   # the defaults of the ops switches
    return UpSwitches(**dict(on, **kw))


DEC1_BUFFERS = frozenset({"dgrad", "mean_table", "tail_residual"})


def _mae_decoder1(B=8, v=40, dtype=torch.bfloat16, x_grad=True, tail=True, dec1=DEC1_BUFFERS, sw=None):
    """decoder1 of swin_t / swin_s (96 -> 48, k = 4, no skip) in training with the fused tail, behind the model's weight-gradient queue"""
    from nerf_mae_amd.model import plan_up_block
    layouts = _layouts("c48") if dtype == torch.bfloat16 else _layouts()
    return plan_up_block(96, 48, 4, False, layouts, dec1, B, v, dtype, x_grad, tail, tail, True, sw or _switches())


def test_up_block_plan_of_the_mae_decoder1():
    from nerf_mae_amd.model import _CONV_LAYOUTS
    p = _mae_decoder1()
    assert p.family == "c48" and (p.c1_fwd, p.c1_dgrad, p.c2_fwd, p.c2_dgrad) == _CONV_LAYOUTS["c48"] == ("c1.wk", "c1.wkd", "c2.wk", "c2.wkd")
    assert p.epilogue_stats and p.composed_fwd and p.composed_bwd and p.centered and p.residual_in_tail and p.fused_tail and p.sign_mask and p.tail_bwd_sums
    assert p.fused_reduce and p.bg_norm_bwd and p.wgrad_main_stream and not p.defer_conv_wgrad and p.defer_upconv_wgrad and not p.proj and p.x_grad
    for B in (1, 2, 4, 8):
        assert _mae_decoder1(B=B) == p
    assert _mae_decoder1(B=3) == p._replace(centered=False)          # centered_wgrad_ok: the scaled weight-gradient reduce takes B in {1, 2, 4, 8}
    assert _mae_decoder1(B=2, v=16) == p and _mae_decoder1(B=2, v=8) == p   # 64^3 and 32^3, the sizes of the GPU tests
    # the residual is formed in the tail only in training with the fused tail: otherwise `cat` is stored
    nograd = _mae_decoder1(x_grad=False)
    assert nograd == p._replace(residual_in_tail=False, x_grad=False, tail_bwd_sums=False, sign_mask=False)
    notail = _mae_decoder1(tail=False)
    assert notail == p._replace(residual_in_tail=False, fused_tail=False, tail_bwd_sums=False, sign_mask=False)
    # a switch changes its own field alone
    assert _mae_decoder1(sw=_switches(cconv_centered=False)) == p._replace(centered=False)
    assert _mae_decoder1(sw=_switches(tail_from_coarse=False)) == p._replace(residual_in_tail=False)
    # ... and so does the buffer a switch that was off when the packer was built leaves out
    assert _mae_decoder1(dec1=DEC1_BUFFERS - {"mean_table"}) == p._replace(centered=False)
    assert _mae_decoder1(dec1=DEC1_BUFFERS - {"tail_residual"}) == p._replace(residual_in_tail=False)
    # 120^3 (v = 30 is no multiple of 8): no decoder-1 record is built
    p120 = _mae_decoder1(v=30, dec1=None)
    assert p120.family == "c48" and p120.epilogue_stats and not (p120.composed_fwd or p120.composed_bwd or p120.centered or p120.residual_in_tail)
    assert p120.fused_tail and p120.sign_mask and not p120.fused_reduce and not p120.bg_norm_bwd      # (120 % 16 != 0)
    with pytest.raises(AttributeError):
        p.centered = False


def test_up_block_plan_in_fp32_is_the_generic_path():
    from nerf_mae_amd.model import _CONV_LAYOUTS, build_model
    p = _mae_decoder1(dtype=torch.float32, dec1=None)
    assert p.family == "generic" and (p.c1_fwd, p.c1_dgrad, p.c2_fwd, p.c2_dgrad) == _CONV_LAYOUTS["generic"] == ("c1.w", "c1.wd", "c2.w", "c2.wd")
    assert not (p.epilogue_stats or p.composed_fwd or p.composed_bwd or p.centered or p.residual_in_tail or p.sign_mask or p.fused_reduce or p.bg_norm_bwd)
    assert p.fused_tail and p.tail_bwd_sums and not p.wgrad_main_stream and p.defer_conv_wgrad and p.defer_upconv_wgrad
    # the same answer from a block's own packer (the layouts and the absent decoder-1 record are read off it)
    m = build_model("swin_t", resolution=32, compute_dtype=torch.float32)
    m.flatten_parameters(torch.device("cpu"))
    assert m._packer.dec1 is None
    q = m.decoder1._plan(2, 8, torch.float32, True, (m,))
    assert (q.family, q.composed_fwd, q.centered, q.fused_tail, q.proj) == ("generic", False, False, True, False)
    assert m.decoder2._plan(2, 4, torch.float32, True, None).proj


def test_loss_tail_record_reaches_the_up_block_plan(monkeypatch):
    """UpBlock3D._plan hands plan_up_block tail_pred = "pred_out is given" and tail_zero_padded = the record's flag (False where it is left out), as it did with
    the 5- and 6-element tuples; no tail: neither"""
    from types import SimpleNamespace
    from nerf_mae_amd import model as M
    seen = []
    monkeypatch.setattr(M, "plan_up_block", lambda *a, **kw: seen.append((a[10], a[11], kw["tail_pred"], kw["tail_zero_padded"])))   # (tail, tail_sums, ...)
    stub = SimpleNamespace(fuse_tail_sums=True)
    blk = M.UpBlock3D(96, 48, 4, use_skip=False)
    blk._pk = SimpleNamespace(views={}, dec1=None)
    blk._key, blk._wq = "decoder1.", None
    pred = torch.empty(1)
    assert M.LossTail._fields == ("model", "xb", "extents", "tokmask", "pred_out", "zero_padded")
    for tail in (M.LossTail(stub, None, None, None, None), M.LossTail(stub, None, None, None, None, True), M.LossTail(stub, None, None, None, pred, True),
                 M.LossTail(stub, None, None, None, pred, zero_padded=False), None):
        blk._plan(2, 8, torch.bfloat16, True, tail)
    assert seen == [(True, True, False, False), (True, True, False, True), (True, True, True, True), (True, True, True, False), (False, False, False, False)]
    # the plain tuples of before are read as the record (LossTail.of): 1, 5 and 6 elements
    for old, new in (((stub,), M.LossTail(stub)), ((stub, None, None, None, pred), M.LossTail(stub, pred_out=pred)),
                     ((stub, None, None, None, None, True), M.LossTail(stub, zero_padded=True))):
        assert M.LossTail.of(old) == new and M.LossTail.of(new) is new
    assert M.LossTail.of(None) is None


def test_up_block_plan_of_the_other_levels_and_backbones():
    from nerf_mae_amd.model import plan_up_block
    bf, sw = torch.bfloat16, _switches()
    # swin_s decoder2 at 160^3: 192 -> 96, k = 2, skip, S = 40
    p = plan_up_block(192, 96, 2, True, _layouts("c48mb"), None, 8, 20, bf, True, False, False, True, sw)
    assert p.family == "c48mb" and (p.c1_fwd, p.c2_dgrad) == ("c1.wkm", "c2.wkmd") and p.proj and not p.epilogue_stats and not p.wgrad_main_stream
    assert p.defer_conv_wgrad and p.defer_upconv_wgrad and not (p.composed_fwd or p.centered or p.fused_tail or p.fused_reduce or p.bg_norm_bwd)
    assert plan_up_block(192, 96, 2, True, _layouts("c48mb"), None, 8, 8, bf, True, False, False, True, sw).family == "generic"   # 16^3: below C48MB_MIN_VOXELS
    # swin_b at 160^3: decoder1 128 -> 64 (k = 4, no skip) and decoder2 256 -> 128 (S = 40)
    for args in ((128, 64, 4, False, _layouts("c64"), None, 8, 40), (256, 128, 2, True, _layouts("c64"), None, 8, 20)):
        p = plan_up_block(*args, bf, True, not args[3], not args[3], True, sw)
        assert p.family == "c64" and (p.c1_fwd, p.c1_dgrad) == ("c1.w64", "c1.w64d") and p.epilogue_stats and p.wgrad_main_stream
        assert not p.defer_conv_wgrad and p.defer_upconv_wgrad and not (p.composed_fwd or p.composed_bwd or p.centered or p.residual_in_tail or p.sign_mask)
    # the voxel heads' decoder1 (heads.py): skip, generic layouts only, packed on its own (no queue)
    p = plan_up_block(96, 48, 4, True, _layouts(), None, 2, 8, bf, True, False, False, False, sw)
    assert p.family == "generic" and p.proj and not (p.composed_fwd or p.composed_bwd or p.centered or p.defer_conv_wgrad or p.defer_upconv_wgrad)


# ---- the Swin block's plan (model.plan_swin_block): which form of each branch an encoder block runs, asked with plain values
def _block_switches(**kw):
    from nerf_mae_amd.model import BlockSwitches
    on = dict(swin_fused=True, swin_attn_widths=(96, 192, 384), swin_attn_min_windows=100, swin_mlp_widths=(192, 384), swin_mlp_min_rows=6000, mlp_fused=True,
              mlp_fused_widths=(96,), mlp_fused_min_rows=4096, token_bwd=True, grouped_wgrad=True, flush_after_first=True)   # the defaults of the ops switches
    return BlockSwitches(**dict(on, **kw))


def _block(C, heads, tokens, rows, B, dtype=torch.bfloat16, streams=True, x_grad=True, hidden=None, lds=True, queue=True, sw=None):
    from nerf_mae_amd.model import plan_swin_block
    return plan_swin_block(C, heads, 4 * C if hidden is None else hidden, tokens, rows, B, dtype, x_grad, streams, lds, queue, sw or _block_switches())


# (C, heads, tokens, rows, B), keywords -> (attn, mlp, token_bwd): swin_s at 160^3 and what the tests run
SWIN_BLOCK_CASES = {
    "stage 0": ((96, 3, 512000, 512000, 8), {}, ("fused", "lds", False)),
    "stage 1": ((192, 6, 64000, 64000, 8), {}, ("fused", "stream", False)),
    "stage 2 (10^3 in 12^3)": ((384, 12, 8000, 13824, 8), {}, ("fused", "stream", True)),
    "stage 3 (5^3 in 8^3)": ((768, 24, 1000, 4096, 8), dict(streams=False), ("tokens", "unfused", True)),
    "stage 2, one grid (27 windows)": ((384, 12, 1000, 1728, 1), {}, ("tokens", "unfused", True)),
    "stage 1, one grid (125 windows)": ((192, 6, 8000, 8000, 1), {}, ("fused", "stream", False)),
    "stage 0 at 120^3 (30^3 in 32^3): the interlock": ((96, 3, 216000, 262144, 8), {}, ("fused", "lds", False)),
    "stage 2 without an input gradient": ((384, 12, 8000, 13824, 8), dict(x_grad=False), ("fused", "stream", False)),
    "fp32, unpadded": ((96, 3, 1024, 1024, 2), dict(dtype=torch.float32, streams=False), ("window", "unfused", False)),
    "fp32, padded": ((384, 12, 16, 128, 2), dict(dtype=torch.float32, streams=False), ("tokens", "unfused", True)),
    "swin_b width": ((128, 4, 1024, 1024, 2), dict(streams=False), ("window", "unfused", False)),
}


def test_swin_block_plan_of_swin_s_and_of_the_test_sizes():
    for name, (dims, kw, want) in SWIN_BLOCK_CASES.items():
        p = _block(*dims, **kw)
        assert (p.attn, p.mlp, p.token_bwd) == want, (name, p)
        assert p.queue_wgrad == (kw.get("dtype") != torch.float32), (name, p)    # the grouped weight-gradient kernel takes bf16 operands
    assert not _block(96, 3, 512000, 512000, 8, queue=False).queue_wgrad
    assert not _block(96, 3, 512000, 512000, 8, sw=_block_switches(grouped_wgrad=False)).queue_wgrad
    # the kernels of csrc/swin_block.hip take heads = C / 32 and a hidden width of 4 C only
    for kw in (dict(hidden=2 * 192), dict(hidden=4 * 192, streams=False)):
        p = _block(192, 6, 64000, 64000, 8, **kw)
        assert (p.attn, p.mlp) == ("window", "unfused"), (kw, p)
    p = _block(192, 4, 64000, 64000, 8)
    assert (p.attn, p.mlp) == ("window", "unfused")
    p = _block(384, 8, 8000, 13824, 8)
    assert (p.attn, p.mlp, p.token_bwd) == ("tokens", "unfused", True)
    with pytest.raises(AttributeError):
        p.attn = "fused"


def test_swin_block_plan_switches_change_what_they_gate_alone(monkeypatch):
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import BlockSwitches
    s0, s1, s2 = (_block(*SWIN_BLOCK_CASES[k][0]) for k in ("stage 0", "stage 1", "stage 2 (10^3 in 12^3)"))
    off = _block_switches(swin_fused=False)
    assert _block(96, 3, 512000, 512000, 8, sw=off) == s0._replace(attn="window")                     # (the LDS MLP is not a Swin kernel)
    assert _block(192, 6, 64000, 64000, 8, sw=off) == s1._replace(attn="window", mlp="unfused")
    assert _block(384, 12, 8000, 13824, 8, sw=off) == s2._replace(attn="tokens", mlp="unfused")
    off = _block_switches(token_bwd=False)
    assert _block(384, 12, 8000, 13824, 8, sw=off) == s2._replace(token_bwd=False)
    assert _block(768, 24, 1000, 4096, 8, streams=False, sw=off) == _block(768, 24, 1000, 4096, 8, streams=False)._replace(attn="window", token_bwd=False)
    assert _block(96, 3, 512000, 512000, 8, sw=off) == s0
    # without the LDS kernel the next eligible form takes over: none at C = 96 by default, the stream kernel where its widths list 96
    assert _block(96, 3, 512000, 512000, 8, lds=False) == s0._replace(mlp="unfused")
    assert _block(96, 3, 512000, 512000, 8, sw=_block_switches(mlp_fused=False)) == s0._replace(mlp="unfused")
    assert _block(96, 3, 512000, 512000, 8, lds=False, sw=_block_switches(swin_mlp_widths=(96, 192, 384))) == s0._replace(mlp="stream")
    # ... and at a padded stage the token-ordered backward is free again
    i = _block(96, 3, 216000, 262144, 8)
    assert _block(96, 3, 216000, 262144, 8, lds=False) == i._replace(mlp="unfused", token_bwd=True)
    # thresholds: one below keeps the unfused form
    assert _block(192, 6, 6336, 6336, 1).attn == "window" and _block(192, 6, 6400, 6400, 1).attn == "fused"          # 99 / 100 windows
    assert _block(192, 6, 5999, 6336, 1).mlp == "unfused" and _block(192, 6, 6000, 6336, 1).mlp == "stream"
    assert _block(96, 3, 4095, 4096, 1).mlp == "unfused" and _block(96, 3, 4096, 4096, 1).mlp == "lds"
    # BlockSwitches.current() reads the ops globals as they are now
    for name, field, value in (("SWIN_ATTN_MIN_WINDOWS", "swin_attn_min_windows", 1), ("SWIN_MLP_MIN_ROWS", "swin_mlp_min_rows", 1),
                               ("MLP_FUSED_MIN_ROWS", "mlp_fused_min_rows", 1), ("TOKEN_BWD", "token_bwd", False), ("GROUPED_WGRAD", "grouped_wgrad", False),
                               ("WQ_FLUSH_AFTER_FIRST", "flush_after_first", False), ("SWIN_MLP_WIDTHS", "swin_mlp_widths", (384,))):
        before = BlockSwitches.current()
        monkeypatch.setattr(ops, name, value)
        assert BlockSwitches.current() == before._replace(**{field: value})


def test_swin_block_plans_itself_and_names_its_queue(monkeypatch):
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import SwinBlock3D, build_model, wgrad_queue_for
    for name in ("SWIN_FUSED", "MLP_FUSED", "TOKEN_BWD", "GROUPED_WGRAD"):
        monkeypatch.setattr(ops, name, True)
    m = build_model("swin_t", resolution=32, compute_dtype=torch.float32)
    m.flatten_parameters(torch.device("cpu"))
    blk = next(b for b in m.stages[2] if isinstance(b, SwinBlock3D))
    p = blk._plan(ops.WinGeom(2, 2, 2, 2, blk.shift_size), torch.float32, True)     # 2^3 tokens in 4^3 window rows
    assert (p.attn, p.mlp, p.token_bwd, p.queue_wgrad) == ("tokens", "unfused", True, False)
    assert ops.mlp_fused_supported(96) and not ops.mlp_fused_supported(100)
    assert wgrad_queue_for(m, torch.float32) is None and wgrad_queue_for(m, torch.bfloat16) is m._wq and wgrad_queue_for(blk, torch.bfloat16) is m._wq
    monkeypatch.setattr(ops, "GROUPED_WGRAD", False)
    assert wgrad_queue_for(m, torch.bfloat16) is None


# ---- the patch embed's plan (model.plan_embed): which rows the embed and stage 0's first block run on, asked with plain values
def _embed_switches(**kw):
    from nerf_mae_amd.model import EmbedSwitches
    return EmbedSwitches(**dict(dict(embed_kept=True, block0_kept=True), **kw))   # the defaults of the ops switches


def _embed_plan(g, mask=True, add_pos=True, capacity=None, aligned=True, block0_ok=True, sw=None):
    from nerf_mae_amd.model import plan_embed
    return plan_embed(g, mask, add_pos, capacity, aligned, block0_ok, sw or _embed_switches())


def test_embed_plan_of_the_mae_step_and_of_the_test_sizes():
    from nerf_mae_amd.model import EmbedPlan, embed_capacity_rows
    # 32^3 (g = 8: 8 windows): no capacity given = a row, or a window slot, for everything
    assert _embed_plan(8) == EmbedPlan("windows", 64 * 9, 8, True)
    assert _embed_plan(8, capacity=192) == EmbedPlan("windows", 64 * 4, 3, True)
    assert _embed_plan(8, aligned=False) == EmbedPlan("rows", 512, 0, True)
    assert _embed_plan(8, capacity=192, aligned=False) == EmbedPlan("rows", 192, 0, True)
    # 160^3 (g = 40: 1000 windows), the capacity a captured step takes from the mask distribution
    cap40 = embed_capacity_rows(40, p_remove=0.75)
    assert cap40 % 64 == 0 and 64000 // 4 < cap40 < 0.4 * 64000
    assert _embed_plan(40, capacity=cap40) == EmbedPlan("windows", 64 * (cap40 // 64 + 1), cap40 // 64, True)
    assert _embed_plan(40, capacity=cap40, aligned=False) == EmbedPlan("rows", cap40, 0, True)
    assert _embed_plan(40) == EmbedPlan("windows", 64 * 1001, 1000, True)
    assert _embed_plan(40, aligned=False) == EmbedPlan("rows", 64000, 0, True)
    assert _embed_plan(40, capacity=10 ** 6, aligned=False).rows == 64000         # never more rows than tokens
    # g % 4 != 0: kept rows, never windows
    assert _embed_plan(10) == EmbedPlan("rows", 1000, 0, True) and _embed_plan(10, capacity=320) == EmbedPlan("rows", 320, 0, True)
    # a first block that does not qualify: kept rows
    assert _embed_plan(8, capacity=192, block0_ok=False) == EmbedPlan("rows", 192, 0, True)
    # no mask, or no position embedding (patch_partition alone): a row for every token, whatever the caller promises
    assert _embed_plan(8, mask=False, capacity=192) == EmbedPlan("dense", 512, 0, True)
    assert _embed_plan(8, mask=False, add_pos=False) == EmbedPlan("dense", 512, 0, False)
    assert _embed_plan(8, add_pos=False, capacity=192) == EmbedPlan("dense", 512, 0, False)
    # window slots and rows at g = 8: capW = max(1, min(cap // 64, 8)), rows = 64 (capW + 1)
    for cap, capW in ((64, 1), (192, 3), (256, 4), (512, 8), (1024, 8), (32, 1)):      # (cap // 64 above the window count; cap < 64)
        p = _embed_plan(8, capacity=cap)
        assert (p.path, p.capW, p.rows) == ("windows", capW, 64 * (capW + 1)), (cap, p)
    assert _embed_plan(8, capacity=32, aligned=False).rows == 32
    with pytest.raises(AttributeError):
        p.path = "dense"


def test_embed_plan_switches_change_what_they_gate_alone(monkeypatch):
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import EmbedPlan, EmbedSwitches
    w, r = _embed_plan(8, capacity=192), _embed_plan(8, capacity=192, aligned=False)
    assert _embed_plan(8, capacity=192, sw=_embed_switches(block0_kept=False)) == w._replace(path="rows", rows=192, capW=0) == r
    assert _embed_plan(8, capacity=192, aligned=False, sw=_embed_switches(block0_kept=False)) == r
    for kw in (dict(), dict(aligned=False)):
        assert _embed_plan(8, capacity=192, sw=_embed_switches(embed_kept=False), **kw) == EmbedPlan("dense", 512, 0, True)    # (the window path needs the kept rows)
    assert _embed_plan(8, mask=False, sw=_embed_switches(embed_kept=False, block0_kept=False)) == _embed_plan(8, mask=False)
    for name, field in (("EMBED_KEPT", "embed_kept"), ("BLOCK0_KEPT", "block0_kept")):
        before = EmbedSwitches.current()
        monkeypatch.setattr(ops, name, not getattr(before, field))
        assert EmbedSwitches.current() == before._replace(**{field: not getattr(before, field)})


def _cuts_windows():
    m = torch.ones(8, 8, 8, dtype=torch.uint8)
    m[:2] = 0          # 128 tokens kept, through the middle of four windows
    return m


def test_refit_bound_against_the_conditions_the_step_held_inline():
    """model.refit_bound (on model.mask_kept_aligned) against what GraphedTrainStep._fit_capture held inline: with an aligned bound, a mask that is neither block
    bits with nb * 4 == g nor constant on every window drops the alignment; with fewer rows than tokens, a mask that keeps more than the rows takes a row for
    every token; otherwise the capture stays.  The two limits broken at once give one widened bound (the inline form captured twice)."""
    from nerf_mae_amd.model import EmbedBound, block_bits_of_mask, bound_of_mask, embed_capacity_rows, mask_kept_aligned, mask_window_aligned, refit_bound
    g = 8
    few = torch.ones(8, 8, 8, dtype=torch.uint8)
    few[:4, :4, :4] = 0          # one block kept: 64 tokens
    many = torch.zeros(8, 8, 8, dtype=torch.uint8)
    many[:4, :4, :4] = 1         # seven blocks kept: 448 tokens
    cut = _cuts_windows()
    masks = {"few": few.numpy(), "many": many.numpy(), "cut": cut.numpy(), "all": np.ones((8, 8, 8), np.uint8), "none": np.zeros((8, 8, 8), np.uint8)}

    def inline(bound, block_mask, bits):     # _fit_capture of before, on a bound; rows = None stands for g^3
        aligned, rows = bound.aligned, g ** 3 if bound.rows is None else bound.rows
        if aligned and not (bits is not None and np.asarray(bits).shape[0] * 4 == g) and not mask_window_aligned(np.asarray(block_mask)):
            aligned = False
        if rows < g ** 3 and g ** 3 - (64 * int(np.asarray(bits).sum()) if bits is not None else int(np.asarray(block_mask).sum())) > rows:
            rows = g ** 3
        return EmbedBound(rows, aligned)

    full = lambda b: b._replace(rows=g ** 3 if b.rows is None else b.rows)   # noqa: E731
    for rows in (None, 64, 128, 256, 448, 512):
        for al in (False, True):
            bound = EmbedBound(rows, al)
            for name, m in masks.items():
                for bits in (None, block_bits_of_mask(m)):
                    got, want = refit_bound(bound, g, *mask_kept_aligned(g, m, bits)), inline(bound, m, bits)
                    assert full(bound if got is None else got) == want, (bound, name, bits is not None, got, want)
                    assert (got is None) == (want == full(bound)), (bound, name, bits is not None, got, want)     # None exactly where nothing changes
    # the cases by name
    assert mask_kept_aligned(g, masks["few"]) == (64, True) and mask_kept_aligned(g, masks["many"]) == (448, True) and mask_kept_aligned(g, masks["cut"]) == (128, False)
    assert refit_bound(EmbedBound(64, False), g, 64, True) is None                                   # fits
    assert refit_bound(EmbedBound(64, False), g, 448, True) == EmbedBound(512, False)                 # widened to a row for every token
    assert refit_bound(EmbedBound(128, True), g, 128, False) == EmbedBound(128, False)                # alignment dropped, capacity kept
    assert refit_bound(EmbedBound(64, True), g, 128, False) == EmbedBound(512, False)                 # both at once: one widened bound
    assert refit_bound(EmbedBound(512, False), g, 512, False) is None and refit_bound(EmbedBound(None, False), g, 512, False) is None   # everything fits
    # block bits with nb * 4 == g are aligned without looking: the mask itself is not read
    bits = block_bits_of_mask(masks["few"])
    assert bits.shape == (2, 2, 2) and mask_kept_aligned(g, object(), bits) == (64, True)
    assert mask_kept_aligned(10, np.zeros((2, 2, 2), np.uint8), np.zeros((2, 2, 2), np.uint8)) == (1000, False)      # g % 4 != 0: bits are no windows
    # the bound of a known mask: what the eager forward computed
    for name, m in masks.items():
        assert bound_of_mask(g, m) == EmbedBound(embed_capacity_rows(g, kept=512 - int(m.sum())), mask_window_aligned(m)), name
    assert bound_of_mask(g, masks["cut"]) == EmbedBound(128, False) and bound_of_mask(g, masks["all"]) == EmbedBound(64, True)
    assert bound_of_mask(g, few) == EmbedBound(64, True)      # a host tensor, as forward() holds it


def test_stage_flush_policy_for_every_input():
    """model.flush_actions against the conditions _StageFlushFn.backward held inline: join first only when an all-reduce follows the flush; leave the flush to
    the next block unless this is the last one of the backward pass or an all-reduce waits for it; the last one runs in the foreground; join after it for an
    all-reduce"""
    from nerf_mae_amd.model import flush_actions
    want = {  # (last, sync_after_flush, flush_after_first) -> (join_before, request, foreground, join_after)
        (False, False, False): (False, False, False, False), (False, False, True): (False, True, False, False),
        (False, True, False): (True, False, False, True), (False, True, True): (True, False, False, True),
        (True, False, False): (False, False, True, False), (True, False, True): (False, False, True, False),
        (True, True, False): (True, False, True, True), (True, True, True): (True, False, True, True),
    }
    for args, res in want.items():
        assert tuple(flush_actions(*args)) == res, args


def test_decoder1_pack_record_names_its_buffers(monkeypatch):
    from nerf_mae_amd import ops
    from nerf_mae_amd.model import UpBlock3D, _Dec1Pack
    blk = UpBlock3D(96, 48, 4, use_skip=False)
    for name in ("CCONV_WGRAD", "CCONV_CENTERED", "TAIL_FROM_COARSE"):
        monkeypatch.setattr(ops, name, True)
    d = _Dec1Pack(blk, torch.device("cpu"))
    assert d.block is blk and d.optional() == DEC1_BUFFERS
    assert d.composed.numel() == ops.cconv_pack_numel() and d.composed.dtype == torch.bfloat16 and d.border.shape == (27, 48)
    assert d.workspace.numel() == ops.cconv_pack_ws_floats() and d.workspace.dtype == torch.float32
    assert d.upconv4.numel() == ops.upconv4_pack_numel() and d.dgrad.numel() == ops.cconv_dgrad_pack_numel()
    assert d.mean_table.shape == (27, 96, 48) and d.tail_residual.numel() == ops.tail_residual_pack_numel()
    monkeypatch.setattr(ops, "CCONV_CENTERED", False)
    monkeypatch.setattr(ops, "CCONV_WGRAD", False)
    d = _Dec1Pack(blk, torch.device("cpu"))
    assert d.mean_table is None and d.dgrad is None and d.optional() == {"tail_residual"}


@pytest.mark.parametrize("dtype,cin,cout,c64", [(torch.bfloat16, 64, 64, True), (torch.float32, 64, 64, False), (torch.bfloat16, 32, 32, False), (torch.bfloat16, 64, 96, False)],
                         ids=["bf16-64-64", "fp32-64-64", "bf16-32-32", "bf16-64-96"])
def test_conv_layer_registers_the_64_channel_block_layouts_only_where_the_kernel_can_run(dtype, cin, cout, c64):
    """conv_layer.register on a bare _Packer (add only reads shapes): `.w` / `.wd` always, `.w64` / `.w64d` if and only if bf16 and both channel counts
    are multiples of 64, decided from the weight's shape"""
    from nerf_mae_amd import conv_layer, ops
    from nerf_mae_amd.model import _Packer
    P = _Packer()
    conv = torch.nn.Conv3d(cin, cout, 3, padding=1)
    conv_layer.register(P, "k", conv, dtype)
    modes = {key: mode for key, _, mode, _, _ in P.items}
    want = {"k.w": P.CONV_F, "k.wd": P.CONV_D}
    if c64:
        want.update({"k.w64": P.C64_F, "k.w64d": P.C64_D})
    assert modes == want and [key for key, *_ in P.items] == list(want)
    assert all(p is conv.weight for _, p, *_ in P.items)
    numel = {key: n for key, *_, n in P.items}
    assert numel["k.w"] == numel["k.wd"] == conv.weight.numel()
    if c64:
        assert numel["k.w64"] == numel["k.w64d"] == ops.conv64_pack_numel(cin, cout) > 0
