"""Host-side mirror of the reference's `SwinTransformer_MAE3D_New` (nerf_mae/model/mae/swin_mae3d.py:1067-1599;
imported there under the alias `SwinTransformer_MAE3D`, run_swin_mae3d.py:22).

Same constructor kwargs, `forward(list_of_grids, is_eval)` tuple contract, attribute contract used by nerf_rpn
(`patch_partition`, `pos_embed`, `stages`, deletable `decoder*`/`out`/`mask_token`; feature_extractor.py:1127-1187)
and `state_dict()` keys/shapes, so reference checkpoints load with strict=True and checkpoints written here load
into the reference.  The nn.Linear/Conv3d/LayerNorm children are *parameter holders only*: every forward and
backward op is a hand-written HIP kernel called through the C ABI (ops.py); activations stay channels-last
(B,A0,A1,A2,C) token-major matrices end to end (the reference's NCDHW round trips, swin_mae3d.py:1470, are gone).

Gradients: each block is one torch.autograd.Function with an explicit backward that launches the dgrad/wgrad
kernels; parameter gradients are accumulated by the kernels (fp32 atomics) straight into `param.grad`, which are
views of one flat fp32 buffer (likewise the parameters), so the optimizer and the data-parallel all-reduce work on
two flat buffers."""
from __future__ import annotations

import math
import random
import os
import struct
from functools import partial
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch
from torch import Tensor, nn

from . import ops
from .ops import WinGeom

WS = 4


# --------------------------------------------------------------------------------------------------
# fixed tables (restated from the reference's formulas; validated against golden vectors in tests)
# --------------------------------------------------------------------------------------------------
def _sincos_1d(dim: int, pos: np.ndarray) -> np.ndarray:
    omega = 1.0 / 10000 ** (np.arange(dim // 2, dtype=np.float64) / (dim / 2.0))
    ang = pos.reshape(-1).astype(np.float64)[:, None] * omega[None, :]
    return np.concatenate([np.sin(ang), np.cos(ang)], axis=1)


def sincos_pos_embed_3d(embed_dim: int, g: int) -> np.ndarray:
    """torch_utils.py:5-31: channel thirds encode (a1, a0, a2) of token (a0,a1,a2); zero-padded when 3*(C//3) < C
    (the defined swin_b deviation)."""
    third = embed_dim // 3
    third -= third % 2
    i, j, k = np.meshgrid(np.arange(g), np.arange(g), np.arange(g), indexing="ij")
    emb = np.concatenate([_sincos_1d(third, j), _sincos_1d(third, i), _sincos_1d(third, k)], axis=1)
    if emb.shape[1] < embed_dim:
        emb = np.concatenate([emb, np.zeros((emb.shape[0], embed_dim - emb.shape[1]))], axis=1)
    return emb.reshape(1, g, g, g, embed_dim)


def relative_position_index(ws: int = WS) -> Tensor:
    c = torch.stack(torch.meshgrid(*[torch.arange(ws)] * 3, indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]) + (ws - 1)
    m = 2 * ws - 1
    return (rel[0] * m * m + rel[1] * m + rel[2]).flatten()


def embed_capacity_rows(g: int, kept: Optional[int] = None, p_remove: Optional[float] = None, block: int = 4) -> int:
    """rows per sample of the compact patch embed (_EmbedFn) on a g^3 token grid: the kept count rounded up to 64-row granules when the mask is known (eager
    forward), or -- for a captured step, whose shapes are fixed before the masks are drawn -- the mean kept count of the block-Bernoulli mask
    (swin_mae3d.py:1366-1373) plus eight standard deviations (GraphedTrainStep checks every mask against it and re-captures with full capacity should one
    ever exceed it)"""
    tps = g ** 3
    if kept is None:
        nb = max(0, (g - block) // block + 1) ** 3
        keep = 1.0 - float(p_remove)
        kept = int(math.ceil(block ** 3 * (nb * keep + 8.0 * math.sqrt(max(nb * keep * (1.0 - keep), 0.0)) + 1.0))) + (tps - nb * block ** 3)
    return int(min(tps, max(64, -(-kept // 64) * 64)))


def mask_window_aligned(mask, ws: int = WS) -> bool:
    """True if the (g,g,g) token mask is constant on every ws^3 window of the unshifted partition and g is a multiple of ws: the condition under which stage 0's
    first block runs on the kept windows only (ops.BLOCK0_KEPT).  Tested on the host, where the mask is drawn."""
    m = np.asarray(mask, dtype=np.uint8)
    if m.ndim != 3 or len(set(m.shape)) != 1 or m.shape[0] == 0 or m.shape[0] % ws:
        return False
    nw = m.shape[0] // ws
    v = (m != 0).reshape(nw, ws, nw, ws, nw, ws)
    return bool((v == v[:, :1, :, :1, :, :1]).all())


class EmbedBound(NamedTuple):
    """what the caller that draws the masks promises about them (it answers for it: the model does not look at a mask on the device).  The default promises
    nothing: a row for every token, masks that may cut through windows."""
    rows: Optional[int] = None   # no mask keeps more tokens per sample than this (rows per sample of the compact patch embed); None: g^3
    aligned: bool = False        # every mask is constant on every 4^3 window (mask_window_aligned): stage 0's first block may run on the kept windows only


def bound_of_mask(g: int, mask) -> EmbedBound:
    """the bound of one known (g,g,g) mask (the eager forward, which draws its mask on the host): exactly the rows it needs, in 64-row granules"""
    m = np.asarray(mask)
    return EmbedBound(embed_capacity_rows(g, kept=g ** 3 - int(m.sum(dtype=np.int64))), mask_window_aligned(m))


def mask_kept_aligned(g: int, block_mask, bits=None):
    """(kept tokens, window-aligned) of a mask for `refit_bound`; bits: the (nb,nb,nb) block bits it travels as, if it does -- with nb * 4 == g every bit is
    one window, aligned without looking"""
    if bits is None:
        m = np.asarray(block_mask)
        return g ** 3 - int(m.sum()), mask_window_aligned(m)
    bits = np.asarray(bits)
    return g ** 3 - 64 * int(bits.sum()), bool(bits.shape[0] * 4 == g or mask_window_aligned(np.asarray(block_mask)))


def refit_bound(bound: EmbedBound, g: int, kept: int, aligned: bool) -> Optional[EmbedBound]:
    """a captured step and the next mask (`mask_kept_aligned`): None if the mask fits what was captured, else the bound to capture the step again with -- a row
    for every token if it keeps more than bound.rows (eight standard deviations above the mean kept count: not expected to happen in a training run), the dense
    first block if it cuts through 4^3 windows, both in ONE widened bound if it does both.  Pure."""
    rows = g ** 3 if bound.rows is not None and bound.rows < g ** 3 and kept > bound.rows else bound.rows
    new = EmbedBound(rows, bool(bound.aligned and aligned))
    return None if new == bound else new


def draw_block_bits(g: Sequence[int], p_remove: float, block: int = 4, rng=random) -> np.ndarray:
    """the draws of `draw_block_mask` only: uint8 array (nb0, nb1, nb2), 1 = block removed (same RNG stream, same order)"""
    nb = [max(0, (gi - block) // block + 1) for gi in g]
    return np.fromiter((rng.random() < p_remove for _ in range(nb[0] * nb[1] * nb[2])), dtype=np.uint8, count=nb[0] * nb[1] * nb[2]).reshape(nb)


def block_bits_of_mask(m, block: int = 4):
    """inverse of the block fill: (g,g,g) {0,1} mask -> its (nb,nb,nb) block bits, or None if the mask is not block-structured on a cube"""
    m = np.asarray(m, dtype=np.uint8)
    if m.ndim != 3 or len(set(m.shape)) != 1:
        return None
    nb = max(0, (m.shape[0] - block) // block + 1)
    bits = m[::block, ::block, ::block][:nb, :nb, :nb]
    full = np.zeros_like(m)
    if nb:
        full[:nb * block, :nb * block, :nb * block] = bits.repeat(block, 0).repeat(block, 1).repeat(block, 2)
    return bits if np.array_equal(full, m) else None


def draw_block_mask(g: Sequence[int], p_remove: float, block: int = 4, rng=random) -> Tensor:
    """swin_mae3d.py:1366-1373: one python-`random` draw per 4x4x4-token block in raster order -> uint8 (g0,g1,g2), 1 = removed.
    The draws keep the reference's order (same RNG stream, same pattern); only the block fill is vectorised (the per-block tensor
    slicing of a literal restatement costs 20-60 ms of host time per step and caps small-batch throughput)."""
    nb = [max(0, (gi - block) // block + 1) for gi in g]
    bits = np.fromiter((rng.random() < p_remove for _ in range(nb[0] * nb[1] * nb[2])), dtype=np.uint8, count=nb[0] * nb[1] * nb[2])
    m = np.zeros(tuple(g), dtype=np.uint8)
    if bits.size:
        blk = bits.reshape(nb).repeat(block, 0).repeat(block, 1).repeat(block, 2)
        m[:blk.shape[0], :blk.shape[1], :blk.shape[2]] = blk
    return torch.from_numpy(m)


# --------------------------------------------------------------------------------------------------
# packed compute-dtype weights
# --------------------------------------------------------------------------------------------------
class _Packer:
    """Owns the flat compute-dtype buffer holding every GEMM operand layout derived from the fp32 master
    parameters, and the device descriptor table for the single-launch pack kernel."""

    CAST, TRANS, CONV_F, CONV_D, CONVT_F, CONVT_D, C48_F, C48_D, C64_F, C64_D, PAD_ROWS, PAD_ROWS_T, PAD_CIN8 = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12
    C48_NUMEL = 41 * 3 * 64 * 8  # conv48.hip fragment order [step][ntile][lane][8]

    def __init__(self):
        self.items = []  # (key, param, mode, dims, numel)
        self.views = {}
        self.dec1 = None    # _Dec1Pack of the MAE decoder1 when its composed ConvTranspose o conv1 kernels apply
        self.swin_early = self.swin_late = None   # ctypes item arrays of the fused Swin-block weight streams (csrc/swin_block.hip), stages < / >= LATE_STAGE

    def add(self, key: str, p: nn.Parameter, mode: int):
        sh = tuple(p.shape)
        if mode in (self.CAST,):
            dims = (0, 0, 0)
        elif mode == self.TRANS:
            dims = (sh[0], int(np.prod(sh[1:])), 0)
        elif mode in (self.CONV_F, self.CONV_D, self.C48_F, self.C48_D, self.C64_F, self.C64_D):
            dims = (sh[0], sh[1], 27)
        else:
            dims = (sh[0], sh[1], int(np.prod(sh[2:])))
        numel = (self.C48_NUMEL * (sh[0] // 48) * (sh[1] // 48) if mode in (self.C48_F, self.C48_D)
                 else ops.conv64_pack_numel(sh[1], sh[0]) if mode in (self.C64_F, self.C64_D) else p.numel())
        if mode in (self.PAD_ROWS, self.PAD_ROWS_T):     # [Co][C] -> [Cop][C] / [C][Cop], Cop = Co rounded up to 8 (GEMM N granule)
            cop = (sh[0] + 7) // 8 * 8
            dims, numel = (sh[0], int(np.prod(sh[1:])), cop), cop * int(np.prod(sh[1:]))
        elif mode == self.PAD_CIN8:                      # conv weights [Co][Ci <= 8][taps] -> [Co][taps][8]
            dims, numel = (sh[0], sh[1], int(np.prod(sh[2:]))), sh[0] * int(np.prod(sh[2:])) * 8
        self.items.append((key, p, mode, dims, numel))

    def build(self, dtype: torch.dtype, device):
        total = sum((n + 63) // 64 * 64 for *_, n in self.items)
        self.buf = torch.empty(total, dtype=dtype, device=device)
        esz = self.buf.element_size()
        descs, blk2desc, blkstart = b"", [], []
        off = 0
        self.split = None   # first block of the decoder packs (they can be produced while the encoder runs)
        self.late = None    # first block of the encoder packs of stages >= LATE_STAGE (96 % of the encoder's elements; produced while stages 0/1 run)
        self._late_ev, self._late_pending = None, False
        for i, (key, p, mode, dims, n) in enumerate(self.items):
            if self.split is None and key.startswith("decoder"):
                self.split = len(blk2desc)
            if self.late is None and self.split is None and key.startswith(f"s{self.LATE_STAGE}."):
                self.late = len(blk2desc)
            self.views[key] = self.buf[off:off + n]
            descs += struct.pack("<QQiiiiq", p.data_ptr(), self.buf.data_ptr() + off * esz, mode, dims[0], dims[1], dims[2], n)
            if mode in (self.TRANS, self.CONV_F, self.CONV_D):   # tiled modes: blkstart = block id (nmh_pack_weights)
                nblk = {self.TRANS: ((dims[0] + 31) // 32) * ((dims[1] + 31) // 32), self.CONV_F: dims[0] * ((dims[1] + 31) // 32),
                        self.CONV_D: dims[1] * ((dims[0] + 31) // 32)}[mode]
                for k in range(nblk):
                    blk2desc.append(i)
                    blkstart.append(k)
            else:
                for s in range(0, n, 1024):
                    blk2desc.append(i)
                    blkstart.append(s)
            off += (n + 63) // 64 * 64
        self.descs = torch.frombuffer(bytearray(descs), dtype=torch.uint8).to(device)
        self.blk2desc = torch.tensor(blk2desc, dtype=torch.int32, device=device)
        self.blkstart = torch.tensor(blkstart, dtype=torch.int64, device=device)
        self.dt = ops.BF16 if dtype == torch.bfloat16 else ops.F32

    LATE_STAGE = 2

    def run(self, late_split: bool = True):
        """encoder layouts on the current stream; the decoder layouts (60 % of the elements, the stride-27 conv gathers) on the
        forked side stream, where they overlap the latency-bound encoder -- `join()` before the decoder reads them.  late_split: the
        encoder layouts of stages >= LATE_STAGE go to the side stream as well (first in its order), and `wait_late()` -- called by the
        model before such a stage runs -- makes the current stream wait for just that launch: the step starts 0.15 ms earlier at every
        batch size.  (False for callers that capture the stages into separate graphs: an event does not cross captures.)"""
        n = self.blk2desc.numel()
        side = ops.side_stream.enabled and os.environ.get("NMH_PACK_SPLIT", "1") != "0"
        sp = self.split if (self.split and side) else n
        lt = self.late if (self.late and side and late_split and sp < n and os.environ.get("NMH_PACK_LATE", "1") != "0") else sp
        self._late_pending = False
        if lt > 0:
            ops.pack_weights(self.dt, self.descs, self.blk2desc[:lt], self.blkstart[:lt], lt)
        if self.swin_early is not None:
            ops.swin_pack(self.swin_early)
        if self.swin_late is not None and not lt < sp:
            ops.swin_pack(self.swin_late)
        with ops.side_stream(enable=sp < n):
            if lt < sp:
                ops.pack_weights(self.dt, self.descs, self.blk2desc[lt:sp], self.blkstart[lt:sp], sp - lt)
                if self.swin_late is not None:
                    ops.swin_pack(self.swin_late)
                if self._late_ev is None:
                    self._late_ev = torch.cuda.Event()
                self._late_ev.record(torch.cuda.current_stream())
                self._late_pending = True
            if sp < n:
                ops.pack_weights(self.dt, self.descs, self.blk2desc[sp:], self.blkstart[sp:], n - sp)
            if self.dec1 is not None:
                self.dec1.pack()

    @staticmethod
    def join():
        ops.join_side()

    def wait_late(self):
        if self._late_pending:
            torch.cuda.current_stream().wait_event(self._late_ev)
            self._late_pending = False

    def __getitem__(self, key):
        return self.views[key]


class _Dec1Pack:
    """operands of the MAE decoder1's composed ConvTranspose o conv1 kernels (csrc/cconv.hip), derived from the fp32 masters on every `_Packer.run`;
    the optional buffers are None when the switch of the path that reads them was off at construction"""

    def __init__(self, block: "UpBlock3D", device):
        bf = dict(dtype=torch.bfloat16, device=device)
        self.block = block
        self.composed = torch.empty(ops.cconv_pack_numel(), **bf)                       # composed weights, fragment order of cconv_fwd
        self.border = torch.empty((27, 48), device=device)                              # border / delta table of the composed bias
        self.workspace = torch.empty(ops.cconv_pack_ws_floats(), dtype=torch.float32, device=device)   # the two weights as fp32 rows (cconv_wgrad reads it)
        self.upconv4 = torch.empty(ops.upconv4_pack_numel(), **bf)                      # transpose-conv fragments of the persistent upconv4_fwd
        self.dgrad = torch.empty(ops.cconv_dgrad_pack_numel(), **bf) if ops.CCONV_WGRAD else None    # composed weights, fragment order of cconv_dgrad
        self.mean_table = torch.empty((27, 96, 48), dtype=torch.float32, device=device) if ops.CCONV_CENTERED else None   # centered form: conv1's output mean
        self.tail_residual = torch.empty(ops.tail_residual_pack_numel(), **bf) if ops.TAIL_FROM_COARSE else None   # transpose-conv fragments of the tail

    def optional(self) -> frozenset:
        """names of the optional buffers held (an input of plan_up_block)"""
        return frozenset(n for n in ("dgrad", "mean_table", "tail_residual") if getattr(self, n) is not None)

    def pack(self):
        up = self.block
        Wt, W1, bt = up.transp_conv.weight, up.conv_block.conv1.weight, up.transp_conv.bias
        if self.mean_table is not None:   # + the table the centered forward's mean comes from
            ops.cconv_pack_centered(Wt, W1, bt, self.composed, self.border, self.workspace, self.mean_table)
        else:
            ops.cconv_pack(Wt, W1, bt, self.composed, self.border, self.workspace)
        ops.upconv4_pack(self.workspace, self.upconv4)
        if self.tail_residual is not None:   # the same weights as the fragments of the tail that forms the residual itself
            ops.tail_residual_pack(self.workspace, self.tail_residual)
        if self.dgrad is not None:
            ops.cconv_dgrad_pack(self.composed, self.dgrad)


def centered_wgrad_ok(B: int, S: int) -> bool:
    """the part of decoder1's centered-form gate that conv2's scaled weight gradient (ops.conv3d_k3_c48_wgrad_scaled) needs on a B x S^3 map: every one
    of its 8 XCD tile ranges of 4x4x16 tiles lies inside one sample (the entry refuses other shapes)"""
    return B in (1, 2, 4, 8) and S % 16 == 0 and ((S // 4) ** 2 * (S // 16)) % (8 // B) == 0


class UpSwitches(NamedTuple):
    """the `ops` switches and thresholds `plan_up_block` depends on, as plain values"""
    tail_from_coarse: bool
    tail_sign_mask: bool
    cconv_wgrad: bool
    cconv_centered: bool
    c48_bwd_reduce: bool
    inbwd_bg: bool
    defer_decoder_wgrad: bool
    side_stream: bool
    c48mb_min_voxels: int
    c64_min_voxels: int
    tail_box: bool = True

    @classmethod
    def current(cls) -> "UpSwitches":
        return cls(ops.TAIL_FROM_COARSE, ops.TAIL_SIGN_MASK, ops.CCONV_WGRAD, ops.CCONV_CENTERED, ops.C48_BWD_REDUCE, ops.INBWD_BG, ops.DEFER_DECODER_WGRAD,
                   ops.side_stream.enabled, ops.C48MB_MIN_VOXELS, ops.C64_MIN_VOXELS, ops.TAIL_BOX)


# conv family -> packed layouts of (conv1 forward, conv1 input gradient, conv2 forward, conv2 input gradient), in order of preference
_CONV_LAYOUTS = {
    "c48": ("c1.wk", "c1.wkd", "c2.wk", "c2.wkd"),          # Cin = Cout = 48 in bf16: LDS-halo kernel with fragment-ordered weights
    "c48mb": ("c1.wkm", "c1.wkmd", "c2.wkm", "c2.wkmd"),    # multiples of 48 at a volume that fills the chip (40^3, 96 / 192 channels): the same kernel on 48-channel blocks
    "c64": ("c1.w64", "c1.w64d", "c2.w64", "c2.w64d"),      # multiples of 64 (swin_b): LDS-halo kernel on 64-channel blocks
    "generic": ("c1.w", "c1.wd", "c2.w", "c2.wd"),
}


class UpPlan(NamedTuple):
    """which kernels one decoder level runs, forward and backward: decided once per forward by `plan_up_block`, kept on ctx (the layout of the saved tensors
    depends on it, and the switches it is derived from are module globals that a test or a caller may change between forward and backward)"""
    family: str              # key of _CONV_LAYOUTS; the four layout keys below are its row
    c1_fwd: str
    c1_dgrad: str
    c2_fwd: str
    c2_dgrad: str
    proj: bool               # skip connection concatenated, 1x1 projection on the residual branch (UpBlock3D ties both to use_skip)
    epilogue_stats: bool     # InstanceNorm statistics come out of the conv epilogue (no extra pass over the 160^3 tensor)
    composed_fwd: bool       # decoder1: y1 straight from the coarse map with the composed weights (4x fewer FLOPs; cat is only the residual)
    # decoder1: conv1's weight gradient through the composition (a quarter of the FLOPs, contraction over the coarse cells), and conv1's input gradient on the
    # fine grid is never formed -- dx and the transpose conv's parameter gradients take their conv1 part through the composition, dcat keeps the residual branch's alone
    composed_bwd: bool
    # centered form (csrc/cconv.hip): the mean of conv1's output comes from the coarse tensor, conv1 stores z = lrelu(y1 - mean) in place of y1 (a1 is not formed),
    # 1 / std goes into conv2's weights per sample; the backward reads z.  Needs the launches that read it (fused sums in conv2's input gradient, the background
    # InstanceNorm backward, the scaled weight-gradient reduce: B in {1, 2, 4, 8})
    centered: bool
    # decoder1 in training: the residual u = ConvT(x) is read by the tail forward alone (the composed kernels take conv1's passes through the coarse tensor, the
    # tail backward reads a sign mask), and the tail forms it from x on the matrix cores -- u (`cat`) is never stored (csrc/norm.hip: tail_fwd_coarse_kernel)
    residual_in_tail: bool
    fused_tail: bool         # d0 = lrelu(IN(y2) + cat) is consumed inside the tail kernels and rebuilt from (y2, cat) in the backward -- never stored
    x_grad: bool             # the tail forward writes d(pred) for the backward
    tail_bwd_sums: bool      # the reductions of the tail BACKWARD (InstanceNorm-backward sums, head weight gradient) are taken by the tail forward's pass
    sign_mask: bool          # ... and then the sign of d0 is all the tail backward still needs of it: 6 bytes per voxel instead of the residual row
    fused_reduce: bool       # the InstanceNorm-backward sums of (da1, y1) come out of conv2's input-gradient epilogue (no separate pass over both 160^3 tensors)
    # decoder1: the HBM-bound InstanceNorm backward (needs conv2's input gradient only) streams on a forked stream UNDER conv2's weight gradient, as one small
    # workgroup per CU beside the persistent kernel's (csrc/norm.hip: in_bwd_apply_bg_kernel); joined in front of its first consumer
    # (the transpose conv's input gradient, a 4000-workgroup GEMM, does not ride along: one of its workgroups per CU at a time crawls -- 2.7 ms for 0.64)
    bg_norm_bwd: bool
    # Conv weight gradients run on the forked side stream -- except the persistent 160^3 kernels (c48 / c64), which own every CU: overlapping them with the next
    # MFMA kernel OR with the HBM-bound InstanceNorm passes AS THEY ARE (100 k workgroups of 120 VGPRs) measured slower (51.2 vs 50.4 ms at 4 grids, 34.8 vs 30.8 ms
    # at 1), so they stay on the main stream; only the pass as ONE small workgroup per CU (bg_norm_bwd) does overlap.
    wgrad_main_stream: bool
    defer_conv_wgrad: bool   # small-level conv weight gradients: queued on the encoder's weight-gradient queue and issued with its next flush, one fork for all of them
    defer_upconv_wgrad: bool # the transpose conv's weight gradient likewise (decoder1 too: only its conv weight gradients stay out of the queue)
    # residual_in_tail on a batch whose target is ZERO outside each sample's extents (the model padded it: forward / forward_static), no pred asked for: the tail
    # forward walks, and the tail backward reads d(pred) and the sign mask in, the valid box of each sample alone -- d(pred) is exactly zero in the padding
    # (csrc/tail_box.hpp); neither is written outside the box
    tail_box: bool = False


class LossTail(NamedTuple):
    """the 1x1 head + loss attached to the last decoder level (_UpBlockFn.forward, built by _decode_and_loss)"""
    model: "SwinTransformer_MAE3D_New"
    xb: Optional[Tensor] = None        # the padded batch (B,4,R,R,R): the target
    extents: Optional[Tensor] = None   # [B,3] int32
    tokmask: Optional[Tensor] = None   # [g^3] uint8
    pred_out: Optional[Tensor] = None  # (B,4,R,R,R) to receive the prediction, or None
    zero_padded: bool = False          # the caller vouches that xb is zero outside each sample's extents (plan_up_block: tail_zero_padded)

    @classmethod
    def of(cls, tail) -> Optional["LossTail"]:
        """None, a LossTail, or the plain tuple (model, xb, extents, tokmask, pred_out[, zero_padded]) that callers passed before the record had names"""
        return tail if tail is None or isinstance(tail, cls) else cls(*tail)


def plan_up_block(cin: int, cout: int, k: int, has_proj: bool, layouts, dec1, B: int, v: int, dtype, x_grad: bool, tail: bool, tail_sums: bool,
                  has_queue: bool, sw: UpSwitches, tail_pred: bool = False, tail_zero_padded: bool = False) -> UpPlan:
    """layouts: the keys of _CONV_LAYOUTS' rows packed for the block; dec1: `_Dec1Pack.optional()` of the record built for THIS block, or None;
    tail / tail_sums: a loss tail is attached / its model's fuse_tail_sums; has_queue: the block has a weight-gradient queue; tail_pred: the tail is asked for
    pred; tail_zero_padded: the caller vouches that the tail's target is zero outside each sample's extents -- the precondition of `tail_box`, true where the
    model pads the batch itself (forward, forward_static behind the batcher) and nowhere else.  Pure: plain values in, UpPlan out."""
    S = v * k
    bf16 = dtype == torch.bfloat16
    fits = S ** 3 * (2 * cout if has_proj else cout) * 2 < 2 ** 32
    has = lambda fam: all(n in layouts for n in _CONV_LAYOUTS[fam])  # noqa: E731
    family = ("c48" if has("c48") else "c48mb" if has("c48mb") and S ** 3 >= sw.c48mb_min_voxels > 0 and fits
              else "c64" if has("c64") and S ** 3 >= sw.c64_min_voxels > 0 and fits else "generic")
    c48 = family == "c48"
    composed_fwd = c48 and dec1 is not None and v % 8 == 0 and not has_proj
    composed_bwd = composed_fwd and sw.cconv_wgrad and v <= 40 and "dgrad" in dec1
    fused_tail = tail and not has_proj
    tail_bwd_sums = tail and x_grad and tail_sums
    sign_mask = tail_bwd_sums and sw.tail_sign_mask and bf16 and cout == 48 and fused_tail and S % 4 == 0
    fused_reduce = c48 and sw.c48_bwd_reduce and S % 16 == 0
    centered = (composed_bwd and sw.cconv_centered and "mean_table" in dec1 and centered_wgrad_ok(B, S) and sw.c48_bwd_reduce and sw.inbwd_bg and sw.side_stream)
    residual_in_tail = (composed_bwd and sw.tail_from_coarse and "tail_residual" in dec1 and sign_mask and k == 4 and ops.tail_from_coarse_ok(S, cout, cin, dtype))
    queue = sw.defer_decoder_wgrad and has_queue
    main = family in ("c48", "c64")
    return UpPlan(family, *_CONV_LAYOUTS[family], proj=has_proj, epilogue_stats=main, composed_fwd=composed_fwd, composed_bwd=composed_bwd, centered=centered,
                  residual_in_tail=residual_in_tail, fused_tail=fused_tail, x_grad=x_grad, tail_bwd_sums=tail_bwd_sums, sign_mask=sign_mask, fused_reduce=fused_reduce,
                  bg_norm_bwd=centered or (fused_reduce and sw.inbwd_bg and cout == 48 and bf16 and sw.side_stream), wgrad_main_stream=main,
                  defer_conv_wgrad=queue and not main, defer_upconv_wgrad=queue,
                  tail_box=residual_in_tail and tail_bwd_sums and sign_mask and tail_zero_padded and not tail_pred and sw.tail_box)


class BlockSwitches(NamedTuple):
    """the `ops` switches and thresholds `plan_swin_block` and `flush_actions` depend on, as plain values"""
    swin_fused: bool
    swin_attn_widths: tuple
    swin_attn_min_windows: int
    swin_mlp_widths: tuple
    swin_mlp_min_rows: int
    mlp_fused: bool
    mlp_fused_widths: tuple
    mlp_fused_min_rows: int
    token_bwd: bool
    grouped_wgrad: bool
    flush_after_first: bool

    @classmethod
    def current(cls) -> "BlockSwitches":
        return cls(ops.SWIN_FUSED, ops.SWIN_ATTN_WIDTHS, ops.SWIN_ATTN_MIN_WINDOWS, ops.SWIN_MLP_WIDTHS, ops.SWIN_MLP_MIN_ROWS, ops.MLP_FUSED, ops.MLP_FUSED_WIDTHS,
                   ops.MLP_FUSED_MIN_ROWS, ops.TOKEN_BWD, ops.GROUPED_WGRAD, ops.WQ_FLUSH_AFTER_FIRST)


class BlockPlan(NamedTuple):
    """which kernels one Swin block runs, forward and backward: decided once per forward by `plan_swin_block`, kept on ctx (the layout of the saved tensors
    depends on it, and the switches it is derived from are module globals that a test or a caller may change between forward and backward)"""
    # "fused": LN1 -> QKV -> window attention -> proj -> row scale -> + residual in ONE launch (csrc/swin_block.hip); saves what the unfused chains save
    # "tokens": the unfused chain with token-ordered saves; "window": the unfused chain in window order
    attn: str
    # "lds": one launch with both weight matrices resident in LDS (csrc/mlp_fused.hip), nothing kept but x1 -- its backward recomputes the rest
    # "stream": one launch on packed weight streams (csrc/swin_block.hip), keeps h_pre and h_act for the unfused backward; "unfused": LN2, fc1 + GELU, fc2
    mlp: str
    # token-ordered backward (padded stages: 10^3 tokens in 12^3 window rows): window order stays inside the attention kernels, the Linear layers of the
    # attention branch see the real tokens only -- the forward then saves LN1(x) and o in token order, and the MLP backward forms no window-ordered dyw
    token_bwd: bool
    # weight / bias gradients are off the critical path.  True (bf16): they are queued (the operands stay referenced by the queue) and issued per stage as
    # grouped launches (ops.WgradQueue); False (fp32 parity mode): one launch each on the forked side stream, joined at the end of the block's backward
    queue_wgrad: bool


def plan_swin_block(C: int, heads: int, hidden: int, tokens: int, rows: int, B: int, dtype, x_grad: bool, has_streams: bool, mlp_lds_supported: bool,
                    has_queue: bool, sw: BlockSwitches) -> BlockPlan:
    """tokens / rows: real tokens / window-ordered rows (pads included) of all B samples; has_streams: the block has packed weight streams (SwinBlock3D._sw);
    mlp_lds_supported: ops.mlp_fused_supported(C); has_queue: the block has a weight-gradient queue.  Pure: plain values in, BlockPlan out."""
    assert tokens % B == 0 and rows % B == 0   # (the row scales and the queue's contraction splits are per sample)
    bf16 = dtype == torch.bfloat16
    # the kernels of csrc/swin_block.hip are built for heads = C / 32 and a hidden width of 4 C: anything else keeps the unfused chain.
    # Dispatch thresholds (tools/bench_swin_block.py): a fused workgroup is one dependent chain of ~45 us whatever the launch size, so launches that
    # cannot give most CUs a workgroup stay on the unfused kernels (one grid per GPU: 27 windows / 16 row tiles at stage 2)
    swin = sw.swin_fused and bf16 and has_streams and heads * 32 == C and hidden == 4 * C
    fused_attn = swin and C in sw.swin_attn_widths and rows // 64 >= sw.swin_attn_min_windows
    # LDS-resident MLP: bf16, a width that profits and enough rows to give every CU work (fewer: too few 64-row workgroups to fill the chip, the unfused chain
    # wins).  Measured (tools/bench_mlp_fused.py, 8 grids per GPU, forward + backward): C = 96 (persistent kernels, both weight matrices resident in LDS)
    # 187 + 478 us against 457 + 555 us for the unfused chain; the chunk-ring kernels win the forward at C = 192 (77 vs 136 us) but lose it back in the
    # backward (249 vs 204 us) and lose both at C = 384 (8000 rows = 125 workgroups, each a serial chain of 48 weight chunks) -- those widths stay off
    # sw.mlp_fused_widths; C = 192 / 384 take the stream kernel instead, C = 96 keeps this one
    lds = sw.mlp_fused and bf16 and C in sw.mlp_fused_widths and tokens >= sw.mlp_fused_min_rows and mlp_lds_supported
    stream = not lds and swin and C in sw.swin_mlp_widths and tokens >= sw.swin_mlp_min_rows
    # token_bwd requires mlp != "lds": that kernel's backward hands dx1 to the attention branch as the window-ordered dyw, the operand of the window-ordered
    # backward, and has no mode that leaves it out
    token_bwd = sw.token_bwd and rows != tokens and x_grad and not lds
    return BlockPlan(attn="fused" if fused_attn else "tokens" if token_bwd else "window", mlp="lds" if lds else "stream" if stream else "unfused",
                     token_bwd=bool(token_bwd), queue_wgrad=bool(sw.grouped_wgrad and bf16 and has_queue))


class EmbedSwitches(NamedTuple):
    """the `ops` switches `plan_embed` depends on, as plain values"""
    embed_kept: bool
    block0_kept: bool

    @classmethod
    def current(cls) -> "EmbedSwitches":
        return cls(ops.EMBED_KEPT, ops.BLOCK0_KEPT)


class EmbedPlan(NamedTuple):
    """what the patch embed and stage 0's first block run on: decided once per forward by `plan_embed`, kept on ctx like the other two plans"""
    # "dense": a row for every token
    # "rows": with a mask the embedding of a removed token is never read -- it is replaced by mask_token -- so the im2row, the GEMM rows, the LayerNorm rows and the
    #   weight-gradient contraction run on the KEPT tokens only, in compact rows [B][rows][.]; the output is the dense token grid
    # "windows": the kept windows + one representative all-mask window per sample, [B][capW + 1][64][.] (csrc/block0.hip): the patch embed's rows are the input rows
    #   of stage 0's first block, whose output _run_stage expands to the dense token grid
    path: str
    rows: int        # rows per sample of the im2row / GEMM / LayerNorm
    capW: int        # window slots per sample in front of the representative one (0 unless path == "windows")
    add_pos: bool    # + pos_embed inside the LayerNorm kernel


def plan_embed(g: int, mask: bool, add_pos: bool, capacity: Optional[int], aligned: bool, block0_ok: bool, sw: EmbedSwitches) -> EmbedPlan:
    """g^3 tokens per sample; mask: a token mask is applied; capacity / aligned: the caller's EmbedBound; block0_ok: stage 0 starts with an unshifted SwinBlock3D
    of a width ops.block0_supported takes.  Pure: plain values in, EmbedPlan out."""
    tps = g ** 3
    kept = mask and sw.embed_kept and add_pos
    if not kept:
        return EmbedPlan("dense", tps, 0, bool(add_pos))
    cap = min(tps, int(capacity)) if capacity else tps
    if sw.block0_kept and aligned and g % 4 == 0 and block0_ok:
        capW = max(1, min(cap // 64, (g // 4) ** 3))
        return EmbedPlan("windows", 64 * (capW + 1), capW, True)
    return EmbedPlan("rows", cap, 0, True)


def wgrad_queue_for(owner, dtype) -> Optional["ops.WgradQueue"]:
    """the weight-gradient queue of `owner` (the model or one of its blocks) if gradients of this compute dtype go through it -- the grouped kernel takes bf16
    operands -- else None: each weight gradient is then a launch of its own"""
    return owner._wq if ops.GROUPED_WGRAD and dtype == torch.bfloat16 else None


class FlushActions(NamedTuple):
    """what the backward of a stage boundary does with the weight-gradient queue (`flush_actions`), in this order"""
    join_before: bool
    request: bool      # leave the flush to the next block's backward, behind its first kernel; otherwise flush now
    foreground: bool   # a flush issued now runs (almost) alone and may split for the whole chip
    join_after: bool


def flush_actions(last: bool, sync_after_flush: bool, flush_after_first: bool) -> FlushActions:
    """last: the first stage -- its flush ends the backward pass and has the chip to itself; sync_after_flush: a gradient all-reduce of the range follows
    the flush (WgradQueue.sync_after_flush); flush_after_first: ops.WQ_FLUSH_AFTER_FIRST.  Pure."""
    # Joining the previous stage's launch here makes the next input-gradient kernel a successor of the side chain: the HIP graph executor then puts
    # the whole next main segment on the side chain's queue, BEHIND the weight gradients just flushed -- the trace showed the two queues alternating
    # (>= 2 kernels in flight for 4 of 52 ms).  With the late join the side chain only hangs off the main chain (fork edges), the operands stay
    # referenced by the queue until the end-of-backward join.
    join_before = sync_after_flush     # the previous stage's launch (if any) has had a whole stage of input-gradient work to finish under
    request = flush_after_first and not last and not sync_after_flush   # issued by the next block's backward behind its first kernel
    return FlushActions(join_before, request, foreground=last, join_after=sync_after_flush)


def _gradbuf(p: nn.Parameter) -> Tensor:
    if p.grad is None:
        p.grad = torch.zeros_like(p)
    return p.grad


# --------------------------------------------------------------------------------------------------
# autograd Functions (one per block; explicit backward launching the HIP dgrad/wgrad kernels)
# --------------------------------------------------------------------------------------------------
class _EmbedFn(torch.autograd.Function):
    """patch conv (im2row + GEMM) -> LayerNorm -> + pos_embed -> masked tokens <- mask_token (swin_mae3d.py:1455-1463), on the rows of the EmbedPlan given
    (model._embed / _embed_nomask).  Same values for every token that is read: the gradients of the compact paths differ from the full pass only by the order of
    fp32 sums.  Returns (tokens, wmap): wmap is the window map of the "windows" path, which _run_stage(0) needs, else None."""

    @staticmethod
    def forward(ctx, anchor, mod, xb, mask_dev, plan):
        m: "SwinTransformer_MAE3D_New" = mod
        p: EmbedPlan = plan
        m._wq.reset()   # first op of every forward pass: drops whatever a failed backward left queued
        B, R = xb.shape[0], xb.shape[2]
        g = R // 4
        tps = g ** 3
        C, dtype, dev = m.embed_dim, m.compute_dtype, xb.device
        rowmap = wmap = None
        if p.path == "windows":
            rowmap, wmap = ops.block0_window_rows(mask_dev, g, p.capW)
        elif p.path == "rows":
            rowmap = ops.embed_kept_rows(mask_dev, p.rows)
        A = torch.empty((B * p.rows, 256), dtype=dtype, device=dev)
        if rowmap is None:
            ops.patch_embed_gather(xb, A, B, R)
        else:
            ops.patch_embed_gather_kept(xb, A, B, R, rowmap, p.rows)
        conv, ln = m.patch_partition[0], m.patch_partition[2]
        y0 = ops.gemm_nt(A, m._pk["pe.w"].view(C, 256), bias=conv.bias)
        T = B * (p.rows if p.path == "windows" else tps)   # rows of the output: compact on the "windows" path alone
        tok = torch.empty((T, C), dtype=dtype, device=dev)
        mean, rstd = torch.empty(T, device=dev), torch.empty(T, device=dev)
        if p.path == "windows":
            ops.block0_embed_norm_fwd(y0, ln.weight, ln.bias, tok, mean, rstd, m.pos_embed.view(-1, C), m.mask_token, wmap, B, g, p.capW, C)
            ctx.mark_non_differentiable(wmap)
        elif p.path == "rows":
            ops.embed_norm_fwd_kept(y0, ln.weight, ln.bias, tok, mean, rstd, T, C, m.pos_embed.view(-1, C), mask_dev, m.mask_token, tps, rowmap, p.rows)
        else:
            ops.layernorm_fwd(y0, ln.weight, ln.bias, tok, mean, rstd, T, C, pos=m.pos_embed.view(-1, C) if p.add_pos else None,
                              mask=mask_dev, mask_token=m.mask_token if mask_dev is not None else None, tokens_per_sample=tps)
        ctx.m, ctx.plan, ctx.saved, ctx.dims = m, p, (A, y0, mean, rstd, mask_dev, rowmap, wmap), (B, g, C)
        return tok, wmap

    @staticmethod
    def backward(ctx, dtok, _dwmap=None):
        m, p = ctx.m, ctx.plan
        A, y0, mean, rstd, mask_dev, rowmap, wmap = ctx.saved
        B, g, C = ctx.dims
        tps = g ** 3
        conv, ln = m.patch_partition[0], m.patch_partition[2]
        dy0 = torch.empty_like(y0)
        if p.path == "windows":   # dtok: the compact input gradient of stage 0's first block
            ops.block0_embed_norm_bwd(dtok.contiguous(), y0, ln.weight, mean, rstd, dy0, _gradbuf(ln.weight), _gradbuf(ln.bias), _gradbuf(m.mask_token), wmap, B, g, p.capW, C)
        elif p.path == "rows":
            ops.embed_norm_bwd_kept(dtok.contiguous(), y0, ln.weight, mean, rstd, dy0, _gradbuf(ln.weight), _gradbuf(ln.bias), B * tps, C, mask_dev,
                                    _gradbuf(m.mask_token), tps, rowmap, p.rows)
        else:
            ops.layernorm_bwd(dtok.contiguous(), y0, ln.weight, mean, rstd, dy0, _gradbuf(ln.weight), _gradbuf(ln.bias), B * tps, C,
                              mask=mask_dev, dmask_token=_gradbuf(m.mask_token) if mask_dev is not None else None, tokens_per_sample=tps)
        q = wgrad_queue_for(m, dy0.dtype)
        if q is not None:
            q.add(dy0, A, _gradbuf(conv.weight).view(C, 256), dbias=_gradbuf(conv.bias), rows_per_sample=p.rows)
            q.flush(foreground=True)
            q.join()      # the backward pass ends here: every deferred weight gradient has been issued and joined
        else:
            ops.gemm_tn(dy0, A, _gradbuf(conv.weight), dbias=_gradbuf(conv.bias))
        return None, None, None, None, None


class _Block0ExpandFn(torch.autograd.Function):
    """compact output of stage 0's first block [B][capW + 1][64][C] -> the dense token grid [B g^3, C]: every removed window receives the rows of its sample's
    representative window (bit-identical to what the block computes for it).  Backward: the kept windows' gradients are copied, the representative row i receives
    the fp32 sum of row i of every removed window, in a fixed order (csrc/block0.hip)."""

    @staticmethod
    def forward(ctx, xc, wmap, B, g, capW):
        ctx.args = (wmap, B, g, capW, xc.shape[-1])
        return ops.block0_expand(xc.contiguous(), wmap, B, g, capW, xc.shape[-1])

    @staticmethod
    def backward(ctx, dy):
        wmap, B, g, capW, C = ctx.args
        return ops.block0_reduce(dy.contiguous(), wmap, B, g, capW, C), None, None, None, None


class _BlockSaved(NamedTuple):
    """what _BlockFn.forward keeps for its backward.  T = real tokens, rows = window-ordered rows (pads included) of the whole batch"""
    x: Tensor                  # [T, C] the block's input
    xnw: Tensor                # LN1(x): [T, C] in token order under plan.token_bwd, else [rows, C] in window order
    mean1: Tensor              # [T] fp32
    rstd1: Tensor
    qkv: Tensor                # [rows, 3 C] in window order, every plan (pad tokens are keys / values)
    o: Tensor                  # attention output in front of proj: [T, C] in token order under plan.token_bwd, else [rows, C] in window order
    lse: Tensor                # [rows * heads] fp32
    x1: Tensor                 # [T, C] x + SD(attn(LN1 x)): all the "lds" MLP keeps
    x1n: Optional[Tensor]      # [T, C] LN2(x1); this and the four below: None under plan.mlp == "lds" (its backward recomputes them)
    mean2: Optional[Tensor]    # [T] fp32
    rstd2: Optional[Tensor]
    h_pre: Optional[Tensor]    # [T, 4 C] fc1 output
    h_act: Optional[Tensor]    # [T, 4 C] gelu(h_pre)
    sd1: Optional[Tensor]      # [B] stochastic-depth row scales of the two branches (None: no scaling)
    sd2: Optional[Tensor]


class _BlockFn(torch.autograd.Function):
    """x + SD(attn(LN1 x)); x + SD(MLP(LN2 x))  (swin_mae3d.py:366-369).  Forward and backward follow the BlockPlan taken in forward."""

    @staticmethod
    def forward(ctx, x, blk, geom, sd1, sd2):
        b: "SwinBlock3D" = blk
        pk, key, sw = b._pk, b._key, b._sw
        T, C, heads = geom.tokens, b.dim, b.num_heads
        dev, dtype = x.device, x.dtype
        tps = T // geom.B
        p = b._plan(geom, dtype, ctx.needs_input_grad[0])
        if p.attn == "fused":
            x1, xnw, mean1, rstd1, qkv, o, lse = ops.swin_attn_fwd(x, b.norm1.weight, b.norm1.bias, sw[ops.SWIN_ATTN_FWD], b.attn.qkv.bias,
                                                                   b.attn.relative_position_bias_table, b.attn.proj.bias, geom, rowscale=sd1, rows_per_scale=tps,
                                                                   token_saves=p.token_bwd)
        elif p.attn == "tokens":
            # LN1 writes its window-ordered output (operand of the qkv product: pad tokens are keys / values) and a token-ordered copy (operand of the
            # qkv weight gradient); the attention core scatters o to token order, proj is a plain T-row GEMM
            xw = torch.empty((geom.rows, C), dtype=dtype, device=dev)
            xnw = torch.empty((T, C), dtype=dtype, device=dev)
            mean1, rstd1 = torch.empty(T, device=dev), torch.empty(T, device=dev)
            ops.layernorm_fwd_window_tokens(x, b.norm1.weight, b.norm1.bias, xw, xnw, mean1, rstd1, C, geom)
            qkv = ops.gemm_nt(xw, pk[key + "qkv.w"].view(3 * C, C), bias=b.attn.qkv.bias)
            o = torch.empty((T, C), dtype=dtype, device=dev)
            lse = torch.empty(geom.rows * heads, device=dev)
            ops.window_attn_fwd_tokens(qkv, b.attn.relative_position_bias_table, o, lse, heads, C, geom)
            x1 = ops.gemm_nt(o, pk[key + "proj.w"].view(C, C), bias=b.attn.proj.bias, resid=x, rowscale=sd1, rows_per_scale=tps)
        else:
            xnw = torch.empty((geom.rows, C), dtype=dtype, device=dev)
            mean1, rstd1 = torch.empty(T, device=dev), torch.empty(T, device=dev)
            ops.layernorm_fwd(x, b.norm1.weight, b.norm1.bias, xnw, mean1, rstd1, geom.rows, C, src_mode=1, geom=geom)
            qkv = ops.gemm_nt(xnw, pk[key + "qkv.w"].view(3 * C, C), bias=b.attn.qkv.bias)
            o = torch.empty((geom.rows, C), dtype=dtype, device=dev)
            lse = torch.empty(geom.rows * heads, device=dev)
            ops.window_attn_fwd(qkv, b.attn.relative_position_bias_table, o, lse, heads, C, geom)
            x1 = torch.empty_like(x)   # x1 = x + sd1 * window_reverse(proj(o)): the reverse + residual are the GEMM's store
            ops.gemm_nt_window_scatter(o, pk[key + "proj.w"].view(C, C), x1, x, b.attn.proj.bias, sd1, tps, geom)
        if p.mlp == "stream":
            x2, x1n, h_pre, mean2, rstd2, h_act = ops.swin_mlp_fwd(x1, b.norm2.weight, b.norm2.bias, sw[ops.SWIN_MLP_FWD], b.mlp[0].bias, b.mlp[3].bias,
                                                                  rowscale=sd2, rows_per_scale=tps, want_hact=True)
        elif p.mlp == "lds":
            x2 = ops.mlp_fused_fwd(x1, b.norm2.weight, b.norm2.bias, pk[key + "fc1.w"].view(4 * C, C), b.mlp[0].bias, pk[key + "fc2.wT"].view(4 * C, C),
                                   b.mlp[3].bias, rowscale=sd2, rows_per_scale=tps)
            x1n = mean2 = rstd2 = h_pre = h_act = None
        else:
            x1n = torch.empty_like(x)
            mean2, rstd2 = torch.empty(T, device=dev), torch.empty(T, device=dev)
            ops.layernorm_fwd(x1, b.norm2.weight, b.norm2.bias, x1n, mean2, rstd2, T, C)
            h_pre = torch.empty((T, 4 * C), dtype=dtype, device=dev)
            h_act = ops.gemm_nt(x1n, pk[key + "fc1.w"].view(4 * C, C), bias=b.mlp[0].bias, act=1, C2=h_pre)
            x2 = ops.gemm_nt(h_act, pk[key + "fc2.w"].view(C, 4 * C), bias=b.mlp[3].bias, resid=x1, rowscale=sd2, rows_per_scale=tps)
        ctx.b, ctx.geom, ctx.plan = b, geom, p
        ctx.saved = _BlockSaved(x, xnw, mean1, rstd1, qkv, o, lse, x1, x1n, mean2, rstd2, h_pre, h_act, sd1, sd2)
        return x2

    @staticmethod
    def backward(ctx, dx2):
        b, geom, p, s = ctx.b, ctx.geom, ctx.plan, ctx.saved
        pk, key = b._pk, b._key
        T, C, heads = geom.tokens, b.dim, b.num_heads
        tps, rpw = T // geom.B, geom.rows // geom.B
        x, sd1, sd2 = s.x, s.sd1, s.sd2
        dx2 = dx2.contiguous()
        q = b._wq if p.queue_wgrad else None

        def wgrad(A, Bm, lin, rowscale=None, rps=tps):
            if q is not None:
                q.add(A, Bm, _gradbuf(lin.weight), dbias=_gradbuf(lin.bias), rowscale=rowscale, rows_per_sample=rps)
            else:
                with ops.side_stream():
                    ops.gemm_tn(A, Bm, _gradbuf(lin.weight), rowscale=rowscale, rows_per_scale=rps, dbias=_gradbuf(lin.bias))
        # ---- MLP branch -> dx1, and dyw = sd1 * dx1 in window order (adjoint of the window reverse) unless the backward stays in token order
        dyw = None if p.token_bwd else torch.empty_like(s.xnw)
        if p.mlp == "lds":
            # one launch: recomputes LN2 / the hidden activations, writes the operands of the two weight gradients and dx1 (+ its window-ordered copy)
            dx1, x1n, h_act, dh = ops.mlp_fused_bwd(s.x1, dx2, b.norm2.weight, b.norm2.bias, pk[key + "fc1.w"].view(4 * C, C), b.mlp[0].bias,
                                                    pk[key + "fc2.wT"].view(4 * C, C), _gradbuf(b.norm2.weight), _gradbuf(b.norm2.bias),
                                                    rowscale=sd2, rows_per_scale=tps, dyw=dyw, dyw_scale=sd1, geom=geom)
            if q is not None:
                q.flush_due()   # the previous stage's weight gradients fork off BEHIND this stage's first input-gradient kernel (ops.WgradQueue.request_flush)
            wgrad(dx2, h_act, b.mlp[3], rowscale=sd2)
            wgrad(dh, x1n, b.mlp[0])
        else:
            dh = ops.gemm_nt(dx2, pk[key + "fc2.wT"].view(4 * C, C), act=2, C2=s.h_pre, rowscale=sd2, rows_per_scale=tps)
            if q is not None:
                q.flush_due()
            wgrad(dx2, s.h_act, b.mlp[3], rowscale=sd2)
            dx1n = ops.gemm_nt(dh, pk[key + "fc1.wT"].view(C, 4 * C))
            wgrad(dh, s.x1n, b.mlp[0])
            dx1 = torch.empty_like(x)
            # (dgamma / dbeta: partial sums now, reduced with the stage's weight gradients)
            ops.layernorm_bwd(dx1n, s.x1, b.norm2.weight, s.mean2, s.rstd2, dx1, _gradbuf(b.norm2.weight), _gradbuf(b.norm2.bias), T, C, dres=dx2,
                              geom=None if p.token_bwd else geom, tokens_per_sample=tps, dyw=dyw, dyw_scale=None if p.token_bwd else sd1, wq=q)
        # ---- attention branch
        dtab = _gradbuf(b.attn.relative_position_bias_table)
        if p.token_bwd:
            # s.xnw / s.o hold LN1(x) / the attention output in TOKEN order; every GEMM below has T rows
            do = ops.gemm_nt(dx1, pk[key + "proj.wT"].view(C, C), rowscale=sd1, rows_per_scale=tps)           # gradient of the attention output, token order
            wgrad(dx1, s.o, b.attn.proj, rowscale=sd1)
            dqkv = torch.empty((T, 3 * C), dtype=x.dtype, device=x.device)
            dq_pad = torch.empty_like(s.qkv)                                                                   # only its pad rows are written (and read)
            ops.window_attn_bwd_tokens(s.qkv, b.attn.relative_position_bias_table, do, s.lse, dqkv, dq_pad, dtab, heads, C, geom)
            dxn = ops.gemm_nt(dqkv, pk[key + "qkv.wT"].view(C, 3 * C))
            wgrad(dqkv, s.xnw, b.attn.qkv)
            g_qb = _gradbuf(b.attn.qkv.bias)
            if q is not None:   # the pad rows' share of the qkv bias gradient, with the stage's weight gradients (one launch for all blocks of the flush)
                q.add_pad_colsum(dq_pad, g_qb, geom)
            else:
                with ops.side_stream():
                    ops.window_pad_rows_colsum(dq_pad, g_qb, geom)
            dx = torch.empty_like(x)
            ops.layernorm_bwd(dxn, x, b.norm1.weight, s.mean1, s.rstd1, dx, _gradbuf(b.norm1.weight), _gradbuf(b.norm1.bias), T, C, dres=dx1, wq=q)
        else:
            # s.xnw / s.o and every gradient below are in window order (rows, pads included)
            do = ops.gemm_nt(dyw, pk[key + "proj.wT"].view(C, C))
            wgrad(dyw, s.o, b.attn.proj, rps=rpw)
            dqkv = torch.empty_like(s.qkv)
            ops.window_attn_bwd(s.qkv, b.attn.relative_position_bias_table, do, s.lse, dqkv, dtab, heads, C, geom)
            dxnw = ops.gemm_nt(dqkv, pk[key + "qkv.wT"].view(C, 3 * C))
            wgrad(dqkv, s.xnw, b.attn.qkv, rps=rpw)
            dx = torch.empty_like(x)
            ops.layernorm_bwd(dxnw, x, b.norm1.weight, s.mean1, s.rstd1, dx, _gradbuf(b.norm1.weight), _gradbuf(b.norm1.bias), T, C, src_mode=1, geom=geom,
                              dres=dx1, wq=q)
        # the block's own side-stream launches (fp32 parity mode) read temporaries of this block: join before they are released.  With the queue
        # (bf16) the operands stay referenced by it and NOTHING may be joined here: a join makes this block's successor wait for every weight
        # gradient the last flush put on the side stream -- the trace showed the two queues taking turns (>= 2 kernels in flight for 4 of 52 ms)
        if q is None:
            ops.join_side()
        return dx, None, None, None, None


class _StageFlushFn(torch.autograd.Function):
    """identity at the input of an encoder stage; its backward runs when the stage's input-gradient chain is complete and issues the
    weight gradients queued by the stage's blocks (and its patch merging) as grouped launches, as `flush_actions` says"""

    @staticmethod
    def forward(ctx, x, wq, last=False):
        ctx.wq, ctx.last = wq, last    # last: the first stage -- its flush ends the backward pass and has the chip to itself
        ctx.flush_after_first = BlockSwitches.current().flush_after_first
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        wq = ctx.wq
        act = flush_actions(ctx.last, wq.sync_after_flush, ctx.flush_after_first)
        if act.join_before:
            wq.join()
        if act.request:
            wq.request_flush()
        else:
            wq.flush(foreground=act.foreground)
        if act.join_after:
            wq.join()
        return g, None, None


class _Fork2Fn(torch.autograd.Function):
    """a feature map with two consumers (the next encoder stage and a decoder skip connection / the FPN neck): identity forward, the two
    incoming gradients are summed by a HIP kernel (autograd's own accumulation would be an ATen add on the dependent chain)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x), x.view_as(x)

    @staticmethod
    def backward(ctx, g1, g2):
        if g1 is None or g2 is None:
            return g1 if g2 is None else g2
        g1, g2 = g1.contiguous(), g2.contiguous()
        if g1.numel() % 8:
            return g1 + g2
        return ops.add(g1, g2)


class _MergeFn(torch.autograd.Function):
    """2x2x2 gather -> LayerNorm(8C) -> Linear(8C,2C,no bias)  (swin_mae3d.py:390-414)."""

    @staticmethod
    def forward(ctx, x, mod, geom):
        m: "PatchMerging3D" = mod
        Cin = m.dim
        H2, W2, D2 = (geom.H + 1) // 2, (geom.W + 1) // 2, (geom.D + 1) // 2
        rows = geom.B * H2 * W2 * D2
        xg = torch.empty((rows, 8 * Cin), dtype=x.dtype, device=x.device)
        mean, rstd = torch.empty(rows, device=x.device), torch.empty(rows, device=x.device)
        ops.layernorm_fwd(x, m.norm.weight, m.norm.bias, xg, mean, rstd, rows, 8 * Cin, src_mode=2, geom=geom)
        y = ops.gemm_nt(xg, m._pk[m._key + "red.w"].view(2 * Cin, 8 * Cin))
        ctx.m, ctx.geom, ctx.saved, ctx.rows = m, geom, (x, xg, mean, rstd), rows
        return y

    @staticmethod
    def backward(ctx, dy):
        m, geom, rows = ctx.m, ctx.geom, ctx.rows
        x, xg, mean, rstd = ctx.saved
        Cin = m.dim
        dy = dy.contiguous()
        dxg = ops.gemm_nt(dy, m._pk[m._key + "red.wT"].view(8 * Cin, 2 * Cin))
        q = wgrad_queue_for(m, dy.dtype)
        if q is not None:
            q.add(dy, xg, _gradbuf(m.reduction.weight), rows_per_sample=rows // geom.B)
        else:
            ops.gemm_tn(dy, xg, _gradbuf(m.reduction.weight))
        dx = torch.empty_like(x)
        ops.layernorm_bwd(dxg, x, m.norm.weight, mean, rstd, dx, _gradbuf(m.norm.weight), _gradbuf(m.norm.bias), rows, 8 * Cin, src_mode=2, geom=geom)
        return dx, None, None


def _conv3(family: str, X, W, Cout, stats_acc=None, **kw):
    """3x3x3 conv by the kernel of an UpPlan's family, W the packed layout of that family (_CONV_LAYOUTS)"""
    if family == "c48":
        return ops.conv3d_k3_c48(X, W, stats_acc=stats_acc, **kw)
    if family == "c64":
        return ops.conv3d_k3_c64(X, W, Cout, stats_acc=stats_acc, **kw)
    assert stats_acc is None   # (UpPlan.epilogue_stats: these two have no statistics epilogue)
    return (ops.conv3d_k3_c48mb if family == "c48mb" else ops.conv3d_k3)(X, W, Cout, **kw)


class _UpBlockFn(torch.autograd.Function):
    """ConvTranspose3d(k=s) -> cat(skip) -> UnetResBlock (unetr_block.py:57-71,193-200), channels-last."""

    @staticmethod
    def forward(ctx, x, skip, mod, B, v, tail=None):
        """tail (a LossTail): the block is the last decoder level and the 1x1 head + loss are
        evaluated here, so that backward can fuse the loss gradient with the backward of the last InstanceNorm; returns the
        loss triple instead of the feature map."""
        m: "UpBlock3D" = mod
        pk, key = m._pk, m._key
        k, Cin, Cout = m.k, m.cin, m.cout
        k3, S = k ** 3, v * k
        V = S ** 3
        dev, dtype = x.device, x.dtype
        p = ctx.plan = m._plan(B, v, dtype, ctx.needs_input_grad[0], tail)
        d1 = pk.dec1
        Cc = 2 * Cout if p.proj else Cout
        xc = x.view(B, v, v, v, Cin)
        new_acc = lambda: ops.acc_zeros((B, Cout, 2), dev)   # noqa: E731  (one slice per reduction: arena slices are single-use)
        # ---- residual branch: transpose conv (+ skip)
        cat = None
        if not p.residual_in_tail:
            cat = torch.empty((B * V, Cc), dtype=dtype, device=dev)
            if p.composed_fwd:   # decoder1: persistent kernel, coarse fragments in registers (csrc/cconv.hip)
                ops.upconv4_fwd(xc, d1.upconv4, m.transp_conv.bias, cat, B, v)
            else:
                ops.upconv_fwd(x, pk[key + "t.w"].view(k3 * Cout, Cin), m.transp_conv.bias, cat, B, v, k, Cin, Cout)   # pixel shuffle in the epilogue
        if p.proj:
            ops.copy_cols(skip.reshape(B * V, Cout), cat[:, Cout:])
        # ---- conv1 + statistics -> InstanceNorm -> LeakyReLU
        scratch = new_acc()
        st1 = torch.empty((B, Cout, 2), device=dev)
        if p.centered:
            mhat = ops.cconv_output_mean(xc, d1.mean_table, d1.border, B, v)
            y1 = ops.cconv_fwd_centered(xc, d1.composed, d1.border, mhat, B, v, stats_acc=scratch).view(B * V, Cout)   # (y1 holds z; statistics of y1 - mhat: mean ~ 0, rstd)
        elif p.composed_fwd:
            y1 = ops.cconv_fwd(xc, d1.composed, d1.border, B, v, stats_acc=scratch).view(B * V, Cout)
        else:
            y1 = _conv3(p.family, cat.view(B, S, S, S, Cc), pk[key + p.c1_fwd], Cout, stats_acc=scratch if p.epilogue_stats else None).view(B * V, Cout)
        if p.epilogue_stats:
            ops.instnorm_finalize(scratch, st1, B, V, Cout)
        else:
            ops.instnorm_stats(y1, st1, scratch, B, V, Cout)
        a1 = None
        if not p.centered:
            a1 = torch.empty_like(y1)
            ops.instnorm_apply(y1, st1, a1, B, V, Cout)
        # ---- conv2 + statistics
        st2 = torch.empty((B, Cout, 2), device=dev)
        scratch = new_acc()
        if p.centered:
            wk2 = torch.empty(B * ops.C48_IMG, dtype=dtype, device=dev)
            ops.conv48_pack_scaled(m.conv_block.conv2.weight, st1, wk2, B)
            y2 = ops.conv3d_k3_c48_per_sample(y1.view(B, S, S, S, Cout), wk2, stats_acc=scratch).view(B * V, Cout)
        else:
            y2 = _conv3(p.family, a1.view(B, S, S, S, Cout), pk[key + p.c2_fwd], Cout, stats_acc=scratch if p.epilogue_stats else None).view(B * V, Cout)
        if p.epilogue_stats:
            ops.instnorm_finalize(scratch, st2, B, V, Cout)
        else:
            ops.instnorm_stats(y2, st2, scratch, B, V, Cout)
        # ---- last InstanceNorm + residual + LeakyReLU: the block's output, or inside the tail
        y3 = st3 = None
        out = None if p.fused_tail else torch.empty_like(y2)
        if p.proj:
            y3 = ops.gemm_nt(cat, pk[key + "c3.w"].view(Cout, Cc))
            st3 = torch.empty((B, Cout, 2), device=dev)
            ops.instnorm_stats(y3, st3, new_acc(), B, V, Cout)
            ops.instnorm_apply(y2, st2, out, B, V, Cout, r=y3, stats_r=st3, rmode=2)
        elif not p.fused_tail:
            ops.instnorm_apply(y2, st2, out, B, V, Cout, r=cat, rmode=1)
        ctx.m, ctx.dims = m, (B, v)
        ctx.saved = (x, cat, y1, st1, a1, y2, st2, y3, st3, out)
        ctx.tail = None
        if tail is None:
            return out
        assert p.fused_tail
        model, xb, extents, tokmask, pred_out = tail.model, tail.xb, tail.extents, tail.tokmask, tail.pred_out
        lsums = torch.empty(8, dtype=torch.float64, device=dev)
        losses = torch.empty(3, device=dev)
        dpred = torch.empty((B * V, 4), device=dev) if p.x_grad else None
        bsum = torch.empty(B * Cout * 4 + 4 * Cout, dtype=torch.float64, device=dev) if p.tail_bwd_sums else None
        smask = torch.empty((B * V, 8), dtype=torch.uint8, device=dev) if p.sign_mask else None
        # the 1x1 head and the loss terms in the same pass over (y2, cat)
        if p.residual_in_tail:
            ops.mae_tail_fwd_from_coarse(y2, st2, xc, d1.tail_residual, m.transp_conv.bias, model.out.conv.weight, model.out.conv.bias, xb, extents, tokmask,
                                         B, S, Cout, lsums, losses, dpred, bsum, smask, pred=pred_out, box=p.tail_box)
        else:
            ops.mae_tail_fwd(y2, st2, cat, out, model.out.conv.weight, model.out.conv.bias, xb, extents, tokmask, B, S, Cout, lsums, losses,
                             pred_out, dpred, bwd_sums=bsum, sign_mask=smask)
        ctx.tail = (model, lsums, dpred, bsum, smask, extents if p.tail_box else None)
        return losses

    @staticmethod
    def backward(ctx, dout):
        m, p = ctx.m, ctx.plan
        B, v = ctx.dims
        x, cat, y1, st1, a1, y2, st2, y3, st3, out = ctx.saved
        pk, key = m._pk, m._key
        k, Cin, Cout = m.k, m.cin, m.cout
        k3, S = k ** 3, v * k
        V = S ** 3
        Cc = 2 * Cout if p.proj else Cout
        dev, dtype = x.device, x.dtype
        # ---- last InstanceNorm + residual (or the tail): dy2, and the residual branch's gradient into dcat
        sums2 = ops.acc_zeros((B, Cout, 2), dev)
        dy2 = torch.empty_like(y2)
        dcat = torch.empty((B * V, Cc), dtype=dtype, device=dev)
        if ctx.tail is not None:   # d(loss)/d(losses[0]) == 1 (the reference calls loss.backward()); d(d0) is never materialised
            model, lsums, dpred, bsum, smask, box_extents = ctx.tail
            ops.mae_tail_bwd(None, y2, st2, dpred, lsums, model.out.conv.weight, sums2, dy2, dcat,
                             _gradbuf(model.out.conv.weight), _gradbuf(model.out.conv.bias), B, V, Cout, r=None if p.sign_mask else cat, bwd_sums=bsum,
                             sign_mask=smask, extents=box_extents, R=S if box_extents is not None else None)
        elif p.proj:
            dout = dout.contiguous()
            sums3 = ops.acc_zeros((B, Cout, 2), dev)
            dy3 = torch.empty_like(y3)
            ops.instnorm_bwd_reduce(dout, out, y2, st2, sums2, B, V, Cout, r=y3, stats_r=st3, sums_r=sums3, rmode=2)
            ops.instnorm_bwd_apply(dout, out, y2, st2, sums2, dy2, B, V, Cout, r=y3, stats_r=st3, sums_r=sums3, rmode=2, dr=dy3)
        else:
            dout = dout.contiguous()
            ops.instnorm_bwd_reduce(dout, out, y2, st2, sums2, B, V, Cout, rmode=1)
            ops.instnorm_bwd_apply(dout, out, y2, st2, sums2, dy2, B, V, Cout, rmode=1, dr=dcat)  # dcat <- g (plain residual)
        # ---- conv2: input gradient, weight gradient beside the InstanceNorm backward behind conv1
        wgrad = ops.conv3d_k3_c48_wgrad if p.family == "c48" else ops.conv3d_k3_wgrad

        def side(fn):   # (UpPlan.wgrad_main_stream / defer_conv_wgrad)
            if p.defer_conv_wgrad:
                m._wq.defer(fn)
            else:
                with ops.side_stream(enable=not p.wgrad_main_stream):
                    fn()
        sums1 = ops.acc_zeros((B, Cout, 2), dev)
        dy2v = dy2.view(B, S, S, S, Cout)
        if p.fused_reduce:   # (centered form: y1 holds z = lrelu(conv1's output - mean))
            reduce = ops.conv3d_k3_c48_bwd_reduce_centered if p.centered else ops.conv3d_k3_c48_bwd_reduce
            da1 = reduce(dy2v, pk[key + p.c2_dgrad], y1, st1, sums1).view(B * V, Cout)
        else:
            da1 = _conv3(p.family, dy2v, pk[key + p.c2_dgrad], Cout).view(B * V, Cout)
        g_c2, g_c1 = _gradbuf(m.conv_block.conv2.weight), _gradbuf(m.conv_block.conv1.weight)
        dy1 = torch.empty_like(dy2)  # (dy2 is still being read by the side-stream wgrad)
        if p.bg_norm_bwd:
            with ops.side_stream():
                (ops.instnorm_bwd_apply_bg_centered if p.centered else ops.instnorm_bwd_apply_bg)(da1, y1, st1, sums1, dy1, B, V, Cout)
        if p.centered:
            ops.conv3d_k3_c48_wgrad_scaled(dy2v, y1.view(B, S, S, S, Cout), st1, g_c2)
        else:
            side(lambda: wgrad(dy2v, a1.view(B, S, S, S, Cout), g_c2))
        if not p.fused_reduce:
            ops.instnorm_bwd_reduce(da1, None, y1, st1, sums1, B, V, Cout, rmode=0)   # sign(a1) == sign(y1 - mean): a1 is not re-read
        if p.bg_norm_bwd:
            ops.join_side()
        else:
            ops.instnorm_bwd_apply(da1, None, y1, st1, sums1, dy1, B, V, Cout, rmode=0)
        # ---- conv1: input gradient into dcat, weight gradient -- or both through the composition (UpPlan.composed_bwd)
        dy1v = dy1.view(B, S, S, S, Cout)
        if p.composed_bwd:
            # all on the main stream: the persistent G kernel, then its reduce / border sums / chain rules
            ops.cconv_wgrad(x.view(B, v, v, v, Cin), dy1v, pk.dec1.workspace, m.transp_conv.bias, g_c1, B, v, dWt=_gradbuf(m.transp_conv.weight), dbt=_gradbuf(m.transp_conv.bias))
        else:
            _conv3(p.family, dy1v, pk[key + p.c1_dgrad], Cc, out=dcat.view(B, S, S, S, Cc), accumulate=not p.proj)
            side(lambda: wgrad(dy1v, cat.view(B, S, S, S, Cc), g_c1))
        if p.proj:
            ops.gemm_nt(dy3, pk[key + "c3.wT"].view(Cc, Cout), out=dcat, accumulate=True)
            g_c3 = _gradbuf(m.conv_block.conv3.weight)
            if p.defer_conv_wgrad:
                m._wq.defer(lambda: ops.gemm_tn(dy3, cat, g_c3))
            else:
                with ops.side_stream():
                    ops.gemm_tn(dy3, cat, g_c3)
        # ---- transpose conv (+ skip)
        dskip = None
        if p.proj and ctx.needs_input_grad[1]:   # (a skip of the frozen prefix needs none: model.frozen_stages)
            dskip = torch.empty((B * V, Cout), dtype=dtype, device=dev)
            ops.copy_cols(dcat[:, Cout:], dskip)
        dx = torch.empty((B * v ** 3, Cin), dtype=dtype, device=dev)
        ops.upconv_dgrad(dcat, pk[key + "t.wd"].view(Cin, k3 * Cout), dx, B, v, k, Cin, Cout)   # reads dcat through the pixel shuffle
        if p.composed_bwd:
            ops.cconv_dgrad(dy1, pk.dec1.dgrad, B, v, add=dx, out=dx)
        g_tw, g_tb = _gradbuf(m.transp_conv.weight), _gradbuf(m.transp_conv.bias)
        if p.defer_upconv_wgrad:
            m._wq.defer(lambda: ops.upconv_wgrad(dcat, x, g_tw, g_tb, B, v, k, Cin, Cout))
        else:
            with ops.side_stream():
                ops.upconv_wgrad(dcat, x, g_tw, g_tb, B, v, k, Cin, Cout)
            ops.join_side()
        return dx, dskip, None, None, None, None


class _LossFn(torch.autograd.Function):
    """UnetOutBlock 1x1 conv + forward_loss (swin_mae3d.py:1513-1549) fused; outputs (loss, loss_rgb, loss_alpha)."""

    @staticmethod
    def forward(ctx, d0, mod, xb, extents, tokmask, pred_out):
        m = mod
        B, R, Cd = xb.shape[0], xb.shape[2], d0.shape[1]
        sums = torch.empty(4, dtype=torch.float64, device=d0.device)
        losses = torch.empty(3, device=d0.device)
        ops.mae_loss_fwd(d0, m.out.conv.weight, m.out.conv.bias, xb, extents, tokmask, B, R, Cd, sums, losses, pred_out)
        ctx.m, ctx.saved, ctx.dims = m, (d0, xb, extents, tokmask, sums), (B, R, Cd)
        return losses

    @staticmethod
    def backward(ctx, dl):
        m = ctx.m
        d0, xb, extents, tokmask, sums = ctx.saved
        B, R, Cd = ctx.dims
        dd0 = torch.empty_like(d0)
        dp8 = torch.empty((d0.shape[0], 8), dtype=d0.dtype, device=d0.device)
        ops.mae_loss_bwd(d0, m.out.conv.weight, m.out.conv.bias, xb, extents, tokmask, B, R, Cd, sums, dd0, dp8,
                         _gradbuf(m.out.conv.weight), _gradbuf(m.out.conv.bias))
        return dd0, None, None, None, None, None


# --------------------------------------------------------------------------------------------------
# modules (parameter names/shapes == reference)
# --------------------------------------------------------------------------------------------------
class _Permute(nn.Module):  # placeholder for torchvision Permute (index 1 of patch_partition; no parameters)
    def __init__(self, dims):
        super().__init__()
        self.dims = dims


class PatchPartition(nn.Sequential):
    """Conv3d(4,C,k=4,s=4) -> channels-last -> LayerNorm (swin_mae3d.py:1120-1129); callable on (B,4,R,R,R) -> (B,g,g,g,C)
    as nerf_rpn uses it (feature_extractor.py:1179)."""

    def forward(self, x):
        m = self._owner()
        m._ensure_ready(x.device)
        tok = m._embed_nomask(x.float().contiguous(), add_pos=False)
        g = x.shape[2] // 4
        return tok.view(x.shape[0], g, g, g, -1)


class WindowAttention3D(nn.Module):
    def __init__(self, dim, window_size, shift_size, num_heads):
        super().__init__()
        self.window_size, self.shift_size, self.num_heads = window_size, shift_size, num_heads
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * WS - 1) ** 3, num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        self.register_buffer("relative_position_index", relative_position_index(WS))


class SwinBlock3D(nn.Module):
    def __init__(self, dim, num_heads, window_size, shift_size, mlp_ratio=4.0, stochastic_depth_prob=0.0, eps=1e-5):
        super().__init__()
        self.dim, self.num_heads, self.shift_size, self.sd_prob = dim, num_heads, list(shift_size), stochastic_depth_prob
        self.norm1 = nn.LayerNorm(dim, eps=eps)
        self.attn = WindowAttention3D(dim, window_size, shift_size, num_heads)
        self.norm2 = nn.LayerNorm(dim, eps=eps)
        hid = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(dim, hid), nn.GELU(), nn.Dropout(0.0), nn.Linear(hid, dim), nn.Dropout(0.0))

    _sw = None   # packed weight streams of the fused kernels, by kind (set by the model's _build_swin_streams for the widths csrc/swin_block.hip supports)
    _wq = None   # the model's weight-gradient queue (set by its _build_packer)

    def _plan(self, geom: WinGeom, dtype, x_grad: bool) -> BlockPlan:
        """plan_swin_block on this block's dimensions and packed streams, with the switches as they are now"""
        return plan_swin_block(self.dim, self.num_heads, self.mlp[0].out_features, geom.tokens, geom.rows, geom.B, dtype, x_grad, self._sw is not None,
                               ops.mlp_fused_supported(self.dim), self._wq is not None, BlockSwitches.current())

    def _sd_noise(self, B, device):
        if not self.training or self.sd_prob == 0.0:
            return None
        keep = 1.0 - self.sd_prob
        return torch.empty(B, device=device).bernoulli_(keep).div_(keep)

    def forward(self, x, sd_noise=None):
        """x: (B,H,W,D,C) channels-last."""
        B, H, W, D, C = x.shape
        geom = WinGeom(B, H, W, D, self.shift_size)
        if sd_noise is None:
            sd_noise = (self._sd_noise(B, x.device), self._sd_noise(B, x.device))
        y = _BlockFn.apply(x.reshape(-1, C), self, geom, sd_noise[0], sd_noise[1])
        return y.view(B, H, W, D, C)


class PatchMerging3D(nn.Module):
    def __init__(self, dim, eps=1e-5):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(8 * dim, 2 * dim, bias=False)
        self.norm = nn.LayerNorm(8 * dim, eps=eps)

    def forward(self, x):
        B, H, W, D, C = x.shape
        geom = WinGeom(B, H, W, D, [0, 0, 0])
        y = _MergeFn.apply(x.reshape(-1, C), self, geom)
        return y.view(B, (H + 1) // 2, (W + 1) // 2, (D + 1) // 2, 2 * C)


class _Stage(nn.Sequential):
    def forward(self, x):
        m = self._owner()
        m._ensure_ready(x.device)
        if x.dtype != m.compute_dtype:
            x = x.to(m.compute_dtype)
        q = wgrad_queue_for(m, m.compute_dtype)
        if q is not None and torch.is_grad_enabled() and x.requires_grad:
            x = _StageFlushFn.apply(x, q)
        m._packer.wait_late()   # the layouts of stages >= LATE_STAGE are produced on the side stream: a stage called on its own must wait for them too
        for mod in self:
            x = mod(x.contiguous())
        return x


class ResBlock3D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv1 = nn.Conv3d(cin, cout, 3, 1, 1)
        self.conv2 = nn.Conv3d(cout, cout, 3, 1, 1)
        if cin != cout:
            self.conv3 = nn.Conv3d(cin, cout, 1, 1)


class UpBlock3D(nn.Module):
    def __init__(self, cin, cout, k, use_skip=True):
        super().__init__()
        self.cin, self.cout, self.k, self.use_skip = cin, cout, k, use_skip
        self.transp_conv = nn.ConvTranspose3d(cin, cout, k, stride=k)
        self.conv_block = ResBlock3D(2 * cout if use_skip else cout, cout)
        self.has_proj = use_skip

    _wq = None   # the model's weight-gradient queue (set by its _build_packer; a block packed on its own, as by heads.py, has none)

    def _plan(self, B, v, dtype, x_grad, tail) -> UpPlan:
        """plan_up_block on this block's packed layouts, the LossTail of _UpBlockFn.forward (or None) and the switches as they are now"""
        pk, tail = self._pk, LossTail.of(tail)
        layouts = {n for row in _CONV_LAYOUTS.values() for n in row if self._key + n in pk.views}
        dec1 = pk.dec1.optional() if (pk.dec1 is not None and pk.dec1.block is self) else None
        return plan_up_block(self.cin, self.cout, self.k, self.has_proj, layouts, dec1, B, v, dtype, x_grad, tail is not None,
                             tail is not None and tail.model.fuse_tail_sums, self._wq is not None, UpSwitches.current(),
                             tail_pred=tail is not None and tail.pred_out is not None, tail_zero_padded=tail is not None and bool(tail.zero_padded))

    def forward(self, x, skip=None, tail=None):
        """channels-last (B,v,v,v,Cin) [+ skip (B,kv,kv,kv,Cout)] -> (B,kv,kv,kv,Cout), or the loss triple when `tail` is given"""
        B, v = x.shape[0], x.shape[1]
        S = v * self.k
        out = _UpBlockFn.apply(x.reshape(-1, self.cin), skip.reshape(-1, self.cout) if self.use_skip else None, self, B, v, LossTail.of(tail))
        return out if tail is not None else out.view(B, S, S, S, self.cout)


class OutBlock3D(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.conv = nn.Conv3d(cin, cout, 1)


class SwinTransformer_MAE3D_New(nn.Module):
    def __init__(self, patch_size: List[int], embed_dim: int, depths: List[int], num_heads: List[int], window_size: List[int],
                 mlp_ratio: float = 4.0, dropout: float = 0.0, attention_dropout: float = 0.0, stochastic_depth_prob: float = 0.1,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, block: Optional[Callable[..., nn.Module]] = None,
                 downsample_layer: Optional[Callable[..., nn.Module]] = None, expand_dim: bool = True, out_channels: int = 4,
                 input_ch_dim: int = 4, decoder_embed_dim: int = 768, masking_prob=0.50, resolution=160, drop_rate=0.10,
                 masking_strategy="random", compute_dtype: torch.dtype = torch.bfloat16):
        super().__init__()
        if list(patch_size) != [4, 4, 4] or list(window_size) != [WS] * 3 or not expand_dim or input_ch_dim != 4 or out_channels != 4:
            raise ValueError("the HIP path implements the configuration the reference trains: patch 4^3, window 4^3, expand_dim, 4->4 channels")
        if dropout != 0.0 or attention_dropout != 0.0:
            raise ValueError("dropout/attention_dropout are 0 in every reference config (run_swin_mae3d.py:400-411)")
        if any(embed_dim * 2 ** s != num_heads[s] * 32 for s in range(len(depths))):
            raise ValueError("head_dim must be 32 (all reference backbones; swin_b uses heads [4,8,16,32], SURVEY 8(c))")
        if embed_dim % 16:
            raise ValueError("embed_dim must be a multiple of 16")
        self.out_channels, self.embed_dim, self.patch_size = out_channels, embed_dim, list(patch_size)
        self.masking_prob, self.resolution, self.compute_dtype = masking_prob, resolution, compute_dtype
        owner = lambda: self  # noqa: E731  (children reach the model without registering it as a submodule)
        self.patch_partition = PatchPartition(nn.Conv3d(4, embed_dim, 4, 4), _Permute([0, 2, 3, 4, 1]), nn.LayerNorm(embed_dim, eps=1e-5))
        self.patch_partition._owner = owner
        self.stages = nn.ModuleList()
        total, bid = sum(depths), 0
        for s, depth in enumerate(depths):
            dim = embed_dim * 2 ** s
            mods: List[nn.Module] = [PatchMerging3D(dim // 2)] if s > 0 else []
            for i in range(depth):
                sd = stochastic_depth_prob * float(bid) / (total - 1)
                mods.append(SwinBlock3D(dim, num_heads[s], list(window_size), [0] * 3 if i % 2 == 0 else [WS // 2] * 3, mlp_ratio, sd))
                bid += 1
            st = _Stage(*mods)
            st._owner = owner
            self.stages.append(st)
        E = embed_dim
        self.decoder4 = UpBlock3D(8 * E, 4 * E, 2)
        self.decoder3 = UpBlock3D(4 * E, 2 * E, 2)
        self.decoder2 = UpBlock3D(2 * E, E, 2)
        self.decoder1 = UpBlock3D(E, E // 2, 4, use_skip=False)
        self.out = OutBlock3D(E // 2, out_channels)
        self.num_patches = g = resolution // patch_size[0]
        self.pos_embed = nn.Parameter(torch.zeros(1, g, g, g, E), requires_grad=False)
        self.mask_token = nn.Parameter(torch.zeros(E))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        self.pos_embed.data.copy_(torch.from_numpy(sincos_pos_embed_3d(E, g)).float())
        nn.init.normal_(self.mask_token, std=0.02)
        self._flat = self._flat_grad = None
        self._packer = None
        self._anchor = None
        self._reducer = None  # dist.GradReducer when data-parallel
        self._frozen_stages = 0  # the frozen prefix: patch embed + stages[:k] run without a graph (frozen_stages)

    @property
    def frozen_stages(self) -> int:
        """k: the patch embed (patch_partition, mask_token) and stages[:k] are a frozen prefix -- they run with autograd off in whatever mode they are in (train():
        the stochastic-depth factors of the one _draw_sd_noise draw), keep nothing for a backward, get no weight-gradient flush and no reducer trigger, and the
        backward pass ends at the input of stage k.  Their gradient views are never written.  0: no prefix.  Fine-tuning only (forward_encoder and the callers of
        _embed_nomask); the optimizer side is finetune.frozen_stage_rules."""
        return self._frozen_stages

    @frozen_stages.setter
    def frozen_stages(self, k):
        n = len(self.stages)
        if isinstance(k, bool) or int(k) != k or not 0 <= int(k) <= n:
            raise ValueError(f"frozen_stages = {k!r}: an integer from 0 (nothing frozen) to {n} (the patch embed and all {n} stages); to freeze anything but a "
                             "leading prefix use freeze= (finetune.freeze_rules)")
        self._frozen_stages = int(k)

    def refuse_frozen_stages(self, who: str):
        """the MAE pre-training path does not implement the frozen prefix: refuse instead of training something untested"""
        if self._frozen_stages:
            raise ValueError(f"{who}: the encoder has frozen_stages = {self._frozen_stages}; the MAE pre-training path does not implement the frozen prefix -- set "
                             "frozen_stages = 0 (freeze= still keeps ranges from being stepped), or fine-tune through finetune.FinetuneStep")

    def _embed_nomask(self, xb: Tensor, add_pos: bool = True) -> Tensor:
        """the unmasked patch embed of the downstream models -> (B g^3, C) tokens; under a frozen prefix without a graph (no _EmbedFn context is kept)"""
        p = self._plan_embed(xb.shape[2] // 4, False, add_pos)
        if self._frozen_stages:
            with torch.no_grad():
                return _EmbedFn.apply(self._anchor, self, xb, None, p)[0]
        return _EmbedFn.apply(self._anchor, self, xb, None, p)[0]

    def _plan_embed(self, g: int, mask: bool, add_pos: bool = True, bound: Optional[EmbedBound] = None) -> EmbedPlan:
        """plan_embed on this model's first block, the caller's bound (None: EmbedBound(), which promises nothing) and the switches as they are now"""
        bound = bound or EmbedBound()
        b0 = self.stages[0][0] if len(self.stages) and len(self.stages[0]) else None
        block0_ok = bool(mask and bound.aligned and isinstance(b0, SwinBlock3D) and not any(b0.shift_size)
                         and ops.block0_supported(self.embed_dim))   # (the library is asked only where the answer can matter)
        return plan_embed(g, mask, add_pos, bound.rows, bound.aligned, block0_ok, EmbedSwitches.current())

    def _embed(self, xb: Tensor, mask_dev: Tensor, bound: Optional[EmbedBound] = None):
        """patch embed of a masked batch -> (the input of stage 0, b0).  b0 = None: the dense token grid (B,g,g,g,C); kept-window path: the compact rows as the
        grid (B, 4 (capW + 1), 4, 4, C) whose token order is its window order, and b0 = (wmap, g, capW), which _run_stage(0) takes.  The caller answers for
        `bound`: it draws the masks."""
        B, g = xb.shape[0], xb.shape[2] // 4
        p = self._plan_embed(g, True, bound=bound)
        tok, wmap = _EmbedFn.apply(self._anchor, self, xb, mask_dev, p)
        if p.path == "windows":
            return tok.view(B, 4 * (p.capW + 1), 4, 4, self.embed_dim), (wmap, g, p.capW)
        return tok.view(B, g, g, g, self.embed_dim), None

    # ---- flat buffers + packed weights ------------------------------------------------------------
    def _trainable(self):
        """trainable parameters in *gradient-completion-friendly* order: [mask_token, patch embed | stage0..3 | decoders, head]
        (mask_token's gradient is produced by the embed backward, i.e. last, so it sits with the embed segment)"""
        ps = [self.mask_token] if "mask_token" in self._parameters else []
        seen = {id(p) for p in ps}
        for p in self.parameters():
            if p.requires_grad and id(p) not in seen:
                ps.append(p)
                seen.add(id(p))
        return ps

    def flat_numel(self) -> int:
        """length of the flat buffer `flatten_parameters` fills: every trainable parameter rounded up to an 8-element granule"""
        return sum((p.numel() + 7) // 8 * 8 for p in self._trainable())   # 8-element granules: every segment boundary is 16-byte aligned in fp32 AND in bf16 buckets

    def flatten_parameters(self, device=None, out=None):
        """Re-home every trainable parameter (and its .grad) as a view of one flat fp32 buffer.  out=(flat, grad): fill this storage (two contiguous fp32
        vectors of flat_numel() elements, e.g. the leading slices of finetune.FlatParameters' buffers) instead of allocating; the granule gaps are cleared."""
        ps = self._trainable()
        n = self.flat_numel()
        if out is None:
            device = device or ps[0].device
            flat = torch.zeros(n, device=device)
            fg = torch.zeros(n, device=device)
        else:
            flat, fg = out
            for t in (flat, fg):
                if t.dtype != torch.float32 or t.dim() != 1 or t.numel() != n or not t.is_contiguous():
                    raise ValueError(f"flatten_parameters: out must be two contiguous fp32 vectors of flat_numel() = {n} elements")
            device = flat.device
            fg.zero_()
        off = 0
        self._offsets = {}
        for p in ps:
            k = p.numel()
            flat[off:off + k].copy_(p.data.reshape(-1))
            p.data = flat[off:off + k].view(p.shape)
            p.grad = fg[off:off + k].view(p.shape)
            self._offsets[id(p)] = off
            if out is not None and k % 8:
                flat[off + k:off + (k + 7) // 8 * 8].zero_()
            off += (k + 7) // 8 * 8
        self._flat, self._flat_grad = flat, fg
        self._build_packer(device)
        return flat, fg

    def _build_packer(self, device):
        P = _Packer()
        P.add("pe.w", self.patch_partition[0].weight, P.CAST)
        for s, st in enumerate(self.stages):
            for i, mod in enumerate(st):
                key = f"s{s}.{i}."
                mod._key = key
                if isinstance(mod, PatchMerging3D):
                    P.add(key + "red.w", mod.reduction.weight, P.CAST)
                    P.add(key + "red.wT", mod.reduction.weight, P.TRANS)
                else:
                    for nm, lin in (("qkv", mod.attn.qkv), ("proj", mod.attn.proj), ("fc1", mod.mlp[0]), ("fc2", mod.mlp[3])):
                        P.add(key + nm + ".w", lin.weight, P.CAST)
                        P.add(key + nm + ".wT", lin.weight, P.TRANS)
        for name in ("decoder4", "decoder3", "decoder2", "decoder1"):
            if not hasattr(self, name):
                continue
            d = getattr(self, name)
            key = name + "."
            d._key = key
            P.add(key + "t.w", d.transp_conv.weight, P.CONVT_F)
            P.add(key + "t.wd", d.transp_conv.weight, P.CONVT_D)
            for cn in ("c1", "c2"):
                conv = getattr(d.conv_block, "conv" + cn[1])
                P.add(key + cn + ".w", conv.weight, P.CONV_F)
                P.add(key + cn + ".wd", conv.weight, P.CONV_D)
                if self.compute_dtype == torch.bfloat16 and tuple(conv.weight.shape[:2]) == (48, 48):
                    P.add(key + cn + ".wk", conv.weight, P.C48_F)     # specialised LDS-halo kernel (decoder1 @160^3)
                    P.add(key + cn + ".wkd", conv.weight, P.C48_D)
                elif (self.compute_dtype == torch.bfloat16 and conv.weight.shape[0] % 48 == 0 and conv.weight.shape[1] % 48 == 0
                      and (d.k * (self.resolution // 4) // {"decoder4": 8, "decoder3": 4, "decoder2": 2, "decoder1": 1}[name]) ** 3 >= ops.C48MB_MIN_VOXELS > 0):
                    P.add(key + cn + ".wkm", conv.weight, P.C48_F)    # the LDS-halo kernel on 48-channel blocks (swin_t/s decoder level 40^3)
                    P.add(key + cn + ".wkmd", conv.weight, P.C48_D)
                elif (self.compute_dtype == torch.bfloat16 and conv.weight.shape[0] % 64 == 0 and conv.weight.shape[1] % 64 == 0
                      and (d.k * (self.resolution // 4) // {"decoder4": 8, "decoder3": 4, "decoder2": 2, "decoder1": 1}[name]) ** 3 >= ops.C64_MIN_VOXELS > 0):
                    P.add(key + cn + ".w64", conv.weight, P.C64_F)    # 64-channel-block LDS-halo kernel (swin_b decoder levels >= 32^3)
                    P.add(key + cn + ".w64d", conv.weight, P.C64_D)
            if d.has_proj:
                P.add(key + "c3.w", d.conv_block.conv3.weight, P.CAST)
                P.add(key + "c3.wT", d.conv_block.conv3.weight, P.TRANS)
        P.build(self.compute_dtype, device)
        self._build_swin_streams(P, device)
        d1 = getattr(self, "decoder1", None)
        if (ops.CCONV and d1 is not None and self.compute_dtype == torch.bfloat16 and (d1.cin, d1.cout, d1.k) == (96, 48, 4) and not d1.has_proj
                and (self.resolution // 4) % 8 == 0):
            P.dec1 = _Dec1Pack(d1, device)
        self._packer = P
        self._pk = P
        self._wq = ops.WgradQueue()   # deferred encoder weight gradients (grouped launches, issued per stage)
        for mod in self.modules():
            if isinstance(mod, (SwinBlock3D, PatchMerging3D, UpBlock3D)):
                mod._pk = P
                mod._wq = self._wq
        self._anchor = torch.zeros(1, device=device, requires_grad=True)

    def _build_swin_streams(self, P, device):
        """weight streams of the fused Swin-block kernels (csrc/swin_block.hip) for every block of a supported width: one flat bf16 buffer, packed from
        the fp32 masters by one launch per group (stages < / >= LATE_STAGE, like the other encoder layouts)"""
        if not (ops.SWIN_FUSED and self.compute_dtype == torch.bfloat16):
            return
        kinds = [ops.SWIN_ATTN_FWD, ops.SWIN_MLP_FWD]
        src = {ops.SWIN_ATTN_FWD: lambda b: (b.attn.qkv.weight, b.attn.proj.weight), ops.SWIN_MLP_FWD: lambda b: (b.mlp[0].weight, b.mlp[3].weight)}
        blocks = [(s, b) for s, st in enumerate(self.stages) for b in st if isinstance(b, SwinBlock3D) and ops.swin_supported(b.dim)]
        total = sum((ops.swin_stream_numel(k, b.dim) + 63) // 64 * 64 for _, b in blocks for k in kinds)
        if not total:
            return
        buf = torch.empty(total, dtype=torch.bfloat16, device=device)
        early, late, off = [], [], 0
        for s, b in blocks:
            b._sw = {}
            for k in kinds:
                n = ops.swin_stream_numel(k, b.dim)
                b._sw[k] = buf[off:off + n]
                w0, w1 = src[k](b)
                (late if s >= _Packer.LATE_STAGE else early).append((w0.data, w1.data if w1 is not None else None, b._sw[k], k, b.dim))
                off += (n + 63) // 64 * 64
        P.swin_buf = buf
        P.swin_early = ops.swin_pack_items(early) if early else None
        P.swin_late = ops.swin_pack_items(late) if late else None

    def _ensure_ready(self, device):
        ps = self._trainable()
        stale = (self._flat is None or self._flat.device != ps[0].device or
                 any(p.data_ptr() != self._flat.data_ptr() + 4 * self._offsets.get(id(p), -1) for p in ps))
        if stale:
            if not ps[0].is_cuda:
                raise RuntimeError("SwinTransformer_MAE3D (HIP) needs its parameters on a HIP device: call .cuda() first (no CPU fallback)")
            self.flatten_parameters()
        self._packer.run()

    def zero_grad(self, set_to_none: bool = False):
        if self._flat_grad is not None:
            self._flat_grad.zero_()
        else:
            super().zero_grad(set_to_none=set_to_none)

    # ---- reference API ----------------------------------------------------------------------------
    def transform(self, x: List[Tensor], device):
        """pad_tensor semantics (torch_utils.py:56-90) without materialising the ones-mask: returns the padded
        batch (B,4,R,R,R) fp32 and the valid extents [B,3] (the analytic mask)."""
        R = self.resolution
        xb = torch.zeros((len(x), 4, R, R, R), dtype=torch.float32, device=device)
        ext = []
        for i, t in enumerate(x):
            a0, a1, a2 = t.shape[1:]
            xb[i, :, :a0, :a1, :a2] = t.to(device=device, dtype=torch.float32, non_blocking=True)
            ext.append([a0, a1, a2])
        return xb, torch.tensor(ext, dtype=torch.int32).to(device, non_blocking=True)

    def _draw_sd_noise(self, B: int, device):
        """row-mode stochastic-depth factors of every block (attention and MLP branch) in TWO launches instead of four per block
        (torchvision StochasticDepth(p, "row"): bernoulli(1-p)/(1-p) per sample, swin_mae3d.py:390-414)"""
        blocks = [m for st in self.stages for m in st if isinstance(m, SwinBlock3D)]
        if not self.training or all(b.sd_prob == 0.0 for b in blocks):
            return None
        keep = getattr(self, "_sd_keep", None)
        if keep is None or keep.device != device or keep.shape[1] != B:
            k = torch.tensor([1.0 - b.sd_prob for b in blocks for _ in (0, 1)], device=device)
            keep = self._sd_keep = k[:, None].expand(-1, B).contiguous()
        noise = torch.bernoulli(keep).div_(keep)
        return [(noise[2 * i], noise[2 * i + 1]) for i in range(len(blocks))]

    def _run_stage(self, si: int, x: Tensor, sd_noise, bi: int, red=None, b0=None):
        """stage `si` on channels-last x; `bi` = index of the stage's first block in `sd_noise`.  Returns (output, next block index).
        b0 (stage 0): the (wmap, g, capW) of _embed -- x holds compact rows, the first block runs on them and its output is expanded to the dense token grid.
        With a data-parallel reducer the stage (each block group of the chunked stage, dist.GradReducer) is preceded by the trigger that
        launches its gradient range's all-reduce -- backward order: blocks of the group, the flush that issues (and joins) their queued weight
        gradients, then the trigger."""
        if si >= _Packer.LATE_STAGE:
            self._packer.wait_late()
        q = wgrad_queue_for(self, self.compute_dtype) if torch.is_grad_enabled() and x.requires_grad else None
        groups = red.chunk_groups if (red is not None and si == getattr(red, "chunk_stage", -1) and red.chunk_groups) else [list(self.stages[si])]
        for k, grp in enumerate(groups):
            if red is not None:
                x = red.trigger(x, red.seg_stage(si, k))  # backward reaching here => this range's gradients are complete
            if q is not None:
                x = _StageFlushFn.apply(x, q, si == self._frozen_stages and k == 0)   # the first live stage's flush ends the backward pass
            for mod in grp:
                if isinstance(mod, SwinBlock3D):
                    x = mod(x, None if sd_noise is None else sd_noise[bi])
                    bi += 1
                    if b0 is not None:
                        (wmap, g, capW), b0 = b0, None
                        x = _Block0ExpandFn.apply(x.reshape(-1, x.shape[-1]), wmap, x.shape[0], g, capW).view(x.shape[0], g, g, g, x.shape[-1])
                else:
                    x = mod(x)
        return x, bi

    def forward_encoder(self, tok: Tensor, sd_noise=None, b0=None):
        """b0: what _embed returned beside `tok` (None: tok is the dense token grid)"""
        feats, x, bi = [], tok, 0
        red = self._reducer
        if sd_noise is None:
            sd_noise = self._draw_sd_noise(tok.shape[0], tok.device)
        self._wq.sync_after_flush = red is not None   # a gradient all-reduce of the range follows the flush: join before it
        nf = self._frozen_stages
        for si in range(len(self.stages)):
            if si < nf:
                # the frozen prefix: no graph, no flush, no trigger, no fork -- the feature goes to the neck / decoder as it is
                with torch.no_grad():
                    x, bi = self._run_stage(si, x, sd_noise, bi, None, b0 if si == 0 else None)
                feats.append(x)
                if si + 1 == nf and si + 1 < len(self.stages) and torch.is_grad_enabled():
                    # the boundary: a leaf that requires a gradient, so that the first live stage keeps its plans (plan_swin_block: x_grad) and gets its flush,
                    # which is the one that ends the backward pass.  Its gradient (one LayerNorm backward's dx store) is computed for nothing.
                    x = x.detach().requires_grad_()
                continue
            x, bi = self._run_stage(si, x, sd_noise, bi, red, b0 if si == 0 else None)
            if si + 1 < len(self.stages) and torch.is_grad_enabled() and x.requires_grad:
                x, skip = _Fork2Fn.apply(x)     # consumed by the next stage and by a decoder / neck
                feats.append(skip)
            else:
                feats.append(x)
        return feats

    def forward_decoder(self, feats: List[Tensor], tail=None) -> Tensor:
        self._packer.join()   # decoder weight layouts are packed on the side stream while the encoder runs
        arena = ops.AccArena.get(feats[3].device)
        if arena is not None:
            arena.begin()     # one clearing launch for every InstanceNorm accumulator of this forward + backward (ops.AccArena)
        f3 = feats[3]
        if self._reducer is not None:
            f3 = self._reducer.trigger(f3, self._reducer.seg_decoder())  # decoder4 is the last decoder op in backward order
            if torch.is_grad_enabled() and f3.requires_grad:
                # backward order: decoder4, THIS flush (the decoder's queued small-level weight gradients are issued and joined), then the
                # trigger that starts the decoder segment's all-reduce
                self._wq.sync_after_flush = True
                f3 = _StageFlushFn.apply(f3, self._wq)
        d = self.decoder4(f3, feats[2])
        d = self.decoder3(d, feats[1])
        d = self.decoder2(d, feats[0])
        return self.decoder1(d, tail=tail)

    fuse_tail = True   # loss backward fused with the last decoder level's InstanceNorm backward (False: separate kernels)
    fuse_tail_sums = __import__("os").environ.get("NMH_TAIL_SUMS", "1") != "0"   # the tail backward's reductions taken in the tail forward pass

    def _decode_and_loss(self, feats, xb, ext, mask_dev, pred):
        if self.fuse_tail:
            return self.forward_decoder(feats, tail=LossTail(self, xb, ext, mask_dev, pred, zero_padded=True))   # (xb: zero outside ext -- transform / the batcher padded it)
        d0 = self.forward_decoder(feats)
        return _LossFn.apply(d0.reshape(-1, d0.shape[-1]), self, xb, ext, mask_dev, pred)

    def forward(self, x: List[Tensor], is_eval: bool = False, block_mask: Optional[Tensor] = None, sd_noise=None, return_pred: bool = False):
        self.refuse_frozen_stages("SwinTransformer_MAE3D_New.forward")
        device = self.mask_token.device
        self._ensure_ready(device)
        xb, ext = self.transform(x, device)
        B, R = xb.shape[0], self.resolution
        g = R // 4
        if block_mask is None:
            block_mask = draw_block_mask((g, g, g), self.masking_prob)
        mask_dev = block_mask.to(torch.uint8).contiguous().view(-1).to(device, non_blocking=True)
        # the mask was drawn on the host: the compact patch embed gets exactly the rows it needs (64-row granules)
        tok, b0 = self._embed(xb, mask_dev, bound_of_mask(g, block_mask.cpu().numpy()))
        feats = self.forward_encoder(tok, sd_noise, b0)
        want_pred = is_eval or return_pred
        pred = torch.empty((B, 4, R, R, R), device=device) if want_pred else None
        losses = self._decode_and_loss(feats, xb, ext, mask_dev, pred)
        loss, loss_rgb, loss_alpha = losses[0], losses[1], losses[2]
        if return_pred:
            return loss, loss_rgb, loss_alpha, pred
        if is_eval:
            patch = lambda t: t.reshape(B, 4, g, 4, g, 4, g, 4).permute(0, 2, 4, 6, 3, 5, 7, 1).reshape(B, g, g, g, 64, 4)  # noqa: E731
            tgt = patch(xb)
            return loss, loss_rgb, loss_alpha, patch(pred), tgt[..., 3:] > 0.01, tgt
        return loss, loss_rgb, loss_alpha

    def forward_static(self, xb: Tensor, ext: Tensor, mask_dev: Tensor, bound: Optional[EmbedBound] = None):
        """graph-capturable training forward: everything already on the device (padded batch (B,4,R,R,R) fp32, extents [B,3]
        int32, token mask [g^3] uint8); no host<->device traffic, no python RNG.  bound: what the caller, who draws the masks, promises about them.
        PRECONDITION: xb is ZERO outside each sample's extents, as `transform` and the batcher's slots make it -- the tail then walks each sample's valid box
        alone (UpPlan.tail_box, ops.TAIL_BOX); on a batch padded with anything else, set ops.TAIL_BOX = False."""
        B, R = xb.shape[0], self.resolution
        g = R // 4
        self._packer.run()
        tok, b0 = self._embed(xb, mask_dev, bound)
        losses = self._decode_and_loss(self.forward_encoder(tok, b0=b0), xb, ext, mask_dev, None)
        return losses[0], losses[1], losses[2]

    def encoder_features(self, xb: Tensor) -> List[Tensor]:
        """nerf_rpn contract (feature_extractor.py:1176-1187): NCDHW feature list [C,2C,4C,8C]."""
        t = self.patch_partition(xb)
        t = t + self.pos_embed.to(t.dtype)
        feats = []
        for st in self.stages:
            t = st(t)
            feats.append(t.permute(0, 4, 1, 2, 3).contiguous())
        return feats


SwinTransformer_MAE3D = SwinTransformer_MAE3D_New  # the alias run_swin_mae3d.py:22 imports

SWIN_CONFIGS = {
    "swin_t": dict(embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24]),
    "swin_s": dict(embed_dim=96, depths=[2, 2, 18, 2], num_heads=[3, 6, 12, 24]),
    "swin_b": dict(embed_dim=128, depths=[2, 2, 18, 2], num_heads=[4, 8, 16, 32]),  # defined deviation, SURVEY 8(c)
    "swin_l": dict(embed_dim=192, depths=[2, 2, 18, 2], num_heads=[6, 12, 24, 48]),
}


def build_model(backbone_type: str = "swin_s", resolution: int = 160, masking_prob: float = 0.75, stochastic_depth_prob: float = 0.1,
                compute_dtype: torch.dtype = torch.bfloat16) -> SwinTransformer_MAE3D_New:
    """The config dict of run_swin_mae3d.py:378-411."""
    cfg = SWIN_CONFIGS[backbone_type]
    return SwinTransformer_MAE3D_New(patch_size=[4, 4, 4], embed_dim=cfg["embed_dim"], depths=cfg["depths"], num_heads=cfg["num_heads"],
                                     window_size=[4, 4, 4], stochastic_depth_prob=stochastic_depth_prob, expand_dim=True,
                                     resolution=resolution, masking_prob=masking_prob, compute_dtype=compute_dtype)
