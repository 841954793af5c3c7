"""Thin tensor-level wrappers over the C ABI (include/nerfmae_hip.h).  PyTorch is used only for device
memory and the current HIP stream; all arithmetic happens in libnerfmae_hip.so.  Every function raises if
the library is missing or a tensor is not a contiguous CUDA(HIP) tensor -- there is no CPU fallback."""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from ._lib import lib

F32, BF16 = 0, 1
WS = 4
PROFILE = None  # set to a dict by bench.py: {(op, dims...): [(start_event, end_event), ...]} recorded on the launch stream
PROFILE_BYTES = {}  # key -> algorithmic HBM bytes per launch (the HBM-bound elementwise passes; bench.py's roofline.hbm_kernels)


def _prof(key, nbytes=None):
    if PROFILE is None:
        return None
    if nbytes is not None:
        PROFILE_BYTES[key] = nbytes
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    PROFILE.setdefault(key, []).append((a, b))
    a.record(torch.cuda.current_stream())
    return b


class side_stream:
    """`with ops.side_stream():` forks a side HIP stream from the current one (also under graph capture) for kernels that are off
    the critical path (weight/bias gradients); `ops.join_side()` makes the current stream wait for it.  The fork/join pair keeps
    allocator lifetimes trivial: every tensor touched on the side stream outlives the join."""
    _streams = {}
    enabled = __import__("os").environ.get("NMH_NO_SIDE", "0") != "1"

    def __init__(self, enable: bool = True):
        self.enable = enable

    @staticmethod
    def auto(grids_per_step: int):
        """Round 1-2: forked kernels cost extra dependency packets at launch, and with 1-2 grids per step the fork/join pairs only added to a
        launch-bound step (23.4 ms with, 19.4 ms without), so the side stream was used from 3 grids on.  Round 3: most of those joins were the
        per-block ones that also serialised the two queues (model._BlockFn.backward); without them the fork pays at every batch size (1 grid
        11.59 -> 11.46 ms, 2 grids 17.63 -> 17.55, 8 grids 51.4 -> 50.5).  NMH_NO_SIDE=1 / NMH_SIDE=1 override; NMH_SIDE_MIN_GRIDS sets the threshold."""
        env = __import__("os").environ
        if env.get("NMH_NO_SIDE", "0") == "1":
            side_stream.enabled = False
        elif env.get("NMH_SIDE", "0") == "1":
            side_stream.enabled = True
        else:
            side_stream.enabled = grids_per_step >= int(env.get("NMH_SIDE_MIN_GRIDS", "1"))

    def __enter__(self):
        if not (side_stream.enabled and self.enable):
            self.ctx = None
            return self
        dev = torch.cuda.current_device()
        if dev not in side_stream._streams:
            side_stream._streams[dev] = torch.cuda.Stream(device=dev)
        self.s = side_stream._streams[dev]
        self.s.wait_stream(torch.cuda.current_stream())
        self.ctx = torch.cuda.stream(self.s)
        self.ctx.__enter__()
        return self

    def __exit__(self, *a):
        if self.ctx is not None:
            self.ctx.__exit__(*a)
        return False


def join_side():
    if side_stream.enabled:
        s = side_stream._streams.get(torch.cuda.current_device())
        if s is not None:
            torch.cuda.current_stream().wait_stream(s)


def dt_of(t: torch.Tensor) -> int:
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise TypeError(f"unsupported dtype {t.dtype}")


def _st() -> int:
    return torch.cuda.current_stream().cuda_stream


def _chk(*ts):
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError("nerf_mae_amd ops need HIP device tensors (no CPU fallback)")
        if not t.is_contiguous():
            raise RuntimeError("nerf_mae_amd ops need contiguous tensors")


class WinGeom:
    """Token grid (B,H,W,D), padded dims and effective shifts for 4x4x4 shifted windows (swin_mae3d.py:62-81)."""

    def __init__(self, B: int, H: int, W: int, D: int, shift: Sequence[int]):
        self.B, self.H, self.W, self.D = B, H, W, D
        self.P = [(s + WS - 1) // WS * WS for s in (H, W, D)]
        self.shift = [0 if WS >= self.P[a] else int(shift[a]) for a in range(3)]
        self.rows = B * self.P[0] * self.P[1] * self.P[2]  # window-ordered rows (incl. pads)
        self.tokens = B * H * W * D
        self.carr = (ctypes.c_int * 10)(B, H, W, D, self.P[0], self.P[1], self.P[2], *self.shift)


def gemm_nt(A, W, bias=None, act=0, C2=None, resid=None, rowscale=None, rows_per_scale=1, out=None, accumulate=False,
            M=None, N=None, K=None):
    """out[M,N] = epi(A[M,K] @ W[N,K]^T)."""
    M = A.shape[0] if M is None else M
    K = A.shape[-1] if K is None else K
    N = W.shape[0] if N is None else N
    ldc = N if out is None else out.stride(0)
    for name, t in (("C2", C2), ("resid", resid)):   # the epilogue indexes both with the output's row stride
        ld = None if t is None else (t.stride(-2) if t.dim() > 1 else N)
        if ld is not None and ld != ldc:
            raise ValueError(f"gemm_nt: {name} has row stride {ld}, out has {ldc}: they must agree")
    _chk(A, W, bias, C2, resid, rowscale, out)
    if out is None:
        out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    lib().call("nmh_gemm_nt", dt_of(A), A, A.stride(0) if A.dim() > 1 else K, W, W.stride(0), M, N, K, out, ldc, bias, act, C2,
               resid, rowscale, rows_per_scale, int(accumulate), _st())
    return out


NT_FAMILIES = ("reg", "dma", "k128", "w22")   # include/nerfmae_hip.h: nmh_gemm_nt_plan


def gemm_nt_plan(dtype, M, N, K, lda=None, ldw=None, win_on=False, up_k=0, ksplit=1, batch=1):
    """The kernel gemm_nt would launch for these arguments, as (family, MT, NT, ring stages, contraction splits, narrow); asked of the
    library's own dispatch (a host query: no launch, no device)."""
    plan = (ctypes.c_int * 6)()
    lib().call("nmh_gemm_nt_plan", BF16 if dtype == torch.bfloat16 else F32, K if lda is None else lda, K if ldw is None else ldw, M, N, K,
               int(win_on), up_k, ksplit, batch, plan)
    return (NT_FAMILIES[plan[0]],) + tuple(plan[1:6])


def gemm_nt_plan_table():
    """Every (dtype, family, MT, NT, ring stages) the gemm_nt launcher holds for plain row-major operands."""
    cnt = (ctypes.c_int * 1)()
    lib().call("nmh_gemm_nt_plan_table", None, 0, cnt)
    n = cnt[0]
    rows = (ctypes.c_int * (5 * n))()
    lib().call("nmh_gemm_nt_plan_table", rows, n, cnt)
    return [(torch.bfloat16 if rows[5 * i] == BF16 else torch.float32, NT_FAMILIES[rows[5 * i + 1]]) + tuple(rows[5 * i + 2:5 * i + 5]) for i in range(n)]


def gemm_tn_plan(dtype, M, N, K, lda=None, rowscale=False, rows_per_scale=1, ws_floats=None):
    """The kernel gemm_tn would launch, as (NTW, KTW, ring stages, rows per split, splits, partials): tile (32 NTW) x (32 KTW); partials 1 =
    workspace partial sums + a reduce launch, 0 = the splits add into dW (fp32 atomics when there are several).  ws_floats defaults to
    the workspace gemm_tn passes."""
    plan = (ctypes.c_int * 6)()
    lib().call("nmh_gemm_tn_plan", BF16 if dtype == torch.bfloat16 else F32, N if lda is None else lda, M, N, K, int(bool(rowscale)), rows_per_scale,
               max(TN_WS_FLOATS, 0) if ws_floats is None else ws_floats, plan)
    return tuple(plan)


_TN_WS = {}
TN_WS_FLOATS = int(__import__("os").environ.get("NMH_TN_WS_MB", "48")) * (1 << 18)   # 0 disables (fp32 atomics instead)


def _tn_workspace(device):
    """scratch for split-contraction partials, one per (device, stream): weight-gradient GEMMs of the main and the side stream overlap"""
    if TN_WS_FLOATS <= 0:
        return None
    key = (device.index, torch.cuda.current_stream().cuda_stream)
    ws = _TN_WS.get(key)
    if ws is None:
        ws = _TN_WS[key] = torch.empty(TN_WS_FLOATS, dtype=torch.float32, device=device)
    return ws


def gemm_tn(A, B, dW, rowscale=None, rows_per_scale=1, omode=0, ldo=None, p0=0, p1=0, N=None, K=None, M=None, dbias=None):
    """dW[N,K] += A[M,N]^T @ B[M,K] (fp32 atomics into dW); dbias[N] += column sums of A (optional, same pass)."""
    _chk(A, B, dW, rowscale, dbias)
    M = A.shape[0] if M is None else M
    N = A.shape[1] if N is None else N
    K = B.shape[1] if K is None else K
    ws = _tn_workspace(A.device)
    lib().call("nmh_gemm_tn", dt_of(A), A, A.stride(0), B, B.stride(0), dW, M, N, K, rowscale, rows_per_scale, omode,
               K if ldo is None else ldo, p0, p1, dbias, ws, 0 if ws is None else ws.numel(), _st())
    return dW


class _TnProblem(ctypes.Structure):   # include/nerfmae_hip.h: nmh_tn_problem
    _fields_ = [("A", ctypes.c_void_p), ("lda", ctypes.c_int64), ("B", ctypes.c_void_p), ("ldb", ctypes.c_int64), ("dW", ctypes.c_void_p),
                ("ldo", ctypes.c_int64), ("dbias", ctypes.c_void_p), ("rowscale", ctypes.c_void_p), ("M", ctypes.c_int64), ("N", ctypes.c_int),
                ("K", ctypes.c_int), ("rows_per_sample", ctypes.c_int), ("stride_k", ctypes.c_int64), ("up_k", ctypes.c_int), ("up_v", ctypes.c_int),
                ("bias_atomic", ctypes.c_int), ("n_inner", ctypes.c_int), ("stride_n2", ctypes.c_int64)]


GROUPED_WGRAD = __import__("os").environ.get("NMH_TNG", "1") != "0"
DEFER_DECODER_WGRAD = __import__("os").environ.get("NMH_DEFER_DEC", "1") == "1"
# A stage's flush forks off behind the FIRST input-gradient kernel of the next stage instead of in front of it (round 5).  In the captured graph both are
# successors of the stage's last kernel; the HIP graph executor keeps the successor captured first on the predecessor's queue and gives the other one a new
# queue plus a cross-queue wait -- and that wait was released only ~10 side kernels later (1 grid: 0.58 ms with the input-gradient queue idle at the
# stage 3 -> 2 boundary, profiles/r5k_timeline_1grids.txt 6.86 -> 7.43 ms).  Captured first, the chain stays on its queue and the side launches take the wait.
WQ_FLUSH_AFTER_FIRST = __import__("os").environ.get("NMH_WQ_FLUSH_AFTER_FIRST", "1") == "1"


class _LnReduceItem(ctypes.Structure):   # include/nerfmae_hip.h: nmh_ln_reduce_item
    _fields_ = [("partials", ctypes.c_void_p), ("dgamma", ctypes.c_void_p), ("dbeta", ctypes.c_void_p), ("partial_rows", ctypes.c_int64), ("C", ctypes.c_int),
                ("reserved", ctypes.c_int)]


def ln_param_grad_reduce(items):
    """items: [(partials, partial_rows, C, dgamma, dbeta)] -> one launch (nmh_layernorm_param_grad_reduce).  The items of a launch run as independent
    workgroups that ADD into dgamma / dbeta with plain read-modify-writes: the same parameter twice in one flush (two forward passes before one
    backward) is split over consecutive launches, like WgradQueue.flush does for a repeated dW"""
    group, seen = [], set()

    def launch(g):
        if not g:
            return
        arr = (_LnReduceItem * len(g))()
        for i, (part, nb, C, dg, db) in enumerate(g):
            _chk(part, dg, db)
            arr[i] = _LnReduceItem(part.data_ptr(), dg.data_ptr(), db.data_ptr(), nb, C, 0)
        lib().call("nmh_layernorm_param_grad_reduce", arr, len(g), _st())

    for it in items:
        if it[3].data_ptr() in seen:
            launch(group)
            group, seen = [], set()
        group.append(it)
        seen.add(it[3].data_ptr())
    launch(group)


class WgradQueue:
    """Deferred weight gradients of the encoder (bf16): `add` records one dW[N,K] += A[M,N]^T . B[M,K] problem (and keeps its operands
    alive), `flush` issues everything recorded so far through nmh_gemm_tn_grouped -- on the forked side stream when that is enabled, so
    the launch overlaps the input-gradient chain of the next stage -- and `join` makes the current stream wait for it and releases the
    operands.  The input-gradient chain of a stage thus runs without any weight-gradient launch in between."""

    def __init__(self):
        self.pending, self.inflight, self._cb, self.sync_after_flush = [], [], False, False
        self.ln_items = []   # LayerNorm parameter-gradient partials of the current flush group (add_ln_partials)
        self.pad_items = {}  # pad-row column sums of the current flush group, by (geometry, width, dtype) (add_pad_colsum)
        self.deferred = []   # closures (other weight-gradient launches) to issue with the next flush, inside the same fork
        self._due = False    # a flush requested by a stage boundary, issued by the next block behind its first kernel (WQ_FLUSH_AFTER_FIRST)

    def reset(self):
        """start of a forward pass: nothing may be queued here -- unless a previous backward pass raised half-way, in which case its
        operands (whole 160^3 gradients) would stay referenced for good and `_cb` would never re-arm the end-of-backward callback"""
        if self.pending or self.deferred or self.inflight or self._cb:
            join_side()
            self.pending, self.deferred, self.inflight, self._cb, self._due = [], [], [], False, False
            self.ln_items, self.pad_items = [], {}

    def defer(self, fn):
        """queue an arbitrary weight-gradient launch (a closure that keeps its operands alive) for the next flush: the decoder's small-level
        weight gradients then share ONE fork / join with the grouped launch of the first encoder stage instead of a fork each"""
        self.deferred.append(fn)
        if not self._cb:
            self._cb = True
            torch.autograd.Variable._execution_engine.queue_callback(self._final)

    def add_ln_partials(self, part, nb, C, dgamma, dbeta):
        """the dgamma / dbeta partial sums of a LayerNorm backward (ops.layernorm_bwd(wq=...)): all of a flush are reduced by ONE launch"""
        if not self.ln_items:
            items = self.ln_items = []
            self.defer(lambda: ln_param_grad_reduce(items))   # (the list object: filled until the flush runs the closure)
        self.ln_items.append((part, nb, C, dgamma, dbeta))

    def add_pad_colsum(self, x, out, geom):
        """the pad rows' share of a qkv bias gradient (ops.window_pad_rows_colsum): all of a flush with the same geometry go out as ONE launch"""
        key = (tuple(geom.carr), x.shape[1], x.dtype)
        groups = self.pad_items
        if key not in groups:
            lst = groups[key] = []
            self.defer(lambda: window_pad_rows_colsum_grouped(lst, geom))   # (the list object: filled until the flush runs the closure)
        groups[key].append((x, out))

    def add(self, A, B, dW, dbias=None, rowscale=None, rows_per_sample=None):
        _chk(A, B, dW, dbias, rowscale)
        if A.dtype != torch.bfloat16 or B.dtype != torch.bfloat16:
            raise RuntimeError("WgradQueue: the grouped weight-gradient kernel takes bf16 operands")
        self.pending.append((A, B, dW, dbias, rowscale, A.shape[0] if rows_per_sample is None else rows_per_sample))
        if not self._cb:   # safety net: whatever is still queued when the backward pass ends is issued and joined there
            self._cb = True
            torch.autograd.Variable._execution_engine.queue_callback(self._final)

    def request_flush(self):
        self._due = True
        if not self._cb:
            self._cb = True
            torch.autograd.Variable._execution_engine.queue_callback(self._final)

    def flush_due(self):
        if self._due:
            self._due = False
            self.flush()

    def _final(self):
        self._cb = False
        self._due = False
        self.flush()
        self.join()

    def _launch(self, group, foreground=False):
        arr = (_TnProblem * len(group))()
        for i, (A, B, dW, dbias, rs, rps) in enumerate(group):
            arr[i] = _TnProblem(A.data_ptr(), A.stride(0), B.data_ptr(), B.stride(0), dW.data_ptr(), B.shape[1],
                                0 if dbias is None else dbias.data_ptr(), 0 if rs is None else rs.data_ptr(), A.shape[0], A.shape[1], B.shape[1], rps)
        ws = _tn_workspace(group[0][0].device)
        lib().call("nmh_gemm_tn_grouped_fg" if foreground else "nmh_gemm_tn_grouped", BF16, arr, len(group), ws,
                   0 if ws is None else ws.numel(), _st())

    def flush(self, foreground=False):
        """foreground: the group will run (almost) alone -- the last flushes of a backward pass -- and may split for the whole chip"""
        if not self.pending and not self.deferred:
            return
        todo, self.pending = self.pending, []
        fns, self.deferred = self.deferred, []
        self.ln_items, self.pad_items = [], {}   # (the queued closures hold the lists they work on)
        with side_stream():
            for fn in fns:
                fn()
            if not todo:
                self.inflight.extend(fns)
                return
            group, seen = [], set()
            for pr in todo:
                if pr[2].data_ptr() in seen:   # the same parameter twice (two forward passes before one backward): separate launches
                    self._launch(group, foreground)
                    group, seen = [], set()
                group.append(pr)
                seen.add(pr[2].data_ptr())
            self._launch(group, foreground)
        self.inflight.extend(todo)   # operands stay referenced until the issuing stream has been joined
        self.inflight.extend(fns)

    def join(self):
        join_side()
        self.inflight = []


def conv3d_k3(X, Wp, Cout, out=None, accumulate=False):
    """X (B,D,H,W,Cin) channels-last, Wp packed [Cout][27][Cin] -> (B,D,H,W,Cout)."""
    _chk(X, Wp, out)
    B, D, H, W, Cin = X.shape
    if out is None:
        out = torch.empty((B, D, H, W, Cout), dtype=X.dtype, device=X.device)
    ev = _prof(("conv3d_k3", B, D, Cin, Cout))
    ws = _tn_workspace(X.device) if B * D * H * W <= 65536 else None     # split contraction on the small decoder levels
    lib().call("nmh_conv3d_k3", dt_of(X), X, Wp, out, B, D, H, W, Cin, Cout, int(accumulate), ws, 0 if ws is None else ws.numel(), _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def conv3d_k3_c48(X, Wk, out=None, accumulate=False, stats_acc=None):
    """specialised Cin=Cout=48 bf16 conv (fragment-ordered weights Wk, pack modes 6/7); stats_acc: optional fp64 [B,48,2] buffer that
    receives the per-(sample,channel) sum / sum-of-squares of the outputs (fused InstanceNorm statistics)"""
    _chk(X, Wk, out, stats_acc)
    B, D, H, W, Cin = X.shape
    if Cin != 48 or X.dtype != torch.bfloat16:
        raise RuntimeError("conv3d_k3_c48 needs bf16 activations with 48 channels")
    if out is None:
        out = torch.empty((B, D, H, W, 48), dtype=X.dtype, device=X.device)
    ev = _prof(("conv3d_k3_c48", B, D, 48, 48))
    lib().call("nmh_conv3d_k3_c48", X, Wk, out, B, D, H, W, int(accumulate), stats_acc, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


TAIL_SIGN_MASK = __import__("os").environ.get("NMH_TAIL_SIGN_MASK", "1") != "0"   # tail backward reads [d0 > 0] bits written by the tail forward instead of the residual
C48_BWD_REDUCE = __import__("os").environ.get("NMH_C48_BWD_REDUCE", "1") != "0"   # decoder1 conv2 input gradient: InstanceNorm-backward sums in the conv epilogue


def conv3d_k3_c48_bwd_reduce(dY, Wkd, y1, stats1, sums, out=None, slope=0.01):
    """dX = conv^T(dY) (48 -> 48, dgrad pack) + the InstanceNorm-backward sums of (dX, y1) in the epilogue (include/nerfmae_hip.h:
    nmh_conv3d_k3_c48_bwd_reduce); sums: fp64 [B,48,2]"""
    _chk(dY, Wkd, y1, stats1, sums, out)
    B, D, H, W, Cin = dY.shape
    if Cin != 48 or dY.dtype != torch.bfloat16 or y1.dtype != torch.bfloat16 or y1.numel() != dY.numel() or sums.dtype != torch.float64:
        raise RuntimeError("conv3d_k3_c48_bwd_reduce needs bf16 tensors with 48 channels and fp64 sums")
    if out is None:
        out = torch.empty((B, D, H, W, 48), dtype=dY.dtype, device=dY.device)
    ev = _prof(("conv3d_k3_c48_bwd_reduce", B, D, 48, 48))
    lib().call("nmh_conv3d_k3_c48_bwd_reduce", dY, Wkd, out, B, D, H, W, y1, stats1, float(slope), sums, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


# decoder1 in the centered form (csrc/cconv.hip): the mean of conv1's output is computed from the coarse tensor before the launch, conv1 stores lrelu(y1 - mean), 1 / std goes
# into conv2's weights per sample -- no normalisation pass over the 160^3 tensor, no second copy of it
CCONV_CENTERED = __import__("os").environ.get("NMH_CCONV_CENTERED", "1") != "0"
C48_IMG = 41 * 3 * 512


def conv48_pack_scaled(W, stats, out, B):
    _chk(W, stats, out)
    if tuple(W.shape) != (48, 48, 3, 3, 3) or W.dtype != torch.float32 or out.numel() < B * C48_IMG or out.dtype != torch.bfloat16:
        raise ValueError("conv48_pack_scaled: shapes")
    lib().call("nmh_conv48_pack_scaled", W, stats, out, B, _st())
    return out


def conv3d_k3_c48_per_sample(X, Wk_per_sample, out=None, stats_acc=None):
    """conv3d_k3_c48 with one weight image per sample (conv48_pack_scaled)"""
    _chk(X, Wk_per_sample, out, stats_acc)
    B, D, H, W, Cin = X.shape
    if Cin != 48 or X.dtype != torch.bfloat16 or Wk_per_sample.numel() < B * C48_IMG:
        raise RuntimeError("conv3d_k3_c48_per_sample needs bf16 activations with 48 channels and B weight images")
    if out is None:
        out = torch.empty((B, D, H, W, 48), dtype=X.dtype, device=X.device)
    ev = _prof(("conv3d_k3_c48", B, D, 48, 48))
    lib().call("nmh_conv3d_k3_c48_per_sample", X, Wk_per_sample, out, B, D, H, W, stats_acc, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def conv3d_k3_c48_bwd_reduce_centered(dY, Wkd, z, stats1, sums, out=None, slope=0.01):
    """conv3d_k3_c48_bwd_reduce reading z = lrelu(y1 - mean) for y1"""
    _chk(dY, Wkd, z, stats1, sums, out)
    B, D, H, W, Cin = dY.shape
    if Cin != 48 or dY.dtype != torch.bfloat16 or z.dtype != torch.bfloat16 or z.numel() != dY.numel() or sums.dtype != torch.float64:
        raise RuntimeError("conv3d_k3_c48_bwd_reduce_centered needs bf16 tensors with 48 channels and fp64 sums")
    if out is None:
        out = torch.empty((B, D, H, W, 48), dtype=dY.dtype, device=dY.device)
    ev = _prof(("conv3d_k3_c48_bwd_reduce", B, D, 48, 48))
    lib().call("nmh_conv3d_k3_c48_bwd_reduce_centered", dY, Wkd, out, B, D, H, W, z, stats1, float(slope), sums, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


CCONV = __import__("os").environ.get("NMH_CCONV", "1") != "0"   # decoder1 forward: ConvTranspose(k = s = 4) composed with conv1 (csrc/cconv.hip)


def cconv_pack(Wt, W1, bt, Wcp, delta, ws=None):
    """composed decoder1 weights (fragment order, bf16) + [27,48] border table from transp_conv.weight [96,48,4,4,4], conv1.weight [48,48,3,3,3],
    transp_conv.bias; ws: cconv_pack_ws_floats() floats of scratch (allocated here when not given)"""
    _chk(Wt, W1, bt, Wcp, delta, ws)
    if tuple(Wt.shape) != (96, 48, 4, 4, 4) or tuple(W1.shape) != (48, 48, 3, 3, 3) or Wcp.numel() < cconv_pack_numel() or delta.numel() < 27 * 48:
        raise ValueError("cconv_pack: shapes")
    if ws is None:
        ws = torch.empty(cconv_pack_ws_floats(), dtype=torch.float32, device=Wcp.device)
    lib().call("nmh_cconv_pack", Wt, W1, bt, Wcp, delta, ws, _st())


def cconv_pack_centered(Wt, W1, bt, Wcp, delta, ws, mean_table):
    """cconv_pack + the [27,96,48] fp32 table of the composed blocks summed over the phases (include/nerfmae_hip.h: nmh_cconv_pack_centered)"""
    _chk(Wt, W1, bt, Wcp, delta, ws, mean_table)
    if mean_table.numel() < 27 * 96 * 48 or mean_table.dtype != torch.float32:
        raise ValueError("cconv_pack_centered: mean_table must hold 27 x 96 x 48 floats")
    lib().call("nmh_cconv_pack_centered", Wt, W1, bt, Wcp, delta, ws, mean_table, _st())


def cconv_output_mean(x, mean_table, delta, B, v):
    """per-(sample, channel) mean of cconv_fwd's output from the COARSE tensor (nmh_cconv_output_mean) -> fp32 [B,48]"""
    _chk(x, mean_table, delta)
    cls = torch.empty(B * (27 * 96 + 48), dtype=torch.float64, device=x.device)   # class sums + dot-product accumulators
    mean = torch.empty((B, 48), dtype=torch.float32, device=x.device)
    lib().call("nmh_cconv_output_mean", x, mean_table, delta, cls, mean, B, v, _st())
    return mean


def cconv_fwd_centered(x, Wcp, delta, mean, B, v, out=None, stats_acc=None, slope=0.01):
    """z = lrelu(cconv_fwd(x) - mean) + the statistics of cconv_fwd(x) - mean (nmh_cconv_fwd_centered)"""
    _chk(x, Wcp, delta, mean, out, stats_acc)
    if x.dtype != torch.bfloat16 or x.shape[-1] != 96 or v % 8:
        raise RuntimeError("cconv_fwd_centered needs bf16 activations with 96 channels on a coarse grid whose edge is a multiple of 8")
    if out is None:
        out = torch.empty((B, 4 * v, 4 * v, 4 * v, 48), dtype=x.dtype, device=x.device)
    ev = _prof(("cconv_fwd", B, 4 * v, 96, 48))
    lib().call("nmh_cconv_fwd_centered", x, Wcp, delta, mean, float(slope), out, B, v, stats_acc, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def cconv_pack_ws_floats() -> int:
    return int(lib().call("nmh_cconv_pack_ws_floats"))


def cconv_pack_numel() -> int:
    return int(lib().call("nmh_cconv_pack_numel"))


def cconv_fwd(x, Wcp, delta, B, v, out=None, stats_acc=None):
    """y1 [B,(4v)^3,48] = conv3x3x3(ConvTranspose_{k=s=4}(x [B,v^3,96])) minus the interior bias constant (see include/nerfmae_hip.h)"""
    _chk(x, Wcp, delta, out, stats_acc)
    if x.dtype != torch.bfloat16 or x.shape[-1] != 96 or v % 8:
        raise RuntimeError("cconv_fwd needs bf16 activations with 96 channels on a coarse grid whose edge is a multiple of 8")
    if out is None:
        out = torch.empty((B, 4 * v, 4 * v, 4 * v, 48), dtype=x.dtype, device=x.device)
    ev = _prof(("cconv_fwd", B, 4 * v, 96, 48))
    lib().call("nmh_cconv_fwd", x, Wcp, delta, out, B, v, stats_acc, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def cconv_dgrad_pack_numel() -> int:
    return int(lib().call("nmh_cconv_dgrad_pack_numel"))


def cconv_dgrad_pack(Wcp, Wdp):
    """the composed weights in the input-gradient kernel's fragment order, gathered from the forward's (include/nerfmae_hip.h: nmh_cconv_dgrad_pack)"""
    _chk(Wcp, Wdp)
    if Wdp.numel() < cconv_dgrad_pack_numel() or Wdp.dtype != torch.bfloat16 or Wcp.numel() < cconv_pack_numel():
        raise ValueError("cconv_dgrad_pack: shapes")
    lib().call("nmh_cconv_dgrad_pack", Wcp, Wdp, _st())


def cconv_dgrad(dy1, Wdp, B, v, add=None, out=None):
    """dx [B,v^3,96] = (add or 0) + ConvT^T(conv1^T(dy1 [B,(4v)^3,48])) (include/nerfmae_hip.h: nmh_cconv_dgrad); add may be out"""
    _chk(dy1, Wdp, add, out)
    if dy1.dtype != torch.bfloat16 or v % 8 or dy1.numel() != B * (4 * v) ** 3 * 48:
        raise RuntimeError("cconv_dgrad needs a bf16 gradient with 48 channels on a fine grid whose edge is a multiple of 32")
    if out is None:
        out = torch.empty((B * v ** 3, 96), dtype=dy1.dtype, device=dy1.device)
    if out.numel() != B * v ** 3 * 96 or (add is not None and (add.numel() != out.numel() or add.dtype != out.dtype)):
        raise ValueError("cconv_dgrad: shapes")
    ev = _prof(("cconv_dgrad", B, 4 * v, 48, 96))
    lib().call("nmh_cconv_dgrad", dy1, Wdp, add, out, B, v, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def upconv4_pack_numel() -> int:
    return int(lib().call("nmh_upconv4_pack_numel"))


def upconv4_pack(pack_ws, Wup):
    """fragment-ordered bf16 weights of the k = s = 4 transpose conv from the scratch cconv_pack filled in this step"""
    _chk(pack_ws, Wup)
    if Wup.numel() < upconv4_pack_numel() or Wup.dtype != torch.bfloat16:
        raise ValueError("upconv4_pack: shapes")
    lib().call("nmh_upconv4_pack", pack_ws, Wup, _st())


def upconv4_fwd(x, Wup, bt, out, B, v):
    """u [B,(4v)^3,48] = ConvTranspose3d_{k=s=4}(x [B,v^3,96]) + bt (include/nerfmae_hip.h: nmh_upconv4_fwd)"""
    _chk(x, Wup, bt, out)
    if x.dtype != torch.bfloat16 or out.dtype != torch.bfloat16 or x.shape[-1] != 96 or v % 8 or out.numel() != B * (4 * v) ** 3 * 48:
        raise RuntimeError("upconv4_fwd needs bf16 activations with 96 channels on a coarse grid whose edge is a multiple of 8")
    ev = _prof(("upconv4_fwd", B, 4 * v, 96, 48))
    lib().call("nmh_upconv4_fwd", x, Wup, bt, out, B, v, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


CCONV_WGRAD = __import__("os").environ.get("NMH_CCONV_WGRAD", "1") != "0"   # conv1's weight gradient through the composition (with NMH_CCONV)
_CCW_WS = {}


def cconv_wgrad(x, dy1, pack_ws, bt, dW1, B, v, dWt=None, dbt=None, phase=0):
    """conv1.weight gradient [48,48,3,3,3] += through the composed ConvTranspose o conv (include/nerfmae_hip.h: nmh_cconv_wgrad); dy1 must be the
    input gradient of the affine-free InstanceNorm behind conv1 (zero per-sample sums).  dWt [96,48,4,4,4] / dbt [48] (fp32, optional): += the
    transpose conv's own parameter gradients through conv1 (used with cconv_dgrad, when conv1's input gradient on the fine grid is not formed)"""
    _chk(x, dy1, pack_ws, bt, dW1, dWt, dbt)
    if (dWt is None) != (dbt is None) or (dWt is not None and (dWt.numel() != 96 * 48 * 64 or dbt.numel() != 48)):
        raise ValueError("cconv_wgrad: dWt / dbt")
    if x.dtype != torch.bfloat16 or dy1.dtype != torch.bfloat16 or v % 8 or v > 40:
        raise RuntimeError("cconv_wgrad needs bf16 operands on a coarse grid whose edge is a multiple of 8 (<= 40)")
    key = x.device.index          # (one workspace per device: phase 2 may run on a side stream behind phase 1)
    if key not in _CCW_WS:
        _CCW_WS[key] = torch.empty(int(lib().call("nmh_cconv_wgrad_ws_floats")), dtype=torch.float32, device=x.device)
    ev = _prof(("cconv_wgrad", B, 4 * v, 96, 48))
    lib().call("nmh_cconv_wgrad", x, dy1, pack_ws, bt, dW1, dWt, dbt, _CCW_WS[key], B, v, int(phase), _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return dW1


C48MB_MIN_VOXELS = int(__import__("os").environ.get("NMH_C48MB_MIN_VOXELS", "32768"))   # 0 disables the 48-channel-block multi-block kernel


def conv3d_k3_c48mb(X, Wk, Cout, out=None, accumulate=False):
    """3x3x3 conv on 48-channel blocks (bf16, Cin and Cout multiples of 48; one fragment-ordered image per (output block, input block), pack
    modes 6/7 on the [Cout][Cin][27] weight): the decoder1 LDS-halo kernel with (tile, output block, input block) work items"""
    _chk(X, Wk, out)
    B, D, H, W, Cin = X.shape
    if Cin % 48 or Cout % 48 or X.dtype != torch.bfloat16:
        raise RuntimeError("conv3d_k3_c48mb needs bf16 activations with channel counts that are multiples of 48")
    if out is None:
        out = torch.empty((B, D, H, W, Cout), dtype=X.dtype, device=X.device)
    ev = _prof(("conv3d_k3_halo", B, D, Cin, Cout))
    lib().call("nmh_conv3d_k3_c48mb", X, Wk, out, B, D, H, W, Cin, Cout, int(accumulate), _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def conv3d_k3_c64(X, Wk, Cout, out=None, accumulate=False, stats_acc=None, bias=None):
    """3x3x3 conv on 64-channel blocks (bf16, Cin and Cout multiples of 64; fragment-ordered weights Wk, pack modes 8/9); stats_acc:
    optional fp64 [B,Cout,2] buffer receiving the fused InstanceNorm statistics"""
    _chk(X, Wk, out, stats_acc, bias)
    B, D, H, W, Cin = X.shape
    if Cin % 64 or Cout % 64 or X.dtype != torch.bfloat16:
        raise RuntimeError("conv3d_k3_c64 needs bf16 activations with channel counts that are multiples of 64")
    if out is None:
        out = torch.empty((B, D, H, W, Cout), dtype=X.dtype, device=X.device)
    ev = _prof(("conv3d_k3_halo", B, D, Cin, Cout))
    lib().call("nmh_conv3d_k3_c64", X, Wk, out, B, D, H, W, Cin, Cout, int(accumulate), stats_acc, bias, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


C64_MIN_VOXELS = int(__import__("os").environ.get("NMH_C64_MIN_VOXELS", "32768"))   # 0 disables the 64-channel-block kernels


def use_conv64(X, Cout):
    """dispatch rule of the 64-channel-block LDS-halo conv: bf16, both channel counts multiples of 64 and a volume whose 4x4x16 tiles are
    mostly full (measured: 0.43 vs 0.24 of peak at 160^3 64->64, 0.37 vs 0.29 at 40^3 256->256, break-even at 20^3)"""
    B, D, H, W, Cin = X.shape
    return (C64_MIN_VOXELS > 0 and X.dtype == torch.bfloat16 and Cin % 64 == 0 and Cout % 64 == 0 and D * H * W >= C64_MIN_VOXELS
            and D * H * W * Cin * 2 < 2 ** 32)


def conv64_pack_numel(Cin, Cout):
    return (Cin // 64) * (Cout // 64) * 54 * 4 * 64 * 8


_C48_WS = {}


def conv3d_k3_c48_wgrad(dY, X, dW):
    """dW[48][48][3][3][3] += weight gradient (specialised LDS-halo kernel + per-workgroup partial reduce)"""
    _chk(dY, X, dW)
    B, D, H, W, Cin = X.shape
    key = X.device.index
    if key not in _C48_WS:
        _C48_WS[key] = torch.empty(lib().call("nmh_conv3d_k3_c48_wgrad_ws_floats"), dtype=torch.float32, device=X.device)
    ev = _prof(("conv3d_k3_c48_wgrad", B, D, 48, 48))
    lib().call("nmh_conv3d_k3_c48_wgrad", dY, X, dW, _C48_WS[key], B, D, H, W, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return dW


def conv3d_k3_c48_wgrad_scaled(dY, Z, stats, dW):
    """conv3d_k3_c48_wgrad on (dY, Z) with every workgroup's partial scaled by rstd[sample][ci] (stats [B,48,2]) in the reduce: the weight gradient of a conv whose
    input is rstd * Z (include/nerfmae_hip.h: nmh_conv3d_k3_c48_wgrad_scaled; B in {1, 2, 4, 8})"""
    _chk(dY, Z, stats, dW)
    B, D, H, W, Cin = Z.shape
    key = Z.device.index
    if key not in _C48_WS:
        _C48_WS[key] = torch.empty(lib().call("nmh_conv3d_k3_c48_wgrad_ws_floats"), dtype=torch.float32, device=Z.device)
    ev = _prof(("conv3d_k3_c48_wgrad", B, D, 48, 48))
    lib().call("nmh_conv3d_k3_c48_wgrad_scaled", dY, Z, stats, dW, _C48_WS[key], B, D, H, W, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return dW


_HALO_WS = {}
HALO_WGRAD = __import__("os").environ.get("NMH_HALO_WGRAD", "1") != "0"


def conv3d_k3_wgrad(dY, X, dW):
    """dW[Cout][Cin][3][3][3] += weight gradient.  bf16 with Cin, Cout multiples of 48: LDS-halo kernel on 48x48 channel blocks
    (own workspace: these launches run on the side stream); otherwise the implicit-GEMM kernel."""
    _chk(dY, X, dW)
    B, D, H, W, Cin = X.shape
    Cout = dY.shape[-1]
    ev = _prof(("conv3d_k3_wgrad", B, D, Cin, Cout))
    # (measured at 4 grids: 40^3 192->96 842 -> 354 us, 20^3 384->192 515 -> 243 us; at 10^3 the 4x4x16 tiles are mostly padding
    # and the implicit GEMM wins: 229 vs 267 us)
    if (HALO_WGRAD and X.dtype == torch.bfloat16 and Cin % 48 == 0 and Cout % 48 == 0 and (Cin // 48) * (Cout // 48) <= 256
            and D * H * W >= 4096):
        key = X.device.index
        if key not in _HALO_WS:
            _HALO_WS[key] = torch.empty(lib().call("nmh_conv3d_k3_c48_wgrad_ws_floats"), dtype=torch.float32, device=X.device)
        lib().call("nmh_conv3d_k3_wgrad_halo", dY, X, dW, _HALO_WS[key], B, D, H, W, Cin, Cout, _st())
    elif (HALO_WGRAD and X.dtype == torch.bfloat16 and Cin % 64 == 0 and Cout % 64 == 0 and (Cin // 64) * (Cout // 64) <= 128
          and D * H * W >= 4096):
        key = ("c64", X.device.index)
        if key not in _HALO_WS:
            _HALO_WS[key] = torch.empty(lib().call("nmh_conv3d_k3_c64_wgrad_ws_floats"), dtype=torch.float32, device=X.device)
        lib().call("nmh_conv3d_k3_c64_wgrad", dY, X, dW, _HALO_WS[key], B, D, H, W, Cin, Cout, _st())
    else:
        lib().call("nmh_conv3d_k3_wgrad", dt_of(X), dY, X, dW, B, D, H, W, Cin, Cout, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return dW


def layernorm_fwd(x, gamma, beta, out, mean, rstd, rows, C, src_mode=0, geom: Optional[WinGeom] = None, eps=1e-5,
                  pos=None, mask=None, mask_token=None, tokens_per_sample=1):
    _chk(x, gamma, beta, out, mean, rstd, pos, mask, mask_token)
    lib().call("nmh_layernorm_fwd", dt_of(x), src_mode, x, out, gamma, beta, eps, mean, rstd, rows, C,
               geom.carr if geom is not None else None, pos, mask, mask_token, tokens_per_sample, _st())
    return out


LN_DEFER_PARAM_GRADS = __import__("os").environ.get("NMH_LN_DEFER", "1") != "0"
EMBED_KEPT = __import__("os").environ.get("NMH_EMBED_KEPT", "1") != "0"   # patch embed (im2row, GEMM, LayerNorm, weight gradient) on the kept tokens only


def embed_kept_rows(mask, cap_rows, out=None):
    """token mask [n] uint8 (1 = removed) -> int32 rowmap [n + 2] (include/nerfmae_hip.h: nmh_patch_embed_kept_rows); out: an int32 [n + 2] buffer to fill"""
    _chk(mask, out)
    n = mask.numel()
    if out is not None and (out.dtype != torch.int32 or out.numel() != n + 2):
        raise RuntimeError("embed_kept_rows: out must be int32 [n + 2]")
    rowmap = torch.empty(n + 2, dtype=torch.int32, device=mask.device) if out is None else out
    lib().call("nmh_patch_embed_kept_rows", mask, n, int(cap_rows), rowmap, _st())
    return rowmap


def patch_embed_gather_kept(x, A, B, R, rowmap, cap_rows):
    _chk(x, A, rowmap)
    ev = _prof(("patch_embed_gather", B, R))
    lib().call("nmh_patch_embed_gather_kept", dt_of(A), x, A, B, R, rowmap, int(cap_rows), _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return A


def embed_norm_fwd_kept(y0, gamma, beta, tok, mean, rstd, rows, C, pos, mask, mask_token, tokens_per_sample, rowmap, cap_rows, eps=1e-5):
    _chk(y0, gamma, beta, tok, mean, rstd, pos, mask, mask_token, rowmap)
    lib().call("nmh_patch_embed_norm_fwd_kept", dt_of(y0), y0, tok, gamma, beta, eps, mean, rstd, rows, C, pos, mask, mask_token, tokens_per_sample, rowmap, int(cap_rows), _st())
    return tok


def embed_norm_bwd_kept(dtok, y0, gamma, mean, rstd, dy0, dgamma, dbeta, rows, C, mask, dmask_token, tokens_per_sample, rowmap, cap_rows):
    _chk(dtok, y0, gamma, mean, rstd, dy0, dgamma, dbeta, mask, dmask_token, rowmap)
    lib().call("nmh_patch_embed_norm_bwd_kept", dt_of(y0), dtok, y0, gamma, mean, rstd, dy0, dgamma, dbeta, rows, C, mask, dmask_token, tokens_per_sample, rowmap, int(cap_rows), _st())
    return dy0


# stage 0's first Swin block on the kept windows plus one representative all-mask window per sample (csrc/block0.hip; model._EmbedFn / _Block0ExpandFn)
BLOCK0_KEPT = __import__("os").environ.get("NMH_BLOCK0_KEPT", "1") != "0"
BLOCK0_LN_PARTIAL_ROWS = 256   # csrc/kernels.hpp: B0_LN_BWD_BLOCKS


def block0_supported(C: int) -> bool:
    return bool(lib().call("nmh_block0_supported", C))


def block0_window_rows(mask, g, cap_windows):
    """token mask [g^3] uint8 (1 = removed, constant on every 4^3 window) -> (rowmap int32 [g^3 + 2] in window-major order, wmap int32 [nW + cap_windows])
    (include/nerfmae_hip.h: nmh_block0_window_rows)"""
    _chk(mask)
    n = g ** 3
    if mask.numel() != n or g % 4:
        raise RuntimeError("block0_window_rows: mask must hold g^3 tokens, g a multiple of 4")
    rowmap = torch.empty(n + 2, dtype=torch.int32, device=mask.device)
    wmap = torch.empty((g // 4) ** 3 + int(cap_windows), dtype=torch.int32, device=mask.device)
    lib().call("nmh_block0_window_rows", mask, g, int(cap_windows), rowmap, wmap, _st())
    return rowmap, wmap


def block0_embed_norm_fwd(y0, gamma, beta, out, mean, rstd, pos, mask_token, wmap, B, g, cap_windows, C, eps=1e-5):
    _chk(y0, gamma, beta, out, mean, rstd, pos, mask_token, wmap)
    lib().call("nmh_block0_embed_norm_fwd", dt_of(y0), y0, out, gamma, beta, eps, mean, rstd, pos, mask_token, wmap, B, g, int(cap_windows), C, _st())
    return out


def block0_embed_norm_bwd(dx0, y0, gamma, mean, rstd, dy0, dgamma, dbeta, dmask_token, wmap, B, g, cap_windows, C):
    _chk(dx0, y0, gamma, mean, rstd, dy0, dgamma, dbeta, dmask_token, wmap)
    part = torch.empty((BLOCK0_LN_PARTIAL_ROWS, 3 * C), dtype=torch.float32, device=y0.device)
    lib().call("nmh_block0_embed_norm_bwd", dt_of(y0), dx0, y0, gamma, mean, rstd, dy0, dgamma, dbeta, dmask_token, part, part.numel(), wmap, B, g, int(cap_windows), C, _st())
    return dy0


def block0_expand(yc, wmap, B, g, cap_windows, C, out=None):
    """compact [B][cap_windows + 1][64][C] -> dense [B * g^3, C]"""
    _chk(yc, wmap, out)
    if yc.numel() != B * (cap_windows + 1) * 64 * C:
        raise RuntimeError("block0_expand: compact tensor must be [B][cap_windows + 1][64][C]")
    if out is None:
        out = torch.empty((B * g ** 3, C), dtype=yc.dtype, device=yc.device)
    lib().call("nmh_block0_expand", dt_of(yc), yc, out, wmap, B, g, int(cap_windows), C, _st())
    return out


def block0_reduce(dy, wmap, B, g, cap_windows, C, out=None):
    """dense gradient [B * g^3, C] -> compact [B * (cap_windows + 1) * 64, C]"""
    _chk(dy, wmap, out)
    if dy.numel() != B * g ** 3 * C:
        raise RuntimeError("block0_reduce: dense tensor must be [B][g^3][C]")
    if out is None:
        out = torch.empty((B * (cap_windows + 1) * 64, C), dtype=dy.dtype, device=dy.device)
    lib().call("nmh_block0_reduce", dt_of(dy), dy, out, wmap, B, g, int(cap_windows), C, _st())
    return out


def layernorm_bwd(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, rows, C, src_mode=0, geom: Optional[WinGeom] = None, dres=None,
                  mask=None, dmask_token=None, tokens_per_sample=1, dyw=None, dyw_scale=None, wq=None):
    """dyw (mode 0, with geom): second output = dx in window order times dyw_scale[sample] (fused window gather).
    wq (a WgradQueue): dgamma / dbeta leave the launch as per-workgroup partial sums and are added by a reduce queued with the stage's weight gradients"""
    _chk(dy, x, gamma, mean, rstd, dx, dgamma, dbeta, dres, mask, dmask_token, dyw, dyw_scale)
    if wq is not None and LN_DEFER_PARAM_GRADS and mask is None and src_mode != 2:
        nb = int(lib().call("nmh_layernorm_bwd_partial_rows", rows, C))
        part = torch.empty((nb, 2 * C), dtype=torch.float32, device=x.device)
        lib().call("nmh_layernorm_bwd_deferred", dt_of(x), src_mode, dy, x, gamma, mean, rstd, dres, dx, part, rows, C,
                   geom.carr if geom is not None else None, dyw, dyw_scale, tokens_per_sample, _st())
        wq.add_ln_partials(part, nb, C, dgamma, dbeta)
        return dx
    lib().call("nmh_layernorm_bwd", dt_of(x), src_mode, dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, C,
               geom.carr if geom is not None else None, mask, dmask_token, tokens_per_sample, dyw, dyw_scale, _st())
    return dx


def gemm_nt_window_scatter(A, W, out, resid, bias, rowscale, tokens_per_sample, geom: WinGeom):
    """out[tok] = resid[tok] + rowscale[sample] * (A[m] @ W^T + bias) for window-ordered rows m (proj + window reverse + residual)"""
    _chk(A, W, out, resid, bias, rowscale)
    M, K = A.shape
    N = W.shape[0]
    lib().call("nmh_gemm_nt_window_scatter", dt_of(A), A, A.stride(0), W, W.stride(0), M, N, K, out, resid, bias, rowscale, tokens_per_sample,
               geom.carr, _st())
    return out


# switches and thresholds of a Swin block's kernel path: model.plan_swin_block holds the rules (and the measurements behind the defaults)
TOKEN_BWD = __import__("os").environ.get("NMH_TOKEN_BWD", "1") != "0"   # padded stages: token-ordered backward, behind the fused and the unfused attention forward
MLP_FUSED = __import__("os").environ.get("NMH_MLP_FUSED", "1") != "0"
MLP_FUSED_MIN_ROWS = int(__import__("os").environ.get("NMH_MLP_FUSED_MIN_ROWS", "4096"))
MLP_FUSED_WIDTHS = tuple(int(v) for v in __import__("os").environ.get("NMH_MLP_FUSED_WIDTHS", "96").split(",") if v)


def mlp_fused_supported(C: int) -> bool:
    return bool(lib().call("nmh_mlp_fused_supported", C))


def mlp_fused_fwd(x1, gamma, beta, W1, b1, W2T, b2, rowscale=None, rows_per_scale=1, out=None, mean=None, rstd=None, eps=1e-5):
    """x2 = x1 + rowscale[row / rows_per_scale] * (gelu(LN(x1) @ W1^T + b1) @ W2 + b2) in one launch (bf16); W1 [4C,C], W2T = fc2.weight^T [4C,C]"""
    _chk(x1, gamma, beta, W1, b1, W2T, b2, rowscale, out, mean, rstd)
    M, C = x1.shape
    if out is None:
        out = torch.empty_like(x1)
    ev = _prof(("mlp_fused_fwd", M, C))
    lib().call("nmh_mlp_fused_fwd", x1, gamma, beta, W1, b1, W2T, b2, rowscale, rows_per_scale, out, mean, rstd, M, C, eps, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def mlp_fused_bwd(x1, dx2, gamma, beta, W1, b1, W2T, dgamma, dbeta, rowscale=None, rows_per_scale=1, dyw=None, dyw_scale=None, geom: Optional[WinGeom] = None, eps=1e-5):
    """-> (dx1, x1n, hact, dh); dgamma / dbeta accumulated; dyw (optional, with geom): dx1 in window order times dyw_scale[sample]"""
    _chk(x1, dx2, gamma, beta, W1, b1, W2T, dgamma, dbeta, rowscale, dyw, dyw_scale)
    M, C = x1.shape
    dx1, x1n = torch.empty_like(x1), torch.empty_like(x1)
    hact = torch.empty((M, 4 * C), dtype=x1.dtype, device=x1.device)
    dh = torch.empty_like(hact)
    ev = _prof(("mlp_fused_bwd", M, C))
    lib().call("nmh_mlp_fused_bwd", x1, dx2, gamma, beta, W1, b1, W2T, rowscale, rows_per_scale, dx1, x1n, hact, dh, dgamma, dbeta, dyw, dyw_scale,
               geom.carr if geom is not None else None, M, C, eps, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return dx1, x1n, hact, dh


# ---- fused Swin-block kernels (csrc/swin_block.hip): bf16, C = 96 * {1, 2, 4} ----
SWIN_ATTN_FWD, SWIN_MLP_FWD = range(2)   # weight-stream kinds (nmh_swin_pack)


class _SwinPackItem(ctypes.Structure):   # include/nerfmae_hip.h: nmh_swin_pack_item
    _fields_ = [("w0", ctypes.c_void_p), ("w1", ctypes.c_void_p), ("dst", ctypes.c_void_p), ("type", ctypes.c_int), ("C", ctypes.c_int)]


SWIN_FUSED = __import__("os").environ.get("NMH_SWIN", "1") != "0"
SWIN_ATTN_MIN_WINDOWS = int(__import__("os").environ.get("NMH_SWIN_ATTN_MIN_WIN", "100"))
SWIN_MLP_MIN_ROWS = int(__import__("os").environ.get("NMH_SWIN_MLP_MIN_ROWS", "6000"))
SWIN_MLP_WIDTHS = tuple(int(v) for v in __import__("os").environ.get("NMH_SWIN_MLP_WIDTHS", "192,384").split(",") if v)   # C = 96 keeps csrc/mlp_fused.hip (weights resident in LDS)
SWIN_ATTN_WIDTHS = tuple(int(v) for v in __import__("os").environ.get("NMH_SWIN_ATTN_WIDTHS", "96,192,384").split(",") if v)


def swin_supported(C: int) -> bool:
    return bool(lib().call("nmh_swin_supported", C))


def swin_stream_numel(kind: int, C: int) -> int:
    return int(lib().call("nmh_swin_stream_numel", kind, C))


def swin_pack_items(items):
    """items: [(w0, w1 | None, dst, kind, C)] -> ctypes array for swin_pack (built once; the pointers are stable: flat parameter buffer, packed buffer)"""
    arr = (_SwinPackItem * len(items))()
    for i, (w0, w1, dst, kind, C) in enumerate(items):
        _chk(w0, w1, dst)
        arr[i] = _SwinPackItem(w0.data_ptr(), w1.data_ptr() if w1 is not None else None, dst.data_ptr(), kind, C)
    return arr


def swin_pack(arr):
    lib().call("nmh_swin_pack", arr, len(arr), _st())


def swin_attn_fwd(x, gamma, beta, wstream, bqkv, table, bproj, geom: WinGeom, rowscale=None, rows_per_scale=1, eps=1e-5, token_saves=False):
    """-> (x1, xnw, mean, rstd, qkv, o, lse): the whole attention branch of a Swin block in one launch (+ what its backward / weight gradients read).
    token_saves: xnw and o come back in token order, [T, C] (for the token-ordered backward: window_attn_bwd_tokens)"""
    _chk(x, gamma, beta, wstream, bqkv, table, bproj, rowscale)
    T, C = x.shape
    heads = C // 32
    dev, dt = x.device, x.dtype
    x1 = torch.empty_like(x)
    xnw = torch.empty((T if token_saves else geom.rows, C), dtype=dt, device=dev)
    mean, rstd = torch.empty(T, device=dev), torch.empty(T, device=dev)
    qkv = torch.empty((geom.rows, 3 * C), dtype=dt, device=dev)
    o = torch.empty((T if token_saves else geom.rows, C), dtype=dt, device=dev)
    lse = torch.empty(geom.rows * heads, device=dev)
    ev = _prof(("swin_attn_fwd", geom.rows, C))
    lib().call("nmh_swin_attn_fwd", x, gamma, beta, wstream, bqkv, table, bproj, rowscale, rows_per_scale, xnw, mean, rstd, qkv, o, lse, x1, geom.carr, C, eps,
               int(token_saves), _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return x1, xnw, mean, rstd, qkv, o, lse


SWIN_MLP_SPLIT = __import__("os").environ.get("NMH_SWIN_SPLIT", "1") != "0"
_SPLIT_WS = {}


def swin_mlp_split_ws(M, C, device):
    """the zero-initialised workspace of the two-workgroups-per-tile MLP forward (None: this shape runs one workgroup per tile); one per shape, device AND
    stream: the blocks of a stage share it (their launches are ordered on the stream and each leaves the arrival counters zero), launches of the same shape on
    another stream -- a second model instance, a standalone stage -- get their own, so that they cannot corrupt each other's counters and partial sums.
    A workspace is never allocated inside a stream capture (it would come from the graph's private pool and outlive the graph in this table): during a
    capture the entry of the capture stream must already exist -- GraphedTrainStep warms up on the stream it then captures on -- and a missing one raises.
    (A launch that aborts half-way leaves non-zero counters behind: swin_mlp_split_ws_reset() clears them.)"""
    key = (device.index, M, C, torch.cuda.current_stream(device).cuda_stream)
    if key not in _SPLIT_WS:
        n = int(lib().call("nmh_swin_mlp_split_ws_bytes", M, C))
        if n > 0 and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("split-MLP workspace requested for the first time inside a stream capture: run one eager step on the capture stream first")
        _SPLIT_WS[key] = torch.zeros(n, dtype=torch.uint8, device=device) if n > 0 else None
    return _SPLIT_WS[key]


def swin_mlp_split_ws_reset(drop: bool = False):
    """zero every split-MLP workspace (after a failed / aborted launch, and at the start of every graph capture: the arrival counters must be zero before the
    next launch); drop=True releases them instead (trainer reset / a stream that is gone)"""
    if drop:
        _SPLIT_WS.clear()
        return
    for ws in _SPLIT_WS.values():
        if ws is not None:
            ws.zero_()


def swin_mlp_split_ws_drop_stream(stream_handle: int):
    """release the workspaces keyed by a stream that is going away (a GraphedTrainStep being deleted)"""
    for k in [k for k in _SPLIT_WS if k[3] == stream_handle]:
        del _SPLIT_WS[k]


def swin_mlp_fwd(x1, gamma, beta, wstream, b1, b2, rowscale=None, rows_per_scale=1, eps=1e-5, want_hact=False, split=None):
    """-> (x2, x1n, hp, mean, rstd[, hact]): the MLP branch in one launch; hp = fc1 pre-activation [M, 4C], hact = gelu(hp) on request.
    split (default SWIN_MLP_SPLIT): two workgroups per 64-row tile where the tiles alone leave half of the chip idle (C = 384, <= 8192 rows)"""
    _chk(x1, gamma, beta, wstream, b1, b2, rowscale)
    M, C = x1.shape
    dev = x1.device
    ws = swin_mlp_split_ws(M, C, dev) if (SWIN_MLP_SPLIT if split is None else split) else None
    x2, x1n = torch.empty_like(x1), torch.empty_like(x1)
    hp = torch.empty((M, 4 * C), dtype=x1.dtype, device=dev)
    mean, rstd = torch.empty(M, device=dev), torch.empty(M, device=dev)
    hact = torch.empty_like(hp) if want_hact else None
    ev = _prof(("swin_mlp_fwd", M, C))
    lib().call("nmh_swin_mlp_fwd", x1, gamma, beta, wstream, b1, b2, rowscale, rows_per_scale, x2, x1n, hp, hact, mean, rstd, M, C, eps,
               ws, ws.numel() if ws is not None else 0, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return (x2, x1n, hp, mean, rstd, hact) if want_hact else (x2, x1n, hp, mean, rstd)


def window_scatter_residual(yw, x, out, rowscale, C, geom: WinGeom):
    _chk(yw, x, out, rowscale)
    lib().call("nmh_window_scatter_residual", dt_of(x), yw, x, out, rowscale, C, geom.carr, _st())
    return out


def window_gather_scale(dx, dyw, rowscale, C, geom: WinGeom):
    _chk(dx, dyw, rowscale)
    lib().call("nmh_window_gather_scale", dt_of(dx), dx, dyw, rowscale, C, geom.carr, _st())
    return dyw


def window_attn_fwd(qkv, bias_table, out, lse, heads, C, geom: WinGeom):
    _chk(qkv, bias_table, out, lse)
    lib().call("nmh_window_attn_fwd", dt_of(qkv), qkv, bias_table, out, lse, heads, C, geom.carr, _st())
    return out


def window_attn_bwd(qkv, bias_table, dout, lse, dqkv, dbias_table, heads, C, geom: WinGeom):
    _chk(qkv, bias_table, dout, lse, dqkv, dbias_table)
    lib().call("nmh_window_attn_bwd", dt_of(qkv), qkv, bias_table, dout, lse, dqkv, dbias_table, heads, C, geom.carr, _st())
    return dqkv


def layernorm_fwd_window_tokens(x, gamma, beta, out_window, out_tokens, mean, rstd, C, geom: WinGeom, eps=1e-5):
    """LN1 with the pad -> roll -> partition gather (out_window [geom.rows, C]) plus a token-ordered copy (out_tokens [T, C])"""
    _chk(x, gamma, beta, out_window, out_tokens, mean, rstd)
    lib().call("nmh_layernorm_fwd_window_tokens", dt_of(x), x, out_window, out_tokens, gamma, beta, eps, mean, rstd, geom.rows, C, geom.carr, _st())


def window_attn_fwd_tokens(qkv, bias_table, out_tok, lse, heads, C, geom: WinGeom):
    """window attention core with its output in token order (out_tok [T, C])"""
    _chk(qkv, bias_table, out_tok, lse)
    lib().call("nmh_window_attn_fwd_tokens", dt_of(qkv), qkv, bias_table, out_tok, lse, heads, C, geom.carr, _st())
    return out_tok


def window_attn_bwd_tokens(qkv, bias_table, dout_tok, lse, dqkv_tok, dqkv_pad, dbias_table, heads, C, geom: WinGeom):
    """attention-core backward with token-ordered dO in / d(qkv) out (include/nerfmae_hip.h: nmh_window_attn_bwd_tokens); dqkv_pad [geom.rows, 3C] receives the pad rows"""
    _chk(qkv, bias_table, dout_tok, lse, dqkv_tok, dqkv_pad, dbias_table)
    lib().call("nmh_window_attn_bwd_tokens", dt_of(qkv), qkv, bias_table, dout_tok, lse, dqkv_tok, dqkv_pad, dbias_table, heads, C, geom.carr, _st())
    return dqkv_tok


def window_pad_rows_colsum(x, out, geom: WinGeom):
    """out[n] += sum of x[row][n] over the window rows that hold no token"""
    _chk(x, out)
    lib().call("nmh_window_pad_rows_colsum", dt_of(x), x, x.shape[1], geom.carr, out, _st())


def window_pad_rows_colsum_grouped(items, geom: WinGeom):
    """items: [(x, out)] of one geometry and width -> one launch (nmh_window_pad_rows_colsum_grouped)"""
    if not items:
        return
    n = len(items)
    xs, outs = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    N, dt = items[0][0].shape[1], dt_of(items[0][0])
    for i, (x, out) in enumerate(items):
        _chk(x, out)
        if x.shape[1] != N or dt_of(x) != dt:
            raise ValueError("window_pad_rows_colsum_grouped: one width / dtype per call")
        xs[i], outs[i] = x.data_ptr(), out.data_ptr()
    lib().call("nmh_window_pad_rows_colsum_grouped", dt, xs, outs, n, N, geom.carr, _st())


def instnorm_stats(x, stats, scratch, B, V, C, eps=1e-5):
    _chk(x, stats, scratch)
    lib().call("nmh_instnorm_stats", dt_of(x), x, stats, scratch, B, V, C, eps, _st())
    return stats


def instnorm_finalize(acc, stats, B, V, C, eps=1e-5):
    _chk(acc, stats)
    lib().call("nmh_instnorm_finalize", acc, stats, B, V, C, eps, _st())
    return stats


def instnorm_apply(x, stats, out, B, V, C, r=None, stats_r=None, rmode=0, slope=0.01):
    _chk(x, stats, out, r, stats_r)
    ev = _prof(("instnorm_apply", B, V, C, rmode), (2 + (rmode != 0)) * x.numel() * x.element_size())
    lib().call("nmh_instnorm_apply", dt_of(x), x, stats, r, stats_r, rmode, out, B, V, C, slope, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return out


def instnorm_bwd_reduce(dout, out, x, stats, sums, B, V, C, r=None, stats_r=None, sums_r=None, rmode=0, slope=0.01):
    _chk(dout, out, x, stats, sums, r, stats_r, sums_r)
    ev = _prof(("instnorm_bwd_reduce", B, V, C, rmode), (2 + (out is not None) + (rmode == 2)) * x.numel() * x.element_size())
    lib().call("nmh_instnorm_bwd_reduce", dt_of(x), dout, out, x, stats, r, stats_r, rmode, sums, sums_r, B, V, C, slope, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())


def instnorm_bwd_apply(dout, out, x, stats, sums, dx, B, V, C, r=None, stats_r=None, sums_r=None, rmode=0, dr=None,
                       dr_accumulate=False, slope=0.01):
    _chk(dout, out, x, stats, sums, dx, r, stats_r, sums_r, dr)
    ev = _prof(("instnorm_bwd_apply", B, V, C, rmode),
               (3 + (out is not None) + (rmode == 2) + (dr is not None) * (1 + int(dr_accumulate))) * x.numel() * x.element_size())
    lib().call("nmh_instnorm_bwd_apply", dt_of(x), dout, out, x, stats, sums, r, stats_r, sums_r, rmode, dx, dr, int(dr_accumulate),
               B, V, C, slope, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())


INBWD_BG = __import__("os").environ.get("NMH_INBWD_BG", "1") != "0"   # decoder-1: IN backward on a forked stream beside conv2's weight gradient (same-box A/B: -0.7 ms at 8 grids)


def instnorm_bwd_apply_bg(dout, x, stats, sums, dx, B, V, C, slope=0.01):
    """nmh_instnorm_bwd_apply(rmode 0, out = None) as a one-workgroup-per-CU background launch (bf16, C = 48)"""
    _chk(dout, x, stats, sums, dx)
    ev = _prof(("instnorm_bwd_apply_bg", B, V, C), 3 * x.numel() * x.element_size())
    lib().call("nmh_instnorm_bwd_apply_bg", dt_of(x), dout, x, stats, sums, dx, B, V, C, slope, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())


def instnorm_bwd_apply_bg_centered(dout, z, stats, sums, dx, B, V, C, slope=0.01):
    """instnorm_bwd_apply_bg reading z = lrelu(y - mean) for y (centered decoder1)"""
    _chk(dout, z, stats, sums, dx)
    ev = _prof(("instnorm_bwd_apply_bg", B, V, C), 3 * z.numel() * z.element_size())
    lib().call("nmh_instnorm_bwd_apply_bg_centered", dt_of(z), dout, z, stats, sums, dx, B, V, C, slope, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())


def patch_embed_gather(x, A, B, R):
    _chk(x, A)
    lib().call("nmh_patch_embed_gather", dt_of(A), x, A, B, R, _st())
    return A


def upconv_fwd(x, Wt, bias, cat, B, v, k, Cin, Cout):
    """ConvTranspose3d(k=stride): cat[fine voxel][0:Cout] = x[coarse] @ Wt^T + bias (pixel shuffle in the GEMM epilogue)"""
    _chk(x, Wt, bias, cat)
    lib().call("nmh_upconv_fwd", dt_of(x), x, Wt, bias, cat, cat.stride(0), B, v, k, Cin, Cout, _st())
    return cat


def upconv_dgrad(dcat, Wd, dx, B, v, k, Cin, Cout):
    _chk(dcat, Wd, dx)
    lib().call("nmh_upconv_dgrad", dt_of(dcat), dcat, dcat.stride(0), Wd, dx, B, v, k, Cin, Cout, _st())
    return dx


def upconv_wgrad(dcat, x, dW, dbias, B, v, k, Cin, Cout):
    _chk(dcat, x, dW, dbias)
    if GROUPED_UPCONV_WGRAD and dcat.dtype == torch.bfloat16 and Cin % 8 == 0 and Cout % 8 == 0 and B * v ** 3 < 2 ** 31 and k * Cout <= 65535:
        return upconv_wgrad_grouped(dcat, x, dW, dbias, B, v, k, Cin, Cout)
    lib().call("nmh_upconv_wgrad", dt_of(dcat), dcat, dcat.stride(0), x, dW, dbias, B, v, k, Cin, Cout, _st())


# One grouped call for the whole gradient: the k taps along x of a (tz, ty) tap row are one problem -- its A rows are the k*Cout-element
# runs of the fine gradient (contiguous without a skip half; with one, k pieces of Cout at the row stride), folded back to (tx, co) by the
# kernel's two-level column map -- i.e. k^2 problems with full tiles, dcat read exactly once (1 grid/GPU, 40^3 -> 160^3: 416 -> 244 us
# against the split shuffled-view gemm_tn).  NMH_TNG_UP=0 keeps the shuffled-view kernel (fp32 always uses it).
GROUPED_UPCONV_WGRAD = int(__import__("os").environ.get("NMH_TNG_UP", "1"))


def upconv_wgrad_grouped(dcat, x, dW, dbias, B, v, k, Cin, Cout):
    """ConvTranspose3d(kernel = stride = k) weight / bias gradient as one nmh_gemm_tn_grouped call (bf16): dW[ci][co][tap] written
    through output strides, the bias gradient by atomic adds from every problem"""
    _chk(dcat, x, dW, dbias)
    k3, ldc, Vf = k ** 3, dcat.stride(0), v * k
    esz = dcat.element_size()
    arr = (_TnProblem * (k * k))()
    for t in range(k * k):   # problem (tz, ty): N = k*Cout columns (tx, co), tap index (tz*k + ty)*k + tx
        tz, ty = t // k, t % k
        off = ((tz * Vf + ty) * Vf) * ldc
        arr[t] = _TnProblem(dcat.data_ptr() + off * esz, ldc, x.data_ptr(), x.stride(0), dW.data_ptr() + (tz * k + ty) * k * 4, k3, dbias.data_ptr(), 0,
                            B * v ** 3, k * Cout, Cin, v ** 3, Cout * k3, k, v, 1, Cout, 1)
    ws = _tn_workspace(dcat.device)
    lib().call("nmh_gemm_tn_grouped", BF16, arr, k * k, ws, 0 if ws is None else ws.numel(), _st())


def upconv_shuffle_fwd(upre, bias, skip, out, B, v, k, Cout):
    _chk(upre, bias, skip, out)
    lib().call("nmh_upconv_shuffle_fwd", dt_of(upre), upre, bias, skip, out, B, v, k, Cout, _st())
    return out


def upconv_shuffle_bwd(dcat, dupre, dskip, dbias, B, v, k, Cout, has_skip):
    _chk(dcat, dupre, dskip, dbias)
    lib().call("nmh_upconv_shuffle_bwd", dt_of(dcat), dcat, dupre, dskip, dbias, B, v, k, Cout, int(has_skip), _st())


def mae_loss_fwd(d0, Wout, bout, target, extents, tokmask, B, R, Cd, sums, losses, pred=None, dpred=None):
    """sums: fp64[4] (fp64[8] when dpred [B*R^3, 4] fp32 is requested for mae_tail_bwd)"""
    _chk(d0, Wout, bout, target, extents, tokmask, sums, losses, pred, dpred)
    if dpred is not None and sums.numel() < 8:
        raise ValueError("mae_loss_fwd: sums needs 8 entries when dpred is requested")
    lib().call("nmh_mae_loss_fwd", dt_of(d0), d0, Wout, bout, target, extents, tokmask, B, R, Cd, sums, losses, pred, dpred, _st())
    return losses


def mae_loss_bwd(d0, Wout, bout, target, extents, tokmask, B, R, Cd, sums, dd0, dpred8, dWout, dbout):
    _chk(d0, Wout, bout, target, extents, tokmask, sums, dd0, dpred8, dWout, dbout)
    lib().call("nmh_mae_loss_bwd", dt_of(d0), d0, Wout, bout, target, extents, tokmask, B, R, Cd, sums, dd0, dpred8, dWout, dbout, _st())


def mae_tail_fwd(y, stats, r, d0, Wout, bout, target, extents, tokmask, B, R, C, sums, losses, pred=None, dpred=None, slope=0.01, bwd_sums=None, sign_mask=None):
    """d0 = lrelu(IN(y) + r), 1x1 head and loss terms in one pass (instnorm_apply rmode 1 + mae_loss_fwd); d0 = None: not stored"""
    _chk(y, stats, r, d0, Wout, bout, target, extents, tokmask, sums, losses, pred, dpred, bwd_sums, sign_mask)
    if sign_mask is not None and (bwd_sums is None or sign_mask.dtype != torch.uint8 or sign_mask.numel() < B * R ** 3 * 8 or C != 48):
        raise ValueError("mae_tail_fwd: sign_mask needs bwd_sums, 48 channels and B*R^3*8 bytes")
    if dpred is not None and sums.numel() < 8:
        raise ValueError("mae_tail_fwd: sums needs 8 entries when dpred is requested")
    if bwd_sums is not None and (dpred is None or bwd_sums.numel() < B * C * 4 + 4 * C):
        raise ValueError("mae_tail_fwd: bwd_sums needs dpred and B*C*4 + 4*C entries")
    # algorithmic bytes: y and r read once, the fp32 target (4 channels) read once, d(pred) (16 B / voxel) and d0 written if requested
    ev = _prof(("mae_tail_fwd", B, R, C), (2 + (d0 is not None)) * y.numel() * y.element_size() + B * R ** 3 * 16 * (1 + (dpred is not None) + (pred is not None))
               + (B * R ** 3 * 8 if sign_mask is not None else 0))
    lib().call("nmh_mae_tail_fwd", dt_of(y), y, stats, r, d0, Wout, bout, target, extents, tokmask, B, R, C, sums, losses, pred, dpred, slope, bwd_sums, sign_mask, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return losses


TAIL_FROM_COARSE = __import__("os").environ.get("NMH_TAIL_FROM_COARSE", "1") != "0"   # decoder1's tail forms the residual ConvT(x) from the coarse tensor (no 160^3 residual tensor)


def tail_residual_pack_numel() -> int:
    return int(lib().call("nmh_tail_residual_pack_numel"))


def tail_residual_pack(pack_ws, Wr):
    """the 64 phase weights of the k = s = 4 transpose conv as the MFMA fragments of mae_tail_fwd_from_coarse, from the scratch cconv_pack filled in this step"""
    _chk(pack_ws, Wr)
    if Wr.numel() < tail_residual_pack_numel() or Wr.dtype != torch.bfloat16:
        raise ValueError("tail_residual_pack: shapes")
    lib().call("nmh_tail_residual_pack", pack_ws, Wr, _st())


def tail_from_coarse_ok(R: int, C: int, Cin: int, dtype) -> bool:
    """shapes mae_tail_fwd_from_coarse takes (include/nerfmae_hip.h)"""
    return dtype == torch.bfloat16 and C == 48 and Cin == 96 and R % 4 == 0 and R <= 256 and ((R // 4) ** 3) % 16 == 0


# the tail walks each sample's valid box alone (csrc/tail_box.hpp): the zero padding of a scene contributes nothing to the loss or its gradient
TAIL_BOX = __import__("os").environ.get("NMH_TAIL_BOX", "1") != "0"


def mae_tail_fwd_from_coarse(y, stats, xcoarse, Wr, bt, Wout, bout, target, extents, tokmask, B, R, C, sums, losses, dpred, bwd_sums, sign_mask, pred=None, slope=0.01,
                             box=False):
    """mae_tail_fwd (training form: d(pred), the backward's sums and the sign mask are all written) with the residual ConvT_{k=s=4}(xcoarse) + bt formed inside.
    box=True: only the ceil(extent / 4) cells per axis of each sample's valid box are walked.  The caller vouches that `target` is zero outside the extents;
    dpred and sign_mask are then left UNWRITTEN outside the box (only mae_tail_bwd(..., extents=, R=) may consume them), and pred cannot be requested."""
    if box and pred is not None:
        raise ValueError("mae_tail_fwd_from_coarse: the box walk does not write pred")
    _chk(y, stats, xcoarse, Wr, bt, Wout, bout, target, extents, tokmask, sums, losses, pred, dpred, bwd_sums, sign_mask)
    if not tail_from_coarse_ok(R, C, xcoarse.shape[-1], y.dtype) or xcoarse.dtype != torch.bfloat16 or xcoarse.numel() != B * (R // 4) ** 3 * 96:
        raise ValueError("mae_tail_fwd_from_coarse: bf16, 48 channels from a 96-channel coarse tensor of edge R / 4, (R / 4)^3 a multiple of 16")
    if sums.numel() < 8 or bwd_sums.numel() < B * C * 4 + 4 * C or sign_mask.dtype != torch.uint8 or sign_mask.numel() < B * R ** 3 * 8 or dpred.numel() < B * R ** 3 * 4:
        raise ValueError("mae_tail_fwd_from_coarse: sums[8], bwd_sums[B*C*4 + 4*C], sign_mask[B*R^3*8], dpred[B*R^3*4]")
    ev = _prof(("mae_tail_fwd", B, R, C), y.numel() * y.element_size() + xcoarse.numel() * 2 + B * R ** 3 * (16 * (2 + (pred is not None)) + 8))
    lib().call("nmh_mae_tail_fwd_from_coarse_box" if box else "nmh_mae_tail_fwd_from_coarse", dt_of(y), y, stats, xcoarse, Wr, bt, Wout, bout, target, extents, tokmask,
               B, R, C, sums, losses, pred, dpred, slope, bwd_sums, sign_mask, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())
    return losses


def mae_tail_bwd(d0, y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, dWout, dbout, B, V, C, slope=0.01, r=None, bwd_sums=None, sign_mask=None, extents=None, R=None):
    """d0 may be None when r (the forward's residual input) is given: the kernel rebuilds d0 from y, stats and r.
    extents (+ R, V = R^3): dpred and sign_mask come from mae_tail_fwd_from_coarse(box=True) and hold each sample's box alone; outside it d(pred) = 0 is used unread"""
    _chk(d0, r, y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, dWout, dbout, bwd_sums, sign_mask, extents)
    if extents is not None:
        if R is None or R ** 3 != V or bwd_sums is None or sign_mask is None or d0 is not None or r is not None or extents.dtype != torch.int32 or extents.numel() < 3 * B:
            raise ValueError("mae_tail_bwd: the box walk takes extents int32 [B, 3] with R (V = R^3), bwd_sums and sign_mask, and neither d0 nor r")
        ev = _prof(("mae_tail_bwd", B, V, C), 3 * y.numel() * y.element_size() + B * V * 24)
        lib().call("nmh_mae_tail_bwd_box", dt_of(y), y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, slope, dWout, dbout, B, R, C, bwd_sums, sign_mask, extents, _st())
        if ev is not None:
            ev.record(torch.cuda.current_stream())
        return
    if d0 is None and r is None and (sign_mask is None or bwd_sums is None):
        raise ValueError("mae_tail_bwd needs d0, r, or the forward's sign mask together with its bwd_sums")
    # two passes (sums, then apply): y and r (or d0) read twice, d(pred) read twice, dy and dr written once
    # (with the forward's sign mask the apply pass reads y, 8 mask bytes and d(pred) per voxel and writes dy and dr: 3 tensor passes, not 4)
    nt = (3 if sign_mask is not None else 4) if bwd_sums is not None else 6
    ev = _prof(("mae_tail_bwd", B, V, C), nt * y.numel() * y.element_size() + (1 if bwd_sums is not None else 2) * B * V * 16
               + (B * V * 8 if sign_mask is not None and bwd_sums is not None else 0))
    lib().call("nmh_mae_tail_bwd", dt_of(y), d0, r, y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, slope, dWout, dbout, B, V, C, bwd_sums, sign_mask, _st())
    if ev is not None:
        ev.record(torch.cuda.current_stream())


GRID_ROT, GRID_FLIP0, GRID_FLIP1, GRID_DENSITY = 1, 2, 4, 8


def grid_prepare(src, dst, R, flags=0):
    """src: one stored scene (W,L,H,4) fp32|uint8 on the device; dst: (4,R,R,R) fp32 slot; returns the valid extents"""
    _chk(src, dst)
    if src.dim() != 4 or src.shape[3] != 4 or src.dtype not in (torch.float32, torch.uint8):
        raise ValueError("grid_prepare: src must be (W,L,H,4) float32 or uint8")
    W, L, H, _ = src.shape
    lib().call("nmh_grid_prepare", int(src.dtype == torch.uint8), src, W, L, H, dst, R, flags, _st())
    return (L, W, H) if flags & GRID_ROT else (W, L, H)


LABEL_PREPARE_DT = {torch.float32: 0, torch.int32: 1, torch.int64: 2, torch.uint8: 3}


def labels_prepare(src, dst, R, flags=0):
    """src: one stored label volume (W,L,H) fp32|int32|int64|uint8 on the device; dst: the (R,R,R) fp32 slot of the label batch; rotation and flips as
    grid_prepare (GRID_DENSITY means nothing here), zero = unlabelled padding; returns the valid extents"""
    _chk(src, dst)
    if src.dim() != 3 or src.dtype not in LABEL_PREPARE_DT:
        raise ValueError(f"labels_prepare: src must be (W,L,H) uint8, int32, int64 or float32, got {tuple(src.shape)} {src.dtype}")
    if dst.dtype != torch.float32 or dst.numel() != R ** 3:
        raise ValueError("labels_prepare: dst must be the (R,R,R) float32 slot")
    W, L, H = src.shape
    ext = (L, W, H) if flags & GRID_ROT else (W, L, H)
    if min(ext) < 1 or max(ext) > R:
        raise ValueError(f"labels_prepare: the result's extents {ext} must lie in 1..{R}")
    lib().call("nmh_labels_prepare", LABEL_PREPARE_DT[src.dtype], src, W, L, H, dst, R, flags, _st())
    return ext


def grid_prepare_rs(src, dst, R, flags=0, angle=0.0, scale=1.0):
    """grid_prepare with rotate_and_scale_scene's trilinear resample (nerf_rpn/datasets.py:478-512) of the augmented grid before the padding; returns
    the valid extents.  Always resamples: a scene that drew no rot-scale belongs in grid_prepare"""
    _chk(src, dst)
    if src.dim() != 4 or src.shape[3] != 4 or src.dtype not in (torch.float32, torch.uint8):
        raise ValueError("grid_prepare_rs: src must be (W,L,H,4) float32 or uint8")
    W, L, H, _ = src.shape
    if dst.dtype != torch.float32 or dst.numel() != 4 * R ** 3:
        raise ValueError("grid_prepare_rs: dst must be the (4,R,R,R) float32 slot")
    lib().call("nmh_grid_prepare_rs", int(src.dtype == torch.uint8), src, W, L, H, dst, R, flags, angle, scale, _st())
    return (L, W, H) if flags & GRID_ROT else (W, L, H)


BOX_SCENES_PER_LAUNCH = 64   # csrc/det_input.hip: NMH_BOX_SCENES


def boxes_augment(boxes, table, out=None):
    """boxes: [sum G, 6|7] fp32 on the device, the scenes' boxes concatenated; table: per scene (first row, count, flags, has_rs, (e0,e1,e2), angle, scale),
    e the scene's extents after rot / flips -> the boxes after augment_rpn_inputs' transforms (nerf_rpn/datasets.py:206-233, 514-522, z_up=True).  The table
    travels as kernel arguments (as step_params' values do): one launch per 64 scenes, no copy, no synchronisation"""
    _chk(boxes, out)
    if boxes.dim() != 2 or boxes.shape[1] not in (6, 7) or boxes.dtype != torch.float32 or not boxes.is_contiguous():
        raise ValueError("boxes_augment: boxes must be contiguous [N, 6|7] float32")
    if out is None:
        out = torch.empty_like(boxes)
    elif out.shape != boxes.shape or out.dtype != torch.float32 or not out.is_contiguous():
        raise ValueError("boxes_augment: out must match boxes")
    rows, cols = boxes.shape
    for first, count, flags, has_rs, ext, angle, scale in table:
        if first < 0 or count < 0 or first + count > rows or (has_rs and cols != 7):
            raise ValueError("boxes_augment: a scene's rows lie outside the boxes, or rot-scale on 6-column boxes")
    if rows == 0:
        return out
    if not table:
        out.copy_(boxes)
        return out
    for a in range(0, len(table), BOX_SCENES_PER_LAUNCH):
        part = table[a:a + BOX_SCENES_PER_LAUNCH]
        it = [int(v) for first, count, flags, has_rs, ext, angle, scale in part for v in (first, count, flags, bool(has_rs), ext[0], ext[1], ext[2])]
        ft = [float(v) for first, count, flags, has_rs, ext, angle, scale in part for v in (angle, scale)]
        # every launch writes all rows (rows of scenes outside its part are copied); later parts therefore transform in place
        lib().call("nmh_boxes_augment", boxes if a == 0 else out, out, cols, rows, len(part), (ctypes.c_int * len(it))(*it), (ctypes.c_float * len(ft))(*ft), _st())
    return out


def bias_grad(dY, db, M, N, rowscale=None, rows_per_scale=1):
    _chk(dY, db, rowscale)
    lib().call("nmh_bias_grad", dt_of(dY), dY, db, M, N, rowscale, rows_per_scale, _st())


def step_params(tokmask=None, block_bits=None, nb=0, g=0, hyper=None, hyper_dev=None, extents=None, extents_dev=None):
    """per-step host parameters as kernel arguments of one launch (no H2D copies): block_bits = numpy uint8 array of nb^3 {0,1} in raster
    order -> token mask [g^3]; hyper = 8 floats -> hyper_dev; extents = [B][3] ints -> extents_dev"""
    import numpy as np
    _chk(tokmask, hyper_dev, extents_dev)
    bits = hy = ex = None
    if tokmask is not None:
        packed = np.packbits(np.asarray(block_bits, dtype=np.uint8).reshape(-1), bitorder="little")
        packed = np.concatenate([packed, np.zeros((-len(packed)) % 4, dtype=np.uint8)])
        bits = (ctypes.c_uint32 * max(1, len(packed) // 4)).from_buffer_copy(packed.tobytes() or b"\0\0\0\0")
    if hyper is not None:
        hy = (ctypes.c_float * 8)(*[float(v) for v in hyper])
    n_ext = 0
    if extents is not None:
        flat = [int(v) for row in extents for v in row]
        n_ext = len(flat)
        ex = (ctypes.c_int * max(1, n_ext))(*flat)
    lib().call("nmh_step_params", bits, nb, g, tokmask, hy, hyper_dev, ex, n_ext, extents_dev, _st())


def grad_to_bf16(g, bucket):
    """fp32 gradient range -> bf16 bucket (data-parallel exchange at half the bytes)"""
    _chk(g, bucket)
    lib().call("nmh_grad_to_bf16", g, bucket, g.numel(), _st())
    return bucket


def grad_from_bf16(bucket, g, scale=1.0):
    _chk(g, bucket)
    lib().call("nmh_grad_from_bf16", bucket, g, g.numel(), scale, _st())
    return g


class AccArena:
    """Pre-zeroed accumulator arena (include/nerfmae_hip.h: nmh_set_prezeroed_arena).  `take` hands out zeroed fp64 slices that are used
    ONCE (reduce into, read back) before the next `begin`; `begin` -- called where a step starts to use them -- clears the WHOLE arena
    with one launch (4 MB: a microsecond of HBM time; clearing only the used part would make the launch depend on the history of
    previous steps, which a captured graph does not replay).  Slices that do not fit come from `torch.empty` (outside the registered
    range, so the library clears them itself): the arena is an optimisation, never a correctness dependency.  One per process."""

    BYTES = 4 << 20
    enabled = __import__("os").environ.get("NMH_ACC_ARENA", "1") != "0"
    _inst = None

    def __init__(self, device):
        self.buf = torch.zeros(self.BYTES // 8, dtype=torch.float64, device=device)
        self.off = 0        # doubles handed out since the last begin()
        lib().call("nmh_set_prezeroed_arena", self.buf, self.BYTES)

    @classmethod
    def get(cls, device):
        if not cls.enabled:
            return None
        if cls._inst is None:
            if torch.cuda.is_current_stream_capturing():   # never born inside a graph's private memory pool
                return None
            cls._inst = cls(device)
        return cls._inst if cls._inst.buf.device == torch.device(device) else None

    def begin(self):
        lib().call("nmh_fill_f32", self.buf, 0.0, self.BYTES // 4, _st())
        self.off = 0

    def take(self, shape):
        n = 1
        for d in shape:
            n *= int(d)
        n_al = (n + 15) // 16 * 16   # 128-byte slices
        if self.off + n_al > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n].view(*shape)
        self.off += n_al
        return t


def acc_zeros(shape, device):
    """an fp64 accumulator for ONE reduce-and-read use: a zeroed arena slice when the arena is active, else an uninitialised tensor (the
    entry point it is passed to clears accumulators outside the arena itself)"""
    ar = AccArena.get(device)
    t = ar.take(shape) if ar is not None else None
    return t if t is not None else torch.empty(shape, dtype=torch.float64, device=device)


def add(a, b):
    """a + b into a fresh tensor (HIP kernel; used for the two gradients of a feature map with two consumers)"""
    _chk(a, b)
    out = torch.empty_like(a)
    lib().call("nmh_add", dt_of(a), a, b, out, a.numel(), _st())
    return out


def add_inplace(a, b):
    _chk(a, b)
    lib().call("nmh_add_inplace", dt_of(a), a, b, a.numel(), _st())
    return a


def pack_weights(dt, descs_dev, blk2desc_dev, blkstart_dev, nblocks):
    lib().call("nmh_pack_weights", dt, descs_dev, blk2desc_dev, blkstart_dev, nblocks, _st())


def grad_sqnorm(g, acc):
    lib().call("nmh_grad_sqnorm", g, g.numel(), acc, _st())


def clip_coef(acc, max_norm, coef, norm_out=None):
    lib().call("nmh_clip_coef", acc, max_norm, coef, norm_out, _st())


def clip_coef_mean(acc, max_norm, inv_k_dev, coef, norm_out=None):
    """clip_coef for a gradient buffer that holds the SUM of k micro-gradients: coef = inv_k * (clip coefficient of the mean), norm_out = the mean's norm"""
    _chk(inv_k_dev, coef, norm_out)
    lib().call("nmh_clip_coef_mean", acc, max_norm, inv_k_dev, coef, norm_out, _st())


def grad_scale(inv_k, inv_k_dev):
    """1 / k -> the device scalar clip_coef_mean reads, as a kernel argument (no copy, no host wait; not graph-capturable, like step_params)"""
    _chk(inv_k_dev)
    lib().call("nmh_grad_scale", float(inv_k), inv_k_dev, _st())


def adamw_step(p, g, m, v, hyper, coef=None):
    lib().call("nmh_adamw_step", p, g, m, v, p.numel(), hyper, coef, _st())


ADAMW_MAX_RANGES = 4096   # NMH_ADAMW_MAX_RANGES of include/nerfmae_hip.h (tests/test_param_ranges_cpu.py compares the two)


def _range_table(bounds, scale):
    """the device table of the two *_ranges entries: bounds int64 [R+1], scale fp32 [R, 2] -> R"""
    R = bounds.numel() - 1
    if bounds.dtype != torch.int64 or scale.dtype != torch.float32 or tuple(scale.shape) != (R, 2) or not (bounds.is_contiguous() and scale.is_contiguous()):
        raise TypeError(f"range table: bounds int64 [R+1] and scale float32 [R, 2], contiguous; got {bounds.dtype} {tuple(bounds.shape)}, {scale.dtype} {tuple(scale.shape)}")
    return R


def grad_sqnorm_ranges(g, bounds, scale, acc):
    """grad_sqnorm over the ranges whose lr_scale is not 0 (nmh_grad_sqnorm_ranges); NmhError for a table the entry refuses"""
    lib().call("nmh_grad_sqnorm_ranges", g, g.numel(), bounds, scale, _range_table(bounds, scale), acc, _st())


def adamw_step_ranges(p, g, m, v, hyper, bounds, scale, coef=None):
    """adamw_step with lr * lr_scale and weight_decay * wd_scale per range; lr_scale 0 freezes the range (nmh_adamw_step_ranges)"""
    lib().call("nmh_adamw_step_ranges", p, g, m, v, p.numel(), hyper, coef, bounds, scale, _range_table(bounds, scale), _st())


# ---- FPN neck (nerf_rpn/model/fpn.py) -----------------------------------------------------------------------
def conv3d_k3_bias(X, Wp, bias, Cout, out=None):
    """conv3d_k3 with a per-output-channel fp32 bias in the epilogue: X (B,D,H,W,Cin) channels-last, Wp packed [Cout][27][Cin]."""
    _chk(X, Wp, bias, out)
    B, D, H, W, Cin = X.shape
    if out is None:
        out = torch.empty((B, D, H, W, Cout), dtype=X.dtype, device=X.device)
    lib().call("nmh_conv3d_k3_bias", dt_of(X), X, Wp, bias, out, B, D, H, W, Cin, Cout, _st())
    return out


def nearest_upsample_add(coarse, fine):
    """fine (B,Df,Hf,Wf,C) += F.interpolate(coarse (B,Dc,Hc,Wc,C), size=fine, mode='nearest'), channels-last, in place."""
    _chk(coarse, fine)
    B, Dc, Hc, Wc, C = coarse.shape
    _, Df, Hf, Wf, _ = fine.shape
    lib().call("nmh_nearest_upsample_add", dt_of(fine), coarse, fine, B, Dc, Hc, Wc, Df, Hf, Wf, C, _st())
    return fine


def nearest_upsample_add_bwd(dfine, dcoarse):
    """adjoint of nearest_upsample_add: dcoarse += sum of dfine over the fine voxels that read each coarse voxel, in place."""
    _chk(dfine, dcoarse)
    B, Dc, Hc, Wc, C = dcoarse.shape
    _, Df, Hf, Wf, _ = dfine.shape
    lib().call("nmh_nearest_upsample_add_bwd", dt_of(dfine), dfine, dcoarse, B, Dc, Hc, Wc, Df, Hf, Wf, C, _st())
    return dcoarse


def ndhwc_to_ncdhw(x):
    """channels-last compute tensor (B,D,H,W,C) -> fp32 NCDHW (B,C,D,H,W)"""
    _chk(x)
    B, D, H, W, C = x.shape
    out = torch.empty((B, C, D, H, W), dtype=torch.float32, device=x.device)
    lib().call("nmh_ndhwc_to_ncdhw", dt_of(x), x, out, B, D * H * W, C, _st())
    return out


def ncdhw_to_ndhwc(g, dtype):
    """fp32 NCDHW gradient (B,C,D,H,W) -> channels-last (B,D,H,W,C) in the compute dtype"""
    g = g.float().contiguous()
    _chk(g)
    B, C, D, H, W = g.shape
    out = torch.empty((B, D, H, W, C), dtype=dtype, device=g.device)
    lib().call("nmh_ncdhw_to_ndhwc", dt_of(out), g, out, B, D * H * W, C, _st())
    return out


def copy_cols(src, dst):
    """dst[m, :C] = src[m, :C] for 2-D views with arbitrary row strides (unit column stride): skip connection <-> concatenated tensor"""
    if src.dim() != 2 or dst.dim() != 2 or src.shape != dst.shape or src.stride(1) != 1 or dst.stride(1) != 1 or src.dtype != dst.dtype:
        raise RuntimeError("copy_cols needs two 2-D views of equal shape and dtype with unit column stride")
    if not (src.is_cuda and dst.is_cuda):
        raise RuntimeError("nerf_mae_amd ops need HIP device tensors (no CPU fallback)")
    M, C = src.shape
    lib().call("nmh_copy_cols", dt_of(src), src, src.stride(0), dst, dst.stride(0), M, C, _st())
    return dst


# ---- voxel super-resolution / semantics heads (csrc/heads.hip) -----------------------------------------------------
def grid_to_cl8(xb, dtype):
    """(B,4,R,R,R) fp32 grid -> (B,R,R,R,8) channels-last in `dtype`, channels 4..7 zero"""
    _chk(xb)
    B, _, D, H, W = xb.shape
    out = torch.empty((B, D, H, W, 8), dtype=dtype, device=xb.device)
    lib().call("nmh_grid_to_cl8", dt_of(out), xb, out, B, D * H * W, _st())
    return out


def head_upsample_fwd(y, Co, B, R, Ro, inv_scale):
    """y [B*R^3][Cp] -> pred (B,Co,Ro,Ro,Ro) fp32 NCDHW, nearest upsampling with ATen's explicit-scale source index"""
    _chk(y)
    pred = torch.empty((B, Co, Ro, Ro, Ro), dtype=torch.float32, device=y.device)
    lib().call("nmh_head_upsample_fwd", dt_of(y), y, pred, B, Co, y.shape[1], R, Ro, inv_scale, _st())
    return pred


def head_upsample_bwd(dpred, Cp, R, dtype, inv_scale):
    _chk(dpred)
    B, Co, Ro = dpred.shape[0], dpred.shape[1], dpred.shape[2]
    g = torch.empty((B * R ** 3, Cp), dtype=dtype, device=dpred.device)
    lib().call("nmh_head_upsample_bwd", dt_of(g), dpred, g, B, Co, Cp, R, Ro, inv_scale, _st())
    return g


def add_cols_f32(src, dst, C):
    """dst[m][:C] += src[m][:C] for fp32 2-D views (rows = leading dim)"""
    _chk(src, dst)
    lib().call("nmh_add_cols_f32", src, src.stride(0), dst, dst.stride(0), src.shape[0], C, _st())
    return dst


def voxel_sr_loss_fwd(pred, target, sums, loss):
    _chk(pred, target, sums, loss)
    B = pred.shape[0]
    lib().call("nmh_voxel_sr_loss_fwd", pred, target, B, pred[0, 0].numel(), sums, loss, _st())


def voxel_sr_loss_bwd(pred, target, sums, gscale, dpred):
    _chk(pred, target, sums, dpred)
    lib().call("nmh_voxel_sr_loss_bwd", pred, target, pred.shape[0], pred[0, 0].numel(), sums, gscale, dpred, _st())


def masked_ce_fwd(logits, labels, class_weights, sums, iou_sums, out):
    _chk(logits, labels, class_weights, sums, iou_sums, out)
    B, K = logits.shape[:2]
    lib().call("nmh_masked_ce_fwd", logits, labels, class_weights, B, K, logits[0, 0].numel(), sums, iou_sums, out, _st())


def masked_ce_bwd(logits, labels, class_weights, sums, gscale, dlogits):
    _chk(logits, labels, class_weights, sums, dlogits)
    B, K = logits.shape[:2]
    lib().call("nmh_masked_ce_bwd", logits, labels, class_weights, B, K, logits[0, 0].numel(), sums, gscale, dlogits, _st())


SEM_EVAL_ROWS = 1024   # rows of the partial slabs (NMH_SEM_EVAL_ROWS): one per workgroup of the evaluation pass


def sem_eval(logits, labels, class_weights=None, totals=None):
    """logits (B,K,*) fp32, labels (B,*) fp32 class ids (0 = unlabelled), class_weights [K] fp32 or None, totals int64 [3][K-1] or None (+= {I, U, T} on the device)
    -> (out fp32[2] = {loss, mean soft IoU}, counts int64 [4][K-1] = {I, U, T, P}, pred_vis int64 (B,V), target_vis int64 (B,V)).  One read of the logits, two
    launches; only the outputs and the two partial slabs are allocated, and the host does not wait."""
    _chk(logits, labels, class_weights, totals)
    if logits.dtype != torch.float32 or labels.dtype != torch.float32 or (class_weights is not None and class_weights.dtype != torch.float32):
        raise RuntimeError("sem_eval: fp32 logits, labels and class weights")
    B, K = logits.shape[:2]
    V = logits[0, 0].numel()
    if labels.numel() != B * V or (class_weights is not None and class_weights.numel() != K):
        raise RuntimeError(f"sem_eval: labels (B,V) and class weights [K] for logits (B,K,V) = ({B},{K},{V}), got {tuple(labels.shape)}")
    if totals is not None and (totals.dtype != torch.int64 or tuple(totals.shape) != (3, K - 1)):
        raise RuntimeError(f"sem_eval: totals int64 [3][{K - 1}]")
    dev = logits.device
    n1 = max(K - 1, 1)
    fpart = torch.empty((SEM_EVAL_ROWS, 2 + 2 * n1), dtype=torch.float64, device=dev)
    ipart = torch.empty((SEM_EVAL_ROWS, 3 * n1), dtype=torch.int64, device=dev)
    out = torch.empty(2, dtype=torch.float32, device=dev)
    counts = torch.empty((4, n1), dtype=torch.int64, device=dev)
    pred_vis = torch.empty((B, V), dtype=torch.int64, device=dev)
    target_vis = torch.empty((B, V), dtype=torch.int64, device=dev)
    lib().call("nmh_sem_eval", logits, labels, class_weights, B, K, V, fpart, ipart, out, counts, pred_vis, target_vis, totals, _st())
    return out, counts, pred_vis, target_vis


_LABEL_DT = {torch.float32: 0, torch.int32: 1, torch.int64: 2}


def sem_label_counts(output, target, K):
    """two label tensors of one shape and dtype (fp32, int32 or int64) -> counts int64 [4][K-1] = {I, U, T, P} over the elements with target > 0"""
    _chk(output, target)
    if output.dtype != target.dtype or output.dtype not in _LABEL_DT or output.shape != target.shape:
        raise RuntimeError("sem_label_counts: output and target of one shape and one dtype out of fp32, int32, int64")
    dev = output.device
    n1 = max(int(K) - 1, 1)
    ipart = torch.empty((SEM_EVAL_ROWS, 3 * n1), dtype=torch.int64, device=dev)
    counts = torch.empty((4, n1), dtype=torch.int64, device=dev)
    lib().call("nmh_sem_label_counts", _LABEL_DT[output.dtype], output, target, output.numel(), int(K), ipart, counts, _st())
    return counts


# ---- the reference's two native downstream ops (csrc/rotated.hip) ------------------------------------------------------------------
ROI_CHANNELS_LAST, ROI_NCWLH = 0, 1


def _roi_args(rois, output_size):
    if rois.dim() != 2 or rois.shape[1] != 8 or rois.dtype != torch.float32:
        raise RuntimeError("rois must be an fp32 [N, 8] tensor: batch index, centre (w,l,h), size (w,l,h), angle in degrees")
    pw, pl, ph = (int(v) for v in output_size)
    return pw, pl, ph


def roi_align_rotated_3d_fwd(x, rois, output_size, spatial_scale, sampling_ratio, layout):
    """layout ROI_CHANNELS_LAST: x (B,W,L,H,C) fp32|bf16 -> [N,PW,PL,PH,C] in x's dtype; ROI_NCWLH: x (B,C,W,L,H) fp32 -> [N,C,PW,PL,PH]"""
    _chk(x, rois)
    pw, pl, ph = _roi_args(rois, output_size)
    n = rois.shape[0]
    if layout == ROI_CHANNELS_LAST:
        B, W, L, H, C = x.shape
        out = torch.empty((n, pw, pl, ph, C), dtype=x.dtype, device=x.device)
    else:
        B, C, W, L, H = x.shape
        out = torch.empty((n, C, pw, pl, ph), dtype=x.dtype, device=x.device)
    lib().call("nmh_roi_align_rotated_3d_fwd", layout, dt_of(x), x, rois, out, n, B, W, L, H, C, pw, pl, ph, spatial_scale, sampling_ratio, _st())
    return out


def roi_align_rotated_3d_bwd(dout, rois, input_shape, output_size, spatial_scale, sampling_ratio, layout):
    """-> fp32 gradient of shape input_shape (zeroed here, then summed into by fp32 atomic adds), whatever dout's dtype"""
    _chk(dout, rois)
    pw, pl, ph = _roi_args(rois, output_size)
    if layout == ROI_CHANNELS_LAST:
        B, W, L, H, C = input_shape
    else:
        B, C, W, L, H = input_shape
    dx = torch.zeros(tuple(input_shape), dtype=torch.float32, device=dout.device)
    lib().call("nmh_roi_align_rotated_3d_bwd", layout, dt_of(dout), dout, rois, dx, rois.shape[0], B, W, L, H, C, pw, pl, ph, spatial_scale, sampling_ratio, _st())
    return dx


def sort_vertices(vertices, mask, num_valid):
    """vertices [B,N,M,2] fp32, mask [B,N,M] bool, num_valid [B,N] int32 -> idx [B,N,9] int32"""
    _chk(vertices, mask, num_valid)
    if vertices.dtype != torch.float32 or mask.dtype != torch.bool or num_valid.dtype != torch.int32:
        raise RuntimeError("sort_vertices needs fp32 vertices, a bool mask and int32 num_valid")
    B, N, M = mask.shape
    if tuple(vertices.shape) != (B, N, M, 2) or tuple(num_valid.shape) != (B, N):
        raise RuntimeError("sort_vertices: vertices [B,N,M,2], mask [B,N,M], num_valid [B,N]")
    idx = torch.empty((B, N, 9), dtype=torch.int32, device=vertices.device)
    lib().call("nmh_sort_vertices", vertices, mask, num_valid, idx, B, N, M, _st())
    return idx


# ---- oriented 3-D box IoU / GIoU / DIoU, all-pairs IoU, rotated NMS (csrc/rotated_iou.hip) -------------------------------------------
OBB_IOU, OBB_GIOU_SMALLEST, OBB_GIOU_ALIGNED, OBB_DIOU_SMALLEST, OBB_DIOU_ALIGNED = range(5)
OBB_NMS_MAX = 16384


def obb_iou_fwd(mode, box1, box2, want_u3d=True, want_z_range=False, want_corners=False):
    """box1, box2 (..., 7) fp32 contiguous, same shape -> (iou, u3d, z_range, loss, corners1, corners2); entries not asked for (and loss in
    OBB_IOU mode) are None.  Nothing but the outputs is allocated and the host does not wait."""
    _chk(box1, box2)
    lead, n = tuple(box1.shape[:-1]), box1.numel() // 7
    new = lambda *tail: torch.empty(lead + tail, dtype=torch.float32, device=box1.device)   # noqa: E731
    iou = new()
    u3d = new() if want_u3d else None
    zr = new() if want_z_range else None
    loss = new() if mode != OBB_IOU else None
    c1, c2 = (new(4, 2), new(4, 2)) if want_corners else (None, None)
    lib().call("nmh_obb_iou_fwd", mode, box1, box2, n, iou, u3d, zr, loss, None, None, c1, c2, _st())
    return iou, u3d, zr, loss, c1, c2


def obb_iou_bwd(mode, box1, box2, g_iou, g_u3d, g_loss, need1, need2):
    """-> (dbox1, dbox2) in the boxes' shape, None for a side that is not needed; a None incoming gradient is zero, and one that is a single
    value expanded over all pairs (every stride 0: the gradient of a sum()) is read as that one value, not copied"""
    gs, g_one = [], 0
    for k, g in enumerate((g_iou, g_u3d, g_loss)):
        if g is not None and g.numel() > 1 and all(s == 0 for s in g.stride()):
            g, g_one = g.as_strided((), ()), g_one | (1 << k)
        gs.append(g)
    g_iou, g_u3d, g_loss = gs
    _chk(box1, box2, g_iou, g_u3d, g_loss)
    d1 = torch.empty_like(box1) if need1 else None
    d2 = torch.empty_like(box2) if need2 else None
    lib().call("nmh_obb_iou_bwd", mode, box1, box2, box1.numel() // 7, g_iou, g_u3d, g_loss, g_one, d1, d2, _st())
    return d1, d2


def obb_iou_pairwise(boxes1, boxes2):
    """[N,7] x [M,7] oriented or [N,6] x [M,6] axis-aligned fp32 -> iou [N,M]"""
    _chk(boxes1, boxes2)
    N, M, ncols = boxes1.shape[0], boxes2.shape[0], boxes1.shape[1]
    iou = torch.empty((N, M), dtype=torch.float32, device=boxes1.device)
    lib().call("nmh_obb_iou_pairwise", ncols, boxes1, boxes2, N, M, iou, _st())
    return iou


def obb_nms(boxes_sorted, categories, iou_threshold):
    """boxes_sorted [N,7|6] fp32 in descending score order, categories int32 [N] or None -> (keep int32 [N] positions, count int32 [1]) on the device"""
    _chk(boxes_sorted, categories)
    N, ncols = boxes_sorted.shape
    if N > OBB_NMS_MAX:
        raise ValueError(f"rotated NMS supports at most {OBB_NMS_MAX} boxes, got {N}")
    dev = boxes_sorted.device
    mask = torch.empty((N, (N + 63) // 64), dtype=torch.int64, device=dev)
    keep = torch.empty((N,), dtype=torch.int32, device=dev)
    count = torch.empty((1,), dtype=torch.int32, device=dev)
    lib().call("nmh_obb_nms_mask", ncols, boxes_sorted, categories, N, iou_threshold, mask, _st())
    lib().call("nmh_obb_nms_scan", mask, N, keep, count, _st())
    return keep, count


# ---- FCOS target assignment and training losses (csrc/fcos.hip) ----------------------------------------------------------------------------
FCOS_MAX_SCENES, FCOS_MAX_LEVELS = 64, 4
FCOS_LOSS_TYPES = {"iou": 0, "linear_iou": 1, "giou": 2, "diou": 3}


def _ptr_table(tensors, n=None):
    """device tensors -> host array of their pointers (None -> NULL); n: the length the entry expects, a plan's level count"""
    assert n is None or len(tensors) == n
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class FcosPlan:
    """feature sizes [(w,l,h)] and strides of 1..4 levels, N scenes -> the host-side level table of the fcos entries, the locations per level
    and in all (P = N sum n_k), and the size of the partial-sum workspace"""

    def __init__(self, feature_sizes, strides, N):
        feature_sizes = [tuple(int(v) for v in f) for f in feature_sizes]
        if not 1 <= len(feature_sizes) <= FCOS_MAX_LEVELS or len(strides) != len(feature_sizes):
            raise ValueError(f"FCOS ops take 1 to {FCOS_MAX_LEVELS} levels with one stride each, got {len(feature_sizes)} sizes and {len(strides)} strides")
        if not 1 <= N <= FCOS_MAX_SCENES:
            raise ValueError(f"FCOS ops take 1 to {FCOS_MAX_SCENES} scenes, got {N}")
        self.L, self.N, self.sizes, self.strides = len(feature_sizes), int(N), feature_sizes, [int(s) for s in strides]
        self.n = [w * l * h for w, l, h in feature_sizes]
        self.P = self.N * sum(self.n)
        self.dims = (ctypes.c_int * (4 * self.L))(*[v for f, s in zip(feature_sizes, self.strides) for v in (*f, s)])
        self.nblocks = lib().cdll.nmh_fcos_num_blocks(self.L, self.dims, self.N)
        if self.nblocks <= 0:
            raise ValueError(f"FCOS ops: unsupported level table {feature_sizes} x {self.strides}")

    def workspace(self, device):
        return torch.empty((2 * self.nblocks,), dtype=torch.float32, device=device)


def fcos_assign(plan, boxes, offsets, ncols, grid_sizes, masks, radius, norm_targets):
    """boxes [G,6|7] fp32 (may be empty), offsets host ints [N+1], grid_sizes int32 [N,3] or None, masks per-level bool / uint8 tensors or None
    -> (labels [P], targets [P,6|8], gt_index [P] int32, ctr_targets [P], valid [P] bool, scalars [2], partials workspace)"""
    _chk(boxes, grid_sizes, *(masks or ()))
    dev = boxes.device
    C = 6 if ncols == 6 else 8
    labels = torch.empty((plan.P,), dtype=torch.float32, device=dev)
    targets = torch.empty((plan.P, C), dtype=torch.float32, device=dev)
    gt_index = torch.empty((plan.P,), dtype=torch.int32, device=dev)
    ctr_t = torch.empty((plan.P,), dtype=torch.float32, device=dev)
    valid = torch.empty((plan.P,), dtype=torch.bool, device=dev)
    scalars = torch.empty((2,), dtype=torch.float32, device=dev)
    partials = plan.workspace(dev)
    offs = (ctypes.c_int * (plan.N + 1))(*offsets)
    lib().call("nmh_fcos_assign", plan.L, plan.dims, plan.N, ncols, boxes if boxes.numel() else None, offs, grid_sizes, _ptr_table(masks, plan.L) if masks else None, radius,
               int(bool(norm_targets)), labels, targets, gt_index, ctr_t, valid, partials, scalars, _st())
    return labels, targets, gt_index, ctr_t, valid, scalars, partials


def fcos_focal_fwd(plan, cls, labels, valid, scalars, world, partials):
    loss = torch.empty((), dtype=torch.float32, device=labels.device)
    lib().call("nmh_fcos_focal_fwd", plan.L, plan.dims, plan.N, _ptr_table(cls, plan.L), labels, valid, scalars, world, partials, loss, _st())
    return loss


def fcos_focal_bwd(plan, cls, labels, valid, scalars, world, g_loss):
    dcls = [torch.empty_like(t) for t in cls]
    lib().call("nmh_fcos_focal_bwd", plan.L, plan.dims, plan.N, _ptr_table(cls, plan.L), labels, valid, scalars, world, g_loss, _ptr_table(dcls, plan.L), _st())
    return dcls


def fcos_pos_fwd(plan, ncols, loss_type, add_l1, reg, ctr, labels, targets, ctr_t, valid, scalars, world, partials):
    reg_loss = torch.empty((), dtype=torch.float32, device=labels.device)
    ctr_loss = torch.empty((), dtype=torch.float32, device=labels.device)
    lib().call("nmh_fcos_pos_fwd", plan.L, plan.dims, plan.N, ncols, loss_type, int(bool(add_l1)), _ptr_table(reg, plan.L), _ptr_table(ctr, plan.L), labels, targets, ctr_t, valid, scalars, world,
               partials, reg_loss, ctr_loss, _st())
    return reg_loss, ctr_loss


def fcos_pos_bwd(plan, ncols, loss_type, add_l1, reg, ctr, labels, targets, ctr_t, valid, scalars, world, g_reg, g_ctr):
    dreg, dctr = [torch.empty_like(t) for t in reg], [torch.empty_like(t) for t in ctr]
    lib().call("nmh_fcos_pos_bwd", plan.L, plan.dims, plan.N, ncols, loss_type, int(bool(add_l1)), _ptr_table(reg, plan.L), _ptr_table(ctr, plan.L), labels, targets, ctr_t, valid, scalars, world,
               g_reg, g_ctr, _ptr_table(dreg, plan.L), _ptr_table(dctr, plan.L), _st())
    return dreg, dctr


def fcos_pos2d_fwd(plan, loss_type, add_l1, proj2d_weight, reg, ctr, labels, targets, ctr_t, valid, scalars, world, partials):
    """fcos_pos_fwd with the 2-D projection term (8 regression columns only)"""
    reg_loss = torch.empty((), dtype=torch.float32, device=labels.device)
    ctr_loss = torch.empty((), dtype=torch.float32, device=labels.device)
    lib().call("nmh_fcos_pos2d_fwd", plan.L, plan.dims, plan.N, 8, loss_type, int(bool(add_l1)), proj2d_weight, _ptr_table(reg, plan.L), _ptr_table(ctr, plan.L), labels, targets, ctr_t, valid,
               scalars, world, partials, reg_loss, ctr_loss, _st())
    return reg_loss, ctr_loss


def fcos_pos2d_bwd(plan, loss_type, add_l1, proj2d_weight, reg, ctr, labels, targets, ctr_t, valid, scalars, world, g_reg, g_ctr):
    dreg, dctr = [torch.empty_like(t) for t in reg], [torch.empty_like(t) for t in ctr]
    lib().call("nmh_fcos_pos2d_bwd", plan.L, plan.dims, plan.N, 8, loss_type, int(bool(add_l1)), proj2d_weight, _ptr_table(reg, plan.L), _ptr_table(ctr, plan.L), labels, targets, ctr_t, valid,
               scalars, world, g_reg, g_ctr, _ptr_table(dreg, plan.L), _ptr_table(dctr, plan.L), _st())
    return dreg, dctr


def fcos_obb_encode(locations, boxes):
    _chk(locations, boxes)
    out = torch.empty((boxes.shape[0], 8), dtype=torch.float32, device=boxes.device)
    lib().call("nmh_fcos_obb_encode", locations, boxes, boxes.shape[0], out, _st())
    return out


def fcos_obb_decode_fwd(locations, regression):
    _chk(locations, regression)
    out = torch.empty((regression.shape[0], 7), dtype=torch.float32, device=regression.device)
    lib().call("nmh_fcos_obb_decode_fwd", locations, regression, regression.shape[0], out, _st())
    return out


def fcos_obb_decode_bwd(regression, gbox):
    _chk(regression, gbox)
    d = torch.empty_like(regression)
    lib().call("nmh_fcos_obb_decode_bwd", regression, gbox, regression.shape[0], d, _st())
    return d


# ---- FCOS inference post-processing (csrc/fcos_post.hip) -----------------------------------------------------------------------------------
FCOS_POST_MASK_BYTES_MAX = 1 << 30          # the suppression workspace N cap^2 / 8 of one call


class FcosPostPlan:
    """locations per level and scene, N scenes, pre_nms_top_n -> the host-side level table of the fcos_post entries, cap = sum over the levels
    of min(pre_nms_top_n, n_k) and the level's first slot"""

    def __init__(self, level_n, N, pre_nms_top_n):
        self.L, self.N, self.n, self.top_n = len(level_n), int(N), [int(v) for v in level_n], int(pre_nms_top_n)
        if not 1 <= self.L <= FCOS_MAX_LEVELS:
            raise ValueError(f"FCOS post-processing takes 1 to {FCOS_MAX_LEVELS} levels, got {self.L}")
        if not 1 <= self.N <= FCOS_MAX_SCENES:
            raise ValueError(f"FCOS post-processing takes 1 to {FCOS_MAX_SCENES} scenes, got {self.N}")
        if self.top_n < 1 or min(self.n) < 1:
            raise ValueError(f"FCOS post-processing: pre_nms_top_n >= 1 and at least one location per level, got {self.top_n} and {self.n}")
        self.cap = sum(min(self.top_n, n) for n in self.n)
        if self.cap > OBB_NMS_MAX:
            raise ValueError(f"FCOS post-processing keeps at most {OBB_NMS_MAX} boxes per scene before NMS, got cap = {self.cap}; lower pre_nms_top_n")
        self.mask_bytes = self.N * self.cap * ((self.cap + 63) // 64) * 8
        if self.mask_bytes > FCOS_POST_MASK_BYTES_MAX:
            raise ValueError(f"FCOS post-processing: the suppression workspace of {self.N} scenes x cap {self.cap} takes {self.mask_bytes} bytes (> {FCOS_POST_MASK_BYTES_MAX}); "
                             "lower pre_nms_top_n or pass fewer scenes per call")
        self.dims = (ctypes.c_int * self.L)(*self.n)
        assert lib().cdll.nmh_fcos_post_cap(self.L, self.dims, self.N, self.top_n) == self.cap


def fcos_post_select(plan, ncols, cls, reg, ctr, locations, masks, grid_sizes, pre_nms_thresh, min_size):
    """per-level head outputs, locations [n,3], optional per-level masks, grid_sizes int32 [N,3] (required for ncols 6) ->
    (pre_boxes [N,cap,1+6|7], pre_scores [N,cap] (-1: no box in the slot), pre_counts [L,N] int32)"""
    _chk(*cls, *reg, *ctr, *locations, *(masks or ()), grid_sizes)
    dev = cls[0].device
    row = 7 if ncols == 6 else 8
    keys = torch.empty((plan.N * sum(plan.n),), dtype=torch.int32, device=dev)
    pre_boxes = torch.empty((plan.N, plan.cap, row), dtype=torch.float32, device=dev)
    pre_scores = torch.empty((plan.N, plan.cap), dtype=torch.float32, device=dev)
    pre_counts = torch.empty((plan.L, plan.N), dtype=torch.int32, device=dev)
    lib().call("nmh_fcos_post_select", plan.L, plan.dims, plan.N, ncols, plan.top_n, _ptr_table(cls, plan.L), _ptr_table(reg, plan.L), _ptr_table(ctr, plan.L), _ptr_table(locations, plan.L),
               _ptr_table(masks, plan.L) if masks else None, grid_sizes, pre_nms_thresh, min_size, keys, pre_boxes, pre_scores, pre_counts, _st())
    return pre_boxes, pre_scores, pre_counts


def fcos_post_nms(plan, ncols, pre_boxes, sorted_scores, order, pre_counts, nms_thresh, post_nms_top_n):
    """the stable descending sort (sorted_scores, order int64) of pre_scores -> (boxes [N,cap,1+6|7], scores [N,cap], counts [N] int32)"""
    _chk(pre_boxes, sorted_scores, order, pre_counts)
    dev = pre_boxes.device
    mask = torch.empty((plan.N, plan.cap, (plan.cap + 63) // 64), dtype=torch.int64, device=dev)
    keep = torch.empty((plan.N, plan.cap), dtype=torch.int32, device=dev)
    boxes, scores = torch.empty_like(pre_boxes), torch.empty_like(sorted_scores)
    counts = torch.empty((plan.N,), dtype=torch.int32, device=dev)
    lib().call("nmh_fcos_post_nms", plan.L, plan.dims, plan.N, ncols, plan.top_n, pre_boxes, sorted_scores, order, pre_counts, nms_thresh, int(post_nms_top_n), mask, keep,
               boxes, scores, counts, _st())
    return boxes, scores, counts


# ---- RPN anchor target assignment, sampling and training losses (csrc/rpn.hip) ---------------------------------------------------------------
RPN_MAX_ANCHORS = 32


class RpnPlan:
    """grid sizes [(W,H,D)] and per-axis strides [(sx,sy,sz)] of 1..4 levels, the base anchors' half extents per level ([A_k][3] host floats), N scenes ->
    the host-side level table of the rpn entries, the anchors per level and scene (n = sum n_k) and the size of the partial-sum workspace"""

    def __init__(self, grid_sizes, strides, half_extents, N):
        grid_sizes = [tuple(int(v) for v in g) for g in grid_sizes]
        strides = [tuple(int(v) for v in s) for s in strides]
        if not 1 <= len(grid_sizes) <= FCOS_MAX_LEVELS or len(strides) != len(grid_sizes) or len(half_extents) != len(grid_sizes):
            raise ValueError(f"RPN ops take 1 to {FCOS_MAX_LEVELS} levels with strides and base anchors for each, got {len(grid_sizes)} grids, {len(strides)} strides, "
                             f"{len(half_extents)} anchor tables")
        if not 1 <= N <= FCOS_MAX_SCENES:
            raise ValueError(f"RPN ops take 1 to {FCOS_MAX_SCENES} scenes, got {N}")
        self.L, self.N, self.grids, self.strides = len(grid_sizes), int(N), grid_sizes, strides
        self.A = [len(h) for h in half_extents]
        if not all(1 <= a <= RPN_MAX_ANCHORS for a in self.A):
            raise ValueError(f"RPN ops take 1 to {RPN_MAX_ANCHORS} anchors per location, got {self.A}")
        self.nloc = [w * h * d for w, h, d in grid_sizes]
        self.n_level = [n * a for n, a in zip(self.nloc, self.A)]
        self.n = sum(self.n_level)
        self.dims = (ctypes.c_int * (7 * self.L))(*[v for g, s, a in zip(grid_sizes, strides, self.A) for v in (*g, *s, a)])
        flat = [float(v) for h in half_extents for row in h for v in row]
        self.base = (ctypes.c_float * len(flat))(*flat)
        self.nblocks = lib().cdll.nmh_rpn_num_blocks(self.L, self.dims, self.N)
        if self.nblocks <= 0 or min(flat) <= 0:
            raise ValueError(f"RPN ops: unsupported level table {grid_sizes} x {strides} x {self.A} anchors")


def rpn_assign(plan, boxes, offsets, ncols, ori_sizes, fg, bg):
    """boxes [G,6|7] fp32 (may be empty), offsets host ints [N+1], ori_sizes int32 [N,3] or None ->
    (labels [N,n] fp32, matched_idxs [N,n] int32, regression_targets [N,n,6|8] fp32)"""
    _chk(boxes, ori_sizes)
    dev = boxes.device
    C = 6 if ncols == 6 else 8
    labels = torch.empty((plan.N, plan.n), dtype=torch.float32, device=dev)
    midx = torch.empty((plan.N, plan.n), dtype=torch.int32, device=dev)
    targets = torch.empty((plan.N, plan.n, C), dtype=torch.float32, device=dev)
    gtmax = torch.empty((max(offsets[-1], 1),), dtype=torch.int32, device=dev)
    offs = (ctypes.c_int * (plan.N + 1))(*offsets)
    lib().call("nmh_rpn_assign", plan.L, plan.dims, plan.base, plan.N, ncols, boxes if boxes.numel() else None, offs, ori_sizes, fg, bg, gtmax, labels, midx, targets, _st())
    return labels, midx, targets


def rpn_sample(labels, batch, want_pos, rng_state):
    """labels [N,n] fp32, rng_state int64 [2] (seed, counter; the counter advances by one) -> (flags [N,n] uint8, counts [N,2] int32)"""
    _chk(labels, rng_state)
    N, n = labels.shape
    flags = torch.empty((N, n), dtype=torch.uint8, device=labels.device)
    counts = torch.empty((N, 2), dtype=torch.int32, device=labels.device)
    lib().call("nmh_rpn_sample", N, n, labels, batch, want_pos, rng_state, flags, counts, _st())
    return flags, counts


def _cams48(cams):
    """fp32 host tensor [4, 3, 4] -> the host array the entries take"""
    if not isinstance(cams, torch.Tensor) or cams.dtype != torch.float32 or cams.is_cuda or tuple(cams.shape) != (4, 3, 4):
        raise ValueError("cameras must be an fp32 host tensor [4, 3, 4]")
    return (ctypes.c_float * 48)(*cams.reshape(-1).tolist())


def _rpn_loss_entry(plan, C, loss_type, targets, boxes, offsets, ori_sizes, midx, cams, res):
    """-> (the ABI entry's stem, its arguments from base_half up to flags, its arguments between flags and the outputs); of the eight entries the smooth-L1 pair
    without the 2-D term takes neither the base table nor the box rows, and only the IoU types take a loss type"""
    if loss_type is not None and loss_type not in FCOS_LOSS_TYPES:
        raise ValueError(f"RPN IoU loss: reg_loss_type must be one of {sorted(FCOS_LOSS_TYPES)}, got {loss_type!r}")
    _chk(boxes, ori_sizes, midx, targets)
    if loss_type is None and cams is None:
        return "nmh_rpn_loss", (plan.N, C), (targets,)
    offs = (ctypes.c_int * (plan.N + 1))(*offsets)
    rows = (boxes if boxes.numel() else None, offs, ori_sizes, midx) + (() if cams is None else (cams, res))
    if loss_type is None:
        return "nmh_rpn_loss2d", (plan.base, plan.N, C), (targets, *rows)
    return "nmh_rpn_iou_loss" + ("" if cams is None else "2d"), (plan.base, plan.N, C, FCOS_LOSS_TYPES[loss_type]), rows


def rpn_loss_fwd(plan, C, loss_type, obj, reg, flags, targets, boxes, offsets, ori_sizes, midx, cams=None, res=None):
    """loss_type None: the smooth-L1 box loss on targets [N,n,C], C 6 | 8; a key of FCOS_LOSS_TYPES: the IoU-type box loss of the oriented RPN over the decoded proposals,
    C 8.  boxes [G,6|7], offsets host ints [N+1], ori_sizes int32 [N,3] or None, midx [N,n] int32 as rpn_assign takes and returns them (smooth-L1 without the 2-D term
    reads none of them).  cams None -> scalars [3] = (objectness loss, box loss, number of sampled anchors); cams the host array of _cams48 and res = max(mesh_size):
    with the 2-D projection term -> scalars [5] = (objectness loss, box loss, sampled anchors, 2-D loss, sampled positives)"""
    name, head, tail = _rpn_loss_entry(plan, C, loss_type, targets, boxes, offsets, ori_sizes, midx, cams, res)
    ns = 3 if cams is None else 5
    partials = torch.empty((ns * plan.nblocks,), dtype=torch.float32, device=flags.device)
    scalars = torch.empty((ns,), dtype=torch.float32, device=flags.device)
    lib().call(name + "_fwd", plan.L, plan.dims, *head, _ptr_table(obj, plan.L), _ptr_table(reg, plan.L), flags, *tail, partials, scalars, _st())
    return scalars


def rpn_loss_bwd(plan, C, loss_type, obj, reg, flags, targets, boxes, offsets, ori_sizes, midx, cams, res, scalars, g_obj, g_reg, g_2d=None, out=None):
    """-> (dobj, dreg) per level; out: the pair of per-level lists to write instead of fresh tensors (every element is written exactly once)"""
    name, head, tail = _rpn_loss_entry(plan, C, loss_type, targets, boxes, offsets, ori_sizes, midx, cams, res)
    dobj, dreg = out if out is not None else ([torch.empty_like(t) for t in obj], [torch.empty_like(t) for t in reg])
    gs = (g_obj, g_reg) if cams is None else (g_obj, g_reg, g_2d)
    lib().call(name + "_bwd", plan.L, plan.dims, *head, _ptr_table(obj, plan.L), _ptr_table(reg, plan.L), flags, *tail, scalars, *gs, _ptr_table(dobj, plan.L), _ptr_table(dreg, plan.L),
               _st())
    return dobj, dreg


# ---- the 2-D projection term on rows of boxes (csrc/proj2d.hip) ------------------------------------------------------------------------------
def proj2d_fwd(pred, target, cams):
    """pred, target [n, 6|7] fp32, cams: the host array of _cams48 -> terms [n]"""
    _chk(pred, target)
    terms = torch.empty((pred.shape[0],), dtype=torch.float32, device=pred.device)
    lib().call("nmh_proj2d_fwd", pred, target, pred.shape[0], pred.shape[1], cams, terms, _st())
    return terms


def proj2d_bwd(pred, target, g_terms, cams):
    _chk(pred, target, g_terms)
    dpred = torch.empty_like(pred)
    lib().call("nmh_proj2d_bwd", pred, target, g_terms, pred.shape[0], pred.shape[1], cams, dpred, _st())
    return dpred


# ---- RPN proposals: decode, top-k per level, per-level NMS, post-NMS cut (csrc/rpn_post.hip) --------------------------------------------------
class RpnPostPlan:
    """RpnPlan + pre_nms_top_n -> what the selection adds to the level table: t_k = min(pre_nms_top_n, n_k) kept per level, the level's first slot,
    cap = sum t_k and the words of the per-(scene, level) suppression matrices"""

    def __init__(self, plan, pre_nms_top_n):
        self.plan, self.top_n = plan, int(pre_nms_top_n)
        if self.top_n < 1:
            raise ValueError(f"RPN proposals: pre_nms_top_n >= 1, got {self.top_n}")
        self.top = [min(self.top_n, n) for n in plan.n_level]
        self.off = [sum(self.top[:k]) for k in range(plan.L)]
        self.cap = sum(self.top)
        if self.cap > OBB_NMS_MAX:
            raise ValueError(f"RPN proposals keep at most {OBB_NMS_MAX} boxes per scene before NMS, got cap = {self.cap}; lower pre_nms_top_n")
        self.mask_words = plan.N * sum(t * ((t + 63) // 64) for t in self.top)
        if self.mask_words * 8 > FCOS_POST_MASK_BYTES_MAX:
            raise ValueError(f"RPN proposals: the suppression workspace of {plan.N} scenes x cap {self.cap} takes {self.mask_words * 8} bytes (> {FCOS_POST_MASK_BYTES_MAX}); "
                             "lower pre_nms_top_n or pass fewer scenes per call")
        assert lib().cdll.nmh_rpn_post_cap(plan.L, plan.dims, plan.N, self.top_n) == self.cap
        assert lib().cdll.nmh_rpn_post_mask_words(plan.L, plan.dims, plan.N, self.top_n) == self.mask_words


def rpn_decode(plan, ncols, reg):
    """per-level regression (N, A*6|8, W, H, D) -> the unclipped decode of every anchor [N, n, 6|7], anchor order"""
    _chk(*reg)
    boxes = torch.empty((plan.N, plan.n, 6 if ncols == 6 else 7), dtype=torch.float32, device=reg[0].device)
    lib().call("nmh_rpn_decode", plan.L, plan.dims, plan.base, plan.N, ncols, _ptr_table(reg, plan.L), boxes, _st())
    return boxes


def rpn_post_select(post, ncols, obj, reg, ori_sizes, mesh_size, score_thresh, min_size):
    """-> (pre_keys [N,cap] int64, pre_boxes [N,cap,6|7], pre_scores [N,cap], pre_index [N,cap] int32, pre_counts [L,N] int32); slot layout and the sort key:
    the header of csrc/rpn_post.hip"""
    _chk(*obj, *reg, ori_sizes)
    plan, dev = post.plan, obj[0].device
    pre_keys = torch.empty((plan.N, post.cap), dtype=torch.int64, device=dev)
    pre_boxes = torch.empty((plan.N, post.cap, 6 if ncols == 6 else 7), dtype=torch.float32, device=dev)
    pre_scores = torch.empty((plan.N, post.cap), dtype=torch.float32, device=dev)
    pre_index = torch.empty((plan.N, post.cap), dtype=torch.int32, device=dev)
    pre_counts = torch.empty((plan.L, plan.N), dtype=torch.int32, device=dev)
    mesh = (ctypes.c_int * 3)(*[int(v) for v in mesh_size])
    lib().call("nmh_rpn_post_select", plan.L, plan.dims, plan.base, plan.N, ncols, post.top_n, _ptr_table(obj, plan.L), _ptr_table(reg, plan.L), ori_sizes, mesh, score_thresh, min_size,
               pre_keys, pre_boxes, pre_scores, pre_index, pre_counts, _st())
    return pre_keys, pre_boxes, pre_scores, pre_index, pre_counts


def rpn_post_nms(post, ncols, pre_boxes, pre_scores, pre_index, sorted_keys, order, pre_counts, nms_thresh, post_nms_top_n):
    """the stable descending sort (sorted_keys, order int64) of pre_keys -> (boxes [N,cap,6|7], scores [N,cap], levels, anchor index [N,cap] int32, counts [N] int32)"""
    _chk(pre_boxes, pre_scores, pre_index, sorted_keys, order, pre_counts)
    if int(post_nms_top_n) < 1:
        raise ValueError(f"RPN proposals: post_nms_top_n >= 1, got {post_nms_top_n}")
    plan, dev = post.plan, pre_boxes.device
    mask = torch.empty((max(post.mask_words, 1),), dtype=torch.int64, device=dev)
    keep = torch.empty((plan.N, post.cap), dtype=torch.int32, device=dev)
    boxes, scores = torch.empty_like(pre_boxes), torch.empty_like(pre_scores)
    levels, index = torch.empty_like(pre_index), torch.empty_like(pre_index)
    counts = torch.empty((plan.N,), dtype=torch.int32, device=dev)
    lib().call("nmh_rpn_post_nms", plan.L, plan.dims, plan.N, ncols, post.top_n, pre_boxes, pre_scores, pre_index, sorted_keys, order, pre_counts, nms_thresh,
               int(post_nms_top_n), mask, keep, boxes, scores, levels, index, counts, _st())
    return boxes, scores, levels, index, counts


# ---- RPNHead's output stage and the ReLU between its convolutions (csrc/rpn_head.hip) -------------------------------------------------------
def _head_args(name, ts, w_cls, w_box, C):
    """per-level channels-last activations (N,W,H,D,Cin) + the two 1x1x1 weights [A,Cin], [A*C,Cin] -> (level table, N, Cin, A)"""
    if not 1 <= len(ts) <= FCOS_MAX_LEVELS:
        raise ValueError(f"{name} takes 1 to {FCOS_MAX_LEVELS} levels, got {len(ts)}")
    if C not in (6, 8):
        raise ValueError(f"{name}: 6 or 8 regression values per anchor, got {C}")
    _chk(*ts, w_cls, w_box)
    N, Cin = ts[0].shape[0], ts[0].shape[-1]
    A = w_cls.numel() // Cin
    if any(t.dim() != 5 or t.shape[0] != N or t.shape[-1] != Cin or t.dtype != ts[0].dtype for t in ts):
        raise ValueError(f"{name}: every level must be (N, W, H, D, Cin) channels-last of one dtype")
    if Cin % 8:
        raise NotImplementedError(f"{name}: channel counts must be multiples of 8, got {Cin}")
    if w_cls.dtype != ts[0].dtype or w_box.dtype != ts[0].dtype or w_cls.numel() != A * Cin or w_box.numel() != A * C * Cin:
        raise ValueError(f"{name}: weights [A,{Cin}] and [A*{C},{Cin}] in the activations' dtype; got {w_cls.numel()} and {w_box.numel()} elements")
    if not 1 <= A <= RPN_MAX_ANCHORS:
        raise ValueError(f"{name} takes 1 to {RPN_MAX_ANCHORS} anchors per location, got {A}")
    vox = (ctypes.c_int * len(ts))(*[t.shape[1] * t.shape[2] * t.shape[3] for t in ts])
    return vox, N, Cin, A


def rpn_head_out_fwd(ts, w_cls, w_box, b_cls, b_box, C, relu):
    """ts: per level the channels-last activation (N,W,H,D,Cin) in the compute dtype; w_cls [A,Cin], w_box [A*C,Cin] in that dtype; b_cls [A], b_box [A*C] fp32;
    relu: rectify ts as it is read -> (objectness [(N,A,W,H,D)], pred_bbox_deltas [(N,A*C,W,H,D)]) fp32, all levels in one launch"""
    vox, N, Cin, A = _head_args("rpn_head_out_fwd", ts, w_cls, w_box, C)
    _chk(b_cls, b_box)
    dev = ts[0].device
    obj = [torch.empty((N, A, *t.shape[1:4]), dtype=torch.float32, device=dev) for t in ts]
    reg = [torch.empty((N, A * C, *t.shape[1:4]), dtype=torch.float32, device=dev) for t in ts]
    lib().call("nmh_rpn_head_out_fwd", dt_of(ts[0]), len(ts), vox, N, Cin, A, C, int(bool(relu)), _ptr_table(ts), w_cls, w_box, b_cls, b_box, _ptr_table(obj), _ptr_table(reg), _st())
    return obj, reg


def rpn_head_out_bwd(ts, w_cls, w_box, g_obj, g_reg, C, relu, dw_cls, dw_box, db_cls, db_box):
    """the dense fp32 gradients of the two outputs -> per level dt = relu'(t) o (G Wcat), channels-last in the compute dtype; dw_cls, dw_box, db_cls, db_box
    (fp32) += the weight and bias gradients summed over all levels in a fixed order"""
    vox, N, Cin, A = _head_args("rpn_head_out_bwd", ts, w_cls, w_box, C)
    _chk(*g_obj, *g_reg, dw_cls, dw_box, db_cls, db_box)
    if len(g_obj) != len(ts) or len(g_reg) != len(ts):
        raise ValueError("rpn_head_out_bwd: one gradient of each output per level")
    for t, go, gr in zip(ts, g_obj, g_reg):
        if go.dtype != torch.float32 or gr.dtype != torch.float32 or tuple(go.shape) != (N, A, *t.shape[1:4]) or tuple(gr.shape) != (N, A * C, *t.shape[1:4]):
            raise ValueError(f"rpn_head_out_bwd: gradients (N,{A},W,H,D) and (N,{A * C},W,H,D) fp32; got {tuple(go.shape)}, {tuple(gr.shape)}")
    if dw_cls.numel() != A * Cin or dw_box.numel() != A * C * Cin or db_cls.numel() != A or db_box.numel() != A * C or any(
            g.dtype != torch.float32 for g in (dw_cls, dw_box, db_cls, db_box)):
        raise ValueError("rpn_head_out_bwd: fp32 gradient buffers of the shapes of the weights and biases")
    dts = [torch.empty_like(t) for t in ts]
    ws = torch.empty((lib().cdll.nmh_rpn_head_bwd_ws_floats(len(ts), vox, N, Cin, A, C),), dtype=torch.float32, device=ts[0].device)
    lib().call("nmh_rpn_head_out_bwd", dt_of(ts[0]), len(ts), vox, N, Cin, A, C, int(bool(relu)), _ptr_table(ts), w_cls, w_box, _ptr_table(g_obj), _ptr_table(g_reg), _ptr_table(dts), ws,
               dw_cls, dw_box, db_cls, db_box, _st())
    return dts


def relu_(x):
    """x = max(x, 0) in place (channels-last, a multiple of 8 elements)"""
    _chk(x)
    lib().call("nmh_relu_", dt_of(x), x, x.numel(), _st())
    return x


def relu_bwd_(dy, y):
    """dy = 0 where y <= 0, in place"""
    _chk(dy, y)
    if dy.shape != y.shape or dy.dtype != y.dtype:
        raise ValueError("relu_bwd_: dy and y of one shape and dtype")
    lib().call("nmh_relu_bwd_", dt_of(dy), dy, y, dy.numel(), _st())
    return dy


# ---- RCNN, the box head of the two-stage detector: its two Linear layers on the channels-last activation (csrc/box_head.hip) ---------------------------
BOX_HEAD_MAX_COLS = 32         # reg_dim + n_classes
BOX_HEAD_MAX_CELLS = 512       # ow * oh * od
BOX_HEAD_MAX_CHANNELS = 2048
BOX_HEAD_MAX_ROWS = 65535      # RoIs per call
WGRAD_FIXED_ROWS = 16384       # voxels per nmh_conv3d_k3_wgrad_fixed call: its plan never has more splits than the workspace mode takes


def box_head_limits(name, M, S, C, reg, ncls):
    """raises what the C entries would answer with -4"""
    if C % 8 or C < 8:
        raise NotImplementedError(f"{name}: channel counts must be multiples of 8, got {C}")
    if reg not in (6, 7) or ncls < 1 or reg + ncls > BOX_HEAD_MAX_COLS:
        raise ValueError(f"{name}: reg_dim 6 or 7 and reg_dim + n_classes <= {BOX_HEAD_MAX_COLS}, got {reg} + {ncls}")
    if not 1 <= S <= BOX_HEAD_MAX_CELLS:
        raise ValueError(f"{name} supports 1 to {BOX_HEAD_MAX_CELLS} cells per RoI, got {S}")
    if C > BOX_HEAD_MAX_CHANNELS:
        raise ValueError(f"{name} supports at most {BOX_HEAD_MAX_CHANNELS} channels, got {C}")
    if M is not None and not 1 <= M <= BOX_HEAD_MAX_ROWS:
        raise ValueError(f"{name} supports 1 to {BOX_HEAD_MAX_ROWS} RoIs per call, got {M}")


def box_head_pack(w_box, w_cls, C, S, dtype, out=None):
    """w_box [reg, C*S], w_cls [ncls, C*S]: nn.Linear's fp32 weights over the NCDHW-flattened volume (column c*S + s) -> wcat [reg + ncls, S*C] in `dtype`,
    column s*C + c, box rows first: the order of the channels-last activation.  The mean form: S = 1 and dtype float32."""
    _chk(w_box, w_cls, out)
    reg, ncls = w_box.shape[0], w_cls.shape[0]
    box_head_limits("box_head_pack", None, S, C, reg, ncls)
    if w_box.dtype != torch.float32 or w_cls.dtype != torch.float32 or w_box.numel() != reg * C * S or w_cls.numel() != ncls * C * S:
        raise ValueError(f"box_head_pack: fp32 weights [reg, {C * S}] and [n_classes, {C * S}]; got {tuple(w_box.shape)}, {tuple(w_cls.shape)}")
    if out is None:
        out = torch.empty((reg + ncls, S * C), dtype=dtype, device=w_box.device)
    elif out.dtype != dtype or out.numel() != (reg + ncls) * S * C:
        raise ValueError("box_head_pack: out must hold (reg + n_classes) * S * C elements of dtype")
    lib().call("nmh_box_head_pack", dt_of(out), reg, ncls, C, S, w_box, w_cls, out, _st())
    return out


def _box_head_args(name, x, wcat, reg, ncls, flatten):
    _chk(x, wcat)
    if x.dim() != 3:
        raise ValueError(f"{name}: x must be [M, S, C] channels-last per RoI, got {tuple(x.shape)}")
    M, S, C = x.shape
    box_head_limits(name, M, S, C, reg, ncls)
    want = x.dtype if flatten else torch.float32
    if wcat.dtype != want or wcat.numel() != (reg + ncls) * (S * C if flatten else C):
        raise ValueError(f"{name}: wcat must be box_head_pack's [{reg + ncls}, {S * C if flatten else C}] in {want}")
    return M, S, C


def box_head_out_fwd(x, wcat, b_box, b_cls, flatten, relu):
    """x [M, S, C] in the compute dtype; wcat: box_head_pack's matrix; b_box [reg], b_cls [ncls] fp32; relu: rectify x as it is read ->
    (pred_bbox_delta [M, reg], pred_scores [M, ncls]) fp32 and, in the mean form, the fp32 mean [M, C] the backward takes (else None)"""
    reg, ncls = b_box.numel(), b_cls.numel()
    M, S, C = _box_head_args("box_head_out_fwd", x, wcat, reg, ncls, flatten)
    _chk(b_box, b_cls)
    out_box = torch.empty((M, reg), dtype=torch.float32, device=x.device)
    out_cls = torch.empty((M, ncls), dtype=torch.float32, device=x.device)
    xmean = None if flatten else torch.empty((M, C), dtype=torch.float32, device=x.device)
    lib().call("nmh_box_head_out_fwd", dt_of(x), M, S, C, reg, ncls, int(bool(flatten)), int(bool(relu)), x, wcat, b_box, b_cls, xmean, out_box, out_cls, _st())
    return out_box, out_cls, xmean


def box_head_out_bwd(x, wcat, xmean, g_box, g_cls, reg, ncls, flatten, relu, dw_box, dw_cls, db_box, db_cls):
    """g_box [M, reg], g_cls [M, ncls]: the fp32 gradients of the two outputs, either may be None (zeros; its dw / db are then not touched and may be None) ->
    dx [M, S, C] in x's dtype; dw_box, dw_cls (nn.Linear's layout), db_box, db_cls (fp32) += the weight and bias gradients in a fixed order"""
    M, S, C = _box_head_args("box_head_out_bwd", x, wcat, reg, ncls, flatten)
    for g, n, dw, db in ((g_box, reg, dw_box, db_box), (g_cls, ncls, dw_cls, db_cls)):
        if g is None:
            continue
        _chk(g, dw, db)
        if g.dtype != torch.float32 or tuple(g.shape) != (M, n):
            raise ValueError(f"box_head_out_bwd: gradients [M, {reg}] and [M, {ncls}] fp32, got {tuple(g.shape)} {g.dtype}")
        if dw is None or db is None or dw.dtype != torch.float32 or db.dtype != torch.float32 or dw.numel() != n * (S * C if flatten else C) or db.numel() != n:
            raise ValueError("box_head_out_bwd: fp32 gradient buffers of the shapes of the weights and biases")
    if not flatten and (xmean is None or xmean.dtype != torch.float32 or tuple(xmean.shape) != (M, C)):
        raise ValueError("box_head_out_bwd: the mean form takes box_head_out_fwd's xmean [M, C]")
    dx = torch.empty_like(x)
    dxmean = None if flatten else torch.empty((M, C), dtype=torch.float32, device=x.device)
    ws = torch.empty((lib().cdll.nmh_box_head_bwd_ws_floats(M, S, C, reg, ncls, int(bool(flatten))),), dtype=torch.float32, device=x.device)
    lib().call("nmh_box_head_out_bwd", dt_of(x), M, S, C, reg, ncls, int(bool(flatten)), int(bool(relu)), x, wcat, xmean, g_box, g_cls, dx, dxmean, ws,
               dw_box if g_box is not None else None, dw_cls if g_cls is not None else None, db_box if g_box is not None else None, db_cls if g_cls is not None else None, _st())
    return dx


def colsum_fixed(dy, db):
    """db [C] fp32 += the column sums of the channels-last dy (.., C), per-workgroup partials added in workgroup order: a conv's bias gradient whose bits do
    not change between runs (bias_grad adds atomically)"""
    _chk(dy, db)
    C = dy.shape[-1]
    R = dy.numel() // C
    if C % 8 or C > BOX_HEAD_MAX_CHANNELS or db.dtype != torch.float32 or db.numel() != C:
        raise ValueError(f"colsum_fixed: C a multiple of 8, at most {BOX_HEAD_MAX_CHANNELS}, and an fp32 db [C]")
    ws = torch.empty((lib().cdll.nmh_box_head_colsum_ws_floats(R, C),), dtype=torch.float32, device=dy.device)
    lib().call("nmh_box_head_colsum", dt_of(dy), dy, R, C, ws, db, _st())
    return db


def conv3d_k3_wgrad_fixed(dY, X, dW):
    """dW[Cout][Cin][3][3][3] += the weight gradient of the generic kernel with a fixed order of additions: the contraction splits leave partial tiles in a
    workspace and a second launch adds them in split order (conv3d_k3_wgrad adds them atomically).  Batches of more than WGRAD_FIXED_ROWS voxels go in slices of
    the batch index, one call after the other on the stream: still one order."""
    _chk(dY, X, dW)
    B, D, H, W, Cin = X.shape
    Cout = dY.shape[-1]
    V = D * H * W
    if V > WGRAD_FIXED_ROWS:
        raise ValueError(f"conv3d_k3_wgrad_fixed takes volumes of at most {WGRAD_FIXED_ROWS} voxels, got {V}")
    step = max(1, WGRAD_FIXED_ROWS // V)
    for b0 in range(0, B, step):
        n = min(step, B - b0)
        need = lib().cdll.nmh_conv3d_k3_wgrad_fixed_ws_floats(dt_of(X), n * V, Cin, Cout)
        if need < 0:
            raise RuntimeError(f"conv3d_k3_wgrad_fixed: no fixed-order plan for {n * V} voxels, {Cin} -> {Cout} channels")
        ws = torch.empty((need,), dtype=torch.float32, device=X.device) if need else None
        lib().call("nmh_conv3d_k3_wgrad_fixed", dt_of(X), dY[b0:b0 + n], X[b0:b0 + n], dW, ws, need, n, D, H, W, Cin, Cout, _st())
    return dW


# ---- RoI stage of the two-stage detector: proposal targets, pyramid RoI pooling, box-head losses, decode (csrc/roi_head.hip) -----------------------
ROI_MAX_GRID = 1024            # points per axis of one oriented RoI's sampling grid; a larger grid is cut to this
ROI_MAX_CELLS = 4096           # ow * oh * od
ROI_MAX_CLASSES = 1024
ROI_MAX_ROWS = 1 << 24         # proposals (cap) and sampled rows (R) per scene


def roi_targets(boxes, levels, counts, gt, gt_labels, offsets, R, want_fg, fg, bg, is_sample, rng_state=None, keep=None, counts2=None):
    """boxes [N,cap,6|7], levels [N,cap] int32, counts [N] int32, gt [G,6|7] with gt_labels [G] fp32 and host offsets [N+1] ->
    (labels [N,R], rois [N,R,1+6|7], gt_rois [N,R,6|7], keep [N,R] int32, counts2 [N,2] int32 or None, max_iou [N,cap], arg [N,cap] int32).
    Sampling takes rng_state (int64 [2]: seed, counter; the counter advances) or the caller's keep and counts2; evaluation has R = cap."""
    _chk(boxes, levels, counts, gt, gt_labels, rng_state, keep, counts2)
    N, cap, B = boxes.shape
    dev = boxes.device
    miou = torch.empty((N, cap), dtype=torch.float32, device=dev)
    arg = torch.empty((N, cap), dtype=torch.int32, device=dev)
    lists = None
    if is_sample:
        if rng_state is not None:
            lists = torch.empty((N, 2, cap), dtype=torch.int32, device=dev)
            keep = torch.empty((N, R), dtype=torch.int32, device=dev)
            counts2 = torch.empty((N, 2), dtype=torch.int32, device=dev)
        else:
            keep, counts2 = keep.clone(), counts2.contiguous()
    else:
        keep, counts2 = torch.empty((N, R), dtype=torch.int32, device=dev), None
    labels = torch.empty((N, R), dtype=torch.float32, device=dev)
    rois = torch.empty((N, R, 1 + B), dtype=torch.float32, device=dev)
    gt_rois = torch.empty((N, R, B), dtype=torch.float32, device=dev)
    offs = (ctypes.c_int * (N + 1))(*offsets)
    lib().call("nmh_roi_targets", N, cap, B, R, int(bool(is_sample)), boxes, levels, counts, gt if gt.numel() else None, gt_labels if gt_labels.numel() else None, offs, want_fg, fg, bg,
               rng_state, miou, arg, lists, keep, counts2, labels, rois, gt_rois, _st())
    return labels, rois, gt_rois, keep, counts2, miou, arg


def roi_level_map(boxes, ncols, k_min, k_max, canonical_scale, canonical_level, eps):
    """boxes [M, ncols | 1+ncols] fp32 (the box in the last ncols columns) -> levels [M] int32"""
    _chk(boxes)
    out = torch.empty((boxes.shape[0],), dtype=torch.int32, device=boxes.device)
    if boxes.shape[0]:
        lib().call("nmh_roi_level_map", boxes.shape[0], boxes, boxes.shape[1], ncols, k_min, k_max, canonical_scale, canonical_level, eps, out, _st())
    return out


class RoiPoolPlan:
    """the host-side level table of the pooling entries: maps (N, C, W, H, D) per level, their scales, the output size and 1 + enlarge_scale"""

    def __init__(self, maps, scales, output_size, enlarge, ncols):
        self.L, self.N, self.C, self.ncols = len(maps), maps[0].shape[0], maps[0].shape[1], ncols
        self.shapes = [tuple(m.shape) for m in maps]
        self.dims = (ctypes.c_int * (3 * self.L))(*[int(v) for m in maps for v in m.shape[2:]])
        self.scales = (ctypes.c_float * self.L)(*[float(s) for s in scales])
        self.out = tuple(int(v) for v in output_size)
        self.enlarge = float(enlarge)


def roi_pool_fwd(plan, maps, rois, level_override):
    """rois [N,R,1+6|7] -> (out [N*R,C,ow,oh,od], argmax int32 of the same shape)"""
    _chk(*maps, rois, level_override)
    R = rois.shape[1]
    out = torch.empty((plan.N * R, plan.C, *plan.out), dtype=torch.float32, device=rois.device)
    arg = torch.empty(out.shape, dtype=torch.int32, device=rois.device)
    lib().call("nmh_roi_pool_fwd", plan.L, plan.dims, plan.scales, plan.N, plan.C, R, plan.ncols, *plan.out, plan.enlarge, _ptr_table(maps, plan.L), rois, level_override, out, arg, _st())
    return out, arg


def roi_pool_bwd(plan, dout, arg, rois, level_override, need):
    """-> per level the gradient of the map (zeroed here, then accumulated with fp32 atomics), None where need[k] is False"""
    dmaps = [torch.zeros(s, dtype=torch.float32, device=dout.device) if n else None for s, n in zip(plan.shapes, need)]
    lib().call("nmh_roi_pool_bwd", plan.L, plan.dims, plan.scales, plan.N, plan.C, rois.shape[1], plan.ncols, *plan.out, plan.enlarge, dout, arg, rois, level_override,
               _ptr_table(dmaps, plan.L), _st())
    return dmaps


def roi_interp_fwd(plan, maps, rois, level_override):
    """oriented rois [N,R,8] -> out [N*R,C,ow,oh,od]: the RoI's sampling grid resampled as F.interpolate(trilinear, align_corners=True)"""
    _chk(*maps, rois, level_override)
    R = rois.shape[1]
    out = torch.empty((plan.N * R, plan.C, *plan.out), dtype=torch.float32, device=rois.device)
    lib().call("nmh_roi_interp_fwd", plan.L, plan.dims, plan.scales, plan.N, plan.C, R, plan.ncols, *plan.out, plan.enlarge, _ptr_table(maps, plan.L), rois, level_override, out, _st())
    return out


def roi_interp_bwd(plan, dout, rois, level_override, need):
    """-> per level the gradient of the map (zeroed here, then accumulated with fp32 atomics), None where need[k] is False"""
    dmaps = [torch.zeros(s, dtype=torch.float32, device=dout.device) if n else None for s, n in zip(plan.shapes, need)]
    lib().call("nmh_roi_interp_bwd", plan.L, plan.dims, plan.scales, plan.N, plan.C, rois.shape[1], plan.ncols, *plan.out, plan.enlarge, dout, rois, level_override,
               _ptr_table(dmaps, plan.L), _st())
    return dmaps


def roi_loss_fwd(ncols, scores, deltas, labels, rois, gt_rois):
    """-> (scalars [4] = (loss_objectness, loss_rpn_box_reg, valid rows, positive rows), targets [M,ncols])"""
    _chk(scores, deltas, labels, rois, gt_rois)
    M, dev = scores.shape[0], scores.device
    nb = lib().cdll.nmh_roi_loss_blocks(M)
    partials = torch.empty((4 * nb,), dtype=torch.float32, device=dev)
    scalars = torch.empty((4,), dtype=torch.float32, device=dev)
    targets = torch.empty((M, ncols), dtype=torch.float32, device=dev)
    lib().call("nmh_roi_loss_fwd", M, scores.shape[1], ncols, scores, deltas, labels, rois, rois.shape[-1], gt_rois, targets, partials, scalars, _st())
    return scalars, targets


def roi_loss_bwd(ncols, scores, deltas, labels, targets, scalars, g_obj, g_reg):
    dscores, ddeltas = torch.empty_like(scores), torch.empty_like(deltas)
    lib().call("nmh_roi_loss_bwd", scores.shape[0], scores.shape[1], ncols, scores, deltas, labels, targets, scalars, g_obj, g_reg, dscores, ddeltas, _st())
    return dscores, ddeltas


def roi_decode(ncols, deltas, rois):
    """deltas [M,ncols], rois [M, ncols | 1+ncols] -> boxes [M,ncols]"""
    _chk(deltas, rois)
    out = torch.empty_like(deltas)
    if deltas.shape[0]:
        lib().call("nmh_roi_decode", deltas.shape[0], ncols, deltas, rois, rois.shape[-1], out, _st())
    return out


# ---- RoI post-processing: softmax, decode, clip, size and score filters, NMS per scene (csrc/roi_post.hip) ----------------------------------------
ROI_POST_MAX_ROWS = OBB_NMS_MAX            # rows per scene: the walk's removed-set is 256 words of LDS
ROI_POST_MASK_BYTES_MAX = 1 << 30         # the suppression workspace N R ceil(R / 64) 8 of one call
ROI_POST_MODES = {"any": 0, "object": 1}


def roi_post_select(N, R, ncols, pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes, score_thresh, min_size, is_reg, threshold_mode):
    """pred_scores [N*R,K] logits, pred_bbox_deltas [N*R,ncols] (None without is_reg), rois [N*R,1+ncols], counts [N] int32, mesh_sizes [N,3] int32 ->
    (cand_boxes [N,R,ncols], cand_scores [N,R], keys [N,R] int32: 0 dropped, else the bits of the score plus 1)"""
    _chk(pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes)
    dev = pred_scores.device
    cand_boxes = torch.empty((N, R, ncols), dtype=torch.float32, device=dev)
    cand_scores = torch.empty((N, R), dtype=torch.float32, device=dev)
    keys = torch.empty((N, R), dtype=torch.int32, device=dev)
    lib().call("nmh_roi_post_select", N, R, pred_scores.shape[1], ncols, pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes, score_thresh, min_size, int(bool(is_reg)),
               int(threshold_mode), cand_boxes, cand_scores, keys, _st())
    return cand_boxes, cand_scores, keys


def roi_post_nms(ncols, cand_boxes, cand_scores, sorted_keys, order, nms_thresh):
    """the stable descending sort (sorted_keys int32, order int64) of the keys -> (boxes [N,R,ncols], scores [N,R], index [N,R] int32, counts [N] int32)"""
    _chk(cand_boxes, cand_scores, sorted_keys, order)
    N, R = cand_scores.shape
    dev = cand_boxes.device
    mask = torch.empty((N, R, (R + 63) // 64), dtype=torch.int64, device=dev)
    keep = torch.empty((N, R), dtype=torch.int32, device=dev)
    boxes, scores = torch.empty_like(cand_boxes), torch.empty_like(cand_scores)
    index = torch.empty((N, R), dtype=torch.int32, device=dev)
    counts = torch.empty((N,), dtype=torch.int32, device=dev)
    lib().call("nmh_roi_post_nms", N, R, ncols, cand_boxes, cand_scores, sorted_keys, order, nms_thresh, mask, keep, boxes, scores, index, counts, _st())
    return boxes, scores, index, counts


# ---- FCOSHead between its tower convolutions: GroupNorm + ReLU and the three 3x3x3 output convs (csrc/fcos_head.hip) ------------------------------
FCOS_HEAD_MAX_LEVELS = 5           # the reference's FCOSHead has five Scale parameters
FCOS_HEAD_MAX_JOBS = 2 * FCOS_HEAD_MAX_LEVELS
FCOS_HEAD_MODES = {"train": 0, "eval": 1, "exp": 2}


def _gn_args(name, xs, towers, G, others=()):
    """xs: the channels-last tensors (N,W,L,H,C) of up to 10 (level, tower) jobs; towers: 0 | 1 per job -> (vox, tower table, N, C)"""
    if not 1 <= len(xs) <= FCOS_HEAD_MAX_JOBS:
        raise ValueError(f"{name} takes 1 to {FCOS_HEAD_MAX_JOBS} tensors, got {len(xs)}")
    _chk(*xs, *[t for o in others for t in o])
    N, C = xs[0].shape[0], xs[0].shape[-1]
    if any(t.dim() != 5 or t.shape[0] != N or t.shape[-1] != C or t.dtype != xs[0].dtype for t in xs):
        raise ValueError(f"{name}: every tensor must be (N, W, L, H, C) channels-last of one dtype")
    for o in others:
        if len(o) != len(xs) or any(a.shape != b.shape or a.dtype != b.dtype for a, b in zip(o, xs)):
            raise ValueError(f"{name}: the tensor lists must agree in shape and dtype")
    if C % 32 or C > 2048:
        raise NotImplementedError(f"{name}: channel counts must be multiples of 32 up to 2048, got {C}")
    if G < 1 or C % G or not (C // G in (1, 2, 4) or (C // G) % 8 == 0):
        raise NotImplementedError(f"{name}: {C} channels in {G} groups: channels per group must be 1, 2, 4 or a multiple of 8")
    if towers is not None and (len(towers) != len(xs) or any(t not in (0, 1) for t in towers)):
        raise ValueError(f"{name}: one tower index 0 | 1 per tensor")
    vox = (ctypes.c_int * len(xs))(*[t.shape[1] * t.shape[2] * t.shape[3] for t in xs])
    tw = None if towers is None else (ctypes.c_int * len(xs))(*[int(t) for t in towers])
    return vox, tw, N, C


def _gn_ws(vox, n, N, C, device):
    return torch.empty((lib().cdll.nmh_fcos_gn_ws_doubles(n, vox, N, C),), dtype=torch.float64, device=device)


def fcos_gn_stats(xs, G, eps=1e-5):
    """nn.GroupNorm(G, C)'s statistics of every tensor in one launch -> stats [len(xs), N, G, 2] fp32 = {mean, rstd} (fp64 sums in a fixed order)"""
    vox, _, N, C = _gn_args("fcos_gn_stats", xs, None, G)
    stats = torch.empty((len(xs), N, G, 2), dtype=torch.float32, device=xs[0].device)
    lib().call("nmh_fcos_gn_stats", dt_of(xs[0]), len(xs), vox, N, C, G, eps, _ptr_table(xs), _gn_ws(vox, len(xs), N, C, xs[0].device), stats, _st())
    return stats


def fcos_gn_apply(xs, towers, stats, gammas, betas, G):
    """y = relu(gamma_c (x - mean) rstd + beta_c) of every tensor in one launch, in the tensors' dtype; gammas, betas: the (cls_tower, bbox_tower) fp32 pairs
    (an unused tower's entry may be None)"""
    vox, tw, N, C = _gn_args("fcos_gn_apply", xs, towers, G)
    _chk(stats, *gammas, *betas)
    if stats.dtype != torch.float32 or stats.numel() != len(xs) * N * G * 2 or len(gammas) != 2 or len(betas) != 2:
        raise ValueError("fcos_gn_apply: stats [jobs, N, G, 2] fp32 and one (gamma, beta) per tower")
    for t in set(towers):
        if gammas[t] is None or betas[t] is None or gammas[t].dtype != torch.float32 or betas[t].dtype != torch.float32 or gammas[t].numel() != C or betas[t].numel() != C:
            raise ValueError(f"fcos_gn_apply: tower {t} needs fp32 gamma and beta of {C} elements")
    ys = [torch.empty_like(x) for x in xs]
    lib().call("nmh_fcos_gn_apply", dt_of(xs[0]), len(xs), vox, tw, N, C, G, _ptr_table(xs), stats, _ptr_table(gammas), _ptr_table(betas), _ptr_table(ys), _st())
    return ys


def fcos_gn_bwd(dys, xs, ys, towers, stats, gammas, dgammas, dbetas, G):
    """the backward of GroupNorm + ReLU for every tensor: -> dxs in the tensors' dtype; dgammas[t], dbetas[t] (fp32) += the parameter gradients over all the
    tensors of tower t, in a fixed order"""
    vox, tw, N, C = _gn_args("fcos_gn_bwd", xs, towers, G, (dys, ys))
    _chk(stats, *gammas, *dgammas, *dbetas)
    if stats.dtype != torch.float32 or stats.numel() != len(xs) * N * G * 2:
        raise ValueError("fcos_gn_bwd: stats [jobs, N, G, 2] fp32")
    for t in set(towers):
        for p in (gammas[t], dgammas[t], dbetas[t]):
            if p is None or p.dtype != torch.float32 or p.numel() != C:
                raise ValueError(f"fcos_gn_bwd: tower {t} needs fp32 gamma, dgamma and dbeta of {C} elements")
    dev = xs[0].device
    sums = torch.empty((len(xs), N, G, 2), dtype=torch.float32, device=dev)
    dxs = [torch.empty_like(x) for x in xs]
    lib().call("nmh_fcos_gn_bwd", dt_of(xs[0]), len(xs), vox, tw, N, C, G, _ptr_table(dys), _ptr_table(xs), _ptr_table(ys), stats, _ptr_table(gammas),
               _gn_ws(vox, len(xs), N, C, dev), sums, _ptr_table(dgammas), _ptr_table(dbetas), _ptr_table(dxs), _st())
    return dxs


def _fcos_out_args(name, acts, nreg, mode):
    """acts: per level the (cls tower, bbox tower) pair of channels-last activations -> (L, dims, N, C, flat job list)"""
    L = len(acts)
    if not 1 <= L <= FCOS_HEAD_MAX_LEVELS:
        raise ValueError(f"{name} takes 1 to {FCOS_HEAD_MAX_LEVELS} levels, got {L}")
    if nreg not in (6, 8):
        raise ValueError(f"{name}: 6 or 8 regression columns, got {nreg}")
    if mode not in FCOS_HEAD_MODES:
        raise ValueError(f"{name}: mode is one of {sorted(FCOS_HEAD_MODES)}, got {mode!r}")
    flat = [t for pair in acts for t in pair]
    _chk(*flat)
    N, C = flat[0].shape[0], flat[0].shape[-1]
    if any(len(pair) != 2 or pair[0].shape != pair[1].shape for pair in acts) or any(t.dim() != 5 or t.shape[0] != N or t.shape[-1] != C or t.dtype != flat[0].dtype for t in flat):
        raise ValueError(f"{name}: per level two (N, W, L, H, C) channels-last activations of one dtype")
    if C % 32 or C > 2048:
        raise NotImplementedError(f"{name}: channel counts must be multiples of 32 up to 2048, got {C}")
    dims = (ctypes.c_int * (3 * L))(*[int(v) for pair in acts for v in pair[0].shape[1:4]])
    return L, dims, N, C, flat


def fcos_head_out_fwd(acts, w16, b_cls, b_box, b_ctr, scales, strides, nreg, ctr_on_reg, mode):
    """acts: per level (cls tower, bbox tower) channels-last activations (N,W,L,H,C); w16: the two towers' packed weights [16][27][C] in the activations' dtype
    (csrc/fcos_head.hip: tower columns); b_*: fp32 biases; scales: per level the fp32 Scale parameter [1]; mode "train" | "eval" | "exp" ->
    (cls [(N,1,W,L,H)], reg [(N,nreg,W,L,H)], ctr [(N,1,W,L,H)], u [(N,nreg,W,L,H)]) fp32, u = bbox_pred + bias before the Scale; one launch"""
    L, dims, N, C, flat = _fcos_out_args("fcos_head_out_fwd", acts, nreg, mode)
    _chk(*w16, b_cls, b_box, b_ctr, *scales)
    if len(w16) != 2 or any(w.dtype != flat[0].dtype or w.numel() != 16 * 27 * C for w in w16):
        raise ValueError(f"fcos_head_out_fwd: two packed weights of 16 x 27 x {C} elements in the activations' dtype")
    if len(scales) != L or len(strides) != L or any(s.dtype != torch.float32 or s.numel() != 1 for s in scales):
        raise ValueError("fcos_head_out_fwd: one fp32 Scale parameter and one stride per level")
    if any(b.dtype != torch.float32 for b in (b_cls, b_box, b_ctr)) or b_cls.numel() != 1 or b_box.numel() != nreg or b_ctr.numel() != 1:
        raise ValueError(f"fcos_head_out_fwd: fp32 biases of 1, {nreg} and 1 elements")
    dev = flat[0].device
    shp = [tuple(pair[0].shape[1:4]) for pair in acts]
    cls = [torch.empty((N, 1, *s), dtype=torch.float32, device=dev) for s in shp]
    reg = [torch.empty((N, nreg, *s), dtype=torch.float32, device=dev) for s in shp]
    ctr = [torch.empty((N, 1, *s), dtype=torch.float32, device=dev) for s in shp]
    u = [torch.empty((N, nreg, *s), dtype=torch.float32, device=dev) for s in shp]
    st = (ctypes.c_float * L)(*[float(s) for s in strides])
    lib().call("nmh_fcos_head_out_fwd", dt_of(flat[0]), L, dims, st, N, C, nreg, int(bool(ctr_on_reg)), FCOS_HEAD_MODES[mode], _ptr_table(flat), _ptr_table(w16), b_cls, b_box, b_ctr,
               _ptr_table(scales), _ptr_table(cls), _ptr_table(reg), _ptr_table(ctr), _ptr_table(u), _st())
    return cls, reg, ctr, u


def fcos_head_out_bwd(acts, g_cls, g_reg, g_ctr, u, scales, strides, nreg, ctr_on_reg, mode, db_cls, db_box, db_ctr, dscales):
    """the dense fp32 gradients of the three outputs through the epilogue -> g16: per level the (cls tower, bbox tower) pair of 16-column gradients (N,W,L,H,16)
    in the activations' dtype, the operand of the input-gradient convolution, and gt: the same as fp32 planes (N,16,W,L,H), the operand of
    fcos_head_out_wgrad; db_* (fp32) and dscales[l] += the bias and Scale gradients over all levels in a fixed order -> (g16, gt)"""
    L, dims, N, C, flat = _fcos_out_args("fcos_head_out_bwd", acts, nreg, mode)
    _chk(*g_cls, *g_reg, *g_ctr, *u, *scales, db_cls, db_box, db_ctr, *dscales)
    if any(len(t) != L for t in (g_cls, g_reg, g_ctr, u, scales, strides, dscales)):
        raise ValueError("fcos_head_out_bwd: one gradient of each output, one saved u, one Scale and its gradient per level")
    for pair, gc, gr, gk, uu in zip(acts, g_cls, g_reg, g_ctr, u):
        s = tuple(pair[0].shape[1:4])
        if any(t.dtype != torch.float32 for t in (gc, gr, gk, uu)) or tuple(gc.shape) != (N, 1, *s) or tuple(gk.shape) != (N, 1, *s) or tuple(gr.shape) != (N, nreg, *s) or uu.shape != gr.shape:
            raise ValueError(f"fcos_head_out_bwd: fp32 gradients (N,1,W,L,H), (N,{nreg},W,L,H), (N,1,W,L,H) per level")
    if any(t.dtype != torch.float32 for t in (db_cls, db_box, db_ctr, *scales, *dscales)) or db_cls.numel() != 1 or db_ctr.numel() != 1 or db_box.numel() != nreg or \
            any(s.numel() != 1 for s in (*scales, *dscales)):
        raise ValueError("fcos_head_out_bwd: fp32 gradient buffers of the shapes of the biases and the Scale parameters")
    dev, dtype = flat[0].device, flat[0].dtype
    g16 = [torch.empty((*t.shape[:4], 16), dtype=dtype, device=dev) for t in flat]
    gt = [torch.empty((N, 16, *t.shape[1:4]), dtype=torch.float32, device=dev) for t in flat]
    st = (ctypes.c_float * L)(*[float(s) for s in strides])
    ws = torch.empty((lib().cdll.nmh_fcos_head_pack_ws_floats(L, dims, N),), dtype=torch.float32, device=dev)
    lib().call("nmh_fcos_head_out_bwd_pack", dt_of(flat[0]), L, dims, st, N, nreg, int(bool(ctr_on_reg)), FCOS_HEAD_MODES[mode], _ptr_table(g_cls), _ptr_table(g_reg), _ptr_table(g_ctr),
               _ptr_table(u), _ptr_table(scales), _ptr_table(g16), _ptr_table(gt), ws, db_cls, db_box, db_ctr, _ptr_table(dscales), _st())
    return [(g16[2 * l], g16[2 * l + 1]) for l in range(L)], [(gt[2 * l], gt[2 * l + 1]) for l in range(L)]


def fcos_head_out_wgrad(acts, gt, nreg, ctr_on_reg, dw_cls, dw_box, dw_ctr):
    """gt: fcos_head_out_bwd's fp32 planes -> dw_cls [1,C,3,3,3], dw_box [nreg,C,3,3,3], dw_ctr [1,C,3,3,3] (fp32) += the weight gradients over all levels, per-workgroup
    partials summed in a fixed order; returns the workspace, which the caller keeps alive when the call runs on a side stream"""
    L, dims, N, C, flat = _fcos_out_args("fcos_head_out_wgrad", acts, nreg, "train")
    gflat = [t for pair in gt for t in pair]
    _chk(*gflat, dw_cls, dw_box, dw_ctr)
    if len(gflat) != len(flat) or any(g.dtype != torch.float32 or tuple(g.shape) != (N, 16, *t.shape[1:4]) for g, t in zip(gflat, flat)):
        raise ValueError("fcos_head_out_wgrad: per level two fp32 gradient planes (N, 16, W, L, H)")
    if any(t.dtype != torch.float32 for t in (dw_cls, dw_box, dw_ctr)) or dw_cls.numel() != 27 * C or dw_ctr.numel() != 27 * C or dw_box.numel() != nreg * 27 * C:
        raise ValueError("fcos_head_out_wgrad: fp32 gradient buffers of the shapes of the weights")
    ws = torch.empty((lib().cdll.nmh_fcos_head_wgrad_ws_floats(L, dims, N, C),), dtype=torch.float32, device=flat[0].device)
    lib().call("nmh_fcos_head_out_wgrad", dt_of(flat[0]), L, dims, N, C, nreg, int(bool(ctr_on_reg)), _ptr_table(flat), _ptr_table(gflat), ws, dw_cls, dw_box, dw_ctr, _st())
    return ws


# ---- detection evaluation: IoU and row best, greedy recall matching, AP claims, precision / recall scan (csrc/det_eval.hip) ----------------------
DET_EVAL_MAX_GT, DET_EVAL_MAX_LIMITS, DET_EVAL_MAX_THRESH = 1024, 8, 8


def det_eval_match(boxes, counts, gt, gt_counts, limits, thresholds, top_k, col_offset=0):
    """boxes [N,cap,col_offset+6|7+..] rows in descending score, counts [N] int32, gt [N,Gmax,6|7] padded, gt_counts [N] int32; limits: ints (negative: no cut),
    thresholds: floats, top_k <= 0: no cut -> (gt_overlaps [N,L,Gmax], counted [N,L] int32, best_iou [N,cap], best_gt [N,cap] int32, tp_mask [N,cap] uint8,
    kept [N,cap] uint8).  Three launches, nothing but the outputs and the IoU workspace is allocated, and the host does not wait."""
    _chk(boxes, counts, gt, gt_counts)
    N, cap, stride = boxes.shape
    Gmax, ncols = gt.shape[1], gt.shape[2]
    if any(t.dtype != torch.float32 for t in (boxes, gt)) or any(t.dtype != torch.int32 for t in (counts, gt_counts)) or gt.shape[0] != N or counts.numel() != N or gt_counts.numel() != N:
        raise RuntimeError("det_eval_match: fp32 boxes [N,cap,C] and gt [N,Gmax,6|7], int32 counts [N] and gt_counts [N]")
    L, T, dev = len(limits), len(thresholds), boxes.device
    new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=dev)   # noqa: E731
    iouT = new((N, Gmax, cap), torch.float32)
    gt_overlaps, counted = new((N, L, Gmax), torch.float32), new((N, L), torch.int32)
    best_iou, best_gt = new((N, cap), torch.float32), new((N, cap), torch.int32)
    tp_mask, kept = new((N, cap), torch.uint8), new((N, cap), torch.uint8)
    lim = (ctypes.c_int * L)(*[int(v) for v in limits])
    thr = (ctypes.c_float * T)(*[float(v) for v in thresholds])
    lib().call("nmh_det_eval_iou", ncols, N, cap, stride, col_offset, boxes, counts, Gmax, gt, gt_counts, iouT, best_iou, best_gt, _st())
    lib().call("nmh_det_eval_match", N, cap, Gmax, counts, gt_counts, iouT, L, lim, gt_overlaps, counted, _st())
    lib().call("nmh_det_eval_claims", N, cap, Gmax, counts, best_iou, best_gt, T, thr, int(top_k), tp_mask, kept, _st())
    return gt_overlaps, counted, best_iou, best_gt, tp_mask, kept


def det_eval_pr(bits, n_det, num_gt, nthresh):
    """bits [M] uint8 (the true-positive byte-masks in the global descending-score order, kept detections first), n_det, num_gt int32 [1] on the device ->
    (tp_cum, fp_cum [T,M] int32, recalls, precisions [T,M] fp32, ap [T] fp64); ap is 0 for M == 0"""
    _chk(bits, n_det, num_gt)
    if bits.dtype != torch.uint8 or n_det.dtype != torch.int32 or num_gt.dtype != torch.int32:
        raise RuntimeError("det_eval_pr: uint8 bits, int32 n_det and num_gt")
    M, dev = bits.numel(), bits.device
    tp_cum, fp_cum = (torch.empty((nthresh, M), dtype=torch.int32, device=dev) for _ in range(2))
    recalls, precisions = (torch.empty((nthresh, M), dtype=torch.float32, device=dev) for _ in range(2))
    ap = torch.zeros((nthresh,), dtype=torch.float64, device=dev)
    lib().call("nmh_det_eval_pr", M, bits, n_det, num_gt, nthresh, tp_cum, fp_cum, recalls, precisions, ap, _st())
    return tp_cum, fp_cum, recalls, precisions, ap
