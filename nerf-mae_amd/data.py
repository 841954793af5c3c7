"""Input pipeline of the MAE pretraining path: stored scenes -> padded device batch.

The reference loads `.npz['rgbsigma']` (W,L,H,4) on the host, applies density->alpha, transposes to (4,W,L,H), augments with
90-degree rotations / flips and pads to (4,R,R,R) in PyTorch on the CPU, then ships 65.5 MB of fp32 (plus an equally large
ones-mask) per grid to the GPU (nerf_rpn/datasets.py:88-101,198-233,247-248; torch_utils.py:56-90).  Here the scene crosses PCIe as
stored (uint8 scenes: 16 MB instead of 131 MB) through a pinned staging buffer and ONE HIP kernel (`nmh_grid_prepare`) does
normalisation, density->alpha, layout change, augmentation and zero padding straight into the batch tensor; the ones-mask is
replaced by three integers per sample (the valid extents).  No arithmetic of the path runs on the CPU.
"""
import random as _random
from typing import List, Optional, Sequence, Tuple, Union

import os

import numpy as np
import torch

from . import ops

Scene = Union[np.ndarray, torch.Tensor]


def load_scene(path: str) -> np.ndarray:
    """`rgbsigma` of one stored scene, (W,L,H,4) float32 or uint8, untouched (data/scannet/run_nerf.py:1904-1913 schema)."""
    with np.load(path) as f:
        return np.ascontiguousarray(f["rgbsigma"])


def _check_probs(flip_prob: float, rotate_prob: float):
    if not (0.0 <= flip_prob <= 1.0):
        raise ValueError("flip_prob must be between 0 and 1, but got {}".format(flip_prob))
    if not (0.0 <= rotate_prob <= 1.0):
        raise ValueError("rotate_prob must be between 0 and 1, but got {}".format(rotate_prob))


def draw_augmentation(flip_prob: float, rotate_prob: float, rng=_random) -> int:
    """flags for `ops.grid_prepare`, drawn in the reference's order (datasets.py:198-233 with boxes=None, z_up=True):
    one draw for the rotation, then one per flip axis"""
    _check_probs(flip_prob, rotate_prob)
    flags = 0
    if rng.random() < rotate_prob:
        flags |= ops.GRID_ROT
    if rng.random() < flip_prob:
        flags |= ops.GRID_FLIP0
    if rng.random() < flip_prob:
        flags |= ops.GRID_FLIP1
    return flags


def draw_detection_augmentation(flip_prob: float, rotate_prob: float, rot_scale_prob: float, oriented: bool, rng=_random) -> Tuple[int, float, float]:
    """(flags, angle, scale) of one scene of the detection path, drawn in the reference's order (datasets.py:181-244, z_up=True): rotation, flip 0,
    flip 1; then, for oriented (7-column) boxes only, one draw against `rot_scale_prob` and, if it is taken, uniform(-pi/18, pi/18) and uniform(0.9, 1.1).
    Axis-aligned boxes make exactly three draws.  (0.0, 1.0) means that rot-scale was not taken: the scene goes through `ops.grid_prepare`"""
    _check_probs(flip_prob, rotate_prob)
    if not (0.0 <= rot_scale_prob <= 1.0):
        raise ValueError(f"rotate_and_scale_prob must be between 0 and 1, but got {rot_scale_prob}")
    flags = draw_augmentation(flip_prob, rotate_prob, rng)
    angle, scale = 0.0, 1.0
    if oriented and rng.random() < rot_scale_prob:
        angle = rng.uniform(-np.pi / 18, np.pi / 18)
        scale = rng.uniform(0.9, 1.1)
    return flags, angle, scale


def synthetic_scene(shape: Sequence[int] = (160, 160, 160), seed: int = 0, dtype=np.float32) -> np.ndarray:
    """A stored-format synthetic scene (W,L,H,4) following SURVEY 8(d): RGB ~ U[0,1); raw density sigma ~ N(0,3^2) inside the
    central 60 % box and -10 outside (float32), so that density->alpha gives a realistic occupied fraction; uint8: RGB and an
    already-normalised alpha, scaled to 0..255."""
    rng = np.random.default_rng(seed)
    W, L, H = shape
    g = np.empty((W, L, H, 4), dtype=np.float32)
    g[..., :3] = rng.random((W, L, H, 3), dtype=np.float32)
    sigma = np.full((W, L, H), -10.0, dtype=np.float32)
    lo, hi = [int(0.2 * s) for s in shape], [int(0.8 * s) for s in shape]
    sigma[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] = rng.standard_normal((hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]), dtype=np.float32) * 3.0
    if dtype == np.uint8:
        alpha = np.clip(1.0 - np.exp(-np.exp(sigma) / 100.0), 0.0, 1.0)
        g[..., 3] = alpha
        return np.round(g * 255.0).astype(np.uint8)
    g[..., 3] = sigma
    return g


def _wait_event(ev):
    """host-side wait by polling: a blocking hipEventSynchronize from the producer thread was measured to stall the kernel / graph
    launches of the training thread for the whole wait (runtime-internal locking), tripling the step time"""
    import time
    while not ev.query():
        time.sleep(2e-4)


class _PinnedSlot:
    """ring of pinned host buffers + device staging buffers for one slot of the batch; a buffer is rewritten only after the event
    recorded behind its previous H2D copy + grid_prepare launch has completed (the host may run several steps ahead of the device)"""

    def __init__(self, depth: int, device):
        self.depth, self.device = depth, device
        self.pin, self.dev, self.ev, self.i = [None] * depth, [None] * depth, [None] * depth, 0

    def acquire(self, numel: int, dtype):
        k = self.i % self.depth
        self.i += 1
        if self.ev[k] is not None:
            _wait_event(self.ev[k])
            self.ev[k] = None
        if self.pin[k] is None or self.pin[k].numel() < numel or self.pin[k].dtype != dtype:
            self.pin[k] = torch.empty(numel, dtype=dtype).pin_memory()
            self.dev[k] = torch.empty(numel, dtype=dtype, device=self.device)
        return k, self.pin[k][:numel], self.dev[k][:numel]

    def release_after(self, k: int, stream):
        ev = torch.cuda.Event()
        ev.record(stream)
        self.ev[k] = ev


class GridBatcher:
    """Turns a list of stored scenes into the network input `(xb (B,4,R,R,R) fp32, extents (B,3) int32)` on `device`.

    Host side: a ring of `depth` pinned staging buffers per slot of the batch, each guarded by an event (see _PinnedSlot), so a
    caller that runs ahead of the device never overwrites a buffer whose H2D copy has not executed yet.  Device side:
    `ops.grid_prepare` per scene on the current stream.  `normalize_density` applies to float scenes (uint8 scenes are stored with
    alpha already normalised, as the reference's /255 branch assumes).  `Prefetcher` runs this on a background thread + copy stream."""

    def __init__(self, resolution: int, device, normalize_density: bool = True, flip_prob: float = 0.0, rotate_prob: float = 0.0, depth: int = 3):
        self.R, self.device = resolution, torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("GridBatcher needs a HIP device (no CPU fallback)")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.normalize_density, self.flip_prob, self.rotate_prob, self.depth = normalize_density, flip_prob, rotate_prob, depth
        self._slots = {}

    _pool = None

    @classmethod
    def _copy_pool(cls):
        # host -> pinned copies of one batch run on a few worker threads (the copy releases the GIL; one thread moves a 66 MB fp32 scene
        # at 5-7 GB/s: 36 ms per batch of 4, more than the 33 ms training step it has to hide under)
        if cls._pool is None:
            from concurrent.futures import ThreadPoolExecutor
            cls._pool = ThreadPoolExecutor(max_workers=int(os.environ.get("NMH_STAGE_THREADS", "8")), thread_name_prefix="nmh-stage")
        return cls._pool

    def _stage_begin(self, slot: int, scene: Scene, slots=None):
        """-> (host tensor, ring index, pinned buffer, device buffer, host-copy futures); a scene that is already on the device comes back as
        (scene, None, None, None, [])"""
        if isinstance(scene, torch.Tensor) and scene.is_cuda:
            return scene.contiguous(), None, None, None, []
        t = torch.from_numpy(scene) if isinstance(scene, np.ndarray) else scene
        t = t.contiguous()
        slots = self._slots if slots is None else slots     # (a subclass stages a second tensor per sample through rings of its own)
        sl = slots.get(slot)
        if sl is None:
            sl = slots[slot] = _PinnedSlot(self.depth, self.device)
        k, pin, dev = sl.acquire(t.numel(), t.dtype)
        futs = []
        if not t.is_pinned():
            flat, n = t.reshape(-1), t.numel()
            nchunk = max(1, min(4, n * t.element_size() // (8 << 20)))     # >= 8 MB per task
            step = (n + nchunk - 1) // nchunk
            pool = self._copy_pool()
            for a in range(0, n, step):
                futs.append(pool.submit(pin[a:a + step].copy_, flat[a:a + step]))
        return t, k, pin, dev, futs

    @staticmethod
    def _stage_end(t, k, pin, dev, futs):
        if k is None:
            return t
        for f in futs:
            f.result()
        # (already page-locked scenes -- data.pin_scene -- are read in place: no host-side copy)
        dev.copy_(t.reshape(-1) if t.is_pinned() else pin, non_blocking=True)
        return dev.view(t.shape)

    def _stage(self, slot: int, scene: Scene):
        """-> (device tensor holding the stored scene, ring index or None)"""
        st = self._stage_begin(slot, scene)
        return self._stage_end(*st), st[1]

    def _batch_out(self, out: Optional[torch.Tensor], shape, name: str = "out") -> torch.Tensor:
        """the output batch: a new one, or the caller's after a check of what the kernels rely on"""
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.device)
        if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"{type(self).__name__}: {name} must be a contiguous float32 {tuple(shape)}")
        return out

    def _prepare_slot(self, i: int, staged, dst: torch.Tensor, R: int, flags: int, angle: float = 0.0, scale: float = 1.0, slots=None):
        """the per-scene sequence for slot i of the batch: finish the staging that `_stage_begin` started (-> the H2D copy), the density flag for a float
        scene under normalize_density, `ops.grid_prepare` -- `ops.grid_prepare_rs` for an (angle, scale) other than (0.0, 1.0) -- into `dst`, and the release
        of the ring buffer behind that launch -> the valid extents"""
        src, k = self._stage_end(*staged), staged[1]
        if self.normalize_density and src.dtype == torch.float32:
            flags |= ops.GRID_DENSITY
        e = ops.grid_prepare(src, dst, R, flags) if (angle, scale) == (0.0, 1.0) else ops.grid_prepare_rs(src, dst, R, flags, angle, scale)
        if k is not None:
            (self._slots if slots is None else slots)[i].release_after(k, torch.cuda.current_stream())
        return e

    def __call__(self, scenes: List[Scene], flags: Optional[List[int]] = None, out: Optional[torch.Tensor] = None,
                 rng=_random) -> Tuple[torch.Tensor, torch.Tensor]:
        xb, ext = self.prepare(scenes, flags, out, rng)
        return xb, torch.tensor(ext, dtype=torch.int32).to(self.device, non_blocking=True)

    def prepare(self, scenes: List[Scene], flags: Optional[List[int]] = None, out: Optional[torch.Tensor] = None, rng=_random):
        """as __call__, but the extents come back as a host list (no device round trip)"""
        B, R = len(scenes), self.R
        xb = self._batch_out(out, (B, 4, R, R, R))
        ext = []
        staged = [self._stage_begin(i, sc) for i, sc in enumerate(scenes)]     # all host copies of the batch in flight at once
        for i in range(B):
            f = flags[i] if flags is not None else draw_augmentation(self.flip_prob, self.rotate_prob, rng)
            ext.append(list(self._prepare_slot(i, staged[i], xb[i], R, f)))
        return xb, ext


class DetectionBatcher(GridBatcher):
    """Input of the detection stack: stored scenes and their boxes -> `(xb (B,4,R,R,R) fp32, extents, targets)`, targets being the per-scene fp32 device
    tensors [G_i, 6|7] that FCOSOverNeRF, NeRFRegionProposalNetwork, fcos_targets and rpn_assign_targets take (views of one buffer).  What the reference's
    BaseDataset.augment_rpn_inputs does per scene on the CPU (datasets.py:173-244, 478-524) is one scene kernel per scene -- `ops.grid_prepare`, or
    `ops.grid_prepare_rs` for a scene that drew the small rotation + scaling -- and ONE box kernel per batch (`ops.boxes_augment`, its per-scene table passed
    as kernel arguments).  Scenes go through GridBatcher's pinned rings, host boxes through one pinned buffer of their own; nothing synchronises."""

    def __init__(self, resolution: int, device, normalize_density: bool = True, flip_prob: float = 0.0, rotate_prob: float = 0.0,
                 rot_scale_prob: float = 0.0, depth: int = 3, z_up: bool = True):
        if not z_up:
            raise NotImplementedError("DetectionBatcher: only z-up scenes (the reference's z_up=False, Hypersim, is not built)")
        super().__init__(resolution, device, normalize_density, flip_prob, rotate_prob, depth)
        self.rot_scale_prob = rot_scale_prob
        self._box_ring = _PinnedSlot(depth, self.device)

    def __call__(self, scenes: List[Scene], boxes, params=None, out: Optional[torch.Tensor] = None, rng=_random):
        xb, ext, targets = self.prepare(scenes, boxes, params, out, rng)
        return xb, torch.tensor(ext, dtype=torch.int32).to(self.device, non_blocking=True), targets

    def _stage_boxes(self, boxes, cols: int, counts: List[int]):
        """-> (device tensor [sum G, cols] holding the untransformed boxes, ring index or None)"""
        total = sum(counts)
        if total == 0:
            return torch.empty((0, cols), dtype=torch.float32, device=self.device), None
        if all(isinstance(b, torch.Tensor) and b.is_cuda for b in boxes):
            return torch.cat([b.to(torch.float32).reshape(-1, cols) for b in boxes]).contiguous(), None
        k, pin, dev = self._box_ring.acquire(total * cols, torch.float32)
        pin, dev = pin.view(total, cols), dev.view(total, cols)
        first = 0
        for b, n in zip(boxes, counts):
            if n and not (isinstance(b, torch.Tensor) and b.is_cuda):
                pin[first:first + n].copy_(torch.as_tensor(b).reshape(n, cols))
            first += n
        dev.copy_(pin, non_blocking=True)
        first = 0
        for b, n in zip(boxes, counts):
            if n and isinstance(b, torch.Tensor) and b.is_cuda:
                dev[first:first + n].copy_(b.reshape(n, cols))
            first += n
        return dev, k

    def prepare(self, scenes: List[Scene], boxes, params=None, out: Optional[torch.Tensor] = None, rng=_random):
        """boxes: one [G_i, 6|7] array per scene (numpy, host tensor or device tensor; the same column count in every scene); params: one
        (flags, angle, scale) per scene as `draw_detection_augmentation` returns them, None: drawn here from `rng`, scene by scene"""
        B, R = len(scenes), self.R
        if len(boxes) != B:
            raise ValueError("DetectionBatcher: one box array per scene")
        cols = {int(b.shape[-1]) for b in boxes}
        if len(cols) != 1 or not cols <= {6, 7} or any(b.ndim != 2 for b in boxes):
            raise ValueError("DetectionBatcher: boxes must be [G, 6] in every scene or [G, 7] in every scene")
        cols = cols.pop()
        counts = [int(b.shape[0]) for b in boxes]
        xb = self._batch_out(out, (B, 4, R, R, R))
        staged = [self._stage_begin(i, sc) for i, sc in enumerate(scenes)]     # all host copies of the batch in flight at once
        ext, table, first = [], [], 0
        for i in range(B):
            f, angle, scale = params[i] if params is not None else draw_detection_augmentation(self.flip_prob, self.rotate_prob, self.rot_scale_prob, cols == 7, rng)
            has_rs = (angle, scale) != (0.0, 1.0)
            if has_rs and cols != 7:
                raise ValueError("DetectionBatcher: rot-scale needs oriented (7-column) boxes")
            e = self._prepare_slot(i, staged[i], xb[i], R, f, angle, scale)
            ext.append(list(e))
            table.append((first, counts[i], f, has_rs, e, angle, scale))
            first += counts[i]
        dev, k = self._stage_boxes(boxes, cols, counts)
        outb = ops.boxes_augment(dev, table)
        if k is not None:
            self._box_ring.release_after(k, torch.cuda.current_stream())
        return xb, ext, [outb[t[0]:t[0] + t[1]] for t in table]


_LABEL_DTYPES = (torch.uint8, torch.int32, torch.int64, torch.float32)


class VoxelBatcher(GridBatcher):
    """Input of the two voxel heads: stored scenes and their stored targets -> `(xb (B,4,R,R,R) fp32, extents, tb)` with ONE augmentation draw per scene applied
    to both halves.  target="labels": a label volume (W,L,H) or (1,W,L,H) per scene, uint8 / int32 / int64 / float32, of the scene's own extents, through
    `ops.labels_prepare` -> tb (B,R,R,R) fp32, what the semantics head's loss and `SemanticEvaluator` take.  target="grid": a stored high-resolution scene
    (W',L',H',4) uint8 / float32 through `ops.grid_prepare` at `target_resolution` -> tb (B,4,Ro,Ro,Ro) fp32, the super-resolution head's target
    (`normalize_density` applies to float targets as to float inputs).  Targets go through pinned rings of their own under the event discipline of the scenes';
    pinned and device-resident targets are read in place.  Nothing synchronises.

    NOT the reference's behaviour for flip_prob / rotate_prob > 0: there the target takes the place of `boxes` in augment_rpn_inputs (datasets.py:150-167), whose
    assertion (:193-196) rejects it, so the reference's voxel runs work with all probabilities 0 only -- the default here.  With probabilities > 0 the draw
    of `draw_augmentation` (the reference's draw order with boxes=None) is applied to input and target alike."""

    def __init__(self, resolution: int, device, target: str = "labels", target_resolution: Optional[int] = None, normalize_density: bool = True,
                 flip_prob: float = 0.0, rotate_prob: float = 0.0, depth: int = 3):
        if target not in ("labels", "grid"):
            raise ValueError(f"VoxelBatcher: target must be 'labels' or 'grid', got {target!r}")
        super().__init__(resolution, device, normalize_density, flip_prob, rotate_prob, depth)
        self.target = target
        self.Ro = int(target_resolution) if (target == "grid" and target_resolution is not None) else resolution
        self._target_slots = {}

    def draw_flags(self, n: int, rng=_random) -> List[int]:
        """the flags of n successive scenes: one `draw_augmentation` each, in scene order"""
        return [draw_augmentation(self.flip_prob, self.rotate_prob, rng) for _ in range(n)]

    def _target_tensor(self, tgt, scene):
        t = torch.from_numpy(tgt) if isinstance(tgt, np.ndarray) else tgt
        if not isinstance(t, torch.Tensor):
            raise ValueError("VoxelBatcher: a target must be a numpy array or a torch tensor")
        if self.target == "grid":
            if t.dim() != 4 or t.shape[3] != 4 or t.dtype not in (torch.uint8, torch.float32):
                raise ValueError(f"VoxelBatcher: a grid target must be (W,L,H,4) uint8 or float32, got {tuple(t.shape)} {t.dtype}")
            return t
        if t.dtype not in _LABEL_DTYPES:
            raise ValueError(f"VoxelBatcher: a label volume must be uint8, int32, int64 or float32, got {t.dtype}")
        if t.dim() == 4 and t.shape[0] == 1:
            t = t[0]
        if t.dim() != 3 or tuple(t.shape) != tuple(scene.shape[:3]):
            raise ValueError(f"VoxelBatcher: a label volume must have its scene's extents {tuple(scene.shape[:3])} (or 1 in front of them), got {tuple(tgt.shape)}")
        return t

    def __call__(self, scenes: List[Scene], targets, flags: Optional[List[int]] = None, out: Optional[torch.Tensor] = None,
                 target_out: Optional[torch.Tensor] = None, rng=_random):
        xb, ext, tb = self.prepare(scenes, targets, flags, out, target_out, rng)
        return xb, torch.tensor(ext, dtype=torch.int32).to(self.device, non_blocking=True), tb

    def prepare(self, scenes: List[Scene], targets, flags: Optional[List[int]] = None, out: Optional[torch.Tensor] = None,
                target_out: Optional[torch.Tensor] = None, rng=_random):
        """targets: one per scene (see the class); flags: one per scene, None: drawn here from `rng`, scene by scene -> (xb, extents as a host list, tb)"""
        B, R, Ro = len(scenes), self.R, self.Ro
        if len(targets) != B:
            raise ValueError("VoxelBatcher: one target per scene")
        if flags is None:
            flags = self.draw_flags(B, rng)
        tgts = [self._target_tensor(t, scenes[i]) for i, t in enumerate(targets)]
        for i in range(B):                                   # (a rotation swaps two extents: the largest decides either way)
            if max(scenes[i].shape[:3]) > R:
                raise ValueError(f"VoxelBatcher: scene {i} of extents {tuple(scenes[i].shape[:3])} does not fit the resolution {R}")
            if self.target == "grid" and max(tgts[i].shape[:3]) > Ro:
                raise ValueError(f"VoxelBatcher: target {i} of extents {tuple(tgts[i].shape[:3])} does not fit the target resolution {Ro}")
        tshape = (B, R, R, R) if self.target == "labels" else (B, 4, Ro, Ro, Ro)
        xb, tb = self._batch_out(out, (B, 4, R, R, R)), self._batch_out(target_out, tshape, "target_out")
        staged = [self._stage_begin(i, sc) for i, sc in enumerate(scenes)]     # all host copies of the batch in flight at once, both halves
        staged_t = [self._stage_begin(i, t, self._target_slots) for i, t in enumerate(tgts)]
        ext = []
        for i in range(B):
            f = int(flags[i]) & (ops.GRID_ROT | ops.GRID_FLIP0 | ops.GRID_FLIP1)
            ext.append(list(self._prepare_slot(i, staged[i], xb[i], R, f)))
            if self.target == "grid":
                self._prepare_slot(i, staged_t[i], tb[i], Ro, f, slots=self._target_slots)
            else:
                tsrc, k = self._stage_end(*staged_t[i]), staged_t[i][1]
                ops.labels_prepare(tsrc, tb[i], R, f)
                if k is not None:
                    self._target_slots[i].release_after(k, torch.cuda.current_stream())
        return xb, ext, tb


def pin_scene(scene: np.ndarray) -> torch.Tensor:
    """page-locked copy of a stored scene: datasets that fit in host memory can be pinned once, after which every epoch's H2D copy
    reads the scene in place"""
    return torch.from_numpy(np.ascontiguousarray(scene)).pin_memory()


class Prefetcher:
    """Asynchronous input pipeline (the reference's DataLoader(num_workers=2, pin_memory=True), run_swin_mae3d.py:578-586): a
    background thread loads the scenes of batch k+1, stages them through the pinned rings and runs the H2D copies and the
    `grid_prepare` kernels on its own copy stream while step k computes; the consumer gets `(xb, extents, event)` and makes its
    stream wait for the event.  `depth` device batches rotate.  A buffer that has been handed out is PENDING until the consumer
    calls `done(slot)` -- which records the event after which it may be overwritten -- and ONLY `done` frees it: the producer first
    waits for the hand-back, then for that event (a consumer whose stream still has the device-to-device copy of batch n-2 queued
    behind a long replay can therefore never have buffer n%depth overwritten underneath it, whatever the thread timing).  The
    consumer MUST call `done` once per delivered batch.  Augmentation flags come from the prefetcher's OWN `random.Random`
    (`seed`), never from the global module the training thread draws its block masks from: both streams stay reproducible."""

    _PENDING = object()

    def __init__(self, batcher: GridBatcher, batches, batch_size: int, load=None, depth: int = 2, rng=None, seed: int = 0):
        import queue
        import threading
        # rng=None: a private generator (the global `random` module belongs to the training thread's mask draws)
        self.b, self.load, self.rng = batcher, load or (lambda s: s), (rng if rng is not None else _random.Random(seed))
        R, dev = batcher.R, batcher.device
        self.bufs = [torch.empty((batch_size, 4, R, R, R), dtype=torch.float32, device=dev) for _ in range(depth)]
        self.free = [None] * depth                      # None: never handed out; _PENDING: with the consumer; else the event after which buffer j may be overwritten
        self._handback = threading.Condition()
        self.stream = torch.cuda.Stream(device=dev, priority=-1)   # high priority: its small copy/prepare kernels slot in between the step's kernels
        self.q = queue.Queue(maxsize=depth - 1 if depth > 1 else 1)
        self.batches = batches
        self.err = None
        self._stop = False                              # close(): the producer leaves its wait loops and exits
        # the producer re-acquires the GIL after every C call (host copy, H2D, kernel launch: ~25 per batch); with CPython's default 5 ms
        # switch interval each hand-over from a busy consumer thread can take that long (measured: a 66 MB host copy 0.07 ms alone, 11 ms
        # next to a spinning Python thread) -- 0.2 ms keeps the producer's latency per call small against a 13-60 ms step
        import sys
        if sys.getswitchinterval() > 2e-4:
            sys.setswitchinterval(2e-4)
        self.t = threading.Thread(target=self._run, daemon=True)
        self.t.start()

    def _run(self):
        try:
            torch.cuda.set_device(self.b.device)
            import time
            st = self.stats = {"batches": 0, "load_s": 0.0, "wait_free_s": 0.0, "prepare_s": 0.0, "put_s": 0.0}   # producer-side wall clock per phase
            for n, batch in enumerate(self.batches):
                j = n % len(self.bufs)
                t0 = time.perf_counter()
                scenes = [self.load(s) for s in batch]
                flags = [draw_augmentation(self.b.flip_prob, self.b.rotate_prob, self.rng) for _ in scenes]
                t1 = time.perf_counter()
                with self._handback:                     # handed out before: wait until the consumer has given it back (done(j)) ...
                    while self.free[j] is Prefetcher._PENDING and not self._stop:
                        self._handback.wait(0.05)
                if self._stop:
                    return
                if self.free[j] is not None:
                    _wait_event(self.free[j])           # ... and until its last read of the buffer has executed
                t2 = time.perf_counter()
                with torch.cuda.stream(self.stream):
                    xb, ext = self.b.prepare(scenes, flags, out=self.bufs[j][:len(scenes)])
                    ev = torch.cuda.Event()
                    ev.record(self.stream)
                t3 = time.perf_counter()
                self.free[j] = Prefetcher._PENDING
                if not self._put((j, xb, ext, ev)):
                    return
                t4 = time.perf_counter()
                st["batches"] += 1; st["load_s"] += t1 - t0; st["wait_free_s"] += t2 - t1; st["prepare_s"] += t3 - t2; st["put_s"] += t4 - t3
            self._put(None)
        except BaseException as e:  # noqa: BLE001
            self.err = e
            self._put(None)

    def _put(self, item) -> bool:
        """bounded put: a consumer that went away must not park the thread for good (also for the terminating None).  False: stopped, `item` was dropped"""
        import queue
        while not self._stop:
            try:
                self.q.put(item, timeout=0.05)
                return True
            except queue.Full:
                continue
        return False

    def __iter__(self):
        try:
            while True:
                item = self.q.get()
                if item is None:
                    if self.err is not None:
                        raise self.err
                    return
                yield item
        finally:
            self.close()                                 # a consumer that leaves early (exception, break) releases the producer thread

    def close(self):
        """stop the producer (idempotent): it leaves its wait loops within 50 ms and drops its references to the staged batches"""
        import queue
        import threading
        self._stop = True
        with self._handback:
            self._handback.notify_all()

        def drain():
            try:
                while True:
                    self.q.get_nowait()
            except queue.Empty:
                pass
        drain()
        # the producer may have passed its `_stop` check just before the drain and still put one more staged batch: wait for it to exit (it leaves every
        # wait loop within 50 ms), then drain again so that no batch -- and no device buffer -- stays referenced by the queue
        t = getattr(self, "t", None)
        if t is not None and t.is_alive() and t is not threading.current_thread():
            t.join(timeout=1.0)
        drain()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def done(self, j: int, stream=None):
        """the consumer has queued its last read of buffer j on `stream`"""
        ev = torch.cuda.Event()
        ev.record(stream or torch.cuda.current_stream())
        with self._handback:
            self.free[j] = ev
            self._handback.notify_all()
