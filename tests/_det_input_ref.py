"""float64 numpy restatement of the reference's detection input pipeline (nerf_rpn/datasets.py): load_single_scene's conversions (:88-101, 247-248),
augment_rpn_inputs with z_up=True (:173-244) and rotate_and_scale_scene (:478-524).  The resample is an explicit 8-tap gather from the closed-form
coordinates below; it does not go through grid_sample.  Also the draw order and the seeded input generators of the golden file
(tests/golden/g25_det_input.npz, tools/gen_golden_det_input.py).  Nothing here imports the code under test.

Output voxel (i,j,k) of a grid with extents (r0,r1,r2) reads the grid at the continuous coordinates
    X = (2i/(r0-1) - 1) r0/2            Y = (2j/(r1-1) - 1) r1/2            Z = (2k/(r2-1) - 1) r2/2
    qx = s (cos a X - sin a Y)          qy = s (sin a X + cos a Y)          qz = s Z
    a0 = (qx/(r0/2) + 1)/2 (r0-1)       a1 = (qy/(r1/2) + 1)/2 (r1-1)       a2 = (qz/(r2/2) + 1)/2 (r2-1)
trilinear over the 8 integer neighbours, a neighbour outside [0,r) on any axis contributing 0."""
import functools
import math
import random

import numpy as np

ROT, FLIP0, FLIP1, DENSITY = 1, 2, 4, 8

# the golden file's cases: (name, seed, (W,L,H), dtype); every case is run with 6-column and with 7-column boxes under random.seed(seed)
PROBS = dict(flip_prob=0.5, rotate_prob=0.5, rot_scale_prob=0.6)
SMALL = [("s0", 2, (12, 10, 8), "f32"), ("s1", 21, (9, 12, 7), "u8"), ("s2", 15, (8, 8, 12), "f32"), ("s3", 4, (12, 10, 8), "u8"),
         ("s4", 19, (9, 12, 7), "f32"), ("s5", 10, (8, 8, 12), "u8"), ("s6", 12, (10, 12, 9), "f32"), ("s7", 3, (11, 7, 12), "u8"),
         ("s8", 5, (12, 9, 10), "f32"), ("s9", 9, (7, 11, 8), "u8"), ("s10", 6, (12, 12, 6), "f32"), ("s11", 28, (6, 9, 12), "u8")]
LARGE = [("m0", 20, (40, 36, 24), "f32"), ("m1", 21, (40, 36, 24), "u8"), ("l0", 22, (160, 132, 96), "u8")]
# the large cases fix their draw (the reference's rotate_and_scale_scene is called directly): rot + flip + rot-scale
LARGE_DRAW = {"m0": (ROT | FLIP1, 0.15, 0.93), "m1": (FLIP0, -0.12, 1.08), "l0": (ROT | FLIP0, 0.16, 0.91)}
N_BOXES = 5
DRAW_SEEDS = 64
SAMPLE = 4096


def make_scene(seed, shape, dtype):
    """stored scene (W,L,H,4): RGB in [0,1), raw density N(0, 3^2) (fp32), or all four channels 0..255 (uint8)"""
    rng = np.random.default_rng(1000 + seed)
    W, L, H = shape
    if dtype == "u8":
        return rng.integers(0, 256, size=(W, L, H, 4), dtype=np.uint8)
    g = rng.random((W, L, H, 4), dtype=np.float32)
    g[..., 3] = (rng.standard_normal((W, L, H)) * 3.0).astype(np.float32)
    return g


def make_boxes(seed, shape, cols, n=N_BOXES):
    """fp32 boxes inside the scene: [n,6] (min, max) or [n,7] (centre, dims, theta)"""
    rng = np.random.default_rng(2000 + seed)
    ext = np.asarray(shape, dtype=np.float64)
    c = rng.uniform(0.2, 0.8, size=(n, 3)) * ext
    d = rng.uniform(0.1, 0.35, size=(n, 3)) * ext
    if cols == 6:
        return np.concatenate([c - d / 2, c + d / 2], 1).astype(np.float32)
    th = rng.uniform(-math.pi / 2, math.pi / 2, size=(n, 1))
    return np.concatenate([c, d, th], 1).astype(np.float32)


def draw(flip_prob, rotate_prob, rot_scale_prob, oriented, rng=random):
    """-> (flags, taken, angle, scale, number of rng calls), in the reference's order (datasets.py:198, 221, 238-241)"""
    n = 3
    flags = 0
    if rng.random() < rotate_prob:
        flags |= ROT
    if rng.random() < flip_prob:
        flags |= FLIP0
    if rng.random() < flip_prob:
        flags |= FLIP1
    taken, angle, scale = False, 0.0, 1.0
    if oriented:
        n += 1
        if rng.random() < rot_scale_prob:
            taken, angle, scale, n = True, rng.uniform(-np.pi / 18, np.pi / 18), rng.uniform(0.9, 1.1), n + 2
    return flags, taken, angle, scale, n


def to_grid(scene, density=True):
    """stored (W,L,H,4) -> channels-first float64 (4,W,L,H): uint8 / 255; fp32: density -> alpha on channel 3"""
    g = scene.astype(np.float64)
    if scene.dtype == np.uint8:
        g = g / 255.0
    elif density:
        g[..., 3] = np.clip(1.0 - np.exp(-np.exp(g[..., 3]) / 100.0), 0.0, 1.0)
    return np.ascontiguousarray(np.transpose(g, (3, 0, 1, 2)))


def rot_flip(grid, flags):
    if flags & ROT:
        grid = np.flip(np.swapaxes(grid, 1, 2), 1)
    if flags & FLIP0:
        grid = np.flip(grid, 1)
    if flags & FLIP1:
        grid = np.flip(grid, 2)
    return np.ascontiguousarray(grid)


def coords(res, angle, scale):
    """-> a0 [r0,r1], a1 [r0,r1], a2 [r2]"""
    r0, r1, r2 = res
    X = ((2.0 * np.arange(r0) / (r0 - 1) - 1.0) * r0 / 2.0)[:, None]
    Y = ((2.0 * np.arange(r1) / (r1 - 1) - 1.0) * r1 / 2.0)[None, :]
    Z = (2.0 * np.arange(r2) / (r2 - 1) - 1.0) * r2 / 2.0
    c, s = math.cos(angle), math.sin(angle)
    qx, qy, qz = scale * (c * X - s * Y), scale * (s * X + c * Y), scale * Z
    return (qx / (r0 / 2.0) + 1.0) / 2.0 * (r0 - 1), (qy / (r1 / 2.0) + 1.0) / 2.0 * (r1 - 1), (qz / (r2 / 2.0) + 1.0) / 2.0 * (r2 - 1)


def resample(grid, angle, scale, want_counts=False):
    """grid (C,r0,r1,r2) float64 -> the resampled grid; want_counts: also the number of in-range taps per voxel [r0,r1,r2]"""
    C, r0, r1, r2 = grid.shape
    a0, a1, a2 = coords((r0, r1, r2), angle, scale)
    x0, y0, z0 = np.floor(a0).astype(np.int64), np.floor(a1).astype(np.int64), np.floor(a2).astype(np.int64)
    fx, fy, fz = a0 - x0, a1 - y0, a2 - z0
    out = np.zeros_like(grid)
    counts = np.zeros((r0, r1, r2), dtype=np.int64)
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                xi, yi, zi = x0 + dx, y0 + dy, z0 + dz
                w = ((fx if dx else 1.0 - fx) * (fy if dy else 1.0 - fy))[:, :, None] * (fz if dz else 1.0 - fz)[None, None, :]
                ok = (((xi >= 0) & (xi < r0) & (yi >= 0) & (yi < r1))[:, :, None] & ((zi >= 0) & (zi < r2))[None, None, :])
                v = grid[:, np.clip(xi, 0, r0 - 1)[:, :, None], np.clip(yi, 0, r1 - 1)[:, :, None], np.clip(zi, 0, r2 - 1)[None, None, :]]
                out += v * (w * ok)[None]
                counts += ok
    return (out, counts) if want_counts else out


def prepare(scene, flags, taken=False, angle=0.0, scale=1.0, density=True):
    """the whole scene side: stored scene -> augmented (4,A0,A1,H) float64"""
    g = rot_flip(to_grid(scene, density), flags)
    return resample(g, angle, scale) if taken else g


def pad(grid, R, fill=0.0):
    out = np.full((grid.shape[0], R, R, R), fill, dtype=grid.dtype)
    out[:, :grid.shape[1], :grid.shape[2], :grid.shape[3]] = grid
    return out


def extents(shape, flags):
    W, L, H = shape
    return (L, W, H) if flags & ROT else (W, L, H)


def boxes_augment(boxes, shape, flags, taken=False, angle=0.0, scale=1.0):
    """boxes [n,6|7] of a scene stored as `shape` -> float64 boxes after the transforms (datasets.py:206-233, 514-522, z_up=True)"""
    b = np.array(boxes, dtype=np.float64)
    e = extents(shape, flags)
    if b.shape[1] == 6:
        if flags & ROT:
            b[:, [0, 1, 3, 4]] = b[:, [1, 0, 4, 3]]
            b[:, [0, 3]] = e[0] - b[:, [3, 0]]
        for axis, f in ((0, FLIP0), (1, FLIP1)):
            if flags & f:
                b[:, [axis, axis + 3]] = e[axis] - b[:, [axis + 3, axis]]
        assert not taken
        return b
    if flags & ROT:
        b[:, [0, 1, 3, 4]] = b[:, [1, 0, 4, 3]]
        b[:, 0] = e[0] - b[:, 0]
    for axis, f in ((0, FLIP0), (1, FLIP1)):
        if flags & f:
            b[:, axis] = e[axis] - b[:, axis]
            b[:, 6] = -b[:, 6]
    if taken:
        c, s = math.cos(angle), math.sin(angle)
        m = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]) / scale
        b[:, 6] -= angle
        b[:, 3:6] /= scale
        h = np.asarray(e, dtype=np.float64) / 2.0
        b[:, :3] = (b[:, :3] - h) @ m + h
    return b


def strided_sample(grid, n=SAMPLE):
    flat = grid.reshape(-1)
    idx = (np.arange(n, dtype=np.int64) * ((flat.size // n) | 1)) % flat.size if flat.size > n else np.arange(flat.size)
    return idx, flat[idx]


@functools.lru_cache(maxsize=None)
def large_reference(name):
    """-> (scene, boxes, (flags, angle, scale), restated grid float64, restated boxes float64) of a LARGE case, computed once per process"""
    _, seed, shape, dtype = next(c for c in LARGE if c[0] == name)
    flags, angle, scale = LARGE_DRAW[name]
    scene, boxes = make_scene(seed, shape, dtype), make_boxes(seed, shape, 7)
    return scene, boxes, (flags, angle, scale), prepare(scene, flags, True, angle, scale), boxes_augment(boxes, shape, flags, True, angle, scale)
