"""numpy restatement of the paired transform of the voxel heads' input pipeline, on a label volume (W,L,H) or a channels-last stored grid (W,L,H,4), by
literally the reference's two operations (nerf_rpn/datasets.py:200-201 `transpose(1, 2)` + `flip(1)` on the channel-first tensor, :222 `flip(axis + 1)`; here
on the arrays without the leading channel axis, so axes 0 and 1), then pad_tensor's zero padding at the high end of every axis (torch_utils.py:56-90).

flags: 1 = the z-up 90-degree rotation, 2 = flip axis 0, 4 = flip axis 1, applied in that order (the bits of ops.GRID_ROT / GRID_FLIP0 / GRID_FLIP1)."""
import numpy as np

ROT, FLIP0, FLIP1 = 1, 2, 4
INV255 = np.float32(1.0) / np.float32(255.0)          # the kernel's fp32 constant 1.0f / 255.0f


def augment(a: np.ndarray, flags: int) -> np.ndarray:
    """the rotation and flips on the first two axes of `a`; the last spatial axis is never touched"""
    if flags & ROT:
        a = np.flip(np.swapaxes(a, 0, 1), 0)
    if flags & FLIP0:
        a = np.flip(a, 0)
    if flags & FLIP1:
        a = np.flip(a, 1)
    return a


def pad(a: np.ndarray, R: int) -> np.ndarray:
    """zero padding of the three leading axes to R at the high end"""
    out = np.zeros((R, R, R) + a.shape[3:], dtype=a.dtype)
    out[:a.shape[0], :a.shape[1], :a.shape[2]] = a
    return out


def labels_ref(vol: np.ndarray, R: int, flags: int) -> np.ndarray:
    """(W,L,H) class ids of any dtype -> (R,R,R) float32"""
    return pad(augment(vol, flags).astype(np.float32), R)


def alpha(sigma: np.ndarray) -> np.ndarray:
    """density -> alpha (datasets.py:247-248) in float32"""
    one, hundred = np.float32(1.0), np.float32(100.0)
    return np.clip(one - np.exp(-np.exp(sigma.astype(np.float32)) / hundred), np.float32(0.0), one).astype(np.float32)


def grid_ref(scene: np.ndarray, R: int, flags: int, normalize_density: bool = True) -> np.ndarray:
    """stored scene (W,L,H,4) uint8 | float32 -> (4,R,R,R) float32: uint8 * (1/255) in fp32; float32 with density -> alpha on channel 3"""
    if scene.dtype == np.uint8:
        g = scene.astype(np.float32) * INV255
    else:
        g = scene.astype(np.float32).copy()
        if normalize_density:
            g[..., 3] = alpha(g[..., 3])
    return np.ascontiguousarray(np.moveaxis(pad(augment(g, flags), R), 3, 0))


def extents(shape, flags: int):
    W, L, H = shape[:3]
    return [L, W, H] if flags & ROT else [W, L, H]
