"""The detection input pipeline on the GPU (csrc/det_input.hip through nerf_mae_amd.ops / data / det_data) against the float64 restatement of
tests/_det_input_ref.py, itself pinned to the recorded reference (tests/golden/g25_det_input.npz) in tests/test_det_input_ref_cpu.py.

Bound: |kernel - restatement64| <= 4 * e_ref(case), e_ref being the reference's own fp32 error against float64 as recorded in the golden file (grid and boxes
separately).  The error is coordinate rounding, about extent * 2^-23 voxels per axis times the local gradient; a different, equally valid fp32 evaluation order
on three independent axes can land on the other side of the float64 value, hence the margin of 4.  Trilinear interpolation with zero padding is continuous
in the coordinates, so no voxel is excluded.  Any real mistake (align_corners, axis order, the sign of the angle, alpha after blending) is >= 1e4 times larger.
Outside the valid extents the output is exactly 0.

The reference-signature wrappers are compared with the golden file itself: their input is the restatement's float64 grid rounded to fp32 (at most 2^-24 from
what the reference was given, up to its e_ref), so the bound is 4 e_ref (kernel against restatement) + e_ref (restatement against golden) + 2^-24.

Targets into the assigners (32^3 scene): integer and boolean results are compared exactly, fp32 results to 1e-4 absolute -- the boxes differ by at most 4 e_ref
(~ 4e-6) from the uploaded restatement and every fp32 result is a smooth function of them with slope O(1) .. O(10) at these sizes."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _det_input_ref as D  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g25_det_input.npz"))
SMALL_RUNS = [(name, cols) for name, _, _, _ in D.SMALL for cols in (6, 7)]
MARGIN = 4.0


def _ops():
    from nerf_mae_amd import ops
    return ops


def _data():
    from nerf_mae_amd import data
    return data


def small(name, cols):
    _, seed, shape, dtype = next(c for c in D.SMALL if c[0] == name)
    d = GOLD[f"{name}_{cols}_draw"]
    return seed, shape, D.make_scene(seed, shape, dtype), D.make_boxes(seed, shape, cols), (int(d[0]), bool(d[1]), float(d[2]), float(d[3]))


def check_grid(got, want, e_ref, tag):
    """got (4,R,R,R) fp32 from the device, want (4,A0,A1,H) float64"""
    got = got.double().cpu().numpy()
    _, a0, a1, h = want.shape
    err = np.abs(got[:, :a0, :a1, :h] - want).max()
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  [{tag}] max err {err:.3e}  e_ref {e_ref:.3e}  ratio {err / max(e_ref, 1e-300):.2f}")
    assert err <= MARGIN * e_ref, f"{tag}: {err:.3e} > {MARGIN} * {e_ref:.3e}"
    outside = got.copy()
    outside[:, :a0, :a1, :h] = 0.0
    assert not outside.any(), f"{tag}: {np.count_nonzero(outside)} non-zero padding voxels"


def check_boxes(got, want, e_ref, tag):
    got = got.double().cpu().numpy()
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    err = np.abs(got - want).max() if want.size else 0.0
    if os.environ.get("NMH_PRINT_ERR"):
        print(f"  [{tag}] boxes max err {err:.3e}  e_ref {e_ref:.3e}")
    assert err <= MARGIN * e_ref, f"{tag}: {err:.3e} > {MARGIN} * {e_ref:.3e}"


# ---- a. every small golden case through the kernel -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cols", SMALL_RUNS)
def test_small_cases(name, cols):
    ops = _ops()
    seed, shape, scene, _, (flags, taken, angle, scale) = small(name, cols)
    R = 16
    dst = torch.full((4, R, R, R), 7.0, dtype=torch.float32, device="cuda")
    f = flags | (ops.GRID_DENSITY if scene.dtype == np.float32 else 0)
    ext = ops.grid_prepare_rs(torch.from_numpy(scene).cuda(), dst, R, f, angle, scale)      # not taken: angle 0, scale 1, still this kernel
    assert tuple(ext) == D.extents(shape, flags)
    check_grid(dst, D.prepare(scene, flags, taken, angle, scale), float(GOLD[f"{name}_{cols}_e_ref_grid"]), f"{name} {cols} columns")


# ---- b. (40,36,24) fp32 and uint8 at R = 40 -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["m0", "m1"])
def test_medium_cases(name):
    ops = _ops()
    scene, _, (flags, angle, scale), want, _ = D.large_reference(name)
    R = 40
    dst = torch.full((4, R, R, R), 7.0, dtype=torch.float32, device="cuda")
    f = flags | (ops.GRID_DENSITY if scene.dtype == np.float32 else 0)
    ops.grid_prepare_rs(torch.from_numpy(scene).cuda(), dst, R, f, angle, scale)
    check_grid(dst, want, float(GOLD[name + "_e_ref_grid"]), name)


# ---- c. boxes ---------------------------------------------------------------------------------------------------------------------------------------
def _box_batch(cols, picks):
    """picks: [(case, rows kept)] -> (concatenated boxes, table, [(want, e_ref)])"""
    cat, table, wants, first = [], [], [], 0
    for name, n in picks:
        _, shape, _, boxes, (flags, taken, angle, scale) = small(name, cols)
        boxes = boxes[:n]
        cat.append(boxes)
        table.append((first, n, flags, taken, D.extents(shape, flags), angle, scale))
        wants.append((D.boxes_augment(boxes, shape, flags, taken, angle, scale), float(GOLD[f"{name}_{cols}_e_ref_boxes"])))
        first += n
    return np.concatenate(cat), table, wants


@pytest.mark.parametrize("cols", [6, 7])
def test_boxes(cols):
    ops = _ops()
    batches = [[("s0", 5), ("s3", 0), ("s7", 3)],                    # three scenes, 5 / 0 / 3 boxes: rot-scale, rot + both flips + rot-scale, not taken
               [(name, D.N_BOXES) for name, _, _, _ in D.SMALL]]    # every small case in one launch
    for picks in batches:
        boxes, table, wants = _box_batch(cols, picks)
        out = ops.boxes_augment(torch.from_numpy(boxes).cuda(), table)
        assert out.shape == boxes.shape and out.dtype == torch.float32
        for (name, _), (first, n, *_), (want, e_ref) in zip(picks, table, wants):
            check_boxes(out[first:first + n], want, e_ref, f"{name} {cols} columns")
    empty = ops.boxes_augment(torch.zeros((0, cols), device="cuda"), [(0, 0, 7, False, (8, 8, 8), 0.0, 1.0)])
    assert empty.shape == (0, cols)


def test_large_boxes():
    ops = _ops()
    for name, _, shape, _ in D.LARGE:
        _, boxes, (flags, angle, scale), _, want = D.large_reference(name)
        out = ops.boxes_augment(torch.from_numpy(boxes).cuda(), [(0, boxes.shape[0], flags, True, D.extents(shape, flags), angle, scale)])
        check_boxes(out, want, float(GOLD[name + "_e_ref_boxes"]), name)


# ---- d, e. the batcher: bit-equal to GridBatcher without rot-scale; deterministic ----------------------------------------------------------------
def _mixed_batch():
    scenes = [D.make_scene(31, (20, 17, 13), "f32"), D.make_scene(32, (16, 24, 11), "u8"), D.make_scene(33, (24, 24, 24), "f32")]
    return scenes, [D.make_boxes(31, (20, 17, 13), 7, n=4), D.make_boxes(32, (16, 24, 11), 7, n=0), D.make_boxes(33, (24, 24, 24), 7, n=2)]


def test_batcher_without_rot_scale_is_gridbatcher_bit_for_bit():
    data = _data()
    scenes, boxes = _mixed_batch()
    flags = [5, 2, 7]
    xb0, ext0 = data.GridBatcher(24, "cuda").prepare(scenes, flags)
    xb1, ext1, targets = data.DetectionBatcher(24, "cuda").prepare(scenes, boxes, [(f, 0.0, 1.0) for f in flags])
    assert ext0 == ext1 and torch.equal(xb0, xb1)
    assert [tuple(t.shape) for t in targets] == [(4, 7), (0, 7), (2, 7)]
    for t, b, sc, f in zip(targets, boxes, scenes, flags):
        check_boxes(t, D.boxes_augment(b, sc.shape[:3], f), 2.0 ** -19, "flags only")      # half an ulp of a coordinate below 32 per subtraction, one per flag


def test_two_runs_are_bit_identical_and_box_sources_agree():
    data = _data()
    scenes, boxes = _mixed_batch()
    params = [(5, 0.15, 0.93), (2, -0.1, 1.08), (0, 0.0, 1.0)]
    b = data.DetectionBatcher(24, "cuda")
    xb0, ext0, t0 = b.prepare(scenes, boxes, params)
    xb0, t0 = xb0.clone(), [t.clone() for t in t0]
    mixed = [torch.from_numpy(boxes[0]).cuda(), torch.from_numpy(boxes[1]), boxes[2]]     # device tensor, host tensor, numpy
    xb1, ext1, t1 = b.prepare([torch.from_numpy(s).cuda() for s in scenes], mixed, params)
    assert ext0 == ext1 and torch.equal(xb0, xb1) and all(torch.equal(a, c) for a, c in zip(t0, t1))
    xb2, _, t2 = b(scenes, [torch.from_numpy(x).cuda() for x in boxes], params)[0:3]
    assert torch.equal(xb0, xb2) and all(torch.equal(a, c) for a, c in zip(t0, t2))
    for i, (sc, (f, a, s)) in enumerate(zip(scenes, params)):
        taken = (a, s) != (0.0, 1.0)
        want = D.prepare(sc, f, taken, a, s)
        assert np.abs(xb0[i].double().cpu().numpy()[:, :want.shape[1], :want.shape[2], :want.shape[3]] - want).max() <= 1e-5      # a sanity bound: the real ones are tests a, b, f


def test_batcher_makes_no_host_synchronisation():
    data = _data()
    scenes, boxes = _mixed_batch()
    params = [(5, 0.15, 0.93), (2, -0.1, 1.08), (0, 0.0, 1.0)]
    b = data.DetectionBatcher(24, "cuda")
    out = torch.empty((3, 4, 24, 24, 24), device="cuda")
    xb0, _, t0 = b.prepare(scenes, boxes, params)                    # allocates the pinned rings
    xb0, t0 = xb0.clone(), [t.clone() for t in t0]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        xb1, _, t1 = b.prepare(scenes, boxes, params, out=out)       # host scenes, host boxes: pinned copies, kernels, nothing that waits
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert xb1.data_ptr() == out.data_ptr() and torch.equal(xb0, xb1) and all(torch.equal(a, c) for a, c in zip(t0, t1))
    assert len({t.untyped_storage().data_ptr() for t in t1}) == 1     # views of one buffer


def test_batcher_draws_in_the_reference_order():
    data = _data()
    scenes, boxes = _mixed_batch()
    b = data.DetectionBatcher(24, "cuda", flip_prob=0.5, rotate_prob=0.5, rot_scale_prob=0.6)
    xb0, ext0, t0 = b.prepare(scenes, boxes, rng=random.Random(4))
    rng = random.Random(4)
    params = [data.draw_detection_augmentation(0.5, 0.5, 0.6, True, rng) for _ in scenes]
    xb1, ext1, t1 = b.prepare(scenes, boxes, params)
    assert ext0 == ext1 and torch.equal(xb0, xb1) and all(torch.equal(a, c) for a, c in zip(t0, t1))
    six = [D.make_boxes(40 + i, s.shape[:3], 6, n=2) for i, s in enumerate(scenes)]
    rng6 = random.Random(4)
    b.prepare(scenes, six, rng=rng6)
    ref6 = random.Random(4)
    for _ in range(3 * len(scenes)):
        ref6.random()
    assert rng6.random() == ref6.random()                           # axis-aligned boxes: exactly three draws per scene


# ---- f. one (160,132,96) uint8 scene through the batcher ------------------------------------------------------------------------------------------
def test_full_size_scene_through_the_batcher():
    data = _data()
    scene, boxes, (flags, angle, scale), want, want_boxes = D.large_reference("l0")
    xb, ext, targets = data.DetectionBatcher(160, "cuda").prepare([scene], [boxes], [(flags, angle, scale)])
    assert ext == [list(D.extents(scene.shape[:3], flags))]
    check_grid(xb[0], want, float(GOLD["l0_e_ref_grid"]), "l0")
    check_boxes(targets[0], want_boxes, float(GOLD["l0_e_ref_boxes"]), "l0")


# ---- g. the targets feed the assigners --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [6, 7])
def test_targets_feed_the_assigners(cols):
    from nerf_mae_amd import fcos_loss, rpn
    from tests import _rpn_ref as R
    data = _data()
    shapes = [(32, 32, 32), (28, 32, 30)]
    scenes = [D.make_scene(50 + i, s, "u8") for i, s in enumerate(shapes)]
    boxes = [D.make_boxes(50, shapes[0], cols, n=3), D.make_boxes(51, shapes[1], cols, n=2)]
    params = [(3, 0.12, 0.95), (4, -0.08, 1.06)] if cols == 7 else [(3, 0.0, 1.0), (4, 0.0, 1.0)]
    _, ext, targets = data.DetectionBatcher(32, "cuda").prepare(scenes, boxes, params)
    want = [torch.from_numpy(D.boxes_augment(b, s, f, (a, k) != (0.0, 1.0), a, k).astype(np.float32)).cuda() for b, s, (f, a, k) in zip(boxes, shapes, params)]
    gen = rpn.AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS)
    runs = []
    for t in (targets, want):
        runs.append(list(fcos_loss.fcos_targets(((8, 8, 8), (4, 4, 4), (2, 2, 2), (1, 1, 1)), (4, 8, 16, 32), t))
                    + list(rpn.rpn_assign_targets(gen, R.MESH, R.GRIDS, t, ext, rotated=cols == 7)))
    assert any(bool((x > 0).any()) for x in runs[1][:1])
    for got, ref in zip(*runs):
        assert got.shape == ref.shape and got.dtype == ref.dtype
        if got.dtype.is_floating_point:
            assert (got - ref).abs().max().item() <= 1e-4
        else:
            assert torch.equal(got, ref)


# ---- h. the reference-signature wrappers against the golden file -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cols", SMALL_RUNS)
def test_augment_rpn_inputs_wrapper(name, cols):
    from nerf_mae_amd import det_data
    seed, shape, scene, boxes, (flags, taken, angle, scale) = small(name, cols)
    grid = torch.from_numpy(D.to_grid(scene).astype(np.float32)).cuda()
    random.seed(seed)
    og, ob = det_data.augment_rpn_inputs(grid, torch.from_numpy(boxes).cuda(), **D.PROBS)
    pre = f"{name}_{cols}_"
    assert tuple(og.shape) == GOLD[pre + "grid"].shape and og.is_contiguous()
    assert np.abs(og.double().cpu().numpy() - GOLD[pre + "grid"]).max() <= (MARGIN + 1) * float(GOLD[pre + "e_ref_grid"]) + 2.0 ** -24
    assert np.abs(ob.double().cpu().numpy() - GOLD[pre + "boxes"]).max() <= (MARGIN + 1) * float(GOLD[pre + "e_ref_boxes"])
    og2, none = det_data.augment_rpn_inputs(grid, None, 0.0, 0.0, 1.0)              # boxes=None: three draws, no rot-scale
    assert none is None and torch.equal(og2, grid)


def test_rotate_and_scale_scene_wrapper():
    from nerf_mae_amd import det_data
    done = 0
    for name, _, _, _ in D.SMALL:
        seed, shape, scene, boxes, (flags, taken, angle, scale) = small(name, 7)
        if flags or not taken:
            continue
        grid = torch.from_numpy(D.to_grid(scene).astype(np.float32)).cuda()
        og, ob = det_data.rotate_and_scale_scene(grid, torch.from_numpy(boxes).cuda(), angle, scale)
        assert np.abs(og.double().cpu().numpy() - GOLD[f"{name}_7_grid"]).max() <= (MARGIN + 1) * float(GOLD[f"{name}_7_e_ref_grid"]) + 2.0 ** -24
        assert np.abs(ob.double().cpu().numpy() - GOLD[f"{name}_7_boxes"]).max() <= (MARGIN + 1) * float(GOLD[f"{name}_7_e_ref_boxes"])
        og2, none = det_data.rotate_and_scale_scene(grid, None, angle, scale)
        assert none is None and torch.equal(og, og2)
        done += 1
    assert done >= 1


# ---- error paths ------------------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    from nerf_mae_amd import det_data
    from nerf_mae_amd._lib import NmhError
    ops, data = _ops(), _data()
    dst = torch.zeros((4, 8, 8, 8), device="cuda")
    with pytest.raises(NmhError):
        ops.grid_prepare_rs(torch.zeros((1, 4, 4, 4), device="cuda"), dst, 8, 0, 0.1, 1.0)        # an extent below 2
    with pytest.raises(NmhError):
        ops.grid_prepare_rs(torch.zeros((9, 4, 4, 4), device="cuda"), dst, 8, 0, 0.1, 1.0)        # does not fit the resolution
    with pytest.raises(ValueError):
        ops.boxes_augment(torch.zeros((2, 6), device="cuda"), [(0, 2, 0, True, (8, 8, 8), 0.1, 1.0)])     # rot-scale on 6 columns
    with pytest.raises(ValueError):
        ops.boxes_augment(torch.zeros((2, 7), device="cuda"), [(1, 2, 0, False, (8, 8, 8), 0.0, 1.0)])    # rows outside the boxes
    with pytest.raises(NotImplementedError):
        data.DetectionBatcher(8, "cuda", z_up=False)
    with pytest.raises(NotImplementedError):
        det_data.augment_rpn_inputs(dst, None, 0.0, 0.0, 0.0, z_up=False)
    with pytest.raises(ValueError):
        data.DetectionBatcher(8, "cuda").prepare([np.zeros((4, 4, 4, 4), np.float32)] * 2, [np.zeros((1, 6), np.float32), np.zeros((1, 7), np.float32)])
