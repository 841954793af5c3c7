"""The float64 restatement of the detection input pipeline (tests/_det_input_ref.py) against the recorded reference (tests/golden/g25_det_input.npz, written
by tools/gen_golden_det_input.py from nerf_rpn/datasets.py on the CPU), the host-side draw of nerf_mae_amd.data against the recorded draws, and the C ABI's
declarations.  No GPU.

The restatement must reproduce every stored grid and box to within the recorded e_ref (the reference's own fp32 error against float64, measured when the
file was written; 3e-8 .. 1.4e-6 on the small grids, 4e-6 at 40 x 36 x 24, 1.9e-5 at 160 x 132 x 96): that pins the restatement the GPU tests compare with."""
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _det_input_ref as D  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g25_det_input.npz"))
SMALL_RUNS = [(name, cols) for name, _, _, _ in D.SMALL for cols in (6, 7)]


def unpack(draw):
    return int(draw[0]), bool(draw[1]), float(draw[2]), float(draw[3]), int(draw[4])


@pytest.mark.parametrize("name,cols", SMALL_RUNS)
def test_small_cases_within_e_ref(name, cols):
    _, seed, shape, dtype = next(c for c in D.SMALL if c[0] == name)
    pre = f"{name}_{cols}_"
    scene, boxes = D.make_scene(seed, shape, dtype), D.make_boxes(seed, shape, cols)
    assert abs(scene.astype(np.float64).sum() - float(GOLD[name + "_input_sum"])) <= 1e-9 * abs(float(GOLD[name + "_input_sum"]))
    flags, taken, angle, scale, calls = unpack(GOLD[pre + "draw"])
    assert (flags, taken, angle, scale, calls) == D.draw(rng=random.Random(seed), oriented=cols == 7, **D.PROBS)
    grid = D.prepare(scene, flags, taken, angle, scale)
    assert grid.shape == GOLD[pre + "grid"].shape == (4,) + D.extents(shape, flags)
    assert np.abs(grid - GOLD[pre + "grid"]).max() <= float(GOLD[pre + "e_ref_grid"])
    assert np.abs(D.boxes_augment(boxes, shape, flags, taken, angle, scale) - GOLD[pre + "boxes"]).max() <= float(GOLD[pre + "e_ref_boxes"])
    assert float(GOLD[pre + "e_ref_grid"]) < 2e-6 and float(GOLD[pre + "e_ref_boxes"]) < 2e-6      # fp32 rounding at extents <= 12, nothing larger


def test_small_cases_cover_every_branch():
    draws = [unpack(GOLD[f"{name}_7_draw"]) for name, _, _, _ in D.SMALL]
    for f in (D.ROT, D.FLIP0, D.FLIP1):
        assert {bool(d[0] & f) for d in draws} == {True, False}
    rs = [d for d in draws if d[1]]
    assert 0 < len(rs) < len(draws)
    assert any(d[2] > 0 for d in rs) and any(d[2] < 0 for d in rs) and any(d[3] < 0.95 for d in rs) and any(d[3] > 1.05 for d in rs)
    assert any(d[0] & D.ROT and shape[0] != shape[1] for d, (_, _, shape, _) in zip(draws, D.SMALL))
    edge = False
    for d, (_, _, shape, _) in zip(draws, D.SMALL):
        if d[1]:
            _, counts = D.resample(np.zeros((1,) + D.extents(shape, d[0])), d[2], d[3], want_counts=True)
            edge = edge or (bool((counts == 0).any()) and bool(((counts > 0) & (counts < 8)).any()))
    assert edge


@pytest.mark.parametrize("name", [c[0] for c in D.LARGE])
def test_large_cases_within_e_ref(name):
    scene, boxes, (flags, angle, scale), grid, out_boxes = D.large_reference(name)
    assert unpack(GOLD[name + "_draw"]) == (flags, True, angle, scale, 6)
    e = float(GOLD[name + "_e_ref_grid"])
    idx, sample = D.strided_sample(grid)
    assert np.abs(sample - GOLD[name + "_sample"]).max() <= e
    assert abs(grid.sum() - float(GOLD[name + "_sum"])) <= e * grid.size
    assert np.abs(out_boxes - GOLD[name + "_boxes"]).max() <= float(GOLD[name + "_e_ref_boxes"])


class CountingRandom(random.Random):
    def __init__(self, seed):
        super().__init__(seed)
        self.calls = 0

    def random(self):
        self.calls += 1
        return super().random()

    def uniform(self, a, b):            # random.Random.uniform calls self.random(): count it once
        before = self.calls
        v = super().uniform(a, b)
        self.calls = before + 1
        return v


@pytest.mark.parametrize("cols", [6, 7])
def test_draw_order_matches_the_recorded_draws(cols):
    from nerf_mae_amd import data, ops
    assert (ops.GRID_ROT, ops.GRID_FLIP0, ops.GRID_FLIP1) == (D.ROT, D.FLIP0, D.FLIP1)
    rows = GOLD[f"draws{cols}"]
    assert rows.shape[0] >= 50
    for seed, row in enumerate(rows):
        flags, taken, angle, scale, calls = unpack(row)
        rng = CountingRandom(seed)
        got = data.draw_detection_augmentation(oriented=cols == 7, rng=rng, **D.PROBS)
        assert got == (flags, angle, scale), (seed, got, row)
        assert rng.calls == calls == (3 if cols == 6 else (6 if taken else 4))
        assert taken == ((angle, scale) != (0.0, 1.0))
    assert {bool(r[1]) for r in GOLD["draws7"]} == {True, False} and not GOLD["draws6"][:, 1].any()


def test_draw_rejects_probabilities_outside_the_unit_interval():
    from nerf_mae_amd import data
    with pytest.raises(ValueError, match="flip_prob must be between 0 and 1"):
        data.draw_detection_augmentation(1.5, 0.5, 0.5, True)
    with pytest.raises(ValueError, match="rotate_prob must be between 0 and 1"):
        data.draw_detection_augmentation(0.5, -0.1, 0.5, True)
    with pytest.raises(ValueError, match="rotate_and_scale_prob must be between 0 and 1"):
        data.draw_detection_augmentation(0.5, 0.5, 1.01, False)
    assert data.draw_detection_augmentation(0.0, 0.0, 0.0, True) == (0, 0.0, 1.0)
    flags, angle, scale = data.draw_detection_augmentation(1.0, 1.0, 1.0, True, random.Random(0))
    assert flags == 7 and abs(angle) <= np.pi / 18 and 0.9 <= scale <= 1.1


def test_header_declares_the_entry_points():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    assert [t for t, _ in sigs["nmh_grid_prepare_rs"][1]][-3:] == ["float", "float", "void*"]
    assert [n for _, n in sigs["nmh_grid_prepare_rs"][1]][:-3] == [n for _, n in sigs["nmh_grid_prepare"][1]][:-1]
    assert "nmh_boxes_augment" in sigs
