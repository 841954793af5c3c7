"""The voxel heads' input pipeline without a GPU: the numpy restatement of the paired transform (tests/_voxel_input_ref.py) against the same torch calls the
reference makes, the class weights against the reference's own results (golden g28, tools/gen_golden_voxel_train.py), the C ABI entry, and the draw order of
data.VoxelBatcher."""
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _voxel_common as V  # noqa: E402
from tests import _voxel_input_ref as P  # noqa: E402


@pytest.mark.parametrize("flags", range(8))
def test_restatement_equals_the_reference_torch_calls(flags):
    """datasets.py:200-201 and :222 on a (1,W,L,H) tensor: transpose(1, 2) + flip(1), flip(1), flip(2), in that order; then the zero padding"""
    W, L, H, R = 5, 7, 3, 8
    vol = np.arange(1, W * L * H + 1, dtype=np.int64).reshape(W, L, H)          # every voxel its own value, none 0
    t = torch.from_numpy(vol)[None]
    if flags & P.ROT:
        t = torch.transpose(t, 1, 2)
        t = torch.flip(t, [1])
    if flags & P.FLIP0:
        t = torch.flip(t, [1])
    if flags & P.FLIP1:
        t = torch.flip(t, [2])
    assert list(t.shape[1:]) == P.extents((W, L, H), flags)
    want = torch.zeros((R, R, R), dtype=torch.float32)
    want[:t.shape[1], :t.shape[2], :t.shape[3]] = t[0].float()
    got = P.labels_ref(vol, R, flags)
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())
    # the channels-last grid takes the same transform on every channel
    scene = np.stack([vol % 251, (vol * 3) % 251, (vol * 7) % 251, (vol * 11) % 251], -1).astype(np.uint8)
    g = P.grid_ref(scene, R, flags)
    assert g.shape == (4, R, R, R)
    for c in range(4):
        assert np.array_equal(g[c], P.labels_ref(scene[..., c], R, flags) * P.INV255)


@pytest.mark.parametrize("case", V.CLASS_WEIGHT_CASES, ids=[c[0] for c in V.CLASS_WEIGHT_CASES])
def test_class_weights_match_the_reference(case):
    """float64 numpy on both sides and the same three operations (divide, log, reciprocal): rtol 1e-12"""
    from nerf_mae_amd.sem_eval import class_weights_from_counts
    name, K, seed, shapes, absent = case
    g = np.load(V.GOLD_WEIGHTS)
    assert int(g[f"{name}.classes"]) == K and int(g[f"{name}.seed"]) == seed and g[f"{name}.shapes"].tolist() == [list(s) for s in shapes]
    counts = sum(np.bincount(v.reshape(-1), minlength=K) for v in V.class_weight_labels(case))
    counts[0] = 0
    assert np.array_equal(counts.astype(np.float64), g[f"{name}.counts"])          # the volumes are the ones the reference saw
    if absent is not None:
        assert counts[absent] == 0
    w = class_weights_from_counts(counts, c=float(g[f"{name}.c"]))
    assert w.dtype == np.float64 and w[0] == 0
    err = np.abs(w - g[f"{name}.weights"]).max() / np.abs(g[f"{name}.weights"]).max()
    V.print_err(f"  [class weights {name}] largest relative deviation {err:.2e}")
    np.testing.assert_allclose(w, g[f"{name}.weights"], rtol=1e-12, atol=0)
    # entry 0 of the histogram is ignored whatever it holds (metrics.py:414)
    counts[0] = 12345
    np.testing.assert_allclose(class_weights_from_counts(counts), g[f"{name}.weights"], rtol=1e-12, atol=0)


def test_an_all_zero_histogram_raises():
    from nerf_mae_amd.sem_eval import class_weights_from_counts
    with pytest.raises(ValueError):
        class_weights_from_counts(np.zeros(19))
    with pytest.raises(ValueError):
        class_weights_from_counts([7] + [0] * 18)          # only unlabelled voxels


def test_header_declares_and_capi_defines_labels_prepare():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    assert "nmh_labels_prepare" in sigs
    ret, args = sigs["nmh_labels_prepare"]
    assert ret == "int" and [n for _, n in args] == ["dt", "src", "W", "L", "H", "dst", "R", "flags", "stream"]
    assert [n for _, n in args][1:] == [n for _, n in sigs["nmh_grid_prepare"][1]][1:]          # the scene kernel's arguments behind the dtype code
    capi = open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "capi.hip")).read()
    assert "int nmh_labels_prepare(int dt, const void* src, int W, int L, int H, float* dst, int R, int flags, void* stream) {" in capi
    assert "k_labels_prepare" in open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "kernels.hpp")).read()


def test_voxel_batcher_draws_through_draw_augmentation():
    from nerf_mae_amd import data
    b = data.VoxelBatcher(8, "cuda:0", flip_prob=0.5, rotate_prob=0.3)          # (no device call before the first prepare)
    for seed in range(20):
        a, c = random.Random(seed), random.Random(seed)
        assert b.draw_flags(3, a) == [data.draw_augmentation(0.5, 0.3, c) for _ in range(3)]
        assert a.random() == c.random()          # and nothing else was drawn
    assert data.VoxelBatcher(8, "cuda:0").draw_flags(4, random.Random(0)) == [0, 0, 0, 0]
    with pytest.raises(ValueError):
        data.VoxelBatcher(8, "cuda:0", target="boxes")


def test_voxel_trainer_refusals_need_no_gpu():
    from nerf_mae_amd.trainer import VoxelTrainer
    with pytest.raises(TypeError):
        VoxelTrainer(torch.nn.Linear(2, 2), [None], [None])
