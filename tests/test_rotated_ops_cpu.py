"""Host-side checks of the rotated RoIAlign / vertex sort ops: the C ABI declares them, the Python module imports without a GPU and refuses
CPU tensors, and the float64 restatement that the GPU tests are measured against (tests/_rotated_ref.py) reproduces analytic results."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rotated_ref as R  # noqa: E402

NAMES = ("nmh_roi_align_rotated_3d_fwd", "nmh_roi_align_rotated_3d_bwd", "nmh_sort_vertices")


def test_header_declares_the_rotated_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    for n in NAMES:
        assert n in sigs, n
        ret, args = sigs[n]
        assert ret == "int" and args[-1] == ("void*", "stream"), (n, ret, args[-1])
    for n in NAMES[:2]:
        assert [a for _, a in sigs[n][1][:2]] == ["layout", "dt"]
    assert [t for t, _ in sigs["nmh_sort_vertices"][1][:4]] == ["const float*", "const unsigned char*", "const int*", "int*"]


def test_rotated_module_imports_and_refuses_cpu_tensors():
    from nerf_mae_amd import rotated
    x = torch.zeros(1, 8, 4, 4, 4)
    rois = torch.tensor([[0.0, 2, 2, 2, 2, 2, 2, 0]])
    with pytest.raises(RuntimeError):
        rotated.roi_align_rotated_3d(x, rois, (2, 2, 2), 1.0, 0)
    with pytest.raises(RuntimeError):
        rotated.ROIAlignRotated3D((2, 2, 2), 0)(x, rois, 1.0)
    with pytest.raises(RuntimeError):
        rotated.roi_align_rotated_3d_channels_last(x.permute(0, 2, 3, 4, 1).contiguous(), rois, (2, 2, 2), 1.0, 2)
    with pytest.raises(RuntimeError):
        rotated.sort_v(torch.zeros(1, 1, 24, 2), torch.zeros(1, 1, 24, dtype=torch.bool), torch.zeros(1, 1, dtype=torch.int32))


def test_restatement_constant_map():
    """a constant map gives the constant in every bin whose samples all lie inside; rotation, scale and grid do not matter"""
    x = torch.full((2, 10, 12, 14, 3), 2.5, dtype=torch.float64)
    rois = torch.tensor([[1.0, 10, 12, 14, 8, 6, 10, 33.0], [0.0, 9, 11, 13, 5, 9, 7, -120.0]])
    for sr in (2, 0):
        out, meta = R.roi_align_ref(x, rois, (3, 2, 4), 0.5, sr)
        assert meta["outside"] == 0.0
        assert torch.allclose(out, torch.full_like(out, 2.5), rtol=0, atol=1e-13)


def test_restatement_linear_map():
    """trilinear interpolation reproduces a linear map, and the mean of a linear function over a symmetric sample grid is its value at the
    bin centre: an unrotated ROI inside the map gives a x + b y + c z at the centre of each bin"""
    W, L, H = 10, 12, 14
    a, b, c = 0.7, -1.3, 0.4
    gx, gy, gz = torch.meshgrid(torch.arange(W, dtype=torch.float64), torch.arange(L, dtype=torch.float64), torch.arange(H, dtype=torch.float64), indexing="ij")
    x = (a * gx + b * gy + c * gz)[None, ..., None]
    scale, pooled = 0.5, (3, 2, 4)
    roi = [0.0, 9.0, 12.4, 13.0, 9.0, 13.0, 11.0, 0.0]       # scaled: centre (4.5, 6.2, 6.5), size (4.5, 6.5, 5.5): inside [0, extent - 1]
    rois = torch.tensor([roi])
    roi = rois.double().tolist()[0]                           # the fp32 values the op is given
    for sr in (2, 0):
        out, meta = R.roi_align_ref(x, rois, pooled, scale, sr)
        assert meta["outside"] == 0.0
        for pw in range(3):
            for pl in range(2):
                for ph in range(4):
                    ctr = [roi[1 + k] * scale - roi[4 + k] * scale / 2 + (p + 0.5) * roi[4 + k] * scale / pooled[k] for k, p in enumerate((pw, pl, ph))]
                    want = a * ctr[0] + b * ctr[1] + c * ctr[2]
                    assert abs(out[0, pw, pl, ph, 0].item() - want) < 1e-12, (sr, pw, pl, ph)


def test_restatement_rotation_quarter_turn():
    """a quarter turn maps ROI-local (xx, yy) to (yy, -xx): on the map f = y the pooled value is -xx at the bin centre plus the centre's y"""
    W = L = H = 16
    gy = torch.arange(L, dtype=torch.float64)[None, :, None].expand(W, L, H)
    x = gy[None, ..., None]
    roi = [0.0, 8.0, 7.0, 8.0, 6.0, 4.0, 4.0, 90.0]
    out, _ = R.roi_align_ref(x, torch.tensor([roi]), (3, 2, 2), 1.0, 2)
    for pw in range(3):
        xx = -3.0 + (pw + 0.5) * 2.0
        assert torch.allclose(out[0, pw, :, :, 0], torch.full((2, 2), 7.0 - xx, dtype=torch.float64), atol=1e-12)


def test_vertex_sort_restatement_on_a_known_pair():
    """unit square against the same square shifted by (0.5, 0.5): the intersection is the square [0, 0.5]^2, area 0.25"""
    c1 = R.rect_corners(0.0, 0.0, 1.0, 1.0, 0.0)
    c2 = R.rect_corners(0.5, 0.5, 1.0, 1.0, 0.0)
    v, m = R.box_pair_vertices(c1, c2)
    assert m.sum() == 4
    ctr = v[m].mean(0)
    idx = R.sort_vertices_ref((v - ctr)[None, None], m[None, None], np.array([[4]]))[0, 0]
    assert idx[4] == idx[0] and len(set(idx[:4])) == 4 and all(i >= 8 and not m[i] for i in idx[5:])
    assert abs(R.shoelace(v[idx[:4]]) - 0.25) < 1e-15
    assert abs(R.clip_area(c1, c2) - 0.25) < 1e-15
    assert math.isclose(R.clip_area(R.rect_corners(0, 0, 2, 1, 0.3), R.rect_corners(0, 0, 2, 1, 0.3)), 2.0, rel_tol=1e-12)
