"""The float64 restatement of the "interpolation" RoI feature type (tests/_roi_interp_ref.py) against the recorded reference (tests/golden/g31_roi_interp.npz,
written by tools/gen_golden_roi_interp.py from nerf_rpn/model/detector.py on the CPU in float64) and against F.interpolate; the conditions on the inputs of
tests/test_roi_interp_gpu.py, asserted from the restatement; the constructor's behaviour.  No GPU.

Continuous results agree to 1e-9 relative to the largest recorded entry (both sides are float64 arithmetic on the same fp32 inputs), the bound
tests/test_roi_head_ref_cpu.py holds the pooling restatement to."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _roi_head_ref as H  # noqa: E402
from tests import _roi_interp_ref as I  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g31_roi_interp.npz"))
G22 = np.load(os.path.join(ROOT, "tests", "golden", "g22_roi_head.npz"))


def close(a, b, name):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= 1e-9, f"{name}: {err:.3e}"


def sampled():
    rois, gts, labs, maps = H.gold_inputs(True)
    L, Ro, Gr, _ = H.targets(rois, gts, labs, keep=GOLD["keep"], n_fg=GOLD["n_fg"])
    return maps, torch.stack(L), torch.stack(Ro), torch.stack(Gr)


def test_inputs_and_kept_rows_are_the_recorded_ones():
    rois, gts, _, maps = H.gold_inputs(True)
    assert tuple(GOLD["seeds"]) == H.GOLD_SEED[True] and tuple(GOLD["out"]) == H.GOLD["out"]
    close(H.input_sums(rois, gts, maps), GOLD["input_sums"], "input sums")
    assert np.array_equal(GOLD["keep"], G22["o_keep"]) and np.array_equal(GOLD["n_fg"], G22["o_n_fg"]), "the kept rows of the recorded pooling run"
    assert np.array_equal(GOLD["sample_labels"], G22["o_sample_labels"])


def test_features_against_the_recorded_reference():
    maps, _, Ro, _ = sampled()
    out, m, _ = I.interp(maps, Ro, out=H.GOLD["out"])
    assert m["floor"] >= I.MARGIN, m
    assert m["axes_gt"] > 0 and m["axes_lt"] + m["axes_eq"] > 0, "grids both larger than and not larger than the output"
    close(out.numpy(), GOLD["pooled"], "interpolated features")
    assert not np.allclose(GOLD["pooled"], G22["o_pooled"], rtol=1e-2, atol=0), "the recorded features differ from the max-pooled ones"


def test_head_losses_targets_and_decode_against_the_recorded_reference():
    maps, L, Ro, Gr = sampled()
    ex = Ro[..., 1:].reshape(-1, 7).clone()
    ex[:, 3:6] *= 1 + H.ENLARGE            # with remap off the reference encodes against the enlarged RoIs, whatever the feature type
    close(ex.numpy(), GOLD["encoded_rois"], "the RoIs the reference encoded against")
    pooled, _, _ = I.interp(maps, Ro, out=H.GOLD["out"])
    hp = {k: v.double() for k, v in H.gold_head(True).items()}
    x = pooled.reshape(pooled.shape[0], -1)
    deltas, scores = x @ hp["RCNN_bbox_pred_w"].T + hp["RCNN_bbox_pred_b"], x @ hp["RCNN_cls_score_w"].T + hp["RCNN_cls_score_b"]
    r = H.loss(scores, deltas, L.reshape(-1), ex, Gr.reshape(-1, 7), True)
    close(r["targets"].numpy(), GOLD["targets"], "regression targets")
    close([r["obj"].item(), r["reg"].item()], GOLD["losses"], "losses")
    boxes, _ = H.decode(deltas, ex, True)
    close(boxes.numpy(), GOLD["proposals"], "decoded proposals")
    close(torch.softmax(scores, 1).numpy(), GOLD["cls_prob"], "cls_prob")


@pytest.mark.parametrize("out", [(1, 1, 1), (2, 2, 2), (3, 2, 1), (5, 4, 3), (7, 7, 7)], ids=lambda o: "x".join(map(str, o)))
def test_resampling_rule_is_f_interpolate_s(out):
    """grid sizes {1,2,3,5,7} x {1,2,4} x {1,3,6}: below, at and above every output size, and single points"""
    g = torch.Generator().manual_seed(2)
    worst = 0.0
    for gx in (1, 2, 3, 5, 7):
        for gy in (1, 2, 4):
            for gz in (1, 3, 6):
                grid = torch.randn((3, gx, gy, gz), generator=g, dtype=torch.float64)
                want = F.interpolate(grid[None], size=out, mode="trilinear", align_corners=True)[0]
                worst = max(worst, float((I.resample(grid, out) - want).abs().max()))
    assert worst <= 1e-13, worst                 # float64 rounding of at most 8 products of values of order 1: a few 1e-16


def test_resampling_adjoint_is_autograd_s():
    g = torch.Generator().manual_seed(4)
    for size, out in (((5, 2, 6), (3, 2, 1)), ((2, 4, 1), (7, 7, 7)), ((1, 1, 1), (2, 2, 2))):
        grid = torch.randn((2, *size), generator=g, dtype=torch.float64, requires_grad=True)
        dout = torch.randn((2, *out), generator=g, dtype=torch.float64)
        (F.interpolate(grid[None], size=out, mode="trilinear", align_corners=True)[0] * dout).sum().backward()
        assert float((I.resample_adjoint(dout, size) - grid.grad).abs().max()) <= 1e-13


def test_output_size_one_takes_the_grids_corner_and_a_single_point_fills_the_output():
    grid = torch.arange(24, dtype=torch.float64).reshape(1, 2, 3, 4)
    assert I.resample(grid, (1, 1, 1)).item() == 0.0
    assert torch.equal(I.resample(grid[:, 1:, 2:, 3:], (2, 3, 2)), torch.full((1, 2, 3, 2), 23.0, dtype=torch.float64))
    assert torch.equal(I.lerp_axis(3, 5), torch.tensor([[1, 0, 0], [.5, .5, 0], [0, 1, 0], [0, .5, .5], [0, 0, 1]], dtype=torch.float64))


def test_map_gradient_is_autograd_s_on_one_case():
    """the analytic gradient of the restatement against autograd through its own forward"""
    c = I.case("cubic-C5-3x2x1")
    leaves = [m.double().requires_grad_(True) for m in c["maps"]]
    res, _, _ = I.interp(leaves, c["rois"], scales=c["scales"], out=c["out"])
    (res * c["dout"].double()).sum().backward()
    for leaf, want in zip(leaves, c["dmaps"]):
        assert float((leaf.grad - want).abs().max()) <= 1e-9 * max(float(want.abs().max()), 1.0)


@pytest.mark.parametrize("name", I.CASES)
def test_gpu_cases_meet_their_conditions(name):
    c = I.case(name)
    m = c["facts"]
    print(name, {k: v for k, v in m.items() if k != "all_masked_rows"})
    assert m["floor"] >= I.MARGIN, m
    assert m["masked_points"] > 0, "points outside the map are present"
    assert not c["noncubic"] or m["all_masked"] >= 1, "on the non-cubic maps a RoI lies wholly outside its map"
    assert len(m["levels_used"]) == len(c["maps"]), "every level is used"
    assert all(bool((c["res"][r] == 0).all()) for r in m["all_masked_rows"])
    if name == "pool4":
        assert (c["rois"][..., 0] == 3).sum() >= 10 and c["dmaps"][3].abs().sum() > 0


def test_gpu_cases_cover_every_relation_of_grid_and_output_size():
    facts = {n: I.case(n)["facts"] for n in I.CASES}
    for k in ("axes_lt", "axes_eq", "axes_gt", "axes_one"):
        assert sum(f[k] for f in facts.values()) > 0, k
    f = facts["cubic-C5-3x2x1"]
    assert min(f["axes_lt"], f["axes_eq"], f["axes_gt"], f["axes_one"]) > 0, "one case has all four"
    assert all(facts[n]["axes_eq"] == 0 and facts[n]["axes_gt"] == 0 for n in I.CASES if "7x7x7" in n), "output (7,7,7): every grid is smaller"
    assert facts["remap"]["axes_lt"] == 0 and facts["remap"]["axes_eq"] == 0, "the remap case: every grid is larger"


def test_exact_zero_case_meets_its_conditions():
    c = I.zeros_case()
    m, R = c["facts"], c["rois"].shape[1]
    assert m["floor"] >= I.MARGIN and m["levels_used"] == {0, 1} and c["distinct_outside"] >= 2, m
    assert {2, 5, R, R + 1} <= set(c["invalid"]) and set(range(R, 2 * R)) <= set(m["all_masked_rows"]) | {R, R + 1}
    assert not c["res"][c["invalid"]].any() and not c["res"][R:].any() and c["res"][:R].abs().sum() > 0
    assert not c["dmaps"][2].any() and all(not d[1].any() for d in c["dmaps"]) and all(d[0].abs().sum() > 0 for d in c["dmaps"][:2])


def test_constructor():
    from nerf_mae_amd import detector as M
    pool = M.ROIPool([2, 2, 2], [2, 4, 8], is_rotated_bbox=True, feature_extracting_type="interpolation")
    assert pool.feature_extracting_type == "interpolation" and pool.is_rotated_bbox
    assert M.ROIPool([2, 2, 2], [2, 4, 8], is_rotated_bbox=True).feature_extracting_type == "pooling"
    with pytest.raises(NotImplementedError, match="oriented"):
        M.ROIPool([2, 2, 2], [2, 4, 8], feature_extracting_type="interpolation")
    for bad in ("Interpolation", "max", ""):
        with pytest.raises(ValueError):
            M.ROIPool([2, 2, 2], [2, 4, 8], is_rotated_bbox=True, feature_extracting_type=bad)
    with pytest.raises(NotImplementedError):
        M.ROIPool([2, 2, 2], [2, 4, 8], is_rotated_bbox=True, feature_extracting_type="interpolation", use_cuda=True)
