"""CPU: the float64 restatement of the voxel-semantics evaluation (tests/_sem_eval_ref.py) against tests/golden/g26_sem_eval.npz, recorded from the reference's own
output_metrics by tools/gen_golden_sem_eval.py: counts and label volumes exactly, the two loss scalars and the evaluation loop's five numbers to 1e-6 (the
recording is fp32).  And the surface of the feature: the head has `output_metrics`, the package exports the evaluator, CPU tensors raise, the header declares
the entries."""
import numpy as np
import pytest
import torch

from tests import _sem_eval_ref as S

TOL = 1e-6


@pytest.fixture(scope="module")
def g26(golden):
    return golden("g26_sem_eval.npz")


@pytest.fixture(scope="module")
def restated():
    out = {}
    for case in S.GOLDEN_CASES:
        logits, labels, cw, ties = S.inputs(case)
        assert not ties.any() and S.argmax_margin(logits) >= S.MARGIN
        out[case[0]] = (logits, labels, cw, S.sem_eval(logits, labels, cw))
    return out


@pytest.mark.parametrize("case", S.GOLDEN_CASES, ids=lambda c: c[0])
def test_restatement_equals_the_recording(case, g26, restated):
    name = case[0]
    logits, labels, cw, r = restated[name]
    sums = np.array([logits.double().sum().item(), labels.double().sum().item(), 0.0 if cw is None else cw.double().sum().item()])
    np.testing.assert_allclose(sums, g26[f"{name}.input_sums"], rtol=1e-12, err_msg="the seeded inputs are not the recorded ones")
    want = {key: g26[f"{name}.{key}"] for key in ("intersection", "union", "target")}
    if case[1] == 2:
        # K = 2: the reference's histc(bins=1, min=1, max=1) has an empty range, which ATen widens to [0, 2], so its one area_pred bin also takes the labelled
        # voxels predicted as class 0 (a stated deviation: here area_pred[1] = #(p == 1)).  The recording is that much larger, exactly.
        pred0 = int(((r["pred_vis"] == 0) & (r["target_vis"] > 0)).sum())
        assert pred0 > 0
        want["union"] = want["union"] - pred0
    for row, key in enumerate(("intersection", "union", "target")):
        assert np.array_equal(r["counts"][row], want[key]), key
    assert r["counts"][2].sum() > 0 and r["counts"][0].sum() > 0
    assert np.array_equal(S.checksum(r["pred_vis"]), g26[f"{name}.pred_vis_sums"])
    assert np.array_equal(S.checksum(r["target_vis"]), g26[f"{name}.target_vis_sums"])
    for got, key in ((r["ce"], "ce"), (r["miou"], "iou_val")):
        want = float(g26[f"{name}.{key}"])
        assert abs(got - want) <= TOL * abs(want), f"{key}: {got!r} vs {want!r}"


def _assert_loop(got, g26):
    for key in ("iou_class", "accuracy_class", "mIoU", "mAcc", "allAcc"):
        np.testing.assert_allclose(np.asarray(got[key], np.float64), g26[f"loop.{key}"], rtol=TOL, atol=0, err_msg=key)


def test_evaluator_formulas_equal_the_recorded_loop(g26, restated):
    tot = sum(restated[n][3]["counts"] for n in S.EVAL_SEQUENCE)
    _assert_loop(S.evaluator_numbers(tot[0], tot[1], tot[2]), g26)
    acc = [S.batch_accuracy(restated[n][3]["counts"][0], restated[n][3]["counts"][2]) for n in S.EVAL_SEQUENCE]
    np.testing.assert_allclose(acc, g26["loop.accuracy"], rtol=TOL)
    assert len({restated[n][0].shape[0] for n in S.EVAL_SEQUENCE}) == 3, "three batches of different size"


def test_the_package_has_the_feature(g26, restated):
    """fails without the feature: the class had no output_metrics and the package no SemanticEvaluator"""
    from nerf_mae_amd import SemanticEvaluator, intersection_and_union, sem_eval_dense  # noqa: F401
    from nerf_mae_amd.heads import SwinTransformer_VoxelSemantics_Pretrained_Skip
    assert callable(getattr(SwinTransformer_VoxelSemantics_Pretrained_Skip, "output_metrics", None))
    ev = SemanticEvaluator(19)
    for n in S.EVAL_SEQUENCE:     # update_counts and compute() are plain tensor arithmetic: they run wherever the counts live
        c = torch.from_numpy(restated[n][3]["counts"])
        m = dict(intersection=c[0], union=c[1], target=c[2])
        ev.update_counts(m)
        assert abs(float(SemanticEvaluator.accuracy(m)) - S.batch_accuracy(c[0].numpy(), c[2].numpy())) < 1e-15
    assert ev.totals.dtype == torch.int64 and tuple(ev.totals.shape) == (3, 18)
    _assert_loop(ev.compute(), g26)
    ev.reset()
    assert int(ev.totals.abs().sum()) == 0
    with pytest.raises(ValueError):
        SemanticEvaluator(33)


def test_output_metrics_on_cpu_tensors_raises():
    from nerf_mae_amd import SemanticEvaluator, intersection_and_union
    from nerf_mae_amd.heads import SwinTransformer_VoxelSemantics_Pretrained_Skip
    torch.manual_seed(0)
    head = SwinTransformer_VoxelSemantics_Pretrained_Skip(resolution=32, out_channels=5, is_eval=True)
    labels, pred = [torch.ones((1, 32, 32, 32))], torch.zeros((1, 5, 32, 32, 32))
    with pytest.raises(RuntimeError):
        head.output_metrics(labels, pred)
    with pytest.raises(RuntimeError):
        SemanticEvaluator(5).update(labels, pred)
    with pytest.raises(RuntimeError):
        intersection_and_union(torch.ones(8, dtype=torch.int64), torch.ones(8, dtype=torch.int64), 5)


def test_header_declares_the_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    assert "nmh_sem_eval" in sigs and "nmh_sem_label_counts" in sigs
    names = [n for _, n in sigs["nmh_sem_eval"][1]]
    assert names == ["logits", "labels", "class_weights", "B", "K", "V", "fpart", "ipart", "out", "counts", "pred_vis", "target_vis", "totals", "stream"]
