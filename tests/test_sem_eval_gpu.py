"""GPU: the voxel-semantics evaluation (csrc/heads.hip sem_eval_kernel behind nerf_mae_amd.sem_eval) against the float64 restatement of tests/_sem_eval_ref.py, which
tests/test_sem_eval_ref_cpu.py pins to the reference's own output_metrics.

Counts and both label volumes are integers: EXACT equality on every case, no voxel left out (the restatement asserts an arg-max margin of 1e-3 on every voxel
outside the crafted exact ties, where the rule is the lowest index).  The loss scalars are held to CE_FWD_TOL = 3e-6 relative, the bound of masked_ce_fwd in
tests/test_head_kernels_gpu.py for the same arithmetic.  Measured on an MI355X (NMH_PRINT_ERR=1, pytest -s): DESIGN.md 3.18.

Shapes: see tests/_sem_eval_ref.py.  7x5x3 with B = 2 is less than one workgroup, and its odd V puts the second sample's planes off 16-byte alignment (scalar
path); 30x32x27 and 32^3 with K = 19 are the head's shapes at resolution 32 (two of them the masked-CE cases of tests/_heads_ref.py); K = 2 and K = 32 are the
ends of the class range (K <= 20 and K <= 32 are two instantiations); 104^3 (16-byte loads) and 65^3 (scalar) are the smallest cubes at which some lane
takes a second grid-stride trip under the cap of 1024 workgroups."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import _sem_eval_ref as S

pytestmark = pytest.mark.gpu
CE_FWD_TOL = 3e-6
ALL = {c[0]: c for c in S.CASES + S.HEADS_CASES + S.SECOND_TRIP_CASES + S.BAD_LABEL_CASES + S.GOLDEN_CASES}
WORST = {"ce": 0.0, "iou_val": 0.0}


@functools.lru_cache(maxsize=None)
def _ref(name):
    """(logits, labels, cw, ties, restatement) of a case, computed once and shared; nothing of it is modified"""
    case = ALL[name]
    logits, labels, cw, ties = S.inputs(case)
    assert S.argmax_margin(logits, ties) >= S.MARGIN, name
    return logits, labels, cw, ties, S.sem_eval(logits, labels, cw, scalars=case[6] != "badlabels")


def _dense(name, totals=None, weights=True):
    from nerf_mae_amd import sem_eval_dense
    logits, labels, cw, _, _ = _ref(name)
    return sem_eval_dense(logits.cuda(), labels.cuda(), cw.cuda() if (cw is not None and weights) else None, totals)


def _check(name, got, ref, scalars=True):
    ce, m, pv, tv = got
    torch.cuda.synchronize()
    for row, key in enumerate(("intersection", "union", "target", "area_pred")):
        assert m[key].dtype == torch.int64 and np.array_equal(m[key].cpu().numpy(), ref["counts"][row]), f"{name}: {key} {m[key].tolist()} vs {ref['counts'][row].tolist()}"
    assert pv.dtype == torch.int64 and tv.dtype == torch.int64 and pv.shape == ref["pred_vis"].shape
    assert torch.equal(pv.cpu(), ref["pred_vis"]), f"{name}: pred_labels_vis differs on {(pv.cpu() != ref['pred_vis']).sum().item()} voxels"
    assert torch.equal(tv.cpu(), ref["target_vis"]), f"{name}: target_vis"
    if scalars:
        figs = {"ce": abs(ce.item() - ref["ce"]) / abs(ref["ce"]), "iou_val": abs(m["iou_val"].item() - ref["miou"]) / max(abs(ref["miou"]), 1e-300)}
        for k, v in figs.items():
            WORST[k] = max(WORST[k], v)
        if os.environ.get("NMH_PRINT_ERR"):
            print(f"  [sem_eval {name}] " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()) + f"   worst so far ce {WORST['ce']:.2e}, iou_val {WORST['iou_val']:.2e}")
        for k, v in figs.items():
            assert v <= CE_FWD_TOL, f"{name} {k}: relative error {v:.2e} > {CE_FWD_TOL:g}"


@pytest.mark.parametrize("name", [c[0] for c in S.CASES + S.HEADS_CASES + S.SECOND_TRIP_CASES])
def test_counts_volumes_and_loss_scalars(name):
    ref = _ref(name)[4]
    assert ref["counts"][0].sum() > 0 and ref["counts"][2].sum() > ref["counts"][0].sum()
    _check(name, _dense(name), ref)


def test_crafted_cases_hold_what_they_claim():
    """the properties the crafted cases are there for, asserted from the restatement (and the kernel agrees with it: test_counts_volumes_and_loss_scalars)"""
    r = _ref("K19-cw-s1-8-B3-blank1")
    assert (r[1][1] == 0).all() and (r[1][0] > 0).any(), "a sample with no labelled voxel"
    c = _ref("K5-cw-s4-8-B2-absent3")[4]["counts"]
    assert c[2][2] == 0 and c[3][2] == 0 and c[1][2] == 0 and c[2][0] > 0, "class 3 absent from prediction and target"
    r = _ref("K19-cw-s1-10-B2-pred0")[4]
    p0 = int(((r["pred_vis"] == 0) & (r["target_vis"] > 0)).sum())
    assert p0 > 100 and r["counts"][3].sum() + p0 == r["counts"][2].sum(), "labelled voxels predicted as class 0 enter no area_pred bin"
    for name in ("K8-nocw-s1-11x6x5-B2-ties", "K19-cw-s1-12-B2-ties"):
        logits, labels, _, ties, r = _ref(name)
        top = logits.topk(3, dim=1).values
        assert ties.sum() > 50 and (top[:, 0] == top[:, 1])[ties].all() and (top[:, 0] == top[:, 2])[ties].any() and ((logits[:, 0] == top[:, 0]) & ties).any()
        assert ((r["pred_vis"] > 0) & ties).any() and (ties & (labels > 0)).any()


@pytest.mark.parametrize("name", [c[0] for c in S.BAD_LABEL_CASES])
def test_labels_equal_to_K_and_255_leave_the_valid_classes_unchanged(name):
    """a label >= K is a labelled voxel of no class: exact counts against the restatement, and I and T equal those of the same inputs with these voxels unlabelled"""
    logits, labels, cw, _, ref = _ref(name)
    K = ALL[name][1]
    assert (labels == K).any() and (labels == 255).any()
    got = _dense(name)
    _check(name, got, ref, scalars=False)
    assert torch.isfinite(got[0]) and torch.isfinite(got[1]["iou_val"])
    from nerf_mae_amd import sem_eval_dense
    clean = labels.clone()
    clean[clean >= K] = 0.0
    m = sem_eval_dense(logits.cuda(), clean.cuda(), None if cw is None else cw.cuda())[1]
    assert torch.equal(m["intersection"], got[1]["intersection"]) and torch.equal(m["target"], got[1]["target"])
    assert (got[1]["area_pred"] >= m["area_pred"]).all() and (got[1]["area_pred"] > m["area_pred"]).any()


def test_class_weights_none_and_given():
    name = "K19-cw-s4-30x32x27-B2"
    logits, labels, cw, _, ref = _ref(name)
    import tests._heads_ref as HR
    plain = HR.masked_ce(logits, labels, None)
    ce, m, _, _ = _dense(name, weights=False)
    assert abs(ce.item() - float(plain["ce"])) <= CE_FWD_TOL * float(plain["ce"])
    assert abs(float(plain["ce"]) - ref["ce"]) > 1e-3 * ref["ce"], "the weights matter in this case"
    assert np.array_equal(m["intersection"].cpu().numpy(), ref["counts"][0])


def test_k_outside_2_to_32_is_rejected():
    from nerf_mae_amd import intersection_and_union, sem_eval_dense
    from nerf_mae_amd._lib import NmhError
    for K in (1, 33):
        with pytest.raises(NmhError):
            sem_eval_dense(torch.zeros((1, K, 8), device="cuda"), torch.zeros((1, 8), device="cuda"))
        with pytest.raises(NmhError):
            intersection_and_union(torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda"), K)


def test_evaluator_three_updates_equal_one_restatement():
    from nerf_mae_amd import SemanticEvaluator
    names = S.EVAL_SEQUENCE
    refs = [_ref(n) for n in names]
    assert len({r[0].shape[0] for r in refs}) == 3
    ev = SemanticEvaluator(19, class_weights=refs[0][2])
    ev.totals = torch.full((3, 18), 2 ** 40, dtype=torch.int64, device="cuda")      # a preset far past fp32's integers comes back exact
    want = np.full((3, 18), 2 ** 40, dtype=np.int64)
    for n, r in zip(names, refs):
        got = ev.update([r[1][b][None] for b in range(r[1].shape[0])], r[0].cuda())
        want += r[4]["counts"][:3]
        acc = SemanticEvaluator.accuracy(got[1])
        assert acc.dtype == torch.float64 and abs(acc.item() - S.batch_accuracy(r[4]["counts"][0], r[4]["counts"][2])) < 1e-15
    assert ev.totals.dtype == torch.int64 and np.array_equal(ev.totals.cpu().numpy(), want)
    ev.reset()
    assert int(ev.totals.abs().sum()) == 0
    for n, r in zip(names, refs):
        ev.update(r[1].cuda(), r[0].cuda())
    total = sum(r[4]["counts"] for r in refs)
    assert np.array_equal(ev.totals.cpu().numpy(), total[:3])
    out, one = ev.compute(), S.evaluator_numbers(total[0], total[1], total[2])
    for key in one:
        assert np.array_equal(np.asarray(out[key]), np.asarray(one[key])), key


def test_evaluator_compute_matches_the_recorded_loop(golden):
    from nerf_mae_amd import SemanticEvaluator
    g = golden("g26_sem_eval.npz")
    ev = SemanticEvaluator(19)
    for n in S.EVAL_SEQUENCE:
        logits, labels, cw, _, _ = _ref(n)
        ev.class_weights = cw
        ce, m, _, _ = ev.update(labels.cuda(), logits.cuda())
        tol = CE_FWD_TOL + 1e-6      # the kernel's bound against float64 plus the 1e-6 within which the float64 restatement meets the fp32 recording
        assert abs(ce.item() - float(g[f"{n}.ce"])) <= tol * float(g[f"{n}.ce"]) and abs(m["iou_val"].item() - float(g[f"{n}.iou_val"])) <= tol * float(g[f"{n}.iou_val"])
    out = ev.compute()
    for key in ("iou_class", "accuracy_class", "mIoU", "mAcc", "allAcc"):
        np.testing.assert_allclose(np.asarray(out[key], np.float64), g[f"loop.{key}"], rtol=1e-12, atol=0, err_msg=key)
    assert 0.1 < out["mIoU"] < out["mAcc"] < 1.0


@pytest.mark.parametrize("name", ["K19-cw-s4-30x32x27-B2", "K5-cw-s2-7x5x3-B2", "K19-cw-s1-12-B2-badlabels"])
def test_labels_only_entry_agrees_with_the_fused_counts(name):
    from nerf_mae_amd import intersection_and_union
    logits, labels, _, _, ref = _ref(name)
    K = ALL[name][1]
    pred = S.predicted(logits)
    for dt in (torch.int64, torch.int32, torch.float32):
        I, U, T = intersection_and_union(pred.to(dt).cuda(), labels.to(dt).cuda(), K)
        torch.cuda.synchronize()
        for got, row in ((I, 0), (U, 1), (T, 2)):
            assert got.dtype == torch.int64 and tuple(got.shape) == (K - 1,) and np.array_equal(got.cpu().numpy(), ref["counts"][row]), (name, dt, row)
    I, U, T = intersection_and_union(pred.cuda(), labels.cuda(), K)      # integer output with fp32 target, and a shape that is not flat
    assert np.array_equal(U.cpu().numpy(), ref["counts"][1])


def _no_sync(fn):
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        return fn()
    finally:
        torch.cuda.set_sync_debug_mode(mode)


def _flat(got):
    ce, m, pv, tv = got
    return [ce, m["iou_val"], m["intersection"], m["union"], m["target"], m["area_pred"], pv, tv]


def test_no_host_synchronisation_determinism_and_capture():
    from nerf_mae_amd import SemanticEvaluator
    name = "K19-cw-s4-30x32x27-B2"
    logits, labels, cw, _, ref = _ref(name)
    ld, bd = logits.cuda(), labels.cuda()
    ev = SemanticEvaluator(19, class_weights=cw.cuda())
    ev.update(bd, ld)                                    # the totals are made on the first call
    first = _no_sync(lambda: ev.update(bd, ld))
    second = _no_sync(lambda: ev.update(bd, ld))
    torch.cuda.synchronize()
    _check(name, first, ref)
    for a, b in zip(_flat(first), _flat(second)):
        assert torch.equal(a, b) and (a.dtype != torch.float32 or torch.equal(a.view(torch.int32), b.view(torch.int32))), "two runs are bit-identical in every output"
    assert np.array_equal(ev.totals.cpu().numpy(), 3 * ref["counts"][:3])
    ev.reset()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sl, sb = torch.zeros_like(ld), torch.zeros_like(bd)
        ev.update(sb, sl)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = ev.update(sb, sl)
    sl.copy_(ld)
    sb.copy_(bd)
    ev.reset()
    for k in (1, 2):
        graph.replay()
        torch.cuda.synchronize()
        assert np.array_equal(ev.totals.cpu().numpy(), k * ref["counts"][:3]), f"replay {k} adds the eager counts once more"
        for a, b in zip(_flat(out), _flat(first)):
            assert torch.equal(a, b)


def test_output_metrics_of_the_head_end_to_end():
    """the head at resolution 32 with the g15 initialisation: forward, then output_metrics on its own logits == the restatement applied to those logits"""
    from oracle.gen_golden_heads import K, R, inputs, sem_labels
    from tests.test_heads import _hip_heads
    _, se, _, _ = _hip_heads(torch.float32)
    se.eval()
    xs, labs = [t.cuda() for t in inputs()], [t.cuda() for t in sem_labels()]
    with torch.no_grad():
        pred = se(xs)
        loss, _, iou = se.loss_fn(labs, pred)
        got = _no_sync(lambda: se.output_metrics(labs, pred))
    torch.cuda.synchronize()
    ce, m, pv, tv = got
    assert set(m) >= {"intersection", "union", "target", "iou_val"} and tuple(pv.shape) == (2, R, R, R) and tuple(tv.shape) == (2, R, R, R)
    dense = torch.zeros((2, R, R, R))
    for i, t in enumerate(sem_labels()):
        dense[i, :t.shape[1], :t.shape[2], :t.shape[3]] = t[0]
    ref = S.sem_eval(pred.cpu(), dense, se.class_weights)     # (the arg-max of given fp32 numbers is exact arithmetic: no margin is needed between the two)
    _check("head-R32", got, ref)
    assert ref["counts"][2].sum() > 10000 and (dense[1, 30:] == 0).all() and (tv[1, 30:] == 0).all()
    assert abs(ce.item() - loss.item()) <= 2 * CE_FWD_TOL * abs(loss.item()) and abs(m["iou_val"].item() - iou.item()) <= 2 * CE_FWD_TOL * abs(iou.item())
