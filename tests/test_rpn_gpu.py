"""RPN anchor target assignment, sampling and losses on the GPU (nerf_mae_amd.rpn over csrc/rpn.hip) against the float64 restatement of
tests/_rpn_ref.py (itself checked against the recorded reference, tests/golden/g20_rpn_targets.npz, in tests/test_rpn_ref_cpu.py).

Tolerance: the project's contract for fp32, assert_close(rtol=1e-3).  Labels and matched indices are compared exactly; that is defined because every
scene used here has a margin of at least 1e-3 on every decision (asserted before each comparison), against an fp32 error of about 1e-6 on an IoU,
or has integer coordinates, where equal IoUs are equal in any precision.  Measured on an MI355X (NMH_PRINT_ERR=1): DESIGN.md 3.11.

Every sampled-set comparison injects the recorded flags; the built-in sampler is checked for its counts, its classes, its determinism and its
uniformity: 64 identical scenes x 8 fixed counters = 512 draws of 8 out of 40 candidates, every candidate's selection count within 6 standard
deviations of Binomial(512, 0.2) (about 102 +- 54: a false alarm needs a 6-sigma event among 40 counts, and the seeds are fixed)."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (mesh, grids, boxes per scene, original sizes or None, anchor levels, scene seed per rotated); seeds by the search of tools/gen_golden_rpn.py
GEOMS = {
    "g20": (R.MESH, R.GRIDS, R.NBOX, R.ORI, 4, R.SEED),
    "non-cubic": ((32, 24, 16), ((8, 6, 4), (4, 3, 2), (2, 1, 1)), (3, 2), ((32, 24, 16), (27, 17, 13)), 3, {False: 1, True: 0}),
    "one-scene": (R.MESH, R.GRIDS, (3,), None, 4, {False: 163, True: 292}),
    "mesh-64": ((64, 64, 64), ((16, 16, 16), (8, 8, 8), (4, 4, 4), (2, 2, 2)), (2,), None, 4, {False: 1318}),
    "mesh-64-one-box": ((64, 64, 64), ((16, 16, 16), (8, 8, 8), (4, 4, 4), (2, 2, 2)), (1,), None, 4, {True: 32}),
}
ASSIGN_CASES = [(name, rotated) for name, g in GEOMS.items() for rotated in sorted(g[5])]


def _m():
    from nerf_mae_amd import rpn
    return rpn


def _gen(levels=4):
    return _m().AnchorGenerator3D(R.ANCHOR_SIZES[:levels], R.ASPECT_RATIOS[:levels])


@functools.lru_cache(maxsize=None)
def case(name, rotated):
    mesh, grids, nbox, ori, levels, seeds = GEOMS[name]
    boxes = R.make_scene(seeds[rotated], nbox=nbox, mesh=mesh, rotated=rotated, ori=ori)
    a = R.assign(boxes, mesh=mesh, grids=grids, ori=ori, rotated=rotated, base=R.base_anchors()[:levels])
    return boxes, a


def _assign(name, rotated, boxes, **kw):
    mesh, grids, _, ori, levels, _ = GEOMS[name]
    dev_ori = None if ori is None else torch.tensor(ori, dtype=torch.int32).cuda()
    return [t.cpu() for t in _m().rpn_assign_targets(_gen(levels), mesh, grids, [b.cuda() for b in boxes], dev_ori, R.FG, R.BG, rotated=rotated, **kw)]


def _compare(out, a, tag):
    labels, midx, tg = out
    assert labels.dtype == torch.float32 and midx.dtype == torch.int32 and tg.dtype == torch.float32
    assert torch.equal(labels.double(), a["labels"]), f"{tag}: {int((labels.double() != a['labels']).sum())} labels differ"
    assert torch.equal(midx.long(), a["matched"]), f"{tag}: {int((midx.long() != a['matched']).sum())} matched indices differ"
    assert_close(tg, a["targets"], 1e-3, f"{tag} regression_targets")


# ---- 1. assignment -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,rotated", ASSIGN_CASES, ids=lambda v: {False: "aabb", True: "obb"}.get(v, v))
def test_assignment_against_float64(name, rotated):
    boxes, a = case(name, rotated)
    for k, v in R.decision_margins(a).items():
        assert v >= 1e-3, (name, rotated, k, v)
    assert (a["labels"] == 1).sum() > 0 and all((g > 0).all() for g in a["gtmax"])
    _compare(_assign(name, rotated, boxes), a, f"{name} {'obb' if rotated else 'aabb'}")


def test_seventy_boxes_cross_the_lds_stage_and_an_empty_scene():
    # integer boxes: every IoU is a ratio of integers below 2^24, so equal IoUs are equal in fp32 and in float64; the thresholds keep their margin
    rng = np.random.default_rng(416)                       # the first seed whose decisions all have their margin
    lo = rng.integers(0, 24, (70, 3))
    b = torch.from_numpy(np.concatenate([lo, lo + rng.integers(3, 9, (70, 3))], 1).astype(np.float32))
    boxes = [b, torch.zeros((0, 6))]
    a = R.assign(boxes)
    assert a["m_thr"] >= 1e-3 and a["m_gt"] >= 1e-3 and a["m_anc"] >= 1e-3, R.decision_margins(a)
    assert (a["matched"][0] >= 64).sum() > 0, "no anchor matched to a box of the second stage"
    labels, midx, tg = [t.cpu() for t in _m().rpn_assign_targets(_gen(), R.MESH, R.GRIDS, [x.cuda() for x in boxes])]
    _compare((labels, midx, tg), a, "70 boxes")
    assert (labels[1] == 0).all() and (midx[1] == -1).all() and (tg[1] == 0).all()
    # the same empty scene with padding: -1 in the padding, 0 elsewhere
    out = _m().rpn_assign_targets(_gen(), R.MESH, R.GRIDS, [x.cuda() for x in boxes], [(32, 32, 32), (24, 28, 20)])
    valid = torch.from_numpy(R.valid_mask((24, 28, 20)))
    assert torch.equal(out[0][1].cpu(), torch.where(valid, 0.0, -1.0).float())


def test_structural_ties():
    M = _m()
    # a cube of side 4 centred at (14, 12, 12): midway on x between the centres 12 and 16 of two level-0 anchors (cubes of side 8), inside both, so
    # IoU = 64 / 512 = 0.125 exactly for both in any evaluation order; it is the box's best and below bg: both anchors come back by the restore
    box = [12.0, 10.0, 10.0, 16.0, 14.0, 14.0]
    a = R.assign([np.array([box])])
    at_max = torch.nonzero(a["labels"][0] == 1)[:, 0]
    ctr = (R.anchors()[at_max.numpy()][:, :3] + R.anchors()[at_max.numpy()][:, 3:]) / 2
    assert int(a["restored"].sum()) == 2 and ctr.tolist() == [[12.0, 12.0, 12.0], [16.0, 12.0, 12.0]] and a["gtmax"][0].tolist() == [0.125]
    labels, midx, _ = [t.cpu() for t in M.rpn_assign_targets(_gen(), R.MESH, R.GRIDS, [torch.tensor([box]).cuda()])]
    assert torch.equal(labels.double(), a["labels"]) and torch.equal(midx.long(), a["matched"])
    assert torch.equal(torch.nonzero(labels[0] == 1)[:, 0], at_max), "both mirrored anchors are restored"
    # two identical boxes: the lower index, everywhere
    labels2, midx2, _ = [t.cpu() for t in M.rpn_assign_targets(_gen(), R.MESH, R.GRIDS, [torch.tensor([box, box]).cuda()])]
    assert torch.equal(labels2, labels) and torch.equal(midx2, midx) and (midx2 <= 0).all()
    assert torch.equal(midx2.long(), R.assign([np.array([box, box])])["matched"])


def test_no_padding_mask_without_original_sizes_and_for_one_scene():
    """ori_sizes=None (the parametrised "one-scene" and "mesh-64" cases above) applies no mask; the loss ignores original_mesh_sizes for N = 1, as the
    reference does, although this scene's original size would pad most of the grid"""
    M = _m()
    boxes, a = case("one-scene", False)
    assert a["valid"].all() and (~torch.from_numpy(R.valid_mask((12, 12, 12)))).sum() > 0
    obj, reg = R.make_heads(R.HEAD_SEED, 1, 6)
    flags = R.make_flags(3, a["labels"])
    fn = M.RPNLossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION)
    want = R.losses([t.double() for t in obj], [t.double() for t in reg], flags, a["targets"])
    got = fn(R.MESH, [t.cuda() for t in obj], [t.cuda() for t in reg], [boxes[0].cuda()], [(12, 12, 12)], sampled=flags.cuda())
    assert_close(torch.stack([got["loss_objectness"], got["loss_rpn_box_reg"]]).cpu(), torch.stack(want), 1e-3, "one-scene losses")


# ---- 2. sampler --------------------------------------------------------------------------------------------------------------------------
def _state(seed, counter):
    return torch.tensor([seed, counter], dtype=torch.int64).cuda()


def test_sampler_counts_classes_determinism_and_counter():
    M = _m()
    lab = torch.tensor([[1.0] * 3 + [0.0] * 4000 + [-1.0] * 97, [1.0] * 3000 + [0.0] * 10 + [-1.0] * 1090, [-1.0] * 4100, [1.0] * 200 + [0.0] * 3900])
    lab = lab[:, torch.randperm(lab.shape[1], generator=torch.Generator().manual_seed(0))].contiguous()
    st = _state(5, 0)
    flags, counts = M.rpn_sample(lab.cuda(), R.BATCH, R.FRACTION, st)
    assert flags.dtype == torch.uint8 and counts.dtype == torch.int32
    want = R.sample_counts(lab)
    assert want == [(3, 253), (128, 10), (0, 0), (128, 128)] and counts.cpu().tolist() == [list(w) for w in want]
    f = flags.cpu()
    assert [(int((r == 1).sum()), int((r == 2).sum())) for r in f] == want
    assert (lab[f == 1] == 1).all() and (lab[f == 2] == 0).all() and (f[lab == -1] == 0).all()
    assert st.cpu().tolist() == [5, 1], "the counter advances by one per call"
    again, _ = M.rpn_sample(lab.cuda(), R.BATCH, R.FRACTION, _state(5, 0))
    assert torch.equal(again.cpu(), f), "the same rng_state gives the same flags"
    other, _ = M.rpn_sample(lab.cuda(), R.BATCH, R.FRACTION, st)
    assert st.cpu().tolist() == [5, 2] and not torch.equal(other.cpu(), f)
    assert not torch.equal(f[3], M.rpn_sample(lab[3:].cuda(), R.BATCH, R.FRACTION, _state(6, 0))[0][0].cpu()), "another seed, another draw"


def test_sampler_is_uniform():
    M = _m()
    n, cand, draw, scenes, counters = 1500, 40, 8, 64, 8
    row = torch.full((n,), -1.0)
    pos = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:cand]
    row[pos] = 1.0
    lab = row[None, :].repeat(scenes, 1).cuda()
    hits = torch.zeros(n, dtype=torch.int64)
    for c in range(counters):
        flags, counts = M.rpn_sample(lab, 2 * draw, 0.5, _state(1234, c))
        assert (counts.cpu() == torch.tensor([draw, 0])).all()
        hits += (flags.cpu() == 1).sum(0)
    S, p = scenes * counters, draw / cand
    assert hits.sum().item() == S * draw and (hits[row != 1] == 0).all()
    dev = (hits[pos].double() - S * p).abs().max().item()
    assert dev <= 6 * math.sqrt(S * p * (1 - p)), (dev, hits[pos].tolist())


# ---- 3. losses ---------------------------------------------------------------------------------------------------------------------------
# The wide case: two scenes of 42^3 + 3^3 anchors (one cube per location: side 16 at stride 2, side 32 at stride 28) are 2 x (290 + 1) = 582 workgroups of
# the loss kernel, more than the 256 partial sums that the final pass takes in its first round, so its strided loop runs.  40000 anchors per scene are
# sampled, so that most workgroups contribute.  Integer boxes; the seed is the first whose decisions all have their margin and which gives both scenes a
# positive anchor on the second level.
WIDE = dict(mesh=(84, 84, 84), grids=((42, 42, 42), (3, 3, 3)), ori=((84, 84, 84), (70, 84, 60)), sizes=((16,), (32,)), ratios=(((1., 1., 1.),),) * 2, nbox=(4, 3),
            seed=262, batch=40000)


@functools.lru_cache(maxsize=None)
def wide_case():
    rng = np.random.default_rng(WIDE["seed"])
    boxes = []
    for k, ori in zip(WIDE["nbox"], WIDE["ori"]):
        size = rng.integers(10, 34, (k, 3))
        lo = (rng.uniform(0, 1, (k, 3)) * (np.asarray(ori) - size + 1)).astype(np.int64)
        boxes.append(torch.from_numpy(np.concatenate([lo, lo + size], 1).astype(np.float32)))
    a = R.assign(boxes, mesh=WIDE["mesh"], grids=WIDE["grids"], ori=WIDE["ori"], base=R.base_anchors(WIDE["sizes"], WIDE["ratios"]))
    for k, v in R.decision_margins(a).items():
        assert v >= 1e-3, ("wide", k, v)
    assert ((a["labels"][:, 42 ** 3:] == 1).sum(1) > 0).all()
    return boxes, a


def _heads(rotated, wide):
    if wide:
        return R.make_heads(R.HEAD_SEED, len(WIDE["nbox"]), 6, grids=WIDE["grids"], A=[1, 1])
    return R.make_heads(R.HEAD_SEED, len(R.NBOX), 8 if rotated else 6)


@functools.lru_cache(maxsize=None)
def ref_losses(rotated, wide=False):
    """float64 losses and the gradients of (1.0 objectness + 0.7 box): of the g20 case for its recorded sampled set, or of the wide case (6 columns)"""
    if wide:
        a = wide_case()[1]
        flags = R.make_flags(3, a["labels"], batch=WIDE["batch"])
    else:
        a = case("g20", rotated)[1]
        g = np.load(os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz"))
        flags = torch.from_numpy(g[("o_" if rotated else "a_") + "flags"])
    heads = [[t.double().requires_grad_(True) for t in ts] for ts in _heads(rotated, wide)]
    out = R.losses(*heads, flags, a["targets"])
    (out[0] + 0.7 * out[1]).backward()
    return flags, [o.detach() for o in out], [[t.grad for t in ts] for ts in heads]


def _run(rotated, flags, heads, wide=False):
    boxes = wide_case()[0] if wide else case("g20", rotated)[0]
    gen = _m().AnchorGenerator3D(WIDE["sizes"], WIDE["ratios"]) if wide else _gen()
    fn = _m().RPNLossComputation(gen, R.FG, R.BG, R.BATCH, R.FRACTION, rotated_bbox=rotated)
    ori = torch.tensor(WIDE["ori"] if wide else R.ORI, dtype=torch.int32).cuda()
    out = fn(WIDE["mesh"] if wide else R.MESH, heads[0], heads[1], [b.cuda() for b in boxes], ori, sampled=None if flags is None else flags.cuda())
    (out["loss_objectness"] + 0.7 * out["loss_rpn_box_reg"]).backward()
    return out


def _gpu_heads(rotated, wide=False):
    return [[t.cuda().requires_grad_(True) for t in ts] for ts in _heads(rotated, wide)]


@pytest.mark.parametrize("rotated,wide", ((False, False), (True, False), (False, True)), ids=("aabb", "obb", "aabb-above-256-partials"))
def test_losses_and_gradients_against_float64(rotated, wide):
    flags, want, wgrads = ref_losses(rotated, wide)
    C = 8 if rotated else 6
    heads = _gpu_heads(rotated, wide)
    out = _run(rotated, flags, heads, wide)
    tag = ("obb" if rotated else "aabb") + (" wide" if wide else "")
    assert_close(torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"]]).detach().cpu(), torch.stack(want), 1e-3, f"{tag} losses")
    if not wide:
        g = np.load(os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz"))
        assert_close(torch.stack([out["loss_objectness"], out["loss_rpn_box_reg"]]).detach().cpu(), torch.from_numpy(g[("o_" if rotated else "a_") + "losses"]), 1e-3, f"g20 {tag} losses")
    assert out["loss_rpn_box_reg_2d"].item() == 0 and not out["loss_rpn_box_reg_2d"].requires_grad
    for name, ts, ws in zip(("d objectness", "d pred_bbox_deltas"), heads, wgrads):
        for k, (t, w) in enumerate(zip(ts, ws)):
            if w.abs().sum() > 0:
                assert_close(t.grad.cpu(), w, 1e-3, f"{tag} {name} level {k}")
            else:
                assert (t.grad == 0).all()
    go, gr = R.flatten_heads([t.grad.cpu() for t in heads[0]], [t.grad.cpu() for t in heads[1]], C)
    assert (go[flags == 0] == 0).all() and (gr[flags != 1] == 0).all(), "gradients are exactly zero at unsampled anchors"
    assert (go[flags != 0] != 0).all() and (gr[flags == 1].abs().sum(-1) > 0).all()


def test_two_runs_are_bit_identical():
    res = []
    for _ in range(2):
        heads = _gpu_heads(True)
        out = _run(True, ref_losses(True)[0], heads)
        res.append([out["loss_objectness"].detach(), out["loss_rpn_box_reg"].detach()] + [t.grad for ts in heads for t in ts])
    assert all(torch.equal(a, b) for a, b in zip(*res))


# ---- 4. capture and synchronisation ------------------------------------------------------------------------------------------------------
def test_forward_backward_with_the_sampler_in_a_captured_graph_and_without_host_synchronisation():
    M = _m()
    boxes, _ = case("g20", True)
    boxes, ori = [b.cuda() for b in boxes], torch.tensor(R.ORI, dtype=torch.int32).cuda()
    fn = M.RPNLossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION, rotated_bbox=True, seed=9)
    base = [[t.cuda() for t in ts] for ts in R.make_heads(R.HEAD_SEED, len(R.NBOX), 8)]

    def leaves():
        return [[t.clone().requires_grad_(True) for t in ts] for ts in base]

    def run(heads):
        out = fn(R.MESH, heads[0], heads[1], boxes, ori)
        flat = [t for ts in heads for t in ts]
        return [out["loss_objectness"].detach(), out["loss_rpn_box_reg"].detach()] + list(torch.autograd.grad(out["loss_objectness"] + out["loss_rpn_box_reg"], flat))

    run(leaves())                                # creates rng_state and the level table (the one host-to-device copy of the object's life)
    eager = []
    for c in range(3):
        fn.rng_state.copy_(_state(9, 100 + c))
        heads = leaves()
        torch.cuda.synchronize()
        mode = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            eager.append(run(heads))
        finally:
            torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert fn.rng_state.cpu().tolist() == [9, 103]
    assert not torch.equal(eager[0][2], eager[1][2]), "another counter, another sample"
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        heads = leaves()
        run(heads)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(heads)
    fn.rng_state.copy_(_state(9, 100))
    for c in range(3):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert len(out) == 10 and all(torch.equal(a, b) for a, b in zip(out, eager[c])), f"replay {c}"
    assert fn.rng_state.cpu().tolist() == [9, 103] and eager[0][1].item() > 0


# ---- 5. error paths ----------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    M = _m()
    boxes, _ = case("g20", False)
    boxes = [b.cuda() for b in boxes]
    heads = _gpu_heads(False)
    fn = M.RPNLossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION)
    with pytest.raises(TypeError):
        fn(R.MESH, [t.double() for t in heads[0]], heads[1], boxes)
    with pytest.raises(RuntimeError):
        fn(R.MESH, [t.cpu() for t in heads[0]], heads[1], boxes)
    with pytest.raises(RuntimeError):
        M.rpn_assign_targets(_gen(), R.MESH, R.GRIDS, [b.cpu() for b in boxes])
    with pytest.raises(TypeError):
        M.rpn_sample(torch.zeros((1, 8), dtype=torch.float64).cuda(), 4, 0.5, _state(0, 0))
    five = M.AnchorGenerator3D(R.ANCHOR_SIZES + ((128,),), R.ASPECT_RATIOS[:1] * 5)
    with pytest.raises(ValueError):
        M.RPNLossComputation(five, R.FG, R.BG, R.BATCH, R.FRACTION)
    with pytest.raises(ValueError):
        M.rpn_assign_targets(five, (64, 64, 64), ((16,) * 3, (8,) * 3, (4,) * 3, (2,) * 3, (1,) * 3), boxes)
    one = M.AnchorGenerator3D(((8,),), (((1., 1., 1.),),))
    with pytest.raises(ValueError):
        M.rpn_assign_targets(one, (8, 8, 8), ((2, 2, 2),), [torch.zeros((0, 6)).cuda()] * 65)
    with pytest.raises(ValueError):
        M.rpn_sample(torch.zeros((65, 8)).cuda(), 4, 0.5, _state(0, 0))
    with pytest.raises(NotImplementedError):
        M.RPNLossComputation(_gen(), R.FG, R.BG, R.BATCH, R.FRACTION, rotated_bbox=True, reg_loss_type="giou")
