"""The RoI stage on the GPU (nerf_mae_amd.detector over csrc/roi_head.hip) against the float64 restatement of tests/_roi_head_ref.py (itself checked against the
recorded reference, tests/golden/g22_roi_head.npz, in tests/test_roi_head_ref_cpu.py).

Tolerance: the project's contract for fp32, assert_close(rtol=1e-3).  Labels, kept rows, levels and exact zeros are compared exactly; that is defined because every
input used here has a margin of at least 1e-3 on every discrete decision (asserted before each comparison; fp32 errs by about 1e-6 on an IoU or a grid position),
or sits on integers, where fp32 is exact.  Geometry: a 32^3 mesh with maps 16^3 / 8^3 / 4^3 (scales 2 / 4 / 8) and a 32 x 24 x 16 mesh with non-cubic maps, two
scenes, 23 axis-aligned or 15 oriented RoIs per scene (tests/_roi_head_ref.pool_rois), C = 8 and C = 5 (the channel tail of a lane's 8), output (2,2,2) and (3,2,1); C = 20
with output (5,4,3) (three channel groups, the last ragged) and C = 12 with output (7,7,7) (three workgroups per RoI); four levels; remap with
oriented boxes on 8 RoIs per scene that use all three levels (tests/_roi_head_ref.remap_case).  Targets and the sampler are also run on 2500 proposals per scene
(H.BIG, H.SAMPLER), where rows are compared by their own margins and the sampler against its restatement in integers.  Measured on an MI355X (NMH_PRINT_ERR=1): DESIGN.md 3.13.

The built-in sampler is checked for its counts, classes, with-replacement draws, one-sided cases, determinism and uniformity: 64 identical scenes x 8 fixed counters =
512 draws of 8 out of 40 foreground candidates, every candidate's count within 6 standard deviations of Binomial(512, 0.2) (about 102 +- 54); and 512 x 8
background draws with replacement over 30 candidates, every count within 6 standard deviations of Binomial(4096, 1/30) (about 137 +- 69).  The seeds are fixed."""
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

from tests import _roi_head_ref as H  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g22_roi_head.npz"))
FORMS = [("a_", False), ("o_", True)]


def _m():
    from nerf_mae_amd import detector
    return detector


def _state(seed, counter):
    return torch.tensor([seed, counter], dtype=torch.int64).cuda()


def _i32(x):
    return torch.as_tensor(np.asarray(x), dtype=torch.int32).cuda()


def _dense(rois):
    """per-scene [K, 1+B] -> the dense triple on the device"""
    d = torch.stack(rois)
    return d[..., 1:].contiguous().cuda(), d[..., 0].to(torch.int32).cuda(), _i32([r.shape[0] for r in rois])


# ---- 1. matching and labels --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre,rotated", FORMS)
def test_targets_in_both_modes_with_the_recorded_keep(pre, rotated):
    M = _m()
    rois, gts, labs, _ = H.gold_inputs(rotated)
    keep, n_fg = GOLD[pre + "keep"], GOLD[pre + "n_fg"]
    for k, nf in ((None, None), (keep, n_fg)):
        L, Ro, Gr, m = H.targets(rois, gts, labs, keep=k, n_fg=nf)
        assert min(m["iou_fg"], m["iou_bg"], m["iou_top2"]) >= H.MARGIN
        boxes, levels, counts = _dense(rois)
        kw = {} if k is None else dict(keep=_i32(k), keep_counts=_i32(np.stack([nf, keep.shape[1] - nf], 1)))
        out = M.roi_targets_dense(boxes, levels, counts, [g.cuda() for g in gts], [l.cuda() for l in labs], H.GOLD["R"], 3, H.FG, H.BG, None, k is not None, **kw)
        labels, r, gr, kept, _ = [None if t is None else t.cpu() for t in out]
        assert labels.dtype == torch.float32 and kept.dtype == torch.int32
        assert torch.equal(labels.double(), torch.stack(L)), "labels"
        assert torch.equal(kept.long(), torch.arange(H.GOLD["K"]).repeat(2, 1) if k is None else torch.as_tensor(keep))
        assert torch.equal(r.double(), torch.stack(Ro)) and torch.equal(gr.double(), torch.stack(Gr)), "rows are copies"
    # the list form in evaluation mode, with scenes of different sizes and rows past the counts
    layer = M.ProposalTargetLayer(2, batch_size=12, is_rotated_bbox=rotated)
    short = [rois[0][:5], rois[1]]
    L, Ro, Gr, _ = H.targets(short, gts, labs)
    l2, r2, g2 = layer([r.cuda() for r in short], [g.cuda() for g in gts], [l.cuda() for l in labs], is_sample=False)
    assert [t.shape[0] for t in l2] == [5, 8] and all(torch.equal(a.cpu().double(), b) for a, b in zip(l2 + r2 + g2, L + Ro + Gr))
    boxes, levels, counts = _dense([torch.cat([short[0], torch.ones(3, short[0].shape[1])]), rois[1]])
    counts[0] = 5
    labels, r, gr, kept, c2 = M.roi_targets_dense(boxes, levels, counts, [g.cuda() for g in gts], [l.cuda() for l in labs], 0, 0, H.FG, H.BG, None, False)
    assert c2 is None and (labels[0, 5:] == -1).all() and (r[0, 5:] == 0).all() and (gr[0, 5:] == 0).all() and (kept[0, 5:] == -1).all()


# ---- 1b. matching and labels past one chunk of either kernel -------------------------------------------------------------------------------
def _pad(per_scene, cap, fill):
    """per-scene [k, ...] float64 -> [N, cap, ...] with `fill` in the rows past k"""
    return torch.stack([torch.cat([t, torch.full((cap - t.shape[0], *t.shape[1:]), fill, dtype=t.dtype)]) for t in per_scene])


def _same_rows(a, b):
    return (a.double() == b).all(-1)


@functools.lru_cache(maxsize=None)
def big_ref(rotated):
    """the six scenes of H.BIG, the float64 matching once, and from it both outcomes of every near-tie in evaluation mode and with a given keep"""
    c = H.big_case(rotated)
    args = (c["rois"], c["gts"], c["labs"])
    ev = H.targets(*args)
    rows = ev[3]["rows"]
    keep, n_fg = H.big_keep(ev[3]["candidates"])
    kw = dict(keep=keep, n_fg=n_fg, rows=rows)
    return c, rows, keep, n_fg, ev, H.targets(*args, rows=rows, alt_arg=True), H.targets(*args, rows=rows, alt_label=True), H.targets(*args, **kw), H.targets(*args, alt_arg=True, **kw)


@pytest.mark.parametrize("pre,rotated", FORMS)
def test_targets_past_one_chunk_with_per_row_margins(pre, rotated):
    """2500 proposals per scene (three 1024-lane chunks of the sampler's walk, ten workgroups of the matching) against up to 130 boxes (three 64-box stages),
    counts on, one past and below the chunk sizes, a scene without proposals and one without boxes, garbage in the rows past the counts.  Rows that keep 1e-3
    on all three IoU decisions (at least 97 % of every scene, tests/test_roi_head_ref_cpu.py) must agree exactly; a row that does not may take either outcome
    of its near-tie.  counts above cap and below 0 are clamped."""
    M = _m()
    c, rows, keep, n_fg, ev, ev_arg, ev_lab, sm, sm_arg = big_ref(rotated)
    cap, R, N = H.BIG["cap"], H.BIG["R"], len(c["counts"])
    boxes, levels = c["boxes"].cuda(), c["levels"].cuda()
    gts, labs = [g.cuda() for g in c["gts"]], [l.cuda() for l in c["labs"]]
    exists = torch.arange(cap)[None] < torch.tensor(c["counts"])[:, None]
    decided = torch.stack([torch.cat([rm["decided"], torch.zeros(cap - rm["decided"].numel(), dtype=torch.bool)]) for rm in rows])
    assert decided.sum() >= 0.97 * exists.sum()
    clamped = [c["counts"][0] + 7] + c["counts"][1:]
    clamped[c["counts"].index(0)] = -3
    kc = _i32([[nf, R - nf] if (keep[i] >= 0).any() else [0, 0] for i, nf in enumerate(n_fg)])
    for counts in (c["counts"], clamped):
        # evaluation: every proposal
        labels, r, gr, kept, c2 = [None if t is None else t.cpu() for t in M.roi_targets_dense(boxes, levels, _i32(counts), gts, labs, 0, 0, H.FG, H.BG, None, False)]
        assert c2 is None and labels.shape == (N, cap)
        assert (labels[~exists] == -1).all() and not r[~exists].any() and not gr[~exists].any() and (kept[~exists] == -1).all(), "rows past the counts are not read"
        assert torch.equal(kept[exists].long(), torch.arange(cap).repeat(N, 1)[exists])
        assert torch.equal(r[exists][:, 1:], c["boxes"][exists]) and torch.equal(r[exists][:, 0], c["levels"][exists].float()), "rows are copies"
        L, L2, G1, G2 = _pad(ev[0], cap, -1.0), _pad(ev_lab[0], cap, -1.0), _pad(ev[2], cap, 0.0), _pad(ev_arg[2], cap, 0.0)
        assert torch.equal(labels.double()[decided], L[decided]) and torch.equal(gr.double()[decided], G1[decided]), "decided rows"
        lab_alt, box_alt = (labels.double() != L) & exists, ~_same_rows(gr, G1) & exists
        print(f"evaluation, {pre}: {int(lab_alt.sum())} labels and {int(box_alt.sum())} matched boxes of {int((exists & ~decided).sum())} undecided rows took the other outcome")
        assert ((labels.double() == L) | (labels.double() == L2)).all() and (_same_rows(gr, G1) | _same_rows(gr, G2)).all(), "an undecided row takes one of its two outcomes"
        i0 = H.BIG["G"].index(0)
        assert labels[i0, 0] == 0 and not gr[i0].any(), "the scene without boxes: IoU 0, label 0, zero gt_rois"
        # sampling with a given keep
        labels, r, gr, kept, c2 = [t.cpu() for t in M.roi_targets_dense(boxes, levels, _i32(counts), gts, labs, R, R // 2, H.FG, H.BG, None, True, keep=_i32(keep), keep_counts=kc)]
        assert torch.equal(kept.long(), keep) and torch.equal(c2, kc.cpu())
        assert torch.equal(r.double(), torch.stack(sm[1])), "rows are copies, zero where keep is -1"
        L, L2, G1, G2 = torch.stack(sm[0]), torch.stack(sm_arg[0]), torch.stack(sm[2]), torch.stack(sm_arg[2])
        slot_decided = torch.stack([torch.cat([rm["decided"], torch.ones(1, dtype=torch.bool)])[keep[i]] for i, rm in enumerate(rows)])      # keep -1 -> the appended True
        assert torch.equal(labels.double()[slot_decided], L[slot_decided]) and torch.equal(gr.double()[slot_decided], G1[slot_decided]), "decided rows"
        first = (labels.double() == L) & _same_rows(gr, G1)
        print(f"given keep, {pre}: {int((~first).sum())} of {int((~slot_decided).sum())} undecided slots took the other box")
        assert (first | ((labels.double() == L2) & _same_rows(gr, G2))).all(), "label and box of an undecided row come from one of its top two boxes"
        assert (L[~slot_decided] != L2[~slot_decided]).any(), "a near-tie between boxes of different labels is among the kept rows"


# ---- 2. the sampler ----------------------------------------------------------------------------------------------------------------------
def _synthetic(n_fg, n_bg, n_mid, scenes=1, seed=0):
    """one box and proposals that are copies of it (IoU 1), disjoint (IoU 0) or half overlapping (IoU 1/3: neither), in a seeded order"""
    gt = torch.tensor([[0.0, 0, 0, 4, 4, 4]])
    rows = [[0.0, 0, 0, 4, 4, 4]] * n_fg + [[10.0, 10, 10, 14, 14, 14]] * n_bg + [[2.0, 0, 0, 6, 4, 4]] * n_mid
    perm = torch.randperm(len(rows), generator=torch.Generator().manual_seed(seed))
    kind = torch.tensor([0] * n_fg + [1] * n_bg + [2] * n_mid)[perm]
    boxes = torch.tensor(rows)[perm][None].repeat(scenes, 1, 1).cuda()
    n = len(rows)
    return boxes, torch.zeros((scenes, n), dtype=torch.int32).cuda(), _i32([n] * scenes), [gt.cuda()] * scenes, [torch.full((1,), 3.0).cuda()] * scenes, kind


def _sample(M, args, R, want, state):
    boxes, levels, counts, gts, labs, _ = args
    return [t.cpu() for t in M.roi_targets_dense(boxes, levels, counts, gts, labs, R, want, 0.5, 0.2, state, True)]


def test_sampler_counts_classes_and_determinism():
    M = _m()
    args = _synthetic(5, 30, 4)
    kind = args[5]
    st = _state(5, 0)
    labels, rois, gt_rois, keep, c2 = _sample(M, args, 16, 8, st)
    assert c2.tolist() == [[5, 11]] and st.cpu().tolist() == [5, 1], "min(want, #fg) foreground rows, the rest background; the counter advances by one"
    k = keep[0].long()
    assert (kind[k[:5]] == 0).all() and len(set(k[:5].tolist())) == 5 and k[:5].tolist() == sorted(k[:5].tolist()), "without replacement, in index order"
    assert (kind[k[5:]] == 1).all(), "background draws stay inside the candidate set"
    assert labels[0].tolist() == [3.0] * 5 + [0.0] * 11, "the matched box's label, 0 in the background slots"
    assert torch.equal(rois[0, :, 1:], args[0][0].cpu()[k]) and (gt_rois[0] == args[3][0].cpu()).all()
    again = _sample(M, args, 16, 8, _state(5, 0))
    assert all(torch.equal(a, b) for a, b in zip(again, (labels, rois, gt_rois, keep, c2))), "the same rng_state gives the same sample"
    other = _sample(M, args, 16, 8, st)
    assert st.cpu().tolist() == [5, 2] and not torch.equal(other[3], keep)
    assert not torch.equal(_sample(M, args, 16, 8, _state(6, 0))[3], keep), "another seed, another draw"
    # more candidates than wanted: a cut
    labels, _, _, keep, c2 = _sample(M, _synthetic(40, 30, 4), 16, 8, _state(1, 0))
    assert c2.tolist() == [[8, 8]] and len(set(keep[0, :8].tolist())) == 8


def test_sampler_one_sided_and_empty_scenes():
    M = _m()
    for n_fg, n_bg, want in ((6, 0, [12, 0]), (0, 7, [0, 12]), (0, 0, [0, 0])):
        args = _synthetic(n_fg, n_bg, 5)
        labels, rois, gt_rois, keep, c2 = _sample(M, args, 12, 6, _state(2, 0))
        assert c2.tolist() == [want]
        if sum(want) == 0:
            assert (keep == -1).all() and (labels == -1).all() and (rois == 0).all() and (gt_rois == 0).all(), "no candidate: label -1 and zero boxes"
        else:
            assert (args[5][keep[0].long()] == (0 if n_fg else 1)).all() and (labels[0] == (3.0 if n_fg else 0.0)).all()
            assert len(set(keep[0].tolist())) > 1, "draws with replacement spread over the candidates"


def test_sampler_is_uniform():
    M = _m()
    scenes, counters, draw = 64, 8, 8
    args = _synthetic(40, 30, 10, scenes=scenes, seed=1)
    kind = args[5]
    n = kind.numel()
    fg_hits, bg_hits = torch.zeros(n, dtype=torch.int64), torch.zeros(n, dtype=torch.int64)
    for c in range(counters):
        _, _, _, keep, c2 = _sample(M, args, 2 * draw, draw, _state(1234, c))
        assert (c2 == torch.tensor([draw, draw])).all()
        fg_hits += torch.bincount(keep[:, :draw].reshape(-1).long(), minlength=n)
        bg_hits += torch.bincount(keep[:, draw:].reshape(-1).long(), minlength=n)
    S = scenes * counters
    for hits, cls, trials, p in ((fg_hits, 0, S, draw / 40), (bg_hits, 1, S * draw, 1 / 30)):
        assert hits[kind != cls].sum() == 0 and hits.sum() == S * draw
        sd = math.sqrt(trials * p * (1 - p))
        dev = (hits[kind == cls].double() - trials * p).abs().max().item()
        assert dev <= 6 * sd, f"class {cls}: a count deviates by {dev:.0f} > 6 sigma = {6 * sd:.0f}"


@functools.lru_cache(maxsize=None)
def sampler_ref():
    c = H.sampler_case()
    rois = H.sampler_rois(c)
    m = H.targets(rois, c["gts"], c["labs"])[3]
    assert all(bool(rm["decided"].all()) for rm in m["rows"])
    return c, rois, m


def test_sampler_equals_its_restatement_across_chunks():
    """keep and counts2 against the draw restated in Python integers (H.sample) on scenes of up to 2500 rows whose rows are all decided by construction: a
    cut in all three chunks, more than 1024 background candidates, one-sided and empty scenes, garbage foreground rows past the counts, R below and above
    1024.  The conditions on these inputs are asserted on the restatement in tests/test_roi_head_ref_cpu.py."""
    M = _m()
    c, rois, m = sampler_ref()
    boxes, levels, counts = c["boxes"].cuda(), c["levels"].cuda(), _i32(c["counts"])
    gts, labs = [g.cuda() for g in c["gts"]], [l.cuda() for l in c["labs"]]
    seed = H.SAMPLER["seed"]
    for R, want in H.SAMPLER["runs"]:
        for counter in H.SAMPLER["counters"]:
            st = _state(seed, counter)
            labels, r, gr, keep, c2 = [t.cpu() for t in M.roi_targets_dense(boxes, levels, counts, gts, labs, R, want, H.FG, H.BG, st, True)]
            ref = [H.sample(f, b, R, want, seed, counter, i) for i, (f, b) in enumerate(m["candidates"])]
            rk, rc = torch.tensor([k for k, _, _ in ref]), torch.tensor([list(n) for _, n, _ in ref])
            differ = int((keep.long() != rk).sum())
            print(f"sampler R {R} want {want} counter {counter}: {differ} of {rk.numel()} slots differ")
            assert torch.equal(c2.long(), rc), (c2.tolist(), rc.tolist())
            assert differ == 0, [(i, int((keep[i].long() != rk[i]).sum())) for i in range(rk.shape[0])]
            assert st.cpu().tolist() == [seed, counter + 1]
            L, Ro, Gr, _ = H.targets(rois, c["gts"], c["labs"], keep=rk, n_fg=rc[:, 0].tolist(), rows=m["rows"])
            assert torch.equal(labels.double(), torch.stack(L)) and torch.equal(r.double(), torch.stack(Ro)) and torch.equal(gr.double(), torch.stack(Gr))


# ---- 3. pooling --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool_ref(key):
    rotated, _, C, out = key
    rois, maps = H.pool_case(key)
    dout = torch.randn((rois.shape[0] * rois.shape[1], C, *out), generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    res, m, dmaps = H.pool(maps, rois, out=out, rotated=rotated, dout=dout)
    return rois, maps, dout, res, m, dmaps


@pytest.mark.parametrize("key", list(H.POOL_CASES), ids=lambda k: f"{'obb' if k[0] else 'aabb'}-{'noncubic' if k[1] else 'cubic'}-C{k[2]}-{'x'.join(map(str, k[3]))}")
def test_pooling_forward_and_backward(key):
    M = _m()
    rotated, _, C, out = key
    rois, maps, dout, res, m, dmaps = pool_ref(key)
    assert m["floor"] >= H.MARGIN and m["cell_gap"] >= H.MARGIN, m
    assert m["padded_cells"] > 0 and m["ragged"] > 0 and (m["masked_points"] > 0 or not rotated), "the cases the kernel can go wrong at are present"
    pool = M.ROIPool(out, H.SCALES, H.ENLARGE, rotated)
    leaves = [t.cuda().requires_grad_(True) for t in maps]
    got = pool(leaves, rois.cuda())
    assert got.shape == res.shape
    assert_close(got, res, 1e-3, "pooled")
    assert torch.equal(got.detach().cpu() == 0, res == 0), "exact zeros where the padding or a masked point won"
    got.backward(dout.cuda())
    for k, (leaf, want) in enumerate(zip(leaves, dmaps)):
        assert_close(leaf.grad, want, 1e-3, f"d map {k}")
        assert (leaf.grad.cpu()[want == 0] == 0).all(), "exactly zero gradient where no cell's maximum came from"
    # where the zero won, no gradient flows: the gradient of only those cells is zero everywhere
    leaves = [t.cuda().requires_grad_(True) for t in maps]
    got = pool(leaves, rois.cuda())
    got.backward((got.detach() == 0).float())
    assert all((leaf.grad == 0).all() for leaf in leaves)
    # the reference's per-scene lists give the same features
    lists = pool([[t[i].cuda() for t in maps] for i in range(rois.shape[0])], [r.cuda() for r in rois])
    assert torch.equal(torch.cat(lists), got.detach())


@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_pooling_over_four_levels(rotated):
    """scales 2 / 4 / 8 / 16 with a 2^3 map behind the cubic three and every third RoI on level 3: the fourth slot of the kernels' level tables"""
    M = _m()
    rois, maps = H.pool4_case(rotated)
    C, out = H.POOL4["C"], H.POOL4["out"]
    dout = torch.randn((rois.shape[0] * rois.shape[1], C, *out), generator=torch.Generator().manual_seed(5), dtype=torch.float32)
    res, m, dmaps = H.pool(maps, rois, scales=H.SCALES4, out=out, rotated=rotated, dout=dout)
    assert m["floor"] >= H.MARGIN and m["cell_gap"] >= H.MARGIN and (rois[..., 0] == 3).sum() >= 10, m
    at3 = (rois[..., 0] == 3).reshape(-1)
    assert res[at3].abs().sum() > 0 and dmaps[3].abs().sum() > 0, "level 3 gives values and takes gradient"
    pool = M.ROIPool(out, H.SCALES4, H.ENLARGE, rotated)
    leaves = [t.cuda().requires_grad_(True) for t in maps]
    got = pool(leaves, rois.cuda())
    assert_close(got, res, 1e-3, "pooled, four levels")
    assert torch.equal(got.detach().cpu() == 0, res == 0), "exact zeros where the padding or a masked point won"
    got.backward(dout.cuda())
    for k, (leaf, want) in enumerate(zip(leaves, dmaps)):
        assert_close(leaf.grad, want, 1e-3, f"d map {k}, four levels")
        assert (leaf.grad.cpu()[want == 0] == 0).all(), "exactly zero gradient where no cell's maximum came from"


def test_pooling_with_remap_and_the_level_mapper():
    M = _m()
    key = (False, False, 8, (2, 2, 2))
    rois, maps = H.pool_case(key)
    rois = rois[:, :20].contiguous()        # the seeded RoIs: under its remapped level one of the three special RoIs lands on a voxel boundary
    kmin, kmax = H.mapper_range(H.SCALES)
    lv, lm = H.level_map(rois[..., 1:], kmin, kmax, 32, 3)
    assert lm >= H.MARGIN and len(set(lv.reshape(-1).tolist())) > 1
    mapper = M.LevelMapper(kmin, kmax, 32, 3)
    got = mapper(rois[..., 1:].cuda())
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), lv)
    res, m, _ = H.pool(maps, rois, out=key[3], rotated=False, levels=lv)
    assert m["floor"] >= H.MARGIN
    pool = M.ROIPool(key[3], H.SCALES, H.ENLARGE, False, max_res=32, remap=True)
    assert_close(pool([t.cuda() for t in maps], rois.cuda()), res, 1e-3, "pooled with remap")
    for pre, rotated in FORMS[:1]:                      # the recorded remap run
        _, gts, labs, gmaps = H.gold_inputs(rotated)
        Ro = torch.stack(H.targets(H.gold_inputs(rotated)[0], gts, labs, keep=GOLD[pre + "keep"], n_fg=GOLD[pre + "n_fg"])[1]).float()
        pool = M.ROIPool(H.GOLD["out"], H.SCALES, H.ENLARGE, rotated, max_res=H.GOLD["max_res"], remap=True)
        assert_close(pool([t.cuda() for t in gmaps], Ro.cuda()), torch.as_tensor(GOLD[pre + "pooled_remap"]), 1e-3, "recorded remap")


def test_oriented_remap_pooling_and_the_model_around_it():
    """remap with oriented boxes: the levels come from the un-enlarged RoIs, the pooling enlarges a copy, and Classification_Model encodes, decodes and returns the
    un-enlarged RoIs (with remap off: the enlarged ones, test_classification_model_against_the_recorded_run)"""
    M = _m()
    c = H.remap_case()
    m = c["margins"]
    assert min(m["level"], m["iou"], m["floor"], m["cell_gap"]) >= H.MARGIN and m["levels_used"] == 3 and m["masked_points"] > 0, m
    rois, gts, labs, maps, keep, n_fg = c["rois"], c["gts"], c["labs"], c["maps"], c["keep"], c["n_fg"]
    dense, out, N, R = torch.stack(rois), H.GOLD["out"], H.GOLD["N"], H.GOLD["R"]
    pool = M.ROIPool(out, H.SCALES, H.ENLARGE, True, max_res=H.GOLD["max_res"], remap=True)
    dev = [t.cuda() for t in maps]
    assert torch.equal(pool.map_levels(dense[..., 1:].cuda()).cpu(), c["levels"])
    res, _, _ = H.pool(maps, dense, out=out, rotated=True, levels=c["levels"])
    assert_close(pool(dev, dense.cuda()), res, 1e-3, "pooled with remap, oriented")
    # the model: the restatement's kept rows pooled at their mapped levels, the tiny head in float64, targets and decode against the un-enlarged RoIs
    L, Ro, Gr, _ = H.targets(rois, gts, labs, keep=keep, n_fg=n_fg)
    Ro = torch.stack(Ro)
    kmin, kmax = H.mapper_range(H.SCALES)
    pooled, _, _ = H.pool(maps, Ro.float(), out=out, rotated=True, levels=H.level_map(Ro[..., 1:], kmin, kmax, H.GOLD["max_res"], len(H.SCALES))[0])
    hp = {k: v.double() for k, v in H.gold_head(True).items()}
    x = pooled.reshape(N * R, -1)
    deltas, scores = x @ hp["RCNN_bbox_pred_w"].T + hp["RCNN_bbox_pred_b"], x @ hp["RCNN_cls_score_w"].T + hp["RCNN_cls_score_b"]
    flat = Ro.reshape(N * R, -1)[:, 1:]
    want = H.loss(scores, deltas, torch.cat(L), flat, torch.cat(Gr), True)
    boxes, margin = H.decode(deltas, flat, True)
    assert margin >= H.MARGIN
    model = _model(M, True)
    model.pooling_model = pool
    args = ([r.cuda() for r in rois], [g.cuda() for g in gts], [l.cuda() for l in labs], dev)
    kw = dict(keep=_i32(keep), keep_counts=_i32(np.stack([n_fg, [R - n for n in n_fg]], 1)))
    (proposals, labels), _, loss = model(*args, is_sample=True, is_reg=True, **kw)
    assert torch.equal(labels.cpu().double(), torch.stack(L))
    assert_close(torch.stack([loss["loss_objectness"], loss["loss_rpn_box_reg"]]), torch.stack([want["obj"], want["reg"]]), 1e-3, "losses with remap")
    assert_close(torch.cat(proposals), boxes, 1e-3, "decoded proposals with remap")
    (sample_rois, _), _, _ = model(*args, is_sample=True, is_reg=False, **kw)
    assert torch.equal(torch.cat(sample_rois).cpu().double(), flat), "the returned RoIs are the un-enlarged ones"


# ---- 4. losses and decode ------------------------------------------------------------------------------------------------------------------
# 2 scenes of 35000 rows are 274 workgroups of the loss kernel, more than the 256 partial sums that the final pass takes in its first round, so its strided
# loop runs; a third of the rows are positive and one in 97 is ignored
WIDE_ROWS = (2, 35000)


def _wide_labels():
    lab = torch.tensor([0.0, 1, 0, 2, 0, 0])[torch.arange(WIDE_ROWS[0] * WIDE_ROWS[1]) % 6]
    lab[::97] = -1.0
    return lab


def _loss_case(rotated, labels=None, N=1, K=300):
    B, g = (7 if rotated else 6), torch.Generator().manual_seed(11)
    rois, gts, _ = H.make_scene(21, rotated, N=N, K=K, G=4)
    ex, gt = torch.cat(rois), torch.cat([b[torch.arange(K) % 4] for b in gts])
    scores, deltas = torch.randn((N * K, 3), generator=g) * 2, torch.randn((N * K, B), generator=g) * 0.3
    lab = torch.tensor([0.0, 1, 2, -1, 0, 1])[torch.arange(N * K) % 6] if labels is None else labels
    return scores, deltas, lab, ex, gt


def _run_loss(M, case, weights=(1.0, 1.0)):
    scores, deltas, lab, ex, gt = case
    s, d = scores.cuda().requires_grad_(True), deltas.cuda().requires_grad_(True)
    loss, targets = M.roi_head_loss(s, d, lab.cuda(), ex.cuda(), gt.cuda(), return_targets=True)
    (weights[0] * loss["loss_objectness"] + weights[1] * loss["loss_rpn_box_reg"]).backward()
    return loss["loss_objectness"].detach(), loss["loss_rpn_box_reg"].detach(), targets, s.grad, d.grad


@pytest.mark.parametrize("rotated,wide", [(False, False), (True, False), (True, True)], ids=["False", "True", "True-above-256-partials"])
def test_loss_forward_and_backward(rotated, wide):
    M = _m()
    N, K = WIDE_ROWS if wide else (1, 300)
    case = _loss_case(rotated, _wide_labels() if wide else None, N, K)
    r = H.loss(case[0], case[1], case[2], case[3][:, 1:], case[4], rotated)
    obj, reg, targets, gs, gd = _run_loss(M, case, (1.0, 0.5))
    assert_close(obj.reshape(1), r["obj"].reshape(1), 1e-3, "loss_objectness")
    assert_close(reg.reshape(1), r["reg"].reshape(1), 1e-3, "loss_rpn_box_reg")
    assert_close(targets, r["targets"], 1e-3, "regression targets")
    assert_close(gs, r["dscores"], 1e-3, "d scores")
    assert_close(gd, 0.5 * r["ddeltas"], 1e-3, "d deltas")
    ignored, notpos = case[2] < 0, ~(case[2] > 0)
    assert (gs.cpu()[ignored] == 0).all() and (gd.cpu()[notpos] == 0).all() and (targets.cpu()[ignored] == 0).all(), "ignored rows take no part"
    again = _run_loss(M, case, (1.0, 0.5))
    assert all(torch.equal(a, b) for a, b in zip(again, (obj, reg, targets, gs, gd))), "bit-identical across two runs"
    # no positive row: the box loss is 0 with zero gradient; no valid row: both
    nopos = _run_loss(M, _loss_case(rotated, torch.tensor([0.0, -1.0]).repeat(N * K // 2), N, K))
    assert nopos[1].item() == 0 and (nopos[4] == 0).all() and nopos[0].item() > 0
    none = _run_loss(M, _loss_case(rotated, torch.full((N * K,), -1.0), N, K))
    assert none[0].item() == 0 and none[1].item() == 0 and (none[3] == 0).all() and (none[4] == 0).all()


def test_decode_clip_and_angle_wrap():
    M = _m()
    for rotated in (False, True):
        scores, deltas, _, ex, _ = _loss_case(rotated)
        deltas = deltas.clone()
        deltas[0, 3], deltas[1, 4], deltas[2, 5] = 50.0, 9.0, 7.7            # above log 2000 = 7.6009
        if rotated:
            deltas[:, 6] = torch.linspace(-1.21, 1.19, 300)                    # several turns on both sides
        want, margin = H.decode(deltas, ex[:, 1:], rotated)
        assert margin >= 1e-3
        if rotated:
            assert (want[:, 6] > 0.5).any() and (want[:, 6] < -0.5).any() and want[:, 6].abs().max() <= math.pi / 2
        got = M.roi_decode(deltas.cuda(), ex.cuda())
        assert not got.requires_grad
        assert_close(got, want, 1e-3, "decoded boxes")
        coder = M.RotatedCoder() if rotated else M.AABBCoder()
        assert torch.equal(coder.decode_single(deltas.cuda(), ex[:, 1:].cuda()), got)
        gt = ex[:, 1:].roll(1, 0)
        assert_close(coder.encode_single(gt.cuda(), ex[:, 1:].cuda()), H.encode(gt, ex[:, 1:], rotated), 1e-3, "encode_single")


# ---- 5. the model --------------------------------------------------------------------------------------------------------------------------
def _model(M, rotated, seed=3):
    layer = M.ProposalTargetLayer(2, batch_size=H.GOLD["N"] * H.GOLD["R"], fg_fraction=0.5, fg_threshold=H.FG, bg_threshold=H.BG, is_rotated_bbox=rotated, seed=seed)
    pool = M.ROIPool(H.GOLD["out"], H.SCALES, H.ENLARGE, rotated, "pooling", H.GOLD["max_res"], False)
    head = M.RCNN(H.GOLD["C"], None, 2, H.GOLD["out"], is_add_layer=False, is_rotated_bbox=rotated, is_flatten=True).cuda()
    hp = H.gold_head(rotated)
    with torch.no_grad():
        head.RCNN_bbox_pred.weight.copy_(hp["RCNN_bbox_pred_w"]); head.RCNN_bbox_pred.bias.copy_(hp["RCNN_bbox_pred_b"])
        head.RCNN_cls_score.weight.copy_(hp["RCNN_cls_score_w"]); head.RCNN_cls_score.bias.copy_(hp["RCNN_cls_score_b"])
    return M.Classification_Model(None, layer, pool, head, n_classes=2, is_rotated_bbox=rotated)


@pytest.mark.parametrize("pre,rotated", FORMS)
def test_classification_model_against_the_recorded_run(pre, rotated):
    M = _m()
    rois, gts, labs, maps = H.gold_inputs(rotated)
    model = _model(M, rotated)
    assert sorted(model.RCNN_model.state_dict()) == ["RCNN_bbox_pred.bias", "RCNN_bbox_pred.weight", "RCNN_cls_score.bias", "RCNN_cls_score.weight"]
    keep, n_fg = GOLD[pre + "keep"], GOLD[pre + "n_fg"]
    before = [r.clone() for r in rois]
    dev_rois = [r.cuda() for r in rois]
    (proposals, labels), probs, loss = model(dev_rois, [g.cuda() for g in gts], [l.cuda() for l in labs], [t.cuda() for t in maps], is_sample=True, is_reg=True,
                                             keep=_i32(keep), keep_counts=_i32(np.stack([n_fg, keep.shape[1] - n_fg], 1)))
    assert all(torch.equal(a.cpu(), b) for a, b in zip(dev_rois, before)), "the caller's RoIs are not written to"
    assert torch.equal(labels.cpu().long(), torch.as_tensor(GOLD[pre + "sample_labels"]))
    got = torch.stack([loss["loss_objectness"], loss["loss_rpn_box_reg"]])
    assert_close(got, torch.as_tensor(GOLD[pre + "losses"]), 1e-3, "losses")
    assert_close(torch.cat(proposals), torch.as_tensor(GOLD[pre + "proposals"]), 1e-3, "decoded proposals")
    assert_close(torch.cat(probs), torch.as_tensor(GOLD[pre + "cls_prob"]), 1e-3, "cls_prob")
    (sample_rois, _), _, _ = model(dev_rois, [g.cuda() for g in gts], [l.cuda() for l in labs], [t.cuda() for t in maps], is_sample=True, is_reg=False,
                                   keep=_i32(keep), keep_counts=_i32(np.stack([n_fg, keep.shape[1] - n_fg], 1)))
    assert_close(torch.cat(sample_rois), torch.as_tensor(GOLD[pre + "encoded_rois"]), 1e-6, "the returned RoIs are the ones the reference encoded against")
    # evaluation: lists sized by the scenes, no loss
    (ev_rois, ev_labels), ev_probs, ev_loss = model(dev_rois, [g.cuda() for g in gts], [l.cuda() for l in labs], [t.cuda() for t in maps], is_sample=False)
    assert ev_loss == 0. and [p.shape for p in ev_probs] == [(8, 2)] * 2
    assert torch.equal(torch.cat(ev_labels).cpu().long(), torch.as_tensor(GOLD[pre + "eval_labels"]))


def test_sampling_path_in_a_captured_graph():
    M = _m()
    rotated = True
    rois, gts, labs, maps = H.gold_inputs(rotated)
    model = _model(M, rotated, seed=9)
    dense, gts, labs = _dense(rois), [g.cuda() for g in gts], [l.cuda() for l in labs]
    base = [t.cuda() for t in maps]
    params = list(model.RCNN_model.parameters())

    def run(leaves):
        (sample_rois, labels), _, loss = model(dense, gts, labs, leaves, is_sample=True)
        grads = torch.autograd.grad(loss["loss_objectness"] + loss["loss_rpn_box_reg"], leaves + params)
        return [loss["loss_objectness"].detach(), loss["loss_rpn_box_reg"].detach(), torch.stack(sample_rois).detach(), labels] + list(grads)

    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                  # leaves made, warmed up and captured on one side stream (Capture)
        leaves = [t.clone().requires_grad_(True) for t in base]
        run(leaves)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s, capture_error_mode="thread_local"):
        out = run(leaves)
    model.sample_model.rng_state.copy_(_state(9, 100))
    seen = []
    for c in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert all(torch.isfinite(t).all() for t in out), f"replay {c}"
        assert out[0].item() > 0 and (out[3] >= 0).all() and any((g != 0).any() for g in out[4:4 + len(leaves)])
        seen.append(out[2].clone())
    assert model.sample_model.rng_state.cpu().tolist() == [9, 102], "the counter advances inside the graph"
    assert not torch.equal(seen[0], seen[1]), "the replays draw different samples"


# ---- 6. error paths ------------------------------------------------------------------------------------------------------------------------
def test_error_paths():
    M = _m()
    rois, gts, labs, maps = H.gold_inputs(False)
    boxes, levels, counts = _dense(rois)
    g, l = [t.cuda() for t in gts], [t.cuda() for t in labs]
    ok = (boxes, levels, counts, g, l, 6, 3, 0.5, 0.2, _state(0, 0), True)

    def swap(i, v):
        return tuple(v if j == i else a for j, a in enumerate(ok))
    M.roi_targets_dense(*ok)
    with pytest.raises(TypeError):
        M.roi_targets_dense(*swap(0, boxes.double()))
    with pytest.raises(RuntimeError):
        M.roi_targets_dense(*swap(0, boxes.cpu()))
    for bad in (swap(0, boxes[..., :5]), swap(1, levels.long()), swap(2, counts[:1]), swap(3, g[:1]), swap(5, 0), swap(5, M.MAX_ROWS + 1), swap(9, None), swap(9, torch.zeros(2).cuda()),
                swap(0, boxes[:1].repeat(M.MAX_SCENES + 1, 1, 1))):
        with pytest.raises(ValueError):
            M.roi_targets_dense(*bad)
    with pytest.raises(NotImplementedError):
        M.ROIPool([2, 2, 2], [2, 4, 8], use_cuda=True)
    with pytest.raises(NotImplementedError):
        M.ROIPool([2, 2, 2], [2, 4, 8], feature_extracting_type="interpolation")
    for kw in (dict(output_size=[64, 64, 2]), dict(output_size=[2, 2]), dict(output_size=[0, 2, 2]), dict(spatial_scale=[1] * (M.MAX_LEVELS + 1)), dict(spatial_scale=[2, 0])):
        with pytest.raises(ValueError):
            M.ROIPool(**{**dict(output_size=[2, 2, 2], spatial_scale=[2, 4, 8]), **kw})
    pool = M.ROIPool([2, 2, 2], [2, 4, 8])
    dev = [t.cuda() for t in maps]
    r = torch.stack(rois).cuda()
    pool(dev, r)
    with pytest.raises(TypeError):
        pool([t.double() for t in dev], r)
    with pytest.raises(RuntimeError):
        pool(maps, r)
    for bad_maps, bad_rois in ((dev[:2], r), (dev, r[:1]), (dev, r[..., :6]), ([dev[0], dev[1], dev[2][:, :2]], r)):
        with pytest.raises(ValueError):
            pool(bad_maps, bad_rois)
    s, d, lab = torch.zeros(4, 2).cuda(), torch.zeros(4, 6).cuda(), torch.zeros(4).cuda()
    ex, gt = r[0, :4], r[0, :4, 1:]
    flat = M.roi_head_loss(s, d, lab, ex, gt)
    assert torch.equal(M.roi_head_loss(s, d, lab.reshape(2, 2), ex, gt)["loss_objectness"], flat["loss_objectness"]), "labels as [N, R]"
    with pytest.raises(TypeError):
        M.roi_head_loss(s.double(), d, lab, ex, gt)
    with pytest.raises(RuntimeError):
        M.roi_head_loss(s.cpu(), d, lab, ex, gt)
    for bad in ((s, d[:, :5], lab, ex, gt), (s[:3], d, lab, ex, gt), (s, d, lab[:3], ex, gt), (s, d, lab, ex[:, :5], gt), (s, d, lab, ex, gt[:, :5]),
                (torch.zeros(4, M.MAX_CLASSES + 1).cuda(), d, lab, ex, gt)):
        with pytest.raises(ValueError):
            M.roi_head_loss(*bad)
    with pytest.raises(ValueError):
        M.roi_decode(d[:, :5], ex)
    with pytest.raises(ValueError):
        M.roi_decode(d, ex[:3])
    with pytest.raises(TypeError):
        M.roi_decode(d.double(), ex)
    with pytest.raises(ValueError):
        M.LevelMapper(1, 3)(torch.zeros(4, 5).cuda())
    M.RotatedCoder(math.log(2000.0)), M.AABBCoder()
    for coder in (M.RotatedCoder, M.AABBCoder):
        with pytest.raises(NotImplementedError):
            coder(bbox_xform_clip=math.log(1000.0 / 16))
