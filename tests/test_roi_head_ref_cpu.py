"""The float64 restatement of the RoI stage (tests/_roi_head_ref.py) against the recorded reference (tests/golden/g22_roi_head.npz, written by
tools/gen_golden_roi_head.py from nerf_rpn/model/detector.py on the CPU in float64), and hand-checkable cases of its rules.  No GPU.

Continuous results agree to 1e-9 relative to the largest recorded entry (both sides are float64 arithmetic on the same fp32 inputs); discrete results exactly.
The oriented run also settles the enlarge_roi quirk: the RoIs the reference encoded and decoded against are the enlarged ones."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests import _roi_head_ref as H  # noqa: E402

GOLD = np.load(os.path.join(ROOT, "tests", "golden", "g22_roi_head.npz"))
CASES = [("a_", False), ("o_", True)]


def close(a, b, name):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (name, a.shape, b.shape)
    err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert err <= 1e-9, f"{name}: {err:.3e}"


def sampled(pre, rotated):
    rois, gts, labs, maps = H.gold_inputs(rotated)
    keep, n_fg = GOLD[pre + "keep"], GOLD[pre + "n_fg"]
    L, Ro, Gr, m = H.targets(rois, gts, labs, keep=keep, n_fg=n_fg)
    return rois, gts, labs, maps, torch.stack(L), torch.stack(Ro), torch.stack(Gr), m


@pytest.mark.parametrize("pre,rotated", CASES)
def test_inputs_are_the_recorded_ones(pre, rotated):
    rois, gts, _, maps = H.gold_inputs(rotated)
    assert tuple(GOLD[pre + "seeds"]) == H.GOLD_SEED[rotated]
    close(H.input_sums(rois, gts, maps), GOLD[pre + "input_sums"], "input sums")


@pytest.mark.parametrize("pre,rotated", CASES)
def test_targets(pre, rotated):
    rois, gts, labs, _ = H.gold_inputs(rotated)
    L, _, Gr, m = H.targets(rois, gts, labs)
    assert min(m["iou_fg"], m["iou_bg"], m["iou_top2"]) >= H.MARGIN
    assert np.array_equal(torch.cat(L).numpy().astype(np.int64), GOLD[pre + "eval_labels"])
    close(torch.cat(Gr).numpy(), GOLD[pre + "eval_gt_rois"], "evaluation gt_rois")
    _, _, _, _, L, _, Gr, m = sampled(pre, rotated)
    for i, (f, b) in enumerate(m["candidates"]):          # the recorded draw is a legal one
        k, n = GOLD[pre + "keep"][i], int(GOLD[pre + "n_fg"][i])
        assert set(k[:n]) <= set(f.tolist()) and len(set(k[:n])) == n and set(k[n:]) <= set(b.tolist())
    assert np.array_equal(L.numpy().astype(np.int64), GOLD[pre + "sample_labels"])
    close(Gr.numpy(), GOLD[pre + "sample_gt_rois"], "sampled gt_rois")


@pytest.mark.parametrize("pre,rotated", CASES)
def test_pooling(pre, rotated):
    _, _, _, maps, _, Ro, _, _ = sampled(pre, rotated)
    out, m, _ = H.pool(maps, Ro, out=H.GOLD["out"], rotated=rotated)
    assert m["floor"] >= H.MARGIN and m["cell_gap"] >= H.MARGIN and m["inside"] and m["padded_cells"] > 0 and m["ragged"] > 0
    close(out.numpy(), GOLD[pre + "pooled"], "pooled")
    if not rotated:
        kmin, kmax = H.mapper_range(H.SCALES)
        lv, lm = H.level_map(Ro[..., 1:], kmin, kmax, H.GOLD["max_res"], len(H.SCALES))
        assert lm >= H.MARGIN and np.array_equal(lv.reshape(-1).numpy(), GOLD[pre + "remap_levels"]) and len(set(lv.reshape(-1).tolist())) > 1
        out, m, _ = H.pool(maps, Ro, out=H.GOLD["out"], rotated=False, levels=lv)
        assert m["floor"] >= H.MARGIN
        close(out.numpy(), GOLD[pre + "pooled_remap"], "pooled with remap")


@pytest.mark.parametrize("pre,rotated", CASES)
def test_head_losses_targets_and_decode(pre, rotated):
    _, _, _, maps, L, Ro, Gr, _ = sampled(pre, rotated)
    B = 7 if rotated else 6
    ex = Ro[..., 1:].reshape(-1, B).clone()
    if rotated:                     # the reference's enlarge_roi wrote the enlarged sizes into the sampled RoIs before they were encoded
        assert not np.allclose(GOLD[pre + "encoded_rois"], ex.numpy(), rtol=1e-3, atol=0)
        ex[:, 3:6] *= 1 + H.ENLARGE
    close(ex.numpy(), GOLD[pre + "encoded_rois"], "the RoIs the reference encoded against")
    pooled, _, _ = H.pool(maps, Ro, out=H.GOLD["out"], rotated=rotated)
    hp = {k: v.double() for k, v in H.gold_head(rotated).items()}
    x = pooled.reshape(pooled.shape[0], -1)
    deltas, scores = x @ hp["RCNN_bbox_pred_w"].T + hp["RCNN_bbox_pred_b"], x @ hp["RCNN_cls_score_w"].T + hp["RCNN_cls_score_b"]
    r = H.loss(scores, deltas, L.reshape(-1), ex, Gr.reshape(-1, B), rotated)
    close(r["targets"].numpy(), GOLD[pre + "targets"], "regression targets")
    close([r["obj"].item(), r["reg"].item()], GOLD[pre + "losses"], "losses")
    boxes, _ = H.decode(deltas, ex, rotated)
    close(boxes.numpy(), GOLD[pre + "proposals"], "decoded proposals")
    close(torch.softmax(scores, 1).numpy(), GOLD[pre + "cls_prob"], "cls_prob")


def test_loss_gradients_are_autograd_s():
    g = torch.Generator().manual_seed(3)
    for rotated in (False, True):
        B = 7 if rotated else 6
        rois, gts, labs = H.make_scene(4, rotated, N=1, K=10, G=3)
        ex, gt = rois[0][:, 1:], gts[0][torch.arange(10) % 3]
        s = torch.randn((10, 3), generator=g, dtype=H.F64, requires_grad=True)
        d = (torch.randn((10, B), generator=g, dtype=H.F64) * 0.3).requires_grad_()
        lab = torch.tensor([0, 1, 2, -1, 0, 1, -1, 2, 0, 0.0])
        r = H.loss(s, d, lab, ex, gt, rotated)
        keep = lab >= 0
        want_obj = torch.nn.functional.cross_entropy(s[keep], lab[keep].long())
        pos = lab > 0
        want_reg = torch.nn.functional.smooth_l1_loss(d[pos], r["targets"][pos], beta=1 / 9, reduction="sum") / int(pos.sum())
        close([r["obj"].item(), r["reg"].item()], [want_obj.item(), want_reg.item()], "losses")
        gs, gd = torch.autograd.grad(want_obj + want_reg, (s, d))
        close(r["dscores"].detach().numpy(), gs.numpy(), "dscores")
        close(r["ddeltas"].detach().numpy(), gd.numpy(), "ddeltas")


# ---- the inputs of the GPU tests at real extents: conditions on the inputs, asserted on the restatement --------------------------------------------
@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_big_scenes_leave_at_most_three_percent_of_a_scene_undecided(rotated):
    """A row is decided if its max IoU keeps MARGIN from both thresholds and from the runner-up.  Measured with BIG_SEED = 0, rows per scene (2500, 1025, 1024,
    1, 0, 2049) against (130, 65, 64, 0, 1, 70) boxes.  Axis-aligned: within 1e-3 of a threshold 8, 5, 8, 0, -, 8 rows (at most 0.78 % of a scene), top-two gap
    below 1e-3 27, 6, 8, 0, -, 26 rows (at most 1.27 %), undecided 1.40 %, 1.07 %, 1.56 %, 0, -, 1.61 %.  Oriented: threshold 13, 6, 1, 0, -, 7 rows (at most
    0.59 %), gap 22, 10, 10, 0, -, 32 rows (at most 1.56 %), undecided 1.40 %, 1.56 %, 1.07 %, 0, -, 1.90 %.  The cap of 3 % is a condition on the inputs: a
    seed that exceeds it is replaced, the cap is not raised."""
    c = H.big_case(rotated)
    assert [r.shape[0] for r in c["rois"]] == list(H.BIG["counts"]) and [g.shape[0] for g in c["gts"]] == list(H.BIG["G"])
    assert max(H.BIG["counts"]) == H.BIG["cap"] and sorted(H.BIG["counts"])[:2] == [0, 1] and {1024, 1025, 2049} <= set(H.BIG["counts"])
    _, _, Gr, m = H.targets(c["rois"], c["gts"], c["labs"])
    near = dict(threshold=0, gap=0)
    for k, rm in zip(H.BIG["counts"], m["rows"]):
        assert rm["decided"].numel() == k
        if k == 0:
            continue
        thr, gap = (rm["d_fg"] < H.MARGIN) | (rm["d_bg"] < H.MARGIN), rm["gap"] < H.MARGIN
        assert torch.equal(~rm["decided"], thr | gap)
        share = float((~rm["decided"]).double().mean())
        print(f"rows {k}: threshold {int(thr.sum())} ({float(thr.double().mean()):.4f}), gap {int(gap.sum())} ({float(gap.double().mean()):.4f}), undecided {share:.4f}")
        assert share <= H.BIG["max_undecided"]
        near["threshold"] += int((rm["d_fg"] < H.MARGIN).sum())
        near["gap"] += int(gap.sum())
        assert (rm["arg2"][gap] != rm["arg"][gap]).all()
    assert near["threshold"] > 0 and near["gap"] > 0, "both kinds of near-tie occur, so the comparison of the undecided rows is exercised"
    # the scene without boxes and the scene without proposals
    i0, i1 = H.BIG["G"].index(0), H.BIG["counts"].index(0)
    assert m["rows"][i0]["best"].tolist() == [0.0] and m["rows"][i0]["arg"].tolist() == [0] and not Gr[i0].any() and Gr[i1].shape == (0, 7 if rotated else 6)
    # the kept rows of the GPU test come from both classes wherever a scene has both
    keep, n_fg = H.big_keep(m["candidates"])
    assert keep.shape == (6, H.BIG["R"]) and n_fg[0] == H.BIG["R"] // 2 and (keep[i1] == -1).all() and all((keep[i] < k).all() for i, k in enumerate(H.BIG["counts"]))
    alt = H.targets(c["rois"], c["gts"], c["labs"], keep=keep, n_fg=n_fg, rows=m["rows"], alt_arg=True)
    base = H.targets(c["rois"], c["gts"], c["labs"], keep=keep, n_fg=n_fg, rows=m["rows"])
    assert any(not torch.equal(a, b) for a, b in zip(alt[2], base[2])), "a kept row has a near-tie between two boxes"


def test_sampler_restatement_and_the_conditions_on_its_scenes():
    """every row of the sampling scenes is decided by construction (IoU 1, 0 or 1/3); the restated draw is a legal one; and the draws of scene 0 depend on
    the running counts of all three 1024-lane chunks"""
    c = H.sampler_case()
    _, _, _, m = H.targets(H.sampler_rois(c), c["gts"], c["labs"])
    assert all(bool(rm["decided"].all()) for rm in m["rows"])
    cand = m["candidates"]
    for (f, b), kind in zip(cand, c["kind"]):
        assert torch.equal(f, torch.nonzero(kind == 0).view(-1)) and torch.equal(b, torch.nonzero(kind == 1).view(-1))
    assert [(f.numel() > 0, b.numel() > 0) for f, b in cand] == [(True, True), (True, False), (False, True), (False, False), (True, True), (False, False)]
    assert c["counts"][-1] == 0 and c["counts"][3] > 0
    chunk = lambda q: min(int(q) // 1024, 2)          # noqa: E731
    f0, b0 = cand[0]
    assert {chunk(q) for q in f0} == {chunk(q) for q in b0} == {0, 1, 2} and b0.numel() > 1024
    assert {R > 1024 for R, _ in H.SAMPLER["runs"]} == {False, True}
    for R, want in H.SAMPLER["runs"]:
        for counter in H.SAMPLER["counters"]:
            for i, (f, b) in enumerate(cand):
                keep, (nf, nb), pos = H.sample(f, b, R, want, H.SAMPLER["seed"], counter, i)
                assert len(keep) == R and nf + nb == (R if f.numel() or b.numel() else 0)
                fl, bl = f.tolist(), b.tolist()
                if fl and bl:
                    assert nf == min(want, len(fl)) and keep[:nf] == sorted(set(keep[:nf])) and set(keep[:nf]) <= set(fl), "distinct, ascending, foreground"
                    assert all(0 <= p < len(bl) and k == bl[p] for k, p in zip(keep[nf:], pos[nf:])), "draws inside the background list"
                elif fl or bl:
                    lst = fl or bl
                    assert (nf, nb) == ((R, 0) if fl else (0, R)) and all(0 <= p < len(lst) and k == lst[p] for k, p in zip(keep, pos))
                    assert len(set(keep)) > R // 4, "with replacement, spread over the list"
                else:
                    assert keep == [-1] * R
                if i == 0:           # a cut, in every chunk: chosen and unchosen foreground rows on both sides of both chunk boundaries
                    assert want < len(fl)
                    chosen = set(keep[:nf])
                    assert {chunk(q) for q in chosen} == {chunk(q) for q in set(fl) - chosen} == {0, 1, 2}
                    assert max(pos[nf:]) >= 1024, "a background draw past the first 1024 list positions"
                if i == 4:           # fewer foreground rows than wanted: all of them, no cut
                    assert len(fl) < want and keep[:nf] == fl
            other = H.sample(f0, b0, R, want, H.SAMPLER["seed"], counter + 1, 0)[0]
            assert other != H.sample(f0, b0, R, want, H.SAMPLER["seed"], counter, 0)[0] != H.sample(f0, b0, R, want, H.SAMPLER["seed"], counter, 1)[0]
    # the hash on a hand-checked value: the splitmix64 finaliser of 1 (the published stream of seed 0 has 0x9E3779B97F4A7C15 added first)
    assert H.mix64(0x9E3779B97F4A7C15) == 0xE220A8397B1DCDAF
    assert H.sample_draw(0, 0, 7) == (H.mix64(0) >> 32) * 7 >> 32 == 0 and 0 <= H.sample_key(3, 5) < 1 << 32


@pytest.mark.parametrize("key", list(H.POOL_WIDE), ids=str)
def test_wide_pooling_cases_keep_their_margins(key):
    rotated, noncubic, C, out = key
    rois, maps = H.pool_case(key)
    _, m, _ = H.pool(maps, rois, out=out, rotated=rotated)
    assert m["floor"] >= H.MARGIN and m["cell_gap"] >= H.MARGIN, m
    assert m["padded_cells"] > 0 and m["ragged"] > 0 and (m["masked_points"] > 0 or not rotated)
    groups, cells = -(-C // 8), out[0] * out[1] * out[2]
    if C == 20:
        assert groups == 3 and C % 8 == 4 and np.isfinite(m["cell_gap"]), "a ragged last channel group, and cells with several points"
    else:
        assert -(-cells * groups // 256) == 3 and m["cell_gap"] == float("inf"), "three workgroups per RoI; at most one point per cell"


@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_four_level_pooling_case_keeps_its_margins(rotated):
    rois, maps = H.pool4_case(rotated)
    assert len(maps) == 4 and tuple(maps[3].shape[2:]) == (2, 2, 2) and (rois[..., 0] == 3).sum() >= 10
    _, m, _ = H.pool(maps, rois, scales=H.SCALES4, out=H.POOL4["out"], rotated=rotated)
    assert m["floor"] >= H.MARGIN and m["cell_gap"] >= H.MARGIN, m


@pytest.mark.parametrize("empty", [False, True], ids=["two-scenes", "with-an-empty-scene"])
@pytest.mark.parametrize("rotated", [False, True], ids=["aabb", "obb"])
def test_joined_case_keeps_its_margins(rotated, empty):
    """the inputs of tests/test_detector_joined_gpu.py: the first stage's decisions, the kept rows' IoU and pooling decisions and the decode's wrap keep their
    margins; every row keeps MARGIN from both IoU thresholds, so the candidate lists that the sampler's restatement draws from are exact"""
    from tests import _rpn_post_ref as P
    c = H.joined_case(rotated, empty)
    ch = H.joined_chain(c, rotated)
    assert not {k: v for k, v in c["marg"].items() if v < P.MARGIN}, c["marg"]
    assert [r.shape[0] for r in c["rois"]] == [100, 100] + [0] * empty and sum(min(H.JOIN["pre"], 13 * n) for n in (512, 64, 8, 1)) == H.JOIN["cap"]
    assert ch["pm"]["floor"] >= H.MARGIN and ch["pm"]["cell_gap"] >= H.MARGIN and ch["wrap"] >= H.MARGIN, (ch["pm"], ch["wrap"])
    assert all(bool(((rm["d_fg"] >= H.MARGIN) & (rm["d_bg"] >= H.MARGIN)).all()) for rm in c["rows"])
    assert all(bool(rm["decided"][k[k >= 0]].all()) for rm, k in zip(c["rows"], c["keep"]))
    assert all(f.numel() >= 3 and b.numel() > 50 for f, b in c["candidates"][:2]) and c["n_fg"][:2] == [c["R"] // 2] * 2
    assert len(set(ch["Ro"][..., 0].reshape(-1).tolist())) >= 3, "the kept rows mix the levels"
    assert float(ch["loss"]["obj"]) > 0 and float(ch["loss"]["reg"]) > 0 and all(d.abs().sum() > 0 for d in ch["dmaps"][:3])
    if empty:
        assert (c["keep"][2] == -1).all() and (ch["L"][2] == -1).all() and all(not d[2].any() for d in ch["dmaps"])


# ---- hand-checkable cases --------------------------------------------------------------------------------------------------------------------
def _one_map(values):
    return [torch.tensor(values, dtype=torch.float32).reshape(1, 1, *np.shape(values))]


def test_padded_max_pool_rule():
    """a 3 x 1 x 1 crop pooled to 2 x 1 x 1: k = 2, the second cell holds one voxel and one padding zero"""
    maps = _one_map(np.array([1.0, 5.0, -3.0, 7.0]).reshape(4, 1, 1))
    # box x in [0.2, 5.8]: half = 2.8 * 1.2 = 3.36, enlarged 3 -+ 1.68 = [1.32, 4.68], scale 2 -> floor 0 .. 2: voxels 0, 1, 2
    roi = torch.tensor([[[0.0, 0.2, 0.0, 0.0, 5.8, 1.0, 1.0]]])
    out, m, _ = H.pool(maps, roi, scales=(2,), out=(2, 1, 1), rotated=False)
    assert out.reshape(-1).tolist() == [5.0, 0.0], "a negative value overlapping the padding gives 0"
    assert m["padded_cells"] == 1
    maps = _one_map(np.array([1.0, 5.0, 3.0, 7.0]).reshape(4, 1, 1))
    assert H.pool(maps, roi, scales=(2,), out=(2, 1, 1), rotated=False)[0].reshape(-1).tolist() == [5.0, 3.0]
    # a crop smaller than the output: one voxel pooled to 2 cells, the second lies wholly in the padding
    roi = torch.tensor([[[0.0, 2.2, 0.0, 0.0, 3.0, 1.0, 1.0]]])
    out, _, _ = H.pool(_one_map(np.array([1.0, -5.0, 3.0, 7.0]).reshape(4, 1, 1)), roi, scales=(2,), out=(2, 1, 1), rotated=False)
    assert out.reshape(-1).tolist() == [-5.0, 0.0]          # s = 1, k = 1: cell 0 is voxel 1 = -5 without padding, cell 1 is padding only


def test_unpadded_cell_keeps_a_negative_maximum():
    roi = torch.tensor([[[0.0, 2.2, 0.0, 0.0, 3.0, 1.0, 1.0]]])      # enlarged [2.36, 2.84] / 2 -> voxel 1 only
    out, _, _ = H.pool(_one_map(np.array([1.0, -5.0, 3.0, 7.0]).reshape(4, 1, 1)), roi, scales=(2,), out=(1, 1, 1), rotated=False)
    assert out.reshape(-1).tolist() == [-5.0]


def test_eight_corner_weight_at_an_integer_point_and_off_it():
    f = np.arange(27, dtype=np.float64).reshape(3, 3, 3)
    maps = _one_map(f)
    # one point (sizes 0.5 * 1.2 / 1 -> ceil 1) at the integer position (1, 2, 1), theta 0: floor == ceil, all eight weights are 1, value = f / 8 * 8
    roi = torch.tensor([[[0.0, 1.0, 2.0, 1.0, 0.5, 0.5, 0.5, 0.0]]])
    out, _, _ = H.pool(maps, roi, scales=(1,), out=(1, 1, 1), rotated=True)
    assert out.item() == f[1, 2, 1]
    # at (1.5, 1, 1): corners x = 1 and 2, |dx| = 0.5, |dy| = |dz| = 0: weights 1 -> (4 f[1,1,1] + 4 f[2,1,1]) / 8
    roi = torch.tensor([[[0.0, 1.5, 1.0, 1.0, 0.5, 0.5, 0.5, 0.0]]])
    out, _, _ = H.pool(maps, roi, scales=(1,), out=(1, 1, 1), rotated=True)
    assert out.item() == (f[1, 1, 1] + f[2, 1, 1]) / 2
    # at (1.5, 1.5, 1.5): every weight is 1 - 1/8: NOT trilinear (which would weigh 1/8 each)
    roi = torch.tensor([[[0.0, 1.5, 1.5, 1.5, 0.5, 0.5, 0.5, 0.0]]])
    out, _, _ = H.pool(maps, roi, scales=(1,), out=(1, 1, 1), rotated=True)
    assert abs(out.item() - f[1:3, 1:3, 1:3].sum() * (1 - 0.125) / 8) < 1e-12
    # a point outside [0, size - 1] is zeroed
    roi = torch.tensor([[[0.0, 2.5, 1.0, 1.0, 0.5, 0.5, 0.5, 0.0]]])
    out, m, _ = H.pool(maps, roi, scales=(1,), out=(1, 1, 1), rotated=True)
    assert out.item() == 0.0 and m["masked_points"] == 1


def test_decode_clip_and_wrap():
    ex = torch.tensor([[10.0, 10, 10, 4, 4, 4, 0.3]] * 3, dtype=H.F64)
    d = torch.zeros((3, 7), dtype=H.F64)
    d[0, 3] = 50.0                                   # clipped at log 2000
    d[1, 6] = (1.7 - 0.3) / (2 * np.pi)              # 1.7 > pi/2 -> 1.7 - pi
    d[2, 6] = (-1.7 - 0.3) / (2 * np.pi)             # -1.7 -> pi - 1.7
    boxes, margin = H.decode(d, ex, True)
    assert abs(boxes[0, 3].item() - 8000.0) < 1e-6 and margin > 0.1
    assert abs(boxes[1, 6].item() - (1.7 - np.pi)) < 1e-12 and abs(boxes[2, 6].item() - (np.pi - 1.7)) < 1e-12
