"""The float64 restatement of the RPN assignment, encodes, count rule and losses (tests/_rpn_ref.py) against labels, matched boxes, encoded targets
and losses recorded from the reference's own Python (tests/golden/g20_rpn_targets.npz, tools/gen_golden_rpn.py), the decision margins that make
exact comparisons of labels and indices defined, the host-side anchor generator against the recorded table, and the C ABI.  No GPU."""
import functools
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

NAMES = ("nmh_rpn_num_blocks", "nmh_rpn_assign", "nmh_rpn_sample", "nmh_rpn_loss_fwd", "nmh_rpn_loss_bwd")
CASES = (("a_", False), ("o_", True))


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g20_rpn_targets.npz")))


@functools.lru_cache(maxsize=None)
def asg(rotated):
    return R.assign(R.make_scene(R.SEED[rotated], rotated=rotated, ori=R.ORI), ori=R.ORI, rotated=rotated)


def test_header_declares_and_capi_defines_the_rpn_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    capi = open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "capi.hip")).read()
    for n in NAMES:
        assert n in sigs, n
        ret, args = sigs[n]
        assert re.search(r"^(int|int64_t)\s+" + n + r"\s*\(", capi, re.M), f"capi.hip does not define {n}"
        if n != "nmh_rpn_num_blocks":
            assert ret == "int" and args[-1] == ("void*", "stream"), (n, ret, args[-1])
    assert [a for _, a in sigs["nmh_rpn_assign"][1][:5]] == ["nlevels", "level_dims", "base_half", "N", "ncols"]
    assert [a for _, a in sigs["nmh_rpn_sample"][1][-4:-1]] == ["rng_state", "flags", "counts"]
    assert [a for _, a in sigs["nmh_rpn_loss_bwd"][1][-3:-1]] == ["dobj", "dreg"]


def test_anchor_table_and_generator_against_the_recorded_reference():
    from nerf_mae_amd.rpn import AnchorGenerator3D
    g = golden()
    base = R.base_anchors()
    assert np.array_equal(np.concatenate(base), g["base"].astype(np.float64)) and [len(b) for b in base] == g["base_counts"].tolist()
    gen = AnchorGenerator3D(R.ANCHOR_SIZES, R.ASPECT_RATIOS, is_normalized=False)
    assert gen.num_anchors_per_location() == g["num_anchors"].tolist() == [13] * 4
    N = len(R.NBOX)
    meshes, features = torch.zeros((N, 4, *R.MESH)), [torch.zeros((N, 1, *s)) for s in R.GRIDS]
    anchors, non_cat = gen(meshes, features)
    assert np.array_equal(torch.cat(gen.cell_anchors).numpy(), g["base"])
    assert len(anchors) == N and len(non_cat) == N and len(non_cat[0]) == len(R.GRIDS)
    assert all(torch.equal(a.double(), torch.from_numpy(R.anchors())) for a in anchors)
    assert [h for lvl in gen.half_extents() for h in lvl] == g["base"][:, 3:].tolist()
    masks = gen.get_padding_masks(meshes, features, R.ORI)
    assert [tuple(m.shape) for m in masks] == [(N, 13, *s) for s in R.GRIDS] and all(m.dtype == torch.bool for m in masks)
    flat = torch.cat([m.permute(0, 2, 3, 4, 1).reshape(N, -1) for m in masks], 1)
    assert all(np.array_equal(flat[i].numpy(), R.valid_mask(R.ORI[i])) for i in range(N))
    # round half to even: sizes 1 and 3 halve to .5 and 1.5
    odd = AnchorGenerator3D(((1, 3, 5),), (((1., 1., 1.),),)).generate_anchors((1, 3, 5), ((1., 1., 1.),))
    assert odd[:, 3].tolist() == [0.0, 2.0, 2.0]


def test_restatement_against_the_recorded_reference():
    g = golden()
    assert (float(g["fg"]), float(g["bg"]), int(g["batch"]), float(g["fraction"])) == (np.float32(R.FG), np.float32(R.BG), R.BATCH, R.FRACTION)
    assert g["ori"].tolist() == [list(o) for o in R.ORI] and g["mesh"].tolist() == list(R.MESH) and int(g["head_seed"]) == R.HEAD_SEED
    for pre, rotated in CASES:
        boxes = R.make_scene(R.SEED[rotated], rotated=rotated, ori=R.ORI)
        assert np.array_equal(torch.cat(boxes).numpy(), g[pre + "boxes"]) and g[pre + "offsets"].tolist() == [0, 5, 8]
        a = asg(rotated)
        C = 8 if rotated else 6
        assert torch.equal(a["labels"], torch.from_numpy(g[pre + "labels"]).double())
        assert torch.equal(a["matched"].clamp(min=0), torch.from_numpy(g[pre + "matched_row"]).long())
        idx = torch.from_numpy(g[pre + "t_index"]).long()
        assert_close(a["targets"].reshape(-1, C)[idx], torch.from_numpy(g[pre + "targets"]).double(), 1e-6, pre + "targets")
        flags = R.make_flags(int(g["flag_seed"]), a["labels"])
        assert torch.equal(flags, torch.from_numpy(g[pre + "flags"]))
        obj, reg = R.make_heads(R.HEAD_SEED, len(boxes), C)
        sums = [sum(t.double().sum().item() for t in ts) for ts in (obj, reg)]
        assert np.allclose(sums, g[pre + "head_sums"], rtol=1e-12), "the head generator drifted from the one that was recorded"
        out = R.losses([t.double() for t in obj], [t.double() for t in reg], flags, a["targets"])
        assert_close(torch.stack(out), torch.from_numpy(g[pre + "losses"]).double(), 1e-6, pre + "losses")


def test_every_decision_has_a_margin_and_every_kind_of_anchor_occurs():
    for rotated in (False, True):
        a = asg(rotated)
        m = R.decision_margins(a)
        assert set(m) == {"m_thr", "m_gt", "m_anc"} | ({"m_tol"} if rotated else set())
        for k, v in m.items():
            assert v >= 1e-3, (rotated, k, v)
        lab, mt, valid, restored = a["labels"], a["matched"], a["valid"], a["restored"]
        assert ((lab == 1) & ~restored).sum() > 0, "no plain positive"
        assert ((mt == -2) & valid).sum() > 0 and (lab[(mt == -2) & valid] == -1).all(), "no between-thresholds anchor"
        assert restored.sum() > 0 and (lab[restored] == 1).all() and (mt[restored] >= 0).all(), "no low-quality restore"
        assert (~valid).sum() > 0 and (lab[~valid] == -1).all() and (mt[~valid] == -1).all() and valid[0].all(), "no padded anchor"
        assert all((gm > 0).all() for gm in a["gtmax"]) and torch.isfinite(a["targets"]).all()


def test_known_answers():
    one = dict(mesh=(8, 8, 8), grids=((1, 1, 1),), base=[np.array([[-4.0, -4, -4, 4, 4, 4]])])
    # the anchor itself: IoU 1, zero targets; half of it: IoU 0.5, dx = 0.25, dw = log(0.5)
    a = R.assign([np.array([[-4.0, -4, -4, 4, 4, 4], ])], **one)
    assert a["labels"].tolist() == [[1.0]] and a["matched"].tolist() == [[0]] and a["targets"].abs().sum() == 0
    a = R.assign([np.array([[0.0, -4, -4, 4, 4, 4]])], fg=0.7, bg=0.6, **one)
    assert a["labels"].tolist() == [[1.0]] and bool(a["restored"][0, 0]), "the only anchor is the box's best: restored although below bg"
    assert np.allclose(a["targets"][0, 0].numpy(), [0.25, 0, 0, np.log(0.5), 0, 0])
    # two identical boxes: the lower index; no boxes: label 0, matched -1, zero targets
    b = [0.0, -4, -4, 4, 4, 4]
    assert R.assign([np.array([b, b])], **one)["matched"].tolist() == [[0]]
    e = R.assign([np.zeros((0, 6))], **one)
    assert e["labels"].tolist() == [[0.0]] and e["matched"].tolist() == [[-1]] and e["targets"].abs().sum() == 0
    # an axis-aligned oriented box: ga = xmax, gb = ymax of the corner pair -> da = db = 0.5
    t = R.encode_obb(np.array([[0.0, 0, 0, 4, 2, 8, 0.0]]), np.array([[-4.0, -4, -4, 4, 4, 4]]))
    assert np.allclose(t[0], [0, 0, 0, np.log(0.5), np.log(0.25), 0, 0.5, 0.5])
    # the count rule: too few positives, too few negatives
    lab = torch.tensor([[1.0] * 3 + [0.0] * 400 + [-1.0] * 5, [1.0] * 300 + [0.0] * 10 + [-1.0] * 98])
    assert R.sample_counts(lab) == [(3, 253), (128, 10)]
    f = R.make_flags(0, lab)
    assert [(int((r == 1).sum()), int((r == 2).sum())) for r in f] == [(3, 253), (128, 10)] and (f[lab == -1] == 0).all()
    assert (lab[f == 1] == 1).all() and (lab[f == 2] == 0).all()
