"""The float64 restatement of the FCOS assignment and losses (tests/_fcos_ref.py) against labels, targets, losses and gradients recorded from
the reference's own Python (tests/golden/g18_fcos_loss.npz, tools/gen_golden_fcos.py), the decision margins that make exact comparisons of
labels and indices defined, and known answers.  No GPU."""
import functools
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _fcos_ref as F  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

CASES = (("a_", False, "giou", False), ("o_", True, "iou", True))


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g18_fcos_loss.npz")))


@functools.lru_cache(maxsize=None)
def asg(use_obb, radius, norm):
    return F.assign(F.make_scene(F.SEED[use_obb], use_obb), radius, norm, orig=F.ORIG)


def test_restatement_against_the_recorded_reference():
    g = golden()
    radius, norm = float(g["radius"]), bool(g["norm"])
    assert int(g["head_seed"]) == F.HEAD_SEED
    for pre, use_obb, loss_type, add_l1 in CASES:
        boxes = F.make_scene(F.SEED[use_obb], use_obb)
        assert np.array_equal(torch.cat(boxes).numpy(), g[pre + "boxes"]) and g[pre + "offsets"].tolist() == [0, 70, 71, 71]
        cls, reg, ctr = F.make_heads(F.HEAD_SEED, use_obb, norm)
        sums = [sum(t.double().sum().item() for t in ts) for ts in (cls, reg, ctr)]
        assert np.allclose(sums, g[pre + "head_sums"], rtol=1e-12), "the head generator drifted from the one that was recorded"
        a = asg(use_obb, radius, norm)
        assert torch.equal(a["labels"], torch.from_numpy(g[pre + "labels"]).double())
        # without a winner the reference leaves the (never used) targets of box 0 in place; the stated semantics give zeros there
        pos = a["labels"] > 0
        assert_close(a["targets"][pos], torch.from_numpy(g[pre + "reg_targets"]).double()[pos], 1e-4, pre + "reg_targets")
        assert a["targets"][~pos].abs().sum() == 0
        heads = [[t.double().requires_grad_(True) for t in ts] for ts in (cls, reg, ctr)]
        out = F.losses(*heads, a, loss_type, add_l1)
        sum(out).backward()
        assert_close(torch.stack([o.detach() for o in out]), torch.from_numpy(g[pre + "losses"]).double(), 1e-4, pre + "losses")
        grads = F.flatten_heads(*[[t.grad for t in ts] for ts in heads])
        for name, v in zip(("grad_cls", "grad_reg", "grad_ctr"), grads):
            assert_close(v, torch.from_numpy(g[pre + name]).double(), 1e-4, pre + name)


def test_every_decision_has_a_margin():
    for use_obb in (False, True):
        for radius in (0.0, 1.5):
            a = asg(use_obb, radius, True)
            for k, v in F.decision_margins(a).items():
                assert v >= 1e-3, (use_obb, radius, k, v)
            assert a["npos"] > 100
            # every level has positives, some locations had more than one candidate, and padded locations exist
            off = np.cumsum([0] + [3 * w * l * h for w, l, h in F.SIZES])
            assert all(a["labels"][off[k]:off[k + 1]].sum() > 0 for k in range(4)), [a["labels"][off[k]:off[k + 1]].sum().item() for k in range(4)]
            assert a["m_vol"] < math.inf and 0.05 < (~a["valid"]).double().mean().item() < 0.5
        for norm in (False, True):
            reg = F.make_heads(F.HEAD_SEED, use_obb, norm)[1]
            assert F.clamp_margin(reg, asg(use_obb, 1.5, norm)) >= 1e-3
    reg = F.make_heads(F.HEAD_SEED, True, True)[1]
    r = F.flatten_heads(reg, reg, reg)[1]
    assert all(0.03 < ((s * r[:, k]) > 0.5).double().mean().item() < 0.1 for k in (6, 7) for s in (-1, 1))     # all four clamp sides occur


def test_known_answers():
    one = dict(sizes=((1, 1, 1),), strides=(4,))
    # the location (2,2,2) at the centre of its box: centerness 1, targets = half sizes
    a = F.assign([torch.tensor([[0.5, 1.0, -1.0, 3.5, 3.0, 5.0]])], 0.0, False, **one)
    assert a["labels"].tolist() == [1.0] and a["ctr"].item() == 1.0 and a["targets"][0].tolist() == [1.5, 1.0, 3.0, 1.5, 1.0, 3.0]
    # two boxes of equal volume: the lower index wins; a smaller one wins whatever its index
    b1, b2 = [0.0, 0.0, 0.0, 4.0, 4.0, 8.0], [0.0, 0.0, 0.0, 8.0, 4.0, 4.0]
    assert F.assign([torch.tensor([b1, b2])], 0.0, False, **one)["gt_index"].tolist() == [0]
    assert F.assign([torch.tensor([b2, b1])], 0.0, False, **one)["gt_index"].tolist() == [0]
    assert F.assign([torch.tensor([b1, [1.0, 1.0, 1.0, 3.0, 3.0, 3.0]])], 0.0, False, **one)["gt_index"].tolist() == [1]
    # strict in-box test, inclusive range: a face through the location excludes it; max distance exactly 16 is still level 0
    assert F.assign([torch.tensor([[2.0, 0.0, 0.0, 4.0, 4.0, 4.0]])], 0.0, False, **one)["labels"].tolist() == [0.0]
    assert F.assign([torch.tensor([[1.0, 1.0, 1.0, 18.0, 3.0, 3.0]])], 0.0, False, **one)["labels"].tolist() == [1.0]
    assert F.assign([torch.tensor([[1.0, 1.0, 1.0, 18.5, 3.0, 3.0]])], 0.0, False, **one)["labels"].tolist() == [0.0]
    # an empty scene: all-zero targets
    e = F.assign([torch.zeros((0, 7))], 1.5, True)
    assert e["labels"].abs().sum() == 0 and e["targets"].abs().sum() == 0 and e["ctr"].abs().sum() == 0 and (e["gt_index"] == -1).all() and e["npos"] == 0
    # the theta == 0 boxes of the generator take the AABB fallback: alpha = 0.5, beta = -0.5
    g = F.gt_prepare(F.make_scene(F.SEED[True], True)[0].double())
    assert torch.equal(g["alpha"][:4], torch.full((4,), 0.5, dtype=F.F64)) and torch.equal(g["beta"][:4], torch.full((4,), -0.5, dtype=F.F64))


def test_decode_inverts_encode():
    rng = np.random.default_rng(3)
    n = 200
    size = rng.uniform(1, 20, (n, 3))
    th = rng.uniform(0.15, math.pi / 2 - 0.15, (n, 1))                  # non-degenerate: away from the near-AABB rule
    boxes = torch.from_numpy(np.concatenate([rng.uniform(20, 60, (n, 3)), size, th], 1))
    locs = torch.from_numpy(rng.uniform(0, 80, (n, 3)))
    back = F.decode(locs, F.encode(locs, boxes))
    # the decode names the sides by its own convention: the rectangle is the same when (w, l, theta) -> (l, w, theta -+ pi/2)
    same = (back[:, :3] - boxes[:, :3]).abs().max().item() < 1e-6
    assert same
    c1, c2 = F.R.corners(boxes), F.R.corners(back)
    d = (c1[:, :, None, :] - c2[:, None, :, :]).norm(dim=-1).amin(-1).max().item()       # every corner of one is a corner of the other
    assert d < 1e-5, d
    assert (back[:, 5] - boxes[:, 5]).abs().max().item() < 1e-9
