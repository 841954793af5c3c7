"""The float64 restatement of the RPN inference path (tests/_rpn_post_ref.py) against decoded boxes and proposals recorded from the reference's own
Python (tests/golden/g21_rpn_proposals.npz, tools/gen_golden_rpn_post.py), the decision margins that make exact comparisons of the discrete outputs
defined, known answers of both decoders and of the selection rules, and the C ABI.  No GPU."""
import functools
import math
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _rpn_post_ref as P  # noqa: E402
from tests import _rpn_ref as R  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

NAMES = ("nmh_rpn_post_cap", "nmh_rpn_post_mask_words", "nmh_rpn_decode", "nmh_rpn_post_select", "nmh_rpn_post_nms")
CASES = (("a_", False), ("o_", True))


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g21_rpn_proposals.npz")))


@functools.lru_cache(maxsize=None)
def case(rotated):
    obj, reg = P.inputs(P.HEAD_SEED[rotated], rotated)
    return (obj, reg) + P.proposals(obj, reg, ori=R.ORI, rotated=rotated, **P.CFG)


def test_header_declares_and_capi_defines_the_rpn_post_entries():
    from nerf_mae_amd._lib import parse_header
    sigs = parse_header()
    capi = open(os.path.join(ROOT, "nerf-mae_amd", "csrc", "capi.hip")).read()
    for n in NAMES:
        assert n in sigs, n
        ret, args = sigs[n]
        assert re.search(r"^(int|int64_t)\s+" + n + r"\s*\(", capi, re.M), f"capi.hip does not define {n}"
        if ret == "int":
            assert args[-1] == ("void*", "stream"), (n, args[-1])
    assert [a for _, a in sigs["nmh_rpn_post_select"][1][:6]] == ["nlevels", "level_dims", "base_half", "N", "ncols", "pre_nms_top_n"]
    assert [a for _, a in sigs["nmh_rpn_post_nms"][1][-6:-1]] == ["boxes", "scores", "levels", "index", "counts"]


def test_restatement_against_the_recorded_reference():
    g = golden()
    assert g["mesh"].tolist() == list(R.MESH) and g["ori"].tolist() == [list(o) for o in R.ORI] and g["grids"].tolist() == [list(v) for v in R.GRIDS]
    assert (int(g["pre_nms_top_n"]), int(g["post_nms_top_n"]), float(g["nms_thresh"]), float(g["score_thresh"])) == tuple(P.CFG[k] for k in
                                                                                                                       ("pre_nms_top_n", "post_nms_top_n", "nms_thresh", "score_thresh"))
    for pre, rotated in CASES:
        obj, reg, res, marg = case(rotated)
        assert int(g[pre + "head_seed"]) == P.HEAD_SEED[rotated]
        sums = [sum(t.double().sum().item() for t in ts) for ts in (obj, reg)]
        assert np.allclose(sums, g[pre + "head_sums"], rtol=1e-12), "the head generator drifted from the one that was recorded"
        dec = P.decode_all(reg, rotated)
        assert_close(dec[:, torch.from_numpy(g[pre + "d_index"]).long()], torch.from_numpy(g[pre + "d_boxes"]).double(), 1e-6, pre + "decode_list")
        # counts, levels, anchor indices and order: exact
        assert [len(r["scores"]) for r in res] == g[pre + "counts"].tolist()
        assert torch.cat([r["level"] for r in res]).tolist() == g[pre + "level"].tolist()
        assert torch.cat([r["index"] for r in res]).tolist() == g[pre + "index"].tolist()
        assert_close(torch.cat([r["boxes"] for r in res]), torch.from_numpy(g[pre + "boxes"]), 1e-6, pre + "boxes")
        assert_close(torch.cat([r["scores"] for r in res]), torch.from_numpy(g[pre + "scores"]), 1e-6, pre + "scores")


def test_every_decision_has_a_margin_and_the_recorded_case_is_not_trivial():
    for rotated in (False, True):
        _, _, res, marg = case(rotated)
        for k, v in marg.items():
            assert v >= P.MARGIN, (rotated, k, v)
        assert math.isinf(marg["m_score"]) and (math.isinf(marg["m_swap"]) != rotated)
        for r in res:
            assert 0 < len(r["scores"]) == P.CFG["post_nms_top_n"] < len(r["pre_scores"])               # NMS and the cut both do real work
            assert len(set(r["level"].tolist())) >= 3
            assert (r["scores"][:-1] >= r["scores"][1:]).all()
        assert res[1]["unmasked"][0] < 8 ** 3 * 13 and res[0]["unmasked"][0] == 8 ** 3 * 13                # the second scene is padded


def test_known_answers():
    anc = torch.tensor([[-4.0, -4, -4, 4, 4, 4]], dtype=P.F64)
    z6, z8 = torch.zeros((1, 6), dtype=P.F64), torch.zeros((1, 8), dtype=P.F64)
    assert torch.equal(P.decode_aabb(z6, anc), anc)
    d = z6.clone(); d[0, 0] = 0.25; d[0, 3] = math.log(0.5); d[0, 5] = 100.0
    b = P.decode_aabb(d, anc)[0]
    assert np.allclose(b.numpy(), [0, -4, -8000, 4, 4, 8000])                       # dd clamped at log(2000): depth 8 * 2000
    # zero deltas: the midpoints form a diamond, scaled to itself; the first edge runs from (0, -4) to (4, 0): theta = -pi/4 (or, swapped, pi/4), sides 4 sqrt(2)
    o, swap, wrap = P.decode_obb(z8, anc, True)
    assert np.allclose(o[0, :6].numpy(), [0, 0, 0, 4 * math.sqrt(2), 4 * math.sqrt(2), 8], atol=1e-6) and swap[0] < 1e-6      # a square: the swap is open
    assert min(abs(o[0, 6].item() + math.pi / 4), abs(o[0, 6].item() - (P.REF_PI / 2 - math.pi / 4))) < 1e-6
    # da = db = 0.5 (clamped from 3): the anchor's own BEV rectangle, and the widths clamp at |log(0.016)|
    d = z8.clone(); d[0, 6] = d[0, 7] = 3.0; d[0, 3] = -100.0; d[0, 4] = 1.0
    o = P.decode_obb(d, anc)[0]
    assert np.allclose(sorted(o[3:5].tolist()), sorted([8 * 0.016, 8 * math.e]), rtol=1e-6) and o[3] > o[4] and -P.REF_PI / 2 <= o[6] < P.REF_PI / 2
    # the order of the bits: -inf < -1 < -0 < +0 < 1 < inf, NaN as -inf, all above the masked key 0 and the fill key 1
    x = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], dtype=np.float32)
    k = P.order_keys(x)
    assert (np.diff(k[:6]) > 0).all() and k[6] == k[0] == 0x007FFFFF and k.min() > 1
    # one level of 2 x 1 x 1 locations and one anchor: the masked anchor is still selected when the cut asks for it, with score 0, last
    one = dict(mesh=(8, 4, 4), grids=((2, 1, 1),), base=[np.array([[-2.0, -2, -2, 2, 2, 2]])])
    obj, reg = [torch.tensor([-3.0, 5.0]).reshape(1, 1, 2, 1, 1)], [torch.zeros((1, 6, 2, 1, 1))]
    res, _ = P.proposals(obj, reg, ori=[(4, 4, 4)], pre_nms_top_n=2, post_nms_top_n=2, **one)
    assert res[0]["index"].tolist() == [0, 1] and res[0]["scores"].tolist() == [torch.sigmoid(torch.tensor(-3.0, dtype=P.F64)).item(), 0.0]
    res, _ = P.proposals(obj, reg, ori=[(4, 4, 4)], pre_nms_top_n=1, post_nms_top_n=2, **one)
    assert res[0]["index"].tolist() == [0]
    # equal logits: the cut goes to the lower memory offset, (a, w, h, d) order, not to the lower anchor index
    two = dict(mesh=(8, 4, 4), grids=((2, 1, 1),), base=[np.array([[-2.0, -2, -2, 2, 2, 2], [-1.0, -1, -1, 1, 1, 1]])])
    obj, reg = [torch.zeros((1, 2, 2, 1, 1))], [torch.zeros((1, 12, 2, 1, 1))]
    res, _ = P.proposals(obj, reg, pre_nms_top_n=2, post_nms_top_n=4, nms_thresh=1.0, **two)
    assert sorted(res[0]["index"].tolist()) == [0, 2]                                # anchor a = 0 at both locations: offsets 0 and 1, anchor indices 0 and 2
