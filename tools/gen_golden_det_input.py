"""Records tests/golden/g25_det_input.npz from the reference's own detection input pipeline (nerf_rpn/datasets.py), run on the CPU.
    python tools/gen_golden_det_input.py --reference PATH_TO_REFERENCE_CHECKOUT
    python tools/gen_golden_det_input.py --search [N]   (no reference needed: prints what the restatement draws for seeds below N)

Every case writes its seeded scene (tests/_det_input_ref.make_scene) as an .npz and its boxes as an .npy into a temporary directory and loads them with
BaseDataset.load_single_scene, so the /255, the density->alpha and the transpose are the reference's.  Inputs are NOT stored: the file carries their sums.

Small cases (_det_input_ref.SMALL): BaseDataset.augment_rpn_inputs under random.seed(seed) with _det_input_ref.PROBS, once with 6-column and once with
7-column boxes.  The draw is read off the run, not re-derived: rotate_and_scale_scene is wrapped to record (angle, scale) and the grid it was given, the
flags are the one combination of rot / flips that maps the input grid onto that grid bit for bit, and random.random / random.uniform are counted.
Stored: the output grid, the output boxes, (flags, taken, angle, scale, rng calls), and e_ref = max |reference fp32 - restatement float64| for grid and
boxes separately.  The draws of seeds 0 .. DRAW_SEEDS-1 on a tiny scene are stored the same way (draws6, draws7).

Large cases (_det_input_ref.LARGE): the draw is fixed (LARGE_DRAW), fed to augment_rpn_inputs through a scripted random.random / random.uniform.  Stored:
e_ref, the float64 sum of the output and a strided sample of 4096 values.

Conditions on the seeds, asserted here from the restatement (tests/_det_input_ref.py), never from code under test: every flag occurs set and clear; rot-scale
occurs taken and not taken, with both signs of the angle, with scale < 0.95 and with scale > 1.05; one case has voxels with some taps out of range and
voxels with all taps out of range; one rotated case has W != L."""
import argparse
import importlib.util
import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _det_input_ref as D  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "g25_det_input.npz")


def conditions(draws):
    """draws: [(shape, flags, taken, angle, scale)] of the 7-column small runs -> asserts the conditions of the docstring"""
    for f in (D.ROT, D.FLIP0, D.FLIP1):
        assert {bool(d[1] & f) for d in draws} == {True, False}, f
    rs = [d for d in draws if d[2]]
    assert len(rs) and len(rs) < len(draws)
    assert any(d[3] > 0 for d in rs) and any(d[3] < 0 for d in rs)
    assert any(d[4] < 0.95 for d in rs) and any(d[4] > 1.05 for d in rs)
    assert any(d[1] & D.ROT and d[0][0] != d[0][1] for d in draws)
    edge = False
    for shape, flags, taken, angle, scale in rs:
        _, counts = D.resample(np.zeros((1,) + D.extents(shape, flags)), angle, scale, want_counts=True)
        edge = edge or (bool((counts == 0).any()) and bool(((counts > 0) & (counts < 8)).any()))
    assert edge


def search(limit):
    for seed in range(limit):
        out = []
        for oriented in (False, True):
            flags, taken, angle, scale, n = D.draw(rng=random.Random(seed), oriented=oriented, **D.PROBS)
            out.append(f"flags {flags} taken {int(taken)} angle {angle:+.4f} scale {scale:.4f} calls {n}")
        print(f"seed {seed}: 6 columns: {out[0]} | 7 columns: {out[1]}")
    try:
        conditions([(shape,) + D.draw(rng=random.Random(seed), oriented=True, **D.PROBS)[:4] for _, seed, shape, _ in D.SMALL])
        print("SMALL meets the conditions")
    except AssertionError as e:
        print("SMALL does not meet the conditions:", repr(e))


def load_reference(ref):
    spec = importlib.util.spec_from_file_location("ref_datasets", os.path.join(ref, "nerf_rpn", "datasets.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Run:
    """one call of the reference's augment_rpn_inputs, observed"""

    def __init__(self, M, script=None):
        self.M, self.script = M, script

    def __call__(self, grid, boxes):
        M, seen = self.M, dict(calls=0, rs=None)
        rs0, rnd0, uni0 = M.rotate_and_scale_scene, random.random, random.uniform
        script = list(self.script) if self.script is not None else None

        def rs(g, b, angle, scale):
            seen["rs"] = (g.clone(), angle, scale)
            return rs0(g, b, angle, scale)

        def rnd():
            seen["calls"] += 1
            return script.pop(0) if script is not None else rnd0()

        def uni(a, b):
            seen["calls"] += 1
            return script.pop(0) if script is not None else uni0(a, b)
        M.rotate_and_scale_scene, random.random, random.uniform = rs, rnd, uni
        try:
            og, ob = M.BaseDataset.augment_rpn_inputs(grid, boxes, D.PROBS["flip_prob"], D.PROBS["rotate_prob"], D.PROBS["rot_scale_prob"], True)
        finally:
            M.rotate_and_scale_scene, random.random, random.uniform = rs0, rnd0, uni0
        pre = seen["rs"][0] if seen["rs"] is not None else og
        hits = [f for f in range(8) if pre.shape == D.rot_flip(grid.numpy(), f).shape and np.array_equal(pre.numpy(), D.rot_flip(grid.numpy(), f))]
        assert len(hits) == 1, hits
        taken = seen["rs"] is not None
        angle, scale = (seen["rs"][1], seen["rs"][2]) if taken else (0.0, 1.0)
        return og.contiguous().numpy(), ob.numpy(), (hits[0], taken, float(angle), float(scale), seen["calls"])


def load(M, tmp, name, scene, boxes):
    np.savez(os.path.join(tmp, name + ".npz"), rgbsigma=scene)
    np.save(os.path.join(tmp, name + ".npy"), boxes)
    ds = M.BaseDataset(features_path=tmp, boxes_path=tmp, normalize_density=scene.dtype != np.uint8)     # uint8 scenes carry alpha already (the /255 branch)
    _, grid, b = ds.load_single_scene(name)
    return grid, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", help="checkout of the reference project")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--search", type=int, nargs="?", const=32, help="print the restatement's draws for the seeds below N")
    args = ap.parse_args()
    if args.search:
        return search(args.search)
    M = load_reference(args.reference)
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    rec, draws7 = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        for name, seed, shape, dtype in D.SMALL:
            scene = D.make_scene(seed, shape, dtype)
            rec[name + "_input_sum"] = np.float64(scene.astype(np.float64).sum())
            for cols in (6, 7):
                boxes = D.make_boxes(seed, shape, cols)
                grid, b = load(M, tmp, f"{name}_{cols}", scene, boxes)
                random.seed(seed)
                og, ob, dr = Run(M)(grid, b)
                flags, taken, angle, scale, calls = dr
                assert dr == tuple(D.draw(rng=random.Random(seed), oriented=cols == 7, **D.PROBS)), (name, cols, dr)
                want_g, want_b = D.prepare(scene, flags, taken, angle, scale), D.boxes_augment(boxes, shape, flags, taken, angle, scale)
                assert og.dtype == np.float32 and ob.dtype == np.float32 and og.shape == want_g.shape
                pre = f"{name}_{cols}_"
                rec[pre + "grid"], rec[pre + "boxes"] = og, ob
                rec[pre + "draw"] = np.array([flags, taken, angle, scale, calls], dtype=np.float64)
                rec[pre + "e_ref_grid"] = np.float64(np.abs(og - want_g).max())
                rec[pre + "e_ref_boxes"] = np.float64(np.abs(ob - want_b).max())
                print(pre, dr, "e_ref grid %.3e boxes %.3e" % (rec[pre + "e_ref_grid"], rec[pre + "e_ref_boxes"]))
                if cols == 7:
                    draws7.append((shape, flags, taken, angle, scale))
        conditions(draws7)
        tiny = np.arange(3 * 2 * 2 * 4, dtype=np.uint8).reshape(3, 2, 2, 4)
        for cols in (6, 7):
            grid, b = load(M, tmp, f"tiny_{cols}", tiny, D.make_boxes(0, (3, 2, 2), cols, n=1))
            rows = []
            for seed in range(D.DRAW_SEEDS):
                random.seed(seed)
                rows.append(Run(M)(grid, b)[2])
            rec[f"draws{cols}"] = np.array(rows, dtype=np.float64)
        assert (rec["draws6"][:, 4] == 3).all() and set(rec["draws7"][:, 4]) == {4.0, 6.0}
        for name, seed, shape, dtype in D.LARGE:
            scene, boxes = D.make_scene(seed, shape, dtype), D.make_boxes(seed, shape, 7)
            flags, angle, scale = D.LARGE_DRAW[name]
            grid, b = load(M, tmp, name, scene, boxes)
            script = [0.0 if flags & f else 0.999 for f in (D.ROT, D.FLIP0, D.FLIP1)] + [0.0, angle, scale]
            og, ob, dr = Run(M, script)(grid, b)
            assert dr == (flags, True, angle, scale, 6), dr
            want_g, want_b = D.prepare(scene, flags, True, angle, scale), D.boxes_augment(boxes, shape, flags, True, angle, scale)
            idx, _ = D.strided_sample(og)
            rec[name + "_input_sum"] = np.float64(scene.astype(np.float64).sum())
            rec[name + "_draw"] = np.array([flags, 1, angle, scale, 6], dtype=np.float64)
            rec[name + "_sum"] = np.float64(og.astype(np.float64).sum())
            rec[name + "_sample"] = og.reshape(-1)[idx]
            rec[name + "_boxes"] = ob
            rec[name + "_e_ref_grid"] = np.float64(np.abs(og - want_g).max())
            rec[name + "_e_ref_boxes"] = np.float64(np.abs(ob - want_b).max())
            print(name, dr, "e_ref grid %.3e boxes %.3e" % (rec[name + "_e_ref_grid"], rec[name + "_e_ref_boxes"]))
    assert all(np.isfinite(v).all() for v in rec.values())
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
