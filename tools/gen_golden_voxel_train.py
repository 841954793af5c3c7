"""Records tests/golden/g28_class_weights.npz from the reference's own calculate_class_weights (nerf_rpn/model/metrics.py:383-426), run on the CPU.
    python tools/gen_golden_voxel_train.py --reference PATH_TO_REFERENCE_CHECKOUT

The function is imported with the stand-ins tools/gen_golden_sem_eval.py uses (np.float, an empty torchmetrics).  It takes a train loader; here that is a list
of `(None, [int64 label tensors], None)` batches of at most two volumes, the volumes being tests/_voxel_common.class_weight_labels(case).  Its prints are
swallowed.

Stored per case (key prefix = the case's name): `weights` (the reference's float64 result), `counts` (np.bincount of the non-zero labels over all volumes with
entry 0 zeroed, float64 integers: the `class_count` the reference divides), `classes`, `seed`, `shapes`, `absent` (-1: none) and `c`.  The volumes are NOT
stored: they follow from the seed and the shapes."""
import argparse
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import _voxel_common as V  # noqa: E402

C_DEFAULT = 1.02


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference project")
    ap.add_argument("--out", default=V.GOLD_WEIGHTS)
    args = ap.parse_args()
    from oracle.gen_golden import _install_shims
    _install_shims()
    tm = types.ModuleType("torchmetrics")
    tm.JaccardIndex = object
    sys.modules["torchmetrics"] = tm
    sys.path.insert(0, args.reference)
    sys.path.insert(0, os.path.join(args.reference, "nerf_rpn"))
    from nerf_rpn.model.metrics import calculate_class_weights
    rec = {}
    for case in V.CLASS_WEIGHT_CASES:
        name, K, seed, shapes, absent = case
        vols = V.class_weight_labels(case)
        loader = [(None, [torch.from_numpy(v) for v in vols[b:b + 2]], None) for b in range(0, len(vols), 2)]
        with contextlib.redirect_stdout(io.StringIO()):
            w = calculate_class_weights(loader, num_classes=K, c=C_DEFAULT)
        assert w.dtype == np.float64 and w.shape == (K,) and np.isfinite(w).all() and w[0] == 0
        counts = sum(np.bincount(v.reshape(-1), minlength=K) for v in vols).astype(np.float64)
        counts[0] = 0
        assert (absent is None) == bool((counts[1:] > 0).all())
        rec[f"{name}.weights"], rec[f"{name}.counts"] = w, counts
        rec[f"{name}.classes"], rec[f"{name}.seed"], rec[f"{name}.c"] = np.int64(K), np.int64(seed), np.float64(C_DEFAULT)
        rec[f"{name}.shapes"], rec[f"{name}.absent"] = np.array(shapes, dtype=np.int64), np.int64(-1 if absent is None else absent)
        print(name, "labelled", int(counts.sum()), "weights %.6f .. %.6f" % (w[1:].min(), w[1:].max()))
    np.savez_compressed(args.out, **rec)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, {len(rec)} arrays")


if __name__ == "__main__":
    main()
