"""What the voxel-pipeline tests share (tests/test_voxel_input_ref_cpu.py, test_voxel_input_gpu.py, test_voxel_trainer_gpu.py) and what
tools/gen_golden_voxel_train.py records from: the class-weight cases, the small models, scenes and targets, and the child-process pattern of
tests/test_finetune_dist_gpu.py (spawn context, one answer per child, timeout, terminate on a dead child, no retry)."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402

GOLD_WEIGHTS = os.path.join(ROOT, "tests", "golden", "g28_class_weights.npz")
R = C.R
RO = 51          # int(32 * 1.6): the SR head's output resolution at R = 32 with out_resolution=256

# (name, classes, seed, shapes of the label volumes, absent class or None): 19 and 21 classes, one with an absent class, one with volumes of different sizes
CLASS_WEIGHT_CASES = [
    ("k19", 19, 2801, [(8, 8, 8), (8, 8, 8)], None),
    ("k21_absent", 21, 2802, [(6, 7, 5), (6, 7, 5), (6, 7, 5)], 5),
    ("k19_sizes", 19, 2803, [(5, 7, 3), (8, 8, 8), (1, 8, 2)], None),
]


def class_weight_labels(case):
    """the int64 label volumes of a case: uniform class ids 0 .. classes-1 from the case's seed, the absent class moved to 0 (unlabelled)"""
    _, K, seed, shapes, absent = case
    rng = np.random.default_rng(seed)
    vols = [rng.integers(0, K, shape, dtype=np.int64) for shape in shapes]
    if absent is not None:
        for v in vols:
            v[v == absent] = 0
    return vols


def print_err(*a):
    if os.environ.get("NMH_PRINT_ERR"):
        print(*a)


def no_stochastic_depth(model):
    for mod in model.modules():
        if hasattr(mod, "sd_prob"):
            mod.sd_prob = 0.0
    return model


def semantics_model(seed=0):
    return no_stochastic_depth(C.semantics_model(seed)).cuda().train()


def sr_model(seed=0):
    from nerf_mae_amd.heads import SwinTransformer_VoxelSR_Pretrained_Skip
    torch.manual_seed(seed)
    m = SwinTransformer_VoxelSR_Pretrained_Skip(resolution=R, out_resolution=256, is_eval=True, compute_dtype=torch.float32)
    return no_stochastic_depth(m).cuda().train()


def label_volume(seed):
    """(1,R,R,R) float32 labels of tests/_finetune_common.label_grid as a stored numpy volume"""
    return C.label_grid(seed).numpy()


def sr_target(seed):
    """a stored uint8 high-resolution scene (RO,RO,RO,4)"""
    from nerf_mae_amd import data
    return data.synthetic_scene((RO, RO, RO), 500 + seed, dtype=np.uint8)


def answers(q, procs, timeout):
    """one answer per child.  A child that died without answering (looked for every few seconds) or the timeout terminates all of them and fails the test"""
    import queue
    import time
    res, t0 = [], time.monotonic()
    while len(res) < len(procs):
        try:
            res.append(q.get(timeout=5))
            continue
        except queue.Empty:
            pass
        dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
        if dead or time.monotonic() - t0 > timeout:
            for p in procs:
                p.terminate()
            pytest.fail(f"{'a child died with exit code ' + str(dead[0]) if dead else 'no answer within ' + str(timeout) + ' s'} "
                        f"(answers so far: {[(r[0], r[1][-500:]) for r in res]})")
    return res


def spawn(target, args_of_rank, timeout=600):
    """two children, one q.get per child; a timeout or a dead child terminates both and fails (no retry)"""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(*args_of_rank(r), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = answers(q, procs, timeout)
    for p in procs:
        p.join(60)
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}: {r[1]}"
    return {r[0]: r[2] for r in res}


def init_gloo(rank, world, port):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
