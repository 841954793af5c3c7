"""float64 restatement of the voxel-semantics evaluation (nerf_mae_amd/sem_eval.py, csrc/heads.hip sem_eval_kernel), written from the definitions in the reference
(output_metrics, feature_extractor.py:2748-2806; intersectionAndUnionGPU, metrics.py:491-518; the evaluation loop, run_voxel_semantics.py:805-958) in plain
torch / numpy and never from the kernel's loops.  tests/test_sem_eval_ref_cpu.py pins it to tests/golden/g26_sem_eval.npz, recorded from the reference's own
output_metrics by tools/gen_golden_sem_eval.py; tests/test_sem_eval_gpu.py compares the kernels with it.

Inputs come from seeds.  After the logits are drawn, the winner of every voxel whose top-two gap is below MARGIN is raised by RAISE, so that every random case
has an asserted arg-max margin (`argmax_margin`) and no voxel is left out of any comparison; the crafted exact ties are the only voxels below the margin, and
there the rule under test (the lowest index wins) is what the restatement applies."""
import numpy as np
import torch

from tests import _heads_ref as HR

F64 = torch.float64
MARGIN, RAISE = 1e-3, 1e-2

# (name, K, class weights?, spatial shape, B, logit sigma, kind).  kind: 'mixed' ~40 % unlabelled; 'blank1' sample 1 has no labelled voxel; 'absent3' class 3 is in
# no label and never predicted; 'pred0' class 0 wins on about a third of the voxels; 'ties' exact ties between two or three classes (class 0 among them) on
# every 5th voxel; 'badlabels' labels equal to K and to 255 on some voxels
CASES = [
    ("K5-cw-s2-7x5x3-B2", 5, True, (7, 5, 3), 2, 2.0, "mixed"),                # less than one workgroup; V odd: the second sample's planes are misaligned
    ("K19-cw-s4-30x32x27-B2", 19, True, (30, 32, 27), 2, 4.0, "mixed"),
    ("K19-nocw-s1-32-B1", 19, False, (32, 32, 32), 1, 1.0, "mixed"),
    ("K2-nocw-s1-9-B3", 2, False, (9, 9, 9), 3, 1.0, "mixed"),
    ("K32-cw-s4-12-B2", 32, True, (12, 12, 12), 2, 4.0, "mixed"),
    ("K19-cw-s1-8-B3-blank1", 19, True, (8, 8, 8), 3, 1.0, "blank1"),
    ("K5-cw-s4-8-B2-absent3", 5, True, (8, 8, 8), 2, 4.0, "absent3"),
    ("K19-cw-s1-10-B2-pred0", 19, True, (10, 10, 10), 2, 1.0, "pred0"),
    ("K8-nocw-s1-11x6x5-B2-ties", 8, False, (11, 6, 5), 2, 1.0, "ties"),
    ("K19-cw-s1-12-B2-ties", 19, True, (12, 12, 12), 2, 1.0, "ties"),
]
BAD_LABEL_CASES = [("K19-cw-s1-12-B2-badlabels", 19, True, (12, 12, 12), 2, 1.0, "badlabels"), ("K5-nocw-s1-7x5x3-B2-badlabels", 5, False, (7, 5, 3), 2, 1.0, "badlabels")]
# one grid-stride trip covers (1024 / B) workgroups x 256 lanes x 4 voxels with 16-byte loads (V % 4 == 0) and x 1 voxel on the scalar path: with B = 1 these two
# are the smallest cubes past 1 048 576 resp. 262 144 voxels (104^3 = 1 124 864, divisible by 4; 65^3 = 274 625, odd), so some lanes take a second trip
SECOND_TRIP_CASES = [("K5-nocw-s1-104-B1", 5, False, (104, 104, 104), 1, 1.0, "mixed"), ("K19-cw-s4-65-B1", 19, True, (65, 65, 65), 1, 4.0, "mixed")]
# the masked-CE cases of tests/_heads_ref.py that carry the shapes 32^3 / K = 19
HEADS_CASES = [c for c in HR.ce_cases() if c[0] in ("K19-cw-s4-V32-B3", "K19-cw-s1-V32-B3-blank1")]
# recorded from the reference (cubes: its transform pads to a cube); the three K = 19 cases of EVAL_SEQUENCE, in this order, are one evaluation loop
GOLDEN_CASES = [
    ("g-K19-cw-s2-8-B1", 19, True, (8, 8, 8), 1, 2.0, "mixed"),
    ("g-K19-cw-s2-10-B2", 19, True, (10, 10, 10), 2, 2.0, "pred0"),
    ("g-K19-cw-s2-12-B3", 19, True, (12, 12, 12), 3, 2.0, "blank1"),
    ("g-K5-nocw-s4-9-B2", 5, False, (9, 9, 9), 2, 4.0, "absent3"),
    ("g-K2-nocw-s1-7-B2", 2, False, (7, 7, 7), 2, 1.0, "mixed"),
    ("g-K32-cw-s1-6-B1", 32, True, (6, 6, 6), 1, 1.0, "mixed"),
]
EVAL_SEQUENCE = [c[0] for c in GOLDEN_CASES[:3]]


def raise_winners(logits):
    """(B,K,*) fp32: wherever the top-two gap is below MARGIN the winner is raised by RAISE (in place); returns the tensor"""
    top = logits.topk(2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < MARGIN
    win = top.indices[:, 0]
    bump = torch.zeros_like(logits).scatter_(1, win.unsqueeze(1), (close.float() * RAISE).unsqueeze(1))
    logits += bump
    return logits


def inputs(case):
    """(logits fp32 (B,K,*shape), labels fp32 (B,*shape), cw fp32 [K] or None, tie mask bool (B,*shape)) of a case, on the CPU"""
    name, K, has_cw, shape, B, sig, kind = case
    if case in HEADS_CASES:
        logits, labels, cw = HR.ce_inputs(case)
        return raise_winners(logits), labels, cw, torch.zeros(labels.shape, dtype=torch.bool)
    g = torch.Generator().manual_seed(sum(map(ord, name)) + 7919)
    logits = torch.randn((B, K) + tuple(shape), generator=g) * sig
    labels = torch.randint(1, K, (B,) + tuple(shape), generator=g).float()
    labels[torch.rand(labels.shape, generator=g) < 0.4] = 0.0
    ties = torch.zeros(labels.shape, dtype=torch.bool)
    hit = (torch.rand(labels.shape, generator=g) < 0.5) & (labels > 0)          # about half of the labelled voxels lean towards their own class
    logits.scatter_add_(1, labels.long().unsqueeze(1), (hit.float() * 2.5 * sig).unsqueeze(1))
    if kind == "blank1":
        labels[1] = 0.0
    if kind == "absent3":
        labels[labels == 3] = 1.0
        logits[:, 3] -= 40.0
    if kind == "pred0":
        up = torch.rand(labels.shape, generator=g) < 0.33
        logits[:, 0] += up.float() * 3.0 * sig
    if kind == "badlabels":
        r = torch.rand(labels.shape, generator=g)
        labels[r < 0.05] = float(K)
        labels[(r >= 0.05) & (r < 0.1)] = 255.0
    raise_winners(logits)
    if kind == "ties":   # every 5th voxel: classes a < b (every third of them a = 0, every fourth also a third class c > b) share the largest value exactly
        flat = logits.view(B, K, -1)
        V = flat.shape[2]
        for b in range(B):
            for i, v in enumerate(range(b, V, 5)):
                a = 0 if i % 3 == 0 else 1 + (i % (K - 1)) % max(K - 2, 1)
                a = min(a, K - 2)
                bb = a + 1 + (i % (K - 1 - a))
                top = float(flat[b, :, v].max()) + 0.5
                flat[b, a, v] = top
                flat[b, bb, v] = top
                if i % 4 == 0 and bb + 1 < K:
                    flat[b, K - 1, v] = top
                ties.view(B, -1)[b, v] = True
    return logits, labels, cw_of(K, g) if has_cw else None, ties


def cw_of(K, g):
    return torch.cat([torch.tensor([0.05]), 0.5 + torch.rand(K - 1, generator=g)])


def predicted(logits):
    """arg-max over the class axis, the lowest index among exact ties, int64 (B,*)"""
    K = logits.shape[1]
    mx = logits.max(dim=1, keepdim=True).values
    idx = torch.arange(K).view((1, K) + (1,) * (logits.dim() - 2)).expand_as(logits)
    return torch.where(logits == mx, idx, torch.full_like(idx, K)).min(dim=1).values


def argmax_margin(logits, ties=None):
    """the smallest top-two gap over the voxels outside `ties`"""
    top = logits.double().topk(2, dim=1).values
    gap = top[:, 0] - top[:, 1]
    if ties is not None:
        gap = gap[~ties]
    return float(gap.min())


def counts(pred, target, K):
    """int64 label tensors of one shape -> numpy int64 [4][K-1] = {intersection, union, target, area_pred} over the elements with target > 0; a target >= K is a
    labelled voxel of no class"""
    p, t = pred.reshape(-1).numpy().astype(np.int64), target.reshape(-1).numpy().astype(np.int64)
    lab = t > 0
    p, t = p[lab], t[lab]

    def hist(x):
        x = x[(x >= 1) & (x < K)]
        return np.bincount(x, minlength=K)[1:K].astype(np.int64)
    inter, area_pred, area_target = hist(p[p == t]), hist(p), hist(t)
    return np.stack([inter, area_pred + area_target - inter, area_target, area_pred])


def sem_eval(logits, labels, cw, scalars=True):
    """-> dict: ce, miou (float64; None with scalars=False, for labels outside [0, K) where the loss is undefined), counts int64 [4][K-1], pred_vis, target_vis
    int64 (B,*)"""
    K = logits.shape[1]
    t = labels.long()
    lab = t > 0
    p = predicted(logits)
    out = dict(counts=counts(p, t, K), pred_vis=p * lab, target_vis=t * lab, ce=None, miou=None)
    if scalars:
        r = HR.masked_ce(logits, labels, cw)
        out["ce"], out["miou"] = float(r["ce"]), float(r["miou"])
    return out


def evaluator_numbers(I, U, T):
    """the evaluation loop's five results from summed counts, in float64 (run_voxel_semantics.py:927-933)"""
    I, U, T = (np.asarray(a, dtype=np.float64) for a in (I, U, T))
    iou_class, accuracy_class = I / (U + 1e-10), I / (T + 1e-10)
    return dict(iou_class=iou_class, accuracy_class=accuracy_class, mIoU=float(np.mean(iou_class)), mAcc=float(np.mean(accuracy_class)),
                allAcc=float(I.sum() / (T.sum() + 1e-10)))


def batch_accuracy(I, T):
    """the loop's per-batch accuracy (run_voxel_semantics.py:905)"""
    return float(np.asarray(I, np.float64).sum() / (np.asarray(T, np.float64).sum() + 1e-10))


def checksum(vol):
    """two int64 sums of a label volume: plain, and weighted by (flat index mod 65521) + 1 (order-sensitive)"""
    f = vol.reshape(-1).numpy().astype(np.int64)
    w = (np.arange(f.size, dtype=np.int64) % 65521) + 1
    return np.array([f.sum(), (f * w).sum()], dtype=np.int64)
