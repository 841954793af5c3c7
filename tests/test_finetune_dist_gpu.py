"""Data-parallel fine-tuning on the GPU (dist.FlatGradReducer, FinetuneStep(reducer=), DetectionTrainer(rank, world)); the models, scenes and boxes of
tests/_finetune_common.py (swin_t, resolution 32, 64 FPN channels), at most two steps.  RCCL refuses two ranks on one device, so two ranks share the GPU over
gloo, as in tests/test_dist_gpu.py; the triggers and the comm stream run for real over a one-rank RCCL group (NMH_DP_FORCE=1).

  triggers        a recording stand-in snapshots a segment's slice of the gradient buffer at each launch: it must equal the final slice
  two ranks       FCOS built with world_size=2, one scene per rank with different positive counts, two FinetuneSteps: both ranks end bit-equal; the
                  exchanged gradient against (g0 + g1) / 2 element by element (the bound of tests/test_dist_gpu.py); (g0 + g1) / 2 against the gradient of ONE
                  process running both scenes as one batch with world_size=1 (the loss normalisers); the parameters after two steps against that process
  trainer         DetectionTrainer.fit() on two ranks
  forced          FinetuneStep with a one-rank reducer against the step without one

relerr over a set of tensors is the LARGEST per-tensor tests/_metrics.relerr (the normalisers, the forced reducer); the parameters of the two-rank run are held
to relerr over the whole buffer, the form its constants were stated in (see the test).  NMH_PRINT_ERR=1 prints every measured value."""
import functools
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _finetune_common as C  # noqa: E402
from tests._metrics import relerr  # noqa: E402

pytestmark = pytest.mark.gpu
LR, WD, CLIP, EPS = 1e-3, 1e-3, 0.1, 1.0     # eps = 1: the update stays linear in tiny gradients, so the order noise of fp32 atomics is not blown up to +-lr
SEEDS = (1, 2)                               # the scene of rank 0 and of rank 1


def _print(*a):
    if os.environ.get("NMH_PRINT_ERR"):
        print(*a)


def _no_stochastic_depth(model):
    for mod in model.modules():
        if hasattr(mod, "sd_prob"):
            mod.sd_prob = 0.0
    return model


def fcos_model(world_size=1, dtype=torch.float32, seed=0):
    from nerf_mae_amd.fcos import FCOSOverNeRF
    torch.manual_seed(seed)
    m = FCOSOverNeRF(C.fcos_args(dtype), C.backbone(dtype), list(C.STRIDES), resolution=C.R, world_size=world_size)
    return _no_stochastic_depth(m).cuda().train()


def rpn_model(dtype=torch.float32):
    from nerf_mae_amd.rpn import NeRFRegionProposalNetwork, RPNHead, _default_anchorgen
    torch.manual_seed(0)
    bb, gen = C.backbone(dtype), _default_anchorgen()
    head = RPNHead(bb.out_channels, gen.num_anchors_per_location()[0], 1, rotate=False, compute_dtype=dtype)
    net = NeRFRegionProposalNetwork(bb, rpn_anchor_generator=gen, rpn_head=head, rpn_fg_iou_thresh=0.35, rpn_bg_iou_thresh=0.2)
    net.check_targets = False
    return _no_stochastic_depth(net).cuda().train()


def boxes_of(seed):
    """rank 0's scene has two boxes, rank 1's one: the positive counts differ for certain (asserted from fcos_targets below)"""
    b = C.obb_boxes(seed)
    return b if seed == SEEDS[0] else b[:1]


def scenes_on_gpu():
    """the two scenes through DetectionBatcher without augmentation -> (meshes, targets), device tensors"""
    from nerf_mae_amd import data
    batcher = data.DetectionBatcher(C.R, torch.device("cuda"), normalize_density=True)
    xb, ext, targets = batcher.prepare([C.scene(s) for s in SEEDS], [boxes_of(s) for s in SEEDS], params=[(0, 0.0, 1.0)] * 2)
    assert ext == [[C.R] * 3] * 2
    torch.cuda.synchronize()
    return [xb[i].clone() for i in range(2)], [t.clone() for t in targets]


def per_tensor(layout, a, b):
    """largest per-tensor relerr of two flat buffers under a name -> [offset, numel] layout"""
    return max(relerr(a[o:o + k], b[o:o + k]) for o, k in layout.values())


# ---- the triggers ----------------------------------------------------------------------------------------------------------------------------------
def _record_triggers(model, batch):
    """one forward + backward with a recording stand-in for the reducer -> (the real reducer whose bounds it uses, {segment: [snapshots]}, the flat parameters)"""
    from nerf_mae_amd.dist import FlatGradReducer, _Trigger
    from nerf_mae_amd.finetune import FlatParameters, loss_fn_for
    flat = FlatParameters(model, torch.device("cuda"))
    real = FlatGradReducer(flat)          # world 1: only its segment table is used

    class Recorder:
        bounds, nseg, snaps = real.bounds, real.nseg, {}
        chunk_stage, chunk_groups, seg_stage, seg_tail = real.chunk_stage, real.chunk_groups, real.seg_stage, real.seg_tail

        def trigger(self, x, seg):
            return _Trigger.apply(x, self, seg)

        def launch(self, seg):
            torch.cuda.synchronize()
            self.snaps.setdefault(seg, []).append(flat._flat_grad[self.bounds[seg]:self.bounds[seg + 1]].clone())

    rec = Recorder()
    flat.base._reducer = rec
    flat.zero_grad()
    losses = loss_fn_for(model)(*batch)
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    return real, rec.snaps, flat


def _check_snapshots(real, snaps, flat, expected):
    assert sorted(snaps) == sorted(expected), (sorted(snaps), sorted(expected))
    for seg, shots in snaps.items():
        assert len(shots) == 1, f"segment {seg} launched {len(shots)} times in one step"
        final = flat._flat_grad[real.bounds[seg]:real.bounds[seg + 1]]
        assert final.any(), f"segment {seg} has no gradient at all"
        assert torch.equal(shots[0], final), (seg, (shots[0] - final).abs().max().item())


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["fcos", "rpn"])
def test_detector_triggers_fire_once_after_every_gradient_of_their_segment(which, dtype):
    """every segment but the embed one (finish() launches it) fires exactly once, the tail -- neck, heads, Scales -- included, and holds its final gradient"""
    meshes, targets = scenes_on_gpu()
    if which == "fcos":
        model = fcos_model(dtype=dtype)
    else:
        model, targets = rpn_model(dtype), [torch.from_numpy(C.aabb_boxes(s)).cuda() for s in SEEDS]
    real, snaps, flat = _record_triggers(model, (meshes, targets))
    assert real.seg_tail() == real.nseg - 1 == 7
    _check_snapshots(real, snaps, flat, range(1, real.nseg))


def test_voxel_head_stage_triggers_fire_and_the_tail_is_left_to_finish():
    """the voxel heads' base decoders defer weight gradients into the queue, so their tail gets no trigger: the stage segments fire, the embed range and the
    tail are finish()'s"""
    meshes, _ = scenes_on_gpu()
    model = _no_stochastic_depth(C.semantics_model()).cuda().train()
    real, snaps, flat = _record_triggers(model, (meshes, [C.label_grid(s).cuda() for s in SEEDS]))
    _check_snapshots(real, snaps, flat, range(1, real.nseg - 1))
    tail = flat._flat_grad[real.bounds[real.seg_tail()]:]
    assert tail.any()


# ---- two ranks on one GPU over gloo ----------------------------------------------------------------------------------------------------------------
def _answers(q, procs, timeout):
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


def _spawn(target, args_of_rank, timeout=600):
    """two children, one q.get per child; a timeout or a dead child terminates both and fails (no retry)"""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=target, args=(*args_of_rank(r), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = _answers(q, procs, timeout)
    for p in procs:
        p.join(60)
    for r in res:
        assert r[1] == "ok", f"rank {r[0]}: {r[1]}"
    return {r[0]: r[2] for r in res}


def _init(rank, world, port):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _step_worker(rank, world, port, comm, out_dir, q):
    _init(rank, world, port)
    try:
        from nerf_mae_amd.dist import FlatGradReducer, broadcast_flat_parameters
        from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for
        from nerf_mae_amd.trainer import FusedAdamW
        m = fcos_model(world_size=world, seed=rank)          # another initialisation on rank 1: the broadcast must equalise it
        flat = FlatParameters(m, torch.device("cuda"))
        broadcast_flat_parameters(flat)
        red = FlatGradReducer(flat, comm_dtype=torch.bfloat16 if comm == "bf16" else None)
        assert red.active and red.world == 2
        opt = FusedAdamW(flat, lr=LR, weight_decay=WD, max_grad_norm=CLIP, eps=EPS)
        step = FinetuneStep(flat, opt, loss_fn_for(m), reducer=red)
        assert flat.base._reducer is red
        meshes, targets = scenes_on_gpu()
        grabbed = {}
        finish = red.finish

        def recording_finish():
            if not grabbed:                                   # the first step: same parameters in every run
                grabbed["own"] = flat._flat_grad.detach().clone()
                finish()
                grabbed["exchanged"] = flat._flat_grad.detach().clone()
            else:
                finish()

        red.finish = recording_finish
        for _ in range(2):
            step([meshes[rank]], [targets[rank]])
        torch.cuda.synchronize()
        final = flat._flat.detach().cpu()
        both = [torch.empty_like(final) for _ in range(world)]
        dist.all_gather(both, final)
        assert torch.equal(both[0], both[1]), (both[0] - both[1]).abs().max()          # check 1
        own = grabbed["own"].cpu()
        owns = [torch.empty_like(own) for _ in range(world)]
        dist.all_gather(owns, own)
        ans = None
        if rank == 0:
            g0, g1, got = owns[0], owns[1], grabbed["exchanged"].cpu()
            exact = (g0 + g1) / 2
            bound = (8e-3 if comm == "bf16" else 1e-5) * (g0.abs() + g1.abs()) / 2 + 1e-12 + 1e-5 * exact.abs().max()          # check 2
            ans = {"exchange_worst": ((got - exact).abs() / bound).max().item(), "g0_max": g0.abs().max().item(), "g1_max": g1.abs().max().item()}
            torch.save({"exact": exact, "final": final}, os.path.join(out_dir, "rank0.pt"))         # by file: 240 MB would crawl through the queue
        q.put((rank, "ok", ans))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


@functools.lru_cache(maxsize=None)
def single_process_runs():
    """S, S': ONE process, both scenes as one batch, world_size=1, two FinetuneSteps without a reducer -> the gradient of the first step and the parameters
    after the second, twice (the path's own run-to-run spread).  Computed once, shared by the bucket dtypes, left unchanged."""
    from nerf_mae_amd.fcos_loss import fcos_targets
    from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for
    from nerf_mae_amd.trainer import FusedAdamW, flat_layout
    meshes, targets = scenes_on_gpu()
    sizes = [(C.R // s,) * 3 for s in C.STRIDES]
    a = C.fcos_args()
    counts = [fcos_targets(sizes, C.STRIDES, [t], a.center_sampling_radius, a.norm_reg_targets, return_scalars=True)[5][0].item() for t in targets]
    runs = []
    for _ in range(2):
        m = fcos_model(world_size=1)
        flat = FlatParameters(m, torch.device("cuda"))
        opt = FusedAdamW(flat, lr=LR, weight_decay=WD, max_grad_norm=CLIP, eps=EPS)
        step = FinetuneStep(flat, opt, loss_fn_for(m))
        _, total = step.forward(meshes, targets)
        total.backward()
        grad = flat._flat_grad.detach().cpu().clone()
        opt.step()
        step(meshes, targets)
        torch.cuda.synchronize()
        runs.append((grad, flat._flat.detach().cpu().clone()))
        layout = flat_layout(flat)
    (gs, ps), (gs2, ps2) = runs
    return dict(counts=counts, layout=layout, grad=gs, params=ps, spread_g=per_tensor(layout, gs2, gs), spread_p=relerr(ps2, ps),
                spread_p_per_tensor=per_tensor(layout, ps2, ps))


@pytest.mark.parametrize("comm", ["fp32", "bf16"])
def test_two_ranks_one_gpu_match_one_process_on_both_scenes(comm, tmp_path):
    """checks 1 to 4 of the module docstring.  Bounds: the exchanged gradient element by element |g_DP - (g0 + g1) / 2| <= c (|g0| + |g1|) / 2 + 1e-12 +
    1e-5 max|exact|, c = 1e-5 (fp32 buckets) or 8e-3 (bf16: one rounding per operand and one of the sum, 2^-8 each); the normalisers per tensor
    relerr((g0 + g1) / 2, g_S) <= 1e-5 + 4 relerr(g_S, g_S'), equal in real arithmetic since mean_r grad(S_r / (N / 2)) = grad(S_0 + S_1) / N; the parameters
    after two steps relerr <= 1e-5 (fp32 buckets) or 5e-5 (bf16) + 4 relerr(S, S'), relerr here over the WHOLE flat buffer: that is the quantity the two
    constants were stated for (tests/test_dist_gpu.py:112).  Per tensor 5e-5 cannot hold with bf16 buckets by the number format alone: a zero-initialised bias
    consists of nothing but two accumulated updates, each linear in the gradient (eps = 1), so it carries the buckets' relative rounding of up to 2^-8 = 3.9e-3
    in full (measured 4.6e-3 on such a tensor, 2.0e-6 with fp32 buckets); the per-tensor figure is printed, and asserted with fp32 buckets only."""
    S = single_process_runs()
    assert S["counts"][0] != S["counts"][1] and min(S["counts"]) > 0, f"positive counts {S['counts']}: with equal counts a missing normaliser exchange is invisible"
    port = 24600 + (os.getpid() % 2000) + (1 if comm == "bf16" else 0)          # apart from tests/test_dist_gpu.py (29600 .., 29700 ..)
    ans = _spawn(_step_worker, lambda r: (r, 2, port, comm, str(tmp_path)))[0]
    ck = torch.load(str(tmp_path / "rank0.pt"), weights_only=True)
    err_g, err_p = per_tensor(S["layout"], ck["exact"], S["grad"]), relerr(ck["final"], S["params"])
    bound_g, bound_p = 1e-5 + 4 * S["spread_g"], (1e-5 if comm == "fp32" else 5e-5) + 4 * S["spread_p"]
    _print(f"  [two ranks, {comm} buckets] positives {S['counts']}  exchanged gradient {ans['exchange_worst']:.3f} x its bound  max|g0| {ans['g0_max']:.3g} max|g1| {ans['g1_max']:.3g}")
    _print(f"  [two ranks, {comm} buckets] normalisers relerr((g0+g1)/2, g_S) {err_g:.2e}  relerr(g_S, g_S') {S['spread_g']:.2e}  bound {bound_g:.2e}")
    _print(f"  [two ranks, {comm} buckets] parameters after two steps relerr {err_p:.2e}  relerr(S, S') {S['spread_p']:.2e}  bound {bound_p:.2e}  "
           f"(per tensor {per_tensor(S['layout'], ck['final'], S['params']):.2e}, S against S' {S['spread_p_per_tensor']:.2e})")
    assert ans["exchange_worst"] <= 1.0, f"exchanged gradient off by {ans['exchange_worst']:.2f}x the stated bound"
    assert err_g <= bound_g, (err_g, bound_g)
    assert err_p <= bound_p, (err_p, bound_p)
    if comm == "fp32":          # no rounding of the buckets: the same constant holds tensor by tensor as well
        err_pt = per_tensor(S["layout"], ck["final"], S["params"])
        assert err_pt <= 1e-5 + 4 * S["spread_p_per_tensor"], (err_pt, S["spread_p_per_tensor"])


# ---- DetectionTrainer on two ranks -----------------------------------------------------------------------------------------------------------------
def _trainer_worker(rank, world, port, out_dir, q):
    _init(rank, world, port)
    try:
        from nerf_mae_amd.trainer import DetectionTrainer
        m = fcos_model(world_size=world, seed=rank)
        with torch.no_grad():
            m.fcos_module.head.cls_logits.bias.fill_(-1.0)          # the untrained head's scores pass pre_nms_thresh (tests/test_finetune_gpu.py)
        save = os.path.join(out_dir, f"rank{rank}")
        lines = []
        tr = DetectionTrainer(m, [C.scene(s) for s in (11, 12, 13, 14)], [C.obb_boxes(s) for s in (11, 12, 13, 14)], [C.scene(s) for s in (15, 16)],
                              [C.obb_boxes(s) for s in (15, 16)], batch_size=1, num_epochs=2, lr=1e-4, weight_decay=1e-3, eval_interval=1, save_path=save,
                              flip_prob=0.5, rotate_prob=0.5, rot_scale_prob=0.5, log=lines.append, rank=rank, world=world)
        assert tr.steps_per_epoch == 2 and tr.args["batch_size"] == 2 and tr.reducer is not None and tr.reducer.active
        hist = tr.fit()
        torch.cuda.synchronize()
        assert tr.global_step == 4 and len(lines) == (2 if rank == 0 else 0)
        final = tr.flat._flat.detach().cpu()
        both = [torch.empty_like(final) for _ in range(world)]
        dist.all_gather(both, final)
        assert torch.equal(both[0], both[1]), (both[0] - both[1]).abs().max()
        tr.flat.check()
        q.put((rank, "ok", hist))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_detection_trainer_fit_on_two_ranks(tmp_path):
    """four scenes, per-rank batch 1, two epochs, validation on two scenes: both ranks end with bit-equal parameters (asserted in the children), only rank 0
    evaluates and writes, both report the same training losses, and nobody hangs"""
    port = 26700 + (os.getpid() % 2000)
    hist = _spawn(_trainer_worker, lambda r: (r, 2, port, str(tmp_path)))
    train_keys = ["epoch", "train_loss", "loss_cls", "loss_reg", "loss_centerness"]
    assert [list(h) for h in hist[1]] == [train_keys] * 2
    for h0, h1 in zip(hist[0], hist[1]):
        for k in ("ap_25", "ap_50", "recall_25_top_15", "recall_50_top_15", "recall_ar_top_15"):
            assert k in h0 and h0[k] == h0[k], (k, h0)
        assert all(h0[k] == h1[k] for k in train_keys), (h0, h1)
        assert h0["loss_reg"] > 0 and h0["train_loss"] == h0["train_loss"]
    files = os.listdir(tmp_path / "rank0")
    assert files and all(f.endswith(".pt") for f in files)
    assert not os.path.exists(tmp_path / "rank1") or not os.listdir(tmp_path / "rank1")


def test_detection_trainer_refuses_a_loss_built_for_another_world():
    from nerf_mae_amd.trainer import DetectionTrainer
    m = fcos_model(world_size=1)
    with pytest.raises(ValueError, match="world_size"):
        DetectionTrainer(m, [C.scene(11)], [C.obb_boxes(11)], batch_size=1, rank=0, world=2)


# ---- the forced one-rank reducer -------------------------------------------------------------------------------------------------------------------
def _forced_worker(port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NMH_DP_FORCE="1")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        from nerf_mae_amd.dist import FlatGradReducer
        from nerf_mae_amd.finetune import FinetuneStep, FlatParameters, loss_fn_for
        from nerf_mae_amd.trainer import FusedAdamW, flat_layout
        meshes, targets = scenes_on_gpu()
        finals, launched = [], None
        for forced in (False, False, True):          # B, B', then the step with the reducer
            m = fcos_model()
            flat = FlatParameters(m, dev)
            red = FlatGradReducer(flat) if forced else None
            opt = FusedAdamW(flat, lr=LR, weight_decay=WD, max_grad_norm=CLIP, eps=EPS)
            step = FinetuneStep(flat, opt, loss_fn_for(m), reducer=red)
            if forced:
                assert red.active and red.world == 1 and red.comm_stream is not None and flat.base._reducer is red
                launched, launch = [], red.launch
                red.launch = lambda seg: (launched.append(seg), launch(seg))[1]
            for _ in range(2):
                step(meshes, targets)
            torch.cuda.synchronize()
            finals.append(flat._flat.detach().cpu().clone())
            layout = flat_layout(flat)
        nseg = red.nseg
        assert launched == (list(range(nseg - 1, 0, -1)) + [0]) * 2, launched          # the triggers in backward order, the embed range from finish(), every step
        q.put((0, "ok", {"err": per_tensor(layout, finals[2], finals[0]), "spread": per_tensor(layout, finals[1], finals[0])}))
    except Exception:  # noqa: BLE001
        import traceback
        q.put((0, traceback.format_exc(), None))
    finally:
        dist.destroy_process_group()


def test_forced_one_rank_reducer_leaves_the_step_as_it_is():
    """NMH_DP_FORCE=1 over a one-rank RCCL group, fp32 buckets: triggers, comm stream and joins are real, the exchange is an identity.  The parameters after
    two steps stay within 4 relerr(B, B') of the step without a reducer, B' being a second run of that step (its own spread)."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_forced_worker, args=(27200 + (os.getpid() % 2000), q))
    p.start()
    _, msg, ans = _answers(q, [p], 600)[0]
    p.join(60)
    assert msg == "ok", msg
    _print(f"  [forced one-rank reducer] parameters relerr(forced, B) {ans['err']:.2e}  relerr(B, B') {ans['spread']:.2e}  bound {4 * ans['spread']:.2e}")
    assert ans["err"] <= 4 * ans["spread"], (ans["err"], ans["spread"])
