"""FCOS head at the launcher's shape: N in {1, 2} scenes, 256 channels, the FPN's levels of a 160^3 grid (40^3, 20^3, 10^3, 5^3), num_convs 4, axis-aligned,
bf16 compute (run_fcos_pretrained.py:331-334).
    python tools/bench_fcos_head.py [reps]

Timed with HIP events, median and minimum of `reps` >= 20 calls after 3 warm-up calls, one process:
  head fwd        FCOSHead.forward_channels_last on channels-last bf16 features (weight packing included, as in every step)
  head fwd+bwd    the same, then the backward of sum(output * cotangent) to the features and every parameter
  gn stats / apply / bwd   the GroupNorm launches of one layer alone (all four levels, both towers)
  out fwd         the output kernel alone
Next to them the stock-torch composition of the same head (nn.Conv3d + nn.GroupNorm + nn.ReLU towers, three 3x3x3 nn.Conv3d, Scale and ReLU on NCDHW tensors)
in bf16, forward and forward+backward, measured in the same run, and ops.instnorm_apply on one tensor of the bytes of the GroupNorm apply pass."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from torch import nn

from nerf_mae_amd import ops
from nerf_mae_amd.fcos import FCOSHead

CIN, DIMS, CONVS, STRIDES = 256, (40, 20, 10, 5), 4, [4, 8, 16, 32]


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 for a, b in ev]
    return statistics.median(us), min(us)


class TorchHead(nn.Module):
    """the reference's FCOSHead, written from its semantics"""

    def __init__(self):
        super().__init__()
        tower = lambda: nn.Sequential(*[m for _ in range(CONVS) for m in (nn.Conv3d(CIN, CIN, 3, padding=1), nn.GroupNorm(32, CIN), nn.ReLU())])
        self.cls_tower, self.bbox_tower = tower(), tower()
        self.cls_logits, self.bbox_pred, self.centerness = nn.Conv3d(CIN, 1, 3, padding=1), nn.Conv3d(CIN, 6, 3, padding=1), nn.Conv3d(CIN, 1, 3, padding=1)
        self.scales = nn.Parameter(torch.ones(len(DIMS)))

    def forward(self, xs):
        out = ([], [], [])
        for l, x in enumerate(xs):
            a, b = self.cls_tower(x), self.bbox_tower(x)
            out[0].append(self.cls_logits(a))
            out[1].append(F.relu(self.bbox_pred(b) * self.scales[l]))
            out[2].append(self.centerness(b))
        return out


def main(reps=20):
    assert torch.cuda.is_available(), "bench_fcos_head.py needs an MI355X"
    reps = max(20, reps)
    torch.manual_seed(0)
    dt = torch.bfloat16
    for scenes in (1, 2):
        print(f"FCOS head: {scenes} scene(s), {CIN} channels, levels {DIMS}, num_convs {CONVS}; {reps} reps; median / min in us")
        head = FCOSHead(CIN, CONVS, STRIDES, compute_dtype=dt).cuda().train()
        feats = [torch.randn(scenes, d, d, d, CIN, device="cuda").to(dt).requires_grad_(True) for d in DIMS]
        outs = head.forward_channels_last(feats)
        cots = [[torch.randn_like(o) for o in os_] for os_ in outs]

        def fwd():
            with torch.no_grad():
                return head.forward_channels_last(feats)

        def fwd_bwd():
            o = head.forward_channels_last(feats)
            torch.autograd.backward([t for os_ in o for t in os_], [t for cs in cots for t in cs])

        print("  head fwd            %9.1f %9.1f" % timed(fwd, reps))
        print("  head fwd+bwd        %9.1f %9.1f" % timed(fwd_bwd, reps))
        xs = [f.detach() for f in feats for _ in (0, 1)]
        towers = [0, 1] * len(DIMS)
        gam, bet = [torch.ones(CIN, device="cuda")] * 2, [torch.zeros(CIN, device="cuda")] * 2
        stats = ops.fcos_gn_stats(xs, 32)
        ys = ops.fcos_gn_apply(xs, towers, stats, gam, bet, 32)
        dg, db = [torch.zeros(CIN, device="cuda") for _ in (0, 1)], [torch.zeros(CIN, device="cuda") for _ in (0, 1)]
        nbytes = sum(x.numel() for x in xs) * 2
        for name, fn, passes in (("gn stats", lambda: ops.fcos_gn_stats(xs, 32), 1), ("gn apply", lambda: ops.fcos_gn_apply(xs, towers, stats, gam, bet, 32), 2),
                                 ("gn bwd", lambda: ops.fcos_gn_bwd(ys, xs, ys, towers, stats, gam, dg, db, 32), 7)):
            med, mn = timed(fn, reps)
            print(f"  {name:18s}  {med:9.1f} {mn:9.1f}   {passes * nbytes / mn / 1e3:7.1f} GB/s over {passes} tensor passes of {nbytes / 1e6:.1f} MB")
        V = sum(d ** 3 for d in DIMS) * 2
        x1 = torch.randn(scenes, V, CIN, device="cuda").to(dt)
        st1 = torch.empty((scenes, CIN, 2), device="cuda")
        ops.instnorm_stats(x1, st1, torch.empty((scenes, CIN, 2), dtype=torch.float64, device="cuda"), scenes, V, CIN)
        o1 = torch.empty_like(x1)
        med, mn = timed(lambda: ops.instnorm_apply(x1, st1, o1, scenes, V, CIN), reps)
        print(f"  instnorm_apply      {med:9.1f} {mn:9.1f}   {2 * x1.numel() * 2 / mn / 1e3:7.1f} GB/s, one tensor of the same bytes")
        acts = [(ys[2 * l], ys[2 * l + 1]) for l in range(len(DIMS))]
        head._pack()
        pk = head._pk
        out_fwd = lambda: ops.fcos_head_out_fwd(acts, [pk["o0.w"], pk["o1.w"]], head.cls_logits.bias, head.bbox_pred.bias, head.centerness.bias,
                                                [s.scale for s in head.scales[:4]], STRIDES, 6, True, "train")
        print("  out fwd             %9.1f %9.1f" % timed(out_fwd, reps))
        ref = TorchHead().cuda().to(dt)
        rx = [f.detach().permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True) for f in feats]
        rcots = None

        def ref_fwd():
            with torch.no_grad():
                return ref(rx)

        def ref_fwd_bwd():
            o = ref(rx)
            torch.autograd.backward([t for os_ in o for t in os_], [torch.ones_like(t) for os_ in o for t in os_] if rcots is None else rcots)

        print("  torch bf16 fwd      %9.1f %9.1f" % timed(ref_fwd, reps))
        print("  torch bf16 fwd+bwd  %9.1f %9.1f" % timed(ref_fwd_bwd, reps))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
