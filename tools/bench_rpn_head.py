"""RPN head at the launcher's shape: 2 scenes, 256 channels, the FPN's levels of a 160^3 grid (40^3, 20^3, 10^3, 5^3), conv_depth 4, A = 5 anchors per
location (run_rpn.py:108,177), axis-aligned (6 columns) and oriented (8 columns), bf16 compute.
    python tools/bench_rpn_head.py [reps]

Timed with HIP events, median and minimum of `reps` >= 20 calls after 3 warm-up calls, one process:
  head fwd        RPNHead.forward_channels_last on channels-last bf16 features (weight packing included, as in every step)
  head fwd+bwd    the same, then the backward of sum(output * cotangent) to the features and every parameter
  out fwd / bwd   the output kernels alone (ops.rpn_head_out_fwd, ops.rpn_head_out_bwd: dt + weight and bias gradients)
  gemm + transpose  what the output kernel replaces: ops.gemm_nt per level (bf16 rows [voxels, A (1 + C)], no ReLU) and ops.ndhwc_to_ncdhw of the result
Next to them the stock-torch composition of the same head (nn.Conv3d + ReLU + two 1x1x1 nn.Conv3d on NCDHW tensors), in fp32 and in bf16, forward and
forward+backward, measured in the same run.  The composition's fp32 outputs are compared with the head's."""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch import nn

from nerf_mae_amd import ops
from nerf_mae_amd.rpn import RPNHead

SCENES, CIN, DIMS, DEPTH, A = 2, 256, (40, 20, 10, 5), 4, 5


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
    """the reference's RPNHead, written from its semantics (Conv3d + ReLU pairs, two 1x1x1 convs)"""

    def __init__(self, C):
        super().__init__()
        self.conv = nn.Sequential(*[m for _ in range(DEPTH) for m in (nn.Conv3d(CIN, CIN, 3, padding=1), nn.ReLU(inplace=True))])
        self.cls_logits, self.bbox_pred = nn.Conv3d(CIN, A, 1), nn.Conv3d(CIN, A * C, 1)

    def forward(self, xs):
        ts = [self.conv(x) for x in xs]
        return [self.cls_logits(t) for t in ts], [self.bbox_pred(t) for t in ts]


def main(reps=20):
    assert torch.cuda.is_available(), "bench_rpn_head.py needs an MI355X"
    reps = max(20, reps)
    torch.manual_seed(0)
    print(f"RPN head: {SCENES} scenes, {CIN} channels, levels {DIMS}, conv_depth {DEPTH}, A = {A}; {reps} reps")
    for rotate in (False, True):
        C = 8 if rotate else 6
        name = "oriented" if rotate else "axis-aligned"
        head = RPNHead(CIN, A, DEPTH, rotate).cuda()
        with torch.no_grad():
            for p in head.conv.parameters():
                if p.dim() > 1:
                    p.normal_(0, (2.0 / (CIN * 27)) ** 0.5)
        ref = TorchHead(C).cuda()
        ref.load_state_dict(head.state_dict())
        x32 = [torch.randn((SCENES, CIN, d, d, d), device="cuda") for d in DIMS]
        xcl = [ops.ncdhw_to_ndhwc(x, torch.bfloat16).requires_grad_(True) for x in x32]
        obj, reg = head.forward_channels_last(xcl)
        cot = [torch.randn_like(t) for t in obj + reg]

        def fwd_bwd():
            o, r = head.forward_channels_last(xcl)
            torch.autograd.grad(o + r, xcl, cot)
        with torch.no_grad():
            t = {"head fwd": timed(lambda: head.forward_channels_last(xcl), reps)}
        t["head fwd+bwd"] = timed(fwd_bwd, reps)
        # the output stage alone, on the last conv's activations
        ts = [torch.randn((SCENES, d, d, d, CIN), device="cuda").bfloat16() for d in DIMS]
        head._pack()
        wc, wb = head._pk["cls.w"], head._pk["box.w"]
        grads = [torch.zeros_like(p) for p in (head.cls_logits.weight, head.bbox_pred.weight, head.cls_logits.bias, head.bbox_pred.bias)]
        go, gr = [c for c in cot[:len(DIMS)]], [c for c in cot[len(DIMS):]]
        t["out fwd"] = timed(lambda: ops.rpn_head_out_fwd(ts, wc, wb, head.cls_logits.bias, head.bbox_pred.bias, C, True), reps)
        t["out bwd"] = timed(lambda: ops.rpn_head_out_bwd(ts, wc, wb, go, gr, C, True, *grads), reps)
        wcat = torch.cat([wc.view(A, CIN), wb.view(A * C, CIN), torch.zeros(((-A * (1 + C)) % 8, CIN), device="cuda", dtype=torch.bfloat16)])
        bcat = torch.cat([head.cls_logits.bias, head.bbox_pred.bias, torch.zeros((-A * (1 + C)) % 8, device="cuda")]).detach()

        def gemm_transpose():
            for x in ts:
                y = ops.gemm_nt(x.view(-1, CIN), wcat, bias=bcat)
                ops.ndhwc_to_ncdhw(y.view(*x.shape[:4], -1))
        t["gemm + transpose"] = timed(gemm_transpose, reps)
        print(f"  {name} kernels:     " + " | ".join(f"{k} median {m:9.1f} us  min {b:9.1f} us" for k, (m, b) in t.items()))
        for dtype in (torch.float32, torch.bfloat16):
            m = ref.to(dtype)
            xs = [x.to(dtype).requires_grad_(True) for x in x32]
            cd = [c.to(dtype) for c in cot]

            def ref_fwd_bwd():
                o, r = m(xs)
                torch.autograd.grad(o + r, xs + list(m.parameters()), cd)
            with torch.no_grad():
                c = {"head fwd": timed(lambda: m(xs), reps)}
                if dtype == torch.float32:
                    o, r = m(xs)
                    err = max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(obj + reg, o + r))
            c["head fwd+bwd"] = timed(ref_fwd_bwd, reps)
            print(f"  {name} torch {str(dtype)[6:]:8s}: " + " | ".join(f"{k} median {a:9.1f} us  min {b:9.1f} us" for k, (a, b) in c.items()))
        print(f"  {name}: the bf16 head's outputs differ from the fp32 composition's by {err:.2e} of the largest")


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else 20)
