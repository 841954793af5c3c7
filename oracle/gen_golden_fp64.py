"""Float64 twins of goldens G7 (formula-filled swin_t), G8 (tiny model), G9, G13 and G14 (training traces), from the REAL reference
(read-only, /root/reference) in the build container.  TEST INFRASTRUCTURE ONLY.   Run: python oracle/gen_golden_fp64.py  (needs /root/reference)

The fp32 originals pin the oracle to within 2e-5 of the reference's fp32 rounding on the host that generated them; on another CPU (other
MKL / oneDNN kernels, another vector width or thread count) fp32 rounding differs, and through the ill-conditioned InstanceNorms of the
formula-filled models and the chaotic AdamW traces it differs by more than those tolerances.  In float64 the reference and the oracle
agree to ~1e-15 on any host, so the CPU tests compare the oracle run in float64 against these files with the SAME tolerances.  The fp32
files stay: the GPU tests compare the HIP fp32 / bf16 paths against them.  Same inputs, seeds and key names as the fp32 generators, except
G8's prediction (pred_sample + pred_sums, see pred_sample).
"""
from __future__ import annotations

import os
import random
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_trace as GT  # noqa: E402
from oracle import gen_golden_trace2 as GT2  # noqa: E402
from oracle.gen_golden import OUT, REF, _install_shims, _np  # noqa: E402
from oracle.mae3d_oracle import formula_fill_, synthetic_grid  # noqa: E402

PRED_STRIDE = 8


def grid64(shape, seed):
    return synthetic_grid(shape, seed).double()


def _np32(t):
    """element-wise arrays are stored rounded to float32 (5e-8 relative, far inside the tests' tolerances) to keep the files small"""
    return _np(t).astype(np.float32)


def pred_sample(p):
    """G8's prediction (2 x 4 x 32^3) in less space: every PRED_STRIDE-th value of the flattened array, and the sum, absolute sum and sum of squares
    of ALL values in float64 -- a deviation of 2e-5 in any single value moves the absolute sum by more than the 1e-10 the test allows"""
    p = p.detach().double().reshape(-1)
    return _np32(p[::PRED_STRIDE]), np.array([p.sum().item(), p.abs().sum().item(), (p * p).sum().item()])


def g7_g8_g9(R):
    """the formula-filled parts of gen_golden.main: G7 (SD off, seeded mask), G8 (+ eval and encoder features), G9"""
    kw = dict(patch_size=[4] * 3, window_size=[4] * 3, expand_dim=True, resolution=32, masking_prob=0.75,
              embed_dim=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24])
    m2 = R.SwinTransformer_MAE3D_New(stochastic_depth_prob=0.0, **kw)
    formula_fill_(m2)
    xg = [grid64((32, 32, 32), 11)]
    random.seed(42)
    l7 = m2(xg)
    l7[0].backward()
    gn = {n: float(p.grad.double().norm()) for n, p in m2.named_parameters() if p.grad is not None}
    random.seed(42)
    with torch.no_grad():
        xb, vb = m2.transform(xg)
        pred7, _ = m2.forward_encoder_ecoder(torch.cat(xb, 0))
    np.savez_compressed(os.path.join(OUT, "g7_swin_t_32_fp64.npz"),
                        losses=np.array([float(v) for v in l7], np.float64), pred=_np32(pred7),
                        grad_names=np.array(list(gn.keys())), grad_norms=np.array(list(gn.values()), np.float64),
                        d_mask_token=_np32(m2.mask_token.grad), d_out_w=_np32(m2.out.conv.weight.grad),
                        d_bias_table_s0b1=_np32(m2.stages[0][1].attn.relative_position_bias_table.grad))

    kw8 = dict(patch_size=[4] * 3, window_size=[4] * 3, expand_dim=True, resolution=32, masking_prob=0.75,
               embed_dim=24, depths=[2, 2, 2, 2], num_heads=[3, 6, 12, 24], stochastic_depth_prob=0.0)
    m8 = R.SwinTransformer_MAE3D_New(**kw8)
    formula_fill_(m8)
    x8 = [grid64((30, 28, 32), 21), grid64((32, 32, 20), 22)]
    random.seed(8)
    l8 = m8(x8)
    l8[0].backward()
    g8 = {"losses": np.array([float(v) for v in l8], np.float64)}
    names = [n for n, p in m8.named_parameters() if p.grad is not None]
    g8["grad_names"] = np.array(names)
    g8["grad_norms"] = np.array([float(dict(m8.named_parameters())[n].grad.double().norm()) for n in names])
    for n in ["mask_token", "patch_partition.0.weight", "stages.1.0.reduction.weight", "decoder1.transp_conv.weight",
              "decoder1.conv_block.conv1.weight", "decoder4.conv_block.conv3.weight", "stages.3.2.attn.qkv.weight",
              "stages.0.1.attn.relative_position_bias_table", "out.conv.bias"]:
        g8["d_" + n] = _np32(dict(m8.named_parameters())[n].grad)
    random.seed(8)
    ev = m8(x8, is_eval=True)
    g8["eval_pred_sum"] = np.array([ev[3].double().sum().item(), ev[3].double().abs().sum().item()])
    g8["eval_mask_count"] = np.array([int(ev[4].sum())])
    g8["eval_shapes"] = np.array([list(ev[3].shape), list(ev[4].shape), list(ev[5].shape)])
    random.seed(8)
    with torch.no_grad():
        xb, vb = m8.transform(x8)
        pred8, _ = m8.forward_encoder_ecoder(torch.cat(xb, 0))
    g8["pred_sample"], g8["pred_sums"] = pred_sample(pred8)
    with torch.no_grad():
        t = m8.patch_partition(torch.cat(xb, 0))
        t = t + m8.pos_embed
        for i, st in enumerate(m8.stages):
            t = st(t)
            f = torch.permute(t, [0, 4, 1, 2, 3]).contiguous()
            g8[f"feat{i}_shape"] = np.array(f.shape)
            g8[f"feat{i}_sum"] = np.array([f.double().sum().item(), f.double().abs().sum().item()])
            if i >= 2:
                g8[f"feat{i}"] = _np32(f)
    np.savez_compressed(os.path.join(OUT, "g8_tiny_model_fp64.npz"), **g8)

    m9 = R.SwinTransformer_MAE3D_New(**kw8)
    formula_fill_(m9)
    opt = torch.optim.AdamW(m9.parameters(), lr=1e-4, weight_decay=1e-3)
    sch = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=1e-4, total_steps=10)
    random.seed(9)
    trace = []
    for step in range(10):
        opt.zero_grad()
        loss, lr_, la_ = m9([grid64((32, 32, 32), 100 + step)])
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m9.parameters(), 0.1)
        opt.step()
        sch.step()
        trace.append([float(loss), float(lr_), float(la_)])
    np.savez_compressed(os.path.join(OUT, "g9_train_trace_fp64.npz"), trace=np.array(trace, np.float64))


def main():
    assert os.path.isdir(REF), "reference not mounted"
    torch.set_default_dtype(torch.float64)
    _install_shims()
    sys.path.insert(0, REF)
    from nerf_mae.model.mae import swin_mae3d as R
    g7_g8_g9(R)
    # G13 / G14: the trace generators themselves, on float64 grids, writing into a scratch directory
    with tempfile.TemporaryDirectory() as tmp:
        for mod, name in ((GT, "g13_train_trace_hd32"), (GT2, "g14_train_trace_wellcond")):
            mod.synthetic_grid, mod.OUT = grid64, tmp
            mod.main()
            os.replace(os.path.join(tmp, name + ".npz"), os.path.join(OUT, name + "_fp64.npz"))
    print("fp64 goldens written to", OUT)


if __name__ == "__main__":
    main()
