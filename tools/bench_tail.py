"""Micro-benchmark of the decoder-tail backward kernels at the bench shape (B grids of 160^3 x 48)."""
import sys
import time
import torch
sys.path.insert(0, ".")
from nerf_mae_amd import ops

B, R, Cd = int(sys.argv[1]) if len(sys.argv) > 1 else 4, 160, 48
V = R ** 3
dev = "cuda"
dt = torch.bfloat16


def box_section(reps=7, n=10):
    """`bench_tail.py B box`: the step's two tail launches (forward with the residual formed from the coarse tensor, apply pass of the backward) walking the whole
    grid against each sample's valid box alone, for the benchmark's extents mix and for full cubes; `reps` interleaved repeats of `n` calls, min / median / max"""
    gd = R // 4
    mix = [[160, 160, 160], [160, 132, 96], [120, 160, 144]]   # bench.py's scenes, cycling over the slots
    y = torch.randn(B * V, Cd, device=dev, dtype=dt)
    xc = torch.randn(B, gd, gd, gd, 96, device=dev, dtype=dt)
    Wt, bt = torch.randn(96, 48, 4, 4, 4, device=dev) * 96 ** -0.5, torch.randn(48, device=dev) * 0.5
    ws = torch.empty(ops.cconv_pack_ws_floats(), dtype=torch.float32, device=dev)
    ops.cconv_pack(Wt, torch.randn(48, 48, 3, 3, 3, device=dev), bt, torch.empty(ops.cconv_pack_numel(), dtype=dt, device=dev), torch.empty(27, 48, device=dev), ws)
    Wres = torch.empty(ops.tail_residual_pack_numel(), dtype=dt, device=dev)
    ops.tail_residual_pack(ws, Wres)
    stats = torch.empty(B, Cd, 2, device=dev)
    ops.instnorm_stats(y, stats, torch.empty(B, Cd, 2, dtype=torch.float64, device=dev), B, V, Cd)
    Wo, bo = torch.randn(4, Cd, device=dev) * 0.1, torch.zeros(4, device=dev)
    tm = (torch.rand(gd ** 3, device=dev) < 0.75).to(torch.uint8)
    lsums, losses = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(3, device=dev)
    dpred, smask = torch.zeros(B * V, 4, device=dev), torch.zeros(B * V, 8, dtype=torch.uint8, device=dev)
    bsum = torch.empty(B * Cd * 4 + 4 * Cd, dtype=torch.float64, device=dev)
    dy, dr = torch.empty_like(y), torch.empty_like(y)
    dW, db, sums = torch.zeros(4, Cd, device=dev), torch.zeros(4, device=dev), torch.empty(B, Cd, 2, dtype=torch.float64, device=dev)
    for name, exts in (("bench mix", [mix[i % 3] for i in range(B)]), ("full cubes", [[R, R, R]] * B)):
        x = torch.rand(B, 4, R, R, R, device=dev)
        for i, e in enumerate(exts):   # zero padding outside the extents: the box walk's precondition
            x[i, :, e[0]:] = 0; x[i, :, :, e[1]:] = 0; x[i, :, :, :, e[2]:] = 0
        ext = torch.tensor(exts, dtype=torch.int32, device=dev)
        inside = sum(((e[0] + 3) // 4) * ((e[1] + 3) // 4) * ((e[2] + 3) // 4) for e in exts) / (B * gd ** 3)

        def fwd(box):
            ops.mae_tail_fwd_from_coarse(y, stats, xc, Wres, bt, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, dpred, bsum, smask, box=box)

        def bwd(box):
            ops.mae_tail_bwd(None, y, stats, dpred, lsums, Wo, sums, dy, dr, dW, db, B, V, Cd, bwd_sums=bsum, sign_mask=smask, **(dict(extents=ext, R=R) if box else {}))

        t = {k: [] for k in ("fwd full", "fwd box", "bwd full", "bwd box")}
        for _ in range(reps):
            for box in (False, True):
                t["fwd box" if box else "fwd full"].append(timeit(lambda: fwd(box), n))
            for box in (False, True):
                fwd(box)
                t["bwd box" if box else "bwd full"].append(timeit(lambda: bwd(box), n))
        print(f"{name} ({B} x {R}^3, {100 * inside:.1f} % of the cells inside):")
        for k, v in t.items():
            v = sorted(v)
            print(f"  tail {k}: min {v[0]:.3f}  median {v[len(v) // 2]:.3f}  max {v[-1]:.3f} ms")


def timeit(f, n=10):
    f(); torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(n):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / n * 1e3


if len(sys.argv) > 2 and sys.argv[2] == "box":
    box_section()
    sys.exit(0)

d0 = torch.randn(B * V, Cd, device=dev, dtype=dt)
y = torch.randn(B * V, Cd, device=dev, dtype=dt)
x = torch.rand(B, 4, R, R, R, device=dev)
ext = torch.tensor([[R, R, R]] * B, dtype=torch.int32, device=dev)
tm = (torch.rand(40 ** 3, device=dev) < 0.75).to(torch.uint8)
Wo, bo = torch.randn(4, Cd, device=dev) * 0.1, torch.zeros(4, device=dev)
stats = torch.empty(B, Cd, 2, device=dev)
scr = torch.empty(B, Cd, 2, dtype=torch.float64, device=dev)
ops.instnorm_stats(y, stats, scr, B, V, Cd)
lsums, losses = torch.empty(8, dtype=torch.float64, device=dev), torch.empty(3, device=dev)
dpred = torch.empty(B * V, 4, device=dev)
ops.mae_loss_fwd(d0, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred)
dy, dr, dd0 = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
dW, db = torch.zeros(4, Cd, device=dev), torch.zeros(4, device=dev)
sums = torch.empty(B, Cd, 2, dtype=torch.float64, device=dev)
r =torch.randn_like(y)


def fused():
    ops.mae_tail_bwd(None, y, stats, dpred, lsums, Wo, sums, dy, dr, dW, db, B, V, Cd, r=r)


def fused_stored():
    ops.mae_tail_bwd(d0, y, stats, dpred, lsums, Wo, sums, dy, dr, dW, db, B, V, Cd)


def unfused():
    ops.mae_loss_bwd(d0, Wo, bo, x, ext, tm, B, R, Cd, lsums, dd0, torch.empty(1, 8, device=dev, dtype=dt), dW, db)
    ops.instnorm_bwd_reduce(dd0, d0, y, stats, sums, B, V, Cd, r=d0, rmode=1)
    ops.instnorm_bwd_apply(dd0, d0, y, stats, sums, dy, B, V, Cd, r=d0, rmode=1, dr=dr)


print(f"fused tail bwd  {timeit(fused):.3f} ms (stored d0: {timeit(fused_stored):.3f})   unfused {timeit(unfused):.3f} ms   loss fwd {timeit(lambda: ops.mae_loss_fwd(d0, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None)):.3f} / with dpred {timeit(lambda: ops.mae_loss_fwd(d0, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred)):.3f} ms")
out = torch.empty_like(y)
t_f0 = timeit(lambda: ops.mae_tail_fwd(y, stats, r, None, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred))
t_f = timeit(lambda: ops.mae_tail_fwd(y, stats, r, out, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred))
t_u = timeit(lambda: (ops.instnorm_apply(y, stats, out, B, V, Cd, r=r, rmode=1), ops.mae_loss_fwd(out, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred)))
print(f"fused tail fwd {t_f:.3f} ms (d0 not stored: {t_f0:.3f})   unfused (in_apply + loss fwd) {t_u:.3f} ms")
bsum = torch.empty(B * Cd * 4 + 4 * Cd, dtype=torch.float64, device=dev)
t_m = timeit(lambda: ops.mae_tail_fwd(y, stats, r, None, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred, bwd_sums=bsum))
print(f"fused tail fwd + backward sums (the step's launch; bf16 C=48: matrix-core kernel) {t_m:.3f} ms")
smask = torch.empty(B * V, 8, dtype=torch.uint8, device=dev)
ops.mae_tail_fwd(y, stats, r, None, Wo, bo, x, ext, tm, B, R, Cd, lsums, losses, None, dpred, bwd_sums=bsum, sign_mask=smask)
t_b = timeit(lambda: ops.mae_tail_bwd(None, y, stats, dpred, lsums, Wo, sums, dy, dr, dW, db, B, V, Cd, bwd_sums=bsum, sign_mask=smask))
gb = B * V * (3 * Cd * 2 + 8 + 16) / 1e9
print(f"tail bwd apply pass with the forward's sums + sign mask (the step's launch) {t_b:.3f} ms ({gb / t_b:.2f} TB/s)")
