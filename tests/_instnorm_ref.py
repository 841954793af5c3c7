"""float64 reference of the InstanceNorm + LeakyReLU (+ residual) kernels of csrc/norm.hip, one function per kernel, with elementwise error
bounds derived from the arithmetic and pure-Python mirrors of the launch geometry.

Tensors are channels-last [B, V, C] float64 (already rounded to the storage type by the caller); statistics are [B, C, 2] = (mean, rstd), sums
[B, C, 2] = (S1, S2) as the kernels lay them out.  Every function that consumes statistics takes the fp32 values the kernel is handed (stats32) and
widens them: what is left between the reference and the kernel is the kernel's own rounding, and the LeakyReLU sign is decided on the same number
(x - mu in fp32 has the exact sign of the real difference of two fp32 values).

Bounds.  u = 2^-24 is the fp32 unit roundoff, 2^-8 the worst relative error of one bf16 rounding.
  gamma(L) = 4 (L + 8) u     fp32 accumulation along a chain of L additions, first-order L u sum|term| for ANY order of that length, with a factor-4
                             margin (the + 8 covers the handful of roundings of the term itself and of the fp64 -> fp32 hand-over).
  L                          the longest fp32 chain of a reduction: the voxels one thread visits in its block, ceil(min(vpb, V) / NV), plus the NV
                             partials the block then adds in fp32; across blocks the sums are fp64 atomics (2^-53: not modelled).
"""
import numpy as np
import torch

U32 = 2.0 ** -24
EPS = float(np.float32(1e-5))      # the kernels receive eps and slope as fp32 arguments
SLOPE = float(np.float32(0.01))
IN_STREAM_MAX_C = 96
DATA_CLASSES = ("benign", "offset", "outlier", "constant", "benign2")


# ---------------------------------------------------------------------------------------------- launch geometry (mirrors of csrc/norm.hip)
def nv(C):
    """voxel lanes of a 256-thread block: one thread per 8-channel chunk, 256 / (C / 8) voxels side by side (idle threads for C = 48, 96, 192)"""
    return 256 // (C // 8)


def in_vox_per_block(V, B=4):
    """voxels per block of the reductions (the forward reduce passes no B: 4)"""
    per_sample = 256 if B >= 4 else 1024 // max(B, 1)
    vpb = -(-V // per_sample)
    vpb = (vpb + 63) // 64 * 64
    return max(vpb, 128)


def in_apply_vpb(V, B, C, streaming=False, mult=8, env_vpb=0):
    """voxels per block of the apply passes; streaming: mult x NV (mult 4 forward, 8 backward) unless NMH_IN_STREAM_VPB sets it"""
    if streaming:
        return env_vpb if env_vpb > 0 else mult * nv(C)
    vpb = (V * B + 1023) // 1024
    vpb = max(vpb, 4 * nv(C))
    return min(vpb, 2048)


def apply_streaming(V, B, C, bf16, min_mb=300.0, on=1):
    """the predicate of the streaming (short block, LDS table) form of the apply passes"""
    return bool(on) and bool(bf16) and C <= IN_STREAM_MAX_C and float(V) * B * C * 2 >= 1.0e6 * min_mb


def reduce_chain(V, C, B=4):
    """L of gamma for in_reduce_kernel: per-thread voxels of the fullest block + the NV partials"""
    vpb = in_vox_per_block(V, B)
    return -(-min(vpb, V) // nv(C)) + nv(C)


def gamma(L):
    return 4.0 * (L + 8) * U32


def c_supported(C):
    return C % 8 == 0 and C // 8 <= 256


# ---------------------------------------------------------------------------------------------- the cases (shared by the CPU emulation and the GPU tests)
CS = (8, 24, 40, 48, 96, 192, 384, 2048)
STATS_BS = (1, 3, 5)
MAX_ELEMS = 2_000_000


def stats_vs(C):
    """voxel counts of the statistics cases, from the formulas: 1, NV - 1 (fewer voxels than lanes), 127 / 128 / 129 around the smallest block, k blocks + 1,
    and one block plus 2 NV + 1 voxels (three of the four unroll slots in use, the third partly: a ragged U = 4 tail); C = 48 also takes the 4099 voxels of
    the figures in the docstring of tests/test_instnorm_ref_cpu.py"""
    n, vpb = nv(C), in_vox_per_block(1)
    k = 2 if C >= 2048 else 3
    vs = {1, max(n - 1, 1), 127, 128, 129, k * vpb + 1, vpb + 2 * n + 1}
    if C == 48:
        vs.add(4099)
    assert all(in_vox_per_block(v) == vpb for v in vs)
    return sorted(vs)


def stats_cases(C):
    return [(B, V) for B in STATS_BS for V in stats_vs(C) if B * V * C <= MAX_ELEMS]


BWD_REDUCE_BS = (1, 2, 4, 5)
BWD_REDUCE_MODES = ("r0_no_out", "r0", "r1", "r2")
# (C, V): small blocks with idle lanes, several blocks, and one volume large enough that per_sample (B >= 4) changes vpb: 33000 voxels are 192 per block
# for B >= 4 and 128 below
BWD_REDUCE_SHAPES = ((48, 129), (192, 385), (8, 33000))
assert in_vox_per_block(33000, 4) == 192 and in_vox_per_block(33000, 2) == 128 and in_vox_per_block(33000, 1) == 128


def bwd_reduce_inputs(B, V, C, dt, mode):
    """-> dict of float64 tensors rounded to dt: x (hard), dout, r, out (the reference forward output, the sign source), stats32, stats_r32, rmode"""
    rmode = {"r0_no_out": 0, "r0": 0, "r1": 1, "r2": 2}[mode]
    x = hard_input(B, V, C, dt, seed=7)
    dout = benign(B, V, C, dt, 8)
    r = benign(B, V, C, dt, 9, 1.0, 0.5) if rmode else None
    st = stats32_of(x)
    st_r = stats32_of(r) if rmode == 2 else None
    out = None
    if mode != "r0_no_out":
        out = apply(x, st, r, st_r, rmode)[0].to(dt).double()
    return dict(x=x, dout=dout, r=r, out=out, stats32=st, stats_r32=st_r, rmode=rmode)


# ---------------------------------------------------------------------------------------------- inputs
def hard_input(B, V, C, dt, seed=0, zero_sample=True):
    """[B, V, C] float64, rounded to dt, the data class varied per channel (channel c has class DATA_CLASSES[c % 5]):
    benign N(0.3, 1.5); offset N(20, 0.5) (mean 40 sigma from zero); outlier N(0, 1) with the sample's FIRST voxel -- the reduction's shift -- at +30;
    constant (the var < 0 clamp: rstd = eps^-1/2, mean exact); and, for B > 1, the last sample all zeros."""
    g = torch.Generator().manual_seed(1234 + seed)
    x = torch.randn(B, V, C, generator=g, dtype=torch.float64)
    cls = torch.arange(C) % 5
    x[:, :, cls == 0] = x[:, :, cls == 0] * 1.5 + 0.3
    x[:, :, cls == 1] = x[:, :, cls == 1] * 0.5 + 20.0
    x[:, 0, cls == 2] += 30.0
    x[:, :, cls == 3] = (torch.arange(C)[cls == 3].double() * 0.125 - 3.0)[None, None, :]
    x[:, :, cls == 4] = x[:, :, cls == 4] * 0.25 - 1.0
    if zero_sample and B > 1:
        x[B - 1] = 0.0
    return x.to(dt).double()


def benign(B, V, C, dt, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(4321 + seed)
    return (torch.randn(B, V, C, generator=g, dtype=torch.float64) * scale + shift).to(dt).double()


def stats32_of(x, eps=EPS):
    """the statistics a kernel downstream is handed: float64 statistics rounded once to fp32, [B, C, 2]"""
    mu, rstd = stats(x, eps)
    return torch.stack([mu, rstd], -1).float()


# ---------------------------------------------------------------------------------------------- the reference, kernel by kernel
def stats(x, eps=EPS):
    """-> mu, rstd = (sigma^2 + eps)^-1/2 (biased variance), each [B, C] float64"""
    mu = x.mean(1)
    var = ((x - mu[:, None]) ** 2).mean(1)
    return mu, (var + eps) ** -0.5


def stats_bounds(x, c, L, eps=EPS):
    """-> (bound on |mean - mu|, bound on |rstd' / rstd - 1|), each [B, C], for sums of (x - c), (x - c)^2 taken in fp32 along chains of length L.
       |mean - mu|   <= 2^-23 |mu| + gamma mean|x - c|                 (the rounding of the stored mean; the fp32 sum of the shifted values)
       rel. rstd     <= 2^-22 + 1/2 (gamma E[(x - c)^2] + 2 |mu - c| dmean) / (sigma^2 + eps),   dmean = gamma mean|x - c|
                        (rstd = (var + eps)^-1/2: half the relative error of var + eps; var = E[(x - c)^2] - (mu - c)^2 inherits the error of both sums)"""
    mu, _ = stats(x, eps)
    var = ((x - mu[:, None]) ** 2).mean(1)
    d = x - c[:, None]
    gm = gamma(L)
    dmean = gm * d.abs().mean(1)
    b_mean = 2.0 ** -23 * mu.abs() + dmean
    b_rstd = 2.0 ** -22 + 0.5 * (gm * (d * d).mean(1) + 2.0 * (mu - c).abs() * dmean) / (var + eps)
    return b_mean, b_rstd


def finalize(acc, V, eps=EPS):
    """in_finalize_kernel on fp64 sums (no shift): acc [..., 2] = (sum x, sum x^2) -> mean, rstd float64 (var clamped at 0)"""
    m = acc[..., 0] / V
    var = (acc[..., 1] / V - m * m).clamp_min(0.0)
    return m, (var + eps) ** -0.5


def _split(stats32):
    s = stats32.double()
    return s[:, None, :, 0], s[:, None, :, 1]


def apply(x, stats32, r=None, stats_r32=None, rmode=0, slope=SLOPE):
    """-> out = lrelu((x - mu) rstd [+ r | + (r - mu_r) rstd_r]) and `mag`, the sum of the magnitudes of the terms the kernel adds, each scaled as it
    enters the sum: (|x| + |mu|) rstd [+ |r| | + (|r| + |mu_r|) rstd_r]"""
    mu, rs = _split(stats32)
    y = (x - mu) * rs
    mag = (x.abs() + mu.abs()) * rs
    if rmode == 1:
        y = y + r
        mag = mag + r.abs()
    elif rmode == 2:
        mur, rsr = _split(stats_r32)
        y = y + (r - mur) * rsr
        mag = mag + (r.abs() + mur.abs()) * rsr
    return torch.where(y > 0, y, slope * y), mag


def apply_bound(ref, mag, bf16):
    """|out - ref| <= 2^-8 |ref| (bf16 store; 2^-23 |ref| for fp32) + 2^-22 mag: at most four fp32 roundings (subtract, scale, add, slope), each
    relative to a value no larger than mag.  LeakyReLU is 1-Lipschitz and continuous: an element whose sign flips inside this error is still inside it."""
    return (2.0 ** -8 if bf16 else 2.0 ** -23) * ref.abs() + 2.0 ** -22 * mag


def _g(dout, sign_source, x, mu, slope):
    src = sign_source if sign_source is not None else x - mu
    return dout * torch.where(src > 0, torch.ones_like(dout), torch.full_like(dout, slope))


def bwd_sums(dout, sign_source, x, stats32, r=None, stats_r32=None, rmode=0, slope=SLOPE):
    """-> dict: S [B, C, 2] = (sum g, sum g xhat), Sr (rmode 2: (sum g, sum g rhat)), and the absolute sums A / Ar of the same terms (for the bounds)"""
    mu, rs = _split(stats32)
    g = _g(dout, sign_source, x, mu, slope)
    xh = (x - mu) * rs
    o = dict(S=torch.stack([g.sum(1), (g * xh).sum(1)], -1), A=torch.stack([g.abs().sum(1), (g * xh).abs().sum(1)], -1), Sr=None, Ar=None)
    if rmode == 2:
        mur, rsr = _split(stats_r32)
        rh = (r - mur) * rsr
        o["Sr"] = torch.stack([g.sum(1), (g * rh).sum(1)], -1)
        o["Ar"] = torch.stack([g.abs().sum(1), (g * rh).abs().sum(1)], -1)
    return o


def bwd_sums_bound(A, L):
    """[B, C, 2]: |S1' - S1| <= (gamma + 2 u) sum|g|  (g = dout * slope rounds once, doubled), |S2' - S2| <= (gamma + 8 u) sum|g xhat|  (g, x - mu, the
    scale by rstd and the product: four roundings per term, doubled); the fp64 atomics across blocks are not modelled (2^-53)"""
    gm = gamma(L)
    return torch.stack([(gm + 2 * U32) * A[..., 0], (gm + 8 * U32) * A[..., 1]], -1)


def bwd_apply(dout, sign_source, x, stats32, sums64, r=None, stats_r32=None, sums_r64=None, rmode=0, slope=SLOPE, dr0=None):
    """-> dict dx, dr (None for rmode 0) and the magnitudes mdx, mdr of the bounds.
    dx = rstd (g - S1/V - xhat S2/V); dr = g [+ dr0] (rmode 1), rstd_r (g - S1r/V - rhat S2r/V) (rmode 2)"""
    V = x.shape[1]
    mu, rs = _split(stats32)
    g = _g(dout, sign_source, x, mu, slope)
    xh = (x - mu) * rs
    m1, m2 = sums64[:, None, :, 0] / V, sums64[:, None, :, 1] / V
    o = dict(dx=rs * (g - m1 - xh * m2), mdx=rs * (g.abs() + m1.abs() + (xh * m2).abs()), dr=None, mdr=None)
    if rmode == 1:
        o["dr"] = g if dr0 is None else dr0 + g
        o["mdr"] = g.abs() if dr0 is None else dr0.abs() + g.abs()
    elif rmode == 2:
        mur, rsr = _split(stats_r32)
        rh = (r - mur) * rsr
        n1, n2 = sums_r64[:, None, :, 0] / V, sums_r64[:, None, :, 1] / V
        o["dr"] = rsr * (g - n1 - rh * n2)
        o["mdr"] = rsr * (g.abs() + n1.abs() + (rh * n2).abs())
    return o


def bwd_apply_bound(ref, mag, bf16):
    """2^-8 |ref| (bf16; 2^-23 |ref| fp32) + 4 * 2^-22 mag: the roundings of g, xhat, S/V (fp64 -> fp32, times an fp32 1/V), the fma and the final scale,
    each relative to a value no larger than mag = rstd (|g| + |S1/V| + |xhat S2/V|), with a factor-4 margin"""
    return (2.0 ** -8 if bf16 else 2.0 ** -23) * ref.abs() + 4.0 * 2.0 ** -22 * mag


def chain_autograd_inputs(B, V, C, rmode, seed=0):
    x = benign(B, V, C, torch.float64, seed, 1.5, 0.3)
    r = benign(B, V, C, torch.float64, seed + 1) if rmode else None
    dout = benign(B, V, C, torch.float64, seed + 2)
    return x, r, dout


# ---------------------------------------------------------------------------------------------- fp32 emulation of the reductions' summation order
def emulate_block_sums(terms, vpb, NV):
    """terms: float32 [V, K] (the per-voxel terms of one sample, already computed in fp32).  Sums them as in_reduce_kernel does: within a block of vpb
    voxels thread vl adds voxels vl, vl + NV, ... in fp32; the block then adds its NV partials in lane order in fp32; blocks meet in fp64.  -> float64 [K]"""
    terms = np.ascontiguousarray(terms, dtype=np.float32)
    V, K = terms.shape
    total = np.zeros(K, dtype=np.float64)
    for v0 in range(0, V, vpb):
        blk = terms[v0:min(v0 + vpb, V)]
        n = blk.shape[0]
        steps = -(-n // NV)
        pad = np.zeros((steps * NV, K), dtype=np.float32)   # (adding +0 is exact: the kernel's idle slots add nothing)
        pad[:n] = blk
        pad = pad.reshape(steps, NV, K)
        part = np.zeros((NV, K), dtype=np.float32)
        for s in range(steps):
            part = (part + pad[s]).astype(np.float32)
        t = np.zeros(K, dtype=np.float32)
        for q in range(NV):
            t = (t + part[q]).astype(np.float32)
        total += t.astype(np.float64)
    return total


def emulate_stats(x, C, shift_first=True, vpb=None, NV=None, eps=EPS, store32=False):
    """fp32 emulation of nmh_instnorm_stats (shift_first) or of epilogue sums + nmh_instnorm_finalize (shift 0) on x [B, V, C] -> mean, rstd [B, C] float64.
    store32: also round the two results to fp32 as the kernel stores them.  Off by default: the store is one rounding to the output format, up to 2^-24
    relative whatever the input, which the bounds carry as a term of its own (2^-23 |mu|, 2^-22) -- the quarter-of-the-bound margin is asked of the
    summation, and a kernel that meets it lands within 1/4 + 1/2 of the bound after the store."""
    B, V, _ = x.shape
    vpb = vpb or in_vox_per_block(V)
    NV = NV or nv(C)
    means, rstds = [], []
    for b in range(B):
        xb = x[b].numpy().astype(np.float32)
        c = xb[0] if shift_first else np.zeros(C, dtype=np.float32)
        d = (xb - c[None]).astype(np.float32)
        s1 = emulate_block_sums(d, vpb, NV)
        s2 = emulate_block_sums((d * d).astype(np.float32), vpb, NV)
        m = s1 / V
        var = np.maximum(s2 / V - m * m, 0.0)
        m = m + c.astype(np.float64)
        rs = 1.0 / np.sqrt(var + eps)
        means.append(m.astype(np.float32).astype(np.float64) if store32 else m)
        rstds.append(rs.astype(np.float32).astype(np.float64) if store32 else rs)
    return torch.from_numpy(np.stack(means)), torch.from_numpy(np.stack(rstds))


def emulate_bwd_sums(dout, sign_source, x, stats32, r, stats_r32, rmode, B_launch, slope=SLOPE):
    """fp32 emulation of nmh_instnorm_bwd_reduce -> S, Sr as bwd_sums"""
    B, V, C = x.shape
    vpb, NV = in_vox_per_block(V, B_launch), nv(C)
    f = np.float32
    S, Sr = np.zeros((B, C, 2)), np.zeros((B, C, 2))
    for b in range(B):
        xb, db = x[b].numpy().astype(f), dout[b].numpy().astype(f)
        mu, rs = stats32[b, :, 0].numpy()[None], stats32[b, :, 1].numpy()[None]
        t = (xb - mu).astype(f)
        src = sign_source[b].numpy().astype(f) if sign_source is not None else t
        g = (db * np.where(src > 0, f(1.0), f(slope))).astype(f)
        S[b, :, 0] = emulate_block_sums(g, vpb, NV)
        S[b, :, 1] = emulate_block_sums(((g * t).astype(f) * rs).astype(f), vpb, NV)
        if rmode == 2:
            mur, rsr = stats_r32[b, :, 0].numpy()[None], stats_r32[b, :, 1].numpy()[None]
            tr = (r[b].numpy().astype(f) - mur).astype(f)
            Sr[b, :, 0] = S[b, :, 0]
            Sr[b, :, 1] = emulate_block_sums(((g * tr).astype(f) * rsr).astype(f), vpb, NV)
    return torch.from_numpy(S), (torch.from_numpy(Sr) if rmode == 2 else None)


# ---------------------------------------------------------------------------------------------- comparison
def ratio_check(got, ref, bound, name, frac=1.0):
    """elementwise |got - ref| <= frac * bound; where the bound is 0 the value must be exact.  -> the worst |err| / bound (printed, for the record)"""
    got, ref, bound = got.detach().double().cpu(), ref.double(), bound.double()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    bad = err > frac * bound
    pos = bound > 0
    worst = float((err[pos] / bound[pos]).max()) if bool(pos.any()) else 0.0
    print(f"  [{name}] max |err| / bound = {worst:.3g}")
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside {frac} x the derived bound; first at {i}: "
                             f"got {got[i].item():.9g}, ref {ref[i].item():.9g}, |err| {err[i].item():.3e} > {frac * bound[i].item():.3e}")
    return worst
