"""Every gemm_nt / gemm_tn kernel the dispatch can pick, against float64, chosen by its named plan.

Each case of tests/_gemm_cases.py names the kernel it is meant to reach; the test asks the library's plan query first and asserts that
name, so a run cannot pass on another kernel.  Inputs are rounded to the storage type before the float64 reference sees them.

Two checks per output.  (1) tests/_metrics.assert_close at the suite's TOL (2e-4 fp32, 3e-2 bf16).  (2) For bf16 an elementwise bound
derived from the arithmetic, so that one dropped 8-element chunk or one wrong row cannot hide in an rms-scaled tolerance:

    |got - ref| <= 2^-8 |ref| + e_acc' + e_f32            e_acc = (K + 8) 2^-22 (|A| |W|^T)

  2^-8 |ref|   one bf16 rounding of the stored value: bf16 keeps 8 significant bits, so round-to-nearest is off by up to 2^-8 relative just
               above a power of two -- this term has no slack of its own (what the fp32 value differs from ref by is in the other two);
  e_acc        fp32 accumulation of exact bf16 products in any order (K 2^-24 |A||W|^T to first order), with a factor-4 margin;
  e_acc'       e_acc carried through the epilogue (csrc/gemm.hip epilogue8), below;
  e_f32        the epilogue's own fp32 roundings: 2^-22 times the sum of the magnitudes of the terms it adds (each add or multiply
               rounds to 2^-24 relative).
  plain, bias          v = acc + b                      e_acc' = e_acc
  act 1                C2 = bf16(v); out = bf16(gelu(v)): |gelu'| <= 1.13, and gelu_fast_f (common.hpp: erf_as_parts states 1.5e-7
                       absolute on erf; v_rcp / v_exp are 1 ulp) is within 0.5 |v| (1.5e-7 + 4 * 2^-24) < 2e-7 |v| of gelu, doubled:
                       e_acc' = 1.13 (e_acc + e_f32) + 4e-7 |v|
  act 2, row scale     out = bf16(acc * gelu'(C2) * s): gelu_grad_fast_f is within 0.5 * 1.5e-7 + 0.4 |x| * 2^-21 of gelu' (the erf formula's
                       own exponential, 1 ulp of v_exp on a value <= 1): e_acc' = |s| (1.13 e_acc + |acc| (1e-7 + 2e-7 |x|) * 2)
                       A scale of 0 gives bound 0: the stored value must be exactly zero.
  resid, scale, accumulate   out = bf16(s (acc + b) + resid + out0), all in fp32 after the bf16 loads of resid and out0 (exact):
                       e_acc' = |s| e_acc; e_f32 = 2^-22 (|s| (|A||W|^T + |b|) + |resid| + |out0|): their own roundings.
Measured on an MI355X, maximum of |got - ref| / bound over all cases: plain 0.982, bias 0.983, act 1 0.983 (C2) / 0.982 (out), act 2 0.977,
resid + scale + accumulate 0.996 -- i.e. the rounding term is met almost exactly by some element of a few hundred thousand (as it must be:
it is sharp) and nothing else contributes visibly; no term was widened.  The kernels are deterministic, so these figures do not move.

gemm_tn writes fp32: the bound keeps the accumulation term over the M contraction rows (whatever the split, partial-sum or atomic order)
and the final fp32 add into the pre-filled output; the bf16 rounding of the row-scaled operand is modelled in the reference itself, as
test_kernels_gpu.test_gemm_tn does:   |got - ref| <= (M + 8) 2^-22 (|As|^T |B|) + 2^-22 |ref|.  Measured: at most 0.001 of the bound -- a
worst-case bound over M >= 777 terms lies far above the error of a sum of random signs, so for gemm_tn check (1) is the sharper of the
two; the bound is kept because it is elementwise (no rms of the whole tensor to hide in) and holds for any summation order.

Not covered: a DMA ring of depth 3 (NMH_GEMM_DMA is read once per process, and no test here starts another process)."""
import functools

import pytest
import torch

from tests._gemm_cases import BF, F32, NT_CASES, TN_CASES
from tests._metrics import assert_close

pytestmark = pytest.mark.gpu

TOL = {F32: 2e-4, BF: 3e-2}
EPILOGUES = ("plain", "bias", "gelu_dual", "gelu_grad_rowscale", "resid_rowscale_accumulate")


def _ops():
    from nerf_mae_amd import ops
    return ops


def _rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def _q(t, dt):
    return t.to(dt).double()


def _bound_check(got, ref, bound, name):
    """elementwise: |got - ref| <= bound everywhere (and the worst ratio, for the record)"""
    got = got.detach().double().cpu()
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    bad = err > bound
    ok = ~bad & (bound > 0)
    print(f"  [{name}] max |got - ref| / bound = {(err[ok] / bound[ok]).max().item() if ok.any() else 0.0:.3f}, {int(bad.sum())} elements outside")
    assert not bad.any(), (f"{name}: {int(bad.sum())} of {bad.numel()} elements outside the derived bound; first at "
                           f"{tuple(bad.nonzero()[0].tolist())}: |err| {err[bad][0].item():.3e} > {bound[bad][0].item():.3e}")


@functools.lru_cache(maxsize=2)
def _nt_reference(cid):
    """operands (rounded to the storage type), the float64 product and |A| |W|^T of one case -- computed once, shared by its five epilogues"""
    c = next(c for c in NT_CASES if c.id == cid)
    M, N, K, dt = c.M, c.N, c.K, c.dtype
    seed = 1000 + NT_CASES.index(c)
    A, W = _q(_rnd(M, K, seed=seed), dt), _q(_rnd(N, K, seed=seed + 1, scale=K ** -0.5), dt)
    r = dict(A=A, W=W, acc=A @ W.T, S=A.abs() @ W.abs().T, b=_rnd(N, seed=seed + 2).double(),
             aux=_q(_rnd(M, N, seed=seed + 3), dt), res=_q(_rnd(M, N, seed=seed + 4), dt), c0=_q(_rnd(M, N, seed=seed + 5), dt))
    # a row scale with a 0 and a value other than 1, over samples whose length is no multiple of any row tile (16 .. 256)
    rps = (M + 2) // 3 | 1
    rs = torch.tensor([1.0 / 0.9, 0.0, 0.75, 1.0])[: (M + rps - 1) // rps]
    r["rps"], r["rs"], r["srow"] = rps, rs, rs.double().repeat_interleave(rps)[:M, None]
    assert rps % 16 != 0 and 0.0 in rs.tolist()
    return r


def _gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.5 ** 0.5))


def _gelu_grad64(x):
    return 0.5 * (1.0 + torch.erf(x * 0.5 ** 0.5)) + x * torch.exp(-0.5 * x * x) * 0.3989422804014327


def _dev(t, dt=None):
    return (t if dt is None else t.to(dt)).cuda().contiguous()


def _run_epilogue(ops, epi, r, dt, call):
    """-> [(name, got, ref, bound)] for one epilogue; `call(**kw)` launches gemm_nt on the case's operands"""
    acc, S, b, K = r["acc"], r["S"], r["b"], r["A"].shape[1]
    M, N = acc.shape
    e_acc = (K + 8) * 2.0 ** -22 * S
    u8, u22 = 2.0 ** -8, 2.0 ** -22
    if epi == "plain":
        return [("plain", call(), acc, u8 * acc.abs() + e_acc + u22 * S)]
    if epi == "bias":
        ref = acc + b
        return [("bias", call(bias=_dev(b.float())), ref, u8 * ref.abs() + e_acc + u22 * (S + b.abs()))]
    if epi == "gelu_dual":
        pre = torch.full((M, N), float("nan"), dtype=dt, device="cuda")
        out = call(bias=_dev(b.float()), act=1, C2=pre)
        v = acc + b
        e_v = e_acc + u22 * (S + b.abs())
        g = _gelu64(v)
        return [("gelu_dual pre", pre, v, u8 * v.abs() + e_v), ("gelu_dual act", out, g, u8 * g.abs() + 1.13 * e_v + 4e-7 * v.abs())]
    if epi == "gelu_grad_rowscale":
        out = call(act=2, C2=_dev(r["aux"], dt), rowscale=_dev(r["rs"]), rows_per_scale=r["rps"])
        s, x = r["srow"], r["aux"]
        ref = acc * _gelu_grad64(x) * s
        bound = u8 * ref.abs() + s.abs() * (1.13 * e_acc + 2 * acc.abs() * (1e-7 + 2e-7 * x.abs())) + u22 * ref.abs() * 2
        return [("gelu_grad_rowscale", out, ref, bound)]
    if epi == "resid_rowscale_accumulate":
        out = _dev(r["c0"], dt)
        call(bias=_dev(b.float()), resid=_dev(r["res"], dt), rowscale=_dev(r["rs"]), rows_per_scale=r["rps"], out=out, accumulate=True)
        s = r["srow"]
        ref = s * (acc + b) + r["res"] + r["c0"]
        bound = u8 * ref.abs() + s.abs() * e_acc + u22 * (s.abs() * (S + b.abs()) + r["res"].abs() + r["c0"].abs())
        return [("resid_rowscale_accumulate", out, ref, bound)]
    raise AssertionError(epi)


def _check_all(results, dt, label):
    for name, got, ref, bound in results:
        assert_close(got, ref.float(), TOL[dt], f"{label} {name}")
        if dt == BF:
            _bound_check(got, ref, bound, f"{label} {name}")


@pytest.mark.parametrize("epi", EPILOGUES)
@pytest.mark.parametrize("cid", [c.id for c in NT_CASES])
def test_gemm_nt_kernel_by_plan(cid, epi, monkeypatch):
    for v in ("NMH_GEMM_W22", "NMH_GEMM_CFG"):
        monkeypatch.delenv(v, raising=False)
    ops = _ops()
    c = next(c for c in NT_CASES if c.id == cid)
    p = ops.gemm_nt_plan(c.dtype, c.M, c.N, c.K)
    assert p[:4] == c.kernel and p[5] == c.narrow, p
    r = _nt_reference(cid)
    A, W = _dev(r["A"], c.dtype), _dev(r["W"], c.dtype)
    _check_all(_run_epilogue(ops, epi, r, c.dtype, lambda **kw: ops.gemm_nt(A, W, **kw)), c.dtype, f"{cid}")


# ---- tiles only a tuning variable reaches: one shape ragged on all three axes ------------------------------------------------------------
RAGGED = (300, 200, 136)
W22_CFGS = (442, 443, 432, 433, 242, 243, 244, 233, 234, 224, 423, 424)
CFG_TILES = [(BF, 1, 8), (BF, 4, 6), (BF, 4, 8), (F32, 1, 2), (F32, 4, 6), (F32, 4, 8)]   # the <MT,NT> tiles no default dispatch returns


@functools.lru_cache(maxsize=2)
def _ragged_reference(dt):
    M, N, K = RAGGED
    A, W = _q(_rnd(M, K, seed=77), dt), _q(_rnd(N, K, seed=78, scale=K ** -0.5), dt)
    r = dict(A=A, W=W, acc=A @ W.T, S=A.abs() @ W.abs().T, b=_rnd(N, seed=79).double(), aux=None,
             res=_q(_rnd(M, N, seed=80), dt), c0=_q(_rnd(M, N, seed=81), dt))
    r["rps"], r["rs"] = 101, torch.tensor([1.0 / 0.9, 0.0, 0.75])
    r["srow"] = r["rs"].double().repeat_interleave(101)[:M, None]
    return r


@pytest.mark.parametrize("epi", ["bias", "resid_rowscale_accumulate"])
@pytest.mark.parametrize("cfg", W22_CFGS)
def test_gemm_nt_forced_w22_configuration(cfg, epi, monkeypatch):
    """the twelve compiled 2 x 2-wave configurations, which NMH_GEMM_W22=<cfg> switches on in any process: 300 x 200 x 136 leaves a partial
    row tile, a partial column tile and a k-tile one chunk deep (K = 2 * 64 + 8) in every one of them"""
    ops = _ops()
    monkeypatch.delenv("NMH_GEMM_CFG", raising=False)
    monkeypatch.setenv("NMH_GEMM_W22", str(cfg))
    assert ops.gemm_nt_plan(BF, *RAGGED)[:4] == ("w22", cfg // 100, cfg // 10 % 10, cfg % 10)
    r = _ragged_reference(BF)
    A, W = _dev(r["A"], BF), _dev(r["W"], BF)
    _check_all(_run_epilogue(ops, epi, r, BF, lambda **kw: ops.gemm_nt(A, W, **kw)), BF, f"w22 {cfg}")


@pytest.mark.parametrize("epi", ["bias", "resid_rowscale_accumulate"])
@pytest.mark.parametrize("dt,mt,nt", CFG_TILES, ids=[f"{'bf16' if d == BF else 'fp32'}_{m}x{n}" for d, m, n in CFG_TILES])
def test_gemm_nt_forced_register_tile(dt, mt, nt, epi, monkeypatch):
    ops = _ops()
    monkeypatch.delenv("NMH_GEMM_W22", raising=False)
    monkeypatch.setenv("NMH_GEMM_CFG", f"{mt},{nt}")
    assert ops.gemm_nt_plan(dt, *RAGGED)[:4] == ("reg", mt, nt, 0)
    r = _ragged_reference(dt)
    A, W = _dev(r["A"], dt), _dev(r["W"], dt)
    _check_all(_run_epilogue(ops, epi, r, dt, lambda **kw: ops.gemm_nt(A, W, **kw)), dt, f"cfg {mt},{nt}")


# ---- strides ------------------------------------------------------------------------------------------------------------------------------
SENTINEL = -7.0


def _slice_of(t, dt, left, right):
    """t as a column slice of a wider device buffer filled with a sentinel -> (slice view, buffer)"""
    rows, cols = t.shape
    buf = torch.full((rows, left + cols + right), SENTINEL, dtype=dt, device="cuda")
    buf[:, left:left + cols] = t.to(dt).cuda()
    return buf[:, left:left + cols], buf


def _untouched(buf, left, cols):
    return bool((buf[:, :left] == SENTINEL).all()) and bool((buf[:, left + cols:] == SENTINEL).all())


@pytest.mark.parametrize("epi", ["gelu_dual", "gelu_grad_rowscale", "resid_rowscale_accumulate"])
@pytest.mark.parametrize("cid", ["reg_1x6", "dma_1x3_narrow", "k128_6", "w22_233"])
def test_gemm_nt_strided_operands(cid, epi, monkeypatch):
    """A, W, out, C2 and resid as column slices of wider buffers (row strides multiples of 8 elements and larger than K / N; out, C2 and resid
    share one stride, as the epilogue requires): same result, same kernel, and not one element outside the slices is written.
    ops.gemm_nt takes contiguous tensors only, so this goes to the C entry."""
    for v in ("NMH_GEMM_W22", "NMH_GEMM_CFG"):
        monkeypatch.delenv(v, raising=False)
    ops = _ops()
    c = next(c for c in NT_CASES if c.id == cid)
    dt, M, N, K = c.dtype, c.M, c.N, c.K
    r = _nt_reference(cid)
    Av, Ab = _slice_of(r["A"], dt, 8, 16)
    Wv, Wb = _slice_of(r["W"], dt, 16, 8)
    lda, ldw, ldc = Av.stride(0), Wv.stride(0), 8 + N + 24
    assert ops.gemm_nt_plan(dt, M, N, K, lda=lda, ldw=ldw)[:4] == c.kernel and lda % 8 == 0 and ldw % 8 == 0 and lda > K and ldc > N
    bufs = []

    def call(bias=None, act=0, C2=None, resid=None, rowscale=None, rows_per_scale=1, out=None, accumulate=False):
        outv, outb = _slice_of(torch.full((M, N), float("nan")) if out is None else out.cpu().float(), dt, 8, 24)
        views = {}
        for name, t in (("C2", C2), ("resid", resid)):
            if t is not None:
                views[name], bb = _slice_of(t.cpu().float(), dt, 8, 24)
                bufs.append((name, bb, 8, N))
        bufs.append(("out", outb, 8, N))
        ops.lib().call("nmh_gemm_nt", ops.dt_of(Av), Av, lda, Wv, ldw, M, N, K, outv, ldc, bias, act, views.get("C2"), views.get("resid"),
                       rowscale, rows_per_scale, int(accumulate), ops._st())
        if C2 is not None and act == 1:
            C2.copy_(views["C2"])
        if out is not None:
            out.copy_(outv)
        return outv

    _check_all(_run_epilogue(ops, epi, r, dt, call), dt, f"strided {cid}")
    for name, bb, left, cols in bufs + [("A", Ab, 8, K), ("W", Wb, 16, K)]:
        assert _untouched(bb, left, cols), f"{name}: written outside its column slice"


# ---- gemm_tn ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _tn_reference(cid, dt):
    c = next(c for c in TN_CASES if c.id == cid)
    seed = 2000 + TN_CASES.index(c)
    A = torch.zeros(c.M, c.lda)
    A[:, :c.N] = _rnd(c.M, c.N, seed=seed)
    A, B = A.to(dt), _rnd(c.M, c.K, seed=seed + 1).to(dt)
    rs = torch.tensor([0.5, 2.0, 0.0, 1.5])[: (c.M + c.rps - 1) // c.rps]
    sc = rs.repeat_interleave(c.rps)[:c.M, None]
    As = (A[:, :c.N].float() * sc).to(dt).double()       # the kernel scales in fp32 and rounds to the storage type (round to nearest even)
    Bd = B.double()
    return dict(A=A, B=B, rs=rs, dW=As.T @ Bd, S=As.abs().T @ Bd.abs(), db=As.sum(0), Sb=As.abs().sum(0))


@pytest.mark.parametrize("omode", [0, 2])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("cid", [c.id for c in TN_CASES])
def test_gemm_tn_by_plan(cid, dt, omode):
    """both tiles x {one split, workspace partials, fp32 atomics}: a row scale whose sample boundary falls inside a split, ragged N under a padded
    row, fused dbias, dW and dbias pre-filled; omode 0 (dW[n][k]) and 2 (the transpose conv's [K][Cout][k3] with n = tap * Cout + co)"""
    ops = _ops()
    c = next(c for c in TN_CASES if c.id == cid)
    M, N, K = c.M, c.N, c.K
    assert ops.gemm_tn_plan(dt, M, N, K, lda=c.lda, rowscale=True, rows_per_scale=c.rps) == c.plan
    r = _tn_reference(cid, dt)
    k3 = 4
    cout = N // k3
    dW = torch.full((N, K) if omode == 0 else (K, cout, k3), 0.25, device="cuda")
    db = torch.full((N,), -0.5, device="cuda")
    ops.gemm_tn(r["A"].cuda(), r["B"].cuda(), dW, rowscale=r["rs"].cuda(), rows_per_scale=c.rps, N=N, dbias=db, omode=omode, p0=cout, p1=k3)
    got = dW if omode == 0 else dW.permute(2, 1, 0).reshape(N, K)    # [k][co][tap] -> [tap * Cout + co][k]
    ref, refb = 0.25 + r["dW"], -0.5 + r["db"]
    assert_close(got, ref.float(), TOL[dt], f"gemm_tn {cid} omode {omode}")
    assert_close(db, refb.float(), TOL[dt], f"gemm_tn {cid} dbias")
    u22 = 2.0 ** -22
    _bound_check(got, ref, (M + 8) * u22 * r["S"] + u22 * (ref.abs() + 0.25), f"gemm_tn {cid} omode {omode}")
    _bound_check(db, refb, (M + 8) * u22 * r["Sb"] + u22 * (refb.abs() + 0.5), f"gemm_tn {cid} dbias")
