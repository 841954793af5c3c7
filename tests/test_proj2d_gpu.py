"""The 2-D projection term on rows of boxes on the GPU (nerf_mae_amd.proj2d over csrc/proj2d.hip) against the float64 restatement tests/_proj2d_ref.py (itself
checked against the recorded reference, tests/golden/g30_proj2d.npz, in tests/test_proj2d_ref_cpu.py).

Rows: tests/_proj2d_ref.make_rows, n = 67 (22 far, 22 near, 22 mixed, 1 exact) and n = 1, 6 and 7 columns, cameras of res 32 and 160.  Every group is compared
as a tensor of its own: assert_close's absolute term is a fraction of the tensor's rms, and far rows (terms of 1 .. 100) would hide near rows (terms of 1e-3).

Tolerances.  Far and mixed rows: the project's contract for fp32, assert_close(rtol=1e-3).  Near rows: fp32 arithmetic that subtracts two pixel coordinates, as
the reference's does, cannot meet 1e-3 there: a term is 0.5 d^2 / beta with d, about 0.01 .. 0.05 px, the difference of two coordinates of 1e2 .. 1e3 px that each
carry about 1e-4 px of rounding; and with 7 columns the two corners are themselves rounded to fp32 before anything is subtracted.  So the bound is not fixed in
advance but comes from the reference itself: g30 holds, on exactly these rows, the reference's result as it runs (fp32) and with float64 inputs, and the bound is
|got - float64| <= 4 max |reference fp32 - float64| elementwise, for the terms and for the gradients (4: the kernel fuses K [R|t] into one matrix and may
contract, another rounding path of the same size).  The reference's own maxima (tools/gen_golden_proj2d.py prints them) are REF_NEAR below; the kernel's
measured errors are in DESIGN.md 3.22."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _proj2d_ref as J  # noqa: E402
from tests._metrics import assert_close  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [(ncols, res, n) for ncols in (6, 7) for res in (32, 160) for n in (J.N_ROWS, 1)]
# (ncols, res) -> max |reference fp32 - reference float64| over the near rows of g30: (terms, gradients); the test reads the arrays, these are for the reader
REF_NEAR = {(6, 32): (9.6e-6, 1.1e-2), (6, 160): (7.6e-6, 1.8e-3), (7, 32): (1.7e-5, 8.1e-2), (7, 160): (1.3e-5, 1.1e-1)}
# the kernel's max |got - float64| on the same rows, measured on an MI355X (NMH_PRINT_ERR=1): with 6 columns the difference is formed from p - t and is exact
# to rounding; with 7 columns the fp32 rounding of the two corners remains
KERNEL_NEAR = {(6, 32): (4.8e-10, 5.4e-7), (6, 160): (6.7e-10, 2.1e-7), (7, 32): (9.2e-6, 5.7e-2), (7, 160): (5.9e-6, 5.1e-2)}


def _m():
    from nerf_mae_amd import proj2d
    return proj2d


@functools.lru_cache(maxsize=None)
def g30():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g30_proj2d.npz")))


@functools.lru_cache(maxsize=None)
def ref(ncols, res, n):
    """rows, groups, float64 terms and gradients (upstream 1)"""
    pred, target, where = J.make_rows(ncols, res, n)
    T, G = J.reference_grad(pred, target, res)
    return pred, target, where, T, G


def _run(pred, target, res, upstream=None):
    p = pred.cuda().requires_grad_(True)
    T = _m().proj2d_terms(p, target.cuda(), res)
    (T.sum() if upstream is None else (T * upstream.cuda()).sum()).backward()
    return T.detach().cpu(), p.grad.cpu()


@pytest.mark.parametrize("ncols,res,n", CASES)
def test_terms_and_gradients_against_float64_per_group(ncols, res, n):
    pred, target, where, T64, G64 = ref(ncols, res, n)
    T, G = _run(pred, target, res)
    assert T.dtype == torch.float32 and tuple(T.shape) == (n,) and tuple(G.shape) == (n, ncols)
    tag = f"{ncols} columns, res {res}, n {n}"
    for group in ("far", "mixed"):
        k = where[group]
        if k:
            assert_close(T[k], T64[k], 1e-3, f"{tag}: {group} terms")
            assert_close(G[k], G64[k], 1e-3, f"{tag}: {group} gradients")
    if where["near"]:
        k, g = where["near"], g30()
        name = f"r{ncols}_{res}_{n}"
        r32, r64 = torch.from_numpy(g[name + "_t32"])[k].double(), torch.from_numpy(g[name + "_t64"])[k]
        g32, g64 = torch.from_numpy(g[name + "_g32"])[k].double(), torch.from_numpy(g[name + "_g64"])[k]
        bound_t, bound_g = 4 * float((r32 - r64).abs().max()), 4 * float((g32 - g64).abs().max())
        err_t, err_g = float((T[k].double() - T64[k]).abs().max()), float((G[k].double() - G64[k]).abs().max())
        if os.environ.get("NMH_PRINT_ERR"):
            print(f"  [{tag}: near] terms {err_t:.2e} (bound {bound_t:.2e}, largest term {float(T64[k].max()):.2e}); gradients {err_g:.2e} (bound {bound_g:.2e}, "
                  f"largest {float(G64[k].abs().max()):.2e})")
        assert (T[k] > 0).all() and err_t <= bound_t, (tag, err_t, bound_t)
        assert err_g <= bound_g, (tag, err_g, bound_g)
    for k in where["exact"]:
        assert T[k].item() == 0 and (G[k] == 0).all(), "prediction == target: term 0, gradient exactly 0"


def test_two_runs_are_bit_identical_and_the_upstream_gradient_scales_linearly():
    pred, target, where, _, _ = ref(7, 32, J.N_ROWS)
    a, b = _run(pred, target, 32), _run(pred, target, 32)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    up = torch.from_numpy(np.random.default_rng(5).choice([0.0, -2.0, 0.25, 8.0], pred.shape[0]).astype(np.float32))       # powers of two: exact scaling
    c = _run(pred, target, 32, up)
    assert torch.equal(c[0], a[0]) and torch.equal(c[1], a[1] * up[:, None])
    # a general upstream gradient, against float64
    w = torch.from_numpy(np.random.default_rng(6).standard_normal(pred.shape[0]).astype(np.float32))
    k = where["far"]
    assert_close(_run(pred, target, 32, w)[1][k], J.reference_grad(pred, target, 32, w)[1][k], 1e-3, "weighted far gradients")


def test_target_gets_no_gradient_and_points_match():
    M = _m()
    pred, target, _, _, _ = ref(7, 160, J.N_ROWS)
    t = target.cuda().requires_grad_(True)
    p = pred.cuda().requires_grad_(True)
    M.proj2d_terms(p, t, 160).sum().backward()
    assert t.grad is None and p.grad is not None
    for rows in (pred, ref(6, 160, J.N_ROWS)[0]):
        assert_close(M.proj2d_points(rows.cuda()).cpu(), J.points(rows.double()), 1e-5, "points")
    assert M.proj2d_terms(pred[:0].cuda(), target[:0].cuda(), 160).shape == (0,)


def test_argument_errors():
    M = _m()
    from nerf_mae_amd._lib import lib
    pred, target, _, _, _ = ref(6, 32, J.N_ROWS)
    p, t = pred.cuda(), target.cuda()
    with pytest.raises(TypeError):
        M.proj2d_terms(p.double(), t.double(), 32)
    with pytest.raises(RuntimeError):
        M.proj2d_terms(pred, target, 32)
    with pytest.raises(ValueError):
        M.proj2d_terms(p[:, :5].contiguous(), t[:, :5].contiguous(), 32)
    with pytest.raises(ValueError):
        M.proj2d_terms(p, ref(7, 32, J.N_ROWS)[1].cuda(), 32)
    with pytest.raises(ValueError):
        M.proj2d_cameras(0)
    cams = (ctypes.c_float * 48)(*M.proj2d_cameras(32).reshape(-1).tolist())
    out, n = torch.empty(p.shape[0], device="cuda"), p.shape[0]
    cdll, vp = lib().cdll, ctypes.c_void_p
    ok = (vp(p.data_ptr()), vp(t.data_ptr()), n, 6, ctypes.cast(cams, vp), vp(out.data_ptr()), None)
    assert cdll.nmh_proj2d_fwd(*ok) == 0
    torch.cuda.synchronize()
    for at, bad in ((3, 5), (3, 8), (2, -1), (0, None), (1, None), (4, None), (5, None)):
        args = list(ok)
        args[at] = bad
        assert cdll.nmh_proj2d_fwd(*args) == -4, (at, bad)
    d = torch.empty_like(p)
    okb = (vp(p.data_ptr()), vp(t.data_ptr()), vp(out.data_ptr()), n, 6, ctypes.cast(cams, vp), vp(d.data_ptr()), None)
    assert cdll.nmh_proj2d_bwd(*okb) == 0
    torch.cuda.synchronize()
    for at, bad in ((4, 9), (0, None), (2, None), (5, None), (6, None)):
        args = list(okb)
        args[at] = bad
        assert cdll.nmh_proj2d_bwd(*args) == -4, (at, bad)
