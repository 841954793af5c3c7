"""Which kernel the two GEMM dispatches pick, asked of the library's own decision function (nmh_gemm_nt_plan / nmh_gemm_tn_plan: host
queries, no GPU).  The launch path decides through the same function (csrc/gemm_plan.hpp), so what is pinned here is what runs."""
import ctypes
import itertools

import pytest
import torch

from tests._gemm_cases import BF, F32, NT_CASES, NT_ENV_ONLY, NT_SHADOWED, TN_CASES


def _ops():
    from nerf_mae_amd import ops
    return ops


@pytest.fixture(autouse=True)
def _default_dispatch(monkeypatch):
    for v in ("NMH_GEMM_W22", "NMH_GEMM_CFG"):   # the two variables the dispatch reads on every call
        monkeypatch.delenv(v, raising=False)


@pytest.mark.parametrize("c", NT_CASES, ids=[c.id for c in NT_CASES])
def test_nt_case_reaches_its_named_kernel(c):
    p = _ops().gemm_nt_plan(c.dtype, c.M, c.N, c.K)
    assert p[:4] == c.kernel and p[5] == c.narrow and p[4] == 1, (c, p)
    assert c.M * c.N * c.K <= 4e9


@pytest.mark.parametrize("c", TN_CASES, ids=[c.id for c in TN_CASES])
@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "fp32"])
def test_tn_case_reaches_its_named_plan(dt, c):
    assert _ops().gemm_tn_plan(dt, c.M, c.N, c.K, lda=c.lda, rowscale=True, rows_per_scale=c.rps) == c.plan
    # a sample boundary inside a split, and N ragged under a padded row
    assert c.rps % c.plan[3] != 0 and c.N % 8 != 0 and c.lda % 8 == 0


def test_tn_table_covers_both_tiles_and_the_three_ways_to_sum_the_splits():
    got = {(c.plan[0], "one" if c.plan[4] == 1 else ("partials" if c.plan[5] else "atomics")) for c in TN_CASES}
    assert got == set(itertools.product((2, 3), ("one", "partials", "atomics")))
    ops = _ops()
    # without a workspace, or with one too small for splits * N * (K + 1) floats, the partial sums fall back to atomics
    c = next(c for c in TN_CASES if c.id == "t96x96_partials")
    assert ops.gemm_tn_plan(BF, c.M, c.N, c.K, lda=c.lda, ws_floats=0)[4:] == (5, 0)
    assert ops.gemm_tn_plan(BF, c.M, c.N, c.K, lda=c.lda, ws_floats=5 * c.N * (c.K + 1))[4:] == (5, 1)
    assert ops.gemm_tn_plan(BF, c.M, c.N, c.K, lda=c.lda, ws_floats=5 * c.N * (c.K + 1) - 1)[4:] == (5, 0)
    # 16 splits still take the workspace, 17 do not
    assert ops.gemm_tn_plan(BF, 16 * 1024, 96, 96)[4:] == (16, 1)
    assert ops.gemm_tn_plan(BF, 16 * 1024 + 1, 96, 96)[4:] == (17, 0)


def test_nt_table_covers_every_kernel_the_default_dispatch_can_return():
    """The launcher's switch (nmh_gemm_nt_plan_table, built from the same lists as the switch) = the case table + the kernels only a
    tuning variable reaches + the shadowed ones, each named with its reason in tests/_gemm_cases.py; nothing is left over."""
    switch = set(_ops().gemm_nt_plan_table())
    assert len(switch) == 47
    covered = {(c.dtype,) + c.kernel for c in NT_CASES}
    assert covered <= switch and set(NT_ENV_ONLY) <= switch and set(NT_SHADOWED) <= switch
    assert not covered & set(NT_ENV_ONLY) and not covered & set(NT_SHADOWED) and not set(NT_ENV_ONLY) & set(NT_SHADOWED)
    assert switch - covered - set(NT_ENV_ONLY) - set(NT_SHADOWED) == set()
    assert all(NT_SHADOWED.values()) and all(NT_ENV_ONLY.values())


def test_nt_sweep_finds_no_kernel_outside_the_case_table():
    """A grid over M, N, K around every threshold, with and without the window-scatter store: whatever the default dispatch returns there is a
    kernel the table covers -- so a kernel listed as shadowed or as reachable by a tuning variable only really is."""
    ops = _ops()
    covered = {(c.dtype,) + c.kernel for c in NT_CASES}
    Ms = [8, 64, 200, 1700, 2047, 2048, 6144, 8192, 8193, 12288, 12289, 16383, 16384, 16385, 32767, 32768, 99999, 100000, 300000]
    Ns = [8, 40, 48, 56, 64, 72, 80, 96, 120, 128, 136, 144, 192, 200, 256, 288, 384, 504, 672, 768, 864, 1536, 3072]
    Ks = [8, 72, 128, 136, 376, 384, 392, 576, 1016, 1024, 1032, 3072]
    seen = set()
    for dt, M, N, K, win in itertools.product((BF, F32), Ms, Ns, Ks, (False, True)):
        seen.add((dt,) + ops.gemm_nt_plan(dt, M, N, K, win_on=win)[:4])
    assert seen <= covered, seen - covered
    assert seen == covered, covered - seen   # and the sweep itself is wide enough to meet every covered kernel


# ---- the model's own Linear shapes ----------------------------------------------------------------------------------------------------------
# 160^3 grids, patch 4: 40^3 / 20^3 / 10^3 / 5^3 tokens per grid at widths 96 / 192 / 384 / 768 (swin_t and swin_s differ in depth
# only, so their Linear shapes are the same), 1 and 8 grids per GPU (bench.py's sweep).  Forward: qkv (3C x C), proj (C x C), fc1 (4C x C),
# fc2 (C x 4C), PatchMerging reduction (C x 4C, on the stage's tokens).  Input gradients: fc2's is fc1's shape, fc1's is fc2's, proj's is its
# own, qkv's is (C x 3C), the reduction's (4C x C).  Literals: the dispatch of the commit before the plan existed, read by hand.
TOKENS = (64000, 8000, 1000, 125)
K6, K8 = ("k128", 1, 6, 0), ("k128", 1, 8, 0)
R6 = ("reg", 1, 6, 0)
W233, W242, W442 = ("w22", 2, 3, 3), ("w22", 2, 4, 2), ("w22", 4, 4, 2)
D2, D3, D6 = ("dma", 1, 2, 4), ("dma", 1, 3, 4), ("dma", 1, 6, 4)
NT_PRODUCT = {   # (grids, stage) -> kernels of qkv, proj (= its dgrad), fc1 (= fc2 dgrad), fc2 (= fc1 dgrad), qkv dgrad, merge, merge dgrad
    (1, 0): (K6, K6, K8, R6, R6, None, None),
    (1, 1): (R6, R6, R6, W233, W233, W233, R6),
    (1, 2): (D3, D2, D6, D2, D2, D2, D6),
    (1, 3): (D2, D2, D2, D2, D2, D2, D2),
    (8, 0): (K6, K6, K8, R6, R6, None, None),
    (8, 1): (R6, R6, R6, W442, W442, W442, R6),
    (8, 2): (W242, W233, W242, W233, W233, W233, W242),
    (8, 3): (D6, D2, D6, D2, D2, D2, D6),
}
# weight gradients dW[N, K] over M tokens (nmh_gemm_tn; the row scale of proj / fc2 is the stochastic-depth factor per grid): rows per split, splits,
# partials -- all on the 96 x 96 tile without a DMA ring; qkv, proj, fc1, fc2, merge
TN_PRODUCT = {
    (1, 0): ((1024, 63, 0), (1024, 63, 0), (1024, 63, 0), (1024, 63, 0), None),
    (1, 1): ((1024, 8, 1),) * 5,
    (1, 2): ((1024, 1, 0),) * 5,
    (1, 3): ((1024, 1, 0),) * 5,
    (8, 0): ((3072, 167, 0), (1024, 500, 0), (4032, 127, 0), (4032, 127, 0), None),
    (8, 1): ((1536, 42, 0), (1024, 63, 0), (2048, 32, 0), (2048, 32, 0), (2048, 32, 0)),
    (8, 2): ((1024, 8, 1),) * 5,
    (8, 3): ((1024, 1, 0),) * 5,
}


@pytest.mark.parametrize("grids,stage", sorted(NT_PRODUCT))
def test_product_linear_shapes_keep_their_kernels(grids, stage):
    ops = _ops()
    C, T = 96 << stage, TOKENS[stage] * grids
    nt_shapes = [(3 * C, C), (C, C), (4 * C, C), (C, 4 * C), (C, 3 * C), (C, 4 * C), (4 * C, C)]
    for (N, K), want in zip(nt_shapes, NT_PRODUCT[(grids, stage)]):
        if want is not None:
            assert ops.gemm_nt_plan(BF, T, N, K)[:4] == want, (T, N, K)
    tn_shapes = [(3 * C, C, False), (C, C, True), (4 * C, C, False), (C, 4 * C, True), (C, 4 * C, False)]
    for (N, K, rs), want in zip(tn_shapes, TN_PRODUCT[(grids, stage)]):
        if want is not None:
            assert ops.gemm_tn_plan(BF, T, N, K, rowscale=rs, rows_per_scale=TOKENS[stage]) == (3, 3, 0) + want, (T, N, K)


# ---- strides ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["dma_1x6", "w22_233", "k128_6", "dma_1x2_narrow"])
def test_nt_rows_off_16_bytes_take_the_register_prefetch_kernel(cid):
    """the DMA ring, the 2 x 2-wave and the two-k-tile kernels fetch 16 aligned bytes per lane: either operand with a row stride that is no
    multiple of 8 elements moves the launch to the register-prefetch kernel; a padded stride that is one changes nothing"""
    ops = _ops()
    c = next(c for c in NT_CASES if c.id == cid)
    assert ops.gemm_nt_plan(BF, c.M, c.N, c.K, lda=c.K + 16, ldw=c.K + 24)[:4] == c.kernel
    for lda, ldw in ((c.K + 4, c.K), (c.K, c.K + 4), (c.K + 1, c.K + 1)):
        assert ops.gemm_nt_plan(BF, c.M, c.N, c.K, lda=lda, ldw=ldw)[0] == "reg", (lda, ldw)


def test_nt_entry_rejects_rows_off_16_bytes():
    """...and the launch entry itself refuses such strides (-2) before anything is launched: every access of the kernels is a 16-byte vector
    (ADirect::load, Vec8), which a row off that alignment would break.  The pointers are never followed."""
    L = _ops().lib().cdll
    p = ctypes.c_void_p(4096)
    for dt, lda, ldw, ldc in ((1, 100, 96, 96), (1, 96, 100, 96), (1, 96, 96, 100), (0, 98, 96, 96), (0, 96, 96, 98)):
        assert L.nmh_gemm_nt(dt, p, lda, p, ldw, 64, 96, 96, p, ldc, None, 0, None, None, None, 1, 0, None) == -2, (dt, lda, ldw, ldc)


def test_plan_queries_reject_what_the_gemms_reject():
    ops = _ops()
    plan = (ctypes.c_int * 6)()
    L = ops.lib().cdll
    assert L.nmh_gemm_nt_plan(1, 96, 96, 64, 100, 96, 0, 0, 1, 1, plan) == -2    # N % 8
    assert L.nmh_gemm_nt_plan(1, 100, 100, 64, 96, 100, 0, 0, 1, 1, plan) == -2  # K % 8
    assert L.nmh_gemm_nt_plan(1, 96, 96, 64, 96, 96, 0, 0, 1, 1, None) == -4
    assert L.nmh_gemm_nt_plan(2, 96, 96, 64, 96, 96, 0, 0, 1, 1, plan) == -4
    assert L.nmh_gemm_tn_plan(1, 100, 64, 96, 96, 0, 1, 0, plan) == -2           # lda % 8
    assert L.nmh_gemm_tn_plan(1, 96, 64, 96, 100, 0, 1, 0, plan) == -2           # K % 8
    assert L.nmh_gemm_tn_plan(1, 96, 64, 96, 96, 0, 1, 0, None) == -4


def test_tuning_variables_are_read_by_the_query_too(monkeypatch):
    ops = _ops()
    monkeypatch.setenv("NMH_GEMM_W22", "443")
    assert ops.gemm_nt_plan(BF, 300, 200, 136)[:4] == ("w22", 4, 4, 3)
    assert ops.gemm_nt_plan(BF, 300, 56, 136)[0] == "reg"          # forced tiles still need N >= 64 and K >= 64
    assert ops.gemm_nt_plan(F32, 300, 200, 136)[0] == "reg"
    monkeypatch.setenv("NMH_GEMM_W22", "0")
    assert ops.gemm_nt_plan(BF, 2050, 192, 392) == ("dma", 1, 2, 4, 1, 1)   # 33 row tiles x 6: the narrow-tile rule is next in line
    monkeypatch.setenv("NMH_GEMM_CFG", "4,8")
    assert ops.gemm_nt_plan(BF, 300, 200, 136)[:4] == ("reg", 4, 8, 0)
    assert ops.gemm_nt_plan(F32, 300, 200, 136)[:4] == ("reg", 4, 8, 0)


def test_gemm_nt_checks_the_shared_row_stride():
    """C2 and resid are indexed with the output's row stride in the epilogue: ops.gemm_nt refuses anything else.  The check comes before the
    device check, so CPU tensors show it (with the strides right they get as far as "need HIP device tensors")"""
    ops = _ops()
    A, W = torch.zeros(16, 8), torch.zeros(8, 8)
    out, wide = torch.zeros(16, 8), torch.zeros(16, 16)
    with pytest.raises(ValueError, match="C2 has row stride 16, out has 8"):
        ops.gemm_nt(A, W, act=1, C2=wide, out=out)
    with pytest.raises(ValueError, match="resid has row stride 16, out has 8"):
        ops.gemm_nt(A, W, resid=wide, out=out)
    with pytest.raises(ValueError, match="C2 has row stride 16, out has 8"):
        ops.gemm_nt(A, W, act=1, C2=wide)                      # out allocated by the call: its stride is N
    with pytest.raises(RuntimeError, match="HIP device tensors"):
        ops.gemm_nt(A, W, resid=torch.zeros(2, 8, 8), out=out)   # leading dimensions do not matter, the row stride does
