"""One table of GEMM cases shared by tests/test_gemm_plan_cpu.py (does every case reach the kernel it names?) and
tests/test_gemm_paths_gpu.py (is that kernel right against float64?).

A gemm_nt plan is what ops.gemm_nt_plan returns: (family, MT, NT, ring stages, contraction splits, narrow); its first four fields name the
kernel -- `ops.gemm_nt_plan_table()` lists every such kernel the launcher holds.  A gemm_tn plan is (NTW, KTW, ring stages, rows per split,
splits, partials).

Shapes: the smallest that satisfy the path's predicate in csrc/gemm_plan.hpp, then perturbed so that M is no multiple of the row tile,
K % 64 == 8 (K = 104 for the two-k-tile kernel: the last 32-deep k-step is live in one lane group of four) and N is no multiple of the
column tile wherever the predicate leaves that free; M * N * K <= 4e9."""
from collections import namedtuple

import torch

BF, F32 = torch.bfloat16, torch.float32

NtCase = namedtuple("NtCase", "id dtype M N K kernel narrow")   # kernel = (family, MT, NT, stages)

NT_CASES = [
    # ---- bf16 ----------------------------------------------------------------------------------------------------------------------
    # 2 x 2-wave kernel: M in [2048, 16384], K >= 384, N % 96 == 0 (64 x 96 tile, ring of 3) / N % 128 == 0 (64 x 128, ring of 2): N cannot be
    # ragged; M = 2050 leaves 2 rows in the last tile.  M >= 32768, N == 192, K >= 576: 128 x 128 tile, the second column tile half empty
    NtCase("w22_233", BF, 2050, 192, 392, ("w22", 2, 3, 3), 0),
    NtCase("w22_242", BF, 2050, 128, 392, ("w22", 2, 4, 2), 0),
    NtCase("w22_442", BF, 32770, 192, 584, ("w22", 4, 4, 2), 0),
    # two-k-tile kernel: K <= 128, M >= 16384; N = 120 / 88 / 56 -> 8 / 6 / 4 column fragments, the last one half empty
    NtCase("k128_8", BF, 16390, 120, 104, ("k128", 1, 8, 0), 0),
    NtCase("k128_6", BF, 16390, 88, 104, ("k128", 1, 6, 0), 0),
    NtCase("k128_4", BF, 16390, 56, 104, ("k128", 1, 4, 0), 0),
    NtCase("k128_8_full_k", BF, 16390, 128, 128, ("k128", 1, 8, 0), 0),
    # LDS-DMA ring of 4 (M <= 8192, K >= 384 with <= 640 workgroups, or K >= 1024); K = 392 / 520: 7 / 9 k-tiles, so the ring wraps, the last
    # tile one 8-element chunk deep.  Narrow tiles: at most 192 workgroups of 96 columns
    NtCase("dma_1x2_narrow", BF, 200, 56, 392, ("dma", 1, 2, 4), 1),
    NtCase("dma_1x3_narrow", BF, 200, 136, 392, ("dma", 1, 3, 4), 1),
    NtCase("dma_1x4_narrow", BF, 1700, 504, 520, ("dma", 1, 4, 4), 1),
    NtCase("dma_1x4", BF, 200, 72, 392, ("dma", 1, 4, 4), 0),
    NtCase("dma_1x3", BF, 8190, 136, 392, ("dma", 1, 3, 4), 0),
    NtCase("dma_1x6", BF, 2000, 664, 1032, ("dma", 1, 6, 4), 0),
    # register-prefetch kernel
    NtCase("reg_1x2_narrow", BF, 8264, 56, 392, ("reg", 1, 2, 0), 1),    # narrow tile on M > 8192: no DMA ring
    NtCase("reg_1x3", BF, 200, 136, 72, ("reg", 1, 3, 0), 0),
    NtCase("reg_1x4", BF, 200, 56, 72, ("reg", 1, 4, 0), 0),
    NtCase("reg_1x4_odd_t16", BF, 200, 80, 72, ("reg", 1, 4, 0), 0),      # five 16-column fragments: the rule's last resort
    NtCase("reg_1x6", BF, 200, 88, 72, ("reg", 1, 6, 0), 0),
    NtCase("reg_2x6", BF, 8264, 88, 1032, ("reg", 2, 6, 0), 0),
    NtCase("reg_2x8", BF, 8264, 72, 1032, ("reg", 2, 8, 0), 0),
    NtCase("reg_4x3", BF, 300, 40, 72, ("reg", 4, 3, 0), 0),
    NtCase("reg_4x4", BF, 8264, 56, 1032, ("reg", 4, 4, 0), 0),
    # ---- fp32: the register-prefetch kernel only (32-deep k-tiles) ---------------------------------------------------------------------
    NtCase("f32_reg_1x3", F32, 200, 136, 72, ("reg", 1, 3, 0), 0),
    NtCase("f32_reg_1x4", F32, 200, 56, 72, ("reg", 1, 4, 0), 0),
    NtCase("f32_reg_1x6", F32, 200, 88, 72, ("reg", 1, 6, 0), 0),
    NtCase("f32_reg_1x8", F32, 100040, 120, 72, ("reg", 1, 8, 0), 0),    # K <= 128 and >= 100000 rows
    NtCase("f32_reg_2x6", F32, 8264, 88, 1032, ("reg", 2, 6, 0), 0),
    NtCase("f32_reg_2x8", F32, 8264, 72, 1032, ("reg", 2, 8, 0), 0),
    NtCase("f32_reg_4x3", F32, 300, 40, 72, ("reg", 4, 3, 0), 0),
    NtCase("f32_reg_4x4", F32, 8264, 56, 1032, ("reg", 4, 4, 0), 0),
]

# Kernels in the launcher's switch that no default dispatch of plain row-major operands returns, each with the predicate that shadows it
# (dtype, family, MT, NT, stages) -> reason
NT_SHADOWED = {
    (BF, "reg", 1, 8, 0): "the <1,8> rule needs K <= 128 and M >= 100000; the two-k-tile kernel <8> takes K <= 128, M >= 16384 first (strides are multiples of 8 at the entry)",
    (BF, "dma", 1, 8, 4): "the <1,8> rule needs K <= 128; the DMA ring needs K >= 384",
}
# Kernels reached only through a tuning variable
NT_ENV_ONLY = {
    **{(BF, "w22", mt, nt, st): "NMH_GEMM_W22" for mt, nt, st in
       [(4, 4, 3), (4, 3, 2), (4, 3, 3), (2, 4, 3), (2, 4, 4), (2, 3, 4), (2, 2, 4), (4, 2, 3), (4, 2, 4)]},
    **{(BF, "dma", 1, nt, 3): "NMH_GEMM_DMA=3" for nt in (2, 3, 4, 6, 8)},
    **{(dt, "reg", 4, nt, 0): "NMH_GEMM_CFG" for dt in (BF, F32) for nt in (6, 8)},
    (F32, "reg", 1, 2, 0): "NMH_GEMM_CFG (the narrow-tile rule is bf16 only)",
}

TnCase = namedtuple("TnCase", "id M N K lda rps plan")   # plan = (NTW, KTW, stages, rows per split, splits, partials)

# N ragged with A rows padded to lda; rps puts a sample boundary inside a split (rows per split = 1024)
TN_CASES = [
    TnCase("t64x96_one_split", 777, 36, 104, 40, 300, (2, 3, 0, 1024, 1, 0)),
    TnCase("t64x96_partials", 3000, 36, 104, 40, 1100, (2, 3, 0, 1024, 3, 1)),
    TnCase("t64x96_atomics", 20000, 36, 96, 40, 7000, (2, 3, 0, 1024, 20, 0)),
    TnCase("t96x96_one_split", 777, 100, 104, 104, 300, (3, 3, 0, 1024, 1, 0)),
    TnCase("t96x96_partials", 5000, 100, 200, 104, 1700, (3, 3, 0, 1024, 5, 1)),
    TnCase("t96x96_atomics", 20000, 100, 96, 104, 7000, (3, 3, 0, 1024, 20, 0)),
]
