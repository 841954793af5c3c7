// Which kernel a gemm_nt / gemm_tn launch takes, decided once as a small named plan (pure host code: no launch, no device call, no
// HIP type).  gemm.hip's launchers switch on these plans and the C-ABI queries nmh_gemm_nt_plan / nmh_gemm_tn_plan return them, so a
// test can name the kernel a shape reaches; the thresholds live here and nowhere else.
#pragma once
#include <cstdlib>

static inline bool lda_ok(long lda, long ldb) { return lda % 8 == 0 && ldb % 8 == 0; }

// ---- gemm_nt -----------------------------------------------------------------------------------------------------------------------
enum NtFamily {
  NT_REG = 0,    // gemm_nt_kernel<T, MT, NT, AL>: register prefetch, (64 MT) x (16 NT) tile
  NT_DMA = 1,    // gemm_nt_dma_kernel<MT, NT, ST>: LDS-DMA ring of ST stages, same tile
  NT_K128 = 2,   // gemm_nt_k128_kernel<NT>: K <= 128, 64 x (16 NT) tile
  NT_W22 = 3,    // gemm_nt_w22_kernel<MT, NT, ST>: 2 x 2 waves, (32 MT) x (32 NT) tile, ring of ST stages
};
struct NtPlan {
  int family, mt, nt, stages;
  int ksplit;   // contraction splits (grid.z factor) of the register-prefetch kernel; 1 elsewhere
  int narrow;   // 1: the tile was picked by the narrow-tile rule (few workgroups, long contraction)
  int w22cfg;   // NT_W22: MT * 100 + NT * 10 + ST as written (a forced value the library does not compile fails in the launcher)
};
struct NtShape {
  bool direct_bf16;   // A is plain row-major bf16 (ADirect<bf16_t>): the only operand the DMA, k128 and w22 kernels take
  long lda, ldb;
  int M, N, K, batch;
  int win_on, up_k, ksplit;   // the EpiParams fields the decision reads
};

// the tiles / configurations the launcher's switch holds (the kernels the library compiles); X-macros so that the switch, the plan
// table of nmh_gemm_nt_plan_table and the compiled set cannot drift apart
#define NMH_NT_REG_TILES(X) X(1, 2) X(1, 3) X(1, 4) X(1, 6) X(1, 8) X(2, 6) X(2, 8) X(4, 3) X(4, 4) X(4, 6) X(4, 8)
#define NMH_NT_DMA_TILES(X) X(2) X(3) X(4) X(6) X(8)   // MT = 1; ring of 3 and of 4
#define NMH_NT_K128_TILES(X) X(8) X(6) X(4)
#define NMH_NT_W22_CFGS(X) X(4, 4, 2) X(4, 4, 3) X(4, 3, 2) X(4, 3, 3) X(2, 4, 2) X(2, 4, 3) X(2, 4, 4) X(2, 3, 3) X(2, 3, 4) X(2, 2, 4) X(4, 2, 3) X(4, 2, 4)

// which launches take the 2 x 2-wave kernel, and with which tile (0: none).  NMH_GEMM_W22=<cfg> forces one tile everywhere it applies (tools/bench_nt_w22.py),
// NMH_GEMM_W22=0 disables.
static inline int w22_config(int M, int N, int K, int win_on) {
  const char* e = getenv("NMH_GEMM_W22");   // (read per dispatch: the tile sweep changes it inside one process)
  const int forced = e ? atoi(e) : -1;
  if (forced >= 0) return (K >= 64 && N >= 64) ? forced : 0;
  // measured (tools/bench_nt_w22.py, graph replay, 8 grids; default dispatch -> this kernel): stage-2 Linears on 8000 rows 384 x 1536: 21.4 -> 17.3 us,
  // 384 x 1152: 17.1 -> 14.2, 384 x 384: 10.0 -> 9.2 (64 x 96 tiles, ring of 3: 60 KB), 1536 x 384 + GELU' epilogue: 31.1 -> 24.9 (64 x 128, ring of 2: 48 KB);
  // stage-1 Linears on 64000 rows 192 x 768: 49.7 -> 40.4, 192 x 576: 37.8 -> 34.0 (128 x 128, ring of 2).  4000 rows: 15.0 -> 13.9; 1000 rows lose (8.1 -> 12).
  if (win_on) return 0;
  if (M >= 2048 && M <= 16384 && K >= 384) {
    if (N % 96 == 0 && N <= 768) return 233;
    if (N % 128 == 0) return 242;
  }
  if (M >= 32768 && N == 192 && K >= 576) return 442;
  return 0;
}

// (64 MT) x (16 NT) tile: the LDS-DMA ring or the register-prefetch kernel.
// The pipelined kernel pays off where few workgroups exist to hide a global-load latency per k-tile (measured, M <= 8192:
// fc2 4000x384x1536 21.9 -> 15.2 us, 500x768x3072 34.6 -> 24.5 us; with K = 384 the 4-deep ring holds most of the contraction at once:
// whole step at 1 grid/GPU 13.75 -> 13.35 ms with the threshold lowered from K >= 1024 to K >= 384); with >= 1000 workgroups the
// register-prefetch kernel's smaller LDS footprint (more co-resident workgroups) wins.  NMH_GEMM_DMA=0 disables, =3/4 forces it.
static inline NtPlan nt_tile_plan(const NtShape& s, int mt, int nt, int narrow) {
  NtPlan p{NT_REG, mt, nt, 0, s.ksplit > 1 ? s.ksplit : 1, narrow, 0};
  if (s.direct_bf16 && mt == 1) {
    static const int dma_st = [] { const char* e = getenv("NMH_GEMM_DMA"); return e ? atoi(e) : -1; }();
    if (dma_st == 0 || !lda_ok(s.lda, s.ldb)) return p;
    static const int min_k = [] { const char* e = getenv("NMH_GEMM_DMA_MINK"); return e ? atoi(e) : 384; }();
    static const long max_m = [] { const char* e = getenv("NMH_GEMM_DMA_MAXM"); return e ? atol(e) : 8192L; }();
    // (K < 1024: only while the launch has <= 640 workgroups -- 4000x1536x384 = 1008 workgroups measured 17.2 us with the register-prefetch kernel against 20.9, 8000x1536x384 = 2000 workgroups 37 us with the register-prefetch
    //  kernel, 50 us with this one)
    const long wgs = ((long)s.M + 64 * mt - 1) / (64 * mt) * ((s.N + 16 * nt - 1) / (16 * nt)) * s.batch;
    const bool auto_on = dma_st < 0 && (long)s.M * s.batch <= max_m && (s.K >= 1024 || (s.K >= min_k && wgs <= 640));
    if (dma_st == 3) { p.family = NT_DMA; p.stages = 3; p.ksplit = 1; }
    else if (dma_st == 4 || auto_on) { p.family = NT_DMA; p.stages = 4; p.ksplit = 1; }
  }
  return p;
}

// 0 and *out filled, or -2 (shape constraint)
static inline int nt_plan(const NtShape& s, NtPlan* out) {
  const int M = s.M, N = s.N, K = s.K, batch = s.batch;
  if (N % 8 != 0 || K % 8 != 0) return -2;
  const int t16 = (N + 15) / 16;
  if (s.direct_bf16) {
    if (batch == 1 && s.ksplit <= 1 && !s.up_k && lda_ok(s.lda, s.ldb)) {
      const int cfg = w22_config(M, N, K, s.win_on);
      if (cfg > 0) { *out = NtPlan{NT_W22, cfg / 100, cfg / 10 % 10, cfg % 10, 1, 0, cfg}; return 0; }
    }
  }
  if (const char* ov = getenv("NMH_GEMM_CFG")) {  // tuning override "MT,NT"
    int mt = ov[0] - '0', nt = atoi(ov + 2);
    if ((mt == 1 && (nt == 2 || nt == 3 || nt == 4 || nt == 6 || nt == 8)) || ((mt == 2 || mt == 4) && (nt == 6 || nt == 8))) { *out = nt_tile_plan(s, mt, nt, 0); return 0; }
  }
  // 64-row tiles (32-45 KB of LDS -> 3-5 workgroups per CU) for (a) small problems (stage 2/3 tokens, 10^3..20^3 decoder volumes), so
  // that more than a few dozen CUs get work, and (b) short contractions (every Linear of the encoder, the transpose convs): those
  // are HBM-bound with a latency-bound prologue/epilogue per workgroup, and co-resident workgroups are what hides it
  // (measured on 256000x288x96: 145 us with 256x128 tiles, 67 us with 64x96)
  if (((long)M * batch <= 8192 || K <= 1024) && t16 >= 4) {
    // wide outputs of the 40^3-token Linears (fc1 / fc2-dgrad: N = 384, K = 96, >= 256 k rows) are write-bound: 128-column tiles store
    // 256-byte-aligned row segments (96-column tiles split every second 128-byte line between two workgroups): 393 -> 312 us at 512 k rows
    if (s.direct_bf16) {
      static const int k128_on = getenv("NMH_GEMM_K128") ? atoi(getenv("NMH_GEMM_K128")) : 1;
      static const long k128_min = getenv("NMH_GEMM_K128_MINM") ? atol(getenv("NMH_GEMM_K128_MINM")) : 16384;
      if (k128_on && batch == 1 && s.ksplit <= 1 && K <= 128 && M >= k128_min && lda_ok(s.lda, s.ldb)) {
        static const long nt8_min = getenv("NMH_GEMM_K128_NT8_MINM") ? atol(getenv("NMH_GEMM_K128_NT8_MINM")) : 16384;   // (1 grid: 64000 rows -- 12.48 -> 12.43 ms with 128-column tiles there too)
        int nt = 0;
        if (t16 % 8 == 0 && (long)M >= nt8_min) nt = 8;
        else if (t16 % 6 == 0) nt = 6;
        else if (t16 % 4 == 0) nt = 4;
        if (nt) { *out = NtPlan{NT_K128, 1, nt, 0, 1, 0, 0}; return 0; }
      }
    }
    // launches of a few dozen workgroups with a long contraction (stage 3 / 4 Linears at 1-2 grids per GPU): one workgroup per CU is
    // bound by its own LDS fragment reads (a wave reads the whole B tile: 56 KB per 64-deep k-tile with 96 columns, 24 KB with 32), so the
    // narrowest tile that still gives at most 1.5 workgroups per CU wins (measured, graph replay: 1000x384x1536 13.3 -> 8.0 us,
    // 125x768x3072 22.7 -> 12.9, 512x768x1536 13.3 -> 8.0, 216x768x768 8.1 -> 5.0; 4000x384x1536 stays at 96 columns: 15.1 vs 17.9 / 23.7)
    if (s.direct_bf16) {
      static const int narrow_on = getenv("NMH_GEMM_NARROW") ? atoi(getenv("NMH_GEMM_NARROW")) : 1;
      if (narrow_on && K >= 384 && s.ksplit <= 1 && lda_ok(s.lda, s.ldb)) {   // (aligned rows: these launches take the LDS-DMA kernel)
        const long rt = ((long)M + 63) / 64 * batch;
        auto fits = [&](int nt) { return t16 % nt == 0 && rt * (t16 / nt) <= 384; };
        if (rt * ((t16 + 5) / 6) <= 192) {   // (252 workgroups of 96 columns -- 4000x384x1536 -- are already one per CU)
          for (int nt = 2; nt <= 4; ++nt)
            if (fits(nt)) { *out = nt_tile_plan(s, 1, nt, 1); return 0; }
        }
      }
    }
    int nt = 4;
    if (t16 % 8 == 0 && K <= 128 && (long)M * batch >= 100000) nt = 8;
    else if (t16 % 6 == 0) nt = 6;
    else if (t16 % 4 == 0) nt = 4;
    else if (t16 % 3 == 0) nt = 3;
    *out = nt_tile_plan(s, 1, nt, 0);
    return 0;
  }
  if (t16 <= 3) { *out = nt_tile_plan(s, 4, 3, 0); return 0; }
  if (t16 == 4) { *out = nt_tile_plan(s, 4, 4, 0); return 0; }
  // long contractions on big M (implicit-GEMM convs at 20^3..40^3, transpose-conv dgrad): 128-row tiles (2 workgroups per CU)
  // measured 10-30 % faster than 256-row tiles (1 per CU) on every decoder shape
  *out = nt_tile_plan(s, 2, t16 % 6 == 0 ? 6 : 8, 0);
  return 0;
}

// ---- gemm_tn -----------------------------------------------------------------------------------------------------------------------
struct TnPlan {
  int ntw, ktw;   // (32 ntw) x (32 ktw) output tile: 2,3 = 64 x 96 (N <= 48, N padded); 3,3 = 96 x 96
  int stages;     // 0: gemm_tn_kernel; 2..4: gemm_tn_dma_kernel with a ring of that many stages
  long mps;       // contraction rows per split
  int splits;     // grid.z
  int part;       // 1: the splits store partial tiles to the workspace and a reduce launch sums them; 0: they add into the output
  //                 (fp32 atomics when splits > 1)
};
struct TnShape {
  bool bf16, conv;   // conv: the B operand is the conv-tap gather (BConv3TN), whose DMA ring is on by default
  long lda, M;
  int N, K;
  bool has_rs; int rps;
  bool has_ws; long ws_floats;
};
// many splits of a small output (the 256000-row stage-0 gradients: 125-250 splits) would write more partial bytes than the operands
// hold; those keep the atomics
static inline int tn_ws_max_splits() { static const int v = getenv("NMH_TN_WS_SPLITS") ? atoi(getenv("NMH_TN_WS_SPLITS")) : 16; return v; }

static inline int tn_plan(const TnShape& s, TnPlan* out) {
  const long Mtot = s.M;
  const int N = s.N, K = s.K;
  if (K % 8 != 0 || s.lda % 8 != 0) return -2;  // N may be ragged: A rows are padded to lda, output guarded by n < N
  TnPlan p{};
  p.ntw = N <= 48 ? 2 : 3;   // 64 x 96 tile (N padded) : 96 x 96 tile
  p.ktw = 3;
  const int BNW = 32 * p.ntw, BKW = 32 * p.ktw;
  const int gx = (N + BNW - 1) / BNW, gy = (K + BKW - 1) / BKW;
  // the load->LDS->MFMA chain of one workgroup is not software-pipelined: latency is hidden by co-resident workgroups, so a
  // long contraction (conv wgrad over 4M voxels) wants ~4 workgroups per CU; short ones are bounded by the atomics instead
  long want = (Mtot >= (1L << 20) ? 1024 : 512) / ((long)gx * gy);  // aim for ~512 workgroups; many output tiles => no split (and no atomics)
  if (want < 1) want = 1;
  long mps = (Mtot + want - 1) / want;
  mps = (mps + 63) / 64 * 64;
  long mps_min = 1024;                 // every split ends in BNW*BKW atomics: give it >= 16 chunks of MFMA work first
  if (const char* e = getenv("NMH_TN_MPS")) mps_min = atol(e);
  if (const char* e = getenv("NMH_TN_WANT")) { want = atol(e) / ((long)gx * gy); if (want < 1) want = 1; mps = ((Mtot + want - 1) / want + 63) / 64 * 64; }
  if (mps < mps_min) mps = mps_min;
  if (s.bf16 && p.ntw == 3) {
    // measured: 8-12 % on the implicit-GEMM conv weight gradients (their gather loader is the longer dependency chain), within
    // noise on the plain ones (which are bound by L2 -> LDS bandwidth of the 96x96 tiles, not by latency): default on for convs only
    static const int dma_direct = [] { const char* e = getenv("NMH_TN_DMA"); return e ? atoi(e) : 0; }();
    static const int dma_conv = [] { const char* e = getenv("NMH_TN_DMA"); return e ? atoi(e) : 3; }();
    const int dma_st = s.conv ? dma_conv : dma_direct;
    if (dma_st && s.lda % 8 == 0) {
      if (s.has_rs) {   // row scales are applied per split: every split must lie inside one sample
        long j = (s.rps + mps - 1) / mps;
        while (j > 1 && s.rps % j) --j;
        mps = s.rps / j;
      }
      p.stages = (dma_st == 2 || dma_st == 4) ? dma_st : 3;
    }
  }
  p.mps = mps;
  p.splits = (int)((Mtot + mps - 1) / mps);
  p.part = (s.has_ws && p.splits > 1 && p.splits <= tn_ws_max_splits() && (long)p.splits * N * (K + 1) <= s.ws_floats) ? 1 : 0;
  *out = p;
  return 0;
}
