// Internal launcher declarations shared by the .hip translation units and the C-ABI layer (capi.hip).
#pragma once
#include <hip/hip_runtime.h>

struct FDiv { unsigned M; int sh; unsigned d; };
FDiv make_fdiv(unsigned d);

// window partition geometry (3-D shifted windows, window edge 4): real dims, padded dims, effective shifts
struct WinMap { int B, H, W, D, PH, PW, PD, s0, s1, s2; };

// GEMM epilogue description (all optional, evaluated in this order):
//   v = acc (+ bias[col]);  act==1: C2 = v, v = gelu(v);  act==2: v *= gelu'(C2);  v *= rowscale[row/rows_per_scale];
//   v += resid;  accumulate: v += C;  C = v.         C, C2, resid share leading dimension ldc.
struct EpiParams {
  void* C; long ldc;
  const float* bias;
  int act; void* C2;
  const void* resid;
  const float* rowscale; int rows_per_scale;
  int accumulate;
  // ConvTranspose3d(kernel = stride = up_k) pixel shuffle folded into the store (up_k > 0): GEMM row m = coarse voxel (b,z,y,x) of a
  // up_v^3 grid, column = tap*up_cout + co  ->  C[fine voxel (b, z*k+tz, y*k+ty, x*k+tx)][co], row stride ldc; bias indexed by co
  int up_k, up_v, up_cout;
  FDiv up_dv, up_dk, up_dc;
  // window reverse folded into the store (win_on): GEMM row = window-ordered row -> token row (pad rows dropped); bias, rowscale
  // (indexed by token / rows_per_scale) and resid (token order) as usual: x1[tok] = x[tok] + s_b * (o . Wproj^T + b)
  int win_on; WinMap wm;
  // split contraction (implicit-GEMM convs on small volumes: too few output tiles to fill the chip, K = 27*Cin long): grid.z = batch * ksplit,
  // every split stores its fp32 accumulators to kpart[split][batch*M][N]; a second launch sums them and applies `accumulate` (no other epilogue)
  int ksplit; int nbatch; float* kpart;
};

// geometry for gemm_tn gather / output remap
struct TnGeom {
  int omode;            // 0: Out[n*ldo+k]; 1: conv3 weight [Cout][Cin][27]; 2: convT weight [Cin][Cout][k3]
  long ldo;
  int Cin, D, H, W; unsigned V;
  FDiv dC, dW, dH, dV;
  float* dbias;         // optional: dbias[n] += sum_m A[m][n]*rs(m) (column sums of the A operand, e.g. a Linear's bias gradient)
  // up_k > 0: the A operand is the pixel-shuffled view of a fine-grid tensor (ConvTranspose3d k = stride backward):
  // A[m][n = tap*Cout + co] = X[fine voxel (m, tap)][co], X row stride up_ldc, Cout = Cin field; dbias is then indexed by co
  int up_k, up_v; long up_ldc; FDiv up_dv, up_dk;
  // split-contraction partials: with a workspace the M splits store plain fp32 partial tiles [split][N][K] (+ [split][N] bias sums)
  // and a second kernel sums them into Out -- instead of gz fp32 global atomics per output element (measured: the atomics are
  // most of the time of the small-M weight gradients)
  float* ws; long ws_floats; float* part;
};


#ifdef __HIPCC__
// window order <-> token order of the 4x4x4 shifted-window partition (pad -> roll(-shift) -> partition; swin_mae3d.py:62-101)
// (32-bit unsigned arithmetic: every row / token count of this path is < 2^31, and a 64-bit div/mod costs ~150 VALU instructions on
//  gfx950 against ~30 for the 32-bit form -- six of them per row made the window gathers / scatters VALU-bound at stage 0)
__device__ __forceinline__ long win_to_tok(const WinMap& w, long m) {
  const unsigned mu = (unsigned)m;
  const int t = (int)(mu & 63u);
  unsigned win = mu >> 6;
  const unsigned nwy = (unsigned)w.PW >> 2, nwx = (unsigned)w.PD >> 2, nwz = (unsigned)w.PH >> 2;
  unsigned q = win / nwx;
  const int wx = (int)(win - q * nwx);
  win = q; q = win / nwy;
  const int wy = (int)(win - q * nwy);
  win = q; q = win / nwz;
  const int wz = (int)(win - q * nwz);
  const unsigned b = q;
  int sz = wz * 4 + (t >> 4) + w.s0, sy = wy * 4 + ((t >> 2) & 3) + w.s1, sx = wx * 4 + (t & 3) + w.s2;
  if (sz >= w.PH) sz -= w.PH;
  if (sy >= w.PW) sy -= w.PW;
  if (sx >= w.PD) sx -= w.PD;
  if (sz >= w.H || sy >= w.W || sx >= w.D) return -1;
  return (long)(((b * (unsigned)w.H + (unsigned)sz) * (unsigned)w.W + (unsigned)sy) * (unsigned)w.D + (unsigned)sx);
}
__device__ __forceinline__ long tok_to_win(const WinMap& w, long tok) {
  const unsigned tu = (unsigned)tok;
  unsigned q = tu / (unsigned)w.D;
  const int x = (int)(tu - q * (unsigned)w.D);
  unsigned q2 = q / (unsigned)w.W;
  const int y = (int)(q - q2 * (unsigned)w.W);
  const unsigned b = q2 / (unsigned)w.H;
  const int z = (int)(q2 - b * (unsigned)w.H);
  int pz = z - w.s0, py = y - w.s1, px = x - w.s2;
  if (pz < 0) pz += w.PH;
  if (py < 0) py += w.PW;
  if (px < 0) px += w.PD;
  const unsigned win = ((b * ((unsigned)w.PH >> 2) + ((unsigned)pz >> 2)) * ((unsigned)w.PW >> 2) + ((unsigned)py >> 2)) * ((unsigned)w.PD >> 2) + ((unsigned)px >> 2);
  return (long)win * 64 + ((pz & 3) << 4) + ((py & 3) << 2) + (px & 3);
}

#endif
int k_gemm_nt(int dt, const void* A, long lda, const void* Bw, long ldb, int M, int N, int K, const EpiParams& ep, hipStream_t st);
// the kernel plans the two GEMM dispatches decide on (gemm_plan.hpp), as int rows for the C ABI: pure host functions, no launch
int k_gemm_nt_plan(int dt, long lda, long ldb, int M, int N, int K, int batch, int win_on, int up_k, int ksplit, int* plan);
int k_gemm_nt_plan_table(int* rows, int cap);
int k_gemm_tn_plan(int dt, long lda, long M, int N, int K, int has_rowscale, int rows_per_scale, long ws_floats, int* plan);
// ConvTranspose3d (kernel = stride = k) as GEMMs with the pixel shuffle folded into addressing (unetr_block.py:151-158):
//   fwd:   cat[fine][0:Cout] = x[coarse] . Wt^T + bias   (Wt packed [(tap,co)][ci])
//   dgrad: dx[coarse][ci] = sum_(tap,co) dcat[fine][co] Wd[ci][(tap,co)]
//   wgrad: dW[ci][co][tap] += sum_coarse x[coarse][ci] dcat[fine][co];  dbias[co] += sum dcat
int k_upconv_fwd(int dt, const void* x, const void* Wt, const float* bias, void* cat, long ldc, int B, int v, int k, int Cin, int Cout, hipStream_t st);
int k_upconv_dgrad(int dt, const void* dcat, long ldc, const void* Wd, void* dx, int B, int v, int k, int Cin, int Cout, hipStream_t st);
int k_upconv_wgrad(int dt, const void* dcat, long ldc, const void* x, float* dW, float* dbias, int B, int v, int k, int Cin, int Cout, hipStream_t st);
int k_conv3_nt(int dt, const void* X, const void* Wp, int B, int D, int H, int W, int Cin, int Cout, const EpiParams& ep, hipStream_t st, float* ws = nullptr, long ws_floats = 0);
int k_gemm_tn(int dt, const void* A, long lda, const void* Bm, long ldb, float* Out, long M, int N, int K, const float* rowscale, int rows_per_scale, const TnGeom& gm, hipStream_t st);
// one problem of a grouped weight-gradient launch (host-side descriptor; mirrors nmh_tn_problem in include/nerfmae_hip.h)
struct TnProblemHost {
  const void* A; long lda;        // [M][N] rows = contraction index (dY)
  const void* B; long ldb;        // [M][K] (layer input)
  float* dW; long ldo;            // [N][K] fp32, accumulated
  float* dbias;                   // optional [N]: += column sums of A (times rowscale)
  const float* rowscale;          // optional [M / rows_per_sample]: factor per sample on the rows of A
  long M; int N, K; int rows_per_sample;
  long stride_k;                  // 0: dW[n*ldo + k]; > 0: dW[n*ldo + k*stride_k] (e.g. the [Cin][Cout][k^3] layout of a ConvTranspose3d weight)
  int up_k, up_v;                 // up_k > 0: A is the pixel-shuffled view of a fine-grid tensor (ConvTranspose3d kernel = stride = up_k backward):
                                  // row m = coarse voxel (b,z,y,x) of an up_v^3 grid -> fine row ((b*V+z*k)*V+y*k)*V+x*k, V = up_v*up_k (A already offset by the tap)
  int bias_atomic;                // dbias is shared with other problems of the call: atomic adds
  int n_inner; long stride_n2;    // n_inner > 0: column n = (n / n_inner, n % n_inner) -> dW[(n % n_inner)*ldo + (n / n_inner)*stride_n2 + k*stride_k], dbias[n % n_inner]
};
int k_gemm_tn_grouped(const TnProblemHost* probs, int nprob, float* ws, long ws_floats, hipStream_t st, bool foreground = false);
int k_conv48(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int accumulate, double* stats_acc, hipStream_t st,
             const void* Y1 = nullptr, const float* stats1 = nullptr, float slope = 0.f, long wk_sample_stride = 0, int centered = 0);
int k_conv48_pack_scaled(const float* W, const float* stats, void* out, int B, hipStream_t st);
int k_conv48_mb(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, hipStream_t st);
int k_conv64(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, double* stats_acc, const float* bias, hipStream_t st);
long k_conv64_pack_numel(int Cin, int Cout);
int k_conv64_wgrad(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, int Cin, int Cout, hipStream_t st);
long k_conv64_wgrad_ws_floats();
int k_in_finalize(int dt, const double* acc, float* stats, int B, long V, int C, float eps, hipStream_t st);
int k_conv48_wgrad(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, hipStream_t st, const float* scale_stats = nullptr);
long k_conv48_wgrad_ws_floats();
int k_conv3_wgrad_halo(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, int Cin, int Cout, hipStream_t st);
int k_conv3_tn(int dt, const void* dY, const void* X, float* dW, int B, int D, int H, int W, int Cin, int Cout, hipStream_t st, float* ws = nullptr, long ws_floats = 0);
long k_conv3_tn_fixed_ws_floats(int dt, long rows, int Cin, int Cout);
int k_nearest_up_add(int dt, const void* coarse, void* fine, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, int C, int bwd, hipStream_t st);
int k_vc_transpose(int dt, const void* src, void* dst, int B, long V, int C, int dir, hipStream_t st);
int k_copy_cols(int dt, const void* src, long lds, void* dst, long ldd, long M, int C, hipStream_t st);

// ---- norm.hip ----
// src_mode: 0 direct rows, 1 window-ordered output rows (gather tokens, pads -> 0), 2 patch-merge gather (8 tokens -> 8C row)
struct LnArgs {
  int dt; int src_mode;
  const void* x; void* out;             // x: token-major [T,C]; out: [rows, Cout] (Cout = C or 8C)
  const float* gamma; const float* beta; float eps;
  float* mean; float* rstd;             // per token (modes 0,1) or per output row (mode 2)
  long rows; int C;                     // rows = output rows; C = normalized width (8*Cin for mode 2)
  WinMap wm;                            // modes 1, 2 (mode 2 uses B,H,W,D as the *input* grid)
  const float* pos; const unsigned char* mask; const float* mask_token; long tokens_per_sample;  // patch-embed post-ops (mode 0)
  void* out_tok;                        // mode 1, optional: a second, TOKEN-ordered copy of the normalised rows [T,C] (operand of a token-ordered weight gradient)
  // mode 0 with a mask, optional (patch embed of the KEPT tokens only, k_mask_rowmap): x holds the kept tokens of every sample in compact rows
  // [B][cap_rows][C] -- token tl of sample b at row b * cap_rows + rowmap[tl]; masked tokens have no row and are not read
  const int* rowmap; long cap_rows;
};
int k_ln_fwd(const LnArgs& a, hipStream_t st);
// mask [n] (1 = removed) -> rowmap [n + 2]: rowmap[t] = number of kept tokens in front of token t (its compact row), -1 for a removed token (and for kept tokens
// beyond cap rows: rowmap[n + 1] = 1 then); rowmap[n] = min(kept count, cap)
int k_mask_rowmap(const unsigned char* mask, int n, int cap, int* rowmap, hipStream_t st);
struct LnBwdArgs {
  int dt; int src_mode;
  const void* dy;                       // mode 0: [T,C]; mode 1: window-ordered [Tw,C]; mode 2: [rows, 8C]
  const void* x; const float* gamma; const float* mean; const float* rstd;
  const void* dres;                     // optional residual gradient added to dx (modes 0,1)
  void* dx;                             // token-major [T,C]
  float* dgamma; float* dbeta;          // fp32 accumulators (atomicAdd)
  long rows; int C; WinMap wm;
  const unsigned char* mask; float* dmask_token; long tokens_per_sample;
  void* dyw; const float* dyw_scale;    // MODE 0 only: second output in window order (wm), scaled per sample (fused window gather)
  int dyw_pads;                         // set by k_ln_bwd: the window-ordered tensor has pad rows (no token) -- the kernel writes their zeros
  float* part;                          // optional [k_ln_bwd_blocks(rows, C)][2C]: every workgroup leaves its dgamma / dbeta sums here (plain stores) instead of adding
                                        // them to dgamma / dbeta with 2C same-address atomics; k_ln_param_reduce adds the column sums later, off the dependent chain
  // mode 0 with a mask, optional (see LnArgs): x and dx are compact [B][cap_rows][C]; masked tokens write no row, the rows behind the kept count are zeroed
  const int* rowmap; long cap_rows;
};
int k_ln_bwd(const LnBwdArgs& a, hipStream_t st);
long k_ln_bwd_blocks(long rows, int C);
struct LnReduceItem { const float* part; float* dgamma; float* dbeta; long nb; int C; int pad_; };   // == nmh_ln_reduce_item
constexpr int LN_REDUCE_MAX = 96;
int k_ln_param_reduce(const LnReduceItem* items, int n, hipStream_t st);

// ---- block0.hip: stage 0's first Swin block on the kept windows only, compact layout [B][capW + 1][64][C] (slot capW = the representative all-mask window) ----
constexpr int B0_LN_BWD_BLOCKS = 256;   // workgroups (at most) of k_b0_ln_bwd: part holds B0_LN_BWD_BLOCKS * 3 C floats
int k_b0_supported(int C);
// mask [g^3] (1 = removed, constant on every 4^3 window) -> rowmap [g^3 + 2] as k_mask_rowmap's, the rows in window-major order (64 * slot + in-window position);
// wmap [nW + capW]: wmap[w] = slot of window w (-1: removed), wmap[nW + k] = window of slot k (-1: behind the kept count)
int k_b0_rowmap(const unsigned char* mask, int g, int capW, int* rowmap, int* wmap, hipStream_t st);
int k_b0_ln_fwd(int dt, const void* y0, void* out, const float* gamma, const float* beta, float eps, float* mean, float* rstd, const float* pos, const float* mask_token,
                const int* wmap, int B, int g, int capW, int C, hipStream_t st);
int k_b0_ln_bwd(int dt, const void* dx0, const void* y0, const float* gamma, const float* mean, const float* rstd, void* dy0, float* dgamma, float* dbeta, float* dmask_token,
                float* part, long part_floats, const int* wmap, int B, int g, int capW, int C, hipStream_t st);
int k_b0_expand(int dt, const void* yc, void* y, const int* wmap, int B, int g, int capW, int C, hipStream_t st);
int k_b0_reduce(int dt, const void* dy, void* dyc, const int* wmap, int B, int g, int capW, int C, hipStream_t st);

int k_window_scatter_residual(int dt, const void* yw, const void* x, void* out, const float* rowscale, int C, const WinMap& wm, hipStream_t st);
int k_window_gather_scale(int dt, const void* dx, void* dyw, const float* rowscale, int C, const WinMap& wm, hipStream_t st);

// ---- cconv.hip: ConvTranspose3d(96 -> 48, k = s = 4) composed with the 3x3x3 conv that follows it (decoder1, forward) ----
int k_cconv_pack(const float* Wt, const float* W1, const float* bt, void* Wcp, float* delta, float* ws, hipStream_t st, float* Mtab = nullptr);
int k_cconv_mean(const void* x, const float* Mtab, const float* delta, double* C27, float* mhat, int B, int v, hipStream_t st);
long k_cconv_pack_numel();
long k_cconv_pack_ws_floats();
int k_cconv_fwd(const void* X, const void* Wcp, const float* delta, void* Y, int B, int v, double* stats_acc, hipStream_t st, const float* mhat = nullptr, float slope = 0.f);
int k_cconv_wgrad(const void* X, const void* dY, const float* WtT, const float* bt, float* dW1, float* dWt, float* dbt, float* ws, int B, int v, int phase, hipStream_t st);
long k_cconv_dpack_numel();
int k_cconv_dpack(const void* Wcp, void* Wdp, hipStream_t st);
int k_cconv_dgrad(const void* dY, const void* Wdp, const void* add, void* DX, int B, int v, hipStream_t st);
long k_cconv_wgrad_ws_floats();
long k_upconv4_pack_numel();
int k_upconv4_pack(const float* ws, void* Wup, hipStream_t st);
int k_upconv4_fwd(const void* X, const void* Wup, const float* bt, void* Y, int B, int v, hipStream_t st);

// ---- mlp_fused.hip: LN -> fc1 -> GELU -> fc2 -> row-scale -> + residual in one launch (bf16), and its backward ----
int k_mlp_fused_supported(int C);
int k_mlp_fused_fwd(const void* x1, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2T, const float* b2, const float* rowscale,
                    int rows_per_scale, void* x2, float* mean, float* rstd, long M, int C, float eps, hipStream_t st);
int k_mlp_fused_bwd(const void* x1, const void* dx2, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2T, const float* rowscale,
                    int rows_per_scale, void* dx1, void* x1n, void* hact, void* dh, float* dgamma, float* dbeta, void* dyw, const float* dyw_scale, const WinMap* wm,
                    long M, int C, float eps, hipStream_t st);

// ---- swin_block.hip: fused Swin-block kernels (bf16, C = 96 NW) ----
struct SwinPackItem { const float* w0; const float* w1; void* dst; int type; int C; };   // mirrors nmh_swin_pack_item
int k_swin_supported(int C);
long k_swin_stream_numel(int type, int C);
int k_swin_pack(const SwinPackItem* items, int n, hipStream_t st);
long k_swin_mlp_split_ws_bytes(long M, int C);
int k_swin_mlp_fwd(const void* x1, const float* gamma, const float* beta, const void* wstream, const float* b1, const float* b2, const float* rowscale, int rows_per_scale,
                   void* x2, void* x1n, void* hp, void* hact, float* mean, float* rstd, long M, int C, float eps, void* split_ws, long split_ws_bytes, hipStream_t st);
int k_swin_attn_fwd(const void* x, const float* gamma, const float* beta, const void* wstream, const float* bqkv, const float* table, const float* bproj,
                    const float* rowscale, int rows_per_scale, void* xnw, float* mean, float* rstd, void* qkv, void* o, float* lse, void* x1,
                    const WinMap& wm, int C, float eps, int token_saves, hipStream_t st);

// instance norm over channels-last [B, V, C]; stats[b][c] = {mean, rstd}
int k_in_stats(int dt, const void* x, float* stats, double* scratch, int B, long V, int C, float eps, hipStream_t st);
// out = lrelu( IN(x) [+ r | + IN(r)] ); rmode 0 none, 1 plain residual, 2 normalized residual (stats_r)
int k_in_apply(int dt, const void* x, const float* stats, const void* r, const float* stats_r, int rmode, void* out, int B, long V, int C, float slope, hipStream_t st);
// sums[b][c] = {sum g, sum g*xhat} (and sums_r for rmode 2), g = dout * lrelu'(out)
int k_in_bwd_reduce(int dt, const void* dout, const void* out, const void* x, const float* stats, const void* r, const float* stats_r, int rmode,
                    double* sums, double* sums_r, int B, long V, int C, float slope, hipStream_t st);
// dx = rstd*(g - S1/V - xhat*S2/V); rmode 1: dr (+)= g ; rmode 2: dr = IN-bwd wrt r
int k_in_bwd_apply(int dt, const void* dout, const void* out, const void* x, const float* stats, const double* sums, const void* r, const float* stats_r,
                   const double* sums_r, int rmode, void* dx, void* dr, int dr_accumulate, int B, long V, int C, float slope, hipStream_t st);
int k_in_bwd_apply_bg(int dt, const void* dout, const void* x, const float* stats, const double* sums, void* dx, int B, long V, int C, float slope, hipStream_t st, int centered = 0);

// ---- attn.hip ----
int k_attn_fwd(int dt, const void* qkv, const float* bias_table, void* out, float* lse, int heads, int C, const WinMap& wm, hipStream_t st, int tok_out = 0);
int k_attn_bwd(int dt, const void* qkv, const float* bias_table, const void* dout, const float* lse, void* dqkv, float* dbias_table, int heads, int C, const WinMap& wm, hipStream_t st, void* dqkv_tok = nullptr);
int k_attn_pad_rows_colsum(int dt, const void* x, int N, const WinMap& wm, float* out, hipStream_t st);
int k_attn_pad_rows_colsum_grouped(int dt, const void* const* xs, float* const* outs, int n, int N, const WinMap& wm, hipStream_t st);

// ---- misc.hip ----
int k_embed_gather(int dt, const float* x, void* A, int B, int R, hipStream_t st, const int* rowmap = nullptr, long cap_rows = 0);
int k_up_cat_fwd(int dt, const void* upre, const float* bias, const void* skip, void* out, int B, int v, int k, int Cout, hipStream_t st);
int k_up_cat_bwd(int dt, const void* dcat, void* dupre, void* dskip, float* dbias, int B, int v, int k, int Cout, int has_skip, hipStream_t st);
struct LossArgs {
  int dt; const void* d0; const float* Wout; const float* bout; const float* target;  // d0 [B,R^3,Cd]; target fp32 NCDHW (B,4,R,R,R)
  const int* extents;                    // [B][3] valid extent per axis (A0,A1,A2)
  const unsigned char* tokmask;          // [g^3] 1 = removed (shared by the batch)
  int B, R, Cd;
  double* sums;                          // [4]: sum_rgb, n_occ, sum_alpha, n_rm  ([8] with dp: + sum over voxels of dp[o])
  float* pred;                           // optional fp32 NCDHW (B,4,R,R,R)
  float* dp;                             // optional fp32 [B*R^3][4]: un-normalised d(loss)/d(pred) (forward only)
  double* bwd_sums;                      // optional (k_tail_fwd): [B][C][4] {sum g_rgb, sum g_rgb*xhat, sum g_a, sum g_a*xhat} + [4][C] head weight-gradient sums,
                                         // all on the un-normalised d(pred): the InstanceNorm-backward / head reductions of the tail backward, taken in the forward pass
  unsigned char* sign_mask;              // optional (k_tail_fwd, bf16 / 48 channels): [B*R^3][8] bytes (Cd = 48: 6 used), bit j of byte c = [d0[voxel][8c + j] > 0]: all the tail
                                         // backward needs of d0 once its sums come from bwd_sums -- it then reads 6 bytes per voxel instead of the 96-byte residual row
};
int k_loss_fwd(const LossArgs& a, hipStream_t st);
int k_loss_finalize(const double* sums, float* losses, hipStream_t st);
int k_loss_bwd(const LossArgs& a, void* dd0, float* dWout, float* dbout, hipStream_t st);
// d0 = lrelu(IN(x)+r) -> out, fused with the 1x1 head and the loss terms (a.d0 unused; sums/pred/dp as in k_loss_fwd)
int k_tail_fwd(const LossArgs& a, const void* x, const float* stats, const void* r, void* out, float slope, hipStream_t st);
// the training form of the pass with the residual r = ConvT_{k=s=4}(xcoarse) + bt formed inside from the coarse tensor (Wr: k_tail_r_pack); d(pred), bwd_sums, sign_mask required
// box: only the cells of each sample's valid box are walked and written (tail_box.hpp; the target must be zero outside the extents, pred is refused)
int k_tail_fwd_coarse(const LossArgs& a, const void* x, const float* stats, const void* xcoarse, const void* Wr, const float* bt, float slope, hipStream_t st, bool box = false);
long k_tail_r_pack_numel();
int k_tail_r_pack(const float* ws, void* Wr, hipStream_t st);
// loss backward + backward of d0 = lrelu(IN(x)+r) in two elementwise passes over (d0, x, dp): dx, dr = g; also head weight/bias gradients
int k_tail_bwd(int dt, const void* d0, const void* r, const void* xin, const float* in_stats, const float* dp, const double* loss_sums, const float* Wout, double* in_sums,
               void* dx, void* dr, float slope, float* dWout, float* dbout, int B, long V, int C, const double* bwd_sums, hipStream_t st, const unsigned char* sign_mask = nullptr,
               const int* extents = nullptr, int R = 0);   // extents (+ R, V = R^3): dp and sign_mask hold each sample's box alone (k_tail_fwd_coarse with box)
int k_bias_grad(int dt, const void* dY, float* db, long M, int N, const float* rowscale, int rows_per_scale, hipStream_t st);
int k_add_inplace(int dt, void* a, const void* b, long n, hipStream_t st);
int k_add(int dt, void* out, const void* a, const void* b, long n, hipStream_t st);
int k_fill_f32(float* p, float v, long n, hipStream_t st);
// ---- heads.hip (voxel super-resolution / semantics heads) ----
int k_grid_to_cl8(int dt, const float* src, void* dst, int B, long V, hipStream_t st);
int k_cl_to_ncdhw_up(int dt, const void* src, float* dst, int B, int Co, int Cp, int R, int Ro, float inv_scale, hipStream_t st);
int k_ncdhw_up_adjoint(int dt, const float* dpred, void* g, int B, int Co, int Cp, int R, int Ro, float inv_scale, hipStream_t st);
int k_add_cols_f32(const float* src, long lds, float* dst, long ldd, long M, int C, hipStream_t st);
int k_sr_loss_fwd(const float* pred, const float* tgt, int B, long V, double* sums, float* loss, hipStream_t st);
int k_sr_loss_bwd(const float* pred, const float* tgt, int B, long V, const double* sums, float gscale, float* dpred, hipStream_t st);
int k_masked_ce_fwd(const float* logits, const float* labels, const float* cw, int B, int K, long V, double* sums, double* iou, float* out, hipStream_t st);
int k_masked_ce_bwd(const float* logits, const float* labels, const float* cw, int B, int K, long V, const double* sums, float gscale, float* dlogits, hipStream_t st);
#define NMH_SEM_EVAL_ROWS 1024   // rows of the caller's partial slabs: one per workgroup of the evaluation pass
int k_sem_eval(const float* logits, const float* labels, const float* cw, int B, int K, long V, double* fpart, long long* ipart, float* out, long long* counts,
               long long* pred_vis, long long* target_vis, long long* totals, hipStream_t st);
int k_sem_label_counts(int dt, const void* output, const void* target, long n, int K, long long* ipart, long long* counts, hipStream_t st);
// ---- rotated.hip (the reference's two native downstream ops: rotated 3-D RoIAlign, polygon vertex sort) ----
// layout 0: channels-last (B,W,L,H,C) in dt -> [N,PW,PL,PH,C] in dt; layout 1: NCWLH fp32 -> [N,C,PW,PL,PH] fp32.  dx is fp32 in both and is added to.
int k_roi_align_rotated_3d_fwd(int layout, int dt, const void* x, const float* rois, void* out, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH,
                               float spatial_scale, int sampling_ratio, hipStream_t st);
int k_roi_align_rotated_3d_bwd(int layout, int dt, const void* dout, const float* rois, float* dx, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH,
                               float spatial_scale, int sampling_ratio, hipStream_t st);
int k_sort_vertices(const float* vertices, const unsigned char* mask, const int* num_valid, int* idx, int B, int N, int M, hipStream_t st);
// ---- rotated_iou.hip (oriented 3-D box IoU / GIoU / DIoU losses, all-pairs IoU, rotated NMS) ----
// mode: 0 IoU, 1 GIoU smallest, 2 GIoU aligned, 3 DIoU smallest, 4 DIoU aligned.  Boxes [n][7] fp32 (x,y,z,w,l,h,theta in radians).
#define NMH_OBB_NMS_MAX 16384
int k_obb_iou_fwd(int mode, const float* b1, const float* b2, long n, float* iou, float* u3d, float* zr, float* loss, float* wc, float* hc, float* c1, float* c2, hipStream_t st);
int k_obb_iou_bwd(int mode, const float* b1, const float* b2, long n, const float* g_iou, const float* g_u3d, const float* g_loss, int g_one, float* d1, float* d2, hipStream_t st);
int k_obb_iou_pairwise(int ncols, const float* b1, const float* b2, int N, int M, float* iou, hipStream_t st);
int k_obb_nms_mask(int ncols, const float* boxes, const int* cat, int N, float thr, unsigned long long* mask, hipStream_t st);
int k_obb_nms_scan(const unsigned long long* mask, int N, int* keep, int* count, hipStream_t st);
// ---- fcos.hip (FCOS target assignment, focal / regression / centerness losses, encode / decode of the midpoint-offset OBB form) ----
// dims: HOST [nlevels][4] = (w, l, h, stride); offs: HOST [N+1]; pointer tables: HOST arrays of nlevels DEVICE pointers.  Dense layout: fcos.hip.
#define NMH_FCOS_MAX_SCENES 64
long k_fcos_num_blocks(int nlevels, const int* dims, int N);
int k_fcos_assign(int nlevels, const int* dims, int N, int ncols, const float* boxes, const int* offs, const int* sizes, const unsigned char* const* masks, float radius,
                  int norm_targets, float* labels, float* targets, int* gt_index, float* ctr_t, unsigned char* valid, float* partials, float* scalars, hipStream_t st);
int k_fcos_focal_fwd(int nlevels, const int* dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world, float* partials,
                     float* loss, hipStream_t st);
int k_fcos_focal_bwd(int nlevels, const int* dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world, const float* g_loss,
                     float* const* dcls, hipStream_t st);
int k_fcos_pos_fwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels, const float* targets,
                   const float* ctr_t, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss, hipStream_t st);
int k_fcos_pos_bwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels, const float* targets,
                   const float* ctr_t, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr, float* const* dreg, float* const* dctr,
                   hipStream_t st);
// the same with the 2-D projection term (ncols 8 only): term += proj2d_weight T / 160 / 16 under the cameras of get_w2cs(160); proj2d_weight < 0: without it
int k_fcos_pos2d_fwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr, const float* labels,
                     const float* targets, const float* ctr_t, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss,
                     hipStream_t st);
int k_fcos_pos2d_bwd(int nlevels, const int* dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr, const float* labels,
                     const float* targets, const float* ctr_t, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr, float* const* dreg,
                     float* const* dctr, hipStream_t st);
int k_fcos_obb_encode(const float* loc, const float* boxes, long n, float* out, hipStream_t st);
int k_fcos_obb_decode_fwd(const float* loc, const float* reg, long n, float* out, hipStream_t st);
int k_fcos_obb_decode_bwd(const float* reg, const float* gbox, long n, float* dreg, hipStream_t st);
// ---- fcos_post.hip (FCOS inference post-processing: threshold, exact top-k, decode, batched NMS, post-NMS cut) ----
// level_n: HOST [nlevels] locations per level and scene; pointer tables as above; cap = sum over levels of min(pre_top_n, n)
long k_fcos_post_cap(int nlevels, const int* level_n, int N, int pre_top_n);
int k_fcos_post_select(int nlevels, const int* level_n, int N, int ncols, int pre_top_n, const float* const* cls, const float* const* reg, const float* const* ctr,
                       const float* const* locs, const unsigned char* const* masks, const int* sizes, float pre_thresh, float min_size, unsigned* keys, float* pre_boxes,
                       float* pre_scores, int* pre_counts, hipStream_t st);
int k_fcos_post_nms(int nlevels, const int* level_n, int N, int ncols, int pre_top_n, const float* pre_boxes, const float* sorted_scores, const long* order, const int* pre_counts,
                    float nms_thresh, int post_top_n, unsigned long long* mask, int* keep, float* boxes, float* scores, int* counts, hipStream_t st);
// ---- rpn.hip (RPN anchor target assignment, balanced sampling, objectness / box losses) ----
// dims: HOST [nlevels][7] = (W, H, D, sx, sy, sz, A); base: HOST [sum A][3] half extents; offs: HOST [N+1]; pointer tables as above.  Layouts: rpn.hip.
#define NMH_RPN_MAX_ANCHORS 32
long k_rpn_num_blocks(int nlevels, const int* dims, int N);
int k_rpn_assign(int nlevels, const int* dims, const float* base, int N, int ncols, const float* boxes, const int* offs, const int* ori, float fg, float bg, unsigned* gtmax,
                 float* labels, int* midx, float* targets, hipStream_t st);
int k_rpn_sample(int N, long n, const float* labels, int batch, int want_pos, long* rng, unsigned char* flags, int* counts, hipStream_t st);
// the losses.  loss_type < 0: smooth-L1 on targets (ncols 6 | 8); else 0 iou, 1 linear_iou, 2 giou, 3 diou over the decoded proposals (ncols 8 only; targets unused).
// base, boxes DEVICE [offs[N]][6|7], offs, midx DEVICE [N][n]: read by the IoU types and by the 2-D term, else unused.  cams: HOST [48], or NULL for the losses without the
// 2-D projection term: partials DEVICE [3 nblocks], scalars DEVICE [3] = (objectness, box, sampled anchors); with it: res > 0, partials [5 nblocks], scalars [5] =
// (objectness, box, sampled anchors, 2-D, sampled positives), and g_2d
int k_rpn_loss_fwd(int nlevels, const int* dims, const float* base, int N, int ncols, int loss_type, const float* const* obj, const float* const* reg, const unsigned char* flags,
                   const float* targets, const float* boxes, const int* offs, const int* ori, const int* midx, const float* cams, float res, float* partials, float* scalars,
                   hipStream_t st);
int k_rpn_loss_bwd(int nlevels, const int* dims, const float* base, int N, int ncols, int loss_type, const float* const* obj, const float* const* reg, const unsigned char* flags,
                   const float* targets, const float* boxes, const int* offs, const int* ori, const int* midx, const float* cams, float res, const float* scalars,
                   const float* g_obj, const float* g_reg, const float* g_2d, float* const* dobj, float* const* dreg, hipStream_t st);
// ---- proj2d.hip (the 2-D projection term on rows of boxes; cams: HOST [48] = the fused K [R|t] of four cameras, row-major 3x4) ----
int k_proj2d_fwd(const float* pred, const float* target, long n, int ncols, const float* cams, float* terms, hipStream_t st);
int k_proj2d_bwd(const float* pred, const float* target, const float* g_terms, long n, int ncols, const float* cams, float* dpred, hipStream_t st);
void k_proj2d_cameras(float res, float* cams);           // HOST -> HOST: the cameras of get_w2cs(res)
// ---- rpn_post.hip (RPN proposals: decode, exact top-k per level on the raw logits, per-level NMS, post-NMS cut) ----
// mesh: HOST [3]; ori: DEVICE [N][3] or NULL.  Slot layout, sort key and tie rules: rpn_post.hip.
long k_rpn_post_cap(int nlevels, const int* dims, int N, int pre_top_n);
long k_rpn_post_mask_words(int nlevels, const int* dims, int N, int pre_top_n);
int k_rpn_decode(int nlevels, const int* dims, const float* base, int N, int ncols, const float* const* reg, float* boxes, hipStream_t st);
int k_rpn_post_select(int nlevels, const int* dims, const float* base, int N, int ncols, int pre_top_n, const float* const* obj, const float* const* reg, const int* ori,
                      const int* mesh, float score_thresh, float min_size, long* pre_keys, float* pre_boxes, float* pre_scores, int* pre_index, int* pre_counts, hipStream_t st);
int k_rpn_post_nms(int nlevels, const int* dims, int N, int ncols, int pre_top_n, const float* pre_boxes, const float* pre_scores, const int* pre_index, const long* sorted_keys,
                   const long* order, const int* pre_counts, float nms_thresh, int post_top_n, unsigned long long* mask, int* keep, float* boxes, float* scores, int* levels,
                   int* index, int* counts, hipStream_t st);
// ---- roi_head.hip (RoI stage of the two-stage detector: proposal targets, pyramid RoI pooling, box-head losses, decode) ----
// offs: HOST [N+1]; dims: HOST [nlevels][3] = (W, H, D); scales: HOST [nlevels]; maps / dmaps: HOST tables of nlevels DEVICE pointers.  Layouts: roi_head.hip.
#define NMH_ROI_MAX_GRID 1024
#define NMH_ROI_MAX_CELLS 4096
#define NMH_ROI_MAX_CLASSES 1024
int k_roi_targets(int N, int cap, int ncols, int R, int is_sample, const float* boxes, const int* levels, const int* counts, const float* gt, const float* gt_labels, const int* offs,
                  int want_fg, float fg, float bg, long* rng, float* miou, int* arg, int* lists, int* keep, int* counts2, float* labels, float* rois, float* gt_rois,
                  hipStream_t st);
int k_roi_level_map(long M, const float* boxes, int stride, int ncols, int k_min, int k_max, float canonical_scale, float canonical_level, float eps, int* out, hipStream_t st);
int k_roi_pool_fwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps, const float* rois,
                   const int* lvl_override, float* out, int* argout, hipStream_t st);
int k_roi_pool_bwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const int* argout,
                   const float* rois, const int* lvl_override, float* const* dmaps, hipStream_t st);
int k_roi_interp_fwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps, const float* rois,
                     const int* lvl_override, float* out, hipStream_t st);
int k_roi_interp_bwd(int nlevels, const int* dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const float* rois,
                     const int* lvl_override, float* const* dmaps, hipStream_t st);
long k_roi_loss_blocks(long M);
int k_roi_loss_fwd(long M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* rois, int roi_stride, const float* gt_rois,
                   float* targets, float* partials, float* scalars, hipStream_t st);
int k_roi_loss_bwd(long M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* targets, const float* scalars, const float* g_obj,
                   const float* g_reg, float* dscores, float* ddeltas, hipStream_t st);
int k_roi_decode(long M, int ncols, const float* deltas, const float* rois, int roi_stride, float* out, hipStream_t st);
// ---- roi_post.hip (RoI post-processing: softmax, decode, clip, size and score filters, NMS per scene) ----
// Everything DEVICE.  N <= NMH_FCOS_MAX_SCENES, R <= NMH_OBB_NMS_MAX, 2 <= n_classes <= NMH_ROI_MAX_CLASSES.  Semantics, sort key and tie rules: roi_post.hip.
int k_roi_post_select(int N, int R, int n_classes, int ncols, const float* pred_scores, const float* pred_bbox_deltas, const float* rois, const int* counts, const int* mesh_sizes,
                      float score_thresh, float min_size, int is_reg, int threshold_mode, float* cand_boxes, float* cand_scores, int* keys, hipStream_t st);
int k_roi_post_nms(int N, int R, int ncols, const float* cand_boxes, const float* cand_scores, const int* sorted_keys, const long* order, float nms_thresh, unsigned long long* mask,
                   int* keep, float* boxes, float* scores, int* index, int* counts_out, hipStream_t st);
// ---- det_eval.hip (detection evaluation: IoU matrix and row best, greedy recall matching, AP claims, precision / recall scan) ----
// limits, thresholds: HOST arrays; everything else DEVICE.  Layouts, tie rules and the deviations from eval.py: det_eval.hip.
#define NMH_DET_EVAL_MAX_GT 1024
#define NMH_DET_EVAL_MAX_LIMITS 8
#define NMH_DET_EVAL_MAX_THRESH 8
int k_det_eval_iou(int ncols, int N, int cap, int row_stride, int col_offset, const float* boxes, const int* counts, int Gmax, const float* gt, const int* gt_counts, float* iouT,
                   float* best_iou, int* best_gt, hipStream_t st);
int k_det_eval_match(int N, int cap, int Gmax, const int* counts, const int* gt_counts, const float* iouT, int nlimits, const int* limits, float* gt_overlaps, int* counted,
                     hipStream_t st);
int k_det_eval_claims(int N, int cap, int Gmax, const int* counts, const float* best_iou, const int* best_gt, int nthresh, const float* thresholds, int top_k, unsigned char* tp_mask,
                      unsigned char* kept, hipStream_t st);
int k_det_eval_pr(long M, const unsigned char* bits, const int* n_det, const int* num_gt, int nthresh, int* tp_cum, int* fp_cum, float* recalls, float* precisions, double* ap,
                  hipStream_t st);
// ---- rpn_head.hip (RPNHead's output stage: cls_logits + bbox_pred from the channels-last activation to the NCDHW fp32 planes, and back; ReLU passes) ----
// vox: HOST [nlevels] voxels per scene; t / obj / reg / g_* / dt_out: HOST tables of nlevels DEVICE pointers.  Layouts: rpn_head.hip.
long k_rpn_head_bwd_ws_floats(int nlevels, const int* vox, int N, int Cin, int A, int C);
int k_rpn_head_out_fwd(int dt, int nlevels, const int* vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box, const float* b_cls,
                       const float* b_box, float* const* obj, float* const* reg, hipStream_t st);
int k_rpn_head_out_bwd(int dt, int nlevels, const int* vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box,
                       const float* const* g_obj, const float* const* g_reg, void* const* dt_out, float* partials, float* dw_cls, float* dw_box, float* db_cls, float* db_box,
                       hipStream_t st);
int k_relu_(int dt, void* x, long n, hipStream_t st);
int k_relu_bwd_(int dt, void* dy, const void* y, long n, hipStream_t st);
// ---- box_head.hip (RCNN, the box head of the two-stage detector: both Linear layers from the channels-last activation [M][S][C] to the fp32 outputs, and back) ----
// Layouts, limits and the order of every sum: box_head.hip.
int k_box_head_pack(int dt, int reg, int ncls, int C, int S, const float* w_box, const float* w_cls, void* wcat, hipStream_t st);
int k_box_head_out_fwd(int dt, int M, int S, int C, int reg, int ncls, int flatten, int relu, const void* x, const void* wcat, const float* b_box, const float* b_cls, float* xmean,
                       float* out_box, float* out_cls, hipStream_t st);
long k_box_head_bwd_ws_floats(int M, int S, int C, int reg, int ncls, int flatten);
int k_box_head_out_bwd(int dt, int M, int S, int C, int reg, int ncls, int flatten, int relu, const void* x, const void* wcat, const float* xmean, const float* g_box,
                       const float* g_cls, void* dx, float* dxmean, float* partials, float* dw_box, float* dw_cls, float* db_box, float* db_cls, hipStream_t st);
long k_box_head_colsum_ws_floats(long R, int C);
int k_box_head_colsum(int dt, const void* dy, long R, int C, float* partials, float* db, hipStream_t st);
// ---- fcos_head.hip (FCOSHead between its tower convolutions: GroupNorm + ReLU forward and backward, the three 3x3x3 output convs with their epilogue, and back) ----
// vox / tower: HOST [njobs]; dims: HOST [3 nlevels] = W, L, H; every const* const* / * const* argument is a HOST table of DEVICE pointers.  Layouts: fcos_head.hip.
long k_fcos_gn_ws_doubles(int njobs, const int* vox, int N, int C);
int k_fcos_gn_stats(int dt, int njobs, const int* vox, int N, int C, int G, float eps, const void* const* x, double* ws, float* stats, hipStream_t st);
int k_fcos_gn_apply(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* x, const float* stats, const float* const* gamma,
                    const float* const* beta, void* const* y, hipStream_t st);
int k_fcos_gn_bwd(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* dy, const void* const* x, const void* const* y, const float* stats,
                  const float* const* gamma, double* ws, float* sums, float* const* dgamma, float* const* dbeta, void* const* dx, hipStream_t st);
int k_fcos_out_fwd(int dt, int nlevels, const int* dims, const float* strides, int N, int C, int nreg, int ctr_on_reg, int mode, const void* const* act, const void* const* w16,
                   const float* b_cls, const float* b_box, const float* b_ctr, const float* const* scale, float* const* cls, float* const* reg, float* const* ctr,
                   float* const* u, hipStream_t st);
long k_fcos_out_pack_ws_floats(int nlevels, const int* dims, int N);
int k_fcos_out_bwd_pack(int dt, int nlevels, const int* dims, const float* strides, int N, int nreg, int ctr_on_reg, int mode, const float* const* g_cls, const float* const* g_reg,
                        const float* const* g_ctr, const float* const* u, const float* const* scale, void* const* g16, float* const* gt, float* partials, float* db_cls,
                        float* db_box, float* db_ctr, float* const* dscale, hipStream_t st);
long k_fcos_out_wgrad_ws_floats(int nlevels, const int* dims, int N, int C);
int k_fcos_out_wgrad(int dt, int nlevels, const int* dims, int N, int C, int nreg, int ctr_on_reg, const void* const* act, const float* const* gt, float* partials, float* dw_cls,
                     float* dw_box, float* dw_ctr, hipStream_t st);
int k_step_params(const unsigned* bits, int nb, int g, unsigned char* tokmask, const float* hyper_host, float* hyper_dev, const int* ext_host, int n_ext, int* ext_dev, hipStream_t st);
int k_grad_cast(int to_bf16, const void* src, void* dst, long n, float scale, hipStream_t st);

struct PackDesc { const float* src; void* dst; int mode; int d0, d1, d2; long n; };
int k_pack_weights(int dt, const PackDesc* descs_dev, const int* blk2desc_dev, const long* blkstart_dev, int nblocks, hipStream_t st);
int k_sqnorm(const float* g, long n, double* acc, hipStream_t st);
int k_clip_coef(const double* acc, float max_norm, float* coef, float* norm_out, hipStream_t st);
// gradient accumulation: the clip of the mean of k micro-gradients from the squared norm of their sum (inv_k: device scalar 1 / k, set by k_grad_scale)
int k_clip_coef_mean(const double* acc, float max_norm, const float* inv_k, float* coef, float* norm_out, hipStream_t st);
int k_grad_scale(float inv_k, float* inv_k_dev, hipStream_t st);
int k_adamw(float* p, float* g, float* m, float* v, long n, const float* hyper /*lr,b1,b2,eps,wd,bc1,bc2,zero_g*/, const float* coef, hipStream_t st);
// the two passes under a range table: bounds[R+1] (device int64), scale[R][2] = (lr_scale, wd_scale); -5 for a table the host check refuses (misc.hip)
int k_sqnorm_ranges(const float* g, long n, const long* bounds, const float* scale, int R, double* acc, hipStream_t st);
int k_adamw_ranges(float* p, float* g, float* m, float* v, long n, const float* hyper, const float* coef, const long* bounds, const float* scale, int R, hipStream_t st);

// raw scene (W,L,H,4) fp32|uint8 -> padded (4,R,R,R) fp32 network input; flags: 1 rotate (z-up 90 deg), 2 flip axis 0, 4 flip axis 1, 8 density->alpha
int k_grid_prepare(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, hipStream_t st);
// misc.hip: the label volume of the same scene, (W,L,H) fp32 / int32 / int64 / uint8 (dt 0..3) -> the (R,R,R) fp32 slot, rot / flips of k_grid_prepare
int k_labels_prepare(int dt, const void* src, int W, int L, int H, float* dst, int R, int flags, hipStream_t st);
// det_input.hip: k_grid_prepare with rotate_and_scale_scene's trilinear resample (angle in radians, scale) applied after rot / flips; extents >= 2
int k_grid_prepare_rs(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, float angle, float scale, hipStream_t st);
// boxes [total_rows, cols = 6 | 7] -> out; host tables itab [n_scenes][7] = first row, count, flags, has_rs, e0, e1, e2 and ftab [n_scenes][2] = angle, scale
int k_boxes_augment(const float* boxes, float* out, int cols, int total_rows, int n_scenes, const int* itab, const float* ftab, hipStream_t st);
