// extern "C" layer of libnerfmae_hip.so (see include/nerfmae_hip.h).  No torch types; plain pointers + sizes.
#include "../../include/nerfmae_hip.h"
#include "kernels.hpp"
#include <cstdio>

static inline WinMap to_wm(const int* w) {
  WinMap m{};
  if (w) { m.B = w[0]; m.H = w[1]; m.W = w[2]; m.D = w[3]; m.PH = w[4]; m.PW = w[5]; m.PD = w[6]; m.s0 = w[7]; m.s1 = w[8]; m.s2 = w[9]; }
  return m;
}
#define ST ((hipStream_t)stream)
#define NMH_DT_BF16_C 1
// required pointers: a NULL yields the argument-error code -4 instead of a device fault
#define REQ(...) do { const void* req_[] = {__VA_ARGS__}; for (const void* q_ : req_) if (!q_) return -4; } while (0)
// hipGetLastError() is sticky per thread: clear whatever an unrelated earlier runtime call left behind, so that the
// post-launch check in the k_* launchers reports only this call's launch status
#define CLR() (void)hipGetLastError()

extern "C" {
int nmh_version(void) { return 100; }
const char* nmh_error_string(int code) {
  if (code == 0) return "ok";
  if (code == -1) return "nmh: unsupported operation";
  if (code == -2) return "nmh: shape constraint violated (channel counts must be multiples of 8; head_dim must be 32)";
  if (code == -3) return "nmh: row too wide for the layernorm kernels";
  if (code == -5) return "nmh: bad range table (1 <= R <= NMH_ADAMW_MAX_RANGES; bounds ascending from 0 to n, interior boundaries multiples of 4; scales finite and >= 0)";
  if (code < 0) return "nmh: invalid argument";
  return hipGetErrorString((hipError_t)code);
}
int nmh_gemm_nt(int dt, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N, int K, void* C, int64_t ldc, const float* bias, int act, void* C2,
                const void* resid, const float* rowscale, int rows_per_scale, int accumulate, void* stream) {
  CLR();
  REQ(A, W, C);
  if (M <= 0) return 0;
  // every operand and output access of the kernels is a 16-byte vector: a row stride that is not a whole number of them would put rows
  // off that alignment, which none of the loaders (ADirect::load, Vec8) is written for
  const int64_t e16 = dt == NMH_DT_BF16_C ? 8 : 4;
  if (lda % e16 || ldw % e16 || ldc % e16) return -2;
  EpiParams ep{C, ldc, bias, act, C2, resid, rowscale, rows_per_scale > 0 ? rows_per_scale : 1, accumulate};
  return k_gemm_nt(dt, A, lda, W, ldw, M, N, K, ep, ST);
}
int nmh_gemm_nt_window_scatter(int dt, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N, int K, void* out, const void* resid, const float* bias,
                               const float* rowscale, int tokens_per_sample, const int* wm, void* stream) {
  CLR();
  REQ(A, W, out, resid, wm);
  if (M <= 0) return 0;
  EpiParams ep{out, N, bias, 0, nullptr, resid, rowscale, tokens_per_sample > 0 ? tokens_per_sample : 1, 0};
  ep.win_on = 1; ep.wm = to_wm(wm);
  return k_gemm_nt(dt, A, lda, W, ldw, M, N, K, ep, ST);
}
int nmh_gemm_tn(int dt, const void* A, int64_t lda, const void* B, int64_t ldb, float* dW, int64_t M, int N, int K, const float* rowscale, int rows_per_scale,
                int omode, int64_t ldo, int p0, int p1, float* dbias, float* ws, int64_t ws_floats, void* stream) {
  CLR();
  REQ(A, B, dW);
  if (M <= 0) return 0;
  TnGeom gm{};
  gm.omode = omode; gm.ldo = ldo; gm.dbias = dbias; gm.ws = ws; gm.ws_floats = ws ? (long)ws_floats : 0;
  if (omode == 2) { gm.Cin = p0; gm.V = (unsigned)p1; gm.dC = make_fdiv(p0); }
  return k_gemm_tn(dt, A, lda, B, ldb, dW, M, N, K, rowscale, rows_per_scale > 0 ? rows_per_scale : 1, gm, ST);
}
int nmh_gemm_nt_plan(int dt, int64_t lda, int64_t ldw, int M, int N, int K, int win_on, int up_k, int ksplit, int batch, int* plan) {
  REQ(plan);
  if ((dt != 0 && dt != NMH_DT_BF16_C) || M <= 0 || N <= 0 || K <= 0 || batch <= 0) return -4;
  return k_gemm_nt_plan(dt, (long)lda, (long)ldw, M, N, K, batch, win_on, up_k, ksplit, plan);
}
int nmh_gemm_nt_plan_table(int* rows, int capacity, int* count) {
  REQ(count);
  *count = k_gemm_nt_plan_table(rows, rows ? capacity : 0);
  return 0;
}
int nmh_gemm_tn_plan(int dt, int64_t lda, int64_t M, int N, int K, int has_rowscale, int rows_per_scale, int64_t ws_floats, int* plan) {
  REQ(plan);
  if ((dt != 0 && dt != NMH_DT_BF16_C) || M <= 0 || N <= 0 || K <= 0) return -4;
  return k_gemm_tn_plan(dt, (long)lda, (long)M, N, K, has_rowscale, rows_per_scale, (long)ws_floats, plan);
}
int nmh_gemm_tn_grouped(int dt, const nmh_tn_problem* probs, int nprob, float* ws, int64_t ws_floats, void* stream) {
  CLR();
  if (nprob <= 0) return 0;
  if (dt != NMH_DT_BF16_C || probs == nullptr) return -4;
  static_assert(sizeof(nmh_tn_problem) == sizeof(TnProblemHost), "descriptor layouts must agree");
  return k_gemm_tn_grouped(reinterpret_cast<const TnProblemHost*>(probs), nprob, ws, ws ? (long)ws_floats : 0, ST);
}
int nmh_gemm_tn_grouped_fg(int dt, const nmh_tn_problem* probs, int nprob, float* ws, int64_t ws_floats, void* stream) {
  CLR();
  if (nprob <= 0) return 0;
  if (dt != NMH_DT_BF16_C || probs == nullptr) return -4;
  return k_gemm_tn_grouped(reinterpret_cast<const TnProblemHost*>(probs), nprob, ws, ws ? (long)ws_floats : 0, ST, true);
}
int nmh_upconv_fwd(int dt, const void* x, const void* Wt, const float* bias, void* cat, int64_t ldc, int B, int v, int k, int Cin, int Cout, void* stream) {
  CLR();
  REQ(x, Wt, cat);
  return k_upconv_fwd(dt, x, Wt, bias, cat, (long)ldc, B, v, k, Cin, Cout, ST);
}
int nmh_upconv_dgrad(int dt, const void* dcat, int64_t ldc, const void* Wd, void* dx, int B, int v, int k, int Cin, int Cout, void* stream) {
  CLR();
  REQ(dcat, Wd, dx);
  return k_upconv_dgrad(dt, dcat, (long)ldc, Wd, dx, B, v, k, Cin, Cout, ST);
}
int nmh_upconv_wgrad(int dt, const void* dcat, int64_t ldc, const void* x, float* dW, float* dbias, int B, int v, int k, int Cin, int Cout, void* stream) {
  CLR();
  REQ(dcat, x, dW);
  return k_upconv_wgrad(dt, dcat, (long)ldc, x, dW, dbias, B, v, k, Cin, Cout, ST);
}
int nmh_conv3d_k3(int dt, const void* X, const void* Wp, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, float* ws, int64_t ws_floats, void* stream) {
  CLR();
  REQ(X, Wp, Y);
  EpiParams ep{Y, Cout, nullptr, 0, nullptr, nullptr, nullptr, 1, accumulate};
  return k_conv3_nt(dt, X, Wp, B, D, H, W, Cin, Cout, ep, ST, ws, ws ? (long)ws_floats : 0);
}
int nmh_conv3d_k3_bias(int dt, const void* X, const void* Wp, const float* bias, void* Y, int B, int D, int H, int W, int Cin, int Cout, void* stream) {
  CLR();
  REQ(X, Wp, bias, Y);
  EpiParams ep{Y, Cout, bias, 0, nullptr, nullptr, nullptr, 1, 0};
  return k_conv3_nt(dt, X, Wp, B, D, H, W, Cin, Cout, ep, ST);
}
int nmh_conv3d_k3_c64(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, double* stats_acc, const float* bias, void* stream) {
  CLR();
  if (!X || !Wk || !Y) return -4;
  return k_conv64(X, Wk, Y, B, D, H, W, Cin, Cout, accumulate, stats_acc, bias, ST);
}
int nmh_conv3d_k3_c64_wgrad(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, int Cin, int Cout, void* stream) {
  CLR();
  if (!dY || !X || !dW || !ws) return -4;
  return k_conv64_wgrad(dY, X, dW, ws, B, D, H, W, Cin, Cout, ST);
}
int64_t nmh_conv3d_k3_c64_wgrad_ws_floats(void) { return (int64_t)k_conv64_wgrad_ws_floats(); }
int64_t nmh_conv3d_k3_c64_pack_numel(int Cin, int Cout) { return (Cin % 64 || Cout % 64) ? -1 : (int64_t)k_conv64_pack_numel(Cin, Cout); }
int nmh_nearest_upsample_add(int dt, const void* coarse, void* fine, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, int C, void* stream) {
  CLR();
  REQ(coarse, fine);
  return k_nearest_up_add(dt, coarse, fine, B, Dc, Hc, Wc, Df, Hf, Wf, C, 0, ST);
}
int nmh_nearest_upsample_add_bwd(int dt, const void* dfine, void* dcoarse, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, int C, void* stream) {
  CLR();
  REQ(dfine, dcoarse);
  return k_nearest_up_add(dt, dcoarse, const_cast<void*>(dfine), B, Dc, Hc, Wc, Df, Hf, Wf, C, 1, ST);
}
int nmh_copy_cols(int dt, const void* src, int64_t lds, void* dst, int64_t ldd, int64_t M, int C, void* stream) {
  CLR();
  REQ(src, dst);
  return k_copy_cols(dt, src, (long)lds, dst, (long)ldd, (long)M, C, ST);
}
int nmh_ndhwc_to_ncdhw(int dt, const void* src, float* dst, int B, int64_t V, int C, void* stream) {
  CLR();
  return k_vc_transpose(dt, src, dst, B, (long)V, C, 0, ST);
}
int nmh_ncdhw_to_ndhwc(int dt, const float* src, void* dst, int B, int64_t V, int C, void* stream) {
  CLR();
  return k_vc_transpose(dt, src, dst, B, (long)V, C, 1, ST);
}
int nmh_conv3d_k3_c48(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int accumulate, double* stats_acc, void* stream) {
  CLR();
  return k_conv48(X, Wk, Y, B, D, H, W, accumulate, stats_acc, ST);
}
int nmh_conv3d_k3_c48_bwd_reduce(const void* dY, const void* Wkd, void* dX, int B, int D, int H, int W, const void* Y1, const float* stats1, float slope,
                                 double* sums, void* stream) {
  CLR();
  REQ(dY, Wkd, dX, Y1, stats1, sums);
  return k_conv48(dY, Wkd, dX, B, D, H, W, 0, sums, ST, Y1, stats1, slope);
}
int nmh_conv48_pack_scaled(const float* W, const float* stats, void* Wk_per_sample, int B, void* stream) {
  CLR();
  REQ(W, stats, Wk_per_sample);
  if (B <= 0) return 0;
  return k_conv48_pack_scaled(W, stats, Wk_per_sample, B, ST);
}
int nmh_conv3d_k3_c48_per_sample(const void* X, const void* Wk_per_sample, void* Y, int B, int D, int H, int W, double* stats_acc, void* stream) {
  CLR();
  REQ(X, Wk_per_sample, Y);
  return k_conv48(X, Wk_per_sample, Y, B, D, H, W, 0, stats_acc, ST, nullptr, nullptr, 0.f, 41L * 3 * 512, 0);
}
int nmh_conv3d_k3_c48_bwd_reduce_centered(const void* dY, const void* Wkd, void* dX, int B, int D, int H, int W, const void* Z, const float* stats1, float slope,
                                          double* sums, void* stream) {
  CLR();
  REQ(dY, Wkd, dX, Z, stats1, sums);
  if (!(slope > 0.f && slope < 1.f)) return -2;
  return k_conv48(dY, Wkd, dX, B, D, H, W, 0, sums, ST, Z, stats1, slope, 0, 1);
}
int nmh_conv3d_k3_c48_wgrad_scaled(const void* dY, const void* Z, const float* stats, float* dW, float* ws, int B, int D, int H, int W, void* stream) {
  CLR();
  REQ(dY, Z, stats, dW, ws);
  return k_conv48_wgrad(dY, Z, dW, ws, B, D, H, W, ST, stats);
}
int nmh_instnorm_bwd_apply_bg_centered(int dt, const void* dout, const void* z, const float* stats, const double* sums, void* dx, int B, int64_t V, int C, float slope, void* stream) {
  CLR();
  REQ(dout, z, stats, sums, dx);
  return k_in_bwd_apply_bg(dt, dout, z, stats, sums, dx, B, (long)V, C, slope, ST, 1);
}
int nmh_conv3d_k3_c48mb(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, void* stream) {
  CLR();
  if (!X || !Wk || !Y) return -4;
  return k_conv48_mb(X, Wk, Y, B, D, H, W, Cin, Cout, accumulate, ST);
}
int nmh_instnorm_finalize(const double* acc, float* stats, int B, int64_t V, int C, float eps, void* stream) {
  CLR();
  return k_in_finalize(0, acc, stats, B, (long)V, C, eps, ST);
}
int nmh_conv3d_k3_c48_wgrad(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, void* stream) {
  CLR();
  return k_conv48_wgrad(dY, X, dW, ws, B, D, H, W, ST);
}
int nmh_conv3d_k3_wgrad_halo(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, int Cin, int Cout, void* stream) {
  CLR();
  return k_conv3_wgrad_halo(dY, X, dW, ws, B, D, H, W, Cin, Cout, ST);
}
int64_t nmh_conv3d_k3_c48_wgrad_ws_floats(void) { return (int64_t)k_conv48_wgrad_ws_floats(); }
int nmh_conv3d_k3_wgrad(int dt, const void* dY, const void* X, float* dW, int B, int D, int H, int W, int Cin, int Cout, void* stream) {
  CLR();
  return k_conv3_tn(dt, dY, X, dW, B, D, H, W, Cin, Cout, ST);
}
int nmh_layernorm_fwd(int dt, int src_mode, const void* x, void* out, const float* gamma, const float* beta, float eps, float* mean, float* rstd, int64_t rows, int C,
                      const int* wm, const float* pos, const unsigned char* mask, const float* mask_token, int64_t tokens_per_sample, void* stream) {
  CLR();
  if (rows <= 0) return 0;
  LnArgs a{dt, src_mode, x, out, gamma, beta, eps, mean, rstd, (long)rows, C, to_wm(wm), pos, mask, mask_token, (long)(tokens_per_sample > 0 ? tokens_per_sample : 1), nullptr};
  return k_ln_fwd(a, ST);
}
int nmh_layernorm_fwd_window_tokens(int dt, const void* x, void* out_window, void* out_tokens, const float* gamma, const float* beta, float eps, float* mean, float* rstd,
                                    int64_t rows, int C, const int* wm, void* stream) {
  CLR();
  REQ(x, out_window, out_tokens, gamma, beta, mean, rstd, wm);
  if (rows <= 0) return 0;
  LnArgs a{dt, 1, x, out_window, gamma, beta, eps, mean, rstd, (long)rows, C, to_wm(wm), nullptr, nullptr, nullptr, 1, out_tokens};
  return k_ln_fwd(a, ST);
}
int nmh_layernorm_bwd(int dt, int src_mode, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres, void* dx,
                      float* dgamma, float* dbeta, int64_t rows, int C, const int* wm, const unsigned char* mask, float* dmask_token, int64_t tokens_per_sample,
                      void* dyw, const float* dyw_scale, void* stream) {
  CLR();
  if (rows <= 0) return 0;
  LnBwdArgs a{dt, src_mode, dy, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, (long)rows, C, to_wm(wm), mask, dmask_token, (long)(tokens_per_sample > 0 ? tokens_per_sample : 1),
              dyw, dyw_scale, 0, nullptr};
  return k_ln_bwd(a, ST);
}
int64_t nmh_layernorm_bwd_partial_rows(int64_t rows, int C) { return rows > 0 && C > 0 && C % 8 == 0 ? (int64_t)k_ln_bwd_blocks((long)rows, C) : 0; }
int nmh_layernorm_bwd_deferred(int dt, int src_mode, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres, void* dx,
                               float* partials, int64_t rows, int C, const int* wm, void* dyw, const float* dyw_scale, int64_t tokens_per_sample, void* stream) {
  CLR();
  REQ(dy, x, gamma, mean, rstd, dx, partials);
  if (rows <= 0) return 0;
  LnBwdArgs a{dt, src_mode, dy, x, gamma, mean, rstd, dres, dx, nullptr, nullptr, (long)rows, C, to_wm(wm), nullptr, nullptr, (long)(tokens_per_sample > 0 ? tokens_per_sample : 1),
              dyw, dyw_scale, 0, partials};
  return k_ln_bwd(a, ST);
}
int nmh_layernorm_param_grad_reduce(const nmh_ln_reduce_item* items, int n, void* stream) {
  CLR();
  static_assert(sizeof(nmh_ln_reduce_item) == sizeof(LnReduceItem), "layout");
  if (n <= 0) return 0;
  REQ(items);
  return k_ln_param_reduce(reinterpret_cast<const LnReduceItem*>(items), n, ST);
}
int64_t nmh_cconv_pack_numel(void) { return (int64_t)k_cconv_pack_numel(); }
int64_t nmh_cconv_pack_ws_floats(void) { return (int64_t)k_cconv_pack_ws_floats(); }
int nmh_cconv_pack(const float* Wt, const float* W1, const float* bt, void* Wcp, float* delta, float* ws, void* stream) {
  CLR();
  REQ(Wt, W1, bt, Wcp, delta, ws);
  return k_cconv_pack(Wt, W1, bt, Wcp, delta, ws, ST);
}
int nmh_cconv_fwd(const void* x, const void* Wcp, const float* delta, void* y1, int B, int v, double* stats_acc, void* stream) {
  CLR();
  REQ(x, Wcp, delta, y1);
  if (B <= 0 || v <= 0) return 0;
  return k_cconv_fwd(x, Wcp, delta, y1, B, v, stats_acc, ST);
}
int nmh_cconv_pack_centered(const float* Wt, const float* W1, const float* bt, void* Wcp, float* delta, float* ws, float* mean_table, void* stream) {
  CLR();
  REQ(Wt, W1, bt, Wcp, delta, ws, mean_table);
  return k_cconv_pack(Wt, W1, bt, Wcp, delta, ws, ST, mean_table);
}
int nmh_cconv_output_mean(const void* x, const float* mean_table, const float* delta, double* class_sums, float* mean, int B, int v, void* stream) {
  CLR();
  REQ(x, mean_table, delta, class_sums, mean);
  if (B <= 0 || v <= 0) return 0;
  return k_cconv_mean(x, mean_table, delta, class_sums, mean, B, v, ST);
}
int nmh_cconv_fwd_centered(const void* x, const void* Wcp, const float* delta, const float* mean, float slope, void* z, int B, int v, double* stats_acc, void* stream) {
  CLR();
  REQ(x, Wcp, delta, mean, z);
  if (B <= 0 || v <= 0) return 0;
  if (!(slope > 0.f && slope < 1.f)) return -2;
  return k_cconv_fwd(x, Wcp, delta, z, B, v, stats_acc, ST, mean, slope);
}
int64_t nmh_cconv_wgrad_ws_floats(void) { return (int64_t)k_cconv_wgrad_ws_floats(); }
int nmh_cconv_wgrad(const void* x, const void* dy1, const float* pack_ws, const float* bt, float* dW1, float* dWt, float* dbt, float* ws, int B, int v, int phase, void* stream) {
  CLR();
  REQ(x, dy1, pack_ws, bt, dW1, ws);
  if (B <= 0 || v <= 0) return 0;
  if (phase < 0 || phase > 2) return -1;
  return k_cconv_wgrad(x, dy1, pack_ws, bt, dW1, dWt, dbt, ws, B, v, phase, ST);
}
int64_t nmh_cconv_dgrad_pack_numel(void) { return (int64_t)k_cconv_dpack_numel(); }
int nmh_cconv_dgrad_pack(const void* Wcp, void* Wdp, void* stream) {
  CLR();
  REQ(Wcp, Wdp);
  return k_cconv_dpack(Wcp, Wdp, ST);
}
int nmh_cconv_dgrad(const void* dy1, const void* Wdp, const void* add, void* dx, int B, int v, void* stream) {
  CLR();
  REQ(dy1, Wdp, dx);
  if (B <= 0 || v <= 0) return 0;
  return k_cconv_dgrad(dy1, Wdp, add, dx, B, v, ST);
}
int64_t nmh_upconv4_pack_numel(void) { return (int64_t)k_upconv4_pack_numel(); }
int nmh_upconv4_pack(const float* pack_ws, void* Wup, void* stream) {
  CLR();
  REQ(pack_ws, Wup);
  return k_upconv4_pack(pack_ws, Wup, ST);
}
int nmh_upconv4_fwd(const void* x, const void* Wup, const float* bt, void* u, int B, int v, void* stream) {
  CLR();
  REQ(x, Wup, bt, u);
  if (B <= 0 || v <= 0) return 0;
  return k_upconv4_fwd(x, Wup, bt, u, B, v, ST);
}
int nmh_mlp_fused_supported(int C) { return k_mlp_fused_supported(C); }
int nmh_mlp_fused_fwd(const void* x1, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2T, const float* b2, const float* rowscale,
                      int rows_per_scale, void* x2, float* mean, float* rstd, int64_t M, int C, float eps, void* stream) {
  CLR();
  REQ(x1, gamma, beta, W1, b1, W2T, b2, x2);
  if (M <= 0) return 0;
  return k_mlp_fused_fwd(x1, gamma, beta, W1, b1, W2T, b2, rowscale, rows_per_scale, x2, mean, rstd, (long)M, C, eps, ST);
}
int nmh_mlp_fused_bwd(const void* x1, const void* dx2, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2T, const float* rowscale,
                      int rows_per_scale, void* dx1, void* x1n, void* hact, void* dh, float* dgamma, float* dbeta, void* dyw, const float* dyw_scale, const int* wm,
                      int64_t M, int C, float eps, void* stream) {
  CLR();
  REQ(x1, dx2, gamma, beta, W1, b1, W2T, dx1, x1n, hact, dh, dgamma, dbeta);
  if (M <= 0) return 0;
  if (dyw && !wm) return -4;
  const WinMap w = to_wm(wm);
  return k_mlp_fused_bwd(x1, dx2, gamma, beta, W1, b1, W2T, rowscale, rows_per_scale, dx1, x1n, hact, dh, dgamma, dbeta, dyw, dyw_scale, wm ? &w : nullptr, (long)M, C, eps, ST);
}
int nmh_swin_supported(int C) { return k_swin_supported(C); }
int64_t nmh_swin_stream_numel(int type, int C) { return (int64_t)k_swin_stream_numel(type, C); }
int nmh_swin_pack(const nmh_swin_pack_item* items, int n, void* stream) {
  CLR();
  if (n <= 0) return 0;
  REQ(items);
  static_assert(sizeof(nmh_swin_pack_item) == sizeof(SwinPackItem), "descriptor layouts must agree");
  return k_swin_pack(reinterpret_cast<const SwinPackItem*>(items), n, ST);
}
int nmh_swin_attn_fwd(const void* x, const float* gamma, const float* beta, const void* wstream, const float* bqkv, const float* bias_table, const float* bproj,
                      const float* rowscale, int rows_per_scale, void* xnw, float* mean, float* rstd, void* qkv, void* o, float* lse, void* x1, const int* wm, int C,
                      float eps, int token_saves, void* stream) {
  CLR();
  REQ(x, gamma, beta, wstream, bqkv, bias_table, bproj, xnw, mean, rstd, qkv, o, lse, x1, wm);
  return k_swin_attn_fwd(x, gamma, beta, wstream, bqkv, bias_table, bproj, rowscale, rows_per_scale, xnw, mean, rstd, qkv, o, lse, x1, to_wm(wm), C, eps, token_saves, ST);
}
int nmh_swin_mlp_fwd(const void* x1, const float* gamma, const float* beta, const void* wstream, const float* b1, const float* b2, const float* rowscale, int rows_per_scale,
                     void* x2, void* x1n, void* hp, void* hact, float* mean, float* rstd, int64_t M, int C, float eps, void* split_ws, int64_t split_ws_bytes,
                     void* stream) {
  CLR();
  REQ(x1, gamma, beta, wstream, b1, b2, x2, x1n, hp, mean, rstd);
  if (M <= 0) return 0;
  if ((long)M * 4 * C >= (1L << 31)) return -2;
  return k_swin_mlp_fwd(x1, gamma, beta, wstream, b1, b2, rowscale, rows_per_scale, x2, x1n, hp, hact, mean, rstd, (long)M, C, eps, split_ws, (long)split_ws_bytes, ST);
}
int64_t nmh_swin_mlp_split_ws_bytes(int64_t M, int C) { return k_swin_mlp_split_ws_bytes((long)M, C); }
int nmh_window_scatter_residual(int dt, const void* yw, const void* x, void* out, const float* rowscale, int C, const int* wm, void* stream) {
  CLR();
  return k_window_scatter_residual(dt, yw, x, out, rowscale, C, to_wm(wm), ST);
}
int nmh_window_gather_scale(int dt, const void* dx, void* dyw, const float* rowscale, int C, const int* wm, void* stream) {
  CLR();
  return k_window_gather_scale(dt, dx, dyw, rowscale, C, to_wm(wm), ST);
}
int nmh_window_attn_fwd(int dt, const void* qkv, const float* bias_table, void* out, float* lse, int heads, int C, const int* wm, void* stream) {
  CLR();
  return k_attn_fwd(dt, qkv, bias_table, out, lse, heads, C, to_wm(wm), ST);
}
int nmh_window_attn_fwd_tokens(int dt, const void* qkv, const float* bias_table, void* out_tok, float* lse, int heads, int C, const int* wm, void* stream) {
  CLR();
  REQ(qkv, bias_table, out_tok, lse, wm);
  return k_attn_fwd(dt, qkv, bias_table, out_tok, lse, heads, C, to_wm(wm), ST, 1);
}
int nmh_window_attn_bwd(int dt, const void* qkv, const float* bias_table, const void* dout, const float* lse, void* dqkv, float* dbias_table, int heads, int C,
                        const int* wm, void* stream) {
  CLR();
  return k_attn_bwd(dt, qkv, bias_table, dout, lse, dqkv, dbias_table, heads, C, to_wm(wm), ST);
}
int nmh_window_attn_bwd_tokens(int dt, const void* qkv, const float* bias_table, const void* dout_tok, const float* lse, void* dqkv_tok, void* dqkv_pad, float* dbias_table,
                               int heads, int C, const int* wm, void* stream) {
  CLR();
  REQ(qkv, bias_table, dout_tok, lse, dqkv_tok, dqkv_pad, dbias_table, wm);
  return k_attn_bwd(dt, qkv, bias_table, dout_tok, lse, dqkv_pad, dbias_table, heads, C, to_wm(wm), ST, dqkv_tok);
}
int nmh_window_pad_rows_colsum(int dt, const void* x, int N, const int* wm, float* out, void* stream) {
  CLR();
  REQ(x, wm, out);
  return k_attn_pad_rows_colsum(dt, x, N, to_wm(wm), out, ST);
}
int nmh_window_pad_rows_colsum_grouped(int dt, const void* const* xs, float* const* outs, int n, int N, const int* wm, void* stream) {
  CLR();
  REQ(xs, outs, wm);
  return k_attn_pad_rows_colsum_grouped(dt, xs, outs, n, N, to_wm(wm), ST);
}
int nmh_instnorm_stats(int dt, const void* x, float* stats, double* scratch, int B, int64_t V, int C, float eps, void* stream) {
  CLR();
  return k_in_stats(dt, x, stats, scratch, B, (long)V, C, eps, ST);
}
int nmh_instnorm_apply(int dt, const void* x, const float* stats, const void* r, const float* stats_r, int rmode, void* out, int B, int64_t V, int C, float slope, void* stream) {
  CLR();
  return k_in_apply(dt, x, stats, r, stats_r, rmode, out, B, (long)V, C, slope, ST);
}
int nmh_instnorm_bwd_reduce(int dt, const void* dout, const void* out, const void* x, const float* stats, const void* r, const float* stats_r, int rmode, double* sums,
                            double* sums_r, int B, int64_t V, int C, float slope, void* stream) {
  CLR();
  return k_in_bwd_reduce(dt, dout, out, x, stats, r, stats_r, rmode, sums, sums_r, B, (long)V, C, slope, ST);
}
int nmh_instnorm_bwd_apply(int dt, const void* dout, const void* out, const void* x, const float* stats, const double* sums, const void* r, const float* stats_r,
                           const double* sums_r, int rmode, void* dx, void* dr, int dr_accumulate, int B, int64_t V, int C, float slope, void* stream) {
  CLR();
  return k_in_bwd_apply(dt, dout, out, x, stats, sums, r, stats_r, sums_r, rmode, dx, dr, dr_accumulate, B, (long)V, C, slope, ST);
}
int nmh_instnorm_bwd_apply_bg(int dt, const void* dout, const void* x, const float* stats, const double* sums, void* dx, int B, int64_t V, int C, float slope, void* stream) {
  CLR();
  REQ(dout, x, stats, sums, dx);
  return k_in_bwd_apply_bg(dt, dout, x, stats, sums, dx, B, (long)V, C, slope, ST);
}
int nmh_patch_embed_gather(int dt, const float* x, void* A, int B, int R, void* stream) {
  CLR(); return k_embed_gather(dt, x, A, B, R, ST); }
int nmh_patch_embed_kept_rows(const unsigned char* mask, int n, int cap, int* rowmap, void* stream) {
  CLR();
  REQ(mask, rowmap);
  return k_mask_rowmap(mask, n, cap, rowmap, ST);
}
int nmh_patch_embed_gather_kept(int dt, const float* x, void* A, int B, int R, const int* rowmap, int64_t cap_rows, void* stream) {
  CLR();
  REQ(x, A, rowmap);
  return k_embed_gather(dt, x, A, B, R, ST, rowmap, (long)cap_rows);
}
int nmh_patch_embed_norm_fwd_kept(int dt, const void* y0, void* tok, const float* gamma, const float* beta, float eps, float* mean, float* rstd, int64_t rows, int C, const float* pos,
                                  const unsigned char* mask, const float* mask_token, int64_t tokens_per_sample, const int* rowmap, int64_t cap_rows, void* stream) {
  CLR();
  REQ(y0, tok, gamma, beta, mean, rstd, mask, mask_token, rowmap);
  if (rows <= 0) return 0;
  if (tokens_per_sample <= 0 || rows % tokens_per_sample || cap_rows <= 0) return -2;
  LnArgs a{dt, 0, y0, tok, gamma, beta, eps, mean, rstd, (long)rows, C, WinMap{}, pos, mask, mask_token, (long)tokens_per_sample, nullptr, rowmap, (long)cap_rows};
  return k_ln_fwd(a, ST);
}
int nmh_patch_embed_norm_bwd_kept(int dt, const void* dtok, const void* y0, const float* gamma, const float* mean, const float* rstd, void* dy0, float* dgamma, float* dbeta,
                                  int64_t rows, int C, const unsigned char* mask, float* dmask_token, int64_t tokens_per_sample, const int* rowmap, int64_t cap_rows, void* stream) {
  CLR();
  REQ(dtok, y0, gamma, mean, rstd, dy0, dgamma, dbeta, mask, dmask_token, rowmap);
  if (rows <= 0) return 0;
  if (tokens_per_sample <= 0 || rows % tokens_per_sample || cap_rows <= 0) return -2;
  LnBwdArgs a{dt, 0, dtok, y0, gamma, mean, rstd, nullptr, dy0, dgamma, dbeta, (long)rows, C, WinMap{}, mask, dmask_token, (long)tokens_per_sample, nullptr, nullptr, 0, nullptr,
              rowmap, (long)cap_rows};
  return k_ln_bwd(a, ST);
}
int nmh_block0_supported(int C) { return k_b0_supported(C); }
int nmh_block0_window_rows(const unsigned char* mask, int g, int cap_windows, int* rowmap, int* wmap, void* stream) {
  CLR();
  REQ(mask, rowmap, wmap);
  return k_b0_rowmap(mask, g, cap_windows, rowmap, wmap, ST);
}
int nmh_block0_embed_norm_fwd(int dt, const void* y0, void* out, const float* gamma, const float* beta, float eps, float* mean, float* rstd, const float* pos,
                              const float* mask_token, const int* wmap, int B, int g, int cap_windows, int C, void* stream) {
  CLR();
  REQ(y0, out, gamma, beta, mean, rstd, mask_token, wmap);
  return k_b0_ln_fwd(dt, y0, out, gamma, beta, eps, mean, rstd, pos, mask_token, wmap, B, g, cap_windows, C, ST);
}
int nmh_block0_embed_norm_bwd(int dt, const void* dx0, const void* y0, const float* gamma, const float* mean, const float* rstd, void* dy0, float* dgamma, float* dbeta,
                              float* dmask_token, float* partials, int64_t partial_floats, const int* wmap, int B, int g, int cap_windows, int C, void* stream) {
  CLR();
  REQ(dx0, y0, gamma, mean, rstd, dy0, dgamma, dbeta, dmask_token, partials, wmap);
  return k_b0_ln_bwd(dt, dx0, y0, gamma, mean, rstd, dy0, dgamma, dbeta, dmask_token, partials, (long)partial_floats, wmap, B, g, cap_windows, C, ST);
}
int nmh_block0_expand(int dt, const void* yc, void* y, const int* wmap, int B, int g, int cap_windows, int C, void* stream) {
  CLR();
  REQ(yc, y, wmap);
  return k_b0_expand(dt, yc, y, wmap, B, g, cap_windows, C, ST);
}
int nmh_block0_reduce(int dt, const void* dy, void* dyc, const int* wmap, int B, int g, int cap_windows, int C, void* stream) {
  CLR();
  REQ(dy, dyc, wmap);
  return k_b0_reduce(dt, dy, dyc, wmap, B, g, cap_windows, C, ST);
}
int nmh_upconv_shuffle_fwd(int dt, const void* upre, const float* bias, const void* skip, void* out, int B, int v, int k, int Cout, void* stream) {
  CLR();
  return k_up_cat_fwd(dt, upre, bias, skip, out, B, v, k, Cout, ST);
}
int nmh_upconv_shuffle_bwd(int dt, const void* dcat, void* dupre, void* dskip, float* dbias, int B, int v, int k, int Cout, int has_skip, void* stream) {
  CLR();
  return k_up_cat_bwd(dt, dcat, dupre, dskip, dbias, B, v, k, Cout, has_skip, ST);
}
int nmh_mae_loss_fwd(int dt, const void* d0, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R,
                     int Cd, double* sums, float* losses, float* pred, float* dpred, void* stream) {
  CLR();
  LossArgs a{dt, d0, Wout, bout, target, extents, tokmask, B, R, Cd, sums, pred, dpred};
  int rc = k_loss_fwd(a, ST);
  if (rc) return rc;
  return k_loss_finalize(sums, losses, ST);
}
int nmh_mae_loss_bwd(int dt, const void* d0, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R,
                     int Cd, const double* sums, void* dd0, void* dpred8, float* dWout, float* dbout, void* stream) {
  CLR();
  LossArgs a{dt, d0, Wout, bout, target, extents, tokmask, B, R, Cd, const_cast<double*>(sums), nullptr, nullptr};
  (void)dpred8;  // kept in the ABI for layout stability; the head weight gradient is now fused into the kernel
  return k_loss_bwd(a, dd0, dWout, dbout, ST);
}
int nmh_mae_tail_fwd(int dt, const void* y, const float* stats, const void* r, void* d0, const float* Wout, const float* bout, const float* target, const int* extents,
                     const unsigned char* tokmask, int B, int R, int C, double* sums, float* losses, float* pred, float* dpred, float slope, double* bwd_sums,
                     unsigned char* sign_mask, void* stream) {
  CLR();
  LossArgs a{dt, nullptr, Wout, bout, target, extents, tokmask, B, R, C, sums, pred, dpred, bwd_sums, sign_mask};
  int rc = k_tail_fwd(a, y, stats, r, d0, slope, ST);
  if (rc) return rc;
  return k_loss_finalize(sums, losses, ST);
}
int64_t nmh_tail_residual_pack_numel(void) { return (int64_t)k_tail_r_pack_numel(); }
int nmh_tail_residual_pack(const float* pack_ws, void* Wr, void* stream) {
  CLR();
  REQ(pack_ws, Wr);
  return k_tail_r_pack(pack_ws, Wr, ST);
}
int nmh_mae_tail_fwd_from_coarse(int dt, const void* y, const float* stats, const void* xcoarse, const void* Wr, const float* bt, const float* Wout, const float* bout,
                                 const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int C, double* sums, float* losses, float* pred,
                                 float* dpred, float slope, double* bwd_sums, unsigned char* sign_mask, void* stream) {
  CLR();
  REQ(y, stats, xcoarse, Wr, bt, Wout, bout, target, extents, tokmask, sums, losses, dpred, bwd_sums, sign_mask);
  LossArgs a{dt, nullptr, Wout, bout, target, extents, tokmask, B, R, C, sums, pred, dpred, bwd_sums, sign_mask};
  int rc = k_tail_fwd_coarse(a, y, stats, xcoarse, Wr, bt, slope, ST);
  if (rc) return rc;
  return k_loss_finalize(sums, losses, ST);
}
int nmh_mae_tail_fwd_from_coarse_box(int dt, const void* y, const float* stats, const void* xcoarse, const void* Wr, const float* bt, const float* Wout, const float* bout,
                                     const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int C, double* sums, float* losses, float* pred,
                                     float* dpred, float slope, double* bwd_sums, unsigned char* sign_mask, void* stream) {
  CLR();
  REQ(y, stats, xcoarse, Wr, bt, Wout, bout, target, extents, tokmask, sums, losses, dpred, bwd_sums, sign_mask);
  if (pred) return -4;   // the box walk leaves the padding unwritten
  LossArgs a{dt, nullptr, Wout, bout, target, extents, tokmask, B, R, C, sums, nullptr, dpred, bwd_sums, sign_mask};
  int rc = k_tail_fwd_coarse(a, y, stats, xcoarse, Wr, bt, slope, ST, true);
  if (rc) return rc;
  return k_loss_finalize(sums, losses, ST);
}
int nmh_mae_tail_bwd_box(int dt, const void* y, const float* stats, const float* dpred, const double* loss_sums, const float* Wout, double* in_sums, void* dy, void* dr,
                         float slope, float* dWout, float* dbout, int B, int R, int C, const double* bwd_sums, const unsigned char* sign_mask, const int* extents,
                         void* stream) {
  CLR();
  REQ(y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, dWout, dbout, bwd_sums, sign_mask, extents);
  return k_tail_bwd(dt, nullptr, nullptr, y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, slope, dWout, dbout, B, (long)R * R * R, C, bwd_sums, ST, sign_mask, extents, R);
}
int nmh_mae_tail_bwd(int dt, const void* d0, const void* r, const void* y, const float* stats, const float* dpred, const double* loss_sums, const float* Wout, double* in_sums,
                     void* dy, void* dr, float slope, float* dWout, float* dbout, int B, int64_t V, int C, const double* bwd_sums, const unsigned char* sign_mask,
                     void* stream) {
  CLR();
  return k_tail_bwd(dt, d0, r, y, stats, dpred, loss_sums, Wout, in_sums, dy, dr, slope, dWout, dbout, B, (long)V, C, bwd_sums, ST, sign_mask);
}
int nmh_grid_prepare(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, void* stream) {
  CLR();
  return k_grid_prepare(src_u8, src, W, L, H, dst, R, flags, ST);
}
int nmh_labels_prepare(int dt, const void* src, int W, int L, int H, float* dst, int R, int flags, void* stream) {
  CLR();
  REQ(src, dst);
  return k_labels_prepare(dt, src, W, L, H, dst, R, flags, ST);
}
int nmh_grid_prepare_rs(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, float angle, float scale, void* stream) {
  CLR();
  REQ(src, dst);
  return k_grid_prepare_rs(src_u8, src, W, L, H, dst, R, flags, angle, scale, ST);
}
int nmh_boxes_augment(const float* boxes, float* out, int cols, int total_rows, int n_scenes, const int* itab, const float* ftab, void* stream) {
  CLR();
  if (total_rows <= 0) return total_rows < 0 ? -4 : 0;
  REQ(boxes, out, itab, ftab);
  return k_boxes_augment(boxes, out, cols, total_rows, n_scenes, itab, ftab, ST);
}
int nmh_bias_grad(int dt, const void* dY, float* db, int64_t M, int N, const float* rowscale, int rows_per_scale, void* stream) {
  CLR();
  if (M <= 0) return 0;
  return k_bias_grad(dt, dY, db, (long)M, N, rowscale, rows_per_scale > 0 ? rows_per_scale : 1, ST);
}
int nmh_add(int dt, const void* a, const void* b, void* out, int64_t n, void* stream) {
  CLR();
  if (n <= 0) return 0;
  if (!a || !b || !out) return -4;
  return k_add(dt, out, a, b, (long)n, ST);
}
int nmh_add_inplace(int dt, void* a, const void* b, int64_t n, void* stream) {
  CLR(); return k_add_inplace(dt, a, b, (long)n, ST); }
int nmh_grid_to_cl8(int dt, const float* grid, void* out, int B, int64_t V, void* stream) {
  CLR();
  if (!grid || !out) return -4;
  return k_grid_to_cl8(dt, grid, out, B, (long)V, ST);
}
int nmh_head_upsample_fwd(int dt, const void* y, float* pred, int B, int Co, int Cp, int R, int Ro, float inv_scale, void* stream) {
  CLR();
  if (!y || !pred || Co > Cp) return -4;
  return k_cl_to_ncdhw_up(dt, y, pred, B, Co, Cp, R, Ro, inv_scale, ST);
}
int nmh_head_upsample_bwd(int dt, const float* dpred, void* g, int B, int Co, int Cp, int R, int Ro, float inv_scale, void* stream) {
  CLR();
  if (!dpred || !g || Co > Cp) return -4;
  return k_ncdhw_up_adjoint(dt, dpred, g, B, Co, Cp, R, Ro, inv_scale, ST);
}
int nmh_add_cols_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream) {
  CLR();
  if (!src || !dst) return -4;
  return k_add_cols_f32(src, (long)lds, dst, (long)ldd, (long)M, C, ST);
}
int nmh_voxel_sr_loss_fwd(const float* pred, const float* target, int B, int64_t V, double* sums, float* loss, void* stream) {
  CLR();
  if (!pred || !target || !sums || !loss) return -4;
  return k_sr_loss_fwd(pred, target, B, (long)V, sums, loss, ST);
}
int nmh_voxel_sr_loss_bwd(const float* pred, const float* target, int B, int64_t V, const double* sums, float gscale, float* dpred, void* stream) {
  CLR();
  if (!pred || !target || !sums || !dpred) return -4;
  return k_sr_loss_bwd(pred, target, B, (long)V, sums, gscale, dpred, ST);
}
int nmh_masked_ce_fwd(const float* logits, const float* labels, const float* class_weights, int B, int K, int64_t V, double* sums, double* iou_sums, float* out, void* stream) {
  CLR();
  if (!logits || !labels || !sums || !iou_sums || !out) return -4;
  return k_masked_ce_fwd(logits, labels, class_weights, B, K, (long)V, sums, iou_sums, out, ST);
}
int nmh_masked_ce_bwd(const float* logits, const float* labels, const float* class_weights, int B, int K, int64_t V, const double* sums, float gscale, float* dlogits, void* stream) {
  CLR();
  if (!logits || !labels || !sums || !dlogits) return -4;
  return k_masked_ce_bwd(logits, labels, class_weights, B, K, (long)V, sums, gscale, dlogits, ST);
}
int nmh_sem_eval(const float* logits, const float* labels, const float* class_weights, int B, int K, int64_t V, double* fpart, int64_t* ipart, float* out,
                 int64_t* counts, int64_t* pred_vis, int64_t* target_vis, int64_t* totals, void* stream) {
  CLR();
  REQ(logits, labels, fpart, ipart, out, counts, pred_vis, target_vis);
  return k_sem_eval(logits, labels, class_weights, B, K, (long)V, fpart, (long long*)ipart, out, (long long*)counts, (long long*)pred_vis, (long long*)target_vis,
                    (long long*)totals, ST);
}
int nmh_sem_label_counts(int dt, const void* output, const void* target, int64_t n, int K, int64_t* ipart, int64_t* counts, void* stream) {
  CLR();
  REQ(ipart, counts);
  if (n > 0) REQ(output, target);
  return k_sem_label_counts(dt, output, target, (long)n, K, (long long*)ipart, (long long*)counts, ST);
}
int nmh_roi_align_rotated_3d_fwd(int layout, int dt, const void* input, const float* rois, void* out, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH,
                                 float spatial_scale, int sampling_ratio, void* stream) {
  CLR();
  if (N <= 0) return 0;
  REQ(input, rois, out);
  return k_roi_align_rotated_3d_fwd(layout, dt, input, rois, out, N, B, W, L, H, C, PW, PL, PH, spatial_scale, sampling_ratio, ST);
}
int nmh_roi_align_rotated_3d_bwd(int layout, int dt, const void* dout, const float* rois, float* dinput, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH,
                                 float spatial_scale, int sampling_ratio, void* stream) {
  CLR();
  if (N <= 0) return 0;
  REQ(dout, rois, dinput);
  return k_roi_align_rotated_3d_bwd(layout, dt, dout, rois, dinput, N, B, W, L, H, C, PW, PL, PH, spatial_scale, sampling_ratio, ST);
}
int nmh_sort_vertices(const float* vertices, const unsigned char* mask, const int* num_valid, int* idx, int B, int N, int M, void* stream) {
  CLR();
  if (B <= 0 || N <= 0) return 0;
  REQ(vertices, mask, num_valid, idx);
  return k_sort_vertices(vertices, mask, num_valid, idx, B, N, M, ST);
}
int nmh_obb_iou_fwd(int mode, const float* box1, const float* box2, int64_t npairs, float* iou, float* u3d, float* z_range, float* loss, float* w_c, float* h_c, float* corners1,
                    float* corners2, void* stream) {
  CLR();
  if (mode < 0 || mode > 4 || npairs < 0) return -4;
  if (npairs == 0) return 0;
  REQ(box1, box2, iou);
  if (mode != 0 && !loss) return -4;
  return k_obb_iou_fwd(mode, box1, box2, (long)npairs, iou, u3d, z_range, loss, w_c, h_c, corners1, corners2, ST);
}
int nmh_obb_iou_bwd(int mode, const float* box1, const float* box2, int64_t npairs, const float* g_iou, const float* g_u3d, const float* g_loss, int g_one, float* dbox1,
                    float* dbox2, void* stream) {
  CLR();
  if (mode < 0 || mode > 4 || npairs < 0 || g_one < 0 || g_one > 7) return -4;
  if (npairs == 0 || (!dbox1 && !dbox2)) return 0;
  REQ(box1, box2);
  return k_obb_iou_bwd(mode, box1, box2, (long)npairs, g_iou, g_u3d, g_loss, g_one, dbox1, dbox2, ST);
}
int nmh_obb_iou_pairwise(int ncols, const float* boxes1, const float* boxes2, int N, int M, float* iou, void* stream) {
  CLR();
  if ((ncols != 6 && ncols != 7) || N < 0 || M < 0) return -4;
  if (N == 0 || M == 0) return 0;
  REQ(boxes1, boxes2, iou);
  return k_obb_iou_pairwise(ncols, boxes1, boxes2, N, M, iou, ST);
}
int nmh_obb_nms_mask(int ncols, const float* boxes, const int* category, int N, float iou_threshold, uint64_t* mask, void* stream) {
  CLR();
  if ((ncols != 6 && ncols != 7) || N < 0 || N > NMH_OBB_NMS_MAX) return -4;
  if (N == 0) return 0;
  REQ(boxes, mask);
  return k_obb_nms_mask(ncols, boxes, category, N, iou_threshold, (unsigned long long*)mask, ST);
}
int nmh_obb_nms_scan(const uint64_t* mask, int N, int* keep, int* count, void* stream) {
  CLR();
  if (N < 0 || N > NMH_OBB_NMS_MAX) return -4;
  REQ(count);
  if (N == 0) return k_fill_f32((float*)count, 0.f, 1, ST);   // an int 0 has the bits of 0.f
  REQ(mask, keep);
  return k_obb_nms_scan((const unsigned long long*)mask, N, keep, count, ST);
}
int64_t nmh_fcos_num_blocks(int nlevels, const int* level_dims, int N) { return k_fcos_num_blocks(nlevels, level_dims, N); }
int nmh_fcos_assign(int nlevels, const int* level_dims, int N, int ncols, const float* boxes, const int* box_offsets, const int* grid_sizes, const unsigned char* const* masks, float radius,
                    int norm_targets, float* labels, float* targets, int* gt_index, float* ctr_targets, unsigned char* valid, float* partials, float* scalars, void* stream) {
  CLR();
  REQ(level_dims, box_offsets, labels, targets, gt_index, ctr_targets, valid, partials, scalars);
  return k_fcos_assign(nlevels, level_dims, N, ncols, boxes, box_offsets, grid_sizes, masks, radius, norm_targets, labels, targets, gt_index, ctr_targets, valid, partials, scalars, ST);
}
int nmh_fcos_focal_fwd(int nlevels, const int* level_dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world,
                       float* partials, float* loss, void* stream) {
  CLR();
  REQ(level_dims, cls, labels, valid, scalars, partials, loss);
  return k_fcos_focal_fwd(nlevels, level_dims, N, cls, labels, valid, scalars, world, partials, loss, ST);
}
int nmh_fcos_focal_bwd(int nlevels, const int* level_dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world,
                       const float* g_loss, float* const* dcls, void* stream) {
  CLR();
  REQ(level_dims, cls, labels, valid, scalars, dcls);
  return k_fcos_focal_bwd(nlevels, level_dims, N, cls, labels, valid, scalars, world, g_loss, dcls, ST);
}
int nmh_fcos_pos_fwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels,
                     const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss,
                     void* stream) {
  CLR();
  REQ(level_dims, reg, ctr, labels, targets, ctr_targets, valid, scalars, partials, reg_loss, ctr_loss);
  return k_fcos_pos_fwd(nlevels, level_dims, N, ncols, loss_type, add_l1, reg, ctr, labels, targets, ctr_targets, valid, scalars, world, partials, reg_loss, ctr_loss, ST);
}
int nmh_fcos_pos_bwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels,
                     const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr,
                     float* const* dreg, float* const* dctr, void* stream) {
  CLR();
  REQ(level_dims, reg, ctr, labels, targets, ctr_targets, valid, scalars, dreg, dctr);
  return k_fcos_pos_bwd(nlevels, level_dims, N, ncols, loss_type, add_l1, reg, ctr, labels, targets, ctr_targets, valid, scalars, world, g_reg, g_ctr, dreg, dctr, ST);
}
int nmh_fcos_pos2d_fwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr,
                       const float* labels, const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, float* partials,
                       float* reg_loss, float* ctr_loss, void* stream) {
  CLR();
  REQ(level_dims, reg, ctr, labels, targets, ctr_targets, valid, scalars, partials, reg_loss, ctr_loss);
  if (!(proj2d_weight >= 0.f) || ncols != 8) return -4;
  return k_fcos_pos2d_fwd(nlevels, level_dims, N, ncols, loss_type, add_l1, proj2d_weight, reg, ctr, labels, targets, ctr_targets, valid, scalars, world, partials, reg_loss, ctr_loss, ST);
}
int nmh_fcos_pos2d_bwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr,
                       const float* labels, const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, const float* g_reg,
                       const float* g_ctr, float* const* dreg, float* const* dctr, void* stream) {
  CLR();
  REQ(level_dims, reg, ctr, labels, targets, ctr_targets, valid, scalars, dreg, dctr);
  if (!(proj2d_weight >= 0.f) || ncols != 8) return -4;
  return k_fcos_pos2d_bwd(nlevels, level_dims, N, ncols, loss_type, add_l1, proj2d_weight, reg, ctr, labels, targets, ctr_targets, valid, scalars, world, g_reg, g_ctr, dreg, dctr, ST);
}
int nmh_fcos_obb_encode(const float* locations, const float* boxes, int64_t n, float* out, void* stream) {
  CLR();
  if (n < 0) return -4;
  if (n == 0) return 0;
  REQ(locations, boxes, out);
  return k_fcos_obb_encode(locations, boxes, (long)n, out, ST);
}
int nmh_fcos_obb_decode_fwd(const float* locations, const float* regression, int64_t n, float* boxes, void* stream) {
  CLR();
  if (n < 0) return -4;
  if (n == 0) return 0;
  REQ(locations, regression, boxes);
  return k_fcos_obb_decode_fwd(locations, regression, (long)n, boxes, ST);
}
int nmh_fcos_obb_decode_bwd(const float* regression, const float* gbox, int64_t n, float* dregression, void* stream) {
  CLR();
  if (n < 0) return -4;
  if (n == 0) return 0;
  REQ(regression, gbox, dregression);
  return k_fcos_obb_decode_bwd(regression, gbox, (long)n, dregression, ST);
}
int64_t nmh_fcos_post_cap(int nlevels, const int* level_n, int N, int pre_nms_top_n) { return level_n ? k_fcos_post_cap(nlevels, level_n, N, pre_nms_top_n) : -1; }
int nmh_fcos_post_select(int nlevels, const int* level_n, int N, int ncols, int pre_nms_top_n, const float* const* cls, const float* const* reg, const float* const* ctr,
                         const float* const* locations, const unsigned char* const* masks, const int* grid_sizes, float pre_nms_thresh, float min_size, uint32_t* keys,
                         float* pre_boxes, float* pre_scores, int* pre_counts, void* stream) {
  CLR();
  REQ(level_n, cls, reg, ctr, locations, keys, pre_boxes, pre_scores, pre_counts);
  return k_fcos_post_select(nlevels, level_n, N, ncols, pre_nms_top_n, cls, reg, ctr, locations, masks, grid_sizes, pre_nms_thresh, min_size, (unsigned*)keys, pre_boxes, pre_scores,
                            pre_counts, ST);
}
int nmh_fcos_post_nms(int nlevels, const int* level_n, int N, int ncols, int pre_nms_top_n, const float* pre_boxes, const float* sorted_scores, const int64_t* order,
                      const int* pre_counts, float nms_thresh, int post_nms_top_n, uint64_t* mask, int* keep, float* boxes, float* scores, int* counts, void* stream) {
  CLR();
  REQ(level_n, pre_boxes, sorted_scores, order, pre_counts, mask, keep, boxes, scores, counts);
  return k_fcos_post_nms(nlevels, level_n, N, ncols, pre_nms_top_n, pre_boxes, sorted_scores, (const long*)order, pre_counts, nms_thresh, post_nms_top_n, (unsigned long long*)mask, keep,
                         boxes, scores, counts, ST);
}
int64_t nmh_rpn_num_blocks(int nlevels, const int* level_dims, int N) { return k_rpn_num_blocks(nlevels, level_dims, N); }
int nmh_rpn_assign(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* boxes, const int* box_offsets, const int* ori_sizes, float fg_iou_thresh,
                   float bg_iou_thresh, uint32_t* gt_max, float* labels, int* matched_idxs, float* targets, void* stream) {
  CLR();
  REQ(level_dims, base_half, box_offsets, labels, matched_idxs, targets);
  return k_rpn_assign(nlevels, level_dims, base_half, N, ncols, boxes, box_offsets, ori_sizes, fg_iou_thresh, bg_iou_thresh, (unsigned*)gt_max, labels, matched_idxs, targets, ST);
}
int nmh_rpn_sample(int N, int64_t n, const float* labels, int batch, int want_pos, int64_t* rng_state, unsigned char* flags, int* counts, void* stream) {
  CLR();
  REQ(labels, rng_state, flags, counts);
  return k_rpn_sample(N, (long)n, labels, batch, want_pos, (long*)rng_state, flags, counts, ST);
}
int nmh_rpn_loss_fwd(int nlevels, const int* level_dims, int N, int ncols, const float* const* objectness, const float* const* regression, const unsigned char* flags,
                     const float* targets, float* partials, float* scalars, void* stream) {
  CLR();
  REQ(level_dims, objectness, regression, flags, targets, partials, scalars);
  return k_rpn_loss_fwd(nlevels, level_dims, nullptr, N, ncols, -1, objectness, regression, flags, targets, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, partials, scalars, ST);
}
int nmh_rpn_loss_bwd(int nlevels, const int* level_dims, int N, int ncols, const float* const* objectness, const float* const* regression, const unsigned char* flags,
                     const float* targets, const float* scalars, const float* g_obj, const float* g_reg, float* const* dobj, float* const* dreg, void* stream) {
  CLR();
  REQ(level_dims, objectness, regression, flags, targets, scalars, dobj, dreg);
  return k_rpn_loss_bwd(nlevels, level_dims, nullptr, N, ncols, -1, objectness, regression, flags, targets, nullptr, nullptr, nullptr, nullptr, nullptr, 0.f, scalars, g_obj, g_reg, nullptr,
                        dobj, dreg, ST);
}
int nmh_rpn_iou_loss_fwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression,
                         const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, float* partials, float* scalars,
                         void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, flags, box_offsets, matched_idxs, partials, scalars);
  if (loss_type < 0) return -4;
  return k_rpn_loss_fwd(nlevels, level_dims, base_half, N, ncols, loss_type, objectness, regression, flags, nullptr, boxes, box_offsets, ori_sizes, matched_idxs, nullptr, 0.f, partials,
                        scalars, ST);
}
int nmh_rpn_iou_loss_bwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression,
                         const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* scalars, const float* g_obj,
                         const float* g_reg, float* const* dobj, float* const* dreg, void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, flags, box_offsets, matched_idxs, scalars, dobj, dreg);
  if (loss_type < 0) return -4;
  return k_rpn_loss_bwd(nlevels, level_dims, base_half, N, ncols, loss_type, objectness, regression, flags, nullptr, boxes, box_offsets, ori_sizes, matched_idxs, nullptr, 0.f, scalars,
                        g_obj, g_reg, nullptr, dobj, dreg, ST);
}
int nmh_rpn_loss2d_fwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* const* objectness, const float* const* regression,
                       const unsigned char* flags, const float* targets, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams,
                       float res, float* partials, float* scalars, void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, flags, targets, box_offsets, matched_idxs, cams, partials, scalars);
  return k_rpn_loss_fwd(nlevels, level_dims, base_half, N, ncols, -1, objectness, regression, flags, targets, boxes, box_offsets, ori_sizes, matched_idxs, cams, res, partials, scalars, ST);
}
int nmh_rpn_loss2d_bwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* const* objectness, const float* const* regression,
                       const unsigned char* flags, const float* targets, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams,
                       float res, const float* scalars, const float* g_obj, const float* g_reg, const float* g_2d, float* const* dobj, float* const* dreg, void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, flags, targets, box_offsets, matched_idxs, cams, scalars, dobj, dreg);
  return k_rpn_loss_bwd(nlevels, level_dims, base_half, N, ncols, -1, objectness, regression, flags, targets, boxes, box_offsets, ori_sizes, matched_idxs, cams, res, scalars, g_obj,
                        g_reg, g_2d, dobj, dreg, ST);
}
int nmh_rpn_iou_loss2d_fwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression,
                           const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams, float res,
                           float* partials, float* scalars, void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, flags, box_offsets, matched_idxs, cams, partials, scalars);
  if (loss_type < 0) return -4;
  return k_rpn_loss_fwd(nlevels, level_dims, base_half, N, ncols, loss_type, objectness, regression, flags, nullptr, boxes, box_offsets, ori_sizes, matched_idxs, cams, res, partials,
                        scalars, ST);
}
int nmh_rpn_iou_loss2d_bwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression,
                           const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams, float res,
                           const float* scalars, const float* g_obj, const float* g_reg, const float* g_2d, float* const* dobj, float* const* dreg, void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, flags, box_offsets, matched_idxs, cams, scalars, dobj, dreg);
  if (loss_type < 0) return -4;
  return k_rpn_loss_bwd(nlevels, level_dims, base_half, N, ncols, loss_type, objectness, regression, flags, nullptr, boxes, box_offsets, ori_sizes, matched_idxs, cams, res, scalars,
                        g_obj, g_reg, g_2d, dobj, dreg, ST);
}
int nmh_proj2d_cameras(float res, float* cams) {
  CLR();
  REQ(cams);
  if (!(res > 0.f)) return -4;
  k_proj2d_cameras(res, cams);
  return 0;
}
int nmh_proj2d_fwd(const float* pred, const float* target, int64_t n, int ncols, const float* cams, float* terms, void* stream) {
  CLR();
  if (n < 0 || (ncols != 6 && ncols != 7)) return -4;
  REQ(cams);
  if (n == 0) return 0;
  REQ(pred, target, terms);
  return k_proj2d_fwd(pred, target, (long)n, ncols, cams, terms, ST);
}
int nmh_proj2d_bwd(const float* pred, const float* target, const float* g_terms, int64_t n, int ncols, const float* cams, float* dpred, void* stream) {
  CLR();
  if (n < 0 || (ncols != 6 && ncols != 7)) return -4;
  REQ(cams);
  if (n == 0) return 0;
  REQ(pred, target, g_terms, dpred);
  return k_proj2d_bwd(pred, target, g_terms, (long)n, ncols, cams, dpred, ST);
}
int64_t nmh_rpn_post_cap(int nlevels, const int* level_dims, int N, int pre_nms_top_n) { return level_dims ? k_rpn_post_cap(nlevels, level_dims, N, pre_nms_top_n) : -1; }
int64_t nmh_rpn_post_mask_words(int nlevels, const int* level_dims, int N, int pre_nms_top_n) { return level_dims ? k_rpn_post_mask_words(nlevels, level_dims, N, pre_nms_top_n) : -1; }
int nmh_rpn_decode(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* const* regression, float* boxes, void* stream) {
  CLR();
  REQ(level_dims, base_half, regression, boxes);
  return k_rpn_decode(nlevels, level_dims, base_half, N, ncols, regression, boxes, ST);
}
int nmh_rpn_post_select(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int pre_nms_top_n, const float* const* objectness, const float* const* regression,
                        const int* ori_sizes, const int* mesh_size, float score_thresh, float min_size, int64_t* pre_keys, float* pre_boxes, float* pre_scores, int* pre_index,
                        int* pre_counts, void* stream) {
  CLR();
  REQ(level_dims, base_half, objectness, regression, mesh_size, pre_keys, pre_boxes, pre_scores, pre_index, pre_counts);
  return k_rpn_post_select(nlevels, level_dims, base_half, N, ncols, pre_nms_top_n, objectness, regression, ori_sizes, mesh_size, score_thresh, min_size, (long*)pre_keys, pre_boxes,
                           pre_scores, pre_index, pre_counts, ST);
}
int nmh_rpn_post_nms(int nlevels, const int* level_dims, int N, int ncols, int pre_nms_top_n, const float* pre_boxes, const float* pre_scores, const int* pre_index,
                     const int64_t* sorted_keys, const int64_t* order, const int* pre_counts, float nms_thresh, int post_nms_top_n, uint64_t* mask, int* keep, float* boxes,
                     float* scores, int* levels, int* index, int* counts, void* stream) {
  CLR();
  REQ(level_dims, pre_boxes, pre_scores, pre_index, sorted_keys, order, pre_counts, mask, keep, boxes, scores, levels, index, counts);
  return k_rpn_post_nms(nlevels, level_dims, N, ncols, pre_nms_top_n, pre_boxes, pre_scores, pre_index, (const long*)sorted_keys, (const long*)order, pre_counts, nms_thresh,
                        post_nms_top_n, (unsigned long long*)mask, keep, boxes, scores, levels, index, counts, ST);
}
int nmh_rpn_head_out_fwd(int dt, int nlevels, const int* level_vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box,
                         const float* b_cls, const float* b_box, float* const* objectness, float* const* regression, void* stream) {
  CLR();
  REQ(level_vox, t, w_cls, w_box, b_cls, b_box, objectness, regression);
  return k_rpn_head_out_fwd(dt, nlevels, level_vox, N, Cin, A, C, relu, t, w_cls, w_box, b_cls, b_box, objectness, regression, ST);
}
int64_t nmh_rpn_head_bwd_ws_floats(int nlevels, const int* level_vox, int N, int Cin, int A, int C) {
  return level_vox ? k_rpn_head_bwd_ws_floats(nlevels, level_vox, N, Cin, A, C) : -1;
}
int nmh_rpn_head_out_bwd(int dt, int nlevels, const int* level_vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box,
                         const float* const* g_obj, const float* const* g_reg, void* const* dt_out, float* partials, float* dw_cls, float* dw_box, float* db_cls, float* db_box,
                         void* stream) {
  CLR();
  REQ(level_vox, t, w_cls, w_box, g_obj, g_reg, dt_out, partials, dw_cls, dw_box, db_cls, db_box);
  return k_rpn_head_out_bwd(dt, nlevels, level_vox, N, Cin, A, C, relu, t, w_cls, w_box, g_obj, g_reg, dt_out, partials, dw_cls, dw_box, db_cls, db_box, ST);
}
int nmh_relu_(int dt, void* x, int64_t n, void* stream) {
  CLR();
  REQ(x);
  return k_relu_(dt, x, (long)n, ST);
}
int nmh_relu_bwd_(int dt, void* dy, const void* y, int64_t n, void* stream) {
  CLR();
  REQ(dy, y);
  return k_relu_bwd_(dt, dy, y, (long)n, ST);
}
int nmh_box_head_pack(int dt, int reg_dim, int n_classes, int C, int S, const float* w_box, const float* w_cls, void* wcat, void* stream) {
  CLR();
  return k_box_head_pack(dt, reg_dim, n_classes, C, S, w_box, w_cls, wcat, ST);
}
int nmh_box_head_out_fwd(int dt, int M, int S, int C, int reg_dim, int n_classes, int flatten, int relu, const void* x, const void* wcat, const float* b_box, const float* b_cls,
                         float* xmean, float* pred_bbox_delta, float* pred_scores, void* stream) {
  CLR();
  return k_box_head_out_fwd(dt, M, S, C, reg_dim, n_classes, flatten, relu, x, wcat, b_box, b_cls, xmean, pred_bbox_delta, pred_scores, ST);
}
int64_t nmh_box_head_bwd_ws_floats(int M, int S, int C, int reg_dim, int n_classes, int flatten) { return k_box_head_bwd_ws_floats(M, S, C, reg_dim, n_classes, flatten); }
int nmh_box_head_out_bwd(int dt, int M, int S, int C, int reg_dim, int n_classes, int flatten, int relu, const void* x, const void* wcat, const float* xmean, const float* g_box,
                         const float* g_cls, void* dx, float* dxmean, float* partials, float* dw_box, float* dw_cls, float* db_box, float* db_cls, void* stream) {
  CLR();
  if ((g_box && (!dw_box || !db_box)) || (g_cls && (!dw_cls || !db_cls))) return -4;
  return k_box_head_out_bwd(dt, M, S, C, reg_dim, n_classes, flatten, relu, x, wcat, xmean, g_box, g_cls, dx, dxmean, partials, g_box ? dw_box : nullptr, g_cls ? dw_cls : nullptr,
                            g_box ? db_box : nullptr, g_cls ? db_cls : nullptr, ST);
}
int64_t nmh_box_head_colsum_ws_floats(int64_t rows, int C) { return k_box_head_colsum_ws_floats((long)rows, C); }
int nmh_box_head_colsum(int dt, const void* dy, int64_t rows, int C, float* partials, float* db, void* stream) {
  CLR();
  return k_box_head_colsum(dt, dy, (long)rows, C, partials, db, ST);
}
int64_t nmh_conv3d_k3_wgrad_fixed_ws_floats(int dt, int64_t rows, int Cin, int Cout) { return k_conv3_tn_fixed_ws_floats(dt, (long)rows, Cin, Cout); }
int nmh_conv3d_k3_wgrad_fixed(int dt, const void* dY, const void* X, float* dW, float* ws, int64_t ws_floats, int B, int D, int H, int W, int Cin, int Cout, void* stream) {
  CLR();
  REQ(dY, X, dW);
  if (B < 1 || D < 1 || H < 1 || W < 1 || Cin < 8 || Cin % 8 || Cout < 8 || Cout % 8) return -4;
  static float dummy_ws;       // a single split needs no workspace, but the fixed-order path is selected by a non-null one
  return k_conv3_tn(dt, dY, X, dW, B, D, H, W, Cin, Cout, ST, ws ? ws : &dummy_ws, ws ? (long)ws_floats : 0);
}
int64_t nmh_fcos_gn_ws_doubles(int njobs, const int* vox, int N, int C) { return vox ? k_fcos_gn_ws_doubles(njobs, vox, N, C) : -1; }
int nmh_fcos_gn_stats(int dt, int njobs, const int* vox, int N, int C, int G, float eps, const void* const* x, double* ws, float* stats, void* stream) {
  CLR();
  REQ(vox, x, ws, stats);
  return k_fcos_gn_stats(dt, njobs, vox, N, C, G, eps, x, ws, stats, ST);
}
int nmh_fcos_gn_apply(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* x, const float* stats, const float* const* gamma,
                      const float* const* beta, void* const* y, void* stream) {
  CLR();
  REQ(vox, tower, x, stats, gamma, beta, y);
  return k_fcos_gn_apply(dt, njobs, vox, tower, N, C, G, x, stats, gamma, beta, y, ST);
}
int nmh_fcos_gn_bwd(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* dy, const void* const* x, const void* const* y, const float* stats,
                    const float* const* gamma, double* ws, float* sums, float* const* dgamma, float* const* dbeta, void* const* dx, void* stream) {
  CLR();
  REQ(vox, tower, dy, x, y, stats, gamma, ws, sums, dgamma, dbeta, dx);
  return k_fcos_gn_bwd(dt, njobs, vox, tower, N, C, G, dy, x, y, stats, gamma, ws, sums, dgamma, dbeta, dx, ST);
}
int nmh_fcos_head_out_fwd(int dt, int nlevels, const int* dims, const float* strides, int N, int C, int nreg, int ctr_on_reg, int mode, const void* const* act, const void* const* w16,
                          const float* b_cls, const float* b_box, const float* b_ctr, const float* const* scale, float* const* cls, float* const* reg, float* const* ctr,
                          float* const* u, void* stream) {
  CLR();
  REQ(dims, strides, act, w16, b_cls, b_box, b_ctr, scale, cls, reg, ctr, u);
  return k_fcos_out_fwd(dt, nlevels, dims, strides, N, C, nreg, ctr_on_reg, mode, act, w16, b_cls, b_box, b_ctr, scale, cls, reg, ctr, u, ST);
}
int64_t nmh_fcos_head_pack_ws_floats(int nlevels, const int* dims, int N) { return dims ? k_fcos_out_pack_ws_floats(nlevels, dims, N) : -1; }
int nmh_fcos_head_out_bwd_pack(int dt, int nlevels, const int* dims, const float* strides, int N, int nreg, int ctr_on_reg, int mode, const float* const* g_cls,
                               const float* const* g_reg, const float* const* g_ctr, const float* const* u, const float* const* scale, void* const* g16, float* const* gt,
                               float* partials, float* db_cls, float* db_box, float* db_ctr, float* const* dscale, void* stream) {
  CLR();
  REQ(dims, strides, g_cls, g_reg, g_ctr, u, scale, g16, gt, partials, db_cls, db_box, db_ctr, dscale);
  return k_fcos_out_bwd_pack(dt, nlevels, dims, strides, N, nreg, ctr_on_reg, mode, g_cls, g_reg, g_ctr, u, scale, g16, gt, partials, db_cls, db_box, db_ctr, dscale, ST);
}
int64_t nmh_fcos_head_wgrad_ws_floats(int nlevels, const int* dims, int N, int C) { return dims ? k_fcos_out_wgrad_ws_floats(nlevels, dims, N, C) : -1; }
int nmh_fcos_head_out_wgrad(int dt, int nlevels, const int* dims, int N, int C, int nreg, int ctr_on_reg, const void* const* act, const float* const* gt, float* partials,
                            float* dw_cls, float* dw_box, float* dw_ctr, void* stream) {
  CLR();
  REQ(dims, act, gt, partials, dw_cls, dw_box, dw_ctr);
  return k_fcos_out_wgrad(dt, nlevels, dims, N, C, nreg, ctr_on_reg, act, gt, partials, dw_cls, dw_box, dw_ctr, ST);
}
int nmh_step_params(const uint32_t* block_bits, int nb, int g, unsigned char* tokmask, const float* hyper, float* hyper_dev, const int* extents, int n_ext, int* extents_dev,
                    void* stream) {
  CLR();
  if ((tokmask && !block_bits) || (hyper && !hyper_dev) || (extents && !extents_dev)) return -4;
  return k_step_params(block_bits, nb, g, tokmask, hyper, hyper_dev, extents, n_ext, extents_dev, ST);
}
int nmh_grad_to_bf16(const float* g, void* bucket, int64_t n, void* stream) {
  CLR();
  if (n <= 0) return 0;
  if (!g || !bucket) return -4;
  return k_grad_cast(1, g, bucket, (long)n, 1.0f, ST);
}
int nmh_grad_from_bf16(const void* bucket, float* g, int64_t n, float scale, void* stream) {
  CLR();
  if (n <= 0) return 0;
  if (!g || !bucket) return -4;
  return k_grad_cast(0, bucket, g, (long)n, scale, ST);
}
char* g_nmh_arena_base = nullptr;
size_t g_nmh_arena_bytes = 0;
int nmh_set_prezeroed_arena(void* base, int64_t bytes) {
  CLR();
  if (bytes < 0 || (bytes > 0 && !base)) return -4;
  g_nmh_arena_base = (char*)base;
  g_nmh_arena_bytes = (size_t)bytes;
  return 0;
}
int nmh_fill_f32(float* p, float v, int64_t n, void* stream) {
  CLR(); return k_fill_f32(p, v, (long)n, ST); }
int nmh_pack_weights(int dt, const void* descs_dev, const int* blk2desc_dev, const int64_t* blkstart_dev, int nblocks, void* stream) {
  CLR();
  static_assert(sizeof(PackDesc) == 40 || sizeof(PackDesc) == 48, "PackDesc layout");
  if (nblocks <= 0) return 0;
  return k_pack_weights(dt, (const PackDesc*)descs_dev, blk2desc_dev, (const long*)blkstart_dev, nblocks, ST);
}
int nmh_grad_sqnorm(const float* g, int64_t n, double* acc, void* stream) {
  CLR(); return k_sqnorm(g, (long)n, acc, ST); }
int nmh_roi_targets(int N, int cap, int ncols, int R, int is_sample, const float* boxes, const int* levels, const int* counts, const float* gt, const float* gt_labels,
                    const int* box_offsets, int want_fg, float fg_threshold, float bg_threshold, int64_t* rng_state, float* max_iou, int* arg, int* lists, int* keep, int* counts2,
                    float* labels, float* rois, float* gt_rois, void* stream) {
  CLR();
  REQ(boxes, levels, counts, box_offsets, max_iou, arg, keep, labels, rois, gt_rois);
  if (is_sample) REQ(counts2);
  return k_roi_targets(N, cap, ncols, R, is_sample, boxes, levels, counts, gt, gt_labels, box_offsets, want_fg, fg_threshold, bg_threshold, (long*)rng_state, max_iou, arg, lists, keep,
                       counts2, labels, rois, gt_rois, ST);
}
int nmh_roi_level_map(int64_t M, const float* boxes, int stride, int ncols, int k_min, int k_max, float canonical_scale, float canonical_level, float eps, int* levels, void* stream) {
  CLR();
  REQ(boxes, levels);
  return k_roi_level_map((long)M, boxes, stride, ncols, k_min, k_max, canonical_scale, canonical_level, eps, levels, ST);
}
int nmh_roi_pool_fwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps,
                     const float* rois, const int* level_override, float* out, int* argmax, void* stream) {
  CLR();
  REQ(level_dims, scales, maps, rois, out, argmax);
  return k_roi_pool_fwd(nlevels, level_dims, scales, N, C, R, ncols, ow, oh, od, enlarge, maps, rois, level_override, out, argmax, ST);
}
int nmh_roi_pool_bwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const int* argmax,
                     const float* rois, const int* level_override, float* const* dmaps, void* stream) {
  CLR();
  REQ(level_dims, scales, dout, argmax, rois, dmaps);
  return k_roi_pool_bwd(nlevels, level_dims, scales, N, C, R, ncols, ow, oh, od, enlarge, dout, argmax, rois, level_override, dmaps, ST);
}
int nmh_roi_interp_fwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps,
                       const float* rois, const int* level_override, float* out, void* stream) {
  CLR();
  REQ(level_dims, scales, maps, rois, out);
  return k_roi_interp_fwd(nlevels, level_dims, scales, N, C, R, ncols, ow, oh, od, enlarge, maps, rois, level_override, out, ST);
}
int nmh_roi_interp_bwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const float* rois,
                       const int* level_override, float* const* dmaps, void* stream) {
  CLR();
  REQ(level_dims, scales, dout, rois, dmaps);
  return k_roi_interp_bwd(nlevels, level_dims, scales, N, C, R, ncols, ow, oh, od, enlarge, dout, rois, level_override, dmaps, ST);
}
int64_t nmh_roi_loss_blocks(int64_t M) { return k_roi_loss_blocks((long)M); }
int nmh_roi_loss_fwd(int64_t M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* rois, int roi_stride, const float* gt_rois,
                     float* targets, float* partials, float* scalars, void* stream) {
  CLR();
  REQ(scores, deltas, labels, rois, gt_rois, targets, partials, scalars);
  return k_roi_loss_fwd((long)M, n_classes, ncols, scores, deltas, labels, rois, roi_stride, gt_rois, targets, partials, scalars, ST);
}
int nmh_roi_loss_bwd(int64_t M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* targets, const float* scalars, const float* g_obj,
                     const float* g_reg, float* dscores, float* ddeltas, void* stream) {
  CLR();
  REQ(scores, deltas, labels, targets, scalars, dscores, ddeltas);
  return k_roi_loss_bwd((long)M, n_classes, ncols, scores, deltas, labels, targets, scalars, g_obj, g_reg, dscores, ddeltas, ST);
}
int nmh_roi_decode(int64_t M, int ncols, const float* deltas, const float* rois, int roi_stride, float* boxes, void* stream) {
  CLR();
  REQ(deltas, rois, boxes);
  return k_roi_decode((long)M, ncols, deltas, rois, roi_stride, boxes, ST);
}
int nmh_roi_post_select(int N, int R, int n_classes, int ncols, const float* pred_scores, const float* pred_bbox_deltas, const float* rois, const int* counts, const int* mesh_sizes,
                        float score_thresh, float min_size, int is_reg, int threshold_mode, float* cand_boxes, float* cand_scores, int* keys, void* stream) {
  CLR();
  REQ(pred_scores, rois, counts, mesh_sizes, cand_boxes, cand_scores, keys);
  if (is_reg) REQ(pred_bbox_deltas);
  return k_roi_post_select(N, R, n_classes, ncols, pred_scores, pred_bbox_deltas, rois, counts, mesh_sizes, score_thresh, min_size, is_reg ? 1 : 0, threshold_mode, cand_boxes, cand_scores,
                           keys, ST);
}
int nmh_roi_post_nms(int N, int R, int ncols, const float* cand_boxes, const float* cand_scores, const int* sorted_keys, const int64_t* order, float nms_thresh, uint64_t* mask, int* keep,
                     float* boxes, float* scores, int* index, int* counts_out, void* stream) {
  CLR();
  REQ(cand_boxes, cand_scores, sorted_keys, order, mask, keep, boxes, scores, index, counts_out);
  return k_roi_post_nms(N, R, ncols, cand_boxes, cand_scores, sorted_keys, (const long*)order, nms_thresh, (unsigned long long*)mask, keep, boxes, scores, index, counts_out, ST);
}
static bool det_eval_dims_ok(int N, int cap, int Gmax) { return N >= 0 && cap >= 0 && cap <= NMH_OBB_NMS_MAX && Gmax >= 0 && Gmax <= NMH_DET_EVAL_MAX_GT; }
int nmh_det_eval_iou(int ncols, int N, int cap, int row_stride, int col_offset, const float* boxes, const int* counts, int Gmax, const float* gt, const int* gt_counts, float* iouT,
                     float* best_iou, int* best_gt, void* stream) {
  CLR();
  if ((ncols != 6 && ncols != 7) || !det_eval_dims_ok(N, cap, Gmax) || col_offset < 0 || row_stride < col_offset + ncols) return -4;
  if (N == 0 || cap == 0) return 0;
  REQ(boxes, counts, gt_counts, best_iou, best_gt);
  if (Gmax > 0) REQ(gt, iouT);
  return k_det_eval_iou(ncols, N, cap, row_stride, col_offset, boxes, counts, Gmax, gt, gt_counts, iouT, best_iou, best_gt, ST);
}
int nmh_det_eval_match(int N, int cap, int Gmax, const int* counts, const int* gt_counts, const float* iouT, int nlimits, const int* limits, float* gt_overlaps, int* counted,
                       void* stream) {
  CLR();
  if (!det_eval_dims_ok(N, cap, Gmax) || nlimits < 1 || nlimits > NMH_DET_EVAL_MAX_LIMITS) return -4;
  if (N == 0) return 0;
  REQ(counts, gt_counts, limits, counted);
  if (Gmax > 0) REQ(gt_overlaps);
  if (Gmax > 0 && cap > 0) REQ(iouT);
  return k_det_eval_match(N, cap, Gmax, counts, gt_counts, iouT, nlimits, limits, gt_overlaps, counted, ST);
}
int nmh_det_eval_claims(int N, int cap, int Gmax, const int* counts, const float* best_iou, const int* best_gt, int nthresh, const float* thresholds, int top_k,
                        unsigned char* tp_mask, unsigned char* kept, void* stream) {
  CLR();
  if (!det_eval_dims_ok(N, cap, Gmax) || nthresh < 1 || nthresh > NMH_DET_EVAL_MAX_THRESH) return -4;
  if (N == 0 || cap == 0) return 0;
  REQ(counts, best_iou, best_gt, thresholds, tp_mask, kept);
  return k_det_eval_claims(N, cap, Gmax, counts, best_iou, best_gt, nthresh, thresholds, top_k, tp_mask, kept, ST);
}
int nmh_det_eval_pr(int64_t M, const unsigned char* bits, const int* n_det, const int* num_gt, int nthresh, int* tp_cum, int* fp_cum, float* recalls, float* precisions, double* ap,
                    void* stream) {
  CLR();
  if (M < 0 || M > 0x7fffffffll || nthresh < 1 || nthresh > NMH_DET_EVAL_MAX_THRESH) return -4;
  if (M == 0) return 0;
  REQ(bits, n_det, num_gt, tp_cum, fp_cum, recalls, precisions, ap);
  return k_det_eval_pr((long)M, bits, n_det, num_gt, nthresh, tp_cum, fp_cum, recalls, precisions, ap, ST);
}
int nmh_clip_coef(const double* acc, float max_norm, float* coef, float* norm_out, void* stream) {
  CLR(); return k_clip_coef(acc, max_norm, coef, norm_out, ST); }
int nmh_clip_coef_mean(const double* acc, float max_norm, const float* inv_k_dev, float* coef, float* norm_out, void* stream) {
  CLR();
  REQ(acc, inv_k_dev, coef);
  return k_clip_coef_mean(acc, max_norm, inv_k_dev, coef, norm_out, ST);
}
int nmh_grad_scale(float inv_k, float* inv_k_dev, void* stream) {
  CLR();
  REQ(inv_k_dev);
  return k_grad_scale(inv_k, inv_k_dev, ST);
}
int nmh_adamw_step(float* p, float* g, float* m, float* v, int64_t n, const float* hyper, const float* coef, void* stream) {
  CLR(); return k_adamw(p, g, m, v, (long)n, hyper, coef, ST); }
int nmh_grad_sqnorm_ranges(const float* g, int64_t n, const int64_t* bounds, const float* scale, int R, double* acc, void* stream) {
  CLR();
  REQ(g, bounds, scale, acc);
  if (((uintptr_t)bounds | (uintptr_t)scale) & 7) return -5;
  return k_sqnorm_ranges(g, (long)n, reinterpret_cast<const long*>(bounds), scale, R, acc, ST);
}
int nmh_adamw_step_ranges(float* p, float* g, float* m, float* v, int64_t n, const float* hyper, const float* coef, const int64_t* bounds, const float* scale, int R,
                          void* stream) {
  CLR();
  REQ(p, g, m, v, hyper, bounds, scale);
  if (((uintptr_t)bounds | (uintptr_t)scale) & 7) return -5;
  return k_adamw_ranges(p, g, m, v, (long)n, hyper, coef, reinterpret_cast<const long*>(bounds), scale, R, ST);
}
}
