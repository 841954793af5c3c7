/* nerfmae_hip.h -- C ABI of libnerfmae_hip.so: the MI355X (gfx950) kernels of the NeRF-MAE 3-D Swin MAE
 * pre-training hot path (reference class SwinTransformer_MAE3D_New, nerf_mae/model/mae/swin_mae3d.py:1067-1599).
 *
 * The reference has no FFI on this path -- every op is a stock PyTorch call.  This header is therefore
 * the native-op surface a maintainer would bind in place of those calls (INTEGRATION.md shows the ctypes / pybind
 * stubs); each entry cites the reference op it replaces.  Conventions:
 *   - plain device pointers + sizes, no torch types; all launches are asynchronous on `stream` (a hipStream_t);
 *   - return 0 on success, a hipError_t (>0) or a negative argument-error code otherwise (nmh_error_string); a NULL in a required
 *     pointer argument returns -4 (invalid argument), never a device fault;
 *   - `dt`: storage/compute type of activations and packed weights: 0 = fp32 (exact fp32 MFMA; the 1e-3-parity
 *     mode), 1 = bf16 (bf16 MFMA, fp32 accumulate).  Parameters, gradients and statistics are always fp32.
 *   - activations are channels-last token/voxel-major matrices [rows, C]; rows of a (B,A0,A1,A2,C) volume are
 *     ((b*A0+a0)*A1+a1)*A2+a2 (A2 fastest) -- the reference's (B,H,W,D,C) order;
 *   - `wm` points to 10 host ints {B, H, W, D, PH, PW, PD, s0, s1, s2}: token grid, grid padded to multiples of 4,
 *     effective cyclic shifts (0 where window >= padded size; swin_mae3d.py:62-81).
 * Every line below that starts with NMH_API is parsed by the Python binding and by tests/test_host_cpu.py::test_capi_library_loads_and_exports_every_declared_symbol.
 */
#ifndef NERFMAE_HIP_H
#define NERFMAE_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define NMH_API __attribute__((visibility("default")))

NMH_API int nmh_version(void);
NMH_API const char* nmh_error_string(int code);

/* C[M,N] = epi(A[M,K] . W[N,K]^T): replaces F.linear (swin_mae3d.py:108,173; torchvision MLP :352-358; PatchMerging.reduction
 * :413), the patch conv as GEMM (:1120-1126), ConvTranspose3d k=s as GEMM (unetr_block.py:151-158) and 1x1x1 convs (:52-55).
 * epilogue order: +bias[N]; act 1: C2=pre-activation, exact-erf GELU; act 2: *= gelu'(C2); *= rowscale[row/rows_per_scale]
 * (stochastic depth, :367-368); += resid; accumulate: += C.  C, C2, resid share ldc. */
NMH_API int nmh_gemm_nt(int dt, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N, int K, void* C, int64_t ldc, const float* bias, int act, void* C2, const void* resid, const float* rowscale, int rows_per_scale, int accumulate, void* stream);
/* Attention output projection with the window reverse folded into the store (swin_mae3d.py:176-197 + the residual of :367):
 * out[tok] = resid[tok] + rowscale[tok / tokens_per_sample] * (A[m] . W^T + bias) for every window-ordered row m that maps to a token
 * (pad rows are dropped); wm as in nmh_window_scatter_residual, which this replaces. */
NMH_API int nmh_gemm_nt_window_scatter(int dt, const void* A, int64_t lda, const void* W, int64_t ldw, int M, int N, int K, void* out, const void* resid, const float* bias, const float* rowscale, int tokens_per_sample, const int* wm, void* stream);
/* dW[N,K] += sum_m A[m,N]*rowscale . B[m,K]  (fp32 atomics): weight gradients of the ops above.
 * omode 0: dW[n*ldo+k]; omode 2: ConvTranspose3d weight [Cin=K][Cout=p0][k3=p1] with n = tap*Cout+co.
 * dbias (optional): dbias[n] += sum_m A[m,n]*rowscale -- the layer's bias gradient from the same pass over A.
 * ws (optional, ws_floats fp32): scratch for the partial tiles of a split contraction; with it the splits are summed by a second
 * launch instead of fp32 global atomics (one scratch per stream: concurrent calls must not share it). */
NMH_API int nmh_gemm_tn(int dt, const void* A, int64_t lda, const void* B, int64_t ldb, float* dW, int64_t M, int N, int K, const float* rowscale, int rows_per_scale, int omode, int64_t ldo, int p0, int p1, float* dbias, float* ws, int64_t ws_floats, void* stream);
/* Which kernel nmh_gemm_nt / nmh_gemm_tn would launch for these arguments: the launch path decides through the same function.
 * Pure host queries: nothing is launched and no device is touched (they work on a machine without a GPU).  Status 0, -2 for a shape
 * the GEMM itself rejects, -4 for a bad argument.
 * nmh_gemm_nt_plan: plan[6] = {family, MT, NT, ring stages, contraction splits, narrow}; family 0: register-prefetch kernel, tile
 *   (64 MT) x (16 NT); 1: LDS-DMA ring, same tile; 2: two-k-tile kernel (K <= 128), 64 x (16 NT); 3: 2 x 2-wave kernel, tile
 *   (32 MT) x (32 NT).  narrow = 1 when the narrow-tile rule picked the tile.  win_on / up_k / ksplit: the epilogue fields the decision
 *   reads (window scatter, transpose-conv store, split contraction: 0 / 0 / 1 for nmh_gemm_nt); batch = grid.z samples (1).
 * nmh_gemm_nt_plan_table: every {dt, family, MT, NT, stages} the launcher can launch for plain row-major operands; rows[5 * capacity]
 *   (may be NULL), *count = number of rows.
 * nmh_gemm_tn_plan: plan[6] = {NTW, KTW, ring stages, rows per split, splits, partials}; output tile (32 NTW) x (32 KTW); stages 0 = the
 *   plain kernel; partials 1 = the splits go through the workspace and a reduce launch, 0 = they add into dW (fp32 atomics when
 *   splits > 1).  ws_floats: the workspace nmh_gemm_tn would be given (0: none). */
NMH_API int nmh_gemm_nt_plan(int dt, int64_t lda, int64_t ldw, int M, int N, int K, int win_on, int up_k, int ksplit, int batch, int* plan);
NMH_API int nmh_gemm_nt_plan_table(int* rows, int capacity, int* count);
NMH_API int nmh_gemm_tn_plan(int dt, int64_t lda, int64_t M, int N, int K, int has_rowscale, int rows_per_scale, int64_t ws_floats, int* plan);
/* Grouped form of nmh_gemm_tn for bf16 operands (dt must be 1): `probs` is a HOST array of nprob descriptors; every problem is
 * dW[N,K] += sum_m rowscale[m / rows_per_sample] * A[m,N]^T . B[m,K] (+ dbias[N] += column sums of A), M a multiple of rows_per_sample.
 * The four Linear weight gradients of every Swin block of a stage (swin_mae3d.py:366-369 backward: attn.qkv, attn.proj, mlp.0, mlp.3)
 * and the PatchMerging reduction (:413) are issued through this entry once the stage's input-gradient chain is done: up to 16 problems
 * per kernel launch (descriptors travel as kernel arguments: graph-capturable), one 96x96 output tile per workgroup, contraction
 * splits only when a launch has too few tiles to fill the chip (partials in ws, summed by one reduce launch per group).
 * Optional geometry (0 = off): stride_k > 0 writes dW[n*ldo + k*stride_k]; up_k/up_v make A the pixel-shuffled view of a fine-grid tensor, so
 * the tap problems of a ConvTranspose3d(kernel = stride) weight gradient (unetr_block.py:151-158 backward) run as one grouped call that
 * reads the fine gradient once (A = dcat + tap offset, dW = weight + tap, ldo = k^3, stride_k = Cout*k^3, bias_atomic = 1).
 * n_inner > 0: column n of A is the pair (n / n_inner, n % n_inner) and lands at dW[(n % n_inner)*ldo + (n / n_inner)*stride_n2 + k*stride_k],
 * its bias gradient at dbias[n % n_inner] -- the k taps along x of one (tz, ty) tap row are then ONE problem whose A rows are the contiguous
 * k*Cout-element runs of the fine gradient -- with up_k > 0 column n is read at fine row (row + n / n_inner), channel n % n_inner, which is
 * contiguous when lda == n_inner and k strided pieces otherwise (a skip half in the row) -- k^2 problems with full 96-column tiles instead of k^3 with 48. */
typedef struct nmh_tn_problem { const void* A; int64_t lda; const void* B; int64_t ldb; float* dW; int64_t ldo; float* dbias; const float* rowscale; int64_t M; int N; int K; int rows_per_sample;
  int64_t stride_k; int up_k; int up_v; int bias_atomic; int n_inner; int64_t stride_n2; } nmh_tn_problem;
NMH_API int nmh_gemm_tn_grouped(int dt, const nmh_tn_problem* probs, int nprob, float* ws, int64_t ws_floats, void* stream);
/* The same call for a group that has the chip to itself -- the flush of the FIRST encoder stage, issued when the backward pass has nothing but
 * the patch-embedding backward left (swin_mae3d.py:1455-1463 backward): the contraction splits aim at 640 workgroups instead of the 256 that
 * suit a launch running underneath the input-gradient chain.  Same arguments, same results up to the summation order of the splits. */
NMH_API int nmh_gemm_tn_grouped_fg(int dt, const nmh_tn_problem* probs, int nprob, float* ws, int64_t ws_floats, void* stream);
/* Y[(b,z,y,x)][Cout] (+)= conv3d(k=3,pad=1) of channels-last X with packed weights [Cout][27][Cin] (nn.Conv3d in
 * UnetResBlock, unetr_block.py:35-44).  Input gradients use the same entry with the dgrad pack [Cin][27 flipped][Cout].
 * ws (optional, ws_floats fp32): scratch for a split contraction -- on small volumes (the 10^3 / 20^3 decoder levels: < 256 output tiles,
 * K = 27*Cin up to 20736) the K loop is cut into up to 8 splits whose fp32 partial tiles are summed by a second launch. */
NMH_API int nmh_conv3d_k3(int dt, const void* X, const void* Wp, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, float* ws, int64_t ws_floats, void* stream);
/* The same convolution with a per-output-channel bias in the epilogue (nn.Conv3d(C, C, 3, padding=1) of the FPN neck,
 * nerf_rpn/model/fpn.py:104). */
NMH_API int nmh_conv3d_k3_bias(int dt, const void* X, const void* Wp, const float* bias, void* Y, int B, int D, int H, int W, int Cin, int Cout, void* stream);
/* FPN top-down pathway (nerf_rpn/model/fpn.py:150-159): fine[b,zf,yf,xf,:] += coarse[b,src(zf),src(yf),src(xf),:] with
 * F.interpolate(mode="nearest", size=fine) source indices src(i) = min(floor(i * (float)in/out), in-1); channels-last, C % 8 == 0.
 * _bwd is its adjoint: dcoarse += sum of dfine over the voxels that read it. */
NMH_API int nmh_nearest_upsample_add(int dt, const void* coarse, void* fine, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, int C, void* stream);
NMH_API int nmh_nearest_upsample_add_bwd(int dt, const void* dfine, void* dcoarse, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, int C, void* stream);
/* dst[m][0..C) = src[m][0..C), row strides lds / ldd in elements: the skip connection entering (and its gradient leaving) the
 * channel-concatenated decoder tensor -- torch.cat((out, skip), dim=1), unetr_block.py:196-197, in channels-last. */
NMH_API int nmh_copy_cols(int dt, const void* src, int64_t lds, void* dst, int64_t ldd, int64_t M, int C, void* stream);
/* channels-last compute tensor [B][V][C] (dt) <-> fp32 NCDHW feature map [B][C][V], the layout nerf_rpn's heads consume
 * (torch.permute(x,[0,4,1,2,3]).contiguous(), feature_extractor.py:1183-1185), and back for the incoming gradient. */
NMH_API int nmh_ndhwc_to_ncdhw(int dt, const void* src, float* dst, int B, int64_t V, int C, void* stream);
NMH_API int nmh_ncdhw_to_ndhwc(int dt, const float* src, void* dst, int B, int64_t V, int C, void* stream);
/* The same convolution specialised for Cin = Cout = 48, bf16 (decoder1.conv_block at 160^3 -- 75 % of the model's FLOPs): persistent
 * LDS-halo implicit GEMM; Wk = fragment-ordered pack [41 steps][3][64 lanes][8] (pack modes 6 fwd / 7 dgrad). */
NMH_API int nmh_conv3d_k3_c48(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int accumulate, double* stats_acc, void* stream);
/* The input-gradient launch of that kernel when the conv's INPUT was LeakyReLU(InstanceNorm3d(Y1)) (decoder1's conv2, unetr_block.py:60-63 backward):
 * dX = conv^T(dY) as nmh_conv3d_k3_c48 with the dgrad pack, and in the same epilogue the two per-(sample, channel) sums the InstanceNorm backward needs,
 * sums [B][48][2] fp64 (zeroed here) = (sum g, sum g * yhat) with g = dX * lrelu'(Y1 - mean), yhat = (Y1 - mean) * rstd, stats1 = (mean, rstd) pairs
 * [B][48][2] -- what nmh_instnorm_bwd_reduce(dX, Y1, rmode 0) would produce in a separate pass over both tensors. */
NMH_API int nmh_conv3d_k3_c48_bwd_reduce(const void* dY, const void* Wkd, void* dX, int B, int D, int H, int W, const void* Y1, const float* stats1, float slope, double* sums, void* stream);
/* The LDS-halo kernel on 48-channel blocks: Cin, Cout multiples of 48 (the 40^3 decoder level of swin_t/s: 96 / 192 channels;
 * UnetResBlock convs, unetr_block.py:35-44); Wk = one fragment-ordered image per (output block, input block), output-block-major
 * (pack modes 6 / 7 on a [Cout][Cin][27] weight).  No fused statistics. */
NMH_API int nmh_conv3d_k3_c48mb(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, void* stream);
/* The same convolution on 64-channel blocks, bf16, Cin and Cout multiples of 64 (swin_b's decoder1 64 -> 64 at 160^3, BASELINE
 * configs[3]; the FPN neck's 256 -> 256 convolutions, nerf_rpn/model/fpn.py:104): persistent LDS-halo implicit GEMM that loops over the
 * input-channel blocks with the accumulators in registers.  Wk = fragment-ordered pack [Cout/64][Cin/64][54 steps][4][64 lanes][8]
 * (pack modes 8 fwd / 9 dgrad; nmh_conv3d_k3_c64_pack_numel elements).  stats_acc as for the 48-channel kernel: fp64 [B][Cout][2];
 * bias (optional fp32 [Cout]) is added before the store (the FPN convolutions carry a bias, the decoder's do not need theirs). */
NMH_API int nmh_conv3d_k3_c64(const void* X, const void* Wk, void* Y, int B, int D, int H, int W, int Cin, int Cout, int accumulate, double* stats_acc, const float* bias, void* stream);
NMH_API int64_t nmh_conv3d_k3_c64_pack_numel(int Cin, int Cout);
/* weight gradient of the 64-channel-block layer (dW fp32 [Cout][Cin][3][3][3], accumulated): X halo + DMA-double-buffered dY tile in
 * swizzled 128-byte LDS rows, both operands by transpose reads, taps split over two workgroup groups; ws = fp32 scratch of
 * nmh_conv3d_k3_c64_wgrad_ws_floats() elements (per-workgroup partials, summed by a second launch). */
NMH_API int nmh_conv3d_k3_c64_wgrad(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, int Cin, int Cout, void* stream);
NMH_API int64_t nmh_conv3d_k3_c64_wgrad_ws_floats(void);
/* stats_acc (optional, fp64 [B][48][2], zeroed by the call): the conv epilogue also accumulates per-(sample,channel) sum and sum of squares of
 * its outputs, i.e. the InstanceNorm3d statistics of the following norm layer; nmh_instnorm_finalize turns them into {mean, rstd}. */
NMH_API int nmh_instnorm_finalize(const double* acc, float* stats, int B, int64_t V, int C, float eps, void* stream);
/* weight gradient of the specialised layer; ws = fp32 scratch of nmh_conv3d_k3_c48_wgrad_ws_floats() elements (per-workgroup partials) */
NMH_API int nmh_conv3d_k3_c48_wgrad(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, void* stream);
/* the same LDS-halo weight-gradient kernel for any Cin, Cout that are multiples of 48 (bf16): (Cin/48)*(Cout/48) independent 48x48
 * blocks on strided channel slices, every activation row read once per block instead of once per tap; ws as above. */
NMH_API int nmh_conv3d_k3_wgrad_halo(const void* dY, const void* X, float* dW, float* ws, int B, int D, int H, int W, int Cin, int Cout, void* stream);
NMH_API int64_t nmh_conv3d_k3_c48_wgrad_ws_floats(void);
/* dW[Cout][Cin][3][3][3] (PyTorch layout, fp32) += conv weight gradient */
NMH_API int nmh_conv3d_k3_wgrad(int dt, const void* dY, const void* X, float* dW, int B, int D, int H, int W, int Cin, int Cout, void* stream);

/* LayerNorm eps over the last dim (swin_mae3d.py:341,351,388,1128) with the surrounding data movement folded in:
 * src_mode 0 rows as-is (+ optional patch-embed post-ops: + pos[tok], masked tokens <- mask_token; :1459-1463,1375-1380),
 * src_mode 1 output in window order (pad -> roll -> partition, :62-101; pad rows are zeros),
 * src_mode 2 patch-merge gather of 8 tokens -> 8C row (:390-402).  mean/rstd are saved per token (modes 0,1) / row (2).
 * backward, mode 0: dyw (optional, with wm) receives the same gradient in window order scaled by dyw_scale[tok / tokens_per_sample]
 * (the adjoint of the attention branch's window reverse; replaces nmh_window_gather_scale). */
NMH_API int nmh_layernorm_fwd(int dt, int src_mode, const void* x, void* out, const float* gamma, const float* beta, float eps, float* mean, float* rstd, int64_t rows, int C, const int* wm, const float* pos, const unsigned char* mask, const float* mask_token, int64_t tokens_per_sample, void* stream);
NMH_API int nmh_layernorm_bwd(int dt, int src_mode, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres, void* dx, float* dgamma, float* dbeta, int64_t rows, int C, const int* wm, const unsigned char* mask, float* dmask_token, int64_t tokens_per_sample, void* dyw, const float* dyw_scale, void* stream);
/* nmh_layernorm_bwd with the parameter gradients taken off the dependent chain: every workgroup of the launch leaves its dgamma / dbeta partial sums in
 * partials [nmh_layernorm_bwd_partial_rows(rows, C)][2C] (fp32, plain stores) instead of adding them to dgamma / dbeta with 2C same-address atomics, and
 * ONE nmh_layernorm_param_grad_reduce launch for any number of such LayerNorms -- issued wherever the caller runs its weight gradients -- adds the
 * column sums: dgamma[c] += sum_b partials[b][c], dbeta[c] += sum_b partials[b][C + c] (partial_rows = the value nmh_layernorm_bwd_partial_rows gave).
 * The input gradient dx (and dyw) are as nmh_layernorm_bwd's; no token mask (the embedding norm keeps the atomic form).  (norm1 / norm2 of a Swin
 * block, swin_mae3d.py:366-369 backward: 2 x 24 launches per step.) */
typedef struct nmh_ln_reduce_item { const float* partials; float* dgamma; float* dbeta; int64_t partial_rows; int C; int reserved; } nmh_ln_reduce_item;
NMH_API int64_t nmh_layernorm_bwd_partial_rows(int64_t rows, int C);
NMH_API int nmh_layernorm_bwd_deferred(int dt, int src_mode, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd, const void* dres, void* dx, float* partials, int64_t rows, int C, const int* wm, void* dyw, const float* dyw_scale, int64_t tokens_per_sample, void* stream);
NMH_API int nmh_layernorm_param_grad_reduce(const nmh_ln_reduce_item* items, int n, void* stream);
/* decoder1, forward, bf16: ConvTranspose3d(96 -> 48, kernel = stride = 4) (unetr_block.py:151-158) COMPOSED with the first 3x3x3 conv of the
 * residual block that follows it (unetr_block.py:35-44; swin_mae3d.py:1246-1257): the conv of the up-sampled map at fine voxel 4j + a only
 * touches 1..8 coarse cells j + n, so y1[4j + a] = sum_n x[j + n] . Wc[a][n] with 216 composed 96 x 48 blocks -- 31 instead of 133 kFLOP per
 * voxel; the up-sampled map itself is not read.  nmh_cconv_pack builds the composed weights (fragment order, nmh_cconv_pack_numel() bf16
 * elements) and the [27][48] fp32 border table from the fp32 master parameters: Wt = transp_conv.weight [96][48][4][4][4], W1 =
 * conv_block.conv1.weight [48][48][3][3][3], bt = transp_conv.bias [48]; ws = nmh_cconv_pack_ws_floats() floats of scratch (the two
 * weights transposed to contiguous rows).  nmh_cconv_fwd: x [B][v^3][96] -> y1 [B][(4v)^3][48] (v a multiple
 * of 8); y1 lacks the per-channel constant that the transpose conv's bias contributes in the interior (the affine-free InstanceNorm that
 * follows removes any such constant, like conv1's own bias) but carries its border variation; stats_acc (optional fp64 [B][48][2]) receives
 * sum / sum of squares of the outputs (fused InstanceNorm statistics, as nmh_conv3d_k3_c48).  The residual path still needs the up-sampled
 * map (nmh_upconv4_fwd below); backward: nmh_cconv_wgrad / nmh_cconv_dgrad. */
NMH_API int64_t nmh_cconv_pack_numel(void);
NMH_API int64_t nmh_cconv_pack_ws_floats(void);
NMH_API int nmh_cconv_pack(const float* Wt, const float* W1, const float* bt, void* Wcp, float* delta, float* ws, void* stream);
NMH_API int nmh_cconv_fwd(const void* x, const void* Wcp, const float* delta, void* y1, int B, int v, double* stats_acc, void* stream);
/* The CENTERED form of decoder1's conv1 -> InstanceNorm -> LeakyReLU -> conv2 (unetr_block.py:57-62), round 6.  y1 is linear in the coarse tensor x, so its mean
 * per (sample, channel) is known before y1 exists: sum over the fine voxels = sum_n S_n . M[n] + border constant, S_n = sum of x over the source cells whose
 * target cell lies in the grid, M[n] = the composed blocks summed over the phases (mean_table, [27][96][48] fp32, built by nmh_cconv_pack_centered next to the pack).
 * nmh_cconv_output_mean: x [B][v^3][96] -> mean [B][48] (class_sums: B * (27 * 96 + 48) doubles of scratch).  nmh_cconv_fwd_centered then stores z = lrelu(y1 - mean) and
 * accumulates the statistics of t = y1 - mean (stats_acc as nmh_cconv_fwd: nmh_instnorm_finalize turns them into (residual mean ~ 0, rstd)).  Since rstd > 0 commutes
 * with the LeakyReLU, lrelu(InstanceNorm(y1)) = rstd * z: the scale goes into conv2's weights per sample (nmh_conv48_pack_scaled, nmh_conv3d_k3_c48_per_sample) and the
 * stand-alone normalisation pass over the 160^3 tensor (nmh_instnorm_apply, 6.3 GB at 8 grids) is gone; the backward reads z (nmh_conv3d_k3_c48_bwd_reduce_centered,
 * nmh_instnorm_bwd_apply_bg_centered, nmh_conv3d_k3_c48_wgrad_scaled). */
NMH_API int nmh_cconv_pack_centered(const float* Wt, const float* W1, const float* bt, void* Wcp, float* delta, float* ws, float* mean_table, void* stream);
NMH_API int nmh_cconv_output_mean(const void* x, const float* mean_table, const float* delta, double* class_sums, float* mean, int B, int v, void* stream);
/* conv2 of the centered decoder1: Wk_per_sample [B][41*3*512] bf16 = the forward fragment pack of W[co][ci][tap] * rstd[b][ci] (stats = (mean, rstd) pairs
 * [B][48][2], fp32 master W [48][48][3][3][3]); nmh_conv3d_k3_c48_per_sample = nmh_conv3d_k3_c48 with the weight image of the tile's sample.
 * Backward: _bwd_reduce_centered = nmh_conv3d_k3_c48_bwd_reduce reading z for y1 (y1 - mean = z > 0 ? z : z / slope); _wgrad_scaled = nmh_conv3d_k3_c48_wgrad on
 * (dY, z) with every workgroup's partial scaled by its sample's rstd[ci] in the reduce (B in {1, 2, 4, 8} and whole tile ranges per sample: -2 otherwise);
 * nmh_instnorm_bwd_apply_bg_centered = nmh_instnorm_bwd_apply_bg reading z. */
NMH_API int nmh_conv48_pack_scaled(const float* W, const float* stats, void* Wk_per_sample, int B, void* stream);
NMH_API int nmh_conv3d_k3_c48_per_sample(const void* X, const void* Wk_per_sample, void* Y, int B, int D, int H, int W, double* stats_acc, void* stream);
NMH_API int nmh_conv3d_k3_c48_bwd_reduce_centered(const void* dY, const void* Wkd, void* dX, int B, int D, int H, int W, const void* Z, const float* stats1, float slope, double* sums, void* stream);
NMH_API int nmh_conv3d_k3_c48_wgrad_scaled(const void* dY, const void* Z, const float* stats, float* dW, float* ws, int B, int D, int H, int W, void* stream);
NMH_API int nmh_instnorm_bwd_apply_bg_centered(int dt, const void* dout, const void* z, const float* stats, const double* sums, void* dx, int B, int64_t V, int C, float slope, void* stream);
NMH_API int nmh_cconv_fwd_centered(const void* x, const void* Wcp, const float* delta, const float* mean, float slope, void* z, int B, int v, double* stats_acc, void* stream);
/* Weight gradient of decoder1's conv1 THROUGH the composition above (backward of unetr_block.py:35-44 with respect to conv1.weight; replaces the
 * 48 -> 48 nmh_conv3d_k3_c48_wgrad launch on the up-sampled map): dW1[c][co][d] += sum_a sum_ci Wt[ci][co][(a+d) mod 4] . G[a][n(a,d)][ci][c] with
 * G[a][n] = sum_j x[j+n]^T dy1[4j+a] -- the same 216 blocks as the forward, a quarter of the FLOPs, contraction over the coarse cells.
 * x [B][v^3][96], dy1 [B][(4v)^3][48] (bf16), pack_ws = the scratch nmh_cconv_pack filled in this step (holds the transposed Wt), bt = transp_conv.bias,
 * ws = nmh_cconv_wgrad_ws_floats() floats.  Exact for a dy1 whose per-sample, per-channel sums vanish -- the input gradient of the affine-free
 * InstanceNorm that conv1 feeds (the term bt[co] * sum_p dy1[p][c] is then carried by the border voxels alone, which the entry sums).
 * dWt [96][48][4][4][4] / dbt [48] (fp32, both or neither; NULL = not wanted): += the gradient of the transpose conv's own weight / bias THROUGH conv1, from
 * the same G blocks and border sums; phase: 0 = everything, 1 = the partial G blocks only (the persistent launch), 2 = the small launches behind it (reduce,
 * border sums, chain rules: they only feed weight gradients and may go to a side stream; same ws) (see nmh_cconv_dgrad: with it conv1's input gradient on the fine grid, which nmh_upconv_wgrad would need, does not exist). */
NMH_API int64_t nmh_cconv_wgrad_ws_floats(void);
NMH_API int nmh_cconv_wgrad(const void* x, const void* dy1, const float* pack_ws, const float* bt, float* dW1, float* dWt, float* dbt, float* ws, int B, int v, int phase, void* stream);
/* Input gradient THROUGH the composition: dx = ConvT^T(conv1^T(dy1)) (backward of unetr_block.py:151-158 after unetr_block.py:35-44) is a stride-4
 * convolution of the fine gradient with a 6x6x6 kernel of 48 -> 96 matrices (the transposes of the same 216 blocks): conv1's input gradient on the fine
 * grid -- a full 48 -> 48 conv pass that only fed the transpose conv's backward -- is never formed.  nmh_cconv_dgrad_pack gathers the forward's
 * fragment-ordered weights into this kernel's order (nmh_cconv_dgrad_pack_numel() bf16 elements).  nmh_cconv_dgrad: dy1 [B][(4v)^3][48] ->
 * dx [B][v^3][96] = (add ? add : 0) + gradient (add may alias dx: the part of dx that comes through the residual branch).  With this entry the
 * transpose conv's own parameter gradients through conv1 come from nmh_cconv_wgrad's G blocks: pass dWt [96][48][4][4][4] / dbt [48] (fp32, accumulated;
 * NULL = not wanted) there; the part through the residual branch stays with nmh_upconv_wgrad on the residual gradient alone. */
NMH_API int64_t nmh_cconv_dgrad_pack_numel(void);
NMH_API int nmh_cconv_dgrad_pack(const void* Wcp, void* Wdp, void* stream);
NMH_API int nmh_cconv_dgrad(const void* dy1, const void* Wdp, const void* add, void* dx, int B, int v, void* stream);
/* The residual branch of the same block, bf16: u = ConvTranspose3d(96 -> 48, kernel = stride = 4)(x) + bias (unetr_block.py:151-158, 193-200), as a
 * persistent kernel with the coarse fragments in registers and the 64 phase weights streamed through LDS (replaces nmh_upconv_fwd at this shape).
 * nmh_upconv4_pack: fragment-ordered bf16 weights (nmh_upconv4_pack_numel() elements) from pack_ws = the scratch nmh_cconv_pack filled in this step
 * (holds the transposed Wt).  nmh_upconv4_fwd: x [B][v^3][96] -> u [B][(4v)^3][48], v a multiple of 8. */
NMH_API int64_t nmh_upconv4_pack_numel(void);
NMH_API int nmh_upconv4_pack(const float* pack_ws, void* Wup, void* stream);
NMH_API int nmh_upconv4_fwd(const void* x, const void* Wup, const float* bt, void* u, int B, int v, void* stream);
/* Fused MLP branch of a Swin block, bf16 (swin_mae3d.py:352-358 torchvision MLP + :368 `x + stochastic_depth(mlp(norm2(x)))`):
 *   x2[row] = x1[row] + rowscale[row / rows_per_scale] * (gelu(LN(x1[row]) . W1^T + b1) . W2^T + b2)
 * in ONE launch: LayerNorm in the MFMA operand registers, the hidden dimension walked in chunks whose GELU output feeds the second
 * GEMM from registers -- neither the pre-activation nor the activation is written.  W1 = fc1 weight [4C][C] (bf16, row-major),
 * W2T = fc2 weight TRANSPOSED [4C][C] (bf16; pack mode 1 of nmh_pack_weights), gamma/beta/b1/b2 fp32.  mean/rstd (optional, [M])
 * receive the LayerNorm statistics.  nmh_mlp_fused_supported(C) != 0 for C in {96,128,192,256,384}; other widths return -1 (callers
 * use nmh_layernorm_fwd + 2 x nmh_gemm_nt).  Replaces nmh_layernorm_fwd + nmh_gemm_nt(act=1) + nmh_gemm_nt(resid, rowscale).
 * backward: from dx2 = dL/dx2 recomputes LN and the hidden activations and writes
 *   dx1 = dx2 + LN_backward(dh . W1)       [M][C]      hact = gelu(pre-activation)          [M][4C]  (B operand of dW2 = (s dx2)^T hact)
 *   x1n = LN(x1)                           [M][C]      dh = s (dx2 . W2) * gelu'(pre-act.)  [M][4C]  (A operand of dW1 = dh^T x1n)
 * accumulates dgamma / dbeta (fp32 atomics) and, when dyw != NULL, also stores dx1 in window order scaled by dyw_scale[row /
 * rows_per_scale] (pad rows zeroed; wm as for nmh_layernorm_bwd) -- the attention branch's incoming gradient.  The two weight /
 * bias gradients stay nmh_gemm_tn(_grouped) calls on (dx2, hact, rowscale) and (dh, x1n). */
NMH_API int nmh_mlp_fused_supported(int C);
NMH_API int nmh_mlp_fused_fwd(const void* x1, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2T, const float* b2, const float* rowscale, int rows_per_scale, void* x2, float* mean, float* rstd, int64_t M, int C, float eps, void* stream);
NMH_API int nmh_mlp_fused_bwd(const void* x1, const void* dx2, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2T, const float* rowscale, int rows_per_scale, void* dx1, void* x1n, void* hact, void* dh, float* dgamma, float* dbeta, void* dyw, const float* dyw_scale, const int* wm, int64_t M, int C, float eps, void* stream);
/* Fused Swin-block kernels, bf16, widths C = 96 NW with NW in {1, 2, 4} (stages 0-2 of swin_t / swin_s); SURVEY 2a K1 + K2:
 * `x = x + stochastic_depth(attn(norm1(x)))`, `x = x + stochastic_depth(mlp(norm2(x)))` (swin_mae3d.py:366-369) with
 * shifted_window_attention (swin_mae3d.py:27-197) and the torchvision MLP (swin_mae3d.py:352-358) each in ONE forward launch (the backward is the
 * unfused chain: nmh_gemm_nt, nmh_window_attn_bwd(_tokens), nmh_layernorm_bwd(_deferred), nmh_gemm_tn_grouped).
 * A workgroup owns 64 token rows (a 4x4x4 window / 64 consecutive tokens) and keeps them in registers as MFMA operand fragments; every one
 * of its NW waves owns a slice of the output features of every product and streams ITS weights -- a private, linear, pre-packed sequence of
 * 1-KB fragment images -- through an LDS ring with LDS-DMA (csrc/swin_block.hip).
 *   nmh_swin_pack: builds weight streams from the fp32 master parameters (once per optimizer step).  type 0: attention forward
 *     (w0 = qkv.weight [3C][C], w1 = proj.weight [C][C]); 1: MLP forward (w0 = mlp.0.weight [4C][C], w1 = mlp.3.weight [C][4C]).
 *     dst: nmh_swin_stream_numel(type, C) bf16 elements.  Up to any number of items per call.
 *   nmh_swin_attn_fwd: x [T][C] token order -> x1[tok] = x[tok] + rowscale[tok / rows_per_scale] * (proj(attn(LN1(x))) + bproj); pad -> roll ->
 *     window partition and their inverses are address arithmetic (wm as for nmh_layernorm_fwd).  Also writes, in the layouts of the unfused
 *     kernels (nmh_layernorm_fwd src_mode 1, nmh_gemm_nt, nmh_window_attn_fwd): xnw [rows][C] = LN1(x) in window order (pad rows zero), mean / rstd
 *     [T], qkv [rows][3C], o [rows][C], lse [rows * heads] -- the operands of the weight gradients and of the backward chain.
 *     token_saves != 0: xnw and o are written in TOKEN order instead ([T][C]; pad rows, which are zero / carry no gradient, are dropped): the operands of
 *     weight gradients that run on the real tokens only (with nmh_window_attn_bwd_tokens).
 *   nmh_swin_mlp_fwd: x2[row] = x1[row] + rowscale[..] * (gelu(LN2(x1) W1^T + b1) W2^T + b2); also writes x1n = LN2(x1) [M][C], the fc1
 *     pre-activation hp [M][4C], mean / rstd [M] and, when hact != NULL, gelu(hp) [M][4C] (the unfused backward's fc2 weight-gradient operand).
 *     split_ws (optional): nmh_swin_mlp_split_ws_bytes(M, C) bytes, zero before the first call and left zero by every call (calls that share it
 *     must be ordered on one stream).  When that size is > 0 (C = 384 and <= 128 row tiles: fewer workgroups than half of the CUs) and the workspace
 *     is given, two workgroups share a row tile -- half of the hidden units each, fp32 partial sums added by whichever finishes last; the sum of two
 *     terms does not depend on the arrival order, so results are reproducible. */
typedef struct nmh_swin_pack_item { const float* w0; const float* w1; void* dst; int type; int C; } nmh_swin_pack_item;
NMH_API int nmh_swin_supported(int C);
NMH_API int64_t nmh_swin_stream_numel(int type, int C);
NMH_API int nmh_swin_pack(const nmh_swin_pack_item* items, int n, void* stream);
NMH_API int nmh_swin_attn_fwd(const void* x, const float* gamma, const float* beta, const void* wstream, const float* bqkv, const float* bias_table, const float* bproj, const float* rowscale, int rows_per_scale, void* xnw, float* mean, float* rstd, void* qkv, void* o, float* lse, void* x1, const int* wm, int C, float eps, int token_saves, void* stream);
NMH_API int nmh_swin_mlp_fwd(const void* x1, const float* gamma, const float* beta, const void* wstream, const float* b1, const float* b2, const float* rowscale, int rows_per_scale, void* x2, void* x1n, void* hp, void* hact, float* mean, float* rstd, int64_t M, int C, float eps, void* split_ws, int64_t split_ws_bytes, void* stream);
NMH_API int64_t nmh_swin_mlp_split_ws_bytes(int64_t M, int C);
/* out[tok] = x[tok] + rowscale[b]*yw[window_row(tok)]: window reverse + un-roll + un-pad (:176-196) + residual + stochastic depth */
NMH_API int nmh_window_scatter_residual(int dt, const void* yw, const void* x, void* out, const float* rowscale, int C, const int* wm, void* stream);
/* dyw[window_row] = rowscale[b]*dx[tok] (0 for pad rows): adjoint of the above */
NMH_API int nmh_window_gather_scale(int dt, const void* dx, void* dyw, const float* rowscale, int C, const int* wm, void* stream);
/* softmax(q k^T / sqrt(32) + bias_table[rel_index] + shift_mask(-100)) v per (window, head): swin_mae3d.py:109-172, 200-211.
 * qkv [windows*64, 3C] window-ordered ([q|k|v], head-major), out [windows*64, C], lse [windows*heads*64]. head_dim must be 32. */
NMH_API int nmh_window_attn_fwd(int dt, const void* qkv, const float* bias_table, void* out, float* lse, int heads, int C, const int* wm, void* stream);
NMH_API int nmh_window_attn_bwd(int dt, const void* qkv, const float* bias_table, const void* dout, const float* lse, void* dqkv, float* dbias_table, int heads, int C, const int* wm, void* stream);
/* The same backward with window order confined to the kernel: dout_tok [T][C] is the TOKEN-ordered gradient of the attention output (rows of a window that
 * are pads read as zero -- the reference's x[:, :H, :W, :D] slice, swin_mae3d.py:196), and the rows of d(qkv) that belong to a token are written to
 * dqkv_tok [T][3C] at their token, so that the Linear layers either side (proj, qkv: input gradients and weight gradients) run on the T real tokens
 * instead of the padded window rows (58 % of them at 10^3 tokens in 12^3, 24 % at 5^3 in 8^3).  Pad rows' d(qkv) -- not zero: pad tokens are keys and
 * values with q = k = v = bias -- go to dqkv_pad [rows][3C] at their window row (real rows of that buffer are not touched), and
 * nmh_window_pad_rows_colsum adds their column sums to the qkv bias gradient: out[n] += sum over pad rows of x[row][n]. */
/* Forward counterparts for the UNFUSED chain (small launches, fp32 parity mode): nmh_layernorm_fwd_window_tokens = nmh_layernorm_fwd src_mode 1 with a second,
 * token-ordered copy of the normalised rows (out_tokens [T][C]); nmh_window_attn_fwd_tokens = nmh_window_attn_fwd with its output scattered to token
 * order (out_tok [T][C], pad rows dropped) -- proj is then a plain T-row nmh_gemm_nt with the residual / row-scale epilogue. */
NMH_API int nmh_layernorm_fwd_window_tokens(int dt, const void* x, void* out_window, void* out_tokens, const float* gamma, const float* beta, float eps, float* mean, float* rstd, int64_t rows, int C, const int* wm, void* stream);
NMH_API int nmh_window_attn_fwd_tokens(int dt, const void* qkv, const float* bias_table, void* out_tok, float* lse, int heads, int C, const int* wm, void* stream);
NMH_API int nmh_window_attn_bwd_tokens(int dt, const void* qkv, const float* bias_table, const void* dout_tok, const float* lse, void* dqkv_tok, void* dqkv_pad, float* dbias_table, int heads, int C, const int* wm, void* stream);
NMH_API int nmh_window_pad_rows_colsum(int dt, const void* x, int N, const int* wm, float* out, void* stream);
/* the same for n buffers of one geometry in ONE launch (xs / outs: HOST arrays of n device pointers, copied into the kernel arguments): the blocks of an
 * encoder stage, issued with the stage's grouped weight gradients */
NMH_API int nmh_window_pad_rows_colsum_grouped(int dt, const void* const* xs, float* const* outs, int n, int N, const int* wm, void* stream);

/* InstanceNorm3d (eps, no affine, biased var) + LeakyReLU(slope) + residual over channels-last [B][V][C] (unetr_block.py:57-71).
 * stats[b][c] = {mean, rstd}; scratch/sums: fp64 [B][C][2].  rmode 0: lrelu(IN(x)); 1: lrelu(IN(x)+r); 2: lrelu(IN(x)+IN(r)).
 * nmh_instnorm_bwd_apply: dr_accumulate (dr += g into an existing dr) exists for rmode 1 only; with any other rmode the call returns -2. */
NMH_API int nmh_instnorm_stats(int dt, const void* x, float* stats, double* scratch, int B, int64_t V, int C, float eps, void* stream);
NMH_API int nmh_instnorm_apply(int dt, const void* x, const float* stats, const void* r, const float* stats_r, int rmode, void* out, int B, int64_t V, int C, float slope, void* stream);
NMH_API int nmh_instnorm_bwd_reduce(int dt, const void* dout, const void* out, const void* x, const float* stats, const void* r, const float* stats_r, int rmode, double* sums, double* sums_r, int B, int64_t V, int C, float slope, void* stream);
NMH_API int nmh_instnorm_bwd_apply(int dt, const void* dout, const void* out, const void* x, const float* stats, const double* sums, const void* r, const float* stats_r, const double* sums_r, int rmode, void* dx, void* dr, int dr_accumulate, int B, int64_t V, int C, float slope, void* stream);
/* the rmode-0 apply pass with the sign taken from x (out = NULL), bf16, C = 48, as a background launch: one persistent workgroup per CU with a footprint
 * (<= 96 VGPRs, no dynamic LDS) that fits on a CU beside the persistent 48 -> 48 weight-gradient kernel -- decoder-1's InstanceNorm backward
 * (unetr_block.py:57-63 backward) issued on a forked stream next to nmh_conv3d_k3_c48_wgrad.  Bit-identical to nmh_instnorm_bwd_apply. */
NMH_API int nmh_instnorm_bwd_apply_bg(int dt, const void* dout, const void* x, const float* stats, const double* sums, void* dx, int B, int64_t V, int C, float slope, void* stream);

/* im2row of the 4x4x4 stride-4 patch conv input: x fp32 (B,4,R,R,R) -> A[(b,z,y,x)][256] (swin_mae3d.py:1120-1126) */
NMH_API int nmh_patch_embed_gather(int dt, const float* x, void* A, int B, int R, void* stream);
/* Patch embed of the KEPT tokens only (the embedding of a removed token is replaced by mask_token right after the LayerNorm, swin_mae3d.py:1375-1380: at
 * mask_ratio 0.75 three quarters of the im2row, of the GEMM rows, of the LayerNorm rows and of the weight-gradient contraction are work on values nobody reads).
 * nmh_patch_embed_kept_rows: token mask [n] (1 = removed) -> rowmap [n + 2]: the compact row of every kept token (raster order), -1 for a removed one;
 *   rowmap[n] = kept count (<= cap), rowmap[n + 1] = 1 if kept tokens did not fit into cap rows (they read -1; the caller sizes cap from the mask it drew).
 * nmh_patch_embed_gather_kept: as nmh_patch_embed_gather into A [B][cap_rows][256], rows behind the kept count zeroed.
 * nmh_patch_embed_norm_fwd_kept / _bwd_kept: nmh_layernorm_fwd / _bwd (mode 0, with pos / mask / mask_token) reading y0 [B][cap_rows][C] through rowmap and
 *   writing token rows [rows][C]; the backward writes d(y0) compact (rows behind the kept count zeroed) and adds the removed tokens' gradients to dmask_token. */
NMH_API int nmh_patch_embed_kept_rows(const unsigned char* mask, int n, int cap, int* rowmap, void* stream);
NMH_API int nmh_patch_embed_gather_kept(int dt, const float* x, void* A, int B, int R, const int* rowmap, int64_t cap_rows, void* stream);
NMH_API int nmh_patch_embed_norm_fwd_kept(int dt, const void* y0, void* tok, const float* gamma, const float* beta, float eps, float* mean, float* rstd, int64_t rows, int C,
                                          const float* pos, const unsigned char* mask, const float* mask_token, int64_t tokens_per_sample, const int* rowmap, int64_t cap_rows,
                                          void* stream);
NMH_API int nmh_patch_embed_norm_bwd_kept(int dt, const void* dtok, const void* y0, const float* gamma, const float* mean, const float* rstd, void* dy0, float* dgamma, float* dbeta,
                                          int64_t rows, int C, const unsigned char* mask, float* dmask_token, int64_t tokens_per_sample, const int* rowmap, int64_t cap_rows,
                                          void* stream);
/* Stage 0's first Swin block on the KEPT windows only.  With a mask that is constant on every 4x4x4 window of a g^3 token grid (g % 4 == 0) every removed window
 * enters the shift-0 block as 64 rows of mask_token (no position), so all removed windows of a sample leave it with the same 64 rows.  Compact layout
 * [B][cap_windows + 1][64][C]: slot k < cap_windows = the k-th kept window in raster order of windows (rows in the window's own (dz, dy, dx) order, zero rows behind
 * the kept count), slot cap_windows = 64 rows of mask_token, the representative of every removed window of the sample.  C % 8 == 0, C <= 128 (nmh_block0_supported).
 * nmh_block0_window_rows: mask [g^3] -> rowmap [g^3 + 2] with the meaning of nmh_patch_embed_kept_rows' but in window-major order (row = 64 slot + position;
 *   rowmap[g^3] = 64 x kept windows, rowmap[g^3 + 1] = 1 if they did not fit), and wmap [nW + cap_windows], nW = (g / 4)^3: wmap[w] = slot of window w or -1,
 *   wmap[nW + k] = window of slot k or -1.  The gather, GEMM and weight gradient of the patch embed take rowmap with cap_rows = 64 (cap_windows + 1).
 * nmh_block0_embed_norm_fwd: LayerNorm + pos_embed of y0 [B][cap_windows + 1][64][C] on the kept rows (the arithmetic of nmh_layernorm_fwd), zero rows behind the
 *   count, mask_token in the representative rows; mean / rstd per compact row.
 * nmh_block0_embed_norm_bwd: its backward from the compact input gradient of the block; dy0 is zero outside the kept rows; dgamma / dbeta / dmask_token (the column
 *   sum of the representative rows) += sums taken in a fixed order through partials (>= 256 * 3 C floats), no float atomics.
 * nmh_block0_expand: compact block output -> dense [B][g^3][C]; every removed window receives the representative window's rows (exact copy).
 * nmh_block0_reduce: dense gradient [B][g^3][C] -> compact: kept windows copied, representative row i = the fp32 sum of row i of every removed window of the sample
 *   (16 contiguous segments of the window range in ascending order, then the 16 partial sums in ascending order), rounded once; windows behind the count zero. */
NMH_API int nmh_block0_supported(int C);
NMH_API int nmh_block0_window_rows(const unsigned char* mask, int g, int cap_windows, int* rowmap, int* wmap, void* stream);
NMH_API int nmh_block0_embed_norm_fwd(int dt, const void* y0, void* out, const float* gamma, const float* beta, float eps, float* mean, float* rstd, const float* pos,
                                      const float* mask_token, const int* wmap, int B, int g, int cap_windows, int C, void* stream);
NMH_API int nmh_block0_embed_norm_bwd(int dt, const void* dx0, const void* y0, const float* gamma, const float* mean, const float* rstd, void* dy0, float* dgamma, float* dbeta,
                                      float* dmask_token, float* partials, int64_t partial_floats, const int* wmap, int B, int g, int cap_windows, int C, void* stream);
NMH_API int nmh_block0_expand(int dt, const void* yc, void* y, const int* wmap, int B, int g, int cap_windows, int C, void* stream);
NMH_API int nmh_block0_reduce(int dt, const void* dy, void* dyc, const int* wmap, int B, int g, int cap_windows, int C, void* stream);
/* ConvTranspose3d(kernel = stride = k) (unetr_block.py:151-158,193-198) as GEMMs with the pixel shuffle folded into the addressing,
 * channels-last.  x [B*v^3][Cin] coarse grid; cat/dcat [B*(v*k)^3][ldc] fine grid, the transpose conv occupies columns [0,Cout)
 * (the skip connection, if any, the rest).  Wt packed [(tap,co)][ci], Wd packed [ci][(tap,co)], dW fp32 [Cin][Cout][k^3]. */
NMH_API int nmh_upconv_fwd(int dt, const void* x, const void* Wt, const float* bias, void* cat, int64_t ldc, int B, int v, int k, int Cin, int Cout, void* stream);
NMH_API int nmh_upconv_dgrad(int dt, const void* dcat, int64_t ldc, const void* Wd, void* dx, int B, int v, int k, int Cin, int Cout, void* stream);
NMH_API int nmh_upconv_wgrad(int dt, const void* dcat, int64_t ldc, const void* x, float* dW, float* dbias, int B, int v, int k, int Cin, int Cout, void* stream);
/* (unfused pieces) ConvTranspose3d(k=stride) pixel shuffle + bias + channel concat with the skip (unetr_block.py:193-198) and its adjoint */
NMH_API int nmh_upconv_shuffle_fwd(int dt, const void* upre, const float* bias, const void* skip, void* out, int B, int v, int k, int Cout, void* stream);
NMH_API int nmh_upconv_shuffle_bwd(int dt, const void* dcat, void* dupre, void* dskip, float* dbias, int B, int v, int k, int Cout, int has_skip, void* stream);
/* UnetOutBlock 1x1 conv (Cd->4) fused with forward_loss (swin_mae3d.py:1513-1549).  target fp32 (B,4,R,R,R); extents [B][3]
 * valid voxels per axis (replaces the pad_tensor ones-mask, torch_utils.py:56-90); tokmask [g^3] 1 = removed token.
 * sums fp64[4] = {sum_rgb, n_occ, sum_alpha, n_removed}; losses fp32[3] = {loss, loss_rgb, loss_alpha}; pred optional (B,4,R,R,R).
 * dpred optional fp32 [B*R^3][4]: un-normalised d(loss)/d(pred) per voxel for nmh_mae_tail_bwd; sums is then fp64[8] (+ sum_v dpred). */
NMH_API int nmh_mae_loss_fwd(int dt, const void* d0, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int Cd, double* sums, float* losses, float* pred, float* dpred, void* stream);
NMH_API int nmh_mae_loss_bwd(int dt, const void* d0, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int Cd, const double* sums, void* dd0, void* dpred8, float* dWout, float* dbout, void* stream);
/* Forward of the decoder tail in one pass: d0 = lrelu(IN(y) + r) (unetr_block.py:62-71) -> 1x1 head -> loss terms
 * (swin_mae3d.py:1496-1549); arguments as nmh_instnorm_apply (rmode 1) + nmh_mae_loss_fwd.  sign_mask (optional, with bwd_sums, bf16 / 48 channels):
 * [B*R^3][8] bytes (6 used), bit j of byte c = [d0[voxel][8c + j] > 0] -- with the backward's sums taken here, the sign is all nmh_mae_tail_bwd still needs of d0:
 * given the mask it reads 8 bytes per voxel instead of the residual row (r and d0 may then both be NULL there). */
NMH_API int nmh_mae_tail_fwd(int dt, const void* y, const float* stats, const void* r, void* d0, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int C, double* sums, float* losses, float* pred, float* dpred, float slope, double* bwd_sums, unsigned char* sign_mask, void* stream);
/* The training form of nmh_mae_tail_fwd for decoder1, whose residual is r = ConvTranspose3d_{k=s=4}(xcoarse) + bt (unetr_block.py:151-158, 193-200): r is formed
 * inside the pass from the coarse tensor xcoarse [B][(R/4)^3][96] (bf16) on the matrix cores instead of being written by nmh_upconv4_fwd and read back -- one
 * 160^3 x 48 write and read less.  Wr: nmh_tail_residual_pack(pack_ws of nmh_cconv_pack) -> nmh_tail_residual_pack_numel() bf16 elements (the 64 phase
 * weights as MFMA fragments).  bf16, C = 48, R a multiple of 4 with (R/4)^3 a multiple of 16, R <= 256; dpred, bwd_sums and sign_mask are required (-4 otherwise:
 * the caller then stores r and uses nmh_mae_tail_fwd).  r enters the sum in fp32 (nmh_mae_tail_fwd reads it rounded to bf16). */
NMH_API int64_t nmh_tail_residual_pack_numel(void);
NMH_API int nmh_tail_residual_pack(const float* pack_ws, void* Wr, void* stream);
NMH_API int nmh_mae_tail_fwd_from_coarse(int dt, const void* y, const float* stats, const void* xcoarse, const void* Wr, const float* bt, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int C, double* sums, float* losses, float* pred, float* dpred, float slope, double* bwd_sums, unsigned char* sign_mask, void* stream);
/* nmh_mae_tail_fwd_from_coarse over the valid box of each sample alone: ceil(extent / 4) coarse cells per axis.  PRECONDITION: target is zero outside the
 * extents (zero-padded scenes).  d(pred) is then exactly zero in the padding and contributes nothing to the losses, their counts, or bwd_sums, so the pass
 * neither visits nor WRITES it: dpred and sign_mask keep their old content outside the box, and only nmh_mae_tail_bwd_box may read them.  Inside the box
 * every byte equals the full walk's; the sums differ by the order of their fp32 partials.  pred must be NULL (-4). */
NMH_API int nmh_mae_tail_fwd_from_coarse_box(int dt, const void* y, const float* stats, const void* xcoarse, const void* Wr, const float* bt, const float* Wout, const float* bout, const float* target, const int* extents, const unsigned char* tokmask, int B, int R, int C, double* sums, float* losses, float* pred, float* dpred, float slope, double* bwd_sums, unsigned char* sign_mask, void* stream);
/* The single apply pass of nmh_mae_tail_bwd (bwd_sums and sign_mask given, bf16, 48 channels) behind nmh_mae_tail_fwd_from_coarse_box: a voxel outside
 * its sample's box takes d(pred) = 0 without reading dpred or sign_mask there (dy = rstd (-S1/V - xhat S2/V), dr = 0, as the full walk gives).
 * extents: the same device array [B][3]; V = R^3, R a multiple of 4, R <= 256. */
NMH_API int nmh_mae_tail_bwd_box(int dt, const void* y, const float* stats, const float* dpred, const double* loss_sums, const float* Wout, double* in_sums, void* dy, void* dr, float slope, float* dWout, float* dbout, int B, int R, int C, const double* bwd_sums, const unsigned char* sign_mask, const int* extents, void* stream);
/* Backward of the decoder tail d0 = lrelu(IN(y) + r) -> 1x1 head -> loss in two elementwise passes that never materialise d(d0)
 * (swin_mae3d.py:1496-1549 + unetr_block.py:62-71 backward): d(d0) = Wout^T dpred is recomputed per element from dpred/loss_sums
 * (both from nmh_mae_loss_fwd).  in_sums[b][c] = {sum g, sum g*yhat}, dy = IN-backward, dr = g; dWout/dbout accumulate the head
 * gradients.  stats = {mean, rstd} of y.  d0 may be NULL when r (the residual input of the forward) is given: d0 is then rebuilt bit-exactly
 * from y, stats and r inside the kernel, and nmh_mae_tail_fwd need not store it either (its d0 may be NULL): one 160^3 x 48 write less.
 * bwd_sums (optional, fp64 [B*C*4 + 4*C], zeroed by nmh_mae_tail_fwd): the forward pass also takes the reductions of this backward
 * ({sum g, sum g*yhat} per (sample, channel) and the head weight gradient, RGB and alpha parts of the loss kept apart until their
 * normalisers are known); passed on to nmh_mae_tail_bwd it makes the backward a single apply pass (one 3-tensor read pass less). */
NMH_API int nmh_mae_tail_bwd(int dt, const void* d0, const void* r, const void* y, const float* stats, const float* dpred, const double* loss_sums, const float* Wout, double* in_sums, void* dy, void* dr, float slope, float* dWout, float* dbout, int B, int64_t V, int C, const double* bwd_sums, const unsigned char* sign_mask, void* stream);
/* Input pipeline in one pass (nerf_rpn/datasets.py:88-101,198-233,247-248 + torch_utils.py:56-90): one stored scene
 * rgbsigma (W,L,H,4), fp32 or uint8, already in device memory -> the (4,R,R,R) fp32 slot of the padded batch: uint8/255, optional
 * density->alpha = clip(1-exp(-exp(sigma)/100),0,1) (fp32 scenes), (W,L,H,C)->(C,W,L,H), the z-up augmentations (flags: 1 = 90-degree
 * rotation [transpose axes 0,1 then flip axis 0], 2 = flip axis 0, 4 = flip axis 1, applied in that order), zero padding at the high
 * end of each axis.  The valid extents of the result are (rot ? L : W, rot ? W : L, H). */
NMH_API int nmh_grid_prepare(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, void* stream);
/* Target side of the voxel-semantics input pipeline (nerf_rpn/datasets.py:150-167 hands the label volume to augment_rpn_inputs, whose two operations are
 * :200-201 transpose + flip and :222 flip; padding torch_utils.py:56-90): one stored label volume (W,L,H) in device memory, dt 0 fp32, 1 int32, 2 int64, 3 uint8
 * (the codes of nmh_sem_label_counts, plus uint8) -> the (R,R,R) fp32 slot of the (B,R,R,R) label batch that nmh_masked_ce_fwd and nmh_sem_eval read.
 * Value = (float)label (negative ones as they are: the loss takes label <= 0 as unlabelled); flags 1 / 2 / 4 with the meaning and order of nmh_grid_prepare, bit 8
 * ignored; zero (= unlabelled) padding at the high end of each axis.  -2: a non-positive extent, an extent of the result above R, an unknown dt. */
NMH_API int nmh_labels_prepare(int dt, const void* src, int W, int L, int H, float* dst, int R, int flags, void* stream);
/* Detection input pipeline (nerf_rpn/datasets.py:173-244, 478-524).  nmh_grid_prepare_rs: nmh_grid_prepare followed, before the padding, by
 * rotate_and_scale_scene's resample of the augmented grid (extents r0,r1,r2 = rot ? L : W, rot ? W : L, H; angle in radians): output voxel (i,j,k) inside
 * the extents is the trilinear blend (align_corners=True, taps outside [0,r) contribute 0) of the augmented grid at
 *   X = (2i/(r0-1) - 1) r0/2 (Y, Z alike);  qx = s (cos a X - sin a Y), qy = s (sin a X + cos a Y), qz = s Z;  a0 = (qx/(r0/2) + 1)/2 (r0-1) (a1, a2 alike)
 * (datasets.py:481-512).  Taps are converted (/255, alpha) before blending.  Every extent must be >= 2 (-2 otherwise).  A scene without rot-scale goes
 * through nmh_grid_prepare: angle 0, scale 1 here is still a resample (equal values up to fp32 blending with zero weights, not the same kernel).
 * nmh_boxes_augment: the box side, z_up=True, one launch for a batch.  boxes/out: [total_rows, cols] fp32 on the device, cols 6 (xmin,ymin,zmin,xmax,ymax,
 * zmax) or 7 (x,y,z,w,l,h,theta); itab [n_scenes][7] = first row, count, flags (1 rot, 2 flip 0, 4 flip 1), has_rs, e0, e1, e2 (the scene's extents after
 * rot / flips) and ftab [n_scenes][2] = angle, scale are HOST arrays, copied into the launch arguments (no H2D copy, no synchronisation); n_scenes <= 64.
 * 6 columns: rot swaps x/y and sets (xmin,xmax) = e0 - (xmax,xmin); a flip of axis a sets (min,max) = e_a - (max,min) (:208-211, 225-229).  7 columns: rot
 * swaps x/y and w/l and sets x = e0 - x, theta unchanged; a flip mirrors the centre and negates theta (:215-217, 230-233); rot-scale (7 columns only):
 * theta -= angle, dims /= scale, centre = (centre - e/2) @ (Rz(angle)/scale) + e/2, a row vector times the matrix (:514-522).  Rows of no scene are copied. */
NMH_API int nmh_grid_prepare_rs(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, float angle, float scale, void* stream);
NMH_API int nmh_boxes_augment(const float* boxes, float* out, int cols, int total_rows, int n_scenes, const int* itab, const float* ftab, void* stream);
NMH_API int nmh_bias_grad(int dt, const void* dY, float* db, int64_t M, int N, const float* rowscale, int rows_per_scale, void* stream);
NMH_API int nmh_add_inplace(int dt, void* a, const void* b, int64_t n, void* stream);
/* out = a + b (out may alias a): the sum of the two gradients of an encoder feature map that feeds both the next stage and a decoder
 * skip connection (swin_mae3d.py:1465-1470 + unetr_block.py:196-197: autograd's accumulation, as a HIP kernel). */
NMH_API int nmh_add(int dt, const void* a, const void* b, void* out, int64_t n, void* stream);
NMH_API int nmh_fill_f32(float* p, float v, int64_t n, void* stream);
/* Accumulator arena.  Every entry point that reduces into a caller-provided accumulator (InstanceNorm statistics and backward sums, the
 * fused conv statistics, loss sums, the gradient norm) clears it first with a launch of its own -- 24 launches of ~5 us on the dependent
 * chain of a training step.  After nmh_set_prezeroed_arena(base, bytes) the caller guarantees that any accumulator lying wholly inside
 * [base, base + bytes) is zero on entry (it clears the used part of the arena with ONE launch per step and never hands out a slice twice
 * between two clears), and those clearing launches are skipped; accumulators outside the range are cleared as before.
 * bytes = 0 removes the arena.  One arena per process (one process per GPU).  Reference: the reductions are ATen kernels there
 * (InstanceNorm3d, unetr_block.py:57-71; forward_loss, swin_mae3d.py:1513-1563) and allocate + clear their own workspaces. */
NMH_API int nmh_set_prezeroed_arena(void* base, int64_t bytes);
/* ---- dense-prediction heads on the pretrained encoder + decoder (nerf_rpn/model/feature_extractor.py:1898-2244 VoxelSR, 2521-2848
 * VoxelSemantics).  Their convolutions / norms / GEMMs are the entries above; these are the head-specific pieces. ----
 * nmh_grid_to_cl8: (B,4,V) fp32 NCDHW grid -> [B*V][8] channels-last in dt (channels 4..7 zero): input of `encoder1`, whose first
 *   3x3x3 conv (4 -> E/2, unetr_block.py:35-44) and 1x1x1 residual conv run on weights padded to 8 input channels (pack mode 12).
 * nmh_head_upsample_fwd: y [B*R^3][Cp] (dt, head GEMM output, first Co columns) -> pred (B,Co,Ro,Ro,Ro) fp32 with nn.Upsample(scale_factor,
 *   mode="nearest") source indices min(floorf(dst * inv_scale), R-1) (feature_extractor.py:2036,2224-2229; a 1x1x1 conv commutes with
 *   nearest upsampling, so `voxel_out` runs before it); Ro == R, inv_scale == 1: plain channels-last -> NCDHW (the semantics head).
 * nmh_head_upsample_bwd: its adjoint, g [B*R^3][Cp] (dt) = sum of dpred over the output voxels that read each source voxel (columns >= Co zero).
 * nmh_add_cols_f32: dst[m][0:C] += src[m][0:C] (row strides in elements): un-padding of gradients computed on padded operands. */
NMH_API int nmh_grid_to_cl8(int dt, const float* grid, void* out, int B, int64_t V, void* stream);
NMH_API int nmh_head_upsample_fwd(int dt, const void* y, float* pred, int B, int Co, int Cp, int R, int Ro, float inv_scale, void* stream);
NMH_API int nmh_head_upsample_bwd(int dt, const float* dpred, void* g, int B, int Co, int Cp, int R, int Ro, float inv_scale, void* stream);
NMH_API int nmh_add_cols_f32(const float* src, int64_t lds, float* dst, int64_t ldd, int64_t M, int C, void* stream);
/* VoxelSR loss (feature_extractor.py:2133-2160): loss = sum_v m (pred_rgb - target_rgb)^2 / sum_v m, m = target_alpha > 0.01; pred and
 * target (B,4,V) fp32; sums fp64[2] = {numerator, sum m}.  _bwd: dpred = gscale * d(loss)/d(pred) (alpha plane 0). */
NMH_API int nmh_voxel_sr_loss_fwd(const float* pred, const float* target, int B, int64_t V, double* sums, float* loss, void* stream);
NMH_API int nmh_voxel_sr_loss_bwd(const float* pred, const float* target, int B, int64_t V, const double* sums, float gscale, float* dpred, void* stream);
/* VoxelSemantics loss (nerf_rpn/model/metrics.py:540-553 with nn.CrossEntropyLoss(weight), feature_extractor.py:2700-2722): logits (B,K,V)
 * fp32, labels (B,V) fp32 class ids (0 = unlabelled), mask m = label > 0, cross entropy over ALL voxels of (logits*m, label*m) with
 * optional class weights [K]; sums fp64[2] = {sum w nll, sum w}; iou_sums fp64 [B][K-1][3] = {sum m p_k, #(label = k), sum_{label=k} p_k}
 * (mIoULoss_new, metrics.py:194-245); out fp32[2] = {loss, mean soft IoU}.  _bwd: dlogits = gscale * d(loss)/d(logits).  K <= 32. */
NMH_API int nmh_masked_ce_fwd(const float* logits, const float* labels, const float* class_weights, int B, int K, int64_t V, double* sums, double* iou_sums, float* out, void* stream);
NMH_API int nmh_masked_ce_bwd(const float* logits, const float* labels, const float* class_weights, int B, int K, int64_t V, const double* sums, float gscale, float* dlogits, void* stream);
/* VoxelSemantics evaluation (feature_extractor.py:2748-2806 output_metrics, metrics.py:491-518 intersectionAndUnionGPU), one read of the logits.  Inputs as
 * nmh_masked_ce_fwd (2 <= K <= 32, else -2).  out fp32[2] = {loss, mean soft IoU} by the definitions of nmh_masked_ce_fwd; p(v) = arg-max of the RAW logits over
 * all K classes, the lowest index on an exact tie; over the voxels with label > 0 and the whole batch, per class c = 1..K-1:  I = #(p == c and label == c),
 * P = #(p == c), T = #(label == c), U = P + T - I;  counts int64 [4][K-1] = {I, U, T, P};  pred_vis / target_vis int64 (B,V) = p * (label > 0), label * (label > 0);
 * totals (optional) int64 [3][K-1] += {I, U, T}.  A label >= K is a labelled voxel of no class: it can count in P, never in T or I, and weighs 0 in the loss.
 * Workspaces (written, never read back by the caller): fpart fp64 [1024][2 + 2(K-1)], ipart int64 [1024][3(K-1)]; B <= 1024, else -2.
 * Two launches, no atomics, no allocation, no host wait; every sum has a fixed order.
 * nmh_sem_label_counts: the same counts from two label arrays of n elements (dt 0 fp32, 1 int32, 2 int64; `output` plays p, `target` the label); needs ipart only. */
NMH_API int nmh_sem_eval(const float* logits, const float* labels, const float* class_weights, int B, int K, int64_t V, double* fpart, int64_t* ipart, float* out,
                         int64_t* counts, int64_t* pred_vis, int64_t* target_vis, int64_t* totals, void* stream);
NMH_API int nmh_sem_label_counts(int dt, const void* output, const void* target, int64_t n, int K, int64_t* ipart, int64_t* counts, void* stream);
/* ---- the reference's two native (CUDA) ops, both on the downstream path that the pretrained encoder + FPN feeds ----
 * Rotated 3-D RoIAlign (nerf_rpn/model/rotated_align/src/cuda_3d/ROIAlignRotated3D_cuda.cu RoIAlignRotated3DForward / ...BackwardFeature, bound by
 * rotated_align/roi_align_rotate_3d.py:10-47, used by detector.py:192-193).  rois [N][8] fp32 = {batch index, centre (w,l,h), size (w,l,h), angle in
 * degrees}; centre and size are multiplied by spatial_scale, sizes clamped to >= 1; a bin is the mean over sampling_ratio^3 trilinear samples
 * (sampling_ratio <= 0: ceil(size / pooled) per axis), rotated about the h axis.
 *   layout 0: input channels-last (B,W,L,H,C) in dt (0 fp32, 1 bf16; fp32 accumulation), out [N,PW,PL,PH,C] in dt; C % 8 == 0, else -2;
 *   layout 1: input NCWLH fp32 (the reference's layout), out [N,C,PW,PL,PH] fp32; dt must be 0.
 * _bwd: dinput (the input's shape, ALWAYS fp32, zeroed by the caller) += the adjoint of dout (out's shape and type), by fp32 atomic adds.
 * Voxel (x,y,z) is element (x*L + y)*H + z.  The reference indexes (x*W + y)*L + z in the forward and mixes x*L / x*W in the backward, which is the
 * same element only when W == L == H: identical to the reference on cubic maps, correct on the rest.  An ROI whose batch index is outside [0, B)
 * gives zeros and no gradient.  N == 0 returns 0 without a launch. */
NMH_API int nmh_roi_align_rotated_3d_fwd(int layout, int dt, const void* input, const float* rois, void* out, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH, float spatial_scale, int sampling_ratio, void* stream);
NMH_API int nmh_roi_align_rotated_3d_bwd(int layout, int dt, const void* dout, const float* rois, float* dinput, int N, int B, int W, int L, int H, int C, int PW, int PL, int PH, float spatial_scale, int sampling_ratio, void* stream);
/* Vertex sort of the oriented-box IoU losses (nerf_rpn/model/rotated_iou/cuda_op/sort_vert_kernel.cu:42-130, bound by cuda_op/sort_vert.cpp and
 * cuda_ext.py:7-22, called from box_intersection_2d.py:141): vertices [B,N,M,2] fp32 centred on the polygon, mask [B,N,M] one byte each,
 * num_valid [B,N] -> idx [B,N,9]: the masked vertices in increasing polar angle over [0, 2 pi), entry num_valid repeats entry 0, the rest (and
 * all nine when num_valid < 3) are the first unmasked j >= 8; two identical boxes (num_valid == 8, entries 0-3 again in 4-7) give entry 4 = entry 0
 * and pads after it.  A vertex with y == 0, where the reference's comparison returns nothing, sorts by its angle (x > 0: 0, x < 0: pi).
 * 9 <= M <= 32, else -4.  B*N == 0 returns 0 without a launch. */
NMH_API int nmh_sort_vertices(const float* vertices, const unsigned char* mask, const int* num_valid, int* idx, int B, int N, int M, void* stream);
/* ---- oriented 3-D box IoU / GIoU / DIoU losses, all-pairs IoU and rotated NMS (csrc/rotated_iou.hip) ----
 * Boxes are fp32 rows (x, y, z, w, l, h, theta), theta in RADIANS about the third axis (the RoIAlign entries above take degrees).
 * Paired losses (nerf_rpn/model/rotated_iou/oriented_iou_loss.py:82-148 cal_iou_3d / cal_giou_3d / cal_diou_3d, over box_intersection_2d.py:11-176 and
 * min_enclosing_box.py:25-166; called from fcos/loss.py:135-171 and rpn.py:143-156).  mode: 0 IoU, 1 GIoU "smallest", 2 GIoU "aligned", 3 DIoU "smallest",
 * 4 DIoU "aligned".  box1, box2 [npairs][7] -> iou, u3d, z_range, loss, w_c, h_c [npairs] and corners1, corners2 [npairs][4][2] (the BEV corners of
 * box2corners_th); every output but iou may be NULL, loss is required in modes 1-4 and untouched in mode 0.
 * _bwd recomputes the geometry from the boxes: g_iou, g_u3d, g_loss [npairs] (NULL = zero; bit 0 / 1 / 2 of g_one set:
 * that gradient is ONE float for all pairs, the expanded gradient of a sum()) -> dbox1, dbox2 [npairs][7], written not added; a NULL dbox
 * skips that side.  A pair without BEV overlap gets an exactly zero gradient from the intersection area.  npairs == 0 returns 0 without a launch. */
NMH_API int nmh_obb_iou_fwd(int mode, const float* box1, const float* box2, int64_t npairs, float* iou, float* u3d, float* z_range, float* loss, float* w_c, float* h_c, float* corners1, float* corners2, void* stream);
NMH_API int nmh_obb_iou_bwd(int mode, const float* box1, const float* box2, int64_t npairs, const float* g_iou, const float* g_u3d, const float* g_loss, int g_one, float* dbox1, float* dbox2, void* stream);
/* box_iou_3d (nerf_rpn/model/fcos/utils.py:212-255, model/utils.py:215-412): boxes1 [N][ncols] x boxes2 [M][ncols] -> iou [N][M], without the N x M x 7
 * repeat.  ncols 7: oriented boxes as above; ncols 6: (x1,y1,z1,x2,y2,z2) with the closed form of _box_inter_union_3d (fcos/utils.py:285-297).  A pair
 * without z overlap or BEV overlap is exactly 0.  N <= 1048560. */
NMH_API int nmh_obb_iou_pairwise(int ncols, const float* boxes1, const float* boxes2, int N, int M, float* iou, void* stream);
/* nms / batched_nms (nerf_rpn/model/fcos/utils.py:109-158): boxes [N][ncols] already ordered by descending score, category [N] int32 or NULL.
 * _mask: mask [N][ceil(N/64)] 64-bit words, bit k of word (i, j) = iou(i, 64 j + k) > iou_threshold and 64 j + k > i (and equal categories);
 * words with j < floor(i / 64) are zero by definition, never read by _scan and not written (only the upper triangle of
 * 64 x 64 blocks is launched): a caller that reads the mask itself must skip or clear them.
 * _scan: the greedy walk over the rows on the device: keep [N] int32 receives the kept positions in order, count [1] their number.  N <= 16384, else -4. */
NMH_API int nmh_obb_nms_mask(int ncols, const float* boxes, const int* category, int N, float iou_threshold, uint64_t* mask, void* stream);
NMH_API int nmh_obb_nms_scan(const uint64_t* mask, int N, int* keep, int* count, void* stream);
/* ---- FCOS target assignment and training losses (csrc/fcos.hip; semantics and the dense layout are stated in that file's header) ----
 * Common arguments.  level_dims: HOST int [nlevels][4] = (w, l, h, stride), 1 <= nlevels <= 4; N scenes, 1 <= N <= 64; else -4.  Level k has n_k = w l h
 * locations per scene; dense index p = N (n_0 + .. + n_{k-1}) + scene n_k + location, P = N sum n_k.  "Level tables" are HOST arrays of nlevels DEVICE
 * pointers to the head's own per-level tensors, (N, 1, w, l, h) for the logits and (N, 6|8, w, l, h) for the regression, read and differentiated in place.
 * scalars: DEVICE float [2] = (valid positives, sum of their centerness targets).  partials: DEVICE float workspace [2 nmh_fcos_num_blocks()].
 * world = world_size >= 1.  Every reduction is per-workgroup partials plus one fixed-order pass: deterministic, no atomics.  Nothing waits on the host. */
NMH_API int64_t nmh_fcos_num_blocks(int nlevels, const int* level_dims, int N);
/* prepare_targets, compute_targets_for_locations[_obb], get_sample_region, compute_centerness_targets (nerf_rpn/model/fcos/loss.py:210-445) with
 * compute_locations / compute_padding_masks (fcos/fcos.py:282-299) and encode_fcos_obb (fcos/utils.py:64-105).  boxes [box_offsets[N]][ncols] DEVICE,
 * ncols 6 (x0,y0,z0,x1,y1,z1) or 7 (x,y,z,w,l,h,theta); box_offsets HOST int [N+1], ascending from 0.  Validity: masks (level table of one byte per
 * location, (N, w, l, h)) if given, else location < grid_sizes [N][3] (DEVICE int) if given, else all valid.  radius = center_sampling_radius (<= 0: none).
 * -> labels [P] (0 / 1), targets [P][6|8], gt_index [P] (row within the scene, -1: none), ctr_targets [P], valid [P] bytes, scalars [2]. */
NMH_API int nmh_fcos_assign(int nlevels, const int* level_dims, int N, int ncols, const float* boxes, const int* box_offsets, const int* grid_sizes, const unsigned char* const* masks, float radius, int norm_targets, float* labels, float* targets, int* gt_index, float* ctr_targets, unsigned char* valid, float* partials, float* scalars, void* stream);
/* torchvision.ops.sigmoid_focal_loss(alpha 0.25, gamma 2, reduction "sum") over the valid locations / max(scalars[0] / world, 1) (fcos/loss.py:538-542),
 * logits read through the level table cls (C = 1) -> loss [1].  _bwd: dcls (level table, the logits' layout) = g_loss[0] d loss / d logit, every
 * element written (0 where invalid); g_loss NULL = zero. */
NMH_API int nmh_fcos_focal_fwd(int nlevels, const int* level_dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world, float* partials, float* loss, void* stream);
NMH_API int nmh_fcos_focal_bwd(int nlevels, const int* level_dims, int N, const float* const* cls, const float* labels, const unsigned char* valid, const float* scalars, float world, const float* g_loss, float* const* dcls, void* stream);
/* Regression and centerness losses on the valid positives, densely masked (fcos/loss.py:544-577): ncols 6: IOULoss (loss.py:77-132), loss_type 0 iou,
 * 1 linear_iou, 2 giou; ncols 8: RotatedIOULoss (loss.py:135-171) over decode_fcos_obb (fcos/utils.py:12-61), loss_type 0 iou, 1 linear_iou, 2 giou, 3 diou
 * ("smallest" enclosing forms), add_l1: SmoothL1 on columns 6:8 (loss.py:570-577); each weighted by the centerness target and divided by
 * scalars[1] / world (0 if scalars[1] == 0) -> reg_loss [1]; BCE-with-logits of the centerness logits against the centerness targets /
 * max(scalars[0] / world, 1) -> ctr_loss [1].  _bwd: dreg, dctr (level tables in the inputs' layouts) = g_reg[0] d reg_loss + g_ctr[0] d ctr_loss, by hand
 * through the pair geometry and the decode; every element written, exactly 0 where label == 0 or invalid; NULL g = zero. */
NMH_API int nmh_fcos_pos_fwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels, const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss, void* stream);
NMH_API int nmh_fcos_pos_bwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, const float* const* reg, const float* const* ctr, const float* labels, const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr, float* const* dreg, float* const* dctr, void* stream);
/* The same two losses with the 2-D projection term of compute_2d_projection_loss (fcos/loss.py:447-475, 579-585; csrc/proj2d.hpp): ncols must be 8 and
 * proj2d_weight >= 0, else -4.  Every valid positive's term gains proj2d_weight T / 160 / 16 before the centerness weight, T between the decodes of its prediction
 * and of its target at location zero under the four cameras of get_w2cs(160) (the reference's literal, whatever the scene size).  Everything else, the
 * centerness loss's bits included, as nmh_fcos_pos_fwd / _bwd. */
NMH_API int nmh_fcos_pos2d_fwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr, const float* labels, const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, float* partials, float* reg_loss, float* ctr_loss, void* stream);
NMH_API int nmh_fcos_pos2d_bwd(int nlevels, const int* level_dims, int N, int ncols, int loss_type, int add_l1, float proj2d_weight, const float* const* reg, const float* const* ctr, const float* labels, const float* targets, const float* ctr_targets, const unsigned char* valid, const float* scalars, float world, const float* g_reg, const float* g_ctr, float* const* dreg, float* const* dctr, void* stream);
/* encode_fcos_obb / decode_fcos_obb (fcos/utils.py:64-105, 12-61) on their own: locations [n][3], boxes [n][7] -> out [n][8]; locations [n][3],
 * regression [n][8] -> boxes [n][7] (theta by atan2); _bwd: gbox [n][7] -> dregression [n][8] (the locations' gradient is gbox[:, :3]).  n == 0: no launch. */
NMH_API int nmh_fcos_obb_encode(const float* locations, const float* boxes, int64_t n, float* out, void* stream);
NMH_API int nmh_fcos_obb_decode_fwd(const float* locations, const float* regression, int64_t n, float* boxes, void* stream);
NMH_API int nmh_fcos_obb_decode_bwd(const float* regression, const float* gbox, int64_t n, float* dregression, void* stream);
/* ---- FCOS inference post-processing (csrc/fcos_post.hip; semantics, the stated tie rules and the slot layout are in that file's header) ----
 * FCOSPostProcessor (nerf_rpn/model/fcos/inference.py:11-195).  level_n: HOST int [nlevels] = locations n_k per level and scene, 1 <= nlevels <= 4; N scenes,
 * 1 <= N <= 64; pre_nms_top_n >= 1; cap = sum over the levels of min(pre_nms_top_n, n_k) <= 16384; else -4 (nmh_fcos_post_cap: -1).  Level tables as above.
 * ncols 6: regression (N, 6, ..), boxes (x0,y0,z0,x1,y1,z1), rows of 1 + 6 floats; ncols 8: regression (N, 8, ..), boxes (x,y,z,w,l,h,theta), rows of 1 + 7;
 * the first float of a row is the level index.  Nothing waits on the host; integer atomics only where their order cannot matter. */
NMH_API int64_t nmh_fcos_post_cap(int nlevels, const int* level_n, int N, int pre_nms_top_n);
/* forward_for_single_feature_map (inference.py:48-129) with clip_boxes_to_mesh / remove_small_boxes (fcos/utils.py:161-209) and decode_fcos_obb
 * (fcos/utils.py:12-61), every (level, scene) in one launch.  locations: level table of [n_k][3]; masks: level table of one byte per location (N, n_k) or NULL;
 * grid_sizes DEVICE int [N][3], required for ncols 6 (the clip), unused for 8.  keys: DEVICE workspace [N sum n_k] uint32.
 * -> pre_boxes [N][cap][1+6|7], pre_scores [N][cap] (level k's slots start at sum of min(pre_nms_top_n, n_j), j < k; a slot that is unused or whose box is
 * smaller than min_size has score -1), pre_counts [nlevels][N] = boxes with a score. */
NMH_API int nmh_fcos_post_select(int nlevels, const int* level_n, int N, int ncols, int pre_nms_top_n, const float* const* cls, const float* const* reg, const float* const* ctr, const float* const* locations, const unsigned char* const* masks, const int* grid_sizes, float pre_nms_thresh, float min_size, uint32_t* keys, float* pre_boxes, float* pre_scores, int* pre_counts, void* stream);
/* select_over_all_levels (inference.py:164-195) over nms (fcos/utils.py:109-124), every scene in one mask launch and one scan launch.  sorted_scores, order
 * [N][cap]: the stable descending sort of pre_scores along cap and its int64 indices.  mask: DEVICE workspace [N][cap][ceil(cap/64)] 64-bit words;
 * keep: DEVICE workspace [N][cap] int.  post_nms_top_n <= 0: no cut.  -> boxes [N][cap][1+6|7], scores [N][cap] in decreasing score, rows past counts[b]
 * zero; counts [N]. */
NMH_API int nmh_fcos_post_nms(int nlevels, const int* level_n, int N, int ncols, int pre_nms_top_n, const float* pre_boxes, const float* sorted_scores, const int64_t* order, const int* pre_counts, float nms_thresh, int post_nms_top_n, uint64_t* mask, int* keep, float* boxes, float* scores, int* counts, void* stream);
/* ---- RPN anchor target assignment, sampling and training losses (csrc/rpn.hip; semantics, tie rules and the layouts are stated in that file's header) ----
 * RegionProposalNetwork.assign_targets_to_anchors / compute_loss (nerf_rpn/model/rpn.py:240-290, 389-419) with Matcher and
 * BalancedPositiveNegativeSampler (model/utils.py:35-211), AnchorGenerator3D (anchor.py) and the coders' encode (coder/).
 * Common arguments.  level_dims: HOST int [nlevels][7] = (W, H, D, stride_x, stride_y, stride_z, A), 1 <= nlevels <= 4, 1 <= A <= 32; N scenes, 1 <= N <= 64;
 * else -4 (nmh_rpn_num_blocks: -1).  Level k has W H D A anchors per scene, anchor ((w H + h) D + d) A + a; a scene's n anchors are its levels concatenated;
 * the dense index is scene n + anchor.  base_half: HOST float [sum A][3], the half extents of the base anchors level by level (> 0).  "Level tables" are
 * HOST arrays of nlevels DEVICE pointers to the head's per-level tensors, (N, A, W, H, D) objectness and (N, A 6|8, W, H, D) regression, channel a C + c,
 * read and differentiated in place.  Nothing waits on the host; atomics only on maxima and integer counts, whose results do not depend on order. */
NMH_API int64_t nmh_rpn_num_blocks(int nlevels, const int* level_dims, int N);
/* boxes [box_offsets[N]][ncols] DEVICE, ncols 6 (x0,y0,z0,x1,y1,z1) or 7 (x,y,z,w,l,h,theta; matched through obb2hbb_3d); box_offsets HOST int [N+1],
 * ascending from 0.  ori_sizes DEVICE int [N][3] or NULL: an anchor at grid index >= ceil(ori / stride) on any axis is padding.  gt_max: DEVICE workspace
 * [box_offsets[N]] uint32 (may be NULL without boxes).  -> labels [N][n] (1 / 0 / -1), matched_idxs [N][n] (box row within the scene, -1, -2),
 * targets [N][n][6|8] (the encode of box max(matched, 0); zeros in a scene without boxes). */
NMH_API int nmh_rpn_assign(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* boxes, const int* box_offsets, const int* ori_sizes, float fg_iou_thresh, float bg_iou_thresh, uint32_t* gt_max, float* labels, int* matched_idxs, float* targets, void* stream);
/* labels [N][n] -> flags [N][n] bytes (0 unsampled, 1 positive, 2 negative), counts [N][2] = (num_pos, num_neg) with num_pos = min(#(label >= 1), want_pos),
 * num_neg = min(#(label == 0), batch - num_pos).  rng_state DEVICE int64 [2] = (seed, counter); the counter is incremented by the call's last launch. */
NMH_API int nmh_rpn_sample(int N, int64_t n, const float* labels, int batch, int want_pos, int64_t* rng_state, unsigned char* flags, int* counts, void* stream);
/* ncols 6 | 8 regression values per anchor.  partials: DEVICE float workspace [3 nmh_rpn_num_blocks()].  -> scalars DEVICE float [3] = (mean over flags != 0
 * of BCE-with-logits(objectness, flag == 1), sum over flags == 1 of smooth-L1(beta 1/9)(regression - targets) / #(flags != 0), #(flags != 0)); the losses
 * are 0 without a sampled anchor.  _bwd: dobj, dreg (level tables in the inputs' layouts) = g_obj[0] d scalars[0] and g_reg[0] d scalars[1], every element
 * written, exactly 0 where flag == 0; NULL g = zero. */
NMH_API int nmh_rpn_loss_fwd(int nlevels, const int* level_dims, int N, int ncols, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* targets, float* partials, float* scalars, void* stream);
NMH_API int nmh_rpn_loss_bwd(int nlevels, const int* level_dims, int N, int ncols, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* targets, const float* scalars, const float* g_obj, const float* g_reg, float* const* dobj, float* const* dreg, void* stream);
/* The IoU-type box regression losses of the oriented RPN: RotatedIOULoss over the decoded proposals (nerf_rpn/model/rpn.py:133-164, 400-417) with
 * MidpointOffsetCoder.decode_single / delta_sp2bbox (coder/midpoint_offset_coder.py:160-223) and rectpoly2obb / regular_obb (coder/misc.py:5-43), differentiated
 * by hand.  ncols must be 8; loss_type 0 iou, 1 linear_iou, 2 giou, 3 diou; else -4.  boxes DEVICE [box_offsets[N]][7] (may be NULL without boxes), box_offsets
 * HOST int [N+1], ori_sizes DEVICE int [N][3] or NULL and matched_idxs DEVICE int [N][n] as in nmh_rpn_assign; partials as in nmh_rpn_loss_fwd.  Only the lanes
 * with flag == 1 decode: box term (A = the decode of the anchor's 8 deltas, B = box row max(matched, 0) of the scene) -log((inter3d + 1) / (u3d + 1)),
 * 1 - that ratio, or the GIoU / DIoU loss over the smallest enclosing rectangle.  -> scalars [3] = (the objectness loss of nmh_rpn_loss_fwd, same bits;
 * sum of the box terms / #(flags != 0); #(flags != 0)).  A flagged positive in a scene without boxes or in the padding contributes 0.  _bwd: as
 * nmh_rpn_loss_bwd; dreg is exactly 0 where flag != 1. */
NMH_API int nmh_rpn_iou_loss_fwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, float* partials, float* scalars, void* stream);
NMH_API int nmh_rpn_iou_loss_bwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* scalars, const float* g_obj, const float* g_reg, float* const* dobj, float* const* dreg, void* stream);
/* The two kinds of loss above with the 2-D projection term, the third return of compute_loss (rpn.py:421-453; csrc/proj2d.hpp).  nmh_rpn_loss2d_*: the
 * smooth-L1 box loss, ncols 6 (boxes [.][6]) or 8 (boxes [.][7]); nmh_rpn_iou_loss2d_*: the IoU types, ncols 8.  Arguments as in the entries above, and
 * cams: HOST float [48] = the four cameras as fused 3x4 matrices K [R|t], row-major (nmh_proj2d_cameras(res) gives the reference's); res > 0: the divisor,
 * max(mesh_size).  partials: DEVICE float workspace [5 nmh_rpn_num_blocks()].  -> scalars DEVICE float [5] = (objectness loss, box loss, #(flags != 0): the
 * bits of the entries above; sum over flags == 1 of T / P / res, 0 if P == 0; P = #(flags == 1)), T between the unclipped decode of the anchor's deltas and its
 * box row max(matched, 0).  A flagged positive in a scene without boxes or in the padding counts in P and contributes 0.  _bwd: dobj, dreg =
 * g_obj[0] d scalars[0] + g_reg[0] d scalars[1] + g_2d[0] d scalars[3], every element written exactly once; NULL g = zero. */
NMH_API int nmh_rpn_loss2d_fwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* targets, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams, float res, float* partials, float* scalars, void* stream);
NMH_API int nmh_rpn_loss2d_bwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* targets, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams, float res, const float* scalars, const float* g_obj, const float* g_reg, const float* g_2d, float* const* dobj, float* const* dreg, void* stream);
NMH_API int nmh_rpn_iou_loss2d_fwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams, float res, float* partials, float* scalars, void* stream);
NMH_API int nmh_rpn_iou_loss2d_bwd(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int loss_type, const float* const* objectness, const float* const* regression, const unsigned char* flags, const float* boxes, const int* box_offsets, const int* ori_sizes, const int* matched_idxs, const float* cams, float res, const float* scalars, const float* g_obj, const float* g_reg, const float* g_2d, float* const* dobj, float* const* dreg, void* stream);
/* ---- The 2-D projection regression term on rows of boxes (csrc/proj2d.hip, csrc/proj2d.hpp) ----
 * compute_2d_projection_loss of the reference's two detectors (rpn.py:421-453, fcos/loss.py:447-475) before weighting and normalisation.  pred, target DEVICE
 * [n][ncols], ncols 6 (x0,y0,z0,x1,y1,z1) or 7 (x,y,z,w,l,h,theta), else -4; cams HOST float [48] as above.  -> terms [n]: the sum over four cameras, two
 * opposite corners and two pixel coordinates of smooth-L1(beta 1/9)(uv_pred - uv_target).  _bwd: dpred [n][ncols] = g_terms[row] d terms[row] / d pred.
 * n == 0: no launch.  nmh_proj2d_cameras: HOST only, cams [48] = the cameras of get_w2cs(res) (rpn.py:58-85) times K = [[600,0,320],[0,600,240],[0,0,1]]. */
NMH_API int nmh_proj2d_cameras(float res, float* cams);
NMH_API int nmh_proj2d_fwd(const float* pred, const float* target, int64_t n, int ncols, const float* cams, float* terms, void* stream);
NMH_API int nmh_proj2d_bwd(const float* pred, const float* target, const float* g_terms, int64_t n, int ncols, const float* cams, float* dpred, void* stream);
/* ---- RPN proposals (csrc/rpn_post.hip; semantics, the stated tie, order and NaN rules and the slot layout are in that file's header) ----
 * The inference half of RegionProposalNetwork.forward (nerf_rpn/model/rpn.py:292-370, 507-512): box_coder.decode_list, _get_top_n_idx and filter_proposals over
 * clip_boxes_to_mesh, remove_small_boxes and batched_nms (model/utils.py).  level_dims, base_half and the level tables as for the entries above.  pre_nms_top_n >= 1;
 * level k keeps t_k = min(pre_nms_top_n, n_k) anchors, cap = sum t_k <= 16384, else -4 (nmh_rpn_post_cap, nmh_rpn_post_mask_words: -1).  ncols 6: regression
 * (N, A 6, ..), boxes (x0,y0,z0,x1,y1,z1); ncols 8: regression (N, A 8, ..), boxes (x,y,z,w,h,d,theta).  Nothing waits on the host. */
NMH_API int64_t nmh_rpn_post_cap(int nlevels, const int* level_dims, int N, int pre_nms_top_n);
/* 64-bit words of the suppression workspace of N scenes: N times the sum over the levels of t_k ceil(t_k / 64). */
NMH_API int64_t nmh_rpn_post_mask_words(int nlevels, const int* level_dims, int N, int pre_nms_top_n);
/* AABBCoder / MidpointOffsetCoder.decode_single of every anchor, not clipped -> boxes [N][n][6|7] in the anchor order of nmh_rpn_assign. */
NMH_API int nmh_rpn_decode(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, const float* const* regression, float* boxes, void* stream);
/* Every (level, scene) in one launch.  ori_sizes DEVICE int [N][3] or NULL (anchors in the padding are masked: below every logit, score 0); mesh_size HOST int [3].
 * -> pre_keys [N][cap] int64 sort keys (high word nlevels - 1 - level; low word 0: empty slot, 1: masked anchor, else the order-preserving transform of the logit),
 * pre_boxes [N][cap][6|7], pre_scores [N][cap] (sigmoid), pre_index [N][cap] (anchor index within the scene), pre_counts [nlevels][N] filled slots. */
NMH_API int nmh_rpn_post_select(int nlevels, const int* level_dims, const float* base_half, int N, int ncols, int pre_nms_top_n, const float* const* objectness, const float* const* regression, const int* ori_sizes, const int* mesh_size, float score_thresh, float min_size, int64_t* pre_keys, float* pre_boxes, float* pre_scores, int* pre_index, int* pre_counts, void* stream);
/* sorted_keys, order [N][cap]: the stable descending sort of pre_keys along cap and its int64 indices.  mask: DEVICE workspace of nmh_rpn_post_mask_words() words; keep:
 * DEVICE workspace [N][cap] int.  post_nms_top_n >= 1.  -> boxes [N][cap][6|7], scores, levels, index [N][cap] in descending logit (ties: the lower slot), the first
 * min(post_nms_top_n, survivors) rows; rows past counts[b] are zero. */
NMH_API int nmh_rpn_post_nms(int nlevels, const int* level_dims, int N, int ncols, int pre_nms_top_n, const float* pre_boxes, const float* pre_scores, const int* pre_index, const int64_t* sorted_keys, const int64_t* order, const int* pre_counts, float nms_thresh, int post_nms_top_n, uint64_t* mask, int* keep, float* boxes, float* scores, int* levels, int* index, int* counts, void* stream);
/* ---- RoI stage of the two-stage detector (nerf_rpn/model/detector.py; kernels and semantics: csrc/roi_head.hip) ----
 * Proposal targets: ProposalTargetLayer._sample_rois_pytorch (detector.py:60-167) over batched_box_iou (model/utils.py:371-458).  boxes [N][cap][ncols],
 * levels [N][cap], counts [N] are the dense results of nmh_rpn_post_nms; gt [G][ncols] with gt_labels [G] fp32 and HOST box_offsets [N+1].  Matching
 * (max IoU, ties to the lowest box) -> max_iou, arg [N][cap].  is_sample: rng_state (seed, counter; the counter advances) drives the device sampler
 * (foreground without, background with replacement; lists: workspace [N][2][cap]) -> keep [N][R], counts2 [N][2]; rng_state NULL: keep and counts2
 * are the caller's.  Evaluation: R == cap, keep[r] = r below counts.  Then labels [N][R], rois [N][R][1+ncols] (level, box), gt_rois [N][R][ncols];
 * keep -1: label -1 and zeros. */
NMH_API int nmh_roi_targets(int N, int cap, int ncols, int R, int is_sample, const float* boxes, const int* levels, const int* counts, const float* gt, const float* gt_labels, const int* box_offsets, int want_fg, float fg_threshold, float bg_threshold, int64_t* rng_state, float* max_iou, int* arg, int* lists, int* keep, int* counts2, float* labels, float* rois, float* gt_rois, void* stream);
/* LevelMapper.__call__ (level_mapper.py:47-59), the remap branch of ROIPool.forward (detector.py:222-236): boxes [M][stride], the box in the last ncols
 * columns -> levels [M] = clamp(floor(canonical_level + log2(cbrt(b3 b4 b5) / canonical_scale) + eps), k_min, k_max) - k_min. */
NMH_API int nmh_roi_level_map(int64_t M, const float* boxes, int stride, int ncols, int k_min, int k_max, float canonical_scale, float canonical_level, float eps, int* levels, void* stream);
/* ROIPool.normal_forward (detector.py:407-438, ncols 6) and ROIPool.rotated_forward (detector.py:264-404, ncols 7) with 'pooling': the per-RoI crop or
 * rotated 8-corner grid and the zero-padded nn.MaxPool3d, all scenes and levels in one launch.  maps: per level (N, C, W, H, D) fp32; level_dims HOST
 * [nlevels][3]; scales HOST [nlevels]; rois [N R][1+ncols]; level_override [N R] or NULL -> out, argmax [N R][C][ow][oh][od] (argmax -1: a zero won). */
NMH_API int nmh_roi_pool_fwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps, const float* rois, const int* level_override, float* out, int* argmax, void* stream);
/* Its adjoint with respect to the maps (autograd through the same lines): fp32 atomic adds into dmaps, which the caller zeroed; a NULL level is skipped. */
NMH_API int nmh_roi_pool_bwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const int* argmax, const float* rois, const int* level_override, float* const* dmaps, void* stream);
/* ROIPool.rotated_forward (detector.py:264-404) with 'interpolation', ncols 7 only (else -4): the rotated 8-corner grid of nmh_roi_pool_fwd, resampled to
 * (ow, oh, od) as F.interpolate(mode="trilinear", align_corners=True) does, all scenes and levels in one launch.  Arguments as nmh_roi_pool_fwd without
 * the argmax -> out [N R][C][ow][oh][od]; a level outside 0 .. nlevels-1 gives zeros. */
NMH_API int nmh_roi_interp_fwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* const* maps, const float* rois, const int* level_override, float* out, void* stream);
/* Its adjoint with respect to the maps (autograd through detector.py:264-404), the geometry formed again from the RoIs: fp32 atomic adds into dmaps, which the
 * caller zeroed; a NULL level is skipped. */
NMH_API int nmh_roi_interp_bwd(int nlevels, const int* level_dims, const float* scales, int N, int C, int R, int ncols, int ow, int oh, int od, float enlarge, const float* dout, const float* rois, const int* level_override, float* const* dmaps, void* stream);
/* Classification_Model.compute_loss (detector.py:536-559) with the targets of box_coder.encode_single (detector.py:616; coder/rotated_coder.py:19-55,
 * coder/AABB_coder.py:7-56): cross-entropy over rows with 0 <= label < n_classes, smooth-L1 (beta 1/9) over rows with label > 0, in fixed order.
 * rois [M][roi_stride], the box in the last ncols columns.  -> targets [M][ncols], scalars [4] = (loss_objectness, loss_rpn_box_reg, valid rows,
 * positive rows); partials: 4 * nmh_roi_loss_blocks(M) floats. */
NMH_API int64_t nmh_roi_loss_blocks(int64_t M);
NMH_API int nmh_roi_loss_fwd(int64_t M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* rois, int roi_stride, const float* gt_rois, float* targets, float* partials, float* scalars, void* stream);
/* Its backward (autograd through detector.py:536-559): every element of dscores [M][n_classes] and ddeltas [M][ncols] in one pass. */
NMH_API int nmh_roi_loss_bwd(int64_t M, int n_classes, int ncols, const float* scores, const float* deltas, const float* labels, const float* targets, const float* scalars, const float* g_obj, const float* g_reg, float* dscores, float* ddeltas, void* stream);
/* RotatedCoder.decode_single (coder/rotated_coder.py:57-121) / AABBCoder.decode_single (coder/AABB_coder.py:86-137), detector.py:609-611. */
NMH_API int nmh_roi_decode(int64_t M, int ncols, const float* deltas, const float* rois, int roi_stride, float* boxes, void* stream);
/* ---- RoI post-processing (Trainer.filter_proposals, nerf_rpn/run_rpn_detect.py:403-439; kernels, semantics, sort key and tie rules: csrc/roi_post.hip) ----
 * 1 <= N <= 64 scenes of 1 <= R <= 16384 rows; 2 <= n_classes <= 1024; ncols 6 or 7; else -4.  Everything is DEVICE memory and fp32 unless stated.
 * pred_scores [N R][n_classes] logits, pred_bbox_deltas [N R][ncols] (may be NULL without is_reg), rois [N R][1+ncols] (level, box), counts [N] (clamped to
 * 0 .. R), mesh_sizes [N][3] int.  Per row: softmax, the decode of nmh_roi_decode (is_reg) or the RoI's own box, clip to the mesh (6 columns) or centre test
 * (7), size filter, score threshold (threshold_mode 0: any class probability >= score_thresh, the reference's reading; 1: the object probability) ->
 * cand_boxes [N R][ncols], cand_scores [N R] (the object probability), keys [N R] int (0: dropped or past counts, else the bits of the score plus 1). */
NMH_API int nmh_roi_post_select(int N, int R, int n_classes, int ncols, const float* pred_scores, const float* pred_bbox_deltas, const float* rois, const int* counts, const int* mesh_sizes, float score_thresh, float min_size, int is_reg, int threshold_mode, float* cand_boxes, float* cand_scores, int* keys, void* stream);
/* sorted_keys, order [N][R]: the stable descending sort of keys along R and its int64 indices.  mask: workspace of N R ceil(R / 64) words; keep: workspace
 * [N][R].  NMS per scene (suppressed iff IoU with a kept box > nms_thresh) -> boxes [N][R][ncols], scores [N][R], index [N][R] (source row, -1 past the
 * count), counts_out [N]; results in descending score, rows past the count zero. */
NMH_API int nmh_roi_post_nms(int N, int R, int ncols, const float* cand_boxes, const float* cand_scores, const int* sorted_keys, const int64_t* order, float nms_thresh, uint64_t* mask, int* keep, float* boxes, float* scores, int* index, int* counts_out, void* stream);
/* ---- detection evaluation (nerf_rpn/eval.py; kernels, tie rules and the two stated deviations: csrc/det_eval.hip) ----
 * Common arguments.  N scenes; boxes [N][cap] rows of row_stride floats in DESCENDING score with the box in columns col_offset .. col_offset + ncols - 1 (ncols 6:
 * x0,y0,z0,x1,y1,z1; 7: x,y,z,w,l,h,theta), read in place; counts [N]; gt [N][Gmax][ncols] padded, gt_counts [N].  cap <= 16384, Gmax <= 1024, at most 8 limits and
 * 8 thresholds, col_offset + ncols <= row_stride, else -4; a NULL required pointer is -4.  N == 0 returns 0 without a launch.  Nothing waits on the host.
 * nmh_det_eval_iou: box_iou_3d (model/utils.py:387-415) of every scene, as eval.py:36 and :357 call it -> iouT [N][Gmax][cap] (ground-truth-major; only entries
 * below counts and gt_counts are written), best_iou, best_gt [N][cap] = overlaps.max(dim=1) of eval.py:358, ties to the lower gt; (0, -1) without ground truth or
 * past counts. */
NMH_API int nmh_det_eval_iou(int ncols, int N, int cap, int row_stride, int col_offset, const float* boxes, const int* counts, int Gmax, const float* gt, const int* gt_counts, float* iouT, float* best_iou, int* best_gt, void* stream);
/* evaluate_box_proposals_recall's per-scene half (eval.py:22-59) for nlimits limits at once; limits HOST int [nlimits], negative: no cut -> gt_overlaps
 * [N][nlimits][Gmax] (the recorded IoUs in the order they were taken, 0 up to gt_counts, -1 behind it and in every slot of a skipped scene), counted [N][nlimits] =
 * the scene's contribution to num_pos (gt_counts, or 0 for a scene skipped by eval.py:28). */
NMH_API int nmh_det_eval_match(int N, int cap, int Gmax, const int* counts, const int* gt_counts, const float* iouT, int nlimits, const int* limits, float* gt_overlaps, int* counted, void* stream);
/* evaluate_box_proposals_ap's true-positive test (eval.py:331-366) per scene for nthresh IoU thresholds (HOST float [nthresh]) without the sequential walk;
 * top_k <= 0: no cut -> tp_mask [N][cap] bytes (bit q: true positive at thresholds[q]), kept [N][cap] bytes (row < min(counts, top_k)). */
NMH_API int nmh_det_eval_claims(int N, int cap, int Gmax, const int* counts, const float* best_iou, const int* best_gt, int nthresh, const float* thresholds, int top_k, unsigned char* tp_mask, unsigned char* kept, void* stream);
/* eval.py:368-387 for nthresh thresholds: bits [M] = the tp_mask bytes in the global descending-score order with the kept detections first; n_det [1] their
 * number, num_gt [1] (DEVICE ints) -> tp_cum, fp_cum [nthresh][M] int32, recalls, precisions [nthresh][M] fp32 (zeros from n_det on), ap [nthresh] fp64.
 * M == 0 returns 0 without a launch and leaves ap untouched. */
NMH_API int nmh_det_eval_pr(int64_t M, const unsigned char* bits, const int* n_det, const int* num_gt, int nthresh, int* tp_cum, int* fp_cum, float* recalls, float* precisions, double* ap, void* stream);
/* ---- RPNHead's output stage (nerf_rpn/model/anchor.py:177-224; kernels, fragment maps and semantics: csrc/rpn_head.hip) ----
 * level_vox: HOST int [nlevels] = W H D per level, 1 <= nlevels <= 4; N scenes; Cin a multiple of 8; 1 <= A <= 32 anchors per location; C 6 | 8, else -4.
 * t: HOST table of per-level DEVICE activations (N, W, H, D, Cin) channels-last in dt; w_cls [A][Cin], w_box [A C][Cin] in dt (the head's column j is row j
 * of w_cls below A and row j - A of w_box above); b_cls [A], b_box [A C] fp32.  relu != 0: t is rectified as it is read.
 * -> objectness (N, A, W, H, D) and pred_bbox_deltas (N, A C, W, H, D) fp32 per level, channel a C + c.  One launch for all levels. */
NMH_API int nmh_rpn_head_out_fwd(int dt, int nlevels, const int* level_vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box, const float* b_cls, const float* b_box, float* const* objectness, float* const* regression, void* stream);
/* Its backward.  g_obj, g_reg: per-level dense fp32 gradients of the two outputs.  -> dt_out per level = relu'(t) o (G Wcat) in dt, channels-last (relu'(0) = 0;
 * no mask with relu == 0); dw_cls, dw_box, db_cls, db_box += Gt relu(t) and the column sums of G over all levels, by per-workgroup partials (DEVICE workspace of
 * nmh_rpn_head_bwd_ws_floats() floats) summed in workgroup order: bit-identical between runs.  Three launches for all levels. */
NMH_API int64_t nmh_rpn_head_bwd_ws_floats(int nlevels, const int* level_vox, int N, int Cin, int A, int C);
NMH_API int nmh_rpn_head_out_bwd(int dt, int nlevels, const int* level_vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box, const float* const* g_obj, const float* const* g_reg, void* const* dt_out, float* partials, float* dw_cls, float* dw_box, float* db_cls, float* db_box, void* stream);
/* The ReLU between the head's convolutions, in place on a channels-last tensor of n elements (n % 8 == 0): x = max(x, 0); dy = 0 where y <= 0. */
NMH_API int nmh_relu_(int dt, void* x, int64_t n, void* stream);
NMH_API int nmh_relu_bwd_(int dt, void* dy, const void* y, int64_t n, void* stream);
/* ---- RCNN, the box head of the two-stage detector (nerf_rpn/model/detector.py:441-496; kernels, layouts and the order of every sum: csrc/box_head.hip) ----
 * x: the head's activation, channels-last per RoI in dt, [M][S][C]: M RoIs (1 .. 65535), S = ow oh od cells (1 .. 512), C channels (a multiple of 8, <= 2048).
 * reg_dim 6 | 7, n_classes >= 1, reg_dim + n_classes <= 32; anything else returns -4.  flatten != 0: the Linear layers read the flattened volume (K = S C);
 * 0: its mean over the cells (K = C).  relu != 0: x is rectified as it is read (the last conv's ReLU).
 * nmh_box_head_pack: w_box [reg_dim][C S], w_cls [n_classes][C S] fp32 in nn.Linear's NCDHW flatten order (column c S + s) -> wcat [reg_dim + n_classes][S C] in
 * dt with column s C + c, box rows first.  The mean form takes wcat in fp32 with S = 1 (dt = 0) whatever the activations' dtype.
 * nmh_box_head_out_fwd -> pred_bbox_delta [M][reg_dim], pred_scores [M][n_classes] fp32 with the biases added; xmean [M][C] fp32 (mean form only, else NULL)
 * receives the fp32 mean of relu?(x) over the cells and is an input of the backward.  A row's sums have one order for every M and every row position. */
NMH_API int nmh_box_head_pack(int dt, int reg_dim, int n_classes, int C, int S, const float* w_box, const float* w_cls, void* wcat, void* stream);
NMH_API int nmh_box_head_out_fwd(int dt, int M, int S, int C, int reg_dim, int n_classes, int flatten, int relu, const void* x, const void* wcat, const float* b_box, const float* b_cls, float* xmean, float* pred_bbox_delta, float* pred_scores, void* stream);
/* Its backward.  g_box [M][reg_dim], g_cls [M][n_classes]: fp32 gradients of the two outputs; either may be NULL (read as zeros; that output's dw / db are then
 * not touched and may be NULL).  -> dx [M][S][C] in dt = relu'(x) o (G wcat) (mean form: / S, through dxmean [M][C] fp32 scratch); dw_box, dw_cls (fp32, nn.Linear's
 * layout) and db_box, db_cls += the weight and bias gradients, by per-workgroup partials (nmh_box_head_bwd_ws_floats() floats) summed in workgroup order:
 * bit-identical between runs. */
NMH_API int64_t nmh_box_head_bwd_ws_floats(int M, int S, int C, int reg_dim, int n_classes, int flatten);
NMH_API int nmh_box_head_out_bwd(int dt, int M, int S, int C, int reg_dim, int n_classes, int flatten, int relu, const void* x, const void* wcat, const float* xmean, const float* g_box, const float* g_cls, void* dx, float* dxmean, float* partials, float* dw_box, float* dw_cls, float* db_box, float* db_cls, void* stream);
/* db [C] fp32 += the column sums of dy [rows][C] in dt (the bias gradient of a channels-last conv), per-workgroup partials (nmh_box_head_colsum_ws_floats()
 * floats) summed in workgroup order.  C a multiple of 8, <= 2048. */
NMH_API int64_t nmh_box_head_colsum_ws_floats(int64_t rows, int C);
NMH_API int nmh_box_head_colsum(int dt, const void* dy, int64_t rows, int C, float* partials, float* db, void* stream);
/* nmh_conv3d_k3_wgrad with a fixed order of additions: the contraction splits leave partial tiles in ws and a second launch adds them in split order.
 * nmh_conv3d_k3_wgrad_fixed_ws_floats(dt, rows = B D H W, Cin, Cout): the floats ws must hold (0: one split, ws may be NULL), or -2 when so many rows would
 * need atomics: pass fewer per call (16384 rows always fit).  The call returns -2 in that case and when ws is too small. */
NMH_API int64_t nmh_conv3d_k3_wgrad_fixed_ws_floats(int dt, int64_t rows, int Cin, int Cout);
NMH_API int nmh_conv3d_k3_wgrad_fixed(int dt, const void* dY, const void* X, float* dW, float* ws, int64_t ws_floats, int B, int D, int H, int W, int Cin, int Cout, void* stream);
/* ---- FCOSHead (nerf_rpn/model/fcos/fcos.py:26-139) between its 3x3x3 tower convolutions; kernels, fragment maps and semantics: csrc/fcos_head.hip ----
 * A job is one channels-last tensor (N, W, L, H, C) in dt of one (level, tower); njobs <= 10, C % 32 == 0, C <= 2048, C / G in {1, 2, 4} or a multiple of 8, else -4.
 * vox: HOST int [njobs] = W L H; tower: HOST int [njobs] in {0, 1}; x, y, dy, dx: HOST tables of njobs DEVICE pointers; gamma, beta, dgamma, dbeta: HOST tables of
 * two DEVICE pointers [C] fp32, one per tower (cls_tower, bbox_tower; an unused tower's entry may be NULL).  One launch covers every job.
 * nmh_fcos_gn_stats: nn.GroupNorm(G, C)'s statistics (fcos.py:63,75; eps inside the root, biased variance) -> stats [njobs][N][G][2] = {mean, rstd} fp32, from fp64
 * per-workgroup partial sums (ws: nmh_fcos_gn_ws_doubles() doubles) added in a fixed order.
 * nmh_fcos_gn_apply: y = relu(gamma_c (x - mean) rstd + beta_c) in dt (GroupNorm + nn.ReLU, fcos.py:63-64, 75-76).
 * nmh_fcos_gn_bwd: dx = rstd (dyh - mean_g(dyh) - xh mean_g(dyh xh)) in dt with dyh = dy [y > 0] gamma_c; dgamma[tower][c] += sum dy [y > 0] xh and
 * dbeta[tower][c] += sum dy [y > 0] over every job of the tower; sums: [njobs][N][G][2] fp32 scratch (the two group means); ws as above. */
NMH_API int64_t nmh_fcos_gn_ws_doubles(int njobs, const int* vox, int N, int C);
NMH_API int nmh_fcos_gn_stats(int dt, int njobs, const int* vox, int N, int C, int G, float eps, const void* const* x, double* ws, float* stats, void* stream);
NMH_API int nmh_fcos_gn_apply(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* x, const float* stats, const float* const* gamma, const float* const* beta, void* const* y, void* stream);
NMH_API int nmh_fcos_gn_bwd(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* dy, const void* const* x, const void* const* y, const float* stats, const float* const* gamma, double* ws, float* sums, float* const* dgamma, float* const* dbeta, void* const* dx, void* stream);
/* The output stage (fcos.py:80-87, 117-137): cls_logits, bbox_pred and centerness, nn.Conv3d(C, 1 | nreg | 1, 3, padding=1), nreg 6 | 8, of nlevels <= 5 levels in one
 * launch.  dims: HOST int [3 nlevels] = W, L, H; strides: HOST float [nlevels] (fpn_strides); act: HOST table of 2 nlevels DEVICE activations, entry 2 l + t the input
 * of tower t (0 cls, 1 bbox) at level l; w16: two packed weights [16][27][C] in dt, row j of tower 0 = cls_logits (j = 0), centerness (j = 1, unless ctr_on_reg), of
 * tower 1 = bbox_pred (j < nreg), centerness (j = nreg, if ctr_on_reg), the other rows zero; scale: nlevels DEVICE pointers to the Scale parameters (fcos.py:17-23).
 * mode 0: norm_reg_targets in training (ReLU on columns 0-5, fcos.py:126-130); 1: in evaluation (those columns times the stride, :132); 2: exp of every column (:136).
 * -> cls (N, 1, W, L, H), reg (N, nreg, W, L, H), ctr (N, 1, W, L, H) fp32 and u (N, nreg, W, L, H): bbox_pred with its bias before the Scale, kept for the backward. */
NMH_API int nmh_fcos_head_out_fwd(int dt, int nlevels, const int* dims, const float* strides, int N, int C, int nreg, int ctr_on_reg, int mode, const void* const* act, const void* const* w16, const float* b_cls, const float* b_box, const float* b_ctr, const float* const* scale, float* const* cls, float* const* reg, float* const* ctr, float* const* u, void* stream);
/* Its backward, first half: the dense fp32 gradients through the epilogue (ReLU mask where the output is > 0, times the Scale, times the output in the exp branch)
 * -> g16: per (level, tower) the 16-column gradient (N, W, L, H, 16) in dt, the dgrad operand of nmh_conv3d_k3; gt: the same as fp32 planes (N, 16, W, L, H), the
 * operand of nmh_fcos_head_out_wgrad; db_cls, db_box, db_ctr += the bias gradients and *dscale[l] += sum g mask (conv + bias), from per-workgroup partials
 * (nmh_fcos_head_pack_ws_floats() floats) summed in a fixed order. */
NMH_API int64_t nmh_fcos_head_pack_ws_floats(int nlevels, const int* dims, int N);
NMH_API int nmh_fcos_head_out_bwd_pack(int dt, int nlevels, const int* dims, const float* strides, int N, int nreg, int ctr_on_reg, int mode, const float* const* g_cls, const float* const* g_reg, const float* const* g_ctr, const float* const* u, const float* const* scale, void* const* g16, float* const* gt, float* partials, float* db_cls, float* db_box, float* db_ctr, float* const* dscale, void* stream);
/* Second half: dw_cls [1][C][3][3][3], dw_box [nreg][C][3][3][3], dw_ctr [1][C][3][3][3] (fp32, nn.Conv3d layout) += the weight gradients over every level, from
 * per-workgroup partials (nmh_fcos_head_wgrad_ws_floats() floats) summed in workgroup order; in bf16 the gradient enters the matrix cores as hi + lo. */
NMH_API int64_t nmh_fcos_head_wgrad_ws_floats(int nlevels, const int* dims, int N, int C);
NMH_API int nmh_fcos_head_out_wgrad(int dt, int nlevels, const int* dims, int N, int C, int nreg, int ctr_on_reg, const void* const* act, const float* const* gt, float* partials, float* dw_cls, float* dw_box, float* dw_ctr, void* stream);
/* Per-step host parameters of the training step in ONE launch, passed as kernel arguments (no host-to-device copies):
 *  - block_bits (HOST, nb^3 bits, bit (a*nb+b)*nb+c = 1: the 4x4x4-token block (a,b,c) is removed; window_masking_3d's raster order,
 *    swin_mae3d.py:1366-1373) is expanded to the token mask tokmask[g^3] (device, uint8; tokens outside the nb^3 blocks stay 0);
 *  - hyper (HOST, 8 floats {lr, beta1, beta2, eps, wd, 1-beta1^t, 1-beta2^t, zero_g}) -> hyper_dev (nmh_adamw_step);
 *  - extents (HOST, n_ext <= 48 ints: [B][3] valid voxels per axis) -> extents_dev (nmh_mae_loss_fwd / nmh_mae_tail_fwd).
 * Any of the three groups may be NULL.  nb^3 <= 4096. */
NMH_API int nmh_step_params(const uint32_t* block_bits, int nb, int g, unsigned char* tokmask, const float* hyper, float* hyper_dev, const int* extents, int n_ext, int* extents_dev, void* stream);
/* bf16 gradient buckets of the data-parallel exchange (DDP's gradient all-reduce, run_swin_mae3d.py:355-357, with half the bytes on the
 * xGMI links): a contiguous range of the flat fp32 gradient buffer -> bf16 bucket (round to nearest even) before the collective, and
 * bucket * scale -> fp32 gradients after it (scale = 1/world for backends that sum).  n % 8 == 0, 16-byte aligned pointers. */
NMH_API int nmh_grad_to_bf16(const float* g, void* bucket, int64_t n, void* stream);
NMH_API int nmh_grad_from_bf16(const void* bucket, float* g, int64_t n, float scale, void* stream);

/* fp32 master weights -> compute-dtype GEMM operand layouts, one launch for the whole model.  descs: device array of
 * {const float* src; void* dst; int mode; int d0,d1,d2; int64 n} (40 bytes, see kernels.hpp PackDesc); one block per 1024 dst elements
 * (blkstart = first element), except the tiled modes, where blkstart = block id: mode 1 (2-D transpose) one block per 32x32 tile of the
 * d0 x d1 source, row-major over ceil(d0/32) x ceil(d1/32); mode 2 (conv fwd) d0 x ceil(d1/32) blocks (co, 32 ci); mode 3 (conv dgrad)
 * d1 x ceil(d0/32) blocks (ci, 32 co). */
NMH_API int nmh_pack_weights(int dt, const void* descs_dev, const int* blk2desc_dev, const int64_t* blkstart_dev, int nblocks, void* stream);
/* clip_grad_norm_ + AdamW (run_swin_mae3d.py:588-592,665-668) over the flat fp32 parameter buffer; hyper (device fp32[8]) =
 * {lr, beta1, beta2, eps, weight_decay, 1-beta1^t, 1-beta2^t, zero_g}; coef (device) = min(1, max_norm/(norm+1e-6)); zero_g != 0:
 * the step also clears g (the next step's zero_grad for free). */
NMH_API int nmh_grad_sqnorm(const float* g, int64_t n, double* acc, void* stream);
NMH_API int nmh_clip_coef(const double* acc, float max_norm, float* coef, float* norm_out, void* stream);
NMH_API int nmh_adamw_step(float* p, float* g, float* m, float* v, int64_t n, const float* hyper, const float* coef, void* stream);
/* Gradient accumulation: k micro-batches per optimizer step, each weighted 1/k as DDP weights its ranks (run_swin_mae3d.py:355-357, 665-669).
 * g holds the SUM G of the k micro-gradients (every weight-gradient kernel adds into it; zero_g of the previous step cleared it) and acc = |G|^2 from
 * nmh_grad_sqnorm or nmh_grad_sqnorm_ranges.  nmh_clip_coef_mean in the place of nmh_clip_coef: with inv_k = *inv_k_dev (device fp32, 1/k),
 *   nrm = sqrt(acc) * inv_k;  coef = inv_k * min(1, max_norm / (nrm + 1e-6))  (coef = inv_k with max_norm <= 0);  norm_out = nrm,
 * the norm of the mean gradient, what clip_grad_norm_ reports after DDP; the AdamW entries, which multiply g by coef, then step on the clipped mean.
 * Evaluated in fp64 and rounded once; with *inv_k_dev == 1 coef and norm_out are the bits of nmh_clip_coef.
 * nmh_grad_scale stores inv_k (in (0, 1], else -4) into inv_k_dev as the kernel argument of a one-thread launch, as nmh_step_params stores hyper: no copy,
 * no host wait, and the value may change between replays of a captured optimizer graph (the ragged last step of an epoch). */
NMH_API int nmh_clip_coef_mean(const double* acc, float max_norm, const float* inv_k_dev, float* coef, float* norm_out, void* stream);
NMH_API int nmh_grad_scale(float inv_k, float* inv_k_dev, void* stream);
/* The same two passes with per-range settings over the flat buffer (one optimizer param group per range: layer-wise learning-rate decay,
 * no-decay sets, frozen ranges).  The table is on the device: bounds int64 [R+1] with 0 = bounds[0] < bounds[1] < ... < bounds[R] = n and
 * every interior boundary a multiple of 4 (a 16-byte group lies in one range); scale float [R][2] = (lr_scale, wd_scale), finite and >= 0.
 * Range r steps with lr * lr_scale and weight_decay * wd_scale; one range (1, 1) gives the bits of nmh_adamw_step.  lr_scale == 0 is FROZEN
 * (requires_grad = False, not torch's lr = 0): p, m and v of the range are not written and nmh_grad_sqnorm_ranges leaves its gradient out
 * of the norm, which is what clip_grad_norm_ sees when frozen parameters have no gradient; the gradient is still cleared under zero_g.
 * nmh_clip_coef sits between the two as before.
 * Both entries check the table on the host and return -5, launching nothing, for R outside 1 .. NMH_ADAMW_MAX_RANGES, bounds that are not
 * as above, a misaligned table or a negative / non-finite scale.  The check copies the table (12 R bytes) on a stream of the library's own
 * and waits for that copy alone, never for `stream`; the table must therefore be complete in memory when the entry is called.  While
 * `stream` is being captured the host may not copy, so only R and n are checked: pass a table once outside the capture first.  The kernels
 * stay inside [0, R) and [0, n) for any table contents. */
#define NMH_ADAMW_MAX_RANGES 4096
NMH_API int nmh_grad_sqnorm_ranges(const float* g, int64_t n, const int64_t* bounds, const float* scale, int R, double* acc, void* stream);
NMH_API int nmh_adamw_step_ranges(float* p, float* g, float* m, float* v, int64_t n, const float* hyper, const float* coef, const int64_t* bounds, const float* scale, int R, void* stream);

#ifdef __cplusplus
}
#endif
#endif
