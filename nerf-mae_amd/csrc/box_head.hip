// Output stage of the reference's box head RCNN (nerf_rpn/model/detector.py:441-496), the second stage's head of the two-stage detector, as gfx950 kernels.
// The head's activations are channels-last per RoI in the compute dtype T, x [M][S][C] (M RoIs, S = ow oh od cells, C channels): the layout the shared
// 3x3x3 conv layer takes with the RoI as its batch index.  The head's two Linear layers, RCNN_bbox_pred (reg = 6 | 7 rows) and RCNN_cls_score (ncls rows),
// are one matrix Wcat [J][K], J = reg + ncls <= 32, box rows first:
//   flatten form   K = S C: a row of x is the contraction vector as it lies in memory; nn.Linear's weight is in NCDHW flatten order (column c S + s), so
//                  box_pack writes Wcat[j][s C + c] = W[j][c S + s] in the compute dtype (one launch per call, from the fp32 masters);
//   mean form      K = C: box_mean_fwd first reduces relu?(x) over the S cells in fp32, ascending s, then divides by S -> xm [M][C] fp32; the product runs
//                  on xm in the exact fp32 path for either compute dtype, Wcat [J][C] being the fp32 masters side by side (box_pack with T = float, S = 1).
// Kernels:
//   box_out_fwd   D[j][row] = sum_k Wcat[j][k] relu?(x[row][k]) + bias -> pred_bbox_delta [M][reg] and pred_scores [M][ncls], fp32, one launch.  A workgroup
//                 owns 32 rows; its 4 waves take the contraction steps w, w + 4, w + 8, ... and their accumulators are added through LDS as
//                 (w0 + w1) + (w2 + w3).  The order of a row's sum therefore depends on K alone: not on M, not on the row's position, not on the other rows;
//   box_out_dx    dx[row][k] = relu'(x[row][k]) sum_j G[row][j] Wcat[j][k], stored in T; a wave owns 32 rows x 64 contraction columns;
//   box_out_dw    per-workgroup partial sums of Gt relu?(x) and of the column sums of G (a tile of ones in place of x) over the workgroup's share of the rows,
//   box_out_red   the partials summed in workgroup order and added to the two weight gradients (in nn.Linear's column order) and the two bias gradients: a
//                 fixed order, two runs are bit-identical.  A null gradient pointer (an output without cotangent) reads as zeros and its parameters' gradient
//                 buffers are not touched;
//   box_mean_bwd  dx[row][s][c] = relu'(x) dxm[row][c] / S, the adjoint of box_mean_fwd;
//   box_colsum    db[c] += sum over the rows of dy [R][C], per-workgroup partials summed in workgroup order: the bias gradient of the head's 3x3x3 convs.
// G = (g_box | g_cls) is fp32 and enters the bf16 matrix cores as hi + lo (mfma32.hpp); everything accumulates in fp32.  relu'(0) = 0.  No scratch; the
// forward uses 16 KiB of LDS for the wave sum, the column sums 8 KiB.
// Fragment use (maps: mfma32.hpp):
//   fwd: D[column j][row]     the row is on the lane;
//   dx:  D[k][row]            registers 4 q .. 4 q + 3 are columns 8 q + 4 h .. + 3 of the lane's row: one 8-byte (bf16) or 16-byte store;
//   dw:  D[column j][k]       the contraction column is on the lane, a register's store is 32 consecutive floats of a partial's row.
#include "mfma32.hpp"
#include "kernels.hpp"

namespace {

constexpr int BOX_MAX_J = 32;                          // reg + ncls: one 32-row accumulator tile
constexpr int BOX_MAX_CELLS = 512;                     // S; 7^3 = 343 fits
constexpr int BOX_MAX_C = 2048;                        // box_colsum: C / 8 <= 256 lanes
constexpr int BOX_MAX_ROWS = 65535;                    // the layout passes in front of the head put the RoI on grid.z
constexpr int BOX_DW_MAX_BLOCKS = 64;
constexpr long BOX_DW_WS_FLOATS = 16L << 20;           // partial sums of the weight-gradient pass: at most 64 MiB
constexpr int BOX_COLSUM_MAX_BLOCKS = 128;

bool bad_geom(int M, int S, int C, int reg, int ncls) {
  return M < 1 || M > BOX_MAX_ROWS || S < 1 || S > BOX_MAX_CELLS || C < 8 || C % 8 || C > BOX_MAX_C || (reg != 6 && reg != 7) || ncls < 1 || reg + ncls > BOX_MAX_J;
}

// ---- Wcat from the fp32 masters -------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void box_pack_kernel(int reg, int J, int C, int S, const float* __restrict__ wb, const float* __restrict__ wc, T* __restrict__ out) {
  const long K = (long)S * C, n = (long)J * K;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int j = (int)(i / K);
    const int k = (int)(i - (long)j * K), s = k / C, c = k - s * C;
    const float* __restrict__ src = j < reg ? wb + (long)j * K : wc + (long)(j - reg) * K;
    out[i] = from_f<T>(src[(long)c * S + s]);
  }
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void box_out_fwd_kernel(int M, int K, int reg, int J, int relu, const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ bb,
                                                          const float* __restrict__ bc, float* __restrict__ ob, float* __restrict__ oc) {
  typedef MM<T> Mm;
  constexpr int E = Mm::E;
  __shared__ float red[4][16][64];
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int m = blockIdx.x * 32 + r;
  const bool min_ = m < M, jin = r < J;
  const T* __restrict__ xrow = x + (long)(min_ ? m : 0) * K;
  const T* __restrict__ wrow = w + (long)(jin ? r : 0) * K;
  f32x16 acc = acc_zero();
  for (int k0 = wave * 2 * E; k0 < K; k0 += 8 * E) {     // wave w: steps w, w + 4, ...: fixed by K alone
    const int kk = k0 + E * h;
    const bool kin = kk < K;                             // K is a multiple of 8: a lane's chunk is inside or outside as a whole
    typename Mm::Exact b = (min_ && kin) ? Mm::load16(xrow + kk) : Mm::zero();
    if (relu) Mm::relu(b);
    const typename Mm::Exact a = (jin && kin) ? Mm::load16(wrow + kk) : Mm::zero();
    Mm::mma(acc, a, b);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) red[wave][i][lane] = acc[i];
  __syncthreads();
  if (wave != 0 || !min_) return;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = acc_row(i, h);
    if (j < J) {
      const float s = (red[0][i][lane] + red[1][i][lane]) + (red[2][i][lane] + red[3][i][lane]);
      if (j < reg) ob[(long)m * reg + j] = s + bb[j];
      else oc[(long)m * (J - reg) + (j - reg)] = s + bc[j - reg];
    }
  }
}

// ---- backward: dx -----------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void box_out_dx_kernel(int M, int K, int reg, int J, int relu, const T* __restrict__ x, const T* __restrict__ w, const float* __restrict__ gb,
                                                         const float* __restrict__ gc, T* __restrict__ dx) {
  typedef MM<T> Mm;
  constexpr int E = Mm::E;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int kch = (K + 63) / 64, total = ((M + 31) / 32) * kch;
  const int wt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wt >= total) return;
  const int mt = wt / kch, c0 = (wt - mt * kch) * 64;
  const int m = mt * 32 + r;
  const bool min_ = m < M, two = c0 + 32 < K;
  const int ca = c0 + r, cb = c0 + 32 + r;
  const float* __restrict__ gbr = gb ? gb + (long)(min_ ? m : 0) * reg : nullptr;
  const float* __restrict__ gcr = gc ? gc + (long)(min_ ? m : 0) * (J - reg) : nullptr;
  f32x16 acc0 = acc_zero(), acc1 = acc_zero();
  for (int j0 = 0; j0 < J; j0 += 2 * E) {
    typename Mm::Wide b = Mm::wzero();
    typename Mm::Exact a0 = Mm::zero(), a1 = Mm::zero();
    ForE<0, E>::run([&](auto I) {
      const int j = j0 + E * h + decltype(I)::value;
      if (j < J) {
        const T* __restrict__ wr = w + (long)j * K;
        if (min_) Mm::template setw<decltype(I)::value>(b, j < reg ? (gbr ? gbr[j] : 0.f) : (gcr ? gcr[j - reg] : 0.f));
        if (ca < K) Mm::template set<decltype(I)::value>(a0, wr[ca], false);
        if (two && cb < K) Mm::template set<decltype(I)::value>(a1, wr[cb], false);
      }
    });
    Mm::mma_wb(acc0, a0, b);
    if (two) Mm::mma_wb(acc1, a1, b);
  }
  if (!min_) return;
  const long row = (long)m * K;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int c = c0 + 8 * s + 4 * h;                    // registers 4 s .. 4 s + 3: four consecutive columns
    if (c < K) Out4<T>::mask_store(dx + row + c, x + row + c, relu != 0, acc0[4 * s], acc0[4 * s + 1], acc0[4 * s + 2], acc0[4 * s + 3]);
  }
  if (two) {
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int c = c0 + 32 + 8 * s + 4 * h;
      if (c < K) Out4<T>::mask_store(dx + row + c, x + row + c, relu != 0, acc1[4 * s], acc1[4 * s + 1], acc1[4 * s + 2], acc1[4 * s + 3]);
    }
  }
}

// ---- backward: weight and bias gradients ----------------------------------------------------------------------------------------------------------
// Workgroup (b, y) sums the 32-row tiles [b tiles / nb, (b + 1) tiles / nb) into partial b, a [J][K + 1] image whose last column holds the column sums of G.
// Wave w of workgroup y owns the output tile 4 y + w: 32 columns j x 32 contraction columns (tile K / 32, rounded up, is the column of ones).
template <typename T>
__global__ __launch_bounds__(256) void box_out_dw_kernel(int M, int K, int reg, int J, int relu, const T* __restrict__ x, const float* __restrict__ gb, const float* __restrict__ gc,
                                                         float* __restrict__ partials) {
  typedef MM<T> Mm;
  constexpr int E = Mm::E;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int nct = (K + 31) / 32;
  const int og = __builtin_amdgcn_readfirstlane(blockIdx.y * 4 + (threadIdx.x >> 6));
  if (og > nct) return;
  const int nb = gridDim.x, b = blockIdx.x, tiles = (M + 31) / 32;
  const int tb = (int)((long)b * tiles / nb), te = (int)((long)(b + 1) * tiles / nb);
  const bool ones = og == nct, jin = r < J;
  const int c = og * 32 + r, ncls = J - reg;
  const float* __restrict__ gcol = !jin ? nullptr : (r < reg ? (gb ? gb + r : nullptr) : (gc ? gc + (r - reg) : nullptr));
  const int gstride = r < reg ? reg : ncls;
  f32x16 acc = acc_zero();
  for (int mt = tb; mt < te; ++mt) {
#pragma unroll
    for (int s = 0; s < 32; s += 2 * E) {
      typename Mm::Wide a = Mm::wzero();
      typename Mm::Exact bf = Mm::zero();
      ForE<0, E>::run([&](auto I) {
        const int m = mt * 32 + s + E * h + decltype(I)::value;
        if (m < M) {
          if (gcol) Mm::template setw<decltype(I)::value>(a, gcol[(long)m * gstride]);
          if (ones) Mm::template set<decltype(I)::value>(bf, from_f<T>(1.f), false);
          else if (c < K) Mm::template set<decltype(I)::value>(bf, x[(long)m * K + c], relu != 0);
        }
      });
      Mm::mma_wa(acc, a, bf);
    }
  }
  const int col = ones ? (r == 0 ? K : -1) : (c < K ? c : -1);
  if (col < 0) return;
  float* __restrict__ P = partials + (long)b * J * (K + 1);
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int j = acc_row(i, h);
    if (j < J) P[(long)j * (K + 1) + col] = acc[i];
  }
}

// K = S C: contraction column k = s C + c of Wcat is column c S + s of the Linear weight
__global__ __launch_bounds__(256) void box_out_red_kernel(int nb, int K, int C, int S, int reg, int J, const float* __restrict__ partials, float* __restrict__ dwb,
                                                          float* __restrict__ dwc, float* __restrict__ dbb, float* __restrict__ dbc) {
  const long Ks = K + 1, n = (long)J * Ks;
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += partials[(long)b * n + e];          // workgroup order: fixed
  const int j = (int)(e / Ks), k = (int)(e - (long)j * Ks);
  const bool box = j < reg;
  const int jj = box ? j : j - reg;
  if (k < K) {
    float* d = box ? dwb : dwc;
    const int sc = k / C, c = k - sc * C;
    if (d) d[(long)jj * K + (long)c * S + sc] += s;
  } else {
    float* d = box ? dbb : dbc;
    if (d) d[jj] += s;
  }
}

// ---- the mean over the cells and its adjoint ----------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void box_mean_fwd_kernel(long n8, int S, int C, int relu, const T* __restrict__ x, float* __restrict__ xm) {
  const int C8 = C / 8;
  const float S_f = (float)S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long m = i / C8;
    const int c = (int)(i - m * C8) * 8;
    float sum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      float v[8];
      Vec8<T>::load(x + (m * S + s) * C + c, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) sum[e] += (relu && v[e] <= 0.f) ? 0.f : v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sum[e] /= S_f;
    Vec8<float>::store(xm + m * C + c, sum);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void box_mean_bwd_kernel(long n8, int S, int C, int relu, const T* __restrict__ x, const float* __restrict__ dxm, T* __restrict__ dx) {
  const int C8 = C / 8;
  const float S_f = (float)S;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long row = i / C8;                             // m S + s
    const int c = (int)(i - row * C8) * 8;
    float d[8], v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    Vec8<float>::load(dxm + (row / S) * C + c, d);
    if (relu) Vec8<T>::load(x + row * C + c, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = (relu && !(v[e] > 0.f)) ? 0.f : d[e] / S_f;
    Vec8<T>::store(dx + row * C + c, d);
  }
}

// ---- column sums in a fixed order -----------------------------------------------------------------------------------------------------------------
// Workgroup b owns the rows [b R / nb, (b + 1) R / nb): lane (rl, c8) adds rows rl, rl + NV, ... of its 8 columns, the NV row lanes are added in ascending order.
template <typename T>
__global__ __launch_bounds__(256) void box_colsum_kernel(const T* __restrict__ dy, long R, int C, float* __restrict__ partials) {
  __shared__ float sm[2048];                             // NV x C <= 256 x 8
  const int nch = C / 8, NV = 256 / nch;
  const int c8 = threadIdx.x % nch, rl = threadIdx.x / nch;
  const long r0 = (long)blockIdx.x * R / gridDim.x, r1 = (long)(blockIdx.x + 1) * R / gridDim.x;
  if (rl < NV) {
    float p[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (long m = r0 + rl; m < r1; m += NV) {
      float v[8];
      Vec8<T>::load(dy + m * C + c8 * 8, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) sm[rl * C + c8 * 8 + e] = p[e];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    float s = 0.f;
    for (int q = 0; q < NV; ++q) s += sm[q * C + c];
    partials[(long)blockIdx.x * C + c] = s;
  }
}
__global__ __launch_bounds__(256) void box_colsum_red_kernel(int nb, int C, const float* __restrict__ partials, float* __restrict__ db) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += partials[(long)b * C + c];          // workgroup order: fixed
  db[c] += s;
}

int dw_blocks(int M, int K, int J) {
  long nb = (M + 31) / 32;
  if (nb > BOX_DW_MAX_BLOCKS) nb = BOX_DW_MAX_BLOCKS;
  const long per = (long)J * (K + 1);
  if (nb * per > BOX_DW_WS_FLOATS) nb = BOX_DW_WS_FLOATS / per;
  return nb < 1 ? 1 : (int)nb;
}
int colsum_blocks(long R) {
  const long nb = (R + 255) / 256;
  return nb > BOX_COLSUM_MAX_BLOCKS ? BOX_COLSUM_MAX_BLOCKS : (int)nb;
}
unsigned ew_grid(long n) {
  const long nb = (n + 255) / 256;
  return (unsigned)(nb > 4096 ? 4096 : (nb < 1 ? 1 : nb));
}

template <typename T>
int launch_fwd(int M, int K, int reg, int J, int relu, const void* x, const void* w, const float* bb, const float* bc, float* ob, float* oc, hipStream_t st) {
  hipLaunchKernelGGL(box_out_fwd_kernel<T>, dim3((unsigned)((M + 31) / 32)), dim3(256), 0, st, M, K, reg, J, relu, (const T*)x, (const T*)w, bb, bc, ob, oc);
  NMH_CHECK_LAUNCH();
  return 0;
}
template <typename T>
int launch_dx(int M, int K, int reg, int J, int relu, const void* x, const void* w, const float* gb, const float* gc, void* dx, hipStream_t st) {
  const long waves = (long)((M + 31) / 32) * ((K + 63) / 64);
  hipLaunchKernelGGL(box_out_dx_kernel<T>, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, M, K, reg, J, relu, (const T*)x, (const T*)w, gb, gc, (T*)dx);
  NMH_CHECK_LAUNCH();
  return 0;
}
template <typename T>
int launch_dw(int M, int K, int C, int S, int reg, int J, int relu, const void* x, const float* gb, const float* gc, float* partials, float* dwb, float* dwc, float* dbb,
              float* dbc, hipStream_t st) {
  const int nb = dw_blocks(M, K, J), tiles = (K + 31) / 32 + 1;
  hipLaunchKernelGGL(box_out_dw_kernel<T>, dim3((unsigned)nb, (unsigned)((tiles + 3) / 4)), dim3(256), 0, st, M, K, reg, J, relu, (const T*)x, gb, gc, partials);
  NMH_CHECK_LAUNCH();
  const long n = (long)J * (K + 1);
  hipLaunchKernelGGL(box_out_red_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, nb, K, C, S, reg, J, partials, dwb, dwc, dbb, dbc);
  NMH_CHECK_LAUNCH();
  return 0;
}

}  // namespace

int k_box_head_pack(int dt, int reg, int ncls, int C, int S, const float* w_box, const float* w_cls, void* wcat, hipStream_t st) {
  if (bad_geom(1, S, C, reg, ncls) || !w_box || !w_cls || !wcat) return -4;
  const int J = reg + ncls;
  const unsigned nb = ew_grid((long)J * S * C);
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(box_pack_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, reg, J, C, S, w_box, w_cls, (bf16_t*)wcat);
  else if (dt == NMH_DT_F32) hipLaunchKernelGGL(box_pack_kernel<float>, dim3(nb), dim3(256), 0, st, reg, J, C, S, w_box, w_cls, (float*)wcat);
  else return -1;
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_box_head_out_fwd(int dt, int M, int S, int C, int reg, int ncls, int flatten, int relu, const void* x, const void* wcat, const float* b_box, const float* b_cls, float* xmean,
                       float* out_box, float* out_cls, hipStream_t st) {
  if (bad_geom(M, S, C, reg, ncls) || !x || !wcat || !b_box || !b_cls || !out_box || !out_cls || (!flatten && !xmean)) return -4;
  if (dt != NMH_DT_BF16 && dt != NMH_DT_F32) return -1;
  const int J = reg + ncls;
  relu = relu ? 1 : 0;
  if (flatten)
    return dt == NMH_DT_BF16 ? launch_fwd<bf16_t>(M, S * C, reg, J, relu, x, wcat, b_box, b_cls, out_box, out_cls, st)
                             : launch_fwd<float>(M, S * C, reg, J, relu, x, wcat, b_box, b_cls, out_box, out_cls, st);
  const long n8 = (long)M * (C / 8);
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(box_mean_fwd_kernel<bf16_t>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, S, C, relu, (const bf16_t*)x, xmean);
  else hipLaunchKernelGGL(box_mean_fwd_kernel<float>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, S, C, relu, (const float*)x, xmean);
  NMH_CHECK_LAUNCH();
  return launch_fwd<float>(M, C, reg, J, 0, xmean, wcat, b_box, b_cls, out_box, out_cls, st);
}

long k_box_head_bwd_ws_floats(int M, int S, int C, int reg, int ncls, int flatten) {
  if (bad_geom(M, S, C, reg, ncls)) return -1;
  const int K = flatten ? S * C : C, J = reg + ncls;
  return (long)dw_blocks(M, K, J) * J * (K + 1);
}

int k_box_head_out_bwd(int dt, int M, int S, int C, int reg, int ncls, int flatten, int relu, const void* x, const void* wcat, const float* xmean, const float* g_box,
                       const float* g_cls, void* dx, float* dxmean, float* partials, float* dw_box, float* dw_cls, float* db_box, float* db_cls, hipStream_t st) {
  if (bad_geom(M, S, C, reg, ncls) || !x || !wcat || !dx || !partials || (!flatten && (!xmean || !dxmean))) return -4;
  if (dt != NMH_DT_BF16 && dt != NMH_DT_F32) return -1;
  const int J = reg + ncls;
  relu = relu ? 1 : 0;
  if (flatten) {
    const int K = S * C;
    if (dt == NMH_DT_BF16) {
      if (int rc = launch_dx<bf16_t>(M, K, reg, J, relu, x, wcat, g_box, g_cls, dx, st)) return rc;
      return launch_dw<bf16_t>(M, K, C, S, reg, J, relu, x, g_box, g_cls, partials, dw_box, dw_cls, db_box, db_cls, st);
    }
    if (int rc = launch_dx<float>(M, K, reg, J, relu, x, wcat, g_box, g_cls, dx, st)) return rc;
    return launch_dw<float>(M, K, C, S, reg, J, relu, x, g_box, g_cls, partials, dw_box, dw_cls, db_box, db_cls, st);
  }
  if (int rc = launch_dx<float>(M, C, reg, J, 0, xmean, wcat, g_box, g_cls, dxmean, st)) return rc;
  const long n8 = (long)M * S * (C / 8);
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(box_mean_bwd_kernel<bf16_t>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, S, C, relu, (const bf16_t*)x, dxmean, (bf16_t*)dx);
  else hipLaunchKernelGGL(box_mean_bwd_kernel<float>, dim3(ew_grid(n8)), dim3(256), 0, st, n8, S, C, relu, (const float*)x, dxmean, (float*)dx);
  NMH_CHECK_LAUNCH();
  return launch_dw<float>(M, C, C, 1, reg, J, 0, xmean, g_box, g_cls, partials, dw_box, dw_cls, db_box, db_cls, st);
}

long k_box_head_colsum_ws_floats(long R, int C) {
  if (R < 1 || C < 8 || C % 8 || C > BOX_MAX_C) return -1;
  return (long)colsum_blocks(R) * C;
}

int k_box_head_colsum(int dt, const void* dy, long R, int C, float* partials, float* db, hipStream_t st) {
  if (R < 1 || C < 8 || C % 8 || C > BOX_MAX_C || !dy || !partials || !db) return -4;
  const int nb = colsum_blocks(R);
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(box_colsum_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (const bf16_t*)dy, R, C, partials);
  else if (dt == NMH_DT_F32) hipLaunchKernelGGL(box_colsum_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (const float*)dy, R, C, partials);
  else return -1;
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(box_colsum_red_kernel, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, st, nb, C, partials, db);
  NMH_CHECK_LAUNCH();
  return 0;
}
