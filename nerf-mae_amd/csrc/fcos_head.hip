// The reference's FCOSHead (nerf_rpn/model/fcos/fcos.py:26-139) between its 3x3x3 tower convolutions, as gfx950 kernels:
//   gn_reduce<fwd>   per-channel (sum x, sum x^2) in fp64 of one voxel share of one (job, scene): per-workgroup partials, no atomics;
//   gn_finalize      the partials summed in a fixed order -> {mean, rstd} per (job, scene, group) (nn.GroupNorm: biased variance, eps inside the root);
//   gn_apply         y = relu(gamma_c (x - mean) rstd + beta_c), stored in the compute dtype;
//   gn_reduce<bwd>   per-channel (sum dy [y > 0] xhat, sum dy [y > 0]) in fp64, the same partial scheme;
//   gn_bwd_finalize  per group mean(dyhat), mean(dyhat xhat) with dyhat = dy [y > 0] gamma_c; per (tower, channel) dgamma += , dbeta += over every level;
//   gn_bwd_apply     dx = rstd (dyhat - mean_g(dyhat) - xhat mean_g(dyhat xhat)), stored in the compute dtype;
//   out_fwd          cls_logits, bbox_pred and centerness (3x3x3, padding 1) of every level in ONE launch as an implicit GEMM on v_mfma_f32_16x16x32_bf16
//                    (v_mfma_f32_16x16x4_f32 for the exact fp32 path), N = 16 columns per tower, K = 27 C, written as the fp32 NCDHW planes with the epilogue
//                    of fcos.py:123-137 (bias, Scale, column-wise ReLU, stride or exp); the bbox columns before the Scale are kept for the backward;
//   out_bwd_pack     the dense fp32 gradients of the three outputs through that epilogue -> per tower a 16-column gradient, channels-last in the compute dtype
//                    (the dgrad operand of nmh_conv3d_k3) and as fp32 planes (the wgrad operand), plus per-workgroup partials of the bias and Scale gradients;
//   out_bwd_red      those partials summed in workgroup order -> db += , dscale_l += ;
//   out_wgrad        per-workgroup partials of dW16[j][tap][c] = sum_v G[j][v] a[v + tap][c] (MFMA, contraction over voxels), then
//   out_wgrad_red    summed in workgroup order and added to the three weight gradients in nn.Conv3d layout.
// A "job" is one (level, tower) tensor: job 2 l + t in the output stage, any order in the GroupNorm calls (tower[j] picks the affine parameters); one launch
// covers every job.  All activations are channels-last (N, W, L, H, C), C % 32 == 0.  No kernel waits for the host, none uses a floating-point atomic: every
// sum has a fixed order, two runs are bit-identical.
//
// Fragment maps (common.hpp: Frag / mma; lane l, i = l & 15, g = l >> 4): element e of A is A[row i][k = 8 g + e], of B is B[k = 8 g + e][col i]; C/D: col = i,
// row = 4 g + r for register r.  One step contracts 32 elements for both dtypes (fp32: eight 16x16x4 instructions, exact).
//   out_fwd:   D[column j][voxel] = sum_{tap, c} W16[j][tap][c] a[voxel + tap][c].  A = 16 B of the packed weight row j, B = 16 B of the neighbour voxel's channels
//              (zero outside the grid).  A wave owns 64 consecutive voxels of one (job, scene) as four tiles that share every A fragment; register r of a lane
//              is column 4 g + r of its voxel, so a store is 16 consecutive floats of one plane.
//   out_wgrad: D[column j][channel] = sum_v G[j][v] a[v + tap][channel]: a step is 32 consecutive voxels of one scene; A = 8 consecutive floats of G's plane j
//              (bf16: split into hi + lo = bf16(G) + bf16(G - hi), two instructions, so that G keeps 16 mantissa bits), B = 8 strided elements of a.
// Tower columns: cls tower j = 0 cls_logits, j = 1 centerness unless centerness_on_reg; bbox tower j = 0 .. nreg-1 bbox_pred, j = nreg centerness if
// centerness_on_reg.  Rows of W16 past the tower's columns are zero.  Tap t = (a 3 + b) 3 + c reads voxel (w + a - 1, l + b - 1, h + c - 1): nn.Conv3d's order.
#include "common.hpp"
#include "kernels.hpp"

namespace {

constexpr int FH_MAX_LEVELS = 5;
constexpr int FH_MAX_JOBS = 2 * FH_MAX_LEVELS;
constexpr int FH_MAX_SPLITS = 64;
constexpr int FH_EW_MAX_BLOCKS = 1024;                 // per job, element-wise passes
constexpr int FH_NQ = 11;                              // partial sums of the pack pass: db_cls, db_ctr, db_box[8], dscale
constexpr int FH_WG_MAX_BLOCKS = 128;
constexpr long FH_WG_WS_FLOATS = 16L << 20;            // partial sums of the weight-gradient pass: at most 64 MiB

template <typename T> struct PtrJ { T* p[FH_MAX_JOBS]; };
template <typename T> struct PtrL { T* p[FH_MAX_LEVELS]; };
template <typename T> struct Ptr2 { T* p[2]; };

template <typename T, int M> bool fill(T* (&dst)[M], int n, T* const* tab, bool required = true) {
  for (int k = 0; k < M; ++k) {
    dst[k] = (tab && k < n) ? tab[k] : nullptr;
    if (required && k < n && !dst[k]) return true;
  }
  return false;
}

// ---- GroupNorm -----------------------------------------------------------------------------------------------------------------------------------
struct GnGeom {
  int J, N, C, G, cpg, oct, rows;                      // oct = C / 8 channel octets; rows = voxels a workgroup of the reduce pass reads at once
  int V[FH_MAX_JOBS], tower[FH_MAX_JOBS], S[FH_MAX_JOBS];
  int blk0[FH_MAX_JOBS + 1];                           // reduce pass: first workgroup (= first partial) of job j, N S[j] each
  int eb0[FH_MAX_JOBS + 1];                            // element-wise passes: first workgroup of job j
};

bool make_gn_geom(int njobs, const int* vox, const int* tower, int N, int C, int G, GnGeom& g) {
  if (njobs < 1 || njobs > FH_MAX_JOBS || !vox || N < 1 || N > 4096 || C < 32 || C % 32 || C > 2048 || G < 1 || C % G) return true;
  const int cpg = C / G;
  if (!(cpg == 1 || cpg == 2 || cpg == 4 || cpg % 8 == 0)) return true;          // an octet of channels lies in whole groups or inside one
  g.J = njobs; g.N = N; g.C = C; g.G = G; g.cpg = cpg; g.oct = C / 8; g.rows = 256 / g.oct;
  long rb = 0, eb = 0;
  for (int j = 0; j < FH_MAX_JOBS; ++j) {
    if (j < njobs) {
      if (vox[j] < 1 || (long)vox[j] * N > (1L << 30) / C * 8) return true;
      if (tower && (tower[j] < 0 || tower[j] > 1)) return true;
      g.V[j] = vox[j]; g.tower[j] = tower ? tower[j] : 0;
      int S = vox[j] / (g.rows * 16);
      g.S[j] = S < 1 ? 1 : (S > FH_MAX_SPLITS ? FH_MAX_SPLITS : S);
      g.blk0[j] = (int)rb; g.eb0[j] = (int)eb;
      rb += (long)N * g.S[j];
      long nb = ((long)N * vox[j] * g.oct + 255) / 256;
      eb += nb > FH_EW_MAX_BLOCKS ? FH_EW_MAX_BLOCKS : nb;
    } else {
      g.V[j] = 1; g.tower[j] = 0; g.S[j] = 1; g.blk0[j] = (int)rb; g.eb0[j] = (int)eb;
    }
  }
  if (rb > (1L << 24)) return true;
  g.blk0[FH_MAX_JOBS] = (int)rb; g.eb0[FH_MAX_JOBS] = (int)eb;
  return false;
}

__device__ __forceinline__ int job_of(const int (&start)[FH_MAX_JOBS + 1], int J, int b) {
  int j = 0;
  while (j + 1 < J && b >= start[j + 1]) ++j;
  return j;
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void gn_reduce_kernel(GnGeom g, PtrJ<const T> x, PtrJ<const T> y, PtrJ<const T> dy, const float* __restrict__ stats,
                                                        double* __restrict__ partials) {
  __shared__ double sm[256 * 16];
  const int b = blockIdx.x, j = job_of(g.blk0, g.J, b);
  const int S = g.S[j], V = g.V[j], rel = b - g.blk0[j], n = rel / S, s = rel - n * S;
  const int vb = (int)((long)s * V / S), ve = (int)((long)(s + 1) * V / S);
  const int t = threadIdx.x, o = t % g.oct, r = t / g.oct;
  double a[8], c[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = c[e] = 0.0;
  if (r < g.rows) {
    float mean[8], rstd[8];
    if (BWD) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float* st = stats + (((long)j * g.N + n) * g.G + (o * 8 + e) / g.cpg) * 2;
        mean[e] = st[0]; rstd[e] = st[1];
      }
    }
    const long base = (long)n * V * g.C + o * 8;
    const T* __restrict__ xp = x.p[j] + base;
    const T* __restrict__ yp = BWD ? y.p[j] + base : nullptr;
    const T* __restrict__ dp = BWD ? dy.p[j] + base : nullptr;
    for (int v = vb + r; v < ve; v += g.rows) {
      float xv[8];
      Vec8<T>::load(xp + (long)v * g.C, xv);
      if (BWD) {
        float yv[8], dv[8];
        Vec8<T>::load(yp + (long)v * g.C, yv);
        Vec8<T>::load(dp + (long)v * g.C, dv);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float m = yv[e] > 0.f ? dv[e] : 0.f;
          a[e] += (double)(m * ((xv[e] - mean[e]) * rstd[e]));
          c[e] += (double)m;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { a[e] += (double)xv[e]; c[e] += (double)xv[e] * (double)xv[e]; }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) { sm[t * 16 + e] = a[e]; sm[t * 16 + 8 + e] = c[e]; }
  __syncthreads();
  for (int idx = t; idx < g.oct * 16; idx += 256) {
    const int oo = idx >> 4, k = idx & 15;
    double sum = 0.0;
    for (int rr = 0; rr < g.rows; ++rr) sum += sm[(rr * g.oct + oo) * 16 + k];      // row order: fixed
    partials[((long)b * g.C + oo * 8 + (k & 7)) * 2 + (k >> 3)] = sum;
  }
}

__global__ __launch_bounds__(256) void gn_finalize_kernel(GnGeom g, const double* __restrict__ partials, float eps, float* __restrict__ stats) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= g.J * g.N * g.G) return;
  const int gi = idx % g.G, n = (idx / g.G) % g.N, j = idx / (g.G * g.N);
  const int S = g.S[j], p0 = g.blk0[j] + n * S;
  double A = 0.0, B = 0.0;
  for (int s = 0; s < S; ++s)
    for (int c = gi * g.cpg; c < (gi + 1) * g.cpg; ++c) {
      const double* p = partials + ((long)(p0 + s) * g.C + c) * 2;
      A += p[0]; B += p[1];
    }
  const double cnt = (double)g.cpg * (double)g.V[j], mean = A / cnt;
  double var = B / cnt - mean * mean;
  if (var < 0.0) var = 0.0;
  stats[(long)idx * 2] = (float)mean;
  stats[(long)idx * 2 + 1] = (float)(1.0 / sqrt(var + (double)eps));
}

template <typename T>
__global__ __launch_bounds__(256) void gn_apply_kernel(GnGeom g, PtrJ<const T> x, const float* __restrict__ stats, Ptr2<const float> gamma, Ptr2<const float> beta, PtrJ<T> y) {
  const int b = blockIdx.x, j = job_of(g.eb0, g.J, b);
  const int V = g.V[j], nbj = g.eb0[j + 1] - g.eb0[j];
  const long total = (long)g.N * V * g.oct;
  const float* __restrict__ gam = gamma.p[g.tower[j]];
  const float* __restrict__ bet = beta.p[g.tower[j]];
  const T* __restrict__ xp = x.p[j];
  T* __restrict__ yp = y.p[j];
  for (long i = (long)(b - g.eb0[j]) * 256 + threadIdx.x; i < total; i += (long)nbj * 256) {
    const int o = (int)(i % g.oct);
    const int n = (int)(i / g.oct / V);
    float xv[8];
    Vec8<T>::load(xp + i * 8, xv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = o * 8 + e;
      const float* st = stats + (((long)j * g.N + n) * g.G + c / g.cpg) * 2;
      const float v = ((xv[e] - st[0]) * st[1]) * gam[c] + bet[c];
      xv[e] = v > 0.f ? v : 0.f;
    }
    Vec8<T>::store(yp + i * 8, xv);
  }
}

__global__ __launch_bounds__(256) void gn_bwd_finalize_kernel(GnGeom g, const double* __restrict__ partials, Ptr2<const float> gamma, float* __restrict__ sums, Ptr2<float> dgamma,
                                                              Ptr2<float> dbeta) {
  const int idx = blockIdx.x * 256 + threadIdx.x, ng = g.J * g.N * g.G;
  if (idx < ng) {
    const int gi = idx % g.G, n = (idx / g.G) % g.N, j = idx / (g.G * g.N);
    const int S = g.S[j], p0 = g.blk0[j] + n * S;
    const float* __restrict__ gam = gamma.p[g.tower[j]];
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < S; ++s)
      for (int c = gi * g.cpg; c < (gi + 1) * g.cpg; ++c) {
        const double* p = partials + ((long)(p0 + s) * g.C + c) * 2;
        s2 += (double)gam[c] * p[0]; s1 += (double)gam[c] * p[1];
      }
    const double cnt = (double)g.cpg * (double)g.V[j];
    sums[(long)idx * 2] = (float)(s1 / cnt);
    sums[(long)idx * 2 + 1] = (float)(s2 / cnt);
    return;
  }
  const int k = idx - ng;
  if (k >= 2 * g.C) return;
  const int tw = k / g.C, c = k - tw * g.C;
  if (!dgamma.p[tw] || !dbeta.p[tw]) return;
  double A = 0.0, B = 0.0;
  bool any = false;
  for (int j = 0; j < g.J; ++j) {                      // job, scene, split order: fixed
    if (g.tower[j] != tw) continue;
    any = true;
    for (int p = g.blk0[j]; p < g.blk0[j] + g.N * g.S[j]; ++p) {
      const double* q = partials + ((long)p * g.C + c) * 2;
      A += q[0]; B += q[1];
    }
  }
  if (any) { dgamma.p[tw][c] += (float)A; dbeta.p[tw][c] += (float)B; }
}

template <typename T>
__global__ __launch_bounds__(256) void gn_bwd_apply_kernel(GnGeom g, PtrJ<const T> dy, PtrJ<const T> x, PtrJ<const T> y, const float* __restrict__ stats,
                                                           const float* __restrict__ sums, Ptr2<const float> gamma, PtrJ<T> dx) {
  const int b = blockIdx.x, j = job_of(g.eb0, g.J, b);
  const int V = g.V[j], nbj = g.eb0[j + 1] - g.eb0[j];
  const long total = (long)g.N * V * g.oct;
  const float* __restrict__ gam = gamma.p[g.tower[j]];
  const T* __restrict__ xp = x.p[j];
  const T* __restrict__ yp = y.p[j];
  const T* __restrict__ dp = dy.p[j];
  T* __restrict__ op = dx.p[j];
  for (long i = (long)(b - g.eb0[j]) * 256 + threadIdx.x; i < total; i += (long)nbj * 256) {
    const int o = (int)(i % g.oct);
    const int n = (int)(i / g.oct / V);
    float xv[8], yv[8], dv[8];
    Vec8<T>::load(xp + i * 8, xv);
    Vec8<T>::load(yp + i * 8, yv);
    Vec8<T>::load(dp + i * 8, dv);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = o * 8 + e;
      const long q = (((long)j * g.N + n) * g.G + c / g.cpg) * 2;
      const float rstd = stats[q + 1], xh = (xv[e] - stats[q]) * rstd;
      const float dh = yv[e] > 0.f ? dv[e] * gam[c] : 0.f;
      xv[e] = rstd * (dh - sums[q] - xh * sums[q + 1]);
    }
    Vec8<T>::store(op + i * 8, xv);
  }
}

// ---- output stage --------------------------------------------------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ Frag<T> frag_zero();
template <> __device__ __forceinline__ Frag<bf16_t> frag_zero<bf16_t>() { Frag<bf16_t> f; f.v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; return f; }
template <> __device__ __forceinline__ Frag<float> frag_zero<float>() {
  Frag<float> f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f.v[e] = 0.f;
  return f;
}
__device__ __forceinline__ Frag<bf16_t> frag_load(const bf16_t* p) { Frag<bf16_t> f; f.v = *reinterpret_cast<const bf16x8*>(p); return f; }
__device__ __forceinline__ Frag<float> frag_load(const float* p) {
  Frag<float> f;
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  f.v[0] = a.x; f.v[1] = a.y; f.v[2] = a.z; f.v[3] = a.w; f.v[4] = b.x; f.v[5] = b.y; f.v[6] = b.z; f.v[7] = b.w;
  return f;
}

enum { FH_MODE_TRAIN = 0, FH_MODE_EVAL = 1, FH_MODE_EXP = 2 };

struct OutGeom {
  int L, N, C, nreg, ctr_on_reg, mode, total;          // total = 64-voxel wave tiles of all jobs
  int W[FH_MAX_LEVELS], Lh[FH_MAX_LEVELS], H[FH_MAX_LEVELS];
  float stride[FH_MAX_LEVELS];
  int tile0[FH_MAX_JOBS + 1];                          // job 2 l + tower: N ceil(V / 64) tiles
  int step0[FH_MAX_LEVELS + 1];                        // weight gradient: 32-voxel steps, N ceil(V / 32) per level
  int pb0[FH_MAX_LEVELS + 1];                          // pack pass: workgroups, ceil(N V / 256) per level
};

bool make_out_geom(int nlevels, const int* dims, const float* strides, int N, int C, int nreg, int ctr_on_reg, int mode, OutGeom& g) {
  if (nlevels < 1 || nlevels > FH_MAX_LEVELS || !dims || N < 1 || N > 4096 || C < 32 || C % 32 || C > 2048 || (nreg != 6 && nreg != 8) || mode < 0 || mode > 2) return true;
  g.L = nlevels; g.N = N; g.C = C; g.nreg = nreg; g.ctr_on_reg = ctr_on_reg ? 1 : 0; g.mode = mode;
  long tiles = 0, steps = 0, pb = 0;
  for (int l = 0; l < FH_MAX_LEVELS; ++l) {
    if (l < nlevels) {
      const int W = dims[3 * l], Lh = dims[3 * l + 1], H = dims[3 * l + 2];
      if (W < 1 || Lh < 1 || H < 1 || (long)W * Lh * H * N > (1L << 30) / C * 8) return true;
      const long V = (long)W * Lh * H;
      g.W[l] = W; g.Lh[l] = Lh; g.H[l] = H; g.stride[l] = strides ? strides[l] : 1.f;
      g.tile0[2 * l] = (int)tiles; tiles += N * ((V + 63) / 64);
      g.tile0[2 * l + 1] = (int)tiles; tiles += N * ((V + 63) / 64);
      g.step0[l] = (int)steps; steps += N * ((V + 31) / 32);
      g.pb0[l] = (int)pb; pb += (N * V + 255) / 256;
    } else {
      g.W[l] = g.Lh[l] = g.H[l] = 1; g.stride[l] = 1.f;
      g.tile0[2 * l] = g.tile0[2 * l + 1] = (int)tiles; g.step0[l] = (int)steps; g.pb0[l] = (int)pb;
    }
  }
  if (tiles > (1L << 28)) return true;
  g.total = (int)tiles; g.tile0[FH_MAX_JOBS] = (int)tiles; g.step0[FH_MAX_LEVELS] = (int)steps; g.pb0[FH_MAX_LEVELS] = (int)pb;
  return false;
}

__device__ __forceinline__ int level_of(const int (&start)[FH_MAX_LEVELS + 1], int L, int b) {
  int l = 0;
  while (l + 1 < L && b >= start[l + 1]) ++l;
  return l;
}

template <typename T>
__global__ __launch_bounds__(256) void out_fwd_kernel(OutGeom g, PtrJ<const T> act, Ptr2<const T> w16, const float* __restrict__ bcls, const float* __restrict__ bbox,
                                                      const float* __restrict__ bctr, PtrL<const float> scale, PtrL<float> cls, PtrL<float> reg, PtrL<float> ctr, PtrL<float> usave) {
  const int lane = threadIdx.x & 63, i = lane & 15, gq = lane >> 4;
  const int wt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wt >= g.total) return;
  const int j = job_of(g.tile0, 2 * g.L, wt), l = j >> 1, tw = j & 1;
  const int W = g.W[l], Lh = g.Lh[l], H = g.H[l], V = W * Lh * H, C = g.C;
  const int tps = (V + 63) / 64, rel = wt - g.tile0[j], n = rel / tps, v0 = (rel - n * tps) * 64;
  const T* __restrict__ xa = act.p[j] + (long)n * V * C + 8 * gq;
  const T* __restrict__ wp = w16.p[tw] + (long)i * 27 * C + 8 * gq;
  int cw[4], cl[4], ch[4];
  bool vin[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int v = v0 + 16 * q + i;
    vin[q] = v < V;
    const int vv = vin[q] ? v : 0, t = vv / H;
    ch[q] = vv - t * H; cw[q] = t / Lh; cl[q] = t - cw[q] * Lh;
  }
  f32x4 acc[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int tap = 0; tap < 27; ++tap) {
    const int da = tap / 9 - 1, db = (tap / 3) % 3 - 1, dc = tap % 3 - 1;
    const T* xq[4];
    bool ok[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int a = cw[q] + da, b = cl[q] + db, c = ch[q] + dc;
      ok[q] = vin[q] && a >= 0 && a < W && b >= 0 && b < Lh && c >= 0 && c < H;
      xq[q] = xa + (ok[q] ? ((long)(a * Lh + b) * H + c) * C : 0L);
    }
    if (!__any(ok[0] || ok[1] || ok[2] || ok[3])) continue;       // wave-uniform
    const T* __restrict__ wt_ = wp + (long)tap * C;
    for (int c0 = 0; c0 < C; c0 += 32) {
      const Frag<T> A = frag_load(wt_ + c0);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const Frag<T> B = ok[q] ? frag_load(xq[q] + c0) : frag_zero<T>();
        mma(acc[q], A, B);
      }
    }
  }
  const int nreg = g.nreg;
  const float sc = tw ? *scale.p[l] : 1.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int v = v0 + 16 * q + i;
    if (!vin[q]) continue;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int col = 4 * gq + r;
      const float a = acc[q][r];
      if (tw == 0) {
        if (col == 0) cls.p[l][(long)n * V + v] = a + bcls[0];
        else if (col == 1 && !g.ctr_on_reg) ctr.p[l][(long)n * V + v] = a + bctr[0];
      } else if (col < nreg) {
        const float u = a + bbox[col], z = u * sc;
        float out;
        if (g.mode == FH_MODE_EXP) out = expf(z);
        else {
          out = col < 6 ? (z > 0.f ? z : 0.f) : z;
          if (g.mode == FH_MODE_EVAL && col < 6) out *= g.stride[l];
        }
        const long at = ((long)n * nreg + col) * V + v;
        usave.p[l][at] = u;
        reg.p[l][at] = out;
      } else if (col == nreg && g.ctr_on_reg) ctr.p[l][(long)n * V + v] = a + bctr[0];
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void out_bwd_pack_kernel(OutGeom g, PtrL<const float> gcls, PtrL<const float> greg, PtrL<const float> gctr, PtrL<const float> usave,
                                                           PtrL<const float> scale, PtrJ<T> g16, PtrJ<float> gt, float* __restrict__ partials) {
  __shared__ float sm[4][FH_NQ];
  const int b = blockIdx.x, l = level_of(g.pb0, g.L, b);
  const int V = g.W[l] * g.Lh[l] * g.H[l], nreg = g.nreg;
  const long idx = (long)(b - g.pb0[l]) * 256 + threadIdx.x;
  const bool active = idx < (long)g.N * V;
  float q[FH_NQ], rc[16], rb[16];
#pragma unroll
  for (int k = 0; k < FH_NQ; ++k) q[k] = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k) rc[k] = rb[k] = 0.f;
  if (active) {
    const int n = (int)(idx / V), v = (int)(idx - (long)n * V);
    const float gc = gcls.p[l][idx], gk = gctr.p[l][idx], sc = *scale.p[l];
    q[0] = gc; q[1] = gk; rc[0] = gc;
    if (!g.ctr_on_reg) rc[1] = gk;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      if (k < nreg) {
        const long at = ((long)n * nreg + k) * V + v;
        const float u = usave.p[l][at], gg = greg.p[l][at], z = u * sc;
        float gz;
        if (g.mode == FH_MODE_EXP) gz = gg * expf(z);
        else {
          gz = (k >= 6 || z > 0.f) ? gg : 0.f;
          if (g.mode == FH_MODE_EVAL && k < 6) gz *= g.stride[l];
        }
        const float du = gz * sc;
        rb[k] = du; q[2 + k] = du; q[10] += gz * u;
      }
    }
    if (g.ctr_on_reg) { if (nreg == 6) rb[6] = gk; else rb[8] = gk; }
    float lo[8], hi[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { lo[k] = rc[k]; hi[k] = rc[8 + k]; }
    Vec8<T>::store(g16.p[2 * l] + idx * 16, lo);
    Vec8<T>::store(g16.p[2 * l] + idx * 16 + 8, hi);
#pragma unroll
    for (int k = 0; k < 8; ++k) { lo[k] = rb[k]; hi[k] = rb[8 + k]; }
    Vec8<T>::store(g16.p[2 * l + 1] + idx * 16, lo);
    Vec8<T>::store(g16.p[2 * l + 1] + idx * 16 + 8, hi);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      gt.p[2 * l][((long)n * 16 + k) * V + v] = rc[k];
      gt.p[2 * l + 1][((long)n * 16 + k) * V + v] = rb[k];
    }
  }
#pragma unroll
  for (int k = 0; k < FH_NQ; ++k) q[k] = wave_sum(q[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < FH_NQ; ++k) sm[threadIdx.x >> 6][k] = q[k];
  }
  __syncthreads();
  if (threadIdx.x < FH_NQ) partials[(long)b * FH_NQ + threadIdx.x] = ((sm[0][threadIdx.x] + sm[1][threadIdx.x]) + sm[2][threadIdx.x]) + sm[3][threadIdx.x];
}

// workgroup k < 10: bias quantity k over the workgroups of every level; k >= 10: dscale of level k - 10.  Lane-strided sums in fp64, then a butterfly: fixed order.
__global__ __launch_bounds__(64) void out_bwd_red_kernel(OutGeom g, const float* __restrict__ partials, float* __restrict__ db_cls, float* __restrict__ db_box, float* __restrict__ db_ctr,
                                                         PtrL<float> dscale) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int l = k - 10, qi = k < 10 ? k : 10;
  if (k >= 10 && l >= g.L) return;
  const int lo = k < 10 ? 0 : g.pb0[l], hi = k < 10 ? g.pb0[g.L] : g.pb0[l + 1];
  double s = 0.0;
  for (int b = lo + lane; b < hi; b += 64) s += (double)partials[(long)b * FH_NQ + qi];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (lane != 0) return;
  if (k == 0) db_cls[0] += (float)s;
  else if (k == 1) db_ctr[0] += (float)s;
  else if (k < 10) { if (k - 2 < g.nreg) db_box[k - 2] += (float)s; }
  else if (dscale.p[l]) *dscale.p[l] += (float)s;
}

template <typename T> struct WideFrag;
template <> struct WideFrag<bf16_t> {
  Frag<bf16_t> hi, lo;
  template <int E> __device__ __forceinline__ void set(float x) {
    const bf16_t h = f2bf(x);
    hi.v[E] = (short)h; lo.v[E] = (short)f2bf(x - bf2f(h));
  }
  __device__ __forceinline__ void mma_into(f32x4& acc, const Frag<bf16_t>& b) const { mma(acc, hi, b); mma(acc, lo, b); }
};
template <> struct WideFrag<float> {
  Frag<float> f;
  template <int E> __device__ __forceinline__ void set(float x) { f.v[E] = x; }
  __device__ __forceinline__ void mma_into(f32x4& acc, const Frag<float>& b) const { mma(acc, f, b); }
};
template <int E> __device__ __forceinline__ void frag_set(Frag<bf16_t>& f, bf16_t x) { f.v[E] = (short)x; }
template <int E> __device__ __forceinline__ void frag_set(Frag<float>& f, float x) { f.v[E] = x; }

// Workgroup (b, tower) sums the steps [b steps / nb, (b + 1) steps / nb) of every level into its partial image [16][27][C]; the (tap, 32-channel) output
// tiles go round the 4 waves and every wave walks all the workgroup's steps for each of its tiles.
template <typename T>
__global__ __launch_bounds__(256) void out_wgrad_kernel(OutGeom g, PtrJ<const T> act, PtrJ<const float> gt, float* __restrict__ partials) {
  const int lane = threadIdx.x & 63, i = lane & 15, gq = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nb = gridDim.x, b = blockIdx.x, tw = blockIdx.y, C = g.C, nct = C / 32;
  const int steps = g.step0[g.L];
  const int sb = (int)((long)b * steps / nb), se = (int)((long)(b + 1) * steps / nb);
  float* __restrict__ P = partials + ((long)tw * nb + b) * 16 * 27 * C;
  for (int it = wave; it < 27 * nct; it += 4) {
    const int tap = it / nct, c0 = (it - tap * nct) * 32;
    const int da = tap / 9 - 1, db = (tap / 3) % 3 - 1, dc = tap % 3 - 1;
    f32x4 acc0 = f32x4{0.f, 0.f, 0.f, 0.f}, acc1 = acc0;
    for (int st = sb; st < se; ++st) {
      const int l = level_of(g.step0, g.L, st);
      const int W = g.W[l], Lh = g.Lh[l], H = g.H[l], V = W * Lh * H;
      const int spl = (V + 31) / 32, rel = st - g.step0[l], n = rel / spl, vb = (rel - n * spl) * 32 + 8 * gq;
      const float* __restrict__ gp = gt.p[2 * l + tw] + ((long)n * 16 + i) * V;
      const T* __restrict__ ap = act.p[2 * l + tw] + (long)n * V * C + c0 + i;
      WideFrag<T> A;
      Frag<T> B0 = frag_zero<T>(), B1 = frag_zero<T>();
      ForE<0, 8>::run([&](auto I) {
        constexpr int E = decltype(I)::value;
        const int v = vb + E;
        float gv = 0.f;
        if (v < V) {
          gv = gp[v];
          const int t = v / H, c = v - t * H + dc, a0 = t / Lh, bb = t - a0 * Lh + db, a = a0 + da;
          if (a >= 0 && a < W && bb >= 0 && bb < Lh && c >= 0 && c < H) {
            const T* src = ap + ((long)(a * Lh + bb) * H + c) * C;
            frag_set<E>(B0, src[0]);
            frag_set<E>(B1, src[16]);
          }
        }
        A.template set<E>(gv);
      });
      A.mma_into(acc0, B0);
      A.mma_into(acc1, B1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float* row = P + ((long)(4 * gq + r) * 27 + tap) * C + c0 + i;
      row[0] = acc0[r];
      row[16] = acc1[r];
    }
  }
}

__global__ __launch_bounds__(256) void out_wgrad_red_kernel(int nb, int C, int nreg, int ctr_on_reg, const float* __restrict__ partials, float* __restrict__ dw_cls,
                                                            float* __restrict__ dw_box, float* __restrict__ dw_ctr) {
  const long per = 16L * 27 * C, e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= 2 * per) return;
  const int tw = (int)(e / per);
  const long r = e - tw * per;
  const int j = (int)(r / (27 * C)), tap = (int)(r / C % 27), c = (int)(r % C);
  float* d;
  if (tw == 0) {
    if (j == 0) d = dw_cls + (long)c * 27 + tap;
    else if (j == 1 && !ctr_on_reg) d = dw_ctr + (long)c * 27 + tap;
    else return;
  } else {
    if (j < nreg) d = dw_box + ((long)j * C + c) * 27 + tap;
    else if (j == nreg && ctr_on_reg) d = dw_ctr + (long)c * 27 + tap;
    else return;
  }
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += partials[((long)tw * nb + b) * per + r];       // workgroup order: fixed
  *d += s;
}

int wgrad_blocks(const OutGeom& g) {
  long nb = g.step0[g.L] < FH_WG_MAX_BLOCKS ? g.step0[g.L] : FH_WG_MAX_BLOCKS;
  const long per = 2L * 16 * 27 * g.C;
  if (nb * per > FH_WG_WS_FLOATS) nb = FH_WG_WS_FLOATS / per;
  return nb < 1 ? 1 : (int)nb;
}

}  // namespace

long k_fcos_gn_ws_doubles(int njobs, const int* vox, int N, int C) {
  GnGeom g;
  if (make_gn_geom(njobs, vox, nullptr, N, C, 1, g)) return -1;
  return (long)g.blk0[FH_MAX_JOBS] * C * 2;
}

int k_fcos_gn_stats(int dt, int njobs, const int* vox, int N, int C, int G, float eps, const void* const* x, double* ws, float* stats, hipStream_t st) {
  GnGeom g;
  if (make_gn_geom(njobs, vox, nullptr, N, C, G, g)) return -4;
  const dim3 grid((unsigned)g.blk0[FH_MAX_JOBS]);
  if (dt == NMH_DT_BF16) {
    PtrJ<const bf16_t> X, Z{};
    if (fill(X.p, njobs, (const bf16_t* const*)x)) return -4;
    hipLaunchKernelGGL((gn_reduce_kernel<bf16_t, false>), grid, dim3(256), 0, st, g, X, Z, Z, (const float*)nullptr, ws);
  } else if (dt == NMH_DT_F32) {
    PtrJ<const float> X, Z{};
    if (fill(X.p, njobs, (const float* const*)x)) return -4;
    hipLaunchKernelGGL((gn_reduce_kernel<float, false>), grid, dim3(256), 0, st, g, X, Z, Z, (const float*)nullptr, ws);
  } else return -1;
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_finalize_kernel, dim3((unsigned)((g.J * g.N * g.G + 255) / 256)), dim3(256), 0, st, g, (const double*)ws, eps, stats);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_gn_apply(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* x, const float* stats, const float* const* gamma,
                    const float* const* beta, void* const* y, hipStream_t st) {
  GnGeom g;
  if (make_gn_geom(njobs, vox, tower, N, C, G, g)) return -4;
  Ptr2<const float> GA, BE;
  fill(GA.p, 2, gamma, false); fill(BE.p, 2, beta, false);
  for (int j = 0; j < njobs; ++j) if (!GA.p[tower[j]] || !BE.p[tower[j]]) return -4;
  const dim3 grid((unsigned)g.eb0[FH_MAX_JOBS]);
  if (dt == NMH_DT_BF16) {
    PtrJ<const bf16_t> X; PtrJ<bf16_t> Y;
    if (fill(X.p, njobs, (const bf16_t* const*)x) || fill(Y.p, njobs, (bf16_t* const*)y)) return -4;
    hipLaunchKernelGGL(gn_apply_kernel<bf16_t>, grid, dim3(256), 0, st, g, X, stats, GA, BE, Y);
  } else if (dt == NMH_DT_F32) {
    PtrJ<const float> X; PtrJ<float> Y;
    if (fill(X.p, njobs, (const float* const*)x) || fill(Y.p, njobs, (float* const*)y)) return -4;
    hipLaunchKernelGGL(gn_apply_kernel<float>, grid, dim3(256), 0, st, g, X, stats, GA, BE, Y);
  } else return -1;
  NMH_CHECK_LAUNCH();
  return 0;
}

template <typename T>
static int gn_bwd_launch(const GnGeom& g, int njobs, const void* const* dy, const void* const* x, const void* const* y, const float* stats, const Ptr2<const float>& GA,
                         double* ws, float* sums, const Ptr2<float>& DG, const Ptr2<float>& DB, void* const* dx, hipStream_t st) {
  PtrJ<const T> DY, X, Y; PtrJ<T> DX;
  if (fill(DY.p, njobs, (const T* const*)dy) || fill(X.p, njobs, (const T* const*)x) || fill(Y.p, njobs, (const T* const*)y) || fill(DX.p, njobs, (T* const*)dx)) return -4;
  hipLaunchKernelGGL((gn_reduce_kernel<T, true>), dim3((unsigned)g.blk0[FH_MAX_JOBS]), dim3(256), 0, st, g, X, Y, DY, stats, ws);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_bwd_finalize_kernel, dim3((unsigned)((g.J * g.N * g.G + 2 * g.C + 255) / 256)), dim3(256), 0, st, g, (const double*)ws, GA, sums, DG, DB);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_bwd_apply_kernel<T>, dim3((unsigned)g.eb0[FH_MAX_JOBS]), dim3(256), 0, st, g, DY, X, Y, stats, (const float*)sums, GA, DX);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_fcos_gn_bwd(int dt, int njobs, const int* vox, const int* tower, int N, int C, int G, const void* const* dy, const void* const* x, const void* const* y, const float* stats,
                  const float* const* gamma, double* ws, float* sums, float* const* dgamma, float* const* dbeta, void* const* dx, hipStream_t st) {
  GnGeom g;
  if (make_gn_geom(njobs, vox, tower, N, C, G, g)) return -4;
  Ptr2<const float> GA; Ptr2<float> DG, DB;
  fill(GA.p, 2, gamma, false); fill(DG.p, 2, dgamma, false); fill(DB.p, 2, dbeta, false);
  for (int j = 0; j < njobs; ++j) if (!GA.p[tower[j]] || !DG.p[tower[j]] || !DB.p[tower[j]]) return -4;
  if (dt == NMH_DT_BF16) return gn_bwd_launch<bf16_t>(g, njobs, dy, x, y, stats, GA, ws, sums, DG, DB, dx, st);
  if (dt == NMH_DT_F32) return gn_bwd_launch<float>(g, njobs, dy, x, y, stats, GA, ws, sums, DG, DB, dx, st);
  return -1;
}

int k_fcos_out_fwd(int dt, int nlevels, const int* dims, const float* strides, int N, int C, int nreg, int ctr_on_reg, int mode, const void* const* act, const void* const* w16,
                   const float* b_cls, const float* b_box, const float* b_ctr, const float* const* scale, float* const* cls, float* const* reg, float* const* ctr,
                   float* const* u, hipStream_t st) {
  OutGeom g;
  if (make_out_geom(nlevels, dims, strides, N, C, nreg, ctr_on_reg, mode, g)) return -4;
  PtrL<const float> SC; PtrL<float> CL, RG, CT, US;
  if (fill(SC.p, nlevels, scale) || fill(CL.p, nlevels, cls) || fill(RG.p, nlevels, reg) || fill(CT.p, nlevels, ctr) || fill(US.p, nlevels, u)) return -4;
  const dim3 grid((unsigned)((g.total + 3) / 4));
  if (dt == NMH_DT_BF16) {
    PtrJ<const bf16_t> A; Ptr2<const bf16_t> Wt;
    if (fill(A.p, 2 * nlevels, (const bf16_t* const*)act) || fill(Wt.p, 2, (const bf16_t* const*)w16)) return -4;
    hipLaunchKernelGGL(out_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, g, A, Wt, b_cls, b_box, b_ctr, SC, CL, RG, CT, US);
  } else if (dt == NMH_DT_F32) {
    PtrJ<const float> A; Ptr2<const float> Wt;
    if (fill(A.p, 2 * nlevels, (const float* const*)act) || fill(Wt.p, 2, (const float* const*)w16)) return -4;
    hipLaunchKernelGGL(out_fwd_kernel<float>, grid, dim3(256), 0, st, g, A, Wt, b_cls, b_box, b_ctr, SC, CL, RG, CT, US);
  } else return -1;
  NMH_CHECK_LAUNCH();
  return 0;
}

long k_fcos_out_pack_ws_floats(int nlevels, const int* dims, int N) {
  OutGeom g;
  if (make_out_geom(nlevels, dims, nullptr, N, 32, 6, 1, 0, g)) return -1;
  return (long)g.pb0[FH_MAX_LEVELS] * FH_NQ;
}

int k_fcos_out_bwd_pack(int dt, int nlevels, const int* dims, const float* strides, int N, int nreg, int ctr_on_reg, int mode, const float* const* g_cls, const float* const* g_reg,
                        const float* const* g_ctr, const float* const* u, const float* const* scale, void* const* g16, float* const* gt, float* partials, float* db_cls,
                        float* db_box, float* db_ctr, float* const* dscale, hipStream_t st) {
  OutGeom g;
  if (make_out_geom(nlevels, dims, strides, N, 32, nreg, ctr_on_reg, mode, g)) return -4;
  PtrL<const float> GC, GR, GK, US, SC; PtrL<float> DS; PtrJ<float> GT;
  if (fill(GC.p, nlevels, g_cls) || fill(GR.p, nlevels, g_reg) || fill(GK.p, nlevels, g_ctr) || fill(US.p, nlevels, u) || fill(SC.p, nlevels, scale) ||
      fill(DS.p, nlevels, dscale) || fill(GT.p, 2 * nlevels, gt)) return -4;
  const dim3 grid((unsigned)g.pb0[FH_MAX_LEVELS]);
  if (dt == NMH_DT_BF16) {
    PtrJ<bf16_t> G16;
    if (fill(G16.p, 2 * nlevels, (bf16_t* const*)g16)) return -4;
    hipLaunchKernelGGL(out_bwd_pack_kernel<bf16_t>, grid, dim3(256), 0, st, g, GC, GR, GK, US, SC, G16, GT, partials);
  } else if (dt == NMH_DT_F32) {
    PtrJ<float> G16;
    if (fill(G16.p, 2 * nlevels, (float* const*)g16)) return -4;
    hipLaunchKernelGGL(out_bwd_pack_kernel<float>, grid, dim3(256), 0, st, g, GC, GR, GK, US, SC, G16, GT, partials);
  } else return -1;
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(out_bwd_red_kernel, dim3(10 + FH_MAX_LEVELS), dim3(64), 0, st, g, (const float*)partials, db_cls, db_box, db_ctr, DS);
  NMH_CHECK_LAUNCH();
  return 0;
}

long k_fcos_out_wgrad_ws_floats(int nlevels, const int* dims, int N, int C) {
  OutGeom g;
  if (make_out_geom(nlevels, dims, nullptr, N, C, 6, 1, 0, g)) return -1;
  return (long)wgrad_blocks(g) * 2 * 16 * 27 * C;
}

int k_fcos_out_wgrad(int dt, int nlevels, const int* dims, int N, int C, int nreg, int ctr_on_reg, const void* const* act, const float* const* gt, float* partials, float* dw_cls,
                     float* dw_box, float* dw_ctr, hipStream_t st) {
  OutGeom g;
  if (make_out_geom(nlevels, dims, nullptr, N, C, nreg, ctr_on_reg, 0, g)) return -4;
  PtrJ<const float> GT;
  if (fill(GT.p, 2 * nlevels, gt)) return -4;
  const int nb = wgrad_blocks(g);
  if (dt == NMH_DT_BF16) {
    PtrJ<const bf16_t> A;
    if (fill(A.p, 2 * nlevels, (const bf16_t* const*)act)) return -4;
    hipLaunchKernelGGL(out_wgrad_kernel<bf16_t>, dim3(nb, 2), dim3(256), 0, st, g, A, GT, partials);
  } else if (dt == NMH_DT_F32) {
    PtrJ<const float> A;
    if (fill(A.p, 2 * nlevels, (const float* const*)act)) return -4;
    hipLaunchKernelGGL(out_wgrad_kernel<float>, dim3(nb, 2), dim3(256), 0, st, g, A, GT, partials);
  } else return -1;
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(out_wgrad_red_kernel, dim3((unsigned)((2L * 16 * 27 * C + 255) / 256)), dim3(256), 0, st, nb, C, nreg, g.ctr_on_reg, (const float*)partials, dw_cls, dw_box, dw_ctr);
  NMH_CHECK_LAUNCH();
  return 0;
}
