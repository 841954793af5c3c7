// Kernels of the dense-prediction heads fine-tuned on the MAE-pretrained encoder + decoder:
// SwinTransformer_VoxelSR_Pretrained_Skip / SwinTransformer_VoxelSemantics_Pretrained_Skip (nerf_rpn/model/feature_extractor.py:
// 1898-2244, 2521-2848).  The convolutions, norms and GEMMs of both heads are the kernels of the MAE path; what is new here is data
// movement around them and the two losses:
//   grid -> 8-channel channels-last input of `encoder1` (4 data channels + 4 zero channels: the GEMM engine contracts in units of 8);
//   nearest-neighbour upsampling of the head output with the channels-last -> NCDHW transposition folded in, and its adjoint
//     (nn.Upsample(scale_factor) followed by a 1x1x1 conv == the 1x1x1 conv followed by the upsampling: the head GEMM runs at the
//     decoder resolution, 4.1x fewer voxels for 160 -> 256);
//   masked RGB MSE of the super-resolution head and the masked, class-weighted cross entropy (+ soft-IoU sums) of the semantics head.
#include "common.hpp"
#include "kernels.hpp"

static inline unsigned hd_blocks(long n) { long b = (n + 255) / 256; return (unsigned)(b > 65535L * 16 ? 65535L * 16 : (b < 1 ? 1 : b)); }

// ---- (B,4,V) fp32 NCDHW grid -> [B*V][8] channels-last in the compute dtype, channels 4..7 zero --------------------------------
template <typename T> __global__ void grid_to_cl8_kernel(const float* __restrict__ src, T* __restrict__ dst, long V, long total) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / V, v = i - b * V;
    const float* s = src + b * 4 * V + v;
    float o[8] = {s[0], s[V], s[2 * V], s[3 * V], 0.f, 0.f, 0.f, 0.f};
    Vec8<T>::store(dst + i * 8, o);
  }
}
int k_grid_to_cl8(int dt, const float* src, void* dst, int B, long V, hipStream_t st) {
  const long total = (long)B * V;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(grid_to_cl8_kernel<bf16_t>, dim3(hd_blocks(total)), dim3(256), 0, st, src, (bf16_t*)dst, V, total);
  else hipLaunchKernelGGL(grid_to_cl8_kernel<float>, dim3(hd_blocks(total)), dim3(256), 0, st, src, (float*)dst, V, total);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ATen's nearest source index for an explicit scale_factor (upsample_nearest3d with scales): min(floorf(dst * (float)(1/scale)), in - 1)
__device__ __forceinline__ int nn_src(int d, float inv_scale, int in) {
  const int s = (int)floorf((float)d * inv_scale);
  return s < in - 1 ? s : in - 1;
}

// ---- head output: src [B*R^3][Cp] (compute dtype, channels-last, first Co columns valid) -> pred (B,Co,Ro,Ro,Ro) fp32, nearest ----
template <typename T> __global__ void cl_to_ncdhw_up_kernel(const T* __restrict__ src, float* __restrict__ dst, int Co, int Cp, int R, int Ro, float inv_scale, long total) {
  const long Vo = (long)Ro * Ro * Ro;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {   // i over (b, zo, yo, xo)
    const long b = i / Vo, vo = i - b * Vo;
    const int xo = (int)(vo % Ro), yo = (int)((vo / Ro) % Ro), zo = (int)(vo / ((long)Ro * Ro));
    const long row = ((b * R + nn_src(zo, inv_scale, R)) * R + nn_src(yo, inv_scale, R)) * R + nn_src(xo, inv_scale, R);
    const T* s = src + row * Cp;
    for (int c = 0; c < Co; ++c) dst[(b * Co + c) * Vo + vo] = to_f<T>(s[c]);
  }
}
int k_cl_to_ncdhw_up(int dt, const void* src, float* dst, int B, int Co, int Cp, int R, int Ro, float inv_scale, hipStream_t st) {
  const long total = (long)B * Ro * Ro * Ro;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(cl_to_ncdhw_up_kernel<bf16_t>, dim3(hd_blocks(total)), dim3(256), 0, st, (const bf16_t*)src, dst, Co, Cp, R, Ro, inv_scale, total);
  else hipLaunchKernelGGL(cl_to_ncdhw_up_kernel<float>, dim3(hd_blocks(total)), dim3(256), 0, st, (const float*)src, dst, Co, Cp, R, Ro, inv_scale, total);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- adjoint: g[B*R^3][Cp] = sum over the output voxels that read each source voxel of dpred (B,Co,Ro^3) fp32; columns >= Co zero ----
__device__ __forceinline__ void nn_copies(int s, float inv_scale, int in, int out, int& lo, int& hi) {
  // [lo, hi): the output indices d with nn_src(d) == s.  Start from the real-valued estimate and correct for float rounding.
  int d = (int)ceilf((float)s / inv_scale);
  if (d > out) d = out;
  while (d > 0 && nn_src(d - 1, inv_scale, in) >= s) --d;
  while (d < out && nn_src(d, inv_scale, in) < s) ++d;
  lo = d;
  while (d < out && nn_src(d, inv_scale, in) == s) ++d;
  hi = d;
}
template <typename T> __global__ void ncdhw_up_adjoint_kernel(const float* __restrict__ dpred, T* __restrict__ g, int Co, int Cp, int R, int Ro, float inv_scale, long total) {
  const long Vo = (long)Ro * Ro * Ro, V = (long)R * R * R;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {   // i over (b, z, y, x) source voxels
    const long b = i / V, v = i - b * V;
    const int x = (int)(v % R), y = (int)((v / R) % R), z = (int)(v / ((long)R * R));
    int z0, z1, y0, y1, x0, x1;
    nn_copies(z, inv_scale, R, Ro, z0, z1);
    nn_copies(y, inv_scale, R, Ro, y0, y1);
    nn_copies(x, inv_scale, R, Ro, x0, x1);
    T* o = g + i * Cp;
    for (int c = 0; c < Cp; ++c) {
      float s = 0.f;
      if (c < Co) {
        const float* p = dpred + (b * Co + c) * Vo;
        for (int zo = z0; zo < z1; ++zo)
          for (int yo = y0; yo < y1; ++yo)
            for (int xo = x0; xo < x1; ++xo) s += p[((long)zo * Ro + yo) * Ro + xo];
      }
      o[c] = from_f<T>(s);
    }
  }
}
int k_ncdhw_up_adjoint(int dt, const float* dpred, void* g, int B, int Co, int Cp, int R, int Ro, float inv_scale, hipStream_t st) {
  const long total = (long)B * R * R * R;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(ncdhw_up_adjoint_kernel<bf16_t>, dim3(hd_blocks(total)), dim3(256), 0, st, dpred, (bf16_t*)g, Co, Cp, R, Ro, inv_scale, total);
  else hipLaunchKernelGGL(ncdhw_up_adjoint_kernel<float>, dim3(hd_blocks(total)), dim3(256), 0, st, dpred, (float*)g, Co, Cp, R, Ro, inv_scale, total);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- dst[m][0:C] += src[m][0:C] (fp32, row strides in elements): un-padding of weight gradients computed on padded operands ----
__global__ void add_cols_f32_kernel(const float* __restrict__ src, long lds, float* __restrict__ dst, long ldd, long M, int C) {
  const long n = M * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const long m = i / C;
    const int c = (int)(i - m * C);
    dst[m * ldd + c] += src[m * lds + c];
  }
}
int k_add_cols_f32(const float* src, long lds, float* dst, long ldd, long M, int C, hipStream_t st) {
  hipLaunchKernelGGL(add_cols_f32_kernel, dim3(hd_blocks(M * C)), dim3(256), 0, st, src, lds, dst, ldd, M, C);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- VoxelSR loss (feature_extractor.py:2133-2160): sums[0] = sum_v m (p_rgb - t_rgb)^2, sums[1] = sum_v m, m = t_alpha > 0.01 ----
__global__ __launch_bounds__(256) void sr_loss_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, long V, long total, double* __restrict__ sums,
                                                      float* __restrict__ dpred, const double* __restrict__ sums_in, float gscale) {
  // dpred == nullptr: forward sums; else backward: dpred = gscale * 2 m (p - t) / sums_in[1] on the RGB planes, 0 on the alpha plane
  __shared__ float sh[8];
  float s0 = 0.f, s1 = 0.f;
  const float k = dpred ? gscale * 2.0f / (float)sums_in[1] : 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / V, v = i - b * V;
    const float* p = pred + b * 4 * V + v;
    const float* t = tgt + b * 4 * V + v;
    const float m = t[3 * V] > 0.01f ? 1.f : 0.f;
    if (dpred) {
      float* d = dpred + b * 4 * V + v;
      d[0] = k * m * (p[0] - t[0]); d[V] = k * m * (p[V] - t[V]); d[2 * V] = k * m * (p[2 * V] - t[2 * V]); d[3 * V] = 0.f;
    } else {
      const float e0 = p[0] - t[0], e1 = p[V] - t[V], e2 = p[2 * V] - t[2 * V];
      s0 += m * (e0 * e0 + e1 * e1 + e2 * e2);
      s1 += m;
    }
  }
  if (dpred) return;
  s0 = wave_sum(s0); s1 = wave_sum(s1);
  if ((threadIdx.x & 63) == 0) { sh[(threadIdx.x >> 6) * 2] = s0; sh[(threadIdx.x >> 6) * 2 + 1] = s1; }
  __syncthreads();
  if (threadIdx.x == 0) {
    atomicAdd(sums, (double)(sh[0] + sh[2] + sh[4] + sh[6]));
    atomicAdd(sums + 1, (double)(sh[1] + sh[3] + sh[5] + sh[7]));
  }
}
__global__ void sr_loss_finalize_kernel(const double* sums, float* loss) { loss[0] = (float)(sums[0] / sums[1]); }
int k_sr_loss_fwd(const float* pred, const float* tgt, int B, long V, double* sums, float* loss, hipStream_t st) {
  hipError_t e = nmh_zero_async(sums, 2 * sizeof(double), st);
  if (e != hipSuccess) return (int)e;
  const long total = (long)B * V;
  unsigned nb = hd_blocks(total);
  if (nb > 2048) nb = 2048;
  hipLaunchKernelGGL(sr_loss_kernel, dim3(nb), dim3(256), 0, st, pred, tgt, V, total, sums, (float*)nullptr, (const double*)nullptr, 0.f);
  hipLaunchKernelGGL(sr_loss_finalize_kernel, dim3(1), dim3(1), 0, st, sums, loss);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_sr_loss_bwd(const float* pred, const float* tgt, int B, long V, const double* sums, float gscale, float* dpred, hipStream_t st) {
  const long total = (long)B * V;
  hipLaunchKernelGGL(sr_loss_kernel, dim3(hd_blocks(total)), dim3(256), 0, st, pred, tgt, V, total, (double*)nullptr, dpred, sums, gscale);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- VoxelSemantics loss (metrics.py:540-553 + nn.CrossEntropyLoss(weight); soft-IoU sums of mIoULoss_new, metrics.py:194-245) ----
// logits (B,K,V) fp32, labels (B,V) fp32 class ids (0 = unlabelled), cw [K] or null.  mask m = label > 0; the cross entropy runs over
// ALL voxels on (logits*m, label*m).  sums[0] = sum_v w nll, sums[1] = sum_v w; iou[b][k-1][3] = {sum_v m p_k, #(label == k), sum_{label==k} p_k}.
template <int KMAX>
__global__ __launch_bounds__(256) void masked_ce_kernel(const float* __restrict__ logits, const float* __restrict__ labels, const float* __restrict__ cw, int K, long V,
                                                        double* __restrict__ sums, double* __restrict__ iou, float* __restrict__ dlogits, const double* __restrict__ sums_in,
                                                        float gscale) {
  extern __shared__ float shm[];      // [2 + 3*(K-1)]
  const int b = blockIdx.y;
  const int nacc = 2 + 3 * (K - 1);
  if (!dlogits) {
    for (int i = threadIdx.x; i < nacc; i += 256) shm[i] = 0.f;
    __syncthreads();
  }
  const float inv_w = dlogits ? gscale / (float)sums_in[1] : 0.f;
  float s_nll = 0.f, s_w = 0.f;
  float sp[KMAX];                      // per-thread sums of m * p_k (256 threads adding to the same LDS words would serialise)
#pragma unroll
  for (int k = 0; k < KMAX; ++k) sp[k] = 0.f;
  const float* lg = logits + (long)b * K * V;
  for (long v = (long)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (long)gridDim.x * blockDim.x) {
    const int t = (int)labels[(long)b * V + v];
    const float m = t > 0 ? 1.f : 0.f;
    float l[KMAX], mx = -3.0e38f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) { l[k] = lg[(long)k * V + v]; mx = fmaxf(mx, l[k] * m); }
    float se = 0.f, sraw = 0.f, mraw = -3.0e38f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) { se += __expf(l[k] * m - mx); mraw = fmaxf(mraw, l[k]); }
    const int tm = t > 0 ? t : 0;
    const float w = cw ? cw[tm] : 1.f;
    if (dlogits) {
      float* dl = dlogits + (long)b * K * V + v;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) dl[(long)k * V] = m * w * inv_w * (__expf(l[k] * m - mx) / se - (k == tm ? 1.f : 0.f));
      continue;
    }
    const float lse = mx + __logf(se);
    float lt = 0.f;
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K && k == tm) lt = l[k] * m;
    s_nll += w * (lse - lt);
    s_w += w;
    // soft IoU terms use the softmax of the RAW logits (mIoULoss_new: F.softmax(inputs) * mask)
#pragma unroll
    for (int k = 0; k < KMAX; ++k)
      if (k < K) sraw += __expf(l[k] - mraw);
    if (t > 0) {
      const float rs = 1.f / sraw;
#pragma unroll
      for (int k = 1; k < KMAX; ++k)
        if (k < K) {
          const float p = __expf(l[k] - mraw) * rs;
          sp[k] += p;
          if (k == t) { atomicAdd(&shm[2 + (k - 1) * 3 + 1], 1.f); atomicAdd(&shm[2 + (k - 1) * 3 + 2], p); }   // one class per voxel: spread over K-1 words
        }
    }
  }
  if (dlogits) return;
  s_nll = wave_sum(s_nll); s_w = wave_sum(s_w);
  if ((threadIdx.x & 63) == 0) { atomicAdd(&shm[0], s_nll); atomicAdd(&shm[1], s_w); }
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K) {
      const float v = wave_sum(sp[k]);
      if ((threadIdx.x & 63) == 0) atomicAdd(&shm[2 + (k - 1) * 3], v);
    }
  __syncthreads();
  if (threadIdx.x < 2) atomicAdd(sums + threadIdx.x, (double)shm[threadIdx.x]);
  for (int i = threadIdx.x; i < 3 * (K - 1); i += 256) atomicAdd(iou + (long)b * 3 * (K - 1) + i, (double)shm[2 + i]);
}
__global__ void masked_ce_finalize_kernel(const double* sums, const double* iou, int B, int K, float* out) {
  // out[0] = weighted CE; out[1] = mean over (sample, class >= 1) of inter / (union + 1e-8), union = sum m p + count - inter
  if (threadIdx.x == 0) {
    out[0] = (float)(sums[0] / sums[1]);
    double acc = 0.0;
    for (int i = 0; i < B * (K - 1); ++i) {
      const double sp = iou[i * 3], cnt = iou[i * 3 + 1], inter = iou[i * 3 + 2];
      acc += inter / (sp + cnt - inter + 1e-8);
    }
    out[1] = (float)(acc / (B * (K - 1)));
  }
}
int k_masked_ce_fwd(const float* logits, const float* labels, const float* cw, int B, int K, long V, double* sums, double* iou, float* out, hipStream_t st) {
  if (K < 2 || K > 32) return -2;
  hipError_t e = nmh_zero_async(sums, 2 * sizeof(double), st);
  if (e == hipSuccess) e = nmh_zero_async(iou, sizeof(double) * 3 * (K - 1) * B, st);
  if (e != hipSuccess) return (int)e;
  unsigned nb = hd_blocks(V);
  if (nb > 1024) nb = 1024;
  hipLaunchKernelGGL(masked_ce_kernel<32>, dim3(nb, B), dim3(256), (2 + 3 * (K - 1)) * sizeof(float), st, logits, labels, cw, K, V, sums, iou, (float*)nullptr, (const double*)nullptr, 0.f);
  hipLaunchKernelGGL(masked_ce_finalize_kernel, dim3(1), dim3(64), 0, st, sums, iou, B, K, out);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_masked_ce_bwd(const float* logits, const float* labels, const float* cw, int B, int K, long V, const double* sums, float gscale, float* dlogits, hipStream_t st) {
  if (K < 2 || K > 32) return -2;
  hipLaunchKernelGGL(masked_ce_kernel<32>, dim3(hd_blocks(V), B), dim3(256), 0, st, logits, labels, cw, K, V, (double*)nullptr, (double*)nullptr, dlogits, sums, gscale);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- VoxelSemantics evaluation (feature_extractor.py:2748-2806 output_metrics + metrics.py:491-518 intersectionAndUnionGPU) ---------
// One read of the logits gives the loss scalars of masked_ce_fwd (same definitions; for a labelled voxel the masked and the raw logits are
// the same numbers, an unlabelled voxel contributes w[0] * log K and nothing else), the predicted label p(v) = arg-max of the RAW logits
// over all K classes (strict >, from class 0 up: the lowest index wins an exact tie), the two int64 label volumes and, per class
// c = 1..K-1 over the labelled voxels (label > 0), the exact counts  I[c] = #(p == c and label == c),  P[c] = #(p == c),
// T[c] = #(label == c).  A label >= K is a labelled voxel of no class: it can add to P, never to T or I, and weighs 0 in the loss.
// Counting: ballot + popcount, lane c of every wave owns class c (64-bit per-lane counters); floating sums: per-lane fp32, xor-tree over
// the wave, the four waves added in fp64 in order.  Every workgroup writes ONE row of two slabs -- fpart [row][2 + 2(K-1)] fp64 =
// {sum w nll, sum w, sum m p_k ..., sum_{label == k} p_k ...} and ipart [row][3(K-1)] int64 = {I.., P.., T..}, row = b * nb + block -- and one
// workgroup adds the rows in a fixed order: no atomics, no clearing launch, two runs give the same bits.
#define SEM_NF(K) (2 + 2 * ((K) - 1))
#define SEM_NI(K) (3 * ((K) - 1))

template <int KMAX>
__device__ __forceinline__ void sem_wave_counts(int p, int t, bool lab, int K, int lane, unsigned long long& ci, unsigned long long& cp, unsigned long long& ct) {
  // called by every lane of the wave (lanes past the end pass lab = false)
#pragma unroll
  for (int c = 1; c < KMAX; ++c)
    if (c < K) {
      const unsigned long long bt = __ballot(lab && t == c), bp = __ballot(lab && p == c);
      if (lane == c) { ct += __popcll(bt); cp += __popcll(bp); ci += __popcll(bt & bp); }
    }
}
// the wave's counters -> LDS [4 waves][3][32]; after a barrier thread i < 3(K-1) writes the workgroup's row
__device__ __forceinline__ void sem_counts_to_row(unsigned long long (*wc)[3][32], int K, unsigned long long ci, unsigned long long cp, unsigned long long ct,
                                                  long long* __restrict__ row) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane < 32) { wc[w][0][lane] = ci; wc[w][1][lane] = cp; wc[w][2][lane] = ct; }
  __syncthreads();
  if ((int)threadIdx.x < SEM_NI(K)) {
    const int j = threadIdx.x / (K - 1), c = 1 + threadIdx.x % (K - 1);
    row[threadIdx.x] = (long long)(wc[0][j][c] + wc[1][j][c] + wc[2][j][c] + wc[3][j][c]);
  }
}

template <int KMAX, int VEC>
__global__ __launch_bounds__(256) void sem_eval_kernel(const float* __restrict__ logits, const float* __restrict__ labels, const float* __restrict__ cw, int K, long V,
                                                       double* __restrict__ fpart, long long* __restrict__ ipart, long long* __restrict__ pred_vis,
                                                       long long* __restrict__ target_vis) {
  __shared__ float cwsh[32];
  __shared__ float fsh[4][SEM_NF(32)];
  __shared__ unsigned long long wc[4][3][32];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 32) cwsh[threadIdx.x] = (cw && (int)threadIdx.x < K) ? cw[threadIdx.x] : 1.f;
  __syncthreads();
  const float w0 = cwsh[0], logK = __logf((float)K);
  float s_nll = 0.f, s_w = 0.f, sp[KMAX], si[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) { sp[k] = 0.f; si[k] = 0.f; }
  unsigned long long ci = 0, cp = 0, ct = 0;
  const float* lg = logits + (long)b * K * V;
  const long step = (long)gridDim.x * 256 * VEC;
  for (long vb = (long)blockIdx.x * 256 * VEC; vb < V; vb += step) {     // workgroup-uniform trip count: the ballots below see whole waves
    const long v = vb + (long)threadIdx.x * VEC;
    const bool in = v < V;                                                // VEC == 4 only with V % 4 == 0: v < V covers v + 3
    float l[VEC][KMAX];
    int t[VEC];
    if (in) {
      if (VEC == 4) {
        const f32x4 q = *reinterpret_cast<const f32x4*>(labels + (long)b * V + v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) t[j] = (int)q[j];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) {
            const f32x4 x = *reinterpret_cast<const f32x4*>(lg + (long)k * V + v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) l[j][k] = x[j];
          }
      } else {
        t[0] = (int)labels[(long)b * V + v];
#pragma unroll
        for (int k = 0; k < KMAX; ++k)
          if (k < K) l[0][k] = lg[(long)k * V + v];
      }
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        t[j] = 0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) l[j][k] = 0.f;
      }
    }
    long long pv[VEC], tv[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const bool lab = t[j] > 0;
      float mx = l[j][0], lt = 0.f;
      int arg = 0;
#pragma unroll
      for (int k = 1; k < KMAX; ++k)
        if (k < K && l[j][k] > mx) { mx = l[j][k]; arg = k; }
      float se = 0.f;
#pragma unroll
      for (int k = 0; k < KMAX; ++k)
        if (k < K) {
          if (k == t[j]) lt = l[j][k];
          l[j][k] = __expf(l[j][k] - mx);
          se += l[j][k];
        }
      const float wt = t[j] < K ? cwsh[t[j] & 31] : 0.f;
      if (in) {
        s_nll += lab ? wt * (mx + __logf(se) - lt) : w0 * logK;
        s_w += lab ? wt : w0;
      }
      const float rs = 1.f / se;
#pragma unroll
      for (int k = 1; k < KMAX; ++k)
        if (k < K) {
          const float p = lab ? l[j][k] * rs : 0.f;      // (a select, not a product: an unlabelled voxel may hold anything)
          sp[k] += p;
          si[k] += k == t[j] ? p : 0.f;
        }
      sem_wave_counts<KMAX>(arg, t[j], lab, K, lane, ci, cp, ct);
      pv[j] = lab ? arg : 0;
      tv[j] = lab ? t[j] : 0;
    }
    if (in) {
      long long* po = pred_vis + (long)b * V + v;
      long long* to = target_vis + (long)b * V + v;
      if (VEC == 4) {
        typedef long long ll2 __attribute__((ext_vector_type(2)));
        reinterpret_cast<ll2*>(po)[0] = ll2{pv[0], pv[1]}; reinterpret_cast<ll2*>(po)[1] = ll2{pv[2], pv[VEC - 1]};
        reinterpret_cast<ll2*>(to)[0] = ll2{tv[0], tv[1]}; reinterpret_cast<ll2*>(to)[1] = ll2{tv[2], tv[VEC - 1]};
      } else {
        po[0] = pv[0]; to[0] = tv[0];
      }
    }
  }
  const int nf = SEM_NF(K);
  s_nll = wave_sum(s_nll); s_w = wave_sum(s_w);
  if (lane == 0) { fsh[wave][0] = s_nll; fsh[wave][1] = s_w; }
#pragma unroll
  for (int k = 1; k < KMAX; ++k)
    if (k < K) {
      const float a = wave_sum(sp[k]), c = wave_sum(si[k]);
      if (lane == 0) { fsh[wave][2 + (k - 1)] = a; fsh[wave][2 + (K - 1) + (k - 1)] = c; }
    }
  const long row = (long)b * gridDim.x + blockIdx.x;
  sem_counts_to_row(wc, K, ci, cp, ct, ipart + row * SEM_NI(K));           // (its barrier also orders fsh)
  if ((int)threadIdx.x < nf) fpart[row * nf + threadIdx.x] = (double)fsh[0][threadIdx.x] + (double)fsh[1][threadIdx.x] + (double)fsh[2][threadIdx.x] + (double)fsh[3][threadIdx.x];
}

// labels only: T = float, int or long long label arrays of n elements; the same counting code, one ipart row per workgroup
template <typename T>
__global__ __launch_bounds__(256) void sem_label_count_kernel(const T* __restrict__ output, const T* __restrict__ target, int K, long n, long long* __restrict__ ipart) {
  __shared__ unsigned long long wc[4][3][32];
  unsigned long long ci = 0, cp = 0, ct = 0;
  const int lane = threadIdx.x & 63;
  for (long vb = (long)blockIdx.x * 256; vb < n; vb += (long)gridDim.x * 256) {
    const long v = vb + threadIdx.x;
    const bool in = v < n;
    const long long t = in ? (long long)target[v] : 0, p = in ? (long long)output[v] : 0;
    const bool lab = t > 0;
    sem_wave_counts<32>((p > 0 && p < K) ? (int)p : 0, (t > 0 && t < K) ? (int)t : 0, lab, K, lane, ci, cp, ct);
  }
  sem_counts_to_row(wc, K, ci, cp, ct, ipart + (long)blockIdx.x * SEM_NI(K));
}

// one column of a slab over rows first, first + stride, ...: 8 independent loads in flight, added in row order (a one-load-per-trip loop waits out the memory
// latency a thousand times over: 50-60 us measured for 1024 rows)
template <typename T>
__device__ __forceinline__ T sem_col_sum(const T* __restrict__ col, int ncols, int nrows, int first, int stride) {
  T s = 0;
  for (int r = first; r < nrows; r += 8 * stride) {
    T v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = r + u * stride < nrows ? col[(long)(r + u * stride) * ncols] : T(0);
#pragma unroll
    for (int u = 0; u < 8; ++u) s += v[u];
  }
  return s;
}
// one workgroup of 1024: rows b * nb .. b * nb + nb - 1 of each slab added in a fixed order (16 resp. 8 interleaved partial sums per column, then those in
// order); out[0] = weighted CE, out[1] = mean over (sample, class >= 1) of inter / (sum m p + T - inter + 1e-8); counts int64 [4][K-1] = {I, U = P + T - I,
// T, P} over the batch; totals (optional) int64 [3][K-1] += {I, U, T}.  fpart == nullptr (labels only): the counts alone.
__global__ __launch_bounds__(1024) void sem_eval_finalize_kernel(const double* __restrict__ fpart, const long long* __restrict__ ipart, int B, int nb, int K,
                                                                 float* __restrict__ out, long long* __restrict__ counts, long long* __restrict__ totals) {
  __shared__ double fs[16][64];
  __shared__ long long is[8][128];
  __shared__ double fres[64];
  __shared__ long long ires[128];
  __shared__ double term[32];
  const int nf = SEM_NF(K), ni = SEM_NI(K), tid = threadIdx.x;
  const int fa = tid & 63, fp = tid >> 6, ia = tid & 127, ip = tid >> 7;
  double f_tot = 0.0, iou_acc = 0.0;     // thread a < 2: the CE sums over the batch; thread k-1 < K-1: the soft-IoU terms of class k over the batch
  long long i_tot = 0;                   // thread a < ni: the batch's count
  for (int b = 0; b < B; ++b) {
    if (fpart && fa < nf) {
      fs[fp][fa] = sem_col_sum(fpart + (long)b * nb * nf + fa, nf, nb, fp, 16);
    }
    if (ia < ni) {
      is[ip][ia] = sem_col_sum(ipart + (long)b * nb * ni + ia, ni, nb, ip, 8);
    }
    __syncthreads();
    if (fpart && tid < nf) {
      double s = 0.0;
      for (int q = 0; q < 16; ++q) s += fs[q][tid];
      fres[tid] = s;
      if (tid < 2) f_tot += s;
    }
    if (tid < ni) {
      long long s = 0;
      for (int q = 0; q < 8; ++q) s += is[q][tid];
      ires[tid] = s;
      i_tot += s;
    }
    __syncthreads();
    if (fpart && tid < K - 1) {
      const double sp = fres[2 + tid], inter = fres[2 + (K - 1) + tid], cnt = (double)ires[2 * (K - 1) + tid];
      iou_acc += inter / (sp + cnt - inter + 1e-8);
    }
    __syncthreads();
  }
  if (fpart) {
    if (tid < 2) fres[tid] = f_tot;
    if (tid < K - 1) term[tid] = iou_acc;
  }
  if (tid < ni) ires[tid] = i_tot;
  __syncthreads();
  if (fpart && tid == 0) {
    out[0] = (float)(fres[0] / fres[1]);
    double acc = 0.0;
    for (int k = 0; k < K - 1; ++k) acc += term[k];
    out[1] = (float)(acc / ((double)B * (K - 1)));
  }
  if (tid < K - 1) {
    const long long I = ires[tid], P = ires[(K - 1) + tid], T = ires[2 * (K - 1) + tid], U = P + T - I;
    counts[tid] = I; counts[(K - 1) + tid] = U; counts[2 * (K - 1) + tid] = T; counts[3 * (K - 1) + tid] = P;
    if (totals) { totals[tid] += I; totals[(K - 1) + tid] += U; totals[2 * (K - 1) + tid] += T; }
  }
}

template <int KMAX>
static void sem_eval_launch(bool vec, unsigned nb, int B, const float* logits, const float* labels, const float* cw, int K, long V, double* fpart, long long* ipart,
                            long long* pred_vis, long long* target_vis, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((sem_eval_kernel<KMAX, 4>), dim3(nb, B), dim3(256), 0, st, logits, labels, cw, K, V, fpart, ipart, pred_vis, target_vis);
  else hipLaunchKernelGGL((sem_eval_kernel<KMAX, 1>), dim3(nb, B), dim3(256), 0, st, logits, labels, cw, K, V, fpart, ipart, pred_vis, target_vis);
}
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
int k_sem_eval(const float* logits, const float* labels, const float* cw, int B, int K, long V, double* fpart, long long* ipart, float* out, long long* counts,
               long long* pred_vis, long long* target_vis, long long* totals, hipStream_t st) {
  if (K < 2 || K > 32 || B < 1 || B > NMH_SEM_EVAL_ROWS || V < 1) return -2;
  // 16-byte loads and stores: every class plane of every sample starts at a multiple of 4 elements
  const bool vec = (V % 4 == 0) && al16(logits) && al16(labels) && al16(pred_vis) && al16(target_vis);
  const long per = 256L * (vec ? 4 : 1), cap = NMH_SEM_EVAL_ROWS / B;     // rows = B * nb <= NMH_SEM_EVAL_ROWS, the extent of the caller's slabs
  long nbl = (V + per - 1) / per;
  const unsigned nb = (unsigned)(nbl > cap ? cap : nbl);
  if (K <= 20) sem_eval_launch<20>(vec, nb, B, logits, labels, cw, K, V, fpart, ipart, pred_vis, target_vis, st);
  else sem_eval_launch<32>(vec, nb, B, logits, labels, cw, K, V, fpart, ipart, pred_vis, target_vis, st);
  hipLaunchKernelGGL(sem_eval_finalize_kernel, dim3(1), dim3(1024), 0, st, (const double*)fpart, (const long long*)ipart, B, (int)nb, K, out, counts, totals);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_sem_label_counts(int dt, const void* output, const void* target, long n, int K, long long* ipart, long long* counts, hipStream_t st) {
  if (K < 2 || K > 32 || n < 0 || dt < 0 || dt > 2) return -2;
  long nbl = (n + 255) / 256;
  const unsigned nb = (unsigned)(nbl > NMH_SEM_EVAL_ROWS ? NMH_SEM_EVAL_ROWS : (nbl < 1 ? 1 : nbl));
  if (dt == 0) hipLaunchKernelGGL(sem_label_count_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)output, (const float*)target, K, n, ipart);
  else if (dt == 1) hipLaunchKernelGGL(sem_label_count_kernel<int>, dim3(nb), dim3(256), 0, st, (const int*)output, (const int*)target, K, n, ipart);
  else hipLaunchKernelGGL(sem_label_count_kernel<long long>, dim3(nb), dim3(256), 0, st, (const long long*)output, (const long long*)target, K, n, ipart);
  hipLaunchKernelGGL(sem_eval_finalize_kernel, dim3(1), dim3(1024), 0, st, (const double*)nullptr, (const long long*)ipart, 1, (int)nb, K, (float*)nullptr, counts, (long long*)nullptr);
  NMH_CHECK_LAUNCH();
  return 0;
}
