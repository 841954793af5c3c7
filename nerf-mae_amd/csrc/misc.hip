// Remaining HBM-bound kernels of the hot path: patch-embed im2row, transpose-conv pixel shuffle (+skip concat),
// fused 1x1 output head + masked MSE loss (forward and backward), bias gradients, weight packing (fp32 master ->
// compute-dtype GEMM operand layouts), and the fused AdamW / grad-clip step.
// Reference semantics: swin_mae3d.py:1120-1129 (patch conv k=s=4), unetr_block.py:150-158,193-200 (ConvTranspose3d k=s,
// cat), unetr_block.py:99-105 + swin_mae3d.py:1513-1549 (head + loss), run_swin_mae3d.py:588-598,665-669 (AdamW, clip).
#include "common.hpp"
#include "kernels.hpp"
#include "../../include/nerfmae_hip.h"   // NMH_ADAMW_MAX_RANGES
#include <cmath>
#include <mutex>

static inline unsigned ew_blocks(long total, int cap = 16384) { long nb = (total + 255) / 256; return (unsigned)(nb > cap ? cap : (nb < 1 ? 1 : nb)); }

// ---- patch embed im2row: A[(b,z,y,x)][ci*64 + kz*16+ky*4+kx] = x[b][ci][4z+kz][4y+ky][4x+kx] ---------------------
// One block per x-line of tokens (b, tz, ty): its 64 source rows (ci, kz, ky) are read as contiguous runs of R floats and staged in LDS as
// [token][256] (token stride padded by 8 bytes: the 8-byte LDS writes of 32 consecutive tokens land in distinct banks); the g token rows are
// then one contiguous run of g*256 elements in A.  (One float4 per lane straight from the 64 rows touched 64 cache lines per wave-load.)
template <typename T> __global__ __launch_bounds__(256) void embed_gather_kernel(const float* __restrict__ x, T* __restrict__ A, int B, int R) {
  extern __shared__ __attribute__((aligned(16))) char esm[];
  const int g = R >> 2;
  constexpr int ROWB = 256 * (int)sizeof(T) + 8;   // bytes per staged token row
  const int line = blockIdx.x;                      // (b, tz, ty)
  const int ty = line % g, tz = (line / g) % g, b = line / (g * g);
  for (int idx = threadIdx.x; idx < 64 * g; idx += 256) {
    const int q = idx / g, tx = idx - q * g;
    const int ci = q >> 4, kz = (q >> 2) & 3, ky = q & 3;
    const float4 v = *reinterpret_cast<const float4*>(x + ((((long)b * 4 + ci) * R + 4 * tz + kz) * R + 4 * ty + ky) * (long)R + 4 * tx);
    T* o = reinterpret_cast<T*>(esm + tx * ROWB) + q * 4;
    o[0] = from_f<T>(v.x); o[1] = from_f<T>(v.y); o[2] = from_f<T>(v.z); o[3] = from_f<T>(v.w);
  }
  __syncthreads();
  constexpr int V8 = 256 * (int)sizeof(T) / 8;      // 8-byte pieces per token row
  unsigned long long* out = reinterpret_cast<unsigned long long*>(A + (long)line * g * 256);
  for (int idx = threadIdx.x; idx < g * V8; idx += 256) {
    const int tx = idx / V8, c = idx - tx * V8;
    out[idx] = *reinterpret_cast<const unsigned long long*>(esm + tx * ROWB + c * 8);
  }
}
// The KEPT tokens only (k_mask_rowmap), into the compact rows [b][rowmap[token]] of A [B][cap][256]: a removed token costs neither its 64 x 16 source bytes nor
// its row (its embedding is replaced by the mask token, swin_mae3d.py:1375-1380).  One WAVE per run of four tokens along x: lane q = (ci, kz, ky) reads the run's
// 64 contiguous source bytes of its row -- 16 per kept token -- and writes elements 4 q .. 4 q + 3 of each kept token's row: the 64 lanes complete the row (no LDS,
// no barrier; the line-per-block kernel above was latency-bound once three quarters of its work were gone).  Every block also zeroes its share of the rows behind
// the kept count, which stay operands of the GEMM and of the weight gradient.
template <typename T> __global__ __launch_bounds__(256) void embed_gather_kept_kernel(const float* __restrict__ x, T* __restrict__ A, int B, int R, const int* __restrict__ rowmap, long cap) {
  const int g = R >> 2, runs = (g + 3) >> 2, n = g * g * g;
  const int q = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long nrun = (long)B * g * g * runs;
  constexpr int V8 = 256 * (int)sizeof(T) / 8;
  for (long u = (long)blockIdx.x * 4 + wave; u < nrun; u += (long)gridDim.x * 4) {
    const int rx = (int)(u % runs);
    const long l = u / runs;
    const int ty = (int)(l % g), tz = (int)((l / g) % g), b = (int)(l / ((long)g * g));
    const int t0 = (tz * g + ty) * g + 4 * rx;
    int r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = 4 * rx + j < g ? rowmap[t0 + j] : -1;
    if ((r[0] & r[1] & r[2] & r[3]) < 0 && r[0] < 0 && r[1] < 0 && r[2] < 0 && r[3] < 0) continue;
    const int ci = q >> 4, kz = (q >> 2) & 3, ky = q & 3;
    const float* src = x + ((((long)b * 4 + ci) * R + 4 * tz + kz) * R + 4 * ty + ky) * (long)R + 16 * rx;
    float4 v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) if (r[j] >= 0) v[j] = *reinterpret_cast<const float4*>(src + 4 * j);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (r[j] >= 0) {
        T* o = A + ((long)b * cap + r[j]) * 256 + q * 4;
        if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(o) = make_uint2(pk_bf16(v[j].x, v[j].y), pk_bf16(v[j].z, v[j].w));
        else *reinterpret_cast<float4*>(o) = v[j];
      }
  }
  const int K = rowmap[n];
  const long tail = cap - K;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < (long)B * tail * V8; i += (long)gridDim.x * 256) {
    const long rr = i / V8, c = i - rr * V8, b = rr / tail;
    reinterpret_cast<unsigned long long*>(A + (b * cap + K + (rr - b * tail)) * 256)[c] = 0ull;
  }
}
int k_embed_gather(int dt, const float* x, void* A, int B, int R, hipStream_t st, const int* rowmap, long cap_rows) {
  const int g = R / 4;
  if (R % 4 || g <= 0 || (rowmap && cap_rows <= 0)) return -2;
  if (rowmap) {
    const long nrun = (long)B * g * g * ((g + 3) / 4);
    long nb = (nrun + 3) / 4;
    if (nb > 65536) nb = 65536;
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(embed_gather_kept_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, x, (bf16_t*)A, B, R, rowmap, cap_rows);
    else hipLaunchKernelGGL(embed_gather_kept_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, x, (float*)A, B, R, rowmap, cap_rows);
    NMH_CHECK_LAUNCH();
    return 0;
  }
  const long lines = (long)B * g * g;
  const size_t lds = (size_t)g * (256 * (dt == NMH_DT_BF16 ? 2 : 4) + 8);
  if (lds > 160 * 1024) return -2;
  if (dt == NMH_DT_BF16) {
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)embed_gather_kernel<bf16_t>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(embed_gather_kernel<bf16_t>, dim3((unsigned)lines), dim3(256), lds, st, x, (bf16_t*)A, B, R);
  } else {
    if (lds > 64 * 1024) hipFuncSetAttribute((const void*)embed_gather_kernel<float>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(embed_gather_kernel<float>, dim3((unsigned)lines), dim3(256), lds, st, x, (float*)A, B, R);
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- compact rows of the kept tokens: rowmap[t] = number of kept tokens in front of token t (raster order), -1 for a removed one -------------------------
// One workgroup; thread i owns the tokens [i per, (i + 1) per).  rowmap[n] = kept count (clamped to cap), rowmap[n + 1] = 1 if kept tokens did not fit (their
// rows read -1: memory-safe, and the host -- which drew the mask -- never lets that happen).
__global__ __launch_bounds__(1024) void mask_rowmap_kernel(const unsigned char* __restrict__ mask, int n, int cap, int* __restrict__ rowmap) {
  // wave w owns the contiguous tokens [w seg, (w + 1) seg), seg a multiple of 1024; per step a lane reads 16 consecutive mask bytes (one 16-byte load; the steps'
  // loads are all in flight at once -- a serial per-token loop took 94 us for 64000 tokens, mostly load latency), counts its kept tokens and takes its place by a
  // scan over the wave.  Segments longer than 8 steps (n > 131072) repeat the sweep.
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int seg = ((n + 16 * 1024 - 1) / (16 * 1024)) * 1024, nstep = seg / 1024, t0 = wave * seg;
  const bool vec = (reinterpret_cast<uintptr_t>(mask) & 15) == 0;
  auto load16 = [&](int t) -> unsigned {   // bit j = token t + j is kept
    unsigned bits = 0;
    if (vec && t + 16 <= n) {
      const uint4 m = *reinterpret_cast<const uint4*>(mask + t);
      const unsigned w[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
      for (int j = 0; j < 16; ++j) bits |= (((w[j >> 2] >> (8 * (j & 3))) & 255u) == 0u ? 1u : 0u) << j;
    } else {
      for (int j = 0; j < 16; ++j) if (t + j < n && mask[t + j] == 0) bits |= 1u << j;
    }
    return bits;
  };
  int cnt = 0;
  for (int s0 = 0; s0 < nstep; ++s0) cnt += __popc(load16(t0 + s0 * 1024 + lane * 16));
  int wtot = cnt;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wtot += __shfl_xor(wtot, o, 64);
  if (lane == 0) wsum[wave] = wtot;
  __syncthreads();
  int pos = 0, tot = 0;
  for (int w = 0; w < 16; ++w) { if (w < wave) pos += wsum[w]; tot += wsum[w]; }
  for (int s0 = 0; s0 < nstep; ++s0) {
    const int t = t0 + s0 * 1024 + lane * 16;
    const unsigned bits = load16(t);
    const int c = __popc(bits);
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
    int r = pos + inc - c;
    for (int j = 0; j < 16; ++j)
      if (t + j < n) { const bool k = (bits >> j) & 1u; rowmap[t + j] = (k && r < cap) ? r : -1; r += k; }
    pos += __shfl(inc, 63, 64);
  }
  if (tid == 0) { rowmap[n] = tot < cap ? tot : cap; rowmap[n + 1] = tot > cap ? 1 : 0; }
}
int k_mask_rowmap(const unsigned char* mask, int n, int cap, int* rowmap, hipStream_t st) {
  if (n <= 0 || cap <= 0) return -2;
  hipLaunchKernelGGL(mask_rowmap_kernel, dim3(1), dim3(1024), 0, st, mask, n, cap, rowmap);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- transpose conv (k = stride) pixel shuffle: out[(b,Z,Y,X)][0:Cout] = upre[(b,Z/k,Y/k,X/k)][tap*Cout + c] + bias[c];
//      out[..][Cout:2Cout] = skip[..]          tap = (Z%k)*k*k + (Y%k)*k + X%k --------------------------------------------
template <typename T> __global__ void up_cat_fwd_kernel(const T* upre, const float* bias, const T* skip, T* out, int B, int v, int k, int Cout) {
  const int V = v * k, Cc = skip ? 2 * Cout : Cout, nch = Cc >> 3, uch = Cout >> 3;
  const unsigned total = (unsigned)V * V * V * nch, Vu = (unsigned)V, ku = (unsigned)k;
  const long b = blockIdx.y, boff = b * ((long)V * V * V);
  for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const unsigned voxl = i / (unsigned)nch;
    const int c = (int)(i - voxl * nch);
    const long vox = boff + voxl;
    float a[8];
    if (c < uch) {
      const unsigned t1 = voxl / Vu, X = voxl - t1 * Vu, Z = t1 / Vu, Y = t1 - Z * Vu;
      const unsigned zq = Z / ku, yq = Y / ku, xq = X / ku;
      const int tap = (int)(((Z - zq * ku) * ku + (Y - yq * ku)) * ku + (X - xq * ku));
      const long m = ((b * v + zq) * v + yq) * v + xq;
      Vec8<T>::load(upre + m * ((long)k * k * k * Cout) + (long)tap * Cout + c * 8, a);
#pragma unroll
      for (int j = 0; j < 8; ++j) a[j] += bias[c * 8 + j];
    } else {
      Vec8<T>::load(skip + vox * Cout + (c - uch) * 8, a);
    }
    Vec8<T>::store(out + vox * Cc + c * 8, a);
  }
}
template <typename T> __global__ void up_cat_bwd_kernel(const T* dcat, T* dupre, T* dskip, float* dbias, int B, int v, int k, int Cout, int has_skip) {
  extern __shared__ float sdb[];
  const int V = v * k, Cc = has_skip ? 2 * Cout : Cout, nch = Cc >> 3, uch = Cout >> 3;
  const unsigned total = (unsigned)V * V * V * nch, Vu = (unsigned)V, ku = (unsigned)k;
  const long b = blockIdx.y, boff = b * ((long)V * V * V);
  for (int i = threadIdx.x; i < Cout; i += blockDim.x) sdb[i] = 0.f;
  __syncthreads();
  // fixed channel chunk per thread (stride is a multiple of nch) so bias partials stay in registers
  const unsigned stride = (gridDim.x * blockDim.x / nch) * nch;
  float pb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) pb[j] = 0.f;
  const unsigned start = blockIdx.x * blockDim.x + threadIdx.x;
  const int c = (int)(start % nch);
  if (start < stride) {
    for (unsigned i = start; i < total; i += stride) {
      const unsigned voxl = i / (unsigned)nch;
      const long vox = boff + voxl;
      float a[8];
      Vec8<T>::load(dcat + vox * Cc + c * 8, a);
      if (c < uch) {
        const unsigned t1 = voxl / Vu, X = voxl - t1 * Vu, Z = t1 / Vu, Y = t1 - Z * Vu;
        const unsigned zq = Z / ku, yq = Y / ku, xq = X / ku;
        const int tap = (int)(((Z - zq * ku) * ku + (Y - yq * ku)) * ku + (X - xq * ku));
        const long m = ((b * v + zq) * v + yq) * v + xq;
        Vec8<T>::store(dupre + m * ((long)k * k * k * Cout) + (long)tap * Cout + c * 8, a);
#pragma unroll
        for (int j = 0; j < 8; ++j) pb[j] += a[j];
      } else {
        Vec8<T>::store(dskip + vox * Cout + (c - uch) * 8, a);
      }
    }
    if (c < uch)
#pragma unroll
      for (int j = 0; j < 8; ++j) atomicAdd(&sdb[c * 8 + j], pb[j]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < Cout; i += blockDim.x) atomicAdd(dbias + i, sdb[i]);
}
int k_up_cat_fwd(int dt, const void* upre, const float* bias, const void* skip, void* out, int B, int v, int k, int Cout, hipStream_t st) {
  if (Cout % 8) return -2;
  long V = (long)v * k;
  long total = V * V * V * ((skip ? 2 : 1) * Cout / 8);
  dim3 grid(ew_blocks(total, 4096), B);
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(up_cat_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)upre, bias, (const bf16_t*)skip, (bf16_t*)out, B, v, k, Cout);
  else hipLaunchKernelGGL(up_cat_fwd_kernel<float>, grid, dim3(256), 0, st, (const float*)upre, bias, (const float*)skip, (float*)out, B, v, k, Cout);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_up_cat_bwd(int dt, const void* dcat, void* dupre, void* dskip, float* dbias, int B, int v, int k, int Cout, int has_skip, hipStream_t st) {
  if (Cout % 8) return -2;
  long V = (long)v * k;
  int nch = (has_skip ? 2 : 1) * Cout / 8;
  long total = V * V * V * nch;
  unsigned nb = ew_blocks(total, 1024);
  if ((long)nb * 256 < nch) nb = (unsigned)((nch + 255) / 256);
  size_t lds = Cout * sizeof(float);
  dim3 grid(nb, B);
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(up_cat_bwd_kernel<bf16_t>, grid, dim3(256), lds, st, (const bf16_t*)dcat, (bf16_t*)dupre, (bf16_t*)dskip, dbias, B, v, k, Cout, has_skip);
  else hipLaunchKernelGGL(up_cat_bwd_kernel<float>, grid, dim3(256), lds, st, (const float*)dcat, (float*)dupre, (float*)dskip, dbias, B, v, k, Cout, has_skip);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- fused 1x1 head (Cd -> 4) + masked MSE loss ------------------------------------------------------------------------
// loss_rgb = sum_{rgb}(p-t)^2 [t_a>0.01] / #{t_a>0.01};  loss_a = sum (sigmoid(p_a)-t_a)^2 [valid & removed] / #{valid & removed}
__device__ __forceinline__ float block_sum_to(float v, float* sh, int slot) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) atomicAdd(&sh[slot], v);
  return v;
}
// One 256-thread block walks 256-voxel tiles of one sample:
//   1. the d0 tile (256 x Cd) is copied to LDS with coalesced 16-B loads;
//   2. thread-per-voxel: 1x1 head from the LDS row, target/mask lookups (coalesced plane reads), loss terms or d(pred);
//   3. (backward) thread = (8-channel chunk, voxel lane): d(d0) chunk written with coalesced 16-B stores and the head weight
//      gradient dW[o][c] += d(pred)[o] * d0[c] accumulated in 32 registers -> LDS -> one set of fp32 atomics per block.
template <typename T, int BWD>
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a, T* dd0, float* dWout, float* dbout) {
  extern __shared__ __attribute__((aligned(16))) char lsm[];
  const int R = a.R, Cd = a.Cd, g = R >> 2, CL = Cd >> 3, NV = 256 / CL;
  const int rowb = Cd * (int)sizeof(T);
  char* tile = lsm;                                               // [256][Cd] T
  float* dps = reinterpret_cast<float*>(lsm + 256 * rowb);        // [256][4]
  float* sacc = dps + 256 * 4;                                    // [4*Cd + 8]
  const int tid = threadIdx.x;
  const long V = (long)R * R * R, b = blockIdx.y;
  const unsigned Vu = (unsigned)V, Ru = (unsigned)R;
  const T* d0 = (const T*)a.d0 + b * V * Cd;
  for (int i = tid; i < 4 * Cd + 8; i += 256) sacc[i] = 0.f;
  float acc[4] = {0.f, 0.f, 0.f, 0.f}, dpa[4] = {0.f, 0.f, 0.f, 0.f};
  float inv_occ = 0.f, inv_rm = 0.f;
  if (BWD) { inv_occ = (float)(1.0 / a.sums[1]); inv_rm = (float)(1.0 / a.sums[3]); }
  const int cl = tid % CL, vl = tid / CL;  // phase-3 role
  float wreg[4][8], wacc[4][8];
  if (BWD) {
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int j = 0; j < 8; ++j) { wreg[o][j] = a.Wout[o * Cd + cl * 8 + j]; wacc[o][j] = 0.f; }
  }
  const int cpr = rowb / 16;  // 16-B chunks per row
  const unsigned ntile = (Vu + 255) / 256;
  for (unsigned vt = blockIdx.x; vt < ntile; vt += gridDim.x) {
    const unsigned v0 = vt * 256;
    const int nvox = (Vu - v0) < 256u ? (int)(Vu - v0) : 256;
    __syncthreads();
    const char* src = reinterpret_cast<const char*>(d0 + (long)v0 * Cd);
    for (int c = tid; c < nvox * cpr; c += 256) *reinterpret_cast<uint4*>(tile + c * 16) = *reinterpret_cast<const uint4*>(src + (long)c * 16);
    __syncthreads();
    if (tid < nvox) {
      const unsigned vox = v0 + tid;
      const unsigned t = vox / Ru;
      const int x = (int)(vox - t * Ru);
      const unsigned zq = t / Ru;
      const int y = (int)(t - zq * Ru), z = (int)zq;
      float p[4] = {a.bout[0], a.bout[1], a.bout[2], a.bout[3]};
      const T* row = reinterpret_cast<const T*>(tile + tid * rowb);
      for (int c = 0; c < Cd; c += 8) {
        float v[8];
        Vec8<T>::load(row + c, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          p[0] += v[j] * a.Wout[c + j]; p[1] += v[j] * a.Wout[Cd + c + j];
          p[2] += v[j] * a.Wout[2 * Cd + c + j]; p[3] += v[j] * a.Wout[3 * Cd + c + j];
        }
      }
      const float* tg = a.target + b * 4 * V + vox;
      const float t0 = tg[0], t1 = tg[V], t2 = tg[2 * V], t3 = tg[3 * V];
      const bool occ = t3 > 0.01f;
      const bool valid = z < a.extents[b * 3] && y < a.extents[b * 3 + 1] && x < a.extents[b * 3 + 2];
      const bool rm = valid && a.tokmask[((z >> 2) * g + (y >> 2)) * g + (x >> 2)] != 0;
      const float sg = 1.0f / (1.0f + __expf(-p[3]));
      if (!BWD) {
        if (occ) { acc[0] += (p[0] - t0) * (p[0] - t0) + (p[1] - t1) * (p[1] - t1) + (p[2] - t2) * (p[2] - t2); acc[1] += 1.f; }
        if (rm) { acc[2] += (sg - t3) * (sg - t3); acc[3] += 1.f; }
        if (a.pred) { float* pr = a.pred + b * 4 * V + vox; pr[0] = p[0]; pr[V] = p[1]; pr[2 * V] = p[2]; pr[3 * V] = p[3]; }
        if (a.dp) {  // un-normalised d(loss)/d(pred): the 1/n_occ, 1/n_removed factors are only known once this kernel has finished
          float4 d;
          d.x = occ ? 2.f * (p[0] - t0) : 0.f; d.y = occ ? 2.f * (p[1] - t1) : 0.f; d.z = occ ? 2.f * (p[2] - t2) : 0.f;
          d.w = rm ? 2.f * (sg - t3) * sg * (1.f - sg) : 0.f;
          *reinterpret_cast<float4*>(a.dp + (b * V + vox) * 4) = d;
          dpa[0] += d.x; dpa[1] += d.y; dpa[2] += d.z; dpa[3] += d.w;
        }
      } else {
        float dp[4];
        dp[0] = occ ? 2.f * (p[0] - t0) * inv_occ : 0.f;
        dp[1] = occ ? 2.f * (p[1] - t1) * inv_occ : 0.f;
        dp[2] = occ ? 2.f * (p[2] - t2) * inv_occ : 0.f;
        dp[3] = rm ? 2.f * (sg - t3) * sg * (1.f - sg) * inv_rm : 0.f;
#pragma unroll
        for (int o = 0; o < 4; ++o) { acc[o] += dp[o]; dps[tid * 4 + o] = dp[o]; }
      }
    }
    if (BWD) {
      __syncthreads();
      if (vl < NV) {
        for (int vv = vl; vv < nvox; vv += NV) {
          const float4 dp = *reinterpret_cast<const float4*>(dps + vv * 4);
          float o8[8], d8[8];
          Vec8<T>::load(reinterpret_cast<const T*>(tile + vv * rowb) + cl * 8, o8);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            d8[j] = dp.x * wreg[0][j] + dp.y * wreg[1][j] + dp.z * wreg[2][j] + dp.w * wreg[3][j];
            wacc[0][j] += dp.x * o8[j]; wacc[1][j] += dp.y * o8[j]; wacc[2][j] += dp.z * o8[j]; wacc[3][j] += dp.w * o8[j];
          }
          Vec8<T>::store(dd0 + (b * V + v0 + vv) * Cd + cl * 8, d8);
        }
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int o = 0; o < 4; ++o) block_sum_to(acc[o], sacc, 4 * Cd + o);
  if (!BWD && a.dp) {
#pragma unroll
    for (int o = 0; o < 4; ++o) block_sum_to(dpa[o], sacc, 4 * Cd + 4 + o);
  }
  if (BWD && vl < NV) {
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int j = 0; j < 8; ++j) atomicAdd(&sacc[o * Cd + cl * 8 + j], wacc[o][j]);
  }
  __syncthreads();
  if (tid < 4) {
    if (!BWD) { atomicAdd(&a.sums[tid], (double)sacc[4 * Cd + tid]); if (a.dp) atomicAdd(&a.sums[4 + tid], (double)sacc[4 * Cd + 4 + tid]); }
    else atomicAdd(&dbout[tid], sacc[4 * Cd + tid]);
  }
  if (BWD)
    for (int i = tid; i < 4 * Cd; i += 256) atomicAdd(&dWout[i], sacc[i]);
}
static inline size_t loss_lds(const LossArgs& a) {
  size_t es = a.dt == NMH_DT_BF16 ? 2 : 4;
  return 256 * a.Cd * es + 256 * 4 * sizeof(float) + (4 * a.Cd + 8) * sizeof(float);
}
int k_loss_fwd(const LossArgs& a, hipStream_t st) {
  if (a.Cd % 8 || a.Cd > 64) return -2;
  hipError_t e = nmh_zero_async(a.sums, (a.dp ? 8 : 4) * sizeof(double), st);
  if (e != hipSuccess) return (int)e;
  long ntile = ((long)a.R * a.R * a.R + 255) / 256;
  dim3 grid((unsigned)(ntile < 2048 ? ntile : 2048), a.B);
  if (a.dt == NMH_DT_BF16) hipLaunchKernelGGL((loss_kernel<bf16_t, 0>), grid, dim3(256), loss_lds(a), st, a, nullptr, nullptr, nullptr);
  else hipLaunchKernelGGL((loss_kernel<float, 0>), grid, dim3(256), loss_lds(a), st, a, nullptr, nullptr, nullptr);
  NMH_CHECK_LAUNCH();
  return 0;
}
__global__ void loss_finalize_kernel(const double* s, float* l) {
  double lr = s[0] / s[1], la = s[2] / s[3];
  l[0] = (float)(lr + la); l[1] = (float)lr; l[2] = (float)la;
}
int k_loss_finalize(const double* sums, float* losses, hipStream_t st) {
  hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(1), 0, st, sums, losses);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_loss_bwd(const LossArgs& a, void* dd0, float* dWout, float* dbout, hipStream_t st) {
  if (a.Cd % 8 || a.Cd > 64) return -2;
  long ntile = ((long)a.R * a.R * a.R + 255) / 256;
  dim3 grid((unsigned)(ntile < 1024 ? ntile : 1024), a.B);
  if (a.dt == NMH_DT_BF16) hipLaunchKernelGGL((loss_kernel<bf16_t, 1>), grid, dim3(256), loss_lds(a), st, a, (bf16_t*)dd0, dWout, dbout);
  else hipLaunchKernelGGL((loss_kernel<float, 1>), grid, dim3(256), loss_lds(a), st, a, (float*)dd0, dWout, dbout);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- column sums of dY (bias gradients) ------------------------------------------------------------------------------------
template <typename T> __global__ __launch_bounds__(256) void bias_grad_kernel(const T* dY, float* db, long M, int N, const float* rs, int rps) {
  extern __shared__ float sdb[];
  const int nch = N >> 3, NV = 256 / nch;
  const int c = threadIdx.x % nch, vl = threadIdx.x / nch;
  for (int i = threadIdx.x; i < N; i += 256) sdb[i] = 0.f;
  __syncthreads();
  if (vl < NV) {
    float p[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = 0.f;
    for (long m = (long)blockIdx.x * NV + vl; m < M; m += (long)gridDim.x * NV) {
      float v[8];
      Vec8<T>::load(dY + m * N + c * 8, v);
      const float s = rs ? rs[m / rps] : 1.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) p[j] += v[j] * s;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) atomicAdd(&sdb[c * 8 + j], p[j]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += 256) atomicAdd(db + i, sdb[i]);
}
template <typename T> __global__ __launch_bounds__(256) void bias_grad_wide_kernel(const T* dY, float* db, long M, int N, const float* rs, int rps) {
  // N/8 > 256: one thread per 8-column chunk, blockIdx.y strides rows
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c * 8 >= N) return;
  float p[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = 0.f;
  for (long m = blockIdx.y; m < M; m += gridDim.y) {
    float v[8];
    Vec8<T>::load(dY + m * N + c * 8, v);
    const float s = rs ? rs[m / rps] : 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] += v[j] * s;
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) atomicAdd(db + c * 8 + j, p[j]);
}
int k_bias_grad(int dt, const void* dY, float* db, long M, int N, const float* rs, int rps, hipStream_t st) {
  if (N % 8) return -2;
  if (N / 8 <= 256) {
    int NV = 256 / (N / 8);
    long nb = (M + (long)NV * 32 - 1) / ((long)NV * 32);  // >= 32 rows per thread before the block touches its N atomics
    if (nb > 512) nb = 512;
    if (nb < 1) nb = 1;
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(bias_grad_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), N * sizeof(float), st, (const bf16_t*)dY, db, M, N, rs, rps);
    else hipLaunchKernelGGL(bias_grad_kernel<float>, dim3((unsigned)nb), dim3(256), N * sizeof(float), st, (const float*)dY, db, M, N, rs, rps);
  } else {
    dim3 grid((N / 8 + 255) / 256, (unsigned)(M < 256 ? M : 256));
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(bias_grad_wide_kernel<bf16_t>, grid, dim3(256), 0, st, (const bf16_t*)dY, db, M, N, rs, rps);
    else hipLaunchKernelGGL(bias_grad_wide_kernel<float>, grid, dim3(256), 0, st, (const float*)dY, db, M, N, rs, rps);
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

template <typename T> __global__ void add_kernel(T* out, const T* a, const T* b, long n8) {   // out may alias a
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float x[8], y[8];
    Vec8<T>::load(a + i * 8, x);
    Vec8<T>::load(b + i * 8, y);
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] += y[j];
    Vec8<T>::store(out + i * 8, x);
  }
}
int k_add(int dt, void* out, const void* a, const void* b, long n, hipStream_t st) {
  if (n % 8) return -2;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(add_kernel<bf16_t>, dim3(ew_blocks(n / 8)), dim3(256), 0, st, (bf16_t*)out, (const bf16_t*)a, (const bf16_t*)b, n / 8);
  else hipLaunchKernelGGL(add_kernel<float>, dim3(ew_blocks(n / 8)), dim3(256), 0, st, (float*)out, (const float*)a, (const float*)b, n / 8);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_add_inplace(int dt, void* a, const void* b, long n, hipStream_t st) { return k_add(dt, a, a, b, n, st); }
// Per-step host parameters without host-to-device copies: the block mask (one bit per 4x4x4-token block, drawn on the host with the
// reference's python RNG), the optimizer hyper-parameters and the valid extents travel as KERNEL ARGUMENTS of one tiny launch that
// expands / stores them into their device buffers.  (Small hipMemcpyAsync uploads were measured to block the calling thread until the
// stream had drained -- the host could never queue the next step behind the running one.)
struct StepParams {
  unsigned bits[128];      // block (a,b,c) of an nb^3 raster, bit index (a*nb+b)*nb+c; 1 = removed
  float hyper[8];
  int ext[48];
  int nb, g, n_ext, has_hyper;
};
__global__ void step_params_kernel(StepParams p, unsigned char* __restrict__ tokmask, float* __restrict__ hyper, int* __restrict__ ext) {
  const int g = p.g, n = g * g * g;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int c = i % g, b = (i / g) % g, a = i / (g * g);
    const int ba = a >> 2, bb = b >> 2, bc = c >> 2;
    unsigned char m = 0;
    if (ba < p.nb && bb < p.nb && bc < p.nb) {
      const int bit = (ba * p.nb + bb) * p.nb + bc;
      m = (p.bits[bit >> 5] >> (bit & 31)) & 1u;
    }
    tokmask[i] = m;
  }
  if (blockIdx.x == 0) {
    if (p.has_hyper && hyper && threadIdx.x < 8) hyper[threadIdx.x] = p.hyper[threadIdx.x];
    if (ext && (int)threadIdx.x < p.n_ext) ext[threadIdx.x] = p.ext[threadIdx.x];
  }
}
int k_step_params(const unsigned* bits, int nb, int g, unsigned char* tokmask, const float* hyper_host, float* hyper_dev, const int* ext_host, int n_ext, int* ext_dev,
                  hipStream_t st) {
  if (nb < 0 || nb * nb * nb > 128 * 32 || n_ext < 0 || n_ext > 48 || (tokmask && g <= 0)) return -4;
  StepParams p{};
  const int nbits = nb * nb * nb;
  for (int i = 0; i < (nbits + 31) / 32; ++i) p.bits[i] = bits ? bits[i] : 0u;
  if (hyper_host) for (int i = 0; i < 8; ++i) p.hyper[i] = hyper_host[i];
  for (int i = 0; i < n_ext; ++i) p.ext[i] = ext_host[i];
  p.nb = nb; p.g = g; p.n_ext = ext_host ? n_ext : 0; p.has_hyper = hyper_host != nullptr;
  const int n = tokmask ? g * g * g : 0;
  p.g = tokmask ? g : 0;
  hipLaunchKernelGGL(step_params_kernel, dim3(n ? (n + 255) / 256 : 1), dim3(256), 0, st, p, tokmask, hyper_dev, ext_dev);
  NMH_CHECK_LAUNCH();
  return 0;
}

// gradient buckets for the data-parallel exchange: fp32 flat gradient segment -> bf16 staging (and back, optionally scaled), 8 elements per thread
__global__ void grad_f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, long n8) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float v[8];
    Vec8<float>::load(src + i * 8, v);
    Vec8<bf16_t>::store(dst + i * 8, v);
  }
}
__global__ void grad_bf16_to_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, long n8, float scale) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long)gridDim.x * blockDim.x) {
    float v[8];
    Vec8<bf16_t>::load(src + i * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= scale;
    Vec8<float>::store(dst + i * 8, v);
  }
}
int k_grad_cast(int to_bf16, const void* src, void* dst, long n, float scale, hipStream_t st) {
  if (n % 8 || ((uintptr_t)src | (uintptr_t)dst) & 15) return -2;
  if (to_bf16) hipLaunchKernelGGL(grad_f32_to_bf16_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0, st, (const float*)src, (bf16_t*)dst, n / 8);
  else hipLaunchKernelGGL(grad_bf16_to_f32_kernel, dim3(ew_blocks(n / 8)), dim3(256), 0, st, (const bf16_t*)src, (float*)dst, n / 8, scale);
  NMH_CHECK_LAUNCH();
  return 0;
}
__global__ void fill_kernel(float* p, float v, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) p[i] = v;
}
int k_fill_f32(float* p, float v, long n, hipStream_t st) {
  hipLaunchKernelGGL(fill_kernel, dim3(ew_blocks(n)), dim3(256), 0, st, p, v, n);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- weight packing: fp32 master parameters -> compute-dtype GEMM operand layouts, all tensors in ONE launch ------------
//  mode 0 cast           dst[i] = src[i]
//  mode 1 transpose 2-D  src [d0][d1] -> dst [d1][d0]
//  mode 2 conv3 fwd      src [Co=d0][Ci=d1][27] -> dst [Co][27][Ci]
//  mode 3 conv3 dgrad    dst [Ci][27][Co], tap flipped (26 - t)
//  mode 4 convT fwd      src [Ci=d0][Co=d1][k3=d2] -> dst [(t*Co+co)][ci]
//  mode 5 convT dgrad    dst [ci][(t*Co+co)]
//  mode 8/9 conv64 fragment order (conv64.hip), see pack_src_index
//  mode 10/11 zero-padded rows / transposed with zero-padded columns (head weights, N padded to 8); mode 12 conv weights with Cin padded to 8
//  mode 6/7 conv48 fragment order (conv48.hip): dst [step 41][ntile 3][lane 64][8] from the mode-2 (fwd) / mode-3 (dgrad) view
//           W'[n][tap][k]: lane (li, g) of co-tile nt holds n = 12*(li>>2) + 4*nt + (li&3), slot j; steps < 36: tap-row r = 4*(s/18)+g, vector c = s%18; steps >= 36: row 8,
//           c = 4*(s-36)+g (c >= 18 -> zero padding)
// (32-bit index math: every packed tensor has < 2^31 elements; 64-bit div/mod is ~10x the instructions)
__device__ __forceinline__ long pack_src_index(const PackDesc& d, long il) {
  const unsigned i = (unsigned)il, d0 = (unsigned)d.d0, d1 = (unsigned)d.d1, d2 = (unsigned)d.d2;
  switch (d.mode) {
    case 1: { unsigned c = i / d0, r = i - c * d0; return (long)(r * d1 + c); }
    case 2: { unsigned t2 = i / d1, ci = i - t2 * d1, co = t2 / 27u, t = t2 - co * 27u; return (long)((co * d1 + ci) * 27u + t); }
    case 3: { unsigned t2 = i / d0, co = i - t2 * d0, ci = t2 / 27u, t = t2 - ci * 27u; return (long)((co * d1 + ci) * 27u + (26u - t)); }
    case 4: { unsigned t2 = i / d0, ci = i - t2 * d0, t = t2 / d1, co = t2 - t * d1; return (long)((ci * d1 + co) * d2 + t); }
    case 5: { unsigned n = d1 * d2, ci = i / n, r = i - ci * n, t = r / d1, co = r - t * d1; return (long)((ci * d1 + co) * d2 + t); }
    case 6: case 7: {
      // one 41 x 3 x 64 x 8 image per (output block ob, contraction block kb) of W'[n][tap][k], ob-major; Co = Ci = 48: a single image
      constexpr unsigned IMG = 41u * 3u * 512u;
      const unsigned blk = i / IMG, iw = i - blk * IMG;
      const unsigned nkb = (d.mode == 6 ? d1 : d0) / 48u, ob = blk / nkb, kb = blk - ob * nkb;
      const int j = (int)(iw & 7), lane = (int)((iw >> 3) & 63);
      const unsigned sn = iw >> 9;
      // MFMA row li of co-tile nt carries channel 12*(li>>2) + 4*nt + (li&3): an accumulator lane then owns 12 CONSECUTIVE channels of
      // its voxel across the three co-tiles (24-byte runs in the epilogue instead of three 8-byte pieces)
      const int nt = (int)(sn % 3), st = (int)(sn / 3), g = lane >> 4, li = lane & 15, n = (int)ob * 48 + 12 * (li >> 2) + 4 * nt + (li & 3);
      int r, c;
      if (st < 36) { r = 4 * (st / 18) + g; c = st % 18; } else { r = 8; c = 4 * (st - 36) + g; }
      if (c >= 18) return -1;
      const int tap = r * 3 + c / 6, k = (int)kb * 48 + (c % 6) * 8 + j;  // tap = (dz+1)*9+(dy+1)*3+(dx+1), r = (dz+1)*3+(dy+1)
      // W'[n][tap][k]: fwd  = W[co=n][ci=k][tap];  dgrad = W[co=k][ci=n][26-tap]   (src layout [Co=d0][Ci=d1][27])
      return d.mode == 6 ? ((long)n * d1 + k) * 27 + tap : ((long)k * d1 + n) * 27 + (26 - tap);
    }
    case 10: { unsigned r = i / d1; return r < d0 ? (long)i : -1; }                                   // [d0][d1] -> [d2 >= d0 rows][d1], zero rows
    case 11: { unsigned c = i / d2, r = i - c * d2; return r < d0 ? (long)(r * d1 + c) : -1; }          // [d0][d1] -> transposed [d1][d2 >= d0], zero columns
    case 12: { unsigned ci = i & 7u, t2 = i >> 3, co = t2 / d2, t = t2 - co * d2; return ci < d1 ? (long)((co * d1 + ci) * d2 + t) : -1; }   // [Co][Ci<=8][taps] -> [Co][taps][8]
    case 8: case 9: {
      // conv64.hip fragment order [os][cs][step 54][co-tile 4][lane 64][8]: lane (li, g) of co-tile nt holds output channel
      // 64 os + 16 (li>>2) + 4 nt + (li&3) (an accumulator lane owns 16 consecutive channels), contraction slot cs*64 + (step&1)*32 + 8g + j of tap step>>1
      const int j = (int)(i & 7), lane = (int)((i >> 3) & 63);
      const unsigned sn = i >> 9;
      const int nt = (int)(sn & 3), sg = (int)(sn >> 2), blk = sg / 54, st = sg - blk * 54;
      const int ncs = (d.mode == 8 ? (int)d1 : (int)d0) / 64, os = blk / ncs, cs = blk - os * ncs;
      const int g = lane >> 4, li = lane & 15, n = os * 64 + 16 * (li >> 2) + 4 * nt + (li & 3), k = cs * 64 + (st & 1) * 32 + 8 * g + j, tap = st >> 1;
      // W'[n][tap][k]: fwd = W[co=n][ci=k][tap]; dgrad = W[co=k][ci=n][26-tap]   (src layout [Co=d0][Ci=d1][27])
      return d.mode == 8 ? ((long)n * d1 + k) * 27 + tap : ((long)k * d1 + n) * 27 + (26 - tap);
    }
    default: return il;
  }
}
template <typename T> __global__ void pack_kernel(const PackDesc* descs, const int* blk2desc, const long* blkstart) {
  const PackDesc d = descs[blk2desc[blockIdx.x]];
  const long base = blkstart[blockIdx.x];
  T* dst = (T*)d.dst;
  if (d.mode == 1) {
    // 2-D transpose, one 32x32 tile per block through LDS (blkstart = tile id): source rows and destination rows are both read /
    // written along their contiguous axis.  (The element-wise gather touched 64 cache lines per wave-load: 420 us for the 50 M
    // transposed Linear weights of swin_s.)
    __shared__ float tile[32][33];
    const int tcn = (d.d1 + 31) >> 5, tr = (int)(base / tcn), tc = (int)(base - (long)tr * tcn);
    const int r0 = tr * 32, c0 = tc * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int r = ty; r < 32; r += 8)
      if (r0 + r < d.d0 && c0 + tx < d.d1) tile[r][tx] = d.src[(long)(r0 + r) * d.d1 + c0 + tx];
    __syncthreads();
#pragma unroll
    for (int c = ty; c < 32; c += 8)
      if (c0 + c < d.d1 && r0 + tx < d.d0) dst[(long)(c0 + c) * d.d0 + r0 + tx] = from_f<T>(tile[tx][c]);
    return;
  }
  if (d.mode == 2 || d.mode == 3) {
    // 3x3x3 conv weights [Co][Ci][27] -> [Co][27][Ci] (fwd) / [Ci][27 flipped][Co] (dgrad), one block per 32 channels of the axis that
    // becomes contiguous (blkstart = block id): the source is read in 108-byte tap rows, the destination written in 32-channel runs
    __shared__ float tl[32][28];
    const int Co = d.d0, Ci = d.d1, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    if (d.mode == 2) {
      const int cchunks = (Ci + 31) >> 5, co = (int)(base / cchunks), ci0 = (int)(base - (long)co * cchunks) * 32;
      const float* sp = d.src + ((long)co * Ci + ci0) * 27;
      const int nci = Ci - ci0 < 32 ? Ci - ci0 : 32;
      for (int i = threadIdx.x; i < nci * 27; i += 256) tl[i / 27][i % 27] = sp[i];       // contiguous run of nci*27 floats
      __syncthreads();
      for (int t = ty; t < 27; t += 8)
        if (tx < nci) dst[((long)co * 27 + t) * Ci + ci0 + tx] = from_f<T>(tl[tx][t]);
    } else {
      const int ochunks = (Co + 31) >> 5, ci = (int)(base / ochunks), co0 = (int)(base - (long)ci * ochunks) * 32;
      const int nco = Co - co0 < 32 ? Co - co0 : 32;
      for (int i = threadIdx.x; i < nco * 27; i += 256) { const int c = i / 27, t = i - c * 27; tl[c][t] = d.src[((long)(co0 + c) * Ci + ci) * 27 + t]; }
      __syncthreads();
      for (int t = ty; t < 27; t += 8)
        if (tx < nco) dst[((long)ci * 27 + t) * Co + co0 + tx] = from_f<T>(tl[tx][26 - t]);
    }
    return;
  }
  if (d.mode == 0) {   // plain cast (every Linear weight's forward operand): 4 consecutive elements per thread, 16-byte loads (blocks start at
    //                   multiples of 1024 elements of 64-element-aligned tensors)
    const long i = base + 4 * threadIdx.x;
    if (i + 3 < d.n) {
      const float4 v = *reinterpret_cast<const float4*>(d.src + i);
      if constexpr (sizeof(T) == 2) *reinterpret_cast<uint2*>(dst + i) = make_uint2(pk_bf16(v.x, v.y), pk_bf16(v.z, v.w));
      else *reinterpret_cast<float4*>(dst + i) = v;
    } else {
      for (long j = i; j < d.n && j < i + 4; ++j) dst[j] = from_f<T>(d.src[j]);
    }
    return;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    long i = base + u * 256 + threadIdx.x;
    if (i < d.n) { const long si = pack_src_index(d, i); dst[i] = from_f<T>(si >= 0 ? d.src[si] : 0.f); }
  }
}
int k_pack_weights(int dt, const PackDesc* descs, const int* blk2desc, const long* blkstart, int nblocks, hipStream_t st) {
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(pack_kernel<bf16_t>, dim3(nblocks), dim3(256), 0, st, descs, blk2desc, blkstart);
  else hipLaunchKernelGGL(pack_kernel<float>, dim3(nblocks), dim3(256), 0, st, descs, blk2desc, blkstart);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- global grad norm, clip coefficient, fused AdamW over the flat parameter buffer ----------------------------------------
__global__ __launch_bounds__(256) void sqnorm_kernel(const float* g, long n, double* acc) {
  __shared__ float sh[4];
  float s = 0.f;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    if (i + 3 < n) { const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i)); s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
    else for (long j = i; j < n; ++j) s += g[j] * g[j];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(acc, (double)(sh[0] + sh[1] + sh[2] + sh[3]));
}
int k_sqnorm(const float* g, long n, double* acc, hipStream_t st) {
  hipError_t e = nmh_zero_async(acc, sizeof(double), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sqnorm_kernel, dim3(ew_blocks((n + 3) / 4, 2048)), dim3(256), 0, st, g, n, acc);
  NMH_CHECK_LAUNCH();
  return 0;
}
__global__ void clip_coef_kernel(const double* acc, float max_norm, float* coef, float* norm_out) {
  double nrm = sqrt(*acc);
  double c = (double)max_norm / (nrm + 1e-6);  // torch.nn.utils.clip_grad_norm_
  *coef = max_norm > 0.f ? (float)(c < 1.0 ? c : 1.0) : 1.0f;
  if (norm_out) *norm_out = (float)nrm;
}
int k_clip_coef(const double* acc, float max_norm, float* coef, float* norm_out, hipStream_t st) {
  hipLaunchKernelGGL(clip_coef_kernel, dim3(1), dim3(1), 0, st, acc, max_norm, coef, norm_out);
  NMH_CHECK_LAUNCH();
  return 0;
}
// Gradient accumulation: g holds the SUM G of k micro-gradients, acc = |G|^2.  The step is taken on the mean G / k: its norm is |G| / k, and the factor the AdamW
// kernels multiply g by is the clip coefficient of the mean times 1 / k.  The factors are multiplied in fp64 and rounded once; with *inv_k == 1 every product is
// exact, so coef and norm_out are the bits of clip_coef_kernel.
__global__ void clip_coef_mean_kernel(const double* acc, float max_norm, const float* inv_k, float* coef, float* norm_out) {
  const double ik = (double)*inv_k;
  double nrm = sqrt(*acc) * ik;
  double c = (double)max_norm / (nrm + 1e-6);
  *coef = (float)(ik * (max_norm > 0.f ? (c < 1.0 ? c : 1.0) : 1.0));
  if (norm_out) *norm_out = (float)nrm;
}
int k_clip_coef_mean(const double* acc, float max_norm, const float* inv_k, float* coef, float* norm_out, hipStream_t st) {
  hipLaunchKernelGGL(clip_coef_mean_kernel, dim3(1), dim3(1), 0, st, acc, max_norm, inv_k, coef, norm_out);
  NMH_CHECK_LAUNCH();
  return 0;
}
// 1 / k of the step as a kernel argument (see step_params_kernel: no host-to-device copy); the value may change between replays of a captured optimizer graph
__global__ void grad_scale_kernel(float inv_k, float* __restrict__ inv_k_dev) { *inv_k_dev = inv_k; }
int k_grad_scale(float inv_k, float* inv_k_dev, hipStream_t st) {
  if (!(inv_k > 0.f) || inv_k > 1.f) return -4;      // 1 / k of k >= 1 micro-batches (NaN fails the first test)
  hipLaunchKernelGGL(grad_scale_kernel, dim3(1), dim3(1), 0, st, inv_k, inv_k_dev);
  NMH_CHECK_LAUNCH();
  return 0;
}
// one element's decoupled-weight-decay Adam update, shared by adamw_kernel and adamw_ranges_kernel (step = lr / bias_correction1, isq = 1 / sqrt(bias_correction2)):
//   m = b1 m + (1 - b1) gc;  v = b2 v + (1 - b2) gc^2;  p = p (1 - lr wd) - step m / (sqrt(v) isq + eps),   gc = g * coef.
// The fused multiply-adds are spelled out and the compiler's own contraction is off inside: every caller then rounds alike, whatever surrounds the inlined
// body -- what "one range (1, 1) gives the bits of nmh_adamw_step" rests on.  The spelling is the one the compiler chose for adamw_kernel's 16-byte loop when
// the choice was its own.
__device__ __forceinline__ void adamw_update(float& pi, float& gi, float& mi, float& vi, float cf, float lr, float wd, float b1, float b2, float eps, float step,
                                             float isq, bool zero_g) {
#pragma clang fp contract(off)
  const float gc = gi * cf;
  mi = fmaf(b1, mi, (1.0f - b1) * gc);
  vi = fmaf(b2, vi, ((1.0f - b2) * gc) * gc);
  pi = fmaf(pi, fmaf(-lr, wd, 1.0f), -((step * mi) / fmaf(sqrtf(vi), isq, eps)));
  if (zero_g) gi = 0.f;
}
// hyper = {lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2} on device (graph-replayable)
__global__ void adamw_kernel(float* p, float* g, float* m, float* v, long n, const float* hyper, const float* coef) {
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6];
  const bool zero_g = hyper[7] != 0.f;   // leave the gradient buffer cleared for the next step (saves the separate 280 MB fill)
  const float cf = coef ? *coef : 1.0f;
  const float step = lr / bc1, isq = 1.0f / sqrtf(bc2);
  auto upd = [&](float& pi, float& gi, float& mi, float& vi) { adamw_update(pi, gi, mi, vi, cf, lr, wd, b1, b2, eps, step, isq, zero_g); };
  // four parameters per thread and iteration (16-byte accesses: the four flat buffers are 16-byte aligned); scalar tail
  const long n4 = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) ? n >> 2 : 0;
  // streaming accesses (non-temporal: 8 x 280 MB pass through once per step) from SHORT blocks -- two iterations per thread: tools/probes/hbm_stream_probe.hip
  // measures 5.3 TB/s for looping grids of 2048-4096 blocks against 6.0-6.25 for blocks that retire after 16-64 bytes per thread and tensor
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    f32x4 pv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p) + i), gv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(g) + i);
    f32x4 mv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m) + i), vv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v) + i);
#pragma unroll
    for (int k = 0; k < 4; ++k) { float a = pv[k], b = gv[k], c = mv[k], d = vv[k]; upd(a, b, c, d); pv[k] = a; gv[k] = b; mv[k] = c; vv[k] = d; }
    __builtin_nontemporal_store(pv, reinterpret_cast<f32x4*>(p) + i); __builtin_nontemporal_store(mv, reinterpret_cast<f32x4*>(m) + i);
    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v) + i);
    if (zero_g) __builtin_nontemporal_store(gv, reinterpret_cast<f32x4*>(g) + i);
  }
  for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float pi = p[i], gi = g[i], mi = m[i], vi = v[i];
    upd(pi, gi, mi, vi);
    p[i] = pi; m[i] = mi; v[i] = vi;
    if (zero_g) g[i] = gi;
  }
}
// blocks of 256 threads for the two AdamW kernels: short blocks, `per` 16-byte groups per thread and tensor (see adamw_kernel)
static unsigned adamw_grid(long n) {
  static const int per = getenv("NMH_ADAMW_ITERS") ? atoi(getenv("NMH_ADAMW_ITERS")) : 2;   // 16-byte groups per thread
  long nb = ((n >> 2) + 256L * per - 1) / (256L * per);
  if (nb < 1) nb = 1;
  if (nb > (1L << 30)) nb = 1L << 30;
  return (unsigned)nb;
}
int k_adamw(float* p, float* g, float* m, float* v, long n, const float* hyper, const float* coef, hipStream_t st) {
  hipLaunchKernelGGL(adamw_kernel, dim3(adamw_grid(n)), dim3(256), 0, st, p, g, m, v, n, hyper, coef);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- the same two passes under a per-range table: (lr_scale, wd_scale) per range of the flat buffer, lr_scale == 0 = frozen ----------
// bounds[R+1] (int64, device): 0 = bounds[0] < ... < bounds[R] = n, every interior boundary a multiple of 4, so a 16-byte group lies in ONE
// range and the range is looked up once per group; scale[R][2] (device) = (lr_scale, wd_scale), finite and >= 0.
// Each block keeps the table in LDS: the scales first (8-byte reads), then the first GROUP of every range as a 32-bit index -- 12 bytes per
// range, 48 KB at NMH_ADAMW_MAX_RANGES.  The lookup is a bisection over broadcast reads (every lane of a wave reads the same or a
// neighbouring word); it never leaves [0, R), whatever the table holds.
__device__ __forceinline__ void range_table_to_lds(float2* sc, int* gb, const long* bounds, const float* scale, int R) {
  for (int r = threadIdx.x; r < R; r += blockDim.x) {
    sc[r] = reinterpret_cast<const float2*>(scale)[r];
    gb[r] = (int)(bounds[r] >> 2);
  }
  __syncthreads();
}
// the last r with gb[r] <= grp (gb[0] = 0)
__device__ __forceinline__ int range_of_group(const int* gb, int R, int grp) {
  int lo = 0, hi = R;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gb[mid] <= grp) lo = mid; else hi = mid;
  }
  return lo;
}
__global__ __launch_bounds__(256) void sqnorm_ranges_kernel(const float* g, long n, const long* bounds, const float* scale, int R, double* acc) {
  extern __shared__ float2 rt_sc[];
  int* gb = reinterpret_cast<int*>(rt_sc + R);
  __shared__ float sh[4];
  range_table_to_lds(rt_sc, gb, bounds, scale, R);
  float s = 0.f;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += (long)gridDim.x * blockDim.x * 4) {
    if (rt_sc[range_of_group(gb, R, (int)(i >> 2))].x == 0.f) continue;   // a frozen range has no gradient as far as the clip is concerned
    if (i + 3 < n) { const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(g + i)); s += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
    else for (long j = i; j < n; ++j) s += g[j] * g[j];
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(acc, (double)(sh[0] + sh[1] + sh[2] + sh[3]));
}
// adamw_kernel with the range's lr * lr_scale and weight_decay * wd_scale; the same loop, accesses and update function, so one range (1, 1) gives its bits.
// A frozen group stores nothing to p, m, v; its gradient is still cleared under zero_g.
__global__ __launch_bounds__(256) void adamw_ranges_kernel(float* p, float* g, float* m, float* v, long n, const float* hyper, const float* coef,
                                                           const long* bounds, const float* scale, int R) {
  extern __shared__ float2 rt_sc[];
  int* gb = reinterpret_cast<int*>(rt_sc + R);
  range_table_to_lds(rt_sc, gb, bounds, scale, R);
  const float lr = hyper[0], b1 = hyper[1], b2 = hyper[2], eps = hyper[3], wd = hyper[4], bc1 = hyper[5], bc2 = hyper[6];
  const bool zero_g = hyper[7] != 0.f;
  const float cf = coef ? *coef : 1.0f;
  const float isq = 1.0f / sqrtf(bc2);
  const long n4 = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) ? n >> 2 : 0;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    // the four loads are issued before the lookup, whose LDS reads then run under their latency
    f32x4 pv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p) + i), gv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(g) + i);
    f32x4 mv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m) + i), vv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v) + i);
    const float2 sc = rt_sc[range_of_group(gb, R, (int)i)];
    if (sc.x != 0.f) {
      const float lr_r = lr * sc.x, wd_r = wd * sc.y, step = lr_r / bc1;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float a = pv[k], b = gv[k], c = mv[k], d = vv[k];
        adamw_update(a, b, c, d, cf, lr_r, wd_r, b1, b2, eps, step, isq, false);
        pv[k] = a; mv[k] = c; vv[k] = d;
      }
      __builtin_nontemporal_store(pv, reinterpret_cast<f32x4*>(p) + i); __builtin_nontemporal_store(mv, reinterpret_cast<f32x4*>(m) + i);
      __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v) + i);
    }
    if (zero_g) { const f32x4 z = {0.f, 0.f, 0.f, 0.f}; __builtin_nontemporal_store(z, reinterpret_cast<f32x4*>(g) + i); }
  }
  for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    const float2 sc = rt_sc[range_of_group(gb, R, (int)(i >> 2))];
    if (sc.x != 0.f) {
      const float lr_r = lr * sc.x, wd_r = wd * sc.y;
      float pi = p[i], gi = g[i], mi = m[i], vi = v[i];
      adamw_update(pi, gi, mi, vi, cf, lr_r, wd_r, b1, b2, eps, lr_r / bc1, isq, false);
      p[i] = pi; m[i] = mi; v[i] = vi;
    }
    if (zero_g) g[i] = 0.f;
  }
}
// The entries' check of a table, on the host: -5 unless 1 <= R <= NMH_ADAMW_MAX_RANGES, bounds[0] = 0 < bounds[1] < ... < bounds[R] = n, every interior
// boundary a multiple of 4 and every scale finite and >= 0.  The table is copied through a pinned buffer on a stream of the library's own,
// so the caller's stream is never waited for (the table has to be complete in memory when the entry is called: it is built once, long
// before the first step).  While `st` is being captured the host may not copy: only R and n are checked there, and the kernels stay inside
// [0, R) and [0, n) for any contents.
static int range_table_check(const long* bounds, const float* scale, int R, long n, hipStream_t st) {
  if (R < 1 || R > NMH_ADAMW_MAX_RANGES || n < 1 || (n >> 2) > 0x7fffffffL) return -5;
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  hipError_t e = hipStreamIsCapturing(st, &cs);
  if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }
  if (cs != hipStreamCaptureStatusNone) return 0;
  static std::mutex mu;
  static hipStream_t side[64] = {};
  static char* host = nullptr;
  std::lock_guard<std::mutex> lock(mu);
  const int dev = NmhPerDeviceOnce::dev();
  const size_t nbnd = (size_t)(R + 1) * sizeof(long), nsc = (size_t)R * 2 * sizeof(float);
  if (!host && (e = hipHostMalloc(reinterpret_cast<void**>(&host), (NMH_ADAMW_MAX_RANGES + 1) * sizeof(long) + NMH_ADAMW_MAX_RANGES * 2 * sizeof(float), hipHostMallocPortable)) != hipSuccess) {
    host = nullptr; (void)hipGetLastError(); return (int)e;
  }
  if (!side[dev] && (e = hipStreamCreateWithFlags(&side[dev], hipStreamNonBlocking)) != hipSuccess) { side[dev] = nullptr; (void)hipGetLastError(); return (int)e; }
  if ((e = hipMemcpyAsync(host, bounds, nbnd, hipMemcpyDeviceToHost, side[dev])) != hipSuccess ||
      (e = hipMemcpyAsync(host + (NMH_ADAMW_MAX_RANGES + 1) * sizeof(long), scale, nsc, hipMemcpyDeviceToHost, side[dev])) != hipSuccess ||
      (e = hipStreamSynchronize(side[dev])) != hipSuccess) { (void)hipGetLastError(); return (int)e; }
  const long* b = reinterpret_cast<const long*>(host);
  const float* s = reinterpret_cast<const float*>(host + (NMH_ADAMW_MAX_RANGES + 1) * sizeof(long));
  if (b[0] != 0 || b[R] != n) return -5;
  for (int r = 0; r < R; ++r) {
    if (b[r + 1] <= b[r] || (r > 0 && (b[r] & 3))) return -5;
    if (!(s[2 * r] >= 0.f) || !(s[2 * r + 1] >= 0.f) || std::isinf(s[2 * r]) || std::isinf(s[2 * r + 1])) return -5;
  }
  return 0;
}
int k_sqnorm_ranges(const float* g, long n, const long* bounds, const float* scale, int R, double* acc, hipStream_t st) {
  const int rc = range_table_check(bounds, scale, R, n, st);
  if (rc) return rc;
  hipError_t e = nmh_zero_async(acc, sizeof(double), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(sqnorm_ranges_kernel, dim3(ew_blocks((n + 3) / 4, 2048)), dim3(256), (size_t)R * 12, st, g, n, bounds, scale, R, acc);
  NMH_CHECK_LAUNCH();
  return 0;
}
int k_adamw_ranges(float* p, float* g, float* m, float* v, long n, const float* hyper, const float* coef, const long* bounds, const float* scale, int R,
                   hipStream_t st) {
  const int rc = range_table_check(bounds, scale, R, n, st);
  if (rc) return rc;
  hipLaunchKernelGGL(adamw_ranges_kernel, dim3(adamw_grid(n)), dim3(256), (size_t)R * 12, st, p, g, m, v, n, hyper, coef, bounds, scale, R);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- input pipeline: raw radiance grid -> padded network input, one pass -------------------------------------------------------
// src: one scene as stored on disk, (W, L, H, 4) channels-last, fp32 or uint8 (nerf_rpn/datasets.py:88-101).  In one pass:
//   uint8 -> /255; density -> alpha = clip(1 - exp(-exp(sigma)/100), 0, 1) on channel 3 (:247-248, fp32 grids, optional);
//   (W,L,H,C) -> (C,W,L,H); z-up 90-degree rotation = transpose axes 0,1 then flip axis 0, and flips of axes 0 / 1 (:198-233);
//   zero padding at the high end of every axis up to R^3 (torch_utils.py:56-90).  dst: (4, R, R, R) fp32 slot of the batch tensor.
// Output voxel (i, j, k) of the (A0, A1, A2 = H) result reads source voxel (w, l, h = k): the last axis is never permuted, so both
// the 16-byte (4-byte for uint8) source reads and the four plane writes are coalesced along k.
// source voxel index (w * L + l) * H + k of output voxel (i, j, k), or -1 in the padding; shared by the scene and the label kernel
__device__ __forceinline__ long prepare_src_voxel(int i, int j, int k, int W, int L, int H, bool rot, bool f0, bool f1) {
  const int A0 = rot ? L : W, A1 = rot ? W : L;
  if (i >= A0 || j >= A1 || k >= H) return -1;
  // undo the flips (applied last), then the rotation: rotated[i][j] = x[j][A0-1-i]
  const int ii = f0 ? A0 - 1 - i : i, jj = f1 ? A1 - 1 - j : j;
  int w, l;
  if (rot) { w = jj; l = A0 - 1 - ii; } else { w = ii; l = jj; }
  return ((long)w * L + l) * H + k;
}
template <typename S>
__global__ __launch_bounds__(256) void grid_prepare_kernel(const S* __restrict__ src, int W, int L, int H, float* __restrict__ dst, int R, int flags) {
  const bool rot = flags & 1, f0 = flags & 2, f1 = flags & 4, dens = flags & 8;
  const long R3 = (long)R * R * R;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < R3; o += (long)gridDim.x * 256) {
    const int k = (int)(o % R);
    const long t = o / R;
    const int j = (int)(t % R), i = (int)(t / R);
    float v0 = 0.f, v1 = 0.f, v2 = 0.f, v3 = 0.f;
    const long sv = prepare_src_voxel(i, j, k, W, L, H, rot, f0, f1);
    if (sv >= 0) {
      const long si = sv * 4;
      if constexpr (sizeof(S) == 1) {
        const uchar4 u = *reinterpret_cast<const uchar4*>(src + si);
        v0 = u.x * (1.0f / 255.0f); v1 = u.y * (1.0f / 255.0f); v2 = u.z * (1.0f / 255.0f); v3 = u.w * (1.0f / 255.0f);
      } else {
        const float4 u = *reinterpret_cast<const float4*>(src + si);
        v0 = u.x; v1 = u.y; v2 = u.z; v3 = u.w;
        if (dens) v3 = fminf(fmaxf(1.0f - expf(-expf(v3) / 100.0f), 0.0f), 1.0f);
      }
    }
    dst[o] = v0; dst[R3 + o] = v1; dst[2 * R3 + o] = v2; dst[3 * R3 + o] = v3;
  }
}
int k_grid_prepare(int src_u8, const void* src, int W, int L, int H, float* dst, int R, int flags, hipStream_t st) {
  const bool rot = flags & 1;
  if ((rot ? L : W) > R || (rot ? W : L) > R || H > R || W <= 0 || L <= 0 || H <= 0) return -2;
  const long R3 = (long)R * R * R;
  const unsigned nb = (unsigned)((R3 + 255) / 256 < 8192 ? (R3 + 255) / 256 : 8192);
  if (src_u8) hipLaunchKernelGGL(grid_prepare_kernel<unsigned char>, dim3(nb), dim3(256), 0, st, (const unsigned char*)src, W, L, H, dst, R, flags);
  else hipLaunchKernelGGL(grid_prepare_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)src, W, L, H, dst, R, flags);
  NMH_CHECK_LAUNCH();
  return 0;
}
// label volume of a scene: (W, L, H) class ids, fp32 / int32 / int64 / uint8 -> the (R, R, R) fp32 slot of the label batch, value = (float)label, under
// the rotation and flips of grid_prepare_kernel (bits 1 / 2 / 4 of flags; bit 8 means nothing here) and with zero = unlabelled padding.  A pure gather,
// reads and writes coalesced along k.
template <typename S>
__global__ __launch_bounds__(256) void labels_prepare_kernel(const S* __restrict__ src, int W, int L, int H, float* __restrict__ dst, int R, int flags) {
  const bool rot = flags & 1, f0 = flags & 2, f1 = flags & 4;
  const long R3 = (long)R * R * R;
  for (long o = (long)blockIdx.x * 256 + threadIdx.x; o < R3; o += (long)gridDim.x * 256) {
    const int k = (int)(o % R);
    const long t = o / R;
    const int j = (int)(t % R), i = (int)(t / R);
    const long sv = prepare_src_voxel(i, j, k, W, L, H, rot, f0, f1);
    dst[o] = sv >= 0 ? (float)src[sv] : 0.f;
  }
}
int k_labels_prepare(int dt, const void* src, int W, int L, int H, float* dst, int R, int flags, hipStream_t st) {
  const bool rot = flags & 1;
  if ((rot ? L : W) > R || (rot ? W : L) > R || H > R || W <= 0 || L <= 0 || H <= 0 || dt < 0 || dt > 3) return -2;
  const long R3 = (long)R * R * R;
  const unsigned nb = (unsigned)((R3 + 255) / 256 < 8192 ? (R3 + 255) / 256 : 8192);
  if (dt == 0) hipLaunchKernelGGL(labels_prepare_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)src, W, L, H, dst, R, flags);
  else if (dt == 1) hipLaunchKernelGGL(labels_prepare_kernel<int>, dim3(nb), dim3(256), 0, st, (const int*)src, W, L, H, dst, R, flags);
  else if (dt == 2) hipLaunchKernelGGL(labels_prepare_kernel<long long>, dim3(nb), dim3(256), 0, st, (const long long*)src, W, L, H, dst, R, flags);
  else hipLaunchKernelGGL(labels_prepare_kernel<unsigned char>, dim3(nb), dim3(256), 0, st, (const unsigned char*)src, W, L, H, dst, R, flags);
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- FPN neck pieces (nerf_rpn/model/fpn.py:150-166, the rank-1 widening of SURVEY 8(f)) ------------------------------------------
// top-down pathway: fine[b][zf][yf][xf][:] += coarse[b][src(zf)][src(yf)][src(xf)][:], src = F.interpolate(mode='nearest', size=fine):
// src(i) = min(int(floorf(i * (float)in / out)), in - 1) exactly as ATen computes it; channels-last, 8 channels per thread.
struct UpGeom { int Dc, Hc, Wc, Df, Hf, Wf; float sz, sy, sx; };
__device__ __forceinline__ int nearest_src(int i, float s, int n) { int v = (int)floorf((float)i * s); return v < n - 1 ? v : n - 1; }
template <typename T>
__global__ __launch_bounds__(256) void nearest_up_add_kernel(const T* __restrict__ coarse, T* __restrict__ fine, int B, UpGeom g, int C8) {
  const long total = (long)B * g.Df * g.Hf * g.Wf * C8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C8);
    long v = i / C8;
    const int xf = (int)(v % g.Wf); v /= g.Wf;
    const int yf = (int)(v % g.Hf); v /= g.Hf;
    const int zf = (int)(v % g.Df);
    const int b = (int)(v / g.Df);
    const long cv = (((long)b * g.Dc + nearest_src(zf, g.sz, g.Dc)) * g.Hc + nearest_src(yf, g.sy, g.Hc)) * g.Wc + nearest_src(xf, g.sx, g.Wc);
    float a[8], s[8];
    Vec8<T>::load(fine + i * 8, a);
    Vec8<T>::load(coarse + (cv * C8 + c) * 8, s);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] += s[j];
    Vec8<T>::store(fine + i * 8, a);
  }
}
// adjoint: dcoarse[b][zc][yc][xc][:] += sum over the fine voxels whose nearest source is (zc,yc,xc) (a contiguous box per axis)
template <typename T>
__global__ __launch_bounds__(256) void nearest_up_add_bwd_kernel(const T* __restrict__ dfine, T* __restrict__ dcoarse, int B, UpGeom g, int C8) {
  const long total = (long)B * g.Dc * g.Hc * g.Wc * C8;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C8);
    long v = i / C8;
    const int xc = (int)(v % g.Wc); v /= g.Wc;
    const int yc = (int)(v % g.Hc); v /= g.Hc;
    const int zc = (int)(v % g.Dc);
    const int b = (int)(v / g.Dc);
    float a[8];
    Vec8<T>::load(dcoarse + i * 8, a);
    // candidate fine range per axis: [floor(c*out/in) - 1, floor((c+1)*out/in) + 1], filtered by the exact source test
    const int z0 = max(0, (int)((long)zc * g.Df / g.Dc) - 1), z1 = min(g.Df - 1, (int)((long)(zc + 1) * g.Df / g.Dc) + 1);
    const int y0 = max(0, (int)((long)yc * g.Hf / g.Hc) - 1), y1 = min(g.Hf - 1, (int)((long)(yc + 1) * g.Hf / g.Hc) + 1);
    const int x0 = max(0, (int)((long)xc * g.Wf / g.Wc) - 1), x1 = min(g.Wf - 1, (int)((long)(xc + 1) * g.Wf / g.Wc) + 1);
    for (int zf = z0; zf <= z1; ++zf) {
      if (nearest_src(zf, g.sz, g.Dc) != zc) continue;
      for (int yf = y0; yf <= y1; ++yf) {
        if (nearest_src(yf, g.sy, g.Hc) != yc) continue;
        for (int xf = x0; xf <= x1; ++xf) {
          if (nearest_src(xf, g.sx, g.Wc) != xc) continue;
          float s[8];
          Vec8<T>::load(dfine + (((((long)b * g.Df + zf) * g.Hf + yf) * g.Wf + xf) * C8 + c) * 8, s);
#pragma unroll
          for (int j = 0; j < 8; ++j) a[j] += s[j];
        }
      }
    }
    Vec8<T>::store(dcoarse + i * 8, a);
  }
}
static UpGeom up_geom(int Dc, int Hc, int Wc, int Df, int Hf, int Wf) {
  UpGeom g{Dc, Hc, Wc, Df, Hf, Wf, (float)Dc / (float)Df, (float)Hc / (float)Hf, (float)Wc / (float)Wf};
  return g;
}
int k_nearest_up_add(int dt, const void* coarse, void* fine, int B, int Dc, int Hc, int Wc, int Df, int Hf, int Wf, int C, int bwd, hipStream_t st) {
  if (C % 8 || B <= 0 || Dc <= 0 || Hc <= 0 || Wc <= 0 || Df <= 0 || Hf <= 0 || Wf <= 0) return -2;
  const UpGeom g = up_geom(Dc, Hc, Wc, Df, Hf, Wf);
  const int C8 = C / 8;
  if (!bwd) {
    const unsigned nb = ew_blocks((long)B * Df * Hf * Wf * C8);
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(nearest_up_add_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, (const bf16_t*)coarse, (bf16_t*)fine, B, g, C8);
    else hipLaunchKernelGGL(nearest_up_add_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)coarse, (float*)fine, B, g, C8);
  } else {  // (dfine = `fine` is read, dcoarse = `coarse` is accumulated into)
    const unsigned nb = ew_blocks((long)B * Dc * Hc * Wc * C8);
    if (dt == NMH_DT_BF16) hipLaunchKernelGGL(nearest_up_add_bwd_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, (const bf16_t*)fine, (bf16_t*)const_cast<void*>(coarse), B, g, C8);
    else hipLaunchKernelGGL(nearest_up_add_bwd_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)fine, (float*)const_cast<void*>(coarse), B, g, C8);
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

// channels-last compute tensors <-> the NCDHW fp32 feature maps the detection heads consume (feature_extractor.py:1183-1185):
// per sample a [V][C] <-> [C][V] transpose through a 32x33 LDS tile, both sides coalesced; dir 0: T [V][C] -> fp32 [C][V], 1: back
template <typename T, int DIR>
__global__ __launch_bounds__(256) void vc_transpose_kernel(const void* __restrict__ src_, void* __restrict__ dst_, long V, int C) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z;
  const long v0 = (long)blockIdx.x * 32;
  const int c0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8 threads
  if (DIR == 0) {
    const T* src = (const T*)src_ + (long)b * V * C;
    float* dst = (float*)dst_ + (long)b * V * C;
#pragma unroll
    for (int r = ty; r < 32; r += 8)
      if (v0 + r < V && c0 + tx < C) tile[r][tx] = to_f(src[(v0 + r) * C + c0 + tx]);
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8)
      if (c0 + r < C && v0 + tx < V) dst[(long)(c0 + r) * V + v0 + tx] = tile[tx][r];
  } else {
    const float* src = (const float*)src_ + (long)b * V * C;
    T* dst = (T*)dst_ + (long)b * V * C;
#pragma unroll
    for (int r = ty; r < 32; r += 8)
      if (c0 + r < C && v0 + tx < V) tile[tx][r] = src[(long)(c0 + r) * V + v0 + tx];
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8)
      if (v0 + r < V && c0 + tx < C) dst[(v0 + r) * C + c0 + tx] = from_f<T>(tile[r][tx]);
  }
}
int k_vc_transpose(int dt, const void* src, void* dst, int B, long V, int C, int dir, hipStream_t st) {
  if (B <= 0 || V <= 0 || C <= 0 || B > 65535 || (C + 31) / 32 > 65535) return -2;
  dim3 grid((unsigned)((V + 31) / 32), (unsigned)((C + 31) / 32), (unsigned)B);
  if (dt == NMH_DT_BF16) {
    if (dir == 0) hipLaunchKernelGGL((vc_transpose_kernel<bf16_t, 0>), grid, dim3(256), 0, st, src, dst, V, C);
    else hipLaunchKernelGGL((vc_transpose_kernel<bf16_t, 1>), grid, dim3(256), 0, st, src, dst, V, C);
  } else {
    if (dir == 0) hipLaunchKernelGGL((vc_transpose_kernel<float, 0>), grid, dim3(256), 0, st, src, dst, V, C);
    else hipLaunchKernelGGL((vc_transpose_kernel<float, 1>), grid, dim3(256), 0, st, src, dst, V, C);
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

// ---- strided 2-D copy: dst[m][0..C) = src[m][0..C) with independent row strides (skip connection into / out of the channel-concatenated
// decoder tensor, unetr_block.py:196-197: torch.cat((out, skip), dim=1) in channels-last = a column block copy), 16 bytes per thread ----
template <typename T>
__global__ __launch_bounds__(256) void copy_cols_kernel(const T* __restrict__ src, long lds, T* __restrict__ dst, long ldd, long M, int Cv) {
  constexpr int E = 16 / sizeof(T);
  const long total = M * Cv;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const long m = i / Cv;
    const int c = (int)(i - m * Cv);
    *reinterpret_cast<uint4*>(dst + m * ldd + c * E) = *reinterpret_cast<const uint4*>(src + m * lds + c * E);
  }
}
int k_copy_cols(int dt, const void* src, long lds, void* dst, long ldd, long M, int C, hipStream_t st) {
  const int E = dt == NMH_DT_BF16 ? 8 : 4;
  if (M <= 0 || C <= 0 || C % E || lds % E || ldd % E || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return -2;
  const unsigned nb = ew_blocks(M * (C / E));
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(copy_cols_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, (const bf16_t*)src, lds, (bf16_t*)dst, ldd, M, C / E);
  else hipLaunchKernelGGL(copy_cols_kernel<float>, dim3(nb), dim3(256), 0, st, (const float*)src, lds, (float*)dst, ldd, M, C / E);
  NMH_CHECK_LAUNCH();
  return 0;
}
