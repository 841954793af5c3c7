// Stage 0's first Swin block on the KEPT windows only.  A removed token enters the encoder as mask_token without a position
// (swin_mae3d.py:1375-1380), the block mask is drawn per 4x4x4-token block and the first block has shift 0: its windows ARE the mask blocks, every removed
// window holds 64 identical rows, and every row-wise or per-window computation gives all removed windows of a sample the same 64 output rows.
//
// Compact layout [B][capW + 1][64][C]: window k of a sample = its k-th kept window (raster order of windows), rows inside a window in the window's own
// (dz, dy, dx) raster order; windows behind the kept count are zero rows; slot capW holds 64 rows of mask_token -- the representative of every removed window of
// that sample.  Seen as a token grid (B, 4 (capW + 1), 4, 4) with shift 0, token order equals window order, so the block's kernels run on it unchanged.
//
//   b0_rowmap      mask -> rowmap [n + 2] (token -> compact row, the patch-embed gather's map) and wmap [nW + capW] (window -> slot, slot -> window)
//   b0_ln_fwd/bwd  the patch-embed LayerNorm (+ pos_embed) on compact rows; the representative rows read mask_token / give d(mask_token)
//   b0_expand      compact block output -> dense [B][n][C]: a removed window receives the representative window's rows
//   b0_reduce      dense gradient -> compact: kept windows copied, the representative row i = fp32 sum (fixed order) of row i of every removed window
// Every sum is taken in an order that depends on the shapes alone (no float atomics).
#include "common.hpp"
#include "kernels.hpp"

namespace {

constexpr int B0_LPR = 16;             // lanes per row: 16 chunks of 8 columns, C <= 128
constexpr int B0_SEG = 16;             // segments of the window range in the representative sum

__device__ __forceinline__ int b0_token(int w, int i, int g) {   // token of in-window position i of window w on a g^3 grid
  const int nw = g >> 2;
  const int wx = w % nw, wy = (w / nw) % nw, wz = w / (nw * nw);
  return ((wz * 4 + (i >> 4)) * g + wy * 4 + ((i >> 2) & 3)) * g + wx * 4 + (i & 3);
}

__device__ __forceinline__ float b0_group_sum(float v) {
#pragma unroll
  for (int o = B0_LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <typename T> __device__ __forceinline__ void b0_copy8(T* d, const T* s) {
  if constexpr (sizeof(T) == 2) *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(s);
  else {
    const float4 a = *reinterpret_cast<const float4*>(s), b = *reinterpret_cast<const float4*>(s + 4);
    *reinterpret_cast<float4*>(d) = a;
    *reinterpret_cast<float4*>(d + 4) = b;
  }
}
template <typename T> __device__ __forceinline__ void b0_zero8(T* d) {
  if constexpr (sizeof(T) == 2) *reinterpret_cast<uint4*>(d) = make_uint4(0u, 0u, 0u, 0u);
  else {
    *reinterpret_cast<float4*>(d) = make_float4(0.f, 0.f, 0.f, 0.f);
    *reinterpret_cast<float4*>(d + 4) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// One workgroup.  A window is kept iff its first token is (the host checks that the mask is constant on every window).
__global__ __launch_bounds__(1024) void b0_rowmap_kernel(const unsigned char* __restrict__ mask, int g, int capW, int* __restrict__ rowmap, int* __restrict__ wmap) {
  __shared__ int wsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nw = g >> 2, nW = nw * nw * nw, n = g * g * g;
  for (int k = tid; k < capW; k += 1024) wmap[nW + k] = -1;
  __syncthreads();
  int base = 0;
  for (int w0 = 0; w0 < nW; w0 += 1024) {
    const int w = w0 + tid;
    const int kept = (w < nW && mask[b0_token(w, 0, g)] == 0) ? 1 : 0;
    int inc = kept;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (lane >= o) inc += v; }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int pos = base, tot = 0;
    for (int v = 0; v < 16; ++v) { if (v < wave) pos += wsum[v]; tot += wsum[v]; }
    const int slot = pos + inc - kept;
    if (w < nW) {
      const int s = (kept && slot < capW) ? slot : -1;
      wmap[w] = s;
      if (s >= 0) wmap[nW + s] = w;
    }
    base += tot;
    __syncthreads();
  }
  __threadfence_block();
  __syncthreads();
  for (int t = tid; t < n; t += 1024) {
    const int tx = t % g, ty = (t / g) % g, tz = t / (g * g);
    const int w = ((tz >> 2) * nw + (ty >> 2)) * nw + (tx >> 2), i = (tz & 3) * 16 + (ty & 3) * 4 + (tx & 3);
    const int s = wmap[w];
    rowmap[t] = s < 0 ? -1 : s * 64 + i;
  }
  if (tid == 0) { rowmap[n] = 64 * (base < capW ? base : capW); rowmap[n + 1] = base > capW ? 1 : 0; }
}

struct B0Ln {
  const void* x; void* out; const float* gamma; const float* beta; float eps; float* mean; float* rstd;
  const float* pos; const float* mask_token; const int* wmap; int B, g, capW, C;
};

// rows [B][capW + 1][64]: 16 lanes per row.  The arithmetic of a kept row is that of ln_fwd_kernel<T, 16, 1, 0> (norm.hip), operation for operation.
template <typename T> __global__ __launch_bounds__(256) void b0_ln_fwd_kernel(B0Ln a) {
  const int sub = threadIdx.x % B0_LPR;
  const int C = a.C, nch = C >> 3, g = a.g;
  const int nw = g >> 2, nW = nw * nw * nw;
  const long rps = 64L * (a.capW + 1), rows = a.B * rps;
  const T* x = (const T*)a.x;
  T* out = (T*)a.out;
  const float invC = 1.0f / (float)C;
  for (long row = (long)blockIdx.x * (256 / B0_LPR) + threadIdx.x / B0_LPR; row < rows; row += (long)gridDim.x * (256 / B0_LPR)) {
    const int rr = (int)(row % rps), slot = rr >> 6, i = rr & 63;
    const bool rep = slot == a.capW;
    const int w = rep ? -1 : a.wmap[nW + slot];
    const bool live = w >= 0;
    const long tp = live ? b0_token(w, i, g) : 0;
    float v[8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
    if (sub < nch && live) {
      Vec8<T>::load(x + row * C + sub * 8, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += v[j];
    }
    const float mean = b0_group_sum(s) * invC;
    float q = 0.f;
    if (sub < nch)
#pragma unroll
      for (int j = 0; j < 8; ++j) { float d = v[j] - mean; q += d * d; }
    const float rstd = rsqrtf(b0_group_sum(q) * invC + a.eps);
    if (sub < nch) {
      const int c = sub;
      float o[8];
      if (rep) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = a.mask_token[c * 8 + j];
      } else if (!live) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[j] - mean) * rstd * a.gamma[c * 8 + j] + a.beta[c * 8 + j];
        if (a.pos) {
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += a.pos[tp * C + c * 8 + j];
        }
      }
      Vec8<T>::store(out + row * C + c * 8, o);
    }
    if (sub == 0) { a.mean[row] = live ? mean : 0.f; a.rstd[row] = live ? rstd : 0.f; }
  }
}

struct B0LnBwd {
  const void* dy; const void* x; const float* gamma; const float* mean; const float* rstd; void* dx; float* part; const int* wmap; int B, g, capW, C;
};

// dx = rstd (gh - mean(gh) - xhat mean(gh xhat)), gh = dy gamma, on the kept rows; zero on every other row (they are operands of the weight gradient).
// part[block][3 C]: the workgroup's sums of dy xhat, dy (kept rows) and of dy over the representative rows, each added in a fixed order.
template <typename T> __global__ __launch_bounds__(256) void b0_ln_bwd_kernel(B0LnBwd a) {
  __shared__ float sp[256 / B0_LPR][3 * 8 * B0_LPR];
  const int sub = threadIdx.x % B0_LPR, rg = threadIdx.x / B0_LPR;
  const int C = a.C, nch = C >> 3, g = a.g;
  const int nw = g >> 2, nW = nw * nw * nw;
  const long rps = 64L * (a.capW + 1), rows = a.B * rps;
  const T* x = (const T*)a.x;
  const T* dy = (const T*)a.dy;
  T* dx = (T*)a.dx;
  const float invC = 1.0f / (float)C;
  float pg[8], pb[8], pm[8], gam[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) { pg[j] = 0.f; pb[j] = 0.f; pm[j] = 0.f; gam[j] = sub < nch ? a.gamma[sub * 8 + j] : 0.f; }
  for (long row = (long)blockIdx.x * (256 / B0_LPR) + rg; row < rows; row += (long)gridDim.x * (256 / B0_LPR)) {
    const int rr = (int)(row % rps), slot = rr >> 6;
    const bool rep = slot == a.capW;
    const bool live = !rep && a.wmap[nW + slot] >= 0;
    float d[8], xh[8], gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { d[j] = 0.f; xh[j] = 0.f; gv[j] = 0.f; }
    float s1 = 0.f, s2 = 0.f;
    if (sub < nch && (live || rep)) Vec8<T>::load(dy + row * C + sub * 8, d);
    if (rep) {
#pragma unroll
      for (int j = 0; j < 8; ++j) pm[j] += d[j];
    } else if (live && sub < nch) {
      const float mean = a.mean[row], rstd = a.rstd[row];
      float xv[8];
      Vec8<T>::load(x + row * C + sub * 8, xv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        xh[j] = (xv[j] - mean) * rstd;
        pg[j] += d[j] * xh[j];
        pb[j] += d[j];
        gv[j] = d[j] * gam[j];
        s1 += gv[j];
        s2 += gv[j] * xh[j];
      }
    }
    const float m1 = b0_group_sum(s1) * invC, m2 = b0_group_sum(s2) * invC;
    if (sub < nch) {
      float o[8];
      const float rstd = live ? a.rstd[row] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = live ? rstd * (gv[j] - m1 - xh[j] * m2) : 0.f;
      Vec8<T>::store(dx + row * C + sub * 8, o);
    }
  }
  if (sub < nch) {
#pragma unroll
    for (int j = 0; j < 8; ++j) { sp[rg][sub * 8 + j] = pg[j]; sp[rg][C + sub * 8 + j] = pb[j]; sp[rg][2 * C + sub * 8 + j] = pm[j]; }
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 3 * C; idx += 256) {
    float t = 0.f;
    for (int r = 0; r < 256 / B0_LPR; ++r) t += sp[r][idx];
    a.part[(long)blockIdx.x * 3 * C + idx] = t;
  }
}

// one workgroup: column sums of part[nb][3 C] in ascending block order, added to dgamma | dbeta | dmask_token
__global__ __launch_bounds__(256) void b0_ln_reduce_kernel(const float* __restrict__ part, int nb, int C, float* dgamma, float* dbeta, float* dmask) {
  for (int idx = threadIdx.x; idx < 3 * C; idx += 256) {
    float t = 0.f;
    for (int b = 0; b < nb; ++b) t += part[(long)b * 3 * C + idx];
    float* dst = idx < C ? dgamma + idx : idx < 2 * C ? dbeta + (idx - C) : dmask + (idx - 2 * C);
    *dst += t;
  }
}

template <typename T> __global__ __launch_bounds__(256) void b0_expand_kernel(const T* __restrict__ yc, T* __restrict__ y, const int* __restrict__ wmap, int B, int g, int capW, int C) {
  const int nch = C >> 3, nw = g >> 2;
  const long n = (long)g * g * g, rps = 64L * (capW + 1), total = B * n * nch;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const long row = idx / nch;
    const int c = (int)(idx - row * nch);
    const int t = (int)(row % n);
    const long b = row / n;
    const int tx = t % g, ty = (t / g) % g, tz = t / (g * g);
    const int w = ((tz >> 2) * nw + (ty >> 2)) * nw + (tx >> 2), i = (tz & 3) * 16 + (ty & 3) * 4 + (tx & 3);
    const int s = wmap[w];
    const long src = b * rps + (s < 0 ? capW : s) * 64L + i;
    b0_copy8<T>(y + row * C + c * 8, yc + src * C + c * 8);
  }
}

// workgroups [0, 64 B): the representative row i of sample b -- 16 segments of the window range, each summed in ascending window order by 16 lanes (8 columns
// each), then the 16 partial sums in ascending order.  The other workgroups copy the kept windows and zero the windows behind the count.
template <typename T> __global__ __launch_bounds__(256) void b0_reduce_kernel(const T* __restrict__ dy, T* __restrict__ dyc, const int* __restrict__ wmap, int B, int g, int capW, int C) {
  __shared__ float sp[B0_SEG][8 * B0_LPR];
  const int nch = C >> 3, nw = g >> 2, nW = nw * nw * nw;
  const long n = (long)g * g * g, rps = 64L * (capW + 1);
  if ((int)blockIdx.x < 64 * B) {
    const int b = blockIdx.x >> 6, i = blockIdx.x & 63;
    const int c = threadIdx.x % B0_LPR, seg = threadIdx.x / B0_LPR;
    const int L = (nW + B0_SEG - 1) / B0_SEG;
    const int w1 = min(nW, (seg + 1) * L);
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (c < nch)
      for (int w = seg * L; w < w1; ++w)
        if (wmap[w] < 0) {
          float v[8];
          Vec8<T>::load(dy + ((long)b * n + b0_token(w, i, g)) * C + c * 8, v);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += v[j];
        }
#pragma unroll
    for (int j = 0; j < 8; ++j) sp[seg][c * 8 + j] = acc[j];
    __syncthreads();
    if ((int)threadIdx.x < nch) {
      float o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float t = 0.f;
        for (int s = 0; s < B0_SEG; ++s) t += sp[s][threadIdx.x * 8 + j];
        o[j] = t;
      }
      Vec8<T>::store(dyc + ((long)b * rps + capW * 64L + i) * C + threadIdx.x * 8, o);
    }
    return;
  }
  const long total = (long)B * capW * 64 * nch, nblk = (long)gridDim.x - 64 * B;
  for (long idx = ((long)blockIdx.x - 64 * B) * 256 + threadIdx.x; idx < total; idx += nblk * 256) {
    const long r = idx / nch;
    const int c = (int)(idx - r * nch);
    const long b = r / (capW * 64L);
    const int rr = (int)(r - b * capW * 64L), slot = rr >> 6, i = rr & 63;
    const int w = wmap[nW + slot];
    T* dst = dyc + (b * rps + rr) * C + c * 8;
    if (w < 0) b0_zero8<T>(dst);
    else b0_copy8<T>(dst, dy + (b * n + b0_token(w, i, g)) * C + c * 8);
  }
}

bool b0_dims_ok(int B, int g, int capW, int C) {
  return B > 0 && g > 0 && g % 4 == 0 && capW > 0 && capW <= (g / 4) * (g / 4) * (g / 4) && C > 0 && C % 8 == 0 && C <= 8 * B0_LPR
         && (long)B * g * g * g < (1L << 31) / 2;
}

}  // namespace

int k_b0_supported(int C) { return (C > 0 && C % 8 == 0 && C <= 8 * B0_LPR) ? 1 : 0; }

int k_b0_rowmap(const unsigned char* mask, int g, int capW, int* rowmap, int* wmap, hipStream_t st) {
  if (!b0_dims_ok(1, g, capW, 8)) return -2;
  hipLaunchKernelGGL(b0_rowmap_kernel, dim3(1), dim3(1024), 0, st, mask, g, capW, rowmap, wmap);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_b0_ln_fwd(int dt, const void* y0, void* out, const float* gamma, const float* beta, float eps, float* mean, float* rstd, const float* pos, const float* mask_token,
                const int* wmap, int B, int g, int capW, int C, hipStream_t st) {
  if (!b0_dims_ok(B, g, capW, C)) return -2;
  const long rows = (long)B * 64 * (capW + 1);
  long nb = (rows + 15) / 16;
  if (nb > 8192) nb = 8192;
  B0Ln a{y0, out, gamma, beta, eps, mean, rstd, pos, mask_token, wmap, B, g, capW, C};
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(b0_ln_fwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(b0_ln_fwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, a);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_b0_ln_bwd(int dt, const void* dx0, const void* y0, const float* gamma, const float* mean, const float* rstd, void* dy0, float* dgamma, float* dbeta, float* dmask_token,
                float* part, long part_floats, const int* wmap, int B, int g, int capW, int C, hipStream_t st) {
  if (!b0_dims_ok(B, g, capW, C)) return -2;
  const long rows = (long)B * 64 * (capW + 1);
  long nb = (rows + 15) / 16;
  if (nb > B0_LN_BWD_BLOCKS) nb = B0_LN_BWD_BLOCKS;
  if (part_floats < nb * 3 * C) return -2;
  B0LnBwd a{dx0, y0, gamma, mean, rstd, dy0, part, wmap, B, g, capW, C};
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(b0_ln_bwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(b0_ln_bwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, a);
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(b0_ln_reduce_kernel, dim3(1), dim3(256), 0, st, part, (int)nb, C, dgamma, dbeta, dmask_token);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_b0_expand(int dt, const void* yc, void* y, const int* wmap, int B, int g, int capW, int C, hipStream_t st) {
  if (!b0_dims_ok(B, g, capW, C)) return -2;
  const long total = (long)B * g * g * g * (C / 8);
  long nb = (total + 255) / 256;
  if (nb > 16384) nb = 16384;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(b0_expand_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (const bf16_t*)yc, (bf16_t*)y, wmap, B, g, capW, C);
  else hipLaunchKernelGGL(b0_expand_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (const float*)yc, (float*)y, wmap, B, g, capW, C);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_b0_reduce(int dt, const void* dy, void* dyc, const int* wmap, int B, int g, int capW, int C, hipStream_t st) {
  if (!b0_dims_ok(B, g, capW, C)) return -2;
  const long total = (long)B * capW * 64 * (C / 8);
  long nb = (total + 255) / 256;
  if (nb > 8192) nb = 8192;
  nb += 64L * B;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(b0_reduce_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (const bf16_t*)dy, (bf16_t*)dyc, wmap, B, g, capW, C);
  else hipLaunchKernelGGL(b0_reduce_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (const float*)dy, (float*)dyc, wmap, B, g, capW, C);
  NMH_CHECK_LAUNCH();
  return 0;
}
