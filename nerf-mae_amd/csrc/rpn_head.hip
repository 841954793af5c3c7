// Output stage of the reference's RPNHead (nerf_rpn/model/anchor.py:177-224) and the ReLU between its convolutions, as gfx950 kernels:
//   head_out_fwd   relu? -> cls_logits (1x1x1, Cin -> A) and bbox_pred (1x1x1, Cin -> A C) of every level in ONE launch, read from the channels-last
//                  activation t (N, W, H, D, Cin) of the last 3x3x3 conv and written as the fp32 planes the loss and the proposal kernels read in place:
//                  objectness (N, A, W, H, D), pred_bbox_deltas (N, A C, W, H, D), channel a C + c;
//   head_out_dt    dt = relu'(t) o (G Wcat): the gradient of t, channels-last in the compute dtype, all levels in one launch;
//   head_out_dw    per-workgroup partial sums of Gt relu(t) and of the column sums of G over the workgroup's share of the voxels of all levels, then
//   head_out_red   the partials summed in workgroup order and added to the weight and bias gradients: a fixed order, two runs are bit-identical;
//   relu_ / relu_bwd_   y = max(y, 0) in place; dy = 0 where y <= 0, in place: 8 elements per lane.
// Wcat is never materialised: "column" j of the head is row j of cls_logits.weight for j < A and row j - A of bbox_pred.weight above, J = A (1 + C) in all.
// relu'(0) = 0.  With relu = 0 (conv_depth 0: the reference's empty nn.Sequential is the identity) t is used as it is and nothing is masked.
//
// Fragment maps (v_mfma_f32_32x32x16_bf16, and v_mfma_f32_32x32x2_f32 for the exact fp32 path): lane l, r = l & 31, h = l >> 5.  bf16: element e = 0..7 of
// A is A[row r][k = 8 h + e], of B is B[k = 8 h + e][col r].  fp32: one element per instruction, A[row r][k = h], B[k = h][col r]; a lane loads 4 consecutive
// contraction elements and four instructions consume them, so the two halves of a step of 8 cover k = 4 h + q.  C/D for both: col = r, row = (i & 3) +
// 8 (i >> 2) + 4 h for register i = 0..15.  A step's contraction indices only have to agree between A and B, which they do by construction.
//   fwd: D[column j][voxel]   = sum_c  Wcat[j][c] relu(t[voxel][c]): the voxel is on the lane, so every register's store is 32 consecutive floats of ONE plane;
//   dt:  D[channel c][voxel]  = sum_j  Wcat[j][c] G[j][voxel]: registers 4 q .. 4 q + 3 are channels 8 q + 4 h .. + 3 of the lane's voxel, one 8-byte store (bf16);
//   dw:  D[column j][channel] = sum_v  G[j][v] relu(t[v][c]): the channel is on the lane, a register's store is 32 consecutive floats of a partial's row.
// G is fp32 and t / Wcat are bf16: in the bf16 path G enters the matrix cores as hi + lo, hi = bf16(G), lo = bf16(G - hi) (two instructions, 16 mantissa
// bits), so that the loss gradient is not rounded to 8 bits before it is summed; everything accumulates in fp32.  No LDS, no scratch: operands are read
// straight from memory (t is read once per 64 output columns: once for A <= 7; the weights and G stay in L1 / L2).
// A wave owns a 32-voxel tile of one (level, scene); tiles are numbered level-major over all levels, start[k] = first tile of level k.
#include "levels4.hpp"
#include "mfma32.hpp"         // MM<T> (the operand fragments of one contraction step), acc_row, acc_zero, Out4<T>
#include "kernels.hpp"

namespace {

constexpr int HEAD_MAX_A = 32;
constexpr int HEAD_DW_MAX_BLOCKS = 1024;
constexpr long HEAD_DW_WS_FLOATS = 16L << 20;          // partial sums of the weight-gradient pass: at most 64 MiB

struct HeadGeom {
  int L, N, Cin, A, C, J, relu, total;                 // J = A (1 + C); total = wave tiles of all levels
  int V[4], tiles[4], start[4];                        // voxels per scene, 32-voxel tiles per scene, first tile; entries past L repeat `total` in start
};

bool make_head_geom(int nlevels, const int* vox, int N, int Cin, int A, int C, int relu, HeadGeom& g) {
  if (nlevels < 1 || nlevels > 4 || !vox || N < 1 || Cin < 8 || Cin % 8 || Cin > 8192 || A < 1 || A > HEAD_MAX_A || (C != 6 && C != 8)) return true;
  g.L = nlevels; g.N = N; g.Cin = Cin; g.A = A; g.C = C; g.J = A * (1 + C); g.relu = relu ? 1 : 0;
  long total = 0;
  for (int k = 0; k < 4; ++k) {
    if (k < nlevels) {
      if (vox[k] < 1 || (long)vox[k] * N > (1L << 30)) return true;
      g.V[k] = vox[k]; g.tiles[k] = (vox[k] + 31) / 32; g.start[k] = (int)total;
      total += (long)g.tiles[k] * N;
      if (total > (1L << 30)) return true;
    } else {
      g.V[k] = g.V[nlevels - 1]; g.tiles[k] = g.tiles[nlevels - 1]; g.start[k] = 0x7fffffff;
    }
  }
  g.total = (int)total;
  return false;
}

struct TileAt { int k, n, v0, V; };
__device__ __forceinline__ TileAt head_tile(const HeadGeom& g, int wt) {
  TileAt q;
  q.k = (wt >= g.start[1]) + (wt >= g.start[2]) + (wt >= g.start[3]);
  const int rem = wt - pick4(g.start, q.k), tl = pick4(g.tiles, q.k);
  q.n = rem / tl; q.v0 = (rem - q.n * tl) * 32; q.V = pick4(g.V, q.k);
  return q;
}

// ---- forward ----------------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void head_out_fwd_kernel(HeadGeom g, Ptr4<const T> t, const T* __restrict__ wc, const T* __restrict__ wb, const float* __restrict__ bc,
                                                           const float* __restrict__ bb, Ptr4<float> obj, Ptr4<float> reg) {
  typedef MM<T> M;
  constexpr int E = M::E;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wt >= g.total) return;
  const TileAt q = head_tile(g, wt);
  const int Cin = g.Cin, A = g.A, J = g.J, V = q.V;
  const int v = q.v0 + r;
  const bool vin = v < V;
  const T* __restrict__ trow = pick4(t.p, q.k) + ((long)q.n * V + (vin ? v : 0)) * Cin;
  float* __restrict__ po = pick4(obj.p, q.k) + (long)q.n * A * V;
  float* __restrict__ pr = pick4(reg.p, q.k) + (long)q.n * (J - A) * V;
  for (int j0 = 0; j0 < J; j0 += 64) {
    const bool two = j0 + 32 < J;                       // wave-uniform
    const int ja = j0 + r, jb = j0 + 32 + r;
    const T* __restrict__ wa = ja < A ? wc + (long)ja * Cin : wb + (long)(ja < J ? ja - A : 0) * Cin;
    const T* __restrict__ wq = jb < A ? wc + (long)jb * Cin : wb + (long)(jb < J ? jb - A : 0) * Cin;
    f32x16 acc0 = acc_zero(), acc1 = acc_zero();
    for (int k0 = 0; k0 < Cin; k0 += 2 * E) {
      const int kk = k0 + E * h;
      const bool kin = kk < Cin;                        // Cin is a multiple of 8: a lane's chunk is inside or outside as a whole
      typename M::Exact b = (vin && kin) ? M::load16(trow + kk) : M::zero();
      if (g.relu) M::relu(b);
      const typename M::Exact a0 = (ja < J && kin) ? M::load16(wa + kk) : M::zero();
      M::mma(acc0, a0, b);
      if (two) {
        const typename M::Exact a1 = (jb < J && kin) ? M::load16(wq + kk) : M::zero();
        M::mma(acc1, a1, b);
      }
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int j = j0 + acc_row(i, h);
      if (vin && j < J) {
        if (j < A) po[(long)j * V + v] = acc0[i] + bc[j];
        else pr[(long)(j - A) * V + v] = acc0[i] + bb[j - A];
      }
    }
    if (two) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = j0 + 32 + acc_row(i, h);
        if (vin && j < J) {
          if (j < A) po[(long)j * V + v] = acc1[i] + bc[j];
          else pr[(long)(j - A) * V + v] = acc1[i] + bb[j - A];
        }
      }
    }
  }
}

// ---- backward: dt -----------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void head_out_dt_kernel(HeadGeom g, Ptr4<const T> t, const T* __restrict__ wc, const T* __restrict__ wb, Ptr4<const float> gobj,
                                                          Ptr4<const float> greg, Ptr4<T> dt) {
  typedef MM<T> M;
  constexpr int E = M::E;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wt = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6));
  if (wt >= g.total) return;
  const TileAt q = head_tile(g, wt);
  const int Cin = g.Cin, A = g.A, J = g.J, V = q.V;
  const int v = q.v0 + r;
  const bool vin = v < V;
  const float* __restrict__ go = pick4(gobj.p, q.k) + (long)q.n * A * V + (vin ? v : 0);
  const float* __restrict__ gr = pick4(greg.p, q.k) + (long)q.n * (J - A) * V + (vin ? v : 0);
  const long row = ((long)q.n * V + (vin ? v : 0)) * Cin;
  const T* __restrict__ trow = pick4(t.p, q.k) + row;
  T* __restrict__ drow = pick4(dt.p, q.k) + row;
  for (int c0 = 0; c0 < Cin; c0 += 64) {
    const bool two = c0 + 32 < Cin;
    const int ca = c0 + r, cb = c0 + 32 + r;
    f32x16 acc0 = acc_zero(), acc1 = acc_zero();
    for (int j0 = 0; j0 < J; j0 += 2 * E) {
      typename M::Wide b = M::wzero();
      typename M::Exact a0 = M::zero(), a1 = M::zero();
      ForE<0, E>::run([&](auto I) {
        const int j = j0 + E * h + decltype(I)::value;
        if (j < J) {
          const T* __restrict__ wrow = j < A ? wc + (long)j * Cin : wb + (long)(j - A) * Cin;
          if (vin) M::template setw<decltype(I)::value>(b, j < A ? go[(long)j * V] : gr[(long)(j - A) * V]);
          if (ca < Cin) M::template set<decltype(I)::value>(a0, wrow[ca], false);
          if (two && cb < Cin) M::template set<decltype(I)::value>(a1, wrow[cb], false);
        }
      });
      M::mma_wb(acc0, a0, b);
      if (two) M::mma_wb(acc1, a1, b);
    }
    if (vin) {
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const int c = c0 + 8 * s + 4 * h;               // registers 4 s .. 4 s + 3: four consecutive channels
        if (c < Cin) Out4<T>::mask_store(drow + c, trow + c, g.relu != 0, acc0[4 * s], acc0[4 * s + 1], acc0[4 * s + 2], acc0[4 * s + 3]);
      }
      if (two) {
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const int c = c0 + 32 + 8 * s + 4 * h;
          if (c < Cin) Out4<T>::mask_store(drow + c, trow + c, g.relu != 0, acc1[4 * s], acc1[4 * s + 1], acc1[4 * s + 2], acc1[4 * s + 3]);
        }
      }
    }
  }
}

// ---- backward: weight and bias gradients ----------------------------------------------------------------------------------------------------------
// Workgroup b sums the tiles [b total / nb, (b + 1) total / nb) into partial b, a [J][Cin + 1] image whose last column holds the column sums of G (a tile of
// ones in place of t).  The output tiles, pairs of 32 columns x 32 channels, go round the 4 waves; every wave walks all the workgroup's voxels for each.
template <typename T>
__global__ __launch_bounds__(256) void head_out_dw_kernel(HeadGeom g, Ptr4<const T> t, Ptr4<const float> gobj, Ptr4<const float> greg, float* __restrict__ partials) {
  typedef MM<T> M;
  constexpr int E = M::E;
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int nb = gridDim.x, b = blockIdx.x;
  const int tb = (int)((long)b * g.total / nb), te = (int)((long)(b + 1) * g.total / nb);
  const int Cin = g.Cin, A = g.A, J = g.J, Cs = Cin + 1;
  const int nct = (Cin + 31) / 32, njp = (J + 63) / 64;
  float* __restrict__ P = partials + (long)b * J * Cs;
  for (int og = wave; og < njp * (nct + 1); og += 4) {
    const int jp = og / (nct + 1), ct = og - jp * (nct + 1);
    const bool ones = ct == nct;                        // the bias column
    const int j0 = jp * 64, c = ct * 32 + r;
    const bool two = j0 + 32 < J;
    const int ja = j0 + r, jb = j0 + 32 + r;
    f32x16 acc0 = acc_zero(), acc1 = acc_zero();
    for (int wt = tb; wt < te; ++wt) {
      const TileAt q = head_tile(g, wt);
      const int V = q.V;
      const float* __restrict__ ga = (ja < A ? pick4(gobj.p, q.k) + ((long)q.n * A + ja) * V : pick4(greg.p, q.k) + ((long)q.n * (J - A) + (ja < J ? ja - A : 0)) * V);
      const float* __restrict__ gb = (jb < A ? pick4(gobj.p, q.k) + ((long)q.n * A + jb) * V : pick4(greg.p, q.k) + ((long)q.n * (J - A) + (jb < J ? jb - A : 0)) * V);
      const T* __restrict__ tp = pick4(t.p, q.k) + (long)q.n * V * Cin + (c < Cin ? c : 0);
#pragma unroll
      for (int s = 0; s < 32; s += 2 * E) {
        typename M::Wide a0 = M::wzero(), a1 = M::wzero();
        typename M::Exact bf = M::zero();
        ForE<0, E>::run([&](auto I) {
          const int v = q.v0 + s + E * h + decltype(I)::value;
          if (v < V) {
            if (ja < J) M::template setw<decltype(I)::value>(a0, ga[v]);
            if (two && jb < J) M::template setw<decltype(I)::value>(a1, gb[v]);
            if (ones) M::template set<decltype(I)::value>(bf, from_f<T>(1.f), false);
            else if (c < Cin) M::template set<decltype(I)::value>(bf, tp[(long)v * Cin], g.relu != 0);
          }
        });
        M::mma_wa(acc0, a0, bf);
        if (two) M::mma_wa(acc1, a1, bf);
      }
    }
    const int col = ones ? (r == 0 ? Cin : -1) : (c < Cin ? c : -1);
    if (col >= 0) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int j = j0 + acc_row(i, h);
        if (j < J) P[(long)j * Cs + col] = acc0[i];
        if (two && j + 32 < J) P[(long)(j + 32) * Cs + col] = acc1[i];
      }
    }
  }
}

__global__ __launch_bounds__(256) void head_out_red_kernel(int nb, int Cin, int A, int J, const float* __restrict__ partials, float* __restrict__ dwc, float* __restrict__ dwb,
                                                           float* __restrict__ dbc, float* __restrict__ dbb) {
  const int Cs = Cin + 1, n = J * Cs;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int b = 0; b < nb; ++b) s += partials[(long)b * n + e];          // workgroup order: fixed
  const int j = e / Cs, c = e - j * Cs;
  if (c < Cin) {
    float* d = j < A ? dwc + (long)j * Cin + c : dwb + (long)(j - A) * Cin + c;
    *d += s;
  } else {
    float* d = j < A ? dbc + j : dbb + (j - A);
    *d += s;
  }
}

// ---- ReLU between the convolutions ------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void relu_kernel(T* __restrict__ x, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float v[8];
    Vec8<T>::load(x + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = v[e] <= 0.f ? 0.f : v[e];          // -0 -> +0; a NaN stays
    Vec8<T>::store(x + i * 8, v);
  }
}
template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(T* __restrict__ dy, const T* __restrict__ y, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    float d[8], v[8];
    Vec8<T>::load(dy + i * 8, d);
    Vec8<T>::load(y + i * 8, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) d[e] = v[e] > 0.f ? d[e] : 0.f;
    Vec8<T>::store(dy + i * 8, d);
  }
}

int dw_blocks(const HeadGeom& g) {
  long nb = g.total < HEAD_DW_MAX_BLOCKS ? g.total : HEAD_DW_MAX_BLOCKS;
  const long per = (long)g.J * (g.Cin + 1);
  if (nb * per > HEAD_DW_WS_FLOATS) nb = HEAD_DW_WS_FLOATS / per;
  return nb < 1 ? 1 : (int)nb;
}

}  // namespace

long k_rpn_head_bwd_ws_floats(int nlevels, const int* vox, int N, int Cin, int A, int C) {
  HeadGeom g;
  if (make_head_geom(nlevels, vox, N, Cin, A, C, 0, g)) return -1;
  return (long)dw_blocks(g) * g.J * (g.Cin + 1);
}

int k_rpn_head_out_fwd(int dt, int nlevels, const int* vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box, const float* b_cls,
                       const float* b_box, float* const* obj, float* const* reg, hipStream_t st) {
  HeadGeom g;
  if (make_head_geom(nlevels, vox, N, Cin, A, C, relu, g) || !all_set(nlevels, t) || !all_set(nlevels, obj) || !all_set(nlevels, reg)) return -4;
  const Ptr4<float> O = make_ptrs<float>(nlevels, obj), R = make_ptrs<float>(nlevels, reg);
  const dim3 grid((unsigned)((g.total + 3) / 4));
  if (dt == NMH_DT_BF16)
    hipLaunchKernelGGL(head_out_fwd_kernel<bf16_t>, grid, dim3(256), 0, st, g, make_ptrs<const bf16_t>(nlevels, (const bf16_t* const*)t), (const bf16_t*)w_cls, (const bf16_t*)w_box, b_cls,
                       b_box, O, R);
  else if (dt == NMH_DT_F32)
    hipLaunchKernelGGL(head_out_fwd_kernel<float>, grid, dim3(256), 0, st, g, make_ptrs<const float>(nlevels, (const float* const*)t), (const float*)w_cls, (const float*)w_box, b_cls, b_box,
                       O, R);
  else return -1;
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_rpn_head_out_bwd(int dt, int nlevels, const int* vox, int N, int Cin, int A, int C, int relu, const void* const* t, const void* w_cls, const void* w_box,
                       const float* const* g_obj, const float* const* g_reg, void* const* dt_out, float* partials, float* dw_cls, float* dw_box, float* db_cls, float* db_box,
                       hipStream_t st) {
  HeadGeom g;
  if (make_head_geom(nlevels, vox, N, Cin, A, C, relu, g) || !all_set(nlevels, t) || !all_set(nlevels, g_obj) || !all_set(nlevels, g_reg) || !all_set(nlevels, dt_out)) return -4;
  if (dt != NMH_DT_BF16 && dt != NMH_DT_F32) return -1;
  const Ptr4<const float> GO = make_ptrs<const float>(nlevels, g_obj), GR = make_ptrs<const float>(nlevels, g_reg);
  const dim3 grid((unsigned)((g.total + 3) / 4));
  const int nb = dw_blocks(g);
  if (dt == NMH_DT_BF16) {
    const Ptr4<const bf16_t> T = make_ptrs<const bf16_t>(nlevels, (const bf16_t* const*)t);
    hipLaunchKernelGGL(head_out_dt_kernel<bf16_t>, grid, dim3(256), 0, st, g, T, (const bf16_t*)w_cls, (const bf16_t*)w_box, GO, GR, make_ptrs<bf16_t>(nlevels, (bf16_t* const*)dt_out));
    NMH_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_out_dw_kernel<bf16_t>, dim3(nb), dim3(256), 0, st, g, T, GO, GR, partials);
  } else {
    const Ptr4<const float> T = make_ptrs<const float>(nlevels, (const float* const*)t);
    hipLaunchKernelGGL(head_out_dt_kernel<float>, grid, dim3(256), 0, st, g, T, (const float*)w_cls, (const float*)w_box, GO, GR, make_ptrs<float>(nlevels, (float* const*)dt_out));
    NMH_CHECK_LAUNCH();
    hipLaunchKernelGGL(head_out_dw_kernel<float>, dim3(nb), dim3(256), 0, st, g, T, GO, GR, partials);
  }
  NMH_CHECK_LAUNCH();
  hipLaunchKernelGGL(head_out_red_kernel, dim3((unsigned)((g.J * (g.Cin + 1) + 255) / 256)), dim3(256), 0, st, nb, g.Cin, g.A, g.J, partials, dw_cls, dw_box, db_cls, db_box);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_relu_(int dt, void* x, long n, hipStream_t st) {
  if (n <= 0) return 0;
  if (n % 8) return -2;
  long nb = (n / 8 + 255) / 256;
  if (nb > 8192) nb = 8192;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(relu_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (bf16_t*)x, n / 8);
  else if (dt == NMH_DT_F32) hipLaunchKernelGGL(relu_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (float*)x, n / 8);
  else return -1;
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_relu_bwd_(int dt, void* dy, const void* y, long n, hipStream_t st) {
  if (n <= 0) return 0;
  if (n % 8) return -2;
  long nb = (n / 8 + 255) / 256;
  if (nb > 8192) nb = 8192;
  if (dt == NMH_DT_BF16) hipLaunchKernelGGL(relu_bwd_kernel<bf16_t>, dim3((unsigned)nb), dim3(256), 0, st, (bf16_t*)dy, (const bf16_t*)y, n / 8);
  else if (dt == NMH_DT_F32) hipLaunchKernelGGL(relu_bwd_kernel<float>, dim3((unsigned)nb), dim3(256), 0, st, (float*)dy, (const float*)y, n / 8);
  else return -1;
  NMH_CHECK_LAUNCH();
  return 0;
}
