// The 2-D projection regression term on rows of boxes, as an operator of its own (the fused losses of rpn.hip and fcos.hip apply the same device code
// of proj2d.hpp to their decoded positives): compute_2d_projection_loss of the reference's detectors (nerf_rpn/model/rpn.py:421-453,
// fcos/loss.py:447-475) before any weighting and normalisation.
//   proj2d_fwd   pred, target [n][6] (x0, y0, z0, x1, y1, z1) or [n][7] (x, y, z, w, l, h, theta) -> terms [n] = T of every row (proj2d.hpp);
//   proj2d_bwd   dpred [n][6|7] = g_terms[row] dT / dpred; the target has no gradient.
// One lane per row, fp32, no LDS, no atomics; every element of the outputs is written.
#include "common.hpp"
#include "kernels.hpp"
#include "proj2d.hpp"

namespace {

template <int NC>
__global__ __launch_bounds__(256) void proj2d_fwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, long n, Proj2dCams cams, float* __restrict__ terms) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (NC == 7) {
    terms[i] = proj2d_term(obb_load(pred + i * 7), obb_load(target + i * 7), cams);
  } else {
    float p[6], t[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { p[k] = pred[i * 6 + k]; t[k] = target[i * 6 + k]; }
    terms[i] = proj2d_term(p, t, cams);
  }
}

template <int NC>
__global__ __launch_bounds__(256) void proj2d_bwd_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ g_terms, long n, Proj2dCams cams,
                                                         float* __restrict__ dpred) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = g_terms[i];
  float* __restrict__ d = dpred + i * NC;
  if (NC == 7) {
    BoxGrad g;
    proj2d_term_grad(obb_load(pred + i * 7), obb_load(target + i * 7), cams, g);
    d[0] = s * g.x; d[1] = s * g.y; d[2] = s * g.z; d[3] = s * g.w; d[4] = s * g.l; d[5] = s * g.h; d[6] = s * g.t;
  } else {
    float p[6], t[6], g[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { p[k] = pred[i * 6 + k]; t[k] = target[i * 6 + k]; }
    proj2d_term_grad(p, t, cams, g);
#pragma unroll
    for (int k = 0; k < 6; ++k) d[k] = s * g[k];
  }
}

bool bad_rows(long n, int ncols) { return n <= 0 || (n + 255) / 256 >= (1L << 31) || (ncols != 6 && ncols != 7); }

}  // namespace

int k_proj2d_fwd(const float* pred, const float* target, long n, int ncols, const float* cams, float* terms, hipStream_t st) {
  if (bad_rows(n, ncols) || !cams) return -4;
  Proj2dCams C;
  for (int k = 0; k < 48; ++k) C.m[k / 12][k % 12] = cams[k];
  const dim3 grid((unsigned)((n + 255) / 256));
  if (ncols == 7) hipLaunchKernelGGL(proj2d_fwd_kernel<7>, grid, dim3(256), 0, st, pred, target, n, C, terms);
  else hipLaunchKernelGGL(proj2d_fwd_kernel<6>, grid, dim3(256), 0, st, pred, target, n, C, terms);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_proj2d_bwd(const float* pred, const float* target, const float* g_terms, long n, int ncols, const float* cams, float* dpred, hipStream_t st) {
  if (bad_rows(n, ncols) || !cams) return -4;
  Proj2dCams C;
  for (int k = 0; k < 48; ++k) C.m[k / 12][k % 12] = cams[k];
  const dim3 grid((unsigned)((n + 255) / 256));
  if (ncols == 7) hipLaunchKernelGGL(proj2d_bwd_kernel<7>, grid, dim3(256), 0, st, pred, target, g_terms, n, C, dpred);
  else hipLaunchKernelGGL(proj2d_bwd_kernel<6>, grid, dim3(256), 0, st, pred, target, g_terms, n, C, dpred);
  NMH_CHECK_LAUNCH();
  return 0;
}

void k_proj2d_cameras(float res, float* cams) {
  Proj2dCams C;
  proj2d_make_cams((double)res, C);
  for (int k = 0; k < 48; ++k) cams[k] = C.m[k / 12][k % 12];
}
