// Oriented 3-D box IoU / GIoU / DIoU losses and rotated NMS of the reference's downstream detectors, as gfx950 kernels:
//   cal_iou_3d / cal_giou_3d / cal_diou_3d (nerf_rpn/model/rotated_iou/oriented_iou_loss.py:82-148, over box_intersection_2d.py and
//     min_enclosing_box.py:25-166; called by fcos/loss.py:135-171 and rpn.py:143-156): obb_iou_fwd / obb_iou_bwd, one box pair per lane;
//   box_iou_3d (fcos/utils.py:229-255, utils.py): obb_iou_pairwise, the [N,M] matrix without the N x M x 7 repeat;
//   nms / batched_nms (fcos/utils.py:109-158): obb_nms_mask (suppression bit matrix) + obb_nms_scan (greedy walk on the device).
//
// Semantics.  A box is (x, y, z, w, l, h, theta) fp32, theta in RADIANS about the third axis (the RoIAlign op of rotated.hip takes
// degrees).  Its bird's-eye-view (BEV) rectangle has the corners of box2corners_th: local (+-w/2, +-l/2) in the order (+,+), (-,+), (-,-),
// (+,-), rotated counter-clockwise by theta, translated by (x, y).  For a pair:
//   inter2d   = area of the intersection of the two BEV rectangles
//   z_overlap = max(0, min(zmax1, zmax2) - max(zmin1, zmin2)),   zmax = z + h/2, zmin = z - h/2
//   inter3d   = inter2d * z_overlap,   u3d = w1 l1 h1 + w2 l2 h2 - inter3d,   iou3d = inter3d / u3d
//   z_range   = max(0, max(zmax1, zmax2) - min(zmin1, zmin2))
// Enclosing rectangle (w_c, h_c) of the eight BEV corners:
//   "aligned":  the axis-aligned extent (x extent, y extent);
//   "smallest": for every line through two of the eight corners except the four diagonals (24 candidates, in the order i < j of
//     min_enclosing_box.py:43-48), proj = extent of the eight corners along the line, dist = their extent across it; candidates with
//     proj * dist == 0 (or coincident points) are left out; the first candidate of minimum proj * dist gives (w_c, h_c) = (proj, dist).
//   GIoU: v_c = z_range w_c h_c,  loss = 1 - iou3d + (v_c - u3d) / v_c          (giou = 1 - loss is formed by the caller)
//   DIoU: loss = 1 - iou3d + d2 / c2,  d2 = |centre1 - centre2|^2 in 3-D,  c2 = w_c^2 + h_c^2 + z_range^2
// The 6-column form of the pairwise and NMS kernels is (x1, y1, z1, x2, y2, z2) with the closed form of _box_inter_union_3d
// (fcos/utils.py:285-297).
//
// Algorithm.  No vertex list exists anywhere, so there is no vertex count to bound and no per-lane array (nothing goes to scratch).
//   Area.  Box 1 is expressed in the frame of box 2, where box 2 is [-a, a] x [-b, b].  For a counter-clockwise polygon P,
//     area(P and box 2) = - sum over the edges of P of the integral of clamp(y, -b, b) dx over the part of the edge with |x| <= a
//     (per vertical line the slice of P is an interval, and its part inside [-b, b] is clamp(top) - clamp(bottom)).  On an edge the integrand
//     is piecewise linear with breaks where y crosses -b and b: three trapezoids, exact, no cancellation between terms of one edge.  Each
//     edge contributes on its own, so touching or coincident edges cannot be counted twice and nothing needs sorting.
//   Disjoint pairs.  The formula's terms cancel only to rounding, so a separating-axis test on the four edge normals (and, in the pairwise
//     and NMS kernels, first the z overlap and the BEV circumscribed circles) decides "no overlap" and gives exactly 0.
//   Area gradient.  The derivative of the intersection area under a motion of one box is the integral of the outward normal velocity over
//     the parts of THAT box's edges inside the other (no pass through the clipping).  Each edge of box 1 is clipped to box 2 in box 2's
//     frame (Liang-Barsky, closed), giving the part [t0, t1] of an edge of length L with outward normal n:
//       d/d(centre) += n (t1 - t0) L;   d/d(size along n) += (t1 - t0) L / 2;   d/d(theta) -= L^2 ((t1 - 1/2)^2 - (t0 - 1/2)^2) / 2
//     and the same with the roles exchanged for box 2.  A pair that the separating-axis test rejects gets exactly 0.
//   Enclosing rectangle gradient.  (w_c, h_c) of the winning candidate are differentiated by hand: to the two extreme corners along and
//     across the line, and through the line's direction to its two corners; corner gradients are then taken to (x, y, w, l, theta) of the
//     box the corner belongs to.  Which corner is extreme is found by unrolled compares on compile-time indices.
//   min / max of the z bounds split a gradient evenly on a tie, as torch.min / torch.max do.
// DEVIATIONS from the reference.  Two identical boxes give iou3d >= 1 - 1e-4 (the reference's vertex method can count touching corners
// twice and overflow its nine index slots there).  The reference's stabilisers (1e-8 in t and in the slope, 1e-14 under the root) are not
// reproduced; they move results by about 1e-8 relative.  For any input, non-finite values and non-positive sizes included, every kernel
// writes only its own outputs; the values for such input are unspecified.
//
// NMS.  Boxes arrive ordered by descending score.  The bit matrix (64-bit words, ceil(N/64) per row, upper triangle only) and the greedy walk are those
// of nms_bits.hpp; here a pair also needs equal categories when categories are given (an offset-coordinates trick is not valid for rotated boxes).
// Kept positions and their count are written to device memory; the host is not involved.
#include "common.hpp"
#include "kernels.hpp"
#include "nms_bits.hpp"

namespace {

template <int MODE>
__global__ __launch_bounds__(256) void obb_iou_fwd_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long n, float* __restrict__ iou, float* __restrict__ u3d,
                                                          float* __restrict__ zr, float* __restrict__ loss, float* __restrict__ wc, float* __restrict__ hc,
                                                          float* __restrict__ c1, float* __restrict__ c2) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const Obb A = obb_load(b1 + p * 7), B = obb_load(b2 + p * 7);
  const PairOut o = obb_pair(A, B);
  iou[p] = o.iou;
  if (u3d) u3d[p] = o.u3d;
  if (zr) zr[p] = o.zr;
  if (MODE == OBB_IOU && !c1 && !c2) return;
  float X[8], Y[8];
  obb_corners(A, X, Y, 0);
  obb_corners(B, X, Y, 4);
  if (c1) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { c1[p * 8 + 2 * k] = X[k]; c1[p * 8 + 2 * k + 1] = Y[k]; }
  }
  if (c2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) { c2[p * 8 + 2 * k] = X[4 + k]; c2[p * 8 + 2 * k + 1] = Y[4 + k]; }
  }
  if (MODE == OBB_IOU) return;
  Encl E;
  const float ls = obb_pair_loss<MODE>(A, B, o, X, Y, E);
  loss[p] = ls;
  if (wc) wc[p] = E.w;
  if (hc) hc[p] = E.h;
}

template <int MODE>
__global__ __launch_bounds__(256) void obb_iou_bwd_kernel(const float* __restrict__ b1, const float* __restrict__ b2, long n, const float* __restrict__ g_iou,
                                                          const float* __restrict__ g_u3d, const float* __restrict__ g_loss, int g_one, float* __restrict__ d1, float* __restrict__ d2) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const Obb A = obb_load(b1 + p * 7), B = obb_load(b2 + p * 7);
  // bit k of g_one: incoming gradient k is ONE value for every pair (the expanded gradient of a sum())
  const float gi_in = g_iou ? g_iou[(g_one & 1) ? 0 : p] : 0.f, gu_in = g_u3d ? g_u3d[(g_one & 2) ? 0 : p] : 0.f, gl = (MODE != OBB_IOU && g_loss) ? g_loss[(g_one & 4) ? 0 : p] : 0.f;
  BoxGrad ga, gb;
  obb_pair_grad<MODE>(A, B, gi_in, gu_in, gl, d2 != nullptr, ga, gb);
  if (d1) { float* q = d1 + p * 7; q[0] = ga.x; q[1] = ga.y; q[2] = ga.z; q[3] = ga.w; q[4] = ga.l; q[5] = ga.h; q[6] = ga.t; }
  if (d2) { float* q = d2 + p * 7; q[0] = gb.x; q[1] = gb.y; q[2] = gb.z; q[3] = gb.w; q[4] = gb.l; q[5] = gb.h; q[6] = gb.t; }
}

// ---- all pairs: tiles of 16 rows x 64 columns, both box tiles staged in LDS with their sin / cos taken once -------------------------
constexpr int PW_ROWS = 16, PW_COLS = 64;
template <bool AABB>
__global__ __launch_bounds__(256) void obb_iou_pairwise_kernel(const float* __restrict__ b1, const float* __restrict__ b2, int N, int M, float* __restrict__ iou) {
  __shared__ BoxTile rows[PW_ROWS], cols[PW_COLS];
  const int t = threadIdx.x;
  const long r0 = (long)blockIdx.y * PW_ROWS, c0 = (long)blockIdx.x * PW_COLS;
  if (t < PW_COLS) stage_box<AABB>(b2, c0 + t, M, cols[t]);
  else if (t < PW_COLS + PW_ROWS) stage_box<AABB>(b1, r0 + (t - PW_COLS), N, rows[t - PW_COLS]);
  __syncthreads();
  const int c = t & (PW_COLS - 1);
  if (c0 + c >= M) return;
  const BoxTile bc = cols[c];
#pragma unroll 1
  for (int r = t >> 6; r < PW_ROWS; r += 4) {
    if (r0 + r >= N) break;
    iou[(r0 + r) * M + c0 + c] = tile_iou<AABB>(rows[r], bc);
  }
}

// ---- NMS: word (i, j) of the suppression matrix per wave, 64 rows x 64 columns per block ------------------------------------------------
template <bool AABB>
__global__ __launch_bounds__(256) void obb_nms_mask_kernel(const float* __restrict__ boxes, const int* __restrict__ cat, int N, float thr, unsigned long long* __restrict__ mask) {
  __shared__ BoxTile rows[64], cols[64];
  __shared__ int rcat[64];
  const int t = threadIdx.x, nw = (N + 63) >> 6;
  int by, j;
  tri_block(blockIdx.x, nw, by, j);
  const int r0 = by * 64, c0 = j * 64;
  if (t < 64) stage_box<AABB>(boxes, c0 + t, N, cols[t]);
  else if (t < 128) { stage_box<AABB>(boxes, r0 + (t - 64), N, rows[t - 64]); rcat[t - 64] = (cat && r0 + (t - 64) < N) ? cat[r0 + (t - 64)] : 0; }
  __syncthreads();
  nms_mask_tile<AABB>(rows, cols, r0, c0, j, N, thr, mask, nw, rcat, cat);       // no early exit: every launched word is written
}

// one workgroup; N <= 16384 (256 words of removed-set)
__global__ __launch_bounds__(256) void obb_nms_scan_kernel(const unsigned long long* __restrict__ mask, int N, int* __restrict__ keep, int* __restrict__ count) {
  __shared__ unsigned long long removed[256], diag[64];
  const int cnt = nms_greedy_walk(mask, (N + 63) >> 6, N, keep, removed, diag);
  if (threadIdx.x == 0) *count = cnt;
}

template <int MODE>
void launch_fwd(const float* b1, const float* b2, long n, float* iou, float* u3d, float* zr, float* loss, float* wc, float* hc, float* c1, float* c2, hipStream_t st) {
  hipLaunchKernelGGL(obb_iou_fwd_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2);
}
template <int MODE>
void launch_bwd(const float* b1, const float* b2, long n, const float* gi, const float* gu, const float* gl, int g_one, float* d1, float* d2, hipStream_t st) {
  hipLaunchKernelGGL(obb_iou_bwd_kernel<MODE>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b1, b2, n, gi, gu, gl, g_one, d1, d2);
}

}  // namespace

int k_obb_iou_fwd(int mode, const float* b1, const float* b2, long n, float* iou, float* u3d, float* zr, float* loss, float* wc, float* hc, float* c1, float* c2, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  switch (mode) {
    case OBB_IOU: launch_fwd<OBB_IOU>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_GIOU_SMALLEST: launch_fwd<OBB_GIOU_SMALLEST>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_GIOU_ALIGNED: launch_fwd<OBB_GIOU_ALIGNED>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_DIOU_SMALLEST: launch_fwd<OBB_DIOU_SMALLEST>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    case OBB_DIOU_ALIGNED: launch_fwd<OBB_DIOU_ALIGNED>(b1, b2, n, iou, u3d, zr, loss, wc, hc, c1, c2, st); break;
    default: return -4;
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_iou_bwd(int mode, const float* b1, const float* b2, long n, const float* gi, const float* gu, const float* gl, int g_one, float* d1, float* d2, hipStream_t st) {
  if (n <= 0 || (n + 255) / 256 >= (1L << 31)) return -4;
  switch (mode) {
    case OBB_IOU: launch_bwd<OBB_IOU>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_GIOU_SMALLEST: launch_bwd<OBB_GIOU_SMALLEST>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_GIOU_ALIGNED: launch_bwd<OBB_GIOU_ALIGNED>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_DIOU_SMALLEST: launch_bwd<OBB_DIOU_SMALLEST>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    case OBB_DIOU_ALIGNED: launch_bwd<OBB_DIOU_ALIGNED>(b1, b2, n, gi, gu, gl, g_one, d1, d2, st); break;
    default: return -4;
  }
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_iou_pairwise(int ncols, const float* b1, const float* b2, int N, int M, float* iou, hipStream_t st) {
  if (N <= 0 || M <= 0 || (ncols != 6 && ncols != 7)) return -4;
  const long gy = ((long)N + PW_ROWS - 1) / PW_ROWS;
  if (gy > 65535) return -4;
  const dim3 grid((unsigned)((M + PW_COLS - 1) / PW_COLS), (unsigned)gy);
  if (ncols == 6) hipLaunchKernelGGL(obb_iou_pairwise_kernel<true>, grid, dim3(256), 0, st, b1, b2, N, M, iou);
  else hipLaunchKernelGGL(obb_iou_pairwise_kernel<false>, grid, dim3(256), 0, st, b1, b2, N, M, iou);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_nms_mask(int ncols, const float* boxes, const int* cat, int N, float thr, unsigned long long* mask, hipStream_t st) {
  if (N <= 0 || N > NMH_OBB_NMS_MAX || (ncols != 6 && ncols != 7)) return -4;
  const unsigned nw = (unsigned)((N + 63) / 64);
  if (ncols == 6) hipLaunchKernelGGL(obb_nms_mask_kernel<true>, dim3(nw * (nw + 1) / 2), dim3(256), 0, st, boxes, cat, N, thr, mask);
  else hipLaunchKernelGGL(obb_nms_mask_kernel<false>, dim3(nw * (nw + 1) / 2), dim3(256), 0, st, boxes, cat, N, thr, mask);
  NMH_CHECK_LAUNCH();
  return 0;
}

int k_obb_nms_scan(const unsigned long long* mask, int N, int* keep, int* count, hipStream_t st) {
  if (N <= 0 || N > NMH_OBB_NMS_MAX) return -4;
  hipLaunchKernelGGL(obb_nms_scan_kernel, dim3(1), dim3(256), 0, st, mask, N, keep, count);
  NMH_CHECK_LAUNCH();
  return 0;
}
