// Box walk of the decoder tail (csrc/norm.hip: tail_fwd_coarse_kernel<true>, tail_bwd_kernel<.., BOX = true>): a sample's target is zero outside
// its extents, so d(pred) is exactly zero there and the tail forward need not visit -- nor the tail backward read -- the padding.  The valid box of a
// sample is Ez x Ey x Ex coarse cells (E = ceil(extent / 4), at most gd = R / 4 <= 64); box cell k maps to (zc, yc, xc) = unravel(k; Ey Ex, Ex).
// Plain integer code for host and device: tests/test_tail_box_cpu.py compiles it for the host and checks it against divmod.
#pragma once
#if defined(__HIPCC__) || defined(__CUDACC__)
#define TAIL_BOX_HD __host__ __device__
#else
#define TAIL_BOX_HD
#endif

struct TailBox {
  unsigned Ez, Ey, Ex;   // cells per axis
  unsigned n;            // Ez * Ey * Ex (0: nothing to walk)
  unsigned m1, m2;       // ceil(2^30 / Ex), ceil(2^30 / (Ey Ex))
};

TAIL_BOX_HD inline unsigned tail_box_mulhi(unsigned a, unsigned b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (unsigned)(((unsigned long long)a * b) >> 32);
#endif
}
// ceil(2^30 / d) for 1 <= d <= 4096: fits 32 bits for d = 1 too (2^32 / d does not)
TAIL_BOX_HD inline unsigned tail_box_magic(unsigned d) { return ((1u << 30) + d - 1u) / d; }
// k / d for k < 2^18 (64^3), 1 <= d <= 4096, m = tail_box_magic(d): floor(4 k m / 2^32) = floor(k m / 2^30); with m d = 2^30 + e, e < d <= 2^12, the
// result is exact while k e < 2^30
TAIL_BOX_HD inline unsigned tail_box_div(unsigned k, unsigned m) { return tail_box_mulhi(k << 2, m); }

// extents (valid voxels per axis, any int) -> the box in cells of a grid of gd^3 cells, gd <= 64
TAIL_BOX_HD inline TailBox tail_box_make(int e0, int e1, int e2, int gd) {
  TailBox t;
  const int c0 = (e0 + 3) >> 2, c1 = (e1 + 3) >> 2, c2 = (e2 + 3) >> 2;
  t.Ez = (unsigned)(e0 <= 0 ? 0 : (c0 < gd ? c0 : gd));
  t.Ey = (unsigned)(e1 <= 0 ? 0 : (c1 < gd ? c1 : gd));
  t.Ex = (unsigned)(e2 <= 0 ? 0 : (c2 < gd ? c2 : gd));
  t.n = t.Ez * t.Ey * t.Ex;
  t.m1 = tail_box_magic(t.Ex ? t.Ex : 1u);
  t.m2 = tail_box_magic(t.n ? t.Ey * t.Ex : 1u);
  return t;
}
// box cell k < t.n -> its coordinates in cells
TAIL_BOX_HD inline void tail_box_unravel(const TailBox& t, unsigned k, unsigned& zc, unsigned& yc, unsigned& xc) {
  zc = tail_box_div(k, t.m2);
  const unsigned rem = k - zc * (t.Ey * t.Ex);
  yc = tail_box_div(rem, t.m1);
  xc = rem - yc * t.Ex;
}
// The share of workgroup `blk` of `nblk` in a box of n cells: [cbeg, cend), whole 64-cell trips (one 16-cell step of each of the four wave pairs) except the last
// of the box.  Empty (cbeg == cend) for the workgroups past the end of a small box.
TAIL_BOX_HD inline void tail_box_range(unsigned n, unsigned nblk, unsigned blk, unsigned& cbeg, unsigned& cend) {
  const unsigned per = ((n + nblk - 1u) / nblk + 63u) / 64u * 64u;
  cbeg = blk * per < n ? blk * per : n;
  cend = cbeg + per < n ? cbeg + per : n;
}
// voxel v < R^3 (R <= 256, mR = ceil(2^32 / R): exact for v < 2^24) inside the box of (bz, by, bx) = 4 (Ez, Ey, Ex) voxels
TAIL_BOX_HD inline bool tail_box_has_voxel(unsigned v, unsigned R, unsigned mR, unsigned bz, unsigned by, unsigned bx) {
  const unsigned row = tail_box_mulhi(v, mR), x = v - row * R, z = tail_box_mulhi(row, mR), y = row - z * R;
  return z < bz && y < by && x < bx;
}
