"""csrc/tail_box.hpp, the integer code of the decoder tail's box walk, compiled for the host and checked against plain division:
the magic-number division behind the unravel, the unravel of a box cell, the workgroups' ranges, and the voxel-in-box test of the backward."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER_DIR = os.path.join(ROOT, "nerf-mae_amd", "csrc")

SHIM = r"""
#include "tail_box.hpp"
extern "C" {
// every divisor d in [d_lo, d_hi] against every k < kmax: the number of wrong quotients
long sweep_div(unsigned d_lo, unsigned d_hi, unsigned kmax) {
  long bad = 0;
  for (unsigned d = d_lo; d <= d_hi; ++d) {
    const unsigned m = tail_box_magic(d);
    for (unsigned k = 0; k < kmax; ++k) bad += tail_box_div(k, m) != k / d;
  }
  return bad;
}
// every cell of every box Ez x Ey x Ex with the three in [lo, hi] (step st), given as extents 4 E - sub: the number of wrong coordinates or counts
long sweep_boxes(int lo, int hi, int st, int sub, int gd) {
  long bad = 0;
  for (int ez = lo; ez <= hi; ez += st)
    for (int ey = lo; ey <= hi; ey += st)
      for (int ex = lo; ex <= hi; ex += st) {
        const TailBox t = tail_box_make(4 * ez - sub, 4 * ey - sub, 4 * ex - sub, gd);
        bad += t.Ez != (unsigned)ez || t.Ey != (unsigned)ey || t.Ex != (unsigned)ex || t.n != (unsigned)(ez * ey * ex);
        for (unsigned k = 0; k < t.n; ++k) {
          unsigned z, y, x;
          tail_box_unravel(t, k, z, y, x);
          bad += z != k / (unsigned)(ey * ex) || y != k % (unsigned)(ey * ex) / (unsigned)ex || x != k % (unsigned)ex;
        }
      }
  return bad;
}
void make(int e0, int e1, int e2, int gd, unsigned* out) {
  const TailBox t = tail_box_make(e0, e1, e2, gd);
  out[0] = t.Ez; out[1] = t.Ey; out[2] = t.Ex; out[3] = t.n;
}
void range(unsigned n, unsigned nblk, unsigned blk, unsigned* out) { tail_box_range(n, nblk, blk, out[0], out[1]); }
// every voxel of an R^3 grid against the box (bz, by, bx): the number of wrong answers
long sweep_voxels(unsigned R, unsigned bz, unsigned by, unsigned bx) {
  const unsigned mR = (unsigned)((0x100000000ULL + R - 1) / R);
  long bad = 0;
  for (unsigned z = 0; z < R; ++z)
    for (unsigned y = 0; y < R; ++y)
      for (unsigned x = 0; x < R; ++x) bad += tail_box_has_voxel((z * R + y) * R + x, R, mR, bz, by, bx) != (z < bz && y < by && x < bx);
  return bad;
}
}
"""


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler to build the tail_box.hpp shim")
    d = tmp_path_factory.mktemp("tail_box")
    src, so = os.path.join(d, "shim.cpp"), os.path.join(d, "shim.so")
    with open(src, "w") as f:
        f.write(SHIM)
    subprocess.run([cxx, "-O2", "-std=c++17", "-shared", "-fPIC", "-I", HEADER_DIR, src, "-o", so], check=True)
    L = ctypes.CDLL(so)
    for name in ("sweep_div", "sweep_boxes", "sweep_voxels"):
        getattr(L, name).restype = ctypes.c_long
    L.sweep_div.argtypes = [ctypes.c_uint] * 3
    L.sweep_boxes.argtypes = [ctypes.c_int] * 5
    L.sweep_voxels.argtypes = [ctypes.c_uint] * 4
    return L


def test_magic_division_is_exact_for_every_divisor_and_cell_index(shim):
    """the divisors the unravel meets at R <= 256 are Ey Ex <= 4096 (on k < 64^3) and Ex <= 64 (on the remainder < 4096): both ranges exhaustively, the first over
    every k < 64^3 -- which covers every box Ez, Ey, Ex in [1, 64] and every cell of it, since the unravel is these two divisions"""
    assert shim.sweep_div(1, 4096, 64 ** 3) == 0
    assert shim.sweep_div(1, 64, 4096) == 0


def test_unravel_agrees_with_divmod_on_whole_boxes(shim):
    # every box with edges 1 .. 16 and every cell of it, extents a multiple of 4 and not (4 E - 3 .. 4 E all round up to E cells)
    for sub in (0, 1, 3):
        assert shim.sweep_boxes(1, 16, 1, sub, 64) == 0
    # the large end: edges 40 .. 64 in steps of 3 (64 included), and the benchmark's boxes at 160^3
    assert shim.sweep_boxes(40, 64, 3, 2, 64) == 0
    out = (ctypes.c_uint * 4)()
    for ext, cells in (((160, 160, 160), (40, 40, 40)), ((160, 132, 96), (40, 33, 24)), ((120, 160, 144), (30, 40, 36)), ((3, 2, 1), (1, 1, 1)), ((25, 19, 31), (7, 5, 8))):
        shim.make(*ext, 40, out)
        assert tuple(out)[:3] == cells and out[3] == cells[0] * cells[1] * cells[2]
    # extents are clamped to the grid, and an empty extent gives an empty box
    shim.make(1000, 4, -5, 8, out)
    assert tuple(out) == (8, 1, 0, 0)


@pytest.mark.parametrize("n", [1, 15, 16, 63, 64, 65, 280, 512, 1728, 31680, 43200, 64000, 262144])
@pytest.mark.parametrize("nblk", [1, 2, 3, 16, 64])
def test_workgroup_ranges_tile_the_box(shim, n, nblk):
    out = (ctypes.c_uint * 2)()
    nxt = 0
    for blk in range(nblk):
        shim.range(n, nblk, blk, out)
        beg, end = out[0], out[1]
        assert beg == nxt and beg <= end <= n          # disjoint, in order, no gap: the union is [0, n)
        if end < n:
            assert (end - beg) % 64 == 0 and end > beg   # whole 64-cell trips, except for the range that ends the box
        assert beg % 64 == 0 or beg == n
        nxt = end
    assert nxt == n


def test_voxel_in_box_test_of_the_backward(shim):
    for R, box in ((32, (32, 32, 32)), (32, (28, 20, 32)), (48, (4, 4, 4)), (48, (44, 36, 48)), (160, (120, 160, 144)), (256, (256, 4, 252))):
        assert shim.sweep_voxels(R, *box) == 0
    assert shim.sweep_voxels(48, 0, 0, 0) == 0
