// Per-level plumbing of the detector kernels (fcos.hip, fcos_post.hip, rpn.hip, rpn_post.hip, roi_head.hip, rpn_head.hip): up to four levels travel by value
// as arrays of 4, the unused entries repeating the last level so that every entry is valid; and the map from a workgroup to its level in a launch whose
// workgroups are laid out level after level (fcos_where in fcos.hip, rpn_where in rpn_geom.hpp, the NMS mask kernel of rpn_post.hip).
#pragma once
#include "common.hpp"

namespace {

template <typename T> struct Ptr4 { T* p[4]; };
// a[i] without a dynamically indexed kernel-argument array (which would go to scratch)
template <typename T> __device__ __forceinline__ T pick4(const T (&a)[4], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3])); }

// the level of workgroup b when level k's workgroups start at blk0[k] (blk0[0] = 0, ascending): the largest k < L with b >= blk0[k]
__device__ __forceinline__ int level_of_block(const int (&blk0)[4], int L, int b) {
  int lvl = 0;
#pragma unroll
  for (int k = 1; k < 4; ++k) if (k < L && b >= blk0[k]) lvl = k;
  return lvl;
}
// workgroup blockIdx.x -> (level, scene, item) when a level holds per[k] workgroups of 256 items for each scene, scene after scene
struct LevelItem { int lvl, scene, i; };
__device__ __forceinline__ LevelItem level_item(const int (&blk0)[4], const int (&per)[4], int L) {
  LevelItem q;
  q.lvl = level_of_block(blk0, L, blockIdx.x);
  const int b = (int)blockIdx.x - pick4(blk0, q.lvl), n = pick4(per, q.lvl);
  q.scene = b / n;
  q.i = (b - q.scene * n) * 256 + (int)threadIdx.x;
  return q;
}

// tab: nlevels pointers, or null for an optional argument (all entries null)
template <typename T> Ptr4<T> make_ptrs(int nlevels, T* const* tab) {
  Ptr4<T> r;
  for (int k = 0; k < 4; ++k) r.p[k] = tab ? tab[k < nlevels ? k : nlevels - 1] : nullptr;
  return r;
}
template <typename T> bool all_set(int nlevels, T* const* tab) {
  if (!tab) return false;
  for (int k = 0; k < nlevels; ++k) if (!tab[k]) return false;
  return true;
}

}  // namespace
