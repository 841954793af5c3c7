// Per-level kernel arguments of the detector kernels (fcos.hip, fcos_post.hip, rpn.hip, rpn_post.hip): up to four levels travel by value as arrays of 4, the
// unused entries repeating the last level so that every entry is valid.
#pragma once
#include "common.hpp"

namespace {

template <typename T> struct Ptr4 { T* p[4]; };
// a[i] without a dynamically indexed kernel-argument array (which would go to scratch)
template <typename T> __device__ __forceinline__ T pick4(const T (&a)[4], int i) { return i == 0 ? a[0] : (i == 1 ? a[1] : (i == 2 ? a[2] : a[3])); }

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
