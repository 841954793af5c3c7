// Operand fragments of the 32x32 matrix-core kernels that read their operands straight from memory (rpn_head.hip, box_head.hip): no LDS staging, one
// 32 x 32 fp32 accumulator tile per wave.
//
// Fragment maps (v_mfma_f32_32x32x16_bf16, and v_mfma_f32_32x32x2_f32 for the exact fp32 path): lane l, r = l & 31, h = l >> 5.  bf16: element e = 0..7 of
// A is A[row r][k = 8 h + e], of B is B[k = 8 h + e][col r].  fp32: one element per instruction, A[row r][k = h], B[k = h][col r]; a lane loads 4 consecutive
// contraction elements and four instructions consume them, so the two halves of a step of 8 cover k = 4 h + q.  C/D for both: col = r, row = (i & 3) +
// 8 (i >> 2) + 4 h for register i = 0..15.  A step's contraction indices only have to agree between A and B, which they do by construction.
// Exact: values of the compute dtype.  Wide: fp32 values (a loss gradient); bf16 carries them as hi + lo, hi = bf16(x), lo = bf16(x - hi) (two
// instructions, 16 mantissa bits), so that they are not rounded to 8 bits before they are summed; everything accumulates in fp32.
#pragma once
#include "common.hpp"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ int acc_row(int i, int h) { return (i & 3) + 8 * (i >> 2) + 4 * h; }

template <typename T> struct MM;
template <> struct MM<bf16_t> {
  static constexpr int E = 8;                           // contraction elements per lane and step
  struct Exact { bf16x8 v; };
  struct Wide { bf16x8 hi, lo; };
  static __device__ __forceinline__ Exact load16(const bf16_t* p) { Exact f; f.v = *reinterpret_cast<const bf16x8*>(p); return f; }
  static __device__ __forceinline__ Exact zero() { Exact f; f.v = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; return f; }
  static __device__ __forceinline__ Wide wzero() { Wide f; f.hi = f.lo = bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; return f; }
  static __device__ __forceinline__ void relu(Exact& f) { f.v = f.v & ~(f.v < 0); }      // the sign bit set: negative (or -0) -> +0
  template <int I> static __device__ __forceinline__ void set(Exact& f, bf16_t x, bool relu_on) { f.v[I] = (relu_on && (short)x < 0) ? (short)0 : (short)x; }
  template <int I> static __device__ __forceinline__ void setw(Wide& f, float x) {
    const bf16_t hi = f2bf(x);
    f.hi[I] = (short)hi; f.lo[I] = (short)f2bf(x - bf2f(hi));
  }
  static __device__ __forceinline__ void mma(f32x16& acc, const Exact& a, const Exact& b) { acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.v, acc, 0, 0, 0); }
  static __device__ __forceinline__ void mma_wa(f32x16& acc, const Wide& a, const Exact& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.hi, b.v, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.lo, b.v, acc, 0, 0, 0);
  }
  static __device__ __forceinline__ void mma_wb(f32x16& acc, const Exact& a, const Wide& b) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.hi, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a.v, b.lo, acc, 0, 0, 0);
  }
};
template <> struct MM<float> {
  static constexpr int E = 4;
  struct Exact { float v[4]; };
  typedef Exact Wide;
  static __device__ __forceinline__ Exact load16(const float* p) { const float4 a = *reinterpret_cast<const float4*>(p); return Exact{{a.x, a.y, a.z, a.w}}; }
  static __device__ __forceinline__ Exact zero() { return Exact{{0.f, 0.f, 0.f, 0.f}}; }
  static __device__ __forceinline__ Wide wzero() { return zero(); }
  static __device__ __forceinline__ void relu(Exact& f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) f.v[e] = f.v[e] < 0.f ? 0.f : f.v[e];
  }
  template <int I> static __device__ __forceinline__ void set(Exact& f, float x, bool relu_on) { f.v[I] = (relu_on && x < 0.f) ? 0.f : x; }
  template <int I> static __device__ __forceinline__ void setw(Wide& f, float x) { f.v[I] = x; }
  static __device__ __forceinline__ void mma(f32x16& acc, const Exact& a, const Exact& b) {
#pragma unroll
    for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.v[e], b.v[e], acc, 0, 0, 0);
  }
  static __device__ __forceinline__ void mma_wa(f32x16& acc, const Wide& a, const Exact& b) { mma(acc, a, b); }
  static __device__ __forceinline__ void mma_wb(f32x16& acc, const Exact& a, const Wide& b) { mma(acc, a, b); }
};
__device__ __forceinline__ f32x16 acc_zero() {
  f32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}

// four consecutive channels of a gradient, zeroed where the rectified tensor t is not positive (relu_on), stored in the compute dtype
template <typename T> struct Out4;
template <> struct Out4<bf16_t> {
  static __device__ __forceinline__ void mask_store(bf16_t* d, const bf16_t* t, bool relu_on, float a, float b, float c, float e) {
    if (relu_on) {
      const uint2 m = *reinterpret_cast<const uint2*>(t);                       // > 0: sign clear and not zero
      const short t0 = (short)(m.x & 0xffff), t1 = (short)(m.x >> 16), t2 = (short)(m.y & 0xffff), t3 = (short)(m.y >> 16);
      a = t0 > 0 ? a : 0.f; b = t1 > 0 ? b : 0.f; c = t2 > 0 ? c : 0.f; e = t3 > 0 ? e : 0.f;
    }
    *reinterpret_cast<uint2*>(d) = make_uint2(pk_bf16(a, b), pk_bf16(c, e));
  }
};
template <> struct Out4<float> {
  static __device__ __forceinline__ void mask_store(float* d, const float* t, bool relu_on, float a, float b, float c, float e) {
    if (relu_on) {
      const float4 m = *reinterpret_cast<const float4*>(t);
      a = m.x > 0.f ? a : 0.f; b = m.y > 0.f ? b : 0.f; c = m.z > 0.f ? c : 0.f; e = m.w > 0.f ? e : 0.f;
    }
    *reinterpret_cast<float4*>(d) = make_float4(a, b, c, e);
  }
};

}  // namespace
