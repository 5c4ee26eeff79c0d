// Device helpers shared by the split-operand kernel files: one copy of what conv_split.hip, linear_split.hip, conv_dma.hip,
// conv_ks.hip and stage_conv.hip each carried.  (stage_conv16.hip, head_fused16.hip and window_attn.hip keep their own
// two-term splits: different signatures.  stage_conv.hip and stage_conv16.hip keep their own lds_barrier: its barrier is
// the builtin, which the compiler may schedule around, not the asm statement below.)
#pragma once
#include "common.hpp"
#include "conv_split.hpp"

#include <type_traits>
#include <utility>

namespace drba {

// fp32 -> (h, m, l) bf16 with round-to-nearest-even at every step; returns the three terms of 2 values packed
__device__ __forceinline__ void split2(float a, float b, unsigned &h, unsigned &m, unsigned &l) {
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  auto pk = [](float x, float y) -> unsigned {
    const bf16x2 p = __builtin_convertvector(f32x2{x, y}, bf16x2);
    return __builtin_bit_cast(unsigned, p);
  };
  h = pk(a, b);
  const float ra = a - __uint_as_float(h << 16), rb = b - __uint_as_float(h & 0xffff0000u);
  m = pk(ra, rb);
  l = pk(ra - __uint_as_float(m << 16), rb - __uint_as_float(m & 0xffff0000u));
}

// two-term fp16 form (conv_split.hip "Two-term form"): x * 2^-kSplitActShift = h + 2^-11 l
__device__ __forceinline__ void split2_f16(float a, float b, unsigned &h, unsigned &l) {
  typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 v = (f32x2){a, b} * (1.f / (float)(1 << kSplitActShift));
  const f16x2 hh = __builtin_convertvector(v, f16x2);
  const f32x2 r = (v - __builtin_convertvector(hh, f32x2)) * 2048.f;
  const f16x2 ll = __builtin_convertvector(r, f16x2);
  h = __builtin_bit_cast(unsigned, hh);
  l = __builtin_bit_cast(unsigned, ll);
}

// LDS traffic of this wave done, then the workgroup barrier; global loads stay in flight (no vmcnt wait)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// compile-time loop: f(std::integral_constant<int, 0>{}) ... f(<N - 1>), for bodies whose index must be a constant in every
// copy (hipcc does not fully unroll an 18 x 12 body on `#pragma unroll` alone)
template <class F, int... I>
__device__ __forceinline__ void static_for_impl(F &&f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void static_for(F &&f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

}  // namespace drba
