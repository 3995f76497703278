// Traits of the two 16-bit element types the MFMA kernels are templated
// on: bf16 (__hip_bfloat16) and fp16 (_Float16, the compiler's native
// half; bit-compatible with __half / at::Half and, unlike __half, still
// convertible to and from float when the build defines
// __HIP_NO_HALF_CONVERSIONS__).
//
// Both feed v_mfma_f32_16x16x32_{bf16,f16} with the same 8-element,
// 4-VGPR A/B fragments and the same C/D layout (tools/mfma_probe.hip), so
// every LDS image, pack LUT and store pattern is shared; only the items
// below differ. Conversions from fp32 round to nearest even and overflow
// to inf, as tensor.to(dtype) does.

#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <cstdint>

namespace elem16 {

using f32x4 = __attribute__((ext_vector_type(4))) float;

template <typename T>
struct Elem16;

template <>
struct Elem16<__hip_bfloat16> {
  using storage = __hip_bfloat16;
  using raw = __bf16;  // element of the register fragments
  using frag8 = __attribute__((ext_vector_type(8))) __bf16;
  using frag4 = __attribute__((ext_vector_type(4))) __bf16;
  static constexpr short kOne = (short)0x3F80;  // 1.0
  static __device__ __forceinline__ f32x4 mfma(frag8 a, frag8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ storage from_float(float f) {
    return (__hip_bfloat16)f;
  }
  static __device__ __forceinline__ uint32_t bits(storage h) {
    return (uint32_t)__bfloat16_as_ushort(h);
  }
};

template <>
struct Elem16<_Float16> {
  using storage = _Float16;
  using raw = _Float16;
  using frag8 = __attribute__((ext_vector_type(8))) _Float16;
  using frag4 = __attribute__((ext_vector_type(4))) _Float16;
  static constexpr short kOne = (short)0x3C00;  // 1.0
  static __device__ __forceinline__ f32x4 mfma(frag8 a, frag8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ storage from_float(float f) {
    return (_Float16)f;  // v_cvt_f16_f32: RNE, overflow -> inf
  }
  static __device__ __forceinline__ uint32_t bits(storage h) {
    return (uint32_t)__builtin_bit_cast(unsigned short, h);
  }
};

// two / four fp32 values -> packed T, lowest element in the low half
template <typename T>
__device__ __forceinline__ uint32_t pack2(float a, float b) {
  using E = Elem16<T>;
  return E::bits(E::from_float(a)) | (E::bits(E::from_float(b)) << 16);
}

template <typename T>
__device__ __forceinline__ uint2 pack4(float a, float b, float c, float d) {
  uint2 u;
  u.x = pack2<T>(a, b);
  u.y = pack2<T>(c, d);
  return u;
}

}  // namespace elem16
