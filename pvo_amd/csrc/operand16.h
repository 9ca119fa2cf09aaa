// operand16.h — the one vocabulary for fp16 / bf16 operands in device code: the vector types the matrix cores and the 16-byte
// accesses use, the MFMA wrappers, and the conversions between float and a 16-bit pattern carried in a uint32_t.  T is the
// storage tag (pvo_half / pvo_bf16); every conversion goes through Elem<T> (common.h), where it is stated once.
#pragma once
#include "common.h"

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));    // 8 x 16-bit: one lane's k-group of an MFMA, one 16-byte access
typedef float v4f __attribute__((ext_vector_type(4)));         // accumulator tile of a 16x16 MFMA
typedef float v16f __attribute__((ext_vector_type(16)));       // accumulator tile of a 32x32 MFMA
typedef _Float16 v8h __attribute__((ext_vector_type(8)));
typedef __bf16 v8b __attribute__((ext_vector_type(8)));

// D[16x16] += A[16x32] B[32x16]: v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x32_bf16
template <typename T> __device__ __forceinline__ v4f pvo_mfma(u32x4 a, u32x4 b, v4f c);
template <> __device__ __forceinline__ v4f pvo_mfma<pvo_half>(u32x4 a, u32x4 b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ v4f pvo_mfma<pvo_bf16>(u32x4 a, u32x4 b, v4f c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(v8b, a), __builtin_bit_cast(v8b, b), c, 0, 0, 0);
}
// D[32x32] += A[32x16] B[16x32]: v_mfma_f32_32x32x16_f16 / v_mfma_f32_32x32x16_bf16
template <typename T> __device__ __forceinline__ v16f pvo_mfma32(u32x4 a, u32x4 b, v16f c);
template <> __device__ __forceinline__ v16f pvo_mfma32<pvo_half>(u32x4 a, u32x4 b, v16f c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(v8h, a), __builtin_bit_cast(v8h, b), c, 0, 0, 0);
}
template <> __device__ __forceinline__ v16f pvo_mfma32<pvo_bf16>(u32x4 a, u32x4 b, v16f c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(v8b, a), __builtin_bit_cast(v8b, b), c, 0, 0, 0);
}

// float -> 16-bit pattern (round to nearest even, in the low half of the result), the pattern's value (the low half of b is
// read), and a float rounded to the storage type
template <typename T> __device__ __forceinline__ uint32_t pvo_bits(float x) {
  return __builtin_bit_cast(uint16_t, Elem<T>::from_f32(x));
}
template <typename T> __device__ __forceinline__ float pvo_val(uint32_t b) {
  return Elem<T>::to_f32(__builtin_bit_cast(typename Elem<T>::store_t, static_cast<uint16_t>(b)));
}
template <typename T> __device__ __forceinline__ float pvo_round(float x) { return Elem<T>::to_f32(Elem<T>::from_f32(x)); }

// 8 x 16-bit (element 2k in the low half of word k) <-> 8 x float
template <typename T> __device__ __forceinline__ void pvo_unpack8(u32x4 v, float f[8]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) { f[2 * k] = pvo_val<T>(v[k] & 0xffffu); f[2 * k + 1] = pvo_val<T>(v[k] >> 16); }
}
template <typename T> __device__ __forceinline__ u32x4 pvo_pack8(const float f[8]) {
  u32x4 v;
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = pvo_bits<T>(f[2 * k]) | (pvo_bits<T>(f[2 * k + 1]) << 16);
  return v;
}
