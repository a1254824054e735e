// MXFP8 (OCP microscaling) quantisation helpers shared by the quantiser, the LayerNorm and the GEMM epilogue:
// blocks of 32 consecutive K elements, e4m3fn elements, one E8M0 scale byte s per block (value = 2^(s-127) * element).
// The definition is stableavatar_amd/mxfp8.py (quantize / dequantize); these reproduce it bit for bit.
#pragma once
#include "common.h"

// E8M0 byte of a block whose absolute maximum is amax (finite): e = the smallest integer with amax * 2^-e <= 448
// = 1.75 * 2^8, i.e. exponent(amax) - 8, one more when the mantissa exceeds 1.75; s = clamp(e + 127, 0, 254)
// (e + 127 <= 247 for every finite fp32); an all-zero block takes e = 0
__device__ __forceinline__ uint32_t mx_scale_byte(float amax) {
  const uint32_t u = __float_as_uint(amax) & 0x7fffffffu;
  const int s = (int)(u >> 23) - 8 + ((u & 0x7fffffu) > 0x600000u ? 1 : 0);
  return u == 0 ? 127u : (uint32_t)max(s, 0);
}

// 2^-e for the scale byte s = e + 127: an exact power of two (biased exponent 254 - s, 7 .. 254)
__device__ __forceinline__ float mx_inv_scale(uint32_t s) { return __uint_as_float((254u - s) << 23); }

// four values (already multiplied by 2^-e, |v| <= 448) -> four e4m3fn bytes, round to nearest even
// (v_cvt_pk_fp8_f32: OCP e4m3fn on gfx950)
__device__ __forceinline__ uint32_t mx_pack4(float a, float b, float c, float d) {
  int r = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  r = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, r, true);
  return (uint32_t)r;
}

// eight values of one block held by this lane, amax = the whole block's maximum (already reduced over the
// lanes that share the block): the lane's eight element bytes; *s_out = the block's scale byte
__device__ __forceinline__ u32x2 mx_quant8(const float* v, float amax, uint32_t* s_out) {
  const uint32_t s = mx_scale_byte(amax);
  const float k = mx_inv_scale(s);
  *s_out = s;
  return (u32x2){mx_pack4(v[0] * k, v[1] * k, v[2] * k, v[3] * k), mx_pack4(v[4] * k, v[5] * k, v[6] * k, v[7] * k)};
}

__device__ __forceinline__ float mx_amax8(const float* v) {
  float m = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) m = fmaxf(m, fabsf(v[j]));
  return m;
}
