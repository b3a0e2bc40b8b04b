// MXFP4 -> bf16 conversion shared by gemm_mx4.hip (dense projections) and moe_mx4.hip (experts):
// one packed word (8 e2m1 codes) and the scale of its K-step into a lane's MFMA B fragment.
#pragma once
#include "common.h"

namespace mlop {

typedef __attribute__((ext_vector_type(2))) __bf16 mx4_bf16x2;

// the scale of K-step j from a tile's scale dword: byte j into the f32 exponent field
template <int J>
__device__ __forceinline__ float mx4_scale(uint32_t ew) {
  return __uint_as_float(((ew >> (8 * J)) & 0xffu) << 23);
}

// the 8 codes of one packed word, scaled, as the bf16x8 MFMA operand
__device__ __forceinline__ bf16x8 mx4_word(uint32_t w, float scale) {
  u32x4 o;
  o[0] = __builtin_bit_cast(uint32_t, (mx4_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 0));
  o[1] = __builtin_bit_cast(uint32_t, (mx4_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 1));
  o[2] = __builtin_bit_cast(uint32_t, (mx4_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 2));
  o[3] = __builtin_bit_cast(uint32_t, (mx4_bf16x2)__builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(w, scale, 3));
  return __builtin_bit_cast(bf16x8, o);
}

// SiLU of a bf16-rounded gate, rounded to bf16 (the fused SiLU-mul epilogues of moe_mx4.hip and
// gemm_mx4t.hip).  d = 1 + exp(-g) above 2^126 (g < -87.3) has a
// denormal reciprocal, which v_rcp_f32 returns as 0; there the reciprocal is taken of d 2^-32 and the
// scale goes back in after the product, which is a normal fp32 again (d = inf, g < -88.7: -0, as
// fp32 division gives).  Elsewhere s = 1 and the arithmetic is silu_bf's bit for bit.
__device__ __forceinline__ float mx4_silu(float g) {
  const float gb = bf2f(f2bf(g));
  const float d = 1.f + __expf(-gb);
  const float s = d > 0x1p100f ? 0x1p-32f : 1.f;
  return bf2f(f2bf(gb * __builtin_amdgcn_rcpf(d * s) * s));
}

}  // namespace mlop
