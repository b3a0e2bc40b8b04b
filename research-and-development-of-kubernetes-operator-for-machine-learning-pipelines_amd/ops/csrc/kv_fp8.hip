// RoPE (K4) + paged KV-cache write (K5) for an fp8 cache: rope_cache.hip's standalone writer
// with OCP e4m3fn pages and one power-of-two scale per (token, kv head) row, for K and for V.
//
//   k_cache / v_cache [NB, Hkv, BS, 128]  e4m3fn bytes, token-major: a row is one 128-B run
//   k_scale / v_scale [NB, Hkv, BS]       one byte b per row, the row's scale is the fp32 whose
//                                         bit pattern is b << 23: 2^(b - 127) for b >= 1, and
//                                         0.0 for the byte 0 of a zero-initialised tensor
//
// The scale exponent of a row is the smallest integer e with amax / 2^e <= 448 (e4m3fn's
// largest finite value), clamped to [-126, 127]: with amax = m 2^x (frexp, 0.5 <= m < 1),
// e = x - 9 if m <= 0.875 else x - 8.  It is taken from amax's exponent and mantissa bits, so
// ops/reference.py's quantiser (torch.frexp) gives the same byte.  amax is taken over the row
// AFTER its rounding to bf16 (the value the bf16 cache would hold), so fp8 rows are the
// quantisation of exactly the rows the bf16 writer stores.  x / 2^e is an exact fp32 product;
// the only rounding is v_cvt_pk_fp8_f32's (nearest even).
#include "common.h"
#include "launch.h"

namespace mlop {

// max over the 16 lanes of a DPP row (the lanes that hold one 128-element head row)
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, detail::dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, detail::dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, detail::dpp<0x141>(v));  // row_half_mirror
  v = fmaxf(v, detail::dpp<0x140>(v));  // row_mirror
  return v;
}

// scale exponent of a row with maximum magnitude amax >= 0 (header).  Zero and bf16 subnormals
// have exponent bits 0: x = -126 there, and the clamp gives the smallest exponent.
__device__ __forceinline__ int fp8_row_exp(float amax) {
  const uint32_t b = __float_as_uint(amax);
  const int x = (int)(b >> 23) - 126;
  const int e = x - ((b & 0x7fffffu) <= 0x600000u ? 9 : 8);
  return min(max(e, -126), 127);
}

// 8 floats of a row -> its 8 e4m3fn bytes at scale 2^e.  |x| / 2^e <= 448 for every finite
// row by the choice of e; the clamp makes an infinite element the largest finite byte.
__device__ __forceinline__ u32x2 quant8(const float (&x)[8], int e) {
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e, e <= 121 for any bf16 amax
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] * inv, -448.f), 448.f);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w1, true);
  return u32x2{(uint32_t)w0, (uint32_t)w1};
}

// grid (T, 2).  blockIdx.y == 0: the q heads, rope_cache_kernel's items and arithmetic (q is
// the bf16 op's q bit for bit).  blockIdx.y == 1: the token's 2 Hkv cache rows, 16 lanes per row
// (lane j holds elements 8j .. 8j + 7: one 8-B store, the row one 128-B run).
__global__ void __launch_bounds__(256) rope_cache_fp8_kernel(
    uint16_t* __restrict__ q_out, uint8_t* __restrict__ k_cache, uint8_t* __restrict__ v_cache,
    uint8_t* __restrict__ k_scale, uint8_t* __restrict__ v_scale, const uint16_t* __restrict__ qkv,
    const int* __restrict__ pos, const float* __restrict__ cos_sin, const int* __restrict__ slots, int Hq,
    int Hkv, int qkv_stride, int BS) {
  constexpr int D = 128, half = 64;
  const int t = blockIdx.x;
  const float* cs = cos_sin + (size_t)pos[t] * D;
  const uint16_t* row = qkv + (size_t)t * qkv_stride;
  if (blockIdx.y == 0) {
    for (int it = threadIdx.x; it < Hq * 8; it += blockDim.x) {
      const int h = it >> 3, c = (it & 7) * 8;
      const u32x4 a = *reinterpret_cast<const u32x4*>(row + h * D + c);
      const u32x4 b = *reinterpret_cast<const u32x4*>(row + h * D + half + c);
      const float4* cp = reinterpret_cast<const float4*>(cs + c);
      const float4* sp = reinterpret_cast<const float4*>(cs + half + c);
      const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
      const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
      u32x4 oa, ob;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float x0 = lo_bf(a[j]), x1 = hi_bf(a[j]);
        const float y0 = lo_bf(b[j]), y1 = hi_bf(b[j]);
        oa[j] = pack2(x0 * cc[2 * j] - y0 * ss[2 * j], x1 * cc[2 * j + 1] - y1 * ss[2 * j + 1]);
        ob[j] = pack2(y0 * cc[2 * j] + x0 * ss[2 * j], y1 * cc[2 * j + 1] + x1 * ss[2 * j + 1]);
      }
      uint16_t* dst = q_out + ((size_t)t * Hq + h) * D;
      *reinterpret_cast<u32x4*>(dst + c) = oa;
      *reinterpret_cast<u32x4*>(dst + half + c) = ob;
    }
    return;
  }
  const int slot = slots[t];
  if (slot < 0) return;  // padding token: no cache write
  const int blk = slot / BS, off = slot % BS;
  const int j = threadIdx.x & 15;
  // (a 16-lane group takes the same trips, so the DPP steps of row16_max see live lanes only)
  for (int rw = threadIdx.x >> 4; rw < 2 * Hkv; rw += blockDim.x >> 4) {
    const bool is_v = rw >= Hkv;
    const int kh = is_v ? rw - Hkv : rw;
    float x[8];
    if (is_v) {
      const u32x4 a = *reinterpret_cast<const u32x4*>(row + (Hq + Hkv + kh) * D + 8 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i) x[2 * i] = lo_bf(a[i]), x[2 * i + 1] = hi_bf(a[i]);
    } else {
      // lanes 0-7 hold the first half of the rotated row (x cos - y sin), lanes 8-15 the
      // second (y cos + x sin), each of elements c .. c + 7 of its half; rounded to bf16 as
      // the bf16 cache would hold it
      const int c = (j & 7) * 8;
      const u32x4 a = *reinterpret_cast<const u32x4*>(row + (Hq + kh) * D + c);
      const u32x4 b = *reinterpret_cast<const u32x4*>(row + (Hq + kh) * D + half + c);
      const float4* cp = reinterpret_cast<const float4*>(cs + c);
      const float4* sp = reinterpret_cast<const float4*>(cs + half + c);
      const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
      const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
      const float ss[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float xv = (i & 1) ? hi_bf(a[i >> 1]) : lo_bf(a[i >> 1]);
        const float yv = (i & 1) ? hi_bf(b[i >> 1]) : lo_bf(b[i >> 1]);
        x[i] = bf2f(f2bf(j < 8 ? xv * cc[i] - yv * ss[i] : yv * cc[i] + xv * ss[i]));
      }
    }
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) amax = fmaxf(amax, fabsf(x[i]));
    amax = row16_max(amax);
    const int e = fp8_row_exp(amax);
    const size_t r = ((size_t)blk * Hkv + kh) * BS + off;
    *reinterpret_cast<u32x2*>((is_v ? v_cache : k_cache) + r * D + 8 * j) = quant8(x, e);
    if (j == 0) (is_v ? v_scale : k_scale)[r] = (uint8_t)(e + 127);
  }
}

void launch_rope_cache_fp8(void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                           const void* qkv, const int* pos, const float* cos_sin, const int* slots, int T,
                           int Hq, int Hkv, int qkv_stride, int BS, hipStream_t st) {
  if (T == 0) return;
  rope_cache_fp8_kernel<<<dim3(T, 2), 256, 0, st>>>((uint16_t*)q_out, (uint8_t*)k_cache, (uint8_t*)v_cache,
                                                    (uint8_t*)k_scale, (uint8_t*)v_scale, (const uint16_t*)qkv,
                                                    pos, cos_sin, slots, Hq, Hkv, qkv_stride, BS);
}

}  // namespace mlop
