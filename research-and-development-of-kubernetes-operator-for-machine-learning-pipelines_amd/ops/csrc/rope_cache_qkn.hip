// Per-head QK-norm + RoPE (K4) + paged KV-cache write (K5): the stand-alone writers of a model
// whose attention applies an RMSNorm with a learned [128] weight to every q head and every k head
// before the rotation (Qwen3).  One writer for bf16 pages (rope_cache.hip's layouts) and one for
// e4m3fn pages with a scale byte per row (kv_fp8.hip's format, unchanged).
//
// Per q / k head row x[128] of the bf16 QKV projection output, all in fp32:
//   r = rsqrt(sum(x^2) / 128 + eps),  y[i] = (x[i] * r) * w[i]      w = q_w or k_w (bf16 [128])
//   out[i]      = y[i] cos[i] - y[i + 64] sin[i]                    i < 64 (HF rotate-half)
//   out[i + 64] = y[i + 64] cos[i] + y[i] sin[i]
// and ONE rounding to bf16 at the end.  V rows are copied (bf16) or quantised (fp8) untouched.
//
// Decomposition (kv_fp8.hip's): 16 lanes - one DPP row - per 128-element head row.  Lane j holds
// the 8 output elements 8j .. 8j + 7; with c = 8 (j & 7) it loads x[c .. c + 7] and
// x[64 + c .. 64 + c + 7] (two 16-B loads), so it owns both rotate-half partners of its outputs
// and nothing crosses lanes but the sum of squares.  Lanes 0-7 store the first half of the rotated
// row, lanes 8-15 the second: one 16-B store per lane (8 B to an e4m3fn page).
//
// Sum of squares, fixed order: each lane sums the squares of the 8 elements it OUTPUTS (lanes 0-7
// the x[c ..] vector, lanes 8-15 the x[64 + c ..] vector) in index order,
//   s = x0 x0;  s = fma(x_i, x_i, s)  i = 1 .. 7,
// then four DPP steps add partners in row16_max's order: quad_perm [1,0,3,2], quad_perm
// [2,3,0,1], row_half_mirror, row_mirror.  Every lane of the row ends with the same bits, and the
// order depends on nothing but the element index: not on the grid, the trip or the launch.
// Floating-point contraction is off in the shared function, so each product and sum below is the
// rounding that is written there, in both writers.
//
// A 16-lane group takes a head row per trip, and the trip count depends on the group's index
// only: all 16 lanes of a DPP row are live together or not at all (head counts that leave
// groups idle in the last trip included).  Nothing in the grid depends on data, no atomics, no
// LDS: the launches are graph-capturable as they are.
#include "common.h"
#include "launch.h"

namespace mlop {

namespace {

constexpr int D = 128, HALF = 64;

__device__ __forceinline__ float row16_sum(float v) {
  v += detail::dpp<0xB1>(v);   // quad_perm [1,0,3,2]
  v += detail::dpp<0x4E>(v);   // quad_perm [2,3,0,1]
  v += detail::dpp<0x141>(v);  // row_half_mirror
  v += detail::dpp<0x140>(v);  // row_mirror
  return v;
}

// kv_fp8.hip's row maximum, scale exponent and quantiser (that file's header has the rule)
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, detail::dpp<0xB1>(v));
  v = fmaxf(v, detail::dpp<0x4E>(v));
  v = fmaxf(v, detail::dpp<0x141>(v));
  v = fmaxf(v, detail::dpp<0x140>(v));
  return v;
}

__device__ __forceinline__ int fp8_row_exp(float amax) {
  const uint32_t b = __float_as_uint(amax);
  const int x = (int)(b >> 23) - 126;
  const int e = x - ((b & 0x7fffffu) <= 0x600000u ? 9 : 8);
  return min(max(e, -126), 127);
}

__device__ __forceinline__ u32x2 quant8(const float (&x)[8], int e) {
  const float inv = __uint_as_float((uint32_t)(127 - e) << 23);  // 2^-e
  float y[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) y[i] = fminf(fmaxf(x[i] * inv, -448.f), 448.f);
  int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], 0, false);
  w0 = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], w0, true);
  int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], 0, false);
  w1 = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], w1, true);
  return u32x2{(uint32_t)w0, (uint32_t)w1};
}

__device__ __forceinline__ void unpack8(const u32x4 v, float (&x)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) x[2 * i] = lo_bf(v[i]), x[2 * i + 1] = hi_bf(v[i]);
}

// Lane j's 8 elements (8j .. 8j + 7) of the normed and rotated head row at `head`, fp32 before
// the final rounding.  Both writers call this, so what they round is the same bits.
__device__ __forceinline__ void qkn_rope8(const uint16_t* __restrict__ head, const uint16_t* __restrict__ w,
                                          const float* __restrict__ cs, int j, float eps, float (&out)[8]) {
#pragma clang fp contract(off)
  const int c = (j & 7) * 8;
  const bool first = j < 8;
  float xa[8], xb[8], wa[8], wb[8];
  unpack8(*reinterpret_cast<const u32x4*>(head + c), xa);
  unpack8(*reinterpret_cast<const u32x4*>(head + HALF + c), xb);
  unpack8(*reinterpret_cast<const u32x4*>(w + c), wa);
  unpack8(*reinterpret_cast<const u32x4*>(w + HALF + c), wb);
  const float4* cp = reinterpret_cast<const float4*>(cs + c);
  const float4* sp = reinterpret_cast<const float4*>(cs + HALF + c);
  const float4 c0 = cp[0], c1 = cp[1], s0 = sp[0], s1 = sp[1];
  const float cc[8] = {c0.x, c0.y, c0.z, c0.w, c1.x, c1.y, c1.z, c1.w};
  const float sn[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
  float m0 = first ? xa[0] : xb[0];
  float s = m0 * m0;
#pragma unroll
  for (int i = 1; i < 8; ++i) {
    const float m = first ? xa[i] : xb[i];
    s = __builtin_fmaf(m, m, s);
  }
  s = row16_sum(s);
  const float r = rsqrtf(s * (1.f / D) + eps);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const float ya = (xa[i] * r) * wa[i];
    const float yb = (xb[i] * r) * wb[i];
    out[i] = first ? ya * cc[i] - yb * sn[i] : yb * cc[i] + ya * sn[i];
  }
}

__device__ __forceinline__ u32x4 pack8(const float (&x)[8]) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = pack2(x[2 * i], x[2 * i + 1]);
  return o;
}

}  // namespace

// grid (T, by): the token's Hq + 2 Hkv head rows (q, k, v in the projection's order) go round the
// 16 by 16-lane groups of its blocks.  A padding token (slot < 0) has its q rows only.
template <bool FP8>
__global__ void __launch_bounds__(256) rope_cache_qk_kernel(
    uint16_t* __restrict__ q_out, void* __restrict__ k_cache, void* __restrict__ v_cache,
    uint8_t* __restrict__ k_scale, uint8_t* __restrict__ v_scale, const uint16_t* __restrict__ qkv,
    const int* __restrict__ pos, const float* __restrict__ cos_sin, const int* __restrict__ slots,
    const uint16_t* __restrict__ q_w, const uint16_t* __restrict__ k_w, float eps, int Hq, int Hkv,
    int qkv_stride, int BS) {
  const int t = blockIdx.x;
  const float* cs = cos_sin + (size_t)pos[t] * D;
  const uint16_t* row = qkv + (size_t)t * qkv_stride;
  const int slot = slots[t];
  const int blk = slot >= 0 ? slot / BS : 0, off = slot >= 0 ? slot % BS : 0;
  const int nrows = slot >= 0 ? Hq + 2 * Hkv : Hq;
  const int j = threadIdx.x & 15;
  // (rw depends on the group only: the 16 lanes of a DPP row take the same trips)
  for (int rw = (threadIdx.x >> 4) + blockIdx.y * 16; rw < nrows; rw += 16 * gridDim.y) {
    const bool is_v = rw >= Hq + Hkv;
    float x[8];
    if (is_v) {
      unpack8(*reinterpret_cast<const u32x4*>(row + (size_t)rw * D + 8 * j), x);
    } else {
      qkn_rope8(row + (size_t)rw * D, rw < Hq ? q_w : k_w, cs, j, eps, x);
    }
    if (rw < Hq) {
      *reinterpret_cast<u32x4*>(q_out + ((size_t)t * Hq + rw) * D + 8 * j) = pack8(x);
      continue;
    }
    const int kh = is_v ? rw - Hq - Hkv : rw - Hq;
    const size_t r = ((size_t)blk * Hkv + kh) * BS + off;
    if constexpr (!FP8) {
      // (a V row's pack8 is exact: its values are bf16 already)
      *reinterpret_cast<u32x4*>((uint16_t*)(is_v ? v_cache : k_cache) + r * D + 8 * j) = pack8(x);
    } else {
      // the row as the bf16 writer stores it, then kv_fp8.hip's amax / exponent / quantiser
      float amax = 0.f;
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        x[i] = bf2f(f2bf(x[i]));
        amax = fmaxf(amax, fabsf(x[i]));
      }
      amax = row16_max(amax);
      const int e = fp8_row_exp(amax);
      *reinterpret_cast<u32x2*>((uint8_t*)(is_v ? v_cache : k_cache) + r * D + 8 * j) = quant8(x, e);
      if (j == 0) (is_v ? v_scale : k_scale)[r] = (uint8_t)(e + 127);
    }
  }
}

// blocks per token: one per 16 head rows, four at the most (Hq + 2 Hkv = 48 rows: three blocks
// of one trip each)
static int qkn_blocks(int Hq, int Hkv) { return std::min(4, std::max(1, cdiv(Hq + 2 * Hkv, 16))); }

void launch_rope_cache_qkn(void* q_out, void* k_cache, void* v_cache, const void* qkv, const int* pos,
                           const float* cos_sin, const int* slots, int T, int Hq, int Hkv, int qkv_stride,
                           int BS, const uint16_t* q_w, const uint16_t* k_w, float eps, hipStream_t st) {
  if (T == 0) return;
  rope_cache_qk_kernel<false><<<dim3(T, qkn_blocks(Hq, Hkv)), 256, 0, st>>>(
      (uint16_t*)q_out, k_cache, v_cache, nullptr, nullptr, (const uint16_t*)qkv, pos, cos_sin, slots, q_w, k_w,
      eps, Hq, Hkv, qkv_stride, BS);
}

void launch_rope_cache_qkn_fp8(void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                               const void* qkv, const int* pos, const float* cos_sin, const int* slots, int T,
                               int Hq, int Hkv, int qkv_stride, int BS, const uint16_t* q_w,
                               const uint16_t* k_w, float eps, hipStream_t st) {
  if (T == 0) return;
  rope_cache_qk_kernel<true><<<dim3(T, qkn_blocks(Hq, Hkv)), 256, 0, st>>>(
      (uint16_t*)q_out, k_cache, v_cache, (uint8_t*)k_scale, (uint8_t*)v_scale, (const uint16_t*)qkv, pos, cos_sin,
      slots, q_w, k_w, eps, Hq, Hkv, qkv_stride, BS);
}

}  // namespace mlop
