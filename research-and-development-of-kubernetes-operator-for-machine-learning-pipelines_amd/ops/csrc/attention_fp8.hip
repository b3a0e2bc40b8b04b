// Paged attention over an fp8 KV cache (kv_fp8.hip's pages and scale bytes): attention.hip's
// paged_attn_kernel - 16-row tiles, four waves per (tile, kv head, partition), page pairs
// round-robin over the waves, split-KV with the in-launch combine - with 1-byte K / V.
//
// Q and P stay bf16 and the MFMAs 16x16x32 bf16: K and V fragments are converted e4m3 -> bf16
// in registers (exact: e4m3 has 3 mantissa bits and a narrower exponent range), so the only
// error of the fp8 cache is the quantisation of the stored rows.  The row scales are powers of
// two and are folded in exactly: S *= 2^e_k on the accumulator, p *= 2^e_v on the way to the
// bf16 P fragment, AFTER l has summed the unscaled p.
//
// K: an fp8 fragment and a bf16 fragment of this MFMA both hold 8 consecutive k per lane, so
// the conversion is lane-local.  Lane (r, g4) loads bytes 16 g4 .. +15 and 64 + 16 g4 .. +15 of
// its token row (two 16-B loads; a row's four lanes read whole 64-B runs): k-step kk holds
// dims 64 (kk >> 1) + 16 g4 + 8 (kk & 1) .. +7, and Q is loaded in the same order (the
// contraction order over d is free).
// V: loaded to VGPRs (16 B = 16 dims of one token row per lane and load), converted, and
// written with ds_write_b128 into the bf16 image attention.hip's vt_frag reads transposed:
// row t at 256 t, 16-B chunk c at slot c ^ vswz(t).  (The 8-bit transposed read of a 128-B-row
// fp8 image would halve the LDS traffic; profiles/fp8_kv.md says why it is not used.)
//
// REQUIREMENT, as attention.hip: pages AND scale rows are zero-initialised at allocation.
// Byte 0 is +0.0 as e4m3 and scale 0.0, and every byte the writer stores is finite; a scale
// byte 255 (+inf) is never written.
#include <type_traits>
#include <algorithm>

#include "common.h"
#include "launch.h"

namespace mlop {

namespace {

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

constexpr int kD = 128;
constexpr int kBS = 16;
constexpr float kNegBig = -1.0e30f;

// the bf16 V image and its transposed read: attention.hip's vswz / vt_base / vt_frag
__device__ __forceinline__ int vswz(int t) { return ((t & 3) << 2) | ((t >> 2) & 3); }
typedef short v4s16 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s16 lds_v4s16;
typedef __attribute__((address_space(3))) u32x4 lds_u32x4;
__device__ __forceinline__ uint32_t vt_base(int lane) {
  const int g4 = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int row = 8 * g4 + q, sw = vswz(row & 15);
  return 256u * row + 16u * ((p >> 1) ^ (sw & 1)) + 8u * (p & 1) + 32u * (sw >> 1);
}
__device__ __forceinline__ bf16x8 vt_frag(uint32_t b, int d) {
  const uint32_t a0 = b ^ (32u * d), a1 = (a0 ^ 16u) + 1024u;
  const v4s16 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s16*)(uintptr_t)a0);
  const v4s16 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s16*)(uintptr_t)a1);
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    f[e] = lo[e];
    f[4 + e] = hi[e];
  }
  return f;
}

__device__ __forceinline__ int wid_of(unsigned t) { return __builtin_amdgcn_readfirstlane((int)(t >> 6)); }

// 8 consecutive e4m3fn bytes -> one bf16 fragment: v_cvt_pk_f32_fp8 per byte pair, then the
// high halves of the two floats in one v_perm_b32 (the conversion to bf16 drops zero bits only)
__device__ __forceinline__ bf16x8 cvt8(uint32_t w0, uint32_t w1) {
  const auto f0 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false);
  const auto f1 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
  const auto f2 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false);
  const auto f3 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
  u32x4 o;
  o[0] = __builtin_amdgcn_perm(__float_as_uint(f0[1]), __float_as_uint(f0[0]), 0x07060302u);
  o[1] = __builtin_amdgcn_perm(__float_as_uint(f1[1]), __float_as_uint(f1[0]), 0x07060302u);
  o[2] = __builtin_amdgcn_perm(__float_as_uint(f2[1]), __float_as_uint(f2[0]), 0x07060302u);
  o[3] = __builtin_amdgcn_perm(__float_as_uint(f3[1]), __float_as_uint(f3[0]), 0x07060302u);
  return __builtin_bit_cast(bf16x8, o);
}

// scale byte i of a dword of four -> the fp32 with bit pattern byte << 23 (kv_fp8.hip)
__device__ __forceinline__ float scale_of(uint32_t w, int i) {
  return __uint_as_float(((w >> (8 * i)) & 0xffu) << 23);
}

template <bool NT>
__device__ __forceinline__ u32x4 load16(const uint8_t* p) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
  else return *reinterpret_cast<const u32x4*>(p);
}

}  // namespace

// NT bit 0: K / V loads non-temporal, bit 1: the output stores (paged_attn_kernel's switch)
template <int G, int NT>
__global__ void __launch_bounds__(256) paged_attn_fp8_kernel(
    uint16_t* __restrict__ out, float* __restrict__ part_o, float* __restrict__ part_ml,
    const uint16_t* __restrict__ q, const uint8_t* __restrict__ kc, const uint8_t* __restrict__ vc,
    const uint8_t* __restrict__ ksc, const uint8_t* __restrict__ vsc,
    const int* __restrict__ block_tables, int bt_stride,
    const int* __restrict__ tile_seq, const int* __restrict__ tile_q0,
    const int* __restrict__ q_start, const int* __restrict__ q_len,
    const int* __restrict__ ctx_len, int Hq, int Hkv, float scale_log2, int part_tokens,
    int nparts, int num_blocks, int* __restrict__ sem) {
  constexpr int QT = 16 / G;
  // wave w builds its page pair's bf16 V image (2 x 16 token rows x 256 B = 8 KB) inside
  // sm_o[w] (8448 B, 256-B aligned: vt_frag), which it alone writes after its loop
  __shared__ __attribute__((aligned(256))) float sm_o[4][16][kD + 4];
  __shared__ float sm_m[4][16];
  __shared__ float sm_l[4][16];
  __shared__ int sm_last;

  const int tile = blockIdx.x, kvh = blockIdx.y, part = blockIdx.z;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int s = tile_seq[tile], q0 = tile_q0[tile];
  const int* bt = block_tables + (size_t)s * bt_stride;
  const int p_begin = part * part_tokens;
  // the wave's first page pair, read in the same round trip as the lengths (clamped into the
  // row, used only if the pair exists)
  const int bt0 = 2 * ((p_begin >> 5) + wid_of(threadIdx.x));
  const int rawA = bt[min(bt0, bt_stride - 1)], rawB = bt[min(bt0 + 1, bt_stride - 1)];
  const int ql = q_len[s], ctx = ctx_len[s], qs = q_start[s];
  const int last_q = min(q0 + QT, ql) - 1;           // last valid query of the tile
  const int kv_end = last_q >= 0 ? ctx - ql + last_q + 1 : 0;
  const int p_end = min(kv_end, p_begin + part_tokens);
  if (p_begin >= p_end && nparts > 1) {              // reducer skips empty partitions
    // kv_end == 0 (graph-bucket padding rows, ctx 0): no partition draws the last ticket of
    // the in-launch combine, so partition 0 writes the zero row attn_reduce_kernel would
    if (sem != nullptr && part == 0 && kv_end <= 0) {
      const int rr = threadIdx.x >> 4, c = (threadIdx.x & 15) * 8;
      const int qi2 = q0 + rr / G;
      if (qi2 < ql)
        *reinterpret_cast<u32x4*>(out + ((size_t)(qs + qi2) * Hq + kvh * G + (rr % G)) * kD + c) =
            u32x4{0u, 0u, 0u, 0u};
    }
    return;
  }

  // this lane's q-row (B operand column) and its causal limit
  const int r = lane & 15, g4 = lane >> 4;
  const int qi = q0 + r / G;
  const bool row_ok = qi < ql;
  const int head = kvh * G + (r % G);
  const int pos_r = row_ok ? ctx - ql + qi : -1;

  // Q in the K loads' d order: k-step kk = dims 64 (kk >> 1) + 16 g4 + 8 (kk & 1) .. +7
  bf16x8 qf[4];
  {
    const uint16_t* qrow = q + ((size_t)(qs + (row_ok ? qi : 0)) * Hq + head) * kD;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      bf16x8 v = *reinterpret_cast<const bf16x8*>(qrow + 64 * (kk >> 1) + 16 * g4 + 8 * (kk & 1));
      qf[kk] = row_ok ? v : bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  }

  f32x4 o[8];
#pragma unroll
  for (int d = 0; d < 8; ++d) o[d] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = kNegBig, l = 0.f;

  const int pp_begin = p_begin >> 5;
  const int pp_end = (p_end + 31) >> 5;
  const int n_pages = (p_end + kBS - 1) / kBS;
  const size_t page_stride = (size_t)Hkv * kBS * kD;  // bytes
  const size_t srow_stride = (size_t)Hkv * kBS;       // scale bytes per page

  // (a generic pointer's low 32 bits are the LDS offset)
  const uint32_t vimg = (uint32_t)(uintptr_t)&sm_o[0][0][0] + wid * 8448u;
  // clamp: a corrupt block table must not become an out-of-bounds fault (pages and scale rows
  // are addressed by the same clamped id)
  auto page_a = [&](int pp) { return min(max(bt[2 * pp], 0), num_blocks - 1); };
  auto page_b = [&](int pp, int pa) { return (2 * pp + 1 < n_pages) ? min(max(bt[2 * pp + 1], 0), num_blocks - 1) : pa; };
  // V load j of this lane: image row 8 j + (lane >> 3) (rows 0-15 page A, 16-31 page B), bytes
  // 16 (lane & 7) .. +15 of the token row = bf16 chunks 2 (lane & 7) and + 1
  const int v_row = lane >> 3, v_c8 = lane & 7;
  const uint32_t v_dst = vimg + 256u * v_row;
  // page ids one pair ahead: the block-table loads of pair pp + 4 run under pair pp
  int pgA = 0, pgB = 0;
  if (pp_begin + wid < pp_end) {
    pgA = min(max(rawA, 0), num_blocks - 1);
    pgB = (bt0 + 1 < n_pages) ? min(max(rawB, 0), num_blocks - 1) : pgA;
  }
  for (int pp = pp_begin + wid; pp < pp_end; pp += 4) {
    const uint8_t* kA = kc + pgA * page_stride + (size_t)kvh * kBS * kD;
    const uint8_t* kB = kc + pgB * page_stride + (size_t)kvh * kBS * kD;

    // K rows of MFMA row r: pair tokens 8*(r>>2) + (r&3) (first S MFMA) and +4 (second)
    const uint8_t* kR = (r >> 3 ? kB : kA) + (8 * ((r >> 2) & 1) + (r & 3)) * kD + 16 * g4;
    const u32x4 ka0 = load16<(NT & 1) != 0>(kR), ka1 = load16<(NT & 1) != 0>(kR + 64);
    const u32x4 kb0 = load16<(NT & 1) != 0>(kR + 4 * kD), kb1 = load16<(NT & 1) != 0>(kR + 4 * kD + 64);
    // the scales of this lane's 8 consecutive pair tokens 8 g4 .. +7: 8 contiguous bytes
    const size_t srow = (size_t)(g4 >> 1 ? pgB : pgA) * srow_stride + (size_t)kvh * kBS + 8 * (g4 & 1);
    const u32x2 ksw = *reinterpret_cast<const u32x2*>(ksc + srow);
    const u32x2 vsw = *reinterpret_cast<const u32x2*>(vsc + srow);
    // this pair's V rows, issued behind the K loads
    const uint8_t* vA = vc + pgA * page_stride + (size_t)kvh * kBS * kD + v_row * kD + 16 * v_c8;
    const uint8_t* vB = vc + pgB * page_stride + (size_t)kvh * kBS * kD + v_row * kD + 16 * v_c8;
    u32x4 vr[4];
    vr[0] = load16<(NT & 1) != 0>(vA);
    vr[1] = load16<(NT & 1) != 0>(vA + 8 * kD);
    vr[2] = load16<(NT & 1) != 0>(vB);
    vr[3] = load16<(NT & 1) != 0>(vB + 8 * kD);
    if (pp + 4 < pp_end) {
      pgA = page_a(pp + 4);
      pgB = page_b(pp + 4, pgA);
    }
    bf16x8 ka[4], kb[4];
    ka[0] = cvt8(ka0[0], ka0[1]); ka[1] = cvt8(ka0[2], ka0[3]);
    ka[2] = cvt8(ka1[0], ka1[1]); ka[3] = cvt8(ka1[2], ka1[3]);
    kb[0] = cvt8(kb0[0], kb0[1]); kb[1] = cvt8(kb0[2], kb0[3]);
    kb[2] = cvt8(kb1[0], kb1[1]); kb[3] = cvt8(kb1[2], kb1[3]);
    bf16x8 vf8[8];
    // S^T[token][row]: lane holds row r, tokens 8*g4 + i (sa) and 8*g4 + 4 + i (sb) of the pair
    f32x4 sa = {0.f, 0.f, 0.f, 0.f}, sb = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      sa = mfma16(ka[kk], qf[kk], sa);
      sb = mfma16(kb[kk], qf[kk], sb);
    }
    const int tokA = pp * 32 + g4 * 8, tokB = tokA + 4;
    float pa[4], pb[4];
    float mx = kNegBig;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ta = tokA + i, tb = tokB + i;
      // S *= 2^e_k first (exact), then the softmax scale
      pa[i] = (ta < p_end && ta <= pos_r) ? sa[i] * scale_of(ksw[0], i) * scale_log2 : -INFINITY;
      pb[i] = (tb < p_end && tb <= pos_r) ? sb[i] * scale_of(ksw[1], i) * scale_log2 : -INFINITY;
      mx = fmaxf(mx, fmaxf(pa[i], pb[i]));
    }
    mx = max_x16_x32(mx);
    const float m_new = fmaxf(m, mx);
    const float alpha = fast_exp2(m - m_new);
    m = m_new;
    float rs = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pa[i] = fast_exp2(pa[i] - m_new);
      pb[i] = fast_exp2(pb[i] - m_new);
      rs += pa[i] + pb[i];
    }
    l = l * alpha + rs;  // the unscaled p
    bf16x8 pf;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      pf[i] = (short)f2bf(pa[i] * scale_of(vsw[0], i));      // p 2^e_v: exact before the rounding
      pf[4 + i] = (short)f2bf(pb[i] * scale_of(vsw[1], i));
    }
    {
      // the bf16 image: a wave's LDS operations execute in order, so these writes follow the
      // previous pair's transposed reads and precede this pair's without a barrier
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int sw = vswz((8 * j + v_row) & 15);
        const uint32_t a = v_dst + 2048u * j;
        *(lds_u32x4*)(uintptr_t)(a + 16u * ((2 * v_c8) ^ sw)) = __builtin_bit_cast(u32x4, cvt8(vr[j][0], vr[j][1]));
        *(lds_u32x4*)(uintptr_t)(a + 16u * ((2 * v_c8 + 1) ^ sw)) = __builtin_bit_cast(u32x4, cvt8(vr[j][2], vr[j][3]));
      }
      asm volatile("" ::: "memory");
      uint32_t b0 = vimg + vt_base(lane);
      asm volatile("" : "+v"(b0));  // no hoisting of the 16 read addresses out of the loop
#pragma unroll
      for (int d = 0; d < 8; ++d) vf8[d] = vt_frag(b0, d);
      asm volatile("" ::: "memory");
    }
#pragma unroll
    for (int d = 0; d < 8; ++d) {
      o[d] *= alpha;
      o[d] = mfma16(vf8[d], pf, o[d]);
    }
  }

  // ---- from here on paged_attn_kernel's merge, store and in-launch combine, unchanged
  l = sum_x16_x32(l);
  // O^T[d][row]: lane holds row r, dims 16*dblk + 4*g4 + i
#pragma unroll
  for (int d = 0; d < 8; ++d)
#pragma unroll
    for (int i = 0; i < 4; ++i) sm_o[wid][r][d * 16 + g4 * 4 + i] = o[d][i];
  if (g4 == 0) {
    sm_m[wid][r] = m;
    sm_l[wid][r] = l;
  }
  __syncthreads();

  const int rr = threadIdx.x >> 4, c = (threadIdx.x & 15) * 8;
  float M = kNegBig;
#pragma unroll
  for (int w = 0; w < 4; ++w) M = fmaxf(M, sm_m[w][rr]);
  float L = 0.f, acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const float f = exp2f(sm_m[w][rr] - M);
    L += f * sm_l[w][rr];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] += f * sm_o[w][rr][c + j];
  }
  const int qi2 = q0 + rr / G;
  const bool row_valid = qi2 < ql;
  const int head2 = kvh * G + (rr % G);
  if (nparts == 1) {
    if (!row_valid) return;
    const float inv = L > 0.f ? 1.f / L : 0.f;
    u32x4 ov;
#pragma unroll
    for (int j = 0; j < 4; ++j) ov[j] = pack2(acc[2 * j] * inv, acc[2 * j + 1] * inv);
    u32x4* dst = reinterpret_cast<u32x4*>(out + ((size_t)(qs + qi2) * Hq + head2) * kD + c);
    if constexpr ((NT & 2) != 0) __builtin_nontemporal_store(ov, dst);
    else *dst = ov;
    return;
  }
  if (row_valid) {
    // sc1 stores (write-through to L2): the hand-off below needs no agent release
    const size_t slab = (((size_t)tile * Hkv + kvh) * nparts + part) * 16;
    const auto rs_o = __builtin_amdgcn_make_buffer_rsrc(part_o + slab * kD, 0, 16 * kD * 4, 0x00020000);
    const uint32_t oo = (uint32_t)(rr * kD + c) * 4u;
    u32x4 w0, w1;
    w0[0] = __float_as_uint(acc[0]); w0[1] = __float_as_uint(acc[1]);
    w0[2] = __float_as_uint(acc[2]); w0[3] = __float_as_uint(acc[3]);
    w1[0] = __float_as_uint(acc[4]); w1[1] = __float_as_uint(acc[5]);
    w1[2] = __float_as_uint(acc[6]); w1[3] = __float_as_uint(acc[7]);
    __builtin_amdgcn_raw_buffer_store_b128(w0, rs_o, oo, 0, 16 /* sc1 */);
    __builtin_amdgcn_raw_buffer_store_b128(w1, rs_o, oo + 16u, 0, 16 /* sc1 */);
    if ((threadIdx.x & 15) == 0) {
      const auto rs_ml = __builtin_amdgcn_make_buffer_rsrc(part_ml + slab * 2, 0, 16 * 2 * 4, 0x00020000);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(M), rs_ml, (uint32_t)rr * 8u, 0, 16);
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(L), rs_ml, (uint32_t)rr * 8u + 4u, 0, 16);
    }
  }
  if (sem == nullptr) return;  // attn_reduce_kernel combines in a second launch
  // in-launch combine: the partition that draws the last ticket reduces every slab and
  // re-arms the counter (attention.hip, same protocol)
  const int nvalid = min(nparts, (kv_end + part_tokens - 1) / part_tokens);
  int* cnt = sem + (size_t)tile * Hkv + kvh;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t = __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sm_last = (t == nvalid - 1);
  }
  __syncthreads();
  if (!sm_last) return;
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(cnt, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();
  if (!row_valid) return;
  const size_t base = ((size_t)tile * Hkv + kvh) * nparts;
  float MM = kNegBig;
  for (int p = 0; p < nvalid; ++p) MM = fmaxf(MM, part_ml[((base + p) * 16 + rr) * 2]);
  float LL = 0.f, a2[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int p = 0; p < nvalid; ++p) {
    const size_t pb = (base + p) * 16 + rr;
    const float f = exp2f(part_ml[pb * 2] - MM);
    LL += f * part_ml[pb * 2 + 1];
    const float4* po = reinterpret_cast<const float4*>(part_o + pb * kD + c);
    const float4 x0 = po[0], x1 = po[1];
    a2[0] += f * x0.x; a2[1] += f * x0.y; a2[2] += f * x0.z; a2[3] += f * x0.w;
    a2[4] += f * x1.x; a2[5] += f * x1.y; a2[6] += f * x1.z; a2[7] += f * x1.w;
  }
  const float inv = LL > 0.f ? 1.f / LL : 0.f;
  u32x4 ov;
#pragma unroll
  for (int j = 0; j < 4; ++j) ov[j] = pack2(a2[2 * j] * inv, a2[2 * j + 1] * inv);
  *reinterpret_cast<u32x4*>(out + ((size_t)(qs + qi2) * Hq + head2) * kD + c) = ov;
}

template <int G>
static void launch_fp8_g(void* out, float* part_o, float* part_ml, const void* q, const void* kc,
                         const void* vc, const void* ks, const void* vs, const int* bt, int bt_stride,
                         const int* tile_seq, const int* tile_q0, const int* q_start, const int* q_len,
                         const int* ctx_len, int num_tiles, int Hq, int Hkv, float scale_log2,
                         int part_tokens, int nparts, int num_blocks, int* sem, hipStream_t st) {
  dim3 grid(num_tiles, Hkv, nparts);
  // the bf16 kernel's load policy (attn_kv_nt op; below 8 query tiles the default policy)
  const int nt = num_tiles >= 8 ? attn_kv_nt(-1) : 0;
  auto kern = nt == 3 ? paged_attn_fp8_kernel<G, 3> : nt ? paged_attn_fp8_kernel<G, 1> : paged_attn_fp8_kernel<G, 0>;
  kern<<<grid, 256, 0, st>>>((uint16_t*)out, part_o, part_ml, (const uint16_t*)q, (const uint8_t*)kc,
                             (const uint8_t*)vc, (const uint8_t*)ks, (const uint8_t*)vs, bt, bt_stride,
                             tile_seq, tile_q0, q_start, q_len, ctx_len, Hq, Hkv, scale_log2, part_tokens,
                             nparts, num_blocks, sem);
  if (nparts > 1 && sem == nullptr)  // partials are fp32 whatever the KV dtype: the bf16 path's reduce
    launch_attn_reduce(out, part_o, part_ml, tile_seq, tile_q0, q_start, q_len, ctx_len, num_tiles, Hq, Hkv,
                       part_tokens, nparts, st);
}

void launch_paged_attention_fp8(void* out, float* part_o, float* part_ml, const void* q, const void* kc,
                                const void* vc, const void* ks, const void* vs, const int* bt,
                                int bt_stride, const int* tile_seq, const int* tile_q0, const int* q_start,
                                const int* q_len, const int* ctx_len, int num_tiles, int Hq, int Hkv,
                                float scale_log2, int part_tokens, int nparts, int num_blocks, int* sem,
                                hipStream_t st) {
  if (num_tiles == 0) return;
#define MLOP_ATTN8_CASE(GG)                                                                              \
  case GG:                                                                                               \
    launch_fp8_g<GG>(out, part_o, part_ml, q, kc, vc, ks, vs, bt, bt_stride, tile_seq, tile_q0, q_start, \
                     q_len, ctx_len, num_tiles, Hq, Hkv, scale_log2, part_tokens, nparts, num_blocks,    \
                     sem, st);                                                                           \
    break;
  switch (Hq / Hkv) {
    MLOP_ATTN8_CASE(1)
    MLOP_ATTN8_CASE(2)
    MLOP_ATTN8_CASE(4)
    MLOP_ATTN8_CASE(8)
    MLOP_ATTN8_CASE(16)
    default: break;
  }
#undef MLOP_ATTN8_CASE
}

}  // namespace mlop
