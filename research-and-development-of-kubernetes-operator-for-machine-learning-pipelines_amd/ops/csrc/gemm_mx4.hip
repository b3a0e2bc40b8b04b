// K23: MXFP4 weights (W4A16, OCP microscaling: e2m1 codes, one e8m0 scale byte per weight row and
// 32 consecutive k).
//
//   C[M, N] = x[M, K] . W^T,   W[n, k] = 2^(e[n, k / 32] - 127) * grid[code[n, k]]     (1 <= M <= 64)
//
// Every W[n, k] is a normal bf16 (e in [2, 252], ops/reference.py "mxfp4 weights"), so the matrix
// cores take the scaled weights themselves: no group accumulator, no fp32 scale multiply, and a
// scale group is exactly one K-step of v_mfma_f32_16x16x32_bf16.
// Device layout (ops.mx4_pack): qw uint32 [N / 16, K / 128, 64, 4] -- one (16 rows x 128 k) tile is
// 1 KiB contiguous; lane l's 16 B hold weight row 16 nb + (l & 15), word j the 8 codes of K-step j
// (k = 128 g + 32 j + 8 (l >> 4) .. + 7), code i at nibble i -- and qe uint32 [N / 16, K / 128, 16],
// the four scale bytes of a row in that tile, K-step j at byte j.
//
//   * conversion: v_cvt_scalef32_pk_bf16_fp4 turns one byte (two codes) and an f32 scale into two
//     scaled bf16; the four byte selects of word j write the four dwords of the lane's B fragment of
//     K-step j in place.  The f32 scale is the byte shifted into the exponent field (e << 23):
//     6 VALU per 8 weights where the int4 kernel spends 21;
//   * one workgroup = 16 x RB weight rows over the WHOLE K; its 4 waves take contiguous ranges of
//     the K / 128 tiles whose sizes differ by at most one (a wave without a tile adds zeros),
//     summed through LDS in a fixed wave order: no atomics, a relaunch is bit-identical;
//   * per tile and row block: one non-temporal 16-B load per lane (the wave reads a whole
//     contiguous 1 KiB) + one 4-B scale load, U tiles in flight in a register ring (8 at RB = 1,
//     4 above, at every MT); the A fragments come through L2 one tile ahead (MT <= 2) or right
//     behind the MFMAs that read them;
//   * 4 K-steps x MT MFMAs straight into acc, K-step outermost so that back-to-back MFMAs are
//     independent.
// Rows >= M are computed from row M - 1 and never stored; nothing in the grid depends on data.
//
// mx4_dequant_kernel: qw, qe -> bf16 [N, K] row-major, 16-B stores, the same conversion (the
// large-M route of ops.gemm_mx4: dequantise into a scratch, then the bf16 GEMMs).
#include "common.h"
#include "launch.h"
#include "mx4_cvt.h"  // mx4_scale, mx4_word (shared with moe_mx4.hip)

namespace mlop {

namespace {

template <int MT, int RB, int U, int AS>
__global__ void __launch_bounds__(256) gemm_mx4_kernel(const uint16_t* __restrict__ A, int lda,
                                                       const u32x4* __restrict__ qw,
                                                       const uint32_t* __restrict__ qe,
                                                       uint16_t* __restrict__ C, int ldc, int M, int K) {
  static_assert(U % AS == 0 && (AS == 1 || AS == 2), "static A slot per ring slot");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = K >> 7;  // 128-wide tiles; this wave's are [g0, g0 + n)
  const int n = G / 4 + (wv < G % 4), g0 = wv * (G / 4) + min(wv, G % 4);
  const int nb0 = blockIdx.x * RB;

  const u32x4* wp[RB];
  const uint32_t* ep[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const size_t tile = (size_t)(nb0 + rb) * G + g0;
    wp[rb] = qw + tile * 64 + lane;
    ep[rb] = qe + tile * 16 + (lane & 15);
  }
  const bf16x8* ap[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t)  // rows past M read row M - 1: their outputs are never stored
    ap[t] = reinterpret_cast<const bf16x8*>(A + (size_t)min(16 * t + (lane & 15), M - 1) * lda + 128 * g0 +
                                            8 * (lane >> 4));

  f32x4 acc[MT][RB];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) acc[t][rb] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 bq[U][RB];
  uint32_t eq[U][RB];
  bf16x8 aq[AS][4][MT];
  auto load_w = [&](int u, int s) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      bq[u][rb] = __builtin_nontemporal_load(wp[rb] + 64 * s);
      eq[u][rb] = ep[rb][16 * s];
    }
  };
  auto load_a = [&](int a, int s) {  // tile s: 128 k = 16 bf16x8 vectors, step j at + 4 j
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t) aq[a][j][t] = ap[t][16 * s + 4 * j];
  };
  auto consume = [&](int u, int a) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const u32x4 w = bq[u][rb];
      const uint32_t ew = eq[u][rb];
      const bf16x8 b[4] = {mx4_word(w[0], mx4_scale<0>(ew)), mx4_word(w[1], mx4_scale<1>(ew)),
                           mx4_word(w[2], mx4_scale<2>(ew)), mx4_word(w[3], mx4_scale<3>(ew))};
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t][rb] = mfma16(aq[a][j][t], b[j], acc[t][rb]);
    }
  };
  // tile s lives in ring slot s % U and A slot s % AS (s0 below is a multiple of U, so both are
  // compile-time).  The steady loop loads unconditionally (a guarded reload drains every load at
  // the top of each pass, gemm_ws.hip); only the prologue and the < 2 U tail tiles are guarded.
  if (n > 0) {
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (u < n) load_w(u, u);
    load_a(0, 0);
    int s0 = 0;
    for (; s0 + 2 * U <= n; s0 += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if constexpr (AS == 2) load_a((u + 1) % AS, s0 + u + 1);
        consume(u, u % AS);
        if constexpr (AS == 1) load_a(0, s0 + u + 1);
        load_w(u, s0 + u + U);
      }
    }
#pragma unroll
    for (int i = 0; i < 2 * U; ++i) {
      const int s = s0 + i;
      if (s < n) {
        if constexpr (AS == 2) {
          if (s + 1 < n) load_a((i + 1) % AS, s + 1);
        }
        consume(i % U, i % AS);
        if constexpr (AS == 1) {
          if (s + 1 < n) load_a(0, s + 1);
        }
        if (s + U < n) load_w(i % U, s + U);
      }
    }
  }

  // combine the 4 waves' partials: red[w][(t RB + rb) 4 + r][lane], summed in a fixed order
  __shared__ float red[4][MT * RB * 4][64];
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wv][(t * RB + rb) * 4 + r][lane] = acc[t][rb][r];
  __syncthreads();
  // thread (w', lane) finishes fragment element r = w' of every (t, rb) block: output row
  // m = 16 t + 4 (lane >> 4) + r, weight row 16 (nb0 + rb) + (lane & 15)
  const int r = wv;
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + 4 * (lane >> 4) + r;
    if (m >= M) continue;
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      const int idx = (t * RB + rb) * 4 + r;
      const float y = (red[0][idx][lane] + red[1][idx][lane]) + (red[2][idx][lane] + red[3][idx][lane]);
      C[(size_t)m * ldc + 16 * (nb0 + rb) + (lane & 15)] = f2bf(y);
    }
  }
}

// one thread = one packed word = 8 consecutive k of one weight row = one 16-B store; consecutive
// threads walk a row, so a wave stores 1 KiB contiguous
__global__ void __launch_bounds__(256) mx4_dequant_kernel(uint16_t* __restrict__ out,
                                                          const uint32_t* __restrict__ qw,
                                                          const uint32_t* __restrict__ qe, int N, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // N K / 8 threads, a multiple of 256
  const int K8 = K >> 3, G = K >> 7;
  const int row = (int)(i / K8), c = (int)(i % K8);  // k = 8 c
  const int g = c >> 4, j = (c >> 2) & 3, lane = (row & 15) + 16 * (c & 3);
  const size_t tile = (size_t)(row >> 4) * G + g;
  const float scale = __uint_as_float(((qe[tile * 16 + (row & 15)] >> (8 * j)) & 0xffu) << 23);
  *reinterpret_cast<bf16x8*>(out + (size_t)row * K + 8 * c) = mx4_word(qw[(tile * 64 + lane) * 4 + j], scale);
}

template <int MT, int RB>
void run_mx4(const uint16_t* A, int lda, const u32x4* qw, const uint32_t* qe, uint16_t* C, int ldc, int M, int N,
             int K, hipStream_t st) {
  // 8 KiB of weights in flight per wave at RB = 1, 16 KiB above, at every MT; the A fragments
  // (16 MT registers per slot) a tile ahead for MT <= 2 (no scratch in any instantiation)
  constexpr int U = RB == 1 ? 8 : 4, AS = MT <= 2 ? 2 : 1;
  gemm_mx4_kernel<MT, RB, U, AS><<<N / (16 * RB), 256, 0, st>>>(A, lda, qw, qe, C, ldc, M, K);
}

template <int RB>
void run_mx4_rb(const uint16_t* A, int lda, const u32x4* qw, const uint32_t* qe, uint16_t* C, int ldc, int M, int N,
                int K, hipStream_t st) {
  switch ((M + 15) >> 4) {
    case 1: run_mx4<1, RB>(A, lda, qw, qe, C, ldc, M, N, K, st); break;
    case 2: run_mx4<2, RB>(A, lda, qw, qe, C, ldc, M, N, K, st); break;
    case 3: run_mx4<3, RB>(A, lda, qw, qe, C, ldc, M, N, K, st); break;
    default: run_mx4<4, RB>(A, lda, qw, qe, C, ldc, M, N, K, st); break;
  }
}

}  // namespace

bool launch_gemm_mx4(const void* A, int lda, const void* qw, const void* qe, void* C, int ldc, int M, int N, int K,
                     int rb, hipStream_t st) {
  if (M < 1 || M > 64 || N < 16 || N % 16 || K < 128 || K % 128) return false;
  if (rb != 0 && ((rb != 1 && rb != 2 && rb != 4) || N % (16 * rb))) return false;
  // rb 0, measured (profiles/mxfp4_weights.md, bench_mx4.py rb): the largest RB of {4, 2, 1} that
  // leaves 192 workgroups up to 16 rows and 128 above, where the A fragments (16 MT registers per
  // tile, re-read by every workgroup) weigh more than idle CUs.  Up to 16 rows RB = 4 also wants
  // its workgroups resident at once (2 per CU by registers = 512): 70B's gate_up (896) ran 17 %
  // slower at one row with RB = 4 than with RB = 2
  if (rb == 0) {
    const int floor_wg = M <= 16 ? 192 : 128;
    const bool rb4 = N % 64 == 0 && N / 64 >= floor_wg && (M > 16 || N / 64 <= 512);
    rb = rb4 ? 4 : N % 32 == 0 && N / 32 >= floor_wg ? 2 : 1;
  }
  auto* a = (const uint16_t*)A;
  auto* w = (const u32x4*)qw;
  auto* e = (const uint32_t*)qe;
  auto* c = (uint16_t*)C;
  if (rb == 4) run_mx4_rb<4>(a, lda, w, e, c, ldc, M, N, K, st);
  else if (rb == 2) run_mx4_rb<2>(a, lda, w, e, c, ldc, M, N, K, st);
  else run_mx4_rb<1>(a, lda, w, e, c, ldc, M, N, K, st);
  return true;
}

bool launch_mx4_dequant(void* out, const void* qw, const void* qe, int N, int K, hipStream_t st) {
  if (N < 16 || N % 16 || K < 128 || K % 128) return false;
  const long blocks = (long)N * K / 8 / 256;
  if (blocks > 0x7fffffffL) return false;
  mx4_dequant_kernel<<<(unsigned)blocks, 256, 0, st>>>((uint16_t*)out, (const uint32_t*)qw, (const uint32_t*)qe, N, K);
  return true;
}

}  // namespace mlop
