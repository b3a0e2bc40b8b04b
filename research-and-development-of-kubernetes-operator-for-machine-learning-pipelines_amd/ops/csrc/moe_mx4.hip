// K24: MXFP4 expert weights (W4A16) for MoE layers: the grouped form of gemm_mx4.hip.
//
//   per expert e:  C[off[e] .. off[e+1], :] = A[those rows] . dequant(W[e])^T      (one launch)
//
// Storage (ops.Mx4Experts): qw uint32 [E, N / 16, K / 128, 64, 4], qe uint32 [E, N / 16, K / 128, 16]:
// gemm_mx4.hip's tile layout with the expert outermost, i.e. the packing of the stacked [E N, K]
// matrix, so mx4_dequant_kernel dequantises a whole layer's experts as it stands.
//
//   * grid = (N / (16 RB), E), a pure function of the shapes: nothing is read back to the host;
//   * a workgroup = one expert x 16 RB weight rows over the WHOLE K.  It reads its expert's two
//     offsets first and returns on an empty expert before touching a weight byte (Qwen3-MoE at
//     batch 1 reads 8 experts of 128);
//   * an expert's rows are walked in chunks of 64 inside the workgroup (any routing skew is
//     correct; a chunk re-reads the workgroup's weights, from L2 where they fit); the chunk's
//     row-tile count (1..4 tiles of 16) is a wave-uniform switch into MT-specialised bodies;
//   * the body is gemm_mx4_kernel's: four waves over balanced ranges of the 128-wide tiles,
//     non-temporal 16-B weight loads in a register ring (8 tiles at RB = 1, 4 above),
//     v_cvt_scalef32_pk_bf16_fp4 straight into the v_mfma_f32_16x16x32_bf16 B fragment, partials
//     summed through LDS in a fixed wave order: no atomics, a relaunch is bit-identical;
//   * A rows come gathered (row r of A) or through a row map (row a_rows[r] of A: the token rows
//     of moe_dispatch_mid / moe_dispatch_wide).  Rows past the chunk's last row read that last
//     row and are never stored;
//   * EPI 1 = SiLU-mul in the combine.  w13's rows are gate / up interleaved in groups of 16
//     (ops.interleave_gate_up), so row block 2 p holds 16 gates and row block 2 p + 1 their ups:
//     with RB even the thread that finishes (row, lane) of block 2 p also sums the same entry of
//     block 2 p + 1, rounds both to bf16 as the unfused path stores them, and writes
//     silu(g) * u to column 16 p + (lane & 15) of the [R, N / 2] output.  silu is mx4_cvt.h's mx4_silu:
//     common.h's silu_bf except for gates in (-88.7, -87.3), where that one's reciprocal is a
//     denormal that v_rcp_f32 flushes (silu = -0 where fp32 division gives about -1e-36).
#include "common.h"
#include "launch.h"
#include "mx4_cvt.h"

namespace mlop {

namespace {

// one chunk of <= 16 MT rows (rows m0 .. m0 + rows of the permuted order) against the expert's
// row blocks nb0 .. nb0 + RB; red is the workgroup's LDS, [wave][(t RB + rb) 4 + r][lane]
template <int MT, int RB, int EPI>
__device__ __forceinline__ void moe_mx4_chunk(const uint16_t* __restrict__ A, int lda, const int* __restrict__ a_rows,
                                              const u32x4* __restrict__ qw, const uint32_t* __restrict__ qe,
                                              uint16_t* __restrict__ C, int ldc, int m0, int rows, int K, int nb0,
                                              float (*red)[16 * RB][64]) {
  constexpr int U = RB == 1 ? 8 : 4, AS = MT <= 2 ? 2 : 1;  // gemm_mx4.hip's ring (no scratch at any MT)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = K >> 7;  // 128-wide tiles; this wave's are [g0, g0 + n)
  const int n = G / 4 + (wv < G % 4), g0 = wv * (G / 4) + min(wv, G % 4);

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
  for (int t = 0; t < MT; ++t) {  // rows past the chunk read its last row: never stored
    const int r = m0 + min(16 * t + (lane & 15), rows - 1);
    const int src = a_rows ? a_rows[r] : r;
    ap[t] = reinterpret_cast<const bf16x8*>(A + (size_t)src * lda + 128 * g0 + 8 * (lane >> 4));
  }

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
  // tile s lives in ring slot s % U and A slot s % AS (s0 is a multiple of U); the steady loop
  // loads unconditionally, only the prologue and the < 2 U tail tiles are guarded
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

#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int rb = 0; rb < RB; ++rb)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wv][(t * RB + rb) * 4 + r][lane] = acc[t][rb][r];
  __syncthreads();
  // thread (w', lane) finishes fragment element r = w' of every (t, rb) block: chunk row
  // m = 16 t + 4 (lane >> 4) + r, weight row 16 (nb0 + rb) + (lane & 15)
  const int r = wv;
  auto total = [&](int idx) {
    return (red[0][idx][lane] + red[1][idx][lane]) + (red[2][idx][lane] + red[3][idx][lane]);
  };
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = 16 * t + 4 * (lane >> 4) + r;
    if (m >= rows) continue;
    uint16_t* crow = C + (size_t)(m0 + m) * ldc;
    if constexpr (EPI == 0) {
#pragma unroll
      for (int rb = 0; rb < RB; ++rb) crow[16 * (nb0 + rb) + (lane & 15)] = f2bf(total((t * RB + rb) * 4 + r));
    } else {
      static_assert(RB % 2 == 0, "a gate block and its up block sit in one workgroup");
#pragma unroll
      for (int p = 0; p < RB / 2; ++p) {
        const float g = total((t * RB + 2 * p) * 4 + r), u = total((t * RB + 2 * p + 1) * 4 + r);
        crow[8 * (nb0 + 2 * p) + (lane & 15)] = f2bf(mx4_silu(g) * bf2f(f2bf(u)));
      }
    }
  }
}

template <int RB, int EPI>
__global__ void __launch_bounds__(256) moe_mx4_kernel(const uint16_t* __restrict__ A, int lda,
                                                      const int* __restrict__ a_rows,
                                                      const u32x4* __restrict__ qw,
                                                      const uint32_t* __restrict__ qe,
                                                      const int* __restrict__ offsets,
                                                      uint16_t* __restrict__ C, int ldc, int N, int K) {
  __shared__ float red[4][16 * RB][64];
  const int e = blockIdx.y;
  const int off0 = offsets[e], off1 = offsets[e + 1];
  if (off1 <= off0) return;  // an expert without rows: no weight byte is read
  const size_t tiles = (size_t)e * (N >> 4) * (K >> 7);  // the expert's first tile
  const u32x4* qw_e = qw + tiles * 64;
  const uint32_t* qe_e = qe + tiles * 16;
  const int nb0 = blockIdx.x * RB;
  for (int m0 = off0; m0 < off1; m0 += 64) {
    if (m0 != off0) __syncthreads();  // the previous chunk's combine has read red
    const int rows = min(64, off1 - m0);
    switch ((rows + 15) >> 4) {
      case 1: moe_mx4_chunk<1, RB, EPI>(A, lda, a_rows, qw_e, qe_e, C, ldc, m0, rows, K, nb0, red); break;
      case 2: moe_mx4_chunk<2, RB, EPI>(A, lda, a_rows, qw_e, qe_e, C, ldc, m0, rows, K, nb0, red); break;
      case 3: moe_mx4_chunk<3, RB, EPI>(A, lda, a_rows, qw_e, qe_e, C, ldc, m0, rows, K, nb0, red); break;
      default: moe_mx4_chunk<4, RB, EPI>(A, lda, a_rows, qw_e, qe_e, C, ldc, m0, rows, K, nb0, red); break;
    }
  }
}

}  // namespace

int moe_mx4_rb(int R, int E, int N, int epi) {
  // the largest RB of {4, 2, 1} that leaves 256 workgroups on experts that can have rows (at most
  // min(E, R) of them); the SiLU-mul form needs a gate block and its up block together (RB >= 2)
  const int live = R < E ? (R < 1 ? 1 : R) : E;
  const int floor_rb = epi ? 2 : 1;
  for (int rb = 4; rb > floor_rb; rb >>= 1)
    if (N % (16 * rb) == 0 && (long)live * (N / (16 * rb)) >= 256) return rb;
  return floor_rb;
}

bool launch_moe_mx4(const void* A, int lda, const int* a_rows, const void* qw, const void* qe, const int* offsets,
                    void* C, int ldc, int R, int E, int N, int K, int epi, int rb, hipStream_t st) {
  if (E < 1 || E > 65535 || N < 16 || N % 16 || K < 128 || K % 128 || (epi != 0 && epi != 1)) return false;
  if (epi == 1 && N % 32) return false;
  if (rb == 0) rb = moe_mx4_rb(R, E, N, epi);
  if ((rb != 1 && rb != 2 && rb != 4) || N % (16 * rb) || (epi == 1 && rb == 1)) return false;
  if (R < 1) return true;
  auto* a = (const uint16_t*)A;
  auto* w = (const u32x4*)qw;
  auto* s = (const uint32_t*)qe;
  auto* c = (uint16_t*)C;
  const dim3 grid(N / (16 * rb), E);
#define MLOP_MOE_MX4(RB_, EPI_) \
  moe_mx4_kernel<RB_, EPI_><<<grid, 256, 0, st>>>(a, lda, a_rows, w, s, offsets, c, ldc, N, K)
  if (epi == 0) {
    if (rb == 4) MLOP_MOE_MX4(4, 0);
    else if (rb == 2) MLOP_MOE_MX4(2, 0);
    else MLOP_MOE_MX4(1, 0);
  } else {
    if (rb == 4) MLOP_MOE_MX4(4, 1);
    else MLOP_MOE_MX4(2, 1);
  }
#undef MLOP_MOE_MX4
  return true;
}

}  // namespace mlop
