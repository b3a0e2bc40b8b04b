// K22: int4 weights (W4A16, symmetric, one bf16 scale per weight row and 128-wide K group).
//
//   C[M, N] = x[M, K] . W^T,   W[n, k] = s[n, k / 128] * q[n, k],  q in [-8, 7]      (1 <= M <= 64)
//
// A decode projection is weight streaming; this kernel streams a quarter of gemm_ws.hip's bytes.
// Device layout (ops.q4_pack): qw uint32 [N / 16, K / 128, 64, 4] -- one (16 rows x 128 k) tile is
// 1 KiB contiguous; lane l's 16 B hold weight row 16 nb + (l & 15), word j the lane's 8-element
// chunk of K-step j (k = 128 g + 32 j + 8 (l >> 4) .. + 7), which is exactly the lane's
// v_mfma_f32_16x16x32_bf16 B fragment of that step (common.h) -- and qs bf16 [N / 16, K / 128, 16],
// the tile's row scales.  A nibble stores u = q + 8; element e of a chunk sits at nibble
// (e >> 1) + 4 (e & 1), so (w >> 4 i) & 0x000f000f holds the adjacent elements 2 i, 2 i + 1 in the
// two halves of a dword.
//
//   * one workgroup = 16 x RB weight rows over the WHOLE K (RB: the largest of 4 / 2 / 1 that
//     leaves a workgroup per CU, launch_gemm_q4); its 4 waves take contiguous ranges of
//     the K / 128 groups whose sizes differ by at most one (a wave without a group adds zeros),
//     summed through LDS in a fixed wave order: no atomics, a relaunch is bit-identical;
//   * per group and row block: one non-temporal 16-B load per lane (the wave reads a whole
//     contiguous 1 KiB) + one scale load, U groups in flight in a register ring; the A fragments
//     come through L2 one group ahead (MT <= 2) or right behind the MFMAs that read them;
//   * dequantisation in registers is exact: w ^ 0x88888888 turns every nibble into q's two's
//     complement, v_bfe_i32 sign-extends it, v_cvt_f32_i32 + v_cvt_pk_bf16_f32 give q as bf16
//     (21 VALU per 8 weights; the 0x4300 | u magic needs 27: there is no packed bf16 add);
//   * 4 K-steps x MT MFMAs into a zeroed group accumulator, then acc += s * gacc with s the scale
//     of weight row lane & 15 -- the same index in the B operand and in the C layout.  The scale
//     never touches the bf16 operand: the MFMAs see exact integers (ref.gemm_q4's association).
// Rows >= M are computed from row M - 1 and never stored; nothing in the grid depends on data.
//
// q4_dequant_kernel: qw, qs -> bf16 [N, K] row-major, 16-B stores, bf16(float(s) * q) (the
// large-M route of ops.gemm_q4: dequantise into a scratch, then the bf16 GEMMs).
#include "common.h"
#include "launch.h"

namespace mlop {

namespace {

typedef __attribute__((ext_vector_type(2))) float q4_f32x2;
typedef __attribute__((ext_vector_type(2))) __bf16 q4_bf16x2;

// two floats -> one dword of two bf16 in ONE v_cvt_pk_bf16_f32 (common.h's pack2 takes two)
__device__ __forceinline__ uint32_t q4_pack2(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(q4_f32x2{lo, hi}, q4_bf16x2));
}

// the 8 weights of one packed word as the bf16x8 MFMA operand
__device__ __forceinline__ bf16x8 q4_word(uint32_t w) {
  const uint32_t x = w ^ 0x88888888u;  // u = q + 8 -> q's 4-bit two's complement
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // elements 2 i (nibble i) and 2 i + 1 (nibble i + 4)
    const float lo = (float)(((int)(x << (28 - 4 * i))) >> 28);
    const float hi = (float)(((int)(x << (12 - 4 * i))) >> 28);
    o[i] = q4_pack2(lo, hi);
  }
  return __builtin_bit_cast(bf16x8, o);
}

template <int MT, int RB, int U, int AS>
__global__ void __launch_bounds__(256) gemm_q4_kernel(const uint16_t* __restrict__ A, int lda,
                                                      const u32x4* __restrict__ qw,
                                                      const uint16_t* __restrict__ qs,
                                                      uint16_t* __restrict__ C, int ldc, int M, int K) {
  static_assert(U % AS == 0 && (AS == 1 || AS == 2), "static A slot per ring slot");
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int G = K >> 7;  // 128-wide groups; this wave's are [g0, g0 + n)
  const int n = G / 4 + (wv < G % 4), g0 = wv * (G / 4) + min(wv, G % 4);
  const int nb0 = blockIdx.x * RB;

  const u32x4* wp[RB];
  const uint16_t* sp[RB];
#pragma unroll
  for (int rb = 0; rb < RB; ++rb) {
    const size_t tile = (size_t)(nb0 + rb) * G + g0;
    wp[rb] = qw + tile * 64 + lane;
    sp[rb] = qs + tile * 16 + (lane & 15);
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
  uint16_t sq[U][RB];
  bf16x8 aq[AS][4][MT];
  auto load_w = [&](int u, int s) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      bq[u][rb] = __builtin_nontemporal_load(wp[rb] + 64 * s);
      sq[u][rb] = sp[rb][16 * s];
    }
  };
  auto load_a = [&](int a, int s) {  // group s: 128 k = 16 bf16x8 vectors, step j at + 4 j
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int t = 0; t < MT; ++t) aq[a][j][t] = ap[t][16 * s + 4 * j];
  };
  auto consume = [&](int u, int a) {
#pragma unroll
    for (int rb = 0; rb < RB; ++rb) {
      bf16x8 b[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = q4_word(bq[u][rb][j]);
      const float s = bf2f(sq[u][rb]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        f32x4 g = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) g = mfma16(aq[a][j][t], b[j], g);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][rb][r] += s * g[r];
      }
    }
  };
  // group s lives in ring slot s % U and A slot s % AS (s0 below is a multiple of U, so both are
  // compile-time).  The steady loop loads unconditionally (a guarded reload drains every load at
  // the top of each pass, gemm_ws.hip); only the prologue and the < 2 U tail groups are guarded.
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
__global__ void __launch_bounds__(256) q4_dequant_kernel(uint16_t* __restrict__ out,
                                                         const uint32_t* __restrict__ qw,
                                                         const uint16_t* __restrict__ qs, int N, int K) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;  // N K / 8 threads, a multiple of 256
  const int K8 = K >> 3, G = K >> 7;
  const int row = (int)(i / K8), c = (int)(i % K8);  // k = 8 c
  const int g = c >> 4, j = (c >> 2) & 3, lane = (row & 15) + 16 * (c & 3);
  const size_t tile = (size_t)(row >> 4) * G + g;
  const bf16x8 qv = q4_word(qw[(tile * 64 + lane) * 4 + j]);
  const float s = bf2f(qs[tile * 16 + (row & 15)]);
  u32x4 o;
#pragma unroll
  for (int e = 0; e < 4; ++e) o[e] = q4_pack2(s * bf2f_s(qv[2 * e]), s * bf2f_s(qv[2 * e + 1]));
  *reinterpret_cast<u32x4*>(out + (size_t)row * K + 8 * c) = o;
}

template <int MT, int RB>
void run_q4(const uint16_t* A, int lda, const u32x4* qw, const uint16_t* qs, uint16_t* C, int ldc, int M, int N,
            int K, hipStream_t st) {
  // MT <= 2: 4 groups in flight and the A fragments a group ahead; above, the A registers
  // (16 MT per slot) leave room for 2 and one A slot (no scratch in any instantiation)
  constexpr int U = MT <= 2 ? 4 : 2, AS = MT <= 2 ? 2 : 1;
  gemm_q4_kernel<MT, RB, U, AS><<<N / (16 * RB), 256, 0, st>>>(A, lda, qw, qs, C, ldc, M, K);
}

template <int RB>
void run_q4_rb(const uint16_t* A, int lda, const u32x4* qw, const uint16_t* qs, uint16_t* C, int ldc, int M, int N,
               int K, hipStream_t st) {
  switch ((M + 15) >> 4) {
    case 1: run_q4<1, RB>(A, lda, qw, qs, C, ldc, M, N, K, st); break;
    case 2: run_q4<2, RB>(A, lda, qw, qs, C, ldc, M, N, K, st); break;
    case 3: run_q4<3, RB>(A, lda, qw, qs, C, ldc, M, N, K, st); break;
    default: run_q4<4, RB>(A, lda, qw, qs, C, ldc, M, N, K, st); break;
  }
}

}  // namespace

bool launch_gemm_q4(const void* A, int lda, const void* qw, const void* qs, void* C, int ldc, int M, int N, int K,
                    int rb, hipStream_t st) {
  if (M < 1 || M > 64 || N < 16 || N % 16 || K < 128 || K % 128) return false;
  if (rb != 0 && ((rb != 1 && rb != 2 && rb != 4) || N % (16 * rb))) return false;
  // rb 0: the largest RB of {4, 2, 1} that still leaves a workgroup per CU (256).  Measured
  // (profiles/int4_weights.md): a workgroup is a serial chain of dependent load -> dequantise ->
  // MFMA groups, so o / qkv / down (N = 4096 .. 6144) at RB = 4 are 64-96 workgroups of latency,
  // not a weight stream; gate_up (N = 28672) keeps RB = 4 and its 4x fewer A reads
  if (rb == 0) rb = N % 64 == 0 && N / 64 >= 256 ? 4 : N % 32 == 0 && N / 32 >= 256 ? 2 : 1;
  auto* a = (const uint16_t*)A;
  auto* w = (const u32x4*)qw;
  auto* s = (const uint16_t*)qs;
  auto* c = (uint16_t*)C;
  if (rb == 4) run_q4_rb<4>(a, lda, w, s, c, ldc, M, N, K, st);
  else if (rb == 2) run_q4_rb<2>(a, lda, w, s, c, ldc, M, N, K, st);
  else run_q4_rb<1>(a, lda, w, s, c, ldc, M, N, K, st);
  return true;
}

bool launch_q4_dequant(void* out, const void* qw, const void* qs, int N, int K, hipStream_t st) {
  if (N < 16 || N % 16 || K < 128 || K % 128) return false;
  const long blocks = (long)N * K / 8 / 256;
  if (blocks > 0x7fffffffL) return false;
  q4_dequant_kernel<<<(unsigned)blocks, 256, 0, st>>>((uint16_t*)out, (const uint32_t*)qw, (const uint16_t*)qs, N, K);
  return true;
}

}  // namespace mlop
