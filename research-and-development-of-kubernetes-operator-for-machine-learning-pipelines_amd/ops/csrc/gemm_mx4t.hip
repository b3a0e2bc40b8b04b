// K25: MXFP4 weights (W4A16) above the streaming kernel's 64 rows: one fused tiled MFMA GEMM, no
// dequantised scratch.
//
//   C[M, N] = epi(x[M, K] . W^T),   W as gemm_mx4.hip's (qw [N / 16, K / 128, 64, 4], qe [N / 16, K / 128, 16])
//
// gemm_mx4.hip splits K over a workgroup's waves, so every workgroup re-reads its 16 MT rows of A
// through L2 for 16 RB weight rows.  Here the four waves split N and share A through LDS:
//
//   * one workgroup (256 threads) = a 16 MT x 128 output tile (MT = 2 / 4 / 8, the smallest that
//     covers min(M, 128); the last M-tile ragged) over one K split; wave w owns the weight row
//     blocks 2 w and 2 w + 1 of the tile's 8;
//   * weights never touch LDS: per 128-wide K tile and row block one 16-B load + one 4-B scale
//     load per lane into a register ring S tiles deep, non-temporal when the launch has one M-tile
//     (each byte is read once) and cached otherwise (the other M-tiles' re-reads should hit L2);
//     the four mx4_word conversions of a tile write the four K-steps' B fragments in place;
//   * A: the 16 MT x 128 bf16 slab of a K tile (4 MT KiB) streams global -> LDS by LDS-DMA
//     (global_load_lds_dwordx4, MT instructions per wave and tile) into a ring of S stages that
//     marches with the weight ring: tile s + S - 1 is issued while tile s is consumed.  One raw
//     s_barrier per tile behind a COUNTED vmcnt (the loads of the S - 2 younger tiles stay in
//     flight; vmcnt is in order, so plain A loads staged through registers would have drained the
//     weight ring at every tile);
//   * LDS image: row r = 256 B, its 16-B chunk c at slot c ^ (r & 15), swizzled through the SOURCE
//     address of the DMA.  Lane l reads row l & 15, chunk 4 j + (l >> 4) of K-step j as one
//     ds_read_b128: 16 lanes = 16 different slots = all 64 banks once;
//   * K-step outermost, MT x 2 independent MFMAs per step into acc[MT][2] (64 registers at MT = 8);
//   * grid: 1-D, XCD-contiguous remap (gemm.hip), the M-tiles of one (weight tile, K split) adjacent
//     on one XCD;
//   * split-K (ks > 1): split s takes a contiguous range of the K / 128 tiles (sizes differ by at
//     most one, none empty) and stores its fp32 partials into slab [ks, M, N]; mx4_tile_reduce_kernel
//     sums the slabs in index order and applies the epilogue.  No atomics: a relaunch is bit-identical;
//   * epilogues: 0 = round to bf16; 1 = SiLU-mul over gate / up interleaved in blocks of 16 rows
//     (ops.interleave_gate_up): a wave's two row blocks are a gate block and its up block, a lane holds
//     the same (m, n mod 16) entry of both, rounds both to bf16 as the plain launch stores them and
//     writes mx4_silu(g) * u to column 16 (n / 32) + n mod 16 of [M, N / 2] (moe_mx4.hip's contract).
// Rows >= M read row M - 1 and are never stored; nothing in the grid depends on data.
#include "common.h"
#include "launch.h"
#include "mx4_cvt.h"

namespace mlop {

namespace {

constexpr int kStages = 4;  // LDS stages of A = register ring slots of the weights

template <int MT, int EPI, bool SPLIT, bool NT>
__global__ void __launch_bounds__(256) gemm_mx4_tile_kernel(const uint16_t* __restrict__ A, int lda,
                                                            const u32x4* __restrict__ qw,
                                                            const uint32_t* __restrict__ qe,
                                                            uint16_t* __restrict__ C, float* __restrict__ P, int M,
                                                            int N, int K, int mtiles, int ks) {
  constexpr int S = kStages, STAGE = MT * 4096, PER = MT + 4;  // bytes per stage; vm loads per wave and tile
  static_assert((S - 2) * PER < 64, "vmcnt is 6 bits");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-contiguous remap (gemm.hip): lids ordered (n-tile, split, m-tile), m-tile fastest
  const int Gd = gridDim.x, L = blockIdx.x;
  const int xq = Gd >> 3, xr = Gd & 7, xcd = L & 7, slot = L >> 3;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + slot;
  const int mt = lid % mtiles, sp = (lid / mtiles) % ks, nt = lid / (mtiles * ks);
  const int G = K >> 7;  // 128-wide tiles; this split's are [g0, g0 + n), n >= 1
  const int n = G / ks + (sp < G % ks), g0 = sp * (G / ks) + min(sp, G % ks);
  const int m0 = mt * 16 * MT;

  const u32x4* wp[2];
  const uint32_t* ep[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const size_t tile = (size_t)(8 * nt + 2 * wv + rb) * G + g0;
    wp[rb] = qw + tile * 64 + lane;
    ep[rb] = qe + tile * 16 + (lane & 15);
  }
  // DMA piece i of this wave = rows 16 i + 4 wv .. + 3 of the slab, 1 KiB of the stage; lane l fills
  // slot l & 15 of row 16 i + 4 wv + (l >> 4) with that row's chunk slot ^ (row & 15)
  const uint16_t* ap[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int row = 16 * i + 4 * wv + (lane >> 4);
    ap[i] = A + (size_t)min(m0 + row, M - 1) * lda + 128 * g0 + 8 * ((lane & 15) ^ (row & 15));
  }
  // fragment of K-step j, row tile t: byte 4096 t + fo[j] of the stage
  int fo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) fo[j] = 256 * (lane & 15) + 16 * ((4 * j + (lane >> 4)) ^ (lane & 15));

  f32x4 acc[MT][2];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 bq[S][2];
  uint32_t eq[S][2];
  auto issue = [&](int u, int s) {  // tile s into ring slot / stage u: weights first, then A
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      bq[u][rb] = NT ? __builtin_nontemporal_load(wp[rb] + 64 * s) : wp[rb][64 * s];
      eq[u][rb] = ep[rb][16 * s];
    }
#pragma unroll
    for (int i = 0; i < MT; ++i)
      __builtin_amdgcn_global_load_lds((const void*)(ap[i] + 128 * s),
                                       (lds_void_t*)(smem + u * STAGE + (4 * i + wv) * 1024), 16, 0, 0);
  };
  auto consume = [&](int u) {
    const uint8_t* sa = smem + u * STAGE;
    const u32x4 w0 = bq[u][0], w1 = bq[u][1];
    const uint32_t e0 = eq[u][0], e1 = eq[u][1];
    const bf16x8 b0[4] = {mx4_word(w0[0], mx4_scale<0>(e0)), mx4_word(w0[1], mx4_scale<1>(e0)),
                          mx4_word(w0[2], mx4_scale<2>(e0)), mx4_word(w0[3], mx4_scale<3>(e0))};
    const bf16x8 b1[4] = {mx4_word(w1[0], mx4_scale<0>(e1)), mx4_word(w1[1], mx4_scale<1>(e1)),
                          mx4_word(w1[2], mx4_scale<2>(e1)), mx4_word(w1[3], mx4_scale<3>(e1))};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bf16x8 a[MT];
#pragma unroll
      for (int t = 0; t < MT; ++t) a[t] = *reinterpret_cast<const bf16x8*>(sa + 4096 * t + fo[j]);
#pragma unroll
      for (int t = 0; t < MT; ++t) {
        acc[t][0] = mfma16(a[t], b0[j], acc[t][0]);
        acc[t][1] = mfma16(a[t], b1[j], acc[t][1]);
      }
    }
  };

#pragma unroll
  for (int t = 0; t < S - 1; ++t)
    if (t < n) issue(t, t);
  // tile s lives in slot s % S (s0 is a multiple of S).  Before tile s is read its loads must have
  // landed in every wave; behind them in the queue are the tiles s + 1 .. s + S - 2 (fewer at the end)
  int s0 = 0;
  for (; s0 + 2 * S <= n; s0 += S) {
#pragma unroll
    for (int u = 0; u < S; ++u) {
      wait_vmcnt<(S - 2) * PER>();
      raw_barrier();  // tile s visible to all waves; slot (s - 1) % S free in all of them
      issue((u + S - 1) % S, s0 + u + S - 1);
      consume(u);
    }
  }
#pragma unroll
  for (int i = 0; i < 2 * S; ++i) {
    const int s = s0 + i;
    if (s < n) {
      const int younger = n - s - 1;
      if (younger >= S - 2) wait_vmcnt<(S - 2) * PER>();
      else if (younger == 1) wait_vmcnt<PER>();
      else wait_vmcnt<0>();
      raw_barrier();
      if (s + S - 1 < n) issue((i + S - 1) % S, s + S - 1);
      consume(i % S);
    }
  }

  // lane: rows m0 + 16 t + 4 (lane >> 4) + r, weight rows 16 (8 nt + 2 wv + rb) + (lane & 15)
  const int col = 16 * (8 * nt + 2 * wv) + (lane & 15);
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = m0 + 16 * t + 4 * (lane >> 4) + r;
      if (m >= M) continue;
      if constexpr (SPLIT) {
        float* prow = P + ((size_t)sp * M + m) * N + col;
        prow[0] = acc[t][0][r];
        prow[16] = acc[t][1][r];
      } else if constexpr (EPI == 0) {
        uint16_t* crow = C + (size_t)m * N + col;
        crow[0] = f2bf(acc[t][0][r]);
        crow[16] = f2bf(acc[t][1][r]);
      } else {
        C[(size_t)m * (N >> 1) + 16 * (4 * nt + wv) + (lane & 15)] =
            f2bf(mx4_silu(acc[t][0][r]) * bf2f(f2bf(acc[t][1][r])));
      }
    }
}

// one thread = 4 adjacent output columns of one row: the ks partials summed in index order, then
// the epilogue (EPI 1: output column c is gate column 32 (c / 16) + c % 16 and the up column 16 on)
template <int EPI>
__global__ void __launch_bounds__(256) mx4_tile_reduce_kernel(const float* __restrict__ P, uint16_t* __restrict__ C,
                                                              int M, int N, int ks) {
  const int NO = EPI ? N >> 1 : N, per_row = NO >> 2;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long)M * per_row) return;
  const int m = (int)(i / per_row), c = 4 * (int)(i % per_row);
  const int src = EPI ? 32 * (c >> 4) + (c & 15) : c;
  const size_t slab = (size_t)M * N;
  const float* p = P + (size_t)m * N + src;
  f32x4 g = *reinterpret_cast<const f32x4*>(p), u = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (EPI) u = *reinterpret_cast<const f32x4*>(p + 16);
  for (int s = 1; s < ks; ++s) {
    g += *reinterpret_cast<const f32x4*>(p + s * slab);
    if constexpr (EPI) u += *reinterpret_cast<const f32x4*>(p + s * slab + 16);
  }
  u32x2 o;
  if constexpr (EPI) {
    o[0] = pack2(mx4_silu(g[0]) * bf2f(f2bf(u[0])), mx4_silu(g[1]) * bf2f(f2bf(u[1])));
    o[1] = pack2(mx4_silu(g[2]) * bf2f(f2bf(u[2])), mx4_silu(g[3]) * bf2f(f2bf(u[3])));
  } else {
    o[0] = pack2(g[0], g[1]);
    o[1] = pack2(g[2], g[3]);
  }
  *reinterpret_cast<u32x2*>(C + (size_t)m * NO + c) = o;
}

template <int MT, int EPI, bool SPLIT, bool NT>
void run_tile(const uint16_t* A, int lda, const u32x4* qw, const uint32_t* qe, uint16_t* C, float* P, int M, int N,
              int K, int mtiles, int ks, hipStream_t st) {
  constexpr int lds = kStages * MT * 4096;
  auto kern = gemm_mx4_tile_kernel<MT, EPI, SPLIT, NT>;
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr = true;
  }
  kern<<<(N / 128) * mtiles * ks, 256, lds, st>>>(A, lda, qw, qe, C, P, M, N, K, mtiles, ks);
}

template <int MT, bool NT>
void run_tile_epi(const uint16_t* A, int lda, const u32x4* qw, const uint32_t* qe, uint16_t* C, float* P, int M,
                  int N, int K, int mtiles, int ks, int epi, hipStream_t st) {
  if (ks > 1) run_tile<MT, 0, true, NT>(A, lda, qw, qe, C, P, M, N, K, mtiles, ks, st);
  else if (epi == 0) run_tile<MT, 0, false, NT>(A, lda, qw, qe, C, P, M, N, K, mtiles, ks, st);
  else run_tile<MT, 1, false, NT>(A, lda, qw, qe, C, P, M, N, K, mtiles, ks, st);
}

}  // namespace

int mx4_tile_mt(int M) { return M <= 32 ? 2 : M <= 64 ? 4 : 8; }

int mx4_tile_ks(int M, int N, int K) {
  if (M < 1 || N < 128 || N % 128 || K < 128 || K % 128) return 0;
  // measured (profiles/mxfp4_tile.md, bench_mx4.py tile, the forced-ks sweep on o and down): split
  // while the 128-wide tiles leave CUs idle (256 CUs), each split keeping at least 4 K tiles (the
  // ring's depth).  The best forced split was this one or within 4 % of it at every M from 32 to
  // 1024 on both shapes; capping the fp32 partials' traffic as well lost up to 45 % (o at 256 rows)
  const int tiles = (N / 128) * cdiv(M, 16 * mx4_tile_mt(M));
  const int ks = min(256 / tiles, (K >> 7) / 4);
  return ks < 1 ? 1 : ks;
}

bool launch_gemm_mx4_tile(const void* A, int lda, const void* qw, const void* qe, void* C, float* slab, int M, int N,
                          int K, int epi, int ks, hipStream_t st) {
  if (M < 1 || N < 128 || N % 128 || K < 128 || K % 128 || (epi != 0 && epi != 1)) return false;
  if (ks < 1 || ks > (K >> 7) || (ks > 1 && slab == nullptr)) return false;
  const int MT = mx4_tile_mt(M), mtiles = cdiv(M, 16 * MT);
  if ((long)(N / 128) * mtiles * ks > 0x7fffffffL) return false;
  auto* a = (const uint16_t*)A;
  auto* w = (const u32x4*)qw;
  auto* e = (const uint32_t*)qe;
  auto* c = (uint16_t*)C;
  if (MT == 2) run_tile_epi<2, true>(a, lda, w, e, c, slab, M, N, K, mtiles, ks, epi, st);
  else if (MT == 4) run_tile_epi<4, true>(a, lda, w, e, c, slab, M, N, K, mtiles, ks, epi, st);
  else if (mtiles == 1) run_tile_epi<8, true>(a, lda, w, e, c, slab, M, N, K, mtiles, ks, epi, st);
  else run_tile_epi<8, false>(a, lda, w, e, c, slab, M, N, K, mtiles, ks, epi, st);
  if (ks > 1) {
    const long threads = (long)M * ((epi ? N / 2 : N) / 4);
    const unsigned blocks = (unsigned)((threads + 255) / 256);
    if (epi == 0) mx4_tile_reduce_kernel<0><<<blocks, 256, 0, st>>>(slab, c, M, N, ks);
    else mx4_tile_reduce_kernel<1><<<blocks, 256, 0, st>>>(slab, c, M, N, ks);
  }
  return true;
}

}  // namespace mlop
