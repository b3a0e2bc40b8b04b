// K26: MXFP4 expert weights (W4A16) above the streaming kernel's 64 rows per expert: gemm_mx4t.hip's
// fused tile in ONE grouped launch over ops.Mx4Experts, no dequantised scratch.
//
//   per expert e:  C[off[e] .. off[e+1], :] = epi(A[those rows] . dequant(W[e])^T)
//
// moe_mx4.hip walks an expert in 64-row chunks and converts the workgroup's weights again for every
// chunk; here a workgroup converts a weight tile once for up to 16 MT = 128 rows:
//
//   * one workgroup (256 threads) = one 16 MT x 128 output tile of one expert over the whole K; wave
//     w owns the weight row blocks 2 w and 2 w + 1 of the tile's 8;
//   * grid: 1-D, (N / 128) x (R / (16 MT) + min(E, R)) workgroups, a pure function of the shapes: the
//     second factor bounds sum_e cdiv(rows_e, 16 MT) for any routing.  XCD-contiguous remap
//     (gemm.hip), the M-tile index fastest: the M-tiles of one (expert, weight tile) are adjacent
//     on one XCD and re-read its weights from L2;
//   * a workgroup finds (expert, first row, rows) of its global M-tile index from offsets itself:
//     every wave scans cdiv(rows_e, 16 MT) over slices of 64 experts (one expert per lane, a
//     shuffle prefix sum, a ballot for the owner).  An index past the total, which covers every
//     M-tile of an expert without rows, returns before a weight byte is read;
//   * the tile's live row tiles LT = cdiv(rows, 16) (the expert may end inside the tile) is a
//     wave-uniform switch into LT-specialised bodies: row tiles >= LT cost no DMA, no ds_read, no
//     MFMA and no accumulator, so an expert of 65 rows pays for 80, not 128;
//   * weights never touch LDS: per 128-wide K tile and row block one 16-B load + one 4-B scale
//     load per lane into a register ring S tiles deep (cached loads: another M-tile of the expert
//     may re-read them), the four mx4_word conversions of a tile write the four K-steps' B
//     fragments in place;
//   * A: the 16 LT x 128 bf16 slab of a K tile streams global -> LDS by LDS-DMA
//     (global_load_lds_dwordx4, LT instructions per wave and tile) into a ring of S stages that
//     marches with the weight ring; one raw s_barrier per tile behind a COUNTED vmcnt.  The DMA takes
//     a per-lane source address, so the row map (a_rows: the token rows of moe_dispatch_mid /
//     moe_dispatch_wide) costs one index load per DMA row at kernel start and no gathered copy;
//   * LDS image (gemm_mx4t.hip's): row r = 256 B, its 16-B chunk c at slot c ^ (r & 15), swizzled
//     through the SOURCE address of the DMA; every ds_read_b128 fragment read is conflict-free;
//   * rows past the tile's last row read that last row (in bounds) and are never stored: they
//     belong to the next expert.  Rows behind offsets[E] are untouched;
//   * no split-K, no atomics: a relaunch is bit-identical;
//   * epilogues: 0 = round to bf16; 1 = SiLU-mul over gate / up interleaved in blocks of 16 rows: a
//     wave's two row blocks are a gate block and its up block, both rounded to bf16 as the plain
//     launch stores them, mx4_silu(g) * u to column 16 (n / 32) + n mod 16 of [R, N / 2]
//     (moe_mx4.hip's contract).
#include "common.h"
#include "launch.h"
#include "mx4_cvt.h"

namespace mlop {

namespace {

constexpr int kStages = 4;  // LDS stages of A = register ring slots of the weights
constexpr int kMT = 8;      // row tiles of 16 per M-tile

// LT live row tiles (rows m0 .. m0 + rows, 16 (LT - 1) < rows <= 16 LT) against the weight row blocks
// 8 nt + 2 wv, + 1 of expert tile base qw / qe (already offset to the expert)
template <int LT, int EPI>
__device__ __forceinline__ void moe_mx4_tile_body(const uint16_t* __restrict__ A, int lda,
                                                  const int* __restrict__ a_rows, const u32x4* __restrict__ qw,
                                                  const uint32_t* __restrict__ qe, uint16_t* __restrict__ C, int m0,
                                                  int rows, int N, int K, int nt, uint8_t* smem) {
  constexpr int S = kStages, STAGE = LT * 4096, PER = LT + 4;  // bytes per stage; vm loads per wave and tile
  static_assert((S - 2) * PER < 64, "vmcnt is 6 bits");
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int n = K >> 7;  // 128-wide K tiles

  const u32x4* wp[2];
  const uint32_t* ep[2];
#pragma unroll
  for (int rb = 0; rb < 2; ++rb) {
    const size_t tile = (size_t)(8 * nt + 2 * wv + rb) * n;
    wp[rb] = qw + tile * 64 + lane;
    ep[rb] = qe + tile * 16 + (lane & 15);
  }
  // DMA piece i of this wave = rows 16 i + 4 wv .. + 3 of the slab, 1 KiB of the stage; lane l fills
  // slot l & 15 of row 16 i + 4 wv + (l >> 4) with that row's chunk slot ^ (row & 15)
  const uint16_t* ap[LT];
#pragma unroll
  for (int i = 0; i < LT; ++i) {
    const int row = 16 * i + 4 * wv + (lane >> 4);
    const int r = m0 + min(row, rows - 1);
    const int src = a_rows ? a_rows[r] : r;
    ap[i] = A + (size_t)src * lda + 8 * ((lane & 15) ^ (row & 15));
  }
  // fragment of K-step j, row tile t: byte 4096 t + fo[j] of the stage
  int fo[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) fo[j] = 256 * (lane & 15) + 16 * ((4 * j + (lane >> 4)) ^ (lane & 15));

  f32x4 acc[LT][2];
#pragma unroll
  for (int t = 0; t < LT; ++t) acc[t][0] = acc[t][1] = f32x4{0.f, 0.f, 0.f, 0.f};

  u32x4 bq[S][2];
  uint32_t eq[S][2];
  auto issue = [&](int u, int s) {  // tile s into ring slot / stage u: weights first, then A
#pragma unroll
    for (int rb = 0; rb < 2; ++rb) {
      bq[u][rb] = wp[rb][64 * s];
      eq[u][rb] = ep[rb][16 * s];
    }
#pragma unroll
    for (int i = 0; i < LT; ++i)
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
      bf16x8 a[LT];
#pragma unroll
      for (int t = 0; t < LT; ++t) a[t] = *reinterpret_cast<const bf16x8*>(sa + 4096 * t + fo[j]);
#pragma unroll
      for (int t = 0; t < LT; ++t) {
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
  for (int t = 0; t < LT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int m = 16 * t + 4 * (lane >> 4) + r;
      if (m >= rows) continue;
      if constexpr (EPI == 0) {
        uint16_t* crow = C + (size_t)(m0 + m) * N + col;
        crow[0] = f2bf(acc[t][0][r]);
        crow[16] = f2bf(acc[t][1][r]);
      } else {
        C[(size_t)(m0 + m) * (N >> 1) + 16 * (4 * nt + wv) + (lane & 15)] =
            f2bf(mx4_silu(acc[t][0][r]) * bf2f(f2bf(acc[t][1][r])));
      }
    }
}

template <int MT, int EPI>
__global__ void __launch_bounds__(256) moe_mx4_tile_kernel(const uint16_t* __restrict__ A, int lda,
                                                           const int* __restrict__ a_rows,
                                                           const u32x4* __restrict__ qw,
                                                           const uint32_t* __restrict__ qe,
                                                           const int* __restrict__ offsets,
                                                           uint16_t* __restrict__ C, int E, int N, int K,
                                                           int mtiles) {
  static_assert(MT == 8, "the LT switch below lists 8 bodies");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  constexpr int TM = 16 * MT;
  const int lane = threadIdx.x & 63;
  // XCD-contiguous remap (gemm.hip): lids ordered (n-tile, m-tile), m-tile fastest
  const int Gd = gridDim.x, L = blockIdx.x;
  const int xq = Gd >> 3, xr = Gd & 7, xcd = L & 7, slot = L >> 3;
  const int lid = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + slot;
  const int mt = lid % mtiles, nt = lid / mtiles;

  // M-tile mt of the launch = M-tile (mt - tiles before expert e) of the expert e whose inclusive
  // tile count first exceeds mt; every wave finds it for itself, lane i of a slice = expert s + i
  int e = -1, m0 = 0, rows = 0;
  for (int s = 0, before = 0; s < E; s += 64) {
    const int i = min(s + lane, E - 1);
    const int o0 = offsets[i], o1 = offsets[i + 1];
    const int cnt = s + lane < E && o1 > o0 ? (o1 - o0 + TM - 1) / TM : 0;
    int incl = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_up(incl, d);
      if (lane >= d) incl += v;
    }
    const unsigned long long owners = __ballot(before + incl > mt);
    if (owners) {
      const int f = __ffsll(owners) - 1;
      const int first = __builtin_amdgcn_readfirstlane(__shfl(o0, f));
      const int last = __builtin_amdgcn_readfirstlane(__shfl(o1, f));
      const int skipped = __builtin_amdgcn_readfirstlane(__shfl(before + incl - cnt, f));
      e = s + f;
      m0 = first + TM * (mt - skipped);
      rows = min(TM, last - m0);
      break;
    }
    before += __builtin_amdgcn_readfirstlane(__shfl(incl, 63));
  }
  if (e < 0) return;  // past the launch's last M-tile: no weight byte is read

  const size_t tiles = (size_t)e * (N >> 4) * (K >> 7);  // the expert's first tile
  const u32x4* qw_e = qw + tiles * 64;
  const uint32_t* qe_e = qe + tiles * 16;
#define MLOP_LT(LT_) \
  case LT_: moe_mx4_tile_body<LT_, EPI>(A, lda, a_rows, qw_e, qe_e, C, m0, rows, N, K, nt, smem); break
  switch ((rows + 15) >> 4) {
    MLOP_LT(1);
    MLOP_LT(2);
    MLOP_LT(3);
    MLOP_LT(4);
    MLOP_LT(5);
    MLOP_LT(6);
    MLOP_LT(7);
    MLOP_LT(8);
  }
#undef MLOP_LT
}

template <int EPI>
void run_moe_tile(const uint16_t* A, int lda, const int* a_rows, const u32x4* qw, const uint32_t* qe,
                  const int* offsets, uint16_t* C, int E, int N, int K, int mtiles, hipStream_t st) {
  constexpr int lds = kStages * kMT * 4096;
  auto kern = moe_mx4_tile_kernel<kMT, EPI>;
  static bool attr = false;
  if (!attr) {
    hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr = true;
  }
  kern<<<(N / 128) * mtiles, 256, lds, st>>>(A, lda, a_rows, qw, qe, offsets, C, E, N, K, mtiles);
}

}  // namespace

bool launch_moe_mx4_tile(const void* A, int lda, const int* a_rows, const void* qw, const void* qe,
                         const int* offsets, void* C, int R, int E, int N, int K, int epi, hipStream_t st) {
  if (E < 1 || N < 128 || N % 128 || K < 128 || K % 128 || (epi != 0 && epi != 1)) return false;
  if (R < 1) return true;
  // sum_e cdiv(rows_e, 16 MT) <= R / (16 MT) + the experts that can have rows, whatever the routing
  const long mtiles = R / (16 * kMT) + (E < R ? E : R);
  if ((N / 128) * mtiles > 0x7fffffffL) return false;
  auto* a = (const uint16_t*)A;
  auto* w = (const u32x4*)qw;
  auto* s = (const uint32_t*)qe;
  auto* c = (uint16_t*)C;
  if (epi == 0) run_moe_tile<0>(a, lda, a_rows, w, s, offsets, c, E, N, K, (int)mtiles, st);
  else run_moe_tile<1>(a, lda, a_rows, w, s, offsets, c, E, N, K, (int)mtiles, st);
  return true;
}

}  // namespace mlop
