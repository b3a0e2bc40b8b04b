// GEMM planner: see gemm_plan.h.  Host-only C++ (no HIP header, no runtime call).
#include "gemm_plan.h"

#include <algorithm>
#include <stddef.h>
#include <stdexcept>

namespace mlop {

namespace {
enum { EPI_NONE = 0, EPI_SILU_MUL = 1, EPI_ROPE = 3 };
enum { WS_NONE = 0, WS_SILU_MUL = 1, WS_ROPE = 3, WS_RES = 5 };
constexpr int kHeadD = 128;
// ring depth of the grouped (MoE) 64-row tiles on narrow N (the down projection): 6 measured
// neutral on Mixtral batch 32 / 64 (1,651 vs 1,655, 3,142 vs 3,134 tok/s, scripts/run141.sh)
constexpr int kGroupedSmallStages = 3;
}  // namespace

// ---------------------------------------------------------------------------
// knobs
static PlanEnv g_knobs;
PlanEnv& gemm_knobs() { return g_knobs; }

// gemm_split_target op: workgroups the split-K of the 16-row tiles aims at (default 512)
int gemm_split_target(int set) {
  if (set >= 1) g_knobs.split_target = set;
  return g_knobs.split_target;
}

// LDS-DMA ring depth of the M <= 128 tiles where the plan names none (3, or 5/6)
int gemm_small_stages(int set) {
  if (set >= 0) g_knobs.small_stages = set;
  return g_knobs.small_stages;
}

// Row-fitted narrow tiles for M <= 64 (plan()): 0 = the 64 x 64 tile; 32 / 64 = BN with BM the
// batch rounded up to 16 / 32 / 64; 1 (default) = BM fitted, BN and ring depth per shape (no padding rows streamed through the A ring: the 16-row
// tile's 4-stage ring is 10 KB instead of 16, so more workgroups stay resident per CU).
// The row-fitted tiles against the 64 x 64 one: M <= 32 cold projections 6-17 % faster (qkv 18.3 -> 15.3 us,
// o+norm 14.9 -> 12.9, gate_up 47.1 -> 45.6, down+norm 32.9 -> 27.3 at M = 16; BN 32 loses:
// profiles/r02_midbatch_decode.md, scripts/run131.sh).  Run-time settable for A/B.
int gemm_small_tile(int set) {
  if (set >= 0) g_knobs.small_tile = set;
  return g_knobs.small_tile;
}

static bool tile_shape_built(int bm, int bn, bool grouped) {
  for (const TileCfg& t : kGemmTiles)
    // dense 256 x 256 is the large-M variants' (gemm_dense_plan variant 1), not a variant-0 tile
    if (t.BM == bm && t.BN == bn && (grouped || !(bm == 256 && bn == 256))) return true;
  return false;
}

// grouped-plan override (scripts/bench_moe_decode.py compares MoE decode tilings in one process):
// BM, BN, ring stages, K splits; -1 = the planner's own choice.  Only tile shapes kGemmTiles
// holds are accepted.
void gemm_grouped_plan(int bm, int bn, int stages, int splits) {
  if (bm > 0 && !tile_shape_built(bm, bn, true))
    throw std::runtime_error("gemm_grouped_plan: no grouped config for this tile");
  int* gp = g_knobs.gp;
  gp[0] = bm, gp[1] = bn, gp[2] = stages, gp[3] = splits;
}

// dense-plan override (scripts/bench_mid_m.py sweeps the mid-M projection tilings in one
// process): variant (0 = gemm_kernel BM x BN, 1 = 256x256 two-stage, 3 = ping-pong, 5 =
// four-wave, 6 = four-wave half height), BM, BN, K splits (plain gemm_kernel only), LDS ring
// depth of the small tiles (0 = the default); -1 = the planner's own choice
void gemm_dense_plan(int variant, int bm, int bn, int splits, int stages) {
  if (variant >= 0 && variant != 0 && variant != 1 && variant != 3 && variant != 5 && variant != 6)
    throw std::runtime_error("gemm_dense_plan: variant must be 0, 1, 3, 5 or 6");
  if (variant == 0 && !tile_shape_built(bm, bn, false))
    throw std::runtime_error("gemm_dense_plan: no dense config for this tile");
  int* dp = g_knobs.dp;
  dp[0] = variant, dp[1] = bm, dp[2] = bn, dp[3] = splits, dp[4] = stages > 0 ? stages : 0;
}

// large-M kernel choice (plan() variants below), settable at run time (gemm_big_variant op) so
// A/B microbenches run in one process
int gemm_big_variant(int set) {
  if (set >= 0) g_knobs.big_variant = set;
  return g_knobs.big_variant;
}
// the grouped <= 32-rows-per-expert rule (plan() below) on / off (gemm_grouped_narrow op)
int gemm_grouped_narrow(int set) {
  if (set >= 0) g_knobs.grouped_narrow = set;
  return g_knobs.grouped_narrow;
}
// the planner's half-height four-wave tile (variant 6) on / off (gemm_half_tile op, A/B runs)
int gemm_half_tile(int set) {
  if (set >= 0) g_knobs.half_tile = set;
  return g_knobs.half_tile;
}

int gemm_sk_mode(int set) {
  if (set >= 0) g_knobs.sk_mode = set;
  return g_knobs.sk_mode;
}

// Small-M QKV: K split even where the plain plan keeps one K range (M <= 16: 192 tiles of 16 x
// 32): the slabs' reduce rides in the RoPE + cache kernel that runs anyway, so a second K range
// costs one fp32 slab and doubles the workgroups streaming the weights (gemm_rope_split op:
// the K ranges, 1 = the plain plan).  Interleaved, scripts/r5_ropesplitk.sh: batch 16 +1.9 %,
// batch 12 +3.0 % (4 ranges: +2.2 / +2.6 %)
int gemm_rope_split(int set) {
  if (set >= 1) g_knobs.rope_split_k = set;
  return g_knobs.rope_split_k;
}

// gemm_mid_chain op: 0 off (default), 1 on (sc1 hand-off), 2 on (acquire hand-off).  Off by
// default: the in-kernel finish adds ~3.5 us to each O / down call (two ticket round trips,
// write-through partials, the band's row totals) against the ~5 us splitk_add_rmsnorm launch it
// replaces, and the row scale costs gate_up ~0.8 us; interleaved on one box, batch 16 -1 % /
// -3 % and batch 64 -2.6 % / -3.7 % (sc1 / acquire); without the band step (a timing probe,
// numerics off) batch 16 +2-3 % and batch 64 -0.6 % (profiles/r06_mid_chain.md).
int gemm_mid_chain(int set) {
  if (set >= 0) g_knobs.mid_chain = set;
  return g_knobs.mid_chain;
}

// rows the weight-streaming kernel takes, (gemv_chain_max_m, ws_max_m]: 0 = off (default, the
// decode chain stays at the GEMV's 4 rows).  Measured slower than the planner's LDS-ring small
// tiles on gate_up / down at every M and on all shapes at M >= 32 (profiles/r06_small_m_ws.md);
// the gemm_ws_max_m op turns it on for A/B runs
int gemm_ws_max_m(int set) {
  if (set >= 0) g_knobs.ws_max_m = set > 64 ? 64 : set;
  return g_knobs.ws_max_m;
}

// Outside the chain, the plain decode projections take this kernel where it measured faster
// than the planner's small tiles (profiles/r06_small_m_ws.md): the O-size (33 MB) and QKV-size
// (50 MB) matrices at 5-8 rows.  Cold-weight microbench: o 8.4 vs 15.9 us, qkv 12.4 vs 17.8 (the
// QKV form also does RoPE + the paged K/V stores, so the rope_cache slab reduce launch goes);
// in the model the planner's O runs nearer 9 us, so end to end batch 8 gains 1.7 % and batch
// 16 is within noise (-1 %): 8 rows.  gate_up / down and 32+ rows stay on the planner.  The
// gemm_ws_small_m op (0 = off) is the A/B switch.
int gemm_ws_small_m(int set) {
  if (set >= 0) g_knobs.ws_small_m = set > 64 ? 64 : set;
  return g_knobs.ws_small_m;
}

// QKV + RoPE takes the weight-streaming kernel up to ws_rope_m rows (gemm_ws_rope_m op): it
// replaces the planner's split-K tile AND the rope_cache slab-reduce launch after it
int gemm_ws_rope_m(int set) {
  if (set >= 0) g_knobs.ws_rope_m = set > 64 ? 64 : set;
  return g_knobs.ws_rope_m;
}

// ---------------------------------------------------------------------------
// predicates

// GEMV (gemv.hip).  Rows: measured (scripts/history INDEX run38): the GEMV wins every decode
// projection at M <= 4 in the running model; at M = 8 the 64-row MFMA tiles stream gate_up /
// down faster (PlanEnv::gemv_max_m = 4).
// Shapes this path takes: 1 <= M <= gemv_max_m, 16-B aligned rows,
// whole row pairs (EPI_NONE), whole 32-row gate/up groups (EPI_SILU_MUL), or a QKV
// projection of 128-wide heads (EPI_ROPE: N = (Hq + 2 Hkv) * 128).
bool gemv_takes(const PlanEnv& e, int M, int N, int K, int epi) {
  if (M < 1 || M > e.gemv_max_m || K % 8 || N < 4) return false;
  if (epi == EPI_SILU_MUL) return N % 32 == 0;
  if (epi == EPI_ROPE) return N % kHeadD == 0;
  return epi == EPI_NONE && N % 4 == 0;
}

// MoE expert GEMMs at decode: M = routed rows in total (<= 8)
bool gemv_grouped_takes(int M, int N, int K, int epi) {
  return M >= 1 && M <= 8 && K % 8 == 0 && N % (epi == EPI_SILU_MUL ? 32 : 4) == 0 &&
         (epi == EPI_NONE || epi == EPI_SILU_MUL);
}

// rows the chain's GEMV form takes (above gemv_max_m the GEMV takes nothing anyway).
// Measured (scripts/history INDEX r4_chain8): the GEMV with the chain at 6 / 8 rows streams
// 1,419 / 1,612 tok/s against the MFMA path's 1,522 / 1,936 (its split-K reduce already
// carries the add + RMSNorm), so PlanEnv::gemv_chain_max_m = 4 stays.
bool gemv_chain_takes(const PlanEnv& e, int M, int N, int K, int epi) {
  return M <= e.gemv_chain_max_m && gemv_takes(e, M, N, K, epi);
}

bool ws_prefer(const PlanEnv& e, int M, int N, int K, int epi) {
  if (M <= e.gemv_chain_max_m || (long)N * K > 32L * 1024 * 1024 || K % 512) return false;
  if (epi == WS_ROPE) return M <= e.ws_rope_m && N % 128 == 0;
  return M <= e.ws_small_m && (epi == WS_NONE || epi == WS_RES) && N % 16 == 0;
}

// Shapes the weight-streaming kernel takes: gemv_chain_max_m < M <= ws_max_m (at most 64), K a
// multiple of 512 (four K
// quarters of whole 4-step rings), 16-B aligned rows, whole 16-row blocks (plain / residual),
// whole 32-row gate / up groups (SiLU-mul), a QKV projection of 128-wide heads (RoPE).
bool ws_takes(const PlanEnv& e, int M, int N, int K, int epi) {
  if (M <= e.gemv_chain_max_m || M > e.ws_max_m || K % 512 || N < 16) return false;
  if (epi == WS_SILU_MUL) return N % 32 == 0;
  if (epi == WS_ROPE) return N % 128 == 0;
  return (epi == WS_NONE || epi == WS_RES) && N % 16 == 0;
}

int decode_chain_max_m(const PlanEnv& e) { return e.ws_max_m > e.gemv_chain_max_m ? e.ws_max_m : e.gemv_chain_max_m; }

bool decode_chain_takes(const PlanEnv& e, int M, int N, int K, int epi) {
  return M <= e.gemv_chain_max_m ? gemv_chain_takes(e, M, N, K, epi) : ws_takes(e, M, N, K, epi);
}

// the four-wave kernel cuts its r = T % CUs tail tiles into K-halves (one extra round of
// half-length items; 2r <= CUs, nk even)
bool gemm_w4_split_ok(const PlanEnv& e, int T, int nk) {
  if (!e.sk_on()) return false;
  const int cus = e.cus;
  const int r = T % cus;
  return r > 0 && 2 * r <= cus && nk % 2 == 0 && nk / 2 >= 3;
}

// true when the four-wave kernel can run this shape (the planner's variant 5)
bool gemm_w4_ok(int M, int N, int K, int lda, int ldb, int ldc) {
  return M > 0 && K % 64 == 0 && K >= 192 && lda % 8 == 0 && ldb % 8 == 0 && N % 256 == 0 &&
         (long)M * lda * 2 < (1l << 31) && (long)N * ldb * 2 < (1l << 31) && (long)M * (ldc > 0 ? ldc : N) * 2 < (1l << 31);
}

// true when the stream-K tail is available here and splits ALL T (<= C / 2) tiles
bool sk_halves_ok(const PlanEnv& e, long T, int nk) {
  return e.sk_on() && T * 2 <= e.cus && sk_choose_d((int)T, nk, e.cus, sk_min_half()) >= 2;
}

// ---------------------------------------------------------------------------
// plan
namespace {

struct Plan {
  int BM, BN, splits, k_chunk, m_tiles, variant;
  int stages;  // LDS-DMA ring depth of the small-M tiles (0: small_stages)
  bool nosplit;  // grouped: one K range (the mid-size MoE split-K below is skipped)
};

// Tile choice by the (per-group) row count:
//   M <= 64 / 128: narrow tiles, many WGs (weight streaming);  M <= 256: the whole
//   batch in one tile (weights read once), BN by how many N tiles fill the chip;
//   large M: variant 0 = 256x128 (3-stage ring), 1 = 256x256 (2-stage, 128x64 per
//   wave: half the LDS + L2 bytes per FLOP), 2 = 256x256 + setprio around MFMAs,
//   3 = 256x256 two-group ping-pong (gemm_pp_kernel), 5 (default) = the four-wave kernel with
//   the hand-scheduled asm K-loop (gemm_w4.hip) where its grid fills the chip, else 3.  (A four-wave 128x128-per-wave
//   variant was measured 10-20% slower: profiles/r02_gemm_fourwave_rejected.md.)
Plan plan(const PlanEnv& env, int M, int N, int K, bool grouped, int n_groups, int rows_per_group) {
  Plan p{};
  p.variant = 0;
  const int mrows = grouped ? rows_per_group : M;
  // grouped (MoE): the ping-pong kernel from ~56 routed rows per expert.  Its 256 x 256 tile
  // streams each expert's weight panel once per n-tile and skips the MFMAs of empty 64-row
  // quadrants, so a half-empty expert tile costs less than the extra m-tiles (each a second walk
  // of the expert's weights) of the narrower kernels: Mixtral gate_up / down at 512 routed rows
  // 474 -> 370 / 266 -> 200 us, 1024 rows 692 -> 389 / 375 -> 208 us; 48 rows per expert equal
  // (scripts/bench_moe_decode.py, profiles/r05_moe_decode.md)
  constexpr int pp_group_min_rows = 56;
  if (grouped && mrows >= pp_group_min_rows && K % kBK == 0 && N % 256 == 0) {
    p.BM = 256; p.BN = 256; p.variant = 3;  // grouped ping-pong
  } else if (mrows <= 64 && !grouped && env.small_tile == 1) {
    // per shape (scripts/run137.sh, cold us at M = 16): wide N (gate_up) 64 columns with a
    // 6-deep ring (47.0 -> 44.8); narrow N 32 columns with an 8-deep ring at BM 16 (qkv
    // 15.3 -> 13.5, o / down unchanged): more weight bytes in flight per CU
    p.BM = mrows <= 16 ? 16 : mrows <= 32 ? 32 : 64;
    p.BN = 64;
    // (M 17-32 narrow projections on the 32-column 8-deep tiles of M <= 16: 1-2 % slower end to
    // end at batch 24 / 32, scripts/history INDEX run140)
    if (p.BM == 16) {
      const bool wide = N >= 16384;
      p.BN = wide ? 64 : 32;
      p.stages = wide ? (p.BM == 16 ? 6 : 0) : 8;
    } else if (p.BM == 64) {
      // M 33-64: narrow N on the 6-deep ring (run133: qkv 19.8 -> 18.4, down+norm 35.9 -> 32.0 us),
      // gate_up on a 4-deep one (run145: 48.2 -> 47.1 at M = 64, 6 stages lose: 50.4)
      p.stages = N < 16384 ? 6 : 4;
    }
  } else if (mrows <= 64 && !grouped && (env.small_tile == 32 || env.small_tile == 64)) {
    p.BM = mrows <= 16 ? 16 : mrows <= 32 ? 32 : 64;
    p.BN = env.small_tile;
  } else if (mrows <= 64) {
    p.BM = 64;
    p.BN = 64;
    // grouped (MoE at a few dozen rows per expert), narrow down projection: ring depth knob
    if (grouped && N < 16384) p.stages = kGroupedSmallStages;
    // grouped at <= 32 rows per expert (Mixtral batch 16-64): down on 32 x 64 tiles with a
    // 6-deep ring and ONE K range, gate_up on a 4-deep ring (scripts/bench_moe_decode.py, cold
    // expert weights, profiles/r05_moe_decode.md: down at 128 routed rows 172.4 -> 160.4 us,
    // 5.45 -> 5.86 TB/s; gate_up 318.2 -> 315.9)
    if (grouped && env.grouped_narrow && mrows <= 32) {
      if (N < 16384) { p.BM = 32; p.stages = 6; p.nosplit = true; }
      else p.stages = 4;
    }
  }
  else if (mrows <= 128) { p.BM = 128; p.BN = 64; }
  else if (mrows <= 256) {
    constexpr int bn_min_tiles = 192;
    p.BM = 256;
    p.BN = ((N + 127) / 128 >= bn_min_tiles) ? 128 : 64;
  } else {
    const int big = env.big_variant;
    constexpr int big_min_m = 1024;
    p.BM = 256;
    p.BN = 128;
    // 128: o / down at 2049-2816 rows (the mixed steps of batch ~512: 144-176 tiles, no K-half
    // tail for the four-wave kernel) ran on the 256 x 128 kernel at 0.55x hipBLASLt; the
    // ping-pong kernel's stream-K tail takes them (o at M = 2560: 122 -> 88 us, down 394 -> 269;
    // scripts/history/r4_m2560.sh)
    constexpr int pp_min_tiles = 128;
    const long t256 = (long)((M + 255) / 256) * ((N + 255) / 256);
    // below pp_min_tiles the 256x256 grid leaves CUs idle, unless the stream-K tail can cut
    // every tile in two (T <= C / 2): o / down at M = 2040 (128 tiles)
    const bool pp_ok = K % kBK == 0 && (t256 >= pp_min_tiles || sk_halves_ok(env, t256, K / kBK));
    // variant 5: the four-wave kernel where its grid fills the chip: >= w4_min_tiles tiles, or
    // a tail it can cut in K-halves (o / down at M = 2048: 128 tiles -> 256 half-tiles); else
    // the ping-pong kernel with its general stream-K tail
    constexpr int w4_min_tiles = 192;
    const bool w4_fills = t256 >= w4_min_tiles || gemm_w4_split_ok(env, (int)t256, K / kBK);
    // Wide projections take the large-M kernels from 512 rows: gate_up / lm_head at M = 512 /
    // 768 ran 127 -> 87 / 191 -> 153 us (8B) and 511 -> 404 us (70B gate_up), batch-512 serving
    // +5.3 %; narrow ones lose there (o / down at M = 512: 31 -> 48 / 66 -> 124 us) and keep the
    // 256 x 128 kernel (scripts/history/r4_bigminm.sh, r4_bigminm2.sh, r4_widemin.sh).
    // Below ~72 tiles of 256 x 256 (o / down at M = 512 - 1024: 32 - 64 tiles) the 256 x 128
    // kernel beats them at every M measured short of 2048 (o at M = 1024: 44.7 vs 48.6 us, down
    // 114.7 vs 129.5); from 72 tiles (qkv at M = 768, 70B qkv at 512) the large-M kernels win.
    constexpr int wide_min_m = 512;
    constexpr int mid_tiles = 72;
    const int big_from = t256 >= mid_tiles ? std::min(big_min_m, wide_min_m) : std::max(big_min_m, 2048);
    if (big == 5 && !(mrows >= big_from && !grouped && w4_fills && gemm_w4_ok(M, N, K, K, K, 0))) {
      if (mrows >= big_from && !grouped && pp_ok) { p.BN = 256; p.variant = 3; }
    } else if (big && mrows >= big_from && !grouped && (big < 3 || pp_ok)) {
      p.BN = 256;
      p.variant = big;
    }
    if (!grouped && big == 5) {
      // long-K narrow projections (down, K = 14336) at 40-71 tiles of 256 x 256 (M 640-1279):
      // the ping-pong kernel's stream-K tail spreads the few tiles' K over every CU (down at
      // M = 768: 105 -> 90 us, 1024: 118 -> 108; hipBLASLt 90 / 111)
      if (p.variant == 0 && K >= 8192 && t256 >= 40 && t256 < mid_tiles && K % kBK == 0 &&
          sk_halves_ok(env, t256, K / kBK)) {
        p.BN = 256;
        p.variant = 3;
      }
      // four-wave vs ping-pong past one full round: the four-wave kernel runs whole rounds of
      // 256 x 256 tiles (a tail of r <= CUs / 2 tiles in K-halves), the ping-pong kernel ~7 %
      // slower per tile but with a stream-K tail that balances ANY remainder.  Estimated time in
      // four-wave tile rounds: w4 = q + (r ? (2r <= C ? 0.55 : 1) : 0), pp = 1.08 T / C + 0.05.
      // (M = 4608: o 147 -> 134 us, down 476 -> 403, qkv 181 -> 172; the headline's M ~ 4088 is
      // whole rounds for every projection and stays on the four-wave kernel; bench_mid_m.py)
      const bool sk = env.sk_on();
      if (p.variant == 5 && sk && t256 > env.cus && pp_ok) {
        const long C = env.cus, q = t256 / C, r = t256 % C;
        const float w4_est = (float)q + (r == 0 ? 0.f : (2 * r <= C ? 0.55f : 1.f));
        const float pp_est = 1.08f * (float)t256 / (float)C + 0.05f;
        if (pp_est < w4_est - 0.03f) p.variant = 3;
      }
      // variant 6, the half-height (128 x 256) four-wave tile, where its grid is at most one
      // round: up to twice the workgroups of the 256 x 256 grid (a lone tile of either height
      // runs ~1.8x faster than one in a full round, so idle CUs cost more than the half tile's
      // lower MFMA density).  bench_mid_m.py (profiles/r05_gemm_w4h.md), planner before -> after:
      // o at M = 1024 / 1536 / 2048 46.2 -> 38.3 / 56.0 -> 47.6 / 65.6 -> 55.2 us, qkv at 384 /
      // 512 / 1024 43.1 -> 33.1 / 44.4 -> 35.3 / 56.0 -> 47.5; past one round it loses to the
      // full tile (qkv 1408: 75.9 vs 72.3).  Long K (down): only with its own K-half tail
      // (t128 <= CUs / 2: 96 -> 256 items, M = 1024 110.8 -> 98.5); without it the full tile's
      // K-halves win (M = 1152: 153.7 vs 131.1), and below ~80 tiles the 256 x 128 split-K kernel
      // (M = 512: 83.1 vs 67.6).
      const long t128 = (long)((M + 127) / 128) * ((N + 255) / 256);
      const bool long_k = K >= 8192;
      if (env.half_tile && sk && mrows >= 384 && (long_k ? t128 >= 80 && 2 * t128 <= env.cus : t128 >= 64 && t128 <= env.cus) &&
          (p.variant == 0 || p.variant == 3 || p.variant == 5) && gemm_w4_ok(M, N, K, K, K, 0)) {
        p.BM = 128;
        p.BN = 256;
        p.variant = 6;
      }
    }
  }
  if (!grouped && env.dp[0] >= 0) {  // bench override (gemm_dense_plan)
    p.variant = env.dp[0];
    p.BM = p.variant == 0 ? env.dp[1] : p.variant == 6 ? 128 : 256;
    p.BN = p.variant == 0 ? env.dp[2] : 256;
    p.stages = env.dp[4];
  }
  if (grouped && env.gp[0] > 0) {  // bench override (gemm_grouped_plan)
    p.BM = env.gp[0];
    p.BN = env.gp[1];
    p.variant = (p.BM == 256 && p.BN == 256) ? 3 : 0;
    p.stages = env.gp[2] > 0 ? env.gp[2] : 0;
  }
  const int n_tiles = (N + p.BN - 1) / p.BN;
  const int real_m_tiles = (M + p.BM - 1) / p.BM;
  p.m_tiles = grouped ? real_m_tiles + n_groups : real_m_tiles;
  p.splits = 1;
  p.k_chunk = K;
  const long tiles = (long)n_tiles * real_m_tiles;
  // run49: down -5..-15% at M 8-64.  The 16-row tiles (M 9-16) aim at 512 workgroups: batch 16
  // +5.6 / +6.0 % interleaved (scripts/r5_splittarget.sh, r5_splittarget2.sh), while 512 lost
  // 1.4-1.6 % at batch 24 / 32 (32-row tiles), 5 % at batch 64 and 4 % at 256
  const int split_target = p.BM <= 16 ? env.split_target : 256;
  constexpr int split_max_tiles = 160;
  if (!grouped && tiles < split_max_tiles && K >= 1024 && p.variant != 3 && p.variant < 5) {
    int s = (int)std::min<long>(8, std::max<long>(1, split_target / tiles));
    int kc = ((K / s + kBK - 1) / kBK) * kBK;
    p.splits = (K + kc - 1) / kc;
    p.k_chunk = kc;
  }
  if (!grouped && env.dp[0] == 0 && env.dp[3] >= 1) {
    const int kc = ((K / env.dp[3] + kBK - 1) / kBK) * kBK;
    p.splits = (K + kc - 1) / kc;
    p.k_chunk = kc;
  }
  return p;
}

// EPI_ROPE: the plain (no split-K) plan must stage whole heads: BN >= 128, i.e. M > 256.
// Small M whose plan splits K: the slabs go to the stream-K scratch and the split-K reduce is
// fused into the RoPE + cache kernel (one launch instead of reduce + rope_cache).
bool rope_slabs_ok(const PlanEnv& env, const Plan& p, int M, int N) {
  return p.splits > 1 && p.variant != 3 && p.variant < 5 && env.sk_on() &&
         (size_t)p.splits * M * N <= (size_t)kSkScratchFloats;
}

bool rope_whole_heads(const Plan& p) { return (p.BM == 256 || p.variant == 6) && p.BN >= 128; }

// the QKV + RoPE plan: the plain plan p, K split for small M (gemm_rope_split above)
Plan rope_split(const PlanEnv& env, Plan p, int K) {
  if (env.rope_split_k > 1 && p.splits == 1 && p.variant == 0 && p.BM <= 64 && K >= 2048) {
    const int kc = ((K / env.rope_split_k + kBK - 1) / kBK) * kBK;
    p.splits = (K + kc - 1) / kc;
    p.k_chunk = kc;
  }
  return p;
}
Plan rope_plan(const PlanEnv& env, int M, int N, int K) { return rope_split(env, plan(env, M, N, K, false, 0, 0), K); }

// The large-M decoder's norm chain: O / down add into the residual and leave per-row sums of
// squares (W4_ADD_SS), gate_up / QKV scale their rows by the RMSNorm factor (W4_RS), so the
// add + RMSNorm passes over [M, H] disappear (norm weights folded into the consumer weights).
// Everything the four-wave chain launch needs, so the caller decides the chain ONCE per forward
// (before the first in-place residual update) and never meets a refusal mid-layer: the shape on
// the four-wave kernel, the stream-K scratch that holds the band tickets reserved, and one
// ticket per band of BM rows.
bool w4_chain_plan_ok(const PlanEnv& env, const Plan& p, int M, int N, int K) {
  if (M <= 0 || gemv_takes(env, M, N, K, EPI_NONE) || gemv_takes(env, M, N, K, EPI_ROPE)) return false;
  if (!env.sk_on()) return false;
  return (p.variant == 5 || p.variant == 6) && p.splits == 1 && p.BN == 256 && (M + p.BM - 1) / p.BM <= kSkMaxWg &&
         gemm_w4_ok(M, N, K, K, K, N);
}

// Mid-M norm chain (rows in (decode_chain_max_m, 64], TP = 1): the decoder layer's two add +
// RMSNorm launches (splitk_add_rmsnorm) fold into the planner's small-tile GEMMs.  O / down
// (epi 0) split K and the tile's last split adds into the residual and leaves the row sums of
// squares (mid_chain_finish); gate_up (epi 1, one K range) scales its accumulator rows by the
// RMSNorm factor in its SiLU epilogue; QKV + RoPE (epi 3) takes the factor in the split-K slab
// reduce of the RoPE + cache kernel, or in the weight-streaming kernel's row-scale prologue at
// 5-8 rows (which computes it from the rows it streams).  (gemm_mid_chain above: off by default.)
bool mid_chain_rows(const PlanEnv& env, int M, int N, int K) {
  return env.mid_chain && M > decode_chain_max_m(env) && M <= 64 && K % kBK == 0 && N % 128 == 0 && env.sk_on();
}
// p: rope_plan for epi 3 (unused where the weight-streaming kernel is preferred), else plan
bool mid_chain_plan_ok(const PlanEnv& env, const Plan& p, int M, int N, int K, int epi) {
  if (!mid_chain_rows(env, M, N, K)) return false;
  if (epi == EPI_ROPE) {
    if (ws_prefer(env, M, N, K, EPI_ROPE)) return K % 512 == 0;
    return !rope_whole_heads(p) && rope_slabs_ok(env, p, M, N);
  }
  if (p.variant != 0 || p.BM > 64 || N % p.BN) return false;
  if (epi == EPI_SILU_MUL) return p.splits == 1;
  if (epi != EPI_NONE || p.splits < 2) return false;
  const long gx = N / p.BN, gy = (M + p.BM - 1) / p.BM;
  return gx * gy + gy <= kSkMaxWg &&
         (size_t)p.splits * M * N + (size_t)M * gx <= (size_t)kSkScratchFloats;
}

// ---------------------------------------------------------------------------
// route

Route refused() { return Route{}; }

Route simple(int family, int finish = FIN_NONE) {
  Route r;
  r.family = family;
  r.finish = finish;
  return r;
}

Route tile_route(int bm, int bn, int stages, bool setprio, const Plan& p) {
  Route r;
  for (int i = 0; i < kNumGemmTiles; ++i) {
    const TileCfg& t = kGemmTiles[i];
    if (t.BM == bm && t.BN == bn && t.stages == stages && t.setprio == setprio) {
      r.family = FAM_TILE;
      r.tile = i;
      r.BM = t.BM, r.BN = t.BN, r.WM = t.WM, r.WN = t.WN, r.stages = t.stages, r.setprio = t.setprio;
      r.splits = p.splits, r.k_chunk = p.k_chunk, r.m_tiles = p.m_tiles;
      return r;
    }
  }
  throw std::runtime_error("gemm planner: tile configuration not in kGemmTiles");
}

// the ping-pong kernel's stream-K tail of a plain launch of T tiles
Route pp_route(const PlanEnv& env, int M, int N, int K, bool grouped) {
  Route r = simple(FAM_PP);
  r.BM = 256, r.BN = 256;
  if (grouped || !env.sk_on()) return r;  // grouped: planned on device from offsets[]
  const int T = ((N + 255) / 256) * ((M + 255) / 256);
  r.sk_d = sk_choose_d(T, K / kBK, env.cus, sk_min_half());
  r.sk_wgs = (T % env.cus) * r.sk_d;
  return r;
}

Route w4_route(int bm) {
  Route r = simple(bm == 128 ? FAM_W4H : FAM_W4);
  r.BM = bm, r.BN = 256;
  return r;
}

// The kernel a plan runs on.  Weight-streaming tiles (M <= 128): a deeper LDS-DMA ring keeps
// more weight bytes in flight per CU (3 stages x 16 KB per workgroup streamed gate_up at
// 4.7 TB/s at M = 64); each tile shape is built at a few ring depths and takes the deepest one
// the plan's depth (or small_stages) reaches.  rope: the RoPE epilogue (whole heads per staged
// chunk, one K range).  w4: the leading dimensions suit the four-wave kernel.
Route resolve(const PlanEnv& env, const Plan& p, int M, int N, int K, bool grouped, bool rope, bool w4) {
  if (rope) {
    if (p.BN == 128) return tile_route(256, 128, 3, false, p);
    if (p.variant >= 5 && w4) return w4_route(p.BM);
    if (p.variant == 3 || p.variant >= 5) return pp_route(env, M, N, K, false);
    return tile_route(256, 256, 2, p.variant == 2, p);
  }
  const int sst = p.stages ? p.stages : env.small_stages;
  if (!grouped && p.variant == 6) return p.splits == 1 && w4 ? w4_route(128) : pp_route(env, M, N, K, false);
  if (p.BM == 16 && (p.BN == 32 || p.BN == 64)) return tile_route(16, p.BN, sst >= 8 ? 8 : sst >= 6 ? 6 : 4, false, p);
  if (p.BM == 32 && p.BN == 32) return tile_route(32, 32, sst >= 8 ? 8 : 4, false, p);
  if (p.BM == 32 && p.BN == 64) return tile_route(32, 64, sst >= 6 ? 6 : 4, false, p);
  if (p.BM == 64 && p.BN == 32) return tile_route(64, 32, 4, false, p);
  if (p.BM == 64) return tile_route(64, 64, p.BN == 64 && sst >= 6 ? 6 : p.BN == 64 && sst == 4 ? 4 : 3, false, p);
  if (p.BM == 128) return tile_route(128, 64, env.small_stages >= 5 ? 5 : 3, false, p);
  if (p.BN == 64) return tile_route(256, 64, 3, false, p);
  if (p.BN == 128) return tile_route(256, 128, 3, false, p);
  if (grouped) {
    if (p.variant == 3) return pp_route(env, M, N, K, true);
    throw std::runtime_error("gemm planner: grouped 256 x 256 plan off the ping-pong kernel");
  }
  if (p.variant == 5 && p.splits == 1 && w4) return w4_route(256);
  if ((p.variant == 3 || p.variant == 5) && p.splits == 1) return pp_route(env, M, N, K, false);
  return tile_route(256, 256, 2, p.variant == 2, p);
}

Route with_slabs(Route r, int finish, int src, int M, int N) {
  r.finish = finish;
  r.ws_src = src;
  r.ws_floats = (long)r.splits * M * N;
  return r;
}

// out = epi(A . B^T), epi none / SiLU-mul
Route route_plain(const PlanEnv& env, const GemmCall& c, int lda, int ldb, int ldc) {
  const int M = c.M, N = c.N, K = c.K, epi = c.op;
  if (gemv_takes(env, M, N, K, epi) && lda % 8 == 0 && ldb % 8 == 0) return simple(FAM_GEMV);
  Plan p = plan(env, M, N, K, false, 0, 0);
  if (p.splits > 1 && c.ws_avail >= 0 && (long)p.splits * M * N > c.ws_avail) { p.splits = 1; p.k_chunk = K; }
  const Route r = resolve(env, p, M, N, K, false, false, gemm_w4_ok(M, N, K, lda, ldb, ldc));
  return r.family == FAM_TILE && r.splits > 1 ? with_slabs(r, FIN_REDUCE, WS_SRC_CALLER, M, N) : r;
}

// QKV projection + RoPE + paged-cache stores
Route route_rope(const PlanEnv& env, const GemmCall& c, int lda) {
  const int M = c.M, N = c.N, K = c.K;
  if (N % 128 || K % kBK) return refused();
  const bool gemv = gemv_takes(env, M, N, K, EPI_ROPE);  // decode M <= 4: gemv.hip
  if (gemv && lda % 8 == 0) return simple(FAM_GEMV);
  Plan p = rope_plan(env, M, N, K);
  const bool whole = rope_whole_heads(p), slabs = rope_slabs_ok(env, p, M, N);
  if (!gemv && !whole && !slabs) return refused();
  if (ws_prefer(env, M, N, K, EPI_ROPE) && lda % 8 == 0) return simple(FAM_WS);  // 5-8 rows: the weight-streaming MFMA kernel
  if (!whole) {  // small M: split-K slabs + fused reduce / RoPE / cache
    if (!slabs) return refused();
    return with_slabs(resolve(env, p, M, N, K, false, false, false), FIN_ROPE_SLABS, WS_SRC_SCRATCH, M, N);
  }
  p.splits = 1;
  p.k_chunk = K;
  return resolve(env, p, M, N, K, false, true, gemm_w4_ok(M, N, K, lda, K, 0));
}

// y = A.B^T; residual += y; out = rmsnorm(residual) * w.  Refused when the shape does not take
// the split-K path: the caller then runs gemm + add_rmsnorm.
Route route_add_rmsnorm(const PlanEnv& env, const GemmCall& c, int lda) {
  const int M = c.M, N = c.N, K = c.K;
  if (gemv_takes(env, M, N, K, EPI_NONE)) return refused();  // decode sizes: GEMV + add_rmsnorm (or the norm chain)
  // 5-8 rows of an O-size projection: the weight-streaming MFMA kernel adds into the residual
  // in place (bf16(res + bf16(y)), norm.hip's rounding), then one RMSNorm pass
  if (ws_prefer(env, M, N, K, EPI_NONE) && lda % 8 == 0) return simple(FAM_WS, FIN_RMSNORM);
  const Plan p = plan(env, M, N, K, false, 0, 0);
  if (p.splits <= 1 || p.splits > kMaxSplits || (c.ws_avail >= 0 && (long)p.splits * M * N > c.ws_avail) || N % 8)
    return refused();
  return with_slabs(resolve(env, p, M, N, K, false, false, false), FIN_ADD_RMSNORM, WS_SRC_CALLER, M, N);
}

Route route_grouped(const PlanEnv& env, const GemmCall& c) {
  const int M = c.M, N = c.N, K = c.K, epi = c.op & 3, n_groups = c.n_groups;
  const int* gp = env.gp;  // gemm_grouped_plan override: BM, BN, stages, splits
  if (!c.indirect && gemv_grouped_takes(M, N, K, epi)) return simple(FAM_GEMV);  // MoE decode: stream only the routed experts' weights
  Plan p = plan(env, M, N, K, true, n_groups, c.rows_per_group);
  // Mid-size MoE batches (a few dozen rows per expert): one m-tile per expert x N/64 tiles
  // is too few workgroups to stream every expert's weights at full rate (down at batch 64:
  // 512 workgroups of K = 14336, 4.7 TB/s).  Split K like the dense path, partials in the
  // stream-K slab buffer (same stream, so never in use by another launch), then the reduce
  // kernel applies the epilogue.  Routed tiles are estimated as one m-tile per expert.
  if (p.variant != 3 && K >= 2048 && gp[3] != 1 && !(p.nosplit && gp[0] <= 0)) {
    const long t_est = (long)((N + p.BN - 1) / p.BN) * std::max(1, std::min(n_groups, (M + p.BM - 1) / p.BM + n_groups));
    constexpr int target = 1024;
    int s = (int)std::min<long>(8, std::max<long>(1, target / std::max<long>(1, t_est)));
    if (gp[3] > 1) s = gp[3];
    while (s > 1 && (K / s) % kBK) --s;
    if (env.sk_on() && s > 1 && (size_t)s * M * N * 4 <= (size_t)kSkScratchFloats * 4) {
      p.splits = s;
      p.k_chunk = K / s;
    }
  }
  const Route r = resolve(env, p, M, N, K, true, false, false);
  return r.family == FAM_TILE && r.splits > 1 ? with_slabs(r, FIN_REDUCE, WS_SRC_SCRATCH, M, N) : r;
}

// The norm chain's GEMMs: O / down (OP_CHAIN_RES_SS, residual += and the row sums of squares),
// gate_up / QKV (OP_CHAIN_RS*, rows scaled by the RMSNorm factor).  By rows: the decode chain
// on the GEMV or the weight-streaming kernel, then the mid chain on the planner's small tiles
// (self-finishing split-K, no finishing launch), then the four-wave chain.
Route route_chain(const PlanEnv& env, const GemmCall& c, int lda, int ldc) {
  const int M = c.M, N = c.N, K = c.K;
  const int epi = c.op == OP_CHAIN_RES_SS ? EPI_NONE : c.op & 3;
  if (M <= decode_chain_max_m(env)) {
    // EPI_RES / PRO_RS: the consumers take their row factors from the residual itself
    if ((c.op == OP_CHAIN_RES_SS && ldc != N) || !decode_chain_takes(env, M, N, K, epi)) return refused();
    return simple(M <= env.gemv_chain_max_m ? FAM_GEMV : FAM_WS);
  }
  const Plan base = plan(env, M, N, K, false, 0, 0);
  const Plan p = epi == EPI_ROPE ? rope_split(env, base, K) : base;
  if (mid_chain_plan_ok(env, p, M, N, K, epi)) {
    if (epi == EPI_ROPE) {
      // 5-8 rows: the weight-streaming kernel computes the row scale from the rows it streams;
      // else the slab path, row scale in the RoPE + cache reduce
      return ws_prefer(env, M, N, K, EPI_ROPE) ? simple(FAM_WS) : route_rope(env, c, lda);
    }
    if (c.op == OP_CHAIN_RS) return refused();  // the mid form's consumer is the SiLU tile only
    Route r = resolve(env, p, M, N, K, false, false, false);
    if (epi == EPI_NONE) { r.ws_src = WS_SRC_SCRATCH; r.ws_floats = (long)r.splits * M * N; }
    return r;
  }
  if (!w4_chain_plan_ok(env, base, M, N, K) || !gemm_w4_ok(M, N, K, lda, K, ldc)) return refused();
  return w4_route(base.BM);
}

}  // namespace

Route gemm_route(const PlanEnv& env, const GemmCall& c) {
  if (c.M <= 0) return refused();
  const bool silu = c.op == OP_SILU_MUL || c.op == OP_GROUPED_SILU || c.op == OP_CHAIN_RS_SILU;
  const int lda = c.lda ? c.lda : c.K, ldb = c.ldb ? c.ldb : c.K;
  const int ldc = c.ldc ? c.ldc : c.op == OP_ROPE || c.op == OP_CHAIN_RS_ROPE ? 0 : silu ? c.N / 2 : c.N;
  switch (c.op) {
    case OP_PLAIN:
    case OP_SILU_MUL: return route_plain(env, c, lda, ldb, ldc);
    case OP_ADD_RMSNORM: return route_add_rmsnorm(env, c, lda);
    case OP_ROPE: return route_rope(env, c, lda);
    case OP_CHAIN_RES_SS:
    case OP_CHAIN_RS:
    case OP_CHAIN_RS_SILU:
    case OP_CHAIN_RS_ROPE: return route_chain(env, c, lda, ldc);
    case OP_GROUPED:
    case OP_GROUPED_SILU: return route_grouped(env, c);
    default: throw std::runtime_error("gemm_route: unknown op");
  }
}

void gemm_route_fields(const Route& r, long out[kRouteFields]) {
  const long f[kRouteFields] = {r.family, r.tile,   r.BM,      r.BN,    r.WM,   r.WN,     r.stages, r.setprio,
                                r.splits, r.k_chunk, r.m_tiles, r.sk_d, r.sk_wgs, r.finish, r.ws_src, r.ws_floats};
  std::copy(f, f + kRouteFields, out);
}

// ---------------------------------------------------------------------------
// views of the route

static GemmCall call(int op, int M, int N, int K) {
  GemmCall c;
  c.op = op, c.M = M, c.N = N, c.K = K;
  return c;
}

bool gemm_rope_supported(const PlanEnv& e, int M, int N, int K) { return gemm_route(e, call(OP_ROPE, M, N, K)).ok(); }

// every GEMM of this shape runs on the four-wave chain (epilogue flags 4, 0|8, 1|8, 3|8)
bool w4_chain_ok(const PlanEnv& e, int M, int N, int K) {
  return M > 0 && w4_chain_plan_ok(e, plan(e, M, N, K, false, 0, 0), M, N, K);
}

bool mid_chain_ok(const PlanEnv& e, int M, int N, int K, int epi) {
  if (!mid_chain_rows(e, M, N, K)) return false;
  return mid_chain_plan_ok(e, epi == EPI_ROPE ? rope_plan(e, M, N, K) : plan(e, M, N, K, false, 0, 0), M, N, K, epi);
}

bool chain_ok(const PlanEnv& e, int M, int N, int K, int epi) {
  if (M <= decode_chain_max_m(e)) return decode_chain_takes(e, M, N, K, epi < 0 ? EPI_NONE : epi);
  if (M <= 64 && epi >= 0) return mid_chain_ok(e, M, N, K, epi);
  return w4_chain_ok(e, M, N, K);
}

long gemm_workspace_floats(const PlanEnv& e, int M, int N, int K, int epi) {
  const Route r = gemm_route(e, call(epi == EPI_SILU_MUL ? OP_SILU_MUL : OP_PLAIN, M, N, K));
  return r.ws_src == WS_SRC_CALLER ? r.ws_floats : 0;
}

// stream-K workgroups a plain launch of this shape would add (0: data-parallel grid only)
int gemm_sk_workgroups(const PlanEnv& e, int M, int N, int K) {
  const Route r = gemm_route(e, call(OP_PLAIN, M, N, K));
  return r.family == FAM_PP ? r.sk_wgs : 0;
}

}  // namespace mlop
