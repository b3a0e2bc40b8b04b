// The GEMM planner (gemm_plan.cc): which kernel, which tile, how many K ranges and which
// finishing launch a projection of a given shape gets.  Plain C++ on shapes and knobs: no HIP
// header, no runtime call, so tests/test_gemm_plan_cpu.py enumerates it without a GPU.  gemm.hip
// fills the two device facts of the environment at the call site, asks for ONE route per launch
// and executes it; the query ops (gemm_workspace, gemm_rope_supported, w4_chain_ok, ...) are
// views of the same route.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define MLOP_HD __host__ __device__
#else
#define MLOP_HD
#endif

namespace mlop {

constexpr int kBK = 64;
constexpr int kMaxSplits = 8;  // plan(): split-K factors are at most 8
// stream-K scratch (gemm.hip gemm_sk_reserve): 2 fp32 256 x 256 slots per stream-K workgroup
constexpr int kSkMaxWg = 256;
constexpr long kSkScratchFloats = 2l * kSkMaxWg * 256 * 256;
constexpr int kSkMinIters = 16;
constexpr int sk_min_half() { return kSkMinIters / 2 > 1 ? kSkMinIters / 2 : 1; }

// d for the r = T % cus tail tiles of a T-tile launch: each is cut into d equal K-ranges
// (d | nk, so no range straddles two tiles), one per extra workgroup, d <= cus / r, when the
// cost model (in K-tile times, calibrated on scripts/bench_proj.py) beats the tail round's nk:
//   nk / d                   the range itself
//   max(2, 0.04 * r * d)     256 KB fp32 partial per workgroup, HBM-bound when all write
//   2 * (d - 1, or d)        the last contributor's slot reads (one CU, ~3 us per slot)
//   1                        a second pipeline fill + ticket
// 0: keep the data-parallel grid.  Host (plain launches) and device (grouped launches, whose
// tile count depends on the routing) evaluate the same function.
MLOP_HD inline int sk_choose_d(int T, int nk, int cus, int min_half) {
  const int r = T % cus;
  if (r == 0) return 0;
  float best = 0.9f * nk;  // require a 10 % gain on the tail round
  int best_d = 0;
  const int dmax = cus / r < 32 ? cus / r : 32;
  for (int d = 2; d <= dmax; ++d) {
    if (nk % d || nk / d < min_half) continue;
    const float w = 0.04f * r * d;
    const float cost = nk / d + (w > 2.f ? w : 2.f) + 2.f * (d >= 3 ? d : d - 1) + 1.f;
    if (cost < best) {
      best = cost;
      best_d = d;
    }
  }
  return best_d;
}

// Everything a routing decision depends on besides the shape: two device facts and the knobs
// (each settable at run time through the op of the same name, for in-process A/B runs).
struct PlanEnv {
  int cus = 0;      // CUs of the device (as the stream-K scratch was planned for)
  bool sk = false;  // the stream-K scratch is reserved on the device (gemm_sk_reserve)
  int small_tile = 1;      // gemm_small_tile: M <= 64 tiles, 1 = fitted per shape, 0 = 64 x 64, 32 / 64 = BN
  int small_stages = 3;    // gemm_small_stages: LDS-DMA ring depth of the M <= 128 tiles (3, or 5 / 6)
  int big_variant = 5;     // gemm_big_variant: large M, 0 256x128, 1 / 2 256x256, 3 ping-pong, 5 four-wave
  int half_tile = 1;       // gemm_half_tile: the four-wave half-height (128 x 256) tile on / off
  int grouped_narrow = 1;  // gemm_grouped_narrow: the grouped <= 32-rows-per-expert rule on / off
  int split_target = 512;  // gemm_split_target: workgroups the split-K of the 16-row tiles aims at
  int rope_split_k = 2;    // gemm_rope_split: K ranges of the small-M QKV + RoPE launch
  int sk_mode = 1;         // gemm_sk_mode: the stream-K scratch in use (1) or ignored (0)
  int mid_chain = 0;       // gemm_mid_chain: the 5-64-row norm chain, 0 off, 1 / 2 on (sc1 / acquire)
  int gp[4] = {-1, -1, -1, -1};     // gemm_grouped_plan: BM, BN, stages, splits (-1: the planner's)
  int dp[5] = {-1, -1, -1, -1, 0};  // gemm_dense_plan: variant, BM, BN, splits, stages
  // gemm_ws_small_m / gemm_ws_rope_m / gemm_ws_max_m: rows up to which the weight-streaming kernel
  // takes the plain O-size projections, QKV + RoPE, and the decode norm chain
  int ws_small_m = 8, ws_rope_m = 8, ws_max_m = 0;
  int gemv_max_m = 4, gemv_chain_max_m = 4;  // rows of the GEMV (gemv.hip) and of its chain form
  bool sk_on() const { return sk_mode && sk && cus > 0; }
};
// the live knobs (cus / sk unset); gemm_live_env() (gemm.hip) = the knobs + the current device's facts
PlanEnv& gemm_knobs();
PlanEnv gemm_live_env();
// the knob ops: set >= 0 (>= 1: split_target, rope_split) changes the value, returns the current one
int gemm_small_tile(int set);
int gemm_small_stages(int set);
int gemm_big_variant(int set);
int gemm_half_tile(int set);
int gemm_grouped_narrow(int set);
int gemm_split_target(int set);
int gemm_rope_split(int set);
int gemm_sk_mode(int set);
int gemm_mid_chain(int set);
int gemm_ws_small_m(int set);
int gemm_ws_rope_m(int set);
int gemm_ws_max_m(int set);

// What a launch computes: the epilogue number of the Python side (ops/__init__.py EPI_*), the
// norm-chain flags 4 (residual += , row sums of squares) and 8 (rows scaled), 16 = grouped.
enum GemmOp {
  OP_PLAIN = 0,
  OP_SILU_MUL = 1,
  OP_ADD_RMSNORM = 2,
  OP_ROPE = 3,
  OP_CHAIN_RES_SS = 4,
  OP_CHAIN_RS = 8,
  OP_CHAIN_RS_SILU = 9,
  OP_CHAIN_RS_ROPE = 11,
  OP_GROUPED = 16,
  OP_GROUPED_SILU = 17,
};

struct GemmCall {
  int op = OP_PLAIN;
  int M = 0, N = 0, K = 0;
  int lda = 0, ldb = 0, ldc = 0;  // 0: dense (K, K, the output width)
  int n_groups = 0, rows_per_group = 0;
  long ws_avail = -1;     // floats of the caller's workspace (-1: whatever the route asks for)
  bool indirect = false;  // grouped: A rows through a_rows, or the slabs handed to the caller
};

enum GemmFamily { FAM_REFUSED = 0, FAM_GEMV, FAM_WS, FAM_TILE, FAM_PP, FAM_W4, FAM_W4H };
enum GemmFinish { FIN_NONE = 0, FIN_REDUCE, FIN_ADD_RMSNORM, FIN_ROPE_SLABS, FIN_RMSNORM };
enum GemmWsSrc { WS_SRC_NONE = 0, WS_SRC_CALLER, WS_SRC_SCRATCH };

// gemm_kernel<BM, BN, WM, WN, EPI, GROUPED, STAGES, SETPRIO> instantiations, in X(bm, bn, wm,
// wn, stages, setprio, rope): the single list behind the launch lookup (gemm.hip launch_tile),
// the legality checks of gemm_dense_plan / gemm_grouped_plan and the planner's ring-depth
// resolution.  rope = also built with the RoPE epilogue (whole 128-wide heads per staged chunk).
#define MLOP_GEMM_TILES(X)       \
  X(16, 32, 1, 2, 8, false, 0)   \
  X(16, 32, 1, 2, 6, false, 0)   \
  X(16, 32, 1, 2, 4, false, 0)   \
  X(16, 64, 1, 2, 8, false, 0)   \
  X(16, 64, 1, 2, 6, false, 0)   \
  X(16, 64, 1, 2, 4, false, 0)   \
  X(32, 32, 1, 2, 8, false, 0)   \
  X(32, 32, 1, 2, 4, false, 0)   \
  X(32, 64, 1, 4, 6, false, 0)   \
  X(32, 64, 1, 4, 4, false, 0)   \
  X(64, 32, 1, 2, 4, false, 0)   \
  X(64, 64, 1, 4, 6, false, 0)   \
  X(64, 64, 1, 4, 4, false, 0)   \
  X(64, 64, 1, 4, 3, false, 0)   \
  X(128, 64, 2, 2, 5, false, 0)  \
  X(128, 64, 2, 2, 3, false, 0)  \
  X(256, 64, 4, 2, 3, false, 0)  \
  X(256, 128, 4, 2, 3, false, 1) \
  X(256, 256, 2, 4, 2, true, 1)  \
  X(256, 256, 2, 4, 2, false, 1)

struct TileCfg {
  int BM, BN, WM, WN, stages;
  bool setprio, rope;
};
#define MLOP_TILE_ENTRY(bm, bn, wm, wn, st, prio, rope) {bm, bn, wm, wn, st, prio, rope != 0},
constexpr TileCfg kGemmTiles[] = {MLOP_GEMM_TILES(MLOP_TILE_ENTRY)};
#undef MLOP_TILE_ENTRY
constexpr int kNumGemmTiles = sizeof(kGemmTiles) / sizeof(kGemmTiles[0]);

// Exactly what one call launches.  gemm_route_fields() is the flat form (this order) the
// gemm_route / gemm_route_env ops and tests/native/gemm_plan_dump.cc print.
struct Route {
  int family = FAM_REFUSED;
  int tile = -1;  // index into kGemmTiles (FAM_TILE), else -1
  int BM = 0, BN = 0, WM = 0, WN = 0, stages = 0, setprio = 0;
  int splits = 1, k_chunk = 0;  // K ranges of the tile family and the K of each
  int m_tiles = 0;              // tile family: m-tiles of the grid (grouped: + one per group)
  int sk_d = 0, sk_wgs = 0;     // ping-pong stream-K tail: K ranges per tail tile, extra workgroups
  int finish = FIN_NONE;
  int ws_src = WS_SRC_NONE;
  long ws_floats = 0;  // fp32 slab floats the launch writes (caller's workspace or the scratch)
  bool ok() const { return family != FAM_REFUSED; }
};
constexpr int kRouteFields = 16;
void gemm_route_fields(const Route& r, long out[kRouteFields]);

Route gemm_route(const PlanEnv& env, const GemmCall& c);

// the knob ops' overrides: throw std::runtime_error on a tile kGemmTiles does not hold
void gemm_grouped_plan(int bm, int bn, int stages, int splits);
void gemm_dense_plan(int variant, int bm, int bn, int splits, int stages);

// ---- predicates (arithmetic on shapes and knobs) ----
bool gemv_takes(const PlanEnv& e, int M, int N, int K, int epi);
bool gemv_chain_takes(const PlanEnv& e, int M, int N, int K, int epi);
bool gemv_grouped_takes(int M, int N, int K, int epi);
bool ws_takes(const PlanEnv& e, int M, int N, int K, int epi);
bool ws_prefer(const PlanEnv& e, int M, int N, int K, int epi);
int decode_chain_max_m(const PlanEnv& e);
bool decode_chain_takes(const PlanEnv& e, int M, int N, int K, int epi);
bool gemm_w4_ok(int M, int N, int K, int lda, int ldb, int ldc);
bool gemm_w4_split_ok(const PlanEnv& e, int T, int nk);
bool sk_halves_ok(const PlanEnv& e, long T, int nk);
// views of the route
bool gemm_rope_supported(const PlanEnv& e, int M, int N, int K);
bool w4_chain_ok(const PlanEnv& e, int M, int N, int K);
bool mid_chain_ok(const PlanEnv& e, int M, int N, int K, int epi);
// the norm chain's GEMM of epilogue epi (0 O / down, 1 gate_up, 3 QKV + RoPE; -1: not given)
// runs at M rows.  Up to decode_chain_max_m rows the decode forms count, up to 64 rows with an
// epilogue given only the mid chain, else only the four-wave chain.
bool chain_ok(const PlanEnv& e, int M, int N, int K, int epi);
long gemm_workspace_floats(const PlanEnv& e, int M, int N, int K, int epi);
int gemm_sk_workgroups(const PlanEnv& e, int M, int N, int K);

}  // namespace mlop
