// Prints the GEMM planner's route (ops/csrc/gemm_plan.h) of every row count for the shapes on
// stdin: tests/test_gemm_plan_cpu.py pins the output against tests/fixtures/gemm_routes_gfx950.txt.
//
//   gemm_plan_dump <cus> <sk 0|1> [big_variant]  <  lines "op N K n_groups"
//
// M runs over 1..8192, 12288 and 16384.  A grouped shape (n_groups > 0, Mixtral's top-2 routing)
// is asked with 2 M routed rows in all and ceil(2 M / n_groups) rows per group.  One output line
// per shape, "op N K n_groups |" and then one "M_first-M_last:route" item per maximal M interval
// with a constant route.  A route is its kernel family and what is not implied by it:
//   -  refused      V  GEMV      S  weight-streaming      W  four-wave      H  four-wave half height
//   P  ping-pong, P<d> with a stream-K tail of d K ranges per tail tile
//   T<i>  tile i of the tile table, then s<splits>k<k_chunk> where K is split, f<finish> and
//         w<ws_src> where not 0 (gemm_plan.h GemmFinish / GemmWsSrc)
// then "+" where gemm_rope_supported (op 3) and "c" where chain_ok with the chain op's epilogue
// (ops 4, 9, 11) hold.  The route fields left out are checked here against what implies them
// (the tile's BM .. setprio against the table, m_tiles against the rows, the tail's workgroups
// against sk_d, ws_floats against splits), so a wrong one fails the run.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "gemm_plan.h"

using namespace mlop;

static void require(bool ok, const char* what, int op, int M, int N, int K) {
  if (ok) return;
  fprintf(stderr, "inconsistent route (%s) at op %d M %d N %d K %d\n", what, op, M, N, K);
  exit(3);
}

static std::string route_item(const PlanEnv& env, int op, int M, int N, int K, int n_groups) {
  GemmCall c;
  c.op = op, c.N = N, c.K = K, c.M = M;
  if (n_groups > 0) {
    c.M = 2 * M;
    c.n_groups = n_groups;
    c.rows_per_group = (c.M + n_groups - 1) / n_groups;
  }
  const Route r = gemm_route(env, c);
  const bool tile = r.family == FAM_TILE;
  require(tile == (r.tile >= 0 && r.tile < kNumGemmTiles), "tile index", op, M, N, K);
  require(r.ws_floats == (r.splits > 1 ? (long)r.splits * c.M * N : 0), "ws_floats", op, M, N, K);
  require((r.ws_src != WS_SRC_NONE) == (r.splits > 1), "ws_src", op, M, N, K);
  require(r.sk_wgs == (r.sk_d ? (((N + 255) / 256) * ((c.M + 255) / 256)) % env.cus * r.sk_d : 0), "sk_wgs", op, M, N, K);
  require(r.sk_d == 0 || r.family == FAM_PP, "sk_d", op, M, N, K);
  std::string s;
  if (tile) {
    const TileCfg& t = kGemmTiles[r.tile];
    require(r.BM == t.BM && r.BN == t.BN && r.WM == t.WM && r.WN == t.WN && r.stages == t.stages &&
                r.setprio == (int)t.setprio, "tile fields", op, M, N, K);
    require(r.m_tiles == (c.M + t.BM - 1) / t.BM + n_groups, "m_tiles", op, M, N, K);
    require(r.splits > 1 || r.k_chunk == K, "k_chunk", op, M, N, K);
    s = "T" + std::to_string(r.tile);
    if (r.splits > 1) s += "s" + std::to_string(r.splits) + "k" + std::to_string(r.k_chunk);
    if (r.finish) s += "f" + std::to_string(r.finish);
    if (r.ws_src) s += "w" + std::to_string(r.ws_src);
  } else {
    require(r.splits == 1 && (r.finish == FIN_NONE || (r.family == FAM_WS && r.finish == FIN_RMSNORM)), "finish", op, M, N, K);
    s = std::string(1, "-VST PWH"[r.family == FAM_PP ? 5 : r.family == FAM_W4 ? 6 : r.family == FAM_W4H ? 7 : r.family]);
    if (r.finish) s += "f" + std::to_string(r.finish);
    if (r.sk_d) s += std::to_string(r.sk_d);
  }
  if (op == OP_ROPE) {
    require(gemm_rope_supported(env, M, N, K) == r.ok(), "gemm_rope_supported", op, M, N, K);
    if (r.ok()) s += "+";
  }
  const int cepi = op == OP_CHAIN_RES_SS ? 0 : op == OP_CHAIN_RS_SILU ? 1 : op == OP_CHAIN_RS_ROPE ? 3 : -1;
  if (cepi >= 0 && chain_ok(env, M, N, K, cepi)) s += "c";
  return s;
}

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: gemm_plan_dump cus sk [big_variant] < shapes\n");
    return 2;
  }
  PlanEnv env;
  env.cus = atoi(argv[1]);
  env.sk = atoi(argv[2]) != 0;
  if (argc > 3) env.big_variant = atoi(argv[3]);
  std::vector<int> ms;
  for (int m = 1; m <= 8192; ++m) ms.push_back(m);
  ms.push_back(12288);
  ms.push_back(16384);
  int op, N, K, ng;
  while (scanf("%d %d %d %d", &op, &N, &K, &ng) == 4) {
    printf("%d %d %d %d |", op, N, K, ng);
    std::string cur;
    int first = 0, last = 0;
    for (int m : ms) {
      const std::string s = route_item(env, op, m, N, K, ng);
      if (s != cur) {
        if (!cur.empty()) printf(" %d-%d:%s", first, last, cur.c_str());
        cur = s;
        first = m;
      }
      last = m;
    }
    printf(" %d-%d:%s\n", first, last, cur.c_str());
  }
  return 0;
}
