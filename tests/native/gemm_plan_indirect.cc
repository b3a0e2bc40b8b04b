// Prints the GEMM planner's route of grouped calls with GemmCall::indirect set (A rows through
// a_rows, or the split-K slabs handed to the caller: launch_grouped_gemm), which the dump program
// and the pinned table do not cover: tests/test_moe_probes_cpu.py compares it with the table.
//
//   gemm_plan_indirect <cus> <sk 0|1> <big_variant>  <  lines "op N K n_groups rows rows_per_group"
//
// One output line per input line: "<family letter> <tile or -1> <splits> <k_chunk>".
#include <cstdio>
#include <cstdlib>

#include "gemm_plan.h"

using namespace mlop;

int main(int argc, char** argv) {
  if (argc < 4) {
    fprintf(stderr, "usage: gemm_plan_indirect cus sk big_variant < calls\n");
    return 2;
  }
  PlanEnv env;
  env.cus = atoi(argv[1]);
  env.sk = atoi(argv[2]) != 0;
  env.big_variant = atoi(argv[3]);
  int op, N, K, ng, M, rpg;
  while (scanf("%d %d %d %d %d %d", &op, &N, &K, &ng, &M, &rpg) == 6) {
    GemmCall c;
    c.op = op, c.N = N, c.K = K, c.M = M, c.n_groups = ng, c.rows_per_group = rpg;
    c.indirect = true;
    const Route r = gemm_route(env, c);
    const int f = r.family == FAM_PP ? 5 : r.family == FAM_W4 ? 6 : r.family == FAM_W4H ? 7 : r.family;
    printf("%c %d %d %d\n", "-VST PWH"[f], r.family == FAM_TILE ? r.tile : -1, r.splits, r.k_chunk);
  }
  return 0;
}
