// Guided decoding (K18) for gfx950: mask a row's logits by the state of its grammar automaton
// before the draw, advance the state by the drawn token behind it.
//
// Arena: int16 [A, ldv], ldv = V rounded up to 8, so every arena row starts on a 16-B boundary.
// A compiled grammar (runtime/guided.py) occupies the rows [base, base + S): entry [base + s, t]
// is the state (local to the grammar) after token t in state s, < 0 = t is not allowed there.
// Row state: int32 [R], indexed by engine row.  Both are only ever written on the engine's
// stream (uploads, admission fills and grammar_advance_kernel), so a draw launched one step
// ahead of the host still sees the state behind the previous token.
#include <algorithm>

#include "common.h"
#include "launch.h"
#include "sampling_common.h"

namespace mlop {

// The arena row of logits row i, or -1: the row is not guided, or an index is out of range
// (never read outside the arena or the state vector).
__device__ __forceinline__ long grammar_row(const int* __restrict__ base, const int* __restrict__ rows,
                                            const int* __restrict__ state, int i, int A, int R) {
  const int b = base[i];
  if (b < 0) return -1;
  const int r = rows[i];
  if (r < 0 || r >= R) return -1;
  const int s = state[r];
  if (s < 0 || (long)b + s >= A) return -1;
  return (long)b + s;
}

// grid (S, n): workgroup s of row i handles the 8-entry chunks [s * per, (s + 1) * per): one
// 16-B table load; where a chunk has a disallowed entry, the two 16-B logits loads / stores
// beside it.  A logits row that does not start on 16 B (odd ld) takes scalar accesses over the
// same range; the last workgroup of a row also takes the V % 8 tail.  Kept entries are never
// rewritten with a computed value: bit-exact.
__global__ void __launch_bounds__(kSampleThreads) grammar_mask_kernel(
    float* __restrict__ logits, int V, long ld, const short* __restrict__ arena, long ldv, int A,
    const int* __restrict__ base, const int* __restrict__ rows, const int* __restrict__ state, int R, int per) {
  const int s = blockIdx.x, S = gridDim.x, i = blockIdx.y;
  const long ar = grammar_row(base, rows, state, i, A, R);
  if (ar < 0) return;
  float* row = logits + i * ld;
  const short* trow = arena + ar * ldv;
  const int nv8 = V >> 3;
  const int j0 = min(nv8, s * per), j1 = min(nv8, j0 + per);
  const float ninf = -INFINITY;
  if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
    const int4* t8 = reinterpret_cast<const int4*>(trow);
    float4* l4 = reinterpret_cast<float4*>(row);
    for (int j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
      const int4 w = t8[j];  // 8 int16: the sign bits are bits 15 and 31 of each word
      if (((w.x | w.y | w.z | w.w) & (int)0x80008000) == 0) continue;
      float4 a = l4[2 * j], b = l4[2 * j + 1];
      if (w.x & 0x8000) a.x = ninf;
      if (w.x < 0) a.y = ninf;
      if (w.y & 0x8000) a.z = ninf;
      if (w.y < 0) a.w = ninf;
      if (w.z & 0x8000) b.x = ninf;
      if (w.z < 0) b.y = ninf;
      if (w.w & 0x8000) b.z = ninf;
      if (w.w < 0) b.w = ninf;
      l4[2 * j] = a;
      l4[2 * j + 1] = b;
    }
  } else {
    for (int j = (j0 << 3) + threadIdx.x; j < (j1 << 3); j += blockDim.x)
      if (trow[j] < 0) row[j] = ninf;
  }
  if (s == S - 1)
    for (int j = (nv8 << 3) + threadIdx.x; j < V; j += blockDim.x)
      if (trow[j] < 0) row[j] = ninf;
}

__global__ void __launch_bounds__(kSampleThreads) grammar_advance_kernel(
    const short* __restrict__ arena, long ldv, int A, int V, const int* __restrict__ base,
    const int* __restrict__ rows, int* __restrict__ state, int R, const long* __restrict__ tokens, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long ar = grammar_row(base, rows, state, i, A, R);
  if (ar < 0) return;
  const long t = min(max(tokens[i], 0L), (long)V - 1);
  const int nx = arena[ar * ldv + t];
  // nx < 0: a token the state does not allow (the stale row of a step launched ahead of the
  // host, drawn after its request ended): the state stays
  if (nx >= 0) state[rows[i]] = nx;
}

// workgroups per row: ~256 workgroups on the chip, >= 2 chunks (32 B of table) per thread
int grammar_splits(int n, int V) {
  if (n <= 0 || n >= 128) return 1;
  const int by_size = V / (8 * kSampleThreads * 2);
  return std::max(1, std::min({64, by_size, (256 + n - 1) / n}));
}

void launch_grammar_mask(float* logits, int n, int V, long ld, const short* arena, long ldv, int A,
                         const int* base, const int* rows, const int* state, int R, hipStream_t st) {
  if (n == 0) return;
  const int S = grammar_splits(n, V);
  const int per = cdiv(V >> 3, S);
  grammar_mask_kernel<<<dim3(S, n), kSampleThreads, 0, st>>>(logits, V, ld, arena, ldv, A, base, rows, state, R, per);
}

void launch_grammar_advance(const short* arena, long ldv, int A, int V, const int* base, const int* rows,
                            int* state, int R, const long* tokens, int n, hipStream_t st) {
  if (n == 0) return;
  grammar_advance_kernel<<<cdiv(n, kSampleThreads), kSampleThreads, 0, st>>>(arena, ldv, A, V, base, rows, state, R,
                                                                           tokens, n);
}

}  // namespace mlop
