// Speculative decoding by prompt lookup for gfx950: the accept rule and the n-gram proposer
// (runtime/spec.py is the contract: accept_reference / propose_reference, token for token).
//
// State: hist int32 [R, max_len] (every token of a running row: prompt + output) and
// hist_len int32 [R], device-resident like the penalty count table and only ever written on the
// engine's stream by spec_accept (and the host's copy when a row is admitted).
//
// Per-step result out int32 [B, 2 + (k + 1) + k]: [emitted count a + 1, next draft count,
// k + 1 emitted tokens, k next drafts]; spec_accept writes columns 0 and 2.., spec_propose
// (launched behind it) columns 1 and 3 + k..; the host reads the whole thing back once.
//
// Integers only, no global atomics: the result does not depend on the order workgroups or
// waves run in.  All stores are ordinary per-lane (vector) stores.
#include <limits.h>

#include "common.h"
#include "launch.h"

namespace mlop {

constexpr int kSpecMaxK = 7;       // drafts per row (spec.MAX_SPEC_TOKENS)
constexpr int kSpecMaxN = 8;       // n-gram length (spec.MAX_NGRAM)
constexpr int kProposeThreads = 256;

// one lane per row: a = leading drafts the sampler reproduced; sampled[qs .. qs + a] are emitted
// and appended to the row's history
__global__ void __launch_bounds__(64) spec_accept_kernel(
    const long* __restrict__ sampled, int T, const int* __restrict__ q_start, const int* __restrict__ drafts,
    const int* __restrict__ nd, const int* __restrict__ rows, int* __restrict__ hist, long ld, int max_len,
    int* __restrict__ hist_len, int R, int* __restrict__ out, int W, int k, int B) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  int* o = out + (size_t)i * W;
  const int qs = q_start[i];
  if (qs < 0 || qs >= T) {  // (a malformed step: nothing emitted, nothing appended)
    o[0] = 0;
    return;
  }
  const int n = min(min(max(nd[i], 0), k), T - 1 - qs);
  int a = 0;
  while (a < n && sampled[qs + a] == (long)drafts[(size_t)i * k + a]) ++a;
  const int r = rows[i];
  const bool ok = r >= 0 && r < R;
  const int L = ok ? min(max(hist_len[r], 0), max_len) : 0;
  for (int j = 0; j <= a; ++j) {
    const int tok = (int)sampled[qs + j];
    o[2 + j] = tok;
    if (ok && L + j < max_len) hist[(size_t)r * ld + L + j] = tok;
  }
  if (ok) hist_len[r] = min(L + a + 1, max_len);
  o[0] = a + 1;
}

__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s));
  return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v = min(v, __shfl_xor(v, s));
  return v;
}

// One workgroup per row.  q = the LAST token of a candidate match, 0 <= q <= L - 2 (so one token
// at least follows it); m(q) = the longest m <= n_max with hist[q-m+1 .. q] == hist[L-m .. L-1].
// A length-n candidate starts at p = q - n + 1 exactly when m(q) >= n, and it can supply cap
// followers exactly when q <= L - 1 - cap.  Per n the block reduces the contract's two indices:
// the largest q among the full-follow candidates and the smallest q among all of them (p and q
// differ by a constant per n).  Threads stride over q: the loads of hist[q - j] are coalesced.
__global__ void __launch_bounds__(kProposeThreads) spec_propose_kernel(
    const int* __restrict__ hist, long ld, int max_len, const int* __restrict__ hist_len, int R,
    const int* __restrict__ rows, const int* __restrict__ cap, int n_max, int n_min, int* __restrict__ out, int W,
    int k) {
  __shared__ int s_suf[kSpecMaxN];                              // the suffix, last token first
  __shared__ int s_red[kProposeThreads / 64][2 * kSpecMaxN];   // per wave: max q (full), min q
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int i = blockIdx.x;
  int* o = out + (size_t)i * W;
  const int r = rows[i];
  const int c = min(max(cap[i], 0), k);
  const int L = (r >= 0 && r < R) ? min(max(hist_len[r], 0), max_len) : 0;
  if (c == 0 || L < n_min + 1) {  // (uniform over the workgroup)
    if (tid == 0) o[1] = 0;
    return;
  }
  const int* h = hist + (size_t)r * ld;
  if (tid < kSpecMaxN) s_suf[tid] = tid < L ? h[L - 1 - tid] : -1;
  __syncthreads();
  int mx[kSpecMaxN], mn[kSpecMaxN];
#pragma unroll
  for (int n = 0; n < kSpecMaxN; ++n) mx[n] = -1, mn[n] = INT_MAX;
  const int q_full = L - 1 - c;
  for (int q = tid; q <= L - 2; q += kProposeThreads) {
    const int lim = min(n_max, q + 1);
    int m = 0;
    bool go = true;
#pragma unroll
    for (int j = 0; j < kSpecMaxN; ++j) {
      if (go && j < lim) go = h[q - j] == s_suf[j];
      else go = false;
      m += go ? 1 : 0;
    }
#pragma unroll
    for (int n = 0; n < kSpecMaxN; ++n)
      if (n < m) {
        mn[n] = min(mn[n], q);
        if (q <= q_full) mx[n] = max(mx[n], q);
      }
  }
#pragma unroll
  for (int n = 0; n < kSpecMaxN; ++n) {
    const int a = wave_max_i(mx[n]), b = wave_min_i(mn[n]);
    if (lane == 0) s_red[wid][n] = a, s_red[wid][kSpecMaxN + n] = b;
  }
  __syncthreads();
  if (tid != 0) return;
  int count = 0, start = 0;
  for (int n = n_max; n >= n_min; --n) {
    int bmx = -1, bmn = INT_MAX;
    for (int w = 0; w < kProposeThreads / 64; ++w) {
      bmx = max(bmx, s_red[w][n - 1]);
      bmn = min(bmn, s_red[w][kSpecMaxN + n - 1]);
    }
    if (bmn == INT_MAX) continue;  // no candidate of this length
    start = (bmx >= 0 ? bmx : bmn) + 1;
    count = min(c, L - start);
    break;
  }
  o[1] = count;
  for (int j = 0; j < count; ++j) o[3 + k + j] = h[start + j];
}

void launch_spec_accept(const long* sampled, int T, const int* q_start, const int* drafts, const int* nd,
                        const int* rows, int* hist, long ld, int max_len, int* hist_len, int R, int* out, int k,
                        int B, hipStream_t st) {
  if (B <= 0) return;
  spec_accept_kernel<<<cdiv(B, 64), 64, 0, st>>>(sampled, T, q_start, drafts, nd, rows, hist, ld, max_len, hist_len,
                                                  R, out, 3 + 2 * k, k, B);
}

void launch_spec_propose(const int* hist, long ld, int max_len, const int* hist_len, int R, const int* rows,
                         const int* cap, int n_max, int n_min, int* out, int k, int B, hipStream_t st) {
  if (B <= 0) return;
  spec_propose_kernel<<<B, kProposeThreads, 0, st>>>(hist, ld, max_len, hist_len, R, rows, cap, n_max, n_min, out,
                                                     3 + 2 * k, k);
}

static_assert(kSpecMaxK + 1 <= 8 && kSpecMaxN <= 8, "a verify row is at most 8 query tokens");

}  // namespace mlop
