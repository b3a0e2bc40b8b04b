// Sampler extensions (K10) for gfx950: repetition / frequency / presence penalties from a
// device-resident count table, and per-token log-probabilities with the top-N alternatives.
//
// Count table: int32 [slots, ldt >= V], one row per penalised request.  Bit 31 = the id occurs
// in the request's prompt, bits 0..30 = how often it occurs in the request's output.  The table
// is only ever written by the kernels below (vector stores and ordinary atomics), all on the
// engine's stream, so a draw always sees every earlier step's token.
//
// Log-probabilities: stage 1 splits a row into slices of <= kLpSlice columns, one workgroup
// each: the slice is read once (16-B loads, bf16 or fp32 input) into registers, reduced to
// (max, sum exp(x - max)) and to its own top N.  The row's top N is inside the union of the
// slices' top N, so stage 2 (one workgroup per row) merges the slices' (max, sum) pairs online,
// sorts the S * N candidates (value descending, ties by lower id) and writes
// logits - logsumexp for the chosen token and the N best.
#include <algorithm>

#include "common.h"
#include "launch.h"
#include "sampling_common.h"

namespace mlop {

constexpr int kLpSlice = 8192;    // columns of one stage-1 slice: 32 per thread, in registers
constexpr int kLpMax = 20;        // top-N bound (sampler.MAX_LOGPROBS)
constexpr int kLpMaxSplits = 48;  // kLpMaxSplits * kLpMax <= kLpCand
constexpr int kLpCand = 1024;     // stage 2's sort capacity

// ---- count table -------------------------------------------------------------------------
__global__ void __launch_bounds__(kSampleThreads) penalty_zero_kernel(int* __restrict__ row, int V4) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < V4) reinterpret_cast<int4*>(row)[j] = make_int4(0, 0, 0, 0);
}

__global__ void __launch_bounds__(kSampleThreads) penalty_fill_kernel(int* __restrict__ row, int V,
                                                                     const long* __restrict__ prompt, int np,
                                                                     const long* __restrict__ output, int no) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < np) {
    const long t = prompt[j];
    if (t >= 0 && t < V) atomicOr(&row[t], (int)0x80000000);
  } else if (j < np + no) {
    const long t = output[j - np];
    if (t >= 0 && t < V) atomicAdd(&row[t], 1);
  }
}

__global__ void __launch_bounds__(kSampleThreads) penalty_update_kernel(int* __restrict__ table, long ldt, int V,
                                                                       int nslots, const int* __restrict__ slots,
                                                                       const long* __restrict__ tokens, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int slot = slots[i];
  const long t = tokens[i];
  if (slot < 0 || slot >= nslots || t < 0 || t >= V) return;
  atomicAdd(&table[slot * ldt + t], 1);
}

// ---- penalties -----------------------------------------------------------------------------
// HF repetition penalty on seen ids, then frequency * count, then presence for counted ids
__device__ __forceinline__ float penalise(float l, int w, float r, float f, float p) {
  const int c = w & 0x7fffffff;
  if (r != 1.f) l = l > 0.f ? l / r : l * r;
  l -= f * (float)c;
  if (c > 0) l -= p;
  return l;
}

// grid (S, n): workgroup s of row i handles 16-B chunks [s * per, (s + 1) * per); only logits
// whose table word is non-zero are read and rewritten, rows with slot < 0 are not touched
__global__ void __launch_bounds__(kSampleThreads) apply_penalties_kernel(
    float* __restrict__ logits, int V, long ld, const int* __restrict__ table, long ldt, int nslots,
    const int* __restrict__ slots, const float* __restrict__ rep, const float* __restrict__ freq,
    const float* __restrict__ pres, int per) {
  const int s = blockIdx.x, S = gridDim.x, row_id = blockIdx.y;
  const int slot = slots[row_id];
  if (slot < 0 || slot >= nslots) return;
  const float r = rep[row_id], f = freq[row_id], p = pres[row_id];
  float* row = logits + row_id * ld;
  const int* trow = table + slot * ldt;
  const int nv4 = V >> 2;
  const int j0 = s * per, j1 = min(nv4, j0 + per);
  float4* l4 = reinterpret_cast<float4*>(row);
  const int4* t4 = reinterpret_cast<const int4*>(trow);
  for (int j = j0 + threadIdx.x; j < j1; j += blockDim.x) {
    const int4 w = t4[j];
    if ((w.x | w.y | w.z | w.w) == 0) continue;
    float4 x = l4[j];
    if (w.x) x.x = penalise(x.x, w.x, r, f, p);
    if (w.y) x.y = penalise(x.y, w.y, r, f, p);
    if (w.z) x.z = penalise(x.z, w.z, r, f, p);
    if (w.w) x.w = penalise(x.w, w.w, r, f, p);
    l4[j] = x;
  }
  if (s == S - 1)
    for (int j = (nv4 << 2) + threadIdx.x; j < V; j += blockDim.x) {
      const int w = trow[j];
      if (w) row[j] = penalise(row[j], w, r, f, p);
    }
}

// ---- log-probabilities ---------------------------------------------------------------------
__device__ __forceinline__ float block_max(float v, float* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  v = wave_max(v);
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  float t = scratch[0];
  for (int i = 1; i < nw; ++i) t = fmaxf(t, scratch[i]);
  __syncthreads();
  return t;
}

// stage 1, grid (S, n): slice s of row i -> part[(i * S + s) * 2] = (max, sum exp(x - max)) and
// the slice's top min(N, len) as kLpMax (value, id) candidates, value descending, ties by lower
// id (-inf / 0x7fffffff padding).  `per` is a multiple of 8, so every slice starts on a 16-B
// boundary of an aligned row.  The slice lives in REGISTERS (32 values per thread, one global
// pass of 16-B loads): each wave extracts the top N of its 64 lanes' values in N rounds of a
// shuffle arg-max (only the winning lane rescans, and only the 8 values of one group), the four waves'
// 4 N candidates are ranked against each other in LDS.  (A radix select over an LDS copy of
// the slice, as sample_presel_kernel does for K <= 1024, was 5x slower here: its histogram
// atomics collide on the few exponent buckets, and N <= 20 needs no general select.)
template <bool BF>
__global__ void __launch_bounds__(kSampleThreads) logprob_slice_kernel(
    float* __restrict__ part, float* __restrict__ cand_v, int* __restrict__ cand_i,
    const void* __restrict__ logits, int V, long ld, const int* __restrict__ want, int per) {
  constexpr int E = kLpSlice / kSampleThreads;  // values per thread
  constexpr int W = BF ? 8 : 4;                 // values per 16-B load
  constexpr int NW = kSampleThreads / 64;
  __shared__ float red[NW];
  __shared__ float wv_s[NW * kLpMax];
  __shared__ int wi_s[NW * kLpMax];
  __shared__ int s_real;
  const int s = blockIdx.x, S = gridDim.x, row_id = blockIdx.y, tid = threadIdx.x;
  const int lane = tid & 63, wid = tid >> 6;
  int N = want[row_id];
  if (N < 0) return;
  N = min(N, kLpMax);
  if (tid == 0) s_real = 0;
  const int j0 = s * per, len = max(0, min(per, V - j0));
  // thread t's value e is slice element W * ((e / W) * 256 + t) + e % W
  float v[E];
#pragma unroll
  for (int q = 0; q < E / W; ++q) {
    const int c0 = W * (q * kSampleThreads + tid);
    if (BF) {
      const uint16_t* row = (const uint16_t*)logits + row_id * ld + j0;
      if (c0 + W <= len) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(row + c0);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          v[q * W + 2 * k] = lo_bf(x[k]);
          v[q * W + 2 * k + 1] = hi_bf(x[k]);
        }
      } else {
#pragma unroll
        for (int k = 0; k < W; ++k) v[q * W + k] = c0 + k < len ? bf2f(row[c0 + k]) : -INFINITY;
      }
    } else {
      const float* row = (const float*)logits + row_id * ld + j0;
      if (c0 + W <= len) {
        const float4 x = *reinterpret_cast<const float4*>(row + c0);
        v[q * W] = x.x;
        v[q * W + 1] = x.y;
        v[q * W + 2] = x.z;
        v[q * W + 3] = x.w;
      } else {
#pragma unroll
        for (int k = 0; k < W; ++k) v[q * W + k] = c0 + k < len ? row[c0 + k] : -INFINITY;
      }
    }
  }
  float m = -INFINITY;
#pragma unroll
  for (int e = 0; e < E; ++e) m = fmaxf(m, v[e]);
  m = block_max(m, red);
  float sum = 0.f;
  if (m > -INFINITY) {
#pragma unroll
    for (int e = 0; e < E; ++e) sum += __expf(v[e] - m);  // padding: exp(-inf) = 0
  }
  sum = block_sum(sum, red);
  const size_t pi = (size_t)row_id * S + s;
  if (tid == 0) {
    part[2 * pi] = m;
    part[2 * pi + 1] = sum;
  }
  // A lane gives up its values in the order "value descending, then id ascending", so what it
  // has left is exactly what comes after its last winner (lim_v, lim_i).  Its values sit in G
  // groups of GE with a best each: a winner changes only its own group's best, so the lane
  // rescans GE values per round, not all E.  rescan(g < 0): every group.  None left: (-inf,
  // 0x7fffffff).
  constexpr int G = 4, GE = E / G;
  static_assert(GE % W == 0, "a 16-B load's values share a group");
  float gv[G], bv;
  int gi[G], bi;
  auto rescan = [&](int gsel, float lim_v, int lim_i) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if (gsel >= 0 && g != gsel) continue;
      float b = -INFINITY;
      int b_i = 0x7fffffff;
#pragma unroll
      for (int k = 0; k < GE; ++k) {
        const int e = g * GE + k;
        const int idx = W * ((e / W) * kSampleThreads + tid) + e % W;
        const float x = v[e];
        if (idx < len && (x < lim_v || (x == lim_v && idx > lim_i))) amax_merge(b, b_i, x, idx);
      }
      gv[g] = b;
      gi[g] = b_i;
    }
    bv = gv[0];
    bi = gi[0];
#pragma unroll
    for (int g = 1; g < G; ++g) amax_merge(bv, bi, gv[g], gi[g]);
  };
  rescan(-1, INFINITY, -1);
  for (int r = 0; r < N; ++r) {
    float wv = bv;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(wv, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      amax_merge(wv, wi, ov, oi);
    }
    if (lane == 0) {
      wv_s[wid * kLpMax + r] = wv;
      wi_s[wid * kLpMax + r] = wi;
    }
    // the winner's lane moves on: value e = (idx / (W * 256)) * W + idx % W, group e / GE
    if (bi == wi && wi != 0x7fffffff) rescan(((wi / (W * kSampleThreads)) * W) / GE, wv, wi);
  }
  __syncthreads();
  // rank the NW * N candidates against each other: a real candidate's rank is its place
  const int C = NW * N;
  const size_t base = pi * kLpMax;
  float cv = -INFINITY;
  int ci = 0x7fffffff, rank = 0;
  if (tid < C) {
    cv = wv_s[(tid / N) * kLpMax + tid % N];
    ci = wi_s[(tid / N) * kLpMax + tid % N];
    if (ci != 0x7fffffff) {
      for (int j = 0; j < C; ++j) {
        const float ov = wv_s[(j / N) * kLpMax + j % N];
        const int oi = wi_s[(j / N) * kLpMax + j % N];
        rank += (ov > cv || (ov == cv && oi < ci)) ? 1 : 0;
      }
      atomicAdd(&s_real, 1);
    }
  }
  __syncthreads();
  if (ci != 0x7fffffff && rank < N) {
    cand_v[base + rank] = cv;
    cand_i[base + rank] = j0 + ci;
  }
  const int filled = min(s_real, N);
  for (int j = filled + tid; j < kLpMax; j += blockDim.x) {
    cand_v[base + j] = -INFINITY;
    cand_i[base + j] = 0x7fffffff;
  }
}

// stage 2, one workgroup per row: online merge of the S (max, sum) pairs, bitonic sort of the
// S * N candidates, out[:, 0] = the chosen token, out[:, 1 .. N] = the top N
template <bool BF>
__global__ void __launch_bounds__(kSampleThreads) logprob_merge_kernel(
    float* __restrict__ out_lp, int* __restrict__ out_id, int ldo, const float* __restrict__ part,
    const float* __restrict__ cand_v, const int* __restrict__ cand_i, const void* __restrict__ logits, int V,
    long ld, const long* __restrict__ chosen, const int* __restrict__ want, int S) {
  __shared__ float cv[kLpCand];
  __shared__ int ci[kLpCand];
  const int row_id = blockIdx.x, tid = threadIdx.x;
  int N = want[row_id];
  if (N < 0) return;
  N = min(min(N, kLpMax), ldo - 1);
  // every thread merges the S pairs itself (S <= kLpMaxSplits, the loads hit the cache)
  float M = -INFINITY, sum = 0.f;
  for (int s = 0; s < S; ++s) {
    const float m = part[2 * ((size_t)row_id * S + s)], z = part[2 * ((size_t)row_id * S + s) + 1];
    if (m > M) {
      sum = sum * __expf(M - m) + z;
      M = m;
    } else if (m > -INFINITY) {
      sum += z * __expf(m - M);
    }
  }
  const float lsum = logf(sum);
  if (tid == 0) {
    const long c = chosen[row_id];
    float x = NAN;
    if (c >= 0 && c < V) x = BF ? bf2f(((const uint16_t*)logits)[row_id * ld + c]) : ((const float*)logits)[row_id * ld + c];
    out_lp[(size_t)row_id * ldo] = (x - M) - lsum;
    out_id[(size_t)row_id * ldo] = (int)c;
  }
  if (N == 0) return;
  const int C = S * N;
  int P = 1;
  while (P < C) P <<= 1;
  for (int j = tid; j < P; j += blockDim.x) {
    if (j < C) {
      const size_t src = ((size_t)row_id * S + j / N) * kLpMax + j % N;
      cv[j] = cand_v[src];
      ci[j] = cand_i[src];
    } else {
      cv[j] = -INFINITY;
      ci[j] = 0x7fffffff;
    }
  }
  __syncthreads();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < P / 2; t += blockDim.x) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = ((lo & size) == 0);
        const float a = cv[lo], b = cv[hi];
        const int ia = ci[lo], ib = ci[hi];
        const bool a_first = (a > b) || (a == b && ia < ib);
        if (a_first != desc) {
          cv[lo] = b; cv[hi] = a;
          ci[lo] = ib; ci[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
  for (int j = tid; j < N && j < C; j += blockDim.x) {
    if (ci[j] == 0x7fffffff) continue;  // fewer than N columns in the row
    out_lp[(size_t)row_id * ldo + 1 + j] = (cv[j] - M) - lsum;
    out_id[(size_t)row_id * ldo + 1 + j] = ci[j];
  }
}

// ---- launchers -----------------------------------------------------------------------------
void launch_penalty_reset(int* row, int V, int ldt, const long* prompt, int np, const long* output, int no,
                          hipStream_t st) {
  const int v4 = ldt >> 2;  // ldt is a multiple of 4: the padding is zeroed too
  penalty_zero_kernel<<<cdiv(v4, kSampleThreads), kSampleThreads, 0, st>>>(row, v4);
  if (np + no > 0)
    penalty_fill_kernel<<<cdiv(np + no, kSampleThreads), kSampleThreads, 0, st>>>(row, V, prompt, np, output, no);
}

void launch_penalty_update(int* table, long ldt, int V, int nslots, const int* slots, const long* tokens, int n,
                           hipStream_t st) {
  if (n == 0) return;
  penalty_update_kernel<<<cdiv(n, kSampleThreads), kSampleThreads, 0, st>>>(table, ldt, V, nslots, slots, tokens, n);
}

// workgroups per row: ~256 workgroups on the chip, >= 2 16-B chunks per thread
int penalty_splits(int n, int V) {
  if (n <= 0 || n >= 128) return 1;
  const int by_size = V / (4 * kSampleThreads * 2);
  return std::max(1, std::min({64, by_size, (256 + n - 1) / n}));
}

void launch_apply_penalties(float* logits, int n, int V, long ld, const int* table, long ldt, int nslots,
                            const int* slots, const float* rep, const float* freq, const float* pres,
                            hipStream_t st) {
  if (n == 0) return;
  const int S = penalty_splits(n, V);
  const int per = cdiv(V >> 2, S);
  apply_penalties_kernel<<<dim3(S, n), kSampleThreads, 0, st>>>(logits, V, ld, table, ldt, nslots, slots, rep, freq,
                                                                pres, per);
}

// slices per row: as many as the LDS slice needs, more for small batches; 0 = V too large
int logprob_splits(int n, int V) {
  if (n <= 0 || V <= 0) return 1;
  const int need = cdiv(V, kLpSlice);
  if (need > kLpMaxSplits) return 0;
  return std::max(need, std::min({kLpMaxSplits, cdiv(V, 512), cdiv(256, n)}));
}

long logprob_workspace_bytes(int n, int V) {
  const int S = logprob_splits(n, V);
  return (long)n * S * (2 * sizeof(float) + kLpMax * (sizeof(float) + sizeof(int)));
}

void launch_token_logprobs(float* out_lp, int* out_id, int ldo, const void* logits, bool bf16, int n, int V,
                           long ld, const long* chosen, const int* want, void* ws, hipStream_t st) {
  if (n == 0) return;
  const int S = logprob_splits(n, V);
  const int per = cdiv(cdiv(V, S), 8) * 8;  // <= kLpSlice: need <= S and kLpSlice % 8 == 0
  float* part = (float*)ws;
  float* cv = part + (size_t)n * S * 2;
  int* ci = (int*)(cv + (size_t)n * S * kLpMax);
  if (bf16) {
    logprob_slice_kernel<true><<<dim3(S, n), kSampleThreads, 0, st>>>(part, cv, ci, logits, V, ld, want, per);
    logprob_merge_kernel<true><<<n, kSampleThreads, 0, st>>>(out_lp, out_id, ldo, part, cv, ci, logits, V, ld, chosen,
                                                            want, S);
  } else {
    logprob_slice_kernel<false><<<dim3(S, n), kSampleThreads, 0, st>>>(part, cv, ci, logits, V, ld, want, per);
    logprob_merge_kernel<false><<<n, kSampleThreads, 0, st>>>(out_lp, out_id, ldo, part, cv, ci, logits, V, ld, chosen,
                                                             want, S);
  }
}

}  // namespace mlop
