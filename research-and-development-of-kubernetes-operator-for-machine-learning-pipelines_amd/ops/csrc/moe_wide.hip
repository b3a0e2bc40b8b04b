// Wide MoE routing for gfx950: 128 experts, top-k <= 8 (Qwen3-MoE).  Two stream-ordered launches,
// no global atomics and no tickets between them (both graph-capturable):
//
//   moe_route_wide   topw, topi = top-k(softmax(bf16(x . Wr^T)))       one launch, T tokens
//   moe_place_wide   offsets, inv, arow from topi                      one workgroup
//
// At 128 experts the router is a real [T, H] x [H, 128] GEMM, so it runs on the matrix cores
// (v_mfma_f32_16x16x32_bf16) with the operands SWAPPED, as in lora.hip: the router rows are the
// row operand (M = experts), a wave's 16 tokens the column operand (N = tokens).  After the K loop
// lane l holds, for token l & 15, the experts 16 tile + 4 (l >> 4) + i of every tile: 32 logits of
// ONE token per lane, a token's 128 logits in the four lanes {c, c + 16, c + 32, c + 48} of its
// column.  Softmax and the top-k selection then need no LDS: 32 values in registers per lane and two
// cross-lane steps (v_permlane16_swap / v_permlane32_swap) per reduction.
//
// Two forms of the K loop:
//   tile form (T > 16): a workgroup is four waves = 64 tokens; the grid runs over 64-token tiles.
//     The router is read from global memory once per workgroup: 128 x 64 K-slabs (16 KB) go
//     through registers into a double-buffered LDS slab that all four waves read their row
//     fragments from (rows padded to 144 B: the 16 rows of a fragment fall on distinct banks).
//     Token fragments go from global memory straight into the operand layout (16 B per lane).
//   K-split form (T <= 16, decode): ONE workgroup; its four waves take one K quarter each of the
//     same 16-token tile, router fragments straight from global memory (each wave reads its own
//     columns: still one read of the matrix), the partial accumulators are summed through the LDS
//     in a fixed wave order.  The time is bounded by the latency of H / 4, not H.
// Rows past T are clamped on load and never written.
//
// Epilogue (both forms, registers only): each fp32 logit is rounded to bf16 and back (what the
// separate router projection stores); row max, p = exp(l - max) and its sum in a fixed order;
// k selection rounds on the bf16 LOGITS (a tie is a tie of representable numbers): every lane
// proposes its best unused (logit, id) as one ordered 64-bit key - the logit's order-preserving
// bits high, 255 - id low, so equal logits go to the lower id - the column's four lanes reduce
// by max and the owner retires the winner.  Weights p_j / sum stay fp32, divided by the sum of
// the k picked ones under renorm; topw / topi come out in descending order.
#include "common.h"
#include "launch.h"

namespace mlop {

namespace {

constexpr int kWideE = 128;        // experts (NT = 8 MFMA tiles); 256 is one more instantiation
constexpr int kWideSplitT = 16;    // T <= 16: the K-split form
constexpr int kWideMaxT = 16384;   // T * k <= 131072 slots for the placement
constexpr int kSlabK = 64;         // K columns of a router slab
constexpr int kSlabLd = kSlabK + 8;  // padded slab row (bf16 elements)

// float -> uint32 whose unsigned order is the float order
__device__ __forceinline__ uint32_t order_bits(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float order_float(uint32_t o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// max of a 64-bit key over the lane group {l, l^16, l^32, l^48} (max_x16_x32 of common.h on two dwords)
__device__ __forceinline__ uint64_t key_max_x16_x32(uint64_t key) {
  uint32_t lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
  auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  uint64_t a = ((uint64_t)rh[0] << 32) | rl[0], b = ((uint64_t)rh[1] << 32) | rl[1];
  key = a > b ? a : b;
  lo = (uint32_t)key, hi = (uint32_t)(key >> 32);
  rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  a = ((uint64_t)rh[0] << 32) | rl[0], b = ((uint64_t)rh[1] << 32) | rl[1];
  return a > b ? a : b;
}

// acc[t][i]: token column lane & 15, expert 16 t + 4 (lane >> 4) + i.  Writes row `tok` of topw / topi
template <int NT>
__device__ __forceinline__ void route_wide_epilogue(const f32x4 (&acc)[NT], int lane, int tok, int T, int k,
                                                    bool renorm, float* __restrict__ topw, int* __restrict__ topi) {
  constexpr int NV = 4 * NT;
  float v[NV];
  float mx = -INFINITY;
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    v[q] = bf2f(f2bf(acc[q >> 2][q & 3])) + 0.f;  // bf16 logit; -0 -> +0 (one order for equal values)
    mx = fmaxf(mx, v[q]);
  }
  mx = max_x16_x32(mx);
  float sum = 0.f;
#pragma unroll
  for (int q = 0; q < NV; ++q) sum += __expf(v[q] - mx);
  sum = sum_x16_x32(sum);  // commutative steps: the column's four lanes hold the same bits
  uint64_t key[NV];
#pragma unroll
  for (int q = 0; q < NV; ++q) {
    const int id = 16 * (q >> 2) + 4 * (lane >> 4) + (q & 3);
    key[q] = ((uint64_t)order_bits(v[q]) << 32) | (uint32_t)(255 - id);  // never 0: 0 marks "used"
  }
  float wsel[8], picked = 0.f;
  int isel[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (j >= k) break;  // wave-uniform
    uint64_t best = 0;
#pragma unroll
    for (int q = 0; q < NV; ++q) best = key[q] > best ? key[q] : best;
    best = key_max_x16_x32(best);
    // ids are unique over the column's four lanes: the low dword names the owner's entry
#pragma unroll
    for (int q = 0; q < NV; ++q)
      if ((uint32_t)key[q] == (uint32_t)best) key[q] = 0;
    isel[j] = 255 - (int)(uint32_t)best;
    // the winner's p from its logit: the same expression on the same bits as in the sum above
    wsel[j] = __expf(order_float((uint32_t)(best >> 32)) - mx) / sum;
    picked += wsel[j];
  }
  const float rn = renorm ? 1.f / picked : 1.f;
  if ((lane >> 4) == 0 && tok < T) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (j >= k) break;
      topw[(size_t)tok * k + j] = wsel[j] * rn;
      topi[(size_t)tok * k + j] = isel[j];
    }
  }
}

// NT: 16-expert MFMA tiles (E = 16 NT).  KSPLIT: grid 1, T <= 16, H % 128 == 0; else grid
// ceil(T / 64), H % 32 == 0.  256 threads.
template <int NT, bool KSPLIT>
__global__ void __launch_bounds__(256) moe_route_wide_kernel(float* __restrict__ topw, int* __restrict__ topi,
                                                             const uint16_t* __restrict__ x,
                                                             const uint16_t* __restrict__ wr, int T, int H, int k,
                                                             int renorm) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  if constexpr (KSPLIT) {
    const int kq = H >> 2, steps = kq >> 5;  // this wave's K quarter, in 32-column MFMA steps
    const int k0 = wv * kq + (lane >> 4) * 8;
    const bf16x8* xp = reinterpret_cast<const bf16x8*>(x + (size_t)min(lane & 15, T - 1) * H + k0);
    const bf16x8* ap = reinterpret_cast<const bf16x8*>(wr + (size_t)(lane & 15) * H + k0);
    const size_t tile = (size_t)2 * H;  // 16 router rows, in bf16x8 units
    // U K-steps in flight (lora.hip's register ring): the next group's loads are issued before
    // this group's MFMAs
    constexpr int U = 2;
    int st = 0;
    if (steps >= U) {
      bf16x8 aq[U][NT], xq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        xq[u] = xp[4 * u];
#pragma unroll
        for (int t = 0; t < NT; ++t) aq[u][t] = ap[t * tile + 4 * u];
      }
      for (; st + 2 * U <= steps; st += U) {
        bf16x8 ac[U][NT], xc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          xc[u] = xq[u];
#pragma unroll
          for (int t = 0; t < NT; ++t) ac[u][t] = aq[u][t];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
          xq[u] = xp[4 * (st + U + u)];
#pragma unroll
          for (int t = 0; t < NT; ++t) aq[u][t] = ap[t * tile + 4 * (st + U + u)];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[t] = mfma16(ac[u][t], xc[u], acc[t]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = mfma16(aq[u][t], xq[u], acc[t]);
      st += U;
    }
    for (; st < steps; ++st) {
      const bf16x8 xc = xp[4 * st];
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] = mfma16(ap[t * tile + 4 * st], xc, acc[t]);
    }
    // the four K quarters, summed by wave 0 in a fixed order
    __shared__ float red[4][4 * NT][64];
#pragma unroll
    for (int q = 0; q < 4 * NT; ++q) red[wv][q][lane] = acc[q >> 2][q & 3];
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int q = 0; q < 4 * NT; ++q)
      acc[q >> 2][q & 3] = (red[0][q][lane] + red[1][q][lane]) + (red[2][q][lane] + red[3][q][lane]);
    route_wide_epilogue<NT>(acc, lane, lane & 15, T, k, renorm != 0, topw, topi);
  } else {
    __shared__ __attribute__((aligned(16))) uint16_t slab[2][16 * NT][kSlabLd];
    const int t0 = blockIdx.x * 64 + wv * 16;
    const uint16_t* xr = x + (size_t)min(t0 + (lane & 15), T - 1) * H + (lane >> 4) * 8;
    // slab fill: 16 NT rows x 8 chunks of 16 B; thread -> chunk (tid & 7) of rows (tid >> 3) + 32 i
    constexpr int FI = 16 * NT / 32;
    const int frow = threadIdx.x >> 3, fcol = (threadIdx.x & 7) * 8;
    const uint16_t* wf = wr + (size_t)frow * H + fcol;
    const int nslab = cdiv(H, kSlabK);
    const u32x4 zero4 = {0u, 0u, 0u, 0u};
    const bf16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    u32x4 fr[FI];
    bf16x8 xq[2];
    // columns past H (the half slab of an H % 64 == 32 row) are fed as zeros
    auto gload = [&](int s) {
      const int c0 = s * kSlabK;
#pragma unroll
      for (int i = 0; i < FI; ++i)
        fr[i] = c0 + fcol < H ? *reinterpret_cast<const u32x4*>(wf + (size_t)32 * i * H + c0) : zero4;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        xq[ks] = c0 + 32 * ks < H ? *reinterpret_cast<const bf16x8*>(xr + c0 + 32 * ks) : zero8;
    };
    auto fill = [&](int b) {
#pragma unroll
      for (int i = 0; i < FI; ++i) *reinterpret_cast<u32x4*>(&slab[b][frow + 32 * i][fcol]) = fr[i];
    };
    gload(0);
    fill(0);
    __syncthreads();
    for (int s = 0; s < nslab; ++s) {
      const bf16x8 xc[2] = {xq[0], xq[1]};
      const bool more = s + 1 < nslab;
      if (more) gload(s + 1);  // in flight under this slab's MFMAs
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 a = *reinterpret_cast<const bf16x8*>(&slab[s & 1][16 * t + (lane & 15)][32 * ks + (lane >> 4) * 8]);
          acc[t] = mfma16(a, xc[ks], acc[t]);
        }
      // the other buffer was last read in iteration s - 1, before that iteration's barrier
      if (more) fill((s + 1) & 1);
      __syncthreads();
    }
    route_wide_epilogue<NT>(acc, lane, t0 + (lane & 15), T, k, renorm != 0, topw, topi);
  }
}

// One workgroup: counting sort of the T*k routed slots by local expert.  offsets [n_local + 1],
// inv [T*k] (slot -> permuted row, -1 when the expert is outside [e0, e0 + n_local)) and arow [T*k]
// (permuted row -> token row), with the meaning moe_dispatch_mid gives them.  Rows inside an
// expert come in ticket order (LDS atomics): no value depends on it.
__global__ void __launch_bounds__(1024) moe_place_wide_kernel(int* __restrict__ offsets, int* __restrict__ arow,
                                                              int* __restrict__ inv, const int* __restrict__ topi,
                                                              int n_slots, int k, int e0, int n_local) {
  __shared__ int cnt[256];
  __shared__ int base[256];
  for (int e = threadIdx.x; e < 256; e += blockDim.x) cnt[e] = 0;
  __syncthreads();
  for (int s = threadIdx.x; s < n_slots; s += blockDim.x) {
    const int e = topi[s] - e0;
    inv[s] = (e >= 0 && e < n_local) ? atomicAdd(&cnt[e], 1) : -1;  // rank inside its expert
  }
  __syncthreads();
  if (threadIdx.x < 64) {  // exclusive scan of the counts: four experts per lane, then over the wave
    const int l = threadIdx.x;
    int c[4], own = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      c[i] = 4 * l + i < n_local ? cnt[4 * l + i] : 0;
      own += c[i];
    }
    int incl = own;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (l >= d) incl += o;
    }
    int run = incl - own;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (4 * l + i < n_local) {
        base[4 * l + i] = run;
        offsets[4 * l + i] = run;
      }
      run += c[i];
    }
    if (l == 63) offsets[n_local] = incl;
  }
  __syncthreads();
  for (int s = threadIdx.x; s < n_slots; s += blockDim.x) {  // this thread's own pass-1 stores
    const int e = topi[s] - e0;
    if (e >= 0 && e < n_local) {
      const int row = base[e] + inv[s];
      inv[s] = row;
      arow[row] = s / k;
    }
  }
}

}  // namespace

bool moe_wide_takes(int T, int E, int k, int H) {
  if (T < 1 || T > kWideMaxT || E != kWideE || k < 1 || k > 8 || H < 128) return false;
  return T <= kWideSplitT ? H % 128 == 0 : H % 32 == 0;
}

void launch_moe_route_wide(float* topw, int* topi, const void* x, const void* wr, int T, int E, int k, int H,
                           bool renorm, hipStream_t st) {
  if (T <= 0) return;
  (void)E;  // 128 = 8 tiles: the only instantiation (moe_wide_takes)
  if (T <= kWideSplitT)
    moe_route_wide_kernel<kWideE / 16, true><<<1, 256, 0, st>>>(topw, topi, (const uint16_t*)x, (const uint16_t*)wr, T,
                                                                H, k, renorm ? 1 : 0);
  else
    moe_route_wide_kernel<kWideE / 16, false><<<cdiv(T, 64), 256, 0, st>>>(topw, topi, (const uint16_t*)x,
                                                                           (const uint16_t*)wr, T, H, k, renorm ? 1 : 0);
}

void launch_moe_place_wide(int* offsets, int* arow, int* inv, const int* topi, int T, int k, int e0, int n_local,
                           hipStream_t st) {
  moe_place_wide_kernel<<<1, 1024, 0, st>>>(offsets, arow, inv, topi, T * k, k, e0, n_local);
}

}  // namespace mlop
