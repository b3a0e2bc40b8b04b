// Multi-LoRA: the batched low-rank update of a ragged step in which every token may use a
// different adapter, or none.  Two launches beside each base projection y = x . W^T:
//
//   lora_shrink      tmp[t, :]  = A[slot(t)] . x[t]                      ([T, G R] fp32)
//   lora_expand_add  y[t, n]   += sum_r tmp[t, g(n) R + r] . B[slot(t), n, r]   (bf16, in place)
//
// Adapter storage is slot-major and fixed: A [S, G R, K] bf16 (G sub-projections sharing the
// input: q / k / v, gate / up), B [S, N, R] bf16 in the base weight's row layout with the
// scaling folded in; rows of smaller ranks and of absent target modules are zero, and
// slot_rank[S] lets both kernels skip the r-tiles that are all zero.  tile_group[N / 16] names
// the A block each 16-column output tile reads.  The only per-step input is tok_slot[T] (-1: no
// adapter; the row is left untouched by the expand and gets zeros from the shrink).
//
// Both kernels follow gemm_ws.hip: a 16-token tile on v_mfma_f32_16x16x32_bf16 with the weight
// rows loaded straight into the MFMA operand layout (common.h).  The operands are swapped with
// respect to gemm_ws (weights are the row operand, tokens the column operand), so a lane ends up
// with 4 consecutive outputs of ONE token: a 16-B fp32 / 8-B bf16 vector per lane.
// A 16-token tile may mix adapters (a prefill chunk boundary, any decode step): the wave loops
// over the distinct slots present in its tile (ballot + readlane, wave-uniform, so the MFMAs
// always run under a full EXEC mask), multiplies the whole tile by that slot's rows and keeps a
// token column's product only where the token uses the slot (what zero operand columns for the
// other tokens would give); every token belongs to one slot, so one accumulator serves the loop.
// No atomics: the shrink's four waves take one K quarter each and are combined through the LDS
// in a fixed order, so a launch is reproducible bit for bit.
#include "common.h"
#include "launch.h"

namespace mlop {

namespace {

// the slot of this lane's token column (l & 15) of tile t0, -1 for none / rows past T / a slot
// outside the storage (never trusted as an index)
__device__ __forceinline__ int lora_lane_slot(const int* __restrict__ tok_slot, int t0, int T, int S, int lane) {
  const int tok = t0 + (lane & 15);
  int s = tok < T ? tok_slot[tok] : -1;
  return (s < 0 || s >= S) ? -1 : s;
}

// next distinct slot among the lanes' pending ones (wave-uniform), or -1; marks its lanes done
__device__ __forceinline__ int lora_next_slot(int& pending, bool& mine) {
  const unsigned long long m = __ballot(pending >= 0);
  if (m == 0) return -1;
  const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
  const int s = __builtin_amdgcn_readlane(pending, leader);
  mine = pending == s;
  if (mine) pending = -1;
  return s;
}

// grid (ceil(T / 16), G R / 16), 256 threads: wave w reduces K quarter w of one 16 x 16 tile.
// (Sixteen waves with a sixteenth of K each measured the same at every shape: profiles/lora.md.)
__global__ void __launch_bounds__(256) lora_shrink_kernel(const uint16_t* __restrict__ x, int ldx,
                                                          const uint16_t* __restrict__ A, float* __restrict__ tmp,
                                                          const int* __restrict__ tok_slot,
                                                          const int* __restrict__ slot_rank, int T, int K, int GR,
                                                          int R, int S) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int t0 = blockIdx.x * 16, r0 = blockIdx.y * 16;
  const int rg = r0 % R;  // first rank index of this tile inside its A block
  int pending = lora_lane_slot(tok_slot, t0, T, S, lane);
  const int kq = K >> 2, steps = kq >> 5;
  const int k0 = wv * kq + (lane >> 4) * 8;
  const bf16x8* xp = reinterpret_cast<const bf16x8*>(x + (size_t)min(t0 + (lane & 15), T - 1) * ldx + k0);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // U K-steps in flight per wave (gemm_ws.hip's register ring): the next group's loads are issued
  // before this group's MFMAs, unconditionally, so the compiler keeps counted waits.  Every token
  // column is multiplied by the slot's rows; a lane keeps the product only if its token uses the
  // slot (the same as feeding zero columns for the other tokens, without touching the operands)
  constexpr int U = 4;
  for (;;) {
    bool mine = false;
    const int s = __builtin_amdgcn_readfirstlane(lora_next_slot(pending, mine));
    if (s < 0) break;
    if (rg >= slot_rank[s]) continue;  // rows rank.. of a slot are zero
    const bf16x8* ap = reinterpret_cast<const bf16x8*>(A + ((size_t)s * GR + r0 + (lane & 15)) * K + k0);
    f32x4 part = {0.f, 0.f, 0.f, 0.f};
    int st = 0;  // step = 32 k = 4 bf16x8 vectors
    if (steps >= U) {
      bf16x8 aq[U], xq[U];
#pragma unroll
      for (int u = 0; u < U; ++u) aq[u] = ap[4 * u], xq[u] = xp[4 * u];
      for (; st + 2 * U <= steps; st += U) {
        bf16x8 ac[U], xc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) ac[u] = aq[u], xc[u] = xq[u];
#pragma unroll
        for (int u = 0; u < U; ++u) aq[u] = ap[4 * (st + U + u)], xq[u] = xp[4 * (st + U + u)];
#pragma unroll
        for (int u = 0; u < U; ++u) part = mfma16(ac[u], xc[u], part);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) part = mfma16(aq[u], xq[u], part);
      st += U;
    }
    for (; st < steps; ++st) part = mfma16(ap[4 * st], xp[4 * st], part);
    if (mine) acc = part;
  }
  // acc[i]: token t0 + (lane & 15), rank row r0 + 4 (lane >> 4) + i.  Thread (w', ln) finishes
  // element i = w' of lane ln, the four K quarters in a fixed order
  __shared__ float red[4][4][64];
#pragma unroll
  for (int i = 0; i < 4; ++i) red[wv][i][lane] = acc[i];
  __syncthreads();
  const int tok = t0 + (lane & 15);
  if (tok < T) {
    const float v = (red[0][wv][lane] + red[1][wv][lane]) + (red[2][wv][lane] + red[3][wv][lane]);
    tmp[(size_t)tok * GR + r0 + 4 * (lane >> 4) + wv] = v;
  }
}

// tmp is fp32 and the matrix cores take bf16: split each value into three bf16 terms
// (hi + mid + lo carries 24 significant bits, each difference exact in fp32), three MFMAs per step
__device__ __forceinline__ void lora_split3(const float (&v)[8], bf16x8& h, bf16x8& m, bf16x8& l) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint16_t hb = f2bf(v[j]);
    const float r1 = v[j] - bf2f(hb);
    const uint16_t mb = f2bf(r1);
    h[j] = (short)hb;
    m[j] = (short)mb;
    l[j] = (short)f2bf(r1 - bf2f(mb));
  }
}

// grid (ceil(T / 16), ceil(N / 64)), 256 threads: each wave owns one 16-token x 16-column tile
__global__ void __launch_bounds__(256) lora_expand_add_kernel(uint16_t* __restrict__ y, int ldy,
                                                              const float* __restrict__ tmp,
                                                              const uint16_t* __restrict__ B,
                                                              const uint8_t* __restrict__ tile_group,
                                                              const int* __restrict__ tok_slot,
                                                              const int* __restrict__ slot_rank, int T, int N, int GR,
                                                              int R, int S) {
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t0 = blockIdx.x * 16, nt = blockIdx.y * 4 + wv;
  if (nt >= (N >> 4)) return;  // wave-uniform; the kernel has no barrier
  const int n0 = nt * 16;
  const int g = min((int)tile_group[nt], GR / R - 1);
  const int my = lora_lane_slot(tok_slot, t0, T, S, lane);
  int pending = my;
  const int kc = (lane >> 4) * 8;
  const float* tp = tmp + (size_t)min(t0 + (lane & 15), T - 1) * GR + g * R;
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (;;) {
    bool mine = false;
    const int s = __builtin_amdgcn_readfirstlane(lora_next_slot(pending, mine));
    if (s < 0) break;
    const int rank = min(slot_rank[s], R);
    const uint16_t* bp = B + ((size_t)s * N + n0 + (lane & 15)) * R;
    f32x4 part = {0.f, 0.f, 0.f, 0.f};
    for (int k = 0; k < rank; k += 32) {
      // R is a multiple of 16, not of 32: the chunks of a step's upper half may lie past the row
      const bool in = k + kc < R;
      const int ko = in ? k + kc : 0;
      bf16x8 bv = *reinterpret_cast<const bf16x8*>(bp + ko);
      const float4 v0 = *reinterpret_cast<const float4*>(tp + ko);
      const float4 v1 = *reinterpret_cast<const float4*>(tp + ko + 4);
      const float v[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      bf16x8 h, m, l;
      lora_split3(v, h, m, l);
      if (!in) bv = h = m = l = zero;
      part = mfma16(bv, l, part);
      part = mfma16(bv, m, part);
      part = mfma16(bv, h, part);
    }
    if (mine) acc = part;  // a lane's token column belongs to one slot
  }
  // acc[i]: token t0 + (lane & 15), column n0 + 4 (lane >> 4) + i.  Rows without an adapter
  // are not written at all
  if (my < 0) return;
  u32x2* p = reinterpret_cast<u32x2*>(y + (size_t)(t0 + (lane & 15)) * ldy + n0 + 4 * (lane >> 4));
  const u32x2 o = *p;
  u32x2 w;
  w.x = pack2(lo_bf(o.x) + acc[0], hi_bf(o.x) + acc[1]);
  w.y = pack2(lo_bf(o.y) + acc[2], hi_bf(o.y) + acc[3]);
  *p = w;
}

}  // namespace

void launch_lora_shrink(const void* x, int ldx, const void* A, float* tmp, const int* tok_slot,
                        const int* slot_rank, int T, int K, int GR, int R, int S, hipStream_t st) {
  if (T <= 0) return;
  lora_shrink_kernel<<<dim3(cdiv(T, 16), GR / 16), 256, 0, st>>>((const uint16_t*)x, ldx, (const uint16_t*)A, tmp,
                                                                  tok_slot, slot_rank, T, K, GR, R, S);
}

void launch_lora_expand_add(void* y, int ldy, const float* tmp, const void* B, const uint8_t* tile_group,
                            const int* tok_slot, const int* slot_rank, int T, int N, int GR, int R, int S,
                            hipStream_t st) {
  if (T <= 0) return;
  lora_expand_add_kernel<<<dim3(cdiv(T, 16), cdiv(N / 16, 4)), 256, 0, st>>>(
      (uint16_t*)y, ldy, tmp, (const uint16_t*)B, tile_group, tok_slot, slot_rank, T, N, GR, R, S);
}

}  // namespace mlop
