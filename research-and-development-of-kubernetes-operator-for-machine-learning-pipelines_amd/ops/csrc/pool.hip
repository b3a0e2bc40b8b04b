// Embedding pooling (K20) for gfx950: the tail of a step that serves embedding requests.
//
// A step's final-normed hidden states x[T, ldx] (bf16) carry `nseg` pool segments, each the
// chunk [r0, r1) of one embedding sequence, with its slot of the fp32 accumulator acc[S, H]:
//
//   pool_accumulate   mean: acc[slot, c] = (init ? 0 : acc[slot, c]) + x[r0, c] + ... + x[r1-1, c],
//                     fp32, the rows STRICTLY in order.  The work is split over (segment, column
//                     slice) only, never over the rows of a segment: no atomics, no cross-row
//                     reduction, so the sum does not depend on how a prompt was cut into chunks
//                     and equals a sequential fp32 loop on the host bit for bit.  A lane owns 8
//                     columns (one 16-B load per row) and keeps kPoolRows rows in flight: the
//                     loads are independent, the adds behind them dependent.
//                     last: the segment flagged kPoolLast copies row r1 - 1; others do nothing.
//   pool_finish       per finished slot: v = acc[slot, :d] * (1 / count) (mean only), then
//                     optionally v / max(||v||, 1e-12), written fp32 to out[slot, :d].  The sum
//                     of squares is taken in a fixed order (below), so a relaunch repeats it.
//
// Rows of x outside every segment are never read, slots no segment names are never written;
// a segment or slot outside the tensors is skipped, not clamped.  The grids depend on the
// host-known counts only (memory-bound row kernels, cdna_hip_programming.md App. B).
#include "common.h"
#include "launch.h"

namespace mlop {

constexpr int kPoolRows = 16;       // rows in flight per lane (16 x 16 B loads, 64 VGPRs)
constexpr int kFinishThreads = 256;

__global__ void __launch_bounds__(64) pool_accumulate_kernel(float* __restrict__ acc,
                                                            const uint16_t* __restrict__ x, long ldx,
                                                            const int4* __restrict__ seg, int T, int H,
                                                            int S, int lanes) {
  const int4 s = seg[blockIdx.y];  // [r0, r1, slot, flags]: uniform
  const int r0 = s.x, r1 = s.y, slot = s.z, flags = s.w;
  const int vi = blockIdx.x * lanes + threadIdx.x;
  if ((int)threadIdx.x >= lanes || vi >= (H >> 3)) return;
  if (r0 < 0 || r1 > T || r0 >= r1 || slot < 0 || slot >= S) return;
  float* a = acc + (size_t)slot * H + vi * 8;
  const uint16_t* p = x + vi * 8;
  float v[8];
  if (flags & kPoolModeLast) {
    if (!(flags & kPoolLast)) return;
    const u32x4 t = *reinterpret_cast<const u32x4*>(p + (size_t)(r1 - 1) * ldx);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v[2 * j] = lo_bf(t[j]);
      v[2 * j + 1] = hi_bf(t[j]);
    }
  } else {
    if (flags & kPoolInit) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = 0.f;
    } else {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + 4);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[j] = a0[j];
        v[4 + j] = a1[j];
      }
    }
    // Every load of a group is unconditional, so the 16 are issued back to back and waited for
    // once; a load under `if (i < n)` compiles to a branch per row with a full vmcnt(0) wait in
    // front of each, one round trip per row.  The last, short group reads its missing rows from the
    // segment's own last row (in bounds, inside the segment) and only its adds are guarded.
    for (int r = r0; r < r1; r += kPoolRows) {
      const int n = r1 - r;  // rows of this group that count (>= kPoolRows: all)
      u32x4 t[kPoolRows];
#pragma unroll
      for (int i = 0; i < kPoolRows; ++i)
        t[i] = *reinterpret_cast<const u32x4*>(p + (size_t)min(r + i, r1 - 1) * ldx);
#pragma unroll
      for (int i = 0; i < kPoolRows; ++i)
        if (i < n) {  // (guarded, not + 0: -0 + 0 would lose the sign)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            v[2 * j] += lo_bf(t[i][j]);
            v[2 * j + 1] += hi_bf(t[i][j]);
          }
        }
    }
  }
  *reinterpret_cast<f32x4*>(a) = f32x4{v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(a + 4) = f32x4{v[4], v[5], v[6], v[7]};
}

// One workgroup per finished slot.  Order of the sum of squares: lane t adds the squares of its
// elements in index order (vectors t, t + 256, ...; inside a vector columns 0..7), the 64 lanes of
// a wave are combined by wave_sum's fixed butterfly, the 4 wave sums added in wave order.
__global__ void __launch_bounds__(kFinishThreads) pool_finish_kernel(float* __restrict__ out, long ldo,
                                                                    const float* __restrict__ acc,
                                                                    const int4* __restrict__ fin, int H,
                                                                    int S) {
  __shared__ float scratch[kFinishThreads / 64];
  const int4 f = fin[blockIdx.x];  // [slot, count, d, flags]: uniform
  const int slot = f.x, count = f.y, d = f.z, flags = f.w;
  if (slot < 0 || slot >= S || d < 1 || d > H || count < 1) return;  // whole block
  const float inv = (flags & kPoolFinMean) ? 1.f / (float)count : 1.f;
  const float* a = acc + (size_t)slot * H;
  float* o = out + (size_t)slot * ldo;
  float nrm = 1.f;
  if (flags & kPoolFinNormalize) {
    float ss = 0.f;
    for (int vi = threadIdx.x; vi * 8 < d; vi += kFinishThreads) {
      const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + vi * 8);
      const f32x4 a1 = *reinterpret_cast<const f32x4*>(a + vi * 8 + 4);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v = (j < 4 ? a0[j & 3] : a1[j & 3]) * inv;
        if (vi * 8 + j < d) ss += v * v;
      }
    }
    ss = block_sum(ss, scratch);
    nrm = fmaxf(sqrtf(ss), 1e-12f);
  }
  for (int vi = threadIdx.x; vi * 8 < d; vi += kFinishThreads) {
    const f32x4 a0 = *reinterpret_cast<const f32x4*>(a + vi * 8);
    const f32x4 a1 = *reinterpret_cast<const f32x4*>(a + vi * 8 + 4);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float v = (j < 4 ? a0[j & 3] : a1[j & 3]) * inv;
      if (vi * 8 + j < d) o[vi * 8 + j] = (flags & kPoolFinNormalize) ? v / nrm : v;
    }
  }
}

void launch_pool_accumulate(float* acc, const void* x, long ldx, const int* seg, int nseg, int T, int H, int S,
                            hipStream_t st) {
  if (nseg <= 0) return;
  // a slice is 64 lanes x 8 columns; with few segments narrower slices (32, 16 lanes) put more
  // waves on the row walk, which is bound by the latency of its loads.  Columns are independent:
  // the slice width changes no result
  const int nvec = H >> 3;
  int lanes = 64;
  while (lanes > 16 && nseg * cdiv(nvec, lanes) < 512) lanes >>= 1;
  pool_accumulate_kernel<<<dim3(cdiv(nvec, lanes), nseg), 64, 0, st>>>(acc, (const uint16_t*)x, ldx, (const int4*)seg,
                                                                      T, H, S, lanes);
}

void launch_pool_finish(float* out, long ldo, const float* acc, const int* fin, int nfin, int H, int S,
                        hipStream_t st) {
  if (nfin <= 0) return;
  pool_finish_kernel<<<nfin, kFinishThreads, 0, st>>>(out, ldo, acc, (const int4*)fin, H, S);
}

}  // namespace mlop
