// torch.ops.mlop.* registrations for the gfx950 kernels.
//
// Every op validates dtype / contiguity / shape on the host before launching
// (a faulting kernel can reset every GPU of the node), runs on the current
// HIP stream (so it is hipGraph-capturable) and mutates pre-allocated outputs
// (cdna_hip_programming.md Guideline 9; the one scratch tensor, gemm_rope_cache's V staging,
// comes from PyTorch's caching allocator, which serves captures from the graph's pool).
#include <climits>
#include <cstdlib>
#include <string>
#include <torch/library.h>
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>
#include <c10/core/DeviceGuard.h>
#include <cmath>

#include "launch.h"
#include "gemm_plan.h"

namespace {

using at::Tensor;

hipStream_t cur_stream() { return c10::hip::getCurrentHIPStream().stream(); }

void check_bf16(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
void check_i32(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kInt, name, " must be int32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void rmsnorm(Tensor out, Tensor x, Tensor w, double eps) {
  check_bf16(out, "out"); check_bf16(x, "x"); check_bf16(w, "w");
  const int64_t H = x.size(-1);
  TORCH_CHECK(H % 8 == 0 && H <= 65536, "hidden size must be a multiple of 8");
  TORCH_CHECK(w.numel() == H && out.numel() == x.numel(), "rmsnorm shape mismatch");
  c10::DeviceGuard g(x.device());
  mlop::launch_rmsnorm(out.data_ptr(), x.data_ptr(), w.data_ptr(), (float)eps,
                       (int)(x.numel() / H), (int)H, cur_stream());
}

void add_rmsnorm(Tensor out, Tensor residual, Tensor x, Tensor w, double eps) {
  check_bf16(out, "out"); check_bf16(residual, "residual"); check_bf16(x, "x"); check_bf16(w, "w");
  const int64_t H = x.size(-1);
  TORCH_CHECK(H % 8 == 0 && H <= 65536, "hidden size must be a multiple of 8");
  TORCH_CHECK(w.numel() == H && out.numel() == x.numel() && residual.numel() == x.numel(),
              "add_rmsnorm shape mismatch");
  c10::DeviceGuard g(x.device());
  mlop::launch_add_rmsnorm(out.data_ptr(), residual.data_ptr(), x.data_ptr(), w.data_ptr(),
                           (float)eps, (int)(x.numel() / H), (int)H, cur_stream());
}

void rope_cache(Tensor q_out, Tensor k_cache, Tensor v_cache, Tensor qkv, Tensor pos,
                Tensor cos_sin, Tensor slots) {
  check_bf16(q_out, "q_out"); check_bf16(k_cache, "k_cache"); check_bf16(v_cache, "v_cache");
  check_i32(pos, "pos"); check_i32(slots, "slots");
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.stride(-1) == 1,
              "qkv must be bf16 with unit inner stride");
  TORCH_CHECK(cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous(), "cos_sin f32");
  TORCH_CHECK(q_out.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4, "rope_cache ranks");
  const int T = (int)q_out.size(0), Hq = (int)q_out.size(1), D = (int)q_out.size(2);
  const int Hkv = (int)k_cache.size(1), BS = (int)k_cache.size(2);
  TORCH_CHECK(k_cache.size(3) == D && v_cache.sizes() == k_cache.sizes(),
              "cache layouts: k and v [NB,Hkv,BS,D] (token-major)");
  TORCH_CHECK(D % 16 == 0, "head dim must be a multiple of 16");
  TORCH_CHECK(qkv.size(0) == T && qkv.size(-1) >= (Hq + 2 * Hkv) * D, "qkv shape");
  TORCH_CHECK(pos.numel() == T && slots.numel() == T, "pos/slots length");
  TORCH_CHECK(cos_sin.size(1) == D, "cos_sin must be [max_pos, D]");
  c10::DeviceGuard g(qkv.device());
  mlop::launch_rope_cache(q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), qkv.data_ptr(),
                          pos.data_ptr<int>(), cos_sin.data_ptr<float>(), slots.data_ptr<int>(), T,
                          Hq, Hkv, D, (int)qkv.stride(0), BS, cur_stream());
}

void silu_mul(Tensor out, Tensor x, int64_t interleaved) {
  check_bf16(out, "out"); check_bf16(x, "x");
  const int64_t I2 = x.size(-1);
  TORCH_CHECK(I2 % (interleaved ? 32 : 16) == 0, "gate_up width must be a multiple of 16/32");
  const int64_t M = x.numel() / I2;
  TORCH_CHECK(out.numel() == M * (I2 / 2), "silu_mul shape mismatch");
  c10::DeviceGuard g(x.device());
  mlop::launch_silu_mul(out.data_ptr(), x.data_ptr(), (int)M, (int)(I2 / 2), (int)interleaved,
                        cur_stream());
}

// multi-LoRA (lora.hip): tmp[t] = A[tok_slot[t]] . x[t]
// (R = rows per A block, for the rank skip; 16 = never skip) and
// y[t, n] += sum_r tmp[t, g(n) R + r] . B[tok_slot[t], n, r] in place
void lora_shrink(Tensor tmp, Tensor x, Tensor A, Tensor tok_slot, Tensor slot_rank, int64_t R) {
  check_bf16(A, "A"); check_i32(tok_slot, "tok_slot"); check_i32(slot_rank, "slot_rank");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.stride(1) == 1 &&
              x.stride(0) % 8 == 0, "x must be bf16 [T, K] with unit inner stride and 16-byte rows");
  TORCH_CHECK(tmp.is_cuda() && tmp.scalar_type() == at::kFloat && tmp.is_contiguous() && tmp.dim() == 2,
              "tmp must be contiguous fp32 [T, G R]");
  TORCH_CHECK(A.dim() == 3, "A must be [S, G R, K]");
  const int64_t T = x.size(0), K = x.size(1), S = A.size(0), GR = A.size(1);
  TORCH_CHECK(K % 128 == 0 && A.size(2) == K, "lora_shrink: K must be a multiple of 128 and match A");
  TORCH_CHECK(GR % 16 == 0 && tmp.size(0) == T && tmp.size(1) == GR, "lora_shrink: tmp shape");
  TORCH_CHECK(R >= 16 && R % 16 == 0 && GR % R == 0, "lora_shrink: R must be a multiple of 16 dividing G R");
  TORCH_CHECK(tok_slot.numel() == T && slot_rank.numel() == S, "lora_shrink: tok_slot [T], slot_rank [S]");
  c10::DeviceGuard g(x.device());
  mlop::launch_lora_shrink(x.data_ptr(), (int)x.stride(0), A.data_ptr(), tmp.data_ptr<float>(),
                           tok_slot.data_ptr<int>(), slot_rank.data_ptr<int>(), (int)T, (int)K, (int)GR,
                           (int)R, (int)S, cur_stream());
}

void lora_expand_add(Tensor y, Tensor tmp, Tensor B, Tensor tile_group, Tensor tok_slot, Tensor slot_rank) {
  check_bf16(B, "B"); check_i32(tok_slot, "tok_slot"); check_i32(slot_rank, "slot_rank");
  TORCH_CHECK(y.is_cuda() && y.scalar_type() == at::kBFloat16 && y.dim() == 2 && y.stride(1) == 1 &&
              y.stride(0) % 8 == 0, "y must be bf16 [T, N] with unit inner stride and 16-byte rows");
  TORCH_CHECK(tmp.is_cuda() && tmp.scalar_type() == at::kFloat && tmp.is_contiguous() && tmp.dim() == 2,
              "tmp must be contiguous fp32 [T, G R]");
  TORCH_CHECK(tile_group.is_cuda() && tile_group.scalar_type() == at::kByte && tile_group.is_contiguous(),
              "tile_group must be uint8");
  TORCH_CHECK(B.dim() == 3, "B must be [S, N, R]");
  const int64_t T = y.size(0), N = y.size(1), S = B.size(0), R = B.size(2), GR = tmp.size(1);
  TORCH_CHECK(N % 16 == 0 && B.size(1) == N && tile_group.numel() == N / 16, "lora_expand_add: N, tile_group");
  TORCH_CHECK(R % 16 == 0 && R > 0 && GR % R == 0 && GR / R <= 255 && tmp.size(0) == T,
              "lora_expand_add: tmp must be [T, G R] with R = B.size(2) a multiple of 16");
  TORCH_CHECK(tok_slot.numel() == T && slot_rank.numel() == S, "lora_expand_add: tok_slot [T], slot_rank [S]");
  c10::DeviceGuard g(y.device());
  mlop::launch_lora_expand_add(y.data_ptr(), (int)y.stride(0), tmp.data_ptr<float>(), B.data_ptr(),
                               tile_group.data_ptr<uint8_t>(), tok_slot.data_ptr<int>(),
                               slot_rank.data_ptr<int>(), (int)T, (int)N, (int)GR, (int)R, (int)S, cur_stream());
}

// fault injection: a device-side delay of `us` microseconds on the current stream
void device_delay(int64_t us) {
  int dev = 0, khz = 0;
  TORCH_CHECK(hipGetDevice(&dev) == hipSuccess, "device_delay: hipGetDevice");
  TORCH_CHECK(hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0,
              "device_delay: wall clock rate");
  TORCH_CHECK(us >= 0 && us <= 10000000, "device_delay: 0..10 s");
  mlop::launch_device_delay((long long)us * khz / 1000, cur_stream());
}

void embedding(Tensor out, Tensor table, Tensor ids, int64_t vocab_start) {
  check_bf16(out, "out"); check_bf16(table, "table");
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kLong && ids.is_contiguous(), "ids int64");
  const int64_t H = table.size(1);
  TORCH_CHECK(H % 8 == 0 && out.size(-1) == H && out.numel() == ids.numel() * H, "embedding shape");
  c10::DeviceGuard g(table.device());
  mlop::launch_embedding(out.data_ptr(), table.data_ptr(), ids.data_ptr<int64_t>(),
                         (int)ids.numel(), (int)H, vocab_start, vocab_start + table.size(0),
                         cur_stream());
}

void flash_prefill(Tensor out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables,
                   Tensor ptile_seq, Tensor ptile_q0, Tensor q_start, Tensor q_len, Tensor ctx_len,
                   double scale, int64_t window) {
  TORCH_CHECK(window >= 0 && window < (1 << 30), "window must be >= 0 (0: no sliding window)");
  check_bf16(out, "out"); check_bf16(q, "q"); check_bf16(k_cache, "k_cache");
  check_bf16(v_cache, "v_cache");
  check_i32(block_tables, "block_tables"); check_i32(ptile_seq, "ptile_seq");
  check_i32(ptile_q0, "ptile_q0"); check_i32(q_start, "q_start"); check_i32(q_len, "q_len");
  check_i32(ctx_len, "ctx_len");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 128, "q must be [T, Hq, 128]");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) == 16 && k_cache.size(3) == 128,
              "k_cache must be [NB, Hkv, 16, 128]");
  TORCH_CHECK(v_cache.sizes() == at::IntArrayRef({k_cache.size(0), k_cache.size(1), 16, 128}),
              "v_cache must be [NB, Hkv, 16, 128] (token-major, as k_cache)");
  const int Hq = (int)q.size(1), Hkv = (int)k_cache.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "Hq % Hkv");
  const int G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8, "flash prefill: GQA group must be 1, 2, 4 or 8");
  TORCH_CHECK(out.sizes() == q.sizes(), "out shape");
  TORCH_CHECK(ptile_seq.numel() == ptile_q0.numel(), "tile arrays");
  // the stream kernel's O stores range-check at 2 GB (masked rows are stored past it)
  TORCH_CHECK(!mlop::flash_stream(-1) || out.numel() * 2 < (int64_t)0x7fffff00, "flash_stream: output >= 2 GB");
  TORCH_CHECK(q_start.numel() == q_len.numel() && q_len.numel() == ctx_len.numel() &&
                  block_tables.size(0) >= q_len.numel(),
              "per-sequence arrays");
  c10::DeviceGuard g(q.device());
  mlop::launch_flash_prefill(out.data_ptr(), q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
                             block_tables.data_ptr<int>(), (int)block_tables.stride(0),
                             ptile_seq.data_ptr<int>(), ptile_q0.data_ptr<int>(),
                             q_start.data_ptr<int>(), q_len.data_ptr<int>(), ctx_len.data_ptr<int>(),
                             (int)ptile_seq.numel(), Hq, Hkv, (float)(scale * 1.4426950408889634),
                             (int)k_cache.size(0), (int)window, cur_stream());
}

// Largest (tile, kv head) pair count that takes the in-launch split-KV combine: no cap (a cap of
// 32 pairs measured the same at 16 x 32k contexts, BASELINE.md long context); settable in-process
// for the tests (attn_fused_max_pairs(); -1 reads it back).
static int g_attn_fused_pairs = 1 << 30;
static int attn_fused_pairs_cap() { return g_attn_fused_pairs; }
int64_t attn_fused_max_pairs(int64_t n) {
  const int prev = attn_fused_pairs_cap();
  if (n >= 0) g_attn_fused_pairs = (int)n;
  return prev;
}

// The arguments the decode attention ops share, whatever the KV format (k_cache: checked by the
// caller as [NB, Hkv, 16, 128] of its format), and what both launches derive from them: the
// partial buffers (nullptr with one partition) and the ticket buffer of the in-launch split-KV
// combine (nullptr: the combine runs as a second launch).
struct DecodeAttention {
  int Hq, Hkv, num_tiles;
  float* part_o;
  float* part_ml;
  int* sem;
};
static DecodeAttention check_decode_attention(const Tensor& out, const Tensor& part_o, const Tensor& part_ml,
                                              const Tensor& part_sem, const Tensor& q, const Tensor& k_cache,
                                              const Tensor& block_tables, const Tensor& tile_seq, const Tensor& tile_q0,
                                              const Tensor& q_start, const Tensor& q_len, const Tensor& ctx_len,
                                              int64_t part_tokens, int64_t nparts) {
  check_bf16(out, "out"); check_bf16(q, "q");
  check_i32(block_tables, "block_tables"); check_i32(tile_seq, "tile_seq");
  check_i32(tile_q0, "tile_q0"); check_i32(q_start, "q_start"); check_i32(q_len, "q_len");
  check_i32(ctx_len, "ctx_len");
  TORCH_CHECK(q.dim() == 3 && q.size(2) == 128, "q must be [T, Hq, 128]");
  const int Hq = (int)q.size(1), Hkv = (int)k_cache.size(1);
  TORCH_CHECK(Hq % Hkv == 0, "Hq % Hkv");
  const int G = Hq / Hkv;
  TORCH_CHECK(G == 1 || G == 2 || G == 4 || G == 8 || G == 16, "GQA group must divide 16");
  TORCH_CHECK(out.sizes() == q.sizes(), "out shape");
  TORCH_CHECK(tile_seq.numel() == tile_q0.numel(), "tile arrays");
  // (the kernel reads bt[min(.., stride - 1)] ahead of the lengths)
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(1) >= 1, "block_tables must be [rows, pages]");
  TORCH_CHECK(q_start.numel() == q_len.numel() && q_len.numel() == ctx_len.numel() &&
                  block_tables.size(0) >= q_len.numel(),
              "per-sequence arrays");
  TORCH_CHECK(part_tokens % 32 == 0 && part_tokens > 0 && nparts >= 1, "partition size");
  const int64_t num_tiles = tile_seq.numel();
  DecodeAttention a{Hq, Hkv, (int)num_tiles, nullptr, nullptr, nullptr};
  if (nparts > 1) {
    TORCH_CHECK(part_o.scalar_type() == at::kFloat && part_ml.scalar_type() == at::kFloat,
                "partials f32");
    TORCH_CHECK(part_o.numel() >= num_tiles * Hkv * nparts * 16 * 128 &&
                    part_ml.numel() >= num_tiles * Hkv * nparts * 16 * 2,
                "partial workspace too small");
    a.part_o = part_o.data_ptr<float>();
    a.part_ml = part_ml.data_ptr<float>();
  }
  // part_sem: zero-initialised int32 tickets, one per (tile, kv head), re-armed by the
  // kernel; empty -> the split-KV combine runs as a second launch
  // Round 3 capped it at 32 pairs: every partition's agent release fence outweighed the
  // saved launch above that (batch 8: 1800 -> 1783 tok/s, scripts/run52.sh).  With the
  // partials stored sc1 and no producer fence it wins at every batch measured (batch 8 / 16
  // / 64: +0.7 / +0.7 / +0.2 %, scripts/history/r4_fusedc.sh), so the cap is off by default.
  if (nparts > 1 && part_sem.numel() > 0 && num_tiles * Hkv <= attn_fused_pairs_cap()) {
    check_i32(part_sem, "part_sem");
    TORCH_CHECK(part_sem.numel() >= num_tiles * Hkv, "part_sem too small");
    a.sem = part_sem.data_ptr<int>();
  }
  return a;
}

void paged_attention(Tensor out, Tensor part_o, Tensor part_ml, Tensor part_sem, Tensor q, Tensor k_cache,
                     Tensor v_cache, Tensor block_tables, Tensor tile_seq, Tensor tile_q0,
                     Tensor q_start, Tensor q_len, Tensor ctx_len, double scale,
                     int64_t part_tokens, int64_t nparts, int64_t window) {
  TORCH_CHECK(window >= 0 && window < (1 << 30), "window must be >= 0 (0: no sliding window)");
  check_bf16(k_cache, "k_cache"); check_bf16(v_cache, "v_cache");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(2) == 16 && k_cache.size(3) == 128,
              "k_cache must be [NB, Hkv, 16, 128]");
  TORCH_CHECK(v_cache.sizes() == at::IntArrayRef({k_cache.size(0), k_cache.size(1), 16, 128}),
              "v_cache must be [NB, Hkv, 16, 128] (token-major, as k_cache)");
  const DecodeAttention a = check_decode_attention(out, part_o, part_ml, part_sem, q, k_cache, block_tables, tile_seq,
                                                   tile_q0, q_start, q_len, ctx_len, part_tokens, nparts);
  c10::DeviceGuard g(q.device());
  const float scale_log2 = (float)(scale * 1.4426950408889634);
  mlop::launch_paged_attention(
      out.data_ptr(), a.part_o, a.part_ml, q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      block_tables.data_ptr<int>(), (int)block_tables.stride(0), tile_seq.data_ptr<int>(),
      tile_q0.data_ptr<int>(), q_start.data_ptr<int>(), q_len.data_ptr<int>(), ctx_len.data_ptr<int>(),
      a.num_tiles, a.Hq, a.Hkv, scale_log2, (int)part_tokens, (int)nparts, (int)k_cache.size(0), a.sem,
      (int)window, cur_stream());
}

// ---- fp8 KV cache (kv_fp8.hip, attention.hip's KvFp8): e4m3fn pages + one scale byte per row
void check_fp8_cache(const Tensor& c, const Tensor& sc, const char* name) {
  TORCH_CHECK(c.is_cuda() && c.scalar_type() == at::kFloat8_e4m3fn && c.is_contiguous(), name,
              " must be a contiguous float8_e4m3fn GPU tensor");
  TORCH_CHECK(c.dim() == 4 && c.size(2) == 16 && c.size(3) == 128, name, " must be [NB, Hkv, 16, 128]");
  TORCH_CHECK(sc.is_cuda() && sc.scalar_type() == at::kByte && sc.is_contiguous(), name,
              " scales must be a contiguous uint8 GPU tensor");
  TORCH_CHECK(sc.sizes() == at::IntArrayRef({c.size(0), c.size(1), 16}), name, " scales must be [NB, Hkv, 16]");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(c.data_ptr()) & 15) == 0 &&
                  (reinterpret_cast<uintptr_t>(sc.data_ptr()) & 15) == 0,
              name, " and its scales must be 16-B aligned");
}

void rope_cache_fp8(Tensor q_out, Tensor k_cache, Tensor v_cache, Tensor k_scale, Tensor v_scale, Tensor qkv,
                    Tensor pos, Tensor cos_sin, Tensor slots) {
  check_bf16(q_out, "q_out");
  check_fp8_cache(k_cache, k_scale, "k_cache"); check_fp8_cache(v_cache, v_scale, "v_cache");
  check_i32(pos, "pos"); check_i32(slots, "slots");
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.stride(-1) == 1 && qkv.dim() == 2,
              "qkv must be 2-d bf16 with unit inner stride");
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous(), "cos_sin f32");
  TORCH_CHECK(q_out.dim() == 3 && q_out.size(2) == 128, "q_out must be [T, Hq, 128]");
  const int T = (int)q_out.size(0), Hq = (int)q_out.size(1);
  const int Hkv = (int)k_cache.size(1);
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), "k and v caches differ in shape");
  TORCH_CHECK(qkv.size(0) == T && qkv.size(-1) >= (Hq + 2 * Hkv) * 128 && qkv.stride(0) % 8 == 0 &&
                  (reinterpret_cast<uintptr_t>(qkv.data_ptr()) & 15) == 0,
              "qkv shape / alignment");
  TORCH_CHECK(pos.numel() == T && slots.numel() == T, "pos/slots length");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin must be [max_pos, 128]");
  c10::DeviceGuard g(qkv.device());
  mlop::launch_rope_cache_fp8(q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                              v_scale.data_ptr(), qkv.data_ptr(), pos.data_ptr<int>(),
                              cos_sin.data_ptr<float>(), slots.data_ptr<int>(), T, Hq, Hkv,
                              (int)qkv.stride(0), 16, cur_stream());
}

// ---- per-head QK-norm writers (rope_cache_qkn.hip): rope_cache / rope_cache_fp8 with an RMSNorm
// of every q and k head before the rotation; head_dim 128 only
struct QknArgs {
  int T, Hq, Hkv;
};
static QknArgs check_qkn(const Tensor& q_out, const Tensor& k_cache, const Tensor& v_cache, const Tensor& qkv,
                         const Tensor& pos, const Tensor& cos_sin, const Tensor& slots, const Tensor& q_w,
                         const Tensor& k_w, double eps) {
  check_bf16(q_out, "q_out");
  check_i32(pos, "pos"); check_i32(slots, "slots");
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.stride(-1) == 1 && qkv.dim() == 2,
              "qkv must be 2-d bf16 with unit inner stride");
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous(), "cos_sin f32");
  TORCH_CHECK(q_out.dim() == 3 && q_out.size(2) == 128, "q_out must be [T, Hq, 128] (QK-norm: head_dim 128 only)");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.size(3) == 128 && v_cache.sizes() == k_cache.sizes(),
              "cache layouts: k and v [NB, Hkv, BS, 128] (token-major)");
  const int T = (int)q_out.size(0), Hq = (int)q_out.size(1), Hkv = (int)k_cache.size(1);
  TORCH_CHECK(qkv.size(0) == T && qkv.size(-1) >= (Hq + 2 * Hkv) * 128 && qkv.stride(0) % 8 == 0 &&
                  (reinterpret_cast<uintptr_t>(qkv.data_ptr()) & 15) == 0,
              "qkv shape / alignment");
  TORCH_CHECK(pos.numel() == T && slots.numel() == T, "pos/slots length");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == 128, "cos_sin must be [max_pos, 128]");
  for (const Tensor* w : {&q_w, &k_w}) {
    check_bf16(*w, "q_norm / k_norm");
    TORCH_CHECK(w->dim() == 1 && w->size(0) == 128 && w->is_contiguous() &&
                    (reinterpret_cast<uintptr_t>(w->data_ptr()) & 15) == 0,
                "q_norm / k_norm must be contiguous 16-B aligned bf16 [128]");
  }
  TORCH_CHECK(eps >= 0, "eps must be >= 0");
  return {T, Hq, Hkv};
}

void rope_cache_qkn(Tensor q_out, Tensor k_cache, Tensor v_cache, Tensor qkv, Tensor pos, Tensor cos_sin,
                    Tensor slots, Tensor q_w, Tensor k_w, double eps) {
  check_bf16(k_cache, "k_cache"); check_bf16(v_cache, "v_cache");
  const QknArgs a = check_qkn(q_out, k_cache, v_cache, qkv, pos, cos_sin, slots, q_w, k_w, eps);
  c10::DeviceGuard g(qkv.device());
  mlop::launch_rope_cache_qkn(q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), qkv.data_ptr(),
                              pos.data_ptr<int>(), cos_sin.data_ptr<float>(), slots.data_ptr<int>(), a.T, a.Hq,
                              a.Hkv, (int)qkv.stride(0), (int)k_cache.size(2), (const uint16_t*)q_w.data_ptr(),
                              (const uint16_t*)k_w.data_ptr(), (float)eps, cur_stream());
}

void rope_cache_qkn_fp8(Tensor q_out, Tensor k_cache, Tensor v_cache, Tensor k_scale, Tensor v_scale, Tensor qkv,
                        Tensor pos, Tensor cos_sin, Tensor slots, Tensor q_w, Tensor k_w, double eps) {
  check_fp8_cache(k_cache, k_scale, "k_cache"); check_fp8_cache(v_cache, v_scale, "v_cache");
  const QknArgs a = check_qkn(q_out, k_cache, v_cache, qkv, pos, cos_sin, slots, q_w, k_w, eps);
  c10::DeviceGuard g(qkv.device());
  mlop::launch_rope_cache_qkn_fp8(q_out.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), k_scale.data_ptr(),
                                  v_scale.data_ptr(), qkv.data_ptr(), pos.data_ptr<int>(),
                                  cos_sin.data_ptr<float>(), slots.data_ptr<int>(), a.T, a.Hq, a.Hkv,
                                  (int)qkv.stride(0), 16, (const uint16_t*)q_w.data_ptr(),
                                  (const uint16_t*)k_w.data_ptr(), (float)eps, cur_stream());
}

void paged_attention_fp8(Tensor out, Tensor part_o, Tensor part_ml, Tensor part_sem, Tensor q, Tensor k_cache,
                         Tensor v_cache, Tensor k_scale, Tensor v_scale, Tensor block_tables, Tensor tile_seq,
                         Tensor tile_q0, Tensor q_start, Tensor q_len, Tensor ctx_len, double scale,
                         int64_t part_tokens, int64_t nparts) {
  check_fp8_cache(k_cache, k_scale, "k_cache"); check_fp8_cache(v_cache, v_scale, "v_cache");
  TORCH_CHECK(v_cache.sizes() == k_cache.sizes(), "k and v caches differ in shape");
  const DecodeAttention a = check_decode_attention(out, part_o, part_ml, part_sem, q, k_cache, block_tables, tile_seq,
                                                   tile_q0, q_start, q_len, ctx_len, part_tokens, nparts);
  c10::DeviceGuard g(q.device());
  const float scale_log2 = (float)(scale * 1.4426950408889634);
  mlop::launch_paged_attention_fp8(
      out.data_ptr(), a.part_o, a.part_ml, q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(),
      k_scale.data_ptr(), v_scale.data_ptr(), block_tables.data_ptr<int>(), (int)block_tables.stride(0),
      tile_seq.data_ptr<int>(), tile_q0.data_ptr<int>(), q_start.data_ptr<int>(), q_len.data_ptr<int>(),
      ctx_len.data_ptr<int>(), a.num_tiles, a.Hq, a.Hkv, scale_log2, (int)part_tokens, (int)nparts,
      (int)k_cache.size(0), a.sem, cur_stream());
}

// ---- lazily backed KV arenas (vmm.hip)
bool vmm_supported(int64_t device) { return mlop::vmm_supported((int)device); }
int64_t vmm_granularity(int64_t device) { return mlop::vmm_granularity((int)device); }

// flat uint8 tensor over a reserved (unbacked) device range; its storage owns the arena
Tensor vmm_arena(int64_t bytes, int64_t device) {
  void* base = nullptr;
  long reserved = 0;
  std::shared_ptr<void> owner = mlop::vmm_reserve((long)bytes, (int)device, &base, &reserved);
  TORCH_CHECK(owner != nullptr, "hipMemAddressReserve failed");
  const at::Device dev(at::kCUDA, (int)device);
  // target_device: the range is not backed yet, so the pointer's device cannot be queried
  return at::for_blob(base, {(int64_t)reserved})
      .deleter([owner, base](void*) mutable {
        mlop::vmm_forget(base);
        owner.reset();
      })
      .options(at::TensorOptions().dtype(at::kByte).device(dev))
      .target_device(dev)
      .make_tensor();
}

bool vmm_map_chunks(Tensor flat, int64_t region_stride, int64_t n_regions, int64_t chunk_bytes, int64_t first,
                    int64_t count, bool async) {
  return mlop::vmm_map_chunks(flat.data_ptr(), (long)region_stride, (int)n_regions, (long)chunk_bytes,
                              (long)first, (long)count, async);
}
int64_t vmm_chunks_ready(Tensor flat) { return mlop::vmm_chunks_ready(flat.data_ptr()); }
int64_t vmm_error(Tensor flat) { return mlop::vmm_error(flat.data_ptr()); }

// the int knobs: "name(int set=-1) -> int", set >= 0 changes the value, returns the current one
template <int (*F)(int)>
int64_t knob(int64_t set) { return F((int)set); }

void gemm_dense_plan(int64_t variant, int64_t bm, int64_t bn, int64_t splits, int64_t stages) {
  mlop::gemm_dense_plan((int)variant, (int)bm, (int)bn, (int)splits, (int)stages);
}
void gemm_grouped_plan(int64_t bm, int64_t bn, int64_t stages, int64_t splits) {
  mlop::gemm_grouped_plan((int)bm, (int)bn, (int)stages, (int)splits);
}
bool gemm_sk_reserve() { return mlop::gemm_sk_reserve(); }

// ---- queries: views of the planner's route for the current device and knobs (gemm_plan.h) ----
int64_t gemm_sk_workgroups(int64_t M, int64_t N, int64_t K) {
  return mlop::gemm_sk_workgroups(mlop::gemm_live_env(), (int)M, (int)N, (int)K);
}
int64_t gemm_workspace(int64_t M, int64_t N, int64_t K, int64_t epi) {
  // epi 2 = GEMM + add + RMSNorm: the split-K slabs of the plain plan
  return mlop::gemm_workspace_floats(mlop::gemm_live_env(), (int)M, (int)N, (int)K, epi == 2 ? 0 : (int)epi);
}
bool gemm_rope_supported(int64_t M, int64_t N, int64_t K) {
  return mlop::gemm_rope_supported(mlop::gemm_live_env(), (int)M, (int)N, (int)K);
}
bool w4_chain_ok(int64_t M, int64_t N, int64_t K) { return mlop::w4_chain_ok(mlop::gemm_live_env(), (int)M, (int)N, (int)K); }
bool mid_chain_ok(int64_t M, int64_t N, int64_t K, int64_t epi) {
  return mlop::mid_chain_ok(mlop::gemm_live_env(), (int)M, (int)N, (int)K, (int)epi);
}
bool gemv_chain_supported(int64_t M, int64_t N, int64_t K, int64_t epi) {
  return mlop::decode_chain_takes(mlop::gemm_live_env(), (int)M, (int)N, (int)K, (int)epi);
}
bool chain_ok(int64_t M, int64_t N, int64_t K, int64_t epi) {
  return mlop::chain_ok(mlop::gemm_live_env(), (int)M, (int)N, (int)K, (int)epi);
}
int64_t decode_chain_max_m() { return mlop::decode_chain_max_m(mlop::gemm_live_env()); }

// The route of one call as a flat int list, in gemm_plan.h's Route field order: family (0 refused, 1
// GEMV, 2 weight-streaming, 3 LDS-DMA tile, 4 ping-pong, 5 four-wave, 6 four-wave half height), tile
// (index into gemm_tile_configs, -1: none), BM, BN, WM, WN, stages, setprio, splits, k_chunk, m_tiles,
// sk_d, sk_wgs, finish (0 none, 1 split-K reduce, 2 split-K add + RMSNorm, 3 RoPE-slab reduce, 4
// RMSNorm), ws_src (0 none, 1 the caller's workspace, 2 the stream-K scratch), ws_floats.
// op: 0 plain, 1 SiLU-mul, 2 GEMM + add + RMSNorm, 3 QKV + RoPE, 4 chain res_ss, 8 / 9 / 11 chain
// row-scaled plain / SiLU-mul / RoPE, 16 / 17 grouped plain / SiLU-mul.
std::vector<int64_t> route_list(const mlop::PlanEnv& env, int64_t M, int64_t N, int64_t K, int64_t op,
                                int64_t n_groups, int64_t rows_per_group) {
  mlop::GemmCall c;
  c.op = (int)op, c.M = (int)M, c.N = (int)N, c.K = (int)K;
  c.n_groups = (int)n_groups, c.rows_per_group = (int)rows_per_group;
  long f[mlop::kRouteFields];
  mlop::gemm_route_fields(mlop::gemm_route(env, c), f);
  return std::vector<int64_t>(f, f + mlop::kRouteFields);
}
std::vector<int64_t> gemm_route(int64_t M, int64_t N, int64_t K, int64_t op, int64_t n_groups, int64_t rows_per_group) {
  return route_list(mlop::gemm_live_env(), M, N, K, op, n_groups, rows_per_group);
}
// the same with the two device facts given: cus CUs, sk = the stream-K scratch reserved
std::vector<int64_t> gemm_route_env(int64_t M, int64_t N, int64_t K, int64_t op, int64_t cus, bool sk,
                                    int64_t n_groups, int64_t rows_per_group) {
  mlop::PlanEnv env = mlop::gemm_knobs();
  env.cus = (int)cus, env.sk = sk;
  return route_list(env, M, N, K, op, n_groups, rows_per_group);
}
// the tile table, 7 ints per entry: BM, BN, WM, WN, stages, setprio, rope
std::vector<int64_t> gemm_tile_configs() {
  std::vector<int64_t> v;
  for (const mlop::TileCfg& t : mlop::kGemmTiles) v.insert(v.end(), {t.BM, t.BN, t.WM, t.WN, t.stages, t.setprio, t.rope});
  return v;
}

// a: bf16 [M, K] activations, unit inner stride, 16-B aligned rows
void check_a(const Tensor& a) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16 && a.dim() == 2 && a.stride(1) == 1 &&
                  a.stride(0) % 8 == 0, "a must be bf16 [M, K], 16-B aligned rows");
}

// the QKV + RoPE + paged-cache argument block of a [M, K] x w [N, K] projection
mlop::RopeEpi rope_args(const Tensor& q_out, const Tensor& k_cache, const Tensor& v_cache, const Tensor& a,
                        const Tensor& w, const Tensor& pos, const Tensor& cos_sin, const Tensor& slots) {
  check_a(a);
  check_bf16(w, "w"); check_bf16(q_out, "q_out"); check_bf16(k_cache, "k_cache");
  check_bf16(v_cache, "v_cache"); check_i32(pos, "pos"); check_i32(slots, "slots");
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous(),
              "cos_sin f32");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K && K % 64 == 0, "w [N, K], K % 64");
  TORCH_CHECK(q_out.dim() == 3 && k_cache.dim() == 4 && v_cache.dim() == 4, "ranks");
  const int64_t Hq = q_out.size(1), D = q_out.size(2), Hkv = k_cache.size(1), BS = k_cache.size(2);
  TORCH_CHECK(D == 128 && k_cache.size(3) == D && v_cache.sizes() == k_cache.sizes(),
              "head_dim 128; k and v [NB,Hkv,BS,D]");
  TORCH_CHECK(N == (Hq + 2 * Hkv) * D && q_out.size(0) == M, "qkv width / q_out rows");
  TORCH_CHECK(pos.numel() == M && slots.numel() == M, "pos/slots length");
  TORCH_CHECK(cos_sin.dim() == 2 && cos_sin.size(1) == D, "cos_sin [max_pos, D]");
  return mlop::RopeEpi{(uint16_t*)q_out.data_ptr(), (uint16_t*)k_cache.data_ptr(),
                       (uint16_t*)v_cache.data_ptr(), pos.data_ptr<int>(), cos_sin.data_ptr<float>(),
                       slots.data_ptr<int>(), (int)Hq, (int)Hkv, (int)BS};
}

// out[M, N or N/2] = epi(a[M, K] . w[N, K]^T)
void gemm(Tensor out, Tensor a, Tensor w, Tensor ws, int64_t epi) {
  TORCH_CHECK(a.is_cuda() && a.scalar_type() == at::kBFloat16 && a.dim() == 2 && a.stride(1) == 1,
              "a must be bf16 [M, K] with unit inner stride");
  check_bf16(w, "w");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.dim() == 2 &&
                  out.stride(1) == 1, "out must be bf16 [M, N]");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K, "w must be [N, K]");
  TORCH_CHECK(K % 64 == 0, "K must be a multiple of 64");
  TORCH_CHECK(N % 8 == 0 && a.stride(0) % 8 == 0 && out.stride(0) % 8 == 0, "16-B aligned rows");
  TORCH_CHECK(epi == 0 || epi == 1, "epi");
  TORCH_CHECK(epi == 0 || N % 32 == 0, "silu_mul epilogue needs N % 32 == 0");
  TORCH_CHECK(out.size(0) == M && out.size(1) == (epi == 0 ? N : N / 2), "out shape");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(a.data_ptr()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(out.data_ptr()) % 16 == 0, "16-B aligned data");
  float* wsp = nullptr;
  int64_t wsn = 0;
  if (ws.defined() && ws.numel() > 0) {
    TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == at::kFloat, "ws f32");
    wsp = ws.data_ptr<float>();
    wsn = ws.numel();
  }
  c10::DeviceGuard g(a.device());
  mlop::launch_gemm(a.data_ptr(), (int)a.stride(0), w.data_ptr(), (int)K, out.data_ptr(),
                    (int)out.stride(0), wsp, wsn, (int)M, (int)N, (int)K, (int)epi, cur_stream());
}

// QKV projection with RoPE + paged-cache stores in the GEMM epilogue; false = this M
// does not take the fused tiling (caller runs gemm + rope_cache)
bool gemm_rope_cache(Tensor q_out, Tensor k_cache, Tensor v_cache, Tensor a, Tensor w, Tensor pos,
                     Tensor cos_sin, Tensor slots) {
  const mlop::RopeEpi re = rope_args(q_out, k_cache, v_cache, a, w, pos, cos_sin, slots);
  c10::DeviceGuard g(a.device());
  return mlop::launch_gemm_rope(a.data_ptr(), (int)a.stride(0), w.data_ptr(), (int)a.size(0), (int)w.size(0),
                                (int)a.size(1), re, cur_stream());
}

// ---- norm chain (TP=1 decoder, unit norm weights): launch_gemm_chain runs each GEMM on the form
// the planner names for its row count (decode GEMV / weight-streaming, mid, four-wave) ----
// ss (f32, M * (H / 128 + 1)) = [M, H / 128] per-row, per-128-column partial sums of squares of
// the residual, then the [M] row totals
static void check_ss(const Tensor& ss, int64_t M, int64_t H, const char* name) {
  TORCH_CHECK(ss.is_cuda() && ss.scalar_type() == at::kFloat && ss.is_contiguous() &&
                  ss.numel() == M * (H / 128 + 1), name, " must be f32 [M * (H / 128 + 1)] contiguous");
}

// residual [M, N] += a . w^T in place, ss_out <- the new residual's sums of squares; false = the
// shape runs on no form of the chain
bool gemm_res_ss(Tensor residual, Tensor a, Tensor w, Tensor ss_out) {
  check_a(a);
  check_bf16(w, "w"); check_bf16(residual, "residual");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K, "w [N, K]");
  TORCH_CHECK(residual.dim() == 2 && residual.size(0) == M && residual.size(1) == N && residual.stride(1) == 1 &&
                  residual.stride(0) % 8 == 0, "residual [M, N]");
  TORCH_CHECK(N % 128 == 0, "N % 128");
  check_ss(ss_out, M, N, "ss");
  c10::DeviceGuard g(a.device());
  return mlop::launch_gemm_chain(mlop::OP_CHAIN_RES_SS, a.data_ptr(), (int)a.stride(0), w.data_ptr(),
                                 residual.data_ptr(), (int)residual.stride(0), (int)M, (int)N, (int)K,
                                 mlop::RopeEpi{}, ss_out.data_ptr<float>(), 0.f, cur_stream());
}

// out = epi(diag(rsqrt(ss / K + eps)) . a . w^T): a is the un-normalised residual, ss_in its
// sums of squares (gemm_res_ss), w the consumer weight with the norm weight folded in
bool gemm_rs(Tensor out, Tensor a, Tensor w, Tensor ss_in, double eps, int64_t epi) {
  check_a(a);
  check_bf16(w, "w"); check_bf16(out, "out");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K, "w [N, K]");
  TORCH_CHECK(epi == 0 || epi == 1, "epi");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == (epi == 0 ? N : N / 2) && out.stride(1) == 1 &&
                  out.stride(0) % 8 == 0, "out [M, N or N/2]");
  TORCH_CHECK(K % 128 == 0, "K % 128");
  check_ss(ss_in, M, K, "ss");
  c10::DeviceGuard g(a.device());
  return mlop::launch_gemm_chain(mlop::OP_CHAIN_RS | (int)epi, a.data_ptr(), (int)a.stride(0), w.data_ptr(),
                                 out.data_ptr(), (int)out.stride(0), (int)M, (int)N, (int)K, mlop::RopeEpi{},
                                 ss_in.data_ptr<float>(), (float)eps, cur_stream());
}

// QKV projection of the norm chain: rows scaled as gemm_rs, then RoPE + paged K / staged V
bool gemm_rs_rope(Tensor q_out, Tensor k_cache, Tensor v_cache, Tensor a, Tensor w, Tensor pos, Tensor cos_sin,
                  Tensor slots, Tensor ss_in, double eps) {
  const mlop::RopeEpi re = rope_args(q_out, k_cache, v_cache, a, w, pos, cos_sin, slots);
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(K % 128 == 0, "K % 128");
  check_ss(ss_in, M, K, "ss");
  c10::DeviceGuard g(a.device());
  return mlop::launch_gemm_chain(mlop::OP_CHAIN_RS_ROPE, a.data_ptr(), (int)a.stride(0), w.data_ptr(), nullptr, 0,
                                 (int)M, (int)N, (int)K, re, ss_in.data_ptr<float>(), (float)eps, cur_stream());
}

// out = rmsnorm(residual += a . w^T) * norm_w through the split-K path; false = not taken
bool gemm_add_rmsnorm(Tensor out, Tensor residual, Tensor a, Tensor w, Tensor norm_w, Tensor ws,
                      double eps) {
  check_a(a);
  check_bf16(w, "w"); check_bf16(out, "out"); check_bf16(residual, "residual");
  check_bf16(norm_w, "norm_w");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K && K % 64 == 0 && N % 8 == 0, "w [N, K], K % 64");
  TORCH_CHECK(out.numel() == M * N && residual.numel() == M * N && norm_w.numel() == N, "shapes");
  TORCH_CHECK(ws.is_cuda() && ws.scalar_type() == at::kFloat, "ws f32");
  c10::DeviceGuard g(a.device());
  return mlop::launch_gemm_add_rmsnorm(a.data_ptr(), (int)a.stride(0), w.data_ptr(), out.data_ptr(),
                                       residual.data_ptr(), norm_w.data_ptr(), (float)eps,
                                       ws.data_ptr<float>(), ws.numel(), (int)M, (int)N, (int)K,
                                       cur_stream());
}

// Decode projection with the residual add + RMSNorm feeding it fused in as a prologue
// (gemv.hip NORM, M <= 4): res_out = bf16(res_in + y); out = epi(rmsnorm(res_out) * norm_w @ w^T).
// weight-streaming MFMA GEMM (gemm_ws.hip), plain / SiLU-mul / residual-add forms, optionally
// with the row-scale prologue; false = shape not taken
bool gemm_ws(Tensor out, Tensor a, Tensor w, int64_t epi, bool rs, double eps) {
  check_a(a);
  check_bf16(w, "w"); check_bf16(out, "out");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.dim() == 2 && w.size(1) == K && w.stride(0) == K, "w [N, K] contiguous");
  TORCH_CHECK(epi == 0 || epi == 1 || epi == 5, "epi 0 / 1 / 5");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == M && out.size(1) == (epi == 1 ? N / 2 : N) && out.stride(1) == 1,
              "out [M, N or N/2]");
  TORCH_CHECK(!(rs && epi == 5), "residual form has no row scale");
  if (!mlop::ws_takes(mlop::gemm_live_env(), (int)M, (int)N, (int)K, (int)epi)) return false;
  c10::DeviceGuard g(a.device());
  mlop::launch_ws(a.data_ptr(), (int)a.stride(0), w.data_ptr(), (int)K, out.data_ptr(), (int)out.stride(0), (int)M,
                  (int)N, (int)K, (int)epi, rs, mlop::RopeEpi{}, (float)eps, cur_stream());
  return true;
}

void gemm_ws_plan(int64_t rb, int64_t u, int64_t nt) { mlop::gemm_ws_plan((int)rb, (int)u, (int)nt); }

// grouped (MoE): rows of a sorted by group, offsets [G+1]; w [G, N, K]
void grouped_gemm(Tensor out, Tensor a, Tensor w, Tensor offsets, int64_t max_rows, int64_t epi,
                  std::optional<Tensor> a_rows) {
  check_bf16(out, "out"); check_bf16(a, "a"); check_bf16(w, "w"); check_i32(offsets, "offsets");
  TORCH_CHECK(a.dim() == 2 && w.dim() == 3 && w.size(2) == a.size(1), "a [M, K], w [G, N, K]");
  // with a_rows the permuted rows are out's (M = out rows) and a holds the token rows they name
  const int64_t M = a_rows ? out.size(0) : a.size(0), K = a.size(1), N = w.size(1), G = w.size(0);
  TORCH_CHECK(offsets.numel() == G + 1, "offsets must be [G + 1]");
  TORCH_CHECK(K % 64 == 0 && N % 32 == 0, "K % 64, N % 32");
  TORCH_CHECK(out.size(0) == M && out.size(1) == (epi == 0 ? N : N / 2), "out shape");
  if (a_rows) {
    check_i32(*a_rows, "a_rows");
    TORCH_CHECK(a_rows->numel() >= M, "a_rows [M]: every permuted row's token row");
  }
  c10::DeviceGuard g(a.device());
  mlop::launch_grouped_gemm(a.data_ptr(), w.data_ptr(), out.data_ptr(), offsets.data_ptr<int>(),
                            (int)G, (int)M, (int)N, (int)K, (int)max_rows, (int)epi, cur_stream(),
                            a_rows ? a_rows->data_ptr<int>() : nullptr);
}

void moe_route(Tensor topw, Tensor topi, Tensor logits) {
  check_bf16(logits, "router logits");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) <= 64, "router logits [T, E<=64]");
  const int64_t T = logits.size(0), E = logits.size(1), k = topi.size(1);
  TORCH_CHECK(k >= 1 && k <= E && k <= 8, "1 <= top_k <= min(E, 8)");
  check_i32(topi, "topi");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.numel() == T * k &&
                  topi.numel() == T * k, "topw/topi [T, k]");
  c10::DeviceGuard g(logits.device());
  mlop::launch_moe_route(topw.data_ptr<float>(), topi.data_ptr<int>(), logits.data_ptr(), (int)T,
                         (int)E, (int)k, cur_stream());
}

void moe_permute(Tensor xp, Tensor offsets, Tensor src, Tensor inv, Tensor x, Tensor topi,
                 int64_t e0, int64_t n_local) {
  check_bf16(xp, "xp"); check_bf16(x, "x"); check_i32(offsets, "offsets"); check_i32(src, "src");
  check_i32(inv, "inv"); check_i32(topi, "topi");
  const int64_t T = topi.size(0), k = topi.size(1), H = x.size(1);
  TORCH_CHECK(x.dim() == 2 && x.size(0) == T && H % 8 == 0, "x [T, H]");
  TORCH_CHECK(xp.size(0) == T * k && xp.size(1) == H, "xp [T*k, H]");
  TORCH_CHECK(n_local >= 1 && n_local <= 256 && offsets.numel() == n_local + 1, "offsets");
  TORCH_CHECK(src.numel() == T * k && inv.numel() == T * k, "src/inv [T*k]");
  c10::DeviceGuard g(x.device());
  mlop::launch_moe_permute(xp.data_ptr(), offsets.data_ptr<int>(), src.data_ptr<int>(),
                           inv.data_ptr<int>(), x.data_ptr(), topi.data_ptr<int>(), (int)T, (int)k,
                           (int)H, (int)e0, (int)n_local, cur_stream());
}

// decode-size dispatch (T <= 16): router GEMV + route + sort + gather in one launch; false = not taken
bool moe_dispatch_small(Tensor topw, Tensor topi, Tensor xp, Tensor offsets, Tensor src, Tensor inv, Tensor x,
                        Tensor router_w, int64_t e0, int64_t n_local, std::optional<Tensor> pro_y,
                        std::optional<Tensor> pro_res, std::optional<Tensor> pro_w, double pro_eps) {
  check_bf16(xp, "xp"); check_bf16(x, "x"); check_bf16(router_w, "router_w"); check_i32(topi, "topi");
  check_i32(offsets, "offsets"); check_i32(src, "src"); check_i32(inv, "inv");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_contiguous(), "topw f32");
  const int64_t T = x.size(0), H = x.size(1), E = router_w.size(0), k = topi.size(1);
  if (!mlop::moe_dispatch_small_takes((int)T, (int)E, (int)k, (int)H)) return false;
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && router_w.size(1) == H, "x [T, H], router_w [E, H]");
  TORCH_CHECK(topi.size(0) == T && topw.numel() == T * k && xp.size(0) == T * k && xp.size(1) == H,
              "topi/topw [T, k], xp [T*k, H]");
  TORCH_CHECK(n_local >= 1 && n_local <= 64 && offsets.numel() == n_local + 1 && src.numel() == T * k &&
                  inv.numel() == T * k, "offsets / src / inv");
  const bool pro = pro_y.has_value();
  if (pro) {  // x is the OUTPUT of the prologue here
    check_bf16(*pro_y, "pro_y"); check_bf16(*pro_res, "pro_res"); check_bf16(*pro_w, "pro_w");
    TORCH_CHECK(pro_y->numel() == T * H && pro_res->numel() == T * H && pro_w->numel() == H && H <= 8192,
                "prologue y / residual [T, H], w [H]");
  }
  c10::DeviceGuard g(x.device());
  mlop::launch_moe_dispatch_small(topw.data_ptr<float>(), topi.data_ptr<int>(), xp.data_ptr(),
                                  offsets.data_ptr<int>(), src.data_ptr<int>(), inv.data_ptr<int>(), x.data_ptr(),
                                  router_w.data_ptr(), (int)T, (int)E, (int)k, (int)H, (int)e0, (int)n_local,
                                  pro ? pro_y->data_ptr() : nullptr, pro ? pro_res->data_ptr() : nullptr,
                                  pro ? pro_w->data_ptr() : nullptr, (float)pro_eps, pro ? x.data_ptr() : nullptr,
                                  cur_stream());
  return true;
}

// mid-size dispatch (16 < T <= moe_mid_max_tokens): router GEMV + route per workgroup, the last sorts; no
// gather (arow: token row of each permuted row); false = not taken
bool moe_dispatch_mid(Tensor topw, Tensor topi, Tensor offsets, Tensor arow, Tensor inv, Tensor x, Tensor router_w,
                      int64_t e0, int64_t n_local, std::optional<Tensor> pro_y, std::optional<Tensor> pro_res,
                      std::optional<Tensor> pro_w, double pro_eps) {
  check_bf16(x, "x"); check_bf16(router_w, "router_w"); check_i32(topi, "topi");
  check_i32(offsets, "offsets"); check_i32(arow, "arow"); check_i32(inv, "inv");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_contiguous(), "topw f32");
  const int64_t T = x.size(0), H = x.size(1), E = router_w.size(0), k = topi.size(1);
  if (!mlop::moe_dispatch_mid_takes((int)T, (int)E, (int)k, (int)H)) return false;
  TORCH_CHECK(x.dim() == 2 && x.is_contiguous() && router_w.size(1) == H && router_w.is_contiguous(),
              "x [T, H], router_w [E, H]");
  TORCH_CHECK(topi.size(0) == T && topi.is_contiguous() && topw.numel() == T * k, "topi/topw [T, k]");
  TORCH_CHECK(n_local >= 1 && n_local <= 64 && offsets.numel() == n_local + 1 && arow.numel() == T * k &&
                  inv.numel() == T * k, "offsets / arow / inv");
  const bool pro = pro_y.has_value();
  if (pro) {  // x is the OUTPUT of the prologue here
    check_bf16(*pro_y, "pro_y"); check_bf16(*pro_res, "pro_res"); check_bf16(*pro_w, "pro_w");
    TORCH_CHECK(pro_y->numel() == T * H && pro_res->numel() == T * H && pro_w->numel() == H && H <= 8192,
                "prologue y / residual [T, H], w [H]");
  }
  c10::DeviceGuard g(x.device());
  mlop::launch_moe_dispatch_mid(topw.data_ptr<float>(), topi.data_ptr<int>(), offsets.data_ptr<int>(),
                                arow.data_ptr<int>(), inv.data_ptr<int>(), x.data_ptr(), router_w.data_ptr(), (int)T,
                                (int)E, (int)k, (int)H, (int)e0, (int)n_local, pro ? pro_y->data_ptr() : nullptr,
                                pro ? pro_res->data_ptr() : nullptr, pro ? pro_w->data_ptr() : nullptr, (float)pro_eps,
                                pro ? x.data_ptr() : nullptr, cur_stream());
  return true;
}

bool moe_combine_add_rmsnorm(Tensor out, Tensor residual, Tensor y, Tensor inv, Tensor topw, Tensor norm_w,
                             double eps) {
  check_bf16(out, "out"); check_bf16(residual, "residual"); check_bf16(y, "y"); check_bf16(norm_w, "norm_w");
  check_i32(inv, "inv");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.dim() == 2, "topw");
  const int64_t T = topw.size(0), k = topw.size(1), H = y.size(1);
  TORCH_CHECK(out.numel() == T * H && residual.numel() == T * H && inv.numel() == T * k && norm_w.numel() == H,
              "combine + norm shapes");
  c10::DeviceGuard g(y.device());
  return mlop::launch_moe_combine_add_rmsnorm(out.data_ptr(), residual.data_ptr(), y.data_ptr(),
                                              inv.data_ptr<int>(), topw.data_ptr<float>(), norm_w.data_ptr(),
                                              (float)eps, (int)T, (int)k, (int)H, cur_stream());
}

// grouped down GEMM + combine + residual add + RMSNorm: the combine sums the GEMM's split-K slabs
// itself (y is written only when the GEMM does not split); false = shape not supported
bool moe_down_combine_add_rmsnorm(Tensor out, Tensor residual, Tensor y, Tensor a, Tensor w2, Tensor offsets,
                                  int64_t max_rows, Tensor inv, Tensor topw, Tensor norm_w, double eps) {
  check_bf16(out, "out"); check_bf16(residual, "residual"); check_bf16(y, "y"); check_bf16(a, "a");
  check_bf16(w2, "w2"); check_bf16(norm_w, "norm_w"); check_i32(offsets, "offsets"); check_i32(inv, "inv");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.dim() == 2, "topw");
  TORCH_CHECK(a.dim() == 2 && w2.dim() == 3 && w2.size(2) == a.size(1), "a [R, I], w2 [G, H, I]");
  const int64_t R = a.size(0), I = a.size(1), H = w2.size(1), G = w2.size(0);
  const int64_t T = topw.size(0), k = topw.size(1);
  TORCH_CHECK(offsets.numel() == G + 1 && I % 64 == 0 && H % 32 == 0, "offsets [G + 1], I % 64, H % 32");
  TORCH_CHECK(y.size(0) == R && y.size(1) == H && out.numel() == T * H && residual.numel() == T * H &&
                  inv.numel() == T * k && norm_w.numel() == H, "y [R, H], out / residual [T, H]");
  c10::DeviceGuard g(a.device());
  return mlop::launch_moe_down_combine_add_rmsnorm(
      out.data_ptr(), residual.data_ptr(), y.data_ptr(), a.data_ptr(), w2.data_ptr(), offsets.data_ptr<int>(), (int)G,
      (int)R, (int)H, (int)I, (int)max_rows, inv.data_ptr<int>(), topw.data_ptr<float>(), norm_w.data_ptr(),
      (float)eps, (int)T, (int)k, cur_stream());
}

void moe_combine(Tensor out, Tensor y, Tensor inv, Tensor topw) {
  check_bf16(out, "out"); check_bf16(y, "y"); check_i32(inv, "inv");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_contiguous() && topw.dim() == 2, "topw");
  const int64_t T = topw.size(0), k = topw.size(1), H = y.size(1);
  TORCH_CHECK(out.size(0) == T && out.size(1) == H && inv.numel() == T * k && H % 8 == 0,
              "combine shapes");
  c10::DeviceGuard g(y.device());
  mlop::launch_moe_combine(out.data_ptr(), y.data_ptr(), inv.data_ptr<int>(),
                           topw.data_ptr<float>(), (int)T, (int)k, (int)H, cur_stream());
}

void check_logits(const Tensor& logits) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat && logits.dim() == 2 &&
                  logits.stride(1) == 1 && logits.stride(0) % 4 == 0,
              "logits must be f32 [n, V] with unit inner stride and 16-B aligned rows");
  TORCH_CHECK(reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0, "logits 16-B aligned");
}

void argmax(Tensor out, Tensor logits) {
  TORCH_CHECK(out.scalar_type() == at::kLong && out.numel() == logits.size(0), "out int64 [n]");
  if (logits.scalar_type() == at::kBFloat16) {
    TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1 && logits.stride(0) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
                "bf16 logits must be [n, V] with unit inner stride and 16-B aligned rows");
    c10::DeviceGuard g(logits.device());
    const int n = (int)logits.size(0), V = (int)logits.size(1);
    const int S = mlop::argmax_splits(n, V);
    at::Tensor ws;  // per-(row, split) keys from the caching allocator (graph-capture safe)
    if (S > 1) ws = at::empty({(int64_t)n * S}, logits.options().dtype(at::kLong));
    mlop::launch_argmax_bf16(out.data_ptr<int64_t>(), logits.data_ptr(), n, V, logits.stride(0),
                             S > 1 ? ws.data_ptr() : nullptr, cur_stream());
    return;
  }
  check_logits(logits);
  c10::DeviceGuard g(logits.device());
  mlop::launch_argmax(out.data_ptr<int64_t>(), logits.data_ptr<float>(), (int)logits.size(0),
                      (int)logits.size(1), logits.stride(0), cur_stream());
}

void sample(Tensor out, Tensor logits, Tensor temps, Tensor top_ks, Tensor top_ps, Tensor uniform, bool full) {
  check_logits(logits);
  const int64_t n = logits.size(0);
  TORCH_CHECK(out.scalar_type() == at::kLong && out.numel() == n, "out int64 [n]");
  TORCH_CHECK(temps.scalar_type() == at::kFloat && temps.numel() == n && temps.is_cuda(), "temps");
  TORCH_CHECK(top_ps.scalar_type() == at::kFloat && top_ps.numel() == n && top_ps.is_cuda(), "top_ps");
  TORCH_CHECK(uniform.scalar_type() == at::kFloat && uniform.numel() == n && uniform.is_cuda(), "u");
  check_i32(top_ks, "top_ks");
  TORCH_CHECK(top_ks.numel() == n, "top_ks");
  c10::DeviceGuard g(logits.device());
  const long wsb = mlop::sample_workspace_bytes((int)n, (int)logits.size(1));
  at::Tensor ws;  // candidate buffers from the caching allocator (graph-capture safe)
  if (wsb > 0) ws = at::empty({wsb}, logits.options().dtype(at::kByte));
  mlop::launch_sample(out.data_ptr<int64_t>(), logits.data_ptr<float>(), (int)n,
                      (int)logits.size(1), logits.stride(0), temps.data_ptr<float>(),
                      top_ks.data_ptr<int>(), top_ps.data_ptr<float>(), uniform.data_ptr<float>(),
                      wsb > 0 ? ws.data_ptr() : nullptr, full, cur_stream());
}


// ---- sampler extensions: penalty count table, penalties, token log-probabilities ----
void check_table(const Tensor& table) {
  check_i32(table, "penalty table");
  TORCH_CHECK(table.dim() == 2 && table.size(1) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(table.data_ptr()) % 16 == 0,
              "penalty table must be int32 [slots, ldt] with ldt % 4 == 0 and 16-B aligned");
}
void check_ids(const Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kLong && t.is_contiguous() && t.dim() == 1, name,
              " must be a contiguous int64 [n] GPU tensor");
}
void check_f32n(const Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kFloat && t.is_contiguous() && t.numel() == n, name,
              " must be a contiguous f32 [n] GPU tensor");
}

void penalty_reset(Tensor table, int64_t slot, int64_t vocab, Tensor prompt_ids, Tensor output_ids) {
  check_table(table);
  check_ids(prompt_ids, "prompt_ids");
  check_ids(output_ids, "output_ids");
  TORCH_CHECK(slot >= 0 && slot < table.size(0), "penalty slot out of range");
  TORCH_CHECK(vocab > 0 && vocab <= table.size(1), "vocab must be in (0, ldt]");
  c10::DeviceGuard g(table.device());
  mlop::launch_penalty_reset(table.data_ptr<int>() + slot * table.size(1), (int)vocab, (int)table.size(1),
                             (const long*)prompt_ids.data_ptr<int64_t>(), (int)prompt_ids.numel(),
                             (const long*)output_ids.data_ptr<int64_t>(), (int)output_ids.numel(), cur_stream());
}

void penalty_update(Tensor table, int64_t vocab, Tensor slots, Tensor tokens) {
  check_table(table);
  check_i32(slots, "slots");
  check_ids(tokens, "tokens");
  TORCH_CHECK(slots.numel() == tokens.numel(), "slots / tokens length");
  TORCH_CHECK(vocab > 0 && vocab <= table.size(1), "vocab must be in (0, ldt]");
  c10::DeviceGuard g(table.device());
  mlop::launch_penalty_update(table.data_ptr<int>(), table.size(1), (int)vocab, (int)table.size(0),
                              slots.data_ptr<int>(), (const long*)tokens.data_ptr<int64_t>(), (int)tokens.numel(),
                              cur_stream());
}

// ---- speculative decoding by prompt lookup (spec.hip) ----
int64_t check_spec_state(const Tensor& hist, const Tensor& hist_len, const Tensor& rows, const Tensor& out) {
  check_i32(hist, "hist");
  check_i32(hist_len, "hist_len");
  check_i32(rows, "rows");
  check_i32(out, "out");
  TORCH_CHECK(hist.dim() == 2 && hist_len.dim() == 1 && hist_len.size(0) == hist.size(0),
              "hist must be int32 [R, max_len] and hist_len int32 [R]");
  const int64_t B = rows.numel();
  TORCH_CHECK(out.dim() == 2 && out.size(0) == B && out.size(1) >= 5 && out.size(1) % 2 == 1,
              "out must be int32 [B, 2 + (k + 1) + k]");
  const int64_t k = (out.size(1) - 3) / 2;
  TORCH_CHECK(k >= 1 && k <= 7, "spec tokens k must be in [1, 7]");
  return k;
}

void spec_accept(Tensor sampled, Tensor q_start, Tensor drafts, Tensor nd, Tensor rows, Tensor hist, Tensor hist_len,
                 Tensor out) {
  const int64_t k = check_spec_state(hist, hist_len, rows, out);
  check_ids(sampled, "sampled");
  check_i32(q_start, "q_start");
  check_i32(drafts, "drafts");
  check_i32(nd, "nd");
  const int64_t B = rows.numel();
  TORCH_CHECK(q_start.numel() == B && nd.numel() == B && drafts.numel() == B * k,
              "q_start / nd must be int32 [B] and drafts int32 [B, k]");
  c10::DeviceGuard g(hist.device());
  mlop::launch_spec_accept((const long*)sampled.data_ptr<int64_t>(), (int)sampled.numel(), q_start.data_ptr<int>(),
                           drafts.data_ptr<int>(), nd.data_ptr<int>(), rows.data_ptr<int>(), hist.data_ptr<int>(),
                           hist.size(1), (int)hist.size(1), hist_len.data_ptr<int>(), (int)hist.size(0),
                           out.data_ptr<int>(), (int)k, (int)B, cur_stream());
}

void spec_propose(Tensor hist, Tensor hist_len, Tensor rows, Tensor cap, int64_t n_max, int64_t n_min, Tensor out) {
  const int64_t k = check_spec_state(hist, hist_len, rows, out);
  check_i32(cap, "cap");
  TORCH_CHECK(cap.numel() == rows.numel(), "cap must be int32 [B]");
  TORCH_CHECK(1 <= n_min && n_min <= n_max && n_max <= 8, "n-gram lengths must satisfy 1 <= n_min <= n_max <= 8");
  c10::DeviceGuard g(hist.device());
  mlop::launch_spec_propose(hist.data_ptr<int>(), hist.size(1), (int)hist.size(1), hist_len.data_ptr<int>(),
                            (int)hist.size(0), rows.data_ptr<int>(), cap.data_ptr<int>(), (int)n_max, (int)n_min,
                            out.data_ptr<int>(), (int)k, (int)rows.numel(), cur_stream());
}

// embedding pooling (pool.hip): seg int32 [>= nseg, 4] = [r0, r1, slot, flags], acc fp32 [S, H]
static void check_pool_state(const Tensor& acc, const Tensor& meta, int64_t n, const char* name) {
  TORCH_CHECK(acc.is_cuda() && acc.scalar_type() == at::kFloat && acc.dim() == 2 && acc.is_contiguous(),
              "acc must be a contiguous fp32 GPU tensor [slots, H]");
  TORCH_CHECK(acc.size(1) % 8 == 0 && acc.size(1) <= 65536 && acc.size(0) <= INT_MAX,
              "hidden size must be a multiple of 8");
  TORCH_CHECK((uintptr_t)acc.data_ptr() % 16 == 0, "acc must be 16-byte aligned");
  check_i32(meta, name);
  TORCH_CHECK(meta.dim() == 2 && meta.size(1) == 4 && n >= 0 && n <= meta.size(0) && n <= 65535, name,
              " must be int32 [n, 4] with n <= 65535");
  TORCH_CHECK((uintptr_t)meta.data_ptr() % 16 == 0, name, " must be 16-byte aligned");
  TORCH_CHECK(meta.device() == acc.device(), name, " must be on acc's device");
}

void pool_accumulate(Tensor acc, Tensor x, Tensor seg, int64_t nseg) {
  check_pool_state(acc, seg, nseg, "seg");
  const int64_t H = acc.size(1);
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 2 && x.size(1) == H &&
                  (x.size(0) == 0 || x.stride(1) == 1) && x.stride(0) >= H && x.stride(0) % 8 == 0,
              "x must be bf16 [T, H] with unit column stride and a row stride that is a multiple of 8");
  TORCH_CHECK((uintptr_t)x.data_ptr() % 16 == 0 && x.size(0) <= INT_MAX, "x must be 16-byte aligned");
  TORCH_CHECK(x.device() == acc.device(), "x must be on acc's device");
  c10::DeviceGuard g(acc.device());
  mlop::launch_pool_accumulate(acc.data_ptr<float>(), x.data_ptr(), x.stride(0), seg.data_ptr<int>(), (int)nseg,
                               (int)x.size(0), (int)H, (int)acc.size(0), cur_stream());
}

void pool_finish(Tensor out, Tensor acc, Tensor fin, int64_t nfin) {
  check_pool_state(acc, fin, nfin, "fin");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kFloat && out.dim() == 2 && out.is_contiguous() &&
                  out.size(0) == acc.size(0) && out.size(1) == acc.size(1) && out.device() == acc.device(),
              "out must be a contiguous fp32 GPU tensor of acc's shape");
  c10::DeviceGuard g(acc.device());
  mlop::launch_pool_finish(out.data_ptr<float>(), out.size(1), acc.data_ptr<float>(), fin.data_ptr<int>(), (int)nfin,
                           (int)acc.size(1), (int)acc.size(0), cur_stream());
}

void apply_penalties(Tensor logits, Tensor table, Tensor slots, Tensor rep, Tensor freq, Tensor pres) {
  check_logits(logits);
  check_table(table);
  const int64_t n = logits.size(0);
  check_i32(slots, "slots");
  TORCH_CHECK(slots.numel() == n, "slots");
  check_f32n(rep, n, "rep");
  check_f32n(freq, n, "freq");
  check_f32n(pres, n, "pres");
  TORCH_CHECK(logits.size(1) <= table.size(1), "the table's rows are shorter than the vocabulary");
  c10::DeviceGuard g(logits.device());
  mlop::launch_apply_penalties(logits.data_ptr<float>(), (int)n, (int)logits.size(1), logits.stride(0),
                               table.data_ptr<int>(), table.size(1), (int)table.size(0), slots.data_ptr<int>(),
                               rep.data_ptr<float>(), freq.data_ptr<float>(), pres.data_ptr<float>(), cur_stream());
}

// ---- guided decoding (guided.hip) ----
void check_grammar(const Tensor& arena, const Tensor& base, const Tensor& rows, const Tensor& state, int64_t n) {
  TORCH_CHECK(arena.is_cuda() && arena.scalar_type() == at::kShort && arena.is_contiguous() && arena.dim() == 2 &&
                  arena.size(1) % 8 == 0 && reinterpret_cast<uintptr_t>(arena.data_ptr()) % 16 == 0,
              "grammar arena must be a contiguous int16 [states, ldv] GPU tensor with ldv % 8 == 0, 16-B aligned");
  check_i32(base, "base");
  check_i32(rows, "rows");
  check_i32(state, "state");
  TORCH_CHECK(base.numel() == n && rows.numel() == n, "base / rows must be int32 [n]");
  TORCH_CHECK(arena.size(0) <= INT_MAX && state.numel() <= INT_MAX, "grammar arena / state too large");
}

void grammar_mask(Tensor logits, Tensor arena, Tensor base, Tensor rows, Tensor state) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat && logits.dim() == 2 && logits.stride(1) == 1 &&
                  (logits.size(0) <= 1 || logits.stride(0) >= logits.size(1)),
              "logits must be f32 [n, V] with unit inner stride and rows that do not overlap");
  const int64_t n = logits.size(0);
  check_grammar(arena, base, rows, state, n);
  TORCH_CHECK(logits.size(1) <= arena.size(1), "the arena's rows are shorter than the vocabulary");
  c10::DeviceGuard g(logits.device());
  mlop::launch_grammar_mask(logits.data_ptr<float>(), (int)n, (int)logits.size(1), logits.stride(0),
                            (const short*)arena.data_ptr<int16_t>(), arena.size(1), (int)arena.size(0),
                            base.data_ptr<int>(), rows.data_ptr<int>(), state.data_ptr<int>(), (int)state.numel(),
                            cur_stream());
}

void grammar_advance(Tensor arena, int64_t vocab, Tensor base, Tensor rows, Tensor state, Tensor tokens) {
  check_ids(tokens, "tokens");
  check_grammar(arena, base, rows, state, tokens.numel());
  TORCH_CHECK(vocab > 0 && vocab <= arena.size(1), "vocab must be in (0, ldv]");
  c10::DeviceGuard g(arena.device());
  mlop::launch_grammar_advance((const short*)arena.data_ptr<int16_t>(), arena.size(1), (int)arena.size(0), (int)vocab,
                               base.data_ptr<int>(), rows.data_ptr<int>(), state.data_ptr<int>(), (int)state.numel(),
                               (const long*)tokens.data_ptr<int64_t>(), (int)tokens.numel(), cur_stream());
}

void token_logprobs(Tensor out_lp, Tensor out_id, Tensor logits, Tensor chosen, Tensor want) {
  const bool bf = logits.scalar_type() == at::kBFloat16;
  if (bf) {
    TORCH_CHECK(logits.is_cuda() && logits.dim() == 2 && logits.stride(1) == 1 && logits.stride(0) % 8 == 0 &&
                    reinterpret_cast<uintptr_t>(logits.data_ptr()) % 16 == 0,
                "bf16 logits must be [n, V] with unit inner stride and 16-B aligned rows");
  } else {
    check_logits(logits);
  }
  const int64_t n = logits.size(0), V = logits.size(1);
  TORCH_CHECK(out_lp.is_cuda() && out_lp.scalar_type() == at::kFloat && out_lp.is_contiguous() &&
                  out_lp.dim() == 2 && out_lp.size(0) == n && out_lp.size(1) >= 1,
              "out_lp must be a contiguous f32 [n, 1 + N]");
  check_i32(out_id, "out_id");
  TORCH_CHECK(out_id.sizes() == out_lp.sizes(), "out_id must have out_lp's shape");
  check_ids(chosen, "chosen");
  check_i32(want, "want");
  TORCH_CHECK(chosen.numel() == n && want.numel() == n, "chosen / want length");
  TORCH_CHECK(mlop::logprob_splits((int)n, (int)V) > 0, "vocabulary too large for token_logprobs");
  c10::DeviceGuard g(logits.device());
  if (n == 0) return;
  at::Tensor ws = at::empty({mlop::logprob_workspace_bytes((int)n, (int)V)}, logits.options().dtype(at::kByte));
  mlop::launch_token_logprobs(out_lp.data_ptr<float>(), out_id.data_ptr<int>(), (int)out_lp.size(1),
                              logits.data_ptr(), bf, (int)n, (int)V, logits.stride(0),
                              (const long*)chosen.data_ptr<int64_t>(), want.data_ptr<int>(), ws.data_ptr(),
                              cur_stream());
}


// ---- K15 custom all-reduce: host-side state, int handles -------------------
int64_t car_create(int64_t rank, int64_t world, int64_t max_bytes, int64_t device, bool split) {
  return mlop::car_create((int)rank, (int)world, (long)max_bytes, (int)device, split ? 1 : 0);
}
Tensor car_ipc_handle(int64_t h) {
  Tensor t = at::empty({128}, at::TensorOptions().dtype(at::kByte));
  mlop::car_ipc_handle((long)h, t.data_ptr());
  return t;
}
void car_open(int64_t h, Tensor handles) {
  TORCH_CHECK(!handles.is_cuda() && handles.scalar_type() == at::kByte && handles.is_contiguous() &&
              handles.dim() == 2 && handles.size(1) == 128, "handles: CPU uint8 [world, 128]");
  mlop::car_open((long)h, handles.data_ptr());
}
void car_all_reduce(int64_t h, Tensor out, Tensor inp, bool two_shot) {
  check_bf16(out, "out"); check_bf16(inp, "inp");
  TORCH_CHECK(out.numel() == inp.numel(), "all_reduce: out/inp size mismatch");
  TORCH_CHECK(inp.numel() % 8 == 0, "all_reduce: numel must be a multiple of 8");
  TORCH_CHECK(inp.numel() * 2 * (two_shot ? 2 : 1) <= mlop::car_max_bytes((long)h),
              "all_reduce: message exceeds the registered buffer");
  c10::DeviceGuard g(inp.device());
  mlop::car_all_reduce((long)h, out.data_ptr(), inp.data_ptr(), (long)inp.numel(), cur_stream(), two_shot);
}
// residual = bf16(residual + bf16(sum over ranks of inp)): one-shot all-reduce + the residual add
void car_all_reduce_add(int64_t h, Tensor residual, Tensor inp) {
  check_bf16(residual, "residual"); check_bf16(inp, "inp");
  TORCH_CHECK(residual.numel() == inp.numel() && residual.is_contiguous() && inp.is_contiguous(),
              "all_reduce_add: contiguous residual / inp of one size");
  TORCH_CHECK(residual.data_ptr() != inp.data_ptr(), "all_reduce_add: residual must not alias inp");
  TORCH_CHECK(inp.numel() % 8 == 0, "all_reduce_add: numel must be a multiple of 8");
  TORCH_CHECK(inp.numel() * 2 <= mlop::car_max_bytes((long)h), "all_reduce_add: message exceeds the registered buffer");
  c10::DeviceGuard g(inp.device());
  mlop::car_all_reduce((long)h, residual.data_ptr(), inp.data_ptr(), (long)inp.numel(), cur_stream(), false, true);
}
// in-place broadcast of any contiguous device tensor (bytes % 16 == 0) from `root`
void car_broadcast(int64_t h, Tensor buf, int64_t root) {
  TORCH_CHECK(buf.is_cuda() && buf.is_contiguous(), "broadcast: contiguous device tensor");
  const long nbytes = (long)(buf.numel() * buf.element_size());
  c10::DeviceGuard g(buf.device());
  mlop::car_broadcast((long)h, buf.data_ptr(), buf.data_ptr(), nbytes, (int)root, cur_stream());
}
// out [world * piece] <- every rank's contiguous piece (bytes % 4 == 0), rank order
void car_all_gather(int64_t h, Tensor out, Tensor piece) {
  TORCH_CHECK(piece.is_cuda() && piece.is_contiguous() && out.is_cuda() && out.is_contiguous() &&
                  out.scalar_type() == piece.scalar_type(), "all-gather: contiguous device tensors of one dtype");
  const long nbytes = (long)(piece.numel() * piece.element_size());
  c10::DeviceGuard g(piece.device());
  mlop::car_all_gather((long)h, out.data_ptr(), (long)(out.numel() * out.element_size()), piece.data_ptr(), nbytes,
                       cur_stream());
}
int64_t car_error(int64_t h) { return mlop::car_error((long)h); }
int64_t car_mem_mode(int64_t h) { return mlop::car_mem_mode((long)h); }
void car_destroy(int64_t h) { mlop::car_destroy((long)h); }

// ---- TP step-header channel over POSIX shared memory (shm_channel.cc) -------------
int64_t chan_create(std::string name, int64_t slots, int64_t consumers) {
  return mlop::chan_create(name, (int)slots, (int)consumers);
}
int64_t chan_open(std::string name) { return mlop::chan_open(name); }
bool chan_send(int64_t h, Tensor vals, int64_t timeout_us) {
  TORCH_CHECK(!vals.is_cuda() && vals.scalar_type() == at::kLong && vals.is_contiguous(), "vals: CPU int64");
  return mlop::chan_send((long)h, vals.data_ptr<int64_t>(), (int)vals.numel(), (long)timeout_us);
}
bool chan_recv(int64_t h, int64_t consumer, Tensor out, int64_t timeout_us) {
  TORCH_CHECK(!out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous(), "out: CPU int64");
  return mlop::chan_recv((long)h, (int)consumer, out.data_ptr<int64_t>(), (int)out.numel(), (long)timeout_us);
}
void chan_unlink(std::string name) { mlop::chan_unlink(name); }
void chan_close(int64_t h, bool unlink) { mlop::chan_close((long)h, unlink); }
int64_t xg_create(std::string name, int64_t world, int64_t slots, int64_t max_words) {
  return mlop::xg_create(name, (int)world, (int)slots, (long)max_words);
}
int64_t xg_open(std::string name, int64_t rank) { return mlop::xg_open(name, (int)rank); }
bool xg_exchange(int64_t h, Tensor vals, Tensor out, Tensor counts, int64_t timeout_us) {
  const long mw = mlop::xg_max_words((long)h);
  TORCH_CHECK(!vals.is_cuda() && vals.scalar_type() == at::kLong && vals.is_contiguous() && vals.dim() == 1,
              "xg_exchange: vals must be a contiguous CPU int64 vector");
  TORCH_CHECK(!out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() && out.dim() == 2 &&
              out.size(1) == mw, "xg_exchange: out must be CPU int64 [world, max_words]");
  TORCH_CHECK(!counts.is_cuda() && counts.scalar_type() == at::kLong && counts.is_contiguous() &&
              counts.numel() == out.size(0), "xg_exchange: counts must be CPU int64 [world]");
  return mlop::xg_exchange((long)h, vals.data_ptr<int64_t>(), (long)vals.numel(), out.data_ptr<int64_t>(),
                           counts.data_ptr<int64_t>(), (long)timeout_us);
}
void xg_close(int64_t h) { mlop::xg_close((long)h); }

// ---- expert-parallel exchange over IPC peer memory (ep_exchange.hip) -------------
int64_t ep_create(int64_t rank, int64_t world, int64_t E, int64_t k, int64_t H, int64_t tcap, int64_t device) {
  return mlop::ep_create((int)rank, (int)world, (int)E, (int)k, (int)H, (int)tcap, (int)device);
}
Tensor ep_ipc_handle(int64_t h) {
  Tensor t = at::empty({64}, at::TensorOptions().dtype(at::kByte));
  mlop::ep_ipc_handle((long)h, t.data_ptr());
  return t;
}
void ep_open(int64_t h, Tensor handles) {
  TORCH_CHECK(!handles.is_cuda() && handles.scalar_type() == at::kByte && handles.is_contiguous() &&
              handles.dim() == 2 && handles.size(1) == 64, "handles: CPU uint8 [world, 64]");
  mlop::ep_open((long)h, handles.data_ptr());
}
// xp [rows, H] bf16 <- this rank's received rows grouped by local expert; offsets int32 [n_local + 1]
void ep_dispatch(int64_t h, Tensor xp, Tensor offsets, Tensor x, Tensor topi) {
  const long H = mlop::ep_hidden((long)h), k = mlop::ep_topk((long)h);
  check_bf16(xp, "xp"); check_bf16(x, "x"); check_i32(topi, "topi"); check_i32(offsets, "offsets");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == H && xp.dim() == 2 && xp.size(1) == H, "ep_dispatch: [*, H] rows");
  TORCH_CHECK(topi.dim() == 2 && topi.size(0) == x.size(0) && topi.size(1) == k, "ep_dispatch: topi [T, k]");
  TORCH_CHECK(offsets.numel() == mlop::ep_local_experts((long)h) + 1, "ep_dispatch: offsets [n_local + 1]");
  TORCH_CHECK(x.size(0) <= mlop::ep_tcap((long)h), "ep_dispatch: T exceeds the exchange's token capacity");
  c10::DeviceGuard g(x.device());
  mlop::ep_dispatch((long)h, xp.data_ptr(), (long)xp.size(0), offsets.data_ptr<int>(), x.data_ptr(),
                    topi.data_ptr<int>(), (int)x.size(0), cur_stream());
}
// out [T, H] bf16 <- sum_j topw[t, j] * expert_j(x[t]) from the owners of the experts
void ep_combine(int64_t h, Tensor out, Tensor y, Tensor topw, Tensor topi) {
  const long H = mlop::ep_hidden((long)h), k = mlop::ep_topk((long)h);
  check_bf16(out, "out"); check_bf16(y, "y"); check_i32(topi, "topi");
  TORCH_CHECK(topw.scalar_type() == at::kFloat && topw.is_cuda() && topw.is_contiguous(), "topw fp32");
  TORCH_CHECK(out.dim() == 2 && out.size(1) == H && y.dim() == 2 && y.size(1) == H, "ep_combine: [*, H] rows");
  TORCH_CHECK(topw.numel() == out.size(0) * k && topi.numel() == out.size(0) * k, "ep_combine: [T, k] routing");
  c10::DeviceGuard g(out.device());
  mlop::ep_combine((long)h, out.data_ptr(), y.data_ptr(), (long)y.size(0), topw.data_ptr<float>(),
                   topi.data_ptr<int>(), (int)out.size(0), cur_stream());
}
int64_t ep_error(int64_t h) { return mlop::ep_error((long)h); }
int64_t ep_mem_mode(int64_t h) { return mlop::ep_mem_mode((long)h); }
void ep_destroy(int64_t h) { mlop::ep_destroy((long)h); }

}  // namespace

// sha256 of the sources this library was built from (ops/build.py writes srchash.cpp)
extern "C" const char* mlop_src_hash();
std::string src_hash() { return std::string(mlop_src_hash()); }

TORCH_LIBRARY(mlop, m) {
  m.def("src_hash() -> str", &src_hash);
  m.def("device_delay(int us) -> ()", &device_delay);
  m.def("car_create(int rank, int world, int max_bytes, int device, bool split=False) -> int", &car_create);
  m.def("car_ipc_handle(int h) -> Tensor", &car_ipc_handle);
  m.def("car_open(int h, Tensor handles) -> ()", &car_open);
  m.def("car_all_reduce(int h, Tensor(a!) out, Tensor inp, bool two_shot=False) -> ()");
  m.def("car_all_reduce_add(int h, Tensor(a!) residual, Tensor inp) -> ()");
  m.def("car_broadcast(int h, Tensor(a!) buf, int root) -> ()");
  m.def("car_all_gather(int h, Tensor(a!) out, Tensor piece) -> ()");
  m.def("car_error(int h) -> int", &car_error);
  m.def("attn_fused_max_pairs(int n) -> int", &attn_fused_max_pairs);
  m.def("car_mem_mode(int h) -> int", &car_mem_mode);
  m.def("car_destroy(int h) -> ()", &car_destroy);
  m.def("chan_create(str name, int slots, int consumers) -> int", &chan_create);
  m.def("chan_open(str name) -> int", &chan_open);
  m.def("chan_send(int h, Tensor vals, int timeout_us) -> bool", &chan_send);
  m.def("chan_recv(int h, int consumer, Tensor(a!) out, int timeout_us) -> bool", &chan_recv);
  m.def("chan_unlink(str name) -> ()", &chan_unlink);
  m.def("chan_close(int h, bool unlink) -> ()", &chan_close);
  m.def("xg_create(str name, int world, int slots, int max_words) -> int", &xg_create);
  m.def("xg_open(str name, int rank) -> int", &xg_open);
  m.def("xg_exchange(int h, Tensor vals, Tensor(a!) out, Tensor(b!) counts, int timeout_us) -> bool", &xg_exchange);
  m.def("xg_close(int h) -> ()", &xg_close);
  m.def("ep_create(int rank, int world, int E, int k, int H, int tcap, int device) -> int", &ep_create);
  m.def("ep_ipc_handle(int h) -> Tensor", &ep_ipc_handle);
  m.def("ep_open(int h, Tensor handles) -> ()", &ep_open);
  m.def("ep_dispatch(int h, Tensor(a!) xp, Tensor(b!) offsets, Tensor x, Tensor topi) -> ()");
  m.def("ep_combine(int h, Tensor(a!) out, Tensor y, Tensor topw, Tensor topi) -> ()");
  m.def("ep_error(int h) -> int", &ep_error);
  m.def("ep_mem_mode(int h) -> int", &ep_mem_mode);
  m.def("ep_destroy(int h) -> ()", &ep_destroy);
  m.def("gemm_workspace(int M, int N, int K, int epi) -> int", &gemm_workspace);
  m.def("gemm_big_variant(int set=-1) -> int", &knob<mlop::gemm_big_variant>);
  m.def("gemm_half_tile(int set=-1) -> int", &knob<mlop::gemm_half_tile>);
  m.def("gemm_small_nt(int set=-1) -> int", &knob<mlop::gemm_small_nt>);
  m.def("attn_kv_nt(int set=-1) -> int", &knob<mlop::attn_kv_nt>);
  m.def("gemm_slab_nt(int set=-1) -> int", &knob<mlop::gemm_slab_nt>);
  m.def("gemm_rope_split(int set=-1) -> int", &knob<mlop::gemm_rope_split>);
  m.def("gemm_split_target(int set=-1) -> int", &knob<mlop::gemm_split_target>);
  m.def("gemm_grouped_narrow(int set=-1) -> int", &knob<mlop::gemm_grouped_narrow>);
  m.def("gemm_ws_max_m(int set=-1) -> int", &knob<mlop::gemm_ws_max_m>);
  m.def("decode_chain_max_m() -> int", &decode_chain_max_m);
  m.def("gemm_ws_plan(int rb, int u, int nt) -> ()", &gemm_ws_plan);
  m.def("gemm_ws_small_m(int set=-1) -> int", &knob<mlop::gemm_ws_small_m>);
  m.def("gemm_ws_rope_m(int set=-1) -> int", &knob<mlop::gemm_ws_rope_m>);
  m.def("flash_persist(int set=-1) -> int", &knob<mlop::flash_persist>);
  m.def("flash_stream(int set=-1) -> int", &knob<mlop::flash_stream>);
  m.def("gemm_grouped_balance(int set=-1) -> int", &knob<mlop::gemm_grouped_balance>);
  m.def("gemm_grouped_order(int set=-1) -> int", &knob<mlop::gemm_grouped_order>);
  m.def("moe_mid_tok(int set=-1) -> int", &knob<mlop::moe_mid_tok>);
  m.def("gemm_mid_chain(int set=-1) -> int", &knob<mlop::gemm_mid_chain>);
  m.def("mid_chain_ok(int M, int N, int K, int epi) -> bool", &mid_chain_ok);
  m.def("moe_mid_max_tokens(int set=-1) -> int", &knob<mlop::moe_mid_max_tokens>);
  m.def("gemm_grouped_plan(int bm, int bn, int stages, int splits) -> ()", &gemm_grouped_plan);
  m.def("gemm_dense_plan(int variant, int bm, int bn, int splits, int stages=0) -> ()", &gemm_dense_plan);
  m.def("gemm_small_stages(int set=-1) -> int", &knob<mlop::gemm_small_stages>);
  m.def("gemm_small_tile(int set=-1) -> int", &knob<mlop::gemm_small_tile>);
  m.def("gemm_sk_mode(int set=-1) -> int", &knob<mlop::gemm_sk_mode>);
  m.def("gemm_sk_reserve() -> bool", &gemm_sk_reserve);
  m.def("gemm_sk_workgroups(int M, int N, int K) -> int", &gemm_sk_workgroups);
  m.def("vmm_supported(int device) -> bool", &vmm_supported);
  m.def("vmm_granularity(int device) -> int", &vmm_granularity);
  m.def("vmm_arena(int bytes, int device) -> Tensor", &vmm_arena);
  m.def("vmm_map_chunks(Tensor flat, int region_stride, int n_regions, int chunk_bytes, int first, "
        "int count, bool async_) -> bool", &vmm_map_chunks);
  m.def("vmm_chunks_ready(Tensor flat) -> int", &vmm_chunks_ready);
  m.def("vmm_error(Tensor flat) -> int", &vmm_error);
  m.def("gemm_rope_supported(int M, int N, int K) -> bool", &gemm_rope_supported);
  m.def("w4_chain_ok(int M, int N, int K) -> bool", &w4_chain_ok);
  m.def("chain_ok(int M, int N, int K, int epi) -> bool", &chain_ok);
  m.def("gemm_route(int M, int N, int K, int op, int n_groups=0, int rows_per_group=0) -> int[]", &gemm_route);
  m.def("gemm_route_env(int M, int N, int K, int op, int cus, bool sk, int n_groups=0, int rows_per_group=0) -> int[]", &gemm_route_env);
  m.def("gemm_tile_configs() -> int[]", &gemm_tile_configs);
  m.def("gemm_res_ss(Tensor(a!) residual, Tensor a, Tensor w, Tensor(b!) ss_out) -> bool");
  m.def("gemm_rs(Tensor(a!) out, Tensor a, Tensor w, Tensor ss_in, float eps, int epi) -> bool");
  m.def("gemm_rs_rope(Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor a, Tensor w, "
        "Tensor pos, Tensor cos_sin, Tensor slots, Tensor ss_in, float eps) -> bool");
  m.def("gemm_rope_cache(Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor a, Tensor w, "
        "Tensor pos, Tensor cos_sin, Tensor slots) -> bool");
  m.def("gemm(Tensor(a!) out, Tensor a, Tensor w, Tensor(b!) ws, int epi) -> ()");
  m.def("grouped_gemm(Tensor(a!) out, Tensor a, Tensor w, Tensor offsets, int max_rows, "
        "int epi, Tensor? a_rows=None) -> ()");
  m.def("gemm_add_rmsnorm(Tensor(a!) out, Tensor(b!) residual, Tensor a, Tensor w, Tensor norm_w, "
        "Tensor(c!) ws, float eps) -> bool");
  m.def("gemv_chain_supported(int M, int N, int K, int epi) -> bool", &gemv_chain_supported);
  m.def("moe_route(Tensor(a!) topw, Tensor(b!) topi, Tensor logits) -> ()");
  m.def("moe_permute(Tensor(a!) xp, Tensor(b!) offsets, Tensor(c!) src, Tensor(d!) inv, Tensor x, "
        "Tensor topi, int e0, int n_local) -> ()");
  m.def("moe_combine(Tensor(a!) out, Tensor y, Tensor inv, Tensor topw) -> ()");
  m.def("moe_dispatch_small(Tensor(a!) topw, Tensor(b!) topi, Tensor(c!) xp, Tensor(d!) offsets, Tensor(e!) src, "
        "Tensor(f!) inv, Tensor(g!) x, Tensor router_w, int e0, int n_local, Tensor? pro_y=None, "
        "Tensor(h!)? pro_res=None, Tensor? pro_w=None, float pro_eps=0.0) -> bool");
  m.def("moe_dispatch_mid(Tensor(a!) topw, Tensor(b!) topi, Tensor(c!) offsets, Tensor(d!) arow, Tensor(e!) inv, "
        "Tensor(f!) x, Tensor router_w, int e0, int n_local, Tensor? pro_y=None, Tensor(g!)? pro_res=None, "
        "Tensor? pro_w=None, float pro_eps=0.0) -> bool");
  m.def("moe_down_combine_add_rmsnorm(Tensor(a!) out, Tensor(b!) residual, Tensor(c!) y, Tensor a, Tensor w2, "
        "Tensor offsets, int max_rows, Tensor inv, Tensor topw, Tensor norm_w, float eps) -> bool");
  m.def("moe_combine_add_rmsnorm(Tensor(a!) out, Tensor(b!) residual, Tensor y, Tensor inv, Tensor topw, "
        "Tensor norm_w, float eps) -> bool");
  m.def("argmax(Tensor(a!) out, Tensor logits) -> ()");
  m.def("sample(Tensor(a!) out, Tensor logits, Tensor temps, Tensor top_ks, Tensor top_ps, "
        "Tensor uniform, bool full) -> ()");
  m.def("penalty_reset(Tensor(a!) table, int slot, int vocab, Tensor prompt_ids, Tensor output_ids) -> ()");
  m.def("penalty_update(Tensor(a!) table, int vocab, Tensor slots, Tensor tokens) -> ()");
  m.def("grammar_mask(Tensor(a!) logits, Tensor arena, Tensor base, Tensor rows, Tensor state) -> ()");
  m.def("grammar_advance(Tensor arena, int vocab, Tensor base, Tensor rows, Tensor(a!) state, Tensor tokens) -> ()");
  m.def("apply_penalties(Tensor(a!) logits, Tensor table, Tensor slots, Tensor rep, Tensor freq, "
        "Tensor pres) -> ()");
  m.def("token_logprobs(Tensor(a!) out_lp, Tensor(b!) out_id, Tensor logits, Tensor chosen, Tensor want) -> ()");
  m.def("spec_accept(Tensor sampled, Tensor q_start, Tensor drafts, Tensor nd, Tensor rows, Tensor(a!) hist, "
        "Tensor(b!) hist_len, Tensor(c!) out) -> ()");
  m.def("spec_propose(Tensor hist, Tensor hist_len, Tensor rows, Tensor cap, int n_max, int n_min, "
        "Tensor(a!) out) -> ()");
  m.def("pool_accumulate(Tensor(a!) acc, Tensor x, Tensor seg, int nseg) -> ()");
  m.def("pool_finish(Tensor(a!) out, Tensor acc, Tensor fin, int nfin) -> ()");
  m.def("rmsnorm(Tensor(a!) out, Tensor x, Tensor w, float eps) -> ()");
  m.def("add_rmsnorm(Tensor(a!) out, Tensor(b!) residual, Tensor x, Tensor w, float eps) -> ()");
  m.def("rope_cache(Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor qkv, "
        "Tensor pos, Tensor cos_sin, Tensor slots) -> ()");
  m.def("silu_mul(Tensor(a!) out, Tensor x, int interleaved=0) -> ()");
  m.def("lora_shrink(Tensor(a!) tmp, Tensor x, Tensor A, Tensor tok_slot, Tensor slot_rank, int R=16) -> ()");
  m.def("lora_expand_add(Tensor(a!) y, Tensor tmp, Tensor B, Tensor tile_group, Tensor tok_slot, "
        "Tensor slot_rank) -> ()");
  m.def("embedding(Tensor(a!) out, Tensor table, Tensor ids, int vocab_start) -> ()");
  m.def("gemm_ws(Tensor(a!) out, Tensor a, Tensor w, int epi, bool rs, float eps) -> bool");
  m.def("flash_prefill(Tensor(a!) out, Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_tables, "
        "Tensor ptile_seq, Tensor ptile_q0, Tensor q_start, Tensor q_len, Tensor ctx_len, float scale, "
        "int window=0) -> ()");
  m.def("paged_attention(Tensor(a!) out, Tensor(b!) part_o, Tensor(c!) part_ml, Tensor(d!) part_sem, Tensor q, "
        "Tensor k_cache, Tensor v_cache, Tensor block_tables, Tensor tile_seq, Tensor tile_q0, "
        "Tensor q_start, Tensor q_len, Tensor ctx_len, float scale, int part_tokens, "
        "int nparts, int window=0) -> ()");
  m.def("rope_cache_fp8(Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor(d!) k_scale, "
        "Tensor(e!) v_scale, Tensor qkv, Tensor pos, Tensor cos_sin, Tensor slots) -> ()");
  m.def("rope_cache_qkn(Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor qkv, Tensor pos, "
        "Tensor cos_sin, Tensor slots, Tensor q_w, Tensor k_w, float eps) -> ()");
  m.def("rope_cache_qkn_fp8(Tensor(a!) q_out, Tensor(b!) k_cache, Tensor(c!) v_cache, Tensor(d!) k_scale, "
        "Tensor(e!) v_scale, Tensor qkv, Tensor pos, Tensor cos_sin, Tensor slots, Tensor q_w, Tensor k_w, "
        "float eps) -> ()");
  m.def("paged_attention_fp8(Tensor(a!) out, Tensor(b!) part_o, Tensor(c!) part_ml, Tensor(d!) part_sem, Tensor q, "
        "Tensor k_cache, Tensor v_cache, Tensor k_scale, Tensor v_scale, Tensor block_tables, Tensor tile_seq, "
        "Tensor tile_q0, Tensor q_start, Tensor q_len, Tensor ctx_len, float scale, int part_tokens, "
        "int nparts) -> ()");
}

TORCH_LIBRARY_IMPL(mlop, CUDA, m) {
  m.impl("rmsnorm", &rmsnorm);
  m.impl("add_rmsnorm", &add_rmsnorm);
  m.impl("rope_cache", &rope_cache);
  m.impl("silu_mul", &silu_mul);
  m.impl("embedding", &embedding);
  m.impl("lora_shrink", &lora_shrink);
  m.impl("lora_expand_add", &lora_expand_add);
  m.impl("paged_attention", &paged_attention);
  m.impl("rope_cache_fp8", &rope_cache_fp8);
  m.impl("rope_cache_qkn", &rope_cache_qkn);
  m.impl("rope_cache_qkn_fp8", &rope_cache_qkn_fp8);
  m.impl("paged_attention_fp8", &paged_attention_fp8);
  m.impl("flash_prefill", &flash_prefill);
  m.impl("gemm", &gemm);
  m.impl("gemm_ws", &gemm_ws);
  m.impl("grouped_gemm", &grouped_gemm);
  m.impl("gemm_add_rmsnorm", &gemm_add_rmsnorm);
  m.impl("gemm_res_ss", &gemm_res_ss);
  m.impl("gemm_rs", &gemm_rs);
  m.impl("gemm_rs_rope", &gemm_rs_rope);
  m.impl("gemm_rope_cache", &gemm_rope_cache);
  m.impl("moe_route", &moe_route);
  m.impl("moe_dispatch_small", &moe_dispatch_small);
  m.impl("moe_dispatch_mid", &moe_dispatch_mid);
  m.impl("moe_down_combine_add_rmsnorm", &moe_down_combine_add_rmsnorm);
  m.impl("moe_combine_add_rmsnorm", &moe_combine_add_rmsnorm);
  m.impl("moe_permute", &moe_permute);
  m.impl("moe_combine", &moe_combine);
  m.impl("argmax", &argmax);
  m.impl("sample", &sample);
  m.impl("penalty_reset", &penalty_reset);
  m.impl("penalty_update", &penalty_update);
  m.impl("grammar_mask", &grammar_mask);
  m.impl("grammar_advance", &grammar_advance);
  m.impl("apply_penalties", &apply_penalties);
  m.impl("token_logprobs", &token_logprobs);
  m.impl("spec_accept", &spec_accept);
  m.impl("spec_propose", &spec_propose);
  m.impl("pool_accumulate", &pool_accumulate);
  m.impl("pool_finish", &pool_finish);
  m.impl("car_all_reduce", &car_all_reduce);
  m.impl("car_all_reduce_add", &car_all_reduce_add);
  m.impl("car_broadcast", &car_broadcast);
  m.impl("car_all_gather", &car_all_gather);
  m.impl("ep_dispatch", &ep_dispatch);
  m.impl("ep_combine", &ep_combine);
}
