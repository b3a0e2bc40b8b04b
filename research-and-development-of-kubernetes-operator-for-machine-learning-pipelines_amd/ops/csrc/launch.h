// Host-side launchers of the gfx950 kernels (raw pointers + stream; no torch
// headers here so the .hip files compile quickly).  Bound to torch in bindings.cpp.
#pragma once

#include <string>
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <memory>

namespace mlop {

void launch_rmsnorm(void* out, const void* x, const void* w, float eps, int M, int H,
                    hipStream_t st);
void launch_add_rmsnorm(void* out, void* residual, const void* x, const void* w, float eps, int M,
                        int H, hipStream_t st);
void launch_rope_cache(void* q_out, void* k_cache, void* v_cache, const void* qkv, const int* pos,
                       const float* cos_sin, const int* slots, int T, int Hq, int Hkv, int D,
                       int qkv_stride, int BS, hipStream_t st);
void launch_silu_mul(void* out, const void* x, int M, int I, int interleaved, hipStream_t st);
void launch_device_delay(long long ticks, hipStream_t st);
// lora.hip: per-token low-rank update (multi-LoRA)
void launch_lora_shrink(const void* x, int ldx, const void* A, float* tmp, const int* tok_slot,
                        const int* slot_rank, int T, int K, int GR, int R, int S, hipStream_t st);
void launch_lora_expand_add(void* y, int ldy, const float* tmp, const void* B, const uint8_t* tile_group,
                            const int* tok_slot, const int* slot_rank, int T, int N, int GR, int R, int S,
                            hipStream_t st);
void launch_embedding(void* out, const void* table, const long* ids, int T, int H, long vocab_start,
                      long vocab_end, hipStream_t st);
void launch_paged_attention(void* out, float* part_o, float* part_ml, const void* q,
                            const void* kc, const void* vc, const int* bt, int bt_stride,
                            const int* tile_seq, const int* tile_q0, const int* q_start,
                            const int* q_len, const int* ctx_len, int num_tiles, int Hq, int Hkv,
                            float scale_log2, int part_tokens, int nparts, int num_blocks,
                            int* sem, int window, hipStream_t st);  // window 0: causal only
// fp8 KV cache (e4m3fn pages [NB, Hkv, 16, 128] + one power-of-two scale byte per row,
// [NB, Hkv, 16]): kv_fp8.hip's RoPE + cache writer and attention.hip's decode kernel over KvFp8
void launch_rope_cache_fp8(void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                           const void* qkv, const int* pos, const float* cos_sin, const int* slots, int T,
                           int Hq, int Hkv, int qkv_stride, int BS, hipStream_t st);
// rope_cache_qkn.hip: the two stand-alone writers with a per-head RMSNorm (weights q_w / k_w, bf16
// [128]) on every q and k head before the rotation (Qwen3); head_dim 128, layouts as above
void launch_rope_cache_qkn(void* q_out, void* k_cache, void* v_cache, const void* qkv, const int* pos,
                           const float* cos_sin, const int* slots, int T, int Hq, int Hkv, int qkv_stride,
                           int BS, const uint16_t* q_w, const uint16_t* k_w, float eps, hipStream_t st);
void launch_rope_cache_qkn_fp8(void* q_out, void* k_cache, void* v_cache, void* k_scale, void* v_scale,
                               const void* qkv, const int* pos, const float* cos_sin, const int* slots, int T,
                               int Hq, int Hkv, int qkv_stride, int BS, const uint16_t* q_w,
                               const uint16_t* k_w, float eps, hipStream_t st);
void launch_paged_attention_fp8(void* out, float* part_o, float* part_ml, const void* q, const void* kc,
                                const void* vc, const void* ks, const void* vs, const int* bt,
                                int bt_stride, const int* tile_seq, const int* tile_q0, const int* q_start,
                                const int* q_len, const int* ctx_len, int num_tiles, int Hq, int Hkv,
                                float scale_log2, int part_tokens, int nparts, int num_blocks, int* sem,
                                hipStream_t st);
int flash_persist(int set);  // 0: one workgroup per flash item; n: persistent grid, n per CU
int flash_stream(int set);   // 1: the persistent grid streams K / V pairs and Q across tiles
int gemm_grouped_balance(int set);  // 1: equal row ranges per expert m-tile; 2: + the 16-row MFMA skip
int gemm_grouped_order(int set);    // grouped tile order: 0 slot fastest, 1 expert-major, 2 auto
int moe_mid_tok(int set);            // tokens per workgroup of the mid MoE dispatch: 0 = by T, 2, 4, 8
void launch_flash_prefill(void* out, const void* q, const void* kc, const void* vc, const int* bt,
                          int bt_stride, const int* ptile_seq, const int* ptile_q0,
                          const int* q_start, const int* q_len, const int* ctx_len, int num_ptiles,
                          int Hq, int Hkv, float scale_log2, int num_blocks, int window, hipStream_t st);
// QKV projection epilogue (EPI_ROPE): the GEMM's C tile is [q heads | k heads | v heads]
// of head_dim 128; q/k are rotated (HF rotate-half, cos/sin table [max_pos, 128]) and
// q goes to q_out [T, Hq, 128], k / v into the paged cache (k [NB, Hkv, BS, 128],
// v [NB, Hkv, 128, BS]; slot < 0 = padding row, no cache write) - rope_cache.hip's
// layout, done from the GEMM's LDS-staged tile instead of a [T, N] round trip.
struct RopeEpi {
  uint16_t* q_out;
  uint16_t* k_cache;
  uint16_t* v_cache;
  const int* pos;
  const float* cos_sin;
  const int* slots;
  int Hq, Hkv, BS;
  // four-wave norm chain (run_w4 only; the large-M TP=1 decoder with unit norm weights, see
  // launch_gemm_chain).  Producer (C += A.B^T): ss_out = [M, N / 128] partial sums of squares of
  // the updated residual rows (one per row and wave column block), then ss_tot [M] = their row
  // sums, added in a fixed order by the last tile of each 256-row band (ss_cnt: one ticket per
  // band).  Consumer: ss_in = a producer's ss_tot; the accumulators of row r are scaled by
  // rsqrt(ss_in[r] * ss_inv_k + ss_eps) = RMSNorm applied after the GEMM.
  const float* ss_in = nullptr;
  float* ss_out = nullptr;
  float* ss_tot = nullptr;
  int* ss_cnt = nullptr;
  float ss_inv_k = 0.f, ss_eps = 0.f;
  // grouped GEMM: A row of permuted row r is a_rows[r] (moe_dispatch_mid: the experts read the
  // token rows in place, no gathered copy); nullptr = row r
  const int* a_rows = nullptr;
  // gemm_kernel: the weight (B) pieces of the LDS-DMA ring load non-temporal (read once by one
  // workgroup: MI355X_MICROARCH.md "nt-weights"); set by run_cfg (gemm_small_nt)
  int b_nt = 0;
  // gemm_kernel: split-K slabs stored non-temporal (not left dirty in L2 for the kernel boundary's
  // write-back; MI355X_MICROARCH.md "boundary"); set by run_cfg (gemm_slab_nt)
  int ws_nt = 0;
  // mid norm chain (gemm.hip mid_chain_finish): 1 = the finishing split reads the partials with
  // plain loads behind one agent acquire, 0 = with sc1 loads only (gemm_mid_chain op 2 / 1)
  int mid_acq = 0;
};
// RoPE + paged-cache stores from the QKV projection's fp32 split-K slabs ws[splits][T][N] (the
// split-K reduce fused in: small-M launch_gemm_rope)
void launch_rope_cache_slabs(const RopeEpi& re, const float* ws, int splits, int T, int N, hipStream_t st);
// The GEMM planner's knobs, predicates and queries (gemm_big_variant, gemm_dense_plan, gemv_takes,
// gemm_rope_supported, w4_chain_ok, ...) are declared in gemm_plan.h.
bool gemm_sk_scratch(float** ws, int** cnt, int* cus);
bool gemm_sk_available(int* cus);
bool run_w4(int epi, const uint16_t* A, int lda, const uint16_t* B, int ldb, uint16_t* C, int ldc, int M, int N,
            int K, hipStream_t st, const RopeEpi& re, int bm = 256);
// one GEMM of the norm chain (op: gemm_plan.h OP_CHAIN_*; epi flags of the four-wave form: 4 = C +=
// A.B^T with ss partials, 8 = rows scaled by ss; 4, 0|8, 1|8, 3|8 are built), on the form the
// planner names for its row count; false = refused, nothing launched
bool launch_gemm_chain(int op, const void* A, int lda, const void* B, void* C, int ldc, int M, int N, int K,
                       const RopeEpi& rope, float* ss, float eps, hipStream_t st);
// non-temporal weight loads of the one-m-tile gemm_kernel launches: bit 0 dense, bit 1 grouped,
// bit 2 the grouped ping-pong kernel
int gemm_small_nt(int set);
// non-temporal K / V page loads of the decode attention kernel
int attn_kv_nt(int set);
int gemm_slab_nt(int set);
// the stream-K scratch of the ping-pong GEMM's tail (and of every other split-K slab / ticket
// user): per-device partial / counter buffers (allocate once, outside graph capture)
bool gemm_sk_reserve();
// K2 skinny GEMV (gemv.hip): decode projections at M <= 8 (epi 0 none, 1 silu-mul, 3 rope)
void launch_gemv(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                 int epi, hipStream_t st);
void launch_gemv_rope(const void* A, int lda, const void* B, int M, int N, int K, const RopeEpi& re,
                      hipStream_t st);
// the decode norm chain's row-scale prologue parameters (gemv.hip PRO_RS)
struct NormPro {
  float eps = 0.f;
};
// decode norm chain (gemv.hip PRO_RS / EPI_RES, M <= 4): C = epi(rowscale(A) . B^T) with
// rowscale = rsqrt(mean(A_row^2) + eps) (norm weights folded into B); residual += A . B^T
// weight-streaming MFMA GEMM (gemm_ws.hip) at gemv_chain_max_m < M <= gemm_ws_max_m (64):
// epi 0 plain, 1 SiLU-mul, 3 RoPE + paged K/V (re), 5 residual += (C in place); rs: A is the raw
// residual, rows scaled by rsqrt(mean(a^2) + eps) (norm weights folded into B)
void gemm_ws_plan(int rb, int u, int nt);
void launch_ws(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K, int epi,
               bool rs, const RopeEpi& re, float eps, hipStream_t st);
void launch_gemv_rs(const void* A, int lda, const void* B, void* C, int ldc, int M, int N, int K, int epi,
                    const RopeEpi& re, float eps, hipStream_t st);
void launch_gemv_res(const void* A, int lda, const void* B, void* residual, int M, int N, int K, hipStream_t st);
void launch_gemv_grouped(const void* A, const void* B, void* C, const int* offsets, int n_groups, int M, int N,
                         int K, int epi, hipStream_t st);
bool launch_gemm_rope(const void* A, int lda, const void* B, int M, int N, int K, const RopeEpi& re,
                      hipStream_t st);
void launch_gemm(const void* A, int lda, const void* B, int ldb, void* C, int ldc, float* ws,
                 long ws_floats, int M, int N, int K, int epi, hipStream_t st);
bool launch_gemm_add_rmsnorm(const void* A, int lda, const void* B, void* out, void* residual,
                             const void* w, float eps, float* ws, long ws_floats, int M, int N,
                             int K, hipStream_t st);
void launch_grouped_gemm(const void* A, const void* B, void* C, const int* offsets, int n_groups,
                         int M, int N, int K, int max_rows, int epi, hipStream_t st, const int* a_rows = nullptr,
                         float** defer_ws = nullptr, int* defer_splits = nullptr);
bool launch_moe_down_combine_add_rmsnorm(void* out, void* residual, void* y, const void* a, const void* w2,
                                         const int* offsets, int n_groups, int R, int H, int I, int max_rows,
                                         const int* inv, const float* topw, const void* norm_w, float eps, int T,
                                         int k, hipStream_t st);
// mid-size MoE dispatch (16 < T <= 16384 tokens): router GEMV + route per token workgroup, the last
// workgroup (agent-scope ticket) sorts the T*k slots by local expert -> offsets, inv and arow (the
// token row of each permuted row: the grouped GEMM reads x through it, no gather)
bool moe_dispatch_mid_takes(int T, int E, int k, int H);
int moe_mid_max_tokens(int set);
void launch_moe_dispatch_mid(float* topw, int* topi, int* offsets, int* arow, int* inv, const void* x, const void* wr,
                             int T, int E, int k, int H, int e0, int n_local, const void* pro_y, void* pro_res,
                             const void* pro_w, float pro_eps, void* pro_xn, hipStream_t st);
void launch_moe_route(float* topw, int* topi, const void* logits, int T, int E, int k,
                      hipStream_t st);
void launch_moe_permute(void* xp, int* offsets, int* src, int* inv, const void* x, const int* topi,
                        int T, int k, int H, int e0, int n_local, hipStream_t st);
void launch_moe_combine(void* out, const void* y, const int* inv, const float* topw, int T, int k,
                        int H, hipStream_t st);
// decode-size MoE dispatch in one launch: router GEMV + route + sort + gather (moe.hip)
bool moe_dispatch_small_takes(int T, int E, int k, int H);
// pro_y != nullptr: prologue residual += pro_y, x = rmsnorm(residual) * pro_w (written to pro_xn)
void launch_moe_dispatch_small(float* topw, int* topi, void* xp, int* offsets, int* src, int* inv, const void* x,
                               const void* wr, int T, int E, int k, int H, int e0, int n_local, const void* pro_y,
                               void* pro_res, const void* pro_w, float pro_eps, void* pro_xn, hipStream_t st);
// combine + residual add + RMSNorm in one launch; false = hidden size not instantiated
bool launch_moe_combine_add_rmsnorm(void* out, void* residual, const void* y, const int* inv, const float* topw,
                                    const void* w, float eps, int T, int k, int H, hipStream_t st);
void launch_argmax(long* out, const float* logits, int n, int V, long ld, hipStream_t st);
// bf16 greedy argmax; ws (>= argmax_splits(n, V) * n int64, or null) splits small batches' rows
int argmax_splits(int n, int V);
void launch_argmax_bf16(long* out, const void* logits, int n, int V, long ld, void* ws, hipStream_t st);
// temperature / top-k / top-p draw; small batches pre-select per-slice top-K candidates into ws
// (sample_workspace_bytes(n, V) bytes, 0 = not needed)
long sample_workspace_bytes(int n, int V);
void launch_sample(long* out, const float* logits, int n, int V, long ld, const float* temps,
                   const int* top_ks, const float* top_ps, const float* uniform, void* ws, bool full,
                   hipStream_t st);
// sampler extensions (sampling_ext.hip).  Count table int32 [nslots, ldt >= V] (ldt % 4 == 0): bit 31 =
// in the prompt, bits 0..30 = occurrences in the output
void launch_penalty_reset(int* row, int V, int ldt, const long* prompt, int np, const long* output, int no,
                          hipStream_t st);
void launch_penalty_update(int* table, long ldt, int V, int nslots, const int* slots, const long* tokens, int n,
                           hipStream_t st);
void launch_apply_penalties(float* logits, int n, int V, long ld, const int* table, long ldt, int nslots,
                            const int* slots, const float* rep, const float* freq, const float* pres,
                            hipStream_t st);
// log-softmax at `chosen` (column 0) and of the top want[i] <= 20 logits (columns 1..) of bf16 / fp32 rows;
// logprob_splits = 0: the vocabulary is too large; ws: logprob_workspace_bytes(n, V) bytes
int logprob_splits(int n, int V);
long logprob_workspace_bytes(int n, int V);
void launch_token_logprobs(float* out_lp, int* out_id, int ldo, const void* logits, bool bf16, int n, int V,
                           long ld, const long* chosen, const int* want, void* ws, hipStream_t st);
// guided decoding (guided.hip).  Arena int16 [A, ldv >= V] (ldv % 8 == 0): entry [base + s, t] = the
// grammar's state after token t in state s, < 0 = not allowed; state int32 [R] by engine row
void launch_grammar_mask(float* logits, int n, int V, long ld, const short* arena, long ldv, int A,
                         const int* base, const int* rows, const int* state, int R, hipStream_t st);
void launch_grammar_advance(const short* arena, long ldv, int A, int V, const int* base, const int* rows,
                            int* state, int R, const long* tokens, int n, hipStream_t st);
// speculative decoding by prompt lookup (spec.hip).  hist int32 [R, ld >= max_len], hist_len [R];
// out int32 [B, 3 + 2k] = [emitted count, next draft count, k + 1 emitted, k next drafts]
void launch_spec_accept(const long* sampled, int T, const int* q_start, const int* drafts, const int* nd,
                        const int* rows, int* hist, long ld, int max_len, int* hist_len, int R, int* out, int k,
                        int B, hipStream_t st);
void launch_spec_propose(const int* hist, long ld, int max_len, const int* hist_len, int R, const int* rows,
                         const int* cap, int n_max, int n_min, int* out, int k, int B, hipStream_t st);
// embedding pooling (pool.hip).  seg int32 [nseg, 4] = [r0, r1, slot, flags] over the rows of x[T, ldx] (bf16),
// acc fp32 [S, H]; fin int32 [nfin, 4] = [slot, count, d, flags], out fp32 [S, ldo >= H]; H % 8 == 0
constexpr int kPoolInit = 1, kPoolLast = 2, kPoolModeLast = 4;  // segment flags
constexpr int kPoolFinNormalize = 1, kPoolFinMean = 2;          // finish flags
void launch_pool_accumulate(float* acc, const void* x, long ldx, const int* seg, int nseg, int T, int H, int S,
                            hipStream_t st);
void launch_pool_finish(float* out, long ldo, const float* acc, const int* fin, int nfin, int H, int S,
                        hipStream_t st);

// lazily backed KV arenas (vmm.hip): reserve VA, back chunks synchronously or on a native
// worker thread; the returned owner must outlive every use of the range
bool vmm_supported(int device);
long vmm_granularity(int device);
std::shared_ptr<void> vmm_reserve(long bytes, int device, void** base_out, long* reserved_out);
void vmm_forget(void* base);
bool vmm_map_chunks(void* base, long region_stride, int n_regions, long chunk_bytes, long first, long count,
                    bool async);
long vmm_chunks_ready(void* base);
int vmm_error(void* base);

// K15 custom one-shot all-reduce (allreduce.hip); handles are opaque state pointers
long car_create(int rank, int world, long max_bytes, int device, int split);
void car_ipc_handle(long h, void* out128);
void car_open(long h, const void* handles);
long car_max_bytes(long h);
// add_out: out = bf16(out + bf16(sum)) (the residual stream; one-shot only, out != in)
void car_all_reduce(long h, void* out, const void* in, long numel, hipStream_t st, bool two_shot = false,
                    bool add_out = false);
void car_broadcast(long h, void* out, const void* in, long nbytes, int root, hipStream_t st);
void car_all_gather(long h, void* out, long out_bytes, const void* in, long nbytes, hipStream_t st);
int car_error(long h);
int car_mem_mode(long h);
void car_destroy(long h);

// host-to-host step-header channel over POSIX shared memory (shm_channel.cc, host code)
long chan_create(const std::string& name, int nslots, int nconsumers);
long chan_open(const std::string& name);
bool chan_send(long h, const int64_t* w, int n, long timeout_us);
bool chan_recv(long h, int consumer, int64_t* w, int n, long timeout_us);
void chan_unlink(const std::string& name);
void chan_close(long h, bool unlink);
long xg_create(const std::string& name, int world, int nslots, long max_words);
long xg_open(const std::string& name, int rank);
long xg_max_words(long h);
bool xg_exchange(long h, const int64_t* in, long n, int64_t* out, int64_t* counts, long timeout_us);
void xg_close(long h);

// expert-parallel dispatch / combine over IPC peer memory (ep_exchange.hip)
long ep_create(int rank, int world, int E, int k, int H, int tcap, int device);
void ep_ipc_handle(long h, void* out64);
void ep_open(long h, const void* handles);
int ep_mem_mode(long h);
int ep_world(long h);
int ep_local_experts(long h);
int ep_hidden(long h);
int ep_topk(long h);
int ep_tcap(long h);
void ep_dispatch(long h, void* xp, long xp_rows, int* offsets, const void* x, const int* topi, int T, hipStream_t st);
void ep_combine(long h, void* out, const void* y, long y_rows, const float* topw, const int* topi, int T,
                hipStream_t st);
int ep_error(long h);
void ep_destroy(long h);

}  // namespace mlop
