"""Mixtral-8x7B (sparse MoE, top-2 of 8 experts) on the Llama attention stack.

MoE block (SURVEY.md §2.5 K11-K14 + CL4):
  router GEMM -> fused softmax/top-k/renormalise (K11) -> expert-sorted
  permutation (K12) -> grouped GEMM over all experts in ONE launch (K13,
  gate_up + SiLU-mul, then down) -> weighted un-permute/combine (K14).

Expert parallel: with ``ep > 1`` each rank owns E/ep experts; routed token
rows travel to their expert's rank with an all-to-all (dispatch) and back
(combine) over RCCL, see ``mlopamd.parallel.moe``.  Attention stays TP.
"""
from __future__ import annotations

import torch

from .. import ops
from .layers import linear
from .llama import LlamaModel


class MixtralModel(LlamaModel):
    # "mxfp4" after quantize_experts_mxfp4(): every layer's w13 / w2 are ops.Mx4Experts
    expert_weight_dtype = "bf16"

    def _init_mlp(self, w):
        cfg = self.cfg
        E, H, I = cfg.num_experts, cfg.hidden_size, cfg.intermediate_size
        ep = self.ps.ep.size
        assert E % ep == 0, "experts must divide by EP size"
        if E > 64 and (ep > 1 or self.ps.tp_size > 1):
            # the wide route (ops.moe_dispatch_wide) serves one rank; sharding it is not built
            raise ValueError(f"{cfg.name}: a model with more than 64 experts ({E}) is served on one GPU only "
                             f"(TP = {self.ps.tp_size}, EP = {ep} asked)")
        if E <= 64 and not cfg.norm_topk_prob:
            raise ValueError(f"{cfg.name}: norm_topk_prob = false needs the wide route (more than 64 experts)")
        self.n_local_experts = E // ep
        self.expert_start = self.ps.ep.rank * self.n_local_experts
        return {
            "router": w(E, H),
            "w13": w(self.n_local_experts, 2 * I, H),
            "w2": w(self.n_local_experts, H, I),
        }

    def _shard_mlp(self, L, F):
        e0, n = self.expert_start, self.n_local_experts
        L["router"].copy_(F["router"].to(self.device, self.dtype))
        L["w13"].copy_(F["w13"][e0:e0 + n].to(self.device, self.dtype))
        L["w2"].copy_(F["w2"][e0:e0 + n].to(self.device, self.dtype))

    @torch.no_grad()
    def quantize_experts_mxfp4(self) -> "MixtralModel":
        """Replace every layer's w13 / w2 by their MXFP4 form (ops.mx4_experts_quantize_pack: each
        expert through ref.mx4_quantize), one layer at a time, each bf16 tensor freed before the
        next is quantised.  Attention projections, router, embedding, LM head and norms stay bf16,
        so the layer keeps its fused QKV + RoPE and O paths; parallel.moe.local_experts sends the
        packed experts through ops.grouped_gemm_mx4."""
        if self.expert_weight_dtype == "mxfp4":
            return self
        cfg = self.cfg
        if self.ps.tp_size > 1 or self.ps.ep.size > 1:
            raise ValueError('expert_weight_dtype="mxfp4" needs tensor parallel size 1 and expert parallel size 1')
        if cfg.hidden_size % 128 or cfg.intermediate_size % 128:
            raise ValueError(f'expert_weight_dtype="mxfp4" needs hidden_size % 128 == 0 and intermediate_size % 128 '
                             f'== 0, not {cfg.hidden_size} / {cfg.intermediate_size} ({cfg.name})')
        largest = 0
        for L in self.layers:
            for name in ("w13", "w2"):
                largest = max(largest, L[name].numel())
                L[name] = ops.mx4_experts_quantize_pack(L[name])
        # the large-batch route dequantises one layer's w13 or w2 at a time into this scratch;
        # reserved here so that a graph capture never grows it
        self.q4_scratch_numel = largest
        ops.q4_reserve_scratch(self.device, largest)
        if self.device.type == "cuda":  # hand the freed bf16 blocks back: the KV pool is sized from free HBM
            torch.cuda.empty_cache()
        self.expert_weight_dtype = "mxfp4"
        return self

    def _folds(self):
        return (("in_norm", "qkv"),)  # post_norm feeds the router and the experts

    def _chain_ok(self, M: int) -> bool:
        return False  # the norm chain is the dense MLP's (gate_up / down on the four-wave kernel)

    def mlp(self, i: int, x: torch.Tensor) -> torch.Tensor:
        from ..parallel.moe import moe_forward

        L = self.layers[i]
        # TP attention (tokens replicated on the EP group): partial sums, summed by the
        # layer's TP all-reduce.  DP attention (tp == 1, ep > 1): all-to-all dispatch.
        mode = "alltoall" if (self.ps.ep.size > 1 and self.ps.tp.size == 1) else "allreduce"
        # all-to-all capacity: the group's agreed token count of this step (engine.EPSync)
        cap = getattr(self, "moe_capacity_tokens", None)
        return moe_forward(x, L["router"], L["w13"], L["w2"], self.cfg.top_k, self.ps.ep,
                           self.expert_start, self.n_local_experts, mode=mode,
                           cap_tokens=max(cap or 0, x.shape[0]), renorm=self.cfg.norm_topk_prob)

    def mlp_row_parallel(self, i, x, residual, next_norm, eps):
        """TP > 1 (experts sharded over the TP ranks): each rank's partial MoE output, summed by
        the TP all-reduce, then the next residual add / norm."""
        m = self.mlp(i, x)
        self.ps.tp.all_reduce(m)
        return ops.add_rmsnorm(m, residual, next_norm, eps)

    def mlp_add_norm(self, i, x, residual, next_norm, eps):
        """TP = EP = 1: MoE block + the next residual add / norm (decode-size dispatch in one
        launch, combine fused into the norm: parallel.moe.moe_forward_add_norm)."""
        if self.ps.ep.size == 1:
            from ..parallel.moe import moe_forward_add_norm

            L = self.layers[i]
            return moe_forward_add_norm(x, L["router"], L["w13"], L["w2"], self.cfg.top_k, self.expert_start,
                                        self.n_local_experts, residual, next_norm, eps,
                                        renorm=self.cfg.norm_topk_prob)
        return ops.add_rmsnorm(self.mlp(i, x), residual, next_norm, eps)

    def attn_out_mlp(self, i, a, residual, next_norm, eps):
        """TP = EP = 1 decode sizes: O projection GEMV, then ONE launch for residual add +
        post-attention RMSNorm + router + route + sort + gather (moe_dispatch_small's
        prologue), the two grouped GEMMs, and the combine fused into the next add + norm.
        More than 64 experts: the add + norm is a launch of its own before the wide dispatch."""
        if self.ps.ep.size == 1 and a.is_cuda and a.shape[0] <= 16:
            from ..parallel.moe import moe_forward_add_norm

            L = self.layers[i]
            o = linear(a, L["o"])
            return moe_forward_add_norm(None, L["router"], L["w13"], L["w2"], self.cfg.top_k, self.expert_start,
                                        self.n_local_experts, residual, next_norm, eps, pre=(o, L["post_norm"]),
                                        renorm=self.cfg.norm_topk_prob)
        return super().attn_out_mlp(i, a, residual, next_norm, eps)

