"""Multi-LoRA adapter storage for the dense Llama / Mistral models (TP = 1).

One base model, N adapters, one batch: every token of a ragged step names a slot of the
slot-major stacks below (or -1 for the base model) and ``LlamaModel.forward(..., lora=step)``
adds ``B[slot] . (A[slot] . x)`` after each projection (``ops.lora_shrink`` /
``ops.lora_expand_add``, ops/csrc/lora.hip).

Per layer and per fused projection of ours (``qkv``, ``o``, ``gate_up``, ``down``):

  A [S, G * R, K]   the G sub-projections sharing the input (q / k / v: 3, gate / up: 2), R rows each
  B [S, N, R]       in the base weight's row layout ([q; k; v], gate_up interleaved in groups of
                    16), scaling folded in (fp32 product, one rounding to the model dtype)
  tile_group [N/16] which A block each 16-column output tile reads

``S = max_adapters`` slots, ``R = max_lora_rank`` rounded up to 16.  Rows of smaller ranks and of
modules an adapter does not target are zero; ``slot_rank[S]`` lets the kernels skip them.  The
stacks are allocated once: loading an adapter copies into a slot in place, so decode graphs
that captured the pointers stay valid.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .config import ModelConfig

# our fused projection -> the PEFT target modules stacked in it (A block order)
PROJ_MODULES = {"qkv": ("q_proj", "k_proj", "v_proj"), "o": ("o_proj",),
                "gate_up": ("gate_proj", "up_proj"), "down": ("down_proj",)}
TARGET_MODULES = tuple(m for ms in PROJ_MODULES.values() for m in ms)
MAX_LORA_RANK = 64
# the RMSNorm weight fold_norms() folds into each projection's input columns (A needs it too)
PROJ_NORM = {"qkv": "in_norm", "gate_up": "post_norm"}


def module_shapes(cfg: ModelConfig) -> dict:
    """PEFT module name -> (out_features, in_features) of the base model."""
    H, I = cfg.hidden_size, cfg.intermediate_size
    return {"q_proj": (cfg.q_size, H), "k_proj": (cfg.kv_size, H), "v_proj": (cfg.kv_size, H),
            "o_proj": (H, cfg.q_size), "gate_proj": (I, H), "up_proj": (I, H), "down_proj": (H, I)}


@dataclass
class Adapter:
    """One adapter on the host, already in our layout: per layer, ``proj -> (A [G, r, K] fp32,
    B [N, r] fp32 with the scaling applied)`` for the projections it targets."""
    rank: int
    layers: list
    target_modules: tuple = ()
    digest: bytes = b""  # content hash of the adapter's files (prefix-cache identity)
    path: str | None = None


@dataclass
class LoraStep:
    """What one forward needs: the per-layer stacks and this step's slot per token."""
    layers: list
    slot_rank: torch.Tensor
    tok_slot: torch.Tensor


def tile_group_of(cfg: ModelConfig, proj: str, n_rows: int) -> torch.Tensor:
    nt = n_rows // 16
    if proj == "qkv":
        q, kv = cfg.q_size // 16, cfg.kv_size // 16
        return torch.cat([torch.zeros(q), torch.ones(kv), torch.full((kv,), 2.0)]).to(torch.uint8)
    if proj == "gate_up":
        return (torch.arange(nt) & 1).to(torch.uint8)
    return torch.zeros(nt, dtype=torch.uint8)


def check_shapes(cfg: ModelConfig) -> None:
    """The kernels' contract (K % 128, N % 16), checked when adapters are enabled / loaded."""
    for m, (n, k) in module_shapes(cfg).items():
        if k % 128 or n % 16:
            raise ValueError(f"LoRA needs in_features % 128 == 0 and out_features % 16 == 0; {m} is [{n}, {k}]")


class LoraStacks:
    def __init__(self, model, max_adapters: int, max_rank: int = MAX_LORA_RANK):
        cfg = model.cfg
        if cfg.is_moe:
            raise ValueError("LoRA adapters are served on dense Llama / Mistral models only (not Mixtral)")
        if model.ps.tp.size > 1 or model.ps.ep.size > 1:
            raise ValueError("LoRA adapters need TP = 1 and EP = 1 (sharding adapters is not implemented)")
        if not 1 <= max_rank <= MAX_LORA_RANK:
            raise ValueError(f"max_lora_rank must be in [1, {MAX_LORA_RANK}]")
        check_shapes(cfg)
        self.model, self.S = model, int(max_adapters)
        self.max_rank = int(max_rank)
        self.R = R = (self.max_rank + 15) // 16 * 16
        dev, dt = model.device, model.dtype
        self.layers = []
        for L in model.layers:
            st = {}
            for proj, mods in PROJ_MODULES.items():
                N, K = L[proj].shape
                st[proj] = (torch.zeros(self.S, len(mods) * R, K, dtype=dt, device=dev),
                            torch.zeros(self.S, N, R, dtype=dt, device=dev),
                            tile_group_of(cfg, proj, N).to(dev), len(mods))
            self.layers.append(st)
        self.slot_rank = torch.zeros(self.S, dtype=torch.int32, device=dev)

    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for st in self.layers for a, b, *_ in st.values() for t in (a, b))

    @torch.no_grad()
    def load(self, slot: int, ad: Adapter) -> None:
        """Copy an adapter into ``slot`` (in place, on the current stream).  The RMSNorm weights
        that ``fold_norms`` moved into qkv / gate_up are folded into the matching A columns."""
        if ad.rank > self.max_rank:
            raise ValueError(f"adapter rank {ad.rank} exceeds max_lora_rank {self.max_rank}")
        if len(ad.layers) != len(self.layers):
            raise ValueError("adapter and model disagree on the number of layers")
        m, R, r = self.model, self.R, ad.rank
        folded = getattr(m, "folded_norms", None)
        for i, (st, src) in enumerate(zip(self.layers, ad.layers)):
            for proj, (A, B, _, G) in st.items():
                A[slot].zero_()
                B[slot].zero_()
                if proj not in src:
                    continue
                a, b = src[proj]  # [G, r, K], [N, r] fp32
                if folded is not None and proj in PROJ_NORM:
                    a = a * folded[i][PROJ_NORM[proj]].float().cpu()[None, None, :]
                A[slot].view(G, R, -1)[:, :r].copy_(a.to(A.dtype))
                B[slot][:, :r].copy_(b.to(B.dtype))
        self.slot_rank[slot] = r

    @torch.no_grad()
    def clear(self, slot: int) -> None:
        for st in self.layers:
            for A, B, *_ in st.values():
                A[slot].zero_()
                B[slot].zero_()
        self.slot_rank[slot] = 0

    def step(self, tok_slot: torch.Tensor) -> LoraStep:
        return LoraStep(self.layers, self.slot_rank, tok_slot)


@torch.no_grad()
def merged_copy(model, ad: Adapter):
    """A deep copy of ``model`` with ``W + B . A`` merged into every targeted projection, in our
    layout (the oracle of the LoRA tests; also the offline alternative to serving an adapter)."""
    import copy

    m = copy.copy(model)
    m.layers = [dict(L) for L in model.layers]
    folded = getattr(model, "folded_norms", None)
    cfg = model.cfg
    for i, (L, src) in enumerate(zip(m.layers, ad.layers)):
        for proj, (a, b) in src.items():
            a = a.to(L[proj].device)
            b = b.to(L[proj].device)
            if folded is not None and proj in PROJ_NORM:
                a = a * folded[i][PROJ_NORM[proj]].float()[None, None, :]
            # the values a slot serves: A and B rounded to the model dtype
            a, b = a.to(L[proj].dtype).float(), b.to(L[proj].dtype).float()
            W = L[proj].float().clone()
            tg = tile_group_of(cfg, proj, W.shape[0]).long().repeat_interleave(16).to(W.device)
            for g in range(a.shape[0]):
                rows = torch.nonzero(tg == g, as_tuple=True)[0]
                W[rows] += b[rows] @ a[g]
            L[proj] = W.to(L[proj].dtype)
    return m
