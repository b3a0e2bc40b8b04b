"""Model architecture configs (random-init; shapes of the public checkpoints).

Llama-3 shapes: public HF ``config.json`` of meta-llama/Meta-Llama-3-8B / -70B
(rope_theta 5e5; Llama-3.1 adds the "llama3" rope scaling, kept optional here).
Mixtral-8x7B: transformers ``MixtralConfig`` defaults (SURVEY.md §2.5 model table).
"""
from __future__ import annotations

from dataclasses import asdict, dataclass, field, replace

# kv_cache_dtype -> (bytes per cached element, scale bytes per (token, kv head) row of K and of V)
KV_CACHE_DTYPE_BYTES = {"bf16": (2, 0), "fp8": (1, 1)}


def kv_dtype_bytes(name: str) -> tuple[int, int]:
    if name not in KV_CACHE_DTYPE_BYTES:
        raise ValueError(f"kv_cache_dtype must be one of {sorted(KV_CACHE_DTYPE_BYTES)}, not {name!r}")
    return KV_CACHE_DTYPE_BYTES[name]


@dataclass(frozen=True)
class ModelConfig:
    name: str
    vocab_size: int
    hidden_size: int
    intermediate_size: int
    num_layers: int
    num_heads: int
    num_kv_heads: int
    head_dim: int = 128
    rope_theta: float = 500000.0
    rms_eps: float = 1e-5
    max_position: int = 8192
    tie_embeddings: bool = False
    # MoE (Mixtral): 0 experts = dense MLP
    num_experts: int = 0
    top_k: int = 2
    rope_scaling: dict | None = field(default=None, hash=False, compare=False)
    eos_token_id: int = 128001
    # further end-of-sequence ids (HF eos_token_id lists, e.g. Llama-3.1-Instruct's
    # [128001, 128008, 128009]: <|eot_id|> must stop generation too)
    extra_eos_ids: tuple = field(default=(), hash=False, compare=False)
    # sliding-window attention (Mistral): the query at position i attends the keys
    # i - W < j <= i on every layer; 0 = full causal attention
    sliding_window: int = 0
    # per-head QK-norm (Qwen3): an RMSNorm with a learned [head_dim] weight on every q head and
    # every k head between the QKV projection and RoPE (layer weights "q_norm" / "k_norm")
    qk_norm: bool = False
    # a base-model checkpoint (LlamaModel / MistralModel / Qwen3Model: no LM head; ours is tied to the
    # embedding table and never asked): it serves embedding requests only.  embed_pooling /
    # embed_normalize: the request defaults a checkpoint's sentence-transformers settings name
    # (embed_pooling None: they name a pooling this runtime does not serve, a request must name its own)
    embedding_only: bool = field(default=False, compare=False)
    embed_pooling: str | None = field(default="last", compare=False)
    embed_normalize: bool = field(default=True, compare=False)

    @property
    def eos_ids(self) -> tuple:
        return (self.eos_token_id, *self.extra_eos_ids)

    @property
    def is_moe(self) -> bool:
        return self.num_experts > 0

    @property
    def q_size(self) -> int:
        return self.num_heads * self.head_dim

    @property
    def kv_size(self) -> int:
        return self.num_kv_heads * self.head_dim

    def num_params(self) -> int:
        H, I, V, L = self.hidden_size, self.intermediate_size, self.vocab_size, self.num_layers
        attn = H * (self.q_size + 2 * self.kv_size) + self.q_size * H
        mlp = 3 * H * I * (self.num_experts if self.is_moe else 1)
        router = H * self.num_experts if self.is_moe else 0
        norms = 2 * H + (2 * self.head_dim if self.qk_norm else 0)
        emb = V * H * (1 if self.tie_embeddings else 2)
        return L * (attn + mlp + router + norms) + emb + H

    def active_params(self) -> int:
        if not self.is_moe:
            return self.num_params()
        dense = replace(self, num_experts=0)
        extra = self.num_layers * 3 * self.hidden_size * self.intermediate_size * (self.top_k - 1)
        return dense.num_params() + extra + self.num_layers * self.hidden_size * self.num_experts

    def weight_bytes(self, dtype_bytes: int = 2) -> int:
        return self.num_params() * dtype_bytes

    def kv_bytes_per_token(self, dtype_bytes: int = 2, kv_cache_dtype: str | None = None) -> int:
        """KV cache bytes of one token over all layers.  ``kv_cache_dtype`` ("bf16" / "fp8"): the
        engine's cache format, its per-row scale bytes included (it overrides ``dtype_bytes``)."""
        scale_bytes = 0
        if kv_cache_dtype is not None:
            dtype_bytes, scale_bytes = kv_dtype_bytes(kv_cache_dtype)
        return 2 * self.num_layers * (self.kv_size * dtype_bytes + self.num_kv_heads * scale_bytes)

    def flops_per_token(self) -> int:
        """Matmul FLOPs of one forward token (2 * active params, attention excluded)."""
        return 2 * self.active_params()

    def to_dict(self) -> dict:
        return asdict(self)


LLAMA3_8B = ModelConfig(
    name="llama3-8b", vocab_size=128256, hidden_size=4096, intermediate_size=14336,
    num_layers=32, num_heads=32, num_kv_heads=8, rope_theta=500000.0, max_position=8192)

LLAMA3_70B = ModelConfig(
    name="llama3-70b", vocab_size=128256, hidden_size=8192, intermediate_size=28672,
    num_layers=80, num_heads=64, num_kv_heads=8, rope_theta=500000.0, max_position=8192)

# Llama-3.1: same shapes, 128k context through the "llama3" RoPE frequency scaling
# (public HF config.json of meta-llama/Llama-3.1-8B / -70B)
_LLAMA31_ROPE = {"rope_type": "llama3", "factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                 "original_max_position_embeddings": 8192}
LLAMA31_8B = replace(LLAMA3_8B, name="llama3.1-8b", max_position=131072, rope_scaling=_LLAMA31_ROPE)
LLAMA31_70B = replace(LLAMA3_70B, name="llama3.1-70b", max_position=131072, rope_scaling=_LLAMA31_ROPE)

MIXTRAL_8X7B = ModelConfig(
    name="mixtral-8x7b", vocab_size=32000, hidden_size=4096, intermediate_size=14336,
    num_layers=32, num_heads=32, num_kv_heads=8, rope_theta=1e6, max_position=32768,
    num_experts=8, top_k=2, eos_token_id=2)

# Mistral-7B-v0.1: public HF config.json of mistralai/Mistral-7B-v0.1 (Llama layout, 4096-token
# sliding window over 32k positions)
MISTRAL_7B = ModelConfig(
    name="mistral-7b", vocab_size=32000, hidden_size=4096, intermediate_size=14336,
    num_layers=32, num_heads=32, num_kv_heads=8, rope_theta=1e4, rms_eps=1e-5, max_position=32768,
    eos_token_id=2, sliding_window=4096)

# tiny shapes for CPU unit tests / GPU smoke (same code paths: GQA 4, head_dim 128)
TINY_LLAMA = ModelConfig(
    name="tiny-llama", vocab_size=512, hidden_size=256, intermediate_size=512, num_layers=2,
    num_heads=4, num_kv_heads=1, max_position=2048, eos_token_id=1)

TINY_MIXTRAL = ModelConfig(
    name="tiny-mixtral", vocab_size=512, hidden_size=256, intermediate_size=256, num_layers=2,
    num_heads=4, num_kv_heads=1, max_position=2048, num_experts=4, top_k=2, eos_token_id=1)

# CPU rehearsals of the 8-rank bench (bench.py --gpus 8 over gloo): 8 q heads so TP = 8 shards them
# (the one kv head is replicated), 8 experts so EP = 8 gives every rank one
TINY_LLAMA_8H = replace(TINY_LLAMA, name="tiny-llama-8h", num_heads=8)
TINY_MIXTRAL_8E = replace(TINY_MIXTRAL, name="tiny-mixtral-8e", num_experts=8)

# Qwen3 (dense): TINY_LLAMA with the per-head QK-norm and Qwen3's eps / theta
TINY_QWEN3 = replace(TINY_LLAMA, name="tiny-qwen3", qk_norm=True, rms_eps=1e-6, rope_theta=1e6)

# Qwen3-8B / -32B: public HF config.json of Qwen/Qwen3-8B and Qwen/Qwen3-32B (Llama layout,
# head_dim 128, GQA 4 / 8, per-head QK-norm)
QWEN3_8B = ModelConfig(
    name="qwen3-8b", vocab_size=151936, hidden_size=4096, intermediate_size=12288, num_layers=36,
    num_heads=32, num_kv_heads=8, rope_theta=1e6, rms_eps=1e-6, max_position=40960, eos_token_id=151645,
    qk_norm=True)
QWEN3_32B = replace(QWEN3_8B, name="qwen3-32b", hidden_size=5120, intermediate_size=25600, num_layers=64,
                    num_heads=64)

PRESETS = {c.name: c for c in (LLAMA3_8B, LLAMA3_70B, LLAMA31_8B, LLAMA31_70B, MIXTRAL_8X7B, MISTRAL_7B, TINY_LLAMA,
                                TINY_MIXTRAL, TINY_LLAMA_8H, TINY_MIXTRAL_8E, TINY_QWEN3)}
# Real-size shapes that are served but are NOT in PRESETS: the GEMM planner's pinned route table
# (tests/fixtures/gemm_routes_gfx950.txt) is derived from every non-tiny PRESETS entry, so a new
# entry there would change that yardstick.  get_config, ALIASES and loader.known_preset look here
# too; the routes of these shapes are pinned in a fixture of their own.
CHECKPOINT_SHAPES = {c.name: c for c in (QWEN3_8B, QWEN3_32B)}
# accepted aliases (MLflow tags / CR annotations use HF-ish names)
ALIASES = {
    "meta-llama/Meta-Llama-3-8B": "llama3-8b", "llama-3-8b": "llama3-8b", "Llama-3-8B": "llama3-8b",
    "meta-llama/Meta-Llama-3-70B": "llama3-70b", "llama-3-70b": "llama3-70b", "Llama-3-70B": "llama3-70b",
    "meta-llama/Llama-3.1-8B": "llama3.1-8b", "meta-llama/Meta-Llama-3.1-8B": "llama3.1-8b",
    "meta-llama/Llama-3.1-70B": "llama3.1-70b", "meta-llama/Meta-Llama-3.1-70B": "llama3.1-70b",
    "mistralai/Mixtral-8x7B-v0.1": "mixtral-8x7b", "Mixtral-8x7B": "mixtral-8x7b",
    "mistralai/Mistral-7B-v0.1": "mistral-7b", "Mistral-7B": "mistral-7b",
    "Qwen/Qwen3-8B": "qwen3-8b", "Qwen3-8B": "qwen3-8b", "Qwen/Qwen3-32B": "qwen3-32b", "Qwen3-32B": "qwen3-32b",
}


def get_config(name: str, **overrides) -> ModelConfig:
    key = ALIASES.get(name, name)
    cfg = PRESETS.get(key) or CHECKPOINT_SHAPES.get(key)
    if cfg is None:
        raise KeyError(f"unknown model '{name}' (known: {sorted([*PRESETS, *CHECKPOINT_SHAPES])})")
    return replace(cfg, **overrides) if overrides else cfg
