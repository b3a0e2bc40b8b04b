"""Checkpoint loading: Hugging Face ``config.json`` + ``*.safetensors`` -> our model layout.

The operator hands a predictor its MLflow artifact URI (``s3://mlflow/<rel>``, reference
``mlflow_operator.py:125-127``).  When that artifact is reachable as a local directory
(``file://`` URI, a plain path, or ``s3://mlflow/<rel>`` under ``MLOP_ARTIFACT_ROOT``)
holding a Llama / Mistral / Mixtral / Qwen3 (dense) checkpoint in the HF layout, the runtime serves those weights;
otherwise it random-initialises the architecture named by the CR / MLflow tags (the
benchmark configuration: no checkpoints are downloadable here).

Layout mapping (HF name -> ours; TP sharding then reuses ``load_shard_from``):
  model.embed_tokens / lm_head / model.norm       -> embed / lm_head / final_norm
  self_attn.{q,k,v}_proj                         -> qkv  ([q; k; v] rows, rotate-half RoPE as HF)
  self_attn.o_proj                               -> o
  self_attn.{q,k}_norm (Qwen3)                   -> q_norm / k_norm  (per head, replicated over TP)
  input_layernorm / post_attention_layernorm     -> in_norm / post_norm
  mlp.{gate,up}_proj                             -> gate_up (rows interleaved in groups of 16:
                                                    the GEMM's SiLU-mul epilogue layout)
  mlp.down_proj                                  -> down
  Mixtral: block_sparse_moe.gate | mlp.gate      -> router
           experts.{e}.w1 / w3 (legacy) or experts.gate_up_proj (fused) -> w13 (interleaved)
           experts.{e}.w2 or experts.down_proj   -> w2
Tensors are read lazily, one layer at a time (safetensors memory map), so a 141 GB
checkpoint never sits in host memory at once.
"""
from __future__ import annotations

import json
import os
from dataclasses import replace
from pathlib import Path

import torch

from .config import CHECKPOINT_SHAPES, ModelConfig, PRESETS

# Qwen3 (dense) is the Llama layer with a per-head QK-norm before RoPE (ModelConfig.qk_norm)
_ARCH_NAMES = {"LlamaForCausalLM": "llama", "MixtralForCausalLM": "mixtral", "MistralForCausalLM": "llama",
               "Qwen3ForCausalLM": "llama"}
# base-model checkpoints (decoder-style embedding models): the same layers, tensor names without the
# "model." prefix, no lm_head.weight; they serve embedding requests only (ModelConfig.embedding_only)
_BASE_ARCHS = {"LlamaModel": "LlamaForCausalLM", "MistralModel": "MistralForCausalLM", "Qwen3Model": "Qwen3ForCausalLM"}
# GQA groups the attention bindings take (bindings.cpp: decode "GQA group must divide 16"; flash prefill 1, 2, 4, 8)
_GQA_GROUPS = (1, 2, 4, 8, 16)


def _is_checkpoint(d: Path) -> bool:
    return (d / "config.json").is_file() and any(d.glob("*.safetensors"))


def _is_adapter(d: Path) -> bool:
    return (d / "adapter_config.json").is_file()


def resolve_adapter_dir(uri: str | None) -> Path | None:
    """Local PEFT adapter directory for an adapter URI (the rules of ``resolve_model_dir``,
    with ``adapter_config.json`` as the marker file), or None."""
    return resolve_model_dir(uri, _is_adapter)


def resolve_model_dir(uri: str | None, marker=_is_checkpoint) -> Path | None:
    """Local checkpoint directory for a model URI, or None (serve random-init weights)."""
    if not uri:
        return None
    if uri.startswith("file://"):
        p = Path(uri[len("file://"):])
    elif uri.startswith("s3://"):
        root = os.environ.get("MLOP_ARTIFACT_ROOT")
        if not root:
            return None
        p = Path(root) / uri[len("s3://"):].split("/", 1)[-1]  # drop the bucket ("mlflow")
    elif "://" in uri:
        return None
    else:
        p = Path(uri)
    for cand in (p, p / "model", p / "checkpoint", p / "artifacts"):
        if marker(cand):
            return cand
    return None


def config_from_hf(d: dict, name: str | None = None) -> ModelConfig:
    """ModelConfig from an HF ``config.json`` dict (Llama / Mistral / Mixtral / dense Qwen3 families)."""
    arch = (d.get("architectures") or ["LlamaForCausalLM"])[0]
    embedding_only = arch in _BASE_ARCHS
    arch = _BASE_ARCHS.get(arch, arch)
    if arch == "Qwen3MoeForCausalLM":
        raise ValueError("Qwen3-MoE checkpoints are not supported: their router (norm_topk_prob, 128 experts) "
                         "differs from Mixtral's; only the dense Qwen3ForCausalLM loads")
    if arch not in _ARCH_NAMES:
        raise ValueError(f"unsupported checkpoint architecture {arch!r} (supported: {sorted(_ARCH_NAMES)}, and the "
                         f"base models {sorted(_BASE_ARCHS)} for embeddings; bidirectional encoders, rerankers and "
                         "classification heads are not served)")
    if d.get("hidden_act", "silu") != "silu":
        raise ValueError(f"unsupported activation {d.get('hidden_act')!r}")
    H, nh = d["hidden_size"], d["num_attention_heads"]
    rp = d.get("rope_parameters") or {}
    theta = rp.get("rope_theta", d.get("rope_theta", 10000.0))
    scaling = d.get("rope_scaling")
    if scaling is None and rp.get("rope_type", "default") not in ("default", None):
        scaling = dict(rp)
    # settings this runtime cannot serve are REJECTED, never dropped (dropping any of them
    # gives wrong logits with no error)
    if scaling:
        rt = scaling.get("rope_type", scaling.get("type", "default"))
        if rt not in ("default", "llama3"):
            raise ValueError(f"unsupported rope_scaling type {rt!r} (supported: default, llama3)")
    max_pos = int(d.get("max_position_embeddings", 8192))
    sw = d.get("sliding_window")
    window = 0
    if sw is not None and d.get("use_sliding_window", True) is not False and int(sw) < max_pos:
        if arch == "LlamaForCausalLM":
            # transformers ignores the key for this architecture: honouring it would change logits
            raise ValueError(f"sliding_window={sw} < max_position_embeddings={max_pos}: "
                             "sliding-window attention is not implemented for LlamaForCausalLM")
        window = int(sw)
    lt = d.get("layer_types")
    if lt and len(set(lt)) > 1:
        raise ValueError(f"layer_types mixes {sorted(set(lt))}: per-layer attention types are not supported")
    if lt and window and set(lt) == {"full_attention"}:
        window = 0
    if lt and not window and set(lt) == {"sliding_attention"}:
        raise ValueError("layer_types asks for sliding_attention without a sliding_window that applies")
    for flag in ("attention_bias", "mlp_bias"):
        if d.get(flag):
            raise ValueError(f"{flag}=true is not supported (bias tensors are not loaded)")
    nkv = d.get("num_key_value_heads") or nh
    qk_norm = arch == "Qwen3ForCausalLM"
    if qk_norm and (nh % nkv or nh // nkv not in _GQA_GROUPS):
        # (Qwen3-14B: 40 query heads over 8 KV heads) fail here, not in a device-path check
        raise ValueError(f"GQA group {nh}/{nkv} = {nh / nkv:g} is not supported: the attention kernels take "
                         f"groups of {', '.join(map(str, _GQA_GROUPS))}")
    eos = d.get("eos_token_id", 2)
    eos_all = tuple(int(e) for e in eos) if isinstance(eos, list) else ((int(eos),) if eos is not None else (2,))
    eos = eos_all[0]
    return ModelConfig(
        name=name or d.get("_name_or_path") or arch, vocab_size=d["vocab_size"], hidden_size=H,
        intermediate_size=d["intermediate_size"], num_layers=d["num_hidden_layers"], num_heads=nh,
        num_kv_heads=nkv, head_dim=d.get("head_dim") or H // nh,
        rope_theta=float(theta), rms_eps=float(d.get("rms_norm_eps", 1e-5)),
        max_position=max_pos,
        tie_embeddings=bool(d.get("tie_word_embeddings", False)) or embedding_only, embedding_only=embedding_only,
        num_experts=int(d.get("num_local_experts", 0) or 0), top_k=int(d.get("num_experts_per_tok", 2)),
        rope_scaling=scaling, eos_token_id=int(eos), extra_eos_ids=eos_all[1:], sliding_window=window,
        qk_norm=qk_norm)


class _Tensors:
    """Name -> tensor over every ``*.safetensors`` shard of a directory (lazy, mmap)."""

    def __init__(self, path: Path):
        from safetensors import safe_open

        self._files = [safe_open(str(f), framework="pt") for f in sorted(path.glob("*.safetensors"))]
        self._where = {k: f for f in self._files for k in f.keys()}

    def has(self, k: str) -> bool:
        return k in self._where

    def get(self, k: str) -> torch.Tensor:
        if k not in self._where:
            raise KeyError(f"checkpoint has no tensor {k!r}")
        return self._where[k].get_tensor(k)


class _LazyLayer:
    """One decoder layer in our layout: every key is read (and re-laid-out) from the
    checkpoint when accessed, nothing is kept (one tensor in host memory at a time)."""

    def __init__(self, thunks: dict):
        self._thunks = thunks

    def __getitem__(self, k):
        return self._thunks[k]()

    def __contains__(self, k):
        return k in self._thunks


class HFWeights:
    """A TP=1 model's weights in our layout, read from an HF checkpoint (the ``full``
    argument of ``LlamaModel.load_shard_from``)."""

    def __init__(self, path: Path, cfg: ModelConfig):
        from ..ops import interleave_gate_up

        self.cfg = cfg
        t = _Tensors(path)
        self._t = t
        # a base-model checkpoint (LlamaModel / MistralModel / Qwen3Model) names its tensors without "model."
        pre = "model." if t.has("model.embed_tokens.weight") or not t.has("embed_tokens.weight") else ""
        self.embed = t.get(pre + "embed_tokens.weight")
        self.final_norm = t.get(pre + "norm.weight")
        self.lm_head = t.get("lm_head.weight") if t.has("lm_head.weight") else self.embed

        def layer(i):
            p = f"{pre}layers.{i}."
            L = {"qkv": lambda: torch.cat([t.get(p + f"self_attn.{n}_proj.weight") for n in "qkv"], 0),
                 "o": lambda: t.get(p + "self_attn.o_proj.weight"),
                 "in_norm": lambda: t.get(p + "input_layernorm.weight"),
                 "post_norm": lambda: t.get(p + "post_attention_layernorm.weight")}
            if cfg.qk_norm:  # (a Llama checkpoint that carries such tensors is loaded as before)
                L["q_norm"] = lambda: t.get(p + "self_attn.q_norm.weight")
                L["k_norm"] = lambda: t.get(p + "self_attn.k_norm.weight")
            if not cfg.is_moe:
                L["gate_up"] = lambda: interleave_gate_up(t.get(p + "mlp.gate_proj.weight"),
                                                          t.get(p + "mlp.up_proj.weight"))
                L["down"] = lambda: t.get(p + "mlp.down_proj.weight")
                return _LazyLayer(L)
            E, I = cfg.num_experts, cfg.intermediate_size
            if t.has(p + "block_sparse_moe.gate.weight"):  # legacy per-expert layout (save_pretrained)
                m = p + "block_sparse_moe."
                L["router"] = lambda: t.get(m + "gate.weight")
                L["w13"] = lambda: torch.stack([interleave_gate_up(t.get(m + f"experts.{e}.w1.weight"),
                                                                   t.get(m + f"experts.{e}.w3.weight"))
                                                for e in range(E)])
                L["w2"] = lambda: torch.stack([t.get(m + f"experts.{e}.w2.weight") for e in range(E)])
            else:  # fused expert tensors (transformers >= 5 module layout)
                m = p + "mlp."
                L["router"] = lambda: t.get(m + "gate.weight")

                def w13():
                    gu = t.get(m + "experts.gate_up_proj")  # [E, 2I, H]: gate rows then up rows
                    return torch.stack([interleave_gate_up(gu[e, :I], gu[e, I:]) for e in range(E)])

                L["w13"] = w13
                L["w2"] = lambda: t.get(m + "experts.down_proj")
            return _LazyLayer(L)

        self.layers = [layer(i) for i in range(cfg.num_layers)]


def embedding_defaults(path: str | os.PathLike) -> tuple:
    """(pooling, normalize) an embedding request to the checkpoint in ``path`` gets when it names none:
    from its sentence-transformers settings (``modules.json`` lists the modules, a ``Normalize`` one
    among them or not; ``1_Pooling/config.json`` holds the pooling mode), ("last", True) without
    them.  A pooling mode this runtime does not serve (CLS, max, weighted mean, ...) gives None: a
    request must then name its pooling."""
    path = Path(path)
    mods, pool = path / "modules.json", path / "1_Pooling" / "config.json"
    if not mods.is_file() and not pool.is_file():
        return "last", True
    normalize = False
    if mods.is_file():
        normalize = any(str(m.get("type", "")).endswith("Normalize") for m in json.loads(mods.read_text()))
    pooling = None
    if pool.is_file():
        pc = json.loads(pool.read_text())
        on = sorted(k for k, v in pc.items() if k.startswith("pooling_mode_") and v is True)
        pooling = {("pooling_mode_lasttoken",): "last", ("pooling_mode_mean_tokens",): "mean"}.get(tuple(on))
    return pooling, normalize


def load_pretrained(path: str | os.PathLike, device="cuda", dtype=torch.bfloat16, pstate=None,
                    name: str | None = None, fold_norms: bool = True):
    """Build our model for the checkpoint in ``path`` and copy its (TP-sharded) weights in."""
    from . import build_model

    path = Path(path)
    cfg = config_from_hf(json.loads((path / "config.json").read_text()), name=name or path.name)
    pooling, normalize = embedding_defaults(path)
    cfg = replace(cfg, embed_pooling=pooling, embed_normalize=normalize)
    model = build_model(cfg, device=device, dtype=dtype, pstate=pstate)
    with torch.no_grad():
        model.load_shard_from(HFWeights(path, cfg))
    # checkpoints carry trained (non-unit) RMSNorm weights: fold them into the projections that
    # consume them so the large-M forward can run the norm chain (LlamaModel._chain_ok needs unit
    # norms).  The same function up to the bf16 rounding of g * W; fold_norms=False keeps them.
    if fold_norms:
        model.fold_norms()
    return model


def known_preset(cfg: ModelConfig) -> str | None:
    """Name of the preset with the same shapes (placement / reporting), if any."""
    for n, p in (*PRESETS.items(), *CHECKPOINT_SHAPES.items()):
        if replace(p, name=cfg.name, eos_token_id=cfg.eos_token_id, rope_scaling=cfg.rope_scaling,
                   max_position=cfg.max_position) == cfg:
            return n
    return None


# ---------------------------------------------------------------- LoRA --

_LORA_KEY = "base_model.model.model.layers.{i}.{blk}.{m}.lora_{ab}.weight"
_LORA_BLOCK = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
               "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}


def _adapter_digest(path: Path) -> bytes:
    import hashlib

    h = hashlib.blake2b(digest_size=16)
    for f in sorted(path.glob("adapter_config.json")) + sorted(path.glob("*.safetensors")):
        h.update(f.name.encode())
        with open(f, "rb") as fh:
            for chunk in iter(lambda: fh.read(1 << 20), b""):
                h.update(chunk)
    return h.digest()


def load_adapter(path: str | os.PathLike, cfg: ModelConfig, max_rank: int | None = None):
    """Read a PEFT-format LoRA adapter directory (``adapter_config.json`` +
    ``adapter_model.safetensors``) into our layout: ``models.lora.Adapter``.  Settings this
    runtime cannot serve raise ValueError (they would otherwise give wrong logits silently)."""
    import math

    from ..ops import interleave_gate_up
    from .lora import MAX_LORA_RANK, PROJ_MODULES, TARGET_MODULES, Adapter, check_shapes, module_shapes

    path = Path(path)
    if not (path / "adapter_config.json").is_file():
        raise ValueError(f"{path} holds no adapter_config.json")
    ac = json.loads((path / "adapter_config.json").read_text())
    if cfg.is_moe:
        raise ValueError("LoRA adapters are served on dense Llama / Mistral models only (not Mixtral)")
    check_shapes(cfg)
    if str(ac.get("peft_type", "LORA")).upper() != "LORA":
        raise ValueError(f"unsupported peft_type {ac.get('peft_type')!r} (only LORA)")
    if ac.get("use_dora"):
        raise ValueError("DoRA adapters (use_dora) are not supported")
    if ac.get("bias", "none") != "none":
        raise ValueError(f"bias={ac.get('bias')!r} is not supported (only 'none')")
    if ac.get("modules_to_save"):
        raise ValueError(f"modules_to_save={ac['modules_to_save']} is not supported")
    for k in ("rank_pattern", "alpha_pattern"):
        if ac.get(k):
            raise ValueError(f"a non-empty {k} is not supported (one rank / alpha per adapter)")
    r = int(ac["r"])
    cap = MAX_LORA_RANK if max_rank is None else min(MAX_LORA_RANK, int(max_rank))
    if r < 1 or r > cap:
        raise ValueError(f"adapter rank {r} is outside [1, {cap}] (the maximum LoRA rank)")
    tm = ac.get("target_modules")
    if isinstance(tm, str) or not tm:
        raise ValueError(f"target_modules must be a list of module names, got {tm!r}")
    bad = sorted(set(tm) - set(TARGET_MODULES))
    if bad:
        raise ValueError(f"unsupported target_modules {bad} (embedding / lm_head and other layers cannot take "
                         f"an adapter; supported: {list(TARGET_MODULES)})")
    alpha = float(ac.get("lora_alpha", r))
    scale = alpha / math.sqrt(r) if ac.get("use_rslora") else alpha / r
    t = _Tensors(path)
    shapes = module_shapes(cfg)
    known = set()
    layers = []
    for i in range(cfg.num_layers):
        per = {}
        for m in tm:
            ka, kb = (_LORA_KEY.format(i=i, blk=_LORA_BLOCK[m], m=m, ab=ab) for ab in "AB")
            known.update((ka, kb))
            a, b = t.get(ka).float(), t.get(kb).float()
            n, k = shapes[m]
            if tuple(a.shape) != (r, k) or tuple(b.shape) != (n, r):
                raise ValueError(f"layer {i} {m}: lora_A {tuple(a.shape)} / lora_B {tuple(b.shape)} do not fit "
                                 f"rank {r} and the base weight [{n}, {k}]")
            per[m] = (a, b * scale)  # the scaling in fp32; one rounding when the slot is filled
        L = {}
        for proj, mods in PROJ_MODULES.items():
            if not any(m in per for m in mods):
                continue
            K = shapes[mods[0]][1]
            A = torch.stack([per[m][0] if m in per else torch.zeros(r, K) for m in mods])
            Bs = [per[m][1] if m in per else torch.zeros(shapes[m][0], r) for m in mods]
            L[proj] = (A, interleave_gate_up(*Bs) if proj == "gate_up" else torch.cat(Bs, 0))
        layers.append(L)
    extra = sorted(k for k in t._where if k not in known)
    if extra:
        raise ValueError(f"adapter holds tensors outside its target_modules / this model: {extra[:4]}")
    return Adapter(rank=r, layers=layers, target_modules=tuple(tm), digest=_adapter_digest(path), path=str(path))
