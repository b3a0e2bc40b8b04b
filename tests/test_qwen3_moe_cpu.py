"""Qwen3-MoE checkpoints off the GPU: the loader (per-expert and fused tensor names, norm_topk_prob
on and off) and the CPU engine against transformers' Qwen3MoeForCausalLM, the config rules, the
published Qwen3-30B-A3B shape and its example CR."""
import dataclasses
import json
import os

import pytest
import torch
import yaml

from mlopamd.models import build_model, config, loader
from mlopamd.models.reference import dense_logits
from mlopamd.parallel.comm import Group, ParallelState
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qwen3_30b_a3b_config.json")) as _fh:
    PUBLISHED = json.load(_fh)  # Qwen/Qwen3-30B-A3B's config.json
TINY = dataclasses.replace(config.get_config("tiny-qwen3"), name="tiny-qwen3-moe", num_experts=128, top_k=8,
                           intermediate_size=64)


@pytest.fixture(scope="module", params=[True, False], ids=["renorm", "raw"])
def tiny_moe(request, tmp_path_factory):
    """({layout: checkpoint dir}, transformers model, tokens, HF logits): built once, read-only."""
    transformers = pytest.importorskip("transformers")
    from safetensors.torch import load_file, save_file

    d, d2 = tmp_path_factory.mktemp("saved"), tmp_path_factory.mktemp("resaved")
    cfg = transformers.Qwen3MoeConfig(
        vocab_size=512, hidden_size=256, intermediate_size=512, moe_intermediate_size=64, num_hidden_layers=2,
        num_attention_heads=4, num_key_value_heads=1, head_dim=128, max_position_embeddings=512, rms_norm_eps=1e-6,
        num_experts=128, num_experts_per_tok=8, norm_topk_prob=request.param, decoder_sparse_step=1,
        mlp_only_layers=[], rope_parameters={"rope_theta": 1e6, "rope_type": "default"})
    torch.manual_seed(0)
    m = transformers.Qwen3MoeForCausalLM(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(1 + 0.2 * torch.randn_like(p))
            elif "mlp" in n:  # larger router / expert weights: the routing decides the logits
                p.mul_(8)
    m.save_pretrained(d)
    # save_pretrained writes one layout (by transformers version); the other one is re-saved from it
    (d2 / "config.json").write_text((d / "config.json").read_text())
    sd = {k: v for f in d.glob("*.safetensors") for k, v in load_file(f).items()}
    out = {k: v for k, v in sd.items() if ".mlp.experts." not in k}
    fused = "model.layers.0.mlp.experts.gate_up_proj" in sd
    for p in (f"model.layers.{i}.mlp.experts." for i in range(2)):
        if fused:
            for e in range(128):
                out[f"{p}{e}.gate_proj.weight"], out[f"{p}{e}.up_proj.weight"] = sd[p + "gate_up_proj"][e].chunk(2)
                out[f"{p}{e}.down_proj.weight"] = sd[p + "down_proj"][e]
        else:
            out[p + "gate_up_proj"] = torch.stack([torch.cat([sd[f"{p}{e}.gate_proj.weight"],
                                                              sd[f"{p}{e}.up_proj.weight"]]) for e in range(128)])
            out[p + "down_proj"] = torch.stack([sd[f"{p}{e}.down_proj.weight"] for e in range(128)])
    save_file({k: v.contiguous() for k, v in out.items()}, d2 / "model.safetensors")
    toks = torch.randint(3, 500, (37,), generator=torch.Generator().manual_seed(5)).tolist()
    with torch.no_grad():
        exp = m(torch.tensor([toks])).logits[0].float()
    return {"fused": d if fused else d2, "per_expert": d2 if fused else d}, m, toks, exp


@pytest.mark.parametrize("layout", ["fused", "per_expert"])
def test_hf_parity_logits_and_greedy(tiny_moe, layout):
    dirs, hf, toks, exp = tiny_moe
    ours = loader.load_pretrained(dirs[layout], device="cpu", dtype=torch.float32)
    assert dataclasses.replace(ours.cfg, name=TINY.name, max_position=TINY.max_position, eos_token_id=TINY.eos_token_id,
                               embed_pooling="last") == dataclasses.replace(TINY, norm_topk_prob=hf.config.norm_topk_prob)
    torch.testing.assert_close(dense_logits(ours, toks), exp, atol=2e-4, rtol=1e-3)
    # the other norm_topk_prob is another function of the same weights
    other = dataclasses.replace(ours.cfg, norm_topk_prob=not ours.cfg.norm_topk_prob)
    flipped = build_model(other, device="cpu", dtype=torch.float32).load_shard_from(ours)
    assert float((dense_logits(flipped, toks) - exp).abs().max()) > 1e-2
    eng = Engine(ours, EngineConfig(max_num_seqs=4, max_num_batched_tokens=16, max_model_len=256,
                                    num_kv_blocks=64, use_graphs=False))
    prompts = [toks, toks[:9]]
    for p, o in zip(prompts, eng.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))):
        ref = hf.generate(torch.tensor([p]), max_new_tokens=6, do_sample=False, min_new_tokens=6, pad_token_id=0,
                          eos_token_id=None)
        assert o == ref[0, len(p):].tolist()


@pytest.mark.parametrize("change, message", [
    (dict(mlp_only_layers=[0, 4]), "mlp_only_layers"),
    (dict(decoder_sparse_step=2), "decoder_sparse_step"),
    (dict(num_experts=64), "num_experts=64"),
    (dict(num_experts_per_tok=16), "num_experts_per_tok=16"),
    (dict(num_attention_heads=40, num_key_value_heads=8), r"GQA group 40/8 = 5\b"),
    (dict(rope_scaling={"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}),
     "rope_scaling type 'yarn'"),
    (dict(moe_intermediate_size=None), "Qwen3-MoE.*moe_intermediate_size"),  # None: the key is left out
    (dict(num_experts_per_tok=None), "Qwen3-MoE.*num_experts_per_tok"),
    (dict(norm_topk_prob=None), "Qwen3-MoE.*norm_topk_prob"),
])
def test_rejected_configs(change, message):
    with pytest.raises(ValueError, match=message):
        loader.config_from_hf({k: v for k, v in dict(PUBLISHED, **change).items() if v is not None or k not in change})


def test_rejected_sharding_and_engine_options(tmp_path):
    for tp, ep in ((2, 2), (1, 2)):
        with pytest.raises(ValueError, match="more than 64 experts"):
            build_model(TINY, device="cpu", dtype=torch.float32, pstate=ParallelState(tp=Group(0, tp), ep=Group(0, ep)))
    with pytest.raises(ValueError, match="norm_topk_prob"):
        build_model(dataclasses.replace(config.TINY_MIXTRAL, norm_topk_prob=False), device="cpu", dtype=torch.float32)
    m = build_model(TINY, device="cpu", dtype=torch.float32)
    base = dict(max_num_seqs=2, max_num_batched_tokens=16, max_model_len=64, num_kv_blocks=16, use_graphs=False)
    for kw in (dict(kv_cache_dtype="fp8"), dict(spec_tokens=2), dict(embed_slots=2)):
        with pytest.raises(ValueError, match="MoE"):
            Engine(m, EngineConfig(**base, **kw))
    (tmp_path / "adapter_config.json").write_text("{}")
    with pytest.raises(ValueError, match="dense"):
        loader.load_adapter(tmp_path, TINY)


def test_published_shape_its_cr_and_the_pinned_dicts():
    from mlopamd.controller import crd, placement

    cfg = loader.config_from_hf(PUBLISHED, name="qwen3-30b-a3b")
    assert cfg == config.get_config("Qwen/Qwen3-30B-A3B") == config.MOE_CHECKPOINT_SHAPES["qwen3-30b-a3b"]
    assert loader.known_preset(cfg) == "qwen3-30b-a3b"
    assert (cfg.hidden_size, cfg.num_layers, cfg.num_heads, cfg.num_kv_heads, cfg.head_dim, cfg.intermediate_size,
            cfg.num_experts, cfg.top_k, cfg.vocab_size, cfg.rope_theta) == (2048, 48, 32, 4, 128, 768, 128, 8, 151936, 1e6)
    assert 30.0e9 < cfg.num_params() < 31.0e9 and 3.0e9 < cfg.active_params() < 3.6e9
    # both dicts feed pinned planner fixtures: the MoE shape is in neither
    assert sorted(config.CHECKPOINT_SHAPES) == ["qwen3-32b", "qwen3-8b"] and len(config.PRESETS) == 11
    assert not any(c.num_experts > 8 for c in config.PRESETS.values())
    with open(crd.MANIFESTS / "examples" / "qwen3" / "qwen3-30b-a3b.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr)
    assert errs == [] and pruned == cr
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert spec.validate() == [] and spec.architecture == "qwen3-30b-a3b"
    p = placement.plan(spec.architecture, max_model_len=spec.max_model_len, max_num_seqs=spec.max_num_seqs,
                       requested_tp=spec.tensor_parallel)
    assert p.fits and p.gpus == 1
