"""Sliding-window attention off the GPU: the checkpoint loader and the dense oracle against
transformers' MistralForCausalLM, the reference attention against a naive loop, the step
metadata's planner span, and the engine's release of pages that fell out of the window."""
import dataclasses
import json
import math

import numpy as np
import pytest
import torch

from mlopamd.models import build_model, loader
from mlopamd.models.config import TINY_LLAMA, get_config
from mlopamd.models.reference import dense_logits
from mlopamd.ops import reference as ref
from mlopamd.runtime.attn_meta import AttnMeta, MetaBuffers, plan_partitions
from mlopamd.runtime.engine import Engine, EngineConfig, Status
from mlopamd.runtime.sampler import SamplingParams


# ------------------------------------------------------------------ HF parity --

def _tiny_mistral(tmp_path, window=8):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.MistralConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                     num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                                     max_position_embeddings=512, rms_norm_eps=1e-5, sliding_window=window,
                                     rope_parameters={"rope_theta": 10000.0, "rope_type": "default"})
    torch.manual_seed(0)
    m = transformers.MistralForCausalLM(cfg).eval()
    with torch.no_grad():  # non-trivial norm weights: a swapped norm would show
        for n, p in m.named_parameters():
            if n.endswith("layernorm.weight") or n == "model.norm.weight":
                p.copy_(1 + 0.2 * torch.randn_like(p))
    m.save_pretrained(tmp_path)
    return m


def _hf_greedy(m, prompt, n):
    out = m.generate(torch.tensor([prompt]), max_new_tokens=n, do_sample=False, min_new_tokens=n,
                     pad_token_id=0, eos_token_id=None)
    return out[0, len(prompt):].tolist()


def test_hf_mistral_sliding_window_parity(tmp_path):
    hf = _tiny_mistral(tmp_path)
    cfg = loader.config_from_hf(json.loads((tmp_path / "config.json").read_text()))
    assert cfg.sliding_window == 8 and cfg.rope_theta == 1e4 and not cfg.is_moe
    ours = loader.load_pretrained(tmp_path, device="cpu", dtype=torch.float32)
    assert ours.cfg.sliding_window == 8
    toks = torch.randint(3, 500, (37,), generator=torch.Generator().manual_seed(5)).tolist()
    with torch.no_grad():
        exp = hf(torch.tensor([toks])).logits[0].float()
    got = dense_logits(ours, toks)
    torch.testing.assert_close(got, exp, atol=2e-4, rtol=1e-3)
    # chunked prefill (16-token chunks) crosses the 8-token window; the engine generates
    # transformers' greedy continuation
    eng = Engine(ours, EngineConfig(max_num_seqs=4, max_num_batched_tokens=16, max_model_len=256,
                                    num_kv_blocks=64, use_graphs=False))
    prompts = [toks, toks[:9]]
    outs = eng.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))
    for p, o in zip(prompts, outs):
        assert o == _hf_greedy(hf, p, 6)
    assert eng.stats["kv_pages_released"] > 0


def test_use_sliding_window_false_is_the_no_window_model(tmp_path):
    transformers = pytest.importorskip("transformers")
    _tiny_mistral(tmp_path)
    toks = torch.randint(3, 500, (37,), generator=torch.Generator().manual_seed(5)).tolist()
    windowed = dense_logits(loader.load_pretrained(tmp_path, device="cpu", dtype=torch.float32), toks)
    d = json.loads((tmp_path / "config.json").read_text())
    d["use_sliding_window"] = False
    (tmp_path / "config.json").write_text(json.dumps(d))
    ours = loader.load_pretrained(tmp_path, device="cpu", dtype=torch.float32)
    assert ours.cfg.sliding_window == 0
    hf = transformers.MistralForCausalLM.from_pretrained(tmp_path, sliding_window=None).eval()
    with torch.no_grad():
        exp = hf(torch.tensor([toks])).logits[0].float()
    got = dense_logits(ours, toks)
    torch.testing.assert_close(got, exp, atol=2e-4, rtol=1e-3)
    # the window changes nothing at positions 0..7 and something from position 8 on
    torch.testing.assert_close(windowed[:8], got[:8], atol=2e-4, rtol=1e-3)
    assert not torch.allclose(windowed[8:], got[8:], atol=1e-2, rtol=0)


# --------------------------------------------------------------------- config --

_BASE = {"hidden_size": 256, "num_attention_heads": 2, "vocab_size": 512, "intermediate_size": 512,
         "num_hidden_layers": 2, "max_position_embeddings": 32768}


def test_config_window_by_architecture():
    mix = dict(_BASE, architectures=["MixtralForCausalLM"], num_local_experts=4, sliding_window=4096)
    cfg = loader.config_from_hf(mix)
    assert cfg.sliding_window == 4096 and cfg.is_moe
    mis = dict(_BASE, architectures=["MistralForCausalLM"], sliding_window=4096)
    assert loader.config_from_hf(mis).sliding_window == 4096
    assert loader.config_from_hf(dict(mis, sliding_window=None)).sliding_window == 0
    assert loader.config_from_hf(dict(mis, use_sliding_window=False)).sliding_window == 0
    assert loader.config_from_hf(dict(mis, sliding_window=32768)).sliding_window == 0  # covers every position
    with pytest.raises(ValueError, match="sliding_window"):
        loader.config_from_hf(dict(_BASE, architectures=["LlamaForCausalLM"], sliding_window=4096))
    with pytest.raises(ValueError, match="layer_types"):
        loader.config_from_hf(dict(mis, layer_types=["sliding_attention", "full_attention"]))
    assert loader.config_from_hf(dict(mis, layer_types=["sliding_attention"] * 2)).sliding_window == 4096


def test_mistral_preset():
    cfg = get_config("mistralai/Mistral-7B-v0.1")
    assert cfg is get_config("Mistral-7B") and cfg.name == "mistral-7b"
    assert (cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_layers) == (32000, 4096, 14336, 32)
    assert (cfg.num_heads, cfg.num_kv_heads, cfg.rope_theta, cfg.rms_eps) == (32, 8, 1e4, 1e-5)
    assert (cfg.max_position, cfg.eos_token_id, cfg.sliding_window) == (32768, 2, 4096)
    assert get_config("mistral-7b", sliding_window=0).sliding_window == 0
    assert TINY_LLAMA.sliding_window == 0


# -------------------------------------------------------- reference attention --

@pytest.mark.parametrize("W", [1, 5, 16, 40])
def test_reference_attention_matches_naive_loop(W):
    g = torch.Generator().manual_seed(W)
    Hkv, G, D, NB = 2, 2, 16, 40
    q_lens, ctx_lens = [1, 7, 3, 1], [50, 7, 33, 1]
    kc = torch.randn(NB, Hkv, 16, D, generator=g)
    vc = torch.randn(NB, Hkv, 16, D, generator=g)
    pages = torch.randperm(NB - 1, generator=g) + 1
    bt = torch.zeros(len(q_lens), 4, dtype=torch.int32)
    p = 0
    for r, c in enumerate(ctx_lens):
        n = (c + 15) // 16
        bt[r, :n] = pages[p:p + n].int()
        p += n
    starts = np.concatenate([[0], np.cumsum(q_lens)[:-1]])
    i32 = lambda a: torch.tensor(np.asarray(a), dtype=torch.int32)  # noqa: E731
    T = sum(q_lens)
    e = torch.empty(0)
    meta = AttnMeta(positions=e, slots=e, block_tables=bt, tile_seq=i32(range(len(q_lens))), tile_q0=i32([0] * 4),
                    ptile_seq=i32([]), ptile_q0=i32([]), q_start=i32(starts), q_len=i32(q_lens),
                    ctx_len=i32(ctx_lens), part_tokens=32, nparts=1, part_o=e, part_ml=e, logits_idx=e,
                    num_tokens=T, window=W)
    q = torch.randn(T, Hkv * G, D, generator=g)
    got = ref.paged_attention(q, kc, vc, meta)
    exp = torch.zeros_like(q)
    for r, (ql, c) in enumerate(zip(q_lens, ctx_lens)):
        for t in range(ql):
            i = c - ql + t
            for h in range(Hkv * G):
                keys = range(max(0, i - W + 1), i + 1)
                k = torch.stack([kc[bt[r, j // 16], h // G, j % 16] for j in keys])
                v = torch.stack([vc[bt[r, j // 16], h // G, j % 16] for j in keys])
                w = torch.softmax(k @ q[starts[r] + t, h] / math.sqrt(D), 0)
                exp[starts[r] + t, h] = w @ v
    torch.testing.assert_close(got, exp, atol=1e-5, rtol=1e-5)
    meta.window = 0
    assert not torch.allclose(ref.paged_attention(q, kc, vc, meta), exp, atol=1e-3)


# ---------------------------------------------------------------- MetaBuffers --

def test_planner_span_and_flash_work_follow_the_window():
    W, G = 128, 4
    mb = MetaBuffers(1024, 4, 32768 // 16, G, 1, 32768, "cpu", window=W)
    plain = MetaBuffers(1024, 4, 32768 // 16, G, 1, 32768, "cpu")
    assert plain.span(32000) == 32000 and plain.meta(1, 1, 1, 32, 1).window == 0
    assert mb.span(32000) == W + 31 + 16 // G - 1 and mb.span(20) == 20
    part, nparts = plan_partitions(1, 1, mb.span(32000))
    assert part * nparts >= mb.span(32000) and nparts == 2          # split over ~W keys ...
    assert plan_partitions(1, 1, plain.span(32000))[1] > 100        # ... not over the context
    assert mb.meta(1, 1, 1, part, nparts).window == W
    # flash tiles' key counts (the LPT order's work): clamped to what a windowed tile reads
    for b in (mb, plain):
        b.fill([0], [600], [2000], [np.arange(600)])
    assert mb.npt == plain.npt == (600 + 31) // 32
    assert plain._pwork[:plain.npt].max() > 2000 - 32  # (unwindowed: the whole causal range)
    clamp = W + 31 + 128 // G - 1
    np.testing.assert_array_equal(mb._pwork[:mb.npt], np.minimum(plain._pwork[:plain.npt], clamp))
    assert mb._pwork[:mb.npt].max() == clamp


# --------------------------------------------------------------- page release --

def _model(W, seed=1):
    return build_model(dataclasses.replace(TINY_LLAMA, sliding_window=W), device="cpu", dtype=torch.float32, seed=seed)


def _prompt(n, seed):
    return torch.randint(2, 500, (n,), generator=torch.Generator().manual_seed(seed)).tolist()


def test_pages_below_the_window_are_released():
    W, chunk, n_prompt, n_gen = 32, 48, 150, 50
    model = _model(W)
    eng = Engine(model, EngineConfig(max_num_seqs=2, max_num_batched_tokens=chunk, max_model_len=256,
                                     num_kv_blocks=32, use_graphs=False))
    free0 = eng.alloc.num_free
    freed = []
    real_free = eng.alloc.free
    eng.alloc.free = lambda blocks: (freed.extend(blocks), real_free(blocks))[1]
    prompt = _prompt(n_prompt, 3)
    seq = eng.add_request(prompt, SamplingParams(max_tokens=n_gen, ignore_eos=True))
    held_max = 0
    while seq.status != Status.FINISHED:
        eng.step()
        held = sum(1 for b in seq.blocks if b)
        assert held == free0 - eng.alloc.num_free
        held_max = max(held_max, held)
    assert held_max <= (W + 31 + chunk) // 16 + 2
    # the last query ran at position 198 (the 200th token is sampled, never fed): the pages
    # below the pair holding its first visible key, 198 - W + 1
    last_q = n_prompt + n_gen - 2
    assert eng.stats["kv_pages_released"] == ((last_q - W + 1) & ~31) >> 4 == 10
    assert eng.alloc.num_free == free0
    # every page of the 199 tokens fed went back exactly once (ids recur: released pages are reused)
    assert 0 not in freed and len(freed) == (n_prompt + n_gen - 1 + 15) // 16
    # same tokens as the dense windowed oracle, and as the engine that keeps every page
    toks = list(prompt)
    for t in seq.output[:8]:
        assert t == int(dense_logits(model, toks)[-1].argmax())
        toks.append(t)
    keep = Engine(model, EngineConfig(max_num_seqs=2, max_num_batched_tokens=chunk, max_model_len=256,
                                      num_kv_blocks=32, use_graphs=False, swa_release=False))
    assert keep.generate([prompt], SamplingParams(max_tokens=n_gen, ignore_eos=True))[0] == seq.output
    assert keep.stats["kv_pages_released"] == 0


def test_release_with_shared_prefix_matches_uncached():
    model = _model(32, seed=4)
    shared = _prompt(64, 7)
    prompts = [shared + _prompt(40, 8), shared + _prompt(25, 9)]
    outs = {}
    for caching in (True, False):
        eng = Engine(model, EngineConfig(max_num_seqs=4, max_num_batched_tokens=96, max_model_len=256,
                                         num_kv_blocks=64, use_graphs=False, enable_prefix_caching=caching))
        free0 = eng.alloc.num_free
        outs[caching] = [eng.generate([p], SamplingParams(max_tokens=20, ignore_eos=True))[0] for p in prompts]
        assert eng.alloc.num_free == free0 and eng.stats["kv_pages_released"] > 0
        if caching:  # the second request took the shared pages, then gave back those below its window
            assert eng.stats["prefix_hit_tokens"] == 64
    assert outs[True] == outs[False]


def test_release_survives_preemption():
    model = _model(32, seed=6)
    # short prompts: all four are admitted at one page each, then grow to ~4 pages apiece
    prompts = [_prompt(10 + 3 * i, 20 + i) for i in range(4)]
    sp = SamplingParams(max_tokens=80, ignore_eos=True)
    big = Engine(model, EngineConfig(max_num_seqs=4, max_num_batched_tokens=64, max_model_len=256,
                                     num_kv_blocks=64, use_graphs=False))
    exp = big.generate(prompts, sp)
    assert big.stats["preemptions"] == 0
    small = Engine(model, EngineConfig(max_num_seqs=4, max_num_batched_tokens=64, max_model_len=256,
                                       num_kv_blocks=9, use_graphs=False))
    free0 = small.alloc.num_free
    assert small.generate(prompts, sp) == exp
    assert small.stats["preemptions"] > 0 and small.stats["kv_pages_released"] > 0
    assert small.alloc.num_free == free0
