"""The serving engine with kv_cache_dtype="fp8" on the GPU (kv_fp8.hip's writer and
attention.hip's KvFp8 decode kernel under chunked prefill, eager and hipGraph decode, prefix caching,
LoRA) against the dense fp32 oracle that fake-quantises post-RoPE K and V with the cache's rule."""
import pytest
import torch

from mlopamd.models import build_model, loader
from mlopamd.models.config import TINY_LLAMA
from mlopamd.models.lora import merged_copy
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from test_lora_cpu import write_adapter

pytestmark = pytest.mark.gpu
GEN = 40


def _check_greedy(model, prompts, outs, tol=0.05, **oracle):
    """The project's near-tie rule: each token is the oracle's argmax, or within tol x the
    logits' standard deviation of it."""
    for p, o in zip(prompts, outs):
        toks, worst = list(p), 0.0
        try:
            for t in o:
                lg = dense_logits(model, toks, **oracle)[-1]
                best = int(lg.argmax())
                gap = float(lg[best] - lg[t])
                worst = max(worst, gap / float(lg.std()))
                assert t == best or gap < tol * float(lg.std()), (len(toks), best, t, gap)
                toks.append(t)
        finally:
            print(f"prompt of {len(p)}: worst accepted-or-failing gap {worst:.4f} of the logits' std (tol {tol})")


@pytest.fixture(scope="module")
def model(gpu):
    return build_model(TINY_LLAMA, device=gpu, seed=3)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]


def _engine(model, graphs=False, dtype="fp8", **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512, num_kv_blocks=128,
               use_graphs=graphs, graph_buckets=(1, 2, 4, 8), kv_cache_dtype=dtype)
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


@pytest.mark.parametrize("graphs", [False, True])
def test_fp8_engine_matches_fake_quant_oracle(model, prompts, graphs):
    eng = _engine(model, graphs)
    assert eng.kv.k[0].dtype == torch.float8_e4m3fn and eng.stats["kv_cache_dtype"] == "fp8"
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert all(len(o) == GEN for o in outs)
    if graphs:
        assert eng.stats["graph_steps"] > 0
    assert eng.stats["mixed_steps"] + eng.stats["prefill_steps"] > 0     # prompt chunks on the 16-row tiles
    assert eng.alloc.num_free == eng.alloc.available - 1                  # every page came back
    _check_greedy(model, prompts, outs, kv_cache_dtype="fp8")


def test_prefix_caching_same_tokens(model):
    g = torch.Generator().manual_seed(5)
    shared = torch.randint(2, 500, (48,), generator=g).tolist()
    reqs = [shared + torch.randint(2, 500, (n,), generator=g).tolist() for n in (7, 21)]
    sp = SamplingParams(max_tokens=16, ignore_eos=True)
    outs = {}
    for on in (True, False):
        eng = _engine(model, enable_prefix_caching=on)
        # one after the other: the second request finds the first one's three full pages
        outs[on] = [eng.generate([r], sp)[0] for r in reqs]
        assert (eng.stats["prefix_hit_tokens"] >= 48) == on
        assert eng.alloc.num_free == eng.alloc.available - 1
    assert outs[True] == outs[False]


def test_same_budget_more_pages(model):
    budget = 6 * 2 ** 20
    kw = dict(num_kv_blocks=None, kv_cache_bytes=budget, max_num_seqs=64, max_model_len=2048, graph_buckets=(1,))
    bf16, fp8 = _engine(model, dtype="bf16", **kw), _engine(model, dtype="fp8", **kw)
    L, Hkv, D = TINY_LLAMA.num_layers, model.n_kv, TINY_LLAMA.head_dim
    per_bf, per_f8 = 2 * L * Hkv * 16 * 2 * D, 2 * L * Hkv * 16 * (D + 1)
    assert bf16.alloc.num_blocks == budget // per_bf
    assert fp8.alloc.num_blocks == budget // per_f8 == (budget * 2 * D) // (per_bf * (D + 1))
    assert fp8.kv.nbytes <= budget < fp8.kv.nbytes + per_f8


def test_no_state_leaks_into_bf16_engines(model, prompts):
    """A bf16 engine built after an fp8 one, in the same process, gives the tokens of one built
    before it: the fp8 path sets no switch."""
    sp = SamplingParams(max_tokens=24, ignore_eos=True)
    before = _engine(model, graphs=True, dtype="bf16").generate(prompts, sp)
    _engine(model, graphs=True).generate(prompts, sp)
    after = _engine(model, graphs=True, dtype="bf16").generate(prompts, sp)
    assert before == after


@pytest.mark.parametrize("graphs", [False, True])
def test_lora_row_under_fp8(model, prompts, tmp_path, graphs):
    """One adapter row and a base row in the same batch (the unfused LoRA forward writes the fp8
    cache too), against the oracle with the adapter merged."""
    d = write_adapter(tmp_path / "r8", TINY_LLAMA, r=8, alpha=8.0, seed=35, std=0.07)
    merged = merged_copy(model, loader.load_adapter(d, TINY_LLAMA))
    eng = _engine(model, graphs, max_adapters=1, max_num_seqs=8)
    eng.load_adapter("r8", d)
    p = prompts[:2]
    outs = eng.generate([p[0], p[1], p[1]], [SamplingParams(max_tokens=24, ignore_eos=True, adapter=a)
                                             for a in ("r8", "r8", None)])
    assert eng.stats["lora_steps"] > 0
    _check_greedy(merged, p, outs[:2], kv_cache_dtype="fp8")
    _check_greedy(model, p[1:], outs[2:], kv_cache_dtype="fp8")
    assert outs[1] != outs[2]
    assert eng.alloc.num_free == eng.alloc.available - 1
