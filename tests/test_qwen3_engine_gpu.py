"""A QK-norm model (tiny-qwen3, every norm weight randomised) through the serving engine on the GPU:
eager and decode graphs, chunked prefill beside decode rows, fp8 KV, a LoRA row, speculation, a
guided request, and a Llama engine in the same process - against the dense fp32 oracle with the
project's near-tie rule (test_model_gpu / test_fp8_kv_engine_gpu: each token is the argmax of the
oracle's last-position logits, or within 0.05 of the row's std of it)."""
import pytest
import torch

from mlopamd.models import build_model, loader
from mlopamd.models.config import TINY_LLAMA, get_config
from mlopamd.models.lora import merged_copy
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.backends import ByteTokenizer
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from test_lora_cpu import write_adapter

pytestmark = pytest.mark.gpu
CFG = get_config("tiny-qwen3")
GEN = 24


def _check_greedy(model, prompts, outs, tol=0.05, **oracle):
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
    m = build_model(CFG, device=gpu, seed=3)
    g = torch.Generator().manual_seed(9)
    noisy = lambda w: w.copy_((1 + 0.2 * torch.randn(w.shape, generator=g)).to(w.device, w.dtype))  # noqa: E731
    with torch.no_grad():
        for L in m.layers:
            for k in ("in_norm", "post_norm", "q_norm", "k_norm"):
                noisy(L[k])
        noisy(m.final_norm)
    m.unit_norms = False
    assert CFG.qk_norm and not torch.equal(m.layers[0]["q_norm"], m.layers[0]["k_norm"])
    return m


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]


def _engine(model, graphs=False, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512, num_kv_blocks=128,
               use_graphs=graphs, graph_buckets=(1, 2, 4, 8))
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


@pytest.mark.parametrize("graphs", [False, True])
def test_engine_matches_dense(model, prompts, graphs):
    eng = _engine(model, graphs)
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert all(len(o) == GEN for o in outs)
    if graphs:
        assert eng.stats["graph_steps"] > 0
    assert eng.alloc.num_free == eng.alloc.available - 1
    _check_greedy(model, prompts, outs)
    # the oracle sees the per-head norm: without it, it is another model
    plain = build_model(TINY_LLAMA, device=model.device, seed=3)
    assert not torch.allclose(dense_logits(model, prompts[0])[-1], dense_logits(plain, prompts[0])[-1], atol=1e-2)


def test_chunked_prefill_beside_decode_rows(model, prompts):
    """16-token chunks: the 150-token prompt is still in prefill while the short ones decode."""
    eng = _engine(model, max_num_batched_tokens=16, mixed_min_chunk=8)
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert eng.stats["mixed_steps"] > 0
    _check_greedy(model, prompts, outs)


@pytest.mark.parametrize("graphs", [False, True])
def test_fp8_kv(model, prompts, graphs):
    eng = _engine(model, graphs, kv_cache_dtype="fp8")
    assert eng.kv.k[0].dtype == torch.float8_e4m3fn
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    _check_greedy(model, prompts, outs, kv_cache_dtype="fp8")
    assert eng.alloc.num_free == eng.alloc.available - 1


@pytest.mark.parametrize("asy", [False, True], ids=["sync", "one-step-ahead"])
def test_prefix_caching_same_tokens(model, asy):
    """A second request that finds the first one's pages (K rows normed and rotated by the writer)
    generates what it generates without the cache, under either scheduling."""
    g = torch.Generator().manual_seed(5)
    shared = torch.randint(2, 500, (48,), generator=g).tolist()
    reqs = [shared + torch.randint(2, 500, (n,), generator=g).tolist() for n in (7, 21)]
    sp = SamplingParams(max_tokens=16, ignore_eos=True)
    outs = {}
    for on in (True, False):
        eng = _engine(model, graphs=True, enable_prefix_caching=on, async_scheduling=asy)
        outs[on] = [eng.generate([r], sp)[0] for r in reqs]
        assert (eng.stats["prefix_hit_tokens"] >= 48) == on
    assert outs[True] == outs[False]


def test_lora_row_beside_a_plain_row(model, prompts, tmp_path):
    d = write_adapter(tmp_path / "r8", CFG, r=8, alpha=8.0, seed=35, std=0.07)
    merged = merged_copy(model, loader.load_adapter(d, CFG))
    eng = _engine(model, max_adapters=1)
    eng.load_adapter("r8", d)
    p = prompts[:2]
    outs = eng.generate([p[0], p[1], p[1]], [SamplingParams(max_tokens=GEN, ignore_eos=True, adapter=a)
                                             for a in ("r8", "r8", None)])
    assert eng.stats["lora_steps"] > 0
    _check_greedy(merged, p, outs[:2])
    _check_greedy(model, p[1:], outs[2:])
    assert outs[1] != outs[2]


def test_speculation_gives_the_same_tokens(model):
    """spec_tokens = 3 against the same engine without speculation: a repeating prompt (so the
    prompt-lookup proposer drafts) and a random one, greedy and seeded."""
    g = torch.Generator().manual_seed(4)
    ps = [list(range(30, 38)) * 6, torch.randint(2, 500, (40,), generator=g).tolist()]
    reqs = [(p, sp) for p in ps for sp in (SamplingParams(max_tokens=GEN, ignore_eos=True),
                                           SamplingParams(max_tokens=GEN, ignore_eos=True, temperature=0.8, top_k=20,
                                                          seed=11))]

    def run(eng):
        return eng.generate([p for p, _ in reqs], [sp for _, sp in reqs])

    base = run(_engine(model, graphs=True))
    eng = _engine(model, graphs=True, spec_tokens=3)
    outs = run(eng)
    assert eng.stats["spec_drafted"] > 0
    assert outs == base


def test_guided_choice_completes(model):
    tok = ByteTokenizer()
    eng = _engine(model, graphs=True, grammar_states=128, max_model_len=128)
    eng.set_tokenizer(tok)
    seqs = [eng.add_request([5, 9, 40], SamplingParams(max_tokens=8, guided={"choice": ["yes", "no", "maybe"]}, **kw))
            for kw in (dict(), dict(temperature=1.5, seed=11))]
    for _ in range(200):
        if not eng.has_work():
            break
        eng.step()
    assert not eng.has_work() and eng.stats["guided_rows"] > 0
    for s in seqs:
        assert s.finish_reason == "stop" and s.output[-1] == CFG.eos_token_id
        assert tok.decode(list(s.output[:-1])) in ("yes", "no", "maybe")


def test_llama_then_qwen3_share_no_state(gpu, model, prompts):
    """A Llama engine's tokens are the same before and after a Qwen3 engine ran in the process."""
    llama = build_model(TINY_LLAMA, device=gpu, seed=3)
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    before = _engine(llama, graphs=True).generate(prompts, sp)
    mine = _engine(model, graphs=True).generate(prompts, sp)
    after = _engine(llama, graphs=True).generate(prompts, sp)
    assert before == after and mine != before
