"""Embedding requests through the serving engine on the GPU (tiny Llama and tiny Qwen3, norm weights
randomised): unchunked and chunked prefill, beside decoding generation rows, both schedulers, fp8 KV,
slots, the prefix cache, and guided / penalised neighbours.

Oracle: ``dense_hidden`` (fp32, no paging, no kernels) pooled by ``pool_reference``.  Error measure of a
vector v against its oracle o: 1 - cos(v, o), and for un-normalised requests also max|v - o| / rms(o).
The bound is measured, not fixed: ``e_direct`` is the same measure for ONE unchunked eager call of the
model's own ``forward`` on the prompt, pooled by the torch reference, its maximum over the prompt set;
every engine vector must stay within 2 x e_direct (the factor: chunked and mixed steps take other GEMM
routes).  Both are printed."""
import numpy as np
import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import get_config
from mlopamd.models.reference import dense_hidden
from mlopamd.ops.reference import (POOL_FIN_MEAN, POOL_FIN_NORMALIZE, POOL_INIT, POOL_LAST, POOL_MODE_LAST,
                                   pool_reference)
from mlopamd.runtime.backends import ByteTokenizer
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from test_qwen3_engine_gpu import _check_greedy

pytestmark = pytest.mark.gpu
GEN = 24


def _noisy_model(name, gpu):
    m = build_model(get_config(name), device=gpu, seed=3)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for w in [L[k] for L in m.layers for k in ("in_norm", "post_norm", "q_norm", "k_norm") if k in L] + [m.final_norm]:
            w.copy_((1 + 0.2 * torch.randn(w.shape, generator=g)).to(w.device, w.dtype))
    m.unit_norms = False
    return m


@pytest.fixture(scope="module")
def models(gpu):
    return {n: _noisy_model(n, gpu) for n in ("tiny-llama", "tiny-qwen3")}


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]


def _engine(model, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=512, max_model_len=512, num_kv_blocks=128, use_graphs=False,
               graph_buckets=(1, 2, 4, 8), embed_slots=4)
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


def _pool(hidden, mode, normalize, dim):
    """float64 [d]: ``hidden`` [T, H] pooled by the torch reference."""
    T, H = hidden.shape
    d = dim or H
    seg = [(0, T, 0, POOL_INIT | POOL_LAST | (0 if mode == "mean" else POOL_MODE_LAST))]
    fin = [(0, T, d, (POOL_FIN_MEAN if mode == "mean" else 0) | (POOL_FIN_NORMALIZE if normalize else 0))]
    return pool_reference(hidden.cpu(), seg, torch.zeros(1, H), fin)[1][0, :d].numpy()


def _err(v, o, normalize):
    v = np.asarray(v, np.float64)
    cos = 1.0 - float(v @ o) / float(np.linalg.norm(v) * np.linalg.norm(o))
    return (cos, 0.0 if normalize else float(np.abs(v - o).max() / np.sqrt(np.mean(o * o))))


_ORACLE, _DIRECT = {}, {}


def _oracle(model, p, mode, normalize, dim, kv=None):
    key = (id(model), tuple(p), kv)
    if key not in _ORACLE:  # computed once, shared and left unchanged
        _ORACLE[key] = dense_hidden(model, p, kv_cache_dtype=kv).cpu()
    return _pool(_ORACLE[key], mode, normalize, dim)


def _direct_hidden(model, p, kv):
    """The model's own forward on the whole prompt in one eager call (no chunking, no cached prefix)."""
    key = (id(model), tuple(p), kv)
    if key not in _DIRECT:
        eng = _engine(model, embed_slots=0, enable_prefix_caching=False, **({"kv_cache_dtype": kv} if kv else {}))
        eng.add_request(p, SamplingParams(max_tokens=1))
        st = eng._build_step(False, True, eng.r_last)
        assert st.chunks == [len(p)]
        _, T, nt, nl, part, nparts, _ = st.launch
        eng.meta.upload(T, nl, eng.rows_hi)
        hidden = model.forward(eng.meta.ids_d[:T], eng.meta.meta(T, nt, nl, part, nparts, eng.meta.npt), eng.kv)
        _DIRECT[key] = hidden.float().cpu()
    return _DIRECT[key]


def _bound(model, ps, mode, normalize, dim, kv=None):
    e = [_err(_pool(_direct_hidden(model, p, kv), mode, normalize, dim), _oracle(model, p, mode, normalize, dim, kv),
              normalize) for p in ps]
    return tuple(max(x[i] for x in e) for i in range(2))


def _check(model, ps, vecs, mode, normalize=True, dim=None, kv=None, what=""):
    e_direct = _bound(model, ps, mode, normalize, dim, kv)
    for p, v in zip(ps, vecs):
        assert v.dtype == np.float32 and v.shape == (dim or model.cfg.hidden_size,)
        e = _err(v, _oracle(model, p, mode, normalize, dim, kv), normalize)
        print(f"{what} {model.cfg.name} {mode} norm={normalize} dim={dim} kv={kv} T={len(p)}: engine 1-cos {e[0]:.3e} "
              f"rel {e[1]:.3e} | e_direct 1-cos {e_direct[0]:.3e} rel {e_direct[1]:.3e}")
        assert e[0] <= 2 * e_direct[0] and e[1] <= 2 * e_direct[1], (e, e_direct)
        if normalize:
            assert abs(float(np.linalg.norm(v.astype(np.float64))) - 1) < 1e-5


@pytest.mark.parametrize("budget", (512, 48), ids=("unchunked", "chunked"))
@pytest.mark.parametrize("mode", ("last", "mean"))
@pytest.mark.parametrize("name", ("tiny-llama", "tiny-qwen3"))
def test_matches_dense_hidden(models, prompts, name, mode, budget):
    """Whole prompts and 48-token chunks (4 of the 150-token prompt); the full normalised vector and
    a raw one cut to 64 components."""
    model = models[name]
    eng = _engine(model, max_num_batched_tokens=budget, enable_prefix_caching=False)
    full = eng.embed(prompts, mode)
    cut = eng.embed(prompts, mode, normalize=False, dim=64)
    assert eng.stats["embed_requests"] == 6 and eng.stats["embed_tokens"] == 2 * sum(map(len, prompts))
    assert eng.stats["embed_steps"] >= (8 if budget == 48 else 2)
    assert eng.alloc.num_free == eng.alloc.available - 1 and len(eng._free_embed) == 4
    _check(model, prompts, full, mode, what="full")
    _check(model, prompts, cut, mode, normalize=False, dim=64, what="cut")


@pytest.mark.parametrize("mode", ("last", "mean"))
def test_input_that_fills_the_context(models, prompts, mode):
    """An embedding input may be exactly max_model_len tokens (no token is generated); one more is refused."""
    model = models["tiny-qwen3"]
    eng = _engine(model, max_model_len=150, max_num_batched_tokens=48, enable_prefix_caching=False)
    _check(model, prompts[2:], eng.embed(prompts[2:], mode), mode, what="full context")
    with pytest.raises(ValueError, match="exceeds max_model_len"):
        eng.add_request(prompts[2] + [5], SamplingParams(embed=mode))
    with pytest.raises(ValueError, match="exceeds max_model_len"):
        eng.add_request(prompts[2], SamplingParams(max_tokens=1))
    assert eng.alloc.num_free == eng.alloc.available - 1


@pytest.mark.parametrize("mode", ("last", "mean"))
def test_fp8_kv(models, prompts, mode):
    model = models["tiny-qwen3"]
    eng = _engine(model, max_num_batched_tokens=48, kv_cache_dtype="fp8", enable_prefix_caching=False)
    assert eng.kv.k[0].dtype == torch.float8_e4m3fn
    _check(model, prompts, eng.embed(prompts, mode), mode, kv="fp8", what="fp8")


def _drive(eng, reqs, after=3):
    """Generation requests first, ``after`` steps, then the others; everything to completion."""
    gen = [eng.add_request(p, sp) for p, sp in reqs if sp.embed is None]
    outs = []
    for _ in range(after):
        outs += list(eng.step())
    emb = [eng.add_request(p, sp) for p, sp in reqs if sp.embed is not None]
    for _ in range(2000):
        if not eng.has_work():
            break
        outs += list(eng.step())
    assert not eng.has_work()
    return gen, emb, outs


@pytest.mark.parametrize("asy", (False, True), ids=("sync", "one-step-ahead"))
@pytest.mark.parametrize("name", ("tiny-llama", "tiny-qwen3"))
def test_beside_decoding_rows(models, prompts, name, asy):
    """Embedding requests arrive while generation rows decode: their chunks ride in mixed steps; the
    generated tokens pass the dense-oracle greedy check, the vectors the bound, under either
    scheduler, with the same finish reasons."""
    model = models[name]
    eng = _engine(model, max_num_batched_tokens=32, mixed_min_chunk=8, async_scheduling=asy)
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    reqs = [(p, sp) for p in prompts[:2]] + [(p, SamplingParams(embed=m)) for m in ("last", "mean") for p in prompts]
    gen, emb, outs = _drive(eng, reqs)
    assert eng.stats["mixed_steps"] > 0 and eng.stats["embed_steps"] > 0
    assert [s.finish_reason for s in gen] == ["length"] * 2 and [s.finish_reason for s in emb] == ["embedding"] * 6
    fin = {o.seq_id: o for o in outs if o.finished}
    for s in emb:
        o = fin[s.seq_id]
        assert o.token == -1 and o.finish_reason == "embedding" and o.embedding is s.embedding and not s.output
    _check_greedy(model, prompts[:2], [s.output for s in gen])
    # ("last" requests may find the generation prompts' pages in the prefix cache: still the same vector)
    _check(model, prompts, [s.embedding for s in emb[:3]], "last", what="mixed")
    _check(model, prompts, [s.embedding for s in emb[3:]], "mean", what="mixed")
    assert eng.alloc.num_free == eng.alloc.available - 1 and len(eng._free_embed) == 4


def test_two_slots_serve_five_requests(models, prompts):
    model = models["tiny-llama"]
    eng = _engine(model, embed_slots=2, max_num_batched_tokens=48)
    ps = [prompts[i % 3] for i in range(5)]
    seqs = [eng.add_request(p, SamplingParams(embed="mean")) for p in ps]
    gen = eng.add_request(prompts[0], SamplingParams(max_tokens=4, ignore_eos=True))  # behind them: needs no slot
    for _ in range(500):
        if not eng.has_work():
            break
        eng.step()
    assert all(s.finish_reason == "embedding" for s in seqs) and len(gen.output) == 4
    assert eng.alloc.num_free == eng.alloc.available - 1 and sorted(eng._free_embed) == [0, 1]
    _check(model, ps, [s.embedding for s in seqs], "mean", what="slots")


def test_prefix_cache(models):
    model = models["tiny-qwen3"]
    g = torch.Generator().manual_seed(5)
    shared = torch.randint(2, 500, (48,), generator=g).tolist()
    reqs = [shared + torch.randint(2, 500, (n,), generator=g).tolist() for n in (7, 21)]
    vec = {}
    for on in (True, False):
        eng = _engine(model, enable_prefix_caching=on)
        vec[on] = [eng.embed([r], "last")[0] for r in reqs]
        assert (eng.stats["prefix_hit_tokens"] >= 48) == on
        hits = eng.stats["prefix_hit_tokens"]
        mean = eng.embed([reqs[1]], "mean")[0]
        assert eng.stats["prefix_hit_tokens"] == hits  # mean pooling computes every token
        _check(model, reqs[1:], [mean], "mean", what=f"prefix cache {on}")
        _check(model, reqs, vec[on], "last", what=f"prefix cache {on}")


def test_guided_and_penalised_neighbours(models, prompts):
    """A guided and a penalised request complete beside embeddings as they do alone."""
    model = models["tiny-llama"]
    tok = ByteTokenizer()
    sps = [SamplingParams(max_tokens=8, guided={"choice": ["yes", "no", "maybe"]}),
           SamplingParams(max_tokens=12, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5)]

    def run(with_embeddings):
        eng = _engine(model, grammar_states=128, max_model_len=256, max_num_batched_tokens=32, mixed_min_chunk=8)
        eng.set_tokenizer(tok)
        reqs = [([5, 9, 40], sps[0]), (prompts[0], sps[1])]
        if with_embeddings:
            reqs += [(p, SamplingParams(embed=m)) for m in ("last", "mean") for p in prompts]
        gen, emb, _ = _drive(eng, reqs, after=1)
        return [(s.output, s.finish_reason) for s in gen], emb

    alone, _ = run(False)
    beside, emb = run(True)
    assert beside == alone and tok.decode(list(alone[0][0][:-1])) in ("yes", "no", "maybe")
    _check(model, prompts, [s.embedding for s in emb[:3]], "last", what="neighbours")
    _check(model, prompts, [s.embedding for s in emb[3:]], "mean", what="neighbours")
