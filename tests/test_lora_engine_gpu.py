"""Multi-LoRA serving end to end on the GPU: three adapters and base requests in one continuous
batch (prefill chunks that mix adapters inside a 16-token tile, eager and graph decode), against
the dense oracle on copies of the model with W + B.A merged in.

Adapters: A, B ~ N(0, 0.07^2), alpha = r, so the delta is about as large as the base weights
(std 0.02) and every adapter's greedy continuation leaves the base model's.  The seeds were picked
on the CPU (fp32 math on the bf16 weights) so that along the oracle's own greedy path at most 3
of the 24 positions per (prompt, adapter) are near-ties (gap < 0.05 std): rank 8 seed 35 ->
3 / 2 / 0 near-ties on the 10 / 60 / 150-token prompts, rank 16 seed 17 -> 3 / 3 / 0, rank 64
seed 26 -> 2 / 1 / 0.
"""
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

ADAPTERS = {"r8": (8, 35), "r16": (16, 17), "r64": (64, 26)}  # name -> (rank, seed)
GEN = 24
TOL = 0.05


@pytest.fixture(scope="module")
def setup(gpu, tmp_path_factory):
    root = tmp_path_factory.mktemp("lora")
    torch.manual_seed(0)
    model = build_model(TINY_LLAMA, device=gpu, seed=3)
    dirs = {n: write_adapter(root / n, TINY_LLAMA, r=r, alpha=float(r), seed=s, std=0.07)
            for n, (r, s) in ADAPTERS.items()}
    oracle = {n: merged_copy(model, loader.load_adapter(d, TINY_LLAMA)) for n, d in dirs.items()}
    oracle[None] = model
    g = torch.Generator().manual_seed(21)
    prompts = [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]
    cache = {}

    def last_logits(name, toks):
        key = (name, tuple(toks))
        if key not in cache:
            cache[key] = dense_logits(oracle[name], toks)[-1]
        return cache[key]

    return model, dirs, prompts, last_logits


def _engine(model, dirs, graphs, **kw):
    cfg = dict(max_num_seqs=16, max_num_batched_tokens=64, max_model_len=512, num_kv_blocks=256,
               use_graphs=graphs, graph_buckets=(1, 2, 4, 8), max_adapters=3)
    cfg.update(kw)
    eng = Engine(model, EngineConfig(**cfg))
    if cfg["max_adapters"]:
        for n, d in dirs.items():
            eng.load_adapter(n, d)
    return eng


def test_oracle_paths_differ(setup):
    """The tolerance below cannot hide a wrong or missing adapter: for every prompt each adapter's
    oracle continuation differs from the base model's and from the other adapters'."""
    _, _, prompts, last_logits = setup
    for p in prompts:
        paths = {}
        for name in (None, *ADAPTERS):
            toks = list(p)
            for _ in range(GEN):
                toks.append(int(last_logits(name, toks).argmax()))
            paths[name] = tuple(toks[len(p):])
        assert len(set(paths.values())) == len(paths), paths


@pytest.mark.parametrize("graphs", [False, True])
def test_mixed_adapters_match_merged_oracle(setup, graphs):
    model, dirs, prompts, last_logits = setup
    eng = _engine(model, dirs, graphs)
    names = [None, *ADAPTERS]
    reqs = [(p, n) for p in prompts for n in names]  # 12 requests: chunks mix adapters inside a tile
    outs = eng.generate([p for p, _ in reqs],
                        [SamplingParams(max_tokens=GEN, ignore_eos=True, adapter=n) for _, n in reqs])
    assert eng.stats["lora_steps"] > 0 and eng.stats["mixed_steps"] + eng.stats["prefill_steps"] > 0
    if graphs:
        assert eng.stats["graph_steps"] > 0 and eng.stats["lora_graph_steps"] > 0
    else:
        assert eng.stats["lora_graph_steps"] == 0
    for (p, name), out in zip(reqs, outs):
        assert len(out) == GEN
        toks, soft = list(p), 0
        for t in out:
            lg = last_logits(name, toks)
            best = int(lg.argmax())
            gap = float(lg[best] - lg[t])
            assert t == best or gap < TOL * float(lg.std()), (name, len(p), len(toks), best, t, gap)
            soft += t != best
            toks.append(t)
        print(f"graphs={graphs} prompt {len(p)} adapter {name}: {soft}/{GEN} near-tie tokens accepted")
        assert soft <= GEN // 4, (name, len(p), soft)
    assert eng.alloc.num_free == eng.alloc.available - 1, "every KV page returns"
    assert not eng._slot_refs.any()


@pytest.mark.parametrize("graphs", [False, True])
def test_base_only_requests_equal_feature_off(setup, graphs):
    """Adapters loaded, none requested: exactly the tokens of an engine without the feature
    (the adapter-free path, decode graphs included)."""
    model, dirs, prompts, _ = setup
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    on = _engine(model, dirs, graphs)
    off = _engine(model, dirs, graphs, max_adapters=0)
    assert off.lora is None and not off.graphs_lora and off.meta.total == on.meta.total
    assert on.generate(prompts, sp) == off.generate(prompts, sp)
    assert on.stats["lora_steps"] == 0
    if graphs:
        assert len(on.graphs_lora) == len(on.graphs) > 0 and on.stats["graph_steps"] > 0
    assert on.alloc.num_free == on.alloc.available - 1
