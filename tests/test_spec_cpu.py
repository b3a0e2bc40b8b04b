"""Speculative decoding by prompt lookup on CPU: the contract of runtime/spec.py, the engine with
speculation on against the same engine with it off (exact tokens and finish reasons, under
forced proposers and the n-gram proposer), and the control plane's spec.speculativeTokens."""
import types

import numpy as np
import pytest
import torch
import yaml

from mlopamd.controller import crd
from mlopamd.controller.kube import ApiError
from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_MIXTRAL
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from mlopamd.runtime.spec import accept_reference, propose_reference

# ---------------------------------------------------------------- contract --


def test_propose_no_room_and_shortest_histories():
    assert propose_reference([5], 4, 3, 1) == []                 # L = n_min: the suffix is all there is
    assert propose_reference([5, 6], 4, 3, 2) == []              # L = n_min (2)
    assert propose_reference([5, 5], 4, 3, 1) == [5]             # L = n_min + 1: p = 0, one follower
    assert propose_reference([5, 6], 4, 3, 1) == []              # L = n_min + 1, no match
    assert propose_reference([1, 2, 1, 2, 1, 2], 3, 8, 8) == []  # L < n + 1 for every n


def test_propose_match_positions():
    # only at p = 0
    assert propose_reference([1, 2, 3, 9, 8, 7, 1, 2, 3], 2, 3, 1) == [9, 8]
    assert propose_reference([1, 2, 3, 9, 8, 7, 1, 2, 3], 7, 3, 1) == [9, 8, 7, 1, 2, 3]  # fewer than cap followers
    # a match ending at L - 2 (p = L - n - 1): it overlaps the suffix, one follower
    assert propose_reference([9, 4, 4, 4], 3, 2, 2) == [4]
    assert propose_reference([3, 9, 4, 4], 3, 1, 1) == [4]


def test_propose_competing_matches():
    #    0  1  2  3  4  5  6  7  8  9 10
    h = [1, 2, 7, 7, 7, 7, 1, 2, 8, 1, 2]
    # n = 2: p = 0 (followers 7 7 7 7 ...) and p = 6 (followers 8 1 2).  cap 3: both can supply 3,
    # the most recent wins; cap 4: only p = 0 can
    assert propose_reference(h, 3, 2, 2) == [8, 1, 2]
    assert propose_reference(h, 4, 2, 2) == [7, 7, 7, 7]
    assert propose_reference(h, 1, 2, 2) == [8]
    # no candidate supplies cap: the smallest p (the most followers)
    assert propose_reference([1, 2, 5, 1, 2, 6, 1, 2], 7, 2, 2) == [5, 1, 2, 6, 1, 2]


def test_propose_fallback_to_shorter_ngram():
    h = [4, 2, 3, 9, 1, 2, 3]          # "1 2 3" never occurred before, "2 3" did
    assert propose_reference(h, 2, 3, 1) == [9, 1]
    assert propose_reference(h, 2, 3, 3) == []                   # n_min = 3 forbids the fallback
    assert propose_reference([5, 1, 3, 6, 2, 3], 1, 3, 2) == []  # only a 1-gram matches, n_min = 2
    assert propose_reference([5, 1, 3, 6, 2, 3], 1, 3, 1) == [6]


def test_propose_period_one_and_caps():
    a = [7, 7, 7, 7]
    assert propose_reference(a, 0, 3, 1) == []
    assert propose_reference(a, 1, 3, 1) == [7]                  # n = 3: p = 0 only (p + 3 + 1 <= 4)
    assert propose_reference(a, 7, 3, 1) == [7]                  # no full-follow candidate: smallest p
    assert propose_reference([7] * 12, 7, 3, 1) == [7] * 7       # the largest p with p + 3 + 7 <= 12: p = 2
    assert propose_reference([7] * 12, 1, 3, 1) == [7]


def test_accept_reference():
    assert accept_reference([5], [], 0) == [5]                                  # nd = 0: a plain row
    assert accept_reference([5, 6, 7, 8], [5, 6, 7], 3) == [5, 6, 7, 8]         # all accepted + the bonus token
    assert accept_reference([5, 6, 7, 8], [9, 6, 7], 3) == [5]                  # first rejected: later matches do not count
    for j in range(4):                                                          # the first mismatch at each j
        d = [10, 11, 12, 13]
        s = d + [14]
        d[j] = 99
        assert accept_reference(s, d, 4) == s[:j + 1]
    assert accept_reference([5, 6, 7], [5, 6, 0, 0], 2) == [5, 6, 7]            # drafts beyond nd are ignored


# ------------------------------------------------------------------ engine --

V = TINY_LLAMA.vocab_size
GEN = 16


@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return build_model(TINY_LLAMA, device="cpu", dtype=torch.float32, seed=1)


def _cfg(**kw):
    base = dict(max_num_seqs=6, max_num_batched_tokens=48, max_model_len=256, num_kv_blocks=96, use_graphs=False,
                mixed_min_chunk=8)
    base.update(kw)
    return EngineConfig(**base)


@pytest.fixture(scope="module")
def work(tiny):
    """Prompts (three of them a repeated segment), their sampling parameters and the spec-off
    engine's outputs.  Stop tokens are taken from a probe run so that they fire, some of them in
    the middle of what an always-right proposer gets accepted in one step."""
    rng = np.random.default_rng(5)
    seg = rng.integers(2, 500, size=6).tolist()
    prompts = [seg * 5, rng.integers(2, 500, size=33).tolist(), (seg * 4)[:19], rng.integers(2, 500, size=9).tolist(),
               seg[:3] * 8, rng.integers(2, 500, size=50).tolist(), rng.integers(2, 500, size=14).tolist(),
               rng.integers(2, 500, size=21).tolist()]

    def params(stops):
        return [
            SamplingParams(max_tokens=GEN, ignore_eos=True),
            SamplingParams(max_tokens=GEN, ignore_eos=True, temperature=0.9, top_k=40, seed=1234),
            SamplingParams(max_tokens=11, ignore_eos=True),                              # max_tokens mid-run
            SamplingParams(max_tokens=GEN, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.2),
            SamplingParams(max_tokens=GEN, ignore_eos=True, stop_token_ids=stops[4]),
            SamplingParams(max_tokens=7, ignore_eos=True, temperature=0.7, top_p=0.9, seed=99),
            SamplingParams(max_tokens=GEN, ignore_eos=True, logprobs=2),
            SamplingParams(max_tokens=GEN, ignore_eos=True, stop_token_ids=stops[7]),
        ]

    none = [[] for _ in prompts]
    probe = Engine(tiny, _cfg()).generate(prompts, params(none))
    stops = list(none)
    stops[4], stops[7] = [probe[4][6]], [probe[7][3]]
    ps = params(stops)
    eng = Engine(tiny, _cfg())
    seqs = _drive(eng, prompts, ps)
    base = [(s.output, s.finish_reason) for s in seqs]
    assert [r for _, r in base].count("stop") >= 2 and [r for _, r in base].count("length") >= 4
    return prompts, ps, base


def _drive(eng, prompts, ps):
    """Requests arrive while others decode (mixed steps admit prompts in the middle)."""
    seqs, i, it = [], 0, 0
    while i < len(prompts) or eng.has_work():
        if i < len(prompts) and it % 3 == 0:
            seqs.append(eng.add_request(prompts[i], ps[i]))
            i += 1
        eng.step()
        it += 1
    return seqs


def _proposer(kind, k, prompts, base):
    ref = {tuple(p): out for p, (out, _) in zip(prompts, base)}
    calls = [0]

    def propose(seq, cap):
        r, n = ref[tuple(seq.prompt)], len(seq.output)
        assert seq.output == r[:n], "the sequence is on the spec-off path"
        right = r[n:n + cap]
        wrong = [(t + 1) % V for t in right] + [3] * (cap - len(right))
        calls[0] += 1
        if kind == "right":
            return right
        if kind == "wrong":
            return wrong
        m = calls[0] % (k + 1)   # cycle: right for m tokens, then wrong
        return right[:m] + wrong[m:]

    return propose


# tight: admission waits for pages and rows lose their drafts when the allocator has none to give
POOLS = {"roomy": dict(num_kv_blocks=96), "tight": dict(num_kv_blocks=8, max_num_seqs=5)}


@pytest.mark.parametrize("pool", list(POOLS))
@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("kind", ["right", "wrong", "cycle", "ngram"])
def test_spec_on_equals_spec_off(tiny, work, kind, k, pool):
    """Greedy, seeded, penalised and log-probability rows, stop tokens inside an accepted run,
    max_tokens reached mid-run, prompts admitted in the middle, a roomy and a tight page pool:
    the tokens and finish reasons of spec_tokens = 0, whatever the proposer proposes."""
    prompts, ps, base = work
    eng = Engine(tiny, _cfg(spec_tokens=k, **POOLS[pool]))
    assert eng.stats["spec_async_off"] == 1 and not eng._async
    if kind != "ngram":
        eng.spec_proposer = _proposer(kind, k, prompts, base)
    seqs = _drive(eng, prompts, ps)
    got = [(s.output, s.finish_reason) for s in seqs]
    assert got == base
    st = eng.stats
    assert eng.alloc.num_free == eng.alloc.available - 1, "every KV page returns"
    assert st["spec_drafted"] > 0 and st["spec_steps"] > 0 and st["spec_graph_steps"] == 0
    assert 0 <= st["spec_accepted"] <= st["spec_drafted"]
    if kind == "wrong":
        assert st["spec_accepted"] == 0
    if kind == "right":
        # (the penalised and the log-probability rows never draft)
        assert st["spec_accepted"] == st["spec_drafted"]
    if kind == "cycle" and k > 1:
        assert 0 < st["spec_accepted"] < st["spec_drafted"]
    # log-probabilities ride along unchanged
    assert len(seqs[6].logprobs) == len(seqs[6].output)


@pytest.mark.parametrize("kind", ["right", "wrong", "cycle", "ngram"])
def test_preemption_by_a_small_page_pool(tiny, kind):
    """Four sequences that grow from 2 to 5 pages each in a pool of 12: the newest are preempted,
    recomputed and re-admitted (their history is rebuilt from prompt + output so far)."""
    rng = np.random.default_rng(8)
    seg = rng.integers(2, 500, size=5).tolist()
    prompts = [seg * 5 + [7], rng.integers(2, 500, size=28).tolist(), (seg * 6)[:27], rng.integers(2, 500, size=30).tolist()]
    sp = [SamplingParams(max_tokens=40, ignore_eos=True),
          SamplingParams(max_tokens=40, ignore_eos=True, temperature=0.8, top_k=30, seed=7),
          SamplingParams(max_tokens=40, ignore_eos=True), SamplingParams(max_tokens=40, ignore_eos=True)]
    off = Engine(tiny, _cfg(num_kv_blocks=13))
    outs = off.generate(prompts, sp)
    assert off.stats["preemptions"] > 0
    on = Engine(tiny, _cfg(num_kv_blocks=13, spec_tokens=4))
    if kind != "ngram":
        on.spec_proposer = _proposer(kind, 4, prompts, [(o, "length") for o in outs])
    assert on.generate(prompts, sp) == outs
    assert on.stats["preemptions"] > 0 and on.stats["spec_drafted"] > 0
    assert on.alloc.num_free == on.alloc.available - 1


def test_spec_off_allocates_nothing(tiny):
    eng = Engine(tiny, _cfg())
    assert eng.spec_k == 0 and not hasattr(eng, "hist") and not eng.graphs_spec
    assert not any(k.startswith("spec_") for k in eng.stats)
    on = Engine(tiny, _cfg(spec_tokens=4))
    assert on.hist.shape == (6, 256) and on.hist.dtype == torch.int32 and on.hist_len.shape == (6,)
    # the metadata layout only grows where the verify step needs it
    assert Engine(tiny, _cfg(async_scheduling=False)).meta.total == eng.meta.total <= on.meta.total


def test_fewer_steps_when_drafts_are_right(tiny, work):
    prompts, ps, base = work
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    off = Engine(tiny, _cfg())
    outs = off.generate(prompts[:1], sp)
    ref = {tuple(p): o for p, o in zip(prompts, outs)}
    on = Engine(tiny, _cfg(spec_tokens=4))
    on.spec_proposer = lambda seq, cap: ref[tuple(seq.prompt)][len(seq.output):len(seq.output) + cap]
    assert on.generate(prompts[:1], sp) == outs
    # GEN - 1 decode tokens per sequence, 5 per verify step
    assert on.stats["decode_steps"] == -(-(GEN - 1) // 5) < off.stats["decode_steps"] == GEN - 1
    assert on.stats["spec_accepted"] == on.stats["spec_drafted"]
    assert on.stats["decode_tokens"] == off.stats["decode_tokens"]


def test_large_batches_run_unspeculated(tiny, work):
    prompts, _, _ = work
    sp = SamplingParams(max_tokens=6, ignore_eos=True)
    eng = Engine(tiny, _cfg(spec_tokens=4, spec_max_batch=2))
    eng.spec_proposer = lambda seq, cap: [5] * cap
    outs = eng.generate(prompts[:4], sp)
    assert outs == Engine(tiny, _cfg()).generate(prompts[:4], sp)
    assert eng.stats["spec_steps"] == 0 and eng.stats["decode_steps"] > 0   # 4 rows decode together


@pytest.mark.parametrize("kw,model,word", [
    (dict(kv_cache_dtype="fp8"), None, "fp8"),
    (dict(max_adapters=2), None, "adapters"),
    (dict(), "moe", "MoE"),
    (dict(), "swa", "sliding-window"),
    (dict(), "tp", "parallelism"),
    (dict(), "ep", "parallelism"),
    (dict(spec_tokens=8), None, "spec_tokens"),
    (dict(spec_ngram_min=0), None, "spec_ngram_min"),
    (dict(spec_ngram_max=9), None, "spec_ngram_min"),
    (dict(spec_ngram_min=3, spec_ngram_max=2), None, "spec_ngram_min"),
])
def test_construction_rejects_unsupported(tiny, kw, model, word):
    m = tiny
    if model == "moe":
        m = build_model(TINY_MIXTRAL, device="cpu", dtype=torch.float32, seed=1)
    elif model == "swa":
        from dataclasses import replace

        m = build_model(replace(TINY_LLAMA, sliding_window=64), device="cpu", dtype=torch.float32, seed=1)
    elif model in ("tp", "ep"):
        size = {"tp": (2, 1), "ep": (1, 2)}[model]
        ps = types.SimpleNamespace(tp=types.SimpleNamespace(size=size[0]), ep=types.SimpleNamespace(size=size[1]))
        m = types.SimpleNamespace(device=tiny.device, cfg=tiny.cfg, ps=ps)
    with pytest.raises(ValueError, match=word):
        Engine(m, _cfg(**{"spec_tokens": 2, **kw}))


# ----------------------------------------------------------- control plane --

def _cr(**spec):
    return {"apiVersion": "mlflow.nizepart.com/v1alpha1", "kind": "MlflowModel", "metadata": {"name": "x"},
            "spec": dict({"modelName": "m", "modelAlias": "a"}, **spec)}


def test_crd_field():
    schema = crd.crd_schema()
    assert crd.ModelSpec.from_spec(_cr()["spec"]).speculative_tokens is None
    for k in (0, 1, 7):
        pruned, errs = crd.admit(_cr(speculativeTokens=k), schema)
        assert errs == [] and pruned["spec"]["speculativeTokens"] == k
        spec = crd.ModelSpec.from_spec(pruned["spec"])
        assert spec.speculative_tokens == k and spec.validate() == []
    prop = schema["properties"]["spec"]["properties"]["speculativeTokens"]
    assert (prop["type"], prop["minimum"], prop["maximum"]) == ("integer", 0, crd.MAX_SPECULATIVE_TOKENS)
    for bad in (8, -1, "4"):
        _, errs = crd.admit(_cr(speculativeTokens=bad), schema)
        assert any("speculativeTokens" in e for e in errs), bad
        assert any("speculativeTokens" in e for e in crd.ModelSpec.from_spec(_cr(speculativeTokens=bad)["spec"]).validate())
    for extra, word in ((dict(tensorParallel=2), "tensorParallel"), (dict(expertParallel=2), "expertParallel"),
                        (dict(kvCacheDtype="fp8"), "fp8"),
                        (dict(adapters=[{"name": "a", "uri": "file:///a"}]), "adapters")):
        errs = crd.ModelSpec.from_spec(_cr(speculativeTokens=3, **extra)["spec"]).validate()
        assert any("speculativeTokens" in e and word in e for e in errs), (extra, errs)
        assert crd.ModelSpec.from_spec(_cr(speculativeTokens=0, **extra)["spec"]).validate() == []


def test_example_cr_admits():
    with open(crd.MANIFESTS / "examples" / "speculative" / "llama3-8b-speculative.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr)
    assert errs == [] and pruned == cr
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert spec.validate() == [] and spec.speculative_tokens == 4


def test_operator_passes_spec_tokens_to_the_engine():
    from test_controller import Env, _ready, run

    async def go():
        env = Env()
        v = env.version(tags={"mlop.architecture": "llama3-8b"})
        env.reg.set_alias("m", "champion", v)
        await env.start()
        with pytest.raises(ApiError) as bad:                               # the apiserver's schema: 422
            await env.create_cr(tensorParallel=1, speculativeTokens=9)
        assert bad.value.status == 422 and "speculativeTokens" in bad.value.message
        await env.create_cr(tensorParallel=1, speculativeTokens=4)
        assert await env.run_until(lambda: _ready(env))
        assert "error" not in await env.status()
        (p,) = (await env.sd())["spec"]["predictors"]
        e = {x["name"]: x["value"] for x in p["componentSpecs"][0]["spec"]["containers"][0]["env"]}
        assert e["MLOP_ENGINE_SPEC_TOKENS"] == "4"
        await env.stop()

        env = Env()                                                        # without the field, or 0: no env entry
        v = env.version(tags={"mlop.architecture": "llama3-8b"})
        env.reg.set_alias("m", "champion", v)
        await env.start()
        await env.create_cr(tensorParallel=1, speculativeTokens=0)
        assert await env.run_until(lambda: _ready(env))
        (p,) = (await env.sd())["spec"]["predictors"]
        assert "MLOP_ENGINE_SPEC_TOKENS" not in [x["name"] for x in p["componentSpecs"][0]["spec"]["containers"][0]["env"]]
        await env.stop()
    run(go())


def test_server_env_and_metrics(tiny, work):
    import os

    from mlopamd.runtime.metrics import RuntimeMetrics
    from mlopamd.runtime.server import engine_kwargs_from_env

    os.environ["MLOP_ENGINE_SPEC_TOKENS"] = "4"
    os.environ["MLOP_ENGINE_SPEC_NGRAM_MAX"] = "5"
    try:
        kw = engine_kwargs_from_env()
        assert kw["spec_tokens"] == 4 and kw["spec_ngram_max"] == 5
    finally:
        del os.environ["MLOP_ENGINE_SPEC_TOKENS"], os.environ["MLOP_ENGINE_SPEC_NGRAM_MAX"]
    met = RuntimeMetrics()
    met.mark_spec(10, 4)
    met.mark_spec(25, 9)
    text = met.exposition().decode()
    val = {ln.split("{")[0]: float(ln.rsplit(" ", 1)[1]) for ln in text.splitlines() if ln.startswith("mlop_spec_")
           and "_total{" in ln}
    assert val == {"mlop_spec_draft_tokens_total": 25.0, "mlop_spec_accepted_tokens_total": 9.0}
