"""Speculative decoding end to end on the GPU: verify steps (eager and the third graph family) with
forced proposers and the device n-gram proposer, against the dense oracle.

A verify step runs its GEMMs at M = rows x (k + 1), so its bf16 logits differ from a plain decode
step's in the last bits and exact equality with spec_tokens = 0 is a CPU statement
(test_spec_cpu.py).  Here every greedy token is checked teacher-forced against ``dense_logits`` with
test_lora_engine_gpu.py's rule: it is the oracle's argmax, or its gap to it is below 0.05 x the
row's std (a near-tie), at most GEN // 4 such tokens per sequence.

The weights are drawn on the CPU (model seed 1) and copied to the GPU model, and the prompts come
from generator seed 23, both picked on the CPU (fp32 math on the bf16 weights) so that the oracle's
own greedy path has few near-ties (top-2 gap < 0.05 std) in its 24 positions: 0 / 0 / 3 / 0 on the
10-token, the 60-token (a 12-token segment five times), the 150-token and the 33-token prompt.
On the MI355X the engine's runs accepted 0 near-tie tokens per sequence on the 10 / 60 / 33-token
prompts and 0-1 on the 150-token one, with every proposer, k and graphs on or off.
"""
import math

import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.attn_meta import MetaBuffers
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams, sample_reference, seeded_uniform

pytestmark = pytest.mark.gpu

GEN = 24
TOL = 0.05
V = TINY_LLAMA.vocab_size


@pytest.fixture(scope="module")
def setup(gpu):
    torch.manual_seed(0)
    host = build_model(TINY_LLAMA, device="cpu", seed=1)
    model = build_model(TINY_LLAMA, device=gpu, seed=1)
    for dst, src in zip(model.weight_tensors(), host.weight_tensors()):
        dst.copy_(src)
    g = torch.Generator().manual_seed(23)
    seg = torch.randint(2, 500, (12,), generator=g).tolist()
    prompts = [torch.randint(2, 500, (10,), generator=g).tolist(), seg * 5,
               torch.randint(2, 500, (150,), generator=g).tolist(), torch.randint(2, 500, (33,), generator=g).tolist()]
    cache = {}

    def last_logits(toks):
        key = tuple(toks)
        if key not in cache:
            cache[key] = dense_logits(model, toks)[-1].cpu()
        return cache[key]

    return model, prompts, last_logits


def _engine(model, graphs, k, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512, num_kv_blocks=256,
               use_graphs=graphs, graph_buckets=(1, 2, 4, 8), mixed_min_chunk=16, spec_tokens=k)
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


def _oracle_drafts(last_logits, toks, cap):
    """The oracle's greedy continuation of ``toks``, teacher-forced on the actual prefix."""
    toks, out = list(toks), []
    for _ in range(cap):
        out.append(int(last_logits(toks).argmax()))
        toks.append(out[-1])
    return out


def _proposer(kind, k, last_logits):
    calls = [0]

    def propose(seq, cap):
        right = _oracle_drafts(last_logits, seq.prompt + seq.output, cap)
        wrong = [(t + 1) % V for t in right]
        calls[0] += 1
        if kind == "right":
            return right
        if kind == "wrong":
            return wrong
        m = calls[0] % (k + 1)  # cycle: right for m tokens, then wrong, so every accept length occurs
        return right[:m] + wrong[m:]

    return propose


def _check_greedy(last_logits, prompt, out, tag):
    """Teacher-forced oracle check; returns the number of near-tie (soft) tokens."""
    assert len(out) == GEN, (tag, len(out))
    toks, soft = list(prompt), 0
    for t in out:
        lg = last_logits(toks)
        best = int(lg.argmax())
        gap = float(lg[best] - lg[t])
        assert t == best or gap < TOL * float(lg.std()), (tag, len(toks), best, t, gap)
        soft += t != best
        toks.append(t)
    print(f"{tag}: {soft}/{GEN} near-tie tokens accepted")
    assert soft <= GEN // 4, (tag, soft)
    return soft


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("graphs", [False, True])
def test_forced_proposers(setup, graphs, k):
    """One sequence at a time, so the step counts are the sequence's own.  Always-right drafts:
    at most ceil((GEN - 1) / (k + 1)) decode steps, plus one per near-tie.  Always-wrong: exactly
    GEN - 1 steps, nothing accepted beyond near-ties.  Cycling: every accept length occurs."""
    model, prompts, last_logits = setup
    eng = _engine(model, graphs, k)
    assert (len(eng.graphs_spec) == len(eng.graphs) == 4) if graphs else not eng.graphs_spec
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    for kind in ("right", "wrong", "cycle"):
        eng.spec_proposer = _proposer(kind, k, last_logits)
        for p in prompts:
            before = dict(eng.stats)
            (out,) = eng.generate([p], sp)
            d = {key: eng.stats[key] - before.get(key, 0) for key in
                 ("decode_steps", "spec_steps", "spec_graph_steps", "spec_drafted", "spec_accepted", "graph_steps")}
            soft = _check_greedy(last_logits, p, out, f"graphs={graphs} k={k} {kind} prompt {len(p)}")
            assert d["spec_graph_steps"] == (d["spec_steps"] if graphs else 0)
            assert d["graph_steps"] == (d["decode_steps"] if graphs else 0)
            # the first token comes with the prompt; every decode step emits one token + its accepted drafts
            assert d["decode_steps"] + d["spec_accepted"] == GEN - 1, d
            if kind == "right":
                assert d["decode_steps"] <= math.ceil((GEN - 1) / (k + 1)) + soft, (d, soft)
            elif kind == "wrong":
                # GEN - 1 steps exactly, unless a near-tie made the sampler draw the "wrong" token
                assert d["spec_accepted"] <= soft and d["spec_steps"] > 0 and d["spec_drafted"] > 0, (d, soft)
            else:
                assert 0 < d["spec_accepted"] < d["spec_drafted"] or k == 1
                assert d["decode_steps"] < GEN - 1
    assert eng.alloc.num_free == eng.alloc.available - 1, "every KV page returns"


@pytest.mark.parametrize("k", [1, 4, 7])
@pytest.mark.parametrize("graphs", [False, True])
def test_batch_with_the_device_proposer(setup, graphs, k):
    """The n-gram proposer on the device (spec_accept + spec_propose behind every step), four
    greedy rows and a seeded sampling row, two of them admitted by mixed steps in the middle."""
    model, prompts, last_logits = setup
    eng = _engine(model, graphs, k)
    greedy = SamplingParams(max_tokens=GEN, ignore_eos=True)
    seeded = SamplingParams(max_tokens=GEN, ignore_eos=True, temperature=0.8, top_k=3, seed=11)
    seqs = [eng.add_request(prompts[1], greedy), eng.add_request(prompts[0], greedy)]
    for _ in range(4):
        eng.step()
    seqs.append(eng.add_request(prompts[2], greedy))
    eng.step()
    seqs.append(eng.add_request(prompts[3], seeded))
    seqs.append(eng.add_request(prompts[3], greedy))
    while eng.has_work():
        eng.step()
    st = eng.stats
    assert st["mixed_steps"] >= 2 and st["spec_steps"] > 0 and st["spec_drafted"] > 0
    assert st["spec_graph_steps"] == (st["spec_steps"] if graphs else 0)
    for s in seqs:
        if s.params is greedy:
            _check_greedy(last_logits, s.prompt, s.output, f"graphs={graphs} k={k} ngram prompt {len(s.prompt)}")
    # the seeded row: the reference draw on the oracle's logits, teacher-forced; a token may differ
    # where bf16 logits move a candidate across the top-k edge or the draw across a CDF step
    s = seqs[3]
    assert len(s.output) == GEN
    toks, off = list(s.prompt), 0
    one = lambda x, dt: torch.tensor([x], dtype=dt)  # noqa: E731
    for i, t in enumerate(s.output):
        lg = last_logits(toks)
        want = int(sample_reference(lg[None], one(0.8, torch.float32), one(3, torch.int32), one(1.0, torch.float32),
                                    one(seeded_uniform(11, i), torch.float32))[0])
        kth = float(lg.topk(3).values[-1])
        assert float(lg[t]) >= kth - TOL * float(lg.std()), (i, t, "outside the oracle's top-k")
        off += t != want
        toks.append(t)
    print(f"graphs={graphs} k={k} seeded row: {off}/{GEN} draws differ from the oracle's")
    assert off <= GEN // 4
    assert eng.alloc.num_free == eng.alloc.available - 1, "every KV page returns"


def _layout_total(max_tokens, max_seqs, mb):
    """MetaBuffers' buffer size as laid out before speculation existed."""
    up = lambda n: (n + 63) // 64 * 64  # noqa: E731
    return (16 + 6 * up(max_tokens) + 3 * up(max_seqs) + up(2 * max_tokens) + up(2 * max_seqs) + up(max_seqs * mb))


@pytest.mark.parametrize("graphs", [False, True])
def test_spec_off_is_the_engine_without_the_feature(setup, graphs):
    model, prompts, last_logits = setup
    off = _engine(model, graphs, 0)
    assert off.spec_k == 0 and not hasattr(off, "hist") and not off.graphs_spec and off._async
    assert off.meta.total == _layout_total(64, 8 + 8, 32) == MetaBuffers(64, 16, 32, off.G, model.n_kv, 512, "cpu").total
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    outs = off.generate(prompts, sp)
    assert not any(key.startswith("spec_") for key in off.stats)
    for p, o in zip(prompts, outs):
        _check_greedy(last_logits, p, o, f"graphs={graphs} spec off prompt {len(p)}")
    assert _engine(model, graphs, 0).generate(prompts, sp) == outs
    if graphs:
        assert off.stats["graph_steps"] > 0
    on = _engine(model, graphs, 4)
    assert on.meta.total >= off.meta.total and on.stats["spec_async_off"] == 1
