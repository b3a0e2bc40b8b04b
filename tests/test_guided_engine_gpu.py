"""Guided decoding through the engine on the GPU (tiny Llama, byte tokenizer, bounded grammars:
every request must finish "stop" with a full match): eager / decode graphs, sync / async,
against the CPU engine, beside penalised and log-probability rows, under speculation, and no
state left behind on a row."""
import itertools
import re

import numpy as np
import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.backends import ByteTokenizer
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

pytestmark = pytest.mark.gpu

TOK = ByteTokenizer()
EOS = TINY_LLAMA.eos_token_id
OBJ = {"type": "object", "properties": {"ok": {"type": "boolean"}, "n": {"enum": [1, 22]}}}
# (spec, full-match regex of the decoded output, longest member in bytes)
GRAMMARS = [({"choice": ["yes", "no", "maybe"]}, r"yes|no|maybe", 5),
            ({"regex": r"[0-9]{3}-[a-f]{2}"}, r"[0-9]{3}-[a-f]{2}", 6),
            ({"json_schema": OBJ}, r'\{"ok": ?(true|false), ?"n": ?(1|22)\}', 22)]
SAMPLING = [dict(), dict(temperature=1.5, seed=11), dict(temperature=1.5, seed=5, top_k=2)]
_MODEL = {}


def model_on(dev):
    if "gpu" not in _MODEL:
        torch.manual_seed(0)
        _MODEL["gpu"] = build_model(TINY_LLAMA, device=dev, seed=3)
    return _MODEL["gpu"]


def engine(model, graphs=False, asy=False, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=128, num_kv_blocks=64, use_graphs=graphs,
               graph_buckets=(1, 2, 4, 8), async_scheduling=asy, grammar_states=128)
    cfg.update(kw)
    eng = Engine(model, EngineConfig(**cfg))
    if cfg["grammar_states"]:
        eng.set_tokenizer(TOK)
    return eng


def run(eng, reqs):
    seqs = [eng.add_request(p, sp) for p, sp in reqs]
    for _ in range(2000):
        if not eng.has_work():
            break
        eng.step()
    assert not eng.has_work()
    return [(list(s.output), s.finish_reason) for s in seqs]


def guided_requests(sampling=SAMPLING):
    reqs, want = [], []
    for i, ((spec, rx, longest), samp) in enumerate(itertools.product(GRAMMARS, sampling)):
        reqs.append(([5 + i, 9, 40 + i], SamplingParams(max_tokens=longest + 2, guided=spec, **samp)))
        want.append(rx)
    return reqs, want


def assert_full_matches(outs, want):
    for (toks, reason), rx in zip(outs, want):
        assert reason == "stop", (reason, TOK.decode(toks))  # a "length" finish is a failure
        assert toks[-1] == EOS and all(3 <= t < 259 for t in toks[:-1])
        assert re.fullmatch(rx, TOK.decode(toks[:-1])), (rx, TOK.decode(toks[:-1]))


def test_eager_graphs_sync_async_identical(gpu):
    model = model_on(gpu)
    reqs, want = guided_requests()
    runs = {}
    for graphs, asy in itertools.product((False, True), (False, True)):
        eng = engine(model, graphs, asy)
        runs[graphs, asy] = run(eng, reqs)
        assert eng.stats["guided_rows"] > 0 and eng.stats["grammar_uploads"] == len(GRAMMARS)
        if graphs:
            assert eng.stats["graph_steps"] > 0
        assert (eng.r_gbase == -1).all() and all(g.refs == 0 for g in eng._g_resident)
    assert_full_matches(runs[False, False], want)
    assert runs[False, False] == runs[False, True]   # sync == async
    assert runs[True, False] == runs[True, True]
    assert runs[False, False] == runs[True, False]   # eager == decode graphs


def test_greedy_tokens_equal_the_cpu_engine(gpu):
    """Greedy guided requests on the GPU engine (bf16 kernels) and on a CPU engine holding the
    same weights in fp32: the same tokens for as long as the allowed logits are not tied, i.e.
    the best two allowed entries of the dense fp32 row differ by at least 0.05 std of the row
    (the project's bound for an engine token against the dense oracle, test_model_gpu); from
    the first tie on, a request's tokens are only required to be full matches."""
    model = model_on(gpu)
    cpu_model = build_model(TINY_LLAMA, device="cpu", dtype=torch.float32, seed=3).load_shard_from(model)
    reqs, want = guided_requests([dict()])
    reqs += [([7 + i, 30, 31, 32 + i], SamplingParams(max_tokens=8, guided=GRAMMARS[1][0])) for i in range(3)]
    want += [GRAMMARS[1][1]] * 3
    gpu_out = run(engine(model, graphs=True, asy=True), reqs)
    cpu_eng = engine(cpu_model)
    cpu_out = run(cpu_eng, reqs)
    assert_full_matches(gpu_out, want)
    assert_full_matches(cpu_out, want)
    compared = 0
    for (prompt, sp), (g, _), (c, _) in zip(reqs, gpu_out, cpu_out):
        gram, state = cpu_eng.compile_guided(sp), 0
        for k, t in enumerate(c):
            row = dense_logits(cpu_model, prompt + c[:k])[-1]
            allowed = torch.from_numpy(gram.next[state] >= 0)
            top = torch.topk(row.masked_fill(~allowed, float("-inf")), 2).values
            if int(allowed.sum()) > 1 and float(top[0] - top[1]) < 0.05 * float(row.std()):
                break  # tied: the engines may part here
            assert g[k] == t, (prompt, k, g, c)
            compared += 1
            state = gram.walk([t], state)
    assert compared >= 20  # the comparison is not vacuous


def test_guided_penalised_and_logprob_rows_share_a_batch(gpu):
    model = model_on(gpu)
    greqs, want = guided_requests()
    others = [([11, 12, 13], SamplingParams(max_tokens=20, ignore_eos=True, repetition_penalty=1e6)),
              ([14, 15, 16], SamplingParams(max_tokens=20, ignore_eos=True, logprobs=3)),
              ([17, 18, 19], SamplingParams(max_tokens=20, ignore_eos=True, temperature=0.9, seed=2))]
    # one guided request that is also penalised and wants log-probabilities
    both = ([20, 21, 22], SamplingParams(max_tokens=24, guided=GRAMMARS[2][0], frequency_penalty=0.5, logprobs=2))
    reqs = [greqs[0], others[0], greqs[4], others[1], greqs[8], others[2], both]
    runs = []
    for graphs, asy in ((False, False), (True, True)):
        eng = engine(model, graphs, asy)
        seqs = [eng.add_request(p, sp) for p, sp in reqs]
        while eng.has_work():
            eng.step()
        assert eng.stats["guided_rows"] > 0 and eng.stats["sampler_ext_rows"] > 0
        runs.append([(list(s.output), s.finish_reason, s.logprobs) for s in seqs])
    assert runs[0] == runs[1]
    outs = [(o, r) for o, r, _ in runs[0]]
    assert_full_matches([outs[0], outs[2], outs[4], outs[6]], [want[0], want[4], want[8], GRAMMARS[2][1]])
    pen, lp = runs[0][1], runs[0][3]
    assert len(pen[0]) == 20 and len(set(pen[0])) == 20 and not set(pen[0]) & {11, 12, 13}
    assert len(lp[0]) == 20 and len(lp[2]) == 20 and all(len(top) == 3 for _, top in lp[2])
    # log-probabilities are those of the logits as the model emitted them: unmasked, so the best
    # alternative of a guided row may be a token its grammar does not allow
    glp = runs[0][6][2]
    assert len(glp) == len(runs[0][6][0]) and all(v <= 0 and len(top) == 2 for v, top in glp)


def test_speculation_carries_guided_rows_undrafted(gpu):
    model = model_on(gpu)
    greqs, want = guided_requests()
    plain = (list(range(30, 38)) * 6, SamplingParams(max_tokens=24, ignore_eos=True))  # a prompt that repeats: drafts
    base_g = run(engine(model, graphs=True, asy=False), greqs)
    base = run(engine(model, graphs=True, asy=False), greqs + [plain])
    eng = engine(model, graphs=True, spec_tokens=4)
    assert run(eng, greqs) == base_g
    assert eng.stats["spec_drafted"] == 0 and eng.stats["guided_rows"] > 0   # guided rows never draft
    eng = engine(model, graphs=True, spec_tokens=4)
    outs = run(eng, greqs + [plain])
    assert eng.stats["spec_drafted"] > 0  # the unguided row beside them does
    assert outs == base
    assert_full_matches(outs[:-1], want)


@pytest.mark.parametrize("asy", [False, True], ids=["sync", "async"])
def test_no_state_leaks_into_the_rows_next_request(gpu, asy):
    model = model_on(gpu)
    plain = ([5, 6, 7, 8], SamplingParams(max_tokens=12, ignore_eos=True, temperature=0.8, seed=9))
    guided = ([5, 6, 7], SamplingParams(max_tokens=24, guided=GRAMMARS[2][0]))
    fresh = run(engine(model, True, asy, max_num_seqs=1), [plain])
    fresh_g = run(engine(model, True, asy, max_num_seqs=1), [guided])
    eng = engine(model, True, asy, max_num_seqs=1)  # one row: every request takes row 0 in turn
    outs = run(eng, [guided, plain, guided, plain])
    assert outs[1] == fresh[0] and outs[3] == fresh[0]
    assert outs[0] == fresh_g[0] and outs[2] == fresh_g[0]
    assert_full_matches([outs[0]], [GRAMMARS[2][1]])
    assert np.all(eng.r_gbase == -1)
