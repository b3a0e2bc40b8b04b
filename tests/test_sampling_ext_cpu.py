"""Sampler extensions on the CPU path (the plain-torch oracle of the HIP kernels): repetition /
presence / frequency penalties from the count table and per-token log-probabilities, through
the sampler, the sync and async engines, the HTTP server, EP request records and TP = 2."""
import asyncio
import json
import os
import socket
import tempfile

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_MIXTRAL, get_config
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import MAX_LOGPROBS, SamplingParams

CFGS = {"tiny-llama": TINY_LLAMA, "tiny-mixtral": TINY_MIXTRAL}
_MODELS = {}


def model_of(name, seed, dtype=torch.float32):
    if (name, seed, dtype) not in _MODELS:
        torch.manual_seed(0)
        _MODELS[name, seed, dtype] = build_model(CFGS[name], device="cpu", dtype=dtype, seed=seed)
    return _MODELS[name, seed, dtype]


def engine(model, asy, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=256, num_kv_blocks=64, use_graphs=False,
               async_scheduling=asy)
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


def penalised_row(l, prompt, out, r, f, p):
    """The issue's three formula lines on one fp32 logits row."""
    l = l.clone().float()
    for t in set(prompt) | set(out):
        c = out.count(t)
        if r != 1:
            l[t] = l[t] / r if l[t] > 0 else l[t] * r
        l[t] -= f * c
        l[t] -= p * (c > 0)
    return l


def oracle_greedy(model, prompt, n, r, f, p):
    """Greedy decode of the penalised dense logits; also the smallest top-2 gap / std seen."""
    out, min_gap = [], float("inf")
    for _ in range(n):
        row = penalised_row(dense_logits(model, list(prompt) + out)[-1], prompt, out, r, f, p)
        top = torch.topk(row, 2).values
        min_gap = min(min_gap, float((top[0] - top[1]) / row.std()))
        out.append(int(row.argmax()))
    return out, min_gap


def prompts_of(seed, lens):
    rng = np.random.default_rng(seed)
    return [rng.integers(2, 500, size=n).tolist() for n in lens]


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-mixtral"])
@pytest.mark.parametrize("asy", [False, True])
def test_greedy_with_penalties_matches_oracle(name, asy):
    model = model_of(name, 1)
    r, f, p = 1.3, 0.5, 0.4
    prompts = prompts_of(5, (7, 19, 33))
    want = []
    for pr in prompts:
        toks, gap = oracle_greedy(model, pr, 12, r, f, p)
        assert gap > 1e-4, gap  # precondition: no near-tie the engine's batching could flip
        want.append(toks)
    eng = engine(model, asy)
    sp = SamplingParams(max_tokens=12, ignore_eos=True, repetition_penalty=r, frequency_penalty=f,
                        presence_penalty=p)
    assert eng.generate(prompts, sp) == want
    assert eng.stats["sampler_ext_rows"] > 0 and len(eng.free_pen_slots) == eng.cfg.penalty_slots


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-mixtral"])
@pytest.mark.parametrize("seed", [1, 3])
def test_huge_repetition_penalty_never_repeats(name, seed):
    """Greedy with repetition_penalty = 1e6: 32 distinct tokens, none from the prompt (plain
    greedy decoding of these models repeats after a handful of tokens)."""
    model = model_of(name, seed)
    prompts = prompts_of(seed, (16, 40))
    for asy in (False, True):
        outs = engine(model, asy).generate(prompts, SamplingParams(max_tokens=32, ignore_eos=True,
                                                                   repetition_penalty=1e6))
        for pr, o in zip(prompts, outs):
            assert len(o) == 32 and len(set(o)) == 32 and not set(o) & set(pr)


def _population(model):
    """Mixed requests: plain greedy, plain seeded, penalised greedy / seeded, logprobs 0 / 3 / 20."""
    rng = np.random.default_rng(11)
    prompts = [rng.integers(2, 500, size=int(rng.integers(3, 50))).tolist() for _ in range(14)]
    probe = engine(model, False).generate(prompts, SamplingParams(max_tokens=3, ignore_eos=True))
    params = []
    for i in range(len(prompts)):
        kw = dict(max_tokens=int(4 + i % 9), ignore_eos=True)
        if i % 2:
            kw["stop_token_ids"] = [probe[i][2]]  # fires on the plain rows (their 3rd greedy token)
        if i % 3 == 1:  # 5 penalised requests (1, 4, 7, 10, 13) against 2 slots
            kw.update(repetition_penalty=1.2 if i % 2 else 0.8, frequency_penalty=0.3, presence_penalty=-0.2)
        if i in (4, 10, 5):
            kw.update(temperature=0.9, top_k=(0, 20)[i == 5], top_p=0.9, seed=100 + i)
        if i in (0, 4, 7, 8):
            kw["logprobs"] = {0: 3, 4: 20, 7: 0, 8: 20}[i]
        params.append(SamplingParams(**kw))
    return prompts, params


def _run_population(model, prompts, params, asy, only=None):
    eng = engine(model, asy, max_num_seqs=5, max_num_batched_tokens=40, num_kv_blocks=8, mixed_min_chunk=8,
                 prefill_min_batch=2, penalty_slots=2)
    seqs, i, it = [], 0, 0
    idx = [j for j in range(len(prompts)) if only is None or j in only]
    while i < len(idx) or eng.has_work():
        if i < len(idx) and it % 2 == 0:
            seqs.append(eng.add_request(prompts[idx[i]], params[idx[i]]))
            i += 1
        if it == 12 and only is None:
            eng.abort(seqs[-1].seq_id)
        eng.step()
        it += 1
        assert it < 2000
    assert eng.alloc.num_free == eng.alloc.available - 1 and len(eng.free_pen_slots) == 2
    return {j: (s.output, s.finish_reason, s.logprobs) for j, s in zip(idx, seqs)}, eng.stats


def test_async_matches_sync_with_slots_preemption_abort():
    """Async == sync EXACTLY: tokens, finish reasons and log-probabilities (ids and values).

    The model here is fp64.  The two schedules run different batch shapes (async decodes a
    finishing row once more; preemption falls on other steps), and a CPU GEMM's row depends on
    the batch size in its last bits: with the fp32 model the tokens, finish reasons and top ids
    are equal but 14 of the log-probability values differ by 1-2 ulp (4.8e-7 .. 9.5e-7), which
    says nothing about the sampler.  With fp64 weights the logits rounded to fp32 ("the logits
    as the model emitted them, converted to fp32") come out the same in both runs of this
    population, so everything after them must be bit-identical.  (The reference ops still
    round some intermediates to fp32: a different population can show a stray 1-ulp value.)"""
    model = model_of("tiny-llama", 1, torch.float64)
    prompts, params = _population(model)
    sync, st_s = _run_population(model, prompts, params, False)
    asy, st_a = _run_population(model, prompts, params, True)
    assert asy == sync  # tokens, finish reasons and log-probabilities, exactly
    assert st_a["preemptions"] > 0 and st_a["async_host_us"] > 0
    reasons = [r for _, r, _ in asy.values()]
    assert all(r is not None for r in reasons)  # every request finished
    assert "stop" in reasons and "abort" in reasons and "length" in reasons
    for j, (out, _, lps) in asy.items():
        n = params[j].logprobs
        assert len(lps) == (0 if n is None else len(out))
        assert all(len(top) == n for _, top in lps)
    # the plain rows are untouched by their penalised neighbours
    plain = {j for j in range(len(prompts)) if not params[j].extended}
    aborted = {j for j, (_, r, _) in asy.items() if r == "abort"}
    alone, st = _run_population(model, prompts, params, True, only=plain)
    assert st["sampler_ext_rows"] == 0
    for j in plain - aborted:
        assert alone[j][:2] == asy[j][:2], j


@pytest.mark.parametrize("name", ["tiny-llama", "tiny-mixtral"])
def test_logprobs_match_dense_log_softmax(name):
    """Log-probabilities are those of the UNPENALISED dense logits (fp64 log-softmax): the ids
    equal under the tie rule, values within 4x the largest |delta| measured here.

    Measured max |delta| against the dense fp64 oracle: 7.78e-7 (tiny-llama), 8.6e-7
    (tiny-mixtral): the fp32 forward in the engine's batching vs the dense forward, plus the
    fp32 log-softmax.  Bound: 4 x 8.6e-7 = 3.5e-6."""
    model = model_of(name, 1)
    prompts = prompts_of(9, (5, 21))
    sps = [SamplingParams(max_tokens=8, ignore_eos=True, logprobs=5, repetition_penalty=1.5),
           SamplingParams(max_tokens=8, ignore_eos=True, logprobs=MAX_LOGPROBS, temperature=0.8, top_k=30, seed=4)]
    eng = engine(model, True)
    seqs = [eng.add_request(p, sp) for p, sp in zip(prompts, sps)]
    while eng.has_work():
        eng.step()
    worst = 0.0
    for s in seqs:
        n = s.params.logprobs
        assert len(s.logprobs) == len(s.output) == 8
        for k, (lp, top) in enumerate(s.logprobs):
            row = dense_logits(model, s.prompt + s.output[:k])[-1].double()
            ref = torch.log_softmax(row, -1)
            order = torch.sort(-row, stable=True).indices[:n].tolist()
            assert [t for t, _ in top] == order
            vals = [v for _, v in top]
            assert lp <= 0 and all(v <= 0 for v in vals) and vals == sorted(vals, reverse=True)
            worst = max(worst, abs(lp - float(ref[s.output[k]])),
                        max(abs(v - float(ref[t])) for t, v in top))
    print(f"{name}: max |logprob - dense fp64| = {worst:.3g}")
    assert worst <= 3.5e-6, worst


@pytest.mark.parametrize("bad", [
    dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("inf")),
    dict(repetition_penalty=float("nan")), dict(presence_penalty=2.5), dict(presence_penalty=-2.01),
    dict(presence_penalty=float("nan")), dict(frequency_penalty=3.0), dict(frequency_penalty=float("-inf")),
    dict(logprobs=-1), dict(logprobs=MAX_LOGPROBS + 1), dict(logprobs=2.0), dict(logprobs=True)])
def test_validation_rejects(bad):
    with pytest.raises(ValueError):
        SamplingParams(**bad).validate()


def test_validation_accepts_and_defaults():
    sp = SamplingParams().validate()
    assert (sp.repetition_penalty, sp.presence_penalty, sp.frequency_penalty, sp.logprobs) == (1.0, 0.0, 0.0, None)
    assert not sp.extended and not sp.penalised
    for ok in (dict(repetition_penalty=1e6), dict(presence_penalty=-2.0, frequency_penalty=2.0),
               dict(logprobs=0), dict(logprobs=MAX_LOGPROBS)):
        assert SamplingParams(**ok).validate().extended
    assert MAX_LOGPROBS == 20


def test_ep_records_carry_penalties_and_rank0_rejects_logprobs():
    from mlopamd.runtime.ep_serving import _pack, _unpack, check_ep_request, packed_words

    reqs = [(7, 1, [5, 6, 7], SamplingParams(max_tokens=9, temperature=0.7, top_k=5, top_p=0.9, seed=3,
                                             stop_token_ids=[11, 12], repetition_penalty=1.3,
                                             presence_penalty=-0.4, frequency_penalty=0.5)),
            (8, 0, [9], SamplingParams())]
    buf = _pack(reqs)
    assert buf.numel() == sum(packed_words(p, sp) for _, _, p, sp in reqs)
    back = _unpack(buf, len(reqs))
    for (rid, r, prompt, sp), (rid2, r2, prompt2, sp2) in zip(reqs, back):
        assert (rid, r, prompt) == (rid2, r2, prompt2) and sp == sp2
    check_ep_request(reqs[0][3])
    with pytest.raises(ValueError, match="expert-parallel"):
        check_ep_request(SamplingParams(logprobs=0))


def test_caller_logits_are_never_modified():
    from mlopamd import ops
    from mlopamd.runtime.sampler import Sampler, SamplerExt

    torch.manual_seed(0)
    logits = torch.randn(3, 64)
    keep = logits.clone()
    table = ops.penalty_table(2, 64, "cpu")
    ops.penalty_reset(table, 1, [3, 3, 9], [int(keep[0].argmax()), 9, 9])
    assert int(table[1, 3]) == -(2**31) and int(table[1, 9]) == -(2**31) + 2 and table.shape[1] % 4 == 0
    ext = SamplerExt(table, [1, -1, -1], [2.0, 1, 1], [0.5, 0, 0], [0.1, 0, 0], [2, -1, 0])
    toks, lp, ids = Sampler("cpu")(logits, [SamplingParams()] * 3), None, None
    toks2, lp, ids = Sampler("cpu").sample_ext(logits, [SamplingParams()] * 3, ext)
    assert torch.equal(logits, keep)
    assert toks2[1:].tolist() == toks[1:].tolist() and int(toks2[0]) != int(toks[0])
    assert int(table[1, int(toks2[0])]) & 0x7FFFFFFF == 1  # the draw was counted
    ref = torch.log_softmax(keep, -1)
    assert ids[0].tolist() == [int(toks2[0])] + torch.topk(keep[0], 2).indices.tolist()
    assert torch.allclose(lp[0], ref[0][ids[0].long()]) and float(lp[2, 0]) == float(ref[2, int(toks2[2])])
    assert lp[1].tolist() == [0, 0, 0]  # a row that did not ask keeps what the buffer held


# ------------------------------------------------------------------ HTTP --
@pytest.fixture(scope="module")
def llm_backend():
    from mlopamd.runtime.backends import LLMBackend
    from mlopamd.runtime.metrics import RuntimeMetrics

    eng = engine(model_of("tiny-llama", 1), True, max_num_seqs=4)
    b = LLMBackend(eng, RuntimeMetrics("llm", "v1", "ns", "tiny"), name="tiny").start()
    yield b
    b.stop()


def test_http_penalties_and_logprobs(llm_backend):
    from aiohttp.test_utils import TestClient, TestServer

    from mlopamd.runtime.server import make_app

    ids = [5, 6, 7, 8]

    async def go():
        async with TestClient(TestServer(make_app(llm_backend, llm_backend.metrics))) as c:
            r = await c.post("/v2/models/tiny/generate", json={"input_ids": ids, "parameters": {
                "max_tokens": 6, "ignore_eos": True, "logprobs": 2, "repetition_penalty": 1.3}})
            body = await r.json()
            assert r.status == 200 and len(body["logprobs"]) == len(body["output_ids"]) == 6
            for e, t in zip(body["logprobs"], body["output_ids"]):
                assert e["token_id"] == t and e["logprob"] <= 0 and len(e["top"]) == 2
                assert all(isinstance(i, int) and v <= 0 for i, v in e["top"])
            r = await c.post("/v2/models/tiny/generate_stream", json={"input_ids": ids, "parameters": {
                "max_tokens": 6, "ignore_eos": True, "logprobs": 2, "repetition_penalty": 1.3}})
            ev = [json.loads(line[6:]) for line in (await r.text()).split("\n\n") if line.startswith("data: ")]
            assert [e["token_id"] for e in ev[:-1]] == body["output_ids"] and ev[-1]["done"]
            assert [(e["logprob"], e["top_logprobs"]) for e in ev[:-1]] == \
                [(e["logprob"], e["top"]) for e in body["logprobs"]]
            r = await c.post("/v2/models/tiny/infer", json={"inputs": [
                {"name": "input_ids", "shape": [len(ids)], "datatype": "INT64", "data": ids}],
                "parameters": {"max_tokens": 6, "ignore_eos": True, "logprobs": 2, "repetition_penalty": 1.3}})
            outs = {o["name"]: o for o in (await r.json())["outputs"]}
            assert outs["output_ids"]["data"] == body["output_ids"]
            assert outs["logprobs"]["shape"] == [6] and outs["logprobs"]["datatype"] == "FP32"
            assert outs["top_logprob_ids"]["shape"] == [6, 2] and outs["top_logprob_ids"]["datatype"] == "INT64"
            assert outs["top_logprobs"]["shape"] == [6, 2] and len(outs["top_logprobs"]["data"]) == 12
            r = await c.post("/v2/models/tiny/infer", json={"inputs": [
                {"name": "input_ids", "shape": [len(ids)], "datatype": "INT64", "data": ids}],
                "parameters": {"max_tokens": 3, "ignore_eos": True, "logprobs": 0}})
            assert [o["name"] for o in (await r.json())["outputs"]] == ["output_ids", "logprobs"]
            for bad in ({"presence_penalty": 2.5}, {"frequency_penalty": -3}, {"repetition_penalty": 0},
                        {"logprobs": 21}, {"logprobs": "3"}):
                for path in ("generate", "generate_stream"):
                    r = await c.post(f"/v2/models/tiny/{path}", json={"input_ids": ids, "parameters": bad})
                    assert r.status == 400, (bad, path, r.status)
            r = await c.post("/v2/models/tiny/generate", json={"input_ids": ids, "parameters": {
                "max_tokens": 4, "ignore_eos": True}})
            plain = await r.json()
            assert r.status == 200 and "logprobs" not in plain and len(plain["output_ids"]) == 4
            r = await c.post("/v2/models/tiny/generate_stream", json={"input_ids": ids, "parameters": {
                "max_tokens": 2, "ignore_eos": True}})
            ev = [json.loads(line[6:]) for line in (await r.text()).split("\n\n") if line.startswith("data: ")]
            assert all("logprob" not in e for e in ev)
    asyncio.run(go())


# ------------------------------------------------------------- TP = 2 (gloo) --
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _entry(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        torch.save(_tp_penalised(world), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


TP_PROMPTS = [[5, 9, 11, 40, 2, 7], list(range(20, 61)), [100, 3]]


def _tp_penalised(world):
    from mlopamd.parallel.comm import make_parallel_state

    cfg = get_config("tiny-llama")
    full = build_model(cfg, device="cpu", dtype=torch.float32, seed=4)
    ps = make_parallel_state(tp_size=world, ep_size=world)
    shard = build_model(cfg, device="cpu", dtype=torch.float32, pstate=ps, seed=4).load_shard_from(full)
    ec = EngineConfig(max_num_seqs=4, max_num_batched_tokens=32, max_model_len=128, num_kv_blocks=40, use_graphs=False)
    eng = Engine(shard, ec)
    sps = [SamplingParams(max_tokens=10, ignore_eos=True, repetition_penalty=1.3, frequency_penalty=0.5,
                          presence_penalty=0.4, logprobs=2),
           SamplingParams(max_tokens=10, ignore_eos=True),
           SamplingParams(max_tokens=10, ignore_eos=True, repetition_penalty=1e6)]
    if ps.tp_rank == 0:
        outs = eng.generate(TP_PROMPTS, sps)
        lps = [s.logprobs for s in eng.seqs.values()]
        eng.shutdown()
        ref_eng = Engine(full, ec)
        ref = ref_eng.generate(TP_PROMPTS, sps)
        return {"tp": outs, "ref": ref, "lps": lps, "ref_lps": [s.logprobs for s in ref_eng.seqs.values()]}
    eng.worker_loop()
    return {"worker_steps": eng.stats["worker_steps"]}


def test_tp2_penalised_greedy_matches_tp1():
    d = tempfile.mkdtemp()
    mp.start_processes(_entry, args=(2, _free_port(), d), nprocs=2, join=True, start_method="spawn")
    r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["tp"] == r0["ref"] and r1["worker_steps"] > 0
    assert len(set(r0["tp"][2])) == 10 and not set(r0["tp"][2]) & set(TP_PROMPTS[2])
    assert [len(l) for l in r0["lps"]] == [10, 0, 0]
    for (a, ta), (b, tb) in zip(r0["lps"][0], r0["ref_lps"][0]):
        assert [t for t, _ in ta] == [t for t, _ in tb] and abs(a - b) < 1e-4
