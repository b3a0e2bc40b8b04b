"""Embedding requests without a GPU: the pooling contract against float64 numpy, the CPU engine (torch
fallbacks) against transformers' own ``last_hidden_state`` on base-model checkpoints, the loader, the
scheduler's slot / preemption / abort paths, the V2 server and the control plane."""
import asyncio
import json
import subprocess
import sys

import numpy as np
import pytest
import torch

from mlopamd.models import build_model, loader
from mlopamd.models.config import TINY_LLAMA
from mlopamd.models.reference import dense_hidden
from mlopamd.ops.reference import (POOL_FIN_MEAN, POOL_FIN_NORMALIZE, POOL_INIT, POOL_LAST, POOL_MODE_LAST,
                                   pool_reference)
from mlopamd.runtime.engine import Engine, EngineConfig, Status
from mlopamd.runtime.sampler import SamplingParams


# ------------------------------------------------------------ reference --
def test_pool_reference_against_numpy():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(40, 64, generator=g).to(torch.bfloat16)
    acc0 = torch.randn(4, 64, generator=g)
    seg = [(3, 20, 1, POOL_INIT), (20, 33, 1, POOL_LAST), (33, 40, 2, 0), (0, 3, 3, POOL_MODE_LAST),
           (3, 9, 0, POOL_MODE_LAST | POOL_LAST | POOL_INIT)]
    fin = [(1, 30, 64, POOL_FIN_MEAN | POOL_FIN_NORMALIZE), (2, 7, 16, POOL_FIN_MEAN), (0, 6, 24, POOL_FIN_NORMALIZE)]
    acc, out = pool_reference(x, seg, acc0, fin)
    xn = x.float().numpy()
    a = np.zeros(64, np.float32)
    for r in range(3, 33):  # one fp32 add per row, in order: the chunk boundary at 20 changes nothing
        a = a + xn[r]
    assert np.array_equal(acc[1].numpy(), a)
    b = acc0[2].numpy().copy()
    for r in range(33, 40):  # no init: the stored value is the first term
        b = b + xn[r]
    assert np.array_equal(acc[2].numpy(), b)
    assert np.array_equal(acc[0].numpy(), xn[8]) and torch.equal(acc[3], acc0[3])  # last row / not the last chunk
    v = a.astype(np.float64) / 30
    np.testing.assert_allclose(out[1].numpy(), v / np.linalg.norm(v), rtol=1e-14)
    np.testing.assert_allclose(out[2, :16].numpy(), b[:16].astype(np.float64) / 7, rtol=1e-14)
    w = xn[8, :24].astype(np.float64)
    np.testing.assert_allclose(out[0, :24].numpy(), w / np.linalg.norm(w), rtol=1e-14)
    assert (out[2, 16:] == 0).all() and (out[0, 24:] == 0).all() and (out[3] == 0).all()
    # a zero vector stays zero under the norm
    _, z = pool_reference(x, [], torch.zeros(1, 64), [(0, 5, 64, POOL_FIN_MEAN | POOL_FIN_NORMALIZE)])
    assert (z == 0).all()


# ------------------------------------------------- engine vs transformers --
def _base_checkpoint(path, family):
    import transformers

    kw = dict(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2,
              num_key_value_heads=1, head_dim=128, max_position_embeddings=512)
    torch.manual_seed(0)
    if family == "qwen3":
        m = transformers.Qwen3Model(transformers.Qwen3Config(**kw, rms_norm_eps=1e-6)).eval()
    else:
        m = transformers.LlamaModel(transformers.LlamaConfig(
            **kw, rms_norm_eps=1e-5, rope_parameters={"rope_theta": 500000.0, "rope_type": "default"})).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(1 + 0.2 * torch.randn_like(p))
    m.save_pretrained(path)
    return m


needs_transformers = pytest.mark.skipif(__import__("importlib").util.find_spec("transformers") is None,
                                        reason="transformers is not installed")


def _hf_pooled(hf, toks, mode, normalize=True):
    with torch.no_grad():
        h = hf(torch.tensor([toks])).last_hidden_state[0].float()
    v = h[-1] if mode == "last" else h.mean(0)
    return v / v.norm() if normalize else v


@needs_transformers
@pytest.mark.parametrize("family", ["llama", "qwen3"])
def test_base_checkpoint_embeds_like_transformers(tmp_path, family):
    hf = _base_checkpoint(tmp_path, family)
    hfc = json.loads((tmp_path / "config.json").read_text())
    assert hfc["architectures"] == ["Qwen3Model" if family == "qwen3" else "LlamaModel"]
    from safetensors import safe_open

    with safe_open(str(next(tmp_path.glob("*.safetensors"))), framework="pt") as f:
        names = set(f.keys())
    assert "embed_tokens.weight" in names and "lm_head.weight" not in names  # no "model." prefix, no head
    (tmp_path / "1_Pooling").mkdir()
    (tmp_path / "1_Pooling" / "config.json").write_text(json.dumps({
        "word_embedding_dimension": 256, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
        "pooling_mode_lasttoken": False, "include_prompt": True}))
    (tmp_path / "modules.json").write_text(json.dumps([
        {"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
        {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"}]))
    ours = loader.load_pretrained(tmp_path, device="cpu", dtype=torch.float32)
    cfg = ours.cfg
    assert cfg.embedding_only and cfg.qk_norm == (family == "qwen3")
    assert (cfg.embed_pooling, cfg.embed_normalize) == ("mean", False)  # no Normalize module listed
    toks = [torch.randint(3, 500, (n,), generator=torch.Generator().manual_seed(5)).tolist() for n in (37, 9)]
    with torch.no_grad():
        ref = hf(torch.tensor([toks[0]])).last_hidden_state[0].float()
    torch.testing.assert_close(dense_hidden(ours, toks[0]), ref, atol=2e-4, rtol=1e-3)
    eng = Engine(ours, EngineConfig(max_num_seqs=4, max_num_batched_tokens=16, max_model_len=256, num_kv_blocks=64,
                                    use_graphs=False, embed_slots=2))
    for mode in ("last", "mean"):
        for t, v in zip(toks, eng.embed(toks, mode)):
            torch.testing.assert_close(torch.from_numpy(v), _hf_pooled(hf, t, mode), atol=2e-4, rtol=1e-3)
        for t, v in zip(toks, eng.embed(toks, mode, normalize=False, dim=32)):
            torch.testing.assert_close(torch.from_numpy(v), _hf_pooled(hf, t, mode, False)[:32], atol=2e-4, rtol=1e-3)
    with pytest.raises(ValueError, match="embeddings only"):
        eng.add_request(toks[0], SamplingParams(max_tokens=4))
    assert not eng.has_work()


def test_sentence_transformers_defaults(tmp_path):
    assert loader.embedding_defaults(tmp_path) == ("last", True)
    (tmp_path / "1_Pooling").mkdir()
    pool = tmp_path / "1_Pooling" / "config.json"
    mods = [{"type": "sentence_transformers.models.Transformer"}, {"type": "sentence_transformers.models.Pooling"},
            {"type": "sentence_transformers.models.Normalize"}]
    (tmp_path / "modules.json").write_text(json.dumps(mods))
    pool.write_text(json.dumps({"pooling_mode_lasttoken": True, "pooling_mode_mean_tokens": False}))
    assert loader.embedding_defaults(tmp_path) == ("last", True)
    pool.write_text(json.dumps({"pooling_mode_cls_token": True, "pooling_mode_mean_tokens": False}))
    assert loader.embedding_defaults(tmp_path) == (None, True)  # CLS pooling: a request must name its own


# ------------------------------------------------------------ scheduler --
@pytest.fixture(scope="module")
def model():
    return build_model(TINY_LLAMA, device="cpu", seed=3)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (150, 130, 40)]


def _engine(model, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=32, max_model_len=512, num_kv_blocks=128, use_graphs=False,
               embed_slots=2, mixed_min_chunk=8)
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


def _want(model, p, mode):
    h = dense_hidden(model, p)
    v = h[-1] if mode == "last" else h.mean(0)
    return (v / v.norm()).numpy()


def _close(v, w):
    return 1 - float(np.dot(v, w)) < 1e-4  # bf16 weights and activations against the fp32 oracle


def _run(eng, limit=2000):
    for _ in range(limit):
        if not eng.has_work():
            return
        eng.step()
    raise AssertionError("the engine did not drain")


@pytest.mark.parametrize("asy", [False, True], ids=["sync", "one-step-ahead"])
def test_preempted_embedding_restarts_with_init(model, prompts, asy):
    """13 usable pages: two decoding rows (40-token prompts growing to 100 tokens, 7 pages each) run out
    of pages while the 130-token embedding (9 pages) is in the middle of its chunked prompt: it is
    preempted, restarts from token 0 (its first chunk overwrites the slot) and gives the right mean."""
    eng = _engine(model, num_kv_blocks=14, enable_prefix_caching=False, async_scheduling=asy)
    sp = SamplingParams(max_tokens=60, ignore_eos=True)
    gen = [eng.add_request(prompts[2], sp), eng.add_request(prompts[2][::-1], sp)]
    eng.step()
    emb = eng.add_request(prompts[1], SamplingParams(embed="mean"))
    _run(eng)
    assert eng.stats["preemptions"] >= 1 and eng.stats["embed_tokens"] > len(prompts[1])  # it did restart
    assert emb.finish_reason == "embedding" and _close(emb.embedding, _want(model, prompts[1], "mean"))
    assert [len(s.output) for s in gen] == [60, 60]
    assert eng.alloc.num_free == eng.alloc.available - 1 and sorted(eng._free_embed) == [0, 1]


def test_abort_frees_the_slot_and_exhausted_slots_wait(model, prompts):
    eng = _engine(model, embed_slots=1)
    a = eng.add_request(prompts[0], SamplingParams(embed="last"))
    b = eng.add_request(prompts[2], SamplingParams(embed="mean"))
    gen = eng.add_request(prompts[2][::-1], SamplingParams(max_tokens=3, ignore_eos=True))
    eng.step()
    assert a.status == Status.PREFILL and a.emb_slot == 0 and b.status == Status.WAITING and not eng._free_embed
    while a.status == Status.PREFILL:
        eng.step()
    # a's last chunk left token budget: b still waited for a's slot, gen behind it needs none and went ahead
    assert a.finish_reason == "embedding" and b.status == Status.WAITING and gen.status != Status.WAITING
    c = eng.add_request(prompts[1], SamplingParams(embed="mean"))
    for _ in range(50):
        if c.status == Status.PREFILL:
            break
        eng.step()
    assert c.status == Status.PREFILL and b.finish_reason == "embedding" and not eng._free_embed
    eng.abort(c.seq_id)
    assert eng._free_embed == [0] and c.finish_reason == "abort" and c.embedding is None
    _run(eng)
    assert _close(a.embedding, _want(model, prompts[0], "last")) and _close(b.embedding, _want(model, prompts[2], "mean"))
    assert len(gen.output) == 3 and eng._free_embed == [0]
    assert eng.alloc.num_free == eng.alloc.available - 1
    assert eng.stats["embed_requests"] == 2


def test_rejections(model, prompts):
    p = prompts[2]
    with pytest.raises(ValueError, match="embed_slots = 0"):
        _engine(model, embed_slots=0).add_request(p, SamplingParams(embed="last"))
    with pytest.raises(ValueError, match="speculative"):
        _engine(model, spec_tokens=2)
    with pytest.raises(ValueError, match="LoRA"):
        _engine(model, max_adapters=1)
    eng = _engine(model)
    for bad, msg in ((dict(embed="cls"), "unknown pooling"), (dict(embed="last", adapter="a"), "adapter"),
                     (dict(embed="last", logprobs=2), "logprobs"), (dict(embed="mean", presence_penalty=0.5), "penalty"),
                     (dict(embed="last", guided={"choice": ["a"]}), "guided"), (dict(embed="last", embed_dim=0), "embed_dim"),
                     (dict(embed="last", embed_dim=257), "embed_dim"), (dict(embed_dim=8), "need embed")):
        with pytest.raises(ValueError, match=msg):
            eng.add_request(p, SamplingParams(**bad))
    assert not eng.has_work() and len(eng._free_embed) == 2
    assert eng.embed([p], "last", dim=256)[0].shape == (256,)


# --------------------------------------------------------------- server --
def test_server_embed_infer_and_metrics(model, prompts):
    from aiohttp.test_utils import TestClient, TestServer

    from mlopamd.runtime.backends import ByteTokenizer, LLMBackend
    from mlopamd.runtime.metrics import RuntimeMetrics
    from mlopamd.runtime.server import make_app

    eng = _engine(model, max_model_len=64, num_kv_blocks=64)
    b = LLMBackend(eng, RuntimeMetrics("llm", "v1", "ns", "tiny"), name="tiny").start()
    off = LLMBackend(_engine(model, embed_slots=0, max_model_len=64, num_kv_blocks=64), None, name="off").start()
    tok = ByteTokenizer()

    async def go():
        async with TestClient(TestServer(make_app(b, b.metrics))) as c, \
                TestClient(TestServer(make_app(off, None))) as c0:
            md = await (await c.get("/v2/models/tiny")).json()
            assert md["embeddings"]["slots"] == 2 and any(o["name"] == "embedding" for o in md["outputs"])
            assert "embeddings" not in await (await c0.get("/v2/models/off")).json()
            r = await c.post("/v2/models/tiny/embed", json={"text_input": "hello"})
            one = await r.json()
            assert r.status == 200 and one["dimensions"] == 256 and len(one["embeddings"]) == 1
            assert one["usage"]["prompt_tokens"] == len(tok.encode("hello"))
            assert _close(np.asarray(one["embeddings"][0]), _want(model, tok.encode("hello"), "last"))
            r = await c.post("/v2/models/tiny/embed", json={"text_input": ["hello", "a longer text"], "parameters": {
                "pooling": "mean", "normalize": False, "dimensions": 8}})
            two = await r.json()
            assert r.status == 200 and two["dimensions"] == 8 and [len(e) for e in two["embeddings"]] == [8, 8]
            ids = [tok.encode("hello"), [5, 6, 7, 8]]
            r = await c.post("/v2/models/tiny/embed", json={"input_ids": ids, "parameters": {"pooling": "last"}})
            three = await r.json()
            assert r.status == 200 and np.allclose(three["embeddings"][0], one["embeddings"][0])
            r = await c.post("/v2/models/tiny/embed", json={"input_ids": ids[1]})
            assert r.status == 200 and np.allclose((await r.json())["embeddings"][0], three["embeddings"][1])
            r = await c.post("/v2/models/tiny/infer", json={"inputs": [
                {"name": "text_input", "shape": [2], "datatype": "BYTES", "data": ["hello", "a longer text"]}],
                "parameters": {"pooling": "last", "dimensions": 16}})
            out = (await r.json())["outputs"]
            assert r.status == 200 and [(o["name"], o["datatype"], o["shape"]) for o in out] == [("embedding", "FP32", [2, 16])]
            assert len(out[0]["data"]) == 32
            r = await c.post("/v2/models/tiny/infer", json={"inputs": [
                {"name": "input_ids", "shape": [4], "datatype": "INT64", "data": ids[1]}], "parameters": {"pooling": "mean"}})
            assert r.status == 200 and (await r.json())["outputs"][0]["shape"] == [1, 256]
            r = await c.post("/v2/models/tiny/generate", json={"text_input": "x", "parameters": {"dimensions": 4}})
            assert r.status == 400  # not an embedding request
            # an embedding request on a generation endpoint is refused, not answered with a 500 or never
            for path in ("generate", "generate_stream"):
                for par in ({"pooling": "last"}, {"pooling": "mean", "max_tokens": 2}):
                    r = await asyncio.wait_for(c.post(f"/v2/models/tiny/{path}", json={"text_input": "x", "parameters": par}), 10)
                    assert r.status == 400 and "embed" in await r.text(), (path, par, r.status)
            # an input may fill the context exactly (no token is generated); one more token is a 400
            r = await c.post("/v2/models/tiny/embed", json={"input_ids": [7] * 64})
            assert r.status == 200 and (await r.json())["usage"]["prompt_tokens"] == 64
            r = await c.post("/v2/models/tiny/generate", json={"input_ids": [7] * 64, "parameters": {"max_tokens": 1}})
            assert r.status == 400
            bad = [{"text_input": "x", "parameters": {"pooling": "cls"}},
                   {"text_input": "x", "parameters": {"pooling": "last", "dimensions": 300}},
                   {"text_input": "x", "parameters": {"pooling": "last", "logprobs": 2}},
                   {"text_input": "x", "parameters": {"pooling": "last", "normalize": "yes"}},
                   {"text_input": "x", "parameters": {"pooling": "last", "encoding_format": "base64"}},
                   {"text_input": []}, {"input_ids": [[5, 6], list(range(2, 80))]}, {"input_ids": [7] * 65}]
            for body in bad:  # over-long inputs are refused, never truncated; none of the batch runs
                r = await c.post("/v2/models/tiny/embed", json=body)
                assert r.status == 400, (body, r.status, await r.text())
            r = await c0.post("/v2/models/off/embed", json={"text_input": "hello"})
            assert r.status == 400 and "embed" in await r.text()
            r = await c0.post("/v2/models/off/generate", json={"input_ids": [5, 6], "parameters": {"max_tokens": 2,
                                                                                                   "ignore_eos": True}})
            assert r.status == 200
            r = await c.post("/v2/models/tiny/generate", json={"input_ids": [5, 6, 7], "parameters": {
                "max_tokens": 3, "ignore_eos": True}})
            assert r.status == 200 and len((await r.json())["output_ids"]) == 3  # still serving
            txt = await (await c.get("/metrics")).text()
            line = lambda name: next(float(l.rsplit(" ", 1)[1]) for l in txt.splitlines() if l.startswith(name + "{"))  # noqa: E731
            nh, nl = len(tok.encode("hello")), len(tok.encode("a longer text"))
            assert line("mlop_embedding_requests_total") == 10
            assert line("mlop_embedding_tokens_total") == 4 * nh + 2 * nl + 3 * 4 + 64
            assert line("mlop_engine_tokens_total") == 3  # the generated tokens: a delivered vector is no token
            ok = [l for l in txt.splitlines() if l.startswith("seldon_api_executor_server_requests_seconds_count{")
                  and 'service="predictions"' in l and 'code="200"' in l]
            assert ok and float(ok[0].rsplit(" ", 1)[1]) == 7
            # a caller of submit() that streams an embedding request gets the closing None and the vector
            req = b.submit([5, 6, 7, 8], SamplingParams(embed="last"), stream=True)
            assert await asyncio.wait_for(req.queue.get(), 10) is None
            assert (await asyncio.wait_for(req.future, 10))["embedding"].shape == (256,)

    try:
        asyncio.run(go())
    finally:
        b.stop()
        off.stop()


def test_server_takes_the_checkpoints_defaults(prompts):
    """A checkpoint whose settings say mean pooling and list no Normalize module: a request gets both
    defaults, and the normalize default also when it names its pooling; embedding_only makes every
    infer an embedding request and refuses generation."""
    from dataclasses import replace

    from aiohttp.test_utils import TestClient, TestServer

    from mlopamd.runtime.backends import LLMBackend
    from mlopamd.runtime.server import make_app

    cfg = replace(TINY_LLAMA, embed_pooling="mean", embed_normalize=False, embedding_only=True)
    m = build_model(cfg, device="cpu", seed=3)
    b = LLMBackend(_engine(m, max_model_len=64, num_kv_blocks=64), None, name="st").start()
    assert b.embedding_only and b.serves_embeddings and b.embedding_defaults() == ("mean", False)
    ids = prompts[2][:20]
    h = dense_hidden(m, ids)

    async def go():
        async with TestClient(TestServer(make_app(b, None))) as c:
            async def vec(par):
                r = await c.post("/v2/models/st/embed", json={"input_ids": ids, **({"parameters": par} if par else {})})
                assert r.status == 200, await r.text()
                return np.asarray((await r.json())["embeddings"][0])

            mean, last = h.mean(0).numpy(), h[-1].numpy()
            for par, want in ((None, mean), ({"pooling": "mean"}, mean), ({"pooling": "last"}, last)):
                v = await vec(par)
                assert _close(v / np.linalg.norm(v), want / np.linalg.norm(want)), par
                assert abs(np.linalg.norm(v) / np.linalg.norm(want) - 1) < 2e-2 and abs(np.linalg.norm(want) - 1) > 0.5, par
            v = await vec({"pooling": "last", "normalize": True})
            assert abs(np.linalg.norm(v) - 1) < 1e-5
            r = await c.post("/v2/models/st/infer", json={"inputs": [
                {"name": "input_ids", "shape": [len(ids)], "datatype": "INT64", "data": ids}]})
            out = (await r.json())["outputs"]
            assert r.status == 200 and out[0]["name"] == "embedding" and out[0]["shape"] == [1, 256]
            r = await c.post("/v2/models/st/generate", json={"input_ids": ids, "parameters": {"max_tokens": 2}})
            assert r.status == 400 and "embeddings only" in await r.text()

    try:
        asyncio.run(go())
    finally:
        b.stop()


# -------------------------------------------------------- control plane --
def test_crd_field_operator_env_and_knobs(monkeypatch):
    import yaml

    from mlopamd.controller import seldon
    from mlopamd.controller.crd import ModelSpec
    from mlopamd.runtime.server import engine_kwargs_from_env

    base = {"modelName": "m", "modelAlias": "champion"}
    assert ModelSpec.from_spec(base).embedding_slots is None
    assert ModelSpec.from_spec({**base, "embeddingSlots": 64}).validate() == []
    assert ModelSpec.from_spec({**base, "embeddingSlots": 0, "tensorParallel": 8}).validate() == []
    for bad in (-1, 4097, "64", True, 1.5):
        assert any("embeddingSlots" in e for e in ModelSpec.from_spec({**base, "embeddingSlots": bad}).validate())
    for par in ({"tensorParallel": 2}, {"expertParallel": 4}):
        errs = ModelSpec.from_spec({**base, "embeddingSlots": 8, **par}).validate()
        assert any("embeddingSlots" in e and "tensorParallel = 1 and expertParallel = 1" in e for e in errs)
    errs = ModelSpec.from_spec({**base, "embeddingSlots": 8, "speculativeTokens": 3}).validate()
    assert any("embeddingSlots" in e and "speculativeTokens" in e for e in errs)
    with open("manifests/crd.yaml") as f:
        crd = yaml.safe_load(f)
    props = crd["spec"]["versions"][0]["schema"]["openAPIV3Schema"]["properties"]["spec"]["properties"]
    assert (props["embeddingSlots"]["type"], props["embeddingSlots"]["minimum"]) == ("integer", 0)
    with open("manifests/examples/embeddings/qwen3-8b-embeddings.yaml") as f:
        spec = ModelSpec.from_spec(yaml.safe_load(f)["spec"])
    assert spec.validate() == [] and spec.embedding_slots == 64
    pred = seldon.build_predictor("1", "s3://mlflow/x", None, 100, runtime=seldon.RUNTIME_LLM, replicas=1,
                                  placement=None, image="img", gpu_resource="amd.com/gpu", model_name="m",
                                  deployment="d", namespace="ns", architecture="qwen3-8b",
                                  engine_args={"embed_slots": spec.embedding_slots})
    env = {e["name"]: e["value"] for e in json.loads(json.dumps(pred))["componentSpecs"][0]["spec"]["containers"][0]["env"]}
    assert env["MLOP_ENGINE_EMBED_SLOTS"] == "64"
    monkeypatch.setenv("MLOP_ENGINE_EMBED_SLOTS", env["MLOP_ENGINE_EMBED_SLOTS"])
    kw = engine_kwargs_from_env()
    assert kw["embed_slots"] == 64 and EngineConfig(**kw).embed_slots == 64
    r = subprocess.run([sys.executable, "scripts/knobs.py", "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
