"""Multi-LoRA serving on CPU (reference ops, fp32): PEFT loader and its rejections, parity with
transformers on the merged model, prefix-cache isolation, scheduling, server and operator."""
import asyncio
import json
import math

import numpy as np
import pytest
import torch

from mlopamd.models import build_model, loader
from mlopamd.models.config import TINY_LLAMA, TINY_MIXTRAL
from mlopamd.models.lora import LoraStacks, merged_copy, module_shapes
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.attn_meta import MetaBuffers, plan_partitions
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.kv_cache import KVCache
from mlopamd.runtime.sampler import SamplingParams

_BLOCK = {"q_proj": "self_attn", "k_proj": "self_attn", "v_proj": "self_attn", "o_proj": "self_attn",
          "gate_proj": "mlp", "up_proj": "mlp", "down_proj": "mlp"}
ALL = tuple(_BLOCK)


def write_adapter(path, cfg, r=8, alpha=16.0, targets=ALL, seed=0, std=0.05, rslora=False, extra_cfg=None,
                  extra_tensors=None):
    """A PEFT-format adapter directory written by hand: adapter_config.json + adapter_model.safetensors."""
    from safetensors.torch import save_file

    path.mkdir(parents=True, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    shapes = module_shapes(cfg)
    tensors = {}
    for i in range(cfg.num_layers):
        for m in targets:
            n, k = shapes[m]
            base = f"base_model.model.model.layers.{i}.{_BLOCK[m]}.{m}"
            tensors[f"{base}.lora_A.weight"] = torch.randn(r, k, generator=g) * std
            tensors[f"{base}.lora_B.weight"] = torch.randn(n, r, generator=g) * std
    tensors.update(extra_tensors or {})
    save_file(tensors, str(path / "adapter_model.safetensors"))
    ac = {"peft_type": "LORA", "r": r, "lora_alpha": alpha, "target_modules": list(targets), "use_rslora": rslora,
          "bias": "none", "use_dora": False, "modules_to_save": None, "rank_pattern": {}, "alpha_pattern": {}}
    ac.update(extra_cfg or {})
    (path / "adapter_config.json").write_text(json.dumps(ac))
    return path


# ------------------------------------------------------------ transformers parity --

def _tiny_hf(tmp_path):
    transformers = pytest.importorskip("transformers")
    cfg = transformers.LlamaConfig(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                   num_attention_heads=2, num_key_value_heads=1, head_dim=128,
                                   max_position_embeddings=512, rms_norm_eps=1e-5, tie_word_embeddings=False,
                                   rope_parameters={"rope_theta": 500000.0, "rope_type": "default"})
    torch.manual_seed(0)
    m = transformers.LlamaForCausalLM(cfg).eval()
    with torch.no_grad():  # non-unit norm weights: the fold into the A matrices must happen
        for n, p in m.named_parameters():
            if n.endswith("layernorm.weight") or n == "model.norm.weight":
                p.copy_(1 + 0.2 * torch.randn_like(p))
    m.save_pretrained(tmp_path)
    return m


def _merge_into_hf(hf, adapter_dir):
    """W += scale * B @ A on a copy of the HF model, straight from the adapter files."""
    import copy

    from safetensors.torch import load_file

    ac = json.loads((adapter_dir / "adapter_config.json").read_text())
    scale = ac["lora_alpha"] / (math.sqrt(ac["r"]) if ac.get("use_rslora") else ac["r"])
    t = load_file(str(adapter_dir / "adapter_model.safetensors"))
    out = copy.deepcopy(hf)
    sd = dict(out.named_parameters())
    with torch.no_grad():
        for k in t:
            if k.endswith("lora_A.weight"):
                name = k[len("base_model.model."):-len(".lora_A.weight")] + ".weight"
                sd[name] += scale * t[k.replace("lora_A", "lora_B")] @ t[k]
    return out


def lora_logits(model, stacks, toks, slot):
    """[T, V] logits of one sequence through LlamaModel.forward(..., lora=) on fresh KV pages."""
    T = len(toks)
    mc = model.cfg
    nblk = (T + 15) // 16
    mb = MetaBuffers(T, 2, nblk, model.n_q // model.n_kv, model.n_kv, 512, model.device)
    kv = KVCache(mc.num_layers, nblk + 1, model.n_kv, mc.head_dim, model.device, model.dtype)
    mb.bt_h[0, :nblk] = np.arange(1, nblk + 1)
    _, nt, nl = mb.fill([0], [T], [T], [toks])
    mb.upload(T, nl, 1)
    part, nparts = plan_partitions(nt, model.n_kv, T)
    meta = mb.meta(T, nt, nl, part, nparts, mb.npt)
    ts = torch.full((T,), slot, dtype=torch.int32)
    with torch.no_grad():
        h = model.forward(mb.ids_d[:T], meta, kv, lora=stacks.step(ts))
        return model.logits(h).float()


@pytest.mark.parametrize("fold", [True, False])
def test_transformers_parity(tmp_path, fold):
    hf = _tiny_hf(tmp_path / "base")
    ours = loader.load_pretrained(tmp_path / "base", device="cpu", dtype=torch.float32, fold_norms=fold)
    assert ours.unit_norms == fold
    full = write_adapter(tmp_path / "full", ours.cfg, r=8, alpha=16.0, seed=1)
    qv = write_adapter(tmp_path / "qv", ours.cfg, r=4, alpha=8.0, targets=("q_proj", "v_proj"), seed=2, rslora=True)
    stacks = LoraStacks(ours, 3, 16)
    for slot, d in ((2, full), (0, qv)):
        stacks.load(slot, loader.load_adapter(d, ours.cfg))
    toks = torch.randint(3, 500, (37,), generator=torch.Generator().manual_seed(5)).tolist()
    with torch.no_grad():
        base = hf(torch.tensor([toks])).logits[0].float()
    for slot, d in ((2, full), (0, qv)):
        with torch.no_grad():
            ref = _merge_into_hf(hf, d)(torch.tensor([toks])).logits[0].float()
        assert (ref - base).abs().max() > 0.05, "the adapter must move the logits for the test to mean anything"
        torch.testing.assert_close(lora_logits(ours, stacks, toks, slot), ref, atol=2e-4, rtol=1e-3)
    # rows without an adapter ride the LoRA forward unchanged; an empty slot is the base model too
    torch.testing.assert_close(lora_logits(ours, stacks, toks, -1), base, atol=2e-4, rtol=1e-3)
    torch.testing.assert_close(lora_logits(ours, stacks, toks, 1), base, atol=2e-4, rtol=1e-3)
    # the merged copy in our layout (the GPU tests' oracle) agrees with the merged HF model
    ad = loader.load_adapter(full, ours.cfg)
    torch.testing.assert_close(dense_logits(merged_copy(ours, ad), toks),
                               _merge_into_hf(hf, full)(torch.tensor([toks])).logits[0].float(),
                               atol=2e-4, rtol=1e-3)


def test_engine_greedy_matches_hf_generate(tmp_path):
    hf = _tiny_hf(tmp_path / "base")
    ours = loader.load_pretrained(tmp_path / "base", device="cpu", dtype=torch.float32)
    dirs = {"full": write_adapter(tmp_path / "full", ours.cfg, r=8, seed=1),
            "qv": write_adapter(tmp_path / "qv", ours.cfg, r=4, alpha=8.0, targets=("q_proj", "v_proj"), seed=2,
                                rslora=True)}
    eng = Engine(ours, EngineConfig(max_num_seqs=4, max_num_batched_tokens=32, max_model_len=256, num_kv_blocks=64,
                                    use_graphs=False, max_adapters=2, max_lora_rank=8))
    for n, d in dirs.items():
        eng.load_adapter(n, d)
    assert [a["name"] for a in eng.adapters()] == ["full", "qv"]
    g = torch.Generator().manual_seed(9)
    prompts = [torch.randint(3, 500, (n,), generator=g).tolist() for n in (21, 40, 7)]
    names = ["full", "qv", None]
    outs = eng.generate(prompts, [SamplingParams(max_tokens=8, ignore_eos=True, adapter=n) for n in names])
    assert eng.stats["lora_steps"] > 0
    for p, n, o in zip(prompts, names, outs):
        m = hf if n is None else _merge_into_hf(hf, dirs[n])
        ref = m.generate(torch.tensor([p]), max_new_tokens=8, do_sample=False, min_new_tokens=8, pad_token_id=0,
                         eos_token_id=None)[0, len(p):].tolist()
        assert o == ref, n
    assert eng.alloc.num_free == eng.alloc.available - 1 or not eng.cfg.enable_prefix_caching


# --------------------------------------------------------------- loader rejections --

def _rejects(tmp_path, match, cfg=TINY_LLAMA, **kw):
    d = write_adapter(tmp_path / "ad", TINY_LLAMA, **kw)
    with pytest.raises(ValueError, match=match):
        loader.load_adapter(d, cfg)


def test_loader_accepts_and_lays_out(tmp_path):
    ad = loader.load_adapter(write_adapter(tmp_path / "ok", TINY_LLAMA, r=8, alpha=4.0, targets=("k_proj", "up_proj")),
                             TINY_LLAMA)
    assert ad.rank == 8 and set(ad.layers[0]) == {"qkv", "gate_up"} and len(ad.digest) == 16
    A, B = ad.layers[0]["qkv"]
    assert A.shape == (3, 8, 256) and B.shape == (TINY_LLAMA.q_size + 2 * TINY_LLAMA.kv_size, 8)
    assert not A[0].any() and A[1].any() and not A[2].any()
    assert not B[:TINY_LLAMA.q_size].any() and B[TINY_LLAMA.q_size:TINY_LLAMA.q_size + 128].any()
    A, B = ad.layers[1]["gate_up"]  # up rows only: the odd 16-row groups of the interleaved layout
    assert not B.view(-1, 2, 16, 8)[:, 0].any() and B.view(-1, 2, 16, 8)[:, 1].any()


def test_rejects_mixtral(tmp_path):
    _rejects(tmp_path, "Mixtral", cfg=TINY_MIXTRAL)


def test_rejects_dora(tmp_path):
    _rejects(tmp_path, "DoRA", extra_cfg={"use_dora": True})


def test_rejects_bias(tmp_path):
    _rejects(tmp_path, "bias", extra_cfg={"bias": "all"})


def test_rejects_modules_to_save(tmp_path):
    _rejects(tmp_path, "modules_to_save", extra_cfg={"modules_to_save": ["lm_head"]})


def test_rejects_rank_pattern(tmp_path):
    _rejects(tmp_path, "rank_pattern", extra_cfg={"rank_pattern": {"q_proj": 4}})


def test_rejects_alpha_pattern(tmp_path):
    _rejects(tmp_path, "alpha_pattern", extra_cfg={"alpha_pattern": {"q_proj": 4}})


def test_rejects_embedding_and_lm_head_targets(tmp_path):
    for t in ("embed_tokens", "lm_head"):
        _rejects(tmp_path, "target_modules", extra_cfg={"target_modules": ["q_proj", t]})


def test_rejects_rank_above_maximum(tmp_path):
    _rejects(tmp_path, "rank", r=128)
    d = write_adapter(tmp_path / "r16", TINY_LLAMA, r=16)
    with pytest.raises(ValueError, match="rank"):
        loader.load_adapter(d, TINY_LLAMA, max_rank=8)


def test_rejects_shape_mismatch_and_stray_tensors(tmp_path):
    d = write_adapter(tmp_path / "stray", TINY_LLAMA, extra_tensors={
        "base_model.model.lm_head.lora_A.weight": torch.zeros(8, 256)})
    with pytest.raises(ValueError, match="outside"):
        loader.load_adapter(d, TINY_LLAMA)
    from dataclasses import replace

    with pytest.raises(ValueError, match="do not fit"):
        loader.load_adapter(write_adapter(tmp_path / "ok", TINY_LLAMA), replace(TINY_LLAMA, intermediate_size=1024))


def test_engine_rejects_tp_ep_mixtral_and_disabled():
    from mlopamd.parallel.comm import Group, ParallelState

    torch.manual_seed(0)
    with pytest.raises(ValueError, match="Mixtral"):
        Engine(build_model(TINY_MIXTRAL, device="cpu", dtype=torch.float32),
               EngineConfig(max_num_seqs=2, num_kv_blocks=8, use_graphs=False, max_adapters=1))
    m = build_model(TINY_LLAMA, device="cpu", dtype=torch.float32)
    eng = Engine(m, EngineConfig(max_num_seqs=2, num_kv_blocks=8, use_graphs=False))
    assert eng.lora is None and eng.adapters() == []
    with pytest.raises(ValueError, match="max_adapters"):
        eng.load_adapter("x", "/nonexistent")
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.add_request([3, 4], SamplingParams(adapter="x"))
    for field in ("tp", "ep"):
        ps = ParallelState(tp=Group(size=2 if field == "tp" else 1), ep=Group(size=2 if field == "ep" else 1))
        fake = type("M", (), {"cfg": TINY_LLAMA, "ps": ps})()
        with pytest.raises(ValueError, match="TP = 1"):
            LoraStacks(fake, 1)


def test_adapter_uri_resolution(tmp_path, monkeypatch):
    d = write_adapter(tmp_path / "root" / "adapters" / "a", TINY_LLAMA)
    assert loader.resolve_adapter_dir(f"file://{d}") == d and loader.resolve_adapter_dir(str(d)) == d
    assert loader.resolve_adapter_dir("s3://mlflow/adapters/a") is None
    monkeypatch.setenv("MLOP_ARTIFACT_ROOT", str(tmp_path / "root"))
    assert loader.resolve_adapter_dir("s3://mlflow/adapters/a") == d
    assert loader.resolve_adapter_dir("https://example.com/a") is None
    assert loader.resolve_model_dir(str(d)) is None  # an adapter directory is no checkpoint


# ------------------------------------------------------------------- engine logic --

@pytest.fixture(scope="module")
def tiny():
    torch.manual_seed(0)
    return build_model(TINY_LLAMA, device="cpu", dtype=torch.float32, seed=1)


@pytest.fixture(scope="module")
def adapter_dirs(tmp_path_factory):
    root = tmp_path_factory.mktemp("adapters")
    return {"x": write_adapter(root / "x", TINY_LLAMA, r=8, seed=11, std=0.07),
            "y": write_adapter(root / "y", TINY_LLAMA, r=16, seed=12, std=0.07),
            "z": write_adapter(root / "z", TINY_LLAMA, r=4, seed=13, std=0.07, targets=("q_proj", "down_proj"))}


def test_prefix_cache_is_per_adapter(tiny, adapter_dirs):
    eng = Engine(tiny, EngineConfig(max_num_seqs=4, max_model_len=256, num_kv_blocks=64, use_graphs=False,
                                    max_adapters=2))
    eng.load_adapter("x", adapter_dirs["x"])
    eng.load_adapter("y", adapter_dirs["y"])
    prompt = torch.randint(3, 500, (100,), generator=torch.Generator().manual_seed(3)).tolist()

    def hits(adapter):
        before = eng.stats["prefix_hit_tokens"]
        out = eng.generate([prompt], SamplingParams(max_tokens=3, ignore_eos=True, adapter=adapter))[0]
        return eng.stats["prefix_hit_tokens"] - before, out

    h1, o1 = hits("x")
    h2, o2 = hits("x")
    h3, o3 = hits("y")
    h4, o4 = hits(None)
    assert (h1, h3, h4) == (0, 0, 0) and h2 == 96 and o1 == o2
    assert len({tuple(o1), tuple(o3), tuple(o4)}) == 3, "adapters this large change the greedy tokens"
    h5, _ = hits(None)
    assert h5 == 96  # base requests share among themselves, as before
    # same name, same slot, other weights: no stale hit
    slot = eng.adapters()[0]["slot"]
    eng.unload_adapter("x")
    eng.load_adapter("x", adapter_dirs["z"])
    assert eng.adapters()[-1]["slot"] == slot
    h6, o6 = hits("x")
    assert h6 == 0 and o6 != o1
    # the engine's tokens are the merged model's
    ad = loader.load_adapter(adapter_dirs["z"], tiny.cfg)
    toks = list(prompt)
    for t in o6:
        assert t == int(dense_logits(merged_copy(tiny, ad), toks)[-1].argmax())
        toks.append(t)


def test_unload_refused_while_in_use(tiny, adapter_dirs):
    eng = Engine(tiny, EngineConfig(max_num_seqs=4, max_model_len=256, num_kv_blocks=64, use_graphs=False,
                                    max_adapters=1))
    eng.load_adapter("x", adapter_dirs["x"])
    with pytest.raises(ValueError, match="slots"):
        eng.load_adapter("y", adapter_dirs["y"])
    with pytest.raises(ValueError, match="already"):
        eng.load_adapter("x", adapter_dirs["x"])
    s = eng.add_request([5, 6, 7, 8], SamplingParams(max_tokens=4, ignore_eos=True, adapter="x"))
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("x")
    eng.step()
    with pytest.raises(RuntimeError, match="in use"):
        eng.unload_adapter("x")
    while eng.has_work():
        eng.step()
    assert len(s.output) == 4
    eng.unload_adapter("x")
    assert eng.adapters() == []
    with pytest.raises(ValueError, match="unknown adapter"):
        eng.add_request([5, 6], SamplingParams(adapter="x"))
    s2 = eng.add_request([5, 6, 7, 8], SamplingParams(max_tokens=2, adapter=None))
    eng.abort(s2.seq_id)
    eng.load_adapter("y", adapter_dirs["y"])
    s3 = eng.add_request([5, 6, 7, 8], SamplingParams(max_tokens=2, adapter="y"))
    eng.abort(s3.seq_id)
    eng.unload_adapter("y")  # an aborted request no longer holds it


def test_async_matches_sync_with_adapters(tiny, adapter_dirs):
    """One-step-ahead scheduling with adapter rows: stop tokens (a row decoded once more, its
    result dropped), an abort and preemptions give exactly the synchronous engine's outputs."""
    rng = np.random.default_rng(11)
    prompts = [rng.integers(2, 500, size=int(rng.integers(3, 50))).tolist() for _ in range(14)]
    names = [("x", "y", None)[i % 3] for i in range(len(prompts))]

    def engine(**kw):
        eng = Engine(tiny, EngineConfig(max_model_len=256, use_graphs=False, max_adapters=2, **kw))
        eng.load_adapter("x", adapter_dirs["x"])
        eng.load_adapter("y", adapter_dirs["y"])
        return eng

    probe = engine(max_num_seqs=8, num_kv_blocks=64, async_scheduling=False)
    third = probe.generate(prompts, [SamplingParams(max_tokens=3, ignore_eos=True, adapter=n) for n in names])
    params = [SamplingParams(max_tokens=int(6 + 4 * (i % 9)), ignore_eos=True, adapter=names[i],
                             stop_token_ids=[third[i][2]] if i % 2 else []) for i in range(len(prompts))]

    def run(asy):
        eng = engine(max_num_seqs=5, max_num_batched_tokens=40, num_kv_blocks=10, mixed_min_chunk=8,
                     async_scheduling=asy)
        seqs, i, it = [], 0, 0
        while i < len(prompts) or eng.has_work():
            if i < len(prompts) and it % 2 == 0:
                seqs.append(eng.add_request(prompts[i], params[i]))
                i += 1
            if it == 12:
                eng.abort(seqs[-1].seq_id)
            eng.step()
            it += 1
        assert eng.alloc.num_free == eng.alloc.available - 1
        assert not eng._slot_refs.any() and (eng.r_slot == -1).all()
        return [(s.output, s.finish_reason) for s in seqs], eng.stats

    sync, st_s = run(False)
    asy, st_a = run(True)
    assert st_a["async_host_us"] > 0 and st_a["lora_steps"] > 0 and st_s["lora_steps"] > 0
    assert st_a["preemptions"] > 0 and st_s["preemptions"] > 0
    assert asy == sync
    assert any(r == "stop" for _, r in asy) and any(r == "abort" for _, r in asy)
    # and the tokens are the merged models': a preempted adapter request kept its adapter
    ads = {n: loader.load_adapter(adapter_dirs[n], tiny.cfg) for n in ("x", "y")}
    merged = {n: merged_copy(tiny, a) for n, a in ads.items()}
    merged[None] = tiny
    for p, n, (out, _) in list(zip(prompts, names, sync))[:6]:
        toks = list(p)
        for t in out:
            assert t == int(dense_logits(merged[n], toks)[-1].argmax())
            toks.append(t)


def test_feature_off_and_base_only_are_unchanged(tiny, adapter_dirs):
    g = torch.Generator().manual_seed(4)
    prompts = [torch.randint(3, 500, (n,), generator=g).tolist() for n in (9, 33, 70)]
    kw = dict(max_num_seqs=4, max_num_batched_tokens=48, max_model_len=256, num_kv_blocks=64, use_graphs=False)
    off = Engine(tiny, EngineConfig(**kw))
    on = Engine(tiny, EngineConfig(max_adapters=2, **kw))
    on.load_adapter("x", adapter_dirs["x"])
    assert off.meta.total == on.meta.total and off.meta.off == on.meta.off
    sp = SamplingParams(max_tokens=6, ignore_eos=True)
    assert off.generate(prompts, sp) == on.generate(prompts, sp)
    assert on.stats["lora_steps"] == 0 and off.stats["lora_steps"] == 0


# ------------------------------------------------------------------------ server --

def _client(app):
    from aiohttp.test_utils import TestClient, TestServer

    return TestClient(TestServer(app))


def test_server_adapter_requests(tiny, adapter_dirs, monkeypatch):
    from mlopamd.runtime.backends import LLMBackend
    from mlopamd.runtime.metrics import RuntimeMetrics
    from mlopamd.runtime.server import load_env_adapters, make_app

    eng = Engine(tiny, EngineConfig(max_num_seqs=4, max_model_len=256, num_kv_blocks=64, use_graphs=False,
                                    max_adapters=2))
    b = LLMBackend(eng, RuntimeMetrics("llm", "v1", "ns", "tiny"), name="tiny")
    assert "adapters" not in b.metadata()
    monkeypatch.setenv("MLOP_ADAPTERS", json.dumps([{"name": "x", "uri": f"file://{adapter_dirs['x']}"},
                                                    {"name": "y", "uri": str(adapter_dirs["y"])}]))
    assert load_env_adapters(eng) == ["x", "y"]
    monkeypatch.setenv("MLOP_ADAPTERS", json.dumps([{"name": "w", "uri": "file:///nonexistent"}]))
    with pytest.raises(FileNotFoundError):
        load_env_adapters(eng)
    b.start()

    async def go():
        async with _client(make_app(b, b.metrics)) as c:
            md = await (await c.get("/v2/models/tiny")).json()
            assert md["adapters"] == [{"name": "x", "rank": 8}, {"name": "y", "rank": 16}]
            outs = {}
            for ad in ("x", "y", None):
                p = {"max_tokens": 5, "ignore_eos": True}
                if ad:
                    p["adapter"] = ad
                r = await c.post("/v2/models/tiny/generate", json={"input_ids": [5, 6, 7, 8, 9], "parameters": p})
                assert r.status == 200, await r.text()
                outs[ad] = (await r.json())["output_ids"]
            assert len({tuple(v) for v in outs.values()}) == 3
            for bad in ("nope", 7, ""):
                r = await c.post("/v2/models/tiny/generate", json={"input_ids": [5, 6, 7], "parameters": {
                    "adapter": bad, "max_tokens": 2}})
                assert r.status == 400, (bad, r.status)
            r = await c.post("/v2/models/tiny/infer", json={"inputs": [
                {"name": "input_ids", "shape": [3], "datatype": "INT64", "data": [5, 6, 7]}],
                "parameters": {"adapter": "nope"}})
            assert r.status == 400
            r = await c.post("/v2/models/tiny/generate", json={"input_ids": [5, 6, 7], "parameters": {
                "max_tokens": 2, "ignore_eos": True}})
            assert r.status == 200  # the engine loop is still serving
    try:
        asyncio.run(go())
    finally:
        b.stop()


def test_ep_predictor_rejects_adapter():
    from mlopamd.runtime.ep_serving import check_ep_request

    check_ep_request(SamplingParams())
    with pytest.raises(ValueError, match="expert-parallel"):
        check_ep_request(SamplingParams(adapter="x"))


# ---------------------------------------------------------------------- operator --

def test_example_cr_and_schema():
    import yaml

    from mlopamd.controller import crd

    schema = crd.crd_schema()
    with open(crd.MANIFESTS / "examples" / "lora" / "llama3-8b-lora.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr, schema)
    assert errs == [] and pruned == cr
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert spec.validate() == [] and [n for n, _ in spec.adapters] == ["support-bot", "sql-assistant"]
    bad = {"apiVersion": "mlflow.nizepart.com/v1alpha1", "kind": "MlflowModel", "metadata": {"name": "x"},
           "spec": {"modelName": "m", "modelAlias": "a", "adapters": [{"name": "n"}, "s"]}}
    _, errs = crd.admit(bad, schema)
    assert any("adapters[0]" in e for e in errs) and any("adapters[1]" in e for e in errs)
    for extra in ({"tensorParallel": 2}, {"expertParallel": 2}):
        s = crd.ModelSpec.from_spec({"modelName": "m", "modelAlias": "a",
                                     "adapters": [{"name": "n", "uri": "s3://mlflow/a"}], **extra})
        assert any("adapters" in e for e in s.validate())
    dup = crd.ModelSpec.from_spec({"modelName": "m", "modelAlias": "a", "adapters": [
        {"name": "n", "uri": "u"}, {"name": "n", "uri": "v"}]})
    assert any("unique" in e for e in dup.validate())


def test_predictor_env_and_unchanged_without_adapters():
    from mlopamd.controller import seldon

    kw = dict(runtime=seldon.RUNTIME_LLM, placement={"tensorParallel": 1, "gpus": 1}, model_name="m",
              deployment="m", namespace="models", architecture="llama3-8b", engine_args={"max_model_len": 4096})
    plain = seldon.build_predictor(3, "s3://mlflow/1/a/artifacts/model", "minio", 100, **kw)
    assert seldon.build_predictor(3, "s3://mlflow/1/a/artifacts/model", "minio", 100, adapters=(), **kw) == plain
    names = [e["name"] for e in plain["componentSpecs"][0]["spec"]["containers"][0]["env"]]
    # the container env of a CR without adapters, as on the commit before this feature
    assert names == ["MLOP_RUNTIME", "MLOP_MODEL_URI", "MLOP_MODEL_NAME", "MLOP_MODEL_VERSION",
                     "SELDON_DEPLOYMENT_ID", "PREDICTOR_ID", "SELDON_NAMESPACE", "HSA_ENABLE_IPC_MODE_LEGACY",
                     "MLOP_ARCHITECTURE", "MLOP_ENGINE_MAX_MODEL_LEN"]
    with_ad = seldon.build_predictor(3, "s3://mlflow/1/a/artifacts/model", "minio", 100,
                                     adapters=(("a", "s3://mlflow/adapters/a"), ("b", "file:///b")), **kw)
    env = {e["name"]: e["value"] for e in with_ad["componentSpecs"][0]["spec"]["containers"][0]["env"]}
    assert json.loads(env["MLOP_ADAPTERS"]) == [{"name": "a", "uri": "s3://mlflow/adapters/a"},
                                                {"name": "b", "uri": "file:///b"}]
    assert env["MLOP_ENGINE_MAX_ADAPTERS"] == "2"
    stripped = json.loads(json.dumps(with_ad))
    c = stripped["componentSpecs"][0]["spec"]["containers"][0]
    c["env"] = [e for e in c["env"] if e["name"] not in ("MLOP_ADAPTERS", "MLOP_ENGINE_MAX_ADAPTERS")]
    assert stripped == plain


def test_operator_deploys_adapters_and_refuses_tp(monkeypatch):
    from test_controller import GROUP, NS, PLURAL, VERSION, Env, _ready, run

    async def go():
        env = Env()
        v = env.version(tags={"mlop.architecture": "llama3-8b"})
        env.reg.set_alias("m", "champion", v)
        await env.start()
        ads = [{"name": "a", "uri": "s3://mlflow/adapters/a"}, {"name": "b", "uri": "s3://mlflow/adapters/b"}]
        await env.create_cr(tensorParallel=1, adapters=ads)
        assert await env.run_until(lambda: _ready(env))
        assert "error" not in await env.status()
        (p,) = (await env.sd())["spec"]["predictors"]
        e = {x["name"]: x["value"] for x in p["componentSpecs"][0]["spec"]["containers"][0]["env"]}
        assert json.loads(e["MLOP_ADAPTERS"]) == ads and e["MLOP_ENGINE_MAX_ADAPTERS"] == "2"
        await env.stop()

        env = Env()
        v = env.version(tags={"mlop.architecture": "llama3-70b"})
        env.reg.set_alias("m", "champion", v)
        await env.start()
        await env.create_cr(tensorParallel=2, adapters=ads)
        await env.clock.sleep(5)
        st = await env.status()
        assert st["phase"] == "Invalid" and "adapters" in st["error"]
        assert await env.sd() is None  # a status.error, not a pod
        await env.stop()
    run(go())
