"""The fp8 KV cache on CPU: the row format's rule (ops/reference.py), the reference engine
serving e4m3fn pages against the fake-quantising dense oracle, page capacity, placement, and
the control plane's spec.kvCacheDtype."""
import dataclasses

import pytest
import torch
import yaml

from mlopamd.controller import crd, placement, seldon
from mlopamd.controller.kube import ApiError
from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_MIXTRAL, get_config
from mlopamd.models.reference import dense_logits
from mlopamd.ops import reference as ref
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.kv_cache import KVCache, blocks_for_budget, kv_dtype_bytes
from mlopamd.runtime.sampler import SamplingParams

bf = torch.bfloat16
D = 128


# ------------------------------------------------------------------ format --

@pytest.mark.parametrize("mag", [1e-6, 0.03, 1.0, 37.0, 1e4])
def test_quantiser_properties(mag):
    g = torch.Generator().manual_seed(int(mag * 1e6) % 9973)
    x = (torch.randn(512, D, generator=g) * mag).to(bf)
    q8, sb = ref.fp8_quantize_rows(x)
    assert q8.dtype == torch.float8_e4m3fn and sb.dtype == torch.uint8 and sb.shape == (512,)
    scale = ref.fp8_scale_decode(sb)
    e = sb.to(torch.int32) - 127
    assert torch.equal(scale, torch.ldexp(torch.ones(512), e))              # a power of two
    ratio = x.float().abs().amax(-1) / scale
    assert float(ratio.min()) > 224 and float(ratio.max()) <= 448          # the smallest exponent that fits
    deq = ref.fp8_dequantize_rows(q8, sb)
    bound = 2.0 ** -4 * x.float().abs() + 2.0 ** -10 * scale[:, None]      # half an ulp + half the subnormal step
    assert ((deq - x.float()).abs() <= bound).all()
    assert torch.equal(ref.fp8_fake_quant(x), deq)


def test_quantiser_exact_rows_and_zero():
    z8, zb = ref.fp8_quantize_rows(torch.zeros(3, D, dtype=bf))
    assert int(z8.view(torch.uint8).sum()) == 0                             # zero bytes ...
    assert (zb == ref.FP8_EXP_MIN + 127).all()                              # ... the smallest exponent
    assert torch.isfinite(ref.fp8_scale_decode(zb)).all() and (ref.fp8_scale_decode(zb) > 0).all()
    # byte 0 (a zero-initialised scale tensor) and every byte the quantiser can write are finite
    every = ref.fp8_scale_decode(torch.arange(0, 255, dtype=torch.uint8))
    assert torch.isfinite(every).all() and float(every[0]) == 0.0
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-1, 2, (64, D), generator=g).to(bf)                   # 0 / +-1 rows
    x[0] = 0
    assert torch.equal(ref.fp8_fake_quant(x), x.float())
    # the exponent steps where amax / 2^e would pass 448 = 0.875 * 2^9
    amax = torch.tensor([448.0, 449.0, 224.0, 225.0, 1.75, 1.7578125])
    assert ref.fp8_row_exponent(amax).tolist() == [0, 1, -1, 0, -8, -7]
    # clamped at both ends of the storage's range
    assert ref.fp8_row_exponent(torch.tensor([1e-45, 3e38])).tolist() == [ref.FP8_EXP_MIN, 120]


def test_reference_ops_take_fp8_pages():
    """ref.rope_cache / gather_kv / paged_attention on an e4m3fn cache: the pages hold the
    quantised rows, and attention over them equals attention over their dequantised copy."""
    g = torch.Generator().manual_seed(1)
    Hq, Hkv, T, NB = 4, 2, 21, 4
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=g).to(bf)
    cs = torch.randn(64, D, generator=g)
    pos, slots = torch.arange(T, dtype=torch.int32), torch.arange(16, 16 + T, dtype=torch.int32)
    k8, v8 = (torch.zeros(NB, Hkv, 16, D, dtype=torch.uint8).view(ref.FP8) for _ in range(2))
    ks, vs = (torch.zeros(NB, Hkv, 16, dtype=torch.uint8) for _ in range(2))
    kb, vb = (torch.zeros(NB, Hkv, 16, D, dtype=bf) for _ in range(2))
    q = ref.rope_cache(qkv, pos, cs, slots, k8, v8, Hq, ks, vs)
    assert torch.equal(q, ref.rope_cache(qkv, pos, cs, slots, kb, vb, Hq))
    assert torch.equal(ref.fp8_dequantize_rows(k8, ks), ref.fp8_fake_quant(kb))
    assert torch.equal(ref.fp8_dequantize_rows(v8, vs), ref.fp8_fake_quant(vb))
    with pytest.raises(AssertionError):
        ref.rope_cache(qkv, pos, cs, slots, k8, v8, Hq)

    class M:
        pass

    m = M()
    i32 = lambda *a: torch.tensor(a, dtype=torch.int32)  # noqa: E731
    m.q_start, m.q_len, m.ctx_len, m.tile_seq = i32(0), i32(T), i32(T), i32(0)
    m.block_tables = i32([1, 2, 0])
    want = ref.paged_attention(q, ref.fp8_dequantize_rows(k8, ks), ref.fp8_dequantize_rows(v8, vs), m)
    assert torch.equal(ref.paged_attention(q, k8, v8, m, ks, vs), want)


# ------------------------------------------------------------------ engine --

def _check_greedy(model, prompts, outs, tol=0.05, **oracle):
    """The project's near-tie rule: each token is the oracle's argmax, or within tol x the
    logits' standard deviation of it."""
    for p, o in zip(prompts, outs):
        toks = list(p)
        for t in o:
            lg = dense_logits(model, toks, **oracle)[-1]
            best = int(lg.argmax())
            gap = float(lg[best] - lg[t])
            assert t == best or gap < tol * float(lg.std()), (len(toks), best, t, gap)
            toks.append(t)


@pytest.fixture(scope="module")
def tiny():
    return build_model(TINY_LLAMA, device="cpu", seed=3)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]


def test_cpu_engine_serves_fp8_kv(tiny, prompts):
    eng = Engine(tiny, EngineConfig(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512,
                                    num_kv_blocks=128, kv_cache_dtype="fp8"))
    assert eng.kv.fp8 and eng.kv.k[0].dtype == torch.float8_e4m3fn and eng.kv.k_scale[0].dtype == torch.uint8
    assert eng.kv.k_scale[0].shape == (128, tiny.n_kv, 16)
    assert eng.stats["kv_cache_dtype"] == "fp8" and eng.meta.flash_min_q == 1 << 30
    outs = eng.generate(prompts, SamplingParams(max_tokens=40, ignore_eos=True))
    assert all(len(o) == 40 for o in outs)
    assert eng.alloc.num_free == eng.alloc.available - 1      # every page came back (page 0: the null page)
    assert int(eng.kv.k_scale_all.max()) > 0                  # the scale rows were written
    _check_greedy(tiny, prompts, outs, kv_cache_dtype="fp8")


def test_dense_oracle_default_is_unquantised(tiny, prompts):
    a = dense_logits(tiny, prompts[0])
    assert torch.equal(a, dense_logits(tiny, prompts[0], None)) and torch.equal(a, dense_logits(tiny, prompts[0], "bf16"))
    assert not torch.equal(a, dense_logits(tiny, prompts[0], "fp8"))
    with pytest.raises(ValueError):
        dense_logits(tiny, prompts[0], "int4")


def test_rejections(tiny):
    swa = build_model(dataclasses.replace(TINY_LLAMA, sliding_window=48), device="cpu", seed=3)
    with pytest.raises(ValueError, match="sliding"):
        Engine(swa, EngineConfig(max_num_seqs=4, num_kv_blocks=16, kv_cache_dtype="fp8"))
    Engine(swa, EngineConfig(max_num_seqs=4, num_kv_blocks=16))          # bf16 serves it as before
    with pytest.raises(ValueError, match="MoE"):
        Engine(build_model(TINY_MIXTRAL, device="cpu", seed=0), EngineConfig(max_num_seqs=4, num_kv_blocks=16,
                                                                             kv_cache_dtype="fp8"))
    with pytest.raises(ValueError, match="kv_cache_dtype"):
        Engine(tiny, EngineConfig(max_num_seqs=4, num_kv_blocks=16, kv_cache_dtype="fp4"))


# ---------------------------------------------------------------- capacity --

def test_capacity_ratio(tiny):
    """One byte budget: fp8 gets floor(budget / (2 L Hkv 16 (D + s))) pages, s = 1 scale byte per
    row, against floor(budget / (2 L Hkv 16 2 D)) for bf16 - the 2 D / (D + s) = 1.98 ratio."""
    assert kv_dtype_bytes("bf16") == (2, 0) and kv_dtype_bytes("fp8") == (1, 1)
    L, Hkv = TINY_LLAMA.num_layers, tiny.n_kv
    budget = 8 * 2 ** 20 + 12345
    per_bf = 2 * L * Hkv * 16 * 2 * D
    per_f8 = 2 * L * Hkv * 16 * (D + 1)
    assert KVCache.bytes_per_block(L, Hkv, D) == per_bf                    # the defaults stay bf16
    assert KVCache.bytes_per_block(L, Hkv, D, *kv_dtype_bytes("fp8")) == per_f8
    assert blocks_for_budget(budget, L, Hkv, D) == budget // per_bf
    assert blocks_for_budget(budget, L, Hkv, D, *kv_dtype_bytes("fp8")) == budget // per_f8
    nbs = {}
    for dt in ("bf16", "fp8"):
        eng = Engine(tiny, EngineConfig(max_num_seqs=256, max_model_len=2048, kv_cache_bytes=budget, kv_cache_dtype=dt))
        nbs[dt] = eng.alloc.num_blocks
        assert eng.kv.nbytes == nbs[dt] * (per_f8 if dt == "fp8" else per_bf) <= budget
    assert nbs == {"bf16": budget // per_bf, "fp8": budget // per_f8}
    # floor(budget / per_f8) is the floored 2 D / (D + s) multiple of budget / per_bf (no rounding
    # of the bf16 count in between), and the whole-page counts are within a page of that ratio
    assert nbs["fp8"] == (budget * 2 * D) // (per_bf * (D + 1))
    assert abs(nbs["fp8"] - nbs["bf16"] * 2 * D / (D + 1)) < 2 * D / (D + 1) + 1


def test_placement_sizes_fp8_with_scales():
    cfg = get_config("llama3-8b")
    assert cfg.kv_bytes_per_token() == cfg.kv_bytes_per_token(kv_cache_dtype="bf16") == 2 * 32 * 8 * 128 * 2
    assert cfg.kv_bytes_per_token(kv_cache_dtype="fp8") == 2 * 32 * 8 * (128 + 1)
    kw = dict(max_model_len=1024, max_num_seqs=2048)
    bf16, none, fp8 = (placement.plan("llama3-8b", kv_cache_dtype=d, **kw) for d in ("bf16", None, "fp8"))
    assert bf16 == none
    assert fp8.kvGBPerGPU == bf16.kvGBPerGPU and fp8.tensorParallel == bf16.tensorParallel == 1
    # the same free bytes hold 256 / 129 times the tokens
    free = bf16.kvTokenCapacity * cfg.kv_bytes_per_token()
    assert abs(fp8.kvTokenCapacity - free / cfg.kv_bytes_per_token(kv_cache_dtype="fp8")) <= 2
    assert 1.98 < fp8.kvTokenCapacity / bf16.kvTokenCapacity < 1.99
    # a target bf16 cannot hold on one GPU and fp8 can
    big = dict(max_model_len=8192, max_num_seqs=512, requested_tp=1)
    assert not placement.plan("llama3-8b", **big).fits and placement.plan("llama3-8b", kv_cache_dtype="fp8", **big).fits


# ----------------------------------------------------------- control plane --

def _cr(**spec):
    return {"apiVersion": "mlflow.nizepart.com/v1alpha1", "kind": "MlflowModel", "metadata": {"name": "x"},
            "spec": dict({"modelName": "m", "modelAlias": "a"}, **spec)}


def test_crd_field():
    schema = crd.crd_schema()
    assert crd.ModelSpec.from_spec(_cr()["spec"]).kv_cache_dtype is None
    for dt in crd.KV_CACHE_DTYPES:
        pruned, errs = crd.admit(_cr(kvCacheDtype=dt), schema)
        assert errs == [] and pruned["spec"]["kvCacheDtype"] == dt          # declared: not pruned
        spec = crd.ModelSpec.from_spec(pruned["spec"])
        assert spec.kv_cache_dtype == dt and spec.validate() == []
    assert schema["properties"]["spec"]["properties"]["kvCacheDtype"]["enum"] == list(crd.KV_CACHE_DTYPES)
    _, errs = crd.admit(_cr(kvCacheDtype="int4"), schema)
    assert any("kvCacheDtype" in e and "Unsupported value" in e for e in errs)
    assert any("kvCacheDtype" in e for e in crd.ModelSpec.from_spec({"modelName": "m", "modelAlias": "a",
                                                                    "kvCacheDtype": "int4"}).validate())
    ep = crd.ModelSpec.from_spec({"modelName": "m", "modelAlias": "a", "kvCacheDtype": "fp8", "expertParallel": 2})
    assert any("expertParallel" in e for e in ep.validate())
    assert crd.ModelSpec.from_spec({"modelName": "m", "modelAlias": "a", "kvCacheDtype": "bf16",
                                    "expertParallel": 2}).validate() == []


def test_example_cr_admits_and_places():
    with open(crd.MANIFESTS / "examples" / "fp8-kv" / "llama3-8b-fp8-kv.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr)
    assert errs == [] and pruned == cr
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert spec.validate() == [] and spec.kv_cache_dtype == "fp8"
    kw = dict(max_model_len=spec.max_model_len, max_num_seqs=spec.max_num_seqs, requested_tp=spec.tensor_parallel)
    p = placement.plan(spec.architecture, kv_cache_dtype=spec.kv_cache_dtype, **kw)
    assert p.fits and p.gpus == 1
    assert p.kvTokenCapacity > 1.9 * placement.plan(spec.architecture, **kw).kvTokenCapacity


def test_operator_passes_the_dtype_to_the_engine():
    from test_controller import GROUP, NS, PLURAL, VERSION, Env, _ready, run  # noqa: F401

    async def go():
        env = Env()
        v = env.version(tags={"mlop.architecture": "llama3-8b"})
        env.reg.set_alias("m", "champion", v)
        await env.start()
        with pytest.raises(ApiError) as bad:                               # the apiserver's schema: 422
            await env.create_cr(tensorParallel=1, kvCacheDtype="int4")
        assert bad.value.status == 422 and "kvCacheDtype" in bad.value.message
        await env.create_cr(tensorParallel=1, maxModelLen=1024, maxNumSeqs=4096, kvCacheDtype="fp8")
        assert await env.run_until(lambda: _ready(env))
        assert "error" not in await env.status()
        (p,) = (await env.sd())["spec"]["predictors"]
        e = {x["name"]: x["value"] for x in p["componentSpecs"][0]["spec"]["containers"][0]["env"]}
        assert e["MLOP_ENGINE_KV_CACHE_DTYPE"] == "fp8"
        assert p["annotations"][seldon.ANN_PREFIX + "placementKey"].endswith("|kv=fp8")
        cap8 = int(p["annotations"][seldon.ANN_PREFIX + "kvTokenCapacity"])
        want = placement.plan("llama3-8b", max_model_len=1024, max_num_seqs=4096, requested_tp=1, kv_cache_dtype="fp8")
        assert cap8 == want.kvTokenCapacity
        await env.stop()

        env = Env()                                                        # a CR without the field: no env entry
        v = env.version(tags={"mlop.architecture": "llama3-8b"})
        env.reg.set_alias("m", "champion", v)
        await env.start()
        await env.create_cr(tensorParallel=1)
        assert await env.run_until(lambda: _ready(env))
        (p,) = (await env.sd())["spec"]["predictors"]
        names = [x["name"] for x in p["componentSpecs"][0]["spec"]["containers"][0]["env"]]
        assert "MLOP_ENGINE_KV_CACHE_DTYPE" not in names
        assert not any("|kv=" in str(val) for val in p["annotations"].values())
        await env.stop()
    run(go())


def test_server_reports_the_dtype(tiny):
    from mlopamd.runtime.backends import LLMBackend
    from mlopamd.runtime.metrics import RuntimeMetrics
    from mlopamd.runtime.server import engine_kwargs_from_env

    eng = Engine(tiny, EngineConfig(max_num_seqs=4, num_kv_blocks=16, kv_cache_dtype="fp8"))
    met = RuntimeMetrics()
    b = LLMBackend(eng, metrics=met)
    assert b.metadata()["kv_cache_dtype"] == "fp8"
    text = met.exposition().decode()
    line = [ln for ln in text.splitlines() if ln.startswith("mlop_kv_cache_dtype_info{")]
    assert len(line) == 1 and 'dtype="fp8"' in line[0] and line[0].rstrip().endswith(" 1.0")
    assert LLMBackend(Engine(tiny, EngineConfig(max_num_seqs=4, num_kv_blocks=16))).metadata()["kv_cache_dtype"] == "bf16"
    import os
    os.environ["MLOP_ENGINE_KV_CACHE_DTYPE"] = "fp8"
    try:
        assert engine_kwargs_from_env()["kv_cache_dtype"] == "fp8"
    finally:
        del os.environ["MLOP_ENGINE_KV_CACHE_DTYPE"]
