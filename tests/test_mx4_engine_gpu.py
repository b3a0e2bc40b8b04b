"""The engine with weight_dtype="mxfp4" on the GPU (dequantise + GEMM above 64 rows, gemm_mx4.hip for
decode, eager and graphs) against the fake-quant fp32 oracle; int4 and bf16 engines beside it."""
import pytest
import torch

from mlopamd import ops
from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_QWEN3
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from test_fp8_kv_engine_gpu import _check_greedy

pytestmark = pytest.mark.gpu
GEN = 24


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]


def _engine(model, graphs=False, **kw):
    cfg = dict(max_num_seqs=8, max_num_batched_tokens=128, max_model_len=512, num_kv_blocks=128,
               use_graphs=graphs, graph_buckets=(1, 2, 4, 8))
    cfg.update(kw)
    return Engine(model, EngineConfig(**cfg))


@pytest.mark.parametrize("mc,graphs,kv", [(TINY_LLAMA, False, "bf16"), (TINY_LLAMA, True, "bf16"),
                                          (TINY_QWEN3, False, "bf16"), (TINY_LLAMA, False, "fp8")],
                         ids=["llama-eager", "llama-graphs", "qwen3-eager", "llama-fp8kv"])
def test_mxfp4_engine_matches_fake_quant_oracle(gpu, prompts, mc, graphs, kv):
    oracle, model = build_model(mc, device=gpu, seed=3), build_model(mc, device=gpu, seed=3)
    eng = _engine(model, graphs, weight_dtype="mxfp4", kv_cache_dtype=kv)
    assert eng.stats["weight_dtype"] == "mxfp4" and isinstance(model.layers[0]["qkv"], ops.Mx4Weight)
    assert model.weight_bytes() == mc.weight_bytes(weight_dtype="mxfp4") < oracle.weight_bytes()
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert all(len(o) == GEN for o in outs)
    if graphs:
        assert eng.stats["graph_steps"] > 0
    assert eng.alloc.num_free == eng.alloc.available - 1                  # every page came back
    _check_greedy(oracle, prompts, outs, weight_dtype="mxfp4", **({"kv_cache_dtype": "fp8"} if kv == "fp8" else {}))


def test_int4_and_bf16_engines_unchanged(gpu, prompts):
    """The int4 engine still holds tuples and follows its oracle; bf16 gives the field-less engine's tokens."""
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    _engine(build_model(TINY_LLAMA, device=gpu, seed=3), weight_dtype="mxfp4").generate(prompts[:1], sp)
    oracle, model = build_model(TINY_LLAMA, device=gpu, seed=3), build_model(TINY_LLAMA, device=gpu, seed=3)
    eng = _engine(model, weight_dtype="int4")
    assert eng.stats["weight_dtype"] == "int4" and isinstance(model.layers[0]["qkv"], tuple)
    _check_greedy(oracle, prompts, eng.generate(prompts, sp), weight_dtype="int4")
    eng = _engine(oracle, weight_dtype="bf16")
    assert "weight_dtype" not in eng.stats and isinstance(oracle.layers[0]["qkv"], torch.Tensor)
    assert eng.generate(prompts, sp) == _engine(build_model(TINY_LLAMA, device=gpu, seed=3)).generate(prompts, sp)
