"""The serving engine with weight_dtype="int4" on the GPU: prompt chunks above 64 rows (dequantise +
bf16 GEMMs) and decode steps (gemm_q4.hip), eager and under decode graphs, against the dense fp32
oracle that fake-quantises the four projections of an untouched bf16 copy of the model."""
import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_QWEN3
from mlopamd.models.reference import dense_logits
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
                                          (TINY_QWEN3, False, "bf16"), (TINY_QWEN3, True, "bf16"),
                                          (TINY_LLAMA, False, "fp8")],
                         ids=["llama-eager", "llama-graphs", "qwen3-eager", "qwen3-graphs", "llama-fp8kv"])
def test_int4_engine_matches_fake_quant_oracle(gpu, prompts, mc, graphs, kv):
    oracle, model = build_model(mc, device=gpu, seed=3), build_model(mc, device=gpu, seed=3)
    eng = _engine(model, graphs, weight_dtype="int4", kv_cache_dtype=kv)
    assert eng.stats["weight_dtype"] == "int4" and isinstance(model.layers[0]["qkv"], tuple)
    assert model.weight_bytes() == mc.weight_bytes(weight_dtype="int4") < oracle.weight_bytes()
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert all(len(o) == GEN for o in outs)
    if graphs:
        assert eng.stats["graph_steps"] > 0
    assert eng.alloc.num_free == eng.alloc.available - 1                  # every page came back
    _check_greedy(oracle, prompts, outs, weight_dtype="int4", **({"kv_cache_dtype": "fp8"} if kv == "fp8" else {}))


def test_bf16_weight_dtype_changes_nothing(gpu, prompts):
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    a = _engine(build_model(TINY_LLAMA, device=gpu, seed=3)).generate(prompts, sp)
    model = build_model(TINY_LLAMA, device=gpu, seed=3)
    eng = _engine(model, weight_dtype="bf16")
    assert "weight_dtype" not in eng.stats and isinstance(model.layers[0]["qkv"], torch.Tensor)
    assert eng.generate(prompts, sp) == a
