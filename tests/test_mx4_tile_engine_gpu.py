"""The mxfp4 engine with the fused tiled kernel (gemm_mx4t.hip) serving 65 .. 256 rows: prompts of 96 and
200 tokens against the fake-quant fp32 oracle, and a 72-request decode eagerly and through the graphs."""
import pytest
import torch

from mlopamd import ops
from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from test_fp8_kv_engine_gpu import _check_greedy

pytestmark = pytest.mark.gpu


def _engine(model, graphs):
    return Engine(model, EngineConfig(max_num_seqs=72, max_num_batched_tokens=256, max_model_len=512,
                                      num_kv_blocks=256, use_graphs=graphs, graph_buckets=(1, 72),
                                      weight_dtype="mxfp4"))


def test_mxfp4_tile_engine(gpu, monkeypatch):
    monkeypatch.setattr(ops, "MX4_TILE_MAX_M", 256)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(2, 500, (n,), generator=g).tolist() for n in (96, 200)]
    oracle, model = build_model(TINY_LLAMA, device=gpu, seed=3), build_model(TINY_LLAMA, device=gpu, seed=3)
    eager = _engine(model, False)
    sp = SamplingParams(max_tokens=8, ignore_eos=True)
    for p in prompts:  # one prompt per step: the prefill GEMMs run at 96 and at 200 rows
        _check_greedy(oracle, [p], eager.generate([p], sp), weight_dtype="mxfp4")
    many = [torch.randint(2, 500, (3,), generator=g).tolist() for _ in range(72)]
    want = eager.generate(many, sp)
    graphs = _engine(model, True)
    got = graphs.generate(many, sp)
    assert graphs.stats["graph_steps"] > 0
    assert got == want  # the same deterministic kernels, replayed: no tolerance
