"""The engine with expert_weight_dtype="mxfp4" on a prompt chunk whose experts average about 200 rows (TINY_MIXTRAL:
4 experts, top-2, a 400-token prompt in one 512-token step), so both expert GEMMs take moe_mx4t.hip: greedy tokens
against the fake-quant fp32 oracle under the project's near-tie rule, eager and with decode graphs."""
import pytest
import torch

from mlopamd import ops
from mlopamd.models import build_model
from mlopamd.models.config import TINY_MIXTRAL
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams
from test_fp8_kv_engine_gpu import _check_greedy

pytestmark = pytest.mark.gpu


def test_long_chunk_matches_fake_quant_oracle(gpu, monkeypatch):
    monkeypatch.setattr(ops, "MX4_MOE_TILE_MIN_AVG_ROWS", 64)
    monkeypatch.setattr(ops, "MX4_MOE_TILE_MAX_AVG_ROWS", 1024)
    model = build_model(TINY_MIXTRAL, device=gpu, seed=3)
    with torch.no_grad():
        for L in model.layers:
            L["router"].mul_(4)  # spread the router logits: the routing, not near-ties, decides
    g = torch.Generator().manual_seed(1)
    prompts = [torch.randint(2, 500, (n,), generator=g).tolist() for n in (400, 9, 21)]
    for graphs in (False, True):
        eng = Engine(model, EngineConfig(max_num_seqs=8, max_num_batched_tokens=512, max_model_len=512, num_kv_blocks=256,
                                         use_graphs=graphs, graph_buckets=(1, 2, 4, 8), expert_weight_dtype="mxfp4"))
        assert isinstance(model.layers[0]["w13"], ops.Mx4Experts)
        outs = eng.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))
        assert all(len(o) == 6 for o in outs) and (eng.stats["graph_steps"] > 0 or not graphs)
        _check_greedy(model, prompts, outs, expert_weight_dtype="mxfp4")
