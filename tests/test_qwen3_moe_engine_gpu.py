"""A tiny Qwen3-MoE (tiny-qwen3 with 128 experts, top-8, moe_intermediate 64; every norm weight
randomised) through the serving engine on the GPU: eager and decode graphs, a 3-row and a 40-row
batch, a prompt longer than 64 tokens in chunks, norm_topk_prob on and off - greedy tokens against
the dense fp32 oracle with the project's near-tie rule (test_qwen3_engine_gpu)."""
import dataclasses

import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import get_config
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

pytestmark = pytest.mark.gpu
GEN = 12


@pytest.fixture(scope="module", params=[True, False], ids=["renorm", "raw"])
def model(request, gpu):
    cfg = dataclasses.replace(get_config("tiny-qwen3"), name="tiny-qwen3-moe", num_experts=128, top_k=8,
                              intermediate_size=64, norm_topk_prob=request.param)
    m = build_model(cfg, device=gpu, seed=3)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for L in m.layers:
            for k in ("in_norm", "post_norm", "q_norm", "k_norm"):
                L[k].copy_((1 + 0.2 * torch.randn(L[k].shape, generator=g)).to(gpu, L[k].dtype))
            L["router"].mul_(4)  # spread the router logits: the routing, not near-ties, decides
    m.unit_norms = False
    return m


@pytest.mark.parametrize("batch", [3, 40])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_engine_matches_dense(model, graphs, batch):
    g = torch.Generator().manual_seed(batch)
    lens = [150, 10, 60] + [int(n) for n in torch.randint(4, 24, (batch - 3,), generator=g)]
    prompts = [torch.randint(2, 500, (n,), generator=g).tolist() for n in lens]
    eng = Engine(model, EngineConfig(max_num_seqs=64, max_num_batched_tokens=64, max_model_len=256, num_kv_blocks=256,
                                     use_graphs=graphs, graph_buckets=(1, 2, 4, 8, 16, 32, 64)))
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert all(len(o) == GEN for o in outs)
    if graphs:
        assert eng.stats["graph_steps"] > 0
    for p, o in list(zip(prompts, outs))[:6]:  # the long chunked prompt and five more rows
        toks = list(p)
        for t in o:
            lg = dense_logits(model, toks)[-1]
            best = int(lg.argmax())
            assert t == best or float(lg[best] - lg[t]) < 0.05 * float(lg.std()), (len(toks), best, t)
            toks.append(t)
