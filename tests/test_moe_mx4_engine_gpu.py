"""The engine with expert_weight_dtype="mxfp4" on the GPU: TINY_MIXTRAL (small / mid dispatch) and the
128-expert tiny Qwen3-MoE of test_qwen3_moe_engine_gpu with intermediate_size 128 (wide dispatch),
eager and decode graphs, 3 and 40 requests (both sides of the 16-token dispatch boundary) - greedy
tokens against the fake-quant fp32 oracle with the project's near-tie rule; a bf16 engine beside it."""
import dataclasses

import pytest
import torch

from mlopamd import ops
from mlopamd.models import build_model
from mlopamd.models.config import TINY_MIXTRAL, get_config
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

pytestmark = pytest.mark.gpu
GEN = 12
QWEN3_MOE = dataclasses.replace(get_config("tiny-qwen3"), name="tiny-qwen3-moe", num_experts=128, top_k=8,
                                intermediate_size=128)


def _model(cfg, gpu):
    m = build_model(cfg, device=gpu, seed=3)
    g = torch.Generator().manual_seed(9)
    with torch.no_grad():
        for L in m.layers:
            for k in ("in_norm", "post_norm", "q_norm", "k_norm"):
                if k in L:
                    L[k].copy_((1 + 0.2 * torch.randn(L[k].shape, generator=g)).to(gpu, L[k].dtype))
            L["router"].mul_(4)  # spread the router logits: the routing, not near-ties, decides
    m.unit_norms = False
    return m


def _engine(model, graphs, **kw):
    return Engine(model, EngineConfig(max_num_seqs=64, max_num_batched_tokens=64, max_model_len=256, num_kv_blocks=256,
                                      use_graphs=graphs, graph_buckets=(1, 2, 4, 8, 16, 32, 64), **kw))


def _prompts(batch):
    g = torch.Generator().manual_seed(batch)
    lens = [150, 10, 60] + [int(n) for n in torch.randint(4, 24, (batch - 3,), generator=g)]
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in lens]


@pytest.fixture(scope="module", params=[TINY_MIXTRAL, QWEN3_MOE], ids=lambda c: c.name)
def model(request, gpu):
    m = _model(request.param, gpu)
    bf16_bytes = m.weight_bytes()
    _engine(m, False, expert_weight_dtype="mxfp4")                         # quantises the experts in place
    assert m.weight_bytes() == request.param.weight_bytes(expert_weight_dtype="mxfp4") < bf16_bytes
    return m


@pytest.mark.parametrize("batch", [3, 40])
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graphs"])
def test_engine_matches_fake_quant_oracle(model, graphs, batch):
    prompts = _prompts(batch)
    eng = _engine(model, graphs, expert_weight_dtype="mxfp4")
    L = model.layers[0]
    assert isinstance(L["w13"], ops.Mx4Experts) and isinstance(L["w2"], ops.Mx4Experts) and isinstance(L["qkv"], torch.Tensor)
    outs = eng.generate(prompts, SamplingParams(max_tokens=GEN, ignore_eos=True))
    assert all(len(o) == GEN for o in outs)
    if graphs:
        assert eng.stats["graph_steps"] > 0
    assert eng.alloc.num_free == eng.alloc.available - 1                  # every page came back
    for p, o in list(zip(prompts, outs))[:6]:  # the long chunked prompt and five more rows
        toks = list(p)
        for t in o:
            lg = dense_logits(model, toks, expert_weight_dtype="mxfp4")[-1]
            best = int(lg.argmax())
            assert t == best or float(lg[best] - lg[t]) < 0.05 * float(lg.std()), (len(toks), best, t)
            toks.append(t)


def test_bf16_engine_unchanged(gpu):
    """expert_weight_dtype="bf16" is the field-less engine: the same tokens, plain tensors."""
    sp = SamplingParams(max_tokens=GEN, ignore_eos=True)
    a, b = _model(TINY_MIXTRAL, gpu), _model(TINY_MIXTRAL, gpu)
    eng = _engine(a, False, expert_weight_dtype="bf16")
    assert "expert_weight_dtype" not in eng.stats and isinstance(a.layers[0]["w13"], torch.Tensor)
    assert a.weight_bytes() == TINY_MIXTRAL.weight_bytes()
    assert eng.generate(_prompts(5), sp) == _engine(b, False).generate(_prompts(5), sp)
