"""A sliding-window model through the serving engine on the GPU (windowed HIP kernels, chunked
prefill across the window, hipGraph decode, release of the pages below the window) against
the dense fp32 oracle with the same window."""
import dataclasses

import pytest
import torch

from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA
from mlopamd.models.reference import dense_logits
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

pytestmark = pytest.mark.gpu
W = 48


def _check_greedy(model, prompts, outs, tol=0.05):
    """As test_model_gpu's: each token is the oracle's argmax, or within a near-tie of it."""
    for p, o in zip(prompts, outs):
        toks = list(p)
        for t in o:
            lg = dense_logits(model, toks)[-1]
            best = int(lg.argmax())
            gap = float(lg[best] - lg[t])
            assert t == best or gap < tol * float(lg.std()), (len(toks), best, t, gap)
            toks.append(t)


@pytest.fixture(scope="module")
def swa_model(gpu):
    return build_model(dataclasses.replace(TINY_LLAMA, sliding_window=W), device=gpu, seed=3)


@pytest.fixture(scope="module")
def prompts():
    g = torch.Generator().manual_seed(0)
    return [torch.randint(2, 500, (n,), generator=g).tolist() for n in (10, 60, 150)]


@pytest.mark.parametrize("graphs", [False, True])
def test_windowed_engine_matches_dense(gpu, swa_model, prompts, graphs):
    outs = {}
    for release in (True, False):
        eng = Engine(swa_model, EngineConfig(max_num_seqs=8, max_num_batched_tokens=64, max_model_len=512,
                                             num_kv_blocks=128, use_graphs=graphs, graph_buckets=(1, 2, 4, 8),
                                             swa_release=release))
        outs[release] = eng.generate(prompts, SamplingParams(max_tokens=40, ignore_eos=True))
        assert all(len(o) == 40 for o in outs[release])
        if graphs:
            assert eng.stats["graph_steps"] > 0
        assert (eng.stats["kv_pages_released"] > 0) == release
        assert eng.alloc.num_free == eng.alloc.available - 1  # every page came back (page 0: the null page)
    assert outs[True] == outs[False]
    _check_greedy(swa_model, prompts, outs[True])
