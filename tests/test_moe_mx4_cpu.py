"""MXFP4 expert weights on CPU: the stacked packing, the reference route of ops.grouped_gemm_mx4, a
TINY_MIXTRAL engine against the fake-quant oracle, the rejections, byte arithmetic and placement, and
spec.expertWeightDtype down to the predictor's environment."""
import dataclasses

import pytest
import torch
import yaml

from mlopamd import ops
from mlopamd.controller import crd, placement
from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_MIXTRAL, get_config
from mlopamd.models.reference import dense_logits
from mlopamd.ops import reference as ref
from mlopamd.parallel.comm import Group, ParallelState
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams

KW = dict(max_num_seqs=4, max_num_batched_tokens=32, max_model_len=256, num_kv_blocks=64)


def _experts(E, N, K, seed, lo=2, hi=252):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (E, N, K), generator=g, dtype=torch.uint8)
    return codes, torch.randint(lo, hi + 1, (E, N, K // 32), generator=g, dtype=torch.uint8)


def test_stacked_packing_round_trips():
    E, N, K = 3, 32, 256
    codes, e = _experts(E, N, K, 1)
    W = ops.mx4_experts_pack(codes, e)
    assert W.qw.shape == (E, 2, 2, 64, 4) and W.qe.shape == (E, 2, 2, 16) and (W.E, W.N, W.K) == (E, N, K)
    assert all(torch.equal(a, b) for a, b in zip(ops.mx4_experts_unpack(W), (codes, e)))
    S = ops.mx4_pack(codes.view(E * N, K), e.view(E * N, -1))               # the [E N, K] matrix, packed
    assert torch.equal(W.qw.view(S.qw.shape), S.qw) and torch.equal(W.qe.view(S.qe.shape), S.qe)
    deq = ref.mx4_dequant(codes.view(E * N, K), e.view(E * N, -1)).view(E, N, K)
    assert torch.equal(ops.mx4_experts_dequant(W), deq)
    Q = ops.mx4_experts_quantize_pack(deq)                                  # each expert through ref.mx4_quantize
    assert all(torch.equal(Q.qw[i], ops.mx4_quantize_pack(deq[i]).qw) for i in range(E))
    with pytest.raises(ValueError, match="K % 128"):
        ops.mx4_experts_quantize_pack(torch.zeros(2, 32, 192, dtype=torch.bfloat16))


@pytest.mark.parametrize("epi", [ops.EPI_NONE, ops.EPI_SILU_MUL])
@pytest.mark.parametrize("mapped", [False, True])
def test_cpu_route_is_per_expert_gemm_mx4(epi, mapped):
    E, N, K, R, off = 4, 64, 128, 12, [0, 0, 5, 6, 9]
    codes, e = _experts(E, N, K, 2, 120, 130)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(R, K, generator=g).to(torch.bfloat16)
    a_rows = torch.randperm(R, generator=g).to(torch.int32) if mapped else None
    out = ops.grouped_gemm_mx4(x, ops.mx4_experts_pack(codes, e), torch.tensor(off, dtype=torch.int32), epi=epi, a_rows=a_rows)
    rows = x if a_rows is None else x[a_rows.long()]
    want = torch.cat([ref.gemm_mx4(rows[off[i]:off[i + 1]], codes[i], e[i], torch.float32) for i in range(E)]).to(torch.bfloat16)
    assert torch.equal(out[:off[-1]], ref.silu_mul(ops.deinterleave_cols(want)) if epi else want)


def test_cpu_engine_follows_the_fake_quant_oracle():
    tiny = build_model(TINY_MIXTRAL, device="cpu", seed=3)
    toks = list(range(5, 45))
    want = dense_logits(tiny, toks, expert_weight_dtype="mxfp4")
    assert not torch.equal(dense_logits(tiny, toks), want)
    bf16_bytes = tiny.weight_bytes()
    eng = Engine(tiny, EngineConfig(expert_weight_dtype="mxfp4", **KW))
    L = tiny.layers[0]
    assert eng.stats["expert_weight_dtype"] == "mxfp4" and "weight_dtype" not in eng.stats
    assert isinstance(L["w13"], ops.Mx4Experts) and isinstance(L["w2"], ops.Mx4Experts)
    assert all(isinstance(L[k], torch.Tensor) for k in ("qkv", "o", "router"))
    assert tiny.weight_bytes() == TINY_MIXTRAL.weight_bytes(expert_weight_dtype="mxfp4") < bf16_bytes
    assert torch.equal(dense_logits(tiny, toks), want)                      # the packed model is its own oracle
    (out,) = eng.generate([toks], SamplingParams(max_tokens=8, ignore_eos=True))
    for t in out:                                                           # the near-tie rule of the engine tests
        lg = dense_logits(tiny, toks)[-1]
        assert t == int(lg.argmax()) or float(lg.max() - lg[t]) < 0.05 * float(lg.std())
        toks.append(t)


def test_rejections_name_the_field():
    def mixtral(tp=1, ep=1, **cfg):
        m = build_model(dataclasses.replace(TINY_MIXTRAL, **cfg), device="cpu", seed=0)
        if tp > 1 or ep > 1:
            m.ps = ParallelState(tp=Group(size=tp), ep=Group(size=ep))      # what a rank of such a group reports
        return m

    for model, extra, word in ((build_model(TINY_LLAMA, device="cpu", seed=0), {}, "MoE"),
                               (mixtral(tp=2), {}, "tensor parallel"), (mixtral(ep=2), {}, "expert parallel"),
                               (mixtral(intermediate_size=192), {}, "intermediate_size"),
                               (mixtral(), {"weight_dtype": "mxfp4"}, "weight_dtype"),
                               (mixtral(), {"expert_weight_dtype": "int4"}, "must be one of")):
        with pytest.raises(ValueError, match="expert_weight_dtype.*" + word):
            Engine(model, EngineConfig(**{"expert_weight_dtype": "mxfp4", **extra, **KW}))


def test_bytes_and_placement():
    cfg = get_config("mixtral-8x7b")
    H, I, L, E = cfg.hidden_size, cfg.intermediate_size, cfg.num_layers, cfg.num_experts
    experts = 3 * H * I * E
    want = L * (experts // 2 + experts // 32) + 2 * (cfg.num_params() - L * experts) + 2 * 2 * I * H * E  # + w13's scratch
    assert cfg.weight_bytes(expert_weight_dtype="mxfp4") == want < cfg.weight_bytes() / 2.6
    kw = dict(max_model_len=4096, max_num_seqs=256)
    p = placement.plan("mixtral-8x7b", expert_weight_dtype="mxfp4", **kw)
    assert p.fits and p.gpus == 1 and p.weightGBPerGPU == round(want / placement.GB, 2)
    for bad in (placement.plan("mixtral-8x7b", expert_weight_dtype="mxfp4", requested_tp=2, **kw),
                placement.plan("mixtral-8x7b", expert_weight_dtype="mxfp4", requested_ep=2, **kw),
                placement.plan("llama3-8b", expert_weight_dtype="mxfp4", **kw)):
        assert not bad.fits and "expertWeightDtype" in bad.reason
    assert not placement.plan("mixtral-8x7b", weight_dtype="mxfp4", **kw).fits


def test_example_cr_reaches_the_predictor_env():
    from test_controller import Env, _ready, run

    with open(crd.MANIFESTS / "examples" / "mxfp4" / "qwen3-30b-a3b-mxfp4.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr, crd.crd_schema())
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert errs == [] and pruned == cr and spec.validate() == [] and spec.expert_weight_dtype == "mxfp4"
    for extra, word in (({"tensorParallel": 2}, "tensorParallel"), ({"weightDtype": "int4"}, "weightDtype")):
        errs = crd.ModelSpec.from_spec({**cr["spec"], **extra}).validate()
        assert any(word in e and "expertWeightDtype" in e for e in errs), errs
    assert placement.plan(spec.architecture, max_model_len=spec.max_model_len, max_num_seqs=spec.max_num_seqs,
                          requested_tp=spec.tensor_parallel, expert_weight_dtype="mxfp4").fits

    async def go():
        env = Env()
        env.reg.set_alias("m", "champion", env.version(tags={"mlop.architecture": spec.architecture}))
        await env.start()
        await env.create_cr(tensorParallel=1, maxModelLen=spec.max_model_len, maxNumSeqs=spec.max_num_seqs,
                            expertWeightDtype="mxfp4")
        assert await env.run_until(lambda: _ready(env))
        (p,) = (await env.sd())["spec"]["predictors"]
        e = {x["name"]: x["value"] for x in p["componentSpecs"][0]["spec"]["containers"][0]["env"]}
        assert e["MLOP_ENGINE_EXPERT_WEIGHT_DTYPE"] == "mxfp4" and "MLOP_ENGINE_WEIGHT_DTYPE" not in e
        await env.stop()
    run(go())
