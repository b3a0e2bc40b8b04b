"""Int4 weights on CPU: the format and device layout (ops/reference.py), the fake-quant oracle,
the weight-byte arithmetic, the control plane's spec.weightDtype and the engine's rejections."""
import pytest
import torch
import yaml

from mlopamd import ops
from mlopamd.controller import crd, placement
from mlopamd.models import build_model
from mlopamd.models.config import TINY_LLAMA, TINY_MIXTRAL, get_config
from mlopamd.models.reference import dense_logits
from mlopamd.ops import reference as ref
from mlopamd.runtime.engine import Engine, EngineConfig
from mlopamd.runtime.sampler import SamplingParams


def test_quantise_pack_round_trip():
    """Every nibble and scale where the layout says (N = 32, K = 256, index by index), the round
    trip, and |w - dequant| <= s / 2 wherever the clamp to 7 / -8 does not bind."""
    g = torch.Generator().manual_seed(1)
    w = torch.randn(32, 256, generator=g).to(torch.bfloat16)
    w[3, 128:] = 0                                                          # an all-zero group
    q, s = ref.q4_quantize(w)
    assert q.dtype == torch.int8 and int(q.min()) >= -8 and int(q.max()) <= 7 and s.dtype == torch.bfloat16
    assert torch.equal(s, (w.float().view(32, 2, 128).abs().amax(-1) / 7).to(torch.bfloat16))
    assert float(s[3, 1]) == 0 and not q[3, 128:].any()
    qw, qs, N, K = ops.q4_pack(q, s)
    assert qw.shape == (2, 2, 64, 4) and qs.shape == (2, 2, 16) and (N, K) == (32, 256)
    words = (qw.to(torch.int64) & 0xFFFFFFFF).tolist()
    for n in range(32):
        for k in range(256):
            lane, j, e = (n & 15) + 16 * ((k % 32) // 8), (k % 128) // 32, k % 8
            u = (words[n // 16][k // 128][lane][j] >> (4 * ((e >> 1) + 4 * (e & 1)))) & 15
            assert u == int(q[n, k]) + 8, (n, k)
        assert torch.equal(qs[n // 16, :, n & 15], s[n])
    q2, s2 = ref.q4_unpack(qw, qs)
    assert torch.equal(q2, q) and torch.equal(s2, s)
    deq = ref.q4_dequant(q, s)
    assert torch.equal(ops.q4_dequant((qw, qs, N, K)), deq)
    sf = s.float().repeat_interleave(128, 1)
    free = (w.float() / sf.clamp_min(1e-30)).abs() <= 7.5                   # the clamp does not bind
    # s / 2 holds for the unrounded product float(s) * q (2^-20: the fp32 division w / s); the bf16
    # dequantised value is that product rounded once, half an ulp (2^-8 relative) further at most
    exact = sf * q.float()
    assert bool(((w.float() - exact).abs() <= sf / 2 * (1 + 2.0 ** -20))[free].all())
    assert bool(((deq.float() - exact).abs() <= exact.abs() * 2.0 ** -8).all())
    x = torch.randn(5, 256, generator=g).to(torch.bfloat16)
    torch.testing.assert_close(ops.gemm_q4(x, (qw, qs, N, K)).float(), ref.gemm_q4(x, q, s).float(), rtol=2 ** -7, atol=0.05)
    with pytest.raises(ValueError, match="K % 128"):
        ref.q4_quantize(torch.zeros(32, 192))
    with pytest.raises(ValueError, match="N % 16"):
        ref.q4_pack(torch.zeros(24, 128, dtype=torch.int8), torch.zeros(24, 1, dtype=torch.bfloat16))


def test_dense_oracle_and_cpu_engine():
    tiny = build_model(TINY_LLAMA, device="cpu", seed=3)
    toks = list(range(5, 45))
    a = dense_logits(tiny, toks)
    assert torch.equal(a, dense_logits(tiny, toks, weight_dtype="bf16"))
    want = dense_logits(tiny, toks, weight_dtype="int4")
    assert not torch.equal(a, want)
    with pytest.raises(ValueError, match="weight_dtype"):
        dense_logits(tiny, toks, weight_dtype="fp8")
    bf16_bytes = tiny.weight_bytes()
    eng = Engine(tiny, EngineConfig(max_num_seqs=4, max_num_batched_tokens=32, max_model_len=256, num_kv_blocks=64,
                                    weight_dtype="int4"))
    assert eng.stats["weight_dtype"] == "int4" and tiny.weight_dtype == "int4"
    assert tiny.weight_bytes() == TINY_LLAMA.weight_bytes(weight_dtype="int4") < bf16_bytes
    assert torch.equal(dense_logits(tiny, toks), want)                      # the packed model is its own oracle
    (out,) = eng.generate([toks], SamplingParams(max_tokens=8, ignore_eos=True))
    seq = list(toks)
    for t in out:                                                           # the near-tie rule of the engine tests
        lg = dense_logits(tiny, seq)[-1]
        assert t == int(lg.argmax()) or float(lg.max() - lg[t]) < 0.05 * float(lg.std())
        seq.append(t)


@pytest.mark.parametrize("name", ["llama3-8b", "llama3-70b"])
def test_weight_bytes_arithmetic(name):
    cfg = get_config(name)
    H, I, L, V = cfg.hidden_size, cfg.intermediate_size, cfg.num_layers, cfg.vocab_size
    shapes = [((cfg.num_heads + 2 * cfg.num_kv_heads) * 128, H), (H, cfg.num_heads * 128), (2 * I, H), (H, I)]
    assert list(cfg.projection_shapes()) == shapes
    packed = sum(n * k // 2 + n * k // 64 for n, k in shapes)
    assert all(ops.q4_bytes(n, k) == n * k // 2 + n * k // 64 for n, k in shapes)
    rest = 2 * (L * 2 * H + 2 * V * H + H)                                  # norms, embedding, LM head: bf16
    scratch = 2 * 2 * I * H                                                 # gate_up, the largest projection
    assert cfg.weight_bytes(weight_dtype="int4") == L * packed + rest + scratch
    assert cfg.weight_bytes(weight_dtype="bf16") == cfg.weight_bytes() == 2 * cfg.num_params()
    assert cfg.weight_bytes() / cfg.weight_bytes(weight_dtype="int4") > 2.7


def _cr(**spec):
    return {"apiVersion": "mlflow.nizepart.com/v1alpha1", "kind": "MlflowModel", "metadata": {"name": "x"},
            "spec": dict({"modelName": "m", "modelAlias": "a"}, **spec)}


def test_crd_field_and_placement():
    schema = crd.crd_schema()
    assert crd.ModelSpec.from_spec(_cr()["spec"]).weight_dtype is None
    for dt in crd.WEIGHT_DTYPES:
        pruned, errs = crd.admit(_cr(weightDtype=dt), schema)
        assert errs == [] and pruned["spec"]["weightDtype"] == dt
        spec = crd.ModelSpec.from_spec(pruned["spec"])
        assert spec.weight_dtype == dt and spec.validate() == []
    _, errs = crd.admit(_cr(weightDtype="fp8"), schema)
    assert any("weightDtype" in e for e in errs)
    base = {"modelName": "m", "modelAlias": "a", "weightDtype": "int4"}
    for extra, word in (({"tensorParallel": 2}, "tensorParallel"), ({"expertParallel": 2}, "expertParallel"),
                        ({"adapters": [{"name": "a", "uri": "s3://a"}]}, "adapters")):
        assert any(word in e for e in crd.ModelSpec.from_spec(dict(base, **extra)).validate())
    # placement charges the smaller weights: more KV tokens, and a 70B that needs one GPU, not two
    kw = dict(max_model_len=4096, max_num_seqs=256)
    b8, q8 = placement.plan("llama3-8b", **kw), placement.plan("llama3-8b", weight_dtype="int4", **kw)
    assert q8.fits and q8.gpus == 1 and q8.weightGBPerGPU < b8.weightGBPerGPU and q8.kvTokenCapacity > b8.kvTokenCapacity
    assert placement.plan("llama3-8b", weight_dtype="bf16", **kw) == b8
    big = dict(max_model_len=4096, max_num_seqs=256)
    assert placement.plan("llama3-70b", **big).gpus > 1
    q70 = placement.plan("llama3-70b", weight_dtype="int4", **big)
    assert q70.fits and q70.gpus == 1
    assert not placement.plan("llama3-70b", weight_dtype="int4", requested_tp=2, **big).fits
    assert not placement.plan("mixtral-8x7b", weight_dtype="int4", **kw).fits
    with open(crd.MANIFESTS / "examples" / "int4" / "llama3-70b-int4.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr, schema)
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert errs == [] and pruned == cr and spec.validate() == [] and spec.weight_dtype == "int4"
    assert placement.plan(spec.architecture, max_model_len=spec.max_model_len, max_num_seqs=spec.max_num_seqs,
                          requested_tp=spec.tensor_parallel, weight_dtype=spec.weight_dtype).fits


def test_engine_rejections():
    kw = dict(max_num_seqs=4, num_kv_blocks=16)
    with pytest.raises(ValueError, match="weight_dtype"):
        Engine(build_model(TINY_LLAMA, device="cpu", seed=3), EngineConfig(weight_dtype="fp8", **kw))
    with pytest.raises(ValueError, match="MoE"):
        Engine(build_model(TINY_MIXTRAL, device="cpu", seed=0), EngineConfig(weight_dtype="int4", **kw))
    with pytest.raises(ValueError, match="LoRA"):
        Engine(build_model(TINY_LLAMA, device="cpu", seed=3), EngineConfig(weight_dtype="int4", max_adapters=2, **kw))
