"""MXFP4 weights on CPU: format, device layout, oracle, byte arithmetic, spec.weightDtype, rejections.
Scale bytes come from [2, 252], all that ``mx4_quantize`` yields from finite bf16 (e = floor(log2(amax))
+ 125); at 253 / 254 the codes for 4 and 6 are past bf16's largest value and cannot round-trip."""
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
from test_q4_cpu import _cr

E_MAX = 252


def _random(N, K, seed):
    """Random codes without negative zero, a 4 or a 6 in every group (its amax then pins e), random e."""
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, 16, (N, K), generator=g, dtype=torch.uint8)
    codes[codes == 8] = 0
    codes.view(N, K // 32, 32)[:, :, 5] = torch.randint(6, 8, (N, K // 32), generator=g, dtype=torch.uint8)
    return codes, torch.randint(2, E_MAX + 1, (N, K // 32), generator=g, dtype=torch.uint8)


def test_pack_and_quantise_round_trips():
    codes, e = _random(32, 256, 1)
    e[0, :4] = torch.tensor([2, 3, E_MAX - 1, E_MAX], dtype=torch.uint8)    # both ends of the range
    W = ops.mx4_pack(codes, e)
    assert W.qw.shape == (2, 2, 64, 4) and W.qe.shape == (2, 2, 16) and (W.N, W.K) == (32, 256)
    words, scales = (W.qw.to(torch.int64) & 0xFFFFFFFF).tolist(), (W.qe.to(torch.int64) & 0xFFFFFFFF).tolist()
    for n in range(32):                                                     # the layout, index by index
        for k in range(256):
            lane, j = (n & 15) + 16 * ((k % 32) // 8), (k % 128) // 32
            assert (words[n // 16][k // 128][lane][j] >> (4 * (k % 8))) & 15 == int(codes[n, k]), (n, k)
            assert (scales[n // 16][k // 128][n & 15] >> (8 * j)) & 255 == int(e[n, k // 32]), (n, k)
    assert all(torch.equal(a, b) for a, b in zip(ref.mx4_unpack(W.qw, W.qe), (codes, e)))
    deq = ref.mx4_dequant(codes, e)
    grid = torch.tensor(ref.MX4_GRID, dtype=torch.float64)
    exact = torch.where(codes >= 8, -1.0, 1.0) * grid[(codes & 7).long()] * 2.0 ** (e.double() - 127).repeat_interleave(32, 1)
    assert torch.equal(deq.double(), exact)                                 # nothing rounds
    assert torch.equal(ops.mx4_dequant(W), deq)
    c3, e3 = ref.mx4_quantize(deq)
    assert torch.equal(c3, codes) and torch.equal(e3, e)
    with pytest.raises(ValueError, match="K % 128"):
        ref.mx4_quantize(torch.zeros(32, 192))
    with pytest.raises(ValueError, match="N % 16"):
        ref.mx4_pack(torch.zeros(24, 128, dtype=torch.uint8), torch.zeros(24, 4, dtype=torch.uint8))


@pytest.mark.parametrize("v,want", [(.25, 0), (.75, 1), (1.25, 1), (1.75, 2), (2.5, 2), (3.5, 4), (5, 4), (7.9, 6),
                                    (.26, .5), (2.51, 3), (5.1, 6)])
@pytest.mark.parametrize("e", [2, 127, E_MAX])
def test_rounding_ties_and_saturation(v, want, e):
    """Ties go to the even code, 7.9 saturates at 6; the group's other entry (6, or 7.9) pins e."""
    s = 2.0 ** (e - 127)
    w = torch.zeros(16, 128)
    w[:, 0], w[:, 1], w[:, 2] = 6 * s, v * s, -v * s
    codes, eb = ref.mx4_quantize(w.to(torch.bfloat16))
    assert bool((eb[:, 0] == e).all()) and bool((eb[:, 1:] == 127).all())
    deq = ref.mx4_dequant(codes, eb).float()
    assert bool((deq[:, 1] == want * s).all()) and bool((deq[:, 2] == -want * s).all())
    assert bool((codes[:, 2] == (codes[:, 1] + 8 if want else 0)).all())     # no negative zero


def test_scale_clamps():
    w = torch.zeros(16, 128)
    w[:, 32] = 2.0 ** -130                                                  # a bf16 subnormal: e = 2, v = 2^-5 -> 0
    w[:, 64], w[:, 65] = 2.0 ** -126, 2.0 ** -124                           # the rule gives 1, clamped to 2: v = .5, 2
    w[:, 96] = 3.0e38                                                       # 1.76 * 2^127: e = 252, v = 7.05 -> 6
    codes, e = ref.mx4_quantize(w.to(torch.bfloat16))
    assert e[0].tolist() == [127, 2, 2, E_MAX]
    assert not codes[:, :64].any()
    assert torch.equal(ref.mx4_dequant(codes, e)[:, 64:].float(), w.to(torch.bfloat16)[:, 64:].float().clamp(max=6 * 2.0 ** 125))


def test_dense_oracle_and_cpu_engine():
    tiny = build_model(TINY_LLAMA, device="cpu", seed=3)
    toks = list(range(5, 45))
    want = dense_logits(tiny, toks, weight_dtype="mxfp4")
    assert not torch.equal(dense_logits(tiny, toks), want)
    bf16_bytes = tiny.weight_bytes()
    eng = Engine(tiny, EngineConfig(max_num_seqs=4, max_num_batched_tokens=32, max_model_len=256, num_kv_blocks=64,
                                    weight_dtype="mxfp4"))
    assert eng.stats["weight_dtype"] == "mxfp4" and tiny.weight_dtype == "mxfp4"
    assert isinstance(tiny.layers[0]["qkv"], ops.Mx4Weight) and not isinstance(tiny.layers[0]["qkv"], tuple)
    assert tiny.weight_bytes() == TINY_LLAMA.weight_bytes(weight_dtype="mxfp4") < bf16_bytes
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
    packed = sum(n * k // 2 + n * k // 32 for n, k in shapes)
    assert all(ops.mx4_bytes(n, k) == n * k // 2 + n * k // 32 for n, k in shapes)
    rest = 2 * (L * 2 * H + 2 * V * H + H)                                  # norms, embedding, LM head: bf16
    assert cfg.weight_bytes(weight_dtype="mxfp4") == L * packed + rest + 2 * 2 * I * H   # + gate_up's scratch
    assert cfg.weight_bytes(weight_dtype="int4") < cfg.weight_bytes(weight_dtype="mxfp4") < cfg.weight_bytes() / 2.6


def test_crd_field_and_placement():
    schema = crd.crd_schema()
    pruned, errs = crd.admit(_cr(weightDtype="mxfp4"), schema)
    assert errs == [] and pruned["spec"]["weightDtype"] == "mxfp4"
    assert crd.ModelSpec.from_spec(pruned["spec"]).validate() == []
    base = {"modelName": "m", "modelAlias": "a", "weightDtype": "mxfp4"}
    for extra, word in (({"tensorParallel": 2}, "tensorParallel"), ({"expertParallel": 2}, "expertParallel"),
                        ({"adapters": [{"name": "a", "uri": "s3://a"}]}, "adapters")):
        errs = crd.ModelSpec.from_spec(dict(base, **extra)).validate()
        assert any(word in e and "mxfp4" in e for e in errs), errs
    kw = dict(max_model_len=4096, max_num_seqs=256)
    m8 = placement.plan("llama3-8b", weight_dtype="mxfp4", **kw)
    assert m8.fits and m8.gpus == 1 and m8.weightGBPerGPU == round(get_config("llama3-8b").weight_bytes(weight_dtype="mxfp4") / placement.GB, 2)
    for bad in (placement.plan("llama3-70b", weight_dtype="mxfp4", requested_tp=2, **kw),
                placement.plan("mixtral-8x7b", weight_dtype="mxfp4", requested_ep=2, **kw),
                placement.plan("mixtral-8x7b", weight_dtype="mxfp4", **kw)):
        assert not bad.fits and "mxfp4" in bad.reason
    with open(crd.MANIFESTS / "examples" / "mxfp4" / "llama3-70b-mxfp4.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr, schema)
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert errs == [] and pruned == cr and spec.validate() == [] and spec.weight_dtype == "mxfp4"
    assert placement.plan(spec.architecture, max_model_len=spec.max_model_len, max_num_seqs=spec.max_num_seqs,
                          requested_tp=spec.tensor_parallel, weight_dtype=spec.weight_dtype).fits


def test_engine_rejections():
    kw = dict(max_num_seqs=4, num_kv_blocks=16)
    with pytest.raises(ValueError, match="mxfp4.*MoE"):
        Engine(build_model(TINY_MIXTRAL, device="cpu", seed=0), EngineConfig(weight_dtype="mxfp4", **kw))
    with pytest.raises(ValueError, match="mxfp4.*LoRA"):
        Engine(build_model(TINY_LLAMA, device="cpu", seed=3), EngineConfig(weight_dtype="mxfp4", max_adapters=2, **kw))
    for tp, ep, word in ((2, 1, "tensor parallel"), (1, 2, "expert parallelism")):
        m = build_model(TINY_LLAMA, device="cpu", seed=3)
        m.ps = ParallelState(tp=Group(size=tp), ep=Group(size=ep))          # what a rank of such a group reports
        with pytest.raises(ValueError, match="mxfp4.*" + word):
            Engine(m, EngineConfig(weight_dtype="mxfp4", **kw))
