"""Qwen3 (dense) checkpoints off the GPU: the loader and the dense oracle against transformers'
Qwen3ForCausalLM (with negative controls for each way the per-head QK-norm can go wrong), the
config rules, the reference contract of ``ref.rope_cache`` with norm weights, the engine at TP = 2
over gloo, and the GEMM planner's routes of the Qwen3 projections, pinned in a fixture of their own.
"""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "tests")) if p not in sys.path]  # (python tests/... --write)

from mlopamd.models import build_model, loader  # noqa: E402
from mlopamd.models.config import CHECKPOINT_SHAPES, PRESETS, TINY_LLAMA, get_config  # noqa: E402
from mlopamd.models.reference import dense_logits  # noqa: E402
from mlopamd.ops import reference as ref  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

# ------------------------------------------------------------------ HF parity --


@pytest.fixture(scope="module")
def tiny_qwen3(tmp_path_factory):
    """(checkpoint dir, transformers model, our model, tokens, HF logits): built once, read-only."""
    transformers = pytest.importorskip("transformers")
    d = tmp_path_factory.mktemp("qwen3")
    cfg = transformers.Qwen3Config(vocab_size=512, hidden_size=256, intermediate_size=512, num_hidden_layers=2,
                                   num_attention_heads=4, num_key_value_heads=1, head_dim=128,
                                   max_position_embeddings=512, rms_norm_eps=1e-6,
                                   rope_parameters={"rope_theta": 1e6, "rope_type": "default"})
    torch.manual_seed(0)
    m = transformers.Qwen3ForCausalLM(cfg).eval()
    with torch.no_grad():  # non-trivial norm weights, q / k norms included: a swapped or dropped norm shows
        for n, p in m.named_parameters():
            if n.endswith("norm.weight"):
                p.copy_(1 + 0.2 * torch.randn_like(p))
    m.save_pretrained(d)
    ours = loader.load_pretrained(d, device="cpu", dtype=torch.float32)
    toks = torch.randint(3, 500, (37,), generator=torch.Generator().manual_seed(5)).tolist()
    with torch.no_grad():
        exp = m(torch.tensor([toks])).logits[0].float()
    return d, m, ours, toks, exp


def _hf_greedy(m, prompt, n):
    out = m.generate(torch.tensor([prompt]), max_new_tokens=n, do_sample=False, min_new_tokens=n,
                     pad_token_id=0, eos_token_id=None)
    return out[0, len(prompt):].tolist()


def test_hf_qwen3_parity(tiny_qwen3):
    d, hf, ours, toks, exp = tiny_qwen3
    cfg = loader.config_from_hf(json.loads((d / "config.json").read_text()))
    assert cfg.qk_norm and cfg.rope_theta == 1e6 and cfg.rms_eps == 1e-6 and not cfg.is_moe
    assert cfg.sliding_window == 0 and cfg.head_dim == 128
    assert ours.cfg.qk_norm and all("q_norm" in L and "k_norm" in L for L in ours.layers)
    # fold_norms (load_pretrained's default) left the per-head weights alone
    assert all(not bool((L["q_norm"] == 1).all()) and not bool((L["k_norm"] == 1).all()) for L in ours.layers)
    got = dense_logits(ours, toks)
    print("max |dense_logits - HF| =", float((got - exp).abs().max()))
    torch.testing.assert_close(got, exp, atol=2e-4, rtol=1e-3)


def test_hf_qwen3_engine_greedy(tiny_qwen3):
    """Eager CPU engine, 16-token chunks (prefill chunks and decode rows share steps): transformers'
    greedy continuation."""
    _, hf, ours, toks, _ = tiny_qwen3
    eng = Engine(ours, EngineConfig(max_num_seqs=4, max_num_batched_tokens=16, max_model_len=256,
                                    num_kv_blocks=64, use_graphs=False))
    prompts = [toks, toks[:9]]
    outs = eng.generate(prompts, SamplingParams(max_tokens=6, ignore_eos=True))
    for p, o in zip(prompts, outs):
        assert o == _hf_greedy(hf, p, 6)


def _logits_variant(model, tokens, how):
    """dense_logits' computation with the QK-norm done wrongly in one way (fp32, one sequence):
    "swap": q_norm and k_norm exchanged; "after": the norm applied after the rotation; "none": no norm;
    "right": the right thing (checks this re-implementation itself)."""
    cfg = model.cfg
    T, D, half = len(tokens), cfg.head_dim, cfg.head_dim // 2
    res = model.embed[torch.tensor(tokens)].float()
    x = ref.rmsnorm(res, model.layers[0]["in_norm"].float(), cfg.rms_eps)
    cs = model.cos_sin[torch.arange(T)]
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    mask = torch.triu(torch.ones(T, T, dtype=torch.bool), 1)
    G = model.n_q // model.n_kv
    from mlopamd.models.reference import _mlp

    for i, L in enumerate(model.layers):
        qkv = F.linear(x, L["qkv"].float())
        q = qkv[:, : model.n_q * D].view(T, model.n_q, D)
        k = qkv[:, model.n_q * D:(model.n_q + model.n_kv) * D].view(T, model.n_kv, D)
        v = qkv[:, (model.n_q + model.n_kv) * D:].view(T, model.n_kv, D)
        qw, kw = (L["k_norm"], L["q_norm"]) if how == "swap" else (L["q_norm"], L["k_norm"])
        if how in ("right", "swap"):
            q, k = ref.head_rmsnorm(q, qw, cfg.rms_eps), ref.head_rmsnorm(k, kw, cfg.rms_eps)
        q, k = ref.rotate(q, cos, sin), ref.rotate(k, cos, sin)
        if how == "after":
            q, k = ref.head_rmsnorm(q, qw, cfg.rms_eps), ref.head_rmsnorm(k, kw, cfg.rms_eps)
        s = torch.einsum("qhd,khd->hqk", q, k.repeat_interleave(G, 1)) / D ** 0.5
        s = s.masked_fill(mask[None], float("-inf"))
        a = torch.einsum("hqk,khd->qhd", s.softmax(-1), v.repeat_interleave(G, 1)).reshape(T, -1)
        res = res + F.linear(a, L["o"].float())
        x = ref.rmsnorm(res, L["post_norm"].float(), cfg.rms_eps)
        res = res + _mlp(model, i, x)
        nxt = model.layers[i + 1]["in_norm"] if i + 1 < len(model.layers) else model.final_norm
        x = ref.rmsnorm(res, nxt.float(), cfg.rms_eps)
    return F.linear(x, model.lm_head.float())


def test_negative_controls_show_each_mistake(tiny_qwen3):
    _, _, ours, toks, exp = tiny_qwen3
    with torch.no_grad():
        torch.testing.assert_close(_logits_variant(ours, toks, "right"), exp, atol=2e-4, rtol=1e-3)
        for how in ("swap", "after", "none"):
            diff = float((_logits_variant(ours, toks, how) - exp).abs().max())
            print(f"QK-norm '{how}': max |logits - HF| = {diff:.4f}")
            assert diff > 1e-2, how


# --------------------------------------------------------------------- config --

# the fields of Qwen/Qwen3-8B's public config.json
QWEN3_8B_JSON = {
    "architectures": ["Qwen3ForCausalLM"], "attention_bias": False, "attention_dropout": 0.0, "bos_token_id": 151643,
    "eos_token_id": 151645, "head_dim": 128, "hidden_act": "silu", "hidden_size": 4096, "initializer_range": 0.02,
    "intermediate_size": 12288, "max_position_embeddings": 40960, "max_window_layers": 36, "model_type": "qwen3",
    "num_attention_heads": 32, "num_hidden_layers": 36, "num_key_value_heads": 8, "rms_norm_eps": 1e-06,
    "rope_scaling": None, "rope_theta": 1000000, "sliding_window": None, "tie_word_embeddings": False,
    "torch_dtype": "bfloat16", "use_cache": True, "use_sliding_window": False, "vocab_size": 151936,
}


def test_qwen3_8b_config_and_presets():
    cfg = loader.config_from_hf(QWEN3_8B_JSON, name="qwen3-8b")
    assert cfg == CHECKPOINT_SHAPES["qwen3-8b"] == get_config("Qwen/Qwen3-8B")
    assert cfg.qk_norm and cfg.sliding_window == 0 and cfg.max_position == 40960 and cfg.eos_token_id == 151645
    assert loader.known_preset(loader.config_from_hf(QWEN3_8B_JSON)) == "qwen3-8b"
    # the transformers >= 5 spelling of the same config
    d5 = dict(QWEN3_8B_JSON, layer_types=["full_attention"] * 36,
              rope_parameters={"rope_theta": 1000000, "rope_type": "default"})
    del d5["rope_theta"], d5["rope_scaling"]
    assert loader.config_from_hf(d5, name="qwen3-8b") == cfg
    big = get_config("Qwen/Qwen3-32B")
    assert (big.hidden_size, big.intermediate_size, big.num_layers, big.num_heads, big.num_kv_heads) == \
        (5120, 25600, 64, 64, 8) and big.qk_norm and big.vocab_size == 151936
    assert loader.known_preset(big) == "qwen3-32b"
    # qk_norm is part of the function: the same shapes without it are another model
    import dataclasses

    assert dataclasses.replace(cfg, qk_norm=False) != cfg
    assert cfg.num_params() - dataclasses.replace(cfg, qk_norm=False).num_params() == 36 * 2 * 128
    tiny = get_config("tiny-qwen3")
    assert tiny == dataclasses.replace(TINY_LLAMA, name="tiny-qwen3", qk_norm=True, rms_eps=1e-6, rope_theta=1e6)
    # the real-size shapes live outside PRESETS: tests/test_gemm_plan_cpu.py derives the planner's
    # pinned route table from every non-tiny PRESETS entry, and that table must not change
    assert [n for n, c in PRESETS.items() if c.qk_norm and not n.startswith("tiny")] == []
    assert not any("qwen" in n.lower() and not n.startswith("tiny") for n in PRESETS)


def test_rejected_configs():
    with pytest.raises(ValueError, match=r"GQA group 40/8 = 5\b"):  # Qwen3-14B
        loader.config_from_hf(dict(QWEN3_8B_JSON, hidden_size=5120, num_attention_heads=40, intermediate_size=17408))
    with pytest.raises(ValueError, match="Qwen3-MoE"):
        loader.config_from_hf(dict(QWEN3_8B_JSON, architectures=["Qwen3MoeForCausalLM"], num_experts=128))
    yarn = {"rope_type": "yarn", "factor": 4.0, "original_max_position_embeddings": 32768}
    with pytest.raises(ValueError, match="rope_scaling type 'yarn'"):
        loader.config_from_hf(dict(QWEN3_8B_JSON, rope_scaling=yarn))
    with pytest.raises(ValueError, match="attention_bias"):
        loader.config_from_hf(dict(QWEN3_8B_JSON, attention_bias=True))
    with pytest.raises(ValueError, match="layer_types"):
        loader.config_from_hf(dict(QWEN3_8B_JSON, use_sliding_window=True, sliding_window=4096,
                                   layer_types=["full_attention"] * 18 + ["sliding_attention"] * 18))
    # the group rule is Qwen3's alone: a Llama config with a group of 5 loads as it did
    llama = dict(QWEN3_8B_JSON, architectures=["LlamaForCausalLM"], num_attention_heads=40, hidden_size=5120)
    assert loader.config_from_hf(llama).num_heads == 40


def test_checkpoint_without_q_norm_is_a_key_error(tiny_qwen3, tmp_path):
    from safetensors.torch import load_file, save_file

    d = tiny_qwen3[0]
    (tmp_path / "config.json").write_text((d / "config.json").read_text())
    for f in d.glob("*.safetensors"):
        save_file({k: v for k, v in load_file(f).items() if "q_norm" not in k}, tmp_path / f.name)
    with pytest.raises(KeyError, match=r"self_attn\.q_norm\.weight"):
        loader.load_pretrained(tmp_path, device="cpu", dtype=torch.float32)
    # the same tensors under a Llama config: loaded as a Llama model, q / k norms ignored
    c = json.loads((d / "config.json").read_text())
    c["architectures"] = ["LlamaForCausalLM"]
    (tmp_path / "config.json").write_text(json.dumps(c))
    m = loader.load_pretrained(tmp_path, device="cpu", dtype=torch.float32)
    assert not m.cfg.qk_norm and "k_norm" not in m.layers[0]


def test_example_cr_admits_and_places():
    from mlopamd.controller import crd, placement

    with open(crd.MANIFESTS / "examples" / "qwen3" / "qwen3-8b.yaml") as fh:
        (cr,) = [d for d in yaml.safe_load_all(fh) if d]
    pruned, errs = crd.admit(cr)
    assert errs == [] and pruned == cr
    spec = crd.ModelSpec.from_spec(cr["spec"])
    assert spec.validate() == [] and spec.architecture == "qwen3-8b"
    p = placement.plan(spec.architecture, max_model_len=spec.max_model_len, max_num_seqs=spec.max_num_seqs,
                       requested_tp=spec.tensor_parallel)
    assert p.fits and p.gpus == 1


# --------------------------------------------------------- reference contract --

def _rope_inputs(T=9, Hq=4, Hkv=2, D=128, NB=6, BS=16, seed=0):
    g = torch.Generator().manual_seed(seed)
    qkv = (torch.randn(T, (Hq + 2 * Hkv) * D + 64, generator=g) *
           torch.exp2(torch.randint(-6, 6, (T, 1), generator=g).float())).bfloat16()
    qkv[1, :D] = 0                                   # an all-zero head
    qkv[2, D:2 * D] = (1e-4 * torch.randn(D, generator=g)).bfloat16()   # eps dominates
    qkv[3, Hq * D:(Hq + 1) * D] = 0
    qkv[3, Hq * D + 77] = 50.0                       # one large element
    pos = torch.randint(0, 512, (T,), generator=g, dtype=torch.int32)
    pos[0], pos[1], pos[2] = 0, 1, 511
    slots = torch.randperm(NB * BS, generator=g)[:T].to(torch.int32)
    slots[4] = -1
    cs = build_model(TINY_LLAMA, device="cpu", dtype=torch.float32).cos_sin[:512].contiguous()
    qw = (1 + 0.3 * torch.randn(D, generator=g)).bfloat16()
    kw = (0.5 + 0.3 * torch.randn(D, generator=g)).bfloat16()
    return qkv, pos, cs, slots, qw, kw


def _expect64(qkv, pos, cs, qw, kw, eps, Hq, Hkv, D=128):
    """The contract in fp64, rounded once to bf16: (q [T, Hq, D], k [T, Hkv, D])."""
    T = qkv.shape[0]
    x = qkv[:, : (Hq + Hkv) * D].double().view(T, Hq + Hkv, D)
    w = torch.cat([qw.double().expand(Hq, D), kw.double().expand(Hkv, D)])[None]
    y = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    c = cs[pos.long()].double()
    out = ref.rotate(y, c[:, None, : D // 2], c[:, None, D // 2:]).bfloat16()
    return out[:, :Hq], out[:, Hq:]


def _ulps(a, b):
    """Distance in bf16 steps between two bf16 tensors (sign-magnitude -> ordered integers)."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a) - key(b)).abs()


def test_reference_contract_within_one_ulp_of_fp64():
    Hq, Hkv, D, eps = 4, 2, 128, 1e-6
    qkv, pos, cs, slots, qw, kw = _rope_inputs(Hq=Hq, Hkv=Hkv)
    kc = torch.full((6, Hkv, 16, D), 7.0, dtype=torch.bfloat16)
    vc = kc.clone()
    q = ref.rope_cache(qkv, pos, cs, slots, kc, vc, Hq, q_norm=qw, k_norm=kw, eps=eps)
    eq, ek = _expect64(qkv, pos, cs, qw, kw, eps, Hq, Hkv)
    # ~140 fp32 operations (127 adds of the mean, rsqrt, 2 products, the rotation's 3) move a value
    # by far less than half a bf16 step (2^-9 relative), so at most to the neighbouring bf16
    assert int(_ulps(q, eq).max()) <= 1
    assert bool((q[1, 0] == 0).all())                 # the zero head stays exactly zero
    seen = torch.zeros(6 * 16, dtype=torch.bool)
    for t in range(qkv.shape[0]):
        s = int(slots[t])
        if s < 0:
            continue
        seen[s] = True
        assert int(_ulps(kc[s // 16, :, s % 16], ek[t]).max()) <= 1
        assert torch.equal(vc[s // 16, :, s % 16], qkv[t, (Hq + Hkv) * D:(Hq + 2 * Hkv) * D].view(Hkv, D))
    # padding rows and unwritten slots keep the sentinel; the padding row still has its q
    kflat, vflat = kc.permute(0, 2, 1, 3).reshape(96, -1), vc.permute(0, 2, 1, 3).reshape(96, -1)
    assert bool((kflat[~seen] == 7).all()) and bool((vflat[~seen] == 7).all()) and int(seen.sum()) == 8
    assert int(_ulps(q[4], eq[4]).max()) <= 1 and bool(q[4].abs().sum() > 0)
    # the norm is not a no-op here, and without weights the function is the one it was
    plain = ref.rope_cache(qkv, pos, cs, slots, kc.clone(), vc.clone(), Hq)
    assert not torch.equal(plain, q)
    with pytest.raises(ValueError, match="both q_norm and k_norm"):
        ref.rope_cache(qkv, pos, cs, slots, kc, vc, Hq, q_norm=qw)
    from mlopamd import ops

    with pytest.raises(ValueError, match="both q_norm and k_norm"):
        ops.rope_cache(qkv, pos, cs, slots, kc, vc, Hq, k_norm=kw)
    k2, v2 = torch.zeros_like(kc), torch.zeros_like(vc)
    assert torch.equal(ops.rope_cache(qkv, pos, cs, slots, k2, v2, Hq, q_norm=qw, k_norm=kw, eps=eps), q)


def test_reference_fp8_quantises_the_bf16_rows():
    Hq, Hkv, D, eps = 4, 2, 128, 1e-6
    qkv, pos, cs, slots, qw, kw = _rope_inputs(Hq=Hq, Hkv=Hkv)
    kb = torch.zeros(6, Hkv, 16, D, dtype=torch.bfloat16)
    vb = torch.zeros_like(kb)
    qb = ref.rope_cache(qkv, pos, cs, slots, kb, vb, Hq, q_norm=qw, k_norm=kw, eps=eps)
    k8 = torch.zeros(6, Hkv, 16, D, dtype=ref.FP8)
    v8 = torch.zeros_like(k8)
    ks = torch.full((6, Hkv, 16), 3, dtype=torch.uint8)
    vs = ks.clone()
    q8 = ref.rope_cache(qkv, pos, cs, slots, k8, v8, Hq, ks, vs, q_norm=qw, k_norm=kw, eps=eps)
    assert torch.equal(q8, qb)
    live = torch.zeros(6, 16, dtype=torch.bool)
    for s in slots.tolist():
        if s >= 0:
            live[s // 16, s % 16] = True
    live = live[:, None, :].expand(6, Hkv, 16)
    for pages, scales, rows in ((k8, ks, kb), (v8, vs, vb)):
        e8, es = ref.fp8_quantize_rows(rows)
        assert torch.equal(pages.view(torch.uint8)[live], e8.view(torch.uint8)[live])
        assert torch.equal(scales[live], es[live])
        assert bool((scales[~live] == 3).all()) and bool((pages.view(torch.uint8)[~live] == 0).all())


# ------------------------------------------------------------------------- TP --

def tp_qwen3(rank, world):
    from test_parallel_cpu import _tp_engine

    return _tp_engine("tiny-qwen3", world)


def test_tp2_engine_matches_tp1():
    """tiny-qwen3 at TP = 2 over gloo == TP = 1 on the same weights (test_tp_engine_matches_tp1's
    method; the per-head norm weights are replicated, the heads sharded)."""
    import torch.multiprocessing as mp
    import tempfile

    import test_parallel_cpu as tpc

    d = tempfile.mkdtemp()
    mp.start_processes(_tp_entry, args=(2, tpc._free_port(), d), nprocs=2, join=True, start_method="spawn")
    r0, r1 = (torch.load(os.path.join(d, f"r{r}.pt"), weights_only=False) for r in range(2))
    assert r0["tp"] == r0["ref"] and r0["mixed"] == r0["ref_mixed"]
    assert r0["stats"]["tp_sync_calls"] > 0 and r1["worker_steps"] > 0


def _tp_entry(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank),
                      WORLD_SIZE=str(world))
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # norm weights away from 1, or the QK-norm would be a plain normalisation on every rank
        import mlopamd.models.llama as llama_mod

        init = llama_mod.init_norm

        calls = []

        def noisy(n, device, dtype):
            calls.append(n)
            g = torch.Generator().manual_seed(len(calls))
            return (init(n, device, dtype).float() + 0.2 * torch.randn(n, generator=g)).to(device, dtype)

        llama_mod.init_norm = noisy
        torch.save(tp_qwen3(rank, world), os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


# -------------------------------------------------------------------- planner --

FIXTURE = os.path.join(ROOT, "tests", "fixtures", "gemm_routes_qwen3_gfx950.txt")


def qwen3_shapes():
    """Every projection of the two Qwen3 configs at TP 1, 2, 4, 8 in the forms a QK-norm model
    runs it in (no RoPE epilogue, no norm chain): (op, N, K, n_groups), sorted, no duplicates."""
    from test_gemm_plan_cpu import ADD_NORM, PLAIN, SILU

    out = set()
    for cfg in CHECKPOINT_SHAPES.values():
        assert cfg.qk_norm
        H, I, D = cfg.hidden_size, cfg.intermediate_size, cfg.head_dim
        for tp in (1, 2, 4, 8):
            hq, hkv = cfg.num_heads // tp, max(cfg.num_kv_heads // tp, 1)
            out |= {(PLAIN, (hq + 2 * hkv) * D, H, 0), (SILU, 2 * I // tp, H, 0), (PLAIN, cfg.vocab_size // tp, H, 0)}
            out |= {(op, H, hq * D, 0) for op in (PLAIN, ADD_NORM)}
            out |= {(op, H, I // tp, 0) for op in (PLAIN, ADD_NORM)}
    return sorted(out)


def _qwen3_dump(tmp):
    import test_gemm_plan_cpu as gp

    exe = gp._build(tmp, False)
    stdin = "".join("%d %d %d %d\n" % s for s in qwen3_shapes())
    out = []
    for name, cus, sk, big in gp.ENVS:
        r = subprocess.run([exe, str(cus), str(sk), str(big)], input=stdin, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and not r.stderr, r.stderr[-3000:]
        out.append(f"# env {name}\n{r.stdout}")
    return "".join(out)


def test_planner_routes_of_the_qwen3_shapes_are_pinned(tmp_path):
    import test_gemm_plan_cpu as gp

    text = _qwen3_dump(tmp_path)
    shapes = qwen3_shapes()
    assert (0, 151936, 4096, 0) in shapes and 151936 % 256 != 0       # the lm_head, and its TP shards
    assert all((0, 151936 // tp, H, 0) in shapes for tp in (1, 2, 4, 8) for H in (4096, 5120))
    # every shape gets a route at every row count.  The plain and SiLU-mul forms are never refused
    # ("-").  Where the add + RMSNorm form declines, ops.gemm_add_rmsnorm runs the plain GEMM of the
    # same (N, K) and the add + norm kernel (as for the Llama presets): over every such M range the
    # plain form of that shape, in that environment, must be routed
    rows = list(gp._rows(text))
    assert {r[1:5] for r in rows} == set(shapes) and len(rows) > 200
    plain = {}
    for env, op, N, K, ng, m0, m1, r in rows:
        if op == gp.PLAIN:
            plain.setdefault((env, N, K), []).append((m0, m1, r["family"]))
    refused = 0
    for env, op, N, K, ng, m0, m1, r in rows:
        if op != gp.ADD_NORM:
            assert r["family"] != "-", (env, op, N, K, m0, m1)
        elif r["family"] == "-":
            refused += 1
            over = [(a, b, f) for a, b, f in plain[env, N, K] if a <= m1 and b >= m0]
            assert over and all(f != "-" for _, _, f in over), (env, N, K, m0, m1, over)
            # the plain intervals cover the refused range without a gap
            assert min(a for a, _, _ in over) <= m0 and max(b for _, b, _ in over) >= m1
    assert refused > 0
    with open(FIXTURE) as f:
        want = f.read()
    assert text == want, "the planner's routes of the Qwen3 shapes differ from " + FIXTURE


if __name__ == "__main__" and "--write" in sys.argv:
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        text = _qwen3_dump(d)
    with open(FIXTURE, "w") as f:
        f.write(text)
    print(f"wrote {FIXTURE}: {len(text)} bytes")
