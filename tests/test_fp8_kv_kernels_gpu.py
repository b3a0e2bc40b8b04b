"""The fp8 KV cache kernels: kv_fp8.hip's RoPE + cache writer and attention.hip's decode
kernel (KvFp8) over e4m3fn pages with one power-of-two scale byte per (token, kv head) row.

Writer: the scale bytes are the reference rule (ops/reference.py) applied to an fp32 RoPE
reference, the stored rows are within half an e4m3 ulp (+ half the subnormal spacing, + the
bf16 rounding of the RoPE result) of it, skipped slots are untouched and q is the bf16 op's q.

Attention: Q, P and the MFMAs are bf16 and the fp8 -> bf16 conversion of K and V is exact, so
the oracle is the fp32 reference over the DEQUANTISED pages the writer produced, at
test_paged_attention's tolerance; the exact probes of tests/attn_probes.py (counting, needle)
run on quantised copies of their caches, whose values the format holds exactly (0 / 1 / 64,
+-1 / +-2) or whose dequantised rows are the expected values (the needle's V)."""
import functools
import math

import numpy as np
import pytest
import torch

import attn_probes as ap
from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
D, BS = 128, 16


def cos_sin_table(max_pos, theta=10000.0):
    inv = 1.0 / theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D)
    ang = torch.arange(max_pos, dtype=torch.float64)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.sin()], -1).float()


def fp8_caches(NB, Hkv, device, fill=0):
    """e4m3fn pages and scale bytes, every byte ``fill`` (0: as the engine allocates them)."""
    mk = lambda *s: torch.full(s, fill, dtype=torch.uint8, device=device)  # noqa: E731
    return (mk(NB, Hkv, BS, D).view(ref.FP8), mk(NB, Hkv, BS, D).view(ref.FP8), mk(NB, Hkv, BS), mk(NB, Hkv, BS))


# ------------------------------------------------------------------ writer --

def rope_fp32(qkv, pos, cs, Hq, Hkv):
    """fp32 RoPE of the k heads and the raw v heads: [T, Hkv, D] each (no bf16 rounding)."""
    T = qkv.shape[0]
    x = qkv.float().view(T, Hq + 2 * Hkv, D)
    c = cs[pos.long()]
    k = ref.rotate(x[:, Hq:Hq + Hkv], c[:, None, :D // 2], c[:, None, D // 2:])
    return k, x[:, Hq + Hkv:]


def writer_inputs(T, Hq, Hkv, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(T, (Hq + 2 * Hkv) * D, generator=g)
    if T >= 7:   # an all-zero token, a huge one and a tiny one
        qkv[2] = 0
        qkv[3] *= 1e4
        qkv[4] *= 1e-6
    pos = torch.randint(0, 301, (T,), generator=g, dtype=torch.int32)
    slots = (torch.randperm(6 * BS, generator=g)[:T] + BS).to(torch.int32)   # pages 1 .. 6 of 8
    if T >= 7:
        slots[1] = -1  # a padding token
    return qkv.to(bf), pos, slots


def boundary_margin(amax):
    """Distance of amax's frexp mantissa from 0.875, where the scale exponent steps (a power of
    two itself is no step: m -> 1 at x and m = 0.5 at x + 1 give the same exponent)."""
    m, _ = torch.frexp(amax.float())
    return torch.where(amax > 0, (m - 0.875).abs(), torch.ones_like(m))


@functools.lru_cache(maxsize=None)
def writer_seed(T, Hq, Hkv):
    """The first seed whose rows' amax all stay clear of an exponent step by 1.5 bf16 ulps (2^-8
    of the mantissa each) on the CPU; the test asserts one ulp on the device's own reference."""
    cs = cos_sin_table(512)
    for seed in range(4000):
        qkv, pos, _ = writer_inputs(T, Hq, Hkv, seed)
        k, v = rope_fp32(qkv, pos, cs, Hq, Hkv)
        if min(float(boundary_margin(t.abs().amax(-1)).min()) for t in (k, v)) > 1.5 * 2.0 ** -8:
            return seed
    raise AssertionError("no seed keeps every row off the exponent steps")


@pytest.mark.parametrize("heads", [(8, 2), (8, 1), (4, 4)], ids=lambda h: f"{h[0]}q{h[1]}kv")
@pytest.mark.parametrize("T", [1, 7, 33])
def test_writer(gpu, T, heads):
    Hq, Hkv = heads
    NB = 8
    qkv, pos, slots = (t.to(gpu) for t in writer_inputs(T, Hq, Hkv, writer_seed(T, Hq, Hkv)))
    cs = cos_sin_table(512).to(gpu)
    SENT = 0x2A  # skipped slots must keep it (pages and scales)
    kc, vc, ks, vs = fp8_caches(NB, Hkv, gpu, fill=SENT)
    q = ops.rope_cache(qkv, pos, cs, slots, kc, vc, Hq, k_scale=ks, v_scale=vs)
    # q: the bf16 op's, bit for bit
    kb, vb = (torch.zeros(NB, Hkv, BS, D, dtype=bf, device=gpu) for _ in range(2))
    q_bf = ops.rope_cache(qkv, pos, cs, slots, kb, vb, Hq)
    assert torch.equal(q.view(torch.int16), q_bf.view(torch.int16))

    k_ref, v_ref = rope_fp32(qkv, pos, cs, Hq, Hkv)          # the device's own fp32 reference
    written = torch.zeros(NB * BS, dtype=torch.bool, device=gpu)
    live = slots >= 0
    written[slots[live].long()] = True
    for name, cache, scales, r in (("k", kc, ks, k_ref), ("v", vc, vs, v_ref)):
        bytes_ = cache.view(torch.uint8).permute(0, 2, 1, 3).reshape(NB * BS, Hkv, D)   # [slot, Hkv, D]
        sbytes = scales.permute(0, 2, 1).reshape(NB * BS, Hkv)
        assert (bytes_[~written] == SENT).all() and (sbytes[~written] == SENT).all(), f"{name}: a skipped slot changed"
        amax = r.abs().amax(-1)[live]
        assert float(boundary_margin(amax).min()) > 2.0 ** -8, "a row within one bf16 ulp of an exponent step"
        want = ref.fp8_row_exponent(amax) + 127
        got = sbytes[slots[live].long()].to(torch.int32)
        assert torch.equal(got, want), f"{name}: scale bytes {got[got != want]} != {want[got != want]}"
        deq = ref.fp8_dequantize_rows(bytes_.view(ref.FP8)[slots[live].long()], sbytes[slots[live].long()])
        rl = r[live]
        bound = 2.0 ** -4 * rl.abs() + 2.0 ** -10 * ref.fp8_scale_decode(sbytes[slots[live].long()])[..., None] \
            + 2.0 ** -8 * rl.abs()
        err = (deq - rl).abs()
        print(f"writer {name} T={T} {Hq}/{Hkv}: max err/bound {float((err / bound.clamp_min(1e-45)).max()):.3f}")
        assert (err <= bound).all(), f"{name}: {int((err > bound).sum())} elements off"
        if T >= 7:   # the all-zero token: zero bytes (RoPE may leave -0: 0x80), the smallest exponent
            z = int(slots[2])
            assert ((bytes_[z] & 0x7F) == 0).all() and (sbytes[z] == ref.FP8_EXP_MIN + 127).all()


# --------------------------------------------------------------- attention --

HKV = 2
CTXS = [1, 15, 16, 17, 31, 32, 33, 127, 129, 300]
# (part_tokens, nparts, in-launch combine): 3 x 128 >= 300
FORMS = {"one": (None, 1, False), "reduce3": (128, 3, False), "fused3": (128, 3, True)}


def oracle_launch(G):
    """Decode rows at every page / pair edge, 5-token rows, a chunk that straddles tiles, a chunk
    of 40 behind 89 cached tokens, a prompt of 40 wholly on the 16-row tiles, one padding row."""
    q_lens = [1] * len(CTXS) + [5, 5, 16 // G + 1, 40, 40, 1]
    return q_lens, CTXS + [35, 300, 260, 129, 40, 0]


@functools.lru_cache(maxsize=8)
def written_case(device, G, seed=0):
    """A launch whose pages the fp8 WRITER filled (every context token through ops.rope_cache),
    its queries, and the fp32 oracle over the dequantised pages."""
    q_lens, ctx_lens = oracle_launch(G)
    Hq = HKV * G
    m = ap.make_layout(q_lens, ctx_lens, HKV, G, device=device, seed=seed)
    g = torch.Generator().manual_seed(seed)
    bt = m.host["bt"]
    pos, slots = [], []
    for r, c in zip(m.host["rows"], ctx_lens):
        j = np.arange(c)
        pos.append(j)
        slots.append(bt[r, j // BS] * BS + j % BS)
    pos, slots = (torch.from_numpy(np.concatenate(a).astype(np.int32)).to(device) for a in (pos, slots))
    N = pos.numel()
    qkv = torch.randn(N, (Hq + 2 * HKV) * D, generator=g)
    qkv[:, (Hq + HKV + 1) * D:] *= 2.0 ** -5    # kv head 1: V rows at Llama's magnitudes (head 0: unit)
    kc, vc, ks, vs = fp8_caches(m.NB, HKV, device)
    ops.rope_cache(qkv.to(bf).to(device), pos, cos_sin_table(512).to(device), slots, kc, vc, Hq, k_scale=ks, v_scale=vs)
    q = torch.randn(m.num_tokens, Hq, D, generator=g).to(bf).to(device)
    cpu = ap.Meta()
    cpu.__dict__.update({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in m.__dict__.items()})
    want = ref.paged_attention(q.cpu().float(), kc.cpu(), vc.cpu(), cpu, ks.cpu(), vs.cpu())   # fp32 throughout
    return m, q, (kc, vc, ks, vs), want.to(device)


def run_fp8(m, q, caches, out=None):
    kc, vc, ks, vs = caches
    out = torch.full_like(q, float("nan")) if out is None else out
    return ops.paged_attention(q, kc, vc, m, out=out, k_scale=ks, v_scale=vs)


def launch_forms(m, q, caches, check, part_tokens, nparts, fused, what):
    m = ap.repartition(m, part_tokens, nparts, sem=fused)
    outs = [run_fp8(m, q, caches)]
    check(outs[0], what)
    if fused:
        assert int(m.part_sem.abs().sum()) == 0, f"{what}: tickets not re-armed"
        outs.append(run_fp8(m, q, caches))
        assert int(m.part_sem.abs().sum()) == 0, f"{what}: tickets not re-armed"
        assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{what}: relaunch differs"
    return outs[0]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("G", [1, 4, 8, 16])
def test_attention_oracle(gpu, attn_fused_all, G, form):
    m, q, caches, want = written_case(str(gpu), G)
    assert m.ptile_seq.numel() == 0 and m.tile_seq.numel() >= 8

    def check(out, what):
        assert torch.isfinite(out).all(), f"{what}: non-finite rows"
        err = (out.float() - want).abs()
        print(f"fp8 attention G={G} {what}: max |err| {float(err.max()):.4f}, "
              f"max err/tol {float((err / (2e-2 + 2e-2 * want.abs())).max()):.3f}")
        torch.testing.assert_close(out.float(), want, atol=2e-2, rtol=2e-2)
        pad = int(m.host["q_start"][m.host["rows"][-1]])           # the ctx-0 row
        assert float(out[pad].abs().max()) == 0.0

    launch_forms(m, q, caches, check, *FORMS[form], form)


@pytest.mark.parametrize("form", list(FORMS))
def test_nt_policies_bit_identical(gpu, attn_fused_all, form):
    m, q, caches, _ = written_case(str(gpu), 4)
    m = ap.repartition(m, *FORMS[form][:2], sem=FORMS[form][2])
    prev = torch.ops.mlop.attn_kv_nt(-1)
    outs = []
    try:
        for nt in (0, 1, 3):
            torch.ops.mlop.attn_kv_nt(nt)
            outs.append(run_fp8(m, q, caches))
    finally:
        torch.ops.mlop.attn_kv_nt(prev)
    assert all(torch.equal(outs[0].view(torch.int16), o.view(torch.int16)) for o in outs[1:])


def test_fused_and_reduce_combine_bit_identical(gpu, attn_fused_all):
    """The in-launch combine and the reduce launch are one function over the same slabs in the
    same order: written_case's launch (contexts 1 .. 300, three partitions of 128, G = 4) gives
    the same bytes either way.  (bf16 and windowed bf16: test_probes_attention_gpu.py.)"""
    m, q, caches, _ = written_case(str(gpu), 4)
    outs = {}
    for form in ("reduce3", "fused3"):
        outs[form] = run_fp8(ap.repartition(m, *FORMS[form][:2], sem=FORMS[form][2]), q, caches)
        assert torch.isfinite(outs[form]).all()
    assert torch.equal(outs["reduce3"].view(torch.int16), outs["fused3"].view(torch.int16))


# ------------------------------------------------------------------ probes --

def quantize_probe(kc, vc, nan_pages):
    """The probe's bf16 caches in the fp8 format (quantised on the CPU by the reference rule).
    The pages that must never be read keep NaN in every page byte (0x7f) and get a NaN-free but
    huge scale (byte 254 = 2^127): touching one cannot stay unnoticed, as in the bf16 probes."""
    dev = kc.device
    nan = torch.as_tensor(np.asarray(nan_pages, np.int64))
    out = []
    for c in (kc, vc):
        c = c.cpu().clone()
        assert torch.isnan(c[nan]).all()
        c[nan] = 0
        assert torch.isfinite(c).all()
        c8, sb = ref.fp8_quantize_rows(c)
        c8.view(torch.uint8)[nan] = 0x7F
        sb[nan] = 254
        out += [c8.to(dev), sb.to(dev)]
    return out[0], out[2], out[1], out[3]


@functools.lru_cache(maxsize=8)
def count_probe(device, G):
    q_lens, ctx_lens = ap.decode_launch(G)
    m, q, kc, vc, exp = ap.build("count", q_lens, ctx_lens, ap.HKV, G, device=device)
    caches = quantize_probe(kc, vc, m.host["nan_pages"])
    # V in {0, 1} and the dead slots' 64 are exact in the format: the expected values stand
    nan = torch.as_tensor(np.asarray(m.host["nan_pages"], np.int64))
    live = torch.ones(m.NB, dtype=torch.bool)
    live[nan] = False
    assert torch.equal(ref.fp8_dequantize_rows(caches[1].cpu(), caches[3].cpu())[live], vc.cpu().float()[live])
    return m, q, caches, exp


@pytest.mark.parametrize("form", ["one", "reduce256", "fused256", "parts32"])
@pytest.mark.parametrize("G", [4, 16])
def test_counting_probe(gpu, attn_fused_all, G, form):
    """Which keys are visible, up to 1500 keys: one bf16 ulp, expected zeros exactly zero."""
    m, q, caches, exp = count_probe(str(gpu), G)
    assert max(m.host["ctx_len"]) == 1500
    launch_forms(m, q, caches, lambda out, what: ap.assert_probe(out, exp, what), *ap.DECODE_FORMS[form], f"count/{form}")


@functools.lru_cache(maxsize=8)
def needle_probe(device, G, schedule, seed=0):
    """The needle probe with its V rows through the format: expected = dequantised V[target]
    (a (token, head)'s expected row IS one stored (token, kv head) row, and the quantiser works
    row by row).  The builder's conditions on its inputs are run again on the dequantised K / V."""
    q_lens, ctx_lens = ap.decode_launch(G)
    seen = {}
    orig = ap._needle_conditions

    def spy(*a):
        seen["args"] = a
        return orig(*a)

    ap._needle_conditions = spy
    try:
        m, q, kc, vc, exp = ap.build("needle", q_lens, ctx_lens, ap.HKV, G, device=device, seed=seed, schedule=schedule)
    finally:
        ap._needle_conditions = orig
    Kl, Vl, *rest = seen["args"]
    Kq, Vq = ref.fp8_fake_quant(Kl), ref.fp8_fake_quant(Vl)
    assert torch.equal(Kq, Kl.float())               # +-1 rows are exact: the scores do not move
    orig(Kq, Vq.to(bf), *rest)                       # margin and leak bounds on the dequantised values
    assert torch.equal(Vq.to(bf).float(), Vq)        # 4 significant bits: the expected rows are bf16 values
    caches = quantize_probe(kc, vc, m.host["nan_pages"])
    return m, q, caches, ref.fp8_fake_quant(exp.cpu()).to(bf).to(device)


@pytest.mark.parametrize("form", ["one", "fused256"])
@pytest.mark.parametrize("schedule", ap.SCHEDULES)
@pytest.mark.parametrize("G", [4, 16])
def test_needle_probe(gpu, attn_fused_all, G, schedule, form):
    """Which V row goes with which K, the running max and its rescale, dead slots and NaN pages
    (pages and scale rows) in the module's conventions."""
    m, q, caches, exp = needle_probe(str(gpu), G, schedule)
    launch_forms(m, q, caches, lambda out, what: ap.assert_probe(out, exp, what), *ap.DECODE_FORMS[form],
                 f"needle/{schedule}/{form}")


def test_missing_scales_and_flash_tiles_are_errors(gpu):
    """No quiet fall-back: an fp8 cache without scales, or metadata with flash tiles, raises."""
    m, q, caches, _ = written_case(str(gpu), 4)
    with pytest.raises(ValueError):
        ops.paged_attention(q, caches[0], caches[1], m)
    q_lens, ctx_lens = [40], [40]
    mf = ap.make_layout(q_lens, ctx_lens, HKV, 4, flash_min_q=17, device=str(gpu))
    kc, vc, ks, vs = fp8_caches(mf.NB, HKV, gpu)
    qq = torch.zeros(40, HKV * 4, D, dtype=bf, device=gpu)
    with pytest.raises(NotImplementedError):
        ops.paged_attention(qq, kc, vc, mf, k_scale=ks, v_scale=vs)
    assert math.isfinite(float(q.float().sum()))
