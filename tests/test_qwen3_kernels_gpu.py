"""The QK-norm RoPE + KV writers on the GPU (ops/csrc/rope_cache_qkn.hip) and the LM head / sampler
at Qwen3's vocabulary (151936: no multiple of 256).

bf16 writer: q and K pages within one bf16 step of the contract computed in fp64 and rounded once
(~140 fp32 operations cannot move a value past a neighbouring bf16: tests/test_qwen3_cpu.py holds
the fp32 reference to the same bound), V pages bit-exact copies.  fp8 writer: device against device
and exact - its q is the bf16 writer's q, its pages and scale bytes are ``ref.fp8_quantize_rows`` of
the bf16 writer's own rows.  Unwritten slots, padding rows' cache entries and everything else keep
their sentinels.
"""
import pytest
import torch

from mlopamd import ops
from mlopamd.models.layers import rope_table
from mlopamd.ops import reference as ref
from mlopamd.runtime.sampler import sample_reference, seeded_uniform

pytestmark = pytest.mark.gpu

bf = torch.bfloat16
D, BS, NB, MAX_POS, EPS = 128, 16, 12, 40960, 1e-6
HEADS = [(2, 1), (4, 1), (16, 8), (32, 8), (64, 8)]   # 3 .. 72 normed rows: < 1 trip, exact, ragged
TOKENS = [1, 3, 33]
_CACHE = {}
_CS_DEV = {}   # the cos / sin table: "cs" on the CPU, and per device


def _inputs(T, Hq, Hkv):
    """CPU inputs of one case and the fp64 expectation, computed once and shared (read-only)."""
    key = (T, Hq, Hkv)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(1000 * T + Hq + Hkv)
    R = Hq + 2 * Hkv
    # +-m 2^e, m in 8..15, e in -6..5 (row_probes.rope_values)
    x = ((1 - 2 * torch.randint(0, 2, (T, R, D), generator=g)) * torch.randint(8, 16, (T, R, D), generator=g)
         ).double() * torch.pow(2.0, torch.randint(-6, 6, (T, R, D), generator=g).double())
    x[0, 0] = 0                                                       # all-zero q head: exactly 0 out
    x[0, Hq] = 1e-4 * torch.randn(D, generator=g).double()            # k head where eps dominates
    x[T - 1, Hq - 1] = 0
    x[T - 1, Hq - 1, 70] = 24.0                                       # one large element, zeros elsewhere
    x[T - 1, Hq + Hkv - 1] = 0
    x[T - 1, Hq + Hkv - 1, 3] = -3.0
    qkv = torch.full((T, R * D + 72), 9.0, dtype=bf)                  # row stride > (Hq + 2 Hkv) 128
    qkv[:, : R * D] = x.reshape(T, R * D).to(bf)
    pos = torch.randint(0, MAX_POS, (T,), generator=g, dtype=torch.int32)
    pos[0] = 0
    if T > 1:
        pos[1], pos[2] = 1, MAX_POS - 1
    # slots scattered over non-adjacent pages; padding rows among them (never row 0 or the last row)
    free = torch.randperm(NB * BS, generator=g)
    free = free[(free // BS) % 2 == 0][:T].to(torch.int32)
    slots = free.clone()
    if T >= 3:
        slots[1] = -1
    if T >= 33:
        slots[17] = -1
    qw = (1 + 0.3 * torch.randn(D, generator=g)).to(bf)
    kw = (0.6 + 0.25 * torch.randn(D, generator=g)).to(bf)
    if "cs" not in _CS_DEV:
        _CS_DEV["cs"] = rope_table(D, MAX_POS, 1e6, None, torch.device("cpu"))
    cs = _CS_DEV["cs"]
    xb = qkv[:, : (Hq + Hkv) * D].double().view(T, Hq + Hkv, D)
    w = torch.cat([qw.double().expand(Hq, D), kw.double().expand(Hkv, D)])[None]
    y = xb * torch.rsqrt(xb.pow(2).mean(-1, keepdim=True) + EPS) * w
    c = cs[pos.long()].double()
    e = ref.rotate(y, c[:, None, :64], c[:, None, 64:]).to(bf)
    case = dict(qkv=qkv, pos=pos, slots=slots, qw=qw, kw=kw, cs=cs, eq=e[:, :Hq], ek=e[:, Hq:],
                v=qkv[:, (Hq + Hkv) * D: R * D].reshape(T, Hkv, D).clone())
    _CACHE[key] = case
    return case


def _dev(case, gpu):
    if gpu not in _CS_DEV:
        _CS_DEV[gpu] = case["cs"].to(gpu)
    return (case["qkv"].to(gpu), case["pos"].to(gpu), _CS_DEV[gpu], case["slots"].to(gpu), case["qw"].to(gpu),
            case["kw"].to(gpu))


def _ulps(a, b):
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7fff), i)
    return (key(a.cpu()) - key(b.cpu())).abs()


def _run_bf16(case, gpu, Hq, Hkv):
    qkv, pos, cs, slots, qw, kw = _dev(case, gpu)
    T = qkv.shape[0]
    kc = torch.full((NB, Hkv, BS, D), 7.0, dtype=bf, device=gpu)
    vc = torch.full((NB, Hkv, BS, D), -7.0, dtype=bf, device=gpu)
    q = torch.full((T, Hq, D), 5.0, dtype=bf, device=gpu)
    out = ops.rope_cache(qkv, pos, cs, slots, kc, vc, Hq, q_out=q, q_norm=qw, k_norm=kw, eps=EPS)
    assert out is q
    return q, kc, vc


def _run_fp8(case, gpu, Hq, Hkv):
    qkv, pos, cs, slots, qw, kw = _dev(case, gpu)
    T = qkv.shape[0]
    k8 = torch.full((NB, Hkv, BS, D), 0x55, dtype=torch.uint8, device=gpu).view(ref.FP8)
    v8 = torch.full((NB, Hkv, BS, D), 0x2a, dtype=torch.uint8, device=gpu).view(ref.FP8)
    ks = torch.full((NB, Hkv, BS), 3, dtype=torch.uint8, device=gpu)
    vs = torch.full((NB, Hkv, BS), 5, dtype=torch.uint8, device=gpu)
    q = torch.full((T, Hq, D), 5.0, dtype=bf, device=gpu)
    ops.rope_cache(qkv, pos, cs, slots, k8, v8, Hq, q_out=q, k_scale=ks, v_scale=vs, q_norm=qw, k_norm=kw, eps=EPS)
    return q, k8, v8, ks, vs


def _live(slots):
    """[NB, BS] bool: the cache rows the launch must have written."""
    m = torch.zeros(NB * BS, dtype=torch.bool)
    m[slots[slots >= 0].long()] = True
    return m.view(NB, BS)


def _rows(cache, slots):
    """[n_live, Hkv, D]: the cache rows of the tokens with a slot, in token order (CPU)."""
    s = slots[slots >= 0].long()
    return cache.cpu()[s // BS, :, s % BS]


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_bf16_writer(gpu, T, Hq, Hkv):
    case = _inputs(T, Hq, Hkv)
    q, kc, vc = _run_bf16(case, gpu, Hq, Hkv)
    torch.cuda.synchronize()
    slots, has = case["slots"], case["slots"] >= 0
    dq, dk = _ulps(q, case["eq"]), _ulps(_rows(kc, slots), case["ek"][has])
    print(f"T={T} Hq={Hq} Hkv={Hkv}: q max {int(dq.max())} ulp ({int((dq > 0).sum())} of {dq.numel()} off), "
          f"k max {int(dk.max())} ulp ({int((dk > 0).sum())} of {dk.numel()} off)")
    assert int(dq.max()) <= 1 and int(dk.max()) <= 1
    assert bool((q[0, 0] == 0).all())                                   # the zero head: exactly 0
    assert bool(q[T - 1, Hq - 1].abs().sum() > 0)
    assert torch.equal(_rows(vc, slots), case["v"][has])                # V: bit-exact copies
    dead = ~_live(slots)[:, None, :].expand(NB, Hkv, BS)
    assert bool((kc.cpu()[dead] == 7).all()) and bool((vc.cpu()[dead] == -7).all())
    # the norm is really there: the same rows without weights differ
    plain = ops.rope_cache(*_dev(case, gpu)[:4], kc.clone(), vc.clone(), Hq)
    assert not torch.equal(plain, q)


@pytest.mark.parametrize("T", TOKENS)
@pytest.mark.parametrize("Hq,Hkv", HEADS)
def test_fp8_writer_is_the_bf16_writer_quantised(gpu, T, Hq, Hkv):
    case = _inputs(T, Hq, Hkv)
    qb, kc, vc = _run_bf16(case, gpu, Hq, Hkv)
    q8, k8, v8, ks, vs = _run_fp8(case, gpu, Hq, Hkv)
    torch.cuda.synchronize()
    assert torch.equal(q8, qb)                                          # bit-identical q
    slots = case["slots"]
    live = _live(slots)[:, None, :].expand(NB, Hkv, BS)
    for pages, scales, rows, fill, sfill in ((k8, ks, kc, 0x55, 3), (v8, vs, vc, 0x2a, 5)):
        e8, es = ref.fp8_quantize_rows(rows.cpu())                      # of the bf16 writer's own rows
        pb, sb = pages.cpu().view(torch.uint8), scales.cpu()
        assert torch.equal(pb[live], e8.view(torch.uint8)[live])
        assert torch.equal(sb[live], es[live])
        assert bool((pb[~live] == fill).all()) and bool((sb[~live] == sfill).all())


@pytest.mark.parametrize("Hq,Hkv", [(4, 1), (32, 8)])
def test_fp8_v_pages_equal_the_plain_fp8_writers(gpu, Hq, Hkv):
    """V rows are untouched by the norm, so the QK-norm fp8 writer and kv_fp8.hip's writer must give
    the same V pages and scale bytes: this holds rope_cache_qkn.hip's copies of the row maximum,
    scale exponent and quantiser to kv_fp8.hip's originals, device against device."""
    case = _inputs(33, Hq, Hkv)
    _, _, v8, _, vs = _run_fp8(case, gpu, Hq, Hkv)
    qkv, pos, cs, slots, _, _ = _dev(case, gpu)
    pk = torch.full((NB, Hkv, BS, D), 0x55, dtype=torch.uint8, device=gpu).view(ref.FP8)
    pv = torch.full((NB, Hkv, BS, D), 0x2a, dtype=torch.uint8, device=gpu).view(ref.FP8)
    pks = torch.full((NB, Hkv, BS), 3, dtype=torch.uint8, device=gpu)
    pvs = torch.full((NB, Hkv, BS), 5, dtype=torch.uint8, device=gpu)
    ops.rope_cache(qkv, pos, cs, slots, pk, pv, Hq, k_scale=pks, v_scale=pvs)
    assert torch.equal(pv.view(torch.uint8), v8.view(torch.uint8)) and torch.equal(pvs, vs)


def test_no_weights_is_the_plain_writer(gpu):
    """Without q_norm / k_norm, ops.rope_cache issues the launch it always did."""
    Hq, Hkv = 4, 1
    case = _inputs(33, Hq, Hkv)
    qkv, pos, cs, slots, _, _ = _dev(case, gpu)
    mk = lambda: (torch.zeros(NB, Hkv, BS, D, dtype=bf, device=gpu), torch.zeros(NB, Hkv, BS, D, dtype=bf, device=gpu),  # noqa: E731
                  torch.zeros(33, Hq, D, dtype=bf, device=gpu))
    k1, v1, q1 = mk()
    k2, v2, q2 = mk()
    ops.rope_cache(qkv, pos, cs, slots, k1, v1, Hq, q_out=q1)
    torch.ops.mlop.rope_cache(q2, k2, v2, qkv, pos, cs, slots)
    assert torch.equal(q1, q2) and torch.equal(k1, k2) and torch.equal(v1, v2)
    with pytest.raises(ValueError, match="both q_norm and k_norm"):
        ops.rope_cache(qkv, pos, cs, slots, k1, v1, Hq, q_norm=case["qw"].to(gpu))
    with pytest.raises(RuntimeError, match="q_norm / k_norm"):          # the binding's weight checks
        ops.rope_cache(qkv, pos, cs, slots, k1, v1, Hq, q_norm=case["qw"].to(gpu),
                       k_norm=torch.ones(64, dtype=bf, device=gpu), eps=EPS)


@pytest.mark.parametrize("fp8", [False, True])
def test_repeats_and_graph_replay_are_bit_identical(gpu, fp8):
    Hq, Hkv = 32, 8
    case = _inputs(33, Hq, Hkv)
    run = _run_fp8 if fp8 else _run_bf16
    first = [t.clone() for t in run(case, gpu, Hq, Hkv)]
    for _ in range(2):
        again = run(case, gpu, Hq, Hkv)
        assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(first, again))
    # captured and replayed once: the eager result
    qkv, pos, cs, slots, qw, kw = _dev(case, gpu)
    outs = [torch.zeros_like(t) for t in first]
    kwargs = dict(q_out=outs[0], q_norm=qw, k_norm=kw, eps=EPS)
    if fp8:
        kwargs.update(k_scale=outs[3], v_scale=outs[4])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.rope_cache(qkv, pos, cs, slots, outs[1], outs[2], Hq, **kwargs)   # warm-up outside capture
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.rope_cache(qkv, pos, cs, slots, outs[1], outs[2], Hq, **kwargs)
    for t in outs:
        t.view(torch.uint8).zero_()
    graph.replay()
    torch.cuda.synchronize()
    live = _live(case["slots"])[:, None, :].expand(NB, Hkv, BS)
    assert torch.equal(outs[0], first[0])
    for got, want in zip(outs[1:], first[1:]):
        assert torch.equal(got.cpu().view(torch.uint8)[live], want.cpu().view(torch.uint8)[live])
        assert bool((got.cpu().view(torch.uint8)[~live] == 0).all())


# ----------------------------------------------------- LM head at V = 151936 --

V = 151936


@pytest.fixture(scope="module")
def lm_head(gpu):
    torch.manual_seed(V)
    return (0.05 * torch.randn(V, 256, device=gpu)).to(bf)


@pytest.mark.parametrize("M", [1, 5, 300, 600])   # GEMV, 16-row tiles, 256-row tiles, ping-pong
def test_lm_head_gemm_at_qwen3_vocab(gpu, lm_head, M):
    """N = 151936 = 593.5 x 256: the last tile column of every route is half empty."""
    torch.manual_seed(M)
    x = torch.randn(M, 256, device=gpu, dtype=bf)
    ops.GEMM_BACKEND = "mlop"
    try:
        y = ops.gemm(x, lm_head)
    finally:
        ops.GEMM_BACKEND = ops.GEMM_BACKEND_DEFAULT
    exp = x.float() @ lm_head.float().t()
    # tests/test_kernels_gpu.py::test_gemm's tolerance
    torch.testing.assert_close(y.float(), exp, atol=3e-2 * exp.abs().max().item() / 10 + 1e-2, rtol=2e-2)


def test_sampling_at_qwen3_vocab(gpu):
    """Greedy and seeded draws over (2, 151936) bf16 logits against sample_reference.  Logits are
    multiples of 1/4 (exact in bf16): a bulk in [0, 2] with ties everywhere and 64 distinct values
    in [8, 24) that carry the mass, so a draw's uniform falls well inside one token's interval.
    Row 0 has 40 of them in the last 128 ids, past the last full 256-id block."""
    g = torch.Generator().manual_seed(7)
    logits = (torch.randint(0, 9, (2, V), generator=g).float() / 4)
    for r in range(2):
        ids = torch.randperm(V - 128, generator=g)[:64]
        if r == 0:
            ids[:40] = V - 128 + torch.randperm(128, generator=g)[:40]
        logits[r, ids] = 8 + torch.randperm(64, generator=g).float() / 4
    logits = logits.to(bf)
    dev = logits.to(gpu)
    order = torch.sort(-logits.float(), stable=True).indices
    assert ops.argmax(dev).cpu().tolist() == order[:, 0].tolist()
    assert int(order[0, 0]) >= V - 128 or int(order[0, 1]) >= V - 128 or int(order[0, 2]) >= V - 128
    tied = logits.clone()
    tied[0, V - 1] = tied[0, V - 3] = tied[1, 5] = tied[1, V - 2] = 30.0   # tied maxima: the lower id wins
    assert ops.argmax(tied.to(gpu)).cpu().tolist() == [V - 3, 5]
    for n, (T, k, p) in enumerate([(0.8, 20, 0.9), (1.0, 0, 1.0), (0.7, 0, 0.5), (1.0, 1000, 1.0), (0.0, 0, 1.0)]):
        temps, ks, ps = torch.full((2,), T), torch.full((2,), k, dtype=torch.int32), torch.full((2,), p)
        u = torch.tensor([seeded_uniform(11, n), seeded_uniform(12, n)], dtype=torch.float32)
        want = sample_reference(logits.float(), temps, ks, ps, u)
        got = ops.sample(dev.float(), temps.to(gpu), ks.to(gpu), ps.to(gpu), u.to(gpu)).cpu()
        print(f"T={T} top_k={k} top_p={p}: drew {got.tolist()}, the reference {want.tolist()}")
        assert got.tolist() == want.tolist(), (T, k, p)
