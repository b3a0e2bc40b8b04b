"""Multi-LoRA kernels (ops/csrc/lora.hip) against an fp64 oracle built from the same bf16 values.

Bounds (set before the kernels ran, not tuned against them):
  shrink   |got - ref| <= 4 K 2^-24 sum_k |x_k a_k| per element: the fp32 summation bound of any
           order, times 4 for the matrix core's internal rounding;
  expand   |got - ref| <= 2^-8 |ref| (the single bf16 rounding of y + delta, with slack) plus the
           same sum bound over the R rank terms of the delta, 4 R 2^-24 sum_r |tmp_r b_r|;
  chain    (graph test: expand fed by the kernel's own shrink) additionally the shrink's bound
           carried through the expand, sum_r E_tmp[r] |b_r|.
"""
import pytest
import torch

from mlopamd import ops

pytestmark = pytest.mark.gpu

S, R = 4, 64
RANKS = (8, 16, 64, 16)
# (K, N, rows of each sub-projection or "interleaved")
SHAPES = {
    "qkv_small": (256, 768, (512, 128, 128)),
    "o_small": (512, 256, (256,)),
    "gate_up_small": (256, 1024, "interleaved"),
    "qkv_8b": (4096, 6144, (4096, 1024, 1024)),
    "down_8b": (14336, 4096, (4096,)),
}
TS = (1, 15, 16, 17, 33, 100)
EPS24 = 2.0 ** -24


def _tile_group(N, parts):
    if parts == "interleaved":
        return (torch.arange(N // 16) & 1).to(torch.uint8), 2
    tg = torch.cat([torch.full((n // 16,), g, dtype=torch.uint8) for g, n in enumerate(parts)])
    return tg, len(parts)


_CACHE = {}


def _weights(name):
    """Adapter stacks of one shape (built once, never modified by a test)."""
    if name in _CACHE:
        return _CACHE[name]
    K, N, parts = SHAPES[name]
    tg, G = _tile_group(N, parts)
    gen = torch.Generator().manual_seed(1000 + sorted(SHAPES).index(name))
    A = torch.randn(S, G * R, K, generator=gen) * K ** -0.5
    B = torch.randn(S, N, R, generator=gen)
    for s, r in enumerate(RANKS):  # rows / columns of the smaller ranks are zero
        A.view(S, G, R, K)[s, :, r:] = 0
        B[s, :, r:] = 0
    dev = "cuda"
    out = dict(K=K, N=N, G=G, A=A.to(dev, torch.bfloat16), B=B.to(dev, torch.bfloat16), tg=tg.to(dev),
               rank=torch.tensor(RANKS, dtype=torch.int32, device=dev),
               col_g=tg.long().repeat_interleave(16).to(dev))
    _CACHE[name] = out
    return out


def _patterns(T):
    runs = [0] * 5 + [2] * 4 + [-1] * 3 + [1] * 4 + [3] * 6 + [-1] * 2 + [0] * 3
    mix = (runs * (T // len(runs) + 1))[:T]
    return {"one": [2] * T, "none": [-1] * T, "runs": mix, "cycle": [t % S for t in range(T)]}


def _shrink_oracle(x, A, ts):
    """fp64 tmp [T, GR] and the per-element sum of |x_k a_k|."""
    xd, sel = x.double(), ts.clamp(min=0).long()
    Ad = A.double()[sel]                                   # [T, GR, K]
    ref = torch.einsum("tk,tjk->tj", xd, Ad)
    mag = torch.einsum("tk,tjk->tj", xd.abs(), Ad.abs())
    live = (ts >= 0)[:, None]
    return ref * live, mag * live


def _expand_oracle(y, tmp, B, col_g, ts):
    """fp64 y + delta [T, N] and the per-element sum of |tmp_r b_r| (rows with slot -1: y, 0)."""
    T, N = y.shape
    sel = ts.clamp(min=0).long()
    Bd = B.double()[sel]                                   # [T, N, R]
    tg = tmp.double().view(T, -1, R)[:, col_g]             # [T, N, R]: each column's A block
    delta = (tg * Bd).sum(-1)
    mag = (tg.abs() * Bd.abs()).sum(-1)
    live = (ts >= 0)[:, None]
    return y.double() + delta * live, mag * live, Bd.abs()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_shrink_expand(gpu, name, T):
    w = _weights(name)
    K, N, G = w["K"], w["N"], w["G"]
    gen = torch.Generator().manual_seed(7 * T + K)
    x = torch.randn(T, K, generator=gen).to("cuda", torch.bfloat16)
    y0 = torch.randn(T, N, generator=gen).to("cuda", torch.bfloat16)
    for pname, pat in _patterns(T).items():
        ts = torch.tensor(pat, dtype=torch.int32, device="cuda")
        # ---- shrink
        ref, mag = _shrink_oracle(x, w["A"], ts)
        got = ops.lora_shrink(x, w["A"], ts, w["rank"], groups=G)
        assert got.dtype == torch.float32 and got.shape == (T, G * R)
        err = (got.double() - ref).abs()
        bound = 4 * K * EPS24 * mag
        print(f"{name} T={T} {pname}: shrink max err/bound {float((err / bound.clamp(min=1e-30)).max()):.3f}")
        assert bool((err <= bound).all()), (name, T, pname, float((err - bound).max()))
        assert bool((got[ts < 0] == 0).all())
        assert torch.equal(got, ops.lora_shrink(x, w["A"], ts, w["rank"], groups=G)), "shrink not reproducible"
        assert torch.equal(got, ops.lora_shrink(x, w["A"], ts, w["rank"])), "rank skip changed the result"
        # ---- expand, fed the oracle's tmp rounded to fp32
        tmp = ref.float()
        yref, ymag, _ = _expand_oracle(y0, tmp, w["B"], w["col_g"], ts)
        y = y0.clone()
        assert ops.lora_expand_add(y, tmp, w["B"], w["tg"], ts, w["rank"]) is y
        err = (y.double() - yref).abs()
        bound = 2.0 ** -8 * yref.abs() + 4 * R * EPS24 * ymag
        print(f"{name} T={T} {pname}: expand max err/bound {float((err / bound.clamp(min=1e-30)).max()):.3f}")
        assert bool((err <= bound).all()), (name, T, pname, float((err - bound).max()))
        assert torch.equal(y[ts < 0], y0[ts < 0]), "rows without an adapter must not be written"
        y2 = y0.clone()
        ops.lora_expand_add(y2, tmp, w["B"], w["tg"], ts, w["rank"])
        assert torch.equal(y, y2), "expand not reproducible"


def test_strided_rows(gpu):
    """x / y as column slices of wider matrices (row stride > width)."""
    w = _weights("qkv_small")
    K, N, G, T = w["K"], w["N"], w["G"], 21
    gen = torch.Generator().manual_seed(5)
    xw = torch.randn(T, K + 64, generator=gen).to("cuda", torch.bfloat16)
    yw = torch.randn(T, N + 32, generator=gen).to("cuda", torch.bfloat16)
    ts = torch.tensor(_patterns(T)["runs"], dtype=torch.int32, device="cuda")
    x, y = xw[:, :K], yw[:, :N]
    got = ops.lora_shrink(x, w["A"], ts, w["rank"], groups=G)
    assert torch.equal(got, ops.lora_shrink(x.contiguous(), w["A"], ts, w["rank"], groups=G))
    yc, tail = y.contiguous(), yw[:, N:].clone()
    ops.lora_expand_add(y, got, w["B"], w["tg"], ts, w["rank"])
    ops.lora_expand_add(yc, got, w["B"], w["tg"], ts, w["rank"])
    assert torch.equal(y, yc) and torch.equal(yw[:, N:], tail)


def test_graph_replay_follows_slot_and_weight_updates(gpu):
    """A captured shrink + expand reads tok_slot and the slot-major stacks through fixed pointers:
    after tok_slot and one slot's weights are overwritten in place, a replay computes the new
    contents."""
    w = _weights("qkv_small")
    K, N, G, T = w["K"], w["N"], w["G"], 33
    A, B, rank = w["A"].clone(), w["B"].clone(), w["rank"].clone()
    gen = torch.Generator().manual_seed(11)
    x = torch.randn(T, K, generator=gen).to("cuda", torch.bfloat16)
    y0 = torch.randn(T, N, generator=gen).to("cuda", torch.bfloat16)
    pats = _patterns(T)
    ts = torch.tensor(pats["cycle"], dtype=torch.int32, device="cuda")
    y = y0.clone()
    tmp = torch.empty(T, G * R, dtype=torch.float32, device="cuda")

    def run():
        ops.lora_shrink(x, A, ts, rank, groups=G, out=tmp)
        ops.lora_expand_add(y, tmp, B, w["tg"], ts, rank)

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        run()
        stream.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=stream):
            run()
    torch.cuda.current_stream().wait_stream(stream)

    def check():
        ref, mag = _shrink_oracle(x, A, ts)
        yref, ymag, Babs = _expand_oracle(y0, ref, B, w["col_g"], ts)
        e_tmp = (4 * K * EPS24 * mag).view(T, G, R)[:, w["col_g"]]       # [T, N, R]
        bound = 2.0 ** -8 * yref.abs() + 4 * R * EPS24 * ymag + (e_tmp * Babs).sum(-1)
        y.copy_(y0)
        g.replay()
        torch.cuda.synchronize()
        err = (y.double() - yref).abs()
        assert bool((err <= bound).all()), float((err - bound).max())
        return y.clone()

    first = check()
    # new step: other slots per token; slot 1 reloaded with a rank-64 adapter
    ts.copy_(torch.tensor(pats["runs"], dtype=torch.int32, device="cuda"))
    A[1] = (torch.randn(G * R, K, generator=gen) * K ** -0.5).to("cuda", torch.bfloat16)
    B[1] = torch.randn(N, R, generator=gen).to("cuda", torch.bfloat16)
    rank[1] = 64
    second = check()
    assert not torch.equal(first, second)
