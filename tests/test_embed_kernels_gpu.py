"""Exact tests of the embedding pooling kernels (ops/csrc/pool.hip) against ``pool_reference``.

``mean`` accumulators must equal the sequential fp32 row loop BIT FOR BIT (the rows hold values whose
fp32 sum depends on the order, so a tree or any reordered sum fails), however a segment is cut into
chunks; ``last`` copies exactly row r1 - 1; rows outside every segment (NaN here) are never read and
unnamed slots never written.  The finished vector is held to rtol 1e-5 of the float64 finish of the
exact fp32 sums: the factor common to all components comes from an fp32 sum of squares whose longest
dependent chain is a few dozen terms, a square root, a divide and a multiply, some tens of fp32 ulps
at worst (1e-5 is about 84), and a relaunch must repeat it bit for bit."""
import pytest
import torch

from mlopamd import ops
from mlopamd.models.config import TINY_LLAMA
from mlopamd.ops.reference import (POOL_FIN_MEAN, POOL_FIN_NORMALIZE, POOL_INIT, POOL_LAST, POOL_MODE_LAST,
                                   pool_reference)

pytestmark = pytest.mark.gpu
HS = (TINY_LLAMA.hidden_size, 4096, 5120, 8192)
LENS = (1, 2, 15, 16, 17, 300)
SLOTS = 9
BIG = float(2 ** 24)
SENTINEL = -7.25


def _i32(rows, dev):
    return torch.tensor(rows, dtype=torch.int32, device=dev).reshape(-1, 4)


def _order_rows(L, H, seed):
    """[L, H] bf16-representable rows whose column sums depend on the order: per column +2^24 at one
    row and -2^24 at another (staggered over the columns), small integers elsewhere: once 2^24 is in
    the running sum the small terms are rounded away, before it they are not."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(1, 4, (L, H), generator=g).float()
    if L >= 2:
        c = torch.arange(H)
        big = c % L
        neg = (big + 1 + (c // L) % (L - 1)) % L
        x[big, c] = BIG
        x[neg, c] = -BIG
    return x


def _layout(H, lens, seed, gap=3):
    """Segments of ``lens`` rows behind `gap` NaN rows each (decode rows, generation prompts), NaN
    padding behind the last: x bf16 [T, H] on the CPU and the segments' (r0, r1)."""
    parts, spans, t = [], [], 0
    for i, L in enumerate(lens):
        parts.append(torch.full((gap + i % 2, H), float("nan")))
        t += gap + i % 2
        parts.append(_order_rows(L, H, seed + i))
        spans.append((t, t + L))
        t += L
    parts.append(torch.full((2, H), float("nan")))
    return torch.cat(parts).to(torch.bfloat16), spans


def _accumulate(x, seg, acc):
    ops.pool_accumulate(x, seg, acc)
    return acc


@pytest.mark.parametrize("H", HS)
def test_mean_is_the_sequential_sum_in_any_layout(gpu, H):
    x, spans = _layout(H, LENS, seed=H)
    slots = [4, 0, 7, 2, 8, 5]  # 1, 3 and 6 are named by no segment
    seg = [(r0, r1, s, POOL_INIT) for (r0, r1), s in zip(spans, slots)]
    acc0 = torch.full((SLOTS, H), float("nan"))  # init: a stale slot (NaN) is overwritten, not added to
    for s in (1, 3, 6):
        acc0[s] = SENTINEL
    want, _ = pool_reference(x, seg, acc0)
    got = _accumulate(x.to(gpu), _i32(seg, gpu), acc0.to(gpu)).cpu()
    assert not torch.isnan(want[slots]).any()
    # the probe does depend on the order: the sequential fp32 sum of the 300-row segment is not the
    # exact sum (the terms between +2^24 and -2^24 were rounded away), which a reordered sum keeps
    a, b = spans[-1]
    assert not torch.equal(x[a:b].double().sum(0), want[slots[-1]].double())
    assert torch.equal(got, want)
    assert (got[[1, 3, 6]] == SENTINEL).all()


@pytest.mark.parametrize("H", HS)
def test_without_init_the_stored_value_is_the_first_term(gpu, H):
    x, spans = _layout(H, (17, 2), seed=3)
    g = torch.Generator().manual_seed(1)
    acc0 = torch.randn(SLOTS, H, generator=g) * 3
    seg = [(*spans[0], 5, 0), (*spans[1], 2, POOL_LAST)]
    want, _ = pool_reference(x, seg, acc0)
    assert not torch.equal(want[5], pool_reference(x, [(*spans[0], 5, POOL_INIT)], acc0)[0][5])
    got = _accumulate(x.to(gpu), _i32(seg, gpu), acc0.to(gpu)).cpu()
    assert torch.equal(got, want)


@pytest.mark.parametrize("L", (17, 300))
@pytest.mark.parametrize("H", HS)
def test_chunking_changes_no_bit(gpu, H, L):
    """One launch, 1 | rest, rest | 1, two halves, 16-row pieces: the accumulator and the finished
    vector are the same bits, and those of the reference."""
    x, ((r0, r1),) = _layout(H, (L,), seed=11)
    xd = x.to(gpu)
    cuts = {"whole": [], "1|rest": [1], "rest|1": [L - 1], "middle": [L // 2], "16s": list(range(16, L, 16))}
    fin = [(3, L, H, POOL_FIN_MEAN | POOL_FIN_NORMALIZE)]
    want_acc, _ = pool_reference(x, [(r0, r1, 3, POOL_INIT)], torch.zeros(SLOTS, H))
    res = {}
    for name, cut in cuts.items():
        acc = torch.full((SLOTS, H), float("nan"), device=gpu)
        edges = [0, *cut, L]
        for i, (a, b) in enumerate(zip(edges, edges[1:])):
            flags = (POOL_INIT if i == 0 else 0) | (POOL_LAST if b == L else 0)
            ops.pool_accumulate(xd, _i32([(r0 + a, r0 + b, 3, flags)], gpu), acc)
        out = torch.zeros(SLOTS, H, device=gpu)
        ops.pool_finish(acc, _i32(fin, gpu), out)
        res[name] = (acc[3].cpu(), out[3].cpu())
    for name, (acc, out) in res.items():
        assert torch.equal(acc, want_acc[3]), name
        assert torch.equal(out, res["whole"][1]), name


@pytest.mark.parametrize("H", HS)
def test_last_copies_exactly_the_last_row(gpu, H):
    """Every row carries its own index (low byte in the even columns, high byte in the odd ones);
    a chunk that is not the sequence's last leaves its slot alone."""
    lens = LENS
    T = sum(lens) + 8
    r = torch.arange(T)
    x = torch.stack([(r & 255).float(), (r >> 8).float()], 1).repeat(1, H // 2).to(torch.bfloat16)
    spans, t = [], 5
    for L in lens:
        spans.append((t, t + L))
        t += L
    seg = [(r0, r1, s, POOL_MODE_LAST | POOL_LAST | (POOL_INIT if s % 2 else 0)) for s, (r0, r1) in enumerate(spans)]
    seg.append((5, 40, 7, POOL_MODE_LAST))              # not the last chunk: nothing, whatever the slot holds
    seg.append((5, 40, 8, POOL_MODE_LAST | POOL_INIT))  # ... also on the sequence's first chunk
    acc0 = torch.full((SLOTS, H), SENTINEL)
    got = _accumulate(x.to(gpu), _i32(seg, gpu), acc0.to(gpu)).cpu()
    for s, (r0, r1) in enumerate(spans):
        assert (got[s, 0::2] == ((r1 - 1) & 255)).all() and (got[s, 1::2] == ((r1 - 1) >> 8)).all(), (s, r0, r1)
    assert (got[6:] == SENTINEL).all()
    assert torch.equal(got, pool_reference(x, seg, acc0)[0])


def _dims(H):
    return sorted({d for d in (32, 100, 1024, H) if d <= H})


@pytest.mark.parametrize("normalize", (True, False), ids=("unit", "raw"))
@pytest.mark.parametrize("H", HS)
def test_finish(gpu, H, normalize):
    """mean (count = the sequence's tokens) and last vectors, cut to d, normalised or not; a zero row
    stays zero; columns from d on and other slots keep what they held; relaunches repeat every bit."""
    g = torch.Generator().manual_seed(H)
    x = (torch.randn(317, H, generator=g) * 2).to(torch.bfloat16)
    seg = [(0, 300, 0, POOL_INIT | POOL_LAST), (300, 317, 1, POOL_INIT | POOL_LAST),
           (0, 300, 2, POOL_MODE_LAST | POOL_LAST)]
    acc0 = torch.full((SLOTS, H), SENTINEL)
    acc0[:3] = float("nan")
    acc0[4] = 0.0
    acc_ref, _ = pool_reference(x, seg, acc0)
    acc = _accumulate(x.to(gpu), _i32(seg, gpu), acc0.to(gpu))
    assert torch.equal(acc.cpu(), acc_ref)
    nf = POOL_FIN_NORMALIZE if normalize else 0
    for d in _dims(H):
        fin = [(0, 300, d, POOL_FIN_MEAN | nf), (1, 17, d, POOL_FIN_MEAN | nf), (2, 300, d, nf),
               (4, 5, d, POOL_FIN_MEAN | nf)]
        _, want = pool_reference(x, [], acc_ref, fin)
        outs = []
        for _ in range(3):
            out = torch.full((SLOTS, H), SENTINEL, device=gpu)
            ops.pool_finish(acc, _i32(fin, gpu), out)
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
        got = outs[0].double()
        assert (got[4, :d] == 0).all() and not torch.isnan(got).any()
        for s in (0, 1, 2):
            w = want[s, :d]
            nz = w != 0
            err = ((got[s, :d] - w).abs()[nz] / w.abs()[nz]).max()
            print(f"H {H} d {d} slot {s} normalize {normalize}: max rel err {float(err):.3e}")
            assert float(err) <= 1e-5
            assert (got[s, :d][~nz] == 0).all()
            if normalize:
                assert abs(float(got[s, :d].square().sum().sqrt()) - 1) < 1e-5
        assert (got[:, d:] == SENTINEL).all() and (got[[3, 5, 6, 7, 8]] == SENTINEL).all()
