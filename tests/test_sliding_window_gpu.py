"""Sliding-window attention kernels (windowed instantiations of the decode / ragged kernel and
of the flash-prefill kernel) against the fp32 reference attention.

Query i attends the keys i - W < j <= i.  In every case the pages below the page pair that
holds a sequence's first visible key are filled with NaN and their block-table entries point
at an out-of-range id: the kernels must SKIP them (block-table entry included), not only mask
them; the oracle is computed from the visible keys alone.  Pages inside the first visible pair
stay finite (masked lanes multiply p = 0 with what they hold)."""
import numpy as np
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref

pytestmark = pytest.mark.gpu
bf = torch.bfloat16
HKV, D = 2, 128
TOL = dict(atol=2e-2, rtol=2e-2)  # test_paged_attention's / test_flash_prefill's


class Meta:
    pass


def make_case(gpu, q_lens, ctx_lens, G, W, flash_min_q=1 << 30, part_tokens=None, nparts=1, seed=0):
    """Rows (q_len, ctx_len) over a random page assignment; ctx 0 rows are graph padding."""
    rng = np.random.RandomState(seed)
    torch.manual_seed(seed)
    S = len(q_lens)
    MB = max(1, max((c + 15) // 16 for c in ctx_lens))
    NB = sum((c + 15) // 16 for c in ctx_lens) + 3
    bad = NB - 1  # never handed out, NaN: where a clamped out-of-range id would land
    kc = torch.randn(NB, HKV, 16, D, device=gpu, dtype=bf)
    vc = torch.randn(NB, HKV, 16, D, device=gpu, dtype=bf)
    kc[bad], vc[bad] = float("nan"), float("nan")
    bt = np.zeros((S, MB), dtype=np.int32)
    pages = rng.permutation(np.arange(1, NB - 1))
    p = 0
    qt, pqt = 16 // G, 128 // G
    ts, tq, pts, ptq = [], [], [], []
    q_start = np.zeros(S, np.int32)
    t = 0
    for r, (ql, c) in enumerate(zip(q_lens, ctx_lens)):
        n = (c + 15) // 16
        bt[r, :n] = pages[p:p + n]
        p += n
        # below the pair of the row's first query's first visible key: NaN pages, wild ids
        first = ((max(0, c - ql - W + 1) & ~31) >> 4) if (W > 0 and c > 0) else 0
        for j in range(first):
            kc[bt[r, j]], vc[bt[r, j]] = float("nan"), float("nan")
            bt[r, j] = NB + 1000 + j
        q_start[r] = t
        if ql >= flash_min_q:
            k = (ql + pqt - 1) // pqt
            pts += [r] * k
            ptq += list(range((k - 1) * pqt, -1, -pqt))
        else:
            k = (ql + qt - 1) // qt
            ts += [r] * k
            tq += list(range(0, k * qt, qt))
        t += ql
    m = Meta()
    d = lambda a: torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device=gpu)  # noqa: E731
    m.block_tables, m.q_start, m.q_len, m.ctx_len = d(bt), d(q_start), d(q_lens), d(ctx_lens)
    m.tile_seq, m.tile_q0, m.ptile_seq, m.ptile_q0 = d(ts), d(tq), d(pts), d(ptq)
    if part_tokens is None:  # one partition over the longest key span of a tile
        part_tokens, nparts = (max(ctx_lens) + 31) // 32 * 32, 1
    m.part_tokens, m.nparts, m.window = part_tokens, nparts, W
    m.part_o = torch.empty(max(1, len(ts)) * HKV * nparts * 16 * 128, device=gpu)
    m.part_ml = torch.empty(max(1, len(ts)) * HKV * nparts * 16 * 2, device=gpu)
    q = torch.randn(t, HKV * G, D, device=gpu, dtype=bf)
    return m, q, kc, vc


def decode_rows(W):
    ctxs = sorted({c for c in (1, W - 1, W, W + 1, 2 * W + 5, 300) if c >= 1})
    q_lens = [1] * len(ctxs) + [1, 1]          # ... and two graph-padding rows (ctx 0)
    ctx_lens = ctxs + [0, 0]
    # short rows of 5 queries: rows of one tile with different window starts
    for c in (5, W + 3, 2 * W + 5, 300):
        if c >= 5:
            q_lens.append(5)
            ctx_lens.append(c)
    return q_lens, ctx_lens


FORMS = ["one", "fused32", "fused64", "reduce32", "reduce64"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("W", [1, 16, 31, 32, 33, 100])
def test_windowed_decode(gpu, attn_fused_all, W, G, form):
    """Window starts off a pair boundary, in the second page of a pair, exactly on a boundary;
    contexts shorter than the window; padding rows; as one partition, split over partitions
    counted from the window start with the in-launch combine, and with the reduce launch."""
    q_lens, ctx_lens = decode_rows(W)
    kw = {}
    if form != "one":
        part = int(form[-2:])
        span = W + 31 + 16 // G - 1          # the longest key span of a tile
        kw = dict(part_tokens=part, nparts=max(2, (span + part - 1) // part))  # (>= 2: the split path)
    m, q, kc, vc = make_case(gpu, q_lens, ctx_lens, G, W, **kw)
    exp = ref.paged_attention(q, kc, vc, m)
    assert torch.isfinite(exp).all()
    if form.startswith("fused"):
        m.part_sem = torch.zeros(m.tile_seq.numel() * HKV, dtype=torch.int32, device=gpu)
    outs = []
    for _ in range(1 if form == "one" else 2):
        out = torch.full_like(q, float("nan"))
        ops.paged_attention(q, kc, vc, m, out=out)
        torch.testing.assert_close(out.float(), exp.float(), **TOL)
        outs.append(out)
        if form.startswith("fused"):
            assert int(m.part_sem.abs().sum()) == 0  # tickets re-armed
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1])
    pad = [i for i, c in enumerate(ctx_lens) if c == 0]
    assert (out[m.q_start[pad].long()] == 0).all()


def test_short_context_equals_no_window(gpu):
    """A context no longer than the window gives the no-window result."""
    G, W = 4, 100
    m, q, kc, vc = make_case(gpu, [1, 1, 5, 1], [1, 99, 100, 64], G, W)
    out_w = ops.paged_attention(q, kc, vc, m)
    m.window = 0
    torch.testing.assert_close(out_w.float(), ref.paged_attention(q, kc, vc, m).float(), **TOL)


@pytest.mark.parametrize("G", [1, 4, 8])
@pytest.mark.parametrize("W", [1, 16, 33, 100])
def test_windowed_flash(gpu, W, G):
    """Flash tiles of fresh prompts and of a later chunk (50 earlier tokens): windows smaller
    than a tile's token span (rows whose first visited pair is wholly masked), key ranges of 1,
    2 and >= 4 pairs, ring starts on every pair index mod 3."""
    q_lens, ctx_lens = [], []
    for ql in (17, 64, 200):
        for before in (0, 50):
            q_lens.append(ql)
            ctx_lens.append(before + ql)
    m, q, kc, vc = make_case(gpu, q_lens, ctx_lens, G, W, flash_min_q=17)
    assert m.ptile_seq.numel() > 0 and m.tile_seq.numel() == 0
    exp = ref.paged_attention(q, kc, vc, m)
    assert torch.isfinite(exp).all()
    out = torch.full_like(q, float("nan"))
    ops.paged_attention(q, kc, vc, m, out=out)
    torch.testing.assert_close(out.float(), exp.float(), **TOL)


def test_windowed_flash_ignores_persistent_grids(gpu):
    """With a window the launcher takes the plain grid whatever flash_persist / flash_stream say."""
    m, q, kc, vc = make_case(gpu, [200, 64, 200], [250, 64, 200], 4, 33, flash_min_q=17)
    exp = ops.paged_attention(q, kc, vc, m)
    prev, prev_s = torch.ops.mlop.flash_persist(-1), torch.ops.mlop.flash_stream(-1)
    try:
        torch.ops.mlop.flash_persist(64)
        torch.ops.mlop.flash_stream(1)
        assert torch.equal(ops.paged_attention(q, kc, vc, m), exp)
    finally:
        torch.ops.mlop.flash_persist(prev)
        torch.ops.mlop.flash_stream(prev_s)


def test_window_zero_is_the_unwindowed_op(gpu):
    """window = 0 selects the same kernels as the ops called without the argument."""
    scale = 1.0 / D ** 0.5
    m, q, kc, vc = make_case(gpu, [1, 1, 3], [700, 33, 300], 4, 0, part_tokens=128, nparts=6)
    sem = torch.zeros(m.tile_seq.numel() * HKV, dtype=torch.int32, device=gpu)
    args = (m.part_o, m.part_ml, sem, q, kc, vc, m.block_tables, m.tile_seq, m.tile_q0, m.q_start, m.q_len,
            m.ctx_len, scale, m.part_tokens, m.nparts)
    a, b = torch.zeros_like(q), torch.zeros_like(q)
    torch.ops.mlop.paged_attention(a, *args)
    torch.ops.mlop.paged_attention(b, *args, 0)
    assert torch.equal(a, b)
    m, q, kc, vc = make_case(gpu, [200, 64], [250, 64], 4, 0, flash_min_q=17)
    args = (q, kc, vc, m.block_tables, m.ptile_seq, m.ptile_q0, m.q_start, m.q_len, m.ctx_len, scale)
    a, b = torch.zeros_like(q), torch.zeros_like(q)
    torch.ops.mlop.flash_prefill(a, *args)
    torch.ops.mlop.flash_prefill(b, *args, 0)
    assert torch.equal(a, b)
    torch.testing.assert_close(a.float(), ref.paged_attention(q, kc, vc, m).float(), **TOL)
