"""Attention probes: inputs for which the set of visible keys, and the key whose V row reaches
the output, are exact, so a check on them does not weaken as the context grows (a random-input
check at atol = rtol = 2e-2 cannot see one wrong key among ~1000: profiles/attention_probes.md).

Counting probe (WHICH keys are visible).  Q = 0, so every visible key weighs exactly 1/n_vis;
live key j of a row holds V[j, d] = 1 if j % 128 == d else 0 (K random), so
    expected[d] = #{visible j = d (mod 128)} / n_vis        (fp64, rounded once to bf16).
In the kernels every p is exp2(0) = 1, l and O are small integers (exact in fp32); the only
roundings are the reciprocal-multiply and the final bf16: one bf16 ulp.  One key too many, too
few or doubled moves a channel by 1 / count_d: at least 1/12 relative at 1500 keys.

Needle probe (WHICH V goes with which K; the running max and its rescale).  K entries are +-1,
V is randn (magnitudes >= 2^-6), the query of (row, token, head) is 4 K[target]: the target
scores 512 / sqrt(128) = 45.25, every other key N(0, 16).  The builder asserts, on the exact scores, that the target
beats every other visible key by >= MARGIN nats and that the leaked weight cannot move any
element of V[target] by a quarter ulp, so expected = V[target] under the same tolerance.

Dead slots (the slots of a row's last page past ctx_len and one whole extra page listed in the
block table behind the context) hold V = 64 and, in the needle probe, K = 2 K[target of the
row's last query]: finite (the kernels' contract for masked slots), but one key read too far
drags the output towards 64.  Pages that must never be touched - below a windowed row's first
visible page pair, and the never-handed-out page NB - 1 - are NaN, and the block-table entries
of the former are out-of-range ids.

Tolerance of both probes: an element whose expected value is 0 must be exactly 0; the others
|out - expected| <= 2^-7 |expected| (one bf16 ulp), no absolute term.

Plain module (imported by the probe test files), no fixtures, no pytest settings."""
import math

import numpy as np
import torch

bf = torch.bfloat16
D, BS = 128, 16
RTOL = 2.0 ** -7         # one bf16 ulp
MARGIN = 20.0            # nats between the needle's target and every other visible key
DEAD_V = 64.0
SCHEDULES = ("diag", "prev", "first", "random")


class Meta:
    pass


# ------------------------------------------------------------------ layout --

def assign_pages(bt, rows, q_lens, ctx_lens, window, NB, rng):
    """Block-table rows ``rows`` of ``bt`` (numpy [R, MB], in place) over a random assignment of
    the pages 1 .. NB - 2: the pages of the context, then ONE extra (dead) page.  Windowed: the
    entries below the page pair of the row's first query's first visible key become out-of-range
    ids; their pages are returned (with NB - 1) as the pages to fill with NaN."""
    need = sum((c + BS - 1) // BS + 1 for c in ctx_lens if c > 0)
    assert need <= NB - 2 and bt.shape[1] >= max((c + BS - 1) // BS + 1 for c in ctx_lens)
    pages = rng.permutation(np.arange(1, NB - 1))
    nan_pages, p = [NB - 1], 0
    for r, ql, c in zip(rows, q_lens, ctx_lens):
        bt[r] = 0
        if c <= 0:
            continue
        n = (c + BS - 1) // BS + 1
        bt[r, :n] = pages[p:p + n]
        p += n
        first = ((max(0, c - ql - window + 1) & ~31) >> 4) if window > 0 else 0
        nan_pages += bt[r, :first].tolist()
        bt[r, :first] = NB + 1000 + np.arange(first)
    return np.asarray(nan_pages, np.int64)


def num_pages(ctx_lens):
    """Pages a probe over these contexts needs: context + dead page per row, page 0 (where the
    unused block-table entries point) and the NaN page NB - 1."""
    return sum((c + BS - 1) // BS + 1 for c in ctx_lens if c > 0) + 2


def repartition(m, part_tokens=None, nparts=1, sem=False):
    """A copy of ``m`` with another split-KV form (None: one partition over the longest context)
    and its own partial buffers; ``sem``: zeroed tickets for the in-launch combine."""
    n = Meta()
    n.__dict__.update(m.__dict__)
    if part_tokens is None:
        part_tokens, nparts = (max(32, int(m.host["ctx_len"].max())) + 31) // 32 * 32, 1
    dev, nt = m.block_tables.device, max(1, m.tile_seq.numel())
    n.part_tokens, n.nparts = part_tokens, nparts
    n.part_o = torch.full((nt * m.Hkv * nparts * 16 * D,), float("nan"), device=dev)
    n.part_ml = torch.full((nt * m.Hkv * nparts * 16 * 2,), float("nan"), device=dev)
    if sem:
        n.part_sem = torch.zeros(nt * m.Hkv, dtype=torch.int32, device=dev)
    return n


def make_layout(q_lens, ctx_lens, Hkv, G, window=0, flash_min_q=1 << 30, part_tokens=None, nparts=1,
                device="cpu", seed=0):
    """The launch metadata of rows (q_len, ctx_len) in make_meta's conventions: shuffled pages,
    shuffled rows among three spare ones, decode tiles of 16/G tokens, flash tiles (128/G tokens,
    latest first) for rows of >= flash_min_q tokens; ctx 0 rows are graph padding."""
    rng = np.random.RandomState(seed)
    S = len(q_lens)
    R = S + 3
    rows = rng.permutation(R)[:S]
    MB = max((c + BS - 1) // BS for c in ctx_lens) + 1
    NB = num_pages(ctx_lens)
    bt = np.zeros((R, MB), np.int32)
    nan_pages = assign_pages(bt, rows, q_lens, ctx_lens, window, NB, rng)
    q_start, q_len, ctx = (np.zeros(R, np.int32) for _ in range(3))
    qt, pqt = 16 // G, 128 // G
    ts, tq, pts, ptq = [], [], [], []
    t = 0
    for r, ql, c in zip(rows, q_lens, ctx_lens):
        q_start[r], q_len[r], ctx[r] = t, ql, c
        if ql >= flash_min_q and G <= 8:
            k = (ql + pqt - 1) // pqt
            pts += [r] * k
            ptq += list(range((k - 1) * pqt, -1, -pqt))
        else:
            k = (ql + qt - 1) // qt
            ts += [r] * k
            tq += list(range(0, k * qt, qt))
        t += ql
    m = Meta()
    d = lambda a: torch.tensor(np.asarray(a, np.int32), dtype=torch.int32, device=device)  # noqa: E731
    m.block_tables, m.q_start, m.q_len, m.ctx_len = d(bt), d(q_start), d(q_len), d(ctx)
    m.tile_seq, m.tile_q0, m.ptile_seq, m.ptile_q0 = d(ts), d(tq), d(pts), d(ptq)
    m.window, m.Hkv, m.G, m.NB, m.num_tokens = window, Hkv, G, NB, t
    m.host = dict(bt=bt, q_start=q_start, q_len=q_len, ctx_len=ctx, rows=np.asarray(rows), nan_pages=nan_pages)
    return repartition(m, part_tokens, nparts)


# -------------------------------------------------------------------- data --

def round_bf16(x):
    """fp64 numpy -> the nearest bf16 (ties to even), ONE rounding; returned as fp64."""
    mant, e = np.frexp(x)
    return np.ldexp(np.rint(mant * 256.0), e - 8)


def _slots(bt, rows, q_len, ctx, window):
    """Every readable slot of the live rows, flat: (row, key position j, page, slot, live, row's
    offset into the flat arrays, row's first readable position)."""
    pages = (ctx[rows] + BS - 1) // BS + 1
    first = np.zeros(len(rows), np.int64)
    if window > 0:  # the page pair of the first query's first visible key; below it: NaN pages
        first = np.maximum(0, ctx[rows] - q_len[rows] - window + 1) & ~31
    lens = pages * BS - first
    off = np.concatenate([[0], np.cumsum(lens)])
    row_i = np.repeat(np.arange(len(rows)), lens)
    j = np.arange(off[-1]) - off[row_i] + first[row_i]
    page = bt[rows[row_i], j // BS]
    return row_i, j, page, j % BS, j < ctx[rows[row_i]], off, first


def _tokens(rows, q_start, q_len, ctx, window):
    """Every query token of the live rows, flat: (row index, token index into q, position, first
    visible key)."""
    row_i = np.repeat(np.arange(len(rows)), q_len[rows])
    qi = np.arange(len(row_i)) - np.concatenate([[0], np.cumsum(q_len[rows])])[row_i]
    pos = ctx[rows[row_i]] - q_len[rows[row_i]] + qi
    lo = np.maximum(0, pos - window + 1) if window > 0 else np.zeros_like(pos)
    return row_i, q_start[rows[row_i]] + qi, pos, lo


def counting_expected(pos, lo):
    """[n, 128] fp64: #{lo <= j <= pos, j % 128 == d} / (pos - lo + 1); 0 where nothing is visible."""
    d = np.arange(D)[None, :]
    below = lambda x: np.maximum(0, (x[:, None] - d + D - 1) // D)  # noqa: E731  #{0 <= j < x, j % 128 == d}
    cnt = below(pos + 1) - below(lo)
    n_vis = np.maximum(pos - lo + 1, 0)
    assert (cnt.sum(1) == n_vis).all()
    return cnt / np.maximum(n_vis, 1)[:, None].astype(np.float64)


def needle_targets(schedule, pos, lo, Hkv, G, rng):
    """[n, Hq] key positions.  diag: pos; prev: pos - 1; first: the first visible key; random: a
    different key for every head of a group (the R % G / R / G row mapping of the kernels)."""
    n, n_vis = len(pos), np.maximum(pos - lo + 1, 1)
    if schedule == "diag":
        t = pos
    elif schedule == "prev":
        t = np.maximum(pos - 1, lo)
    elif schedule == "first":
        t = lo
    else:
        assert schedule == "random", schedule
        base = rng.randint(0, 1 << 30, size=(n, Hkv, 1))
        step = np.maximum(1, n_vis // G)[:, None, None]
        t = lo[:, None, None] + (base + np.arange(G)[None, None, :] * step) % n_vis[:, None, None]
        return t.reshape(n, Hkv * G)
    return np.repeat(t[:, None], Hkv * G, 1)


def make_data(kind, host, Hkv, G, window, NB, num_tokens, device="cpu", seed=0, schedule="diag"):
    """q, k_cache, v_cache, expected of probe ``kind`` ("count" / "needle") laid out from the
    block tables of ``host`` (numpy: bt, q_start, q_len, ctx_len, rows = the launch's rows,
    nan_pages)."""
    rng = np.random.RandomState(seed + 1)
    gen = torch.Generator().manual_seed(seed + 1)
    bt, q_start, q_len, ctx = (np.asarray(host[k], np.int64) for k in ("bt", "q_start", "q_len", "ctx_len"))
    rows = np.unique(np.asarray(host["rows"], np.int64))
    Hq = Hkv * G
    live_rows = rows[ctx[rows] > 0]
    row_i, j, page, slot, live, off, first = _slots(bt, live_rows, q_len, ctx, window)
    assert ((page >= 1) & (page < NB - 1)).all(), "a readable slot on a page that is not the row's"
    N = len(j)
    page_t, slot_t, live_t = torch.from_numpy(page), torch.from_numpy(slot), torch.from_numpy(live)
    trow_i, tok, pos, lo = _tokens(rows, q_start, q_len, ctx, window)   # padding rows: pos = -1
    # index of the live rows among `rows`, to find a token's keys in the flat slot arrays
    live_of = np.full(len(rows), -1)
    live_of[ctx[rows] > 0] = np.arange(len(live_rows))
    tl = live_of[trow_i]
    vc = torch.full((NB, Hkv, BS, D), DEAD_V, dtype=bf)
    expected = torch.zeros(num_tokens, Hq, D, dtype=bf)
    if kind == "count":
        kc = torch.randn(NB, Hkv, BS, D, generator=gen).to(bf)
        vals = torch.full((N, D), DEAD_V, dtype=bf)
        vals[live_t] = torch.eye(D, dtype=bf)[torch.from_numpy(j[live] % D)]
        vc[page_t, :, slot_t] = vals[:, None, :].expand(N, Hkv, D)
        q = torch.zeros(num_tokens, Hq, D, dtype=bf)
        e = torch.from_numpy(round_bf16(counting_expected(pos, lo))).to(bf)
        expected[torch.from_numpy(tok)] = e[:, None, :].expand(len(tok), Hq, D)
    else:
        assert kind == "needle", kind
        pm1 = lambda *s: (torch.randint(0, 2, s, generator=gen) * 2 - 1).float()  # noqa: E731
        kc = pm1(NB, Hkv, BS, D)
        # (randn, its magnitudes kept >= 2^-6: a relative tolerance needs V[target] off zero, and
        # the generator does return an exact 0 now and then)
        Vl = torch.randn(N, Hkv, D, generator=gen)
        Kl, Vl = pm1(N, Hkv, D), torch.where(Vl < 0, Vl.clamp_max(-2.0 ** -6), Vl.clamp_min(2.0 ** -6)).to(bf)
        q = 4 * pm1(num_tokens, Hq, D)                    # (padding rows: any finite query)
        ok = tl >= 0
        tgt = needle_targets(schedule, pos[ok], lo[ok], Hkv, G, rng)            # [n, Hq]
        flat = torch.from_numpy(off[tl[ok]][:, None] + tgt - first[tl[ok]][:, None])  # into Kl / Vl
        kvh = torch.arange(Hq) // G
        q[torch.from_numpy(tok[ok])] = 4 * Kl[flat, kvh[None, :]]
        expected[torch.from_numpy(tok[ok])] = Vl[flat, kvh[None, :]]
        # dead slots: twice the K of the target of the row's last query (its group's first head)
        last = np.zeros(len(live_rows), np.int64)
        last[tl[ok]] = np.arange(ok.sum())                 # tokens ascend inside a row: the last wins
        dead_k = 2 * Kl[flat[torch.from_numpy(last)][:, ::G], torch.arange(Hkv)[None, :]]   # [rows, Hkv, D]
        Kd = torch.where(live_t[:, None, None], Kl, dead_k[torch.from_numpy(row_i)])
        Vd = torch.where(live_t[:, None, None], Vl, torch.tensor(DEAD_V, dtype=bf))
        kc[page_t, :, slot_t] = Kd
        vc[page_t, :, slot_t] = Vd
        _needle_conditions(Kl, Vl, q, live, off, first, ctx, live_rows, q_start, q_len, window, tgt,
                           tl[ok], G)
        kc, q = kc.to(bf), q.to(bf)
    nan = torch.from_numpy(np.asarray(host["nan_pages"], np.int64))
    kc[nan], vc[nan] = float("nan"), float("nan")
    return q.to(device), kc.to(device), vc.to(device), expected.to(device)


def _needle_conditions(Kl, Vl, q, live, off, first, ctx, live_rows, q_start, q_len, window, tgt, tl, G):
    """Conditions on the needle probe's INPUTS (not on any kernel): on the exact scores (K = +-1
    and q = +-4 give integer dot products, exact in fp32; scaled in fp64) every target beats every
    other visible key by >= MARGIN nats, and the weight that leaks to the other keys moves no
    element of V[target] by a quarter of a bf16 ulp."""
    inv = 1.0 / math.sqrt(D)
    vlive = Vl[torch.from_numpy(live)].double().abs()
    vmax, vmin = float(vlive.max()), float(vlive.min())
    assert vmin > 0
    worst_margin, worst_leak, t0 = float("inf"), 0.0, 0
    for i, r in enumerate(live_rows):
        ql, c, f = int(q_len[r]), int(ctx[r]), int(first[i])
        if ql == 0:
            continue
        K = Kl[off[i]:off[i] + c - f].repeat_interleave(G, dim=1)               # [n, Hq, D] keys f .. c - 1
        qq = q[q_start[r]:q_start[r] + ql]                                        # [ql, Hq, D]
        dots = torch.einsum("qhd,khd->qhk", qq, K)                                # exact integers
        pos = torch.arange(c - ql, c)[:, None, None]
        keys = torch.arange(f, c)[None, None, :]
        hidden = keys > pos
        if window > 0:
            hidden = hidden | (keys <= pos - window)
        assert tl[t0] == i
        target = torch.from_numpy(tgt[t0:t0 + ql])[:, :, None]                    # [ql, Hq, 1]
        t0 += ql
        assert (torch.gather(dots, 2, target - f) == 4 * D).all(), "the target is not the query's key"
        assert not torch.gather(hidden.expand_as(dots), 2, target - f).any(), "a hidden target"
        dots = dots.masked_fill(hidden | (keys == target), float("-inf"))
        worst_margin = min(worst_margin, (4 * D - float(dots.max())) * inv)
        leak = torch.exp((dots - 4 * D) * inv).sum(-1, dtype=torch.float64)
        worst_leak = max(worst_leak, float(leak.max()))
    assert worst_margin >= MARGIN, f"needle margin {worst_margin:.2f} nats < {MARGIN}: pick another seed"
    assert worst_leak * 2 * vmax <= 2.0 ** -10 * vmin, (worst_leak, vmax, vmin)


def build(kind, q_lens, ctx_lens, Hkv=2, G=4, window=0, flash_min_q=1 << 30, part_tokens=None, nparts=1,
          device="cpu", seed=0, schedule="diag"):
    """meta, q, k_cache, v_cache, expected of one probe launch."""
    m = make_layout(q_lens, ctx_lens, Hkv, G, window, flash_min_q, part_tokens, nparts, device, seed)
    return (m,) + make_data(kind, m.host, Hkv, G, window, m.NB, m.num_tokens, device, seed, schedule)


# -------------------------------------------------------------- geometries --
# The launches of tests/test_probes_attention_gpu.py; tests/test_attention_probes_cpu.py runs the
# fp32 reference over the same ones.

PROBES = [("count", "diag")] + [("needle", s) for s in SCHEDULES]
HKV = 2
DECODE_G = [1, 2, 4, 8, 16]
FLASH_G = [1, 2, 4, 8]
WIN_DECODE_W, WIN_DECODE_G = [1, 16, 31, 32, 33, 100], [1, 4, 8]
WIN_FLASH_W = [1, 16, 33, 100]
FLASH_MIN_Q = 17


def decode_launch(G):
    """One decode / ragged launch: q_len 1 rows at every page, pair and partition edge and at 1500
    keys, short multi-token rows (the last one spans two tiles), a prompt of 40 on the decode
    tiles and two graph-padding rows (ctx 0)."""
    ctxs = [1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 1500]
    q_lens = [1] * len(ctxs) + [3, 5, 16 // G + 1, 40, 1, 1]
    return q_lens, ctxs + [35, 300, 260, 40, 0, 0]


# (part_tokens, nparts, in-launch combine); 47 x 32 >= 1500: every pair boundary a partition boundary
DECODE_FORMS = {"one": (None, 1, False), "reduce256": (256, 6, False), "fused256": (256, 6, True),
                "parts32": (32, 47, False)}
WIN_FORMS = ["one", "fused32", "fused64", "reduce32", "reduce64"]


def windowed_decode_launch(W):
    """test_sliding_window_gpu's decode rows (window starts off / on pair boundaries, contexts
    shorter than the window, padding rows, 5-token rows) and a row at 1500 keys."""
    ctxs = sorted({c for c in (1, W - 1, W, W + 1, 2 * W + 5, 300, 1500) if c >= 1})
    q_lens, ctx_lens = [1] * len(ctxs) + [1, 1], ctxs + [0, 0]
    for c in (5, W + 3, 2 * W + 5, 300):
        if c >= 5:
            q_lens.append(5)
            ctx_lens.append(c)
    return q_lens, ctx_lens


def windowed_form(form, W, G):
    """(part_tokens, nparts, in-launch combine) of a WIN_FORMS entry: partitions of 32 / 64 keys
    over the longest key span of a windowed tile, at least two."""
    if form == "one":
        return None, 1, False
    part = int(form[-2:])
    span = W + 31 + 16 // G - 1
    return part, max(2, (span + part - 1) // part), form.startswith("fused")


# fresh prompts with partial last tiles; a 300-token chunk ending at 1500 keys with a decode row
# in the same launch; one long prompt (many causal tiles)
FLASH_LAUNCHES = {"fresh": ([17, 40, 129, 200], [17, 40, 129, 200]),
                  "chunk": ([300, 1], [1500, 700]),
                  "long": ([1024], [1024])}


def windowed_flash_launch():
    q_lens, ctx_lens = [], []
    for ql in (17, 64, 200):
        for before in (0, 50):
            q_lens.append(ql)
            ctx_lens.append(before + ql)
    return q_lens, ctx_lens


# ------------------------------------------------------------------- check --

def mismatch(out, expected):
    """None if ``out`` meets the probes' tolerance, else a description of the worst element."""
    o, e = out.detach().double().cpu(), expected.detach().double().cpu()
    if o.shape != e.shape:
        return f"shape {tuple(o.shape)} != {tuple(e.shape)}"
    bad = ~torch.isfinite(o) | ((e == 0) & (o != 0)) | ((o - e).abs() > RTOL * e.abs())
    if not bad.any():
        return None
    err = torch.where(torch.isfinite(o), (o - e).abs() / e.abs().clamp_min(2.0 ** -126), torch.tensor(float("inf")))
    err = torch.where(bad, err, torch.zeros_like(err))
    t, h, d = np.unravel_index(int(err.argmax()), tuple(o.shape))
    return (f"{int(bad.sum())} of {bad.numel()} elements off ({int(bad.any(-1).sum())} (token, head) rows); worst at "
            f"token {t} head {h} channel {d}: got {float(o[t, h, d])!r}, expected {float(e[t, h, d])!r}")


def assert_probe(out, expected, what=""):
    msg = mismatch(out, expected)
    assert msg is None, f"{what}: {msg}" if what else msg
