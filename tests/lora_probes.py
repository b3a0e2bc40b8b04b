"""Exact probes for the multi-LoRA kernels of mlopamd/ops/csrc/lora.hip: ``lora_shrink`` in every
form of its K loop and ``lora_expand_add`` at every R, with tiles that mix up to 16 slots.

Every probe takes a back end (``HipBackend``: the raw ops; ``RefBackend``: the CPU definitions of
mlopamd.ops; ``Faulty``: a plain-torch restatement of the two kernels that carries the fault table)
and returns a list of failure messages, empty when the back end passes.  All data are integers,
powers of two or single products, so every expectation is ONE value, computed in fp64 and asserted
to be exact in fp32, and "equal" means the same bits (fp32 for ``tmp``, bf16 for ``y``; the sign of
a zero is ignored: torch's ``!=``).  No tolerance and no measured number is used anywhere.
``x``, ``tmp`` and ``y`` are the first T rows of buffers with PAD sentinel rows behind them; ``tmp``
is prefilled.  Inputs are drawn or built on the CPU, so the builders' conditions hold for the very
tensors a device gets.  profiles/lora_probes.md has the reasoning, the case tables, the fault table
and the measured results.
"""
import collections

import torch

from gemm_probes import PAD, SENTINEL, _gen, describe, sentinel_bad
from row_probes import PLANT_ROUNDED, PLANTS

bf = torch.bfloat16
NAN, INF = float("nan"), float("inf")
S = 17                     # slots of every adapter stack: one tile can hold 16 distinct ones
U = 4                      # lora.hip: K steps in flight per wave
I32_MAX, I32_MIN = 2 ** 31 - 1, -2 ** 31
OUT_OF_RANGE = (S, S + 5, I32_MAX, -2, I32_MIN)
# slot_rank of slot s (capped at R): every value of the list, 0 and the non-multiples of 16 included
RANKS = (0, 1, 8, 16, 17, 32, 33, 48, 64, 64, 48, 33, 32, 17, 16, 8, 64)
RANK_VALUES = (0, 1, 8, 16, 17, 32, 33, 48, 64)
ONE_SLOT, LAST_SLOT, POISON_SLOT = 9, 16, 5
VARIANTS = 4               # tile patterns rotate over the launches of a probe
TAIL_FILL = 5.0            # the columns behind a strided y
TS = (1, 15, 16, 17, 33)
GR_PAIRS = [(G, R) for G in (1, 2, 3) for R in (16, 32, 48, 64)]


# ------------------------------------------------------------- back ends --

class HipBackend:
    """The raw ops the wrappers of mlopamd.ops call."""

    def __init__(self, device):
        from mlopamd import ops

        self.ops, self.device = ops, device
        ops.load()

    def shrink(self, tmp, x, A, tok_slot, slot_rank, groups):
        torch.ops.mlop.lora_shrink(tmp, x, A, tok_slot, slot_rank, A.shape[1] // groups if groups else 16)

    def expand(self, y, tmp, B, tile_group, tok_slot, slot_rank):
        torch.ops.mlop.lora_expand_add(y, tmp, B, tile_group, tok_slot, slot_rank)


class RefBackend:
    """The CPU definitions of mlopamd.ops: what the probes must accept."""

    def __init__(self):
        from mlopamd import ops

        self.ops = ops

    def shrink(self, tmp, x, A, tok_slot, slot_rank, groups):
        tmp.copy_(self.ops.lora_shrink(x, A, tok_slot, slot_rank, groups=groups))

    def expand(self, y, tmp, B, tile_group, tok_slot, slot_rank):
        self.ops.lora_expand_add(y, tmp, B, tile_group, tok_slot, slot_rank)


def shrink_form(K):
    """(main-loop trips, drain, scalar tail steps) of one wave's K loop: a restatement of
    lora_shrink_kernel's control flow (steps = K / 128 per wave quarter, U = 4 in flight)."""
    steps = K // 128
    if steps < U:
        return (0, 0, steps)
    main = steps // U - 1
    return (main, 1, steps - (main + 1) * U)


def form_name(K):
    main, drain, tail = shrink_form(K)
    parts = ([f"{main} main"] if main else []) + (["drain"] if drain else []) + ([f"{tail} tail"] if tail else [])
    return " + ".join(parts)


def split3(v):
    """fp32 v -> (hi, mid, lo) bf16: the CPU restatement of lora.hip's lora_split3."""
    h = v.to(bf)
    r1 = v - h.float()
    m = r1.to(bf)
    return h, m, (r1 - m.float()).to(bf)


def _trunc(x):
    """fp32 -> bf16 by truncation."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(bf)


def _row_past(t):
    """The rows of a view buf[:T] and the one behind them (the buffer's first sentinel row)."""
    return torch.as_strided(t, (t.shape[0] + 1, t.shape[1]), t.stride(), t.storage_offset())


SHRINK_FAULTS = ["quarter_dropped", "last_tail_step_dropped", "group_used_twice", "prefetch_one_group_back",
                 "x_stride_k", "tmp_rounded_to_bf16", "no_slot_rows_unwritten", "rank_skip_rg_plus_16"]
SLOT_FAULTS = ["first_slots_product_for_all", "later_slots_ignored", "slot_modulo_s"]
EXPAND_FAULTS = ["loop_bound_k_plus_32", "upper_half_dropped", "upper_half_not_zeroed", "group_per_64_columns",
                 "group_always_0", "split_2_terms", "split_1_term", "delta_rounded_first", "truncating_store",
                 "no_slot_rows_rewritten"]
ALL_FAULTS = SHRINK_FAULTS + SLOT_FAULTS + EXPAND_FAULTS + ["row_t_written"]


class Faulty:
    """The two kernels restated in plain torch (fp64 sums of the same products, which the probes'
    data make exact), with one fault injected (None: no fault)."""

    def __init__(self, fault=None):
        assert fault is None or fault in ALL_FAULTS, fault
        self.fault = fault

    def _slots(self, tok_slot, n_slots):
        """Per token: the slot whose rows are multiplied (-1: none) and whether the token keeps the
        product (lora_lane_slot and lora_next_slot)."""
        f = self.fault
        ts = tok_slot.long()
        if f == "slot_modulo_s":
            ts = torch.where(ts >= n_slots, ts % n_slots, ts)
        ts = torch.where((ts < 0) | (ts >= n_slots), torch.full_like(ts, -1), ts)
        use, keep = ts.clone(), ts >= 0
        if f in ("first_slots_product_for_all", "later_slots_ignored"):
            for t0 in range(0, ts.numel(), 16):
                tile = ts[t0:t0 + 16]
                live = tile[tile >= 0]
                if not live.numel():
                    continue
                if f == "first_slots_product_for_all":
                    use[t0:t0 + 16] = torch.where(tile >= 0, live[0], tile)
                else:
                    keep[t0:t0 + 16] = tile == live[0]
        return ts, use, keep

    def _k_index(self, K):
        """The k columns one launch multiplies, in the order of the wave quarters and steps."""
        f = self.fault
        main, drain, tail = shrink_form(K)
        steps, full = K // 128, (main + drain) * U
        seq = list(range(steps))
        if f == "last_tail_step_dropped" and tail:
            seq = seq[:-1]
        elif f == "group_used_twice" and drain:      # the tail starts at the drained group
            seq = seq[:full] + seq[full - U:full] + seq[full:]
        elif f == "prefetch_one_group_back" and main:  # trip i refetches group i: g0 g0 g1 ...
            seq = seq[:U] + seq[:full - U] + seq[full:]
        idx = [q * (K // 4) + 32 * st + i for q in range(4) if not (f == "quarter_dropped" and q == 2)
               for st in seq for i in range(32)]
        return torch.tensor(idx, dtype=torch.long)

    def shrink(self, tmp, x, A, tok_slot, slot_rank, groups):
        f = self.fault
        T, K = x.shape
        GR = A.shape[1]
        if T == 0:
            return
        R = GR // groups if groups else 16
        if f == "x_stride_k":
            x = torch.as_strided(x, (T, K), (K, 1), x.storage_offset())
        ts, use, keep = self._slots(tok_slot, A.shape[0])
        idx = self._k_index(K)
        rg = (torch.arange(GR) // 16 * 16) % R
        out = torch.zeros(T, GR, dtype=torch.float64)
        for s in torch.unique(use[keep]).tolist():
            rows = keep & (use == s)
            rank = int(slot_rank[s])
            live = (rg + 16 <= rank) if f == "rank_skip_rg_plus_16" else (rg < rank)
            if bool(live.any()):
                out[rows.nonzero()[:, 0][:, None], live.nonzero()[:, 0][None, :]] = \
                    x[rows][:, idx].double() @ A[s][live][:, idx].double().t()
        out = out.float()
        if f == "tmp_rounded_to_bf16":
            out = out.to(bf).float()
        if f == "no_slot_rows_unwritten":
            out[ts < 0] = tmp[ts < 0]
        tmp.copy_(out)
        if f == "row_t_written":
            _row_past(tmp)[-1] = tmp[-1]

    def _col_weights(self, rank, R):
        """How often column r of a slot's B rows enters the sum (the expand's step loop)."""
        f = self.fault
        w = torch.zeros(R, dtype=torch.float64)
        k = 0
        while (k + 32 <= rank) if f == "loop_bound_k_plus_32" else (k < rank):
            w[k:min(k + (16 if f == "upper_half_dropped" else 32), R)] += 1
            if f == "upper_half_not_zeroed" and k + 32 > R:  # both chunks past the row are the row's first
                w[:8] += 2
            k += 32
        return w

    def expand(self, y, tmp, B, tile_group, tok_slot, slot_rank):
        f = self.fault
        T, N = y.shape
        R = B.shape[2]
        if T == 0:
            return
        G = tmp.shape[1] // R
        ts, use, keep = self._slots(tok_slot, B.shape[0])
        tg = tile_group.long()
        if f == "group_per_64_columns":
            tg = tg[torch.arange(N // 16) // 4 * 4]
        elif f == "group_always_0":
            tg = torch.zeros_like(tg)
        col_g = tg.clamp(max=G - 1).repeat_interleave(16)
        h, m, l = split3(tmp)
        terms = h.double() + (m.double() if f != "split_1_term" else 0) + \
            (l.double() if f not in ("split_1_term", "split_2_terms") else 0)
        acc = torch.zeros(T, N, dtype=torch.float64)
        for s in torch.unique(use[keep]).tolist():
            rows = (keep & (use == s)).nonzero()[:, 0]
            w = self._col_weights(min(int(slot_rank[s]), R), R)
            v = terms[rows].view(-1, G, R)[:, col_g]                       # [rows, N, R]
            on = w != 0
            acc[rows] = (v[:, :, on] * (B[s].double()[:, on] * w[on])[None]).sum(-1)
        delta = acc.float()
        if f == "delta_rounded_first":
            delta = delta.to(bf).float()
        s32 = y.float() + delta
        out = _trunc(s32) if f == "truncating_store" else s32.to(bf)
        write = torch.ones(T, dtype=torch.bool) if f == "no_slot_rows_rewritten" else ts >= 0
        y[write] = out[write]
        if f == "row_t_written":
            _row_past(y)[-1] = y[-1]


# ------------------------------------------------------------ slot patterns --

def _tile_pattern(kind, rot):
    """The 16 tok_slot entries of one tile: 16 distinct slots, runs of 2 or 3 slots between rows
    without one (-1 and every out-of-range value), no slot at all, one slot throughout."""
    if kind == 0:
        return [(5 * i + 3 + rot) % 16 for i in range(16)]
    if kind == 1:
        a, b, c, d = [(4 * rot + 1 + 3 * i) % 16 for i in range(4)]
        return [a, a, -1, b, b, b, S, c, c, S + 5, d, d, d, I32_MAX, -2, I32_MIN]
    return [-1] * 16 if kind == 2 else [ONE_SLOT] * 16


def tok_slots(T, variant):
    """tok_slot of a T-token launch: tile i has pattern (i + variant) % 4; the last, partial tile of
    a launch of several holds LAST_SLOT, which no pattern uses."""
    out = []
    for i in range(-(-T // 16)):
        out += _tile_pattern((i + variant) % 4, variant + i)
    out = out[:T]
    if T > 16 and T % 16:
        out[T // 16 * 16:] = [LAST_SLOT] * (T % 16)
    return out


def slot_ranks(R):
    return [min(r, R) for r in RANKS]


def valid(slots):
    return [0 <= s < S for s in slots]


def _meta(T, variant, R):
    """(slots list, tok_slot int32, slot_rank int32, per-token rank with -1 for no slot)."""
    slots = tok_slots(T, variant)
    ranks = slot_ranks(R)
    tr = [ranks[s] if 0 <= s < S else -1 for s in slots]
    return slots, torch.tensor(slots, dtype=torch.int64).to(torch.int32), torch.tensor(ranks, dtype=torch.int32), tr


def _padded(T, n, fill, dtype, extra=0, tail=None):
    """A [T + PAD, n + extra] buffer of ``fill`` (``tail`` in the extra columns) and its [:T, :n] view."""
    buf = torch.full((T + PAD, n + extra), fill, dtype=dtype)
    if extra:
        buf[:, n:] = tail
    return buf, buf[:T, :n]


def _msgs(*ms):
    return [m for m in ms if m]


def _count(info, key, n):
    info[key] = info.get(key, 0) + n


# ================================================================= shrink ==

ShrinkCase = collections.namedtuple("ShrinkCase", "id K T G R")
# the issue's K list plus 1408 and 1664: one main trip with 3 tail steps, several with 1
SHRINK_KS = (128, 384, 512, 640, 896, 1024, 1152, 1408, 1664, 1920, 4096, 14336)
CROSS_KS = (512, 1152)


def _shrink_cases():
    keys = [(K, 17, G, R) for K in SHRINK_KS for G, R in ((3, 64), (2, 48))]
    keys += [(K, 17, G, R) for K in CROSS_KS for G, R in GR_PAIRS]
    keys += [(K, T, G, R) for K in CROSS_KS for T in TS for G, R in ((3, 64), (1, 16))]
    return [ShrinkCase(f"shrink-K{K}-T{T}-G{G}-R{R}", K, T, G, R) for K, T, G, R in dict.fromkeys(keys)]


SHRINK_CASES = _shrink_cases()


def shrink_bytes(case):
    return S * case.G * case.R * case.K * 2


def selector_columns(K):
    """The k columns a selector probe must visit: all 8 positions of the first and of the last
    16-byte vector of every wave quarter, and one position of the first and of the last vector of
    every group of U steps inside a quarter."""
    kq, cols = K // 4, []
    for q in range(4):
        cols += [q * kq + i for i in range(8)] + [(q + 1) * kq - 8 + i for i in range(8)]
        for g0 in range(0, kq, 32 * U):
            g1 = min(g0 + 32 * U, kq)
            cols += [q * kq + g0 + (g0 // 8) % 8, q * kq + g1 - 8 + (g1 // 8 - 1) % 8]
    return list(dict.fromkeys(cols))


def _plan(T, R, wanted, fits):
    """Launches [(variant, {token: item})] that hand every wanted item to a token with a slot
    that ``fits(rank, item)``; every variant runs at least once.  Tokens left over (no slot, or
    none of the open items fits) take items in turn: they are checked all the same."""
    todo, plan, n, idle = list(wanted), [], 0, 0
    useful = set(range(VARIANTS))
    while todo or n < VARIANTS:
        variant = n % VARIANTS
        n += 1
        if n > VARIANTS and variant not in useful:
            assert useful, ("the plan cannot place", todo[:4])
            continue
        tr = _meta(T, variant, R)[3]
        give, before = {}, len(todo)
        for t in range(T):
            pick = next((w for w in todo if tr[t] >= 0 and fits(tr[t], w)), None)
            if pick is not None:
                todo.remove(pick)
            give[t] = pick if pick is not None else wanted[(n + 3 * t) % len(wanted)]
        if len(todo) == before and n <= VARIANTS:
            useful.discard(variant)
        idle = idle + 1 if len(todo) == before else 0
        assert idle <= 2 * VARIANTS, ("the plan cannot place", todo[:4])
        plan.append((variant, give))
    return plan


def shrink_selector_plan(case):
    return _plan(case.T, case.R, selector_columns(case.K), lambda rank, k: rank >= 1)


def code_a(n_slots, GR, K):
    """int32 [S, GR, K] codes in [-125, 126] without 0 that differ between neighbours in s, j and
    k, and between a k and the same place of the next step, group of steps and quarter."""
    s = torch.arange(n_slots, dtype=torch.int32)[:, None, None]
    j = torch.arange(GR, dtype=torch.int32)[None, :, None]
    k = torch.arange(K, dtype=torch.int32)[None, None, :]
    c = (s * 53 + j * 29 + (k * 7 + (k >> 5) * 13 + (k >> 7) * 31)) % 251 - 125
    return torch.where(c == 0, torch.full_like(c, 126), c)


def _zero_above_rank(W4, R):
    """W4 [S, G, R, *] (A) in place: rows at or above the slot's rank are zero."""
    for s, r in enumerate(slot_ranks(R)):
        W4[s, :, r:] = 0
    return W4


_LAST = {}


def _cached(key, build):
    """The adapter stack of the case in hand: built and moved to the device once per probe."""
    if _LAST.get("key") != key:
        _LAST.clear()
        _LAST.update(key=key, value=build())
    return _LAST["value"]


def selector_a(case):
    A = code_a(S, case.G * case.R, case.K)
    return _zero_above_rank(A.view(S, case.G, case.R, case.K), case.R).view(S, -1, case.K).to(bf)


def _run_shrink(case, be, device, A_dev, x, ts, sr, groups, strided):
    """One launch: x [T, K] into a NaN-padded buffer (a column slice of a wider one if strided),
    tmp prefilled.  Returns the CPU tmp buffer [T + PAD, G R]."""
    T = x.shape[0]
    xbuf, xv = _padded(T, case.K, NAN, bf, 8 if strided else 0, NAN)
    xv.copy_(x)
    xbuf = xbuf.to(device)
    tbuf = torch.full((T + PAD, case.G * case.R), SENTINEL, dtype=torch.float32, device=device)
    be.shrink(tbuf[:T], xbuf[:T, :case.K], A_dev, ts.to(device), sr.to(device), groups)
    return tbuf.cpu()


def probe_shrink_selector(case, be, device, info=None):
    """One-hot x rows: tmp[t, j] must be A[slot(t), j, k_t]."""
    info = {} if info is None else info
    K, T, GR = case.K, case.T, case.G * case.R
    A = selector_a(case)
    A_dev = A.to(device)
    msgs = []
    for n, (variant, give) in enumerate(shrink_selector_plan(case)):
        slots, ts, sr, tr = _meta(T, variant, case.R)
        kt = torch.tensor([give[t] for t in range(T)], dtype=torch.long)
        x = torch.zeros(T, K, dtype=bf)
        x[torch.arange(T), kt] = 1
        ok = torch.tensor(valid(slots))
        exp = torch.zeros(T, GR)
        exp[ok] = A[ts[ok].long(), :, kt[ok]].float()
        tbuf = _run_shrink(case, be, device, A_dev, x, ts, sr, case.G if n % 4 in (0, 3) else None, variant % 2 == 1)
        what = f"{case.id} selector launch {n}"
        bad = tbuf[:T] != exp
        if bool(bad.any()):
            t, j = (int(v) for v in bad.nonzero()[0])
            k = int(kt[t])
            msgs.append(f"{what}: token {t} row {j}: K step {k % (K // 4) // 32} of quarter {k // (K // 4)}, slot "
                        f"{slots[t]} (k = {k}): got {float(tbuf[t, j]):g}, expected {float(exp[t, j]):g}")
        msgs += _msgs(describe(what, bad, tbuf[:T], exp), sentinel_bad(what, tbuf, T))
        _count(info, "checked", T * GR)
        _count(info, "launches", 1)
        if len(msgs) > 4:
            break
    return msgs


def shrink_inputs(case):
    """CPU (x [VARIANTS, T, K], A [S, G R, K]) bf16 integers in [-4, 4].  Row 0 of every A block
    is 4 p[k] and x of every fourth token is p[k] |x| with |x| in {3, 4} and an odd sum of |x|:
    those sums are 4 (odd number) >= 1536, which is no bf16."""
    gen = _gen(case.id, "cpu")
    K, T, G, R = case.K, case.T, case.G, case.R
    x = torch.randint(-4, 5, (VARIANTS, T, K), generator=gen)
    A = torch.randint(-4, 5, (S, G, R, K), generator=gen, dtype=torch.int8)
    p = 1 - 2 * torch.randint(0, 2, (K,), generator=gen)
    A[:, :, 0] = (4 * p).to(torch.int8)
    mag = torch.randint(3, 5, (VARIANTS, -(-T // 4), K), generator=gen)
    mag[:, :, 0] = 3 + (mag[:, :, 1:].sum(-1) % 2 == 1)   # |x[0]| = 4 if the rest is odd: an odd total
    x[:, ::4] = mag * p
    _zero_above_rank(A, R)
    return x.to(bf), A.view(S, G * R, K).to(bf)


def shrink_expect(x, A, slots):
    """fp64 tmp [T, G R]: zero rows for tokens without a slot."""
    out = torch.zeros(x.shape[0], A.shape[1], dtype=torch.float64)
    for s in sorted({s for s in slots if 0 <= s < S}):
        rows = torch.tensor([t for t, v in enumerate(slots) if v == s])
        out[rows] = x[rows].double() @ A[s].double().t()
    return out


def _check_tmp(what, tbuf, T, exp64, rows, info):
    exp = exp64.float()
    assert bool((exp.double() == exp64)[rows].all())
    got = tbuf[:T]
    bad = (got != exp) & rows[:, None]
    _count(info, "checked", int(rows.sum()) * got.shape[1])
    return _msgs(describe(what, bad, got, exp), sentinel_bad(what, tbuf, T))


def _shrink_launches(case, be, device, what, x, A, A_dev, poison, info):
    """Every variant with ``groups = G`` and with ``groups = None``: exact, and the same bits.
    ``A`` is the clean stack of the expectation, ``A_dev`` the one the back end gets."""
    msgs = []
    for variant in range(VARIANTS):
        slots, ts, sr, tr = _meta(case.T, variant, case.R)
        xv, rows = poison(variant, slots, x[variant].clone())
        exp = shrink_expect(torch.nan_to_num(xv.float(), 0, 0, 0), A, slots)  # poisoned rows are not checked
        got = [_run_shrink(case, be, device, A_dev, xv, ts, sr, g, variant % 2 == 1) for g in (case.G, None)]
        w = f"{what} variant {variant}"
        msgs += _check_tmp(w, got[0], case.T, exp, rows, info) + _check_tmp(w + " groups=None", got[1], case.T, exp, rows, info)
        if not torch.equal(got[0][:case.T][rows], got[1][:case.T][rows]):
            msgs.append(f"{w}: groups = G and groups = None differ in bits")
        info.setdefault("inexact_in_bf16", 0)
        info["inexact_in_bf16"] += int(((exp.float().to(bf).double() != exp) & rows[:, None]).sum())
        _count(info, "launches", 2)
    return msgs


def probe_shrink_data(case, be, device, info=None):
    """Integers in [-4, 4]: sum |x a| <= 16 K < 2^24, so tmp is the fp64 sum, exactly."""
    info = {} if info is None else info
    assert 16 * case.K < 2 ** 24
    x, A = _cached(("data", case.id), lambda: shrink_inputs(case))
    A_dev = A.to(device)
    msgs = _shrink_launches(case, be, device, f"{case.id} data", x, A, A_dev,
                            lambda v, slots, xv: (xv, torch.ones(case.T, dtype=torch.bool)), info)
    assert info["inexact_in_bf16"] >= 1 or case.T < 4, case.id  # an output rounded to bf16 would show
    return msgs


def isolation_rows(slots):
    """(tokens that must stay exact, tokens whose x row is poisoned).  Poisoned x: every token
    without a slot and token 1 of every tile if it has one; poisoned A: POISON_SLOT's block."""
    ok = valid(slots)
    x_bad = [not ok[t] or t % 16 == 1 for t in range(len(slots))]
    exact = [not (ok[t] and (x_bad[t] or slots[t] == POISON_SLOT)) for t in range(len(slots))]
    return torch.tensor(exact), torch.tensor(x_bad)


def probe_shrink_isolation(case, be, device, info=None):
    """The integer data with NaN / Inf in the A block of a slot that a neighbour uses, in the x
    row of a neighbour and in the x rows of the tokens without a slot."""
    info = {} if info is None else info
    x, A = _cached(("data", case.id), lambda: shrink_inputs(case))
    Ap = A.clone()
    Ap[POISON_SLOT, 0::2], Ap[POISON_SLOT, 1::2] = NAN, INF

    def poison(variant, slots, xv):
        exact, x_bad = isolation_rows(slots)
        xv[x_bad, 0::2], xv[x_bad, 1::2] = NAN, -INF
        return xv, exact

    return _shrink_launches(case, be, device, f"{case.id} isolation", x, A, Ap.to(device), poison, info)


SHRINK_PROBES = {"selector": probe_shrink_selector, "data": probe_shrink_data, "isolation": probe_shrink_isolation}


# ================================================================= expand ==

ExpandCase = collections.namedtuple("ExpandCase", "id N T G R strided")
EXPAND_NS = (16, 48, 64, 80, 768, 1024)
CROSS_NS = (80, 768)


def _expand_cases():
    keys = [(N, 17, G, R, 0) for N in EXPAND_NS for G, R in ((3, 64), (2, 48), (1, 16))]
    keys += [(N, 17, G, R, 0) for N in CROSS_NS for G, R in GR_PAIRS]
    keys += [(N, T, G, R, 0) for N in CROSS_NS for T in TS for G, R in ((3, 64), (2, 16))]
    keys += [(N, T, G, R, 1) for N in EXPAND_NS for T, G, R in ((17, 2, 48), (33, 3, 16))]
    return [ExpandCase(f"expand-N{N}-T{T}-G{G}-R{R}" + ("-strided" if st else ""), N, T, G, R, st)
            for N, T, G, R, st in dict.fromkeys(keys)]


EXPAND_CASES = _expand_cases()


def tile_groups(N, G):
    """uint8 [N / 16]: the q / k / v split 512 / 128 / 128 at N = 768, interleaved gate / up at 1024,
    a group that changes with every tile elsewhere; groups above G - 1 fold onto the last."""
    nt = N // 16
    if N == 768:
        g = [0] * 32 + [1] * 8 + [2] * 8
    elif N == 1024:
        g = [i & 1 for i in range(nt)]
    else:
        g = [(i + G - 1) % G for i in range(nt)]
    return torch.tensor([min(v, G - 1) for v in g], dtype=torch.uint8)


def expand_blocks(N):
    """(blocks along N, live waves of the last one)."""
    nt = N // 16
    return (-(-nt // 4), (nt - 1) % 4 + 1)


def selector_ranks(R):
    """Both ends of every 8-wide chunk of R."""
    return [r for c in range(R // 8) for r in (8 * c, 8 * c + 7)]


def expand_selector_plan(case):
    wanted = [(g, r) for r in selector_ranks(case.R) for g in range(case.G)]
    return _plan(case.T, case.R, wanted, lambda rank, w: rank > w[1])


def code_b(N, R):
    """fp32 [S, N, R] integer codes in [-63, 64] without 0, distinct between neighbours in s, n and r,
    between a column and the same place of the next tile, a rank and the same place of the next chunk."""
    s = torch.arange(S, dtype=torch.int32)[:, None, None]
    n = torch.arange(N, dtype=torch.int32)[None, :, None]
    r = torch.arange(R, dtype=torch.int32)[None, None, :]
    c = (s * 19 + n * 7 + r * 5 + (n >> 4) * 3 + (r >> 3) * 11) % 127 - 63
    return torch.where(c == 0, torch.full_like(c, 64), c).float()


def _zero_cols_above_rank(B, R):
    """B [S, N, R] in place: columns at or above the slot's rank are zero."""
    for s, r in enumerate(slot_ranks(R)):
        B[s, :, r:] = 0
    return B


def y0_integers(T, N, gen):
    """bf16 integers in [-64, 64] with a -0.0 in every row."""
    y0 = torch.randint(-64, 65, (T, N), generator=gen).to(bf)
    y0[torch.arange(T), (torch.arange(T) * 7 + 3) % N] = -0.0
    return y0


def expand_expect(y0, tmp, B, tg, slots, R):
    """(bf16 y, fp64 y0 + delta): the fp64 sum, asserted exact in fp32, rounded once.  Rows of
    tokens without a slot are y0.  NaN operands are taken as 0: their rows are not checked."""
    T, N = y0.shape
    col_g = tg.long().repeat_interleave(16)
    t64 = torch.nan_to_num(tmp.double(), 0, 0, 0).view(T, -1, R)[:, col_g]        # [T, N, R]
    ok = torch.tensor(valid(slots))
    sel = torch.tensor([s if 0 <= s < S else 0 for s in slots])
    delta = (t64 * torch.nan_to_num(B.double(), 0, 0, 0)[sel]).sum(-1) * ok[:, None]
    s64 = y0.double() + delta
    return torch.where(ok[:, None], s64.float().to(bf), y0), s64


def _run_expand(case, be, device, y0, tmp, B_dev, tg, ts, sr, tmp_sentinel=SENTINEL):
    """One launch.  Returns the CPU y buffer [T + PAD, N (+ 24 if strided)]."""
    T, N = y0.shape
    ybuf, yv = _padded(T, N, SENTINEL, bf, 24 if case.strided else 0, TAIL_FILL)
    yv.copy_(y0)
    tbuf, tv = _padded(T, tmp.shape[1], tmp_sentinel, torch.float32)
    tv.copy_(tmp)
    ybuf, tbuf = ybuf.to(device), tbuf.to(device)
    be.expand(ybuf[:T, :N], tbuf[:T], B_dev, tg.to(device), ts.to(device), sr.to(device))
    return ybuf.cpu()


def _check_y(what, ybuf, y0, exp, slots, rows, info):
    """Checked rows equal ``exp``; rows without a slot keep y0's bits, the sign of a zero too;
    the sentinel rows and the columns behind a strided y are untouched."""
    T, N = y0.shape
    got = ybuf[:T, :N]
    ok = torch.tensor(valid(slots))
    bad = (got != exp) & rows[:, None]
    bad |= (got.view(torch.int16) != y0.view(torch.int16)) & ~ok[:, None]
    _count(info, "checked", int((rows | ~ok).sum()) * N)
    msgs = _msgs(describe(what, bad, got, exp), sentinel_bad(what, ybuf[:, :N], T))
    if ybuf.shape[1] > N and not bool((ybuf[:, N:] == TAIL_FILL).all()):
        msgs.append(f"{what}: the columns behind y were written")
    return msgs


def _all_rows(T):
    return torch.ones(T, dtype=torch.bool)


def probe_expand_selector(case, be, device, info=None):
    """tmp one-hot at rank column r_t of A block g_t: y must be y0 + B[slot, n, r_t] in the columns
    of group g_t and y0 elsewhere."""
    info = {} if info is None else info
    N, T, G, R = case.N, case.T, case.G, case.R
    B = _zero_cols_above_rank(code_b(N, R), R).to(bf)
    B_dev, tg = B.to(device), tile_groups(N, G)
    y0 = y0_integers(T, N, _gen(case.id, "cpu"))
    msgs = []
    for n, (variant, give) in enumerate(expand_selector_plan(case)):
        slots, ts, sr, tr = _meta(T, variant, R)
        tmp = torch.zeros(T, G * R)
        for t in range(T):
            tmp[t, give[t][0] * R + give[t][1]] = 1
        exp, s64 = expand_expect(y0, tmp, B, tg, slots, R)
        assert bool((s64.abs() <= 128).all())
        ybuf = _run_expand(case, be, device, y0, tmp, B_dev, tg, ts, sr)
        msgs += _check_y(f"{case.id} selector launch {n}", ybuf, y0, exp, slots, _all_rows(T), info)
        _count(info, "launches", 1)
        if len(msgs) > 4:
            break
    return msgs


def expand_data_inputs(case):
    """CPU (tmp [VARIANTS, T, G R] integers in [-8, 8], B integers in [-4, 4] zero above the ranks, y0)."""
    gen = _gen(case.id + "/data", "cpu")
    tmp = torch.randint(-8, 9, (VARIANTS, case.T, case.G * case.R), generator=gen).float()
    B = _zero_cols_above_rank(torch.randint(-4, 5, (S, case.N, case.R), generator=gen).float(), case.R).to(bf)
    return tmp, B, y0_integers(case.T, case.N, gen)


def probe_expand_data(case, be, device, info=None):
    """Integers: y must be bf16(y0 + delta) of the exact integer, one rounding to nearest even."""
    info = {} if info is None else info
    tmp, B, y0 = expand_data_inputs(case)
    B_dev, tg = B.to(device), tile_groups(case.N, case.G)
    msgs = []
    for variant in range(VARIANTS):
        slots, ts, sr, tr = _meta(case.T, variant, case.R)
        exp, s64 = expand_expect(y0, tmp[variant], B, tg, slots, case.R)
        assert bool((s64.float().double() == s64).all())
        _count(info, "rounded", int((exp.double() != s64).sum()))
        ybuf = _run_expand(case, be, device, y0, tmp[variant], B_dev, tg, ts, sr)
        msgs += _check_y(f"{case.id} data variant {variant}", ybuf, y0, exp, slots, _all_rows(case.T), info)
        _count(info, "launches", 1)
    return msgs


# the split probe's values: v = sv 2^a (1 + j / 128 + m + l), b = sb 2^e, y0 = -b sv 2^a (1 + j / 128 - 2^-7).
# b v + y0 = b sv 2^a (2^-7 + m + l): in units of 2^(a - 14) |b|, 128 + 32.5 + 2^-9 (the tie 160.5 goes down
# to the even 160; the true value goes up to 161) or 128 + 33.5 - 2^-9 (161.5 goes up to 162; the true value
# down to 161).  Without mid both give 128.
SPLIT_TAILS = ((2.0 ** -9 + 2.0 ** -15, 2.0 ** -23), (2.0 ** -9 + 2.0 ** -14 + 2.0 ** -15, -2.0 ** -23))
SPLIT_BINADES = (-3, 0, 2, 5)
SPLIT_JS = (0, 5, 77)


def split_value(i):
    """(v, y0 / b) of index i: the binades, mantissas, both tails and both signs in turn."""
    a = SPLIT_BINADES[i % 4]
    j = SPLIT_JS[(i // 4) % 3]
    m, l = SPLIT_TAILS[(i // 12) % 2]
    sv = 1 - 2 * ((i // 24) % 2)
    return sv * 2.0 ** a * (1 + j / 128 + m + l), -sv * 2.0 ** a * (1 + j / 128 - 2.0 ** -7)


def split_inputs(case, variant):
    """tmp with one nonzero entry per (token, A block), B = +-2^e in every column below the rank,
    y0 of the form above.  ``planted``: the elements whose token has a slot of rank >= 1."""
    N, T, G, R = case.N, case.T, case.G, case.R
    slots, ts, sr, tr = _meta(T, variant, R)
    tg = tile_groups(N, G)
    n = torch.arange(N)
    b = (1 - 2 * (n % 2)).double() * torch.pow(2.0, (n % 5 - 2).double())
    B = _zero_cols_above_rank(b[None, :, None].expand(S, N, R).clone(), R).to(bf)
    tmp = torch.zeros(T, G * R, dtype=torch.float64)
    y0 = torch.zeros(T, N, dtype=torch.float64)
    col_g = tg.long().repeat_interleave(16)
    for t in range(T):
        for g in range(G):
            v, y_over_b = split_value(t + 7 * g + 5 * variant)
            tmp[t, g * R + (5 * t + 3 * g + variant) % max(tr[t], 1)] = v
            y0[t, col_g == g] = (y_over_b * b)[col_g == g]
    planted = torch.tensor([r >= 1 for r in tr])
    assert bool((tmp.float().double() == tmp).all()) and bool((y0.float().to(bf).double() == y0).all())
    return tmp.float(), B, y0.float().to(bf), tg, slots, ts, sr, planted


def split_conditions(case, variant):
    """Asserts what keeps the probe sensitive and returns the number of planted elements: hi, mid and
    lo are nonzero, y0 + b v is exact in fp32, and the expand with a 1-term and with a 2-term split
    differs from the 3-term one in the bf16 bits of every planted element."""
    tmp, B, y0, tg, slots, ts, sr, planted = split_inputs(case, variant)
    nz = tmp != 0
    assert all(bool((p.float()[nz] != 0).all()) for p in split3(tmp))
    exp, s64 = expand_expect(y0, tmp, B, tg, slots, case.R)
    assert bool((s64.float().double() == s64).all())
    h, m, l = split3(tmp)
    for part in (h.float(), h.float() + m.float()):
        short, _ = expand_expect(y0, part, B, tg, slots, case.R)
        assert bool((short != exp)[planted].all()), (case.id, variant)
    assert bool((exp == y0)[~planted].all())
    return int(planted.sum()) * case.N


def probe_expand_split(case, be, device, info=None):
    """Values that need hi, mid and lo, a ``lo`` beyond a bf16 tie on the side nearest-even does not take."""
    info = {} if info is None else info
    msgs = []
    for variant in range(VARIANTS):
        tmp, B, y0, tg, slots, ts, sr, planted = split_inputs(case, variant)
        exp, _ = expand_expect(y0, tmp, B, tg, slots, case.R)
        ybuf = _run_expand(case, be, device, y0, tmp, B.to(device), tg, ts, sr)
        msgs += _check_y(f"{case.id} split variant {variant}", ybuf, y0, exp, slots, _all_rows(case.T), info)
        _count(info, "planted", int(planted.sum()) * case.N)
        _count(info, "launches", 1)
    return msgs


def rounding_inputs(case, variant):
    """Even tokens: a unit tmp entry per A block, B and y0 the tie plants of row_probes (y0 + b).
    Odd tokens: tmp = 257 (no bf16) per A block; in the columns with b = 1, y0 = 1: 258."""
    N, T, G, R = case.N, case.T, case.G, case.R
    slots, ts, sr, tr = _meta(T, variant, R)
    P = len(PLANTS)
    n = torch.arange(N)
    b = torch.tensor([p[1] for p in PLANTS], dtype=torch.float64)[n % P]
    yp = torch.tensor([p[0] for p in PLANTS], dtype=torch.float64)[n % P]
    B = _zero_cols_above_rank(b[None, :, None].expand(S, N, R).clone(), R).to(bf)
    tmp = torch.zeros(T, G * R)
    y0 = torch.zeros(T, N, dtype=torch.float64)
    for t in range(T):
        for g in range(G):
            tmp[t, g * R + (3 * t + g + variant) % max(tr[t], 1)] = 257.0 if t % 2 else 1.0
        y0[t] = (b == 1).double() if t % 2 else yp
    return tmp, B, y0.float().to(bf), tile_groups(N, G), slots, ts, sr, tr


def probe_expand_rounding(case, be, device, info=None):
    """The add is one fp32 add of the unrounded delta, stored to nearest even."""
    info = {} if info is None else info
    msgs = []
    for variant in range(VARIANTS):
        tmp, B, y0, tg, slots, ts, sr, tr = rounding_inputs(case, variant)
        exp, s64 = expand_expect(y0, tmp, B, tg, slots, case.R)
        assert bool((s64.float().double() == s64).all())
        P = len(PLANTS)
        for t in range(case.T):  # the builder's own check of the plants
            if tr[t] >= 1:
                row = exp[t].double()
                want = torch.tensor(PLANT_ROUNDED, dtype=torch.float64)[torch.arange(case.N) % P]
                assert t % 2 or bool((row == want).all()), (case.id, t)
                assert not t % 2 or bool((row[torch.arange(case.N) % P == 0] == 258).all())
        ybuf = _run_expand(case, be, device, y0, tmp, B.to(device), tg, ts, sr)
        msgs += _check_y(f"{case.id} rounding variant {variant}", ybuf, y0, exp, slots, _all_rows(case.T), info)
        _count(info, "launches", 1)
    return msgs


def probe_expand_isolation(case, be, device, info=None):
    """The integer data with NaN in the tmp rows of the tokens without a slot, in the tmp row of a
    neighbour, in the B block of POISON_SLOT and in tmp's sentinel rows."""
    info = {} if info is None else info
    tmp, B, y0 = expand_data_inputs(case)
    Bp = B.clone()
    Bp[POISON_SLOT, 0::2], Bp[POISON_SLOT, 1::2] = NAN, INF
    B_dev, tg = Bp.to(device), tile_groups(case.N, case.G)
    msgs = []
    for variant in range(VARIANTS):
        slots, ts, sr, tr = _meta(case.T, variant, case.R)
        exact, t_bad = isolation_rows(slots)
        tv = tmp[variant].clone()
        tv[t_bad] = NAN
        exp, _ = expand_expect(y0, tv, Bp, tg, slots, case.R)
        ybuf = _run_expand(case, be, device, y0, tv, B_dev, tg, ts, sr, tmp_sentinel=NAN)
        msgs += _check_y(f"{case.id} isolation variant {variant}", ybuf, y0, exp, slots, exact, info)
        _count(info, "launches", 1)
    return msgs


EXPAND_PROBES = {"selector": probe_expand_selector, "data": probe_expand_data, "split": probe_expand_split,
                 "rounding": probe_expand_rounding, "isolation": probe_expand_isolation}


# ================================================================== chain ==

ChainCase = collections.namedtuple("ChainCase", "id K N T G R")
CHAIN_CASES = [ChainCase(f"chain-K{K}-N{N}-T{T}-G{G}-R{R}", K, N, T, G, R) for K in CROSS_KS
               for N, T, G, R in ((768, 33, 3, 64), (80, 17, 2, 48), (1024, 17, 2, 16), (48, 15, 1, 32))]


def probe_chain(case, be, device, info=None):
    """The integer shrink feeds the expand through the same tmp buffer: y is the rounded exact integer."""
    info = {} if info is None else info
    K, N, T, G, R = case.K, case.N, case.T, case.G, case.R
    x, A = shrink_inputs(ShrinkCase(case.id, K, T, G, R))
    gen = _gen(case.id + "/expand", "cpu")
    B = _zero_cols_above_rank(torch.randint(-4, 5, (S, N, R), generator=gen).float(), R).to(bf)
    y0, tg = y0_integers(T, N, gen), tile_groups(N, G)
    A_dev, B_dev = A.to(device), B.to(device)
    assert 64 + 4 * R * 16 * K < 2 ** 24
    msgs = []
    for variant in range(VARIANTS):
        slots, ts, sr, tr = _meta(T, variant, R)
        t64 = shrink_expect(x[variant], A, slots)
        exp, s64 = expand_expect(y0, t64.float(), B, tg, slots, R)
        h, m, l = split3(t64.float())
        _count(info, "mid_in_use", int((m.float() != 0).sum()))
        xbuf, xv = _padded(T, K, NAN, bf)
        xv.copy_(x[variant])
        ybuf, yv = _padded(T, N, SENTINEL, bf)
        yv.copy_(y0)
        xbuf, ybuf = xbuf.to(device), ybuf.to(device)
        tbuf = torch.full((T + PAD, G * R), SENTINEL, dtype=torch.float32, device=device)
        tsd, srd = ts.to(device), sr.to(device)
        be.shrink(tbuf[:T], xbuf[:T], A_dev, tsd, srd, G)
        be.expand(ybuf[:T], tbuf[:T], B_dev, tg.to(device), tsd, srd)
        what = f"{case.id} variant {variant}"
        msgs += _check_tmp(what + " tmp", tbuf.cpu(), T, t64, _all_rows(T), info)
        msgs += _check_y(what, ybuf.cpu(), y0, exp, slots, _all_rows(T), info)
        _count(info, "launches", 2)
    assert info["mid_in_use"] >= 1 or T < 4
    return msgs


def probe_empty(be, device):
    """T = 0: each op raises nothing and writes nothing."""
    K, N, G, R = 512, 80, 2, 48
    case = ShrinkCase("empty", K, 0, G, R)
    sr = torch.tensor(slot_ranks(R), dtype=torch.int32)
    ts = torch.zeros(0, dtype=torch.int32)
    A = torch.ones(S, G * R, K, dtype=bf)
    tbuf = _run_shrink(case, be, device, A.to(device), torch.zeros(0, K, dtype=bf), ts, sr, G, False)
    ecase = ExpandCase("empty", N, 0, G, R, 0)
    ybuf = _run_expand(ecase, be, device, torch.zeros(0, N, dtype=bf), torch.zeros(0, G * R),
                       torch.ones(S, N, R, dtype=bf).to(device), tile_groups(N, G), ts, sr)
    return _msgs(sentinel_bad("0-token shrink", tbuf, 0), sentinel_bad("0-token expand", ybuf, 0))
