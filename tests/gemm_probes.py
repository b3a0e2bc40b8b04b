"""Exact probes for the GEMM family: one case per route class of the pinned planner table, at the
first and (a cheap form of) the last row count of the class's smallest interval, with inputs
for which the product is an exact integer whatever the summation order.

Case selection.  tests/fixtures/gemm_routes_gfx950.txt pins, per (op, N, K, n_groups) shape, the
route of every row count; its serving block (``# env cus256_sk``) is parsed here with
test_gemm_plan_cpu's own ``_rows``.  A route CLASS is (op, family, tile, splits, K % k_chunk != 0,
finish, ws_src, sk_d); refused routes are left out.  Of each class the interval with the smallest
M_first * N * K gives two cases (``second_m``).  The list is built at import: no GPU needed.

Inputs.  A is +-1 with probability 1/4 each, else 0; W is +-1 with probability q / 2 each, q =
min(1/2, 2048 / K), so a sum has std <= 32: every partial sum is an integer far below 2^24, exact
in fp32 through any split-K slab, stream-K slot or MFMA accumulation, and the bf16 result is the
rounding of one exact integer (|y| <= 256: the integer itself).  Integers up to 256 are bf16
numbers, so neither a slab kept in bf16 nor a truncating store can show on them: the plain ops
(0, 16) therefore carry a PLANT - the last row of A is all ones and a few columns of W hold
runs of ones at the lowest k (and of -1 at the highest), which makes that row's outputs 259
(rounds to 260, truncates to 258), 263 - 5 = 258 (a bf16 slab turns 263 into 264) and 515.

Checks (``probe``): exact equality for the plain ops; one bf16 ulp, |out - exp| <= 2^-7 |exp|
with no absolute term and expected 0 -> exactly 0, for everything that rounds a non-integer
(SiLU-mul, RMSNorm, row-scaled chain GEMMs); RoPE adds 2^-18 (|x| + |y|), the fp32 evaluation
error of x cos - y sin under cancellation.  Output buffers carry 3 sentinel rows of 7.0, caches
are prefilled with 64.0, workspaces and ss buffers with NaN.  The SiLU-mul and RoPE epilogues
round the projection to bf16 before they use it, by design (a fused launch repeats GEMM -> bf16
-> silu_mul / rope_cache bit for bit): the identity on integers, and where the row-scaled chain
forms (ops 9, 11) make it visible the expectation rounds there too (``bf16_either``), the
bound staying one ulp.  profiles/gemm_probes.md has the reasoning and the measured results.
"""
import collections
import hashlib

import torch

from test_gemm_plan_cpu import (ADD_NORM, CHAIN_RES_SS, CHAIN_RS, CHAIN_RS_ROPE, CHAIN_RS_SILU, FIXTURE, GROUPED,
                                GROUPED_SILU, PLAIN, ROPE, SILU, _rows)

ENV = "cus256_sk"
bf = torch.bfloat16
NAN = float("nan")
ULP = 2.0 ** -7       # one bf16 ulp, relative (profiles/attention_probes.md)
TINY = 2.0 ** -126    # the smallest normal bf16 / fp32
ROPE_ABS = 2.0 ** -18
FP32_SLOP = 2.0 ** -21  # relative: acc * rinv in fp32 with a v_rsq factor, a few fp32 ulps
EPS = 1e-5
D, BS, POS_ROWS, ROPE_THETA = 128, 16, 8192, 5e5
PAD, SENTINEL, CACHE_FILL = 3, 7.0, 64.0
MAX_MADDS = 2e11
FAMILY = "-VSTPWH"    # gemm_plan.h GemmFamily, as tests/native/gemm_plan_dump.cc letters them
SILU_OPS, ROPE_OPS, RS_OPS = (SILU, CHAIN_RS_SILU, GROUPED_SILU), (ROPE, CHAIN_RS_ROPE), (CHAIN_RS, CHAIN_RS_SILU, CHAIN_RS_ROPE)
PLANT = ((259, 0), (263, 5), (515, 0))  # (+1 at the lowest k, -1 at the highest k) of a planted W column

Case = collections.namedtuple("Case", "id op N K n_groups M cls")


# ------------------------------------------------------------- case list --

def route_class(op, K, r):
    """The class of a route given as a dict: ``_rows``'s (family a letter) or ROUTE_FIELDS zipped
    with the live ``gemm_route`` (family a GemmFamily number)."""
    fam = r["family"] if isinstance(r["family"], str) else FAMILY[r["family"]]
    tail = r["splits"] > 1 and K % r["k_chunk"] != 0
    return (op, fam, r["tile"] if fam == "T" else -1, r["splits"], tail, r["finish"], r["ws_src"], r["sk_d"])


def class_name(cls):
    op, fam, tile, splits, tail, fin, ws, d = cls
    return fam + (str(tile) if fam == "T" else "") + (f"s{splits}" if splits > 1 else "") + (str(d) if d else "")


def second_m(m0, m1):
    """The class's large-M case: the interval's last row count, or where that is far away the
    largest M = m0 + 256 j - 1 <= m0 + 1023 in it (a ragged last tile that stays cheap)."""
    if m1 <= 4 * m0 + 256:
        return m1
    return m0 + 256 * min((m1 - m0 + 1) // 256, 4) - 1


def _select():
    with open(FIXTURE) as f:
        rows = [r for r in _rows(f.read()) if r[0] == ENV and r[7]["family"] != "-"]
    best = {}
    for env, op, N, K, ng, m0, m1, r in rows:
        cls, key = route_class(op, K, r), (m0 * N * K, N, K, ng, m0, m1)
        if cls not in best or key < best[cls][0]:
            best[cls] = (key, r)
    classes, cases = {}, []
    for cls in sorted(best):
        (_, N, K, ng, m0, m1), r = best[cls]
        classes[cls] = dict(N=N, K=K, n_groups=ng, m_first=m0, m_last=m1, route=r, ms=(m0, second_m(m0, m1)))
        for M in dict.fromkeys(classes[cls]["ms"]):
            cases.append(Case(f"op{cls[0]}-N{N}-K{K}-M{M}-{class_name(cls)}", cls[0], N, K, ng, M, cls))
    return classes, cases


CLASSES, CASES = _select()
# op 8 (row-scaled, no epilogue) is in no model's shape list: one GEMV-form and one four-wave
# shape at the N / 2 of the op-9 cases (the planner's answer for them is checked on the CPU)
OP8_CASES = [Case("op8-N1792-K4096-M4-V", CHAIN_RS, 1792, 4096, 0, 4, (CHAIN_RS, "V")),
             Case("op8-N3584-K8192-M1281-W", CHAIN_RS, 3584, 8192, 0, 1281, (CHAIN_RS, "W"))]
BY_ID = {c.id: c for c in CASES + OP8_CASES}


def rows_of(case):
    """Rows of A: a grouped shape is asked, as the dump program does, with 2 M routed rows."""
    return 2 * case.M if case.n_groups else case.M


def rows_per_group(case):
    return (rows_of(case) + case.n_groups - 1) // case.n_groups


def madds(case):
    return rows_of(case) * case.N * case.K


def route_call(case):
    """Arguments of ``torch.ops.mlop.gemm_route`` for the case."""
    if case.n_groups:
        return (rows_of(case), case.N, case.K, case.op, case.n_groups, rows_per_group(case))
    return (case.M, case.N, case.K, case.op)


# ---------------------------------------------------------------- inputs --

def seed_of(cid):
    return int.from_bytes(hashlib.sha256(cid.encode()).digest()[:7], "little")


def _gen(cid, device):
    g = torch.Generator(device=device)
    g.manual_seed(seed_of(cid))
    return g


def w_density(K):
    return min(0.5, 2048.0 / K)


def silu_density(op, K):
    """q of the gate / up weights.  Sigmoid as 1 / (1 + exp(-g)) in fp32 - the kernels' and the CPU
    reference's form - is 0 below g = -88.7, where exp overflows and the true SiLU is ~ 1e-37: a
    bound with no absolute term cannot accept that, and at std 32 one gate in 300 is that low.  So
    q is lowered (never the bound widened) until the gates have std 11.3, 7.8 sigma away: 256 / K,
    and 128 / K where the row-scaled chain multiplies by x in [-8, 8] and divides by its RMS."""
    return min(0.5, (128.0 if op == CHAIN_RS_SILU else 256.0) / K)


def tern(shape, p, gen):
    """bf16 +-1 with probability p / 2 each, else 0."""
    u = torch.rand(shape, generator=gen, device=gen.device)
    return (u < p / 2).to(bf) - (u >= 1 - p / 2).to(bf)


def resid(shape, gen, density=1.0):
    """bf16 integers in [-8, 8] (``density`` of them; the rest 0)."""
    r = torch.randint(-8, 9, shape, generator=gen, device=gen.device)
    if density < 1:
        r = r * (torch.rand(shape, generator=gen, device=gen.device) < density)
    return r.to(bf)


def group_counts(R, G, gen):
    """R routed rows over G experts, unevenly; from 10 rows on one expert is empty and one has 1 row."""
    fixed, free = ([0, 1], R - 1) if R >= 10 else ([], R)
    n = G - len(fixed)
    cuts = sorted(torch.randint(0, free + 1, (n - 1,), generator=gen).tolist())
    parts = [b - a for a, b in zip([0] + cuts, cuts + [free])]
    perm = torch.randperm(G, generator=gen).tolist()
    counts = fixed + parts
    return [counts[i] for i in perm]


def plant(a_row, w):
    """The rounding plant (module docstring) into row ``a_row`` of A and columns of w [N, K]."""
    N, K = w.shape
    a_row.fill_(1)
    for j, (p, m) in enumerate(PLANT):
        if p + m <= K:
            n = (37 + 101 * j) % N
            w[n].zero_()
            w[n, :p] = 1
            if m:
                w[n, K - m:] = -1


def rope_geometry(N):
    """(Hq, Hkv) of a QKV width: 4:1 (N = 768: 4 + 1 + 1 heads), or 8:1 where the head count is
    no multiple of 6 (the K = 8192 model's shards: N = 1280 is 8 + 1 + 1)."""
    h = N // D
    assert N % D == 0 and (h % 6 == 0 or h % 10 == 0), N
    return (4 * (h // 6), h // 6) if h % 6 == 0 else (8 * (h // 10), h // 10)


def rope_meta(M, gen):
    """positions (every 4th row at 0, row 1 at the table's last row), slots (a permutation with rows
    5 and M - 1 padding when M > 5) and the number of cache blocks; CPU int32 tensors."""
    pos = torch.randint(0, POS_ROWS, (M,), generator=gen, dtype=torch.int32)
    pos[::4] = 0
    if M > 1:
        pos[1] = POS_ROWS - 1
    NB = M // BS + 8
    slots = torch.randperm(NB * BS, generator=gen)[:M].to(torch.int32)
    if M > 5:
        slots[5] = slots[M - 1] = -1
    return pos, slots, NB


_COS_SIN = {}


def cos_sin(device):
    from mlopamd.models.layers import rope_table

    key = str(device)
    if key not in _COS_SIN:
        _COS_SIN[key] = rope_table(D, POS_ROWS, ROPE_THETA, device=device)
    return _COS_SIN[key]


# ------------------------------------------------ expectations and checks --

def silu_mul64(g, u):
    return g / (1 + torch.exp(-g)) * u


def ulp_bad(out, exp, extra=None, exact=None):
    """Elements outside one bf16 ulp of exp (fp64): |out - exp| <= 2^-7 |exp| (+ extra), so an
    expected 0 must be exactly 0; an expected value below the smallest normal counts as 0 (a
    zero or a subnormal is accepted); where ``exact`` the tolerance is 0."""
    o = out.double()
    tol = ULP * exp.abs() + (0 if extra is None else extra)
    if exact is not None:
        tol = torch.where(exact, torch.zeros_like(tol), tol)
    bad = ~((o - exp).abs() <= tol)  # NaN is bad
    sub = (exp != 0) & (exp.abs() < TINY)
    return torch.where(sub, ~(o.abs() <= TINY), bad)


def describe(what, bad, got, exp):
    """None, or the count of wrong elements and rows and the worst one."""
    if not bool(bad.any()):
        return None
    bad2, got2, exp2 = (t.reshape(t.shape[0], -1) for t in (bad, got, exp))
    err = torch.where(bad2, (got2.double() - exp2.double()).abs().nan_to_num(nan=1e300, posinf=1e300), -1.0)
    i = int(err.argmax())
    r, c = divmod(i, bad2.shape[1])
    return (f"{what}: {int(bad.sum())} of {bad.numel()} elements off ({int(bad2.any(1).sum())} rows); worst at row {r} "
            f"column {c}: got {float(got2[r, c]):.6g}, expected {float(exp2[r, c]):.6g}")


def sentinel_bad(what, buf, M):
    n = int((buf[M:] != SENTINEL).sum())
    return f"{what}: {n} elements of the {PAD} rows behind the output were written" if n else None


def blame_k(a_row, w_rows, diffs, k_chunk):
    """The k whose product - or the 64-wide K tile whose products -, dropped (diff = -a w) or counted
    twice (+a w), explains every listed wrong element of one output row, where few enough do to
    tell, and its K range."""
    prod = a_row.double()[None, :] * w_rows.double()
    for sign, what in ((-1, "dropped"), (1, "counted twice")):
        ks = (prod * sign == diffs.double()[:, None]).all(0).nonzero().flatten().tolist()
        if 0 < len(ks) <= 4:
            where = f", K range {sorted({k // k_chunk for k in ks})} of {k_chunk}" if k_chunk else ""
            return f"one product {what} at k = {ks}{where} explains the row"
    tiles = prod.view(prod.shape[0], -1, 64).sum(-1)  # the same for a whole 64-wide K tile
    for sign, what in ((-1, "dropped"), (1, "counted twice")):
        ts = (tiles * sign == diffs.double()[:, None]).all(0).nonzero().flatten().tolist()
        if 0 < len(ts) <= 4:
            where = f", K range {sorted({t * 64 // k_chunk for t in ts})} of {k_chunk}" if k_chunk else ""
            return f"one 64-wide K tile {what} at k = {[t * 64 for t in ts]}{where} explains the row"
    return None


def check_plain(what, buf, M, exact, a=None, w=None, k_chunk=0):
    """Exact equality of buf[:M] with the rounded exact product; the sentinel rows untouched."""
    exp = exact.float().to(bf)
    bad = buf[:M] != exp
    msgs = [describe(what, bad, buf[:M], exp), sentinel_bad(what, buf, M)]
    if msgs[0] and a is not None:
        r = int(bad.sum(1).argmax())
        cols = bad[r].nonzero().flatten()[:64]
        hint = blame_k(a[r], w[cols], buf[r, cols].double() - exact[r, cols], k_chunk)
        if hint:
            msgs[0] += f"; row {r}: {hint}"
    return [m for m in msgs if m]


def check_ulp(what, buf, M, exp, extra=None, exact=None):
    return [m for m in (describe(what, ulp_bad(buf[:M], exp, extra, exact), buf[:M], exp), sentinel_bad(what, buf, M)) if m]


def check_residual(what, buf, M, res, y):
    """The new residual: bf16(res + y), exact; where |sum| > 256 either rounding order."""
    s = res.double() + y
    e1 = s.float().to(bf)
    e2 = (res.float() + y.float().to(bf).float()).to(bf)
    got = buf[:M]
    second = (s.abs() > 256) & (got == e2) & (got != e1)
    bad = (got != e1) & ~second
    return [m for m in (describe(what, bad, got, e1), sentinel_bad(what, buf, M)) if m], int(second.sum())


def norm64(r, nw):
    r = r.double()
    return r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + EPS) * nw.double()


def rope64(x, pos, cs, Hq, Hkv):
    """fp64 (q, k, v, q_extra, k_extra) of x [M, N] with the fp32 table's values."""
    M = x.shape[0]
    x = x.view(M, Hq + 2 * Hkv, D)
    c = cs[pos.long()].double()
    cos, sin = c[:, None, :D // 2], c[:, None, D // 2:]
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1)
    extra = ROPE_ABS * (x1.abs() + x2.abs()).repeat(1, 1, 2)
    return rot[:, :Hq], rot[:, Hq:Hq + Hkv], x[:, Hq + Hkv:], extra[:, :Hq], extra[:, Hq:Hq + Hkv]


def bf16_either(x):
    """The bf16 values an fp32 evaluation of x (fp64) can round to: the kernels round
    fp32(acc * rinv), a few fp32 ulps from x, so an x that close to a bf16 tie may go either way;
    everywhere else both entries are the one rounding of x."""
    return [(x * (1 + s)).float().to(bf).double() for s in (-FP32_SLOP, FP32_SLOP)]


def pair_variants(y):
    """The four (first half, second half) combinations of ``bf16_either`` over the D / 2 rotation
    pairs of a projection y [M, heads * D]."""
    lo, hi = bf16_either(y)
    out = []
    for a in (lo, hi):
        for b in (lo, hi):
            t = a.clone().view(y.shape[0], -1, 2, D // 2)
            t[:, :, 1] = b.view(y.shape[0], -1, 2, D // 2)[:, :, 1]
            out.append(t.view(y.shape))
    return out


def either_bad(out, exps, extras=None):
    """Outside one ulp of every expectation of the list."""
    bad = None
    for i, e in enumerate(exps):
        b = ulp_bad(out, e, None if extras is None else extras[i])
        bad = b if bad is None else bad & b
    return bad


def check_rope(what, q, kc, vc, xs, pos, slots, cs, Hq, Hkv, integers):
    """q, the K cache and the V cache after a QKV + RoPE launch over the projection xs[0]: the
    exact integers (``integers``: rows at position 0 must then equal them, and V too), or the
    ``pair_variants`` of a row-scaled projection, any of which the output may follow.  Untouched
    cache slots must still hold CACHE_FILL."""
    dev = xs[0].device
    pos, slots = pos.to(dev), slots.to(dev).long()
    at0 = (pos == 0)[:, None, None] if integers else None
    live = slots >= 0
    blk, off = slots[live] // BS, slots[live] % BS
    bads, first = {}, {}
    for x in xs:
        qe, ke, ve, qx, kx = rope64(x, pos, cs, Hq, Hkv)
        todo = [("q", q, qe, ulp_bad(q, qe, qx, None if at0 is None else at0.expand_as(qe)))]
        for name, cache, e, ex in (("K cache", kc, ke, kx), ("V cache", vc, ve, None)):
            full = torch.full(cache.shape, CACHE_FILL, dtype=torch.float64, device=dev)
            extra = torch.zeros_like(full)
            exact = torch.ones(cache.shape, dtype=torch.bool, device=dev)  # an untouched slot: exactly the fill
            full[blk, :, off] = e[live]
            if ex is not None:
                extra[blk, :, off] = ex[live]
            if not integers:
                exact[blk, :, off] = False
            elif ex is not None:  # K of an integer projection: exact at position 0; its V: everywhere
                exact[blk, :, off] = at0[live].expand(-1, Hkv, D)
            todo.append((name, cache, full, ulp_bad(cache, full, extra, exact)))
        for name, got, exp, bad in todo:
            bads[name] = bad if name not in bads else bads[name] & bad
            first.setdefault(name, (got, exp))
    return [m for m in (describe(f"{what} {n}", bads[n], *first[n]) for n in bads) if m]


# -------------------------------------------------------------- back ends --

class HipBackend:
    """The raw ops the wrappers of mlopamd.ops call, with no knob touched and no autotuner."""

    def __init__(self, device):
        from mlopamd import ops

        self.ops, self.device = ops, device
        ops.load()
        ops._sk_reserve(device)  # once, as serving does

    def writes_ss(self, M):
        return M > self.ops.decode_chain_max_m()  # the decode forms leave the ss buffer alone (gemm.hip launch_gemm_chain)

    def _ws(self, M, N, K, epi):
        n = torch.ops.mlop.gemm_workspace(M, N, K, epi)
        return torch.full((n,), NAN, dtype=torch.float32, device=self.device)

    def gemm(self, out, a, w, epi):
        torch.ops.mlop.gemm(out, a, w, self._ws(a.shape[0], w.shape[0], a.shape[1], epi), epi)

    def grouped(self, out, a, w, offsets, rpg, epi):
        torch.ops.mlop.grouped_gemm(out, a, w, offsets, rpg, epi, None)

    def add_rmsnorm(self, out, res, a, w, nw):
        return torch.ops.mlop.gemm_add_rmsnorm(out, res, a, w, nw, self._ws(a.shape[0], w.shape[0], a.shape[1], 2), EPS)

    def rope(self, q, kc, vc, a, w, pos, cs, slots):
        return torch.ops.mlop.gemm_rope_cache(q, kc, vc, a, w, pos, cs, slots)

    def res_ss(self, res, a, w, ss):
        return torch.ops.mlop.gemm_res_ss(res, a, w, ss)

    def rs(self, out, x, w, ss, epi):
        return torch.ops.mlop.gemm_rs(out, x, w, ss, EPS, epi)

    def rs_rope(self, q, kc, vc, x, w, pos, cs, slots, ss):
        return torch.ops.mlop.gemm_rs_rope(q, kc, vc, x, w, pos, cs, slots, ss, EPS)


class RefBackend:
    """The CPU definitions of mlopamd.ops (fp32 torch): what the probes must accept.  The
    row-scaled forms scale the fp32 product, as the kernels scale their accumulators (the ops'
    own CPU path scales and rounds x first, which no integer probe can follow), and round it to
    bf16 before the SiLU-mul / the rotation, as every epilogue does."""

    def __init__(self):
        from mlopamd import ops

        self.ops = ops

    def writes_ss(self, M):
        return True

    def gemm(self, out, a, w, epi):
        self.ops.gemm(a, w, out=out, epi=epi)

    def grouped(self, out, a, w, offsets, rpg, epi):
        out.copy_(self.ops.grouped_gemm(a, w, offsets, epi=epi, avg_rows=rpg))

    def add_rmsnorm(self, out, res, a, w, nw):
        out.copy_(self.ops.gemm_add_rmsnorm(a, w, res, nw, EPS))
        return True

    def rope(self, q, kc, vc, a, w, pos, cs, slots):
        self.ops.qkv_rope_cache(a, w, pos, cs, slots, kc, vc, q.shape[1], q_out=q)
        return True

    def res_ss(self, res, a, w, ss):
        self.ops.gemm_res_ss(a, w, res, ss)
        return True

    def _scaled(self, x, w, ss):
        M, K = x.shape
        return (x.float() @ w.float().t()) * torch.rsqrt(self.ops.ss_parts(ss, M, K)[1].view(M, 1) / K + EPS)

    def rs(self, out, x, w, ss, epi):
        y = self._scaled(x, w, ss).to(bf)
        out.copy_(self.ops.reference.silu_mul(self.ops.deinterleave_cols(y)) if epi else y)
        return True

    def rs_rope(self, q, kc, vc, x, w, pos, cs, slots, ss):
        q.copy_(self.ops.reference.rope_cache(self._scaled(x, w, ss).to(bf), pos, cs, slots, kc, vc, q.shape[1]))
        return True


# ----------------------------------------------------------------- probes --

def _padded(M, n, device, fill=SENTINEL):
    return torch.full((M + PAD, n), fill, dtype=bf, device=device)


def _gate_up(case, gen, ops):
    I = case.N // 2
    p = silu_density(case.op, case.K)
    g, u = tern((I, case.K), p, gen), tern((I, case.K), p, gen)
    return g, u, ops.interleave_gate_up(g, u)


def _ss_from(x, ops):
    """An ss buffer of x's rows: NaN partials, the totals (exact integers) filled in."""
    M, K = x.shape
    ss = ops.ss_buffer(M, K, x.device).fill_(NAN)
    ops.ss_parts(ss, M, K)[1].copy_(x.double().pow(2).sum(-1))
    return ss


def _rinv64(x):
    return torch.rsqrt(x.double().pow(2).sum(-1, keepdim=True) / x.shape[1] + EPS)


def probe(case, be, device, info=None):
    """Runs the case's launches on back end ``be`` and returns the list of failure messages
    (empty: passed).  ``info`` (a dict) receives the sensitivity figures of the reference and
    the count of residual elements that took the second rounding order."""
    op, N, K, M = case.op, case.N, case.K, rows_of(case)
    ops = be.ops
    gen, cgen = _gen(case.id, device), _gen(case.id, "cpu")
    info = {} if info is None else info
    what = f"{case.id} [{class_name(case.cls) if len(case.cls) > 2 else case.cls[1]}]"
    k_chunk = CLASSES[case.cls]["route"]["k_chunk"] if case.cls in CLASSES else 0
    q = w_density(K)

    def stats(y, gu=None):
        info["over256"] = float((y.abs() > 256).double().mean())
        if gu is not None:
            info["silu_in_range"] = float(((gu[0].abs() <= 100) & (gu[1].abs() <= 100)).double().mean())

    if op in (PLAIN, SILU):
        a = tern((M, K), 0.5, gen)
        if op == PLAIN:
            w = tern((N, K), q, gen)
            plant(a[M - 1], w)
            out = _padded(M, N, device)
            be.gemm(out[:M], a, w, 0)
            info["out"] = out
            y = a.double() @ w.double().t()
            stats(y)
            return check_plain(what, out, M, y, a, w, k_chunk)
        g, u, w = _gate_up(case, gen, ops)
        out = _padded(M, N // 2, device)
        be.gemm(out[:M], a, w, 1)
        yg, yu = a.double() @ g.double().t(), a.double() @ u.double().t()
        stats(torch.cat([yg, yu], 1), (yg, yu))
        return check_ulp(what, out, M, silu_mul64(yg, yu))

    if op in (GROUPED, GROUPED_SILU):
        G = case.n_groups
        counts = group_counts(M, G, cgen)
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + c)
        offsets = torch.tensor(offs, dtype=torch.int32, device=device)
        a = tern((M, K), 0.5, gen)
        w = tern((G, N, K), q if op == GROUPED else silu_density(op, K), gen)
        if op == GROUPED:
            plant(a[M - 1], w[max(e for e in range(G) if counts[e])])
        else:  # every expert's rows are gate / up interleaved in groups of 16
            w = torch.stack([ops.interleave_gate_up(w[e, :N // 2], w[e, N // 2:]) for e in range(G)])
        out = _padded(M, N if op == GROUPED else N // 2, device)
        be.grouped(out[:M], a, w, offsets, rows_per_group(case), op & 1)
        y = torch.empty(M, N, dtype=torch.float64, device=device)
        for e in range(G):
            y[offs[e]:offs[e + 1]] = a[offs[e]:offs[e + 1]].double() @ w[e].double().t()
        info["counts"], info["out"] = counts, out
        if op == GROUPED:
            stats(y)
            msgs = check_plain(what, out, M, y)
        else:
            y = ops.deinterleave_cols(y)
            stats(y, (y[:, :N // 2], y[:, N // 2:]))
            msgs = check_ulp(what, out, M, silu_mul64(y[:, :N // 2], y[:, N // 2:]))
        return [m + f" (rows per expert {counts})" for m in msgs]

    if op in (ADD_NORM, CHAIN_RES_SS):
        a, w = tern((M, K), 0.5, gen), tern((N, K), q, gen)
        res = resid((M, N), gen)
        y = a.double() @ w.double().t()
        stats(y)
        r = _padded(M, N, device)
        r[:M] = res
        if op == ADD_NORM:
            nw = (0.5 + torch.rand(N, generator=gen, device=device)).to(bf)
            out = _padded(M, N, device)
            if not be.add_rmsnorm(out[:M], r[:M], a, w, nw):
                return [f"{what}: the launch was refused"]
            msgs, info["second_order"] = check_residual(what + " residual", r, M, res, y)
            msgs += check_ulp(what + " norm", out, M, norm64(r[:M], nw))
            # one-hot: A = 0, residual row m is 16 at column 131 m % N: the output is 0 off that column
            # and 16 rsqrt(256 / N + eps) w on it; a column group missing from the sum of squares gives
            # 16 rsqrt(eps), one counted twice is off by sqrt(2)
            hot = torch.zeros(M, N, dtype=bf, device=device)
            hot[torch.arange(M, device=device), (131 * torch.arange(M, device=device)) % N] = 16
            r2, out2 = _padded(M, N, device), _padded(M, N, device)
            r2[:M] = hot
            be.add_rmsnorm(out2[:M], r2[:M], torch.zeros_like(a), w, nw)
            msgs += check_residual(what + " one-hot residual", r2, M, hot, torch.zeros_like(y))[0]
            msgs += check_ulp(what + " one-hot norm", out2, M, norm64(hot, nw))
            return msgs
        ss = ops.ss_buffer(M, N, device).fill_(NAN)
        if not be.res_ss(r[:M], a, w, ss):
            return [f"{what}: the launch was refused"]
        msgs, info["second_order"] = check_residual(what + " residual", r, M, res, y)
        if be.writes_ss(M):
            part, tot = ops.ss_parts(ss, M, N)
            sq = r[:M].double().pow(2)
            e_part = sq.view(M, N // 128, 128).sum(-1)
            msgs += [m for m in (describe(what + " ss partials", ~(part.double() == e_part), part, e_part),
                                 describe(what + " ss totals", ~(tot.double() == sq.sum(-1)).view(M, 1), tot.view(M, 1),
                                          sq.sum(-1).view(M, 1))) if m]
        elif not bool(torch.isnan(ss).all()):
            msgs.append(f"{what}: the decode form wrote into the ss buffer")
        r2, ss2 = _padded(M, N, device), ops.ss_buffer(M, N, device).fill_(NAN)
        r2[:M] = res
        be.res_ss(r2[:M], a, w, ss2)
        if not (torch.equal(r2, r) and torch.equal(ss2.view(torch.int32), ss.view(torch.int32))):
            msgs.append(f"{what}: a relaunch is not bit-identical")
        return msgs

    if op in (CHAIN_RS, CHAIN_RS_SILU):
        x = resid((M, K), gen, 0.5)
        ss, rinv = _ss_from(x, ops), _rinv64(x)
        if op == CHAIN_RS:
            w = tern((N, K), q, gen)
            out = _padded(M, N, device)
            if not be.rs(out[:M], x, w, ss, 0):
                return [f"{what}: the launch was refused"]
            y = (x.double() @ w.double().t()) * rinv
            stats(y)
            return check_ulp(what, out, M, y)
        g, u, w = _gate_up(case, gen, ops)
        out = _padded(M, N // 2, device)
        if not be.rs(out[:M], x, w, ss, 1):
            return [f"{what}: the launch was refused"]
        yg, yu = (x.double() @ g.double().t()) * rinv, (x.double() @ u.double().t()) * rinv
        stats(torch.cat([yg, yu], 1), (yg, yu))
        # (the figure for the profile note: how far the designed bf16 rounding of gate and up takes the
        # output from the SiLU-mul of the un-rounded product)
        info["off_unrounded"] = float(ulp_bad(out[:M], silu_mul64(yg, yu)).double().mean())
        exps = [silu_mul64(ga, ub) for ga in bf16_either(yg) for ub in bf16_either(yu)]
        return [m for m in (describe(what, either_bad(out[:M], exps), out[:M], exps[0]), sentinel_bad(what, out, M)) if m]

    assert op in ROPE_OPS, op
    Hq, Hkv = rope_geometry(N)
    pos, slots, NB = rope_meta(M, cgen)
    cs = cos_sin(device)
    w = tern((N, K), q, gen)
    qo = torch.full((M, Hq, D), NAN, dtype=bf, device=device)
    kc = torch.full((NB, Hkv, BS, D), CACHE_FILL, dtype=bf, device=device)
    vc = kc.clone()
    if op == ROPE:
        a = tern((M, K), 0.5, gen)
        ok = be.rope(qo, kc, vc, a, w, pos.to(device), cs, slots.to(device))
        y = a.double() @ w.double().t()
    else:
        a = resid((M, K), gen, 0.5)
        ok = be.rs_rope(qo, kc, vc, a, w, pos.to(device), cs, slots.to(device), _ss_from(a, ops))
        y = (a.double() @ w.double().t()) * _rinv64(a)
    if not ok:
        return [f"{what}: the launch was refused"]
    stats(y)
    if op != ROPE:
        qe, _, _, qx, _ = rope64(y, pos.to(device), cs, Hq, Hkv)
        info["off_unrounded"] = float(ulp_bad(qo, qe, qx).double().mean())
    return check_rope(what, qo, kc, vc, [y] if op == ROPE else pair_variants(y), pos, slots, cs, Hq, Hkv, op == ROPE)
