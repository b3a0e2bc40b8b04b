"""Exact probes for the MoE path: routing and dispatch (ops/csrc/moe.hip), the grouped gate_up
GEMM read through ``a_rows`` (gemm.hip) and the tail that combines, adds into the residual and
normalises - with the grouped down GEMM's split-K slabs summed by the tail itself.  The
pieces (inputs, checks, back-end split) are tests/gemm_probes.py's; profiles/moe_probes.md has
the reasoning, the derivation of each bound and the measured figures.

Routing.  x is +-1 / 0 (``tern``, density 1/2), the router weight 0.25 * tern of density
min(1, 128 / H): every logit is an integer over 4, |4 l| <= 256 - exact in fp32 in any summation
order and a bf16 number.  Router row 0 is copied into row E - 1 (and row 2 into row 3 from 8
experts on), so every token ties those pairs.  The expectation is the definition in fp64: topi the
first k of a STABLE descending sort (lower index first), compared with torch.equal; topw =
exp(l_j - l_max) / sum over the chosen k, relative 2^-18 with no absolute term.  The prologue
form (``pro``) makes its own x, so its logits are recomputed in fp64 from the kernel's xn and
two experts are interchangeable only where those logits round to one bf16 value or lie within a
bf16 ulp of each other (``near_tie_tokens``: at most 2 % of a case's tokens).

Layout, from the definition: offsets the exclusive cumsum of the local experts' counts, inv -1
exactly on the non-local slots, the local slots' rows a permutation of [0, n) inside their
expert's range (in slot order for moe_dispatch_small), src / arow and xp the inverse, and
nothing written behind row n: every buffer is prefilled with a sentinel (7.0, -7) and is PAD
entries longer than the op sees.

Tail.  y is integers in [-8, 8], topw eighths in [1/8, 1] (all different within a token), so
every w y and their sum is exact in fp32: m = bf16(sum) is one rounding of an exact number and
the new residual bf16(res + m) is exact too.  Rows behind the valid ones hold NaN.
"""
import collections

import torch

import gemm_probes as gp
from gemm_probes import EPS, NAN, PAD, SENTINEL, ULP, bf

ISENT = -7                 # the sentinel of the int32 buffers
TOPW_REL = 2.0 ** -18      # profiles/moe_probes.md "The bound on topw"
NEAR_TIE_CAP = 0.02
LOGIT_MAX, SPREAD_MAX = 8.25, 5.25
RANGES = ("full", "half", "none")
MID_TOKS = (0, 2, 4, 8)
K_SLOTS = 2                # the slots per token of the GEMM-bearing probes

# (T, E, k, H)
SMALL = [(1, 8, 2, 1024), (16, 8, 2, 8192), (16, 64, 8, 2048), (5, 4, 1, 4096), (16, 64, 1, 1024)]
MID = [(17, 8, 2, 1024), (33, 64, 8, 4096), (600, 64, 8, 1024), (300, 8, 2, 8192)]
ROUTE = [(1, 8, 2, 1024), (600, 64, 8, 1024), (129, 8, 2, 1024)]  # H only shapes the logits' generator
PERMUTE_RANKS = (150, 8, 264, 256)  # T, k, H, n_local: 1200 slots by destination rank
COMBINE = [(1, 2, 8), (9, 2, 2056), (3, 1, 8192), (16, 8, 2048)]  # (T, k, H)
COMBINE_NORM = [(1, 2, 512), (9, 8, 8192), (17, 2, 4096)]
COMBINE_NORM_REFUSED = (3, 2, 520)

GROUPED_CASES = [c for c in gp.CASES if c.op in (gp.GROUPED, gp.GROUPED_SILU)]
DOWN_CASES = [c for c in gp.CASES if c.op == gp.GROUPED]


def is_slab(case):
    """The table's route of the case's shape splits K: the tail sums the slabs, y is not formed."""
    return gp.CLASSES[case.cls]["route"]["splits"] > 1


def _first_m(pred):
    return min((c for c in DOWN_CASES if pred(c)), key=lambda c: c.M)


# the partial-range form of the down tail: at one slab class and one class that forms y
DOWN_PARTIAL = [_first_m(is_slab), _first_m(lambda c: not is_slab(c) and c.M >= 129)]

# generator salts: the (deterministic) generator of a case is seeded from its id + salt; a salt is
# there where salt 0 misses a condition that test_moe_probes_cpu asserts from the reference alone
# (a tie at the k / k + 1 boundary, |l| <= 8.25, the 2 % cap): ``python tests/test_moe_probes_cpu.py``
SALT = {"small-T1-E8-k2-H1024": 2, "mid-T600-E64-k8-H1024": 68, "route-T600-E64-k8-H1024": 14}


def dispatch_id(kind, T, E, k, H, pro=False):
    return f"{kind}-T{T}-E{E}-k{k}-H{H}" + ("-pro" if pro else "")


def _gens(cid, device):
    key = f"{cid}#{SALT.get(cid, 0)}"
    return gp._gen(key, device), gp._gen(key, "cpu")


# ---------------------------------------------------------------- routing --

def router_weight(E, H, gen):
    wr = 0.25 * gp.tern((E, H), min(1.0, 128.0 / H), gen)
    wr[E - 1] = wr[0]
    if E >= 8:
        wr[3] = wr[2]
    return wr


def expected_route(l, k):
    """(topi int32, topw fp64) of fp64 logits: stable descending sort, softmax over the chosen k."""
    order = torch.sort(l, dim=-1, descending=True, stable=True).indices[:, :k]
    lc = l.gather(1, order)
    p = torch.exp(lc - lc[:, :1])
    return order.to(torch.int32), p / p.sum(-1, keepdim=True)


def boundary_ties(l, k):
    """Per token: the k-th and (k + 1)-th sorted logits are equal."""
    s = torch.sort(l, dim=-1, descending=True).values
    return s[:, k - 1] == s[:, k] if k < l.shape[1] else torch.zeros(l.shape[0], dtype=torch.bool, device=l.device)


def router_inputs(cid, T, E, k, H, device, empty=False):
    """(x, wr, dead): ``dead`` (with ``empty``) is an expert no token chooses - one the reference
    finds, or expert 1 with its row zeroed and the logit -8 through a planted column."""
    _, gen = _gens(cid, device)  # the CPU generator: the GPU runs the very tensors the CPU test checked
    x = gp.tern((T, H), 0.5, gen).to(device)
    wr = router_weight(E, H, gen).to(device)
    if not empty:
        return x, wr, None
    chosen = set(expected_route(x.double() @ wr.double().t(), k)[0].flatten().tolist())
    free = [e for e in range(E) if e not in chosen]
    if free:
        return x, wr, free[0]
    x[:, H - 1] = 1
    wr[:, H - 1] = 0
    wr[1] = 0
    wr[1, H - 1] = -8
    return x, wr, 1


def pro_inputs(cid, T, E, k, H, device, empty=False):
    """(o, res, nw, wr, dead) of the prologue form: integer o and res; ``empty`` plants column
    H - 1 (o + res = 8 under a norm weight of 1: xn ~ 1.6 there) against -8 in the zeroed row 1."""
    _, gen = _gens(cid, device)
    o, res = gp.resid((T, H), gen).to(device), gp.resid((T, H), gen).to(device)
    nw = (0.5 + torch.rand(H, generator=gen)).to(bf).to(device)
    wr = router_weight(E, H, gen).to(device)
    if not empty:
        return o, res, nw, wr, None
    o[:, H - 1] = res[:, H - 1] = 4
    nw[H - 1] = 1
    wr[:, H - 1] = 0
    wr[1] = 0
    wr[1, H - 1] = -8
    return o, res, nw, wr, 1


def local_range(rng, E, dead):
    return {"full": (0, E), "half": (E // 2, E - E // 2), "none": (dead, 1)}[rng]


def _where(bad):
    """(token, slot) of the first True of a [T, k] mask."""
    i = int(bad.flatten().nonzero()[0])
    return divmod(i, bad.shape[1])


def check_topi(what, topi, ei, l, accept=None):
    bad = topi != ei
    if accept is not None:
        bad = bad & ~accept
    if not bool(bad.any()):
        return []
    t, j = _where(bad)
    g, e = int(topi[t, j]), int(ei[t, j])
    lg = float(l[t, g]) if 0 <= g < l.shape[1] else NAN
    return [f"{what} topi: {int(bad.sum())} of {bad.numel()} slots wrong ({int(bad.any(1).sum())} tokens); token {t} slot {j}: "
            f"got expert {g} (logit {lg:.6g}), expected expert {e} (logit {float(l[t, e]):.6g})"]


def check_topw(what, topw, ew, tol, info):
    rel = (topw.double() - ew).abs() / ew
    info["topw_rel"] = max(info.get("topw_rel", 0.0), float(rel.nan_to_num(nan=1e300).max()))
    bad = ~(rel <= tol)
    if not bool(bad.any()):
        return []
    t, j = _where(bad)
    return [f"{what} topw: {int(bad.sum())} of {bad.numel()} weights outside the bound; token {t} slot {j}: got "
            f"{float(topw[t, j]):.9g}, expected {float(ew[t, j]):.9g} (relative {float(rel[t, j]):.3g})"]


def check_route(what, topw, topi, l, k, info):
    """Exact logits: the ids of the stable sort, the weights within 2^-18."""
    ei, ew = expected_route(l, k)
    return check_topi(what, topi, ei, l) + check_topw(what, topw, ew, TOPW_REL, info)


def logit_figures(l, k, info):
    s = torch.sort(l, dim=-1, descending=True).values
    info["logit_max"], info["spread"] = float(l.abs().max()), float((s[:, 0] - s[:, k - 1]).max())
    info["ties"], info["any_tie"] = float(boundary_ties(l, k).double().mean()), bool(boundary_ties(l, k).any())


def check_route_near(what, topw, topi, xn, wr, k, info):
    """Logits recomputed in fp64 from the kernel's own xn: the stable sort of their bf16
    roundings, either of two experts where the fp64 logits cannot tell them apart - never
    between two experts with the same router row, whose logits are the same arithmetic and tie
    exactly; the weights follow the kernel's ids, each bf16 logit possibly one ulp off."""
    l = xn.double() @ wr.double().t()
    E = l.shape[1]
    same_row = (wr[:, None, :] == wr[None, :, :]).all(-1)
    lb = l.float().to(bf).double()
    ei, _ = expected_route(lb, k)
    gi = topi.long().clamp(0, E - 1)
    lg, le = l.gather(1, gi), l.gather(1, ei.long())
    near = (lg.float().to(bf) == le.float().to(bf)) | ((lg - le).abs() <= ULP * torch.maximum(lg.abs(), le.abs()))
    near = near & ~same_row[gi, ei.long()]
    used = (topi != ei) & near
    info["near_tie_tokens"] = max(info.get("near_tie_tokens", 0.0), float(used.any(1).double().mean()))
    msgs = check_topi(what, topi, ei, lb, near)
    dup = torch.sort(topi, dim=1).values
    if bool((dup[:, 1:] == dup[:, :-1]).any()):
        msgs.append(f"{what} topi: token {_where(dup[:, 1:] == dup[:, :-1])[0]} chose one expert twice")
    lk = lb.gather(1, gi)
    p = torch.exp(lk - lk.max(1, keepdim=True).values)
    tol = TOPW_REL + torch.expm1(2 * ULP * lk.abs().max(1, keepdim=True).values)
    return msgs + check_topw(what, topw, p / p.sum(-1, keepdim=True), tol, info)


# ----------------------------------------------------------------- layout --

def check_layout(what, topi, e0, nl, offsets, inv, back, xp, x, slot_order, back_is_slot):
    """offsets [nl + 1 + PAD], inv and back (src: row -> slot, or arow: row -> token) [T k + PAD],
    xp [T k + PAD, H] or None, against the definition over the op's own ``topi`` [T, k]."""
    T, k = topi.shape
    S = T * k
    dev = topi.device
    flat = topi.reshape(-1).long() - e0
    local = (flat >= 0) & (flat < nl)
    counts = torch.bincount(flat[local], minlength=nl)
    eoff = torch.cat([torch.zeros(1, dtype=torch.long, device=dev), counts.cumsum(0)])
    n = int(eoff[-1])
    msgs = []
    got_off = offsets[:nl + 1].long()
    if not torch.equal(got_off, eoff):
        e = int((got_off != eoff).nonzero()[0])
        msgs.append(f"{what} offsets: entry {e} (local expert {min(e, nl - 1)}) is {int(got_off[e])}, expected {int(eoff[e])}")
    iv = inv[:S].long()
    kept, dropped = ~local & (iv != -1), local & (iv < 0)
    if bool(kept.any()):
        s = int(kept.nonzero()[0])
        msgs.append(f"{what} inv: {int(kept.sum())} non-local slots are not -1; slot {s} (token {s // k}, expert "
                    f"{int(topi.reshape(-1)[s])}) has row {int(iv[s])}")
    if bool(dropped.any()):
        s = int(dropped.nonzero()[0])
        msgs.append(f"{what} inv: {int(dropped.sum())} local slots have no row; slot {s} (token {s // k}, expert "
                    f"{int(topi.reshape(-1)[s])}) has {int(iv[s])}")
    ls = local.nonzero().flatten()
    rows, es = iv[ls], flat[ls]
    outside = (rows < eoff[es]) | (rows >= eoff[es + 1])
    if bool((outside & (rows >= 0)).any()):
        i = int((outside & (rows >= 0)).nonzero()[0])
        msgs.append(f"{what} inv: slot {int(ls[i])} (expert {int(es[i]) + e0}) has row {int(rows[i])}, outside its expert's "
                    f"rows [{int(eoff[es[i]])}, {int(eoff[es[i] + 1])})")
    if not torch.equal(torch.sort(rows).values, torch.arange(n, device=dev)):
        msgs.append(f"{what} inv: the local slots' rows are no permutation of [0, {n})")
    if slot_order:
        order = torch.argsort(es, stable=True)
        want = torch.empty_like(rows)
        want[order] = torch.arange(n, device=dev)
        if not torch.equal(rows, want):
            i = int((rows != want).nonzero()[0])
            msgs.append(f"{what} inv: slot order not kept inside an expert; slot {int(ls[i])} has row {int(rows[i])}, "
                        f"expected {int(want[i])}")
    ok = (rows >= 0) & (rows < n)
    rs, ss = rows[ok], ls[ok]
    want = ss if back_is_slot else ss // k
    wrong = back[rs].long() != want
    if bool(wrong.any()):
        i = int(wrong.nonzero()[0])
        msgs.append(f"{what} {'src' if back_is_slot else 'arow'}: row {int(rs[i])} (slot {int(ss[i])}, token {int(ss[i]) // k}) "
                    f"names {int(back[rs[i]])}, expected {int(want[i])}")
    if xp is not None:
        wrong = (xp[rs].view(torch.int16) != x[ss // k].view(torch.int16)).any(1)
        if bool(wrong.any()):
            i = int(wrong.nonzero()[0])
            msgs.append(f"{what} xp: row {int(rs[i])} is not x[{int(ss[i]) // k}] bit for bit ({int(wrong.sum())} rows)")
        behind = (xp[n:] != SENTINEL).any(1)
        if bool(behind.any()):
            msgs.append(f"{what} xp: row {n + int(behind.nonzero()[0])} behind the {n} valid rows was written")
    for name, buf, first in (("src" if back_is_slot else "arow", back, n), ("inv", inv, S), ("offsets", offsets, nl + 1)):
        behind = buf[first:] != ISENT
        if bool(behind.any()):
            msgs.append(f"{what} {name}: entry {first + int(behind.nonzero()[0])} behind the {first} valid ones was written")
    return msgs


def _ints(n, device):
    return torch.full((n,), ISENT, dtype=torch.int32, device=device)


def probe_dispatch(kind, shape, rng, be, device, info=None, pro=False):
    """moe_dispatch_small / moe_dispatch_mid (``kind`` "small" / "mid") over one local range; the
    mid form launches twice, the second result bit-identical in topi and offsets."""
    T, E, k, H = shape
    info = {} if info is None else info
    cid = dispatch_id(kind, T, E, k, H, pro)
    what = f"{cid} [{rng}]"
    S = T * k
    if pro:
        o, res, nw, wr, dead = pro_inputs(cid, T, E, k, H, device, rng == "none")
        x = None
    else:
        x, wr, dead = router_inputs(cid, T, E, k, H, device, rng == "none")
    e0, nl = local_range(rng, E, dead)
    runs = []
    for launch in range(2 if kind == "mid" else 1):
        topw = torch.full((T, k), NAN, dtype=torch.float32, device=device)
        topi = _ints(S, device).view(T, k)
        offsets, inv, back = _ints(nl + 1 + PAD, device), _ints(S + PAD, device), _ints(S + PAD, device)
        xp = gp._padded(S, H, device) if kind == "small" else None
        r, p = None, None
        xs = x
        if pro:
            r = gp._padded(T, H, device)
            r[:T] = res
            xs = torch.full((T, H), NAN, dtype=bf, device=device)
            p = (o, r[:T], nw, EPS)
        if kind == "small":
            ok = be.dispatch_small(topw, topi, xp[:S], offsets[:nl + 1], back[:S], inv[:S], xs, wr, e0, nl, p)
        else:
            ok = be.dispatch_mid(topw, topi, offsets[:nl + 1], back[:S], inv[:S], xs, wr, e0, nl, p)
        if not ok:
            return [f"{what}: the launch was refused"]
        runs.append((topw, topi, offsets, inv, back, xp, r, xs))
    topw, topi, offsets, inv, back, xp, r, xs = runs[0]
    msgs = []
    if pro:
        m, info["second_order"] = gp.check_residual(what + " residual", r, T, res, o.double())
        msgs += m
        # the kernel rounds r * rs to bf16 before the weight, by design (norm.hip's rounding)
        scaled = gp.norm64(r[:T], torch.ones_like(nw))
        exps = [gp.norm64(r[:T], nw)] + [s * nw.double() for s in gp.bf16_either(scaled)]
        m = gp.describe(what + " xn", gp.either_bad(xs, exps), xs, exps[0])
        msgs += [m] if m else []
        l = xs.double() @ wr.double().t()
        msgs += check_route_near(what, topw, topi, xs, wr, k, info)
    else:
        l = x.double() @ wr.double().t()
        logit_figures(l, k, info)
        msgs += check_route(what, topw, topi, l, k, info)
    if rng == "none" and bool((expected_route(l.float().to(bf).double(), k)[0] == dead).any()):
        msgs.append(f"{what}: the probe's own condition failed, expert {dead} is chosen")
    msgs += check_layout(what, topi, e0, nl, offsets, inv, back, xp, xs, kind == "small", kind == "small")
    if len(runs) == 2 and not (torch.equal(runs[1][1], topi) and torch.equal(runs[1][2], offsets)):
        msgs.append(f"{what}: a relaunch is not bit-identical in topi and offsets")
    return msgs


def probe_route_permute(shape, rng, be, device, info=None):
    """moe_route over the exact logits given as a bf16 tensor, then moe_permute of its ids."""
    T, E, k, H = shape
    info = {} if info is None else info
    cid = dispatch_id("route", T, E, k, H)
    what = f"{cid} [{rng}]"
    S = T * k
    x, wr, dead = router_inputs(cid, T, E, k, H, device, rng == "none")
    e0, nl = local_range(rng, E, dead)
    l = x.double() @ wr.double().t()
    logits = l.to(bf)
    if not torch.equal(logits.double(), l):
        return [f"{what}: the probe's own condition failed, a logit is no bf16 number"]
    logit_figures(l, k, info)
    topw = torch.full((T, k), NAN, dtype=torch.float32, device=device)
    topi = _ints(S, device).view(T, k)
    be.route(topw, topi, logits)
    msgs = check_route(what, topw, topi, l, k, info)
    offsets, inv, src = _ints(nl + 1 + PAD, device), _ints(S + PAD, device), _ints(S + PAD, device)
    xp = gp._padded(S, H, device)
    be.permute(xp[:S], offsets[:nl + 1], src[:S], inv[:S], x, topi, e0, nl)
    return msgs + check_layout(what, topi, e0, nl, offsets, inv, src, xp, x, False, True)


def probe_permute_ranks(be, device, info=None):
    """moe_permute as the all-to-all exchange uses it: the ids are destination ranks, 256 of them
    (moe_sort_kernel's largest n_local), some -1 (padding rows), and more slots than one pass of
    the sorting workgroup."""
    T, k, H, nl = PERMUTE_RANKS
    what = f"permute-ranks-T{T}-k{k}-H{H}-n{nl}"
    gen, _ = _gens(what, device)
    S = T * k
    x = gp.resid((T, H), gen)
    topi = torch.randint(0, nl, (T, k), generator=gen, device=device, dtype=torch.int32)
    topi[torch.rand((T, k), generator=gen, device=device) < 0.1] = -1
    topi[0, 0], topi[0, 1] = 0, nl - 1
    offsets, inv, src = _ints(nl + 1 + PAD, device), _ints(S + PAD, device), _ints(S + PAD, device)
    xp = gp._padded(S, H, device)
    be.permute(xp[:S], offsets[:nl + 1], src[:S], inv[:S], x, topi, 0, nl)
    return check_layout(what, topi, 0, nl, offsets, inv, src, xp, x, False, True)


# ------------------------------------------- grouped GEMM through a_rows --

def rows_behind(what, buf, n):
    """Rows n.. of buf (invalid rows of the op's own buffer, then the PAD rows) still hold the sentinel."""
    bad = (buf[n:] != SENTINEL).any(1)
    if not bool(bad.any()):
        return None
    return f"{what}: {int(bad.sum())} rows behind the {n} valid rows were written, the first one row {n + int(bad.nonzero()[0])}"


def _offsets(counts, device):
    offs = [0]
    for c in counts:
        offs.append(offs[-1] + c)
    return offs, torch.tensor(offs, dtype=torch.int32, device=device)


def pair_counts(n, G, T, gen):
    """``group_counts`` with no expert above T rows: token t's two rows, r and r + T of the rows
    sorted by expert, then lie under two different experts."""
    while True:
        c = gp.group_counts(n, G, gen)
        if max(c) <= T:
            return c


def probe_a_rows(case, be, device, info=None, partial=False):
    """The grouped branch of gemm_probes.probe with A the [T, K] token rows and ``a_rows`` the
    token of each of the 2 T permuted rows; ``partial``: a third of the rows are not valid."""
    op, N, K, G, T = case.op, case.N, case.K, case.n_groups, case.M
    info = {} if info is None else info
    R = K_SLOTS * T
    n = R - R // 3 if partial else R
    cid = case.id + "-arows" + ("-part" if partial else "")
    what = f"{cid} [{gp.class_name(case.cls) if len(case.cls) > 2 else case.cls[1]}]"
    gen, cgen = _gens(cid, device)
    counts = pair_counts(n, G, T, cgen)
    offs, offsets = _offsets(counts, device)
    pi = torch.randperm(T, generator=cgen)
    a_rows = torch.full((R,), T + 7, dtype=torch.int32)
    a_rows[:n] = pi[torch.arange(n) % T].to(torch.int32)
    a_rows = a_rows.to(device)
    a = gp.tern((T, K), 0.5, gen)
    w = gp.tern((G, N, K), gp.w_density(K) if op == gp.GROUPED else gp.silu_density(op, K), gen)
    if op == gp.GROUPED:
        gp.plant(a[int(a_rows[n - 1])], w[max(e for e in range(G) if counts[e])])
    else:
        w = torch.stack([be.ops.interleave_gate_up(w[e, :N // 2], w[e, N // 2:]) for e in range(G)])
    out = gp._padded(R, N if op == gp.GROUPED else N // 2, device)
    be.grouped_rows(out[:R], a, w, offsets, gp.rows_per_group(case), op & 1, a_rows)
    y = torch.empty(n, N, dtype=torch.float64, device=device)
    for e in range(G):
        y[offs[e]:offs[e + 1]] = a[a_rows[offs[e]:offs[e + 1]].long()].double() @ w[e].double().t()
    info["counts"] = counts
    if op == gp.GROUPED:
        info["over256"] = float((y.abs() > 256).double().mean())
        msgs = gp.check_plain(what, out[:n], n, y)
    else:
        y = be.ops.deinterleave_cols(y)
        g, u = y[:, :N // 2], y[:, N // 2:]
        info["over256"] = float((y.abs() > 256).double().mean())
        info["silu_in_range"] = float(((g.abs() <= 100) & (u.abs() <= 100)).double().mean())
        msgs = gp.check_ulp(what, out[:n], n, gp.silu_mul64(g, u))
    msgs += [m for m in (rows_behind(what, out, n),) if m]
    return [m + f" ({n} valid rows of {R}, rows per expert {counts})" for m in msgs]


# ------------------------------------------------------------------- tail --

Tail = collections.namedtuple("Tail", "inv offsets offs topw n dead counts")


def tail_layout(T, k, G, partial, cgen, device):
    """inv (a random permutation of the n local slots' rows), offsets over G uneven experts, topw
    in eighths (all different within a token) and the token whose slots are all -1 (T >= 2);
    ``partial``: half of the slots are not local."""
    local = torch.rand((T, k), generator=cgen) < 0.5 if partial else torch.ones((T, k), dtype=torch.bool)
    dead = T // 2 if T >= 2 else None
    if dead is not None:
        local[dead] = False
    if not bool(local.any()):
        local[0, 0] = True
    n = int(local.sum())
    counts = gp.group_counts(n, G, cgen)
    offs, offsets = _offsets(counts, device)
    inv = torch.full((T * k,), -1, dtype=torch.int32)
    inv[local.flatten()] = torch.randperm(n, generator=cgen).to(torch.int32)
    topw = (torch.rand((T, 8), generator=cgen).argsort(1)[:, :k] + 1).float() / 8
    buf = _ints(T * k + PAD, device)
    buf[:T * k] = inv.to(device)
    return Tail(buf, offsets, offs, topw.to(device), n, dead, counts)


def combine64(y, tl, T, k):
    """sum_j w_j y[inv] in fp64 over y [n or more rows, H] fp64 (the bf16 values)."""
    iv = tl.inv[:T * k].view(T, k).long()
    g = torch.where((iv >= 0)[..., None], y[iv.clamp(min=0)], torch.zeros((), dtype=torch.float64, device=y.device))
    return (g * tl.topw.double()[..., None]).sum(1)


def check_exact(what, buf, M, exp):
    e = exp.float().to(bf)
    return [m for m in (gp.describe(what, buf[:M] != e, buf[:M], e), gp.sentinel_bad(what, buf, M)) if m]


def check_tail(what, out, r, res, m64, nw, tl, T, info):
    """The new residual bf16(res + bf16(m)), exact; the normed output within one ulp of norm64 of
    it; the token with no local slot bit-identical."""
    m = m64.float().to(bf).double()
    msgs, info["second_order"] = gp.check_residual(what + " residual", r, T, res, m)
    msgs += gp.check_ulp(what + " norm", out, T, gp.norm64(r[:T], nw))
    if tl.dead is not None and not torch.equal(r[tl.dead].view(torch.int16), res[tl.dead].view(torch.int16)):
        msgs.append(f"{what} residual: token {tl.dead} has no local slot, yet its residual changed")
    if int(tl.inv[T * tl.topw.shape[1]:].ne(ISENT).sum()):
        msgs.append(f"{what}: inv was written")
    return msgs


def _y_rows(R, H, n, gen, device):
    y = torch.full((R, H), NAN, dtype=bf, device=device)
    y[:n] = gp.resid((n, H), gen)
    return y


def probe_combine(shape, be, device, info=None, partial=True):
    T, k, H = shape
    what = f"combine-T{T}-k{k}-H{H}"
    gen, cgen = _gens(what, device)
    tl = tail_layout(T, k, 4, partial, cgen, device)
    y = _y_rows(T * k, H, tl.n, gen, device)
    out = gp._padded(T, H, device)
    be.combine(out[:T], y, tl.inv[:T * k], tl.topw)
    return check_exact(what, out, T, combine64(y.double(), tl, T, k))


def probe_combine_norm(shape, be, device, info=None, partial=True):
    T, k, H = shape
    info = {} if info is None else info
    what = f"combine_norm-T{T}-k{k}-H{H}"
    gen, cgen = _gens(what, device)
    tl = tail_layout(T, k, 4, partial, cgen, device)
    y = _y_rows(T * k, H, tl.n, gen, device)
    res = gp.resid((T, H), gen)
    nw = (0.5 + torch.rand(H, generator=gen, device=device)).to(bf)
    r, out = gp._padded(T, H, device), gp._padded(T, H, device)
    r[:T] = res
    ok = be.combine_norm(out[:T], r[:T], y, tl.inv[:T * k], tl.topw, nw)
    if H % 512 or H > 8192:  # no whole waves, or more than 1024 threads: refused, nothing written
        msgs = [f"{what}: the launch was not refused"] if ok else []
        if not (torch.equal(r[:T], res) and bool((out == SENTINEL).all()) and bool((r[T:] == SENTINEL).all())):
            msgs.append(f"{what}: a refused launch wrote")
        return msgs
    if not ok:
        return [f"{what}: the launch was refused"]
    return check_tail(what, out, r, res, combine64(y.double(), tl, T, k), nw, tl, T, info)


def probe_down(case, be, device, info=None, partial=False, slab=None):
    """moe_down_combine_add_rmsnorm at a grouped down shape of the table: G = n_groups, H = N,
    I = K, T = M tokens of 2 slots.  y is prefilled with NaN: it stays NaN exactly when the route
    splits K (``slab``: the tail summed the slabs), else its valid rows hold the exact product."""
    G, H, I, T = case.n_groups, case.N, case.K, case.M
    info = {} if info is None else info
    slab = is_slab(case) if slab is None else slab
    k, R = K_SLOTS, K_SLOTS * T
    cid = case.id + "-down" + ("-part" if partial else "")
    what = f"{cid} [{'slabs' if slab else 'y formed'}]"
    gen, cgen = _gens(cid, device)
    tl = tail_layout(T, k, G, partial, cgen, device)
    n = tl.n
    a = gp.tern((R, I), 0.5, gen)
    w2 = gp.tern((G, H, I), gp.w_density(I), gen)
    gp.plant(a[n - 1], w2[max(e for e in range(G) if tl.counts[e])])
    a[n:] = NAN
    res = gp.resid((T, H), gen)
    nw = (0.5 + torch.rand(H, generator=gen, device=device)).to(bf)
    r, out = gp._padded(T, H, device), gp._padded(T, H, device)
    r[:T] = res
    y = torch.full((R + PAD, H), NAN, dtype=bf, device=device)
    if not be.down(out[:T], r[:T], y[:R], a, w2, tl.offsets, gp.rows_per_group(case), tl.inv[:T * k], tl.topw, nw):
        return [f"{what}: the launch was refused"]
    yv = torch.zeros(R, H, dtype=torch.float64, device=device)
    for e in range(G):
        yv[tl.offs[e]:tl.offs[e + 1]] = a[tl.offs[e]:tl.offs[e + 1]].double() @ w2[e].double().t()
    info["over256"], info["n"], info["counts"] = float((yv[:n].abs() > 256).double().mean()), n, tl.counts
    yb = yv.float().to(bf)
    msgs = check_tail(what, out, r, res, combine64(yb.double(), tl, T, k), nw, tl, T, info)
    if be.forms_y:
        nan = torch.isnan(y)
        info["y_formed"] = not bool(nan.all())
        if slab and not bool(nan.all()):
            msgs.append(f"{what} y: {int((~nan).any(1).sum())} rows were written, the table's route sums slabs")
        if not slab:
            bad = y[:n] != yb[:n]
            m = gp.describe(what + " y", bad, y[:n], yb[:n])
            msgs += [m] if m else []
            if not bool(nan[n:].all()):
                msgs.append(f"{what} y: row {n + int((~nan[n:]).any(1).nonzero()[0])} behind the {n} valid rows was written")
    return [m + f" ({n} valid rows of {R}, rows per expert {tl.counts})" for m in msgs]


# -------------------------------------------------------------- back ends --

class HipMoe(gp.HipBackend):
    """The raw MoE ops, as the wrappers of mlopamd.ops call them."""
    forms_y = True

    def route(self, topw, topi, logits):
        torch.ops.mlop.moe_route(topw, topi, logits)

    def permute(self, xp, offsets, src, inv, x, topi, e0, nl):
        torch.ops.mlop.moe_permute(xp, offsets, src, inv, x, topi, e0, nl)

    def dispatch_small(self, topw, topi, xp, offsets, src, inv, x, wr, e0, nl, pro=None):
        return torch.ops.mlop.moe_dispatch_small(topw, topi, xp, offsets, src, inv, x, wr, e0, nl, *(pro or ()))

    def dispatch_mid(self, topw, topi, offsets, arow, inv, x, wr, e0, nl, pro=None):
        return torch.ops.mlop.moe_dispatch_mid(topw, topi, offsets, arow, inv, x, wr, e0, nl, *(pro or ()))

    def grouped_rows(self, out, a, w, offsets, rpg, epi, a_rows):
        torch.ops.mlop.grouped_gemm(out, a, w, offsets, rpg, epi, a_rows)

    def combine(self, out, y, inv, topw):
        torch.ops.mlop.moe_combine(out, y, inv, topw)

    def combine_norm(self, out, res, y, inv, topw, nw):
        return torch.ops.mlop.moe_combine_add_rmsnorm(out, res, y, inv, topw, nw, EPS)

    def down(self, out, res, y, a, w2, offsets, rpg, inv, topw, nw):
        return torch.ops.mlop.moe_down_combine_add_rmsnorm(out, res, y, a, w2, offsets, rpg, inv, topw, nw, EPS)


class RefMoe(gp.RefBackend):
    """The CPU definitions of mlopamd.ops.  The fused dispatch has none of its own: it is the
    chain the CPU engine runs (add_rmsnorm, the router projection, moe_route, moe_permute).  What
    the GPU ops leave unwritten (rows behind the valid ones) is not copied out."""
    forms_y = False

    def route(self, topw, topi, logits):
        w, i = self.ops.moe_route(logits, topi.shape[1])
        topw.copy_(w)
        topi.copy_(i)

    def _permute(self, x, topi, e0, nl):
        xp, off, src, inv = self.ops.moe_permute(x, topi, e0, nl)
        return xp, off, src, inv, int(off[-1])

    def permute(self, xp, offsets, src, inv, x, topi, e0, nl):
        xp_, off, src_, inv_, n = self._permute(x, topi, e0, nl)
        xp[:n], src[:n] = xp_[:n], src_[:n]
        offsets.copy_(off)
        inv.copy_(inv_)

    def _route_x(self, topw, topi, x, wr, pro):
        if pro is not None:
            y, res, nw, eps = pro
            x.copy_(self.ops.add_rmsnorm(y, res, nw, eps))
        self.route(topw, topi, self.ops.gemm(x, wr))

    def dispatch_small(self, topw, topi, xp, offsets, src, inv, x, wr, e0, nl, pro=None):
        self._route_x(topw, topi, x, wr, pro)
        self.permute(xp, offsets, src, inv, x, topi, e0, nl)
        return True

    def dispatch_mid(self, topw, topi, offsets, arow, inv, x, wr, e0, nl, pro=None):
        self._route_x(topw, topi, x, wr, pro)
        _, off, src, inv_, n = self._permute(x, topi, e0, nl)
        arow[:n] = torch.div(src[:n], topi.shape[1], rounding_mode="floor")
        offsets.copy_(off)
        inv.copy_(inv_)
        return True

    def grouped_rows(self, out, a, w, offsets, rpg, epi, a_rows):
        n = int(offsets[-1])
        out[:n] = self.ops.grouped_gemm(a, w, offsets, epi=epi, avg_rows=rpg, a_rows=a_rows)[:n]

    def combine(self, out, y, inv, topw):
        out.copy_(self.ops.moe_combine(y, inv, topw))

    def combine_norm(self, out, res, y, inv, topw, nw):
        if y.shape[1] % 512 or y.shape[1] > 8192:  # the raw op's contract; the wrapper then runs combine + add_rmsnorm
            return False
        out.copy_(self.ops.moe_combine_add_rmsnorm(y, inv, topw, res, nw, EPS))
        return True

    def down(self, out, res, y, a, w2, offsets, rpg, inv, topw, nw):
        out.copy_(self.ops.moe_down_combine_add_rmsnorm(a, w2, offsets, inv, topw, res, nw, EPS, rpg))
        return True
