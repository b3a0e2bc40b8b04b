"""Exact probes for the draw kernels of ops/csrc/sampling.hip (``ops.sample``): the expected
TOKEN of every row, from an fp64 oracle of the contract in runtime/sampler.py, on logits full
of ties.  profiles/sampler_probes.md has the reasoning, the derivation of MARGIN and the
measured figures.  No GPU is needed to import or to build the cases.

Logits.  Every row is bf16 numbers cast to fp32, as the LM head's output is: eighths in
[-8, 20], clip(6 + 3.5 randn), so a value of the top few hundred is shared by several ids.  Tie
groups are planted where the kernels partition a row: the row maximum (an eighth above the drawn one) at ids 300 and
448 (two waves of one 256-stride sweep) and on both sides of the slice boundary ``per``; or at
ids 0 and V - 1; or at 255, 256 and in the last, short slice; and the value of the K-th rank
at ids 255, 256, 300, 448, per - 1, per, 2 per - 1, 2 per, the start of the last slice and V - 3,
so the K-th place is contested by more ids than there are places left; the ``plateau`` rows put
1500 more ids there, more than the kernel's tie list holds.

Decisions with a margin.  The contract orders equal logits by lower id, so the candidate set,
the nucleus and the order of the draw are fixed; what fp32 arithmetic can still move is a
cumulative mass against u or p.  Each row picks a target rank, puts u at the midpoint of the
target's CDF interval (rounded to the 24-bit grid of ``seeded_uniform``) and p at the midpoint
between the cumulative masses on either side of the wanted cut, and takes the first temperature
of a fixed list at which every such decision is at least MARGIN = 2^-12 of the mass away from
its nearest edge.  The comparison is then ``==`` on the token id.  Edge rows (u = 0,
u = 1 - 2^-24, top_p = 1e-6, T in {1e-40, 1e-6, 1e30}, greedy and top_k = 1 rows in mixed
batches) put u or p ON an edge on purpose; the distance to the edges that remain is their margin.
"""
import collections
import zlib

import numpy as np
import torch

from mlopamd.runtime.sampler import MAX_TOP_K, Sampler, SamplingParams, seeded_uniform

MARGIN = 2.0 ** -12
U_TOP = 1.0 - 2.0 ** -24          # the largest value seeded_uniform returns
TOP_NEED = 2.0 ** -10 - 2.0 ** -24  # rows with u = U_TOP: their last interval is at least 2^-10 wide
P_TINY = 1e-6
REPEATS = 3
SLICE = 8192                      # sampling.hip kPreselSlice
TS = (1.0, 0.7, 2.0, 4.0, 16.0, 64.0)          # candidate rows: the first that meets MARGIN
TS_COLD = (0.25, 0.1, 0.05, 0.03)              # full rows with p = 1: the mass on the tied maxima
TS_FULL = (1.0, 0.7, 0.5, 2.0, 4.0, 0.25, 0.1)
KS = (1, 2, 50, 1023, 1024)
TOP_VALUE = 20.0
PLATEAU = 1500                    # > sampling.hip kMaxCand

Row = collections.namedtuple("Row", "kind T k p u expect margin ok boundary seed gen_index")
Launch = collections.namedtuple("Launch", "name n V via full logits rows")


def f32(x):
    return float(np.float32(x))


def splits(n, V):
    """(S, per) of sampling.hip's sample_splits: S = 1 is the single-stage path."""
    if n <= 0 or n >= 64:
        return 1, V
    S = max((V + SLICE - 1) // SLICE, min(16, (256 + n - 1) // n))
    return (S, (V + S - 1) // S) if S > 1 else (1, V)


# ------------------------------------------------------------------ oracle --

def stable_order(l):
    """Descending value, equal logits by lower id."""
    return np.argsort(-l, kind="stable")


def members(l, order, k):
    """How many of ``order`` are candidates: exactly min(k, V) for 0 < k <= MAX_TOP_K; for a
    full row the whole vocabulary, or every id whose logit reaches the k-th value."""
    V = l.size
    if 0 < k <= MAX_TOP_K:
        return min(k, V)
    if k <= 0 or k >= V:
        return V
    return int((l >= l[order[k - 1]]).sum())


def oracle(l, T, k, p, u, order=None):
    """(token, (margin of u, margin of p), boundary) of one row, fp64.  A margin: the smallest
    distance of the decision from an edge that rounding could carry it over, as a share of the
    mass it is compared with - u against both ends of the token's interval (not against 0 at u = 0, where the first
    positive weight wins for any rounding, and not against the end of the nucleus, which the walk
    cannot leave), p times the candidates' mass against the cumulative masses on both sides of the
    cut (with a one-token nucleus: only the one above).  ``boundary``: more ids hold the last
    candidate's value than there are places for it."""
    l = np.asarray(l, dtype=np.float64)
    order = stable_order(l) if order is None else order
    if T <= 0:
        return int(order[0]), (1.0, 1.0), bool(l.size > 1 and l[order[1]] == l[order[0]])
    full = k <= 0 or k > MAX_TOP_K
    m = members(l, order, k)
    cand = order[:m]
    boundary = bool(m < l.size and l[order[m]] == l[cand[-1]])
    with np.errstate(over="ignore", under="ignore"):
        w = np.exp((l[cand] - l[cand[0]]) / T)
    cum = np.cumsum(w)
    keep, margin, mp = m, 1.0, 1.0
    if p < 1.0:
        lim = p * cum[-1]
        keep = min(int(np.searchsorted(cum, lim, side="left")) + 1, m)
        mp = (cum[keep - 1] - lim) / cum[-1]
        if keep > 1:
            mp = min(mp, (lim - cum[keep - 2]) / cum[-1])
    nuc, wn = cand[:keep], w[:keep]
    if full:  # the draw walks the nucleus in vocabulary order
        o = np.argsort(nuc, kind="stable")
        nuc, wn = nuc[o], wn[o]
    c = np.cumsum(wn)
    t = u * c[-1]
    j = min(int(np.searchsorted(c, t, side="right")), keep - 1)
    last = int(np.nonzero(wn)[0][-1])
    if j < last:
        margin = min(margin, c[j] / c[-1] - u)
    if u > 0:
        margin = min(margin, u - (c[j - 1] / c[-1] if j else 0.0))
    return int(nuc[j]), (float(margin), float(mp)), boundary


def u_for(l, T, k, p, j, order, token=None):
    """u at the midpoint of the interval of rank j of the draw order (a candidate rank, or a rank
    in vocabulary order for a full row - or there the rank of ``token``), on the 24-bit grid; and
    the interval."""
    l = np.asarray(l, dtype=np.float64)
    m = members(l, order, k)
    cand = order[:m]
    with np.errstate(over="ignore", under="ignore"):
        w = np.exp((l[cand] - l[cand[0]]) / T)
    cum = np.cumsum(w)
    keep = m if p >= 1.0 else min(int(np.searchsorted(cum, p * cum[-1], side="left")) + 1, m)
    nuc, wn = cand[:keep], w[:keep]
    if k <= 0 or k > MAX_TOP_K:
        o = np.argsort(nuc, kind="stable")
        nuc, wn = nuc[o], wn[o]
        if token is not None:
            j = int(np.searchsorted(nuc, token))
    c = np.cumsum(wn) / wn.sum()
    j = j % keep
    lo, hi = (float(c[j - 1]) if j else 0.0), float(c[j])
    return round((lo + hi) / 2 * 2 ** 24) / 2 ** 24, lo, hi


def p_for(l, T, k, keep, order):
    """top_p (an fp32 number) at the midpoint between the cumulative masses on either side of a
    cut that keeps ``keep`` candidates."""
    l = np.asarray(l, dtype=np.float64)
    cand = order[:members(l, order, k)]
    with np.errstate(over="ignore", under="ignore"):
        cum = np.cumsum(np.exp((l[cand] - l[cand[0]]) / T))
    lo = cum[keep - 2] if keep > 1 else 0.0
    return f32((lo + cum[keep - 1]) / 2 / cum[-1])


# ------------------------------------------------------------------ logits --

def _gen(key):
    return torch.Generator().manual_seed(zlib.crc32(key.encode()))


def planted_ids(V, per, variant):
    """(ids of the row maximum, ids that get the K-th rank's value)."""
    S = (V + per - 1) // per
    last = (S - 1) * per
    mx = {0: [300, 448, per - 1, per], 1: [0, V - 1], 2: [255, 256, last + 1, V - 2], 3: [7]}[variant]
    mx = sorted({i for i in mx if 0 <= i < V})
    kth = [255, 256, 300, 448, per - 1, per, 2 * per - 1, 2 * per, last, V - 3]
    return mx, sorted({i for i in kth if 0 <= i < V and i not in mx})


def make_row(key, V, per, k, variant, plateau=False):
    """One row of logits, float64 array of bf16 numbers.  ``plateau``: PLATEAU more ids, spread
    over the row, hold the K-th rank's value - more than sample_kernel's tie list takes."""
    g = _gen(key)
    l = torch.clamp(torch.round((6.0 + 3.5 * torch.randn(V, generator=g, dtype=torch.float64)) * 8) / 8,
                    -8.0, TOP_VALUE - 0.125).numpy()
    mx, kth = planted_ids(V, per, variant)
    l[mx] = l.max() + 0.125
    if 0 < k < V:
        if plateau:
            kth = sorted(set(kth) | set(range(3, V, max(1, V // PLATEAU))) - set(mx))
        l[kth] = np.sort(l)[V - k]  # the k-th largest: it stays the k-th largest
    assert np.array_equal(torch.from_numpy(l).to(torch.bfloat16).double().numpy(), l)
    return l


def runs(v):
    """[(start, length)] of the runs of equal values of a sorted array."""
    cut = np.flatnonzero(np.diff(v)) + 1
    starts = np.concatenate(([0], cut))
    return list(zip(starts.tolist(), np.diff(np.concatenate((starts, [v.size]))).tolist()))


# ------------------------------------------------------------------- kinds --

CAND_KINDS = ("first", "maxhi", "tie_lo", "rank_last", "cut_between", "cut_inside", "cut_first", "u0", "utop",
              "utop_cut", "p_tiny", "tiny40_lo", "tiny40_hi", "tiny40_u0", "tiny6_lo", "tiny6_hi", "hot_last",
              "hot_cut", "greedy", "plateau_last", "plateau_lo")
SEEDABLE = ("first", "maxhi", "tie_lo", "cut_inside", "cut_first", "p_tiny", "tiny40_lo", "tiny40_hi", "tiny6_hi",
            "hot_cut", "greedy")
FULL_KINDS = ("p1_lo", "p1_hi", "pcut_lo", "pcut_hi", "u0", "utop", "p_tiny", "tiny40_hi", "tiny6_lo")
FULL_SEEDABLE = ("p1_lo", "p1_hi", "pcut_lo", "pcut_hi", "p_tiny", "tiny40_hi")
# which planted maximum a kind needs (else: by row); 3 is a maximum no other id shares
VARIANT_CAND = {"maxhi": 0, "tiny40_lo": 2, "tiny40_hi": 0, "tiny40_u0": 2, "tiny6_lo": 0, "tiny6_hi": 2, "first": 3}
VARIANT_FULL = {"p1_lo": 1, "p1_hi": 1, "utop": 1, "u0": 1, "hot_lo": 1, "hot_hi": 1}


def variant_of(kind, k, i):
    return (VARIANT_CAND if 0 < k <= MAX_TOP_K else VARIANT_FULL).get(kind, i % 3)


def _group_cut(vals, start, inside):
    """A cut (number kept) at the first run of equal values that ends behind rank ``start``:
    behind the run (between two tie groups) or in its middle (inside one: a run of two at least)."""
    for s, n in runs(vals):
        if s + n <= start or (inside and n < 2):
            continue
        return s + (n + 1) // 2 if inside else s + n
    return 1 if inside else vals.size


def solve(l, k, kind, parity=0, seed=None):
    """The Row of (logits, top_k, kind): T, p and u from the reference alone.  ``seed``: u is not
    the midpoint but the first ``seeded_uniform(seed, index)`` that lies MARGIN inside the
    target's interval (the rows that go through ``Sampler.__call__``)."""
    order = stable_order(l)
    full = k <= 0 or k > MAX_TOP_K
    m = members(l, order, k)
    vals = l[order[:m]]
    gmax = int((vals == vals[0]).sum())
    if kind == "greedy":
        tok, margin, boundary = oracle(l, 0.0, k, 1.0, 0.5, order)
        return Row(kind, 0.0, k, 1.0, 0.5, tok, 1.0, True, boundary, None, 0)
    fixed = {"tiny40": 1e-40, "tiny6": 1e-6, "hot": 1e30}.get(kind.split("_")[0])
    if fixed is not None:
        ts = (fixed,)
    elif full:
        ts = TS_COLD if kind in ("p1_lo", "p1_hi", "utop", "u0") else TS_FULL
    else:
        ts = ((TS[1], TS[0]) + TS[2:] if parity else TS) + ((1e30,) if kind.startswith("utop") else ())
    need = TOP_NEED if kind.startswith("utop") else MARGIN
    margin = None
    for T in ts:
        T = f32(T)
        p, u, j, token = 1.0, None, 0, None
        if kind == "cut_between":
            keep = _group_cut(vals, max(1, m // 2), False)
            p, j = p_for(l, T, k, keep, order), keep - 1
        elif kind in ("cut_inside", "cut_first", "utop_cut", "pcut_lo", "pcut_hi"):
            keep = _group_cut(vals, min(4, m - 1) if full else m // 3, True)
            p, j = p_for(l, T, k, keep, order), (0 if kind in ("cut_first", "pcut_lo") else keep - 1)
        elif kind == "hot_cut":
            keep = m // 2 + 1
            p, j = p_for(l, T, k, keep, order), keep - 1
        elif kind == "p_tiny":
            p, u = f32(P_TINY), (0.75 if seed is None else seeded_uniform(seed, 0))
        if kind in ("maxhi", "tiny40_hi", "tiny6_hi"):
            j, token = min(gmax, m) - 1, int(order[gmax - 1])  # the highest id among the tied maxima
        elif kind in ("tiny40_lo", "tiny6_lo"):
            token = int(order[0])
        elif kind in ("tie_lo", "plateau_lo"):
            j = int(np.argmax(vals == vals[-1]))
        elif kind in ("rank_last", "hot_last", "plateau_last"):
            j = m - 1
        elif kind == "hot_mid":
            j = m // 2
        elif kind in ("p1_hi", "hot_hi"):
            j = -1  # the highest vocabulary id of the nucleus
        elif kind in ("u0", "tiny40_u0"):
            u = 0.0
        if kind.startswith("utop"):
            u = U_TOP
        lo = hi = None
        if u is None:
            u, lo, hi = u_for(l, T, k, p, j, order, token if full else None)
            if seed is not None:
                gi = next((g for g in range(100000) if lo + MARGIN < seeded_uniform(seed, g) < hi - MARGIN),
                          None)
                if gi is None:
                    continue
                u = seeded_uniform(seed, gi)
        gi = gi if seed is not None and lo is not None else 0
        tok, margin, boundary = oracle(l, T, k, p, u, order)
        if margin[0] >= need and margin[1] >= MARGIN:
            return Row(kind, T, k, p, u, tok, min(margin), True, boundary, seed, gi)
    raise AssertionError(f"no temperature of {ts} gives {kind} at top_k {k} its margin ({margin})")


# ---------------------------------------------------------------- launches --

def _catalog(V, full_kinds=FULL_KINDS, cand_kinds=CAND_KINDS):
    cand = [(k, kind) for kind in cand_kinds for k in KS]
    fullc = [(k, kind) for kind in full_kinds for k in (0, 1025, V - 1, V, V + 7)]
    if V <= 1024:  # uniform over a vocabulary this small still leaves every id 2^-10 of the mass
        fullc += [(k, kind) for kind in ("hot_lo", "hot_hi") for k in (0, 1025)]
    else:  # uniform over the 1025 members and the ties at their last value: every one of them counts
        fullc += [(1025, "hot_mid")]
    return cand, fullc


def build_launch(name, n, V, via="ops", mix="cand", start=0):
    """n rows of [n, V] logits, each with its own T, top_k, top_p and u.  ``mix``: "cand" (rows of
    the candidate kernels and greedy rows), "full" (full-vocabulary rows) or "all" (both)."""
    _, per = splits(n, V)
    if per == V:
        per = (V + 15) // 16
    seeded = via == "sampler"
    cand, fullc = _catalog(V, FULL_SEEDABLE, SEEDABLE) if seeded else _catalog(V)
    cat = {"cand": cand, "full": fullc, "all": [x for pair in zip(cand, fullc * 3) for x in pair]}[mix]
    rows, logits = [], np.empty((n, V), dtype=np.float32)
    for i in range(n):
        k, kind = cat[(start + i) % len(cat)]
        l = make_row(f"{name}/{i}", V, per, k, variant_of(kind, k, start + i), kind.startswith("plateau"))
        row = solve(l, k, kind, parity=(start + i) & 1, seed=1000 + i if seeded else None)
        rows.append(row)
        logits[i] = l
    full = any(r.T > 0 and (r.k <= 0 or r.k > MAX_TOP_K) for r in rows)
    return Launch(name, n, V, via, full, torch.from_numpy(logits), rows)


# name, n, V, via, mix, start: `start` rotates the catalog so the small launches differ
SPECS = [
    ("one-n64-V1000", 64, 1000, "ops", "cand", 0),
    ("one-n64-V4096", 64, 4096, "ops", "cand", 31),
    ("one-n64-V32000", 64, 32000, "ops", "cand", 62),
    ("two-n63-V32000", 63, 32000, "ops", "cand", 17),
    ("two-n63-V4096", 63, 4096, "ops", "cand", 80),
    ("two-n63-V1000", 63, 1000, "ops", "cand", 17),   # K > V: stage 2 selects among -inf padding
    ("full-n64-V4096", 64, 4096, "ops", "full", 0),
    ("full-n64-V1000", 64, 1000, "ops", "full", 23),
    ("full-n4-V131080", 4, 131080, "ops", "full", 7),
    ("mixed-n64-V32000", 64, 32000, "ops", "all", 5),
    ("mixed-n8-V128256-sampler", 8, 128256, "sampler", "all", 3),
    ("mixed-n64-V4096-sampler", 64, 4096, "sampler", "all", 0),
]
_TWO_V = (1000, 4096, 32000, 128256, 131072, 131080)
SPECS += [(f"two-n1-V{V}", 1, V, "ops", "cand", 11 * i + 4) for i, V in enumerate(_TWO_V)]
SPECS += [(f"two-n4-V{V}", 4, V, "ops", "cand", 13 * i + 40) for i, V in enumerate(_TWO_V)]
NAMES = [s[0] for s in SPECS]
_CACHE = {}


def launch(name):
    """The Launch of a name, built once per process: the GPU runs the very rows whose margins the
    CPU test asserts."""
    if name not in _CACHE:
        _CACHE[name] = build_launch(*SPECS[NAMES.index(name)])
    return _CACHE[name]


# ---------------------------------------------------------------- back ends --

def run_reference(la):
    """``sample_reference`` / ``Sampler`` on the CPU: the contract itself."""
    return _run(la, torch.device("cpu"))


def _run(la, device):
    x = la.logits.to(device)
    if la.via == "sampler":
        params = [SamplingParams(temperature=r.T, top_k=r.k, top_p=r.p, seed=r.seed) for r in la.rows]
        out = Sampler(device, seed=5)(x, params, gen_index=[r.gen_index for r in la.rows])
    else:
        from mlopamd import ops

        t = lambda v, dt: torch.tensor(v, dtype=dt).to(device)  # noqa: E731
        out = ops.sample(x, t([r.T for r in la.rows], torch.float32), t([r.k for r in la.rows], torch.int32),
                         t([r.p for r in la.rows], torch.float32), t([r.u for r in la.rows], torch.float32),
                         full=la.full)
    return out.cpu().tolist()


def probe(la, run=None, device=None, info=None, repeats=REPEATS):
    """Messages of a launch issued REPEATS times: every row's token == the oracle's, and the
    repeats identical.  ``run``: launch -> token list (default: the ops on ``device``)."""
    run = run or (lambda la: _run(la, device))
    outs = [run(la) for _ in range(repeats)]
    msgs = []
    if any(o != outs[0] for o in outs[1:]):
        bad = sorted({i for o in outs[1:] for i in range(la.n) if o[i] != outs[0][i]})
        msgs.append(f"{la.name}: {len(bad)} rows differ between {REPEATS} identical launches, first row {bad[0]} "
                    f"({la.rows[bad[0]].kind}, top_k {la.rows[bad[0]].k}): {[o[bad[0]] for o in outs]}")
    wrong = [i for i in range(la.n) if outs[0][i] != la.rows[i].expect]
    for i in wrong[:4]:
        r = la.rows[i]
        l = la.logits[i]
        msgs.append(f"{la.name} row {i} ({r.kind}, T {r.T:g}, top_k {r.k}, top_p {r.p:.7g}, u {r.u:.8f}): got token "
                    f"{outs[0][i]} (logit {float(l[outs[0][i]]) if 0 <= outs[0][i] < la.V else 'out of range'}), "
                    f"expected {r.expect} (logit {float(l[r.expect])}); margin {r.margin:.3g}")
    if len(wrong) > 4:
        msgs.append(f"{la.name}: {len(wrong)} of {la.n} rows wrong")
    if info is not None:
        info.update(figures(la), wrong=len(wrong), wrong_kinds=sorted({la.rows[i].kind for i in wrong}))
    return msgs


def figures(la):
    """The conditions that keep a launch sensitive, from the reference alone."""
    return {"min_margin": min(r.margin for r in la.rows),
            "margin_ok": all(r.ok and r.margin >= MARGIN for r in la.rows),
            "boundary_rows": sum(r.boundary for r in la.rows)}
