"""The sampler probes of tests/sampler_probes.py, without a GPU: ``sample_reference`` (the
contract) passes every one, the reference alone meets the conditions that keep them sensitive
(MARGIN on 100 % of the rows, contested K-th places, every kind on both paths), and an emulator
of the three kernels' structure in plain numpy with ONE fault injected fails them.  The same
faults against the inputs and the 1e-5 allowance of test_kernels_gpu.py's
test_sample_matches_reference give the table of profiles/sampler_probes.md, printed by
``python tests/test_sampler_probes_cpu.py``."""
import numpy as np
import pytest
import torch

import sampler_probes as sp
from mlopamd.runtime.sampler import MAX_TOP_K, sample_reference

OPS = [n for n in sp.NAMES if not n.endswith("sampler")]


# ------------------------------------------------ 1. the reference passes --

@pytest.mark.parametrize("name", sp.NAMES)
def test_reference_passes_every_probe(name):
    la = sp.launch(name)
    info = {}
    msgs = sp.probe(la, run=sp.run_reference, info=info)
    print(name, info)
    assert info["margin_ok"] and info["min_margin"] >= sp.MARGIN, (name, info)  # every row: none is skipped
    assert not msgs, "\n".join(msgs)


def test_reference_orders_equal_logits_by_lower_id():
    """The stated contract on rows small enough to read."""
    l = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 1.0]] * 6)
    t = lambda v, dt=torch.float32: torch.tensor(v, dtype=dt)  # noqa: E731
    T = t([0.0, 1.0, 1.0, 1.0, 1e-40, 1e30])
    k = t([0, 1, 2, 2, 4, 4], torch.int32)
    p = t([1.0, 1.0, 1.0, 0.4, 1.0, 1.0])
    u = t([0.5, 0.99, 0.75, 0.99, 0.5, 0.8])
    # greedy; top_k 1: the lowest tied id; top_k 2: ids 1 and 2, the second half is id 2; top_p 0.4
    # cuts inside the tie group and keeps id 1; T -> 0+: uniform over the three maxima (the fourth
    # candidate, id 0, weighs 0); T = 1e30: uniform over the candidates 1, 2, 4, 0
    assert sample_reference(l, T, k, p, u).tolist() == [1, 1, 2, 1, 2, 0]
    # the full path keeps every tie at the k-th value (k = 1025 > V: all) and walks in vocabulary order
    full = sample_reference(l[:2], t([1e-40, 1e-40]), t([0, 1025], torch.int32), t([1.0, 1.0]), t([0.9, 0.1]))
    assert full.tolist() == [4, 1]


# ------------------------------- 2. the conditions of a sensitive probe --

def ties_at_last(la, i):
    """How many ids hold the value of row i's last candidate."""
    l = la.logits[i].double().numpy()
    order = sp.stable_order(l)
    return int((l == l[order[sp.members(l, order, la.rows[i].k) - 1]]).sum())


def test_rows_are_tied_and_cover_both_paths():
    seen = {1: set(), 2: set()}
    listed = {1: 0, 2: 0}
    for name in OPS:
        la = sp.launch(name)
        path = 1 if sp.splits(la.n, la.V)[0] == 1 else 2
        for i, r in enumerate(la.rows):
            l = la.logits[i]
            assert torch.equal(l.to(torch.bfloat16).float(), l)          # the LM head's numbers
            assert l.unique().numel() <= 225                             # eighths in [-8, 20]: ties everywhere
            if 0 < r.k <= MAX_TOP_K:
                seen[path].add((r.k, r.kind))
                if r.T > 0 and r.k < la.V - 1:
                    assert r.boundary, (name, i, r)                      # the K-th place is contested
                if r.kind.startswith("plateau") and la.V >= 4096:
                    listed[path] += ties_at_last(la, i) > MAX_TOP_K
    want = {(k, kind) for kind in sp.CAND_KINDS for k in sp.KS}
    assert want <= seen[1] and want <= seen[2], (want - seen[1], want - seen[2])
    assert min(listed.values()) >= 2, listed  # more ties than sample_kernel's tie list holds, on both paths


def test_full_rows_cover_every_top_k_with_and_without_top_p():
    seen = set()
    for name in OPS:
        la = sp.launch(name)
        for r in la.rows:
            if r.T > 0 and (r.k <= 0 or r.k > MAX_TOP_K):
                seen.add(("0" if r.k == 0 else "1025" if r.k == 1025 else f"V{r.k - la.V:+d}", r.p < 1.0))
    assert seen == {(k, c) for k in ("0", "1025", "V-1", "V+0", "V+7") for c in (False, True)}, seen


def test_slice_arithmetic_of_the_cases():
    """The shapes sit where sample_splits changes: full 8192-float slices, a 17th slice, a slice
    shorter than K, a vocabulary shorter than K."""
    assert sp.splits(4, 131072) == (16, 8192) and sp.splits(4, 131080)[0] == 17
    assert sp.splits(4, 4096) == (16, 256) and sp.splits(63, 32000) == (5, 6400)
    assert sp.splits(64, 32000) == (1, 32000) and sp.splits(1, 1000) == (16, 63)


# ---------------------------------------- 3. an emulator with one fault --

FAULTS = {
    "bound_hi": "boundary ties taken from the highest ids",
    "k_minus": "K - 1 candidates",
    "k_plus": "K + 1 candidates",
    "drop_slice": "one slice's candidates dropped",
    "drop_last": "the last, short slice dropped",
    "trunc_short": "a slice shorter than K truncated",
    "desc_ties": "ties drawn in descending-id order",
    "cut_short": "top-p cut one candidate short",
    "cut_long": "top-p cut one candidate long",
    "p_unnorm": "top-p against the unrenormalised mass",
    "top_pad": "u at the top returns padding (id 0)",
    "greedy_hi": "greedy returns the highest tied id",
    "full_drop_ties": "full path: ties at the K-th value dropped (top_k > 1024)",
    "full_nuc_hi": "full path: nucleus ties taken from the highest ids",
    "nan_tiny_T": "NaN prefix sum at a subnormal T",
}


def top_of(ids, l, K, hi=False):
    """The K of ``ids`` (ascending) that a select keeps, as a set: by value, ties at the K-th value
    to the lowest ids (``hi``: to the highest)."""
    o = ids[np.argsort(-l[ids], kind="stable")]
    if K >= o.size or not hi:
        return o[:K]
    gt, eq = o[l[o] > l[o[K - 1]]], o[l[o] == l[o[K - 1]]]
    return np.concatenate((gt, eq[::-1][:K - gt.size]))


def weights(l, ids, T):
    d = l[ids] - l[ids].max()
    with np.errstate(over="ignore", under="ignore"):
        return np.where(d == 0, 1.0, np.exp(d / T))


def emulate_row(l, T, k, p, u, n, fault=None):
    """sampling.hip's structure on one row: slices, per-slice top-K, union, select, sort, scan, cut
    and walk; the full path's members, nucleus and walk in vocabulary order."""
    V = l.size
    S, per = sp.splits(n, V)
    greedy = T <= 0
    with np.errstate(over="ignore", divide="ignore"):
        inv_t_finite = greedy or bool(np.isfinite(np.float32(1) / np.float32(T)))
    if not greedy and (k <= 0 or k > MAX_TOP_K):
        order = sp.stable_order(l)
        if fault == "nan_tiny_T" and not inv_t_finite:
            return int(order[0])
        m = k if fault == "full_drop_ties" and MAX_TOP_K < k < V else sp.members(l, order, k)
        cand = order[:m]
        cum = np.cumsum(weights(l, cand, T))
        keep = m if p >= 1 else min(int(np.searchsorted(cum, p * cum[-1], side="left")) + 1, m)
        nuc = cand[:keep]
        if fault == "full_nuc_hi" and p < 1:
            v = l[cand[keep - 1]]
            gt, eq = nuc[l[nuc] > v], cand[l[cand] == v]
            nuc = np.concatenate((gt, eq[::-1][:keep - gt.size]))
        nuc = np.sort(nuc)
        c = np.cumsum(weights(l, nuc, T))
        return int(nuc[min(int(np.searchsorted(c, u * c[-1], side="right")), keep - 1)])
    hi = fault == "bound_hi" or (greedy and fault == "greedy_hi")
    K = 1 if greedy else min(k, MAX_TOP_K)
    ids = np.arange(V)
    if S > 1:  # stage 1: every slice's own top-K, written in index order
        parts, last = [], (V - 1) // per
        for s in range(S):
            sl = ids[s * per:(s + 1) * per]
            if (fault == "drop_slice" and s == 1) or (fault == "drop_last" and s == last) or not sl.size:
                continue
            Ks = sl.size - 1 if fault == "trunc_short" and sl.size < K else min(K, sl.size)
            parts.append(np.sort(top_of(sl, l, Ks, hi)))
        ids = np.concatenate(parts)
    if greedy:
        return int(top_of(ids, l, 1, hi)[0])
    K = {"k_minus": max(1, K - 1), "k_plus": K + 1}.get(fault, K)
    cand = np.sort(top_of(ids, l, min(K, ids.size), hi))
    if fault == "desc_ties":
        cand = cand[::-1]
    cand = cand[np.argsort(-l[cand], kind="stable")]
    if fault == "nan_tiny_T" and not inv_t_finite:
        return int(cand[-1])  # both searches fall through to the last candidate
    scan = np.cumsum(weights(l, cand, T))
    lim = p * scan[-1] if p < 1 else scan[-1]
    if fault == "p_unnorm" and p < 1:
        lim = p * weights(l, np.arange(V), T).sum()
    cut = min(int(np.searchsorted(scan, lim, side="left")), cand.size - 1)
    if p < 1:
        cut = {"cut_short": max(0, cut - 1), "cut_long": min(cand.size - 1, cut + 1)}.get(fault, cut)
    if fault == "top_pad" and u >= sp.U_TOP:
        return 0
    return int(cand[min(int(np.searchsorted(scan[:cut + 1], u * scan[cut], side="right")), cut)])


def emulator(fault=None):
    def run(la):
        x = la.logits.double().numpy()
        return [emulate_row(x[i], r.T, r.k, r.p, r.u, la.n, fault) for i, r in enumerate(la.rows)]
    return run


def test_the_clean_emulator_passes_every_probe():
    for name in sp.NAMES:
        msgs = sp.probe(sp.launch(name), run=emulator(), repeats=1)
        assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("fault", FAULTS)
def test_one_fault_fails_a_probe(fault):
    failed = [name for name in OPS if sp.probe(sp.launch(name), run=emulator(fault), repeats=1)]
    print(fault, failed)
    assert failed, FAULTS[fault]


# ----------------- 4. the same faults against today's inputs and check --

LEGACY_SHAPES = [(16, 32000), (4, 128256), (64, 32000), (8, 1000)]


def legacy_inputs(n, V):
    """The inputs of test_sample_matches_reference (from a CPU generator): tie-free fp32
    3 randn, top_k in {0, 1, 50}, top_p in {1, 0.9, 0.5}, random u."""
    g = torch.Generator().manual_seed(1)
    x = 3 * torch.randn(n, V, generator=g)
    temps = torch.tensor([0.0, 0.7, 1.0, 1.3] * (n // 4))
    ks = torch.tensor([0, 1, 50, 0] * (n // 4), dtype=torch.int32)
    ps = torch.tensor([1.0, 1.0, 0.9, 0.5] * (n // 4))
    return x, temps, ks, ps, torch.rand(n, generator=g)


def legacy_rejects(x, temps, ks, ps, u, got, eps=1e-5):
    """The rows test_sample_matches_reference's check rejects: the drawn token must own the
    interval of the fp64 CDF that holds u; within eps of an edge the neighbour passes too."""
    n, V = x.shape
    kmax = min(MAX_TOP_K, V)
    xd = x.double()
    vals, idx = torch.topk(xd, kmax, dim=-1)
    bad = []
    for i in range(n):
        if float(temps[i]) <= 0 or int(ks[i]) == 1:
            if int(got[i]) != int(idx[i, 0]):
                bad.append(i)
            continue
        pp, ui, T = float(ps[i]), float(u[i]), float(temps[i])
        ok = False
        if int(ks[i]) == 0:
            w = torch.exp((xd[i] - xd[i].max()) / T)
            order = torch.sort(-xd[i], stable=True).indices
            cum = torch.cumsum(w[order], 0) / w.sum()
            keep0 = int((cum < pp).sum()) + 1 if pp < 1 else V
            keeps = {min(keep0, V)} | {kk for kk in (keep0 - 1, keep0 + 1)
                                       if pp < 1 and 1 <= kk <= V and abs(float(cum[kk - 1]) - pp) < eps}
            for keep in keeps:
                nuc = torch.zeros(V, dtype=torch.bool)
                nuc[order[:keep]] = True
                if not nuc[int(got[i])]:
                    continue
                c = torch.cumsum(w * nuc, 0) / (w * nuc).sum()
                j = int(got[i])
                ok |= (0.0 if j == 0 else float(c[j - 1])) - eps <= ui <= float(c[j]) + eps
        else:
            k = min(int(ks[i]), kmax)
            pr = torch.softmax(vals[i, :k] / T, dim=-1)
            c = torch.cumsum(pr, dim=-1)
            keeps = {k}
            if pp < 1.0:
                keep = min(int((c < pp).sum()) + 1, k)
                keeps = {keep} | {kk for kk in (keep - 1, keep + 1) if 1 <= kk <= k and abs(float(c[kk - 1]) - pp) < eps}
            for keep in keeps:
                cc = torch.cumsum(pr[:keep] / c[keep - 1], dim=-1)
                pos = (idx[i, :keep] == int(got[i])).nonzero()
                if pos.numel():
                    j = int(pos[0])
                    ok |= (0.0 if j == 0 else float(cc[j - 1])) - eps <= ui <= (1.0 if j == keep - 1 else float(cc[j])) + eps
        if not ok:
            bad.append(i)
    return bad


def legacy_run(fault, shapes=LEGACY_SHAPES):
    """Rows of today's inputs that today's check rejects under a fault, per shape."""
    out = {}
    for n, V in shapes:
        x, temps, ks, ps, u = legacy_inputs(n, V)
        xn = x.double().numpy()
        got = [emulate_row(xn[i], float(temps[i]), int(ks[i]), float(ps[i]), float(u[i]), n, fault) for i in range(n)]
        out[(n, V)] = len(legacy_rejects(x, temps, ks, ps, u, got))
    return out


def test_todays_inputs_let_the_tie_faults_through():
    """Why this suite exists: on tie-free randn rows the clean emulator passes today's check, and
    so does a sampler that breaks every tie the wrong way."""
    shapes = [(16, 32000), (8, 1000)]
    assert not any(legacy_run(None, shapes).values())
    for fault in ("bound_hi", "desc_ties", "greedy_hi", "full_nuc_hi", "nan_tiny_T", "trunc_short", "top_pad"):
        assert not any(legacy_run(fault, shapes).values()), fault


if __name__ == "__main__":
    print("| fault | rows today's check rejects, of 16 / 4 / 64 / 8 | probes that fail, of %d launches |" % len(OPS))
    print("|---|---|---|")
    for fault, text in FAULTS.items():
        legacy = legacy_run(fault)
        failed = [name for name in OPS if sp.probe(sp.launch(name), run=emulator(fault), repeats=1)]
        print(f"| {text} | {' / '.join(str(legacy[s]) for s in LEGACY_SHAPES)}"
              f"{'' if any(legacy.values()) else ' (let through)'} | {len(failed)} |")
