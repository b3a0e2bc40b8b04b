"""The multi-LoRA probes of tests/lora_probes.py, without a GPU: the case lists reach every form
of the shrink's K loop, every R and every slot pattern, the builders alone meet the conditions that
keep the probes sensitive, the CPU definitions of the ops pass every probe, and every fault of the
restated kernels fails at least one (profiles/lora_probes.md holds the table this file prints with
``python tests/test_lora_probes_cpu.py``)."""
import pytest
import torch

import lora_probes as lp

bf = torch.bfloat16
CPU = torch.device("cpu")


# ------------------------------------------------------------ 1. coverage --

def test_the_k_list_reaches_every_form_of_the_loop():
    forms = {K: lp.shrink_form(K) for K in lp.SHRINK_KS}
    assert forms[128] == (0, 0, 1) and forms[384] == (0, 0, 3) and forms[512] == (0, 1, 0)
    assert forms[640] == (0, 1, 1) and forms[896] == (0, 1, 3) and forms[1024] == (1, 1, 0)
    assert forms[1152] == (1, 1, 1) and forms[1920] == (2, 1, 3) and forms[4096] == (7, 1, 0)
    assert forms[14336] == (27, 1, 0)
    seen = {(min(m, 2), t) for m, d, t in forms.values()}
    assert seen >= {(m, t) for m in (0, 1, 2) for t in (0, 1, 3)}, seen
    # without a main trip: with and without the prologue + drain
    assert {(d, t) for m, d, t in forms.values() if m == 0} >= {(0, 1), (0, 3), (1, 0), (1, 1), (1, 3)}
    # the mirror against the kernel's own loop
    for K in range(128, 4097, 128):
        steps, st, main = K // 128, 0, 0
        if steps >= lp.U:
            while st + 2 * lp.U <= steps:
                st, main = st + lp.U, main + 1
            st += lp.U
        assert lp.shrink_form(K) == (main, int(steps >= lp.U), steps - st), K


def test_shrink_cases_hold_what_the_issue_lists():
    keys = {(c.K, c.T, c.G, c.R) for c in lp.SHRINK_CASES}
    for K in (128, 384, 512, 640, 896, 1024, 1152, 1920, 4096, 14336):
        assert {(K, 17, 3, 64), (K, 17, 2, 48)} <= keys
    for K in (512, 1152):
        assert {(K, 17, G, R) for G in (1, 2, 3) for R in (16, 32, 48, 64)} <= keys
        assert {T for k, T, G, R in keys if k == K} == {1, 15, 16, 17, 33}
    assert max(lp.shrink_bytes(c) for c in lp.SHRINK_CASES) == 17 * 192 * 14336 * 2
    assert sorted(lp.shrink_bytes(c) for c in lp.SHRINK_CASES)[-2] < 50 << 20


def test_expand_cases_hold_what_the_issue_lists():
    keys = {(c.N, c.T, c.G, c.R, c.strided) for c in lp.EXPAND_CASES}
    assert {c.N for c in lp.EXPAND_CASES} == {16, 48, 64, 80, 768, 1024}
    assert {(c.G, c.R) for c in lp.EXPAND_CASES} == set(lp.GR_PAIRS)
    assert {c.T for c in lp.EXPAND_CASES} == {1, 15, 16, 17, 33}
    for N in (16, 48, 64, 80, 768, 1024):
        assert {R for n, T, G, R, st in keys if n == N} >= {16, 48, 64}  # the !in path at every N
        assert any(st for n, T, G, R, st in keys if n == N)
    assert [lp.expand_blocks(N) for N in (16, 48, 64, 80)] == [(1, 1), (1, 3), (1, 4), (2, 1)]
    assert lp.tile_groups(768, 3).tolist() == [0] * 32 + [1] * 8 + [2] * 8
    assert lp.tile_groups(1024, 2).tolist() == [0, 1] * 32
    for N in (48, 64, 80):  # the group changes inside a block of 64 columns
        assert len(set(lp.tile_groups(N, 3).tolist()[:4])) > 1
    for c in lp.EXPAND_CASES:
        assert int(lp.tile_groups(c.N, c.G).max()) <= c.G - 1
    assert {(c.K, c.T > 16) for c in lp.CHAIN_CASES} >= {(512, True), (1152, True)}


def test_slot_patterns():
    assert len(lp.RANKS) == lp.S == 17 and set(lp.RANKS) == set(lp.RANK_VALUES)
    tiles = {}
    for T in lp.TS:
        for v in range(lp.VARIANTS):
            sl = lp.tok_slots(T, v)
            assert len(sl) == T
            for t0 in range(0, T, 16):
                tiles.setdefault(T, []).append(sl[t0:t0 + 16])
    full = [t for T in (16, 17, 33) for t in tiles[T] if len(t) == 16]
    assert any(len(set(t)) == 16 and all(0 <= s < 16 for s in t) for t in full)        # 16 distinct slots
    assert any(set(t) == {-1} for t in full) and any(set(t) == {lp.ONE_SLOT} for t in full)
    runs = [t for t in full if set(lp.OUT_OF_RANGE) <= set(t)]
    assert runs and all(-1 in t and t[0] == t[1] != t[3] == t[4] == t[5] for t in runs)
    for T in (17, 33):  # the last, partial tile holds a slot of its own
        for v in range(lp.VARIANTS):
            sl = lp.tok_slots(T, v)
            assert sl[T - 1] == lp.LAST_SLOT and lp.LAST_SLOT not in sl[:T // 16 * 16]
    # every rank value is in use at R = 64, tokens on a rank-0 slot and on ranks 17 and 33 among them
    used = {lp.RANKS[s] for T in (16, 17, 33) for t in tiles[T] for s in t if 0 <= s < lp.S}
    assert used == set(lp.RANK_VALUES)
    assert lp.slot_ranks(48)[8] == 48 and lp.slot_ranks(16)[4] == 16 and lp.slot_ranks(32)[6] == 32


def test_selector_plans_visit_what_they_must():
    for c in lp.SHRINK_CASES:
        K, kq = c.K, c.K // 4
        cols = lp.selector_columns(K)
        for q in range(4):
            assert set(range(q * kq, q * kq + 8)) | set(range((q + 1) * kq - 8, (q + 1) * kq)) <= set(cols)
            vecs = {k // 8 for k in cols}
            for g0 in range(0, kq, 128):
                assert (q * kq + g0) // 8 in vecs and (q * kq + min(g0 + 128, kq)) // 8 - 1 in vecs
        seen, variants = set(), set()
        for variant, give in lp.shrink_selector_plan(c):
            tr = lp._meta(c.T, variant, c.R)[3]
            seen |= {give[t] for t in range(c.T) if tr[t] >= 1}
            variants.add(variant)
        assert seen >= set(cols) and variants == set(range(lp.VARIANTS)), c.id
    for c in lp.EXPAND_CASES:
        want = {(g, r) for g in range(c.G) for ch in range(c.R // 8) for r in (8 * ch, 8 * ch + 7)}
        seen = set()
        for variant, give in lp.expand_selector_plan(c):
            tr = lp._meta(c.T, variant, c.R)[3]
            seen |= {give[t] for t in range(c.T) if tr[t] > give[t][1]}
        assert seen >= want, c.id


# ------------------------------------- 2. the conditions of a sensitive probe --

def test_codes_differ_from_their_neighbours():
    A = lp.code_a(lp.S, 48, 1152)
    assert int(A.min()) >= -127 and int(A.max()) <= 127 and bool((A != 0).all())
    assert bool((A[1:] != A[:-1]).all()) and bool((A[:, 1:] != A[:, :-1]).all())
    for d in (1, 32, 128, 288):  # the next k, step, group of steps and quarter
        assert bool((A[:, :, d:] != A[:, :, :-d]).all()), d
    assert bool((lp.selector_a(lp.SHRINK_CASES[0]).float() == lp._zero_above_rank(
        lp.code_a(lp.S, 192, 128).view(lp.S, 3, 64, 128), 64).view(lp.S, 192, 128).float()).all())
    B = lp.code_b(80, 64)
    assert float(B.min()) >= -64 and float(B.max()) <= 64 and bool((B != 0).all())
    assert bool((B[1:] != B[:-1]).all()) and bool((B[:, 1:] != B[:, :-1]).all()) and bool((B[:, :, 1:] != B[:, :, :-1]).all())
    assert bool((B[:, 16:] != B[:, :-16]).all()) and bool((B[:, :, 8:] != B[:, :, :-8]).all())
    assert bool((B[:, :, 32:] != B[:, :, :-32]).all()) and bool((B[:, :, 16:] != B[:, :, :-16]).all())


def test_integer_data_keeps_the_contract_and_shows_a_rounded_tmp():
    for c in lp.SHRINK_CASES:
        if c.K > 2048:
            continue
        x, A = lp.shrink_inputs(c)
        assert float(x.abs().max()) <= 4 and float(A.abs().max()) <= 4 and 16 * c.K < 2 ** 24
        A4 = A.view(lp.S, c.G, c.R, c.K)
        for s, r in enumerate(lp.slot_ranks(c.R)):
            assert bool((A4[s, :, r:] == 0).all()) and (r == 0 or bool((A4[s, :, r - 1] != 0).any()))
        for v in range(lp.VARIANTS):
            slots = lp.tok_slots(c.T, v)
            e = lp.shrink_expect(x[v], A, slots)
            if any(0 <= s < lp.S and lp.slot_ranks(c.R)[s] for t, s in enumerate(slots) if t % 4 == 0):
                assert bool((e.float().to(bf).double() != e).any()), (c.id, v)


def test_isolation_has_a_poisoned_neighbour_in_a_checked_tile():
    for T in (15, 16, 17, 33):
        hit = 0
        for v in range(lp.VARIANTS):
            slots = lp.tok_slots(T, v)
            exact, x_bad = lp.isolation_rows(slots)
            for t0 in range(0, T, 16):
                tile = slots[t0:t0 + 16]
                ok = lp.valid(tile)
                checked = [t for t in range(len(tile)) if ok[t] and bool(exact[t0 + t])]
                hit += bool(checked) and lp.POISON_SLOT in tile and any(not o for o in ok) or 0
                assert not (ok[1] if len(tile) > 1 else False) or not bool(exact[t0 + 1])
        assert hit >= 1, T


def test_the_worked_example_of_the_split():
    """v = 1 + 2^-9 + 2^-15 + 2^-23, b = 1, y0 = -(1 - 2^-7): 161, 160 and 128 units of 2^-14."""
    v = torch.tensor([1 + 2.0 ** -9 + 2.0 ** -15 + 2.0 ** -23])
    assert lp.split_value(1) == (float(v), -(1 - 2.0 ** -7))
    h, m, l = (p.float() for p in lp.split3(v))
    assert float(h) == 1 and float(m) == 2.0 ** -9 + 2.0 ** -15 and float(l) == 2.0 ** -23
    y0 = -(1 - 2.0 ** -7)
    units = [float((y0 + s).to(bf)) * 2 ** 14 for s in (h + m + l, h + m, h)]
    assert units == [161, 160, 128]


def test_split_and_rounding_builders():
    planted = 0
    for c in lp.EXPAND_CASES:
        for v in range(lp.VARIANTS):
            planted += lp.split_conditions(c, v)
    assert planted > 0
    seen = set()
    for i in range(48):
        v, y = lp.split_value(i)
        seen.add((v > 0, int(torch.tensor(abs(v)).log2().floor())))
    assert len(seen) == 8  # four binades, both signs
    assert [float(torch.tensor(a + b, dtype=torch.float64).float().to(bf)) for a, b in lp.PLANTS] == list(lp.PLANT_ROUNDED)
    assert float(torch.tensor(257.0).to(bf)) == 256 and float(torch.tensor(258.0).to(bf)) == 258


# ------------------------------------------- 3. the CPU definitions pass --

def _run_all(be, shrink_cases, expand_cases, chain_cases):
    out = []
    for cases, probes in ((shrink_cases, lp.SHRINK_PROBES), (expand_cases, lp.EXPAND_PROBES)):
        for case in cases:
            for name, fn in probes.items():
                if fn(case, be, CPU):
                    out.append(f"{case.id.split('-')[0]}/{name} {case.id}")
    for case in chain_cases:
        if lp.probe_chain(case, be, CPU):
            out.append(f"chain {case.id}")
    return out


@pytest.mark.parametrize("case", lp.SHRINK_CASES, ids=[c.id for c in lp.SHRINK_CASES])
def test_reference_shrink(case):
    be = lp.RefBackend()
    for name, fn in lp.SHRINK_PROBES.items():
        info = {}
        msgs = fn(case, be, CPU, info)
        assert not msgs, "\n".join(msgs)
        assert info["checked"] > 0


@pytest.mark.parametrize("case", lp.EXPAND_CASES, ids=[c.id for c in lp.EXPAND_CASES])
def test_reference_expand(case):
    be = lp.RefBackend()
    for name, fn in lp.EXPAND_PROBES.items():
        msgs = fn(case, be, CPU)
        assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", lp.CHAIN_CASES, ids=[c.id for c in lp.CHAIN_CASES])
def test_reference_chain(case):
    msgs = lp.probe_chain(case, lp.RefBackend(), CPU)
    assert not msgs, "\n".join(msgs)


def test_reference_empty_launches_and_out_of_range_slots():
    assert not lp.probe_empty(lp.RefBackend(), CPU)
    from mlopamd import ops

    ts = torch.tensor(list(lp.OUT_OF_RANGE) + [-1, 2], dtype=torch.int64).to(torch.int32)
    A, x = torch.ones(lp.S, 16, 128, dtype=bf), torch.ones(7, 128, dtype=bf)
    sr = torch.full((lp.S,), 16, dtype=torch.int32)
    tmp = ops.lora_shrink(x, A, ts, sr)
    assert bool((tmp[:6] == 0).all()) and bool((tmp[6] == 128).all())
    y = torch.full((7, 16), 3.0, dtype=bf)
    ops.lora_expand_add(y, tmp, torch.ones(lp.S, 16, 16, dtype=bf), torch.zeros(1, dtype=torch.uint8), ts, sr)
    assert bool((y[:6] == 3).all()) and bool((y[6] == 3 + 16 * 128).all())


# ---------------------------------------------------------- 4. fault table --

def _pick(cases, *ids):
    by = {c.id: c for c in cases}
    return [by[i] for i in ids]


# the cases a fault runs on: small ones of every form it can show on
FAULT_SHRINK_CASES = _pick(lp.SHRINK_CASES, "shrink-K384-T17-G2-R48", "shrink-K640-T17-G3-R64", "shrink-K1152-T33-G3-R64",
                           "shrink-K512-T17-G1-R16")
FAULT_EXPAND_CASES = _pick(lp.EXPAND_CASES, "expand-N80-T17-G2-R48", "expand-N80-T33-G3-R64", "expand-N48-T17-G1-R16",
                           "expand-N64-T33-G3-R16-strided")
FAULT_CHAIN_CASES = _pick(lp.CHAIN_CASES, "chain-K512-N48-T15-G1-R32")


def caught_by(fault):
    """The probes (``family/probe case``) that fail on the back end with this fault."""
    be = lp.Faulty(fault)
    shrink = fault is None or fault in lp.SHRINK_FAULTS + lp.SLOT_FAULTS + ["row_t_written"]
    expand = fault is None or fault in lp.EXPAND_FAULTS + lp.SLOT_FAULTS + ["row_t_written"]
    return _run_all(be, FAULT_SHRINK_CASES if shrink else [], FAULT_EXPAND_CASES if expand else [],
                    FAULT_CHAIN_CASES if fault is None else [])


def test_the_restated_kernels_pass_without_a_fault():
    assert caught_by(None) == []


@pytest.mark.parametrize("fault", lp.ALL_FAULTS)
def test_every_fault_fails_a_probe(fault):
    hits = caught_by(fault)
    print(fault, hits)
    assert hits, fault


if __name__ == "__main__":
    letters = {c.id.split("-", 1)[1]: chr(97 + i) for i, c in enumerate(FAULT_SHRINK_CASES)}
    letters.update({c.id.split("-", 1)[1]: chr(112 + i) for i, c in enumerate(FAULT_EXPAND_CASES)})
    print("cases: " + ", ".join(f"{v} = {k}" for k, v in letters.items()))
    print()
    print("| fault | caught by (probe: cases) |")
    print("|---|---|")
    for fault in lp.ALL_FAULTS:
        by_probe = {}
        for hit in caught_by(fault):
            probe, case = hit.split(" ")
            by_probe.setdefault(probe, []).append(letters[case.split("-", 1)[1]])
        cells = [p + ": " + " ".join(c) for p, c in by_probe.items()]
        print(f"| {fault} | {'; '.join(cells) or 'MISSED'} |")
