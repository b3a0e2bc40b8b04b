"""The row-kernel probes of tests/row_probes.py, without a GPU: the case lists reach every launch
form of the kernels, the reference alone meets the conditions that keep the probes sensitive,
the CPU definitions of the ops pass every probe, and small faulty variants of those definitions
each fail at least one (profiles/row_probes.md holds the table this file prints with
``python tests/test_row_probes_cpu.py``)."""
import pytest
import torch

import row_probes as rp

bf = torch.bfloat16
CPU = torch.device("cpu")
REF_BYTES = 32 << 20  # above this a case's membership launches are sampled on the CPU


# ------------------------------------------------------------ 1. coverage --

def test_norm_cases_reach_every_launch_form():
    forms = {(c.M, c.H): rp.norm_form(c.M, c.H) for c in rp.NORM_CASES}
    block = [f for f in forms.values() if f[0] == "block"]
    assert {f[1] for f in block} == {1, 2, 4, 8}
    idle = {rp.norm_form(M, H)[1] for (M, H) in forms if rp.last_wave_idle(M, H)}
    assert idle >= {2, 8}, idle
    assert forms[(2, 65536)] == ("block", 8, 1024)
    for vpl in (1, 2, 4, 8, 16):
        ms = [M for (M, H), f in forms.items() if f == ("wave", vpl)]
        assert 256 in ms and any(M % 4 for M in ms), (vpl, ms)
    assert any(M >= 256 and H % 512 and f[0] == "block" for (M, H), f in forms.items())
    assert forms[(257, 5120)][0] == "block"  # H / 512 = 10 is no wave form either
    # both forms of the op, the same shapes
    assert {(c.M, c.H) for c in rp.NORM_CASES if c.add} == {(c.M, c.H) for c in rp.NORM_CASES if not c.add}
    # the mirror against norm.hip's own numbers
    assert rp.norm_form(1, 4096) == ("block", 1, 512) and rp.norm_form(255, 8192) == ("block", 2, 512)
    assert rp.norm_form(256, 8192) == ("wave", 16) and rp.norm_form(4096, 14336) == ("block", 4, 448)


def test_membership_makes_every_vector_hot_and_launches_fit():
    for c in rp.NORM_CASES:
        cols = rp.hot_columns(c.H)
        assert {x // 8 for x in cols} == set(range(c.H // 8))
        assert set(range(8)) <= set(cols) and set(range(c.H - 8, c.H)) <= set(cols)
        L = rp.membership_rows(c.M, c.H)
        assert rp.norm_form(L, c.H) == rp.norm_form(c.M, c.H) and L * c.H * 2 <= rp.LAUNCH_BYTES
        if rp.norm_form(c.M, c.H)[0] == "wave":
            assert L >= 256 and L % 4 == c.M % 4 and (L + 1) // 2 >= len(cols)  # one launch
        elif c.M < 256:
            assert L == 254


def test_silu_cases_cross_the_grid_cap():
    assert max(rp.silu_vectors(c) for c in rp.SILU_CASES) > rp.SILU_CAP
    M, I = 293, 14336
    assert M * (I // 8) > rp.SILU_CAP >= (M - 1) * (I // 8)  # the smallest such M at this I
    for il in (0, 1):
        assert {(c.M, c.I) for c in rp.SILU_CASES if c.interleaved == il} >= {(1, 16), (3, 48), (37, 14336), (M, I)}
    assert any((c.I // 8) % 2 for c in rp.SILU_CASES)
    assert max(c.M * c.I for c in rp.SILU_CASES) >= rp.N_FINITE


def test_rope_cases_reach_both_grids_and_both_row_trips():
    bf16 = {rp.rope_blocks(c) for c in rp.ROPE_CASES if not c.fp8}
    assert {(1, 1), (2, 1), (2, 2)} <= bf16, bf16
    fp8 = {rp.rope_blocks(c) for c in rp.ROPE_CASES if c.fp8}
    assert {(2, 1, False), (2, 2, False), (2, 2, True)} <= fp8, fp8
    assert {c.D for c in rp.ROPE_CASES if not c.fp8} == {64, 128, 256}
    assert {c.strided for c in rp.ROPE_CASES if c.fp8} == {True, False}
    for f in (0, 1):
        assert {(c.Hq, c.Hkv, c.T) for c in rp.ROPE_CASES if c.fp8 == f and c.D == 128 and not c.strided} == \
            {(q, k, T) for q, k in rp.ROPE_GEOMETRIES for T in (1, 17, 33)}


def test_rope_meta_and_plants():
    placed_all = set()
    for c in rp.ROPE_CASES:
        qkv, pos, slots, NB, placed = rp.rope_inputs(c)
        assert NB == c.T // 16 + 8 and bool((qkv[:, :c.Hq * c.D] != 0).all())
        live = slots[slots >= 0].tolist()
        assert 0 not in live and len(set(live)) == len(live) and max(live) < NB * 16
        assert int(pos.max()) == 8191 and int(pos.min()) >= 0
        if c.T > 1:
            assert 0 in pos.tolist() and int(pos[3]) == int(pos[2]) + 1
            assert int(slots[5]) == int(slots[c.T - 1]) == -1 and int((slots < 0).sum()) == 2
            assert {48, 63} <= set(live)
        assert ("k", 14 / 8) in {(k[1], v) for k, v in placed.items()}
        placed_all |= {(k[1], v) for k, v in placed.items()}
    assert placed_all == set(rp.AMAX_PLANTS)
    for D in (64, 128, 256):
        cs = rp.selector_table(D)
        assert torch.unique(cs, dim=0).shape[0] == 8192
        body = torch.cat([cs[:rp.SCALE_POS], cs[rp.SCALE_POS + 1:]])
        assert bool(((body == 0) | (body.abs() == 1)).all()) and bool((body[:, :D // 2].abs() + body[:, D // 2:].abs() == 1).all())


def test_embedding_ids_hold_every_edge():
    for c in rp.EMB_CASES:
        ids = rp.emb_ids(c, CPU).tolist()
        assert len(ids) == c.T
        if c.T > 1:
            vs, ve = c.vocab_start, c.vocab_start + rp.EMB_ROWS
            assert {vs - 1, vs, ve - 1, ve, 0, rp.EMB_VOCAB - 1} <= set(ids) and len(set(ids)) < len(ids)
    t = rp.emb_table(5120, CPU)
    assert bool(torch.isfinite(t.float()).all()) and bool((t[:, 1:] != t[:, :-1]).all()) and bool((t[1:] != t[:-1]).all())


# ------------------------------------- 2. the conditions of a sensitive probe --

def test_norm_conditions():
    for H in sorted({c.H for c in rp.NORM_CASES}):
        assert rp.hot_is_stable(rp.HOT, H), H
        e = rp.eps_conditions(H)
        assert e[0] != e[1] and e[0] != e[2], (H, e)
        # a loud row: 16 rsqrt(256 + eps) rounds to 1, and 256 H is an exact fp32 sum
        assert float(rp._bf16_of(16 / (256 + rp.EPS) ** 0.5)) == 1.0 and 256 * H <= 2 ** 24
        # a vector left out of a one-hot row's sum, counted twice, or a loud vector leaking in
        c = float(rp._bf16_of(rp.hot_value(rp.HOT, H)))
        for wrong in (rp.HOT / rp.EPS ** 0.5, rp.hot_value(rp.HOT, H) / 2 ** 0.5, rp.HOT / ((4 + 8 * 256) / H + rp.EPS) ** 0.5):
            assert H == 8 or float(rp._bf16_of(wrong)) != c, (H, wrong)
    # data: squares are at most 64 and the sums stay below 2^24 (E x^2 = 24), exact in fp32 in any order
    gen = torch.Generator().manual_seed(0)
    assert float(rp.resid((4, 65536), gen).double().pow(2).sum(-1).max()) < 2 ** 24 and 64 * 65536 <= 2 ** 22


def _either_fraction(lo, hi):
    return float((lo != hi).double().mean())


def test_either_way_elements_are_rare():
    gen = torch.Generator().manual_seed(1)
    for H in (8, 4096, 65536):
        rows = 4096 // H + 2
        x, w = rp.resid((rows, H), gen), rp.norm_weights(H, gen)
        lo, hi, _ = rp.norm_either(x, w)
        assert _either_fraction(lo, hi) <= 0.01
    g, u = (3 * torch.randn(64, 4096, generator=gen)).to(bf), torch.randn(64, 4096, generator=gen).to(bf)
    lo, hi, _ = rp.silu_either(g, u)
    assert _either_fraction(lo, hi) <= 0.01


def test_silu_gate_rules_hold_for_the_reference_and_the_kernels_form():
    """Every finite bf16 gate at |u| in {0.5, 1}: torch's silu and the kernel's g / (1 + exp(-g)) in
    fp32 lie within the probe's bound; the flush rule is needed at a handful of gates only."""
    g = rp.finite_bf16(CPU)
    for u in (1.0, -0.5):
        exp = rp.silu_mul64(g.double(), torch.full_like(g, u).double())
        for s in (torch.nn.functional.silu(g.float()), g.float() / (1 + torch.exp(-g.float()))):
            out = (s.to(bf).float() * u).to(bf)
            bad = rp.ulp_bad(out, exp)
            assert int((bad & (g.double() >= rp.FLUSH_BELOW)).sum()) == 0
            assert int(bad.sum()) <= 8
    assert float(rp._bf16_of(8 / (1 + 2.718281828459045 ** -8))) == 8.0  # the layout probe's gate


# ------------------------------------------- 3. the CPU definitions pass --

def _norm_info(case, name, be):
    info = {}
    fn = rp.NORM_PROBES[name]
    L = rp.membership_rows(case.M, case.H)
    big = -(-len(rp.hot_columns(case.H)) // ((L + 1) // 2)) * L * case.H * 2 > REF_BYTES
    msgs = fn(case, be, CPU, info, sample=big) if name == "membership" else fn(case, be, CPU, info)
    return msgs, info


@pytest.mark.parametrize("case", rp.NORM_CASES, ids=[c.id for c in rp.NORM_CASES])
def test_reference_norm(case):
    be = rp.RefBackend()
    for name in rp.norm_probes_of(case):
        msgs, info = _norm_info(case, name, be)
        assert not msgs, "\n".join(msgs)
        assert info.get("either", 0.0) <= 0.01, (name, info)


@pytest.mark.parametrize("case", rp.SILU_CASES, ids=[c.id for c in rp.SILU_CASES])
def test_reference_silu(case):
    be = rp.RefBackend()
    for name, fn in rp.SILU_PROBES.items():
        info = {}
        msgs = fn(case, be, CPU, info)
        assert not msgs, "\n".join(msgs)
        assert info.get("either", 0.0) <= 0.01, (name, info)
        if name == "gates" and case.M * case.I >= rp.N_FINITE:
            assert info["gates"] == rp.N_FINITE


@pytest.mark.parametrize("case", rp.EMB_CASES, ids=[c.id for c in rp.EMB_CASES])
def test_reference_embedding(case):
    msgs = rp.probe_embedding(case, rp.RefBackend(), CPU)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", rp.ROPE_CASES, ids=[c.id for c in rp.ROPE_CASES])
def test_reference_rope(case):
    msgs = rp.probe_rope(case, rp.RefBackend(), CPU)
    assert not msgs, "\n".join(msgs)


@pytest.mark.parametrize("case", rp.REAL_CASES, ids=[c.id for c in rp.REAL_CASES])
def test_reference_rope_real_table(case):
    msgs = rp.probe_rope_real(case, rp.RefBackend(), CPU)
    assert not msgs, "\n".join(msgs)


def test_reference_empty_launches():
    be = rp.RefBackend()
    msgs = [m for add in (False, True) for m in rp.probe_norm_empty(be, CPU, add)]
    msgs += [m for il in (0, 1) for m in rp.probe_silu_empty(be, CPU, il)]
    msgs += rp.probe_embedding_empty(be, CPU)
    msgs += [m for f in (0, 1) for m in rp.probe_rope_empty(be, CPU, f)]
    assert not msgs, "\n".join(msgs)


# ---------------------------------------------------------- 4. fault table --

def _trunc(x):
    """fp32 -> bf16 by truncation."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(bf)


def _row_past(t):
    """The rows of a view out[:M] and the one behind them (the buffer's first sentinel row)."""
    return torch.as_strided(t, (t.shape[0] + 1, t.shape[1]), t.stride(), t.storage_offset())


class Faulty(rp.RefBackend):
    """The ops restated in plain torch, with one fault injected (None: no fault)."""

    def __init__(self, fault):
        super().__init__()
        self.fault = fault

    # --- norm
    def _norm(self, out, r32, w, eps, stored=None):
        f, H = self.fault, r32.shape[1]
        v = r32 if f == "norm_from_unrounded_sum" or stored is None else stored.float()
        sq = v * v
        ss = sq.sum(-1, keepdim=True)
        if f == "last_vector_out":
            ss = ss - sq[:, -8:].sum(-1, keepdim=True)
        elif f == "one_wave_dropped":
            ss = ss - sq[:, 512:1024].sum(-1, keepdim=True)
        elif f == "vector_twice":
            ss = ss + sq[:, -16:-8].sum(-1, keepdim=True) + sq[:, :8].sum(-1, keepdim=True)
        elif f == "neighbour_vector_added":
            ss = ss + sq[:, :8].sum(-1, keepdim=True).roll(-1, 0)
        n = -(-H // 512) * 512 if f == "mean_over_512" else H
        e = {"eps_omitted": 0.0, "eps_1e-6": 1e-6}.get(f, eps)
        inv = torch.rsqrt(ss / n + e)
        wf = w.float()
        if f == "single_rounding":
            y = (wf * v * inv).to(bf)
        elif f == "truncating_store":
            y = _trunc(wf * (v * inv).to(bf).float())
        else:
            y = (wf * (v * inv).to(bf).float()).to(bf)
        out.copy_(y)
        if f == "row_m_written" and out.shape[0]:
            _row_past(out)[-1] = out[-1]

    def rmsnorm(self, out, x, w, eps):
        self._norm(out, x.float(), w, eps)

    def add_rmsnorm(self, out, res, x, w, eps):
        s = x.float() + res.float()
        res.copy_(_trunc(s) if self.fault == "residual_truncated" else s.to(bf))
        self._norm(out, s, w, eps, stored=res)

    # --- SiLU-mul
    def silu_mul(self, out, x, interleaved):
        f = self.fault
        M, I = x.shape[0], x.shape[1] // 2
        if f == "interleave_in_plain_layout":
            interleaved = 1
        if interleaved and I % 16 == 0:
            v = x.view(M, I // 16, 2, 16)
            g, u = v[:, :, 0], v[:, :, 1]
            if f == "groups_shifted":
                u = u.roll(-1, 1)
            g, u = g.reshape(M, I), u.reshape(M, I)
        else:
            g, u = x[:, :I], x[:, I:]
        if f == "halves_swapped":
            g, u = u, g
        g, u = g.float(), u.float()
        s = g / (1 + torch.exp(g if f == "sigmoid_plus" else -g))
        y = (s * u).to(bf) if f == "no_intermediate_rounding" else (s.to(bf).float() * u).to(bf)
        if f == "beyond_cap_unwritten":
            n = min(M * I, rp.SILU_CAP * 8)
            out.view(-1)[:n] = y.reshape(-1)[:n]
        else:
            out.copy_(y)

    # --- embedding
    def embedding(self, out, table, ids, vocab_start):
        f = self.fault
        local = ids - vocab_start
        ok = (local >= 0) & ((local <= table.shape[0]) if f == "inclusive_vocab_end" else (local < table.shape[0]))
        rows = table[(local + (f == "row_off_by_one")).clamp(0, table.shape[0] - 1)].clone()
        if f == "columns_past_2048_not_copied":
            rows[:, 2048:] = out[:, 2048:]
        rows[~ok] = out[~ok] if f == "outside_rows_unwritten" else 0
        out.copy_(rows)

    # --- RoPE and the cache writers
    def rope(self, q, kc, vc, qkv, pos, cs, slots, ks=None, vs=None):
        f = self.fault
        T, Hq, D = q.shape
        Hkv, half = kc.shape[1], D // 2
        x = qkv.float().reshape(T, Hq + 2 * Hkv, D)
        p = pos.long()
        if f == "position_off_by_one":
            p = (p + 1) % cs.shape[0]
        elif f == "previous_tokens_position":
            p = p.roll(1)
        c = cs[p]
        cos, sin = c[:, None, :half], c[:, None, half:]
        if f == "pair_read_at_i_plus_1":
            cos, sin = cos.roll(-1, -1), sin.roll(-1, -1)
        if f == "sin_sign_flipped":
            sin = -sin
        n_rot = Hq + (2 * Hkv if f == "v_rotated" else Hkv)
        x1, x2 = x[:, :n_rot, :half], x[:, :n_rot, half:]
        a, b = x1 * cos - x2 * sin, x2 * cos + x1 * sin
        rows32 = torch.cat([torch.cat([b, a] if f == "rope_halves_swapped" else [a, b], -1), x[:, n_rot:]], 1)
        rows = rows32.to(bf)
        keep = slots >= 0 if f == "padding_q_skipped" else torch.ones(T, dtype=torch.bool)
        q[keep] = rows[keep, :Hq]
        for t in range(T):
            s = int(slots[t])
            if s < 0:
                if f != "padding_written":
                    continue
                s = 0
            b_, o = (s // 17, s % 17 % 16) if f == "slot_split_by_17" else divmod(s, 16)
            for h in range(Hkv):
                hd = h % 8 if f == "kv_head_modulo_8" else h
                for cache, sc, i in ((kc, ks, Hq + h), (vc, vs, Hq + Hkv + h)):
                    if ks is None:
                        cache[b_, hd, o] = rows[t, i]
                        continue
                    amax = float((rows32 if f == "amax_before_rounding" else rows.float())[t, i].abs().amax())
                    m, e = torch.frexp(torch.tensor(amax, dtype=torch.float64))
                    step = float(m) < 0.875 if f == "step_at_less_than" else float(m) <= 0.875
                    e = max(-126, min(127, -126 if amax == 0 else int(e) - (9 if step else 8)))
                    y = (rows[t, i].float() * 2.0 ** -e).clamp(-448, 448).to(rp.FP8)
                    cache.view(torch.uint8)[b_, hd, o] = y.view(torch.uint8)
                    if not (f == "scale_for_k_only" and cache is vc):
                        sc[b_, hd, o] = e + 127

    def rope_fp8(self, q, kc, vc, ks, vs, qkv, pos, cs, slots):
        self.rope(q, kc, vc, qkv, pos, cs, slots, ks, vs)


NORM_FAULTS = ["last_vector_out", "one_wave_dropped", "vector_twice", "neighbour_vector_added", "mean_over_512",
               "eps_omitted", "eps_1e-6", "single_rounding", "truncating_store", "residual_truncated",
               "norm_from_unrounded_sum", "row_m_written"]
SILU_FAULTS = ["halves_swapped", "groups_shifted", "interleave_in_plain_layout", "no_intermediate_rounding",
               "sigmoid_plus", "beyond_cap_unwritten"]
EMB_FAULTS = ["inclusive_vocab_end", "row_off_by_one", "outside_rows_unwritten", "columns_past_2048_not_copied"]
ROPE_FAULTS = ["position_off_by_one", "previous_tokens_position", "pair_read_at_i_plus_1", "sin_sign_flipped",
               "rope_halves_swapped", "v_rotated", "slot_split_by_17", "kv_head_modulo_8", "padding_written",
               "padding_q_skipped"]
FP8_FAULTS = ["step_at_less_than", "amax_before_rounding", "scale_for_k_only"]
ALL_FAULTS = NORM_FAULTS + SILU_FAULTS + EMB_FAULTS + ROPE_FAULTS + FP8_FAULTS


def _pick(cases, *ids):
    by = {c.id: c for c in cases}
    return [by[i] for i in ids]


# the cases a fault runs on: small ones of every form it can show on
FAULT_NORM_CASES = _pick(rp.NORM_CASES, "norm-M3-H4104", "add-M3-H4104", "add-M258-H1024", "norm-M257-H512")
FAULT_SILU_CASES = _pick(rp.SILU_CASES, "silu-M3-I48-plain", "silu-M3-I48-il", "silu-M37-I14336-plain")
FAULT_SILU_CAP_CASE = _pick(rp.SILU_CASES, "silu-M293-I14336-plain")[0]
FAULT_EMB_CASES = _pick(rp.EMB_CASES, "emb-H2056-v500-T77", "emb-H256-v0-T77")
FAULT_ROPE_CASES = _pick(rp.ROPE_CASES, "bf16-q32-kv8-T17", "bf16-q4-kv12-T17")
FAULT_FP8_CASES = _pick(rp.ROPE_CASES, "fp8-q32-kv8-T17", "fp8-q4-kv12-T33")


def caught_by(fault):
    """The probes (``family/probe case``) that fail on the back end with this fault."""
    be, hits = Faulty(fault), []

    def note(name, msgs):
        if msgs:
            hits.append(name)

    if fault is None or fault in NORM_FAULTS:
        for case in FAULT_NORM_CASES:
            for name in rp.norm_probes_of(case):
                note(f"norm/{name} {case.id}", _norm_info(case, name, be)[0])
    if fault is None or (fault in SILU_FAULTS and fault != "beyond_cap_unwritten"):
        for case in FAULT_SILU_CASES:
            for name, fn in rp.SILU_PROBES.items():
                note(f"silu/{name} {case.id}", fn(case, be, CPU))
    if fault == "beyond_cap_unwritten":
        note(f"silu/layout {FAULT_SILU_CAP_CASE.id}", rp.probe_silu_layout(FAULT_SILU_CAP_CASE, be, CPU))
    if fault is None or fault in EMB_FAULTS:
        for case in FAULT_EMB_CASES:
            note(f"embedding {case.id}", rp.probe_embedding(case, be, CPU))
    if fault is None or fault in ROPE_FAULTS:
        for case in FAULT_ROPE_CASES + FAULT_FP8_CASES[:1]:
            note(f"rope/selector {case.id}", rp.probe_rope(case, be, CPU))
    if fault is None or fault in FP8_FAULTS:
        for case in FAULT_FP8_CASES:
            note(f"rope/selector {case.id}", rp.probe_rope(case, be, CPU))
    return hits


def test_the_restated_ops_pass_without_a_fault():
    assert caught_by(None) == []


@pytest.mark.parametrize("fault", ALL_FAULTS)
def test_every_fault_fails_a_probe(fault):
    hits = caught_by(fault)
    print(fault, hits)
    assert hits, fault


if __name__ == "__main__":
    print("| fault | caught by (probe: cases) |")
    print("|---|---|")
    for fault in ALL_FAULTS:
        by_probe = {}
        for hit in caught_by(fault):
            probe, case = hit.split(" ")
            by_probe.setdefault(probe, []).append(case)
        cells = [p + ": " + ", ".join(c) for p, c in by_probe.items()]
        print(f"| {fault} | {'; '.join(cells) or 'MISSED'} |")
