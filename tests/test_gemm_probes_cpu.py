"""The GEMM probes of tests/gemm_probes.py, without a GPU: the case list covers every route class
of the pinned table's serving block, the reference alone meets the conditions that keep the
probes sensitive, the CPU definitions of the ops pass the probes at the small cases, and an
emulated tiled split-K GEMM with ONE fault injected fails them (profiles/gemm_probes.md holds
the table this file prints with ``python tests/test_gemm_probes_cpu.py``)."""
import subprocess

import pytest
import torch

import gemm_probes as gp
import test_gemm_plan_cpu as plan
from mlopamd import ops

bf = torch.bfloat16
N_CLASSES = 142       # of the cus256_sk block when this test was written: a planner change that adds a
#                       class shows up here as well as in the diff of the table
REF_MAX_MADDS = 1.2e8  # the cases the CPU definitions of the ops run in well under a second


# ------------------------------------------------------------ 1. coverage --

def test_every_class_has_its_two_cases():
    with open(plan.FIXTURE) as f:
        rows = [r for r in plan._rows(f.read()) if r[0] == gp.ENV and r[7]["family"] != "-"]
    classes = {gp.route_class(op, K, r) for _, op, N, K, ng, m0, m1, r in rows}
    assert classes == set(gp.CLASSES) and len(classes) == N_CLASSES
    assert len({c.id for c in gp.CASES}) == len(gp.CASES)
    by_cls = {}
    for c in gp.CASES:
        by_cls.setdefault(c.cls, []).append(c)
    for cls, info in gp.CLASSES.items():
        m0, m1 = info["m_first"], info["m_last"]
        ms = sorted(c.M for c in by_cls[cls])
        assert ms == sorted({m0, gp.second_m(m0, m1)}), (cls, ms)
        assert m0 <= ms[-1] <= m1 and (ms[-1] == m1 or (ms[-1] - m0 + 1) % 256 == 0 and m1 > 4 * m0 + 256), (cls, ms)
        # the interval is one of the table's own, of this class
        assert any((op, N, K, ng, a, b) == (cls[0], info["N"], info["K"], info["n_groups"], m0, m1) and
                   gp.route_class(op, K, r) == cls for _, op, N, K, ng, a, b, r in rows), cls
    assert max(gp.madds(c) for c in gp.CASES + gp.OP8_CASES) <= gp.MAX_MADDS


def test_the_classes_no_kernel_test_ran_are_there():
    have = set(gp.CLASSES)
    fam = lambda op, f: {c for c in have if c[0] == op and c[1] == f}  # noqa: E731
    assert fam(plan.ADD_NORM, "S") and fam(plan.ROPE, "S")             # weight-streaming at 5 to 8 rows
    assert any(c[3] > 1 and c[4] for c in have)                        # split-K with an uneven last range
    assert {(c[3], gp.CLASSES[c]["route"]["k_chunk"]) for c in have if c[0] == 0 and c[4] and c[2] == 17} >= \
        {(7, 640), (5, 832), (6, 704), (3, 1408)}
    with open(plan.FIXTURE) as f:
        tails = {r["sk_d"] for e, *_, r in plan._rows(f.read()) if e == gp.ENV and r["sk_d"]}
    assert tails and {c[7] for c in have if c[7]} == tails             # every P<d>
    for op in (plan.PLAIN, plan.SILU, plan.ROPE, plan.CHAIN_RES_SS, plan.CHAIN_RS_SILU, plan.CHAIN_RS_ROPE):
        assert fam(op, "H") and fam(op, "W"), op
    # the plant's run of 263 ones at the lowest k lies within the first K range of every split route of
    # the planted ops (ranges of 256 hold at most 256 products of +-1: whatever they sum to is a bf16 number)
    chunks = {gp.CLASSES[c]["route"]["k_chunk"] for c in have if c[3] > 1 and c[0] in (plan.PLAIN, plan.GROUPED)}
    assert all(k <= 256 or k >= 512 > gp.PLANT[1][0] for k in chunks), chunks
    # the TP-sharded QKV widths
    assert {c.N for c in gp.CASES if c.op in (plan.PLAIN, plan.ROPE)} >= {768, 1536, 2560, 3072}


def test_grouped_rows_are_uneven_with_an_empty_and_a_one_row_expert():
    for c in gp.CASES:
        if not c.n_groups:
            continue
        R = gp.rows_of(c)
        counts = gp.group_counts(R, c.n_groups, gp._gen(c.id, "cpu"))
        assert len(counts) == c.n_groups and sum(counts) == R and min(counts) >= 0
        assert counts == gp.group_counts(R, c.n_groups, gp._gen(c.id, "cpu"))  # seeded from the id
        if R >= 10:
            assert 0 in counts and 1 in counts and len(set(counts)) > 2, (c.id, counts)
        assert gp.rows_per_group(c) == -(-R // c.n_groups)


def test_op8_shapes_are_on_the_forms_their_ids_name(tmp_path):
    """The two op-8 cases are not in the table: ask the planner (the dump program) directly."""
    exe = plan._build(tmp_path, False)
    stdin = "".join(f"{c.op} {c.N} {c.K} 0\n" for c in gp.OP8_CASES)
    r = subprocess.run([exe, "256", "1", "5"], input=stdin, capture_output=True, text=True, timeout=120, check=True)
    rows = list(plan._rows("# env x\n" + r.stdout))
    for c in gp.OP8_CASES:
        hit = [r for _, op, N, K, ng, m0, m1, r in rows if (op, N, K) == (c.op, c.N, c.K) and m0 <= c.M <= m1]
        assert len(hit) == 1 and hit[0]["family"] == c.cls[1], (c.id, hit)


# ------------------------------------- 2. the conditions of a sensitive probe --

def sample_figures(case, rows=8, cols=512):
    """The reference alone on a sample of the case's product (its first rows and columns, whole
    K; the entries are i.i.d., so any rows and columns serve): the fraction of |exact| > 256,
    where a +-1 error can round away, and for the SiLU ops of |g|, |u| <= 100, where +-1 moves
    the result by more than an ulp."""
    gen = gp._gen(case.id, "cpu")
    M, n, K = min(gp.rows_of(case), rows), min(case.N, cols), case.K
    silu = case.op in gp.SILU_OPS
    if case.op in gp.RS_OPS:
        a = gp.resid((M, K), gen, 0.5).float()
        scale = gp._rinv64(a).float()
    else:
        a, scale = gp.tern((M, K), 0.5, gen).float(), 1.0
    w = gp.tern((n, K), gp.silu_density(case.op, K) if silu else gp.w_density(K), gen).float()
    y = (a @ w.t()) * scale  # integers below 2^24: exact in fp32
    over = float((y.abs() > 256).float().mean())
    return over, (float((y.abs() <= 100).float().mean()) if silu else 1.0)


def test_sensitivity_conditions_hold_for_every_case():
    for c in gp.CASES + gp.OP8_CASES:
        q = gp.silu_density(c.op, c.K) if c.op in gp.SILU_OPS else gp.w_density(c.K)
        # std of one sum: K terms, each +-1 with probability q / 2 (x in [-8, 8] at density 1 / 2: E x^2
        # = 12.75, divided out again by the row's RMS): at most 32, so 256 is 8 sigma away
        assert c.K * q / 2 <= 1024, c.id
        over, in_range = sample_figures(c)
        assert over <= 0.01, (c.id, over)
        # |g| and |u| each in range on a fraction p of the sample: both on at least 2 p - 1
        assert 2 * in_range - 1 >= 0.95, (c.id, in_range)


# ------------------------------------------- 3. the CPU definitions pass --

SMALL = [c for c in gp.CASES + gp.OP8_CASES if gp.madds(c) <= REF_MAX_MADDS]


def test_small_cases_span_every_op():
    assert {c.op for c in SMALL} == {c.op for c in gp.CASES + gp.OP8_CASES}


@pytest.mark.parametrize("case", SMALL, ids=[c.id for c in SMALL])
def test_reference_meets_the_probe(case):
    info = {}
    msgs = gp.probe(case, gp.RefBackend(), torch.device("cpu"), info)
    assert not msgs, "\n".join(msgs)
    assert info["over256"] <= 0.01 and info.get("silu_in_range", 1.0) >= 0.95, info


# ---------------------------------------------------------- 4. fault table --

FAULTS = ["last_k_dropped", "remainder_dropped", "k_tile_read_twice", "ranges_overlap_one_tile", "slab_left_out",
          "clamped_rows_stored", "last_row_reads_previous", "n_tile_shifted_16", "gate_up_group_off_by_one",
          "bf16_slab", "truncating_store"]
# K -> k_chunk: two even ranges; seven ranges with a ragged last one (the table's s7k640); seven of
# 33 K tiles with a ragged last one
GEOMETRIES = {1024: 512, 4096: 640, 14336: 2112}
EM, EN, BM, BN = 70, 512, 64, 64


def emulate(a, w, k_chunk, epi, fault=None):
    """A tiled split-K GEMM a [M, K] x w [N, K]^T as the kernels organise it: M tiles of BM rows
    (rows past M clamped to the last one, never stored), N tiles of BN columns, K ranges of
    k_chunk into fp32 slabs, a reduce, the epilogue and one bf16 store into a buffer with
    sentinel rows; ``fault`` injects one error.  Returns (out [M + PAD, N or N / 2], applies):
    ``applies`` is False where the fault is a no-op in this geometry."""
    M, K = a.shape
    N = w.shape[0]
    af, wf = a.float(), w.float()
    ranges = [(k0, min(k0 + k_chunk, K)) for k0 in range(0, K, k_chunk)]
    applies = True
    if fault == "last_k_dropped":
        ranges[-1] = (ranges[-1][0], K - 1)
    elif fault == "remainder_dropped":
        applies = K % k_chunk != 0
        if applies:
            ranges.pop()
    elif fault == "ranges_overlap_one_tile":
        ranges[1] = (ranges[1][0] - 64, ranges[1][1])
    Mp = -(-M // BM) * BM
    rows = torch.arange(Mp).clamp(max=M - 1)
    if fault == "last_row_reads_previous":
        rows[M - 1] = M - 2
    slabs = []
    for i, (k0, k1) in enumerate(ranges):
        ak, wk = af[rows, k0:k1], wf[:, k0:k1]
        if fault == "k_tile_read_twice" and i == 0:  # the second 64-wide tile comes from the first one's address
            ak, wk = ak.clone(), wk.clone()
            ak[:, 64:128], wk[:, 64:128] = ak[:, :64], wk[:, :64]
        s = ak @ wk.t()
        if fault == "bf16_slab" and i == 0:
            s = s.to(bf).float()
        slabs.append(s)
    if fault == "slab_left_out":
        slabs.pop(1)
    acc = torch.zeros(Mp, N)
    for s in slabs:
        acc += s
    if fault == "n_tile_shifted_16":
        acc[:, BN:2 * BN] = acc[:, BN:2 * BN].roll(16, 1)
    if epi:
        v = acc.view(Mp, N // 32, 2, 16)
        gate, up = v[:, :, 0], v[:, :, 1]
        if fault == "gate_up_group_off_by_one":
            up = up.roll(-1, 1)
        gate, up = gate.reshape(Mp, N // 2), up.reshape(Mp, N // 2)
        acc = torch.nn.functional.silu(gate.to(bf).float()).to(bf).float() * up.to(bf).float()
    elif fault == "gate_up_group_off_by_one":
        applies = False
    if fault == "truncating_store":
        val = (acc.contiguous().view(torch.int32) & -65536).view(torch.float32).to(bf)
    else:
        val = acc.to(bf)
    out = torch.full((M + gp.PAD, val.shape[1]), gp.SENTINEL, dtype=bf)
    n = min(Mp, M + gp.PAD) if fault == "clamped_rows_stored" else M
    out[:n] = val[:n]
    return out, applies


def probe_inputs(K, epi, seed=0):
    gen = torch.Generator().manual_seed(seed)
    a = gp.tern((EM, K), 0.5, gen)
    if epi:
        p = gp.silu_density(plan.SILU, K)
        g, u = gp.tern((EN // 2, K), p, gen), gp.tern((EN // 2, K), p, gen)
        return a, ops.interleave_gate_up(g, u), (g, u)
    w = gp.tern((EN, K), gp.w_density(K), gen)
    gp.plant(a[EM - 1], w)
    return a, w, None


def probe_verdict(a, w, gu, out, k_chunk):
    if gu is None:
        return gp.check_plain("emulated", out, EM, a.double() @ w.double().t(), a, w, k_chunk)
    yg, yu = a.double() @ gu[0].double().t(), a.double() @ gu[1].double().t()
    return gp.check_ulp("emulated", out, EM, gp.silu_mul64(yg, yu))


def randn_outside(K, k_chunk, epi, fault):
    """Elements of the emulated faulty GEMM that test_gemm's check (randn x, 0.05 randn w, atol =
    3e-3 max|y| + 1e-2, rtol = 2e-2 against the fp32 product) would flag; (count, of)."""
    torch.manual_seed(0)
    x = torch.randn(EM, K).to(bf)
    if epi:
        g, u = (0.05 * torch.randn(EN // 2, K)).to(bf), (0.05 * torch.randn(EN // 2, K)).to(bf)
        w = ops.interleave_gate_up(g, u)
        exp = ops.reference.silu_mul((x.float() @ torch.cat([g, u]).float().t()).to(bf)).float()
    else:
        w = (0.05 * torch.randn(EN, K)).to(bf)
        exp = x.float() @ w.float().t()
    out = emulate(x, w, k_chunk, epi, fault)[0][:EM].float()
    atol = 3e-2 * exp.abs().max().item() / 10 + 1e-2
    return int(((out - exp).abs() > atol + 2e-2 * exp.abs()).sum()), exp.numel()


def fault_row(fault, K):
    """(verdict, messages, randn count): verdict "caught" / "MISSED" / "no-op"."""
    epi = int(fault == "gate_up_group_off_by_one")
    k_chunk = GEOMETRIES[K]
    a, w, gu = probe_inputs(K, epi)
    out, applies = emulate(a, w, k_chunk, epi, fault)
    if not applies:
        return "no-op", [], None
    msgs = probe_verdict(a, w, gu, out, k_chunk)
    return ("caught" if msgs else "MISSED"), msgs, randn_outside(K, k_chunk, epi, fault)


@pytest.mark.parametrize("K", list(GEOMETRIES))
def test_clean_emulator_passes(K):
    for epi in (0, 1):
        a, w, gu = probe_inputs(K, epi)
        out, _ = emulate(a, w, GEOMETRIES[K], epi)
        assert not probe_verdict(a, w, gu, out, GEOMETRIES[K])
        assert randn_outside(K, GEOMETRIES[K], epi, None)[0] == 0


@pytest.mark.parametrize("K", list(GEOMETRIES))
@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_fails_the_exact_probe(fault, K):
    verdict, msgs, randn = fault_row(fault, K)
    if verdict == "no-op":
        assert (fault, K) in NO_OPS
        return
    assert (fault, K) not in NO_OPS
    print(fault, K, msgs, randn)
    assert verdict == "caught", (fault, K, randn)


NO_OPS = {("remainder_dropped", 1024)}  # K = 1024 is two even ranges: there is no remainder


def test_a_dropped_product_is_named():
    """The failure message points at the k of a single dropped product, and at its K range."""
    _, msgs, _ = fault_row("last_k_dropped", 4096)
    assert "dropped at k = [4095]" in msgs[0] and "K range [6] of 640" in msgs[0], msgs
    # a whole 64-wide tile: the last one of the second range
    a, w, _ = probe_inputs(4096, 0)
    y = a.double() @ w.double().t()
    out = torch.full((EM + gp.PAD, EN), gp.SENTINEL, dtype=bf)
    out[:EM] = (y - a[:, 1216:1280].double() @ w[:, 1216:1280].double().t()).float().to(bf)
    msgs = gp.check_plain("tile", out, EM, y, a, w, 640)
    assert "one 64-wide K tile dropped at k = [1216], K range [1] of 640" in msgs[0], msgs


if __name__ == "__main__":
    print("| fault | " + " | ".join(f"K = {K}, ranges of {c}" for K, c in GEOMETRIES.items()) + " |")
    print("|---|" + "---|" * len(GEOMETRIES))
    for fault in FAULTS:
        cells = []
        for K in GEOMETRIES:
            verdict, msgs, randn = fault_row(fault, K)
            cells.append(verdict if randn is None else f"{verdict}; randn {randn[0]} of {randn[1]}")
        print(f"| {fault} | " + " | ".join(cells) + " |")
