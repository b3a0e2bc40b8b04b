"""The MoE probes of tests/moe_probes.py, without a GPU: the CPU definitions of the ops pass
them, the reference alone meets the conditions that keep them sensitive (tie shares, exact
integer ranges, the 2 % cap of the prologue form, three slab cases), and an emulated MoE block in
plain torch with ONE fault injected fails them (profiles/moe_probes.md holds the tables this
file prints with ``python tests/test_moe_probes_cpu.py``)."""
import os
import subprocess

import pytest
import torch

import gemm_probes as gp
import moe_probes as mp
import test_gemm_plan_cpu as plan
from mlopamd import ops

bf = torch.bfloat16
CPU = torch.device("cpu")
REF_MAX_MADDS = 1.2e8  # as test_gemm_probes_cpu: the GEMM-bearing cases the CPU ops run in well under a second
DISPATCH = [("small", s) for s in mp.SMALL] + [("mid", s) for s in mp.MID]
SMALL_GROUPED = [c for c in mp.GROUPED_CASES if gp.madds(c) <= REF_MAX_MADDS]
SMALL_DOWN = [c for c in mp.DOWN_CASES if gp.madds(c) <= REF_MAX_MADDS]


def _id(v):
    return v.id if hasattr(v, "id") else "-".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------- 1. the CPU definitions pass --

@pytest.mark.parametrize("pro", [False, True], ids=["x", "pro"])
@pytest.mark.parametrize("kind,shape", DISPATCH, ids=[f"{k}-{_id(s)}" for k, s in DISPATCH])
def test_reference_meets_the_dispatch_probe(kind, shape, pro):
    for rng in mp.RANGES:
        info = {}
        msgs = mp.probe_dispatch(kind, shape, rng, mp.RefMoe(), CPU, info, pro)
        assert not msgs, "\n".join(msgs)
        assert info.get("near_tie_tokens", 0.0) <= mp.NEAR_TIE_CAP, (kind, shape, rng, info)


@pytest.mark.parametrize("shape", mp.ROUTE, ids=_id)
def test_reference_meets_the_route_probe(shape):
    for rng in mp.RANGES:
        msgs = mp.probe_route_permute(shape, rng, mp.RefMoe(), CPU)
        assert not msgs, "\n".join(msgs)


def test_reference_meets_the_rank_permute_probe():
    assert not mp.probe_permute_ranks(mp.RefMoe(), CPU)


@pytest.mark.parametrize("partial", [False, True], ids=["full", "part"])
@pytest.mark.parametrize("case", SMALL_GROUPED, ids=_id)
def test_reference_meets_the_a_rows_probe(case, partial):
    info = {}
    msgs = mp.probe_a_rows(case, mp.RefMoe(), CPU, info, partial)
    assert not msgs, "\n".join(msgs)
    assert info["over256"] <= 0.01 and info.get("silu_in_range", 1.0) >= 0.95, info


def test_reference_meets_the_tail_probes():
    be = mp.RefMoe()
    for shape in mp.COMBINE:
        assert not mp.probe_combine(shape, be, CPU), shape
    for shape in mp.COMBINE_NORM + [mp.COMBINE_NORM_REFUSED]:
        assert not mp.probe_combine_norm(shape, be, CPU), shape


@pytest.mark.parametrize("partial", [False, True], ids=["full", "part"])
@pytest.mark.parametrize("case", SMALL_DOWN, ids=_id)
def test_reference_meets_the_down_probe(case, partial):
    info = {}
    msgs = mp.probe_down(case, mp.RefMoe(), CPU, info, partial)
    assert not msgs, "\n".join(msgs)
    assert info["over256"] <= 0.01, info


def test_reference_route_breaks_ties_towards_the_lower_index():
    """ops.reference.moe_route has the kernels' tie rule, and its weights are torch.topk's."""
    l = torch.tensor([[1.0, 3.0, 3.0, -2.0, 3.0, 1.0]]).to(bf)
    w, i = ops.reference.moe_route(l, 2)
    assert i.tolist() == [[1, 2]] and i.dtype == torch.int32
    w, i = ops.reference.moe_route(l, 4)
    assert i.tolist() == [[1, 2, 4, 0]]
    g = torch.Generator().manual_seed(0)
    l = torch.randn(64, 8, generator=g).to(bf)
    w, i = ops.reference.moe_route(l, 2)
    tw, ti = torch.topk(torch.softmax(l.float(), -1), 2, -1)
    assert (w - tw / tw.sum(-1, keepdim=True)).abs().max() <= 1e-6
    assert torch.equal(torch.softmax(l.float(), -1).gather(1, i.long()), tw)


# ------------------------------------- 2. the conditions of a sensitive probe --

def route_figures(kind, shape):
    """The reference alone on the exact logits of a case (its full-range inputs)."""
    T, E, k, H = shape
    x, wr, _ = mp.router_inputs(mp.dispatch_id(kind, T, E, k, H), T, E, k, H, CPU)
    l = x.double() @ wr.double().t()
    info = {"bf16": torch.equal(l.to(bf).double(), l), "fp32": torch.equal(x.float() @ wr.float().t(), l.float())}
    mp.logit_figures(l, k, info)
    _, ew = mp.expected_route(l, k)
    w32 = ops.reference.moe_route(l.to(bf), k)[0]
    info["fp32_rel"] = float(((w32.double() - ew).abs() / ew).max())
    return info


ROUTED = DISPATCH + [("route", s) for s in mp.ROUTE]


@pytest.mark.parametrize("kind,shape", ROUTED, ids=[f"{k}-{_id(s)}" for k, s in ROUTED])
def test_logits_are_exact_and_tied(kind, shape):
    T, E, k, H = shape
    f = route_figures(kind, shape)
    print(kind, shape, f)
    assert f["bf16"] and f["fp32"], f                  # integers over 4: bf16 numbers, exact in fp32
    assert f["logit_max"] <= mp.LOGIT_MAX and f["spread"] <= mp.SPREAD_MAX, f
    if k < E:
        assert f["any_tie"], f                          # the tie rule decides at least one token
        assert T < 100 or f["ties"] >= 0.05, f
    assert f["fp32_rel"] <= 2.0 ** -21.7, f            # plain fp32 torch against fp64: far inside 2^-18


def test_empty_range_inputs_keep_their_expert_unchosen():
    for kind, shape in ROUTED:
        T, E, k, H = shape
        x, wr, dead = mp.router_inputs(mp.dispatch_id(kind, T, E, k, H), T, E, k, H, CPU, empty=True)
        l = x.double() @ wr.double().t()
        assert torch.equal(l.to(bf).double(), l) and float(l.abs().max()) <= mp.LOGIT_MAX, (kind, shape)
        assert not bool((mp.expected_route(l, k)[0] == dead).any()), (kind, shape, dead)
        assert not bool((wr[0] != wr[E - 1]).any())     # the plant leaves the tied pair tied


def test_tail_inputs_are_exact_in_fp32():
    """w y is an eighth of an integer, |sum| <= 8 k <= 64: 9 bits before the point and 3 behind it,
    exact in fp32 in any order; the weights of a token are all different."""
    for T, k, H in mp.COMBINE + mp.COMBINE_NORM:
        tl = mp.tail_layout(T, k, 4, True, gp._gen("x", "cpu"), CPU)
        w = tl.topw
        assert bool(((w * 8) == (w * 8).round()).all()) and float(w.min()) >= 0.125 and float(w.max()) <= 1.0
        assert all(len(set(row)) == k for row in w.tolist())
        assert tl.n == int((tl.inv[:T * k] >= 0).sum()) and sum(tl.counts) == tl.n
        if T >= 2:
            assert bool((tl.inv[:T * k].view(T, k)[tl.dead] == -1).all())
        assert sorted(tl.inv[:T * k][tl.inv[:T * k] >= 0].tolist()) == list(range(tl.n))


def test_three_down_cases_sum_slabs():
    """From the pinned table: which down cases leave y unformed (the tail's SLABS template)."""
    slab = [c for c in mp.DOWN_CASES if mp.is_slab(c)]
    assert len(slab) + sum(mp.is_slab(c) for c in mp.DOWN_PARTIAL) >= 3
    assert {c.M for c in slab} == {129, 220} and all(c.K >= 2048 for c in slab)
    assert [mp.is_slab(c) for c in mp.DOWN_PARTIAL] == [True, False]
    fams = {c.cls[1] for c in mp.DOWN_CASES if not mp.is_slab(c)}
    assert fams == {"T", "P", "V"}, fams               # V: the table's GEMV rows, on the tile kernel when indirect
    # every op-16 and op-17 class of the table has its two row counts here
    assert {c.cls for c in mp.GROUPED_CASES} == {c for c in gp.CLASSES if c[0] in (gp.GROUPED, gp.GROUPED_SILU)}


def indirect_routes(tmp):
    """{case id: (family, tile, splits, k_chunk)} of the grouped cases asked as launch_grouped_gemm asks
    them with a_rows or deferred slabs (GemmCall::indirect), under the table's serving environment."""
    if not os.path.exists(plan.CXX):
        pytest.skip("ROCm clang++ not available")
    exe = os.path.join(str(tmp), "gemm_plan_indirect")
    srcs = [os.path.join(plan.ROOT, "tests", "native", "gemm_plan_indirect.cc"), os.path.join(plan.CSRC, "gemm_plan.cc")]
    subprocess.run([plan.CXX, "-std=c++17", "-O1", f"-I{plan.CSRC}", *srcs, "-o", exe], check=True)
    _, cus, sk, big = next(e for e in plan.ENVS if e[0] == gp.ENV)
    stdin = "".join(f"{c.op} {c.N} {c.K} {c.n_groups} {gp.rows_of(c)} {gp.rows_per_group(c)}\n" for c in mp.GROUPED_CASES)
    r = subprocess.run([exe, str(cus), str(sk), str(big)], input=stdin, capture_output=True, text=True, timeout=120, check=True)
    out = {}
    for c, line in zip(mp.GROUPED_CASES, r.stdout.splitlines(), strict=True):
        fam, tile, splits, kc = line.split()
        out[c.id] = (fam, int(tile), int(splits), int(kc))
    return out


def test_indirect_calls_take_the_tables_kernels_and_never_the_gemv(tmp_path):
    """gemm_route cannot be asked about an indirect call from Python; the planner itself can.  The
    classes of the table keep their kernel; its GEMV rows (1 to 4 of the table, 2 to 8 routed rows)
    go to a tile kernel, unsplit - so the GPU probes' ``y formed`` / ``slabs`` expectation, taken
    from the table, is the planner's answer for the calls they make."""
    routes = indirect_routes(tmp_path)
    print({c.id: routes[c.id] for c in mp.GROUPED_CASES})
    for c in mp.GROUPED_CASES:
        fam, tile, splits, kc = routes[c.id]
        _, tfam, ttile, tsplits = c.cls[:4]
        if tfam == "V":
            assert fam == "T" and splits == 1, (c.id, routes[c.id])
        else:
            assert (fam, tile if fam == "T" else -1, splits) == (tfam, ttile, tsplits), (c.id, routes[c.id])
    for c in mp.DOWN_CASES:
        assert (routes[c.id][2] > 1) == mp.is_slab(c), c.id


def test_pair_counts_put_a_token_under_two_experts():
    for c in mp.GROUPED_CASES:
        for partial in (False, True):
            T = c.M
            R = 2 * T
            n = R - R // 3 if partial else R
            counts = mp.pair_counts(n, c.n_groups, T, gp._gen(c.id, "cpu"))
            assert sum(counts) == n and max(counts) <= T, (c.id, counts)


# ---------------------------------------------------------- 3. fault table --

FAULTS = ["ties_higher", "no_renorm", "weights_swapped", "inv_neighbour", "local_dropped", "nonlocal_kept",
          "offsets_off_by_one", "arow_next_token", "slab_left_out", "slab_stride_valid_rows", "residual_not_added",
          "row_behind_written"]


class EmuMoe(mp.RefMoe):
    """An MoE block in plain torch (the CPU ops, and a down GEMM that goes through split-K slabs
    from I = 2048 on, as route_grouped splits) carrying at most one fault."""
    forms_y = True

    def __init__(self, fault=None):
        super().__init__()
        self.fault, self.applied = fault, False

    def hit(self, name):
        if self.fault == name:
            self.applied = True
        return self.fault == name

    def route(self, topw, topi, logits):
        k, E = topi.shape[1], logits.shape[1]
        p = torch.softmax(logits.float(), -1)
        if self.hit("ties_higher"):
            idx = E - 1 - torch.sort(p.flip(-1), dim=-1, descending=True, stable=True).indices[:, :k]
        else:
            idx = torch.sort(p, dim=-1, descending=True, stable=True).indices[:, :k]
        w = p.gather(1, idx)
        topw.copy_(w if self.hit("no_renorm") else w / w.sum(-1, keepdim=True))
        topi.copy_(idx)

    def _layout_faults(self, offsets, inv, back, xp, topi, e0, nl, arow):
        T, k = topi.shape
        flat = topi.reshape(-1).long() - e0
        local = (flat >= 0) & (flat < nl)
        n = int(offsets[nl])
        ls, nls = local.nonzero().flatten(), (~local).nonzero().flatten()
        f = self.fault
        if f == "inv_neighbour" and n >= 2:
            inv[ls[0]] += 1 if int(inv[ls[0]]) + 1 < n else -1
        elif f == "local_dropped" and n >= 1:
            inv[ls[0]] = -1
        elif f == "nonlocal_kept" and len(nls):
            inv[nls[0]] = n
        elif f == "offsets_off_by_one":
            offsets[(nl + 1) // 2] += 1
        elif f == "arow_next_token" and arow and n >= 1 and T > 1:
            back[0] = (back[0] + 1) % T
        elif f == "row_behind_written" and n < back.numel():
            back[n] = 0
            if xp is not None:
                xp[n] = 0
        else:
            return
        self.applied = True

    def permute(self, xp, offsets, src, inv, x, topi, e0, nl):
        super().permute(xp, offsets, src, inv, x, topi, e0, nl)
        self._layout_faults(offsets, inv, src, xp, topi, e0, nl, False)

    def dispatch_mid(self, topw, topi, offsets, arow, inv, x, wr, e0, nl, pro=None):
        super().dispatch_mid(topw, topi, offsets, arow, inv, x, wr, e0, nl, pro)
        self._layout_faults(offsets, inv, arow, None, topi, e0, nl, True)
        return True

    def grouped_rows(self, out, a, w, offsets, rpg, epi, a_rows):
        if a.shape[0] > 1 and self.hit("arow_next_token"):
            a_rows = a_rows.clone()
            a_rows[0] = (a_rows[0] + 1) % a.shape[0]
        super().grouped_rows(out, a, w, offsets, rpg, epi, a_rows)
        n = int(offsets[-1])
        if n < out.shape[0] and self.hit("row_behind_written"):
            out[n] = 0

    def _tail_faults(self, inv, topw, res):
        T, k = topw.shape
        iv = inv.view(T, k)
        if k >= 2 and self.fault == "weights_swapped":
            both = ((iv[:, 0] >= 0) & (iv[:, 1] >= 0)).nonzero().flatten()
            if len(both):
                topw = topw.clone()
                t = int(both[0])
                topw[t, 0], topw[t, 1] = topw[t, 1].clone(), topw[t, 0].clone()
                self.applied = True
        if res is not None and self.hit("residual_not_added"):
            res.zero_()
        return topw

    def combine(self, out, y, inv, topw):
        super().combine(out, y, inv, self._tail_faults(inv, topw, None))

    def combine_norm(self, out, res, y, inv, topw, nw):
        if y.shape[1] % 512 or y.shape[1] > 8192:
            return False
        return super().combine_norm(out, res, y, inv, self._tail_faults(inv, topw, res), nw)

    def down(self, out, res, y, a, w2, offsets, rpg, inv, topw, nw):
        R, I = a.shape
        G, H, _ = w2.shape
        off = offsets.tolist()
        n = off[-1]
        splits = 2 if I >= 2048 else 1
        kc = I // splits
        ws = torch.full((splits * R, H), gp.NAN)  # the slab buffer ws[s][R][H]: only valid rows are written
        for sp in range(splits):
            ks = slice(sp * kc, (sp + 1) * kc)
            for e in range(G):
                if off[e + 1] > off[e]:
                    ws[sp * R + off[e]:sp * R + off[e + 1]] = a[off[e]:off[e + 1], ks].float() @ w2[e][:, ks].float().t()
        stride = n if splits > 1 and self.hit("slab_stride_valid_rows") else R
        first = 1 if splits > 1 and self.hit("slab_left_out") else 0
        acc = torch.zeros(n, H)
        for sp in range(first, splits):
            acc += ws[sp * stride + torch.arange(n)]
        yb = torch.zeros(R, H, dtype=bf)
        yb[:n] = acc.to(bf)
        if splits == 1:
            y[:n] = yb[:n]
        if n < R and self.hit("row_behind_written"):
            y[n] = 0
        topw = self._tail_faults(inv, topw, res)
        out.copy_(self.ops.add_rmsnorm(self.ops.moe_combine(yb, inv, topw), res, nw, gp.EPS))
        return True


def _case(op, N, K, M):
    return gp.Case(f"emu-op{op}-N{N}-K{K}-M{M}", op, N, K, 4, M, (op, "T"))


EMU_SMALL, EMU_MID, EMU_ROUTE = (16, 64, 8, 2048), (17, 8, 2, 1024), (129, 8, 2, 1024)
EMU_CASES = {
    "small [full]": lambda be: mp.probe_dispatch("small", EMU_SMALL, "full", be, CPU),
    "small [half]": lambda be: mp.probe_dispatch("small", EMU_SMALL, "half", be, CPU),
    "small [none]": lambda be: mp.probe_dispatch("small", EMU_SMALL, "none", be, CPU),
    "small pro [half]": lambda be: mp.probe_dispatch("small", EMU_SMALL, "half", be, CPU, None, True),
    "mid [full]": lambda be: mp.probe_dispatch("mid", EMU_MID, "full", be, CPU),
    "mid [half]": lambda be: mp.probe_dispatch("mid", EMU_MID, "half", be, CPU),
    "mid pro [half]": lambda be: mp.probe_dispatch("mid", EMU_MID, "half", be, CPU, None, True),
    "route + permute [half]": lambda be: mp.probe_route_permute(EMU_ROUTE, "half", be, CPU),
    "permute by rank": lambda be: mp.probe_permute_ranks(be, CPU),
    "a_rows op 16": lambda be: mp.probe_a_rows(_case(gp.GROUPED, 256, 512, 20), be, CPU),
    "a_rows op 16, partial": lambda be: mp.probe_a_rows(_case(gp.GROUPED, 256, 512, 20), be, CPU, None, True),
    "a_rows op 17, partial": lambda be: mp.probe_a_rows(_case(gp.GROUPED_SILU, 256, 512, 20), be, CPU, None, True),
    "combine": lambda be: mp.probe_combine((9, 2, 2056), be, CPU),
    "combine_norm": lambda be: mp.probe_combine_norm((17, 2, 4096), be, CPU),
    "down, y formed": lambda be: mp.probe_down(_case(gp.GROUPED, 512, 512, 20), be, CPU, None, False, False),
    "down, y formed, partial": lambda be: mp.probe_down(_case(gp.GROUPED, 512, 512, 20), be, CPU, None, True, False),
    "down, slabs": lambda be: mp.probe_down(_case(gp.GROUPED, 512, 2048, 20), be, CPU, None, False, True),
    "down, slabs, partial": lambda be: mp.probe_down(_case(gp.GROUPED, 512, 2048, 20), be, CPU, None, True, True),
}


def fault_row(fault):
    """{case: "caught" / "MISSED" / "no-op"} ("no-op": the fault changes nothing in that case)."""
    row = {}
    for name, run in EMU_CASES.items():
        be = EmuMoe(fault)
        msgs = run(be)
        row[name] = "no-op" if not be.applied else "caught" if msgs else "MISSED"
    return row


def test_clean_emulator_passes():
    for name, run in EMU_CASES.items():
        msgs = run(EmuMoe())
        assert not msgs, (name, msgs)


@pytest.mark.parametrize("fault", FAULTS)
def test_every_fault_fails_a_probe(fault):
    row = fault_row(fault)
    print(fault, row)
    assert "caught" in row.values(), (fault, row)
    assert "MISSED" not in row.values(), (fault, row)  # wherever the fault changes something, a probe says so


def test_failure_messages_name_the_place():
    msgs = EMU_CASES["small [half]"](EmuMoe("ties_higher"))
    assert any("topi" in m and "token" in m and "expected expert" in m for m in msgs), msgs
    msgs = EMU_CASES["mid [half]"](EmuMoe("arow_next_token"))
    assert any("arow: row 0" in m for m in msgs), msgs
    msgs = EMU_CASES["mid [half]"](EmuMoe("offsets_off_by_one"))
    assert any("offsets: entry" in m and "local expert" in m for m in msgs), msgs
    msgs = EMU_CASES["down, slabs, partial"](EmuMoe("slab_left_out"))
    assert any("residual" in m and "row" in m for m in msgs), msgs


def find_salts():
    """For the cases whose conditions salt 0 misses: the first salt that meets them."""
    found = {}
    for kind, shape in ROUTED:
        T, E, k, H = shape
        for pro in ((False, True) if kind != "route" else (False,)):
            cid = mp.dispatch_id(kind, T, E, k, H, pro)
            for salt in range(200):
                mp.SALT[cid] = salt
                try:
                    if pro:
                        test_reference_meets_the_dispatch_probe(kind, shape, True)
                    else:
                        test_logits_are_exact_and_tied(kind, shape)
                        x, wr, dead = mp.router_inputs(cid, T, E, k, H, CPU, empty=True)
                        assert float((x.double() @ wr.double().t()).abs().max()) <= mp.LOGIT_MAX
                    break
                except AssertionError:
                    continue
            if salt:
                found[cid] = salt
    return found


if __name__ == "__main__":
    import sys

    if sys.argv[1:] == ["salts"]:
        print(find_salts())
        sys.exit(0)
    print("| case | max abs l | spread | boundary ties | fp32 torch topw error |")
    print("|---|---|---|---|---|")
    for kind, shape in ROUTED:
        f = route_figures(kind, shape)
        print(f"| {kind} {shape} | {f['logit_max']} | {f['spread']} | {f['ties']:.3f} | 2^{torch.log2(torch.tensor(f['fp32_rel'])):.1f} |")
    print()
    print("| fault | caught in | no-op in |")
    print("|---|---|---|")
    for fault in FAULTS:
        row = fault_row(fault)
        assert "MISSED" not in row.values()
        print(f"| {fault} | " + ", ".join(n for n, v in row.items() if v == "caught") + " | " +
              (", ".join(n for n, v in row.items() if v == "no-op") or "-") + " |")
