"""The attention probes of tests/attn_probes.py, without a GPU: the fp32 reference attention
meets them on every launch geometry of tests/test_probes_attention_gpu.py, an emulated attention
with ONE fault injected (a key too many, too few, doubled, a V row from the wrong key) fails them
at 1500 keys, and they hold through the host planner's own metadata (MetaBuffers)."""
import math

import numpy as np
import pytest
import torch

import attn_probes as ap
from mlopamd.ops import reference as ref
from mlopamd.runtime.attn_meta import MetaBuffers, plan_partitions

D = ap.D


# ------------------------------------------------ 1. reference == expected --

def _reference_meets(q_lens, ctx_lens, G, window=0, flash_min_q=1 << 30):
    for kind, schedule in ap.PROBES:
        m, q, kc, vc, exp = ap.build(kind, q_lens, ctx_lens, ap.HKV, G, window, flash_min_q, schedule=schedule)
        ap.assert_probe(ref.paged_attention(q, kc, vc, m), exp, f"{kind}/{schedule} G={G} W={window}")


@pytest.mark.parametrize("G", ap.DECODE_G)
def test_reference_decode(G):
    _reference_meets(*ap.decode_launch(G), G)


@pytest.mark.parametrize("G", ap.WIN_DECODE_G)
@pytest.mark.parametrize("W", ap.WIN_DECODE_W)
def test_reference_windowed_decode(W, G):
    _reference_meets(*ap.windowed_decode_launch(W), G, W)


@pytest.mark.parametrize("G", ap.FLASH_G)
@pytest.mark.parametrize("launch", list(ap.FLASH_LAUNCHES))
def test_reference_flash(launch, G):
    _reference_meets(*ap.FLASH_LAUNCHES[launch], G, flash_min_q=ap.FLASH_MIN_Q)


@pytest.mark.parametrize("G", ap.FLASH_G)
@pytest.mark.parametrize("W", ap.WIN_FLASH_W)
def test_reference_windowed_flash(W, G):
    _reference_meets(*ap.windowed_flash_launch(), G, W, flash_min_q=ap.FLASH_MIN_Q)


# ---------------------------------------------------------- 2. fault table --

PART = 256   # partition size of the emulated split-KV faults


def row_kv(m, kc, vc):
    """The one live row's K, V [n, Hkv, D] (fp64) for the key positions first .. last page + the
    dead page, through the block table, and ``first`` (windowed: the first readable position)."""
    h = m.host
    r = int(h["rows"][0])
    ql, c = int(h["q_len"][r]), int(h["ctx_len"][r])
    first = (max(0, c - ql - m.window + 1) & ~31) if m.window > 0 else 0
    pages = torch.from_numpy(h["bt"][r, first // 16:(c + 15) // 16 + 1].astype(np.int64))
    gather = lambda cache: cache[pages].permute(0, 2, 1, 3).reshape(-1, cache.shape[1], D).double()  # noqa: E731
    return gather(kc), gather(vc), first, ql, c


FAULTS = ["causal+1", "causal-1", "window+1", "window-1", "part_first_dropped", "part_first_doubled",
          "diag_pair_dropped", "v_swap_t_t^4", "v_three_pairs_back"]


def emulate(q, K, V, first, ql, c, W, fault=None):
    """Attention of one row from a visibility mask, per-key weights and a V-row index map (all
    [ql, n] / [n] over the key positions first .. first + n - 1), in fp64, rounded once to bf16,
    with ``fault`` injected.  Returns (out [ql, Hq, D] bf16, changed): ``changed`` says whether
    the fault alters the visible set, its weights or the K-V pairing of a visible key at all."""
    n, G = K.shape[0], q.shape[1] // K.shape[1]
    keys = torch.arange(first, first + n)
    pos = torch.arange(c - ql, c)[:, None]
    lo = (pos - W + 1).clamp_min(0) if W > 0 else torch.zeros_like(pos)

    def plan(fault):
        hi_f, lo_f = pos, lo
        weight, vmap = torch.ones(n, dtype=torch.float64), torch.arange(n)
        if fault == "causal+1":
            hi_f = pos + 1
        elif fault == "causal-1":
            hi_f = pos - 1
        elif fault == "window+1" and W > 0:
            lo_f = lo - 1
        elif fault == "window-1" and W > 0:
            lo_f = lo + 1
        vis = (keys[None] <= hi_f) & (keys[None] >= lo_f)
        # partitions count from the first readable key (kv_lo), as in the kernels
        if fault == "part_first_dropped":
            weight[(keys - first) % PART == 0] = 0
        elif fault == "part_first_doubled":
            weight[(keys - first) % PART == 0] = 2
        elif fault == "diag_pair_dropped":
            vis = vis & ((keys[None] >> 5) != (pos >> 5))
        elif fault == "v_swap_t_t^4":          # the decode kernel's in-pair token permutation
            vmap = vmap ^ 4
        elif fault == "v_three_pairs_back":    # a ring slot consumed before its refill landed
            vmap = torch.where(vmap >= 96, vmap - 96, vmap)
        return vis.double() * weight[None], vmap

    w_ok, vmap_ok = plan(None)
    w, vmap = plan(fault)
    seen = w.sum(0) > 0
    changed = bool((w != w_ok).any() or (vmap != vmap_ok)[seen].any())
    Kh, Vh = K.repeat_interleave(G, dim=1), V[vmap].repeat_interleave(G, dim=1)
    s = torch.einsum("qhd,khd->hqk", q.double(), Kh) / math.sqrt(D)
    s = s.masked_fill(w[None] == 0, float("-inf"))
    mx = s.amax(-1, keepdim=True)
    p = torch.exp(s - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))) * w[None]
    # (0 x the dead slots' 64 / NaN-free by construction; a faulty V map may read a dead row)
    o = torch.einsum("hqk,khd->qhd", p, Vh) / p.sum(-1).clamp_min(1e-300).permute(1, 0)[:, :, None]
    return torch.from_numpy(ap.round_bf16(o.numpy())).to(ap.bf), changed


GEOMETRIES = [(1, 0), (300, 0), (1, 100), (300, 100)]     # (q_len, window), ending at key 1499
_table_cache = {}


def fault_table():
    """{(q_len, W): {fault: (applies, caught by the counting probe, caught by a needle probe,
    missed by the random 2e-2 check)}}; the clean run is asserted on the way."""
    if _table_cache:
        return _table_cache
    G = 4
    for ql, W in GEOMETRIES:
        runs = []
        for kind, schedule in ap.PROBES:
            m, q, kc, vc, exp = ap.build(kind, [ql], [1500], ap.HKV, G, W, schedule=schedule)
            K, V, first, _, c = row_kv(m, kc, vc)
            qs = int(m.host["q_start"][m.host["rows"][0]])
            runs.append((kind, q[qs:qs + ql], K, V, first, exp[qs:qs + ql]))
        # the random check the suite had: randn Q / K / V, the fp32-reference tolerance
        g = torch.Generator().manual_seed(0)
        n = runs[0][2].shape[0]
        rq = torch.randn(ql, ap.HKV * G, D, generator=g).to(ap.bf)
        rK, rV = (torch.randn(n, ap.HKV, D, generator=g).to(ap.bf).double() for _ in range(2))
        r_ok, _ = emulate(rq, rK, rV, first, ql, c, W)
        tab = {}
        for fault in [None] + FAULTS:
            caught = {"count": False, "needle": False}
            applies = False
            for kind, q, K, V, first, exp in runs:
                out, changed = emulate(q, K, V, first, ql, c, W, fault)
                applies |= changed
                caught[kind] |= ap.mismatch(out, exp) is not None
            r_out, _ = emulate(rq, rK, rV, first, ql, c, W, fault)
            missed = torch.allclose(r_out.float(), r_ok.float(), atol=2e-2, rtol=2e-2)
            tab[fault] = (applies, caught["count"], caught["needle"], missed)
        _table_cache[(ql, W)] = tab
    return _table_cache


@pytest.mark.parametrize("ql,W", GEOMETRIES)
def test_fault_table(ql, W):
    """Every fault that changes the visible set, its weights or the K-V pairing fails a probe at
    1500 keys; the unfaulted emulation passes both."""
    tab = fault_table()[(ql, W)]
    print(f"\nq_len {ql} W {W}: fault -> applies, counting, needle, missed by the random 2e-2 check")
    for fault, row in tab.items():
        print(f"  {fault}: {row}")
    assert tab[None][:3] == (False, False, False)
    n_applied = 0
    for fault in FAULTS:
        applies, by_count, by_needle, _ = tab[fault]
        if not applies:
            assert not by_count and not by_needle, fault   # a no-op fault must not trip a probe
            continue
        n_applied += 1
        assert by_count or by_needle, f"{fault} slipped through both probes"
    # the window faults and the partition faults each need their geometry; the rest apply everywhere
    assert n_applied >= (6 if W == 0 else 7)


def test_random_check_misses_single_keys_at_1500():
    """What the probes are for: on the q_len 1 row at 1500 keys the randn check at atol = rtol =
    2e-2 sees neither a causal limit off by one nor a partition's first key dropped or doubled."""
    tab = fault_table()[(1, 0)]
    for fault in ("causal+1", "causal-1", "part_first_dropped", "part_first_doubled"):
        applies, by_count, _, missed = tab[fault]
        assert applies and missed and by_count, (fault, tab[fault])


# -------------------------------------------------- 3. the host planner's --

def planner_case(kind, schedule, window, device="cpu", G=4, seed=0):
    """A mixed step through MetaBuffers: four decode rows and one 300-token prompt chunk ending at
    1500 keys, block tables assigned by the probe, everything else by fill_mixed /
    plan_partitions / meta."""
    d_ctx = np.asarray([1500, 33, 257, 700], np.int64)
    p_ql, p_ctx = [300], [1500]
    d_rows, p_rows = np.asarray([5, 0, 3, 6]), [2]
    ctx_all, ql_all = list(d_ctx) + p_ctx, [1] * len(d_ctx) + p_ql
    NB = ap.num_pages(ctx_all)
    mb = MetaBuffers(512, 8, max(ctx_all) // 16 + 2, G, ap.HKV, 2048, device, flash_min_q=ap.FLASH_MIN_Q,
                     window=window)
    rows = np.concatenate([d_rows, p_rows])
    nan_pages = ap.assign_pages(mb.bt_h, rows, ql_all, ctx_all, window, NB, np.random.RandomState(seed))
    T, nt, nl = mb.fill_mixed(d_rows, d_ctx, np.zeros(len(d_rows), np.int64), p_rows, p_ql, p_ctx,
                              [np.zeros(p_ql[0], np.int64)])
    mb.upload(T, nl)
    part, nparts = plan_partitions(nt, ap.HKV, mb.span(max(ctx_all)))
    meta = mb.meta(T, nt, nl, part, nparts, mb.npt)
    assert mb.npt > 0 and nt == len(d_rows) and meta.window == window
    host = dict(bt=mb.bt_h, q_start=mb.view_h("q_start"), q_len=mb.view_h("q_len"), ctx_len=mb.view_h("ctx_len"),
                rows=rows, nan_pages=nan_pages)
    return (meta,) + ap.make_data(kind, host, ap.HKV, G, window, NB, T, device, seed, schedule)


@pytest.mark.parametrize("window", [0, 100])
def test_reference_through_the_planner(window):
    for kind, schedule in ap.PROBES:
        meta, q, kc, vc, exp = planner_case(kind, schedule, window)
        assert meta.nparts > 1     # a few decode tiles: the planner splits the keys
        ap.assert_probe(ref.paged_attention(q, kc, vc, meta), exp, f"{kind}/{schedule} W={window}")
