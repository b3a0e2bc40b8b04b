"""Guided decoding kernels on the GPU (ops/csrc/guided.hip): ``grammar_mask`` bit for bit against
``mask_reference``, ``grammar_advance`` exactly against ``advance_reference``, and
``Sampler.sample_ext`` with guided rows against ``sample_reference`` on the masked rows."""
import numpy as np
import pytest
import torch

from mlopamd import ops
from mlopamd.runtime.guided import advance_reference, mask_reference
from mlopamd.runtime.sampler import Sampler, SamplerExt, SamplingParams, sample_reference

pytestmark = pytest.mark.gpu

CASES = [(1, 128256, 3), (4, 128256, 600), (5, 1003, 7), (64, 32000, 40)]
_ARENAS = {}


def arena_of(V, S):
    """Host arena int16 [S + 3, ldv]: grammar A at base 0 (state 0: everything allowed, state 1:
    only v = 0, state 2: only v = V - 1, the rest ~30 % allowed) and grammar B at base S (3
    states, ~50 % allowed, the last one in the last arena row).  Entries >= 0 are valid states
    of their grammar; the padding columns hold -1."""
    if (V, S) not in _ARENAS:
        rng = np.random.default_rng(V + S)
        ldv = (V + 7) // 8 * 8
        a = np.full((S + 3, ldv), -1, np.int16)
        a[0, :V] = rng.integers(0, S, V)
        a[1, 0] = S - 1
        a[2, V - 1] = 0
        a[3:S, :V] = np.maximum(rng.integers(-2 * S, S, (S - 3, V), dtype=np.int16), -1)
        a[S:, :V] = np.maximum(rng.integers(-3, 3, (3, V), dtype=np.int16), -1)
        _ARENAS[V, S] = torch.from_numpy(a)
    return _ARENAS[V, S]


def scenario(k, S, rng):
    """(base, state) of a logits row: 0 unguided, 1 all allowed, 2 only v = 0, 3 only v = V - 1,
    4 a random state of A, 5 grammar B (non-zero base), 6 the last arena row."""
    return [(-1, 0), (0, 0), (0, 1), (0, 2), (0, int(rng.integers(min(3, S - 1), S))), (S, int(rng.integers(0, 2))),
            (S, 2)][k % 7]


def launches(n, S, rng):
    """Per launch (base [n], rows [n], state [R]): every scenario lands on some row of some
    launch, unguided rows in every launch, engine rows a permutation (R = n + 3)."""
    R = n + 3
    for shift in range(7 if n < 7 else 2):
        base, state = np.full(n, -1, np.int32), rng.integers(0, 3, R).astype(np.int32)
        rows = rng.permutation(R)[:n].astype(np.int32)
        for i in range(n):
            k = (i + shift) % 7 if n > 1 else (shift + 1) % 7
            base[i], state[rows[i]] = scenario(k, S, rng)
        if n > 1:
            base[(shift * 3) % n] = -1  # (and an unguided row wherever the cycle put none)
        yield base, rows, state


def logits_of(n, V, ld, pad):
    torch.manual_seed(V + n)
    buf = 4 * torch.randn(n, ld + pad)
    buf[:, ::101] = -0.0
    buf[:, 5::211] = float("-inf")   # entries that are -inf already, and +inf
    buf[:, 7::223] = float("inf")
    return buf


@pytest.mark.parametrize("n,V,S", CASES)
def test_grammar_mask_bit_exact(gpu, n, V, S):
    arena = arena_of(V, S)
    arena_d = arena.to(gpu)
    rng = np.random.default_rng(n)
    # contiguous rows (ld = V: odd for V = 1003, so most rows start off a 16-B boundary), and for
    # the small case rows inside a wider buffer whose padding must stay as it was
    for pad in ((0, 3) if V == 1003 else (0,)):
        buf = logits_of(n, V, V, pad)
        for base, rows, state in launches(n, S, rng):
            want = buf.clone()
            mask_reference(want[:, :V], arena, base, state, rows)
            got_buf = buf.clone().to(gpu)
            got = got_buf[:, :V]
            assert got.stride(0) == V + pad
            ops.grammar_mask(got, arena_d, torch.from_numpy(base).to(gpu), torch.from_numpy(rows).to(gpu),
                             torch.from_numpy(state).to(gpu))
            # the int32 views: -inf exactly where the reference has it, every other bit untouched
            assert torch.equal(got_buf.cpu().view(torch.int32), want.view(torch.int32))
            for i in np.nonzero(base < 0)[0]:
                assert torch.equal(got_buf[i].cpu().view(torch.int32), buf[i].view(torch.int32))
            # (what the scenarios promise: the single survivors are v = 0 and v = V - 1)
            for i in range(n):
                left = (~torch.isneginf(got[i].cpu())).nonzero().flatten().tolist()
                if base[i] == 0 and state[rows[i]] in (1, 2):
                    assert left == [0 if state[rows[i]] == 1 else V - 1]


@pytest.mark.parametrize("n,V,S", CASES)
def test_grammar_advance_exact(gpu, n, V, S):
    arena = arena_of(V, S)
    arena_d = arena.to(gpu)
    rng = np.random.default_rng(100 + n)
    for base, rows, state in launches(n, S, rng):
        tok = rng.integers(0, V, n)
        tok[::3] = [(-3, V + 10, 2**40, 0, V - 1, -2**40)[j % 6] for j in range(len(tok[::3]))]  # clamped
        want = torch.from_numpy(state.copy())
        advance_reference(arena, base, want, torch.from_numpy(tok), rows, vocab=V)
        got = torch.from_numpy(state.copy()).to(gpu)
        ops.grammar_advance(arena_d, torch.from_numpy(base).to(gpu), torch.from_numpy(rows).to(gpu), got,
                            torch.from_numpy(tok).to(gpu), V)
        assert got.cpu().tolist() == want.tolist()
        # rows that are not guided, and engine rows no logits row names, keep their state; a
        # token the state does not allow keeps it too (both happen in these launches)
        named = set(rows[base >= 0].tolist())
        assert all(int(want[r]) == int(state[r]) for r in range(len(state)) if r not in named)
    # nx < 0 keeps the state: only v = 0 is allowed in state 1 of grammar A
    st = torch.tensor([1], dtype=torch.int32, device=gpu)
    one = lambda v: torch.tensor([v], dtype=torch.int32, device=gpu)  # noqa: E731
    ops.grammar_advance(arena_d, one(0), one(0), st, torch.tensor([V - 1], device=gpu), V)
    assert st.tolist() == [1]
    ops.grammar_advance(arena_d, one(0), one(0), st, torch.tensor([-7], device=gpu), V)  # clamps to v = 0
    assert st.tolist() == [S - 1]


@pytest.mark.parametrize("V,reps", [(1000, 1), (32000, 1), (1000, 3)], ids=["split-1000", "split-32000", "single-stage"])
def test_sample_ext_guided_rows_match_reference(gpu, monkeypatch, V, reps):
    """One guided row per (top_k, top_p, u) and allowed-set size, on logits with many ties; rows
    with fewer allowed tokens than top_k, full-vocabulary rows (top_k 0 and 2000), greedy rows
    and unguided rows.  ``reps`` = 3 makes the batch large enough for the single-stage draw."""
    rng = np.random.default_rng(V)
    combos = [(k, p, u) for k in (0, 1, 2, 2000) for p in (1.0, 0.3) for u in (0.0, 0.5, 1 - 2**-24)] * reps
    sizes = [1, 2, 3, 5, 40]
    params, us, allowed = [], [], []
    for j, (k, p, u) in enumerate(combos):
        params.append(SamplingParams(temperature=1.0, top_k=k, top_p=p))
        us.append(u)
        allowed.append(sizes[j % len(sizes)])
    for extra in range(4):  # greedy guided, greedy unguided, sampling unguided x 2
        params.append(SamplingParams(temperature=0.0 if extra < 2 else 0.8, top_k=0 if extra != 3 else 7))
        us.append(0.25)
        allowed.append(3 if extra == 0 else 0)
    n = len(params)
    S = n + 1
    ldv = (V + 7) // 8 * 8
    arena = np.full((S + 2, ldv), -1, np.int16)
    base = np.full(n, -1, np.int32)
    rows = rng.permutation(n + 2)[:n].astype(np.int32)
    state = np.zeros(n + 2, np.int32)
    for i, cnt in enumerate(allowed):
        if cnt:
            ids = rng.choice(V, cnt, replace=False)
            if i % 4 == 0:
                ids[0] = 0
            if i % 4 == 1:
                ids[-1] = V - 1
            arena[2 + i, ids] = (i + 1) % S   # a grammar at base 2 whose state i is logits row i's
            base[i], state[rows[i]] = 2, i
    arena_t = torch.from_numpy(arena)
    logits = (torch.from_numpy(rng.integers(0, 9, (n, V))).float() / 2).to(torch.bfloat16)  # ties everywhere
    masked = mask_reference(logits.float().clone(), arena_t, base, state, rows)
    u_t = torch.tensor(us, dtype=torch.float32)
    want = sample_reference(masked, torch.tensor([p.temperature for p in params]),
                            torch.tensor([p.top_k for p in params]), torch.tensor([p.top_p for p in params]), u_t)
    want_state = torch.from_numpy(state.copy())
    advance_reference(arena_t, base, want_state, want, rows, vocab=V)
    monkeypatch.setattr(torch, "rand", lambda *a, **kw: u_t.clone().to(kw.get("device", "cpu")))
    sampler, arena_d, logits_d = Sampler(gpu), arena_t.to(gpu), logits.to(gpu)
    none = np.full(n, -1, np.int32)
    runs = []
    for _ in range(3):
        gstate = torch.from_numpy(state.copy()).to(gpu)
        ext = SamplerExt(None, none, np.ones(n), np.zeros(n), np.zeros(n), none, V, arena_d, base, rows, gstate)
        toks, lp, ids = sampler.sample_ext(logits_d, params, ext)
        assert lp is None and ids is None
        runs.append((toks.cpu().tolist(), gstate.cpu().tolist()))
    assert runs[0] == runs[1] == runs[2]
    toks = runs[0][0]
    for i in range(n):  # every token is allowed, whatever else holds
        assert base[i] < 0 or arena[base[i] + state[rows[i]], toks[i]] >= 0, (i, toks[i], params[i], us[i])
    assert toks == want.tolist()
    assert runs[0][1] == want_state.tolist()
    assert torch.equal(logits_d.cpu(), logits)  # the caller's logits are never written
