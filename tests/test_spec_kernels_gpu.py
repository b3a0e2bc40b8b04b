"""``torch.ops.mlop.spec_accept`` / ``spec_propose`` (ops/csrc/spec.hip) against the contract of
runtime/spec.py, on the MI355X: integers only, exact, three identical repeats.  And the existing
paged-attention entry on verify-shaped rows (q_len 1..8) whose pages hold stale KV beyond the
context: what a rejected draft leaves behind must never reach an output bit."""
import numpy as np
import pytest
import torch

from mlopamd import ops
from mlopamd.ops import reference as ref
from mlopamd.runtime.spec import out_width, propose_reference, spec_accept_cpu
from test_kernels_gpu import close, make_meta

pytestmark = pytest.mark.gpu
bf = torch.bfloat16

K = 7
W = out_width(K)
MAXLEN = 4100
R = 20
ROWS8 = [17, 3, 11, 0, 19, 5, 8, 13]  # non-contiguous, unordered
SENT = -7
LENGTHS = (255, 256, 257, 511, 513, 4096)


def _histories(n_max, n_min):
    """(name, tokens): every length the kernel's strides and edges care about, histories dense
    in competing matches (3-token vocabulary), with none, with ids up to 128255, and planted ones."""
    rng = np.random.default_rng(100 * n_max + n_min)
    out = []
    for L in (1, n_min, n_min + 1, n_max, n_max + 1, *LENGTHS):
        out.append((f"dense{L}", rng.integers(0, 3, size=L).tolist()))
        out.append((f"sparse{L}", rng.integers(0, 128256, size=L).tolist()))
        out.append((f"period1_{L}", [128255] * L))
    for L in LENGTHS:
        fill = (128255 - np.arange(L)).tolist()  # all distinct: no accidental match
        suf = [7, 128255, 9, 128254, 11, 128253, 13, 128252][:n_max]
        n = len(suf)
        h = list(fill)
        h[:n], h[L - n:] = suf, suf
        out.append((f"only_p0_{L}", h))
        h = list(fill)  # the last legal p = L - n - 1: the match overlaps the suffix by n - 1
        h[L - n - 1:] = [5] * (n + 1)
        out.append((f"last_p_{L}", h))
        h = list(fill)  # an old match with many followers and a recent one with two
        h[L - n:] = suf
        h[10:10 + n] = suf
        h[L - n - 2 - n:L - n - 2] = suf
        out.append((f"competing_{L}", h))
        h = list(fill)  # only a shorter n-gram matches: fallback from n_max
        h[L - n:] = suf
        h[40:40 + n_min] = suf[n - n_min:]
        out.append((f"fallback_{L}", h))
    return out


def _run_propose(gpu, hists, caps, rows, n_max, n_min):
    B = len(rows)
    hist = torch.full((R, MAXLEN), 99, dtype=torch.int32)
    hlen = torch.zeros(R, dtype=torch.int32)
    for r, h in zip(rows, hists):
        hist[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
        hlen[r] = len(h)
    hist, hlen = hist.to(gpu), hlen.to(gpu)
    rows_d = torch.tensor(rows, dtype=torch.int32, device=gpu)
    cap_d = torch.tensor(caps, dtype=torch.int32, device=gpu)
    res = []
    for _ in range(3):
        out = torch.full((B, W), SENT, dtype=torch.int32, device=gpu)
        ops.spec_propose(hist, hlen, rows_d, cap_d, n_max, n_min, out)
        res.append(out.cpu().numpy())
    assert (res[0] == res[1]).all() and (res[0] == res[2]).all(), "three identical repeats"
    return res[0]


@pytest.mark.parametrize("n_max,n_min", [(3, 1), (8, 2), (1, 1), (8, 8)])
@pytest.mark.parametrize("B", [1, 8])
def test_spec_propose_matches_reference(gpu, n_max, n_min, B):
    cases = [(name, h, cap) for name, h in _histories(n_max, n_min) for cap in (0, 1, K)]
    rows = ROWS8[:B] if B > 1 else [14]
    seen = set()
    for i in range(0, len(cases), B):
        chunk = cases[i:i + B]
        chunk = (chunk * B)[:B]
        got = _run_propose(gpu, [h for _, h, _ in chunk], [c for _, _, c in chunk], rows, n_max, n_min)
        for j, (name, h, cap) in enumerate(chunk):
            want = propose_reference(h, cap, n_max, n_min)
            assert got[j, 1] == len(want), (name, cap, got[j].tolist(), want)
            assert got[j, 3 + K:3 + K + len(want)].tolist() == want, (name, cap, got[j].tolist(), want)
            # nothing else of the row is written
            assert (got[j, 3 + K + len(want):] == SENT).all() and got[j, 0] == SENT
            assert (got[j, 2:3 + K] == SENT).all()
            seen.add(len(want))
    assert seen >= {0, 1, K}, seen  # the cases reach empty, one-token and full proposals


@pytest.mark.parametrize("B", [1, 8])
def test_spec_accept_matches_reference(gpu, B):
    rng = np.random.default_rng(B)
    rows = ROWS8[:B] if B > 1 else [14]
    for trial in range(6):
        nd = rng.integers(0, K + 1, size=B)
        if trial == 0:
            nd[:] = 0           # plain decode rows
        if trial == 1:
            nd[:] = K
        q_len = 1 + nd
        q0 = np.cumsum(q_len) - q_len
        T = int(q_len.sum())
        sampled = rng.integers(0, 128256, size=T).astype(np.int64)
        sampled[-1] = 128255
        drafts = np.zeros((B, K), np.int32)
        for i in range(B):
            # (trial 1: every other row accepts all of its drafts)
            a = int(nd[i]) if (trial == 1 and i % 2 == 0) else int(rng.integers(0, nd[i] + 1))
            drafts[i, :nd[i]] = sampled[q0[i]:q0[i] + nd[i]]
            if a < nd[i]:
                drafts[i, a] = (drafts[i, a] + 1) % 128256  # the first mismatch at j = a
                drafts[i, a + 1:nd[i]] = sampled[q0[i] + a + 1:q0[i] + nd[i]]  # later matches do not count
        hist = rng.integers(0, 128256, size=(R, MAXLEN)).astype(np.int32)
        hlen = rng.integers(1, 4000, size=R).astype(np.int32)
        hlen[rows[0]] = MAXLEN - 1      # the append is clamped to the row
        hlen[rows[-1]] = 1 if B > 1 else MAXLEN - 1
        out = np.full((B, W), SENT, np.int32)
        e_hist, e_len, e_out = hist.copy(), hlen.copy(), out.copy()
        spec_accept_cpu(sampled, q0.astype(np.int32), drafts, nd.astype(np.int32), np.asarray(rows, np.int32),
                        e_hist, e_len, e_out)
        d = lambda a: torch.from_numpy(np.array(a)).to(gpu)  # noqa: E731  (a copy: hist and hist_len are written)
        args = (d(sampled), d(q0.astype(np.int32)), d(drafts), d(nd.astype(np.int32)), d(np.asarray(rows, np.int32)))
        for _ in range(3):
            hist_d, len_d, out_d = d(hist), d(hlen), d(out)
            ops.spec_accept(*args, hist_d, len_d, out_d)
            assert (out_d.cpu().numpy() == e_out).all(), (trial, out_d.cpu().numpy(), e_out)
            assert (len_d.cpu().numpy() == e_len).all()
            assert (hist_d.cpu().numpy() == e_hist).all()
        assert (e_out[:, 0] >= 1).all() and (e_out[:, 0] <= nd + 1).all()


def test_accept_then_propose_on_one_stream(gpu):
    """The engine's use: spec_propose right behind spec_accept sees the appended tokens."""
    seg = [5, 6, 7, 8, 9]
    hist = torch.zeros(R, MAXLEN, dtype=torch.int32)
    hist[3, :12] = torch.tensor(seg + seg + [5, 6], dtype=torch.int32)
    hlen = torch.zeros(R, dtype=torch.int32)
    hlen[3] = 12
    hist, hlen = hist.to(gpu), hlen.to(gpu)
    i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=gpu)  # noqa: E731
    out = torch.full((1, W), SENT, dtype=torch.int32, device=gpu)
    sampled = torch.tensor([7, 8, 1], dtype=torch.int64, device=gpu)
    ops.spec_accept(sampled, i32([0]), i32([[7, 8, 9, 0, 0, 0, 0]]), i32([3]), i32([3]), hist, hlen, out)
    ops.spec_propose(hist, hlen, i32([3]), i32([K]), 3, 1, out)
    o = out.cpu().numpy()[0]
    h = seg + seg + [5, 6, 7, 8]   # the third token (1 != 9) ends the run: 7, 8 accepted, then 1 emitted
    assert o[0] == 3 and o[2:5].tolist() == [7, 8, 1] and int(hlen[3]) == 15
    want = propose_reference(h + [1], K, 3, 1)
    assert o[1] == len(want) and o[3 + K:3 + K + len(want)].tolist() == want


@pytest.mark.parametrize("Hq,Hkv", [(32, 8), (8, 1), (16, 8)])
@pytest.mark.parametrize("mode", ["single", "split", "split_fused"])
def test_stale_kv_beyond_context_is_never_read(gpu, Hq, Hkv, mode, attn_fused_all):
    """Verify-shaped rows (q_len 1..8; contexts ending mid-page and on a page edge): the KV slots
    beyond ctx_len inside the last page (a rejected draft's) and the page a short block-table row
    points at (0) hold huge finite values.  The output equals the clean launch bit for bit."""
    torch.manual_seed(0)
    np.random.seed(0)
    G, NB = Hq // Hkv, 300
    q_lens = [1, 2, 3, 4, 5, 6, 7, 8]
    ctx_lens = [40, 48, 100, 128, 333, 512, 9, 1040]
    kw = {} if mode == "single" else dict(part_tokens=128, nparts=9)
    kc = torch.randn(NB, Hkv, 16, 128, device=gpu, dtype=bf)
    vc = torch.randn(NB, Hkv, 16, 128, device=gpu, dtype=bf)
    m, T = make_meta(gpu, q_lens, ctx_lens, Hkv, G, NB, **({"part_tokens": 2048, "nparts": 1} if not kw else kw))
    if mode == "split_fused":
        m.part_sem = torch.zeros(m.tile_seq.numel() * Hkv, dtype=torch.int32, device=gpu)
    q = torch.randn(T, Hq, 128, device=gpu, dtype=bf)
    clean = ops.paged_attention(q, kc, vc, m).clone()
    close(clean, ref.paged_attention(q, kc, vc, m), atol=2e-2, rtol=2e-2)
    bt, ctx = m.block_tables.cpu().numpy(), m.ctx_len.cpu().numpy()
    kp, vp = kc.clone(), vc.clone()
    n_poisoned = 0
    for r in np.nonzero(ctx)[0].tolist():
        c = int(ctx[r])
        if c % 16:
            page = int(bt[r, (c - 1) // 16])
            kp[page, :, c % 16:, :] = 3e38
            vp[page, :, c % 16:, :] = -3e38
            n_poisoned += 16 - c % 16
    kp[0], vp[0] = 3e38, -3e38  # what the block-table entries past a row's pages name
    assert n_poisoned > 0 and torch.isfinite(kp.float()).all()
    for _ in range(2):
        out = ops.paged_attention(q, kp, vp, m)
        assert torch.equal(out.view(torch.int16), clean.view(torch.int16))
        if mode == "split_fused":
            assert int(m.part_sem.abs().sum()) == 0
