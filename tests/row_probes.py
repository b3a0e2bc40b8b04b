"""Exact probes for the memory-bound row kernels: RMSNorm and add+RMSNorm (norm.hip), SiLU-mul in
both layouts and the embedding gather (elementwise.hip), and the stand-alone RoPE + paged-cache
writers for bf16 (rope_cache.hip) and fp8 pages (kv_fp8.hip).

Every probe takes a back end (``HipBackend``: the raw ops; ``RefBackend``: the CPU definitions
of mlopamd.ops; the CPU test file adds faulty ones) and returns a list of failure messages,
empty when the back end passes.  Inputs are chosen so that the expectation is one bf16 value,
or one of two where an fp32 evaluation within a derived slop (gemm_probes.FP32_SLOP, silu_slop) can land on either side of a bf16
rounding boundary, and "equal" means the same bf16 bits (the sign of a zero is ignored: torch's
``!=``).  Output buffers carry PAD sentinel rows behind row M, caches and scale tensors are
prefilled.  profiles/row_probes.md has the reasoning, the case table and the measured results.
"""
import collections

import torch

from gemm_probes import (BS, CACHE_FILL, EPS, PAD, POS_ROWS, SENTINEL, ULP, _gen, bf16_either,
                         check_rope, cos_sin, describe, resid, rope_meta, sentinel_bad, silu_mul64, ulp_bad)

bf = torch.bfloat16
NAN = float("nan")
FP8 = torch.float8_e4m3fn
FILL8 = 0x2A            # prefill of fp8 pages and scale bytes
LAUNCH_BYTES = 64 << 20  # the largest single tensor of a launch


# ------------------------------------------------------------- back ends --

class HipBackend:
    """The raw ops the wrappers of mlopamd.ops call."""

    def __init__(self, device):
        from mlopamd import ops

        self.ops, self.device = ops, device
        ops.load()

    def rmsnorm(self, out, x, w, eps):
        torch.ops.mlop.rmsnorm(out, x, w, eps)

    def add_rmsnorm(self, out, res, x, w, eps):
        torch.ops.mlop.add_rmsnorm(out, res, x, w, eps)

    def silu_mul(self, out, x, interleaved):
        torch.ops.mlop.silu_mul(out, x, int(interleaved))

    def embedding(self, out, table, ids, vocab_start):
        torch.ops.mlop.embedding(out, table, ids, vocab_start)

    def rope(self, q, kc, vc, qkv, pos, cs, slots):
        torch.ops.mlop.rope_cache(q, kc, vc, qkv, pos, cs, slots)

    def rope_fp8(self, q, kc, vc, ks, vs, qkv, pos, cs, slots):
        torch.ops.mlop.rope_cache_fp8(q, kc, vc, ks, vs, qkv, pos, cs, slots)


class RefBackend:
    """The CPU definitions of mlopamd.ops: what the probes must accept."""

    def __init__(self):
        from mlopamd import ops

        self.ops = ops

    def rmsnorm(self, out, x, w, eps):
        out.copy_(self.ops.rmsnorm(x, w, eps))

    def add_rmsnorm(self, out, res, x, w, eps):
        self.ops.add_rmsnorm(x, res, w, eps, out=out)

    def silu_mul(self, out, x, interleaved):
        out.copy_(self.ops.silu_mul(x, interleaved=bool(interleaved)))

    def embedding(self, out, table, ids, vocab_start):
        out.copy_(self.ops.embedding(ids, table, vocab_start))

    def rope(self, q, kc, vc, qkv, pos, cs, slots):
        self.ops.rope_cache(qkv, pos, cs, slots, kc, vc, q.shape[1], q_out=q)

    def rope_fp8(self, q, kc, vc, ks, vs, qkv, pos, cs, slots):
        self.ops.rope_cache(qkv, pos, cs, slots, kc, vc, q.shape[1], q_out=q, k_scale=ks, v_scale=vs)


def _padded(M, n, device, fill=SENTINEL):
    return torch.full((M + PAD, n), fill, dtype=bf, device=device)


def _msgs(*ms):
    return [m for m in ms if m]


# =================================================================== norm ==

NormCase = collections.namedtuple("NormCase", "id M H add")
WAVE_MIN_M = 256


def norm_form(M, H):
    """The launch form of an [M, H] norm: a restatement of ``dispatch_wave()`` and ``dispatch()`` of
    mlopamd/ops/csrc/norm.hip.  ("wave", VPL), or ("block", VPT, threads)."""
    if M >= WAVE_MIN_M and H % 512 == 0 and H // 512 in (1, 2, 4, 8, 16):
        return ("wave", H // 512)
    nvec, vpt = H // 8, 1
    while vpt < 8 and nvec // vpt > 512:
        vpt <<= 1
    return ("block", vpt, (-(-nvec // vpt) + 63) // 64 * 64)


def last_wave_idle(M, H):
    """A block launch whose thread count was rounded up: the last wave has idle lanes."""
    f = norm_form(M, H)
    return f[0] == "block" and -(-(H // 8) // f[1]) % 64 != 0


NORM_SHAPES = [(3, 8), (5, 512), (2, 4096), (3, 4104), (2, 5120), (2, 8192), (3, 8200), (2, 14336), (2, 16384),
               (2, 16392), (2, 16416), (2, 32768), (2, 65536),
               (256, 4104), (257, 5120),                    # many rows the wave form refuses
               (256, 512), (257, 512), (256, 1024), (258, 1024), (256, 2048), (259, 2048),
               (256, 4096), (257, 4096), (256, 8192), (258, 8192)]
NORM_CASES = [NormCase(f"{'add' if add else 'norm'}-M{M}-H{H}", M, H, add) for add in (False, True) for M, H in NORM_SHAPES]
HOT, LOUD, TINY_HOT = 2.0, 16.0, 2.0 ** -10


def norm_weights(H, gen):
    """bf16 1 + 0.1 randn with 0, -1 and 2 at a few columns."""
    w = (1 + 0.1 * torch.randn(H, generator=gen, device=gen.device)).to(bf)
    for c, v in ((3, 0.0), (H // 2 + 1, -1.0), (H - 2, 2.0)):
        w[c] = v
    return w


def hot_columns(H):
    """Column 8 v + v % 8 of every 16-byte vector v, and all 8 positions of the first and the last."""
    nvec = H // 8
    cols = [8 * v + v % 8 for v in range(nvec)] + list(range(8)) + list(range(H - 8, H))
    return list(dict.fromkeys(cols))


def hot_value(A, H, eps=EPS):
    """fp64 A inv of a row whose only element is A."""
    return A / (A * A / H + eps) ** 0.5


def _bf16_of(v):
    return torch.tensor(v, dtype=torch.float64).float().to(bf)


def hot_is_stable(A, H):
    """A inv lies farther than 2^-12 (relative) from a bf16 rounding boundary."""
    c = hot_value(A, H)
    return bool(_bf16_of(c * (1 - 2.0 ** -12)) == _bf16_of(c * (1 + 2.0 ** -12)))


def membership_rows(M, H):
    """Rows per membership launch: at most 254 on the block form (the case's own M where many rows
    fall back to it), and on the wave form one launch of at least 256 rows with M's M % 4."""
    n_hot = len(hot_columns(H))
    if norm_form(M, H)[0] == "block":
        return 254 if M < WAVE_MIN_M else M
    L = max(M, 2 * n_hot)
    L += (M - L) % 4
    assert L * H * 2 <= LAUNCH_BYTES
    return L


def norm_either(r, w, eps=EPS):
    """(e_lo, e_hi, e_nearest) bf16: w bf16(r inv) with inv anywhere within FP32_SLOP of the fp64 one."""
    r64 = r.double()
    c = r64 * torch.rsqrt(r64.pow(2).mean(-1, keepdim=True) + eps)
    wf = w.float()
    lo, hi = ((e.float() * wf).to(bf) for e in bf16_either(c))
    return lo, hi, (c.float().to(bf).float() * wf).to(bf)


def _launch_norm(be, add, M, x, res, w, eps=EPS):
    """One launch into sentinel-padded buffers.  ``res`` (add form) is the residual input; returns
    (out buffer, residual buffer or None)."""
    H = x.shape[1]
    out = _padded(M, H, x.device)
    if not add:
        be.rmsnorm(out[:M], x, w, eps)
        return out, None
    rbuf = _padded(M, H, x.device)
    rbuf[:M] = res
    be.add_rmsnorm(out[:M], rbuf[:M], x, w, eps)
    return out, rbuf


def _check_either(what, out, M, r, w, info, eps=EPS):
    lo, hi, near = norm_either(r, w, eps)
    got = out[:M]
    bad = (got != lo) & (got != hi)
    info["checked"] = info.get("checked", 0) + got.numel()
    info["second"] = info.get("second", 0) + int(((got != near) & ~bad).sum())
    info["either"] = max(info.get("either", 0.0), float((lo != hi).double().mean()))
    return _msgs(describe(what, bad, got, lo), sentinel_bad(what, out, M))


def _check_residual(what, rbuf, M, x, res):
    exp = (x.double() + res.double()).float().to(bf)
    return _msgs(describe(what + " residual", rbuf[:M] != exp, rbuf[:M], exp), sentinel_bad(what + " residual", rbuf, M))


def _split(t, add, odd_rows_to_res=None):
    """(x, residual) with x + residual = t: all of t in x, or (add form) in the residual on the
    rows of the mask; None for the plain form's residual."""
    if not add:
        return t, None
    x, r = t.clone(), torch.zeros_like(t)
    r[odd_rows_to_res] = t[odd_rows_to_res]
    x[odd_rows_to_res] = 0
    return x, r


def probe_norm_membership(case, be, device, info=None, sample=False):
    """One-hot rows (A = 2 at a hot column) alternating with loud rows (all 16): every vector of the
    row is hot once.  ``sample``: the first, a middle and the last launch only."""
    info = {} if info is None else info
    M, H, add = case.M, case.H, case.add
    assert hot_is_stable(HOT, H), (H, hot_value(HOT, H))
    w = norm_weights(H, _gen(case.id, device))
    cols = hot_columns(H)
    L = membership_rows(M, H)
    per = (L + 1) // 2  # hot rows of a launch: rows 0, 2, 4, ...
    launches = range(-(-len(cols) // per))
    if sample and len(launches) > 3:
        launches = [0, len(launches) // 2, len(launches) - 1]
    c = _bf16_of(hot_value(HOT, H)).to(device)
    msgs = []
    info["launches"], info["rows"] = len(launches), L
    for n in launches:
        hc = torch.tensor([cols[(n * per + i) % len(cols)] for i in range(per)], device=device)
        hr = torch.arange(0, L, 2, device=device)
        t = torch.full((L, H), LOUD, dtype=bf, device=device)
        t[hr] = 0
        t[hr, hc] = HOT
        exp = w.expand(L, H).clone()
        exp[hr] = 0
        exp[hr, hc] = (c.float() * w[hc].float()).to(bf)
        if add:  # hot element in x on even hot rows, in the residual on odd ones; loud rows 8 + 8
            to_res = torch.zeros(L, dtype=torch.bool, device=device)
            to_res[hr[1::2]] = True
            x, r = _split(t, True, to_res)
            x[1::2], r[1::2] = LOUD / 2, LOUD / 2
        else:
            x, r = t, None
        out, rbuf = _launch_norm(be, add, L, x, r, w)
        what = f"{case.id} membership launch {n}"
        msgs += _msgs(describe(what, out[:L] != exp, out[:L], exp), sentinel_bad(what, out, L))
        if add:
            msgs += _msgs(describe(what + " residual", rbuf[:L] != t, rbuf[:L], t), sentinel_bad(what + " residual", rbuf, L))
        info["checked"] = info.get("checked", 0) + L * H
        if len(msgs) > 4:
            break
    return msgs


def eps_conditions(H):
    """The expected bf16 hot value of the tiny one-hot row under eps, no eps and eps = 1e-6."""
    return [_bf16_of(hot_value(TINY_HOT, H, e)) if e else _bf16_of(H ** 0.5) for e in (EPS, 0.0, 1e-6)]


def probe_norm_eps(case, be, device, info=None):
    """An all-zero row gives exact zeros; a one-hot row with A^2 / H << eps gives A rsqrt(eps)."""
    info = {} if info is None else info
    M, H, add = case.M, case.H, case.add
    e = eps_conditions(H)
    assert e[0] != e[1] and e[0] != e[2], (H, e)
    w = norm_weights(H, _gen(case.id, device))
    t = torch.zeros(M, H, dtype=bf, device=device)
    rows = torch.arange(1, M, 2, device=device)
    t[rows, (rows * 131 + 4) % H] = TINY_HOT
    to_res = torch.zeros(M, dtype=torch.bool, device=device)
    to_res[rows[1::2]] = True
    x, r = _split(t, add, to_res)
    out, rbuf = _launch_norm(be, add, M, x, r, w)
    msgs = _check_either(f"{case.id} eps", out, M, t, w, info)
    zero = out[:M:2]
    if not bool((zero == 0).all()):
        msgs.append(f"{case.id} eps: an all-zero row is not exactly zero")
    if add:
        msgs += _check_residual(f"{case.id} eps", rbuf, M, x, r)
    return msgs


def probe_norm_data(case, be, device, info=None):
    """Integer rows (the sum of squares is exact in fp32 in any order): both roundings of HF's
    w bf16(x inv), every column, the weights."""
    info = {} if info is None else info
    M, H, add = case.M, case.H, case.add
    gen = _gen(case.id, "cpu")  # drawn on the CPU: every back end gets the tensors the conditions were checked on
    w = norm_weights(H, gen).to(device)
    if add:
        x = torch.randint(-4, 5, (M, H), generator=gen).to(bf).to(device)
        r = torch.randint(-4, 5, (M, H), generator=gen).to(bf).to(device)
        t = x + r
    else:
        x, r = resid((M, H), gen).to(device), None
        t = x
    out, rbuf = _launch_norm(be, add, M, x, r, w)
    msgs = _check_either(f"{case.id} data", out, M, t, w, info)
    if add:
        msgs += _check_residual(f"{case.id} data", rbuf, M, x, r)
    return msgs


# sums that fall on a bf16 tie or beside one: 257 -> 256, 259 -> 260, -257 -> -256, 385.5 -> 386, 256.5 -> 256,
# and further ties 257 + 2 n (each another mantissa: another chance that the unrounded sum shows)
PLANTS = ((256.0, 1.0), (258.0, 1.0), (-256.0, -1.0), (384.0, 1.5), (0.5, 256.0)) + tuple((256.0 + 2 * n, 1.0) for n in range(2, 8))
PLANT_ROUNDED = (256.0, 260.0, -256.0, 386.0, 256.0) + tuple(256.0 + 2 * n + 2 * (n % 2) for n in range(2, 8))


def plant_columns(m, H):
    n = min(len(PLANTS), H)
    return [(m * 37 + j * (H // n)) % H for j in range(n)]


def residual_inputs(case, device):
    """x, r (small integers with the plants in the first rows), w, the planted rows.  Drawn on the
    CPU, so the builder's conditions hold for the very tensors every back end gets."""
    M, H = case.M, case.H
    gen = _gen(case.id + "/residual", "cpu")
    x = torch.randint(-4, 5, (M, H), generator=gen).to(bf)
    r = torch.randint(-4, 5, (M, H), generator=gen).to(bf)
    rows = list(range(min(M, 3)))
    for m in rows:
        for c, (a, b) in zip(plant_columns(m, H), PLANTS):
            x[m, c], r[m, c] = a, b
    return x.to(device), r.to(device), norm_weights(H, gen).to(device), rows


def probe_norm_residual(case, be, device, info=None):
    """add form only: the stored residual is bf16(x + r) (ties to even) and the norm is taken from
    the rounded residual."""
    info = {} if info is None else info
    assert case.add
    M = case.M
    x, r, w, rows = residual_inputs(case, device)
    rounded = (x.double() + r.double()).float().to(bf)
    for m in rows:
        for c, e in zip(plant_columns(m, case.H), PLANT_ROUNDED):
            assert float(rounded[m, c]) == e
    # the unrounded sum would give another expected value somewhere in the planted rows
    lo, hi, _ = norm_either(rounded[rows], w)
    ulo, uhi, _ = norm_either(x[rows].double() + r[rows].double(), w)
    info["unrounded_differs"] = int(((ulo != lo) & (ulo != hi) & (uhi != lo) & (uhi != hi)).sum())
    assert info["unrounded_differs"] >= 1
    out, rbuf = _launch_norm(be, True, M, x, r, w)
    return _check_residual(f"{case.id} rounding", rbuf, M, x, r) + _check_either(f"{case.id} rounding", out, M, rounded, w, info)


def probe_norm_empty(be, device, add):
    H = 512
    w = norm_weights(H, _gen("empty", device))
    x = torch.zeros(0, H, dtype=bf, device=device)
    out, rbuf = _launch_norm(be, add, 0, x, x.clone() if add else None, w)
    return _msgs(sentinel_bad("0-row norm", out, 0), sentinel_bad("0-row residual", rbuf, 0) if add else None)


NORM_PROBES = {"membership": probe_norm_membership, "eps": probe_norm_eps, "data": probe_norm_data,
               "residual": probe_norm_residual}


def norm_probes_of(case):
    return [p for p in NORM_PROBES if p != "residual" or case.add]


# =============================================================== SiLU-mul ==

SiluCase = collections.namedtuple("SiluCase", "id M I interleaved")
SILU_CAP = 2048 * 256  # vectors one pass of the grid covers (elementwise.hip launch_silu_mul)
SILU_SHAPES = [(1, 16), (3, 48), (5, 40), (37, 14336), (293, 14336)]
# the interleaved layout is groups of 16 gates and 16 ups: I = 40 (I / 8 odd) has none, the op refuses it
SILU_CASES = [SiluCase(f"silu-M{M}-I{I}-{'il' if il else 'plain'}", M, I, il)
              for M, I in SILU_SHAPES for il in (0, 1) if not (il and I % 16)]
SILU_REFUSED = (5, 40)
N_FINITE = 65280
FLUSH_BELOW = -87.25  # fp32 exp(-g) > 2^126: v_rcp may flush its result


def silu_vectors(case):
    return case.M * (case.I // 8)


def finite_bf16(device):
    b = torch.arange(65536, dtype=torch.int32, device=device)
    b = b[(b & 0x7F80) != 0x7F80]
    assert b.numel() == N_FINITE
    return b.to(torch.int16).view(bf)


def silu_slop(g):
    """Relative error bound of fp32 g / (1 + exp2(-g log2e)) with v_exp and v_rcp (profile)."""
    return (g.abs() + 4) * 2.0 ** -23


def _launch_silu(case, be, g, u):
    """g, u [M, I] -> the padded output buffer of a launch in the case's layout."""
    x = torch.cat([g, u], 1)
    if case.interleaved:  # the engine's own helper, for columns
        x = be.ops.interleave_gate_up(g.t().contiguous(), u.t().contiguous()).t().contiguous()
        assert torch.equal(be.ops.deinterleave_cols(x), torch.cat([g, u], 1))
    out = _padded(case.M, case.I, g.device)
    be.silu_mul(out[:case.M], x, case.interleaved)
    return out


def probe_silu_gates(case, be, device, info=None):
    """Every finite bf16 bit pattern as a gate (where the tensor has room), ups in {+-1, +-0.5}."""
    info = {} if info is None else info
    M, I = case.M, case.I
    gen = _gen(case.id, device)
    idx = (torch.arange(M * I, device=device) * 4093 + 17) % N_FINITE  # 4093 is coprime to 65280
    g = finite_bf16(device)[idx].view(M, I)
    info["gates"] = int(torch.unique(idx).numel())
    u = torch.tensor([1, -1, 0.5, -0.5], dtype=bf, device=device)[torch.randint(0, 4, (M, I), generator=gen, device=device)]
    out = _launch_silu(case, be, g, u)
    exp = silu_mul64(g.double(), u.double())
    o = out[:M].double()
    flush = (g.double() < FLUSH_BELOW) & (o.abs() <= (1 + ULP) * exp.abs()) & (o * exp >= 0)
    bad = ulp_bad(out[:M], exp) & ~flush
    info["checked"], info["flush_rule"] = M * I, int((flush & ulp_bad(out[:M], exp)).sum())
    what = f"{case.id} gates"
    return _msgs(describe(what, bad, out[:M], exp), sentinel_bad(what, out, M))


def silu_either(g, u):
    s = g.double() / (1 + torch.exp(-g.double()))
    sl = silu_slop(g.double())
    uf = u.float()
    lo, hi = (((s * (1 + d)).float().to(bf).float() * uf).to(bf) for d in (-sl, sl))
    return lo, hi, (s.float().to(bf).float() * uf).to(bf)


def probe_silu_data(case, be, device, info=None):
    """Gates 3 randn, ups randn: bf16(bf16(silu(g)) u), silu within its derived fp32 slop."""
    info = {} if info is None else info
    M, I = case.M, case.I
    gen = _gen(case.id, "cpu")  # drawn on the CPU: every back end gets the tensors the condition was checked on
    g = (3 * torch.randn(M, I, generator=gen)).to(bf).to(device)
    u = torch.randn(M, I, generator=gen).to(bf).to(device)
    out = _launch_silu(case, be, g, u)
    lo, hi, near = silu_either(g, u)
    got = out[:M]
    bad = (got != lo) & (got != hi)
    info["checked"], info["second"] = M * I, int(((got != near) & ~bad).sum())
    info["either"] = float((lo != hi).double().mean())
    what = f"{case.id} data"
    return _msgs(describe(what, bad, got, lo), sentinel_bad(what, out, M))


def probe_silu_layout(case, be, device, info=None):
    """Gates all 8 (bf16(silu(8)) = 8), up of column i = (-1)^(i // 7) 2^(i % 7 - 3): a swapped half
    or a shifted group is wrong in every column it touches."""
    info = {} if info is None else info
    M, I = case.M, case.I
    i = torch.arange(I, device=device)
    up = (torch.pow(2.0, (i % 7 - 3).double()) * (1 - 2 * ((i // 7) % 2))).to(bf)
    g = torch.full((M, I), 8.0, dtype=bf, device=device)
    u = up.expand(M, I).contiguous()
    out = _launch_silu(case, be, g, u)
    exp = (8 * u.float()).to(bf)
    info["checked"] = M * I
    what = f"{case.id} layout"
    return _msgs(describe(what, out[:M] != exp, out[:M], exp), sentinel_bad(what, out, M))


def probe_silu_empty(be, device, interleaved):
    out = _padded(0, 32, device)
    be.silu_mul(out[:0], torch.zeros(0, 64, dtype=bf, device=device), interleaved)
    return _msgs(sentinel_bad("0-row silu_mul", out, 0))


SILU_PROBES = {"gates": probe_silu_gates, "data": probe_silu_data, "layout": probe_silu_layout}


# ============================================================== embedding ==

EmbCase = collections.namedtuple("EmbCase", "id H vocab_start T")
EMB_ROWS, EMB_VOCAB = 1000, 2000
EMB_CASES = [EmbCase(f"emb-H{H}-v{vs}-T{T}", H, vs, T) for H in (8, 256, 2048, 2056, 4096, 5120) for vs in (0, 500)
             for T in (1, 77)]


def emb_table(H, device):
    r = torch.arange(EMB_ROWS, dtype=torch.int32, device=device)[:, None]
    c = torch.arange(H, dtype=torch.int32, device=device)[None, :]
    return (((r * 131 + c * 7 + 1) & 0x7F7F).to(torch.int16)).view(bf)


def emb_ids(case, device):
    vs, ve = case.vocab_start, case.vocab_start + EMB_ROWS
    if case.T == 1:
        return torch.tensor([ve - 1], dtype=torch.long, device=device)
    special = [vs - 1, vs, ve - 1, ve, 0, EMB_VOCAB - 1, vs + 7, vs + 7, ve - 1, vs + 8]
    rest = torch.randint(0, EMB_VOCAB, (case.T - len(special),), generator=_gen(case.id, "cpu")).tolist()
    return torch.tensor(special + rest, dtype=torch.long, device=device)


def probe_embedding(case, be, device, info=None):
    info = {} if info is None else info
    table, ids = emb_table(case.H, device), emb_ids(case, device)
    T = ids.numel()
    out = _padded(T, case.H, device)
    be.embedding(out[:T], table, ids, case.vocab_start)
    local = ids - case.vocab_start
    inside = (local >= 0) & (local < EMB_ROWS)
    exp = torch.where(inside[:, None], table[local.clamp(0, EMB_ROWS - 1)], torch.zeros((), dtype=bf, device=device))
    info["checked"], info["inside"] = T * case.H, int(inside.sum())
    return _msgs(describe(case.id, out[:T] != exp, out[:T], exp), sentinel_bad(case.id, out, T))


def probe_embedding_empty(be, device):
    out = _padded(0, 256, device)
    be.embedding(out[:0], emb_table(256, device), torch.zeros(0, dtype=torch.long, device=device), 0)
    return _msgs(sentinel_bad("0-token embedding", out, 0))


# =================================================================== RoPE ==

RopeCase = collections.namedtuple("RopeCase", "id fp8 Hq Hkv T D strided")
ROPE_GEOMETRIES = [(32, 8), (8, 1), (64, 8), (16, 16), (4, 12)]
ROPE_CASES = [RopeCase(f"{'fp8' if f else 'bf16'}-q{hq}-kv{hkv}-T{T}", f, hq, hkv, T, 128, False)
              for f in (0, 1) for hq, hkv in ROPE_GEOMETRIES for T in (1, 17, 33)]
ROPE_CASES += [RopeCase(f"bf16-q8-kv1-T17-D{D}", 0, 8, 1, 17, D, False) for D in (64, 256)]
ROPE_CASES += [RopeCase(f"{'fp8' if f else 'bf16'}-q32-kv8-T17-strided", f, 32, 8, 17, 128, True) for f in (0, 1)]
SCALE_POS, SCALE_COS = 4097, 0.8755
# amax plants of the fp8 writer: (cache, amax).  14 2^k has mantissa exactly 0.875 (the step: x - 9),
# "scaled" is 256 at the position whose pair 0 has cos 0.8755: 224.128 in fp32, 224 = 14 * 16 in bf16
AMAX_PLANTS = (("k", 14 / 8), ("v", 56.0), ("k", 30.0), ("v", 15 / 4), ("k", 8.0), ("v", 0.5), ("k", 448.0),
               ("v", 448.0), ("k", 0.0), ("v", 0.0), ("k", "scaled"))


def rope_blocks(case):
    """(grid.y, trips of the item loop) of rope_cache_kernel<false>; for the fp8 writer the trips
    of its row loop (16 rows a trip) and whether the last one is partly populated."""
    if case.fp8:
        return (2, -(-2 * case.Hkv // 16), 2 * case.Hkv % 16 != 0)
    items = (case.Hq + case.Hkv) * (case.D // 16) + case.Hkv * (case.D // 8)
    by = min(2, -(-items // 256))
    return (by, -(-items // (256 * by)))


_SELECTOR = {}


def selector_table(D, device="cpu"):
    """[POS_ROWS, D] fp32 cos | sin: pair i of row p is the identity or a quarter turn (module
    profile), so a rotation is an exact signed permutation and every row differs from every other.
    Row SCALE_POS scales pair 0 by SCALE_COS instead (the fp8 writer's amax-after-rounding plant)."""
    key = (D, str(device))
    if key not in _SELECTOR:
        p = torch.arange(POS_ROWS)[:, None]
        i = torch.arange(D // 2)[None, :]
        turn = ((p >> (i % 13)) & 1) ^ ((i // 13) & 1)
        sin = turn * torch.where((p + i) % 3 == 0, -1, 1)
        cs = torch.cat([1 - turn, sin], 1).float()
        cs[SCALE_POS, 0], cs[SCALE_POS, D // 2] = SCALE_COS, 0.0
        _SELECTOR[key] = cs.to(device)
    return _SELECTOR[key]


def selector_meta(T, gen):
    """CPU int32 positions, slots and the page count.  Positions hold 0 and the table's last row,
    p and p + 1 on neighbouring tokens and SCALE_POS on token 4; slots are a permutation of the
    NB pages' slots without slot 0 (where a lost padding guard lands), with offsets 0 and 15 of
    page 3 in use and tokens 5 and T - 1 padding."""
    NB = T // BS + 8
    if T == 1:
        return torch.tensor([POS_ROWS - 1], dtype=torch.int32), torch.tensor([2 * BS + 15], dtype=torch.int32), NB
    pos = torch.randint(0, POS_ROWS - 1, (T,), generator=gen, dtype=torch.int32)
    pos[0], pos[1], pos[3], pos[4] = 0, POS_ROWS - 1, pos[2] + 1, SCALE_POS
    fixed = [3 * BS, 3 * BS + 15]
    free = [s for s in (1 + torch.randperm(NB * BS - 1, generator=gen)).tolist() if s not in fixed]
    slots = torch.tensor(free[:T], dtype=torch.int32)
    slots[2], slots[3] = fixed
    slots[5] = slots[T - 1] = -1
    return pos, slots, NB


def rope_values(shape, gen, e_lo=-6, e_hi=5):
    """+-m 2^e, m in 8..15: four significant bits, never zero."""
    m = torch.randint(8, 16, shape, generator=gen).double()
    e = torch.randint(e_lo, e_hi + 1, shape, generator=gen).double()
    s = 1 - 2 * torch.randint(0, 2, shape, generator=gen).double()
    return s * m * torch.pow(2.0, e)


def rope_inputs(case):
    """CPU qkv [T, (Hq + 2 Hkv) D] bf16, positions, slots, NB and the amax plants placed:
    {(token, cache, head): amax}."""
    gen = _gen(case.id, "cpu")
    T, Hq, Hkv, D = case.T, case.Hq, case.Hkv, case.D
    pos, slots, NB = selector_meta(T, gen)
    x = rope_values((T, Hq + 2 * Hkv, D), gen)
    live = [t for t in range(min(T, 5)) if int(slots[t]) >= 0]
    placed = {}
    for n, (cache, amax) in enumerate(AMAX_PLANTS):
        t = 4 if amax == "scaled" else live[(n // 2) % len(live)]
        h = (n // 2 // len(live)) % Hkv
        if (t, cache, h) in placed or (amax == "scaled" and (T < 5 or D != 128)):
            continue
        placed[(t, cache, h)] = amax
        row = x[t, Hq + h + (Hkv if cache == "v" else 0)]
        if amax == "scaled":
            row.copy_(rope_values((D,), gen, -4, 2))
            row[0], row[D // 2] = 256.0, 0.125
        elif amax == 0:
            row.zero_()
        else:
            k = int(torch.tensor(amax).log2().floor())  # below amax, within 9 binades: exact in e4m3
            row.copy_(rope_values((D,), gen, k - 12, k - 4))
            row[int(torch.randint(0, D, (1,), generator=gen))] = -amax
    return x.view(T, -1).float().to(bf), pos, slots, NB, placed


def rope_expect(qkv, pos, cs, Hq, Hkv, D):
    """bf16 (q, k, v) rows of the rotation, from fp64."""
    T, half = qkv.shape[0], D // 2
    x = qkv.double().reshape(T, Hq + 2 * Hkv, D)
    c = cs[pos.long()].double()
    cos, sin = c[:, None, :half], c[:, None, half:]
    x1, x2 = x[:, :Hq + Hkv, :half], x[:, :Hq + Hkv, half:]
    rot = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], -1).float().to(bf)
    return rot[:, :Hq], rot[:, Hq:], x[:, Hq + Hkv:].float().to(bf)


def fp8_expect(rows):
    """(dequantised fp32 rows, scale bytes) of bf16 rows [..., D] under the cache's rule: the
    smallest e with amax / 2^e <= 448, clamped; a zero row the smallest exponent."""
    xf = rows.float()
    a = xf.abs().amax(-1)
    m, x = torch.frexp(a.double())
    e = x - 9 + (m > 0.875).to(x.dtype)
    e = torch.where(a == 0, torch.full_like(e, -126), e).clamp(-126, 127)
    y = torch.ldexp(xf, -e[..., None]).to(FP8).float()
    return torch.ldexp(y, e[..., None]), (e + 127).to(torch.uint8)


def _scatter(shape, fill, dtype, blk, off, rows):
    full = torch.full(shape, fill, dtype=dtype)
    full[blk, :, off] = rows
    return full


def run_rope(case, be, device, qkv, pos, slots, NB, cs):
    """Launches the case's op; returns CPU (q, K cache, V cache, K scales, V scales), the fp8
    caches as bytes."""
    T, Hq, Hkv, D = qkv.shape[0], case.Hq, case.Hkv, case.D
    W = qkv.shape[1]
    if case.strided:  # a column slice of a wider buffer: row stride W + 24
        wide = torch.full((T, W + 24), NAN, dtype=bf, device=device)
        wide[:, 8:8 + W] = qkv.to(device)
        x = wide[:, 8:8 + W]
    else:
        x = qkv.to(device)
    q = torch.full((T, Hq, D), NAN, dtype=bf, device=device)
    pos, slots, cs = pos.to(device), slots.to(device), cs.to(device)
    if not case.fp8:
        kc = torch.full((NB, Hkv, BS, D), CACHE_FILL, dtype=bf, device=device)
        vc = kc.clone()
        be.rope(q, kc, vc, x, pos, cs, slots)
        return q.cpu(), kc.cpu(), vc.cpu(), None, None
    kc = torch.full((NB, Hkv, BS, D), FILL8, dtype=torch.uint8, device=device)
    vc, ks = kc.clone(), torch.full((NB, Hkv, BS), FILL8, dtype=torch.uint8, device=device)
    vs = ks.clone()
    be.rope_fp8(q, kc.view(FP8), vc.view(FP8), ks, vs, x, pos, cs, slots)
    return q.cpu(), kc.cpu(), vc.cpu(), ks.cpu(), vs.cpu()


def check_rope_rows(what, got, qkv, pos, slots, NB, cs, Hq, Hkv, D, fp8, info, exact_fp8=True):
    """q, caches and scales against the expectation; unwritten slots keep their prefill."""
    q, kc, vc, ks, vs = got
    qe, ke, ve = rope_expect(qkv, pos, cs, Hq, Hkv, D)
    live = slots >= 0
    blk, off = (slots[live] // BS).long(), (slots[live] % BS).long()
    msgs = _msgs(describe(what + " q", q != qe, q, qe))
    info["checked"] = info.get("checked", 0) + q.numel()
    shape = (NB, Hkv, BS, D)
    for name, cache, sc, e in (("K cache", kc, ks, ke[live]), ("V cache", vc, vs, ve[live])):
        info["checked"] += cache.numel()
        if not fp8:
            full = _scatter(shape, CACHE_FILL, bf, blk, off, e)
            msgs += _msgs(describe(f"{what} {name}", cache != full, cache, full))
            continue
        deq, byte = fp8_expect(e)
        if exact_fp8:  # every row is an e4m3 row already, but K at the position that scales pair 0
            inexact = (deq != e.float()).any(-1)
            info["inexact_rows"] = info.get("inexact_rows", 0) + int(inexact.sum())
            assert not bool(inexact[(pos[live] != SCALE_POS) | (name[0] == "V")].any()), what
        written = torch.zeros(shape[:3], dtype=torch.bool)
        written[blk, :, off] = True
        full_b = _scatter(shape[:3], FILL8, torch.uint8, blk, off, byte)
        msgs += _msgs(describe(f"{what} {name} scale bytes", (sc != full_b).view(NB, -1), sc.view(NB, -1), full_b.view(NB, -1)))
        got_deq = cache.view(FP8).float() * (sc.to(torch.int32) << 23).view(torch.float32)[..., None]
        full = _scatter(shape, 0.0, torch.float32, blk, off, deq)
        bad = torch.where(written[..., None], got_deq != full, cache != FILL8)
        msgs += _msgs(describe(f"{what} {name} pages", bad.view(NB, -1), got_deq.view(NB, -1), full.view(NB, -1)))
    return msgs


def probe_rope(case, be, device, info=None):
    """The selector-table probe: bit for bit."""
    info = {} if info is None else info
    qkv, pos, slots, NB, placed = rope_inputs(case)
    info["placed"] = placed
    cs = selector_table(case.D)
    got = run_rope(case, be, device, qkv, pos, slots, NB, cs)
    msgs = check_rope_rows(case.id, got, qkv, pos, slots, NB, cs, case.Hq, case.Hkv, case.D, case.fp8, info)
    return msgs


REAL_CASES = [RopeCase("bf16-real-table", 0, 32, 8, 33, 128, False), RopeCase("fp8-real-table", 1, 32, 8, 33, 128, False)]


def probe_rope_real(case, be, device, info=None):
    """The real rope_table on integer rows through gemm_probes.check_rope (ROPE_ABS).  The fp8
    writer's q is checked the same way, and its pages and scales against the quantisation of the
    rows the bf16 writer stored (kv_fp8.hip: fp8 rows are the quantisation of exactly those)."""
    info = {} if info is None else info
    gen = _gen(case.id, "cpu")
    T, Hq, Hkv = case.T, case.Hq, case.Hkv
    pos, slots, NB = rope_meta(T, gen)
    x = resid((T, (Hq + 2 * Hkv) * 128), gen)
    cs = cos_sin("cpu")
    bcase = case._replace(fp8=0)
    q, kc, vc, _, _ = run_rope(bcase, be, device, x, pos, slots, NB, cs)
    msgs = check_rope(case.id, q, kc, vc, [x.double()], pos, slots, cs, Hq, Hkv, True)
    info["checked"] = q.numel() + 2 * kc.numel()
    if not case.fp8:
        return msgs
    q8, kc8, vc8, ks, vs = run_rope(case, be, device, x, pos, slots, NB, cs)
    msgs += _msgs(describe(case.id + " q against the bf16 writer's", q8 != q, q8, q))
    live = slots >= 0
    blk, off = (slots[live] // BS).long(), (slots[live] % BS).long()
    for name, c8, sc, cb in (("K", kc8, ks, kc), ("V", vc8, vs, vc)):
        deq, byte = fp8_expect(cb[blk, :, off])
        got = c8.view(FP8).float() * (sc.to(torch.int32) << 23).view(torch.float32)[..., None]
        msgs += _msgs(describe(f"{case.id} {name} scale bytes", sc[blk, :, off] != byte, sc[blk, :, off], byte),
                      describe(f"{case.id} {name} pages", got[blk, :, off] != deq, got[blk, :, off], deq))
        written = torch.zeros(sc.shape, dtype=torch.bool)
        written[blk, :, off] = True
        if bool((sc[~written] != FILL8).any()) or bool((c8[~written] != FILL8).any()):
            msgs.append(f"{case.id} {name}: an unwritten slot lost its prefill")
    return msgs


def probe_rope_empty(be, device, fp8):
    case = RopeCase("empty", fp8, 8, 1, 0, 128, False)
    qkv = torch.zeros(0, 10 * 128, dtype=bf)
    z = torch.zeros(0, dtype=torch.int32)
    q, kc, vc, ks, vs = run_rope(case, be, device, qkv, z, z, 8, selector_table(128))
    fill = FILL8 if fp8 else CACHE_FILL
    ok = bool((kc == fill).all()) and bool((vc == fill).all()) and (not fp8 or bool((ks == FILL8).all() and (vs == FILL8).all()))
    return [] if ok else ["0-token rope_cache wrote into a cache"]
