"""Plain PyTorch (fp32 math) definitions of every HIP op.

They are the numerics oracle of the GPU tests (``tests/test_kernels_gpu.py``)
and the execution path for CPU tensors, so the scheduler / engine / TP logic is
unit-testable in a GPU-less container.  Layouts match the kernels exactly:
``k_cache[NB, Hkv, BS, D]`` and ``v_cache[NB, Hkv, BS, D]`` (both token-major).
"""
from __future__ import annotations

import math

import torch


def rmsnorm(x, w, eps):
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (w.float() * (xf * inv).to(x.dtype).float()).to(x.dtype)


def add_rmsnorm(x, residual, w, eps):
    r = (x.float() + residual.float()).to(x.dtype)
    return rmsnorm(r, w, eps), r


def silu_mul(x):
    I = x.shape[-1] // 2
    g, u = x[..., :I].float(), x[..., I:].float()
    return (torch.nn.functional.silu(g).to(x.dtype).float() * u).to(x.dtype)


def embedding(ids, table, vocab_start=0):
    ids = ids.reshape(-1).long()
    local = ids - vocab_start
    ok = (local >= 0) & (local < table.shape[0])
    out = table[local.clamp(0, table.shape[0] - 1)].clone()
    out[~ok] = 0
    return out


def rotate(x, cos, sin):
    half = x.shape[-1] // 2
    x1, x2 = x[..., :half], x[..., half:]
    return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)


# ------------------------------------------------------------ fp8 KV rows --
# The fp8 KV cache stores K (after RoPE) and V as OCP e4m3fn with one power-of-two scale per
# (token, kv head) row.  The scale is 2^e with the smallest integer e such that
# amax(row) / 2^e <= 448: with amax = m 2^x (frexp, 0.5 <= m < 1), e = x - 9 if m <= 0.875 else
# x - 8, clamped to [-126, 127]; a zero row takes the smallest exponent.  It is stored as the byte
# e + 127, and decoded as the fp32 whose bit pattern is byte << 23: 2^(byte - 127) for byte >= 1
# and 0.0 for byte 0 (the content of a zero-initialised scale tensor), so every byte the kernels
# can meet is finite.  Integer arithmetic throughout: kv_fp8.hip computes the same byte.
FP8 = torch.float8_e4m3fn
FP8_MAX = 448.0
FP8_EXP_MIN, FP8_EXP_MAX = -126, 127


def fp8_row_exponent(amax: torch.Tensor) -> torch.Tensor:
    """int32 scale exponents of rows with maximum magnitudes ``amax`` (>= 0)."""
    m, x = torch.frexp(amax.float())
    e = x - torch.where(m <= 0.875, 9, 8).to(x.dtype)
    e = torch.where(amax == 0, torch.full_like(e, FP8_EXP_MIN), e)
    return e.clamp(FP8_EXP_MIN, FP8_EXP_MAX).to(torch.int32)


def fp8_scale_decode(scale_bytes: torch.Tensor) -> torch.Tensor:
    """uint8 scale bytes -> fp32 scales (bit pattern byte << 23)."""
    return (scale_bytes.to(torch.int32) << 23).view(torch.float32)


def fp8_quantize_rows(x: torch.Tensor):
    """Rows [..., D] -> (e4m3fn [..., D], uint8 scale bytes [...]).  x / 2^e is exact in fp32;
    the one rounding is the conversion to e4m3fn (nearest even)."""
    xf = x.float()
    e = fp8_row_exponent(xf.abs().amax(-1))
    y = torch.ldexp(xf, -e[..., None]).clamp(-FP8_MAX, FP8_MAX)
    return y.to(FP8), (e + 127).to(torch.uint8)


def fp8_dequantize_rows(x8: torch.Tensor, scale_bytes: torch.Tensor) -> torch.Tensor:
    """fp32 rows of an e4m3fn tensor [..., D] and its scale bytes [...] (exact)."""
    return x8.float() * fp8_scale_decode(scale_bytes)[..., None]


def fp8_fake_quant(x: torch.Tensor) -> torch.Tensor:
    """x's rows through the fp8 cache format and back (fp32)."""
    return fp8_dequantize_rows(*fp8_quantize_rows(x))


def head_rmsnorm(x, w, eps):
    """Per-head RMSNorm of fp32 head rows [..., D] with the weight ``w`` [D], no rounding:
    ``x * rsqrt(mean(x^2) + eps) * w`` (the QK-norm of ``rope_cache``)."""
    return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w.float()


def rope_cache(qkv, positions, cos_sin, slots, k_cache, v_cache, n_q_heads, k_scale=None, v_scale=None,
               q_norm=None, k_norm=None, eps=0.0):
    """Rotate q/k, scatter k/v into the paged cache, return q [T, Hq, D].  An e4m3fn cache takes
    the rows (rounded to the model dtype as a bf16 cache would hold them) quantised by
    ``fp8_quantize_rows``, their scale bytes going to ``k_scale`` / ``v_scale`` [NB, Hkv, BS].

    ``q_norm`` / ``k_norm`` (weights [D], both or neither): per-head QK-norm (Qwen3).  Every q head
    and every k head x of the row the GEMM stored becomes ``x * rsqrt(mean(x^2) + eps) * w`` in
    fp32, THEN comes the rotation, and one rounding to the model dtype at the end; V is untouched.
    transformers rounds to the model dtype between the norm and the rotation; fp32 throughout is
    this project's convention for RoPE and the more accurate of the two (one rounding, not two)."""
    if (q_norm is None) != (k_norm is None):
        raise ValueError("QK-norm needs both q_norm and k_norm")
    T = qkv.shape[0]
    Hkv, BS, D = k_cache.shape[1], k_cache.shape[2], k_cache.shape[3]
    half = D // 2
    x = qkv[:, : (n_q_heads + 2 * Hkv) * D].float().view(T, n_q_heads + 2 * Hkv, D)
    cs = cos_sin[positions.long()].float()  # [T, D]
    cos, sin = cs[:, None, :half], cs[:, None, half:]
    xq, xk = x[:, :n_q_heads], x[:, n_q_heads:n_q_heads + Hkv]
    if q_norm is not None:
        xq, xk = head_rmsnorm(xq, q_norm, eps), head_rmsnorm(xk, k_norm, eps)
    q = rotate(xq, cos, sin).to(qkv.dtype)
    k = rotate(xk, cos, sin).to(qkv.dtype)
    v = x[:, n_q_heads + Hkv:].to(qkv.dtype)
    fp8 = k_cache.dtype == FP8
    if fp8:
        assert k_scale is not None and v_scale is not None, "an fp8 KV cache needs its scale tensors"
        (k, ks), (v, vs) = fp8_quantize_rows(k), fp8_quantize_rows(v)
    for t in range(T):
        s = int(slots[t])
        if s < 0:
            continue
        b, o = divmod(s, BS)
        k_cache[b, :, o, :] = k[t]
        v_cache[b, :, o, :] = v[t]
        if fp8:
            k_scale[b, :, o] = ks[t]
            v_scale[b, :, o] = vs[t]
    return q


def gather_kv(k_cache, v_cache, block_table, n, k_scale=None, v_scale=None):
    """Contiguous K, V [n, Hkv, D] of one sequence from its pages (an e4m3fn cache with its scale
    bytes: the dequantised rows, fp32)."""
    BS = k_cache.shape[2]
    pages = [int(p) for p in block_table[: (n + BS - 1) // BS]]
    fp8 = k_cache.dtype == FP8
    if not pages:
        Hkv, D = k_cache.shape[1], k_cache.shape[3]
        z = torch.zeros(0, Hkv, D, dtype=torch.float32 if fp8 else k_cache.dtype, device=k_cache.device)
        return z, z
    if fp8:
        assert k_scale is not None and v_scale is not None, "an fp8 KV cache needs its scale tensors"
        page = lambda c, sc, p: fp8_dequantize_rows(c[p], sc[p])  # noqa: E731
    else:
        page = lambda c, sc, p: c[p]  # noqa: E731
    k = torch.cat([page(k_cache, k_scale, p).permute(1, 0, 2) for p in pages], 0)[:n]  # [n, Hkv, D]
    v = torch.cat([page(v_cache, v_scale, p).permute(1, 0, 2) for p in pages], 0)[:n]  # [n, Hkv, D]
    return k, v


def paged_attention(q, k_cache, v_cache, meta, k_scale=None, v_scale=None):
    """Causal GQA attention of every query token of ``meta`` over its paged context.  With a
    sliding window ``meta.window = W > 0`` the query at position i attends the keys
    i - W < j <= i; pages wholly below the first query's window are not read at all.  An e4m3fn
    cache is read through its scale bytes (``gather_kv``)."""
    W = int(getattr(meta, "window", 0) or 0)
    out = torch.zeros_like(q)
    Hq, D = q.shape[1], q.shape[2]
    Hkv = k_cache.shape[1]
    G = Hq // Hkv
    scale = 1.0 / math.sqrt(D)
    qs, ql, cl = (meta.q_start.cpu().tolist(), meta.q_len.cpu().tolist(), meta.ctx_len.cpu().tolist())
    bt = meta.block_tables.cpu()
    # only rows referenced by this launch's tiles are live (other rows hold stale values)
    live = set(meta.tile_seq.cpu().tolist())
    if getattr(meta, "ptile_seq", None) is not None:
        live |= set(meta.ptile_seq.cpu().tolist())
    for s in sorted(live):
        if ql[s] == 0 or cl[s] == 0:
            continue
        # first page any query of the row can see (everything below may have been released)
        BS = k_cache.shape[2]
        lo = max(0, cl[s] - ql[s] - W + 1) // BS * BS if W > 0 else 0
        k, v = gather_kv(k_cache, v_cache, bt[s][lo // BS:], cl[s] - lo, k_scale, v_scale)
        k = k.float().repeat_interleave(G, dim=1)  # [n, Hq, D]
        v = v.float().repeat_interleave(G, dim=1)
        qq = q[qs[s]:qs[s] + ql[s]].float()      # [ql, Hq, D]
        scores = torch.einsum("qhd,khd->hqk", qq, k) * scale
        pos = torch.arange(cl[s] - ql[s], cl[s], device=q.device)[:, None]
        keys = torch.arange(lo, cl[s], device=q.device)[None, :]
        masked = keys > pos
        if W > 0:
            masked = masked | (keys <= pos - W)
        scores = scores.masked_fill(masked[None], float("-inf"))
        p = torch.softmax(scores, dim=-1)
        out[qs[s]:qs[s] + ql[s]] = torch.einsum("hqk,khd->qhd", p, v).to(q.dtype)
    return out


# ------------------------------------------------------------------ MoE --

def moe_route(logits, top_k):
    """softmax -> top-k -> renormalise.  Ties go to the lower expert index, as in the HIP routes
    (strict > over ascending e): a stable descending sort, where torch.topk promises no order."""
    p = torch.softmax(logits.float(), dim=-1)
    w, idx = torch.sort(p, dim=-1, descending=True, stable=True)
    w, idx = w[..., :top_k], idx[..., :top_k]
    w = w / w.sum(-1, keepdim=True)
    return w, idx.to(torch.int32)


def moe_permute(x, topi, e0, n_local):
    """Rows routed to local experts, grouped by expert (stable in slot order), padded to T*k rows.
    Returns (xp [T*k, H], offsets int32 [n_local+1], src int32 [T*k], inv int32 [T*k])."""
    T, k = topi.shape
    flat = topi.reshape(-1).long() - e0
    ok = (flat >= 0) & (flat < n_local)
    slots = torch.nonzero(ok, as_tuple=True)[0]
    e = flat[slots]
    order = torch.argsort(e, stable=True)
    slots, e = slots[order], e[order]
    n = slots.numel()
    counts = torch.bincount(e, minlength=n_local)
    offsets = torch.zeros(n_local + 1, dtype=torch.int32, device=x.device)
    offsets[1:] = torch.cumsum(counts, 0).to(torch.int32)
    xp = torch.zeros(T * k, x.shape[1], dtype=x.dtype, device=x.device)
    xp[:n] = x[slots // k]
    src = torch.full((T * k,), -1, dtype=torch.int32, device=x.device)
    src[:n] = slots.to(torch.int32)
    inv = torch.full((T * k,), -1, dtype=torch.int32, device=x.device)
    inv[slots] = torch.arange(n, dtype=torch.int32, device=x.device)
    return xp, offsets, src, inv


def grouped_gemm(xp, w, offsets):
    """Per group e: rows [off[e], off[e+1]) of xp times w[e]^T (w: [E, N, K]); other rows 0."""
    out = torch.zeros(xp.shape[0], w.shape[1], dtype=xp.dtype, device=xp.device)
    off = offsets.tolist()
    for e in range(w.shape[0]):
        a, b = off[e], off[e + 1]
        if b > a:
            out[a:b] = (xp[a:b].float() @ w[e].float().t()).to(xp.dtype)
    return out


def moe_combine(y, inv, topw):
    T, k = topw.shape
    out = torch.zeros(T, y.shape[1], dtype=torch.float32, device=y.device)
    inv = inv.long().view(T, k)
    for j in range(k):
        ok = inv[:, j] >= 0
        if ok.any():
            out[ok] += topw[ok, j, None].float() * y[inv[ok, j]].float()
    return out.to(y.dtype)


# ----------------------------------------------------------------- LoRA --

def _lora_slots(tok_slot, S):
    """int64 slots with every entry outside [0, S) turned into -1 (lora.hip lora_lane_slot)."""
    ts = tok_slot.long()
    return torch.where((ts < 0) | (ts >= S), torch.full_like(ts, -1), ts)


def lora_shrink(x, A, tok_slot, slot_rank=None):
    """tmp[t] = A[tok_slot[t]] . x[t] in fp32 ([T, G R]); rows with slot -1, or with a slot outside
    the storage (never an index), are zero."""
    T = x.shape[0]
    tmp = torch.zeros(T, A.shape[1], dtype=torch.float32, device=x.device)
    ts = _lora_slots(tok_slot, A.shape[0])
    for s in torch.unique(ts[ts >= 0]).tolist():
        rows = ts == s
        tmp[rows] = x[rows].float() @ A[s].float().t()
    return tmp


def lora_expand_add(y, tmp, B, tile_group, tok_slot, slot_rank=None):
    """In place: y[t, n] += sum_r tmp[t, g(n) R + r] . B[tok_slot[t], n, r] (fp32 sum, one rounding to
    y's dtype); g(n) = tile_group[n // 16].  Rows with slot -1, or with a slot outside the storage,
    are not written."""
    R = B.shape[2]
    ts = _lora_slots(tok_slot, B.shape[0])
    col_g = tile_group.long().repeat_interleave(16)
    for s in torch.unique(ts[ts >= 0]).tolist():
        rows = torch.nonzero(ts == s, as_tuple=True)[0]
        acc = y[rows].float()
        for g in torch.unique(col_g).tolist():
            cols = torch.nonzero(col_g == g, as_tuple=True)[0]
            acc[:, cols] += tmp[rows, g * R:(g + 1) * R] @ B[s][cols].float().t()
        y[rows] = acc.to(y.dtype)
    return y


# -------------------------------------------------------------- pooling --
# Embedding pooling (csrc/pool.hip).  Segment rows [r0, r1, slot, flags], finish rows
# [slot, count, d, flags]; the flag bits are those of csrc/launch.h.
POOL_INIT, POOL_LAST, POOL_MODE_LAST = 1, 2, 4
POOL_FIN_NORMALIZE, POOL_FIN_MEAN = 1, 2


def pool_reference(x, seg, acc, fin=None):
    """The contract of ``ops.pool_accumulate`` / ``ops.pool_finish``.

    ``x`` [T, H] (bf16), ``seg`` int [nseg, 4], ``acc`` fp32 [S, H], ``fin`` int [nfin, 4] or None.
    Returns (acc', out): acc' = a copy of ``acc`` after the segments, in order.  A ``mean``
    segment: acc'[slot] = (0 if POOL_INIT else acc'[slot]) + x[r0] + ... + x[r1 - 1], one fp32 add
    per row, the rows strictly in order.  A POOL_MODE_LAST segment writes float(x[r1 - 1]) if it
    carries POOL_LAST and nothing otherwise.  out: float64 [S, H], zero but for the finished slots'
    first d columns: v = acc'[slot, :d] / count (POOL_FIN_MEAN only), then v / max(||v||, 1e-12)
    under POOL_FIN_NORMALIZE, all in float64 from the exact fp32 sums."""
    acc = acc.detach().to("cpu", torch.float32).clone()
    xs = x.detach().to("cpu")
    for r0, r1, slot, flags in torch.as_tensor(seg).reshape(-1, 4).tolist():
        if flags & POOL_MODE_LAST:
            if flags & POOL_LAST:
                acc[slot] = xs[r1 - 1].float()
            continue
        a = torch.zeros_like(acc[slot]) if flags & POOL_INIT else acc[slot].clone()
        for r in range(r0, r1):
            a = a + xs[r].float()
        acc[slot] = a
    out = torch.zeros(acc.shape, dtype=torch.float64)
    for slot, count, d, flags in (torch.as_tensor(fin).reshape(-1, 4).tolist() if fin is not None else ()):
        v = acc[slot, :d].double()
        if flags & POOL_FIN_MEAN:
            v = v / count
        if flags & POOL_FIN_NORMALIZE:
            v = v / max(float(v.square().sum().sqrt()), 1e-12)
        out[slot, :d] = v
    return acc, out
