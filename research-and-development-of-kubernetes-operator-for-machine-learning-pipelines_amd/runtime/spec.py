"""Speculative decoding by prompt lookup: the contract, in plain Python / NumPy.

A verify step feeds a row its last sampled token plus ``nd <= k`` draft tokens and gets
``nd + 1`` logits rows.  Row j is sampled with the row's own SamplingParams at output
position ``gen + j``; ``a`` = the number of leading drafts the sampler reproduced; the step
emits ``sampled[0..a]`` (always at least one token).  Row j + 1's logits were computed on the
right prefix exactly when drafts 0..j were accepted, so every emitted token is the one the
sampler would have drawn without speculation: greedy, seeded and unseeded rows alike, and no
rejection-sampling arithmetic anywhere.

The proposer looks the sequence's last n tokens up in its own history (prompt + output) and
proposes what followed them there.  ``ops/csrc/spec.hip`` (``torch.ops.mlop.spec_accept`` /
``spec_propose``) is held to these two functions token for token; they are also the CPU path.
"""
from __future__ import annotations

import numpy as np

MAX_SPEC_TOKENS = 7   # k: a row's 1 + k tokens stay within 8 query tokens
MAX_NGRAM = 8


def accept_reference(sampled, drafts, nd: int) -> list:
    """``sampled``: the nd + 1 tokens drawn on the verify rows; ``drafts``: the nd proposed
    tokens.  Returns the emitted tokens ``sampled[0..a]``, a = leading j < nd with
    sampled[j] == drafts[j]."""
    a = 0
    while a < nd and int(sampled[a]) == int(drafts[a]):
        a += 1
    return [int(t) for t in sampled[:a + 1]]


def propose_reference(hist, cap: int, n_max: int, n_min: int) -> list:
    """Up to ``cap`` draft tokens for the history ``hist`` (its first L tokens are passed).

    For n = n_max down to n_min (skipped while L < n + 1): the suffix is hist[L-n:L]; the
    candidates are the starts p in [0, L-n-1] with hist[p:p+n] == suffix (the suffix itself is
    excluded, so a token follows every match).  The largest p with p + n + cap <= L wins (the
    most recent match that can supply ``cap`` followers), else the smallest candidate (the one
    with the most followers); the drafts are hist[p+n : min(p+n+cap, L)].  The first n with a
    candidate decides; none, or cap == 0: the empty list."""
    hist = [int(t) for t in hist]
    L = len(hist)
    if cap <= 0:
        return []
    for n in range(n_max, n_min - 1, -1):
        if L < n + 1:
            continue
        suffix = hist[L - n:]
        cands = [p for p in range(L - n) if hist[p:p + n] == suffix]
        if not cands:
            continue
        full = [p for p in cands if p + n + cap <= L]
        p = max(full) if full else min(cands)
        return hist[p + n:min(p + n + cap, L)]
    return []


def out_width(k: int) -> int:
    """Columns of the per-row result of spec_accept / spec_propose: [emitted count, next draft
    count, k + 1 emitted tokens, k next drafts]."""
    return 2 + (k + 1) + k


def spec_accept_cpu(sampled, q_start, drafts, nd, rows, hist, hist_len, out) -> None:
    """``ops.spec_accept`` on NumPy views (the CPU engine): per row i, accept, append the emitted
    tokens to hist[rows[i]] and write out[i, 0] = a + 1, out[i, 2:2+a+1] = the tokens."""
    cap_len = hist.shape[1]
    for i, r in enumerate(rows.tolist()):
        n, qs = int(nd[i]), int(q_start[i])
        em = accept_reference(sampled[qs:qs + n + 1], drafts[i], n)
        L = int(hist_len[r])
        m = max(0, min(len(em), cap_len - L))
        hist[r, L:L + m] = em[:m]
        hist_len[r] = L + m
        out[i, 0] = len(em)
        out[i, 2:2 + len(em)] = em


def spec_propose_cpu(hist, hist_len, rows, cap, n_max, n_min, out) -> None:
    """``ops.spec_propose`` on NumPy views: out[i, 1] = the draft count, out[i, 2+(k+1):] = the drafts."""
    k = (out.shape[1] - 3) // 2
    for i, r in enumerate(rows.tolist()):
        d = propose_reference(hist[r, :int(hist_len[r])], min(int(cap[i]), k), n_max, n_min)
        out[i, 1] = len(d)
        out[i, 3 + k:3 + k + len(d)] = d


__all__ = ["accept_reference", "propose_reference", "out_width", "MAX_SPEC_TOKENS", "MAX_NGRAM"]
