"""Token sampling (K10): greedy, temperature, top-k, top-p, repetition / presence / frequency
penalties and per-token log-probabilities.

GPU path: the fused HIP kernel ``torch.ops.mlop.sample`` (per-row top-k select
+ softmax + top-p + inverse-CDF draw, no full-vocab sort).  Greedy batches use
the HIP argmax directly on the LM head's bf16 logits (no fp32 copy).  CPU path: the same semantics in plain torch (oracle for tests).

Penalties read a device-resident count table (one row per penalised request: bit 31 = the id is
in the prompt, bits 0..30 = its count in the output so far), updated on the device right after
every draw, so a draw launched one step ahead of the host still sees the previous token
(``torch.ops.mlop.apply_penalties`` / ``penalty_update`` / ``penalty_reset``).  Log-probabilities
are the log-softmax of the logits as the model emitted them (before penalties, temperature and
truncation), by ``torch.ops.mlop.token_logprobs`` straight from the bf16 rows.

Guided decoding (runtime/guided.py) is the same pattern with another table: a per-row automaton
state on the device, ``grammar_mask`` before the draw and ``grammar_advance`` behind it.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from .. import ops

I32_MAX = 2**31 - 1
# stop ids per request: bounded so every backend (single GPU, TP, the EP group's fixed control
# slot, ep_serving.py) accepts and rejects the same requests
MAX_STOP_IDS = 256
MAX_LOGPROBS = 20  # top-N alternatives per token (sampling_ext.hip kLpMax)
POOLING_MODES = ("last", "mean")  # SamplingParams.embed (pool.hip)


@dataclass
class SamplingParams:
    max_tokens: int = 128
    temperature: float = 0.0
    top_k: int = 0          # 0 = disabled
    top_p: float = 1.0
    ignore_eos: bool = False
    stop_token_ids: list = field(default_factory=list)
    seed: int | None = None
    repetition_penalty: float = 1.0   # HF semantics: seen logits / r if > 0 else * r
    presence_penalty: float = 0.0     # subtracted once from every id generated so far
    frequency_penalty: float = 0.0    # subtracted per occurrence in the output so far
    logprobs: int | None = None       # None: off; N: the token's logprob + the top N alternatives
    adapter: str | None = None        # name of a loaded LoRA adapter (Engine.load_adapter); None: the base model
    # guided decoding (runtime/guided.py): exactly one of {"choice": [str, ...]}, {"regex": str},
    # {"json_schema": dict | str}; the output then fully matches it (engines with grammar_states > 0)
    guided: dict | None = None
    # embedding request (engines with embed_slots > 0): no token is generated; the prompt's final-normed
    # hidden states are pooled ("last": the last token's, "mean": over every token), cut to the first
    # ``embed_dim`` components (None: all) and, under ``embed_normalize``, scaled to unit L2 norm
    embed: str | None = None
    embed_normalize: bool = True
    embed_dim: int | None = None

    @property
    def greedy(self) -> bool:
        return self.temperature <= 0.0

    @property
    def penalised(self) -> bool:
        return self.repetition_penalty != 1.0 or self.presence_penalty != 0.0 or self.frequency_penalty != 0.0

    @property
    def extended(self) -> bool:
        """Needs the sampler's extended path (count-table slot, log-probabilities and / or a
        grammar state)."""
        return self.logprobs is not None or self.penalised or self.guided is not None

    def validate(self) -> "SamplingParams":
        """Raise ValueError for parameters no sampler can honour (a bad request fails alone)."""
        import math

        # every integer must survive the int32 / int64 tensors the sampler and the EP request
        # broadcast build from it: an unbounded value would raise inside the engine step and
        # take the whole serving loop down instead of this one request
        if not isinstance(self.max_tokens, int) or not 1 <= self.max_tokens <= I32_MAX:
            raise ValueError(f"max_tokens must be an int in [1, {I32_MAX}], got {self.max_tokens}")
        if not math.isfinite(float(self.temperature)) or self.temperature < 0:
            raise ValueError(f"temperature must be finite and >= 0, got {self.temperature}")
        if not isinstance(self.top_k, int) or self.top_k < 0:
            raise ValueError(f"top_k must be an int >= 0, got {self.top_k}")
        if self.top_k > I32_MAX:
            self.top_k = 0  # beyond any vocabulary: the same as no top-k bound (full vocabulary)
        if not (0.0 < float(self.top_p) <= 1.0):
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p}")
        if len(self.stop_token_ids) > MAX_STOP_IDS:
            raise ValueError(f"at most {MAX_STOP_IDS} stop_token_ids, got {len(self.stop_token_ids)}")
        if any(not isinstance(t, int) or not 0 <= t <= I32_MAX for t in self.stop_token_ids):
            raise ValueError(f"stop_token_ids must be ints in [0, {I32_MAX}]")
        if self.seed is not None and (not isinstance(self.seed, int) or not 0 <= self.seed < 2**63):
            raise ValueError("seed must be an int in [0, 2**63)")
        r = self.repetition_penalty
        if isinstance(r, bool) or not isinstance(r, (int, float)) or not math.isfinite(r) or r <= 0:
            raise ValueError(f"repetition_penalty must be finite and > 0, got {r}")
        for name in ("presence_penalty", "frequency_penalty"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not -2.0 <= v <= 2.0:
                raise ValueError(f"{name} must be finite and in [-2, 2], got {v}")
        n = self.logprobs
        if n is not None and (isinstance(n, bool) or not isinstance(n, int) or not 0 <= n <= MAX_LOGPROBS):
            raise ValueError(f"logprobs must be None or an int in [0, {MAX_LOGPROBS}], got {n}")
        if self.adapter is not None and (not isinstance(self.adapter, str) or not self.adapter):
            raise ValueError(f"adapter must be None or a non-empty string, got {self.adapter!r}")
        if self.guided is not None:
            from .guided import check_spec

            check_spec(self.guided)  # the shape only: Engine.check_request compiles it
        if self.embed is None:
            if self.embed_dim is not None or self.embed_normalize is not True:
                raise ValueError("embed_dim / embed_normalize need embed (a pooling mode)")
            return self
        if self.embed not in POOLING_MODES:
            raise ValueError(f"unknown pooling {self.embed!r} (supported: {', '.join(POOLING_MODES)}; CLS and other "
                             "pooling modes of bidirectional encoders are not served)")
        if not isinstance(self.embed_normalize, bool):
            raise ValueError(f"embed_normalize must be a bool, got {self.embed_normalize!r}")
        d = self.embed_dim
        if d is not None and (isinstance(d, bool) or not isinstance(d, int) or not 1 <= d <= I32_MAX):
            raise ValueError(f"embed_dim must be None or an int >= 1, got {d!r}")
        for bad, what in ((self.guided is not None, "guided"), (self.logprobs is not None, "logprobs"),
                          (self.penalised, "a penalty"), (self.adapter is not None, "adapter")):
            if bad:
                raise ValueError(f"an embedding request cannot carry {what}: it generates no token")
        return self


MAX_TOP_K = 1024  # candidates of the top-k kernel; top_k = 0 or > MAX_TOP_K draws from the whole vocabulary


def seeded_uniform(seed: int, index: int) -> float:
    """The uniform of draw ``index`` (the token's position in the request's output) of a request
    with ``SamplingParams.seed``: a splitmix64 hash of (seed, index), 24 bits, exact in fp32.
    Independent of the batch the request rides in, of preemption and of other requests."""
    z = (int(seed) * 0x9E3779B97F4A7C15 + (int(index) + 1) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    z ^= z >> 31
    return (z >> 40) / float(1 << 24)


def _sample_full_row(l: torch.Tensor, T: float, k: int, p: float, u: float) -> int:
    """One row without a candidate bound (top_k = 0 or > MAX_TOP_K), fp64: members = the top-k
    by value (ties at the k-th value all kept) or the whole vocabulary; nucleus = the smallest
    prefix of the members sorted by value (equal logits by lower id) whose softmax mass reaches
    p of the members' mass; the draw = inverse CDF over the nucleus in vocabulary order.  Every
    T > 0 is a sampling row: as T -> 0+ the weights become the indicator of the row maximum and
    the draw is uniform over the tied maxima."""
    V = l.numel()
    l = l.double()
    member = torch.ones(V, dtype=torch.bool)
    if 0 < k < V or p < 1.0:
        order = torch.sort(-l, stable=True).indices  # descending value, equal logits by lower id
    if 0 < k < V:
        member = l >= l[order[k - 1]]
    w = torch.exp((l - l.max()) / T) * member
    nucleus = member
    if p < 1.0:
        cum = torch.cumsum(w[order], 0)
        keep = min(int((cum < p * float(cum[-1])).sum()) + 1, int(member.sum()))
        nucleus = torch.zeros(V, dtype=torch.bool)
        nucleus[order[:keep]] = True
    c = torch.cumsum(w * nucleus, 0)
    return int(min(int((c <= u * float(c[-1])).sum()), V - 1))


def sample_reference(logits: torch.Tensor, temps: torch.Tensor, top_k: torch.Tensor,
                     top_p: torch.Tensor, uniform: torch.Tensor) -> torch.Tensor:
    """Plain-torch sampler, fp64: the contract the kernels of sampling.hip are held to.

    temps/top_k/top_p/uniform: [n].  Equal logits are ordered by LOWER ID, everywhere: the
    order below is a stable descending sort of the row.  Rows with temp <= 0 are greedy (the
    first of that order).  Every temp > 0 is a sampling row, however small: as T -> 0+ the
    weights exp((l - max) / T) become the indicator of the maximum and the draw is uniform over
    the tied maxima among the candidates.  0 < top_k <= MAX_TOP_K: candidates = the first
    min(top_k, V) of the order (exactly that many: ties at the k-th value go to the lower
    ids); top-p keeps the smallest prefix of them whose mass reaches p of the candidates' mass;
    the token is the first candidate of that prefix, in the same order, whose cumulative mass
    exceeds u times the prefix's.  top_k = 0 (or larger than MAX_TOP_K): the softmax over the
    WHOLE vocabulary, ties at the k-th value all kept (``_sample_full_row``)."""
    n, V = logits.shape
    out = torch.empty(n, dtype=torch.int64, device=logits.device)
    kmax = min(MAX_TOP_K, V)
    lf = logits.float().cpu()
    for i in range(n):
        T, k = float(temps[i]), int(top_k[i])
        if T > 0.0 and (k <= 0 or k > MAX_TOP_K):
            out[i] = _sample_full_row(lf[i], T, k, float(top_p[i]), float(uniform[i]))
            continue
        if T <= 0.0:
            out[i] = lf[i].argmax()  # the first of the maxima
            continue
        order = torch.sort(-lf[i], stable=True).indices  # descending value, equal logits by lower id
        k = min(k, kmax)
        v = lf[i][order[:k]].double()
        c = torch.cumsum(torch.exp((v - v[0]) / T), dim=-1)
        pp = float(top_p[i])
        keep = k
        if pp < 1.0:
            keep = min(int((c < pp * float(c[-1])).sum()) + 1, k)
        j = int((c[:keep] <= float(uniform[i]) * float(c[keep - 1])).sum())
        out[i] = order[min(j, keep - 1)]
    return out


def penalties_reference(logits: torch.Tensor, table: torch.Tensor, slots, rep, freq, pres) -> torch.Tensor:
    """Plain-torch ``apply_penalties`` (sampling_ext.hip), in place on fp32 ``logits`` [n, V].
    Row i with slots[i] >= 0 reads table row slots[i] (bit 31 = in the prompt, bits 0..30 = count
    c in the output); on every seen id (word != 0), in this order: l = l / r if l > 0 else l * r
    (r != 1); l -= f * c; l -= p if c > 0."""
    assert logits.dtype == torch.float32
    V = logits.shape[1]
    for i, s in enumerate(torch.as_tensor(slots).tolist()):
        if s < 0:
            continue
        w = table[s, :V]
        seen = w != 0
        c = (w & 0x7FFFFFFF).to(torch.float32)
        r = torch.tensor(float(rep[i]), dtype=torch.float32)
        f = torch.tensor(float(freq[i]), dtype=torch.float32)
        p = torch.tensor(float(pres[i]), dtype=torch.float32)
        l = logits[i]
        if float(r) != 1.0:
            l = torch.where(seen, torch.where(l > 0, l / r, l * r), l)
        l = torch.where(seen, l - f * c, l)
        l = torch.where(c > 0, l - p, l)
        logits[i] = l
    return logits


def logprobs_reference(out_lp: torch.Tensor, out_id: torch.Tensor, logits: torch.Tensor, chosen, want) -> None:
    """Plain-torch ``token_logprobs``: row i with want[i] = N >= 0 gets the fp32 log-softmax of
    its (unpenalised) logits at chosen[i] in column 0 and the N largest entries in columns
    1..N, value descending, ties by lower id (a stable sort)."""
    for i, n in enumerate(torch.as_tensor(want).tolist()):
        if n < 0:
            continue
        lp = torch.log_softmax(logits[i].float(), dim=-1)
        c = int(chosen[i])
        out_lp[i, 0], out_id[i, 0] = lp[c], c
        n = min(n, out_lp.shape[1] - 1, lp.numel())
        if n:
            order = torch.sort(-logits[i].float(), stable=True).indices[:n]
            out_lp[i, 1:1 + n] = lp[order]
            out_id[i, 1:1 + n] = order.to(out_id.dtype)


class SamplerExt:
    """What the extended path needs besides the rows' SamplingParams: the count table and, per
    row of the logits, the table slot (-1: no penalty), the three penalties and the number of
    top log-probabilities wanted (-1: none).  Guided rows: the grammar arena, per row of the
    logits the first arena row of its grammar (``gbase``, -1: not guided) and its engine row
    (``rows``), and the per-engine-row automaton state on the device (``gstate``)."""

    __slots__ = ("table", "slots", "rep", "freq", "pres", "want", "vocab", "arena", "gbase", "rows", "gstate")

    def __init__(self, table, slots, rep, freq, pres, want, vocab=None, arena=None, gbase=None, rows=None,
                 gstate=None):
        self.table, self.vocab = table, vocab
        self.arena, self.gstate = arena, gstate
        self.gbase = None if gbase is None else np.ascontiguousarray(gbase, dtype=np.int32)
        self.rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int32)
        self.slots = np.ascontiguousarray(slots, dtype=np.int32)
        self.rep = np.ascontiguousarray(rep, dtype=np.float32)
        self.freq = np.ascontiguousarray(freq, dtype=np.float32)
        self.pres = np.ascontiguousarray(pres, dtype=np.float32)
        self.want = np.ascontiguousarray(want, dtype=np.int32)


class Sampler:
    def __init__(self, device, seed: int = 0):
        self.device = torch.device(device)
        self.gen = torch.Generator(device=self.device)
        self.gen.manual_seed(seed)

    def sample_ext(self, logits: torch.Tensor, params, ext: SamplerExt, gen_index=None):
        """Draw with penalties and / or log-probabilities: (tokens int64 [n], lp f32 [n, 1 + N] or
        None, ids int32 [n, 1 + N] or None), N = the largest ``want`` of the batch.  fp32 copy ->
        ``apply_penalties`` -> ``grammar_mask`` -> the plain draw on those rows -> ``grammar_advance``
        -> ``penalty_update`` -> ``token_logprobs`` on the ORIGINAL logits.  Rows without a slot or a
        grammar draw from untouched rows, so they get the tokens the plain path gives them."""
        n = logits.shape[0]
        dev = logits.device

        def put(a):
            return torch.from_numpy(a).to(dev, non_blocking=True)

        penalised = bool((ext.slots >= 0).any())
        guided = ext.gbase is not None and bool((ext.gbase >= 0).any())
        if penalised or guided:
            work = logits.float()
            if work.data_ptr() == logits.data_ptr():
                work = work.clone()  # never the caller's tensor
            if penalised:
                slots_d = put(ext.slots)
                ops.apply_penalties(work, ext.table, slots_d, put(ext.rep), put(ext.freq), put(ext.pres))
            if guided:
                gbase_d, rows_d = put(ext.gbase), put(ext.rows)
                ops.grammar_mask(work, ext.arena, gbase_d, rows_d, ext.gstate)
            toks = self(work, params, gen_index)
            if guided:
                ops.grammar_advance(ext.arena, gbase_d, rows_d, ext.gstate, toks, ext.vocab)
            if penalised:
                ops.penalty_update(ext.table, slots_d, toks, ext.vocab)
        else:
            toks = self(logits, params, gen_index)
        nmax = int(ext.want.max()) if n else -1
        if nmax < 0:
            return toks, None, None
        lp = torch.zeros(n, 1 + nmax, dtype=torch.float32, device=dev)
        ids = torch.zeros(n, 1 + nmax, dtype=torch.int32, device=dev)
        ops.token_logprobs(lp, ids, logits, toks, put(ext.want))
        return toks, lp, ids

    def __call__(self, logits: torch.Tensor, params: list[SamplingParams], gen_index=None) -> torch.Tensor:
        """``gen_index``: per row, the position of this draw in its request's output (array, or a
        callable returning one; only consulted when a row has ``SamplingParams.seed``)."""
        n = logits.shape[0]
        if getattr(params, "all_greedy", False) or all(p.greedy for p in params[:n]):
            return ops.argmax(logits) if logits.is_cuda else logits.argmax(-1)
        dev = logits.device
        logits = logits.float()  # the top-k / top-p kernel works on fp32 rows
        rows = params[:n]
        temps = torch.tensor([p.temperature for p in rows], dtype=torch.float32)
        ks = torch.tensor([p.top_k for p in rows], dtype=torch.int32)
        ps = torch.tensor([p.top_p for p in rows], dtype=torch.float32)
        u = torch.rand(n, generator=self.gen, device=self.device, dtype=torch.float32)
        seeded = [i for i, p in enumerate(rows) if p.seed is not None and not p.greedy]
        if seeded:
            gi = gen_index() if callable(gen_index) else gen_index
            us = [seeded_uniform(rows[i].seed, int(gi[i]) if gi is not None else 0) for i in seeded]
            u[torch.tensor(seeded, device=self.device)] = torch.tensor(us, dtype=torch.float32).to(self.device)
        if logits.is_cuda:
            full = bool((((ks <= 0) | (ks > MAX_TOP_K)) & (temps > 0)).any())
            return ops.sample(logits, temps.to(dev, non_blocking=True), ks.to(dev, non_blocking=True),
                              ps.to(dev, non_blocking=True), u, full=full)
        return sample_reference(logits, temps, ks, ps, u)
