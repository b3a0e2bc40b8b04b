"""Continuous-batching inference engine (G5) with hipGraph-captured decode (G1).

One engine per model replica (DP replica = one engine; a TP replica runs one
engine per rank in lock-step, rank 0 owning the scheduler and broadcasting
step metadata).

Step policy:
  * prefill steps pack up to ``max_num_batched_tokens`` prompt tokens of
    admitted requests (chunked: a long prompt spans several steps);
  * decode steps run every running sequence, one token each, replaying the
    hipGraph captured for the smallest batch bucket >= B (padded rows attend to
    nothing), so a decode step costs one graph launch + one metadata H2D + one
    token D2H;
  * prompt work is scheduled when requests wait and either nothing is decoding,
    enough requests are queued (``prefill_min_batch``) or the oldest has waited
    ``max_decode_gap`` decode steps (bounded TTFT without fragmenting decode);
    while sequences decode it runs as a MIXED step (``mixed_prefill``): every
    running row's decode token plus prompt chunks up to the token budget in one
    eager ragged forward, so decode rides in the prefill's larger-M GEMMs
    instead of stalling behind a separate prefill pass;
  * KV pages come from a free-list; on exhaustion the newest running sequence
    is preempted (pages freed, recomputed later);
  * with ``spec_tokens`` = k > 0 (speculative decoding by prompt lookup, runtime/spec.py) a
    decode-only step of at most ``spec_max_batch`` rows becomes a VERIFY step when a row has
    drafts: each row feeds its last token and up to k drafts, every token is sampled, the leading
    drafts the sampler reproduced are accepted; it replays the verify graph of its bucket.
    Such an engine steps synchronously.
  * with ``grammar_states`` > 0 (guided decoding, runtime/guided.py) a request may carry a regex,
    a list of choices or a JSON schema: its compiled token table lives in a device arena, its
    automaton state in a device vector indexed by engine row; the sampler masks the row's logits
    by the state before the draw and advances the state behind it, so the host never reads it.
  * with ``embed_slots`` > 0 a request may ask for an EMBEDDING (``SamplingParams.embed``): a
    prefill-only sequence.  Its prompt is chunked like any other, in prompt-only and mixed steps;
    behind the forward of every step that carries one of its chunks ops.pool_accumulate pools the
    chunk's hidden states into the sequence's slot of an fp32 accumulator, and behind its last
    chunk ops.pool_finish scales / truncates / normalises the vector.  It gets no logits row, never
    joins the running rows and gives its pages and row back with its last chunk's launch.
"""
from __future__ import annotations

import collections
import itertools
import operator
import os
import sys
import threading
import time
from dataclasses import dataclass, field
from enum import Enum

import numpy as np
import torch

from .. import ops
from .attn_meta import MetaBuffers, plan_partitions
from .kv_cache import (BLOCK_SIZE, KV_DTYPES, BlockAllocator, KVCache, blocks_for_budget, blocks_needed,
                       kv_dtype_bytes, prefix_hashes)
from .sampler import MAX_LOGPROBS, Sampler, SamplerExt, SamplingParams
from .tracing import StepTracer, TorchProfileWindow


KIND_STOP, KIND_EAGER, KIND_GRAPH, KIND_BARRIER = 0, 1, 2, 3


class StepSync:
    """Lock-step execution across a tensor-parallel group.  Rank 0 alone
    schedules.  Per step it sends two things:

      * the step header [kind, T, num_tiles, n_logits, part_tokens, nparts, bucket,
        num_flash_tiles, greedy] HOST to host, over the TP group's gloo (CPU) group: a worker
        learns what step t+1 is while the device still runs step t, so it enqueues step t+1's
        forward (and its graph replay) ahead, exactly as the leader does under one-step-ahead
        scheduling, and no worker ever reads a device tensor back to decide what to run;
      * the step's packed metadata buffer (attn_meta.MetaBuffers: int32 metadata, ids and
        logits index in ONE device buffer, already uploaded by one H2D, decode ids gathered on
        the device from the previous step's tokens) as ONE in-stream device broadcast of its
        used prefix (header word 9: up to the highest block-table row in use): the K15 IPC
        broadcast kernel on GPU (parallel/custom_ar.py: each worker copies the leader's bytes in
        one hop, no host round trip), RCCL / gloo otherwise, ordered after the previous forward
        on every rank's stream.
    STOP / BARRIER steps carry the header only."""

    NHDR = 10

    def __init__(self, group, cpu_group=None):
        import os

        self.g = group
        self.cpu = cpu_group
        self.is_leader = group.rank == 0
        self.hdr = torch.zeros(self.NHDR, dtype=torch.int64)
        # the header's host path: the native shared-memory channel (TP groups live on one node),
        # gloo's broadcast as the fallback (the channel cannot be built on every rank)
        self.chan = None
        if cpu_group is not None:
            from ..parallel.comm import HostChannel

            try:  # collective: every rank gets a channel, or every rank raises and uses gloo
                self.chan = HostChannel(cpu_group, words=self.NHDR)
            except HostChannel.Unavailable as e:
                print(f"[engine] TP step-header channel unavailable ({e}): gloo broadcast", file=sys.stderr)
                self.chan = None

    def _bcast_header(self):
        import torch.distributed as dist

        if self.cpu is None:  # no host group (single process): nothing to agree on
            return
        if self.chan is not None:
            if self.is_leader:
                self.chan.send(self.hdr)
            else:
                self.chan.recv(self.hdr)
            return
        dist.broadcast(self.hdr, src=dist.get_global_rank(self.cpu, 0), group=self.cpu)

    def send(self, eng, kind, T, nt, nl, part, nparts, bucket, npt=0, greedy=0):
        n = eng.meta.extent(eng.rows_hi)
        self.hdr[:] = torch.tensor([kind, T, nt, nl, part, nparts, bucket, npt, greedy, n], dtype=torch.int64)
        self._bcast_header()
        if kind not in (KIND_STOP, KIND_BARRIER):
            self.g.broadcast(eng.meta.dbuf[:n], 0)

    def recv(self, eng):
        self._bcast_header()
        hdr = tuple(self.hdr.tolist())
        if hdr[0] not in (KIND_STOP, KIND_BARRIER):
            self.g.broadcast(eng.meta.dbuf[:hdr[9]], 0)
        return hdr[:9]


class _Tokens:
    """Token ids chosen inside ``_execute`` (TP greedy: no logits were gathered)."""

    __slots__ = ("ids",)

    def __init__(self, ids):
        self.ids = ids

    def __getitem__(self, k):
        return _Tokens(self.ids[k])


class EPSync:
    """Lock-step agreement of a data-parallel-attention / expert-parallel group (config 5, CL4).

    Every rank schedules its OWN requests, but each MoE layer is an all-to-all over the whole
    group, so every rank must run a forward in the same step, with the same MoE capacity, and
    either all replay a decode graph of the same bucket or all run eager.  Once per step every
    rank calls ``agree``: [has_work, wants_eager, tokens, bucket, busy] from every rank over the
    group's shared-memory all-gather (parallel/comm.py ``HostAllGather``: one host hop, no GPU
    sync; gloo when shared memory is unavailable), reduced by MAX on each rank -> what the whole
    group does this step.  A rank with nothing to do joins with a padding-only forward."""

    def __init__(self, group, cpu_group):
        from ..parallel.comm import make_host_allgather

        self.g, self.cpu = group, cpu_group
        self.last_any = 1
        self.last_busy = 1
        self.xg = make_host_allgather(cpu_group, 8)
        self._v = torch.zeros(5, dtype=torch.int64)

    def agree(self, has_work: int, eager: int, tokens: int, bucket: int, busy: int = 1):
        """``busy``: this rank still holds requests (queued, running or in flight) even if it
        launches nothing this step; the group is done only when no rank is busy."""
        v = self._v
        v[0], v[1], v[2], v[3], v[4] = has_work, eager, tokens, bucket, busy
        rows = self.xg.exchange(v)
        any_work, any_eager, t_max, b_max, any_busy = torch.stack(rows).max(dim=0).values.tolist()
        self.last_any, self.last_busy = any_work, any_busy
        return any_work, any_eager, t_max, b_max


class Status(Enum):
    WAITING = 0
    PREFILL = 1
    RUNNING = 2
    FINISHED = 3


@dataclass
class Sequence:
    seq_id: int
    prompt: list
    params: SamplingParams
    output: list = field(default_factory=list)
    blocks: list = field(default_factory=list)
    row: int = -1
    num_cached: int = 0
    status: Status = Status.WAITING
    arrival: float = field(default_factory=time.perf_counter)
    first_token_time: float | None = None
    finish_time: float | None = None
    finish_reason: str | None = None
    hashes: list = field(default_factory=list)  # prefix hashes of this sequence's full pages
    n_reg: int = 0                              # leading pages matched in / registered to the prefix cache
    n_rel: int = 0                              # leading pages released below the sliding window (null page 0)
    pen_slot: int = -1                          # row of the penalty count table held while admitted
    logprobs: list = field(default_factory=list)  # per output token (logprob, [(id, logprob), ...]) when asked for
    slot: int = -1                              # LoRA adapter slot (-1: base model); kept across preemption
    prefix_seed: bytes = b""                    # seed of the prefix hash chain: the adapter's identity
    grammar: object = None                      # guided decoding: the compiled guided.Grammar (pinned)
    g_admitted: bool = False                    # ... and whether the sequence's row holds a reference on its arena range
    emb_slot: int = -1                          # embedding request: its accumulator slot, held until the vector is delivered
    embedding: object = None                    # ... and the vector (np.float32 [d]) once it is

    @property
    def length(self) -> int:
        return len(self.prompt) + len(self.output)

    def token_at(self, i: int) -> int:
        n = len(self.prompt)
        return self.prompt[i] if i < n else self.output[i - n]

    def tokens(self, a: int, b: int):
        n = len(self.prompt)
        if b <= n:
            return self.prompt[a:b]
        if a >= n:
            return self.output[a - n:b - n]
        return list(self.prompt[a:]) + self.output[:b - n]


@dataclass
class EngineConfig:
    max_num_seqs: int = 256
    max_num_batched_tokens: int = 8192
    max_model_len: int = 4096
    num_kv_blocks: int | None = None       # None: size from kv_cache_bytes / free HBM
    kv_cache_bytes: int | None = None
    gpu_memory_utilization: float = 0.90
    kv_fraction: float = 0.5  # pages for this share of max_num_seqs x max_model_len (mean context;
                              # preemption covers the tail) - same policy as controller/placement.py
    use_graphs: bool = True
    graph_buckets: tuple = (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024)
    prefill_min_batch: int = 1
    max_decode_gap: int = 0
    mixed_prefill: bool = True    # prefill chunks ride in the decode step (one forward)
    mixed_min_chunk: int = 64     # below this many free token slots, decode alone
    seed: int = 0
    enable_prefix_caching: bool = True  # share computed prompt pages between requests (same prefix)
    # one-step-ahead scheduling (TP = EP = 1, mixed prefill): step t+1 is built and launched
    # while step t still runs on the device; step t's tokens are read back afterwards
    async_scheduling: bool = True
    # rows of the penalty count table (int32 [penalty_slots, vocab], allocated on the first
    # penalised request): penalised requests admitted at once; further ones wait for a slot
    penalty_slots: int = 64
    # sliding-window models: give back the KV pages that fell wholly below a sequence's window
    # (False: keep them until the sequence ends; the A/B and debugging switch)
    swa_release: bool = True
    # multi-LoRA: adapter slots held in HBM beside the base model (0 = feature off: nothing is
    # allocated or captured) and the largest adapter rank a slot takes (<= 64)
    max_adapters: int = 0
    max_lora_rank: int = 64
    # element type of the paged KV cache: "bf16" (the model's dtype), or "fp8" = OCP e4m3fn pages
    # with one power-of-two scale byte per (token, kv head) row (ops/reference.py "fp8 KV rows"):
    # 2 D / (D + 1) = 1.98x the pages per byte.  fp8 has no sliding-window, flash-prefill, MoE or
    # fused-epilogue kernels: those models are rejected, prompt chunks run on the 16-row tiles.
    kv_cache_dtype: str = "bf16"
    # speculative decoding by prompt lookup (runtime/spec.py): up to ``spec_tokens`` (k <= 7) draft
    # tokens per row, found by matching the sequence's last ``spec_ngram_max`` .. ``spec_ngram_min``
    # tokens in its own history, are verified in one pass with the row's decode token; outputs are
    # exactly those of k = 0.  0 = off: nothing is allocated, captured or routed differently.  Such
    # an engine runs synchronous steps (the host needs the accept counts to place the next step).
    # Decode steps of more than ``spec_max_batch`` rows run unspeculated: 16 is the largest batch
    # measured, where 60 % accepted drafts still give 1.4-2.3x (profiles/spec_decode.md)
    spec_tokens: int = 0
    spec_ngram_max: int = 3
    spec_ngram_min: int = 1
    spec_max_batch: int = 16
    # guided decoding (runtime/guided.py): rows of the device arena of compiled grammars (int16
    # [grammar_states, vocab rounded up to 8]; a grammar takes one row per automaton state) and the
    # number of compiled grammars the host keeps.  0 = off: nothing is allocated and a guided
    # request is refused.  Not with tensor or expert parallelism.
    grammar_states: int = 0
    grammar_cache: int = 16
    # embedding requests (SamplingParams.embed): slots of the fp32 pooling accumulator ([embed_slots,
    # hidden] plus an output buffer and its pinned mirror) = embedding sequences admitted at once;
    # further ones wait for a slot.  0 = off: nothing is allocated and such a request is refused.
    # Not with tensor or expert parallelism, speculation, LoRA slots or MoE models.
    embed_slots: int = 0


@dataclass
class StepOutput:
    seq_id: int
    token: int
    finished: bool
    finish_reason: str | None = None
    logprob: float | None = None        # SamplingParams.logprobs: the token's log-probability
    top_logprobs: list | None = None    # ... and the top-N [(id, logprob), ...]
    embedding: np.ndarray | None = None  # an embedding request's vector (fp32 [d]): token -1, reason "embedding"


class _ParamsList(list):
    pass


class _AllGreedy:
    """Stands in for a list of greedy SamplingParams of any length."""

    all_greedy = True

    def __getitem__(self, k):
        return self


_ALL_GREEDY = _AllGreedy()


class _Step:
    """One step as ``Engine._build_step`` planned it and ``Engine._issue`` launches it.  The decode
    part: engine ``rows`` (int32 [B]) and their context lengths ``ctx_d``.  The prompt part (all
    empty in a decode step): the sequences of ``batch`` with their ``chunks`` (tokens this step),
    ``p_ctx`` (cached length after it), ``done`` (the prompt completes) and ``done_seqs``.  The
    logits rows are the decode rows, then ``done_seqs``: engine rows ``srows``, sequences ``seqs``.

    A speculative verify step (``nd`` not None) feeds decode row i its last token and ``nd[i]`` of
    ``drafts[i]``: its ``nlog`` logits rows are the rows' tokens in order, row i's from ``q0[i]``,
    ``srows`` the engine row and ``goff`` the offset inside its row of each.

    Embedding sequences of ``batch``: ``emb_done`` (its prompt completes; such a sequence is never in
    ``done`` / ``done_seqs``) and, once ``_chunks_done`` ran, ``emb_out``: the (sequence, slot, d) whose
    vectors this step finishes."""

    __slots__ = ("rows", "ctx_d", "B", "batch", "chunks", "p_ctx", "done", "done_seqs", "srows", "seqs",
                 "T", "launch", "params", "greedy", "nd", "drafts", "q0", "goff", "nlog", "emb_done", "emb_out")


class _Pending:
    """The in-flight step of one-step-ahead scheduling: its logits ``rows`` with their ``epochs``
    and ``seqs`` at launch, the sampled tokens on the device (``toks_d``: the next step's decode
    ids) and on their way to the pinned ``toks_h`` behind ``ev``, log-probabilities likewise
    (``lp``: pinned values, pinned ids, the rows' wanted counts; or None) and ``retire``, the ids
    of the sequences whose pending token is their last."""

    __slots__ = ("rows", "epochs", "seqs", "toks_d", "toks_h", "ev", "lp", "retire", "emb")

    def __init__(self, rows, epochs, seqs, toks_d, toks_h, ev, lp, emb=()):
        self.rows, self.epochs, self.seqs, self.toks_d, self.toks_h = rows, epochs, seqs, toks_d, toks_h
        self.ev, self.lp, self.retire = ev, lp, set()
        self.emb = emb  # (sequence, slot, d) of the embeddings the step finishes (pinned mirror, behind ev)


class StepBatch:
    """One step's outputs as arrays (no per-token Python objects on the hot path);
    iterating yields ``StepOutput`` lazily."""

    __slots__ = ("seq_ids", "tokens", "fin", "reasons", "lps", "embs")

    def __init__(self, seq_ids, tokens, fin, reasons: dict, lps: dict | None = None, embs: dict | None = None):
        self.seq_ids, self.tokens, self.fin, self.reasons = seq_ids, tokens, fin, reasons
        self.embs = embs or None  # seq_id -> vector of the embedding requests that finished
        # seq_id -> (logprob, [(id, logprob), ...]) of the rows that asked for log-probabilities
        # (a sequence has at most one token per step); None when no row did
        self.lps = lps or None

    @classmethod
    def from_list(cls, outs: list):
        return cls(np.array([o.seq_id for o in outs], dtype=np.int64),
                   np.array([o.token for o in outs], dtype=np.int64),
                   np.array([o.finished for o in outs], dtype=bool),
                   {o.seq_id: o.finish_reason for o in outs if o.finished},
                   {o.seq_id: (o.logprob, o.top_logprobs) for o in outs if o.logprob is not None},
                   {o.seq_id: o.embedding for o in outs if o.embedding is not None})

    @classmethod
    def concat(cls, a: "StepBatch", b: "StepBatch"):
        reasons = dict(a.reasons)
        reasons.update(b.reasons)
        lps = None
        if a.lps or b.lps:
            lps = dict(a.lps or {})
            lps.update(b.lps or {})
        embs = {**(a.embs or {}), **(b.embs or {})}
        return cls(np.concatenate([a.seq_ids, b.seq_ids]), np.concatenate([a.tokens, b.tokens]),
                   np.concatenate([a.fin, b.fin]), reasons, lps, embs)

    def __len__(self):
        return len(self.seq_ids)

    def _out(self, sid, tok, f):
        lp = self.lps.get(sid) if self.lps else None
        return StepOutput(sid, tok, f, self.reasons.get(sid) if f else None, *(lp or (None, None)),
                          self.embs.get(sid) if self.embs else None)

    def __iter__(self):
        for sid, tok, f in zip(self.seq_ids.tolist(), self.tokens.tolist(), self.fin.tolist()):
            yield self._out(sid, tok, f)

    @property
    def finished(self) -> list:
        return [self._out(int(self.seq_ids[i]), int(self.tokens[i]), True) for i in np.nonzero(self.fin)[0]]


class Engine:
    def __init__(self, model, cfg: EngineConfig | None = None):
        self.model = model
        self.checkpoint_dir = None  # set by deploy.build_engine when the weights came from a checkpoint
        self.cfg = cfg = cfg or EngineConfig()
        self.device = model.device
        mc = model.cfg
        self.max_model_len = min(cfg.max_model_len, mc.max_position)
        self._kv_bytes = kv_dtype_bytes(cfg.kv_cache_dtype)  # ValueError for an unknown name
        self.fp8_kv = cfg.kv_cache_dtype == "fp8"
        if self.fp8_kv:
            if int(getattr(mc, "sliding_window", 0) or 0) > 0:
                raise ValueError('kv_cache_dtype="fp8" does not support sliding-window models '
                                 f"(sliding_window = {mc.sliding_window}): no windowed fp8 attention kernel")
            if getattr(mc, "is_moe", False) or model.ps.ep.size > 1:
                raise ValueError('kv_cache_dtype="fp8" is not supported for MoE models / expert parallelism')
            if mc.head_dim != 128:
                raise ValueError('kv_cache_dtype="fp8" needs head_dim 128')
        self.spec_k = int(cfg.spec_tokens or 0)
        # optional callable (seq, cap) -> list[int]: replaces the device n-gram proposals (the
        # extension point of a draft-model proposer; lets tests force any acceptance pattern)
        self.spec_proposer = None
        if self.spec_k:
            self._check_spec(cfg, mc, model)
        # multi-LoRA: the slot-major adapter stacks, allocated before the KV pool is sized from
        # what is left (raises for Mixtral / TP > 1 / EP)
        self.lora = None
        self._adapters: dict[str, dict] = {}
        if cfg.max_adapters > 0:
            from ..models.lora import LoraStacks

            self.lora = LoraStacks(model, cfg.max_adapters, cfg.max_lora_rank)
        self._free_slots = list(range(max(0, cfg.max_adapters) - 1, -1, -1))
        self._slot_refs = np.zeros(max(0, cfg.max_adapters), np.int64)  # live sequences per slot
        self.graphs_lora: dict[int, tuple] = {}
        self._step_lora = False  # the step being launched has at least one adapter row
        # guided decoding: the grammar arena and the per-row automaton state, allocated before
        # the KV pool is sized from what is left
        self.stats = collections.Counter()
        self._guided_init(cfg, model)
        # embedding requests: the pooling accumulator, likewise ahead of the KV pool
        self._embed_init(cfg, model)
        nb = cfg.num_kv_blocks or self._auto_blocks()
        tp = model.ps.tp
        self.step_sync = StepSync(tp, model.ps.tp_cpu) if tp.size > 1 else None
        ep = model.ps.ep
        self.ep_sync = EPSync(ep, model.ps.ep_cpu) if (tp.size == 1 and ep.size > 1) else None
        if tp.size > 1:  # every rank must address the same page ids: agree on the minimum
            t = torch.tensor([nb], dtype=torch.int64, device=self.device)
            import torch.distributed as dist

            dist.all_reduce(t, op=dist.ReduceOp.MIN, group=tp.handle)
            nb = int(t.item())
        t_kv = time.perf_counter()
        # TP ranks must all hold every page id the leader hands out: eager backing there
        self.kv = KVCache(mc.num_layers, nb, model.n_kv, mc.head_dim, self.device,
                          KV_DTYPES[cfg.kv_cache_dtype][0] or model.dtype, lazy=False if tp.size > 1 else None)
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        kv_alloc_ms = int(1e3 * (time.perf_counter() - t_kv))
        self.alloc = BlockAllocator(nb, available=self.kv.ready_blocks())
        self.max_blocks_per_seq = blocks_needed(self.max_model_len)
        self.buckets = sorted(b for b in cfg.graph_buckets if b <= cfg.max_num_seqs) or [cfg.max_num_seqs]
        if self.buckets[-1] < cfg.max_num_seqs:
            self.buckets.append(cfg.max_num_seqs)
        self.G = model.n_q // model.n_kv
        max_tokens, pad_rows, spec_kw = max(cfg.max_num_batched_tokens, cfg.max_num_seqs), self.buckets[-1], {}
        if self.spec_k:
            # a verify step: up to spec_max_batch rows of k + 1 tokens, a logits row for each.  Its
            # graph of bucket b has b (k + 1) tokens and b (ceil((k + 1) / qt) + 1) tiles: a row's
            # own tiles, and one more so that the token slots the rows leave unused always fit
            # the padding tiles (qt tokens each); every padding tile needs a padding row
            self.spec_max_batch = max(1, min(cfg.spec_max_batch, cfg.max_num_seqs))
            qt = max(1, 16 // self.G)
            self._spec_tpr = (self.spec_k + qt) // qt + 1
            self.spec_buckets = [b for b in self.buckets if b <= self.spec_max_batch]
            max_tokens = max(max_tokens, self.spec_max_batch * max(self.spec_k + 1, self._spec_tpr))  # (and tiles)
            pad_rows = max(pad_rows, max(self.spec_buckets, default=0) * self._spec_tpr)
            spec_kw = {"max_logits": self.spec_max_batch * (self.spec_k + 1)}
        self.meta = MetaBuffers(max_tokens, cfg.max_num_seqs + pad_rows, self.max_blocks_per_seq,
                                self.G, model.n_kv, self.max_model_len, self.device,
                                window=getattr(mc, "sliding_window", 0), **spec_kw,
                                # fp8 pages have no flash-prefill kernel: every row on the 16-row tiles
                                # (the route G > 8 takes)
                                **({"flash_min_q": 1 << 30} if self.fp8_kv else {}))
        self.window = self.meta.window
        self._swa = self.window > 0 and cfg.swa_release
        self.free_rows = list(range(cfg.max_num_seqs - 1, -1, -1))
        self.rows_hi = 0  # high-water row + 1: the block-table rows a step's upload / broadcast moves
        # struct-of-arrays state of running rows: the decode hot path is vectorised
        R = cfg.max_num_seqs
        self.r_len = np.zeros(R, np.int64)      # tokens in the sequence (prompt + output)
        self.r_gen = np.zeros(R, np.int64)      # generated tokens
        self.r_maxgen = np.zeros(R, np.int64)
        self.r_last = np.zeros(R, np.int64)     # last token (next decode input)
        self.r_ignore = np.zeros(R, bool)       # ignore_eos
        self.r_hasstop = np.zeros(R, bool)      # has stop_token_ids (checked in Python)
        self.r_nblk = np.zeros(R, np.int64)     # block-table entries in use (len(seq.blocks))
        self.r_nrel = np.zeros(R, np.int64)     # leading entries released below the sliding window
        self.r_sid = np.zeros(R, np.int64)
        self.r_random = np.zeros(R, bool)       # non-greedy sampling
        # sampler extensions, set when a request takes its row (_admit_ext): the row's slot of the
        # penalty count table (-1: none), its penalties, the top log-probabilities it wants (-1:
        # none), and "this row needs the sampler" (non-greedy, penalised or log-probabilities)
        self.r_pen_slot = np.full(R, -1, np.int32)
        self.r_rep = np.ones(R, np.float32)
        self.r_freq = np.zeros(R, np.float32)
        self.r_pres = np.zeros(R, np.float32)
        self.r_want = np.full(R, -1, np.int32)
        self.r_sampler = np.zeros(R, bool)
        self.r_slot = np.full(R, -1, np.int32)  # the row's LoRA adapter slot (-1: base model)
        self.r_gbase = np.full(R, -1, np.int32)  # first arena row of the row's grammar (-1: not guided)
        self.pen_table = None  # int32 [penalty_slots, vocab]: allocated by the first request that needs it
        self.free_pen_slots = list(range(max(0, cfg.penalty_slots) - 1, -1, -1))
        self._last_lp = None   # the last _sample's (logprobs, ids) device tensors, or None
        self._lp_h = None      # async: pinned double buffers of the log-probability read-back
        self.r_epoch = np.zeros(R, np.int64)    # bumped when a row is released (async: stale results)
        self.r_tokidx = np.zeros(R, np.int64)   # async: the row's pending token in the in-flight step
        # rows of ``self.running`` in order, and their output lists (kept in step with the
        # list: appended rows go to ``_rows_add``, finished rows are masked out in
        # ``_decode_finish``, a preempted one popped off the end; anything else sets dirty)
        self._rows = np.zeros(0, np.int32)
        self._outs: list[list] = []
        self._rows_add: list[int] = []
        self._rows_dirty = True
        self.sampler = Sampler(self.device, cfg.seed)
        self.waiting: collections.deque[Sequence] = collections.deque()
        self.prefilling: list[Sequence] = []
        self.running: list[Sequence] = []
        self.seqs: dict[int, Sequence] = {}
        self._ids = itertools.count()
        self._decode_since_prefill = 0
        self.graphs: dict[int, tuple] = {}
        self.graph_pool = None
        self.stats["kv_pages_released"] = 0
        if self.fp8_kv:
            # (only when it is not the default: the other entries are counters that callers
            # difference between two readings; read it as stats.get("kv_cache_dtype", "bf16"))
            self.stats["kv_cache_dtype"] = cfg.kv_cache_dtype
        # one-step-ahead (async) scheduling state: the in-flight step, its token read-back
        # buffers (two pinned, alternating) and the event after its metadata upload.  Under TP
        # only the leader schedules (workers follow the host-side headers, StepSync); under EP
        # every rank runs it, the per-step agreement happens at launch time (_ep_agree)
        self._async = cfg.async_scheduling and cfg.mixed_prefill
        self.graphs_spec: dict[int, tuple] = {}
        self._step_spec = False  # the step being launched is a verify step
        if self.spec_k:
            if self._async:
                # the host needs a step's accept counts to place the next step's tokens
                self._async = False
                self.stats["spec_async_off"] = 1
            self._spec_init()
        self._pending = None
        self._ids_gather = None
        self._meta_ev = None
        cuda = self.device.type == "cuda"
        nmax = self.meta.max_tokens
        self._toks_h = [torch.zeros(nmax, dtype=torch.int64, pin_memory=cuda) for _ in range(2)]
        self._toks_flip = 0
        self._src_h = torch.zeros(R, dtype=torch.int64, pin_memory=cuda)
        self._src_d = torch.zeros(R, dtype=torch.int64, device=self.device)
        self._ids_later = np.zeros(R, np.int64)  # per row: placeholder ids of a step whose ids _launch gathers
        if self.lora is not None:
            # per-token adapter slot of a step, beside the packed metadata (whose layout and upload
            # stay as they are): pinned host side, rewritten only after _wait_meta like the metadata
            self._ts_h = torch.full((nmax,), -1, dtype=torch.int32, pin_memory=cuda)
            self._ts_hn = self._ts_h.numpy()
            self._ts_d = torch.full((nmax,), -1, dtype=torch.int32, device=self.device)
            self.stats["lora_bytes"] = self.lora.nbytes()
        if self.ep_sync is not None and self.device.type == "cuda":
            self._setup_ep_exchange()
        self.stats["kv_alloc_ms"] = kv_alloc_ms
        self.stats.update(self.kv.timing_ms)
        self.tracer = StepTracer()
        self.profile_window = TorchProfileWindow()
        import os

        # fault injection (canary tests of the GPU-side guards): every forward step also runs a
        # device delay kernel of this many microseconds (ops/csrc/elementwise.hip device_delay)
        self._inject_device_us = int(os.environ.get("MLOP_INJECT_STEP_DEVICE_US", "0") or 0)
        if self._inject_device_us and self.device.type != "cuda":
            self._inject_device_us = 0
        if self._inject_device_us:
            from .. import ops as _ops

            _ops.load()

        # TP decode graphs capture the row-parallel all-reduces (K15 one-shot kernel, or RCCL
        # inside capture); the vocab gather runs after the replay (``_gather``).
        if cfg.use_graphs and self.device.type == "cuda":
            self.capture_graphs()
        self.kv.start_background_fill()  # after capture: the rest of a lazy KV arena
        self.stats["kv_ready_blocks_at_start"] = self.alloc.available

    def _setup_ep_exchange(self):
        """DP-attention + EP on GPU: the device-side MoE exchange over IPC peer memory
        (parallel/ep_ipc.py), sized for the largest forward this engine runs; collective over
        the EP group (every rank builds its engine together).  Without it (CPU): the group's
        all_to_all (parallel/moe.py)."""
        import os

        ep, mc = self.model.ps.ep, self.model.cfg
        if ep.ex is not None or not getattr(mc, "num_experts", 0):
            return
        from ..parallel.ep_ipc import EPExchange

        ep.ex = EPExchange(ep.rank, ep.size, mc.num_experts, mc.top_k, mc.hidden_size, self.meta.max_tokens,
                           self.device, group=ep.handle)

    # ------------------------------------------------------ speculation --
    def _check_spec(self, cfg, mc, model):
        """ValueError for what a speculative engine does not serve yet (each a follow-up)."""
        from .spec import MAX_NGRAM, MAX_SPEC_TOKENS

        k = cfg.spec_tokens
        if not isinstance(k, int) or not 1 <= k <= MAX_SPEC_TOKENS:
            raise ValueError(f"spec_tokens must be an int in [0, {MAX_SPEC_TOKENS}], got {k!r}")
        if not 1 <= cfg.spec_ngram_min <= cfg.spec_ngram_max <= MAX_NGRAM:
            raise ValueError(f"need 1 <= spec_ngram_min <= spec_ngram_max <= {MAX_NGRAM}, got "
                             f"{cfg.spec_ngram_min} / {cfg.spec_ngram_max}")
        if cfg.spec_max_batch < 1:
            raise ValueError(f"spec_max_batch must be >= 1, got {cfg.spec_max_batch}")
        if model.ps.tp.size > 1 or model.ps.ep.size > 1:
            raise ValueError("spec_tokens > 0 is not supported with tensor or expert parallelism")
        if getattr(mc, "is_moe", False):
            raise ValueError("spec_tokens > 0 is not supported for MoE models")
        if int(getattr(mc, "sliding_window", 0) or 0) > 0:
            raise ValueError(f"spec_tokens > 0 is not supported for sliding-window models "
                             f"(sliding_window = {mc.sliding_window})")
        if cfg.kv_cache_dtype == "fp8":
            raise ValueError('spec_tokens > 0 is not supported with kv_cache_dtype="fp8"')
        if cfg.max_adapters > 0:
            raise ValueError("spec_tokens > 0 is not supported with LoRA adapters (max_adapters > 0)")

    def _spec_init(self):
        """The speculative engine's state: every running row's tokens on the device (``hist`` /
        ``hist_len``, written by ops.spec_accept), the per-step arguments of the two kernels in
        ONE pinned buffer (one H2D) and their result (one D2H), and each row's next drafts."""
        from .spec import out_width

        R, k, dev = self.cfg.max_num_seqs, self.spec_k, self.device
        cuda = dev.type == "cuda"
        self.hist = torch.zeros(R, self.max_model_len, dtype=torch.int32, device=dev)
        self.hist_len = torch.zeros(R, dtype=torch.int32, device=dev)
        W = self._spec_w = out_width(k)
        self._spec_arg_h = torch.zeros(R * (4 + k), dtype=torch.int32, pin_memory=cuda)
        self._spec_arg_d = torch.zeros(R * (4 + k), dtype=torch.int32, device=dev)
        self._spec_out_d = torch.zeros(R, W, dtype=torch.int32, device=dev)
        self._spec_out_h = torch.zeros(R, W, dtype=torch.int32, pin_memory=cuda)
        self.r_nd = np.zeros(R, np.int64)            # the row's drafts for its next step
        self.r_drafts = np.zeros((R, k), np.int64)
        self.r_ext = np.zeros(R, bool)               # on the sampler's extended path: never drafts
        self.stats["spec_hist_bytes"] = self.hist.numel() * 4
        for key in ("spec_steps", "spec_graph_steps", "spec_drafted", "spec_accepted"):
            self.stats[key] = 0

    def _hist_load(self, s: Sequence) -> None:
        """A sequence is about to join the running rows (its prompt completes in the step being
        launched, re-admission after preemption included): its tokens so far go to hist[row], on
        the engine's stream; the step's spec_accept appends its first token behind them."""
        n = s.length
        self.hist[s.row, :n].copy_(torch.tensor(s.prompt + s.output, dtype=torch.int32))
        self.hist_len[s.row:s.row + 1].fill_(n)
        self.r_nd[s.row] = 0
        self.r_ext[s.row] = s.params.extended

    def _spec_drafts(self, rows):
        """Draft counts and drafts (int64 [B], [B, k]) of a decode-only step over ``rows``, or None:
        no row has any.  A row's cap is min(k, tokens it may still generate - 1, positions left -
        1), 0 on the sampler's extended path (penalties / log-probabilities: the draw depends on
        the previous token's table update).  The pages up to len + drafts are ensured; a row the
        allocator cannot serve drops its drafts (nothing is preempted for a draft)."""
        k = self.spec_k
        left = np.minimum(self.r_maxgen[rows] - self.r_gen[rows], self.max_model_len - self.r_len[rows]) - 1
        cap = np.where(self.r_ext[rows], 0, np.clip(left, 0, k))
        if self.spec_proposer is not None:
            nd, drafts = np.zeros(len(rows), np.int64), np.zeros((len(rows), k), np.int64)
            V = self.model.cfg.vocab_size
            for i in np.nonzero(cap)[0].tolist():
                d = [int(t) for t in self.spec_proposer(self.running[i], int(cap[i]))][:int(cap[i])]
                bad = next((j for j, t in enumerate(d) if not 0 <= t < V), len(d))
                nd[i] = bad
                drafts[i, :bad] = d[:bad]
        else:
            nd, drafts = np.minimum(self.r_nd[rows], cap), self.r_drafts[rows]
        for i in np.nonzero(nd)[0].tolist():
            if not self._ensure_blocks(self.running[i], int(self.r_len[rows[i]] + nd[i])):
                nd[i] = 0
        return (nd, drafts) if nd.any() else None

    def _spec_post(self, st: _Step, toks_d):
        """Behind a step's draw, on the same stream: ops.spec_accept over its logits sequences (the
        decode rows, then the completed prompts; plain rows have no drafts), ops.spec_propose for
        their next step, and ONE read-back of both: int32 [n, 2 + (k + 1) + k] (NumPy)."""
        k, B = self.spec_k, st.B
        arows = self._sample_rows(st.rows, st.done_seqs)
        n = len(arows)
        a = self._spec_arg_h.numpy()
        q0, nd, rw, cap = (a[i * n:(i + 1) * n] for i in range(4))  # [q_start | nd | rows | cap | drafts]
        dr = a[4 * n:(4 + k) * n].reshape(n, k)
        q0[:] = np.arange(n)
        nd[:] = 0
        dr[:] = 0
        if st.nd is not None:
            q0[:B], nd[:B], dr[:B] = st.q0, st.nd, st.drafts
            q0[B:] = st.nlog + np.arange(n - B)
        rw[:] = arows
        cap[:] = np.where(self.r_ext[arows], 0, k)
        m = (4 + k) * n
        ad = self._spec_arg_d
        ad[:m].copy_(self._spec_arg_h[:m], non_blocking=True)
        out_d = self._spec_out_d[:n]
        ops.spec_accept(toks_d, ad[:n], ad[4 * n:m].view(n, k), ad[n:2 * n], ad[2 * n:3 * n], self.hist,
                        self.hist_len, out_d)
        if self.spec_proposer is None:
            ops.spec_propose(self.hist, self.hist_len, ad[2 * n:3 * n], ad[3 * n:4 * n], self.cfg.spec_ngram_max,
                             self.cfg.spec_ngram_min, out_d)
        if self.device.type != "cuda":
            return out_d.numpy(), arows
        out_h = self._spec_out_h[:n]
        out_h.copy_(out_d, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return out_h.numpy(), arows

    def _spec_finish(self, rows, cnt, emitted, lp=None) -> StepBatch:
        """Bookkeeping of a verify step: running row i emitted ``emitted[i, :cnt[i]]``.  Stop
        tokens and EOS are applied in order: emission ends at the first one and the sequence
        finishes there."""
        run, eos = self.running, self.model.cfg.eos_ids
        n = len(rows)
        m = np.zeros(n, np.int64)
        last = np.zeros(n, np.int64)
        fin_stop = np.zeros(n, bool)
        toks = []
        for i, (s, c) in enumerate(zip(run, cnt.tolist())):
            t = emitted[i, :c].tolist()
            r = rows[i]
            stops = s.params.stop_token_ids if self.r_hasstop[r] else ()
            for j, tok in enumerate(t):
                if (not self.r_ignore[r] and tok in eos) or tok in stops:
                    t, fin_stop[i] = t[:j + 1], True
                    break
            s.output.extend(t)
            toks.extend(t)
            m[i], last[i] = len(t), t[-1]
        self.r_len[rows] += m
        self.r_gen[rows] += m
        self.r_last[rows] = last
        self.stats["decode_tokens"] += int(m.sum()) - n
        fin_len = (self.r_gen[rows] >= self.r_maxgen[rows]) | (self.r_len[rows] >= self.max_model_len)
        fin = fin_stop | fin_len
        lps = self._deliver_lp(run, lp, self.r_want[rows]) if lp is not None else None
        sids = np.repeat(self.r_sid[rows], m)
        fin_t = np.zeros(len(toks), bool)
        fin_t[np.cumsum(m) - 1] = fin  # a sequence finishes with its last emitted token
        reasons = self._retire_rows(rows, fin, fin_stop)
        return StepBatch(sids, np.asarray(toks, dtype=np.int64), fin_t, reasons, lps)

    # -------------------------------------------------- guided decoding --
    def _guided_init(self, cfg, model):
        """The grammar arena (int16 [grammar_states, ldv]) and the per-row automaton state, the
        host-side cache of compiled grammars and the list of those resident in the arena."""
        n = cfg.grammar_states
        self.g_arena = self.g_state = self._tok_bytes = None
        self._g_cache: collections.OrderedDict = collections.OrderedDict()
        self._g_lock = threading.Lock()
        self._g_resident: list = []
        self._g_tick = 0
        if not n:
            return
        from .guided import MAX_STATES

        if isinstance(n, bool) or not isinstance(n, int) or not 0 < n <= MAX_STATES:
            raise ValueError(f"grammar_states must be an int in [0, {MAX_STATES}], got {n!r}")
        if not isinstance(cfg.grammar_cache, int) or cfg.grammar_cache < 1:
            raise ValueError(f"grammar_cache must be an int >= 1, got {cfg.grammar_cache!r}")
        if model.ps.tp.size > 1 or model.ps.ep.size > 1:
            raise ValueError("grammar_states > 0 is not supported with tensor or expert parallelism")
        self.g_arena = ops.grammar_arena(n, model.cfg.vocab_size, self.device)
        self.g_state = torch.zeros(cfg.max_num_seqs, dtype=torch.int32, device=self.device)
        self.stats["grammar_arena_bytes"] = self.g_arena.numel() * 2
        self.stats["guided_rows"] = 0

    def set_tokenizer(self, tokenizer) -> None:
        """The tokenizer whose ids this engine's requests use: guided decoding walks the bytes of
        its tokens (ValueError for a tokenizer it cannot read).  Compiled grammars are dropped."""
        from .guided import token_bytes

        tb = token_bytes(tokenizer, self.model.cfg.vocab_size) if self.g_arena is not None else None
        with self._g_lock:
            self._tok_bytes = tb
            self._g_cache.clear()

    def compile_guided(self, params: SamplingParams):
        """The compiled grammar of a guided request, from the cache or compiled here, in the
        caller's thread; ValueError for what this engine cannot serve."""
        from . import guided

        if self.g_arena is None:
            raise ValueError("this engine serves no guided requests (grammar_states = 0)")
        if self._tok_bytes is None:
            raise ValueError("guided decoding needs the tokenizer (Engine.set_tokenizer)")
        if params.ignore_eos:
            raise ValueError("guided requests end with EOS: ignore_eos cannot be combined with guided")
        key = guided.spec_key(params.guided)
        with self._g_lock:
            g = self._g_cache.get(key)
            if g is not None:
                self._g_cache.move_to_end(key)
                return g
            tb = self._tok_bytes
        g = guided.compile(params.guided, tb, self.model.cfg.eos_ids, self.cfg.grammar_states)
        with self._g_lock:
            if tb is self._tok_bytes:
                g = self._g_cache.setdefault(key, g)
                while len(self._g_cache) > self.cfg.grammar_cache:
                    self._g_cache.popitem(last=False)
        return g

    def _grammar_place(self, g) -> bool:
        """Make ``g`` resident in the arena: first fit over the free ranges; while none is large
        enough, the least recently used grammar no admitted row refers to gives up its range.
        False: the arena is held by live requests (the caller waits).  The upload is one copy on
        the engine's stream, behind every launched step that still reads the range."""
        self._g_tick += 1
        g.tick = self._g_tick
        if g.base >= 0:
            return True
        S, A = g.num_states, self.cfg.grammar_states
        while True:
            pos = 0
            for r in sorted(self._g_resident, key=lambda r: r.base):
                if r.base - pos >= S:
                    break
                pos = r.base + r.num_states
            if pos + S <= A and all(pos + S <= r.base or r.base + r.num_states <= pos for r in self._g_resident):
                break
            idle = [r for r in self._g_resident if r.refs == 0]
            if not idle:
                return False
            victim = min(idle, key=lambda r: r.tick)
            victim.base = -1
            self._g_resident.remove(victim)
            self.stats["grammar_evictions"] += 1
        V = g.next.shape[1]
        self.g_arena[pos:pos + S, :V].copy_(torch.from_numpy(g.next), non_blocking=False)
        g.base = pos
        self._g_resident.append(g)
        self.stats["grammar_uploads"] += 1
        return True

    def _admit_guided(self, seq: Sequence) -> bool:
        """A guided request takes its row: its grammar becomes resident (False: no range, it
        waits) and the row's state is set on the engine's stream: 0, or after preemption the
        state reached by walking the output so far through the host copy of the table."""
        g = seq.grammar
        if not self._grammar_place(g):
            return False
        g.refs += 1
        seq.g_admitted = True
        r = seq.row
        self.g_state[r:r + 1].fill_(g.walk(seq.output))
        self.r_gbase[r] = g.base
        return True

    # ------------------------------------------------------- embeddings --
    def _embed_init(self, cfg, model):
        """The pooling state of an engine that serves embedding requests: the fp32 accumulator and
        the finished vectors ([embed_slots, H] each), the pinned mirror the vectors come back
        through, and a step's segment / finish rows (int32 [2 embed_slots, 4]: a step carries at
        most one chunk per slot) on both sides of their H2D."""
        n = cfg.embed_slots
        self._pool_acc = None
        self._free_embed: list = []
        self._step_pool = None  # the step being launched: (segments, finish rows, [(slot, d)]) or None
        if not n:
            return
        if isinstance(n, bool) or not isinstance(n, int) or not 0 < n <= 65535:
            raise ValueError(f"embed_slots must be an int in [0, 65535], got {n!r}")
        if model.ps.tp.size > 1 or model.ps.ep.size > 1:
            raise ValueError("embed_slots > 0 is not supported with tensor or expert parallelism "
                             "(the pooled rows would need the segment metadata on every rank)")
        if self.spec_k:
            raise ValueError("embed_slots > 0 is not supported on a speculative engine (spec_tokens > 0)")
        if cfg.max_adapters > 0:
            raise ValueError("embed_slots > 0 is not supported with LoRA adapters (max_adapters > 0)")
        if getattr(model.cfg, "is_moe", False):
            raise ValueError("embed_slots > 0 is not supported for MoE models")
        H, dev = model.cfg.hidden_size, self.device
        if H % 8:
            raise ValueError(f"embed_slots > 0 needs a hidden size that is a multiple of 8, got {H}")
        cuda = dev.type == "cuda"
        self._pool_acc = torch.zeros(n, H, dtype=torch.float32, device=dev)
        self._pool_out = torch.zeros(n, H, dtype=torch.float32, device=dev)
        self._pool_out_h = torch.zeros(n, H, dtype=torch.float32, pin_memory=cuda)
        self._pool_h = torch.zeros(2 * n, 4, dtype=torch.int32, pin_memory=cuda)
        self._pool_hn = self._pool_h.numpy()
        self._pool_d = torch.zeros(2 * n, 4, dtype=torch.int32, device=dev)
        self._free_embed = list(range(n - 1, -1, -1))
        self.stats["embed_bytes"] = 2 * n * H * 4
        for key in ("embed_requests", "embed_tokens", "embed_steps"):
            self.stats[key] = 0

    def _fill_pool(self, st: _Step) -> None:
        """The step's pool segments and finish rows into the pinned buffer (rewritten only after
        ``_wait_meta``, like the metadata): one segment per embedding sequence of ``st.batch``, its
        chunk's rows in the step's token order (the decode rows, then each prompt chunk).  Leaves
        ``_step_pool`` (None: the step carries no embedding chunk)."""
        self._step_pool = None
        if self._pool_acc is None or not any(s.params.embed is not None for s in st.batch):
            return
        S = self.cfg.embed_slots
        seg, fin = self._pool_hn[:S], self._pool_hn[S:]
        H = self.model.cfg.hidden_size
        t, ns, fins = st.B, 0, []
        for s, n, c, e in zip(st.batch, st.chunks, st.p_ctx, st.emb_done):
            p = s.params
            if p.embed is not None:
                mean = p.embed == "mean"
                flags = (0 if mean else ops.POOL_MODE_LAST) | (ops.POOL_LAST if e else 0)
                if c - n == 0:  # the first computed chunk (again after preemption): overwrite the slot
                    flags |= ops.POOL_INIT
                seg[ns] = (t, t + n, s.emb_slot, flags)
                ns += 1
                self.stats["embed_tokens"] += n
                if e:
                    d = p.embed_dim or H
                    f_flags = (ops.POOL_FIN_MEAN if mean else 0) | (ops.POOL_FIN_NORMALIZE if p.embed_normalize else 0)
                    fin[len(fins)] = (s.emb_slot, s.length, d, f_flags)  # (mean: over the sequence's own tokens)
                    fins.append((s.emb_slot, d))
            t += n
        self._step_pool = (ns, len(fins), fins)

    def _pool_run(self, hidden) -> None:
        """Behind a step's forward, on its stream: pool the step's segments, finish the vectors that
        completed and start their copies to the pinned mirror (a slot's row of the mirror belongs
        to its sequence until the vector is delivered)."""
        ns, nf, fins = self._step_pool
        S = self.cfg.embed_slots
        cuda = self.device.type == "cuda"
        ops.pool_accumulate(hidden, self._pool_d[:S], self._pool_acc, ns)
        if nf:
            ops.pool_finish(self._pool_acc, self._pool_d[S:], self._pool_out, nf)
            for slot, d in fins:
                self._pool_out_h[slot, :d].copy_(self._pool_out[slot, :d], non_blocking=cuda)
        self.stats["embed_steps"] += 1

    def _deliver_embeds(self, emb) -> list:
        """StepOutputs of the embeddings a step finished, once its copies to the pinned mirror have
        executed; a sequence aborted meanwhile (its slot freed, maybe re-taken) is dropped."""
        outs = []
        for s, slot, d in emb:
            if s.status == Status.FINISHED or s.emb_slot != slot:
                continue
            s.embedding = self._pool_out_h[slot, :d].numpy().copy()
            if s.first_token_time is None:
                s.first_token_time = time.perf_counter()
            self._finish(s, "embedding")
            self.stats["embed_requests"] += 1
            outs.append(StepOutput(s.seq_id, -1, True, "embedding", embedding=s.embedding))
        return outs

    def embed(self, prompts, pooling: str = "last", normalize: bool = True, dim: int | None = None) -> list:
        """Offline batch API beside ``generate``: one fp32 vector (np.ndarray [dim or hidden]) per prompt."""
        sp = SamplingParams(embed=pooling, embed_normalize=normalize, embed_dim=dim)
        seqs = [self.add_request(p, sp) for p in prompts]
        while any(s.status != Status.FINISHED for s in seqs):
            self.step()
        return [s.embedding for s in seqs]

    # ----------------------------------------------------------- sizing --
    def _auto_blocks(self) -> int:
        mc, m = self.model.cfg, self.model
        if self.cfg.kv_cache_bytes:
            budget = self.cfg.kv_cache_bytes
        elif self.device.type == "cuda" and os.environ.get("MLOP_SHARE_GPU", "0") not in ("", "0", "false"):
            # one-GPU rehearsal of a multi-rank pod: the ranks size their pools concurrently, so
            # a "free HBM" reading races the others' allocations; split the card's usable
            # capacity evenly instead (every rank holds a same-size weight shard)
            _, total = torch.cuda.mem_get_info(self.device)
            n = int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", 1)))
            usable = total * self.cfg.gpu_memory_utilization - 4 * 2**30 - n * m.weight_bytes()
            budget = int(max(usable / max(1, n), 2**30))
        elif self.device.type == "cuda":
            free, total = torch.cuda.mem_get_info(self.device)
            reserve = total * (1 - self.cfg.gpu_memory_utilization) + 4 * 2**30
            budget = int(max(free - reserve, 2**30))
        else:
            budget = 64 * 2**20
        need = int(self.cfg.kv_fraction * self.cfg.max_num_seqs *
                   blocks_needed(min(self.cfg.max_model_len, mc.max_position))) + 2
        nb = blocks_for_budget(budget, mc.num_layers, m.n_kv, mc.head_dim, *self._kv_bytes)
        return int(min(nb, need))

    # -------------------------------------------------------- requests --
    def check_request(self, prompt, params: SamplingParams | None = None) -> None:
        """ValueError when this engine cannot serve the request (empty / too long prompt, token
        ids outside the vocabulary, unusable sampling parameters)."""
        if not prompt:
            raise ValueError("empty prompt")
        # (a generation prompt needs room for one token; an embedding input may fill the context)
        embed = params is not None and params.embed is not None
        if len(prompt) >= self.max_model_len + int(embed):
            raise ValueError(f"prompt of {len(prompt)} tokens exceeds max_model_len {self.max_model_len}")
        V = self.model.cfg.vocab_size
        if min(prompt) < 0 or max(prompt) >= V:
            raise ValueError(f"prompt token ids must be in [0, {V})")
        params = (params or SamplingParams()).validate()
        if params.penalised and self.cfg.penalty_slots <= 0:
            raise ValueError("this engine serves no penalised requests (penalty_slots = 0)")
        if params.adapter is not None and params.adapter not in self._adapters:
            raise ValueError(f"unknown adapter {params.adapter!r} (loaded: {sorted(self._adapters)})")
        if params.guided is not None:
            self.compile_guided(params)  # compiles it (or finds it in the cache): ValueError for a bad one
        if params.embed is None:
            if getattr(self.model.cfg, "embedding_only", False):
                raise ValueError("this model serves embeddings only (a base-model checkpoint without an LM head): "
                                 "the request must name a pooling mode")
            return
        if self._pool_acc is None:
            raise ValueError("this engine serves no embedding requests (embed_slots = 0)")
        H = self.model.cfg.hidden_size
        if params.embed_dim is not None and params.embed_dim > H:
            raise ValueError(f"embed_dim must be in [1, {H}] (the model's hidden size), got {params.embed_dim}")

    def add_request(self, prompt, params: SamplingParams | None = None, seq_id: int | None = None) -> Sequence:
        params = params or SamplingParams()
        prompt = list(prompt)
        self.check_request(prompt, params)
        sid = next(self._ids) if seq_id is None else seq_id
        seq = Sequence(sid, prompt, params)
        if params.adapter is not None:
            ad = self._adapters[params.adapter]
            seq.slot, seq.prefix_seed = ad["slot"], ad["seed"]
            self._slot_refs[seq.slot] += 1
        if params.guided is not None:
            # pinned: the sequence keeps its compiled grammar whatever the cache drops meanwhile
            seq.grammar = self.compile_guided(params)
        self.seqs[sid] = seq
        self.waiting.append(seq)
        return seq

    def abort(self, seq_id: int) -> None:
        seq = self.seqs.get(seq_id)
        if seq is None or seq.status == Status.FINISHED:
            return
        for lst in (self.prefilling, self.running):
            if seq in lst:
                lst.remove(seq)
        self._rows_dirty = True
        if seq in self.waiting:
            self.waiting.remove(seq)
        self._finish(seq, "abort")

    def has_work(self) -> bool:
        return bool(self.waiting or self.prefilling or self.running or self._pending_alive())

    @property
    def num_running(self) -> int:
        return len(self.running) + len(self.prefilling)

    def kv_usage(self) -> float:
        return self.alloc.usage()

    # ------------------------------------------------------ bookkeeping --
    def _ensure_blocks(self, seq: Sequence, ctx: int) -> bool:
        need = blocks_needed(ctx) - len(seq.blocks)
        if need <= 0:
            return True
        if not self.alloc.can_allocate(need):
            return False
        new = self.alloc.allocate(need)
        start = len(seq.blocks)
        seq.blocks.extend(new)
        self.meta.bt_h[seq.row, start:start + need] = new
        self.r_nblk[seq.row] = len(seq.blocks)
        return True

    def _release_window(self, seq: Sequence, nxt: int) -> None:
        """Sliding window: give back every page wholly below the pair-aligned start of the window
        of the sequence's NEXT query (position ``nxt``: it attends nxt - W + 1 .. nxt, and the
        kernels read from the page pair holding that first key).  Released block-table entries
        become the null page 0; the list keeps its length.  Pages registered in the prefix
        cache drop this reference and stay cached, as when a sequence ends.  Called while a step
        is built: a page handed to another sequence is written by that step or a later one,
        behind every launched step that still reads it."""
        first = min(((max(0, nxt - self.window + 1)) & ~31) >> 4, len(seq.blocks))
        if first <= seq.n_rel:
            return
        gone = [b for b in seq.blocks[seq.n_rel:first] if b]
        if gone:
            self.alloc.free(gone)
            self.stats["kv_pages_released"] += len(gone)
        seq.blocks[seq.n_rel:first] = [0] * (first - seq.n_rel)
        self.meta.bt_h[seq.row, seq.n_rel:first] = 0
        seq.n_rel = first
        self.r_nrel[seq.row] = first

    def _release(self, seq: Sequence):
        if seq.blocks:
            # (released window entries are the null page: never freed)
            self.alloc.free([b for b in seq.blocks if b] if seq.n_rel else seq.blocks)
            seq.blocks = []
        seq.n_reg = 0
        seq.n_rel = 0
        if seq.pen_slot >= 0:
            # the slot's pending penalty_update launches (a speculatively decoded row) are already
            # on the stream: the next owner's penalty_reset is enqueued behind them
            self.free_pen_slots.append(seq.pen_slot)
            seq.pen_slot = -1
        if seq.g_admitted:
            # the grammar stays resident until its range is needed (_grammar_place)
            seq.grammar.refs -= 1
            seq.g_admitted = False
        if seq.row >= 0:
            self.r_pen_slot[seq.row], self.r_want[seq.row] = -1, -1
            self.r_gbase[seq.row] = -1
            self.r_slot[seq.row] = -1
            self.r_nblk[seq.row] = 0
            self.r_nrel[seq.row] = 0
            self.r_epoch[seq.row] += 1  # an in-flight step's result for this row is stale
            self.free_rows.append(seq.row)
            seq.row = -1
        seq.num_cached = 0

    def _admit_ext(self, seq: Sequence) -> bool:
        """A request takes its row: its sampler-extension state.  A penalised request also takes a
        slot of the count table (False: none free, it waits) and the slot is rebuilt from the
        prompt (mask) and the output so far (counts: re-admission after preemption), on the
        engine's stream, so ahead of the first step that draws for it."""
        r, p = seq.row, seq.params
        self.r_slot[r] = seq.slot
        self.r_sampler[r] = (not p.greedy) or p.extended
        self.r_want[r] = -1 if p.logprobs is None else p.logprobs
        self.r_pen_slot[r] = -1
        self.r_gbase[r] = -1
        if p.penalised and not self.free_pen_slots:
            return False
        if seq.grammar is not None and not self._admit_guided(seq):
            return False  # the arena is held by live requests: it waits, like for a table slot
        if not p.penalised:
            return True
        if self.pen_table is None:
            self.pen_table = ops.penalty_table(self.cfg.penalty_slots, self.model.cfg.vocab_size, self.device)
            self.stats["penalty_table_bytes"] = self.pen_table.numel() * 4
        seq.pen_slot = self.free_pen_slots.pop()
        ops.penalty_reset(self.pen_table, seq.pen_slot, seq.prompt, seq.output, self.model.cfg.vocab_size)
        self.r_pen_slot[r] = seq.pen_slot
        self.r_rep[r], self.r_freq[r], self.r_pres[r] = p.repetition_penalty, p.frequency_penalty, p.presence_penalty
        return True

    def _ext_of(self, rows):
        """The sampler-extension arrays of a step's logits rows (None: no row uses them)."""
        slots, want, gbase = self.r_pen_slot[rows], self.r_want[rows], self.r_gbase[rows]
        guided = self.g_arena is not None and bool((gbase >= 0).any())
        if not ((slots >= 0).any() or (want >= 0).any() or guided):
            return None
        self.stats["sampler_ext_rows"] += int(((slots >= 0) | (want >= 0)).sum())
        if not guided:
            return SamplerExt(self.pen_table, slots, self.r_rep[rows], self.r_freq[rows], self.r_pres[rows], want,
                              self.model.cfg.vocab_size)
        self.stats["guided_rows"] += int((gbase >= 0).sum())
        return SamplerExt(self.pen_table, slots, self.r_rep[rows], self.r_freq[rows], self.r_pres[rows], want,
                          self.model.cfg.vocab_size, self.g_arena, gbase, rows, self.g_state)

    def _register_running(self, s: Sequence, in_flight: int = 0):
        """Row registers of a sequence that joins the running rows; ``in_flight`` = 1: its first
        token is still being computed (it counts in the lengths now, ``r_last`` comes with it)."""
        r, p = s.row, s.params
        self.r_random[r] = not p.greedy
        self.r_len[r], self.r_gen[r], self.r_maxgen[r] = s.length + in_flight, len(s.output) + in_flight, p.max_tokens
        if not in_flight:
            self.r_last[r] = s.output[-1] if s.output else s.prompt[-1]
        self.r_ignore[r], self.r_hasstop[r], self.r_sid[r] = p.ignore_eos, bool(p.stop_token_ids), s.seq_id
        self._rows_add.append(r)  # s was just appended to self.running

    def _finish(self, seq: Sequence, reason: str):
        seq.status = Status.FINISHED
        seq.finish_reason = reason
        seq.finish_time = time.perf_counter()
        self._release(seq)
        if seq.emb_slot >= 0:
            # (kept across preemption; an in-flight step that still writes the slot is ahead of
            # the next owner's first chunk on the stream)
            self._free_embed.append(seq.emb_slot)
            seq.emb_slot = -1
        if seq.slot >= 0:  # the adapter may be unloaded once no live sequence names it
            self._slot_refs[seq.slot] -= 1
            seq.slot = -1

    def _preempt(self, seq: Sequence):
        self.stats["preemptions"] += 1
        self._release(seq)
        seq.status = Status.WAITING
        self.waiting.appendleft(seq)

    # ------------------------------------------------------- scheduling --
    def _want_prefill(self) -> bool:
        if self.prefilling:
            return True
        if not self.waiting or not self.free_rows:
            return False
        if not self.running:
            return True
        c = self.cfg
        return (len(self.waiting) >= c.prefill_min_batch
                or (c.max_decode_gap and self._decode_since_prefill >= c.max_decode_gap))

    def step(self) -> list[StepOutput]:
        """One scheduler step (traced: ``self.tracer`` spans, optional torch.profiler window)."""
        self.profile_window.before_step()
        t0 = time.perf_counter()
        n0d, n0p = self.stats["decode_tokens"], self.stats["prefill_tokens"]
        kind, out = self._step()
        self._check_peers()
        self.tracer.record(kind, t0, time.perf_counter(), decode_tokens=self.stats["decode_tokens"] - n0d,
                           prefill_tokens=self.stats["prefill_tokens"] - n0p, running=len(self.running),
                           waiting=len(self.waiting))
        self.profile_window.after_step()
        return out

    def _check_peers(self):
        """Error words of the device-side collectives (K15 all-reduce / broadcast / all-gather, the
        EP exchange; host-mapped, so this is a plain load, no sync): a flag wait that timed out
        means a peer rank died or wedged and its results are garbage.  Fail loudly -- the launcher
        restarts the predictor -- instead of serving them."""
        ps = getattr(self.model, "ps", None)
        if ps is None:
            return
        for name, obj in (("tensor-parallel custom collectives", getattr(ps.tp, "car", None)),
                          ("expert-parallel exchange", getattr(getattr(ps, "ep", None), "ex", None))):
            code = obj.error() if obj is not None else 0
            if code:
                raise RuntimeError(f"{name}: a peer flag wait timed out (error word {code}): a rank died "
                                   f"or wedged, results since then are invalid")

    def _step(self):
        self._launched = False
        kind, out = self._step_local()
        if self.ep_sync is not None and not self._launched:
            self._ep_idle()  # nothing launched here (idle, or nothing schedulable): still join
        return kind, out

    def _ep_idle(self):
        """EP rank with nothing scheduled: agree, then run a padding-only forward (one row
        that attends nothing) eagerly, or replay the agreed decode graph on padding rows."""
        any_work, eager, t_max, bucket = self.ep_sync.agree(0, 0, 0, 0, int(self.has_work()))
        if not any_work:
            return
        self._wait_meta()  # async: the previous step's metadata H2D must have read the host buffer
        empty = np.zeros(0, dtype=np.int32)
        if eager or bucket not in self.graphs:
            self.meta.fill_decode(empty, empty, np.zeros(0, dtype=np.int64), pad_to=1)
            self.meta.upload(1, 1, self.rows_hi)
            self.model.moe_capacity_tokens = t_max
            self.model.forward(self.meta.ids_d[:1], self.meta.meta(1, 1, 1, 32, 1), self.kv)
        else:
            self.meta.fill_decode(empty, empty, np.zeros(0, dtype=np.int64), pad_to=bucket)
            self.meta.upload(bucket, bucket, self.rows_hi)
            self.graphs[bucket][0].replay()
        self._record_meta_ev()
        self.stats["ep_idle_steps"] += 1

    def _step_local(self):
        if self.alloc.available < self.alloc.num_blocks and not self.kv.fill_failed:
            self.alloc.grow(self.kv.ready_blocks())  # lazily backed KV chunks became ready
            if self.kv.fill_failed:
                self.stats["kv_fill_failed"] = 1
                self.stats["kv_blocks_backed"] = self.alloc.available
        if self._async and (self._pending is not None or self.running):
            return self._async_step()
        if self._want_prefill():
            mixed = bool(self.running) and self.cfg.mixed_prefill
            out = self._sync_step(decode=mixed, prompt=True)
            if out is not None:
                self._decode_since_prefill = 0
                return ("mixed" if mixed else "prefill"), out
        if self.running:
            self._decode_since_prefill += 1
            return "decode", self._sync_step(decode=True, prompt=False) or StepBatch.from_list([])
        return "idle", []

    # ---------------------------------------------------------- prefill --
    def _collect_prefill(self, budget: int):
        """Admit prompt chunks up to ``budget`` tokens: continuing chunked
        prefills first, then waiting requests (each needs a free row + pages)."""
        batch, chunks = [], []
        for seq in list(self.prefilling):
            if budget <= 0:
                break
            n = min(seq.length - seq.num_cached, budget)
            if self._swa:  # between chunks: the pages below the next chunk's first window
                self._release_window(seq, seq.num_cached)
            if not self._ensure_blocks(seq, seq.num_cached + n):
                break
            batch.append(seq)
            chunks.append(n)
            budget -= n
        skip = 0  # embedding requests at the head of the queue that wait for a slot: those behind go on
        while budget > 0 and len(self.waiting) > skip and self.free_rows:
            seq = self.waiting[skip]
            if seq.params.embed is not None and seq.emb_slot < 0:
                if not self._free_embed:
                    skip += 1
                    continue
                seq.emb_slot = self._free_embed.pop()
            seq.row = self.free_rows.pop()
            self.rows_hi = max(self.rows_hi, seq.row + 1)
            if not self._admit_ext(seq):
                self._release(seq)  # no free slot of the penalty table: it waits, like for a row
                break
            # (mean pooling needs every token's hidden state: it matches no cached page)
            if self.cfg.enable_prefix_caching and seq.params.embed != "mean":
                self._match_prefix(seq)
                if self._swa:  # a hit took all its pages: those below the window go straight back
                    self._release_window(seq, seq.num_cached)
            n = min(seq.length - seq.num_cached, budget)
            if not self._ensure_blocks(seq, seq.num_cached + n):
                self._release(seq)  # matched prefix pages back to the cache, row freed
                break
            del self.waiting[skip]
            # prefix-cache stats once per admission (a head request that waits for pages
            # re-matches every step and must not inflate the hit rate)
            self.stats["prefix_query_tokens"] += seq.length
            self.stats["prefix_hit_tokens"] += seq.num_cached
            seq.status = Status.PREFILL
            self.prefilling.append(seq)
            batch.append(seq)
            chunks.append(n)
            budget -= n
        return batch, chunks

    def _match_prefix(self, seq: Sequence) -> None:
        """Reuse cached pages of this sequence's longest cached prefix (never the page
        holding its last token: that one is computed to get the next-token logits)."""
        nfull = (seq.length - 1) // BLOCK_SIZE
        if nfull <= 0:
            return
        if len(seq.hashes) < nfull:
            prev = seq.hashes[-1] if seq.hashes else seq.prefix_seed
            seq.hashes += prefix_hashes(seq.tokens(0, nfull * BLOCK_SIZE), nfull, len(seq.hashes), prev)
        m = 0
        for h in seq.hashes[:nfull]:
            b = self.alloc.lookup(h)
            if b is None:
                break
            self.alloc.take(b)
            seq.blocks.append(b)
            m += 1
        if m:
            self.meta.bt_h[seq.row, :m] = seq.blocks
            self.r_nblk[seq.row] = m
            seq.num_cached = m * BLOCK_SIZE
            seq.n_reg = m

    def _register_prefix(self, seq: Sequence, ctx: int) -> None:
        """Publish the pages this prefill filled (full pages of computed tokens)."""
        full = ctx // BLOCK_SIZE
        if full <= seq.n_reg:
            return
        if len(seq.hashes) < full:
            prev = seq.hashes[-1] if seq.hashes else seq.prefix_seed
            seq.hashes += prefix_hashes(seq.tokens(0, full * BLOCK_SIZE), full, len(seq.hashes), prev)
        for i in range(max(seq.n_reg, seq.n_rel), full):  # (not the null entries of released pages)
            self.alloc.register(seq.blocks[i], seq.hashes[i])
        seq.n_reg = full

    def _lp_entry(self, lp_h, id_h, i: int, n: int):
        """Row i of a step's log-probability read-back -> (logprob, [(id, logprob)] * n)."""
        return float(lp_h[i, 0]), list(zip(id_h[i, 1:1 + n].tolist(), lp_h[i, 1:1 + n].tolist()))

    # ------------------------------------------------------------ steps --
    def _build_step(self, decode: bool, prompt: bool, ids: np.ndarray):
        """Plan one step and fill its metadata: every running row's next token (``decode``), prompt
        chunks up to the token budget (``prompt``), or both in ONE eager ragged forward (a mixed
        step, chunked-prefill piggybacking: the decode rows share the prefill's weight reads and
        its larger-M GEMMs instead of paying a separate M=B pass).  A decode-only step replays
        the graph of the smallest bucket >= B where one was captured.  ``ids``: per engine row, the
        decode rows' input ids (``r_last``; placeholders when ``_launch`` gathers them on the
        device).  None: nothing to run (no row decodes, fewer than ``mixed_min_chunk`` token slots
        beside the decode rows, or no prompt chunk fits); what was preempted or admitted on the
        way stays so."""
        cfg, meta, n_kv = self.cfg, self.meta, self.model.n_kv
        st = _Step()
        budget = cfg.max_num_batched_tokens
        rows = ctx_d = np.zeros(0, np.int32)
        if decode:
            rows, ctx_d = self._decode_rows()  # (may preempt)
            if len(rows) == 0:
                return None
            ctx_d = ctx_d.astype(np.int32)
            budget -= len(rows)
        B = len(rows)
        batch, chunks = [], []
        if prompt:
            if decode and budget < cfg.mixed_min_chunk:
                return None
            batch, chunks = self._collect_prefill(budget)
            if not batch:
                return None
        p_ctx = [s.num_cached + n for s, n in zip(batch, chunks)]
        done = [c == s.length for s, c in zip(batch, p_ctx)]
        # an embedding sequence's last chunk gets no logits row and joins nothing: emb_done, not done
        emb_done = [d and s.params.embed is not None for s, d in zip(batch, done)]
        done = [d and not e for d, e in zip(done, emb_done)]
        done_seqs = [s for s, d in zip(batch, done) if d]
        last = ids[rows]
        mctx = max(int(ctx_d.max()) if B else 0, max(p_ctx, default=0))
        st.nd = st.drafts = st.q0 = st.goff = None
        spec = self._spec_drafts(rows) if (self.spec_k and B and not batch and B <= self.spec_max_batch) else None
        self._step_spec = spec is not None
        if spec is not None:
            # a verify step: row i's last token and its drafts, causal inside the row, a logits
            # row for every token; replays the verify graph of the bucket where one was captured
            k = self.spec_k
            st.nd, st.drafts = nd, drafts = spec
            q_lens = 1 + nd
            st.q0 = np.cumsum(q_lens) - q_lens
            toks = [[int(last[i]), *drafts[i, :nd[i]].tolist()] for i in range(B)]
            bucket = next((b for b in self.buckets if b >= B), None)
            pad = {}
            if self.graphs_spec.get(bucket) is not None:
                pad = {"pad_tokens": bucket * (k + 1), "pad_tiles": bucket * self._spec_tpr}
            T, nt, nl = meta.fill_verify(rows, q_lens, ctx_d + nd.astype(np.int32), toks, **pad)
            if pad:
                st.launch = (KIND_GRAPH, T, nt, nl, 0, 0, bucket)
            else:
                st.launch = (KIND_EAGER, T, nt, nl, *plan_partitions(nt, n_kv, meta.span(mctx + k)), 0)
        elif batch:
            T, nt, nl = meta.fill_mixed(rows, ctx_d, last, [s.row for s in batch], chunks, p_ctx,
                                        [s.tokens(s.num_cached, c) for s, c in zip(batch, p_ctx)], want_logits=done)
            st.launch = (KIND_EAGER, T, nt, nl, *plan_partitions(nt, n_kv, meta.span(mctx)), 0)
        else:
            bucket = next((b for b in self.buckets if b >= B), None)
            if bucket is not None and self.graphs.get(bucket) is not None:
                meta.fill_decode(rows, ctx_d, last, pad_to=bucket)
                self._repad = (rows, ctx_d, last, mctx)  # EP: the group may re-pad it
                st.launch = (KIND_GRAPH, bucket, bucket, bucket, 0, 0, bucket)
            else:
                meta.fill_decode(rows, ctx_d, last, pad_to=B)
                st.launch = (KIND_EAGER, B, B, B, *plan_partitions(B, n_kv, meta.span(mctx)), 0)
        st.T = st.launch[1]
        self._fill_tok_slot(st.T, rows, batch, chunks)
        # a falsy r_sampler lets the sampler take the all-greedy fast path without a per-sequence scan
        if not self.r_sampler[rows].any() and not any(self.r_sampler[s.row] for s in done_seqs):
            st.params = _ALL_GREEDY
        else:
            st.params = _ParamsList([s.params for s in (self.running if decode else ())] + [s.params for s in done_seqs])
        st.greedy = st.params is _ALL_GREEDY
        st.rows, st.ctx_d, st.B, st.srows = rows, ctx_d, B, self._sample_rows(rows, done_seqs)
        st.nlog = B + len(done_seqs)
        if spec is not None:
            # one draw per token: the row's own params repeated, output positions consecutive
            st.nlog = int(q_lens.sum())
            st.srows = np.repeat(rows, q_lens)
            st.goff = np.arange(st.nlog) - np.repeat(st.q0, q_lens)
            if not st.greedy:
                st.params = _ParamsList([s.params for s, q in zip(self.running, q_lens.tolist()) for _ in range(q)])
        st.batch, st.chunks, st.p_ctx, st.done, st.done_seqs = batch, chunks, p_ctx, done, done_seqs
        st.emb_done, st.emb_out = emb_done, []
        self._fill_pool(st)
        return st

    def _issue(self, st: _Step):
        """Launch a built step and draw its tokens: (token ids, (log-probabilities, ids) or None),
        both on the device; (None, None) when it has no logits row (prompt chunks, none the last
        of its prompt)."""
        logits = self._launch(*st.launch, greedy=st.greedy)
        B = st.B
        if st.batch:
            self.stats["mixed_steps" if B else "prefill_steps"] += 1
            self.stats["prefill_tokens"] += st.T - B
        else:
            self.stats["graph_steps" if st.launch[0] == KIND_GRAPH else "eager_decode_steps"] += 1
            self.stats["decode_steps"] += 1
        if B:
            self.stats["decode_tokens"] += B
        if st.nd is not None:
            self.stats["spec_steps"] += 1
            self.stats["spec_graph_steps"] += int(st.launch[0] == KIND_GRAPH)
            self.stats["spec_drafted"] += int(st.nd.sum())
        if logits is None:
            return None, None
        if st.launch[0] == KIND_GRAPH:
            logits = logits[:st.nlog]  # (its padding rows)
        if st.nd is not None:
            gen_index = lambda: self.r_gen[st.srows] + st.goff  # noqa: E731
        else:
            gen_index = lambda: self._gen_index(st.rows, st.done_seqs)  # noqa: E731
        toks_d = self._sample(logits, st.params, gen_index, st.srows)
        lp_d, self._last_lp = self._last_lp, None
        return toks_d, lp_d

    def _sync_step(self, decode: bool, prompt: bool):
        """Build a step, run it and apply its tokens at once: the synchronous engine (and, under
        one-step-ahead scheduling, prompt work while nothing decodes).  None: nothing to run."""
        t0 = time.perf_counter()
        st = self._build_step(decode, prompt, self.r_last)
        if st is None:
            return None
        t1 = time.perf_counter()
        if self.spec_k:
            for s in st.done_seqs:
                self._hist_load(s)
        toks_d, lp_d = self._issue(st)
        toks = lp = res = None
        if toks_d is not None and self.spec_k:
            # every sampled token of a speculative engine goes through spec_accept (the history
            # holds every token of a running row); the tokens come back with the accept counts
            # and the rows' next drafts in one read
            res, arows = self._spec_post(st, toks_d)
            toks = res[:, 2].astype(np.int64)
            if self.spec_proposer is None:
                self.r_nd[arows], self.r_drafts[arows] = res[:, 1], res[:, 3 + self.spec_k:]
            if lp_d is not None:
                lp = (lp_d[0].cpu().numpy(), lp_d[1].cpu().numpy())
                if st.nd is not None:  # per token -> per row (such a row has no drafts)
                    lp = (lp[0][st.q0], lp[1][st.q0])
        elif toks_d is not None:
            toks = toks_d.cpu().numpy().astype(np.int64)
            lp = None if lp_d is None else (lp_d[0].cpu().numpy(), lp_d[1].cpu().numpy())
        elif self.device.type == "cuda":
            torch.cuda.synchronize()
        t2 = time.perf_counter()
        B = st.B
        if st.nd is not None:
            self.stats["spec_accepted"] += int(res[:B, 0].sum()) - B
        if st.nd is not None and (res[:B, 0] != 1).any():
            out = self._spec_finish(st.rows, res[:B, 0], res[:B, 2:3 + self.spec_k], lp)
        else:
            out = self._decode_finish(st.rows, toks[:B], lp) if B else None
        if st.batch:
            p_out = self._chunks_done(st, [] if toks is None else toks[B:].tolist(), lp)
            if st.emb_out:  # (the step has executed: the tokens were read, or the device synchronised)
                p_out += self._deliver_embeds(st.emb_out)
            if out is None or p_out:
                p_out = StepBatch.from_list(p_out)
                out = p_out if out is None else StepBatch.concat(out, p_out)
        # host-side cost accounting (us): prep before launch, device (launch..tokens), bookkeeping
        t3 = time.perf_counter()
        if B and st.batch:
            self.stats["mixed_host_us"] += int(1e6 * (t1 - t0 + t3 - t2))
            self.stats["mixed_device_us"] += int(1e6 * (t2 - t1))
        elif B:
            self.stats["decode_host_prep_us"] += int(1e6 * (t1 - t0))
            self.stats["decode_device_us"] += int(1e6 * (t2 - t1))
            self.stats["decode_host_post_us"] += int(1e6 * (t3 - t2))
        return out

    def _chunks_done(self, st: _Step, tokens=None, lp=None) -> list:
        """The prompt chunks of a launched step: cached lengths, prefix pages, and the sequences
        whose prompt completed join the running rows.  ``tokens`` None: their first token is still
        in flight (one-step-ahead: the row registers count it, ``r_tokidx`` says where it will
        be); else those tokens (and ``lp``, the step's log-probabilities), applied at once: the
        StepOutputs are returned, and a sequence that ends with its first token never registers."""
        outs = []
        for s, c, d, e, ti in zip(st.batch, st.p_ctx, st.done, st.emb_done,
                                  itertools.accumulate(st.done, initial=st.B)):
            s.num_cached = c
            if self.cfg.enable_prefix_caching:
                self._register_prefix(s, c)
            if e:
                # an embedding's last chunk is launched: its pages (the registered ones stay cached) and
                # its row go back now, its slot when the vector is delivered (_deliver_embeds)
                self.prefilling.remove(s)
                st.emb_out.append((s, s.emb_slot, s.params.embed_dim or self.model.cfg.hidden_size))
                self._release(s)
            if not d:
                continue
            self.prefilling.remove(s)
            s.status = Status.RUNNING
            self.running.append(s)
            if tokens is None:  # (ti: the sequence's logits row in the step)
                self._register_running(s, in_flight=1)
                self.r_tokidx[s.row] = ti
                continue
            entry = None
            if lp is not None and s.params.logprobs is not None:
                entry = self._lp_entry(lp[0], lp[1], ti, s.params.logprobs)
                s.logprobs.append(entry)
            o = self._append(s, tokens[ti - st.B])
            if entry is not None:
                o.logprob, o.top_logprobs = entry
            if not o.finished:
                self._register_running(s)
            outs.append(o)
        return outs

    # ------------------------------------------------- async scheduling --
    # Step t+1 is built from the scheduler state as it stands after step t's LAUNCH: every
    # running row decodes again (a row whose step-t token turns out to be EOS / a stop token
    # is computed once more and its result dropped), its input id is gathered on the device
    # from step t's sampled tokens, and lengths / page needs are advanced at launch time (they
    # do not depend on token values).  Step t's tokens are read back (pinned copy + event,
    # so the read waits for step t only, never for the step queued behind it) and applied
    # after step t+1 is queued: the host's bookkeeping and the next step's preparation run
    # while the device computes, and the device never waits for the host between steps.
    # A row's results are stale once it was released (finish, abort, preemption): r_epoch.

    def _pending_alive(self) -> bool:
        p = self._pending
        if p is None:
            return False
        if any(s.status != Status.FINISHED for s, _, _ in p.emb):
            return True
        return bool(len(p.rows)) and bool((self.r_epoch[p.rows] == p.epochs).any())

    def _record_meta_ev(self):
        """One-step-ahead: the event behind this step's metadata H2D (and what else read the
        pinned host side); ``_wait_meta`` waits for it before the next step rewrites them."""
        if self._async and self.device.type == "cuda":
            self._meta_ev = torch.cuda.Event()
            self._meta_ev.record()

    def _wait_meta(self):
        """The previous step's metadata H2D has executed: the host buffers may be rewritten."""
        ev, self._meta_ev = self._meta_ev, None
        if ev is not None:
            ev.synchronize()

    def _async_step(self):
        prev, self._pending = self._pending, None
        if not self.running:
            # nothing decodes: finish the in-flight step (its finished rows free their slots),
            # then this step's prompt work runs as a synchronous prefill step
            out = self._async_post(prev) if prev is not None else StepBatch.from_list([])
            if self._want_prefill():
                p = self._sync_step(decode=False, prompt=True)
                if p is not None and len(p):
                    self._decode_since_prefill = 0
                    return "prefill", StepBatch.concat(out, p)
                if p is not None:
                    return "prefill", out
            return "idle", out
        kind, pend = "idle", None
        if self.running:
            self._wait_meta()
            if self._want_prefill():
                pend = self._async_launch(prev, mixed=True)
                if pend is not None:
                    kind = "mixed"
                    self._decode_since_prefill = 0
            if pend is None:
                self._decode_since_prefill += 1
                pend = self._async_launch(prev, mixed=False)
                kind = "decode" if pend is not None else kind
        self._pending = pend
        out = self._async_post(prev) if prev is not None else StepBatch.from_list([])
        return kind, out

    def _async_launch(self, prev, mixed: bool):
        """Build, launch and advance one step; returns its pending record (None: nothing to run)."""
        t0 = time.perf_counter()
        # decode input ids: on the device from the in-flight step, else the host's last token
        st = self._build_step(True, mixed, self.r_last if prev is None else self._ids_later)
        if st is None:
            return None
        rows, B = st.rows, st.B
        if prev is not None:
            self._src_h[:B].copy_(torch.from_numpy(self.r_tokidx[rows]))
            self._ids_gather = (B, prev.toks_d)
        toks_d, lp_d = self._issue(st)
        n = int(toks_d.shape[0])
        toks_h = self._toks_h[self._toks_flip][:n]
        lp_h = None
        if lp_d is not None:  # log-probabilities ride back beside the tokens, behind the same event
            if self._lp_h is None:
                size, pin = self.meta.max_tokens * (1 + MAX_LOGPROBS), self.device.type == "cuda"
                self._lp_h = [(torch.zeros(size, dtype=torch.float32, pin_memory=pin),
                               torch.zeros(size, dtype=torch.int32, pin_memory=pin)) for _ in range(2)]
            w = lp_d[0].shape[1]
            lp_h = tuple(h[:n * w].view(n, w) for h in self._lp_h[self._toks_flip])
        self._toks_flip ^= 1
        cuda = self.device.type == "cuda"
        toks_h.copy_(toks_d, non_blocking=cuda)
        if lp_h is not None:
            lp_h[0].copy_(lp_d[0], non_blocking=cuda)
            lp_h[1].copy_(lp_d[1], non_blocking=cuda)
        ev = None
        if cuda:
            ev = torch.cuda.Event()
            ev.record()
        # advance what does not depend on token values: decode rows gained a token (pending)
        seqs_d = list(self.running)  # aligned with rows (_decode_rows synced them)
        self.r_len[rows] += 1
        self.r_gen[rows] += 1
        self.r_tokidx[rows] = np.arange(B)
        self._chunks_done(st)
        pend = _Pending(st.srows, self.r_epoch[st.srows].copy(), seqs_d + st.done_seqs, toks_d, toks_h, ev,
                        None if lp_h is None else (lp_h[0], lp_h[1], self.r_want[st.srows].copy()), st.emb_out)
        self._retire_by_length(pend)
        self.stats["async_host_us"] += int(1e6 * (time.perf_counter() - t0))
        return pend

    def _keep_running(self, rows, keep) -> None:
        """Only the indices ``keep`` of the running set stay in it: ``running``, ``_outs`` and
        ``_rows`` (``rows``: the synced ``_rows``)."""
        run, outs = self.running, self._outs
        if len(keep) == 0:
            self.running, self._outs = [], []
        elif len(keep) == 1:
            self.running, self._outs = [run[keep[0]]], [outs[keep[0]]]
        else:
            get = operator.itemgetter(*keep.tolist())
            self.running, self._outs = list(get(run)), list(get(outs))
        self._rows = rows[keep]

    def _retire_by_length(self, pend):
        """Rows whose pending token is their last (max_tokens / max_model_len) leave the
        running set now; they finish when that token is applied."""
        rows = self._sync_rows()
        fin = (self.r_gen[rows] >= self.r_maxgen[rows]) | (self.r_len[rows] >= self.max_model_len)
        if not fin.any():
            return
        pend.retire = {self.running[i].seq_id for i in np.nonzero(fin)[0].tolist()}
        self._keep_running(rows, np.nonzero(~fin)[0])

    def _stop_mask(self, rows, toks, seqs) -> np.ndarray:
        """Per row: its new token is an EOS id the request does not ignore, or one of its stop tokens."""
        eos = self.model.cfg.eos_ids
        is_eos = (toks == eos[0]) if len(eos) == 1 else np.isin(toks, eos)
        fin_stop = (~self.r_ignore[rows]) & is_eos
        for i in np.nonzero(self.r_hasstop[rows])[0].tolist():
            if int(toks[i]) in seqs[i].params.stop_token_ids:
                fin_stop[i] = True
        return fin_stop

    def _async_post(self, pend) -> StepBatch:
        """Apply an in-flight step's tokens and deliver the embeddings it finished (waits for that
        step only: both came back behind its own event)."""
        out = self._async_post_tokens(pend)
        if pend.emb:
            e_out = self._deliver_embeds(pend.emb)
            if e_out:
                out = StepBatch.concat(out, StepBatch.from_list(e_out))
        return out

    def _async_post_tokens(self, pend) -> StepBatch:
        t0 = time.perf_counter()
        if pend.ev is not None:
            pend.ev.synchronize()
        rows = pend.rows
        n = len(rows)
        toks = pend.toks_h[:n].numpy().copy() if n else np.zeros(0, np.int64)
        lp = pend.lp
        if lp is not None:
            lp = (lp[0].numpy().copy(), lp[1].numpy().copy(), lp[2])
        alive = self.r_epoch[rows] == pend.epochs
        if not alive.all():
            ai = np.nonzero(alive)[0]
            rows, toks = rows[ai], toks[ai]
            seqs = [pend.seqs[i] for i in ai.tolist()]
            if lp is not None:  # a released row's log-probabilities go with its token
                lp = tuple(a[ai] for a in lp)
        else:
            seqs = pend.seqs
        if not len(rows):
            return StepBatch.from_list([])
        lps = self._deliver_lp(seqs, lp, lp[2]) if lp is not None else None
        now = time.perf_counter()
        for s in seqs:
            if s.first_token_time is None:
                s.first_token_time = now
        collections.deque(map(list.append, [s.output for s in seqs], toks.tolist()), maxlen=0)
        self.r_last[rows] = toks
        fin_stop = self._stop_mask(rows, toks, seqs)
        retire = pend.retire
        fin_len = np.zeros(len(rows), bool)
        if retire:
            fin_len = np.fromiter((s.seq_id in retire for s in seqs), dtype=bool, count=len(seqs))
        fin = fin_stop | fin_len
        sids = self.r_sid[rows].copy()
        reasons = {}
        fi = np.nonzero(fin)[0]
        if len(fi):
            done = [seqs[i] for i in fi.tolist()]
            stopped = set()
            for i, s in zip(fi.tolist(), done):
                reasons[s.seq_id] = "stop" if fin_stop[i] else "length"
                if s.seq_id not in retire:
                    stopped.add(s.seq_id)
            if stopped:  # still in the running set (speculatively decoding again)
                self.running = [s for s in self.running if s.seq_id not in stopped]
                self._rows_dirty = True
            for s in done:
                self._finish(s, reasons[s.seq_id])
        self.stats["async_host_us"] += int(1e6 * (time.perf_counter() - t0))
        return StepBatch(sids, toks, fin, reasons, lps)

    # ----------------------------------------------------------- decode --
    def _decode_rows(self):
        """Rows of the running batch with a KV slot for their next token: only rows
        crossing a page boundary allocate (vectorised test, Python only for those
        few); on exhaustion the newest sequence is preempted."""
        while True:
            rows = self._sync_rows()
            ctx = self.r_len[rows]
            if self._swa:
                # this step's query sits at ctx - 1; rows whose window start crossed a page pair
                # (once per 32 tokens per row) give back the pages below it
                first = (np.maximum(ctx - self.window, 0) & ~31) >> 4
                for i in np.nonzero(first > self.r_nrel[rows])[0].tolist():
                    self._release_window(self.running[i], int(ctx[i]) - 1)
            nblk = self.r_nblk[rows]
            want = (ctx + BLOCK_SIZE - 1) // BLOCK_SIZE
            need = np.nonzero(want > nblk)[0]
            if len(need) and self.alloc.can_allocate(len(need)) and (want[need] - nblk[need] == 1).all():
                # the steady-state case, vectorised: each crossing row takes exactly one page
                new = self.alloc.allocate(len(need))
                r = rows[need]
                self.meta.bt_h[r, nblk[need]] = new
                self.r_nblk[r] += 1
                run = self.running
                collections.deque(map(list.append, [run[i].blocks for i in need.tolist()], new), maxlen=0)
                return rows, ctx
            ok = True
            for i in need.tolist():
                s = self.running[i]
                # the row's length (async: it counts the in-flight step's token, s.length not yet)
                if not self._ensure_blocks(s, int(ctx[i])):
                    # an embedding sequence still in prefill is newer work than any running row: it
                    # restarts from token 0 (its next first chunk overwrites its slot) before a row does
                    victim = next((v for v in reversed(self.prefilling) if v.params.embed is not None), None)
                    if victim is not None:
                        self.prefilling.remove(victim)
                        self._preempt(victim)
                        ok = False
                        break
                    self._preempt(self.running.pop())  # newest goes back to the queue
                    self._rows = self._rows[:-1]
                    self._outs.pop()
                    ok = False
                    break
            if ok:
                return rows, ctx

    def _sync_rows(self) -> np.ndarray:
        """``self._rows`` brought in step with ``self.running`` (O(appended) per step; a
        full rebuild only after an out-of-band change such as an abort)."""
        if self._rows_dirty:
            run = self.running
            self._rows = np.fromiter((s.row for s in run), dtype=np.int32, count=len(run))
            self._outs = [s.output for s in run]
            self._rows_add.clear()
            self._rows_dirty = False
        elif self._rows_add:
            n = len(self._rows_add)
            self._rows = np.concatenate([self._rows, np.asarray(self._rows_add, dtype=np.int32)])
            self._outs.extend(s.output for s in self.running[-n:])
            self._rows_add.clear()
        return self._rows

    def _fill_tok_slot(self, T: int, d_rows, batch=(), chunks=()) -> None:
        """The step's adapter slot per token, in the metadata's token order: the decode rows, then
        each prompt chunk; graph padding rows get -1.  Leaves ``_step_lora`` = some row of the
        step uses an adapter (False: the step takes the adapter-free path, decode graphs included)."""
        self._step_lora = False
        if self.lora is None or not self._slot_refs.any():
            return
        ts = self._ts_hn
        t = len(d_rows)
        if t:
            ts[:t] = self.r_slot[d_rows]
        for s, n in zip(batch, chunks):
            ts[t:t + n] = s.slot
            t += n
        ts[t:T] = -1
        self._step_lora = bool((ts[:T] >= 0).any())

    # --------------------------------------------------------- adapters --
    def load_adapter(self, name: str, path) -> None:
        """Load the PEFT-format LoRA adapter in ``path`` into a free slot under ``name``; requests
        then select it with ``SamplingParams(adapter=name)``."""
        if self.lora is None:
            raise ValueError("this engine serves no adapters (EngineConfig.max_adapters = 0)")
        from ..models.loader import load_adapter

        self.add_adapter(name, load_adapter(path, self.model.cfg, self.cfg.max_lora_rank))

    def add_adapter(self, name: str, ad) -> None:
        """Install a ``models.lora.Adapter`` (already in our layout) under ``name``.  The copy into
        the slot runs on the engine's stream, behind every launched step."""
        if self.lora is None:
            raise ValueError("this engine serves no adapters (EngineConfig.max_adapters = 0)")
        if not isinstance(name, str) or not name:
            raise ValueError("adapter name must be a non-empty string")
        if name in self._adapters:
            raise ValueError(f"adapter {name!r} is already loaded (unload it first)")
        if not self._free_slots:
            raise ValueError(f"all {self.cfg.max_adapters} adapter slots are in use")
        slot = self._free_slots.pop()
        try:
            self.lora.load(slot, ad)
        except Exception:
            self.lora.clear(slot)
            self._free_slots.append(slot)
            raise
        import hashlib

        # prefix-cache identity: name + content, never the slot (a slot is reused)
        seed = hashlib.blake2b(b"lora\0" + name.encode() + b"\0" + ad.digest, digest_size=16).digest()
        self._adapters[name] = {"slot": slot, "seed": seed, "rank": ad.rank, "path": ad.path,
                                "target_modules": list(ad.target_modules)}

    def unload_adapter(self, name: str) -> None:
        """Free an adapter's slot; refused while a live sequence references it."""
        ad = self._adapters.get(name)
        if ad is None:
            raise ValueError(f"unknown adapter {name!r}")
        if self._slot_refs[ad["slot"]] > 0:
            raise RuntimeError(f"adapter {name!r} is in use by {int(self._slot_refs[ad['slot']])} live sequence(s)")
        self.lora.clear(ad["slot"])
        self._free_slots.append(ad["slot"])
        del self._adapters[name]

    def adapters(self) -> list:
        """The loaded adapters: [{name, slot, rank, target_modules, path}]."""
        return [{"name": n, **{k: v for k, v in a.items() if k != "seed"}} for n, a in self._adapters.items()]

    def _deliver_lp(self, seqs, lp, want) -> dict | None:
        """A step's log-probabilities onto the sequences that asked (``seqs`` aligned with the
        leading rows of ``lp``); returns seq_id -> entry for the step's StepBatch."""
        lps = {}
        for i in np.nonzero(want[:len(seqs)] >= 0)[0].tolist():
            entry = self._lp_entry(lp[0], lp[1], i, int(want[i]))
            seqs[i].logprobs.append(entry)
            lps[seqs[i].seq_id] = entry
        return lps or None

    def _decode_finish(self, rows, toks, lp=None) -> StepBatch:
        """Vectorised bookkeeping of one decode token per running row."""
        self.r_len[rows] += 1
        self.r_gen[rows] += 1
        self.r_last[rows] = toks
        fin_len = (self.r_gen[rows] >= self.r_maxgen[rows]) | (self.r_len[rows] >= self.max_model_len)
        run = self.running
        fin_stop = self._stop_mask(rows, toks, run)
        fin = fin_stop | fin_len
        # one token onto every running sequence's output list, at C speed
        collections.deque(map(list.append, self._outs, toks.tolist()), maxlen=0)
        lps = self._deliver_lp(run, lp, self.r_want[rows]) if lp is not None else None
        sids = self.r_sid[rows].copy()
        return StepBatch(sids, toks, fin, self._retire_rows(rows, fin, fin_stop), lps)

    def _retire_rows(self, rows, fin, fin_stop) -> dict:
        """The running rows flagged in ``fin`` finish ("stop" where ``fin_stop``, else "length") and
        leave the running set; returns seq_id -> reason."""
        run = self.running
        reasons = {}
        fi = np.nonzero(fin)[0]
        if len(fi):
            done = [run[i] for i in fi.tolist()]
            for i, s in zip(fi.tolist(), done):
                reasons[s.seq_id] = "stop" if fin_stop[i] else "length"
            self._keep_running(rows, np.nonzero(~fin)[0])
            for s in done:
                self._finish(s, reasons[s.seq_id])
        return reasons

    def _append(self, s: Sequence, tok: int) -> StepOutput:
        s.output.append(int(tok))
        if s.first_token_time is None:
            s.first_token_time = time.perf_counter()
        p = s.params
        reason = None
        if (not p.ignore_eos and tok in self.model.cfg.eos_ids) or tok in p.stop_token_ids:
            reason = "stop"
        elif len(s.output) >= p.max_tokens:
            reason = "length"
        elif s.length >= self.max_model_len:
            reason = "length"
        if reason:
            if s in self.running:
                self.running.remove(s)
            self._finish(s, reason)
        return StepOutput(s.seq_id, int(tok), reason is not None, reason)

    # --------------------------------------------------------- execution --
    def _launch(self, kind: int, T: int, nt: int, nl: int, part: int, nparts: int, bucket: int,
                greedy: bool = False):
        """Ship this step's metadata to the device and run it.  With tensor
        parallelism, rank 0 (the only rank that schedules) puts the step header in the
        packed metadata buffer and broadcasts it to the TP group in ONE collective
        (SURVEY §2.5 CL5); the other ranks run the same ``_execute`` from ``worker_loop``.
        Returns logits, or (TP, all-greedy rows) the chosen token ids already."""
        self._launched = True
        npt = self.meta.npt  # flash-prefill tiles of the metadata just filled
        if self.ep_sync is not None:
            kind, T, nt, nl, part, nparts, bucket = self._ep_agree(kind, T, nt, nl, part, nparts, bucket)
        self.meta.upload(T, nl, self.rows_hi)
        if self._step_lora:  # ahead of _meta_ev: the same event guards the pinned host side
            self._ts_d[:T].copy_(self._ts_h[:T], non_blocking=True)
        if self._step_pool is not None:  # the pool segments and finish rows, under the same event
            self._pool_d.copy_(self._pool_h, non_blocking=True)
        g = self._ids_gather
        if g is not None:
            # async: decode rows' input ids = the previous (in-flight) step's sampled tokens,
            # gathered on the device after the metadata H2D (which carried placeholders) and
            # before the TP broadcast of the buffer, so the workers receive the real ids
            self._ids_gather = None
            B, toks_d = g
            self._src_d[:B].copy_(self._src_h[:B], non_blocking=True)
            if toks_d.dtype == self.meta.ids_d.dtype and toks_d.dim() == 1:  # one gather kernel, no copy
                torch.index_select(toks_d, 0, self._src_d[:B], out=self.meta.ids_d[:B])
            else:
                self.meta.ids_d[:B].copy_(toks_d.index_select(0, self._src_d[:B]))
        if self.step_sync is not None:
            t0 = time.perf_counter()
            self.step_sync.send(self, kind, T, nt, nl, part, nparts, bucket, npt, int(greedy))
            self.stats["tp_sync_us"] += int(1e6 * (time.perf_counter() - t0))
            self.stats["tp_sync_calls"] += 1
        self._record_meta_ev()
        return self._execute(kind, T, nt, nl, part, nparts, bucket, npt, greedy)

    def _ep_agree(self, kind, T, nt, nl, part, nparts, bucket):
        """EP lock-step: the group's common step shape.  Someone eager -> everyone eager, MoE
        capacity = the group's largest token count (a graph-planned decode runs its padded
        rows eagerly); all graph -> everyone replays the largest agreed bucket (re-padded)."""
        any_work, eager, t_max, b_max = self.ep_sync.agree(1, int(kind == KIND_EAGER), T, bucket)
        if eager:
            if kind == KIND_GRAPH:
                rows, ctx, last, mctx = self._repad
                part, nparts = plan_partitions(T, self.model.n_kv, self.meta.span(mctx))
                kind, nt, nl = KIND_EAGER, T, T
            self.model.moe_capacity_tokens = t_max
            return kind, T, nt, nl, part, nparts, 0
        if b_max != bucket:
            rows, ctx, last, _ = self._repad
            self.meta.fill_decode(rows, ctx, last, pad_to=b_max)
            self.stats["ep_repadded_steps"] += 1
        return kind, b_max, b_max, b_max, part, nparts, b_max

    def _execute(self, kind, T, nt, nl, part, nparts, bucket, npt=0, greedy=0):
        if self._inject_device_us:  # fault injection: this step is slower on the device only
            torch.ops.mlop.device_delay(self._inject_device_us)
        lora = self._step_lora
        if lora:
            self.stats["lora_steps"] += 1
        if kind == KIND_GRAPH:
            family = self.graphs_spec if self._step_spec else self.graphs_lora if lora else self.graphs
            graph, logits_buf = family[bucket]
            graph.replay()
            if lora:
                self.stats["lora_graph_steps"] += 1
            return self._gather(logits_buf, greedy)
        meta = self.meta.meta(T, nt, nl, part, nparts, npt)
        if lora:
            hidden = self.model.forward(self.meta.ids_d[:T], meta, self.kv, lora=self.lora.step(self._ts_d[:T]))
        else:
            hidden = self.model.forward(self.meta.ids_d[:T], meta, self.kv)
        if self._step_pool is not None:  # embedding chunks: pooled before the LM head (and when nl == 0)
            self._pool_run(hidden)
        if nl == 0:
            return None
        return self._gather(self.model.logits_local(hidden[meta.logits_idx]), greedy)

    def _gather(self, local, greedy):
        """Vocab-parallel LM head -> what the sampler needs (CL3).  Greedy rows need only each
        rank's (max logit, its global index): an [n, 2] all-gather instead of the [n, V/TP]
        logits shard per rank (70B TP=8: 16 032 columns).  Ties keep the lowest vocabulary
        index, as an argmax over the full row does."""
        tp = self.model.ps.tp
        if tp.size == 1:
            return local
        if not greedy:
            return tp.all_gather(local, dim=-1)
        idx = ops.argmax(local) if local.is_cuda else local.argmax(-1)
        val = local.gather(1, idx.view(-1, 1)).float()
        pair = torch.cat([val, (idx.view(-1, 1) + self.model.vocab_start).float()], dim=1)  # [n, 2]
        allp = tp.all_gather(pair.contiguous(), dim=1).view(-1, tp.size, 2)  # [n, tp, 2]
        best = allp[:, :, 0].argmax(dim=1)  # first max: the lowest rank = the lowest vocab index
        return _Tokens(allp[torch.arange(allp.shape[0], device=allp.device), best, 1].to(torch.int64))

    def _sample(self, out, params, gen_index=None, rows=None):
        """Tokens of a step's logits rows.  ``rows``: the engine rows they belong to, in order; a
        row with a penalty or log-probabilities takes the sampler's extended path, whose
        log-probability tensors are left in ``self._last_lp`` for the caller to read back."""
        self._last_lp = None
        if isinstance(out, _Tokens):
            return out.ids
        if rows is not None and not getattr(params, "all_greedy", False):
            ext = self._ext_of(np.asarray(rows, dtype=np.int64))
            if ext is not None:
                toks, lp, ids = self.sampler.sample_ext(out, params, ext, gen_index)
                self._last_lp = None if lp is None else (lp, ids)
                return toks
        return self.sampler(out, params, gen_index)

    def _sample_rows(self, rows, done_seqs):
        """Engine rows of a step's logits rows: the decode rows, then the completed prompts."""
        if not done_seqs:
            return rows  # (``_rows`` as it stood: it is replaced, never written in place)
        return np.concatenate([rows, np.asarray([s.row for s in done_seqs], dtype=rows.dtype)])

    def _gen_index(self, rows, done_seqs):
        """Output position of each row's draw (seeded sampling): decode rows' generated count
        (it counts an in-flight token under async scheduling), then the prompts that completed."""
        return np.concatenate([self.r_gen[rows], np.asarray([len(s.output) for s in done_seqs], dtype=np.int64)])

    def worker_loop(self):
        """Non-zero TP ranks: replay rank 0's steps until it sends STOP."""
        assert self.step_sync is not None
        while True:
            hdr = self.step_sync.recv(self)
            if hdr[0] == KIND_STOP:
                return
            if hdr[0] == KIND_BARRIER:
                self._world_barrier()
                continue
            self._execute(*hdr)
            self._check_peers()
            self.stats["worker_steps"] += 1

    def sync_point(self):
        """Device sync + a barrier of the WHOLE world that the TP workers join too
        (they are parked in ``worker_loop``): the bench's timing brackets."""
        if self.step_sync is not None and self.step_sync.is_leader:
            self.step_sync.send(self, KIND_BARRIER, 0, 0, 0, 0, 0, 0)
        self._world_barrier()

    def _world_barrier(self):
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        import torch.distributed as dist

        if dist.is_initialized():
            dist.barrier()
            if self.device.type == "cuda":
                torch.cuda.synchronize(self.device)  # the barrier's own collective, on both sides

    def shutdown(self):
        if self.step_sync is not None and self.step_sync.is_leader:
            self.step_sync.send(self, KIND_STOP, 0, 0, 0, 0, 0, 0)

    # ----------------------------------------------------------- graphs --
    def capture_graphs(self):
        """Capture one decode graph per batch bucket (largest first, shared pool)."""
        m = self.model
        stream = torch.cuda.Stream(self.device)
        stream.wait_stream(torch.cuda.current_stream(self.device))
        self.graph_pool = torch.cuda.graph_pool_handle()
        empty = np.zeros(0, dtype=np.int32)
        t0 = time.perf_counter()
        verbose = False

        def capture(**kw):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.graph_pool, stream=stream):
                logits = m.logits_local(m.forward(ids, meta, self.kv, **kw))
            return g, logits

        with torch.cuda.stream(stream):
            for bi, b in enumerate(sorted(self.buckets, reverse=True)):
                self.meta.fill_decode(empty, empty, np.zeros(0, dtype=np.int64), pad_to=b)
                self.meta.upload(b, b)
                m.moe_capacity_tokens = b  # EP: every rank's graph of bucket b exchanges b rows
                part, nparts = plan_partitions(b, m.n_kv, self.meta.span(self.max_model_len))
                meta = self.meta.meta(b, b, b, part, nparts)
                ids = self.meta.ids_d[:b]
                # decode fills (fill_decode) give every row, padding included, its own logits row
                # in order: logits_idx is the identity, so the graph skips the row gather
                for _ in range(2 if bi == 0 else 1):  # warm-up (allocator, autotune, lazy init)
                    m.logits_local(m.forward(ids, meta, self.kv))
                stream.synchronize()
                if verbose:
                    print(f"[engine] capturing decode graph {bi + 1}/{len(self.buckets)} (batch {b}) "
                          f"at {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
                self.graphs[b] = capture()
                if self.lora is not None:
                    # second family: the LoRA forward of the same bucket, replayed by decode steps
                    # with an adapter row.  It reads tok_slot and the slot stacks through fixed
                    # pointers; captured with every row on the base model (-1)
                    self._ts_d[:b].fill_(-1)
                    step = self.lora.step(self._ts_d[:b])
                    m.logits_local(m.forward(ids, meta, self.kv, lora=step))
                    stream.synchronize()
                    self.graphs_lora[b] = capture(lora=step)
            for b in sorted(self.spec_buckets if self.spec_k else (), reverse=True):
                # third family: the verify step of bucket b, b (k + 1) tokens with a logits row
                # each (identity index, as above); captured on padding rows only
                T, nt, _ = self.meta.fill_verify(empty, empty, empty, [], pad_tokens=b * (self.spec_k + 1),
                                                 pad_tiles=b * self._spec_tpr)
                self.meta.upload(T, T)
                part, nparts = plan_partitions(nt, m.n_kv, self.meta.span(self.max_model_len))
                meta = self.meta.meta(T, nt, T, part, nparts)
                ids = self.meta.ids_d[:T]
                m.logits_local(m.forward(ids, meta, self.kv))
                stream.synchronize()
                self.graphs_spec[b] = capture()
        torch.cuda.current_stream(self.device).wait_stream(stream)
        torch.cuda.synchronize(self.device)
        self.stats["graph_capture_ms"] = int(1e3 * (time.perf_counter() - t0))

    # ------------------------------------------------------ offline API --
    def generate(self, prompts, params: SamplingParams | list | None = None):
        """Offline batch API.  EP group: EVERY rank calls it (each with its own prompts, maybe
        none) and the ranks keep stepping together until the whole group is done."""
        if not isinstance(params, list):
            params = [params or SamplingParams()] * len(prompts)
        seqs = [self.add_request(p, sp) for p, sp in zip(prompts, params)]
        if self.ep_sync is not None:
            while True:
                self.step()
                if self.ep_sync.last_busy == 0 and all(s.status == Status.FINISHED for s in seqs):
                    return [s.output for s in seqs]
        while any(s.status != Status.FINISHED for s in seqs):
            self.step()
        return [s.output for s in seqs]
