"""Speculative decoding by prompt lookup at the Llama-3-8B shapes (random weights), one GPU.

Three measurements, one JSON line each; results: profiles/spec_decode.md.

``steps``: seconds per plain graph decode step (spec_tokens = 0) against seconds per verify step at
k in --k, batches --batches, context --ctx.  A hook forces nd = k drafts (wrong ones: a step's
cost does not depend on acceptance, and the context then grows one token per step on both sides).
Host clock around a window of steps that ends in a device synchronise; the engines take turns
round by round (interleaved), min / median / max over the rounds are reported.

``kernels``: ``ops.spec_accept`` and ``ops.spec_propose`` alone, device events.

``e2e``: generated tok/s of the decode phase with a replay proposer: recorded tokens with each
draft corrupted at a rate that gives about 30 / 60 / 90 % accepted drafts, against spec-off on the
same box, alternating.  What is replayed is the path of the SAME engine (same k, same batch) under
an always-wrong proposer, not the spec-off engine's: a verify graph runs its GEMMs at bucket x
(k + 1) rows whatever the rows draft, so its logits differ from a decode graph's in the last bits
and on random weights (near-flat logits) the two paths part within a few tokens, while the
verify path itself does not depend on which drafts were right.  It can still be left where rows
finish at different times and the batch drops to a smaller bucket; the proposer then has nothing
to replay, and the acceptance actually reached is reported beside each target."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlopamd import ops  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--layers", type=int, default=None, help="fewer layers (rehearsal)")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 2, 4, 8, 16])
ap.add_argument("--k", type=int, nargs="+", default=[1, 2, 3, 4, 5, 7])
ap.add_argument("--ctx", type=int, default=512)
ap.add_argument("--gen", type=int, default=128)
ap.add_argument("--steps", type=int, default=40, help="steps per timed window")
ap.add_argument("--rounds", type=int, default=4, help="rounds (the first one warms up)")
ap.add_argument("--rates", type=float, nargs="+", default=[0.3, 0.6, 0.9])
ap.add_argument("--only", nargs="+", default=["steps", "kernels", "e2e"])
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_spec.py measures on the GPU only")
ops.load()
dev = torch.device("cuda", 0)

from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import get_config  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig, Status  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402
from mlopamd.runtime.spec import out_width  # noqa: E402


def emit(**kw):
    print(json.dumps(kw), flush=True)


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


kw = {} if args.layers is None else {"num_layers": args.layers}
cfg = get_config(args.model, **kw)
model = build_model(cfg, device=dev)
V = cfg.vocab_size
BMAX = max(args.batches)
MAXLEN = args.ctx + max(args.gen, args.steps * (args.rounds + 1)) + 64


def engine(k):
    return Engine(model, EngineConfig(max_num_seqs=BMAX, max_num_batched_tokens=max(2048, args.ctx), max_model_len=MAXLEN,
                                      num_kv_blocks=BMAX * (MAXLEN // 16 + 2) + 8, graph_buckets=tuple(args.batches),
                                      enable_prefix_caching=False, spec_tokens=k, spec_max_batch=BMAX))


engines = {k: engine(k) for k in [0, *args.k]}
g = torch.Generator().manual_seed(1)
PROMPTS = [torch.randint(1000, V - 1000, (args.ctx,), generator=g).tolist() for _ in range(BMAX)]


def start(eng, b, max_tokens):
    """b requests prefilled and decoding."""
    seqs = [eng.add_request(p, SamplingParams(max_tokens=max_tokens, ignore_eos=True)) for p in PROMPTS[:b]]
    while any(s.status != Status.RUNNING for s in seqs):
        eng.step()
    return seqs


def stop(eng, seqs):
    for s in seqs:
        eng.abort(s.seq_id)
    while eng.has_work():
        eng.step()


def window(eng, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        eng.step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n


def bench_steps():
    for b in args.batches:
        live = {}
        for k, eng in engines.items():
            eng.spec_proposer = (lambda seq, cap: [7] * cap) if k else None  # nd = cap = k, never accepted
            live[k] = start(eng, b, MAXLEN)
        times = {k: [] for k in engines}
        for rnd in range(args.rounds):
            for k, eng in engines.items():
                before = dict(eng.stats)
                dt = window(eng, args.steps)
                if rnd:
                    times[k].append(dt)
                    key = "spec_graph_steps" if k else "graph_steps"
                    assert eng.stats[key] - before.get(key, 0) == args.steps, (k, key, "the window left the graph path")
        base = statistics.median(times[0])
        for k in engines:
            s = spread(times[k])
            emit(what="step", batch=b, k=k, ctx=args.ctx, us={n: round(v * 1e6, 1) for n, v in s.items()},
                 rounds=len(times[k]), steps=args.steps,
                 **({"break_even_tokens_per_step": round(s["median"] / base, 3)} if k else {}))
        for k, eng in engines.items():
            stop(eng, live[k])
            eng.spec_proposer = None


def bench_kernels():
    for k in args.k:
        W = out_width(k)
        for b in args.batches:
            for L in (args.ctx, 4096):
                hist = torch.randint(0, 64, (BMAX, max(L, 4096) + 64), dtype=torch.int32, device=dev)
                hlen = torch.full((BMAX,), L, dtype=torch.int32, device=dev)
                i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)  # noqa: E731
                rows, cap, nd = i32(list(range(b))), i32([k] * b), i32([k] * b)
                q0 = i32([i * (k + 1) for i in range(b)])
                drafts = torch.randint(0, 64, (b, k), dtype=torch.int32, device=dev)
                sampled = torch.randint(0, 64, (b * (k + 1),), dtype=torch.int64, device=dev)
                out = torch.zeros(b, W, dtype=torch.int32, device=dev)
                res = {}

                def accept():
                    hlen.fill_(L)
                    ops.spec_accept(sampled, q0, drafts, nd, rows, hist, hlen, out)

                for name, fn in (("fill", lambda: hlen.fill_(L)), ("fill+accept", accept),
                                 ("propose", lambda: ops.spec_propose(hist, hlen, rows, cap, 3, 1, out))):
                    for _ in range(5):
                        fn()
                    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    s.record()
                    for _ in range(200):
                        fn()
                    e.record()
                    torch.cuda.synchronize()
                    res[name] = round(s.elapsed_time(e) / 200 * 1e3, 2)
                emit(what="kernel", k=k, batch=b, hist_len=L, accept_us=round(res["fill+accept"] - res["fill"], 2),
                     propose_us=res["propose"])


def iid_rate(target, k):
    """P(a draft token is right), independent per token, that makes E[accepted] / k = target."""
    lo, hi = 0.0, 1.0
    for _ in range(40):
        q = (lo + hi) / 2
        acc = sum(q ** j for j in range(1, k + 1)) / k
        lo, hi = (q, hi) if acc < target else (lo, q)
    return (lo + hi) / 2


def decode_run(eng, b):
    """(decode-phase seconds, tokens it generated, outputs) of b requests of --gen tokens."""
    seqs = start(eng, b, args.gen)
    torch.cuda.synchronize()
    n0 = sum(len(s.output) for s in seqs)
    t0 = time.perf_counter()
    while eng.has_work():
        eng.step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return dt, sum(len(s.output) for s in seqs) - n0, [s.output for s in seqs]


def bench_e2e():
    off = engines[0]
    for b in args.batches:
        decode_run(off, b)  # warm
        refs = {}
        for k in args.k:  # the verify path of (b, k): every step drafts k wrong tokens
            engines[k].spec_proposer = lambda seq, cap: [7] * cap
            _, _, outs = decode_run(engines[k], b)
            engines[k].spec_proposer = None
            refs[k] = {tuple(p): o for p, o in zip(PROMPTS, outs)}
        runs = [(0, None)] + [(k, r) for k in args.k for r in args.rates]
        rates = {run: [] for run in runs}
        acc = {run: [] for run in runs}
        for rnd in range(args.rounds):
            for run in runs:
                k, target = run
                eng = engines[k]
                if k:
                    q = iid_rate(target, k)
                    rng = np.random.default_rng(1000 * rnd + k)

                    def propose(seq, cap, q=q, rng=rng, ref=refs[k]):
                        r, n = ref[tuple(seq.prompt)], len(seq.output)
                        if seq.output != r[:n]:
                            return []  # left the recorded path: nothing to replay
                        d = r[n:n + cap]
                        bad = rng.random(len(d)) >= q
                        return [(t + 1) % V if x else t for t, x in zip(d, bad)]

                    eng.spec_proposer = propose
                before = dict(eng.stats)
                dt, n, _ = decode_run(eng, b)
                eng.spec_proposer = None
                if rnd:
                    rates[run].append(n / dt)
                    dr = eng.stats["spec_drafted"] - before.get("spec_drafted", 0) if k else 0
                    acc[run].append((eng.stats["spec_accepted"] - before.get("spec_accepted", 0)) / dr if dr else 0.0)
        base = statistics.median(rates[(0, None)])
        for run in runs:
            k, target = run
            s = spread(rates[run])
            emit(what="e2e", batch=b, k=k, target_acceptance=target, ctx=args.ctx, gen=args.gen,
                 tok_s={n: round(v, 1) for n, v in s.items()}, rounds=len(rates[run]),
                 **({"acceptance": round(statistics.mean(acc[run]), 3), "vs_off": round(s["median"] / base, 3)} if k else {}))


emit(what="setup", model=cfg.name, layers=cfg.num_layers, batches=args.batches, k=args.k, ctx=args.ctx,
     device=torch.cuda.get_device_name(0))
if "steps" in args.only:
    bench_steps()
if "kernels" in args.only:
    bench_kernels()
if "e2e" in args.only:
    bench_e2e()
