"""Guided decoding at the Llama-3-8B shapes (random weights), one GPU.  One JSON line per
measurement; results: profiles/guided_decoding.md.

``steps``: seconds per graph decode step at batches --batches with 0 %, 50 % and 100 % guided rows,
for a small grammar (a 3-way choice, repeated) and a JSON grammar of about 500 states, greedy and
at temperature 0.8.  Host clock around a window of steps that ends in a device synchronise; the
mixes take turns round by round (interleaved) inside one engine, min / median / max over the
rounds are reported.  The benchmark grammars are unbounded (a member, a separator, a member, ...)
and their EOS entries are removed from the host table before the upload, so a guided row decodes
for as long as the window lasts.  ``--baseline`` measures the unguided mixes only and needs no
guided feature: run from a checkout of the parent commit (``--repo``) in alternation with this
tree it gives the parent's step on the same box.

``kernels``: ``ops.grammar_mask`` and ``ops.grammar_advance`` alone at (n, V) = (1, 128256) and
(64, 128256), device events.

``compile``: host seconds to compile each grammar over a byte vocabulary and over a synthetic
128k-token vocabulary (every byte plus random 2..12-byte ASCII tokens)."""
import argparse
import json
import os
import random
import statistics
import sys
import time

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                help="the checkout whose mlopamd package is measured")
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--layers", type=int, default=None, help="fewer layers (rehearsal)")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 16, 64])
ap.add_argument("--fracs", type=float, nargs="+", default=[0.0, 0.5, 1.0])
ap.add_argument("--temps", type=float, nargs="+", default=[0.0, 0.8])
ap.add_argument("--ctx", type=int, default=128)
ap.add_argument("--steps", type=int, default=40, help="steps per timed window")
ap.add_argument("--rounds", type=int, default=4, help="rounds (the first one warms up)")
ap.add_argument("--states", type=int, default=4096, help="EngineConfig.grammar_states")
ap.add_argument("--baseline", action="store_true", help="unguided mixes only, no guided feature needed")
ap.add_argument("--tag", default="", help="copied into every JSON line")
ap.add_argument("--only", nargs="+", default=["compile", "kernels", "steps"])
args = ap.parse_args()
sys.path.insert(0, args.repo)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from mlopamd import ops  # noqa: E402


def emit(**kw):
    print(json.dumps({**({"tag": args.tag} if args.tag else {}), **kw}), flush=True)


def spread(xs):
    return {"min": min(xs), "median": statistics.median(xs), "max": max(xs)}


WORDS = {"regex": "(?:yes|no|maybe)(?: (?:yes|no|maybe))*"}
SCHEMA = {"type": "object", "properties": {
    "id": {"type": "string", "pattern": "[A-Z]{3}-[0-9]{6}"}, "name": {"type": "string", "maxLength": 10},
    "email": {"type": "string", "maxLength": 12}, "age": {"type": "integer"}, "score": {"type": "number"},
    "tags": {"type": "array", "items": {"enum": ["new", "vip", "trial", "churned"]}, "maxItems": 4},
    "address": {"type": "object", "properties": {"city": {"type": "string", "maxLength": 6},
                                                 "zip": {"type": "string", "pattern": "[0-9]{5}"}}},
    "active": {"type": "boolean"}}}


def grammars():
    from mlopamd.runtime import guided

    return {"choice": WORDS, "json": {"regex": "(?:" + guided.schema_to_regex(SCHEMA) + "\\n)+"}}


def bench_compile():
    from mlopamd.runtime import guided
    from mlopamd.runtime.backends import ByteTokenizer

    rnd = random.Random(0)
    alphabet = b"abcdefghijklmnopqrstuvwxyzABCDEFGHIJ0123456789 {}[]\":,.-_\n"
    V = 128256
    big = [None] * 3 + [bytes([b]) for b in range(256)]
    big += [bytes(rnd.choices(alphabet, k=rnd.randint(2, 12))) for _ in range(128000 - len(big))]
    big += [None] * (V - len(big))
    vocabs = {"bytes": guided.token_bytes(ByteTokenizer(), V), "synthetic128k": big}
    for gname, spec in grammars().items():
        for vname, tb in vocabs.items():
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                g = guided.compile(spec, tb, [128001])
                ts.append(time.perf_counter() - t0)
            emit(what="compile", grammar=gname, vocab=vname, states=g.num_states,
                 table_mb=round(g.next.nbytes / 2**20, 1), seconds={k: round(v, 3) for k, v in spread(ts).items()})


def bench_kernels():
    from mlopamd.runtime import guided
    from mlopamd.runtime.backends import ByteTokenizer

    dev = torch.device("cuda", 0)
    V = 128256
    g = guided.compile(grammars()["json"], guided.token_bytes(ByteTokenizer(), V), [128001])
    S = g.num_states
    arena = ops.grammar_arena(S + 8, V, dev)
    arena[8:8 + S, :V].copy_(torch.from_numpy(g.next))
    for n in (1, 64):
        logits = torch.randn(n, V, device=dev)
        i32 = lambda a: torch.tensor(a, dtype=torch.int32, device=dev)  # noqa: E731
        base, rows = i32([8] * n), i32(list(range(n)))
        state0 = i32([(7 * i) % (S - 1) for i in range(n)])
        state = state0.clone()
        toks = torch.randint(3, 259, (n,), device=dev)
        work = logits.clone()
        res = {}
        for name, fn in (("copy", lambda: work.copy_(logits)),
                         ("copy+mask", lambda: (work.copy_(logits), ops.grammar_mask(work, arena, base, rows, state))),
                         ("advance", lambda: ops.grammar_advance(arena, base, rows, state, toks, V))):
            for _ in range(5):
                fn()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            s.record()
            for _ in range(200):
                fn()
            e.record()
            torch.cuda.synchronize()
            res[name] = s.elapsed_time(e) / 200 * 1e3
        allowed = float((g.next[state0.cpu().numpy() % S] >= 0).mean())
        emit(what="kernel", n=n, V=V, states=S, allowed_fraction=round(allowed, 5),
             mask_us=round(res["copy+mask"] - res["copy"], 2), copy_us=round(res["copy"], 2),
             advance_us=round(res["advance"], 2))


def bench_steps():
    from mlopamd.models import build_model
    from mlopamd.models.config import get_config
    from mlopamd.runtime.engine import Engine, EngineConfig, Status
    from mlopamd.runtime.sampler import SamplingParams

    dev = torch.device("cuda", 0)
    cfg = get_config(args.model, **({} if args.layers is None else {"num_layers": args.layers}))
    model = build_model(cfg, device=dev)
    V, BMAX = cfg.vocab_size, max(args.batches)
    maxlen = args.ctx + args.steps * (args.rounds + 1) + 64
    kw = {} if args.baseline else {"grammar_states": args.states}
    eng = Engine(model, EngineConfig(max_num_seqs=BMAX, max_num_batched_tokens=max(2048, args.ctx), max_model_len=maxlen,
                                     num_kv_blocks=BMAX * (maxlen // 16 + 2) + 8, graph_buckets=tuple(args.batches),
                                     enable_prefix_caching=False, **kw))
    specs = {}
    if not args.baseline:
        from mlopamd.runtime.backends import ByteTokenizer

        eng.set_tokenizer(ByteTokenizer())
        for name, spec in grammars().items():
            g = eng.compile_guided(SamplingParams(guided=spec))
            g.next[:-1, list(cfg.eos_ids)] = -1  # never ends: the rows decode for the whole window
            specs[name] = spec
        emit(what="engine", grammar_arena_bytes=eng.stats["grammar_arena_bytes"],
             states={n: eng.compile_guided(SamplingParams(guided=s)).num_states for n, s in specs.items()})
    gen = torch.Generator().manual_seed(1)
    prompts = [torch.randint(1000, V - 1000, (args.ctx,), generator=gen).tolist() for _ in range(BMAX)]

    def window(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            eng.step()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    for b in args.batches:
        for T in args.temps:
            mixes = [("none", 0)]
            if not args.baseline:
                for name in specs:
                    for f in args.fracs:
                        ng = int(round(b * f))
                        if ng and (name, ng) not in mixes:
                            mixes.append((name, ng))
            times = {m: [] for m in mixes}
            for rnd in range(args.rounds):
                for m in mixes:  # interleaved: every mix once per round
                    name, ng = m
                    samp = dict(temperature=T, seed=3) if T > 0 else {}
                    seqs = [eng.add_request(p, SamplingParams(max_tokens=maxlen, ignore_eos=i >= ng,
                                                              guided=specs[name] if i < ng else None, **samp)
                                            if not args.baseline else
                                            SamplingParams(max_tokens=maxlen, ignore_eos=True, **samp))
                            for i, p in enumerate(prompts[:b])]
                    while any(s.status != Status.RUNNING for s in seqs):
                        eng.step()
                    before = dict(eng.stats)
                    dt = window(args.steps)
                    assert eng.stats["graph_steps"] - before.get("graph_steps", 0) == args.steps, "left the graph path"
                    if not args.baseline:
                        assert (eng.stats["guided_rows"] - before.get("guided_rows", 0) > 0) == (ng > 0)
                    if rnd:
                        times[m].append(dt)
                    for s in seqs:
                        eng.abort(s.seq_id)
                    while eng.has_work():
                        eng.step()
            base = statistics.median(times[mixes[0]])
            for (name, ng), ts in times.items():
                s = spread(ts)
                emit(what="step", batch=b, temperature=T, grammar=name, guided_rows=ng, ctx=args.ctx,
                     us={k: round(v * 1e6, 1) for k, v in s.items()}, rounds=len(ts), steps=args.steps,
                     ratio_to_unguided=round(s["median"] / base, 4))


if "compile" in args.only:
    bench_compile()
if {"kernels", "steps"} & set(args.only):
    if not torch.cuda.is_available():
        raise SystemExit("bench_guided.py measures kernels and steps on the GPU only")
    ops.load()
    if "kernels" in args.only:
        bench_kernels()
    if "steps" in args.only:
        bench_steps()
