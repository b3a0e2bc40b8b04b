"""The wide MoE dispatch (moe_wide.hip, 128 experts) against the only other way this tree can compute
the same thing, and one decode / one prompt step of the Qwen3-30B-A3B shape (profiles/qwen3_moe.md).
One JSON line per measurement; the variants alternate round by round in one process.

  dispatch  ops.moe_dispatch_wide at H = 2048, k = 8, T = --tokens, against the baseline
            ``linear(x, router_w)`` + torch softmax / topk (+ renormalise) + ``ops.moe_permute``.
            Device events around --iters launches; best and slowest of --rounds rounds.
  engine    --seqs sequences of --prompt / --gen tokens through a random-init engine of
            qwen3-30b-a3b's shapes at --layers layers: prompt tok/s (one --prompt-token step per
            sequence) and decode tok/s (graph steps of --seqs rows).

``--md FILE`` appends this run's table, as markdown, to FILE.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlopamd import ops  # noqa: E402
from mlopamd.models.layers import linear  # noqa: E402

ops.load()
dev = torch.device("cuda", 0)
bf = torch.bfloat16
E, H, K = 128, 2048, 8


def timeit(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def md_append(path, title, header, rows):
    if not path:
        return
    lines = [f"\n{title}\n", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)]
    lines += ["| " + " | ".join(str(c) for c in r) + " |" for r in rows]
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


def bench_dispatch(args):
    torch.manual_seed(0)
    wr = (0.05 * torch.randn(E, H, device=dev)).to(bf)
    table = []
    for T in (int(t) for t in args.tokens.split(",")):
        x = torch.randn(T, H, device=dev, dtype=bf)

        def baseline():
            p = torch.softmax(linear(x, wr).float(), -1)
            w, i = torch.topk(p, K, dim=-1)
            w = w / w.sum(-1, keepdim=True)
            return w, ops.moe_permute(x, i.to(torch.int32), 0, E)

        runs = {"wide": lambda: ops.moe_dispatch_wide(x, wr, K, 0, E), "route_only": lambda: ops.moe_route_wide(x, wr, K),
                "baseline": baseline}
        # same function (reported, not asserted: a logit whose fp32 sum rounds to the other bf16
        # neighbour under the other summation order moves its weight by up to 2^-8 |logit|)
        diff = float((ops.moe_route_wide(x, wr, K)[0] - baseline()[0]).abs().max())
        print(json.dumps(dict(bench="dispatch", tokens=T, max_weight_diff_vs_baseline=round(diff, 5))), flush=True)
        times = {n: [] for n in runs}
        for _ in range(args.rounds):
            for n, fn in runs.items():
                times[n].append(timeit(fn, args.iters))
        for n, ts in times.items():
            print(json.dumps(dict(bench="dispatch", variant=n, tokens=T, us=round(min(ts), 2),
                                  us_rounds=[round(v, 2) for v in ts])), flush=True)
        best = {n: min(ts) for n, ts in times.items()}
        table.append([T] + [f"{best[n]:.2f} ({max(times[n]):.2f})" for n in runs] +
                     [f"{best['baseline'] / best['wide']:.2f}x"])
    md_append(args.md, f"dispatch, H = {H}, E = {E}, k = {K}; us per call: best of {args.rounds} rounds (slowest round)",
              ["tokens", *runs, "baseline / wide"], table)


def bench_engine(args):
    from mlopamd.models import build_model
    from mlopamd.models.config import get_config
    from mlopamd.runtime.engine import Engine, EngineConfig, Status
    from mlopamd.runtime.sampler import SamplingParams

    cfg = get_config("qwen3-30b-a3b", num_layers=args.layers)
    model = build_model(cfg, device=dev)
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, cfg.vocab_size - 1, (args.prompt,), generator=g).tolist() for _ in range(args.seqs)]
    rows = []
    for rnd in range(args.rounds):
        eng = Engine(model, EngineConfig(max_num_seqs=args.seqs, max_num_batched_tokens=args.prompt,
                                         max_model_len=args.prompt + args.gen + 16, kv_cache_bytes=int(8e9),
                                         kv_fraction=1.0, graph_buckets=(args.seqs,), enable_prefix_caching=False))
        eng.kv.wait_ready()
        seqs = [eng.add_request(p, SamplingParams(max_tokens=args.gen, ignore_eos=True)) for p in prompts]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        while any(s.status in (Status.WAITING, Status.PREFILL) for s in seqs):
            eng.step()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        n1 = sum(len(s.output) for s in seqs)
        steps0 = eng.stats["graph_steps"]
        while any(s.status != Status.FINISHED for s in seqs):
            eng.step()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        r = dict(bench="engine", round=rnd, layers=cfg.num_layers, seqs=args.seqs, prompt=args.prompt, gen=args.gen,
                 prompt_step_ms=round((t1 - t0) / args.seqs * 1e3, 3),
                 decode_step_ms=round((t2 - t1) / max(1, (args.seqs * args.gen - n1) / args.seqs) * 1e3, 3),
                 graph_steps=eng.stats["graph_steps"] - steps0)
        print(json.dumps(r), flush=True)
        rows.append(r)
        del eng, seqs
        torch.cuda.empty_cache()
    md_append(args.md, f"engine, qwen3-30b-a3b shapes at {cfg.num_layers} layers, batch {args.seqs}, {args.prompt}-token "
                       f"prompt steps, {args.gen} decode steps: ms per step, best of {args.rounds} rounds (all rounds)",
              ["step", "ms"],
              [[k, f"{min(r[k] for r in rows)} ({' / '.join(str(r[k]) for r in rows)})"]
               for k in ("prompt_step_ms", "decode_step_ms")])


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("what", choices=["dispatch", "engine"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=200, help="dispatch: calls per timing")
ap.add_argument("--tokens", default="1,16,64,1024,4096", help="dispatch: token counts")
ap.add_argument("--seqs", type=int, default=1)
ap.add_argument("--prompt", type=int, default=2048)
ap.add_argument("--gen", type=int, default=64)
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--md", default=None, help="append this run's table to a markdown file")
a = ap.parse_args()
{"dispatch": bench_dispatch, "engine": bench_engine}[a.what](a)
