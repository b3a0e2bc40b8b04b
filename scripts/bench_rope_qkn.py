"""The QK-norm RoPE + KV writers (rope_cache_qkn.hip) against the plain writers at the same shapes,
and a QK-norm engine against a Llama engine on the same unfused route (profiles/qwen3.md).  One
JSON line per measurement; the variants alternate round by round in one process.

  writer   RoPE + cache write of T tokens (Hq = 32, Hkv = 8): rope_cache / rope_cache_fp8 and the
           same launches with q_norm / k_norm.  Bytes moved per token are the same for a pair (the
           two 256-B weights aside), so the difference is the norm's arithmetic and its lane map.
  engine   --seqs sequences of --prompt / --gen tokens through three random-init engines of
           --model's shapes (qwen3-8b, or llama3-8b): "fused" has qk_norm off (the QKV epilogues
           and the norm chain, the Llama route), "qkn" has it on (plain QKV GEMM + the QK-norm
           writer, no chain), and "unfused" is qkn's route with the plain writer in place of the
           QK-norm one.  fused vs unfused is the cost of leaving the fused epilogues and the chain,
           unfused vs qkn the cost of the norm itself.  Batch 1 and batch 64 are --seqs 1 / 64.

The headline's mixed load (2048 requests in steady state, prompt chunks beside decode rows) is not
a mode of this script: it is ``python bench.py --gpus 1 --model qwen3-8b``, next to the same
command without --model on the same box.  ``--md FILE`` appends this run's table, as markdown, to
FILE (profiles/qwen3.md is made of such tables).
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlopamd import ops  # noqa: E402

ops.load()
dev = torch.device("cuda", 0)
bf = torch.bfloat16
Hq, Hkv, D = 32, 8, 128


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
    """Append a markdown table to ``path`` (--md)."""
    if not path:
        return
    lines = [f"\n{title}\n", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)]
    lines += ["| " + " | ".join(str(c) for c in r) + " |" for r in rows]
    with open(path, "a") as f:
        f.write("\n".join(lines) + "\n")


def bench_writer(args):
    table = []
    for T in (int(t) for t in args.tokens.split(",")):
        NB = T // 16 + 64
        qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=dev).to(bf)
        pos = torch.randint(0, 1024, (T,), device=dev, dtype=torch.int32)
        slots = (torch.randperm((NB - 1) * 16, device=dev)[:T] + 16).to(torch.int32)
        cs = torch.randn(1024, D, device=dev)
        kb, vb = (torch.zeros(NB, Hkv, 16, D, device=dev, dtype=bf) for _ in range(2))
        k8, v8 = (torch.zeros(NB, Hkv, 16, D, dtype=torch.uint8, device=dev).view(ops.ref.FP8) for _ in range(2))
        ks, vs = (torch.zeros(NB, Hkv, 16, dtype=torch.uint8, device=dev) for _ in range(2))
        q = torch.empty(T, Hq, D, device=dev, dtype=bf)
        qw, kw = (1 + 0.1 * torch.randn(D, device=dev)).to(bf), (1 + 0.1 * torch.randn(D, device=dev)).to(bf)
        n = dict(q_norm=qw, k_norm=kw, eps=1e-6)
        f8 = dict(k_scale=ks, v_scale=vs)
        runs = {"bf16": lambda: ops.rope_cache(qkv, pos, cs, slots, kb, vb, Hq, q_out=q),
                "bf16_qkn": lambda: ops.rope_cache(qkv, pos, cs, slots, kb, vb, Hq, q_out=q, **n),
                "fp8": lambda: ops.rope_cache(qkv, pos, cs, slots, k8, v8, Hq, q_out=q, **f8),
                "fp8_qkn": lambda: ops.rope_cache(qkv, pos, cs, slots, k8, v8, Hq, q_out=q, **f8, **n)}
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for k, fn in runs.items():
                times[k].append(timeit(fn, args.iters))
        # bytes the launch must move: the qkv row in, q and K / V rows out (fp8: 1 byte + scales)
        for k, ts in times.items():
            kv_bytes = 2 * Hkv * ((D + 1) if k.startswith("fp8") else 2 * D)
            nbytes = T * ((Hq + 2 * Hkv) * D * 2 + Hq * D * 2 + kv_bytes)
            s = sorted(ts)
            print(json.dumps(dict(bench="writer", variant=k, tokens=T, us=round(s[0], 2),
                                  us_median=round(s[len(s) // 2], 2), us_rounds=[round(x, 2) for x in ts],
                                  gb_s=round(nbytes / s[0] / 1e3, 1))), flush=True)
        best = {k: min(ts) for k, ts in times.items()}
        table.append([T] + [f"{best[k]:.2f} ({max(times[k]):.2f})" for k in runs] +
                     [f"{best['bf16_qkn'] / best['bf16']:.2f}", f"{best['fp8_qkn'] / best['fp8']:.2f}"])
    md_append(args.md, f"writer, us per launch: best of {args.rounds} rounds (slowest round)",
              ["tokens", *runs, "bf16 ratio", "fp8 ratio"], table)


def bench_engine(args):
    from mlopamd.models import build_model
    from mlopamd.models.config import get_config
    from mlopamd.runtime.engine import Engine, EngineConfig, Status
    from mlopamd.runtime.sampler import SamplingParams

    base = get_config(args.model, **({"num_layers": args.layers} if args.layers else {}))
    qkn_cfg = dataclasses.replace(base, qk_norm=True)
    models = {"fused": build_model(dataclasses.replace(base, qk_norm=False), device=dev),
              "qkn": build_model(qkn_cfg, device=dev)}
    # "unfused": the QK-norm model's route with the plain writers (what the norm itself costs)
    models["unfused"] = models["qkn"]
    plain = ops.rope_cache

    def no_norm(*a, q_norm=None, k_norm=None, eps=0.0, **kw):
        return plain(*a, **kw)

    max_len = args.prompt + args.gen + 16
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, base.vocab_size - 1, (args.prompt,), generator=g).tolist() for _ in range(args.seqs)]
    res = {name: [] for name in models}
    for rnd in range(args.rounds):
        for name, model in models.items():
            ops.rope_cache = no_norm if name == "unfused" else plain
            try:
                eng = Engine(model, EngineConfig(max_num_seqs=args.seqs, max_num_batched_tokens=args.chunk,
                                                 max_model_len=max_len, kv_cache_bytes=int(args.kv_gb * 1e9),
                                                 kv_fraction=1.0, graph_buckets=(args.seqs,),
                                                 enable_prefix_caching=False))
                eng.kv.wait_ready()
                seqs = [eng.add_request(p, SamplingParams(max_tokens=args.gen, ignore_eos=True)) for p in prompts]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                while any(s.status in (Status.WAITING, Status.PREFILL) for s in seqs):
                    eng.step()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                n1 = sum(len(s.output) for s in seqs)
                while any(s.status != Status.FINISHED for s in seqs):
                    eng.step()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
            finally:
                ops.rope_cache = plain
            print(json.dumps(dict(bench="engine", round=rnd, variant=name, model=base.name, layers=base.num_layers,
                                  seqs=args.seqs, prompt=args.prompt, gen=args.gen,
                                  prefill_tok_s=round(args.seqs * args.prompt / (t1 - t0)),
                                  decode_tok_s=round((args.seqs * args.gen - n1) / (t2 - t1)),
                                  graph_steps=eng.stats["graph_steps"])), flush=True)
            res[name].append((round(args.seqs * args.prompt / (t1 - t0)), round((args.seqs * args.gen - n1) / (t2 - t1))))
            del eng, seqs
            torch.cuda.empty_cache()
    md_append(args.md, f"engine, {base.name} shapes, batch {args.seqs}, {args.prompt} + {args.gen} tokens: tok/s, best of "
                       f"{args.rounds} rounds (all rounds)",
              ["variant", "prefill", "decode"],
              [[n, *(f"{max(x[i] for x in r)} ({' / '.join(str(x[i]) for x in r)})" for i in (0, 1))] for n, r in res.items()])


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("what", choices=["writer", "engine"])
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=200, help="writer: launches per timing")
ap.add_argument("--tokens", default="1,64,2048,4096", help="writer: token counts")
ap.add_argument("--seqs", type=int, default=64)
ap.add_argument("--prompt", type=int, default=128)
ap.add_argument("--gen", type=int, default=64)
ap.add_argument("--chunk", type=int, default=8192, help="engine: max_num_batched_tokens")
ap.add_argument("--model", default="qwen3-8b")
ap.add_argument("--layers", type=int, default=0, help="engine: override the layer count (0: the model's)")
ap.add_argument("--md", default=None, help="append this run's table to a markdown file")
ap.add_argument("--kv-gb", type=float, default=40.0, help="engine: kv_cache_bytes, in GB")
a = ap.parse_args()
{"writer": bench_writer, "engine": bench_engine}[a.what](a)
