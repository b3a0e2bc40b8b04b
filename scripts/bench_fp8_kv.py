"""fp8 KV cache against bf16, the pieces bench_decode_attn.py --kv-dtype does not cover
(profiles/fp8_kv.md).  One JSON line per measurement; the two formats alternate round by round.

  writer   RoPE + cache write of T tokens (Llama-3-8B heads): rope_cache (bf16) vs rope_cache_fp8
  prefill  B prompts of L tokens: flash prefill on bf16 pages vs the 16-row tiles on bf16 and on
           fp8 pages (under fp8 prompt chunks run there: the price of the missing fp8 flash kernel)
  engine   the headline-shaped engine (Llama-3-8B, --seqs sequences, --prompt / --gen tokens) with
           kv_cache_dtype bf16 and fp8: prefill and decode tok/s, pages of one byte budget
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from mlopamd import ops  # noqa: E402

ops.load()
dev = torch.device("cuda", 0)
bf = torch.bfloat16
Hq, Hkv, D = 32, 8, 128


def timeit(fn, iters=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def interleaved(runs: dict, rounds: int) -> dict:
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(timeit(fn))
    return times


def report(what, times, **extra):
    for k, ts in times.items():
        s = sorted(ts)
        print(json.dumps(dict(bench=what, variant=k, us=round(s[0], 1), us_rounds=[round(x, 1) for x in ts],
                              spread_pct=round(100 * (s[-1] - s[0]) / s[0], 2), **extra)), flush=True)


def fp8_pool(NB):
    mk = lambda *s: torch.zeros(s, dtype=torch.uint8, device=dev)  # noqa: E731
    return mk(NB, Hkv, 16, D).view(ops.ref.FP8), mk(NB, Hkv, 16, D).view(ops.ref.FP8), mk(NB, Hkv, 16), mk(NB, Hkv, 16)


def bench_writer(args):
    for T in (int(t) for t in args.tokens.split(",")):
        NB = T // 16 + 64
        qkv = torch.randn(T, (Hq + 2 * Hkv) * D, device=dev).to(bf)
        pos = torch.randint(0, 1024, (T,), device=dev, dtype=torch.int32)
        slots = (torch.randperm((NB - 1) * 16, device=dev)[:T] + 16).to(torch.int32)
        cs = torch.randn(1024, D, device=dev)
        kb, vb = (torch.zeros(NB, Hkv, 16, D, device=dev, dtype=bf) for _ in range(2))
        k8, v8, ks, vs = fp8_pool(NB)
        q = torch.empty(T, Hq, D, device=dev, dtype=bf)
        runs = {"bf16": lambda: ops.rope_cache(qkv, pos, cs, slots, kb, vb, Hq, q_out=q),
                "fp8": lambda: ops.rope_cache(qkv, pos, cs, slots, k8, v8, Hq, q_out=q, k_scale=ks, v_scale=vs)}
        report("writer", interleaved(runs, args.rounds), tokens=T)


def bench_prefill(args):
    from test_kernels_gpu import make_meta

    B, L = args.seqs, args.prompt
    np.random.seed(0)
    NB = B * ((L + 15) // 16) + 8
    kc = torch.randn(NB, Hkv, 16, D, device=dev).to(bf)
    vc = torch.randn(NB, Hkv, 16, D, device=dev).to(bf)
    k8, ks = ops.ref.fp8_quantize_rows(kc)
    v8, vs = ops.ref.fp8_quantize_rows(vc)
    np.random.seed(1)
    m_flash, T = make_meta(dev, [L] * B, [L] * B, Hkv, Hq // Hkv, NB, flash_min_q=17)
    np.random.seed(1)
    m_tiles, _ = make_meta(dev, [L] * B, [L] * B, Hkv, Hq // Hkv, NB)
    q = torch.randn(T, Hq, D, device=dev).to(bf)
    runs = {"bf16_flash": lambda: ops.paged_attention(q, kc, vc, m_flash),
            "bf16_tiles16": lambda: ops.paged_attention(q, kc, vc, m_tiles),
            "fp8_tiles16": lambda: ops.paged_attention(q, k8, v8, m_tiles, k_scale=ks, v_scale=vs)}
    report("prefill", interleaved(runs, args.rounds), seqs=B, prompt=L)


def bench_engine(args):
    from mlopamd.models import build_model
    from mlopamd.models.config import get_config
    from mlopamd.runtime.engine import Engine, EngineConfig, Status
    from mlopamd.runtime.sampler import SamplingParams

    cfg = get_config(args.model, **({"num_layers": args.layers} if args.layers else {}))
    model = build_model(cfg, device=dev)
    max_len = args.prompt + args.gen + 16
    g = torch.Generator().manual_seed(0)
    prompts = [torch.randint(3, cfg.vocab_size - 1, (args.prompt,), generator=g).tolist() for _ in range(args.seqs)]
    budget = int(args.kv_gb * 1e9)
    for rnd in range(args.rounds):
        for dt in ("bf16", "fp8"):
            eng = Engine(model, EngineConfig(max_num_seqs=args.seqs, max_num_batched_tokens=args.chunk,
                                             max_model_len=max_len, kv_cache_bytes=budget, kv_fraction=1.0,
                                             graph_buckets=(args.seqs,), enable_prefix_caching=False,
                                             kv_cache_dtype=dt))
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
            print(json.dumps(dict(bench="engine", round=rnd, kv_cache_dtype=dt, model=cfg.name, layers=cfg.num_layers,
                                  seqs=args.seqs, prompt=args.prompt, gen=args.gen, kv_budget_gb=args.kv_gb,
                                  kv_pages=eng.alloc.num_blocks, kv_gb=round(eng.kv.nbytes / 1e9, 3),
                                  prefill_tok_s=round(args.seqs * args.prompt / (t1 - t0)),
                                  decode_tok_s=round((args.seqs * args.gen - n1) / (t2 - t1)),
                                  graph_steps=eng.stats["graph_steps"], preemptions=eng.stats["preemptions"])),
                  flush=True)
            del eng, seqs
            torch.cuda.empty_cache()


ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("what", choices=["writer", "prefill", "engine"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--tokens", default="2048,4096", help="writer: token counts")
ap.add_argument("--seqs", type=int, default=4)
ap.add_argument("--prompt", type=int, default=2048)
ap.add_argument("--gen", type=int, default=128)
ap.add_argument("--chunk", type=int, default=10240, help="engine: max_num_batched_tokens")
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--layers", type=int, default=0, help="engine: override the layer count (0: the preset's)")
ap.add_argument("--kv-gb", type=float, default=100.0, help="engine: kv_cache_bytes of both formats, in GB")
a = ap.parse_args()
{"writer": bench_writer, "prefill": bench_prefill, "engine": bench_engine}[a.what](a)
