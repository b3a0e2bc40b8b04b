"""Embedding requests: what the pooling launch costs and how fast the engine embeds.

  1. pool_accumulate + pool_finish alone (HIP events, one pair per launch pair, median of --reps after a
     warm-up), H = 4096, for (segments x rows) = (1 x 8192), (64 x 128), (512 x 16) and the shape of the
     engine run's own steps (16 x 512 by default), ``mean`` and ``last`` interleaved per round.  The
     1 x 8192 ``mean`` case is the serial row walk of one long segment.
  2. the engine on Llama-3-8B shapes (random weights, --layers of them): embeddings per second for
     --n inputs of --len tokens, beside the same step shapes run as generation prefill (max_tokens = 1:
     the same chunks plus the LM head and the sampler, no pooling), A / B interleaved per round.

Prints one JSON line.  Usage: python scripts/bench_embed.py [--layers 32] [--n 64] [--len 512] [--rounds 3]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mlopamd import ops  # noqa: E402
from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import get_config  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--len", type=int, default=512, dest="length")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--batched-tokens", type=int, default=8192)
args = ap.parse_args()

dev = torch.device("cuda", 0)
ops.load()
H = 4096


def kernel_us(nseg, rows, mode):
    T = nseg * rows
    x = torch.randn(T, H, device=dev).to(torch.bfloat16)
    acc = torch.zeros(nseg, H, device=dev)
    out = torch.zeros(nseg, H, device=dev)
    m = 0 if mode == "mean" else ops.POOL_MODE_LAST
    seg = torch.tensor([(i * rows, (i + 1) * rows, i, ops.POOL_INIT | ops.POOL_LAST | m) for i in range(nseg)],
                       dtype=torch.int32, device=dev)
    fin = torch.tensor([(i, rows, H, ops.POOL_FIN_NORMALIZE | (ops.POOL_FIN_MEAN if mode == "mean" else 0))
                        for i in range(nseg)], dtype=torch.int32, device=dev)
    ts = []
    for i in range(args.reps + 5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.pool_accumulate(x, seg, acc)
        ops.pool_finish(acc, fin, out)
        b.record()
        b.synchronize()
        if i >= 5:
            ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


res = {"kernel_us": {}, "H": H}
# (the last: the pooling launch of the engine run below, 16 whole 512-token prompts per 8192-token step)
shapes = [(1, 8192), (64, 128), (512, 16), (args.batched_tokens // args.length, args.length)]
per = {(s, m): [] for s in shapes for m in ("mean", "last")}
for _ in range(args.rounds):
    for s in shapes:
        for m in ("mean", "last"):
            per[(s, m)].append(kernel_us(*s, m))
for (s, m), v in per.items():
    res["kernel_us"][f"{s[0]}x{s[1]}_{m}"] = round(statistics.median(v), 1)

cfg = get_config("llama3-8b", num_layers=args.layers)
model = build_model(cfg, device=dev)
g = torch.Generator().manual_seed(0)
prompts = [torch.randint(2, cfg.vocab_size - 1, (args.length,), generator=g).tolist() for _ in range(args.n)]
eng = Engine(model, EngineConfig(max_num_seqs=args.n, max_num_batched_tokens=args.batched_tokens,
                                 max_model_len=args.length + 16, embed_slots=args.n, use_graphs=False,
                                 enable_prefix_caching=False))


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


runs = {"embed_last": lambda: eng.embed(prompts, "last"), "embed_mean": lambda: eng.embed(prompts, "mean"),
        "prefill": lambda: eng.generate(prompts, SamplingParams(max_tokens=1, ignore_eos=True))}
for fn in runs.values():
    fn()  # warm-up (autotune, allocator)
t = {k: [] for k in runs}
for _ in range(args.rounds):
    for k, fn in runs.items():
        t[k].append(timed(fn))
res["engine"] = {"layers": args.layers, "inputs": args.n, "tokens_per_input": args.length,
                 **{f"{k}_per_s": round(args.n / statistics.median(v), 1) for k, v in t.items()},
                 **{f"{k}_s": [round(x, 4) for x in v] for k, v in t.items()},
                 "embed_steps": int(eng.stats["embed_steps"])}
print(json.dumps(res))
