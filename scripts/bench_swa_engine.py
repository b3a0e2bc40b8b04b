"""Sliding-window serving end to end: N sequences of PROMPT tokens through the engine on a
random-init windowed model (default mistral-7b: window 4096), then GEN decode steps, with the
release of pages below the window on and off.  Reports the KV pages held when the last prompt
has been prefilled (every sequence running), the peak over the run, the pages released, and
prefill / decode tok/s.  One JSON line per setting."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlopamd import ops  # noqa: E402
from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import get_config  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig, Status  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="mistral-7b")
ap.add_argument("--layers", type=int, default=0, help="override the layer count (0: the preset's)")
ap.add_argument("--window", type=int, default=-1, help="override the preset's sliding window (-1: keep)")
ap.add_argument("--seqs", type=int, default=8)
ap.add_argument("--prompt", type=int, default=16384)
ap.add_argument("--gen", type=int, default=128)
ap.add_argument("--chunk", type=int, default=8192, help="max_num_batched_tokens")
ap.add_argument("--release", default="1,0", help="swa_release settings to run, comma-separated")
args = ap.parse_args()

ops.load()
dev = torch.device("cuda", 0)
over = {}
if args.layers:
    over["num_layers"] = args.layers
if args.window >= 0:
    over["sliding_window"] = args.window
cfg = get_config(args.model, **over)
model = build_model(cfg, device=dev)
max_len = args.prompt + args.gen + 16
pages = args.seqs * ((max_len + 15) // 16) + 64
g = torch.Generator().manual_seed(0)
prompts = [torch.randint(3, cfg.vocab_size - 1, (args.prompt,), generator=g).tolist() for _ in range(args.seqs)]

for rel in (int(r) for r in args.release.split(",")):
    eng = Engine(model, EngineConfig(max_num_seqs=args.seqs, max_num_batched_tokens=args.chunk,
                                     max_model_len=max_len, num_kv_blocks=pages, swa_release=bool(rel),
                                     graph_buckets=(args.seqs,), enable_prefix_caching=False))
    # (pages in use: the allocator's page ids grow while a lazily backed pool fills, page 0 is
    # the null page)
    held = lambda: eng.alloc.available - 1 - eng.alloc.num_free  # noqa: E731
    seqs = [eng.add_request(p, SamplingParams(max_tokens=args.gen, ignore_eos=True)) for p in prompts]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    peak = 0
    while any(s.status in (Status.WAITING, Status.PREFILL) for s in seqs):
        eng.step()
        peak = max(peak, held())
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    held_prefill = held()
    while any(s.status != Status.FINISHED for s in seqs):
        eng.step()
        peak = max(peak, held())
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(json.dumps(dict(model=cfg.name, layers=cfg.num_layers, window=cfg.sliding_window, swa_release=rel,
                          seqs=args.seqs, prompt=args.prompt, gen=args.gen,
                          pages_held_all_running=held_prefill,
                          pages_per_seq=round(held_prefill / args.seqs, 1), pages_peak=peak,
                          pages_released=eng.stats["kv_pages_released"],
                          prefill_tok_s=round(args.seqs * args.prompt / (t1 - t0)),
                          decode_tok_s=round(args.seqs * (args.gen - 1) / (t2 - t1)),
                          graph_steps=eng.stats["graph_steps"])), flush=True)
    assert held() == 0
    del eng
