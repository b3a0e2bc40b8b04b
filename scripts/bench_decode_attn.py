"""Decode paged-attention microbench (Llama-3-8B heads: 32 q / 8 kv, D=128, pages of 16
tokens scattered over the pool): B sequences x 1 query token at context L.  Reports
the KV bytes streamed per call and the effective HBM rate (roofline ~6.3 TB/s).

--window W runs the sliding-window kernel (each row reads its last W keys, from the page pair
holding the first of them; the partitions are planned over that span as the engine does);
--exact-ctx makes every context exactly L (default: uniform in L/2 .. 3L/2), so a windowed
launch at a long context can be compared with the plain kernel at context W."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from mlopamd import ops  # noqa: E402
from mlopamd.runtime.attn_meta import plan_partitions  # noqa: E402
from test_kernels_gpu import make_meta  # noqa: E402

ops.load()
dev = torch.device("cuda")
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


ap = argparse.ArgumentParser()
ap.add_argument("--window", type=int, default=0, help="sliding window in tokens (0: full causal attention)")
ap.add_argument("--exact-ctx", action="store_true", help="every context exactly L")
ap.add_argument("--fused-combine", action="store_true",
                help="split-KV launches combine in the launch (tickets), as the engine's; default: reduce launch")
ap.add_argument("--cases", default=os.environ.get("CASES", "2048x384,1024x384,256x1024,64x4096,8x8192"),
                help="comma-separated BxL")
args = ap.parse_args()
W = args.window
cases = [(int(b), int(l)) for b, l in (c.split("x") for c in args.cases.split(","))]
for B, L in cases:
    np.random.seed(0)
    ctx = [L] * B if args.exact_ctx else np.random.randint(max(16, L // 2), L * 3 // 2 + 1, size=B).tolist()
    NB = sum((c + 15) // 16 for c in ctx) + 8
    kc = torch.randn(NB, Hkv, 16, D, device=dev, dtype=bf)
    vc = torch.randn(NB, Hkv, 16, D, device=dev, dtype=bf)
    kw = {}
    if W:  # the engine's plan: over the longest key span of a tile (MetaBuffers.span)
        part, nparts = plan_partitions(B, Hkv, min(max(ctx), W + 31 + 16 // (Hq // Hkv) - 1))
        kw = dict(part_tokens=part, nparts=nparts)
    m, T = make_meta(dev, [1] * B, ctx, Hkv, Hq // Hkv, NB, **kw)
    m.window = W
    nparts = m.nparts
    if nparts > 1 and args.fused_combine:  # the in-launch combine, as the engine runs it
        m.part_sem = torch.zeros(B * Hkv, dtype=torch.int32, device=dev)
    q = torch.randn(T, Hq, D, device=dev, dtype=bf)
    t = min(timeit(lambda: ops.paged_attention(q, kc, vc, m)) for _ in range(3))
    keys = sum(c - (max(0, c - W) & ~31) for c in ctx) if W else sum(ctx)  # from the window's page pair
    byts = keys * Hkv * D * 2 * 2
    print(json.dumps(dict(B=B, window=W, mean_ctx=round(float(np.mean(ctx)), 1), nparts=nparts, us=round(t, 1),
                          kv_gb=round(byts / 1e9, 3), tbps=round(byts / t / 1e6, 2))), flush=True)
