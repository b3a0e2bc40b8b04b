"""Decode paged-attention microbench (Llama-3-8B heads: 32 q / 8 kv, D=128, pages of 16
tokens scattered over the pool): B sequences x 1 query token at context L.  Reports
the KV bytes streamed per call and the effective HBM rate (roofline ~6.3 TB/s).

--window W runs the sliding-window kernel (each row reads its last W keys, from the page pair
holding the first of them; the partitions are planned over that span as the engine does);
--exact-ctx makes every context exactly L (default: uniform in L/2 .. 3L/2), so a windowed
launch at a long context can be compared with the plain kernel at context W.

Every input is seeded (contexts, page layout, q, caches).  --dump DIR writes each case's output
bytes (DIR/<case>.out) and a sha256 of its inputs and of the output (DIR/<case>.json), so two
processes - two builds of the kernels - can show they ran the same case and compare results."""
import argparse
import hashlib
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
D = 128


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes())
    return h.hexdigest()


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
ap.add_argument("--kv-dtype", default="bf16", choices=["bf16", "fp8", "both"],
                help="KV cache format; both: the bf16 and the fp8 kernel interleaved round by round on the same "
                     "metadata (the fp8 pages are the quantised bf16 pages), with the run-to-run spread of each")
ap.add_argument("--rounds", type=int, default=3, help="timed rounds per format (each 10 launches; min and spread reported)")
ap.add_argument("--heads", default="32x8", help="HqxHkv (the GQA group Hq / Hkv must divide 16)")
ap.add_argument("--dump", default=None, metavar="DIR", help="write each case's output bytes and input checksum here")
args = ap.parse_args()
W = args.window
Hq, Hkv = (int(x) for x in args.heads.split("x"))
if args.dump:
    os.makedirs(args.dump, exist_ok=True)
if W and args.kv_dtype != "bf16":
    sys.exit("the fp8 cache has no sliding-window kernel")
cases = [(int(b), int(l)) for b, l in (c.split("x") for c in args.cases.split(","))]
for B, L in cases:
    np.random.seed(0)      # contexts and the page layout (make_meta)
    torch.manual_seed(0)   # q and the caches
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
    keys = sum(c - (max(0, c - W) & ~31) for c in ctx) if W else sum(ctx)  # from the window's page pair
    runs = {}
    if args.kv_dtype in ("bf16", "both"):
        runs["bf16"] = (lambda: ops.paged_attention(q, kc, vc, m), keys * Hkv * D * 2 * 2)
    if args.kv_dtype in ("fp8", "both"):
        k8, ks = ops.ref.fp8_quantize_rows(kc)
        v8, vs = ops.ref.fp8_quantize_rows(vc)
        if args.kv_dtype == "fp8":
            del kc, vc
        runs["fp8"] = (lambda: ops.paged_attention(q, k8, v8, m, k_scale=ks, v_scale=vs), keys * Hkv * (D + 1) * 2)
    if args.dump:
        meta_in = (m.block_tables, m.tile_seq, m.tile_q0, m.q_start, m.q_len, m.ctx_len)
        ins = {"bf16": lambda: (q, kc, vc) + meta_in, "fp8": lambda: (q, k8, ks, v8, vs) + meta_in}
        for d, (fn, _) in runs.items():
            out = fn()
            torch.cuda.synchronize()
            tag = f"{B}x{L}_{args.heads}_{d}_w{W}_{'fused' if args.fused_combine else 'reduce'}"
            raw = out.contiguous().view(torch.uint8).cpu().numpy().tobytes()
            with open(os.path.join(args.dump, tag + ".out"), "wb") as f:
                f.write(raw)
            with open(os.path.join(args.dump, tag + ".json"), "w") as f:
                json.dump(dict(case=tag, nparts=nparts, part_tokens=m.part_tokens, inputs_sha256=sha(*ins[d]()),
                               out_sha256=hashlib.sha256(raw).hexdigest()), f)
    times = {d: [] for d in runs}
    for _ in range(args.rounds):  # interleaved: one round of each format after the other
        for d, (fn, _) in runs.items():
            times[d].append(timeit(fn))
    for d, (_, byts) in runs.items():
        t, ts = min(times[d]), sorted(times[d])
        print(json.dumps(dict(B=B, kv_dtype=d, window=W, mean_ctx=round(float(np.mean(ctx)), 1), nparts=nparts,
                              us=round(t, 1), us_rounds=[round(x, 1) for x in times[d]],
                              spread_pct=round(100 * (ts[-1] - ts[0]) / ts[0], 2),
                              kv_gb=round(byts / 1e9, 3), tbps=round(byts / t / 1e6, 2))), flush=True)
