"""Multi-LoRA (K16) at the Llama-3-8B shapes.

Kernels: ``ops.lora_shrink`` / ``ops.lora_expand_add`` for the four projections at
T in {1, 16, 64, 256, 2048, 4096} tokens with 1 and 8 distinct adapters per step (tokens assigned
round-robin, so every 16-token tile mixes all of them), rank 16 in R = 64 storage, against the
torch formulation on the same device: ``index_select`` of the per-token A / B and ``bmm`` (B as
[S, N, G R] with zeros outside a column's own block where G > 1).  Microseconds per call from
device events, warmed, >= 50 calls; the torch side is skipped ("not measured") where its gathered
operand would exceed ``--torch-max-gib``.

Engine (``--engine``): generated tok/s of the model named by ``--model`` with every row on one of 8 adapters against base-only requests on the same engine, alternating,
at batch 1 / 64 / 1024.  One JSON line per measurement; results: profiles/lora.md."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mlopamd import ops  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--tokens", type=int, nargs="+", default=[1, 16, 64, 256, 2048, 4096])
ap.add_argument("--adapters", type=int, nargs="+", default=[1, 8])
ap.add_argument("--rank", type=int, default=16)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--torch-max-gib", type=float, default=8.0)
ap.add_argument("--engine", action="store_true", help="also the engine tok/s comparison")
ap.add_argument("--model", default="llama3-8b")
ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 1024])
ap.add_argument("--prompt", type=int, default=128)
ap.add_argument("--gen", type=int, default=64)
ap.add_argument("--no-kernels", action="store_true")
args = ap.parse_args()

if not torch.cuda.is_available():
    raise SystemExit("bench_lora.py measures on the GPU only")
ops.load()
dev = torch.device("cuda")
S, R = 8, 64
# Llama-3-8B: (name, K, N, rows per sub-projection or None for the 16-interleaved gate_up)
SHAPES = [("qkv", 4096, 6144, (4096, 1024, 1024)), ("o", 4096, 4096, (4096,)),
          ("gate_up", 4096, 28672, None), ("down", 14336, 4096, (4096,))]


def timeit(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return round(s.elapsed_time(e) / calls * 1e3, 2)


def emit(**kw):
    print(json.dumps(kw), flush=True)


def kernels():
    g = torch.Generator(device=dev).manual_seed(0)
    for name, K, N, parts in SHAPES:
        if parts is None:
            G, tg = 2, (torch.arange(N // 16, device=dev) & 1).to(torch.uint8)
        else:
            G = len(parts)
            tg = torch.cat([torch.full((n // 16,), i, dtype=torch.uint8, device=dev) for i, n in enumerate(parts)])
        A = torch.zeros(S, G, R, K, device=dev, dtype=torch.bfloat16)
        A[:, :, :args.rank] = (torch.randn(S, G, args.rank, K, device=dev, generator=g) * K ** -0.5).to(A.dtype)
        A = A.view(S, G * R, K)
        B = torch.zeros(S, N, R, device=dev, dtype=torch.bfloat16)
        B[:, :, :args.rank] = torch.randn(S, N, args.rank, device=dev, generator=g).to(B.dtype)
        rank = torch.full((S,), args.rank, dtype=torch.int32, device=dev)
        # torch formulation's B: [S, N, G R], a column's own block filled
        col_g = tg.long().repeat_interleave(16)
        Bf = torch.zeros(S, N, G, R, device=dev, dtype=torch.bfloat16)
        Bf[:, torch.arange(N, device=dev), col_g] = B
        Bf = Bf.view(S, N, G * R)
        for T in args.tokens:
            x = torch.randn(T, K, device=dev, generator=g).to(torch.bfloat16)
            y = torch.randn(T, N, device=dev, generator=g).to(torch.bfloat16)
            for nad in args.adapters:
                ts = (torch.arange(T, device=dev) % nad).to(torch.int32)
                tl = ts.long()
                tmp = ops.lora_shrink(x, A, ts, rank, groups=G)
                rec = dict(proj=name, K=K, N=N, G=G, T=T, adapters=nad, rank=args.rank)
                rec["shrink_us"] = timeit(lambda: ops.lora_shrink(x, A, ts, rank, groups=G, out=tmp), args.calls)
                rec["expand_us"] = timeit(lambda: ops.lora_expand_add(y, tmp, B, tg, ts, rank), args.calls)
                gib_a = T * G * R * K * 2 / 2**30
                gib_b = T * N * G * R * 2 / 2**30
                if gib_a <= args.torch_max_gib:
                    rec["torch_shrink_us"] = timeit(
                        lambda: torch.bmm(A.index_select(0, tl), x.unsqueeze(2)), max(5, args.calls // 5))
                else:
                    rec["torch_shrink_us"] = f"not measured (index_select of {gib_a:.1f} GiB)"
                if gib_b <= args.torch_max_gib:
                    tb = tmp.to(torch.bfloat16).unsqueeze(2)
                    rec["torch_expand_us"] = timeit(
                        lambda: y.add_(torch.bmm(Bf.index_select(0, tl), tb).squeeze(2)), max(5, args.calls // 5))
                else:
                    rec["torch_expand_us"] = f"not measured (index_select of {gib_b:.1f} GiB)"
                emit(**rec)
        del A, B, Bf


def engine():
    from mlopamd.models.lora import PROJ_MODULES, Adapter, module_shapes
    from mlopamd.runtime.deploy import build_engine
    from mlopamd.runtime.sampler import SamplingParams

    bmax = max(args.batches)
    eng = build_engine(args.model, device="cuda", max_num_seqs=bmax, max_model_len=1024,
                       max_num_batched_tokens=8192, max_adapters=S, max_lora_rank=R,
                       graph_buckets=tuple(sorted(set(args.batches))))
    cfg = eng.model.cfg
    shapes = module_shapes(cfg)
    for i in range(S):
        gen = torch.Generator().manual_seed(100 + i)
        layers = []
        for _ in range(cfg.num_layers):
            L = {}
            for proj, mods in PROJ_MODULES.items():
                K = shapes[mods[0]][1]
                n = sum(shapes[m][0] for m in mods)
                L[proj] = (torch.randn(len(mods), args.rank, K, generator=gen) * 0.01,
                           torch.randn(n, args.rank, generator=gen) * 0.01)
            layers.append(L)
        eng.add_adapter(f"a{i}", Adapter(rank=args.rank, layers=layers, digest=bytes([i])))
    emit(engine=args.model, lora_bytes=int(eng.stats["lora_bytes"]), kv_blocks=eng.kv.num_blocks)
    g = torch.Generator().manual_seed(1)
    for b in args.batches:
        prompts = [torch.randint(1000, 100000, (args.prompt,), generator=g).tolist() for _ in range(b)]
        for rnd in range(3):  # round 0 warms both paths
            for mode in ("base", "lora"):
                sp = [SamplingParams(max_tokens=args.gen, ignore_eos=True,
                                     adapter=f"a{j % S}" if mode == "lora" else None) for j in range(b)]
                torch.cuda.synchronize()
                before = dict(eng.stats)
                t0 = time.perf_counter()
                eng.generate(prompts, sp)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if rnd:
                    emit(engine=args.model, batch=b, mode=mode, round=rnd, tok_s=round(b * args.gen / dt, 1),
                         seconds=round(dt, 3), lora_steps=eng.stats["lora_steps"] - before.get("lora_steps", 0),
                         graph_steps=eng.stats["graph_steps"] - before.get("graph_steps", 0),
                         prefix_hit_tokens=eng.stats["prefix_hit_tokens"] - before.get("prefix_hit_tokens", 0))


if not args.no_kernels:
    kernels()
if args.engine:
    engine()
