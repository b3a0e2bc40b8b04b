"""MXFP4 expert weights (moe_mx4.hip) against the bf16 grouped GEMM, on one GPU, the routes
alternating round by round in one process.

    python scripts/bench_moe_mx4.py kernel      # gate_up and down of one MoE layer: us per launch
    python scripts/bench_moe_mx4.py engine      # engine tok/s with bf16 and mxfp4 experts

kernel: one layer's experts at Mixtral-8x7B (8 experts, top-2) and Qwen3-30B-A3B (128 experts, top-8)
shapes; T tokens routed uniformly at random (distinct experts per token), sorted by ``ops.moe_permute``.
Per (model, T): ``ops.grouped_gemm`` over bf16 experts, ``ops.grouped_gemm_mx4`` forced onto the
streaming kernel, forced onto dequantise + grouped GEMM (the two sides of
MLOP_MX4_MOE_MAX_AVG_ROWS, the tile route off) and forced onto the fused tiled kernel (moe_mx4t.hip).  Weight copies and routings rotate with coprime periods so that a call
streams weights the calls before it have pushed out of the caches.  Device events; one JSON line per
(model, projection, T) with the median of the rounds and their min / max.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mlopamd import ops  # noqa: E402
from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import get_config  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

MODELS = {"mixtral-8x7b": (8, 2, 4096, 14336), "qwen3-30b-a3b": (128, 8, 2048, 768)}  # E, top-k, H, I
ROUTINGS = 17  # coprime with every copy count below


def _time(fn, warm, iters):
    for i in range(warm):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def _stats(row, name, ts):
    row.update({f"{name}_us": round(statistics.median(ts), 2), f"{name}_min": round(min(ts), 2),
                f"{name}_max": round(max(ts), 2)})


def bench_kernel(args):
    dev = torch.device("cuda", 0)
    ops.load()
    for name in args.models:
        E, k, H, I = MODELS[name]
        copies = 2 if E == 8 else 4
        g = torch.Generator(device=dev).manual_seed(0)
        wb = {"gate_up": [(0.02 * torch.randn(E, 2 * I, H, device=dev, generator=g)).to(torch.bfloat16) for _ in range(copies)],
              "down": [(0.02 * torch.randn(E, H, I, device=dev, generator=g)).to(torch.bfloat16) for _ in range(copies)]}
        wm = {p: [ops.mx4_experts_quantize_pack(w) for w in ws] for p, ws in wb.items()}
        ops.q4_reserve_scratch(dev, E * 2 * I * H)
        for T in args.tokens:
            routes = []
            for _ in range(ROUTINGS):
                topi = torch.rand(T, E, device=dev, generator=g).topk(k, dim=1).indices.to(torch.int32)
                x = torch.randn(T, H, device=dev, dtype=torch.bfloat16, generator=g)
                xp, off, _src, _inv = ops.moe_permute(x, topi, 0, E)
                act = torch.randn(T * k, I, device=dev, dtype=torch.bfloat16, generator=g)
                routes.append((xp, act, off))
            avg = max(1, T * k // E)
            for proj, epi in (("gate_up", ops.EPI_SILU_MUL), ("down", ops.EPI_NONE)):
                a_of = (lambda r: r[0]) if proj == "gate_up" else (lambda r: r[1])

                def mx4(i, limit, tile=False):
                    r = routes[i % ROUTINGS]
                    ops.MX4_MOE_MAX_AVG_ROWS = limit
                    ops.MX4_MOE_TILE_MIN_AVG_ROWS, ops.MX4_MOE_TILE_MAX_AVG_ROWS = 0, (1 << 30 if tile else 0)
                    return ops.grouped_gemm_mx4(a_of(r), wm[proj][i % copies], r[2], epi=epi, avg_rows=avg)

                fns = {"bf16": lambda i: ops.grouped_gemm(a_of(routes[i % ROUTINGS]), wb[proj][i % copies],
                                                          routes[i % ROUTINGS][2], epi=epi, avg_rows=avg),
                       "mxfp4_kernel": lambda i: mx4(i, 1 << 30), "mxfp4_dequant": lambda i: mx4(i, 0),
                       "mxfp4_tile": lambda i: mx4(i, 0, True)}
                iters = max(8, min(200, 4096 // max(16, T)))
                ts = {n: [] for n in fns}
                for _ in range(args.rounds):
                    for n, fn in fns.items():
                        ts[n].append(_time(fn, copies, iters))
                N = 2 * I if proj == "gate_up" else H
                row = dict(bench="kernel", model=name, proj=proj, T=T, avg_rows=avg,
                           rb=int(torch.ops.mlop.moe_mx4_rb(T * k, E, N, epi)))
                for n, v in ts.items():
                    _stats(row, n, v)
                print(json.dumps(row), flush=True)
        del wb, wm
        torch.cuda.empty_cache()


def bench_engine(args):
    dev = torch.device("cuda", 0)
    ops.load()
    g = torch.Generator().manual_seed(0)
    for name in args.models:
        cfg = get_config(name, num_layers=args.layers)
        for rnd in range(args.rounds):
            for xd in ("bf16", "mxfp4"):
                model = build_model(cfg, device=dev, seed=0)
                eng = Engine(model, EngineConfig(max_num_seqs=512, max_num_batched_tokens=2048, max_model_len=1024,
                                                 num_kv_blocks=4096, graph_buckets=(1, 8, 64, 512), expert_weight_dtype=xd))
                row = dict(bench="engine", model=name, round=rnd, expert_weight_dtype=xd, layers=cfg.num_layers,
                           weight_gb=round(model.weight_bytes() / 1e9, 3))
                for batch in args.batches:
                    prompts = [torch.randint(2, 1000, (16,), generator=g).tolist() for _ in range(batch)]
                    eng.generate(prompts, SamplingParams(max_tokens=8, ignore_eos=True))  # warm-up, graph capture
                    torch.cuda.synchronize()
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    eng.generate(prompts, SamplingParams(max_tokens=args.gen, ignore_eos=True))
                    b.record()
                    b.synchronize()
                    row[f"tok_s_b{batch}"] = round(batch * args.gen / (a.elapsed_time(b) / 1e3), 1)
                print(json.dumps(row), flush=True)
                del eng, model
                torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "engine"])
    ap.add_argument("--models", nargs="*", default=list(MODELS))
    ap.add_argument("--tokens", type=int, nargs="*", default=[1, 4, 16, 64, 256, 1024, 2048, 4096])
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8, 64, 512])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--gen", type=int, default=64)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_moe_mx4 measures on a GPU"
    {"kernel": bench_kernel, "engine": bench_engine}[args.what](args)


if __name__ == "__main__":
    main()
