"""MXFP4 weights (gemm_mx4.hip) against the bf16 and int4 routes, on one GPU, the three alternating
round by round in one process.

    python scripts/bench_mx4.py kernel          # the projections: us, achieved TB/s of packed bytes
    python scripts/bench_mx4.py rb              # gemm_mx4_kernel with 1 / 2 / 4 row blocks per workgroup
    python scripts/bench_mx4.py engine          # a Llama-3-8B engine with bf16, int4 and mxfp4 weights
    python scripts/bench_mx4.py tile            # gemm_mx4t.hip against bf16, the dequantise route and the streaming kernel
    python scripts/bench_mx4.py tile-engine     # the mxfp4 engine with MLOP_MX4_TILE_MAX_M = 0 and --tile-max-m, alternating

kernel: the four Llama-3-8B projections and 70B's gate_up.  M <= 64: ``ops.gemm_mx4`` and ``ops.gemm_q4``
(the weight-streaming kernels) against ``ops.gemm`` over the bf16 weight; M = 128, 512, 2048:
dequantise + GEMM against the GEMM alone.  Each timed window flushes nothing: like the decode loop,
every call streams weights that the other projections' traffic has pushed out of the caches (the
weights rotate over enough copies to exceed them).  Device events; one JSON line per (shape, M) with
the median of the rounds and their min / max.

tile: per shape and M the bf16 ``ops.gemm``, dequantise + GEMM, the tiled op with the launcher's split
and (o, down) every forced split of --ks, and the streaming kernel up to 64 rows; TB/s of packed bytes
and TF/s (2 M N K) from the shapes.  tile-engine: decode at batch 64 and 256 and prefill 4 x 2048, each
knob value in a fresh child process (the knob is read at import), alternating round by round.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

from mlopamd import ops  # noqa: E402
from mlopamd.models import build_model  # noqa: E402
from mlopamd.models.config import get_config  # noqa: E402
from mlopamd.runtime.engine import Engine, EngineConfig  # noqa: E402
from mlopamd.runtime.sampler import SamplingParams  # noqa: E402

SHAPES = {"8b-qkv": (6144, 4096), "8b-o": (4096, 4096), "8b-gate_up": (28672, 4096), "8b-down": (4096, 14336),
          "70b-gate_up": (57344, 8192)}
CACHE_BYTES = 512 * 2 ** 20  # rotate over more weight bytes than L2 + MALL hold


def _time(fn, n_copies, iters):
    """us per call over one window of ``iters`` calls, fn(i) using weight copy i % n_copies."""
    for i in range(n_copies):
        fn(i)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / iters


def _rounds(fns, copies, iters, rounds):
    """{name: [us per round]}, the routes alternating A, B, C, A, B, C ..."""
    out = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            out[k].append(_time(fn, copies, iters))
    return out


def _stats(row, name, ts, nbytes):
    m = statistics.median(ts)
    row.update({f"{name}_us": round(m, 2), f"{name}_min": round(min(ts), 2), f"{name}_max": round(max(ts), 2),
                f"{name}_TBps": round(nbytes / m / 1e6, 3)})


def _weights(N, K, dev, bf16=True, q4=True):
    copies = max(2, -(-CACHE_BYTES // ops.q4_bytes(N, K)))
    copies = min(copies, max(2, int(6 * 2 ** 30 // (2 * N * K))))  # bf16 copies: at most 6 GiB
    wb = [(0.02 * torch.randn(N, K, device=dev)).to(torch.bfloat16) for _ in range(copies)]
    wq = [ops.q4_quantize_pack(w) for w in wb] if q4 else None
    wm = [ops.mx4_quantize_pack(w) for w in wb]
    return copies, (wb if bf16 else None), wq, wm


def bench_kernel(args):
    dev = torch.device("cuda", 0)
    ops.load()
    for name, (N, K) in SHAPES.items():
        if args.shapes and name not in args.shapes:
            continue
        copies, wb, wq, wm = _weights(N, K, dev)
        ops.q4_reserve_scratch(dev, N * K)
        for M in args.rows:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            iters = max(8, min(200, int(2e9 // (N * K * max(M, 16) // 16))))
            t = _rounds({"bf16": lambda i: ops.gemm(x, wb[i % copies]), "int4": lambda i: ops.gemm_q4(x, wq[i % copies]),
                         "mxfp4": lambda i: ops.gemm_mx4(x, wm[i % copies])}, copies, iters, args.rounds)
            row = dict(bench="kernel", shape=name, N=N, K=K, M=M,
                       route="ws-kernel" if M <= ops.MX4_WS_MAX_M else "dequant+gemm")
            _stats(row, "bf16", t["bf16"], 2 * N * K)
            _stats(row, "int4", t["int4"], ops.q4_bytes(N, K))
            _stats(row, "mxfp4", t["mxfp4"], ops.mx4_bytes(N, K))
            if 0 < M <= ops.MX4_WS_KERNEL_MAX_M:  # the other side of the MLOP_MX4_WS_MAX_M crossover
                scr = ops.q4_reserve_scratch(dev, N * K)[: N * K].view(N, K)
                td = _rounds({"d": lambda i: ops.gemm(x, ops.mx4_dequant(wm[i % copies], scr))}, copies, iters, args.rounds)
                _stats(row, "mxfp4_dequant_route", td["d"], ops.mx4_bytes(N, K))
            print(json.dumps(row), flush=True)
        del wb, wq, wm
        torch.cuda.empty_cache()


def bench_rb(args):
    """gemm_mx4_kernel alone at every row-block count the shape allows: the launcher's rule comes from here."""
    dev = torch.device("cuda", 0)
    ops.load()
    for name, (N, K) in SHAPES.items():
        if args.shapes and name not in args.shapes:
            continue
        copies, _, _, wm = _weights(N, K, dev, bf16=False)
        for M in [m for m in args.rows if m <= ops.MX4_WS_KERNEL_MAX_M]:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            iters = max(8, min(200, int(2e9 // (N * K * max(M, 16) // 16))))
            fns = {f"rb{rb}": (lambda i, rb=rb: torch.ops.mlop.gemm_mx4(y, x, wm[i % copies].qw, wm[i % copies].qe, N, rb))
                   for rb in (1, 2, 4) if N % (16 * rb) == 0}
            t = _rounds(fns, copies, iters, args.rounds)
            row = dict(bench="rb", shape=name, N=N, K=K, M=M)
            for k, ts in t.items():
                _stats(row, k, ts, ops.mx4_bytes(N, K))
            print(json.dumps(row), flush=True)
        del wm
        torch.cuda.empty_cache()


def bench_engine(args):
    dev = torch.device("cuda", 0)
    ops.load()
    cfg = get_config("llama3-8b", num_layers=args.layers)
    g = torch.Generator().manual_seed(0)
    for rnd in range(args.rounds):
        for wd in ("bf16", "int4", "mxfp4"):
            model = build_model(cfg, device=dev, seed=0)
            eng = Engine(model, EngineConfig(max_num_seqs=64, max_num_batched_tokens=2048, max_model_len=4096,
                                             num_kv_blocks=2048, graph_buckets=(1, 8, 64), weight_dtype=wd))
            row = dict(bench="engine", round=rnd, weight_dtype=wd, layers=cfg.num_layers,
                       weight_gb=round(model.weight_bytes() / 1e9, 3))
            for batch in (1, 8, 64):
                prompts = [torch.randint(2, 1000, (16,), generator=g).tolist() for _ in range(batch)]
                sp = SamplingParams(max_tokens=args.gen, ignore_eos=True)
                eng.generate(prompts, SamplingParams(max_tokens=8, ignore_eos=True))  # warm-up, graph capture
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                eng.generate(prompts, sp)
                b.record()
                b.synchronize()
                row[f"decode_tok_s_b{batch}"] = round(batch * args.gen / (a.elapsed_time(b) / 1e3), 1)
            prompts = [torch.randint(2, 1000, (2048,), generator=g).tolist() for _ in range(4)]
            eng.generate(prompts[:1], SamplingParams(max_tokens=1, ignore_eos=True))
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            eng.generate(prompts, SamplingParams(max_tokens=1, ignore_eos=True))
            b.record()
            b.synchronize()
            row["prefill_tok_s"] = round(4 * 2048 / (a.elapsed_time(b) / 1e3), 1)
            print(json.dumps(row), flush=True)
            del eng, model
            torch.cuda.empty_cache()


def bench_tile(args):
    dev = torch.device("cuda", 0)
    ops.load()
    for name, (N, K) in SHAPES.items():
        if args.shapes and name not in args.shapes:
            continue
        copies, wb, _, wm = _weights(N, K, dev, q4=False)
        scr = ops.q4_reserve_scratch(dev, N * K)[: N * K].view(N, K)
        for M in args.rows:
            x = torch.randn(M, K, device=dev, dtype=torch.bfloat16)
            y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
            iters = max(8, min(200, int(2e9 // (N * K * max(M, 16) // 16))))

            def tile(ks):
                return lambda i: torch.ops.mlop.gemm_mx4_tile(y, x, wm[i % copies].qw, wm[i % copies].qe, N, 0, ks)

            ks0 = int(torch.ops.mlop.mx4_tile_ks(M, N, K))
            fns = {"bf16": lambda i: ops.gemm(x, wb[i % copies]),
                   "dequant": lambda i: ops.gemm(x, ops.mx4_dequant(wm[i % copies], scr)), "tile": tile(0)}
            if M <= ops.MX4_WS_KERNEL_MAX_M:
                fns["ws"] = lambda i: torch.ops.mlop.gemm_mx4(y, x, wm[i % copies].qw, wm[i % copies].qe, N, 0)
            if name in ("8b-o", "8b-down"):
                fns.update({f"tile_ks{ks}": tile(ks) for ks in args.ks if ks != ks0 and ks <= K // 128})
            t = _rounds(fns, copies, iters, args.rounds)
            row = dict(bench="tile", shape=name, N=N, K=K, M=M, ks=ks0)
            for k, ts in t.items():
                _stats(row, k, ts, 2 * N * K if k == "bf16" else ops.mx4_bytes(N, K))
                row[f"{k}_TFps"] = round(2 * M * N * K / statistics.median(ts) / 1e6, 1)
            print(json.dumps(row), flush=True)
        del wb, wm
        torch.cuda.empty_cache()


def _tile_engine_child(args):
    """One engine in this process (MLOP_MX4_TILE_MAX_M came with the environment): one JSON row."""
    dev = torch.device("cuda", 0)
    ops.load()
    cfg = get_config("llama3-8b", num_layers=args.layers)
    g = torch.Generator().manual_seed(0)
    eng = Engine(build_model(cfg, device=dev, seed=0),
                 EngineConfig(max_num_seqs=256, max_num_batched_tokens=2048, max_model_len=4096, num_kv_blocks=4096,
                              graph_buckets=(64, 256), weight_dtype=args.weights))
    row = dict(bench="tile-engine", weight_dtype=args.weights, tile_max_m=ops.MX4_TILE_MAX_M, layers=cfg.num_layers)

    def timed(prompts, sp):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        eng.generate(prompts, sp)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / 1e3

    for batch in (64, 256):
        prompts = [torch.randint(2, 1000, (16,), generator=g).tolist() for _ in range(batch)]
        eng.generate(prompts, SamplingParams(max_tokens=8, ignore_eos=True))  # warm-up, graph capture
        row[f"decode_tok_s_b{batch}"] = round(batch * args.gen / timed(prompts, SamplingParams(max_tokens=args.gen, ignore_eos=True)), 1)
    prompts = [torch.randint(2, 1000, (2048,), generator=g).tolist() for _ in range(4)]
    eng.generate(prompts[:1], SamplingParams(max_tokens=1, ignore_eos=True))
    row["prefill_tok_s"] = round(4 * 2048 / timed(prompts, SamplingParams(max_tokens=1, ignore_eos=True)), 1)
    print(json.dumps(row), flush=True)


def bench_tile_engine(args):
    if args.child:
        return _tile_engine_child(args)
    base = [sys.executable, __file__, "tile-engine", "--child", "--layers", str(args.layers), "--gen", str(args.gen)]
    for _ in range(args.rounds):
        for wd, knob in (("bf16", "0"), ("mxfp4", "0"), ("mxfp4", str(args.tile_max_m))):
            subprocess.run(base + ["--weights", wd], env=dict(os.environ, MLOP_MX4_TILE_MAX_M=knob), check=True, timeout=900)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["kernel", "rb", "engine", "tile", "tile-engine"])
    ap.add_argument("--rows", type=int, nargs="*", default=[1, 4, 8, 16, 32, 64, 128, 512, 2048])
    ap.add_argument("--shapes", nargs="*", default=[])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--layers", type=int, default=32)
    ap.add_argument("--gen", type=int, default=128)
    ap.add_argument("--ks", type=int, nargs="*", default=[1, 2, 4, 8], help="tile: forced K splits on o and down")
    ap.add_argument("--tile-max-m", type=int, default=1024, help="tile-engine: the knob value set against 0")
    ap.add_argument("--weights", default="mxfp4", help="tile-engine child: weight_dtype")
    ap.add_argument("--child", action="store_true", help="tile-engine: run one engine in this process")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mx4 measures on a GPU"
    {"kernel": bench_kernel, "rb": bench_rb, "engine": bench_engine, "tile": bench_tile,
     "tile-engine": bench_tile_engine}[args.what](args)


if __name__ == "__main__":
    main()
